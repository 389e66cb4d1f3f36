/*
 * forma_rt.h — C ABI of the MI355X-native path tracer that drops in for
 * fo-rma's CPU ray tracer (zehreken/fo-rma, src/cpu_ray_tracer + src/shapes).
 *
 * Everything here is plain C: POD structs with explicit layout, opaque handles,
 * integer error codes. No torch or HIP types appear in any signature (a HIP
 * stream is passed as `void*`). A `#[repr(C)]` Rust mirror of this header is in
 * INTEGRATION.md.
 *
 * Which reference interface each entry point replaces (paths relative to the
 * reference root):
 *
 *   fr_prim / fr_scene_create ........ shapes/hitable.rs:4-14 (trait Hitable), the
 *                                      Sphere/Plane/AABB/Rectangle constructors
 *                                      (shapes/sphere.rs:75-83, plane.rs:48-66,
 *                                      aabb.rs:36-44, rectangle.rs:36-44) and
 *                                      cpu_ray_tracer/scene.rs:4-15 (Scene.objects)
 *   fr_scene_builtin ................. cpu_ray_tracer/scenes.rs:6,41,110
 *                                      (get_simple_scene / get_plane_scene / get_objects)
 *   fr_scene_from_json ............... basics/scene_loader.rs:3-7 (construct_scene_from_json)
 *                                      + basics/scene.rs:55-99 (mesh/material dispatch),
 *                                      mapped to tracer primitives
 *   fr_scene_translate / _rotate ..... shapes/hitable.rs:12-13, shapes/plane.rs:62-68
 *   fr_camera_init ................... cpu_ray_tracer/camera.rs:24-60 (Camera::new)
 *   fr_camera_look ................... camera.rs:24-60 generalised to a JSON camera
 *   fr_camera_orbit .................. camera.rs:97-122 (Camera::orbit)
 *   fr_camera_translate .............. camera.rs:74-95 (Camera::translate)
 *   fr_update_delta .................. cpu_ray_tracer/tracer.rs:30-52 (update's key bitmask)
 *   fr_ctx_render / fr_render_hip .... cpu_ray_tracer/tracer.rs:160-219 (save_image +
 *                                      get_color) and tracer.rs:57-81 (render, 1 spp)
 *   fr_mctx_* / fr_render_hip_multi .. tracer.rs:83-134 (render_mt row tiling), one
 *                                      device per row shard instead of one thread;
 *                                      fr_mctx keeps the per-device contexts and a
 *                                      page-locked frame across renders (update loop)
 *
 * Errors: 0 = ok, negative = FR_E*; the message is in fr_last_error() (thread-local).
 * Threading: calls on distinct fr_scene / fr_ctx objects are re-entrant. A fr_ctx is
 * bound to one device and one HIP stream and must not be used by two threads at once.
 */
#ifndef FORMA_RT_H
#define FORMA_RT_H

#if !defined(__HIPCC_RTC__) /* hiprtc (the scene-specialised build) provides these types */
#include <stddef.h>
#endif
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FR_ABI_VERSION 6 /* 2: fr_stats.trace_launches; FR_TRIANGLE; post effects; FR_FLAG_MT_BANDS
                            3: fr_stats.scatters/.occupancy; fr_ctx_download_async, fr_ctx_wait,
                               fr_host_alloc/free; item-major sample buffer
                            4: fr_mctx_* (persistent multi-device context); fr_ctx_trace_log(_read);
                               entry points restore the caller's current HIP device
                            5: FR_FLAG_SCENE_JIT, fr_ctx_prepare, fr_ctx_jit_info
                            6: FR_FLAG_SCENE_JIT compiles in the background (renders never wait),
                               FR_FLAG_SCENE_JIT_WAIT, fr_ctx_jit_state, fr_jit_wait
                               (still 6, additive: FR_FLAG_ACCUMULATE, fr_ctx_accum_reset / _info,
                               fr_mctx_accum_reset / _info; FR_FLAG_ACCUM_ERROR,
                               fr_ctx_accum_error, fr_ctx_download_error, fr_mctx_accum_error;
                               FR_FLAG_ADAPTIVE, fr_adapt_info, fr_ctx_adapt, fr_ctx_download_counts,
                               fr_mctx_adapt; fr_ctx_denoise, fr_ctx_download_denoised,
                               fr_ctx_denoised_buffers; fr_ctx_gbuffer, fr_ctx_download_gbuffer,
                               fr_denoise_guide, fr_ctx_denoise_guided; fr_camera_axial,
                               fr_ctx_camera_path, fr_selftest_camray, fr_selftest_boxinv; fr_temporal,
                               fr_ctx_temporal, fr_ctx_temporal_reset, fr_ctx_download_temporal) */
/* (still 6, additive too: fr_ray, fr_cast_info, fr_camera_pixel_ray, fr_ctx_cast, fr_ctx_download_hits,
   fr_ctx_cast_info, fr_ctx_gbuffer_info; fr_ctx_trace_log_read which = 5) */
/* (still 6, additive too: FR_CAST_TMAX, FR_CAST_OUT_DEVICE, fr_occl_info, fr_ctx_occluded,
   fr_ctx_download_occluded, fr_ctx_occluded_info, fr_ctx_hit_buffers) */
/* (still 6, additive too: FR_UPDATE_REBUILD, FR_SCENE_SYNC_*, FR_TABLE_*, fr_scene_info, fr_scene_update,
   fr_scene_rebuild, fr_ctx_scene_info, fr_scene_download_table) */

/* error codes */
#define FR_OK 0
#define FR_EARG (-1)   /* invalid argument */
#define FR_EPARSE (-2) /* JSON syntax error or unsupported mesh */
#define FR_EHIP (-3)   /* a HIP runtime call failed */
#define FR_ENODEV (-4) /* no HIP device / requested device missing */
#define FR_ENOMEM (-5) /* allocation failed */

/* primitive kinds (one Hitable implementation each) */
#define FR_SPHERE 0u /* shapes/sphere.rs */
#define FR_PLANE 1u  /* shapes/plane.rs (bounded, world-axis extent) */
#define FR_AABB 2u   /* build-defined axis-aligned box (JSON "cube" with a signed-permutation rotation) */
#define FR_OBB 3u    /* build-defined oriented box (JSON "cube", any other rotation) */
#define FR_STUB 4u   /* shapes/aabb.rs / rectangle.rs: hit() and scatter() always false */
#define FR_TRIANGLE 5u /* build-defined triangle: JSON triangle/circle/cylinder/tetrahedron meshes, tilted quads */

/* material ids as the reference stores them (u8 `material` field) */
#define FR_LAMBERTIAN 0u /* sphere.rs:84-89, plane.rs:101-106 */
#define FR_METAL 1u      /* sphere.rs:91-105, plane.rs:108-122 */
#define FR_DIELECTRIC 2u /* sphere.rs:107-145 (spheres and boxes only) */
#define FR_LIGHT 3u      /* sphere.rs:147-152 (no emission: attenuation 1) */

/* flags for fr_params.flags */
#define FR_FLAG_WRITE_U8 1u /* also write the u8 image (tracer.rs:177-184) */
/* save_image_mt (tracer.rs:83-158): 4 row bands of H/4 rows, v = ((H/4 - y_band) + r)/H
   + band * 0.25, each sample gamma-corrected and quantised to u8, the u8 values averaged
   as acc += u8 / spp in f32 and truncated; rows past 4 * (H/4) stay 0. mean_rgb then
   holds acc (0..255). Render the plain simple scene (fr_scene_builtin 0) with
   max_depth 50 to match the reference call. */
#define FR_FLAG_MT_BANDS 2u
/* Scene-specialised trace kernel (render.hip / jit.cpp): for list-loop scenes of at most 64
   primitives, the kernel compiled once per scene with the primitive records as constants
   (hiprtc; one code object per GPU architecture, cached per process and on disk,
   FR_JIT_CACHE). Same image bits as without the flag; shared slab planes are computed once
   per segment. A render never waits for the compile: when no code object exists yet it is
   queued on a background host thread and the render runs the compiled-in kernel
   (fr_ctx_jit_state says FR_JIT_PENDING); a later render picks the scene kernel up.
   fr_ctx_prepare, FR_FLAG_SCENE_JIT_WAIT, and FR_SCENE_JIT=1 in the environment wait for it
   instead (FR_SCENE_JIT=0 turns it off for every render). */
#define FR_FLAG_SCENE_JIT 4u
#define FR_FLAG_SCENE_JIT_WAIT 8u /* with FR_FLAG_SCENE_JIT: compile on the render's thread if needed */
/* with FR_FLAG_SCENE_JIT (not _WAIT): use the scene kernel only if its code object is in this
   process or the disk cache; never compile or queue a compile (FR_JIT_MISS otherwise). For
   one-shot callers: a queued background compile runs to its end when the process exits, so
   a process that renders once and exits would otherwise wait for hiprtc at exit. */
#define FR_FLAG_SCENE_JIT_CACHED 16u
/* Progressive accumulation: the frame is traced exactly like the plain frame (same kernels,
   records and counters), but its per-pixel sum S (its spp samples added in sample order from
   zero) is added to the context's accumulator A (3 f32 per pixel of the shard) and the
   outputs show the running mean: A = S when the frame starts an accumulation, else A = A + S
   (one f32 add per channel); n += spp; mean = A / (float)n; u8 from that mean. The first frame
   of an accumulation is bit-identical to the plain render. A frame continues the context's
   accumulation iff the scene (as uploaded: any edit counts), the 104 bytes of the camera,
   width, height, max_depth, shard_index and shard_count equal the previous accumulating
   frame's; otherwise, and after fr_ctx_accum_reset, it starts a new one. seed and spp may
   differ from frame to frame (give every frame its own seed). Plain renders on the same
   context in between neither read nor disturb A and n. A is plain f32 without compensation:
   it stops improving in the region of 2^24 samples per pixel (so does Q of
   FR_FLAG_ACCUM_ERROR, whose estimate moreover cannot resolve a relative error under about
   2^-12 sqrt(K) after K frames: see there); a frame that would take n past 2^32 - 1 is FR_EARG. FR_EARG with FR_FLAG_MT_BANDS (save_image_mt has its own averaging)
   and through fr_render_hip / fr_render_hip_multi (their context dies with the call). */
#define FR_FLAG_ACCUMULATE 32u
/* With FR_FLAG_ACCUMULATE only: the accumulation also carries a second-moment accumulator Q
   (3 f32 per pixel of the shard, indexed, kept and grown like A), from which
   fr_ctx_accum_error estimates each pixel's remaining noise. After A is updated the frame does,
   per channel and in f32 with every operation rounded once and nothing fused,
   q = (S * S) / (float)spp, then Q = q when the frame starts an accumulation, else Q = Q + q.
   The mean and the u8 image are exactly those of the frame without this flag. The bit is part
   of what a frame must share with the previous accumulating frame to continue its accumulation
   (see FR_FLAG_ACCUMULATE): a frame whose bit differs starts a new one, so Q never misses a
   frame of the accumulation it describes. FR_EARG without FR_FLAG_ACCUMULATE and with spp 0.

   The estimate, for a pixel with n samples in K >= 2 frames, fn = (float)n, fk = (float)(K - 1),
   per channel c, every operation rounded once in f32:
     m_c = A_c / fn
     v_c = max((Q_c - A_c * m_c) / fk, 0)          a NaN reads 0
     err = sqrt(((v_r + v_g) + v_b) / fn)          standard error of the summed channels' mean
     den = max((m_r + m_g) + m_b, FR_ERR_FLOOR)    a NaN reads FR_ERR_FLOOR
     rel = err / den, or 0 where (m_r + m_g) + m_b is NaN or infinite: such a pixel does not
           change with more frames, so there is nothing to wait for
   S_k has mean spp_k mu and variance spp_k sigma^2, so (sum_k S_k^2 / spp_k - A^2 / n) / (K - 1)
   is an unbiased estimate of the per-sample variance sigma^2 for frames of any spp, and v_c / n
   is the variance of the mean. rel is never NaN and never negative. Q - A^2 / n in f32 loses
   everything below about K 2^-24 of m^2: a pixel whose true relative error is under about
   2^-12 sqrt(K) reads as 0 or as noise of that size, far under one u8 step. */
#define FR_FLAG_ACCUM_ERROR 64u
#define FR_ERR_FLOOR 0.0078125f /* 2^-7 */
/* Adaptive sampling, with FR_FLAG_ACCUMULATE | FR_FLAG_ACCUM_ERROR only (FR_EARG without either):
   the frame traces and resolves only the 8x8 tiles of the context's active tile list, which
   fr_ctx_adapt builds from the error estimate. The granularity is the tile of a shard in the
   trace kernel's own order (tile = pixel slot >> 6: tiles left to right within an 8-row strip,
   the shard's strips top to bottom). For the pixels of the list's tiles the frame does what the
   accumulating frame does, with the tile's own counts: A += S, Q += S^2 / spp, n_t += spp,
   K_t += 1, mean = A / (float)n_t, u8 from that mean, in FR_FLAG_ACCUMULATE's and
   FR_FLAG_ACCUM_ERROR's operation order; S is bit for bit what the plain frame of the same
   parameters and seed sums for that pixel (a pixel's random streams depend on the seed, its
   index in the image and the sample block alone). A, Q, the counts and the output buffers of
   every other pixel are left exactly as they are: a plain render on the same context in
   between leaves its own values in the inactive tiles of the outputs, where they stay.
   FR_EARG, before anything is enqueued, when the frame would start a new accumulation and when
   the live accumulation is not tiled (no fr_ctx_adapt since it started). An empty list is not
   an error: nothing is traced, outputs and state are untouched and the accumulation's frames
   and samples do not move. fr_stats.samples = (image pixels in the list's tiles) x spp;
   segments, hits and prim_tests count what was traced. A frame without this flag in a tiled
   accumulation is the adaptive frame whose list is every tile; the two kinds mix freely (the
   flag is not part of what a frame must share to continue an accumulation). FR_EARG through
   fr_render_hip / fr_render_hip_multi, as FR_FLAG_ACCUMULATE. fr_ctx_prepare with the flag
   allocates (for the whole shard) and changes no state. */
#define FR_FLAG_ADAPTIVE 128u
/* fr_ctx_jit_state: which trace kernel the last render (or fr_ctx_prepare) ran */
#define FR_JIT_OFF 0     /* compiled-in kernel: not asked for, a BVH scene, or > 64 primitives */
#define FR_JIT_USED 1    /* the scene-specialised kernel */
#define FR_JIT_PENDING 2 /* asked for, compile still running: the compiled-in kernel ran */
#define FR_JIT_FAILED 3  /* asked for, compile failed: the compiled-in kernel ran */
#define FR_JIT_MISS 4    /* asked for cached only (FR_FLAG_SCENE_JIT_CACHED), none cached: compiled-in kernel */

/*
 * One primitive, in the order it is tested (list order decides ties, tracer.rs:195-200).
 * Geometry `g` by kind:
 *   FR_SPHERE : g[0..2] center, g[3] radius
 *   FR_PLANE  : g[0..2] position, g[3..5] orientation, g[6..8] size (half extents per world axis)
 *   FR_AABB   : g[0..2] min corner, g[3..5] max corner
 *   FR_OBB    : g[0..2] center, g[3..5] local x axis, g[6..8] local y axis, g[9..11] local z axis
 *               (unit rows of the world->local rotation), g[12..14] half extents
 *   FR_STUB   : unused
 *   FR_TRIANGLE: g[0..2], g[3..5], g[6..8] the world vertices v0, v1, v2 (winding v0 -> v1 -> v2)
 * `material` is the raw reference id; unknown ids fall back as sphere.rs:68 / plane.rs:55 do.
 */
typedef struct fr_prim {
  uint32_t kind;
  uint32_t material;
  float color[3];
  float fuzz;
  float g[16];
} fr_prim;

/* Mirrors the fields of cpu_ray_tracer::camera::Camera (camera.rs:8-21), f32 throughout. */
typedef struct fr_camera {
  float position[3];
  float lower_left[3];
  float horizontal[3];
  float vertical[3];
  float u[3];
  float v[3];
  float w[3];
  float aspect;
  float lens_radius;
  float focus_dist; /* stored 2.0 by Camera::new, never used (camera.rs:56) */
  float radius;     /* orbit radius, 5.0 (camera.rs:57) */
  float rotation;   /* orbit angle, 0.0 (camera.rs:58) */
} fr_camera;

/*
 * Render parameters. Rows are grouped into strips of `strip_rows` (must be 8) rows;
 * strip k belongs to shard (k % shard_count). A shard renders only its own strips,
 * so shards of one image are disjoint and stitch bit-exactly.
 * RNG: one stream per (seed, global pixel index y*W+x, block of 16 samples); a block's
 * samples draw from it in order.
 */
typedef struct fr_params {
  uint32_t width, height;
  uint32_t spp;       /* samples per pixel (save_image's `sample`) */
  uint32_t max_depth; /* tracer.rs:10 MAX_DEPTH (reference default 50); 1..64 */
  uint64_t seed;
  uint32_t strip_rows;  /* must be 8 */
  uint32_t shard_index; /* 0 <= shard_index < shard_count */
  uint32_t shard_count; /* >= 1 */
  uint32_t flags;       /* FR_FLAG_* */
} fr_params;

typedef struct fr_stats {
  uint64_t segments;   /* get_color calls (ray segments traced) */
  uint64_t hits;       /* segments whose closest-hit loop found an object */
  uint64_t samples;    /* paths started = pixels * spp */
  uint64_t prim_tests; /* segments * n_prims */
  double kernel_ms;    /* HIP-event time of the whole render on its stream (all kernels) */
  double total_ms;     /* host wall time of the call */
  double trace_ms;     /* HIP-event time of the trace kernel(s) alone, summed over launches */
  uint32_t trace_launches; /* trace kernel launches of the render (sample-block passes) */
  uint32_t occupancy;  /* resident trace-kernel workgroups per CU (the persistent grid's size / CUs) */
  uint64_t scatters;   /* successful scatters (tracer.rs:205: a segment continued by a new ray) */
} fr_stats;

typedef struct fr_scene fr_scene; /* opaque: host primitive list + per-device copies */
typedef struct fr_ctx fr_ctx;     /* opaque: one device, one stream, output buffers */
typedef struct fr_mctx fr_mctx;   /* opaque: one fr_ctx per device entry + a page-locked host frame */

/* ---- library ---- */
const char* fr_last_error(void);
int fr_abi_version(void);
int fr_device_count(int* count);

/* ---- scenes (host) ---- */
int fr_scene_create(const fr_prim* prims, uint32_t n, fr_scene** out);
int fr_scene_builtin(int which, uint32_t width, uint32_t height, fr_scene** out, fr_camera* cam_out);
int fr_scene_from_json(const char* json_text, size_t len, uint32_t width, uint32_t height,
                       fr_scene** out, fr_camera* cam_out);
void fr_scene_free(fr_scene* scene);
uint32_t fr_scene_count(const fr_scene* scene);
int fr_scene_get_prims(const fr_scene* scene, fr_prim* out, uint32_t n);
int fr_scene_translate(fr_scene* scene, uint32_t index, const float v[3]);
int fr_scene_rotate(fr_scene* scene, uint32_t index, const float v[3]);

/* Moving scenes. fr_scene_update replaces the n listed primitives of the host
   list (index NULL: primitives 0..n-1; duplicates allowed, the last one wins). Every index is
   checked first: one out of range, or an unknown kind, is FR_EARG and nothing moves. n = 0 is a
   no-op. The edit is geometric when every listed primitive keeps the kind, material, colour and
   fuzz of the one it replaces, bit for bit, and stays boundable or not (finite box, sphere,
   oriented box or triangle: boundable; plane, stub, non-finite geometry: not). A geometric edit
   keeps the scene's device copies: each patches the edited primitives' records in place and refits
   its tree's boxes on the device, inside the first render, cast, G-buffer or occlusion call after
   the edit (when a moved primitive leaves the extent the tree was padded for, that copy is packed
   and built again instead: fr_ctx_scene_info says which happened). Any other edit, and any call
   with FR_UPDATE_REBUILD, takes the path of fr_scene_translate: pack, build, upload. Either way
   the scene counts as edited: an accumulation restarts, a G-buffer of the old scene is refused.
   fr_scene_rebuild asks for that full path at the next use (a refitted tree keeps its topology
   and walks slower the further the primitives have moved).
   Ordering: work enqueued before the catch-up, on any stream of any context of that device, reads
   the old scene (the catch-up starts with a device-wide wait); work enqueued after it reads the
   new one, on whichever context: a context that finds the copy already caught up has its streams
   wait for the patch. Calls that use one scene from several threads must not overlap an update. */
#define FR_UPDATE_REBUILD 1u
#define FR_SCENE_SYNC_NONE 0u  /* the copy was current */
#define FR_SCENE_SYNC_PACK 1u  /* packed, built and uploaded */
#define FR_SCENE_SYNC_REFIT 2u /* patched in place, tree refitted */
typedef struct fr_scene_info {
  uint32_t last_sync;      /* FR_SCENE_SYNC_*: what this context's last call that used the scene did to the copy */
  uint32_t prims_patched;  /* _REFIT: primitives rewritten */
  uint32_t nodes_refit;    /* _REFIT: tree nodes recomputed (0: the copy has no tree) */
  uint32_t refit_launches; /* _REFIT: refit kernel launches (one per tree height) */
  uint64_t packs, refits;  /* the copy's running counts */
  uint64_t version, edit_seq; /* the host list's */
  float host_ms;           /* _REFIT: host preparation of the rows */
  float h2d_ms, patch_ms, refit_ms; /* _REFIT: its copy, patch kernel and refit launches by device events; -1 while pending */
  uint32_t has_tree, n_nodes;
} fr_scene_info;
int fr_scene_update(fr_scene* scene, const uint32_t* index /* NULL: 0..n-1 */, const fr_prim* prims, uint32_t n, uint32_t flags);
int fr_scene_rebuild(fr_scene* scene);
/* Diagnostics: one table of the scene's copy on `device`, as it stands, after a device-wide wait.
   out NULL: *bytes receives the size only. FR_EARG when the scene has no copy there or cap is short. */
#define FR_TABLE_RECORDS 0u      /* 64 B per primitive, list order */
#define FR_TABLE_LEAF_RECORDS 1u /* 64 B per leaf slot */
#define FR_TABLE_LEAF_ORDER 2u   /* uint32 per leaf slot: the list index */
#define FR_TABLE_NODES 3u        /* 64 B per tree node */
#define FR_TABLE_SLOT_BOUNDS 4u  /* 32 B per leaf slot: lo xyz, 0, hi xyz, 0 */
#define FR_TABLE_NODE_UNIONS 5u  /* 32 B per tree node, unpadded */
int fr_scene_download_table(fr_scene* scene, int device, uint32_t which, void* out, size_t cap, size_t* bytes);
/* What this context's last call that used `scene` did to the scene's copy on the context's device
   (a second context that finds the copy caught up reads FR_SCENE_SYNC_NONE), and that copy's counts.
   Nothing is waited for. */
int fr_ctx_scene_info(fr_ctx* ctx, fr_scene* scene, fr_scene_info* out);

/* ---- camera (host; tan/cos/sin are host-only) ---- */
int fr_camera_init(fr_camera* cam, uint32_t width, uint32_t height);
int fr_camera_look(fr_camera* cam, const float from[3], const float at[3], const float vup[3],
                   float vfov_deg, float aperture, uint32_t width, uint32_t height);
int fr_camera_orbit(fr_camera* cam, const float delta[3]);
int fr_camera_translate(fr_camera* cam, const float delta[3]);
int fr_update_delta(uint8_t keys, float delta_time, float delta_out[3]);

/* ---- GPU render context ---- */
int fr_ctx_create(int device, void* hip_stream /* NULL = own stream */, fr_ctx** out);
void fr_ctx_free(fr_ctx* ctx);
/* Enqueue one render of the shard described by params (async on the ctx stream).
   The scene is uploaded to the ctx device on first use and stays resident. */
int fr_ctx_render(fr_ctx* ctx, fr_scene* scene, const fr_camera* cam, const fr_params* params);
/* Wait for the last render; fill counters and kernel time. */
int fr_ctx_sync(fr_ctx* ctx, fr_stats* stats);
/* Copy the shard's rows of the last render into full-image host buffers
   (mean_rgb: W*H*3 f32, rgb8: W*H*3 u8; either may be NULL). Rows of other shards
   are left untouched. */
int fr_ctx_download(fr_ctx* ctx, float* mean_rgb, uint8_t* rgb8);
/* The same copies enqueued on the ctx's copy stream, after the last render; returns at
   once. The host buffers must stay valid until fr_ctx_wait (pinned memory from
   fr_host_alloc makes the copy asynchronous). The next fr_ctx_render's trace kernel does
   not wait for these copies; only its writes of the output buffers do, so one frame's
   gather overlaps the next frame's trace. */
int fr_ctx_download_async(fr_ctx* ctx, float* mean_rgb, uint8_t* rgb8);
/* Block until every render and download enqueued on the ctx has completed. */
int fr_ctx_wait(fr_ctx* ctx);
/* Device pointers of the last render's full-image output buffers. */
int fr_ctx_device_buffers(fr_ctx* ctx, float** d_mean_rgb, uint8_t** d_rgb8);
/* Launch log: enable != 0 starts a new log (previous entries dropped); every later render
   records HIP events around each trace-kernel launch (on the launch's stream) and around
   the whole render (trace + sum kernels). _read waits for the logged work and writes up
   to cap durations (ms) in order: which = 0 the trace launches, 1 the renders; which = 2
   / 3 the same entries as (start, end) pairs in ms from the first logged trace launch's
   start (2 values per entry, a timeline); which = 4 the stages of every fr_ctx_temporal call,
   three entries per call in order: the prior (reprojection and the copy of the view's G-buffer
   words, or the fills of an empty prior; nothing when the prior is kept), totals and prep, the
   picture (the levels, or the finalise kernel); which = 5 every cast kernel (fr_ctx_cast),
   occlusion kernel (fr_ctx_occluded) and G-buffer pass (fr_ctx_gbuffer) enqueued while the log is
   on; *n = the entries logged. Lets a caller streaming K frames average all K of them and see the gaps between them. */
int fr_ctx_trace_log(fr_ctx* ctx, int enable);
int fr_ctx_trace_log_read(fr_ctx* ctx, int which, double* ms, uint32_t cap, uint32_t* n);
/* Everything a render of these parameters sets up before its first launch, without
   rendering: the scene's device copy, the output and sample buffers and, with
   FR_FLAG_SCENE_JIT, the scene-specialised kernel (compiled or loaded here, so the first
   timed frame does not pay for it). fr_ctx_jit_info then describes that kernel. */
int fr_ctx_prepare(fr_ctx* ctx, fr_scene* scene, const fr_camera* cam, const fr_params* params);
/* The last render's trace kernel: *used = 1 when it ran the scene-specialised kernel
   (FR_FLAG_SCENE_JIT), *ms = the time that render spent getting it (hiprtc compile, disk
   cache load or 0 when already loaded), *compiled = 1 when hiprtc ran. Any may be NULL. */
int fr_ctx_jit_info(fr_ctx* ctx, int* used, double* ms, int* compiled);
/* *state = FR_JIT_* of the last render. For FR_JIT_FAILED, fr_last_error() then holds the
   compiler's message. */
int fr_ctx_jit_state(fr_ctx* ctx, int* state);
/* Block until no scene-kernel compile is queued or running in this process. */
int fr_jit_wait(void);
/* Camera ray form. A camera whose u, v, horizontal and vertical each lie along one axis (every
   camera fr_camera_init / fr_camera_look builds for an unrotated view) and that passes the
   zero-sign conditions of DESIGN.md 4.2 has its rays generated by a shorter sequence that
   gives the same bits. fr_camera_axial: 1 when cam is of that class, 0 when not (host only, no
   device; FR_EARG for NULL). fr_ctx_camera_path: *axial = 1 when the last render (or
   fr_ctx_prepare) took the short form; 0 for any other camera, and for every camera while
   the environment has FR_CAM_GENERAL=1. */
int fr_camera_axial(const fr_camera* cam);
int fr_ctx_camera_path(fr_ctx* ctx, int* axial);
/* Diagnostic: both ray forms on the device for n lens/jitter tuples in[4 i] = (kx, ky, s, t),
   kx, ky the lens point's integers (2^23-scaled); out[12 i] = the general form's o.xyz, d.xyz,
   then the short form's, as bit patterns. FR_EARG when cam is not of the axial class. */
int fr_selftest_camray(int device, const fr_camera* cam, const float* in, uint32_t n, uint32_t* out);
/* Diagnostic: the trace kernel's segment set-up on the device for n directions in[3 i] = d.xyz;
   out[3 i] = the bit patterns of the three box reciprocals, RN(1 / d) clamped to +-2^100. */
int fr_selftest_boxinv(int device, const float* in, uint32_t n, uint32_t* out);
/* FR_FLAG_ACCUMULATE: the next accumulating frame starts a new accumulation. */
int fr_ctx_accum_reset(fr_ctx* ctx);
/* Frames and samples per pixel in the accumulator (0, 0 when there is none). Host-side, as of
   the last enqueued frame; no sync. Either may be NULL. */
int fr_ctx_accum_info(fr_ctx* ctx, uint32_t* frames, uint32_t* samples);
/* The error estimate of the live accumulation (FR_FLAG_ACCUM_ERROR) and its summary. */
typedef struct fr_accum_error { /* 32 bytes */
  uint32_t frames, samples;     /* K and n the estimate was taken at */
  uint64_t pixels;              /* pixels of the shard(s) */
  uint64_t converged;           /* of them, rel <= threshold */
  float max_rel, threshold;     /* the largest rel of those pixels; the threshold asked for */
} fr_accum_error;
/* Computes rel (FR_FLAG_ACCUM_ERROR) for every pixel of this context's shard as of the last
   enqueued accumulating frame, into a W x H f32 map on the device, and its summary: two small
   kernels behind every enqueued frame's resolve, then a wait for them alone. The pending
   render, its stats, A and Q are left as they are, so it may be called between streamed
   frames. Integer counts and a maximum over bit patterns: the same accumulation gives the
   same summary bit for bit. FR_EARG when the context has no live accumulation, when the live
   one carries no Q, when it has fewer than two frames, and for a NaN or negative threshold
   (+infinity is allowed and counts every pixel). */
int fr_ctx_accum_error(fr_ctx* ctx, float threshold, fr_accum_error* out);
/* Copies the map of the last fr_ctx_accum_error into rel (W x H f32, row-major): this shard's
   rows only, the others are left untouched. */
int fr_ctx_download_error(fr_ctx* ctx, float* rel);
/* Adaptive sampling (FR_FLAG_ADAPTIVE): the selection's summary. */
typedef struct fr_adapt_info {  /* 56 bytes */
  uint32_t frames, samples;     /* frames enqueued in the accumulation; sum of their spp (the largest per-tile n possible) */
  uint32_t tiles, active_tiles; /* tiles of the shard(s) with at least one pixel in the image; of them, in the list */
  uint64_t pixels, active_pixels; /* image pixels of the shard(s); of them, in active tiles */
  uint64_t converged;           /* pixels with rel <= threshold (as fr_accum_error.converged) */
  float max_rel, threshold;
  uint32_t min_samples, pad;    /* pad = 0 */
} fr_adapt_info;
/* Computes rel for every pixel of the shard as fr_ctx_accum_error does, with the pixel's tile's
   own n_t and K_t for n and K, into the map fr_ctx_download_error reads, and builds the
   context's active tile list, in ascending tile order: a tile is active iff the maximum of rel
   over its image pixels is > threshold (compared as uint32 bits) or its n_t < min_samples. The
   same conditions and FR_EARGs as fr_ctx_accum_error; like it, it runs behind every enqueued
   frame's resolve and waits for that alone. The first successful call makes the live
   accumulation tiled: n_t and K_t start from its uniform (n, K) and every later frame's
   resolve maintains them; they and the list die with the accumulation (fr_ctx_accum_reset, or
   a frame that starts a new one), and a new accumulation is uniform until the next call. For a
   given accumulation the result is the same bits every time, so a tile that was inactive stays
   inactive under the same threshold. On a tiled accumulation fr_ctx_accum_error uses n_t and
   K_t too; its frames and samples, and fr_ctx_accum_info's, are the totals given here. */
int fr_ctx_adapt(fr_ctx* ctx, float threshold, uint32_t min_samples, fr_adapt_info* out);
/* The per-pixel sample and frame counts of the live accumulation (each pixel's tile's n_t and
   K_t; the uniform n and K while it is not tiled): W x H uint32 each, either may be NULL; this
   shard's rows only. Waits for the enqueued resolves. FR_EARG without a live accumulation. */
int fr_ctx_download_counts(fr_ctx* ctx, uint32_t* samples, uint32_t* frames);

/* Variance-guided denoise of the live accumulation: an a-trous wavelet filter (SVGF's spatial
   part) of the mean A / n, steered by the per-pixel variance of the mean that A, Q and the counts
   give (each pixel's tile's n_t and K_t on a tiled accumulation). Prep: per channel m = A / n and
   v as fr_ctx_accum_error's, C = (m_r, m_g, m_b), var = ((v_r + v_g) + v_b) / n; a pixel is valid
   iff |m_c| <= FR_DN_MEAN_MAX in every channel and var <= FR_DN_VAR_MAX (a NaN or infinite pixel
   is not). Level i = 0 .. levels-1 with step s = 1 << i: an invalid pixel keeps its bits; a valid
   pixel p gets g = the (1 2 1) x (1 2 1) weighted mean of var over its valid 3x3 neighbours,
   sden = k g + FR_DN_EPS, and over the 5x5 taps q = p + s (dx, dy) that are inside the image and
   valid, dy outer and dx inner, w = (h[dy] h[dx]) sden / (sden + |C_q - C_p|^2) with
   h = (1/16, 1/4, 3/8, 1/4, 1/16): C' = sum(w C_q) / sum(w), var' = sum(w^2 var_q) / sum(w)^2.
   Every operation rounds once in f32 in a fixed order (fo-rma_amd/csrc/denoise.h), so the
   result is the same bits every time. rgb8 = to_u8 of the filtered mean, as a frame's.
   The variance that comes out is what the filter steered by, not an error estimate of the
   filtered picture: the filter trades variance for bias, and on reference frames the map read
   23 to 46 times under the real squared error.
   Out of scope: shards. The 8-row strips of different shards live on different devices and a tap
   reaches up to 2 * 2^(levels-1) rows away; the data path has no exchange step, so only a whole
   image (shard_count 1) is filtered and there is no fr_mctx_denoise. */
#define FR_DN_EPS 9.5367431640625e-07f /* 2^-20 */
#define FR_DN_MEAN_MAX 1099511627776.0f /* 2^40 */
#define FR_DN_VAR_MAX 1208925819614629174706176.0f /* 2^80 */
#define FR_DN_LEVELS_DEFAULT 4u
#define FR_DN_K_DEFAULT 4.0f
/* Enqueue the filter on the live accumulation; returns at once. levels 1..6, k finite in (0, 1024].
   It runs behind the resolve of every frame enqueued so far and reads A, Q and the counts only:
   the outputs of the frames, the pending render and its stats are untouched, and the result
   describes the accumulation as of the call (later frames do not update it).
   FR_EARG: no live accumulation, no Q, fewer than two frames (the conditions of fr_ctx_accum_error),
   shard_count != 1, levels or k out of range. */
int fr_ctx_denoise(fr_ctx* ctx, uint32_t levels, float k);
/* Waits for the last fr_ctx_denoise; any pointer may be NULL. FR_EARG if none was enqueued since
   the buffers were (re)allocated. mean_rgb W*H*3 f32, rgb8 W*H*3 u8, var W*H f32. */
int fr_ctx_download_denoised(fr_ctx* ctx, float* mean_rgb, uint8_t* rgb8, float* var);
/* Device pointers of the denoised mean and u8 (for fr_rgb_to_rgba_device / fr_post_process_device). */
int fr_ctx_denoised_buffers(fr_ctx* ctx, float** d_mean_rgb, uint8_t** d_rgb8);

/* First-hit feature buffers of a view (AOV output, and what fr_ctx_denoise_guided steers by): per
   pixel (x, y) of the W x H image the pinhole primary ray
     u = ((float)x + 0.5) / (float)W, v = ((float)(H - y) + 0.5) / (float)H,
     o = position, d = ((lower_left + u horizontal) + v vertical) - position
   (get_ray with the jitter fixed at 0.5; lens_radius is ignored) through the scene's closest-hit
   loop: list order, t_min = 0.001, t_max = the closest root so far, strict comparisons, every
   operation rounded once in f32 (fo-rma_amd/csrc/gbuffer.h). prim = the winner's list index or
   FR_GBUFFER_MISS; depth = the winner's own accepted root t (not the shared hit record's last
   written t, which a later plane can leave stale); normal = the winner's normal at that root;
   position = o + t d; albedo = the primitive's attenuation (its colour, or 1 for the light
   material). A miss has depth 0, normal and position 0 and albedo 1.
   fr_ctx_gbuffer uploads or reuses the scene's device copy, enqueues one pass behind the
   context's enqueued resolves and returns at once; the buffers are keyed by that upload, the
   camera's 104 bytes, W and H, allocated on first use and kept while the size is unchanged.
   Frames, the accumulation, the outputs of the frames, the pending render and its stats are
   untouched. A scene that has a tree (48 primitives or more, at most 32 planes) is walked through
   it from a camera within the tree's reach, with the bits of the list loop; smaller scenes and
   cameras farther out test every primitive of the list for every pixel (fr_ctx_gbuffer_info
   says which). FR_EARG for a width or height of 0 and for more than 2^27 pixels. */
#define FR_GBUFFER_MISS 0xFFFFFFFFu
int fr_ctx_gbuffer(fr_ctx* ctx, fr_scene* scene, const fr_camera* cam, uint32_t width, uint32_t height);
/* Waits for the last fr_ctx_gbuffer; any pointer may be NULL. prim and depth W*H, normal,
   position and albedo W*H*3, row-major. FR_EARG if no G-buffer was enqueued since the buffers were
   (re)allocated. */
int fr_ctx_download_gbuffer(fr_ctx* ctx, uint32_t* prim, float* depth, float* normal, float* position,
                            float* albedo);
/* *tree = 1 if the last fr_ctx_gbuffer walked the scene's tree, 0 if the list. The host's record:
   nothing is waited for. FR_EARG if no G-buffer was enqueued. */
int fr_ctx_gbuffer_info(fr_ctx* ctx, int* tree);

/* Ray queries: the closest hit of each of the caller's n rays (o, d), through the same
   closest-hit loop as fr_ctx_gbuffer (list order, t_min = 0.001, t_max = FLT_MAX, strict
   comparisons, every operation rounded once in f32; fo-rma_amd/csrc/cast.h). A hit is a G-buffer
   pixel: prim = the winner's list index or FR_GBUFFER_MISS, t = its own accepted root, normal,
   position = o + t d and albedo; a miss has t 0, normal and position 0 and albedo 1. d is taken as
   it is (not normalised). A scene that has a tree is walked through it, with the bits of the list
   loop; FR_CAST_LIST walks the list in order all the same.
   fr_ctx_cast uploads or reuses the scene's device copy, copies host rays before it returns (the
   caller may free them), enqueues one kernel behind the context's enqueued resolves and returns at
   once. The ray and hit buffers are allocated on first use and replaced when n grows. Frames, the
   accumulation, the outputs, the pending render and its stats, the G-buffer and the temporal
   history are untouched. FR_EARG, with nothing enqueued, for n = 0, n > 2^27, a NULL pointer or an
   unknown flag. */
typedef struct fr_ray { float o[3]; float pad0; float d[3]; float pad1; } fr_ray;      /* 32 bytes; pads ignored (pad1: FR_CAST_TMAX) */
typedef struct fr_cast_info { uint32_t n, tree, waves_tree, waves_list; } fr_cast_info; /* tree: 1 if the scene's tree was walked */
#define FR_CAST_LIST        1u   /* walk the list in order even if the scene has a tree */
#define FR_CAST_RAYS_DEVICE 2u   /* rays is a device pointer on the context's device, complete at the call,
                                    valid until fr_ctx_download_hits returns */
#define FR_CAST_TMAX 16u         /* fr_ray::pad1 is the ray's t_max: closest starts at it instead of FLT_MAX
                                    and nothing else changes, so the hit is the list loop's over (0.001,
                                    t_max), planes gated on their denominator against closest as ever;
                                    whatever NaN (a miss), +-inf, 0 or a negative gives in the loop's
                                    comparisons is the answer. Without it the pad is ignored */
#define FR_CAST_OUT_DEVICE 8u    /* fr_ctx_occluded only: out is a device pointer of n bytes on the context's
                                    device, written by the kernel, valid until the query has completed */
/* The pinhole ray of pixel (x, y) of a W x H view, fr_ctx_gbuffer's: o = position,
   d = ((lower_left + u horizontal) + v vertical) - position. Host only. FR_EARG for a NULL
   pointer, W or H of 0, x >= W or y >= H. */
int fr_camera_pixel_ray(const fr_camera* cam, uint32_t x, uint32_t y, uint32_t W, uint32_t H, fr_ray* out); /* host only */
int fr_ctx_cast(fr_ctx* ctx, fr_scene* scene, const fr_ray* rays, uint32_t n, uint32_t flags);
/* Waits for the last fr_ctx_cast; any pointer may be NULL. prim and t n, normal, position and
   albedo n*3. FR_EARG if nothing was cast since the buffers were (re)allocated. */
int fr_ctx_download_hits(fr_ctx* ctx, uint32_t* prim, float* t, float* normal, float* position, float* albedo);
/* The last fr_ctx_cast: its n, whether the tree was walked, and the waves (64 rays) that walked
   the tree and that fell back to the list (a wave with a ray whose origin lies beyond the tree's
   reach or is NaN, whose direction is below 2^-60 in every component, or whose o / d overflows,
   walks the list for all its rays); the two sum to ceil(n / 64). */
int fr_ctx_cast_info(fr_ctx* ctx, fr_cast_info* out);   /* waits, like the download */
/* The device addresses of the last fr_ctx_cast's hits, left on the device: three arrays of *n
   16-byte words, g0 = (normal xyz, t), g1 = (position xyz, the bits of prim), alb = (albedo rgb, 0),
   on the context's device, valid until the next fr_ctx_cast of a larger n or fr_ctx_free. Any
   pointer may be NULL. Nothing is waited for: the words are complete after fr_ctx_sync,
   fr_ctx_cast_info or fr_ctx_download_hits. FR_EARG if nothing was cast. */
int fr_ctx_hit_buffers(fr_ctx* ctx, void** g0, void** g1, void** alb, uint32_t* n);

/* Occlusion queries (any hit): out[i] = 1 if a primitive of the scene is hit by ray i within
   (0.001, t_max_i), else 0; t_max_i is fr_ray::pad1 with FR_CAST_TMAX, else FLT_MAX. The answer is
   the OR over every primitive of the list of its own test against t_max_i, with the arithmetic
   of fr_ctx_cast, and equals "fr_ctx_cast with FR_CAST_TMAX finds a hit" on every ray, t_max of
   NaN (never occluded), infinities, 0 and negatives included. Which primitive occludes is not
   reported. A scene that has a tree is walked through it, each ray stopping at its first hit;
   FR_CAST_LIST tests the list all the same. Flags: FR_CAST_LIST | FR_CAST_RAYS_DEVICE |
   FR_CAST_TMAX | FR_CAST_OUT_DEVICE. Without FR_CAST_OUT_DEVICE the bytes stay in a buffer the
   context owns (it grows with n) until fr_ctx_download_occluded fetches them, and out is not used
   and may be NULL.
   fr_ctx_occluded has fr_ctx_cast's shape: it uploads or reuses the scene's device copy, copies
   host rays before it returns, enqueues one kernel behind the context's enqueued resolves and
   returns at once. Frames, the accumulation, the outputs, the pending render and its stats, the
   G-buffer, the temporal history and the last fr_ctx_cast's hits and info are untouched. FR_EARG,
   with nothing enqueued, for n = 0, n > 2^27, a NULL ctx, scene or rays, an unknown flag, or
   FR_CAST_OUT_DEVICE with a NULL out. */
typedef struct fr_occl_info { uint32_t n, tree, waves_tree, waves_list, occluded, pad[3]; } fr_occl_info; /* 32 bytes */
int fr_ctx_occluded(fr_ctx* ctx, fr_scene* scene, const fr_ray* rays, uint32_t n, uint32_t flags, uint8_t* out);
/* Waits for the last fr_ctx_occluded, then copies its n bytes to host (NULL: only waits). After a
   FR_CAST_OUT_DEVICE query the bytes are read from the caller's buffer, which must still be there.
   FR_EARG if nothing was queried. */
int fr_ctx_download_occluded(fr_ctx* ctx, uint8_t* host);
/* The last fr_ctx_occluded: its n, whether the tree was walked, the waves (64 rays) that walked
   the tree and that fell back to the list (fr_ctx_cast_info's rule; the two sum to ceil(n / 64))
   and the number of occluded rays, counted on the device. Waits, like the download. */
int fr_ctx_occluded_info(fr_ctx* ctx, fr_occl_info* out);

/* Feature-guided denoise of the live accumulation: fr_ctx_denoise's a-trous filter with every
   non-centre tap's weight extended by the G-buffer of the same view.
   Prep: fr_ctx_denoise's m, var and validity; a hit pixel is also invalid unless depth <=
   FR_DN_FEAT_MAX, |position_c| <= FR_DN_FEAT_MAX and |normal_c| <= FR_DN_NORMAL_MAX (comparisons
   with NaN are false). With demodulate: a_c = albedo_c if FR_DN_ALB_MIN <= albedo_c <=
   FR_DN_ALB_MAX, else 1; C_c = m_c / a_c and var = ((v_r / (a_r a_r) + v_g / (a_g a_g)) +
   v_b / (a_b a_b)) / n. Without: a = 1 and the pixel is fr_ctx_denoise's.
   Level: fr_ctx_denoise's loops, order and variance prefilter. A tap is also skipped unless it
   and the centre are both hits or both misses. Between two hits
     c = (N_p.x N_q.x + N_p.y N_q.y) + N_p.z N_q.z, c = c > 0 ? c : 0, wn = c squared normal_pow2 times,
     e = dot(N_p, P_q - P_p) in the same association, z = sigma_z t_p, zden = z z + FR_DN_EPS,
     wz = zden / (zden + e e),   w = (((h h) wc) wn) wz;
   between two misses, and for the centre tap by definition, wn = wz = 1.
   Last level: mean_c = C'_c a_c for every pixel, rgb8 = to_u8 of that mean, and var is the
   variance the filter steered by in the demodulated space (of C, not of the mean); like
   fr_ctx_denoise's it is no error estimate of the filtered picture.
   The results land in fr_ctx_denoise's output buffers: fr_ctx_download_denoised and
   fr_ctx_denoised_buffers serve the last denoise of either kind. Shards are out of scope as for
   fr_ctx_denoise. */
#define FR_DN_FEAT_MAX 1099511627776.0f /* 2^40 */
#define FR_DN_NORMAL_MAX 1024.0f /* 2^10 */
#define FR_DN_ALB_MIN 0.015625f /* 2^-6 */
#define FR_DN_ALB_MAX 64.0f /* 2^6 */
#define FR_DN_SIGMA_Z_DEFAULT 0.03125f /* 2^-5 */
#define FR_DN_NORMAL_POW2_DEFAULT 4u
typedef struct fr_denoise_guide {
  float sigma_z;        /* finite, in (0, 1024] */
  uint32_t normal_pow2; /* 0..8: the normal weight is max(dot, 0)^(2^normal_pow2) */
  uint32_t demodulate;  /* 0 or 1 */
  uint32_t pad;         /* 0 */
} fr_denoise_guide;     /* 16 bytes */
/* Enqueue the guided filter; returns at once. guide NULL: FR_DN_SIGMA_Z_DEFAULT,
   FR_DN_NORMAL_POW2_DEFAULT, demodulate 1. FR_EARG, with nothing enqueued: everything
   fr_ctx_denoise refuses, a guide field out of range, no G-buffer, and a G-buffer whose scene
   upload, camera, width or height differs from the live accumulation's (fr_last_error says
   which). */
int fr_ctx_denoise_guided(fr_ctx* ctx, uint32_t levels, float k, const fr_denoise_guide* guide);

/* Temporal reuse: the live accumulation of the current view plus the accumulators of the
   previous view, reprojected per pixel through the G-buffers of both views (the temporal part
   of SVGF; fr_ctx_denoise's levels are the spatial part). Only the camera moves: a scene edit
   drops the history. Every operation rounds once in f32 (fo-rma_amd/csrc/temporal.h).
   History of a view: per image pixel the totals (A_T[3], Q_T[3], n_T, K_T), n_T and K_T in f32,
   as of the view's last fr_ctx_temporal call, with that view's G-buffer and camera.
   Reprojection, once, on the first call after a new accumulation started (an accumulating frame
   that did not continue the one before: another camera, or fr_ctx_accum_reset and the same camera,
   which reuses the view's own history). For a pixel with features (N, t, P, id):
     a miss has no history;
     q = P - pos0, e = ll0 - pos0, nrm = cross(hor0, ver0), hh = dot(hor0, hor0), vv = dot(ver0, ver0)
     (the previous camera; nrm, hh, vv once on the host), s = dot(e, nrm) / dot(q, nrm),
     r = s q - e, u = dot(r, hor0) / hh, v = dot(r, ver0) / vv, fx = floor(u W), fy = floor(v H);
     valid iff s > 0, 0 <= fx < W and 1 <= fy <= H, compared on the floats (NaN fails); the source
     pixel is (fx, H - fy): fr_ctx_gbuffer's primary ray inverted. The fetch is nearest-pixel.
     The source is accepted iff its id equals id, dot(N, N0) >= normal_min, d d <= z z + FR_DN_EPS
     with d = dot(N, P0 - P) and z = sigma_z t, and its totals have n_T > 0 and finite A_T, Q_T
     (tested in this order; the first failure is the pixel's reason).
     cap = n_max, or n_max_specular if the primitive's scatter class is metal or dielectric;
     f = n_T > cap ? cap / n_T : 1; the prior is A' = A_T f, Q' = Q_T f, n' = n_T f,
     K' = 1 + (K_T - 1) f. f = 0 (a cap of 0) and every rejected pixel: a prior of all zeros.
   While the accumulation goes on, later calls keep the prior's bits. Without a history (first
   view, fr_ctx_temporal_reset, another scene upload, size or max_depth): all zeros, every reason
   FR_TP_NO_HISTORY.
   Totals, every call: A_T = A + A', Q_T = Q + Q', n_T = (float)n + n', K_T = (float)K + K' (a
   tiled accumulation's own counts); they become the view's history.
   Picture: prep is fr_ctx_denoise's (with guide: fr_ctx_denoise_guided's) of (A_T, Q_T, n_T,
   K_T - 1). A pixel with K_T < 2, a first frame without accepted history, has no variance and
   takes var = (g g) / n_T, g = max((C_r + C_g) + C_b, FR_ERR_FLOOR), C the (demodulated) mean:
   a relative standard error of 1, except that a miss (the sky is a function of the direction
   alone) takes var = 0; valid iff |m_c| <= FR_DN_MEAN_MAX and var <= FR_DN_VAR_MAX (and
   the guided feature caps). levels = 0: the mean (remodulated with a guide), its u8 and var
   straight from prep; 1..6: that many levels of fr_ctx_denoise (guide: fr_ctx_denoise_guided).
   The results land in fr_ctx_denoise's output buffers. One frame (K = 1) is accepted.
   Enqueued behind the context's resolves; returns at once. guide NULL: unguided levels. opt
   NULL: the FR_TP_*_DEFAULT values. FR_EARG, with nothing enqueued and no state moved: no live
   accumulation, no Q, shard_count != 1, levels > 6, k or an option out of range, no G-buffer, a
   G-buffer whose scene upload, camera, width or height differs from the live accumulation's. */
#define FR_TP_NONE 0xFFFFFFFFu /* the source of a pixel without one */
#define FR_TP_REUSED 0u
#define FR_TP_NO_HISTORY 1u
#define FR_TP_MISS 2u
#define FR_TP_OFFSCREEN 3u /* behind the previous camera, or out of its frame */
#define FR_TP_ID 4u
#define FR_TP_NORMAL 5u
#define FR_TP_PLANE 6u
#define FR_TP_HISTORY 7u /* the source's totals are empty or not finite */
#define FR_TP_N_MAX_DEFAULT 32.0f
#define FR_TP_N_MAX_SPECULAR_DEFAULT 4.0f
#define FR_TP_SIGMA_Z_DEFAULT 0.03125f /* 2^-5 */
#define FR_TP_NORMAL_MIN_DEFAULT 0.9f
#define FR_TP_N_MAX_MAX 16777216.0f /* 2^24 */
typedef struct fr_temporal {
  float n_max, n_max_specular; /* samples; n_max finite in (0, 2^24], n_max_specular finite in [0, 2^24] */
  float sigma_z;               /* finite, in (0, 1024] */
  float normal_min;            /* finite, in [-1, 1] */
  uint32_t pad[4];             /* 0 */
} fr_temporal;                 /* 32 bytes */
int fr_ctx_temporal(fr_ctx* ctx, uint32_t levels, float k, const fr_denoise_guide* guide, const fr_temporal* opt);
/* Drops the history (host state only): the next fr_ctx_temporal starts with an empty prior. */
int fr_ctx_temporal_reset(fr_ctx* ctx);
/* Waits for the last fr_ctx_temporal; any pointer may be NULL. prior_a, prior_q, total_a, total_q
   W*H*3 f32; prior_n, prior_k, total_n, total_k W*H f32; source (y0 W + x0, or FR_TP_NONE) and
   reason (FR_TP_*) W*H, row-major. FR_EARG if no fr_ctx_temporal was enqueued since the buffers
   were (re)allocated. */
int fr_ctx_download_temporal(fr_ctx* ctx, float* prior_a, float* prior_q, float* prior_n, float* prior_k,
                             float* total_a, float* total_q, float* total_n, float* total_k, uint32_t* source,
                             uint32_t* reason);

/* ---- persistent multi-device context (tracer.rs:83-134 render_mt, one device per shard) ----
   Entry i of `devices` renders row shard i of n of every frame on its own fr_ctx (device
   entries may repeat). Contexts, device buffers and the page-locked host frame persist
   across renders; a frame no larger than the last allocates nothing. */
int fr_mctx_create(const int* devices, int n, fr_mctx** out);
void fr_mctx_free(fr_mctx* mctx);
int fr_mctx_count(const fr_mctx* mctx);
/* The i-th shard's context (owned by the mctx). */
int fr_mctx_ctx(fr_mctx* mctx, int i, fr_ctx** out);
/* Enqueue one frame: every shard's render, then its asynchronous gather into the host
   frame; returns at once. params' shard fields are ignored (shard i of n). The u8 image
   is gathered when params->flags has FR_FLAG_WRITE_U8. */
int fr_mctx_render(fr_mctx* mctx, fr_scene* scene, const fr_camera* cam, const fr_params* params);
/* Wait for every shard and gather; stats summed over shards (times: the slowest shard). */
int fr_mctx_sync(fr_mctx* mctx, fr_stats* stats);
/* The page-locked host frame (W*H*3 f32 means, W*H*3 u8), valid until the next render. */
int fr_mctx_frame(fr_mctx* mctx, const float** mean_rgb, const uint8_t** rgb8);
/* Wait, then copy the host frame into caller buffers (either may be NULL). */
int fr_mctx_download(fr_mctx* mctx, float* mean_rgb, uint8_t* rgb8);
/* FR_FLAG_ACCUMULATE passes through fr_mctx_render to every shard's context; these reset every
   shard's accumulation and report shard 0's figures (all shards agree by construction). */
int fr_mctx_accum_reset(fr_mctx* mctx);
int fr_mctx_accum_info(fr_mctx* mctx, uint32_t* frames, uint32_t* samples);
/* fr_ctx_accum_error on every shard: pixels and converged are the shards' sums, max_rel their
   maximum, frames and samples shard 0's. rel, when not NULL, receives the whole W x H map. */
int fr_mctx_accum_error(fr_mctx* mctx, float threshold, fr_accum_error* out, float* rel /* or NULL */);
/* FR_FLAG_ADAPTIVE passes through fr_mctx_render. fr_ctx_adapt on every shard: the counts are
   the shards' sums, max_rel their maximum, frames and samples the largest of the shards' (a
   shard whose list was empty did not advance). */
int fr_mctx_adapt(fr_mctx* mctx, float threshold, uint32_t min_samples, fr_adapt_info* out);

/* Page-locked host memory (hipHostMalloc) for fr_ctx_download_async targets. */
int fr_host_alloc(size_t bytes, void** out);
void fr_host_free(void* p);

/* ---- synchronous conveniences ---- */
/* One shard on one device; writes the shard's rows into caller-owned host buffers. */
int fr_render_hip(fr_scene* scene, const fr_camera* cam, const fr_params* params, int device,
                  float* mean_rgb, uint8_t* rgb8, fr_stats* stats);
/* The whole image row-sharded across devices 0..n_gpus-1: an fr_mctx created, used once and freed. */
int fr_render_hip_multi(fr_scene* scene, const fr_camera* cam, const fr_params* params, int n_gpus,
                        float* mean_rgb, uint8_t* rgb8, fr_stats* stats);

/* ---- post-process effects (src/shaders/compute/<name>.comp.wgsl, rendering/post_processor.rs:101-129) ----
   Effect ids in shader_utils.rs:58-71 order. Images are RGBA8, row-major, W*H*4 bytes.
   Effects run in the given order, each reading the previous one's output, exactly like
   the reference's ping-pong between its two intermediate textures; `time` is the
   control uniform's values[0] (post_processor.rs:114, seconds), used by noise.
   Implementation-defined WGSL details are fixed in DESIGN.md §4.10. */
#define FR_FX_NONE 0
#define FR_FX_NOISE 1
#define FR_FX_PIXELATE 2
#define FR_FX_INVERT_COLOR 3
#define FR_FX_WAVE 4
#define FR_FX_INTERLACE 5
#define FR_FX_FLIP_AXIS 6
#define FR_FX_GRAYSCALE 7
#define FR_FX_STEP 8
#define FR_FX_WATERCOLOR 9
#define FR_FX_CHROMOSTEREOPSIS 10
#define FR_FX_ANAGLYPH 11
/* Host buffers in and out (synchronous). */
int fr_post_process(int device, const int* effects, uint32_t n_effects, float time, uint32_t width, uint32_t height,
                    const uint8_t* rgba_in, uint8_t* rgba_out);
/* Device buffers, in place on d_rgba (d_scratch: another W*H*4 bytes), async on `stream`. */
int fr_post_process_device(void* stream, const int* effects, uint32_t n_effects, float time, uint32_t width,
                           uint32_t height, uint8_t* d_rgba, uint8_t* d_scratch);
/* Device RGB8 (a render's u8 output) -> RGBA8 with alpha 255, async on `stream`. */
int fr_rgb_to_rgba_device(void* stream, const uint8_t* d_rgb, uint8_t* d_rgba, size_t pixels);

/* ---- diagnostics ---- */
/* Run the device f32/RNG primitives on n inputs (op codes in DESIGN.md §7); used by the
   parity tests to show the GPU arithmetic is bit-identical to the host's. */
int fr_selftest_ops(int device, int op, const float* a, const float* b, uint32_t n, float* out);
int fr_selftest_rng(int device, uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t n, uint32_t* out);
/* Compare the device's fast reciprocal (rcp + one Newton step) with the correctly rounded
   1.0f / x for every f32 bit pattern in [base, base + count): mismatches per exponent
   field in bad[256], first mismatching pattern in first[256] (0xFFFFFFFF = none). */
int fr_selftest_recip(int device, uint64_t base, uint64_t count, uint64_t* bad, uint32_t* first);
/* Compare div_rn (q0 = a y, one FMA residual correction, y = RN(1 / b)) with the IEEE
   division for every a in [1, 2) and the b = 1 + m 2^-23, m in [b_base, b_base + b_count):
   *bad = differing pairs, *first = least (m << 23 | a's mantissa) among them (~0 = none). */
int fr_selftest_div(int device, uint32_t b_base, uint32_t b_count, uint64_t* bad, uint64_t* first);
/* No device needed: hiprtc compiles the scene-specialised kernel for `arch` with n 64-B
   device records (16 u32 each, kind in word 15); targs = trace_kernel's 8 template
   arguments, or NULL for the headline's (all boxes, diffuse, depth <= 8, 8-B records);
   *code_bytes = the code object's size, *ms = the compile time. */
int fr_selftest_jit(const char* arch, const uint32_t* rec, uint32_t n, const int* targs, size_t* code_bytes,
                    double* ms);

#ifdef __cplusplus
}
#endif
#endif /* FORMA_RT_H */
