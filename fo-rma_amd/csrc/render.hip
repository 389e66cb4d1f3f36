// render.hip — the host driver of the gfx950 path-tracing megakernel (trace_kernel.h).
//
// Replaces cpu_ray_tracer/tracer.rs:160-219 (save_image + recursive get_color)
// and the shapes/ hit/scatter code it calls. A persistent grid pulls work items
// (one pixel's 16-sample RNG block) from a global counter; every lane holds one path
// segment per loop iteration and a lane whose path ends starts its next sample at
// once (path regeneration), so lanes never wait for each other's pixels. Each
// sample's colour goes to a per-sample buffer that sum_kernel adds per pixel in
// sample order, exactly as `col = col + get_color(...)` does (tracer.rs:170-175).
// The attenuation product is unwound right-to-left from a per-lane LDS stack,
// reproducing the recursion's association a0*(a1*(...*terminal)) bit for bit.
//
// Closest hit: small scenes test primitive i on every lane at once (wave-uniform:
// the kind switch is a scalar branch, records arrive by scalar loads); large ones
// walk a BVH per lane (LDS stack), cut at the planes (bvh.h). Layout and rooflines:
// DESIGN.md §4-§5.
//
// This file: the scene upload (pack.h builds the bytes), the fr_ctx lifecycle, grid
// sizing, and the enqueue of a frame that plan.h has planned; sync, download, trace log.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <chrono>
#include <cmath>
#include <string>
#include <vector>

#include "accum_error.h"
#include "denoise.h"
#include "gbuffer.h"
#include "cast.h"
#include "hipchk.h"
#include "jit.h"
#include "pack.h"
#include "plan.h"
#include "refit.h"
#include "sum.h"
#include "temporal.h"
#include "trace_kernel.h"

namespace fr {

// ABI layout, mirrored by ctypes (forma_rt.py) and the Rust binding
static_assert(sizeof(fr_prim) == 88, "fr_prim layout");
static_assert(sizeof(fr_camera) == 104, "fr_camera layout");
static_assert(sizeof(fr_params) == 40, "fr_params layout");
static_assert(sizeof(fr_stats) == 72, "fr_stats layout");
static_assert(sizeof(fr_accum_error) == 32, "fr_accum_error layout");
static_assert(sizeof(fr_adapt_info) == 56, "fr_adapt_info layout");
static_assert(sizeof(fr_scene_info) == 72, "fr_scene_info layout");

struct DeviceCopy {
  int device = -1;
  uint64_t version = 0;
  uint64_t edit_seq = 0;  // the scene's edit sequence these tables hold
  uint64_t uid = 0;  // process-unique per upload or patch: names these exact records (fr_ctx's kernel cache)
  void* blob = nullptr;
  PackedScene ps;  // the blob's layout and facts (its bytes released after the upload)
  // In-place catch-up: the staged rows (pinned host and device, reused: every patch starts with a
  // device-wide wait, so the last copy out of them is done), the events around its parts and the
  // event every user's streams wait for while it may be pending.
  PatchRow* h_rows = nullptr;
  PatchRow* d_rows = nullptr;
  uint32_t cap_rows = 0;
  hipEvent_t ev_part[3] = {};  // before the copy, after it, after the patch kernel
  hipEvent_t ev_done = nullptr;
  bool patch_pending = false;
  float host_ms = 0.0f;  // the last patch's host preparation
  uint64_t packs = 0, refits = 0;
};

// What one use of a scene did to its device copy (fr_ctx_scene_info).
struct SceneSync {
  const DeviceCopy* copy = nullptr;
  uint32_t kind = FR_SCENE_SYNC_NONE, prims = 0, nodes = 0, launches = 0;
  uint64_t refit_no = 0;  // the copy's refit count after it (its events are those of this patch)
};

// Sums the trace kernel's per-wave counters (KWork::wave_counters) into counters[0..2].
__global__ __launch_bounds__(256) void reduce_counters(const unsigned long long* __restrict__ wc, uint32_t waves,
                                                       unsigned long long* __restrict__ counters) {
  __shared__ unsigned long long part[3][256];
  unsigned long long v[3] = {0, 0, 0};
  for (uint32_t w = threadIdx.x; w < waves; w += 256)
    for (int k = 0; k < 3; ++k) v[k] += wc[3 * w + k];
  for (int k = 0; k < 3; ++k) part[k][threadIdx.x] = v[k];
  __syncthreads();
  for (uint32_t h = 128; h > 0; h >>= 1) {
    if (threadIdx.x < h)
      for (int k = 0; k < 3; ++k) part[k][threadIdx.x] += part[k][threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x < 3) atomicAdd(&counters[threadIdx.x], part[threadIdx.x][0]);  // passes on two streams
}

// ---- device scene copies ----------------------------------------------------

static std::atomic<uint64_t> g_uploads{0};

static RefitTables refit_tables(const DeviceCopy* c) {
  char* b = static_cast<char*>(c->blob);
  const PackedScene& ps = c->ps;
  return RefitTables{reinterpret_cast<float4*>(b + ps.off_rec),
                     reinterpret_cast<float4*>(b + ps.off_lrec),
                     reinterpret_cast<BvhNode*>(b + ps.off_bvh),
                     reinterpret_cast<RefitBox*>(b + ps.off_slot_bounds),
                     reinterpret_cast<RefitBox*>(b + ps.off_unions),
                     reinterpret_cast<const uint32_t*>(b + ps.off_slot_of),
                     reinterpret_cast<const uint32_t*>(b + ps.off_sched),
                     ps.facts.n,
                     ps.n_slots,
                     ps.n_nodes};
}

// A copy at the scene's version and an older edit sequence catches up in place (DESIGN.md
// §4.7a): the primitives stamped since are packed on the host, copied and scattered, and every
// node is refitted, on `stream`. *patched = false, with nothing enqueued or changed, when the
// copy's tree cannot take an edit: a primitive whose own bounds leave the packed extent (the
// packed padding and reach would fall below a fresh build's) or whose bounds verdict at the
// packed reach is not its slot's. The caller re-packs then.
static int patch_copy(fr_scene* s, DeviceCopy* c, hipStream_t stream, SceneSync* sync, bool* patched) {
  *patched = false;
  const auto t0 = std::chrono::steady_clock::now();
  PackedScene& ps = c->ps;
  const uint32_t n = static_cast<uint32_t>(s->prims.size());
  if (ps.facts.n != n || s->stamp.size() != n) return FR_OK;
  const bool tree = ps.facts.bvh_ok && ps.n_nodes + ps.n_slots > 0;
  const float extent = ps.facts.bvh_extent;
  const float reach = bvh_origin_reach(extent, ps.facts.bvh_sphere_rmin);
  std::vector<uint32_t> ids;
  for (uint32_t i = 0; i < n; ++i)
    if (s->stamp[i] > c->edit_seq) ids.push_back(i);
  const uint32_t m = static_cast<uint32_t>(ids.size());
  if (tree)
    for (uint32_t i : ids) {
      RefitBox own, at_reach;
      if (bvh_prim_bounds(s->prims[i], -1.0f, &own))
        for (int k = 0; k < 3; ++k)
          if (!(fabsf(own.lo[k]) <= extent) || !(fabsf(own.hi[k]) <= extent)) return FR_OK;
      if (bvh_prim_bounds(s->prims[i], reach, &at_reach) != (ps.slot_of[i] != kNoSlot)) return FR_OK;
    }
  // write-after-read: everything enqueued on this device so far reads the old tables
  HIPCHK(hipDeviceSynchronize());
  if (m > c->cap_rows) {
    if (c->h_rows) HIPCHK(hipHostFree(c->h_rows));
    if (c->d_rows) HIPCHK(hipFree(c->d_rows));
    c->h_rows = c->d_rows = nullptr;
    c->cap_rows = 0;
    HIPCHK(hipHostMalloc(&c->h_rows, static_cast<size_t>(m) * sizeof(PatchRow), hipHostMallocDefault));
    HIPCHK(hipMalloc(&c->d_rows, static_cast<size_t>(m) * sizeof(PatchRow)));
    c->cap_rows = m;
  }
  if (!c->ev_done) {
    for (hipEvent_t& e : c->ev_part) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipEventCreate(&c->ev_done));
  }
  for (uint32_t k = 0; k < m; ++k) {
    const fr_prim& p = s->prims[ids[k]];
    PatchRow& r = c->h_rows[k];
    r = PatchRow{};
    r.index = ids[k];
    pack_record(p, r.rec);
    leaf_record(r.rec, r.lrec);
    r.bounds = refit_empty();
    if (tree) (void)bvh_prim_bounds(p, reach, &r.bounds);
    memcpy(&ps.rec_words[16u * static_cast<size_t>(ids[k])], r.rec, 64);  // the scene-specialised build's constants
  }
  c->host_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  const RefitTables t = refit_tables(c);
  uint32_t launches = 0;
  HIPCHK(hipEventRecord(c->ev_part[0], stream));
  if (m) HIPCHK(hipMemcpyAsync(c->d_rows, c->h_rows, static_cast<size_t>(m) * sizeof(PatchRow), hipMemcpyHostToDevice, stream));
  HIPCHK(hipEventRecord(c->ev_part[1], stream));
  if (m) HIPCHK(launch_scene_patch(stream, t, c->d_rows, m));
  HIPCHK(hipEventRecord(c->ev_part[2], stream));
  if (tree && m) HIPCHK(launch_bvh_refit(stream, t, ps.sched, 1e-4f * extent + 1e-4f, &launches));
  HIPCHK(hipEventRecord(c->ev_done, stream));
  c->patch_pending = true;
  c->edit_seq = s->edit_seq;
  c->uid = ++g_uploads;
  ++c->refits;
  *sync = SceneSync{c, FR_SCENE_SYNC_REFIT, m, launches ? ps.n_nodes : 0u, launches, c->refits};
  *patched = true;
  return FR_OK;
}

// The scene's copy on `device`: the cached one while the scene's version and edit sequence
// stand, patched in place when only the sequence moved (patch_copy, on streams[0]), else packed
// (pack.h) and uploaded. While a patch may be pending, every stream of `streams` (the ones the
// caller reads the scene on) waits for it.
static int upload_scene(fr_scene* s, int device, bool force_bvh, DeviceCopy** out, const hipStream_t (&streams)[3],
                        SceneSync* sync) {
  std::lock_guard<std::mutex> g(s->mu);
  DeviceCopy* c = nullptr;
  for (DeviceCopy* e : s->copies)
    if (e->device == device) c = e;
  *sync = SceneSync{c};
  if (c && c->version == s->version) {
    bool current = c->edit_seq == s->edit_seq;
    if (!current) {
      const int rc = patch_copy(s, c, streams[0], sync, &current);
      if (rc) return rc;
    }
    if (current) {
      if (c->patch_pending && hipEventQuery(c->ev_done) == hipSuccess) c->patch_pending = false;
      if (c->patch_pending)
        for (hipStream_t st : streams) HIPCHK(hipStreamWaitEvent(st, c->ev_done, 0));
      *out = c;
      return FR_OK;
    }
  }
  if (!c) {
    c = new DeviceCopy();
    c->device = device;
    s->copies.push_back(c);
  }
  HIPCHK(hipFree(c->blob));
  c->blob = nullptr;
  c->ps = pack_scene(s->prims, force_bvh);
  HIPCHK(hipMalloc(&c->blob, c->ps.bytes.size()));
  HIPCHK(hipMemcpy(c->blob, c->ps.bytes.data(), c->ps.bytes.size(), hipMemcpyHostToDevice));
  std::vector<unsigned char>().swap(c->ps.bytes);
  c->version = s->version;
  c->edit_seq = s->edit_seq;
  c->patch_pending = false;
  c->uid = ++g_uploads;
  ++c->packs;
  *sync = SceneSync{c, FR_SCENE_SYNC_PACK, 0, 0, 0, c->refits};
  *out = c;
  return FR_OK;
}

void release_device_copies(fr_scene* s) {
  std::lock_guard<std::mutex> g(s->mu);
  for (DeviceCopy* c : s->copies) {
    if (c->blob) {
      int cur = 0;
      if (hipGetDevice(&cur) == hipSuccess) {
        (void)hipSetDevice(c->device);
        (void)hipFree(c->blob);
        if (c->d_rows) (void)hipFree(c->d_rows);
        if (c->h_rows) (void)hipHostFree(c->h_rows);
        for (hipEvent_t e : c->ev_part)
          if (e) (void)hipEventDestroy(e);
        if (c->ev_done) (void)hipEventDestroy(c->ev_done);
        (void)hipSetDevice(cur);
      }
    }
    delete c;
  }
  s->copies.clear();
}

}  // namespace fr

using namespace fr;

constexpr int kCntWords = 64;  // counter words per frame slot (fr_ctx::d_cnt)

struct fr_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_start = nullptr;
  std::vector<hipEvent_t> ev_trace;  // start/stop pairs around each pass's trace kernel
  std::vector<hipEvent_t> ev_sum;    // end of each pass's sum kernel
  // Pass pipeline: traces alternate between `stream` and `stream2`,
  // sums run on `stream_sum`, so a pass's sum and tail overlap the next pass's trace.
  hipStream_t stream2 = nullptr, stream_sum = nullptr;
  // fr_ctx_download_async: D2H copies of the last render on their own stream; the next
  // render's first sum kernel (the first writer of d_mean / d_u8) waits for ev_copy, so a
  // frame's gather overlaps the next frame's trace.
  hipStream_t stream_copy = nullptr;
  hipEvent_t ev_copy = nullptr;
  bool copy_pending = false;
  int passes = 0;
  int occupancy = 0;  // trace-kernel workgroups per CU of the last launch (occupancy API)
  bool cam_axial = false;  // the last prepared or rendered frame's camera rays take cam_ray_axial
  float* d_mean = nullptr;
  uint8_t* d_u8 = nullptr;
  // [0..3] counters, [4..30] and [32..63] diagnostics (FR_SECCNT, FR_PROF, FR_DIAG builds);
  // [31] queue head: one set of kCntWords per frame slot
  unsigned long long* d_cnt = nullptr;
  unsigned long long* last_cnt = nullptr;  // the last render's set
  // Frame pipeline (FR_FRAME_PIPE): one-pass frames alternate between two
  // frame slots (sample buffer half, counter set), so frame k+1's trace starts when frame k's
  // trace ends while frame k's sum runs beside it; ev_fslot[s] = the end of the last sum
  // that used slot s, which the next frame on that slot waits for.
  int frame_slot = 0, frame_parity = 0;
  int fs_n = 0;            // slots in the current layout (2 to 4; 0: not pipelined)
  size_t fs_bytes = 0;     // sample-buffer bytes per slot in that layout
  hipEvent_t ev_fslot[kFrameSlots] = {};
  bool fslot_used[kFrameSlots] = {};
  unsigned long long* d_wcnt = nullptr;  // per-wave partial counters (KWork::wave_counters)
  float* d_samples = nullptr;
  float* d_running = nullptr;
  size_t cap_mean = 0, cap_u8 = 0, cap_samples = 0, cap_running = 0;  // bytes
  // Progressive accumulation (FR_FLAG_ACCUMULATE): A, 3 f32 per pixel slot of
  // the shard like d_running, and the host's record of what it holds as of the last enqueued
  // accumulating frame (plan.h). Only the last pass's sum of an accumulating frame touches
  // d_accum, and every sum of the context runs on stream_sum, streamed and pipelined frames
  // included: the read-modify-writes of consecutive frames are ordered by that stream alone.
  float* d_accum = nullptr;
  size_t cap_accum = 0;
  AccumState accum;
  // FR_FLAG_ACCUM_ERROR: Q, the second-moment accumulator, exists once a frame
  // asked for it and then has A's size, lifetime and ordering (the sum stream alone). accum_kp:
  // the last accumulating frame's constants, which map A's and Q's pixel slots to the image
  // for the error kernel (a plain render in between changes `last`, not these).
  float* d_sq = nullptr;
  size_t cap_sq = 0;
  KParams accum_kp{};
  // fr_ctx_accum_error's outputs: the W x H map of rel, the per-workgroup partials and the
  // summary; err_kp: the frame constants the map was written with (fr_ctx_download_error)
  float* d_err = nullptr;
  uint32_t* d_err_part = nullptr;
  ErrSummary* d_err_sum = nullptr;
  size_t cap_err = 0, cap_err_part = 0;
  KParams err_kp{};
  bool err_valid = false;
  // Adaptive sampling (FR_FLAG_ADAPTIVE), one uint32 per tile of the shard
  // each: the tiled accumulation's counts n_t and K_t, which the resolves maintain on the sum
  // stream; the active tile list an adaptive frame's trace and sums read; the selection's
  // per-tile scratch. `tiled`: the host's record (plan.h), dead with the accumulation.
  uint32_t* d_nt = nullptr;
  uint32_t* d_kt = nullptr;
  uint32_t* d_list = nullptr;
  uint32_t* d_tile_px = nullptr;
  AdaptSummary* d_adapt_sum = nullptr;
  size_t cap_nt = 0, cap_kt = 0, cap_list = 0, cap_tile_px = 0;
  TiledState tiled;
  // fr_ctx_denoise: the ping and pong pixel buffers and the three outputs,
  // allocated on first use and kept while the image size is unchanged. dn_valid: a denoise was
  // enqueued since they were (re)allocated.
  DnPixel* d_dn_ping = nullptr;
  DnPixel* d_dn_pong = nullptr;
  float* d_dn_mean = nullptr;
  uint8_t* d_dn_u8 = nullptr;
  float* d_dn_var = nullptr;
  uint32_t dn_w = 0, dn_h = 0;
  bool dn_valid = false;
  // fr_ctx_gbuffer: the view's feature buffers, W*H float4 each, allocated on
  // first use and kept while the image size is unchanged, and their key: the scene upload, the
  // camera's 104 bytes and the size they were enqueued for. gb_valid: a pass was enqueued since
  // they were (re)allocated.
  float4* d_gb0 = nullptr;
  float4* d_gb1 = nullptr;
  float4* d_gb_alb = nullptr;
  uint32_t gb_w = 0, gb_h = 0;
  uint64_t gb_uid = 0;
  fr_camera gb_cam{};
  bool gb_valid = false;
  bool gb_tree = false;  // the last fr_ctx_gbuffer walked the scene's tree (fr_ctx_gbuffer_info)
  // fr_ctx_cast: the rays' device copy (host rays arrive through the pinned
  // h_cast_rays; ev_cast: the end of the last copy out of it), the hits as the G-buffer's three
  // words per ray and the striped wave counter (cast.h), allocated on first use and replaced when n
  // outgrows cast_cap rays. cast_valid: a cast was enqueued since they were (re)allocated.
  float4* d_cast_rays = nullptr;
  float4* h_cast_rays = nullptr;
  size_t cap_cast_rays = 0, cap_cast_host = 0;  // bytes
  hipEvent_t ev_cast = nullptr;
  bool cast_copy_pending = false;
  float4* d_hit0 = nullptr;
  float4* d_hit1 = nullptr;
  float4* d_hit_alb = nullptr;
  uint32_t* d_cast_waves = nullptr;
  uint32_t cast_cap = 0, cast_n = 0;
  bool cast_valid = false, cast_tree = false;
  // fr_ctx_occluded: one byte per ray and a wave counter of its own (the last
  // cast's stays what it is), allocated on first use; the bytes are replaced when n outgrows
  // occl_cap. occl_out: where the last query wrote (d_occl, or the caller's device buffer).
  uint8_t* d_occl = nullptr;
  uint32_t* d_occl_waves = nullptr;
  const uint8_t* occl_out = nullptr;
  uint32_t occl_cap = 0, occl_n = 0;
  bool occl_valid = false, occl_tree = false;
  // fr_ctx_temporal. accum_gen: the accumulation generation, advanced whenever
  // accum_step starts a new accumulation. d_gb_cls: the G-buffer's scene's effective scatter
  // classes, gb_n of them, copied with every fr_ctx_gbuffer (the scene's own table dies with an
  // edit of the scene). Per image pixel, allocated on first use and kept while the size is
  // unchanged: the totals' two words in two buffers each (tp.read: the one the current prior was
  // reprojected from; the calls write the other), the history view's G-buffer words and camera,
  // the prior's two words, the source map and the reason codes. tp_valid: a call was enqueued
  // since they were (re)allocated; tp_last: the totals buffer it wrote.
  uint64_t accum_gen = 0;
  uint32_t* d_gb_cls = nullptr;
  size_t cap_gb_cls = 0;
  uint32_t gb_n = 0;
  float4* d_tp_ta[2] = {nullptr, nullptr};
  float4* d_tp_tq[2] = {nullptr, nullptr};
  float4* d_tp_g0 = nullptr;
  float4* d_tp_g1 = nullptr;
  float4* d_tp_pa = nullptr;
  float4* d_tp_pq = nullptr;
  uint32_t* d_tp_src = nullptr;
  uint32_t* d_tp_why = nullptr;
  uint32_t tp_w = 0, tp_h = 0, tp_last = 0;
  GbCam tp_cam{};
  TemporalState tp;
  bool tp_valid = false;
  // the last render was adaptive: the image pixels it traced (fr_stats), or none (empty list)
  bool last_adaptive = false, last_empty = false;
  uint64_t last_active_pixels = 0;
  int num_cus = 0;
  size_t device_bytes = 0;  // HBM size (the sample buffer budget's default)
  fr_params last{};
  uint32_t last_n = 0;
  bool pending = false;
  // the last render was enqueued while the one before it still ran (frames streamed): the
  // next render reserves slots for overlapping even if it finds the device idle (PlanHistory)
  bool streaming = false;
  std::chrono::steady_clock::time_point t0;
  // the last render's trace kernel: scene-specialised (jit.h) or compiled in
  bool jit_used = false;
  JitStats jit_stats{};
  int jit_state = FR_JIT_OFF;
  // the scene kernel the last lookup found and what it was for (upload, specialisation
  // flags), pinned loaded: a frame of the same scene and shape skips the lookup (its
  // prelude and key hashing are ~0.1 ms of host time per render)
  hipFunction_t jc_fn = nullptr;
  std::shared_ptr<void> jc_pin;
  uint64_t jc_uid = 0;
  uint32_t jc_flags = 0;
  bool jc_small = false;
  // fr_ctx_trace_log: event pairs around every trace launch since the log was enabled,
  // across renders (ev_trace holds only the last render's), so a caller streaming K
  // frames can average the kernel's duration over all of them
  // log 0: trace launches (on the launch's stream); log 1: whole renders (ev0 .. ev1)
  bool log_on = false;
  // log 2: the three stages of every fr_ctx_temporal call (prior, totals and prep, picture), on the sum stream
  // log 3: every cast kernel and G-buffer pass, on the sum stream
  std::vector<hipEvent_t> log_ev[4];  // 2 per entry (start, end); reused across logs
  size_t log_n[4] = {0, 0, 0, 0};     // entries logged
  // what this context's last use of a scene did to the scene's device copy (fr_ctx_scene_info)
  SceneSync scene_sync{};
};

// The scene's device copy for a call of this context, caught up (upload_scene): a patch goes on
// the context's first trace stream, and the streams its kernels read scenes on wait for it.
static int ctx_scene(fr_ctx* c, fr_scene* scene, bool force_bvh, DeviceCopy** out) {
  const hipStream_t streams[3] = {c->stream, c->stream2, c->stream_sum};
  return upload_scene(scene, c->device, force_bvh, out, streams, &c->scene_sync);
}

static hipError_t log_event(fr_ctx* c, int which, size_t k, hipStream_t st) {
  std::vector<hipEvent_t>& v = c->log_ev[which];
  while (v.size() <= k) {
    hipEvent_t e;
    const hipError_t err = hipEventCreate(&e);
    if (err != hipSuccess) return err;
    v.push_back(e);
  }
  return hipEventRecord(v[k], st);
}
static hipError_t log_start(fr_ctx* c, int which, hipStream_t st) {
  return log_event(c, which, 2 * c->log_n[which], st);
}
static hipError_t log_end(fr_ctx* c, int which, hipStream_t st) {
  const hipError_t e = log_event(c, which, 2 * c->log_n[which] + 1, st);
  if (e == hipSuccess) ++c->log_n[which];
  return e;
}

// A device buffer of at least `bytes`: a smaller one is freed first, and its capacity
// reads 0 until the new allocation stands.
template <class T>
static int grow(T*& ptr, size_t& cap, size_t bytes) {
  if (bytes <= cap) return FR_OK;
  if (ptr) HIPCHK(hipFree(ptr));
  ptr = nullptr;
  cap = 0;
  HIPCHK(hipMalloc(&ptr, bytes));
  cap = bytes;
  return FR_OK;
}

// An accumulator (A or Q) at `bytes` or more, its contents kept: fr_ctx_prepare may grow it for
// a larger frame while an accumulation of a smaller one is live. The copy goes on the sum
// stream, behind every sum that reads or writes the old buffer, which is freed once it is done.
static int grow_kept(fr_ctx* c, float*& buf, size_t& cap, size_t bytes) {
  if (bytes <= cap) return FR_OK;
  float* bigger = nullptr;
  HIPCHK(hipMalloc(&bigger, bytes));
  if (buf) {
    hipError_t e = hipMemcpyAsync(bigger, buf, cap, hipMemcpyDeviceToDevice, c->stream_sum);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream_sum);
    if (e != hipSuccess) {
      (void)hipFree(bigger);
      HIPCHK(e);
    }
    HIPCHK(hipFree(buf));
  }
  buf = bigger;
  cap = bytes;
  return FR_OK;
}

// A at `bytes` or more, and Q with it when the context has one or this frame asks for one
// (with_q): Q is allocated and grown with A, so a live accumulation's Q survives as A does.
static int grow_accum(fr_ctx* c, size_t bytes, bool with_q) {
  int rc = grow_kept(c, c->d_accum, c->cap_accum, bytes);
  if (!rc && (with_q || c->d_sq)) rc = grow_kept(c, c->d_sq, c->cap_sq, c->cap_accum);
  return rc;
}

static int grow_events(std::vector<hipEvent_t>& v, size_t n, unsigned flags) {
  while (v.size() < n) {
    hipEvent_t e;
    HIPCHK(hipEventCreateWithFlags(&e, flags));
    v.push_back(e);
  }
  return FR_OK;
}

static JitSpec jit_spec(const KernelId& id, const uint32_t* rec, uint32_t n) {
  return JitSpec{id.name.c_str(), id.targs, kTargBool, 8, tuning_defines(), rec, n};
}

// The scene-specialised kernel of one render (jit.h), when the plan asks for one.
struct SceneKernel {
  hipFunction_t fn = nullptr;  // null: the compiled-in kernel runs (not asked, pending, missed or failed)
  std::shared_ptr<void> pin;   // its module: launches are noted (jit_note_launch)
  JitStats stats{};            // the lookup's time and state
  int state = FR_JIT_OFF;
};

// Looked up (loaded, or compiled when waiting) before anything is enqueued, so a first
// frame's events do not span the compile; a frame of the same upload and specialisation
// reuses the context's pinned kernel.
static int find_scene_kernel(fr_ctx* c, const DeviceCopy* dc, const FramePlan& fp, SceneKernel* sk) {
  if (!fp.jit_on || !fp.kp.P) return FR_OK;
  const uint32_t jc_flags = fp.kp.flags & (KF_DEFER | KF_NIBBLE | KF_DIFFUSE | FR_FLAG_MT_BANDS);
  if (c->jc_fn && c->jc_uid == dc->uid && c->jc_flags == jc_flags && c->jc_small == fp.small_depth) {
    sk->fn = c->jc_fn;
    sk->pin = c->jc_pin;
    sk->stats.reused = 1;
    sk->stats.state = FR_JIT_USED;
  } else {
    const KernelId id = kernel_id(fp.sel);
    const int rc = jit_trace_kernel(c->device, jit_spec(id, dc->ps.rec_words.data(), dc->ps.facts.n), fp.jit_wait,
                                    &sk->fn, &sk->stats, fp.jit_cached_only);
    if (rc) return rc;
    sk->pin = sk->stats.pin;
    c->jc_fn = sk->fn;  // null (pending or failed): looked up again next render
    c->jc_pin = sk->stats.pin;
    c->jit_stats.pin.reset();
    c->jc_uid = dc->uid;
    c->jc_flags = jc_flags;
    c->jc_small = fp.small_depth;
  }
  sk->state = sk->stats.state;
  return FR_OK;
}

// Persistent grid: as many workgroups as are resident at once (the occupancy API reads the
// kernel's registers and this launch's LDS), or fewer for a small pass. A workgroup
// beyond the resident count would start only after the queue has drained.
struct Grid {
  int per_cu = 0;       // resident workgroups per CU
  uint32_t blocks = 0;  // workgroups launched
  size_t lds = 0;       // the launch's LDS bytes (the plan's, plus the BVH kernels' staging)
  bool staged = false;  // KF_STAGE
};

template <class Kern>
static Grid size_grid(Kern kern, hipFunction_t jfn, const FramePlan& fp, uint32_t n_items, int num_cus) {
  Grid g;
  g.lds = fp.lds + fp.table_bytes;
  const hipError_t oe =
      jfn ? hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&g.per_cu, jfn, static_cast<int>(kBlock), g.lds)
          : hipOccupancyMaxActiveBlocksPerMultiprocessor(&g.per_cu, kern, static_cast<int>(kBlock), g.lds);
  if (oe != hipSuccess || g.per_cu < 1) g.per_cu = 1;
  // the per-wave counter slots (fr_ctx::d_wcnt) hold kMaxWgPerCu workgroups per CU
  if (g.per_cu > static_cast<int>(kMaxWgPerCu)) g.per_cu = static_cast<int>(kMaxWgPerCu);
  // BVH kernels store their samples unstaged unless FR_BVH_STAGE asks (PlanEnv::bvh_stage)
  if (fp.stage_bytes && fp.bvh_stage) {
    const bool force_stage = fp.bvh_stage == 1;
    int staged = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&staged, kern, static_cast<int>(kBlock),
                                                     g.lds + fp.stage_bytes) == hipSuccess &&
        (staged >= g.per_cu || (force_stage && staged >= 1))) {
      g.per_cu = staged < static_cast<int>(kMaxWgPerCu) ? staged : static_cast<int>(kMaxWgPerCu);
      g.lds += fp.stage_bytes;
      g.staged = true;
    }
  }
  int launch_per_cu = g.per_cu;
  // only full 8-workgroup grids give a slot up: the BVH kernels (6 per CU) lost a sixth of
  // their grid for a sum of a twentieth of their frame (C5 55.6 -> 58.0 ms)
  if (fp.reserve && g.per_cu >= static_cast<int>(kMaxWgPerCu)) launch_per_cu -= static_cast<int>(fp.reserve);
  g.per_cu = launch_per_cu;
  uint64_t cap = static_cast<uint64_t>(g.per_cu) * static_cast<uint64_t>(num_cus);
  if (fp.max_wgs && fp.max_wgs < cap) cap = fp.max_wgs;  // FR_MAX_WGS
  const uint64_t want = (static_cast<uint64_t>(n_items) + kBlock - 1u) / kBlock;  // workgroups the pass could use
  g.blocks = static_cast<uint32_t>(want < cap ? (want ? want : 1u) : cap);
  return g;
}

// One trace launch of the plan's specialisation (select_kernel), or of the scene kernel.
struct Launched {
  int rc = FR_OK;
  Grid grid;
};

template <class Kern>
static int enqueue_trace(Kern kern, const SceneKernel& sk, const Grid& g, hipStream_t st, KArgs a) {
  if (g.staged) a.kp.flags |= KF_STAGE;
  a.kp.n_static = g.blocks * kBlock;  // one 64-item batch per wave of the grid
  if (sk.fn) {
    // the same by-value KArgs at kernarg offset 0 as the compiled-in kernels take
    size_t bytes = sizeof(KArgs);
    void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &bytes, HIP_LAUNCH_PARAM_END};
    HIPCHK(hipModuleLaunchKernel(sk.fn, g.blocks, 1, 1, kBlock, 1, 1, static_cast<uint32_t>(g.lds), st, nullptr, cfg));
    jit_note_launch(sk.pin, st);  // an LRU eviction waits for the last launch on every stream used
  } else {
    hipLaunchKernelGGL(kern, dim3(g.blocks), dim3(kBlock), g.lds, st, a);
  }
  return FR_OK;
}

static Launched launch_trace(const FramePlan& fp, int num_cus, const SceneKernel& sk, hipStream_t st, const KArgs& a) {
  return select_kernel(fp.sel, [&](auto tag) {
    using T = decltype(tag);
    auto kern = trace_kernel<T::KS, T::HP, T::KREJ, T::MAXD, T::BV, T::MT, T::DEFER, T::MAT>;
    Launched l;
    l.grid = size_grid(kern, sk.fn, fp, a.kp.n_items, num_cus);
    l.rc = enqueue_trace(kern, sk, l.grid, st, a);
    return l;
  });
}

static KScene kscene(const DeviceCopy* dc, const FramePlan& fp) {
  const PackedScene& ps = dc->ps;
  const char* b = static_cast<const char*>(dc->blob);
  KScene ks;
  ks.rec = reinterpret_cast<const float4*>(b + ps.off_rec);
  ks.mat = reinterpret_cast<const float4*>(b + ps.off_mat);
  ks.cls = reinterpret_cast<const uint32_t*>(b + ps.off_cls);
  ks.att = reinterpret_cast<const float4*>(b + ps.off_att);
  ks.acls = reinterpret_cast<const uint32_t*>(b + ps.off_acls);
  ks.n = ps.facts.n;
  ks.bvh = reinterpret_cast<const float4*>(b + ps.off_bvh);
  ks.bvh_order = reinterpret_cast<const uint32_t*>(b + ps.off_bvh_order);
  ks.lrec = reinterpret_cast<const float4*>(b + ps.off_lrec);
  ks.segs = reinterpret_cast<const uint4*>(b + ps.off_segs);
  ks.runs = reinterpret_cast<const uint4*>(b + ps.off_runs);
  ks.n_runs = ps.n_runs;
  ks.n_segs = fp.use_bvh ? ps.facts.n_segs : 0u;
  ks.reach = bvh_origin_reach(ps.facts.bvh_extent, ps.facts.bvh_sphere_rmin);
  ks.att_nonneg = ps.att_nonneg ? 1u : 0u;
  return ks;
}

// Whether Camera::get_ray's short form (trace_kernel.h cam_ray_axial) gives this camera's rays
// bit for bit: the argument, term by term, is DESIGN.md §4.2. Every condition is needed by
// one dropped operation; a camera that fails any takes cam_ray, which is untouched.
static bool is_zero(float x) { return x == 0.0f; }                    // +0 or -0
static bool is_neg_zero(float x) { return x == 0.0f && std::signbit(x); }
static bool cam_axial(const KCam& k) {
  const float all[] = {k.px, k.py, k.pz, k.lx, k.ly, k.lz, k.hx, k.hy, k.hz, k.vx,
                       k.vy, k.vz, k.ux, k.uy, k.uz, k.bx, k.by, k.bz, k.lens, k.dz};
  for (float x : all)
    if (!std::isfinite(x)) return false;
  // the lens offset's products use lens_s (exact) and never underflow to a zero that the
  // lens draw did not put there
  if (!(k.lens_pre & kCamLensPre) || !(k.lens > 0.0f)) return false;
  if (!(k.lens_s * fabsf(k.ux) >= 0x1p-100f) || !(k.lens_s * fabsf(k.by) >= 0x1p-100f)) return false;
  // the eight components whose products are dropped
  if (!(is_zero(k.uy) && is_zero(k.uz) && is_zero(k.bx) && is_zero(k.bz) && is_zero(k.hy) && is_zero(k.hz) &&
        is_zero(k.vx) && is_zero(k.vz)))
    return false;
  // a dropped +-0 addend changes only a -0 partner: no partner may be -0
  if (is_zero(k.lx) || is_zero(k.ly) || is_zero(k.lz)) return false;
  if (is_neg_zero(k.px) || is_neg_zero(k.py) || is_neg_zero(k.pz)) return false;
  return true;
}

static KCam kcam(const fr_camera* cam, bool allow_axial = true) {
  KCam kc;
  kc.px = cam->position[0], kc.py = cam->position[1], kc.pz = cam->position[2];
  kc.lx = cam->lower_left[0], kc.ly = cam->lower_left[1], kc.lz = cam->lower_left[2];
  kc.hx = cam->horizontal[0], kc.hy = cam->horizontal[1], kc.hz = cam->horizontal[2];
  kc.vx = cam->vertical[0], kc.vy = cam->vertical[1], kc.vz = cam->vertical[2];
  kc.ux = cam->u[0], kc.uy = cam->u[1], kc.uz = cam->u[2];
  kc.bx = cam->v[0], kc.by = cam->v[1], kc.bz = cam->v[2];
  kc.lens = cam->lens_radius;
  kc.lens_s = ldexpf(kc.lens, -23);
  kc.lens_pre = std::isfinite(kc.lens) && ldexpf(kc.lens_s, 23) == kc.lens ? kCamLensPre : 0u;
  kc.dz = kc.lz - kc.pz;
  if (allow_axial && cam_axial(kc)) kc.lens_pre |= kCamAxial;
  return kc;
}

// A/B and tests: FR_CAM_GENERAL=1 sends every camera through cam_ray (read per frame)
static bool cam_general_forced() {
  const char* e = getenv("FR_CAM_GENERAL");
  return e && *e && strcmp(e, "0") != 0;
}

namespace fr {
KCam kcam_for_selftest(const fr_camera* cam) { return kcam(cam); }  // selftest.hip
}

extern "C" {

int fr_device_count(int* count) {
  if (!count) return set_error(FR_EARG, "null count");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    return set_error(FR_ENODEV, "hipGetDeviceCount: %s", hipGetErrorString(e));
  }
  *count = n;
  return FR_OK;
}

int fr_ctx_create(int device, void* stream, fr_ctx** out) {
  if (!out) return set_error(FR_EARG, "fr_ctx_create: null output");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return set_error(FR_ENODEV, "no HIP device");
  if (device < 0 || device >= n) return set_error(FR_ENODEV, "device %d not present (%d devices)", device, n);
  SET_DEVICE(device);
  fr_ctx* c = new fr_ctx();
  c->device = device;
  if (stream) {
    c->stream = static_cast<hipStream_t>(stream);
  } else {
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
      delete c;
      return set_error(FR_EHIP, "hipStreamCreate failed");
    }
    c->own_stream = true;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
    c->num_cus = prop.multiProcessorCount;
    c->device_bytes = prop.totalGlobalMem;
  }
  if (c->num_cus <= 0) c->num_cus = 256;
  bool ok = hipEventCreate(&c->ev0) == hipSuccess && hipEventCreate(&c->ev1) == hipSuccess &&
            hipEventCreateWithFlags(&c->ev_start, hipEventDisableTiming) == hipSuccess &&
            hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) == hipSuccess &&
            hipStreamCreateWithFlags(&c->stream_sum, hipStreamNonBlocking) == hipSuccess &&
            hipStreamCreateWithFlags(&c->stream_copy, hipStreamNonBlocking) == hipSuccess &&
            hipEventCreateWithFlags(&c->ev_copy, hipEventDisableTiming) == hipSuccess;
  for (int k = 0; ok && k < kFrameSlots; ++k)
    ok = hipEventCreateWithFlags(&c->ev_fslot[k], hipEventDisableTiming) == hipSuccess;
  // per-wave counters: one set per pass slot (traces of consecutive passes overlap)
  ok = ok && hipMalloc(&c->d_cnt, kFrameSlots * kCntWords * sizeof(unsigned long long)) == hipSuccess &&
       hipMalloc(&c->d_wcnt, kFrameSlots * 3 * sizeof(unsigned long long) * kMaxWgPerCu * (kBlock / 64u) *
                                 c->num_cus) == hipSuccess;
  if (!ok) {
    fr_ctx_free(c);
    return set_error(FR_EHIP, "fr_ctx_create: event/counter allocation failed");
  }
  *out = c;
  return FR_OK;
}

void fr_ctx_free(fr_ctx* c) {
  if (!c) return;
  int cur = -1;
  (void)hipGetDevice(&cur);
  (void)hipSetDevice(c->device);
  // every stream drained before any buffer or event it may still use goes
  for (hipStream_t s : {c->stream, c->stream2, c->stream_sum, c->stream_copy})
    if (s) (void)hipStreamSynchronize(s);
  // the scene kernels' launch events on this context's trace streams go before the streams do
  {
    const hipStream_t ts[2] = {c->stream, c->stream2};
    jit_forget_streams(ts, 2);
  }
  for (void* d : {static_cast<void*>(c->d_mean), static_cast<void*>(c->d_u8), static_cast<void*>(c->d_cnt),
                  static_cast<void*>(c->d_wcnt), static_cast<void*>(c->d_samples), static_cast<void*>(c->d_running),
                  static_cast<void*>(c->d_accum), static_cast<void*>(c->d_sq), static_cast<void*>(c->d_err),
                  static_cast<void*>(c->d_err_part), static_cast<void*>(c->d_err_sum), static_cast<void*>(c->d_nt),
                  static_cast<void*>(c->d_kt), static_cast<void*>(c->d_list), static_cast<void*>(c->d_tile_px),
                  static_cast<void*>(c->d_adapt_sum), static_cast<void*>(c->d_dn_ping),
                  static_cast<void*>(c->d_dn_pong), static_cast<void*>(c->d_dn_mean), static_cast<void*>(c->d_dn_u8),
                  static_cast<void*>(c->d_dn_var), static_cast<void*>(c->d_gb0), static_cast<void*>(c->d_gb1),
                  static_cast<void*>(c->d_gb_alb), static_cast<void*>(c->d_gb_cls), static_cast<void*>(c->d_tp_ta[0]),
                  static_cast<void*>(c->d_tp_ta[1]), static_cast<void*>(c->d_tp_tq[0]),
                  static_cast<void*>(c->d_tp_tq[1]), static_cast<void*>(c->d_tp_g0), static_cast<void*>(c->d_tp_g1),
                  static_cast<void*>(c->d_tp_pa), static_cast<void*>(c->d_tp_pq), static_cast<void*>(c->d_tp_src),
                  static_cast<void*>(c->d_tp_why), static_cast<void*>(c->d_cast_rays), static_cast<void*>(c->d_hit0),
                  static_cast<void*>(c->d_hit1), static_cast<void*>(c->d_hit_alb), static_cast<void*>(c->d_cast_waves),
                  static_cast<void*>(c->d_occl), static_cast<void*>(c->d_occl_waves)})
    if (d) (void)hipFree(d);
  if (c->h_cast_rays) (void)hipHostFree(c->h_cast_rays);
  for (hipEvent_t e : {c->ev0, c->ev1, c->ev_start, c->ev_copy, c->ev_cast})
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->ev_fslot)
    if (e) (void)hipEventDestroy(e);
  for (const std::vector<hipEvent_t>* v : {&c->ev_trace, &c->ev_sum, &c->log_ev[0], &c->log_ev[1], &c->log_ev[2],
                                             &c->log_ev[3]})
    for (hipEvent_t e : *v) (void)hipEventDestroy(e);
  for (hipStream_t s : {c->stream2, c->stream_sum, c->stream_copy})
    if (s) (void)hipStreamDestroy(s);
  if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  if (cur >= 0) (void)hipSetDevice(cur);  // the caller's current device (torch's) stays as it was
}

static int render_impl(fr_ctx* c, fr_scene* scene, const fr_camera* cam, const fr_params* p, bool dry);

int fr_ctx_render(fr_ctx* c, fr_scene* scene, const fr_camera* cam, const fr_params* p) {
  return render_impl(c, scene, cam, p, false);
}

int fr_ctx_prepare(fr_ctx* c, fr_scene* scene, const fr_camera* cam, const fr_params* p) {
  return render_impl(c, scene, cam, p, true);
}

// Enqueues a planned frame on frame slot fs: the slot's setup, then per pass the trace,
// the counter reduce and the sum, then the frame's end events. acc: an accumulating frame's
// resolve, which its last pass's sum runs (null: a plain frame).
static int enqueue_frame(fr_ctx* c, const DeviceCopy* dc, const FramePlan& fp, KArgs args, const SceneKernel& sk,
                         int fs, const SumAccum* acc) {
  unsigned long long* const cnt = c->d_cnt + kCntWords * fs;
  c->t0 = std::chrono::steady_clock::now();
  // The frame's setup (slot wait, counter clear, start events) goes on the stream its trace
  // runs on: with overlapping traces (stream2 every other frame) a setup on c->stream would
  // wait behind the previous frame's whole trace there, and so would this frame's trace.
  hipStream_t setup = c->stream;
  if (fp.fpipe && fp.fpipe_overlap && c->frame_parity) setup = c->stream2;
  // the last frame that used this slot's counters and samples (or, after a layout change,
  // every earlier frame) has been summed
  for (int k = 0; k < kFrameSlots; ++k)
    if (c->fslot_used[k] && (k == fs || fp.relayout)) HIPCHK(hipStreamWaitEvent(setup, c->ev_fslot[k], 0));
  c->fs_n = fp.nfs;
  c->fs_bytes = fp.slot_bytes;
  HIPCHK(hipMemsetAsync(cnt, 0, kCntWords * sizeof(unsigned long long), setup));
#ifdef FR_DIAG
  {
    const unsigned long long z[2] = {0, 0};
    HIPCHK(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_fr_diag_lens), z, sizeof(z), 0, hipMemcpyHostToDevice, setup));
    HIPCHK(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_fr_diag_rus), z, sizeof(z), 0, hipMemcpyHostToDevice, setup));
    void* tc = nullptr;
    HIPCHK(hipGetSymbolAddress(&tc, HIP_SYMBOL(g_fr_tb_cost)));
    HIPCHK(hipMemsetAsync(tc, 0, (1u << 20) * sizeof(unsigned int), setup));
  }
#endif
  HIPCHK(hipEventRecord(c->ev0, setup));
  if (c->log_on) HIPCHK(log_start(c, 1, setup));
  HIPCHK(hipEventRecord(c->ev_start, setup));
  if (setup != c->stream2) HIPCHK(hipStreamWaitEvent(c->stream2, c->ev_start, 0));
  HIPCHK(hipStreamWaitEvent(c->stream_sum, c->ev_start, 0));
  const PackedScene& ps = dc->ps;
  const uint32_t sum_blocks = (fp.kp.P + kSumThreads - 1u) / kSumThreads;
  // (BVH kernels with 8-B records store attenuation classes: the class table)
  const float4* sum_att =
      fp.bvh_nib ? reinterpret_cast<const float4*>(static_cast<const char*>(dc->blob) + ps.off_acls_att) : args.sc.att;
  const uint32_t sum_n = fp.bvh_nib ? ps.facts.n_aclass : ps.facts.n;
  bool jit_used = false;
  int traced = 0;  // trace launches whose events were recorded
  int summed = 0;
  for (int pass = 0; pass < fp.passes || (pass == 0 && fp.kp.P); ++pass) {
    const int slot = fp.fpipe ? fs : pass % 2;
    // one trace stream for pipelined frames: frame k+1's trace follows frame k's trace
    hipStream_t ts = fp.fpipe ? (fp.fpipe_overlap && c->frame_parity ? c->stream2 : c->stream)
                     : slot   ? c->stream2
                              : c->stream;
    float* samples = c->d_samples ? c->d_samples + static_cast<size_t>(slot) * (fp.slot_bytes / sizeof(float)) : nullptr;
    const PassPlan pp = pass_plan(fp, pass);
    KParams& kp = args.kp;
    kp.b0 = pp.b0, kp.nb = pp.nb, kp.n_items = pp.n_items, kp.n_coarse = pp.n_coarse, kp.b_fine = pp.b_fine;
    if (kp.n_items) {
      if (pass >= 2) HIPCHK(hipStreamWaitEvent(ts, c->ev_sum[pass - 2], 0));  // the slot's last reader is done
      unsigned long long* wcnt = c->d_wcnt + static_cast<size_t>(slot) * 3 * kMaxWgPerCu * (kBlock / 64u) * c->num_cus;
      args.kw.queue = reinterpret_cast<uint32_t*>(cnt + 31 - (fp.fpipe ? 0 : slot));
      args.kw.samples = samples;
      args.kw.wave_counters = wcnt;
      // a pipelined frame's queue head is cnt[31], cleared with its counters (before ev_start,
      // which stream2 waits for); passes of a multi-pass frame reuse two heads
      if (!fp.fpipe) HIPCHK(hipMemsetAsync(args.kw.queue, 0, sizeof(uint32_t), ts));
      HIPCHK(hipEventRecord(c->ev_trace[2 * traced], ts));
      if (c->log_on) HIPCHK(log_start(c, 0, ts));
      const Launched l = launch_trace(fp, c->num_cus, sk, ts, args);
      if (l.rc) return l.rc;
      c->occupancy = l.grid.per_cu;
      jit_used = sk.fn != nullptr;
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(c->ev_trace[2 * traced + 1], ts));
      if (c->log_on) HIPCHK(log_end(c, 0, ts));
      HIPCHK(hipStreamWaitEvent(c->stream_sum, c->ev_trace[2 * traced + 1], 0));
      // on the sum stream, after the trace: the frame's end (ev1 on c->stream) waits for
      // the sums, so fr_ctx_sync reads d_cnt after every pass's reduce, and the next
      // frame's d_cnt memset (c->stream) cannot overtake a reduce of this one
      hipLaunchKernelGGL(reduce_counters, dim3(1), dim3(256), 0, c->stream_sum, wcnt, l.grid.blocks * (kBlock / 64u),
                         cnt);
      HIPCHK(hipGetLastError());
      ++traced;
    }
    const int first = pass == 0, last = pass + 1 >= fp.passes;
    if (first && c->copy_pending) HIPCHK(hipStreamWaitEvent(c->stream_sum, c->ev_copy, 0));  // last gather done
    HIPCHK(launch_sum(fp.wps, sum_blocks ? sum_blocks : 1u, c->stream_sum, kp, samples, c->d_running,
                      c->d_mean, c->d_u8, first, last, sum_att, sum_n, acc));
    HIPCHK(hipEventRecord(c->ev_sum[pass], c->stream_sum));
    summed = pass + 1;
    if (last) break;
  }
  // frame end: on the context's stream (the next frame's trace waits for this one's sums),
  // or, pipelined, on the sum stream (the next frame's trace starts when this trace ends)
  hipStream_t end_stream = c->stream;
  if (fp.fpipe)
    end_stream = c->stream_sum;
  else if (summed)
    HIPCHK(hipStreamWaitEvent(c->stream, c->ev_sum[summed - 1], 0));
  HIPCHK(hipEventRecord(c->ev_fslot[fs], end_stream));
  c->fslot_used[fs] = true;
  c->last_cnt = cnt;
  if (fp.fpipe) {
    c->frame_slot = (fs + 1) % fp.nfs;
    c->frame_parity ^= 1;
  }
  c->passes = traced;
  c->jit_used = jit_used;
  HIPCHK(hipEventRecord(c->ev1, end_stream));
  if (c->log_on) HIPCHK(log_end(c, 1, end_stream));
  return FR_OK;
}

// dry (fr_ctx_prepare): everything a render of these parameters sets up before its first
// launch — the scene's device copy, the output and sample buffers, the scene-specialised
// kernel when asked for — and nothing enqueued.
static int render_impl(fr_ctx* c, fr_scene* scene, const fr_camera* cam, const fr_params* p, bool dry) {
  if (!c || !scene || !cam) return set_error(FR_EARG, "fr_ctx_render: null argument");
  int rc = check_params(p);
  if (rc) return rc;
  SET_DEVICE(c->device);
  const PlanEnv env = read_plan_env();
  DeviceCopy* dc = nullptr;
  if ((rc = ctx_scene(c, scene, env.bvh_force, &dc))) return rc;
  const size_t pixels = static_cast<size_t>(p->width) * p->height;
  if (pixels * 3 * sizeof(float) > c->cap_mean && c->copy_pending)
    HIPCHK(hipStreamSynchronize(c->stream_copy));  // a gather still reads them
  if ((rc = grow(c->d_mean, c->cap_mean, pixels * 3 * sizeof(float)))) return rc;
  if ((rc = grow(c->d_u8, c->cap_u8, pixels * 3))) return rc;
  // The previous frame of this context still running (its end event pending): frames are
  // being streamed, and this trace shares the CUs with the previous frame's trace or sum
  const bool prev_in_flight = !dry && c->pending && hipEventQuery(c->ev1) == hipErrorNotReady;
  // an adaptive frame (FR_FLAG_ADAPTIVE) is planned over the context's active tile list; it
  // fails, or with an empty list ends, here, before anything is enqueued. A dry run plans the
  // whole shard (the list's upper bound) and reads no state.
  const bool adaptive = !dry && (p->flags & FR_FLAG_ADAPTIVE) != 0;
  if (adaptive) {
    AdaptiveFrame af;
    if ((rc = adaptive_step(c->accum, c->tiled, accum_key(dc->uid, *cam, *p), &af))) return rc;
    if (af == AdaptiveFrame::kEmpty) {  // nothing to trace: outputs, A, Q, counts and totals stay
      c->last = *p;
      c->last_adaptive = c->last_empty = true;
      c->last_active_pixels = 0;
      return FR_OK;
    }
  }
  FramePlan fp;
  if ((rc = make_plan(*p, camera_reach(*cam), dc->ps.facts, c->num_cus, c->device_bytes, env, dry,
                      PlanHistory{prev_in_flight, c->streaming, c->fs_n, c->fs_bytes}, &fp,
                      adaptive ? &c->tiled.active_tiles : nullptr)))
    return rc;
  if (adaptive) fp.kp.tile_list = c->d_list, fp.kp.flags |= KF_LIST;
  if (!dry) c->streaming = prev_in_flight;
  if (fp.relayout) c->frame_slot = 0;
  const int fs = fp.fpipe ? c->frame_slot % fp.nfs : 0;
  if ((rc = grow(c->d_samples, c->cap_samples, fp.slot_bytes * fp.slots))) return rc;
  if (fp.passes > 1 && (rc = grow(c->d_running, c->cap_running, fp.running_bytes))) return rc;
  // an accumulating frame (the flag is not in the plan: plan.h): continue or restart is
  // decided, and may fail, before anything is enqueued; the state moves once the frame is
  const bool accumulate = (p->flags & FR_FLAG_ACCUMULATE) != 0;
  AccumStep step;
  SumAccum acc;
  if (accumulate) {
    const bool with_q = (p->flags & FR_FLAG_ACCUM_ERROR) != 0;
    if ((rc = grow_accum(c, fp.running_bytes ? fp.running_bytes : 1u, with_q))) return rc;
    if (!dry && (rc = accum_step(c->accum, accum_key(dc->uid, *cam, *p), p->spp, &step))) return rc;
    acc = SumAccum{c->d_accum, step.start, static_cast<float>(step.next.samples), with_q ? c->d_sq : nullptr};
    // a tiled accumulation goes on: the resolve takes each tile's own divisor and advances its counts
    if (!dry && !step.start && c->tiled.tiled) acc.n_t = c->d_nt, acc.k_t = c->d_kt;
  }
  const size_t n_ev = static_cast<size_t>(fp.passes > 0 ? fp.passes : 1);
  if ((rc = grow_events(c->ev_sum, n_ev, hipEventDisableTiming))) return rc;
  if ((rc = grow_events(c->ev_trace, 2 * n_ev, hipEventDefault))) return rc;
  KWork kw{};
  kw.counters = c->d_cnt + kCntWords * fs;
  SceneKernel sk;
  if ((rc = find_scene_kernel(c, dc, fp, &sk))) return rc;
  const KCam kc = kcam(cam, !cam_general_forced());
  c->cam_axial = (kc.lens_pre & kCamAxial) != 0;
  if (dry) {
    c->jit_used = sk.fn != nullptr;
  } else {
    if ((rc = enqueue_frame(c, dc, fp, KArgs{kscene(dc, fp), kc, fp.kp, kw}, sk, fs,
                            accumulate ? &acc : nullptr)))
      return rc;
    if (accumulate) {
      c->accum = step.next;
      if (!adaptive) c->accum_kp = fp.kp;  // the whole shard's constants (an adaptive frame's are its list's)
      if (step.start) c->tiled = TiledState{};  // a new accumulation is uniform: counts and list are dead
      if (step.start) ++c->accum_gen;           // (fr_ctx_temporal reprojects once per generation)
    }
    c->last_adaptive = adaptive;
    c->last_empty = false;
    c->last_active_pixels = adaptive ? c->tiled.active_pixels : 0;
    c->last = *p;
    c->last_n = dc->ps.facts.n;
    c->pending = true;
  }
  c->jit_stats = sk.stats;
  c->jit_state = sk.state;
  return FR_OK;
}

int fr_ctx_sync(fr_ctx* c, fr_stats* st) {
  if (!c) return set_error(FR_EARG, "fr_ctx_sync: null ctx");
  SET_DEVICE(c->device);
  HIPCHK(hipStreamSynchronize(c->stream));
  if (!c->pending) return set_error(FR_EARG, "fr_ctx_sync: nothing rendered");
  HIPCHK(hipEventSynchronize(c->ev1));  // the frame's end (on the sum stream when pipelined)
  if (st && c->last_empty) {  // an adaptive frame with an empty list: nothing was traced
    memset(st, 0, sizeof(*st));
    return FR_OK;
  }
  if (st) {
    unsigned long long cnt[kCntWords] = {};
    HIPCHK(hipMemcpy(cnt, c->last_cnt, sizeof(cnt), hipMemcpyDeviceToHost));
#ifdef FR_PROF
    {
      double tot = 0;
      for (int k = 0; k < PF_N; ++k) tot += static_cast<double>(cnt[20 + k]);
      fprintf(stderr, "FR_PROF {\"claim\": %.4f, \"reject\": %.4f, \"hit\": %.4f, \"shade\": %.4f, \"end\": %.4f, "
              "\"wave_cycles\": %.4e}\n", cnt[20] / tot, cnt[21] / tot, cnt[22] / tot, cnt[23] / tot, cnt[24] / tot, tot);
    }
#endif
#ifdef FR_SECCNT
    fprintf(stderr, "FR_SECCNT [");
    for (int k = 0; k < SC_N; ++k) fprintf(stderr, k ? ", %llu" : "%llu", cnt[4 + k]);
    fprintf(stderr, "]\nFR_SECLANES [");
    for (int k = 0; k < SC_N; ++k) fprintf(stderr, k ? ", %llu" : "%llu", cnt[32 + k]);
    fprintf(stderr, "]\n");
#endif
#ifdef FR_DIAG
    unsigned long long dl[2], dr[2];
    HIPCHK(hipMemcpyFromSymbol(dl, HIP_SYMBOL(g_fr_diag_lens), sizeof(dl)));
    HIPCHK(hipMemcpyFromSymbol(dr, HIP_SYMBOL(g_fr_diag_rus), sizeof(dr)));
    fprintf(stderr,
            "FR_DIAG {\"iter_w\": %llu, \"regen_w\": %llu, \"regen_l\": %llu, \"hit_w\": %llu, \"end_w\": %llu, "
            "\"end_l\": %llu, \"unwind_w\": %llu, \"unwind_l\": %llu, \"lens_w\": %llu, \"lens_l\": %llu, "
            "\"rus_w\": %llu, \"rus_l\": %llu, \"merged_w\": %llu, \"merged_l\": %llu, \"segments\": %llu, "
            "\"hits\": %llu, \"node_w\": %llu, \"node_l\": %llu, \"leaf_w\": %llu, \"leaf_l\": %llu, "
            "\"node_coh_w\": %llu, \"node_u2_w\": %llu, \"node_u34_w\": %llu, \"node_primary_l\": %llu}\n",
            cnt[4 + DG_ITER], cnt[4 + DG_REGEN_W], cnt[4 + DG_REGEN_L], cnt[4 + DG_HIT_W], cnt[4 + DG_END_W],
            cnt[4 + DG_END_L], cnt[4 + DG_UNW_W], cnt[4 + DG_UNW_L], dl[0], dl[1], dr[0], dr[1], cnt[4 + DG_LENS_W],
            cnt[4 + DG_LENS_L], cnt[0], cnt[1], cnt[4 + DG_NODE_W], cnt[4 + DG_NODE_L], cnt[4 + DG_LEAF_W],
            cnt[4 + DG_LEAF_L], cnt[4 + DG_NCOH_W], cnt[4 + DG_NU2_W], cnt[4 + DG_NU4_W], cnt[4 + DG_NPRIM_L]);
    if (const char* path = getenv("FR_DIAG_COST")) {
      std::vector<unsigned int> tc(1u << 20);
      HIPCHK(hipMemcpyFromSymbol(tc.data(), HIP_SYMBOL(g_fr_tb_cost), tc.size() * 4));
      if (FILE* f = fopen(path, "wb")) {
        fwrite(tc.data(), 4, tc.size(), f);
        fclose(f);
      }
    }
    if (const char* path = getenv("FR_DIAG_TIMES")) {
      std::vector<unsigned long long> wt(2 * 65536);
      HIPCHK(hipMemcpyFromSymbol(wt.data(), HIP_SYMBOL(g_fr_wave_times), wt.size() * 8));
      std::vector<unsigned long long> wd(65536);
      HIPCHK(hipMemcpyFromSymbol(wd.data(), HIP_SYMBOL(g_fr_wave_drain), wd.size() * 8));
      wt.insert(wt.end(), wd.begin(), wd.end());
      if (const char* pi = getenv("FR_DIAG_ITERS")) {
        std::vector<unsigned long long> ti(1024 * 1024);
        HIPCHK(hipMemcpyFromSymbol(ti.data(), HIP_SYMBOL(g_fr_iter_times), ti.size() * 8));
        if (FILE* f = fopen(pi, "wb")) {
          fwrite(ti.data(), 8, ti.size(), f);
          fclose(f);
        }
      }
      std::vector<unsigned int> wi(2 * 65536);
      HIPCHK(hipMemcpyFromSymbol(wi.data(), HIP_SYMBOL(g_fr_wave_iters), wi.size() * 4));
      for (size_t k = 0; k < wi.size(); k += 2) wt.push_back((static_cast<unsigned long long>(wi[k + 1]) << 32) | wi[k]);
      if (FILE* f = fopen(path, "wb")) {
        fwrite(wt.data(), 8, wt.size(), f);
        fclose(f);
      }
    }
#endif
    float ms = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
    const fr_params& p = c->last;
    const ShardStrips ss = shard_strips(p.height, p.shard_index, p.shard_count, (p.flags & FR_FLAG_MT_BANDS) != 0);
    st->segments = cnt[0];
    st->hits = cnt[1];
    st->samples = (c->last_adaptive ? c->last_active_pixels : ss.rows * p.width) * static_cast<uint64_t>(p.spp);
    st->prim_tests = cnt[0] * static_cast<uint64_t>(c->last_n);
    st->kernel_ms = ms;
    double tms = 0.0;
    for (int i = 0; i < c->passes; ++i) {
      float t = 0.0f;
      HIPCHK(hipEventElapsedTime(&t, c->ev_trace[2 * i], c->ev_trace[2 * i + 1]));
      tms += t;
    }
    st->trace_ms = tms;
    st->trace_launches = static_cast<uint32_t>(c->passes);
    st->occupancy = static_cast<uint32_t>(c->occupancy);
    // every path traces one segment more than it scatters (tracer.rs:189-210: each scatter
    // is followed by one more get_color), so the kernel counts segments and hits only
    st->scatters = cnt[0] - (c->last_adaptive ? c->last_active_pixels : ss.traced_rows * p.width) * static_cast<uint64_t>(p.spp);
    st->total_ms =
        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c->t0).count();
  }
  return FR_OK;
}

// Enqueues the D2H copies of this shard's rows of the last render on `st`.
static int enqueue_download(fr_ctx* c, hipStream_t st, float* mean_rgb, uint8_t* rgb8) {
  const fr_params& p = c->last;
  const size_t row_f = static_cast<size_t>(p.width) * 3;  // elements per row
  if (p.shard_count == 1) {  // the whole image: one contiguous copy per output
    const size_t n = static_cast<size_t>(p.height) * row_f;
    if (mean_rgb) HIPCHK(hipMemcpyAsync(mean_rgb, c->d_mean, n * 4, hipMemcpyDeviceToHost, st));
    if (rgb8) HIPCHK(hipMemcpyAsync(rgb8, c->d_u8, n, hipMemcpyDeviceToHost, st));
    return FR_OK;
  }
  // full strips of this shard form a strided 2-D region; the trailing partial strip is separate
  const ShardStrips ss = shard_strips(p.height, p.shard_index, p.shard_count, false);
  const size_t first = static_cast<size_t>(p.shard_index) * kStripRows * row_f;
  const size_t pitch = static_cast<size_t>(p.shard_count) * kStripRows * row_f;
  const size_t width = kStripRows * row_f;
  const size_t o = static_cast<size_t>(ss.partial) * kStripRows * row_f;        // the partial strip's offset
  const size_t o_n = (p.height - ss.partial * kStripRows) * row_f;              // and its elements
  if (mean_rgb) {
    if (ss.full)
      HIPCHK(hipMemcpy2DAsync(mean_rgb + first, pitch * 4, c->d_mean + first, pitch * 4, width * 4, ss.full,
                              hipMemcpyDeviceToHost, st));
    if (ss.has_partial) HIPCHK(hipMemcpyAsync(mean_rgb + o, c->d_mean + o, o_n * 4, hipMemcpyDeviceToHost, st));
  }
  if (rgb8) {
    if (ss.full)
      HIPCHK(hipMemcpy2DAsync(rgb8 + first, pitch, c->d_u8 + first, pitch, width, ss.full, hipMemcpyDeviceToHost, st));
    if (ss.has_partial) HIPCHK(hipMemcpyAsync(rgb8 + o, c->d_u8 + o, o_n, hipMemcpyDeviceToHost, st));
  }
  return FR_OK;
}

int fr_ctx_download(fr_ctx* c, float* mean_rgb, uint8_t* rgb8) {
  if (!c || !c->pending) return set_error(FR_EARG, "fr_ctx_download: nothing rendered");
  SET_DEVICE(c->device);
  HIPCHK(hipStreamWaitEvent(c->stream, c->ev1, 0));  // the last render's end (its sums)
  const int rc = enqueue_download(c, c->stream, mean_rgb, rgb8);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  return FR_OK;
}

int fr_ctx_download_async(fr_ctx* c, float* mean_rgb, uint8_t* rgb8) {
  if (!c || !c->pending) return set_error(FR_EARG, "fr_ctx_download_async: nothing rendered");
  SET_DEVICE(c->device);
  HIPCHK(hipStreamWaitEvent(c->stream_copy, c->ev1, 0));  // after the last render's sum
  const int rc = enqueue_download(c, c->stream_copy, mean_rgb, rgb8);
  if (rc) return rc;
  HIPCHK(hipEventRecord(c->ev_copy, c->stream_copy));
  c->copy_pending = true;
  return FR_OK;
}

int fr_ctx_wait(fr_ctx* c) {
  if (!c) return set_error(FR_EARG, "fr_ctx_wait: null ctx");
  SET_DEVICE(c->device);
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipStreamSynchronize(c->stream2));
  HIPCHK(hipStreamSynchronize(c->stream_sum));
  HIPCHK(hipStreamSynchronize(c->stream_copy));
  return FR_OK;
}

int fr_host_alloc(size_t bytes, void** out) {
  if (!out) return set_error(FR_EARG, "fr_host_alloc: null output");
  *out = nullptr;
  if (hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess || !*out)
    return set_error(FR_ENOMEM, "hipHostMalloc(%zu) failed", bytes);
  return FR_OK;
}

void fr_host_free(void* p) {
  if (p) (void)hipHostFree(p);
}

int fr_ctx_device_buffers(fr_ctx* c, float** d_mean, uint8_t** d_u8) {
  if (!c) return set_error(FR_EARG, "fr_ctx_device_buffers: null ctx");
  if (d_mean) *d_mean = c->d_mean;
  if (d_u8) *d_u8 = c->d_u8;
  return FR_OK;
}

int fr_render_hip(fr_scene* scene, const fr_camera* cam, const fr_params* params, int device, float* mean_rgb,
                  uint8_t* rgb8, fr_stats* stats) {
  if (params && (params->flags & FR_FLAG_ACCUMULATE))
    return set_error(FR_EARG,
                     "fr_render_hip: FR_FLAG_ACCUMULATE needs a context that outlives the call (fr_ctx_render)");
  fr_ctx* c = nullptr;
  int rc = fr_ctx_create(device, nullptr, &c);
  if (rc) return rc;
  fr_params p = *params;
  if (rgb8) p.flags |= FR_FLAG_WRITE_U8;
  rc = fr_ctx_render(c, scene, cam, &p);
  if (!rc) rc = fr_ctx_sync(c, stats);
  if (!rc) rc = fr_ctx_download(c, mean_rgb, rgb8);
  fr_ctx_free(c);
  return rc;
}

// Test hook, no device needed: the run-time build of the headline specialisation (all
// boxes, <= 15 primitives, diffuse, depth <= 8) for `n` 64-B records compiles for `arch`.
// targs: the 8 template arguments of another specialisation (NULL: the headline's).
int fr_selftest_jit(const char* arch, const uint32_t* rec, uint32_t n, const int* targs_in, size_t* code_bytes,
                    double* ms) {
  if (!arch || !rec || n == 0 || n > kJitMaxPrims) return set_error(FR_EARG, "fr_selftest_jit: bad arguments");
  KernelId id{{KS_AABB, 0, FR_KREJ_NIB, static_cast<int>(kSmallDepth), 0, 0, 2, 1}, ""};
  if (targs_in) memcpy(id.targs, targs_in, sizeof id.targs);
  id.name = kernel_name(id.targs);
  return jit_compile_probe(arch, jit_spec(id, rec, n), code_bytes, ms);
}

int fr_ctx_jit_info(fr_ctx* c, int* used, double* ms, int* compiled) {
  if (!c) return set_error(FR_EARG, "fr_ctx_jit_info: null ctx");
  if (used) *used = c->jit_used ? 1 : 0;
  if (ms) *ms = c->jit_state != FR_JIT_OFF ? c->jit_stats.ms : 0.0;
  if (compiled) *compiled = c->jit_state != FR_JIT_OFF ? c->jit_stats.compiled : 0;
  return FR_OK;
}

int fr_ctx_jit_state(fr_ctx* c, int* state) {
  if (!c || !state) return set_error(FR_EARG, "fr_ctx_jit_state: null argument");
  *state = c->jit_state;
  if (c->jit_state == FR_JIT_FAILED) set_error(FR_EHIP, "%s", c->jit_stats.error.c_str());
  return FR_OK;
}

int fr_jit_wait(void) { return jit_wait_all(); }

int fr_camera_axial(const fr_camera* cam) {
  if (!cam) return set_error(FR_EARG, "fr_camera_axial: null camera");
  return (kcam(cam).lens_pre & kCamAxial) ? 1 : 0;
}

int fr_ctx_camera_path(fr_ctx* c, int* axial) {
  if (!c || !axial) return set_error(FR_EARG, "fr_ctx_camera_path: null argument");
  *axial = c->cam_axial ? 1 : 0;
  return FR_OK;
}

int fr_ctx_accum_reset(fr_ctx* c) {
  if (!c) return set_error(FR_EARG, "fr_ctx_accum_reset: null ctx");
  c->accum = AccumState{};  // (host state only: the next accumulating frame's sum overwrites A)
  c->tiled = TiledState{};  // the counts and the tile list die with the accumulation
  return FR_OK;
}

int fr_ctx_accum_info(fr_ctx* c, uint32_t* frames, uint32_t* samples) {
  if (!c) return set_error(FR_EARG, "fr_ctx_accum_info: null ctx");
  if (frames) *frames = c->accum.live ? c->accum.frames : 0u;
  if (samples) *samples = c->accum.live ? c->accum.samples : 0u;
  return FR_OK;
}

// The error estimate on demand. Both kernels and the summary's copy go on
// the sum stream, behind the resolve of every frame enqueued so far (each of them is there),
// and only that stream is waited for: the pending render's events, counters and stats, A and Q
// stay as they are.
int fr_ctx_accum_error(fr_ctx* c, float threshold, fr_accum_error* out) {
  if (!c || !out) return set_error(FR_EARG, "fr_ctx_accum_error: null argument");
  if (!(threshold >= 0.0f))
    return set_error(FR_EARG, "fr_ctx_accum_error: threshold %g must be >= 0 (+infinity counts every pixel)",
                     static_cast<double>(threshold));
  const AccumState& a = c->accum;
  if (!a.live) return set_error(FR_EARG, "fr_ctx_accum_error: no live accumulation (no FR_FLAG_ACCUMULATE frame yet, or reset)");
  if (!a.has_q || !c->d_sq)
    return set_error(FR_EARG, "fr_ctx_accum_error: the live accumulation carries no Q: its frames lack FR_FLAG_ACCUM_ERROR");
  if (a.frames < 2)
    return set_error(FR_EARG, "fr_ctx_accum_error: %u frame in the accumulation, the estimate needs two", a.frames);
  SET_DEVICE(c->device);
  const KParams& kp = c->accum_kp;
  const uint32_t groups = (kp.P + kSumThreads - 1u) / kSumThreads;
  int rc;
  // (a larger map: the sum stream is idle after the last call's wait, nothing reads the old one)
  if ((rc = grow(c->d_err, c->cap_err, static_cast<size_t>(kp.W) * kp.H * sizeof(float)))) return rc;
  if ((rc = grow(c->d_err_part, c->cap_err_part, (groups ? groups : 1u) * 2u * sizeof(uint32_t)))) return rc;
  if (!c->d_err_sum) HIPCHK(hipMalloc(&c->d_err_sum, sizeof(ErrSummary)));
  c->err_valid = false;
  if (c->tiled.tiled)  // per-tile n_t and K_t (frames and samples below stay the host's totals)
    HIPCHK(launch_adapt(c->stream_sum, kp, c->d_accum, c->d_sq, c->d_nt, c->d_kt, threshold, 0u, c->d_err,
                        c->d_err_part, nullptr, nullptr, nullptr, c->d_err_sum));
  else
    HIPCHK(launch_accum_error(c->stream_sum, kp, c->d_accum, c->d_sq, static_cast<float>(a.samples),
                              static_cast<float>(a.frames - 1u), threshold, c->d_err, c->d_err_part, c->d_err_sum));
  ErrSummary sum{};
  HIPCHK(hipMemcpyAsync(&sum, c->d_err_sum, sizeof(sum), hipMemcpyDeviceToHost, c->stream_sum));
  HIPCHK(hipStreamSynchronize(c->stream_sum));
  c->err_kp = kp;
  c->err_valid = true;
  const ShardStrips ss = shard_strips(kp.H, kp.shard_index, kp.shard_count, false);
  out->frames = a.frames;
  out->samples = a.samples;
  out->pixels = ss.rows * kp.W;
  out->converged = sum.converged;
  memcpy(&out->max_rel, &sum.max_bits, sizeof(float));
  out->threshold = threshold;
  return FR_OK;
}

// The selection: like fr_ctx_accum_error on the sum stream, behind every
// enqueued resolve, and waited for there alone. Each frame's sum follows its trace, so every
// enqueued trace, the readers of the previous list, has finished when the select kernel runs.
int fr_ctx_adapt(fr_ctx* c, float threshold, uint32_t min_samples, fr_adapt_info* out) {
  if (!c || !out) return set_error(FR_EARG, "fr_ctx_adapt: null argument");
  if (!(threshold >= 0.0f))
    return set_error(FR_EARG, "fr_ctx_adapt: threshold %g must be >= 0 (+infinity selects by min_samples alone)",
                     static_cast<double>(threshold));
  const AccumState& a = c->accum;
  if (!a.live) return set_error(FR_EARG, "fr_ctx_adapt: no live accumulation (no FR_FLAG_ACCUMULATE frame yet, or reset)");
  if (!a.has_q || !c->d_sq)
    return set_error(FR_EARG, "fr_ctx_adapt: the live accumulation carries no Q: its frames lack FR_FLAG_ACCUM_ERROR");
  if (a.frames < 2)
    return set_error(FR_EARG, "fr_ctx_adapt: %u frame in the accumulation, the estimate needs two", a.frames);
  SET_DEVICE(c->device);
  const KParams& kp = c->accum_kp;
  const uint32_t groups = (kp.P + kSumThreads - 1u) / kSumThreads;
  const size_t tile_bytes = (kp.n_tiles ? kp.n_tiles : 1u) * sizeof(uint32_t);
  int rc;
  if ((rc = grow(c->d_err, c->cap_err, static_cast<size_t>(kp.W) * kp.H * sizeof(float)))) return rc;
  if ((rc = grow(c->d_err_part, c->cap_err_part, (groups ? groups : 1u) * 2u * sizeof(uint32_t)))) return rc;
  if ((rc = grow(c->d_tile_px, c->cap_tile_px, tile_bytes))) return rc;
  if (!c->d_adapt_sum) HIPCHK(hipMalloc(&c->d_adapt_sum, sizeof(AdaptSummary)));
  if (!c->tiled.tiled) {
    // the accumulation becomes tiled: every tile starts from the uniform (n, K). The arrays
    // may be an earlier, dead accumulation's: its resolves, their last users, are on the sum
    // stream, which is drained before a larger pair replaces them.
    HIPCHK(hipStreamSynchronize(c->stream_sum));
    if ((rc = grow(c->d_nt, c->cap_nt, tile_bytes))) return rc;
    if ((rc = grow(c->d_kt, c->cap_kt, tile_bytes))) return rc;
    HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c->d_nt), static_cast<int>(a.samples), kp.n_tiles,
                             c->stream_sum));
    HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c->d_kt), static_cast<int>(a.frames), kp.n_tiles,
                             c->stream_sum));
  }
  // The previous list is overwritten in place. Its readers are the traces and sums of the
  // adaptive frames enqueued so far: the sums are ahead of the select kernel on the sum stream,
  // and each trace has finished before its frame's sum starts. (A larger list is a new
  // allocation: the stream is drained first.)
  if (c->cap_list < tile_bytes) HIPCHK(hipStreamSynchronize(c->stream_sum));
  if ((rc = grow(c->d_list, c->cap_list, tile_bytes))) return rc;
  c->err_valid = false;
  HIPCHK(launch_adapt(c->stream_sum, kp, c->d_accum, c->d_sq, c->d_nt, c->d_kt, threshold, min_samples, c->d_err,
                      c->d_err_part, c->d_tile_px, c->d_list, c->d_adapt_sum, nullptr));
  AdaptSummary sum{};
  HIPCHK(hipMemcpyAsync(&sum, c->d_adapt_sum, sizeof(sum), hipMemcpyDeviceToHost, c->stream_sum));
  HIPCHK(hipStreamSynchronize(c->stream_sum));
  c->err_kp = kp;
  c->err_valid = true;
  c->tiled.tiled = true;
  c->tiled.tiles = kp.n_tiles;
  c->tiled.active_tiles = sum.active_tiles;
  c->tiled.active_pixels = sum.active_pixels;
  const ShardStrips ss = shard_strips(kp.H, kp.shard_index, kp.shard_count, false);
  memset(out, 0, sizeof(*out));
  out->frames = a.frames;
  out->samples = a.samples;
  out->tiles = kp.n_tiles;  // (every tile of a shard starts inside the image)
  out->active_tiles = sum.active_tiles;
  out->pixels = ss.rows * kp.W;
  out->active_pixels = sum.active_pixels;
  out->converged = sum.converged;
  memcpy(&out->max_rel, &sum.max_bits, sizeof(float));
  out->threshold = threshold;
  out->min_samples = min_samples;
  return FR_OK;
}

// What fr_ctx_denoise and fr_ctx_denoise_guided (`who`) refuse alike, before anything is enqueued.
static int denoise_refusal(const fr_ctx* c, const char* who, uint32_t levels, float k) {
  if (levels < 1u || levels > kDnLevelsMax)
    return set_error(FR_EARG, "%s: levels %u must be 1 to %u", who, levels, kDnLevelsMax);
  if (!(k > 0.0f && k <= kDnKMax))
    return set_error(FR_EARG, "%s: k %g must be finite, > 0 and <= %g", who, static_cast<double>(k),
                     static_cast<double>(kDnKMax));
  const AccumState& a = c->accum;
  if (!a.live) return set_error(FR_EARG, "%s: no live accumulation (no FR_FLAG_ACCUMULATE frame yet, or reset)", who);
  if (!a.has_q || !c->d_sq)
    return set_error(FR_EARG, "%s: the live accumulation carries no Q: its frames lack FR_FLAG_ACCUM_ERROR", who);
  if (a.frames < 2)
    return set_error(FR_EARG, "%s: %u frame in the accumulation, the variance needs two", who, a.frames);
  if (c->accum_kp.shard_count != 1)
    return set_error(FR_EARG, "%s: shard_count %u: the filter's taps cross the strips of other shards, "
                              "only a whole image (shard_count 1) is filtered", who, c->accum_kp.shard_count);
  return FR_OK;
}

// The ping and pong buffers and the three outputs at the live accumulation's size.
static int denoise_buffers(fr_ctx* c) {
  const KParams& kp = c->accum_kp;
  if (c->dn_w != kp.W || c->dn_h != kp.H || !c->d_dn_var) {
    // another size: the kernels and copies that use the old buffers are on the sum stream
    HIPCHK(hipStreamSynchronize(c->stream_sum));
    c->dn_valid = false;
    c->dn_w = c->dn_h = 0;
    const size_t px = static_cast<size_t>(kp.W) * kp.H;
    size_t caps[5] = {};  // (grow with no capacity: each buffer is replaced)
    int rc;
    if ((rc = grow(c->d_dn_ping, caps[0], px * sizeof(DnPixel)))) return rc;
    if ((rc = grow(c->d_dn_pong, caps[1], px * sizeof(DnPixel)))) return rc;
    if ((rc = grow(c->d_dn_mean, caps[2], px * 3 * sizeof(float)))) return rc;
    if ((rc = grow(c->d_dn_u8, caps[3], px * 3))) return rc;
    if ((rc = grow(c->d_dn_var, caps[4], px * sizeof(float)))) return rc;
    c->dn_w = kp.W;
    c->dn_h = kp.H;
  }
  return FR_OK;
}

// The filter on demand. Like fr_ctx_accum_error's kernels, prep and the levels
// go on the sum stream, behind the resolve of every frame enqueued so far and ahead of every
// later one; unlike it nothing is waited for. A, Q, the counts, d_mean, d_u8, the pending
// render and its stats are read or untouched: the results have buffers of their own.
int fr_ctx_denoise(fr_ctx* c, uint32_t levels, float k) {
  if (!c) return set_error(FR_EARG, "fr_ctx_denoise: null ctx");
  int rc;
  if ((rc = denoise_refusal(c, "fr_ctx_denoise", levels, k))) return rc;
  SET_DEVICE(c->device);
  if ((rc = denoise_buffers(c))) return rc;
  const AccumState& a = c->accum;
  const bool tiled = c->tiled.tiled;
  HIPCHK(launch_denoise(c->stream_sum, c->accum_kp, c->d_accum, c->d_sq, tiled ? c->d_nt : nullptr,
                        tiled ? c->d_kt : nullptr, a.samples, a.frames, levels, k, c->d_dn_ping, c->d_dn_pong,
                        c->d_dn_mean, c->d_dn_u8, c->d_dn_var));
  c->dn_valid = true;
  return FR_OK;
}

// fr_ctx_gbuffer's default walk for a scene with a tree, by the rule of DESIGN.md §5: the tree,
// because at 1080p on 10,000 spheres no pixel differed from the list pass and the tree pass's
// median was below the list pass's minimum (profiles/gbuffer_tree_1080p.json).
constexpr bool kGbTreeDefault = true;

// The tables of a scene's device copy as the cast and G-buffer walks read them (cast.h).
static CastScene cast_scene(const DeviceCopy* dc) {
  const PackedScene& ps = dc->ps;
  const char* b = static_cast<const char*>(dc->blob);
  CastScene cs;
  cs.gb.rec = reinterpret_cast<const float4*>(b + ps.off_rec);
  cs.gb.runs = reinterpret_cast<const uint4*>(b + ps.off_runs);
  cs.gb.cls = reinterpret_cast<const uint32_t*>(b + ps.off_cls);
  cs.gb.att = reinterpret_cast<const float4*>(b + ps.off_att);
  cs.gb.n_runs = ps.n_runs;
  cs.gb.n = ps.facts.n;
  cs.bvh = reinterpret_cast<const float4*>(b + ps.off_bvh);
  cs.bvh_order = reinterpret_cast<const uint32_t*>(b + ps.off_bvh_order);
  cs.lrec = reinterpret_cast<const float4*>(b + ps.off_lrec);
  cs.segs = reinterpret_cast<const uint4*>(b + ps.off_segs);
  cs.n_segs = ps.facts.bvh_ok ? ps.facts.n_segs : 0u;
  cs.levels = ps.facts.bvh_levels;
  cs.reach = bvh_origin_reach(ps.facts.bvh_extent, ps.facts.bvh_sphere_rmin);
  return cs;
}

// What this context's last use of `scene` did to the scene's copy on its device, and the copy's
// running counts. The device times of a refit read -1 while it is pending.
int fr_ctx_scene_info(fr_ctx* c, fr_scene* scene, fr_scene_info* out) {
  if (!c || !scene || !out) return set_error(FR_EARG, "fr_ctx_scene_info: null argument");
  SET_DEVICE(c->device);
  std::lock_guard<std::mutex> g(scene->mu);
  const DeviceCopy* dc = nullptr;
  for (const DeviceCopy* e : scene->copies)
    if (e->device == c->device) dc = e;
  *out = fr_scene_info{};
  out->h2d_ms = out->patch_ms = out->refit_ms = -1.0f;
  out->version = scene->version;
  out->edit_seq = scene->edit_seq;
  if (!dc) return FR_OK;
  out->packs = dc->packs;
  out->refits = dc->refits;
  out->has_tree = dc->ps.facts.bvh_ok ? 1u : 0u;
  out->n_nodes = dc->ps.n_nodes;
  const SceneSync& sy = c->scene_sync;
  if (sy.copy != dc) return FR_OK;
  out->last_sync = sy.kind;
  out->prims_patched = sy.prims;
  out->nodes_refit = sy.nodes;
  out->refit_launches = sy.launches;
  if (sy.kind == FR_SCENE_SYNC_REFIT && sy.refit_no == dc->refits) {
    out->host_ms = dc->host_ms;
    if (hipEventQuery(dc->ev_done) == hipSuccess) {
      HIPCHK(hipEventElapsedTime(&out->h2d_ms, dc->ev_part[0], dc->ev_part[1]));
      HIPCHK(hipEventElapsedTime(&out->patch_ms, dc->ev_part[1], dc->ev_part[2]));
      HIPCHK(hipEventElapsedTime(&out->refit_ms, dc->ev_part[2], dc->ev_done));
    }
  }
  return FR_OK;
}

// One table of the scene's copy on `device` as it stands (a copy that is behind the list is not
// caught up), after a device-wide wait. out NULL: *bytes only.
int fr_scene_download_table(fr_scene* scene, int device, uint32_t which, void* out, size_t cap, size_t* bytes) {
  if (!scene || (!out && !bytes)) return set_error(FR_EARG, "fr_scene_download_table: null argument");
  std::lock_guard<std::mutex> g(scene->mu);
  const DeviceCopy* dc = nullptr;
  for (const DeviceCopy* e : scene->copies)
    if (e->device == device) dc = e;
  if (!dc || !dc->blob) return set_error(FR_EARG, "fr_scene_download_table: the scene has no copy on device %d", device);
  const PackedScene& ps = dc->ps;
  size_t off = 0, size = 0;
  switch (which) {
    case FR_TABLE_RECORDS: off = ps.off_rec, size = 64u * static_cast<size_t>(ps.facts.n); break;
    case FR_TABLE_LEAF_RECORDS: off = ps.off_lrec, size = 64u * static_cast<size_t>(ps.n_slots); break;
    case FR_TABLE_LEAF_ORDER: off = ps.off_bvh_order, size = 4u * static_cast<size_t>(ps.n_slots); break;
    case FR_TABLE_NODES: off = ps.off_bvh, size = sizeof(BvhNode) * static_cast<size_t>(ps.n_nodes); break;
    case FR_TABLE_SLOT_BOUNDS: off = ps.off_slot_bounds, size = sizeof(RefitBox) * static_cast<size_t>(ps.n_slots); break;
    case FR_TABLE_NODE_UNIONS: off = ps.off_unions, size = sizeof(RefitBox) * static_cast<size_t>(ps.n_nodes); break;
    default: return set_error(FR_EARG, "fr_scene_download_table: unknown table %u", which);
  }
  if (bytes) *bytes = size;
  if (!out) return FR_OK;
  if (cap < size) return set_error(FR_EARG, "fr_scene_download_table: %zu bytes, the buffer holds %zu", size, cap);
  SET_DEVICE(device);
  HIPCHK(hipDeviceSynchronize());
  if (size) HIPCHK(hipMemcpy(out, static_cast<const char*>(dc->blob) + off, size, hipMemcpyDeviceToHost));
  return FR_OK;
}

// The view's feature buffers: one pass on the sum stream, behind whatever is
// enqueued there; nothing is waited for. Frames, A, Q, d_mean, d_u8, the pending render and its
// stats are untouched: the pass reads the scene's device copy and writes buffers of its own.
int fr_ctx_gbuffer(fr_ctx* c, fr_scene* scene, const fr_camera* cam, uint32_t width, uint32_t height) {
  if (!c || !scene || !cam) return set_error(FR_EARG, "fr_ctx_gbuffer: null argument");
  if (!width || !height) return set_error(FR_EARG, "fr_ctx_gbuffer: width %u and height %u must be > 0", width, height);
  if (static_cast<uint64_t>(width) * height > 0x7FFFFFFFull / 16u)
    return set_error(FR_EARG, "fr_ctx_gbuffer: %u x %u pixels, at most 2^27 are supported", width, height);
  SET_DEVICE(c->device);
  const PlanEnv env = read_plan_env();
  DeviceCopy* dc = nullptr;
  int rc;
  if ((rc = ctx_scene(c, scene, env.bvh_force, &dc))) return rc;
  if (c->gb_w != width || c->gb_h != height || !c->d_gb_alb) {
    HIPCHK(hipStreamSynchronize(c->stream_sum));  // the kernels and copies that use the old buffers
    c->gb_valid = false;
    c->gb_w = c->gb_h = 0;
    const size_t bytes = static_cast<size_t>(width) * height * sizeof(float4);
    size_t caps[3] = {};  // (grow with no capacity: each buffer is replaced)
    if ((rc = grow(c->d_gb0, caps[0], bytes))) return rc;
    if ((rc = grow(c->d_gb1, caps[1], bytes))) return rc;
    if ((rc = grow(c->d_gb_alb, caps[2], bytes))) return rc;
    c->gb_w = width;
    c->gb_h = height;
  }
  const PackedScene& ps = dc->ps;
  const CastScene cs = cast_scene(dc);
  const GbScene& gs = cs.gb;
  // scenes with a tree walk it (gbuffer_tree_kernel) from a camera within the
  // scene's reach (plan.cpp's cam_near). FR_BVH=0 keeps the list; FR_GBUFFER_WALK=list / tree
  // picks the walk whatever the default is (A/B: tools/gbuffer_time.py sets it for itself)
  const char* walk = getenv("FR_GBUFFER_WALK");
  const bool want_tree = walk && !strcmp(walk, "tree") ? true : walk && !strcmp(walk, "list") ? false : kGbTreeDefault;
  const bool tree = want_tree && cs.n_segs > 0 && !env.bvh_off &&
                    camera_reach(*cam) <= bvh_origin_reach(ps.facts.bvh_extent, ps.facts.bvh_sphere_rmin);
  const GbCam gc{V3{cam->position[0], cam->position[1], cam->position[2]},
                 V3{cam->lower_left[0], cam->lower_left[1], cam->lower_left[2]},
                 V3{cam->horizontal[0], cam->horizontal[1], cam->horizontal[2]},
                 V3{cam->vertical[0], cam->vertical[1], cam->vertical[2]}};
  // fr_ctx_temporal's cap reads the hit primitive's class: a copy the context owns (the scene's
  // table is freed by the scene's next edit, which hipFree orders behind this copy)
  const size_t cls_bytes = static_cast<size_t>(gs.n) * sizeof(uint32_t);
  if (c->cap_gb_cls < cls_bytes) {
    HIPCHK(hipStreamSynchronize(c->stream_sum));  // a reprojection may read the smaller table
    c->gb_valid = false;
    if ((rc = grow(c->d_gb_cls, c->cap_gb_cls, cls_bytes))) return rc;
  }
  if (c->log_on) HIPCHK(log_start(c, 3, c->stream_sum));
  if (tree)
    HIPCHK(launch_gbuffer_tree(c->stream_sum, cs, gc, width, height, c->d_gb0, c->d_gb1, c->d_gb_alb));
  else
    HIPCHK(launch_gbuffer(c->stream_sum, gs, gc, width, height, c->d_gb0, c->d_gb1, c->d_gb_alb));
  if (c->log_on) HIPCHK(log_end(c, 3, c->stream_sum));
  c->gb_tree = tree;
  if (cls_bytes) HIPCHK(hipMemcpyAsync(c->d_gb_cls, gs.cls, cls_bytes, hipMemcpyDeviceToDevice, c->stream_sum));
  c->gb_n = gs.n;
  c->gb_uid = dc->uid;
  c->gb_cam = *cam;
  c->gb_valid = true;
  return FR_OK;
}

// px pixels (or hits) of the three device words, unpacked on the host after a wait for the sum
// stream: only the planes asked for are copied.
static int download_words(fr_ctx* c, size_t px, const float4* d0, const float4* d1, const float4* dalb, uint32_t* prim,
                          float* depth, float* normal, float* position, float* albedo) {
  const bool want0 = depth || normal, want1 = prim || position;
  std::vector<float> g0(want0 ? 4 * px : 0), g1(want1 ? 4 * px : 0), al(albedo ? 4 * px : 0);
  hipStream_t st = c->stream_sum;
  if (want0) HIPCHK(hipMemcpyAsync(g0.data(), d0, px * sizeof(float4), hipMemcpyDeviceToHost, st));
  if (want1) HIPCHK(hipMemcpyAsync(g1.data(), d1, px * sizeof(float4), hipMemcpyDeviceToHost, st));
  if (albedo) HIPCHK(hipMemcpyAsync(al.data(), dalb, px * sizeof(float4), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (size_t i = 0; i < px; ++i) {
    if (prim) memcpy(&prim[i], &g1[4 * i + 3], 4);
    if (depth) depth[i] = g0[4 * i + 3];
    if (normal) memcpy(&normal[3 * i], &g0[4 * i], 12);
    if (position) memcpy(&position[3 * i], &g1[4 * i], 12);
    if (albedo) memcpy(&albedo[3 * i], &al[4 * i], 12);
  }
  return FR_OK;
}

int fr_ctx_download_gbuffer(fr_ctx* c, uint32_t* prim, float* depth, float* normal, float* position, float* albedo) {
  if (!c) return set_error(FR_EARG, "fr_ctx_download_gbuffer: null ctx");
  if (!c->gb_valid) return set_error(FR_EARG, "fr_ctx_download_gbuffer: no G-buffer (fr_ctx_gbuffer first)");
  SET_DEVICE(c->device);
  return download_words(c, static_cast<size_t>(c->gb_w) * c->gb_h, c->d_gb0, c->d_gb1, c->d_gb_alb, prim, depth, normal,
                        position, albedo);
}

int fr_ctx_gbuffer_info(fr_ctx* c, int* tree) {
  if (!c || !tree) return set_error(FR_EARG, "fr_ctx_gbuffer_info: null argument");
  if (!c->gb_valid) return set_error(FR_EARG, "fr_ctx_gbuffer_info: no G-buffer (fr_ctx_gbuffer first)");
  *tree = c->gb_tree ? 1 : 0;
  return FR_OK;
}

// The n rays of a query on the device: the caller's device pointer, or the context's copy of the
// caller's host rays, which leave through a pinned buffer the context owns (copied before the
// call returns; the device copy stays asynchronous on the sum stream).
static int stage_rays(fr_ctx* c, const fr_ray* rays, uint32_t n, bool host_rays, const float4** d_rays) {
  *d_rays = reinterpret_cast<const float4*>(rays);
  if (!host_rays) return FR_OK;
  const size_t ray_bytes = static_cast<size_t>(n) * sizeof(fr_ray);
  int rc;
  if (!c->ev_cast) HIPCHK(hipEventCreateWithFlags(&c->ev_cast, hipEventDisableTiming));
  if (c->cap_cast_rays < ray_bytes) {
    HIPCHK(hipStreamSynchronize(c->stream_sum));  // an earlier query may still read the smaller copy
    if ((rc = grow(c->d_cast_rays, c->cap_cast_rays, ray_bytes))) return rc;
  }
  if (c->cast_copy_pending) HIPCHK(hipEventSynchronize(c->ev_cast));
  c->cast_copy_pending = false;
  if (c->cap_cast_host < ray_bytes) {
    if (c->h_cast_rays) HIPCHK(hipHostFree(c->h_cast_rays));
    c->h_cast_rays = nullptr;
    c->cap_cast_host = 0;
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&c->h_cast_rays), ray_bytes, hipHostMallocDefault));
    c->cap_cast_host = ray_bytes;
  }
  memcpy(c->h_cast_rays, rays, ray_bytes);
  HIPCHK(hipMemcpyAsync(c->d_cast_rays, c->h_cast_rays, ray_bytes, hipMemcpyHostToDevice, c->stream_sum));
  HIPCHK(hipEventRecord(c->ev_cast, c->stream_sum));
  c->cast_copy_pending = true;
  *d_rays = c->d_cast_rays;
  return FR_OK;
}

// Ray queries: one cast kernel on the sum stream, behind whatever is enqueued
// there; nothing is waited for but the pinned staging buffer's previous copy. Frames, A, Q, the
// outputs, the pending render and its stats, the G-buffer and the history are untouched.
int fr_ctx_cast(fr_ctx* c, fr_scene* scene, const fr_ray* rays, uint32_t n, uint32_t flags) {
  if (!c || !scene || !rays) return set_error(FR_EARG, "fr_ctx_cast: null argument");
  if (!n || n > (1u << 27)) return set_error(FR_EARG, "fr_ctx_cast: n %u must be 1 to 2^27", n);
  if (flags & ~(FR_CAST_LIST | FR_CAST_RAYS_DEVICE | FR_CAST_TMAX))
    return set_error(FR_EARG, "fr_ctx_cast: unknown flags 0x%x", flags);
  SET_DEVICE(c->device);
  const PlanEnv env = read_plan_env();
  DeviceCopy* dc = nullptr;
  int rc;
  if ((rc = ctx_scene(c, scene, env.bvh_force, &dc))) return rc;
  if (n > c->cast_cap || !c->d_cast_waves) {
    HIPCHK(hipStreamSynchronize(c->stream_sum));  // the kernels and copies that use the old buffers
    c->cast_valid = false;
    c->cast_cap = 0;
    const size_t bytes = static_cast<size_t>(n) * sizeof(float4);
    size_t caps[3] = {};  // (grow with no capacity: each buffer is replaced)
    if ((rc = grow(c->d_hit0, caps[0], bytes))) return rc;
    if ((rc = grow(c->d_hit1, caps[1], bytes))) return rc;
    if ((rc = grow(c->d_hit_alb, caps[2], bytes))) return rc;
    if (!c->d_cast_waves) HIPCHK(hipMalloc(&c->d_cast_waves, kCastWaveBytes));
    c->cast_cap = n;
  }
  const float4* d_rays = nullptr;
  if ((rc = stage_rays(c, rays, n, !(flags & FR_CAST_RAYS_DEVICE), &d_rays))) return rc;
  const CastScene cs = cast_scene(dc);
  const bool tree = cs.n_segs > 0 && !(flags & FR_CAST_LIST);
  HIPCHK(hipMemsetAsync(c->d_cast_waves, 0, kCastWaveBytes, c->stream_sum));
  if (c->log_on) HIPCHK(log_start(c, 3, c->stream_sum));
  HIPCHK(launch_cast(c->stream_sum, cs, tree, d_rays, n, c->d_hit0, c->d_hit1, c->d_hit_alb, c->d_cast_waves,
                     (flags & FR_CAST_TMAX) != 0));
  if (c->log_on) HIPCHK(log_end(c, 3, c->stream_sum));
  c->cast_n = n;
  c->cast_tree = tree;
  c->cast_valid = true;
  return FR_OK;
}

int fr_ctx_download_hits(fr_ctx* c, uint32_t* prim, float* t, float* normal, float* position, float* albedo) {
  if (!c) return set_error(FR_EARG, "fr_ctx_download_hits: null ctx");
  if (!c->cast_valid) return set_error(FR_EARG, "fr_ctx_download_hits: no hits (fr_ctx_cast first)");
  SET_DEVICE(c->device);
  return download_words(c, c->cast_n, c->d_hit0, c->d_hit1, c->d_hit_alb, prim, t, normal, position, albedo);
}

// Waits for stream_sum and sums the first k words of every stripe of a striped wave counter
// (cast.h kCastStripes) into sum[0..k).
static int sum_stripes(fr_ctx* c, const uint32_t* d_waves, uint32_t k, uint32_t* sum) {
  std::vector<uint32_t> stripes(kCastWaveBytes / 4);
  HIPCHK(hipMemcpyAsync(stripes.data(), d_waves, kCastWaveBytes, hipMemcpyDeviceToHost, c->stream_sum));
  HIPCHK(hipStreamSynchronize(c->stream_sum));
  for (uint32_t j = 0; j < k; ++j) sum[j] = 0;
  for (uint32_t s = 0; s < kCastStripes; ++s)
    for (uint32_t j = 0; j < k; ++j) sum[j] += stripes[s * kCastStripeWords + j];
  return FR_OK;
}

int fr_ctx_cast_info(fr_ctx* c, fr_cast_info* out) {
  if (!c || !out) return set_error(FR_EARG, "fr_ctx_cast_info: null argument");
  if (!c->cast_valid) return set_error(FR_EARG, "fr_ctx_cast_info: no hits (fr_ctx_cast first)");
  SET_DEVICE(c->device);
  uint32_t waves[2];
  int rc;
  if ((rc = sum_stripes(c, c->d_cast_waves, 2, waves))) return rc;
  out->n = c->cast_n;
  out->tree = c->cast_tree ? 1u : 0u;
  out->waves_tree = waves[0];
  out->waves_list = waves[1];
  return FR_OK;
}

int fr_ctx_hit_buffers(fr_ctx* c, void** g0, void** g1, void** alb, uint32_t* n) {
  if (!c) return set_error(FR_EARG, "fr_ctx_hit_buffers: null ctx");
  if (!c->cast_valid) return set_error(FR_EARG, "fr_ctx_hit_buffers: no hits (fr_ctx_cast first)");
  if (g0) *g0 = c->d_hit0;
  if (g1) *g1 = c->d_hit1;
  if (alb) *alb = c->d_hit_alb;
  if (n) *n = c->cast_n;
  return FR_OK;
}

// Occlusion queries: fr_ctx_cast's driver with one byte per ray for the hits
// and a wave counter of its own. Frames, A, Q, the outputs, the pending render and its stats, the
// G-buffer, the history and the last cast's hits and counter are untouched.
int fr_ctx_occluded(fr_ctx* c, fr_scene* scene, const fr_ray* rays, uint32_t n, uint32_t flags, uint8_t* out) {
  if (!c || !scene || !rays) return set_error(FR_EARG, "fr_ctx_occluded: null argument");
  if (!n || n > (1u << 27)) return set_error(FR_EARG, "fr_ctx_occluded: n %u must be 1 to 2^27", n);
  if (flags & ~(FR_CAST_LIST | FR_CAST_RAYS_DEVICE | FR_CAST_TMAX | FR_CAST_OUT_DEVICE))
    return set_error(FR_EARG, "fr_ctx_occluded: unknown flags 0x%x", flags);
  const bool out_device = (flags & FR_CAST_OUT_DEVICE) != 0;
  if (out_device && !out) return set_error(FR_EARG, "fr_ctx_occluded: FR_CAST_OUT_DEVICE with a NULL out");
  SET_DEVICE(c->device);
  const PlanEnv env = read_plan_env();
  DeviceCopy* dc = nullptr;
  int rc;
  if ((rc = ctx_scene(c, scene, env.bvh_force, &dc))) return rc;
  if (!c->d_occl_waves) HIPCHK(hipMalloc(&c->d_occl_waves, kCastWaveBytes));
  if (!out_device && n > c->occl_cap) {
    HIPCHK(hipStreamSynchronize(c->stream_sum));  // the kernels and copies that use the old bytes
    if (c->occl_out == c->d_occl) c->occl_valid = false;
    c->occl_cap = 0;
    size_t cap = 0;  // (grow with no capacity: the buffer is replaced)
    if ((rc = grow(c->d_occl, cap, n))) return rc;
    c->occl_cap = n;
  }
  const float4* d_rays = nullptr;
  if ((rc = stage_rays(c, rays, n, !(flags & FR_CAST_RAYS_DEVICE), &d_rays))) return rc;
  const CastScene cs = cast_scene(dc);
  const bool tree = cs.n_segs > 0 && !(flags & FR_CAST_LIST);
  uint8_t* d_out = out_device ? out : c->d_occl;
  HIPCHK(hipMemsetAsync(c->d_occl_waves, 0, kCastWaveBytes, c->stream_sum));
  if (c->log_on) HIPCHK(log_start(c, 3, c->stream_sum));
  HIPCHK(launch_occlude(c->stream_sum, cs, tree, d_rays, n, (flags & FR_CAST_TMAX) != 0, d_out, c->d_occl_waves));
  if (c->log_on) HIPCHK(log_end(c, 3, c->stream_sum));
  c->occl_n = n;
  c->occl_tree = tree;
  c->occl_out = d_out;
  c->occl_valid = true;
  return FR_OK;
}

int fr_ctx_download_occluded(fr_ctx* c, uint8_t* host) {
  if (!c) return set_error(FR_EARG, "fr_ctx_download_occluded: null ctx");
  if (!c->occl_valid) return set_error(FR_EARG, "fr_ctx_download_occluded: no query (fr_ctx_occluded first)");
  SET_DEVICE(c->device);
  if (host) HIPCHK(hipMemcpyAsync(host, c->occl_out, c->occl_n, hipMemcpyDeviceToHost, c->stream_sum));
  HIPCHK(hipStreamSynchronize(c->stream_sum));
  return FR_OK;
}

int fr_ctx_occluded_info(fr_ctx* c, fr_occl_info* out) {
  if (!c || !out) return set_error(FR_EARG, "fr_ctx_occluded_info: null argument");
  if (!c->occl_valid) return set_error(FR_EARG, "fr_ctx_occluded_info: no query (fr_ctx_occluded first)");
  SET_DEVICE(c->device);
  uint32_t sum[3];
  int rc;
  if ((rc = sum_stripes(c, c->d_occl_waves, 3, sum))) return rc;
  *out = fr_occl_info{c->occl_n, c->occl_tree ? 1u : 0u, sum[0], sum[1], sum[2], {0, 0, 0}};
  return FR_OK;
}

// A guide field out of range, as fr_ctx_denoise_guided and fr_ctx_temporal (`who`) refuse it.
static int guide_refusal(const char* who, const fr_denoise_guide& gd) {
  if (!(gd.sigma_z > 0.0f && gd.sigma_z <= kDnSigmaZMax))
    return set_error(FR_EARG, "%s: sigma_z %g must be finite, > 0 and <= %g", who, static_cast<double>(gd.sigma_z),
                     static_cast<double>(kDnSigmaZMax));
  if (gd.normal_pow2 > kDnNormalPow2Max)
    return set_error(FR_EARG, "%s: normal_pow2 %u must be 0 to %u", who, gd.normal_pow2, kDnNormalPow2Max);
  if (gd.demodulate > 1u) return set_error(FR_EARG, "%s: demodulate %u must be 0 or 1", who, gd.demodulate);
  if (gd.pad != 0u) return set_error(FR_EARG, "%s: pad %u must be 0", who, gd.pad);
  return FR_OK;
}

// What fr_ctx_denoise_guided and fr_ctx_temporal (`who`) refuse alike of the G-buffer: none, or one
// of another scene upload, camera or size than the live accumulation's.
static int gbuffer_refusal(const fr_ctx* c, const char* who) {
  if (!c->gb_valid) return set_error(FR_EARG, "%s: no G-buffer (fr_ctx_gbuffer first)", who);
  const AccumState& a = c->accum;
  const KParams& kp = c->accum_kp;
  if (c->gb_uid != a.key.scene_uid)
    return set_error(FR_EARG, "%s: the G-buffer is of another scene upload than the live accumulation", who);
  if (memcmp(&c->gb_cam, &a.key.cam, sizeof(fr_camera)) != 0)
    return set_error(FR_EARG, "%s: the G-buffer is of another camera than the live accumulation", who);
  if (c->gb_w != kp.W)
    return set_error(FR_EARG, "%s: the G-buffer's width %u differs from the live accumulation's %u", who, c->gb_w, kp.W);
  if (c->gb_h != kp.H)
    return set_error(FR_EARG, "%s: the G-buffer's height %u differs from the live accumulation's %u", who, c->gb_h, kp.H);
  return FR_OK;
}

// The guided filter on demand: fr_ctx_denoise's place on the sum stream, behind
// the G-buffer pass it reads (the same stream), into the same output buffers.
int fr_ctx_denoise_guided(fr_ctx* c, uint32_t levels, float k, const fr_denoise_guide* g) {
  if (!c) return set_error(FR_EARG, "fr_ctx_denoise_guided: null ctx");
  static const char* who = "fr_ctx_denoise_guided";
  int rc;
  if ((rc = denoise_refusal(c, who, levels, k))) return rc;
  const fr_denoise_guide dflt{kDnSigmaZDefault, kDnNormalPow2Default, 1u, 0u};
  const fr_denoise_guide gd = g ? *g : dflt;
  if ((rc = guide_refusal(who, gd))) return rc;
  if ((rc = gbuffer_refusal(c, who))) return rc;
  const AccumState& a = c->accum;
  const KParams& kp = c->accum_kp;
  SET_DEVICE(c->device);
  if ((rc = denoise_buffers(c))) return rc;
  const bool tiled = c->tiled.tiled;
  HIPCHK(launch_denoise_guided(c->stream_sum, kp, c->d_accum, c->d_sq, tiled ? c->d_nt : nullptr,
                               tiled ? c->d_kt : nullptr, a.samples, a.frames, levels, k,
                               DnGuide{gd.sigma_z, gd.normal_pow2, gd.demodulate}, c->d_gb0, c->d_gb1, c->d_gb_alb,
                               c->d_dn_ping, c->d_dn_pong, c->d_dn_mean, c->d_dn_u8, c->d_dn_var));
  c->dn_valid = true;
  return FR_OK;
}

int fr_ctx_download_denoised(fr_ctx* c, float* mean_rgb, uint8_t* rgb8, float* var) {
  if (!c) return set_error(FR_EARG, "fr_ctx_download_denoised: null ctx");
  if (!c->dn_valid) return set_error(FR_EARG, "fr_ctx_download_denoised: no denoised image (fr_ctx_denoise first)");
  SET_DEVICE(c->device);
  const size_t px = static_cast<size_t>(c->dn_w) * c->dn_h;
  hipStream_t st = c->stream_sum;
  if (mean_rgb && px) HIPCHK(hipMemcpyAsync(mean_rgb, c->d_dn_mean, px * 3 * sizeof(float), hipMemcpyDeviceToHost, st));
  if (rgb8 && px) HIPCHK(hipMemcpyAsync(rgb8, c->d_dn_u8, px * 3, hipMemcpyDeviceToHost, st));
  if (var && px) HIPCHK(hipMemcpyAsync(var, c->d_dn_var, px * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return FR_OK;
}

int fr_ctx_denoised_buffers(fr_ctx* c, float** d_mean_rgb, uint8_t** d_rgb8) {
  if (!c) return set_error(FR_EARG, "fr_ctx_denoised_buffers: null ctx");
  if (!c->dn_valid) return set_error(FR_EARG, "fr_ctx_denoised_buffers: no denoised image (fr_ctx_denoise first)");
  if (d_mean_rgb) *d_mean_rgb = c->d_dn_mean;
  if (d_rgb8) *d_rgb8 = c->d_dn_u8;
  return FR_OK;
}

// ---- temporal reuse -----------------------------------------------------

static_assert(sizeof(fr_temporal) == 32, "fr_temporal layout");

// The history's and the prior's buffers at the live accumulation's size. Another size loses the
// history with its buffers.
static int temporal_buffers(fr_ctx* c) {
  const KParams& kp = c->accum_kp;
  if (c->tp_w == kp.W && c->tp_h == kp.H && c->d_tp_why) return FR_OK;
  HIPCHK(hipStreamSynchronize(c->stream_sum));  // the kernels and copies that use the old buffers
  c->tp_valid = false;
  c->tp = TemporalState{};
  c->tp_w = c->tp_h = 0;
  const size_t px = static_cast<size_t>(kp.W) * kp.H;
  int rc;
  for (float4** b : {&c->d_tp_ta[0], &c->d_tp_ta[1], &c->d_tp_tq[0], &c->d_tp_tq[1], &c->d_tp_g0, &c->d_tp_g1,
                     &c->d_tp_pa, &c->d_tp_pq}) {
    size_t cap = 0;  // (grow with no capacity: each buffer is replaced)
    if ((rc = grow(*b, cap, px * sizeof(float4)))) return rc;
  }
  for (uint32_t** b : {&c->d_tp_src, &c->d_tp_why}) {
    size_t cap = 0;
    if ((rc = grow(*b, cap, px * sizeof(uint32_t)))) return rc;
  }
  c->tp_w = kp.W;
  c->tp_h = kp.H;
  return FR_OK;
}

static GbCam gb_cam_of(const fr_camera& cam) {
  return GbCam{V3{cam.position[0], cam.position[1], cam.position[2]},
               V3{cam.lower_left[0], cam.lower_left[1], cam.lower_left[2]},
               V3{cam.horizontal[0], cam.horizontal[1], cam.horizontal[2]},
               V3{cam.vertical[0], cam.vertical[1], cam.vertical[2]}};
}

// Everything a call enqueues, on the sum stream: behind the resolve of every frame enqueued so
// far and behind the G-buffer pass, ahead of every later frame's resolve.
static int temporal_enqueue(fr_ctx* c, const TemporalStep& st, uint32_t levels, float k, const fr_denoise_guide* g,
                            const TpOpt& opt) {
  const KParams& kp = c->accum_kp;
  const AccumState& a = c->accum;
  hipStream_t s = c->stream_sum;
  const size_t px = static_cast<size_t>(kp.W) * kp.H;
  const bool log = c->log_on;  // fr_ctx_trace_log: an event pair around each of the three stages
  if (log) HIPCHK(log_start(c, 2, s));
  if (st.action == TemporalAction::kReproject)
    HIPCHK(launch_temporal_reproject(s, tp_cam(c->tp_cam), opt, kp.W, kp.H, c->d_gb0, c->d_gb1, c->d_gb_cls, c->gb_n,
                                     c->d_tp_g0, c->d_tp_g1, c->d_tp_ta[st.read], c->d_tp_tq[st.read], c->d_tp_pa,
                                     c->d_tp_pq, c->d_tp_src, c->d_tp_why));
  if (st.action == TemporalAction::kEmpty && px) {
    HIPCHK(hipMemsetAsync(c->d_tp_pa, 0, px * sizeof(float4), s));
    HIPCHK(hipMemsetAsync(c->d_tp_pq, 0, px * sizeof(float4), s));
    HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c->d_tp_src), static_cast<int>(kTpNone), px, s));
    HIPCHK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(c->d_tp_why), static_cast<int>(kTpNoHistory), px, s));
  }
  if (st.action != TemporalAction::kKeep && px) {
    // the view's own G-buffer words join its history, behind the reprojection that read the last view's
    HIPCHK(hipMemcpyAsync(c->d_tp_g0, c->d_gb0, px * sizeof(float4), hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(c->d_tp_g1, c->d_gb1, px * sizeof(float4), hipMemcpyDeviceToDevice, s));
  }
  if (log) HIPCHK(log_end(c, 2, s));
  if (log) HIPCHK(log_start(c, 2, s));
  const bool tiled = c->tiled.tiled;
  HIPCHK(launch_temporal_prep(s, kp, c->d_accum, c->d_sq, tiled ? c->d_nt : nullptr, tiled ? c->d_kt : nullptr,
                              a.samples, a.frames, c->d_tp_pa, c->d_tp_pq, c->d_tp_ta[st.write], c->d_tp_tq[st.write],
                              g ? c->d_gb0 : nullptr, c->d_gb1, g ? c->d_gb_alb : nullptr,
                              g ? g->demodulate : 0u, c->d_dn_ping));
  if (log) HIPCHK(log_end(c, 2, s));
  if (log) HIPCHK(log_start(c, 2, s));
  if (levels == 0)
    HIPCHK(launch_temporal_finalise(s, kp.W, kp.H, c->d_dn_ping, g ? c->d_gb_alb : nullptr, g ? g->demodulate : 0u,
                                    c->d_dn_mean, c->d_dn_u8, c->d_dn_var));
  else if (g)
    HIPCHK(launch_denoise_guided_levels(s, kp.W, kp.H, levels, k, DnGuide{g->sigma_z, g->normal_pow2, g->demodulate},
                                        c->d_gb0, c->d_gb1, c->d_gb_alb, c->d_dn_ping, c->d_dn_pong, c->d_dn_mean,
                                        c->d_dn_u8, c->d_dn_var));
  else
    HIPCHK(launch_denoise_levels(s, kp.W, kp.H, levels, k, c->d_dn_ping, c->d_dn_pong, c->d_dn_mean, c->d_dn_u8,
                                 c->d_dn_var));
  if (log) HIPCHK(log_end(c, 2, s));
  return FR_OK;
}

// Temporal reuse on demand: fr_ctx_denoise's place on the sum stream and its output buffers;
// nothing is waited for. A, Q, the counts, d_mean, d_u8, the pending render and its stats are read
// or untouched. Within one accumulation the prior stands: a later call's opt does not change it.
int fr_ctx_temporal(fr_ctx* c, uint32_t levels, float k, const fr_denoise_guide* g, const fr_temporal* opt) {
  if (!c) return set_error(FR_EARG, "fr_ctx_temporal: null ctx");
  static const char* who = "fr_ctx_temporal";
  if (levels > kDnLevelsMax) return set_error(FR_EARG, "%s: levels %u must be 0 to %u", who, levels, kDnLevelsMax);
  if (!(k > 0.0f && k <= kDnKMax))
    return set_error(FR_EARG, "%s: k %g must be finite, > 0 and <= %g", who, static_cast<double>(k),
                     static_cast<double>(kDnKMax));
  const AccumState& a = c->accum;
  if (!a.live) return set_error(FR_EARG, "%s: no live accumulation (no FR_FLAG_ACCUMULATE frame yet, or reset)", who);
  if (!a.has_q || !c->d_sq)
    return set_error(FR_EARG, "%s: the live accumulation carries no Q: its frames lack FR_FLAG_ACCUM_ERROR", who);
  if (c->accum_kp.shard_count != 1)
    return set_error(FR_EARG, "%s: shard_count %u: a reprojected pixel's source lies in the strips of other shards, "
                              "only a whole image (shard_count 1) is reused", who, c->accum_kp.shard_count);
  int rc;
  if (g && (rc = guide_refusal(who, *g))) return rc;
  const fr_temporal dflt{kTpNMaxDefault, kTpNMaxSpecularDefault, kTpSigmaZDefault, kTpNormalMinDefault, {0u, 0u, 0u, 0u}};
  const fr_temporal o = opt ? *opt : dflt;
  if (!(o.n_max > 0.0f && o.n_max <= kTpNMaxMax))
    return set_error(FR_EARG, "%s: n_max %g must be finite, > 0 and <= %g", who, static_cast<double>(o.n_max),
                     static_cast<double>(kTpNMaxMax));
  if (!(o.n_max_specular >= 0.0f && o.n_max_specular <= kTpNMaxMax))
    return set_error(FR_EARG, "%s: n_max_specular %g must be finite, >= 0 and <= %g", who,
                     static_cast<double>(o.n_max_specular), static_cast<double>(kTpNMaxMax));
  if (!(o.sigma_z > 0.0f && o.sigma_z <= kDnSigmaZMax))
    return set_error(FR_EARG, "%s: temporal sigma_z %g must be finite, > 0 and <= %g", who,
                     static_cast<double>(o.sigma_z), static_cast<double>(kDnSigmaZMax));
  if (!(o.normal_min >= -1.0f && o.normal_min <= 1.0f))
    return set_error(FR_EARG, "%s: normal_min %g must be finite, >= -1 and <= 1", who, static_cast<double>(o.normal_min));
  for (uint32_t p : o.pad)
    if (p != 0u) return set_error(FR_EARG, "%s: temporal pad %u must be 0", who, p);
  if ((rc = gbuffer_refusal(c, who))) return rc;
  SET_DEVICE(c->device);
  if ((rc = denoise_buffers(c))) return rc;
  if ((rc = temporal_buffers(c))) return rc;
  const TemporalStep st =
      temporal_step(c->tp, c->accum_gen, TemporalKey{a.key.scene_uid, a.key.width, a.key.height, a.key.max_depth});
  if ((rc = temporal_enqueue(c, st, levels, k, g, TpOpt{o.n_max, o.n_max_specular, o.sigma_z, o.normal_min}))) {
    c->tp = TemporalState{};  // part of a call may stand on the device: the history is not to be trusted
    c->tp_valid = false;
    return rc;
  }
  c->tp = st.next;
  if (st.action != TemporalAction::kKeep) c->tp_cam = gb_cam_of(a.key.cam);
  c->tp_last = st.write;
  c->tp_valid = true;
  c->dn_valid = true;
  return FR_OK;
}

int fr_ctx_temporal_reset(fr_ctx* c) {
  if (!c) return set_error(FR_EARG, "fr_ctx_temporal_reset: null ctx");
  c->tp = TemporalState{};  // (host state only: the next call's prior is filled afresh)
  return FR_OK;
}

int fr_ctx_download_temporal(fr_ctx* c, float* prior_a, float* prior_q, float* prior_n, float* prior_k, float* total_a,
                             float* total_q, float* total_n, float* total_k, uint32_t* source, uint32_t* reason) {
  if (!c) return set_error(FR_EARG, "fr_ctx_download_temporal: null ctx");
  if (!c->tp_valid) return set_error(FR_EARG, "fr_ctx_download_temporal: no temporal call (fr_ctx_temporal first)");
  SET_DEVICE(c->device);
  const size_t px = static_cast<size_t>(c->tp_w) * c->tp_h;
  hipStream_t st = c->stream_sum;
  // the device words are unpacked on the host: only the planes asked for are copied
  struct Plane {
    const float4* dev;
    float *rgb, *w;
    std::vector<float> host;
  } planes[4] = {{c->d_tp_pa, prior_a, prior_n, {}},
                 {c->d_tp_pq, prior_q, prior_k, {}},
                 {c->d_tp_ta[c->tp_last], total_a, total_n, {}},
                 {c->d_tp_tq[c->tp_last], total_q, total_k, {}}};
  for (Plane& p : planes) {
    if (!(p.rgb || p.w) || !px) continue;
    p.host.resize(4 * px);
    HIPCHK(hipMemcpyAsync(p.host.data(), p.dev, px * sizeof(float4), hipMemcpyDeviceToHost, st));
  }
  if (source && px) HIPCHK(hipMemcpyAsync(source, c->d_tp_src, px * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (reason && px) HIPCHK(hipMemcpyAsync(reason, c->d_tp_why, px * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (Plane& p : planes) {
    if (p.host.empty()) continue;
    for (size_t i = 0; i < px; ++i) {
      if (p.rgb) memcpy(&p.rgb[3 * i], &p.host[4 * i], 12);
      if (p.w) p.w[i] = p.host[4 * i + 3];
    }
  }
  return FR_OK;
}

// The per-tile counts spread over the tiles' pixels on the host (slot_xy's tile order): not a
// hot path, and the arrays are one uint32 per 64 pixels.
int fr_ctx_download_counts(fr_ctx* c, uint32_t* samples, uint32_t* frames) {
  if (!c) return set_error(FR_EARG, "fr_ctx_download_counts: null ctx");
  const AccumState& a = c->accum;
  if (!a.live) return set_error(FR_EARG, "fr_ctx_download_counts: no live accumulation");
  SET_DEVICE(c->device);
  const KParams& kp = c->accum_kp;
  std::vector<uint32_t> nt(kp.n_tiles, a.samples), kt(kp.n_tiles, a.frames);
  if (c->tiled.tiled && kp.n_tiles) {
    HIPCHK(hipMemcpyAsync(nt.data(), c->d_nt, kp.n_tiles * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream_sum));
    HIPCHK(hipMemcpyAsync(kt.data(), c->d_kt, kp.n_tiles * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream_sum));
    HIPCHK(hipStreamSynchronize(c->stream_sum));
  }
  for (uint32_t tile = 0; tile < kp.n_tiles; ++tile) {
    const uint32_t ls = tile / kp.tiles_per_row, tc = tile - ls * kp.tiles_per_row;
    const uint32_t y0 = (kp.shard_index + ls * kp.shard_count) * kStripRows, x0 = tc * 8u;
    for (uint32_t y = y0; y < y0 + kStripRows && y < kp.H; ++y)
      for (uint32_t x = x0; x < x0 + 8u && x < kp.W; ++x) {
        if (samples) samples[static_cast<size_t>(y) * kp.W + x] = nt[tile];
        if (frames) frames[static_cast<size_t>(y) * kp.W + x] = kt[tile];
      }
  }
  return FR_OK;
}

int fr_ctx_download_error(fr_ctx* c, float* rel) {
  if (!c || !rel) return set_error(FR_EARG, "fr_ctx_download_error: null argument");
  if (!c->err_valid) return set_error(FR_EARG, "fr_ctx_download_error: no error map (fr_ctx_accum_error first)");
  SET_DEVICE(c->device);
  const KParams& kp = c->err_kp;
  hipStream_t st = c->stream_sum;
  const size_t row = kp.W;  // elements per row
  if (kp.shard_count == 1) {
    HIPCHK(hipMemcpyAsync(rel, c->d_err, row * kp.H * sizeof(float), hipMemcpyDeviceToHost, st));
  } else {  // this shard's strips, as enqueue_download copies them
    const ShardStrips ss = shard_strips(kp.H, kp.shard_index, kp.shard_count, false);
    const size_t first = static_cast<size_t>(kp.shard_index) * kStripRows * row;
    const size_t pitch = static_cast<size_t>(kp.shard_count) * kStripRows * row;
    const size_t width = kStripRows * row;
    if (ss.full)
      HIPCHK(hipMemcpy2DAsync(rel + first, pitch * 4, c->d_err + first, pitch * 4, width * 4, ss.full,
                              hipMemcpyDeviceToHost, st));
    if (ss.has_partial) {
      const size_t o = static_cast<size_t>(ss.partial) * kStripRows * row;
      HIPCHK(hipMemcpyAsync(rel + o, c->d_err + o, (kp.H - ss.partial * kStripRows) * row * 4, hipMemcpyDeviceToHost, st));
    }
  }
  HIPCHK(hipStreamSynchronize(st));
  return FR_OK;
}

int fr_ctx_trace_log(fr_ctx* c, int enable) {
  if (!c) return set_error(FR_EARG, "fr_ctx_trace_log: null ctx");
  if (enable) {
    SET_DEVICE(c->device);
    // the pairs of an earlier log may still be pending on the streams (a pipelined render
    // records its end on the sum stream): drain them before their events are recorded again
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipStreamSynchronize(c->stream2));
    HIPCHK(hipStreamSynchronize(c->stream_sum));
    c->log_n[0] = c->log_n[1] = c->log_n[2] = c->log_n[3] = 0;
  }
  c->log_on = enable != 0;
  return FR_OK;
}

int fr_ctx_trace_log_read(fr_ctx* c, int which, double* ms, uint32_t cap, uint32_t* n) {
  if (!c || !n || which < 0 || which > 5) return set_error(FR_EARG, "fr_ctx_trace_log_read: bad argument");
  SET_DEVICE(c->device);
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipStreamSynchronize(c->stream2));
  HIPCHK(hipStreamSynchronize(c->stream_sum));  // a pipelined render's end event is recorded there
  // which 0 / 1: durations of the trace launches / renders; 2 / 3: their start and end times
  // (two values each) from the first logged trace launch's start (a timeline); 4: durations of
  // the stages of the fr_ctx_temporal calls, three entries per call; 5: durations of the cast
  // and occlusion kernels and G-buffer passes
  const int w = which == 5 ? 3 : which == 4 ? 2 : which & 1;
  *n = static_cast<uint32_t>(c->log_n[w]);
  for (size_t i = 0; i < c->log_n[w] && ms; ++i) {
    if (which < 2 || which >= 4) {
      if (i >= cap) break;
      float t = 0.0f;
      HIPCHK(hipEventElapsedTime(&t, c->log_ev[w][2 * i], c->log_ev[w][2 * i + 1]));
      ms[i] = t;
    } else {
      if (2 * i + 1 >= cap || c->log_n[0] == 0) break;
      float a = 0.0f, b = 0.0f;
      HIPCHK(hipEventElapsedTime(&a, c->log_ev[0][0], c->log_ev[w][2 * i]));
      HIPCHK(hipEventElapsedTime(&b, c->log_ev[0][0], c->log_ev[w][2 * i + 1]));
      ms[2 * i] = a;
      ms[2 * i + 1] = b;
    }
  }
  return FR_OK;
}

}  // extern "C"
