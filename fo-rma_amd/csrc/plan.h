// plan.h — the frame plan: everything a render decides between its parameter check and
// its first enqueue, as a value. No HIP call, no pointer into device memory, and the
// environment is read in one function (read_plan_env), so the decisions can be printed
// and tested without a device (tests/c/plan_check.cpp). render.hip turns a plan into
// launches; plan.cpp is built by the host compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <utility>

#include "../../include/forma_rt.h"
#include "bvh.h"
#include "kparams.h"

namespace fr {

// List-loop scenes up to this many primitives may be compiled into the kernel (jit.h): the
// unrolled list stays within a few KB of code, and every record is staged in LDS
// (kRecLds) for the winner's shading as in the list kernels.
constexpr uint32_t kJitMaxPrims = 64;

constexpr int kFrameSlots = 4;  // frame slots a context holds at most (FR_FRAME_SLOTS, default 2)

// The driver's environment knobs, read once per render (tests change them between renders
// of one process).
struct PlanEnv {
  // FR_BVH=1 builds the BVH below the size/cost thresholds (A/B runs); FR_BVH=0 never uses
  // it: the in-order loop (A/B and tests)
  bool bvh_force = false, bvh_off = false;
  // the deferred unwind (kDeferMaxPrims); FR_DEFER=0 keeps the unwind in the trace kernel,
  // FR_DEFER=1 the 12-B records for small scenes too (A/B)
  bool defer_off = false, defer_12b = false;
  // FR_MAT=0 keeps the general shading step for diffuse-only scenes (A/B, tests)
  bool mat_off = false;
  // FR_PIPELINE (default 1) asks for at least that many passes; the buffer budget
  // (FR_SAMPLE_BUFFER_GB) may force more. Two pipelined passes measured 0.6 % faster
  // on C3, but overlapping launches blur each launch's own HIP-event time (DESIGN.md
  // §4.6), so one pass is the default.
  uint32_t pipeline = 1;
  // Bytes of per-sample colours one pass may hold: FR_SAMPLE_BUFFER_GB, else min(32 GiB,
  // 1/8 of the device's HBM) (32 GiB on MI355X: C4's shard and C5 trace in one pass)
  bool buffer_set = false;
  double buffer_gb = 0.0;
  // frame pipeline (fr_ctx::frame_slot): one-pass frames whose sample buffer fits twice
  // (FR_FRAME_PIPE=0 turns it off). Streamed scene_08 frames, shard 0 of N on one MI355X:
  // 17.01 -> 16.59 ms at N = 1, 2.52 -> 2.29 ms at N = 8
  // Traces: frame k+1's trace follows frame k's on one stream, or, for a shard with fewer
  // than two pixel slots per grid lane (two items per lane and block or fewer: the queue's
  // drain is a large part of the frame, shards 0 of 4 and of 8), consecutive frames' traces
  // alternate between two streams, so the next frame's trace fills the CUs the previous
  // one's drain leaves idle: shard 0/8 2.47 -> 2.29 ms per frame, 0/4 4.27-4.46 -> 4.28
  // (steadier), the same at N = 1 and 2, where serial traces keep each launch's own event
  // time. FR_FRAME_PIPE=1 / 2 forces serial / overlapping traces.
  enum FramePipe { kAuto, kOff, kSerial, kOverlap } frame_pipe = kAuto;
  // Two slots (FR_FRAME_SLOTS=3 or 4 asks for more when the budget holds them). With round
  // 3's sum, which ran longer than the trace beside it, three slots let frame k + 2's trace
  // start before frame k's sum ended; since round 4's sum keeps pace, two are faster (C3
  // streamed 16.27 -> 16.17 ms per frame, N = 2 shards -0.3 %, N = 4 and 8 the same).
  int frame_slots = 2;
  // FR_FRAME_PIPE_RESERVE=k: workgroup slots per CU a pipelined trace leaves free (A/B;
  // unset: FramePlan::reserve's rule)
  bool reserve_set = false;
  uint32_t reserve = 0;
  // the scene-specialised kernel (jit.h): FR_SCENE_JIT=1 / 0 forces it on / off; unset,
  // the caller's FR_FLAG_SCENE_JIT decides
  int scene_jit = -1;
  // BVH kernels store their samples unstaged unless FR_BVH_STAGE asks: "1" staged even at a
  // lower residency, "2" staged when it costs no residency (A/B, tests). At 7 workgroups per
  // CU the pair staging measured slower than plain stores (C5 51.45 ms unstaged, 51.87
  // staged; with 8-bin trees 48.39 / 48.63); at 6 it had paid (66.8 -> 64.3 ms, round 2).
  int bvh_stage = 0;
  // FR_MAX_WGS=k caps the grid (tests: with a few workgroups every wave claims many
  // batches, partly used ones included, so the claim paths run at small image sizes)
  uint32_t max_wgs = 0;
};
PlanEnv read_plan_env();

// What the decisions read of a scene's device copy (pack.h fills it).
struct SceneFacts {
  uint32_t n = 0;
  uint32_t kinds = 0;  // bit k set if a primitive of kind k is present
  bool has_plane = false;
  bool bvh_ok = false;   // segments and trees built (else the in-order loop only)
  uint32_t n_segs = 0;   // closest-hit segments: BVH runs and planes (bvh.h)
  // traversal-stack levels a lane can use: the trees' largest internal-node depth + 1 (a
  // lane at depth d holds at most d entries and writes the free one): the BVH launch's LDS
  uint32_t bvh_levels = kBvhStack;
  float bvh_extent = 0;  // largest |coordinate| of the primitives' bounds (bvh.h)
  float bvh_sphere_rmin = -1.0f;  // the smallest sphere's radius (-1: no sphere): bvh_origin_reach
  bool diffuse = true;   // no metal or dielectric scatter class (trace_kernel MAT = 1)
  // attenuation classes: the scene's distinct attenuations (bit patterns), when there are at
  // most kNibbleMaxPrims of them (else 0): BVH kernels with 8-B records store a path's
  // winners as classes (KScene::acls), and sum_nib_kernel reads this table instead of one
  // entry per primitive
  uint32_t n_aclass = 0;
};

// What a plan reads of the context's earlier frames.
struct PlanHistory {
  bool prev_in_flight = false;  // the previous frame's end event is still pending
  bool streaming = false;       // the frame before was enqueued while its predecessor ran
  int fs_n = 0;                 // frame slots of the current buffer layout (0: not pipelined)
  size_t fs_bytes = 0;          // sample-buffer bytes per slot in that layout
};

int check_params(const fr_params* p);

// The strips (kStripRows rows each) shard `index` of `count` owns: strip k for k = index,
// index + count, ...
struct ShardStrips {
  uint32_t strips = 0;       // strips of the whole image
  uint32_t count = 0;        // this shard's
  uint64_t rows = 0;         // image rows in them
  uint64_t traced_rows = 0;  // rows traced: render_mt never traces the rows past 4 * (H / 4) (tracer.rs:87)
  uint32_t full = 0;         // whole strips (a strided 2-D region of the image)
  bool has_partial = false;  // the image's trailing short strip is this shard's
  uint32_t partial = 0;      // its strip index
};
ShardStrips shard_strips(uint32_t height, uint32_t shard_index, uint32_t shard_count, bool mt_bands);

// largest |coordinate| a primary ray's origin can have (the BVH node cull's reach, bvh.h)
float camera_reach(const fr_camera& cam);

// What picks the trace_kernel specialisation.
struct KernelInputs {
  uint32_t kinds = 0;
  bool has_plane = false, bvh = false, small_depth = false;
  uint32_t flags = 0;  // KParams.flags: FR_FLAG_MT_BANDS, KF_DEFER, KF_NIBBLE, KF_DIFFUSE
};

struct FramePlan {
  KParams kp{};  // the frame's constants; pass_plan and the grid fill the rest per launch
  bool use_bvh = false, small_depth = false, defer = false, nibble = false, diffuse_k = false, bvh_nib = false;
  uint32_t wps = 3;      // words per sample in the buffer
  size_t per_block = 0;  // sample-buffer bytes of one sample block of the shard
  uint32_t nblocks = 0, nb_pass = 0;
  size_t cap_blocks = 0;  // blocks the sample-buffer budget holds
  int passes = 0;
  int nfs = 0;  // frame slots (0: not pipelined)
  bool fpipe = false, fpipe_overlap = false;
  bool stream_mode = false;  // frames are being streamed: this trace shares the CUs
  bool relayout = false;     // the sample buffer's slot layout changes with this frame
  uint32_t reserve = 0;      // workgroup slots per CU the trace grid leaves free
  size_t slot_bytes = 0, running_bytes = 0;
  int slots = 1;
  size_t lds = 0;
  size_t stage_bytes = 0;  // BVH kernels: LDS for sample staging, taken if it costs no residency
  size_t table_bytes = 0;  // list kernels with 8-B records: LDS for the waves' batch tables (kparams.h)
  // always 0 (the record's form follows KParams.flags) and read by nothing here. It stays for
  // one reason: the previous revision's tests/c/plan_check.cpp prints it, and that revision's
  // tests are run against this library before it is accepted. Delete it with the next change.
  int sum_kind = 0;
  bool jit_on = false, jit_wait = false, jit_cached_only = false;
  int bvh_stage = 0;     // PlanEnv's, for the grid sizing
  uint32_t max_wgs = 0;  // PlanEnv's
  KernelInputs sel;
};

// FR_OK, or FR_EARG (fr_last_error) when the shard exceeds the 32-bit work-item range.
// active_tiles: null for every frame but an adaptive one (FR_FLAG_ADAPTIVE), whose n_tiles, P,
// magics, sample buffer and passes then follow from the length of the context's active tile
// list instead of the shard's tile count; 0 gives a plan without passes. The plan stays a pure
// function of its arguments (KParams::tile_list is the driver's to set).
int make_plan(const fr_params& p, float cam_reach, const SceneFacts& sf, int num_cus, size_t device_bytes,
              const PlanEnv& env, bool dry, const PlanHistory& hist, FramePlan* out,
              const uint32_t* active_tiles = nullptr);

struct PassPlan {
  uint32_t b0 = 0, nb = 0, n_items = 0, n_coarse = 0, b_fine = 0;
};
PassPlan pass_plan(const FramePlan& fp, int pass);

// ---- progressive accumulation (FR_FLAG_ACCUMULATE) ----------------------------------
// A context's accumulator A holds the f32 sum of n samples per pixel of one still view; an
// accumulating frame adds its own per-pixel sum to it and shows A / n (sum.hip's resolve).
// The flag itself never enters the plan: make_plan drops it from KParams.flags, so an
// accumulating frame has the plain frame's plan, kernels and scene-kernel cache key.
// FR_FLAG_ACCUM_ERROR (a second accumulator Q of S^2 / spp) is dropped with it.

// What must stay the same from one accumulating frame to the next for A to go on. seed and
// spp are not part of it: frames of different spp add up, and equal seeds are the caller's
// business.
struct AccumKey {
  uint64_t scene_uid = 0;  // the scene upload's identity: a new one with every edit of the scene
  fr_camera cam{};         // compared as its 104 bytes
  uint32_t width = 0, height = 0, max_depth = 0, shard_index = 0, shard_count = 0;
  // the frame's FR_FLAG_ACCUM_ERROR bit (0 or 1): Q describes an accumulation only if every
  // frame of it added to Q, so a frame whose bit differs starts a new accumulation
  uint32_t error = 0;
};
AccumKey accum_key(uint64_t scene_uid, const fr_camera& cam, const fr_params& p);
bool same_view(const AccumKey& a, const AccumKey& b);

// A context's accumulation as of its last enqueued accumulating frame.
struct AccumState {
  bool live = false;  // false: nothing accumulated yet, or reset (fr_ctx_accum_reset)
  AccumKey key;
  uint32_t frames = 0;   // frames in A
  uint32_t samples = 0;  // n: samples per pixel in A
  bool has_q = false;    // the accumulation carries Q (every frame of it had FR_FLAG_ACCUM_ERROR)
};

struct AccumStep {
  bool start = false;  // A = S; else A = A + S
  AccumState next;     // the state once this frame is enqueued; next.samples is the divisor n
};

// The next accumulating frame of `spp` samples seen through `key`: continues `prev` iff prev
// is live and of the same view, else starts anew. FR_EARG (fr_last_error) when continuing
// would take n past 2^32 - 1; *out is then untouched.
int accum_step(const AccumState& prev, const AccumKey& key, uint32_t spp, AccumStep* out);

// ---- adaptive sampling (FR_FLAG_ADAPTIVE) ----------------------------
// fr_ctx_adapt makes the live accumulation tiled: from then on every 8x8 tile of the shard has
// its own sample and frame counts on the device, and the context holds a list of the tiles an
// adaptive frame traces. AccumState's frames and samples stay the host's totals: the frames
// enqueued and the sum of their spp, the largest count a tile can have. The tiled state dies
// with the accumulation (a frame that starts a new one, fr_ctx_accum_reset).
struct TiledState {
  bool tiled = false;
  uint32_t tiles = 0;          // tiles of the shard (each holds at least one image pixel)
  uint32_t active_tiles = 0;   // length of the list as of the last fr_ctx_adapt
  uint64_t active_pixels = 0;  // image pixels in the list's tiles
};

enum class AdaptiveFrame { kTrace, kEmpty };

// An adaptive frame seen through `key` on accumulation `prev`: FR_EARG (fr_last_error) when it
// would start a new accumulation or the live one is not tiled, before anything is enqueued;
// kEmpty when the list is empty (nothing is traced and no state moves); else kTrace, and the
// frame then goes through accum_step like any accumulating frame.
int adaptive_step(const AccumState& prev, const TiledState& tiled, const AccumKey& key, AdaptiveFrame* out);

// ---- temporal reuse (fr_ctx_temporal) --------------------------------
// A context keeps the totals of the last view fr_ctx_temporal was called for (the history) in
// one of two buffers and the current accumulation's prior beside them. What a call does is
// decided by the accumulation generation, a count the driver advances whenever accum_step starts
// a new accumulation, not by comparing cameras: fr_ctx_accum_reset followed by the same camera
// reprojects the view's own history.
struct TemporalKey {  // what must match for a history to be reprojected
  uint64_t scene_uid = 0;
  uint32_t width = 0, height = 0, max_depth = 0;
};

struct TemporalState {
  bool has_history = false;  // an earlier call's totals stand (false: none yet, dropped, or reset)
  TemporalKey key;           // the history's
  uint64_t gen = 0;          // the accumulation generation of the last call
  uint32_t read = 0;         // the totals buffer that generation's reprojection read; totals go to read ^ 1
};

enum class TemporalAction {
  kEmpty,      // no usable history: the prior is all zeros, every reason "no history yet"
  kKeep,       // the generation of the last call: the prior stands as it is
  kReproject,  // a new accumulation and a matching history: the prior is reprojected from it
};

struct TemporalStep {
  TemporalAction action = TemporalAction::kEmpty;
  uint32_t read = 0, write = 1;  // totals buffers: the reprojection's source, this call's destination
  TemporalState next;            // the state once the call is enqueued
};

// The fr_ctx_temporal call on accumulation generation `gen` seen through `key`: keeps the prior
// while the generation is that of the last call; reprojects when it changed and the history's
// scene upload, width, height and max_depth match; drops the history and starts empty otherwise.
TemporalStep temporal_step(const TemporalState& prev, uint64_t gen, const TemporalKey& key);

// ---- kernel choice ----------------------------------------------------------------

template <int KS_, bool HP_, int KREJ_, int MAXD_, bool BV_, bool MT_, int DEFER_, int MAT_ = 0>
struct KTag {
  static constexpr int KS = KS_, KREJ = KREJ_, MAXD = MAXD_, DEFER = DEFER_, MAT = MAT_;
  static constexpr bool HP = HP_, BV = BV_, MT = MT_;
};

template <int KS, bool HP, bool BV, bool MT, class F>
auto select_depth(bool small_depth, uint32_t flags, F&& f) {
  if constexpr (BV && !MT) {
    // diffuse scenes of <= 15 distinct attenuations: 8-B records of attenuation classes
    if ((flags & KF_DEFER) && (flags & KF_NIBBLE) && (flags & KF_DIFFUSE))
      return f(KTag<KS, HP, FR_KREJ_BVH, kSmallDepth, true, false, 2, 1>{});
  }
  if constexpr (!BV && !MT) {
    if (flags & KF_DEFER) {
      if ((flags & KF_NIBBLE) && (flags & KF_DIFFUSE))
        return f(KTag<KS, HP, FR_KREJ_NIB, kSmallDepth, false, false, 2, 1>{});
      if (flags & KF_NIBBLE) return f(KTag<KS, HP, FR_KREJ_NIB, kSmallDepth, false, false, 2>{});
      if (flags & KF_DIFFUSE) return f(KTag<KS, HP, FR_KREJ, kSmallDepth, false, false, 1, 1>{});
      return f(KTag<KS, HP, FR_KREJ, kSmallDepth, false, false, 1>{});
    }
  }
  const bool diffuse = (flags & KF_DIFFUSE) != 0;
  if (small_depth && diffuse) return f(KTag<KS, HP, FR_KREJ, kSmallDepth, BV, MT, 0, 1>{});
  if (small_depth) return f(KTag<KS, HP, FR_KREJ, kSmallDepth, BV, MT, 0>{});
  if (diffuse) return f(KTag<KS, HP, FR_KREJ, 0, BV, MT, 0, 1>{});
  return f(KTag<KS, HP, FR_KREJ, 0, BV, MT, 0>{});
}

// Picks the specialisation and calls f(KTag<...>{}): single-kind scenes (all boxes, all
// spheres) drop the per-primitive kind switch; HAS_PLANE adds the stale-record
// bookkeeping; small depth uses the u16 stack with the unrolled unwind. BVH kernels walk
// the list's segments (bvh.h); scenes with planes use the general kernel, which tests each
// plane in list order between the runs. The cascade is the set of compiled kernels: f is
// instantiated for exactly the tags reachable here.
template <class F>
auto select_kernel(const KernelInputs& in, F&& f) {
  if (in.flags & FR_FLAG_MT_BANDS) {  // save_image_mt: the general kernels, in-order loop
    if (in.has_plane) return select_depth<KS_ANY, true, false, true>(in.small_depth, in.flags, f);
    return select_depth<KS_ANY, false, false, true>(in.small_depth, in.flags, f);
  }
  if (in.kinds == (1u << FR_AABB)) {
    if (in.bvh) return select_depth<KS_AABB, false, true, false>(in.small_depth, in.flags, f);
    return select_depth<KS_AABB, false, false, false>(in.small_depth, in.flags, f);
  }
  if (in.kinds == (1u << FR_SPHERE)) {
    if (in.bvh) return select_depth<KS_SPHERE, false, true, false>(in.small_depth, in.flags, f);
    return select_depth<KS_SPHERE, false, false, false>(in.small_depth, in.flags, f);
  }
  if (in.has_plane) {
    if (in.bvh) return select_depth<KS_ANY, true, true, false>(in.small_depth, in.flags, f);
    return select_depth<KS_ANY, true, false, false>(in.small_depth, in.flags, f);
  }
  if (in.bvh) return select_depth<KS_ANY, false, true, false>(in.small_depth, in.flags, f);
  return select_depth<KS_ANY, false, false, false>(in.small_depth, in.flags, f);
}

// A specialisation by value: trace_kernel's eight template arguments and the name
// expression the run-time build lowers and looks up (jit.cpp).
struct KernelId {
  int targs[8] = {};
  std::string name;
};
constexpr bool kTargBool[8] = {false, true, false, false, true, true, false, false};
std::string kernel_name(const int targs[8]);  // "fr::trace_kernel<KS, HP, KREJ, MAXD, BV, MT, DEFER, MAT>"
KernelId kernel_id(const KernelInputs& in);

// This build's tuning values (tuning.h's FR_TUNING list) and instrument flags as #define
// lines: the prelude of the run-time build of trace_kernel.h, which is then the same
// specialisation as the one compiled into the library, with only the list walk replaced.
std::string tuning_defines();

}  // namespace fr
