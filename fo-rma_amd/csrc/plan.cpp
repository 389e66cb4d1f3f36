// plan.cpp — the frame plan (plan.h): pure arithmetic over the render parameters, the
// scene's facts, the device's size and the environment's knobs.
#include "plan.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "internal.h"

namespace fr {

static bool env_is(const char* e, const char* v) { return e && strcmp(e, v) == 0; }

PlanEnv read_plan_env() {
  PlanEnv env;
  const char* e = getenv("FR_BVH");
  env.bvh_force = env_is(e, "1");
  env.bvh_off = env_is(e, "0");
  e = getenv("FR_DEFER");
  env.defer_off = env_is(e, "0");
  env.defer_12b = env_is(e, "1");
  env.mat_off = env_is(getenv("FR_MAT"), "0");
  if ((e = getenv("FR_PIPELINE"))) env.pipeline = static_cast<uint32_t>(atoi(e) > 0 ? atoi(e) : 1);
  if ((e = getenv("FR_SAMPLE_BUFFER_GB"))) env.buffer_set = true, env.buffer_gb = atof(e);
  e = getenv("FR_FRAME_PIPE");
  if (e && *e) env.frame_pipe = env_is(e, "0") ? PlanEnv::kOff : env_is(e, "2") ? PlanEnv::kOverlap : PlanEnv::kSerial;
  if ((e = getenv("FR_FRAME_SLOTS"))) env.frame_slots = std::max(2, std::min(kFrameSlots, atoi(e)));
  if ((e = getenv("FR_FRAME_PIPE_RESERVE"))) env.reserve_set = true, env.reserve = static_cast<uint32_t>(atoi(e));
  e = getenv("FR_SCENE_JIT");
  if (e && *e) env.scene_jit = env_is(e, "0") ? 0 : 1;
  e = getenv("FR_BVH_STAGE");
  env.bvh_stage = env_is(e, "1") ? 1 : env_is(e, "2") ? 2 : 0;
  if ((e = getenv("FR_MAX_WGS")) && atoi(e) > 0) env.max_wgs = static_cast<uint32_t>(atoi(e));
  return env;
}

int check_params(const fr_params* p) {
  if (!p) return set_error(FR_EARG, "null params");
  if (p->width == 0 || p->height == 0) return set_error(FR_EARG, "width/height must be > 0");
  if (static_cast<uint64_t>(p->width) * p->height > (1ull << 31))
    return set_error(FR_EARG, "image too large (pixel index must fit in 31 bits)");
  if (p->width > 65535 || p->height > 65535)
    return set_error(FR_EARG, "width/height must be < 65536 (packed pixel coordinates)");
  if (p->max_depth > kMaxDepth) return set_error(FR_EARG, "max_depth %u > %u", p->max_depth, kMaxDepth);
  if (p->strip_rows != kStripRows) return set_error(FR_EARG, "strip_rows must be %u", kStripRows);
  if (p->shard_count == 0 || p->shard_index >= p->shard_count)
    return set_error(FR_EARG, "shard_index %u / shard_count %u invalid", p->shard_index, p->shard_count);
  if ((p->flags & FR_FLAG_ACCUMULATE) && (p->flags & FR_FLAG_MT_BANDS))
    return set_error(FR_EARG, "FR_FLAG_ACCUMULATE with FR_FLAG_MT_BANDS: save_image_mt has its own averaging");
  if ((p->flags & FR_FLAG_ACCUM_ERROR) && !(p->flags & FR_FLAG_ACCUMULATE))
    return set_error(FR_EARG, "FR_FLAG_ACCUM_ERROR without FR_FLAG_ACCUMULATE: the error estimate is an accumulation's");
  if ((p->flags & FR_FLAG_ADAPTIVE) && (~p->flags & (FR_FLAG_ACCUMULATE | FR_FLAG_ACCUM_ERROR)))
    return set_error(FR_EARG, "FR_FLAG_ADAPTIVE needs FR_FLAG_ACCUMULATE | FR_FLAG_ACCUM_ERROR: its tile list comes "
                     "from an accumulation's error estimate");
  if ((p->flags & FR_FLAG_ACCUM_ERROR) && p->spp == 0)
    return set_error(FR_EARG, "FR_FLAG_ACCUM_ERROR with spp 0: a frame without samples has no S^2 / spp");
  return FR_OK;
}

ShardStrips shard_strips(uint32_t height, uint32_t shard_index, uint32_t shard_count, bool mt_bands) {
  ShardStrips s;
  s.strips = (height + kStripRows - 1) / kStripRows;
  const uint32_t mt_end = mt_bands ? (height / 4u) * 4u : height;
  for (uint32_t k = shard_index; k < s.strips; k += shard_count) {
    const uint32_t r0 = k * kStripRows, r1 = r0 + kStripRows < height ? r0 + kStripRows : height;
    ++s.count;
    s.rows += r1 - r0;
    s.traced_rows += r1 <= mt_end ? r1 - r0 : r0 < mt_end ? mt_end - r0 : 0u;
    if (r1 - r0 == kStripRows)
      ++s.full;
    else
      s.has_partial = true, s.partial = k;
  }
  return s;
}

float camera_reach(const fr_camera& cam) {
  return std::max(std::max(fabsf(cam.position[0]), fabsf(cam.position[1])), fabsf(cam.position[2])) +
         fabsf(cam.lens_radius);
}

static size_t sample_buffer_cap(size_t device_bytes, const PlanEnv& env) {
  double gb = device_bytes ? static_cast<double>(device_bytes) / 8.0 / (1ull << 30) : 8.0;
  if (gb > 32.0) gb = 32.0;
  if (env.buffer_set) gb = env.buffer_gb;
  if (gb < 0.001) gb = 0.001;
  return static_cast<size_t>(gb * (1ull << 30));
}

int make_plan(const fr_params& p, float cam_reach, const SceneFacts& sf, int num_cus, size_t device_bytes,
              const PlanEnv& env, bool dry, const PlanHistory& hist, FramePlan* out, const uint32_t* active_tiles) {
  FramePlan fp;
  const bool mt = (p.flags & FR_FLAG_MT_BANDS) != 0;
  // the node cull holds for origins within the scene's reach (bvh.h bvh_origin_reach)
  const bool cam_near = cam_reach <= bvh_origin_reach(sf.bvh_extent, sf.bvh_sphere_rmin);
  // save_image_mt renders run the in-order list kernels (select_kernel), whose LDS layout
  // (sample staging, no traversal stack) the size below must follow
  fp.use_bvh = sf.bvh_ok && sf.n_segs > 0 && cam_near && !env.bvh_off && !mt;
  KParams& kp = fp.kp;
  kp.W = p.width;
  kp.H = p.height;
  kp.rW = 1.0f / (static_cast<float>(p.width) * 16777216.0f);  // = RN(1 / W) 2^-24
  kp.rH = 1.0f / (static_cast<float>(p.height) * 16777216.0f);
  kp.sW = static_cast<float>(p.width) * 16777216.0f;
  kp.sH = static_cast<float>(p.height) * 16777216.0f;
  kp.spp = p.spp;
  kp.max_depth = p.max_depth;
  kp.seed = p.seed;
  kp.shard_index = p.shard_index;
  kp.shard_count = p.shard_count;
  // (an accumulating frame is planned, traced and cached as the plain frame: the flag stops here)
  kp.flags = p.flags & ~(FR_FLAG_ACCUMULATE | FR_FLAG_ACCUM_ERROR | FR_FLAG_ADAPTIVE);
  kp.tiles_per_row = (p.width + 7u) / 8u;
  kp.band_h = p.height / 4u;
  kp.n_tiles = shard_strips(p.height, p.shard_index, p.shard_count, mt).count * kp.tiles_per_row;
  // an adaptive frame: the compact tiles of the active list (at most the shard's)
  if (active_tiles) kp.n_tiles = std::min(*active_tiles, kp.n_tiles);
  kp.P = kp.n_tiles * 64u;
  fastdiv_magic(kp.n_tiles, kp.tiles_magic, kp.tiles_shift);
  fastdiv_magic(kp.tiles_per_row, kp.row_magic, kp.row_shift);
  // (an empty list: no blocks, so no passes, no items and no buffers)
  fp.nblocks = active_tiles && !kp.P ? 0u : (p.spp + kBlockSamples - 1) / kBlockSamples;
  // sample slots per item: a frame of spp < 16 (update()'s 1-spp frames) needs only spp
  kp.ks = p.spp < kBlockSamples ? (p.spp ? p.spp : 1u) : kBlockSamples;
  fp.small_depth = p.max_depth <= kSmallDepth && sf.n < 65536u;
  fp.diffuse_k = sf.diffuse && !env.mat_off;
  // BVH kernels defer too when the scene is diffuse and has at most 15 distinct attenuations
  // (C5: one): 8-B records of attenuation classes
  const bool may_defer = fp.small_depth && !mt && !env.defer_off;
  fp.bvh_nib = may_defer && fp.use_bvh && fp.diffuse_k && sf.n_aclass > 0;
  fp.defer = fp.bvh_nib || (may_defer && !fp.use_bvh && sf.n <= kDeferMaxPrims);
  fp.nibble = fp.bvh_nib || (fp.defer && sf.n <= kNibbleMaxPrims && !env.defer_12b);
  if (fp.defer) kp.flags |= KF_DEFER;
  if (fp.nibble) kp.flags |= KF_NIBBLE;
  if (fp.diffuse_k) kp.flags |= KF_DIFFUSE;
  fp.wps = fp.nibble ? 2u : 3u;
  fp.per_block = static_cast<size_t>(kp.P) * kp.ks * fp.wps * sizeof(float);
  // Passes of nb_pass blocks each. With more than one pass the sample buffer holds two
  // pass slots (a pass traces into one while the previous pass's sum reads the other).
  const uint32_t passes_u = fp.nblocks ? std::min(env.pipeline, fp.nblocks) : 0u;
  uint32_t nb_pass = passes_u ? (fp.nblocks + passes_u - 1) / passes_u : 0u;
  const size_t cap_blocks = fp.per_block ? sample_buffer_cap(device_bytes, env) / fp.per_block : fp.nblocks;
  fp.cap_blocks = cap_blocks;
  // 32-bit item indices. After the queue drains, every wave may still bump the counter
  // once per lane (each claim retires >= 1 lane): <= 8 blocks/CU x 4 waves x 64 x 64 on
  // 256 CUs = 2^25 past n_items, so keep 2^28 of headroom below 2^32.
  constexpr uint32_t kItemLimit = 0xFFFFFFFFu - (1u << 28);
  // The pass holding the last block runs its kFineSub sub-blocks as items: up to
  // (nb + kFineSub - 1) x P items.
  const uint32_t fine_extra = fp.nblocks > 1 ? kFineSub - 1u : 0u;
  if (kp.P && kItemLimit / kp.P < 1u + fine_extra)
    return set_error(FR_EARG, "shard of %u pixel slots exceeds the 32-bit work-item range at spp %u; use more shards",
                     kp.P, p.spp);
  uint32_t nb_max = static_cast<uint32_t>(passes_u > 1 ? cap_blocks / 2 : cap_blocks);
  if (kp.P && nb_max > kItemLimit / kp.P - fine_extra) nb_max = kItemLimit / kp.P - fine_extra;
  if (nb_max < 1) nb_max = 1;
  if (nb_pass > nb_max) {
    nb_pass = nb_max;
    if (fp.nblocks > nb_pass && nb_pass > static_cast<uint32_t>(cap_blocks / 2) && cap_blocks / 2 >= 1)
      nb_pass = static_cast<uint32_t>(cap_blocks / 2);  // two slots must fit
  }
  fp.nb_pass = nb_pass;
  fp.passes = nb_pass ? static_cast<int>((fp.nblocks + nb_pass - 1) / nb_pass) : 0;
  // the frame pipeline (PlanEnv::frame_pipe, frame_slots)
  if (fp.passes == 1 && env.frame_pipe != PlanEnv::kOff)
    for (int k = env.frame_slots; k >= 2 && !fp.nfs; --k)
      if (cap_blocks >= static_cast<uint64_t>(k) * fp.nblocks) fp.nfs = k;
  fp.fpipe = fp.nfs > 0;
  const uint64_t grid_lanes = static_cast<uint64_t>(num_cus) * (kMaxWgPerCu - 1u) * kBlock;
  // (round 6: below three slots per grid lane, so N = 2 shards of a 1080p frame overlap too;
  // at N = 1 a launch's own HIP-event time stays the launch's, and the gain measured 0.3 %)
  fp.fpipe_overlap = fp.fpipe && (env.frame_pipe == PlanEnv::kAuto ? static_cast<uint64_t>(kp.P) < 3u * grid_lanes
                                                                   : env.frame_pipe == PlanEnv::kOverlap);
  // one frame of memory: the first frame of a burst that follows a host wait (a timed region
  // after its warm-up) still overlaps; a caller that waits for every frame (update()) never does
  fp.stream_mode = (!dry && hist.prev_in_flight) || hist.streaming;
  fp.slot_bytes = fp.per_block * nb_pass;
  // a new layout (slot count or size, or not pipelined): every earlier frame must have been
  // summed before this one reuses the buffers; in one layout only this slot's last user
  fp.relayout = !fp.fpipe || fp.nfs != hist.fs_n || fp.slot_bytes != hist.fs_bytes;
  fp.slots = fp.passes > 1 ? 2 : fp.fpipe ? fp.nfs : 1;
  fp.running_bytes = static_cast<size_t>(kp.P) * 3 * sizeof(float);
  // pipelined frames leave room on every CU for the previous frame's sum workgroups:
  // one slot at N = 1 (two cost 6 %); until round 5 two for shards
  // whose traces overlap (shard 1/8 2.23 -> 2.18 ms per frame against one).
  // Round 6: overlapping traces of streamed frames take half the CU slots each (reserve
  // 4 of 8), so two frames' traces run side by side and each fills the other's drain:
  // shards of 8 stream at 1.81 ms per frame against 1.90 with reserve 2, of 4 at 3.60
  // against 3.70, of 2 at 7.21 against 7.30 (profiles/r06i_*, r06j_*). A frame whose
  // predecessor has finished shares the CUs with nothing: no reserve.
  if (fp.fpipe) fp.reserve = env.reserve_set ? env.reserve : !fp.stream_mode ? 0u : fp.fpipe_overlap ? 4u : 1u;
  const size_t n_att = sf.n <= kAttLds ? sf.n : 0u;
  const size_t stack_bytes = fp.nibble        ? 0u
                             : fp.defer       ? kSmallDepth * kBlock * sizeof(uint8_t)
                             : fp.small_depth ? kSmallDepth * kBlock * sizeof(uint16_t)
                                              : static_cast<size_t>(p.max_depth ? p.max_depth : 1u) * kBlock *
                                                    sizeof(uint32_t);
  const size_t n_rec = sf.n <= kRecLds ? sf.n : 0u;
  const size_t stage_n = stage_samples(fp.use_bvh, fp.nibble);
  // the waves' batch tables, in front of everything else (trace_kernel.h): every launch adds them
  fp.table_bytes = has_batch_table(fp.use_bvh, fp.nibble) ? kBatchTableBytes : 0u;
  fp.lds = (stage_n > 1 && (!fp.use_bvh || fp.nibble) ? kBlock * stage_n * fp.wps * sizeof(float) : 0u) +
           (n_att ? n_att + 1 : 0) * 16 + n_rec * 64 + stack_bytes +
           (fp.use_bvh ? (sf.bvh_levels + 1u) * kBlock * sizeof(uint32_t) : 0u);  // + the sentinel row
  fp.stage_bytes = fp.use_bvh && !fp.nibble && stage_n > 1 ? kBlock * stage_n * 3 * sizeof(float) : 0u;
  // the scene-specialised kernel (jit.h): list-loop scenes of <= kJitMaxPrims primitives,
  // when the caller asks (FR_FLAG_SCENE_JIT; FR_SCENE_JIT=1 / 0 forces it on / off)
  const bool want = env.scene_jit >= 0 ? env.scene_jit != 0 : (p.flags & FR_FLAG_SCENE_JIT) != 0;
#if defined(FR_DIAG)
  const bool build_ok = false;  // diagnostics builds keep their device globals in this library
#else
  const bool build_ok = true;
#endif
  fp.jit_on = want && build_ok && !fp.use_bvh && sf.n >= 1 && sf.n <= kJitMaxPrims;
  // prepare, FR_FLAG_SCENE_JIT_WAIT and the environment's FR_SCENE_JIT=1 wait for the
  // compile; plain FR_FLAG_SCENE_JIT renders run the compiled-in kernel until it is done
  fp.jit_wait = dry || (p.flags & FR_FLAG_SCENE_JIT_WAIT) != 0 || env.scene_jit == 1;
  fp.jit_cached_only = !fp.jit_wait && (p.flags & FR_FLAG_SCENE_JIT_CACHED) != 0;
  fp.bvh_stage = env.bvh_stage;
  fp.max_wgs = env.max_wgs;
  fp.sel = KernelInputs{sf.kinds, sf.has_plane, fp.use_bvh, fp.small_depth, kp.flags};
  *out = fp;
  return FR_OK;
}

PassPlan pass_plan(const FramePlan& fp, int pass) {
  const KParams& kp = fp.kp;
  PassPlan pp;
  pp.b0 = static_cast<uint32_t>(pass) * fp.nb_pass;
  pp.nb = pass < fp.passes ? std::min(fp.nb_pass, fp.nblocks - pp.b0) : 0u;
  pp.n_items = pp.nb * kp.P;
  pp.n_coarse = pp.n_items;
  if (kFineSub > 1 && fp.nblocks > 1 && pp.nb && pp.b0 + pp.nb == fp.nblocks) {
    // the pixels' last block, as sub-blocks of kFineSamples: the queue's last items
    const uint32_t n_last = kp.spp - (fp.nblocks - 1u) * kBlockSamples;
    pp.n_coarse = (pp.nb - 1u) * kp.P;
    pp.b_fine = fp.nblocks - 1u;
    pp.n_items = pp.n_coarse + ((n_last + kFineSamples - 1u) / kFineSamples) * kp.P;
  }
  return pp;
}

AccumKey accum_key(uint64_t scene_uid, const fr_camera& cam, const fr_params& p) {
  AccumKey k;
  k.scene_uid = scene_uid;
  k.cam = cam;
  k.width = p.width, k.height = p.height, k.max_depth = p.max_depth;
  k.shard_index = p.shard_index, k.shard_count = p.shard_count;
  k.error = (p.flags & FR_FLAG_ACCUM_ERROR) ? 1u : 0u;
  return k;
}

bool same_view(const AccumKey& a, const AccumKey& b) {
  return a.scene_uid == b.scene_uid && memcmp(&a.cam, &b.cam, sizeof(fr_camera)) == 0 && a.width == b.width &&
         a.height == b.height && a.max_depth == b.max_depth && a.shard_index == b.shard_index &&
         a.shard_count == b.shard_count && a.error == b.error;
}

int accum_step(const AccumState& prev, const AccumKey& key, uint32_t spp, AccumStep* out) {
  AccumStep s;
  s.start = !(prev.live && same_view(prev.key, key));
  if (!s.start && spp > 0xFFFFFFFFu - prev.samples)
    return set_error(FR_EARG, "accumulation of %u samples per pixel cannot take %u more (32-bit count); "
                     "fr_ctx_accum_reset starts a new one", prev.samples, spp);
  s.next.live = true;
  s.next.key = key;
  s.next.frames = s.start ? 1u : prev.frames + 1u;  // (<= samples while spp >= 1; wraps only with spp 0 frames)
  s.next.samples = s.start ? spp : prev.samples + spp;
  s.next.has_q = key.error != 0;
  *out = s;
  return FR_OK;
}

int adaptive_step(const AccumState& prev, const TiledState& tiled, const AccumKey& key, AdaptiveFrame* out) {
  if (!(prev.live && same_view(prev.key, key)))
    return set_error(FR_EARG, "FR_FLAG_ADAPTIVE: the frame would start a new accumulation, which has no tile list "
                     "(render plain accumulating frames, then fr_ctx_adapt)");
  if (!tiled.tiled)
    return set_error(FR_EARG, "FR_FLAG_ADAPTIVE: the live accumulation has no tile list (fr_ctx_adapt first)");
  *out = tiled.active_tiles ? AdaptiveFrame::kTrace : AdaptiveFrame::kEmpty;
  return FR_OK;
}

TemporalStep temporal_step(const TemporalState& prev, uint64_t gen, const TemporalKey& key) {
  TemporalStep s;
  const bool same = prev.key.scene_uid == key.scene_uid && prev.key.width == key.width &&
                    prev.key.height == key.height && prev.key.max_depth == key.max_depth;
  if (prev.has_history && prev.gen == gen && same) {
    s.action = TemporalAction::kKeep;
    s.read = prev.read;
  } else if (prev.has_history && same) {
    s.action = TemporalAction::kReproject;
    s.read = prev.read ^ 1u;  // the last view's totals went to the buffer its own reprojection did not read
  } else {
    s.action = TemporalAction::kEmpty;
    s.read = 0;
  }
  s.write = s.read ^ 1u;
  s.next.has_history = true;
  s.next.key = key;
  s.next.gen = gen;
  s.next.read = s.read;
  return s;
}

std::string kernel_name(const int t[8]) {
  char name[160];
  auto b = [](int v) { return v ? "true" : "false"; };
  snprintf(name, sizeof name, "fr::trace_kernel<%d, %s, %d, %d, %s, %s, %d, %d>", t[0], b(t[1]), t[2], t[3], b(t[4]),
           b(t[5]), t[6], t[7]);
  return name;
}

std::string tuning_defines() {
  std::string d;
  auto def = [&](const char* name, long v) { d += std::string("#define ") + name + " " + std::to_string(v) + "\n"; };
#define X(n) def(#n, n);
  FR_TUNING(X)
#undef X
#ifdef FR_PROF
  d += "#define FR_PROF\n";  // section clocks go to the launch's counters, not device globals
#endif
#ifdef FR_SECCNT
  d += "#define FR_SECCNT\n";  // region entry counts go to the launch's counters (tools/isa_sections.py)
#endif
  return d;
}

KernelId kernel_id(const KernelInputs& in) {
  return select_kernel(in, [](auto tag) {
    using T = decltype(tag);
    KernelId id;
    const int t[8] = {T::KS, T::HP, T::KREJ, T::MAXD, T::BV, T::MT, T::DEFER, T::MAT};
    memcpy(id.targs, t, sizeof t);
    id.name = kernel_name(t);
    return id;
  });
}

}  // namespace fr
