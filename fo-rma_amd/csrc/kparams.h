// kparams.h — the launch contract the host driver and the device code share: block and
// tile sizes, the KParams flag bits, the sample-buffer and LDS layout constants, KParams
// itself and the invariant division it carries. The FR_* tuning values: tuning.h.
//
// Host-safe: compiles under g++ with no HIP headers (plan.cpp, pack.cpp), under hipcc
// (trace_kernel.h, sum.h) and under hiprtc (the run-time build of trace_kernel.h).
#pragma once
#include <stdint.h>
#include "tuning.h"

#if defined(__HIPCC_RTC__) || defined(__HIPCC__) || defined(__HIP__)
#define FR_KHD __host__ __device__ __forceinline__
#define FR_KHD_CONSTEXPR __host__ __device__ constexpr
#else
#define FR_KHD static inline
#define FR_KHD_CONSTEXPR constexpr
#endif

namespace fr {

constexpr uint32_t kBlock = 256;      // 4 waves, one 8x8 pixel tile each
constexpr uint32_t kStripRows = 8;    // rows per shard strip == tile height
constexpr uint32_t kMaxDepth = 64;    // LDS stack bound (64 KB per workgroup)
constexpr uint32_t kMaxWgPerCu = 8;   // 2048 threads per CU / kBlock: the persistent grid's cap
constexpr uint32_t kSmallDepth = 8;
// Deferred unwind (DEFER kernels: depth <= 8, <= kDeferMaxPrims primitives, no BVH, not
// render_mt): a path's sample slot holds the record {t, winners 0-3, winners 4-7} instead
// of its colour: t = the sky blend parameter 0.5 (unit(d).y + 1) of the escaping ray, or
// kDeferAbsorbed (-1, which no t in [0, 1] or NaN equals) for a path that returns 0; the
// winners as u8 primitive indices, kDeferUnit on empty levels. sum_kernel rebuilds
// a0 * (a1 * (... * term)) from it in the same order, at full SIMD width instead of in the
// few lanes whose paths end in a given iteration.
constexpr uint32_t kDeferMaxPrims = 254;
constexpr uint32_t kDeferUnit = 255;
constexpr uint32_t kDeferAbsorbed = 0xBF800000u;  // -1.0f
constexpr uint32_t KF_DEFER = 1u << 31;            // internal KParams.flags bit: records, not colours
constexpr uint32_t KF_STAGE = 1u << 30;            // internal: BVH kernel stages its samples in LDS
// Scenes of <= kNibbleMaxPrims primitives (the headline scene_08 has 6) keep the winners
// as 4-bit entries in one register instead of an LDS stack (15 = empty level) and store
// 8-B records {t, winners}: 2 words per sample instead of 3 (KF_NIBBLE, DEFER == 2).
constexpr uint32_t kNibbleMaxPrims = 15;
constexpr uint32_t kNibbleUnit = 15;
constexpr uint32_t KF_NIBBLE = 1u << 29;           // internal: 8-B deferred records
constexpr uint32_t KF_DIFFUSE = 1u << 28;          // internal: no metal/dielectric (trace_kernel MAT = 1)
// internal: an adaptive frame, KParams::tile_list maps its compact tiles (set by the driver with
// the pointer, after the plan: it is no part of the kernel choice). The seeding tests this bit
// of a word it already holds instead of the pointer.
constexpr uint32_t KF_LIST = 1u << 27;
// RNG contract, not tuning: one stream per 16-sample block (oracle.cpp agrees; the goldens pin it)
constexpr uint32_t kBlockSamples = 16;  // samples per RNG stream (numerics contract)
// The last block of a pixel with more than one block is split into sub-blocks of
// kFineSamples samples, each its own stream (key kFineKey | s / kFineSamples): the queue
// ends with short items, so the drain after the last claim is short.
// (Splitting the last 2, 3 or 4 blocks measured 0.9-2.7 % slower at 1 GPU for 1-2 % at
// shard 0 of 8; one queue head per XCD, with stealing, 1.4 % slower.)
constexpr uint32_t kFineSamples = 4;
constexpr uint32_t kFineSub = kBlockSamples / kFineSamples;  // sub-blocks per block
constexpr uint32_t kFineKey = 0x80000000u;
static_assert(kFineSamples >= 1 && kBlockSamples % kFineSamples == 0 && kFineSub <= 4,
              "sub-block index packs into 2 bits of the claim's block word");

// KS: KS_AABB / KS_SPHERE when every primitive has that kind (no per-primitive kind
// switch), else KS_ANY (trace_kernel's first template argument).
enum { KS_ANY = 0, KS_AABB = 1, KS_SPHERE = 2 };

struct KParams {
  uint32_t W, H, spp, max_depth;
  uint64_t seed;
  uint32_t shard_index, shard_count, tiles_per_row, n_tiles, flags;
  uint32_t P;         // pixel slots of the shard: n_tiles x 64, tile order
  uint32_t b0, nb;    // this pass renders sample blocks [b0, b0 + nb)
  uint32_t n_items;   // nb x P work items (pixel slot, block); < 2^32 per pass
  uint32_t tiles_magic, tiles_shift;  // x / n_tiles = fastdiv(x, tiles_magic, tiles_shift)
  // the jitter's (x + r) / W as 2^24 (x + r) / (2^24 W), the 2^24 folded into the operands
  // (exact scalings): rW = RN(1 / W) 2^-24 = RN(1 / (2^24 W)) (host IEEE division), sW =
  // 2^24 W; the same for H
  float rW, rH, sW, sH;
  uint32_t row_magic, row_shift;      // x / tiles_per_row = fastdiv(x, row_magic, row_shift)
  uint32_t band_h;                    // FR_FLAG_MT_BANDS: rows per band, H / 4 (tracer.rs:87)
  uint32_t ks;          // sample slots per work item in the sample buffer: min(spp, kBlockSamples)
  // items handed out without the queue: wave w of the grid starts on batch w (one batch
  // per wave, n_static = waves x 64); the queue counts from n_static
  uint32_t n_static;
  // items [n_coarse, n_items) are the sub-blocks of block b_fine (the pixels' last block,
  // when spp > kBlockSamples and this pass holds it): item = n_coarse + k * P + q for
  // sub-block k; n_coarse = n_items when the pass has none
  uint32_t n_coarse, b_fine;
  // FR_FLAG_ADAPTIVE: the context's active tile list, ascending real tiles
  // of the shard. Non-null only for an adaptive frame, whose n_tiles, P, items and magics are
  // then the list's: a compact slot q stands for real slot (tile_list[q >> 6] << 6) | (q & 63)
  // (slot_xy). Null, and KF_LIST clear, for every other frame.
  const uint32_t* tile_list;
};

// Unsigned 32-bit division by the invariant n_tiles: q = (t + ((x - t) >> s1)) >> s2 with
// t = mulhi(x, m), l = ceil(log2 d), m = floor(2^32 (2^l - d) / d) + 1, s1 = min(l, 1),
// s2 = max(l - 1, 0) (Granlund-Montgomery; d = 1 gives m = 1, q = x). tests/test_fastdiv.py.
FR_KHD uint32_t fastdiv(uint32_t x, uint32_t m, uint32_t shifts) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint32_t t = __umulhi(x, m);
#else
  const uint32_t t = static_cast<uint32_t>((static_cast<uint64_t>(x) * m) >> 32);
#endif
  return (t + ((x - t) >> (shifts & 1u))) >> (shifts >> 1);
}

// The host's half: m and the packed shifts (s1 | s2 << 1) for the divisor d.
static inline void fastdiv_magic(uint32_t d, uint32_t& m, uint32_t& shifts) {
  if (d < 1) d = 1;
  const uint32_t l = d == 1 ? 0u : 32u - static_cast<uint32_t>(__builtin_clz(d - 1));
  m = static_cast<uint32_t>(((static_cast<uint64_t>(1) << 32) * ((static_cast<uint64_t>(1) << l) - d)) / d + 1);
  shifts = (l < 1 ? l : 1u) | ((l > 0 ? l - 1 : 0u) << 1);
}

constexpr uint32_t kAttLds = 1024;  // attenuation/class entries staged in LDS (16 B each)
constexpr uint32_t kRecLds = 64;    // whole 64-B records staged in LDS for small scenes
// Sample colours a lane stages in LDS before storing them to the (item-major) sample
// buffer: 4 x 12 B = three 16-B stores per 4 samples (4 x 8 B = two, for 8-B records)
// instead of four scattered stores, which L2 wrote back as partial lines (3.5x WRITE_SIZE).
// The BVH kernels stage 2 samples when the 6 KB this adds to their LDS (which holds the
// traversal stack) keeps their resident workgroups per CU (KF_STAGE, decided at launch):
// C5 66.8 -> 64.3 ms; on scenes whose LDS tables fill the CU it would cost a workgroup.
// (BVH kernels with 8-B records stage like the list kernels: their LDS holds no unwind stack)
constexpr uint32_t kStage = 4, kBvhStage = 2;
FR_KHD_CONSTEXPR uint32_t stage_samples(bool bvh, bool nib = false) { return bvh && !nib ? kBvhStage : kStage; }
// a sub-block's group store starts at the sub-block's first sample and never writes
// another sub-block's slots
static_assert(kStage <= kFineSamples && kBvhStage <= kFineSamples && kFineSamples % kStage == 0 &&
                  kFineSamples % kBvhStage == 0,
              "a staging group never exceeds a sub-block");

// Per-wave batch table (trace_kernel's claim step): when a wave seeds a batch
// of 64 items, lane k stores everything item base + k needs to start as one 32-B entry in
// LDS, and a claiming lane reads its entry back instead of deriving it.
// Only the list kernels with 8-B records have the table: their LDS holds no stack and at
// most kNibbleMaxPrims records (< 10 KB with the staging), so 8 KB more keeps every resident
// workgroup. The other kernels' LDS is spoken for (unwind and traversal stacks, up to
// kAttLds attenuations): they keep the batch in registers.
constexpr uint32_t kBatchEntryBytes = 32;
constexpr uint32_t kBatchTableBytes = kBlock * kBatchEntryBytes;  // 64 entries for each of the 4 waves
FR_KHD_CONSTEXPR bool has_batch_table(bool bvh, bool nib) { return nib && !bvh; }
// An entry: the item's four stream words, then {fx, fy, se, slot}:
//   fx, fy  the jitter's numerator bases 2^24 x + 2^23 and 2^24 yrow + 2^23 (yrow = H - y);
//   se      first sample | end sample << 8 | need << 16 | slot's bits 32.. << 24, samples
//           counted from the start of the item's 16-sample block (the loop reads a sample's
//           number only modulo kBlockSamples and against its end); need = kNeedJit for an
//           item to trace. An entry past the image edge or the pass's items has first ==
//           end == need == 0, as after an unsuccessful claim;
//   slot    the item's first sample slot in the buffer, in samples: (item - k P) ks for
//           sub-block k, below 2^36 (items are 32-bit, ks <= 16); its low 32 bits.
struct BatchEntry {
  uint32_t s0, s1, s2, s3;
  float fx, fy;
  uint32_t se, slot;
};
static_assert(sizeof(BatchEntry) == kBatchEntryBytes, "two 16-B LDS accesses per entry");
constexpr uint32_t kNeedJit = 3;  // trace_kernel's NEED_JIT

}  // namespace fr
