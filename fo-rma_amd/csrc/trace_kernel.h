// trace_kernel.h — the device side of the tracer: work-item mapping, kernel argument
// structs and the persistent path-tracing megakernel (trace_kernel).
//
// Compiled twice: into libforma_rt.so by hipcc (every specialisation, render.hip), and
// at run time by hiprtc for a scene-specialised list kernel (FR_JIT_N defined: the
// closest-hit list walk becomes an unrolled sequence of tests on the scene's records
// as compile-time constants, jit.cpp). Everything here must therefore
// compile under hiprtc: no host-only headers.
#pragma once
#if !defined(__HIPCC_RTC__)
#include <hip/hip_runtime.h>
#include <float.h>
#include <type_traits>
#include "../../include/forma_rt.h"
#include "bvh.h"
#else
#include <type_traits>
#include "forma_rt.h"
#include "bvh.h"
#ifndef FLT_MAX
#define FLT_MAX __FLT_MAX__
#endif
#endif

#ifdef FR_DIAG
// rejection-loop trip counters (wave trips via first active lane, lane tries)
__device__ unsigned long long g_fr_diag_lens[2];
__device__ unsigned long long g_fr_diag_rus[2];
#define FR_DIAG_TRY(arr)                                                           \
  do {                                                                             \
    const unsigned long long m_ = __ballot(1);                                     \
    if ((threadIdx.x & 63u) == static_cast<uint32_t>(__ffsll(m_) - 1)) {             \
      atomicAdd(&arr[0], 1ull);                                                    \
      atomicAdd(&arr[1], static_cast<unsigned long long>(__popcll(m_)));           \
    }                                                                              \
  } while (0)
// per-wave start/end (s_memrealtime, 100 MHz) for the residency-over-time profile
__device__ unsigned long long g_fr_wave_times[2 * 65536];
__device__ unsigned long long g_fr_wave_drain[65536];  // first drained claim of the wave
// segments traced per (sample block, tile) batch of 64 items: index item >> 6 (< 2^20 kept)
__device__ unsigned int g_fr_tb_cost[1u << 20];
// per wave: iterations at its first drained claim and at its end
__device__ unsigned int g_fr_wave_iters[2 * 65536];
// every 64th wave: the time of each of its first 1024 loop iterations (100 MHz)
__device__ unsigned long long g_fr_iter_times[1024 * 1024];
#endif
#include "rt_core.h"  // (its rejection loops count their trips through FR_DIAG_TRY)
#include "kparams.h"  // block sizes, KF_* bits, KParams, fastdiv: what the host driver shares

namespace fr {

// (the FR_* tuning values: tuning.h)
// work items reserved per step of the global counter: one tile of one sample block,
// seeded by the wave's 64 lanes at once (trace_kernel's claim step)
constexpr uint32_t kBatch = 64;

struct KScene {
  // one 64-B record per primitive (g0..g3; kind in the bits of g3.w): one scalar
  // load brings a primitive into SGPRs in the closest-hit loop
  const float4* __restrict__ rec;
  const float4* __restrict__ mat;   // colour rgb, fuzz
  const uint32_t* __restrict__ cls; // effective ScatterClass
  // attenuation class of each primitive (BVH kernels with 8-B records: the winners are
  // stored as classes, indices into a table of the scene's <= 15 distinct attenuations)
  const uint32_t* __restrict__ acls;
  const float4* __restrict__ att;   // attenuation rgb (colour, or 1 for light)
  const float4* __restrict__ bvh;   // BVH nodes, four float4 each (bvh.h)
  const uint32_t* __restrict__ bvh_order;  // primitive index of each leaf slot
  const float4* __restrict__ lrec;  // the primitives' records in leaf-slot order
  const uint4* __restrict__ segs;   // BvhSegment list: runs (one tree each) and planes, in list order
  // kind runs of the list (KS_ANY in-order loop): {kind, first, end, 0} for each maximal run
  // of consecutive primitives of one kind, in list order
  const uint4* __restrict__ runs;
  uint32_t n_runs;
  uint32_t n;
  uint32_t n_segs;                  // segment count (0: no BVH)
  uint32_t att_nonneg;              // every attenuation component finite and >= +0
  float reach;                      // BVH node cull is conservative for max|o_k| <= reach (bvh.h)
};


// Work buffers of one render pass.
struct KWork {
  uint32_t* queue;            // next unclaimed item (zeroed before the pass)
  // per-sample colours or deferred records, item-major: sample s of item (b, q) at
  // [(item * ks + s - 16 b)] x WPS words (3, or 2 for 8-B records), item = (b - b0) * P + q,
  // so one item's samples are contiguous (192 or 128 B at ks = 16)
  float* samples;
  unsigned long long* counters;  // [0] segments, [1] hits, [2] scatters (reduce_counters)
  // per-wave partial counters, [wave][3], stored by every wave of the grid and summed
  // into counters by reduce_counters after the launch
  unsigned long long* wave_counters;
};

// camera.rs fields the ray generator reads: position, lower_left_corner,
// horizontal, vertical, u, v (named b* here), lens_radius
struct KCam {
  float px, py, pz, lx, ly, lz, hx, hy, hz, vx, vy, vz, ux, uy, uz, bx, by, bz, lens;
  float lens_s;       // lens 2^-23
  // kCamLensPre: lens_s is exact (no underflow): the lens sample uses it
  // kCamAxial:   the camera is of the axis-aligned class (cam_axial): cam_ray_axial's terms
  uint32_t lens_pre;
  float dz;           // RN(lz - pz), the axial ray's d.z (the same f32 subtraction, on the host)
};
static_assert(sizeof(KCam) == 22 * 4, "KCam is 22 words");
constexpr uint32_t kCamLensPre = 1u, kCamAxial = 2u;

// Camera::get_ray (camera.rs:62-72) for the lens point rd = lens (kx, ky) 2^-23 (cam_lens) and
// the jittered (s, t).
struct CamRay {
  V3 o, d;
};
// lens * (k 2^-23) = (lens 2^-23) * k when lens 2^-23 is exact (kCamLensPre): the same
// product, one rounding. kx, ky: the integers of the 2^23-scaled rejection test.
struct CamLens {
  float x, y;
};
__host__ __device__ __forceinline__ CamLens cam_lens(const KCam& cm, float kx, float ky) {
  if (__builtin_expect((cm.lens_pre & kCamLensPre) != 0u, 1)) return CamLens{cm.lens_s * kx, cm.lens_s * ky};
  return CamLens{cm.lens * (kx * kSignedUnitScale), cm.lens * (ky * kSignedUnitScale)};
}
__host__ __device__ __forceinline__ CamRay cam_ray(const KCam& cm, CamLens rd, float s, float t) {
  const V3 cpos{cm.px, cm.py, cm.pz}, cllc{cm.lx, cm.ly, cm.lz}, chor{cm.hx, cm.hy, cm.hz};
  const V3 cver{cm.vx, cm.vy, cm.vz}, cu{cm.ux, cm.uy, cm.uz}, cv{cm.bx, cm.by, cm.bz};
  const V3 off = add(scl(rd.x, cu), scl(rd.y, cv));
  return CamRay{add(cpos, off), sub(sub(add(add(cllc, scl(s, chor)), scl(t, cver)), cpos), off)};
}
// The same ray for a camera of the axial class (KCam::lens_pre & kCamAxial, decided by the
// host's cam_axial): u = (ux, +-0, +-0), v = (+-0, vy, +-0), horizontal = (hx, +-0, +-0),
// vertical = (+-0, vy', +-0). The products with those zeros and the additions of the zeros
// they give are dropped: 16 operations for cam_ray's 32, the same bits (DESIGN.md §4.2
// goes through them term by term; fr_selftest_camray compares the two on the device).
__host__ __device__ __forceinline__ CamRay cam_ray_axial(const KCam& cm, CamLens rd, float s, float t) {
  const float ox = rd.x * cm.ux, oy = rd.y * cm.by;
  float oz = cm.pz, dz = cm.dz;
#if defined(__HIP_DEVICE_COMPILE__)
  // the two uniform values enter their lane registers here: the compiler otherwise moves the
  // copies to the block where this form and cam_ray join, and cam_ray's side runs them too
  asm volatile("v_mov_b32 %0, %1" : "=v"(oz) : "s"(cm.pz));
  asm volatile("v_mov_b32 %0, %1" : "=v"(dz) : "s"(cm.dz));
#endif
  return CamRay{V3{cm.px + ox, cm.py + oy, oz},
                V3{((cm.lx + s * cm.hx) - cm.px) - ox, ((cm.ly + t * cm.vy) - cm.py) - oy, dz}};
}

struct KArgs {
  KScene sc;
  KCam cam;
  KParams kp;
  KWork kw;
};

__device__ __forceinline__ V3 xyz(float4 a) { return V3{a.x, a.y, a.z}; }

// The scene is read-only for the kernel's lifetime: reading it through the constant
// address space lets the compiler use scalar loads even though the kernel stores to
// global memory inside the same loop.
typedef __attribute__((address_space(4))) const float cfloat;
struct RecRef {  // the 4 float4 of one primitive record, read through addrspace(4)
  cfloat* p;
  __device__ __forceinline__ float4 operator[](int k) const {
    return make_float4(p[4 * k], p[4 * k + 1], p[4 * k + 2], p[4 * k + 3]);
  }
};
__device__ __forceinline__ RecRef rec_at(const float4* base, uint32_t i) {
  return RecRef{(cfloat*)(reinterpret_cast<uintptr_t>(base)) + 16u * i};
}

// The kernel's arguments read again from the kernarg segment (scalar loads), where they are
// used, rather than held in SGPRs (and spilled) across the lane loop: the pointer passes
// through an empty asm, so the compiler cannot hoist or merge the loads it feeds.
// get(a) returns the wanted member of the arguments a by value.
template <class Get>
__device__ __forceinline__ auto kernarg_reload(const KArgs& args, Get get) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef __attribute__((address_space(4))) const KArgs cargs;
  cargs* ap = (cargs*)(__builtin_amdgcn_kernarg_segment_ptr());
  asm volatile("" : "+s"(ap));
  return get(*ap);
#else
  return get(args);  // (the host pass only parses the kernel)
#endif
}

// Raw buffer loads (SGPR resource over a uniform base pointer). Used where an LDS and a
// global read of the same value sit on two sides of a uniform branch: a buffer load
// cannot be merged with the LDS read into one generic (flat) load.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* base) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0x7FFFFFFF, 0x00020000);
}
__device__ __forceinline__ float4 buf_load4(const void* base, uint32_t byte_off) {
  return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(buf_rsrc(base), byte_off, 0, 0));
}
__device__ __forceinline__ uint32_t buf_load1(const void* base, uint32_t byte_off) {
  return __builtin_amdgcn_raw_buffer_load_b32(buf_rsrc(base), byte_off, 0, 0);
}

// FR_DIAG builds count, per phase, wave-level trips (one per SIMT pass of the wave)
// and lane-level work, to measure SIMT efficiency. Never enabled in the product.
#ifdef FR_DIAG
enum { DG_ITER, DG_REGEN_W, DG_REGEN_L, DG_LENS_W, DG_LENS_L, DG_RUS_W, DG_RUS_L, DG_END_W, DG_END_L,
       DG_UNW_W, DG_UNW_L, DG_HIT_W, DG_NODE_W, DG_NODE_L, DG_LEAF_W, DG_LEAF_L, DG_NCOH_W, DG_NU2_W, DG_NU4_W,
       DG_NPRIM_L, DG_N };
#define DIAG_WAVE(slot)                                                         \
  do {                                                                          \
    const unsigned long long m_ = __ballot(1);                                  \
    if (lane == static_cast<uint32_t>(__ffsll(m_) - 1)) atomicAdd(&dg[slot], 1u); \
  } while (0)
#define DIAG_LANE(slot)                                                         \
  do {                                                                          \
    const unsigned long long m_ = __ballot(1);                                  \
    if (lane == static_cast<uint32_t>(__ffsll(m_) - 1))                         \
      atomicAdd(&dg[slot], static_cast<uint32_t>(__popcll(m_)));                \
  } while (0)
#else
#define DIAG_WAVE(slot) do {} while (0)
#define DIAG_LANE(slot) do {} while (0)
#endif

// FR_PROF builds read the shader clock (s_memtime, wave-uniform) at the section
// boundaries of the lane loop and add each wave's cycles per section into
// counters[20 + k]: wall-clock residency by section. Never enabled in the product.
#ifdef FR_PROF
enum { PF_CLAIM, PF_REJ, PF_HIT, PF_SHADE, PF_END, PF_N };
#define PROF_MARK(k)                                       \
  do {                                                     \
    const uint64_t t_ = __builtin_amdgcn_s_memtime();      \
    pf_acc[k] += t_ - pf_t;                                \
    pf_t = t_;                                             \
  } while (0)
#else
#define PROF_MARK(k) do {} while (0)
#endif

// Per-phase instruction accounting (tools/isa_sections.py; never in the product). The lane
// loop is cut into regions at SEC(k):
//   FR_SEC_MARKS: SEC(k) is an assembler comment, so the ISA listing (hipcc -S) can be split
//                 into regions and each region's VALU instructions counted (static);
//   FR_SECCNT:    SEC(k) counts the wave-level entries of region k (first active lane, an LDS
//                 add; per launch into counters[4 + k]) (dynamic).
// Static VALU per region x wave entries per region = the launch's VALU instructions by phase.
// The first SC_N regions are counted; the others only mark a boundary in the listing, and
// their entries follow from a counted one (SETUP ~ CLAIM, ACC = NEED, POSTHIT = HIT,
// POSTSHADE = LATCH = ITER; GRAB = the batches the queue hands out).
// The BVH walk's node step and leaf tests each have a scalar path (every walking lane at one
// node or leaf) and a vector path, exclusive per entry: they are separate regions (SC_NODES /
// SC_NODEV, SC_LTESTS / SC_LTESTV), so a static count never adds both paths' instructions to
// one entry. SC_LIST: one primitive test of the compiled-in list loops (in a BVH kernel, the
// in-order fallback for far origins); SC_LROOT: a leaf sphere test's root step (discriminant
// > 0 on some lane). FR_SECCNT also sums the active lanes of every entry
// (counters[32 + k]).
enum { SC_ITER, SC_CLAIM, SC_JIT, SC_NEED, SC_REJ, SC_CAM, SC_SCAT, SC_HIT, SC_SKY, SC_SHADE, SC_END, SC_NODE,
       SC_LEAF, SC_NODES, SC_NODEV, SC_LTESTS, SC_LTESTV, SC_LIST, SC_LROOT, SC_N, SC_GRAB = SC_N, SC_SETUP, SC_ACC, SC_POSTHIT,
       SC_POSTSHADE, SC_LATCH, SC_NODET };
#if defined(FR_SEC_MARKS) && defined(__HIP_DEVICE_COMPILE__)
#define SEC(k) asm volatile(";FRSEC " #k)
#elif defined(FR_SECCNT)
#define SEC(k)                                                                       \
  do {                                                                               \
    const unsigned long long m_ = __ballot(1);                                       \
    if ((k) < SC_N && lane == static_cast<uint32_t>(__ffsll(m_) - 1)) {            \
      atomicAdd(&sec_cnt[(k) < SC_N ? (k) : 0], 1u);                               \
      atomicAdd(&sec_cnt[SC_N + ((k) < SC_N ? (k) : 0)], lanes_in(m_));            \
    }                                                                                \
  } while (0)
#else
#define SEC(k) do {} while (0)
#endif

// HAS_PLANE: planes may leave the shared record's t/p stale (plane.rs:27-29), so
// the last written t is tracked separately from the winner's.
// (two 32-bit popcounts: a 64-bit one leaves a 64-bit count whose compare the SALU
// cannot do, and the compiler moved it to the VALU)
// This lane's bit of a lane mask as its branch condition: LLVM's inverse ballot, which
// becomes the mask itself (an s_and_saveexec on it, no VALU). Declared by its intrinsic
// name: the hiprtc that builds the scene kernel (the one PyTorch ships) predates clang's
// __builtin_amdgcn_inverse_ballot_w64, its LLVM has the intrinsic.
extern "C" __device__ bool fr_inverse_ballot(unsigned long long) __asm("llvm.amdgcn.inverse.ballot.i64");
__device__ __forceinline__ bool lane_in(unsigned long long m) { return fr_inverse_ballot(m); }

__device__ __forceinline__ uint32_t lanes_in(unsigned long long m) {
  return static_cast<uint32_t>(__builtin_popcount(static_cast<uint32_t>(m)) +
                               __builtin_popcount(static_cast<uint32_t>(m >> 32)));
}
// The same count as one 64-bit scalar popcount with a 32-bit result: the count passes through an
// empty asm as a 32-bit scalar, so the compiler cannot widen the compare that follows to the
// 64-bit one it moves to the VALU. Not for a loop's own test: the asm (convergent, like every
// device asm) keeps the loop from being rotated, and the rejection loop then carries its state
// through 14 register copies per pass.
__device__ __forceinline__ uint32_t lanes_in_once(unsigned long long m) {
  uint32_t c = static_cast<uint32_t>(__builtin_popcountll(m));
#if defined(__HIP_DEVICE_COMPILE__)
  asm("" : "+s"(c));
#endif
  return c;
}
__device__ __forceinline__ uint32_t lanes_set(bool b) { return lanes_in(__builtin_amdgcn_ballot_w64(b)); }

// LDS byte address of a pointer into __shared__ memory, and the u32 at such an address
__device__ __forceinline__ uint32_t lds_addr(const uint32_t* p) {
  return static_cast<uint32_t>(reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) const uint32_t*)p));
}
__device__ __forceinline__ __attribute__((address_space(3))) uint32_t& lds_u32_at(uint32_t a) {
  return *reinterpret_cast<__attribute__((address_space(3))) uint32_t*>(static_cast<uintptr_t>(a));
}
// Per-lane select on a lane mask (a ballot): one v_cndmask_b32. The compiler turned chains
// of selects on compare results into branches with the conditions materialised as 0/1
// values in VGPRs; masks combined with SALU ops and this select keep them in SGPRs.
__device__ __forceinline__ uint32_t lane_sel(unsigned long long m, uint32_t if_set, uint32_t if_clear) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t r;
  asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(r) : "v"(if_clear), "v"(if_set), "s"(m));
  return r;
#else
  return if_set;  // device only
#endif
}

// The shard's real tile of slot q: q >> 6, or for an adaptive frame (KParams::tile_list) the
// list's entry for the compact tile. Every caller's wave covers one tile (a batch, a sum wave
// and an error wave are 64 consecutive slots from a multiple of 64), so the index is uniform
// and the entry comes by one scalar load.
__device__ __forceinline__ uint32_t slot_tile(const KParams& kp, uint32_t q) {
  uint32_t tile = q >> 6;
#if defined(__HIP_DEVICE_COMPILE__)
  if (kp.flags & KF_LIST) tile = kp.tile_list[__builtin_amdgcn_readfirstlane(tile)];
#endif
  return tile;
}

// Pixel slot q of a shard -> image coordinates. Slots run tile by tile (8x8 pixels,
// tiles left to right within an 8-row strip, the shard's strips top to bottom); slots
// past the image edge are invalid. LIST = false: for kernels that never run an adaptive
// frame (the plain and untiled accumulating sums), which then read no tile list.
template <bool LIST = true>
__device__ __forceinline__ bool slot_xy(const KParams& kp, uint32_t q, uint32_t& x, uint32_t& y) {
  const uint32_t tile = LIST ? slot_tile(kp, q) : q >> 6, l = q & 63u;
  const uint32_t ls = fastdiv(tile, kp.row_magic, kp.row_shift);  // tile / tiles_per_row
  const uint32_t tc = tile - ls * kp.tiles_per_row;
  const uint32_t strip = kp.shard_index + ls * kp.shard_count;
  x = tc * 8u + (l & 7u);
  y = strip * kStripRows + (l >> 3);
  return x < kp.W && y < kp.H;
}

// Work item -> (block word bw, pixel slot q, image x, y); false for a slot past the image
// edge. item = (b - b0) * P + q with P = 64 * n_tiles (split via the tile-block index),
// or n_coarse + k * P + q for sub-block k of block b_fine. bw = b for a whole block,
// b | kFineKey | k << 28 for a sub-block (b < 2^28: spp < 2^32).
__device__ __forceinline__ bool item_xy(const KParams& kp, uint32_t item, uint32_t& bw, uint32_t& q, uint32_t& x,
                                        uint32_t& y) {
  const bool fine = item >= kp.n_coarse;
  const uint32_t tb = (fine ? item - kp.n_coarse : item) >> 6;  // n_coarse is a multiple of 64
  const uint32_t bl = fastdiv(tb, kp.tiles_magic, kp.tiles_shift);
  bw = fine ? (kp.b_fine | kFineKey | (bl << 28)) : kp.b0 + bl;
  q = ((tb - bl * kp.n_tiles) << 6) | (item & 63u);
  return slot_xy(kp, q, x, y);
}

// RNG stream key of a block word: the block index, or kFineKey | s / kFineSamples for a
// sub-block starting at sample s (oracle.cpp stream_key agrees)
__host__ __device__ __forceinline__ uint32_t stream_key(uint32_t bw) {
  return (bw & kFineKey) ? (kFineKey | ((bw & 0x0FFFFFFFu) * kFineSub + ((bw >> 28) & 3u))) : bw;
}

// Everything a work item needs to start, as its batch-table entry (kparams.h BatchEntry):
// computed by the lane that seeds the item's slot, once per 64 items at full width, so the
// claim step only copies it. The divisions, integer multiplies and int-to-float
// conversions of the item's pixel, sample range and buffer slot all happen here.
__device__ __forceinline__ BatchEntry batch_entry(const KParams& kp, uint32_t item) {
  uint32_t bw, q, x, y;
  const bool in_image = item_xy(kp, item, bw, q, x, y);
  const Rng st = rng_seed(kp.seed, y * kp.W + x, stream_key(bw));
  // a sub-block k of block b_fine: samples [16 b + 4 k, +4) of the block's slot (item - k P
  // in the buffer); a whole block: k = 0
  const uint32_t k = (bw >> 28) & 3u;
  const bool fine = (bw & kFineKey) != 0u;
  const uint32_t first = k * kFineSamples;
  const uint32_t left = kp.spp - (bw & 0x0FFFFFFFu) * kBlockSamples;  // the block's samples below spp
  const uint32_t span = first + (fine ? kFineSamples : kBlockSamples);
  const uint32_t end = span < left ? span : left;
  const bool ok = in_image && item < kp.n_items;
  BatchEntry e;
  e.s0 = st.s0;
  e.s1 = st.s1;
  e.s2 = st.s2;
  e.s3 = st.s3;
  // 2^24 x + 2^23, exact (x, yrow < 2^23): the jitter's numerator bases (step 1);
  // tracer.rs:171-172: v = ((H - y) + r) / H
  e.fx = static_cast<float>(x) * 16777216.0f + 8388608.0f;
  e.fy = static_cast<float>(kp.H - y) * 16777216.0f + 8388608.0f;
  const uint64_t slot = static_cast<uint64_t>(item - k * kp.P) * kp.ks;
  e.se = (ok ? (first | (end << 8) | (kNeedJit << 16)) : 0u) | (static_cast<uint32_t>(slot >> 32) << 24);
  e.slot = static_cast<uint32_t>(slot);
  return e;
}

// 16-B LDS accesses at a byte address (a batch-table entry is two)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __attribute__((address_space(3))) u32x4& lds_u32x4_at(uint32_t a) {
  return *reinterpret_cast<__attribute__((address_space(3))) u32x4*>(static_cast<uintptr_t>(a));
}
// Orders this wave's LDS accesses across a point where lanes exchange data through LDS (the
// batch table): no instruction, the LDS serves one wave's operations in order.
__device__ __forceinline__ void wave_lds_order() {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
#endif
}

// Persistent path-tracing kernel. Work item = (pixel slot q, sample block b): the
// kBlockSamples samples [16b, 16b + 16) of one pixel, drawn in order from the RNG
// stream (seed, pixel, b). Each sample's colour goes to kw.samples; sum_kernel then
// adds every pixel's samples in sample order, exactly as save_image's
// `col = col + get_color(...)` (tracer.rs:170-175). Items are independent, so lanes
// never wait for one another's pixels: a wave claims 64 items (one tile, one block)
// per global atomic and hands them to its free lanes (ballot + mbcnt).
//
// Per iteration of the lane loop:
//   0. lanes without an item claim one;
//   1. one merged rejection loop serves both random_in_unit_circle (lens sample of a
//      new camera ray, utility.rs:4-13) and random_in_unit_sphere (scatter,
//      utility.rs:15-25): a circle try is a sphere try without the third draw, and
//      dot(p,p) = (px*px + py*py) + 0 is the same value. It stops once at most KREJ
//      lanes still reject; those keep their RNG state and go on next iteration (their
//      draws stay in stream order, so results do not depend on KREJ);
//   2. closest hit + shading for lanes holding a ray;
//   3. path end: unwind the attenuations, store the sample colour, next sample.
// MAXD > 0: max_depth <= MAXD is known at compile time; the stack holds u16 primitive
// indices (n < 65536) and is unwound by an unrolled, predicated sequence.
// MAXD == 0: any max_depth, u32 indices, a loop.
// KS: the KS_* enum (kparams.h).

// f(integral_constant<I>) for I = I0, I0 + 1, ... while I < n (n <= N), unrolled
template <uint32_t I, uint32_t N, class F>
__device__ __forceinline__ void unroll_below(uint32_t n, F& f) {
  if constexpr (I < N) {
    if (I < n) {
      f(std::integral_constant<uint32_t, I>{});
      unroll_below<I + 1u, N>(n, f);
    }
  }
}

#ifdef FR_JIT_N
// The scene-specialised build's records: FR_JIT_REC (jit.cpp) lists each primitive's 64-B
// device record as 16 u32 bit patterns (kind in word 15), so every float is exact,
// signed zeros and non-finite values included.
constexpr uint32_t kJitRec[FR_JIT_N][16] = {FR_JIT_REC};
template <uint32_t I>
struct JitRec {
  __device__ __forceinline__ float4 operator[](int k) const {
    return make_float4(__builtin_bit_cast(float, kJitRec[I][4 * k]), __builtin_bit_cast(float, kJitRec[I][4 * k + 1]),
                       __builtin_bit_cast(float, kJitRec[I][4 * k + 2]),
                       __builtin_bit_cast(float, kJitRec[I][4 * k + 3]));
  }
};
// The axis on which boxes i and i + 1 are a mirrored pair that starts at i (slab_mirror_axis,
// rt_core.h), else -1. Pairs are taken greedily from the front of the list and do not overlap:
// box i + 1 of a pair starts none.
constexpr int jit_pair_axis(uint32_t i) {
  if (i + 1u >= FR_JIT_N || kJitRec[i][15] != FR_AABB || kJitRec[i + 1u][15] != FR_AABB) return -1;
  if (i > 0u && jit_pair_axis(i - 1u) >= 0) return -1;
  float lo_i[3] = {}, hi_i[3] = {}, lo_j[3] = {}, hi_j[3] = {};
  for (int k = 0; k < 3; ++k) {
    lo_i[k] = __builtin_bit_cast(float, kJitRec[i][k]);
    hi_i[k] = __builtin_bit_cast(float, kJitRec[i][4 + k]);
    lo_j[k] = __builtin_bit_cast(float, kJitRec[i + 1u][k]);
    hi_j[k] = __builtin_bit_cast(float, kJitRec[i + 1u][4 + k]);
  }
  return slab_mirror_axis(lo_i, hi_i, lo_j, hi_j);
}
#endif

// amdgpu_num_sgpr caps the scalar registers (MI355X_MICROARCH.md "Residency and
// cooperative launch": <= 80 SGPRs admit 8 workgroups of 256 threads per CU, 82-96
// admit 7); FR_NUM_SGPR and its measurement: tuning.h.
// MAT = 1: no metal or dielectric primitive (every scatter is lambertian: lambertian, light,
// or none for stubs): the shading step drops those branches (the headline scene's case).
template <int KS, bool HAS_PLANE, int KREJ, int MAXD, bool BVH, bool MT, int DEFER, int MAT = 0>
// Waves per SIMD the kernels ask for: the list-loop kernels at least 7 (<= 72 VGPRs), the
// BVH kernels at least 6 (<= 80); without the request the general (KS_ANY) and BVH
// kernels settle at 83-94 VGPRs, 5 waves. Measured (tools/ab_bench.py): 7 for the list
// kernels (scene_01 C2 37.9 -> 36.0 ms, a few VGPRs spilled to scratch), 6 for the BVH
// ones (7 or 8 spill more: C5 +2-10 %, scene_06 +12-20 %). The per-kernel values and
// FR_MIN_WAVES (n > 0 forces n on every kernel): tuning.h.
#define FR_OCC_ATTR                                                                                      \
  __attribute__((amdgpu_waves_per_eu(FR_MIN_WAVES ? FR_MIN_WAVES : BVH ? FR_BVH_WAVES                 \
                                                      : DEFER == 2 ? FR_NIB_WAVES                       \
                                                      : (DEFER == 1 && MAT == 1) ? FR_DIFF12_WAVES : 7)))
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_num_sgpr(FR_NUM_SGPR))) FR_OCC_ATTR void trace_kernel(
    KArgs args) {
  // one by-value struct: the kernarg segment holds it at offset 0 (the camera is read
  // back from there in the lens step)
  const KScene& sc = args.sc;
  const KParams& kp = args.kp;
  const KWork& kw = args.kw;
  // LDS: [n_att + 1 x (attenuation rgb, scatter class bits)][n_rec x 64-B record]
  //      [stack: MAXD ? kBlock x MAXD u16 (lane-major) : max_depth x kBlock u32]
  // Entry n of the attenuations is (1, 1, 1): the depth-8 stack's empty levels hold n.
  // Staging the winner's data keeps per-lane global gathers off the shading path.
  // [STG > 1: kBlock x STG staged sample colours (12 B each), lane-major] in front,
  // [TABLE: the waves' batch tables, 64 x 32-B entries each (kparams.h)] before all.
  extern __shared__ uint32_t lds[];
  constexpr bool NIB = DEFER == 2;             // 8-B records, winners in a register
  constexpr uint32_t STG = stage_samples(BVH, NIB);
  constexpr bool DIFFUSE = MAT == 1;           // lambertian scatters only
  constexpr uint32_t WPS = NIB ? 2u : 3u;      // words per sample in the buffer
  constexpr bool TABLE = has_batch_table(BVH, NIB);
  constexpr uint32_t TABW = TABLE ? kBatchTableBytes / 4u : 0u;  // the tables' words
  static_assert(!TABLE || !MT, "a batch-table entry holds no render_mt band offset");
  // list kernels always stage; BVH kernels when the launch gave them the LDS (KF_STAGE)
  const bool staged = STG > 1 && (!BVH || NIB || (kp.flags & KF_STAGE) != 0u);
  float* stage = reinterpret_cast<float*>(lds) + TABW + threadIdx.x * (WPS * STG);
  // DEFER kernels (<= kDeferMaxPrims primitives) always hold the attenuations in LDS, and
  // the 8-B-record kernels (<= kNibbleMaxPrims) the records too: compile-time facts there,
  // so their global-load fallbacks are not compiled
  // (a BVH kernel with 8-B records stores attenuation classes, not primitive indices: its
  // scenes are larger than these tables)
  constexpr bool ATT_LDS = DEFER != 0 && !BVH, REC_LDS = NIB && !BVH;
  static_assert(kDeferMaxPrims <= kAttLds && kNibbleMaxPrims <= kRecLds, "LDS staging bounds");
  const uint32_t n_att = ATT_LDS || sc.n <= kAttLds ? sc.n : 0u;
  const uint32_t n_att_st = n_att ? n_att + 1u : 0u;  // with the unit entry
  const uint32_t n_rec = REC_LDS || sc.n <= kRecLds ? sc.n : 0u;
  float4* att_lds = reinterpret_cast<float4*>(lds + TABW + (staged ? kBlock * WPS * STG : 0u));
  float4* rec_lds = att_lds + n_att_st;
  uint32_t* stack = reinterpret_cast<uint32_t*>(rec_lds + 4u * n_rec);
  uint16_t* hstack = reinterpret_cast<uint16_t*>(stack);
  const uint32_t tid = threadIdx.x;
  const uint32_t lane = tid & 63u;
  static_assert(MAXD == 0 || MAXD == 8, "the u16 stack is one 16-B row per lane");
  static_assert(!DEFER || (MAXD == 8 && !MT && (!BVH || (NIB && DIFFUSE))),
                "deferred unwind: depth <= 8 list kernels, or diffuse BVH kernels with 8-B records");
  uint2* drow = reinterpret_cast<uint2*>(stack) + tid;  // DEFER: this lane's 8 u8 levels
  uint8_t* bstack = reinterpret_cast<uint8_t*>(stack);
  uint4* hrow = reinterpret_cast<uint4*>(stack) + tid;  // this lane's MAXD = 8 levels
  // BVH traversal stack, after the unwind stack: kBvhStack x kBlock u32 (level-major)
  // (8-B-record kernels keep their winners in a register: no unwind stack in front)
  uint32_t* tstack = stack + (NIB ? 0u : MAXD ? (MAXD * kBlock) / 2u : (kp.max_depth ? kp.max_depth : 1u) * kBlock);
  // ... addressed by LDS byte address. Its first level is a sentinel row of kBvhEnd below
  // level 0, so that the top of an empty stack reads kBvhEnd: a pop needs no empty test.
  // tbase: level 0's first entry
  constexpr uint32_t kLevelB = 4u * kBlock;
  const uint32_t tbase = lds_addr(tstack) + kLevelB;
  if (BVH) tstack[tid] = kBvhEnd;  // (each lane reads only its own column)
  // MAXD > 0 stack entries: with the attenuations in LDS, the entry's byte offset in
  // att_lds (n_att <= kAttLds, so < 2^16), read by the unwind without index arithmetic;
  // otherwise the primitive index
  const uint32_t ent_shift = n_att ? 4u : 0u;
  const uint32_t unit_ent = sc.n << ent_shift;
  const uint32_t unit2 = unit_ent | (unit_ent << 16);  // two empty levels
  if (DEFER == 1)
    *drow = make_uint2(~0u, ~0u);
  else if (!DEFER && MAXD > 0)
    *hrow = make_uint4(unit2, unit2, unit2, unit2);
  for (uint32_t i = tid; i < n_att_st; i += kBlock) {
    const float4 a = sc.att[i];
    att_lds[i] = make_float4(a.x, a.y, a.z, __uint_as_float(i < n_att ? sc.cls[i] : 0u));
  }
  for (uint32_t i = tid; i < 4u * n_rec; i += kBlock) rec_lds[i] = sc.rec[i];
#ifdef FR_DIAG
  __shared__ uint32_t dg[DG_N];
  if (tid < DG_N) dg[tid] = 0;
  const uint32_t gw = blockIdx.x * (kBlock / 64u) + (tid >> 6);
  if (lane == 0 && gw < 65536) {
    g_fr_wave_times[2 * gw] = __builtin_amdgcn_s_memrealtime();
    g_fr_wave_drain[gw] = ~0ull;
  }
#endif
#ifdef FR_SECCNT
  __shared__ uint32_t sec_cnt[2 * SC_N];  // wave entries, then active lanes summed over them
  if (tid < 2 * SC_N) sec_cnt[tid] = 0;
#endif
  __syncthreads();


  // NEED_JIT: a sample starts (its jitter, then its first lens try); NEED_LENS: a camera
  // lane's lens try after a rejected one
  enum : uint32_t { NEED_NONE = 0, NEED_LENS = 1, NEED_SPHERE = 2, NEED_JIT = 3 };
  static_assert(NEED_JIT == kNeedJit && NEED_NONE == 0u, "a batch-table entry holds the claim's need");
  uint32_t depth = 0;  // scatters of the path (not NIB: wnib holds them)
  // NIB: the winners as 4-bit entries, the last one pushed in bits 28..31 and the first in
  // bits 32 - 4 depth .. 35 - 4 depth, 15 on the levels below (empty). sum_kernel multiplies
  // nibble 7 first, so the path's winners are applied innermost first and the empty levels'
  // unit entries last (x * 1 = x). With d pushes nibble 8 - d is the first empty one:
  // depth < max_depth iff the nibbles under dmask are still empty.
  uint32_t wnib = ~0u;
  const uint32_t dmask = kp.max_depth ? (0xFu << (4u * (8u - min(kp.max_depth, 8u)))) : 0u;
  // stack push at level `depth` of the scatter winner
  auto push = [&](uint32_t pi) {
    if (NIB)
      wnib = (wnib >> 4) | (pi << 28);
    else if (DEFER)
      bstack[tid * 8u + depth] = static_cast<uint8_t>(pi);
    else if (MAXD > 0)
      hstack[tid * MAXD + depth] = static_cast<uint16_t>(pi << ent_shift);
    else
      stack[depth * kBlock + tid] = pi;
  };

  // the ray; while a lens sample is pending d.xy = (u, v); while a scatter sample is
  // pending o = hit point and d = scatter base ((p + n), or reflect(unit(d), n) for metal)
  V3 o{0.0f, 0.0f, 0.0f}, d{0.0f, 0.0f, 1.0f};
  V3 sn{0.0f, 0.0f, 0.0f};  // metal: normal
  float sfuzz = 0.0f, fx = 0.0f, fy = 0.0f, vofs = 0.0f;
  bool smetal = false;
  uint32_t sbest = 0, s = 0, s_end = 0, nseg = 0, nhit = 0;  // (scatters = segments - samples: the host's)
  // (a sample's index within its block is s mod kBlockSamples: blocks start at multiples of it)
  static_assert((kBlockSamples & (kBlockSamples - 1u)) == 0u, "blocks of a power-of-two sample count");
#ifdef FR_DIAG
  uint32_t diag_tb = 0, diag_seg0 = 0;  // the item's batch index, segments at its claim
  uint32_t diag_iter = 0;               // loop iterations of this wave
#endif
  float* out = kw.samples;   // the item's first sample slot (item-major buffer)
  Rng rng{0u, 0u, 0u, 0u};
  // (a lane needs a work item when its block's samples are done: s == s_end, both 0 at the
  // start, and a claim that finds no pixel leaves them equal; a compare the loop's ballot
  // takes directly, where a carried bool cost a select and a compare per iteration)
  bool active = true, have_ray = false;
  uint32_t need = NEED_NONE;

#ifdef FR_PROF
  uint64_t pf_acc[PF_N] = {0, 0, 0, 0, 0};
  uint64_t pf_t = __builtin_amdgcn_s_memtime();
#endif
  // the wave's claimed item batch [q_next, q_end): wave-uniform, updated only under
  // the uniform branch below, so it lives in scalar registers
  uint32_t q_next = 0, q_end = 0;
  // Stream starts of the wave's batch: lane k holds item (batch base + k)'s. The whole
  // wave seeds a batch when it reserves one, so rng_seed (16 quarter-rate 32-bit
  // multiplies) runs once per 64 items at full width instead of in every iteration in
  // which a lane or two claim; a claiming lane fetches its stream by a lane permute.
  Rng held{0u, 0u, 0u, 0u};
  // ... and the same slot's pixel (x | y << 16, all ones past the image edge) and sample
  // block, so a claiming lane fetches those by permute too instead of dividing the item
  uint32_t held_xy = 0xFFFFFFFFu, held_b = 0u;
  // TABLE kernels hold none of these: the seeding lane goes on to everything else the item
  // needs to start (batch_entry) and stores it as slot k of the wave's batch table in LDS,
  // this lane's own entry at byte tid * 32 of the tables. A claiming lane reads its item's
  // entry from there: no permutes, and no per-item setup in the few lanes that claim.
  const uint32_t tab_mine = lds_addr(lds) + tid * kBatchEntryBytes;
  auto seed_entry = [&](const KParams& kq, uint32_t item) {
    const BatchEntry e = batch_entry(kq, item);
    lds_u32x4_at(tab_mine) = u32x4{e.s0, e.s1, e.s2, e.s3};
    lds_u32x4_at(tab_mine + 16u) = u32x4{__float_as_uint(e.fx), __float_as_uint(e.fy), e.se, e.slot};
  };
  // A wave's first batch is its own (wave w of the grid: batch w), seeded here: 7168
  // first claims at once on one counter would queue for ~80 us (about 88 returning
  // atomics per us on one word, MI355X_MICROARCH.md "dequeue").
  {
    const KParams k0 = kernarg_reload(args, [](const auto& a) { return a.kp; });
    q_next = (blockIdx.x * (kBlock / 64u) + (tid >> 6)) * kBatch;
    q_end = q_next + kBatch;
    if constexpr (TABLE) {
      seed_entry(k0, q_next + lane);
      wave_lds_order();
    } else {
      uint32_t bb, qq, xx, yy;
      const bool in_image = item_xy(k0, q_next + lane, bb, qq, xx, yy);
      held = rng_seed(k0.seed, yy * k0.W + xx, stream_key(bb));
      held_xy = in_image ? (xx | (yy << 16)) : 0xFFFFFFFFu;
      held_b = bb;
    }
  }
  while (active) {
    SEC(SC_ITER);
    DIAG_WAVE(DG_ITER);
#ifdef FR_DIAG
    if (lane == 0 && (gw & 63u) == 0 && (gw >> 6) < 1024u && diag_iter < 1024u)
      g_fr_iter_times[(gw >> 6) * 1024u + diag_iter] = __builtin_amdgcn_s_memrealtime();
    ++diag_iter;
#endif
    const unsigned long long m = __builtin_amdgcn_ballot_w64(s == s_end);  // lanes needing an item
    // Lanes whose item is done wait (idle) until FR_CLAIM_MIN of them need one, or until no
    // active lane has other work: the claim step (its lane permutes and item setup) then
    // runs for several lanes at once instead of in nearly every iteration for one or two.
    // Only when work starts changes, never what a sample computes (results bit-identical).
    constexpr uint32_t CLAIM_MIN = NIB ? (BVH ? FR_CLAIM_MIN_BVH : FR_CLAIM_MIN_NIB) : FR_CLAIM_MIN;
    if (m && (CLAIM_MIN <= 1 || lanes_in_once(m) >= CLAIM_MIN || m == __ballot(1))) {
      SEC(SC_CLAIM);
      // 0. claim work items: the free lanes take consecutive items of the wave's batch;
      // when it runs out, the first free lane reserves the next batch of kBatch = 64
      // items (one tile of one sample block) globally. n <= 64, so one batch suffices.
      // (Prefetching the next item in batched refill passes measured slower.)
      const uint32_t n = static_cast<uint32_t>(__popcll(m));
      const uint32_t r = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32),
                                                   __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
      const uint32_t next = __builtin_amdgcn_readfirstlane(q_next);
      const uint32_t avail = __builtin_amdgcn_readfirstlane(q_end) - next;
      if constexpr (TABLE) {
        // The wave reserves the next batch only once the current one is used up: while it
        // holds fewer items than there are free lanes, the first `avail` of them claim now
        // and the others in the next iteration, from the new batch. A step then never needs
        // entries of two batches, so the seeding overwrites the table in place. One wave's
        // LDS operations stay in order: no barrier between the seeding and the claims' reads.
        // (A retired lane seeds no entry, so its slot may keep a stale one: the item number,
        // not the entry, says that the queue has drained.)
        const bool grab = avail == 0u;
        unsigned long long mc = m;  // the lanes that claim in this step
        uint32_t take = n, start = next;
        if (!grab && n > avail) {
          mc = m & __builtin_amdgcn_ballot_w64(r < avail);
          take = avail;
        }
        if (grab) {
          SEC(SC_GRAB);
          wave_lds_order();  // (earlier claims' reads of the old entries)
          const int first = __ffsll(static_cast<long long>(m)) - 1;
          uint32_t base = 0;
          if (static_cast<int>(lane) == first) base = atomicAdd(kw.queue, kBatch);
          base = __builtin_amdgcn_readlane(base, first);
          // the item split's parameters reloaded from the kernarg segment here (once per 64
          // items) rather than held in SGPRs across the loop, like the camera (step 1)
          const KParams kg = kernarg_reload(args, [](const auto& a) { return a.kp; });
          base += kg.n_static;  // past the waves' first batches
          q_end = base + kBatch;
          seed_entry(kg, base + lane);
          wave_lds_order();
          start = base;
        }
        q_next = start + take;
        const uint32_t item = start + r;
        if (lane_in(mc) && item >= kp.n_items) {
#ifdef FR_DIAG
          if (gw < 65536) {
            const unsigned long long now = __builtin_amdgcn_s_memrealtime();
            if (now < g_fr_wave_drain[gw]) {
              g_fr_wave_drain[gw] = now;
              g_fr_wave_iters[2 * gw] = diag_iter;
            }
          }
#endif
          active = false;  // queue drained
          continue;
        }
        // the claim is a fetch: no division, multiply or conversion (batch_entry did them)
        if (lane_in(mc)) {
          SEC(SC_SETUP);
          // (a batch starts at a multiple of 64: the item's slot in its batch is item mod 64)
          const uint32_t ea = lds_addr(lds) + (tid & ~63u) * kBatchEntryBytes + (item & (kBatch - 1u)) * kBatchEntryBytes;
          const u32x4 e0 = lds_u32x4_at(ea), e1 = lds_u32x4_at(ea + 16u);
          rng = Rng{e0.x, e0.y, e0.z, e0.w};  // this item's stream: rng_seed(seed, y * W + x, stream_key(b))
          fx = __uint_as_float(e1.x);
          fy = __uint_as_float(e1.y);
          // (an entry past the image edge: s == s_end and no need, as an unsuccessful claim)
          s = e1.z & 0xFFu;
          s_end = (e1.z >> 8) & 0xFFu;
          need = (e1.z >> 16) & 0xFFu;  // NEED_JIT: a sample starts, its jitter and lens sample in step 1
          // the slot as a register pair {low word, bits 32..}: one shift-and-add forms the
          // address (through an empty asm: the compiler otherwise shifts the halves apart)
          uint64_t slot = (static_cast<uint64_t>(e1.z >> 24) << 32) | e1.w;
#if defined(__HIP_DEVICE_COMPILE__)
          asm volatile("" : "+v"(slot));
#endif
          out = kw.samples + WPS * slot;
#ifdef FR_DIAG
          if (s != s_end) {
            diag_tb = item >> 6;
            diag_seg0 = nseg;
          }
#endif
        }
      } else {
        uint32_t base = 0;
        const bool grab = n > avail;
        const int first = __ffsll(static_cast<long long>(m)) - 1;
        // The item's stream start, pixel and block, by lane permute from the lane that
        // seeded them: first from the current batch (claims r < avail), then, after a grab,
        // from the new batch (claims r >= avail). Every lane of the wave is active at both
        // permutes (a permute reads 0 from an inactive source): a lane retires only after
        // the queue has drained, and from then on no batch holds a valid item.
        int sl = static_cast<int>(((next + r) & (kBatch - 1u)) << 2);
        Rng st{static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(sl, static_cast<int>(held.s0))),
               static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(sl, static_cast<int>(held.s1))),
               static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(sl, static_cast<int>(held.s2))),
               static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(sl, static_cast<int>(held.s3)))};
        uint32_t xy = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(sl, static_cast<int>(held_xy)));
        uint32_t b = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(sl, static_cast<int>(held_b)));
        if (grab) {
          SEC(SC_GRAB);
          if (static_cast<int>(lane) == first) base = atomicAdd(kw.queue, kBatch);
          base = __builtin_amdgcn_readlane(base, first);
          // A slot past the image or the queue gets a stream that is never used.
          // the item split's parameters reloaded from the kernarg segment here (once per 64
          // items) rather than held in SGPRs across the loop, like the camera (step 1)
          const KParams kg = kernarg_reload(args, [](const auto& a) { return a.kp; });
          base += kg.n_static;  // past the waves' first batches
          q_end = base + kBatch;
          uint32_t bb, qq, xx, yy;
          const bool in_image = item_xy(kg, base + lane, bb, qq, xx, yy);
          held = rng_seed(kg.seed, yy * kg.W + xx, stream_key(bb));
          held_xy = in_image ? (xx | (yy << 16)) : 0xFFFFFFFFu;
          held_b = bb;
          // claims r >= avail take the new batch's slots r - avail (base is a multiple of 64)
          sl = static_cast<int>(((r - avail) & (kBatch - 1u)) << 2);
          const Rng st2{static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(sl, static_cast<int>(held.s0))),
                        static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(sl, static_cast<int>(held.s1))),
                        static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(sl, static_cast<int>(held.s2))),
                        static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(sl, static_cast<int>(held.s3)))};
          const uint32_t xy2 = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(sl, static_cast<int>(held_xy)));
          const uint32_t b2 = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(sl, static_cast<int>(held_b)));
          if (r >= avail) {
            st = st2;
            xy = xy2;
            b = b2;
          }
        }
        q_next = grab ? base + (n - avail) : next + n;
        const uint32_t item = r < avail ? next + r : base + (r - avail);
        if (lane_in(m) && item >= kp.n_items) {
#ifdef FR_DIAG
          if (gw < 65536) {
            const unsigned long long now = __builtin_amdgcn_s_memrealtime();
            if (now < g_fr_wave_drain[gw]) {
              g_fr_wave_drain[gw] = now;
              g_fr_wave_iters[2 * gw] = diag_iter;
            }
          }
#endif
          active = false;  // queue drained
          continue;
        }
        if (lane_in(m)) {
          SEC(SC_SETUP);
          const uint32_t x = xy & 0xFFFFu, y = xy >> 16;
          bool ok = xy != 0xFFFFFFFFu;
          uint32_t yrow = kp.H - y;  // tracer.rs:171-172: v = ((H - y) + r) / H
          if (MT) {
            // render_mt (tracer.rs:86-103): band k from the top is thread t_id = 3 - k;
            // v = ((t_height - y_band) + r) / H + t_id * 0.25; rows past 4 * t_height unused
            const uint32_t k = kp.band_h ? y / kp.band_h : 4u;
            ok = ok && k < 4u;
            yrow = kp.band_h - (y - k * kp.band_h);
            vofs = static_cast<float>(3u - k) * 0.25f;
          }
          if (ok) {
            rng = st;  // this item's stream: rng_seed(seed, y * W + x, stream_key(b))
            // a sub-block k of block b_fine: samples [16 b + 4 k, +4) of the block's slot
            // (item - k * P in the buffer); a whole block: k = 0
            const uint32_t k = (b >> 28) & 3u;
            const bool fine = (b & kFineKey) != 0u;
            const uint32_t j0 = k * kFineSamples;
            s = (b & 0x0FFFFFFFu) * kBlockSamples + j0;
            out = kw.samples + WPS * (static_cast<size_t>(item - k * kp.P) * kp.ks);
#ifdef FR_DIAG
            diag_tb = item >> 6;
            diag_seg0 = nseg;
#endif
            s_end = min(s + (fine ? kFineSamples : kBlockSamples), kp.spp);
            // 2^24 x + 2^23, exact (x, yrow < 2^23): the jitter's numerator base (step 1)
            fx = static_cast<float>(x) * 16777216.0f + 8388608.0f;
            fy = static_cast<float>(yrow) * 16777216.0f + 8388608.0f;
            need = NEED_JIT;  // a sample starts: its jitter and lens sample in step 1
          }
        }
      }
    }
    PROF_MARK(PF_CLAIM);
    bool ended = false;
    V3 term{0.0f, 0.0f, 0.0f};
    // DEFER: the terminal as sky parameter bits. Every place that ends a path writes it (the sky
    // its parameter, a hit or an absorbed scatter kDeferAbsorbed), so it has no value before:
    // a default assigned here was a v_mov_b32 in every iteration, for every lane
    uint32_t tsky;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "=v"(tsky));  // (defined, by no instruction)
#else
    tsky = kDeferAbsorbed;
#endif
    if (need != NEED_NONE) {
      SEC(SC_NEED);
      // 1. merged rejection loop
      // mrej: the lanes that still reject (dd >= 2^46), one compare per pass: the loop test
      // counts it and the next pass's branch and the accept test take it back as their
      // lane condition (inverse ballot, no instruction; a compare on dd in each of them
      // cost the pass a second v_cmp, a bool carried through the loop a select and a compare).
      // Every lane here makes the first try, outside the loop: px, py and dd need no
      // initial values then
      // (the sphere/circle condition as a lane mask: one compare serves the tries and the
      // camera/scatter branch, which the compiler otherwise tested with a second v_cmp)
      const unsigned long long msph = __builtin_amdgcn_ballot_w64(need == NEED_SPHERE);
      float pz = 0.0f;  // a circle try keeps pz = 0
      DIAG_WAVE(DG_LENS_W);
      DIAG_LANE(DG_LENS_L);
      // the test in the 2^23-scaled domain (rng_signed_unit_scaled): same decisions
      float px = rng_signed_unit_scaled(rng);
      float py = rng_signed_unit_scaled(rng);
      // A sample's first draws are its jitter (tracer.rs:171-172), then its lens try: a
      // starting lane's first try takes four draws where a scatter lane's takes three (and a
      // camera lane's retry two). The third draw is made by both kinds in one instruction
      // sequence; a starting lane's first two are its jitter and it draws its try's fourth
      // in the branch below (the jitter's own two draws in their own branch, in the quarter
      // of lanes that start a sample, cost a branch of 31 VALU)
      const unsigned long long mjit = __builtin_amdgcn_ballot_w64(need == NEED_JIT);
      float pw = 0.0f;
      if (lane_in(msph | mjit)) pw = rng_signed_unit_scaled(rng);
      if (lane_in(msph)) pz = pw;
      if (lane_in(mjit)) {
        SEC(SC_JIT);
        // 2^24 r = (int32)u >> 8 + 2^23 (rng_f32_scaled; exact), so 2^24 x + 2^24 r =
        // (2^24 x + 2^23) + px, one rounding either way. 2^24 (x + r) = RN(2^24 x + 2^24 r)
        // (rounding commutes with the exact scaling), so the quotients are (x + r) / W's
        // bits: numerator +0 or in [1, 2^56], divisor 2^24 W
        d.x = div_rn(fx + px, kp.sW, kp.rW);
        d.y = div_rn(fy + py, kp.sH, kp.rH);
        if (MT) d.y = d.y + vofs;  // render_mt's band offset (tracer.rs:103)
        px = pw;
        py = rng_signed_unit_scaled(rng);
        need = NEED_LENS;
      }
      float dd = px * px + py * py + pz * pz;
      unsigned long long mrej = __builtin_amdgcn_ballot_w64(dd >= kUnitBallScaled);
      while (lanes_in(mrej) > static_cast<uint32_t>(KREJ)) {
        SEC(SC_REJ);
        DIAG_WAVE(DG_LENS_W);
        DIAG_LANE(DG_LENS_L);
        if (lane_in(mrej)) {
          px = rng_signed_unit_scaled(rng);
          py = rng_signed_unit_scaled(rng);
          if (lane_in(msph)) pz = rng_signed_unit_scaled(rng);
          dd = px * px + py * py + pz * pz;
        }
        mrej = __builtin_amdgcn_ballot_w64(dd >= kUnitBallScaled);
      }
      SEC(SC_ACC);
      // The accepted lanes: camera lanes, then scatter lanes, as two branches in sequence on
      // disjoint lane masks, not an if / else. Each writes o and d where they live: in the
      // linear order the two sides of an if / else run in, the camera side's new direction and
      // the scatter side's old one are live together, so the new direction went to fresh
      // registers and was copied into d's where the sides joined (two v_mov_b32 per iteration,
      // and the moves that shuffled `need` there).
      // the accepted point is k 2^-23 per coordinate (2r - 1, exact), k = (px, py, pz):
      // the scale is folded into the operation that uses it (below)
      const unsigned long long macc = ~mrej;
      if (lane_in(macc & ~msph)) {
        SEC(SC_CAM);
        // Camera::get_ray (camera.rs:62-72)
        // scalar loads of the camera from the kernarg segment, here, rather than 19
        // SGPRs held (and spilled) across the loop
        // An axial camera (every bundled scene's) takes the short form: one scalar branch on
        // the host's verdict, a run-time fact of the frame (update() moves the camera)
        KCam cm = kernarg_reload(args, [](const auto& a) { return a.cam; });
#if defined(__HIP_DEVICE_COMPILE__)
        // (dz loaded with the rest, ahead of the branch: left to the axial side alone it
        // became a second scalar load, and a second wait, inside it)
        asm volatile("" : "+s"(cm.dz));
#endif
        const CamLens rd = cam_lens(cm, px, py);
        // (two branches in sequence here too, for the same reason; the second form's flag
        // through an empty asm, or the compiler threads the two back into an if / else)
        uint32_t general = (cm.lens_pre & kCamAxial) ^ kCamAxial;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+s"(general));
#endif
        if (cm.lens_pre & kCamAxial) {
          const CamRay cr = cam_ray_axial(cm, rd, d.x, d.y);
          o = cr.o;
          d = cr.d;
        }
        if (general) {
          const CamRay cr = cam_ray(cm, rd, d.x, d.y);
          o = cr.o;
          d = cr.d;
        }
        if (!NIB) depth = 0;
        have_ray = true;
      }
      if (lane_in(macc & msph)) {
        SEC(SC_SCAT);
        bool ok = true;
        V3 dir;
        if (!DIFFUSE && smetal) {
          const V3 r{px * kSignedUnitScale, py * kSignedUnitScale, pz * kSignedUnitScale};
          dir = add(d, scl(sfuzz, r));  // reflected + fuzz * rus
          ok = dot(dir, sn) > 0.0f;     // sphere.rs:104 / plane.rs:121
        } else {
          // ((p + n) + rus) - p; p + n + k 2^-23 as one fma (the product is exact)
          const V3 dr{__builtin_fmaf(px, kSignedUnitScale, d.x), __builtin_fmaf(py, kSignedUnitScale, d.y),
                      __builtin_fmaf(pz, kSignedUnitScale, d.z)};
          dir = sub(dr, o);
        }
        if (ok) {
          if (!(NIB && DIFFUSE)) push(sbest);  // (NIB && DIFFUSE kernels pushed at the shading step)
          if (!NIB) ++depth;
          d = dir;
          have_ray = true;
        } else {
          ended = true;  // absorbed: get_color returns 0
          tsky = kDeferAbsorbed;
        }
      }
      if (lane_in(macc)) need = NEED_NONE;
    }
    PROF_MARK(PF_REJ);
    if (have_ray) {
      SEC(SC_HIT);
      // 2. closest hit over the list in order (tracer.rs:190-200): only the accepted t
      // of each test is needed here; the record is formed for the winner below.
      ++nseg;
      // the box test's reciprocal is RN(1 / d) clamped to +-2^100 (rt_core.h seg_box_inv):
      // recip_nr where one guard over the three components (recip_box_ok3) admits it, which
      // implies |d_k| in [2^-100, 2^126) for each, where the clamp is the identity; the rare
      // fallback divides and clamps (one branch)
      const V3 inv = seg_box_inv(d);
      const V3 boinv{o.x * inv.x, o.y * inv.y, o.z * inv.z};  // (box tests only)
      const float a_dd = dot(d, d);
      const SphereSeg ssg = sphere_seg(a_dd);  // unused (removed) in kernels without spheres
      float closest = FLT_MAX, t_last = 0.0f;
      int best = -1;
      // The node cull is conservative only under three conditions (bvh.h); a wave holding a
      // lane outside any of them tests the list in order instead, which the BVH walk equals
      // bit for bit:
      //  - the origin within the scene's reach (sc.reach = bvh_origin_reach: up to
      //    kBvhOriginReach extents, less with spheres). A stale plane record (plane.rs:27-40)
      //    can put a scatter origin p = o + t_stale d far outside; a NaN origin fails too.
      //  - a direction component of kBvhTinyDir or more: with every component tiny the hits
      //    lie at t ~ 2^100, where neither the padding's allowance nor the clamped reciprocal
      //    (below) holds.
      //  - o inv finite: |o| 2^100 overflows from |o| = 2^28, and fma(lo, inv, -inf) puts both
      //    planes of a slab the origin is inside at -inf.
      bool list_walk = !BVH;
      if (BVH) {
        const float ao = fmax3_num(__builtin_fabsf(o.x), __builtin_fabsf(o.y), __builtin_fabsf(o.z));
        const float ad = fmax3_num(__builtin_fabsf(d.x), __builtin_fabsf(d.y), __builtin_fabsf(d.z));
        const float aoi = fmax3_num(__builtin_fabsf(boinv.x), __builtin_fabsf(boinv.y), __builtin_fabsf(boinv.z));
        list_walk = __ballot(!(ao <= sc.reach) | !(ad >= kBvhTinyDir) | !(aoi <= FLT_MAX)) != 0;
      }
      if (BVH && !list_walk) {
        // The list cut at its planes (bvh.h), walked in list order: each plane tested
        // where it stands, each run of other primitives through its own tree. A
        // primitive's candidate t does not depend on t_max, so a run's effect is the
        // least (t, index) of the run below `closest`: a primitive listed before the
        // current winner may take an exact tie, tested with t_max one ulp above
        // closest. Boxes are padded, so no primitive the list loop accepts is culled
        // (DESIGN.md §4.7). A lane steps into the nearer entered child and stacks the
        // other; lanes that reach a leaf wait for the wave's others, so leaves are
        // tested together.
        typedef __attribute__((address_space(4))) const uint32_t cu32;
        for (uint32_t sg = 0; sg < sc.n_segs; ++sg) {
          const cu32* sp = (cu32*)(reinterpret_cast<uintptr_t>(sc.segs)) + 4u * __builtin_amdgcn_readfirstlane(sg);
          if (HAS_PLANE && sp[0]) {
            const uint32_t i = sp[3];
            const RecRef r4 = rec_at(sc.rec, i);  // scalar loads
            float t = 0.0f;
            const int r = plane_test(xyz(r4[0]), xyz(r4[1]), xyz(r4[2]), o, d, 0.001f, closest, t);
            if (r) t_last = t;
            if (r == 2) {
              closest = t;
              best = static_cast<int>(i);
            }
            continue;
          }
          uint32_t ref = sp[1];
          // this lane's next free traversal-stack entry as its LDS byte address (level-major:
          // one level is kBlock entries, kLevelB bytes); the stack is empty while it is in
          // level 0, and the entry below it is the sentinel row. (As an index, every read and
          // write cost an address add.)
          uint32_t tso = tbase + 4u * tid;
          // node slabs as fma(lo, inv, -o inv): a cull only, covered by the padding for
          // origins within the scene's reach (bvh.h bvh_origin_reach; the host checks the camera,
          // the ballot above every segment's origin).
          // The cull's reciprocal is clamped to +-2^100 (bvh.h kBvhInvClamp): an exact-zero
          // direction component (a lambertian bounce ((p + n) + r) - p at |p| ~ 5000 gives one
          // every few thousand scatters) has inv = +-inf, and fma(lo, inf, -(o inf)) is
          // inf - inf = NaN, which culled boxes the ray is inside. With the clamp, o inv is
          // finite and a slab that holds the ray's hit by the padding (>= 1e-4) stays
          // >= 1e-4 * 2^100 wide on that axis. (Today `inv` arrives clamped: a lane with
          // recip_box_ok3 has |inv| <= 2^100 and a wave without one clamps every lane above, so
          // the fmed3 changes no value; it keeps the cull right if that fallback ever changes.)
          const V3 invc{__builtin_amdgcn_fmed3f(inv.x, -kBvhInvClamp, kBvhInvClamp),
                        __builtin_amdgcn_fmed3f(inv.y, -kBvhInvClamp, kBvhInvClamp),
                        __builtin_amdgcn_fmed3f(inv.z, -kBvhInvClamp, kBvhInvClamp)};
          const V3 oinv{o.x * invc.x, o.y * invc.y, o.z * invc.z};
          while (ref != kBvhEnd) {
            while (ref < kBvhLeaf) {
              SEC(SC_NODE);
              DIAG_WAVE(DG_NODE_W);
              DIAG_LANE(DG_NODE_L);
#ifdef FR_DIAG
              {
                // distinct nodes among the walking lanes (1, 2, 3-4, more), and lanes of primary rays
                unsigned long long m_ = __ballot(1);
                uint32_t u_ = 0;
                while (m_ && u_ < 5) {
                  const uint32_t r_ = __builtin_amdgcn_readlane(ref, __ffsll(m_) - 1);
                  m_ &= ~__ballot(ref == r_);
                  ++u_;
                }
                if (u_ == 1) DIAG_WAVE(DG_NCOH_W);
                if (u_ == 2) DIAG_WAVE(DG_NU2_W);
                if (u_ == 3 || u_ == 4) DIAG_WAVE(DG_NU4_W);
                if (depth == 0) DIAG_LANE(DG_NPRIM_L);
              }
#endif
              // the stack's top, read before the node arrives (the sentinel kBvhEnd when the
              // stack is empty)
              typedef unsigned long long Mask;  // lane masks (ballots of single compares)
              const uint32_t tdown = tso - kLevelB;
              const uint32_t top = lds_u32_at(tdown);
              // the step's outcome, applied after the scalar or vector path (each path doing it
              // itself left a register copy of the stack position at the loop's latch)
              uint32_t t_near, t_far;
              Mask t_many, t_both;
              // internal node: both children's boxes; the nearer entered child next (the
              // left one on a tie) and the other stacked when both are entered; neither: the
              // stack's top (the sentinel ends the walk). Branch-free: the far child is written
              // to the free entry either way (a node at depth d has at most d entries below it,
              // d < kBvhStack) and the index moves only on a push or pop. (A ballot of an & of
              // compares went through a 0/1 VGPR and a compare: the compares' own masks are
              // combined with SALU ops.)
              auto node_pick = [&](const Slab& sl, const Slab& sr, const uint32_t cl, const uint32_t cr) {
                const Mask ml = __builtin_amdgcn_ballot_w64(sl.tn <= sl.tf) &
                                __builtin_amdgcn_ballot_w64(sl.tf >= 0.001f) & __builtin_amdgcn_ballot_w64(sl.tn <= closest);
                const Mask mr = __builtin_amdgcn_ballot_w64(sr.tn <= sr.tf) &
                                __builtin_amdgcn_ballot_w64(sr.tf >= 0.001f) & __builtin_amdgcn_ballot_w64(sr.tn <= closest);
                const Mask mgol = ml & (__builtin_amdgcn_ballot_w64(sl.tn <= sr.tn) | ~mr);
                const Mask many = ml | mr;
                // near = mgol ? cl : cr and far = the other, as xors with cl ^ cr: in the scalar
                // step cl and cr are SGPRs, and a select between two SGPRs needs one of them
                // copied to a VGPR first (one scalar operand per VALU instruction)
                const uint32_t cx = cl ^ cr;
                const uint32_t near = cl ^ lane_sel(mgol, 0u, cx);
                t_near = near;
                t_far = near ^ cx;
                t_many = many;
                t_both = ml & mr;
              };
              auto node_step = [&](const float4 na, const float4 nb, const float4 nc, const uint32_t cl,
                                   const uint32_t cr) {
                node_pick(slab3_fused(xyz(na), xyz(nb), oinv, invc),
                          slab3_fused(V3{na.w, nc.x, nc.y}, V3{nb.w, nc.z, nc.w}, oinv, invc), cl, cr);
              };
              const uint32_t ref0 = __builtin_amdgcn_readfirstlane(ref);
              if (__ballot(ref != ref0) == 0) {
                // every walking lane is at the same node (90 % of C5's node steps): scalar
                // loads, the slab arithmetic on SGPR operands (the distinct asm ends keep the
                // two paths from being merged over copies of the node into VGPRs). With vector
                // loads only, C5 trace 52.9 -> 62.3 ms: the vector memory path returns 64 B
                // per lane per step
                const RecRef nd = rec_at(sc.bvh, ref0);
                const float4 r = nd[3];
                SEC(SC_NODES);
                node_step(nd[0], nd[1], nd[2], __float_as_uint(r.x), __float_as_uint(r.y));
                asm volatile("; bvh node step: scalar");
              } else {
                SEC(SC_NODEV);
                const uint32_t nb0 = ref * 64u;  // node byte offset (< 2^32: nodes < 2^26)
                const uint4 nr = __builtin_bit_cast(uint4, buf_load4(sc.bvh, nb0 + 48u));
                node_step(buf_load4(sc.bvh, nb0), buf_load4(sc.bvh, nb0 + 16u), buf_load4(sc.bvh, nb0 + 32u), nr.x, nr.y);
                asm volatile("; bvh node step: vector");
              }
              SEC(SC_NODET);
              lds_u32_at(tso) = t_far;  // the far child
              const uint32_t tpop = lane_sel(t_many, tso, tdown);
              ref = lane_sel(t_many, t_near, top);
              tso = lane_sel(t_both, tso + kLevelB, tpop);
            }
            if (ref == kBvhEnd) break;
            SEC(SC_LEAF);
            DIAG_WAVE(DG_LEAF_W);
            DIAG_LANE(DG_LEAF_L);
            // leaf: slots [first, first + count) of the leaf-order records; one test of
            // primitive i (list index) whose leaf-order record r is at `slot`
            auto leaf_test = [&](const uint32_t i, const auto& r) {
              const float tmax =
                  static_cast<int>(i) < best ? __uint_as_float(__float_as_uint(closest) + 1u) : closest;
              const uint32_t k = KS == KS_AABB ? FR_AABB : KS == KS_SPHERE ? FR_SPHERE : __float_as_uint(r[3].w);
              float t = 0.0f;
              bool h = false;
              if (k == FR_SPHERE) {
                const float4 g = r[0];  // centre, RN(radius^2) (the leaf records' form)
                const SphereDisc q = sphere_disc_rr(xyz(g), g.w, o, d, a_dd);
                if (q.disc > 0.0f) {
                  SEC(SC_LROOT);
                  h = sphere_roots_fast(q, a_dd, ssg, 0.001f, tmax, t);
                }
              } else if (k == FR_AABB) {
                h = slab_root(slab3_box(xyz(r[0]), xyz(r[1]), o, inv, boinv), 0.001f, tmax, t);
              } else if (k == FR_TRIANGLE) {
                h = tri_root(xyz(r[0]), xyz(r[1]), xyz(r[2]), o, d, 0.001f, tmax, t);
              } else if (k == FR_OBB) {
                const float4 a = r[0], b = r[1], c = r[2], e = r[3];
                const ObbFrame f = obb_frame(xyz(a), xyz(b), xyz(c), xyz(e), o, d);
                h = slab_root(slab3(V3{-a.w, -b.w, -c.w}, V3{a.w, b.w, c.w}, f.ol, f.inv), 0.001f, tmax, t);
              }
              if (h) {
                closest = t;
                best = static_cast<int>(i);
                if (HAS_PLANE) t_last = t;
              }
            };
            const uint32_t first = ref & ((1u << kBvhSlotBits) - 1u);
            const uint32_t cnt = ((ref >> kBvhSlotBits) & 15u) + 1u;
            const uint32_t leaf0 = __builtin_amdgcn_readfirstlane(ref);
            if (__ballot(ref != leaf0) == 0) {
              // every lane at one leaf: its records through scalar loads
              typedef __attribute__((address_space(4))) const uint32_t cu32l;
              const cu32l* ord = (cu32l*)(reinterpret_cast<uintptr_t>(sc.bvh_order));
              const uint32_t first0 = leaf0 & ((1u << kBvhSlotBits) - 1u);
              const uint32_t cnt0 = ((leaf0 >> kBvhSlotBits) & 15u) + 1u;
              for (uint32_t kk = 0; kk < cnt0; ++kk) {
                SEC(SC_LTESTS);
                leaf_test(ord[first0 + kk], rec_at(sc.lrec, first0 + kk));
              }
              asm volatile("; bvh leaf: scalar");
            } else {
              for (uint32_t kk = 0; kk < cnt; ++kk) {
                SEC(SC_LTESTV);
                const uint32_t slot = first + kk;
                // buffer loads: 32-bit offsets from the arrays' bases (slots < 2^26)
                struct LeafRec {
                  const float4* base;
                  uint32_t off;
                  __device__ float4 operator[](uint32_t k) const { return buf_load4(base, off + 16u * k); }
                } const r{sc.lrec, slot * 64u};
                leaf_test(buf_load1(sc.bvh_order, slot * 4u), r);
              }
              asm volatile("; bvh leaf: vector");
            }
            tso -= kLevelB;  // pop (the sentinel kBvhEnd when the stack was empty)
            ref = lds_u32_at(tso);
          }
        }
      }
      // one primitive of kind K at list index i (wave-uniform), its record read through r4:
      // scalar loads (RecRef), or compile-time constants in the scene-specialised build
      auto test_rec = [&](auto kind_tag, uint32_t i, const auto& r4) {
        constexpr uint32_t K = decltype(kind_tag)::value;
        float t = 0.0f;
        bool h = false;
        if constexpr (K == FR_AABB) {
          h = slab_root(slab3_box(xyz(r4[0]), xyz(r4[1]), o, inv, boinv), 0.001f, closest, t);
        } else if constexpr (K == FR_SPHERE) {
          const float4 g = r4[0];
          h = sphere_root_fast(xyz(g), g.w, o, d, a_dd, ssg, 0.001f, closest, t);
        } else if constexpr (K == FR_PLANE) {
          const int r = plane_test(xyz(r4[0]), xyz(r4[1]), xyz(r4[2]), o, d, 0.001f, closest, t);
          if (r) t_last = t;
          h = r == 2;
        } else if constexpr (K == FR_TRIANGLE) {
          h = tri_root(xyz(r4[0]), xyz(r4[1]), xyz(r4[2]), o, d, 0.001f, closest, t);
        } else if constexpr (K == FR_OBB) {
          const float4 a = r4[0], b = r4[1], c = r4[2], e = r4[3];
          const ObbFrame f = obb_frame(xyz(a), xyz(b), xyz(c), xyz(e), o, d);
          h = slab_root(slab3(V3{-a.w, -b.w, -c.w}, V3{a.w, b.w, c.w}, f.ol, f.inv), 0.001f, closest, t);
        }
        if (h) {
          closest = t;
          best = static_cast<int>(i);
          if (HAS_PLANE) t_last = t;
        }
#if defined(FR_JIT_N) && defined(__HIP_DEVICE_COMPILE__)
        // scene-specialised list: the winner (and the last written t) settled after every
        // test; otherwise the compiler sinks the chain of selects into the shading step and
        // keeps every test's hit mask and t live until then (a 43-primitive list spilled
        // 64 SGPRs and 62 VGPRs)
        if constexpr (!std::is_same<typename std::decay<decltype(r4)>::type, RecRef>::value) {
          asm volatile("" : "+v"(best));
          if (HAS_PLANE) asm volatile("" : "+v"(t_last));
        }
#endif
      };
      auto test_one = [&](auto kind_tag, uint32_t i) {
        SEC(SC_LIST);
        test_rec(kind_tag, i, rec_at(sc.rec, i));
      };
      typedef std::integral_constant<uint32_t, FR_AABB> TagAabb;
      typedef std::integral_constant<uint32_t, FR_SPHERE> TagSphere;
#ifdef FR_JIT_N
      if constexpr (!BVH) {
        // Scene-specialised build (jit.cpp): the list in order, unrolled, every record a
        // compile-time constant. The tests and their order are the list loop's, so the
        // results are the same bits; what changes is that slab distances and other terms
        // two primitives share (a coordinate plane common to several boxes) are computed
        // once per segment, and no record is loaded.
        auto test_j = [&](auto ic) {
          constexpr uint32_t I = decltype(ic)::value;
          constexpr uint32_t K = kJitRec[I][15];
          if constexpr (jit_pair_axis(I) >= 0) {
            // boxes I and I + 1 are mirror images on one axis: one test in ray order and one
            // update at their place in the list (slab_pair_root, rt_core.h)
            float t = 0.0f;
            bool first = false;
            const JitRec<I> r4{};
            constexpr int AX = jit_pair_axis(I);
            const bool h = slab_pair_root<AX>(xyz(r4[0]), xyz(r4[1]), boinv, inv, 0.001f, closest, t, first);
            // selects, not a branch: the hit tests stay one basic block
            closest = h ? t : closest;
            best = h ? static_cast<int>(I + 1u) : best;
            best = (h & first) ? static_cast<int>(I) : best;
            if (HAS_PLANE) t_last = h ? t : t_last;
#if defined(__HIP_DEVICE_COMPILE__)
            asm volatile("" : "+v"(best));
            if (HAS_PLANE) asm volatile("" : "+v"(t_last));
#endif
          } else if constexpr (I > 0u && jit_pair_axis(I - 1u) >= 0) {
            // tested with box I - 1
          } else if constexpr (K == FR_AABB || K == FR_SPHERE || K == FR_PLANE || K == FR_TRIANGLE || K == FR_OBB) {
            test_rec(std::integral_constant<uint32_t, K>{}, I, JitRec<I>{});
          }
          // FR_STUB: never hits (aabb.rs:21-34, rectangle.rs:21-34)
        };
        unroll_below<0u, FR_JIT_N>(FR_JIT_N, test_j);
      } else
#endif
      if constexpr (NIB && !BVH && KS != KS_ANY) {
        // <= kNibbleMaxPrims primitives: the tests unrolled over the compile-time bound with
        // an exit at n, each index an inline constant (the winner select needs no index
        // register) and each record at a constant offset. C3 trace 17.45 -> 17.29 ms as a
        // counted loop with an exit, -> 16.95 ms unrolled; shard 0/8 -1.6 %
        auto test_k = [&](auto ic) {
          if constexpr (KS == KS_AABB)
            test_one(TagAabb{}, decltype(ic)::value);
          else
            test_one(TagSphere{}, decltype(ic)::value);
        };
        // n through an empty asm here: otherwise the 15 tests' exit conditions are hoisted
        // out of the lane loop as lane masks held (and spilled) in SGPRs
        uint32_t n_here = sc.n;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+s"(n_here));
#endif
        unroll_below<0u, kNibbleMaxPrims>(n_here, test_k);
      } else if constexpr (KS != KS_ANY) {
        for (uint32_t ii = 0; ii < (list_walk ? sc.n : 0u); ++ii) {
          // the index is wave-uniform; say so, or the compiler may fall back to vector loads
          const uint32_t i = __builtin_amdgcn_readfirstlane(ii);
          if constexpr (KS == KS_AABB)
            test_one(TagAabb{}, i);
          else
            test_one(TagSphere{}, i);
        }
      } else {
        // The list in order, as its kind runs: one scalar kind branch per run instead of a
        // dependent kind load and branch per primitive, and a tight loop per run whose
        // record loads do not wait on a kind test (the same tests in the same order).
        typedef __attribute__((address_space(4))) const uint32_t cu32r;
        for (uint32_t rr = 0; rr < (list_walk ? sc.n_runs : 0u); ++rr) {
          const cu32r* rp = (cu32r*)(reinterpret_cast<uintptr_t>(sc.runs)) + 4u * __builtin_amdgcn_readfirstlane(rr);
          const uint32_t k = rp[0], i0 = rp[1], i1 = rp[2];
          if (k == FR_AABB) {
            for (uint32_t i = i0; i < i1; ++i) test_one(TagAabb{}, __builtin_amdgcn_readfirstlane(i));
          } else if (k == FR_SPHERE) {
            for (uint32_t i = i0; i < i1; ++i) test_one(TagSphere{}, __builtin_amdgcn_readfirstlane(i));
          } else if (k == FR_PLANE) {
            for (uint32_t i = i0; i < i1; ++i)
              test_one(std::integral_constant<uint32_t, FR_PLANE>{}, __builtin_amdgcn_readfirstlane(i));
          } else if (k == FR_TRIANGLE) {
            for (uint32_t i = i0; i < i1; ++i)
              test_one(std::integral_constant<uint32_t, FR_TRIANGLE>{}, __builtin_amdgcn_readfirstlane(i));
          } else if (k == FR_OBB) {
            for (uint32_t i = i0; i < i1; ++i)
              test_one(std::integral_constant<uint32_t, FR_OBB>{}, __builtin_amdgcn_readfirstlane(i));
          }  // FR_STUB: never hits (aabb.rs:21-34, rectangle.rs:21-34)
        }
      }
      PROF_MARK(PF_HIT);
      SEC(SC_POSTHIT);
      if (best < 0) {
        SEC(SC_SKY);
        if (DEFER)
          // the sqrt and division by their core sequences under a range guard (sky_t_fast,
          // bit-identical to sky_t): C3 frame 15.52 -> 15.27 ms (in round 3, before the sum
          // ran beside the trace, it had measured neutral)
          tsky = __float_as_uint(sky_t_fast(d));  // tracer.rs:211-218, the blend in sum_kernel
        else
          term = sky(d);  // tracer.rs:211-218
        ended = true;
        have_ray = false;
      } else {
        DIAG_WAVE(DG_HIT_W);
        ++nhit;
        ended = true;  // unless a scatter continues the path
        tsky = kDeferAbsorbed;
        have_ray = false;
        if (NIB ? (dmask != 0u && (wnib & dmask) == dmask) : depth < kp.max_depth) {
          SEC(SC_SHADE);
          // the shared HitRecord: normal of the winner at its own t; p = point_at(last t written)
          const V3 pw = add(o, scl(closest, d));
          // the winner's record and class: LDS when staged (n_rec / n_att are uniform;
          // separate branches keep LDS and global reads in their own address spaces)
          float4 b0, b1, b2, b3;
          if (REC_LDS || n_rec) {
            const float4* rb = rec_lds + 4 * best;
            b0 = rb[0];
            b1 = rb[1];
            b2 = rb[2];
            b3 = rb[3];
          } else {
            const uint32_t off = 64u * static_cast<uint32_t>(best);
            b0 = buf_load4(sc.rec, off);
            b1 = buf_load4(sc.rec, off + 16u);
            b2 = buf_load4(sc.rec, off + 32u);
            b3 = buf_load4(sc.rec, off + 48u);
          }
          // (a single-kind scene has no stubs: with DIFFUSE every class scatters lambertian)
          const uint32_t c = (DIFFUSE && KS != KS_ANY) ? static_cast<uint32_t>(SC_LAMBERT)
                             : ATT_LDS || n_att        ? __float_as_uint(att_lds[best].w)
                                                       : buf_load1(sc.cls, 4u * best);
          const uint32_t kb = KS == KS_AABB ? FR_AABB : KS == KS_SPHERE ? FR_SPHERE : __float_as_uint(b3.w);
          V3 n;
          if (kb == FR_AABB) {
            n = slab_normal(slab3_box(xyz(b0), xyz(b1), o, inv, boinv), closest, d);
          } else if (kb == FR_SPHERE) {
            n = divs(sub(pw, xyz(b0)), b0.w);
          } else if (kb == FR_PLANE) {
            n = scl(-1.0f, xyz(b1));
          } else if (kb == FR_TRIANGLE) {
            // precomputed winding normal, turned to face the ray except for dielectric
            n = xyz(b3);
            if (c != SC_DIELECTRIC && dot(n, d) > 0.0f) n = scl(-1.0f, n);
          } else {
            const ObbFrame f = obb_frame(xyz(b0), xyz(b1), xyz(b2), xyz(b3), o, d);
            const Slab sl = slab3(V3{-b0.w, -b1.w, -b2.w}, V3{b0.w, b1.w, b2.w}, f.ol, f.inv);
            n = obb_normal(xyz(b1), xyz(b2), xyz(b3), sl, closest, f.dl);
          }
          const V3 p = HAS_PLANE ? add(o, scl(t_last, d)) : pw;
          // Written for every hit lane, so that only the rarer materials' values are set
          // under a branch (fewer register copies where the branches join): an absorbed
          // path (SC_NONE) ends here and its o, d and sbest are not read again.
          const V3 din = d;
          o = p;
          d = add(p, n);  // lambertian / light: target = (p + n) + rus
          sbest = static_cast<uint32_t>(best);
          smetal = !DIFFUSE && c == SC_METAL;
          ended = c == SC_NONE;
          if (c != SC_NONE && (DIFFUSE || c != SC_DIELECTRIC)) need = NEED_SPHERE;
          // a lambertian scatter always continues the path (sphere.rs:84-89): with only those
          // (and stubs, which end it above) the winner is pushed here, not held to the scatter
          if (NIB && DIFFUSE && c != SC_NONE) {
            if (BVH)
              push(buf_load1(sc.acls, 4u * static_cast<uint32_t>(best)));  // the winner's attenuation class
            else
              push(static_cast<uint32_t>(best));
          }
          if (!DIFFUSE && c == SC_DIELECTRIC) {
            // one draw, no rejection loop (sphere.rs:107-145)
            d = scatter_dielectric(din, n, rng);
            push(static_cast<uint32_t>(best));
            if (!NIB) ++depth;
            have_ray = true;
          } else if (smetal) {
            // metal: reflect(unit(d), n) + fuzz * rus
            sfuzz = sc.mat[best].w;
            sn = n;
            d = reflect(unit(din), n);
          }
        }
      }
    }
    PROF_MARK(PF_SHADE);
    SEC(SC_POSTSHADE);
    if (ended) {
      SEC(SC_END);
      // 3. attenuation * get_color(...) (tracer.rs:206-207), innermost first
      DIAG_WAVE(DG_END_W);
      DIAG_LANE(DG_END_L);
      V3 col = term;
      if (NIB) {
        col = V3{__uint_as_float(tsky), __uint_as_float(wnib), 0.0f};
        wnib = ~0u;  // the next sample starts empty
      } else if (DEFER) {
        const uint2 w = *drow;
        *drow = make_uint2(~0u, ~0u);  // the next sample starts empty
        col = V3{__uint_as_float(tsky), __uint_as_float(w.x), __uint_as_float(w.y)};
      } else if (MAXD > 0) {
        // One read brings the lane's 8 levels; empty ones point at the unit entry
        // (x * 1.0f == x), so the product a0*(a1*(...*term)) needs no per-level branch
        // and its reads do not wait on each other.
        const uint4 w = *hrow;
        *hrow = make_uint4(unit2, unit2, unit2, unit2);  // the next sample starts empty
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
        if (n_att) {
          const char* att_bytes = reinterpret_cast<const char*>(att_lds);
#pragma unroll
          for (int j = MAXD - 1; j >= 0; --j) {
            DIAG_WAVE(DG_UNW_W);
            const uint32_t off = (j & 1) ? (ws[j >> 1] >> 16) : (ws[j >> 1] & 0xFFFFu);  // byte offset
            col = mul(xyz(*reinterpret_cast<const float4*>(att_bytes + off)), col);
          }
        } else {
          // global attenuations: only the levels in use
#pragma unroll
          for (int j = MAXD - 1; j >= 0; --j)
            if (j < static_cast<int>(depth)) col = mul(xyz(sc.att[(ws[j >> 1] >> (16 * (j & 1))) & 0xFFFFu]), col);
        }
      } else {
        // An absorbed path (terminal colour +0) stays +0 through any chain of finite,
        // non-negative attenuations: skip its unwind (sc.att_nonneg is the host's check).
        const bool zero_term = (__float_as_uint(term.x) | __float_as_uint(term.y) | __float_as_uint(term.z)) == 0u;
        const int udepth = sc.att_nonneg && zero_term ? 0 : static_cast<int>(depth);
        if (n_att) {
          for (int j = udepth - 1; j >= 0; --j) {
            const uint32_t pi = stack[j * kBlock + tid];
            col = mul(xyz(att_lds[pi]), col);
          }
        } else {
          for (int j = udepth - 1; j >= 0; --j) col = mul(xyz(sc.att[stack[j * kBlock + tid]]), col);
        }
      }
      const uint32_t jj = s & (kBlockSamples - 1u);  // the sample's index in its block
      if (!staged) {
        out[WPS * jj] = col.x;
        out[WPS * jj + 1] = col.y;
        if (WPS == 3) out[WPS * jj + 2] = col.z;
      } else {
        // stage the colour; every STG-th sample of the block, and its last, go out together
        // (a group never spans sub-blocks: kparams.h)
        float* sl = stage + WPS * (jj & (STG - 1u));
        sl[0] = col.x;
        sl[1] = col.y;
        if (WPS == 3) sl[2] = col.z;
        const bool full = (jj & (STG - 1u)) == STG - 1u;
        if (full || s + 1u == s_end) {
          float* dst = out + WPS * (jj & ~(STG - 1u));
          if (full && kp.ks == kBlockSamples) {
            if constexpr ((WPS * STG) % 4u == 0u) {
              // 16-B aligned: item * 192 (128) B + a multiple of 48 (32) B
              const float4* src = reinterpret_cast<const float4*>(stage);
#pragma unroll
              for (uint32_t k = 0; k < WPS * STG / 4u; ++k) {
                reinterpret_cast<float4*>(dst)[k] = src[k];
#if defined(__HIP_DEVICE_COMPILE__)
                // 12-B records (three stores): each 16-B store follows its LDS read, not every
                // read first (registers)
                if (WPS * STG > 8u) asm volatile("" ::: "memory");
#endif
              }
            } else {
              // 8-B aligned: item * 192 B + a multiple of 24 B
              const float2* src = reinterpret_cast<const float2*>(stage);
#pragma unroll
              for (uint32_t k = 0; k < WPS * STG / 2u; ++k) reinterpret_cast<float2*>(dst)[k] = src[k];
            }
          } else {
            for (uint32_t k = 0; k < WPS * ((jj & (STG - 1u)) + 1u); ++k) dst[k] = stage[k];
          }
        }
      }
#ifdef FR_DIAG
      if (s + 1u == s_end && diag_tb < (1u << 20)) atomicAdd(&g_fr_tb_cost[diag_tb], nseg - diag_seg0);
#endif
      if (++s != s_end) need = NEED_JIT;  // next sample of the block, same stream (else: a new item)
    }
    PROF_MARK(PF_END);
    SEC(SC_LATCH);
  }

  // Per-wave counter reduction into the wave's own slot (plain stores): the waves leave
  // the drain within a fraction of a millisecond, and three returning atomics per wave on
  // one cache line queued long enough there to hold the kernel's end back.
  unsigned long long a = nseg, b = nhit, sct = 0;
  for (int m = 32; m > 0; m >>= 1) {
    a += __shfl_xor(a, m);
    b += __shfl_xor(b, m);
    sct += __shfl_xor(sct, m);
  }
  if (lane == 0) {
    unsigned long long* wc = kw.wave_counters + 3u * (blockIdx.x * (kBlock / 64u) + (tid >> 6));
    wc[0] = a;
    wc[1] = b;
    wc[2] = sct;
  }
#ifdef FR_SECCNT
  __syncthreads();
  if (tid < SC_N) atomicAdd(&kw.counters[4 + tid], static_cast<unsigned long long>(sec_cnt[tid]));
  if (tid < SC_N) atomicAdd(&kw.counters[32 + tid], static_cast<unsigned long long>(sec_cnt[SC_N + tid]));
#endif
#ifdef FR_PROF
  if (lane == 0)
    for (int k = 0; k < PF_N; ++k) atomicAdd(&kw.counters[20 + k], static_cast<unsigned long long>(pf_acc[k]));
#endif
#ifdef FR_DIAG
  if (lane == 0 && gw < 65536) {
    g_fr_wave_times[2 * gw + 1] = __builtin_amdgcn_s_memrealtime();
    g_fr_wave_iters[2 * gw + 1] = diag_iter;
  }
  __syncthreads();
  if (tid < DG_N) atomicAdd(&kw.counters[4 + tid], static_cast<unsigned long long>(dg[tid]));
#endif
}

}  // namespace fr
