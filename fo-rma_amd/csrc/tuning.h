// tuning.h — every build-time tuning knob of the device code, with its default and the
// measurement behind it. None of them changes what a kernel computes. A build overrides one
// with -DNAME=V (make variant DEFS=...); FR_TUNING names each knob once, and
// tuning_defines() (plan.cpp) forwards this build's values from it to the run-time build of
// the scene kernel, so the library, the scene kernel and the tools read one table.
//
// Compiles under g++, hipcc and hiprtc; no other file in csrc/ holds an #ifndef default.
#pragma once

// Rejection loop: lanes left to the next iteration (tuning only, results unchanged)
#ifndef FR_KREJ
#define FR_KREJ 4
#endif
// ... for the 8-B-record kernels (scenes of <= 15 primitives, the headline's): measured
// C3 trace 20.81 -> 20.69 ms at 6 (7 and 8 the same within noise); 6 on the other kernels
// cost C2 +1.7 % and a 10k-sphere BVH frame +1.2 %, so they keep FR_KREJ
// Re-tuned for the scene-specialised kernel (round 3): 9 with
// FR_CLAIM_MIN_NIB 3 streams C3 at 16.49 ms per frame against 16.63 (6 / 2), three runs;
// shard 0/8 unchanged (tools/gpu_knob_shards.sh, profiles/r03k_knob_shards.log)
#ifndef FR_KREJ_NIB
#define FR_KREJ_NIB 9
#endif
// ... for the BVH kernels with 8-B attenuation-class records: C5 trace 39.51 -> 39.17 ms at 2
// (0: 39.87, 1: 39.27, 3: 39.31, 6: 40.14; profiles/r06af_ab_c5_krej.log, four runs)
#ifndef FR_KREJ_BVH
#define FR_KREJ_BVH 2
#endif

// Lanes that must wait for an item before the wave claims (tuning only)
#ifndef FR_CLAIM_MIN
#define FR_CLAIM_MIN 1
#endif
// ... for the 8-B-record kernels (the headline's): C3 18.50 -> 18.28 ms at 2 (18.31 at 4, 18.46
// at 6); 4 on every kernel cost C2 +2 %, so the others keep FR_CLAIM_MIN
#ifndef FR_CLAIM_MIN_NIB
#define FR_CLAIM_MIN_NIB 3
#endif
#ifndef FR_CLAIM_MIN_BVH
#define FR_CLAIM_MIN_BVH FR_CLAIM_MIN
#endif

// The trace kernels' SGPR cap (amdgpu_num_sgpr; trace_kernel.h): measured on scene_08, 96
// beats 80 (fewer SGPR spills) and 102
#ifndef FR_NUM_SGPR
#define FR_NUM_SGPR 96
#endif

// Waves per SIMD the trace kernels ask for (amdgpu_waves_per_eu; trace_kernel.h has the
// list kernels' 7).
// The 8-B-record (headline) kernel at 8 waves: with FR_KREJ_NIB = 6, C3 trace 20.67 ->
// 20.49 ms and shard 0/4 -0.6 % (shard 0/8 +0.3 %); at KREJ 4 it had measured -0.3 % / +1.1 %
#ifndef FR_NIB_WAVES
#define FR_NIB_WAVES 8
#endif
// diffuse-only 12-B-record kernels
#ifndef FR_DIFF12_WAVES
#define FR_DIFF12_WAVES 7
#endif
// BVH kernels: 7 (72 VGPRs, one value spilled to scratch in the scatter step) over 6 (74
// VGPRs with the split scalar/vector node step): C5 trace 54.0 -> 51.4 ms
#ifndef FR_BVH_WAVES
#define FR_BVH_WAVES 7
#endif
// 0: the per-kernel values above; n > 0 forces n waves per SIMD on every trace kernel
#ifndef FR_MIN_WAVES
#define FR_MIN_WAVES 0
#endif

// sum_kernel: samples whose colour rebuilds interleave (the sums stay in order)
#ifndef FR_SUM_UNROLL
#define FR_SUM_UNROLL 2
#endif

// occlude_kernel's list loop (scene_walk.h AnyHit): primitives tested between two ballots that ask whether any lane of
// the wave is still unoccluded. 10,000 spheres through the list at 1080p, pixel rays / short
// bounce rays: 1: 8.07 / 5.39 ms, 8: 6.63 / 4.51 ms, 16: 6.25 / 4.25 ms, 64: 6.00 / 4.14 ms,
// 256: 6.15 / 4.11 ms
#ifndef FR_OCCL_EXIT_EVERY
#define FR_OCCL_EXIT_EVERY 64
#endif

// Every knob above, once.
#define FR_TUNING(X)    \
  X(FR_KREJ)            \
  X(FR_KREJ_NIB)        \
  X(FR_KREJ_BVH)        \
  X(FR_CLAIM_MIN)       \
  X(FR_CLAIM_MIN_NIB)   \
  X(FR_CLAIM_MIN_BVH)   \
  X(FR_NUM_SGPR)        \
  X(FR_NIB_WAVES)       \
  X(FR_DIFF12_WAVES)    \
  X(FR_BVH_WAVES)       \
  X(FR_MIN_WAVES)       \
  X(FR_SUM_UNROLL)      \
  X(FR_OCCL_EXIT_EVERY)
