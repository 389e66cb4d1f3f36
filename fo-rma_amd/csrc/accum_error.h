// accum_error.h — the per-pixel error estimate of a progressive accumulation
// (FR_FLAG_ACCUM_ERROR): its f32 arithmetic, shared by sum.hip's resolve, the
// error kernel (accum_error.hip) and a CPU program (tests/c/accum_error_check.cpp), and the
// launch of the error and summary kernels. Every named operation rounds once in f32; the
// build rules of rt_core.h hold (no contraction, IEEE '/' and sqrt).
#pragma once
#include <stdint.h>

#include "rt_core.h"

namespace fr {

// FR_ERR_FLOOR (forma_rt.h): the smallest denominator of the relative error, 2^-7, about half
// a u8 step of the summed channels
constexpr float kErrFloor = 0.0078125f;

// What a frame of spp samples and per-pixel sum s adds to the second-moment accumulator Q:
// RN(RN(s * s) / (float)spp). s has mean spp * mu and variance spp * sigma^2, so the sum of
// these over K frames, less A^2 / n, is (K - 1) sigma^2 in expectation for frames of any spp.
FR_HD float accum_sq_term(float s, float fspp) { return (s * s) / fspp; }
FR_HD V3 accum_sq_term(V3 s, float fspp) {
  return V3{accum_sq_term(s.x, fspp), accum_sq_term(s.y, fspp), accum_sq_term(s.z, fspp)};
}

// One channel: the mean m = A / n and the estimated per-sample variance
// max((Q - RN(A * m)) / (K - 1), 0); a NaN (A or Q not finite) reads 0.
FR_HD float accum_var(float a, float q, float fn, float fk, float& m) {
  m = a / fn;
  return fmax_num((q - a * m) / fk, 0.0f);
}

// The relative standard error of a pixel's mean, its three channels summed: fn = (float)n
// samples per pixel, fk = (float)(K - 1) for K >= 2 frames. err = sqrt(((v_r + v_g) + v_b) / fn)
// over den = max((m_r + m_g) + m_b, kErrFloor). Never NaN and never negative, so its bits
// order as uint32. A pixel whose summed mean is NaN or infinite reads 0: more frames do not
// change it, so there is nothing to wait for.
FR_HD float accum_rel_error(V3 a, V3 q, float fn, float fk) {
  float mr, mg, mb;
  const float vr = accum_var(a.x, q.x, fn, fk, mr);
  const float vg = accum_var(a.y, q.y, fn, fk, mg);
  const float vb = accum_var(a.z, q.z, fn, fk, mb);
  const float err = sqrtf(((vr + vg) + vb) / fn);
  const float msum = (mr + mg) + mb;
  const float den = fmax_num(msum, kErrFloor);
  // (msum - msum is 0 exactly for a finite msum, NaN otherwise)
  return (msum - msum) == 0.0f ? err / den : 0.0f;
}

}  // namespace fr

#if defined(__HIPCC__) || defined(__HIP__)
#include "kparams.h"

namespace fr {

// The summary the second kernel leaves on the device: 16 bytes.
struct ErrSummary {
  unsigned long long converged;  // pixels with rel <= threshold
  uint32_t max_bits;             // the largest rel, as its bits
  uint32_t pad;
};

// Enqueues the error kernel (one thread per pixel slot of kp's shard: rel to err_map[y * W + x])
// and the one-workgroup reduce of its per-workgroup {count, max} partials into *summary.
// partials: 2 x uint32 per workgroup of kSumThreads slots.
hipError_t launch_accum_error(hipStream_t stream, const KParams& kp, const float* accum, const float* sq, float fn,
                              float fk, float threshold, float* err_map, uint32_t* partials, ErrSummary* summary);

// fr_ctx_adapt's summary on the device: 32 bytes.
struct AdaptSummary {
  unsigned long long converged;      // pixels with rel <= threshold
  unsigned long long active_pixels;  // image pixels in the list's tiles
  uint32_t max_bits;                 // the largest rel, as its bits
  uint32_t active_tiles;             // the list's length
  uint32_t pad[2];
};

// The estimate of a tiled accumulation: rel from each tile's own n_t and K_t
// into err_map, then either (adapt) the selection, the ordered active tile list and *adapt,
// or (summary) accum_error_reduce's *summary. kp: the whole shard's constants.
// tile_pixels, list: one uint32 per tile of the shard.
hipError_t launch_adapt(hipStream_t stream, const KParams& kp, const float* accum, const float* sq,
                        const uint32_t* n_t, const uint32_t* k_t, float threshold, uint32_t min_samples,
                        float* err_map, uint32_t* partials, uint32_t* tile_pixels, uint32_t* list,
                        AdaptSummary* adapt, ErrSummary* summary);

}  // namespace fr
#endif
