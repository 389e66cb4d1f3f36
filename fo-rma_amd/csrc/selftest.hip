// selftest.hip — diagnostics kernels and their fr_selftest_* entry points: single device
// operations of rt_core.h and the trace kernel's arithmetic, checked by the tests against
// host IEEE results (tests/test_gpu_parity.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hipchk.h"
#include "rt_core.h"
#include "trace_kernel.h"

namespace fr {

KCam kcam_for_selftest(const fr_camera* cam);  // render.hip: the frame's own KCam of this camera

// Camera::get_ray by both forms (trace_kernel.h cam_ray, cam_ray_axial) for tuple i
__global__ void camray_kernel(KCam cm, const float* in, uint32_t n, uint32_t* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float kx = in[4 * i], ky = in[4 * i + 1], s = in[4 * i + 2], t = in[4 * i + 3];
  const CamLens rd = cam_lens(cm, kx, ky);
  const CamRay g = cam_ray(cm, rd, s, t), a = cam_ray_axial(cm, rd, s, t);
  const float w[12] = {g.o.x, g.o.y, g.o.z, g.d.x, g.d.y, g.d.z, a.o.x, a.o.y, a.o.z, a.d.x, a.d.y, a.d.z};
  for (int k = 0; k < 12; ++k) out[12 * i + k] = __float_as_uint(w[k]);
}

// The trace kernel's segment set-up (rt_core.h seg_box_inv) on direction i: its three box
// reciprocals' bits
__global__ void boxinv_kernel(const float* in, uint32_t n, uint32_t* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const V3 inv = seg_box_inv(V3{in[3 * i], in[3 * i + 1], in[3 * i + 2]});
  out[3 * i] = __float_as_uint(inv.x);
  out[3 * i + 1] = __float_as_uint(inv.y);
  out[3 * i + 2] = __float_as_uint(inv.z);
}

__global__ void ops_kernel(int op, const float* a, const float* b, uint32_t n, float* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = a[i], y = b[i];
  float r;
  switch (op) {
    case 0: r = x + y; break;
    case 1: r = x - y; break;
    case 2: r = x * y; break;
    case 3: r = x / y; break;
    case 4: r = sqrtf(x); break;
    case 5: r = schlick(x, y); break;
    case 6: r = static_cast<float>(to_u8(x)); break;
    case 7: r = unit(V3{x, y, 1.0f}).x; break;
    case 8: r = 1.0f / x; break;
    case 9: r = div_rn(x, y, 1.0f / y); break;  // the kernel's jitter division
    case 10: r = recip_nr_ok(x) ? recip_nr(x) : 1.0f / x; break;
    case 11: r = fmax3_num(x, y, b[(i + 1) % n]); break;  // vs fmaxf(fmaxf(x, y), z)
    case 12: r = fmin3_num(x, y, b[(i + 1) % n]); break;  // vs fminf(fminf(x, y), z)
    case 17: r = fmin_num(fmin_num(x, y), b[(i + 1) % n]); break;  // chained v_min_f32
    case 13: r = fmax_num(fmax_num(x, y), b[(i + 1) % n]); break;  // chained v_max_f32
    case 14: {  // sky_t_fast against sky_t on the direction (x, y, z = b[i + 1]): 0 when equal bits
      const V3 dv{x, y, b[(i + 1) % n]};
      r = __uint_as_float(__float_as_uint(sky_t_fast(dv)) ^ __float_as_uint(sky_t(dv)));
      break;
    }
    case 15: r = sky_t_fast(V3{x, y, b[(i + 1) % n]}); break;
    case 16: {
      // sphere_root_fast against sphere_root: thread 16k reads a[16k..16k+10] = centre,
      // radius, origin, direction, t_max (t_min = 0.001). 0: same verdict and t bits;
      // 1: verdicts differ; 2: both hit with different t
      if (i % 16u != 0u || i + 16u > n) {
        r = 0.0f;
        break;
      }
      const float* q = a + i;
      const V3 c{q[0], q[1], q[2]}, o{q[4], q[5], q[6]}, dv{q[7], q[8], q[9]};
      const float aa = dot(dv, dv);
      float t0 = 0.0f, t1 = 0.0f;
      const bool h0 = sphere_root(c, q[3], o, dv, aa, 0.001f, q[10], t0);
      const bool h1 = sphere_root_fast(c, q[3], o, dv, aa, sphere_seg(aa), 0.001f, q[10], t1);
      r = h0 != h1 ? 1.0f : (h0 && __float_as_uint(t0) != __float_as_uint(t1)) ? 2.0f : 0.0f;
      break;
    }
    default: r = 0.0f;
  }
  out[i] = r;
}

// Exhaustive check of recip_nr (rcp + one FMA Newton step) against the correctly
// rounded 1.0f / x over x = [base, base + count): per exponent field (256 buckets) the
// number of results whose bits differ (NaN == NaN) and the first such input.
__global__ void recip_check_kernel(uint64_t base, uint64_t count, unsigned long long* bad, uint32_t* first) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < count; i += stride) {
    const uint32_t bits = static_cast<uint32_t>(base + i);
    const float x = __uint_as_float(bits);
    const float want = 1.0f / x, got = recip_nr(x);
    const bool same = __float_as_uint(want) == __float_as_uint(got) || (want != want && got != got);
    if (!same) {
      const uint32_t e = (bits >> 23) & 0xFFu;
      atomicAdd(&bad[e], 1ull);
      atomicMin(&first[e], bits);
    }
  }
}

// Exhaustive check of div_rn against the correctly rounded a / b over the mantissa
// space: the threads take every a = 1 + i 2^-23 (all 2^23 of [1, 2)), the loop every
// b = 1 + m 2^-23 with m in [b_base, b_base + b_count), y = RN(1 / b). Division by powers
// of two on either operand scales both results exactly while no intermediate leaves the
// normal range, so [1, 2) x [1, 2) covers every use (rt_core.h div_rn). bad[0] counts the
// pairs whose bits differ, first[0] holds the least (m << 23 | i) of them.
__global__ void div_check_kernel(uint32_t b_base, uint32_t b_count, unsigned long long* bad,
                                 unsigned long long* first) {
  // four a per thread (i + j 2^21), so that each y = 1.0f / b serves four pairs
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (1u << 21)) return;
  unsigned long long nbad = 0, fbad = ~0ull;
  for (uint32_t k = 0; k < b_count; ++k) {
    const uint32_t m = b_base + k;
    const float b = __uint_as_float(0x3F800000u | m);
    const float y = 1.0f / b;
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      const uint32_t ia = i + (j << 21);
      const float a = __uint_as_float(0x3F800000u | ia);
      const float want = a / b, got = div_rn(a, b, y);
      if (__float_as_uint(want) != __float_as_uint(got)) {
        ++nbad;
        fbad = min(fbad, (static_cast<unsigned long long>(m) << 23) | ia);
      }
    }
  }
  if (nbad) {
    atomicAdd(bad, nbad);
    atomicMin(first, fbad);
  }
}

__global__ void rng_kernel(uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t n, uint32_t* out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  Rng r = rng_seed(seed, pixel, sample);
  for (uint32_t i = 0; i < n; ++i) out[i] = rng_next(r);
}

}  // namespace fr

using namespace fr;

extern "C" {

int fr_selftest_ops(int device, int op, const float* a, const float* b, uint32_t n, float* out) {
  if (!a || !b || !out) return set_error(FR_EARG, "fr_selftest_ops: null buffer");
  SET_DEVICE(device);
  float *da = nullptr, *db = nullptr, *dout = nullptr;
  const size_t bytes = (n ? n : 1) * sizeof(float);
  HIPCHK(hipMalloc(&da, bytes));
  HIPCHK(hipMalloc(&db, bytes));
  HIPCHK(hipMalloc(&dout, bytes));
  HIPCHK(hipMemcpy(da, a, n * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(db, b, n * sizeof(float), hipMemcpyHostToDevice));
  if (n) hipLaunchKernelGGL(ops_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, op, da, db, n, dout);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, dout, n * sizeof(float), hipMemcpyDeviceToHost));
  HIPCHK(hipFree(da));
  HIPCHK(hipFree(db));
  HIPCHK(hipFree(dout));
  return FR_OK;
}

int fr_selftest_rng(int device, uint64_t seed, uint32_t pixel, uint32_t sample, uint32_t n, uint32_t* out) {
  if (!out) return set_error(FR_EARG, "fr_selftest_rng: null buffer");
  SET_DEVICE(device);
  uint32_t* d = nullptr;
  HIPCHK(hipMalloc(&d, (n ? n : 1) * sizeof(uint32_t)));
  hipLaunchKernelGGL(rng_kernel, dim3(1), dim3(64), 0, 0, seed, pixel, sample, n, d);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, d, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIPCHK(hipFree(d));
  return FR_OK;
}

int fr_selftest_camray(int device, const fr_camera* cam, const float* in, uint32_t n, uint32_t* out) {
  if (!cam || !in || !out) return set_error(FR_EARG, "fr_selftest_camray: null argument");
  const KCam kc = kcam_for_selftest(cam);
  if (!(kc.lens_pre & kCamAxial)) return set_error(FR_EARG, "fr_selftest_camray: not an axial camera");
  SET_DEVICE(device);
  float* din = nullptr;
  uint32_t* dout = nullptr;
  HIPCHK(hipMalloc(&din, (n ? n : 1) * 4 * sizeof(float)));
  HIPCHK(hipMalloc(&dout, (n ? n : 1) * 12 * sizeof(uint32_t)));
  HIPCHK(hipMemcpy(din, in, n * 4 * sizeof(float), hipMemcpyHostToDevice));
  if (n) hipLaunchKernelGGL(camray_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, kc, din, n, dout);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, dout, n * 12 * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIPCHK(hipFree(din));
  HIPCHK(hipFree(dout));
  return FR_OK;
}

int fr_selftest_boxinv(int device, const float* in, uint32_t n, uint32_t* out) {
  if (!in || !out) return set_error(FR_EARG, "fr_selftest_boxinv: null argument");
  SET_DEVICE(device);
  float* din = nullptr;
  uint32_t* dout = nullptr;
  HIPCHK(hipMalloc(&din, (n ? n : 1) * 3 * sizeof(float)));
  HIPCHK(hipMalloc(&dout, (n ? n : 1) * 3 * sizeof(uint32_t)));
  HIPCHK(hipMemcpy(din, in, n * 3 * sizeof(float), hipMemcpyHostToDevice));
  if (n) hipLaunchKernelGGL(boxinv_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, din, n, dout);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out, dout, n * 3 * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIPCHK(hipFree(din));
  HIPCHK(hipFree(dout));
  return FR_OK;
}

/* Diagnostic: exhaustive recip_nr check over [base, base + count) bit patterns;
   bad[256] / first[256] per exponent field (first = 0xFFFFFFFF when none). */
int fr_selftest_recip(int device, uint64_t base, uint64_t count, uint64_t* bad, uint32_t* first) {
  if (!bad || !first || base + count > (1ull << 32)) return set_error(FR_EARG, "fr_selftest_recip: bad arguments");
  SET_DEVICE(device);
  unsigned long long* dbad = nullptr;
  uint32_t* dfirst = nullptr;
  HIPCHK(hipMalloc(&dbad, 256 * sizeof(unsigned long long)));
  HIPCHK(hipMalloc(&dfirst, 256 * sizeof(uint32_t)));
  HIPCHK(hipMemset(dbad, 0, 256 * sizeof(unsigned long long)));
  HIPCHK(hipMemset(dfirst, 0xFF, 256 * sizeof(uint32_t)));
  if (count) hipLaunchKernelGGL(recip_check_kernel, dim3(8192), dim3(256), 0, 0, base, count, dbad, dfirst);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(bad, dbad, 256 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(first, dfirst, 256 * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIPCHK(hipFree(dbad));
  HIPCHK(hipFree(dfirst));
  return FR_OK;
}

/* Diagnostic: div_rn against the IEEE division for every a mantissa and the b mantissas
   [b_base, b_base + b_count) (both operands in [1, 2)); *bad = differing pairs, *first =
   the least (b mantissa << 23 | a mantissa) among them (all ones when none). */
int fr_selftest_div(int device, uint32_t b_base, uint32_t b_count, uint64_t* bad, uint64_t* first) {
  if (!bad || !first || static_cast<uint64_t>(b_base) + b_count > (1ull << 23))
    return set_error(FR_EARG, "fr_selftest_div: bad arguments");
  SET_DEVICE(device);
  unsigned long long* d = nullptr;
  HIPCHK(hipMalloc(&d, 2 * sizeof(unsigned long long)));
  HIPCHK(hipMemset(d, 0, sizeof(unsigned long long)));
  HIPCHK(hipMemset(d + 1, 0xFF, sizeof(unsigned long long)));
  const uint32_t chunk = 512;  // b values per launch (2^32 pairs, a few ms)
  for (uint32_t k = 0; k < b_count; k += chunk) {
    hipLaunchKernelGGL(div_check_kernel, dim3((1u << 21) / 256), dim3(256), 0, 0, b_base + k,
                       min(chunk, b_count - k), d, d + 1);
    HIPCHK(hipGetLastError());
  }
  unsigned long long h[2];
  HIPCHK(hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost));
  HIPCHK(hipFree(d));
  *bad = h[0];
  *first = h[1];
  return FR_OK;
}

}  // extern "C"
