// mctx.cpp — the multi-device context, over the C ABI's single-device contexts.
//
// render_mt's row tiling over devices (tracer.rs:83-134).
// One fr_ctx per entry of the device list (duplicates allowed: two contexts on one device
// rehearse a two-device run), each rendering shard i of n of every frame; the shards'
// strips land in one page-locked host frame by asynchronous D2H copies, one per context.
// Everything is allocated at creation or on a frame of a larger size; a frame of the same
// size allocates nothing.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "hipchk.h"
#include "plan.h"

using namespace fr;

struct fr_mctx {
  std::vector<fr_ctx*> ctx;
  float* h_mean = nullptr;  // pinned full frame: W x H x 3 f32, then W x H x 3 u8
  uint8_t* h_u8 = nullptr;
  size_t cap_pixels = 0;
  uint32_t width = 0, height = 0;
  bool pending = false;
  std::chrono::steady_clock::time_point t0;
};

extern "C" {

void fr_mctx_free(fr_mctx* m) {
  if (!m) return;
  for (fr_ctx* c : m->ctx) fr_ctx_free(c);  // each drains its streams first
  if (m->h_mean) (void)hipHostFree(m->h_mean);
  delete m;
}

int fr_mctx_create(const int* devices, int n, fr_mctx** out) {
  if (!devices || n < 1 || !out) return set_error(FR_EARG, "fr_mctx_create: bad arguments");
  *out = nullptr;
  fr_mctx* m = new fr_mctx();
  for (int i = 0; i < n; ++i) {
    fr_ctx* c = nullptr;
    const int rc = fr_ctx_create(devices[i], nullptr, &c);
    if (rc) {
      const std::string msg = fr_last_error();
      fr_mctx_free(m);
      return set_error(rc, "fr_mctx_create: entry %d (device %d): %s", i, devices[i], msg.c_str());
    }
    m->ctx.push_back(c);
  }
  *out = m;
  return FR_OK;
}

int fr_mctx_count(const fr_mctx* m) { return m ? static_cast<int>(m->ctx.size()) : 0; }

int fr_mctx_ctx(fr_mctx* m, int i, fr_ctx** out) {
  if (!m || !out || i < 0 || i >= static_cast<int>(m->ctx.size())) return set_error(FR_EARG, "fr_mctx_ctx: bad index");
  *out = m->ctx[i];
  return FR_OK;
}

int fr_mctx_render(fr_mctx* m, fr_scene* scene, const fr_camera* cam, const fr_params* params) {
  if (!m || !scene || !cam || !params) return set_error(FR_EARG, "fr_mctx_render: null argument");
  const int n = static_cast<int>(m->ctx.size());
  fr_params p = *params;
  p.shard_count = static_cast<uint32_t>(n);
  p.shard_index = 0;
  int rc = check_params(&p);
  if (rc) return rc;
  const size_t pixels = static_cast<size_t>(p.width) * p.height;
  if (pixels > m->cap_pixels) {
    // a larger frame: the previous frame's gathers may still write the old host frame
    for (fr_ctx* c : m->ctx)
      if ((rc = fr_ctx_wait(c))) return rc;
    if (m->h_mean) HIPCHK(hipHostFree(m->h_mean));
    m->h_mean = nullptr;
    m->h_u8 = nullptr;
    m->cap_pixels = 0;
    void* h = nullptr;
    HIPCHK(hipHostMalloc(&h, pixels * 3 * (sizeof(float) + 1), hipHostMallocDefault));
    m->h_mean = static_cast<float*>(h);
    m->h_u8 = reinterpret_cast<uint8_t*>(m->h_mean + pixels * 3);
    m->cap_pixels = pixels;
  }
  m->width = p.width;
  m->height = p.height;
  m->t0 = std::chrono::steady_clock::now();
  // enqueue every shard and its gather, then return: the devices run concurrently
  // (params' flags go to every shard as they are: with FR_FLAG_ACCUMULATE each shard's context
  // accumulates its own strips, with FR_FLAG_ADAPTIVE it traces its own tile list)
  for (int i = 0; i < n; ++i) {
    p.shard_index = static_cast<uint32_t>(i);
    if ((rc = fr_ctx_render(m->ctx[i], scene, cam, &p))) return set_error(rc, "shard %d: %s", i, fr_last_error());
    if ((rc = fr_ctx_download_async(m->ctx[i], m->h_mean, (p.flags & FR_FLAG_WRITE_U8) ? m->h_u8 : nullptr)))
      return set_error(rc, "shard %d: %s", i, fr_last_error());
  }
  m->pending = true;
  return FR_OK;
}

int fr_mctx_sync(fr_mctx* m, fr_stats* stats) {
  if (!m) return set_error(FR_EARG, "fr_mctx_sync: null mctx");
  if (!m->pending) return set_error(FR_EARG, "fr_mctx_sync: nothing rendered");
  fr_stats agg;
  memset(&agg, 0, sizeof(agg));
  for (size_t i = 0; i < m->ctx.size(); ++i) {
    fr_stats st;
    int rc = fr_ctx_sync(m->ctx[i], &st);
    if (!rc) rc = fr_ctx_wait(m->ctx[i]);  // the shard's gather has landed
    if (rc) return set_error(rc, "shard %zu: %s", i, fr_last_error());
    agg.segments += st.segments;
    agg.hits += st.hits;
    agg.samples += st.samples;
    agg.prim_tests += st.prim_tests;
    agg.scatters += st.scatters;
    agg.kernel_ms = std::max(agg.kernel_ms, st.kernel_ms);  // the slowest shard
    agg.trace_ms = std::max(agg.trace_ms, st.trace_ms);
    agg.trace_launches = std::max(agg.trace_launches, st.trace_launches);
    agg.occupancy = st.occupancy;
  }
  agg.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - m->t0).count();
  if (stats) *stats = agg;
  return FR_OK;
}

int fr_mctx_frame(fr_mctx* m, const float** mean_rgb, const uint8_t** rgb8) {
  if (!m || !m->pending) return set_error(FR_EARG, "fr_mctx_frame: nothing rendered");
  if (mean_rgb) *mean_rgb = m->h_mean;
  if (rgb8) *rgb8 = m->h_u8;
  return FR_OK;
}

int fr_mctx_download(fr_mctx* m, float* mean_rgb, uint8_t* rgb8) {
  if (!m || !m->pending) return set_error(FR_EARG, "fr_mctx_download: nothing rendered");
  for (fr_ctx* c : m->ctx) {
    const int rc = fr_ctx_wait(c);
    if (rc) return rc;
  }
  const size_t n = static_cast<size_t>(m->width) * m->height * 3;
  if (mean_rgb) memcpy(mean_rgb, m->h_mean, n * sizeof(float));
  if (rgb8) memcpy(rgb8, m->h_u8, n);
  return FR_OK;
}

int fr_mctx_accum_reset(fr_mctx* m) {
  if (!m) return set_error(FR_EARG, "fr_mctx_accum_reset: null mctx");
  for (fr_ctx* c : m->ctx) {
    const int rc = fr_ctx_accum_reset(c);
    if (rc) return rc;
  }
  return FR_OK;
}

// Every shard sees the same scene, camera and parameters but its shard index, so all
// continue or restart together: shard 0's figures are every shard's.
int fr_mctx_accum_info(fr_mctx* m, uint32_t* frames, uint32_t* samples) {
  if (!m || m->ctx.empty()) return set_error(FR_EARG, "fr_mctx_accum_info: null mctx");
  return fr_ctx_accum_info(m->ctx[0], frames, samples);
}

// Every shard's estimate (fr_ctx_accum_error): counts add, the maximum is the shards' maximum,
// and each shard's rows of the map land in `rel`.
int fr_mctx_accum_error(fr_mctx* m, float threshold, fr_accum_error* out, float* rel) {
  if (!m || m->ctx.empty() || !out) return set_error(FR_EARG, "fr_mctx_accum_error: null argument");
  fr_accum_error agg;
  memset(&agg, 0, sizeof(agg));
  for (size_t i = 0; i < m->ctx.size(); ++i) {
    fr_accum_error e;
    int rc = fr_ctx_accum_error(m->ctx[i], threshold, &e);
    if (!rc && rel) rc = fr_ctx_download_error(m->ctx[i], rel);
    if (rc) return set_error(rc, "shard %zu: %s", i, std::string(fr_last_error()).c_str());
    if (i == 0) agg.frames = e.frames, agg.samples = e.samples;
    agg.pixels += e.pixels;
    agg.converged += e.converged;
    agg.max_rel = std::max(agg.max_rel, e.max_rel);  // (rel is never NaN)
  }
  agg.threshold = threshold;
  *out = agg;
  return FR_OK;
}

// Every shard's selection (fr_ctx_adapt): counts add, the maximum is the shards' maximum.
int fr_mctx_adapt(fr_mctx* m, float threshold, uint32_t min_samples, fr_adapt_info* out) {
  if (!m || m->ctx.empty() || !out) return set_error(FR_EARG, "fr_mctx_adapt: null argument");
  fr_adapt_info agg;
  memset(&agg, 0, sizeof(agg));
  for (size_t i = 0; i < m->ctx.size(); ++i) {
    fr_adapt_info e;
    const int rc = fr_ctx_adapt(m->ctx[i], threshold, min_samples, &e);
    if (rc) return set_error(rc, "shard %zu: %s", i, std::string(fr_last_error()).c_str());
    agg.frames = std::max(agg.frames, e.frames);
    agg.samples = std::max(agg.samples, e.samples);
    agg.tiles += e.tiles;
    agg.active_tiles += e.active_tiles;
    agg.pixels += e.pixels;
    agg.active_pixels += e.active_pixels;
    agg.converged += e.converged;
    agg.max_rel = std::max(agg.max_rel, e.max_rel);  // (rel is never NaN)
  }
  agg.threshold = threshold;
  agg.min_samples = min_samples;
  *out = agg;
  return FR_OK;
}

int fr_render_hip_multi(fr_scene* scene, const fr_camera* cam, const fr_params* params, int n_gpus,
                        float* mean_rgb, uint8_t* rgb8, fr_stats* stats) {
  if (!params || n_gpus < 1) return set_error(FR_EARG, "fr_render_hip_multi: bad arguments");
  if (params->flags & FR_FLAG_ACCUMULATE)
    return set_error(FR_EARG,
                     "fr_render_hip_multi: FR_FLAG_ACCUMULATE needs a context that outlives the call (fr_mctx_render)");
  int avail = 0;
  if (hipGetDeviceCount(&avail) != hipSuccess || avail < n_gpus)
    return set_error(FR_ENODEV, "fr_render_hip_multi: %d devices requested, %d present", n_gpus, avail);
  std::vector<int> devs(n_gpus);
  for (int g = 0; g < n_gpus; ++g) devs[g] = g;
  fr_mctx* m = nullptr;
  int rc = fr_mctx_create(devs.data(), n_gpus, &m);
  if (rc) return rc;
  fr_params p = *params;
  if (rgb8) p.flags |= FR_FLAG_WRITE_U8;
  rc = fr_mctx_render(m, scene, cam, &p);
  if (!rc) rc = fr_mctx_sync(m, stats);
  if (!rc) rc = fr_mctx_download(m, mean_rgb, rgb8);
  fr_mctx_free(m);
  return rc;
}

}  // extern "C"
