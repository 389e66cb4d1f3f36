/* denoise_guided_abi.c — a C consumer of include/forma_rt.h's G-buffer and guided-denoise calls
   (tests/test_denoise_guided_host.py), compiled as tests/c/denoise_abi.c is: the three
   prototypes and the guide's layout that the Rust mirror of INTEGRATION.md assumes, checked from
   C and printed as JSON. */
#include <stddef.h>
#include <stdio.h>

#include "forma_rt.h"

int main(void) {
  /* the calls exist with these signatures, and refuse null handles without a device */
  int (*gb)(fr_ctx*, fr_scene*, const fr_camera*, uint32_t, uint32_t) = fr_ctx_gbuffer;
  int (*get)(fr_ctx*, uint32_t*, float*, float*, float*, float*) = fr_ctx_download_gbuffer;
  int (*run)(fr_ctx*, uint32_t, float, const fr_denoise_guide*) = fr_ctx_denoise_guided;
  const int rc[3] = {gb(NULL, NULL, NULL, 1, 1), get(NULL, NULL, NULL, NULL, NULL, NULL),
                     run(NULL, FR_DN_LEVELS_DEFAULT, FR_DN_K_DEFAULT, NULL)};
  printf("{\"miss\": %u, \"feat_max\": %.17g, \"normal_max\": %.17g, \"alb_min\": %.17g, \"alb_max\": %.17g, "
         "\"sigma_z\": %.9g, \"normal_pow2\": %u, \"guide_size\": %u, \"guide_offsets\": [%u, %u, %u, %u], "
         "\"abi_version\": %d, \"null_rc\": [%d, %d, %d]}\n",
         FR_GBUFFER_MISS, (double)FR_DN_FEAT_MAX, (double)FR_DN_NORMAL_MAX, (double)FR_DN_ALB_MIN, (double)FR_DN_ALB_MAX,
         (double)FR_DN_SIGMA_Z_DEFAULT, FR_DN_NORMAL_POW2_DEFAULT, (unsigned)sizeof(fr_denoise_guide),
         (unsigned)offsetof(fr_denoise_guide, sigma_z), (unsigned)offsetof(fr_denoise_guide, normal_pow2),
         (unsigned)offsetof(fr_denoise_guide, demodulate), (unsigned)offsetof(fr_denoise_guide, pad), fr_abi_version(),
         rc[0], rc[1], rc[2]);
  return 0;
}
