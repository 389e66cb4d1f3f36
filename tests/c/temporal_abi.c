/* temporal_abi.c — a C consumer of include/forma_rt.h's temporal-reuse calls
   (tests/test_temporal_host.py), compiled as tests/c/denoise_guided_abi.c is: the three prototypes,
   the constants and the options' layout that the Rust mirror of INTEGRATION.md assumes, checked
   from C and printed as JSON. */
#include <stddef.h>
#include <stdio.h>

#include "forma_rt.h"

int main(void) {
  /* the calls exist with these signatures, and refuse null handles without a device */
  int (*run)(fr_ctx*, uint32_t, float, const fr_denoise_guide*, const fr_temporal*) = fr_ctx_temporal;
  int (*reset)(fr_ctx*) = fr_ctx_temporal_reset;
  int (*get)(fr_ctx*, float*, float*, float*, float*, float*, float*, float*, float*, uint32_t*, uint32_t*) =
      fr_ctx_download_temporal;
  const int rc[3] = {run(NULL, FR_DN_LEVELS_DEFAULT, FR_DN_K_DEFAULT, NULL, NULL), reset(NULL),
                     get(NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL)};
  printf("{\"none\": %u, \"reasons\": [%u, %u, %u, %u, %u, %u, %u, %u], \"n_max\": %.9g, \"n_max_specular\": %.9g, "
         "\"n_max_max\": %.9g, \"sigma_z\": %.9g, \"normal_min\": %.9g, \"size\": %u, \"offsets\": [%u, %u, %u, %u, %u], "
         "\"abi_version\": %d, \"null_rc\": [%d, %d, %d]}\n",
         FR_TP_NONE, FR_TP_REUSED, FR_TP_NO_HISTORY, FR_TP_MISS, FR_TP_OFFSCREEN, FR_TP_ID, FR_TP_NORMAL, FR_TP_PLANE,
         FR_TP_HISTORY, (double)FR_TP_N_MAX_DEFAULT, (double)FR_TP_N_MAX_SPECULAR_DEFAULT, (double)FR_TP_N_MAX_MAX,
         (double)FR_TP_SIGMA_Z_DEFAULT, (double)FR_TP_NORMAL_MIN_DEFAULT, (unsigned)sizeof(fr_temporal),
         (unsigned)offsetof(fr_temporal, n_max), (unsigned)offsetof(fr_temporal, n_max_specular),
         (unsigned)offsetof(fr_temporal, sigma_z), (unsigned)offsetof(fr_temporal, normal_min),
         (unsigned)offsetof(fr_temporal, pad), fr_abi_version(), rc[0], rc[1], rc[2]);
  return 0;
}
