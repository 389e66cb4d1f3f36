/* denoise_abi.c — a C consumer of include/forma_rt.h's denoise calls
   (tests/test_denoise_host.py), compiled as tests/c/accum_error_abi.c is: the three prototypes
   the Rust mirror of INTEGRATION.md assumes, checked from C and printed as JSON. */
#include <stdio.h>

#include "forma_rt.h"

int main(void) {
  /* the calls exist with these signatures, and refuse null handles without a device */
  int (*run)(fr_ctx*, uint32_t, float) = fr_ctx_denoise;
  int (*get)(fr_ctx*, float*, uint8_t*, float*) = fr_ctx_download_denoised;
  int (*buf)(fr_ctx*, float**, uint8_t**) = fr_ctx_denoised_buffers;
  const int rc[3] = {run(NULL, FR_DN_LEVELS_DEFAULT, FR_DN_K_DEFAULT), get(NULL, NULL, NULL, NULL), buf(NULL, NULL, NULL)};
  printf("{\"eps\": %.17g, \"mean_max\": %.17g, \"var_max\": %.17g, \"levels\": %u, \"k\": %.9g, "
         "\"abi_version\": %d, \"null_rc\": [%d, %d, %d]}\n",
         (double)FR_DN_EPS, (double)FR_DN_MEAN_MAX, (double)FR_DN_VAR_MAX, FR_DN_LEVELS_DEFAULT, (double)FR_DN_K_DEFAULT,
         fr_abi_version(), rc[0], rc[1], rc[2]);
  return 0;
}
