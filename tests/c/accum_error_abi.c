/* accum_error_abi.c — a C consumer of include/forma_rt.h's fr_accum_error
   (tests/test_accum_error_host.py), compiled as tests/c/abi_consumer.c is: the layout the Rust
   mirror of INTEGRATION.md assumes, pinned at compile time and printed as JSON. */
#include <stddef.h>
#include <stdio.h>

#include "forma_rt.h"

_Static_assert(sizeof(fr_accum_error) == 32, "fr_accum_error is 32 bytes");
_Static_assert(offsetof(fr_accum_error, frames) == 0, "frames");
_Static_assert(offsetof(fr_accum_error, samples) == 4, "samples");
_Static_assert(offsetof(fr_accum_error, pixels) == 8, "pixels");
_Static_assert(offsetof(fr_accum_error, converged) == 16, "converged");
_Static_assert(offsetof(fr_accum_error, max_rel) == 24, "max_rel");
_Static_assert(offsetof(fr_accum_error, threshold) == 28, "threshold");
_Static_assert(FR_FLAG_ACCUM_ERROR == 64u && FR_FLAG_ACCUMULATE == 32u, "flags");

#define FIELD(f) printf("\"%s\": [%zu, %zu], ", #f, offsetof(fr_accum_error, f), sizeof(((fr_accum_error*)0)->f))

int main(void) {
  /* the calls exist with these signatures, and refuse null handles without a device */
  int (*one)(fr_ctx*, float, fr_accum_error*) = fr_ctx_accum_error;
  int (*map)(fr_ctx*, float*) = fr_ctx_download_error;
  int (*all)(fr_mctx*, float, fr_accum_error*, float*) = fr_mctx_accum_error;
  fr_accum_error e;
  const int rc[3] = {one(NULL, 0.5f, &e), map(NULL, NULL), all(NULL, 0.5f, &e, NULL)};
  printf("{");
  FIELD(frames);
  FIELD(samples);
  FIELD(pixels);
  FIELD(converged);
  FIELD(max_rel);
  FIELD(threshold);
  printf("\"sizeof\": %zu, \"flag\": %u, \"floor\": %.10g, \"abi_version\": %d, \"null_rc\": [%d, %d, %d]}\n",
         sizeof(fr_accum_error), FR_FLAG_ACCUM_ERROR, (double)FR_ERR_FLOOR, fr_abi_version(), rc[0], rc[1], rc[2]);
  return 0;
}
