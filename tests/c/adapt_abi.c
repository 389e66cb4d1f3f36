/* adapt_abi.c — a C consumer of include/forma_rt.h's fr_adapt_info (tests/test_adaptive_host.py),
   compiled as tests/c/accum_error_abi.c is: the layout the Rust mirror of INTEGRATION.md assumes,
   pinned at compile time and printed as JSON. */
#include <stddef.h>
#include <stdio.h>

#include "forma_rt.h"

_Static_assert(sizeof(fr_adapt_info) == 56, "fr_adapt_info is 56 bytes");
_Static_assert(FR_FLAG_ADAPTIVE == 128u, "flag");

#define FIELD(f) printf("\"%s\": [%zu, %zu], ", #f, offsetof(fr_adapt_info, f), sizeof(((fr_adapt_info*)0)->f))

int main(void) {
  /* the calls exist with these signatures, and refuse null handles without a device */
  int (*one)(fr_ctx*, float, uint32_t, fr_adapt_info*) = fr_ctx_adapt;
  int (*counts)(fr_ctx*, uint32_t*, uint32_t*) = fr_ctx_download_counts;
  int (*all)(fr_mctx*, float, uint32_t, fr_adapt_info*) = fr_mctx_adapt;
  fr_adapt_info e;
  const int rc[3] = {one(NULL, 0.5f, 0, &e), counts(NULL, NULL, NULL), all(NULL, 0.5f, 0, &e)};
  printf("{");
  FIELD(frames);
  FIELD(samples);
  FIELD(tiles);
  FIELD(active_tiles);
  FIELD(pixels);
  FIELD(active_pixels);
  FIELD(converged);
  FIELD(max_rel);
  FIELD(threshold);
  FIELD(min_samples);
  FIELD(pad);
  printf("\"sizeof\": %zu, \"flag\": %u, \"abi_version\": %d, \"null_rc\": [%d, %d, %d]}\n", sizeof(fr_adapt_info),
         FR_FLAG_ADAPTIVE, fr_abi_version(), rc[0], rc[1], rc[2]);
  return 0;
}
