// accum_check.cpp — test harness (tests/test_accumulate_host.py): the continue / restart /
// overflow decision of progressive accumulation (fo-rma_amd/csrc/plan.cpp: accum_key,
// same_view, accum_step) as a CPU program, built with -fsanitize=address,undefined
// -fno-sanitize-recover=all. It walks one context's history frame by frame, the way
// render.hip does (the state moves only when a frame is accepted), and prints one JSON line
// per frame: {"case", "rc", "start", "frames", "samples"} and, for a refused frame, "error".
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/forma_rt.h"
#include "../../fo-rma_amd/csrc/internal.h"
#include "../../fo-rma_amd/csrc/plan.h"

// A host-only build makes no device copies of a scene.
namespace fr {
void release_device_copies(fr_scene* s) { s->copies.clear(); }
}  // namespace fr

static fr::AccumState g_state;

// One accumulating frame on the context: decided, and enqueued if accepted.
static int frame(const char* name, uint64_t uid, const fr_camera& cam, const fr_params& p) {
  fr::AccumStep step;
  const fr::AccumState before = g_state;
  const int rc = fr::accum_step(g_state, fr::accum_key(uid, cam, p), p.spp, &step);
  if (rc) {
    // a refused frame leaves the state as it was
    if (memcmp(&before.key, &g_state.key, sizeof before.key) != 0 || before.frames != g_state.frames ||
        before.samples != g_state.samples || before.live != g_state.live)
      return 1;
    printf("{\"case\": \"%s\", \"rc\": %d, \"error\": \"%s\", \"frames\": %u, \"samples\": %u}\n", name, rc,
           fr_last_error(), g_state.frames, g_state.samples);
    return 0;
  }
  if (!step.next.live) return 1;
  g_state = step.next;
  printf("{\"case\": \"%s\", \"rc\": 0, \"start\": %d, \"frames\": %u, \"samples\": %u}\n", name, step.start ? 1 : 0,
         g_state.frames, g_state.samples);
  return 0;
}

int main() {
  fr_camera cam;
  if (fr_camera_init(&cam, 33, 17) != FR_OK) return 2;
  fr_params p{};
  p.width = 33, p.height = 17, p.spp = 4, p.max_depth = 8, p.seed = 1, p.strip_rows = fr::kStripRows;
  p.shard_index = 0, p.shard_count = 1, p.flags = FR_FLAG_ACCUMULATE | FR_FLAG_WRITE_U8;
  if (fr::check_params(&p) != FR_OK) return 2;
  int bad = 0;
  bad |= frame("first", 7, cam, p);
  p.seed = 2;  // seed is not part of the view
  bad |= frame("continue", 7, cam, p);
  p.flags = FR_FLAG_ACCUMULATE;  // nor are the other flags
  bad |= frame("continue_other_flags", 7, cam, p);
  for (uint32_t spp : {1u, 16u, 2u}) {  // frames of different spp add up
    p.spp = spp;
    bad |= frame("mixed_spp", 7, cam, p);
  }
  p.spp = 4;
  bad |= frame("scene_upload", 8, cam, p);  // an edited scene is a new upload
  bad |= frame("continue", 8, cam, p);
  const float delta[3] = {0.25f, 0.0f, 0.0f};
  fr_camera_orbit(&cam, delta);
  bad |= frame("camera_orbit", 8, cam, p);
  bad |= frame("continue", 8, cam, p);
  // one bit of one camera field (the last of its 104 bytes' fields)
  uint32_t bits;
  memcpy(&bits, &cam.rotation, 4);
  bits ^= 1u;
  memcpy(&cam.rotation, &bits, 4);
  bad |= frame("camera_last_field_bit", 8, cam, p);
  cam.position[0] += 1.0f;
  bad |= frame("camera_first_field", 8, cam, p);
  p.width = 32;
  bad |= frame("width", 8, cam, p);
  p.height = 24;
  bad |= frame("height", 8, cam, p);
  p.max_depth = 50;
  bad |= frame("max_depth", 8, cam, p);
  p.shard_count = 2;
  bad |= frame("shard_count", 8, cam, p);
  p.shard_index = 1;
  bad |= frame("shard_index", 8, cam, p);
  bad |= frame("continue", 8, cam, p);
  g_state = fr::AccumState{};  // fr_ctx_accum_reset
  bad |= frame("reset", 8, cam, p);
  // the 32-bit sample count: 2^32 - 1 is reachable, one more is not
  g_state.samples = 0xFFFFFFFFu - 4u;
  bad |= frame("fill_to_limit", 8, cam, p);
  p.spp = 1;
  bad |= frame("overflow", 8, cam, p);
  p.spp = 0;
  bad |= frame("zero_spp_at_limit", 8, cam, p);
  p.spp = 1;
  p.max_depth = 8;  // a frame that restarts cannot overflow
  bad |= frame("restart_at_limit", 8, cam, p);
  // the flag with save_image_mt's bands is refused with the parameters
  p.flags = FR_FLAG_ACCUMULATE | FR_FLAG_MT_BANDS;
  printf("{\"case\": \"mt_bands\", \"rc\": %d, \"error\": \"%s\"}\n", fr::check_params(&p), fr_last_error());
  p.flags = FR_FLAG_MT_BANDS;
  printf("{\"case\": \"mt_bands_plain\", \"rc\": %d}\n", fr::check_params(&p));
  return bad;
}
