// plan_check.cpp — test harness (tests/test_plan.py): the frame plan and the scene packer
// (fo-rma_amd/csrc/plan.cpp, pack.cpp) as a CPU program, built with
// -fsanitize=address,undefined -fno-sanitize-recover=all, printing what they decide.
//
//   plan_check plan KEY=VALUE...   one frame plan: the render parameters (w h spp depth
//                                  shard=i/n flags seed), the scene's facts (n kinds
//                                  has_plane bvh_ok n_segs bvh_levels bvh_extent bvh_sphere_rmin
//                                  diffuse n_aclass), the device (cus device_gib), the camera's reach
//                                  and the context's history (prev_in_flight streaming fs_n
//                                  fs_bytes dry); the knobs come from the environment
//   plan_check kernels             every specialisation select_kernel can reach, once each
//   plan_check strips H COUNT      the strip geometry of each shard, plain and MT bands
//   plan_check pack FILE...        each scene file (or "empty") through pack_scene
//   plan_check tuning              tuning_defines(): this build's tuning values as the #define
//                                  lines the scene kernel's run-time build starts with (plain text)
// One JSON line per case on stdout.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../include/forma_rt.h"
#include "../../fo-rma_amd/csrc/internal.h"
#include "../../fo-rma_amd/csrc/pack.h"
#include "../../fo-rma_amd/csrc/plan.h"

// A host-only build makes no device copies of a scene: fr_scene_free has none to release.
namespace fr {
void release_device_copies(fr_scene* s) { s->copies.clear(); }
}  // namespace fr

static int do_plan(int argc, char** argv) {
  std::map<std::string, std::string> kv;
  for (int i = 0; i < argc; ++i) {
    const char* eq = strchr(argv[i], '=');
    if (!eq) return 2;
    kv[std::string(argv[i], static_cast<size_t>(eq - argv[i]))] = eq + 1;
  }
  auto num = [&](const char* k, double dflt) { return kv.count(k) ? atof(kv[k].c_str()) : dflt; };
  auto u32 = [&](const char* k, uint32_t dflt) { return static_cast<uint32_t>(num(k, dflt)); };
  fr_params p{};
  p.width = u32("w", 64);
  p.height = u32("h", 36);
  p.spp = u32("spp", 4);
  p.max_depth = u32("depth", 8);
  p.seed = static_cast<uint64_t>(num("seed", 1));
  p.flags = u32("flags", 0);
  p.strip_rows = fr::kStripRows;
  p.shard_count = 1;
  if (kv.count("shard")) sscanf(kv["shard"].c_str(), "%u/%u", &p.shard_index, &p.shard_count);
  fr::SceneFacts sf;
  sf.n = u32("n", 6);
  sf.kinds = u32("kinds", 1u << FR_AABB);
  sf.has_plane = u32("has_plane", 0) != 0;
  sf.bvh_ok = u32("bvh_ok", 0) != 0;
  sf.n_segs = u32("n_segs", sf.bvh_ok ? 1 : 0);
  sf.bvh_levels = u32("bvh_levels", fr::kBvhStack);
  sf.bvh_extent = static_cast<float>(num("bvh_extent", 10.0));
  sf.bvh_sphere_rmin = static_cast<float>(num("bvh_sphere_rmin", -1.0));
  sf.diffuse = u32("diffuse", 1) != 0;
  sf.n_aclass = u32("n_aclass", 0);
  fr::PlanHistory hist;
  hist.prev_in_flight = u32("prev_in_flight", 0) != 0;
  hist.streaming = u32("streaming", 0) != 0;
  hist.fs_n = static_cast<int>(u32("fs_n", 0));
  hist.fs_bytes = static_cast<size_t>(num("fs_bytes", 0));
  const size_t device_bytes = static_cast<size_t>(num("device_gib", 256) * 1073741824.0);
  int rc = fr::check_params(&p);
  fr::FramePlan fp;
  if (!rc)
    rc = fr::make_plan(p, static_cast<float>(num("reach", 5.0)), sf, static_cast<int>(u32("cus", 256)), device_bytes,
                       fr::read_plan_env(), u32("dry", 0) != 0, hist, &fp);
  if (rc) {
    printf("{\"rc\": %d, \"error\": \"%s\"}\n", rc, fr_last_error());
    return 0;
  }
  const fr::KernelId id = fr::kernel_id(fp.sel);
  const fr::KParams& kp = fp.kp;
  printf("{\"rc\": 0, \"P\": %u, \"n_tiles\": %u, \"ks\": %u, \"flags\": %u, \"use_bvh\": %d, \"small_depth\": %d, "
         "\"defer\": %d, \"nibble\": %d, \"diffuse_k\": %d, \"bvh_nib\": %d, \"wps\": %u, \"per_block\": %zu, "
         "\"nblocks\": %u, \"nb_pass\": %u, \"cap_blocks\": %zu, \"passes\": %d, \"nfs\": %d, \"fpipe\": %d, "
         "\"overlap\": %d, \"stream_mode\": %d, \"relayout\": %d, \"reserve\": %u, \"slot_bytes\": %zu, \"slots\": %d, "
         "\"running_bytes\": %zu, \"lds\": %zu, \"stage_bytes\": %zu, \"jit_on\": %d, "
         "\"jit_wait\": %d, \"jit_cached_only\": %d, \"bvh_stage\": %d, \"max_wgs\": %u, \"kernel\": \"%s\", "
         "\"targs\": [%d, %d, %d, %d, %d, %d, %d, %d], \"pass\": [",
         kp.P, kp.n_tiles, kp.ks, kp.flags, fp.use_bvh, fp.small_depth, fp.defer, fp.nibble, fp.diffuse_k, fp.bvh_nib,
         fp.wps, fp.per_block, fp.nblocks, fp.nb_pass, fp.cap_blocks, fp.passes, fp.nfs, fp.fpipe, fp.fpipe_overlap,
         fp.stream_mode, fp.relayout, fp.reserve, fp.slot_bytes, fp.slots, fp.running_bytes, fp.lds, fp.stage_bytes,
         fp.jit_on, fp.jit_wait, fp.jit_cached_only, fp.bvh_stage, fp.max_wgs, id.name.c_str(), id.targs[0],
         id.targs[1], id.targs[2], id.targs[3], id.targs[4], id.targs[5], id.targs[6], id.targs[7]);
  for (int pass = 0; pass < fp.passes; ++pass) {
    const fr::PassPlan pp = fr::pass_plan(fp, pass);
    printf("%s[%u, %u, %u, %u, %u]", pass ? ", " : "", pp.b0, pp.nb, pp.n_items, pp.n_coarse, pp.b_fine);
  }
  printf("]}\n");
  return 0;
}

static int do_kernels() {
  std::set<std::string> seen;
  size_t inputs = 0;
  const uint32_t kind_sets[] = {1u << FR_AABB, 1u << FR_SPHERE, (1u << FR_AABB) | (1u << FR_SPHERE),
                                (1u << FR_SPHERE) | (1u << FR_PLANE), 1u << FR_TRIANGLE, 1u << FR_STUB, 0u};
  const uint32_t bits[] = {FR_FLAG_MT_BANDS, fr::KF_DEFER, fr::KF_NIBBLE, fr::KF_DIFFUSE};
  for (uint32_t kinds : kind_sets)
    for (int hp = 0; hp < 2; ++hp)
      for (int bvh = 0; bvh < 2; ++bvh)
        for (int small = 0; small < 2; ++small)
          for (uint32_t m = 0; m < 16; ++m) {
            uint32_t flags = 0;
            for (int k = 0; k < 4; ++k)
              if (m >> k & 1u) flags |= bits[k];
            const fr::KernelId id = fr::kernel_id(fr::KernelInputs{kinds, hp != 0, bvh != 0, small != 0, flags});
            ++inputs;
            if (id.name != fr::kernel_name(id.targs)) return 1;
            if (seen.insert(id.name).second)
              printf("{\"kernel\": \"%s\", \"targs\": [%d, %d, %d, %d, %d, %d, %d, %d]}\n", id.name.c_str(), id.targs[0],
                     id.targs[1], id.targs[2], id.targs[3], id.targs[4], id.targs[5], id.targs[6], id.targs[7]);
          }
  printf("{\"inputs\": %zu, \"distinct\": %zu}\n", inputs, seen.size());
  return 0;
}

static int do_strips(uint32_t height, uint32_t count) {
  for (int mt = 0; mt < 2; ++mt)
    for (uint32_t i = 0; i < count; ++i) {
      const fr::ShardStrips s = fr::shard_strips(height, i, count, mt != 0);
      printf("{\"H\": %u, \"shard\": %u, \"of\": %u, \"mt\": %d, \"strips\": %u, \"count\": %u, \"rows\": %llu, "
             "\"traced_rows\": %llu, \"full\": %u, \"has_partial\": %d, \"partial\": %u}\n",
             height, i, count, mt, s.strips, s.count, static_cast<unsigned long long>(s.rows),
             static_cast<unsigned long long>(s.traced_rows), s.full, s.has_partial, s.partial);
    }
  return 0;
}

static uint32_t word_at(const fr::PackedScene& ps, size_t off) {
  uint32_t w;
  memcpy(&w, &ps.bytes[off], 4);  // (a read past the blob is the sanitizer's to catch)
  return w;
}

static int do_pack(const char* path) {
  std::vector<fr_prim> prims;
  if (strcmp(path, "empty") != 0) {
    FILE* f = fopen(path, "rb");
    if (!f) return 2;
    std::string text;
    char buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
    fclose(f);
    fr_scene* scene = nullptr;
    fr_camera cam;
    if (fr_scene_from_json(text.data(), text.size(), 32, 18, &scene, &cam) != FR_OK) return 2;
    prims.resize(fr_scene_count(scene));
    if (!prims.empty()) fr_scene_get_prims(scene, prims.data(), static_cast<uint32_t>(prims.size()));
    fr_scene_free(scene);
  }
  const fr::PackedScene ps = fr::pack_scene(prims, false);
  const fr::SceneFacts& sf = ps.facts;
  const size_t offs[] = {ps.off_mat, ps.off_cls, ps.off_att,  ps.off_rec,  ps.off_bvh,     ps.off_bvh_order,
                         ps.off_lrec, ps.off_segs, ps.off_runs, ps.off_acls, ps.off_acls_att};
  printf("{\"file\": \"%s\", \"bytes\": %zu, \"offsets\": [", path, ps.bytes.size());
  for (size_t k = 0; k < sizeof offs / sizeof offs[0]; ++k) printf("%s%zu", k ? ", " : "", offs[k]);
  const bool rec_equal = ps.rec_words.size() == 16u * prims.size() &&
                         (prims.empty() || memcmp(ps.rec_words.data(), &ps.bytes[ps.off_rec], 64u * prims.size()) == 0);
  printf("], \"n\": %u, \"kinds\": %u, \"has_plane\": %d, \"bvh_ok\": %d, \"n_segs\": %u, \"bvh_levels\": %u, "
         "\"diffuse\": %d, \"n_aclass\": %u, \"att_nonneg\": %d, \"n_runs\": %u, \"rec_words\": %zu, "
         "\"rec_words_equal_region\": %d, \"att_n\": [%u, %u, %u, %u], \"rec0_kind\": %u, \"prims\": [",
         sf.n, sf.kinds, sf.has_plane, sf.bvh_ok, sf.n_segs, sf.bvh_levels, sf.diffuse, sf.n_aclass, ps.att_nonneg,
         ps.n_runs, ps.rec_words.size(), rec_equal ? 1 : 0, word_at(ps, ps.off_att + 16u * sf.n),
         word_at(ps, ps.off_att + 16u * sf.n + 4), word_at(ps, ps.off_att + 16u * sf.n + 8),
         word_at(ps, ps.off_att + 16u * sf.n + 12), word_at(ps, ps.off_rec + 60));
  for (size_t i = 0; i < prims.size(); ++i) {  // what the facts derive from: kind, material, colour bits
    uint32_t c[3];
    memcpy(c, prims[i].color, 12);
    printf("%s[%u, %u, %u, %u, %u]", i ? ", " : "", prims[i].kind, prims[i].material, c[0], c[1], c[2]);
  }
  printf("]}\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && strcmp(argv[1], "plan") == 0) return do_plan(argc - 2, argv + 2);
  if (argc == 2 && strcmp(argv[1], "kernels") == 0) return do_kernels();
  if (argc == 4 && strcmp(argv[1], "strips") == 0)
    return do_strips(static_cast<uint32_t>(atoi(argv[2])), static_cast<uint32_t>(atoi(argv[3])));
  if (argc == 2 && strcmp(argv[1], "tuning") == 0) return fputs(fr::tuning_defines().c_str(), stdout) < 0;
  if (argc >= 3 && strcmp(argv[1], "pack") == 0) {
    for (int i = 2; i < argc; ++i)
      if (do_pack(argv[i])) return 2;
    return 0;
  }
  fprintf(stderr, "usage: %s plan KEY=VALUE... | kernels | strips H COUNT | pack FILE... | tuning\n", argv[0]);
  return 2;
}
