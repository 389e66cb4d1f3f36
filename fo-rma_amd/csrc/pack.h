// pack.h — a scene's device blob, built on the host without a device (pack.cpp): the
// tables the kernels read (KScene), 256-B aligned in one allocation, and what the frame
// plan needs to know about them (SceneFacts). render.hip uploads the bytes as they are.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/forma_rt.h"
#include "plan.h"
#include "refit.h"

namespace fr {

struct PackedScene {
  std::vector<unsigned char> bytes;  // the blob (released once uploaded)
  // byte offsets of the tables: material (rgb, fuzz), scatter class, attenuation (n + 1
  // entries: entry n is the unit), the 64-B records, BVH nodes, leaf order, the leaves'
  // records, segments, kind runs, attenuation class per primitive, the class table
  size_t off_mat = 0, off_cls = 0, off_att = 0;
  size_t off_rec = 0;
  size_t off_bvh = 0, off_bvh_order = 0, off_lrec = 0, off_segs = 0, off_runs = 0;
  size_t off_acls = 0, off_acls_att = 0;
  // the refit's tables (refit.h), after the others: each leaf slot's bounds, the slot of each
  // primitive (kNoSlot: none), the nodes' unpadded unions, the node ids by height
  size_t off_slot_bounds = 0, off_slot_of = 0, off_unions = 0, off_sched = 0;
  std::vector<uint32_t> slot_of;  // the host's copy of that table
  RefitSchedule sched;
  uint32_t n_slots = 0, n_nodes = 0;
  uint32_t n_runs = 0;
  bool att_nonneg = true;  // every attenuation component finite and >= +0 (no -0)
  SceneFacts facts;
  std::vector<uint32_t> rec_words;  // the n 64-B records as packed (the scene-specialised build's constants)
};

// force_bvh: build the BVH below the size/cost thresholds too (FR_BVH=1)
PackedScene pack_scene(const std::vector<fr_prim>& prims, bool force_bvh);

// One primitive's 64-B record as pack_scene writes it (kind bits in word 15; a triangle's normal
// is the host's unit(cross(e1, e2))), and the leaf record made of it (a sphere's carries RN(r r)).
void pack_record(const fr_prim& p, float rec[16]);
void leaf_record(const float rec[16], float lrec[16]);

}  // namespace fr
