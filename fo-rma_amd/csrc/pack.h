// pack.h — a scene's device blob, built on the host without a device (pack.cpp): the
// tables the kernels read (KScene), 256-B aligned in one allocation, and what the frame
// plan needs to know about them (SceneFacts). render.hip uploads the bytes as they are.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/forma_rt.h"
#include "plan.h"

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
  uint32_t n_runs = 0;
  bool att_nonneg = true;  // every attenuation component finite and >= +0 (no -0)
  SceneFacts facts;
  std::vector<uint32_t> rec_words;  // the n 64-B records as packed (the scene-specialised build's constants)
};

// force_bvh: build the BVH below the size/cost thresholds too (FR_BVH=1)
PackedScene pack_scene(const std::vector<fr_prim>& prims, bool force_bvh);

}  // namespace fr
