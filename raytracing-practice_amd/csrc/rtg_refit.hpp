// rtg_refit.hpp — launch parameters of rtg_scene_update's kernels (rtg_refit.hip), filled by rtg_api.cpp.
#pragma once
#include "rtg_internal.hpp"
#include "rtg_primbox.hpp"

namespace rtg {

// Stage 1: `count` updates; prims holds three float4 per update (rtg_prim_update: {p0, radius}, {p1, -}, {p2, -}).
struct UpdateArgs {
  const int32_t* indices;  // input primitive index of each update; null: update i is primitive i
  const float4* prims;
  int64_t count;
  int64_t num_prims;
  // the inverse of HostScene::prim_index: per input primitive its slot with the kind bits of a leaf reference
  // (kQuadRefBit, kTriRefBit), so the kind never changes
  const int32_t* slot_of;
  float4* spheres;
  float4* quads;
  float4* tris;
  float* tri_boxes;  // 6 floats per triangle slot, rounded outward
  int64_t num_spheres, num_quads, num_tris;
  // [0] the bits of the largest |coordinate| (a double) of the applied primitives' boxes, [1] updates left out
  // (degenerate triangle, non-finite value, index out of range); both zero before the launch
  unsigned long long* words;
};

// Stage 2: all child boxes of `num_nodes` W-wide nodes from the records, for the culling margin `pads`.
struct RefitArgs {
  float* nodes;
  int64_t num_nodes;
  const int32_t* refs;
  int64_t num_refs;
  const float4* spheres;
  const float4* quads;
  const float* tri_boxes;
  int64_t num_spheres, num_quads, num_tris;
  CullPads pads;
  int32_t* parent;    // per node: parent node * W + slot, -1 for the root (written by refit_parents_kernel)
  uint32_t* arrived;  // per node: children whose boxes are in place
};

hipError_t launch_update_records(const UpdateArgs& A, hipStream_t st);
hipError_t launch_refit(const RefitArgs& A, int width, hipStream_t st);

}  // namespace rtg
