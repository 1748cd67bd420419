// rtg_primbox.hpp — the fp32 culling box of one primitive record, as the device computes it: shared by the Morton
// builder (rtg_gpubvh.hip prim_bounds_kernel) and the refit of a live scene (rtg_refit.hip), so a refitted box is
// the box a device build of the same records would start from. One formula, two users.
#pragma once
#include "rtg_internal.hpp"

namespace rtg {

struct Box6 {
  float lo[3], hi[3];
};

// The culling margin of the host builder (rtg_api.cpp culling_box; DESIGN.md §4 "conservative culling"):
// each plane moves outward by c (|v| + M), c = 2^-21 for spheres, 2^-23 (1 + 2^-16) on an axis-aligned quad's
// flat axis and 2^-24 (6 U + 3 |v| + 2M) on its in-plane axes (U its extent there), 2^-18 on every axis of
// other quads and of triangles; here the M terms come from the host
// (pads, rounded up) and the |v| terms are doubled, so that the box's own fp32 arithmetic (centre +- r, the
// corner sums, the minimum extent, this subtraction: a few 2^-24 |v|) is covered as well
struct CullPads {
  float sphere, quad, flat, inplane;  // 2^-21 M, 2^-18 M, 2^-23 M (1 + 2^-16), 2^-23 M; rounded up
};
// M terms of the culling pads (m: M rounded up; power-of-two scalings are exact, the flat factor is rounded up by
// one ulp)
inline CullPads cull_pads(float m) {
  return CullPads{m * 0x1p-21f, m * 0x1p-18f, __builtin_nextafterf(m * 0x1p-23f * (1.0f + 0x1p-16f), __builtin_inff()),
                  m * 0x1p-23f};
}
__device__ __forceinline__ float pad_by(float v, float rel, float abs_pad) { return fabsf(v) * rel + abs_pad; }

// Box of one primitive record (the fp32 records the render kernels intersect), unpadded; thin axes other
// than an axis-aligned quad's flat one get the reference's 0.0001 minimum extent (aabb::pad_to_minimums,
// aabb.hpp:135-154).
// A triangle's box is its three vertices' (tri_boxes, 6 floats per slot: the plane-form record
// the kernels intersect does not hold the vertices).
__device__ inline Box6 prim_box(const float4* spheres, const float4* quads, const float* tri_boxes, int32_t ref, int* flat) {
  Box6 b;
  *flat = -1;
  if (ref & kTriRefBit) {
    const float* t = tri_boxes + static_cast<int64_t>(ref & kRefSlotMask) * 6;
    for (int k = 0; k < 3; ++k) b.lo[k] = t[k], b.hi[k] = t[3 + k];
  } else if (ref & kQuadRefBit) {
    const float4* q = quads + static_cast<int64_t>(ref & ~kQuadRefBit) * 5;
    const float4 Q = q[0], u = q[1], v = q[2], n = q[4];
    const float px[4] = {Q.x, Q.x + u.x, Q.x + v.x, Q.x + u.x + v.x};
    const float py[4] = {Q.y, Q.y + u.y, Q.y + v.y, Q.y + u.y + v.y};
    const float pz[4] = {Q.z, Q.z + u.z, Q.z + v.z, Q.z + u.z + v.z};
    b.lo[0] = fminf(fminf(px[0], px[1]), fminf(px[2], px[3]));
    b.lo[1] = fminf(fminf(py[0], py[1]), fminf(py[2], py[3]));
    b.lo[2] = fminf(fminf(pz[0], pz[1]), fminf(pz[2], pz[3]));
    b.hi[0] = fmaxf(fmaxf(px[0], px[1]), fmaxf(px[2], px[3]));
    b.hi[1] = fmaxf(fmaxf(py[0], py[1]), fmaxf(py[2], py[3]));
    b.hi[2] = fmaxf(fmaxf(pz[0], pz[1]), fmaxf(pz[2], pz[3]));
    // flat axis (rtg_api.cpp quad_flat_axis): u and v each along one coordinate axis, normal exactly +-e_k
    const int nu = (u.x != 0.0f) + (u.y != 0.0f) + (u.z != 0.0f), nv = (v.x != 0.0f) + (v.y != 0.0f) + (v.z != 0.0f);
    const int iu = u.x != 0.0f ? 0 : u.y != 0.0f ? 1 : 2, iv = v.x != 0.0f ? 0 : v.y != 0.0f ? 1 : 2;
    if (nu == 1 && nv == 1 && iu != iv) {
      const int k = 3 - iu - iv;
      const float nn[3] = {n.x, n.y, n.z};
      if (fabsf(nn[k]) == 1.0f && nn[iu] == 0.0f && nn[iv] == 0.0f) *flat = k;
    }
  } else {
    const float4 s0 = spheres[static_cast<int64_t>(ref) * 2];
    const float4 s1 = spheres[static_cast<int64_t>(ref) * 2 + 1];
    const float r = fabsf(s0.w);
    const float c0[3] = {s0.x, s0.y, s0.z};
    const float c1[3] = {s0.x + s1.x, s0.y + s1.y, s0.z + s1.z};
    for (int k = 0; k < 3; ++k) {
      b.lo[k] = fminf(c0[k], c1[k]) - r;
      b.hi[k] = fmaxf(c0[k], c1[k]) + r;
    }
  }
  for (int k = 0; k < 3; ++k) {
    if (b.hi[k] - b.lo[k] < 0.0001f && k != *flat) {  // a flat axis gets its own pad (pad_prim_box)
      b.lo[k] -= 0.00005f;
      b.hi[k] += 0.00005f;
    }
  }
  return b;
}

// The pad rule: moves every plane of prim_box's box outward by the culling margin of its primitive and axis.
// A triangle takes the pads of a quad that is not axis-aligned (flat < 0), as in culling_box.
__device__ inline void pad_prim_box(Box6* b, const float4* quads, int32_t ref, int flat, const CullPads& pads) {
  const bool quad = (ref & (kQuadRefBit | kTriRefBit)) != 0;
  float qu[3] = {0.0f, 0.0f, 0.0f}, qv[3] = {0.0f, 0.0f, 0.0f};
  if (ref & kQuadRefBit) {
    const float4* q = quads + static_cast<int64_t>(ref & ~kQuadRefBit) * 5;
    const float4 u = q[1], v = q[2];
    qu[0] = u.x, qu[1] = u.y, qu[2] = u.z, qv[0] = v.x, qv[1] = v.y, qv[2] = v.z;
  }
  for (int k = 0; k < 3; ++k) {
    // in-plane axis of an axis-aligned quad: 2^-24 (6 U_k + 3 |v| + 2M) as on the host, here 8 and 8 2^-24
    const bool inplane = quad && flat >= 0 && k != flat;
    const float rel = !quad || inplane ? 0x1p-20f : k == flat ? 0x1p-22f : 0x1p-17f;
    const float ab = !quad ? pads.sphere
                     : inplane ? fmaf(fabsf(qu[k]) + fabsf(qv[k]), 0x1p-21f, pads.inplane)
                     : k == flat ? pads.flat : pads.quad;
    b->lo[k] -= pad_by(b->lo[k], rel, ab);
    b->hi[k] += pad_by(b->hi[k], rel, ab);
  }
}

}  // namespace rtg
