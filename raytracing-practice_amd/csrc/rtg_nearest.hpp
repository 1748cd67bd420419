// rtg_nearest.hpp — what the proximity-query kernel families share (rtg_nearest.hip: rtg_closest_point, one winner
// per point; rtg_nearest_k.hip: rtg_closest_points, a sorted list of k per point): the distance tests, the node
// steps with their distance keys, the (code, d^2) stack pops and pushes, the record of one (point, primitive) pair,
// the scene copy of the LDS schedule and the counter flush. One copy, so both families compute the same d^2, prune
// by the same bound and write the same record for the same pair (DESIGN.md §3 "Proximity queries", §4).
#pragma once
#include <algorithm>
#include <cstdint>

#include "rtg_trav.hpp"

namespace rtg {

// rtg_nearest.hip: dynamic LDS of the whole-scene schedule (see there); `entries` counts 8-byte (code, bound) rows
// per lane, which is also the size of one candidate-list entry of rtg_nearest_k.hip
int nearest_lds_layout(const DevScene& S, int waves, int entries, DevNearest* Q);

namespace {

__device__ __forceinline__ uint64_t nballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ uint32_t nwave_sum(uint32_t x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

constexpr float kPointLimit = 1e30f;       // a coordinate of this magnitude or more: a miss for that point
constexpr uint32_t kNoPoint = 0xffffffffu;  // a lane's point index when it holds none
constexpr float kPruneRel = 1.0f + 0x1p-19f;
constexpr float kPruneAbs = 0x1p-120f;  // the denormal guard: lower bounds below it never prune
__device__ __forceinline__ float prune_bound(float best2) { return fmaf(best2, kPruneRel, kPruneAbs); }
__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

struct NearWave {
  uint32_t points = 0, found = 0;
  bool overflow = false, corrupt = false;
};

// Per-lane state of the walk
struct Near {
  V3 p;
  float time;
  // the walk's bound. rtg_closest_point: squared distance of the nearest primitive so far (starts at the query
  // radius squared). rtg_closest_points: the same until the lane's list is full, then its tail's squared distance
  float best2;
  int32_t best;  // rtg_closest_point: the nearest primitive's leaf reference, -1: none
  int32_t todo;  // inner node code (>= 0), leaf code (< 0) or kTravDone
  int32_t sp;
};

// ---- the distance tests: one fixed fp32 expression of d^2 per primitive kind -------------------------------------
// Sphere: | |p - c(time)| - |r| |, one square root. Large spheres (the render's kSphereF64Radius) form the
// difference in f64: in fp32 the shell distance of a point near a radius-30 sphere loses 2^-24 of the radius.
__device__ __forceinline__ float sphere_dist(float4 s0, float4 s1, V3 p, float time) {
  const V3 C = madd(time, xyz(s1), xyz(s0));
  const float r = fabsf(s0.w);
  if (r < kSphereF64Radius) {
    const V3 v = sub(p, C);
    return sqrtf(dot(v, v)) - r;
  }
  const double x = static_cast<double>(p.x) - static_cast<double>(C.x);
  const double y = static_cast<double>(p.y) - static_cast<double>(C.y);
  const double z = static_cast<double>(p.z) - static_cast<double>(C.z);
  return static_cast<float>(sqrt(x * x + y * y + z * z) - static_cast<double>(r));
}

// |hp - a u - b v|^2: the squared distance from p = Q + hp to the surface point (a, b)
__device__ __forceinline__ float plane_point_d2(V3 hp, V3 u, V3 v, float a, float b) {
  const V3 e = madd(-b, v, madd(-a, u, hp));
  return dot(e, e);
}

// Quad {Q, D}, {u, .}, {v, .}, {w, .}, {n, .}: the parallelogram Q + a u + b v, a, b in [0, 1]. (a, b) of p's
// projection from w as quad_t forms them; outside the parallelogram the nearest point lies on an edge whose
// constraint the projection violates (at most two: a's and b's), where it is the clamped projection onto that
// edge's line, from the Gram entries u.u, u.v, v.v formed here in fp32.
__device__ __forceinline__ float quad_near(const float4* q, V3 p, float& a, float& b) {
  const V3 u = xyz(q[1]), v = xyz(q[2]), w = xyz(q[3]);
  const V3 hp = sub(p, xyz(q[0]));
  const float pa = dot(w, cross(hp, v));
  const float pb = dot(w, cross(u, hp));
  const bool oa = !(pa >= 0.0f && pa <= 1.0f), ob = !(pb >= 0.0f && pb <= 1.0f);
  const float uv = dot(u, v);
  a = clamp01(pa);
  b = pb;
  if (oa) b = clamp01((dot(hp, v) - a * uv) / dot(v, v));
  float d2 = plane_point_d2(hp, u, v, a, b);
  if (ob) {
    const float b2 = clamp01(pb);
    const float a2 = clamp01((dot(hp, u) - b2 * uv) / dot(u, u));
    const float e2 = plane_point_d2(hp, u, v, a2, b2);
    if (!oa || e2 < d2) d2 = e2, a = a2, b = b2;
  }
  return d2;
}

// Triangle edge record {Q, u.u}, {u, u.v}, {v, v.v}: the vertex-based region walk (Ericson, Real-Time Collision
// Detection 5.1.5) over the vertex, edge and face regions from the six dot products of p - vertex with the two
// edges; those at Q + u and Q + v follow from the two at Q and u.u, u.v, v.v.
// The dot products and the three region determinants are formed in fp64 from the record's fp32 vertices: on a
// 1:100 sliver (u.u = 100, u.v = 50, v.v = 25.01) the determinants are differences of products near 2500 that
// leave about 1, which in fp32 (and already with the record's products, rounded to fp32) put the foot point 1.3e-5 S
// off on the first MI355X run. (s, t) are rounded once; d^2 is then the fp32 expression every kind shares.
__device__ __forceinline__ double ddot(double ax, double ay, double az, double bx, double by, double bz) {
  return ax * bx + ay * by + az * bz;
}
__device__ __forceinline__ float tri_near(const float4* E, V3 p, float& s, float& t) {
  const float4 e0 = E[0], e1 = E[1], e2 = E[2];
  const V3 u = xyz(e1), v = xyz(e2);
  const double ux = u.x, uy = u.y, uz = u.z, vx = v.x, vy = v.y, vz = v.z;
  const double ax = static_cast<double>(p.x) - static_cast<double>(e0.x);
  const double ay = static_cast<double>(p.y) - static_cast<double>(e0.y);
  const double az = static_cast<double>(p.z) - static_cast<double>(e0.z);
  const double uu = ddot(ux, uy, uz, ux, uy, uz), uv = ddot(ux, uy, uz, vx, vy, vz), vv = ddot(vx, vy, vz, vx, vy, vz);
  const double d1 = ddot(ux, uy, uz, ax, ay, az), d2 = ddot(vx, vy, vz, ax, ay, az);
  const double d3 = d1 - uu, d4 = d2 - uv;  // at Q + u
  const double d5 = d1 - uv, d6 = d2 - vv;  // at Q + v
  const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  double ds, dt;
  if (d1 <= 0.0 && d2 <= 0.0) {
    ds = 0.0, dt = 0.0;
  } else if (d3 >= 0.0 && d4 <= d3) {
    ds = 1.0, dt = 0.0;
  } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
    ds = d1 / uu, dt = 0.0;
  } else if (d6 >= 0.0 && d5 <= d6) {
    ds = 0.0, dt = 1.0;
  } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
    ds = 0.0, dt = d2 / vv;
  } else if (va <= 0.0 && d4 - d3 >= 0.0 && d5 - d6 >= 0.0) {
    dt = (d4 - d3) / ((d4 - d3) + (d5 - d6));
    ds = 1.0 - dt;
  } else {
    const double den = 1.0 / (va + vb + vc);
    ds = vb * den, dt = vc * den;
  }
  s = clamp01(static_cast<float>(ds));
  t = clamp01(static_cast<float>(dt));
  return plane_point_d2(sub(p, xyz(e0)), u, v, s, t);
}

// d^2 of the primitive behind a leaf reference
__device__ __forceinline__ float prim_d2(const DevScene& S, const float4* edges, int32_t ref, V3 p, float time) {
  float a, b;
  if (ref & kTriRefBit) return tri_near(edges + static_cast<int64_t>(ref & kRefSlotMask) * 3, p, a, b);
  if (ref & kQuadRefBit) return quad_near(S.quads + static_cast<int64_t>(ref & ~kQuadRefBit) * 5, p, a, b);
  const float4* s = S.spheres + static_cast<int64_t>(ref) * S.sphere_f4;
  const float d = sphere_dist(s[0], s[1], p, time);
  return d * d;
}

// the slot-table entry of a reference: sphere slots, then quad slots, then triangle slots
__device__ __forceinline__ int64_t ref_entry(const DevScene& S, int32_t ref) {
  if (ref & kTriRefBit) return S.num_spheres + S.num_quads + (ref & kRefSlotMask);
  if (ref & kQuadRefBit) return S.num_spheres + (ref & ~kQuadRefBit);
  return ref;
}

// The next stack entry whose lower bound still passes; entries the bound has overtaken are dropped without a
// look at their nodes.
template <class Stk>
__device__ __forceinline__ void near_pop(Near& t, const Stk& sc, const Stk& sb) {
  const float bound = prune_bound(t.best2);
  t.todo = kTravDone;
  while (t.sp > 0) {
    --t.sp;
    if (!(__int_as_float(sb.load(t.sp)) > bound)) {
      t.todo = sc.load(t.sp);
      break;
    }
  }
}

// The key of a child: the bits of its box's d^2 (non-negative floats order as their bits), ~0 for an empty slot
// or a box past the bound.
__device__ __forceinline__ uint32_t near_key(V3 p, float lox, float loy, float loz, float hix, float hiy, float hiz,
                                             int32_t code, float bound) {
  const float dx = fmaxf(fmaxf(lox - p.x, p.x - hix), 0.0f);
  const float dy = fmaxf(fmaxf(loy - p.y, p.y - hiy), 0.0f);
  const float dz = fmaxf(fmaxf(loz - p.z, p.z - hiz), 0.0f);
  const float d2 = dx * dx + dy * dy + dz * dz;
  return (code != kEmptyChild && !(d2 > bound)) ? __float_as_uint(d2) : ~0u;
}

template <class Stk>
__device__ __forceinline__ bool near_push(Near& t, const Stk& sc, const Stk& sb, int32_t code, uint32_t key) {
  if (t.sp >= sc.capacity()) return false;
  sc.store(t.sp, code);
  sb.store(t.sp, static_cast<int32_t>(key));
  ++t.sp;
  return true;
}

// One 4-wide node (rows lo.x, lo.y, lo.z, hi.x, hi.y, hi.z, code): from LDS (kGeomLds, codes are absolute LDS
// addresses) or through the caches (kGeomGlobal, codes are byte offsets into the node array).
template <class Stk, int GEOM>
__device__ __forceinline__ void near_node4(Near& t, const DevScene& S, const Stk& sc, const Stk& sb, NearWave& w) {
  if (t.todo >= S.node_limit) {  // corrupt child code: report, never read out of bounds
    w.corrupt = true;
    t.todo = kTravDone;
    return;
  }
  nf4 lx, ly, lz, hx, hy, hz;
  int4 cc;
  if constexpr (GEOM == kGeomLds) {
    const uint32_t na = static_cast<uint32_t>(t.todo);
    lx = lds_ld4(na), ly = lds_ld4(na + 16), lz = lds_ld4(na + 32);
    hx = lds_ld4(na + 48), hy = lds_ld4(na + 64), hz = lds_ld4(na + 80);
    const nf4 c4 = lds_ld4(na + 96);
    cc = *reinterpret_cast<const int4*>(&c4);
  } else {
    const char* nb = reinterpret_cast<const char*>(S.nodes) + t.todo;
    auto row = [&](int32_t off) -> nf4 { return *reinterpret_cast<const nf4*>(nb + off); };
    lx = row(0), ly = row(16), lz = row(32), hx = row(48), hy = row(64), hz = row(80);
    cc = *reinterpret_cast<const int4*>(nb + 96);
  }
  const float bound = prune_bound(t.best2);
  int32_t c0 = cc.x, c1 = cc.y, c2 = cc.z, c3 = cc.w;
  uint32_t k0 = near_key(t.p, lx.x, ly.x, lz.x, hx.x, hy.x, hz.x, c0, bound);
  uint32_t k1 = near_key(t.p, lx.y, ly.y, lz.y, hx.y, hy.y, hz.y, c1, bound);
  uint32_t k2 = near_key(t.p, lx.z, ly.z, lz.z, hx.z, hy.z, hz.z, c2, bound);
  uint32_t k3 = near_key(t.p, lx.w, ly.w, lz.w, hx.w, hy.w, hz.w, c3, bound);
  psort(k0, c0, k1, c1);
  psort(k2, c2, k3, c3);
  psort(k0, c0, k2, c2);
  psort(k1, c1, k3, c3);
  psort(k1, c1, k2, c2);
  if (k0 == ~0u) {
    near_pop(t, sc, sb);
    return;
  }
  // far to near, so the nearest sibling is popped first; a full stack is reported, never written past
  bool ok = true;
  if (k3 != ~0u) ok = near_push(t, sc, sb, c3, k3) && ok;
  if (k2 != ~0u) ok = near_push(t, sc, sb, c2, k2) && ok;
  if (k1 != ~0u) ok = near_push(t, sc, sb, c1, k1) && ok;
  if (!ok) w.overflow = true;
  t.todo = c0;
}

// One child-pair node (RTG_BVH_MEDIAN): left lo = (a.x, a.y, a.z), hi = (a.w, b.x, b.y); right lo = (b.z, b.w,
// c.x), hi = (c.y, c.z, c.w); codes are node indices. Two boxes, one compare.
template <class Stk>
__device__ __forceinline__ void near_node2(Near& t, const DevScene& S, const Stk& sc, const Stk& sb, NearWave& w) {
  if (t.todo >= S.num_nodes) {
    w.corrupt = true;
    t.todo = kTravDone;
    return;
  }
  const float4* n = S.nodes + static_cast<int64_t>(t.todo) * 4;
  const float4 a = n[0], b = n[1], c = n[2];
  const int4 ch = *reinterpret_cast<const int4*>(n + 3);
  const float bound = prune_bound(t.best2);
  int32_t c0 = ch.x, c1 = ch.y;
  uint32_t k0 = near_key(t.p, a.x, a.y, a.z, a.w, b.x, b.y, c0, bound);
  uint32_t k1 = near_key(t.p, b.z, b.w, c.x, c.y, c.z, c.w, c1, bound);
  psort(k0, c0, k1, c1);
  if (k0 == ~0u) {
    near_pop(t, sc, sb);
    return;
  }
  if (k1 != ~0u && !near_push(t, sc, sb, c1, k1)) w.overflow = true;
  t.todo = c0;
}

// The record of point p against the primitive behind `ref`, at distance `dist`: the primitive's test once more for
// (a, b), then point and side; the input index from the slot table.
__device__ __forceinline__ void nearest_record(const DevScene& S, const DevNearest& Q, int32_t ref, V3 p, float time,
                                               float dist, float4& o0, float4& o1) {
  V3 pt;
  float u, v;
  bool out;
  if (ref & (kTriRefBit | kQuadRefBit)) {
    V3 q0, e1, e2, n;
    if (ref & kTriRefBit) {
      const int64_t slot = ref & kRefSlotMask;
      const float4* E = Q.edges + slot * 3;
      tri_near(E, p, u, v);
      q0 = xyz(E[0]), e1 = xyz(E[1]), e2 = xyz(E[2]);
      n = xyz(S.tris[slot * 3]);
    } else {
      const float4* q = S.quads + static_cast<int64_t>(ref & ~kQuadRefBit) * 5;
      quad_near(q, p, u, v);
      q0 = xyz(q[0]), e1 = xyz(q[1]), e2 = xyz(q[2]);
      n = xyz(q[4]);
    }
    pt = madd(v, e2, madd(u, e1, q0));
    out = dot(n, sub(p, q0)) > 0.0f;
  } else {
    const float4* s = S.spheres + static_cast<int64_t>(ref) * S.sphere_f4;
    const float4 s0 = s[0], s1 = s[1];
    const V3 C = madd(time, xyz(s1), xyz(s0));
    const V3 d = sub(p, C);
    const float len = sqrtf(dot(d, d));
    // p at the centre: the shell point along +x
    const V3 outward = len > 0.0f ? scl(1.0f / len, d) : v3(1.0f, 0.0f, 0.0f);
    pt = madd(fabsf(s0.w), outward, C);
    out = sphere_dist(s0, s1, p, time) > 0.0f;
    // get_sphere_uv, in the spec functions write_hit uses
    const float theta = acos_spec(-outward.y);
    const float phi = atan2_spec(-outward.z, outward.x) + kPi;
    u = div_rn(phi, 2.0f * kPi);
    v = div_rn(theta, kPi);
  }
  o0 = make_float4(dist, __int_as_float(Q.prim_index[ref_entry(S, ref)]), u, v);
  o1 = make_float4(pt.x, pt.y, pt.z, __int_as_float(out ? 1 : -1));
}

// Schedule 3: the workgroup's copy of the scene in dynamic LDS at the launch's offsets: nodes (inner codes rebased
// to absolute LDS addresses), sphere records at a 48-byte stride, quad and triangle edge records, leaf references.
// L and N are S and Q pointing at the copies; the caller's __syncthreads() publishes them.
__device__ __forceinline__ void nearest_scene_to_lds(const DevScene& S, const DevNearest& Q, unsigned char* smem,
                                                     DevScene& L, DevNearest& N) {
  const int fill = static_cast<int>(blockDim.x);
  const uint32_t lds_base =
      static_cast<uint32_t>(reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) unsigned char*)smem));
  float4* l_nodes = reinterpret_cast<float4*>(smem + Q.lds_nodes);
  const int32_t rebase = static_cast<int32_t>(lds_base) + Q.lds_nodes;
  for (int64_t k = threadIdx.x; k < S.num_nodes * 7; k += fill) {
    float4 v = S.nodes[k];
    if (k % 7 == 6) {  // code row
      int4 c = *reinterpret_cast<int4*>(&v);
      c.x = c.x >= 0 ? c.x + rebase : c.x;
      c.y = c.y >= 0 ? c.y + rebase : c.y;
      c.z = c.z >= 0 ? c.z + rebase : c.z;
      c.w = c.w >= 0 ? c.w + rebase : c.w;
      v = *reinterpret_cast<float4*>(&c);
    }
    l_nodes[k] = v;
  }
  float4* l_spheres = reinterpret_cast<float4*>(smem + Q.lds_spheres);  // 48-byte stride, as the ray query's copy
  float4* l_quads = reinterpret_cast<float4*>(smem + Q.lds_quads);
  float4* l_edges = reinterpret_cast<float4*>(smem + Q.lds_edges);
  int32_t* l_refs = reinterpret_cast<int32_t*>(smem + Q.lds_refs);
  for (int64_t k = threadIdx.x; k < S.num_spheres * 2; k += fill) l_spheres[(k >> 1) * 3 + (k & 1)] = S.spheres[k];
  for (int64_t k = threadIdx.x; k < S.num_quads * 5; k += fill) l_quads[k] = S.quads[k];
  for (int64_t k = threadIdx.x; k < S.num_tris * 3; k += fill) l_edges[k] = Q.edges[k];
  if (S.ref_mode == 0)
    for (int64_t k = threadIdx.x; k < S.num_refs; k += fill) l_refs[k] = S.refs[k];
  L.spheres = l_spheres;
  L.sphere_f4 = 3;
  L.quads = l_quads;
  L.refs = l_refs;
  L.nodes = l_nodes;
  L.root_code = rebase;
  L.node_limit = rebase + static_cast<int32_t>(S.num_nodes) * 112;
  N.edges = l_edges;
}

__device__ __forceinline__ void flush_nearest(const DevNearest& Q, NearWave& w) {
  const uint32_t points = nwave_sum(w.points), found = nwave_sum(w.found);
  const bool of = nballot(w.overflow) != 0, cr = nballot(w.corrupt) != 0;
  if (__lane_id() == 0) {
    atomicAdd(&Q.counters[0], static_cast<unsigned long long>(points));
    atomicAdd(&Q.counters[3], static_cast<unsigned long long>(found));
    if (of) atomicAdd(&Q.counters[4], 1ull);
    if (cr) atomicAdd(&Q.counters[5], 1ull);
  }
}

}  // namespace
}  // namespace rtg
