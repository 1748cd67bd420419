// rtg_nearest.hip — gfx950 kernels of rtg_closest_point: batched nearest-surface queries on the scene's BVH.
//
// For each of N points: the primitive whose surface is nearest, how far it is and where on it (DESIGN.md §3
// "Proximity queries", §4 "Proximity semantics"). The tree, the records and the lane-refill hand-out are the ray
// query's (rtg_query.hip); the walk is its own:
//   - the bound is a squared distance. A node step computes every child box's d^2 = sum max(lo - p, 0, p - hi)^2,
//     orders the (d^2, code) pairs in registers (the 5-comparator network of node_step4), descends into the
//     nearest child that passes the bound and pushes the others far-to-near;
//   - a stack entry is (code, d^2) on two parallel stacks of the existing classes (LdsStack / SpillStack), so a
//     pop skips an entry whose bound the best distance has passed since, without touching its node: best-first
//     order with a depth-first memory footprint (16 entries x 64 lanes x 8 B = 8 KiB of LDS per wave);
//   - a leaf trip tests one primitive per lane with the point-to-primitive distance tests below, gathered by
//     ballot as the ray query's leaf trips are.
// During the walk a lane keeps its point, the best squared distance and the winner's reference; the record
// (point, u, v, side, dist) is recomputed once for the winner at write-out.
//
// Pruning is conservative: an entry is skipped only when its fp32 lower bound exceeds best^2 (1 + 2^-19) plus a
// denormal guard, and the node boxes are padded outward, so the winner is a function of the point and the
// records alone (lowest input index at bit-equal d^2), never of the tree or the schedule.
#include <algorithm>
#include <cstdint>

#include "rtg_trav.hpp"

namespace rtg {
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
  float best2;   // squared distance of the nearest primitive so far (starts at the query radius squared)
  int32_t best;  // its leaf reference, -1: none
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

// A candidate against the lane's best. At bit-equal d^2 the lower input index wins; the indices are read only in
// the wave-uniform branch taken when some lane ties (the first candidate of a lane ties with the query radius).
__device__ __forceinline__ void near_take(Near& t, const DevScene& S, const DevNearest& Q, int32_t ref, float d2) {
  bool take = d2 < t.best2;
  const bool tie = d2 == t.best2;
  if (nballot(tie) != 0 && tie)
    take = t.best < 0 || Q.prim_index[ref_entry(S, ref)] < Q.prim_index[ref_entry(S, t.best)];
  if (take) {
    t.best2 = d2;
    t.best = ref;
  }
}

// The next stack entry whose lower bound still passes; entries the best distance has overtaken are dropped
// without a look at their nodes.
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

// One primitive of the leaf at t.todo; the lane stays at the rest of the leaf for its next leaf trip, or pops.
template <class Stk>
__device__ __forceinline__ void near_leaf(Near& t, const DevScene& S, const DevNearest& Q, const Stk& sc, const Stk& sb,
                                          NearWave& w) {
  const int32_t code = ~t.todo;
  const int32_t first = code >> 3;
  const int32_t count = (code & 7) + 1;
  if (static_cast<int64_t>(first) + count > S.num_refs) {
    w.corrupt = true;
    t.todo = kTravDone;
    return;
  }
  const int32_t kind = S.ref_mode == 2 ? kQuadRefBit : (S.ref_mode == 3 ? kTriRefBit : 0);
  const int32_t ref = S.ref_mode == 0 ? S.refs[first] : (first | kind);
  near_take(t, S, Q, ref, prim_d2(S, Q.edges, ref, t.p, t.time));
  if (count > 1)
    t.todo = ~(((first + 1) << 3) | (count - 2));
  else
    near_pop(t, sc, sb);
}

// The record of a finished lane: the winner's test once more for (a, b), then point, side and dist; the input
// index from the slot table; two 16-byte stores.
__device__ __forceinline__ void write_nearest(const DevScene& S, const DevNearest& Q, const Near& t, float max_dist,
                                              uint32_t idx, NearWave& w) {
  float4 o0 = make_float4(-1.0f, __int_as_float(-1), 0.0f, 0.0f);
  float4 o1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const float dist = sqrtf(t.best2);
  if (t.best >= 0 && dist <= max_dist) {
    ++w.found;
    const int32_t ref = t.best;
    const V3 p = t.p;
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
      const V3 C = madd(t.time, xyz(s1), xyz(s0));
      const V3 d = sub(p, C);
      const float len = sqrtf(dot(d, d));
      // p at the centre: the shell point along +x
      const V3 outward = len > 0.0f ? scl(1.0f / len, d) : v3(1.0f, 0.0f, 0.0f);
      pt = madd(fabsf(s0.w), outward, C);
      out = sphere_dist(s0, s1, p, t.time) > 0.0f;
      // get_sphere_uv, in the spec functions write_hit uses
      const float theta = acos_spec(-outward.y);
      const float phi = atan2_spec(-outward.z, outward.x) + kPi;
      u = div_rn(phi, 2.0f * kPi);
      v = div_rn(theta, kPi);
    }
    o0 = make_float4(dist, __int_as_float(Q.prim_index[ref_entry(S, ref)]), u, v);
    o1 = make_float4(pt.x, pt.y, pt.z, __int_as_float(out ? 1 : -1));
  }
  float4* o = Q.out + static_cast<uint64_t>(idx) * 2;
  o[0] = o0;
  o[1] = o1;
}

// One wave answers points from the launch's cursor until none are left: the hand-out, the refill threshold and
// the node-trip / leaf-trip split of query_stream (rtg_query.hip), around the distance walk.
template <class Stk, int WIDE, int GEOM>
__device__ __forceinline__ void nearest_stream(const DevScene& S, const DevNearest& Q, const Stk& sc, const Stk& sb,
                                               NearWave& w) {
  Near t = {};
  t.todo = kTravDone;
  t.best = -1;
  float max_dist = 0.0f;
  uint32_t idx = kNoPoint;
  bool exhausted = false;               // wave-uniform: the cursor has passed the last point
  uint32_t blk_next = 0, blk_end = 0;  // wave-uniform: the points of the wave's block not yet handed out
  for (;;) {
    uint64_t want = nballot(idx == kNoPoint);
    while (want != 0 && !exhausted) {
      if (blk_next == blk_end) {  // the wave's block is handed out: reserve the next one
        unsigned long long base = 0;
        if (__lane_id() == 0) base = atomicAdd(&Q.counters[6], static_cast<unsigned long long>(Q.block));
        const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(base));
        const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(base >> 32));
        const uint64_t first = (static_cast<uint64_t>(hi) << 32) | lo;
        if (first >= Q.num_points) {
          exhausted = true;
          break;
        }
        blk_next = static_cast<uint32_t>(first);
        blk_end = static_cast<uint32_t>(min(first + static_cast<uint64_t>(Q.block), static_cast<uint64_t>(Q.num_points)));
      }
      const uint32_t take = min(static_cast<uint32_t>(__popcll(want)), blk_end - blk_next);
      const uint32_t rank = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(want >> 32),
                                                      __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(want), 0u));
      if (idx == kNoPoint && rank < take) {
        idx = blk_next + rank;
        ++w.points;
        const float4 r = Q.points[idx];
        t.p = xyz(r);
        t.time = Q.times != nullptr ? Q.times[idx] : 0.0f;
        max_dist = r.w;
        // the radius as a squared bound, rounded up: every primitive with sqrt(d^2) <= max_dist passes it
        const float m2 = max_dist * max_dist;
        t.best2 = fmaf(m2, 0x1p-22f, m2);
        t.best = -1;
        t.sp = 0;
        t.todo = S.num_nodes > 0 ? S.root_code : kTravDone;
        // a non-finite or far-out coordinate, a NaN or negative radius, a non-finite time: a miss, no walk
        const bool ok = fabsf(t.p.x) < kPointLimit && fabsf(t.p.y) < kPointLimit && fabsf(t.p.z) < kPointLimit &&
                        max_dist >= 0.0f && fabsf(t.time) < __builtin_inff();
        if (!ok) {
          t.todo = kTravDone;
          max_dist = -1.0f;
        } else if (S.occluder >= 0) {  // the sphere kept out of the tree: first, it seeds the bound
          const float4* sp4 = S.spheres + static_cast<int64_t>(S.occluder) * S.sphere_f4;
          const float d = sphere_dist(sp4[0], sp4[1], t.p, t.time);
          near_take(t, S, Q, S.occluder, d * d);
        }
      }
      blk_next += take;
      want = nballot(idx == kNoPoint);  // lanes the block's end left without a point: from the next block
    }
    const uint64_t has_m = nballot(idx != kNoPoint);
    if (has_m == 0) break;  // only once the cursor is exhausted
    const int need = max(1, (__popcll(has_m) * Q.refill_batch + 63) >> 6);
    for (;;) {
      const int at_leaf = __popcll(nballot(t.todo < 0));
      const bool inner_left = nballot(static_cast<uint32_t>(t.todo) < static_cast<uint32_t>(kTravDone)) != 0;
      const bool leaf_trip = at_leaf >= Q.leaf_batch || !inner_left;
      if (leaf_trip && t.todo < 0) near_leaf(t, S, Q, sc, sb, w);
      constexpr int kNodeReps = GEOM == kGeomLds ? 1 : 2;  // as the ray query
#pragma unroll
      for (int rep = 0; rep < kNodeReps; ++rep) {
        if (static_cast<uint32_t>(t.todo) < static_cast<uint32_t>(kTravDone)) {
          if constexpr (WIDE == 4)
            near_node4<Stk, GEOM>(t, S, sc, sb, w);
          else
            near_node2<Stk>(t, S, sc, sb, w);
        }
      }
      const uint64_t trav = nballot(t.todo != kTravDone);
      if (trav == 0 || static_cast<int>(__popcll(~trav & has_m)) >= need) break;
    }
    if (t.todo == kTravDone && idx != kNoPoint) {
      write_nearest(S, Q, t, max_dist, idx, w);
      idx = kNoPoint;
    }
  }
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

constexpr int kNearestWavesPerSimd = 6;  // the mixed query kernels' budget (<= 80 registers)

// Schedule 3: persistent workgroups (the host picks 4, 8 or 16 waves and how many share a CU) with the whole
// scene in LDS: nodes (inner codes rebased to absolute LDS addresses), the code and bound stacks, sphere, quad
// and triangle edge records, leaf references. 4-wide trees.
template <bool SPILL>
__global__ __launch_bounds__(1024, kNearestWavesPerSimd) void nearest_kernel_lds(DevScene S, DevNearest Q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int fill = static_cast<int>(blockDim.x);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int slot = blockIdx.x * (fill >> 6) + wave;
  // per wave: lds_stack code rows, then lds_stack bound rows
  int32_t* lstk = reinterpret_cast<int32_t*>(smem + Q.lds_stacks) + wave * 2 * Q.lds_stack * 64 + lane;
  const uint32_t lds_base =
      static_cast<uint32_t>(reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) unsigned char*)smem));
  DevScene L = S;
  DevNearest N = Q;
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
  __syncthreads();
  NearWave w;
  if constexpr (SPILL) {
    int32_t* g = Q.spill + static_cast<int64_t>(slot) * 2 * Q.spill_depth * 64 + lane;
    const SpillStack<kLdsStack> sc{lstk, g, Q.lds_stack, Q.lds_stack + Q.spill_depth};
    const SpillStack<kLdsStack> sb{lstk + Q.lds_stack * 64, g + Q.spill_depth * 64, Q.lds_stack, Q.lds_stack + Q.spill_depth};
    nearest_stream<SpillStack<kLdsStack>, 4, kGeomLds>(L, N, sc, sb, w);
  } else {
    nearest_stream<LdsStack<kLdsStack>, 4, kGeomLds>(L, N, LdsStack<kLdsStack>{lstk},
                                                     LdsStack<kLdsStack>{lstk + kLdsStack * 64}, w);
  }
  flush_nearest(Q, w);
}

// Schedule 4: 256-thread workgroups, the scene through the caches; 4-wide and child-pair trees. Up to 16 entries
// per lane and stack in LDS, deeper ones in the spill area (empty where the tree needs none).
// (its 32 KiB of stacks per workgroup hold a SIMD to five waves: the launch bound asks for no more)
template <int WIDE>
__global__ __launch_bounds__(256, kNearestWavesPerSimd - 1) void nearest_kernel(DevScene S, DevNearest Q) {
  __shared__ int32_t s_stack[4 * 2 * kLdsStack * 64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int slot = blockIdx.x * 4 + wave;
  int32_t* lstk = s_stack + wave * 2 * kLdsStack * 64 + lane;
  int32_t* g = Q.spill + static_cast<int64_t>(slot) * 2 * Q.spill_depth * 64 + lane;
  const SpillStack<kLdsStack> sc{lstk, g, Q.lds_stack, Q.lds_stack + Q.spill_depth};
  const SpillStack<kLdsStack> sb{lstk + kLdsStack * 64, g + Q.spill_depth * 64, Q.lds_stack, Q.lds_stack + Q.spill_depth};
  NearWave w;
  nearest_stream<SpillStack<kLdsStack>, WIDE, kGeomGlobal>(S, Q, sc, sb, w);
  flush_nearest(Q, w);
}

// ---- edge records of updated triangles (rtg_scene_update on a RTG_BVH_REFIT | RTG_BVH_NEAREST scene) -------------
// One lane per update, after update_records_kernel (rtg_refit.hip) and with its acceptance rule for a triangle:
// the record rtg_scene_create writes for the same values, the three products in fp64 from the widened floats.
__device__ __forceinline__ bool efinite3(float4 v) {
  const float inf = __builtin_inff();
  return fabsf(v.x) < inf && fabsf(v.y) < inf && fabsf(v.z) < inf;
}
__global__ __launch_bounds__(256) void update_edges_kernel(const int32_t* indices, const float4* prims, int64_t count,
                                                           int64_t num_prims, const int32_t* slot_of, float4* edges,
                                                           int64_t num_tris) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int64_t idx = indices ? static_cast<int64_t>(indices[i]) : i;
  const int32_t ref = idx >= 0 && idx < num_prims ? slot_of[idx] : -1;
  if (ref < 0 || !(ref & kTriRefBit)) return;
  const int64_t slot = ref & kRefSlotMask;
  const float4 r0 = prims[3 * i], r1 = prims[3 * i + 1], r2 = prims[3 * i + 2];
  if (!efinite3(r0) || !efinite3(r1) || !efinite3(r2) || slot >= num_tris) return;
  const double q[3] = {r0.x, r0.y, r0.z}, u[3] = {r1.x, r1.y, r1.z}, v[3] = {r2.x, r2.y, r2.z};
  const double nx = u[1] * v[2] - u[2] * v[1], ny = u[2] * v[0] - u[0] * v[2], nz = u[0] * v[1] - u[1] * v[0];
  if (!(nx * nx + ny * ny + nz * nz > 0.0)) return;  // |u x v| == 0: the update leaves this triangle out
  double reach = 0.0;  // of the vertex box with the reference's minimum extent (update_records_kernel)
  for (int k = 0; k < 3; ++k) {
    const double a = q[k] + u[k], b = q[k] + v[k];
    const double lo = fmin(q[k], fmin(a, b)) - 0.0001, hi = fmax(q[k], fmax(a, b)) + 0.0001;
    reach = fmax(reach, fmax(fabs(lo), fabs(hi)));
  }
  if (!(reach < 1e30)) return;
  const double uu = u[0] * u[0] + u[1] * u[1] + u[2] * u[2];
  const double uv = u[0] * v[0] + u[1] * v[1] + u[2] * v[2];
  const double vv = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
  float4* e = edges + slot * 3;
  e[0] = make_float4(r0.x, r0.y, r0.z, static_cast<float>(uu));
  e[1] = make_float4(r1.x, r1.y, r1.z, static_cast<float>(uv));
  e[2] = make_float4(r2.x, r2.y, r2.z, static_cast<float>(vv));
}

}  // namespace

// The family: scene in LDS for 4-wide trees with LdsStack and with SpillStack; the plain grid for 4-wide and for
// child-pair trees. Every kernel handles all primitive kinds. variant: 3 LDS scene, 4 plain grid.
KernelChoice choose_nearest_kernel(const DevScene& S, int variant, bool spill) {
  KernelChoice k;
  if (variant == 3 && S.node_width == 4) {
    k.fn = spill ? reinterpret_cast<const void*>(&nearest_kernel_lds<true>)
                 : reinterpret_cast<const void*>(&nearest_kernel_lds<false>);
    k.dynamic_lds = true;
  } else if (variant == 4) {
    k.fn = S.node_width == 4 ? reinterpret_cast<const void*>(&nearest_kernel<4>)
                             : reinterpret_cast<const void*>(&nearest_kernel<2>);
    k.block = 256;
  }
  return k;
}

// Dynamic LDS of the whole-scene schedule for workgroups of `waves` waves with `entries` stack entries per lane
// (and stack) in LDS, or -1 when it exceeds one CU's 160 KiB: nodes, the two stacks, sphere, quad and triangle
// edge records, leaf references.
int nearest_lds_layout(const DevScene& S, int waves, int entries, DevNearest* Q) {
  auto a16 = [](int64_t x) { return (x + 15) & ~int64_t(15); };
  if (S.node_width != 4) return -1;
  int64_t off = a16(S.num_nodes * 112);
  const int64_t stacks = off;
  off = a16(off + int64_t(waves) * entries * 64 * 8);
  const int64_t spheres = off;
  off = a16(off + S.num_spheres * 48);
  const int64_t quads = off;
  off = a16(off + S.num_quads * 80);
  const int64_t edges = off;
  off = a16(off + S.num_tris * 48);
  const int64_t refs = off;
  off = a16(off + (S.ref_mode == 0 ? S.num_refs * 4 : 0));
  if (off > 160 * 1024) return -1;
  if (Q) {
    Q->lds_nodes = 0;
    Q->lds_stacks = static_cast<int32_t>(stacks);
    Q->lds_spheres = static_cast<int32_t>(spheres);
    Q->lds_quads = static_cast<int32_t>(quads);
    Q->lds_edges = static_cast<int32_t>(edges);
    Q->lds_refs = static_cast<int32_t>(refs);
  }
  return static_cast<int>(off);
}

hipError_t launch_nearest(const KernelChoice& k, const DevScene& S, const DevNearest& Q, int lds_bytes, int grid_blocks,
                          hipStream_t stream) {
  if (!k.fn) return hipErrorInvalidValue;
  if (k.dynamic_lds) {
    const hipError_t e = hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    if (e != hipSuccess) return e;
  }
  DevScene s = S;
  DevNearest q = Q;
  void* args[] = {&s, &q};
  return hipLaunchKernel(k.fn, dim3(grid_blocks), dim3(k.block), args, k.dynamic_lds ? lds_bytes : 0, stream);
}

hipError_t launch_update_edges(const int32_t* indices, const float4* prims, int64_t count, int64_t num_prims,
                               const int32_t* slot_of, float4* edges, int64_t num_tris, hipStream_t stream) {
  if (count <= 0 || num_tris <= 0) return hipSuccess;
  const unsigned blocks = static_cast<unsigned>((count + 255) / 256);
  hipLaunchKernelGGL(update_edges_kernel, dim3(blocks), dim3(256), 0, stream, indices, prims, count, num_prims, slot_of,
                     edges, num_tris);
  return hipGetLastError();
}

}  // namespace rtg
