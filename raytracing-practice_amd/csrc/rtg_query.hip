// rtg_query.hip — gfx950 kernels of rtg_intersect: batched ray queries (closest hit / any hit).
//
// Traversal only: rays come from memory, hit records go back to memory; no camera, no materials, no
// textures. The node and leaf steps, the primitive tests and the exact-t tie rule are the render's
// (rtg_trav.hpp), so a closest-hit query with tmin = 0.001 and tmax = inf returns the t and the winner of
// the render segment with the same origin, direction and time.
//
// Work distribution: lane refill (DESIGN.md §3 "ray queries"). A wave owns 64 ray slots. Rays are handed
// out from a launch-wide cursor (DevQuery::counters[6]), from which one lane reserves a block of rays for its
// wave (DevQuery::block, one atomicAdd; the first form, one add per refill for the wave's demand, made the
// cursor the bottleneck: 4096 waves adding to one address). The lanes without a ray are counted by a ballot
// and a lane's rank among them (mbcnt) picks its ray from the block: the pattern of the render's tile hand-out. Query rays share no pixel and no coherence, so a ray's cost says
// nothing about its neighbours': a lane whose walk has ended writes its record and takes the next ray while
// the other lanes keep their stacks, and a single long ray never idles 63 lanes. The write-out and the
// refill run as one pass, once refill_batch / 64 of the wave's live lanes have finished (or none is still
// walking): per pass the wave pays one atomic round trip, two 16-byte loads, the setup of a traversal and
// the divergent finish code, about the cost of a few node trips, whatever the number of lanes it serves.
//
// Data movement: a ray is two 16-byte loads {origin, tmin}, {dir, tmax}; a hit two 16-byte stores
// {t, prim, u, v}, {normal, front_face}. tmin and the closest hit so far (from tmax) live in the lane.
// LDS holds what traversal reads and nothing else: nodes, stacks, primitive records, leaf references.
#include <algorithm>
#include <cstdint>

#include "rtg_raysort.hpp"
#include "rtg_trav.hpp"

namespace rtg {
namespace {

__device__ __forceinline__ uint64_t qballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ uint32_t qwave_sum(uint32_t x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}
__device__ __forceinline__ bool finite3(V3 a) {
  const float inf = __builtin_inff();
  return fabsf(a.x) < inf && fabsf(a.y) < inf && fabsf(a.z) < inf;
}

// origins the culling margin can be widened for (rtg_api.cpp ensure_origin_reach); a ray from farther out is a miss
constexpr float kQueryOriginLimit = 1e30f;
__device__ __forceinline__ bool reach3(V3 a) {
  return fabsf(a.x) < kQueryOriginLimit && fabsf(a.y) < kQueryOriginLimit && fabsf(a.z) < kQueryOriginLimit;
}
constexpr uint32_t kNoRay = 0xffffffffu;  // a lane's ray index when it holds none
// the interval's lower end is at least the smallest normal float: a root at t <= 0 is never a hit (the
// primitive tests return -1 for a miss)
constexpr float kQueryTMinFloor = 0x1p-126f;

struct QueryWave {
  uint32_t rays = 0, hits = 0;
  bool overflow = false, corrupt = false;
};

// The hit record of a finished lane: one re-read of the winning primitive, (u, v), the unit geometric normal
// turned against the ray (set_face_normal), the input index from the slot table, two 16-byte stores.
template <int PRIMS>
__device__ __forceinline__ void write_hit(const DevScene& S, const DevQuery& Q, const Trav& tr, V3 o, V3 d, float time,
                                          uint32_t idx, QueryWave& w) {
  float4 h0 = make_float4(-1.0f, __int_as_float(-1), 0.0f, 0.0f);
  float4 h1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (tr.best >= 0) {
    ++w.hits;
    const int32_t ref = tr.best;
    const float t = tr.tbest;
    const V3 p = madd(t, d, o);
    constexpr bool kTrisOnly = (PRIMS & kPrimsKind) == kPrimsTris;
    V3 outward;
    float u, v;
    int64_t entry;  // of the slot table: sphere slots, then quad slots, then triangle slots
    if (kTrisOnly || (ref & kTriRefBit)) {
      const int32_t slot = ref & kRefSlotMask;
      const float4* T = S.tris + static_cast<int64_t>(slot) * 3;
      u = tri_edge(T[1], p);
      v = tri_edge(T[2], p);
      outward = xyz(T[0]);
      entry = S.num_spheres + S.num_quads + slot;
    } else if (ref & kQuadRefBit) {
      const int32_t slot = ref & ~kQuadRefBit;
      const float4* q = S.quads + static_cast<int64_t>(slot) * 5;
      const V3 hp = sub(p, xyz(q[0]));
      const V3 wv = xyz(q[3]);
      u = dot(wv, cross(hp, xyz(q[2])));
      v = dot(wv, cross(xyz(q[1]), hp));
      outward = xyz(q[4]);
      entry = S.num_spheres + slot;
    } else {
      const float4* s = S.spheres + static_cast<int64_t>(ref) * S.sphere_f4;
      const float4 s0 = s[0], s1 = s[1];
      const V3 C = madd(time, xyz(s1), xyz(s0));
      outward = scl(div_rn(1.0f, s0.w), sub(p, C));
      // get_sphere_uv, in the spec functions the render's shading uses
      const float theta = acos_spec(-outward.y);
      const float phi = atan2_spec(-outward.z, outward.x) + kPi;
      u = div_rn(phi, 2.0f * kPi);
      v = div_rn(theta, kPi);
      entry = ref;
    }
    const bool front = dot(d, outward) < 0.0f;
    const V3 n = front ? outward : neg(outward);
    h0 = make_float4(t, __int_as_float(Q.prim_index[entry]), u, v);
    h1 = make_float4(n.x, n.y, n.z, __int_as_float(front ? 1 : 0));
  }
  float4* h = Q.hits + static_cast<uint64_t>(idx) * 2;
  h[0] = h0;
  h[1] = h1;
}

// One wave answers rays from the launch's cursor until none are left. PERM (RTG_QUERY_SORT): the cursor runs over
// the sorted order, a cursor position's ray index comes from DevQuery::perm; the PERM = false instantiations never
// read that member and are the kernels of the unsorted query as they were before the flag existed.
template <class Stk, int WIDE, int GEOM, int PRIMS, bool ANY, bool PERM>
__device__ __forceinline__ void query_stream(const DevScene& S, const DevQuery& Q, const Stk& stk, QueryWave& w) {
  constexpr int QRY = ANY ? kQueryAny : kQueryClosest;
  Trav tr = {};
  tr.todo = kTravDone;
  V3 o = v3(0.0f, 0.0f, 0.0f), d = o;
  float time = 0.0f, tmin = 0.0f, tfloor = 0.0f;
  uint32_t idx = kNoRay;
  bool exhausted = false;  // wave-uniform: the cursor has passed the last ray
  uint32_t blk_next = 0, blk_end = 0;  // wave-uniform: the rays of the wave's block not yet handed out
  Counts<false> cnt;
  for (;;) {
    // refill: every lane without a ray takes the next one
    uint64_t want = qballot(idx == kNoRay);
    while (want != 0 && !exhausted) {
      if (blk_next == blk_end) {  // the wave's block is handed out: reserve the next one
        unsigned long long base = 0;
        if (__lane_id() == 0) base = atomicAdd(&Q.counters[6], static_cast<unsigned long long>(Q.block));
        const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(base));
        const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(base >> 32));
        const uint64_t first = (static_cast<uint64_t>(hi) << 32) | lo;
        if (first >= Q.num_rays) {
          exhausted = true;
          break;
        }
        blk_next = static_cast<uint32_t>(first);
        blk_end = static_cast<uint32_t>(min(first + static_cast<uint64_t>(Q.block), static_cast<uint64_t>(Q.num_rays)));
      }
      const uint32_t take = min(static_cast<uint32_t>(__popcll(want)), blk_end - blk_next);
      const uint32_t rank = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(want >> 32),
                                                      __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(want), 0u));
      if (idx == kNoRay && rank < take) {
        if constexpr (PERM)
          idx = Q.perm[blk_next + rank];
        else
          idx = blk_next + rank;
        ++w.rays;
        const float4* r = Q.rays + static_cast<uint64_t>(idx) * 2;
        const float4 r0 = r[0], r1 = r[1];
        o = xyz(r0);
        d = xyz(r1);
        time = Q.times != nullptr ? Q.times[idx] : 0.0f;
        tmin = fmaxf(r0.w, kQueryTMinFloor);
        // the node steps' entry floor: kCullTMin for the render's interval, below the ray's own tmin otherwise
        tfloor = fminf(kCullTMin, 0.9f * tmin);
        trav_begin<WIDE>(tr, S, o, d, -1);
        tr.tbest = r1.w;
        // a non-finite component, an origin past kQueryOriginLimit, a NaN bound or dir == 0: a miss, no traversal
        const bool ok = reach3(o) && finite3(d) && fabsf(time) < __builtin_inff() && r0.w == r0.w && r1.w == r1.w &&
                        tr.a > 0.0f && tr.a < __builtin_inff();
        if (!ok) tr.todo = kTravDone;
        if (ok && S.occluder >= 0) {  // the sphere kept out of the BVH (DevScene::occluder)
          const float4* sp4 = S.spheres + static_cast<int64_t>(S.occluder) * S.sphere_f4;
          const float th = sphere_t(sp4[0], sp4[1], o, d, tr.a, tr.inv_a, time, tmin, tr.tbest, false);
          if (th > 0.0f) {
            tr.tbest = th;
            tr.best = S.occluder;
            if (ANY) tr.todo = kTravDone;
          }
        }
      }
      blk_next += take;
      want = qballot(idx == kNoRay);  // lanes the block's end left without a ray: from the next block
    }
    const uint64_t has_m = qballot(idx != kNoRay);
    if (has_m == 0) break;  // only once the cursor is exhausted
    const int need = max(1, (__popcll(has_m) * Q.refill_batch + 63) >> 6);
    for (;;) {
      const int at_leaf = __popcll(qballot(tr.todo < 0));
      const bool inner_left = qballot(at_inner(tr)) != 0;
      const bool leaf_trip = at_leaf >= Q.leaf_batch || !inner_left;
      if (leaf_trip && tr.todo < 0)
        leaf_step<Stk, false, GEOM != kGeomLds, false, WIDE, GEOM, PRIMS, true, QRY>(tr, S, o, d, time, stk, cnt,
                                                                                 w.corrupt, tmin);
      constexpr int kNodeReps = GEOM == kGeomLds ? 1 : 2;  // as the render (render_stream)
#pragma unroll
      for (int rep = 0; rep < kNodeReps; ++rep) {
        if (at_inner(tr)) {
          if constexpr (WIDE == 4)
            node_step4<Stk, false, GEOM, true>(tr, S, stk, cnt, w.overflow, w.corrupt, tfloor);
          else
            node_step<Stk, false>(tr, S, stk, cnt, w.overflow, w.corrupt, tfloor);
        }
      }
      const uint64_t trav = qballot(trav_active(tr));
      if (trav == 0 || static_cast<int>(__popcll(~trav & has_m)) >= need) break;
    }
    if (!trav_active(tr) && idx != kNoRay) {
      write_hit<PRIMS>(S, Q, tr, o, d, time, idx, w);
      idx = kNoRay;
    }
  }
}

__device__ __forceinline__ void flush_query(const DevQuery& Q, QueryWave& w) {
  const uint32_t rays = qwave_sum(w.rays), hits = qwave_sum(w.hits);
  const bool of = qballot(w.overflow) != 0, cr = qballot(w.corrupt) != 0;
  if (__lane_id() == 0) {
    atomicAdd(&Q.counters[0], static_cast<unsigned long long>(rays));
    atomicAdd(&Q.counters[3], static_cast<unsigned long long>(hits));
    if (of) atomicAdd(&Q.counters[4], 1ull);
    if (cr) atomicAdd(&Q.counters[5], 1ull);
  }
}

template <class Stk, int GEOM, int PRIMS, bool ANY, bool PERM>
__device__ __forceinline__ void query_run(const DevScene& S, const DevQuery& Q, const Stk& stk) {
  QueryWave w;
  query_stream<Stk, 4, GEOM, PRIMS, ANY, PERM>(S, Q, stk, w);
  flush_query(Q, w);
}

// Schedules 3 and 5: persistent workgroups (the host picks 4, 8 or 16 waves and how many share a CU) with the
// whole scene (kGeomLds) or the first nodes of the tree (kGeomTreelet) in LDS, 4-wide trees. A traversal-only
// lane carries no path state: the triangle-only LDS kernels and the child-pair grid kernels fit 64 registers (8
// waves per SIMD) without scratch; the others are compiled for 6 (<= 80 registers; at 8 they spilled 16-92 B per
// lane). The host packs a CU by the compiled register count (rtg_api.cpp rtg_intersect).
constexpr int query_waves_per_simd(bool small) { return small ? 8 : 6; }
template <bool SPILL, int PRIMS, bool ANY, int GEOM, bool PERM>
__global__ __launch_bounds__(1024, query_waves_per_simd((PRIMS & kPrimsKind) == kPrimsTris && GEOM == kGeomLds))
void query_kernel_lds(DevScene S, DevQuery Q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int fill = static_cast<int>(blockDim.x);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int slot = blockIdx.x * (fill >> 6) + wave;
  int32_t* lstk = reinterpret_cast<int32_t*>(smem + Q.lds_stacks) + wave * Q.lds_stack * 64 + lane;
  const uint32_t lds_base =
      static_cast<uint32_t>(reinterpret_cast<uintptr_t>((__attribute__((address_space(3))) unsigned char*)smem));
  DevScene L = S;
  if constexpr (GEOM == kGeomTreelet) {
    float4* l_top = reinterpret_cast<float4*>(smem + Q.lds_nodes);
    for (int k = threadIdx.x; k < S.treelet_bytes / 16; k += fill) l_top[k] = S.nodes[k];
    L.treelet_lds = lds_base + static_cast<uint32_t>(Q.lds_nodes);
  } else {
    float4* l_nodes = reinterpret_cast<float4*>(smem + Q.lds_nodes);
    const int32_t rebase = static_cast<int32_t>(lds_base) + Q.lds_nodes;
    for (int64_t k = threadIdx.x; k < S.num_nodes * 7; k += fill) {
      float4 v = S.nodes[k];
      if (k % 7 == 6) {  // code row: inner-node codes become absolute LDS addresses
        int4 c = *reinterpret_cast<int4*>(&v);
        c.x = c.x >= 0 ? c.x + rebase : c.x;
        c.y = c.y >= 0 ? c.y + rebase : c.y;
        c.z = c.z >= 0 ? c.z + rebase : c.z;
        c.w = c.w >= 0 ? c.w + rebase : c.w;
        v = *reinterpret_cast<float4*>(&c);
      }
      l_nodes[k] = v;
    }
    float4* l_tris = reinterpret_cast<float4*>(smem + Q.lds_tris);
    for (int64_t k = threadIdx.x; k < S.num_tris * 3; k += fill) l_tris[k] = S.tris[k];
    if (Q.lds_tri_meta >= 0) {
      int2* l_meta = reinterpret_cast<int2*>(smem + Q.lds_tri_meta);
      for (int64_t k = threadIdx.x; k < S.num_tris; k += fill) l_meta[k] = S.tri_meta[k];
      L.tri_meta = l_meta;
    }
    L.tris = l_tris;
    if constexpr ((PRIMS & kPrimsKind) != kPrimsTris) {
      // sphere records at a 48-byte stride (an odd number of 16-byte bank slots), as the render's LDS copy
      float4* l_spheres = reinterpret_cast<float4*>(smem + Q.lds_spheres);
      float4* l_quads = reinterpret_cast<float4*>(smem + Q.lds_quads);
      int32_t* l_refs = reinterpret_cast<int32_t*>(smem + Q.lds_refs);
      for (int64_t k = threadIdx.x; k < S.num_spheres * 2; k += fill) l_spheres[(k >> 1) * 3 + (k & 1)] = S.spheres[k];
      for (int64_t k = threadIdx.x; k < S.num_quads * 5; k += fill) l_quads[k] = S.quads[k];
      if (S.ref_mode == 0)
        for (int64_t k = threadIdx.x; k < S.num_refs; k += fill) l_refs[k] = S.refs[k];
      L.spheres = l_spheres;
      L.sphere_f4 = 3;
      L.quads = l_quads;
      L.refs = l_refs;
    }
    L.nodes = l_nodes;
    L.root_code = rebase;
    L.node_limit = rebase + static_cast<int32_t>(S.num_nodes) * 112;
  }
  __syncthreads();
  if constexpr (SPILL) {
    const SpillStack<kLdsStack> stk{lstk, Q.spill + static_cast<int64_t>(slot) * Q.spill_depth * 64 + lane, Q.lds_stack,
                                    Q.lds_stack + Q.spill_depth};
    query_run<SpillStack<kLdsStack>, GEOM, PRIMS, ANY, PERM>(L, Q, stk);
  } else {
    query_run<LdsStack<kLdsStack>, GEOM, PRIMS, ANY, PERM>(L, Q, LdsStack<kLdsStack>{lstk});
  }
}

// Schedule 4: 256-thread workgroups, the scene through the caches; 4-wide trees and the child-pair MEDIAN tree
// (trav_begin<2>'s clamped reciprocals). One stack form: up to 16 entries per lane in LDS, deeper ones in the
// spill area (empty where the tree needs none).
template <int WIDE, bool ANY, bool PERM>
__global__ __launch_bounds__(256, query_waves_per_simd(WIDE == 2)) void query_kernel(DevScene S, DevQuery Q) {
  __shared__ int32_t s_stack[4 * kLdsStack * 64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int slot = blockIdx.x * 4 + wave;
  const SpillStack<kLdsStack> stk{s_stack + wave * kLdsStack * 64 + lane,
                                  Q.spill + static_cast<int64_t>(slot) * Q.spill_depth * 64 + lane, Q.lds_stack,
                                  Q.lds_stack + Q.spill_depth};
  QueryWave w;
  query_stream<SpillStack<kLdsStack>, WIDE, kGeomGlobal, kPrimsAny | kPrimsTriMix, ANY, PERM>(S, Q, stk, w);
  flush_query(Q, w);
}

// The largest |origin coordinate| among the rays of a device-resident batch that can hit (reach3), as float bits (ordered
// like the floats, being non-negative): rtg_intersect widens the culling margin for it before the query runs.
// BOX (RTG_QUERY_SORT): the same pass also finds the batch's six-axis box (rtg_raysort.hpp sort_point), twelve
// words after the reach's 64-bit word, coded so that every one is reduced by atomicMax from 0 (sort_box_code; the
// lower ends complemented): per wave by shuffles, per workgroup through LDS, one atomic per word and workgroup.
template <bool BOX>
__global__ __launch_bounds__(256) void origin_reach_kernel(const float4* __restrict__ rays, uint32_t n,
                                                           unsigned int* __restrict__ out) {
  float m = 0.0f;
  uint32_t box[BOX ? 2 * kSortAxes : 1] = {};
  for (uint64_t k = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x; k < n;
       k += static_cast<uint64_t>(gridDim.x) * blockDim.x) {
    const float4 r = rays[k * 2];
    const float a = fmaxf(fmaxf(fabsf(r.x), fabsf(r.y)), fabsf(r.z));
    if (a < kQueryOriginLimit) m = fmaxf(m, a);
    if constexpr (BOX) {
      const float4 dr = rays[k * 2 + 1];
      float p[kSortAxes];
      if (sort_point(r.x, r.y, r.z, dr.x, dr.y, dr.z, p)) {
#pragma unroll
        for (int x = 0; x < kSortAxes; ++x) {
          const uint32_t c = sort_box_code(p[x]);
          box[x] = max(box[x], ~c);
          box[kSortAxes + x] = max(box[kSortAxes + x], c);
        }
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  if ((threadIdx.x & 63) == 0 && m > 0.0f) atomicMax(out, __float_as_uint(m));
  if constexpr (BOX) {
    __shared__ uint32_t s_box[4][2 * kSortAxes];
#pragma unroll
    for (int x = 0; x < 2 * kSortAxes; ++x) {
      uint32_t v = box[x];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v = max(v, static_cast<uint32_t>(__shfl_xor(static_cast<int>(v), off, 64)));
      if ((threadIdx.x & 63) == 0) s_box[threadIdx.x >> 6][x] = v;
    }
    __syncthreads();
    if (threadIdx.x < 2 * kSortAxes) {
      const uint32_t v = max(max(s_box[0][threadIdx.x], s_box[1][threadIdx.x]), max(s_box[2][threadIdx.x], s_box[3][threadIdx.x]));
      if (v != 0) atomicMax(out + 2 + threadIdx.x, v);
    }
  }
}

template <bool SPILL, int PRIMS, int GEOM>
const void* lds_query_fn(bool any, bool perm) {
  if (perm)
    return any ? reinterpret_cast<const void*>(&query_kernel_lds<SPILL, PRIMS, true, GEOM, true>)
               : reinterpret_cast<const void*>(&query_kernel_lds<SPILL, PRIMS, false, GEOM, true>);
  return any ? reinterpret_cast<const void*>(&query_kernel_lds<SPILL, PRIMS, true, GEOM, false>)
             : reinterpret_cast<const void*>(&query_kernel_lds<SPILL, PRIMS, false, GEOM, false>);
}
template <int WIDE>
const void* grid_query_fn(bool any, bool perm) {
  if (perm)
    return any ? reinterpret_cast<const void*>(&query_kernel<WIDE, true, true>)
               : reinterpret_cast<const void*>(&query_kernel<WIDE, false, true>);
  return any ? reinterpret_cast<const void*>(&query_kernel<WIDE, true, false>)
             : reinterpret_cast<const void*>(&query_kernel<WIDE, false, false>);
}

}  // namespace

// The family (16 kernels, and their 16 twins for RTG_QUERY_SORT: `perm`): {whole scene in LDS, treelet} x {mixed
// class: LdsStack, SpillStack; triangle-only class: LdsStack (whole scene), SpillStack (treelet)} x {closest, any};
// the plain grid for 4-wide and child-pair trees x {closest, any}. variant: 3 LDS scene, 5 treelet, 4 plain grid.
KernelChoice choose_query_kernel(const DevScene& S, int variant, bool any, bool spill, bool perm) {
  constexpr int kMix = kPrimsAny | kPrimsTriMix;
  KernelChoice k;
  // the triangle-only class: records in reference order, no kind bit, and no sphere beside the tree (a mesh on a
  // scene-spanning sphere has a triangle-only tree too, but its winner may be the occluder: the mixed class)
  const bool tris_only = S.ref_mode == 3 && S.occluder < 0;
  if (variant == 3 && S.node_width == 4) {
    k.fn = tris_only && !spill ? lds_query_fn<false, kPrimsTris, kGeomLds>(any, perm)
           : spill             ? lds_query_fn<true, kMix, kGeomLds>(any, perm)
                               : lds_query_fn<false, kMix, kGeomLds>(any, perm);
    k.dynamic_lds = true;
  } else if (variant == 5 && S.node_width == 4) {
    k.fn = tris_only ? lds_query_fn<true, kPrimsTris, kGeomTreelet>(any, perm)
           : spill   ? lds_query_fn<true, kMix, kGeomTreelet>(any, perm)
                     : lds_query_fn<false, kMix, kGeomTreelet>(any, perm);
    k.dynamic_lds = true;
  } else if (variant == 4) {
    k.fn = S.node_width == 4 ? grid_query_fn<4>(any, perm) : grid_query_fn<2>(any, perm);
    k.block = 256;
  }
  return k;
}

// Dynamic LDS of the whole-scene query schedule for workgroups of `waves` waves with `entries` stack entries
// per lane in LDS, or -1 when it exceeds one CU's 160 KiB: nodes, stacks, then the primitive records and leaf
// references; the triangles' cold records last and only where they fit. No materials, textures or noise tables.
int query_lds_layout(const DevScene& S, int waves, int entries, DevQuery* Q) {
  auto a16 = [](int64_t x) { return (x + 15) & ~int64_t(15); };
  if (S.node_width != 4) return -1;
  int64_t off = a16(S.num_nodes * 112);
  const int64_t stacks = off;
  off = a16(off + int64_t(waves) * entries * 64 * 4);
  const int64_t spheres = off;
  off = a16(off + S.num_spheres * 48);
  const int64_t quads = off;
  off = a16(off + S.num_quads * 80);
  const int64_t tris = off;
  off = a16(off + S.num_tris * 48);
  const int64_t refs = off;
  off = a16(off + (S.ref_mode == 0 ? S.num_refs * 4 : 0));
  if (off > 160 * 1024) return -1;
  int64_t tri_meta = -1;
  if (S.num_tris > 0 && off + S.num_tris * 8 <= 160 * 1024) {
    // only where they do not cost a workgroup of the CU (the host packs 160 KiB / bytes workgroups)
    const int64_t with = a16(off + S.num_tris * 8);
    if (160 * 1024 / with == 160 * 1024 / off) {
      tri_meta = off;
      off = with;
    }
  }
  if (Q) {
    Q->lds_nodes = 0;
    Q->lds_stacks = static_cast<int32_t>(stacks);
    Q->lds_spheres = static_cast<int32_t>(spheres);
    Q->lds_quads = static_cast<int32_t>(quads);
    Q->lds_tris = static_cast<int32_t>(tris);
    Q->lds_refs = static_cast<int32_t>(refs);
    Q->lds_tri_meta = static_cast<int32_t>(tri_meta);
  }
  return static_cast<int>(off);
}

// The treelet schedule: the stacks, then as many of the first nodes as fit; sets S->treelet_bytes.
int query_treelet_layout(DevScene* S, int waves, int entries, DevQuery* Q) {
  const int64_t stacks = int64_t(waves) * entries * 64 * 4;
  const int64_t room = 160 * 1024 - stacks;
  if (S->node_width != 4 || room < 112) return -1;
  const int64_t nodes = std::min<int64_t>(S->num_nodes, room / 112);
  S->treelet_bytes = static_cast<int32_t>(nodes * 112);
  Q->lds_stacks = 0;
  Q->lds_nodes = static_cast<int32_t>(stacks);
  Q->lds_tri_meta = -1;
  return static_cast<int>(stacks + nodes * 112);
}

hipError_t launch_query(const KernelChoice& k, const DevScene& S, const DevQuery& Q, int lds_bytes, int grid_blocks,
                        hipStream_t stream) {
  if (!k.fn) return hipErrorInvalidValue;
  if (k.dynamic_lds) {
    const hipError_t e = hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    if (e != hipSuccess) return e;
  }
  DevScene s = S;
  DevQuery q = Q;
  void* args[] = {&s, &q};
  return hipLaunchKernel(k.fn, dim3(grid_blocks), dim3(k.block), args, k.dynamic_lds ? lds_bytes : 0, stream);
}

hipError_t launch_origin_reach(const void* rays, uint32_t n, unsigned int* out, bool box, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const unsigned blocks = static_cast<unsigned>(std::min<uint64_t>((static_cast<uint64_t>(n) + 255) / 256, 1024));
  if (box)
    hipLaunchKernelGGL(origin_reach_kernel<true>, dim3(blocks), dim3(256), 0, stream, static_cast<const float4*>(rays), n, out);
  else
    hipLaunchKernelGGL(origin_reach_kernel<false>, dim3(blocks), dim3(256), 0, stream, static_cast<const float4*>(rays), n, out);
  return hipGetLastError();
}

}  // namespace rtg
