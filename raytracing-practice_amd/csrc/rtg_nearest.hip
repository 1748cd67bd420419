// rtg_nearest.hip — gfx950 kernels of rtg_closest_point: batched nearest-surface queries on the scene's BVH.
//
// For each of N points: the primitive whose surface is nearest, how far it is and where on it (DESIGN.md §3
// "Proximity queries", §4 "Proximity semantics"). The tree, the records and the lane-refill hand-out are the ray
// query's (rtg_query.hip); the walk is its own (its steps and distance tests in rtg_nearest.hpp, shared with the
// k-nearest family of rtg_nearest_k.hip):
//   - the bound is a squared distance. A node step computes every child box's d^2 = sum max(lo - p, 0, p - hi)^2,
//     orders the (d^2, code) pairs in registers (the 5-comparator network of node_step4), descends into the
//     nearest child that passes the bound and pushes the others far-to-near;
//   - a stack entry is (code, d^2) on two parallel stacks of the existing classes (LdsStack / SpillStack), so a
//     pop skips an entry whose bound the best distance has passed since, without touching its node: best-first
//     order with a depth-first memory footprint (16 entries x 64 lanes x 8 B = 8 KiB of LDS per wave);
//   - a leaf trip tests one primitive per lane with the point-to-primitive distance tests, gathered by
//     ballot as the ray query's leaf trips are.
// During the walk a lane keeps its point, the best squared distance and the winner's reference; the record
// (point, u, v, side, dist) is recomputed once for the winner at write-out.
//
// Pruning is conservative: an entry is skipped only when its fp32 lower bound exceeds best^2 (1 + 2^-19) plus a
// denormal guard, and the node boxes are padded outward, so the winner is a function of the point and the
// records alone (lowest input index at bit-equal d^2), never of the tree or the schedule.
#include "rtg_nearest.hpp"

namespace rtg {
namespace {

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

// The record of a finished lane: the winner's record (nearest_record) or the miss record; two 16-byte stores.
__device__ __forceinline__ void write_nearest(const DevScene& S, const DevNearest& Q, const Near& t, float max_dist,
                                              uint32_t idx, NearWave& w) {
  float4 o0 = make_float4(-1.0f, __int_as_float(-1), 0.0f, 0.0f);
  float4 o1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const float dist = sqrtf(t.best2);
  if (t.best >= 0 && dist <= max_dist) {
    ++w.found;
    nearest_record(S, Q, t.best, t.p, t.time, dist, o0, o1);
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
  DevScene L = S;
  DevNearest N = Q;
  nearest_scene_to_lds(S, Q, smem, L, N);
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
