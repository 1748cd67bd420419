// rtg_nearest_k.hip — gfx950 kernels of rtg_closest_points: for each of N points the k nearest primitives' surfaces,
// sorted (DESIGN.md §3 "k nearest", §4 "Proximity semantics").
//
// The tree, the records, the hand-out, the node steps, the (code, d^2) stacks and the distance tests are
// rtg_closest_point's (rtg_nearest.hpp). What differs is what a lane keeps and prunes against:
//   - a candidate list of k entries (d^2, leaf reference) per lane in LDS, entry j of lane l at word [j][l] (the
//     d^2 rows, then the reference rows), lane-contiguous as the stacks are: every access is conflict-free, a lane
//     touches its own column only, and nothing is synchronised. k x 64 x 8 B per wave of dynamic LDS, sized by
//     the launch's k;
//   - the list is kept sorted by (d^2, input index); an insertion shifts from the tail. In registers a lane keeps
//     its count and the walk's bound: the radius bound until the list is full, the tail's d^2 from then on. A
//     candidate past the bound never touches LDS;
//   - a finished lane writes its entries in order, each record formed by nearest_record as rtg_closest_point forms
//     its winner's, then miss records up to k, then its count.
// The bound starts loose and tightens only once k candidates are in, so the walk visits more of the tree than the
// one-winner walk does; pruning stays conservative by the same prune_bound, so the list is a function of the
// point, the time, the records and the input indices alone.
#include "rtg_nearest.hpp"

namespace rtg {
namespace {

// A lane's column of its wave's candidate lists
struct NearList {
  int32_t* w;  // entry j: d^2 bits at w[j * 64], leaf reference at w[(k + j) * 64]
  int32_t k;
  __device__ __forceinline__ float d2(int32_t j) const { return __int_as_float(w[j * 64]); }
  __device__ __forceinline__ int32_t ref(int32_t j) const { return w[(k + j) * 64]; }
  __device__ __forceinline__ void set(int32_t j, float d2, int32_t ref) const {
    w[j * 64] = __float_as_int(d2);
    w[(k + j) * 64] = ref;
  }
};

// A candidate into the lane's sorted list: entries that sort after it move one place toward the tail (the tail
// of a full list drops out), the candidate takes the gap. At bit-equal d^2 the lower input index sorts first; the
// indices are read only in the wave-uniform branch taken when some lane ties. t.best2 is the bound: unchanged
// until the list is full, then the tail's d^2.
__device__ __forceinline__ void near_insert(Near& t, int32_t& count, const NearList& L, const DevScene& S,
                                            const DevNearest& Q, int32_t ref, float d2) {
  if (!(d2 <= t.best2)) return;
  int32_t j = count;
  while (j > 0) {
    const float e2 = L.d2(j - 1);
    bool after = e2 > d2;
    const bool tie = e2 == d2;
    if (nballot(tie) != 0 && tie) after = Q.prim_index[ref_entry(S, L.ref(j - 1))] > Q.prim_index[ref_entry(S, ref)];
    if (!after) break;
    if (j < L.k) L.set(j, e2, L.ref(j - 1));
    --j;
  }
  if (j >= L.k) return;  // a full list whose tail ties and has the lower index
  L.set(j, d2, ref);
  count = min(count + 1, L.k);
  if (count == L.k) t.best2 = L.d2(L.k - 1);
}

// One primitive of the leaf at t.todo; the lane stays at the rest of the leaf for its next leaf trip, or pops.
template <class Stk>
__device__ __forceinline__ void near_leaf_k(Near& t, int32_t& count, const NearList& L, const DevScene& S,
                                            const DevNearest& Q, const Stk& sc, const Stk& sb, NearWave& w) {
  const int32_t code = ~t.todo;
  const int32_t first = code >> 3;
  const int32_t left = (code & 7) + 1;
  if (static_cast<int64_t>(first) + left > S.num_refs) {
    w.corrupt = true;
    t.todo = kTravDone;
    return;
  }
  const int32_t kind = S.ref_mode == 2 ? kQuadRefBit : (S.ref_mode == 3 ? kTriRefBit : 0);
  const int32_t ref = S.ref_mode == 0 ? S.refs[first] : (first | kind);
  near_insert(t, count, L, S, Q, ref, prim_d2(S, Q.edges, ref, t.p, t.time));
  if (left > 1)
    t.todo = ~(((first + 1) << 3) | (left - 2));
  else
    near_pop(t, sc, sb);
}

// The k records of a finished lane, each two 16-byte stores: its entries in list order while sqrt(d^2) <= max_dist
// (the square root is monotone, so the entries the rounded-up radius bound let in beyond that sit at the end), miss
// records for the rest, then the count. The lane loops over its own entries: k is wave-uniform, so the loop is.
__device__ __forceinline__ void write_list(const DevScene& S, const DevNearestK& K, const Near& t, int32_t count,
                                           const NearList& L, float max_dist, uint32_t idx, NearWave& w) {
  float4* o = K.q.out + static_cast<uint64_t>(idx) * static_cast<uint64_t>(K.k) * 2;
  int32_t found = 0;
  for (int32_t j = 0; j < K.k; ++j) {
    float4 o0 = make_float4(-1.0f, __int_as_float(-1), 0.0f, 0.0f);
    float4 o1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (j < count) {
      const float dist = sqrtf(L.d2(j));
      if (dist <= max_dist) {
        ++found;
        nearest_record(S, K.q, L.ref(j), t.p, t.time, dist, o0, o1);
      }
    }
    o[2 * j] = o0;
    o[2 * j + 1] = o1;
  }
  if (K.counts != nullptr) K.counts[idx] = found;
  w.found += static_cast<uint32_t>(found);
}

// One wave answers points from the launch's cursor until none are left: nearest_stream's hand-out, refill
// threshold and node-trip / leaf-trip split (rtg_nearest.hip), around the walk with a list.
template <class Stk, int WIDE, int GEOM>
__device__ __forceinline__ void nearest_k_stream(const DevScene& S, const DevNearestK& K, const Stk& sc, const Stk& sb,
                                                 const NearList& L, NearWave& w) {
  const DevNearest& Q = K.q;
  Near t = {};
  t.todo = kTravDone;
  t.best = -1;
  int32_t count = 0;  // entries of the lane's list
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
        count = 0;
        t.sp = 0;
        t.todo = S.num_nodes > 0 ? S.root_code : kTravDone;
        // a non-finite or far-out coordinate, a NaN or negative radius, a non-finite time: k misses, no walk
        const bool ok = fabsf(t.p.x) < kPointLimit && fabsf(t.p.y) < kPointLimit && fabsf(t.p.z) < kPointLimit &&
                        max_dist >= 0.0f && fabsf(t.time) < __builtin_inff();
        if (!ok) {
          t.todo = kTravDone;
          max_dist = -1.0f;
        } else if (S.occluder >= 0) {  // the sphere kept out of the tree: an ordinary candidate, tested first
          const float4* sp4 = S.spheres + static_cast<int64_t>(S.occluder) * S.sphere_f4;
          const float d = sphere_dist(sp4[0], sp4[1], t.p, t.time);
          near_insert(t, count, L, S, Q, S.occluder, d * d);
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
      if (leaf_trip && t.todo < 0) near_leaf_k(t, count, L, S, Q, sc, sb, w);
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
      write_list(S, K, t, count, L, max_dist, idx, w);
      idx = kNoPoint;
    }
  }
}

// Four waves per SIMD (<= 128 registers): with 8 KiB of stacks and up to 8 KiB of lists per wave a CU's 160 KiB
// hold at most 17 waves at k = 2 and 10 at k = 16, so the LDS, not the registers, bounds this family's occupancy
constexpr int kNearestKWavesPerSimd = 4;

// Schedule 3: persistent workgroups (the host picks 4, 8 or 16 waves and how many share a CU) with the whole
// scene in LDS as nearest_kernel_lds holds it, the stacks and the lists. 4-wide trees.
template <bool SPILL>
__global__ __launch_bounds__(1024, kNearestKWavesPerSimd) void nearest_k_kernel_lds(DevScene S, DevNearestK K) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const DevNearest& Q = K.q;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int slot = blockIdx.x * (static_cast<int>(blockDim.x) >> 6) + wave;
  // per wave: lds_stack code rows, then lds_stack bound rows; k d^2 rows, then k reference rows
  int32_t* lstk = reinterpret_cast<int32_t*>(smem + Q.lds_stacks) + wave * 2 * Q.lds_stack * 64 + lane;
  const NearList L{reinterpret_cast<int32_t*>(smem + K.lds_lists) + wave * 2 * K.k * 64 + lane, K.k};
  DevScene LS = S;
  DevNearestK N = K;
  nearest_scene_to_lds(S, Q, smem, LS, N.q);
  __syncthreads();
  NearWave w;
  if constexpr (SPILL) {
    int32_t* g = Q.spill + static_cast<int64_t>(slot) * 2 * Q.spill_depth * 64 + lane;
    const SpillStack<kLdsStack> sc{lstk, g, Q.lds_stack, Q.lds_stack + Q.spill_depth};
    const SpillStack<kLdsStack> sb{lstk + Q.lds_stack * 64, g + Q.spill_depth * 64, Q.lds_stack, Q.lds_stack + Q.spill_depth};
    nearest_k_stream<SpillStack<kLdsStack>, 4, kGeomLds>(LS, N, sc, sb, L, w);
  } else {
    nearest_k_stream<LdsStack<kLdsStack>, 4, kGeomLds>(LS, N, LdsStack<kLdsStack>{lstk},
                                                       LdsStack<kLdsStack>{lstk + kLdsStack * 64}, L, w);
  }
  flush_nearest(Q, w);
}

// Schedule 4: 256-thread workgroups, the scene through the caches; 4-wide and child-pair trees. Dynamic LDS: the
// four waves' stacks (16 entries per lane and stack; deeper ones in the spill area), then their lists.
template <int WIDE>
__global__ __launch_bounds__(256, kNearestKWavesPerSimd) void nearest_k_kernel(DevScene S, DevNearestK K) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const DevNearest& Q = K.q;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int slot = blockIdx.x * 4 + wave;
  int32_t* lstk = reinterpret_cast<int32_t*>(smem) + wave * 2 * kLdsStack * 64 + lane;
  const NearList L{reinterpret_cast<int32_t*>(smem + K.lds_lists) + wave * 2 * K.k * 64 + lane, K.k};
  int32_t* g = Q.spill + static_cast<int64_t>(slot) * 2 * Q.spill_depth * 64 + lane;
  const SpillStack<kLdsStack> sc{lstk, g, Q.lds_stack, Q.lds_stack + Q.spill_depth};
  const SpillStack<kLdsStack> sb{lstk + kLdsStack * 64, g + Q.spill_depth * 64, Q.lds_stack, Q.lds_stack + Q.spill_depth};
  NearWave w;
  nearest_k_stream<SpillStack<kLdsStack>, WIDE, kGeomGlobal>(S, K, sc, sb, L, w);
  flush_nearest(Q, w);
}

}  // namespace

// The family, as choose_nearest_kernel's: variant 3 the scene in LDS (4-wide trees), 4 the plain grid. Every
// kernel takes its LDS as dynamic shared memory.
KernelChoice choose_nearest_k_kernel(const DevScene& S, int variant, bool spill) {
  KernelChoice k;
  k.dynamic_lds = true;
  if (variant == 3 && S.node_width == 4) {
    k.fn = spill ? reinterpret_cast<const void*>(&nearest_k_kernel_lds<true>)
                 : reinterpret_cast<const void*>(&nearest_k_kernel_lds<false>);
  } else if (variant == 4) {
    k.fn = S.node_width == 4 ? reinterpret_cast<const void*>(&nearest_k_kernel<4>)
                             : reinterpret_cast<const void*>(&nearest_k_kernel<2>);
    k.block = 256;
  }
  return k;
}

// Dynamic LDS of schedule 3 with the lists, or -1 past 160 KiB. A list entry is the size of a stack entry pair
// (64 lanes x 8 B per row), so this is nearest_lds_layout with k more rows per wave; the lists follow the stacks.
int nearest_k_lds_layout(const DevScene& S, int waves, int entries, int k, DevNearestK* K) {
  const int bytes = nearest_lds_layout(S, waves, entries + k, K ? &K->q : nullptr);
  if (bytes >= 0 && K) K->lds_lists = K->q.lds_stacks + waves * entries * 64 * 8;
  return bytes;
}

// Dynamic LDS of schedule 4: four waves' stacks, then their lists
int nearest_k_grid_lds(int k, DevNearestK* K) {
  const int stacks = 4 * 2 * kLdsStack * 64 * 4;
  if (K) K->lds_lists = stacks;
  return stacks + 4 * k * 64 * 8;
}

hipError_t launch_nearest_k(const KernelChoice& k, const DevScene& S, const DevNearestK& K, int lds_bytes,
                            int grid_blocks, hipStream_t stream) {
  if (!k.fn || K.k < 1 || K.k > 16) return hipErrorInvalidValue;
  const hipError_t e = hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  if (e != hipSuccess) return e;
  DevScene s = S;
  DevNearestK q = K;
  void* args[] = {&s, &q};
  return hipLaunchKernel(k.fn, dim3(grid_blocks), dim3(k.block), args, lds_bytes, stream);
}

}  // namespace rtg
