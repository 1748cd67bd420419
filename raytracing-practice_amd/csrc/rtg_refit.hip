// rtg_refit.hip — rtg_scene_update: new primitive records on the device, then every node box of the existing tree
// refitted bottom-up (DESIGN.md §3 "Scene updates"). The topology, leaf references, slots and tie ranks stay.
//
//   1. update_records_kernel  one lane per updated primitive: the record rtg_scene_create would write for the same
//                             values (fp64 from the widened floats, compile_scene's order, rounded once), the
//                             triangle's vertex box, the batch's coordinate reach (for M) and the invalid count
//   2. refit_parents_kernel   one lane per child slot: parent[child] = node * W + slot, arrival counters cleared.
//                             Derived on every update: rtg_scene_prepare may have renumbered the node array
//   3. refit_up_kernel        one lane per child slot, W lanes = one node (a wave refits 16 four-wide or 32 child-pair
//                             nodes). A leaf slot's lane unites its <= 8 primitives' culling boxes (rtg_primbox.hpp)
//                             in registers and stores them into the node's plane rows; the group then arrives at its
//                             node's counter with the number of its leaf slots. The group whose arrival completes a
//                             node loads the node's W child boxes (one per lane), unites them with cross-lane
//                             exchanges, writes the union into the parent's slot and arrives there: the last arriver
//                             walks up, the others leave. Nobody waits, so the pass cannot hang.
// Scopes (per-XCD L2s are not coherent): box words are written and read with agent-scope relaxed atomics (they
// bypass the non-coherent levels), every arrival is an agent-scope acq_rel fetch_add preceded by a release fence
// and followed by an acquire fence executed by all lanes of the group, as bounds_up_kernel (rtg_gpubvh.hip) does.
// Code rows and the parent table are not written by this kernel and are read with plain loads.
#include <cstdint>

#include "rtg_internal.hpp"
#include "rtg_primbox.hpp"
#include "rtg_refit.hpp"

namespace rtg {
namespace {

constexpr float kInfF = __builtin_huge_valf();

// ---- fp64 helpers with the operator semantics of the host compiler (rtg_api.cpp D3; vec3.hpp:100-155) ----
struct D3 {
  double x, y, z;
};
__device__ __forceinline__ D3 widen(float4 v) { return D3{static_cast<double>(v.x), static_cast<double>(v.y), static_cast<double>(v.z)}; }
__device__ __forceinline__ D3 operator+(D3 a, D3 b) { return D3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ D3 operator-(D3 a, D3 b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ D3 operator*(double t, D3 a) { return D3{t * a.x, t * a.y, t * a.z}; }
__device__ __forceinline__ D3 operator/(D3 a, double t) { return (1 / t) * a; }
__device__ __forceinline__ double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ D3 cross(D3 a, D3 b) {
  return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ D3 unit_vector(D3 v) { return v / sqrt(dot(v, v)); }
__device__ __forceinline__ float f32(double x) { return static_cast<float>(x); }
__device__ __forceinline__ float round_down(double x) {
  float f = static_cast<float>(x);
  if (static_cast<double>(f) > x) f = nextafterf(f, -kInfF);
  return f;
}
__device__ __forceinline__ float round_up(double x) {
  float f = static_cast<float>(x);
  if (static_cast<double>(f) < x) f = nextafterf(f, kInfF);
  return f;
}

// aabb(point a, point b) with pad_to_minimums, then united into lo / hi (rtg_bvh.cpp box_from_points, box_union)
__device__ __forceinline__ void add_point_box(D3 a, D3 b, double lo[3], double hi[3]) {
  const double pa[3] = {a.x, a.y, a.z}, pb[3] = {b.x, b.y, b.z};
  for (int k = 0; k < 3; ++k) {
    double l = pa[k] <= pb[k] ? pa[k] : pb[k], h = pa[k] <= pb[k] ? pb[k] : pa[k];
    if (h - l < 0.0001) {
      l -= 0.0001 / 2.0f;
      h += 0.0001 / 2.0f;
    }
    lo[k] = l <= lo[k] ? l : lo[k];
    hi[k] = h >= hi[k] ? h : hi[k];
  }
}

__device__ __forceinline__ bool finite3(float4 v) { return fabsf(v.x) < kInfF && fabsf(v.y) < kInfF && fabsf(v.z) < kInfF; }

__global__ __launch_bounds__(256) void update_records_kernel(UpdateArgs A) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  double reach = 0.0;
  bool invalid = false;
  if (i < A.count) {
    const int64_t idx = A.indices ? static_cast<int64_t>(A.indices[i]) : i;
    const float4 r0 = A.prims[3 * i], r1 = A.prims[3 * i + 1], r2 = A.prims[3 * i + 2];  // {p0, radius}, {p1, -}, {p2, -}
    const int32_t ref = idx >= 0 && idx < A.num_prims ? A.slot_of[idx] : -1;
    const D3 p0 = widen(r0), p1 = widen(r1), p2 = widen(r2);
    double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    invalid = ref < 0 || !finite3(r0) || !finite3(r1);
    if (!invalid && (ref & kTriRefBit)) {
      const int64_t slot = ref & kRefSlotMask;
      const D3 Q = p0, u = p1, v = p2;
      const D3 n = cross(u, v);
      invalid = !finite3(r2) || !(dot(n, n) > 0.0) || slot >= A.num_tris;  // |u x v| == 0: no plane
      add_point_box(Q, Q + u, lo, hi);
      add_point_box(Q, Q + v, lo, hi);
      for (int k = 0; k < 3; ++k) reach = fmax(reach, fmax(fabs(lo[k]), fabs(hi[k])));
      invalid = invalid || !(reach < 1e30);
      if (!invalid) {
        // the plane and the two edge planes of the inside test, as compile_scene forms them
        const D3 normal = unit_vector(n);
        const double D = dot(normal, Q);
        const D3 w = n / dot(n, n);
        const D3 Ae = cross(v, w), Be = cross(w, u);
        float4* t = A.tris + slot * 3;
        t[0] = make_float4(f32(normal.x), f32(normal.y), f32(normal.z), f32(D));
        t[1] = make_float4(f32(Ae.x), f32(Ae.y), f32(Ae.z), f32(-dot(Ae, Q)));
        t[2] = make_float4(f32(Be.x), f32(Be.y), f32(Be.z), f32(-dot(Be, Q)));
        float2* b = reinterpret_cast<float2*>(A.tri_boxes + slot * 6);  // 24-B rows: 8-B aligned
        b[0] = make_float2(round_down(lo[0]), round_down(lo[1]));
        b[1] = make_float2(round_down(lo[2]), round_up(hi[0]));
        b[2] = make_float2(round_up(hi[1]), round_up(hi[2]));
      }
    } else if (!invalid && (ref & kQuadRefBit)) {
      const int64_t slot = ref & ~kQuadRefBit;
      const D3 Q = p0, u = p1, v = p2;
      const D3 qu = Q + u;
      add_point_box(Q, qu + v, lo, hi);
      add_point_box(qu, Q + v, lo, hi);
      for (int k = 0; k < 3; ++k) reach = fmax(reach, fmax(fabs(lo[k]), fabs(hi[k])));
      invalid = !finite3(r2) || !(reach < 1e30) || slot >= A.num_quads;
      if (!invalid) {
        const D3 n = cross(u, v);
        const D3 normal = unit_vector(n);
        const double D = dot(normal, Q);
        const D3 w = n / dot(n, n);
        float4* q = A.quads + slot * 5;
        const float mat = q[1].w, tie = q[2].w;  // the cold words of the rows stay
        q[0] = make_float4(f32(Q.x), f32(Q.y), f32(Q.z), f32(D));
        q[1] = make_float4(f32(u.x), f32(u.y), f32(u.z), mat);
        q[2] = make_float4(f32(v.x), f32(v.y), f32(v.z), tie);
        q[3] = make_float4(f32(w.x), f32(w.y), f32(w.z), 0.0f);
        q[4] = make_float4(f32(normal.x), f32(normal.y), f32(normal.z), 0.0f);
      }
    } else if (!invalid) {
      const int64_t slot = ref;
      const double r = static_cast<double>(r0.w);
      const D3 dir = p1 - p0;
      const D3 rr{r, r, r};
      if (r1.x != r0.x || r1.y != r0.y || r1.z != r0.z) {  // moving: the boxes at time 0 and 1 (sphere.hpp:32-44)
        const D3 at0 = p0 + 0.0 * dir, at1 = p0 + 1.0 * dir;
        add_point_box(at0 - rr, at0 + rr, lo, hi);
        add_point_box(at1 - rr, at1 + rr, lo, hi);
      } else {
        add_point_box(p0 - rr, p0 + rr, lo, hi);
      }
      for (int k = 0; k < 3; ++k) reach = fmax(reach, fmax(fabs(lo[k]), fabs(hi[k])));
      invalid = !(fabsf(r0.w) < kInfF) || !(reach < 1e30) || slot >= A.num_spheres;
      if (!invalid) {
        float4* s = A.spheres + slot * 2;
        const float mat = s[1].w;
        s[0] = make_float4(r0.x, r0.y, r0.z, r0.w);
        s[1] = make_float4(f32(dir.x), f32(dir.y), f32(dir.z), mat);
      }
    }
    if (invalid) reach = 0.0;
  }
  // the wave's reach and invalid count, then one atomic each (non-negative doubles order as their bits)
  unsigned long long bits = static_cast<unsigned long long>(__double_as_longlong(reach));
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = static_cast<unsigned long long>(__shfl_xor(static_cast<long long>(bits), off, 64));
    bits = o > bits ? o : bits;
  }
  const unsigned long long bad = __popcll(__ballot(invalid));
  if ((threadIdx.x & 63) == 0) {
    if (bits != 0) atomicMax(&A.words[0], bits);
    if (bad != 0) atomicAdd(&A.words[1], bad);
  }
}

// word of child box plane j (0..2 lo.xyz, 3..5 hi.xyz) of slot s in a node: W = 4 plane rows of four, W = 2 the
// child-pair layout {lo0, hi0, lo1, hi1, codes}
template <int W>
__device__ __forceinline__ int box_word(int s, int j) {
  return W == 4 ? j * 4 + s : s * 6 + j;
}
template <int W>
constexpr int node_words() {
  return W == 4 ? 28 : 16;
}
template <int W>
constexpr int code_word() {
  return W == 4 ? 24 : 12;
}
// inner child code -> node index, -1: a leaf, an empty slot or a code that names no node
template <int W>
__device__ __forceinline__ int64_t inner_child(int32_t code, int64_t num_nodes) {
  if (code < 0) return -1;
  if (W == 4 && code % 112 != 0) return -1;
  const int64_t c = W == 4 ? code / 112 : code;
  return c > 0 && c < num_nodes ? c : -1;
}

template <int W>
__global__ __launch_bounds__(256) void refit_parents_kernel(const int32_t* __restrict__ nodes, int64_t num_nodes,
                                                            int32_t* __restrict__ parent, uint32_t* __restrict__ arrived) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int64_t node = t / W;
  const int slot = static_cast<int>(t - node * W);
  if (node >= num_nodes) return;
  if (slot == 0) {
    arrived[node] = 0u;
    if (node == 0) parent[0] = -1;
  }
  const int64_t c = inner_child<W>(nodes[node * node_words<W>() + code_word<W>() + slot], num_nodes);
  if (c > 0) parent[c] = static_cast<int32_t>(node * W + slot);
}

template <int W>
__global__ __launch_bounds__(256) void refit_up_kernel(RefitArgs A) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  int64_t node = t / W;
  const int slot = static_cast<int>(t - node * W);
  if (node >= A.num_nodes) return;  // whole groups: num_nodes * W lanes are W-aligned
  uint32_t* words = reinterpret_cast<uint32_t*>(A.nodes);
  const int32_t* codes = reinterpret_cast<const int32_t*>(A.nodes) + node * node_words<W>() + code_word<W>();
  int nchild = 0, arrive = 0;  // the node's children, and the leaf slots among them: this group's arrival
  for (int k = 0; k < W; ++k) {
    const int32_t c = codes[k];
    nchild += c != kEmptyChild;
    arrive += c < 0 && c != kEmptyChild;
  }
  const int32_t code = codes[slot];
  if (code < 0 && code != kEmptyChild) {  // a leaf slot: the union of its primitives' culling boxes
    const int64_t first = static_cast<int64_t>(~code) >> 3;
    const int count = (~code & 7) + 1;
    Box6 b;
    for (int k = 0; k < 3; ++k) b.lo[k] = kInfF, b.hi[k] = -kInfF;
    for (int64_t r = first; r < first + count && r < A.num_refs; ++r) {
      const int32_t ref = A.refs[r];
      const int64_t ps = ref & kRefSlotMask;
      const bool known = ref >= 0 && ((ref & kTriRefBit) ? !(ref & kQuadRefBit) && ps < A.num_tris
                                      : (ref & kQuadRefBit) ? ps < A.num_quads : ps < A.num_spheres);
      if (!known) continue;  // a reference no record answers: nothing to bound
      int flat;
      Box6 p = prim_box(A.spheres, A.quads, A.tri_boxes, ref, &flat);
      pad_prim_box(&p, A.quads, ref, flat, A.pads);
      for (int k = 0; k < 3; ++k) b.lo[k] = fminf(b.lo[k], p.lo[k]), b.hi[k] = fmaxf(b.hi[k], p.hi[k]);
    }
    uint32_t* w = words + node * node_words<W>();
    for (int k = 0; k < 3; ++k) {
      __hip_atomic_store(w + box_word<W>(slot, k), __float_as_uint(b.lo[k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(w + box_word<W>(slot, 3 + k), __float_as_uint(b.hi[k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  const int leader = static_cast<int>(threadIdx.x & 63) & ~(W - 1);
  while (arrive > 0) {  // every condition below is the same for the W lanes of a group
    // release this group's box stores, acquire the other children's: the arrival that completes the node goes on
    __atomic_thread_fence(__ATOMIC_RELEASE);
    uint32_t old = 0;
    if (slot == 0)
      old = __hip_atomic_fetch_add(&A.arrived[node], static_cast<uint32_t>(arrive), __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    old = static_cast<uint32_t>(__shfl(static_cast<int>(old), leader, 64));
    if (static_cast<int>(old) + arrive != nchild) break;
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    const int32_t p = A.parent[node];
    if (p < 0) break;  // the root: its own box is nobody's child box
    // the node's union: one child box per lane (an empty slot's inverted box is neutral), cross-lane min / max
    const uint32_t* w = words + node * node_words<W>();
    float u[6];
    for (int k = 0; k < 6; ++k)
      u[k] = __uint_as_float(__hip_atomic_load(w + box_word<W>(slot, k), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    for (int off = 1; off < W; off <<= 1)
      for (int k = 0; k < 3; ++k) {
        u[k] = fminf(u[k], __shfl_xor(u[k], off, 64));
        u[3 + k] = fmaxf(u[3 + k], __shfl_xor(u[3 + k], off, 64));
      }
    const int64_t pnode = p / W;
    const int pslot = p % W;
    if (pnode >= A.num_nodes) break;
    uint32_t* pw = words + pnode * node_words<W>();
    // W = 4: lanes 0..2 of the group write the lo and hi plane of one axis each; W = 2: three planes each
    for (int k = slot; k < 3; k += W) {
      __hip_atomic_store(pw + box_word<W>(pslot, k), __float_as_uint(u[k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(pw + box_word<W>(pslot, 3 + k), __float_as_uint(u[3 + k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    node = pnode;
    arrive = 1;
    nchild = 0;
    const int32_t* pc = reinterpret_cast<const int32_t*>(pw) + code_word<W>();
    for (int k = 0; k < W; ++k) nchild += pc[k] != kEmptyChild;
  }
}

unsigned blocks_for(int64_t n) { return static_cast<unsigned>((n + 255) / 256); }

}  // namespace

hipError_t launch_update_records(const UpdateArgs& A, hipStream_t st) {
  if (A.count <= 0) return hipSuccess;
  hipLaunchKernelGGL(update_records_kernel, dim3(blocks_for(A.count)), dim3(256), 0, st, A);
  return hipGetLastError();
}

hipError_t launch_refit(const RefitArgs& A, int width, hipStream_t st) {
  if (A.num_nodes <= 0) return hipSuccess;
  const int32_t* codes = reinterpret_cast<const int32_t*>(A.nodes);
  if (width == 4) {
    hipLaunchKernelGGL(refit_parents_kernel<4>, dim3(blocks_for(A.num_nodes * 4)), dim3(256), 0, st, codes, A.num_nodes,
                       A.parent, A.arrived);
    hipLaunchKernelGGL(refit_up_kernel<4>, dim3(blocks_for(A.num_nodes * 4)), dim3(256), 0, st, A);
  } else if (width == 2) {
    hipLaunchKernelGGL(refit_parents_kernel<2>, dim3(blocks_for(A.num_nodes * 2)), dim3(256), 0, st, codes, A.num_nodes,
                       A.parent, A.arrived);
    hipLaunchKernelGGL(refit_up_kernel<2>, dim3(blocks_for(A.num_nodes * 2)), dim3(256), 0, st, A);
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace rtg
