// rtg_raysort.hpp — the coherence key of RTG_QUERY_SORT (rtg_intersect), shared by the device sort
// (rtg_raysort.hip), the pre-pass of device batches (rtg_query.hip) and the host twin (rtg_api.cpp
// rtg_ray_sort_keys_host), so the three compute one key from one text (DESIGN.md §3 "Ray sorting").
//
// A ray is a point in six dimensions: its origin and its direction scaled to unit L1 norm (every component in
// [-1, 1], no square root). The batch's box in those six axes is found first; the host splits kSortKeyBits
// among the axes by the box's extents (sort_layout) and a ray's key interleaves its per-axis cell numbers,
// origin bits above direction bits. Every operation is a single fp32 operation in a fixed order (the
// translation units are built with -ffp-contract=off; the divide is the compiler's correctly rounded `/`, not
// div_rn, which is exact only away from the ends of the fp32 range: a direction component may be anything).
#ifndef RTG_RAYSORT_HPP
#define RTG_RAYSORT_HPP
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rtgpu.h"

namespace rtg {

// tunable (DESIGN.md §8 "Ray sorting": 13 was tried, 0-5 % slower end to end): 2^12 four-byte counters are 16 KiB
// of a workgroup's LDS
constexpr int kSortKeyBits = 12;
constexpr int kSortBuckets = 1 << kSortKeyBits;
constexpr uint32_t kSortInvalidKey = kSortBuckets - 1;  // rays the query does not trace: the end of the order
constexpr int kSortAxes = 6;
// the sort kernels' shape: a workgroup of kSortThreads lanes owns one chunk of the batch and walks it in steps
// of kSortThreads * kSortRaysPerLane rays; chunks hold at least RTG_QUERY_SORT_CHUNK rays (so that flushing
// kSortBuckets counters is amortised) and there are at most kSortWgsPerCu chunks per CU
constexpr int kSortThreads = 512;
constexpr int kSortRaysPerLane = 4;
constexpr int kSortWgsPerCu = 2;
constexpr int kSortScanTile = 4096;  // matrix entries per workgroup of the scan kernels (1024 lanes x 4)
static_assert(RTG_QUERY_SORT_CHUNK % (kSortThreads * kSortRaysPerLane) == 0, "a chunk is whole steps");
static_assert(kSortBuckets % kSortScanTile == 0, "a matrix of whole bucket rows is whole scan tiles");

// What a key is computed from, by value in the kernel arguments: per axis the box's lower end, cells / extent,
// cells - 1 (as a float: the clamp comes before the conversion), the axis' bit count and the key bit that each
// of its cell bits lands on.
struct SortLayout {
  float lo[kSortAxes], scale[kSortAxes], top[kSortAxes];
  uint8_t bits[kSortAxes];
  uint8_t pos[kSortAxes][16];
};

// The six coordinates of a ray, and whether it belongs to the box: origin within the query's reach (1e30, as
// rtg_query.hip kQueryOriginLimit), direction finite and not zero. (NaN fails every comparison.)
__host__ __device__ inline bool sort_point(float ox, float oy, float oz, float dx, float dy, float dz, float p[kSortAxes]) {
  const float lim = 1e30f, inf = __builtin_inff();
  const float l1 = (__builtin_fabsf(dx) + __builtin_fabsf(dy)) + __builtin_fabsf(dz);
  const bool ok = __builtin_fabsf(ox) < lim && __builtin_fabsf(oy) < lim && __builtin_fabsf(oz) < lim && l1 > 0.0f && l1 < inf;
  p[0] = ox;
  p[1] = oy;
  p[2] = oz;
  p[3] = dx / l1;
  p[4] = dy / l1;
  p[5] = dz / l1;
  return ok;
}

// cell = min(int((x - lo) * scale), cells - 1) per axis, its bits dealt to their key positions
__host__ __device__ inline uint32_t sort_key(const SortLayout& L, const float p[kSortAxes]) {
  uint32_t key = 0;
#pragma unroll
  for (int a = 0; a < kSortAxes; ++a) {
    float v = (p[a] - L.lo[a]) * L.scale[a];
    v = __builtin_fminf(__builtin_fmaxf(v, 0.0f), L.top[a]);
    const uint32_t cell = static_cast<uint32_t>(static_cast<int32_t>(v));
    const int nb = L.bits[a];  // uniform over the launch
    for (int j = 0; j < nb; ++j) key |= ((cell >> j) & 1u) << L.pos[a][j];
  }
  return key;
}

// Box words on the device: a float's bits mapped so that unsigned order is float order; the lower ends are kept
// complemented, so all twelve are reduced by atomicMax from 0 (0 itself is the code of no float but a NaN: empty)
__host__ __device__ inline uint32_t sort_box_code(float f) {
  const uint32_t b = __builtin_bit_cast(uint32_t, f);
  return (b >> 31) ? ~b : b | 0x80000000u;
}
inline float sort_box_decode(uint32_t c) {
  const uint32_t b = (c >> 31) ? c & 0x7fffffffu : ~c;
  return __builtin_bit_cast(float, b);
}

// ---- host side (rtg_raysort.hip) ----
// One ray into a host batch's box (*any: the box holds a ray already); rays sort_point rejects leave it alone.
inline void sort_box_add(const rtg_ray& r, bool* any, float lo[kSortAxes], float hi[kSortAxes]) {
  float p[kSortAxes];
  if (!sort_point(r.origin[0], r.origin[1], r.origin[2], r.dir[0], r.dir[1], r.dir[2], p)) return;
  for (int a = 0; a < kSortAxes; ++a) {
    lo[a] = *any && lo[a] < p[a] ? lo[a] : p[a];
    hi[a] = *any && hi[a] > p[a] ? hi[a] : p[a];
  }
  *any = true;
}
// The batch box of a host batch: lo / hi per axis over the rays sort_point accepts; false: none (empty box).
bool sort_box_host(const rtg_ray* rays, int64_t n, float lo[kSortAxes], float hi[kSortAxes]);
// The bit shares and the layout of a box. Each of the kSortKeyBits bits goes to the axis whose cell is widest
// at that moment, origin extents counted relative to `scene_extent` and direction extents relative to 2 (ties to
// the lower axis); an axis of zero extent gets none, an empty box leaves every key 0. Origin bits above direction
// bits, each group interleaved from its most significant bits down.
void sort_layout(const float lo[kSortAxes], const float hi[kSortAxes], bool empty, double scene_extent, SortLayout* L);

// One sorted query's launch shape and its buffers inside one allocation: perm | matrix | tile sums | keys.
struct SortPlan {
  uint32_t chunk = 0, workgroups = 0;
  uint32_t* perm = nullptr;       // [n] ray index at each cursor position
  uint32_t* matrix = nullptr;     // [kSortBuckets][workgroups] counts, then starts
  uint32_t* tile_sums = nullptr;  // one per kSortScanTile entries of the matrix
  uint16_t* keys = nullptr;       // [n]
};
// Fills P for n > 0 rays on a device of num_cus CUs (pointers from `base` when it is not null); returns the bytes.
size_t sort_plan(int64_t n, int num_cus, void* base, SortPlan* P);
hipError_t launch_ray_sort(const SortLayout& L, const void* rays, uint32_t n, const SortPlan& P, hipStream_t stream);

}  // namespace rtg
#endif
