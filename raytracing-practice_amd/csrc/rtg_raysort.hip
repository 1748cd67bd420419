// rtg_raysort.hip — gfx950 kernels of RTG_QUERY_SORT: one unstable counting pass that buckets a ray batch by its
// coherence key (rtg_raysort.hpp) and leaves a permutation for the query kernels' cursor (DevQuery::perm).
//
// Traversal needs rays that are neighbours in key space to be neighbours in the cursor, not a total or a stable
// order, so there is one pass over 2^kSortKeyBits buckets and no second one inside a bucket. Work split: the batch
// is cut into contiguous chunks, one workgroup each (at most kSortWgsPerCu per CU, at least RTG_QUERY_SORT_CHUNK
// rays: a workgroup flushes a whole row of bucket counters whatever it counted). Data movement:
//   1. sort_keys_kernel     rays (2 x 16 B, kSortRaysPerLane rays loaded per lane before the first is used) ->
//                           16-bit keys; counts in LDS (ds_add, 16 KiB); the row to matrix[bucket][workgroup]
//   2. sort_scan_*          exclusive scan of the matrix as it lies in memory (bucket-major: a bucket's workgroups
//                           are adjacent), three launches: tile sums, the spine in one workgroup, the tiles again.
//                           Every (bucket, workgroup) pair gets its start; bucket boundaries are deterministic
//   3. sort_scatter_kernel  the workgroup's row of starts into LDS, the chunk's keys again (2 B per ray, not 32);
//                           a lane's position is what ds_add_rtn returns on its bucket's start; perm[position] =
//                           ray index
// No global atomic anywhere; the order inside a bucket is whatever the LDS atomics gave (the answers do not
// depend on it: hits[i] answers rays[i]).
#include <algorithm>

#include "rtg_raysort.hpp"

namespace rtg {
namespace {

constexpr int kScanThreads = kSortScanTile / 4;

__global__ __launch_bounds__(kSortThreads) void sort_keys_kernel(SortLayout L, const float4* __restrict__ rays, uint32_t n,
                                                                 uint32_t chunk, uint16_t* __restrict__ keys,
                                                                 uint32_t* __restrict__ matrix) {
  __shared__ uint32_t cnt[kSortBuckets];
  for (int b = threadIdx.x; b < kSortBuckets; b += kSortThreads) cnt[b] = 0;
  __syncthreads();
  const uint32_t begin = blockIdx.x * chunk;
  const uint32_t end = begin + min(chunk, n - begin);  // (begin < n: the host launches ceil(n / chunk) workgroups)
  for (uint32_t base = begin; base < end; base += kSortThreads * kSortRaysPerLane) {
    float4 r0[kSortRaysPerLane], r1[kSortRaysPerLane];
#pragma unroll
    for (int r = 0; r < kSortRaysPerLane; ++r) {
      const uint32_t idx = base + r * kSortThreads + threadIdx.x;
      if (idx < end) {
        r0[r] = rays[static_cast<uint64_t>(idx) * 2];
        r1[r] = rays[static_cast<uint64_t>(idx) * 2 + 1];
      }
    }
#pragma unroll
    for (int r = 0; r < kSortRaysPerLane; ++r) {
      const uint32_t idx = base + r * kSortThreads + threadIdx.x;
      if (idx < end) {
        float p[kSortAxes];
        const bool ok = sort_point(r0[r].x, r0[r].y, r0[r].z, r1[r].x, r1[r].y, r1[r].z, p);
        const uint32_t key = ok ? sort_key(L, p) : kSortInvalidKey;
        keys[idx] = static_cast<uint16_t>(key);
        atomicAdd(&cnt[key], 1u);
      }
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < kSortBuckets; b += kSortThreads) matrix[static_cast<uint32_t>(b) * gridDim.x + blockIdx.x] = cnt[b];
}

// Exclusive scan of one value per lane over a workgroup of kScanThreads lanes: shuffles inside a wave, the wave
// sums through LDS. `total` is the workgroup's sum.
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* wave_sum, uint32_t& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = __shfl_up(inc, off, 64);
    if (lane >= off) inc += t;
  }
  if (lane == 63) wave_sum[wave] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < kScanThreads / 64; ++w) {
    const uint32_t t = wave_sum[w];
    before += w < wave ? t : 0u;
    all += t;
  }
  __syncthreads();  // wave_sum is free for the next call
  total = all;
  return before + inc - v;
}

__global__ __launch_bounds__(kScanThreads) void sort_scan_reduce_kernel(const uint4* __restrict__ matrix, uint32_t* __restrict__ tile_sums) {
  __shared__ uint32_t wave_sum[kScanThreads / 64];
  const uint4 x = matrix[static_cast<uint32_t>(blockIdx.x) * kScanThreads + threadIdx.x];
  uint32_t total;
  (void)block_scan(x.x + x.y + x.z + x.w, wave_sum, total);
  if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kScanThreads) void sort_scan_spine_kernel(uint32_t* __restrict__ tile_sums, uint32_t tiles) {
  __shared__ uint32_t wave_sum[kScanThreads / 64];
  uint32_t carry = 0;
  for (uint32_t base = 0; base < tiles; base += kScanThreads) {
    const uint32_t i = base + threadIdx.x;
    uint32_t total;
    const uint32_t ex = block_scan(i < tiles ? tile_sums[i] : 0u, wave_sum, total);
    if (i < tiles) tile_sums[i] = carry + ex;
    carry += total;
  }
}

__global__ __launch_bounds__(kScanThreads) void sort_scan_apply_kernel(uint4* __restrict__ matrix, const uint32_t* __restrict__ tile_sums) {
  __shared__ uint32_t wave_sum[kScanThreads / 64];
  const uint32_t i = static_cast<uint32_t>(blockIdx.x) * kScanThreads + threadIdx.x;
  const uint4 x = matrix[i];
  uint32_t total;
  const uint32_t s = tile_sums[blockIdx.x] + block_scan(x.x + x.y + x.z + x.w, wave_sum, total);
  matrix[i] = make_uint4(s, s + x.x, s + x.x + x.y, s + x.x + x.y + x.z);
}

__global__ __launch_bounds__(kSortThreads) void sort_scatter_kernel(const uint16_t* __restrict__ keys, uint32_t n, uint32_t chunk,
                                                                    const uint32_t* __restrict__ matrix, uint32_t* __restrict__ perm) {
  __shared__ uint32_t start[kSortBuckets];
  for (int b = threadIdx.x; b < kSortBuckets; b += kSortThreads) start[b] = matrix[static_cast<uint32_t>(b) * gridDim.x + blockIdx.x];
  __syncthreads();
  const uint32_t begin = blockIdx.x * chunk;
  const uint32_t end = begin + min(chunk, n - begin);
  for (uint32_t idx = begin + threadIdx.x; idx < end; idx += kSortThreads) {
    const uint32_t key = keys[idx] & (kSortBuckets - 1);
    const uint32_t at = atomicAdd(&start[key], 1u);
    if (at < n) perm[at] = idx;  // (always: the starts are the scan of these keys' counts)
  }
}

}  // namespace

bool sort_box_host(const rtg_ray* rays, int64_t n, float lo[kSortAxes], float hi[kSortAxes]) {
  bool any = false;
  for (int64_t k = 0; k < n; ++k) sort_box_add(rays[k], &any, lo, hi);
  return any;
}

void sort_layout(const float lo[kSortAxes], const float hi[kSortAxes], bool empty, double scene_extent, SortLayout* L) {
  *L = SortLayout{};
  if (empty) return;
  double cell[kSortAxes];  // the width of an axis' cells, relative
  for (int a = 0; a < kSortAxes; ++a) {
    const double ext = static_cast<double>(hi[a]) - static_cast<double>(lo[a]);
    cell[a] = a < 3 ? ext / (scene_extent > 0.0 ? scene_extent : 1.0) : ext / 2.0;
  }
  int bits[kSortAxes] = {};
  for (int k = 0; k < kSortKeyBits; ++k) {
    int widest = 0;
    for (int a = 1; a < kSortAxes; ++a)
      if (cell[a] > cell[widest]) widest = a;
    if (!(cell[widest] > 0.0)) break;
    ++bits[widest];
    cell[widest] *= 0.5;
  }
  int used = 0;
  for (int a = 0; a < kSortAxes; ++a) used += bits[a];
  int next = used - 1;  // the key's bits from the top: origin axes round by round, then the direction axes
  for (int group = 0; group < 2; ++group)
    for (int round = 0; round < kSortKeyBits; ++round)
      for (int a = group * 3; a < group * 3 + 3; ++a)
        if (bits[a] > round) L->pos[a][bits[a] - 1 - round] = static_cast<uint8_t>(next--);
  for (int a = 0; a < kSortAxes; ++a) {
    const float cells = static_cast<float>(1 << bits[a]);
    L->bits[a] = static_cast<uint8_t>(bits[a]);
    L->lo[a] = lo[a];
    L->scale[a] = bits[a] > 0 ? cells / (hi[a] - lo[a]) : 0.0f;
    L->top[a] = cells - 1.0f;
  }
}

size_t sort_plan(int64_t n, int num_cus, void* base, SortPlan* P) {
  auto a16 = [](size_t x) { return (x + 15) & ~size_t(15); };
  const int64_t step = kSortThreads * kSortRaysPerLane;
  const int64_t cap = std::max(1, num_cus * kSortWgsPerCu);
  int64_t chunk = std::max<int64_t>(RTG_QUERY_SORT_CHUNK, (n + cap - 1) / cap);
  chunk = (chunk + step - 1) / step * step;
  const int64_t wgs = (n + chunk - 1) / chunk;
  const size_t perm = 0, matrix = a16(static_cast<size_t>(n) * 4);
  const size_t sums = matrix + static_cast<size_t>(wgs) * kSortBuckets * 4;
  const size_t keys = a16(sums + static_cast<size_t>(wgs) * (kSortBuckets / kSortScanTile) * 4);
  P->chunk = static_cast<uint32_t>(chunk);
  P->workgroups = static_cast<uint32_t>(wgs);
  if (base) {
    char* b = static_cast<char*>(base);
    P->perm = reinterpret_cast<uint32_t*>(b + perm);
    P->matrix = reinterpret_cast<uint32_t*>(b + matrix);
    P->tile_sums = reinterpret_cast<uint32_t*>(b + sums);
    P->keys = reinterpret_cast<uint16_t*>(b + keys);
  }
  return keys + static_cast<size_t>(n) * 2;
}

hipError_t launch_ray_sort(const SortLayout& L, const void* rays, uint32_t n, const SortPlan& P, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const uint32_t tiles = P.workgroups * (kSortBuckets / kSortScanTile);
  hipLaunchKernelGGL(sort_keys_kernel, dim3(P.workgroups), dim3(kSortThreads), 0, stream, L, static_cast<const float4*>(rays), n,
                     P.chunk, P.keys, P.matrix);
  hipLaunchKernelGGL(sort_scan_reduce_kernel, dim3(tiles), dim3(kScanThreads), 0, stream, reinterpret_cast<const uint4*>(P.matrix),
                     P.tile_sums);
  hipLaunchKernelGGL(sort_scan_spine_kernel, dim3(1), dim3(kScanThreads), 0, stream, P.tile_sums, tiles);
  hipLaunchKernelGGL(sort_scan_apply_kernel, dim3(tiles), dim3(kScanThreads), 0, stream, reinterpret_cast<uint4*>(P.matrix),
                     P.tile_sums);
  hipLaunchKernelGGL(sort_scatter_kernel, dim3(P.workgroups), dim3(kSortThreads), 0, stream, P.keys, n, P.chunk, P.matrix, P.perm);
  return hipGetLastError();
}

}  // namespace rtg
