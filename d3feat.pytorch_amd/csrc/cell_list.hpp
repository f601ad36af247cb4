// The hashed uniform cell list shared by the radius search (radius_neighbors.hip) and the nearest-neighbour search over
// cloud pairs (nearest_pairs.hip): workspace layout, cell key, bucket hash and the range allocator.  A list built by either
// file's build entry is read by nearest_pairs.hip's query; the radius search reads its own.
//
// Supports are bucketed by a 64-bit cell key (cloud, cx, cy, cz) hashed into a power-of-two table; the cell edge is
// radius * kCellSlack and cell coordinates are computed in f64, so a 27-cell scan provably covers every support with
// d2 < radius^2.  Hash collisions neither lose nor duplicate candidates: the searches over cloud pairs
// (pair_search.hpp) accept a point only while scanning ITS OWN cell key; radius_neighbors.hip scans every distinct bucket of a query once and accepts a point iff it
// belongs to the query's cloud and d2 < radius^2, without reading the keys (the argument is at the head of that file).
#pragma once
#include "common.hpp"

namespace d3f {
namespace cells {

constexpr double kCellSlack = 1.0 + 1e-4;

__host__ __device__ inline uint32_t table_size_for(int Ns) {
  uint32_t m = 64;
  while (m < 2u * (uint32_t)(Ns > 0 ? Ns : 1)) m <<= 1;
  return m;
}

struct GridLayout {
  uint32_t M;
  int32_t* cnt;      // [M + 64]  per-bucket population; cnt[M] is the global range allocator
  int32_t* start;    // [M]
  int32_t* end;      // [M]       fill cursor during the scatter == range end afterwards
  uint64_t* key_tmp; // [Ns]      cell key of support i (input order)
  float4* pts;       // [Ns]      supports in bucket order: x, y, z, bit-cast global index
  uint64_t* key;     // [Ns]      cell key per sorted support
  size_t bytes;
};

inline GridLayout grid_layout(void* ws, int Ns) {
  GridLayout g;
  g.M = table_size_for(Ns);
  Carver c(ws);
  const size_t n = (size_t)(Ns > 0 ? Ns : 1);
  g.cnt = c.take<int32_t>(g.M + 64);
  g.start = c.take<int32_t>(g.M);
  g.end = c.take<int32_t>(g.M);
  g.key_tmp = c.take<uint64_t>(n);
  g.pts = c.take<float4>(n);
  g.key = c.take<uint64_t>(n);
  g.bytes = align_up(c.off, 256);
  return g;
}

__device__ __forceinline__ int cell_coord(float v, double inv_cell) { return (int)floor((double)v * inv_cell); }

// the key keeps the cloud (batch element) in its top 16 bits; 65535 itself stays free for "no key" marks
constexpr int kMaxClouds = 65535;
__device__ __forceinline__ uint64_t pack_key(int b, int cx, int cy, int cz) {
  return ((uint64_t)(uint32_t)b << 48) | ((uint64_t)(uint32_t)(cx + 32768) << 32) |
         ((uint64_t)(uint32_t)(cy + 32768) << 16) | (uint64_t)(uint32_t)(cz + 32768);
}

__device__ __forceinline__ uint32_t bucket_of(uint64_t key, uint32_t mask) {
  return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32) & mask;
}

// Per-cloud tables (d3f_cloud_grid_build): cloud b owns the buckets [2 start_b, 2 start_b + 2 len_b) of the same table,
// so the headers and -- ranges being handed out bucket by bucket -- the stored points of ONE cloud are contiguous: the
// searches against a target cloud touch ~40 B per target point instead of cache lines spread over the whole scene's
// list.  The hash is reduced to the cloud's range by a multiply-shift.  Which of the two placements a list uses is
// written into the list itself: cnt[M + kPlacementWord] is 0 (one hashed table, d3f_radius_grid_build) or 1.
constexpr int kPlacementWord = 1;
__device__ __forceinline__ uint32_t bucket_of_cloud(uint64_t key, uint32_t first, uint32_t n) {
  const uint32_t h = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32);
  return first + (uint32_t)(((uint64_t)h * n) >> 32);
}

__global__ static __launch_bounds__(1024) void grid_alloc_kernel(uint32_t M, int32_t* __restrict__ cnt,
                                                          int32_t* __restrict__ start, int32_t* __restrict__ end) {
  // ranges need to be disjoint, not ordered; the running total is ONE word, so a whole workgroup of 16 waves reserves
  // its buckets together (wave scans, wave totals combined through LDS, one atomic) -- per-bucket atomics on that word
  // serialise, per-wave ones still queued 2048 deep at level 0 (23 us)
  __shared__ int wtot[16], wbase[16];
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = b < M ? cnt[b] : 0;
  int incl = c;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
    for (int w = 0; w < 16; ++w) { wbase[w] = total; total += wtot[w]; }
    const int base = total > 0 ? atomicAdd(&cnt[M], total) : 0;
    for (int w = 0; w < 16; ++w) wbase[w] += base;
  }
  __syncthreads();
  if (b >= M) return;
  const int s = c ? wbase[wave] + incl - c : 0;
  start[b] = s;
  end[b] = s;
}

}  // namespace cells
}  // namespace d3f
