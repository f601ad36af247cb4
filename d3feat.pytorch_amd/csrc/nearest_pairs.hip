// Nearest neighbour within a radius over a LIST of cloud pairs -- the mining step of the 3DMatch training pickles
// (datasets/preprocess.py): for pair p = (source cloud a, target cloud b, rigid transform T_p) every point of a is moved
// into b's frame and its nearest point of b with d2 < radius^2 is looked up.  The reference has no counterpart (its
// README points to the authors' download for the finished files).
//
// One cell list over ALL clouds of a scene (cell_list.hpp; the cloud index is the batch element of the cell key) serves
// every pair, so a fragment is stored once however many partners it has.  The list comes from d3f_cloud_grid_build
// below (clouds located by a prefix of their lengths, up to 65535 of them, every cloud's buckets and points contiguous:
// cell_list.hpp) or from d3f_radius_grid_build (up to D3F_MAX_BATCH clouds hashed into one table); the list says which.
//
// Result contract (restated in NumPy by datasets/preprocess.py, bit for bit):
//   q  = f32(((T0 x + T1 y) + T2 z) + T3) per component, in f64, x y z the f32 source coordinates widened;
//   d2 = ((dx dx) + (dy dy)) + (dz dz) in f32 without FMA (d3f::sqdist_exact), accepted when d2 < radius * radius
//        (f32 product), the lowest target index among equal d2;
//   a query whose cell lies outside the addressable grid sets D3F_ST_CELL_RANGE and yields -1.
//
// Work distribution: a group of G lanes (G = 8 unless asked otherwise) serves one query.  The 27 cells are dealt round
// robin to the lanes of the group, each lane walks the buckets of its cells side by side and keeps the minimum of the
// packed key (d2 bits << 32 | index), the group's minimum is taken by G's log2 DPP exchanges.  At 1.25 voxel sizes a
// query meets a few dozen candidates in ~9 occupied cells: a whole wave per query (radius_neighbors.hip, which has to
// RANK its candidates) leaves most lanes idle, a lane per query serialises 27 dependent bucket walks.  Measured on a
// 60-fragment scene (profiles/nearest_pairs_bench.txt): 4, 8 and 16 lanes are within 4 % of each other (15.0 / 15.2 /
// 15.5 ms for 42 M queries), 32 lanes 13 % behind -- the kernel is bound by the number of cache lines it asks the L2
// for (two 4-byte headers per cell out of two arrays, 24 B per candidate out of two more), not by its lanes.
#include "pair_search.hpp"

namespace {

using namespace d3f::cells;
using d3f::shfl_xor_u64;

constexpr int kBlock = 512;   // 8 waves share one add to out_count

constexpr uint64_t kNoKey = ~0ull;   // no cell key has the cloud field 65535 (B <= kMaxClouds)

__global__ void cloud_count_kernel(const float* __restrict__ s, int Ns, const int32_t* __restrict__ cloud_start, int B,
                                   double inv_cell, uint32_t mask, int32_t* __restrict__ cnt,
                                   uint64_t* __restrict__ key_tmp, int32_t* __restrict__ status) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) cnt[mask + 1 + kPlacementWord] = 1;   // per-cloud tables (cell_list.hpp)
  if (i >= Ns || i >= cloud_start[B]) return;  // Ns is a row capacity; cloud_start[B] rows are live
  const int b = prefix_find(cloud_start, 0, B, i);
  // a point outside the addressable cells (or not finite) is reported and NOT inserted: its packed key would spill into
  // the cloud field, and the scatter must find every point in the bucket it was counted in
  int cx, cy, cz;
  const bool in_x = query_cell(s[3 * i + 0], inv_cell, cx), in_y = query_cell(s[3 * i + 1], inv_cell, cy),
             in_z = query_cell(s[3 * i + 2], inv_cell, cz);
  if (!(in_x && in_y && in_z)) {
    atomicOr(status, D3F_ST_CELL_RANGE);
    key_tmp[i] = kNoKey;
    return;
  }
  const uint64_t key = pack_key(b, cx, cy, cz);
  key_tmp[i] = key;
  const int first = cloud_start[b];
  atomicAdd(&cnt[bucket_of_cloud(key, 2u * first, 2u * (cloud_start[b + 1] - first))], 1);
}

__global__ void cloud_scatter_kernel(const float* __restrict__ s, int Ns, const int32_t* __restrict__ cloud_start, int B,
                                     const uint64_t* __restrict__ key_tmp, int32_t* __restrict__ end,
                                     float4* __restrict__ pts, uint64_t* __restrict__ key) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Ns || i >= cloud_start[B]) return;
  const uint64_t k = key_tmp[i];
  if (k == kNoKey) return;   // not counted, not stored
  // (the key's cloud field is the b the count kernel found: only in-range cells are packed, so nothing spills into it)
  const int b = (int)(k >> 48), first = cloud_start[b];
  const int pos = atomicAdd(&end[bucket_of_cloud(k, 2u * first, 2u * (cloud_start[b + 1] - first))], 1);
  pts[pos] = make_float4(s[3 * i + 0], s[3 * i + 1], s[3 * i + 2], __int_as_float(i));
  key[pos] = k;
}

struct PairArgs {
  const float* points;
  const int32_t* cloud_start;
  const int32_t* pairs;
  const double* transforms;
  const int64_t* row_start;
  const int32_t* placement;   // cell_list.hpp: 0 = one hashed table, 1 = per-cloud tables
  int32_t* out_nn;
  int32_t* out_count;
  int32_t* status;
  CellSearch S;   // pair_search.hpp
  long long rows;
  int B, P, Ns, iters;
};

template <int G>
__global__ __launch_bounds__(kBlock) void nearest_pairs_kernel(const PairArgs A) {
  constexpr int kRowsPerWave = 64 / G, kRowsPerBlock = (kBlock / 64) * kRowsPerWave;
  const int lane = threadIdx.x & 63, sub = lane & (G - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long long total = A.row_start[A.P] < A.rows ? A.row_start[A.P] : A.rows;   // rows is out_nn's capacity
  const bool per_cloud = *A.placement != 0;
  const double cell = 1.0 / A.S.inv_cell, reach = (double)A.S.prune_r * (1.0 + 1e-4);
  // a workgroup serves A.iters consecutive slices of kRowsPerBlock rows: the pair of a wave's first row is searched for
  // once and then followed, and the hits of a pair are added to out_count once per wave and pair, not once per slice
  // (thousands of waves adding to ONE word each slice serialise on it: 12 of 17 ms of a scene went there)
  const long long base = (long long)blockIdx.x * A.iters * kRowsPerBlock + wave * kRowsPerWave;
  int p0 = -1, acc = 0, acc_p = 0;
  long long p0_end = 0;
  for (int it = 0; it < A.iters; ++it) {
    const long long r0 = base + (long long)it * kRowsPerBlock;   // the wave's first row (wave-uniform)
    if (r0 >= total) break;   // (the one workgroup barrier is after the loop)
    if (p0 < 0 || r0 >= p0_end) {
      p0 = prefix_find(A.row_start, p0 < 0 ? 0 : p0 + 1, A.P, r0);
      p0_end = A.row_start[p0 + 1];
    }
    const long long r = r0 + lane / G;
    const bool live = r < total;
    int p = p0;   // a lane's own row is almost always in the pair of the wave's first row
    if (live && r >= p0_end) p = prefix_find(A.row_start, p0 + 1, A.P, r);
    const int a = A.pairs[2 * p], b = A.pairs[2 * p + 1];
    bool ok = live && (unsigned)a < (unsigned)A.B && (unsigned)b < (unsigned)A.B;
    int src = 0, tgt0 = 0, tgt_n = 0;
    if (ok) {
      const int sa = A.cloud_start[a];
      const long long i = r - A.row_start[p];
      ok = i < (long long)(A.cloud_start[a + 1] - sa) && sa + i < (long long)A.Ns;   // (row_start: prefix of the SOURCE lengths)
      src = ok ? sa + (int)i : 0;
      tgt0 = A.cloud_start[b];
      tgt_n = A.cloud_start[b + 1] - tgt0;
    }

    double x = 0.0, y = 0.0, z = 0.0;
    if (ok) {
      x = (double)A.points[3 * (size_t)src + 0];
      y = (double)A.points[3 * (size_t)src + 1];
      z = (double)A.points[3 * (size_t)src + 2];
    }
    uint64_t mine;
    float4 win;   // (the winner's coordinates: the ICP kernel's sums want them, nothing here does)
    const uint64_t best = nearest_in_cloud<G>(A.S, ok, x, y, z, A.transforms + 12 * (size_t)p, b, tgt0, tgt_n, per_cloud,
                                              cell, reach, sub, A.status, mine, win);
    const bool found = live && sub == 0 && best != ~0ull;
    if (live && sub == 0) A.out_nn[r] = found ? (int32_t)(uint32_t)best - tgt0 : -1;

    const uint64_t hits = __ballot(found);
    // (the wave is converged here: the loop's only exit above is wave-uniform, so __all / __ballot see all 64 lanes)
    if (__all(!live || p == p0)) {   // all but the waves on a pair boundary
      if (acc_p != p0) {
        if (lane == 0 && acc) atomicAdd(&A.out_count[acc_p], acc);
        acc = 0;
        acc_p = p0;
      }
      acc += (int)__popcll(hits);
    } else {   // a wave across a pair boundary: one add per pair it holds
      uint64_t rest = hits;
      while (rest) {
        const int first = __ffsll((unsigned long long)rest) - 1;
        const int pp = __shfl(p, first, 64);
        const uint64_t same = __ballot(found && p == pp);
        if (lane == first) atomicAdd(&A.out_count[pp], (int)__popcll(same));
        rest &= ~same;
      }
    }
  }
  // what the waves of the workgroup still hold goes out as ONE add when it belongs to one pair (it nearly always does)
  __shared__ int w_pair[kBlock / 64], w_hits[kBlock / 64];
  if (lane == 0) {
    w_pair[wave] = acc_p;
    w_hits[wave] = acc;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int sum = 0, pair = -1;
    bool one = true;
    for (int w = 0; w < kBlock / 64; ++w) {
      if (!w_hits[w]) continue;
      if (pair >= 0 && w_pair[w] != pair) one = false;
      pair = w_pair[w];
      sum += w_hits[w];
    }
    if (one) {
      if (sum) atomicAdd(&A.out_count[pair], sum);
    } else {
      for (int w = 0; w < kBlock / 64; ++w)
        if (w_hits[w]) atomicAdd(&A.out_count[w_pair[w]], w_hits[w]);
    }
  }
}

template <int G>
void launch_pairs(PairArgs& a, hipStream_t stream) {
  const long long per_block = (kBlock / 64) * (64 / G);
  // slices per workgroup: as many as leave every CU a few dozen workgroups (the result does not depend on it)
  long long iters = a.rows / (per_block * 8192);
  a.iters = (int)(iters < 1 ? 1 : (iters > 16 ? 16 : iters));
  const long long span = per_block * a.iters;
  nearest_pairs_kernel<G><<<(unsigned)((a.rows + span - 1) / span), kBlock, 0, stream>>>(a);
}

}  // namespace

extern "C" {

int d3f_cloud_grid_build(const float* points, int Ns, const int32_t* cloud_start, int B, float radius, void* grid_ws,
                         size_t grid_ws_bytes, int32_t* status, void* stream_) {
  if (!points || !cloud_start || !grid_ws || !status || Ns < 0 || B < 1 || B > kMaxClouds || !(radius > 0.0f))
    return D3F_EINVAL;
  hipStream_t stream = (hipStream_t)stream_;
  GridLayout g = grid_layout(grid_ws, Ns);
  if (grid_ws_bytes < g.bytes) return D3F_EWORKSPACE;
  const double inv_cell = 1.0 / ((double)radius * kCellSlack);
  if (d3f::zero_async(g.cnt, sizeof(int32_t) * (g.M + 64), stream) != hipSuccess) return D3F_ELAUNCH;
  if (Ns > 0) {
    cloud_count_kernel<<<d3f::cdiv(Ns, 256), 256, 0, stream>>>(points, Ns, cloud_start, B, inv_cell, g.M - 1, g.cnt,
                                                              g.key_tmp, status);
    D3F_LAUNCH_CHECK();
  }
  grid_alloc_kernel<<<d3f::cdiv(g.M, 1024), 1024, 0, stream>>>(g.M, g.cnt, g.start, g.end);
  D3F_LAUNCH_CHECK();
  if (Ns > 0) {
    cloud_scatter_kernel<<<d3f::cdiv(Ns, 256), 256, 0, stream>>>(points, Ns, cloud_start, B, g.key_tmp, g.end, g.pts,
                                                                g.key);
    D3F_LAUNCH_CHECK();
  }
  return D3F_OK;
}

int d3f_nearest_pairs_lanes(const void* grid_ws, const float* points, int Ns, const int32_t* cloud_start, int B,
                            float grid_radius, float radius, const int32_t* pairs, const double* transforms,
                            const int64_t* row_start, int P, int64_t rows, int32_t* out_nn, int32_t* out_count,
                            int32_t* status, int lanes, void* stream_) {
  if (!grid_ws || !points || !cloud_start || !row_start || !status || Ns < 0 || B < 1 || B > kMaxClouds || P < 0 ||
      rows < 0 || rows > 0x7fffffffll || !(radius > 0.0f) || !(grid_radius >= radius) ||
      (P > 0 && (!pairs || !transforms || !out_count)) || (rows > 0 && !out_nn))
    return D3F_EINVAL;
  if (lanes != 0 && lanes != 4 && lanes != 8 && lanes != 16 && lanes != 32) return D3F_EINVAL;
  if (P == 0 || rows == 0) return D3F_OK;
  PairArgs a;
  a.points = points;
  a.cloud_start = cloud_start;
  a.pairs = pairs;
  a.transforms = transforms;
  a.row_start = row_start;
  a.S = cell_search(grid_ws, Ns, grid_radius, radius, &a.placement);
  a.out_nn = out_nn;
  a.out_count = out_count;
  a.status = status;
  a.rows = rows;
  a.B = B;
  a.P = P;
  a.Ns = Ns;
  hipStream_t stream = (hipStream_t)stream_;
  switch (lanes) {
    case 4: launch_pairs<4>(a, stream); break;
    case 16: launch_pairs<16>(a, stream); break;
    case 32: launch_pairs<32>(a, stream); break;
    default: launch_pairs<8>(a, stream); break;
  }
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_nearest_pairs(const void* grid_ws, const float* points, int Ns, const int32_t* cloud_start, int B,
                      float grid_radius, float radius, const int32_t* pairs, const double* transforms,
                      const int64_t* row_start, int P, int64_t rows, int32_t* out_nn, int32_t* out_count,
                      int32_t* status, void* stream_) {
  return d3f_nearest_pairs_lanes(grid_ws, points, Ns, cloud_start, B, grid_radius, radius, pairs, transforms, row_start,
                                 P, rows, out_nn, out_count, status, 0, stream_);
}

}  // extern "C"
