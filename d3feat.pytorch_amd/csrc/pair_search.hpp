// The per-query search of a cloud-pair cell list, shared by the nearest-neighbour kernel (nearest_pairs.hip) and the
// ICP search kernel (icp.hip) so that both evaluate ONE statement of the contract:
//   q  = f32(((T0 x + T1 y) + T2 z) + T3) per component, in f64, x y z the f32 source coordinates widened;
//   d2 = ((dx dx) + (dy dy)) + (dz dz) in f32 without FMA (d3f::sqdist_exact), accepted when d2 < radius * radius
//        (f32 product), the lowest target index among equal d2;
//   a query whose cell lies outside the addressable grid sets D3F_ST_CELL_RANGE in the caller's status word and finds
//   nothing.
// A group of G lanes serves one query (work distribution: nearest_pairs.hip's header).
#pragma once
#include "cell_list.hpp"

namespace d3f {
namespace cells {

// largest p in [lo, n - 1] with pre[p] <= r, for a non-decreasing prefix pre[0..n] with pre[lo] <= r < pre[n]
template <typename T>
__device__ __forceinline__ int prefix_find(const T* __restrict__ pre, int lo, int n, long long r) {
  int hi = n;
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((long long)pre[mid] <= r) lo = mid; else hi = mid;
  }
  return lo;
}

// cell coordinate as cell_coord computes it, or false when it (or a neighbour cell) cannot be keyed
__device__ __forceinline__ bool query_cell(float v, double inv_cell, int& c) {
  const double f = floor((double)v * inv_cell);
  const bool ok = f >= -32767.0 && f <= 32766.0;   // false for NaN too
  c = ok ? (int)f : 0;
  return ok;
}

// the cell list and the radius of one launch
struct CellSearch {
  const int32_t* start;
  const int32_t* end;
  const float4* pts;
  const uint64_t* key;
  double inv_cell;
  float r2, prune_r;
  uint32_t mask;
};

// The CellSearch of one launch at `radius` over the list in grid_ws (d3f_cloud_grid_build / d3f_radius_grid_build over
// Ns rows at grid_radius >= radius); *placement is the list's placement word (cell_list.hpp).
inline CellSearch cell_search(const void* grid_ws, int Ns, float grid_radius, float radius, const int32_t** placement) {
  const GridLayout g = grid_layout(const_cast<void*>(grid_ws), Ns);
  CellSearch S;
  S.start = g.start;
  S.end = g.end;
  S.pts = g.pts;
  S.key = g.key;
  S.inv_cell = 1.0 / ((double)grid_radius * kCellSlack);   // cells of the list the grid was built with
  S.r2 = radius * radius;                                  // float32 product, like the radius search
  S.prune_r = radius;
  S.mask = g.M - 1;
  *placement = g.cnt + g.M + kPlacementWord;
  return S;
}

// Bucket headers of the cells lane `sub` of a group of G walks for the query point (qx, qy, qz) in cell (cx, cy, cz) of
// cloud b (first stored row tgt0, tgt_n rows): per cell the key nk, the first entry st and the length len (0 for a
// cell it skips).  The 27 cells are dealt round robin to the lanes; the loads are independent.  A cell whose box is
// farther from the query than the radius holds no accepted point and is skipped (same margin as radius_query_kernel).
template <int G>
__device__ __forceinline__ void cell_headers(const CellSearch& S, bool ok, float qx, float qy, float qz, int cx, int cy,
                                             int cz, int b, int tgt0, int tgt_n, bool per_cloud, double cell,
                                             double reach, int sub, uint64_t (&nk)[(27 + G - 1) / G],
                                             int (&st)[(27 + G - 1) / G], int (&len)[(27 + G - 1) / G]) {
  constexpr int kCells = (27 + G - 1) / G;
#pragma unroll
  for (int c = 0; c < kCells; ++c) {
    const int k = sub + c * G;
    st[c] = len[c] = 0;
    nk[c] = 0;
    if (ok && tgt_n > 0 && k < 27) {
      const int dx = k % 3 - 1, dy = (k / 3) % 3 - 1, dz = k / 9 - 1;
      auto gap = [&](float v, int cc) -> double {
        const double lo = (double)cc * cell, hi = lo + cell, xx = (double)v;
        return xx < lo ? lo - xx : (xx > hi ? xx - hi : 0.0);
      };
      const double gx = gap(qx, cx + dx), gy = gap(qy, cy + dy), gz = gap(qz, cz + dz);
      if (gx * gx + gy * gy + gz * gz <= reach * reach) {
        nk[c] = pack_key(b, cx + dx, cy + dy, cz + dz);
        const uint32_t bk = per_cloud ? bucket_of_cloud(nk[c], 2u * tgt0, 2u * tgt_n) : bucket_of(nk[c], S.mask);
        st[c] = S.start[bk];
        len[c] = S.end[bk] - st[c];
      }
    }
  }
}

// The query (x, y, z) of target cloud b (first stored row tgt0, tgt_n rows) under the row-major 3x4 transform T, by the
// G lanes of its group (sub = lane & (G - 1)).  Returns the group's least packed key (d2 bits << 32 | global index of
// the stored point), ~0 when none is accepted; `mine` is this LANE's least key and `win` the stored point that gave it,
// so the one lane with mine == the returned key holds the winner's coordinates.  `ok` is cleared when the query's cell
// is not addressable (D3F_ST_CELL_RANGE is then OR-ed into *status by the group's first lane).
template <int G>
__device__ __forceinline__ uint64_t nearest_in_cloud(const CellSearch& S, bool& ok, double x, double y, double z,
                                                     const double* __restrict__ T, int b, int tgt0, int tgt_n,
                                                     bool per_cloud, double cell, double reach, int sub,
                                                     int32_t* status, uint64_t& mine, float4& win) {
  constexpr int kCells = (27 + G - 1) / G;   // cells per lane
  float qx = 0.0f, qy = 0.0f, qz = 0.0f;
  int cx = 0, cy = 0, cz = 0;
  if (ok) {
    qx = (float)(((T[0] * x + T[1] * y) + T[2] * z) + T[3]);   // (-ffp-contract=off: no FMA)
    qy = (float)(((T[4] * x + T[5] * y) + T[6] * z) + T[7]);
    qz = (float)(((T[8] * x + T[9] * y) + T[10] * z) + T[11]);
    const bool in_x = query_cell(qx, S.inv_cell, cx), in_y = query_cell(qy, S.inv_cell, cy),
               in_z = query_cell(qz, S.inv_cell, cz);
    if (!(in_x && in_y && in_z)) {
      if (sub == 0) atomicOr(status, D3F_ST_CELL_RANGE);
      ok = false;
    }
  }

  uint64_t nk[kCells];
  int st[kCells], len[kCells];
  int longest = 0;
  cell_headers<G>(S, ok, qx, qy, qz, cx, cy, cz, b, tgt0, tgt_n, per_cloud, cell, reach, sub, nk, st, len);
#pragma unroll
  for (int c = 0; c < kCells; ++c) longest = len[c] > longest ? len[c] : longest;
  // the lane's buckets side by side: entry t of each of them is loaded before any is looked at, so a step costs one
  // memory latency, not one per cell (an exhausted bucket re-reads entry 0 of the list, which its key check discards)
  uint64_t best = ~0ull;
  win = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  for (int t = 0; t < longest; ++t) {
    uint64_t kk[kCells];
    float4 sp[kCells];
#pragma unroll
    for (int c = 0; c < kCells; ++c) {
      const int pos = t < len[c] ? st[c] + t : 0;
      kk[c] = S.key[pos];
      sp[c] = S.pts[pos];
    }
#pragma unroll
    for (int c = 0; c < kCells; ++c) {
      const float d2 = d3f::sqdist_exact(qx, qy, qz, sp[c].x, sp[c].y, sp[c].z);
      const uint64_t packed = ((uint64_t)__float_as_uint(d2) << 32) | (uint32_t)__float_as_int(sp[c].w);
      // (kk == nk: not another cell hashed into the same bucket)
      if (t < len[c] && kk[c] == nk[c] && d2 < S.r2 && packed < best) {
        best = packed;
        win = sp[c];
      }
    }
  }
  mine = best;
#pragma unroll
  for (int o = 1; o < G; o <<= 1) {
    const uint64_t other = d3f::shfl_xor_u64(best, o);
    best = other < best ? other : best;
  }
  return best;
}

}  // namespace cells
}  // namespace d3f
