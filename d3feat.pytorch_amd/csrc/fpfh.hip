// FPFH descriptors of every point of the stacked clouds of one cell list -- what the reference's users compute with
// Open3D's compute_fpfh_feature on the CPU, and the training-free descriptor of the registration chain.  fpfh.hpp states
// the rule; this file is the two radius passes over a point's OWN cloud that evaluate it and the host twin.
//
// Order independence.  Every sum over neighbours is an integer (fpfh.hpp): the SPFH histograms are int32 counts, the
// FPFH sums int64 products of an integer weight and a count.  Bucket order, lanes, groups, stacking and cell size
// cannot change them, and the descriptor is a function of them alone.
//
// Work distribution, both kernels.  A group of G = 8 lanes serves one query and walks its 27 cells as the pair search
// does (pair_search.hpp: cells dealt round robin, a lane's buckets side by side).  A workgroup is ONE wave and serves 64
// consecutive queries in 8 slices of 8, so a slice's results are 8 consecutive rows; they meet in LDS, where a
// run-time bin index is free, and all 64 lanes write them out as one contiguous run.
//
// The SPFH pass (spfh_kernel).  Per accepted candidate: the neighbour's normal through the input row the stored point
// carries in .w (as icp.hip reads normals), ~60 f64 operations (2 sqrt and 5 divisions among them: pair_bins), three
// ds_add_u32 into the query's 33 counters.  The slice's histograms are 8 x 33 int32 = 1056 B of LDS; the row stride of 33
// words is odd, so the 8 groups of a wave fall into different banks unless their bins differ by the same amount as
// their rows, and lanes of one group that meet in one counter are combined by the LDS atomic unit.  Each row of the
// table the next pass reads is 36 int32: the 33 counts, n, two zeros -- 144 B, nine 16-byte loads.
//
// The FPFH pass (fpfh_kernel).  Per accepted candidate: its table row in nine 16-byte loads, one f64 division and rint
// for W_j, 33 v_mad_i64_i32 into the lane's own int64 sums (compile-time bin index: registers).  The lanes of a group
// add their sums into the slice's 8 x 33 int64 (2112 B of LDS, ds_add_u64); then lane l forms entries l, l + 64, ... of
// the slice's 8 rows -- two f64 divisions each, all lanes busy --, the entries meet in LDS once more so that a lane can
// scale its entry by the row's norm (unit rows), and the 8 rows leave as one contiguous store.
// A neighbour's usable normal is read off its row: n_j >= 1 exactly when j is usable (the neighbour relation is
// symmetric and i is usable), so this pass never loads a normal.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):
//   spfh_kernel: 124 VGPRs, no scratch, no spill, 1056 B LDS, 4 waves per SIMD
//   fpfh_kernel: 183 VGPRs, no scratch, no spill, 3168 B LDS, 2 waves per SIMD
// Measured (profiles/fpfh_bench.txt: 1.45 M points, 121 neighbours each): 14.8 ms and 21.1 ms against 4.9 ms for
// normals_kernel over the same cells.  The SPFH pass is its f64 work.  The FPFH pass is not its 33 multiply-adds, and
// not its occupancy either: with G = 16 (two cells per lane, 161 VGPRs, 3 waves per SIMD) it took 20.1 ms.  What is
// left is the gather itself: every accepted candidate costs its lane nine 16-byte loads, and the 64 lanes of a wave
// load from 64 different rows.  A narrower table (16-bit counts while n < 65536: 80 B a row) is the next thing to try.
#include "fpfh.hpp"
#include "pair_search.hpp"

namespace {

using namespace d3f::cells;
namespace fp = d3f::fpfh;

constexpr int kBlock = 64;   // one wave: the barriers below order a wave's own LDS traffic
constexpr int kG = 8;
constexpr int kPerSlice = 64 / kG;

struct FpfhArgs {
  const float* points;
  const float* nrm;
  const int32_t* cloud_start;
  const int32_t* placement;
  CellSearch S;
  int32_t* table;     // [Ns, kRow]
  int32_t* count;     // [Ns]
  int32_t* spfh;      // [Ns, 33] or null
  float* desc;        // [Ns, row_width]
  int32_t* status;
  double r2;
  int B, Ns, row_width, unit;
};

// the query of one group: its point, cloud and cell; ok is cleared for a row that is not searched
struct Query {
  float px, py, pz;
  int b, c0, cn, cx, cy, cz;
};

__device__ __forceinline__ Query load_query(const FpfhArgs& A, long long i, bool& ok, int sub, bool flag) {
  Query q = {0.0f, 0.0f, 0.0f, 0, 0, 0, 0, 0, 0};
  if (!ok) return q;
  q.px = A.points[3 * (size_t)i + 0];
  q.py = A.points[3 * (size_t)i + 1];
  q.pz = A.points[3 * (size_t)i + 2];
  q.b = prefix_find(A.cloud_start, 0, A.B, i);
  q.c0 = A.cloud_start[q.b];
  q.cn = A.cloud_start[q.b + 1] - q.c0;
  const bool in_x = query_cell(q.px, A.S.inv_cell, q.cx), in_y = query_cell(q.py, A.S.inv_cell, q.cy),
             in_z = query_cell(q.pz, A.S.inv_cell, q.cz);
  if (!(in_x && in_y && in_z)) {   // the build did not store it either
    if (flag && sub == 0) atomicOr(A.status, D3F_ST_CELL_RANGE);
    ok = false;
  }
  return q;
}

template <int G>
__global__ __launch_bounds__(kBlock) void spfh_kernel(const FpfhArgs A) {
  constexpr int kCells = (27 + G - 1) / G;
  __shared__ int32_t hist[kPerSlice * fp::kHist];
  const int lane = threadIdx.x, sub = lane & (G - 1), grp = lane / G;
  const long long base = (long long)blockIdx.x * 64;
  const int live = A.cloud_start[A.B] < A.Ns ? A.cloud_start[A.B] : A.Ns;   // Ns is a row capacity
  const bool per_cloud = *A.placement != 0;
  const double cell = 1.0 / A.S.inv_cell, reach = (double)A.S.prune_r * (1.0 + 1e-4);
  for (int slice = 0; slice < G; ++slice) {
    for (int e = lane; e < kPerSlice * fp::kHist; e += 64) hist[e] = 0;
    __syncthreads();
    const long long first = base + slice * kPerSlice, i = first + grp;
    bool ok = i < live;
    double nix = 0.0, niy = 0.0, niz = 0.0;
    if (ok) {
      const float x = A.nrm[3 * (size_t)i + 0], y = A.nrm[3 * (size_t)i + 1], z = A.nrm[3 * (size_t)i + 2];
      ok = fp::usable_normal(x, y, z);
      nix = (double)x; niy = (double)y; niz = (double)z;
    }
    const Query q = load_query(A, i, ok, sub, true);
    uint64_t nk[kCells];
    int st[kCells], len[kCells], longest = 0;
    cell_headers<G>(A.S, ok, q.px, q.py, q.pz, q.cx, q.cy, q.cz, q.b, q.c0, q.cn, per_cloud, cell, reach, sub, nk, st,
                    len);
#pragma unroll
    for (int c = 0; c < kCells; ++c) longest = len[c] > longest ? len[c] : longest;
    int32_t* mine = hist + grp * fp::kHist;
    for (int t = 0; t < longest; ++t) {
      uint64_t kk[kCells];
      float4 sp[kCells];
#pragma unroll
      for (int c = 0; c < kCells; ++c) {
        const int pos = t < len[c] ? st[c] + t : 0;
        kk[c] = A.S.key[pos];
        sp[c] = A.S.pts[pos];
      }
      bool in[kCells];
      float nj[kCells][3];
#pragma unroll
      for (int c = 0; c < kCells; ++c) {   // the normals of this step's accepted candidates, side by side like the buckets
        const float d2f = d3f::sqdist_exact(q.px, q.py, q.pz, sp[c].x, sp[c].y, sp[c].z);
        in[c] = t < len[c] && kk[c] == nk[c] && d2f < A.S.r2;
        // (.w of a stored point of an accepted cell is an input row below the live rows)
        const size_t j = in[c] ? (size_t)(uint32_t)__float_as_int(sp[c].w) : 0;
        nj[c][0] = A.nrm[3 * j + 0];
        nj[c][1] = A.nrm[3 * j + 1];
        nj[c][2] = A.nrm[3 * j + 2];
      }
#pragma unroll
      for (int c = 0; c < kCells; ++c) {
        const double dx = (double)sp[c].x - (double)q.px, dy = (double)sp[c].y - (double)q.py,
                     dz = (double)sp[c].z - (double)q.pz;
        const double d2 = fp::sqdist_f64(dx, dy, dz);
        if (in[c] && d2 != 0.0 && fp::usable_normal(nj[c][0], nj[c][1], nj[c][2])) {
          int bt, b2, b3;
          fp::pair_bins(dx, dy, dz, d2, nix, niy, niz, (double)nj[c][0], (double)nj[c][1], (double)nj[c][2], bt, b2, b3);
          atomicAdd(mine + bt, 1);
          atomicAdd(mine + fp::kBins + b2, 1);
          atomicAdd(mine + 2 * fp::kBins + b3, 1);
        }
      }
    }
    __syncthreads();
    // the slice's 8 rows of the table are one contiguous run
    for (int e = lane; e < kPerSlice * fp::kRow; e += 64) {
      const int r = e / fp::kRow, col = e % fp::kRow;
      const long long row = first + r;
      if (row >= A.Ns) continue;
      int v = 0;
      if (col < fp::kHist) {
        v = hist[r * fp::kHist + col];
        if (A.spfh) A.spfh[fp::kHist * (size_t)row + col] = v;
      } else if (col == fp::kHist) {
        for (int k = 0; k < fp::kBins; ++k) v += hist[r * fp::kHist + k];   // every histogram sums to n
        A.count[row] = v;
        if (v > fp::kMaxNeighbors) atomicOr(A.status, D3F_ST_CAND_OVERFLOW);
      }
      A.table[fp::kRow * (size_t)row + col] = v;
    }
    __syncthreads();
  }
}

template <int G>
__global__ __launch_bounds__(kBlock) void fpfh_kernel(const FpfhArgs A) {
  constexpr int kCells = (27 + G - 1) / G;
  __shared__ unsigned long long sums[kPerSlice * fp::kHist];
  __shared__ float entries[kPerSlice * fp::kHist];
  const int lane = threadIdx.x, sub = lane & (G - 1), grp = lane / G;
  const long long base = (long long)blockIdx.x * 64;
  const int live = A.cloud_start[A.B] < A.Ns ? A.cloud_start[A.B] : A.Ns;
  const bool per_cloud = *A.placement != 0;
  const double cell = 1.0 / A.S.inv_cell, reach = (double)A.S.prune_r * (1.0 + 1e-4);
  const int4* rows = reinterpret_cast<const int4*>(A.table);
  for (int slice = 0; slice < G; ++slice) {
    for (int e = lane; e < kPerSlice * fp::kHist; e += 64) sums[e] = 0;
    __syncthreads();
    const long long first = base + slice * kPerSlice, i = first + grp;
    bool ok = i < live;
    if (ok) {   // n_i >= 1: a usable normal, an addressable cell and somebody to sum over
      const int n = A.table[fp::kRow * (size_t)i + fp::kHist];
      ok = n >= 1 && n <= fp::kMaxNeighbors;
    }
    const Query q = load_query(A, i, ok, sub, false);
    uint64_t nk[kCells];
    int st[kCells], len[kCells], longest = 0;
    cell_headers<G>(A.S, ok, q.px, q.py, q.pz, q.cx, q.cy, q.cz, q.b, q.c0, q.cn, per_cloud, cell, reach, sub, nk, st,
                    len);
#pragma unroll
    for (int c = 0; c < kCells; ++c) longest = len[c] > longest ? len[c] : longest;
    int64_t acc[fp::kHist];
#pragma unroll
    for (int k = 0; k < fp::kHist; ++k) acc[k] = 0;
    for (int t = 0; t < longest; ++t) {
      uint64_t kk[kCells];
      float4 sp[kCells];
#pragma unroll
      for (int c = 0; c < kCells; ++c) {
        const int pos = t < len[c] ? st[c] + t : 0;
        kk[c] = A.S.key[pos];
        sp[c] = A.S.pts[pos];
      }
#pragma unroll
      for (int c = 0; c < kCells; ++c) {
        const float d2f = d3f::sqdist_exact(q.px, q.py, q.pz, sp[c].x, sp[c].y, sp[c].z);
        const double dx = (double)sp[c].x - (double)q.px, dy = (double)sp[c].y - (double)q.py,
                     dz = (double)sp[c].z - (double)q.pz;
        const double d2 = fp::sqdist_f64(dx, dy, dz);
        if (t < len[c] && kk[c] == nk[c] && d2f < A.S.r2 && d2 != 0.0) {
          const size_t j = (size_t)(uint32_t)__float_as_int(sp[c].w);
          int4 r[fp::kRow / 4];
#pragma unroll
          for (int k = 0; k < fp::kRow / 4; ++k) r[k] = rows[(fp::kRow / 4) * j + k];
          const int n_j = r[8].y;
          if (n_j >= 1) {   // (0: an unusable normal)
            const int64_t W = fp::neighbor_weight(A.r2, d2, n_j);
#pragma unroll
            for (int k = 0; k < fp::kHist / 4; ++k) {
              acc[4 * k + 0] += W * r[k].x;
              acc[4 * k + 1] += W * r[k].y;
              acc[4 * k + 2] += W * r[k].z;
              acc[4 * k + 3] += W * r[k].w;
            }
            acc[32] += W * r[8].x;
          }
        }
      }
    }
    if (ok) {
#pragma unroll
      for (int k = 0; k < fp::kHist; ++k) atomicAdd(&sums[grp * fp::kHist + k], (unsigned long long)acc[k]);
    }
    __syncthreads();
    for (int e = lane; e < kPerSlice * fp::kHist; e += 64) {
      const int r = e / fp::kHist, col = e % fp::kHist;
      const long long row = first + r;
      float v = 0.0f;
      if (row < A.Ns) {
        const int n = A.table[fp::kRow * (size_t)row + fp::kHist];
        if (n >= 1 && n <= fp::kMaxNeighbors) {
          const int h = col / fp::kBins;
          int64_t tot = 0;
          for (int k = 0; k < fp::kBins; ++k) tot += (int64_t)sums[r * fp::kHist + h * fp::kBins + k];
          v = fp::descriptor_entry((int64_t)sums[e], tot, A.table[fp::kRow * (size_t)row + col], n);
        }
      }
      entries[e] = v;
    }
    __syncthreads();
    const int W = A.row_width;
    for (int e = lane; e < kPerSlice * W; e += 64) {   // the slice's 8 rows are one contiguous run
      const int r = e / W, col = e % W;
      const long long row = first + r;
      if (row >= A.Ns) continue;
      float v = col < fp::kHist ? entries[r * fp::kHist + col] : 0.0f;
      if (A.unit && v != 0.0f) {
        double q = 0.0;
        for (int k = 0; k < fp::kHist; ++k) q += (double)entries[r * fp::kHist + k] * (double)entries[r * fp::kHist + k];
        v = fp::unit_entry(v, q);
      }
      A.desc[(size_t)W * (size_t)row + col] = v;
    }
    __syncthreads();
  }
}

bool width_ok(int row_width) { return row_width == fp::kHist || row_width == 64; }

float sqdist_f32(float ax, float ay, float az, float bx, float by, float bz) {   // d3f::sqdist_exact on the host
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return (dx * dx + dy * dy) + dz * dz;   // (-ffp-contract=off: no FMA)
}

}  // namespace

extern "C" {

size_t d3f_fpfh_ws_bytes(int Ns) {
  return d3f::align_up((size_t)(Ns > 0 ? Ns : 1) * fp::kRow * sizeof(int32_t), 256);
}

int d3f_fpfh_passes(const void* grid_ws, const float* points, const float* normals, int Ns, const int32_t* cloud_start,
                    int B, float grid_radius, float radius, int row_width, int unit, float* desc, int32_t* count,
                    int32_t* spfh, int32_t* status, void* ws, size_t ws_bytes, int passes, void* stream_) {
  if (passes < 1 || passes > 3 || !grid_ws || !points || !normals || !cloud_start || !status || Ns < 0 || B < 1 ||
      B > kMaxClouds ||
      !(radius > 0.0f) || !isfinite(radius) || !(grid_radius >= radius) || !width_ok(row_width) ||
      (Ns > 0 && (!desc || !count || !ws)) || ((uintptr_t)ws & 15))
    return D3F_EINVAL;
  if (Ns == 0) return D3F_OK;
  if (ws_bytes < d3f_fpfh_ws_bytes(Ns)) return D3F_EWORKSPACE;
  FpfhArgs a;
  a.points = points;
  a.nrm = normals;
  a.cloud_start = cloud_start;
  a.S = cell_search(grid_ws, Ns, grid_radius, radius, &a.placement);
  a.table = static_cast<int32_t*>(ws);
  a.count = count;
  a.spfh = spfh;
  a.desc = desc;
  a.status = status;
  a.r2 = (double)radius * (double)radius;
  a.B = B;
  a.Ns = Ns;
  a.row_width = row_width;
  a.unit = unit != 0;
  const unsigned blocks = (unsigned)d3f::cdiv(Ns, kBlock);
  if (passes & 1) {
    spfh_kernel<kG><<<blocks, kBlock, 0, (hipStream_t)stream_>>>(a);
    D3F_LAUNCH_CHECK();
  }
  if (passes & 2) {
    fpfh_kernel<kG><<<blocks, kBlock, 0, (hipStream_t)stream_>>>(a);
    D3F_LAUNCH_CHECK();
  }
  return D3F_OK;
}

int d3f_fpfh(const void* grid_ws, const float* points, const float* normals, int Ns, const int32_t* cloud_start, int B,
             float grid_radius, float radius, int row_width, int unit, float* desc, int32_t* count, int32_t* spfh,
             int32_t* status, void* ws, size_t ws_bytes, void* stream_) {
  return d3f_fpfh_passes(grid_ws, points, normals, Ns, cloud_start, B, grid_radius, radius, row_width, unit, desc, count,
                         spfh, status, ws, ws_bytes, 3, stream_);
}

int d3f_fpfh_host(const float* points, const float* normals, int Ns, const int32_t* cloud_start, int B, float radius,
                  int row_width, int unit, float* desc, int32_t* count, int32_t* spfh) {
  if (!points || !normals || !cloud_start || Ns < 0 || B < 1 || B > kMaxClouds || !(radius > 0.0f) ||
      !isfinite(radius) || !width_ok(row_width) || (Ns > 0 && (!desc || !count)))
    return D3F_EINVAL;
  for (int b = 0; b < B; ++b)
    if (cloud_start[b] < 0 || cloud_start[b + 1] < cloud_start[b] || cloud_start[b + 1] > Ns) return D3F_EINVAL;
  const float r2f = radius * radius;
  const double r2 = (double)radius * (double)radius;
  int32_t* table = new int32_t[(size_t)(Ns > 0 ? Ns : 1) * fp::kRow]();
  for (size_t k = 0; k < (size_t)Ns * row_width; ++k) desc[k] = 0.0f;
  for (int i = 0; i < Ns; ++i) count[i] = 0;
  auto usable = [&](int i) { return fp::usable_normal(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]); };
  // f64 d2 of an accepted pair, 0 for a pair that is not one
  auto accepted = [&](int i, int j, double& dx, double& dy, double& dz) -> double {
    const float* p = points + 3 * (size_t)i;
    const float* s = points + 3 * (size_t)j;
    if (!(sqdist_f32(p[0], p[1], p[2], s[0], s[1], s[2]) < r2f) || !usable(j)) return 0.0;
    dx = (double)s[0] - (double)p[0];
    dy = (double)s[1] - (double)p[1];
    dz = (double)s[2] - (double)p[2];
    return fp::sqdist_f64(dx, dy, dz);
  };
  for (int b = 0; b < B; ++b) {
    const int c0 = cloud_start[b], c1 = cloud_start[b + 1];
    for (int i = c0; i < c1; ++i) {
      if (!usable(i)) continue;
      int32_t* row = table + fp::kRow * (size_t)i;
      for (int j = c0; j < c1; ++j) {
        double dx, dy, dz;
        const double d2 = accepted(i, j, dx, dy, dz);
        if (d2 == 0.0) continue;
        int bt, b2, b3;
        fp::pair_bins(dx, dy, dz, d2, (double)normals[3 * i], (double)normals[3 * i + 1], (double)normals[3 * i + 2],
                      (double)normals[3 * j], (double)normals[3 * j + 1], (double)normals[3 * j + 2], bt, b2, b3);
        row[bt] += 1;
        row[fp::kBins + b2] += 1;
        row[2 * fp::kBins + b3] += 1;
        row[fp::kHist] += 1;
      }
      count[i] = row[fp::kHist];
    }
    for (int i = c0; i < c1; ++i) {
      const int32_t* row = table + fp::kRow * (size_t)i;
      const int n = row[fp::kHist];
      if (n < 1 || n > fp::kMaxNeighbors) continue;
      int64_t S[fp::kHist] = {0};
      for (int j = c0; j < c1; ++j) {
        double dx, dy, dz;
        const double d2 = accepted(i, j, dx, dy, dz);
        if (d2 == 0.0) continue;
        const int32_t* other = table + fp::kRow * (size_t)j;
        const int64_t W = fp::neighbor_weight(r2, d2, other[fp::kHist]);
        for (int k = 0; k < fp::kHist; ++k) S[k] += W * other[k];
      }
      float* out = desc + (size_t)row_width * i;
      for (int h = 0; h < 3; ++h) {
        int64_t tot = 0;
        for (int k = 0; k < fp::kBins; ++k) tot += S[h * fp::kBins + k];
        for (int k = 0; k < fp::kBins; ++k) {
          const int col = h * fp::kBins + k;
          out[col] = fp::descriptor_entry(S[col], tot, row[col], n);
        }
      }
      if (unit) {
        double q = 0.0;
        for (int k = 0; k < fp::kHist; ++k) q += (double)out[k] * (double)out[k];
        for (int k = 0; k < fp::kHist; ++k)
          if (out[k] != 0.0f) out[k] = fp::unit_entry(out[k], q);
      }
    }
  }
  if (spfh)
    for (int i = 0; i < Ns; ++i)
      for (int k = 0; k < fp::kHist; ++k) spfh[fp::kHist * (size_t)i + k] = table[fp::kRow * (size_t)i + k];
  delete[] table;
  return D3F_OK;
}

}  // extern "C"
