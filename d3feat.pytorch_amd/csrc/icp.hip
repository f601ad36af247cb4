// Batched point-to-point ICP over a LIST of cloud pairs of one cell list -- the refinement after RANSAC
// (geometric_registration/registration.py; the reference leaves it to Open3D on the CPU).  All P pairs advance together,
// without host synchronisation and with a launch sequence that does not depend on the data: one setup launch, then per
// iteration a search launch and a fit launch.
//
// CONVENTION (easy to get backwards).  Pair p = (MOVING cloud a, FIXED cloud b) and T_p maps points of a into b's frame
// -- exactly the (source, target, transform) of d3f_nearest_pairs.  For a gt.log key i_j, whose matrix maps fragment j
// into fragment i (what d3f_ransac_rigid returns: "target onto source"), the moving cloud is j and the fixed cloud is i:
// a RANSAC result is a valid T_init as it stands with pairs = (j, i).
//
// The search of iteration k is nearest_pairs.hip's, word for word (pair_search.hpp: one statement of q, d2, the
// acceptance and the tie rule serves both kernels).  That kernel is bound by the cache lines it asks the L2 for, not by
// its lanes, so the sums the fit needs ride in the same pass: the lane whose candidate wins its group's minimum still
// holds that candidate's coordinates and adds, in f64, n, sum x', sum y', sum x' y'^T and sum d2 to its own 17
// accumulators (x' = x - px, y' = y - py; the pivots px, py are row 0 of the moving / fixed cloud -- nothing promises
// clouds near the origin, and the raw second moment of clouds at (300, -200, 50) costs 1e-8 in t).  No index is written.
//
// Determinism and batch independence.  There is no floating-point atomic.  A workgroup serves kRows consecutive rows of
// ONE pair (block blk belongs to the pair p with first(p) <= blk < first(p + 1), first(p) = row_start[p] / kRows + p:
// a prefix that needs no scan and leaves every pair at least the cdiv(len, kRows) blocks it needs); a lane adds its rows
// in slice order, the wave is reduced by a fixed butterfly (DPP / permlane swaps, common.hpp), the 8 waves in wave order
// through LDS, and the pair's workgroups are added by one wave in the order lane = block mod 64, blocks ascending, then
// the same butterfly.  Every order depends on the pair's length alone, so a pair's sums -- and with them its whole
// trajectory -- are bit-identical alone, inside any batch, and from run to run.
//
// Point-to-plane form (d3f_icp_rigid_plane; kernels instantiated with kPlane).  Same setup, search, prefix, reduction
// orders and stopping rule; only what the winning lane adds and what the fit solves differ.  The lane reads the normal
// of the matched fixed point through the index the stored point carries and adds the 21 + 6 entries of the 6x6 normal
// equations of the linearised point-to-plane residual (plane.hpp), 29 sums with n and sum d2; the fit is a Cholesky
// solve by one lane.  Point-to-point ICP removes the error ALONG a plane only slowly; this form does not penalise it.
//
// Information matrices (d3f_pair_information; the search kernel instantiated with kInfo).  The 6x6 information matrix
// of a pair -- what gt.info holds and what a pose graph takes per edge -- is a handful of sums over exactly the accepted
// rows of ONE search under a given T, so it is a third kind of the same kernel: the winning lane adds n, sum x,
// sum x x^T (upper triangle) of the moving point, the same of the matched fixed point y, and sum d2: 20 RAW moments, no
// pivots (a product of two f32 values is exact in f64 and nothing is subtracted afterwards, so there is no cancellation
// to protect).  Setup, prefix, reduction orders and flags are ICP's (the same code: icp_setup_kernel, pair_sums); a
// finishing launch adds the pair's block sums and writes them.  Three launches whatever the data.
//
// Coloured form (d3f_icp_rigid_color; kernels instantiated with kColor; color_icp.hpp has the rule).  Point-to-plane's
// winner branch with J and r scaled by sqrt(lambda_geometric), plus a second rank-1 update with the colour row
// J_C = sc [a x d, d], r_C = sc ((I_y - I_x) + (a - c) . d) when the matched fixed point's field (d, I_y: one 16-byte
// read through the same index) and the moving row's intensity are finite.  31 sums: the 29, n_color and the unweighted
// sum of squared colour residuals; the fit is kPlane's on the first 29 and reports n_color and color_rmse at the stop.
#include "color_icp.hpp"
#include "pair_search.hpp"
#include "plane.hpp"
#include "rigid.hpp"

namespace {

using namespace d3f::cells;

constexpr int kBlock = 512;
constexpr int kG = 8;                                // lanes per query, nearest_pairs.hip's default
constexpr int kRows = D3F_ICP_BLOCK_ROWS;            // rows per workgroup
constexpr int kRowsPerSlice = (kBlock / 64) * (64 / kG);
constexpr int kSlices = kRows / kRowsPerSlice;
constexpr int kPoint = 0, kPlane = 1;   // what the fit minimises
constexpr int kInfo = 2;                // no fit: the raw moments of the accepted rows (d3f_pair_information)
constexpr int kColor = 3;               // kPlane's fit over geometric and colour rows (d3f_icp_rigid_color)
constexpr int sums_of(int kind) {
  return kind == kPlane ? d3f::plane::kPlaneSums : kind == kInfo ? D3F_INFO_MOMENTS : kind == kColor ? d3f::color::kColorSums : 17;
}
// where sum d2 sits: the last sum, but for kColor, whose first 29 sums are kPlane's
constexpr int d2_of(int kind) { return kind == kColor ? d3f::plane::kPlaneSums - 1 : sums_of(kind) - 1; }
static_assert(kRows % kRowsPerSlice == 0, "a workgroup serves whole slices");

struct IcpArgs {
  const float* points;
  const float* normals;       // [Ns,3], input row order (kPlane)
  const int32_t* cloud_start;
  const int32_t* pairs;
  const int64_t* row_start;
  const int32_t* placement;   // cell_list.hpp: 0 = one hashed table, 1 = per-cloud tables
  CellSearch S;               // pair_search.hpp
  const double* T_init;       // [P,12]
  double* T_cur;              // [P,12] ws: T_k
  double* prev;               // [P,2]  ws: fitness_{k-1}, rmse_{k-1}
  int32_t* done;              // [P]    ws: the pair has stopped
  double* partial;            // [blocks, sums_of(kind)] ws
  double* T;
  int32_t* count;
  double* rmse;
  int32_t* iterations;
  int32_t* status;
  double* trace;
  double rel_fitness, rel_rmse;
  long long rows;
  int B, P, Ns, max_iters;
  double* moments;            // [P, D3F_INFO_MOMENTS] (kInfo)
  const float4* field;        // [Ns] (d, I), input row order (kColor)
  int32_t* n_color;           // [P] (kColor)
  double* color_rmse;         // [P] (kColor)
  double sg, sc;              // sqrt(lambda_geometric), sqrt(1 - lambda_geometric) (kColor)
};

__device__ __forceinline__ long long first_block(const IcpArgs& A, int p) { return A.row_start[p] / kRows + p; }

// rows of pair p that are searched: its segment of row_start, at most the moving cloud's length (a valid pair only)
__device__ __forceinline__ long long pair_rows(const IcpArgs& A, int p, int a) {
  const long long seg = A.row_start[p + 1] - A.row_start[p], len = A.cloud_start[a + 1] - A.cloud_start[a];
  const long long m = seg < len ? seg : len;
  return m > 0 ? m : 0;
}

__device__ __forceinline__ void write_pose(double* __restrict__ o, const double* __restrict__ rt) {
#pragma unroll
  for (int k = 0; k < 12; ++k) o[k] = rt[k];
  o[12] = 0.0; o[13] = 0.0; o[14] = 0.0; o[15] = 1.0;
}

// kFit: the pair is iterated (kPoint, kPlane); without it (kInfo) the flags, the copy of T and `done` are all there is
template <bool kFit, bool kColorOut = false>
__global__ void icp_setup_kernel(const IcpArgs A) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (A.trace) {
    const long long n = 2ll * A.P * (A.max_iters + 1);
    for (long long k = i; k < n; k += (long long)gridDim.x * blockDim.x) A.trace[k] = __longlong_as_double(0x7ff8000000000000ll);
  }
  if (i >= A.P) return;
  const int p = (int)i;
  const int a = A.pairs[2 * p], b = A.pairs[2 * p + 1];
  int st = 0;
  if (!((unsigned)a < (unsigned)A.B && (unsigned)b < (unsigned)A.B) || A.row_start[p] < 0 ||
      A.row_start[p + 1] < A.row_start[p] || A.row_start[p + 1] > A.rows)
    st |= D3F_ICP_ST_PAIR;
  bool finite = true;
  for (int k = 0; k < 12; ++k) {
    const double v = A.T_init[12 * (size_t)p + k];
    A.T_cur[12 * (size_t)p + k] = v;
    finite = finite && isfinite(v);
  }
  if (!finite) st |= D3F_ICP_ST_NONFINITE;
  A.done[p] = st != 0;   // never searched
  A.status[p] = st;
  if constexpr (kFit) {
    A.prev[2 * p] = 0.0;
    A.prev[2 * p + 1] = 0.0;
    A.iterations[p] = 0;
    if (st) {   // the result is T_init (kInfo: zero moments, written by the finishing launch)
      write_pose(A.T + 16 * (size_t)p, A.T_init + 12 * (size_t)p);
      A.count[p] = 0;
      A.rmse[p] = 0.0;
      if constexpr (kColorOut) {
        A.n_color[p] = 0;
        A.color_rmse[p] = 0.0;
      }
    }
  }
}

// Pair p's block sums in the fixed order of the header: lane = block mod 64, blocks ascending, then the butterfly.  One
// wave; a = the pair's moving cloud.
template <int kSums>
__device__ __forceinline__ void pair_sums(const IcpArgs& A, int p, int a, int lane, double (&v)[kSums]) {
  const long long m = pair_rows(A, p, a), nblk = (m + kRows - 1) / kRows, first = first_block(A, p);
#pragma unroll
  for (int k = 0; k < kSums; ++k) v[k] = 0.0;
  for (long long j = lane; j < nblk; j += 64) {
    const double* part = A.partial + (size_t)(first + j) * kSums;
#pragma unroll
    for (int k = 0; k < kSums; ++k) v[k] += part[k];
  }
  d3f::wave_sum_f64(v);
}

template <int kKind>
__global__ __launch_bounds__(kBlock) void icp_search_kernel(const IcpArgs A) {
  constexpr int kSums = sums_of(kKind);
  const int lane = threadIdx.x & 63, sub = lane & (kG - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // the pair of this workgroup: the largest p with first_block(p) <= blockIdx.x (first_block(0) = 0)
  const long long blk = blockIdx.x;
  int p = 0, hi = A.P;
  while (hi - p > 1) {
    const int mid = p + ((hi - p) >> 1);
    if (first_block(A, mid) <= blk) p = mid; else hi = mid;
  }
  if (A.done[p]) return;   // (everything up to the barrier below is uniform over the workgroup)
  const int a = A.pairs[2 * p], b = A.pairs[2 * p + 1];   // in [0, B): the setup launch stopped the others
  const long long m = pair_rows(A, p, a), row0 = (blk - first_block(A, p)) * kRows;
  if (row0 < 0 || row0 >= m) return;   // a block of the prefix's slack
  const int sa = A.cloud_start[a], tgt0 = A.cloud_start[b], tgt_n = A.cloud_start[b + 1] - tgt0;
  const bool per_cloud = *A.placement != 0;
  const double cell = 1.0 / A.S.inv_cell, reach = (double)A.S.prune_r * (1.0 + 1e-4);
  const double* T = A.T_cur + 12 * (size_t)p;
  const bool pivots = tgt_n > 0 && (long long)sa < (long long)A.Ns && (long long)tgt0 < (long long)A.Ns;
  double px[3] = {0.0, 0.0, 0.0}, py[3] = {0.0, 0.0, 0.0};
  if (kKind != kInfo && pivots) {   // (kInfo adds raw moments: `pivots` only says that both clouds have a row 0)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      px[k] = (double)A.points[3 * (size_t)sa + k];
      py[k] = (double)A.points[3 * (size_t)tgt0 + k];
    }
  }

  double acc[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
  for (int it = 0; it < kSlices; ++it) {
    const long long i = row0 + it * kRowsPerSlice + wave * (64 / kG) + lane / kG;
    bool ok = pivots && i < m && sa + i < (long long)A.Ns;
    double x = 0.0, y = 0.0, z = 0.0;
    if (ok) {
      const size_t src = (size_t)(sa + i);
      x = (double)A.points[3 * src + 0];
      y = (double)A.points[3 * src + 1];
      z = (double)A.points[3 * src + 2];
    }
    uint64_t mine;
    float4 win;
    const uint64_t best =
        nearest_in_cloud<kG>(A.S, ok, x, y, z, T, b, tgt0, tgt_n, per_cloud, cell, reach, sub, A.status + p, mine, win);
    const bool winner = ok && best != ~0ull && mine == best;   // the one lane of the group that holds the winner
    if constexpr (kKind == kPlane || kKind == kColor) {
      if (winner) {
        // a = T_k x - py in f64 (NOT the f32-rounded query: at coordinates of 300 that rounding is 3e-5 of residual
        // noise), c = y - py, nrm the matched point's normal; J = [a x nrm, nrm], r = (a - c) . nrm
        const size_t w = (size_t)(uint32_t)__float_as_int(win.w);
        const double nrm[3] = {(double)A.normals[3 * w + 0], (double)A.normals[3 * w + 1], (double)A.normals[3 * w + 2]};
        const double a[3] = {(((T[0] * x + T[1] * y) + T[2] * z) + T[3]) - py[0],
                             (((T[4] * x + T[5] * y) + T[6] * z) + T[7]) - py[1],
                             (((T[8] * x + T[9] * y) + T[10] * z) + T[11]) - py[2]};
        const double c[3] = {(double)win.x - py[0], (double)win.y - py[1], (double)win.z - py[2]};
        double J[6] = {a[1] * nrm[2] - a[2] * nrm[1], a[2] * nrm[0] - a[0] * nrm[2], a[0] * nrm[1] - a[1] * nrm[0],
                       nrm[0], nrm[1], nrm[2]};
        double r = ((a[0] - c[0]) * nrm[0] + (a[1] - c[1]) * nrm[1]) + (a[2] - c[2]) * nrm[2];
        if constexpr (kKind == kColor) {   // scaled before any product is formed (sg = 1 changes no bit)
#pragma unroll
          for (int i = 0; i < 6; ++i) J[i] *= A.sg;
          r *= A.sg;
        }
        acc[0] += 1.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
#pragma unroll
          for (int j = i; j < 6; ++j) acc[1 + d3f::plane::upper6(i, j)] += J[i] * J[j];
          acc[22 + i] += J[i] * r;
        }
        acc[d2_of(kKind)] += (double)__uint_as_float((uint32_t)(best >> 32));
        if constexpr (kKind == kColor) {
          // the colour row: the matched fixed point's (d, I_y) and the moving row's I_x (its stacked row is sa + i)
          const float4 f = A.field[w];
          const float ix = A.field[(size_t)(sa + i)].w;
          if (isfinite(f.x) && isfinite(f.y) && isfinite(f.z) && isfinite(f.w) && isfinite(ix)) {
            const double d[3] = {(double)f.x, (double)f.y, (double)f.z};
            const double rc = ((double)f.w - (double)ix) +
                              (((a[0] - c[0]) * d[0] + (a[1] - c[1]) * d[1]) + (a[2] - c[2]) * d[2]);
            const double Jc[6] = {A.sc * (a[1] * d[2] - a[2] * d[1]), A.sc * (a[2] * d[0] - a[0] * d[2]),
                                  A.sc * (a[0] * d[1] - a[1] * d[0]), A.sc * d[0], A.sc * d[1], A.sc * d[2]};
            const double rs = A.sc * rc;
#pragma unroll
            for (int i2 = 0; i2 < 6; ++i2) {
#pragma unroll
              for (int j = i2; j < 6; ++j) acc[1 + d3f::plane::upper6(i2, j)] += Jc[i2] * Jc[j];
              acc[22 + i2] += Jc[i2] * rs;
            }
            acc[d3f::plane::kPlaneSums] += 1.0;
            acc[d3f::plane::kPlaneSums + 1] += rc * rc;
          }
        }
      }
    } else if constexpr (kKind == kInfo) {
      if (winner) {
        const double xs[3] = {x, y, z}, ys[3] = {(double)win.x, (double)win.y, (double)win.z};
        acc[0] += 1.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          acc[1 + r] += xs[r];
          acc[10 + r] += ys[r];
#pragma unroll
          for (int c = r; c < 3; ++c) {   // upper triangle row by row: xx, xy, xz, yy, yz, zz
            acc[4 + (r * (7 - r)) / 2 + (c - r)] += xs[r] * xs[c];
            acc[13 + (r * (7 - r)) / 2 + (c - r)] += ys[r] * ys[c];
          }
        }
        acc[d2_of(kKind)] += (double)__uint_as_float((uint32_t)(best >> 32));
      }
    } else if (winner) {
      const double xd[3] = {x - px[0], y - px[1], z - px[2]};
      const double yd[3] = {(double)win.x - py[0], (double)win.y - py[1], (double)win.z - py[2]};
      acc[0] += 1.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        acc[1 + k] += xd[k];
        acc[4 + k] += yd[k];
      }
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[7 + 3 * r + c] += xd[r] * yd[c];
      acc[d2_of(kKind)] += (double)__uint_as_float((uint32_t)(best >> 32));
    }
  }
  d3f::wave_sum_f64(acc);
  __shared__ double red[kBlock / 64][kSums];
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kSums; ++k) red[wave][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < kSums) {
    double s = red[0][threadIdx.x];
    for (int w = 1; w < kBlock / 64; ++w) s += red[w][threadIdx.x];
    A.partial[(size_t)blk * kSums + threadIdx.x] = s;
  }
}

// n_color and color_rmse of the pose a coloured pair stops at
__device__ __forceinline__ void write_color(const IcpArgs& A, int p, const double (&v)[d3f::color::kColorSums]) {
  const double nc = v[d3f::plane::kPlaneSums];
  A.n_color[p] = (int)nc;
  A.color_rmse[p] = nc > 0.0 ? sqrt(v[d3f::plane::kPlaneSums + 1] / nc) : 0.0;
}

// one wave per pair: the pair's block sums in a fixed order, the stopping rule, the fit
template <int kKind>
__global__ __launch_bounds__(64) void icp_fit_kernel(const IcpArgs A, int k_iter) {
  constexpr int kSums = sums_of(kKind);
  const int p = blockIdx.x, lane = threadIdx.x;
  if (A.done[p]) return;
  const int a = A.pairs[2 * p], b = A.pairs[2 * p + 1];
  double v[kSums];
  pair_sums(A, p, a, lane, v);
  if (lane != 0) return;
  const int sa = A.cloud_start[a], len_a = A.cloud_start[a + 1] - sa, tgt0 = A.cloud_start[b];
  const double n = v[0], sd2 = v[d2_of(kKind)];
  const double fitness = len_a > 0 ? n / (double)len_a : 0.0, rmse = n > 0.0 ? sqrt(sd2 / n) : 0.0;
  if (A.trace) {
    double* tr = A.trace + 2 * ((size_t)p * (A.max_iters + 1) + k_iter);
    tr[0] = n;
    tr[1] = sd2;
  }
  double* T = A.T_cur + 12 * (size_t)p;
  bool stop = false;
  if (n < 3.0) {
    atomicOr(A.status + p, D3F_ICP_ST_FEW);
    stop = true;
  } else if (k_iter >= 1 && fabs(fitness - A.prev[2 * p]) < A.rel_fitness && fabs(rmse - A.prev[2 * p + 1]) < A.rel_rmse) {
    stop = true;
  } else if (k_iter >= A.max_iters) {
    stop = true;
  }
  if (stop) {
    write_pose(A.T + 16 * (size_t)p, T);
    A.count[p] = (int)n;
    A.rmse[p] = rmse;
    if constexpr (kKind == kColor) write_color(A, p, v);
    A.done[p] = 1;
    return;
  }
  double px[3], py[3];   // (n >= 3: both clouds have a row 0 inside the stack, the search read it)
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    px[k] = (double)A.points[3 * (size_t)sa + k];
    py[k] = (double)A.points[3 * (size_t)tgt0 + k];
  }
  if constexpr (kKind == kPlane || kKind == kColor) {
    double Tk[12], Tn[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) Tk[k] = T[k];
    if (!d3f::plane::plane_step(v, py, Tk, Tn)) {   // the free slide of a single plane, or an overlap of zero normals
      atomicOr(A.status + p, D3F_ICP_ST_SINGULAR);
      write_pose(A.T + 16 * (size_t)p, T);
      A.count[p] = (int)n;
      A.rmse[p] = rmse;
      if constexpr (kKind == kColor) write_color(A, p, v);
      A.done[p] = 1;
      return;
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = Tn[k];
  } else {
    double R[9], t[3];
    d3f::rigid::fit_from_sums(v, px, py, R, t);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      T[4 * r] = R[3 * r];
      T[4 * r + 1] = R[3 * r + 1];
      T[4 * r + 2] = R[3 * r + 2];
      T[4 * r + 3] = t[r];
    }
  }
  A.prev[2 * p] = fitness;
  A.prev[2 * p + 1] = rmse;
  A.iterations[p] = k_iter + 1;
}

// one wave per pair: the pair's block sums, written as they are (zeros for a pair the setup launch stopped)
__global__ __launch_bounds__(64) void info_finish_kernel(const IcpArgs A) {
  constexpr int kSums = sums_of(kInfo);
  const int p = blockIdx.x, lane = threadIdx.x;
  double v[kSums] = {};
  if (!A.done[p]) pair_sums(A, p, A.pairs[2 * p], lane, v);   // (uniform over the wave)
  if (lane != 0) return;
#pragma unroll
  for (int k = 0; k < kSums; ++k) A.moments[(size_t)p * kSums + k] = v[k];
  A.count[p] = (int)v[0];
}

struct IcpLayout {
  double* T_cur;
  double* prev;
  int32_t* done;
  double* partial;
  long long blocks;
  size_t bytes;
};

IcpLayout icp_layout(void* ws, int P, long long rows, int kind) {
  IcpLayout l;
  const size_t n = (size_t)(P > 0 ? P : 1);
  l.blocks = (rows > 0 ? rows : 0) / kRows + (long long)n + 1;
  d3f::Carver c(ws);
  l.T_cur = c.take<double>(12 * n);
  l.prev = c.take<double>(2 * n);
  l.done = c.take<int32_t>(n);
  l.partial = c.take<double>((size_t)l.blocks * sums_of(kind));
  l.bytes = d3f::align_up(c.off, 256);
  return l;
}

// What the three kinds share on the host: the checks of the common arguments and the common part of IcpArgs.  D3F_OK
// with P == 0 means there is nothing to launch.
int icp_prepare(int kind, const void* grid_ws, const float* points, int Ns, const int32_t* cloud_start, int B,
                float grid_radius, float max_distance, const int32_t* pairs, const int64_t* row_start, int P,
                int64_t rows, const double* T_init, int32_t* count, int32_t* status, void* ws, size_t ws_bytes,
                IcpArgs& a, long long& blocks) {
  if (!grid_ws || !points || !cloud_start || !row_start || Ns < 0 || B < 1 || B > kMaxClouds || P < 0 || P > 65535 ||
      rows < 0 || rows > 0x7fffffffll || !(max_distance > 0.0f) || !(grid_radius >= max_distance) ||
      (P > 0 && (!pairs || !T_init || !count || !status || !ws)))
    return D3F_EINVAL;
  if (P == 0) return D3F_OK;
  if (ws_bytes < icp_layout(nullptr, P, rows, kind).bytes) return D3F_EWORKSPACE;
  const IcpLayout l = icp_layout(ws, P, rows, kind);
  a.points = points;
  a.cloud_start = cloud_start;
  a.pairs = pairs;
  a.row_start = row_start;
  a.S = cell_search(grid_ws, Ns, grid_radius, max_distance, &a.placement);
  a.T_init = T_init;
  a.T_cur = l.T_cur;
  a.prev = l.prev;
  a.done = l.done;
  a.partial = l.partial;
  a.count = count;
  a.status = status;
  a.rows = rows;
  a.B = B;
  a.P = P;
  a.Ns = Ns;
  blocks = l.blocks;
  return D3F_OK;
}

template <int kKind>
int icp_run(const void* grid_ws, const float* points, const float* normals, const float* field,
            double lambda_geometric, int32_t* n_color, double* color_rmse, int Ns, const int32_t* cloud_start, int B,
            float grid_radius, float max_distance, const int32_t* pairs, const int64_t* row_start, int P, int64_t rows,
            const double* T_init, int max_iters, double rel_fitness, double rel_rmse, double* T, int32_t* count,
            double* rmse, int32_t* iterations, int32_t* status, double* trace, void* ws, size_t ws_bytes,
            void* stream_) {
  if (max_iters < 0 || max_iters > D3F_ICP_MAX_ITERS || !(rel_fitness >= 0.0) || !(rel_rmse >= 0.0) ||
      (P > 0 && (!T || !rmse || !iterations)))
    return D3F_EINVAL;
  if (kKind == kColor && (!(lambda_geometric >= 0.0 && lambda_geometric <= 1.0) || (P > 0 && (!n_color || !color_rmse))))
    return D3F_EINVAL;
  IcpArgs a = {};
  long long blocks = 0;
  const int rc = icp_prepare(kKind, grid_ws, points, Ns, cloud_start, B, grid_radius, max_distance, pairs, row_start, P,
                             rows, T_init, count, status, ws, ws_bytes, a, blocks);
  if (rc != D3F_OK || P == 0) return rc;
  a.normals = normals;
  a.field = reinterpret_cast<const float4*>(field);
  a.n_color = n_color;
  a.color_rmse = color_rmse;
  a.sg = sqrt(lambda_geometric);
  a.sc = sqrt(1.0 - lambda_geometric);
  a.T = T;
  a.rmse = rmse;
  a.iterations = iterations;
  a.trace = trace;
  a.rel_fitness = rel_fitness;
  a.rel_rmse = rel_rmse;
  a.max_iters = max_iters;
  hipStream_t stream = (hipStream_t)stream_;
  const long long fill = trace ? 2ll * P * (max_iters + 1) : P;
  long long setup_blocks = ((fill > P ? fill : P) + 255) / 256;
  if (setup_blocks > 4096) setup_blocks = 4096;
  if (setup_blocks < (P + 255) / 256) setup_blocks = (P + 255) / 256;
  icp_setup_kernel<true, kKind == kColor><<<(unsigned)setup_blocks, 256, 0, stream>>>(a);
  D3F_LAUNCH_CHECK();
  for (int k = 0; k <= max_iters; ++k) {
    icp_search_kernel<kKind><<<(unsigned)blocks, kBlock, 0, stream>>>(a);
    icp_fit_kernel<kKind><<<(unsigned)P, 64, 0, stream>>>(a, k);
  }
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int info_run(const void* grid_ws, const float* points, int Ns, const int32_t* cloud_start, int B, float grid_radius,
             float max_distance, const int32_t* pairs, const int64_t* row_start, int P, int64_t rows, const double* T,
             double* moments, int32_t* count, int32_t* status, void* ws, size_t ws_bytes, void* stream_) {
  if (P > 0 && !moments) return D3F_EINVAL;
  IcpArgs a = {};
  long long blocks = 0;
  const int rc = icp_prepare(kInfo, grid_ws, points, Ns, cloud_start, B, grid_radius, max_distance, pairs, row_start, P,
                             rows, T, count, status, ws, ws_bytes, a, blocks);
  if (rc != D3F_OK || P == 0) return rc;
  a.moments = moments;
  hipStream_t stream = (hipStream_t)stream_;
  icp_setup_kernel<false><<<(unsigned)((P + 255) / 256), 256, 0, stream>>>(a);
  D3F_LAUNCH_CHECK();
  icp_search_kernel<kInfo><<<(unsigned)blocks, kBlock, 0, stream>>>(a);
  info_finish_kernel<<<(unsigned)P, 64, 0, stream>>>(a);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

}  // namespace

extern "C" {

size_t d3f_pair_information_ws_bytes(int P, int64_t rows) { return icp_layout(nullptr, P, rows, kInfo).bytes; }

int d3f_pair_information(const void* grid_ws, const float* points, int Ns, const int32_t* cloud_start, int B,
                         float grid_radius, float max_distance, const int32_t* pairs, const int64_t* row_start, int P,
                         int64_t rows, const double* T, double* moments, int32_t* count, int32_t* status, void* ws,
                         size_t ws_bytes, void* stream_) {
  return info_run(grid_ws, points, Ns, cloud_start, B, grid_radius, max_distance, pairs, row_start, P, rows, T, moments,
                  count, status, ws, ws_bytes, stream_);
}

size_t d3f_icp_rigid_ws_bytes(int P, int64_t rows) { return icp_layout(nullptr, P, rows, kPoint).bytes; }
size_t d3f_icp_rigid_plane_ws_bytes(int P, int64_t rows) { return icp_layout(nullptr, P, rows, kPlane).bytes; }

int d3f_icp_rigid(const void* grid_ws, const float* points, int Ns, const int32_t* cloud_start, int B,
                  float grid_radius, float max_distance, const int32_t* pairs, const int64_t* row_start, int P,
                  int64_t rows, const double* T_init, int max_iters, double rel_fitness, double rel_rmse, double* T,
                  int32_t* count, double* rmse, int32_t* iterations, int32_t* status, double* trace, void* ws,
                  size_t ws_bytes, void* stream_) {
  return icp_run<kPoint>(grid_ws, points, nullptr, nullptr, 1.0, nullptr, nullptr, Ns, cloud_start, B, grid_radius, max_distance, pairs, row_start, P,
                         rows, T_init, max_iters, rel_fitness, rel_rmse, T, count, rmse, iterations, status, trace, ws,
                         ws_bytes, stream_);
}

int d3f_icp_rigid_plane(const void* grid_ws, const float* points, const float* normals, int Ns,
                        const int32_t* cloud_start, int B, float grid_radius, float max_distance, const int32_t* pairs,
                        const int64_t* row_start, int P, int64_t rows, const double* T_init, int max_iters,
                        double rel_fitness, double rel_rmse, double* T, int32_t* count, double* rmse,
                        int32_t* iterations, int32_t* status, double* trace, void* ws, size_t ws_bytes, void* stream_) {
  if (!normals) return D3F_EINVAL;
  return icp_run<kPlane>(grid_ws, points, normals, nullptr, 1.0, nullptr, nullptr, Ns, cloud_start, B, grid_radius, max_distance, pairs, row_start, P,
                         rows, T_init, max_iters, rel_fitness, rel_rmse, T, count, rmse, iterations, status, trace, ws,
                         ws_bytes, stream_);
}

size_t d3f_icp_rigid_color_ws_bytes(int P, int64_t rows) { return icp_layout(nullptr, P, rows, kColor).bytes; }

int d3f_icp_rigid_color(const void* grid_ws, const float* points, const float* normals, const float* field, int Ns,
                        const int32_t* cloud_start, int B, float grid_radius, float max_distance, const int32_t* pairs,
                        const int64_t* row_start, int P, int64_t rows, const double* T_init, double lambda_geometric,
                        int max_iters, double rel_fitness, double rel_rmse, double* T, int32_t* count, double* rmse,
                        int32_t* iterations, int32_t* status, int32_t* n_color, double* color_rmse, double* trace,
                        void* ws, size_t ws_bytes, void* stream_) {
  if (!normals || !field) return D3F_EINVAL;
  return icp_run<kColor>(grid_ws, points, normals, field, lambda_geometric, n_color, color_rmse, Ns, cloud_start, B,
                         grid_radius, max_distance, pairs, row_start, P, rows, T_init, max_iters, rel_fitness, rel_rmse,
                         T, count, rmse, iterations, status, trace, ws, ws_bytes, stream_);
}

int d3f_icp_fit_host(const double* sums_host, const double* px_host, const double* py_host, double* out_host) {
  if (!sums_host || !px_host || !py_host || !out_host || !(sums_host[0] >= 1.0)) return D3F_EINVAL;
  double R[9], t[3];
  d3f::rigid::fit_from_sums(sums_host, px_host, py_host, R, t);
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) out_host[4 * a + b] = R[3 * a + b];
    out_host[4 * a + 3] = t[a];
  }
  out_host[12] = 0.0; out_host[13] = 0.0; out_host[14] = 0.0; out_host[15] = 1.0;
  return D3F_OK;
}

int d3f_icp_plane_fit_host(const double* sums_host, const double* py_host, const double* T_k_host, double* T_next_host,
                           int* singular_host) {
  if (!sums_host || !py_host || !T_k_host || !T_next_host || !singular_host) return D3F_EINVAL;
  *singular_host = d3f::plane::plane_step(sums_host, py_host, T_k_host, T_next_host) ? 0 : 1;
  T_next_host[12] = 0.0; T_next_host[13] = 0.0; T_next_host[14] = 0.0; T_next_host[15] = 1.0;
  return D3F_OK;
}

}  // extern "C"
