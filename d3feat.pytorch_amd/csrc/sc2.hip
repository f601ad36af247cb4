// Batched spatial-compatibility (SC2) pose estimation of P correspondence sets (include/d3feat_hip.h: d3f_sc2_rigid):
// four launches of static shape, no host synchronisation, no atomics, graph-capturable.  The rule is csrc/sc2.hpp; this
// file is its two carriers.  A pair's outputs depend on nothing but its own rows: the same bits alone or in any batch.
//
// 1. matrix_kernel: grid (ceil(max_count / 32), P), 256 threads.  A workgroup owns a strip of 32 rows of the pair's
//    bit matrix; their points sit in LDS as f64.  Wave v takes the words w = v, v + 4, ...: lane l holds column
//    64 w + l in registers and tests it against the strip's rows in turn (the row is an LDS broadcast); __ballot IS the
//    word, lane r keeps row r's and the 32 lanes store them with plain vector stores.  The degrees are the popcounts
//    summed over the same walk (per wave, then over the 4 waves through LDS: integers, order-free).  Every word of the
//    [max_count, W] slice is written, zeros beyond the count: the workspace needs no clearing.
// 2. seeds_kernel: grid P.  The degrees in LDS (<= 32 KB); the rank of a row is the count of rows that beat it.
// 3. hypothesis_kernel: grid (num_seeds, P).  The seed's row in LDS (<= 1 KB); a wave takes one candidate j at a time,
//    reads its row coalesced (<= 2 words per lane), ANDs, popcounts and wave-sums into the LDS array of candidate keys;
//    set_size - 1 rounds of a workgroup maximum pick the set; one thread fits, all count the inliers.  The key
//    ((count + 1) << 32) | ~rank and the f64 (R, t) go to the workspace.
// 4. select_kernel: grid P.  The maximum key, then rigid::refine (RANSAC's refinement).
// d3f_sc2_rigid_host: the same rule on one CPU thread.
#include <algorithm>
#include <vector>

#include "common.hpp"
#include "rigid_refine.hpp"
#include "sc2.hpp"

namespace {

using namespace d3f::sc2;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / D3F_WAVE;
constexpr int kStrip = 32;   // rows of the matrix per workgroup
static_assert(kThreads == d3f::rigid::kRefineThreads, "the refinement's tree is written for this workgroup");
static_assert(kMaxCount == D3F_SC2_MAX_COUNT && kMaxSet == D3F_SC2_MAX_SET && kMaxSeeds == D3F_SC2_MAX_SEEDS, "sc2.hpp");
static_assert(kStFew == D3F_SC2_ST_FEW && kStNoHypothesis == D3F_SC2_ST_NO_HYPOTHESIS && kStSegment == D3F_SC2_ST_SEGMENT,
              "sc2.hpp");

// the workspace: matrix | degrees | seed table | keys | poses, each part aligned to 256 bytes
struct Layout {
  size_t matrix, degree, seeds, keys, poses, total;
};

Layout layout_of(int P, int max_count, int num_seeds) {
  const size_t p = (size_t)(P > 0 ? P : 1), m = (size_t)(max_count > 0 ? max_count : 1), s = (size_t)(num_seeds > 0 ? num_seeds : 1);
  Layout l;
  l.matrix = 0;
  l.degree = l.matrix + d3f::align_up(8 * p * m * (size_t)words_of((int)m), 256);
  l.seeds = l.degree + d3f::align_up(4 * p * m, 256);
  l.keys = l.seeds + d3f::align_up(4 * p * s, 256);
  l.poses = l.keys + d3f::align_up(8 * p * s, 256);
  l.total = l.poses + d3f::align_up(8 * 12 * p * s, 256);
  return l;
}

struct Params {
  const float* src;
  const float* tgt;
  int rows;
  const int32_t* seg;
  int P, max_count, W;
  float tau2;       // the inlier test's, f32
  double compat2;   // compat_threshold^2
  int num_seeds, set_size, refine_iters;
  double* T;
  int32_t *inliers, *best_seed, *best_count, *status;
  int32_t *degree, *seed_rows, *consensus, *hyp_count;   // optional
  float* hyp_rt;                                         // optional
  unsigned long long* matrix;                            // [P, max_count, W]
  int32_t *ws_degree, *ws_seeds;                         // [P, max_count], [P, num_seeds]
  unsigned long long* ws_keys;                           // [P, num_seeds]
  double* ws_poses;                                      // [P, num_seeds, 12]
};

__device__ __forceinline__ int block_sum_i(int* slot, int v) {
  v = d3f::wave_sum_i(v);
  __syncthreads();
  if (d3f::lane_id() == 0) slot[threadIdx.x / D3F_WAVE] = v;
  __syncthreads();
  return (slot[0] + slot[1]) + (slot[2] + slot[3]);
}

__global__ __launch_bounds__(kThreads) void matrix_kernel(Params a) {
  __shared__ double pt[kStrip][6];
  __shared__ int wdeg[kWaves][kStrip];
  const int p = blockIdx.y, row0 = blockIdx.x * kStrip, tid = threadIdx.x;
  const int lane = d3f::lane_id(), wave = tid / D3F_WAVE;
  int off, n;
  pair_segment(a.seg, p, a.rows, a.max_count, off, n);
  if (tid < kStrip * 6) {
    const int r = tid / 6, c = tid % 6, i = row0 + r;
    double v = 0.0;
    if (i < n) v = (double)(c < 3 ? a.src[3 * (size_t)(off + i) + c] : a.tgt[3 * (size_t)(off + i) + (c - 3)]);
    pt[r][c] = v;
  }
  __syncthreads();
  unsigned long long* M = a.matrix + (size_t)p * a.max_count * a.W;
  const int live_rows = min(kStrip, n - row0);   // <= 0: the strip lies beyond the pair's rows
  int deg = 0;                                   // lane r < kStrip: row r's bits in this wave's words
  for (int w = wave; w < a.W; w += kWaves) {
    unsigned long long mine = 0ull;
    if (64 * w < n && live_rows > 0) {           // uniform over the wave
      const int j = 64 * w + lane;
      const bool live = j < n;
      double cs[3] = {0.0, 0.0, 0.0}, cg[3] = {0.0, 0.0, 0.0};
      if (live) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          cs[c] = (double)a.src[3 * (size_t)(off + j) + c];
          cg[c] = (double)a.tgt[3 * (size_t)(off + j) + c];
        }
      }
      for (int r = 0; r < live_rows; ++r) {
        const double A = dist2(pt[r], cs), B = dist2(pt[r] + 3, cg);   // the row: an LDS broadcast
        const unsigned long long word = __ballot(live && j != row0 + r && compatible(A, B, a.compat2));
        if (lane == r) mine = word;
      }
    }
    deg += __popcll(mine);
    if (lane < kStrip && row0 + lane < a.max_count) M[(size_t)(row0 + lane) * a.W + w] = mine;
  }
  if (lane < kStrip) wdeg[wave][lane] = deg;
  __syncthreads();
  if (tid < kStrip && row0 + tid < a.max_count) {
    int d = 0;
#pragma unroll
    for (int v = 0; v < kWaves; ++v) d += wdeg[v][tid];
    a.ws_degree[(size_t)p * a.max_count + row0 + tid] = d;
    if (a.degree && row0 + tid < n) a.degree[off + row0 + tid] = d;
  }
}

__global__ __launch_bounds__(kThreads) void seeds_kernel(Params a) {
  __shared__ int deg[kMaxCount];
  const int p = blockIdx.x, tid = threadIdx.x;
  int off, n;
  pair_segment(a.seg, p, a.rows, a.max_count, off, n);
  for (int i = tid; i < n; i += kThreads) deg[i] = a.ws_degree[(size_t)p * a.max_count + i];
  const int S = min(a.num_seeds, n);
  for (int r = S + tid; r < a.num_seeds; r += kThreads) {
    a.ws_seeds[(size_t)p * a.num_seeds + r] = -1;
    if (a.seed_rows) a.seed_rows[(size_t)p * a.num_seeds + r] = -1;
  }
  __syncthreads();
  for (int i = tid; i < n; i += kThreads) {
    const int di = deg[i];
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += seed_before(deg[j], j, di, i) ? 1 : 0;   // deg[j]: an LDS broadcast
    if (rank < S) {                                                              // the ranks are a permutation
      a.ws_seeds[(size_t)p * a.num_seeds + rank] = i;
      if (a.seed_rows) a.seed_rows[(size_t)p * a.num_seeds + rank] = i;
    }
  }
}

__global__ __launch_bounds__(kThreads, 4) void hypothesis_kernel(Params a) {   // 4 waves per SIMD: what its LDS allows
  __shared__ unsigned long long seedrow[kMaxWords];
  __shared__ uint32_t ckey[kMaxCount];
  __shared__ double ss[3 * kMaxSet], sg[3 * kMaxSet];
  __shared__ int sset[kMaxSet];
  __shared__ uint32_t wtop[kWaves];
  __shared__ int islot[kWaves];
  __shared__ float srt[12];
  const int rank = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
  const int lane = d3f::lane_id(), wave = tid / D3F_WAVE;
  int off, n;
  pair_segment(a.seg, p, a.rows, a.max_count, off, n);
  const size_t slot = (size_t)p * a.num_seeds + rank;
  int32_t* cons = a.consensus ? a.consensus + slot * a.set_size : nullptr;
  const int i = a.ws_seeds[slot];
  if (i < 0) {   // uniform: no seed of this rank
    if (cons)
      for (int k = tid; k < a.set_size; k += kThreads) cons[k] = -1;
    if (a.hyp_rt && tid < 12) a.hyp_rt[12 * slot + tid] = 0.0f;
    if (tid == 0) {
      a.ws_keys[slot] = 0ull;
      if (a.hyp_count) a.hyp_count[slot] = -1;
    }
    return;
  }
  const unsigned long long* M = a.matrix + (size_t)p * a.max_count * a.W;
  if (tid < a.W) seedrow[tid] = M[(size_t)i * a.W + tid];
  for (int j = tid; j < n; j += kThreads) ckey[j] = 0u;
  __syncthreads();
  // s_ij of every candidate: one wave per candidate, the row read coalesced
  const unsigned long long r0 = lane < a.W ? seedrow[lane] : 0ull, r1 = lane + 64 < a.W ? seedrow[lane + 64] : 0ull;
  for (int j = wave; j < n; j += kWaves) {
    if (!((seedrow[j >> 6] >> (j & 63)) & 1ull)) continue;   // uniform over the wave
    const unsigned long long* rj = M + (size_t)j * a.W;
    int c = 0;
    if (lane < a.W) c = __popcll(r0 & rj[lane]);
    if (lane + 64 < a.W) c += __popcll(r1 & rj[lane + 64]);
    c = d3f::wave_sum_i(c);
    if (lane == 0) ckey[j] = candidate_key(c, j);
  }
  __syncthreads();
  // the set: the seed, then set_size - 1 rounds of the largest remaining key
  const int d = a.ws_degree[(size_t)p * a.max_count + i];
  const int m = min(a.set_size - 1, d), cnt = m + 1;
  if (tid == 0) sset[0] = i;
  for (int k = 0; k < m; ++k) {
    uint32_t best = 0u;
    for (int j = tid; j < n; j += kThreads) best = max(best, ckey[j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = max(best, (uint32_t)__shfl_xor((int)best, o, 64));
    if (lane == 0) wtop[wave] = best;
    __syncthreads();
    best = max(max(wtop[0], wtop[1]), max(wtop[2], wtop[3]));
    if (tid == 0) {   // m <= d: a candidate is left, best > 0 (were it not, the seed itself keeps the row in range)
      const int j = best ? candidate_of(best) : i;
      sset[k + 1] = j;
      ckey[j] = 0u;
    }
    __syncthreads();
  }
  __syncthreads();
  if (tid < cnt) {
    const size_t r = 3 * (size_t)(off + sset[tid]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      ss[3 * tid + c] = (double)a.src[r + c];
      sg[3 * tid + c] = (double)a.tgt[r + c];
    }
  }
  if (cons)
    for (int k = tid; k < a.set_size; k += kThreads) cons[k] = k < cnt ? sset[k] : -1;
  __syncthreads();
  const bool valid = d >= 2;
  if (tid == 0) {
    float rt[12];
    if (valid) {
      double R[9], t[3];
      d3f::rigid::fit(ss, sg, cnt, R, t);
      d3f::rigid::to_f32(R, t, rt);
#pragma unroll
      for (int k = 0; k < 9; ++k) a.ws_poses[12 * slot + k] = R[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) a.ws_poses[12 * slot + 9 + k] = t[k];
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k) rt[k] = 0.0f;
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) srt[k] = rt[k];
  }
  __syncthreads();
  float rt[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) rt[k] = srt[k];
  int c = 0;
  if (valid)
    for (int r = tid; r < n; r += kThreads) {
      const size_t q = 3 * (size_t)(off + r);
      c += d3f::rigid::inlier_f32(rt, a.tgt[q], a.tgt[q + 1], a.tgt[q + 2], a.src[q], a.src[q + 1], a.src[q + 2], a.tau2) ? 1 : 0;
    }
  c = block_sum_i(islot, c);
  if (a.hyp_rt && tid < 12) a.hyp_rt[12 * slot + tid] = rt[tid];
  if (tid == 0) {
    a.ws_keys[slot] = valid ? hypothesis_key(c, rank) : 0ull;
    if (a.hyp_count) a.hyp_count[slot] = valid ? c : -1;
  }
}

__global__ __launch_bounds__(kThreads) void select_kernel(Params a) {
  __shared__ double red[kThreads][d3f::rigid::kRed];
  __shared__ unsigned long long wbest[kWaves];
  const int p = blockIdx.x, tid = threadIdx.x;
  int off, n;
  int st = pair_segment(a.seg, p, a.rows, a.max_count, off, n);
  unsigned long long best = 0ull;
  for (int s = tid; s < a.num_seeds; s += kThreads) {
    const unsigned long long k = a.ws_keys[(size_t)p * a.num_seeds + s];
    best = k > best ? k : best;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(best, o, 64);
    best = other > best ? other : best;
  }
  if (d3f::lane_id() == 0) wbest[tid / D3F_WAVE] = best;
  __syncthreads();
  best = wbest[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) best = wbest[w] > best ? wbest[w] : best;
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
  int seed = -1, pre = 0, fin = 0;
  if (st == 0 && best == 0ull) st = kStNoHypothesis;
  if (st == 0) {   // uniform over the workgroup
    const size_t slot = (size_t)p * a.num_seeds + (int)~(uint32_t)(best & 0xffffffffull);
    seed = a.ws_seeds[slot];
    pre = (int)(best >> 32) - 1;
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = a.ws_poses[12 * slot + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = a.ws_poses[12 * slot + 9 + k];
    fin = d3f::rigid::refine(a.src, a.tgt, off, n, a.tau2, a.refine_iters, red, R, t);
  }
  if (tid == 0) {
    double* o = a.T + 16 * (size_t)p;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      o[4 * r] = R[3 * r];
      o[4 * r + 1] = R[3 * r + 1];
      o[4 * r + 2] = R[3 * r + 2];
      o[4 * r + 3] = t[r];
    }
    o[12] = 0.0; o[13] = 0.0; o[14] = 0.0; o[15] = 1.0;
    a.inliers[p] = fin;
    a.best_seed[p] = seed;
    a.best_count[p] = pre;
    a.status[p] = st;
  }
}

// the rule on one CPU thread: pair p; M = the pair's [max_count, W] slice (zeroed by the caller)
void host_pair(const Params& a, int p, unsigned long long* M) {
  int off, n;
  int st = pair_segment(a.seg, p, a.rows, a.max_count, off, n);
  const int W = a.W, S = std::min(a.num_seeds, n);
  std::vector<double> ps(3 * (size_t)n), pg(3 * (size_t)n);
  for (int i = 0; i < 3 * n; ++i) {
    ps[i] = (double)a.src[3 * (size_t)off + i];
    pg[i] = (double)a.tgt[3 * (size_t)off + i];
  }
  std::vector<int> deg((size_t)n, 0);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j)
      if (i != j && compatible(dist2(&ps[3 * i], &ps[3 * j]), dist2(&pg[3 * i], &pg[3 * j]), a.compat2)) {
        M[(size_t)i * W + (j >> 6)] |= 1ull << (j & 63);
        ++deg[i];
      }
  if (a.degree)
    for (int i = 0; i < n; ++i) a.degree[off + i] = deg[i];
  std::vector<int> order((size_t)n);
  for (int i = 0; i < n; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return seed_before(deg[x], x, deg[y], y); });
  unsigned long long best = 0ull;
  double bestR[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, bestt[3] = {0, 0, 0};
  std::vector<uint32_t> keys;
  for (int rank = 0; rank < a.num_seeds; ++rank) {
    const size_t slot = (size_t)p * a.num_seeds + rank;
    const int i = rank < S ? order[rank] : -1;
    if (a.seed_rows) a.seed_rows[slot] = i;
    if (a.hyp_count) a.hyp_count[slot] = -1;
    if (a.hyp_rt)
      for (int k = 0; k < 12; ++k) a.hyp_rt[12 * slot + k] = 0.0f;
    if (a.consensus)
      for (int k = 0; k < a.set_size; ++k) a.consensus[slot * a.set_size + k] = -1;
    if (i < 0) continue;
    keys.clear();
    for (int j = 0; j < n; ++j)
      if ((M[(size_t)i * W + (j >> 6)] >> (j & 63)) & 1ull) {
        int s = 0;
        for (int w = 0; w < W; ++w) s += __builtin_popcountll(M[(size_t)i * W + w] & M[(size_t)j * W + w]);
        keys.push_back(candidate_key(s, j));
      }
    std::sort(keys.begin(), keys.end(), [](uint32_t x, uint32_t y) { return x > y; });
    const int m = std::min(a.set_size - 1, deg[i]), cnt = m + 1;
    int set[kMaxSet];
    double ss[3 * kMaxSet], sg[3 * kMaxSet];
    set[0] = i;
    for (int k = 0; k < m; ++k) set[k + 1] = candidate_of(keys[k]);
    for (int k = 0; k < cnt; ++k) {
      if (a.consensus) a.consensus[slot * a.set_size + k] = set[k];
      for (int c = 0; c < 3; ++c) {
        ss[3 * k + c] = ps[3 * (size_t)set[k] + c];
        sg[3 * k + c] = pg[3 * (size_t)set[k] + c];
      }
    }
    if (deg[i] < 2) continue;
    double R[9], t[3];
    float rt[12];
    d3f::rigid::fit(ss, sg, cnt, R, t);
    d3f::rigid::to_f32(R, t, rt);
    int c = 0;
    for (int r = 0; r < n; ++r) {
      const size_t q = 3 * (size_t)(off + r);
      c += d3f::rigid::inlier_f32(rt, a.tgt[q], a.tgt[q + 1], a.tgt[q + 2], a.src[q], a.src[q + 1], a.src[q + 2], a.tau2) ? 1 : 0;
    }
    if (a.hyp_count) a.hyp_count[slot] = c;
    if (a.hyp_rt)
      for (int k = 0; k < 12; ++k) a.hyp_rt[12 * slot + k] = rt[k];
    const unsigned long long key = hypothesis_key(c, rank);
    if (key > best) {
      best = key;
      for (int k = 0; k < 9; ++k) bestR[k] = R[k];
      for (int k = 0; k < 3; ++k) bestt[k] = t[k];
    }
  }
  int seed = -1, pre = 0, fin = 0;
  if (st == 0 && best == 0ull) st = kStNoHypothesis;
  if (st == 0) {
    seed = order[(int)~(uint32_t)(best & 0xffffffffull)];
    pre = (int)(best >> 32) - 1;
    fin = d3f::rigid::refine_host(a.src, a.tgt, off, n, a.tau2, a.refine_iters, bestR, bestt);
  } else {
    const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int k = 0; k < 9; ++k) bestR[k] = eye[k];
    for (int k = 0; k < 3; ++k) bestt[k] = 0.0;
  }
  double* o = a.T + 16 * (size_t)p;
  for (int r = 0; r < 3; ++r) {
    o[4 * r] = bestR[3 * r];
    o[4 * r + 1] = bestR[3 * r + 1];
    o[4 * r + 2] = bestR[3 * r + 2];
    o[4 * r + 3] = bestt[r];
  }
  o[12] = 0.0; o[13] = 0.0; o[14] = 0.0; o[15] = 1.0;
  a.inliers[p] = fin;
  a.best_seed[p] = seed;
  a.best_count[p] = pre;
  a.status[p] = st;
}

// the argument checks both entries share
int prepare(const float* src, const float* tgt, int rows, const int32_t* seg, int P, int max_count,
            double distance_threshold, double compat_threshold, int num_seeds, int set_size, int refine_iters, double* T,
            int32_t* inliers, int32_t* best_seed, int32_t* best_count, int32_t* status, int32_t* degree, int32_t* seed_rows,
            int32_t* consensus, int32_t* hyp_count, float* hyp_rt, Params& a) {
  if ((rows > 0 && (!src || !tgt)) || !seg || !T || !inliers || !best_seed || !best_count || !status || rows < 0 ||
      P < 1 || P > 65535 || max_count < 1 || max_count > D3F_SC2_MAX_COUNT || num_seeds < 1 ||
      num_seeds > D3F_SC2_MAX_SEEDS || set_size < 3 || set_size > D3F_SC2_MAX_SET || refine_iters < 0 ||
      refine_iters > D3F_RANSAC_MAX_REFINE || !(distance_threshold > 0.0) || !(distance_threshold < INFINITY) ||
      !(compat_threshold > 0.0) || !(compat_threshold < INFINITY))
    return D3F_EINVAL;
  const float tau = (float)distance_threshold;
  if (!(tau > 0.0f) || !(tau < INFINITY)) return D3F_EINVAL;
  a = {};
  a.src = src; a.tgt = tgt; a.rows = rows; a.seg = seg;
  a.P = P; a.max_count = max_count; a.W = words_of(max_count);
  a.tau2 = tau * tau;
  a.compat2 = compat_threshold * compat_threshold;
  a.num_seeds = num_seeds; a.set_size = set_size; a.refine_iters = refine_iters;
  a.T = T; a.inliers = inliers; a.best_seed = best_seed; a.best_count = best_count; a.status = status;
  a.degree = degree; a.seed_rows = seed_rows; a.consensus = consensus; a.hyp_count = hyp_count; a.hyp_rt = hyp_rt;
  return D3F_OK;
}

}  // namespace

extern "C" {

size_t d3f_sc2_rigid_ws_bytes(int P, int max_count, int num_seeds) { return layout_of(P, max_count, num_seeds).total; }

int d3f_sc2_rigid(const float* src, const float* tgt, int rows, const int32_t* seg, int P, int max_count,
                  double distance_threshold, double compat_threshold, int num_seeds, int set_size, int refine_iters,
                  double* T, int32_t* inliers, int32_t* best_seed, int32_t* best_count, int32_t* status, int32_t* degree,
                  int32_t* seed_rows, int32_t* consensus, int32_t* hyp_count, float* hyp_rt, void* ws, size_t ws_bytes,
                  void* stream) {
  Params a;
  const int rc = prepare(src, tgt, rows, seg, P, max_count, distance_threshold, compat_threshold, num_seeds, set_size,
                         refine_iters, T, inliers, best_seed, best_count, status, degree, seed_rows, consensus, hyp_count,
                         hyp_rt, a);
  if (rc != D3F_OK) return rc;
  if (!ws) return D3F_EINVAL;
  const Layout l = layout_of(P, max_count, num_seeds);
  if (ws_bytes < l.total) return D3F_EWORKSPACE;
  char* base = (char*)ws;
  a.matrix = (unsigned long long*)(base + l.matrix);
  a.ws_degree = (int32_t*)(base + l.degree);
  a.ws_seeds = (int32_t*)(base + l.seeds);
  a.ws_keys = (unsigned long long*)(base + l.keys);
  a.ws_poses = (double*)(base + l.poses);
  hipStream_t s = (hipStream_t)stream;
  matrix_kernel<<<dim3(d3f::cdiv(max_count, kStrip), P), kThreads, 0, s>>>(a);
  seeds_kernel<<<P, kThreads, 0, s>>>(a);
  hypothesis_kernel<<<dim3(num_seeds, P), kThreads, 0, s>>>(a);
  select_kernel<<<P, kThreads, 0, s>>>(a);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_sc2_rigid_host(const float* src_host, const float* tgt_host, int rows, const int32_t* seg_host, int P,
                       int max_count, double distance_threshold, double compat_threshold, int num_seeds, int set_size,
                       int refine_iters, double* T_host, int32_t* inliers_host, int32_t* best_seed_host,
                       int32_t* best_count_host, int32_t* status_host, int32_t* degree_host, int32_t* seed_rows_host,
                       int32_t* consensus_host, int32_t* hyp_count_host, float* hyp_rt_host, uint64_t* matrix_host) {
  Params a;
  const int rc = prepare(src_host, tgt_host, rows, seg_host, P, max_count, distance_threshold, compat_threshold,
                         num_seeds, set_size, refine_iters, T_host, inliers_host, best_seed_host, best_count_host,
                         status_host, degree_host, seed_rows_host, consensus_host, hyp_count_host, hyp_rt_host, a);
  if (rc != D3F_OK) return rc;
  const size_t slice = (size_t)max_count * a.W;
  std::vector<unsigned long long> own(matrix_host ? 0 : slice);
  for (int p = 0; p < P; ++p) {
    unsigned long long* M = matrix_host ? (unsigned long long*)matrix_host + (size_t)p * slice : own.data();
    std::fill(M, M + slice, 0ull);
    host_pair(a, p, M);
  }
  return D3F_OK;
}

}  // extern "C"
