// Batched RANSAC rigid registration of P correspondence sets -- what the reference hands to Open3D's
// registration_ransac_based_on_correspondence, as two launches per batch (no host synchronisation, graph-capturable).
//
// Input: src / tgt [rows,3] f32, seg [P,2] int32 = (offset, count) per pair.  Output: the transform that maps the
// TARGET onto the SOURCE, src ~ R tgt + t (the gt.log convention).  Sampler, minimal-set checks, solver and inlier test
// are the __host__ __device__ functions of rigid.hpp (their exact formulas are written there).
//
// 1. score_kernel: grid (ceil(H / 1024), P), 256 threads.  Each thread owns 4 hypotheses h = 1024 bx + 256 j + tid:
//    draws 3 indices, checks them, fits (R, t) in f64 and keeps the f32 image in registers (48 VGPRs).  The pair's
//    correspondences stream through LDS in tiles of 256; every lane reads the same LDS address (a broadcast), and each
//    point read feeds 4 inlier tests of ~17 VALU instructions each.  Counts are integers: no reduction-order effect.
//    The block's best key  ((count + 1) << 32) | ~h  (0 for an invalid hypothesis) goes to its slot of a per-block slab:
//    the largest key is the largest count, ties to the LOWEST h.  Optionally every hypothesis' count (-1 when invalid)
//    and f32 (R row-major, t) are written for tests.
// 2. refine_kernel: one workgroup per pair.  Maximum of the pair's slab slots, re-derivation of the winner from the hash
//    (nothing per hypothesis is stored), then refine_iters x { inliers under the current (R, t) -> f64 centroids and
//    cross-covariance over them (per-thread strided partial sums, then a fixed LDS tree: the same order on every run)
//    -> Horn fit }, then a final recount.  A refit needs >= 3 inliers, else the current transform is kept.  The loop
//    is rigid::refine of rigid_refine.hpp, which sc2.hip runs too.
#include "common.hpp"
#include "rigid.hpp"
#include "rigid_refine.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kHypPerThread = 4;
constexpr int kHypPerBlock = kThreads * kHypPerThread;
constexpr int kTile = 256;

// (offset, count) of pair p, with the pair's status bits for what makes it unusable
__device__ __forceinline__ int pair_segment(const int32_t* __restrict__ seg, int p, int rows, int& off, int& count) {
  off = seg[2 * p];
  count = seg[2 * p + 1];
  if (off < 0 || count < 0 || count > D3F_RANSAC_MAX_COUNT || (long long)off + count > rows) {
    count = 0;
    return D3F_RANSAC_ST_SEGMENT;
  }
  return count < 3 ? D3F_RANSAC_ST_FEW : 0;
}

// hypothesis h of a pair: draw, check, fit.  false: invalid (R, t untouched)
__device__ __forceinline__ bool hypothesis(const float* __restrict__ src, const float* __restrict__ tgt, int off,
                                           int count, uint64_t key, int h, float edge_ratio, double R[9], double t[3]) {
  int idx[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) idx[k] = d3f::rigid::draw(key, h, k, count);
  if (idx[0] == idx[1] || idx[0] == idx[2] || idx[1] == idx[2]) return false;
  double s[9], g[9];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      s[3 * k + a] = (double)src[3 * (size_t)(off + idx[k]) + a];
      g[3 * k + a] = (double)tgt[3 * (size_t)(off + idx[k]) + a];
    }
  if (!d3f::rigid::triple_ok(s, g, (double)edge_ratio)) return false;
  d3f::rigid::fit(s, g, 3, R, t);
  return true;
}

using d3f::rigid::kRed;
using d3f::rigid::to_f32;
static_assert(kThreads == d3f::rigid::kRefineThreads, "the refinement's tree is written for this workgroup");

__global__ __launch_bounds__(kThreads) void score_kernel(const float* __restrict__ src, const float* __restrict__ tgt,
                                                         int rows, const int32_t* __restrict__ seg, int first_pair,
                                                         int H, float tau2, float edge_ratio, uint64_t seed,
                                                         unsigned long long* __restrict__ slab, int nblk,
                                                         int32_t* __restrict__ hyp_count, float* __restrict__ hyp_rt) {
  __shared__ float4 ts[kTile], tt[kTile];
  __shared__ unsigned long long wbest[kThreads / D3F_WAVE];
  const int p = blockIdx.y, tid = threadIdx.x;
  int off, count;
  const int st = pair_segment(seg, p, rows, off, count);
  const uint64_t key = d3f::rigid::pair_key(seed, first_pair + p);
  float rt[kHypPerThread][12];
  bool valid[kHypPerThread];
  int cnt[kHypPerThread];
#pragma unroll
  for (int j = 0; j < kHypPerThread; ++j) {
    const int h = blockIdx.x * kHypPerBlock + j * kThreads + tid;
    double R[9], t[3];
    valid[j] = st == 0 && h < H && hypothesis(src, tgt, off, count, key, h, edge_ratio, R, t);
    if (valid[j]) {
      to_f32(R, t, rt[j]);
    } else {
#pragma unroll
      for (int i = 0; i < 12; ++i) rt[j][i] = 0.0f;
    }
    cnt[j] = 0;
  }
  const int n_all = st == 0 ? count : 0;
  for (int base = 0; base < n_all; base += kTile) {
    const int n = min(kTile, n_all - base);
    __syncthreads();   // the previous tile is consumed
    if (tid < n) {
      const size_t r = 3 * (size_t)(off + base + tid);
      ts[tid] = make_float4(src[r], src[r + 1], src[r + 2], 0.0f);
      tt[tid] = make_float4(tgt[r], tgt[r + 1], tgt[r + 2], 0.0f);
    }
    __syncthreads();
#pragma unroll 2
    for (int i = 0; i < n; ++i) {
      const float4 a = ts[i], b = tt[i];   // same address in every lane: LDS broadcast
#pragma unroll
      for (int j = 0; j < kHypPerThread; ++j)
        cnt[j] += d3f::rigid::inlier_f32(rt[j], b.x, b.y, b.z, a.x, a.y, a.z, tau2) ? 1 : 0;
    }
  }
  unsigned long long best = 0ull;
#pragma unroll
  for (int j = 0; j < kHypPerThread; ++j) {
    const int h = blockIdx.x * kHypPerBlock + j * kThreads + tid;
    const unsigned long long k =
        valid[j] ? (((unsigned long long)(uint32_t)(cnt[j] + 1) << 32) | (unsigned long long)(uint32_t)~(uint32_t)h) : 0ull;
    best = k > best ? k : best;
    if (h < H) {
      const size_t o = (size_t)p * H + h;
      if (hyp_count) hyp_count[o] = valid[j] ? cnt[j] : -1;
      if (hyp_rt) {
#pragma unroll
        for (int i = 0; i < 12; ++i) hyp_rt[12 * o + i] = rt[j][i];
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(best, o, 64);
    best = other > best ? other : best;
  }
  if (d3f::lane_id() == 0) wbest[tid / D3F_WAVE] = best;
  __syncthreads();
  if (tid == 0) {
    unsigned long long b = wbest[0];
#pragma unroll
    for (int w = 1; w < kThreads / D3F_WAVE; ++w) b = wbest[w] > b ? wbest[w] : b;
    slab[(size_t)p * nblk + blockIdx.x] = b;
  }
}

__global__ __launch_bounds__(kThreads) void refine_kernel(const float* __restrict__ src, const float* __restrict__ tgt,
                                                          int rows, const int32_t* __restrict__ seg, int first_pair,
                                                          float tau2, float edge_ratio, uint64_t seed, int refine_iters,
                                                          const unsigned long long* __restrict__ slab, int nblk,
                                                          double* __restrict__ T, int32_t* __restrict__ inliers,
                                                          int32_t* __restrict__ best_h, int32_t* __restrict__ best_count,
                                                          int32_t* __restrict__ status) {
  __shared__ double red[kThreads][kRed];
  __shared__ unsigned long long wbest[kThreads / D3F_WAVE];
  const int p = blockIdx.x, tid = threadIdx.x;
  int off, count;
  int st = pair_segment(seg, p, rows, off, count);
  unsigned long long best = 0ull;
  for (int b = tid; b < nblk; b += kThreads) best = slab[(size_t)p * nblk + b] > best ? slab[(size_t)p * nblk + b] : best;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(best, o, 64);
    best = other > best ? other : best;
  }
  if (d3f::lane_id() == 0) wbest[tid / D3F_WAVE] = best;
  __syncthreads();
  best = wbest[0];
#pragma unroll
  for (int w = 1; w < kThreads / D3F_WAVE; ++w) best = wbest[w] > best ? wbest[w] : best;
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
  int h = -1, pre = 0, fin = 0;
  if (st == 0 && best == 0ull) st = D3F_RANSAC_ST_NO_HYPOTHESIS;
  if (st == 0) {   // uniform over the workgroup: every thread re-derives the same winner
    h = (int)~(uint32_t)(best & 0xffffffffull);
    pre = (int)(best >> 32) - 1;
    hypothesis(src, tgt, off, count, d3f::rigid::pair_key(seed, first_pair + p), h, edge_ratio, R, t);
    fin = d3f::rigid::refine(src, tgt, off, count, tau2, refine_iters, red, R, t);
  }
  if (tid == 0) {
    double* o = T + 16 * (size_t)p;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      o[4 * a] = R[3 * a];
      o[4 * a + 1] = R[3 * a + 1];
      o[4 * a + 2] = R[3 * a + 2];
      o[4 * a + 3] = t[a];
    }
    o[12] = 0.0; o[13] = 0.0; o[14] = 0.0; o[15] = 1.0;
    inliers[p] = fin;
    best_h[p] = h;
    best_count[p] = pre;
    status[p] = st;
  }
}

}  // namespace

extern "C" {

size_t d3f_ransac_rigid_ws_bytes(int P, int H) {
  const size_t nblk = H > 0 ? (size_t)d3f::cdiv(H, kHypPerBlock) : 1;
  return d3f::align_up(8 * (size_t)(P > 0 ? P : 1) * nblk, 256);
}

int d3f_ransac_rigid(const float* src, const float* tgt, int rows, const int32_t* seg, int P, int first_pair, int H,
                     float distance_threshold, float edge_ratio, int refine_iters, uint64_t seed, double* T,
                     int32_t* inliers, int32_t* best_hypothesis, int32_t* best_count, int32_t* status,
                     int32_t* hyp_count, float* hyp_rt, void* ws, size_t ws_bytes, void* stream) {
  if ((rows > 0 && (!src || !tgt)) || !seg || !T || !inliers || !best_hypothesis || !best_count || !status || !ws || rows < 0 ||
      P < 1 || P > 65535 || first_pair < 0 || H < 1 || H > D3F_RANSAC_MAX_HYPOTHESES || refine_iters < 0 ||
      refine_iters > D3F_RANSAC_MAX_REFINE || !(distance_threshold > 0.0f) || !(distance_threshold < INFINITY) ||
      !(edge_ratio >= 0.0f && edge_ratio <= 1.0f))
    return D3F_EINVAL;
  if (ws_bytes < d3f_ransac_rigid_ws_bytes(P, H)) return D3F_EWORKSPACE;
  const int nblk = d3f::cdiv(H, kHypPerBlock);
  const float tau2 = distance_threshold * distance_threshold;
  unsigned long long* slab = (unsigned long long*)ws;
  hipStream_t s = (hipStream_t)stream;
  score_kernel<<<dim3(nblk, P), kThreads, 0, s>>>(src, tgt, rows, seg, first_pair, H, tau2, edge_ratio, seed, slab,
                                                  nblk, hyp_count, hyp_rt);
  refine_kernel<<<P, kThreads, 0, s>>>(src, tgt, rows, seg, first_pair, tau2, edge_ratio, seed, refine_iters, slab, nblk,
                                       T, inliers, best_hypothesis, best_count, status);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_ransac_sample_host(uint64_t seed, int p, int h, int count, int32_t* out_host) {
  if (!out_host || p < 0 || h < 0 || count < 1) return D3F_EINVAL;
  const uint64_t key = d3f::rigid::pair_key(seed, p);
  for (int k = 0; k < 3; ++k) out_host[k] = d3f::rigid::draw(key, h, k, count);
  return D3F_OK;
}

int d3f_rigid_fit_host(const double* src_host, const double* tgt_host, int n, double* out_host) {
  if (!src_host || !tgt_host || !out_host || n < 1) return D3F_EINVAL;
  double R[9], t[3];
  d3f::rigid::fit(src_host, tgt_host, n, R, t);
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) out_host[4 * a + b] = R[3 * a + b];
    out_host[4 * a + 3] = t[a];
  }
  out_host[12] = 0.0; out_host[13] = 0.0; out_host[14] = 0.0; out_host[15] = 1.0;
  return D3F_OK;
}

}  // extern "C"
