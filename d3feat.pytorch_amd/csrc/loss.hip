// Fused descriptor-matching loss: all-pairs L2 distance + circle loss + detector loss, forward and backward.
//
// Replaces reference utils/loss.py: cdist 'euclidean' (:8-44), CircleLoss.forward (:111-141) and
// DetLoss.forward (:149-158) -- ~40 small PyTorch launches and two host syncs per step in the reference.
// M (sampled correspondences) is 128 in training / 64 in validation (config.py:78).  At M <= 128, C <= 64 the M x M
// problem of every stacked pair is cut into strips of lines, one workgroup each, and a second tiny launch sums the
// scalars (the tiled kernels below); larger problems fall back to ONE workgroup of 1024 threads working on the global
// buffers, a single pair at a time.  Distances go to the caller's `dists` buffer (an output of the reference API as
// well) in either form.
//
// Semantics reproduced literally (including the reference's quirk that masked entries contribute exp(-0) = 1 to
// the log-sum-exp because their detached weight is clamped to 0):
//   D      = sqrt(sum_c (a_i - p_j)^2 + 1e-12)
//   pos    = D - 1e5*neg_mask,  pw = max(0, pos - pos_margin)       T+ = s*(pos - pos_margin)*pw
//   neg    = D + 1e5*(1-neg_mask), nw = max(0, neg_margin - neg)    T- = s*(neg_margin - neg)*nw
//   desc   = mean_i softplus(lse_j T+ + lse_j T-)/s + mean_j softplus(lse_i T+ + lse_i T-)/s
//   det    = mean_i (D_ii - min_j (D + 1e5*I)_ij) * (sa_i + sp_i)
#include "common.hpp"

namespace {

constexpr int kThreads = 1024;
constexpr int kMaxM = 1024;

struct LossParams {
  float s, safe_radius, pos_margin, neg_margin;
};

__device__ __forceinline__ float softplus_t(float x) { return x > 20.0f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float sigmoid_sp(float x) { return x > 20.0f ? 1.0f : 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ void terms(float d, bool negm, const LossParams& P, float& tpos, float& pw, float& tneg,
                                      float& nw) {
  const float pos = d - 1e5f * (negm ? 1.0f : 0.0f);
  pw = fmaxf(0.0f, pos - P.pos_margin);
  tpos = P.s * (pos - P.pos_margin) * pw;
  const float neg = d + 1e5f * (negm ? 0.0f : 1.0f);
  nw = fmaxf(0.0f, P.neg_margin - neg);
  tneg = P.s * (P.neg_margin - neg) * nw;
}

// wave-cooperative statistics of one line of D: element t of the line is D[base + t*stride] (mask alike)
__device__ void line_stats(const float* __restrict__ D, long dbase, long dstride, const uint8_t* __restrict__ negm,
                           long nbase, long nstride, int M, int self, const LossParams& P, float& lse_p, float& lse_n,
                           float& sumd, float& cmin, int& carg) {
  const int lane = threadIdx.x & 63;
  float mp = -INFINITY, mn = -INFINITY, sd = 0.0f, cm = INFINITY;
  int ca = 0x7fffffff;
  for (int t = lane; t < M; t += 64) {
    const float d = D[dbase + t * dstride];
    float tp, pw, tn, nw;
    terms(d, negm[nbase + t * nstride] != 0, P, tp, pw, tn, nw);
    mp = fmaxf(mp, tp);
    mn = fmaxf(mn, tn);
    sd += d;
    const float dm = d + (t == self ? 1e5f : 0.0f);
    if (dm < cm) { cm = dm; ca = t; }
  }
  mp = d3f::wave_max(mp);
  mn = d3f::wave_max(mn);
  sd = d3f::wave_sum(sd);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {  // (value, index) lexicographic min -> first minimal index like torch.min
    const float ov = __shfl_xor(cm, o, 64);
    const int oa = __shfl_xor(ca, o, 64);
    if (ov < cm || (ov == cm && oa < ca)) { cm = ov; ca = oa; }
  }
  float ep = 0.0f, en = 0.0f;
  for (int t = lane; t < M; t += 64) {
    const float d = D[dbase + t * dstride];
    float tp, pw, tn, nw;
    terms(d, negm[nbase + t * nstride] != 0, P, tp, pw, tn, nw);
    ep += expf(tp - mp);
    en += expf(tn - mn);
  }
  ep = d3f::wave_sum(ep);
  en = d3f::wave_sum(en);
  lse_p = mp + logf(ep);
  lse_n = mn + logf(en);
  sumd = sd;
  cmin = cm;
  carg = ca;
}

__device__ float block_sum(float v, float* sh) {
  v = d3f::wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.0f;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += sh[w];
  return t;
}

// the tiled kernels' domain; beyond it the one-workgroup kernels run on the global buffers
static bool cache_ok(int M, int C) { return M <= 128 && C <= 64; }

// stats layout (floats): [0,M) lse_pr  [M,2M) lse_nr  [2M,3M) lse_pc  [3M,4M) lse_nc  [4M,5M) cn  [5M,6M) cnarg(int)
__global__ __launch_bounds__(kThreads) void loss_fwd_kernel(
    const float* __restrict__ a, const float* __restrict__ p, int M, int C, const uint8_t* __restrict__ negm,
    const float* __restrict__ sa, const float* __restrict__ sp, LossParams P, float* __restrict__ D,
    float* __restrict__ fp_out, float* __restrict__ avgneg_out, float* __restrict__ scalars,
    float* __restrict__ stats) {
  __shared__ float sh[16];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, nw = blockDim.x >> 6;
  for (int t = tid; t < M * M; t += blockDim.x) {
    const int i = t / M, j = t % M;
    float acc = 0.0f;
    for (int c = 0; c < C; ++c) {
      const float df = a[(size_t)i * C + c] - p[(size_t)j * C + c];
      acc += df * df;
    }
    D[t] = sqrtf(acc + 1e-12f);
  }
  __threadfence_block();
  __syncthreads();
  const long ld = M;   // row stride of D
  for (int i = wave; i < M; i += nw) {
    float lp, ln, sd, cm; int ca;
    line_stats(D, (long)i * ld, 1, negm, (long)i * M, 1, M, i, P, lp, ln, sd, cm, ca);
    if (lane == 0) {
      stats[i] = lp;
      stats[M + i] = ln;
      stats[4 * M + i] = cm;
      ((int*)stats)[5 * M + i] = ca;
      const float fp = D[(long)i * ld + i];  // max_j D*I = D_ii (D > 0)
      fp_out[i] = fp;
      avgneg_out[i] = (sd - fp) / (float)(M - 1);
    }
  }
  for (int j = wave; j < M; j += nw) {
    float lp, ln, sd, cm; int ca;
    line_stats(D, (long)j, ld, negm, (long)j, M, M, j, P, lp, ln, sd, cm, ca);
    if (lane == 0) {
      stats[2 * M + j] = lp;
      stats[3 * M + j] = ln;
    }
  }
  __threadfence_block();
  __syncthreads();
  float l = 0.0f, dt = 0.0f, ac = 0.0f, fps = 0.0f, ans = 0.0f;
  for (int i = tid; i < M; i += blockDim.x) {
    l += softplus_t(stats[i] + stats[M + i]) / P.s + softplus_t(stats[2 * M + i] + stats[3 * M + i]) / P.s;
    const float diff = fp_out[i] - stats[4 * M + i];
    dt += diff * (sa[i] + sp[i]);
    ac += diff < 0.0f ? 1.0f : 0.0f;
    fps += fp_out[i];
    ans += avgneg_out[i];
  }
  l = block_sum(l, sh);
  dt = block_sum(dt, sh);
  ac = block_sum(ac, sh);
  fps = block_sum(fps, sh);
  ans = block_sum(ans, sh);
  if (tid == 0) {
    scalars[0] = l / (float)M;
    scalars[1] = dt / (float)M;
    scalars[2] = ac * 100.0f / (float)M;
    scalars[3] = fps / (float)M;
    scalars[4] = ans / (float)M;
    scalars[5] = l / (float)M + dt / (float)M;  // desc + det: the step's loss with unit weights (trainer.py:98)
  }
}

// G [M,M] = dL/dD / D: the caller's workspace
__global__ __launch_bounds__(kThreads) void loss_bwd_kernel(
    const float* __restrict__ a, const float* __restrict__ p, int M, int C, const uint8_t* __restrict__ negm,
    const float* __restrict__ sa, const float* __restrict__ sp, LossParams P, const float* __restrict__ D,
    const float* __restrict__ stats, const float* __restrict__ g_desc, const float* __restrict__ g_det,
    float* __restrict__ G, float* __restrict__ ga, float* __restrict__ gp, float* __restrict__ gsa,
    float* __restrict__ gsp) {
  const int tid = threadIdx.x;
  const float gd = g_desc ? *g_desc : 0.0f, gt = g_det ? *g_det : 0.0f;
  const float invM = 1.0f / (float)M;
  for (int t = tid; t < M * M; t += blockDim.x) {
    const int i = t / M, j = t % M;
    const float d = D[t];
    float tp, pw, tn, nw;
    terms(d, negm[t] != 0, P, tp, pw, tn, nw);
    const float sr = sigmoid_sp(stats[i] + stats[M + i]);
    const float sc = sigmoid_sp(stats[2 * M + j] + stats[3 * M + j]);
    float g = gd * invM * (sr * (expf(tp - stats[i]) * pw - expf(tn - stats[M + i]) * nw) +
                           sc * (expf(tp - stats[2 * M + j]) * pw - expf(tn - stats[3 * M + j]) * nw));
    const float w = gt * invM * (sa[i] + sp[i]);
    if (j == i) g += w;
    if (j == ((const int*)stats)[5 * M + i]) g -= w;
    G[t] = g / d;
  }
  __threadfence_block();
  __syncthreads();
  for (int t = tid; t < M * C; t += blockDim.x) {
    const int i = t / C, c = t % C;
    float acc = 0.0f;
    const float ai = a[t];
    for (int j = 0; j < M; ++j) acc += G[(size_t)i * M + j] * (ai - p[(size_t)j * C + c]);
    ga[t] = acc;
  }
  for (int t = tid; t < M * C; t += blockDim.x) {
    const int j = t / C, c = t % C;
    float acc = 0.0f;
    const float pj = p[t];
    for (int i = 0; i < M; ++i) acc += G[(size_t)i * M + j] * (pj - a[(size_t)i * C + c]);
    gp[t] = acc;
  }
  for (int i = tid; i < M; i += blockDim.x) {
    const float v = gt * invM * (D[(size_t)i * M + i] - stats[4 * M + i]);
    if (gsa) gsa[i] = v;
    if (gsp) gsp[i] = v;
  }
}

// ---- tiled variants (M <= 128, C <= 64: the training / validation shapes) ------------------------------------------
// The one-workgroup kernels above spend 71 + 55 us per step on ONE of 256 CUs (16k distances x 32 channels through
// LDS, then 256 wave-serial line statistics).  Here the matrix is cut into strips of kLossStrip lines: workgroup g owns
// rows [g L, (g+1) L) AND columns [g L, (g+1) L) -- it computes its row strip and its column strip of D itself (the
// same expression in the same order, so both copies of an element are bit-identical), takes the row statistics from
// the one and the column statistics from the other, and never needs another workgroup's data.  Forward: the scalar
// sums over all lines are left to a second, tiny launch (loss_finalize_kernel) -- a dependent launch costs 1.7 us here
// (profiles/r03_launch_floor.txt), an in-kernel rendezvous of 8 workgroups more.  Backward: ga needs row strips of G, gp
// column strips: no cross-workgroup dependency at all.
constexpr int kLossStrip = 8;

__host__ __device__ inline size_t tiled_lds_bytes(int M, int C) {
  // a, p [M][C+1]; row strip [L][M+1]; column strip [M][L+1]; mask bytes of both strips
  return sizeof(float) * ((size_t)2 * M * (C + 1) + (size_t)kLossStrip * (M + 1) + (size_t)M * (kLossStrip + 1)) +
         (size_t)2 * kLossStrip * M;
}

__global__ __launch_bounds__(256) void loss_fwd_tile_kernel(const float* __restrict__ a, const float* __restrict__ p,
                                                            int M, int C, const uint8_t* __restrict__ negm, LossParams P,
                                                            float* __restrict__ D, float* __restrict__ fp_out,
                                                            float* __restrict__ avgneg_out, float* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int L = kLossStrip;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int CS = C + 1, RS = M + 1, KS = L + 1;
  float* al = lds;
  float* pl = al + (size_t)M * CS;
  float* Dr = pl + (size_t)M * CS;            // [L][RS]  rows l0 .. l0+L-1
  float* Dc = Dr + (size_t)L * RS;            // [M][KS]  columns l0 .. l0+L-1
  uint8_t* mr = (uint8_t*)(Dc + (size_t)M * KS);   // [L][M]
  uint8_t* mc = mr + (size_t)L * M;                // [M][L]
  const int l0 = blockIdx.x * L, nl = min(L, M - l0);
  {  // blockIdx.y = fragment pair of a stacked batch: its own M x M problem
    const size_t pr = blockIdx.y;
    a += pr * M * C; p += pr * M * C; negm += pr * M * M; D += pr * M * M;
    fp_out += pr * M; avgneg_out += pr * M; stats += pr * 6 * M;
  }
  for (int t = tid; t < M * C; t += 256) {
    al[(t / C) * CS + t % C] = a[t];
    pl[(t / C) * CS + t % C] = p[t];
  }
  for (int t = tid; t < nl * M; t += 256) {
    mr[t] = negm[(size_t)(l0 + t / M) * M + t % M];
    const int i = t / nl, c = t % nl;
    mc[i * L + c] = negm[(size_t)i * M + l0 + c];
  }
  __syncthreads();
  for (int t = tid; t < nl * M; t += 256) {
    {  // row strip
      const int r = t / M, j = t % M;
      float acc = 0.0f;
      for (int c = 0; c < C; ++c) {
        const float df = al[(l0 + r) * CS + c] - pl[j * CS + c];
        acc += df * df;
      }
      const float d = sqrtf(acc + 1e-12f);
      Dr[r * RS + j] = d;
      D[(size_t)(l0 + r) * M + j] = d;
    }
    {  // column strip
      const int i = t / nl, cc = t % nl;
      float acc = 0.0f;
      for (int c = 0; c < C; ++c) {
        const float df = al[i * CS + c] - pl[(l0 + cc) * CS + c];
        acc += df * df;
      }
      Dc[i * KS + cc] = sqrtf(acc + 1e-12f);
    }
  }
  __syncthreads();
  for (int r = wave; r < nl; r += 4) {
    const int i = l0 + r;
    float lp, ln, sd, cm; int ca;
    line_stats(Dr, (long)r * RS, 1, mr, (long)r * M, 1, M, i, P, lp, ln, sd, cm, ca);
    if (lane == 0) {
      stats[i] = lp;
      stats[M + i] = ln;
      stats[4 * M + i] = cm;
      ((int*)stats)[5 * M + i] = ca;
      const float fp = Dr[r * RS + i];  // max_j D*I = D_ii (D > 0)
      fp_out[i] = fp;
      avgneg_out[i] = (sd - fp) / (float)(M - 1);
    }
  }
  for (int cc = wave; cc < nl; cc += 4) {
    const int j = l0 + cc;
    float lp, ln, sd, cm; int ca;
    line_stats(Dc, (long)cc, KS, mc, (long)cc, L, M, j, P, lp, ln, sd, cm, ca);
    if (lane == 0) {
      stats[2 * M + j] = lp;
      stats[3 * M + j] = ln;
    }
  }
}

// scalars of the loss from the per-line statistics (second launch of the tiled forward).  One workgroup walks the
// `pairs` problems of a stacked batch one after the other (pairs <= 32, M <= 128: nothing to spread) and leaves
// total = sum_p (w_desc desc_p + w_det det_p) -- the step's loss, whose gradient is the SUM of the pairs' gradients.
__global__ __launch_bounds__(256) void loss_finalize_kernel(int M, const float* __restrict__ sa, const float* __restrict__ sp,
                                                            LossParams P, const float* __restrict__ fp_out,
                                                            const float* __restrict__ avgneg_out,
                                                            const float* __restrict__ stats, float* __restrict__ scalars,
                                                            int pairs, float w_desc, float w_det,
                                                            float* __restrict__ total) {
  __shared__ float sh[16];
  const int tid = threadIdx.x;
  float tot = 0.0f;
  for (int pr = 0; pr < pairs; ++pr, sa += M, sp += M, fp_out += M, avgneg_out += M, stats += 6 * M, scalars += 6) {
    float l = 0.0f, dt = 0.0f, ac = 0.0f, fps = 0.0f, ans = 0.0f;
    for (int i = tid; i < M; i += blockDim.x) {
      l += softplus_t(stats[i] + stats[M + i]) / P.s + softplus_t(stats[2 * M + i] + stats[3 * M + i]) / P.s;
      const float diff = fp_out[i] - stats[4 * M + i];
      dt += diff * (sa[i] + sp[i]);
      ac += diff < 0.0f ? 1.0f : 0.0f;
      fps += fp_out[i];
      ans += avgneg_out[i];
    }
    l = block_sum(l, sh);
    dt = block_sum(dt, sh);
    ac = block_sum(ac, sh);
    fps = block_sum(fps, sh);
    ans = block_sum(ans, sh);
    if (tid == 0) {
      scalars[0] = l / (float)M;
      scalars[1] = dt / (float)M;
      scalars[2] = ac * 100.0f / (float)M;
      scalars[3] = fps / (float)M;
      scalars[4] = ans / (float)M;
      scalars[5] = l / (float)M + dt / (float)M;  // desc + det: the step's loss with unit weights (trainer.py:98)
    }
    tot += w_desc * (l / (float)M) + w_det * (dt / (float)M);
  }
  if (tid == 0 && total) *total = tot;
}

__device__ __forceinline__ float loss_grad_entry(float d, bool negm, int i, int j, int M, const LossParams& P,
                                                 const float* __restrict__ stats, float gdM, float w) {
  float tp, pw, tn, nw;
  terms(d, negm, P, tp, pw, tn, nw);
  const float sr = sigmoid_sp(stats[i] + stats[M + i]);
  const float sc = sigmoid_sp(stats[2 * M + j] + stats[3 * M + j]);
  float g = gdM * (sr * (expf(tp - stats[i]) * pw - expf(tn - stats[M + i]) * nw) +
                   sc * (expf(tp - stats[2 * M + j]) * pw - expf(tn - stats[3 * M + j]) * nw));
  if (j == i) g += w;
  if (j == ((const int*)stats)[5 * M + i]) g -= w;
  return g / d;
}

__global__ __launch_bounds__(256) void loss_bwd_tile_kernel(const float* __restrict__ a, const float* __restrict__ p,
                                                            int M, int C, const uint8_t* __restrict__ negm,
                                                            const float* __restrict__ sa, const float* __restrict__ sp,
                                                            LossParams P, const float* __restrict__ D,
                                                            const float* __restrict__ stats,
                                                            const float* __restrict__ g_desc, const float* __restrict__ g_det,
                                                            float* __restrict__ ga, float* __restrict__ gp,
                                                            float* __restrict__ gsa, float* __restrict__ gsp,
                                                            float w_desc, float w_det) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int L = kLossStrip;
  const int tid = threadIdx.x;
  const int CS = C + 1, RS = M + 1, KS = L + 1;
  float* al = lds;
  float* pl = al + (size_t)M * CS;
  float* Gr = pl + (size_t)M * CS;            // [L][RS]  rows of G = dL/dD / D
  float* Gc = Gr + (size_t)L * RS;            // [M][KS]  columns of G
  const int l0 = blockIdx.x * L, nl = min(L, M - l0);
  {  // blockIdx.y = fragment pair of a stacked batch
    const size_t pr = blockIdx.y;
    a += pr * M * C; p += pr * M * C; negm += pr * M * M; D += pr * M * M; stats += pr * 6 * M;
    sa += pr * M; sp += pr * M; ga += pr * M * C; gp += pr * M * C;
    if (gsa) gsa += pr * M;
    if (gsp) gsp += pr * M;
  }
  const float gd = (g_desc ? *g_desc : 0.0f) * w_desc, gt = (g_det ? *g_det : 0.0f) * w_det;
  const float invM = 1.0f / (float)M;
  for (int t = tid; t < M * C; t += 256) {
    al[(t / C) * CS + t % C] = a[t];
    pl[(t / C) * CS + t % C] = p[t];
  }
  for (int t = tid; t < nl * M; t += 256) {
    {
      const int r = t / M, j = t % M, i = l0 + r;
      const size_t e = (size_t)i * M + j;
      Gr[r * RS + j] = loss_grad_entry(D[e], negm[e] != 0, i, j, M, P, stats, gd * invM, gt * invM * (sa[i] + sp[i]));
    }
    {
      const int i = t / nl, cc = t % nl, j = l0 + cc;
      const size_t e = (size_t)i * M + j;
      Gc[i * KS + cc] = loss_grad_entry(D[e], negm[e] != 0, i, j, M, P, stats, gd * invM, gt * invM * (sa[i] + sp[i]));
    }
  }
  __syncthreads();
  for (int t = tid; t < nl * C; t += 256) {
    {
      const int r = t / C, c = t % C, i = l0 + r;
      const float ai = al[i * CS + c];
      float acc = 0.0f;
      for (int j = 0; j < M; ++j) acc += Gr[r * RS + j] * (ai - pl[j * CS + c]);
      ga[(size_t)i * C + c] = acc;
    }
    {
      const int cc = t / C, c = t % C, j = l0 + cc;
      const float pj = pl[j * CS + c];
      float acc = 0.0f;
      for (int i = 0; i < M; ++i) acc += Gc[i * KS + cc] * (pj - al[i * CS + c]);
      gp[(size_t)j * C + c] = acc;
    }
  }
  for (int r = tid; r < nl; r += 256) {
    const int i = l0 + r;
    const float v = gt * invM * (D[(size_t)i * M + i] - stats[4 * M + i]);
    if (gsa) gsa[i] = v;
    if (gsp) gsp[i] = v;
  }
}

// ---- batch-hard contrastive loss + detector loss (reference utils/loss.py:47-97 with metric 'euclidean', :149-158) ----
// Rows are independent: one wave per row i of a pair computes the row of D with the circle kernels' expression, adds 10
// where the keypoints are closer than safe_radius (reference :57-60, evaluated in f64 like its NumPy), and keeps the
// row's furthest positive (the diagonal), closest negative (lowest index on ties, like torch.min) and sum.
//   dists = D + 10*near,  near_ij = (dist_keypts_ij + (i == j ? 10 : 0)) < safe_radius
//   desc  = mean_i [max(fp_i - pos_margin, 0) + max(neg_margin - cn_i, 0)],  det = mean_i (fp_i - cn_i)(sa_i + sp_i)
// stats layout (floats, d3f_circle_det_loss_stats_floats(M) per pair): [0,M) D_ii  [M,2M) D_i,arg_i  [2M,3M) fp
// [4M,5M) cn  [5M,6M) arg_i (int).  The backward reads only these, the descriptors and the scores.
__global__ __launch_bounds__(256) void contrastive_fwd_kernel(const float* __restrict__ a, const float* __restrict__ p,
                                                              int M, int C, const double* __restrict__ dk,
                                                              double safe_radius, float* __restrict__ dists,
                                                              float* __restrict__ fp_out,
                                                              float* __restrict__ avgneg_out,
                                                              float* __restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= M) return;
  {  // blockIdx.y = fragment pair of a stacked batch: its own M x M problem
    const size_t pr = blockIdx.y;
    a += pr * M * C; p += pr * M * C; dk += pr * M * M; dists += pr * M * M;
    fp_out += pr * M; avgneg_out += pr * M; stats += pr * 6 * M;
  }
  const float* ai = a + (size_t)i * C;
  float sd = 0.0f, cm = INFINITY, cmd = 0.0f, dii = 0.0f, fpv = 0.0f;
  int ca = 0x7fffffff;
  for (int j = lane; j < M; j += 64) {
    const float* pj = p + (size_t)j * C;
    float acc = 0.0f;
    for (int c = 0; c < C; ++c) {
      const float df = ai[c] - pj[c];
      acc += df * df;
    }
    const float d = sqrtf(acc + 1e-12f);
    const bool near = (dk[(size_t)i * M + j] + (i == j ? 10.0 : 0.0)) < safe_radius;
    const float e = d + (near ? 10.0f : 0.0f);
    dists[(size_t)i * M + j] = e;
    sd += e;
    if (j == i) {
      dii = d;
      fpv = e;
    } else if (e < cm) {   // j ascending within the lane: the first minimum stays
      cm = e;
      ca = j;
      cmd = d;
    }
  }
  sd = d3f::wave_sum(sd);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {  // (value, index) lexicographic min -> first minimal index like torch.min
    const float ov = __shfl_xor(cm, o, 64);
    const int oa = __shfl_xor(ca, o, 64);
    const float od = __shfl_xor(cmd, o, 64);
    if (ov < cm || (ov == cm && oa < ca)) { cm = ov; ca = oa; cmd = od; }
  }
  if (ca >= M) {   // no ordered candidate (a row of NaN): NaN statistics, and an index the backward may read
    ca = i == 0 ? 1 : 0;
    cm = cmd = __builtin_nanf("");
  }
  const int owner = i & 63;   // the lane that met j == i
  dii = __shfl(dii, owner, 64);
  fpv = __shfl(fpv, owner, 64);
  if (lane == 0) {
    stats[i] = dii;
    stats[M + i] = cmd;
    stats[2 * M + i] = fpv;
    stats[3 * M + i] = 0.0f;
    stats[4 * M + i] = cm;
    ((int*)stats)[5 * M + i] = ca;
    fp_out[i] = fpv;
    avgneg_out[i] = (sd - fpv) / (float)(M - 1);
  }
}

// scalars of the contrastive + detector loss from the per-row statistics; pairs and total as loss_finalize_kernel
__global__ __launch_bounds__(256) void contrastive_finalize_kernel(int M, const float* __restrict__ sa,
                                                                   const float* __restrict__ sp, float pos_margin,
                                                                   float neg_margin, const float* __restrict__ avgneg_out,
                                                                   const float* __restrict__ stats,
                                                                   float* __restrict__ scalars, int pairs, float w_desc,
                                                                   float w_det, float* __restrict__ total) {
  __shared__ float sh[16];
  const int tid = threadIdx.x;
  float tot = 0.0f;
  for (int pr = 0; pr < pairs; ++pr, sa += M, sp += M, avgneg_out += M, stats += 6 * M, scalars += 6) {
    float l = 0.0f, dt = 0.0f, ac = 0.0f, fps = 0.0f, ans = 0.0f;
    for (int i = tid; i < M; i += blockDim.x) {
      const float fp = stats[2 * M + i], cn = stats[4 * M + i];
      l += fmaxf(fp - pos_margin, 0.0f) + fmaxf(neg_margin - cn, 0.0f);
      const float diff = fp - cn;
      dt += diff * (sa[i] + sp[i]);
      ac += diff < 0.0f ? 1.0f : 0.0f;
      fps += fp;
      ans += avgneg_out[i];
    }
    l = block_sum(l, sh);
    dt = block_sum(dt, sh);
    ac = block_sum(ac, sh);
    fps = block_sum(fps, sh);
    ans = block_sum(ans, sh);
    if (tid == 0) {
      scalars[0] = l / (float)M;
      scalars[1] = dt / (float)M;
      scalars[2] = ac * 100.0f / (float)M;
      scalars[3] = fps / (float)M;
      scalars[4] = ans / (float)M;
      scalars[5] = l / (float)M + dt / (float)M;
    }
    tot += w_desc * (l / (float)M) + w_det * (dt / (float)M);
  }
  if (tid == 0 && total) *total = tot;
}

// torch.max(x, 0) (elementwise, reference :93): the gradient is split in half where x == 0 exactly
__device__ __forceinline__ float hinge_grad(float x) { return x > 0.0f ? 1.0f : (x == 0.0f ? 0.5f : 0.0f); }

// d loss / d dists of row i, at (i, i) and at (i, arg_i): the only entries that reach the loss
__device__ __forceinline__ void contrastive_row_grads(const float* __restrict__ stats, int M, int i, float pos_margin,
                                                      float neg_margin, float gdM, float gtM, float s, float& g_fp,
                                                      float& g_cn) {
  const float fp = stats[2 * M + i], cn = stats[4 * M + i];
  g_fp = gdM * hinge_grad(fp - pos_margin) + gtM * s;
  g_cn = -gdM * hinge_grad(neg_margin - cn) - gtM * s;
}

// wave m2 < M: grad of anchor row i = m2 (+ both score gradients); wave m2 >= M: grad of positive row j = m2 - M, which
// collects its diagonal term and, in ascending i, every row whose closest negative it is (a fixed order: no atomics)
__global__ __launch_bounds__(256) void contrastive_bwd_kernel(const float* __restrict__ a, const float* __restrict__ p,
                                                              int M, int C, const float* __restrict__ sa,
                                                              const float* __restrict__ sp, float pos_margin,
                                                              float neg_margin, const float* __restrict__ stats,
                                                              const float* __restrict__ g_desc,
                                                              const float* __restrict__ g_det, float w_desc, float w_det,
                                                              float* __restrict__ ga, float* __restrict__ gp,
                                                              float* __restrict__ gsa, float* __restrict__ gsp) {
  const int lane = threadIdx.x & 63;
  const int m2 = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m2 >= 2 * M) return;
  {
    const size_t pr = blockIdx.y;
    a += pr * M * C; p += pr * M * C; stats += pr * 6 * M;
    sa += pr * M; sp += pr * M; ga += pr * M * C; gp += pr * M * C;
    if (gsa) gsa += pr * M;
    if (gsp) gsp += pr * M;
  }
  const float invM = 1.0f / (float)M;
  const float gdM = (g_desc ? *g_desc : 0.0f) * w_desc * invM, gtM = (g_det ? *g_det : 0.0f) * w_det * invM;
  const int* arg = (const int*)stats + 5 * M;
  if (m2 < M) {
    const int i = m2, k = arg[i];
    float g_fp, g_cn;
    contrastive_row_grads(stats, M, i, pos_margin, neg_margin, gdM, gtM, sa[i] + sp[i], g_fp, g_cn);
    const float wd = g_fp / stats[i], wn = g_cn / stats[M + i];
    for (int c = lane; c < C; c += 64) {
      const float ac = a[(size_t)i * C + c];
      ga[(size_t)i * C + c] = wd * (ac - p[(size_t)i * C + c]) + wn * (ac - p[(size_t)k * C + c]);
    }
    if (lane == 0) {
      const float v = gtM * (stats[2 * M + i] - stats[4 * M + i]);
      if (gsa) gsa[i] = v;
      if (gsp) gsp[i] = v;
    }
    return;
  }
  const int j = m2 - M;
  float acc[4];
  const int nc = (C + 63) / 64;
  {
    float g_fp, g_cn;
    contrastive_row_grads(stats, M, j, pos_margin, neg_margin, gdM, gtM, sa[j] + sp[j], g_fp, g_cn);
    const float wd = g_fp / stats[j];
    for (int q = 0; q < 4; ++q) {
      const int c = lane + 64 * q;
      acc[q] = (q < nc && c < C) ? wd * (p[(size_t)j * C + c] - a[(size_t)j * C + c]) : 0.0f;
    }
  }
  for (int base = 0; base < M; base += 64) {
    const int i0 = base + lane;
    unsigned long long hit = __ballot(i0 < M && arg[i0] == j);
    while (hit) {
      const int i = base + __builtin_ctzll(hit);
      hit &= hit - 1;
      float g_fp, g_cn;
      contrastive_row_grads(stats, M, i, pos_margin, neg_margin, gdM, gtM, sa[i] + sp[i], g_fp, g_cn);
      const float wn = g_cn / stats[M + i];
      for (int q = 0; q < 4; ++q) {
        const int c = lane + 64 * q;
        if (q < nc && c < C) acc[q] += wn * (p[(size_t)j * C + c] - a[(size_t)i * C + c]);
      }
    }
  }
  for (int q = 0; q < 4; ++q) {
    const int c = lane + 64 * q;
    if (q < nc && c < C) gp[(size_t)j * C + c] = acc[q];
  }
}

// ---- keypoint selection + L2 normalisation of the selected descriptors -------------------------------------------
// The reference normalises ALL N descriptors (architectures.py:318, F.normalize) and then indexes the M sampled
// correspondences out of them and out of the scores (trainer.py:91-94): ~10 PyTorch launches forward and ~15 backward
// (two zero-filled [N,C] scatter targets, their sum, the normalisation's backward over all N rows).  Training only
// ever looks at the 2M selected rows, so one launch gathers and normalises them and one scatters the gradient back.
//   out[m,:] = x[idx[m],:] / max(||x[idx[m],:]||, 1e-12)          (torch F.normalize semantics)
__global__ __launch_bounds__(256) void select_normalize_fwd_kernel(const float* __restrict__ x,
                                                                   const float* __restrict__ scores, int N, int C,
                                                                   d3f::SampledRows sr, float* __restrict__ out_a,
                                                                   float* __restrict__ out_p, float* __restrict__ sa,
                                                                   float* __restrict__ sp) {
  const int lane = threadIdx.x & 63;
  const int m2 = blockIdx.x * 4 + (threadIdx.x >> 6);  // 0..2M-1: anchors then positives
  if (m2 >= 2 * sr.M) return;
  const bool pos = m2 >= sr.M;
  const int m = pos ? m2 - sr.M : m2;
  const long row = d3f::sampled_row(sr, m2, N);
  float ss = 0.0f;
  for (int c = lane; c < C; c += 64) {
    const float v = x[row * C + c];
    ss += v * v;
  }
  ss = d3f::wave_sum(ss);
  const float denom = fmaxf(sqrtf(ss), 1e-12f);
  float* o = (pos ? out_p : out_a) + (size_t)m * C;
  for (int c = lane; c < C; c += 64) o[c] = x[row * C + c] / denom;
  if (lane == 0 && scores) (pos ? sp : sa)[m] = scores[row];   // no scores: the detector runs on the sampled rows itself
}

// grad_x[row,:] += g/n - y (y.g)/n  with y = x/n the normalised row (n > eps); grad_scores[row] += g_s
__global__ __launch_bounds__(256) void select_normalize_bwd_kernel(const float* __restrict__ x, int N, int C,
                                                                   d3f::SampledRows sr, const float* __restrict__ g_a,
                                                                   const float* __restrict__ g_p,
                                                                   const float* __restrict__ g_sa,
                                                                   const float* __restrict__ g_sp,
                                                                   float* __restrict__ grad_x,
                                                                   float* __restrict__ grad_s) {
  const int lane = threadIdx.x & 63;
  const int m2 = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m2 >= 2 * sr.M) return;
  const bool pos = m2 >= sr.M;
  const int m = pos ? m2 - sr.M : m2;
  const long row = d3f::sampled_row(sr, m2, N);
  const float* g = (pos ? g_p : g_a) + (size_t)m * C;
  float ss = 0.0f, dot = 0.0f;
  for (int c = lane; c < C; c += 64) {
    const float v = x[row * C + c];
    ss += v * v;
    dot += v * (g ? g[c] : 0.0f);
  }
  ss = d3f::wave_sum(ss);
  dot = d3f::wave_sum(dot);
  const float n = sqrtf(ss);
  if (g) {
    for (int c = lane; c < C; c += 64) {
      const float v = x[row * C + c];
      // n <= eps: the forward divided by the constant eps
      const float gv = n > 1e-12f ? (g[c] - v * dot / ss) / n : g[c] / 1e-12f;
      atomicAdd(&grad_x[row * C + c], gv);
    }
  }
  const float* gs = pos ? g_sp : g_sa;
  if (lane == 0 && gs && grad_s) atomicAdd(&grad_s[row], gs[m]);
}

}  // namespace

extern "C" {

size_t d3f_circle_det_loss_stats_floats(int M) { return 6 * (size_t)(M > 0 ? M : 1); }
size_t d3f_circle_det_loss_ws_bytes(int M) { return sizeof(float) * (size_t)(M > 0 ? M : 1) * (size_t)(M > 0 ? M : 1); }

// The one-workgroup kernels (!cache_ok) serve one pair and know neither weights nor a total.
int d3f_circle_det_loss_forward(const float* anchor, const float* positive, int M, int C, int pairs,
                                const uint8_t* neg_mask, const float* anc_score, const float* pos_score, float log_scale,
                                float safe_radius, float pos_margin, float neg_margin, float w_desc, float w_det,
                                float* dists, float* furthest_positive, float* average_negative, float* out_scalars,
                                float* out_total, float* stats, void* stream) {
  if (!anchor || !positive || !neg_mask || !anc_score || !pos_score || !dists || !furthest_positive ||
      !average_negative || !out_scalars || !stats || M < 2 || M > kMaxM || C < 1 || pairs < 1 || pairs > 32)
    return D3F_EINVAL;
  const LossParams P = {log_scale, safe_radius, pos_margin, neg_margin};
  if (cache_ok(M, C)) {
    loss_fwd_tile_kernel<<<dim3(d3f::cdiv(M, kLossStrip), pairs), 256, tiled_lds_bytes(M, C), (hipStream_t)stream>>>(
        anchor, positive, M, C, neg_mask, P, dists, furthest_positive, average_negative, stats);
    loss_finalize_kernel<<<1, 256, 0, (hipStream_t)stream>>>(M, anc_score, pos_score, P, furthest_positive,
                                                             average_negative, stats, out_scalars, pairs, w_desc, w_det,
                                                             out_total);
  } else {
    if (pairs != 1 || out_total || w_desc != 1.0f || w_det != 1.0f) return D3F_EINVAL;
    loss_fwd_kernel<<<1, kThreads, 0, (hipStream_t)stream>>>(anchor, positive, M, C, neg_mask, anc_score, pos_score, P,
                                                             dists, furthest_positive, average_negative, out_scalars,
                                                             stats);
  }
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_circle_det_loss_backward(const float* anchor, const float* positive, int M, int C, int pairs,
                                 const uint8_t* neg_mask, const float* anc_score, const float* pos_score, float log_scale,
                                 float safe_radius, float pos_margin, float neg_margin, float w_desc, float w_det,
                                 const float* dists, const float* stats, const float* grad_desc, const float* grad_det,
                                 float* grad_anchor, float* grad_positive, float* grad_anc_score, float* grad_pos_score,
                                 void* ws, size_t ws_bytes, void* stream) {
  if (!anchor || !positive || !neg_mask || !anc_score || !pos_score || !dists || !stats || !grad_anchor ||
      !grad_positive || M < 2 || M > kMaxM || C < 1 || pairs < 1 || pairs > 32)
    return D3F_EINVAL;
  const LossParams P = {log_scale, safe_radius, pos_margin, neg_margin};
  if (cache_ok(M, C)) {
    loss_bwd_tile_kernel<<<dim3(d3f::cdiv(M, kLossStrip), pairs), 256, tiled_lds_bytes(M, C), (hipStream_t)stream>>>(
        anchor, positive, M, C, neg_mask, anc_score, pos_score, P, dists, stats, grad_desc, grad_det, grad_anchor,
        grad_positive, grad_anc_score, grad_pos_score, w_desc, w_det);
  } else {
    if (pairs != 1 || w_desc != 1.0f || w_det != 1.0f || !ws) return D3F_EINVAL;
    if (ws_bytes < d3f_circle_det_loss_ws_bytes(M)) return D3F_EWORKSPACE;
    loss_bwd_kernel<<<1, kThreads, 0, (hipStream_t)stream>>>(anchor, positive, M, C, neg_mask, anc_score, pos_score, P,
                                                             dists, stats, grad_desc, grad_det, (float*)ws, grad_anchor,
                                                             grad_positive, grad_anc_score, grad_pos_score);
  }
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_contrastive_det_loss_forward(const float* anchor, const float* positive, int M, int C, int pairs,
                                     const double* dist_keypts, const float* anc_score, const float* pos_score,
                                     double safe_radius, float pos_margin, float neg_margin, float w_desc, float w_det,
                                     float* dists, float* furthest_positive, float* average_negative,
                                     float* out_scalars, float* out_total, float* stats, void* stream) {
  if (!anchor || !positive || !dist_keypts || !anc_score || !pos_score || !dists || !furthest_positive ||
      !average_negative || !out_scalars || !stats || M < 2 || M > kMaxM || C < 1 || C > 256 || pairs < 1 || pairs > 32)
    return D3F_EINVAL;
  contrastive_fwd_kernel<<<dim3(d3f::cdiv(M, 4), pairs), 256, 0, (hipStream_t)stream>>>(
      anchor, positive, M, C, dist_keypts, safe_radius, dists, furthest_positive, average_negative, stats);
  D3F_LAUNCH_CHECK();
  contrastive_finalize_kernel<<<1, 256, 0, (hipStream_t)stream>>>(M, anc_score, pos_score, pos_margin, neg_margin,
                                                                  average_negative, stats, out_scalars, pairs, w_desc,
                                                                  w_det, out_total);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_contrastive_det_loss_backward(const float* anchor, const float* positive, int M, int C, int pairs,
                                      const float* anc_score, const float* pos_score, float pos_margin, float neg_margin,
                                      float w_desc, float w_det, const float* stats, const float* grad_desc,
                                      const float* grad_det, float* grad_anchor, float* grad_positive,
                                      float* grad_anc_score, float* grad_pos_score, void* stream) {
  if (!anchor || !positive || !anc_score || !pos_score || !stats || !grad_anchor || !grad_positive || M < 2 ||
      M > kMaxM || C < 1 || C > 256 || pairs < 1 || pairs > 32)
    return D3F_EINVAL;
  contrastive_bwd_kernel<<<dim3(d3f::cdiv(2 * M, 4), pairs), 256, 0, (hipStream_t)stream>>>(
      anchor, positive, M, C, anc_score, pos_score, pos_margin, neg_margin, stats, grad_desc, grad_det, w_desc, w_det,
      grad_anchor, grad_positive, grad_anc_score, grad_pos_score);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

/* Sampled-correspondence front end of the loss -- replaces F.normalize over all N descriptors
 * (models/architectures.py:318) followed by the four index selections of trainer.py:91-94.  The rows are resolved by
 * d3f::make_sampled_rows (common.hpp); out_a/out_p [pairs*M,C] normalised descriptors, sa/sp [pairs*M] scores. */
int d3f_select_normalize_forward(const float* x, const float* scores, int N, int C, const int64_t* idx_a,
                                 const int64_t* idx_p, int idx_stride, int M, int pairs, const int32_t* p_offset,
                                 const int32_t* pair_len, float* out_a, float* out_p, float* sa, float* sp,
                                 void* stream) {
  d3f::SampledRows sr;
  if (!d3f::make_sampled_rows(idx_a, idx_p, idx_stride, M, pairs, p_offset, pair_len, sr) || !x || !out_a || !out_p ||
      (scores && (!sa || !sp)) || N < 1 || C < 1)
    return D3F_EINVAL;
  select_normalize_fwd_kernel<<<d3f::cdiv(2 * sr.M, 4), 256, 0, (hipStream_t)stream>>>(x, scores, N, C, sr, out_a,
                                                                                         out_p, sa, sp);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

/* grad_x [N,C] and grad_scores [N] must be ONE allocation of N*(C+1) floats starting at grad_x (cleared here with a
 * single fill); g_* may be NULL for outputs that received no gradient.  grad_scores NULL: only grad_x [N,C] is cleared
 * and written (the detector's rows form adds its own part to it, d3f_detection_rows_backward). */
int d3f_select_normalize_backward(const float* x, int N, int C, const int64_t* idx_a, const int64_t* idx_p,
                                  int idx_stride, int M, int pairs, const int32_t* p_offset, const int32_t* pair_len,
                                  const float* g_a, const float* g_p, const float* g_sa, const float* g_sp,
                                  float* grad_x, float* grad_scores, void* stream) {
  d3f::SampledRows sr;
  if (!d3f::make_sampled_rows(idx_a, idx_p, idx_stride, M, pairs, p_offset, pair_len, sr) || !x || !grad_x || N < 1 ||
      C < 1 || (grad_scores && grad_scores != grad_x + (size_t)N * C))
    return D3F_EINVAL;
  if (d3f::zero_async(grad_x, sizeof(float) * (size_t)N * (C + (grad_scores ? 1 : 0)), (hipStream_t)stream) != hipSuccess)
    return D3F_ELAUNCH;
  select_normalize_bwd_kernel<<<d3f::cdiv(2 * sr.M, 4), 256, 0, (hipStream_t)stream>>>(x, N, C, sr, g_a, g_p, g_sa,
                                                                                         g_sp, grad_x, grad_scores);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

}  // extern "C"
