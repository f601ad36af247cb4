// The refinement that follows a winning hypothesis, shared by RANSAC (registration.hip) and the spatial-compatibility
// estimator (sc2.hip): refine_iters x { inliers under the f32 image of the current (R, t) -> f64 centroids and
// cross-covariance over them -> Horn fit }, then a final recount.  A refit needs >= 3 inliers, else the current
// transform is kept.  The summation order is fixed: worker s of kRefineThreads adds rows s, s + 256, ... ascending
// into its partial sums, and the partials are folded by the tree  red[s] += red[s + h],  h = 128, 64, ..., 1.
// refine (device: one workgroup of kRefineThreads threads) and refine_host (one CPU thread, the workers in turn) run
// the same f64 operations in the same order.
#pragma once
#include "rigid.hpp"

namespace d3f {
namespace rigid {

constexpr int kRefineThreads = 256;
constexpr int kRed = 16;   // doubles per thread in the refinement's LDS tree

D3F_HD inline void to_f32(const double R[9], const double t[3], float rt[12]) {
#pragma unroll
  for (int i = 0; i < 9; ++i) rt[i] = (float)R[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) rt[9 + i] = (float)t[i];
}

#if defined(__HIPCC__)
// sums v[0..n) over the workgroup in a fixed tree order; every thread gets the totals
template <int N>
__device__ __forceinline__ void block_sum(double (*red)[kRed], double v[N]) {
  const int tid = threadIdx.x;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) red[tid][k] = v[k];
  __syncthreads();
  for (int s = kRefineThreads / 2; s > 0; s >>= 1) {
    if (tid < s) {
#pragma unroll
      for (int k = 0; k < N; ++k) red[tid][k] += red[tid + s][k];
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = red[0][k];
}

// Refines (R, t) over rows [off, off + count) of src / tgt; returns the final inlier count.  Uniform over the
// workgroup: every thread holds the same (R, t) on entry and on return.
__device__ __forceinline__ int refine(const float* __restrict__ src, const float* __restrict__ tgt, int off, int count,
                                      float tau2, int refine_iters, double (*red)[kRed], double R[9], double t[3]) {
  const int tid = threadIdx.x;
  int fin = 0;
  for (int it = 0; it <= refine_iters; ++it) {
    float rt[12];
    to_f32(R, t, rt);
    // inlier count and f64 centroid sums over this thread's rows (ascending)
    double v[kRed];
#pragma unroll
    for (int k = 0; k < 7; ++k) v[k] = 0.0;
    for (int i = tid; i < count; i += kRefineThreads) {
      const size_t r = 3 * (size_t)(off + i);
      const float sx = src[r], sy = src[r + 1], sz = src[r + 2], gx = tgt[r], gy = tgt[r + 1], gz = tgt[r + 2];
      if (inlier_f32(rt, gx, gy, gz, sx, sy, sz, tau2)) {
        v[0] += 1.0;
        v[1] += sx; v[2] += sy; v[3] += sz;
        v[4] += gx; v[5] += gy; v[6] += gz;
      }
    }
    block_sum<7>(red, v);
    const int n_in = (int)v[0];
    fin = n_in;
    if (it == refine_iters || n_in < 3) break;
    const double cs[3] = {v[1] / n_in, v[2] / n_in, v[3] / n_in}, ct[3] = {v[4] / n_in, v[5] / n_in, v[6] / n_in};
    double S[kRed];
#pragma unroll
    for (int k = 0; k < 9; ++k) S[k] = 0.0;
    for (int i = tid; i < count; i += kRefineThreads) {
      const size_t r = 3 * (size_t)(off + i);
      const float sx = src[r], sy = src[r + 1], sz = src[r + 2], gx = tgt[r], gy = tgt[r + 1], gz = tgt[r + 2];
      if (inlier_f32(rt, gx, gy, gz, sx, sy, sz, tau2)) {
        const double ds[3] = {sx - cs[0], sy - cs[1], sz - cs[2]}, dg[3] = {gx - ct[0], gy - ct[1], gz - ct[2]};
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
          for (int b = 0; b < 3; ++b) S[3 * a + b] += dg[a] * ds[b];
      }
    }
    block_sum<9>(red, S);
    rotation_from_covariance(S, R);
    translation(R, cs, ct, t);
  }
  return fin;
}
#endif

// The same loop on one CPU thread: the 256 workers in turn, then the same tree.
template <int N>
inline void tree_sum_host(double (*red)[kRed], double v[N]) {
  for (int s = kRefineThreads / 2; s > 0; s >>= 1)
    for (int w = 0; w < s; ++w)
      for (int k = 0; k < N; ++k) red[w][k] += red[w + s][k];
  for (int k = 0; k < N; ++k) v[k] = red[0][k];
}

inline int refine_host(const float* src, const float* tgt, int off, int count, float tau2, int refine_iters, double R[9],
                       double t[3]) {
  static thread_local double red[kRefineThreads][kRed];
  int fin = 0;
  for (int it = 0; it <= refine_iters; ++it) {
    float rt[12];
    to_f32(R, t, rt);
    for (int w = 0; w < kRefineThreads; ++w) {
      double* v = red[w];
      for (int k = 0; k < 7; ++k) v[k] = 0.0;
      for (int i = w; i < count; i += kRefineThreads) {
        const size_t r = 3 * (size_t)(off + i);
        const float sx = src[r], sy = src[r + 1], sz = src[r + 2], gx = tgt[r], gy = tgt[r + 1], gz = tgt[r + 2];
        if (inlier_f32(rt, gx, gy, gz, sx, sy, sz, tau2)) {
          v[0] += 1.0;
          v[1] += sx; v[2] += sy; v[3] += sz;
          v[4] += gx; v[5] += gy; v[6] += gz;
        }
      }
    }
    double v[7];
    tree_sum_host<7>(red, v);
    const int n_in = (int)v[0];
    fin = n_in;
    if (it == refine_iters || n_in < 3) break;
    const double cs[3] = {v[1] / n_in, v[2] / n_in, v[3] / n_in}, ct[3] = {v[4] / n_in, v[5] / n_in, v[6] / n_in};
    for (int w = 0; w < kRefineThreads; ++w) {
      double* S = red[w];
      for (int k = 0; k < 9; ++k) S[k] = 0.0;
      for (int i = w; i < count; i += kRefineThreads) {
        const size_t r = 3 * (size_t)(off + i);
        const float sx = src[r], sy = src[r + 1], sz = src[r + 2], gx = tgt[r], gy = tgt[r + 1], gz = tgt[r + 2];
        if (inlier_f32(rt, gx, gy, gz, sx, sy, sz, tau2)) {
          const double ds[3] = {sx - cs[0], sy - cs[1], sz - cs[2]}, dg[3] = {gx - ct[0], gy - ct[1], gz - ct[2]};
          for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) S[3 * a + b] += dg[a] * ds[b];
        }
      }
    }
    double S[9];
    tree_sum_host<9>(red, S);
    rotation_from_covariance(S, R);
    translation(R, cs, ct, t);
  }
  return fin;
}

}  // namespace rigid
}  // namespace d3f
