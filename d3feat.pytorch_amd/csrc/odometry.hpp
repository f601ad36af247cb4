// Depth odometry: the relative pose of two depth frames by projective point-to-plane ICP over a depth pyramid
// (odometry.hip; d3f_depth_pyramid, d3f_depth_odometry_step, d3f_depth_odometry and their host twins).  KinectFusion's
// tracker, frame to frame.  Everything here is __host__ __device__ and reads no state: the kernels and the host twins
// run this text, and ops.depth_pyramid_numpy / depth_odometry_step_numpy / depth_odometry_numpy restate it.  f32
// arithmetic runs in exactly the order written (the library is built with -ffp-contract=off; f32 division and sqrtf
// are correctly rounded on both sides); f64 is used only where stated.
//
// Frames: depth [F,H,W] uint16 raw units or f32 metres, K [F,4] = fx, fy, cx, cy, depth_scale and depth_max as in
// tsdf.hpp.  A pixel is VALID when d > 0 and not d > depth_max (back_project's test): a NaN or an infinity is invalid.
//
// Pyramid, levels >= 1.  Level 0 is the depth in metres as f32, 0 where invalid.  Level l+1 has H >> 1 by W >> 1 pixels
// (an odd last row or column is dropped); its pixel (u, v) looks at the 2x2 block (2u..2u+1, 2v..2v+1) of level l in
// raster order: with k valid (> 0) pixels it is their sequential f32 sum divided by (float)k, and 0 when k = 0 or when
// the maximum minus the minimum of the valid ones exceeds depth_diff.  Intrinsics of level l+1: fx/2, fy/2,
// (cx - 0.5)/2, (cy - 0.5)/2 in f32.  Only the pyramid is stored (4 bytes per pixel); vertices and normals are
// recomputed from the depth where they are needed.
//
// Vertex V(u,v) = (((f32(u) - cx) d) / fx, ((f32(v) - cy) d) / fy, d): back_project's X, Y with an identity C.
// Normal at (u,v): exists when 1 <= u <= W-2, 1 <= v <= H-2, the centre and its four axis neighbours are valid and every
// neighbour has |d_nb - d_c| <= depth_diff.  e1 = V(u+1,v) - V(u-1,v), e2 = V(u,v+1) - V(u,v-1), c = e1 x e2 with each
// component (e1_i e2_j - e1_j e2_i), len = sqrtf((c0 c0 + c1 c1) + c2 c2); none when len is 0 or not finite;
// n = c / len, negated when (n0 V0 + n1 V1) + n2 V2 > 0 (it faces the camera).
//
// Pair p = (moving frame a, fixed frame b), T maps a's camera frame into b's (ops.icp_rigid's convention).  One
// association at level l under T: M = T rounded to f32 [12]; for every valid pixel of a's level l, x = V_a(u,v),
// a_r = ((M[r][0] x0 + M[r][1] x1) + M[r][2] x2) + M[r][3]; skip unless a_2 > 0; u' = floorf(((fx a_0) / a_2 + cx) +
// 0.5f), v' likewise, compared as floats against W and H before any conversion (integrate_frame's test); skip unless
// b's pixel (u', v') is valid and has a normal; y = V_b(u',v'); accept when ((a-y)_0^2 + (a-y)_1^2) + (a-y)_2^2 <=
// max_distance^2 in f32.  An accepted pixel adds, in f64 from the f32 values a, y, n, the 29 sums of plane.hpp
// { n, sum J J^T upper, sum J r, sum d2 } with J = [a x n, n], r = (a - y) . n, pivot py = 0 (camera-frame points are
// metres from the origin).  The fit is plane::plane_step; fewer than kMinPixels accepted pixels, or a singular system,
// leave T unchanged.
#pragma once
#include "plane.hpp"
#include "tsdf.hpp"

namespace d3f {
namespace odo {

constexpr int kMaxLevels = 8;
constexpr int kMinPixels = 6;
constexpr int kSums = plane::kPlaneSums;

// level dimensions and the pixel offset of a level inside one frame's packed pyramid
D3F_HD inline int level_h(int H, int l) { return H >> l; }
D3F_HD inline int level_w(int W, int l) { return W >> l; }
D3F_HD inline int64_t level_offset(int H, int W, int l) {
  int64_t off = 0;
  for (int k = 0; k < l; ++k) off += (int64_t)(H >> k) * (int64_t)(W >> k);
  return off;
}

D3F_HD inline bool valid(float d) { return d > 0.0f; }   // of a pyramid pixel: invalid ones were stored as 0

// level 0: metres, 0 where invalid
template <typename DepthT>
D3F_HD inline float level0_pixel(const DepthT* image, size_t i, float depth_scale, float depth_max) {
  const float d = tsdf::depth_value(image, i, depth_scale);
  return (!(d > 0.0f) || d > depth_max) ? 0.0f : d;
}

// pixel (u, v) of the next level from the level `src` of width Ws
D3F_HD inline float down_pixel(const float* src, int Ws, int u, int v, float depth_diff) {
  float sum = 0.0f, lo = 0.0f, hi = 0.0f;
  int k = 0;
  for (int dy = 0; dy < 2; ++dy)
    for (int dx = 0; dx < 2; ++dx) {
      const float d = src[(size_t)(2 * v + dy) * (size_t)Ws + (size_t)(2 * u + dx)];
      if (!valid(d)) continue;
      sum = sum + d;
      lo = (k == 0 || d < lo) ? d : lo;
      hi = (k == 0 || d > hi) ? d : hi;
      ++k;
    }
  if (k == 0 || hi - lo > depth_diff) return 0.0f;
  return sum / (float)k;
}

// intrinsics of the next level
D3F_HD inline void down_intrinsics(const float* K, float* out) {
  out[0] = K[0] / 2.0f;
  out[1] = K[1] / 2.0f;
  out[2] = (K[2] - 0.5f) / 2.0f;
  out[3] = (K[3] - 0.5f) / 2.0f;
}

D3F_HD inline void vertex(int u, int v, float d, const float* K, float* V) {
  V[0] = (((float)u - K[2]) * d) / K[0];
  V[1] = (((float)v - K[3]) * d) / K[1];
  V[2] = d;
}

// the normal n and the vertex V of pixel (u, v) of a level image H x W; false: there is none
D3F_HD inline bool normal_at(const float* img, int H, int W, int u, int v, const float* K, float depth_diff, float* n,
                             float* V) {
  if (!(u >= 1 && u <= W - 2 && v >= 1 && v <= H - 2)) return false;
  const size_t i = (size_t)v * (size_t)W + (size_t)u;
  const float dc = img[i], dl = img[i - 1], dr = img[i + 1], du = img[i - (size_t)W], dd = img[i + (size_t)W];
  if (!(valid(dc) && valid(dl) && valid(dr) && valid(du) && valid(dd))) return false;
  if (!(fabsf(dl - dc) <= depth_diff && fabsf(dr - dc) <= depth_diff && fabsf(du - dc) <= depth_diff &&
        fabsf(dd - dc) <= depth_diff))
    return false;
  float R[3], L[3], D[3], U[3];
  vertex(u + 1, v, dr, K, R);
  vertex(u - 1, v, dl, K, L);
  vertex(u, v + 1, dd, K, D);
  vertex(u, v - 1, du, K, U);
  const float e1[3] = {R[0] - L[0], R[1] - L[1], R[2] - L[2]};
  const float e2[3] = {D[0] - U[0], D[1] - U[1], D[2] - U[2]};
  const float c0 = e1[1] * e2[2] - e1[2] * e2[1];
  const float c1 = e1[2] * e2[0] - e1[0] * e2[2];
  const float c2 = e1[0] * e2[1] - e1[1] * e2[0];
  const float len = sqrtf((c0 * c0 + c1 * c1) + c2 * c2);
  if (!(len > 0.0f) || !(len <= 3.402823466e+38f)) return false;   // 0, NaN or infinite
  vertex(u, v, dc, K, V);
  n[0] = c0 / len;
  n[1] = c1 / len;
  n[2] = c2 / len;
  if ((n[0] * V[0] + n[1] * V[1]) + n[2] * V[2] > 0.0f) {
    n[0] = -n[0];
    n[1] = -n[1];
    n[2] = -n[2];
  }
  return true;
}

// One level of one pair: A the moving image with Ka, B the fixed image with Kb (both H x W), M [12] = T in f32.
struct PairLevel {
  const float* A;
  const float* B;
  const float* Ka;
  const float* Kb;
  int H, W;
  float M[12];
  float depth_diff, max_d2;
};

// the association of the moving pixel i = v W + u: the raster index of the accepted fixed pixel, or -1; a, y, n as above
D3F_HD inline int associate(const PairLevel& L, int u, int v, float* a, float* y, float* n) {
  const float d = L.A[(size_t)v * (size_t)L.W + (size_t)u];
  if (!valid(d)) return -1;
  float x[3];
  vertex(u, v, d, L.Ka, x);
  for (int r = 0; r < 3; ++r)
    a[r] = ((L.M[4 * r] * x[0] + L.M[4 * r + 1] * x[1]) + L.M[4 * r + 2] * x[2]) + L.M[4 * r + 3];
  if (!(a[2] > 0.0f)) return -1;
  const float up = floorf(((L.Kb[0] * a[0]) / a[2] + L.Kb[2]) + 0.5f);
  const float vp = floorf(((L.Kb[1] * a[1]) / a[2] + L.Kb[3]) + 0.5f);
  if (!(up >= 0.0f && up < (float)L.W && vp >= 0.0f && vp < (float)L.H)) return -1;
  const int ub = (int)up, vb = (int)vp;
  if (!normal_at(L.B, L.H, L.W, ub, vb, L.Kb, L.depth_diff, n, y)) return -1;
  const float e0 = a[0] - y[0], e1 = a[1] - y[1], e2 = a[2] - y[2];
  if (!((e0 * e0 + e1 * e1) + e2 * e2 <= L.max_d2)) return -1;
  return vb * L.W + ub;
}

// what an accepted pixel adds to the 29 sums: f64 from the f32 values
D3F_HD inline void add_pixel(double* acc, const float* af, const float* yf, const float* nf) {
  const double a[3] = {(double)af[0], (double)af[1], (double)af[2]};
  const double nrm[3] = {(double)nf[0], (double)nf[1], (double)nf[2]};
  const double e[3] = {a[0] - (double)yf[0], a[1] - (double)yf[1], a[2] - (double)yf[2]};
  const double J[6] = {a[1] * nrm[2] - a[2] * nrm[1], a[2] * nrm[0] - a[0] * nrm[2], a[0] * nrm[1] - a[1] * nrm[0],
                       nrm[0], nrm[1], nrm[2]};
  const double r = (e[0] * nrm[0] + e[1] * nrm[1]) + e[2] * nrm[2];
  acc[0] += 1.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = i; j < 6; ++j) acc[1 + plane::upper6(i, j)] += J[i] * J[j];
    acc[22 + i] += J[i] * r;
  }
  acc[kSums - 1] += (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
}

// T_k [12] -> T_next [12] from the sums of one association; false (T_next = T_k): too few pixels or singular.
// *singular says which.
D3F_HD inline bool fit(const double* sums, const double* Tk, double* Tn, bool* singular) {
  *singular = false;
  if (sums[0] < (double)kMinPixels) {
    for (int k = 0; k < 12; ++k) Tn[k] = Tk[k];
    return false;
  }
  const double py[3] = {0.0, 0.0, 0.0};
  const bool ok = plane::plane_step(sums, py, Tk, Tn);
  *singular = !ok;
  return ok;
}

// the 6x6 information matrix (rotation first, in the fixed frame) from the sums: sum J J^T
D3F_HD inline void information(const double* sums, double* out36) {
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) out36[6 * i + j] = sums[1 + (i <= j ? plane::upper6(i, j) : plane::upper6(j, i))];
}

}  // namespace odo
}  // namespace d3f
