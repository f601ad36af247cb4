// Rigid-registration building blocks shared by the RANSAC kernels (registration.hip) and their host-side twins
// (d3f_ransac_sample_host, d3f_rigid_fit_host): the counter-based correspondence sampler and the least-squares rigid
// fit.  Everything here is __host__ __device__ and reads no state, so a test can restate it bit for bit on the CPU.
//
// Sampler.  splitmix64(x):  x += 0x9E3779B97F4A7C15;  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9;
//                           x = (x ^ (x >> 27)) * 0x94D049BB133111EB;  return x ^ (x >> 31)      (all mod 2^64)
//   pair key   K_p  = splitmix64(splitmix64(seed) ^ p)                   p = pair index (first_pair + row of seg)
//   draw k of hypothesis h (k = 0, 1, 2):
//              z    = splitmix64(K_p ^ (4 h + k))
//              idx  = ((z >> 32) * count) >> 32                           in [0, count) for count >= 1
//
// Rigid fit (Horn 1987, closed form with unit quaternions).  For pairs (src_i, tgt_i) the fit minimises
// sum |R tgt_i + t - src_i|^2 over proper rotations R: centroids cs, ct; S[3a+b] = sum (tgt_i - ct)_a (src_i - cs)_b;
// q = the eigenvector of the largest eigenvalue of Horn's symmetric 4x4 matrix N(S), found by kJacobiSweeps cyclic
// Jacobi sweeps (fixed count, no data-dependent exit); R = R(q), t = cs - R ct.  A unit quaternion always gives
// det R = +1, so no reflection patch-up is needed.  Everything is double precision.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define D3F_HD __host__ __device__
#else
#define D3F_HD
#endif

namespace d3f {
namespace rigid {

constexpr int kJacobiSweeps = 6;   // cyclic Jacobi converges quadratically; a fixed count keeps the work data-independent

D3F_HD inline uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

D3F_HD inline uint64_t pair_key(uint64_t seed, int p) { return splitmix64(splitmix64(seed) ^ (uint64_t)(uint32_t)p); }

D3F_HD inline int draw(uint64_t key, int h, int k, int count) {
  const uint64_t z = splitmix64(key ^ (((uint64_t)(uint32_t)h << 2) | (uint64_t)k));
  return (int)(((z >> 32) * (uint64_t)(uint32_t)count) >> 32);
}

// Largest-eigenvalue eigenvector of the symmetric 4x4 matrix A (destroyed) -> q[4] (unit length up to rounding).
D3F_HD inline void top_eigenvector4(double A[4][4], double q[4]) {
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
#pragma unroll
    for (int p = 0; p < 3; ++p) {
#pragma unroll
      for (int r = p + 1; r < 4; ++r) {
        const double apr = A[p][r];
        if (apr == 0.0) continue;
        const double theta = (A[r][r] - A[p][p]) / (2.0 * apr);
        double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
        if (theta < 0.0) t = -t;
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
        for (int k = 0; k < 4; ++k) {   // A <- A J (columns p, r)
          const double akp = A[k][p], akr = A[k][r];
          A[k][p] = c * akp - s * akr;
          A[k][r] = s * akp + c * akr;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {   // A <- J^T A (rows p, r)
          const double apk = A[p][k], ark = A[r][k];
          A[p][k] = c * apk - s * ark;
          A[r][k] = s * apk + c * ark;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {   // V <- V J
          const double vkp = V[k][p], vkr = V[k][r];
          V[k][p] = c * vkp - s * vkr;
          V[k][r] = s * vkp + c * vkr;
        }
      }
    }
  }
  int best = 0;   // largest diagonal entry, lowest index on ties
#pragma unroll
  for (int i = 1; i < 4; ++i)
    if (A[i][i] > A[best][best]) best = i;
#pragma unroll
  for (int i = 0; i < 4; ++i) q[i] = V[i][best];
}

// R (row-major 3x3) of the rotation that best maps the centred target points onto the centred source points, from the
// cross-covariance S[3a+b] = sum tgt'_a src'_b.
D3F_HD inline void rotation_from_covariance(const double S[9], double R[9]) {
  const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7],
               Szz = S[8];
  double N[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                    {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                    {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                    {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
  double q[4];
  top_eigenvector4(N, q);
  const double nrm = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  const double w = q[0] / nrm, x = q[1] / nrm, y = q[2] / nrm, z = q[3] / nrm;
  R[0] = w * w + x * x - y * y - z * z; R[1] = 2.0 * (x * y - w * z);         R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z);         R[4] = w * w - x * x + y * y - z * z; R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y);         R[7] = 2.0 * (y * z + w * x);         R[8] = w * w - x * x - y * y + z * z;
}

// t = cs - R ct
D3F_HD inline void translation(const double R[9], const double cs[3], const double ct[3], double t[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) t[a] = cs[a] - (R[3 * a] * ct[0] + R[3 * a + 1] * ct[1] + R[3 * a + 2] * ct[2]);
}

// Least-squares fit of n >= 1 pairs given as xyz triples (double), src ~ R tgt + t.  Sums in index order.
D3F_HD inline void fit(const double* src, const double* tgt, int n, double R[9], double t[3]) {
  double cs[3] = {0, 0, 0}, ct[3] = {0, 0, 0}, S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) {
      cs[a] += src[3 * i + a];
      ct[a] += tgt[3 * i + a];
    }
  for (int a = 0; a < 3; ++a) {
    cs[a] /= n;
    ct[a] /= n;
  }
  for (int i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) S[3 * a + b] += (tgt[3 * i + a] - ct[a]) * (src[3 * i + b] - cs[b]);
  rotation_from_covariance(S, R);
  translation(R, cs, ct, t);
}

// The ICP step's fit from sums over the accepted correspondences (icp.hip; d3f_icp_fit_host): y ~ R x + t for moving
// points x and fixed points y, given about pivots px, py as
//   sums[17] = { n, sum x' (3), sum y' (3), sum x'_a y'_b (9, row-major in a), sum d2 }   x' = x - px, y' = y - py.
// Centroids cx = sum x' / n, cy = sum y' / n; S[3a+b] = sum x'_a y'_b - n cx_a cy_b is the cross-covariance of the
// centred points, handed to rotation_from_covariance with the moving cloud in its "target" role and the fixed cloud in
// its "source" role; t = (cy + py) - R (cx + px).  n >= 1.
D3F_HD inline void fit_from_sums(const double sums[17], const double px[3], const double py[3], double R[9],
                                 double t[3]) {
  const double n = sums[0];
  double cx[3], cy[3], S[9], cs[3], ct[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    cx[a] = sums[1 + a] / n;
    cy[a] = sums[4 + a] / n;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) S[3 * a + b] = sums[7 + 3 * a + b] - n * cx[a] * cy[b];
  rotation_from_covariance(S, R);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    cs[a] = cy[a] + py[a];
    ct[a] = cx[a] + px[a];
  }
  translation(R, cs, ct, t);
}

// Minimal-set checks of a drawn triple (points as doubles, exact images of the f32 inputs):
//   distinct indices; both triangles non-degenerate: |(b - a) x (c - a)|^2 >= kMinCross2;
//   edge_ratio > 0: for each of the 3 edges, with squared lengths la2 (source) and lb2 (target),
//   min(la2, lb2) >= edge_ratio^2 * max(la2, lb2)   (Open3D's edge-length checker, squared).
constexpr double kMinCross2 = 1e-12;   // |cross| >= 1e-6 (squared length units): twice the triangle area

D3F_HD inline double cross_norm2(const double* a, const double* b, const double* c) {
  const double u0 = b[0] - a[0], u1 = b[1] - a[1], u2 = b[2] - a[2];
  const double v0 = c[0] - a[0], v1 = c[1] - a[1], v2 = c[2] - a[2];
  const double x = u1 * v2 - u2 * v1, y = u2 * v0 - u0 * v2, z = u0 * v1 - u1 * v0;
  return x * x + y * y + z * z;
}

D3F_HD inline double dist2(const double* a, const double* b) {
  const double d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
  return d0 * d0 + d1 * d1 + d2 * d2;
}

// s, t: the triple's source / target points as 3 consecutive xyz each
D3F_HD inline bool triple_ok(const double s[9], const double t[9], double edge_ratio) {
  if (cross_norm2(s, s + 3, s + 6) < kMinCross2 || cross_norm2(t, t + 3, t + 6) < kMinCross2) return false;
  if (edge_ratio > 0.0) {
    const double r2 = edge_ratio * edge_ratio;
    for (int e = 0; e < 3; ++e) {
      const int i = e, j = (e + 1) % 3;
      const double la2 = dist2(s + 3 * i, s + 3 * j), lb2 = dist2(t + 3 * i, t + 3 * j);
      const double lo = la2 < lb2 ? la2 : lb2, hi = la2 < lb2 ? lb2 : la2;
      if (!(lo >= r2 * hi)) return false;
    }
  }
  return true;
}

// The inlier test, f32 with this exact evaluation order (no contraction beyond the explicit fmaf):
//   e_a = fmaf(R[a][0], x, fmaf(R[a][1], y, fmaf(R[a][2], z, t[a]))) - src_a      (a = 0, 1, 2)
//   d2  = fmaf(e_2, e_2, fmaf(e_1, e_1, e_0 * e_0));      inlier  <=>  d2 < tau2
D3F_HD inline bool inlier_f32(const float* rt, float x, float y, float z, float sx, float sy, float sz, float tau2) {
  const float e0 = fmaf(rt[0], x, fmaf(rt[1], y, fmaf(rt[2], z, rt[9]))) - sx;
  const float e1 = fmaf(rt[3], x, fmaf(rt[4], y, fmaf(rt[5], z, rt[10]))) - sy;
  const float e2 = fmaf(rt[6], x, fmaf(rt[7], y, fmaf(rt[8], z, rt[11]))) - sz;
  const float d2 = fmaf(e2, e2, fmaf(e1, e1, e0 * e0));
  return d2 < tau2;
}

}  // namespace rigid
}  // namespace d3f
