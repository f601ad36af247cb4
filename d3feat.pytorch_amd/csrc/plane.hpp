// The two small solvers of the point-to-plane refinement, shared by the kernels (normals.hip, icp.hip) and their
// host-side twins (d3f_normal_from_moments_host, d3f_icp_plane_fit_host).  Everything here is __host__ __device__, reads
// no state and is double precision.  No matrix is indexed by a run-time value: every loop over a matrix has constant
// bounds and is unrolled, so the kernels keep them in registers.
//
// Normal from moments (include/d3feat_hip.h has the contract).  m[10] = { n, sum u (3), sum u u^T (xx xy xz yy yz zz) }
// are the integer moments of the quantised neighbour offsets u = rint((p_j - p_i) Q).  C = (S - s s^T / n) / n, scaled
// by 1 / Q^2 (a power of two: exact) to squared length units; its eigenvectors come from kJacobiSweeps3 cyclic Jacobi
// sweeps (fixed count, no data-dependent exit).  The normal is the column of the smallest diagonal entry, the lowest
// index on ties, normalised; its sign makes n . to_view >= 0, and when that dot product is exactly 0 the first
// non-zero component positive.  n < 1 or a largest eigenvalue that is not positive gives (0, 0, 0).
//
// Point-to-plane step from sums (icp.hip).  sums[29] = { n, the 21 upper entries of sum J J^T row by row, sum J r (6),
// sum d2 } with J = [a x nrm, nrm], r = (a - c) . nrm, a = T_k x - py, c = y - py.  Cholesky of the 6x6; a pivot
// <= kPlanePivot * max_i A_ii is singular (the pose stays).  Else v = -A^-1 sum J r = (alpha, beta, gamma, t_d),
// R_d = Rz(gamma) Ry(beta) Rx(alpha), R_next = R_d R_k, t_next = R_d (t_k - py) + py + t_d.
#pragma once
#include <math.h>
#include <stdint.h>

#include "rigid.hpp"

namespace d3f {
namespace plane {

constexpr int kJacobiSweeps3 = 6;
constexpr double kPlanePivot = 1e-10;
constexpr int kPlaneSums = 29;

// Q = 2^floor(log2(2^20 / radius)) of the integer moments, on the host in double (ilogb is exact)
inline double quantum_scale(float radius) { return ldexp(1.0, ilogb(1048576.0 / (double)radius)); }

// one Jacobi rotation in the (p, q) plane of a symmetric 3x3 (r the third index): app, aqq, apq the 2x2 block, arp, arq
// the third row's entries, v?p / v?q the two columns of the accumulated eigenvectors
D3F_HD inline void jacobi3(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q,
                           double& v1p, double& v1q, double& v2p, double& v2q) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
  if (theta < 0.0) t = -t;
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  app -= t * apq;
  aqq += t * apq;
  apq = 0.0;
  const double rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
  const double a0 = v0p, b0 = v0q, a1 = v1p, b1 = v1q, a2 = v2p, b2 = v2q;
  v0p = c * a0 - s * b0; v0q = s * a0 + c * b0;
  v1p = c * a1 - s * b1; v1q = s * a1 + c * b1;
  v2p = c * a2 - s * b2; v2q = s * a2 + c * b2;
}

D3F_HD inline void normal_from_moments(const int64_t (&m)[10], double Q, double view_x, double view_y, double view_z,
                                       float& out_x, float& out_y, float& out_z) {
  out_x = 0.0f; out_y = 0.0f; out_z = 0.0f;
  if (m[0] < 1) return;
  const double n = (double)m[0], sx = (double)m[1], sy = (double)m[2], sz = (double)m[3];
  const double w = 1.0 / (Q * Q);
  double a00 = ((double)m[4] - sx * sx / n) / n * w, a01 = ((double)m[5] - sx * sy / n) / n * w,
         a02 = ((double)m[6] - sx * sz / n) / n * w, a11 = ((double)m[7] - sy * sy / n) / n * w,
         a12 = ((double)m[8] - sy * sz / n) / n * w, a22 = ((double)m[9] - sz * sz / n) / n * w;
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
  for (int sweep = 0; sweep < kJacobiSweeps3; ++sweep) {
    jacobi3(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);   // (0, 1), third index 2
    jacobi3(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);   // (0, 2), third index 1
    jacobi3(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);   // (1, 2), third index 0
  }
  const double top = a00 > a11 ? (a00 > a22 ? a00 : a22) : (a11 > a22 ? a11 : a22);
  if (!(top > 0.0)) return;
  const bool one = a11 < a00, two = a22 < (one ? a11 : a00);
  double x = two ? v02 : (one ? v01 : v00), y = two ? v12 : (one ? v11 : v10), z = two ? v22 : (one ? v21 : v20);
  const double nrm = sqrt((x * x + y * y) + z * z);
  x /= nrm; y /= nrm; z /= nrm;
  const double dot = (x * view_x + y * view_y) + z * view_z;
  bool flip = dot < 0.0;
  if (dot == 0.0) flip = x != 0.0 ? x < 0.0 : (y != 0.0 ? y < 0.0 : z < 0.0);
  if (flip) { x = -x; y = -y; z = -z; }
  out_x = (float)x; out_y = (float)y; out_z = (float)z;
}

// entry (i, j), i <= j, of the packed upper triangle of a 6x6, row by row
D3F_HD constexpr int upper6(int i, int j) { return i * 6 - i * (i - 1) / 2 + (j - i); }

// v = -A^-1 b for the symmetric 6x6 A given by its packed upper triangle (upper6) and the right-hand side b, by
// Cholesky; false (v untouched) when a pivot is <= kPlanePivot * max_i A_ii or not a number.  The point-to-plane step
// below and the fast-global-registration step (fgr.hpp) share it.
D3F_HD inline bool solve6(const double A[21], const double b[6], double v[6]) {
  double L[21], top = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double d = A[upper6(i, i)];
    top = d > top ? d : top;
  }
  const double floor_ = kPlanePivot * top;
  bool ok = true;
  // A = U^T U with U upper triangular, kept in the packed layout of the sums
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double d = A[upper6(i, i)];
#pragma unroll
    for (int k = 0; k < i; ++k) d -= L[upper6(k, i)] * L[upper6(k, i)];
    if (!(d > floor_)) ok = false;   // (NaN too)
    const double root = sqrt(ok ? d : 1.0);
    L[upper6(i, i)] = root;
#pragma unroll
    for (int j = i + 1; j < 6; ++j) {
      double s = A[upper6(i, j)];
#pragma unroll
      for (int k = 0; k < i; ++k) s -= L[upper6(k, i)] * L[upper6(k, j)];
      L[upper6(i, j)] = s / root;
    }
  }
  if (!ok) return false;
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {   // U^T y = -b
    double s = -b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= L[upper6(k, i)] * y[k];
    y[i] = s / L[upper6(i, i)];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {   // U v = y
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) s -= L[upper6(i, k)] * v[k];
    v[i] = s / L[upper6(i, i)];
  }
  return true;
}

// T_k [12] row-major 3x4 -> T_next [12]; false (T_next = T_k) when the system is singular
D3F_HD inline bool plane_step(const double sums[kPlaneSums], const double py[3], const double Tk[12], double Tn[12]) {
#pragma unroll
  for (int k = 0; k < 12; ++k) Tn[k] = Tk[k];
  double v[6];
  if (!solve6(sums + 1, sums + 22, v)) return false;
  const double ca = cos(v[0]), sa = sin(v[0]), cb = cos(v[1]), sb = sin(v[1]), cg = cos(v[2]), sg = sin(v[2]);
  const double D[9] = {cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa,
                       sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa,
                       -sb,     cb * sa,                cb * ca};
  const double u[3] = {Tk[3] - py[0], Tk[7] - py[1], Tk[11] - py[2]};
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) Tn[4 * r + c] = (D[3 * r] * Tk[c] + D[3 * r + 1] * Tk[4 + c]) + D[3 * r + 2] * Tk[8 + c];
    Tn[4 * r + 3] = (((D[3 * r] * u[0] + D[3 * r + 1] * u[1]) + D[3 * r + 2] * u[2]) + py[r]) + v[3 + r];
  }
  return true;
}

}  // namespace plane
}  // namespace d3f
