// The rule of the ISS keypoint detector (Zhong 2009; Open3D's compute_iss_keypoints), stated once for the two kernels
// (iss.hip), the host twins (d3f_iss_saliency_from_moments_host, d3f_radius_nms_host) and the NumPy restatement
// (registration.iss_numpy).  include/d3feat_hip.h has the contract.  Everything here is __host__ __device__ and reads
// no state.
//
// Saliency.  The neighbourhood of point i at salient_radius, the scale Q and the ten int64 moments m[10] are those of
// d3f_estimate_normals (plane.hpp), so they do not depend on the order in which neighbours are met.  The covariance
// C = (S - s s^T / n) / n / Q^2 is formed in f64 exactly as normal_from_moments forms it and diagonalised by the same
// kJacobiSweeps3 sweeps of plane::jacobi3; no eigenvector is wanted.  With e1 >= e2 >= e3 the sorted diagonal, the
// point is salient when
//   n >= min_neighbors,  e1 > 0,  e2 < gamma_21 e1,  e3 < gamma_32 e2
// -- products, no division, so no 0 / 0 -- and its saliency is (float)e3 in squared length units; a point that is not
// salient, or whose e3 is not positive or rounds to 0.0f, gets 0.0f.
//
// Suppression (Open3D's IsLocalMaxima).  Row i of any f32 score is kept when score[i] > 0 (a NaN is not), no neighbour
// j within non_max_radius has score[j] > score[i], strictly -- equal scores both survive, which keeps the result
// independent of the row order -- and the neighbourhood, i included, holds at least min_neighbors points.  No
// arithmetic beyond the distance test.
#pragma once
#include "plane.hpp"

namespace d3f {
namespace iss {

// d3f::sqdist_exact for host and device: ((dx dx) + (dy dy)) + (dz dz) in f32 (-ffp-contract=off: no FMA)
D3F_HD inline float sqdist_f32(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return (dx * dx + dy * dy) + dz * dz;
}

// plane::jacobi3 on the matrix alone: the eigenvector columns it also turns are dead here and the compiler drops them
D3F_HD inline void rotate(double& app, double& aqq, double& apq, double& arp, double& arq) {
  double v0p = 0.0, v0q = 0.0, v1p = 0.0, v1q = 0.0, v2p = 0.0, v2q = 0.0;
  plane::jacobi3(app, aqq, apq, arp, arq, v0p, v0q, v1p, v1q, v2p, v2q);
}

D3F_HD inline float saliency_from_moments(const int64_t (&m)[10], double Q, double gamma_21, double gamma_32,
                                          int min_neighbors) {
  if (m[0] < 1 || m[0] < (int64_t)min_neighbors) return 0.0f;
  const double n = (double)m[0], sx = (double)m[1], sy = (double)m[2], sz = (double)m[3];
  const double w = 1.0 / (Q * Q);
  double a00 = ((double)m[4] - sx * sx / n) / n * w, a01 = ((double)m[5] - sx * sy / n) / n * w,
         a02 = ((double)m[6] - sx * sz / n) / n * w, a11 = ((double)m[7] - sy * sy / n) / n * w,
         a12 = ((double)m[8] - sy * sz / n) / n * w, a22 = ((double)m[9] - sz * sz / n) / n * w;
  for (int sweep = 0; sweep < plane::kJacobiSweeps3; ++sweep) {
    rotate(a00, a11, a01, a02, a12);   // (0, 1), third index 2
    rotate(a00, a22, a02, a01, a12);   // (0, 2), third index 1
    rotate(a11, a22, a12, a01, a02);   // (1, 2), third index 0
  }
  const double lo01 = a00 < a11 ? a00 : a11, hi01 = a00 < a11 ? a11 : a00;
  const double e1 = hi01 > a22 ? hi01 : a22, e3 = lo01 < a22 ? lo01 : a22;
  const double e2 = hi01 > a22 ? (lo01 > a22 ? lo01 : a22) : hi01;
  if (!(e1 > 0.0 && e2 < gamma_21 * e1 && e3 < gamma_32 * e2)) return 0.0f;
  const float s = (float)e3;
  return s > 0.0f ? s : 0.0f;
}

}  // namespace iss
}  // namespace d3f
