// Coloured ICP (Park, Zhou, Koltun 2017; Open3D's registration_colored_icp): the rule, stated once, for the gradient
// kernel (normals.hip, kColor), the coloured search and fit (icp.hip, kColor) and the host twin
// (d3f_color_gradient_from_moments_host).  include/d3feat_hip.h has the contract; registration.py restates it in NumPy.
//
// Intensity.  One f32 per point beside the points; USABLE when 0 <= I <= 1 compared as floats, anything else (NaN
// included) means "no colour".  q = (int64) rint((double) I * 2^20), 0 <= q <= 2^20.
//
// Colour gradient from moments.  m[13] = the ten integer moments of normals.hip over the point's neighbours WITH A
// USABLE INTENSITY (n, sum u (3), sum u u^T: xx xy xz yy yz zz; u = rint((p_j - p_i) Q)), then sum u_x c, sum u_y c,
// sum u_z c with c = q_j - q_i.  |u| <= 2^20 and |c| <= 2^20: a product is below 2^40, 2^22 neighbours fit an int64, and
// integer addition commutes -- so, as for the normals, neither lanes, bucket order, stacking nor cell size can change
// the moments, and everything below is a function of them and of the f32 normal nrm alone, in f64:
//   S  = sum u u^T / Q^2       (about the point itself, NOT centred: the fitted intensity passes through I_i)
//   h  = sum u c / (Q 2^20)
//   e1 = normalise(nrm x axis), axis the unit vector of nrm's component of the smallest magnitude (lowest index on
//        ties); e2 = nrm x e1;  E = [e1 e2]
//   G  = E^T S E (2x2), g2 = E^T h;  d = E G^-1 g2 by the closed form of the 2x2, so d . nrm = 0 to rounding:
//        the least-squares slope of the intensity over the neighbourhood, on the tangent plane, in intensity per metre.
// Invalid (three NaNs): the point's own intensity is not usable, n < min_neighbors, nrm is zero (or not finite), or
// det G <= kGradientPivot max(G00, G11)^2 (neighbours on one line).  field = (d_x, d_y, d_z, I) in f32, .w NaN when the
// intensity is not usable: one 16-byte read per matched row in the ICP kernel, and a finiteness test drops what must
// be dropped.
//
// The coloured fit (icp.hip).  Per accepted row a, c, J = [a x nrm, nrm], r = (a - c) . nrm are point-to-plane's
// (plane.hpp); J and r are multiplied by sg = sqrt(lambda_geometric) before any product is formed.  When field[y] of the
// matched FIXED point is finite in all four entries and field[x].w of the moving point is finite, the row
//   J_C = sc [a x d, d],  r_C = sc ((I_y - I_x) + (a - c) . d),  sc = sqrt(1 - lambda_geometric)
// goes into the same 21 + 6 sums (a second rank-1 update after the geometric one).
// sums[31] = { the 29 of plane.hpp over both kinds of rows, n_color, sum ((I_y - I_x) + (a - c) . d)^2 unweighted };
// the fit is plane::plane_step on the first 29.  lambda_geometric = 1: sg is exactly 1 and the colour rows add +-0 to
// accumulators that start at +0, so the result is d3f_icp_rigid_plane's bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#include "plane.hpp"

namespace d3f {
namespace color {

constexpr int kGradientMoments = 13;
constexpr int kColorSums = plane::kPlaneSums + 2;   // ..., n_color, sum r_C^2 (unweighted)
constexpr double kGradientPivot = 1e-6;
constexpr double kIntensityScale = 1048576.0;       // 2^20

D3F_HD inline bool usable(float I) { return I >= 0.0f && I <= 1.0f; }   // false for NaN

D3F_HD inline int64_t quantised(float I) { return (int64_t)rint((double)I * kIntensityScale); }

// out[4] = (d, I); the rule of the header.  `intensity` is the point's own.
D3F_HD inline void gradient_from_moments(const int64_t (&m)[kGradientMoments], double Q, float nrm_x, float nrm_y,
                                         float nrm_z, float intensity, int min_neighbors, float (&out)[4]) {
  const float nan = __builtin_nanf("");
  out[0] = nan; out[1] = nan; out[2] = nan;
  out[3] = usable(intensity) ? intensity : nan;
  if (!usable(intensity) || m[0] < (int64_t)min_neighbors) return;
  const double nx = (double)nrm_x, ny = (double)nrm_y, nz = (double)nrm_z;
  const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
  if (!(ax + ay + az > 0.0)) return;   // zero (or NaN) normal
  // e1 = nrm x axis: axis = x -> (0, nz, -ny); y -> (-nz, 0, nx); z -> (ny, -nx, 0)
  const bool use_y = ay < ax, use_z = az < (use_y ? ay : ax);
  double e1x = use_z ? ny : (use_y ? -nz : 0.0), e1y = use_z ? -nx : (use_y ? 0.0 : nz),
         e1z = use_z ? 0.0 : (use_y ? nx : -ny);
  const double len = sqrt((e1x * e1x + e1y * e1y) + e1z * e1z);
  e1x /= len; e1y /= len; e1z /= len;
  const double e2x = ny * e1z - nz * e1y, e2y = nz * e1x - nx * e1z, e2z = nx * e1y - ny * e1x;
  const double w = 1.0 / (Q * Q), wh = 1.0 / (Q * kIntensityScale);
  const double sxx = (double)m[4] * w, sxy = (double)m[5] * w, sxz = (double)m[6] * w, syy = (double)m[7] * w,
               syz = (double)m[8] * w, szz = (double)m[9] * w;
  const double hx = (double)m[10] * wh, hy = (double)m[11] * wh, hz = (double)m[12] * wh;
  // S e1, S e2
  const double a1x = (sxx * e1x + sxy * e1y) + sxz * e1z, a1y = (sxy * e1x + syy * e1y) + syz * e1z,
               a1z = (sxz * e1x + syz * e1y) + szz * e1z;
  const double a2x = (sxx * e2x + sxy * e2y) + sxz * e2z, a2y = (sxy * e2x + syy * e2y) + syz * e2z,
               a2z = (sxz * e2x + syz * e2y) + szz * e2z;
  const double g00 = (e1x * a1x + e1y * a1y) + e1z * a1z, g01 = (e1x * a2x + e1y * a2y) + e1z * a2z,
               g11 = (e2x * a2x + e2y * a2y) + e2z * a2z;
  const double b0 = (e1x * hx + e1y * hy) + e1z * hz, b1 = (e2x * hx + e2y * hy) + e2z * hz;
  const double det = g00 * g11 - g01 * g01, top = g00 > g11 ? g00 : g11;
  if (!(det > kGradientPivot * (top * top))) return;   // (NaN too)
  const double c0 = (g11 * b0 - g01 * b1) / det, c1 = (g00 * b1 - g01 * b0) / det;
  out[0] = (float)(e1x * c0 + e2x * c1);
  out[1] = (float)(e1y * c0 + e2y * c1);
  out[2] = (float)(e1z * c0 + e2z * c1);
}

}  // namespace color
}  // namespace d3f
