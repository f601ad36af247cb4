// RGB-D odometry: depth odometry (odometry.hpp) with a photometric term, the "hybrid" objective of Park, Zhou, Koltun
// 2017 after Steinbruecker et al. 2011 (odometry.hip; d3f_rgbd_pyramid, d3f_rgbd_odometry_step, d3f_rgbd_odometry
// and their host twins).  Everything here is __host__ __device__ and reads no state: the kernels and the host twins run
// this text, and ops.rgbd_pyramid_numpy / rgbd_odometry_step_numpy / rgbd_odometry_numpy restate it.  f32 arithmetic
// runs in exactly the order written (-ffp-contract=off; f32 division is correctly rounded on both sides); f64 is used
// only where stated.
//
// Intensity, level 0: from uint8 [F,H,W,3] (R, G, B) I = ((0.299f R + 0.587f G) + 0.114f B) / 255.0f with R, G, B
// converted to f32 first; from uint8 [F,H,W] I = f32(v) / 255.0f; f32 [F,H,W] is taken as it is.  Intensity pyramid:
// the level table of the depth pyramid; pixel (u, v) of level l+1 is (((i00 + i10) + i01) + i11) / 4.0f with i_xy the
// pixel (2u + x, 2v + y) of level l: the 2x2 block in raster order.  An odd last row or column is dropped.  There is no
// validity: a non-finite value propagates into the coarser pixels above it and is excluded where it is read.  The
// intensity is a second packed f32 array beside the depth pyramid, 4 bytes per pixel.
//
// Association: odo::associate, unchanged -- the accepted pixels, the index and a, y, n are those of the depth
// odometry.  An accepted moving pixel (u, v) has a photometric term as well when all of this holds:
//   px = (fx a_0) / a_2 + cx, py = (fy a_1) / a_2 + cy (the fixed level's intrinsics; the projection before it is
//   rounded); x0 = floorf(px), y0 = floorf(py); 1 <= x0 <= W - 3 and 1 <= y0 <= H - 3, compared as floats: the 2x2
//   bilinear footprint (x0..x0+1, y0..y0+1) and the central differences at its four pixels lie inside the image;
//   the moving intensity I_a(u, v) and the 12 fixed intensities read below are finite; q below is finite.
// With wx = px - x0, wy = py - y0 and, for values c00 c10 c01 c11 at (x0,y0) (x0+1,y0) (x0,y0+1) (x0+1,y0+1),
//   bilinear(c) = t + wy (b - t), t = c00 + wx (c10 - c00), b = c01 + wx (c11 - c01):
//   I_b = bilinear of the fixed intensity; gx = bilinear of (I(x+1,y) - I(x-1,y)) / 2.0f; gy = bilinear of
//   (I(x,y+1) - I(x,y-1)) / 2.0f;  r_I = I_b - I_a(u, v);
//   g0 = gx fx, g1 = gy fy, q = (g0 / a_2, g1 / a_2, -((g0 a_0 + g1 a_1) / (a_2 a_2))): the derivative of the sampled
//   intensity with respect to the point a, so the Jacobian row is J_I = [a x q, q] -- the geometric row with q in
//   place of the normal, and plane::plane_step solves the combined system unchanged.
// Sums, 31 per pair: the first 29 are plane.hpp's, where sum J J^T and sum J r hold the geometric rows and, in f64 from
// the f32 values a, q, r_I, the photometric rows scaled by w = f64(photo_weight): (w J_I)(w J_I)^T and (w J_I)(w r_I).
// n and sum d2 stay the geometric count and squared distance.  Sum 29 is n_photo, sum 30 is sum r_I^2 (unweighted).
// photo_weight == 0 skips the term: n_photo = 0 and the first 29 sums are the depth odometry's bit for bit.
#pragma once
#include "odometry.hpp"

namespace d3f {
namespace rgbd {

constexpr int kSums = odo::kSums + 2;
constexpr int kPhotoCount = odo::kSums;       // n_photo
constexpr int kPhotoSquares = odo::kSums + 1; // sum r_I^2

D3F_HD inline bool finite(float x) { return fabsf(x) <= 3.402823466e+38f; }   // false for a NaN and an infinity

// level 0 from 8-bit colour / 8-bit grey
D3F_HD inline float intensity_rgb(const uint8_t* c) {
  return ((0.299f * (float)c[0] + 0.587f * (float)c[1]) + 0.114f * (float)c[2]) / 255.0f;
}
D3F_HD inline float intensity_grey(uint8_t v) { return (float)v / 255.0f; }

// pixel (u, v) of the next level from the level `src` of width Ws
D3F_HD inline float down_pixel(const float* src, int Ws, int u, int v) {
  const float* r0 = src + (size_t)(2 * v) * (size_t)Ws + (size_t)(2 * u);
  const float* r1 = r0 + (size_t)Ws;
  return (((r0[0] + r0[1]) + r1[0]) + r1[1]) / 4.0f;
}

D3F_HD inline float bilinear(float c00, float c10, float c01, float c11, float wx, float wy) {
  const float t = c00 + wx * (c10 - c00);
  const float b = c01 + wx * (c11 - c01);
  return t + wy * (b - t);
}

// The photometric term of an accepted moving pixel: Ia its intensity, a its point in the fixed frame, IB the fixed
// intensity image (H x W) with the intrinsics Kb.  false: there is none.  *r = r_I, q [3] as above.
D3F_HD inline bool photometric(const float* IB, int H, int W, const float* Kb, float Ia, const float* a, float* r,
                               float* q) {
  const float px = (Kb[0] * a[0]) / a[2] + Kb[2];
  const float py = (Kb[1] * a[1]) / a[2] + Kb[3];
  const float x0f = floorf(px), y0f = floorf(py);
  if (!(x0f >= 1.0f && x0f <= (float)(W - 3) && y0f >= 1.0f && y0f <= (float)(H - 3))) return false;   // (NaN too)
  const float wx = px - x0f, wy = py - y0f;
  const float* c = IB + (size_t)(int)y0f * (size_t)W + (size_t)(int)x0f;   // the footprint's first pixel
  const size_t w = (size_t)W;
  const float u0 = c[-(ptrdiff_t)w], u1 = c[1 - (ptrdiff_t)w];                       // row y0 - 1: x0, x0 + 1
  const float m0 = c[-1], m1 = c[0], m2 = c[1], m3 = c[2];                           // row y0: x0 - 1 .. x0 + 2
  const float n0 = c[w - 1], n1 = c[w], n2 = c[w + 1], n3 = c[w + 2];                // row y0 + 1
  const float d0 = c[2 * w], d1 = c[2 * w + 1];                                      // row y0 + 2: x0, x0 + 1
  if (!(finite(Ia) && finite(u0) && finite(u1) && finite(m0) && finite(m1) && finite(m2) && finite(m3) &&
        finite(n0) && finite(n1) && finite(n2) && finite(n3) && finite(d0) && finite(d1)))
    return false;
  const float Ib = bilinear(m1, m2, n1, n2, wx, wy);
  const float gx = bilinear((m2 - m0) / 2.0f, (m3 - m1) / 2.0f, (n2 - n0) / 2.0f, (n3 - n1) / 2.0f, wx, wy);
  const float gy = bilinear((n1 - u0) / 2.0f, (n2 - u1) / 2.0f, (d0 - m1) / 2.0f, (d1 - m2) / 2.0f, wx, wy);
  const float g0 = gx * Kb[0], g1 = gy * Kb[1];
  q[0] = g0 / a[2];
  q[1] = g1 / a[2];
  q[2] = -((g0 * a[0] + g1 * a[1]) / (a[2] * a[2]));
  if (!(finite(q[0]) && finite(q[1]) && finite(q[2]))) return false;
  *r = Ib - Ia;
  return true;
}

// what a photometric term adds to the 31 sums: f64 from the f32 values, the row scaled by w = f64(photo_weight)
D3F_HD inline void add_photometric(double* acc, const float* af, const float* qf, float rf, double w) {
  const double a[3] = {(double)af[0], (double)af[1], (double)af[2]};
  const double q[3] = {(double)qf[0], (double)qf[1], (double)qf[2]};
  const double J[6] = {w * (a[1] * q[2] - a[2] * q[1]), w * (a[2] * q[0] - a[0] * q[2]), w * (a[0] * q[1] - a[1] * q[0]),
                       w * q[0], w * q[1], w * q[2]};
  const double r = (double)rf, rw = w * r;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = i; j < 6; ++j) acc[1 + plane::upper6(i, j)] += J[i] * J[j];
    acc[22 + i] += J[i] * rw;
  }
  acc[kPhotoCount] += 1.0;
  acc[kPhotoSquares] += r * r;
}

}  // namespace rgbd
}  // namespace d3f
