// TSDF fusion of depth frames into dense volumes and the extraction of their zero crossings (tsdf.hip: d3f_tsdf_bounds;
// tsdf_integrate.hip: d3f_tsdf_integrate, tsdf_extract.hip: d3f_tsdf_extract, both dense and sparse; and their host
// twins).  Everything here
// is __host__ __device__ and reads no state: the kernels and the host twins run this text, and ops.tsdf_numpy /
// tsdf_extract_numpy restate it.  All arithmetic is f32 in exactly the order written; the library is built with
// -ffp-contract=off and f32 division is correctly rounded on both sides, so device, host twin and NumPy agree bit for
// bit.
//
// Volume v: a lattice nx x ny x nz (ix fastest in memory) with origin[3] and a voxel size, in some frame; lattice point
// (ix, iy, iz) = origin_a + voxel * f32(i_a).  It owns the frames [frame_start[v], frame_start[v + 1]).
// Frame f: a depth image H x W (uint16 raw units or f32 metres), intrinsics K = (fx, fy, cx, cy), M [3x4 row-major]
// mapping the volume's frame into the camera, C [3x4] its inverse (camera into the volume's frame; the bounds only).
//
// Integration, per voxel (x, y, z), frames in order, from D = 0, w = 0 or from the stored values (into != 0):
//   p_r = ((M[r][0] x + M[r][1] y) + M[r][2] z) + M[r][3]                      r = 0, 1, 2
//   skip unless p_z > 0
//   u = floorf(((fx p_x) / p_z + cx) + 0.5f), v likewise with fy, p_y, cy;  skip unless 0 <= u < W and 0 <= v < H
//       (compared as floats, before any conversion: a NaN or a huge value is a skip, never an index)
//   d = f32(raw) / depth_scale (uint16) | raw (f32);  skip unless d > 0;  skip if d > depth_max
//   sdf = d - p_z;  skip if sdf < -trunc;  t = fminf(1, sdf / trunc)
//   D = (D w + t) / (w + 1);  w = w + 1
// With colour (kCc = 1 or 3; tsdf_color.hpp), before D and w and with the w from before the increment, per channel
//   c = (c w + c_pixel) / (w + 1),  c_pixel = colour_pixel() at the unrounded projection
// integrate_frame<kCc> is the one frame body and integrate_voxel<kCc> the one frame loop of every form: dense and
// sparse, from zero and continued, with colour and without (kCc = 0 reads and computes nothing of the colour).
//
// Bounds, per valid pixel (u, v) (d > 0 and not d > depth_max) of a volume's frames:
//   X = ((f32(u) - cx) d) / fx,  Y = ((f32(v) - cy) d) / fy,  q_r = ((C[r][0] X + C[r][1] Y) + C[r][2] d) + C[r][3]
//   minimum and maximum per component under the ORDER of order_key(): exact, so order of arrival cannot matter.
//
// Extraction.  A voxel is VALID when w >= min_weight and |D| < 1.  For a valid voxel and each axis x, y, z in that
// order: the +1 neighbour on the axis, when it is inside the lattice, valid, and (D0 < 0) != (D1 < 0), gives one point
// -- the voxel's lattice point with that axis's coordinate moved by voxel * (|D0| / (|D0| + |D1|)).  Output order:
// volume, lattice index of the lower voxel, axis; the result is a pure function of the volume.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define D3F_HD __host__ __device__
#else
#define D3F_HD
#endif

namespace d3f {
namespace tsdf {

D3F_HD inline float depth_value(const uint16_t* image, size_t i, float depth_scale) {
  return (float)image[i] / depth_scale;
}
D3F_HD inline float depth_value(const float* image, size_t i, float) { return image[i]; }

D3F_HD inline float lattice(float origin, float voxel, int i) { return origin + voxel * (float)i; }

// what one frame observes at one voxel: false when the frame skips it; else t, and (uf, vf), the voxel's projection
// whose rounding names the depth pixel that was read (colour_pixel reads the colour there)
template <typename DepthT>
D3F_HD inline bool observe_frame(float x, float y, float z, const float* M, const float* K, const DepthT* image, int H,
                                 int W, float depth_scale, float depth_max, float trunc, float& t, float& uf, float& vf) {
  const float px = ((M[0] * x + M[1] * y) + M[2] * z) + M[3];
  const float py = ((M[4] * x + M[5] * y) + M[6] * z) + M[7];
  const float pz = ((M[8] * x + M[9] * y) + M[10] * z) + M[11];
  if (!(pz > 0.0f)) return false;
  uf = (K[0] * px) / pz + K[2];
  vf = (K[1] * py) / pz + K[3];
  const float u = floorf(uf + 0.5f);
  const float v = floorf(vf + 0.5f);
  if (!(u >= 0.0f && u < (float)W && v >= 0.0f && v < (float)H)) return false;
  const float d = depth_value(image, (size_t)(int)v * (size_t)W + (size_t)(int)u, depth_scale);
  if (!(d > 0.0f) || d > depth_max) return false;
  const float sdf = d - pz;
  if (sdf < -trunc) return false;
  t = fminf(1.0f, sdf / trunc);
  return true;
}

// the colour frame colour [H, W, kCc] at the projection (uf, vf) of an observed voxel, bilinear over the 2 x 2 pixels
// around it, each index clamped into the image (the rule is tsdf_color.hpp's): cp [kCc]
template <int kCc>
D3F_HD inline void colour_pixel(const float* colour, int H, int W, float uf, float vf, float* cp) {
  // observed: -0.5 <= uf < W - 0.5 and likewise vf, so the conversions to int are safe
  const float u0 = floorf(uf), v0 = floorf(vf);
  const float a = uf - u0, b = vf - v0;
  const int iu = (int)u0, iv = (int)v0;
  const size_t c0 = (size_t)(iu < 0 ? 0 : iu), c1 = (size_t)(iu + 1 < W ? iu + 1 : W - 1);
  const size_t r0 = (size_t)(iv < 0 ? 0 : iv) * (size_t)W, r1 = (size_t)(iv + 1 < H ? iv + 1 : H - 1) * (size_t)W;
#pragma unroll
  for (int ch = 0; ch < kCc; ++ch) {
    const float c00 = colour[(r0 + c0) * kCc + ch], c01 = colour[(r0 + c1) * kCc + ch];
    const float c10 = colour[(r1 + c0) * kCc + ch], c11 = colour[(r1 + c1) * kCc + ch];
    cp[ch] = (c00 * (1.0f - a) + c01 * a) * (1.0f - b) + (c10 * (1.0f - a) + c11 * a) * b;
  }
}

// one frame into one voxel.  kCc colour channels: colour [H, W, kCc] is the frame's colour image and c [kCc] the
// voxel's colour, updated with the w from before the increment; kCc = 0: no colour, neither is touched
template <int kCc, typename DepthT>
D3F_HD inline void integrate_frame(float x, float y, float z, const float* M, const float* K, const DepthT* image,
                                   const float* colour, int H, int W, float depth_scale, float depth_max, float trunc,
                                   float& D, float& w, float* c) {
  float t, uf, vf;
  if (!observe_frame(x, y, z, M, K, image, H, W, depth_scale, depth_max, trunc, t, uf, vf)) return;
  if constexpr (kCc > 0) {
    float cp[kCc];
    colour_pixel<kCc>(colour, H, W, uf, vf, cp);
#pragma unroll
    for (int ch = 0; ch < kCc; ++ch) c[ch] = (c[ch] * w + cp[ch]) / (w + 1.0f);
  }
  D = (D * w + t) / (w + 1.0f);
  w = w + 1.0f;
}

// the frames [f0, f1) of a volume into the voxel at (x, y, z), continuing from the (D, w, c) given; images [F, H, W],
// colours [F, H, W, kCc], M [F, 12], K [F, 4].  "From D = 0, w = 0, c = 0" is the caller passing zeros.  The running
// mean is sequential over the frames, so the frames [f0, k) from zeros and then [k, f1) from their result give exactly
// what [f0, f1) gives from zeros (the entries' into != 0)
template <int kCc, typename DepthT>
D3F_HD inline void integrate_voxel(float x, float y, float z, int f0, int f1, const float* M, const float* K,
                                   const DepthT* images, const float* colours, int H, int W, float depth_scale,
                                   float depth_max, float trunc, float& D, float& w, float* c) {
  const size_t pixels = (size_t)H * (size_t)W;
  for (int f = f0; f < f1; ++f)
    integrate_frame<kCc>(x, y, z, M + 12 * (size_t)f, K + 4 * (size_t)f, images + pixels * (size_t)f,
                         colours + pixels * (size_t)f * kCc, H, W, depth_scale, depth_max, trunc, D, w, c);
}

// the volume of global voxel g / of frame f: the last v with start[v] <= i (start rises; empty ranges are skipped)
template <typename T>
D3F_HD inline int owner(const T* start, int V, T i) {
  int lo = 0, hi = V;   // start[lo] <= i < start[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (start[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// ---------------------------------------------------------------------------------------------------------- bounds
// a key whose UNSIGNED order is the order of the floats (-inf < ... < -0 < +0 < ... < +inf; NaNs at the two ends)
D3F_HD inline uint32_t float_bits(float v) {
  union { float f; uint32_t u; } c;
  c.f = v;
  return c.u;
}
D3F_HD inline float bits_float(uint32_t u) {
  union { float f; uint32_t u; } c;
  c.u = u;
  return c.f;
}
D3F_HD inline uint32_t order_key(float v) {
  const uint32_t u = float_bits(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
D3F_HD inline float order_value(uint32_t k) { return bits_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
constexpr uint32_t kKeyPosInf = 0xff800000u;   // order_key(+inf): where a minimum starts
constexpr uint32_t kKeyNegInf = 0x007fffffu;   // order_key(-inf): where a maximum starts

// the back-projected point of pixel (u, v) in the volume's frame; false: the pixel holds no valid depth
template <typename DepthT>
D3F_HD inline bool back_project(const DepthT* image, int W, int u, int v, const float* K, const float* C,
                                float depth_scale, float depth_max, float q[3]) {
  const float d = depth_value(image, (size_t)v * (size_t)W + (size_t)u, depth_scale);
  if (!(d > 0.0f) || d > depth_max) return false;
  const float X = (((float)u - K[2]) * d) / K[0];
  const float Y = (((float)v - K[3]) * d) / K[1];
  for (int r = 0; r < 3; ++r) q[r] = ((C[4 * r] * X + C[4 * r + 1] * Y) + C[4 * r + 2] * d) + C[4 * r + 3];
  return true;
}

// ------------------------------------------------------------------------------------------------------ extraction
D3F_HD inline bool valid(float D, float w, float min_weight) { return w >= min_weight && fabsf(D) < 1.0f; }

// the crossings of the voxel at local index `local` of a lattice nx x ny x nz whose `count` values of D / w start at
// Dv / wv (nothing at or beyond `count` is read): bit a of the result is set when axis a emits a point
D3F_HD inline int crossings(const float* Dv, const float* wv, int64_t local, int64_t count, int ix, int iy, int iz,
                            int nx, int ny, int nz, float min_weight) {
  const float D0 = Dv[local];
  if (!valid(D0, wv[local], min_weight)) return 0;
  const int64_t step[3] = {1, (int64_t)nx, (int64_t)nx * (int64_t)ny};
  const bool inside[3] = {ix + 1 < nx, iy + 1 < ny, iz + 1 < nz};
  int mask = 0;
  for (int a = 0; a < 3; ++a) {
    if (!inside[a] || local + step[a] >= count) continue;
    const float D1 = Dv[local + step[a]];
    if (valid(D1, wv[local + step[a]], min_weight) && ((D0 < 0.0f) != (D1 < 0.0f))) mask |= 1 << a;
  }
  return mask;
}

// the point of axis a: out[3]
D3F_HD inline void crossing_point(const float* Dv, int64_t local, int ix, int iy, int iz, int nx, int ny, int a,
                                  const float* origin, float voxel, float* out) {
  const int64_t step = a == 0 ? 1 : (a == 1 ? (int64_t)nx : (int64_t)nx * (int64_t)ny);
  const float a0 = fabsf(Dv[local]), a1 = fabsf(Dv[local + step]);
  out[0] = lattice(origin[0], voxel, ix);
  out[1] = lattice(origin[1], voxel, iy);
  out[2] = lattice(origin[2], voxel, iz);
  out[a] = out[a] + voxel * (a0 / (a0 + a1));
}

D3F_HD inline int popcount3(int mask) { return (mask & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1); }

}  // namespace tsdf
}  // namespace d3f
