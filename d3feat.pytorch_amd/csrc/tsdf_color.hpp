// Colour in TSDF volumes: fused beside D and w, sampled at points and carried by the ray-caster (tsdf_integrate.hip,
// tsdf_raycast.hip; the d3f_tsdf_*_color entry points and their host twins).  Stated in the terms of tsdf.hpp,
// tsdf_sparse.hpp and tsdf_raycast.hpp, which it includes:
// everything here is __host__ __device__ and reads no state, all arithmetic is f32 in exactly the order written
// (-ffp-contract=off, correctly rounded division), and ops.tsdf_numpy(color=) / tsdf_sample_color_numpy /
// tsdf_raycast_numpy(color=) restate it, so device, host twin and NumPy agree bit for bit.  A NaN is a NaN: which of
// its bit patterns an operation produces differs between processors and is not part of the contract.
//
// Colour volume.  Cv f32 [total, Cc], channel last, beside D and w of tsdf.hpp; a sparse pool is Cp f32 [B, 512, Cc]
// beside the pool of tsdf_sparse.hpp.  Cc is 1 (intensity: what the RGB-D tracker compares, 4 bytes per voxel) or 3
// (R, G, B).
//
// Colour frames.  f32 [F, H, W, Cc] in [0, 1], registered to the depth pixel by pixel.  The kernels read f32 only; the
// callers make the frames once: uint8 RGB is f32(c) / 255.0f per channel for Cc = 3, and rgbd::intensity_rgb /
// intensity_grey (rgbd_odometry.hpp) for Cc = 1 -- level 0 of the tracker's intensity pyramid, so the model holds what
// the tracker compares.
//
// Integration (the text is tsdf.hpp's: integrate_frame<kCc> and colour_pixel<kCc>).  On exactly the frames where
// integrate_frame updates D and w (observe_frame is true), with the w from BEFORE the increment, per channel
//   c = (c w + c_pixel) / (w + 1)
// then D and w as tsdf.hpp has them.  There is no second weight: w is the weight of the colour too, and D and w are
// those of the colourless integration bit for bit.
//   c_pixel is the image at the voxel's projection (uf, vf) = ((fx p_x) / p_z + cx, (fy p_y) / p_z + cy), the very
//   values whose rounding floorf(. + 0.5f) names the depth pixel, bilinear over the 2 x 2 pixels around it:
//   u0 = floorf(uf), a = uf - u0, v0 = floorf(vf), b = vf - v0; the taps (u0, u0 + 1) x (v0, v0 + 1), each index
//   clamped into the image (a projection within half a pixel of the border reads the border pixel), and
//   c_pixel = (c00 (1 - a) + c01 a) (1 - b) + (c10 (1 - a) + c11 a) b,  c_vu the tap of row v0 + v, column u0 + u.
//   The depth pixel is always one of the taps.  The DEPTH is read at the nearest pixel, as tsdf.hpp says; the colour is
//   not, because a voxel is not a pixel: at voxel 0.02 and 16.7 mm pixels the nearest pixel's colour sits up to half
//   a pixel off the voxel, the offsets do not average out (a mean of 0.1 pixel = 1.7 mm where the two pitches are
//   6 : 5), and an RGB-D tracker finds that offset between a frame and the render of the model.
// A non-finite colour value in any of the four taps propagates into the voxel's colour; it is a value, never an index.
// Continuing (into != 0 with channels > 0) starts integrate_voxel from the stored (D, w, c), so the frames [0, k) and
// then [k, F) give the colour of one call bit for bit.  A slot of a sparse pool that does not exist, like a voxel of
// an absent brick, is w = 0 with colour 0.
//
// color_at(sampler, colour, q, min_weight, out[Cc]): the colour at a point q of the volume's frame.
//   g_a = (q_a - origin_a) / voxel.  OUTSIDE unless 0 <= g_a <= f32(n_a - 1) on all three axes, compared as floats
//   before any conversion (a NaN is outside, never an index); outside too when some n_a < 2 (no cell).
//   i_a = min(floorf(g_a), n_a - 2), f_a = g_a - i_a: a point on the last lattice plane is inside with f = 1.
//   t_c = ((f_x or 1 - f_x) (f_y or 1 - f_y)) (f_z or 1 - f_z) for the 8 corners c of the cell, x fastest; f_a where
//   the corner is the +1 one on axis a, 1 - f_a where it is not.
//   s = the sum of t_c, and per channel the sum of t_c c_c, over the corners with w >= min_weight, both from 0 in corner
//   order; the colour is that sum divided by s.  Outside, or s not > 0: every channel is NaN.
// The weights are renormalised over the weighted corners instead of asking for all 8, so rim points and hits in partly
// observed cells still get a colour.  Nothing beyond the volume's voxels, the tables or the pool is read.
//
// Ray-cast colour.  At a hit of cast_ray the colour is color_at(ray_point(depth)); without a hit it is NaN -- not 0,
// so the render goes into the intensity pyramid as it is and the tracker's finiteness test drops those pixels.  Depth
// and normals are cast_ray's, untouched.
#pragma once
#include "tsdf_raycast_sparse.hpp"

namespace d3f {
namespace raycast {

D3F_HD inline float color_nan() { return tsdf::bits_float(0x7fc00000u); }

// the cell of q: i[3] its base voxel, f[3] the point's place in it; false: outside.  Sampler: Lattice or SparseLattice
template <typename Sampler>
D3F_HD inline bool color_cell(const Sampler& L, const float q[3], int i[3], float f[3]) {
  if (L.nx < 2 || L.ny < 2 || L.nz < 2) return false;
  const float g[3] = {(q[0] - L.ox) / L.voxel, (q[1] - L.oy) / L.voxel, (q[2] - L.oz) / L.voxel};
  const int n[3] = {L.nx, L.ny, L.nz};
  if (!(g[0] >= 0.0f && g[0] <= (float)(n[0] - 1) && g[1] >= 0.0f && g[1] <= (float)(n[1] - 1) && g[2] >= 0.0f &&
        g[2] <= (float)(n[2] - 1)))
    return false;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float base = fminf(floorf(g[a]), (float)(n[a] - 2));
    i[a] = (int)base;
    f[a] = g[a] - base;
  }
  return true;
}

// the renormalised trilinear mean of the weighted corners: wgt [8] and col [8, kCc] of the corners, x fastest
template <int kCc>
D3F_HD inline void color_blend(const float* wgt, const float* col, const float f[3], float min_weight, float* out) {
  const float tx[2] = {1.0f - f[0], f[0]}, ty[2] = {1.0f - f[1], f[1]}, tz[2] = {1.0f - f[2], f[2]};
  float s = 0.0f, acc[kCc];
#pragma unroll
  for (int ch = 0; ch < kCc; ++ch) acc[ch] = 0.0f;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float t = (tx[c & 1] * ty[(c >> 1) & 1]) * tz[c >> 2];
    const bool weighted = wgt[c] >= min_weight;
    s = weighted ? s + t : s;
#pragma unroll
    for (int ch = 0; ch < kCc; ++ch) acc[ch] = weighted ? acc[ch] + t * col[c * kCc + ch] : acc[ch];
  }
#pragma unroll
  for (int ch = 0; ch < kCc; ++ch) out[ch] = s > 0.0f ? acc[ch] / s : color_nan();
}

template <int kCc>
D3F_HD inline void color_none(float* out) {
#pragma unroll
  for (int ch = 0; ch < kCc; ++ch) out[ch] = color_nan();
}

// dense: colour [count, kCc] are the volume's voxels, beside L.D and L.w
template <int kCc>
D3F_HD inline void color_at(const Lattice& L, const float* colour, const float q[3], float min_weight, float* out) {
  int i[3];
  float f[3];
  color_none<kCc>(out);
  if (!color_cell(L, q, i, f)) return;
  const int64_t sy = (int64_t)L.nx, sz = (int64_t)L.nx * (int64_t)L.ny;
  const int64_t at = (int64_t)i[0] + sy * (int64_t)i[1] + sz * (int64_t)i[2];
  if (at + sz + sy + 1 >= L.count) return;   // vol_start and dims that disagree: nothing beyond the volume is read
  float wgt[8], col[8 * kCc];
#pragma unroll
  for (int c = 0; c < 8; ++c) wgt[c] = L.w[at + (c & 1) + sy * ((c >> 1) & 1) + sz * (c >> 2)];
#pragma unroll
  for (int c = 0; c < 8; ++c)
#pragma unroll
    for (int ch = 0; ch < kCc; ++ch)
      col[c * kCc + ch] = colour[(at + (c & 1) + sy * ((c >> 1) & 1) + sz * (c >> 2)) * kCc + ch];
  color_blend<kCc>(wgt, col, f, min_weight, out);
}

// sparse: colour [rows, 512, kCc] is the pool of the whole batch, beside L.D and L.w; a corner in an absent brick is
// w = 0 with colour 0, as in sample()
template <int kCc>
D3F_HD inline void color_at(const SparseLattice& L, const float* colour, const float q[3], float min_weight,
                            float* out) {
  int i[3];
  float f[3];
  color_none<kCc>(out);
  if (!color_cell(L, q, i, f)) return;
  int64_t at[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int cx = i[0] + (c & 1), cy = i[1] + ((c >> 1) & 1), cz = i[2] + (c >> 2);
    const int64_t row = brick_row(L, cx >> 3, cy >> 3, cz >> 3);
    at[c] = row < 0 ? -1 : row * tsdf::kBrickVoxels + ((cx & 7) + 8 * (cy & 7) + 64 * (cz & 7));
  }
  float wgt[8], col[8 * kCc];
#pragma unroll
  for (int c = 0; c < 8; ++c) wgt[c] = at[c] < 0 ? 0.0f : L.w[at[c]];
#pragma unroll
  for (int c = 0; c < 8; ++c)
#pragma unroll
    for (int ch = 0; ch < kCc; ++ch) col[c * kCc + ch] = at[c] < 0 ? 0.0f : colour[at[c] * kCc + ch];
  color_blend<kCc>(wgt, col, f, min_weight, out);
}

// the colour of pixel (u, v) whose ray cast_ray ended at `depth` (0: no hit)
template <int kCc, typename Sampler>
D3F_HD inline void hit_color(const Sampler& L, const float* colour, const float* K, const float* C, int u, int v,
                             float depth, float min_weight, float* out) {
  if (!(depth > 0.0f)) {
    color_none<kCc>(out);
    return;
  }
  const float x = ((float)u - K[2]) / K[0], y = ((float)v - K[3]) / K[1];
  float q[3];
  ray_point(C, x, y, depth, q);
  color_at<kCc>(L, colour, q, min_weight, out);
}

}  // namespace raycast
}  // namespace d3f
