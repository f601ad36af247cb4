// Ray-casting a dense TSDF volume from a camera: a volume plus a pose gives a depth image and, when asked, a normal
// image (tsdf_raycast.hip; d3f_tsdf_raycast and its host twin).  Everything here is __host__ __device__ and reads no
// state: the kernel and the host twin run this text, and ops.tsdf_raycast_numpy restates it.  All arithmetic is f32 in
// exactly the order written (the library is built with -ffp-contract=off, f32 division and square root are correctly
// rounded on both sides), so device, host twin and NumPy agree bit for bit.
//
// View r looks at volume view_volume[r] of a batch laid out as in tsdf.hpp (lattice nx x ny x nz, ix fastest, origin,
// voxel; D and w as d3f_tsdf_integrate leaves them).  Its image is H x W with K = (fx, fy, cx, cy); C [3x4 row-major]
// maps the camera into the volume's frame.  Per pixel (u, v):
//   ray      x = (f32(u) - cx) / fx,  y = (f32(v) - cy) / fy.  The ray's parameter is the camera z-depth -- the depth
//            the integration measures sdf = d - p_z along, so D is linear in it for a single frame.
//   samples  z_k = depth_min + step * f32(k), k = 0, 1, ... while z_k <= depth_max: always from k, never accumulated,
//            so skipping any k changes no bit.  A view whose step is not > 0, or whose (depth_max - depth_min) / step
//            exceeds kMaxSamples, casts nothing: its image is 0.
//   point    X = x z, Y = y z;  q_r = ((C[r][0] X + C[r][1] Y) + C[r][2] z) + C[r][3]
//   cell     g_a = (q_a - origin_a) / voxel, i_a = floorf(g_a); INSIDE when i_a >= 0 and i_a + 1 < n_a on all three
//            axes, compared as floats before any conversion (a NaN or a huge value is a skip, never an index);
//            f_a = g_a - i_a.  VALID when inside and all 8 corners of the cell have w >= min_weight.  |D| < 1 is NOT
//            required: D = 1 is free space, and a ray must be able to arrive from it.
//   value    trilinear, lerp(a, b, t) = a + t * (b - a): along x on the four (y, z) edges, then along y, then along z.
//   hit      sample k - 1 valid with value t0 > 0 and sample k valid with not (t1 > 0):
//            depth = (z_k - step) + step * (t0 / (t0 - t1)).  The ray ends there.
//   end      a valid sample with t1 < 0 whose predecessor was not a valid positive one ends the ray WITHOUT a hit: a
//            back face, or a surface first met from inside.
//   no hit   the pixel holds 0; so does a hit that is not in (0, depth_max].
//   normal   at a hit, the gradient of the trilinear D by six more samples, g_a = value(q + voxel e_a) - value(q -
//            voxel e_a) with q the point of the hit depth; any of the six invalid: no normal, (0, 0, 0).  Rotated into
//            the camera frame by the transpose of C's rotation, n_j = (C[0][j] g_0 + C[1][j] g_1) + C[2][j] g_2,
//            divided by len = sqrtf((n_0^2 + n_1^2) + n_2^2) under the len test of odo::normal_at (0, NaN or infinite:
//            no normal).  The gradient points towards positive D -- out of the surface into the free space in front of
//            it, the sign of tsdf_mesh's normals.  A hit is reached from t0 > 0, so D falls along the ray there and
//            the normal faces the camera, n . ray < 0 -- the side odo::normal_at flips its normals to.  normal_at
//            forces that sign; here it follows from the volume, so at a silhouette, where the difference over two
//            voxels is not the slope along the ray, a normal may face away by a little.
//
// The box clip.  Only samples inside the lattice can be valid, so a ray's k range may be cut to the stretch where it
// crosses the lattice's box (a slab test on q(z) ~ o + z dir).  The slab test rounds differently from the rule, so the
// box is widened by a voxel and the k range by a sample on either side, and the inside test above still decides: the
// clip changes no bit (samples left out are invalid ones before the first or after the last valid one, which neither
// start, end nor hit anything).
//
// The sampler.  clip_range and cast_ray are templates over the type that stands for the volume: they read its members
// ox, oy, oz, voxel, nx, ny, nz and call two overloaded functions on it, sample() (the trilinear D at a point) and
// march() (the same for sample k of the marching loop, which may also name the last of the samples after k that are
// certainly invalid too: the loop goes on behind it).  Here the sampler is the dense Lattice, whose march() is its
// sample() and names nothing; tsdf_raycast_sparse.hpp adds the sampler of a sparse volume.
#pragma once
#include "tsdf.hpp"

namespace d3f {
namespace raycast {

constexpr int kMaxSamples = 65536;   // samples of one ray at most (D3F_RAYCAST_MAX_SAMPLES)

struct Lattice {            // one volume
  const float* D;             // its voxels
  const float* w;
  int64_t count;              // how many there are: nothing at or beyond it is read
  float ox, oy, oz, voxel;
  int nx, ny, nz;
};

D3F_HD inline float lerp(float a, float b, float t) { return a + t * (b - a); }

// the trilinear D at q; false: outside the lattice's cells, or a corner without weight
D3F_HD inline bool sample(const Lattice& L, float qx, float qy, float qz, float min_weight, float& value) {
  const float gx = (qx - L.ox) / L.voxel, gy = (qy - L.oy) / L.voxel, gz = (qz - L.oz) / L.voxel;
  const float ix = floorf(gx), iy = floorf(gy), iz = floorf(gz);
  if (!(ix >= 0.0f && ix + 1.0f < (float)L.nx && iy >= 0.0f && iy + 1.0f < (float)L.ny && iz >= 0.0f &&
        iz + 1.0f < (float)L.nz))
    return false;
  const int64_t sy = (int64_t)L.nx, sz = (int64_t)L.nx * (int64_t)L.ny;
  const int64_t i = (int64_t)(int)ix + sy * (int64_t)(int)iy + sz * (int64_t)(int)iz;
  if (i + sz + sy + 1 >= L.count) return false;   // vol_start and dims that disagree: nothing beyond the volume is read
  // the 16 loads of a sample: no branch stands between them (the weights are tested without short circuit and the value
  // is formed whatever they say), so all are issued before any is used
  const float w000 = L.w[i], w100 = L.w[i + 1], w010 = L.w[i + sy], w110 = L.w[i + sy + 1];
  const float w001 = L.w[i + sz], w101 = L.w[i + sz + 1], w011 = L.w[i + sz + sy], w111 = L.w[i + sz + sy + 1];
  const float d000 = L.D[i], d100 = L.D[i + 1], d010 = L.D[i + sy], d110 = L.D[i + sy + 1];
  const float d001 = L.D[i + sz], d101 = L.D[i + sz + 1], d011 = L.D[i + sz + sy], d111 = L.D[i + sz + sy + 1];
  const bool weighted = (w000 >= min_weight) & (w100 >= min_weight) & (w010 >= min_weight) & (w110 >= min_weight) &
                        (w001 >= min_weight) & (w101 >= min_weight) & (w011 >= min_weight) & (w111 >= min_weight);
  const float fx = gx - ix, fy = gy - iy, fz = gz - iz;
  const float e00 = lerp(d000, d100, fx), e10 = lerp(d010, d110, fx);
  const float e01 = lerp(d001, d101, fx), e11 = lerp(d011, d111, fx);
  value = lerp(lerp(e00, e10, fy), lerp(e01, e11, fy), fz);
  return weighted;
}

// sample k of the marching loop at q = the ray's point of z_k; `last` comes in as k.  A dense lattice knows nothing
// about the samples after an invalid one.
D3F_HD inline bool march(const Lattice& L, const float* C, float x, float y, float step, float depth_min, int k,
                         const float q[3], float min_weight, float& value, int& last) {
  (void)C, (void)x, (void)y, (void)step, (void)depth_min, (void)k, (void)last;
  return sample(L, q[0], q[1], q[2], min_weight, value);
}

// the point of camera z-depth z on the ray (x, y), in the volume's frame
D3F_HD inline void ray_point(const float* C, float x, float y, float z, float q[3]) {
  const float X = x * z, Y = y * z;
  q[0] = ((C[0] * X + C[1] * Y) + C[2] * z) + C[3];
  q[1] = ((C[4] * X + C[5] * Y) + C[6] * z) + C[7];
  q[2] = ((C[8] * X + C[9] * Y) + C[10] * z) + C[11];
}

// one axis of the slab test: the lattice spans [origin, origin + voxel (n - 1)], taken a voxel wider on either side
D3F_HD inline void clip_axis(float dir, float o, float origin, float voxel, int n, float& zin, float& zout,
                             bool& empty) {
  const float lo = origin - voxel, hi = origin + voxel * (float)n;
  if (dir == 0.0f) {
    if (o < lo || o > hi) empty = true;
  } else {
    const float ta = (lo - o) / dir, tb = (hi - o) / dir;
    zin = fmaxf(zin, fminf(ta, tb));      // a NaN leaves the range as it is
    zout = fminf(zout, fmaxf(ta, tb));
  }
}

// the k range [k0, k1] of the ray (x, y) that can be inside the lattice (empty: k1 < k0); conservative, see above
template <typename Sampler>
D3F_HD inline void clip_range(const Sampler& L, const float* C, float x, float y, float step, float depth_min,
                              float depth_max, int& k0, int& k1) {
  float zin = depth_min, zout = depth_max;
  bool empty = false;
  clip_axis((C[0] * x + C[1] * y) + C[2], C[3], L.ox, L.voxel, L.nx, zin, zout, empty);
  clip_axis((C[4] * x + C[5] * y) + C[6], C[7], L.oy, L.voxel, L.ny, zin, zout, empty);
  clip_axis((C[8] * x + C[9] * y) + C[10], C[11], L.oz, L.voxel, L.nz, zin, zout, empty);
  float lo = floorf((zin - depth_min) / step) - 1.0f, hi = ceilf((zout - depth_min) / step) + 1.0f;
  lo = fminf(fmaxf(lo, 0.0f), (float)(kMaxSamples + 1));   // bounded before the conversion, a NaN included
  hi = fmaxf(fminf(hi, (float)kMaxSamples), -1.0f);
  k0 = (int)lo;
  k1 = empty ? -1 : (int)hi;
}

// the depth of pixel (u, v), 0 without a hit; normal[3] receives the camera-frame normal when `want_normal`, else zeros
template <typename Sampler>
D3F_HD inline float cast_ray(const Sampler& L, const float* K, const float* C, int u, int v, float step,
                             float depth_min, float depth_max, float min_weight, bool clip, bool want_normal,
                             float normal[3]) {
  normal[0] = normal[1] = normal[2] = 0.0f;
  if (!(step > 0.0f) || !((depth_max - depth_min) / step <= (float)kMaxSamples)) return 0.0f;
  const float x = ((float)u - K[2]) / K[0], y = ((float)v - K[3]) / K[1];
  int k0 = 0, k1 = kMaxSamples;
  if (clip) clip_range(L, C, x, y, step, depth_min, depth_max, k0, k1);
  bool positive = false;     // the previous sample was valid with a value > 0
  float t0 = 0.0f, depth = 0.0f;
  for (int k = k0; k <= k1; ++k) {
    const float z = depth_min + step * (float)k;
    if (!(z <= depth_max)) break;
    float q[3], t1;
    ray_point(C, x, y, z, q);
    int last = k;              // the last sample known to be invalid when this one is
    if (!march(L, C, x, y, step, depth_min, k, q, min_weight, t1, last)) {
      positive = false;
      k = last;
      continue;
    }
    if (positive && !(t1 > 0.0f)) {
      depth = (z - step) + step * (t0 / (t0 - t1));
      break;
    }
    if (t1 < 0.0f) break;     // a back face, or a surface first met from inside
    positive = t1 > 0.0f;
    t0 = t1;
  }
  if (!(depth > 0.0f && depth <= depth_max)) return 0.0f;
  if (want_normal) {
    float q[3], xp = 0.0f, xm = 0.0f, yp = 0.0f, ym = 0.0f, zp = 0.0f, zm = 0.0f;
    ray_point(C, x, y, depth, q);
    bool ok = sample(L, q[0] + L.voxel, q[1], q[2], min_weight, xp);
    ok = sample(L, q[0] - L.voxel, q[1], q[2], min_weight, xm) && ok;
    ok = sample(L, q[0], q[1] + L.voxel, q[2], min_weight, yp) && ok;
    ok = sample(L, q[0], q[1] - L.voxel, q[2], min_weight, ym) && ok;
    ok = sample(L, q[0], q[1], q[2] + L.voxel, min_weight, zp) && ok;
    ok = sample(L, q[0], q[1], q[2] - L.voxel, min_weight, zm) && ok;
    const float g[3] = {xp - xm, yp - ym, zp - zm};
    if (ok) {
      const float n0 = (C[0] * g[0] + C[4] * g[1]) + C[8] * g[2];
      const float n1 = (C[1] * g[0] + C[5] * g[1]) + C[9] * g[2];
      const float n2 = (C[2] * g[0] + C[6] * g[1]) + C[10] * g[2];
      const float len = sqrtf((n0 * n0 + n1 * n1) + n2 * n2);
      if (len > 0.0f && len <= 3.402823466e+38f) {   // not 0, NaN or infinite
        normal[0] = n0 / len;
        normal[1] = n1 / len;
        normal[2] = n2 / len;
      }
    }
  }
  return depth;
}

}  // namespace raycast
}  // namespace d3f
