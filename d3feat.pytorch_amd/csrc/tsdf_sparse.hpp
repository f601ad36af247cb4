// Sparse TSDF volumes: a dense table over bricks of 8 x 8 x 8 voxels plus a compact pool that holds D and w only for
// the bricks a depth pixel can reach within the truncation distance (tsdf_sparse.hip: d3f_tsdf_sparse_mark, _index;
// tsdf_integrate.hip: _integrate; tsdf_extract.hip: _extract; and their host twins).  Stated in the terms of tsdf.hpp, which it includes: everything here is
// __host__ __device__ and reads no state, all arithmetic is f32 in exactly the order written (-ffp-contract=off), and
// ops.tsdf_allocate_numpy / tsdf_sparse_numpy / tsdf_extract_sparse_numpy restate it, so device, host twin and NumPy
// agree bit for bit -- and, for every voxel that can produce output, with the dense path of tsdf.hpp.
//
// Bricks.  A volume keeps its origin, dims = (nx, ny, nz) and voxel.  Its brick lattice is nb_a = ceil(n_a / 8) per
// axis, bx fastest; voxel (ix, iy, iz) lives in brick (ix >> 3, iy >> 3, iz >> 3) at in-brick index (the SLOT)
// (ix & 7) + 8 (iy & 7) + 64 (iz & 7).  A slot of an edge brick with i_a >= n_a does not exist: it is stored as D = 0,
// w = 0 and is never valid.  A voxel in a brick that was not allocated is D = 0, w = 0 and never valid either.
//
// Allocation (mark), per valid pixel (u, v) (back_project's test: d > 0 and not d > depth_max) of every frame of the
// volume, with su = {(f32(u) - 0.5) - cx, (f32(u) + 0.5) - cx}, sv likewise with cy, and
// z = {d - trunc > 0 ? d - trunc : 0, d + trunc}: the 8 corners
//   X = (su z) / fx,  Y = (sv z) / fy,  q_r = ((C[r][0] X + C[r][1] Y) + C[r][2] z) + C[r][3]
// in the order z, sv, su (su fastest), their componentwise minimum and maximum by `q < lo ? q : lo` / `q > hi ? q : hi`
// from the first corner, then per axis
//   flo = floorf((lo - origin) / voxel) - 1,   fhi = floorf((hi - origin) / voxel) + 1        (one voxel wider)
// The pixel is skipped unless fhi >= 0 and flo <= f32(n - 1) on every axis (compared as floats: a NaN is a skip, never
// an index); otherwise both are clamped to [0, n - 1] and every brick of the box [flo >> 3, fhi >> 3]^3 is flagged.
// Flags are idempotent and the result is a set: the order of arrival cannot matter and no atomic decides anything.
//
// Why the flagged bricks are a superset of what the dense volume can emit.  A voxel is VALID in the dense volume only
// if |D| < 1, and D is a mean of values t <= 1, so some frame gave it t < 1, i.e. sdf < trunc; integrate_frame also
// demands sdf >= -trunc and p_z > 0, so in that frame p_z lies in [max(d - trunc, 0), d + trunc], and the voxel rounded
// to that pixel: its projection ((fx p_x) / p_z + cx, ...) lies in [u - 0.5, u + 0.5) x [v - 0.5, v + 0.5).  The
// voxel's camera-frame position is therefore (s z, t z, z) with (s, t, z) inside the box whose corners are taken
// above; that map is linear in s and in t for fixed z and the images of the segments are again segments, so the
// position lies in the convex hull of the 8 corner images, and so does its image under the affine map C: inside the componentwise
// minimum and maximum.  What is not exact is the f32 rounding of M, C and the projection, about 1e-6 m against voxels
// of millimetres: the one-voxel widening absorbs it.  Every brick that holds a dense-valid voxel is therefore
// allocated.  An allocated brick integrates ALL frames of its volume with integrate_voxel unchanged, so its D and w are
// the dense ones bit for bit, and extraction sees the same valid voxels with the same values.
//
// Index.  The flags are scanned in brick-lattice order, volume after volume: brick_index[lattice_start[v] + l] is the
// rank of lattice brick l among the flagged bricks of ITS volume, or -1; brick_start [V + 1] is the prefix of the
// allocated bricks over the volumes and brick_coord [B, 3] = (bx, by, bz) lists them in pool order.  Pool row of
// brick l of volume v = brick_start[v] + brick_index[lattice_start[v] + l].
//
// Integration.  The pool is D, w [B, 512]; every existing slot gets integrate_voxel over all frames of its volume
// (the volume of pool row b is owner(brick_start, V, b)), every other slot D = 0, w = 0.
//
// Extraction: tsdf.hpp's rule (valid(), the sign test, the point) per existing slot.  The +1 neighbour on an axis
// comes from the same brick or, across a face, from the brick that brick_index names; an absent brick, like a neighbour
// outside the lattice, is an invalid neighbour.  Output order: volume, brick in lattice order, slot, axis.  The points
// equal the dense ones bit for bit as a set of rows; the order is this one.
#pragma once
#include "tsdf.hpp"

namespace d3f {
namespace tsdf {

constexpr int kBrickVoxels = 512;

D3F_HD inline int brick_count(int n) { return n > 0 ? ((n - 1) >> 3) + 1 : 0; }   // bricks along an axis of n voxels

struct Bricks {                 // the sparse batch: device pointers on the device side, host pointers in the twins
  const int64_t* lattice_start;   // [V + 1] prefix of the lattice bricks nbx nby nbz
  const int64_t* brick_start;     // [V + 1] prefix of the allocated bricks
  const int32_t* brick_index;     // [L] rank inside the volume, or -1
  const int32_t* brick_coord;     // [B, 3]
  const float* origin;            // [V, 3]
  const int32_t* dims;            // [V, 3]
  const float* voxel;             // [V]
  int V;
  int64_t L, B;
};

// f clamped to [0, n - 1] as an index; f is a whole number or NaN-free by the test before it
D3F_HD inline int clamp_index(float f, int n) { return f <= 0.0f ? 0 : (f >= (float)(n - 1) ? n - 1 : (int)f); }

// the box of bricks [lo, hi] (inclusive, per axis) that pixel (u, v) of a frame flags in a volume; false: no valid
// depth, or the box misses the lattice
template <typename DepthT>
D3F_HD inline bool pixel_bricks(const DepthT* image, int W, int u, int v, const float* K, const float* C,
                                float depth_scale, float depth_max, float trunc, const float* origin,
                                const int32_t* dims, float voxel, int lo[3], int hi[3]) {
  const float d = depth_value(image, (size_t)v * (size_t)W + (size_t)u, depth_scale);
  if (!(d > 0.0f) || d > depth_max) return false;
  const float zn = d - trunc;
  const float z[2] = {zn > 0.0f ? zn : 0.0f, d + trunc};
  const float su[2] = {((float)u - 0.5f) - K[2], ((float)u + 0.5f) - K[2]};
  const float sv[2] = {((float)v - 0.5f) - K[3], ((float)v + 0.5f) - K[3]};
  float qlo[3] = {0.0f, 0.0f, 0.0f}, qhi[3] = {0.0f, 0.0f, 0.0f};
  for (int c = 0; c < 8; ++c) {
    const float zz = z[c >> 2];
    const float X = (su[c & 1] * zz) / K[0];
    const float Y = (sv[(c >> 1) & 1] * zz) / K[1];
    for (int r = 0; r < 3; ++r) {
      const float q = ((C[4 * r] * X + C[4 * r + 1] * Y) + C[4 * r + 2] * zz) + C[4 * r + 3];
      if (c == 0) {
        qlo[r] = q;
        qhi[r] = q;
      } else {
        qlo[r] = q < qlo[r] ? q : qlo[r];
        qhi[r] = q > qhi[r] ? q : qhi[r];
      }
    }
  }
  for (int r = 0; r < 3; ++r) {
    const float flo = floorf((qlo[r] - origin[r]) / voxel) - 1.0f;
    const float fhi = floorf((qhi[r] - origin[r]) / voxel) + 1.0f;
    if (!(fhi >= 0.0f && flo <= (float)(dims[r] - 1))) return false;
    lo[r] = clamp_index(flo, dims[r]) >> 3;
    hi[r] = clamp_index(fhi, dims[r]) >> 3;
  }
  return true;
}

// the voxel (i[3]) of slot s of pool row b of volume v; false: the slot does not exist (or the row's coordinates are
// not those of a lattice brick)
D3F_HD inline bool slot_voxel(const int32_t* dims, const int32_t* coord, int s, int i[3]) {
  const int in[3] = {s & 7, (s >> 3) & 7, s >> 6};
  bool ok = true;
  for (int a = 0; a < 3; ++a) {
    ok = ok && coord[a] >= 0 && coord[a] < brick_count(dims[a]);
    i[a] = coord[a] * 8 + in[a];
    ok = ok && i[a] < dims[a];
  }
  return ok;
}

// the crossings of slot s of pool row b of volume v (bit a: axis a emits) and, for those axes, at[a] = the position of
// the +1 neighbour in the pool; i[3] = the voxel.  Nothing outside brick_index [L] and the pool [B, 512] is read.
D3F_HD inline int sparse_crossings(const Bricks& k, const float* D, const float* w, float min_weight, int v, int64_t b,
                                   int s, int i[3], int64_t at[3]) {
  const int32_t* n = k.dims + 3 * (size_t)v;
  const int32_t* c = k.brick_coord + 3 * (size_t)b;
  if (!slot_voxel(n, c, s, i)) return 0;
  const int64_t here = b * kBrickVoxels + s;
  const float D0 = D[here];
  if (!valid(D0, w[here], min_weight)) return 0;
  int mask = 0;
  for (int a = 0; a < 3; ++a) {
    if (i[a] + 1 >= n[a]) continue;
    const int step = 1 << (3 * a);
    if (((s >> (3 * a)) & 7) < 7) {
      at[a] = here + step;
    } else {
      int nb[3] = {c[0], c[1], c[2]};
      nb[a] += 1;                                              // inside the brick lattice: i[a] + 1 < n[a]
      const int64_t l = k.lattice_start[v] +
                        ((int64_t)nb[2] * brick_count(n[1]) + nb[1]) * (int64_t)brick_count(n[0]) + nb[0];
      if (l < 0 || l >= k.L) continue;
      const int32_t rank = k.brick_index[l];
      if (rank < 0) continue;                                  // an absent brick: the neighbour is invalid
      const int64_t row = k.brick_start[v] + rank;
      if (row < 0 || row >= k.B) continue;
      at[a] = row * kBrickVoxels + (s - 7 * step);
    }
    const float D1 = D[at[a]];
    if (valid(D1, w[at[a]], min_weight) && ((D0 < 0.0f) != (D1 < 0.0f))) mask |= 1 << a;
  }
  return mask;
}

// the point of axis a of voxel i[3] with the values D0 (the voxel) and D1 (its +1 neighbour): crossing_point's
D3F_HD inline void sparse_point(float D0, float D1, const int i[3], int a, const float* origin, float voxel,
                                float* out) {
  const float a0 = fabsf(D0), a1 = fabsf(D1);
  out[0] = lattice(origin[0], voxel, i[0]);
  out[1] = lattice(origin[1], voxel, i[1]);
  out[2] = lattice(origin[2], voxel, i[2]);
  out[a] = out[a] + voxel * (a0 / (a0 + a1));
}

}  // namespace tsdf
}  // namespace d3f
