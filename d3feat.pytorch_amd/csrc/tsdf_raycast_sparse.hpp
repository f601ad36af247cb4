// Ray-casting a sparse TSDF volume, growing its bricks and continuing its integration (tsdf_raycast.hip:
// d3f_tsdf_raycast_sparse and its host twin; tsdf_integrate.hip: d3f_tsdf_sparse_integrate, into != 0).  Stated in the
// terms of tsdf_raycast.hpp and tsdf_sparse.hpp, which it includes: everything here is __host__ __device__ and reads
// no state, all arithmetic is f32 in the order written there, and ops.tsdf_raycast_sparse_numpy restates it.
//
// The rule is cast_ray of tsdf_raycast.hpp unchanged -- the same text, instantiated for another sampler -- with ONE
// thing replaced: where the D and w of a cell's corner voxel come from.
//   Voxel (ix, iy, iz) of volume v lies in lattice brick l = ((iz >> 3) nby + (iy >> 3)) nbx + (ix >> 3) of its volume
//   (nb_a = ceil(n_a / 8)), whose pool row is brick_start[v] + brick_index[lattice_start[v] + l], at slot
//   (ix & 7) + 8 (iy & 7) + 64 (iz & 7).  A voxel of an absent brick (brick_index < 0) is D = 0, w = 0, as
//   tsdf_sparse.hpp says.
// The sparse render is therefore, by definition, tsdf_raycast of the densified pool (ops.tsdf_densify), bit for bit,
// depth and normals: the inside test, the validity test w >= min_weight on all 8 corners, the trilinear value, the hit,
// the end and the normal are those of tsdf_raycast.hpp.  The voxels a pool lacks are free space or unseen space, which
// a ray does not need: a hit only asks for the last positive sample before the crossing, and both lie within the
// truncation distance of a surface, where the bricks are.
//
// A sample.  The brick of the cell's base voxel is looked up first.  When the cell lies inside that brick (ix & 7 < 7,
// and so for y and z: 343 of 512 cells) that is one table read and the 16 loads come from one pair of rows.  Otherwise
// the bricks of all 8 corners are looked up before any is used.  A corner of an absent brick contributes D = 0, w = 0
// without a load from the pool.  Every index is checked before use: a table entry is read only inside the volume's
// part of brick_index [L], a pool row only when it lies in [0, B) -- tables that do not fit their dims give an
// unspecified image, and nothing out of range is read.
//
// Brick skipping.  When the base voxel's brick is absent and min_weight > 0, the sample is invalid whatever the other
// corners hold (w = 0 at the base corner), and so is every later sample whose base voxel is certainly in the same
// brick.  The ray is q(z) ~ o + z dir as in the box clip, every coordinate monotone in z.  The EXIT zout is taken by a
// slab test on the brick's box SHRUNK by one voxel on every side, [origin + voxel (8 b + 1), origin + voxel (8 b + 7)],
// so that its rounding (about 1e-6 of a voxel; the reciprocals of dir are formed once) cannot matter; and nothing is
// skipped unless sample k itself lies at least 1/16 voxel inside every face of the brick (g_a - 8 b_a in [1/16, 8 -
// 1/16], from the values the sample has in hand).  Between z_k and zout every coordinate then lies between its value at
// sample k and the far side of the shrunk slab: inside the brick by 1/16 voxel at least.  The samples skipped are k + 1
// .. floor((zout - depth_min) / step) - 1: the first sample that may have left the shrunk box, less one more.  Samples
// are always computed from k, the skipped ones would only have cleared `positive`, which this one clears, so a skip
// changes no bit; skip = 0 looks every sample up and is the switch that proves it, as clip = 0 is for the box clip.
// With min_weight <= 0 an absent brick is a valid D = 0 and nothing is skipped.  A brick is 8 voxels and the default
// step trunc / 2 = 2.5 voxels: a skip saves a table read or two, not hundreds; what the sparse march saves is that empty
// space costs one 4-byte read of a table that stays in the L2 instead of 16 loads from the volume.
//
// Growing a pool (ops.tsdf_extend).  The bricks of a sparse volume united with those that further frames flag under
// tsdf_sparse.hpp's allocation rule, in lattice order: the tables are those of one allocation over all the frames.
// Rows that existed move to their new place bit for bit; new rows hold D = 0, w = 0.  CONSEQUENCE: a brick allocated
// late holds only the frames integrated after it appeared.  Where earlier frames saw that space as free (t = 1, which
// the dense volume would have averaged in) it is not the dense value; where they did not see it at all it is.
//
// Continuing an integration (d3f_tsdf_sparse_integrate, into != 0): every existing slot of a row whose volume owns a
// frame in the call continues integrate_voxel_into from its stored (D, w); the rows of a volume without a frame, and
// the slots beyond dims, are left alone.  For fixed tables the frames [0, k) and then [k, F) into the result give
// the pool of one call bit for bit.
#pragma once
#include "tsdf_raycast.hpp"
#include "tsdf_sparse.hpp"

namespace d3f {
namespace raycast {

struct SparseLattice {      // one sparse volume: a sampler of cast_ray
  const float* D;             // the pool [rows, 512] of the whole batch
  const float* w;
  const int32_t* index;       // the volume's part of brick_index
  int64_t cells;              // how many of its entries may be read
  int64_t row0;               // brick_start[v]
  int64_t rows;               // B: a row at or beyond it is never read
  float ox, oy, oz, voxel;
  int nx, ny, nz;
  int nbx, nby;               // bricks along x and y
  bool skip;                  // brick skipping
};

// the pool row of lattice brick (bx, by, bz), or -1: absent, or not in the tables
D3F_HD inline int64_t brick_row(const SparseLattice& L, int bx, int by, int bz) {
  const int64_t l = ((int64_t)bz * L.nby + by) * (int64_t)L.nbx + bx;
  if (l < 0 || l >= L.cells) return -1;
  const int32_t rank = L.index[l];
  const int64_t row = L.row0 + rank;
  return (rank < 0 || row < 0 || row >= L.rows) ? -1 : row;
}

// sample() of tsdf_raycast.hpp with the corners taken from the pool; `absent`: the cell is inside the lattice and the
// brick of its base voxel is not there; b = (bx, by, bz) that brick and in[a] = g_a - 8 b_a the point's place in it
D3F_HD inline bool sample(const SparseLattice& L, float qx, float qy, float qz, float min_weight, float& value,
                          bool& absent, int b[3], float in[3]) {
  absent = false;
  const float gx = (qx - L.ox) / L.voxel, gy = (qy - L.oy) / L.voxel, gz = (qz - L.oz) / L.voxel;
  const float ix = floorf(gx), iy = floorf(gy), iz = floorf(gz);
  if (!(ix >= 0.0f && ix + 1.0f < (float)L.nx && iy >= 0.0f && iy + 1.0f < (float)L.ny && iz >= 0.0f &&
        iz + 1.0f < (float)L.nz))
    return false;
  const int vx = (int)ix, vy = (int)iy, vz = (int)iz;
  const int jx = vx & 7, jy = vy & 7, jz = vz & 7;
  b[0] = vx >> 3;
  b[1] = vy >> 3;
  b[2] = vz >> 3;
  in[0] = gx - (float)(8 * b[0]);
  in[1] = gy - (float)(8 * b[1]);
  in[2] = gz - (float)(8 * b[2]);
  const int64_t base = brick_row(L, b[0], b[1], b[2]);
  absent = base < 0;
  float d[8], c[8];          // D and w of the corners, x fastest
  if (jx < 7 && jy < 7 && jz < 7) {
    // the cell lies in the base voxel's brick: the 16 loads of one pair of rows, no branch between them
    if (absent) {
#pragma unroll
      for (int j = 0; j < 8; ++j) d[j] = c[j] = 0.0f;
    } else {
      const int64_t at = base * tsdf::kBrickVoxels + (jx + 8 * jy + 64 * jz);
#pragma unroll
      for (int j = 0; j < 8; ++j) c[j] = L.w[at + (j & 1) + 8 * ((j >> 1) & 1) + 64 * (j >> 2)];
#pragma unroll
      for (int j = 0; j < 8; ++j) d[j] = L.D[at + (j & 1) + 8 * ((j >> 1) & 1) + 64 * (j >> 2)];
    }
  } else {
    // the cell straddles 2, 4 or 8 bricks: all the lookups first, then the loads
    int64_t at[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int cx = vx + (j & 1), cy = vy + ((j >> 1) & 1), cz = vz + (j >> 2);
      const int64_t row = brick_row(L, cx >> 3, cy >> 3, cz >> 3);
      at[j] = row < 0 ? -1 : row * tsdf::kBrickVoxels + ((cx & 7) + 8 * (cy & 7) + 64 * (cz & 7));
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) c[j] = at[j] < 0 ? 0.0f : L.w[at[j]];
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = at[j] < 0 ? 0.0f : L.D[at[j]];
  }
  const bool weighted = (c[0] >= min_weight) & (c[1] >= min_weight) & (c[2] >= min_weight) & (c[3] >= min_weight) &
                        (c[4] >= min_weight) & (c[5] >= min_weight) & (c[6] >= min_weight) & (c[7] >= min_weight);
  const float fx = gx - ix, fy = gy - iy, fz = gz - iz;
  const float e00 = lerp(d[0], d[1], fx), e10 = lerp(d[2], d[3], fx);
  const float e01 = lerp(d[4], d[5], fx), e11 = lerp(d[6], d[7], fx);
  value = lerp(lerp(e00, e10, fy), lerp(e01, e11, fy), fz);
  return weighted;
}

D3F_HD inline bool sample(const SparseLattice& L, float qx, float qy, float qz, float min_weight, float& value) {
  bool absent;
  int b[3];
  float in[3];
  return sample(L, qx, qy, qz, min_weight, value, absent, b, in);
}

// one axis of the exit test: where the ray leaves [origin + voxel (8 b + 1), origin + voxel (8 b + 7)].  The
// reciprocal of dir does not depend on the sample: the compiler keeps it across the marching loop.
D3F_HD inline void brick_axis(float dir, float o, float origin, float voxel, int b, float& zout, bool& unknown) {
  if (dir == 0.0f) return;                    // the coordinate stays where sample k has it
  const float lo = origin + voxel * (float)(8 * b + 1), hi = origin + voxel * (float)(8 * b + 7);
  const float inv = 1.0f / dir;
  const float exit = fmaxf((lo - o) * inv, (hi - o) * inv);
  if (!(exit == exit)) unknown = true;        // a NaN
  zout = fminf(zout, exit);
}

// the last sample after k that is certainly in the absent brick b of sample k (k itself: none is); in[a] = g_a - 8 b_a,
// where sample k lies in that brick, in voxels
D3F_HD inline int skip_brick(const SparseLattice& L, const float* C, float x, float y, float step, float depth_min,
                             int k, const int b[3], const float in[3]) {
  const float margin = 0.0625f;
  if (!(in[0] >= margin && in[0] <= 8.0f - margin && in[1] >= margin && in[1] <= 8.0f - margin && in[2] >= margin &&
        in[2] <= 8.0f - margin))
    return k;                                 // too close to a face of the brick for anything to be certain
  float zout = 3.402823466e+38f;
  bool unknown = false;
  brick_axis((C[0] * x + C[1] * y) + C[2], C[3], L.ox, L.voxel, b[0], zout, unknown);
  brick_axis((C[4] * x + C[5] * y) + C[6], C[7], L.oy, L.voxel, b[1], zout, unknown);
  brick_axis((C[8] * x + C[9] * y) + C[10], C[11], L.oz, L.voxel, b[2], zout, unknown);
  if (unknown) return k;
  float next = floorf((zout - depth_min) * (1.0f / step));      // the first sample that may have left, less one
  next = fminf(next, (float)(kMaxSamples + 1));                  // bounded before the conversion
  if (!(next > (float)(k + 1))) return k;
  return (int)next - 1;
}

// march() of tsdf_raycast.hpp for a sparse volume: the sample, and the skip over an absent brick
D3F_HD inline bool march(const SparseLattice& L, const float* C, float x, float y, float step, float depth_min, int k,
                         const float q[3], float min_weight, float& value, int& last) {
  bool absent;
  int b[3];
  float in[3];
  const bool ok = sample(L, q[0], q[1], q[2], min_weight, value, absent, b, in);
  if (absent && L.skip && min_weight > 0.0f) last = skip_brick(L, C, x, y, step, depth_min, k, b, in);
  return ok;
}

}  // namespace raycast
}  // namespace d3f
