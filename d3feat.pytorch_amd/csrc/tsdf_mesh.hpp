// Triangle meshes with normals from the TSDF volumes of tsdf.hpp (tsdf_mesh.hip; d3f_tsdf_mesh and its host twin): dual
// contouring of the lattice ("naive surface nets"), which needs no case table.  Everything here is __host__ __device__
// and reads no state: the kernels and the host twin run this text, and ops.tsdf_mesh_numpy restates it.  The terms are
// those of tsdf.hpp (VALID, lattice(), crossing_point()); all arithmetic is f32 in exactly the order written.  The
// library is built with -ffp-contract=off and f32 division and sqrtf are correctly rounded on both sides (hipcc's
// default), so device, host twin and NumPy agree bit for bit.
//
// Cell.  The cell of voxel (ix, iy, iz) spans the corners (ix..ix+1, iy..iy+1, iz..iz+1); it exists only when ix+1 <
// nx, iy+1 < ny and iz+1 < nz, and its index is the local index of that lowest voxel.  A cell is COMPLETE when all 8
// corners are VALID.  No corner beyond the volume's own voxel range is read (the guard of crossings()).
// Cell edges, in a fixed order of 12: axis a = 0, 1, 2; within an axis the offsets (d1, d2) on the two other axes, taken
// in ascending axis order, (0,0), (1,0), (0,1), (1,1).  An edge CROSSES when (D_lower < 0) != (D_upper < 0).
// Vertex.  A COMPLETE cell with k >= 1 crossing edges is ACTIVE and owns one vertex: with p_i the point crossing_point()
// makes for its i-th crossing edge in that order (the point tsdf_extract emits for the edge),
//   s = ((p_1 + p_2) + ...) per component;   vertex = s / (float)k.
// Normal of that vertex: g_a = the sequential sum, over the 4 edges of axis a in the same order and crossing or not, of
// D_upper - D_lower;  n = g / sqrtf((g0 g0 + g1 g1) + g2 g2), or (0, 0, 0) when that length is 0 or not finite.  It
// points towards positive D: free space, the camera's side.
// Faces.  A crossing lattice edge with lower voxel e and axis a, b = (a + 1) % 3, c = (a + 2) % 3: the four cells around
// it are q0..q3 = e + (db, dc) for (-1,-1), (0,-1), (0,0), (-1,0) on the axes (b, c).  The edge emits a quad only if all
// four exist and are COMPLETE (they are then ACTIVE), as two triangles: (q0,q1,q2), (q0,q2,q3) if D[e] < 0, otherwise
// (q3,q2,q1), (q3,q1,q0) -- counter-clockwise seen from positive D.
// Output order.  Vertices: volume, cell index.  Faces: volume, local index of e, axis, a quad's two triangles
// consecutive; entries are int32 vertex indices LOCAL to their volume.  A pure function of the volume.  A vertex that
// no face uses is legal (the rim of an observed region).
#pragma once
#include "tsdf.hpp"

namespace d3f {
namespace tsdf {

// The 27 voxels around voxel e, bit (dx + 1) + 3 (dy + 1) + 9 (dz + 1) for the offset (dx, dy, dz) in {-1, 0, 1}^3:
// ok = VALID (a voxel outside the lattice or the volume's voxel range is not), neg = D < 0.
struct Hood {
  uint32_t ok, neg;
};
constexpr int kHoodSelf = 13;                    // the bit of e itself
constexpr uint32_t kCellCorners = 0x361Bu;       // the 8 corners of the cell whose lowest voxel is bit 0

D3F_HD inline int hood_bit(int dx, int dy, int dz) { return (dx + 1) + 3 * (dy + 1) + 9 * (dz + 1); }
D3F_HD inline int hood_step(int a) { return a == 0 ? 1 : (a == 1 ? 3 : 9); }

// the neighbourhood of the voxel at local index `local` of a lattice nx x ny x nz whose `count` values of D / w start at
// Dv / wv.  An invalid e gives ok = 0 at once: neither its cell nor any of its edges can emit.
D3F_HD inline Hood hood(const float* Dv, const float* wv, int64_t local, int64_t count, int ix, int iy, int iz, int nx,
                        int ny, int nz, float min_weight) {
  Hood h = {0u, 0u};
  if (local < 0 || local >= count || !valid(Dv[local], wv[local], min_weight)) return h;
  for (int dz = -1; dz <= 1; ++dz)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int x = ix + dx, y = iy + dy, z = iz + dz;
        if (x < 0 || x >= nx || y < 0 || y >= ny || z < 0 || z >= nz) continue;
        const int64_t i = local + dx + (int64_t)nx * dy + (int64_t)nx * (int64_t)ny * dz;
        if (i < 0 || i >= count) continue;
        const float D = Dv[i];
        if (!valid(D, wv[i], min_weight)) continue;
        const uint32_t bit = 1u << hood_bit(dx, dy, dz);
        h.ok |= bit;
        if (D < 0.0f) h.neg |= bit;
      }
  return h;
}

// the same neighbourhood from a sampler instead of a dense pointer (tsdf_mesh_sparse.hpp): sample(dx, dy, dz) gives
// bit 0 = the voxel e + (dx, dy, dz) is VALID, bit 1 = it is VALID and its D < 0
template <typename Sample>
D3F_HD inline Hood hood_from(Sample sample) {
  Hood h = {0u, 0u};
  if (!(sample(0, 0, 0) & 1)) return h;
  for (int dz = -1; dz <= 1; ++dz)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int f = sample(dx, dy, dz);
        if (!(f & 1)) continue;
        const uint32_t bit = 1u << hood_bit(dx, dy, dz);
        h.ok |= bit;
        if (f & 2) h.neg |= bit;
      }
  return h;
}

// the cell whose lowest voxel is bit `lowest` of the neighbourhood (an offset in {-1, 0}^3): exists and is COMPLETE
D3F_HD inline bool cell_complete(const Hood& h, int lowest) {
  const uint32_t m = kCellCorners << lowest;
  return (h.ok & m) == m;
}

// the two corners (bits 0..2 = offsets on x, y, z) of edge j = 0..3 of axis a of a cell, in the order of the rule
D3F_HD inline void cell_edge(int a, int j, int& lower, int& upper) {
  const int a1 = a == 0 ? 1 : 0, a2 = a == 2 ? 1 : 2;      // the two other axes, ascending
  lower = ((j & 1) << a1) | (((j >> 1) & 1) << a2);
  upper = lower | (1 << a);
}

// the crossing edges of e's own cell: bit 4 a + j; 0 unless the cell is COMPLETE.  Non-zero: the cell is ACTIVE.
D3F_HD inline int cell_crossings(const Hood& h) {
  if (!cell_complete(h, kHoodSelf)) return 0;
  int mask = 0;
  for (int a = 0; a < 3; ++a)
    for (int j = 0; j < 4; ++j) {
      int c0, c1;
      cell_edge(a, j, c0, c1);
      const int b0 = hood_bit(c0 & 1, (c0 >> 1) & 1, (c0 >> 2) & 1), b1 = hood_bit(c1 & 1, (c1 >> 1) & 1, (c1 >> 2) & 1);
      if (((h.neg >> b0) & 1u) != ((h.neg >> b1) & 1u)) mask |= 1 << (4 * a + j);
    }
  return mask;
}

// the quads of the three lattice edges that rise from e: bit a is set when the edge of axis a emits one
D3F_HD inline int face_mask(const Hood& h) {
  int mask = 0;
  for (int a = 0; a < 3; ++a) {
    if (((h.neg >> kHoodSelf) & 1u) == ((h.neg >> (kHoodSelf + hood_step(a))) & 1u)) continue;
    const int sb = hood_step((a + 1) % 3), sc = hood_step((a + 2) % 3);
    bool all = true;
    for (int q = 0; q < 4; ++q)
      all = all && cell_complete(h, kHoodSelf - ((q == 0 || q == 3) ? sb : 0) - ((q == 0 || q == 1) ? sc : 0));
    if (all) mask |= 1 << a;
  }
  return mask;
}

// the local index of cell q = 0..3 around the edge of axis a that rises from the voxel at `local`
D3F_HD inline int64_t face_cell(int64_t local, int nx, int ny, int a, int q) {
  const int64_t step[3] = {1, (int64_t)nx, (int64_t)nx * (int64_t)ny};
  const int64_t db = (q == 0 || q == 3) ? -1 : 0, dc = (q == 0 || q == 1) ? -1 : 0;
  return local + db * step[(a + 1) % 3] + dc * step[(a + 2) % 3];
}

// the two triangles of a quad from the vertex indices of q0..q3; inside = D[e] < 0
D3F_HD inline void quad_triangles(const int32_t q[4], bool inside, int32_t* out) {
  if (inside) {
    out[0] = q[0]; out[1] = q[1]; out[2] = q[2];
    out[3] = q[0]; out[4] = q[2]; out[5] = q[3];
  } else {
    out[0] = q[3]; out[1] = q[2]; out[2] = q[1];
    out[3] = q[3]; out[4] = q[1]; out[5] = q[0];
  }
}

// vertex[3] and normal[3] of the ACTIVE cell of voxel (ix, iy, iz) from the D of its 8 corners (d[c], bits 0..2 of c =
// the offsets on x, y, z), whose crossing edges are `edges` (cell_crossings()).  The point of an edge is
// crossing_point()'s, in its arithmetic: the lower corner's lattice point moved by voxel * (|D0| / (|D0| + |D1|)).
D3F_HD inline void cell_vertex(const float d[8], int ix, int iy, int iz, int edges, const float* origin, float voxel,
                               float* vertex, float* normal) {
  float s[3] = {0.0f, 0.0f, 0.0f}, g[3];
  int k = 0;
  for (int a = 0; a < 3; ++a) {
    float sum = 0.0f;
    for (int j = 0; j < 4; ++j) {
      int c0, c1;
      cell_edge(a, j, c0, c1);
      const float diff = d[c1] - d[c0];
      sum = j == 0 ? diff : sum + diff;
      if (!((edges >> (4 * a + j)) & 1)) continue;
      const float a0 = fabsf(d[c0]), a1 = fabsf(d[c1]);
      float p[3] = {lattice(origin[0], voxel, ix + (c0 & 1)), lattice(origin[1], voxel, iy + ((c0 >> 1) & 1)),
                    lattice(origin[2], voxel, iz + ((c0 >> 2) & 1))};
      p[a] = p[a] + voxel * (a0 / (a0 + a1));
      for (int r = 0; r < 3; ++r) s[r] = k == 0 ? p[r] : s[r] + p[r];
      ++k;
    }
    g[a] = sum;
  }
  const float len = sqrtf((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
  const bool ok = len > 0.0f && len <= 3.402823466e+38f;      // neither 0 nor infinite nor NaN
  for (int r = 0; r < 3; ++r) {
    vertex[r] = s[r] / (float)k;
    normal[r] = ok ? g[r] / len : 0.0f;
  }
}

// the same for the ACTIVE cell at `local` = (ix, iy, iz) of a dense lattice (every corner is then inside the volume's
// voxel range): the 8 corners are read and the form above does the rest
D3F_HD inline void cell_vertex(const float* Dv, int64_t local, int ix, int iy, int iz, int nx, int ny, int edges,
                               const float* origin, float voxel, float* vertex, float* normal) {
  const int64_t step[3] = {1, (int64_t)nx, (int64_t)nx * (int64_t)ny};
  float d[8];
  for (int c = 0; c < 8; ++c) d[c] = Dv[local + (c & 1) * step[0] + ((c >> 1) & 1) * step[1] + ((c >> 2) & 1) * step[2]];
  cell_vertex(d, ix, iy, iz, edges, origin, voxel, vertex, normal);
}

}  // namespace tsdf
}  // namespace d3f
