// Triangle meshes with normals straight from a sparse TSDF pool (tsdf_mesh_sparse.hip: d3f_tsdf_sparse_mesh and its
// host twin).  Stated in the terms of tsdf_mesh.hpp and tsdf_sparse.hpp, which it includes: everything here is
// __host__ __device__ and reads no state, all arithmetic is f32 in the order written there, and
// ops.tsdf_mesh_sparse_numpy restates it.
//
// The rule is tsdf_mesh.hpp unchanged -- COMPLETE cell, ACTIVE cell, crossing edge, vertex, normal, quad, the two
// triangles and their winding are that text (Hood, cell_complete, cell_crossings, face_mask, quad_triangles,
// cell_vertex) -- with ONE thing replaced: where the D and w of a voxel come from.
//   Voxel (ix, iy, iz) of volume v lies in lattice brick ((iz >> 3) nby + (iy >> 3)) nbx + (ix >> 3), whose pool row is
//   brick_start[v] + brick_index[lattice_start[v] + l], at slot (ix & 7) + 8 (iy & 7) + 64 (iz & 7).  A voxel of an
//   absent brick (brick_index < 0) is D = 0, w = 0 and is never VALID; so is a slot with i_a >= n_a and a voxel
//   outside the lattice, whatever min_weight is.
// The sparse mesh is therefore, by definition, tsdf_mesh of the densified pool (ops.tsdf_densify; for min_weight > 0,
// where a voxel of D = 0, w = 0 is not VALID there either): the same vertices, normals and faces bit for bit.  Only the
// order differs, and with it the numbering of the vertices.
//
// Output order.  Vertices: volume, pool row (which is brick in lattice order), slot of the cell's lowest voxel.
// Faces: volume, pool row and slot of the edge's lower voxel e, axis, a quad's two triangles consecutive; entries are
// int32 vertex indices LOCAL to their volume.  vertex_start, face_start [V + 1]: a volume without bricks owns an empty
// range, read where its rows would begin.  Capacities and the status bits are those of tsdf_mesh.hip.
//
// The halo.  Everything a brick's 512 slots need lies in the 10 x 10 x 10 voxels -1..8 per axis around it: the
// neighbourhood of a slot reaches one voxel each way, and the four cells around an edge reach one voxel down.  Those
// voxels live in the up to 27 bricks around the brick, which are looked up ONCE per brick (brick_neighbour(): through
// brick_index, -1 when the brick is absent or outside the lattice, every index bounded before use as in
// sparse_crossings()), not once per voxel.  halo_source() names the pool position of a halo voxel, or -1; a slot's
// Hood comes from the flags of the halo (hood_from() with a sampler) and a cell's 8 corner values from its D.  The
// cells around an edge can lie in four different bricks; one that reaches an absent brick is incomplete: no quad.
// Nothing outside brick_index [L], the tables and the pool [B, 512] is read.
//
// Equivalence to the densely integrated volume.  tsdf_sparse.hpp proves that every dense-VALID voxel lies in an
// allocated brick and that an allocated brick holds the dense D and w bit for bit; a voxel that is VALID here is in an
// allocated brick and so VALID there with the same values.  The VALID sets and their values coincide, and the mesh is
// a function of nothing else: the mesh of a pool that was allocated and integrated over the same frames in one go is
// the mesh of the densely integrated volume (tsdf_integrate + tsdf_mesh), bit for bit, up to the order above.
// This does NOT hold for bricks added late by ops.tsdf_extend (tsdf_raycast_sparse.hpp): a brick allocated late holds
// only the frames integrated after it appeared, and where earlier frames saw that space as free it is not the dense
// value.
#pragma once
#include "tsdf_mesh.hpp"
#include "tsdf_sparse.hpp"

namespace d3f {
namespace tsdf {

constexpr int kHaloEdge = 10;                    // voxels -1..8 per axis
constexpr int kHaloVoxels = 1000;
constexpr int kBrickWords = kBrickVoxels / 64;   // 64-bit words of one bit per slot

// halo voxel h of in-brick coordinates (hx, hy, hz) in -1..8
D3F_HD inline int halo_index(int hx, int hy, int hz) { return (hx + 1) + kHaloEdge * (hy + 1) + 100 * (hz + 1); }

// the pool row of the brick at offset j = hood_bit(dx, dy, dz) from pool row b of volume v, or -1: absent, outside
// the brick lattice, or not in the tables
D3F_HD inline int64_t brick_neighbour(const Bricks& k, int v, int64_t b, int j) {
  if (j == kHoodSelf) return b;
  const int32_t* n = k.dims + 3 * (size_t)v;
  const int32_t* c = k.brick_coord + 3 * (size_t)b;
  const int nb[3] = {c[0] + j % 3 - 1, c[1] + (j / 3) % 3 - 1, c[2] + j / 9 - 1};
  for (int a = 0; a < 3; ++a)
    if (nb[a] < 0 || nb[a] >= brick_count(n[a])) return -1;
  const int64_t l = k.lattice_start[v] + ((int64_t)nb[2] * brick_count(n[1]) + nb[1]) * (int64_t)brick_count(n[0]) + nb[0];
  if (l < 0 || l >= k.L) return -1;
  const int32_t rank = k.brick_index[l];
  if (rank < 0) return -1;
  const int64_t row = k.brick_start[v] + rank;
  return (row < 0 || row >= k.B) ? -1 : row;
}

// where halo voxel h = 0..999 of the brick at c[3] of a volume of dims n[3] lies in the pool, given the rows of the 27
// bricks around it (brick_neighbour()), or -1: outside the lattice, or in a brick that is not there
D3F_HD inline int64_t halo_source(const int32_t* n, const int32_t* c, const int64_t* rows, int h) {
  const int in[3] = {h % kHaloEdge - 1, (h / kHaloEdge) % kHaloEdge - 1, h / 100 - 1};
  int d[3];
  for (int a = 0; a < 3; ++a) {
    if (c[a] < 0 || c[a] >= brick_count(n[a])) return -1;
    const int i = c[a] * 8 + in[a];
    if (i < 0 || i >= n[a]) return -1;
    d[a] = in[a] < 0 ? -1 : (in[a] > 7 ? 1 : 0);
  }
  const int64_t row = rows[hood_bit(d[0], d[1], d[2])];
  return row < 0 ? -1 : row * kBrickVoxels + ((in[0] & 7) + 8 * (in[1] & 7) + 64 * (in[2] & 7));
}

// the flags of a halo voxel whose pool position is `at`: bit 0 = VALID, bit 1 = VALID and D < 0; *value = its D (0
// when it has none)
D3F_HD inline int halo_flags(const float* D, const float* w, int64_t at, float min_weight, float* value) {
  *value = 0.0f;
  if (at < 0) return 0;
  const float d = D[at];
  *value = d;
  if (!valid(d, w[at], min_weight)) return 0;
  return d < 0.0f ? 3 : 1;
}

// the neighbourhood of slot (x, y, z) = 0..7 of a brick from the flags [1000] of its halo
D3F_HD inline Hood halo_hood(const uint8_t* flags, int x, int y, int z) {
  return hood_from([&](int dx, int dy, int dz) { return (int)flags[halo_index(x + dx, y + dy, z + dz)]; });
}

// the D of the 8 corners of the cell of slot (x, y, z) from the halo's D [1000]
D3F_HD inline void halo_corners(const float* value, int x, int y, int z, float d[8]) {
  for (int c = 0; c < 8; ++c) d[c] = value[halo_index(x + (c & 1), y + ((c >> 1) & 1), z + ((c >> 2) & 1))];
}

// cell q = 0..3 around the edge of axis a that rises from slot (x, y, z): the offset j = hood_bit() of the brick that
// holds its lowest voxel (offsets in {-1, 0}) and that voxel's slot there
D3F_HD inline void face_cell_sparse(int x, int y, int z, int a, int q, int& j, int& slot) {
  int i[3] = {x, y, z};
  if (q == 0 || q == 3) i[(a + 1) % 3] -= 1;
  if (q == 0 || q == 1) i[(a + 2) % 3] -= 1;
  j = hood_bit(i[0] < 0 ? -1 : 0, i[1] < 0 ? -1 : 0, i[2] < 0 ? -1 : 0);
  slot = (i[0] & 7) + 8 * (i[1] & 7) + 64 * (i[2] & 7);
}

}  // namespace tsdf
}  // namespace d3f
