// What tsdf_mesh.hip and tsdf_mesh_sparse.hip share beyond the rule of tsdf_mesh.hpp and the scan of tsdf_batch.hpp: the
// outputs of a mesh call with their check, the workspace, and the two capacity rules -- a vertex beyond
// vertex_capacity, a triangle beyond face_capacity or with a vertex index beyond int32 is dropped and leaves its bit in
// the status.  Host and device run this text.  Included by .hip files only.
#pragma once
#include "tsdf_batch.hpp"
#include "tsdf_mesh.hpp"

namespace d3f {
namespace tsdf {

struct MeshOut {
  float* vertices;          // [vertex_capacity, 3]
  float* normals;           // [vertex_capacity, 3]
  int32_t* faces;           // [face_capacity, 3]
  int64_t* vertex_start;    // [V + 1]
  int64_t* face_start;      // [V + 1]
  int32_t* status;
  int64_t vertex_capacity, face_capacity;
};

// what an emit form and a twin ask of their outputs (the starts are asked for with the model's tables)
static inline bool mesh_out_ok(const float* origin, const float* voxel, const MeshOut& out) {
  return origin && voxel && out.status && out.vertex_capacity >= 0 && out.face_capacity >= 0 &&
         (out.vertex_capacity == 0 || (out.vertices && out.normals)) && (out.face_capacity == 0 || out.faces);
}

// the scans of the vertex counts and of the triangle counts of `blocks` blocks, and the ballots of their ACTIVE cells,
// `words` of 64 cells per block
struct MeshWs {
  BlockScan vertices, faces;
  uint64_t* active;        // [blocks * words]
  size_t bytes;
  MeshWs(void* ws, int64_t blocks, int words) {
    d3f::Carver c(ws);
    vertices.carve(c, blocks);
    faces.carve(c, blocks);
    active = c.take<uint64_t>((size_t)blocks * words);
    bytes = d3f::align_up(c.off, 256);
  }
};

// row pos of the vertices can be written; otherwise the vertex is dropped and `bits` says so
__host__ __device__ inline bool vertex_fits(const MeshOut& out, int64_t pos, int& bits) {
  if (pos >= 0 && pos < out.vertex_capacity) return true;
  bits |= D3F_TSDF_ST_OVERFLOW;
  return false;
}

// the quads of a voxel's edges (`quads`: face_mask()) as two triangles each into the rows from fpos on; returns the
// status bits.  inside = D < 0 at the voxel; row_of(a, n) gives the vertex row, LOCAL to its volume, of cell n = 0..3
// around the edge of axis a.
template <typename RowOf>
__host__ __device__ inline int write_quads(const MeshOut& out, int quads, bool inside, int64_t fpos, RowOf row_of) {
  int bits = 0;
  for (int a = 0; a < 3; ++a) {
    if (!((quads >> a) & 1)) continue;
    if (fpos < 0 || fpos >= out.face_capacity) {
      bits |= D3F_TSDF_ST_FACE_OVERFLOW;
      fpos += 2;
      continue;
    }
    int32_t q[4], t[6];
    bool fits = true;      // false: more than 2^31 - 1 vertices in one volume, and no wrapped index is written
    for (int n = 0; n < 4; ++n) {
      const int64_t row = row_of(a, n);
      fits = fits && row >= 0 && row <= 0x7fffffff;
      q[n] = (int32_t)row;
    }
    quad_triangles(q, inside, t);
    for (int tri = 0; tri < 2; ++tri, ++fpos) {
      if (fpos >= out.face_capacity)
        bits |= D3F_TSDF_ST_FACE_OVERFLOW;
      else if (!fits)
        bits |= D3F_TSDF_ST_OVERFLOW;
      else
        for (int r = 0; r < 3; ++r) out.faces[3 * fpos + r] = t[3 * tri + r];
    }
  }
  return bits;
}

}  // namespace tsdf
}  // namespace d3f
