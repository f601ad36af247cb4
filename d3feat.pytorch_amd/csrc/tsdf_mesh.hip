// Triangle meshes with normals from a batch of TSDF volumes (include/d3feat_hip.h: d3f_tsdf_mesh_count, d3f_tsdf_mesh;
// the rule is csrc/tsdf_mesh.hpp).  The shape of tsdf_extract.hip: one thread per voxel, 256 per workgroup.
//   count   per block the ACTIVE cells (vertices) and the triangles, in one pass; the ballot of ACTIVE cells is kept,
//           one bit per voxel (a 64-bit word per wave).
//   scan    the two-level exclusive scan of tsdf_batch.hpp, over the vertex counts and over the triangle counts.
//   emit    recomputes the neighbourhood and writes vertices and normals at group offset + block offset + in-block
//           rank, and the triangles likewise.  The vertex index of a neighbouring cell is its block's scanned offset
//           plus the popcount of the ballot bits below it (vertex_position()): no dense index volume, no atomic decides
//           a position, no floating-point atomics.
// A voxel that is not VALID ends after one read of D and w (it is a corner of its own cell and of every cell around its
// three edges), which is most of a fragment; the others read their 27 neighbours from cache.
// The host twin runs the same tsdf_mesh.hpp text on the CPU and makes no GPU call.
#include <vector>

#include "tsdf_mesh_batch.hpp"   // includes tsdf_batch.hpp and tsdf_mesh.hpp

namespace {

using namespace d3f::tsdf;

constexpr int kWords = kWaves;            // ballot words per block: one per wave

// what global voxel g of volume v emits: its neighbourhood, and where it lies
struct Voxel {
  Hood h;
  int64_t local;
  int ix, iy, iz, nx, ny;
};
__host__ __device__ inline Voxel look(const Volumes& b, const float* D, const float* w, float min_weight, int v,
                                      int64_t g) {
  Voxel x;
  int nz;
  const int64_t base = b.vol_start[v];
  x.local = g - base;
  locate(b, v, x.local, x.ix, x.iy, x.iz, x.nx, x.ny, nz);
  x.h = hood(D + base, w + base, x.local, b.vol_start[v + 1] - base, x.ix, x.iy, x.iz, x.nx, x.ny, nz, min_weight);
  return x;
}

__global__ void __launch_bounds__(kThreads) mesh_count_kernel(Volumes b, const float* __restrict__ D,
                                                              const float* __restrict__ w, float min_weight,
                                                              int32_t* __restrict__ vertex_count,
                                                              int32_t* __restrict__ face_count,
                                                              uint64_t* __restrict__ active) {
  __shared__ int wave_total[kWaves];
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  int is_active = 0, triangles = 0;
  if (g < b.total) {
    const Voxel x = look(b, D, w, min_weight, owner(b.vol_start, b.V, g), g);
    if (x.h.ok) {
      is_active = cell_crossings(x.h) != 0;
      triangles = 2 * popcount3(face_mask(x.h));
    }
  }
  const unsigned long long ballot = __ballot(is_active);
  if (d3f::lane_id() == 0) active[(size_t)blockIdx.x * kWaves + threadIdx.x / D3F_WAVE] = ballot;
  const int nv = workgroup_sum(is_active, wave_total);
  __syncthreads();                                 // wave_total is written again
  const int nf = workgroup_sum(triangles, wave_total);
  if (threadIdx.x == 0) {
    vertex_count[blockIdx.x] = nv;
    face_count[blockIdx.x] = nf;
  }
}

// the number of ACTIVE cells below global voxel g: the global row of g's vertex when its cell is ACTIVE
template <typename Offsets, typename Words>
__host__ __device__ inline int64_t vertex_position(const Offsets* block_offset, const Offsets* group_offset,
                                                   const Words* active, int64_t g) {
  const int64_t block = g / kThreads, word = g / D3F_WAVE;
  int64_t pos = group_offset[block / kScanThreads] + block_offset[block];
  for (int64_t k = block * kWaves; k < word; ++k) pos += __builtin_popcountll(active[k]);
  return pos + __builtin_popcountll(active[word] & ((1ull << (g % D3F_WAVE)) - 1ull));
}

// the vertex of voxel x's ACTIVE cell into row pos, the triangles of its edges into the rows from fpos on; returns the
// status bits.  vertex_of(global voxel) gives the global row of that voxel's vertex.
template <typename VertexOf>
__host__ __device__ inline int emit_voxel(const Volumes& b, const float* D, int v, const Voxel& x, int edges, int quads,
                                          int64_t pos, int64_t fpos, const MeshOut& out, VertexOf vertex_of) {
  int bits = 0;
  const int64_t base = b.vol_start[v];
  if (edges && vertex_fits(out, pos, bits))
    cell_vertex(D + base, x.local, x.ix, x.iy, x.iz, x.nx, x.ny, edges, b.origin + 3 * v, b.voxel[v],
                out.vertices + 3 * pos, out.normals + 3 * pos);
  if (!quads) return bits;
  const int64_t first = vertex_of(base);          // vertex_start[v]
  return bits | write_quads(out, quads, (x.h.neg >> kHoodSelf) & 1u, fpos, [&](int a, int n) {
           return vertex_of(base + face_cell(x.local, x.nx, x.ny, a, n)) - first;
         });
}

__global__ void __launch_bounds__(kThreads) mesh_emit_kernel(Volumes b, const float* __restrict__ D,
                                                             const float* __restrict__ w, float min_weight,
                                                             const int64_t* __restrict__ v_block_offset,
                                                             const int64_t* __restrict__ v_group_offset,
                                                             const int64_t* __restrict__ f_block_offset,
                                                             const int64_t* __restrict__ f_group_offset,
                                                             const uint64_t* __restrict__ active, MeshOut out) {
  __shared__ int wave_vertices[kWaves], wave_quads[kWaves];
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const bool live = g < b.total;
  Voxel x = {};
  int v = 0, edges = 0, quads = 0;
  if (live) {
    v = owner(b.vol_start, b.V, g);
    x = look(b, D, w, min_weight, v, g);
    if (x.h.ok) {
      edges = cell_crossings(x.h);
      quads = face_mask(x.h);
    }
  }
  const int wave = (int)threadIdx.x / D3F_WAVE;
  int v_before = rank_in_wave(edges != 0, wave_vertices, wave), q_before = rank_in_wave(quads, wave_quads, wave);
  __syncthreads();
  v_before += words_below(wave_vertices, wave);
  const int f_before = 2 * (q_before + words_below(wave_quads, wave));
  if (!live) return;
  const int64_t group = blockIdx.x / kScanThreads;
  const int64_t pos = v_group_offset[group] + v_block_offset[blockIdx.x] + v_before;
  const int64_t fpos = f_group_offset[group] + f_block_offset[blockIdx.x] + f_before;
  if (x.local == 0) {                             // the first voxel of a volume: where the volume's rows begin
    out.vertex_start[v] = pos;
    out.face_start[v] = fpos;
  }
  if (!edges && !quads) return;
  const int bits = emit_voxel(b, D, v, x, edges, quads, pos, fpos, out, [&](int64_t voxel) {
    return vertex_position(v_block_offset, v_group_offset, active, voxel);
  });
  if (bits) atomicOr(out.status, bits);
}

int run_mesh_count(const Volumes& b, const float* D, const float* w, float min_weight, int64_t* vertex_start,
                   int64_t* face_start, const MeshWs& x, int64_t blocks, hipStream_t stream) {
  mesh_count_kernel<<<(unsigned)blocks, kThreads, 0, stream>>>(b, D, w, min_weight, x.vertices.block_count,
                                                              x.faces.block_count, x.active);
  D3F_LAUNCH_CHECK();
  const int rc = run_block_scan(x.vertices, blocks, vertex_start + b.V, stream);
  return rc != D3F_OK ? rc : run_block_scan(x.faces, blocks, face_start + b.V, stream);
}

bool mesh_args_ok(const float* D, const float* w, const int64_t* vol_start, const int32_t* dims, int V, int64_t total,
                  const int64_t* vertex_start, const int64_t* face_start) {
  return batch_ok(V, total) && total > 0 && voxel_blocks(total) <= 0x7fffffff && D && w && vol_start && dims &&
         vertex_start && face_start;
}

}  // namespace

extern "C" {

size_t d3f_tsdf_mesh_ws_bytes(int64_t total_voxels) {
  if (total_voxels < 0) return 0;
  return MeshWs(nullptr, voxel_blocks(total_voxels), kWords).bytes + 256;
}

int d3f_tsdf_mesh_count(const float* D, const float* w, const int64_t* vol_start, const int32_t* dims, int V,
                        int64_t total_voxels, float min_weight, int64_t* vertex_start, int64_t* face_start, void* ws,
                        size_t ws_bytes, void* stream) {
  if (!mesh_args_ok(D, w, vol_start, dims, V, total_voxels, vertex_start, face_start) || !ws) return D3F_EINVAL;
  const int64_t blocks = voxel_blocks(total_voxels);
  const MeshWs x(ws, blocks, kWords);
  if (ws_bytes < x.bytes) return D3F_EWORKSPACE;
  const Volumes b = {vol_start, nullptr, dims, nullptr, V, total_voxels};
  return run_mesh_count(b, D, w, min_weight, vertex_start, face_start, x, blocks, (hipStream_t)stream);
}

int d3f_tsdf_mesh(const float* D, const float* w, const int64_t* vol_start, const float* origin, const int32_t* dims,
                  const float* voxel, int V, int64_t total_voxels, float min_weight, int counted,
                  int64_t vertex_capacity, int64_t face_capacity, float* vertices, float* normals, int32_t* faces,
                  int64_t* vertex_start, int64_t* face_start, int32_t* status, void* ws, size_t ws_bytes,
                  void* stream) {
  const MeshOut out = {vertices, normals, faces, vertex_start, face_start, status, vertex_capacity, face_capacity};
  if (!mesh_args_ok(D, w, vol_start, dims, V, total_voxels, vertex_start, face_start) || !mesh_out_ok(origin, voxel, out) ||
      !ws)
    return D3F_EINVAL;
  const int64_t blocks = voxel_blocks(total_voxels);
  const MeshWs x(ws, blocks, kWords);
  if (ws_bytes < x.bytes) return D3F_EWORKSPACE;
  const Volumes b = {vol_start, origin, dims, voxel, V, total_voxels};
  if (!counted) {
    const int rc = run_mesh_count(b, D, w, min_weight, vertex_start, face_start, x, blocks, (hipStream_t)stream);
    if (rc != D3F_OK) return rc;
  }
  mesh_emit_kernel<<<(unsigned)blocks, kThreads, 0, (hipStream_t)stream>>>(
      b, D, w, min_weight, x.vertices.block_offset, x.vertices.group_offset, x.faces.block_offset, x.faces.group_offset,
      x.active, out);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_tsdf_mesh_host(const float* D, const float* w, const int64_t* vol_start, const float* origin,
                       const int32_t* dims, const float* voxel, int V, int64_t total_voxels, float min_weight,
                       int64_t vertex_capacity, int64_t face_capacity, float* vertices, float* normals, int32_t* faces,
                       int64_t* vertex_start, int64_t* face_start, int32_t* status) {
  const MeshOut out = {vertices, normals, faces, vertex_start, face_start, status, vertex_capacity, face_capacity};
  if (!mesh_args_ok(D, w, vol_start, dims, V, total_voxels, vertex_start, face_start) || !mesh_out_ok(origin, voxel, out) ||
      !host_layout_ok(vol_start, dims, V, total_voxels))
    return D3F_EINVAL;
  const Volumes b = {vol_start, origin, dims, voxel, V, total_voxels};
  // the device's own bookkeeping: a bit per voxel and the ACTIVE cells below each block (all of them: one group)
  const int64_t blocks = voxel_blocks(total_voxels);
  std::vector<uint64_t> active((size_t)blocks * kWaves, 0);
  std::vector<int64_t> block_offset((size_t)blocks, 0), group_offset((size_t)(blocks / kScanThreads + 1), 0);
  for (int v = 0; v < V; ++v)
    for (int64_t g = vol_start[v]; g < vol_start[v + 1]; ++g)
      if (cell_crossings(look(b, D, w, min_weight, v, g).h)) active[(size_t)(g / D3F_WAVE)] |= 1ull << (g % D3F_WAVE);
  int64_t pos = 0;
  for (int64_t k = 0; k < blocks; ++k) {
    block_offset[(size_t)k] = pos;
    for (int j = 0; j < kWaves; ++j) pos += __builtin_popcountll(active[(size_t)(k * kWaves + j)]);
  }
  const auto vertex_of = [&](int64_t voxel_index) {
    return vertex_position(block_offset.data(), group_offset.data(), active.data(), voxel_index);
  };
  int64_t fpos = 0;
  for (int v = 0; v < V; ++v) {
    vertex_start[v] = vertex_of(vol_start[v]);
    face_start[v] = fpos;
    for (int64_t g = vol_start[v]; g < vol_start[v + 1]; ++g) {
      const Voxel x = look(b, D, w, min_weight, v, g);
      if (!x.h.ok) continue;
      const int edges = cell_crossings(x.h), quads = face_mask(x.h);
      *status |= emit_voxel(b, D, v, x, edges, quads, vertex_of(g), fpos, out, vertex_of);
      fpos += 2 * popcount3(quads);
    }
  }
  vertex_start[V] = pos;
  face_start[V] = fpos;
  return D3F_OK;
}

}  // extern "C"
