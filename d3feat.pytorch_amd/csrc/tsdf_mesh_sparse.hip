// Triangle meshes with normals straight from a sparse TSDF pool (include/d3feat_hip.h: d3f_tsdf_sparse_mesh_count,
// d3f_tsdf_sparse_mesh; the rule is csrc/tsdf_mesh_sparse.hpp).  The shape of tsdf_mesh.hip with bricks for blocks:
// one workgroup of 256 threads per pool row, each thread owning the slots t and t + 256.
//   stage   threads 0..26 resolve the bricks around the row once (brick_neighbour()); then the workgroup loads the
//           10 x 10 x 10 halo into LDS: 4000 bytes of D and one byte of flags (VALID, D < 0) per voxel, every thread
//           writing its own entries.  A slot forms its Hood from the flags and a cell's corners come from the D: after
//           the stage neither pass reads the pool or brick_index again.
//   count   per row the ACTIVE cells (vertices) and the triangles; the ballot of ACTIVE cells is kept, 8 words of 64
//           bits per row (word = slot / 64).
//   scan    the two-level exclusive scan of tsdf_batch.hpp over the rows' vertex counts and triangle counts; then
//           vertex_start / face_start are read where a volume's rows begin (as sparse_point_start_kernel does).
//   emit    stages the halo again and writes vertices and normals at group offset + row offset + rank inside the row, and
//           the triangles likewise.  The vertex of a neighbouring cell, in this row or one of the 7 rows below it, is its
//           row's scanned offset plus the popcount of that row's ballot words below the slot (vertex_position()): no
//           dense index volume, no hash, no atomic decides a position; the only atomic is the atomicOr on the status.
// The host twin runs the same tsdf_mesh_sparse.hpp text on the CPU, halo and all, and makes no GPU call.
//
// Resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):
//   sparse_mesh_count_kernel  VGPRs 34, SGPRs 55, no scratch, LDS 5248 bytes, 8 waves per SIMD
//   sparse_mesh_emit_kernel   VGPRs 56, SGPRs 79, no scratch, LDS 5280 bytes, 8 waves per SIMD
#include <vector>

#include "tsdf_mesh_batch.hpp"   // includes tsdf_batch.hpp and tsdf_mesh.hpp
#include "tsdf_mesh_sparse.hpp"

namespace {

using namespace d3f::tsdf;

constexpr int kSlotsPerThread = kBrickVoxels / kThreads;

struct Halo {
  float value[kHaloVoxels];      // D
  uint8_t flags[kHaloVoxels];    // halo_flags()
  int64_t rows[27];              // brick_neighbour()
};

// the halo of pool row b of volume v into LDS; ends with a barrier
__device__ inline void stage_halo(const Bricks& k, const float* __restrict__ D, const float* __restrict__ w,
                                  float min_weight, int v, int64_t b, Halo& halo) {
  if (threadIdx.x < 27) halo.rows[threadIdx.x] = brick_neighbour(k, v, b, (int)threadIdx.x);
  __syncthreads();
  for (int h = (int)threadIdx.x; h < kHaloVoxels; h += kThreads) {
    float value;
    const int64_t at = halo_source(k.dims + 3 * (size_t)v, k.brick_coord + 3 * (size_t)b, halo.rows, h);
    halo.flags[h] = (uint8_t)halo_flags(D, w, at, min_weight, &value);
    halo.value[h] = value;
  }
  __syncthreads();
}

__host__ inline void stage_halo_host(const Bricks& k, const float* D, const float* w, float min_weight, int v, int64_t b,
                                     Halo& halo) {
  for (int j = 0; j < 27; ++j) halo.rows[j] = brick_neighbour(k, v, b, j);
  for (int h = 0; h < kHaloVoxels; ++h) {
    const int64_t at = halo_source(k.dims + 3 * (size_t)v, k.brick_coord + 3 * (size_t)b, halo.rows, h);
    halo.flags[h] = (uint8_t)halo_flags(D, w, at, min_weight, halo.value + h);
  }
}

// what slot s of a staged brick emits: its neighbourhood, its cell's crossing edges and the quads of its three edges
struct Slot {
  Hood h;
  int x, y, z, edges, quads;
};
__host__ __device__ inline Slot look(const Halo& halo, int s) {
  Slot t;
  t.x = s & 7;
  t.y = (s >> 3) & 7;
  t.z = s >> 6;
  t.h = halo_hood(halo.flags, t.x, t.y, t.z);
  t.edges = t.h.ok ? cell_crossings(t.h) : 0;
  t.quads = t.h.ok ? face_mask(t.h) : 0;
  return t;
}

__global__ void __launch_bounds__(kThreads) sparse_mesh_count_kernel(Bricks k, const float* __restrict__ D,
                                                                     const float* __restrict__ w, float min_weight,
                                                                     int32_t* __restrict__ vertex_count,
                                                                     int32_t* __restrict__ face_count,
                                                                     uint64_t* __restrict__ active) {
  __shared__ Halo halo;
  __shared__ int wave_vertices[kWaves], wave_triangles[kWaves];
  const int64_t b = (int64_t)blockIdx.x;
  if (b >= k.B) return;                                   // uniform: the whole workgroup
  stage_halo(k, D, w, min_weight, owner(k.brick_start, k.V, b), b, halo);
  const int wave = (int)threadIdx.x / D3F_WAVE;
  int nv = 0, nf = 0;
#pragma unroll
  for (int half = 0; half < kSlotsPerThread; ++half) {
    const Slot t = look(halo, half * kThreads + (int)threadIdx.x);
    const unsigned long long ballot = __ballot(t.edges != 0);
    if (d3f::lane_id() == 0) active[(size_t)b * kBrickWords + half * kWaves + wave] = ballot;
    nv += t.edges != 0;
    nf += 2 * popcount3(t.quads);
  }
  nv = workgroup_sum(nv, wave_vertices);
  nf = workgroup_sum(nf, wave_triangles);
  if (threadIdx.x == 0) {
    vertex_count[b] = nv;
    face_count[b] = nf;
  }
}

// the rows before the first pool row of volume v (a volume without bricks owns no row: the prefix is read where its
// rows would begin); start[V] is the scan's grand total, already written
__global__ void __launch_bounds__(kThreads) sparse_mesh_start_kernel(const int64_t* __restrict__ brick_start, int V,
                                                                     int64_t B, BlockScan vs, BlockScan fs,
                                                                     int64_t* vertex_start, int64_t* face_start) {
  const int v = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (v >= V) return;
  const int64_t first = brick_start[v];
  const bool has = first >= 0 && first < B;
  vertex_start[v] = has ? vs.group_offset[first / kScanThreads] + vs.block_offset[first] : vertex_start[V];
  face_start[v] = has ? fs.group_offset[first / kScanThreads] + fs.block_offset[first] : face_start[V];
}

// the number of ACTIVE cells below slot s of pool row `row`: the global row of that cell's vertex when it is ACTIVE
template <typename Words>
__host__ __device__ inline int64_t vertex_position(const int64_t* block_offset, const int64_t* group_offset,
                                                   const Words* active, int64_t row, int s) {
  int64_t pos = group_offset[row / kScanThreads] + block_offset[row];
  const Words* words = active + row * kBrickWords;
  for (int j = 0; j < (s >> 6); ++j) pos += __builtin_popcountll(words[j]);
  return pos + __builtin_popcountll(words[s >> 6] & ((1ull << (s & 63)) - 1ull));
}

// the vertex of slot t's ACTIVE cell into row pos, the triangles of its edges into the rows from fpos on; returns the
// status bits.  vertex_of(pool row, slot) gives the global row of that cell's vertex; `first` = vertex_start[v].
template <typename VertexOf>
__host__ __device__ inline int emit_slot(const Bricks& k, const Halo& halo, int v, int64_t b, const Slot& t, int64_t pos,
                                         int64_t fpos, int64_t first, const MeshOut& out, VertexOf vertex_of) {
  int bits = 0;
  if (t.edges && vertex_fits(out, pos, bits)) {
    const int32_t* c = k.brick_coord + 3 * (size_t)b;
    float d[8];
    halo_corners(halo.value, t.x, t.y, t.z, d);
    cell_vertex(d, c[0] * 8 + t.x, c[1] * 8 + t.y, c[2] * 8 + t.z, t.edges, k.origin + 3 * (size_t)v, k.voxel[v],
                out.vertices + 3 * pos, out.normals + 3 * pos);
  }
  return bits | write_quads(out, t.quads, (t.h.neg >> kHoodSelf) & 1u, fpos, [&](int a, int n) {
           int j, slot;
           face_cell_sparse(t.x, t.y, t.z, a, n, j, slot);
           const int64_t row = halo.rows[j];                 // there: the cell is COMPLETE, so its lowest voxel is VALID
           return (row >= 0 ? vertex_of(row, slot) : first) - first;
         });
}

__global__ void __launch_bounds__(kThreads) sparse_mesh_emit_kernel(Bricks k, const float* __restrict__ D,
                                                                    const float* __restrict__ w, float min_weight,
                                                                    BlockScan vs, BlockScan fs,
                                                                    const uint64_t* __restrict__ active, MeshOut out) {
  __shared__ Halo halo;
  __shared__ int word_vertices[kBrickWords], word_quads[kBrickWords];
  const int64_t b = (int64_t)blockIdx.x;
  if (b >= k.B) return;                                   // uniform: the whole workgroup
  const int v = owner(k.brick_start, k.V, b);
  stage_halo(k, D, w, min_weight, v, b, halo);
  const int wave = (int)threadIdx.x / D3F_WAVE;
  Slot t[kSlotsPerThread];
  int v_before[kSlotsPerThread], q_before[kSlotsPerThread];
#pragma unroll
  for (int half = 0; half < kSlotsPerThread; ++half) {
    t[half] = look(halo, half * kThreads + (int)threadIdx.x);
    v_before[half] = rank_in_wave(t[half].edges != 0, word_vertices, half * kWaves + wave);
    q_before[half] = rank_in_wave(t[half].quads, word_quads, half * kWaves + wave);
  }
  __syncthreads();
  const int64_t group = b / kScanThreads;
  const int64_t row_vertex = vs.group_offset[group] + vs.block_offset[b];
  const int64_t row_face = fs.group_offset[group] + fs.block_offset[b];
  int64_t bs = k.brick_start[v];
  if (bs < 0 || bs > b) bs = b;                            // a prefix that does not fit the rows
  const int64_t first = vs.group_offset[bs / kScanThreads] + vs.block_offset[bs];
  int bits = 0;
#pragma unroll
  for (int half = 0; half < kSlotsPerThread; ++half) {
    if (!t[half].edges && !t[half].quads) continue;
    const int word = half * kWaves + wave;
    const int64_t pos = row_vertex + v_before[half] + words_below(word_vertices, word);
    const int64_t fpos = row_face + 2 * (q_before[half] + words_below(word_quads, word));
    bits |= emit_slot(k, halo, v, b, t[half], pos, fpos, first, out, [&](int64_t row, int slot) {
      return vertex_position(vs.block_offset, vs.group_offset, active, row, slot);
    });
  }
  if (bits) atomicOr(out.status, bits);
}

int run_count(const Bricks& k, const float* D, const float* w, float min_weight, int64_t* vertex_start,
              int64_t* face_start, const MeshWs& x, hipStream_t stream) {
  sparse_mesh_count_kernel<<<(unsigned)k.B, kThreads, 0, stream>>>(k, D, w, min_weight, x.vertices.block_count,
                                                                  x.faces.block_count, x.active);
  D3F_LAUNCH_CHECK();
  int rc = run_block_scan(x.vertices, k.B, vertex_start + k.V, stream);
  if (rc != D3F_OK) return rc;
  rc = run_block_scan(x.faces, k.B, face_start + k.V, stream);
  if (rc != D3F_OK) return rc;
  sparse_mesh_start_kernel<<<d3f::cdiv(k.V, kThreads), kThreads, 0, stream>>>(k.brick_start, k.V, k.B, x.vertices,
                                                                              x.faces, vertex_start, face_start);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

bool tables_ok(const float* D, const float* w, const int64_t* lattice_start, const int64_t* brick_start,
               const int32_t* brick_index, const int32_t* brick_coord, const int32_t* dims,
               const int64_t* vertex_start, const int64_t* face_start) {
  return D && w && lattice_start && brick_start && brick_index && brick_coord && dims && vertex_start && face_start;
}

}  // namespace

extern "C" {

size_t d3f_tsdf_sparse_mesh_ws_bytes(int64_t bricks) {
  if (bricks < 0) return 0;
  return MeshWs(nullptr, bricks, kBrickWords).bytes + 256;
}

int d3f_tsdf_sparse_mesh_count(const float* D, const float* w, const int64_t* lattice_start,
                               const int64_t* brick_start, const int32_t* brick_index, const int32_t* brick_coord,
                               const int32_t* dims, int V, int64_t lattice_bricks, int64_t bricks, float min_weight,
                               int64_t* vertex_start, int64_t* face_start, void* ws, size_t ws_bytes, void* stream) {
  if (!pool_ok(V, lattice_bricks, bricks) || bricks == 0 ||
      !tables_ok(D, w, lattice_start, brick_start, brick_index, brick_coord, dims, vertex_start, face_start) || !ws)
    return D3F_EINVAL;
  const MeshWs x(ws, bricks, kBrickWords);
  if (ws_bytes < x.bytes) return D3F_EWORKSPACE;
  const Bricks k = {lattice_start, brick_start, brick_index, brick_coord, nullptr, dims, nullptr, V, lattice_bricks,
                    bricks};
  return run_count(k, D, w, min_weight, vertex_start, face_start, x, (hipStream_t)stream);
}

int d3f_tsdf_sparse_mesh(const float* D, const float* w, const int64_t* lattice_start, const int64_t* brick_start,
                         const int32_t* brick_index, const int32_t* brick_coord, const float* origin,
                         const int32_t* dims, const float* voxel, int V, int64_t lattice_bricks, int64_t bricks,
                         float min_weight, int counted, int64_t vertex_capacity, int64_t face_capacity, float* vertices,
                         float* normals, int32_t* faces, int64_t* vertex_start, int64_t* face_start, int32_t* status,
                         void* ws, size_t ws_bytes, void* stream) {
  const MeshOut out = {vertices, normals, faces, vertex_start, face_start, status, vertex_capacity, face_capacity};
  if (!pool_ok(V, lattice_bricks, bricks) || bricks == 0 ||
      !tables_ok(D, w, lattice_start, brick_start, brick_index, brick_coord, dims, vertex_start, face_start) ||
      !mesh_out_ok(origin, voxel, out) || !ws)
    return D3F_EINVAL;
  const MeshWs x(ws, bricks, kBrickWords);
  if (ws_bytes < x.bytes) return D3F_EWORKSPACE;
  const Bricks k = {lattice_start, brick_start, brick_index, brick_coord, origin, dims, voxel, V, lattice_bricks,
                    bricks};
  if (!counted) {
    const int rc = run_count(k, D, w, min_weight, vertex_start, face_start, x, (hipStream_t)stream);
    if (rc != D3F_OK) return rc;
  }
  sparse_mesh_emit_kernel<<<(unsigned)bricks, kThreads, 0, (hipStream_t)stream>>>(k, D, w, min_weight, x.vertices,
                                                                                  x.faces, x.active, out);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_tsdf_sparse_mesh_host(const float* D, const float* w, const int64_t* lattice_start, const int64_t* brick_start,
                              const int32_t* brick_index, const int32_t* brick_coord, const float* origin,
                              const int32_t* dims, const float* voxel, int V, int64_t lattice_bricks, int64_t bricks,
                              float min_weight, int64_t vertex_capacity, int64_t face_capacity, float* vertices,
                              float* normals, int32_t* faces, int64_t* vertex_start, int64_t* face_start,
                              int32_t* status) {
  const MeshOut out = {vertices, normals, faces, vertex_start, face_start, status, vertex_capacity, face_capacity};
  if (!pool_ok(V, lattice_bricks, bricks) || !lattice_start || !brick_start || !brick_index || !dims || !vertex_start ||
      !face_start || !mesh_out_ok(origin, voxel, out) || (bricks > 0 && (!D || !w || !brick_coord)) ||
      !host_tables_ok(lattice_start, brick_start, dims, V, lattice_bricks, bricks) ||
      !host_coords_ok(lattice_start, brick_start, brick_coord, dims, V))
    return D3F_EINVAL;
  const Bricks k = {lattice_start, brick_start, brick_index, brick_coord, origin, dims, voxel, V, lattice_bricks,
                    bricks};
  // the device's own bookkeeping: a bit per slot and the ACTIVE cells below each row (all of them: one group)
  std::vector<uint64_t> active((size_t)bricks * kBrickWords, 0);
  std::vector<int64_t> block_offset((size_t)bricks, 0), group_offset((size_t)(bricks / kScanThreads + 1), 0);
  std::vector<Halo> halo(1);
  int64_t pos = 0;
  for (int v = 0; v < V; ++v)
    for (int64_t b = brick_start[v]; b < brick_start[v + 1]; ++b) {
      stage_halo_host(k, D, w, min_weight, v, b, halo[0]);
      block_offset[(size_t)b] = pos;
      for (int s = 0; s < kBrickVoxels; ++s)
        if (look(halo[0], s).edges) {
          active[(size_t)b * kBrickWords + (s >> 6)] |= 1ull << (s & 63);
          ++pos;
        }
    }
  const auto vertex_of = [&](int64_t row, int slot) {
    return vertex_position(block_offset.data(), group_offset.data(), active.data(), row, slot);
  };
  int64_t fpos = 0;
  for (int v = 0; v < V; ++v) {
    const int64_t first = brick_start[v] < bricks ? block_offset[(size_t)brick_start[v]] : pos;
    vertex_start[v] = first;
    face_start[v] = fpos;
    for (int64_t b = brick_start[v]; b < brick_start[v + 1]; ++b) {
      stage_halo_host(k, D, w, min_weight, v, b, halo[0]);
      for (int s = 0; s < kBrickVoxels; ++s) {
        const Slot t = look(halo[0], s);
        if (!t.edges && !t.quads) continue;
        *status |= emit_slot(k, halo[0], v, b, t, vertex_of(b, s), fpos, first, out, vertex_of);
        fpos += 2 * popcount3(t.quads);
      }
    }
  }
  vertex_start[V] = pos;
  face_start[V] = fpos;
  return D3F_OK;
}

}  // extern "C"
