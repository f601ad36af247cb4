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
//   sparse_mesh_emit_kernel   VGPRs 58, SGPRs 79, no scratch, LDS 5280 bytes, 8 waves per SIMD
#include <vector>

#include "tsdf_batch.hpp"
#include "tsdf_mesh_sparse.hpp"

namespace {

using namespace d3f::tsdf;

constexpr int kWaves = kThreads / D3F_WAVE;
constexpr int kSlotsPerThread = kBrickVoxels / kThreads;

struct SparseMeshWs {
  BlockScan vertices, faces;
  uint64_t* active;        // [B * 8] ballots of the ACTIVE cells
  size_t bytes;
  SparseMeshWs(void* ws, int64_t B) {
    d3f::Carver c(ws);
    vertices.carve(c, B);
    faces.carve(c, B);
    active = c.take<uint64_t>((size_t)B * kBrickWords);
    bytes = d3f::align_up(c.off, 256);
  }
};

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
  nv = d3f::wave_sum_i(nv);
  nf = d3f::wave_sum_i(nf);
  if (d3f::lane_id() == 0) {
    wave_vertices[wave] = nv;
    wave_triangles[wave] = nf;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int sv = 0, sf = 0;
    for (int j = 0; j < kWaves; ++j) {
      sv += wave_vertices[j];
      sf += wave_triangles[j];
    }
    vertex_count[b] = sv;
    face_count[b] = sf;
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

struct MeshOut {
  float* vertices;          // [vertex_capacity, 3]
  float* normals;           // [vertex_capacity, 3]
  int32_t* faces;           // [face_capacity, 3]
  int32_t* status;
  int64_t vertex_capacity, face_capacity;
};

// the vertex of slot t's ACTIVE cell into row pos, the triangles of its edges into the rows from fpos on; returns the
// status bits.  vertex_of(pool row, slot) gives the global row of that cell's vertex; `first` = vertex_start[v].
template <typename VertexOf>
__host__ __device__ inline int emit_slot(const Bricks& k, const Halo& halo, int v, int64_t b, const Slot& t, int64_t pos,
                                         int64_t fpos, int64_t first, const MeshOut& out, VertexOf vertex_of) {
  int bits = 0;
  if (t.edges) {
    if (pos >= 0 && pos < out.vertex_capacity) {
      const int32_t* c = k.brick_coord + 3 * (size_t)b;
      float d[8];
      halo_corners(halo.value, t.x, t.y, t.z, d);
      cell_vertex(d, c[0] * 8 + t.x, c[1] * 8 + t.y, c[2] * 8 + t.z, t.edges, k.origin + 3 * (size_t)v, k.voxel[v],
                  out.vertices + 3 * pos, out.normals + 3 * pos);
    } else {
      bits |= D3F_TSDF_ST_OVERFLOW;
    }
  }
  for (int a = 0; a < 3; ++a) {
    if (!((t.quads >> a) & 1)) continue;
    if (fpos < 0 || fpos >= out.face_capacity) {
      bits |= D3F_TSDF_ST_FACE_OVERFLOW;
      fpos += 2;
      continue;
    }
    int32_t q[4], tri[6];
    bool fits = true;      // false: more than 2^31 - 1 vertices in one volume, and no wrapped index is written
    for (int n = 0; n < 4; ++n) {
      int j, slot;
      face_cell_sparse(t.x, t.y, t.z, a, n, j, slot);
      const int64_t row = halo.rows[j];                      // there: the cell is COMPLETE, so its lowest voxel is VALID
      const int64_t at = (row >= 0 ? vertex_of(row, slot) : first) - first;
      fits = fits && at >= 0 && at <= 0x7fffffff;
      q[n] = (int32_t)at;
    }
    quad_triangles(q, (t.h.neg >> kHoodSelf) & 1u, tri);
    for (int n = 0; n < 2; ++n, ++fpos) {
      if (fpos >= out.face_capacity)
        bits |= D3F_TSDF_ST_FACE_OVERFLOW;
      else if (!fits)
        bits |= D3F_TSDF_ST_OVERFLOW;
      else
        for (int r = 0; r < 3; ++r) out.faces[3 * fpos + r] = tri[3 * n + r];
    }
  }
  return bits;
}

__global__ void __launch_bounds__(kThreads) sparse_mesh_emit_kernel(Bricks k, const float* __restrict__ D,
                                                                    const float* __restrict__ w, float min_weight,
                                                                    BlockScan vs, BlockScan fs,
                                                                    const uint64_t* __restrict__ active, MeshOut out) {
  __shared__ Halo halo;
  __shared__ int word_vertices[kBrickWords], word_triangles[kBrickWords];
  const int64_t b = (int64_t)blockIdx.x;
  if (b >= k.B) return;                                   // uniform: the whole workgroup
  const int v = owner(k.brick_start, k.V, b);
  stage_halo(k, D, w, min_weight, v, b, halo);
  const int lane = d3f::lane_id(), wave = (int)threadIdx.x / D3F_WAVE;
  const unsigned long long below = (1ull << lane) - 1ull;
  Slot t[kSlotsPerThread];
  int v_before[kSlotsPerThread], f_before[kSlotsPerThread];
#pragma unroll
  for (int half = 0; half < kSlotsPerThread; ++half) {
    t[half] = look(halo, half * kThreads + (int)threadIdx.x);
    const unsigned long long mv = __ballot(t[half].edges != 0);
    v_before[half] = __popcll(mv & below);
    f_before[half] = 0;
    int f_total = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const unsigned long long m = __ballot((t[half].quads >> a) & 1);
      f_before[half] += 2 * __popcll(m & below);
      f_total += 2 * __popcll(m);
    }
    if (lane == 0) {
      word_vertices[half * kWaves + wave] = __popcll(mv);
      word_triangles[half * kWaves + wave] = f_total;
    }
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
    int64_t pos = row_vertex + v_before[half], fpos = row_face + f_before[half];
    for (int j = 0; j < half * kWaves + wave; ++j) {
      pos += word_vertices[j];
      fpos += word_triangles[j];
    }
    bits |= emit_slot(k, halo, v, b, t[half], pos, fpos, first, out, [&](int64_t row, int slot) {
      return vertex_position(vs.block_offset, vs.group_offset, active, row, slot);
    });
  }
  if (bits) atomicOr(out.status, bits);
}

int run_count(const Bricks& k, const float* D, const float* w, float min_weight, int64_t* vertex_start,
              int64_t* face_start, const SparseMeshWs& x, hipStream_t stream) {
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

bool out_ok(const float* origin, const float* voxel, const MeshOut& out) {
  return origin && voxel && out.status && out.vertex_capacity >= 0 && out.face_capacity >= 0 &&
         (out.vertex_capacity == 0 || (out.vertices && out.normals)) && (out.face_capacity == 0 || out.faces);
}

}  // namespace

extern "C" {

size_t d3f_tsdf_sparse_mesh_ws_bytes(int64_t bricks) {
  if (bricks < 0) return 0;
  return SparseMeshWs(nullptr, bricks).bytes + 256;
}

int d3f_tsdf_sparse_mesh_count(const float* D, const float* w, const int64_t* lattice_start,
                               const int64_t* brick_start, const int32_t* brick_index, const int32_t* brick_coord,
                               const int32_t* dims, int V, int64_t lattice_bricks, int64_t bricks, float min_weight,
                               int64_t* vertex_start, int64_t* face_start, void* ws, size_t ws_bytes, void* stream) {
  if (!pool_ok(V, lattice_bricks, bricks) || bricks == 0 ||
      !tables_ok(D, w, lattice_start, brick_start, brick_index, brick_coord, dims, vertex_start, face_start) || !ws)
    return D3F_EINVAL;
  const SparseMeshWs x(ws, bricks);
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
  const MeshOut out = {vertices, normals, faces, status, vertex_capacity, face_capacity};
  if (!pool_ok(V, lattice_bricks, bricks) || bricks == 0 ||
      !tables_ok(D, w, lattice_start, brick_start, brick_index, brick_coord, dims, vertex_start, face_start) ||
      !out_ok(origin, voxel, out) || !ws)
    return D3F_EINVAL;
  const SparseMeshWs x(ws, bricks);
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
  const MeshOut out = {vertices, normals, faces, status, vertex_capacity, face_capacity};
  if (!pool_ok(V, lattice_bricks, bricks) || !lattice_start || !brick_start || !brick_index || !dims || !vertex_start ||
      !face_start || !out_ok(origin, voxel, out) || (bricks > 0 && (!D || !w || !brick_coord)) ||
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
