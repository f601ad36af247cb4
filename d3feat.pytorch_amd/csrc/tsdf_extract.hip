// The zero crossings of a fused TSDF model as one stacked cloud, from a batch of dense volumes or from the allocated
// bricks of sparse ones (include/d3feat_hip.h: d3f_tsdf[_sparse]_extract{_ws_bytes, _count, , _host}; the rules are
// crossings() / crossing_point() of csrc/tsdf.hpp and sparse_crossings() / sparse_point() of csrc/tsdf_sparse.hpp).
//   count   per block of 256 cells the points its cells emit (workgroup_sum).
//   scan    the exclusive scan of the block counts in two levels (tsdf_batch.hpp: groups of 1024 counts, coalesced,
//           then the group totals); its grand total is point_start[V].
//   emit    recomputes the crossings and writes at group offset + block offset + in-block rank (ballots + a prefix
//           over the four waves: rank_in_wave, words_below).  No atomic decides a position.
//   extract_count_kernel<Model> and extract_emit_kernel<Model> are the two kernels.  Model is Volumes or Bricks, and what
//   depends on it is overloaded on it below, as in tsdf_integrate.hip:
//     dense   a cell is a global voxel, a block 256 consecutive ones: its volume is found per thread (owner()), and the
//             first voxel of a volume writes point_start[v] in the emit pass.
//     sparse  a cell is a slot of the pool, a block half a brick: the brick and its volume are uniform over the workgroup
//             and computed from blockIdx, so the brick's tables come through scalar loads; the +1 neighbour across a
//             brick face is found through brick_index.  A volume may own no row, so point_start[v] is read from the
//             scan where its rows would begin, by a kernel of its own after the count.
// The host twins run the same text on the CPU, cell after cell in output order, and make no GPU call.
#include <type_traits>

#include "tsdf_batch.hpp"   // Volumes, Bricks, locate(), the argument checks, the two-level scan, the workgroup's rank

namespace {

using namespace d3f::tsdf;

constexpr int kBlocksPerBrick = kBrickVoxels / kThreads;

// ------------------------------------------------------------------------------------------ what depends on the model
// A cell is an index into D and w, named as first + off: `first` is where the cell's volume (dense) or brick (sparse)
// begins, `off` its place in there.  Cell<Model>: the crossings of a cell (mask, bit a: axis a emits), its volume, and
// what the point of an axis needs.
template <typename Model> struct Cell;
template <> struct Cell<Volumes> {
  int mask, v;
  int64_t local;
  int ix, iy, iz, nx, ny;
};
template <> struct Cell<Bricks> {
  int mask, v;
  int64_t here;     // the slot in the pool
  int i[3];         // its voxel
  int64_t at[3];    // the +1 neighbours of the axes of mask
};

// a neighbour beyond the volume's own voxel range (vol_start and dims that disagree) is never read
__host__ __device__ inline Cell<Volumes> look(const Volumes& b, const float* D, const float* w, float min_weight, int v,
                                              int64_t first, int64_t off) {
  Cell<Volumes> c;
  int nz;
  c.v = v;
  c.local = off;
  locate(b, v, off, c.ix, c.iy, c.iz, c.nx, c.ny, nz);
  c.mask = crossings(D + first, w + first, off, b.vol_start[v + 1] - first, c.ix, c.iy, c.iz, c.nx, c.ny, nz, min_weight);
  return c;
}
__host__ __device__ inline Cell<Bricks> look(const Bricks& k, const float* D, const float* w, float min_weight, int v,
                                             int64_t first, int64_t off) {
  Cell<Bricks> c;
  c.v = v;
  c.here = first + off;
  c.mask = sparse_crossings(k, D, w, min_weight, v, first / kBrickVoxels, (int)off, c.i, c.at);
  return c;
}

// this thread's cell; live = false: it has none (and mask = 0)
__device__ inline Cell<Volumes> crossing_at(const Volumes& b, const float* D, const float* w, float min_weight,
                                            bool& live) {
  const int64_t g = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  live = g < b.total;
  if (!live) return Cell<Volumes>{0, 0, 0, 0, 0, 0, 1, 1};
  const int v = owner(b.vol_start, b.V, g);
  const int64_t first = b.vol_start[v];
  return look(b, D, w, min_weight, v, first, g - first);
}
__device__ inline Cell<Bricks> crossing_at(const Bricks& k, const float* D, const float* w, float min_weight,
                                           bool& live) {
  const int64_t b = (int64_t)blockIdx.x / kBlocksPerBrick;          // uniform, and so is the volume
  live = b < k.B;
  if (!live) return Cell<Bricks>{0, 0, 0, {0, 0, 0}, {0, 0, 0}};
  return look(k, D, w, min_weight, owner(k.brick_start, k.V, b), b * kBrickVoxels,
              (int)(blockIdx.x % kBlocksPerBrick) * kThreads + (int)threadIdx.x);
}

// the point of axis a of cell c
__host__ __device__ inline void write_point(const Volumes& b, const float* D, const Cell<Volumes>& c, int a,
                                            float* out) {
  crossing_point(D + b.vol_start[c.v], c.local, c.ix, c.iy, c.iz, c.nx, c.ny, a, b.origin + 3 * c.v, b.voxel[c.v], out);
}
__host__ __device__ inline void write_point(const Bricks& k, const float* D, const Cell<Bricks>& c, int a, float* out) {
  sparse_point(D[c.here], D[c.at[a]], c.i, a, k.origin + 3 * (size_t)c.v, k.voxel[c.v], out);
}

inline int64_t cell_blocks(const Volumes& b) { return voxel_blocks(b.total); }
inline int64_t cell_blocks(const Bricks& k) { return k.B * kBlocksPerBrick; }

// the argument checks.  The device forms want a model that is not empty and never dereference a table on the host;
// `emit`: origin and voxel are needed too (the count forms take neither)
inline bool device_model_ok(const Volumes& b, bool emit) {
  return batch_ok(b.V, b.total) && b.total != 0 && b.vol_start && b.dims && (!emit || (b.origin && b.voxel));
}
inline bool device_model_ok(const Bricks& k, bool emit) {
  return pool_ok(k.V, k.L, k.B) && k.B != 0 && k.lattice_start && k.brick_start && k.brick_index && k.brick_coord &&
         k.dims && (!emit || (k.origin && k.voxel));
}
// the twins read their tables.  An empty pool is legal there, and its pool pointers may then be null
inline bool host_model_ok(const Volumes& b, const float* D, const float* w) {
  return batch_ok(b.V, b.total) && b.total != 0 && D && w && b.vol_start && b.origin && b.dims && b.voxel &&
         host_layout_ok(b.vol_start, b.dims, b.V, b.total);
}
inline bool host_model_ok(const Bricks& k, const float* D, const float* w) {
  return pool_ok(k.V, k.L, k.B) && k.lattice_start && k.brick_start && k.brick_index && k.origin && k.dims && k.voxel &&
         (k.B == 0 || (D && w && k.brick_coord)) &&
         host_tables_ok(k.lattice_start, k.brick_start, k.dims, k.V, k.L, k.B) &&
         host_coords_ok(k.lattice_start, k.brick_start, k.brick_coord, k.dims, k.V);
}

// ---------------------------------------------------------------------------------------------------------- one cell
// the points of cell c into the rows from pos on, which it advances; true: a point lay beyond the capacity
template <typename Model>
__host__ __device__ inline bool write_points(const Model& m, const float* D, const Cell<Model>& c, int64_t& pos,
                                             int64_t capacity, float* points) {
  bool overflow = false;
  for (int a = 0; a < 3; ++a) {
    if (!((c.mask >> a) & 1)) continue;
    if (pos >= 0 && pos < capacity)
      write_point(m, D, c, a, points + 3 * pos);
    else
      overflow = true;
    ++pos;
  }
  return overflow;
}

// ------------------------------------------------------------------------------------------------------- the kernels
template <typename Model>
__global__ void __launch_bounds__(kThreads) extract_count_kernel(Model m, const float* __restrict__ D,
                                                                 const float* __restrict__ w, float min_weight,
                                                                 int32_t* __restrict__ block_count) {
  __shared__ int wave_total[kWaves];
  bool live;
  const int n = workgroup_sum(popcount3(crossing_at(m, D, w, min_weight, live).mask), wave_total);
  if (threadIdx.x == 0) block_count[blockIdx.x] = n;
}

// point_start[v] = the points before the first pool row of volume v (a volume without bricks owns no block: the prefix
// is read where its rows would begin); point_start[V] is the scan's grand total, already written
__global__ void __launch_bounds__(kThreads) sparse_point_start_kernel(const int64_t* __restrict__ brick_start, int V,
                                                                      int64_t blocks,
                                                                      const int64_t* __restrict__ block_offset,
                                                                      const int64_t* __restrict__ group_offset,
                                                                      int64_t* point_start) {
  const int v = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (v >= V) return;
  const int64_t first = brick_start[v] * kBlocksPerBrick;
  point_start[v] = (first >= 0 && first < blocks) ? group_offset[first / kScanThreads] + block_offset[first]
                                                  : point_start[V];
}

template <typename Model>
__global__ void __launch_bounds__(kThreads) extract_emit_kernel(Model m, const float* __restrict__ D,
                                                                const float* __restrict__ w, float min_weight,
                                                                const int64_t* __restrict__ block_offset,
                                                                const int64_t* __restrict__ group_offset,
                                                                int64_t capacity, float* __restrict__ points,
                                                                int64_t* __restrict__ point_start, int32_t* status) {
  __shared__ int wave_total[kWaves];
  bool live;
  const Cell<Model> c = crossing_at(m, D, w, min_weight, live);
  const int wave = (int)threadIdx.x / D3F_WAVE;
  int before = rank_in_wave(c.mask, wave_total, wave);
  __syncthreads();
  before += words_below(wave_total, wave);
  if (!live) return;
  int64_t pos = group_offset[blockIdx.x / kScanThreads] + block_offset[blockIdx.x] + before;
  if constexpr (std::is_same<Model, Volumes>::value)
    if (c.local == 0) point_start[c.v] = pos;     // the first voxel of a volume: where the volume's points begin
  if (c.mask == 0) return;
  if (write_points(m, D, c, pos, capacity, points)) atomicOr(status, D3F_TSDF_ST_OVERFLOW);
}

// ----------------------------------------------------------------------- the launches (device), the loop (host twin)
// the count form (count, no emit), the emit form after it (emit, no count), or both in one call
template <typename Model>
int run_extract(const Model& m, const float* D, const float* w, float min_weight, bool count, bool emit,
                int64_t capacity, float* points, int64_t* point_start, int32_t* status, void* ws, size_t ws_bytes,
                void* stream) {
  if (!device_model_ok(m, emit) || cell_blocks(m) > 0x7fffffff || !D || !w || !point_start || !ws ||
      (emit && (!status || capacity < 0 || (capacity > 0 && !points))))
    return D3F_EINVAL;
  const int64_t blocks = cell_blocks(m);
  const ScanWs x(ws, blocks);
  if (ws_bytes < x.bytes) return D3F_EWORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  if (count) {
    extract_count_kernel<Model><<<(unsigned)blocks, kThreads, 0, s>>>(m, D, w, min_weight, x.block_count);
    D3F_LAUNCH_CHECK();
    const int rc = run_block_scan(x, blocks, point_start + m.V, s);
    if (rc != D3F_OK) return rc;
    if constexpr (std::is_same<Model, Bricks>::value) {
      sparse_point_start_kernel<<<d3f::cdiv(m.V, kThreads), kThreads, 0, s>>>(m.brick_start, m.V, blocks,
                                                                              x.block_offset, x.group_offset,
                                                                              point_start);
      D3F_LAUNCH_CHECK();
    }
  }
  if (emit) {
    extract_emit_kernel<Model><<<(unsigned)blocks, kThreads, 0, s>>>(m, D, w, min_weight, x.block_offset,
                                                                    x.group_offset, capacity, points, point_start,
                                                                    status);
    D3F_LAUNCH_CHECK();
  }
  return D3F_OK;
}

template <typename Model>
int extract_host(const Model& m, const float* D, const float* w, float min_weight, int64_t capacity, float* points,
                 int64_t* point_start, int32_t* status) {
  if (!point_start || !status || capacity < 0 || (capacity > 0 && !points) || !host_model_ok(m, D, w))
    return D3F_EINVAL;
  int64_t pos = 0;
  for (int v = 0; v < m.V; ++v) {
    point_start[v] = pos;
    int64_t begin, end;
    volume_cells(m, v, begin, end);
    for (int64_t at = begin; at < end; ++at) {
      const int64_t first = cell_first(m, v, at);
      if (write_points(m, D, look(m, D, w, min_weight, v, first, at - first), pos, capacity, points))
        *status |= D3F_TSDF_ST_OVERFLOW;
    }
  }
  point_start[m.V] = pos;
  return D3F_OK;
}

}  // namespace

extern "C" {

size_t d3f_tsdf_extract_ws_bytes(int64_t total_voxels) {
  if (total_voxels < 0) return 0;
  return ScanWs(nullptr, voxel_blocks(total_voxels)).bytes + 256;
}

int d3f_tsdf_extract_count(const float* D, const float* w, const int64_t* vol_start, const int32_t* dims, int V,
                           int64_t total_voxels, float min_weight, int64_t* point_start, void* ws, size_t ws_bytes,
                           void* stream) {
  const Volumes b = {vol_start, nullptr, dims, nullptr, V, total_voxels};
  return run_extract(b, D, w, min_weight, true, false, 0, nullptr, point_start, nullptr, ws, ws_bytes, stream);
}

int d3f_tsdf_extract(const float* D, const float* w, const int64_t* vol_start, const float* origin,
                     const int32_t* dims, const float* voxel, int V, int64_t total_voxels, float min_weight,
                     int counted, int64_t capacity, float* points, int64_t* point_start, int32_t* status, void* ws,
                     size_t ws_bytes, void* stream) {
  const Volumes b = {vol_start, origin, dims, voxel, V, total_voxels};
  return run_extract(b, D, w, min_weight, !counted, true, capacity, points, point_start, status, ws, ws_bytes, stream);
}

int d3f_tsdf_extract_host(const float* D, const float* w, const int64_t* vol_start, const float* origin,
                          const int32_t* dims, const float* voxel, int V, int64_t total_voxels, float min_weight,
                          int64_t capacity, float* points, int64_t* point_start, int32_t* status) {
  const Volumes b = {vol_start, origin, dims, voxel, V, total_voxels};
  return extract_host(b, D, w, min_weight, capacity, points, point_start, status);
}

size_t d3f_tsdf_sparse_extract_ws_bytes(int64_t bricks) {
  if (bricks < 0) return 0;
  return ScanWs(nullptr, bricks * kBlocksPerBrick).bytes + 256;
}

int d3f_tsdf_sparse_extract_count(const float* D, const float* w, const int64_t* lattice_start,
                                  const int64_t* brick_start, const int32_t* brick_index, const int32_t* brick_coord,
                                  const int32_t* dims, int V, int64_t lattice_bricks, int64_t bricks, float min_weight,
                                  int64_t* point_start, void* ws, size_t ws_bytes, void* stream) {
  const Bricks k = {lattice_start, brick_start, brick_index, brick_coord, nullptr, dims, nullptr, V, lattice_bricks,
                    bricks};
  return run_extract(k, D, w, min_weight, true, false, 0, nullptr, point_start, nullptr, ws, ws_bytes, stream);
}

int d3f_tsdf_sparse_extract(const float* D, const float* w, const int64_t* lattice_start, const int64_t* brick_start,
                            const int32_t* brick_index, const int32_t* brick_coord, const float* origin,
                            const int32_t* dims, const float* voxel, int V, int64_t lattice_bricks, int64_t bricks,
                            float min_weight, int counted, int64_t capacity, float* points, int64_t* point_start,
                            int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  const Bricks k = {lattice_start, brick_start, brick_index, brick_coord, origin, dims, voxel, V, lattice_bricks,
                    bricks};
  return run_extract(k, D, w, min_weight, !counted, true, capacity, points, point_start, status, ws, ws_bytes, stream);
}

int d3f_tsdf_sparse_extract_host(const float* D, const float* w, const int64_t* lattice_start,
                                 const int64_t* brick_start, const int32_t* brick_index, const int32_t* brick_coord,
                                 const float* origin, const int32_t* dims, const float* voxel, int V,
                                 int64_t lattice_bricks, int64_t bricks, float min_weight, int64_t capacity,
                                 float* points, int64_t* point_start, int32_t* status) {
  const Bricks k = {lattice_start, brick_start, brick_index, brick_coord, origin, dims, voxel, V, lattice_bricks,
                    bricks};
  return extract_host(k, D, w, min_weight, capacity, points, point_start, status);
}

}  // extern "C"
