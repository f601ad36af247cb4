// What the tsdf*.hip files share beyond the rules of tsdf.hpp and tsdf_sparse.hpp: the batch of volumes and its
// frames (Volumes, beside Bricks the two models tsdf_integrate.hip, tsdf_extract.hip and tsdf_raycast.hip are templated
// on), the position of a voxel in its lattice, the cells a host twin walks, the argument checks (dense and sparse), the
// two-level exclusive scan of per-block counts with its workspace, and the two things a workgroup does around it in
// tsdf_extract.hip, tsdf_mesh.hip and tsdf_mesh_sparse.hip (count per block of 256 cells -> scan -> emit at group offset
// + block offset + in-block rank): workgroup_sum() and rank_in_wave() / words_below().  Included by .hip files only.
#pragma once
#include "common.hpp"
#include "tsdf.hpp"
#include "tsdf_sparse.hpp"   // Bricks, brick_count

namespace d3f {
namespace tsdf {

constexpr int kThreads = 256;
constexpr int kScanThreads = 1024;       // block counts per group of the two-level scan

struct Volumes {            // the batch: device pointers on the device side, host pointers in the twins
  const int64_t* vol_start;   // [V + 1] voxel prefix
  const float* origin;        // [V, 3]
  const int32_t* dims;        // [V, 3] = nx, ny, nz
  const float* voxel;         // [V]
  int V;
  int64_t total;
};

struct Frames {             // the depth frames of a batch
  const void* images;           // [F, H, W] uint16 or f32
  const int32_t* frame_start;   // [V + 1]
  const float* K;               // [F, 4]
  const float* M;               // [F, 12] volume -> camera (camera -> volume where a kernel back-projects)
  const float* trunc;           // [V]
  int F, H, W;
  float depth_scale, depth_max;
};

// (ix, iy, iz) of local voxel index `local` of volume v
__host__ __device__ inline void locate(const Volumes& b, int v, int64_t local, int& ix, int& iy, int& iz, int& nx,
                                       int& ny, int& nz) {
  nx = b.dims[3 * v] > 0 ? b.dims[3 * v] : 1;
  ny = b.dims[3 * v + 1] > 0 ? b.dims[3 * v + 1] : 1;
  nz = b.dims[3 * v + 2];
  ix = (int)(local % nx);
  const int64_t row = local / nx;
  iy = (int)(row % ny);
  iz = (int)(row / ny);
}

// the cells (voxels; pool slots) that a host twin walks for volume v, [begin, end), and where the volume or the brick
// of cell `at` begins
inline void volume_cells(const Volumes& b, int v, int64_t& begin, int64_t& end) {
  begin = b.vol_start[v];
  end = b.vol_start[v + 1];
}
inline void volume_cells(const Bricks& k, int v, int64_t& begin, int64_t& end) {
  begin = k.brick_start[v] * kBrickVoxels;
  end = k.brick_start[v + 1] * kBrickVoxels;
}
inline int64_t cell_first(const Volumes& b, int v, int64_t) { return b.vol_start[v]; }
inline int64_t cell_first(const Bricks&, int, int64_t at) { return at - at % kBrickVoxels; }

// -------------------------------------------------------------------------------------------------- argument checks
static inline bool batch_ok(int V, int64_t total) { return V >= 1 && V <= D3F_TSDF_MAX_VOLUMES && total >= 0; }

static inline int frames_ok(const void* depth, int F, int H, int W, const int32_t* frame_start, const float* K,
                            const float* X, float depth_scale, float depth_max) {
  if (F < 0 || H < 1 || W < 1 || (int64_t)H * W > (int64_t)1 << 30 || !frame_start || !(depth_scale > 0.0f) ||
      !(depth_max > 0.0f))
    return 0;
  return F == 0 || (depth && K && X);
}

static inline int64_t voxel_blocks(int64_t total) { return (total + kThreads - 1) / kThreads; }

// host pointers only: vol_start is the prefix of dims, from 0 to total
static inline bool host_layout_ok(const int64_t* vol_start, const int32_t* dims, int V, int64_t total) {
  if (vol_start[0] != 0 || vol_start[V] != total) return false;
  for (int v = 0; v < V; ++v)
    if (dims[3 * v] < 1 || dims[3 * v + 1] < 1 || dims[3 * v + 2] < 1 ||
        (int64_t)dims[3 * v] * dims[3 * v + 1] * dims[3 * v + 2] != vol_start[v + 1] - vol_start[v])
      return false;
  return true;
}

// the sparse batch.  The lattice: at least one brick per volume, all of them indexable by int32
static inline bool lattice_ok(int V, int64_t L) { return batch_ok(V, L) && L >= V && L <= 0x7fffffff; }

static inline bool pool_ok(int V, int64_t L, int64_t B) { return lattice_ok(V, L) && B >= 0 && B <= L; }

// host pointers only: lattice_start is the prefix of the brick lattices of dims, from 0 to L
static inline bool host_lattice_ok(const int64_t* lattice_start, const int32_t* dims, int V, int64_t L) {
  if (lattice_start[0] != 0 || lattice_start[V] != L) return false;
  for (int v = 0; v < V; ++v) {
    if (dims[3 * v] < 1 || dims[3 * v + 1] < 1 || dims[3 * v + 2] < 1) return false;
    const int64_t n = (int64_t)brick_count(dims[3 * v]) * brick_count(dims[3 * v + 1]) * brick_count(dims[3 * v + 2]);
    if (n != lattice_start[v + 1] - lattice_start[v]) return false;
  }
  return true;
}

// host pointers only: host_lattice_ok, and brick_start rises from 0 to B (so every row of every volume lies in the pool)
static inline bool host_tables_ok(const int64_t* lattice_start, const int64_t* brick_start, const int32_t* dims, int V,
                                  int64_t L, int64_t B) {
  if (!host_lattice_ok(lattice_start, dims, V, L) || brick_start[0] != 0 || brick_start[V] != B) return false;
  for (int v = 0; v < V; ++v)
    if (brick_start[v + 1] < brick_start[v]) return false;
  return true;
}

// host pointers only, after host_tables_ok: a volume holds no more bricks than its lattice, and every row's
// coordinates lie in its volume's lattice (what the extract and mesh twins ask on top: they read brick_coord)
static inline bool host_coords_ok(const int64_t* lattice_start, const int64_t* brick_start, const int32_t* brick_coord,
                                  const int32_t* dims, int V) {
  for (int v = 0; v < V; ++v) {
    if (brick_start[v + 1] - brick_start[v] > lattice_start[v + 1] - lattice_start[v]) return false;
    for (int64_t b = brick_start[v]; b < brick_start[v + 1]; ++b)
      for (int a = 0; a < 3; ++a)
        if (brick_coord[3 * b + a] < 0 || brick_coord[3 * b + a] >= brick_count(dims[3 * v + a])) return false;
  }
  return true;
}

// ------------------------------------------------------------------------------------------------------------ scan
// one exclusive scan of `blocks` int32 counts: its arrays in a workspace
struct BlockScan {
  int64_t* block_offset;   // [blocks] exclusive prefix of the counts inside the block's group
  int64_t* group_total;    // [groups]
  int64_t* group_offset;   // [groups] exclusive prefix of the group totals
  int32_t* block_count;    // [blocks]
  int64_t groups;
  void carve(d3f::Carver& c, int64_t blocks) {
    groups = (blocks + kScanThreads - 1) / kScanThreads;
    block_offset = c.take<int64_t>((size_t)blocks);
    group_total = c.take<int64_t>((size_t)groups);
    group_offset = c.take<int64_t>((size_t)groups);
    block_count = c.take<int32_t>((size_t)blocks);
  }
};

// exclusive scan of one value per thread over the kScanThreads threads of a workgroup; returns the thread's prefix and
// the sum of all in `total`
__device__ inline int64_t workgroup_exclusive_scan(int64_t value, int64_t* lds, int64_t& total) {
  const int t = (int)threadIdx.x;
  lds[t] = value;
  __syncthreads();
  for (int off = 1; off < kScanThreads; off <<= 1) {
    const int64_t add = t >= off ? lds[t - off] : 0;
    __syncthreads();
    lds[t] += add;
    __syncthreads();
  }
  const int64_t inclusive = lds[t];
  total = lds[kScanThreads - 1];
  __syncthreads();
  return inclusive - value;
}

// level 1: one workgroup per group of 1024 block counts (coalesced): offsets inside the group, and the group's total
__global__ static void __launch_bounds__(kScanThreads) scan_groups_kernel(const int32_t* __restrict__ block_count,
                                                                          int64_t blocks,
                                                                          int64_t* __restrict__ block_offset,
                                                                          int64_t* __restrict__ group_total) {
  __shared__ int64_t lds[kScanThreads];
  const int64_t i = (int64_t)blockIdx.x * kScanThreads + threadIdx.x;
  int64_t total;
  const int64_t prefix = workgroup_exclusive_scan(i < blocks ? (int64_t)block_count[i] : 0, lds, total);
  if (i < blocks) block_offset[i] = prefix;
  if (threadIdx.x == 0) group_total[blockIdx.x] = total;
}

// level 2: ONE workgroup scans the group totals, 1024 at a time with a carry.  *grand_total = the sum of all counts.
__global__ static void __launch_bounds__(kScanThreads) scan_totals_kernel(const int64_t* __restrict__ group_total,
                                                                          int64_t groups,
                                                                          int64_t* __restrict__ group_offset,
                                                                          int64_t* grand_total) {
  __shared__ int64_t lds[kScanThreads];
  int64_t carry = 0;
  for (int64_t base = 0; base < groups; base += kScanThreads) {
    const int64_t i = base + threadIdx.x;
    int64_t total;
    const int64_t prefix = workgroup_exclusive_scan(i < groups ? group_total[i] : 0, lds, total);
    if (i < groups) group_offset[i] = carry + prefix;
    carry += total;
  }
  if (threadIdx.x == 0) *grand_total = carry;
}

// both levels over s.block_count; *grand_total (device) receives the sum
static inline int run_block_scan(const BlockScan& s, int64_t blocks, int64_t* grand_total, hipStream_t stream) {
  scan_groups_kernel<<<(unsigned)s.groups, kScanThreads, 0, stream>>>(s.block_count, blocks, s.block_offset,
                                                                      s.group_total);
  D3F_LAUNCH_CHECK();
  scan_totals_kernel<<<1, kScanThreads, 0, stream>>>(s.group_total, s.groups, s.group_offset, grand_total);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

struct ScanWs : BlockScan {     // one scan over `counts` counts (blocks of cells; lattice bricks) in a workspace
  size_t bytes;
  ScanWs(void* ws, int64_t counts) {
    d3f::Carver c(ws);
    carve(c, counts);
    bytes = d3f::align_up(c.off, 256);
  }
};

// ------------------------------------------------------------------- a workgroup of kThreads: the count and the rank
constexpr int kWaves = kThreads / D3F_WAVE;

// the sum of `n` over the workgroup, in thread 0.  One barrier, before the sum: the other waves are not held until
// thread 0 has added up, so wave_total [kWaves] must not be written again before another barrier
__device__ inline int workgroup_sum(int n, int* wave_total) {
  n = d3f::wave_sum_i(n);
  if (d3f::lane_id() == 0) wave_total[threadIdx.x / D3F_WAVE] = n;
  __syncthreads();
  int s = 0;
  if (threadIdx.x == 0)
    for (int k = 0; k < kWaves; ++k) s += wave_total[k];
  return s;
}

// the rank of a thread's first item among the items of its workgroup, in two steps around ONE barrier of the caller's.
// Before it: the set bits of `mask` (bits 0..2, an item each) in the lower lanes of this wave are returned, and lane 0
// writes those of the whole wave to totals[word].  After it: words_below() adds the words under `word`.  A wave that
// ranks several masks gives each its own word (or its own array), in the order of the output.
__device__ inline int rank_in_wave(int mask, int* totals, int word) {
  const int lane = d3f::lane_id();
  const unsigned long long below = (1ull << lane) - 1ull;
  int before = 0, total = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const unsigned long long m = __ballot((mask >> a) & 1);
    before += __popcll(m & below);
    total += __popcll(m);
  }
  if (lane == 0) totals[word] = total;
  return before;
}
__device__ inline int words_below(const int* totals, int word) {
  int s = 0;
  for (int k = 0; k < word; ++k) s += totals[k];
  return s;
}

}  // namespace tsdf
}  // namespace d3f
