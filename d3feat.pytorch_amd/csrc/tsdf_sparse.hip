// Sparse TSDF volumes: bricks of 8 x 8 x 8 voxels allocated only where a depth pixel can reach within the truncation
// distance (include/d3feat_hip.h: d3f_tsdf_sparse_mark, _index, _extract; the rule is csrc/tsdf_sparse.hpp).  The
// integration into the allocated bricks, d3f_tsdf_sparse_integrate, is csrc/tsdf_integrate.hip.
//   mark       one workgroup per 1024 pixels of one frame: the frame, its volume, K and C are workgroup-uniform and
//              come through scalar loads; a lane flags the bricks of its pixel's box with plain stores of 1
//              (idempotent: no atomic decides anything; a flag that is already set is not written again).
//   index      the flags are the counts of the two-level scan of tsdf_batch.hpp (groups of 1024 lattice bricks), then
//              one thread per lattice brick writes its rank (or -1), its coordinates at its pool row, and the volume's
//              first row.
//   extract    tsdf.hip's count -> scan -> emit over blocks of 256 pool slots (two per brick); the +1 neighbour across
//              a brick face is found through brick_index.  No atomic decides a position.
// The host twins run the same tsdf_sparse.hpp text on the CPU and make no GPU call.
#include "tsdf_batch.hpp"    // includes tsdf_sparse.hpp

namespace {

using namespace d3f::tsdf;

constexpr int kMarkPixels = 4;            // pixels per thread of the mark kernel

// ------------------------------------------------------------------------------------------------------------ mark
// flags the bricks of pixel (u, v) of frame f in volume v; flags [L]
template <typename DepthT>
__host__ __device__ inline void mark_pixel(const Frames& fr, const Bricks& k, int vol, int f, int u, int v,
                                           int32_t* flags) {
  int lo[3], hi[3];
  const int32_t* n = k.dims + 3 * (size_t)vol;
  const DepthT* image = (const DepthT*)fr.images + (size_t)fr.H * (size_t)fr.W * (size_t)f;
  if (!pixel_bricks(image, fr.W, u, v, fr.K + 4 * (size_t)f, fr.M + 12 * (size_t)f, fr.depth_scale, fr.depth_max,
                    fr.trunc[vol], k.origin + 3 * (size_t)vol, n, k.voxel[vol], lo, hi))
    return;
  const int64_t nbx = brick_count(n[0]), nby = brick_count(n[1]), base = k.lattice_start[vol];
  for (int bz = lo[2]; bz <= hi[2]; ++bz)
    for (int by = lo[1]; by <= hi[1]; ++by)
      for (int bx = lo[0]; bx <= hi[0]; ++bx) {
        const int64_t l = base + ((int64_t)bz * nby + by) * nbx + bx;
        if (l >= 0 && l < k.L && flags[l] == 0) flags[l] = 1;
      }
}

template <typename DepthT>
__global__ void __launch_bounds__(kThreads) sparse_mark_kernel(Frames fr, Bricks k, int32_t* flags) {
  const int f = (int)blockIdx.y;
  if (f < fr.frame_start[0] || f >= fr.frame_start[k.V]) return;      // a frame no volume owns
  const int vol = owner(fr.frame_start, k.V, (int32_t)f);
  const int pixels = fr.H * fr.W;
  for (int j = 0; j < kMarkPixels; ++j) {
    const int p = ((int)blockIdx.x * kMarkPixels + j) * kThreads + (int)threadIdx.x;
    if (p >= pixels) break;
    mark_pixel<DepthT>(fr, k, vol, f, p % fr.W, p / fr.W, flags);
  }
}

// ----------------------------------------------------------------------------------------------------------- index
struct ScanWs : BlockScan {     // one scan over `counts` counts (lattice bricks; blocks of pool slots) in a workspace
  size_t bytes;
  ScanWs(void* ws, int64_t counts) {
    d3f::Carver c(ws);
    carve(c, counts);
    bytes = d3f::align_up(c.off, 256);
  }
};

// (bx, by, bz) of lattice brick `local` of a volume of dims n
__host__ __device__ inline void brick_position(const int32_t* n, int64_t local, int32_t* out) {
  const int64_t nbx = brick_count(n[0]) > 0 ? brick_count(n[0]) : 1;
  const int64_t nby = brick_count(n[1]) > 0 ? brick_count(n[1]) : 1;
  out[0] = (int32_t)(local % nbx);
  out[1] = (int32_t)((local / nbx) % nby);
  out[2] = (int32_t)(local / nbx / nby);
}

__global__ void __launch_bounds__(kThreads) sparse_index_kernel(const int32_t* __restrict__ flags,
                                                                const int64_t* __restrict__ lattice_start,
                                                                const int32_t* __restrict__ dims, int V, int64_t L,
                                                                const int64_t* __restrict__ block_offset,
                                                                const int64_t* __restrict__ group_offset,
                                                                int32_t* __restrict__ brick_index,
                                                                int32_t* __restrict__ brick_coord,
                                                                int64_t* __restrict__ brick_start) {
  const int64_t l = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (l >= L) return;
  const int v = owner(lattice_start, V, l);
  int64_t ls = lattice_start[v];
  if (ls < 0 || ls > l) ls = l;                                        // a prefix that does not start at 0
  const int64_t first = group_offset[ls / kScanThreads] + block_offset[ls];
  if (l == ls) brick_start[v] = first;
  if (flags[l] == 0) {
    brick_index[l] = -1;
    return;
  }
  const int64_t row = group_offset[l / kScanThreads] + block_offset[l];
  brick_index[l] = (int32_t)(row - first);
  if (row >= 0 && row < L) brick_position(dims + 3 * (size_t)v, l - ls, brick_coord + 3 * row);
}

// --------------------------------------------------------------------------------------------------------- extract
constexpr int kBlocksPerBrick = kBrickVoxels / kThreads;

__global__ void __launch_bounds__(kThreads) sparse_count_kernel(Bricks k, const float* __restrict__ D,
                                                                const float* __restrict__ w, float min_weight,
                                                                int32_t* __restrict__ block_count) {
  __shared__ int wave_total[kThreads / D3F_WAVE];
  const int64_t b = (int64_t)blockIdx.x / kBlocksPerBrick;
  const int s = (int)(blockIdx.x % kBlocksPerBrick) * kThreads + (int)threadIdx.x;
  int n = 0;
  if (b < k.B) {
    int i[3];
    int64_t at[3];
    n = popcount3(sparse_crossings(k, D, w, min_weight, owner(k.brick_start, k.V, b), b, s, i, at));
  }
  n = d3f::wave_sum_i(n);
  if (d3f::lane_id() == 0) wave_total[threadIdx.x / D3F_WAVE] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int j = 0; j < kThreads / D3F_WAVE; ++j) t += wave_total[j];
    block_count[blockIdx.x] = t;
  }
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

__global__ void __launch_bounds__(kThreads) sparse_emit_kernel(Bricks k, const float* __restrict__ D,
                                                               const float* __restrict__ w, float min_weight,
                                                               const int64_t* __restrict__ block_offset,
                                                               const int64_t* __restrict__ group_offset,
                                                               int64_t capacity, float* __restrict__ points,
                                                               int32_t* status) {
  __shared__ int wave_total[kThreads / D3F_WAVE];
  const int64_t b = (int64_t)blockIdx.x / kBlocksPerBrick;
  const int s = (int)(blockIdx.x % kBlocksPerBrick) * kThreads + (int)threadIdx.x;
  const bool live = b < k.B;
  int mask = 0, v = 0, i[3] = {0, 0, 0};
  int64_t at[3] = {0, 0, 0};
  if (live) {
    v = owner(k.brick_start, k.V, b);
    mask = sparse_crossings(k, D, w, min_weight, v, b, s, i, at);
  }
  const int lane = d3f::lane_id(), wave = (int)threadIdx.x / D3F_WAVE;
  const unsigned long long below = (1ull << lane) - 1ull;
  int before = 0, total = 0;   // points of the lower lanes of this wave; of the whole wave
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const unsigned long long m = __ballot((mask >> a) & 1);
    before += __popcll(m & below);
    total += __popcll(m);
  }
  if (lane == 0) wave_total[wave] = total;
  __syncthreads();
  for (int j = 0; j < wave; ++j) before += wave_total[j];
  if (!live || mask == 0) return;
  int64_t pos = group_offset[blockIdx.x / kScanThreads] + block_offset[blockIdx.x] + before;
  const float D0 = D[b * kBrickVoxels + s];
  bool overflow = false;
  for (int a = 0; a < 3; ++a) {
    if (!((mask >> a) & 1)) continue;
    if (pos >= 0 && pos < capacity)
      sparse_point(D0, D[at[a]], i, a, k.origin + 3 * (size_t)v, k.voxel[v], points + 3 * pos);
    else
      overflow = true;
    ++pos;
  }
  if (overflow) atomicOr(status, D3F_TSDF_ST_OVERFLOW);
}

// ---------------------------------------------------------------- launches (the argument checks are tsdf_batch.hpp's)
int64_t extract_blocks(int64_t B) { return B * kBlocksPerBrick; }

int run_sparse_count(const Bricks& k, const float* D, const float* w, float min_weight, int64_t* point_start,
                     const ScanWs& x, int64_t blocks, hipStream_t stream) {
  sparse_count_kernel<<<(unsigned)blocks, kThreads, 0, stream>>>(k, D, w, min_weight, x.block_count);
  D3F_LAUNCH_CHECK();
  const int rc = run_block_scan(x, blocks, point_start + k.V, stream);
  if (rc != D3F_OK) return rc;
  sparse_point_start_kernel<<<d3f::cdiv(k.V, kThreads), kThreads, 0, stream>>>(k.brick_start, k.V, blocks,
                                                                               x.block_offset, x.group_offset,
                                                                               point_start);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

template <typename DepthT>
void mark_host(const Frames& fr, const Bricks& k, int32_t* flags) {
  for (int v = 0; v < k.V; ++v) {
    const int f0 = fr.frame_start[v] < 0 ? 0 : fr.frame_start[v];
    const int f1 = fr.frame_start[v + 1] > fr.F ? fr.F : fr.frame_start[v + 1];
    for (int f = f0; f < f1; ++f)
      for (int y = 0; y < fr.H; ++y)
        for (int x = 0; x < fr.W; ++x) mark_pixel<DepthT>(fr, k, v, f, x, y, flags);
  }
}

}  // namespace

extern "C" {

int d3f_tsdf_sparse_mark(const void* depth, int depth_is_f32, int F, int H, int W, const int32_t* frame_start, int V,
                         const float* intrinsics, const float* camera_to_volume, const float* origin,
                         const int32_t* dims, const float* voxel, const float* trunc, const int64_t* lattice_start,
                         int64_t lattice_bricks, float depth_scale, float depth_max, int32_t* flags, void* stream) {
  if (!lattice_ok(V, lattice_bricks) || !origin || !dims || !voxel || !trunc || !lattice_start || !flags ||
      !frames_ok(depth, F, H, W, frame_start, intrinsics, camera_to_volume, depth_scale, depth_max) || F > 65535)
    return D3F_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (d3f::zero_async(flags, (size_t)lattice_bricks * sizeof(int32_t), s) != hipSuccess) return D3F_ELAUNCH;
  if (F == 0) return D3F_OK;
  const Frames fr = {depth, frame_start, intrinsics, camera_to_volume, trunc, F, H, W, depth_scale, depth_max};
  const Bricks k = {lattice_start, nullptr, nullptr, nullptr, origin, dims, voxel, V, lattice_bricks, 0};
  const dim3 grid((unsigned)d3f::cdiv((int64_t)H * W, kThreads * kMarkPixels), (unsigned)F);
  if (depth_is_f32)
    sparse_mark_kernel<float><<<grid, kThreads, 0, s>>>(fr, k, flags);
  else
    sparse_mark_kernel<uint16_t><<<grid, kThreads, 0, s>>>(fr, k, flags);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_tsdf_sparse_mark_host(const void* depth, int depth_is_f32, int F, int H, int W, const int32_t* frame_start,
                              int V, const float* intrinsics, const float* camera_to_volume, const float* origin,
                              const int32_t* dims, const float* voxel, const float* trunc,
                              const int64_t* lattice_start, int64_t lattice_bricks, float depth_scale, float depth_max,
                              int32_t* flags) {
  if (!lattice_ok(V, lattice_bricks) || !origin || !dims || !voxel || !trunc || !lattice_start || !flags ||
      !frames_ok(depth, F, H, W, frame_start, intrinsics, camera_to_volume, depth_scale, depth_max) ||
      !host_lattice_ok(lattice_start, dims, V, lattice_bricks))
    return D3F_EINVAL;
  for (int64_t l = 0; l < lattice_bricks; ++l) flags[l] = 0;
  const Frames fr = {depth, frame_start, intrinsics, camera_to_volume, trunc, F, H, W, depth_scale, depth_max};
  const Bricks k = {lattice_start, nullptr, nullptr, nullptr, origin, dims, voxel, V, lattice_bricks, 0};
  if (depth_is_f32)
    mark_host<float>(fr, k, flags);
  else
    mark_host<uint16_t>(fr, k, flags);
  return D3F_OK;
}

size_t d3f_tsdf_sparse_index_ws_bytes(int64_t lattice_bricks) {
  if (lattice_bricks < 0) return 0;
  return ScanWs(nullptr, lattice_bricks).bytes + 256;
}

int d3f_tsdf_sparse_index(const int32_t* flags, const int64_t* lattice_start, const int32_t* dims, int V,
                          int64_t lattice_bricks, int32_t* brick_index, int32_t* brick_coord, int64_t* brick_start,
                          void* ws, size_t ws_bytes, void* stream) {
  if (!lattice_ok(V, lattice_bricks) || !flags || !lattice_start || !dims || !brick_index || !brick_coord ||
      !brick_start || !ws)
    return D3F_EINVAL;
  ScanWs x(ws, lattice_bricks);
  if (ws_bytes < x.bytes) return D3F_EWORKSPACE;
  x.block_count = const_cast<int32_t*>(flags);            // the flags are the counts of the scan
  hipStream_t s = (hipStream_t)stream;
  const int rc = run_block_scan(x, lattice_bricks, brick_start + V, s);
  if (rc != D3F_OK) return rc;
  sparse_index_kernel<<<(unsigned)voxel_blocks(lattice_bricks), kThreads, 0, s>>>(
      flags, lattice_start, dims, V, lattice_bricks, x.block_offset, x.group_offset, brick_index, brick_coord,
      brick_start);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_tsdf_sparse_index_host(const int32_t* flags, const int64_t* lattice_start, const int32_t* dims, int V,
                               int64_t lattice_bricks, int32_t* brick_index, int32_t* brick_coord,
                               int64_t* brick_start) {
  if (!lattice_ok(V, lattice_bricks) || !flags || !lattice_start || !dims || !brick_index || !brick_coord ||
      !brick_start || !host_lattice_ok(lattice_start, dims, V, lattice_bricks))
    return D3F_EINVAL;
  int64_t row = 0;
  for (int v = 0; v < V; ++v) {
    brick_start[v] = row;
    for (int64_t l = lattice_start[v]; l < lattice_start[v + 1]; ++l) {
      if (flags[l] == 0) {
        brick_index[l] = -1;
        continue;
      }
      brick_index[l] = (int32_t)(row - brick_start[v]);
      brick_position(dims + 3 * (size_t)v, l - lattice_start[v], brick_coord + 3 * row);
      ++row;
    }
  }
  brick_start[V] = row;
  return D3F_OK;
}

size_t d3f_tsdf_sparse_extract_ws_bytes(int64_t bricks) {
  if (bricks < 0) return 0;
  return ScanWs(nullptr, extract_blocks(bricks)).bytes + 256;
}

int d3f_tsdf_sparse_extract_count(const float* D, const float* w, const int64_t* lattice_start,
                                  const int64_t* brick_start, const int32_t* brick_index, const int32_t* brick_coord,
                                  const int32_t* dims, int V, int64_t lattice_bricks, int64_t bricks, float min_weight,
                                  int64_t* point_start, void* ws, size_t ws_bytes, void* stream) {
  const int64_t blocks = extract_blocks(bricks);
  if (!pool_ok(V, lattice_bricks, bricks) || bricks == 0 || blocks > 0x7fffffff || !D || !w || !lattice_start ||
      !brick_start || !brick_index || !brick_coord || !dims || !point_start || !ws)
    return D3F_EINVAL;
  const ScanWs x(ws, blocks);
  if (ws_bytes < x.bytes) return D3F_EWORKSPACE;
  const Bricks k = {lattice_start, brick_start, brick_index, brick_coord, nullptr, dims, nullptr, V, lattice_bricks,
                    bricks};
  return run_sparse_count(k, D, w, min_weight, point_start, x, blocks, (hipStream_t)stream);
}

int d3f_tsdf_sparse_extract(const float* D, const float* w, const int64_t* lattice_start, const int64_t* brick_start,
                            const int32_t* brick_index, const int32_t* brick_coord, const float* origin,
                            const int32_t* dims, const float* voxel, int V, int64_t lattice_bricks, int64_t bricks,
                            float min_weight, int counted, int64_t capacity, float* points, int64_t* point_start,
                            int32_t* status, void* ws, size_t ws_bytes, void* stream) {
  const int64_t blocks = extract_blocks(bricks);
  if (!pool_ok(V, lattice_bricks, bricks) || bricks == 0 || blocks > 0x7fffffff || !D || !w || !lattice_start ||
      !brick_start || !brick_index || !brick_coord || !origin || !dims || !voxel || !point_start || !status || !ws ||
      capacity < 0 || (capacity > 0 && !points))
    return D3F_EINVAL;
  const ScanWs x(ws, blocks);
  if (ws_bytes < x.bytes) return D3F_EWORKSPACE;
  const Bricks k = {lattice_start, brick_start, brick_index, brick_coord, origin, dims, voxel, V, lattice_bricks,
                    bricks};
  if (!counted) {
    const int rc = run_sparse_count(k, D, w, min_weight, point_start, x, blocks, (hipStream_t)stream);
    if (rc != D3F_OK) return rc;
  }
  sparse_emit_kernel<<<(unsigned)blocks, kThreads, 0, (hipStream_t)stream>>>(
      k, D, w, min_weight, x.block_offset, x.group_offset, capacity, points, status);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_tsdf_sparse_extract_host(const float* D, const float* w, const int64_t* lattice_start,
                                 const int64_t* brick_start, const int32_t* brick_index, const int32_t* brick_coord,
                                 const float* origin, const int32_t* dims, const float* voxel, int V,
                                 int64_t lattice_bricks, int64_t bricks, float min_weight, int64_t capacity,
                                 float* points, int64_t* point_start, int32_t* status) {
  if (!pool_ok(V, lattice_bricks, bricks) || !lattice_start || !brick_start || !brick_index || !origin || !dims ||
      !voxel || !point_start || !status || capacity < 0 || (capacity > 0 && !points) ||
      (bricks > 0 && (!D || !w || !brick_coord)) ||
      !host_tables_ok(lattice_start, brick_start, dims, V, lattice_bricks, bricks) ||
      !host_coords_ok(lattice_start, brick_start, brick_coord, dims, V))
    return D3F_EINVAL;
  const Bricks k = {lattice_start, brick_start, brick_index, brick_coord, origin, dims, voxel, V, lattice_bricks,
                    bricks};
  int64_t pos = 0;
  for (int v = 0; v < V; ++v) {
    point_start[v] = pos;
    for (int64_t b = brick_start[v]; b < brick_start[v + 1]; ++b)
      for (int s = 0; s < kBrickVoxels; ++s) {
        int i[3];
        int64_t at[3];
        const int mask = sparse_crossings(k, D, w, min_weight, v, b, s, i, at);
        for (int a = 0; a < 3; ++a) {
          if (!((mask >> a) & 1)) continue;
          if (pos < capacity)
            sparse_point(D[b * kBrickVoxels + s], D[at[a]], i, a, origin + 3 * (size_t)v, voxel[v], points + 3 * pos);
          else
            *status |= D3F_TSDF_ST_OVERFLOW;
          ++pos;
        }
      }
  }
  point_start[V] = pos;
  return D3F_OK;
}

}  // extern "C"
