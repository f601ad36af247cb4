// Sparse TSDF volumes: bricks of 8 x 8 x 8 voxels allocated only where a depth pixel can reach within the truncation
// distance (include/d3feat_hip.h: d3f_tsdf_sparse_mark, _index; the rule is csrc/tsdf_sparse.hpp).  The integration
// into the allocated bricks, d3f_tsdf_sparse_integrate, is csrc/tsdf_integrate.hip, the extraction of their zero
// crossings, d3f_tsdf_sparse_extract, csrc/tsdf_extract.hip.
//   mark       one workgroup per 1024 pixels of one frame: the frame, its volume, K and C are workgroup-uniform and
//              come through scalar loads; a lane flags the bricks of its pixel's box with plain stores of 1
//              (idempotent: no atomic decides anything; a flag that is already set is not written again).
//   index      the flags are the counts of the two-level scan of tsdf_batch.hpp (groups of 1024 lattice bricks), then
//              one thread per lattice brick writes its rank (or -1), its coordinates at its pool row, and the volume's
//              first row.
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

}  // extern "C"
