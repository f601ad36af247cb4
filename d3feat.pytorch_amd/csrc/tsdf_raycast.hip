// Ray-casting a batch of dense TSDF volumes (include/d3feat_hip.h: d3f_tsdf_raycast; the rule is csrc/tsdf_raycast.hpp).
//   One thread per ray, the grid over (blocks of 16 x 16 pixels, views): R views of V volumes run in one launch.  A
//   wave covers an 8 x 8 pixel tile, not 64 pixels of one row, so neighbouring rays fetch neighbouring voxels; the four
//   waves of a block sit 2 x 2.  The view is blockIdx.y, uniform by construction: its volume, intrinsics and matrix
//   come through scalar loads.  A sample makes 16 dependent-address loads (D and w of the 8 corners), issued together
//   before any is used; no LDS, no atomics; the sample loop leaves as soon as the ray has ended, and the box clip of
//   the rule keeps it to the stretch of the ray that crosses the lattice.  Every pixel is written once, by its thread.
// The host twin runs the same tsdf_raycast.hpp text on the CPU and makes no GPU call.
#include "tsdf_batch.hpp"
#include "tsdf_color.hpp"     // includes tsdf_raycast.hpp; the colour behind a hit

namespace {

using namespace d3f::tsdf;
namespace rc = d3f::raycast;

constexpr int kTile = 8;                  // a wave's pixels: kTile x kTile
constexpr int kBlockTiles = 2;            // a block's waves: kBlockTiles x kBlockTiles
constexpr int kBlockEdge = kTile * kBlockTiles;
static_assert(kTile * kTile == D3F_WAVE && kBlockTiles * kBlockTiles * D3F_WAVE == kThreads, "tile layout");

struct Views {              // device pointers on the device side, host pointers in the twin
  const int32_t* view_volume;   // [R]
  const float* K;               // [R, 4]
  const float* C;               // [R, 12] camera -> volume
  const float* step;            // [V]
  int R, H, W;
  float depth_min, depth_max, min_weight;
  int clip;
};

// the lattice of view r's volume; false: the view names no volume of the batch, or one whose voxels are not all in D / w
__host__ __device__ inline bool view_lattice(const Volumes& b, const Views& vw, const float* D, const float* w, int r,
                                             rc::Lattice& L, int& vol) {
  vol = vw.view_volume[r];
  if (vol < 0 || vol >= b.V) return false;
  const int64_t start = b.vol_start[vol], count = b.vol_start[vol + 1] - start;
  if (start < 0 || count < 0 || start + count > b.total) return false;
  L.D = D + start;
  L.w = w + start;
  L.count = count;
  L.ox = b.origin[3 * vol];
  L.oy = b.origin[3 * vol + 1];
  L.oz = b.origin[3 * vol + 2];
  L.voxel = b.voxel[vol];
  L.nx = b.dims[3 * vol];
  L.ny = b.dims[3 * vol + 1];
  L.nz = b.dims[3 * vol + 2];
  return true;
}

__host__ __device__ inline void cast_pixel(const Volumes& b, const Views& vw, const float* D, const float* w, int r,
                                           int u, int v, float* depth, float* normals) {
  const size_t at = ((size_t)r * (size_t)vw.H + (size_t)v) * (size_t)vw.W + (size_t)u;
  float* n = normals ? normals + 3 * at : nullptr;
  rc::Lattice L;
  int vol;
  if (!view_lattice(b, vw, D, w, r, L, vol)) {
    depth[at] = 0.0f;
    if (n) n[0] = n[1] = n[2] = 0.0f;
    return;
  }
  float nrm[3];
  depth[at] = rc::cast_ray(L, vw.K + 4 * (size_t)r, vw.C + 12 * (size_t)r, u, v, vw.step[vol], vw.depth_min,
                           vw.depth_max, vw.min_weight, vw.clip != 0, n != nullptr, nrm);
  if (n) {
    n[0] = nrm[0];
    n[1] = nrm[1];
    n[2] = nrm[2];
  }
}

// grid (blocks of 16 x 16 pixels, R)
__global__ void __launch_bounds__(kThreads) raycast_kernel(Volumes b, Views vw, const float* __restrict__ D,
                                                           const float* __restrict__ w, int blocks_x,
                                                           float* __restrict__ depth, float* __restrict__ normals) {
  const int r = (int)blockIdx.y;
  const int lane = d3f::lane_id(), wave = (int)threadIdx.x / D3F_WAVE;
  const int bx = (int)blockIdx.x % blocks_x, by = (int)blockIdx.x / blocks_x;
  const int u = bx * kBlockEdge + (wave % kBlockTiles) * kTile + (lane % kTile);
  const int v = by * kBlockEdge + (wave / kBlockTiles) * kTile + (lane / kTile);
  if (u >= vw.W || v >= vw.H) return;
  cast_pixel(b, vw, D, w, r, u, v, depth, normals);
}

// cast_pixel, and behind it the colour of the hit (tsdf_color.hpp): Cv [total, kCc] beside D and w, colour [R, H, W, kCc]
template <int kCc>
__host__ __device__ inline void cast_pixel_color(const Volumes& b, const Views& vw, const float* D, const float* w,
                                                 const float* Cv, int r, int u, int v, float* depth, float* normals,
                                                 float* colour) {
  cast_pixel(b, vw, D, w, r, u, v, depth, normals);
  const size_t at = ((size_t)r * (size_t)vw.H + (size_t)v) * (size_t)vw.W + (size_t)u;
  rc::Lattice L;
  int vol;
  float c[kCc];
  if (view_lattice(b, vw, D, w, r, L, vol))
    rc::hit_color<kCc>(L, Cv + b.vol_start[vol] * kCc, vw.K + 4 * (size_t)r, vw.C + 12 * (size_t)r, u, v, depth[at],
                       vw.min_weight, c);
  else
    rc::color_none<kCc>(c);
#pragma unroll
  for (int ch = 0; ch < kCc; ++ch) colour[at * kCc + ch] = c[ch];
}

template <int kCc>
__global__ void __launch_bounds__(kThreads) raycast_color_kernel(Volumes b, Views vw, const float* __restrict__ D,
                                                                 const float* __restrict__ w,
                                                                 const float* __restrict__ Cv, int blocks_x,
                                                                 float* __restrict__ depth,
                                                                 float* __restrict__ normals,
                                                                 float* __restrict__ colour) {
  const int r = (int)blockIdx.y;
  const int lane = d3f::lane_id(), wave = (int)threadIdx.x / D3F_WAVE;
  const int bx = (int)blockIdx.x % blocks_x, by = (int)blockIdx.x / blocks_x;
  const int u = bx * kBlockEdge + (wave % kBlockTiles) * kTile + (lane % kTile);
  const int v = by * kBlockEdge + (wave / kBlockTiles) * kTile + (lane / kTile);
  if (u >= vw.W || v >= vw.H) return;
  cast_pixel_color<kCc>(b, vw, D, w, Cv, r, u, v, depth, normals, colour);
}

bool args_ok(const float* D, const float* w, const int64_t* vol_start, const float* origin, const int32_t* dims,
             const float* voxel, int V, int64_t total_voxels, const int32_t* view_volume, int R, int H, int W,
             const float* intrinsics, const float* camera_to_volume, const float* step, float depth_min,
             float depth_max, float* depth) {
  if (!batch_ok(V, total_voxels) || R < 0 || R > D3F_TSDF_MAX_VOLUMES || H < 1 || W < 1 ||
      (int64_t)H * W > (int64_t)1 << 30 || !vol_start || !origin || !dims || !voxel || !step ||
      !(depth_min >= 0.0f) || !(depth_max >= depth_min) || !(depth_max <= 3.402823466e+38f))
    return false;
  if (R == 0) return true;
  return view_volume && intrinsics && camera_to_volume && depth && (total_voxels == 0 || (D && w));
}

}  // namespace

extern "C" {

int d3f_tsdf_raycast(const float* D, const float* w, const int64_t* vol_start, const float* origin,
                     const int32_t* dims, const float* voxel, int V, int64_t total_voxels, const int32_t* view_volume,
                     int R, int H, int W, const float* intrinsics, const float* camera_to_volume, const float* step,
                     float depth_min, float depth_max, float min_weight, int clip, float* depth, float* normals,
                     void* stream) {
  if (!args_ok(D, w, vol_start, origin, dims, voxel, V, total_voxels, view_volume, R, H, W, intrinsics,
               camera_to_volume, step, depth_min, depth_max, depth))
    return D3F_EINVAL;
  if (R == 0) return D3F_OK;
  const int blocks_x = d3f::cdiv(W, kBlockEdge), blocks_y = d3f::cdiv(H, kBlockEdge);
  if ((int64_t)blocks_x * blocks_y > 0x7fffffff) return D3F_EINVAL;
  const Volumes b = {vol_start, origin, dims, voxel, V, total_voxels};
  const Views vw = {view_volume, intrinsics, camera_to_volume, step, R, H, W, depth_min, depth_max, min_weight, clip};
  const dim3 grid((unsigned)(blocks_x * blocks_y), (unsigned)R);
  raycast_kernel<<<grid, kThreads, 0, (hipStream_t)stream>>>(b, vw, D, w, blocks_x, depth, normals);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_tsdf_raycast_host(const float* D, const float* w, const int64_t* vol_start, const float* origin,
                          const int32_t* dims, const float* voxel, int V, int64_t total_voxels,
                          const int32_t* view_volume, int R, int H, int W, const float* intrinsics,
                          const float* camera_to_volume, const float* step, float depth_min, float depth_max,
                          float min_weight, int clip, float* depth, float* normals, void* stream) {
  (void)stream;
  if (!args_ok(D, w, vol_start, origin, dims, voxel, V, total_voxels, view_volume, R, H, W, intrinsics,
               camera_to_volume, step, depth_min, depth_max, depth) ||
      !host_layout_ok(vol_start, dims, V, total_voxels))
    return D3F_EINVAL;
  const Volumes b = {vol_start, origin, dims, voxel, V, total_voxels};
  const Views vw = {view_volume, intrinsics, camera_to_volume, step, R, H, W, depth_min, depth_max, min_weight, clip};
  for (int r = 0; r < R; ++r)
    for (int v = 0; v < H; ++v)
      for (int u = 0; u < W; ++u) cast_pixel(b, vw, D, w, r, u, v, depth, normals);
  return D3F_OK;
}

int d3f_tsdf_raycast_color(const float* D, const float* w, const float* Cv, int channels, const int64_t* vol_start,
                           const float* origin, const int32_t* dims, const float* voxel, int V, int64_t total_voxels,
                           const int32_t* view_volume, int R, int H, int W, const float* intrinsics,
                           const float* camera_to_volume, const float* step, float depth_min, float depth_max,
                           float min_weight, int clip, float* depth, float* normals, float* color, void* stream) {
  if (!args_ok(D, w, vol_start, origin, dims, voxel, V, total_voxels, view_volume, R, H, W, intrinsics,
               camera_to_volume, step, depth_min, depth_max, depth) ||
      (channels != 1 && channels != 3))
    return D3F_EINVAL;
  if (R == 0) return D3F_OK;
  const int blocks_x = d3f::cdiv(W, kBlockEdge), blocks_y = d3f::cdiv(H, kBlockEdge);
  if ((int64_t)blocks_x * blocks_y > 0x7fffffff || !color || (total_voxels > 0 && !Cv)) return D3F_EINVAL;
  const Volumes b = {vol_start, origin, dims, voxel, V, total_voxels};
  const Views vw = {view_volume, intrinsics, camera_to_volume, step, R, H, W, depth_min, depth_max, min_weight, clip};
  const dim3 grid((unsigned)(blocks_x * blocks_y), (unsigned)R);
  if (channels == 1)
    raycast_color_kernel<1><<<grid, kThreads, 0, (hipStream_t)stream>>>(b, vw, D, w, Cv, blocks_x, depth, normals,
                                                                        color);
  else
    raycast_color_kernel<3><<<grid, kThreads, 0, (hipStream_t)stream>>>(b, vw, D, w, Cv, blocks_x, depth, normals,
                                                                        color);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_tsdf_raycast_color_host(const float* D, const float* w, const float* Cv, int channels,
                                const int64_t* vol_start, const float* origin, const int32_t* dims, const float* voxel,
                                int V, int64_t total_voxels, const int32_t* view_volume, int R, int H, int W,
                                const float* intrinsics, const float* camera_to_volume, const float* step,
                                float depth_min, float depth_max, float min_weight, int clip, float* depth,
                                float* normals, float* color, void* stream) {
  (void)stream;
  if (!args_ok(D, w, vol_start, origin, dims, voxel, V, total_voxels, view_volume, R, H, W, intrinsics,
               camera_to_volume, step, depth_min, depth_max, depth) ||
      (channels != 1 && channels != 3) || !host_layout_ok(vol_start, dims, V, total_voxels))
    return D3F_EINVAL;
  if (R == 0) return D3F_OK;
  if (!color || (total_voxels > 0 && !Cv)) return D3F_EINVAL;
  const Volumes b = {vol_start, origin, dims, voxel, V, total_voxels};
  const Views vw = {view_volume, intrinsics, camera_to_volume, step, R, H, W, depth_min, depth_max, min_weight, clip};
  for (int r = 0; r < R; ++r)
    for (int v = 0; v < H; ++v)
      for (int u = 0; u < W; ++u) {
        if (channels == 1)
          cast_pixel_color<1>(b, vw, D, w, Cv, r, u, v, depth, normals, color);
        else
          cast_pixel_color<3>(b, vw, D, w, Cv, r, u, v, depth, normals, color);
      }
  return D3F_OK;
}

}  // extern "C"
