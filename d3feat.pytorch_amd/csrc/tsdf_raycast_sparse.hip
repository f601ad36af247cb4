// Ray-casting a batch of sparse TSDF volumes (include/d3feat_hip.h: d3f_tsdf_raycast_sparse; the rule is
// csrc/tsdf_raycast_sparse.hpp, the marching loop that of csrc/tsdf_raycast.hpp instantiated for the sparse sampler).
//   Laid out like tsdf_raycast.hip: one thread per ray, the grid over (blocks of 16 x 16 pixels, views), a wave per
//   8 x 8 pixel tile so that neighbouring rays read the same table entries and neighbouring slots of the same rows; the
//   view is blockIdx.y, uniform by construction, so its volume, its part of the tables, intrinsics and matrix come
//   through scalar loads.  A sample reads one entry of brick_index (4 bytes; the table of a fragment is a few hundred
//   KB and stays in the L2) and, when the brick is there, makes the 16 loads of its 8 corners from one pair of 2 KB
//   rows; a cell that straddles bricks looks all of them up first.  An absent brick costs the table read alone, and
//   the samples that stay inside it are skipped.  No LDS, no atomics, nothing read back; every pixel is written once.
// The host twin runs the same text on the CPU and makes no GPU call.
#include "tsdf_batch.hpp"
#include "tsdf_color.hpp"     // includes tsdf_raycast_sparse.hpp; the colour behind a hit

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
  int clip, skip;
};

// the sampler of view r's volume; false: the view names no volume of the batch
__host__ __device__ inline bool view_lattice(const Bricks& k, const Views& vw, const float* D, const float* w, int r,
                                             rc::SparseLattice& L, int& vol) {
  vol = vw.view_volume[r];
  if (vol < 0 || vol >= k.V) return false;
  const int64_t first = k.lattice_start[vol], end = k.lattice_start[vol + 1];
  L.D = D;
  L.w = w;
  L.rows = k.B;
  L.row0 = k.brick_start[vol];
  const bool fits = first >= 0 && end >= first && end <= k.L;       // else no entry of the table is read
  L.index = k.brick_index + (fits ? first : 0);
  L.cells = fits ? end - first : 0;
  L.ox = k.origin[3 * vol];
  L.oy = k.origin[3 * vol + 1];
  L.oz = k.origin[3 * vol + 2];
  L.voxel = k.voxel[vol];
  L.nx = k.dims[3 * vol];
  L.ny = k.dims[3 * vol + 1];
  L.nz = k.dims[3 * vol + 2];
  L.nbx = brick_count(L.nx);
  L.nby = brick_count(L.ny);
  L.skip = vw.skip != 0;
  return true;
}

__host__ __device__ inline void cast_pixel(const Bricks& k, const Views& vw, const float* D, const float* w, int r,
                                           int u, int v, float* depth, float* normals) {
  const size_t at = ((size_t)r * (size_t)vw.H + (size_t)v) * (size_t)vw.W + (size_t)u;
  float* n = normals ? normals + 3 * at : nullptr;
  rc::SparseLattice L;
  int vol;
  if (!view_lattice(k, vw, D, w, r, L, vol)) {
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
__global__ void __launch_bounds__(kThreads) raycast_sparse_kernel(Bricks k, Views vw, const float* __restrict__ D,
                                                                  const float* __restrict__ w, int blocks_x,
                                                                  float* __restrict__ depth,
                                                                  float* __restrict__ normals) {
  const int r = (int)blockIdx.y;
  const int lane = d3f::lane_id(), wave = (int)threadIdx.x / D3F_WAVE;
  const int bx = (int)blockIdx.x % blocks_x, by = (int)blockIdx.x / blocks_x;
  const int u = bx * kBlockEdge + (wave % kBlockTiles) * kTile + (lane % kTile);
  const int v = by * kBlockEdge + (wave / kBlockTiles) * kTile + (lane / kTile);
  if (u >= vw.W || v >= vw.H) return;
  cast_pixel(k, vw, D, w, r, u, v, depth, normals);
}

// cast_pixel, and behind it the colour of the hit (tsdf_color.hpp): Cp [B, 512, kCc] beside the pool, colour
// [R, H, W, kCc]
template <int kCc>
__host__ __device__ inline void cast_pixel_color(const Bricks& k, const Views& vw, const float* D, const float* w,
                                                 const float* Cp, int r, int u, int v, float* depth, float* normals,
                                                 float* colour) {
  cast_pixel(k, vw, D, w, r, u, v, depth, normals);
  const size_t at = ((size_t)r * (size_t)vw.H + (size_t)v) * (size_t)vw.W + (size_t)u;
  rc::SparseLattice L;
  int vol;
  float c[kCc];
  if (view_lattice(k, vw, D, w, r, L, vol))
    rc::hit_color<kCc>(L, Cp, vw.K + 4 * (size_t)r, vw.C + 12 * (size_t)r, u, v, depth[at], vw.min_weight, c);
  else
    rc::color_none<kCc>(c);
#pragma unroll
  for (int ch = 0; ch < kCc; ++ch) colour[at * kCc + ch] = c[ch];
}

template <int kCc>
__global__ void __launch_bounds__(kThreads) raycast_sparse_color_kernel(Bricks k, Views vw,
                                                                        const float* __restrict__ D,
                                                                        const float* __restrict__ w,
                                                                        const float* __restrict__ Cp, int blocks_x,
                                                                        float* __restrict__ depth,
                                                                        float* __restrict__ normals,
                                                                        float* __restrict__ colour) {
  const int r = (int)blockIdx.y;
  const int lane = d3f::lane_id(), wave = (int)threadIdx.x / D3F_WAVE;
  const int bx = (int)blockIdx.x % blocks_x, by = (int)blockIdx.x / blocks_x;
  const int u = bx * kBlockEdge + (wave % kBlockTiles) * kTile + (lane % kTile);
  const int v = by * kBlockEdge + (wave / kBlockTiles) * kTile + (lane / kTile);
  if (u >= vw.W || v >= vw.H) return;
  cast_pixel_color<kCc>(k, vw, D, w, Cp, r, u, v, depth, normals, colour);
}

bool args_ok(const float* D, const float* w, const int64_t* lattice_start, const int64_t* brick_start,
             const int32_t* brick_index, const float* origin, const int32_t* dims, const float* voxel, int V,
             int64_t lattice_bricks, int64_t bricks, const int32_t* view_volume, int R, int H, int W,
             const float* intrinsics, const float* camera_to_volume, const float* step, float depth_min,
             float depth_max, float* depth) {
  if (!batch_ok(V, lattice_bricks) || lattice_bricks < V || lattice_bricks > 0x7fffffff || bricks < 0 ||
      bricks > lattice_bricks || R < 0 || R > D3F_TSDF_MAX_VOLUMES || H < 1 || W < 1 ||
      (int64_t)H * W > (int64_t)1 << 30 || !lattice_start || !brick_start || !brick_index || !origin || !dims ||
      !voxel || !step || !(depth_min >= 0.0f) || !(depth_max >= depth_min) || !(depth_max <= 3.402823466e+38f))
    return false;
  if (R == 0) return true;
  return view_volume && intrinsics && camera_to_volume && depth && (bricks == 0 || (D && w));
}

// host pointers only: lattice_start is the prefix of the brick lattices of dims, brick_start rises from 0 to B
bool host_tables_ok(const int64_t* lattice_start, const int64_t* brick_start, const int32_t* dims, int V, int64_t L,
                    int64_t B) {
  if (lattice_start[0] != 0 || lattice_start[V] != L || brick_start[0] != 0 || brick_start[V] != B) return false;
  for (int v = 0; v < V; ++v) {
    if (dims[3 * v] < 1 || dims[3 * v + 1] < 1 || dims[3 * v + 2] < 1) return false;
    const int64_t n = (int64_t)brick_count(dims[3 * v]) * brick_count(dims[3 * v + 1]) * brick_count(dims[3 * v + 2]);
    if (n != lattice_start[v + 1] - lattice_start[v] || brick_start[v + 1] < brick_start[v]) return false;
  }
  return true;
}

}  // namespace

extern "C" {

int d3f_tsdf_raycast_sparse(const float* D, const float* w, const int64_t* lattice_start, const int64_t* brick_start,
                            const int32_t* brick_index, const float* origin, const int32_t* dims, const float* voxel,
                            int V, int64_t lattice_bricks, int64_t bricks, const int32_t* view_volume, int R, int H,
                            int W, const float* intrinsics, const float* camera_to_volume, const float* step,
                            float depth_min, float depth_max, float min_weight, int clip, int skip, float* depth,
                            float* normals, void* stream) {
  if (!args_ok(D, w, lattice_start, brick_start, brick_index, origin, dims, voxel, V, lattice_bricks, bricks,
               view_volume, R, H, W, intrinsics, camera_to_volume, step, depth_min, depth_max, depth))
    return D3F_EINVAL;
  if (R == 0) return D3F_OK;
  const int blocks_x = d3f::cdiv(W, kBlockEdge), blocks_y = d3f::cdiv(H, kBlockEdge);
  if ((int64_t)blocks_x * blocks_y > 0x7fffffff) return D3F_EINVAL;
  const Bricks k = {lattice_start, brick_start, brick_index, nullptr, origin, dims, voxel, V, lattice_bricks, bricks};
  const Views vw = {view_volume, intrinsics, camera_to_volume, step, R, H, W, depth_min, depth_max, min_weight, clip,
                    skip};
  const dim3 grid((unsigned)(blocks_x * blocks_y), (unsigned)R);
  raycast_sparse_kernel<<<grid, kThreads, 0, (hipStream_t)stream>>>(k, vw, D, w, blocks_x, depth, normals);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_tsdf_raycast_sparse_host(const float* D, const float* w, const int64_t* lattice_start,
                                 const int64_t* brick_start, const int32_t* brick_index, const float* origin,
                                 const int32_t* dims, const float* voxel, int V, int64_t lattice_bricks, int64_t bricks,
                                 const int32_t* view_volume, int R, int H, int W, const float* intrinsics,
                                 const float* camera_to_volume, const float* step, float depth_min, float depth_max,
                                 float min_weight, int clip, int skip, float* depth, float* normals, void* stream) {
  (void)stream;
  if (!args_ok(D, w, lattice_start, brick_start, brick_index, origin, dims, voxel, V, lattice_bricks, bricks,
               view_volume, R, H, W, intrinsics, camera_to_volume, step, depth_min, depth_max, depth) ||
      !host_tables_ok(lattice_start, brick_start, dims, V, lattice_bricks, bricks))
    return D3F_EINVAL;
  const Bricks k = {lattice_start, brick_start, brick_index, nullptr, origin, dims, voxel, V, lattice_bricks, bricks};
  const Views vw = {view_volume, intrinsics, camera_to_volume, step, R, H, W, depth_min, depth_max, min_weight, clip,
                    skip};
  for (int r = 0; r < R; ++r)
    for (int v = 0; v < H; ++v)
      for (int u = 0; u < W; ++u) cast_pixel(k, vw, D, w, r, u, v, depth, normals);
  return D3F_OK;
}

int d3f_tsdf_raycast_sparse_color(const float* D, const float* w, const float* Cp, int channels,
                                  const int64_t* lattice_start, const int64_t* brick_start,
                                  const int32_t* brick_index, const float* origin, const int32_t* dims,
                                  const float* voxel, int V, int64_t lattice_bricks, int64_t bricks,
                                  const int32_t* view_volume, int R, int H, int W, const float* intrinsics,
                                  const float* camera_to_volume, const float* step, float depth_min, float depth_max,
                                  float min_weight, int clip, int skip, float* depth, float* normals, float* color,
                                  void* stream) {
  if (!args_ok(D, w, lattice_start, brick_start, brick_index, origin, dims, voxel, V, lattice_bricks, bricks,
               view_volume, R, H, W, intrinsics, camera_to_volume, step, depth_min, depth_max, depth) ||
      (channels != 1 && channels != 3))
    return D3F_EINVAL;
  if (R == 0) return D3F_OK;
  const int blocks_x = d3f::cdiv(W, kBlockEdge), blocks_y = d3f::cdiv(H, kBlockEdge);
  if ((int64_t)blocks_x * blocks_y > 0x7fffffff || !color || (bricks > 0 && !Cp)) return D3F_EINVAL;
  const Bricks k = {lattice_start, brick_start, brick_index, nullptr, origin, dims, voxel, V, lattice_bricks, bricks};
  const Views vw = {view_volume, intrinsics, camera_to_volume, step, R, H, W, depth_min, depth_max, min_weight, clip,
                    skip};
  const dim3 grid((unsigned)(blocks_x * blocks_y), (unsigned)R);
  if (channels == 1)
    raycast_sparse_color_kernel<1><<<grid, kThreads, 0, (hipStream_t)stream>>>(k, vw, D, w, Cp, blocks_x, depth,
                                                                               normals, color);
  else
    raycast_sparse_color_kernel<3><<<grid, kThreads, 0, (hipStream_t)stream>>>(k, vw, D, w, Cp, blocks_x, depth,
                                                                               normals, color);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_tsdf_raycast_sparse_color_host(const float* D, const float* w, const float* Cp, int channels,
                                       const int64_t* lattice_start, const int64_t* brick_start,
                                       const int32_t* brick_index, const float* origin, const int32_t* dims,
                                       const float* voxel, int V, int64_t lattice_bricks, int64_t bricks,
                                       const int32_t* view_volume, int R, int H, int W, const float* intrinsics,
                                       const float* camera_to_volume, const float* step, float depth_min,
                                       float depth_max, float min_weight, int clip, int skip, float* depth,
                                       float* normals, float* color, void* stream) {
  (void)stream;
  if (!args_ok(D, w, lattice_start, brick_start, brick_index, origin, dims, voxel, V, lattice_bricks, bricks,
               view_volume, R, H, W, intrinsics, camera_to_volume, step, depth_min, depth_max, depth) ||
      (channels != 1 && channels != 3) || !host_tables_ok(lattice_start, brick_start, dims, V, lattice_bricks, bricks))
    return D3F_EINVAL;
  if (R == 0) return D3F_OK;
  if (!color || (bricks > 0 && !Cp)) return D3F_EINVAL;
  const Bricks k = {lattice_start, brick_start, brick_index, nullptr, origin, dims, voxel, V, lattice_bricks, bricks};
  const Views vw = {view_volume, intrinsics, camera_to_volume, step, R, H, W, depth_min, depth_max, min_weight, clip,
                    skip};
  for (int r = 0; r < R; ++r)
    for (int v = 0; v < H; ++v)
      for (int u = 0; u < W; ++u) {
        if (channels == 1)
          cast_pixel_color<1>(k, vw, D, w, Cp, r, u, v, depth, normals, color);
        else
          cast_pixel_color<3>(k, vw, D, w, Cp, r, u, v, depth, normals, color);
      }
  return D3F_OK;
}

}  // extern "C"
