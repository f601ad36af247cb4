// TSDF integration: depth frames, and colour frames beside them, fused into a batch of dense volumes or into the
// allocated bricks of sparse ones, from zero or continuing from what is stored (include/d3feat_hip.h: the four
// d3f_tsdf[_sparse]_integrate[_host], colour by `channels`, continuing by `into`; the rule is integrate_voxel<kCc> of
// csrc/tsdf.hpp, the colour csrc/tsdf_color.hpp, the bricks csrc/tsdf_sparse.hpp).
//   One thread owns a cell of D / w / the colour array for ALL frames of its volume: the model is read never (kInto:
//   once, the cell's stored values, from which the running mean continues) and written once with coalesced stores, no
//   atomics, deterministic by construction.  The volume is uniform over the workgroup, so its frame range, the frame
//   loop, trunc, the frame matrices and the intrinsics live in scalar registers and come through scalar loads; the
//   depth images are gathered (neighbouring ix project to neighbouring pixels), and with colour the 2 x 2 pixels
//   around the projection.  A volume that owns no frame in a kInto call is left alone.
//   integrate_kernel<Model, DepthT, kInto, kCc> is the one kernel.  Model is Volumes or Bricks, and what depends on it
//   is overloaded on it below, as make_sampler is for the readers (tsdf_raycast.hip):
//     dense   grid (blocks of the largest volume, V): the volume is blockIdx.y, one voxel per thread, lanes along ix.
//     sparse  grid (B): one workgroup per allocated brick, whose volume owner() finds; lanes along ix (a wave is one z
//             plane of the brick), each thread owns slots t and t + 256.  A slot beyond dims is not in the lattice: it
//             holds 0, and kInto leaves it as it is.
// The host twins run the same text on the CPU, cell after cell, and make no GPU call.
#include "tsdf_batch.hpp"   // Volumes, Frames, locate(), volume_cells() / cell_first() of the twins, the argument checks
#include "tsdf_color.hpp"   // includes tsdf_sparse.hpp (Bricks, slot_voxel) and the rule of the colour

namespace {

using namespace d3f::tsdf;

// ------------------------------------------------------------------------------------------ what depends on the model
// a cell is an index into D and w (and, times kCc, into the colour array): a global voxel, or a slot of the pool.  It
// is named as first + off: `first` is where the cell's volume (dense) or brick (sparse) begins, which is uniform over
// a workgroup, `off` its place in there
template <typename Model> constexpr int kCellsPerThread = 1;                       // kThreads apart
template <> constexpr int kCellsPerThread<Bricks> = kBrickVoxels / kThreads;

// this workgroup's volume and this thread's first cell; false: there is none
__device__ inline bool thread_cells(const Volumes& b, int& v, int64_t& first, int64_t& off) {
  v = (int)blockIdx.y;
  first = b.vol_start[v];
  off = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  return off < b.vol_start[v + 1] - first && first >= 0 && first + off < b.total;
}
__device__ inline bool thread_cells(const Bricks& k, int& v, int64_t& first, int64_t& off) {
  const int64_t b = (int64_t)blockIdx.x;
  if (b >= k.B) return false;
  v = owner(k.brick_start, k.V, b);
  first = b * kBrickVoxels;
  off = threadIdx.x;
  return true;
}

// the lattice coordinates of cell first + off of volume v; false: the cell is not in the lattice
__host__ __device__ inline bool cell_voxel(const Volumes& b, int v, int64_t, int64_t off, int i[3]) {
  int nx, ny, nz;
  locate(b, v, off, i[0], i[1], i[2], nx, ny, nz);
  return true;
}
__host__ __device__ inline bool cell_voxel(const Bricks& k, int v, int64_t first, int64_t off, int i[3]) {
  return slot_voxel(k.dims + 3 * (size_t)v, k.brick_coord + 3 * (size_t)(first / kBrickVoxels), (int)off, i);
}

// the argument checks, in the three steps of integrate() below.  `largest`: max_volume_voxels of the dense device
// form, which sizes its grid (the dense twin, which ignores its own, passes total_voxels); the bricks of the sparse
inline bool model_ok(const Volumes& b, int64_t largest) {
  return batch_ok(b.V, b.total) && largest >= 0 && largest <= b.total && b.vol_start && b.origin && b.dims && b.voxel;
}
inline bool model_ok(const Bricks& k, int64_t) {
  return batch_ok(k.V, k.B) && k.B <= 0x7fffffff && k.origin && k.dims && k.voxel && k.brick_start;
}
inline int64_t cell_count(const Volumes& b) { return b.total; }
inline int64_t cell_count(const Bricks& k) { return k.B; }

// kHost: the tables are host memory and are read; the device forms never dereference one on the host
template <bool kHost>
bool layout_ok(const Volumes& b, int64_t largest) {
  if (kHost) return host_layout_ok(b.vol_start, b.dims, b.V, b.total);
  return voxel_blocks(largest) <= 0x7fffffff;
}
template <bool kHost>
bool layout_ok(const Bricks& k, int64_t) {
  if (!k.brick_coord) return false;
  if (!kHost) return true;
  if (k.brick_start[0] != 0 || k.brick_start[k.V] != k.B) return false;
  for (int v = 0; v < k.V; ++v)
    if (k.brick_start[v + 1] < k.brick_start[v]) return false;
  return true;
}

inline dim3 launch_grid(const Volumes& b, int64_t largest) {
  return dim3((unsigned)voxel_blocks(largest), (unsigned)b.V);
}
inline dim3 launch_grid(const Bricks& k, int64_t) { return dim3((unsigned)k.B); }

// ------------------------------------------------------------------------------------------------------- one cell
// kInto: the cell's stored (D, w, c) come first and the frames continue from them (the entries' into != 0); without
// it they start from zero.  kCc > 0: colours [F, H, W, kCc] are fused into the cell's row of C_out (tsdf_color.hpp)
template <typename DepthT, bool kInto, int kCc, typename Model>
__host__ __device__ inline void fuse_cell(const Model& m, const Frames& fr, int v, int64_t first, int64_t off,
                                          const float* colours, float* D_out, float* w_out, float* C_out) {
  const int64_t at = first + off;
  float D = 0.0f, w = 0.0f, c[kCc > 0 ? kCc : 1];
#pragma unroll
  for (int ch = 0; ch < kCc; ++ch) c[ch] = 0.0f;
  if (kInto) {
    D = D_out[at];
    w = w_out[at];
#pragma unroll
    for (int ch = 0; ch < kCc; ++ch) c[ch] = C_out[at * kCc + ch];
  }
  int i[3];
  if (cell_voxel(m, v, first, off, i)) {
    int f0 = fr.frame_start[v], f1 = fr.frame_start[v + 1];
    if (f0 < 0) f0 = 0;
    if (f1 > fr.F) f1 = fr.F;
    const float voxel = m.voxel[v];
    const float x = lattice(m.origin[3 * v], voxel, i[0]), y = lattice(m.origin[3 * v + 1], voxel, i[1]);
    const float z = lattice(m.origin[3 * v + 2], voxel, i[2]);
    integrate_voxel<kCc>(x, y, z, f0, f1, fr.M, fr.K, (const DepthT*)fr.images, colours, fr.H, fr.W, fr.depth_scale,
                         fr.depth_max, fr.trunc[v], D, w, c);
  }
  D_out[at] = D;
  w_out[at] = w;
#pragma unroll
  for (int ch = 0; ch < kCc; ++ch) C_out[at * kCc + ch] = c[ch];   // a wave writes 64 kCc consecutive floats
}

template <typename Model, typename DepthT, bool kInto, int kCc>
__global__ void __launch_bounds__(kThreads) integrate_kernel(Model m, Frames fr, const float* __restrict__ colours,
                                                             float* __restrict__ D_out, float* __restrict__ w_out,
                                                             float* __restrict__ C_out) {
  int v;
  int64_t first, off;
  if (!thread_cells(m, v, first, off)) return;
  if (kInto && fr.frame_start[v + 1] <= fr.frame_start[v]) return;
#pragma unroll
  for (int j = 0; j < kCellsPerThread<Model>; ++j)
    fuse_cell<DepthT, kInto, kCc>(m, fr, v, first, off + j * kThreads, colours, D_out, w_out, C_out);
}

// ------------------------------------------------------------------- the launch (device) or the loop (host twin)
template <bool kHost, typename DepthT, bool kInto, int kCc, typename Model>
void fuse(const Model& m, int64_t largest, const Frames& fr, const float* colours, float* D, float* w, float* C,
          hipStream_t stream) {
  if constexpr (kHost) {
    for (int v = 0; v < m.V; ++v) {
      if (kInto && fr.frame_start[v + 1] <= fr.frame_start[v]) continue;   // a volume without a frame keeps its values
      int64_t begin, end;
      volume_cells(m, v, begin, end);
      for (int64_t at = begin; at < end; ++at) {
        const int64_t first = cell_first(m, v, at);
        fuse_cell<DepthT, kInto, kCc>(m, fr, v, first, at - first, colours, D, w, C);
      }
    }
  } else {
    integrate_kernel<Model, DepthT, kInto, kCc><<<launch_grid(m, largest), kThreads, 0, stream>>>(m, fr, colours, D, w,
                                                                                                C);
  }
}

template <bool kHost, typename DepthT, bool kInto, typename Model>
void fuse_channels(const Model& m, int64_t largest, const Frames& fr, int channels, const float* colours, float* D,
                   float* w, float* C, hipStream_t stream) {
  if (channels == 1)
    fuse<kHost, DepthT, kInto, 1>(m, largest, fr, colours, D, w, C, stream);
  else if (channels == 3)
    fuse<kHost, DepthT, kInto, 3>(m, largest, fr, colours, D, w, C, stream);
  else
    fuse<kHost, DepthT, kInto, 0>(m, largest, fr, colours, D, w, C, stream);
}

// channels 0: no colour; 1 or 3: colours [F, H, W, channels] and C [cells, channels] are needed
bool colour_ok(int channels, int F, const float* colours, const float* C) {
  if (channels == 0) return true;
  return (channels == 1 || channels == 3) && (F == 0 || colours) && C;
}

template <bool kHost, bool kInto, typename Model>
void fuse_depth(const Model& m, int64_t largest, const Frames& fr, int depth_is_f32, int channels,
                const float* colours, float* D, float* w, float* C, hipStream_t stream) {
  if (depth_is_f32)
    fuse_channels<kHost, float, kInto>(m, largest, fr, channels, colours, D, w, C, stream);
  else
    fuse_channels<kHost, uint16_t, kInto>(m, largest, fr, channels, colours, D, w, C, stream);
}

// every entry point.  channels other than 0, 1 and 3 are rejected before anything else; an empty model is D3F_OK before
// D, w or the colour pointers are looked at; `into` picks kInto, here and nowhere else
template <bool kHost, typename Model>
int integrate(const Model& m, int64_t largest, const Frames& fr, int depth_is_f32, int channels, const float* colours,
              int into, float* D, float* w, float* C, void* stream) {
  if (channels != 0 && channels != 1 && channels != 3) return D3F_EINVAL;
  if (!model_ok(m, largest) || !fr.trunc ||
      !frames_ok(fr.images, fr.F, fr.H, fr.W, fr.frame_start, fr.K, fr.M, fr.depth_scale, fr.depth_max))
    return D3F_EINVAL;
  if (cell_count(m) == 0 || largest == 0) return D3F_OK;
  if (!D || !w || !layout_ok<kHost>(m, largest) || !colour_ok(channels, fr.F, colours, C)) return D3F_EINVAL;
  if (into)
    fuse_depth<kHost, true>(m, largest, fr, depth_is_f32, channels, colours, D, w, C, (hipStream_t)stream);
  else
    fuse_depth<kHost, false>(m, largest, fr, depth_is_f32, channels, colours, D, w, C, (hipStream_t)stream);
  if constexpr (!kHost) D3F_LAUNCH_CHECK();
  return D3F_OK;
}

}  // namespace

// the C ABI: a twin's argument list is its device form's; it ignores stream, the dense one max_volume_voxels too
extern "C" {

int d3f_tsdf_integrate(const void* depth, const float* color, int channels, int depth_is_f32, int F, int H, int W,
                       const int32_t* frame_start, const int64_t* vol_start, int V, int64_t total_voxels,
                       int64_t max_volume_voxels, const float* intrinsics, const float* volume_to_camera,
                       const float* origin, const int32_t* dims, const float* voxel, const float* trunc,
                       float depth_scale, float depth_max, int into, float* D, float* w, float* Cv, void* stream) {
  const Volumes b = {vol_start, origin, dims, voxel, V, total_voxels};
  const Frames fr = {depth, frame_start, intrinsics, volume_to_camera, trunc, F, H, W, depth_scale, depth_max};
  return integrate<false>(b, max_volume_voxels, fr, depth_is_f32, channels, color, into, D, w, Cv, stream);
}

int d3f_tsdf_integrate_host(const void* depth, const float* color, int channels, int depth_is_f32, int F, int H, int W,
                            const int32_t* frame_start, const int64_t* vol_start, int V, int64_t total_voxels, int64_t,
                            const float* intrinsics, const float* volume_to_camera, const float* origin,
                            const int32_t* dims, const float* voxel, const float* trunc, float depth_scale,
                            float depth_max, int into, float* D, float* w, float* Cv, void*) {
  const Volumes b = {vol_start, origin, dims, voxel, V, total_voxels};
  const Frames fr = {depth, frame_start, intrinsics, volume_to_camera, trunc, F, H, W, depth_scale, depth_max};
  return integrate<true>(b, total_voxels, fr, depth_is_f32, channels, color, into, D, w, Cv, nullptr);
}

int d3f_tsdf_sparse_integrate(const void* depth, const float* color, int channels, int depth_is_f32, int F, int H,
                              int W, const int32_t* frame_start, int V, const float* intrinsics,
                              const float* volume_to_camera, const float* origin, const int32_t* dims,
                              const float* voxel, const float* trunc, const int64_t* brick_start,
                              const int32_t* brick_coord, int64_t bricks, float depth_scale, float depth_max,
                              int into, float* D, float* w, float* Cp, void* stream) {
  const Bricks k = {nullptr, brick_start, nullptr, brick_coord, origin, dims, voxel, V, 0, bricks};
  const Frames fr = {depth, frame_start, intrinsics, volume_to_camera, trunc, F, H, W, depth_scale, depth_max};
  return integrate<false>(k, bricks, fr, depth_is_f32, channels, color, into, D, w, Cp, stream);
}

int d3f_tsdf_sparse_integrate_host(const void* depth, const float* color, int channels, int depth_is_f32, int F, int H,
                                   int W, const int32_t* frame_start, int V, const float* intrinsics,
                                   const float* volume_to_camera, const float* origin, const int32_t* dims,
                                   const float* voxel, const float* trunc, const int64_t* brick_start,
                                   const int32_t* brick_coord, int64_t bricks, float depth_scale, float depth_max,
                                   int into, float* D, float* w, float* Cp, void*) {
  const Bricks k = {nullptr, brick_start, nullptr, brick_coord, origin, dims, voxel, V, 0, bricks};
  const Frames fr = {depth, frame_start, intrinsics, volume_to_camera, trunc, F, H, W, depth_scale, depth_max};
  return integrate<true>(k, bricks, fr, depth_is_f32, channels, color, into, D, w, Cp, nullptr);
}

}  // extern "C"
