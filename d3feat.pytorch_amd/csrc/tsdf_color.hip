// The colour of a TSDF volume at arbitrary points (include/d3feat_hip.h: d3f_tsdf_sample_color,
// d3f_tsdf_sample_color_sparse; the rule is color_at of csrc/tsdf_color.hpp).  It colours what the extract and mesh
// kernels emit -- clouds and mesh vertices, dense or sparse -- without touching those kernels.
//   One thread per point; point i belongs to the volume owner(point_start, V, i), as d3f_tsdf_extract lays the clouds
//   out.  A thread makes the 8 weight loads and the 8 Cc colour loads of its cell together (the sparse form after its 8
//   table lookups) and writes its row of the output once; neighbouring points of an extracted cloud are neighbouring
//   voxels, so the loads of a wave fall into a few rows.  No LDS, no atomics, nothing read back.  A point that no
//   volume owns (i < point_start[0] or i >= point_start[V]) gets NaN.
// The host twins run the same text on the CPU and make no GPU call.
#include "tsdf_batch.hpp"
#include "tsdf_color.hpp"

namespace {

using namespace d3f::tsdf;
namespace rc = d3f::raycast;

struct Points {             // device pointers on the device side, host pointers in the twins
  const float* xyz;             // [N, 3] in the frame of the point's volume
  const int64_t* point_start;   // [V + 1]
  int64_t N;
  float min_weight;
};

// the volume of point i, or -1
__host__ __device__ inline int point_volume(const Points& p, int V, int64_t i) {
  if (i < p.point_start[0] || i >= p.point_start[V]) return -1;
  return owner(p.point_start, V, i);
}

template <int kCc>
__host__ __device__ inline void sample_point(const Volumes& b, const Points& p, const float* w, const float* Cv,
                                             int64_t i, float* out) {
  float c[kCc];
  rc::color_none<kCc>(c);
  const int vol = point_volume(p, b.V, i);
  if (vol >= 0) {
    const int64_t start = b.vol_start[vol], count = b.vol_start[vol + 1] - start;
    if (start >= 0 && count >= 0 && start + count <= b.total) {
      const rc::Lattice L = {nullptr,           w + start,         count,
                             b.origin[3 * vol], b.origin[3 * vol + 1], b.origin[3 * vol + 2],
                             b.voxel[vol],      b.dims[3 * vol],   b.dims[3 * vol + 1],
                             b.dims[3 * vol + 2]};
      rc::color_at<kCc>(L, Cv + start * kCc, p.xyz + 3 * i, p.min_weight, c);
    }
  }
#pragma unroll
  for (int ch = 0; ch < kCc; ++ch) out[i * kCc + ch] = c[ch];
}

template <int kCc>
__host__ __device__ inline void sample_point_sparse(const Bricks& k, const Points& p, const float* w, const float* Cp,
                                                    int64_t i, float* out) {
  float c[kCc];
  rc::color_none<kCc>(c);
  const int vol = point_volume(p, k.V, i);
  if (vol >= 0) {
    const int64_t first = k.lattice_start[vol], end = k.lattice_start[vol + 1];
    const bool fits = first >= 0 && end >= first && end <= k.L;       // else no entry of the table is read
    rc::SparseLattice L;
    L.D = nullptr;
    L.w = w;
    L.index = k.brick_index + (fits ? first : 0);
    L.cells = fits ? end - first : 0;
    L.row0 = k.brick_start[vol];
    L.rows = k.B;
    L.ox = k.origin[3 * vol];
    L.oy = k.origin[3 * vol + 1];
    L.oz = k.origin[3 * vol + 2];
    L.voxel = k.voxel[vol];
    L.nx = k.dims[3 * vol];
    L.ny = k.dims[3 * vol + 1];
    L.nz = k.dims[3 * vol + 2];
    L.nbx = brick_count(L.nx);
    L.nby = brick_count(L.ny);
    L.skip = false;
    rc::color_at<kCc>(L, Cp, p.xyz + 3 * i, p.min_weight, c);
  }
#pragma unroll
  for (int ch = 0; ch < kCc; ++ch) out[i * kCc + ch] = c[ch];
}

template <int kCc>
__global__ void __launch_bounds__(kThreads) sample_color_kernel(Volumes b, Points p, const float* __restrict__ w,
                                                                const float* __restrict__ Cv,
                                                                float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < p.N) sample_point<kCc>(b, p, w, Cv, i, out);
}

template <int kCc>
__global__ void __launch_bounds__(kThreads) sample_color_sparse_kernel(Bricks k, Points p,
                                                                       const float* __restrict__ w,
                                                                       const float* __restrict__ Cp,
                                                                       float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < p.N) sample_point_sparse<kCc>(k, p, w, Cp, i, out);
}

bool points_ok(int channels, const float* points, const int64_t* point_start, int64_t N, const float* out) {
  return (channels == 1 || channels == 3) && N >= 0 && point_start && (N == 0 || (points && out)) &&
         voxel_blocks(N) <= 0x7fffffff;
}

bool dense_ok(const float* Cv, const float* w, const int64_t* vol_start, const float* origin, const int32_t* dims,
              const float* voxel, int V, int64_t total) {
  return batch_ok(V, total) && vol_start && origin && dims && voxel && (total == 0 || (Cv && w));
}

bool sparse_ok(const float* Cp, const float* w, const int64_t* lattice_start, const int64_t* brick_start,
               const int32_t* brick_index, const float* origin, const int32_t* dims, const float* voxel, int V,
               int64_t L, int64_t B) {
  return batch_ok(V, L) && L >= V && L <= 0x7fffffff && B >= 0 && B <= L && lattice_start && brick_start &&
         brick_index && origin && dims && voxel && (B == 0 || (Cp && w));
}

// host pointers only: point_start rises within [0, N]
bool host_points_ok(const int64_t* point_start, int V, int64_t N) {
  if (point_start[0] < 0 || point_start[V] > N) return false;
  for (int v = 0; v < V; ++v)
    if (point_start[v + 1] < point_start[v]) return false;
  return true;
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

int d3f_tsdf_sample_color(const float* Cv, const float* w, int channels, const int64_t* vol_start, const float* origin,
                          const int32_t* dims, const float* voxel, int V, int64_t total_voxels, const float* points,
                          const int64_t* point_start, int64_t N, float min_weight, float* out, void* stream) {
  if (!dense_ok(Cv, w, vol_start, origin, dims, voxel, V, total_voxels) ||
      !points_ok(channels, points, point_start, N, out))
    return D3F_EINVAL;
  if (N == 0) return D3F_OK;
  const Volumes b = {vol_start, origin, dims, voxel, V, total_voxels};
  const Points p = {points, point_start, N, min_weight};
  const unsigned blocks = (unsigned)voxel_blocks(N);
  if (channels == 1)
    sample_color_kernel<1><<<blocks, kThreads, 0, (hipStream_t)stream>>>(b, p, w, Cv, out);
  else
    sample_color_kernel<3><<<blocks, kThreads, 0, (hipStream_t)stream>>>(b, p, w, Cv, out);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_tsdf_sample_color_host(const float* Cv, const float* w, int channels, const int64_t* vol_start,
                               const float* origin, const int32_t* dims, const float* voxel, int V,
                               int64_t total_voxels, const float* points, const int64_t* point_start, int64_t N,
                               float min_weight, float* out, void* stream) {
  (void)stream;
  if (!dense_ok(Cv, w, vol_start, origin, dims, voxel, V, total_voxels) ||
      !points_ok(channels, points, point_start, N, out) || !host_layout_ok(vol_start, dims, V, total_voxels) ||
      !host_points_ok(point_start, V, N))
    return D3F_EINVAL;
  const Volumes b = {vol_start, origin, dims, voxel, V, total_voxels};
  const Points p = {points, point_start, N, min_weight};
  for (int64_t i = 0; i < N; ++i) {
    if (channels == 1)
      sample_point<1>(b, p, w, Cv, i, out);
    else
      sample_point<3>(b, p, w, Cv, i, out);
  }
  return D3F_OK;
}

int d3f_tsdf_sample_color_sparse(const float* Cp, const float* w, int channels, const int64_t* lattice_start,
                                 const int64_t* brick_start, const int32_t* brick_index, const float* origin,
                                 const int32_t* dims, const float* voxel, int V, int64_t lattice_bricks,
                                 int64_t bricks, const float* points, const int64_t* point_start, int64_t N,
                                 float min_weight, float* out, void* stream) {
  if (!sparse_ok(Cp, w, lattice_start, brick_start, brick_index, origin, dims, voxel, V, lattice_bricks, bricks) ||
      !points_ok(channels, points, point_start, N, out))
    return D3F_EINVAL;
  if (N == 0) return D3F_OK;
  const Bricks k = {lattice_start, brick_start, brick_index, nullptr, origin, dims, voxel, V, lattice_bricks, bricks};
  const Points p = {points, point_start, N, min_weight};
  const unsigned blocks = (unsigned)voxel_blocks(N);
  if (channels == 1)
    sample_color_sparse_kernel<1><<<blocks, kThreads, 0, (hipStream_t)stream>>>(k, p, w, Cp, out);
  else
    sample_color_sparse_kernel<3><<<blocks, kThreads, 0, (hipStream_t)stream>>>(k, p, w, Cp, out);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_tsdf_sample_color_sparse_host(const float* Cp, const float* w, int channels, const int64_t* lattice_start,
                                      const int64_t* brick_start, const int32_t* brick_index, const float* origin,
                                      const int32_t* dims, const float* voxel, int V, int64_t lattice_bricks,
                                      int64_t bricks, const float* points, const int64_t* point_start, int64_t N,
                                      float min_weight, float* out, void* stream) {
  (void)stream;
  if (!sparse_ok(Cp, w, lattice_start, brick_start, brick_index, origin, dims, voxel, V, lattice_bricks, bricks) ||
      !points_ok(channels, points, point_start, N, out) ||
      !host_tables_ok(lattice_start, brick_start, dims, V, lattice_bricks, bricks) ||
      !host_points_ok(point_start, V, N))
    return D3F_EINVAL;
  const Bricks k = {lattice_start, brick_start, brick_index, nullptr, origin, dims, voxel, V, lattice_bricks, bricks};
  const Points p = {points, point_start, N, min_weight};
  for (int64_t i = 0; i < N; ++i) {
    if (channels == 1)
      sample_point_sparse<1>(k, p, w, Cp, i, out);
    else
      sample_point_sparse<3>(k, p, w, Cp, i, out);
  }
  return D3F_OK;
}

}  // extern "C"
