// Reading a fused TSDF model, dense or sparse (include/d3feat_hip.h: d3f_tsdf_raycast, d3f_tsdf_raycast_sparse,
// d3f_tsdf_sample_color, d3f_tsdf_sample_color_sparse, each with its _host twin).  The rules are
// csrc/tsdf_raycast.hpp (the marching loop), csrc/tsdf_raycast_sparse.hpp (the sparse sampler it is instantiated for)
// and csrc/tsdf_color.hpp (the colour at a point and behind a hit); here is what surrounds them, written once for
// both kinds of model: make_sampler builds the Lattice of a volume of `Volumes` or the SparseLattice of one of `Bricks`.
//   Ray-cast.  One thread per ray, the grid over (blocks of 16 x 16 pixels, views): R views of V volumes run in one
//   launch.  A wave covers an 8 x 8 pixel tile, not 64 pixels of one row, so neighbouring rays fetch neighbouring
//   voxels (sparse: the same table entries and neighbouring slots of the same rows); the four waves of a block sit
//   2 x 2.  The view is blockIdx.y, uniform by construction: its volume, its part of the tables, intrinsics and matrix
//   come through scalar loads.  A dense sample makes 16 dependent-address loads (D and w of the 8 corners), issued
//   together before any is used.  A sparse sample reads one entry of brick_index (4 bytes; the table of a fragment is a
//   few hundred KB and stays in the L2) and, when the brick is there, makes the 16 loads of its 8 corners from one pair
//   of 2 KB rows; a cell that straddles bricks looks all of them up first; an absent brick costs the table read alone,
//   and the samples that stay inside it are skipped.  The sample loop leaves as soon as the ray has ended, and the box
//   clip of the rule keeps it to the stretch of the ray that crosses the lattice.  Every pixel is written once, by its
//   thread: depth, normals and, with channels > 0, the colour of the hit.
//   Point sampling colours what the extract and mesh kernels emit -- clouds and mesh vertices -- without touching
//   those kernels.  One thread per point; point i belongs to the volume owner(point_start, V, i), as d3f_tsdf_extract
//   lays the clouds out.  A thread makes the 8 weight loads and the 8 Cc colour loads of its cell together (the sparse
//   form after its 8 table lookups) and writes its row of the output once; neighbouring points of an extracted cloud
//   are neighbouring voxels, so the loads of a wave fall into a few rows.  A point that no volume owns
//   (i < point_start[0] or i >= point_start[V]) gets NaN.
// No LDS, no atomics, nothing read back.  The host twins run the same cast_pixel / sample_point text on the CPU and
// make no GPU call.
#include "tsdf_batch.hpp"
#include "tsdf_color.hpp"     // includes tsdf_raycast.hpp and tsdf_raycast_sparse.hpp

namespace {

using namespace d3f::tsdf;
namespace rc = d3f::raycast;

constexpr int kTile = 8;                  // a wave's pixels: kTile x kTile
constexpr int kBlockTiles = 2;            // a block's waves: kBlockTiles x kBlockTiles
constexpr int kBlockEdge = kTile * kBlockTiles;
static_assert(kTile * kTile == D3F_WAVE && kBlockTiles * kBlockTiles * D3F_WAVE == kThreads, "tile layout");

// ------------------------------------------------------------------------------------------------------ the model
// A model is the `Volumes` of dense D, w [total] or the `Bricks` of a pool D, w [B, 512]; everything below is written
// for either, and make_sampler is the one place that tells them apart.
template <typename Lattice>
struct Sampler {
  Lattice L;
  const float* colour;        // the colours that L's voxel indices address
  bool ok;                    // false: `vol` names no volume of the batch, or (dense) one whose voxels are not all there
};

// the sampler of volume `vol`: its voxels in D and w, its colours in Cv [total, Cc] (Cc = 0: none)
__host__ __device__ inline Sampler<rc::Lattice> make_sampler(const Volumes& b, const float* D, const float* w,
                                                             const float* Cv, int Cc, int vol, bool skip) {
  (void)skip;
  Sampler<rc::Lattice> s;
  s.ok = false;
  if (vol < 0 || vol >= b.V) return s;
  const int64_t start = b.vol_start[vol], count = b.vol_start[vol + 1] - start;
  if (start < 0 || count < 0 || start + count > b.total) return s;
  s.ok = true;
  s.colour = Cv + start * Cc;
  s.L.D = D + start;
  s.L.w = w + start;
  s.L.count = count;
  s.L.ox = b.origin[3 * vol];
  s.L.oy = b.origin[3 * vol + 1];
  s.L.oz = b.origin[3 * vol + 2];
  s.L.voxel = b.voxel[vol];
  s.L.nx = b.dims[3 * vol];
  s.L.ny = b.dims[3 * vol + 1];
  s.L.nz = b.dims[3 * vol + 2];
  return s;
}

// the sampler of sparse volume `vol`: the whole pool D, w, Cp [B, 512, Cc] and the volume's part of the tables
__host__ __device__ inline Sampler<rc::SparseLattice> make_sampler(const Bricks& k, const float* D, const float* w,
                                                                   const float* Cp, int Cc, int vol, bool skip) {
  (void)Cc;
  Sampler<rc::SparseLattice> s;
  s.ok = false;
  if (vol < 0 || vol >= k.V) return s;
  const int64_t first = k.lattice_start[vol], end = k.lattice_start[vol + 1];
  const bool fits = first >= 0 && end >= first && end <= k.L;       // else no entry of the table is read
  s.ok = true;
  s.colour = Cp;
  s.L.D = D;
  s.L.w = w;
  s.L.rows = k.B;
  s.L.row0 = k.brick_start[vol];
  s.L.index = k.brick_index + (fits ? first : 0);
  s.L.cells = fits ? end - first : 0;
  s.L.ox = k.origin[3 * vol];
  s.L.oy = k.origin[3 * vol + 1];
  s.L.oz = k.origin[3 * vol + 2];
  s.L.voxel = k.voxel[vol];
  s.L.nx = k.dims[3 * vol];
  s.L.ny = k.dims[3 * vol + 1];
  s.L.nz = k.dims[3 * vol + 2];
  s.L.nbx = brick_count(s.L.nx);
  s.L.nby = brick_count(s.L.ny);
  s.L.skip = skip;
  return s;
}

Volumes dense_model(const int64_t* vol_start, const float* origin, const int32_t* dims, const float* voxel, int V,
                    int64_t total) {
  return {vol_start, origin, dims, voxel, V, total};
}

Bricks sparse_model(const int64_t* lattice_start, const int64_t* brick_start, const int32_t* brick_index,
                    const float* origin, const int32_t* dims, const float* voxel, int V, int64_t L, int64_t B) {
  return {lattice_start, brick_start, brick_index, nullptr, origin, dims, voxel, V, L, B};
}

// how many voxels / slots D, w and the colours hold
int64_t stored(const Volumes& b) { return b.total; }
int64_t stored(const Bricks& k) { return k.B; }

bool model_ok(const Volumes& b) { return batch_ok(b.V, b.total) && b.vol_start && b.origin && b.dims && b.voxel; }
bool model_ok(const Bricks& k) {
  return pool_ok(k.V, k.L, k.B) && k.lattice_start && k.brick_start && k.brick_index && k.origin && k.dims && k.voxel;
}

// host pointers only, after model_ok: the tables are those of dims
bool host_model_ok(const Volumes& b) { return host_layout_ok(b.vol_start, b.dims, b.V, b.total); }
bool host_model_ok(const Bricks& k) { return host_tables_ok(k.lattice_start, k.brick_start, k.dims, k.V, k.L, k.B); }

// -------------------------------------------------------------------------------------------------------- ray-cast
struct Views {              // device pointers on the device side, host pointers in the twin
  const int32_t* view_volume;   // [R]
  const float* K;               // [R, 4]
  const float* C;               // [R, 12] camera -> volume
  const float* step;            // [V]
  int R, H, W;
  float depth_min, depth_max, min_weight;
  int clip, skip;               // skip: brick skipping, which the dense sampler has none of
};

Views views(const int32_t* view_volume, const float* K, const float* C, const float* step, int R, int H, int W,
            float depth_min, float depth_max, float min_weight, int clip, int skip) {
  return {view_volume, K, C, step, R, H, W, depth_min, depth_max, min_weight, clip, skip};
}

template <int kCc>
struct Colour {             // the colour forms: what they read and write on top
  const float* Cv;              // [total, kCc] beside D and w, or the pool [B, 512, kCc]
  float* image;                 // [R, H, W, kCc]
};
template <>
struct Colour<0> {};

template <int kCc>
__host__ __device__ inline Colour<kCc> colour_of(const float* Cv, float* image) {
  if constexpr (kCc > 0)
    return {Cv, image};
  else
    return {};
}

// pixel (u, v) of view r: depth and normals (when asked for); for kCc > 0 that, and behind it the colour of the hit
// (tsdf_color.hpp) from the depth just written -- the colourless pixel stays one piece of code, which is what keeps the
// colour kernels' sample loop the colourless kernel's (profiles/tsdf_raycast_refactor_identity.txt, 5)
template <typename Model, int kCc>
__host__ __device__ inline void cast_pixel(const Model& m, const Views& vw, const float* D, const float* w,
                                           const Colour<kCc>& col, int r, int u, int v, float* depth, float* normals) {
  const size_t at = ((size_t)r * (size_t)vw.H + (size_t)v) * (size_t)vw.W + (size_t)u;
  const float *K = vw.K + 4 * (size_t)r, *C = vw.C + 12 * (size_t)r;
  const int vol = vw.view_volume[r];
  if constexpr (kCc > 0) {
    cast_pixel<Model, 0>(m, vw, D, w, Colour<0>(), r, u, v, depth, normals);
    const auto s = make_sampler(m, D, w, col.Cv, kCc, vol, vw.skip != 0);
    float c[kCc];
    if (s.ok)
      rc::hit_color<kCc>(s.L, s.colour, K, C, u, v, depth[at], vw.min_weight, c);
    else
      rc::color_none<kCc>(c);
#pragma unroll
    for (int ch = 0; ch < kCc; ++ch) col.image[at * kCc + ch] = c[ch];
  } else {
    float* n = normals ? normals + 3 * at : nullptr;
    const auto s = make_sampler(m, D, w, nullptr, 0, vol, vw.skip != 0);
    if (!s.ok) {
      depth[at] = 0.0f;
      if (n) n[0] = n[1] = n[2] = 0.0f;
      return;
    }
    float nrm[3];
    depth[at] = rc::cast_ray(s.L, K, C, u, v, vw.step[vol], vw.depth_min, vw.depth_max, vw.min_weight, vw.clip != 0,
                             n != nullptr, nrm);
    if (n) {
      n[0] = nrm[0];
      n[1] = nrm[1];
      n[2] = nrm[2];
    }
  }
}

// grid (blocks of 16 x 16 pixels, R); Cv and colour are null and untouched where kCc = 0
template <typename Model, int kCc>
__global__ void __launch_bounds__(kThreads) raycast_kernel(Model m, Views vw, const float* __restrict__ D,
                                                           const float* __restrict__ w, const float* __restrict__ Cv,
                                                           int blocks_x, float* __restrict__ depth,
                                                           float* __restrict__ normals, float* __restrict__ colour) {
  const int r = (int)blockIdx.y;
  const int lane = d3f::lane_id(), wave = (int)threadIdx.x / D3F_WAVE;
  const int bx = (int)blockIdx.x % blocks_x, by = (int)blockIdx.x / blocks_x;
  const int u = bx * kBlockEdge + (wave % kBlockTiles) * kTile + (lane % kTile);
  const int v = by * kBlockEdge + (wave / kBlockTiles) * kTile + (lane / kTile);
  if (u >= vw.W || v >= vw.H) return;
  cast_pixel<Model, kCc>(m, vw, D, w, colour_of<kCc>(Cv, colour), r, u, v, depth, normals);
}

// R, H, W, the depth range and the pointer rules, the same for either model
bool views_ok(const Views& vw, const float* depth) {
  if (vw.R < 0 || vw.R > D3F_TSDF_MAX_VOLUMES || vw.H < 1 || vw.W < 1 || (int64_t)vw.H * vw.W > (int64_t)1 << 30 ||
      !vw.step || !(vw.depth_min >= 0.0f) || !(vw.depth_max >= vw.depth_min) || !(vw.depth_max <= 3.402823466e+38f))
    return false;
  return vw.R == 0 || (vw.view_volume && vw.K && vw.C && depth);
}

template <bool kHost, typename Model, int kCc>
int cast_views(const Model& m, const Views& vw, const float* D, const float* w, const float* Cv, float* depth,
               float* normals, float* color, hipStream_t stream) {
  if constexpr (kHost) {
    const Colour<kCc> col = colour_of<kCc>(Cv, color);
    for (int r = 0; r < vw.R; ++r)
      for (int v = 0; v < vw.H; ++v)
        for (int u = 0; u < vw.W; ++u) cast_pixel<Model, kCc>(m, vw, D, w, col, r, u, v, depth, normals);
  } else {
    const int blocks_x = d3f::cdiv(vw.W, kBlockEdge), blocks_y = d3f::cdiv(vw.H, kBlockEdge);
    if ((int64_t)blocks_x * blocks_y > 0x7fffffff) return D3F_EINVAL;
    const dim3 grid((unsigned)(blocks_x * blocks_y), (unsigned)vw.R);
    raycast_kernel<Model, kCc><<<grid, kThreads, 0, stream>>>(m, vw, D, w, Cv, blocks_x, depth, normals, color);
    D3F_LAUNCH_CHECK();
  }
  return D3F_OK;
}

// every ray-cast entry; channels = 0 is the colourless form, whose Cv and colour image are not looked at.
// R = 0 is D3F_OK before the colour pointers are looked at; the twins check the tables before that.
template <bool kHost, typename Model>
int raycast(const Model& m, const Views& vw, const float* D, const float* w, const float* Cv, int channels,
            float* depth, float* normals, float* color, void* stream) {
  if ((channels != 0 && channels != 1 && channels != 3) || !model_ok(m) || !views_ok(vw, depth) ||
      (vw.R > 0 && stored(m) > 0 && !(D && w)) || (kHost && !host_model_ok(m)))
    return D3F_EINVAL;
  if (vw.R == 0) return D3F_OK;
  if (channels && (!color || (stored(m) > 0 && !Cv))) return D3F_EINVAL;
  const hipStream_t s = (hipStream_t)stream;
  if (channels == 0) return cast_views<kHost, Model, 0>(m, vw, D, w, nullptr, depth, normals, nullptr, s);
  if (channels == 1) return cast_views<kHost, Model, 1>(m, vw, D, w, Cv, depth, normals, color, s);
  return cast_views<kHost, Model, 3>(m, vw, D, w, Cv, depth, normals, color, s);
}

// -------------------------------------------------------------------------------------------------- point sampling
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

template <typename Model, int kCc>
__host__ __device__ inline void sample_point(const Model& m, const Points& p, const float* w, const float* Cv,
                                             int64_t i, float* out) {
  float c[kCc];
  rc::color_none<kCc>(c);
  const auto s = make_sampler(m, w, w, Cv, kCc, point_volume(p, m.V, i), false);   // color_at reads no D: w stands in
  if (s.ok) rc::color_at<kCc>(s.L, s.colour, p.xyz + 3 * i, p.min_weight, c);
#pragma unroll
  for (int ch = 0; ch < kCc; ++ch) out[i * kCc + ch] = c[ch];
}

template <typename Model, int kCc>
__global__ void __launch_bounds__(kThreads) sample_color_kernel(Model m, Points p, const float* __restrict__ w,
                                                                const float* __restrict__ Cv,
                                                                float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < p.N) sample_point<Model, kCc>(m, p, w, Cv, i, out);
}

bool points_ok(int channels, const Points& p, const float* out) {
  return (channels == 1 || channels == 3) && p.N >= 0 && p.point_start && (p.N == 0 || (p.xyz && out)) &&
         voxel_blocks(p.N) <= 0x7fffffff;
}

// host pointers only: point_start rises within [0, N]
bool host_points_ok(const int64_t* point_start, int V, int64_t N) {
  if (point_start[0] < 0 || point_start[V] > N) return false;
  for (int v = 0; v < V; ++v)
    if (point_start[v + 1] < point_start[v]) return false;
  return true;
}

template <bool kHost, typename Model, int kCc>
int sample_points(const Model& m, const Points& p, const float* w, const float* Cv, float* out, hipStream_t stream) {
  if constexpr (kHost) {
    for (int64_t i = 0; i < p.N; ++i) sample_point<Model, kCc>(m, p, w, Cv, i, out);
  } else {
    sample_color_kernel<Model, kCc><<<(unsigned)voxel_blocks(p.N), kThreads, 0, stream>>>(m, p, w, Cv, out);
    D3F_LAUNCH_CHECK();
  }
  return D3F_OK;
}

// every sampling entry
template <bool kHost, typename Model>
int sample_color(const Model& m, const Points& p, const float* w, const float* Cv, int channels, float* out,
                 void* stream) {
  if (!model_ok(m) || (stored(m) > 0 && !(Cv && w)) || !points_ok(channels, p, out) ||
      (kHost && !(host_model_ok(m) && host_points_ok(p.point_start, m.V, p.N))))
    return D3F_EINVAL;
  if (p.N == 0) return D3F_OK;
  if (channels == 1) return sample_points<kHost, Model, 1>(m, p, w, Cv, out, (hipStream_t)stream);
  return sample_points<kHost, Model, 3>(m, p, w, Cv, out, (hipStream_t)stream);
}

}  // namespace

extern "C" {

int d3f_tsdf_raycast(const float* D, const float* w, const float* Cv, int channels, const int64_t* vol_start,
                     const float* origin, const int32_t* dims, const float* voxel, int V, int64_t total_voxels,
                     const int32_t* view_volume, int R, int H, int W, const float* intrinsics,
                     const float* camera_to_volume, const float* step, float depth_min, float depth_max,
                     float min_weight, int clip, float* depth, float* normals, float* color, void* stream) {
  return raycast<false>(
      dense_model(vol_start, origin, dims, voxel, V, total_voxels),
      views(view_volume, intrinsics, camera_to_volume, step, R, H, W, depth_min, depth_max, min_weight, clip, 0), D, w,
      Cv, channels, depth, normals, color, stream);
}

int d3f_tsdf_raycast_host(const float* D, const float* w, const float* Cv, int channels, const int64_t* vol_start,
                          const float* origin, const int32_t* dims, const float* voxel, int V, int64_t total_voxels,
                          const int32_t* view_volume, int R, int H, int W, const float* intrinsics,
                          const float* camera_to_volume, const float* step, float depth_min, float depth_max,
                          float min_weight, int clip, float* depth, float* normals, float* color, void* stream) {
  return raycast<true>(
      dense_model(vol_start, origin, dims, voxel, V, total_voxels),
      views(view_volume, intrinsics, camera_to_volume, step, R, H, W, depth_min, depth_max, min_weight, clip, 0), D, w,
      Cv, channels, depth, normals, color, stream);
}

int d3f_tsdf_raycast_sparse(const float* D, const float* w, const float* Cp, int channels,
                            const int64_t* lattice_start, const int64_t* brick_start, const int32_t* brick_index,
                            const float* origin, const int32_t* dims, const float* voxel, int V,
                            int64_t lattice_bricks, int64_t bricks, const int32_t* view_volume, int R, int H, int W,
                            const float* intrinsics, const float* camera_to_volume, const float* step,
                            float depth_min, float depth_max, float min_weight, int clip, int skip, float* depth,
                            float* normals, float* color, void* stream) {
  return raycast<false>(
      sparse_model(lattice_start, brick_start, brick_index, origin, dims, voxel, V, lattice_bricks, bricks),
      views(view_volume, intrinsics, camera_to_volume, step, R, H, W, depth_min, depth_max, min_weight, clip, skip), D,
      w, Cp, channels, depth, normals, color, stream);
}

int d3f_tsdf_raycast_sparse_host(const float* D, const float* w, const float* Cp, int channels,
                                 const int64_t* lattice_start, const int64_t* brick_start,
                                 const int32_t* brick_index, const float* origin, const int32_t* dims,
                                 const float* voxel, int V, int64_t lattice_bricks, int64_t bricks,
                                 const int32_t* view_volume, int R, int H, int W, const float* intrinsics,
                                 const float* camera_to_volume, const float* step, float depth_min, float depth_max,
                                 float min_weight, int clip, int skip, float* depth, float* normals, float* color,
                                 void* stream) {
  return raycast<true>(
      sparse_model(lattice_start, brick_start, brick_index, origin, dims, voxel, V, lattice_bricks, bricks),
      views(view_volume, intrinsics, camera_to_volume, step, R, H, W, depth_min, depth_max, min_weight, clip, skip), D,
      w, Cp, channels, depth, normals, color, stream);
}

int d3f_tsdf_sample_color(const float* Cv, const float* w, int channels, const int64_t* vol_start, const float* origin,
                          const int32_t* dims, const float* voxel, int V, int64_t total_voxels, const float* points,
                          const int64_t* point_start, int64_t N, float min_weight, float* out, void* stream) {
  return sample_color<false>(dense_model(vol_start, origin, dims, voxel, V, total_voxels),
                             Points{points, point_start, N, min_weight}, w, Cv, channels, out, stream);
}

int d3f_tsdf_sample_color_host(const float* Cv, const float* w, int channels, const int64_t* vol_start,
                               const float* origin, const int32_t* dims, const float* voxel, int V,
                               int64_t total_voxels, const float* points, const int64_t* point_start, int64_t N,
                               float min_weight, float* out, void* stream) {
  return sample_color<true>(dense_model(vol_start, origin, dims, voxel, V, total_voxels),
                            Points{points, point_start, N, min_weight}, w, Cv, channels, out, stream);
}

int d3f_tsdf_sample_color_sparse(const float* Cp, const float* w, int channels, const int64_t* lattice_start,
                                 const int64_t* brick_start, const int32_t* brick_index, const float* origin,
                                 const int32_t* dims, const float* voxel, int V, int64_t lattice_bricks,
                                 int64_t bricks, const float* points, const int64_t* point_start, int64_t N,
                                 float min_weight, float* out, void* stream) {
  return sample_color<false>(
      sparse_model(lattice_start, brick_start, brick_index, origin, dims, voxel, V, lattice_bricks, bricks),
      Points{points, point_start, N, min_weight}, w, Cp, channels, out, stream);
}

int d3f_tsdf_sample_color_sparse_host(const float* Cp, const float* w, int channels, const int64_t* lattice_start,
                                      const int64_t* brick_start, const int32_t* brick_index, const float* origin,
                                      const int32_t* dims, const float* voxel, int V, int64_t lattice_bricks,
                                      int64_t bricks, const float* points, const int64_t* point_start, int64_t N,
                                      float min_weight, float* out, void* stream) {
  return sample_color<true>(
      sparse_model(lattice_start, brick_start, brick_index, origin, dims, voxel, V, lattice_bricks, bricks),
      Points{points, point_start, N, min_weight}, w, Cp, channels, out, stream);
}

}  // extern "C"
