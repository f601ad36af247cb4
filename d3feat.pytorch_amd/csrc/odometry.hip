// Depth odometry on the device: the depth pyramid and batched frame-to-frame projective point-to-plane ICP
// (include/d3feat_hip.h: d3f_depth_pyramid, d3f_depth_odometry_step, d3f_depth_odometry; the rule is csrc/odometry.hpp).
// All P pairs advance together, without host synchronisation and with a launch sequence that depends on the level
// table and the iteration counts alone: one setup launch, then per iteration an association launch and a fit launch,
// coarsest level first, and at the end one more association at level 0 and a finishing launch.
//   pyramid    one launch per level, one thread per output pixel of all frames; a tiny launch writes the intrinsics of
//              every level of every frame.
//   associate  grid (chunks of the level, P): the pair is blockIdx.y, so the pair, its two images, their intrinsics,
//              T rounded to f32 and the level's dimensions are workgroup-uniform and come through scalar loads.  A
//              workgroup of 256 threads serves kChunk = 1024 consecutive raster pixels of the pair's moving image, a
//              thread the pixels tid, tid + 256, ... of the chunk in that order (coalesced reads of the moving image);
//              the fixed image is gathered at the projected pixel and its four neighbours -- neighbouring moving pixels
//              project to neighbouring fixed pixels, so the gathers of a wave fall into a few cache lines.  Vertices
//              and normals are recomputed from the depth: nothing but the pyramid is read.
//   fit        one wave per pair adds the pair's chunk sums (lane = chunk mod 64, chunks ascending, then the
//              butterfly) and one lane runs plane::plane_step: icp.hip's scheme.
// Determinism: no floating-point atomic.  A lane adds its pixels in a fixed order, the wave is reduced by common.hpp's
// butterfly, the 4 waves are added in wave order through LDS, and the pair's chunks by one wave in the order above.
// Every order depends on H, W and the level alone, so a pair's sums and its whole trajectory are bit-identical alone,
// inside any batch, and from run to run.  The host twins run the same odometry.hpp text pixel by pixel in raster order
// and make no GPU call.  The arguments of a batch, the set-up and finishing rules, the workspace, the reduction of a
// pair's chunks and the coarse-to-fine schedule are in odometry_batch.hpp, which rgbd_odometry.hip marches by too.
#include "odometry_batch.hpp"

namespace {

using namespace d3f::odo;

// -------------------------------------------------------------------------------------------------------- pyramid
template <typename DepthT>
__global__ void __launch_bounds__(kThreads) pyramid_level0_kernel(const DepthT* __restrict__ depth, int64_t frames,
                                                                  int64_t pixels, int64_t frame_pixels,
                                                                  float depth_scale, float depth_max,
                                                                  float* __restrict__ pyr) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= frames * pixels) return;
  const int64_t f = i / pixels, local = i - f * pixels;
  pyr[f * frame_pixels + local] = level0_pixel(depth, (size_t)i, depth_scale, depth_max);
}

// level l -> l + 1: (Hs, Ws) the source's dimensions at offset src_off of a frame, the result at dst_off
__global__ void __launch_bounds__(kThreads) pyramid_down_kernel(float* pyr, int64_t frames, int64_t frame_pixels,
                                                                int Hs, int Ws, int64_t src_off, int64_t dst_off,
                                                                float depth_diff) {
  const int Hn = Hs >> 1, Wn = Ws >> 1;
  const int64_t pixels = (int64_t)Hn * Wn;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= frames * pixels) return;
  const int64_t f = i / pixels, local = i - f * pixels;
  const int v = (int)(local / Wn), u = (int)(local - (int64_t)v * Wn);
  pyr[f * frame_pixels + dst_off + local] = down_pixel(pyr + f * frame_pixels + src_off, Ws, u, v, depth_diff);
}

D3F_HD inline void frame_intrinsics(const float* K, int levels, float* out) {
  for (int k = 0; k < 4; ++k) out[k] = K[k];
  for (int l = 1; l < levels; ++l) down_intrinsics(out + 4 * (l - 1), out + 4 * l);
}

__global__ void __launch_bounds__(kThreads) pyramid_intrinsics_kernel(const float* __restrict__ K, int F, int levels,
                                                                      float* __restrict__ KL) {
  const int f = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (f < F) frame_intrinsics(K + 4 * (size_t)f, levels, KL + 4 * (size_t)f * (size_t)levels);
}

// ------------------------------------------------------------------------------------------------------ odometry
// kRun: the whole odometry (the outputs of a stopped pair are written here); else the step entry point
template <bool kRun>
__global__ void __launch_bounds__(kThreads) odo_setup_kernel(const OdoArgs A) {
  const int p = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (p >= A.P) return;
  const int st = pair_status(A, p);
  for (int k = 0; k < 12; ++k) A.T_cur[12 * (size_t)p + k] = A.T_init[12 * (size_t)p + k];
  A.done[p] = st != 0;
  A.sing[p] = 0;
  if constexpr (kRun) {
    if (st) {
      const double zero[kSums] = {};
      finish_pair(A, p, st, false, zero, A.T_init + 12 * (size_t)p);
    }
  }
}

// grid (chunks of the level, P)
__global__ void __launch_bounds__(kThreads) odo_associate_kernel(const OdoArgs A, int level) {
  const int p = (int)blockIdx.y, chunk = (int)blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int Hl = level_h(A.H, level), Wl = level_w(A.W, level), pixels = Hl * Wl;
  const int first = chunk * kChunk;
  if (A.done[p]) {   // (uniform over the workgroup: nothing is summed for this pair; its index is -1 everywhere)
    if (A.index)
      for (int k = 0; k < kPerThread; ++k) {
        const int i = first + k * kThreads + (int)threadIdx.x;
        if (i < pixels) A.index[(size_t)p * (size_t)pixels + (size_t)i] = -1;
      }
    return;
  }
  const int a = A.pairs[2 * p], b = A.pairs[2 * p + 1];   // in [0, F): the setup launch stopped the others
  PairLevel L;
  make_level(A, a, b, level, A.T_cur + 12 * (size_t)p, L);

  double acc[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
  for (int k = 0; k < kPerThread; ++k) {
    const int i = first + k * kThreads + (int)threadIdx.x;
    if (i >= pixels) break;
    const int v = i / Wl, u = i - v * Wl;
    float av[3], yv[3], nv[3];
    const int t = associate(L, u, v, av, yv, nv);
    if (t >= 0) add_pixel(acc, av, yv, nv);
    if (A.index) A.index[(size_t)p * (size_t)pixels + (size_t)i] = t;
  }
  d3f::wave_sum_f64(acc);
  __shared__ double red[kThreads / 64][kSums];
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kSums; ++k) red[wave][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < kSums) {
    double s = red[0][threadIdx.x];
    for (int w = 1; w < kThreads / 64; ++w) s += red[w][threadIdx.x];
    A.partial[((size_t)p * (size_t)gridDim.x + (size_t)chunk) * kSums + threadIdx.x] = s;
  }
}

enum { kFit = 0, kFinish = 1, kWriteSums = 2 };

// one wave per pair: the pair's sums, then the fit / the final outputs / the sums as they are
template <int kWhat>
__global__ void __launch_bounds__(64) odo_pair_kernel(const OdoArgs A, int level, int chunks) {
  const int p = (int)blockIdx.x, lane = (int)threadIdx.x;
  const bool done = A.done[p] != 0;   // (uniform over the wave)
  if (done && kWhat != kWriteSums) return;
  double v[kSums] = {};
  if (!done) pair_sums(A.partial, p, chunks, lane, v);
  if (lane != 0) return;
  double* T = A.T_cur + 12 * (size_t)p;
  if constexpr (kWhat == kFit) {
    double Tk[12], Tn[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) Tk[k] = T[k];
    bool singular;
    if (fit(v, Tk, Tn, &singular)) {
#pragma unroll
      for (int k = 0; k < 12; ++k) T[k] = Tn[k];
    }
    if (level == 0) A.sing[p] = singular ? 1 : 0;
  } else if constexpr (kWhat == kFinish) {
    finish_pair(A, p, 0, A.sing[p] != 0, v, T);
  } else {
#pragma unroll
    for (int k = 0; k < kSums; ++k) A.sums[(size_t)p * kSums + k] = v[k];
  }
}

// ------------------------------------------------------------------------------------------------------ host side
bool pyramid_ok(const void* depth, int F, int H, int W, const float* K, int levels, float depth_scale, float depth_max,
                float depth_diff, const float* pyr, const float* KL) {
  return depth && K && pyr && KL && shape_ok(F, H, W, levels) && depth_scale > 0.0f && depth_max > 0.0f &&
         depth_diff >= 0.0f;
}

// the sums of one association of the valid pair (a, b) on the host: raster order
void host_sums(const OdoArgs& A, int p, int level, const double* T, double* sums, int32_t* index) {
  PairLevel L;
  make_level(A, A.pairs[2 * p], A.pairs[2 * p + 1], level, T, L);
  for (int k = 0; k < kSums; ++k) sums[k] = 0.0;
  for (int v = 0; v < L.H; ++v)
    for (int u = 0; u < L.W; ++u) {
      float av[3], yv[3], nv[3];
      const int t = associate(L, u, v, av, yv, nv);
      if (t >= 0) add_pixel(sums, av, yv, nv);
      if (index) index[(size_t)v * (size_t)L.W + (size_t)u] = t;
    }
}

template <typename DepthT>
void pyramid_host(const DepthT* depth, int F, int H, int W, const float* K, int levels, float depth_scale,
                  float depth_max, float depth_diff, float* pyr, float* KL) {
  const int64_t pixels = (int64_t)H * W, frame_pixels = level_offset(H, W, levels);
  for (int f = 0; f < F; ++f) {
    float* frame = pyr + (size_t)f * (size_t)frame_pixels;
    for (int64_t i = 0; i < pixels; ++i)
      frame[i] = level0_pixel(depth, (size_t)f * (size_t)pixels + (size_t)i, depth_scale, depth_max);
    for (int l = 0; l + 1 < levels; ++l) {
      const int Hs = level_h(H, l), Ws = level_w(W, l), Hn = Hs >> 1, Wn = Ws >> 1;
      const float* src = frame + level_offset(H, W, l);
      float* dst = frame + level_offset(H, W, l + 1);
      for (int v = 0; v < Hn; ++v)
        for (int u = 0; u < Wn; ++u) dst[(size_t)v * (size_t)Wn + (size_t)u] = down_pixel(src, Ws, u, v, depth_diff);
    }
    frame_intrinsics(K + 4 * (size_t)f, levels, KL + 4 * (size_t)f * (size_t)levels);
  }
}

}  // namespace

extern "C" {

int64_t d3f_depth_pyramid_pixels(int H, int W, int levels) {
  return shape_ok(1, H, W, levels) ? level_offset(H, W, levels) : 0;
}

int d3f_depth_pyramid(const void* depth, int depth_is_f32, int F, int H, int W, const float* intrinsics, int levels,
                      float depth_scale, float depth_max, float depth_diff, float* pyramid, float* level_intrinsics,
                      void* stream) {
  if (!pyramid_ok(depth, F, H, W, intrinsics, levels, depth_scale, depth_max, depth_diff, pyramid, level_intrinsics))
    return D3F_EINVAL;
  const int64_t pixels = (int64_t)H * W, frame_pixels = level_offset(H, W, levels);
  const int64_t blocks = ((int64_t)F * pixels + kThreads - 1) / kThreads;
  if (blocks > 0x7fffffff) return D3F_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (depth_is_f32)
    pyramid_level0_kernel<float><<<(unsigned)blocks, kThreads, 0, s>>>((const float*)depth, F, pixels, frame_pixels,
                                                                       depth_scale, depth_max, pyramid);
  else
    pyramid_level0_kernel<uint16_t><<<(unsigned)blocks, kThreads, 0, s>>>((const uint16_t*)depth, F, pixels,
                                                                          frame_pixels, depth_scale, depth_max, pyramid);
  D3F_LAUNCH_CHECK();
  for (int l = 0; l + 1 < levels; ++l) {
    const int Hs = level_h(H, l), Ws = level_w(W, l);
    const int64_t n = (int64_t)F * (Hs >> 1) * (Ws >> 1);
    pyramid_down_kernel<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, s>>>(
        pyramid, F, frame_pixels, Hs, Ws, level_offset(H, W, l), level_offset(H, W, l + 1), depth_diff);
    D3F_LAUNCH_CHECK();
  }
  pyramid_intrinsics_kernel<<<(unsigned)d3f::cdiv(F, kThreads), kThreads, 0, s>>>(intrinsics, F, levels,
                                                                                  level_intrinsics);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_depth_pyramid_host(const void* depth, int depth_is_f32, int F, int H, int W, const float* intrinsics,
                           int levels, float depth_scale, float depth_max, float depth_diff, float* pyramid,
                           float* level_intrinsics) {
  if (!pyramid_ok(depth, F, H, W, intrinsics, levels, depth_scale, depth_max, depth_diff, pyramid, level_intrinsics))
    return D3F_EINVAL;
  if (depth_is_f32)
    pyramid_host((const float*)depth, F, H, W, intrinsics, levels, depth_scale, depth_max, depth_diff, pyramid,
                 level_intrinsics);
  else
    pyramid_host((const uint16_t*)depth, F, H, W, intrinsics, levels, depth_scale, depth_max, depth_diff, pyramid,
                 level_intrinsics);
  return D3F_OK;
}

size_t d3f_depth_odometry_ws_bytes(int P, int H, int W) {
  if (P < 0 || H < 1 || W < 1 || (int64_t)H * (int64_t)W > (int64_t)1 << 30) return 0;
  return odo_layout(nullptr, P, H, W).bytes;
}

int d3f_depth_odometry_step(const float* pyramid, const float* level_intrinsics, int F, int H, int W, int levels,
                            const int32_t* pairs, int P, const double* T, int level, float max_distance,
                            float depth_diff, double* sums, int32_t* index, void* ws, size_t ws_bytes, void* stream) {
  OdoArgs a = {};
  int rc = odo_prepare(pyramid, level_intrinsics, F, H, W, levels, pairs, P, T, max_distance, depth_diff, a);
  if (rc != D3F_OK) return rc;
  if (level < 0 || level >= levels || (P > 0 && !sums)) return D3F_EINVAL;
  if (P == 0) return D3F_OK;
  if ((rc = odo_workspace(a, ws, ws_bytes)) != D3F_OK) return rc;
  a.sums = sums;
  a.index = index;
  hipStream_t s = (hipStream_t)stream;
  const int chunks = chunks_of(H, W, level);
  odo_setup_kernel<false><<<(unsigned)d3f::cdiv(P, kThreads), kThreads, 0, s>>>(a);
  D3F_LAUNCH_CHECK();
  odo_associate_kernel<<<dim3((unsigned)chunks, (unsigned)P), kThreads, 0, s>>>(a, level);
  odo_pair_kernel<kWriteSums><<<(unsigned)P, 64, 0, s>>>(a, level, chunks);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_depth_odometry_step_host(const float* pyramid, const float* level_intrinsics, int F, int H, int W, int levels,
                                 const int32_t* pairs, int P, const double* T, int level, float max_distance,
                                 float depth_diff, double* sums, int32_t* index) {
  OdoArgs a = {};
  const int rc = odo_prepare(pyramid, level_intrinsics, F, H, W, levels, pairs, P, T, max_distance, depth_diff, a);
  if (rc != D3F_OK) return rc;
  if (level < 0 || level >= levels || (P > 0 && !sums)) return D3F_EINVAL;
  const size_t pixels = (size_t)level_h(H, level) * (size_t)level_w(W, level);
  for (int p = 0; p < P; ++p) {
    int32_t* idx = index ? index + (size_t)p * pixels : nullptr;
    if (pair_status(a, p)) {
      for (int k = 0; k < kSums; ++k) sums[(size_t)p * kSums + k] = 0.0;
      if (idx)
        for (size_t i = 0; i < pixels; ++i) idx[i] = -1;
      continue;
    }
    host_sums(a, p, level, T + 12 * (size_t)p, sums + (size_t)p * kSums, idx);
  }
  return D3F_OK;
}

int d3f_depth_odometry(const float* pyramid, const float* level_intrinsics, int F, int H, int W, int levels,
                       const int32_t* pairs, int P, const double* T_init, const int32_t* iterations_host,
                       float max_distance, float depth_diff, double* T, int32_t* count, double* rmse, int32_t* status,
                       double* information, void* ws, size_t ws_bytes, void* stream) {
  OdoArgs a = {};
  int rc = odo_prepare(pyramid, level_intrinsics, F, H, W, levels, pairs, P, T_init, max_distance, depth_diff, a);
  if (rc != D3F_OK) return rc;
  if (!iterations_ok(iterations_host, levels) || (P > 0 && (!T || !count || !rmse || !status))) return D3F_EINVAL;
  if (P == 0) return D3F_OK;
  if ((rc = odo_workspace(a, ws, ws_bytes)) != D3F_OK) return rc;
  a.T = T;
  a.count = count;
  a.rmse = rmse;
  a.status = status;
  a.info = information;
  hipStream_t s = (hipStream_t)stream;
  odo_setup_kernel<true><<<(unsigned)d3f::cdiv(P, kThreads), kThreads, 0, s>>>(a);
  D3F_LAUNCH_CHECK();
  const bool launched = march(
      H, W, levels, iterations_host,
      [&](int l, int chunks) {
        odo_associate_kernel<<<dim3((unsigned)chunks, (unsigned)P), kThreads, 0, s>>>(a, l);
        odo_pair_kernel<kFit><<<(unsigned)P, 64, 0, s>>>(a, l, chunks);
      },
      [&](int chunks) {
        odo_associate_kernel<<<dim3((unsigned)chunks, (unsigned)P), kThreads, 0, s>>>(a, 0);
        odo_pair_kernel<kFinish><<<(unsigned)P, 64, 0, s>>>(a, 0, chunks);
      });
  return launched ? D3F_OK : D3F_ELAUNCH;
}

int d3f_depth_odometry_host(const float* pyramid, const float* level_intrinsics, int F, int H, int W, int levels,
                            const int32_t* pairs, int P, const double* T_init, const int32_t* iterations_host,
                            float max_distance, float depth_diff, double* T, int32_t* count, double* rmse,
                            int32_t* status, double* information) {
  OdoArgs a = {};
  const int rc = odo_prepare(pyramid, level_intrinsics, F, H, W, levels, pairs, P, T_init, max_distance, depth_diff, a);
  if (rc != D3F_OK) return rc;
  if (!iterations_ok(iterations_host, levels) || (P > 0 && (!T || !count || !rmse || !status))) return D3F_EINVAL;
  a.T = T;
  a.count = count;
  a.rmse = rmse;
  a.status = status;
  a.info = information;
  for (int p = 0; p < P; ++p) {
    double sums[kSums] = {}, Tk[12], Tn[12];
    const int st = pair_status(a, p);
    if (st) {
      finish_pair(a, p, st, false, sums, T_init + 12 * (size_t)p);
      continue;
    }
    for (int k = 0; k < 12; ++k) Tk[k] = T_init[12 * (size_t)p + k];
    bool last_singular = false;
    for (int l = levels - 1; l >= 0; --l)
      for (int it = 0; it < iterations_host[l]; ++it) {
        host_sums(a, p, l, Tk, sums, nullptr);
        bool singular;
        if (fit(sums, Tk, Tn, &singular))
          for (int k = 0; k < 12; ++k) Tk[k] = Tn[k];
        if (l == 0) last_singular = singular;
      }
    host_sums(a, p, 0, Tk, sums, nullptr);
    finish_pair(a, p, 0, last_singular, sums, Tk);
  }
  return D3F_OK;
}

}  // extern "C"
