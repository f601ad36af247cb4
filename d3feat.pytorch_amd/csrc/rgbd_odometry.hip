// RGB-D odometry on the device: the intensity pyramid and batched frame-to-frame tracking with a geometric and a
// photometric term (include/d3feat_hip.h: d3f_rgbd_pyramid, d3f_rgbd_odometry_step, d3f_rgbd_odometry; the rule is
// csrc/rgbd_odometry.hpp on top of csrc/odometry.hpp).  The launch structure, the workspace and the determinism scheme
// are odometry.hip's, through odometry_batch.hpp: one setup launch, then per iteration an association launch over
// (chunks of 1024 pixels, pairs) and a fit launch of one wave per pair, coarsest level first, one more association at
// level 0 and a finishing launch; no host synchronisation, no floating-point atomic, every summation order fixed by
// H, W and the level alone.  What is new:
//   pyramid    the intensity only (the depth pyramid is d3f_depth_pyramid's): one launch per level, one thread per
//              output pixel of all frames.
//   associate  after odo::associate has accepted a pixel, the thread reads its own intensity (the same coalesced
//              address pattern as its depth) and gathers the fixed intensity over the 4 x 4 block around the
//              projection, without the corners (12 values in 4 rows); neighbouring moving pixels project to
//              neighbouring fixed pixels, so a wave's gathers fall into a few cache lines, as for the depth.
//   sums       31 per pair: the 29 of the depth tracker, n_photo and sum r_I^2.  photo_weight == 0 is uniform over the
//              launch and skips the gather altogether.
// The host twins run the same header text pixel by pixel in raster order and make no GPU call.
#include "odometry_batch.hpp"
#include "rgbd_odometry.hpp"

namespace {

using namespace d3f::odo;
namespace rgbd = d3f::rgbd;

constexpr int kSums31 = rgbd::kSums;
static_assert(kSums31 == D3F_RGBD_SUMS, "the header's count of sums");
static_assert(kSums31 <= kThreads, "a thread per sum in the workgroup's reduction");

struct RgbdArgs {
  OdoArgs o;
  const float* inten;       // [F, frame_pixels]
  int32_t* n_photo;         // [P] (the odometry entry point)
  float photo_weight;
};

enum { kColorRgb8 = D3F_RGBD_COLOR_RGB8, kColorGrey8 = D3F_RGBD_COLOR_GREY8, kColorF32 = D3F_RGBD_COLOR_F32 };

template <int kKind>
D3F_HD inline float level0_intensity(const void* color, size_t i) {
  if constexpr (kKind == kColorRgb8) return rgbd::intensity_rgb((const uint8_t*)color + 3 * i);
  else if constexpr (kKind == kColorGrey8) return rgbd::intensity_grey(((const uint8_t*)color)[i]);
  else return ((const float*)color)[i];
}

// -------------------------------------------------------------------------------------------------------- pyramid
template <int kKind>
__global__ void __launch_bounds__(kThreads) intensity_level0_kernel(const void* __restrict__ color, int64_t frames,
                                                                    int64_t pixels, int64_t frame_pixels,
                                                                    float* __restrict__ inten) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= frames * pixels) return;
  const int64_t f = i / pixels, local = i - f * pixels;
  inten[f * frame_pixels + local] = level0_intensity<kKind>(color, (size_t)i);
}

// level l -> l + 1: (Hs, Ws) the source's dimensions at offset src_off of a frame, the result at dst_off
__global__ void __launch_bounds__(kThreads) intensity_down_kernel(float* inten, int64_t frames, int64_t frame_pixels,
                                                                  int Hs, int Ws, int64_t src_off, int64_t dst_off) {
  const int Hn = Hs >> 1, Wn = Ws >> 1;
  const int64_t pixels = (int64_t)Hn * Wn;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= frames * pixels) return;
  const int64_t f = i / pixels, local = i - f * pixels;
  const int v = (int)(local / Wn), u = (int)(local - (int64_t)v * Wn);
  inten[f * frame_pixels + dst_off + local] = rgbd::down_pixel(inten + f * frame_pixels + src_off, Ws, u, v);
}

// ------------------------------------------------------------------------------------------------------ odometry
// what the finishing step writes for pair p (finish_pair, and the photometric count beside it)
D3F_HD inline void finish_rgbd(const RgbdArgs& A, int p, int st, bool singular, const double* sums, const double* T) {
  finish_pair(A.o, p, st, singular, sums, T);
  A.n_photo[p] = A.o.status[p] ? 0 : (int)sums[rgbd::kPhotoCount];
}

// one accepted-or-not moving pixel (u, v) of the level L: its sums into acc, its index returned
D3F_HD inline int add_moving_pixel(const PairLevel& L, const float* IA, const float* IB, float photo_weight, int u,
                                   int v, double* acc) {
  float av[3], yv[3], nv[3];
  const int t = associate(L, u, v, av, yv, nv);
  if (t < 0) return t;
  add_pixel(acc, av, yv, nv);
  if (photo_weight != 0.0f) {   // (uniform over a launch)
    float r, q[3];
    if (rgbd::photometric(IB, L.H, L.W, L.Kb, IA[(size_t)v * (size_t)L.W + (size_t)u], av, &r, q))
      rgbd::add_photometric(acc, av, q, r, (double)photo_weight);
  }
  return t;
}

// kRun: the whole odometry (the outputs of a stopped pair are written here); else the step entry point
template <bool kRun>
__global__ void __launch_bounds__(kThreads) rgbd_setup_kernel(const RgbdArgs A) {
  const int p = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (p >= A.o.P) return;
  const int st = pair_status(A.o, p);
  for (int k = 0; k < 12; ++k) A.o.T_cur[12 * (size_t)p + k] = A.o.T_init[12 * (size_t)p + k];
  A.o.done[p] = st != 0;
  A.o.sing[p] = 0;
  if constexpr (kRun) {
    if (st) {
      const double zero[kSums31] = {};
      finish_rgbd(A, p, st, false, zero, A.o.T_init + 12 * (size_t)p);
    }
  }
}

// grid (chunks of the level, P)
__global__ void __launch_bounds__(kThreads) rgbd_associate_kernel(const RgbdArgs A, int level) {
  const int p = (int)blockIdx.y, chunk = (int)blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int Hl = level_h(A.o.H, level), Wl = level_w(A.o.W, level), pixels = Hl * Wl;
  const int first = chunk * kChunk;
  if (A.o.done[p]) {   // (uniform over the workgroup: nothing is summed for this pair; its index is -1 everywhere)
    if (A.o.index)
      for (int k = 0; k < kPerThread; ++k) {
        const int i = first + k * kThreads + (int)threadIdx.x;
        if (i < pixels) A.o.index[(size_t)p * (size_t)pixels + (size_t)i] = -1;
      }
    return;
  }
  const int a = A.o.pairs[2 * p], b = A.o.pairs[2 * p + 1];   // in [0, F): the setup launch stopped the others
  PairLevel L;
  make_level(A.o, a, b, level, A.o.T_cur + 12 * (size_t)p, L);
  const size_t off = (size_t)level_offset(A.o.H, A.o.W, level);
  const float* IA = A.inten + (size_t)a * (size_t)A.o.frame_pixels + off;
  const float* IB = A.inten + (size_t)b * (size_t)A.o.frame_pixels + off;

  double acc[kSums31];
#pragma unroll
  for (int k = 0; k < kSums31; ++k) acc[k] = 0.0;
  for (int k = 0; k < kPerThread; ++k) {
    const int i = first + k * kThreads + (int)threadIdx.x;
    if (i >= pixels) break;
    const int v = i / Wl, u = i - v * Wl;
    const int t = add_moving_pixel(L, IA, IB, A.photo_weight, u, v, acc);
    if (A.o.index) A.o.index[(size_t)p * (size_t)pixels + (size_t)i] = t;
  }
  d3f::wave_sum_f64(acc);
  __shared__ double red[kThreads / 64][kSums31];
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kSums31; ++k) red[wave][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < kSums31) {
    double s = red[0][threadIdx.x];
    for (int w = 1; w < kThreads / 64; ++w) s += red[w][threadIdx.x];
    A.o.partial[((size_t)p * (size_t)gridDim.x + (size_t)chunk) * kSums31 + threadIdx.x] = s;
  }
}

enum { kFit = 0, kFinish = 1, kWriteSums = 2 };

// one wave per pair: the pair's sums, then the fit / the final outputs / the sums as they are
template <int kWhat>
__global__ void __launch_bounds__(64) rgbd_pair_kernel(const RgbdArgs A, int level, int chunks) {
  const int p = (int)blockIdx.x, lane = (int)threadIdx.x;
  const bool done = A.o.done[p] != 0;   // (uniform over the wave)
  if (done && kWhat != kWriteSums) return;
  double v[kSums31] = {};
  if (!done) pair_sums(A.o.partial, p, chunks, lane, v);
  if (lane != 0) return;
  double* T = A.o.T_cur + 12 * (size_t)p;
  if constexpr (kWhat == kFit) {
    double Tk[12], Tn[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) Tk[k] = T[k];
    bool singular;
    if (fit(v, Tk, Tn, &singular)) {
#pragma unroll
      for (int k = 0; k < 12; ++k) T[k] = Tn[k];
    }
    if (level == 0) A.o.sing[p] = singular ? 1 : 0;
  } else if constexpr (kWhat == kFinish) {
    finish_rgbd(A, p, 0, A.o.sing[p] != 0, v, T);
  } else {
#pragma unroll
    for (int k = 0; k < kSums31; ++k) A.o.sums[(size_t)p * kSums31 + k] = v[k];
  }
}

// ------------------------------------------------------------------------------------------------------ host side
bool color_ok(const void* color, int kind, int F, int H, int W, int levels, const float* inten) {
  return color && inten && shape_ok(F, H, W, levels) && kind >= kColorRgb8 && kind <= kColorF32;
}

bool weight_ok(float w) { return w >= 0.0f && rgbd::finite(w); }

template <int kKind>
void intensity_host(const void* color, int F, int H, int W, int levels, float* inten) {
  const int64_t pixels = (int64_t)H * W, frame_pixels = level_offset(H, W, levels);
  for (int f = 0; f < F; ++f) {
    float* frame = inten + (size_t)f * (size_t)frame_pixels;
    for (int64_t i = 0; i < pixels; ++i) frame[i] = level0_intensity<kKind>(color, (size_t)f * (size_t)pixels + (size_t)i);
    for (int l = 0; l + 1 < levels; ++l) {
      const int Hs = level_h(H, l), Ws = level_w(W, l), Hn = Hs >> 1, Wn = Ws >> 1;
      const float* src = frame + level_offset(H, W, l);
      float* dst = frame + level_offset(H, W, l + 1);
      for (int v = 0; v < Hn; ++v)
        for (int u = 0; u < Wn; ++u) dst[(size_t)v * (size_t)Wn + (size_t)u] = rgbd::down_pixel(src, Ws, u, v);
    }
  }
}

// the sums of one association of the valid pair p on the host: raster order
void host_sums(const RgbdArgs& A, int p, int level, const double* T, double* sums, int32_t* index) {
  PairLevel L;
  const int a = A.o.pairs[2 * p], b = A.o.pairs[2 * p + 1];
  make_level(A.o, a, b, level, T, L);
  const size_t off = (size_t)level_offset(A.o.H, A.o.W, level);
  const float* IA = A.inten + (size_t)a * (size_t)A.o.frame_pixels + off;
  const float* IB = A.inten + (size_t)b * (size_t)A.o.frame_pixels + off;
  for (int k = 0; k < kSums31; ++k) sums[k] = 0.0;
  for (int v = 0; v < L.H; ++v)
    for (int u = 0; u < L.W; ++u) {
      const int t = add_moving_pixel(L, IA, IB, A.photo_weight, u, v, sums);
      if (index) index[(size_t)v * (size_t)L.W + (size_t)u] = t;
    }
}

int rgbd_prepare(const float* pyr, const float* inten, const float* KL, int F, int H, int W, int levels,
                 const int32_t* pairs, int P, const double* T, float max_distance, float depth_diff, float photo_weight,
                 RgbdArgs& a) {
  if (!inten || !weight_ok(photo_weight)) return D3F_EINVAL;
  a.inten = inten;
  a.photo_weight = photo_weight;
  return odo_prepare(pyr, KL, F, H, W, levels, pairs, P, T, max_distance, depth_diff, a.o);
}

}  // namespace

extern "C" {

int d3f_rgbd_pyramid(const void* color, int color_kind, int F, int H, int W, int levels, float* intensity,
                     void* stream) {
  if (!color_ok(color, color_kind, F, H, W, levels, intensity)) return D3F_EINVAL;
  const int64_t pixels = (int64_t)H * W, frame_pixels = level_offset(H, W, levels);
  const int64_t blocks = ((int64_t)F * pixels + kThreads - 1) / kThreads;
  if (blocks > 0x7fffffff) return D3F_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (color_kind == kColorRgb8)
    intensity_level0_kernel<kColorRgb8><<<(unsigned)blocks, kThreads, 0, s>>>(color, F, pixels, frame_pixels, intensity);
  else if (color_kind == kColorGrey8)
    intensity_level0_kernel<kColorGrey8><<<(unsigned)blocks, kThreads, 0, s>>>(color, F, pixels, frame_pixels, intensity);
  else
    intensity_level0_kernel<kColorF32><<<(unsigned)blocks, kThreads, 0, s>>>(color, F, pixels, frame_pixels, intensity);
  D3F_LAUNCH_CHECK();
  for (int l = 0; l + 1 < levels; ++l) {
    const int Hs = level_h(H, l), Ws = level_w(W, l);
    const int64_t n = (int64_t)F * (Hs >> 1) * (Ws >> 1);
    intensity_down_kernel<<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, s>>>(
        intensity, F, frame_pixels, Hs, Ws, level_offset(H, W, l), level_offset(H, W, l + 1));
    D3F_LAUNCH_CHECK();
  }
  return D3F_OK;
}

int d3f_rgbd_pyramid_host(const void* color, int color_kind, int F, int H, int W, int levels, float* intensity) {
  if (!color_ok(color, color_kind, F, H, W, levels, intensity)) return D3F_EINVAL;
  if (color_kind == kColorRgb8) intensity_host<kColorRgb8>(color, F, H, W, levels, intensity);
  else if (color_kind == kColorGrey8) intensity_host<kColorGrey8>(color, F, H, W, levels, intensity);
  else intensity_host<kColorF32>(color, F, H, W, levels, intensity);
  return D3F_OK;
}

size_t d3f_rgbd_odometry_ws_bytes(int P, int H, int W) {
  if (P < 0 || H < 1 || W < 1 || (int64_t)H * (int64_t)W > (int64_t)1 << 30) return 0;
  return odo_layout(nullptr, P, H, W, kSums31).bytes;
}

int d3f_rgbd_odometry_step(const float* pyramid, const float* intensity, const float* level_intrinsics, int F, int H,
                           int W, int levels, const int32_t* pairs, int P, const double* T, int level,
                           float max_distance, float depth_diff, float photo_weight, double* sums, int32_t* index,
                           void* ws, size_t ws_bytes, void* stream) {
  RgbdArgs a = {};
  int rc = rgbd_prepare(pyramid, intensity, level_intrinsics, F, H, W, levels, pairs, P, T, max_distance, depth_diff,
                        photo_weight, a);
  if (rc != D3F_OK) return rc;
  if (level < 0 || level >= levels || (P > 0 && !sums)) return D3F_EINVAL;
  if (P == 0) return D3F_OK;
  if ((rc = odo_workspace(a.o, ws, ws_bytes, kSums31)) != D3F_OK) return rc;
  a.o.sums = sums;
  a.o.index = index;
  hipStream_t s = (hipStream_t)stream;
  const int chunks = chunks_of(H, W, level);
  rgbd_setup_kernel<false><<<(unsigned)d3f::cdiv(P, kThreads), kThreads, 0, s>>>(a);
  D3F_LAUNCH_CHECK();
  rgbd_associate_kernel<<<dim3((unsigned)chunks, (unsigned)P), kThreads, 0, s>>>(a, level);
  rgbd_pair_kernel<kWriteSums><<<(unsigned)P, 64, 0, s>>>(a, level, chunks);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_rgbd_odometry_step_host(const float* pyramid, const float* intensity, const float* level_intrinsics, int F,
                                int H, int W, int levels, const int32_t* pairs, int P, const double* T, int level,
                                float max_distance, float depth_diff, float photo_weight, double* sums,
                                int32_t* index) {
  RgbdArgs a = {};
  const int rc = rgbd_prepare(pyramid, intensity, level_intrinsics, F, H, W, levels, pairs, P, T, max_distance,
                              depth_diff, photo_weight, a);
  if (rc != D3F_OK) return rc;
  if (level < 0 || level >= levels || (P > 0 && !sums)) return D3F_EINVAL;
  const size_t pixels = (size_t)level_h(H, level) * (size_t)level_w(W, level);
  for (int p = 0; p < P; ++p) {
    int32_t* idx = index ? index + (size_t)p * pixels : nullptr;
    if (pair_status(a.o, p)) {
      for (int k = 0; k < kSums31; ++k) sums[(size_t)p * kSums31 + k] = 0.0;
      if (idx)
        for (size_t i = 0; i < pixels; ++i) idx[i] = -1;
      continue;
    }
    host_sums(a, p, level, T + 12 * (size_t)p, sums + (size_t)p * kSums31, idx);
  }
  return D3F_OK;
}

int d3f_rgbd_odometry(const float* pyramid, const float* intensity, const float* level_intrinsics, int F, int H, int W,
                      int levels, const int32_t* pairs, int P, const double* T_init, const int32_t* iterations_host,
                      float max_distance, float depth_diff, float photo_weight, double* T, int32_t* count, double* rmse,
                      int32_t* status, int32_t* n_photo, double* information, void* ws, size_t ws_bytes, void* stream) {
  RgbdArgs a = {};
  int rc = rgbd_prepare(pyramid, intensity, level_intrinsics, F, H, W, levels, pairs, P, T_init, max_distance,
                        depth_diff, photo_weight, a);
  if (rc != D3F_OK) return rc;
  if (!iterations_ok(iterations_host, levels) || (P > 0 && (!T || !count || !rmse || !status || !n_photo)))
    return D3F_EINVAL;
  if (P == 0) return D3F_OK;
  if ((rc = odo_workspace(a.o, ws, ws_bytes, kSums31)) != D3F_OK) return rc;
  a.o.T = T;
  a.o.count = count;
  a.o.rmse = rmse;
  a.o.status = status;
  a.o.info = information;
  a.n_photo = n_photo;
  hipStream_t s = (hipStream_t)stream;
  rgbd_setup_kernel<true><<<(unsigned)d3f::cdiv(P, kThreads), kThreads, 0, s>>>(a);
  D3F_LAUNCH_CHECK();
  const bool launched = march(
      H, W, levels, iterations_host,
      [&](int l, int chunks) {
        rgbd_associate_kernel<<<dim3((unsigned)chunks, (unsigned)P), kThreads, 0, s>>>(a, l);
        rgbd_pair_kernel<kFit><<<(unsigned)P, 64, 0, s>>>(a, l, chunks);
      },
      [&](int chunks) {
        rgbd_associate_kernel<<<dim3((unsigned)chunks, (unsigned)P), kThreads, 0, s>>>(a, 0);
        rgbd_pair_kernel<kFinish><<<(unsigned)P, 64, 0, s>>>(a, 0, chunks);
      });
  return launched ? D3F_OK : D3F_ELAUNCH;
}

int d3f_rgbd_odometry_host(const float* pyramid, const float* intensity, const float* level_intrinsics, int F, int H,
                           int W, int levels, const int32_t* pairs, int P, const double* T_init,
                           const int32_t* iterations_host, float max_distance, float depth_diff, float photo_weight,
                           double* T, int32_t* count, double* rmse, int32_t* status, int32_t* n_photo,
                           double* information) {
  RgbdArgs a = {};
  const int rc = rgbd_prepare(pyramid, intensity, level_intrinsics, F, H, W, levels, pairs, P, T_init, max_distance,
                              depth_diff, photo_weight, a);
  if (rc != D3F_OK) return rc;
  if (!iterations_ok(iterations_host, levels) || (P > 0 && (!T || !count || !rmse || !status || !n_photo)))
    return D3F_EINVAL;
  a.o.T = T;
  a.o.count = count;
  a.o.rmse = rmse;
  a.o.status = status;
  a.o.info = information;
  a.n_photo = n_photo;
  for (int p = 0; p < P; ++p) {
    double sums[kSums31] = {}, Tk[12], Tn[12];
    const int st = pair_status(a.o, p);
    if (st) {
      finish_rgbd(a, p, st, false, sums, T_init + 12 * (size_t)p);
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
    finish_rgbd(a, p, 0, last_singular, sums, Tk);
  }
  return D3F_OK;
}

}  // extern "C"
