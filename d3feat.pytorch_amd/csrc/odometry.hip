// Depth and RGB-D odometry on the device: the depth and intensity pyramids and ONE batched frame-to-frame tracker for
// both (include/d3feat_hip.h: d3f_depth_pyramid, d3f_depth_odometry_step, d3f_depth_odometry, d3f_rgbd_pyramid,
// d3f_rgbd_odometry_step, d3f_rgbd_odometry and their host twins; the rules are csrc/odometry.hpp and, on top of it,
// csrc/rgbd_odometry.hpp).  Everything below the pyramids is a template on `bool kPhoto`, whether a pixel has a
// photometric term: the depth tracker is the RGB-D tracker with that term compiled out.  Without it a pair has the 29
// sums of plane.hpp, and neither the arguments nor the kernels know of an intensity; with it there are 31 (n_photo and
// sum r_I^2 follow), and fit() and finish() read the first 29 whatever follows them.
// All P pairs advance together, without host synchronisation and with a launch sequence that depends on the level
// table and the iteration counts alone: one setup launch, then per iteration an association launch and a fit launch,
// coarsest level first, and at the end one more association at level 0 and a finishing launch.
//   pyramid    one launch per level, one thread per output pixel of all frames, the same kernels for the depth and the
//              intensity with the pixel rule as their argument; a tiny launch writes the intrinsics of every level of
//              every frame.
//   associate  grid (chunks of the level, P): the pair is blockIdx.y, so the pair, its images, their intrinsics, T
//              rounded to f32 and the level's dimensions are workgroup-uniform and come through scalar loads.  A
//              workgroup of 256 threads serves kChunk = 1024 consecutive raster pixels of the pair's moving image, a
//              thread the pixels tid, tid + 256, ... of the chunk in that order (coalesced reads of the moving image);
//              the fixed image is gathered at the projected pixel and its four neighbours -- neighbouring moving pixels
//              project to neighbouring fixed pixels, so the gathers of a wave fall into a few cache lines.  Vertices
//              and normals are recomputed from the depth: nothing but the pyramid is read.  kPhoto: after
//              odo::associate has accepted a pixel, the thread reads its own intensity (the address pattern of its
//              depth) and gathers the fixed intensity over the 4 x 4 block around the projection, without the corners
//              (12 values in 4 rows).  photo_weight == 0 is uniform over the launch and skips the gather altogether.
//   fit        one wave per pair adds the pair's chunk sums (lane = chunk mod 64, chunks ascending, then the
//              butterfly) and one lane runs plane::plane_step: icp.hip's scheme.
// Determinism: no floating-point atomic.  A lane adds its pixels in a fixed order, the wave is reduced by common.hpp's
// butterfly, the 4 waves are added in wave order through LDS, and the pair's chunks by one wave in the order above.
// Every order depends on H, W and the level alone, so a pair's sums and its whole trajectory are bit-identical alone,
// inside any batch, and from run to run.  The host twins run the same header text pixel by pixel in raster order and
// make no GPU call.
#include "common.hpp"
#include "rgbd_odometry.hpp"

namespace {

using namespace d3f::odo;
namespace rgbd = d3f::rgbd;

constexpr int kThreads = 256;
constexpr int kChunk = D3F_ODO_CHUNK;          // pixels per workgroup
constexpr int kPerThread = kChunk / kThreads;
static_assert(kChunk % kThreads == 0, "a thread serves whole pixels");
static_assert(kSums == D3F_ODO_SUMS && rgbd::kSums == D3F_RGBD_SUMS, "the header's counts of sums");
static_assert(rgbd::kSums <= kThreads, "a thread per sum in the workgroup's reduction");
static_assert(kMaxLevels == D3F_ODO_MAX_LEVELS, "the header's bound on the levels");

template <bool kPhoto>
constexpr int kSumsOf = kPhoto ? rgbd::kSums : kSums;

// -------------------------------------------------------------------------------------------------------- pyramid
// A pixel rule says what a pixel of level 0 is (of pixel i of all frames) and what one of the next level is (pixel
// (u, v) from the level `src` of width Ws).
template <typename DepthT>
struct DepthRule {
  const DepthT* image;
  float depth_scale, depth_max, depth_diff;
  D3F_HD float level0(size_t i) const { return level0_pixel(image, i, depth_scale, depth_max); }
  D3F_HD float down(const float* src, int Ws, int u, int v) const { return down_pixel(src, Ws, u, v, depth_diff); }
};

enum { kColorRgb8 = D3F_RGBD_COLOR_RGB8, kColorGrey8 = D3F_RGBD_COLOR_GREY8, kColorF32 = D3F_RGBD_COLOR_F32 };

template <int kKind>
struct IntensityRule {
  const void* color;
  D3F_HD float level0(size_t i) const {
    if constexpr (kKind == kColorRgb8) return rgbd::intensity_rgb((const uint8_t*)color + 3 * i);
    else if constexpr (kKind == kColorGrey8) return rgbd::intensity_grey(((const uint8_t*)color)[i]);
    else return ((const float*)color)[i];
  }
  D3F_HD float down(const float* src, int Ws, int u, int v) const { return rgbd::down_pixel(src, Ws, u, v); }
};

template <typename Rule>
__global__ void __launch_bounds__(kThreads) pyramid_level0_kernel(const Rule rule, int64_t frames, int64_t pixels,
                                                                  int64_t frame_pixels, float* __restrict__ pyr) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= frames * pixels) return;
  const int64_t f = i / pixels, local = i - f * pixels;
  pyr[f * frame_pixels + local] = rule.level0((size_t)i);
}

// level l -> l + 1: (Hs, Ws) the source's dimensions at offset src_off of a frame, the result at dst_off
template <typename Rule>
__global__ void __launch_bounds__(kThreads) pyramid_down_kernel(const Rule rule, float* pyr, int64_t frames,
                                                                int64_t frame_pixels, int Hs, int Ws, int64_t src_off,
                                                                int64_t dst_off) {
  const int Hn = Hs >> 1, Wn = Ws >> 1;
  const int64_t pixels = (int64_t)Hn * Wn;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= frames * pixels) return;
  const int64_t f = i / pixels, local = i - f * pixels;
  const int v = (int)(local / Wn), u = (int)(local - (int64_t)v * Wn);
  pyr[f * frame_pixels + dst_off + local] = rule.down(pyr + f * frame_pixels + src_off, Ws, u, v);
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

bool shape_ok(int F, int H, int W, int levels) {
  return F >= 1 && H >= 1 && W >= 1 && levels >= 1 && levels <= kMaxLevels && (H >> (levels - 1)) >= 1 &&
         (W >> (levels - 1)) >= 1 && (int64_t)H * (int64_t)W <= (int64_t)1 << 30;
}

// the packed pyramid of F frames by `rule` on the device, one launch per level
template <typename Rule>
int pyramid_device(const Rule rule, int F, int H, int W, int levels, float* pyr, hipStream_t s) {
  const int64_t pixels = (int64_t)H * W, frame_pixels = level_offset(H, W, levels);
  const int64_t blocks = ((int64_t)F * pixels + kThreads - 1) / kThreads;
  if (blocks > 0x7fffffff) return D3F_EINVAL;
  pyramid_level0_kernel<Rule><<<(unsigned)blocks, kThreads, 0, s>>>(rule, F, pixels, frame_pixels, pyr);
  D3F_LAUNCH_CHECK();
  for (int l = 0; l + 1 < levels; ++l) {
    const int Hs = level_h(H, l), Ws = level_w(W, l);
    const int64_t n = (int64_t)F * (Hs >> 1) * (Ws >> 1);
    pyramid_down_kernel<Rule><<<(unsigned)((n + kThreads - 1) / kThreads), kThreads, 0, s>>>(
        rule, pyr, F, frame_pixels, Hs, Ws, level_offset(H, W, l), level_offset(H, W, l + 1));
    D3F_LAUNCH_CHECK();
  }
  return D3F_OK;
}

// the same on the host, pixel by pixel
template <typename Rule>
int pyramid_host(const Rule rule, int F, int H, int W, int levels, float* pyr) {
  const int64_t pixels = (int64_t)H * W, frame_pixels = level_offset(H, W, levels);
  for (int f = 0; f < F; ++f) {
    float* frame = pyr + (size_t)f * (size_t)frame_pixels;
    for (int64_t i = 0; i < pixels; ++i) frame[i] = rule.level0((size_t)f * (size_t)pixels + (size_t)i);
    for (int l = 0; l + 1 < levels; ++l) {
      const int Hs = level_h(H, l), Ws = level_w(W, l), Hn = Hs >> 1, Wn = Ws >> 1;
      const float* src = frame + level_offset(H, W, l);
      float* dst = frame + level_offset(H, W, l + 1);
      for (int v = 0; v < Hn; ++v)
        for (int u = 0; u < Wn; ++u) dst[(size_t)v * (size_t)Wn + (size_t)u] = rule.down(src, Ws, u, v);
    }
  }
  return D3F_OK;
}

// build(rule) with the rule of the depth frames / of the colour frames
template <typename Build>
int with_depth_rule(const void* depth, int depth_is_f32, float depth_scale, float depth_max, float depth_diff,
                    Build build) {
  if (depth_is_f32) return build(DepthRule<float>{(const float*)depth, depth_scale, depth_max, depth_diff});
  return build(DepthRule<uint16_t>{(const uint16_t*)depth, depth_scale, depth_max, depth_diff});
}

template <typename Build>
int with_intensity_rule(const void* color, int kind, Build build) {
  if (kind == kColorRgb8) return build(IntensityRule<kColorRgb8>{color});
  if (kind == kColorGrey8) return build(IntensityRule<kColorGrey8>{color});
  return build(IntensityRule<kColorF32>{color});
}

bool pyramid_ok(const void* depth, int F, int H, int W, const float* K, int levels, float depth_scale, float depth_max,
                float depth_diff, const float* pyr, const float* KL) {
  return depth && K && pyr && KL && shape_ok(F, H, W, levels) && depth_scale > 0.0f && depth_max > 0.0f &&
         depth_diff >= 0.0f;
}

bool color_ok(const void* color, int kind, int F, int H, int W, int levels, const float* inten) {
  return color && inten && shape_ok(F, H, W, levels) && kind >= kColorRgb8 && kind <= kColorF32;
}

// ------------------------------------------------------------------------------------------------------ arguments
struct OdoArgs {
  const float* pyr;         // [F, frame_pixels]
  const float* KL;          // [F, levels, 4]
  const int32_t* pairs;     // [P, 2]
  const double* T_init;     // [P, 12]
  double* T_cur;            // [P, 12] ws
  int32_t* done;            // [P] ws: the pair is not iterated (PAIR / NONFINITE)
  int32_t* sing;            // [P] ws: the last fit at level 0 was singular
  double* partial;          // [P * chunks of level 0, sums per pair] ws
  int32_t* index;           // [P, pixels of the level] or null (the step entry point)
  double* sums;             // [P, sums per pair] (the step entry point)
  double* T;                // [P, 16]
  int32_t* count;
  double* rmse;
  int32_t* status;
  double* info;             // [P, 36] or null
  int64_t frame_pixels;
  int F, H, W, levels, P;
  float depth_diff, max_d2;
};

template <bool kPhoto>
struct Args : OdoArgs {};

template <>
struct Args<true> : OdoArgs {
  const float* inten;       // [F, frame_pixels]
  int32_t* n_photo;         // [P] (the odometry entry point)
  float photo_weight;
};

// the intensity images of one level of one pair, and the weight of the term
struct Intensity {
  const float* IA;
  const float* IB;
  float photo_weight;
};

D3F_HD inline int chunks_of(int H, int W, int l) {
  return (int)(((int64_t)level_h(H, l) * (int64_t)level_w(W, l) + kChunk - 1) / kChunk);
}

// level l of the valid pair (a, b) under T [12]
D3F_HD inline void make_level(const OdoArgs& A, int a, int b, int l, const double* T, PairLevel& L) {
  const int64_t off = level_offset(A.H, A.W, l);
  L.A = A.pyr + (size_t)a * (size_t)A.frame_pixels + (size_t)off;
  L.B = A.pyr + (size_t)b * (size_t)A.frame_pixels + (size_t)off;
  L.Ka = A.KL + ((size_t)a * (size_t)A.levels + (size_t)l) * 4;
  L.Kb = A.KL + ((size_t)b * (size_t)A.levels + (size_t)l) * 4;
  L.H = level_h(A.H, l);
  L.W = level_w(A.W, l);
  for (int k = 0; k < 12; ++k) L.M[k] = (float)T[k];
  L.depth_diff = A.depth_diff;
  L.max_d2 = A.max_d2;
}

template <bool kPhoto>
D3F_HD inline Intensity make_intensity(const Args<kPhoto>& A, int a, int b, int l) {
  Intensity I = {};
  if constexpr (kPhoto) {
    const size_t off = (size_t)level_offset(A.H, A.W, l);
    I.IA = A.inten + (size_t)a * (size_t)A.frame_pixels + off;
    I.IB = A.inten + (size_t)b * (size_t)A.frame_pixels + off;
    I.photo_weight = A.photo_weight;
  }
  return I;
}

D3F_HD inline int pair_status(const OdoArgs& A, int p) {
  const int a = A.pairs[2 * p], b = A.pairs[2 * p + 1];
  int st = 0;
  if (!((unsigned)a < (unsigned)A.F && (unsigned)b < (unsigned)A.F)) st |= D3F_ODO_ST_PAIR;
  bool finite = true;
  for (int k = 0; k < 12; ++k) {
    const double v = A.T_init[12 * (size_t)p + k];
    finite = finite && (v - v == 0.0);   // false for a NaN and for an infinity
  }
  if (!finite) st |= D3F_ODO_ST_NONFINITE;
  return st;
}

D3F_HD inline void write_pose(double* o, const double* rt) {
  for (int k = 0; k < 12; ++k) o[k] = rt[k];
  o[12] = 0.0; o[13] = 0.0; o[14] = 0.0; o[15] = 1.0;
}

// what the finishing step writes for pair p from the sums of the last association (st: the setup's flags)
template <bool kPhoto>
D3F_HD inline void finish(const Args<kPhoto>& A, int p, int st, bool singular, const double* sums, const double* T) {
  const bool few = sums[0] < (double)kMinPixels;
  if (!st) st = few ? D3F_ODO_ST_FEW : (singular ? D3F_ODO_ST_SINGULAR : 0);
  A.status[p] = st;
  write_pose(A.T + 16 * (size_t)p, st ? A.T_init + 12 * (size_t)p : T);
  A.count[p] = st ? 0 : (int)sums[0];
  A.rmse[p] = st ? 0.0 : sqrt(sums[kSums - 1] / sums[0]);
  if (A.info) {
    double out[36];
    information(sums, out);
    for (int k = 0; k < 36; ++k) A.info[36 * (size_t)p + k] = st ? 0.0 : out[k];
  }
  if constexpr (kPhoto) A.n_photo[p] = A.status[p] ? 0 : (int)sums[rgbd::kPhotoCount];
}

// one accepted-or-not moving pixel (u, v) of the level L: its sums into acc, its index returned
template <bool kPhoto>
D3F_HD inline int add_moving_pixel(const PairLevel& L, const Intensity& I, int u, int v, double* acc) {
  float av[3], yv[3], nv[3];
  const int t = associate(L, u, v, av, yv, nv);
  if (t >= 0) {
    add_pixel(acc, av, yv, nv);
    if constexpr (kPhoto) {
      if (I.photo_weight != 0.0f) {   // (uniform over a launch)
        float r, q[3];
        if (rgbd::photometric(I.IB, L.H, L.W, L.Kb, I.IA[(size_t)v * (size_t)L.W + (size_t)u], av, &r, q))
          rgbd::add_photometric(acc, av, q, r, (double)I.photo_weight);
      }
    }
  }
  return t;
}

// -------------------------------------------------------------------------------------------------------- kernels
// kRun: the whole odometry (the outputs of a stopped pair are written here); else the step entry point
template <bool kPhoto, bool kRun>
__global__ void __launch_bounds__(kThreads) odo_setup_kernel(const Args<kPhoto> A) {
  const int p = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (p >= A.P) return;
  const int st = pair_status(A, p);
  for (int k = 0; k < 12; ++k) A.T_cur[12 * (size_t)p + k] = A.T_init[12 * (size_t)p + k];
  A.done[p] = st != 0;
  A.sing[p] = 0;
  if constexpr (kRun) {
    if (st) {
      const double zero[kSumsOf<kPhoto>] = {};
      finish(A, p, st, false, zero, A.T_init + 12 * (size_t)p);
    }
  }
}

// grid (chunks of the level, P)
template <bool kPhoto>
__global__ void __launch_bounds__(kThreads) odo_associate_kernel(const Args<kPhoto> A, int level) {
  constexpr int kN = kSumsOf<kPhoto>;
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
  const Intensity I = make_intensity(A, a, b, level);

  double acc[kN];
#pragma unroll
  for (int k = 0; k < kN; ++k) acc[k] = 0.0;
  for (int k = 0; k < kPerThread; ++k) {
    const int i = first + k * kThreads + (int)threadIdx.x;
    if (i >= pixels) break;
    const int v = i / Wl, u = i - v * Wl;
    int t;
    if constexpr (kPhoto) {
      t = add_moving_pixel<true>(L, I, u, v, acc);
    } else {   // add_moving_pixel<false> written out: through the call the compiler orders this instantiation otherwise,
               // and an iteration at 640 x 480 was measured 1.3 % slower (profiles/odometry_refactor_identity.txt)
      float av[3], yv[3], nv[3];
      t = associate(L, u, v, av, yv, nv);
      if (t >= 0) add_pixel(acc, av, yv, nv);
    }
    if (A.index) A.index[(size_t)p * (size_t)pixels + (size_t)i] = t;
  }
  d3f::wave_sum_f64(acc);
  __shared__ double red[kThreads / 64][kN];
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kN; ++k) red[wave][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < kN) {
    double s = red[0][threadIdx.x];
    for (int w = 1; w < kThreads / 64; ++w) s += red[w][threadIdx.x];
    A.partial[((size_t)p * (size_t)gridDim.x + (size_t)chunk) * kN + threadIdx.x] = s;
  }
}

enum { kFit = 0, kFinish = 1, kWriteSums = 2 };

// pair p's chunk sums ([.., kN] in `partial`) in the fixed order: lane = chunk mod 64, chunks ascending, then the
// butterfly.  One wave.
template <int kN>
__device__ __forceinline__ void pair_sums(const double* partial, int p, int chunks, int lane, double (&v)[kN]) {
#pragma unroll
  for (int k = 0; k < kN; ++k) v[k] = 0.0;
  for (int j = lane; j < chunks; j += 64) {
    const double* part = partial + ((size_t)p * (size_t)chunks + (size_t)j) * kN;
#pragma unroll
    for (int k = 0; k < kN; ++k) v[k] += part[k];
  }
  d3f::wave_sum_f64(v);
}

// one wave per pair: the pair's sums, then the fit / the final outputs / the sums as they are
template <bool kPhoto, int kWhat>
__global__ void __launch_bounds__(64) odo_pair_kernel(const Args<kPhoto> A, int level, int chunks) {
  constexpr int kN = kSumsOf<kPhoto>;
  const int p = (int)blockIdx.x, lane = (int)threadIdx.x;
  const bool done = A.done[p] != 0;   // (uniform over the wave)
  if (done && kWhat != kWriteSums) return;
  double v[kN] = {};
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
    finish(A, p, 0, A.sing[p] != 0, v, T);
  } else {
#pragma unroll
    for (int k = 0; k < kN; ++k) A.sums[(size_t)p * kN + k] = v[k];
  }
}

// ------------------------------------------------------------------------------------------------------ host side
// the sums of one association of the valid pair p on the host: raster order
template <bool kPhoto>
void host_sums(const Args<kPhoto>& A, int p, int level, const double* T, double* sums, int32_t* index) {
  PairLevel L;
  const int a = A.pairs[2 * p], b = A.pairs[2 * p + 1];
  make_level(A, a, b, level, T, L);
  const Intensity I = make_intensity(A, a, b, level);
  for (int k = 0; k < kSumsOf<kPhoto>; ++k) sums[k] = 0.0;
  for (int v = 0; v < L.H; ++v)
    for (int u = 0; u < L.W; ++u) {
      const int t = add_moving_pixel<kPhoto>(L, I, u, v, sums);
      if (index) index[(size_t)v * (size_t)L.W + (size_t)u] = t;
    }
}

struct OdoLayout {
  double* T_cur;
  int32_t* done;
  int32_t* sing;
  double* partial;
  size_t bytes;
};

OdoLayout odo_layout(void* ws, int P, int H, int W, int sums) {
  OdoLayout l;
  const size_t n = (size_t)(P > 0 ? P : 1);
  d3f::Carver c(ws);
  l.T_cur = c.take<double>(12 * n);
  l.done = c.take<int32_t>(n);
  l.sing = c.take<int32_t>(n);
  l.partial = c.take<double>(n * (size_t)chunks_of(H, W, 0) * (size_t)sums);
  l.bytes = d3f::align_up(c.off, 256);
  return l;
}

template <bool kPhoto>
size_t ws_bytes_of(int P, int H, int W) {
  if (P < 0 || H < 1 || W < 1 || (int64_t)H * (int64_t)W > (int64_t)1 << 30) return 0;
  return odo_layout(nullptr, P, H, W, kSumsOf<kPhoto>).bytes;
}

template <bool kPhoto>
int odo_workspace(Args<kPhoto>& a, void* ws, size_t ws_bytes) {
  if (!ws) return D3F_EINVAL;
  if (ws_bytes < odo_layout(nullptr, a.P, a.H, a.W, kSumsOf<kPhoto>).bytes) return D3F_EWORKSPACE;
  const OdoLayout l = odo_layout(ws, a.P, a.H, a.W, kSumsOf<kPhoto>);
  a.T_cur = l.T_cur;
  a.done = l.done;
  a.sing = l.sing;
  a.partial = l.partial;
  return D3F_OK;
}

// What the entry points are given to track by: the pyramids (`inten` and `photo_weight` count with kPhoto alone), the
// pairs and their poses, the thresholds.
struct Tracked {
  const float* pyr;
  const float* inten;
  const float* KL;
  int F, H, W, levels;
  const int32_t* pairs;
  int P;
  const double* T;
  float max_distance, depth_diff, photo_weight;
};

// the checks and the common part of the arguments; D3F_OK with P == 0 means there is nothing to do
template <bool kPhoto>
int odo_prepare(const Tracked& in, Args<kPhoto>& a) {
  if constexpr (kPhoto) {
    if (!in.inten || !(in.photo_weight >= 0.0f && rgbd::finite(in.photo_weight))) return D3F_EINVAL;
    a.inten = in.inten;
    a.photo_weight = in.photo_weight;
  }
  if (!in.pyr || !in.KL || !shape_ok(in.F, in.H, in.W, in.levels) || in.P < 0 || in.P > 65535 ||
      !(in.max_distance > 0.0f) || !(in.depth_diff >= 0.0f) || (in.P > 0 && (!in.pairs || !in.T)))
    return D3F_EINVAL;
  a.pyr = in.pyr;
  a.KL = in.KL;
  a.pairs = in.pairs;
  a.T_init = in.T;
  a.frame_pixels = level_offset(in.H, in.W, in.levels);
  a.F = in.F;
  a.H = in.H;
  a.W = in.W;
  a.levels = in.levels;
  a.P = in.P;
  a.depth_diff = in.depth_diff;
  a.max_d2 = in.max_distance * in.max_distance;
  return D3F_OK;
}

// ONE association at `level`, on the host or on the device
template <bool kPhoto>
int odo_step(const Tracked& in, int level, double* sums, int32_t* index, bool host, void* ws, size_t ws_bytes,
             void* stream) {
  constexpr int kN = kSumsOf<kPhoto>;
  Args<kPhoto> a = {};
  int rc = odo_prepare(in, a);
  if (rc != D3F_OK) return rc;
  const int P = in.P;
  if (level < 0 || level >= in.levels || (P > 0 && !sums)) return D3F_EINVAL;
  if (host) {
    const size_t pixels = (size_t)level_h(in.H, level) * (size_t)level_w(in.W, level);
    for (int p = 0; p < P; ++p) {
      int32_t* idx = index ? index + (size_t)p * pixels : nullptr;
      if (pair_status(a, p)) {
        for (int k = 0; k < kN; ++k) sums[(size_t)p * kN + k] = 0.0;
        if (idx)
          for (size_t i = 0; i < pixels; ++i) idx[i] = -1;
        continue;
      }
      host_sums(a, p, level, in.T + 12 * (size_t)p, sums + (size_t)p * kN, idx);
    }
    return D3F_OK;
  }
  if (P == 0) return D3F_OK;
  if ((rc = odo_workspace(a, ws, ws_bytes)) != D3F_OK) return rc;
  a.sums = sums;
  a.index = index;
  hipStream_t s = (hipStream_t)stream;
  const int chunks = chunks_of(in.H, in.W, level);
  odo_setup_kernel<kPhoto, false><<<(unsigned)d3f::cdiv(P, kThreads), kThreads, 0, s>>>(a);
  D3F_LAUNCH_CHECK();
  odo_associate_kernel<kPhoto><<<dim3((unsigned)chunks, (unsigned)P), kThreads, 0, s>>>(a, level);
  odo_pair_kernel<kPhoto, kWriteSums><<<(unsigned)P, 64, 0, s>>>(a, level, chunks);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

struct Outputs {
  double* T;
  int32_t* count;
  double* rmse;
  int32_t* status;
  int32_t* n_photo;   // (kPhoto alone)
  double* information;
};

// The whole odometry.  The coarse-to-fine schedule is iterations[l] fits at level l, coarsest level first, then one
// more association at level 0 and the finishing step: it depends on the level table and the counts alone.
template <bool kPhoto>
int odo_run(const Tracked& in, const int32_t* iterations, const Outputs& out, bool host, void* ws, size_t ws_bytes,
            void* stream) {
  Args<kPhoto> a = {};
  int rc = odo_prepare(in, a);
  if (rc != D3F_OK) return rc;
  const int P = in.P, levels = in.levels;
  bool counts_ok = iterations != nullptr;
  for (int l = 0; counts_ok && l < levels; ++l) counts_ok = iterations[l] >= 0 && iterations[l] <= D3F_ODO_MAX_ITERS;
  if (!counts_ok || (P > 0 && (!out.T || !out.count || !out.rmse || !out.status || (kPhoto && !out.n_photo))))
    return D3F_EINVAL;
  a.T = out.T;
  a.count = out.count;
  a.rmse = out.rmse;
  a.status = out.status;
  a.info = out.information;
  if constexpr (kPhoto) a.n_photo = out.n_photo;
  if (host) {
    for (int p = 0; p < P; ++p) {
      double sums[kSumsOf<kPhoto>] = {}, Tk[12], Tn[12];
      const int st = pair_status(a, p);
      if (st) {
        finish(a, p, st, false, sums, in.T + 12 * (size_t)p);
        continue;
      }
      for (int k = 0; k < 12; ++k) Tk[k] = in.T[12 * (size_t)p + k];
      bool last_singular = false;
      for (int l = levels - 1; l >= 0; --l)
        for (int it = 0; it < iterations[l]; ++it) {
          host_sums(a, p, l, Tk, sums, nullptr);
          bool singular;
          if (fit(sums, Tk, Tn, &singular))
            for (int k = 0; k < 12; ++k) Tk[k] = Tn[k];
          if (l == 0) last_singular = singular;
        }
      host_sums(a, p, 0, Tk, sums, nullptr);
      finish(a, p, 0, last_singular, sums, Tk);
    }
    return D3F_OK;
  }
  if (P == 0) return D3F_OK;
  if ((rc = odo_workspace(a, ws, ws_bytes)) != D3F_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  odo_setup_kernel<kPhoto, true><<<(unsigned)d3f::cdiv(P, kThreads), kThreads, 0, s>>>(a);
  D3F_LAUNCH_CHECK();
  for (int l = levels - 1; l >= 0; --l) {
    const int chunks = chunks_of(in.H, in.W, l);
    for (int k = 0; k < iterations[l]; ++k) {
      odo_associate_kernel<kPhoto><<<dim3((unsigned)chunks, (unsigned)P), kThreads, 0, s>>>(a, l);
      odo_pair_kernel<kPhoto, kFit><<<(unsigned)P, 64, 0, s>>>(a, l, chunks);
    }
    if (hipGetLastError() != hipSuccess) return D3F_ELAUNCH;
  }
  const int chunks = chunks_of(in.H, in.W, 0);
  odo_associate_kernel<kPhoto><<<dim3((unsigned)chunks, (unsigned)P), kThreads, 0, s>>>(a, 0);
  odo_pair_kernel<kPhoto, kFinish><<<(unsigned)P, 64, 0, s>>>(a, 0, chunks);
  return hipGetLastError() == hipSuccess ? D3F_OK : D3F_ELAUNCH;
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
  hipStream_t s = (hipStream_t)stream;
  const int rc = with_depth_rule(depth, depth_is_f32, depth_scale, depth_max, depth_diff,
                                 [&](auto rule) { return pyramid_device(rule, F, H, W, levels, pyramid, s); });
  if (rc != D3F_OK) return rc;
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
  for (int f = 0; f < F; ++f)
    frame_intrinsics(intrinsics + 4 * (size_t)f, levels, level_intrinsics + 4 * (size_t)f * (size_t)levels);
  return with_depth_rule(depth, depth_is_f32, depth_scale, depth_max, depth_diff,
                         [&](auto rule) { return pyramid_host(rule, F, H, W, levels, pyramid); });
}

int d3f_rgbd_pyramid(const void* color, int color_kind, int F, int H, int W, int levels, float* intensity,
                     void* stream) {
  if (!color_ok(color, color_kind, F, H, W, levels, intensity)) return D3F_EINVAL;
  return with_intensity_rule(color, color_kind, [&](auto rule) {
    return pyramid_device(rule, F, H, W, levels, intensity, (hipStream_t)stream);
  });
}

int d3f_rgbd_pyramid_host(const void* color, int color_kind, int F, int H, int W, int levels, float* intensity) {
  if (!color_ok(color, color_kind, F, H, W, levels, intensity)) return D3F_EINVAL;
  return with_intensity_rule(color, color_kind,
                             [&](auto rule) { return pyramid_host(rule, F, H, W, levels, intensity); });
}

size_t d3f_depth_odometry_ws_bytes(int P, int H, int W) { return ws_bytes_of<false>(P, H, W); }

size_t d3f_rgbd_odometry_ws_bytes(int P, int H, int W) { return ws_bytes_of<true>(P, H, W); }

int d3f_depth_odometry_step(const float* pyramid, const float* level_intrinsics, int F, int H, int W, int levels,
                            const int32_t* pairs, int P, const double* T, int level, float max_distance,
                            float depth_diff, double* sums, int32_t* index, void* ws, size_t ws_bytes, void* stream) {
  return odo_step<false>({pyramid, nullptr, level_intrinsics, F, H, W, levels, pairs, P, T, max_distance, depth_diff,
                          0.0f}, level, sums, index, false, ws, ws_bytes, stream);
}

int d3f_depth_odometry_step_host(const float* pyramid, const float* level_intrinsics, int F, int H, int W, int levels,
                                 const int32_t* pairs, int P, const double* T, int level, float max_distance,
                                 float depth_diff, double* sums, int32_t* index) {
  return odo_step<false>({pyramid, nullptr, level_intrinsics, F, H, W, levels, pairs, P, T, max_distance, depth_diff,
                          0.0f}, level, sums, index, true, nullptr, 0, nullptr);
}

int d3f_depth_odometry(const float* pyramid, const float* level_intrinsics, int F, int H, int W, int levels,
                       const int32_t* pairs, int P, const double* T_init, const int32_t* iterations_host,
                       float max_distance, float depth_diff, double* T, int32_t* count, double* rmse, int32_t* status,
                       double* information, void* ws, size_t ws_bytes, void* stream) {
  return odo_run<false>({pyramid, nullptr, level_intrinsics, F, H, W, levels, pairs, P, T_init, max_distance,
                         depth_diff, 0.0f}, iterations_host, {T, count, rmse, status, nullptr, information}, false,
                        ws, ws_bytes, stream);
}

int d3f_depth_odometry_host(const float* pyramid, const float* level_intrinsics, int F, int H, int W, int levels,
                            const int32_t* pairs, int P, const double* T_init, const int32_t* iterations_host,
                            float max_distance, float depth_diff, double* T, int32_t* count, double* rmse,
                            int32_t* status, double* information) {
  return odo_run<false>({pyramid, nullptr, level_intrinsics, F, H, W, levels, pairs, P, T_init, max_distance,
                         depth_diff, 0.0f}, iterations_host, {T, count, rmse, status, nullptr, information}, true,
                        nullptr, 0, nullptr);
}

int d3f_rgbd_odometry_step(const float* pyramid, const float* intensity, const float* level_intrinsics, int F, int H,
                           int W, int levels, const int32_t* pairs, int P, const double* T, int level,
                           float max_distance, float depth_diff, float photo_weight, double* sums, int32_t* index,
                           void* ws, size_t ws_bytes, void* stream) {
  return odo_step<true>({pyramid, intensity, level_intrinsics, F, H, W, levels, pairs, P, T, max_distance, depth_diff,
                         photo_weight}, level, sums, index, false, ws, ws_bytes, stream);
}

int d3f_rgbd_odometry_step_host(const float* pyramid, const float* intensity, const float* level_intrinsics, int F,
                                int H, int W, int levels, const int32_t* pairs, int P, const double* T, int level,
                                float max_distance, float depth_diff, float photo_weight, double* sums,
                                int32_t* index) {
  return odo_step<true>({pyramid, intensity, level_intrinsics, F, H, W, levels, pairs, P, T, max_distance, depth_diff,
                         photo_weight}, level, sums, index, true, nullptr, 0, nullptr);
}

int d3f_rgbd_odometry(const float* pyramid, const float* intensity, const float* level_intrinsics, int F, int H, int W,
                      int levels, const int32_t* pairs, int P, const double* T_init, const int32_t* iterations_host,
                      float max_distance, float depth_diff, float photo_weight, double* T, int32_t* count, double* rmse,
                      int32_t* status, int32_t* n_photo, double* information, void* ws, size_t ws_bytes, void* stream) {
  return odo_run<true>({pyramid, intensity, level_intrinsics, F, H, W, levels, pairs, P, T_init, max_distance,
                        depth_diff, photo_weight}, iterations_host, {T, count, rmse, status, n_photo, information},
                       false, ws, ws_bytes, stream);
}

int d3f_rgbd_odometry_host(const float* pyramid, const float* intensity, const float* level_intrinsics, int F, int H,
                           int W, int levels, const int32_t* pairs, int P, const double* T_init,
                           const int32_t* iterations_host, float max_distance, float depth_diff, float photo_weight,
                           double* T, int32_t* count, double* rmse, int32_t* status, int32_t* n_photo,
                           double* information) {
  return odo_run<true>({pyramid, intensity, level_intrinsics, F, H, W, levels, pairs, P, T_init, max_distance,
                        depth_diff, photo_weight}, iterations_host, {T, count, rmse, status, n_photo, information},
                       true, nullptr, 0, nullptr);
}

}  // extern "C"
