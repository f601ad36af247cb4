// The batched marching of the pair trackers, shared by odometry.hip (depth only) and rgbd_odometry.hip (depth and
// intensity): the arguments of a batch of pairs, the per-pair set-up and finishing rules, the workspace layout, the
// fixed-order reduction of a pair's chunk sums and the coarse-to-fine launch schedule.  The association kernels
// themselves stay in the two sources: they differ in what a pixel adds.  Both keep the same determinism scheme: a
// workgroup of kThreads serves kChunk consecutive raster pixels of one pair, a wave adds the pair's chunks in the order
// lane = chunk mod 64, chunks ascending, then the butterfly.  The first 29 sums of a pair are always plane.hpp's, so
// fit() and finish_pair() read them whatever follows them.
#pragma once
#include "common.hpp"
#include "odometry.hpp"

namespace d3f {
namespace odo {

constexpr int kThreads = 256;
constexpr int kChunk = D3F_ODO_CHUNK;          // pixels per workgroup
constexpr int kPerThread = kChunk / kThreads;
static_assert(kChunk % kThreads == 0, "a thread serves whole pixels");
static_assert(kSums == D3F_ODO_SUMS, "the header's count of sums");
static_assert(kMaxLevels == D3F_ODO_MAX_LEVELS, "the header's bound on the levels");

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
D3F_HD inline void finish_pair(const OdoArgs& A, int p, int st, bool singular, const double* sums, const double* T) {
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
}

#if defined(__HIPCC__)
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
#endif

// ------------------------------------------------------------------------------------------------------ host side
struct OdoLayout {
  double* T_cur;
  int32_t* done;
  int32_t* sing;
  double* partial;
  size_t bytes;
};

inline OdoLayout odo_layout(void* ws, int P, int H, int W, int sums = kSums) {
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

inline bool shape_ok(int F, int H, int W, int levels) {
  return F >= 1 && H >= 1 && W >= 1 && levels >= 1 && levels <= kMaxLevels && (H >> (levels - 1)) >= 1 &&
         (W >> (levels - 1)) >= 1 && (int64_t)H * (int64_t)W <= (int64_t)1 << 30;
}

// the checks and the common part of OdoArgs; D3F_OK with P == 0 means there is nothing to do
inline int odo_prepare(const float* pyr, const float* KL, int F, int H, int W, int levels, const int32_t* pairs, int P,
                       const double* T, float max_distance, float depth_diff, OdoArgs& a) {
  if (!pyr || !KL || !shape_ok(F, H, W, levels) || P < 0 || P > 65535 || !(max_distance > 0.0f) ||
      !(depth_diff >= 0.0f) || (P > 0 && (!pairs || !T)))
    return D3F_EINVAL;
  a.pyr = pyr;
  a.KL = KL;
  a.pairs = pairs;
  a.T_init = T;
  a.frame_pixels = level_offset(H, W, levels);
  a.F = F;
  a.H = H;
  a.W = W;
  a.levels = levels;
  a.P = P;
  a.depth_diff = depth_diff;
  a.max_d2 = max_distance * max_distance;
  return D3F_OK;
}

inline int odo_workspace(OdoArgs& a, void* ws, size_t ws_bytes, int sums = kSums) {
  if (!ws) return D3F_EINVAL;
  if (ws_bytes < odo_layout(nullptr, a.P, a.H, a.W, sums).bytes) return D3F_EWORKSPACE;
  const OdoLayout l = odo_layout(ws, a.P, a.H, a.W, sums);
  a.T_cur = l.T_cur;
  a.done = l.done;
  a.sing = l.sing;
  a.partial = l.partial;
  return D3F_OK;
}

inline bool iterations_ok(const int32_t* iterations, int levels) {
  if (!iterations) return false;
  for (int l = 0; l < levels; ++l)
    if (iterations[l] < 0 || iterations[l] > D3F_ODO_MAX_ITERS) return false;
  return true;
}

// The coarse-to-fine schedule: iterations_host[l] times iterate(l, chunks of l), coarsest level first, then
// last(chunks of level 0) once.  It depends on the level table and the counts alone.  false: a launch failed.
template <typename Iterate, typename Last>
inline bool march(int H, int W, int levels, const int32_t* iterations_host, Iterate iterate, Last last) {
  for (int l = levels - 1; l >= 0; --l) {
    const int chunks = chunks_of(H, W, l);
    for (int k = 0; k < iterations_host[l]; ++k) iterate(l, chunks);
    if (hipGetLastError() != hipSuccess) return false;
  }
  last(chunks_of(H, W, 0));
  return hipGetLastError() == hipSuccess;
}

}  // namespace odo
}  // namespace d3f
