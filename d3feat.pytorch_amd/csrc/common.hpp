// Shared device helpers for libd3feat_hip.so (gfx950 only; wave = 64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "d3feat_hip.h"

#define D3F_WAVE 64
#define D3F_MAX_BATCH 64  // clouds per stacked batch the kernels index by linear scan

#define D3F_LAUNCH_CHECK()                          \
  do {                                              \
    if (hipGetLastError() != hipSuccess) return D3F_ELAUNCH; \
  } while (0)

namespace d3f {

// Zero-fill as an ordinary kernel launch.  hipMemsetAsync nodes were observed NOT to re-execute under hipGraph replay
// of this library's launches (second replay saw dirty allocators), so every re-initialisation is a kernel.
__global__ static void zero_fill_kernel(uint32_t* __restrict__ p, size_t n_words) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += (size_t)gridDim.x * blockDim.x) p[i] = 0u;
}
static inline hipError_t zero_async(void* p, size_t bytes, hipStream_t stream) {
  const size_t words = (bytes + 3) / 4;  // all buffers of this library are 4-byte multiples
  if (words == 0) return hipSuccess;
  size_t blocks = (words + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  zero_fill_kernel<<<(unsigned)blocks, 256, 0, stream>>>((uint32_t*)p, words);
  return hipGetLastError();
}

// the library's tunables (misc.hip; d3f_set_tunables): plain loads of a process-wide struct, no environment reads
const d3f_tunables& tunables();

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// Carves aligned sub-buffers out of one caller-provided workspace.
struct Carver {
  char* base;
  size_t off;
  explicit Carver(void* p) : base((char*)p), off(0) {}
  template <typename T>
  T* take(size_t n) {
    off = align_up(off, 256);
    T* r = (T*)(base + off);
    off += n * sizeof(T);
    return r;
  }
};

// (batch element, first row of that element) of stacked row `i`, given per-element lengths.
__device__ __forceinline__ void locate_batch(const int32_t* __restrict__ len, int B, int i, int& b, int& start) {
  int s = 0, k = 0;
  for (; k < B - 1; ++k) {
    const int l = len[k];
    if (i < s + l) break;
    s += l;
  }
  b = k;
  start = s;
}

__device__ __forceinline__ int batch_offset(const int32_t* __restrict__ len, int b) {
  int s = 0;
  for (int k = 0; k < b; ++k) s += len[k];
  return s;
}

// Rows of a stacked batch partitioned into groups of `group` consecutive clouds (e.g. the 2 fragments of a pair when 8
// pairs are stacked for inference): per-group scalars (feature maximum, table width) are indexed by group_of_row.
// len == nullptr: one group.
struct RowGroups {
  const int32_t* len;
  int B;
  int group;
};
__device__ __forceinline__ int group_of_row(const RowGroups& rg, int row) {
  if (!rg.len || rg.group <= 0) return 0;
  int b, st;
  locate_batch(rg.len, rg.B, row, b, st);
  return b / rg.group;
}

// The 2M sampled rows of a training step (loss.hip: select + normalise; detection.hip: the detector on those rows):
// m2 in [0, M) are the anchors, [M, 2M) the positives.  idx_a / idx_p int64, element m at idx[m * idx_stride]; idx_p is
// offset by *p_offset when given.  pair_len (stacked pairs): the rows of pair m / M_pair are local to its own two clouds
// (2p, 2p + 1 of the stack).
struct SampledRows {
  const int64_t* idx_a;
  const int64_t* idx_p;
  int idx_stride;
  int M;
  const int32_t* p_offset;
  const int32_t* pair_len;
  int M_pair;
};
__device__ __forceinline__ long sampled_row(const SampledRows& sr, int m2, int N) {
  const bool pos = m2 >= sr.M;
  const int m = pos ? m2 - sr.M : m2;
  long row = pos ? sr.idx_p[(size_t)m * sr.idx_stride] + (sr.p_offset ? (long)*sr.p_offset : 0)
                 : sr.idx_a[(size_t)m * sr.idx_stride];
  if (sr.pair_len) row += batch_offset(sr.pair_len, 2 * (m / sr.M_pair) + (pos ? 1 : 0));
  return row < 0 ? 0 : (row >= N ? N - 1 : row);
}
// The SampledRows of an entry point's (idx_a, idx_p, idx_stride, M, pairs, p_offset, pair_len), M per pair; false is
// D3F_EINVAL.  pair_len NULL: the global rows of ONE pair, p_offset optional.  pair_len [2 pairs]: cloud-local rows.
static inline bool make_sampled_rows(const int64_t* idx_a, const int64_t* idx_p, int idx_stride, int M, int pairs,
                                     const int32_t* p_offset, const int32_t* pair_len, SampledRows& sr) {
  if (!idx_a || !idx_p || idx_stride < 1 || M < 1 || pairs < 1 || 2 * pairs > D3F_MAX_BATCH) return false;
  if (pair_len ? p_offset != nullptr : pairs != 1) return false;
  if ((long long)pairs * M > (1 << 24)) return false;   // 2 * rows is a grid size, and the detector's partial count
  sr = {idx_a, idx_p, idx_stride, pairs * M, p_offset, pair_len, M};
  return true;
}

// squared distance with the reference's float32 evaluation order and NO fused multiply-add:
// d2 = dx*dx; d2 += dy*dy; d2 += dz*dz   (nanoflann.hpp:433-441).  NOTE: on AMD the __f*_rn intrinsics are plain
// operators, so this is only exact because the library is compiled with -ffp-contract=off (see _native.build).
__device__ __forceinline__ float sqdist_exact(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = __fsub_rn(ax, bx), dy = __fsub_rn(ay, by), dz = __fsub_rn(az, bz);
  float d2 = __fmul_rn(dx, dx);
  d2 = __fadd_rn(d2, __fmul_rn(dy, dy));
  d2 = __fadd_rn(d2, __fmul_rn(dz, dz));
  return d2;
}

__device__ __forceinline__ int lane_id() { return threadIdx.x & (D3F_WAVE - 1); }

// Measurement aid (d3f_debug_set_phase_clock): per-phase shader cycles of a kernel's waves.  `out` (device uint64, null
// in normal operation): out[0] = number of waves recorded (atomic ticket, taken once per wave at its end), out[1] =
// record capacity; record r (8 words) starts at out[8 + 8 r] and holds the cycles the wave spent before each lap(i).
// The laps live in scalar registers until the wave's last instruction: no memory operation of the clock sits inside
// the measured phases (an atomic per lap would queue behind the kernel's own loads and be waited for by its vmcnt).
struct PhaseClock {
  unsigned long long* out;
  unsigned long long t, acc[6];
  __device__ __forceinline__ void start(unsigned long long* o) {
    out = o;
    if (out) {
#pragma unroll
      for (int i = 0; i < 6; ++i) acc[i] = 0;
      t = __builtin_readcyclecounter();
    }
  }
  __device__ __forceinline__ void lap(int i) {
    if (out) {
      const unsigned long long n = __builtin_readcyclecounter();
#pragma unroll
      for (int j = 0; j < 6; ++j)
        if (j == i) acc[j] += n - t;
      t = n;
    }
  }
  __device__ __forceinline__ void done() {
    if (out && (threadIdx.x & 63) == 0) {
      const unsigned long long r = atomicAdd(out, 1ull);
      if (r < out[1]) {
#pragma unroll
        for (int j = 0; j < 6; ++j) out[8 + 8 * r + j] = acc[j];
      }
    }
  }
};
unsigned long long* phase_clock_ptr();   // kpconv_fused.hip

// x of lane (l ^ j) for the butterfly distances of a 64-lane wave WITHOUT the LDS crossbar: __shfl_xor compiles to
// ds_bpermute_b32 (an LDS-pipe instruction with its address arithmetic and ~100 cycles of dependent latency) -- the
// 64-key bitonic network of a query is 21 dependent exchanges of a 64-bit key = 42 of them.  Distances 1, 2, 8 are one
// DPP move (quad_perm / row_ror), 4 is two (row_shl / row_shr under complementary bank masks), 16 and 32 are gfx950's
// v_permlane16_swap / v_permlane32_swap (rows of the two operands exchanged; the lane's row bit picks the half).
__device__ __forceinline__ uint32_t lane_xor(uint32_t x, int j, int lane) {
  switch (j) {
    case 1: return (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0xB1, 0xF, 0xF, false);    // quad_perm [1,0,3,2]
    case 2: return (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x4E, 0xF, 0xF, false);    // quad_perm [2,3,0,1]
    case 4: {
      int r = __builtin_amdgcn_update_dpp((int)x, (int)x, 0x104, 0xF, 0x5, false);                  // banks 0, 2 <- lane + 4
      return (uint32_t)__builtin_amdgcn_update_dpp(r, (int)x, 0x114, 0xF, 0xA, false);              // banks 1, 3 <- lane - 4
    }
    case 8: return (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x128, 0xF, 0xF, false);   // row_ror:8
    case 16: {
      const auto p = __builtin_amdgcn_permlane16_swap(x, x, false, false);
      return (lane & 16) ? p[0] : p[1];
    }
    case 32: {
      const auto p = __builtin_amdgcn_permlane32_swap(x, x, false, false);
      return (lane & 32) ? p[0] : p[1];
    }
    default: return __shfl_xor(x, j, 64);
  }
}
__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int m) {
  const int lane = threadIdx.x & 63;
  const uint32_t lo = lane_xor((uint32_t)v, m, lane), hi = lane_xor((uint32_t)(v >> 32), m, lane);
  return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ double shfl_xor_f64(double v, int m) {
  return __longlong_as_double((long long)shfl_xor_u64((uint64_t)__double_as_longlong(v), m));
}
// every entry of v summed over the wave, in every lane: the fixed butterfly the deterministic f64 reductions share
template <int kN>
__device__ __forceinline__ void wave_sum_f64(double (&v)[kN]) {
#pragma unroll
  for (int k = 0; k < kN; ++k)
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v[k] += shfl_xor_f64(v[k], o);
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

}  // namespace d3f
