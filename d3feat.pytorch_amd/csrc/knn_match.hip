// k-nearest descriptor matching on the f32 matrix cores: the k best target columns of every source row by the rule of
// knn_match.hpp, without forming the Ns x Nt distance matrix.
//
//   sweep   the row side of matching.hip's row_argmin_kernel: workgroup = 4 waves x (RT x 16) source rows whose A
//           fragments stay in registers, target descriptors stream through in tiles of 64, the same
//           v_mfma_f32_16x16x4_f32 chain per (row, column) product.  A lane owns 4 RT rows and, of each 16-column block,
//           one column; per row it keeps its best KMAX candidates (product, column) in registers, sorted by (rounded
//           distance, column).  One compare per product on the raw product drops what cannot rank among the lane's k
//           (knn_match.hpp says why that is exact); the threshold is shared among the 16 lanes of a row every other tile.
//           Insertion is an unrolled compare-and-shift on the rounded roots.  After the sweep the 16 lanes of a row
//           merge their lists by k rounds of a butterfly minimum over 64-bit keys (distance bits << 32 | column) and
//           the chunk's k keys of the row go to the workspace [chunks, rows, k].
//   merge   one thread per row folds the chunks' sorted keys into the k best and unpacks idx / dist.
// No atomics, no LDS, no barrier: every output is written by exactly one thread.
#include "knn_match.hpp"

namespace {

using namespace d3f::match;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

constexpr u64 kEmpty = ~0ull;   // no candidate: ranks behind every key, unpacks to idx -1 / dist +inf

// the rule's key of a product: -inf where the reference's distance is NaN (2 - 2a < 0, or a NaN product)
__device__ __forceinline__ float dkey(float a) {
  const float v = fmaf(-2.0f, a, 2.0f);   // (2a is exact: one rounding, as in 2 - 2a)
  return !(v >= 0.0f) ? -INFINITY : sqrt_rn(v);
}

// (a, j) into the list sorted by (rounded distance, column); j is larger than every column in it, so it goes behind
// its equals.  Fully unrolled: the list stays in registers.
template <int KMAX>
__device__ __forceinline__ void insert(float (&la)[KMAX], int (&lj)[KMAX], float a, int j) {
  const float dn = dkey(a);
  bool lt[KMAX];
#pragma unroll
  for (int s = 0; s < KMAX; ++s) lt[s] = lj[s] < 0 || dn < dkey(la[s]);
#pragma unroll
  for (int s = KMAX - 1; s > 0; --s) {
    la[s] = lt[s] ? (lt[s - 1] ? la[s - 1] : a) : la[s];
    lj[s] = lt[s] ? (lt[s - 1] ? lj[s - 1] : j) : lj[s];
  }
  la[0] = lt[0] ? a : la[0];
  lj[0] = lt[0] ? j : lj[0];
}

// seg != nullptr: blockIdx.z = pair, as in row_argmin_kernel; `out` rows are those of the stacked source matrix.
// out [gridDim.y, out_rows, k] keys: chunk c of a row holds its k best of the columns [c cpc, (c + 1) cpc), ascending.
template <int C, int RT, int KMAX>
__global__ __launch_bounds__(256) void knn_sweep_kernel(const float* __restrict__ S, int Ns, const float* __restrict__ T,
                                                        int Nt, int cols_per_chunk, int k, u64* __restrict__ out,
                                                        int out_rows, const int32_t* __restrict__ seg = nullptr) {
  static_assert(C % 16 == 0, "descriptor width must be a multiple of 16");
  if (seg) {
    const int32_t* e = seg + 4 * blockIdx.z;
    const int so = e[0], sn = e[1], to = e[2], tn = e[3];
    S += (size_t)so * C;
    T += (size_t)to * C;
    out += (size_t)so * k;
    Ns = sn;
    Nt = tn;
    if (Ns < 1 || Nt < 1) return;
  }
  constexpr int KS = C / 16;  // float4 chunks per lane: reduction index c = 16*u + 4*(lane>>4) + t
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int row0 = (blockIdx.x * 4 + wave) * (16 * RT);
  const int cbeg = blockIdx.y * cols_per_chunk, cend = min(Nt, cbeg + cols_per_chunk);
  if (row0 >= Ns || cbeg >= cend) return;   // (no barrier in this kernel: a wave may leave alone)
  // A fragments: A[i = li][kk = lk] for step (u,t) of row tile rt is S[row0 + 16rt + li][16u + 4lk + t]
  float4 afrag[RT][KS];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int r = min(row0 + 16 * rt + li, Ns - 1);
#pragma unroll
    for (int u = 0; u < KS; ++u) afrag[rt][u] = *(const float4*)(S + (size_t)r * C + 16 * u + 4 * lk);
  }
  // per lane and row: the sorted candidates among THIS lane's columns and thr, the largest product known to be the k-th
  // of some lane's list over earlier columns; a product a <= thr cannot rank among the row's k.
  float la[RT][4][KMAX], thr[RT][4];
  int lj[RT][4][KMAX];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      thr[rt][r] = -INFINITY;
#pragma unroll
      for (int s = 0; s < KMAX; ++s) { la[rt][r][s] = -INFINITY; lj[rt][r][s] = -1; }
    }

  for (int col0 = cbeg; col0 < cend; col0 += kColsPerTile) {
    float4 bfrag[4][KS];
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
      const int cj = min(col0 + 16 * nb + li, Nt - 1);
#pragma unroll
      for (int u = 0; u < KS; ++u) bfrag[nb][u] = *(const float4*)(T + (size_t)cj * C + 16 * u + 4 * lk);
    }
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
      f32x4 acc[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) acc[rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      // (the order of row_argmin_kernel: u ascending, then x, y, z, w -- a product is the same bit pattern in both)
#pragma unroll
      for (int u = 0; u < KS; ++u) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(afrag[rt][u].x, bfrag[nb][u].x, acc[rt], 0, 0, 0);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(afrag[rt][u].y, bfrag[nb][u].y, acc[rt], 0, 0, 0);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(afrag[rt][u].z, bfrag[nb][u].z, acc[rt], 0, 0, 0);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(afrag[rt][u].w, bfrag[nb][u].w, acc[rt], 0, 0, 0);
      }
      // D layout: col = li (target col0 + 16nb + li), row = 4*lk + r of row tile rt; columns ascend within a lane
      const int j = col0 + 16 * nb + li;
      bool any = false;  // one branch per 16 x 16*RT products instead of one per product
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) any |= !(acc[rt][r] <= thr[rt][r]);   // (a NaN product is a candidate: it ranks first)
      if (any && j < cend) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (!(acc[rt][r] <= thr[rt][r])) {
              insert<KMAX>(la[rt][r], lj[rt][r], acc[rt][r], j);
              // the lane's k-th product, once it has k (an empty slot holds -inf; fmaxf keeps thr over a NaN)
              float ak = -INFINITY;
#pragma unroll
              for (int s = 0; s < KMAX; ++s) ak = s == k - 1 ? la[rt][r][s] : ak;
              thr[rt][r] = fmaxf(thr[rt][r], ak);
            }
      }
    }
    // every other tile: share the threshold among the 16 lanes of each row (their columns all lie behind now)
    if (((col0 - cbeg) / kColsPerTile) & 1) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float f = thr[rt][r];
#pragma unroll
          for (int o = 8; o > 0; o >>= 1) f = fmaxf(f, __shfl_xor(f, o, 64));
          thr[rt][r] = f;
        }
    }
  }
  // merge the 16 lanes that share a row: k rounds, each takes the smallest head; keys are distinct, so one lane pops
  u64* o = out + (size_t)blockIdx.y * out_rows * k;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      u64 key[KMAX];
#pragma unroll
      for (int s = 0; s < KMAX; ++s)
        key[s] = (s < k && lj[rt][r][s] >= 0) ? ((u64)ord_bits(dkey(la[rt][r][s])) << 32) | (uint32_t)lj[rt][r][s] : kEmpty;
      const int row = row0 + 16 * rt + 4 * lk + r;
#pragma unroll
      for (int s = 0; s < KMAX; ++s)
        if (s < k) {
          u64 m = key[0];
#pragma unroll
          for (int x = 8; x > 0; x >>= 1) {
            const u64 ok = d3f::shfl_xor_u64(m, x);
            m = ok < m ? ok : m;
          }
          if (li == 0 && row < Ns) o[(size_t)row * k + s] = m;
          const bool pop = key[0] == m;   // (all empty: every lane "pops" an empty list)
#pragma unroll
          for (int q = 0; q + 1 < KMAX; ++q) key[q] = pop ? key[q + 1] : key[q];
          key[KMAX - 1] = pop ? kEmpty : key[KMAX - 1];
        }
    }
}

// one thread per source row: the k best of the chunks' keys (each chunk's are ascending), unpacked.
// seg == nullptr: one problem of Ns x Nt; else blockIdx.y = pair and rows / outputs are offset by its src_off.
__global__ void knn_merge_kernel(const u64* __restrict__ ws, int ws_rows, int ws_chunks, int Ns, int Nt, int cols_per_chunk,
                                 int k, const int32_t* __restrict__ seg, int32_t* __restrict__ idx, float* __restrict__ dist) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (seg) {
    const int32_t* e = seg + 4 * blockIdx.y;
    Ns = e[1];
    Nt = e[3];
    if (i >= Ns) return;
    i += e[0];
  } else if (i >= Ns) {
    return;
  }
  u64 best[D3F_KNN_MAX];
#pragma unroll
  for (int s = 0; s < D3F_KNN_MAX; ++s) best[s] = kEmpty;
  // the chunks the sweep wrote for this pair (a target longer than the host bound is cut at the grid, like the sweep's)
  const int chunks = Nt > 0 ? min(ws_chunks, (Nt + cols_per_chunk - 1) / cols_per_chunk) : 0;
  for (int c = 0; c < chunks; ++c) {
    const u64* p = ws + ((size_t)c * ws_rows + i) * k;
    for (int s = 0; s < k; ++s) {
      const u64 key = p[s];
      if (key == kEmpty) break;
      bool lt[D3F_KNN_MAX];
#pragma unroll
      for (int q = 0; q < D3F_KNN_MAX; ++q) lt[q] = key < best[q];
#pragma unroll
      for (int q = D3F_KNN_MAX - 1; q > 0; --q) best[q] = lt[q] ? (lt[q - 1] ? best[q - 1] : key) : best[q];
      best[0] = lt[0] ? key : best[0];
    }
  }
#pragma unroll
  for (int s = 0; s < D3F_KNN_MAX; ++s)
    if (s < k) {
      const u64 key = best[s];
      const uint32_t ob = (uint32_t)(key >> 32);
      const float d = __uint_as_float((ob & 0x80000000u) ? (ob & 0x7fffffffu) : ~ob);   // ord_bits undone
      const bool empty = key == kEmpty;
      idx[(size_t)i * k + s] = empty ? -1 : (int32_t)(key & 0xffffffffull);
      dist[(size_t)i * k + s] = empty ? INFINITY : (d == -INFINITY ? __uint_as_float(0x7fc00000u) : d);
    }
}

// Row tiles per wave.  The lists cost 8 RT KMAX registers, the B fragments of a tile C, the A fragments RT C / 4:
// two row tiles where that leaves two waves per SIMD (KMAX <= 4, C <= 64), one otherwise.
template <int C, int KMAX>
constexpr int row_tiles() { return (C <= 64 && KMAX <= 4) ? 2 : 1; }

static int kmax_of(int k) { return k <= 2 ? 2 : (k <= 4 ? 4 : 8); }
static int rows_per_wg(int C, int k) { return (C <= 64 && kmax_of(k) <= 4) ? 128 : 64; }

template <int C, int KMAX>
int launch(const float* S, int src_rows, int Ns, const float* T, int Nt, const int32_t* seg, int P, int k, int32_t* idx,
           float* dist, void* ws, size_t ws_bytes, hipStream_t stream) {
  constexpr int RT = row_tiles<C, KMAX>();
  const int gx = d3f::cdiv(Ns, 64 * RT);
  int chunks, cpc;
  chunking(gx * P, Nt, chunks, cpc);
  if (ws_bytes < sizeof(u64) * (size_t)chunks * src_rows * k) return D3F_EWORKSPACE;
  knn_sweep_kernel<C, RT, KMAX><<<dim3(gx, chunks, P), 256, 0, stream>>>(S, seg ? 0 : Ns, T, seg ? 0 : Nt, cpc, k,
                                                                        (u64*)ws, src_rows, seg);
  knn_merge_kernel<<<dim3(d3f::cdiv(Ns, 256), P), 256, 0, stream>>>((const u64*)ws, src_rows, chunks, Ns, Nt, cpc, k, seg,
                                                                     idx, dist);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

template <int C>
int launch_k(const float* S, int src_rows, int Ns, const float* T, int Nt, const int32_t* seg, int P, int k,
             int32_t* idx, float* dist, void* ws, size_t ws_bytes, hipStream_t stream) {
  switch (kmax_of(k)) {
    case 2: return launch<C, 2>(S, src_rows, Ns, T, Nt, seg, P, k, idx, dist, ws, ws_bytes, stream);
    case 4: return launch<C, 4>(S, src_rows, Ns, T, Nt, seg, P, k, idx, dist, ws, ws_bytes, stream);
    default: return launch<C, 8>(S, src_rows, Ns, T, Nt, seg, P, k, idx, dist, ws, ws_bytes, stream);
  }
}

// Ns / Nt: the one problem's sizes, or (batched) the host bounds max_src / max_tgt that size the grid
int dispatch(const float* S, int src_rows, int Ns, const float* T, int Nt, const int32_t* seg, int P, int C, int k,
             int32_t* idx, float* dist, void* ws, size_t ws_bytes, hipStream_t stream) {
  switch (C) {
    case 16: return launch_k<16>(S, src_rows, Ns, T, Nt, seg, P, k, idx, dist, ws, ws_bytes, stream);
    case 32: return launch_k<32>(S, src_rows, Ns, T, Nt, seg, P, k, idx, dist, ws, ws_bytes, stream);
    case 64: return launch_k<64>(S, src_rows, Ns, T, Nt, seg, P, k, idx, dist, ws, ws_bytes, stream);
    case 128: return launch_k<128>(S, src_rows, Ns, T, Nt, seg, P, k, idx, dist, ws, ws_bytes, stream);
    default: return D3F_EINVAL;
  }
}

// bytes of the [chunks, rows, k] keys for any width: the fewest row workgroups (128 rows each) give the most chunks
size_t ws_bytes_of(int src_rows, int Ns, int Nt, int P, int k) {
  if (src_rows < 1 || Ns < 1 || Nt < 1 || P < 1 || k < 1 || k > D3F_KNN_MAX) return 0;
  int chunks, cpc;
  chunking(d3f::cdiv(Ns, 128) * P, Nt, chunks, cpc);
  return d3f::align_up(sizeof(u64) * (size_t)chunks * src_rows * k, 256);
}

}  // namespace

extern "C" {

size_t d3f_knn_match_ws_bytes(int Ns, int Nt, int k) { return ws_bytes_of(Ns, Ns, Nt, 1, k); }

int d3f_knn_match(const float* src_desc, int Ns, const float* tgt_desc, int Nt, int C, int k, int32_t* idx, float* dist,
                  void* ws, size_t ws_bytes, void* stream) {
  if (!src_desc || !tgt_desc || !idx || !dist || !ws || Ns < 1 || Nt < 1 || k < 1 || k > D3F_KNN_MAX) return D3F_EINVAL;
  return dispatch(src_desc, Ns, Ns, tgt_desc, Nt, nullptr, 1, C, k, idx, dist, ws, ws_bytes, (hipStream_t)stream);
}

size_t d3f_knn_match_batched_ws_bytes(int src_rows, int P, int max_src, int max_tgt, int k) {
  return ws_bytes_of(src_rows, max_src, max_tgt, P, k);
}

int d3f_knn_match_batched(const float* src_desc, int src_rows, const float* tgt_desc, int tgt_rows, const int32_t* seg,
                          int P, int max_src, int max_tgt, int C, int k, int32_t* idx, float* dist, void* ws,
                          size_t ws_bytes, void* stream) {
  if (!src_desc || !tgt_desc || !seg || !idx || !dist || !ws || src_rows < 1 || tgt_rows < 1 || P < 1 || P > 65535 ||
      max_src < 1 || max_tgt < 1 || k < 1 || k > D3F_KNN_MAX)
    return D3F_EINVAL;
  return dispatch(src_desc, src_rows, max_src, tgt_desc, max_tgt, seg, P, C, k, idx, dist, ws, ws_bytes,
                  (hipStream_t)stream);
}

}  // extern "C"
