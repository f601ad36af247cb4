// Training items from a device-resident 3DMatch split (include/d3feat_hip.h, "Training items ..."): the augmented
// clouds, the correspondence sample and its keypoint distances of up to 16 items per call, in two launches.  The
// arithmetic lives in augment.hpp (shared with d3f_augment_item_host); this file is the parallel form of it.
//
// augment_points_kernel: one thread per output coordinate, grid (blocks, job).
// augment_select_kernel: ONE workgroup of 1024 threads per job.
//   corr_len <= k: all rows in table order.
//   corr_len >  k: radix select of the k-th smallest sort key z(7, j), 8 bits per pass from the top.  Each pass
//     recomputes all keys (nothing is stored: 20 integer operations against 8 bytes of traffic), histograms the next
//     digit of those that match the prefix found so far in LDS, and finds the digit at which the running count crosses
//     k.  Invariant: `below` keys are smaller than every key with the prefix (all selected), and
//     below < k <= below + count(prefix).  As soon as below + count(prefix) <= kCap those keys are gathered into LDS
//     with their rows, bitonic-sorted by (key, row) and the first k written.  Keys are distinct, so after the last
//     pass count(prefix) = 1 and the loop ends with exactly k candidates at the latest: exact for any corr_len < 2^31
//     however crowded a bin is.  The gather order depends on LDS atomics, the sorted result does not.
#include <algorithm>
#include <utility>
#include <vector>

#include "augment.hpp"
#include "common.hpp"

namespace {

namespace aug = d3f::augment;

struct Jobs {   // travels in the kernel argument (16 x 176 B), like the prefix table of atb_grouped_kernel
  d3f_augment_job j[D3F_AUGMENT_MAX_JOBS];
};

constexpr int kPointThreads = 256;
constexpr int kSelThreads = 1024;
constexpr int kBins = 256;
constexpr int kCap = D3F_AUGMENT_CANDIDATES;
static_assert(D3F_AUGMENT_MAX_NODE <= kCap, "the last pass leaves exactly k candidates");
static_assert(kCap <= kSelThreads && (kCap & (kCap - 1)) == 0, "one thread per candidate slot of the sort");

__global__ __launch_bounds__(kPointThreads) void augment_points_kernel(const float* __restrict__ points,
                                                                       const Jobs jobs, double noise) {
  const d3f_augment_job& J = jobs.j[blockIdx.y];
  const long long e0 = 3ll * J.src_len, total = e0 + 3ll * J.tgt_len;
  const float* src = points + 3 * J.src_off;
  const float* tgt = points + 3 * J.tgt_off;
  for (long long e = (long long)blockIdx.x * kPointThreads + threadIdx.x; e < total;
       e += (long long)gridDim.x * kPointThreads) {
    if (e < e0) {
      const uint32_t i = (uint32_t)(e / 3);
      const int a = (int)(e - 3ll * i);
      J.out_src[e] = aug::source_coord(src + 3ll * i, J.key, a, i, noise);
    } else {
      const long long f = e - e0;
      const uint32_t i = (uint32_t)(f / 3);
      const int a = (int)(f - 3ll * i);
      J.out_tgt[f] = aug::target_coord(tgt + 3ll * i, J.R, J.t, J.key, a, i, noise);
    }
  }
}

__device__ __forceinline__ bool key_row_greater(uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) {
  return ka > kb || (ka == kb && ia > ib);
}

__global__ __launch_bounds__(kSelThreads) void augment_select_kernel(const float* __restrict__ points,
                                                                     const int32_t* __restrict__ corr, const Jobs jobs,
                                                                     int k, double noise) {
  __shared__ uint32_t hist[kBins];
  __shared__ uint64_t ckey[kCap];
  __shared__ uint32_t crow[kCap];
  __shared__ float apt[3 * D3F_AUGMENT_MAX_NODE];
  __shared__ uint32_t s_digit, s_below, s_count, s_n;
  const d3f_augment_job& J = jobs.j[blockIdx.x];
  const uint32_t tid = threadIdx.x;
  const uint32_t M = (uint32_t)J.corr_len;
  const uint64_t key = J.key;
  const int32_t* tab = corr + 2 * J.corr_off;
  uint32_t m;
  if (M <= (uint32_t)k) {
    m = M;
    if (tid < m) crow[tid] = tid;
    __syncthreads();
  } else {
    m = (uint32_t)k;
    uint64_t prefix = 0;
    uint32_t below = 0, cand = M;
    int shift = 64;
    do {
      shift -= 8;
      const bool first = shift == 56;
      if (tid < kBins) hist[tid] = 0u;
      __syncthreads();
      for (uint32_t j = tid; j < M; j += kSelThreads) {
        const uint64_t z = aug::z_of(key, aug::kStreamSelect, j);
        if (first || (z >> (shift + 8)) == prefix) atomicAdd(&hist[(uint32_t)(z >> shift) & (kBins - 1)], 1u);
      }
      __syncthreads();
      if (tid < kBins) {
        uint32_t c = 0;
        for (uint32_t b = 0; b < tid; ++b) c += hist[b];
        const uint32_t h = hist[tid], need = m - below;      // 1 <= need <= count(prefix)
        if (c < need && need <= c + h) {                      // exactly one digit: the count crosses `need` once
          s_digit = tid;
          s_below = below + c;
          s_count = h;
        }
      }
      __syncthreads();
      prefix = (prefix << 8) | s_digit;
      below = s_below;
      cand = below + s_count;
      __syncthreads();   // everyone has read s_* and hist before the next pass rewrites them
    } while (cand > (uint32_t)kCap && shift > 0);
    if (tid == 0) s_n = 0u;
    __syncthreads();
    for (uint32_t j = tid; j < M; j += kSelThreads) {
      const uint64_t z = aug::z_of(key, aug::kStreamSelect, j);
      if ((z >> shift) <= prefix) {
        const uint32_t slot = atomicAdd(&s_n, 1u);
        if (slot < (uint32_t)kCap) {    // (always: the histograms counted exactly these keys)
          ckey[slot] = z;
          crow[slot] = j;
        }
      }
    }
    __syncthreads();
    const uint32_t n = cand < (uint32_t)kCap ? cand : (uint32_t)kCap;
    uint32_t P = 1;
    while (P < n) P <<= 1;
    if (tid >= n && tid < P) {   // padding sorts behind every real (key, row)
      ckey[tid] = ~0ull;
      crow[tid] = ~0u;
    }
    for (uint32_t size = 2; size <= P; size <<= 1) {
      for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
        __syncthreads();
        const uint32_t p = tid ^ stride;
        if (tid < P && p > tid) {
          const uint64_t ka = ckey[tid], kb = ckey[p];
          const uint32_t ia = crow[tid], ib = crow[p];
          const bool ascending = (tid & size) == 0;
          if (key_row_greater(ka, ia, kb, ib) == ascending) {
            ckey[tid] = kb; ckey[p] = ka;
            crow[tid] = ib; crow[p] = ia;
          }
        }
      }
    }
    __syncthreads();
  }
  // the selected rows, and their augmented source points (recomputed, not read back from out_src)
  if (tid < m) {
    const uint32_t j = crow[tid];
    const int32_t s = tab[2ll * j], t = tab[2ll * j + 1];
    J.out_corr[2 * tid] = (int64_t)s;
    J.out_corr[2 * tid + 1] = (int64_t)t;
    const uint32_t row = aug::clamp_row(s, J.src_len);
    const float* p = points + 3 * (J.src_off + (long long)row);
#pragma unroll
    for (int a = 0; a < 3; ++a) apt[3 * tid + a] = aug::source_coord(p, key, a, row, noise);
  }
  __syncthreads();
  for (uint32_t e = tid; e < m * m; e += kSelThreads) {
    const uint32_t r = e / m, c = e - r * m;
    J.out_dist[e] = sqrt(aug::dist2(apt + 3 * r, apt + 3 * c));
  }
}

bool job_ok(const d3f_augment_job& J, int64_t sum_n, int64_t sum_m) {
  return J.src_len >= 1 && J.tgt_len >= 0 && J.corr_len >= 1 && J.src_off >= 0 && J.tgt_off >= 0 && J.corr_off >= 0 &&
         J.src_off + J.src_len <= sum_n && J.tgt_off + J.tgt_len <= sum_n && J.corr_off + J.corr_len <= sum_m &&
         J.out_src && (J.out_tgt || J.tgt_len == 0) && J.out_corr && J.out_dist;
}

}  // namespace

extern "C" {

size_t d3f_augment_pairs_ws_bytes(int B, int k) {
  (void)B;
  (void)k;
  return 0;
}

int d3f_augment_pairs(const float* points, int64_t sum_n, const int32_t* corr, int64_t sum_m, const d3f_augment_job* jobs,
                      int B, int k, double noise, void* ws, size_t ws_bytes, void* stream) {
  (void)ws;
  if (!points || !corr || !jobs || B < 1 || B > D3F_AUGMENT_MAX_JOBS || k < 1 || k > D3F_AUGMENT_MAX_NODE ||
      !(noise >= 0.0) || !(noise < INFINITY) || sum_n < 1 || sum_m < 1)
    return D3F_EINVAL;
  if (ws_bytes < d3f_augment_pairs_ws_bytes(B, k)) return D3F_EWORKSPACE;
  Jobs table = {};
  long long most = 0;
  for (int b = 0; b < B; ++b) {
    if (!job_ok(jobs[b], sum_n, sum_m)) return D3F_EINVAL;
    table.j[b] = jobs[b];
    most = std::max(most, 3ll * jobs[b].src_len + 3ll * jobs[b].tgt_len);
  }
  hipStream_t s = (hipStream_t)stream;
  const unsigned blocks = (unsigned)std::min<long long>(d3f::cdiv(most, kPointThreads), 2048);
  augment_points_kernel<<<dim3(blocks, B), kPointThreads, 0, s>>>(points, table, noise);
  augment_select_kernel<<<B, kSelThreads, 0, s>>>(points, corr, table, k, noise);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_augment_item_host(const float* points_host, const int32_t* corr_host, const d3f_augment_job* job, int k,
                          double noise) {
  if (!points_host || !corr_host || !job || k < 1 || !(noise >= 0.0) || !(noise < INFINITY)) return D3F_EINVAL;
  const d3f_augment_job& J = *job;
  if (!job_ok(J, J.src_off + J.src_len > J.tgt_off + J.tgt_len ? J.src_off + J.src_len : J.tgt_off + J.tgt_len,
              J.corr_off + J.corr_len))
    return D3F_EINVAL;
  const float* src = points_host + 3 * J.src_off;
  const float* tgt = points_host + 3 * J.tgt_off;
  const int32_t* tab = corr_host + 2 * J.corr_off;
  for (int32_t i = 0; i < J.src_len; ++i)
    for (int a = 0; a < 3; ++a) J.out_src[3ll * i + a] = aug::source_coord(src + 3ll * i, J.key, a, (uint32_t)i, noise);
  for (int32_t i = 0; i < J.tgt_len; ++i)
    for (int a = 0; a < 3; ++a)
      J.out_tgt[3ll * i + a] = aug::target_coord(tgt + 3ll * i, J.R, J.t, J.key, a, (uint32_t)i, noise);
  const int32_t M = J.corr_len;
  const int m = M <= k ? M : k;
  std::vector<int32_t> rows((size_t)m);
  if (M <= k) {
    for (int r = 0; r < m; ++r) rows[r] = r;
  } else {
    std::vector<std::pair<uint64_t, int32_t>> keys((size_t)M);
    for (int32_t j = 0; j < M; ++j) keys[j] = {aug::z_of(J.key, aug::kStreamSelect, (uint32_t)j), j};
    std::partial_sort(keys.begin(), keys.begin() + m, keys.end());
    for (int r = 0; r < m; ++r) rows[r] = keys[r].second;
  }
  std::vector<float> apt(3 * (size_t)m);
  for (int r = 0; r < m; ++r) {
    const int32_t s = tab[2ll * rows[r]], t = tab[2ll * rows[r] + 1];
    J.out_corr[2 * r] = s;
    J.out_corr[2 * r + 1] = t;
    const uint32_t row = aug::clamp_row(s, J.src_len);
    for (int a = 0; a < 3; ++a) apt[3 * r + a] = aug::source_coord(src + 3ll * row, J.key, a, row, noise);
  }
  for (int r = 0; r < m; ++r)
    for (int c = 0; c < m; ++c) J.out_dist[(size_t)r * m + c] = sqrt(aug::dist2(&apt[3 * r], &apt[3 * c]));
  return m;
}

uint64_t d3f_augment_key_host(uint64_t key, int stream, uint32_t index) { return aug::z_of(key, stream, index); }

}  // extern "C"
