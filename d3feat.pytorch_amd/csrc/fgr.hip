// Batched fast global registration of P correspondence sets (include/d3feat_hip.h: d3f_fgr_rigid) -- what a pipeline
// would hand to Open3D's registration_fgr_based_on_correspondence, as ONE launch: no host synchronisation, no
// floating-point atomic, graph-capturable.  The rule (tuple test, centring, annealing, the Gauss-Newton step, the
// summation order) is csrc/fgr.hpp; this file is its two carriers.
//
// fgr_kernel: grid P, 256 threads; a workgroup runs its pair from the tuple test to the result.
//   Tuple test: chunks of 256 trials h in order, one per thread.  A ballot per wave plus the prefix over the 4 wave
//   counts ranks every passing trial among all passing trials so far, so "the first max_tuples in order of h" is
//   exact; the loop leaves as soon as the cap is reached.  Multiplicities are integers added with atomicAdd to the
//   pair's slice of the workspace (order-free) and read back with agent-scope loads, which are served where the
//   atomics were performed.
//   Loop: the rows are STREAMED on every iteration -- one path for every count.  A pair has at most 65536 rows of 28
//   bytes (1.8 MB; a few thousand rows, ~100 KB, in practice): that does not fit LDS at the upper end but sits in L2 for
//   all 128 passes, and a second, LDS-resident path would be a second summation carrier to keep bit-equal.  Thread s
//   adds rows s, s + 256, ... into 16 f64 partials in registers, the wave butterfly and 4 LDS slots per sum give every
//   thread the totals; thread 0 takes the 6x6 step and hands the pose on through LDS (the solve's registers are
//   then live in no row loop).
// d3f_fgr_rigid_host: the same rule on one CPU thread, the 256 workers in turn, the same tree.
#include <vector>

#include "common.hpp"
#include "fgr.hpp"

namespace {

using namespace d3f::fgr;

constexpr int kThreads = kWorkers;
constexpr int kWaves = kThreads / D3F_WAVE;

struct Params {
  const float* src;
  const float* tgt;
  int rows;
  const int32_t* seg;
  int first_pair;
  double delta;
  int iterations;
  double division_factor;
  int anneal_every;
  double tuple_scale;
  int tuple_trials, max_tuples;
  uint64_t seed;
  double* T;
  int32_t *inliers, *tuples;
  double* weight_sum;
  int32_t *status, *multiplicity;
  double* trace;
  int32_t* mult;   // the workspace: one slot per row
};

// (offset, count) of pair p and its status bits; count = 0 when the segment cannot be addressed
D3F_HD inline int pair_segment(const int32_t* seg, int p, int rows, int& off, int& count) {
  off = seg[2 * p];
  count = seg[2 * p + 1];
  if (off < 0 || count < 0 || count > D3F_RANSAC_MAX_COUNT || (long long)off + count > rows) {
    off = 0;
    count = 0;
    return kStSegment;
  }
  return count < 3 ? kStFew : 0;
}

D3F_HD inline void write_trace(double* trace, int p, int iterations, int it, double mu, double wsum, const double d[6]) {
  if (!trace) return;
  double* o = trace + 8 * ((size_t)p * iterations + it);
  o[0] = mu;
  o[1] = wsum;
  for (int k = 0; k < 6; ++k) o[2 + k] = d[k];
}

__device__ __forceinline__ int load_mult(const int32_t* m) {
  return __hip_atomic_load(m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// every entry of v summed over the workgroup in the rule's tree; every thread gets the totals
template <int N>
__device__ __forceinline__ void block_sum(double (*slot)[kSums], double (&v)[N]) {
  d3f::wave_sum_f64(v);
  __syncthreads();   // the slots' previous values are consumed
  if (d3f::lane_id() == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) slot[threadIdx.x / D3F_WAVE][k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = ((slot[0][k] + slot[1][k]) + slot[2][k]) + slot[3][k];
}

__device__ __forceinline__ int block_sum_i(int* slot, int v) {
  v = d3f::wave_sum_i(v);
  __syncthreads();
  if (d3f::lane_id() == 0) slot[threadIdx.x / D3F_WAVE] = v;
  __syncthreads();
  return (slot[0] + slot[1]) + (slot[2] + slot[3]);
}

__global__ __launch_bounds__(kThreads) void fgr_kernel(Params a) {
  __shared__ double slot[kWaves][kSums];
  __shared__ int islot[kWaves];
  __shared__ double pose[12];
  const int p = blockIdx.x, tid = threadIdx.x;
  int off, count;
  int st = pair_segment(a.seg, p, a.rows, off, count);
  const float* src = a.src + 3 * (size_t)off;
  const float* tgt = a.tgt + 3 * (size_t)off;
  int32_t* mult = a.mult + off;
  const int trials = trials_of(a.tuple_trials, count);

  // ---- tuple test
  for (int i = tid; i < count; i += kThreads)
    __hip_atomic_store(mult + i, trials == 0 ? 1 : 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  int taken = 0;
  if (st == 0 && trials > 0) {
    const uint64_t key = d3f::rigid::pair_key(a.seed, a.first_pair + p);
    for (int base = 0; base < trials; base += kThreads) {
      const int h = base + tid;
      int idx[3];
      const bool ok = h < trials && tuple_trial(a.src, a.tgt, off, count, key, h, a.tuple_scale, idx);
      const unsigned long long ballot = __ballot(ok);
      const int lane = d3f::lane_id(), wave = tid / D3F_WAVE;
      __syncthreads();   // the previous chunk's counts are consumed
      if (lane == 0) islot[wave] = __popcll(ballot);
      __syncthreads();
      int before = taken, total = 0;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        before += w < wave ? islot[w] : 0;
        total += islot[w];
      }
      const int rank = before + __popcll(ballot & ((1ull << lane) - 1ull));
      if (ok && (a.max_tuples == 0 || rank < a.max_tuples)) {
#pragma unroll
        for (int k = 0; k < 3; ++k) atomicAdd(mult + idx[k], 1);
      }
      taken += total;
      if (a.max_tuples > 0 && taken >= a.max_tuples) {
        taken = a.max_tuples;
        break;
      }
    }
  }
  __syncthreads();   // (the workgroup's atomics are performed before any thread reads a multiplicity)

  // ---- centring over the live rows
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0}, ca[3] = {0, 0, 0}, cb[3] = {0, 0, 0};
  double wsum = 0.0;
  if (st == 0) {
    double v[6] = {0, 0, 0, 0, 0, 0};
    int n = 0;
    for (int i = tid; i < count; i += kThreads) {
      if (load_mult(mult + i) > 0) {
        ++n;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          v[c] += (double)src[3 * (size_t)i + c];
          v[3 + c] += (double)tgt[3 * (size_t)i + c];
        }
      }
    }
    const int live = block_sum_i(islot, n);
    block_sum<6>(slot, v);
    if (live < 3) {
      st |= kStFew;
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        ca[c] = v[c] / (double)live;
        cb[c] = v[3 + c] / (double)live;
      }
    }
  }
  double mu = 0.0;
  if (st == 0) {
    double top = 0.0;
    bool nan = false;
    for (int i = tid; i < count; i += kThreads) {
      if (load_mult(mult + i) > 0) {
        const double a0 = (double)src[3 * (size_t)i] - ca[0], a1 = (double)src[3 * (size_t)i + 1] - ca[1],
                     a2 = (double)src[3 * (size_t)i + 2] - ca[2];
        const double b0 = (double)tgt[3 * (size_t)i] - cb[0], b1 = (double)tgt[3 * (size_t)i + 1] - cb[1],
                     b2 = (double)tgt[3 * (size_t)i + 2] - cb[2];
        const double da = (a0 * a0 + a1 * a1) + a2 * a2, db = (b0 * b0 + b1 * b1) + b2 * b2;
        nan = nan || !d3f::posegraph::finite_d(da) || !d3f::posegraph::finite_d(db);
        top = da > top ? da : top;
        top = db > top ? db : top;
      }
    }
    // the maximum is order-free; "some distance is not finite" travels as a count
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double other = d3f::shfl_xor_f64(top, o);
      top = other > top ? other : top;
    }
    const int bad = block_sum_i(islot, nan ? 1 : 0);
    __syncthreads();
    if (d3f::lane_id() == 0) slot[tid / D3F_WAVE][0] = top;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kWaves; ++w) top = slot[w][0] > top ? slot[w][0] : top;
    if (bad) st |= kStNonFinite;
    mu = top;
  }

  // ---- graduated non-convexity
  if (st == 0) {
    const double delta2 = a.delta * a.delta;
    for (int it = 0; it < a.iterations; ++it) {
      mu = anneal(mu, it, a.anneal_every, a.division_factor, delta2);
      double S[kSums];
#pragma unroll
      for (int k = 0; k < kSums; ++k) S[k] = 0.0;
      for (int i = tid; i < count; i += kThreads) {
        const int m = load_mult(mult + i);
        if (m > 0) {
          const float av[3] = {src[3 * (size_t)i], src[3 * (size_t)i + 1], src[3 * (size_t)i + 2]};
          const float bv[3] = {tgt[3 * (size_t)i], tgt[3 * (size_t)i + 1], tgt[3 * (size_t)i + 2]};
          add_row(av, bv, m, ca, cb, R, t, mu, S);
        }
      }
      block_sum<kSums>(slot, S);
      if (tid == 0) {   // one thread takes the step; the pose travels through LDS
        double d[6];
        const int rc = step(S, R, t, d);
        if (rc != kStepNonFinite) write_trace(a.trace, p, a.iterations, it, mu, S[0], d);
#pragma unroll
        for (int k = 0; k < 9; ++k) pose[k] = R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) pose[9 + k] = t[k];
        islot[0] = rc;
      }
      __syncthreads();
      const int rc = islot[0];
#pragma unroll
      for (int k = 0; k < 9; ++k) R[k] = pose[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) t[k] = pose[9 + k];
      if (rc == kStepNonFinite) {
        st |= kStNonFinite;
        break;
      }
      wsum = S[0];
      if (rc == kStepSingular) {
        st |= kStSingular;
        break;
      }
    }
  }

  // ---- result and recount
  double T[16];
  float rt[12];
  const bool keep = (st & (kStFew | kStSegment | kStNonFinite)) == 0;
  if (keep) {
    result(R, t, ca, cb, T, rt);
  } else {
    identity(T, rt);
    wsum = 0.0;
  }
  int inl = 0;
  if (keep) {
    const float tau = (float)a.delta, tau2 = tau * tau;
    int n = 0;
    for (int i = tid; i < count; i += kThreads)
      n += d3f::rigid::inlier_f32(rt, tgt[3 * (size_t)i], tgt[3 * (size_t)i + 1], tgt[3 * (size_t)i + 2],
                                  src[3 * (size_t)i], src[3 * (size_t)i + 1], src[3 * (size_t)i + 2], tau2) ? 1 : 0;
    inl = block_sum_i(islot, n);
  }
  if (a.multiplicity)
    for (int i = tid; i < count; i += kThreads) a.multiplicity[off + i] = load_mult(mult + i);
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 16; ++k) a.T[16 * (size_t)p + k] = T[k];
    a.inliers[p] = inl;
    a.tuples[p] = taken;
    a.weight_sum[p] = wsum;
    a.status[p] = st;
  }
}

// the rule on one CPU thread: pair p
void host_pair(const Params& a, int p) {
  int off, count;
  int st = pair_segment(a.seg, p, a.rows, off, count);
  const float* src = a.src + 3 * (size_t)off;
  const float* tgt = a.tgt + 3 * (size_t)off;
  const int trials = trials_of(a.tuple_trials, count);
  std::vector<int32_t> mult((size_t)count, trials == 0 ? 1 : 0);
  int taken = 0;
  if (st == 0 && trials > 0) {
    const uint64_t key = d3f::rigid::pair_key(a.seed, a.first_pair + p);
    for (int h = 0; h < trials; ++h) {
      int idx[3];
      if (!tuple_trial(a.src, a.tgt, off, count, key, h, a.tuple_scale, idx)) continue;
      for (int k = 0; k < 3; ++k) ++mult[idx[k]];
      ++taken;
      if (a.max_tuples > 0 && taken >= a.max_tuples) break;
    }
  }
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0}, ca[3] = {0, 0, 0}, cb[3] = {0, 0, 0};
  double wsum = 0.0, mu = 0.0;
  std::vector<double> part6((size_t)kWorkers * 6), part((size_t)kWorkers * kSums);
  if (st == 0) {
    int live = 0;
    for (int s = 0; s < kWorkers; ++s) {
      double* v = &part6[6 * (size_t)s];
      for (int c = 0; c < 6; ++c) v[c] = 0.0;
      for (int i = s; i < count; i += kWorkers)
        if (mult[i] > 0) {
          ++live;
          for (int c = 0; c < 3; ++c) {
            v[c] += (double)src[3 * (size_t)i + c];
            v[3 + c] += (double)tgt[3 * (size_t)i + c];
          }
        }
    }
    double v[6];
    tree_sum<6>((double(*)[6])part6.data(), v);
    if (live < 3) {
      st |= kStFew;
    } else {
      for (int c = 0; c < 3; ++c) {
        ca[c] = v[c] / (double)live;
        cb[c] = v[3 + c] / (double)live;
      }
    }
  }
  if (st == 0) {
    double top = 0.0;
    bool nan = false;
    for (int i = 0; i < count; ++i)
      if (mult[i] > 0) {
        const double a0 = (double)src[3 * (size_t)i] - ca[0], a1 = (double)src[3 * (size_t)i + 1] - ca[1],
                     a2 = (double)src[3 * (size_t)i + 2] - ca[2];
        const double b0 = (double)tgt[3 * (size_t)i] - cb[0], b1 = (double)tgt[3 * (size_t)i + 1] - cb[1],
                     b2 = (double)tgt[3 * (size_t)i + 2] - cb[2];
        const double da = (a0 * a0 + a1 * a1) + a2 * a2, db = (b0 * b0 + b1 * b1) + b2 * b2;
        nan = nan || !d3f::posegraph::finite_d(da) || !d3f::posegraph::finite_d(db);
        top = da > top ? da : top;
        top = db > top ? db : top;
      }
    if (nan) st |= kStNonFinite;
    mu = top;
  }
  if (st == 0) {
    const double delta2 = a.delta * a.delta;
    for (int it = 0; it < a.iterations; ++it) {
      mu = anneal(mu, it, a.anneal_every, a.division_factor, delta2);
      for (int s = 0; s < kWorkers; ++s) {
        double* S = &part[kSums * (size_t)s];
        for (int k = 0; k < kSums; ++k) S[k] = 0.0;
        for (int i = s; i < count; i += kWorkers)
          if (mult[i] > 0) add_row(src + 3 * (size_t)i, tgt + 3 * (size_t)i, mult[i], ca, cb, R, t, mu, S);
      }
      double S[kSums], d[6];
      tree_sum<kSums>((double(*)[kSums])part.data(), S);
      const int rc = step(S, R, t, d);
      if (rc == kStepNonFinite) {
        st |= kStNonFinite;
        break;
      }
      wsum = S[0];
      write_trace(a.trace, p, a.iterations, it, mu, wsum, d);
      if (rc == kStepSingular) {
        st |= kStSingular;
        break;
      }
    }
  }
  double T[16];
  float rt[12];
  const bool keep = (st & (kStFew | kStSegment | kStNonFinite)) == 0;
  int inl = 0;
  if (keep) {
    result(R, t, ca, cb, T, rt);
    const float tau = (float)a.delta, tau2 = tau * tau;
    for (int i = 0; i < count; ++i)
      inl += d3f::rigid::inlier_f32(rt, tgt[3 * (size_t)i], tgt[3 * (size_t)i + 1], tgt[3 * (size_t)i + 2],
                                    src[3 * (size_t)i], src[3 * (size_t)i + 1], src[3 * (size_t)i + 2], tau2) ? 1 : 0;
  } else {
    identity(T, rt);
    wsum = 0.0;
  }
  if (a.multiplicity)
    for (int i = 0; i < count; ++i) a.multiplicity[off + i] = mult[i];
  for (int k = 0; k < 16; ++k) a.T[16 * (size_t)p + k] = T[k];
  a.inliers[p] = inl;
  a.tuples[p] = taken;
  a.weight_sum[p] = wsum;
  a.status[p] = st;
}

// the argument checks both entries share
int prepare(const float* src, const float* tgt, int rows, const int32_t* seg, int P, int first_pair,
            double distance_threshold, int iterations, double division_factor, int anneal_every, double tuple_scale,
            int tuple_trials, int max_tuples, uint64_t seed, double* T, int32_t* inliers, int32_t* tuples,
            double* weight_sum, int32_t* status, int32_t* multiplicity, double* trace, Params& a) {
  if ((rows > 0 && (!src || !tgt)) || !seg || !T || !inliers || !tuples || !weight_sum || !status || rows < 0 || P < 1 ||
      P > D3F_FGR_MAX_PAIRS || first_pair < 0 || iterations < 1 || iterations > D3F_FGR_MAX_ITERS || anneal_every < 1 ||
      !(distance_threshold > 0.0) || !(distance_threshold < INFINITY) || !(division_factor > 1.0) ||
      !(division_factor < INFINITY) || !(tuple_scale > 0.0 && tuple_scale <= 1.0) || tuple_trials > D3F_FGR_MAX_TRIALS ||
      max_tuples < 0)
    return D3F_EINVAL;
  a = {src, tgt, rows, seg, first_pair, distance_threshold, iterations, division_factor, anneal_every, tuple_scale,
       tuple_trials, max_tuples, seed, T, inliers, tuples, weight_sum, status, multiplicity, trace, nullptr};
  return D3F_OK;
}

}  // namespace

extern "C" {

size_t d3f_fgr_rigid_ws_bytes(int rows) { return d3f::align_up(4 * (size_t)(rows > 0 ? rows : 1), 256); }

int d3f_fgr_rigid(const float* src, const float* tgt, int rows, const int32_t* seg, int P, int first_pair,
                  double distance_threshold, int iterations, double division_factor, int anneal_every,
                  double tuple_scale, int tuple_trials, int max_tuples, uint64_t seed, double* T, int32_t* inliers,
                  int32_t* tuples, double* weight_sum, int32_t* status, int32_t* multiplicity, double* trace, void* ws,
                  size_t ws_bytes, void* stream) {
  Params a;
  const int rc = prepare(src, tgt, rows, seg, P, first_pair, distance_threshold, iterations, division_factor,
                         anneal_every, tuple_scale, tuple_trials, max_tuples, seed, T, inliers, tuples, weight_sum,
                         status, multiplicity, trace, a);
  if (rc != D3F_OK) return rc;
  if (!ws) return D3F_EINVAL;
  if (ws_bytes < d3f_fgr_rigid_ws_bytes(rows)) return D3F_EWORKSPACE;
  a.mult = (int32_t*)ws;
  fgr_kernel<<<(unsigned)P, kThreads, 0, (hipStream_t)stream>>>(a);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_fgr_rigid_host(const float* src_host, const float* tgt_host, int rows, const int32_t* seg_host, int P,
                       int first_pair, double distance_threshold, int iterations, double division_factor,
                       int anneal_every, double tuple_scale, int tuple_trials, int max_tuples, uint64_t seed,
                       double* T_host, int32_t* inliers_host, int32_t* tuples_host, double* weight_sum_host,
                       int32_t* status_host, int32_t* multiplicity_host, double* trace_host) {
  Params a;
  const int rc = prepare(src_host, tgt_host, rows, seg_host, P, first_pair, distance_threshold, iterations,
                         division_factor, anneal_every, tuple_scale, tuple_trials, max_tuples, seed, T_host,
                         inliers_host, tuples_host, weight_sum_host, status_host, multiplicity_host, trace_host, a);
  if (rc != D3F_OK) return rc;
  for (int p = 0; p < P; ++p) host_pair(a, p);
  return D3F_OK;
}

}  // extern "C"
