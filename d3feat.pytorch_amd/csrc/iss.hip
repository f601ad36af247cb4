// ISS keypoints of every point of the stacked clouds of one cell list, and radius non-maximum suppression of any score
// over the same list (iss.hpp has the rule, include/d3feat_hip.h the contract).  Two kernels, each one launch.
//
// iss_saliency_kernel is normals_kernel's walk (normals.hip: G = 8 lanes per query, the 27 cells dealt round robin by
// cell_headers<G>, ten int64 sums per lane, a butterfly, "G slices, then all 64 lanes solve") with
// iss::saliency_from_moments in place of the eigenvector solve: the moments are the same integers, so the saliency is
// a function of the neighbourhood alone -- bit-identical for any row order, stacking and cell size.  It is a sibling
// and not a third instantiation of that template, so normals.hip compiles to what it compiled to before.
//
// radius_nms_kernel gives each query one group of G lanes over the same cell walk.  A query whose score is not > 0
// (NaN included) walks nothing: with the gate and a sparse score that is most rows.  A neighbour's score is read
// through the input row the stored point carries in .w (as normals.hip reads intensities).  Each lane keeps a `beaten`
// bit and a count; the group combines them by OR and sum.  A beaten query KEEPS WALKING, so that count is the whole
// neighbourhood for every row that walks and the outputs are a pure function of (points, score, radius,
// min_neighbors).  No LDS, no atomics except the status word, no floating-point sums.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):
//   iss_saliency_kernel: 106 VGPRs, no scratch, no spill, no LDS, 4 waves per SIMD (normals_kernel's figures)
//   radius_nms_kernel:    56 VGPRs, no scratch, no spill, no LDS, 8 waves per SIMD
// Measured (profiles/iss_bench.txt: 1.45 M points, 122 neighbours each at 0.15 m, 57 at 0.10 m): the saliency pass takes
// 4.78 ms against 4.79 ms for normals_kernel over the same cells, measured in turns (0.998 x; two measurements of the
// normals arm differ by 0.0004) -- the walk is the cost, the solve after it is not; the suppression takes 2.86 ms on
// that saliency (95 % of the rows walk) and 2.91 ms when every row walks.
#include "iss.hpp"
#include "pair_search.hpp"

namespace {

using namespace d3f::cells;

constexpr int kBlock = 256;
constexpr int kG = 8;
constexpr int kMoments = 10;

struct IssArgs {
  const float* points;
  const int32_t* cloud_start;
  const int32_t* placement;   // cell_list.hpp: 0 = one hashed table, 1 = per-cloud tables
  CellSearch S;
  int32_t* status;
  int B, Ns, min_neighbors;
  // saliency pass
  float* saliency;            // [Ns]
  int32_t* count;             // [Ns]
  int64_t* moments;           // [Ns,10] or null
  double Q, gamma_21, gamma_32;
  // suppression pass
  const float* score;         // [Ns]
  uint8_t* keep;              // [Ns]
};

// the query of one group: its point, cloud and cell; ok is cleared for a point outside the addressable grid
struct Query {
  float px, py, pz;
  int b, c0, cn, cx, cy, cz;
};

__device__ __forceinline__ Query load_query(const IssArgs& A, long long i, bool& ok, int sub) {
  Query q = {0.0f, 0.0f, 0.0f, 0, 0, 0, 0, 0, 0};
  if (!ok) return q;
  q.px = A.points[3 * (size_t)i + 0];
  q.py = A.points[3 * (size_t)i + 1];
  q.pz = A.points[3 * (size_t)i + 2];
  q.b = prefix_find(A.cloud_start, 0, A.B, i);
  q.c0 = A.cloud_start[q.b];
  q.cn = A.cloud_start[q.b + 1] - q.c0;
  const bool in_x = query_cell(q.px, A.S.inv_cell, q.cx), in_y = query_cell(q.py, A.S.inv_cell, q.cy),
             in_z = query_cell(q.pz, A.S.inv_cell, q.cz);
  if (!(in_x && in_y && in_z)) {   // the build did not store it either
    if (sub == 0) atomicOr(A.status, D3F_ST_CELL_RANGE);
    ok = false;
  }
  return q;
}

template <int G>
__global__ __launch_bounds__(kBlock) void iss_saliency_kernel(const IssArgs A) {
  constexpr int kCells = (27 + G - 1) / G, kPerSlice = 64 / G;
  const int lane = threadIdx.x & 63, sub = lane & (G - 1);
  const long long base = ((long long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)) * 64;   // the wave's first query
  const int live = A.cloud_start[A.B] < A.Ns ? A.cloud_start[A.B] : A.Ns;   // Ns is a row capacity
  const bool per_cloud = *A.placement != 0;
  const double cell = 1.0 / A.S.inv_cell, reach = (double)A.S.prune_r * (1.0 + 1e-4);
  int64_t keep[kMoments];
#pragma unroll
  for (int k = 0; k < kMoments; ++k) keep[k] = 0;
  for (int slice = 0; slice < G; ++slice) {
    const long long i = base + slice * kPerSlice + lane / G;
    bool ok = i < live;
    const Query q = load_query(A, i, ok, sub);
    uint64_t nk[kCells];
    int st[kCells], len[kCells], longest = 0;
    cell_headers<G>(A.S, ok, q.px, q.py, q.pz, q.cx, q.cy, q.cz, q.b, q.c0, q.cn, per_cloud, cell, reach, sub, nk, st,
                    len);
#pragma unroll
    for (int c = 0; c < kCells; ++c) longest = len[c] > longest ? len[c] : longest;
    int64_t acc[kMoments];
#pragma unroll
    for (int k = 0; k < kMoments; ++k) acc[k] = 0;
    for (int t = 0; t < longest; ++t) {
      uint64_t kk[kCells];
      float4 sp[kCells];
#pragma unroll
      for (int c = 0; c < kCells; ++c) {
        const int pos = t < len[c] ? st[c] + t : 0;
        kk[c] = A.S.key[pos];
        sp[c] = A.S.pts[pos];
      }
#pragma unroll
      for (int c = 0; c < kCells; ++c) {
        const float d2 = d3f::sqdist_exact(q.px, q.py, q.pz, sp[c].x, sp[c].y, sp[c].z);
        if (t < len[c] && kk[c] == nk[c] && d2 < A.S.r2) {
          // |d| < radius (1 + 2^-23) and Q radius <= 2^20: the rounded product fits an int32 with room to spare
          const int ux = (int)rint((double)__fsub_rn(sp[c].x, q.px) * A.Q),
                    uy = (int)rint((double)__fsub_rn(sp[c].y, q.py) * A.Q),
                    uz = (int)rint((double)__fsub_rn(sp[c].z, q.pz) * A.Q);
          acc[0] += 1;
          acc[1] += ux;
          acc[2] += uy;
          acc[3] += uz;
          acc[4] += (long long)ux * ux;
          acc[5] += (long long)ux * uy;
          acc[6] += (long long)ux * uz;
          acc[7] += (long long)uy * uy;
          acc[8] += (long long)uy * uz;
          acc[9] += (long long)uz * uz;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kMoments; ++k) {
#pragma unroll
      for (int o = 1; o < G; o <<= 1) acc[k] += (int64_t)d3f::shfl_xor_u64((uint64_t)acc[k], o);
      if (sub == slice) keep[k] = acc[k];
    }
  }
  // lane l holds the moments of the query of slice l mod G, group l / G
  const long long i = base + sub * kPerSlice + lane / G;
  if (i >= A.Ns) return;
  const bool row = i < live;   // (a row outside the grid walked nothing: its moments are zeros)
  A.saliency[i] = row ? d3f::iss::saliency_from_moments(keep, A.Q, A.gamma_21, A.gamma_32, A.min_neighbors) : 0.0f;
  A.count[i] = row ? (int)keep[0] : 0;
  if (A.moments) {
#pragma unroll
    for (int k = 0; k < kMoments; ++k) A.moments[kMoments * (size_t)i + k] = row ? keep[k] : 0;
  }
}

template <int G>
__global__ __launch_bounds__(kBlock) void radius_nms_kernel(const IssArgs A) {
  constexpr int kCells = (27 + G - 1) / G;
  const int sub = threadIdx.x & (G - 1);
  const long long i = ((long long)blockIdx.x * kBlock + threadIdx.x) / G;   // the group's query
  const int live = A.cloud_start[A.B] < A.Ns ? A.cloud_start[A.B] : A.Ns;
  const bool per_cloud = *A.placement != 0;
  const double cell = 1.0 / A.S.inv_cell, reach = (double)A.S.prune_r * (1.0 + 1e-4);
  const float own = i < live ? A.score[i] : 0.0f;
  bool ok = own > 0.0f;   // false for a NaN: such a row is not searched
  const Query q = load_query(A, i, ok, sub);
  uint64_t nk[kCells];
  int st[kCells], len[kCells], longest = 0;
  cell_headers<G>(A.S, ok, q.px, q.py, q.pz, q.cx, q.cy, q.cz, q.b, q.c0, q.cn, per_cloud, cell, reach, sub, nk, st,
                  len);
#pragma unroll
  for (int c = 0; c < kCells; ++c) longest = len[c] > longest ? len[c] : longest;
  int beaten = 0, n = 0;
  for (int t = 0; t < longest; ++t) {
    uint64_t kk[kCells];
    float4 sp[kCells];
#pragma unroll
    for (int c = 0; c < kCells; ++c) {
      const int pos = t < len[c] ? st[c] + t : 0;
      kk[c] = A.S.key[pos];
      sp[c] = A.S.pts[pos];
    }
#pragma unroll
    for (int c = 0; c < kCells; ++c) {
      const float d2 = d3f::sqdist_exact(q.px, q.py, q.pz, sp[c].x, sp[c].y, sp[c].z);
      if (t < len[c] && kk[c] == nk[c] && d2 < A.S.r2) {
        // (.w of a stored point of an accepted cell is an input row below the live rows)
        n += 1;
        beaten |= A.score[(size_t)(uint32_t)__float_as_int(sp[c].w)] > own ? 1 : 0;   // a NaN beats nobody
      }
    }
  }
#pragma unroll
  for (int o = 1; o < G; o <<= 1) {
    beaten |= __shfl_xor(beaten, o, 64);
    n += __shfl_xor(n, o, 64);
  }
  if (sub != 0 || i >= A.Ns) return;
  A.keep[i] = ok && !beaten && n >= A.min_neighbors ? 1 : 0;
  A.count[i] = n;   // 0 for a row that did not walk
}

bool common_ok(const void* grid_ws, const float* points, int Ns, const int32_t* cloud_start, int B, float grid_radius,
               float radius, int min_neighbors, const int32_t* status) {
  return grid_ws && points && cloud_start && status && Ns >= 0 && B >= 1 && B <= kMaxClouds && radius > 0.0f &&
         isfinite(radius) && grid_radius >= radius && min_neighbors >= 1;
}

bool gamma_ok(double g) { return g > 0.0 && g <= 1.0; }

IssArgs common_args(const void* grid_ws, const float* points, int Ns, const int32_t* cloud_start, int B,
                    float grid_radius, float radius, int min_neighbors, int32_t* status) {
  IssArgs a = {};
  a.points = points;
  a.cloud_start = cloud_start;
  a.S = cell_search(grid_ws, Ns, grid_radius, radius, &a.placement);
  a.status = status;
  a.B = B;
  a.Ns = Ns;
  a.min_neighbors = min_neighbors;
  return a;
}

}  // namespace

extern "C" {

int d3f_iss_saliency(const void* grid_ws, const float* points, int Ns, const int32_t* cloud_start, int B,
                     float grid_radius, float radius, double gamma_21, double gamma_32, int min_neighbors,
                     float* saliency, int32_t* count, int64_t* moments, int32_t* status, void* stream_) {
  if (!common_ok(grid_ws, points, Ns, cloud_start, B, grid_radius, radius, min_neighbors, status) ||
      !gamma_ok(gamma_21) || !gamma_ok(gamma_32) || (Ns > 0 && (!saliency || !count)))
    return D3F_EINVAL;
  if (Ns == 0) return D3F_OK;
  IssArgs a = common_args(grid_ws, points, Ns, cloud_start, B, grid_radius, radius, min_neighbors, status);
  a.saliency = saliency;
  a.count = count;
  a.moments = moments;
  a.Q = d3f::plane::quantum_scale(radius);
  a.gamma_21 = gamma_21;
  a.gamma_32 = gamma_32;
  iss_saliency_kernel<kG><<<(unsigned)d3f::cdiv(Ns, kBlock), kBlock, 0, (hipStream_t)stream_>>>(a);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_radius_nms(const void* grid_ws, const float* points, int Ns, const int32_t* cloud_start, int B,
                   float grid_radius, float radius, const float* score, int min_neighbors, uint8_t* keep,
                   int32_t* count, int32_t* status, void* stream_) {
  if (!common_ok(grid_ws, points, Ns, cloud_start, B, grid_radius, radius, min_neighbors, status) ||
      (Ns > 0 && (!score || !keep || !count)))
    return D3F_EINVAL;
  if (Ns == 0) return D3F_OK;
  IssArgs a = common_args(grid_ws, points, Ns, cloud_start, B, grid_radius, radius, min_neighbors, status);
  a.score = score;
  a.keep = keep;
  a.count = count;
  radius_nms_kernel<kG><<<(unsigned)d3f::cdiv((long long)Ns * kG, kBlock), kBlock, 0, (hipStream_t)stream_>>>(a);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_iss_keypoints(const void* grid_ws, const float* points, int Ns, const int32_t* cloud_start, int B,
                      float grid_radius, float salient_radius, float non_max_radius, double gamma_21, double gamma_32,
                      int min_neighbors, float* saliency, uint8_t* keep, int32_t* count_salient, int32_t* count_nms,
                      int32_t* status, void* stream_) {
  const int rc = d3f_iss_saliency(grid_ws, points, Ns, cloud_start, B, grid_radius, salient_radius, gamma_21, gamma_32,
                                  min_neighbors, saliency, count_salient, nullptr, status, stream_);
  if (rc != D3F_OK) return rc;
  return d3f_radius_nms(grid_ws, points, Ns, cloud_start, B, grid_radius, non_max_radius, saliency, min_neighbors,
                        keep, count_nms, status, stream_);
}

int d3f_iss_saliency_from_moments_host(const int64_t* m_host, double Q, double gamma_21, double gamma_32,
                                       int min_neighbors, float* out_host) {
  if (!m_host || !out_host || !(Q > 0.0) || !gamma_ok(gamma_21) || !gamma_ok(gamma_32) || min_neighbors < 1)
    return D3F_EINVAL;
  int64_t m[kMoments];
  for (int k = 0; k < kMoments; ++k) m[k] = m_host[k];
  *out_host = d3f::iss::saliency_from_moments(m, Q, gamma_21, gamma_32, min_neighbors);
  return D3F_OK;
}

int d3f_radius_nms_host(const float* points, const float* score, int Ns, const int32_t* cloud_start, int B,
                        float radius, int min_neighbors, uint8_t* keep, int32_t* count) {
  if (!points || !cloud_start || Ns < 0 || B < 1 || B > kMaxClouds || !(radius > 0.0f) || !isfinite(radius) ||
      min_neighbors < 1 || (Ns > 0 && (!score || !keep || !count)))
    return D3F_EINVAL;
  for (int b = 0; b < B; ++b)
    if (cloud_start[b] < 0 || cloud_start[b + 1] < cloud_start[b] || cloud_start[b + 1] > Ns) return D3F_EINVAL;
  const float r2 = radius * radius;
  for (int i = 0; i < Ns; ++i) {
    keep[i] = 0;
    count[i] = 0;
  }
  for (int b = 0; b < B; ++b) {
    const int c0 = cloud_start[b], c1 = cloud_start[b + 1];
    for (int i = c0; i < c1; ++i) {
      const float own = score[i];
      if (!(own > 0.0f)) continue;
      const float* p = points + 3 * (size_t)i;
      bool beaten = false;
      int n = 0;
      for (int j = c0; j < c1; ++j) {
        const float* s = points + 3 * (size_t)j;
        if (!(d3f::iss::sqdist_f32(p[0], p[1], p[2], s[0], s[1], s[2]) < r2)) continue;
        n += 1;
        beaten = beaten || score[j] > own;
      }
      keep[i] = !beaten && n >= min_neighbors ? 1 : 0;
      count[i] = n;
    }
  }
  return D3F_OK;
}

}  // extern "C"
