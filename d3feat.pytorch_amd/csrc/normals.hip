// Surface normals of every point of the stacked clouds of one cell list -- what point-to-plane ICP (icp.hip) needs and
// the reference leaves to Open3D's estimate_normals on the CPU.  A radius search over the point's OWN cloud forms the
// covariance moments of its neighbourhood; the normal is the eigenvector of the smallest eigenvalue, turned towards a
// viewpoint.
//
// Order independence.  The fill order of a bucket is decided by atomics, so a floating-point sum over the neighbours
// would differ from run to run.  The moments are therefore INTEGERS (include/d3feat_hip.h): the f32 offset p_j - p_i is
// scaled by the power of two Q = 2^floor(log2(2^20 / radius)) and rounded to u, |u| <= 2^20, and n, sum u, sum u u^T
// are added in int64 (a product is below 2^40: 2^22 neighbours fit; one v_mad_i64_i32 per moment).  Integer addition
// commutes, so neither the lanes, the groups nor the bucket order can change them, and everything after them
// (plane.hpp) is a function of the moments alone.
//
// Work distribution.  A group of G lanes serves one query and walks its 27 cells as the pair search does
// (pair_search.hpp: cells dealt round robin, a lane's buckets side by side); every accepted candidate goes into the
// lane's own ten sums and the group is combined by a butterfly of log2 G exchanges.  The eigenproblem is ~2000 f64
// instructions against ~40 per candidate, so leaving it to one lane of G would idle the rest for most of the kernel: a
// wave serves 64 consecutive queries in G slices of 64 / G, lane l keeps the sums of slice l mod G, and then all 64
// lanes solve one eigenproblem each.  G = 8: a neighbourhood at twice the ICP distance holds ~100 points in ~15
// occupied cells, 8 lanes walk 3-4 cells each; ~110 VGPRs (two sets of ten int64 sums and four buckets in flight)
// leave 4 waves per SIMD.  No LDS and no barrier, so the workgroup is 256 lanes only to keep the tail of the grid fine.
//
// Colour gradients (d3f_color_gradients; the kernel instantiated with kColor) -- what coloured ICP needs per fixed
// point (color_icp.hpp has the rule).  The same neighbourhood, the same Q and u; only neighbours with a usable intensity
// count, and three more int64 sums ride along: sum u c with c = q_j - q_i the difference of the intensities quantised to
// 2^-20.  A neighbour's intensity is read through the input row the stored point carries in .w (as icp.hip reads
// normals); the query's own normal is an input.  All 13 moments are integers, so the argument above holds unchanged.
// The closed-form 2x2 solve takes the eigenproblem's place in the same "G slices, then all 64 lanes solve" structure.
#include "color_icp.hpp"
#include "pair_search.hpp"
#include "plane.hpp"

namespace {

using namespace d3f::cells;

constexpr int kBlock = 256;
constexpr int kG = 8;
constexpr int kMoments = 10;
constexpr int moments_of(bool color) { return color ? d3f::color::kGradientMoments : kMoments; }

struct NormalArgs {
  const float* points;
  const int32_t* cloud_start;
  const int32_t* placement;   // cell_list.hpp: 0 = one hashed table, 1 = per-cloud tables
  CellSearch S;
  float* normals;
  int32_t* count;
  int64_t* moments;
  int32_t* status;
  double Q;
  float view[3];
  int B, Ns, min_neighbors;
  const float* intensity;     // [Ns] (kColor)
  const float* nrm_in;        // [Ns,3] normals of the rows (kColor)
  float4* field;              // [Ns] (d, I) (kColor)
};

template <int G, bool kColor>
__global__ __launch_bounds__(kBlock) void normals_kernel(const NormalArgs A) {
  constexpr int kMoments = moments_of(kColor);
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
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    int b = 0, c0 = 0, cn = 0, cx = 0, cy = 0, cz = 0;
    [[maybe_unused]] int qi = 0;   // the query's quantised intensity (kColor)
    if constexpr (kColor) {   // a point without a usable intensity is not searched: count 0, zero moments
      const float own = ok ? A.intensity[i] : -1.0f;
      ok = d3f::color::usable(own);
      qi = ok ? (int)d3f::color::quantised(own) : 0;
    }
    if (ok) {
      px = A.points[3 * (size_t)i + 0];
      py = A.points[3 * (size_t)i + 1];
      pz = A.points[3 * (size_t)i + 2];
      b = prefix_find(A.cloud_start, 0, A.B, i);
      c0 = A.cloud_start[b];
      cn = A.cloud_start[b + 1] - c0;
      const bool in_x = query_cell(px, A.S.inv_cell, cx), in_y = query_cell(py, A.S.inv_cell, cy),
                 in_z = query_cell(pz, A.S.inv_cell, cz);
      if (!(in_x && in_y && in_z)) {   // the build did not store it either
        if (sub == 0) atomicOr(A.status, D3F_ST_CELL_RANGE);
        ok = false;
      }
    }
    uint64_t nk[kCells];
    int st[kCells], len[kCells], longest = 0;
    cell_headers<G>(A.S, ok, px, py, pz, cx, cy, cz, b, c0, cn, per_cloud, cell, reach, sub, nk, st, len);
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
        const float d2 = d3f::sqdist_exact(px, py, pz, sp[c].x, sp[c].y, sp[c].z);
        bool in = t < len[c] && kk[c] == nk[c] && d2 < A.S.r2;
        [[maybe_unused]] float nb = 0.0f;
        if constexpr (kColor) {
          if (in) {   // (.w of a stored point of an accepted cell is an input row below the live rows)
            nb = A.intensity[(size_t)(uint32_t)__float_as_int(sp[c].w)];
            in = d3f::color::usable(nb);
          }
        }
        if (in) {
          // |d| < radius (1 + 2^-23) and Q radius <= 2^20: the rounded product fits an int32 with room to spare
          const int ux = (int)rint((double)__fsub_rn(sp[c].x, px) * A.Q), uy = (int)rint((double)__fsub_rn(sp[c].y, py) * A.Q),
                    uz = (int)rint((double)__fsub_rn(sp[c].z, pz) * A.Q);
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
          if constexpr (kColor) {
            const int dq = (int)d3f::color::quantised(nb) - qi;
            acc[10] += (long long)ux * dq;
            acc[11] += (long long)uy * dq;
            acc[12] += (long long)uz * dq;
          }
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
  const bool row = i < live;
  const int n = row ? (int)keep[0] : 0;
  if constexpr (kColor) {
    const float nan = __builtin_nanf("");
    float out[4] = {nan, nan, nan, nan};
    if (row)
      d3f::color::gradient_from_moments(keep, A.Q, A.nrm_in[3 * (size_t)i + 0], A.nrm_in[3 * (size_t)i + 1],
                                        A.nrm_in[3 * (size_t)i + 2], A.intensity[i], A.min_neighbors, out);
    A.field[i] = make_float4(out[0], out[1], out[2], out[3]);
    if (A.count) A.count[i] = n;
  } else {
    float nx = 0.0f, ny = 0.0f, nz = 0.0f;
    if (row && n >= A.min_neighbors)
      d3f::plane::normal_from_moments(keep, A.Q, (double)A.view[0] - (double)A.points[3 * (size_t)i + 0],
                                      (double)A.view[1] - (double)A.points[3 * (size_t)i + 1],
                                      (double)A.view[2] - (double)A.points[3 * (size_t)i + 2], nx, ny, nz);
    A.normals[3 * (size_t)i + 0] = nx;
    A.normals[3 * (size_t)i + 1] = ny;
    A.normals[3 * (size_t)i + 2] = nz;
    A.count[i] = n;
  }
  if (A.moments) {
#pragma unroll
    for (int k = 0; k < kMoments; ++k) A.moments[kMoments * (size_t)i + k] = row ? keep[k] : 0;
  }
}

using d3f::plane::quantum_scale;

}  // namespace

extern "C" {

int d3f_estimate_normals(const void* grid_ws, const float* points, int Ns, const int32_t* cloud_start, int B,
                         float grid_radius, float radius, int min_neighbors, const float* viewpoint_host,
                         float* normals, int32_t* count, int64_t* moments, int32_t* status, void* stream_) {
  if (!grid_ws || !points || !cloud_start || !status || Ns < 0 || B < 1 || B > kMaxClouds || !(radius > 0.0f) ||
      !isfinite(radius) || !(grid_radius >= radius) || min_neighbors < 1 || (Ns > 0 && (!normals || !count)))
    return D3F_EINVAL;
  if (Ns == 0) return D3F_OK;
  NormalArgs a;
  a.points = points;
  a.cloud_start = cloud_start;
  a.S = cell_search(grid_ws, Ns, grid_radius, radius, &a.placement);
  a.normals = normals;
  a.count = count;
  a.moments = moments;
  a.status = status;
  a.Q = quantum_scale(radius);
  for (int k = 0; k < 3; ++k) a.view[k] = viewpoint_host ? viewpoint_host[k] : 0.0f;
  a.B = B;
  a.Ns = Ns;
  a.min_neighbors = min_neighbors;
  normals_kernel<kG, false><<<(unsigned)d3f::cdiv(Ns, kBlock), kBlock, 0, (hipStream_t)stream_>>>(a);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_color_gradients(const void* grid_ws, const float* points, int Ns, const int32_t* cloud_start, int B,
                        float grid_radius, float radius, int min_neighbors, const float* normals,
                        const float* intensity, float* field, int32_t* count, int64_t* moments, int32_t* status,
                        void* stream_) {
  if (!grid_ws || !points || !cloud_start || !status || Ns < 0 || B < 1 || B > kMaxClouds || !(radius > 0.0f) ||
      !isfinite(radius) || !(grid_radius >= radius) || min_neighbors < 1 ||
      (Ns > 0 && (!normals || !intensity || !field)))
    return D3F_EINVAL;
  if (Ns == 0) return D3F_OK;
  NormalArgs a = {};
  a.points = points;
  a.cloud_start = cloud_start;
  a.S = cell_search(grid_ws, Ns, grid_radius, radius, &a.placement);
  a.count = count;
  a.moments = moments;
  a.status = status;
  a.Q = quantum_scale(radius);
  a.B = B;
  a.Ns = Ns;
  a.min_neighbors = min_neighbors;
  a.intensity = intensity;
  a.nrm_in = normals;
  a.field = reinterpret_cast<float4*>(field);
  normals_kernel<kG, true><<<(unsigned)d3f::cdiv(Ns, kBlock), kBlock, 0, (hipStream_t)stream_>>>(a);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_color_gradient_from_moments_host(const int64_t* m_host, double Q, const float* nrm_host, float intensity,
                                         int min_neighbors, float* out_host) {
  if (!m_host || !nrm_host || !out_host || !(Q > 0.0) || min_neighbors < 1) return D3F_EINVAL;
  int64_t m[d3f::color::kGradientMoments];
  for (int k = 0; k < d3f::color::kGradientMoments; ++k) m[k] = m_host[k];
  float out[4];
  d3f::color::gradient_from_moments(m, Q, nrm_host[0], nrm_host[1], nrm_host[2], intensity, min_neighbors, out);
  for (int k = 0; k < 4; ++k) out_host[k] = out[k];
  return D3F_OK;
}

int d3f_normal_from_moments_host(const int64_t* m_host, double Q, const double* to_view_host, float* out_host) {
  if (!m_host || !to_view_host || !out_host || !(Q > 0.0)) return D3F_EINVAL;
  int64_t m[10];
  for (int k = 0; k < 10; ++k) m[k] = m_host[k];
  d3f::plane::normal_from_moments(m, Q, to_view_host[0], to_view_host[1], to_view_host[2], out_host[0], out_host[1],
                                  out_host[2]);
  return D3F_OK;
}

}  // extern "C"
