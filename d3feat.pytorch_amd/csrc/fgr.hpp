// Fast global registration (Zhou, Park, Koltun, ECCV 2016) of one correspondence set: the rule that the kernel
// (fgr.hip; d3f_fgr_rigid) and its host twin (d3f_fgr_rigid_host) share.  Everything here is __host__ __device__, reads
// no state and is double precision.  Inputs and convention are d3f_ransac_rigid's: src / tgt [rows,3] f32, pair p owns
// the rows seg[p] = (offset, count), and the result maps the TARGET onto the SOURCE, src ~ R tgt + t.  Below a_i is
// the pair's source row i and b_i its target row i, both as the exact f64 images of the f32 inputs.
//
// Tuple test (Open3D's "tuple constraint" with this project's sampler).  K_p = rigid::pair_key(seed, first_pair + p).
// For h = 0 .. trials - 1 the indices i_k = rigid::draw(K_p, h, k, count), k = 0, 1, 2, PASS when they are distinct and
// rigid::triple_ok(a_i, b_i, tuple_scale) holds (both triangles non-degenerate, every edge
// min(la2, lb2) >= tuple_scale^2 max(la2, lb2)).  Only the first max_tuples passing h, in order of h, count
// (max_tuples = 0: all of them); every counted triple adds 1 to the integer multiplicity m_i of its three
// correspondences -- Open3D's duplicated correspondence list, held as counts.  trials = tuple_trials when that is
// >= 0, and Open3D's min(100 count, D3F_FGR_MAX_TRIALS) when it is negative; trials = 0 turns the test off: m_i = 1.
// Fewer than 3 correspondences with m_i > 0 (the LIVE ones): D3F_FGR_ST_FEW.
//
// Centring.  c_a, c_b = the f64 means of a_i, b_i over the live rows (each counted once, whatever m_i);
// D2 = the largest of |a_i - c_a|^2 and |b_i - c_b|^2 over them.  The loop works on a'_i = a_i - c_a, b'_i = b_i - c_b:
// no rescaling, everything stays in metres.
//
// Annealing.  mu = D2 at the start.  Before iteration `it`, when it % anneal_every == 0 and mu > delta^2:
// mu = max(mu / division_factor, delta^2), delta = distance_threshold.  (Open3D normalises the scene to unit size,
// compares mu with the UNSQUARED normalised distance and does not clamp; here mu is a squared distance in metres
// throughout and stops at delta^2.)  The default 128 iterations with anneal_every = 4 and division_factor = 1.4 bring a
// 3 m scene down to delta = 0.05: D2 / delta^2 = 9 / 0.0025 = 3600 = 1.4^24.3, so 25 divisions, the last before
// iteration 96, and 32 iterations at mu = delta^2.
//
// Iteration, with the current (R, t) (identity and zero at the start):
//   q_i = R b'_i + t,  r_i = a'_i - q_i,  w_i = m_i (mu / (|r_i|^2 + mu))^2            (live rows only)
//   a step (omega, v) moves q by omega x q + v, so J_i = [[q_i]x, -I] (3x6) and the normal equations are
//   (sum w J^T J) (omega, v) = -sum w J^T r.  Of their 21 + 6 sums only 16 are different numbers; those are added:
//     S[0] = sum w,  S[1..3] = sum w q,  S[4..9] = sum w (qx qx, qx qy, qx qz, qy qy, qy qz, qz qz),
//     S[10..12] = sum w (r x q),  S[13..15] = sum w r
//   sum w J^T J = [[ (tr Q) I - Q, [s]x ], [ [s]x^T, S[0] I ]]  with Q = sum w q q^T, s = sum w q;
//   sum w J^T r = ( S[10..12], -S[13..15] ).
//   Solve with plane::solve6 (Cholesky, pivot threshold kPlanePivot).  A pivot below it stops the pair where it is:
//   D3F_FGR_ST_SINGULAR, the pose of the iterations before stays.  A sum that is not finite (or c_a, c_b, D2):
//   D3F_FGR_ST_NONFINITE and the identity.
//   Update with the exact exponential:  E = so3_exp(omega);  R <- E R,  t <- E t + v.
// There is no early exit on convergence: fixed counts keep the launch shape static and a pair's result independent of
// the batch it is in.
//
// Result.  T = [R, c_a + t - R c_b] as a row-major 4x4; inliers = the number of ALL the pair's correspondences, whatever
// their m_i, that pass rigid::inlier_f32 at (float)delta squared in f32 under the f32 image of T (the number
// d3f_ransac_rigid reports); tuples = the counted triples; weight_sum = S[0] of the last iteration that was summed.
// D3F_FGR_ST_SEGMENT: as for RANSAC.  FEW, SEGMENT or NONFINITE: T is the identity and inliers is 0.
//
// Summation order.  Worker s of kWorkers = 256 adds its rows s, s + 256, ... in ascending order (the rows that are not
// live add nothing); the 256 partials are then summed by the fixed tree of tree_sum below: within each group of 64 the
// butterfly p[i] += p[i + o] for o = 1, 2, 4, .. 32 (i a multiple of 2 o), then the four group totals in order,
// ((g0 + g1) + g2) + g3.  The kernel's wave butterfly (d3f::wave_sum_f64) is that tree; the host twin runs tree_sum.
#pragma once
#include <math.h>
#include <stdint.h>

#include "plane.hpp"
#include "posegraph.hpp"
#include "rigid.hpp"

namespace d3f {
namespace fgr {

constexpr int kWorkers = 256;
constexpr int kSums = 16;
constexpr int kStFew = 1, kStSingular = 2, kStSegment = 4, kStNonFinite = 8;   // D3F_FGR_ST_*
constexpr int kMaxTrials = 1 << 22;                                            // D3F_FGR_MAX_TRIALS

D3F_HD inline int trials_of(int tuple_trials, int count) {
  if (tuple_trials >= 0) return tuple_trials < kMaxTrials ? tuple_trials : kMaxTrials;
  const long long t = 100ll * count;
  return t < kMaxTrials ? (int)t : kMaxTrials;
}

// trial h of a pair: the three drawn indices and whether the triple passes
D3F_HD inline bool tuple_trial(const float* src, const float* tgt, int off, int count, uint64_t key, int h,
                               double tuple_scale, int idx[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) idx[k] = rigid::draw(key, h, k, count);
  if (idx[0] == idx[1] || idx[0] == idx[2] || idx[1] == idx[2]) return false;
  double s[9], g[9];
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      s[3 * k + a] = (double)src[3 * (size_t)(off + idx[k]) + a];
      g[3 * k + a] = (double)tgt[3 * (size_t)(off + idx[k]) + a];
    }
  return rigid::triple_ok(s, g, tuple_scale);
}

// mu before iteration `it`
D3F_HD inline double anneal(double mu, int it, int anneal_every, double division_factor, double delta2) {
  if (it % anneal_every == 0 && mu > delta2) {
    mu = mu / division_factor;
    if (!(mu > delta2)) mu = delta2;
  }
  return mu;
}

// one live row's terms added to S[kSums]; a, b the row's f32 coordinates, m > 0 its multiplicity
D3F_HD inline void add_row(const float a[3], const float b[3], int m, const double ca[3], const double cb[3],
                           const double R[9], const double t[3], double mu, double S[kSums]) {
  const double b0 = (double)b[0] - cb[0], b1 = (double)b[1] - cb[1], b2 = (double)b[2] - cb[2];
  const double qx = ((R[0] * b0 + R[1] * b1) + R[2] * b2) + t[0];
  const double qy = ((R[3] * b0 + R[4] * b1) + R[5] * b2) + t[1];
  const double qz = ((R[6] * b0 + R[7] * b1) + R[8] * b2) + t[2];
  const double rx = ((double)a[0] - ca[0]) - qx, ry = ((double)a[1] - ca[1]) - qy, rz = ((double)a[2] - ca[2]) - qz;
  const double e = mu / (((rx * rx + ry * ry) + rz * rz) + mu);
  const double w = (double)m * (e * e);
  S[0] += w;
  S[1] += w * qx; S[2] += w * qy; S[3] += w * qz;
  S[4] += w * (qx * qx); S[5] += w * (qx * qy); S[6] += w * (qx * qz);
  S[7] += w * (qy * qy); S[8] += w * (qy * qz); S[9] += w * (qz * qz);
  S[10] += w * (ry * qz - rz * qy); S[11] += w * (rz * qx - rx * qz); S[12] += w * (rx * qy - ry * qx);
  S[13] += w * rx; S[14] += w * ry; S[15] += w * rz;
}

// the fixed tree over the kWorkers partials p[s][k] of N sums -> out[k]
template <int N>
inline void tree_sum(double (*p)[N], double out[N]) {
  for (int g = 0; g < kWorkers; g += 64)
    for (int o = 1; o < 64; o <<= 1)
      for (int i = 0; i < 64; i += 2 * o)
        for (int k = 0; k < N; ++k) p[g + i][k] += p[g + i + o][k];
  for (int k = 0; k < N; ++k) out[k] = ((p[0][k] + p[64][k]) + p[128][k]) + p[192][k];
}

constexpr int kStepOk = 0, kStepSingular = 1, kStepNonFinite = 2;

// the totals S -> the step d = (omega, v) and the updated (R, t); on kStepSingular / kStepNonFinite (R, t) stay
D3F_HD inline int step(const double S[kSums], double R[9], double t[3], double d[6]) {
#pragma unroll
  for (int k = 0; k < 6; ++k) d[k] = 0.0;
  bool fin = true;
#pragma unroll
  for (int k = 0; k < kSums; ++k) fin = fin && posegraph::finite_d(S[k]);
  if (!fin) return kStepNonFinite;
  const double A[21] = {S[7] + S[9], -S[5], -S[6], 0.0, -S[3], S[2],
                        S[4] + S[9], -S[8], S[3], 0.0, -S[1],
                        S[4] + S[7], -S[2], S[1], 0.0,
                        S[0], 0.0, 0.0,
                        S[0], 0.0,
                        S[0]};
  const double b[6] = {S[10], S[11], S[12], -S[13], -S[14], -S[15]};
  if (!plane::solve6(A, b, d)) {
#pragma unroll
    for (int k = 0; k < 6; ++k) d[k] = 0.0;
    return kStepSingular;
  }
  double E[9], Rn[9], tn[3];
  posegraph::so3_exp(d, E);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) Rn[3 * r + c] = (E[3 * r] * R[c] + E[3 * r + 1] * R[3 + c]) + E[3 * r + 2] * R[6 + c];
    tn[r] = ((E[3 * r] * t[0] + E[3 * r + 1] * t[1]) + E[3 * r + 2] * t[2]) + d[3 + r];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = Rn[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = tn[k];
  return kStepOk;
}

// T [16] = [R, c_a + t - R c_b] and its f32 image rt[12] (R row-major, then t) for the inlier count
D3F_HD inline void result(const double R[9], const double t[3], const double ca[3], const double cb[3], double T[16],
                          float rt[12]) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double tf = (ca[r] + t[r]) - ((R[3 * r] * cb[0] + R[3 * r + 1] * cb[1]) + R[3 * r + 2] * cb[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      T[4 * r + c] = R[3 * r + c];
      rt[3 * r + c] = (float)R[3 * r + c];
    }
    T[4 * r + 3] = tf;
    rt[9 + r] = (float)tf;
  }
  T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
}

D3F_HD inline void identity(double T[16], float rt[12]) {
  const double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, z[3] = {0, 0, 0};
  result(R, z, z, z, T, rt);
}

}  // namespace fgr
}  // namespace d3f
