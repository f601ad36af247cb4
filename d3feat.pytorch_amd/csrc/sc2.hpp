// Spatial compatibility of second order -- the rule of d3f_sc2_rigid (sc2.hip) and of its host twin, written once.
// Everything here is __host__ __device__, f64 and integer, and reads no state, so a test can restate it bit for bit.
// After Chen, Sun, Ren, Tai: "SC^2-PCR: A Second Order Spatial Compatibility for Efficient and Robust Point Cloud
// Registration", CVPR 2022.  Two correspondences are compatible when they preserve the distance between their points;
// inliers are compatible with each other AND with the same third parties, outliers only by chance.  There is no
// sampling and no seed: after one f64 test per pair of correspondences everything is integer (bit rows, AND, popcount).
//
// Pair of n correspondences, a_i / b_i the source / target row i as exact f64 images of the f32 inputs.
// 1. Compatibility, without a square root.  For i != j:  A = ((dx dx + dy dy) + dz dz) of a_i - a_j, B the same of
//    b_i - b_j,  s = (A + B) - tau^2,  C_ij = (s < 0) || (s s < 4 (A B));  C_ii = 0.  That is
//    | |a_i - a_j| - |b_i - b_j| | < tau  squared twice; only + - * in f64 (no contraction), so device, host and NumPy
//    set the same bits.  A non-finite coordinate fails both comparisons: its row and column are empty.
//    Row i is W = ceil(max_count / 64) 64-bit words; bit l of word w is j = 64 w + l; bits j >= n and rows i >= n are 0.
// 2. Seeds.  d_i = popcount(row i).  Seed rank orders the rows by descending d_i, ties to the lower i; the first
//    S = min(num_seeds, n) ranks are seeds.  A seed with d_i < 2 gives no hypothesis (its set has fewer than 3 points).
// 3. Consensus set of seed i.  For every j with C_ij = 1:  s_ij = popcount(row_i & row_j).  The set is i, then the
//    min(set_size - 1, d_i) candidates by descending s_ij, ties to the lower j, in that order.
// 4. Hypothesis.  rigid::fit over the set in that order; its f32 image is scored over ALL n rows with
//    rigid::inlier_f32 at tau_d^2, tau_d = (float)distance_threshold.
// 5. Winner.  The largest count, ties to the lowest seed rank.  No valid seed: kStNoHypothesis, identity, inliers 0.
// 6. Refinement.  rigid::refine of rigid_refine.hpp, RANSAC's, from the winner's f64 (R, t).
//
// Differences from the paper, on purpose:
//   - seeds come from the integer degree; the paper takes the leading eigenvector of the second-order matrix and
//     non-maximum suppression;
//   - one selection stage and an unweighted fit; the paper has two stages and spectral weights;
//   - no sampling anywhere;
//   - the authors' code was not at hand to compare with.
#pragma once
#include "rigid.hpp"

namespace d3f {
namespace sc2 {

constexpr int kStFew = 1, kStNoHypothesis = 2, kStSegment = 4;   // D3F_SC2_ST_*
constexpr int kMaxCount = 8192, kMaxSet = 64, kMaxSeeds = 4096;  // D3F_SC2_MAX_*
constexpr int kMaxWords = kMaxCount / 64;

D3F_HD inline int words_of(int max_count) { return (max_count + 63) >> 6; }

// (offset, count) of pair p and its status bits; count = 0 when the segment cannot be addressed
D3F_HD inline int pair_segment(const int32_t* seg, int p, int rows, int max_count, int& off, int& count) {
  off = seg[2 * p];
  count = seg[2 * p + 1];
  if (off < 0 || count < 0 || count > max_count || (long long)off + count > rows) {
    off = 0;
    count = 0;
    return kStSegment;
  }
  return count < 3 ? kStFew : 0;
}

D3F_HD inline double dist2(const double* a, const double* b) {
  const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  return (dx * dx + dy * dy) + dz * dz;
}

// rule 1 from the two squared distances
D3F_HD inline bool compatible(double A, double B, double tau2) {
  const double s = (A + B) - tau2;
  return (s < 0.0) || (s * s < 4.0 * (A * B));
}

// rule 2: row j (degree dj) ranks before row i (degree di)
D3F_HD inline bool seed_before(int dj, int j, int di, int i) { return dj > di || (dj == di && j < i); }

// rule 3 as one unsigned key per candidate: larger s first, then the lower j; 0 is "no candidate"
D3F_HD inline uint32_t candidate_key(int s, int j) { return ((uint32_t)(s + 1) << 13) | (uint32_t)(kMaxCount - 1 - j); }
D3F_HD inline int candidate_of(uint32_t key) { return kMaxCount - 1 - (int)(key & (uint32_t)(kMaxCount - 1)); }

// rule 5 as one key per seed rank: larger count first, then the lower rank; 0 is "no hypothesis"
D3F_HD inline unsigned long long hypothesis_key(int count, int rank) {
  return ((unsigned long long)(uint32_t)(count + 1) << 32) | (unsigned long long)(uint32_t)~(uint32_t)rank;
}

}  // namespace sc2
}  // namespace d3f
