// FPFH descriptors (Rusu, Blodow, Beetz 2009, in the form Open3D's compute_fpfh_feature computes): the rule, stated
// once, for the two kernels (fpfh.hip), the host twin (d3f_fpfh_host) and the NumPy restatement
// (registration.fpfh_numpy).  include/d3feat_hip.h has the contract.  Everything here is __host__ __device__ and reads
// no state.  The arithmetic is f64 from the f32 inputs widened, only + - * / sqrt floor rint in exactly the order
// written; the library is built with -ffp-contract=off, so device, host twin and NumPy agree bit for bit.  No libm
// transcendental appears: their last bits differ between the three, and one such bit moves a count.
//
// Order independence (normals.hip has the argument): the fill order of a bucket is decided by atomics, so everything
// summed over neighbours is an INTEGER.  Integer addition commutes, so lanes, groups, bucket order, stacking and cell
// size cannot change a sum, and everything after the sums is a function of them alone.
//
// Neighbourhood of point i: the points j != i of the SAME cloud with
//   d2f = ((dx dx) + (dy dy)) + (dz dz) < radius * radius   in f32 without FMA (d3f::sqdist_exact; the f32 product, strict:
//         the acceptance of the other searches and of d3f_estimate_normals),
//   a usable normal (any component != 0), and
//   d2  = ((dx dx) + (dy dy)) + (dz dz) != 0                 in f64 from the widened coordinates, dp = p_j - p_i.
// A point whose own normal is (0, 0, 0) has no descriptor and is nobody's neighbour.  Both tests are symmetric in i and
// j, so j is a neighbour of i exactly when i is one of j.  n_i = the number of neighbours.
//
// Pair features of (i, j) (pair_bins):
//   dist = sqrt(d2), a1 = ((n_i.x dp.x + n_i.y dp.y) + n_i.z dp.z) / dist, a2 likewise with n_j.
//   |a1| < |a2| (Open3D's acos(|a1|) > acos(|a2|) without the acos): the points swap roles -- n1 = n_j, n2 = n_i,
//   dp = -dp, f3 = -a2; else n1 = n_i, n2 = n_j, f3 = a1.
//   v = dp x n1, |v| = sqrt((vx vx + vy vy) + vz vz).  |v| = 0: the three bins are 5 (Open3D's all-zero features).
//   Else v /= |v| per component, w = n1 x v, f2 = v . n2, y = w . n2, x = n1 . n2 (dot products summed left to right).
// Bins, 11 per feature:
//   f2, f3: t = floor((11 (f + 1)) 0.5); bin = 10 when t >= 10, (int) t when t >= 0, else 0.
//   theta = atan2(y, x) goes to the number of boundaries theta_b = -pi + 2 pi b / 11 (b = 1..10) it reaches, WITHOUT
//   atan2: with s_b = y cos(theta_b) - x sin(theta_b) (proportional to sin(theta - theta_b)), for y < 0 the bin is the
//   number of b <= 5 with s_b >= 0, else 5 + the number of b >= 6 with s_b >= 0; x = y = 0 is bin 5 (atan2's 0).  The
//   (cos, sin) of b = 1..5 are the constants below, those of b = 11 - k are (cos, -sin) of b = k.
// SPFH: c_i[33] int32 = the three histograms of i's neighbours as counts (theta, f2, f3; 11 bins each): one increment per
//   histogram per neighbour, so each histogram sums to n_i.
// FPFH: each neighbour j weighs
//   W_j = (int64) rint((2^32 min(r2 / d2, 2^12)) / n_j),   r2 = (double) radius * (double) radius,
//   S_i[b] = sum_j W_j c_j[b] in int64, tot_h = the sum of histogram h's 11 S (int64), and
//   desc_i[b] = f32((100 S_i[b]) / tot_h + (100 c_i[b]) / n_i) in f64 (integers converted to f64 first; the first term
//   is 0 when tot_h = 0).  n_i = 0 (or an unusable own normal): 33 zeros, count 0 -- the count tells the two apart from
//   a described point.
//   The cap 2^12 (a neighbour closer than radius / 64) is the one deliberate departure from Open3D, where a single
//   near-duplicate point dominates the whole descriptor.
// Unit rows (optional; what the matching kernel reads: matching.hip ranks by the inner product of UNIT rows, which for
//   them is the order of the L2 distance): q = the sum of the squares of the 33 f32 entries widened, added in f64 in
//   the order b = 0..32; unit_i[b] = f32((double) desc_i[b] / sqrt(q)).  A row of zeros stays a row of zeros.
// Overflow: c_j[b] <= n_j and r2 / d2 <= 2^12, so a term W_j c_j[b] is at most 2^44 + 1/2 n_j and kMaxNeighbors = 2^18
//   neighbours keep S and tot_h below 2^63.  A point with more neighbours than that sets D3F_ST_CAND_OVERFLOW in the
//   status word and gets 33 zeros (its count is still reported).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define D3F_HD __host__ __device__
#else
#define D3F_HD
#endif

namespace d3f {
namespace fpfh {

constexpr int kBins = 11, kHist = 3 * kBins;
constexpr int kRow = 36;                    // a row of the SPFH table: 33 counts, n, two zeros (16-byte aligned rows)
constexpr int kMaxNeighbors = 1 << 18;
constexpr double kWeightScale = 4294967296.0, kWeightCap = 4096.0;
// cos and sin of theta_b = -pi + 2 pi b / 11, b = 1..5
constexpr double kCos1 = -0.8412535328311811, kSin1 = -0.5406408174555978;
constexpr double kCos2 = -0.4154150130018863, kSin2 = -0.9096319953545184;
constexpr double kCos3 = 0.14231483827328512, kSin3 = -0.9898214418809327;
constexpr double kCos4 = 0.6548607339452851, kSin4 = -0.7557495743542583;
constexpr double kCos5 = 0.9594929736144975, kSin5 = -0.2817325568414295;

D3F_HD inline bool usable_normal(float x, float y, float z) { return x != 0.0f || y != 0.0f || z != 0.0f; }

// d2 of the rule, f64
D3F_HD inline double sqdist_f64(double dx, double dy, double dz) { return (dx * dx + dy * dy) + dz * dz; }

D3F_HD inline int feature_bin(double f) {
  const double t = floor((11.0 * (f + 1.0)) * 0.5);
  return t >= 10.0 ? 10 : (t >= 0.0 ? (int)t : 0);
}

D3F_HD inline int theta_bin(double y, double x) {
  if (x == 0.0 && y == 0.0) return 5;
  if (y < 0.0)
    return (int)(y * kCos1 - x * kSin1 >= 0.0) + (int)(y * kCos2 - x * kSin2 >= 0.0) +
           (int)(y * kCos3 - x * kSin3 >= 0.0) + (int)(y * kCos4 - x * kSin4 >= 0.0) +
           (int)(y * kCos5 - x * kSin5 >= 0.0);
  return 5 + (int)(y * kCos5 - x * -kSin5 >= 0.0) + (int)(y * kCos4 - x * -kSin4 >= 0.0) +
         (int)(y * kCos3 - x * -kSin3 >= 0.0) + (int)(y * kCos2 - x * -kSin2 >= 0.0) +
         (int)(y * kCos1 - x * -kSin1 >= 0.0);
}

// The three bins (each 0..10) of the pair (i, j): p = p_j - p_i (f64 from the f32 coordinates), d2 = sqdist_f64(p) != 0,
// ni and nj the widened normals.
D3F_HD inline void pair_bins(double px, double py, double pz, double d2, double nix, double niy, double niz, double njx,
                             double njy, double njz, int& b_theta, int& b_f2, int& b_f3) {
  const double dist = sqrt(d2);
  const double a1 = ((nix * px + niy * py) + niz * pz) / dist, a2 = ((njx * px + njy * py) + njz * pz) / dist;
  const bool swap = fabs(a1) < fabs(a2);
  const double n1x = swap ? njx : nix, n1y = swap ? njy : niy, n1z = swap ? njz : niz;
  const double n2x = swap ? nix : njx, n2y = swap ? niy : njy, n2z = swap ? niz : njz;
  const double qx = swap ? -px : px, qy = swap ? -py : py, qz = swap ? -pz : pz;
  const double f3 = swap ? -a2 : a1;
  double vx = qy * n1z - qz * n1y, vy = qz * n1x - qx * n1z, vz = qx * n1y - qy * n1x;
  const double vn = sqrt((vx * vx + vy * vy) + vz * vz);
  if (vn == 0.0) {
    b_theta = b_f2 = b_f3 = 5;
    return;
  }
  vx /= vn; vy /= vn; vz /= vn;
  const double wx = n1y * vz - n1z * vy, wy = n1z * vx - n1x * vz, wz = n1x * vy - n1y * vx;
  const double f2 = (vx * n2x + vy * n2y) + vz * n2z;
  const double y = (wx * n2x + wy * n2y) + wz * n2z, x = (n1x * n2x + n1y * n2y) + n1z * n2z;
  b_theta = theta_bin(y, x);
  b_f2 = feature_bin(f2);
  b_f3 = feature_bin(f3);
}

// W_j; n_j >= 1
D3F_HD inline int64_t neighbor_weight(double r2, double d2, int n_j) {
  const double ratio = r2 / d2;
  return (int64_t)rint((kWeightScale * (ratio < kWeightCap ? ratio : kWeightCap)) / (double)n_j);
}

// one entry of the descriptor: S = S_i[b], tot = tot_h of b's histogram, c = c_i[b], n = n_i >= 1
D3F_HD inline float descriptor_entry(int64_t S, int64_t tot, int c, int n) {
  const double first = tot == 0 ? 0.0 : (100.0 * (double)S) / (double)tot;
  return (float)(first + (100.0 * (double)c) / (double)n);
}

// one entry of the unit row: d = desc_i[b], q = the row's sum of squares > 0
D3F_HD inline float unit_entry(float d, double q) { return (float)((double)d / sqrt(q)); }

}  // namespace fpfh
}  // namespace d3f
