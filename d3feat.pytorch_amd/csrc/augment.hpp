// Training-item augmentation shared by the device kernels (augment.hip) and their host twin (d3f_augment_item_host).
// Everything here is __host__ __device__ and reads no state, so a test can restate it bit for bit on the CPU
// (datasets.ThreeDMatch.augment_items_numpy).  The only generator is splitmix64 of rigid.hpp.
//
// An item has a 64-bit key K.  Stream s (small integer) and index i (uint32) give
//   z(s, i) = splitmix64(K ^ ((uint64(s) << 32) | i))          distinct (s, i) -> distinct z: splitmix64 is a bijection
//   u(s, i) = double(z >> 11) * 2^-53                          in [0, 1), exact in f64
// Streams: 1..3 noise of the source cloud's x, y, z; 4..6 noise of the target cloud's x, y, z; 7 the sort keys of the
// correspondence sample (the k rows j of the pair's table with the smallest z(7, j), ascending).
//
// Points, all f64 in exactly this order (the library is built with -ffp-contract=off: nothing is fused), rounded to f32
// once at the end:
//   source  out_a = float(double(p_a) + u(1 + a, i) * noise)
//   target  q_a   = ((R[a][0] * x + R[a][1] * y) + R[a][2] * z) + t[a];   out_a = float(q_a + u(4 + a, i) * noise)
// Keypoint distance between two augmented f32 source points: d2 = (dx * dx + dy * dy) + dz * dz in f64, sqrt(d2).
#pragma once
#include "rigid.hpp"

namespace d3f {
namespace augment {

constexpr int kStreamSrc = 1, kStreamTgt = 4, kStreamSelect = 7;

D3F_HD inline uint64_t z_of(uint64_t key, int stream, uint32_t i) {
  return d3f::rigid::splitmix64(key ^ (((uint64_t)(uint32_t)stream << 32) | (uint64_t)i));
}

D3F_HD inline double u_of(uint64_t key, int stream, uint32_t i) {
  return (double)(z_of(key, stream, i) >> 11) * 0x1.0p-53;
}

// coordinate a of augmented source point i; p = the point's 3 floats
D3F_HD inline float source_coord(const float* p, uint64_t key, int a, uint32_t i, double noise) {
  const double n = u_of(key, kStreamSrc + a, i) * noise;
  return (float)((double)p[a] + n);
}

// coordinate a of augmented target point i; R row-major [9], t [3]
D3F_HD inline float target_coord(const float* p, const double* R, const double* t, uint64_t key, int a, uint32_t i,
                                 double noise) {
  const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
  const double rx = R[3 * a] * x, ry = R[3 * a + 1] * y, rz = R[3 * a + 2] * z;
  const double q = ((rx + ry) + rz) + t[a];
  const double n = u_of(key, kStreamTgt + a, i) * noise;
  return (float)(q + n);
}

D3F_HD inline double dist2(const float* a, const float* b) {
  const double dx = (double)a[0] - (double)b[0], dy = (double)a[1] - (double)b[1], dz = (double)a[2] - (double)b[2];
  const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
  return (xx + yy) + zz;
}

// a source row index of the correspondence table, kept inside the cloud (the dataset validates its tables once; the
// clamp only keeps a bad table from reading outside the store)
D3F_HD inline uint32_t clamp_row(int32_t r, int32_t len) { return r < 0 ? 0u : (r >= len ? (uint32_t)(len - 1) : (uint32_t)r); }

}  // namespace augment
}  // namespace d3f
