// k-nearest descriptor matching -- the rule of d3f_knn_match (knn_match.hip), and what it shares with the mutual
// nearest neighbour of matching.hip: the distance of a product, its order-preserving bits and the split of the target
// range over workgroups.  registration.knn_match_numpy restates the rule in NumPy.
//
// Source descriptors S [Ns,C], target descriptors T [Nt,C], f32, C in {16, 32, 64, 128}, 1 <= k <= D3F_KNN_MAX:
//
//   a    = S @ T.T                            f32: the product bits of matching.hip's v_mfma_f32_16x16x4_f32 chain
//   d    = sqrt(f32(2) - f32(2) * a)          f32, correctly rounded; NaN where 2 - 2a < 0 (and where a is NaN)
//   key  = where(isnan(d), -inf, d)
//   idx  = argsort(key, axis=1, kind='stable')[:, :k]       ascending (key, column): NaN first, like np.argmin
//   dist = take_along_axis(d, idx, 1)
//
//   - slots s >= Nt hold idx = -1, dist = +inf;
//   - neighbours rank on the ROUNDED distance: two different products that round to one distance keep column order;
//   - the column is part of the key, so the keys of a row are distinct and the result is a function of the product
//     bits alone: the same for any split of the columns over workgroups, any merge order, alone or batched, from run
//     to run.  No floating-point atomic is used (no atomic at all);
//   - slot 0 is the row arg-min of d3f_mutual_nn on the same descriptors: both kernels form a (row, column) product by
//     the same instruction sequence and rank it by dist_of() below.  The one exception is a NaN product, which the
//     mutual kernel's row side never admits and this rule ranks first.
//
// What makes the filter exact.  v = fma(-2, a, 2) does not increase with a, and the correctly rounded root does not
// decrease with v, so  a_new <= a_e  implies  d_new >= d_e.  A lane that holds k candidates of a row, the k-th with
// product a_k, may therefore drop -- by one compare on the raw product, without a margin -- every LATER column with
// a <= a_k: it ranks behind all k of them (a later column loses an equal distance).  The largest a_k among the 16
// lanes of a row does the same for all of them once their columns lie behind.
#pragma once
#include "common.hpp"

namespace d3f {
namespace match {

constexpr int kColsPerTile = 64;

__device__ __forceinline__ uint32_t ord_bits(float f) {  // monotone float -> uint32
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// The correctly rounded square root of v = 2 - 2a, the reference's np.sqrt.  __fsqrt_rn is NOT that: the HIP headers map
// it to the native v_sqrt_f32 (1 ulp), which tells apart products that np.sqrt rounds to ONE distance -- the later,
// larger product then wins where np.argmin keeps the earlier index.  v_sqrt_f32 is within 1 ulp, so the residuals of its
// two neighbours decide: the compiler's own expansion of sqrtf, without the denormal scaling and class checks (v is 0
// or at least 2^-23; +inf, the "no candidate yet" value, comes back as +inf).  sqrtf itself costs 0.497 against 0.470 ms
// at 19k x 19k x 32 with everything else equal: the root sits on the column side's dependent chain of every 16 columns.
__device__ __forceinline__ float sqrt_rn(float v) {
  float s = __builtin_amdgcn_sqrtf(v);
  const float sd = __uint_as_float(__float_as_uint(s) - 1u), su = __uint_as_float(__float_as_uint(s) + 1u);
  const float rd = fmaf(-sd, s, v), ru = fmaf(-su, s, v);
  s = rd <= 0.0f ? sd : s;
  return ru > 0.0f ? su : s;
}
// the reference's distance; a negative v (its NaN) ranks below every distance
__device__ __forceinline__ float dist_of(float v) { return v < 0.0f ? -INFINITY : sqrt_rn(v); }

// workgroups along the target range: ~2048 in all (8 per CU), column chunks of whole tiles that fit the LDS table
static inline void chunking(int gx, int Nt, int& chunks, int& cpc) {
  const int target = d3f::tunables().match_wgs > 0 ? d3f::tunables().match_wgs : 2048;
  chunks = target / (gx > 0 ? gx : 1);
  const int max_chunks = d3f::cdiv(Nt, 4 * kColsPerTile);
  if (chunks > max_chunks) chunks = max_chunks;
  const int min_chunks = d3f::cdiv(Nt, 4096);   // 32 KB of keys per workgroup at most
  if (chunks < min_chunks) chunks = min_chunks;
  if (chunks < 1) chunks = 1;
  cpc = d3f::cdiv(Nt, chunks);
  cpc = d3f::cdiv(cpc, kColsPerTile) * kColsPerTile;
  chunks = d3f::cdiv(Nt, cpc);
}

}  // namespace match
}  // namespace d3f
