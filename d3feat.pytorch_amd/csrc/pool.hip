// Neighbor max-pool and nearest ("closest") pool, forward + backward.
//
// Replaces reference models/blocks.py:94-110 (max_pool: cat zero shadow row, gather [n2,H,d], torch.max over H)
// and :79-91 (closest_pool: gather column 0).  The reference materialises the gathered [n2,H,d] tensor; here a
// thread owns one (query, 4 channels) group (one channel when C % 4 != 0); consecutive lanes own consecutive channel
// groups, so every neighbor row is read as coalesced 16-B loads and the neighbor index is (nearly) wave-uniform.
// The 4-channel max-pool forward goes further: its rows belong to waves, which read each index row once and keep the
// gathers of 8 neighbors in flight (max_pool_fwd_v4_kernel).
// Element indices are 32-bit whenever the matrices have fewer than 2^31 elements: a 64-bit division by a run-time C per
// thread costs more than the loads of these kernels (closest_pool forward at 38k x 128: 47 -> 15 us).
#include "common.hpp"

namespace {

// argmax convention: first maximal neighbor in row order, like torch.max(dim=1) on CPU/ROCm.
// `clear` (optional, Ns*C floats): the scatter target of the backward pass, zeroed here on the side so that the
// backward needs no fill launch of its own.
__global__ void max_pool_fwd_kernel(const float* __restrict__ x, int Ns, int C, const int32_t* __restrict__ idx,
                                    int Nq, int H, float* __restrict__ out, int32_t* __restrict__ argmax,
                                    float* __restrict__ clear, const int32_t* __restrict__ width, d3f::RowGroups rg) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (clear)
    for (size_t i = t; i < (size_t)Ns * C; i += (size_t)gridDim.x * blockDim.x) clear[i] = 0.0f;
  if (t >= (size_t)Nq * C) return;
  const int n = (int)(t / C), c = (int)(t % C);
  if (rg.len) {  // stacked pairs: every group of clouds has the width of the table its own batch would have had
    const int Hg = width ? min(H, max(1, width[d3f::group_of_row(rg, n)])) : H;
    const int32_t* grow = idx + (size_t)n * H;
    float gbest = -INFINITY;
    int garg = Ns;
    for (int h = 0; h < Hg; ++h) {
      const int m = grow[h];
      const bool real = m >= 0 && m < Ns;
      const float v = real ? x[(size_t)m * C + c] : 0.0f;
      if (v > gbest || h == 0) { gbest = v; garg = real ? m : Ns; }
    }
    out[(size_t)n * C + c] = gbest;
    if (argmax) argmax[(size_t)n * C + c] = garg;
    return;
  }
  const int32_t* row = idx + (size_t)n * H;
  float best = -INFINITY;
  int arg = Ns;
  // the reference's table has min(limit, max_count) columns (dataloader.py:64-66): with a wider, static-shape table the
  // device-resident max_count says how many leading columns it would have kept
  const int Hw = width ? min(H, max(1, __builtin_amdgcn_readfirstlane(*width))) : H;  // wave-uniform loop bound
  for (int h = 0; h < Hw; ++h) {
    const int m = row[h];
    const bool real = m >= 0 && m < Ns;
    const float v = real ? x[(size_t)m * C + c] : 0.0f;  // shadow row is zeros (blocks.py:103)
    if (v > best || h == 0) {
      best = v;
      arg = real ? m : Ns;
    }
  }
  out[(size_t)n * C + c] = best;
  if (argmax) argmax[(size_t)n * C + c] = arg;
}

// One gather group of max_pool_fwd_v4_kernel: the 16-byte gathers of G consecutive neighbors (entries j0 .. j0 + G - 1
// of the index chunk, which the L lanes of a row hold as ea = columns 0 .. L - 1 and eb = columns L .. 2L - 1) issued
// back to back, then compared in row order as they return.  Every load is unconditional and every update a select (a
// conditional load or a branch around a compare costs the counted waits: kpconv_dx_gather.hip): a shadow entry loads
// the row `spare` (the query's first neighbor, which the wave has just read: one fixed row for every shadow of the
// launch measured 2-7 % slower) and the shadow's zero is selected afterwards.  Entries past the chunk repeat its last
// one and are not counted.
template <bool kWave, int G>
__device__ __forceinline__ void max_pool_gather_group(const float4* __restrict__ x4, int Ns, uint32_t C4, uint32_t c4,
                                                      int ea, int eb, int spare, int lane0, int L, int j0, int h0,
                                                      int Hw, float4& best, int4& arg) {
  int m[G];
  float4 v[G];
#pragma unroll
  for (int k = 0; k < G; ++k) {
    const int j = min(j0 + k, 2 * L - 1);
    const int e = j < L ? ea : eb, src = j < L ? j : j - L;
    m[k] = kWave ? __builtin_amdgcn_readlane(e, src) : __shfl(e, lane0 + src);
  }
#pragma unroll
  for (int k = 0; k < G; ++k) v[k] = x4[(uint32_t)(m[k] >= 0 && m[k] < Ns ? m[k] : spare) * C4 + c4];
#pragma unroll
  for (int k = 0; k < G; ++k) {
    const int h = h0 + j0 + k;
    const bool real = m[k] >= 0 && m[k] < Ns;
    const uint32_t keep = real ? ~0u : 0u;  // shadow row is zeros (blocks.py:103); a mask, so that the load stays put
    const auto kept = [keep](float f) { return __uint_as_float(__float_as_uint(f) & keep); };
    const float4 u = make_float4(kept(v[k].x), kept(v[k].y), kept(v[k].z), kept(v[k].w));
    const int mm = real ? m[k] : Ns;
    const bool counted = j0 + k < 2 * L && h < Hw;
    const bool tx = counted && (u.x > best.x || h == 0), ty = counted && (u.y > best.y || h == 0);
    const bool tz = counted && (u.z > best.z || h == 0), tw = counted && (u.w > best.w || h == 0);
    best.x = tx ? u.x : best.x; arg.x = tx ? mm : arg.x;
    best.y = ty ? u.y : best.y; arg.y = ty ? mm : arg.y;
    best.z = tz ? u.z : best.z; arg.z = tz ? mm : arg.z;
    best.w = tw ? u.w : best.w; arg.w = tw ? mm : arg.w;
  }
}

// 4 channels per lane (C % 4 == 0), 32-bit element indices.  Rows belong to waves: the L lanes of a row cover its C4
// channel groups.  kWave = false: C4 divides 64, a wave takes 64 / C4 consecutive rows (L = C4); kWave = true: one row
// per wave and ceil(C4 / 64) waves per row (L = 64, the lanes past C4 idle).  The lanes of a row read its index row
// once, 2L columns per pair of coalesced loads, and hand the entries out by shuffle (readlane when the wave has one
// row); the gathers run 8 neighbors at a time (max_pool_gather_group).  The row's cloud and its group's table width
// come from one coalesced load of the lengths and one of the widths per wave, issued together with the index row.
// No lane leaves before the last shuffle: the rows and channel groups past the end are clamped and not stored.
// 62 / 55 VGPRs; per 3-pair stack 85.8 / 38.6 / 30.2 / 26.4 -> 50.4 / 23.3 / 15.2 / 9.9 us
// (profiles/maxpool_rows_timeline.txt).
template <bool kWave>
__global__ __launch_bounds__(256) void max_pool_fwd_v4_kernel(const float* __restrict__ x, int Ns, int C4,
                                                              const int32_t* __restrict__ idx, int Nq, int H,
                                                              float* __restrict__ out, int32_t* __restrict__ argmax,
                                                              float* __restrict__ clear,
                                                              const int32_t* __restrict__ width, d3f::RowGroups rg) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (clear) {
    const uint32_t n4 = (uint32_t)Ns * (uint32_t)C4;
    for (uint32_t i = t; i < n4; i += gridDim.x * blockDim.x) ((float4*)clear)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const int lane = (int)(threadIdx.x & 63u);
  // workgroups go to the 8 XCDs round robin: XCD k takes the k-th eighth of the rows, so that queries next to each
  // other, which share most of their neighbors, gather through the same L2 (64.7 -> 50.4 us at 23.8k x 128)
  const uint32_t per_xcd = gridDim.x >> 3, left = gridDim.x & 7u, xcd = blockIdx.x & 7u;
  const uint32_t block = xcd * per_xcd + min(xcd, left) + (blockIdx.x >> 3);
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(block * 4u + (threadIdx.x >> 6)));
  const int L = kWave ? 64 : C4;                                  // lanes per row (kWave = false: a power of two)
  const int lshift = kWave ? 6 : __builtin_ctz((unsigned)C4);
  const uint32_t parts = kWave ? ((uint32_t)C4 + 63u) >> 6 : 1u;  // waves per row
  const uint32_t unit = wave / parts, part = wave - unit * parts;
  const uint32_t n_first = unit << (6 - lshift);
  if (n_first >= (uint32_t)Nq) return;                            // the whole wave
  const int sub = lane >> lshift, sl = lane - (sub << lshift), lane0 = sub << lshift;
  const uint32_t n_own = n_first + (uint32_t)sub, c_own = part * 64u + (uint32_t)sl;
  const bool live = n_own < (uint32_t)Nq && c_own < (uint32_t)C4;
  const uint32_t n = min(n_own, (uint32_t)Nq - 1u), c4 = min(c_own, (uint32_t)C4 - 1u);
  const int32_t* row = idx + (size_t)n * H;
  int ea = row[min(sl, H - 1)], eb = row[min(L + sl, H - 1)];     // first chunk of the index row, two entries per lane

  // the reference's table has min(limit, max_count) columns (dataloader.py:64-66): with a wider, static-shape table the
  // device-resident max_count says how many leading columns it would have kept; stacked pairs: every group of clouds
  // has the width of the table its own batch would have had
  int Hw = H, Hmax = H;
  if (width) {
    const bool grouped = rg.len && rg.group > 0;
    const int wd = width[grouped ? min(lane, (rg.B - 1) / rg.group) : 0];
    int g = 0;
    if (grouped) {
      const int len = rg.len[min(lane, rg.B - 1)];
      int b = 0, end = 0;                                         // locate_batch for every row of the wave at once
      for (int k = 0; k < rg.B - 1; ++k) {
        end += __builtin_amdgcn_readlane(len, k);
        b += (int)n >= end;
      }
      g = b / rg.group;
    }
    Hw = min(H, max(1, __shfl(wd, g)));
    Hmax = Hw;
    if (!kWave)
      for (int o = 32; o >= L; o >>= 1) Hmax = max(Hmax, __shfl_xor(Hmax, o));
    Hmax = __builtin_amdgcn_readfirstlane(Hmax);
  }

  float4 best = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
  int4 arg = make_int4(Ns, Ns, Ns, Ns);
  if (Ns <= 0) {
    best = make_float4(0.f, 0.f, 0.f, 0.f);                       // no support row to read: every entry is the shadow
  } else {
    const float4* x4 = (const float4*)x;
    const int spare = min(max(kWave ? __builtin_amdgcn_readlane(ea, 0) : __shfl(ea, lane0), 0), Ns - 1);
    for (int h0 = 0; h0 < Hmax; h0 += 2 * L) {
      if (h0 > 0) {                                               // tables wider than 2L columns
        ea = row[min(h0 + sl, H - 1)];
        eb = row[min(h0 + L + sl, H - 1)];
      }
      const int cnt = min(2 * L, Hmax - h0);
      int j0 = 0;
      for (; j0 + 8 <= cnt; j0 += 8)  // (groups of 4 and of 16, 43 and 81 VGPRs: 2-7 % slower on a step's 4 launches)
        max_pool_gather_group<kWave, 8>(x4, Ns, (uint32_t)C4, c4, ea, eb, spare, lane0, L, j0, h0, Hw, best, arg);
      if (cnt - j0 > 4)
        max_pool_gather_group<kWave, 8>(x4, Ns, (uint32_t)C4, c4, ea, eb, spare, lane0, L, j0, h0, Hw, best, arg);
      else if (cnt - j0 > 0)
        max_pool_gather_group<kWave, 4>(x4, Ns, (uint32_t)C4, c4, ea, eb, spare, lane0, L, j0, h0, Hw, best, arg);
    }
  }
  if (!live) return;
  const uint32_t o = n * (uint32_t)C4 + c4;
  ((float4*)out)[o] = best;
  if (argmax) ((int4*)argmax)[o] = arg;
}

__global__ void max_pool_bwd_kernel(const float* __restrict__ go, const int32_t* __restrict__ argmax, int Nq, int C,
                                    int Ns, float* __restrict__ gx) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)Nq * C) return;
  const int m = argmax[t];
  if (m >= 0 && m < Ns) atomicAdd(&gx[(size_t)m * C + (t % C)], go[t]);
}

__global__ void max_pool_bwd32_kernel(const float* __restrict__ go, const int32_t* __restrict__ argmax, uint32_t total,
                                      uint32_t C, int Ns, float* __restrict__ gx) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const int m = argmax[t];
  if (m >= 0 && m < Ns) atomicAdd(&gx[(uint32_t)m * C + t % C], go[t]);
}

// out has Cs extra columns per row filled from `skip` [Nq, Cs]: the decoder's upsample + concatenation
// (architectures.py:311-313 after blocks.py:712) written by ONE launch (Cs = 0: plain closest_pool)
__global__ void closest_pool_fwd_kernel(const float* __restrict__ x, int Ns, int C, const int32_t* __restrict__ idx,
                                        int Nq, int H, const float* __restrict__ skip, int Cs,
                                        float* __restrict__ out, float* __restrict__ clear) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (clear)
    for (size_t i = t; i < (size_t)Ns * C; i += (size_t)gridDim.x * blockDim.x) clear[i] = 0.0f;
  const int W = C + Cs;
  if (t >= (size_t)Nq * W) return;
  const int n = (int)(t / W), c = (int)(t % W);
  if (c < C) {
    const int m = idx[(size_t)n * H];
    out[t] = (m >= 0 && m < Ns) ? x[(size_t)m * C + c] : 0.0f;
  } else {
    out[t] = skip[(size_t)n * Cs + (c - C)];
  }
}

// 16 bytes per thread (C % 4 == 0 and Cs % 4 == 0), 32-bit element indices
__global__ void closest_pool_fwd_v4_kernel(const float* __restrict__ x, int Ns, int C4, const int32_t* __restrict__ idx,
                                           int Nq, int H, const float* __restrict__ skip, int Cs4,
                                           float* __restrict__ out, float* __restrict__ clear) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (clear) {
    const uint32_t n4 = (uint32_t)Ns * (uint32_t)C4;
    for (uint32_t i = t; i < n4; i += gridDim.x * blockDim.x) ((float4*)clear)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const uint32_t W4 = (uint32_t)(C4 + Cs4);
  if (t >= (uint32_t)Nq * W4) return;
  const uint32_t n = t / W4, c = t - n * W4;
  float4 v;
  if (c < (uint32_t)C4) {
    const int m = idx[(size_t)n * H];
    v = (m >= 0 && m < Ns) ? ((const float4*)x)[(size_t)m * C4 + c] : make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    v = ((const float4*)skip)[(size_t)n * Cs4 + (c - C4)];
  }
  ((float4*)out)[t] = v;
}

// go has row stride ld >= C (the gradient of a concatenation arrives as a column slice: no contiguous copy needed)
__global__ void closest_pool_bwd_kernel(const float* __restrict__ go, int ld, const int32_t* __restrict__ idx, int Nq,
                                        int H, int C, int Ns, float* __restrict__ gx) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)Nq * C) return;
  const int n = (int)(t / C), c = (int)(t % C);
  const int m = idx[(size_t)n * H];
  if (m >= 0 && m < Ns) atomicAdd(&gx[(size_t)m * C + c], go[(size_t)n * ld + c]);
}

__global__ void closest_pool_bwd32_kernel(const float* __restrict__ go, uint32_t ld, const int32_t* __restrict__ idx,
                                          uint32_t total, uint32_t H, uint32_t C, int Ns, float* __restrict__ gx) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= total) return;
  const uint32_t n = t / C, c = t - n * C;
  const int m = idx[(size_t)n * H];
  // (a zero contributes nothing, bit for bit -- and the descriptor head's incoming gradient is zero in ~70 % of its rows:
  // the losses read the correspondences only)
  const float v = go[(size_t)n * ld + c];
  if (m >= 0 && m < Ns && v != 0.0f) atomicAdd(&gx[(uint32_t)m * C + c], v);
}

// ---- gather forms of the two backward passes (the deterministic mode) -------------------------------------------------
// The scatters above add in arrival order.  These walk the CSR transpose of the table (reverse_table.hip: rev_ent[rev_ptr[s]
// .. rev_ptr[s+1]) = the query rows that list support s, ASCENDING) and write every row of grad_x exactly once: no clear
// launch, no atomic, the same bits on every replay.  A thread owns one float4 (or one float) of one support row, so the
// threads of a row read the same entries (one broadcast request) and 16 contiguous bytes of each listed query row; four
// entries are fetched before the first is added.
//   max_pool      gx[s, c] = base[s, c] + go[q1, c] + go[q2, c] + ...   q1 < q2 < ... in rev(s) with argmax[q, c] == s
//   closest_pool  gx[s, c] = go[n1, c] + go[n2, c] + ...                n1 < n2 < ... with idx[n, 0] == s (rev of column 0)
// added left to right in float32; base (optional, may be gx itself) is a gradient an older consumer left for the same
// tensor and comes FIRST.  A query that lists s twice is one term; rows nobody lists and shadow entries give base / 0.
template <typename I>
__global__ __launch_bounds__(256) void max_pool_bwd_gather_kernel(const float* __restrict__ go,
                                                                  const int32_t* __restrict__ argmax,
                                                                  const int32_t* __restrict__ ptr,
                                                                  const int32_t* __restrict__ ent, I total, I C, int Nq,
                                                                  const float* base, float* gx) {
  const I t = (I)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const I s = t / C, c = t - s * C;
  float acc = base ? base[t] : 0.0f;
  int prev = -1;
  for (int i = ptr[s], e = ptr[s + 1]; i < e; ++i) {
    const int q = ent[i];
    if (q == prev || (unsigned)q >= (unsigned)Nq) continue;
    prev = q;
    const I o = (I)q * C + c;
    if (argmax[o] == (int)s) acc += go[o];
  }
  gx[t] = acc;
}

__global__ __launch_bounds__(256) void max_pool_bwd_gather_v4_kernel(const float4* __restrict__ go,
                                                                     const int4* __restrict__ argmax,
                                                                     const int32_t* __restrict__ ptr,
                                                                     const int32_t* __restrict__ ent, uint32_t total4,
                                                                     uint32_t C4, int Nq, const float4* base, float4* gx) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= total4) return;
  const uint32_t s = t / C4, c4 = t - s * C4;
  const int si = (int)s;
  float4 acc = base ? base[t] : make_float4(0.f, 0.f, 0.f, 0.f);
  int prev = -1;
  int i = ptr[s];
  const int e = ptr[s + 1];
  for (; i + 4 <= e; i += 4) {
    int q[4];
    bool live[4];
    int4 a[4];
    float4 g[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = ent[i + j];
#pragma unroll
    for (int j = 0; j < 4; ++j) live[j] = q[j] != (j ? q[j - 1] : prev) && (unsigned)q[j] < (unsigned)Nq;
    prev = q[3];
#pragma unroll
    for (int j = 0; j < 4; ++j) {   // (a dead entry re-reads row 0: entries exist only when Nq > 0)
      const uint32_t o = (uint32_t)(live[j] ? q[j] : 0) * C4 + c4;
      a[j] = argmax[o];
      g[j] = go[o];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (live[j] && a[j].x == si) acc.x += g[j].x;
      if (live[j] && a[j].y == si) acc.y += g[j].y;
      if (live[j] && a[j].z == si) acc.z += g[j].z;
      if (live[j] && a[j].w == si) acc.w += g[j].w;
    }
  }
  for (; i < e; ++i) {
    const int q = ent[i];
    if (q == prev || (unsigned)q >= (unsigned)Nq) continue;
    prev = q;
    const uint32_t o = (uint32_t)q * C4 + c4;
    const int4 a = argmax[o];
    const float4 g = go[o];
    if (a.x == si) acc.x += g.x;
    if (a.y == si) acc.y += g.y;
    if (a.z == si) acc.z += g.z;
    if (a.w == si) acc.w += g.w;
  }
  gx[t] = acc;
}

template <typename I>
__global__ __launch_bounds__(256) void closest_pool_bwd_gather_kernel(const float* __restrict__ go, I ld,
                                                                      const int32_t* __restrict__ ptr,
                                                                      const int32_t* __restrict__ ent, I total, I C,
                                                                      int Nq, float* __restrict__ gx) {
  const I t = (I)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const I s = t / C, c = t - s * C;
  float acc = 0.0f;
  for (int i = ptr[s], e = ptr[s + 1]; i < e; ++i) {
    const int n = ent[i];
    if ((unsigned)n < (unsigned)Nq) acc += go[(I)n * ld + c];
  }
  gx[t] = acc;
}

// ld4 = row stride of go in float4
__global__ __launch_bounds__(256) void closest_pool_bwd_gather_v4_kernel(const float4* __restrict__ go, uint32_t ld4,
                                                                         const int32_t* __restrict__ ptr,
                                                                         const int32_t* __restrict__ ent, uint32_t total4,
                                                                         uint32_t C4, int Nq, float4* __restrict__ gx) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  if (t >= total4) return;
  const uint32_t s = t / C4, c4 = t - s * C4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  int i = ptr[s];
  const int e = ptr[s + 1];
  for (; i + 4 <= e; i += 4) {
    int n[4];
    float4 g[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) n[j] = ent[i + j];
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] = go[(uint32_t)((unsigned)n[j] < (unsigned)Nq ? n[j] : 0) * ld4 + c4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if ((unsigned)n[j] < (unsigned)Nq) {
        acc.x += g[j].x; acc.y += g[j].y; acc.z += g[j].z; acc.w += g[j].w;
      }
  }
  for (; i < e; ++i) {
    const int n = ent[i];
    if ((unsigned)n >= (unsigned)Nq) continue;
    const float4 g = go[(uint32_t)n * ld4 + c4];
    acc.x += g.x; acc.y += g.y; acc.z += g.z; acc.w += g.w;
  }
  gx[t] = acc;
}

}  // namespace

extern "C" {

int d3f_max_pool_forward(const float* x, int Ns, int C, const int32_t* idx, int Nq, int H, float* out,
                         int32_t* argmax_out, float* grad_x_clear, const int32_t* width_dev, const int32_t* q_len,
                         int B, int group, void* stream) {
  if (!x || !idx || !out || Ns < 0 || C < 1 || Nq < 0 || H < 1) return D3F_EINVAL;
  if (q_len && (B < 1 || B > D3F_MAX_BATCH || group < 1)) return D3F_EINVAL;
  const d3f::RowGroups rg = {q_len, B, group};
  if (Nq == 0) {
    if (grad_x_clear && d3f::zero_async(grad_x_clear, sizeof(float) * (size_t)Ns * C, (hipStream_t)stream) != hipSuccess)
      return D3F_ELAUNCH;
    return D3F_OK;
  }
  const bool small = (long long)Nq * C < (1ll << 31) && (long long)Ns * C < (1ll << 31);
  const bool aligned = ((uintptr_t)x | (uintptr_t)out | (uintptr_t)argmax_out | (uintptr_t)grad_x_clear) % 16 == 0;
  if (C % 4 == 0 && small && aligned) {
    const int C4 = C / 4;
    if (C4 < 64 && 64 % C4 == 0)  // 64 / C4 rows per wave
      max_pool_fwd_v4_kernel<false><<<d3f::cdiv(d3f::cdiv((long long)Nq * C4, 64), 4), 256, 0, (hipStream_t)stream>>>(
          x, Ns, C4, idx, Nq, H, out, argmax_out, grad_x_clear, width_dev, rg);
    else                          // ceil(C4 / 64) waves per row
      max_pool_fwd_v4_kernel<true><<<d3f::cdiv((long long)Nq * d3f::cdiv(C4, 64), 4), 256, 0, (hipStream_t)stream>>>(
          x, Ns, C4, idx, Nq, H, out, argmax_out, grad_x_clear, width_dev, rg);
  }
  else
    max_pool_fwd_kernel<<<d3f::cdiv((long long)Nq * C, 256), 256, 0, (hipStream_t)stream>>>(
        x, Ns, C, idx, Nq, H, out, argmax_out, grad_x_clear, width_dev, rg);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_max_pool_backward(const float* grad_out, const int32_t* argmax, int Nq, int C, int Ns, float* grad_x,
                          int grad_x_precleared, void* stream) {
  if (!grad_out || !argmax || !grad_x || Nq < 0 || C < 1 || Ns < 0) return D3F_EINVAL;
  if (!grad_x_precleared &&
      d3f::zero_async(grad_x, sizeof(float) * (size_t)Ns * C, (hipStream_t)stream) != hipSuccess)
    return D3F_ELAUNCH;
  if (Nq == 0) return D3F_OK;
  if ((long long)Nq * C < (1ll << 31) && (long long)Ns * C < (1ll << 31))
    max_pool_bwd32_kernel<<<d3f::cdiv((long long)Nq * C, 256), 256, 0, (hipStream_t)stream>>>(
        grad_out, argmax, (uint32_t)Nq * (uint32_t)C, (uint32_t)C, Ns, grad_x);
  else
    max_pool_bwd_kernel<<<d3f::cdiv((long long)Nq * C, 256), 256, 0, (hipStream_t)stream>>>(grad_out, argmax, Nq, C,
                                                                                            Ns, grad_x);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_closest_pool_forward(const float* x, int Ns, int C, const int32_t* idx, int Nq, int H, const float* skip,
                             int Cs, float* out, float* grad_x_clear, void* stream) {
  if (!x || !idx || !out || Ns < 0 || C < 1 || Nq < 0 || H < 1 || Cs < 0 || (Cs > 0 && !skip)) return D3F_EINVAL;
  if (Nq == 0) {
    if (grad_x_clear && d3f::zero_async(grad_x_clear, sizeof(float) * (size_t)Ns * C, (hipStream_t)stream) != hipSuccess)
      return D3F_ELAUNCH;
    return D3F_OK;
  }
  const bool small = (long long)Nq * (C + Cs) < (1ll << 31) && (long long)Ns * C < (1ll << 31);
  const bool aligned = ((uintptr_t)x | (uintptr_t)out | (uintptr_t)skip | (uintptr_t)grad_x_clear) % 16 == 0;
  if (C % 4 == 0 && Cs % 4 == 0 && small && aligned)
    closest_pool_fwd_v4_kernel<<<d3f::cdiv((long long)Nq * ((C + Cs) / 4), 256), 256, 0, (hipStream_t)stream>>>(
        x, Ns, C / 4, idx, Nq, H, skip, Cs / 4, out, grad_x_clear);
  else
    closest_pool_fwd_kernel<<<d3f::cdiv((long long)Nq * (C + Cs), 256), 256, 0, (hipStream_t)stream>>>(
        x, Ns, C, idx, Nq, H, skip, Cs, out, grad_x_clear);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_closest_pool_backward(const float* grad_out, int ld, const int32_t* idx, int Nq, int H, int C, int Ns,
                              float* grad_x, int grad_x_precleared, void* stream) {
  if (!grad_out || !idx || !grad_x || Nq < 0 || C < 1 || Ns < 0 || H < 1 || ld < C) return D3F_EINVAL;
  if (!grad_x_precleared &&
      d3f::zero_async(grad_x, sizeof(float) * (size_t)Ns * C, (hipStream_t)stream) != hipSuccess)
    return D3F_ELAUNCH;
  if (Nq == 0) return D3F_OK;
  if ((long long)Nq * ld < (1ll << 31) && (long long)Ns * C < (1ll << 31))
    closest_pool_bwd32_kernel<<<d3f::cdiv((long long)Nq * C, 256), 256, 0, (hipStream_t)stream>>>(
        grad_out, (uint32_t)ld, idx, (uint32_t)Nq * (uint32_t)C, (uint32_t)H, (uint32_t)C, Ns, grad_x);
  else
    closest_pool_bwd_kernel<<<d3f::cdiv((long long)Nq * C, 256), 256, 0, (hipStream_t)stream>>>(grad_out, ld, idx, Nq,
                                                                                                H, C, Ns, grad_x);
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_max_pool_backward_gather(const float* grad_out, const int32_t* argmax, int Nq, int C, int Ns,
                                 const int32_t* rev_ptr, const int32_t* rev_ent, const float* grad_base, float* grad_x,
                                 void* stream) {
  if (((!grad_out || !argmax) && Nq > 0) || !rev_ptr || !rev_ent || !grad_x || Nq < 0 || C < 1 || Ns < 0)
    return D3F_EINVAL;   // (no query rows: nothing is read through grad_out / argmax, every row is grad_base or 0)
  if (Ns == 0) return D3F_OK;
  const long long total = (long long)Ns * C;
  const bool small = (long long)Nq * C < (1ll << 31) && total < (1ll << 31);
  const bool aligned = ((uintptr_t)grad_out | (uintptr_t)argmax | (uintptr_t)grad_base | (uintptr_t)grad_x) % 16 == 0;
  if (small && aligned && C % 4 == 0)
    max_pool_bwd_gather_v4_kernel<<<d3f::cdiv(total / 4, 256), 256, 0, (hipStream_t)stream>>>(
        (const float4*)grad_out, (const int4*)argmax, rev_ptr, rev_ent, (uint32_t)(total / 4), (uint32_t)(C / 4), Nq,
        (const float4*)grad_base, (float4*)grad_x);
  else if (small)
    max_pool_bwd_gather_kernel<uint32_t><<<d3f::cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(
        grad_out, argmax, rev_ptr, rev_ent, (uint32_t)total, (uint32_t)C, Nq, grad_base, grad_x);
  else if (total < 256ll * 0x7fffffffll)
    max_pool_bwd_gather_kernel<size_t><<<d3f::cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(
        grad_out, argmax, rev_ptr, rev_ent, (size_t)total, (size_t)C, Nq, grad_base, grad_x);
  else
    return D3F_EINVAL;
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

int d3f_closest_pool_backward_gather(const float* grad_out, int ld, int Nq, int C, int Ns, const int32_t* rev_ptr,
                                     const int32_t* rev_ent, float* grad_x, void* stream) {
  if ((!grad_out && Nq > 0) || !rev_ptr || !rev_ent || !grad_x || Nq < 0 || C < 1 || Ns < 0 || ld < C) return D3F_EINVAL;
  if (Ns == 0) return D3F_OK;
  const long long total = (long long)Ns * C;
  const bool small = (long long)Nq * ld < (1ll << 31) && total < (1ll << 31);
  const bool aligned = ((uintptr_t)grad_out | (uintptr_t)grad_x) % 16 == 0;
  if (small && aligned && C % 4 == 0 && ld % 4 == 0)
    closest_pool_bwd_gather_v4_kernel<<<d3f::cdiv(total / 4, 256), 256, 0, (hipStream_t)stream>>>(
        (const float4*)grad_out, (uint32_t)(ld / 4), rev_ptr, rev_ent, (uint32_t)(total / 4), (uint32_t)(C / 4), Nq,
        (float4*)grad_x);
  else if (small)
    closest_pool_bwd_gather_kernel<uint32_t><<<d3f::cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(
        grad_out, (uint32_t)ld, rev_ptr, rev_ent, (uint32_t)total, (uint32_t)C, Nq, grad_x);
  else if (total < 256ll * 0x7fffffffll)
    closest_pool_bwd_gather_kernel<size_t><<<d3f::cdiv(total, 256), 256, 0, (hipStream_t)stream>>>(
        grad_out, (size_t)ld, rev_ptr, rev_ent, (size_t)total, (size_t)C, Nq, grad_x);
  else
    return D3F_EINVAL;
  D3F_LAUNCH_CHECK();
  return D3F_OK;
}

}  // extern "C"
