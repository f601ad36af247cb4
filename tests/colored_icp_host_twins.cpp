// A stand-alone program for the host twin of the colour gradient under the host sanitizers (no GPU call is made, and
// nothing here is loaded into Python).  Build and run from the repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Iinclude -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined d3feat.pytorch_amd/csrc/normals.hip \
//         tests/colored_icp_host_twins.cpp -o /tmp/colored_icp_host_twins && /tmp/colored_icp_host_twins
//
// It calls d3f_color_gradient_from_moments_host on the moments of a linear intensity ramp over a plane in three
// orientations (the exact gradient must come back), and on every invalid case of the contract: too few neighbours, a
// zero normal, a NaN normal, collinear neighbours, no neighbours at all, the point's own intensity NaN, below 0 and
// above 1, the largest moments the contract allows, and null arguments; every buffer is sized exactly, so a read or
// write past an end is reported.  Exit status 0 and "ok" mean that the sanitizers saw nothing.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "d3feat_hip.h"

static const double Q = 4194304.0;   // 2^22: a radius in (0.125, 0.25]

// moments of the offsets `u` (already quantised) with intensity differences `c` (quantised)
static std::vector<int64_t> moments_of(const std::vector<int64_t>& u, const std::vector<int64_t>& c) {
  std::vector<int64_t> m(13, 0);
  for (size_t k = 0; k < c.size(); ++k) {
    const int64_t x = u[3 * k], y = u[3 * k + 1], z = u[3 * k + 2];
    m[0] += 1;
    m[1] += x; m[2] += y; m[3] += z;
    m[4] += x * x; m[5] += x * y; m[6] += x * z; m[7] += y * y; m[8] += y * z; m[9] += z * z;
    m[10] += x * c[k]; m[11] += y * c[k]; m[12] += z * c[k];
  }
  return m;
}

static bool three_nans(const std::vector<float>& o) { return isnan(o[0]) && isnan(o[1]) && isnan(o[2]); }

static int ramp(int plane) {
  // a 7 x 7 lattice of spacing 0.01 in the plane whose normal is axis `plane`; intensity 0.5 + 0.5 s + 0.4 t
  std::vector<int64_t> u, c;
  for (int i = -3; i <= 3; ++i)
    for (int j = -3; j <= 3; ++j) {
      const double s = 0.01 * i, t = 0.01 * j;
      int64_t v[3] = {0, 0, 0};
      v[(plane + 1) % 3] = (int64_t)rint(s * Q);
      v[(plane + 2) % 3] = (int64_t)rint(t * Q);
      u.insert(u.end(), v, v + 3);
      c.push_back((int64_t)rint((0.5 * s + 0.4 * t) * 1048576.0));
    }
  const std::vector<int64_t> m = moments_of(u, c);
  float nrm[3] = {0.0f, 0.0f, 0.0f};
  nrm[plane] = plane == 1 ? -1.0f : 1.0f;
  std::vector<float> out(4, 0.0f);
  if (d3f_color_gradient_from_moments_host(m.data(), Q, nrm, 0.5f, 4, out.data())) return 1;
  double want[3] = {0.0, 0.0, 0.0};
  want[(plane + 1) % 3] = 0.5;
  want[(plane + 2) % 3] = 0.4;
  for (int k = 0; k < 3; ++k)
    if (!(fabs((double)out[k] - want[k]) < 1e-4)) return 2;
  if (out[3] != 0.5f || out[plane] != 0.0f) return 3;
  printf("  ramp, normal along %d: d = (%g, %g, %g)\n", plane, out[0], out[1], out[2]);
  // the same moments: every invalid case gives exactly three NaNs, and .w follows the intensity alone
  const float up[3] = {nrm[0], nrm[1], nrm[2]}, zero[3] = {0.0f, 0.0f, 0.0f}, bad[3] = {NAN, 0.0f, 1.0f};
  if (d3f_color_gradient_from_moments_host(m.data(), Q, up, 0.5f, 50, out.data()) || !three_nans(out) || out[3] != 0.5f)
    return 4;   // 49 neighbours, 50 asked for
  if (d3f_color_gradient_from_moments_host(m.data(), Q, zero, 0.25f, 4, out.data()) || !three_nans(out) || out[3] != 0.25f)
    return 5;
  if (d3f_color_gradient_from_moments_host(m.data(), Q, bad, 1.0f, 4, out.data()) || !three_nans(out) || out[3] != 1.0f)
    return 6;
  for (float I : {NAN, -0.1f, 1.5f, INFINITY})
    if (d3f_color_gradient_from_moments_host(m.data(), Q, up, I, 4, out.data()) || !three_nans(out) || !isnan(out[3]))
      return 7;
  if (d3f_color_gradient_from_moments_host(m.data(), Q, up, 0.0f, 4, out.data()) || three_nans(out) || out[3] != 0.0f)
    return 8;   // 0 and 1 are usable
  return 0;
}

static int corners() {
  std::vector<float> out(4, 0.0f);
  const float up[3] = {0.0f, 0.0f, 1.0f}, tilt[3] = {0.6f, 0.0f, 0.8f};
  // collinear neighbours: the 2x2 is singular
  std::vector<int64_t> u, c;
  for (int i = -4; i <= 4; ++i) {
    u.push_back(1000 * i); u.push_back(2000 * i); u.push_back(0);
    c.push_back(300 * i);
  }
  std::vector<int64_t> m = moments_of(u, c);
  if (d3f_color_gradient_from_moments_host(m.data(), Q, up, 0.5f, 4, out.data()) || !three_nans(out)) return 1;
  // no neighbour, and neighbours that all coincide with the point
  std::vector<int64_t> none(13, 0);
  if (d3f_color_gradient_from_moments_host(none.data(), Q, up, 0.5f, 1, out.data()) || !three_nans(out)) return 2;
  none[0] = 100;
  if (d3f_color_gradient_from_moments_host(none.data(), Q, up, 0.5f, 4, out.data()) || !three_nans(out)) return 3;
  // the largest moments the contract allows: 2^22 neighbours at |u| = 2^20, |c| = 2^20
  std::vector<int64_t> big(13, 0);
  const int64_t n = (int64_t)1 << 22, e = (int64_t)1 << 20;
  big[0] = n;
  big[4] = big[7] = n * e * e;
  big[5] = n / 2 * e * e;
  big[10] = n * e * e;
  big[11] = -(n * e * e);
  if (d3f_color_gradient_from_moments_host(big.data(), Q, up, 1.0f, 4, out.data()) || three_nans(out)) return 4;
  if (!(fabs(out[0]) < 1e300) || out[2] != 0.0f) return 5;
  // a tilted normal: the gradient stays on the tangent plane
  if (d3f_color_gradient_from_moments_host(big.data(), Q, tilt, 1.0f, 4, out.data()) || three_nans(out)) return 6;
  const double dot = (double)out[0] * 0.6 + (double)out[2] * 0.8;
  const double size = fabs(out[0]) + fabs(out[1]) + fabs(out[2]);
  if (!(fabs(dot) <= 1e-6 * (size > 1.0 ? size : 1.0))) return 7;
  // null arguments, a Q that is not positive, min_neighbors below 1
  if (d3f_color_gradient_from_moments_host(nullptr, Q, up, 0.5f, 4, out.data()) != D3F_EINVAL) return 8;
  if (d3f_color_gradient_from_moments_host(m.data(), Q, nullptr, 0.5f, 4, out.data()) != D3F_EINVAL) return 9;
  if (d3f_color_gradient_from_moments_host(m.data(), Q, up, 0.5f, 4, nullptr) != D3F_EINVAL) return 10;
  if (d3f_color_gradient_from_moments_host(m.data(), 0.0, up, 0.5f, 4, out.data()) != D3F_EINVAL) return 11;
  if (d3f_color_gradient_from_moments_host(m.data(), Q, up, 0.5f, 0, out.data()) != D3F_EINVAL) return 12;
  return 0;
}

int main() {
  const int rc = ramp(0) * 1000000 + ramp(1) * 10000 + ramp(2) * 100 + corners();
  printf(rc ? "FAILED %d\n" : "ok\n", rc);
  return rc ? 1 : 0;
}
