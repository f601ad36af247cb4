// A stand-alone program for the host twins of the depth odometry under the host sanitizers (no GPU call is made, and
// nothing here is loaded into Python).  Build and run from the repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Iinclude -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined d3feat.pytorch_amd/csrc/odometry.hip tests/odometry_host_twins.cpp \
//         -o /tmp/odometry_host_twins && /tmp/odometry_host_twins
//
// It calls d3f_depth_pyramid_host, d3f_depth_odometry_step_host and d3f_depth_odometry_host on small images of odd
// size (37 x 23: levels of 18 x 11 and 9 x 5) with holes, a NaN and an infinity, with a frame index out of range and a
// non-finite pose in the batch, and on a 5 x 5 image whose coarsest level is 1 x 1; every buffer is sized exactly, so a
// read or write past an end is reported.  Exit status 0 and "ok" mean that the sanitizers saw nothing.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "d3feat_hip.h"

static int check(int H, int W, int levels) {
  const int F = 2, P = 4;
  const int64_t frame_pixels = d3f_depth_pyramid_pixels(H, W, levels);
  if (frame_pixels <= 0) return 1;
  std::vector<float> depth((size_t)F * H * W), K = {30.0f, 30.0f, (W - 1) / 2.0f, (H - 1) / 2.0f,
                                                   30.0f, 30.0f, (W - 1) / 2.0f, (H - 1) / 2.0f};
  for (int f = 0; f < F; ++f)
    for (int v = 0; v < H; ++v)
      for (int u = 0; u < W; ++u)
        depth[((size_t)f * H + v) * W + u] = 1.0f + 0.002f * u + 0.003f * v + 0.004f * f + 0.01f * sinf(0.7f * u) * cosf(0.5f * v);
  if (H > 12 && W > 20) {
    for (int v = 5; v < 12; ++v)
      for (int u = 10; u < 20; ++u) depth[(size_t)v * W + u] = 0.0f;
    depth[(size_t)3 * W + 7] = NAN;
    depth[(size_t)H * W + (size_t)2 * W + 9] = INFINITY;
  }
  std::vector<float> pyr((size_t)F * frame_pixels), KL((size_t)F * levels * 4);
  if (d3f_depth_pyramid_host(depth.data(), 1, F, H, W, K.data(), levels, 1000.0f, 6.0f, 0.05f, pyr.data(), KL.data()))
    return 2;
  std::vector<uint16_t> raw((size_t)F * H * W, 1000);
  std::vector<float> pyr16((size_t)F * frame_pixels);
  if (d3f_depth_pyramid_host(raw.data(), 0, F, H, W, K.data(), levels, 1000.0f, 6.0f, 0.05f, pyr16.data(), KL.data()))
    return 3;
  if (d3f_depth_pyramid_host(depth.data(), 1, F, H, W, K.data(), levels, 1000.0f, 6.0f, 0.05f, pyr.data(), KL.data()))
    return 4;
  const int32_t pairs[2 * P] = {1, 0, 0, 1, 2, 0, 1, 0};
  std::vector<double> T((size_t)P * 12, 0.0);
  for (int p = 0; p < P; ++p) {
    T[12 * p + 0] = T[12 * p + 5] = T[12 * p + 10] = 1.0;
    T[12 * p + 3] = 0.004 * p;
  }
  T[12 * 3 + 7] = NAN;
  for (int level = 0; level < levels; ++level) {
    const size_t pixels = (size_t)(H >> level) * (size_t)(W >> level);
    std::vector<double> sums((size_t)P * D3F_ODO_SUMS);
    std::vector<int32_t> index((size_t)P * pixels);
    if (d3f_depth_odometry_step_host(pyr.data(), KL.data(), F, H, W, levels, pairs, P, T.data(), level, 0.1f, 0.05f,
                                     sums.data(), index.data()))
      return 5;
    if (d3f_depth_odometry_step_host(pyr.data(), KL.data(), F, H, W, levels, pairs, P, T.data(), level, 0.1f, 0.05f,
                                     sums.data(), nullptr))
      return 6;
    for (size_t i = 0; i < pixels; ++i)
      if (index[2 * pixels + i] != -1 || index[3 * pixels + i] != -1) return 7;
    printf("  %d x %d level %d: accepted %g and %g pixels\n", W, H, level, sums[0], sums[D3F_ODO_SUMS]);
  }
  std::vector<int32_t> iterations(levels, 3), count(P), status(P);
  std::vector<double> To((size_t)P * 16), rmse(P), info((size_t)P * 36);
  if (d3f_depth_odometry_host(pyr.data(), KL.data(), F, H, W, levels, pairs, P, T.data(), iterations.data(), 0.1f, 0.05f,
                              To.data(), count.data(), rmse.data(), status.data(), info.data()))
    return 8;
  if (d3f_depth_odometry_host(pyr.data(), KL.data(), F, H, W, levels, pairs, P, T.data(), iterations.data(), 0.1f, 0.05f,
                              To.data(), count.data(), rmse.data(), status.data(), nullptr))
    return 9;
  printf("  %d x %d odometry: status %d %d %d %d, count %d %d\n", W, H, status[0], status[1], status[2], status[3],
         count[0], count[1]);
  if (status[2] != D3F_ODO_ST_PAIR || status[3] != D3F_ODO_ST_NONFINITE) return 10;
  return 0;
}

int main() {
  const int rc = check(23, 37, 3) * 100 + check(5, 5, 3);
  printf(rc ? "FAILED %d\n" : "ok\n", rc);
  return rc ? 1 : 0;
}
