// A stand-alone program for the host twins of the RGB-D odometry under the host sanitizers (no GPU call is made, and
// nothing here is loaded into Python).  Build and run from the repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Iinclude -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined d3feat.pytorch_amd/csrc/odometry.hip \
//         tests/rgbd_odometry_host_twins.cpp -o /tmp/rgbd_odometry_host_twins && /tmp/rgbd_odometry_host_twins
//
// It calls d3f_rgbd_pyramid_host (8-bit colour, 8-bit grey and f32), d3f_rgbd_odometry_step_host and
// d3f_rgbd_odometry_host on small images of odd size (37 x 23: levels of 18 x 11 and 9 x 5) with holes in the depth, a
// NaN and an infinity in the intensity, a pose that pushes projections to and past every image border, a frame index
// out of range and a non-finite pose in the batch, and on a 5 x 5 image whose coarsest level is 1 x 1; every buffer is
// sized exactly, so a read or write past an end is reported.  Exit status 0 and "ok" mean that the sanitizers saw
// nothing.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "d3feat_hip.h"

static int check(int H, int W, int levels) {
  const int F = 2, P = 5;
  const int64_t frame_pixels = d3f_depth_pyramid_pixels(H, W, levels);
  if (frame_pixels <= 0) return 1;
  std::vector<float> depth((size_t)F * H * W), K = {30.0f, 30.0f, (W - 1) / 2.0f, (H - 1) / 2.0f,
                                                   30.0f, 30.0f, (W - 1) / 2.0f, (H - 1) / 2.0f};
  std::vector<float> grey((size_t)F * H * W);
  std::vector<uint8_t> rgb((size_t)F * H * W * 3), g8((size_t)F * H * W);
  for (int f = 0; f < F; ++f)
    for (int v = 0; v < H; ++v)
      for (int u = 0; u < W; ++u) {
        const size_t i = ((size_t)f * H + v) * W + u;
        depth[i] = 1.0f + 0.002f * u + 0.003f * v + 0.004f * f + 0.01f * sinf(0.7f * u) * cosf(0.5f * v);
        grey[i] = 0.5f + 0.25f * sinf(0.55f * u + 0.2f * f) * cosf(0.4f * v);
        g8[i] = (uint8_t)(255.0f * grey[i]);
        rgb[3 * i] = g8[i];
        rgb[3 * i + 1] = (uint8_t)(250.0f * grey[i]);
        rgb[3 * i + 2] = (uint8_t)(240.0f * grey[i]);
      }
  if (H > 12 && W > 20) {
    for (int v = 5; v < 12; ++v)
      for (int u = 10; u < 20; ++u) depth[(size_t)v * W + u] = 0.0f;
    grey[(size_t)3 * W + 7] = NAN;
    grey[(size_t)H * W + (size_t)2 * W + 9] = INFINITY;
  }
  std::vector<float> pyr((size_t)F * frame_pixels), KL((size_t)F * levels * 4), inten((size_t)F * frame_pixels);
  if (d3f_depth_pyramid_host(depth.data(), 1, F, H, W, K.data(), levels, 1000.0f, 6.0f, 0.05f, pyr.data(), KL.data()))
    return 2;
  if (d3f_rgbd_pyramid_host(rgb.data(), D3F_RGBD_COLOR_RGB8, F, H, W, levels, inten.data())) return 3;
  if (d3f_rgbd_pyramid_host(g8.data(), D3F_RGBD_COLOR_GREY8, F, H, W, levels, inten.data())) return 4;
  if (d3f_rgbd_pyramid_host(grey.data(), D3F_RGBD_COLOR_F32, F, H, W, levels, inten.data())) return 5;
  if (d3f_rgbd_pyramid_host(grey.data(), 3, F, H, W, levels, inten.data()) != D3F_EINVAL) return 6;
  const int32_t pairs[2 * P] = {1, 0, 0, 1, 2, 0, 1, 0, 1, 0};
  std::vector<double> T((size_t)P * 12, 0.0);
  for (int p = 0; p < P; ++p) {
    T[12 * p + 0] = T[12 * p + 5] = T[12 * p + 10] = 1.0;
    T[12 * p + 3] = 0.004 * p;
  }
  T[12 * 3 + 7] = NAN;
  T[12 * 4 + 3] = 0.45;    // the last pair: projections run over the right border
  T[12 * 4 + 7] = -0.3;    // and over the top
  for (int level = 0; level < levels; ++level) {
    const size_t pixels = (size_t)(H >> level) * (size_t)(W >> level);
    std::vector<double> sums((size_t)P * D3F_RGBD_SUMS);
    std::vector<int32_t> index((size_t)P * pixels);
    for (float w : {0.3f, 0.0f}) {
      if (d3f_rgbd_odometry_step_host(pyr.data(), inten.data(), KL.data(), F, H, W, levels, pairs, P, T.data(), level,
                                      w == 0.0f ? 0.1f : 1.0f, 0.05f, w, sums.data(), index.data()))
        return 7;
      if (d3f_rgbd_odometry_step_host(pyr.data(), inten.data(), KL.data(), F, H, W, levels, pairs, P, T.data(), level,
                                      0.1f, 0.05f, w, sums.data(), nullptr))
        return 8;
      for (int p = 0; p < P; ++p)
        for (int k = 0; k < D3F_RGBD_SUMS; ++k)
          if (!(fabs(sums[(size_t)p * D3F_RGBD_SUMS + k]) < 1e300)) return 9;   // a NaN or an infinity got in
      if (w == 0.0f && (sums[29] != 0.0 || sums[30] != 0.0)) return 10;
      if (sums[29] > sums[0]) return 11;
    }
    for (size_t i = 0; i < pixels; ++i)
      if (index[2 * pixels + i] != -1 || index[3 * pixels + i] != -1) return 12;
    printf("  %d x %d level %d: accepted %g pixels of pair 0\n", W, H, level, sums[0]);
  }
  if (d3f_rgbd_odometry_step_host(pyr.data(), inten.data(), KL.data(), F, H, W, levels, pairs, P, T.data(), 0, 0.1f,
                                  0.05f, -1.0f, nullptr, nullptr) != D3F_EINVAL)
    return 13;
  std::vector<int32_t> iterations(levels, 3), count(P), status(P), n_photo(P);
  std::vector<double> To((size_t)P * 16), rmse(P), info((size_t)P * 36);
  if (d3f_rgbd_odometry_host(pyr.data(), inten.data(), KL.data(), F, H, W, levels, pairs, P, T.data(), iterations.data(),
                             0.1f, 0.05f, 0.3f, To.data(), count.data(), rmse.data(), status.data(), n_photo.data(),
                             info.data()))
    return 14;
  if (d3f_rgbd_odometry_host(pyr.data(), inten.data(), KL.data(), F, H, W, levels, pairs, P, T.data(), iterations.data(),
                             0.1f, 0.05f, 0.3f, To.data(), count.data(), rmse.data(), status.data(), n_photo.data(),
                             nullptr))
    return 15;
  printf("  %d x %d odometry: status %d %d %d %d %d, count %d %d, n_photo %d %d\n", W, H, status[0], status[1],
         status[2], status[3], status[4], count[0], count[1], n_photo[0], n_photo[1]);
  if (status[2] != D3F_ODO_ST_PAIR || status[3] != D3F_ODO_ST_NONFINITE || n_photo[2] != 0 || n_photo[3] != 0) return 16;
  return 0;
}

int main() {
  const int rc = check(23, 37, 3) * 100 + check(5, 5, 3);
  printf(rc ? "FAILED %d\n" : "ok\n", rc);
  return rc ? 1 : 0;
}
