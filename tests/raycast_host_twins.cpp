// A stand-alone program for the host twins of the ray-caster and of the continued integration under the host sanitizers
// (no GPU call is made, and nothing here is loaded into Python).  Build and run from the repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Iinclude -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined d3feat.pytorch_amd/csrc/tsdf.hip \
//         d3feat.pytorch_amd/csrc/tsdf_integrate.hip d3feat.pytorch_amd/csrc/tsdf_raycast.hip \
//         tests/raycast_host_twins.cpp -o /tmp/raycast_host_twins && /tmp/raycast_host_twins
//
// Two volumes of different dims (13 x 9 x 7 and 5 x 1 x 4, the second without a cell along y) are fused from two frames
// of 37 x 23 by d3f_tsdf_integrate_host, and again as one frame followed by the same entry with into = 1; the two must
// agree bit for bit.  d3f_tsdf_raycast_host then renders six views in the order 1, 0, 1, 0, 0, 0 -- among them a pose
// holding a NaN, a pose holding an infinity and a camera far outside -- with and without normals and with the clip on
// and off, which must agree bit for bit.  Every buffer is sized exactly, so a read or write past an end is reported.
// Exit status 0 and "ok" mean that the sanitizers saw nothing.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "d3feat_hip.h"

int main() {
  const int H = 23, W = 37, F = 4, V = 2;
  std::vector<float> depth((size_t)F * H * W);
  for (int f = 0; f < F; ++f)
    for (int v = 0; v < H; ++v)
      for (int u = 0; u < W; ++u) depth[((size_t)f * H + v) * W + u] = 1.0f + 0.002f * u + 0.003f * v + 0.004f * (f % 2);
  depth[(size_t)3 * W + 7] = NAN;
  depth[(size_t)H * W + (size_t)2 * W + 9] = INFINITY;
  std::vector<float> K((size_t)F * 4), M((size_t)F * 12, 0.0f);
  for (int f = 0; f < F; ++f) {
    const float k[4] = {30.0f, 30.0f, 18.0f, 11.0f};
    memcpy(&K[4 * f], k, sizeof k);
    M[12 * f] = M[12 * f + 5] = M[12 * f + 10] = 1.0f;
    M[12 * f + 3] = 0.01f * (f % 2);
  }
  const int32_t dims[6] = {13, 9, 7, 5, 1, 4};
  const int64_t vol_start[3] = {0, 13 * 9 * 7, 13 * 9 * 7 + 5 * 1 * 4};
  const int64_t total = vol_start[2];
  const float origin[6] = {-0.3f, -0.2f, 0.9f, -0.1f, 0.0f, 0.95f}, voxel[2] = {0.05f, 0.05f}, trunc[2] = {0.1f, 0.1f};
  const float step[2] = {0.05f, 0.05f};
  const int32_t both[3] = {0, 2, 4}, first[3] = {0, 1, 2};
  std::vector<float> D(total), w(total), D2(total), w2(total);
  if (d3f_tsdf_integrate_host(depth.data(), nullptr, 0, 1, F, H, W, both, vol_start, V, total, total, K.data(),
                              M.data(), origin, dims, voxel, trunc, 1000.0f, 6.0f, 0, D.data(), w.data(), nullptr,
                              nullptr))
    return 2;
  // frames 0 and 2 first, then frames 1 and 3 into the result
  std::vector<float> da, db, Ka, Kb, Ma, Mb;
  for (int f = 0; f < F; ++f) {
    std::vector<float>&d = f % 2 ? db : da, &k = f % 2 ? Kb : Ka, &m = f % 2 ? Mb : Ma;
    d.insert(d.end(), depth.begin() + (size_t)f * H * W, depth.begin() + (size_t)(f + 1) * H * W);
    k.insert(k.end(), K.begin() + 4 * f, K.begin() + 4 * (f + 1));
    m.insert(m.end(), M.begin() + 12 * f, M.begin() + 12 * (f + 1));
  }
  if (d3f_tsdf_integrate_host(da.data(), nullptr, 0, 1, 2, H, W, first, vol_start, V, total, total, Ka.data(),
                              Ma.data(), origin, dims, voxel, trunc, 1000.0f, 6.0f, 0, D2.data(), w2.data(), nullptr,
                              nullptr))
    return 3;
  if (d3f_tsdf_integrate_host(db.data(), nullptr, 0, 1, 2, H, W, first, vol_start, V, total, total, Kb.data(),
                              Mb.data(), origin, dims, voxel, trunc, 1000.0f, 6.0f, 1, D2.data(), w2.data(), nullptr,
                              nullptr))
    return 4;
  if (memcmp(D.data(), D2.data(), total * sizeof(float)) || memcmp(w.data(), w2.data(), total * sizeof(float))) return 5;
  const int32_t none[3] = {0, 0, 0};                                         // no volume owns a frame: nothing changes
  if (d3f_tsdf_integrate_host(db.data(), nullptr, 0, 1, 2, H, W, none, vol_start, V, total, total, Kb.data(), Mb.data(),
                              origin, dims, voxel, trunc, 1000.0f, 6.0f, 1, D2.data(), w2.data(), nullptr, nullptr))
    return 6;
  if (memcmp(D.data(), D2.data(), total * sizeof(float))) return 7;

  const int R = 6;
  const int32_t view_volume[R] = {1, 0, 1, 0, 0, 0};
  std::vector<float> Kv((size_t)R * 4), C((size_t)R * 12, 0.0f);
  for (int r = 0; r < R; ++r) {
    memcpy(&Kv[4 * r], &K[0], 4 * sizeof(float));
    C[12 * r] = C[12 * r + 5] = C[12 * r + 10] = 1.0f;
    C[12 * r + 3] = 0.01f * r;
  }
  C[12 * 3 + 6] = NAN;
  C[12 * 4 + 11] = INFINITY;
  C[12 * 5 + 3] = 1.0e6f;
  std::vector<float> image((size_t)R * H * W), normals((size_t)R * H * W * 3), image2(image.size()), normals2(normals.size());
  for (int clip = 0; clip < 2; ++clip) {
    std::vector<float>&im = clip ? image : image2, &nr = clip ? normals : normals2;
    if (d3f_tsdf_raycast_host(D.data(), w.data(), nullptr, 0, vol_start, origin, dims, voxel, V, total, view_volume, R,
                              H, W, Kv.data(), C.data(), step, 0.1f, 6.0f, 1.0f, clip, im.data(), nr.data(), nullptr,
                              nullptr))
      return 8;
  }
  if (memcmp(image.data(), image2.data(), image.size() * sizeof(float)) ||
      memcmp(normals.data(), normals2.data(), normals.size() * sizeof(float)))
    return 9;
  if (d3f_tsdf_raycast_host(D.data(), w.data(), nullptr, 0, vol_start, origin, dims, voxel, V, total, view_volume, R, H,
                            W, Kv.data(), C.data(), step, 0.1f, 6.0f, 1.0f, 1, image2.data(), nullptr, nullptr,
                            nullptr))
    return 10;
  if (memcmp(image.data(), image2.data(), image.size() * sizeof(float))) return 11;
  int hits[R] = {0, 0, 0, 0, 0, 0};
  for (int r = 0; r < R; ++r)
    for (int i = 0; i < H * W; ++i) {
      const float d = image[(size_t)r * H * W + i];
      if (!(d >= 0.0f && d <= 6.0f)) return 12;
      hits[r] += d > 0.0f;
    }
  printf("hits per view: %d %d %d %d %d %d\n", hits[0], hits[1], hits[2], hits[3], hits[4], hits[5]);
  if (hits[0] || hits[2] || hits[3] || hits[4] || hits[5] || !hits[1]) return 13;   // only view 1 sees a surface
  if (d3f_tsdf_raycast_host(D.data(), w.data(), nullptr, 0, vol_start, origin, dims, voxel, V, total, view_volume, 0, H,
                            W, nullptr, nullptr, step, 0.1f, 6.0f, 1.0f, 1, nullptr, nullptr, nullptr, nullptr))
    return 14;
  const float bad_step[2] = {0.0f, 1e-9f};                                    // casts nothing: zeros, no long loop
  if (d3f_tsdf_raycast_host(D.data(), w.data(), nullptr, 0, vol_start, origin, dims, voxel, V, total, view_volume, R, H,
                            W, Kv.data(), C.data(), bad_step, 0.1f, 6.0f, 1.0f, 1, image2.data(), nullptr, nullptr,
                            nullptr))
    return 15;
  for (float d : image2)
    if (d != 0.0f) return 16;
  printf("ok\n");
  return 0;
}
