// A stand-alone program for the host twins of the sparse ray-caster, of the continued sparse integration and of the
// colour integration (dense and sparse) under the host sanitizers (no GPU call is made, and nothing here is loaded into Python).  Build and run from the repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Iinclude -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined d3feat.pytorch_amd/csrc/tsdf.hip \
//         d3feat.pytorch_amd/csrc/tsdf_integrate.hip d3feat.pytorch_amd/csrc/tsdf_sparse.hip \
//         d3feat.pytorch_amd/csrc/tsdf_raycast.hip \
//         tests/raycast_sparse_host_twins.cpp -o /tmp/raycast_sparse_host_twins && /tmp/raycast_sparse_host_twins
//
// Two volumes of different dims (13 x 9 x 7: 2 x 2 x 1 lattice bricks with borders at index 7 | 8 on two axes, and
// 5 x 1 x 4, without a cell along y) go through d3f_tsdf_sparse_mark_host, _index_host and _integrate_host over two
// frames of 37 x 23 each, and again as one frame followed by the same entry with into = 1; the two pools must
// agree bit for bit.  The colour forms follow with channels = 1 and 3, dense (d3f_tsdf_integrate_host) and sparse
// (d3f_tsdf_sparse_integrate_host): the whole call against two frames followed by the other two with into = 1,
// bit for bit on D, w and the colour, D and w those of the channels = 0 calls, and the pool's
// colour that of the dense volume.  d3f_tsdf_raycast_sparse_host then renders six views in the order 1, 0, 1, 0, 0, 0 -- among them a
// pose holding a NaN, a pose holding an infinity and a camera far outside -- with the skip and the clip on and off, with
// and without normals, at min_weight 1 and 0, and all must equal d3f_tsdf_raycast_host on the pool scattered into dense
// volumes, bit for bit; then again with two of the bricks taken out of the tables.
// Every buffer is sized exactly (the pool to the allocated bricks, brick_coord to them too, the colour frames and
// Cv / Cp to their channels), so a read or write past an
// end is reported.  Exit status 0 and "ok" mean that the sanitizers saw nothing.
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
  std::vector<float> K((size_t)F * 4), M((size_t)F * 12, 0.0f), Cf((size_t)F * 12, 0.0f);
  for (int f = 0; f < F; ++f) {
    const float k[4] = {30.0f, 30.0f, 18.0f, 11.0f};
    memcpy(&K[4 * f], k, sizeof k);
    M[12 * f] = M[12 * f + 5] = M[12 * f + 10] = 1.0f;
    M[12 * f + 3] = 0.01f * (f % 2);
    Cf[12 * f] = Cf[12 * f + 5] = Cf[12 * f + 10] = 1.0f;              // the inverse: camera -> volume
    Cf[12 * f + 3] = -0.01f * (f % 2);
  }
  const int32_t dims[6] = {13, 9, 7, 5, 1, 4};
  const int64_t lattice_start[3] = {0, 4, 5};                          // 2 x 2 x 1 bricks, then 1 x 1 x 1
  const int64_t L = lattice_start[2];
  const int64_t vol_start[3] = {0, 13 * 9 * 7, 13 * 9 * 7 + 5 * 1 * 4};
  const int64_t total = vol_start[2];
  const float origin[6] = {-0.3f, -0.2f, 0.9f, -0.1f, 0.0f, 0.95f}, voxel[2] = {0.05f, 0.05f}, trunc[2] = {0.1f, 0.1f};
  const float step[2] = {0.05f, 0.05f};
  const int32_t both[3] = {0, 2, 4}, first[3] = {0, 1, 2};

  std::vector<int32_t> flags(L), index(L), coord_all((size_t)L * 3);
  int64_t brick_start[3];
  if (d3f_tsdf_sparse_mark_host(depth.data(), 1, F, H, W, both, V, K.data(), Cf.data(), origin, dims, voxel, trunc,
                                lattice_start, L, 1000.0f, 6.0f, flags.data()))
    return 2;
  if (d3f_tsdf_sparse_index_host(flags.data(), lattice_start, dims, V, L, index.data(), coord_all.data(), brick_start))
    return 3;
  const int64_t B = brick_start[2];
  printf("bricks: %lld of %lld\n", (long long)B, (long long)L);
  if (B < 1 || B > L) return 4;
  std::vector<int32_t> coord(coord_all.begin(), coord_all.begin() + 3 * B);        // exactly B rows
  std::vector<float> D((size_t)B * 512), w((size_t)B * 512), D2(D.size()), w2(w.size());
  if (d3f_tsdf_sparse_integrate_host(depth.data(), nullptr, 0, 1, F, H, W, both, V, K.data(), M.data(), origin, dims,
                                     voxel, trunc, brick_start, coord.data(), B, 1000.0f, 6.0f, 0, D.data(), w.data(),
                                     nullptr, nullptr))
    return 5;
  // frames 0 and 2 first, then frames 1 and 3 into the result
  std::vector<float> da, db, Ka, Kb, Ma, Mb;
  for (int f = 0; f < F; ++f) {
    std::vector<float>&d = f % 2 ? db : da, &k = f % 2 ? Kb : Ka, &m = f % 2 ? Mb : Ma;
    d.insert(d.end(), depth.begin() + (size_t)f * H * W, depth.begin() + (size_t)(f + 1) * H * W);
    k.insert(k.end(), K.begin() + 4 * f, K.begin() + 4 * (f + 1));
    m.insert(m.end(), M.begin() + 12 * f, M.begin() + 12 * (f + 1));
  }
  if (d3f_tsdf_sparse_integrate_host(da.data(), nullptr, 0, 1, 2, H, W, first, V, Ka.data(), Ma.data(), origin, dims,
                                     voxel, trunc, brick_start, coord.data(), B, 1000.0f, 6.0f, 0, D2.data(), w2.data(),
                                     nullptr, nullptr))
    return 6;
  if (d3f_tsdf_sparse_integrate_host(db.data(), nullptr, 0, 1, 2, H, W, first, V, Kb.data(), Mb.data(), origin, dims,
                                     voxel, trunc, brick_start, coord.data(), B, 1000.0f, 6.0f, 1, D2.data(), w2.data(),
                                     nullptr, nullptr))
    return 7;
  if (memcmp(D.data(), D2.data(), D.size() * sizeof(float)) || memcmp(w.data(), w2.data(), w.size() * sizeof(float)))
    return 8;
  const int32_t none[3] = {0, 0, 0};                                         // no volume owns a frame: nothing changes
  if (d3f_tsdf_sparse_integrate_host(db.data(), nullptr, 0, 1, 2, H, W, none, V, Kb.data(), Mb.data(), origin, dims,
                                     voxel, trunc, brick_start, coord.data(), B, 1000.0f, 6.0f, 1, D2.data(), w2.data(),
                                     nullptr, nullptr))
    return 9;
  if (memcmp(D.data(), D2.data(), D.size() * sizeof(float)) || memcmp(w.data(), w2.data(), w.size() * sizeof(float)))
    return 10;

  // colour, 1 and 3 channels, dense and sparse: the whole call against frames 0 and 2 followed by frames 1 and 3 into
  // the result; D and w are those of the colourless calls.  The colour frames and Cv / Cp are sized exactly
  std::vector<float> Dv(total), wv(total), Dv2(total), wv2(total), Dc(total), wc(total), Dq(D.size()), wq(w.size());
  if (d3f_tsdf_integrate_host(depth.data(), nullptr, 0, 1, F, H, W, both, vol_start, V, total, total, K.data(),
                              M.data(), origin, dims, voxel, trunc, 1000.0f, 6.0f, 0, Dv.data(), wv.data(), nullptr,
                              nullptr))
    return 30;
  for (int Cc = 1; Cc <= 3; Cc += 2) {
    std::vector<float> colour((size_t)F * H * W * Cc), ca, cb;
    for (size_t i = 0; i < colour.size(); ++i) colour[i] = 0.5f + 0.4f * sinf(0.37f * (float)i);
    for (int f = 0; f < F; ++f) {
      std::vector<float>& c = f % 2 ? cb : ca;
      c.insert(c.end(), colour.begin() + (size_t)f * H * W * Cc, colour.begin() + (size_t)(f + 1) * H * W * Cc);
    }
    std::vector<float> Cv((size_t)total * Cc), Cv2(Cv.size()), Cp((size_t)B * 512 * Cc), Cp2(Cp.size());
    if (d3f_tsdf_integrate_host(depth.data(), colour.data(), Cc, 1, F, H, W, both, vol_start, V, total, total, K.data(),
                                M.data(), origin, dims, voxel, trunc, 1000.0f, 6.0f, 0, Dc.data(), wc.data(), Cv.data(),
                                nullptr))
      return 31;
    if (d3f_tsdf_integrate_host(da.data(), ca.data(), Cc, 1, 2, H, W, first, vol_start, V, total, total, Ka.data(),
                                Ma.data(), origin, dims, voxel, trunc, 1000.0f, 6.0f, 0, Dv2.data(), wv2.data(),
                                Cv2.data(), nullptr))
      return 32;
    if (d3f_tsdf_integrate_host(db.data(), cb.data(), Cc, 1, 2, H, W, first, vol_start, V, total, total, Kb.data(),
                                Mb.data(), origin, dims, voxel, trunc, 1000.0f, 6.0f, 1, Dv2.data(), wv2.data(),
                                Cv2.data(), nullptr))
      return 33;
    if (memcmp(Dc.data(), Dv.data(), Dv.size() * sizeof(float)) || memcmp(wc.data(), wv.data(), wv.size() * sizeof(float)) ||
        memcmp(Dc.data(), Dv2.data(), Dv.size() * sizeof(float)) || memcmp(wc.data(), wv2.data(), wv.size() * sizeof(float)) ||
        memcmp(Cv.data(), Cv2.data(), Cv.size() * sizeof(float)))
      return 34;
    if (d3f_tsdf_sparse_integrate_host(depth.data(), colour.data(), Cc, 1, F, H, W, both, V, K.data(), M.data(), origin,
                                       dims, voxel, trunc, brick_start, coord.data(), B, 1000.0f, 6.0f, 0, Dq.data(),
                                       wq.data(), Cp.data(), nullptr))
      return 35;
    if (d3f_tsdf_sparse_integrate_host(da.data(), ca.data(), Cc, 1, 2, H, W, first, V, Ka.data(), Ma.data(), origin,
                                       dims, voxel, trunc, brick_start, coord.data(), B, 1000.0f, 6.0f, 0, D2.data(),
                                       w2.data(), Cp2.data(), nullptr))
      return 36;
    if (d3f_tsdf_sparse_integrate_host(db.data(), cb.data(), Cc, 1, 2, H, W, first, V, Kb.data(), Mb.data(), origin,
                                       dims, voxel, trunc, brick_start, coord.data(), B, 1000.0f, 6.0f, 1, D2.data(),
                                       w2.data(), Cp2.data(), nullptr))
      return 37;
    if (memcmp(Dq.data(), D.data(), D.size() * sizeof(float)) || memcmp(wq.data(), w.data(), w.size() * sizeof(float)) ||
        memcmp(Dq.data(), D2.data(), D.size() * sizeof(float)) || memcmp(wq.data(), w2.data(), w.size() * sizeof(float)) ||
        memcmp(Cp.data(), Cp2.data(), Cp.size() * sizeof(float)))
      return 38;
    // a slot inside the lattice holds the dense colour of its voxel; a slot beyond dims holds 0
    int seen = 0;
    for (int v = 0; v < V; ++v)
      for (int64_t b = brick_start[v]; b < brick_start[v + 1]; ++b)
        for (int s = 0; s < 512; ++s) {
          const int ix = coord[3 * b] * 8 + (s & 7), iy = coord[3 * b + 1] * 8 + ((s >> 3) & 7);
          const int iz = coord[3 * b + 2] * 8 + (s >> 6);
          const bool in = ix < dims[3 * v] && iy < dims[3 * v + 1] && iz < dims[3 * v + 2];
          const int64_t at = vol_start[v] + ((int64_t)iz * dims[3 * v + 1] + iy) * dims[3 * v] + ix;
          for (int ch = 0; ch < Cc; ++ch) {
            const float c = Cp[(b * 512 + s) * Cc + ch];
            if (in ? memcmp(&c, &Cv[at * Cc + ch], sizeof c) != 0 : c != 0.0f) return 39;
          }
          seen += in && wq[b * 512 + s] > 0.0f;
        }
    printf("colour, %d channel(s): %d coloured slots\n", Cc, seen);
    if (!seen) return 40;
  }

  // the pool scattered into dense volumes: zero outside the allocated bricks
  std::vector<float> Dd(total, 0.0f), wd(total, 0.0f);
  for (int v = 0; v < V; ++v)
    for (int64_t b = brick_start[v]; b < brick_start[v + 1]; ++b)
      for (int s = 0; s < 512; ++s) {
        const int ix = coord[3 * b] * 8 + (s & 7), iy = coord[3 * b + 1] * 8 + ((s >> 3) & 7);
        const int iz = coord[3 * b + 2] * 8 + (s >> 6);
        if (ix >= dims[3 * v] || iy >= dims[3 * v + 1] || iz >= dims[3 * v + 2]) continue;
        const int64_t at = vol_start[v] + ((int64_t)iz * dims[3 * v + 1] + iy) * dims[3 * v] + ix;
        Dd[at] = D[b * 512 + s];
        wd[at] = w[b * 512 + s];
      }

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
  // pass 1: the tables say that bricks (1, 0, 0) and (1, 1, 0) of the first volume are absent (their rows stay in the
  // pool, unused), and the dense volumes lose those voxels: absent bricks beside present ones, cells that straddle both
  for (int pass = 0; pass < 2; ++pass)
  for (int mw = 0; mw < 2; ++mw) {                        // min_weight 1, then 0: absent bricks become a valid D = 0
    const float min_weight = mw ? 0.0f : 1.0f;
    if (pass == 1 && mw == 0) {
      index[1] = index[3] = -1;
      for (int iz = 0; iz < 7; ++iz)
        for (int iy = 0; iy < 9; ++iy)
          for (int ix = 8; ix < 13; ++ix) Dd[((size_t)iz * 9 + iy) * 13 + ix] = wd[((size_t)iz * 9 + iy) * 13 + ix] = 0.0f;
    }
    if (d3f_tsdf_raycast_host(Dd.data(), wd.data(), nullptr, 0, vol_start, origin, dims, voxel, V, total, view_volume,
                              R, H, W, Kv.data(), C.data(), step, 0.1f, 6.0f, min_weight, 1, image.data(),
                              normals.data(), nullptr, nullptr))
      return 11;
    for (int mode = 0; mode < 4; ++mode) {
      if (d3f_tsdf_raycast_sparse_host(D.data(), w.data(), nullptr, 0, lattice_start, brick_start, index.data(), origin,
                                       dims, voxel, V, L, B, view_volume, R, H, W, Kv.data(), C.data(), step, 0.1f,
                                       6.0f, min_weight, mode & 1, mode >> 1, image2.data(), normals2.data(), nullptr,
                                       nullptr))
        return 12;
      if (memcmp(image.data(), image2.data(), image.size() * sizeof(float)) ||
          memcmp(normals.data(), normals2.data(), normals.size() * sizeof(float)))
        return 13 + mode;
    }
    if (d3f_tsdf_raycast_sparse_host(D.data(), w.data(), nullptr, 0, lattice_start, brick_start, index.data(), origin,
                                     dims, voxel, V, L, B, view_volume, R, H, W, Kv.data(), C.data(), step, 0.1f, 6.0f,
                                     min_weight, 1, 1, image2.data(), nullptr, nullptr, nullptr))
      return 17;
    if (memcmp(image.data(), image2.data(), image.size() * sizeof(float))) return 18;
    if (!mw && !pass) {
      int hits[R] = {0, 0, 0, 0, 0, 0};
      for (int r = 0; r < R; ++r)
        for (int i = 0; i < H * W; ++i) hits[r] += image[(size_t)r * H * W + i] > 0.0f;
      printf("hits per view: %d %d %d %d %d %d\n", hits[0], hits[1], hits[2], hits[3], hits[4], hits[5]);
      if (hits[0] || hits[2] || hits[3] || hits[4] || hits[5] || !hits[1]) return 19;   // only view 1 sees a surface
    }
  }
  if (d3f_tsdf_raycast_sparse_host(D.data(), w.data(), nullptr, 0, lattice_start, brick_start, index.data(), origin,
                                   dims, voxel, V, L, B, view_volume, 0, H, W, nullptr, nullptr, step, 0.1f, 6.0f, 1.0f,
                                   1, 1, nullptr, nullptr, nullptr, nullptr))
    return 20;
  // no brick at all: a pool of no rows is never read
  const int64_t empty_start[3] = {0, 0, 0};
  std::vector<int32_t> absent(L, -1);
  if (d3f_tsdf_raycast_sparse_host(nullptr, nullptr, nullptr, 0, lattice_start, empty_start, absent.data(), origin,
                                   dims, voxel, V, L, 0, view_volume, R, H, W, Kv.data(), C.data(), step, 0.1f, 6.0f,
                                   1.0f, 1, 1, image2.data(), normals2.data(), nullptr, nullptr))
    return 21;
  for (float d : image2)
    if (d != 0.0f) return 22;
  printf("ok\n");
  return 0;
}
