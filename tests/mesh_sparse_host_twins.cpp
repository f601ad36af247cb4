// A stand-alone program for the host twin of the sparse mesh under the host sanitizers (no GPU call is made, and
// nothing here is loaded into Python).  Build and run from the repository root:
//
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Iinclude -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined d3feat.pytorch_amd/csrc/tsdf_mesh_sparse.hip \
//         tests/mesh_sparse_host_twins.cpp -o /tmp/mesh_sparse_host_twins && /tmp/mesh_sparse_host_twins
//
// Three volumes in one batch: 17 x 9 x 10 voxels (3 x 2 x 2 lattice bricks, edge bricks on every axis) of which 9
// bricks are allocated, a volume without bricks, and 5 x 1 x 1 voxels with its one brick.  D of the first is a tilted
// plane that crosses brick faces, edges and the corner, next to absent bricks; a few slots have w = 0.  One table entry
// names a rank beyond the pool, which must read as an absent brick.  d3f_tsdf_sparse_mesh_host runs with capacities 0
// (the totals), with the exact capacities and with half of them; every buffer is sized exactly, so a read or write
// past an end is reported; the rows below the smaller capacities must equal the full result and the status bits must be
// the ones the capacities call for.  Exit status 0 and "ok" mean that the sanitizers saw nothing.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "d3feat_hip.h"

#define CHECK(x)                                             \
  do {                                                       \
    if (!(x)) {                                              \
      printf("FAILED line %d: %s\n", __LINE__, #x);          \
      return 1;                                              \
    }                                                        \
  } while (0)

int main() {
  const int V = 3;
  const int32_t dims[9] = {17, 9, 10, 4, 4, 4, 5, 1, 1};
  const float origin[9] = {0.1f, -0.2f, 0.3f, 0.0f, 0.0f, 0.0f, 1.0f, 1.0f, 1.0f};
  const float voxel[3] = {0.05f, 0.02f, 0.1f};
  const int64_t lattice_start[4] = {0, 12, 13, 14};
  // volume 0: lattice bricks 2 (bx = 2, by = 0, bz = 0), 4 and 11 are absent; brick 7 is named with a rank beyond the pool
  std::vector<int32_t> index = {0, 1, -1, 2, -1, 3, 4, 1000, 5, 6, 7, -1, -1, 0};
  std::vector<int32_t> coord;
  int64_t rows = 0;
  for (int l = 0; l < 12; ++l)
    if (index[l] >= 0 && index[l] < 100) {
      const int32_t c[3] = {l % 3, (l / 3) % 2, l / 6};
      coord.insert(coord.end(), c, c + 3);
      ++rows;
    }
  CHECK(rows == 8);
  const int32_t last[3] = {0, 0, 0};
  coord.insert(coord.end(), last, last + 3);
  const int64_t B = rows + 1;
  const int64_t brick_start[4] = {0, rows, rows, B};
  std::vector<float> D((size_t)B * 512, 0.0f), w((size_t)B * 512, 0.0f);
  for (int64_t b = 0; b < rows; ++b)
    for (int s = 0; s < 512; ++s) {
      const int ix = coord[3 * b] * 8 + (s & 7), iy = coord[3 * b + 1] * 8 + ((s >> 3) & 7);
      const int iz = coord[3 * b + 2] * 8 + (s >> 6);
      if (ix >= 17 || iy >= 9 || iz >= 10) continue;
      const float sdf = ((float)ix - 7.6f) + 0.4f * ((float)iy - 7.7f) + 0.3f * ((float)iz - 7.8f);
      D[(size_t)b * 512 + s] = fminf(1.0f, fmaxf(-1.0f, sdf / 4.0f));
      w[(size_t)b * 512 + s] = (ix + 2 * iy + 3 * iz) % 37 == 0 ? 0.0f : 1.0f;
    }
  for (int s = 0; s < 5; ++s) {
    D[(size_t)rows * 512 + s] = s < 2 ? -0.5f : 0.5f;
    w[(size_t)rows * 512 + s] = 1.0f;
  }

  int64_t vs[4], fs[4], vs2[4], fs2[4];
  int32_t status = 0;
  CHECK(d3f_tsdf_sparse_mesh_host(D.data(), w.data(), lattice_start, brick_start, index.data(), coord.data(), origin,
                                  dims, voxel, V, 14, B, 1.0f, 0, 0, nullptr, nullptr, nullptr, vs, fs, &status) == 0);
  const int64_t nv = vs[V], nf = fs[V];
  printf("vertices %lld, triangles %lld, starts %lld %lld %lld / %lld %lld %lld, status %d\n", (long long)nv,
         (long long)nf, (long long)vs[0], (long long)vs[1], (long long)vs[2], (long long)fs[0], (long long)fs[1],
         (long long)fs[2], status);
  CHECK(nv > 0 && nf > 0 && vs[0] == 0 && vs[1] == nv && vs[2] == nv && fs[1] == nf && fs[2] == nf);   // 5 x 1 x 1: no cell
  CHECK(status == (D3F_TSDF_ST_OVERFLOW | D3F_TSDF_ST_FACE_OVERFLOW));
  std::vector<float> vert((size_t)nv * 3), norm((size_t)nv * 3);
  std::vector<int32_t> face((size_t)nf * 3);
  status = 0;
  CHECK(d3f_tsdf_sparse_mesh_host(D.data(), w.data(), lattice_start, brick_start, index.data(), coord.data(), origin,
                                  dims, voxel, V, 14, B, 1.0f, nv, nf, vert.data(), norm.data(), face.data(), vs2, fs2,
                                  &status) == 0);
  CHECK(status == 0 && memcmp(vs, vs2, sizeof vs) == 0 && memcmp(fs, fs2, sizeof fs) == 0);
  for (int64_t i = 0; i < 3 * nf; ++i) CHECK(face[(size_t)i] >= 0 && face[(size_t)i] < nv);
  for (int64_t i = 0; i < 3 * nv; ++i) CHECK(isfinite(vert[(size_t)i]) && isfinite(norm[(size_t)i]));
  const int64_t hv = nv / 2, hf = nf / 2 + 1;               // an odd face capacity cuts a quad in two
  std::vector<float> vert2((size_t)hv * 3), norm2((size_t)hv * 3);
  std::vector<int32_t> face2((size_t)hf * 3);
  status = 0;
  CHECK(d3f_tsdf_sparse_mesh_host(D.data(), w.data(), lattice_start, brick_start, index.data(), coord.data(), origin,
                                  dims, voxel, V, 14, B, 1.0f, hv, hf, vert2.data(), norm2.data(), face2.data(), vs2, fs2,
                                  &status) == 0);
  CHECK(status == (D3F_TSDF_ST_OVERFLOW | D3F_TSDF_ST_FACE_OVERFLOW));
  CHECK(memcmp(vs, vs2, sizeof vs) == 0 && memcmp(fs, fs2, sizeof fs) == 0);
  CHECK(memcmp(vert.data(), vert2.data(), vert2.size() * sizeof(float)) == 0);
  CHECK(memcmp(norm.data(), norm2.data(), norm2.size() * sizeof(float)) == 0);
  CHECK(memcmp(face.data(), face2.data(), face2.size() * sizeof(int32_t)) == 0);
  // no bricks at all: nothing is read from the pool
  const int64_t none[4] = {0, 0, 0, 0};
  std::vector<int32_t> absent(14, -1);
  status = 0;
  CHECK(d3f_tsdf_sparse_mesh_host(nullptr, nullptr, lattice_start, none, absent.data(), nullptr, origin, dims, voxel, V,
                                  14, 0, 1.0f, 0, 0, nullptr, nullptr, nullptr, vs2, fs2, &status) == 0);
  CHECK(status == 0 && vs2[V] == 0 && fs2[V] == 0);
  printf("ok\n");
  return 0;
}
