"""Times the mesh extraction of one fragment-sized TSDF volume against the point extraction of the SAME volume in the same
run (csrc/tsdf_mesh.hip against csrc/tsdf_extract.hip): the volume of profiles/tsdf_bench.py -- 50 synthetic depth
frames of 640 x 480 of the analytic room of tests/tsdf_scene.py scaled up 2.4 times, voxel 0.006 m, trunc 5 voxels,
about 2 x 10^8 voxels -- integrated once on the device.

  * d3f_tsdf_mesh_count (count + two scans), d3f_tsdf_mesh counted (emit), d3f_tsdf_mesh uncounted (both), and the same
    three of d3f_tsdf_extract: device events on the stream around each C-ABI call on tensors that are already on the
    device, REPEAT times after WARMUP runs, the two passes alternating; median, minimum, maximum;
  * the bytes the mesh pass must move (ops.tsdf_mesh_bytes) over its time, as a share of the HBM copy rate measured in
    MI355X_MICROARCH.md (6.29 TB/s, float4 copy);
  * the ratio mesh / extract, and what it means for staging an LDS tile of D / w (worth trying above about 3).

    python profiles/tsdf_mesh_bench.py            ->  profiles/tsdf_mesh_bench.txt

Needs the GPU; there is no fallback."""
import datetime
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import tsdf_bench as TB  # noqa: E402  (puts the repository and tests/ on the path)
from d3feat_pytorch_amd import _native, ops  # noqa: E402
from d3feat_pytorch_amd.datasets import fragments as fr  # noqa: E402

REPEAT, WARMUP = 9, 2
TILE_RATIO = 3.0


def timed_alternating(fns):
    """Milliseconds [len(fns), REPEAT] of the calls ``fns`` between device events, taken in turn, after WARMUP rounds."""
    for _ in range(WARMUP):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(REPEAT):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1))
    return np.array(out)


def main():
    assert torch.cuda.is_available(), "tsdf_mesh_bench needs the GPU"
    dev = torch.device('cuda')
    L = _native.lib()
    depth, poses = TB.make_sequence()
    F, voxel = TB.FRAMES, TB.VOXEL
    M = np.stack([fr.rigid_inverse(P) @ poses[0] for P in poses])
    C = np.stack([fr.rigid_inverse(poses[0]) @ P for P in poses])
    origin, dims = fr.place_volumes(ops.tsdf_bounds(depth, [0, F], TB.K, C).cpu().numpy(), voxel)
    D, w, tvs = ops.tsdf_integrate(depth, [0, F], TB.K, M, origin, dims, voxel, 5 * voxel)
    o, n, vx, _, vol_start = ops._tsdf_volumes(origin, dims, voxel, 1)
    total = int(vol_start[-1])
    to, tn, tvx = ops._on(dev, o, n, vx)
    stream = torch.cuda.current_stream().cuda_stream
    p = ops._p

    # sizes, through the public operators (which also checks one against the other)
    vertices, normals, faces, vertex_start, face_start = ops.tsdf_mesh(D, w, tvs, origin, dims, voxel)
    points, point_start = ops.tsdf_extract(D, w, tvs, origin, dims, voxel)
    nv, nf, npts = int(vertices.shape[0]), int(faces.shape[0]), int(points.shape[0])
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    mesh_bytes = L.d3f_tsdf_mesh_ws_bytes(total)
    mesh_ws = torch.empty(mesh_bytes, dtype=torch.uint8, device=dev)
    ext_bytes = L.d3f_tsdf_extract_ws_bytes(total)
    ext_ws = torch.empty(ext_bytes, dtype=torch.uint8, device=dev)

    def mesh_count():
        _native.check(L.d3f_tsdf_mesh_count(p(D), p(w), p(tvs), p(tn), 1, total, 1.0, p(vertex_start), p(face_start),
                                            p(mesh_ws), mesh_bytes, stream), "d3f_tsdf_mesh_count")

    def mesh(counted):
        _native.check(L.d3f_tsdf_mesh(p(D), p(w), p(tvs), p(to), p(tn), p(tvx), 1, total, 1.0, counted, nv, nf,
                                      p(vertices), p(normals), p(faces), p(vertex_start), p(face_start), p(status),
                                      p(mesh_ws), mesh_bytes, stream), "d3f_tsdf_mesh")

    def extract_count():
        _native.check(L.d3f_tsdf_extract_count(p(D), p(w), p(tvs), p(tn), 1, total, 1.0, p(point_start), p(ext_ws),
                                               ext_bytes, stream), "d3f_tsdf_extract_count")

    def extract(counted):
        _native.check(L.d3f_tsdf_extract(p(D), p(w), p(tvs), p(to), p(tn), p(tvx), 1, total, 1.0, counted, npts,
                                         p(points), p(point_start), p(status), p(ext_ws), ext_bytes, stream),
                      "d3f_tsdf_extract")

    ms_mc, ms_ec = timed_alternating([mesh_count, extract_count])          # the counts stay in the workspaces
    ms_me, ms_ee = timed_alternating([lambda: mesh(1), lambda: extract(1)])
    ms_m, ms_e = timed_alternating([lambda: mesh(0), lambda: extract(0)])
    assert int(status.item()) == 0 and int(vertex_start[1]) == nv and int(face_start[1]) == nf
    assert int(point_start[1]) == npts

    def line(name, ms):
        return "%-46s median %9.3f ms   min %9.3f   max %9.3f   (%d runs)" % (name, np.median(ms), ms.min(), ms.max(),
                                                                              len(ms))
    t_mesh, t_ext = float(np.median(ms_m)), float(np.median(ms_e))
    moved = ops.tsdf_mesh_bytes(total, nv, nf)
    ratio = t_mesh / t_ext
    out = ["Mesh extraction against point extraction on one fragment-sized volume: %d frames of %d x %d, voxel %g m, "
           "trunc %g m, room scaled %.1f x" % (F, TB.WIDTH, TB.HEIGHT, voxel, 5 * voxel, TB.SCALE),
           "device: %s (%s)   date: %s" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName,
                                           datetime.date.today().isoformat()), "",
           "volume: %d x %d x %d = %d voxels (%.2f GB of D and w); %.1f %% of them with w > 0"
           % (n[0, 0], n[0, 1], n[0, 2], total, 8e-9 * total, 100 * float((w > 0).float().mean().item())),
           "mesh: %d vertices, %d triangles;   cloud: %d points" % (nv, nf, npts), "",
           line("d3f_tsdf_mesh_count (count + 2 scans)", ms_mc), line("d3f_tsdf_mesh, counted (emit)", ms_me),
           line("d3f_tsdf_mesh (count + scans + emit)", ms_m), "",
           line("d3f_tsdf_extract_count (count + scan)", ms_ec), line("d3f_tsdf_extract, counted (emit)", ms_ee),
           line("d3f_tsdf_extract (count + scan + emit)", ms_e), "",
           "tsdf_mesh: %.0f bytes (tsdf_mesh_bytes) in %.3f ms = %.1f GB/s = %.1f %% of the %.2f TB/s HBM copy rate"
           % (moved, t_mesh, moved / t_mesh * 1e-6, 100 * moved / t_mesh * 1e-9 / TB.HBM_COPY_TBS, TB.HBM_COPY_TBS),
           "ratio tsdf_mesh / tsdf_extract on the same volume: %.2f" % ratio]
    if ratio <= TILE_RATIO:
        out.append("LDS tile of D / w: NOT staged.  The ratio is below %.0f: the mesh pass is a pass over the same 8 bytes "
                   "per voxel, a voxel that is not valid ends after one read of D and w, and the neighbourhood reads of "
                   "the others come from cache." % TILE_RATIO)
    else:
        out.append("LDS tile of D / w: the ratio is above %.0f, so a tile is worth trying (not staged in this build)."
                   % TILE_RATIO)
    text = "\n".join(out) + "\n"
    print(text)
    dest = os.environ.get("TSDF_MESH_BENCH_OUT", os.path.join(HERE, "tsdf_mesh_bench.txt"))
    with open(dest, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
