"""Sparse against dense TSDF fusion of one fragment, in one run, at the size of profiles/tsdf_bench.py (whose sequence,
timer and line format this uses): 50 synthetic depth frames of 640 x 480 of the analytic room of tests/tsdf_scene.py
scaled up 2.4 times, voxel 0.006 m, trunc 0.03 m.

  * the dense integrate, extract-count and extract-emit launches (csrc/tsdf_integrate.hip, csrc/tsdf_extract.hip), unchanged;
  * the sparse mark, index, integrate, extract-count and extract-emit launches (csrc/tsdf_sparse.hip and the same two files): device events
    around each C-ABI call on tensors that are already on the device, REPEAT times after a warm-up; median, minimum,
    maximum;
  * allocated bricks over lattice bricks, and the bytes of the sparse volume (pool plus tables, ops.tsdf_sparse_bytes)
    over the bytes of the dense one (8 per voxel) -- the figure the sparse volumes exist for;
  * the share of slots in allocated bricks that end with w > 0, and of those that are valid (|D| < 1): what a tighter
    allocation could still save;
  * a check that the sparse points are the dense points as a set of rows, bit for bit.
No pass mark is set for the times: what is measured is written down, also where sparse is slower.

    python profiles/tsdf_sparse_bench.py            ->  profiles/tsdf_sparse_bench.txt

Needs the GPU; there is no fallback."""
import datetime
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import tsdf_bench as B  # noqa: E402  (puts the repository and tests/ on the path)
from d3feat_pytorch_amd import _native, ops  # noqa: E402
from d3feat_pytorch_amd.datasets import fragments as fr  # noqa: E402

TRUNC = 5 * B.VOXEL


def sorted_rows(points):
    u = points.cpu().numpy().view(np.uint32).reshape(-1, 3)
    return u[np.lexsort((u[:, 2], u[:, 1], u[:, 0]))]


def main():
    assert torch.cuda.is_available(), "tsdf_sparse_bench needs the GPU"
    dev = torch.device('cuda')
    L = _native.lib()
    depth, poses = B.make_sequence()
    F, H, W = B.FRAMES, B.HEIGHT, B.WIDTH
    out = ["Sparse against dense TSDF fusion of one fragment: %d frames of %d x %d, voxel %g m, trunc %g m, room "
           "scaled %.1f x" % (F, W, H, B.VOXEL, TRUNC, B.SCALE),
           "device: %s (%s)   date: %s" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName,
                                           datetime.date.today().isoformat()), ""]
    M = np.stack([fr.rigid_inverse(P) @ poses[0] for P in poses])
    C = np.stack([fr.rigid_inverse(poses[0]) @ P for P in poses])
    d, fs, Kf, Mf = ops._tsdf_frames(depth, [0, F], B.K, M)
    Cf = ops._tsdf_frames(depth, [0, F], B.K, C)[3]
    origin, dims = fr.place_volumes(ops.tsdf_bounds(depth, [0, F], B.K, C).cpu().numpy(), B.VOXEL)
    o, n, vx, tr, vol_start = ops._tsdf_volumes(origin, dims, B.VOXEL, 1, TRUNC)
    total = int(vol_start[-1])
    ls = ops._lattice_start(n)
    lattice = int(ls[-1])
    td, tfs, tK, tM, tC, to, tn, tvx, ttr, tvs, tls = ops._on(dev, d, fs, Kf, Mf, Cf, o, n, vx, tr, vol_start, ls)
    stream = torch.cuda.current_stream().cuda_stream
    p, check, dmax = ops._p, _native.check, ops.TSDF_DEPTH_MAX

    # ------------------------------------------------------------------------------------------------ sparse
    flags = torch.empty(lattice, dtype=torch.int32, device=dev)
    brick_index = torch.empty(lattice, dtype=torch.int32, device=dev)
    coord = torch.empty((lattice, 3), dtype=torch.int32, device=dev)
    brick_start = torch.zeros(2, dtype=torch.int64, device=dev)
    index_bytes = L.d3f_tsdf_sparse_index_ws_bytes(lattice)
    index_ws = torch.empty(index_bytes, dtype=torch.uint8, device=dev)

    def run_mark():
        check(L.d3f_tsdf_sparse_mark(p(td), 0, F, H, W, p(tfs), 1, p(tK), p(tC), p(to), p(tn), p(tvx), p(ttr), p(tls),
                                     lattice, 1000.0, dmax, p(flags), stream), "d3f_tsdf_sparse_mark")

    def run_index():
        check(L.d3f_tsdf_sparse_index(p(flags), p(tls), p(tn), 1, lattice, p(brick_index), p(coord), p(brick_start),
                                      p(index_ws), index_bytes, stream), "d3f_tsdf_sparse_index")

    ms_mark = B.timed(run_mark)
    ms_index = B.timed(run_index)
    bricks = int(brick_start[1].item())
    sv = ops.SparseVolumes(brick_index, coord[:bricks].clone(), brick_start, o, n, vx)
    Ds = torch.empty((bricks, 512), dtype=torch.float32, device=dev)
    ws_ = torch.empty((bricks, 512), dtype=torch.float32, device=dev)

    def run_sparse_integrate():
        check(L.d3f_tsdf_sparse_integrate(p(td), None, 0, 0, F, H, W, p(tfs), 1, p(tK), p(tM), p(to), p(tn), p(tvx),
                                          p(ttr), p(brick_start), p(sv.brick_coord), bricks, 1000.0, dmax, 0, p(Ds),
                                          p(ws_), None, stream), "d3f_tsdf_sparse_integrate")

    sparse_bytes_ws = L.d3f_tsdf_sparse_extract_ws_bytes(bricks)
    sparse_ws = torch.empty(sparse_bytes_ws, dtype=torch.uint8, device=dev)
    sparse_start = torch.zeros(2, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    tables = (p(tls), p(brick_start), p(brick_index), p(sv.brick_coord))

    def run_sparse_count():
        check(L.d3f_tsdf_sparse_extract_count(p(Ds), p(ws_), *tables, p(tn), 1, lattice, bricks, 1.0, p(sparse_start),
                                              p(sparse_ws), sparse_bytes_ws, stream), "d3f_tsdf_sparse_extract_count")

    ms_sparse_integrate = B.timed(run_sparse_integrate)
    ms_sparse_count = B.timed(run_sparse_count)
    npts = int(sparse_start[1].item())
    sparse_points = torch.empty((npts, 3), dtype=torch.float32, device=dev)

    def run_sparse_emit():
        check(L.d3f_tsdf_sparse_extract(p(Ds), p(ws_), *tables, p(to), p(tn), p(tvx), 1, lattice, bricks, 1.0, 1, npts,
                                        p(sparse_points), p(sparse_start), p(status), p(sparse_ws), sparse_bytes_ws,
                                        stream), "d3f_tsdf_sparse_extract")

    ms_sparse_emit = B.timed(run_sparse_emit)
    assert int(status.item()) == 0
    seen = float((ws_ > 0).float().mean().item())
    valid = float(((ws_ >= 1) & (Ds.abs() < 1)).float().mean().item())
    sparse_bytes = ops.tsdf_sparse_bytes(sv)
    sparse_rows = sorted_rows(sparse_points)
    del Ds, ws_, sparse_points, sparse_ws

    # ------------------------------------------------------------------------------------------------- dense
    D = torch.empty(total, dtype=torch.float32, device=dev)
    w = torch.empty(total, dtype=torch.float32, device=dev)

    def run_integrate():
        check(L.d3f_tsdf_integrate(p(td), None, 0, 0, F, H, W, p(tfs), p(tvs), 1, total, total, p(tK), p(tM), p(to),
                                   p(tn), p(tvx), p(ttr), 1000.0, dmax, 0, p(D), p(w), None, stream),
              "d3f_tsdf_integrate")

    nbytes = L.d3f_tsdf_extract_ws_bytes(total)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    point_start = torch.zeros(2, dtype=torch.int64, device=dev)

    def run_count():
        check(L.d3f_tsdf_extract_count(p(D), p(w), p(tvs), p(tn), 1, total, 1.0, p(point_start), p(ws), nbytes, stream),
              "d3f_tsdf_extract_count")

    ms_integrate = B.timed(run_integrate)
    ms_count = B.timed(run_count)
    assert int(point_start[1].item()) == npts, "the sparse and the dense volume give different numbers of points"
    points = torch.empty((npts, 3), dtype=torch.float32, device=dev)

    def run_emit():
        check(L.d3f_tsdf_extract(p(D), p(w), p(tvs), p(to), p(tn), p(tvx), 1, total, 1.0, 1, npts, p(points),
                                 p(point_start), p(status), p(ws), nbytes, stream), "d3f_tsdf_extract")

    ms_emit = B.timed(run_emit)
    assert int(status.item()) == 0
    same = np.array_equal(sorted_rows(points), sparse_rows)
    assert same, "the sparse points are not the dense points as a set of rows"

    dense_bytes = 8 * total
    med = np.median
    out += ["volume: %d x %d x %d = %d voxels; brick lattice %d x %d x %d = %d bricks"
            % (n[0, 0], n[0, 1], n[0, 2], total, (n[0, 0] + 7) // 8, (n[0, 1] + 7) // 8, (n[0, 2] + 7) // 8, lattice),
            "allocated bricks: %d of %d = %.1f %%" % (bricks, lattice, 100.0 * bricks / lattice),
            "bytes: sparse %d (pool %d + tables %d) over dense %d = %.1f %%   (%.3f GB against %.3f GB)"
            % (sparse_bytes, 4096 * bricks, sparse_bytes - 4096 * bricks, dense_bytes, 100.0 * sparse_bytes / dense_bytes,
               1e-9 * sparse_bytes, 1e-9 * dense_bytes),
            "slots of allocated bricks that end with w > 0: %.1f %%; that are valid (w >= 1, |D| < 1): %.1f %%"
            % (100 * seen, 100 * valid),
            "points: %d, the same rows bit for bit from both volumes: %s" % (npts, same), "",
            "dense (csrc/tsdf.hip)",
            B.line("d3f_tsdf_integrate", ms_integrate),
            B.line("d3f_tsdf_extract_count (count + scan)", ms_count),
            B.line("d3f_tsdf_extract, counted (emit)", ms_emit), "",
            "sparse (csrc/tsdf_sparse.hip)",
            B.line("d3f_tsdf_sparse_mark", ms_mark),
            B.line("d3f_tsdf_sparse_index (scan + tables)", ms_index),
            B.line("d3f_tsdf_sparse_integrate", ms_sparse_integrate),
            B.line("d3f_tsdf_sparse_extract_count (count + scan)", ms_sparse_count),
            B.line("d3f_tsdf_sparse_extract, counted (emit)", ms_sparse_emit), ""]
    dense_sum = med(ms_integrate) + med(ms_count) + med(ms_emit)
    sparse_sum = med(ms_mark) + med(ms_index) + med(ms_sparse_integrate) + med(ms_sparse_count) + med(ms_sparse_emit)
    out += ["medians summed: dense integrate + count + emit %.3f ms; sparse mark + index + integrate + count + emit %.3f "
            "ms = %.2f x the dense" % (dense_sum, sparse_sum, sparse_sum / dense_sum),
            "sparse mark + integrate %.3f ms against dense integrate %.3f ms = %.2f x"
            % (med(ms_mark) + med(ms_sparse_integrate), med(ms_integrate),
               (med(ms_mark) + med(ms_sparse_integrate)) / med(ms_integrate)),
            "projections per second, integrate alone: dense %.3g (%d voxels x %d frames), sparse %.3g (%d slots x %d frames)"
            % (total * F / (med(ms_integrate) * 1e-3), total, F, 512.0 * bricks * F / (med(ms_sparse_integrate) * 1e-3),
               512 * bricks, F)]
    text = "\n".join(out) + "\n"
    print(text)
    dest = os.environ.get("TSDF_SPARSE_BENCH_OUT", os.path.join(HERE, "tsdf_sparse_bench.txt"))
    with open(dest, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
