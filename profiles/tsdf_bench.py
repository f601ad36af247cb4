"""Times the TSDF fusion of one fragment at the benchmark's own size (datasets/fragments.py, csrc/tsdf.hip, csrc/tsdf_integrate.hip, csrc/tsdf_extract.hip): 50 synthetic
depth frames of 640 x 480 of the analytic room of tests/tsdf_scene.py scaled up 2.4 times, voxel 0.006 m, trunc 5 voxels
-- about 2 x 10^8 voxels.

  * fuse_fragments(device='cuda') end to end (host clock around a call that ends with the clouds on the host), after a
    warm-up call;
  * the bounds, integrate, extract-count (count + scan) and extract-emit launches on their own: device events around
    each C-ABI call on tensors that are already on the device, REPEAT times after a warm-up; median, minimum, maximum;
  * the bytes the integrate kernel must write (8 per voxel, nothing is read back from the volume) over its time, as a
    share of the HBM copy rate measured in MI355X_MICROARCH.md (6.29 TB/s, float4 copy), and the projections per
    second.  This shows whether the store stream bounds the kernel; it does not separate arithmetic from load latency;
  * the share of voxels that end with w > 0 (what a block-sparse volume would keep);
  * the NumPy restatement (ops.tsdf_numpy) on NUMPY_SLABS z planes spread evenly over the volume, host clock, scaled to
    all planes: an ESTIMATE of its time on the fragment, labelled as such.

    python profiles/tsdf_bench.py            ->  profiles/tsdf_bench.txt

Needs the GPU; there is no fallback."""
import datetime
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

import tsdf_scene as S  # noqa: E402
from d3feat_pytorch_amd import _native, ops  # noqa: E402
from d3feat_pytorch_amd.datasets import fragments as fr  # noqa: E402

REPEAT, WARMUP = 7, 2
SCALE, FRAMES, VOXEL = 2.4, 50, 0.006
WIDTH, HEIGHT = 640, 480
K = np.array([480.0, 480.0, 319.5, 239.5])
HBM_COPY_TBS = 6.29
NUMPY_SLABS = 8


def make_sequence():
    """50 cameras along the path of the room's first six, the room scaled by SCALE."""
    poses = []
    for j in range(FRAMES):
        i = 6.0 * j / FRAMES
        eye = np.array([0.25 + 0.04 * i, 0.6 + 0.01 * i, 0.25 + 0.01 * i]) * SCALE
        poses.append(S.look_at(eye, (S.CENTER + np.array([0.0, 0.01 * i, 0.01 * i])) * SCALE))
    poses = np.stack(poses)
    depth = np.stack([S.to_raw(S.render(P, WIDTH, HEIGHT, K, SCALE)) for P in poses])
    return depth, poses


def timed(fn):
    """Milliseconds of REPEAT runs of ``fn`` between device events, after WARMUP runs."""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPEAT):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return np.array(out)


def line(name, ms):
    return "%-46s median %9.3f ms   min %9.3f   max %9.3f   (%d runs)" % (name, np.median(ms), ms.min(), ms.max(), len(ms))


def main():
    assert torch.cuda.is_available(), "tsdf_bench needs the GPU"
    dev = torch.device('cuda')
    L = _native.lib()
    depth, poses = make_sequence()
    out = ["TSDF fusion of one fragment: %d frames of %d x %d, voxel %g m, trunc %g m, room scaled %.1f x"
           % (FRAMES, WIDTH, HEIGHT, VOXEL, 5 * VOXEL, SCALE),
           "device: %s (%s)   date: %s" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName,
                                           datetime.date.today().isoformat()), ""]

    # ---------------------------------------------------------------------------------------------- end to end
    fr.fuse_fragments(depth, K, poses, frames_per_fragment=FRAMES, voxel=VOXEL)          # warm-up
    wall = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        clouds, _ = fr.fuse_fragments(depth, K, poses, frames_per_fragment=FRAMES, voxel=VOXEL)
        wall.append((time.perf_counter() - t0) * 1e3)
    wall = np.array(wall)
    out.append(line("fuse_fragments(device='cuda'), host clock", wall))
    out.append("    (uploads the frames twice, reads the bounds and the point count back, copies the cloud to the host)")
    out.append("points of the fragment: %d" % len(clouds[0]))

    # ---------------------------------------------------------------------------------------------- the launches
    M = np.stack([fr.rigid_inverse(P) @ poses[0] for P in poses])
    C = np.stack([fr.rigid_inverse(poses[0]) @ P for P in poses])
    d, fs, Kf, Mf = ops._tsdf_frames(depth, [0, FRAMES], K, M)
    Cf = ops._tsdf_frames(depth, [0, FRAMES], K, C)[3]
    bounds = ops.tsdf_bounds(depth, [0, FRAMES], K, C).cpu().numpy()
    origin, dims = fr.place_volumes(bounds, VOXEL)
    o, n, vx, tr, vol_start = ops._tsdf_volumes(origin, dims, VOXEL, 1, 5 * VOXEL)
    total = int(vol_start[-1])
    td, tfs, tK, tM, tC, to, tn, tvx, ttr, tvs = ops._on(dev, d, fs, Kf, Mf, Cf, o, n, vx, tr, vol_start)
    D = torch.empty(total, dtype=torch.float32, device=dev)
    w = torch.empty(total, dtype=torch.float32, device=dev)
    tb = torch.empty((1, 6), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    p = ops._p

    def run_bounds():
        _native.check(L.d3f_tsdf_bounds(p(td), 0, FRAMES, HEIGHT, WIDTH, p(tfs), 1, p(tK), p(tC), 1000.0,
                                        ops.TSDF_DEPTH_MAX, p(tb), stream), "d3f_tsdf_bounds")

    def run_integrate():
        _native.check(L.d3f_tsdf_integrate(p(td), None, 0, 0, FRAMES, HEIGHT, WIDTH, p(tfs), p(tvs), 1, total, total,
                                           p(tK), p(tM), p(to), p(tn), p(tvx), p(ttr), 1000.0, ops.TSDF_DEPTH_MAX, 0,
                                           p(D), p(w), None, stream), "d3f_tsdf_integrate")

    nbytes = L.d3f_tsdf_extract_ws_bytes(total)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    point_start = torch.zeros(2, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def run_count():
        _native.check(L.d3f_tsdf_extract_count(p(D), p(w), p(tvs), p(tn), 1, total, 1.0, p(point_start), p(ws), nbytes,
                                               stream), "d3f_tsdf_extract_count")

    ms_bounds = timed(run_bounds)
    ms_integrate = timed(run_integrate)
    ms_count = timed(run_count)
    npts = int(point_start[1].item())
    points = torch.empty((npts, 3), dtype=torch.float32, device=dev)

    def run_emit():
        _native.check(L.d3f_tsdf_extract(p(D), p(w), p(tvs), p(to), p(tn), p(tvx), 1, total, 1.0, 1, npts, p(points),
                                         p(point_start), p(status), p(ws), nbytes, stream), "d3f_tsdf_extract")

    ms_emit = timed(run_emit)
    assert int(status.item()) == 0 and npts == len(clouds[0])
    seen = float((w > 0).float().mean().item())
    out += ["", "volume: %d x %d x %d = %d voxels (%.2f GB of D and w)" % (n[0, 0], n[0, 1], n[0, 2], total, 8e-9 * total),
            line("d3f_tsdf_bounds", ms_bounds), line("d3f_tsdf_integrate", ms_integrate),
            line("d3f_tsdf_extract_count (count + scan)", ms_count),
            line("d3f_tsdf_extract, counted (emit)", ms_emit), ""]
    t = np.median(ms_integrate) * 1e-3
    floor_ms = 8e-9 * total / HBM_COPY_TBS
    out.append("integrate: %.3f TB/s written = %.1f %% of the %.2f TB/s HBM copy rate (the store stream alone would take "
               "%.3f ms); %.3g projections/s (%d voxels x %d frames)"
               % (8e-12 * total / t, 100 * 8e-12 * total / t / HBM_COPY_TBS, HBM_COPY_TBS, floor_ms, total * FRAMES / t,
                  total, FRAMES))
    out.append("    bound: %s" % ("not the store stream; projection arithmetic against the latency of the depth gather is "
                                  "NOT separated by this measurement (no arithmetic floor computed, no counter run)"
                                  if np.median(ms_integrate) > 2 * floor_ms else "the store stream"))
    t = (np.median(ms_count) + np.median(ms_emit)) * 1e-3
    out.append("extract: reads D and w twice (count, emit): %.3f TB/s read = %.1f %% of the copy rate"
               % (16e-12 * total / t, 100 * 16e-12 * total / t / HBM_COPY_TBS))
    out.append("voxels that end with w > 0: %.1f %%" % (100 * seen))

    # ---------------------------------------------------------------------------------------------- NumPy
    # NUMPY_SLABS single z planes spread evenly over the volume, each swept as a volume of its own (the restatement's
    # equality with the device is what the tests check; here only its time is taken)
    nx, ny, nz = (int(a) for a in n[0])
    planes = [int((k + 0.5) * nz / NUMPY_SLABS) for k in range(NUMPY_SLABS)]
    t_np = 0.0
    for iz in planes:
        slab_origin = origin[0].copy()
        slab_origin[2] = origin[0][2] + np.float32(VOXEL) * np.float32(iz)
        t0 = time.perf_counter()
        ops.tsdf_numpy(depth, [0, FRAMES], K, M, [slab_origin], [[nx, ny, 1]], VOXEL, 5 * VOXEL)
        t_np += time.perf_counter() - t0
    out += ["", "NumPy restatement on %d of the %d z planes, spread evenly (%s): %.2f s"
            % (NUMPY_SLABS, nz, ", ".join(str(i) for i in planes), t_np),
            "    ESTIMATE for the whole fragment (x %d / %d): %.0f s = %.1f min"
            % (nz, NUMPY_SLABS, t_np * nz / NUMPY_SLABS, t_np * nz / NUMPY_SLABS / 60)]
    text = "\n".join(out) + "\n"
    print(text)
    dest = os.environ.get("TSDF_BENCH_OUT", os.path.join(HERE, "tsdf_bench.txt"))
    with open(dest, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
