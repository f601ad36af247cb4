"""Times what colour costs in the TSDF path (csrc/tsdf_color.hpp) on the fragment of profiles/tsdf_bench.py -- 50 frames
of 640 x 480 of the analytic room scaled 2.4 times, voxel 0.006 m, about 2 x 10^8 voxels -- painted with the analytic
texture ``tex`` of tests/rgbd_cases.py:

  * d3f_tsdf_integrate with channels = 0 against 1 and 3 channels, and with into = 1 without colour and with 3
    channels;
  * d3f_tsdf_sparse_integrate likewise, on the bricks of the same fragment;
  * ops.tsdf_raycast of 1 view and of 16 views of 640 x 480, without colour and with a 1- and a 3-channel volume;
  * ops.tsdf_sample_color on the extracted cloud, 1 and 3 channels.

The arm without colour is the code as it was before colour existed (its kernels are untouched) and is the baseline of
every ratio.  Device events around each call on tensors that are already on the device; the arms of a group take turns
inside one run (window k of every arm, then window k + 1), REPEAT windows after WARMUP rounds; median, minimum, maximum.
Bytes are counted from the shapes: what a kernel must write, and the colour it must gather.

    python profiles/tsdf_color_bench.py            ->  profiles/tsdf_color_bench.txt

Needs the GPU; there is no fallback."""
import datetime
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, HERE)

import rgbd_cases as RC  # noqa: E402
import tsdf_bench as TB  # noqa: E402
from d3feat_pytorch_amd import _native, ops  # noqa: E402
from d3feat_pytorch_amd.datasets import fragments as fr  # noqa: E402

REPEAT, WARMUP = 10, 2
VIEWS = 16


def paint(depth, poses):
    """f32 [F,H,W] intensity: ``tex`` at every pixel's world point, one frame at a time."""
    return np.concatenate([RC.paint(depth[f:f + 1], TB.K, poses[f:f + 1]) for f in range(depth.shape[0])])


def take_turns(arms):
    """name -> milliseconds [REPEAT] of the callables ``arms`` (name -> fn), one window each per round."""
    for _ in range(WARMUP):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in arms}
    for _ in range(REPEAT):
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1))
    return {name: np.array(ms) for name, ms in out.items()}


def report(out, title, ms, base, note):
    out.append(title)
    ref = np.median(ms[base])
    for name, t in ms.items():
        out.append("    %-28s median %9.3f ms   min %9.3f   max %9.3f   (%d windows)   x %.3f   %s"
                   % (name, np.median(t), t.min(), t.max(), len(t), np.median(t) / ref, note.get(name, "")))
    out.append("")


def main():
    assert torch.cuda.is_available(), "tsdf_color_bench needs the GPU"
    dev = torch.device('cuda')
    L = _native.lib()
    p = ops._p
    stream = torch.cuda.current_stream().cuda_stream
    F, H, W, VOXEL = TB.FRAMES, TB.HEIGHT, TB.WIDTH, TB.VOXEL
    trunc = 5 * VOXEL
    depth, poses = TB.make_sequence()
    inten = paint(depth, poses)
    frames = {1: ops.tsdf_color_frames(inten, depth.shape), 3: ops.tsdf_color_frames(RC.to_rgb8(inten), depth.shape)}
    out = ["Colour in the TSDF path: %d frames of %d x %d, voxel %g m, trunc %g m, room scaled %.1f x, painted with tex"
           % (F, W, H, VOXEL, trunc, TB.SCALE),
           "device: %s (%s)   date: %s" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName,
                                           datetime.date.today().isoformat()),
           "arms take turns inside one run; x = median over the median of the arm without colour", ""]

    M = np.stack([fr.rigid_inverse(P) @ poses[0] for P in poses])
    C = np.stack([fr.rigid_inverse(poses[0]) @ P for P in poses])
    d, fs, Kf, Mf = ops._tsdf_frames(depth, [0, F], TB.K, M)
    bounds = ops.tsdf_bounds(depth, [0, F], TB.K, C).cpu().numpy()
    origin, dims = fr.place_volumes(bounds, VOXEL)
    o, n, vx, tr, vol_start = ops._tsdf_volumes(origin, dims, VOXEL, 1, trunc)
    total = int(vol_start[-1])
    td, tfs, tK, tM, to, tn, tvx, ttr, tvs = ops._on(dev, d, fs, Kf, Mf, o, n, vx, tr, vol_start)
    tc = {c: ops._on(dev, a)[0] for c, a in frames.items()}
    D = torch.empty(total, dtype=torch.float32, device=dev)
    w = torch.empty(total, dtype=torch.float32, device=dev)
    Cv = {c: torch.empty((total, c), dtype=torch.float32, device=dev) for c in (1, 3)}
    out.append("volume: %d x %d x %d = %d voxels; D and w %.2f GB, + %.2f GB (1 channel) or %.2f GB (3 channels)"
               % (n[0, 0], n[0, 1], n[0, 2], total, 8e-9 * total, 4e-9 * total, 12e-9 * total))
    out.append("")

    # ------------------------------------------------------------------------------------------------ integrate
    tc[0], Cv[0] = None, None                            # channels = 0: no colour frames, no colour volume
    rest = (0, F, H, W, p(tfs), p(tvs), 1, total, total, p(tK), p(tM), p(to), p(tn), p(tvx), p(ttr), 1000.0,
            ops.TSDF_DEPTH_MAX)

    def dense(c, into=0):
        args = (p(td), p(tc[c]), c) + rest + (into, p(D), p(w), p(Cv[c]), stream)
        return lambda: _native.check(L.d3f_tsdf_integrate(*args), "d3f_tsdf_integrate")
    ms = take_turns({"Cc = %d" % c: dense(c) for c in (0, 1, 3)})
    report(out, "integrate (d3f_tsdf_integrate), one launch", ms, "Cc = 0",
           {"Cc = %d" % c: "writes %.2f GB" % ((8 + 4 * c) * 1e-9 * total) for c in (0, 1, 3)})
    ms = take_turns({"Cc = %d" % c: dense(c, 1) for c in (0, 3)})            # continues what the arms above left
    report(out, "integrate into (d3f_tsdf_integrate, into = 1), one launch", ms, "Cc = 0",
           {"Cc = %d" % c: "reads and writes %.2f GB" % ((8 + 4 * c) * 1e-9 * total) for c in (0, 3)})
    for c in (0, 1, 3):                                  # the ray-cast and the sampling below read a volume fused once
        dense(c)()

    # ------------------------------------------------------------------------------------------- sparse integrate
    sv = ops.tsdf_allocate(depth, [0, F], TB.K, C, origin, dims, VOXEL, trunc)
    tls, bs, bi, bc, so, sn, svx = ops._sparse_tables(sv, dev)
    B = sv.bricks
    slots = B * ops.TSDF_BRICK_VOXELS
    Dp = torch.empty(slots, dtype=torch.float32, device=dev)
    wp = torch.empty(slots, dtype=torch.float32, device=dev)
    Cp = {c: torch.empty((slots, c), dtype=torch.float32, device=dev) for c in (1, 3)}
    Cp[0] = None
    srest = (0, F, H, W, p(tfs), 1, p(tK), p(tM), p(so), p(sn), p(svx), p(ttr), p(bs), p(bc), B, 1000.0,
             ops.TSDF_DEPTH_MAX)

    def sparse(c, into=0):
        args = (p(td), p(tc[c]), c) + srest + (into, p(Dp), p(wp), p(Cp[c]), stream)
        return lambda: _native.check(L.d3f_tsdf_sparse_integrate(*args), "d3f_tsdf_sparse_integrate")
    ms = take_turns({"Cc = %d" % c: sparse(c) for c in (0, 1, 3)})
    report(out, "sparse integrate, %d bricks of %d (%.1f %% of the lattice)" % (B, int(sv.lattice_start[-1]),
                                                                              100.0 * B / int(sv.lattice_start[-1])),
           ms, "Cc = 0", {"Cc = %d" % c: "writes %.3f GB" % ((8 + 4 * c) * 1e-9 * slots) for c in (0, 1, 3)})
    ms = take_turns({"Cc = %d" % c: sparse(c, 1) for c in (0, 3)})
    report(out, "sparse integrate into, the same bricks", ms, "Cc = 0",
           {"Cc = %d" % c: "reads and writes %.3f GB" % ((8 + 4 * c) * 1e-9 * slots) for c in (0, 3)})

    # -------------------------------------------------------------------------------------------------- ray-cast
    for views in (1, VIEWS):
        args = (D, w, tvs, origin, dims, VOXEL, trunc, TB.K, C[:views], H, W, [0] * views)

        def cast(c, args=args):
            return (lambda: ops.tsdf_raycast(*args)) if c == 0 else (lambda: ops.tsdf_raycast(*args, color=Cv[c]))
        ms = take_turns({"Cc = %d" % c: cast(c) for c in (0, 1, 3)})
        report(out, "ray-cast (ops.tsdf_raycast), %d view%s of %d x %d" % (views, "" if views == 1 else "s", W, H), ms,
               "Cc = 0", {"Cc = %d" % c: "writes %.1f MB" % ((4 + 4 * c) * 1e-6 * views * H * W) for c in (0, 1, 3)})

    # ---------------------------------------------------------------------------------------------------- sample
    pts, ps = ops.tsdf_extract(D, w, tvs, origin, dims, VOXEL)
    N = int(pts.shape[0])
    ms = take_turns({"Cc = %d" % c: (lambda c=c: ops.tsdf_sample_color(Cv[c], w, tvs, origin, dims, VOXEL, pts, ps))
                     for c in (1, 3)})
    report(out, "ops.tsdf_sample_color on the extracted cloud, %d points (x: against one channel)" % N, ms, "Cc = 1",
           {"Cc = %d" % c: "reads %.1f MB of corners, writes %.1f MB" % ((32 + 32 * c) * 1e-6 * N, 4 * c * 1e-6 * N)
            for c in (1, 3)})

    text = "\n".join(out) + "\n"
    print(text)
    dest = os.environ.get("TSDF_COLOR_BENCH_OUT", os.path.join(HERE, "tsdf_color_bench.txt"))
    with open(dest, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
