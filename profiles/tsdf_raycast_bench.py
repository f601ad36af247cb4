"""Times the ray-caster (ops.tsdf_raycast, csrc/tsdf_raycast.hip) and the frame-to-model pass of track_sequence that is
built on it:

    python profiles/tsdf_raycast_bench.py            ->  profiles/tsdf_raycast_bench.txt

  * the fragment of profiles/tsdf_bench.py (50 frames of 640 x 480, voxel 0.006 m, about 2 x 10^8 voxels) is fused once;
    d3f_tsdf_raycast then renders ONE 640 x 480 view of it and a batch of 16 views, each with the box clip on and
    off: device events around the C-ABI call on buffers made beforehand, the four arms taking turns, medians after a
    warm-up.  The clipped and the unclipped images are compared bit for bit;
  * for scale, on the same volume: d3f_tsdf_extract (count + scan + emit into a sized buffer) and one streaming pass over
    the bytes of D and w (two reductions by torch);
  * the 50-frame sequence of profiles/odometry_bench.py tracked by fragments.track_sequence frame to frame and with
    model=dict(frames_per_fragment=50, voxel=0.01): host clock around calls that end with the poses on the host,
    after a warm-up call, the two taking turns; the model pass's share per step (49 steps: ray-cast, pyramid, odometry,
    one read-back, integrate) and the error of the last frame against the analytic pose;
  * the kernel's register and scratch figures as the compiler reports them (-Rpass-analysis=kernel-resource-usage on
    csrc/tsdf_raycast.hip with the library's own flags), when hipcc is there.

Needs the GPU; there is no fallback."""
import datetime
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
sys.path.insert(0, HERE)

import odometry_bench as OB  # noqa: E402
import tsdf_bench as TB  # noqa: E402
from d3feat_pytorch_amd import _native, ops  # noqa: E402
from d3feat_pytorch_amd.datasets import fragments as fr  # noqa: E402

REPS = 7
BATCH = 16
MODEL = dict(frames_per_fragment=50, voxel=0.01)


def kernel_resources():
    """The compiler's report for raycast_kernel<Volumes, 0>, or None when there is no hipcc."""
    src = os.path.join(_native.CSRC, "tsdf_raycast.hip")
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-pass-failed", "-fPIC",
               "-I" + os.path.join(REPO, "include"), "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
               os.path.join(tmp, "raycast.o")]
        try:
            text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, check=True, cwd=tmp,
                                  universal_newlines=True).stdout
        except (OSError, subprocess.CalledProcessError):
            return None
    block = text[text.find("raycast_kernelIN3d3f4tsdf7VolumesELi0E"):]       # raycast_kernel<Volumes, 0>, mangled
    out = {}
    for key in ("VGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "VGPRs Spill",
                "LDS Size [bytes/block]"):
        m = re.search(r" %s: (\d+)" % re.escape(key), block)
        if m:
            out[key] = int(m.group(1))
    return out


def main():
    assert torch.cuda.is_available(), "tsdf_raycast_bench needs the GPU"
    dev = torch.device('cuda')
    L, p, stream = _native.lib(), ops._p, torch.cuda.current_stream().cuda_stream
    out = []

    def say(s=""):
        print(s, flush=True)
        out.append(s)

    say("Ray-casting the fragment of tsdf_bench.py: %d frames of %d x %d, voxel %g m, trunc %g m, step trunc / 2"
        % (TB.FRAMES, TB.WIDTH, TB.HEIGHT, TB.VOXEL, 5 * TB.VOXEL))
    say("device: %s (%s)   date: %s" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName,
                                        datetime.date.today().isoformat()))
    say()

    # ------------------------------------------------------------------------------------------------ the volume
    depth, poses = TB.make_sequence()
    M = np.stack([fr.rigid_inverse(P) @ poses[0] for P in poses])
    C = np.stack([fr.rigid_inverse(poses[0]) @ P for P in poses])
    origin, dims = fr.place_volumes(ops.tsdf_bounds(depth, [0, TB.FRAMES], TB.K, C).cpu().numpy(), TB.VOXEL)
    trunc = 5 * TB.VOXEL
    D, w, tvs = ops.tsdf_integrate(depth, [0, TB.FRAMES], TB.K, M, origin, dims, TB.VOXEL, trunc)
    total = int(D.numel())
    say("volume: %d x %d x %d = %d voxels (%.2f GB of D and w)" % (dims[0, 0], dims[0, 1], dims[0, 2], total,
                                                                  8e-9 * total))
    o, n, vx, _, _ = ops._tsdf_volumes(origin, dims, TB.VOXEL, 1)
    views = list(range(0, TB.FRAMES, 3))[:BATCH]
    vv, Kv, Cv, st, H, W = ops._raycast_views(1, trunc, TB.K, C[views], TB.HEIGHT, TB.WIDTH, [0] * BATCH, None,
                                              ops.RAYCAST_DEPTH_MIN, ops.TSDF_DEPTH_MAX)
    to, tn, tvx, tvv, tK, tC, tst = ops._on(dev, o, n, vx, vv, Kv, Cv, st)
    images = {(R, clip): torch.empty((R, H, W), dtype=torch.float32, device=dev) for R in (1, BATCH) for clip in (1, 0)}
    samples = int((ops.TSDF_DEPTH_MAX - ops.RAYCAST_DEPTH_MIN) / float(st[0])) + 1

    def cast(R, clip):
        def run():
            _native.check(L.d3f_tsdf_raycast(p(D), p(w), None, 0, p(tvs), p(to), p(tn), p(tvx), 1, total, p(tvv), R, H,
                                             W, p(tK), p(tC), p(tst), ops.RAYCAST_DEPTH_MIN, ops.TSDF_DEPTH_MAX, 1.0,
                                             clip, p(images[(R, clip)]), None, None, stream), "d3f_tsdf_raycast")
        return run

    arms = {"1 view, clip on": cast(1, 1), "1 view, clip off": cast(1, 0), "%d views, clip on" % BATCH: cast(BATCH, 1),
            "%d views, clip off" % BATCH: cast(BATCH, 0)}
    ms, spread = OB.medians(arms, REPS)
    for R in (1, BATCH):
        assert OB.same(images[(R, 1)], images[(R, 0)]), "the clip changed a bit"
    hit = float((images[(BATCH, 1)] > 0).float().mean())
    truth = np.stack([TB.S.render(poses[f], TB.WIDTH, TB.HEIGHT, TB.K, TB.SCALE) for f in views[:2]])
    got = images[(BATCH, 1)][:2].cpu().numpy()
    err = np.abs(got - truth)[got > 0]
    say("d3f_tsdf_raycast, 640 x 480, up to %d samples per ray at step %g m; medians of %d (range); clipped == unclipped "
        "bit for bit" % (samples, float(st[0]), REPS))
    for name in arms:
        R = 1 if name.startswith("1 ") else BATCH
        say("  %-22s %9.3f ms  (%.3f..%.3f) = %.3f ms per view, %.1f ns per ray"
            % ((name, ms[name]) + spread[name] + (ms[name] / R, 1e6 * ms[name] / (R * H * W))))
    say("  the clip is worth %.1f x on one view and %.1f x on the batch; the batch of %d takes %.1f x one view"
        % (ms["1 view, clip off"] / ms["1 view, clip on"],
           ms["%d views, clip off" % BATCH] / ms["%d views, clip on" % BATCH], BATCH,
           ms["%d views, clip on" % BATCH] / ms["1 view, clip on"]))
    say("  hit share of the batch %.4f; first two views against the analytic depth: %.4f of the hits within a voxel, "
        "median %.3f mm" % (hit, float((err <= TB.VOXEL).mean()), 1e3 * float(np.median(err))))

    # ------------------------------------------------------------------------------------------------ for scale
    pts, ps = ops.tsdf_extract(D, w, tvs, origin, dims, TB.VOXEL)
    npts = int(ps[-1])
    scale_arms = {"extract": lambda: ops.tsdf_extract(D, w, tvs, origin, dims, TB.VOXEL, capacity=npts),
                  "stream": lambda: (D.sum(), w.sum())}
    ms2, spread2 = OB.medians(scale_arms, REPS)
    say()
    say("for scale, the same volume:")
    say("  ops.tsdf_extract into %d rows (count, scan, emit)  %9.3f ms  (%.3f..%.3f)" % ((npts, ms2["extract"]) +
                                                                                       spread2["extract"]))
    say("  one streaming pass over D and w (two torch sums)      %9.3f ms  (%.3f..%.3f) = %.2f TB/s"
        % ((ms2["stream"],) + spread2["stream"] + (8e-12 * total / (ms2["stream"] * 1e-3),)))
    say("  one clipped view takes %.2f x the streaming pass and %.2f x the extraction"
        % (ms["1 view, clip on"] / ms2["stream"], ms["1 view, clip on"] / ms2["extract"]))
    del D, w, pts, images

    # ------------------------------------------------------------------------------------------------ tracking
    sdepth, sK, sposes = OB.make_sequence(50, 640, 480)
    truth = np.linalg.inv(sposes[0]) @ sposes[-1]

    def track(model):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fr.track_sequence(sdepth, sK, model=model)
        return 1e3 * (time.perf_counter() - t0), res

    track(None), track(MODEL)                                   # warm-up
    t_ff, t_mo = [], []
    for _ in range(3):
        a, res_ff = track(None)
        b, res_mo = track(MODEL)
        t_ff.append(a)
        t_mo.append(b)
    t_ff, t_mo = float(np.median(t_ff)), float(np.median(t_mo))
    steps = sdepth.shape[0] - 1
    say()
    say("track_sequence on the 50 frames of odometry_bench.py (640 x 480, clean depth), host clock, medians of 3:")
    say("  frame to frame                                  %9.1f ms; frame 49 off by %.4f deg / %.3f mm"
        % ((t_ff,) + OB.pose_error(res_ff[0][-1], truth)))
    say("  with model=%s   %9.1f ms; frame 49 off by %.4f deg / %.3f mm; model_status != 0 on %d pairs"
        % ((MODEL, t_mo) + OB.pose_error(res_mo[0][-1], truth) + (int((res_mo[2] != 0).sum()),)))
    say("  the model pass adds %.1f ms = %.2f ms per step (%d steps: ray-cast, pyramid, odometry, one read-back, "
        "integrate)" % (t_mo - t_ff, (t_mo - t_ff) / steps, steps))

    # ------------------------------------------------------------------------------------------------ the kernel
    res = kernel_resources()
    say()
    say("raycast_kernel<Volumes, 0> as compiled for gfx950: %s" % (", ".join("%s %d" % kv for kv in res.items()) if res else
                                                        "not measured (no hipcc here)"))
    text = "\n".join(out) + "\n"
    dest = os.environ.get("TSDF_RAYCAST_BENCH_OUT", os.path.join(HERE, "tsdf_raycast_bench.txt"))
    with open(dest, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
