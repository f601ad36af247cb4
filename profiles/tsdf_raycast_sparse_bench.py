"""Times the sparse ray-caster (ops.tsdf_raycast_sparse, csrc/tsdf_raycast.hip) against the dense one and against
the only route there was before it, and the frame-to-model pass of track_sequence with a sparse model:

    python profiles/tsdf_raycast_sparse_bench.py            ->  profiles/tsdf_raycast_sparse_bench.txt

  * the fragment of profiles/tsdf_bench.py (50 frames of 640 x 480, voxel 0.006 m) is fused once into a sparse pool and
    once into the dense volume.  d3f_tsdf_raycast_sparse renders ONE 640 x 480 view and a batch of 16, each with the
    brick skip on and off, and d3f_tsdf_raycast renders the same views of the dense volume: device events around the
    C-ABI call on buffers made beforehand, the six arms taking turns, medians after a warm-up, the range next to them.
    All images of a view are compared bit for bit (for this fragment the sparse render equals the dense one);
  * ops.tsdf_densify + ops.tsdf_raycast on the same views, the route of the parent commit: host clock around calls that
    end with a synchronisation (the scatter's indices are made on the host), after a warm-up;
  * the bytes of both representations;
  * how many samples of a ray fall into absent bricks (counted on the device by plain tensor arithmetic that restates
    the base-voxel lookup, over the clipped range up to the hit): the number a second skipping level would be judged on;
  * the 50-frame sequence of profiles/odometry_bench.py tracked with model=dict(frames_per_fragment=50, voxel=0.01),
    dense and sparse, and sparse at voxel 0.006: host clock, after a warm-up call, the arms taking turns;
  * the kernels' register and scratch figures as the compiler reports them, when hipcc is there.

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


def kernel_resources(kernel, source="tsdf_raycast.hip"):
    """The compiler's report for the kernel of csrc/``source`` whose mangled name holds ``kernel``, or None when there
    is no hipcc."""
    src = os.path.join(_native.CSRC, source)
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-pass-failed", "-fPIC",
               "-I" + os.path.join(REPO, "include"), "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o",
               os.path.join(tmp, "kernel.o")]
        try:
            text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, check=True, cwd=tmp,
                                  universal_newlines=True).stdout
        except (OSError, subprocess.CalledProcessError):
            return None
    block = text[text.find(kernel):]
    out = {}
    for key in ("VGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "VGPRs Spill",
                "LDS Size [bytes/block]"):
        m = re.search(r" %s: (\d+)" % re.escape(key), block)
        if m:
            out[key] = int(m.group(1))
    return out


def absent_samples(sv, bi, K, C, H, W, step, depth, dev):
    """(samples inside the lattice, of them in absent bricks), means per ray of one view: the base-voxel lookup of
    csrc/tsdf_raycast_sparse.hpp restated with tensors, over every sample up to the hit (all of them without a hit)."""
    f32 = torch.float32
    K, C = torch.tensor(K, dtype=f32, device=dev), torch.tensor(C, dtype=f32, device=dev)
    u = torch.arange(W, dtype=f32, device=dev)[None, :].expand(H, W)
    v = torch.arange(H, dtype=f32, device=dev)[:, None].expand(H, W)
    x, y = (u - K[2]) / K[0], (v - K[3]) / K[1]
    o = torch.tensor(sv.origin[0], dtype=f32, device=dev)
    n = [int(a) for a in sv.dims[0]]
    nb = [(a + 7) // 8 for a in n]
    vx = float(sv.voxel[0])
    inside_n = torch.zeros((H, W), dtype=torch.int64, device=dev)
    absent_n = torch.zeros((H, W), dtype=torch.int64, device=dev)
    last = torch.where(depth > 0, depth + step, torch.full_like(depth, ops.TSDF_DEPTH_MAX))
    for k in range(int((ops.TSDF_DEPTH_MAX - ops.RAYCAST_DEPTH_MIN) / step) + 1):
        z = ops.RAYCAST_DEPTH_MIN + step * k
        X, Y = x * z, y * z
        i = [torch.floor(((((C[4 * r] * X + C[4 * r + 1] * Y) + C[4 * r + 2] * z) + C[4 * r + 3]) - o[r]) / vx)
             for r in range(3)]
        inside = (z <= last)
        for r in range(3):
            inside = inside & (i[r] >= 0) & (i[r] + 1 < n[r])
        b = [torch.where(inside, i[r], torch.zeros_like(i[r])).long() >> 3 for r in range(3)]
        rank = bi[(b[2] * nb[1] + b[1]) * nb[0] + b[0]]
        inside_n += inside
        absent_n += inside & (rank < 0)
    return float(inside_n.float().mean()), float(absent_n.float().mean())


def main():
    assert torch.cuda.is_available(), "tsdf_raycast_sparse_bench needs the GPU"
    dev = torch.device('cuda')
    L, p, stream = _native.lib(), ops._p, torch.cuda.current_stream().cuda_stream
    out = []

    def say(s=""):
        print(s, flush=True)
        out.append(s)

    trunc = 5 * TB.VOXEL
    say("Ray-casting the fragment of tsdf_bench.py from a sparse pool: %d frames of %d x %d, voxel %g m, trunc %g m, step "
        "trunc / 2" % (TB.FRAMES, TB.WIDTH, TB.HEIGHT, TB.VOXEL, trunc))
    say("device: %s (%s)   date: %s" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName,
                                        datetime.date.today().isoformat()))
    say()

    # ------------------------------------------------------------------------------------------- the two volumes
    depth, poses = TB.make_sequence()
    M = np.stack([fr.rigid_inverse(P) @ poses[0] for P in poses])
    C = np.stack([fr.rigid_inverse(poses[0]) @ P for P in poses])
    origin, dims = fr.place_volumes(ops.tsdf_bounds(depth, [0, TB.FRAMES], TB.K, C).cpu().numpy(), TB.VOXEL)
    sv = ops.tsdf_allocate(depth, [0, TB.FRAMES], TB.K, C, origin, dims, TB.VOXEL, trunc)
    Ds, ws = ops.tsdf_integrate_sparse(depth, [0, TB.FRAMES], TB.K, M, sv, trunc)
    D, w, tvs = ops.tsdf_integrate(depth, [0, TB.FRAMES], TB.K, M, origin, dims, TB.VOXEL, trunc)
    total, B, lattice = int(D.numel()), sv.bricks, int(sv.lattice_start[-1])
    sparse_bytes = ops.tsdf_sparse_bytes(sv)
    say("volume: %d x %d x %d = %d voxels; %d of %d bricks allocated (%.1f %%)"
        % (dims[0, 0], dims[0, 1], dims[0, 2], total, B, lattice, 100.0 * B / lattice))
    say("bytes: dense D and w %.3f GB; sparse pool and tables %.1f MB (%.1f %% of the dense bytes; brick_index alone "
        "%.2f MB)" % (8e-9 * total, 1e-6 * sparse_bytes, 100.0 * sparse_bytes / (8.0 * total), 4e-6 * lattice))

    o, n, vx, _, _ = ops._tsdf_volumes(origin, dims, TB.VOXEL, 1)
    views = list(range(0, TB.FRAMES, 3))[:BATCH]
    vv, Kv, Cv, st, H, W = ops._raycast_views(1, trunc, TB.K, C[views], TB.HEIGHT, TB.WIDTH, [0] * BATCH, None,
                                              ops.RAYCAST_DEPTH_MIN, ops.TSDF_DEPTH_MAX)
    to, tn, tvx, tvv, tK, tC, tst = ops._on(dev, o, n, vx, vv, Kv, Cv, st)
    tls, bs, bi, _, _, _, _ = ops._sparse_tables(sv, dev)
    kinds = ("skip on", "skip off", "dense")
    images = {(R, kind): torch.empty((R, H, W), dtype=torch.float32, device=dev) for R in (1, BATCH) for kind in kinds}

    def cast(R, kind):
        def sparse():
            _native.check(L.d3f_tsdf_raycast_sparse(p(Ds), p(ws), None, 0, p(tls), p(bs), p(bi), p(to), p(tn), p(tvx),
                                                    1, lattice, B, p(tvv), R, H, W, p(tK), p(tC), p(tst),
                                                    ops.RAYCAST_DEPTH_MIN, ops.TSDF_DEPTH_MAX, 1.0, 1,
                                                    int(kind == "skip on"), p(images[(R, kind)]), None, None, stream),
                          "d3f_tsdf_raycast_sparse")

        def dense():
            _native.check(L.d3f_tsdf_raycast(p(D), p(w), None, 0, p(tvs), p(to), p(tn), p(tvx), 1, total, p(tvv), R, H,
                                             W, p(tK), p(tC), p(tst), ops.RAYCAST_DEPTH_MIN, ops.TSDF_DEPTH_MAX, 1.0, 1,
                                             p(images[(R, kind)]), None, None, stream), "d3f_tsdf_raycast")
        return dense if kind == "dense" else sparse

    names = {(R, kind): "%d view%s, %s" % (R, "" if R == 1 else "s", "dense volume" if kind == "dense" else
                                            "sparse, " + kind) for R in (1, BATCH) for kind in kinds}
    arms = {names[key]: cast(*key) for key in names}
    ms, spread = OB.medians(arms, REPS)
    for R in (1, BATCH):
        assert OB.same(images[(R, "skip on")], images[(R, "skip off")]), "the skip changed a bit"
    equal_dense = all(OB.same(images[(R, "skip on")], images[(R, "dense")]) for R in (1, BATCH))
    say()
    say("kernel times, 640 x 480, step %g m, box clip on; device events, medians of %d (range); skip on == skip off bit "
        "for bit; sparse == dense render bit for bit on this fragment: %s" % (float(st[0]), REPS, equal_dense))
    for key, name in names.items():
        R = key[0]
        say("  %-28s %9.3f ms  (%.3f..%.3f) = %.3f ms per view, %.2f ns per ray"
            % ((name, ms[name]) + spread[name] + (ms[name] / R, 1e6 * ms[name] / (R * H * W))))
    for R in (1, BATCH):
        say("  %2d view%s: sparse / dense = %.2f; the skip is worth %.2f x"
            % (R, " " if R == 1 else "s", ms[names[(R, "skip on")]] / ms[names[(R, "dense")]],
               ms[names[(R, "skip off")]] / ms[names[(R, "skip on")]]))

    # ------------------------------------------------------------------------- the route of the parent commit
    del D, w
    torch.cuda.empty_cache()

    def parent_route(R):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        Dd, wd, vs = ops.tsdf_densify(Ds, ws, sv)
        img = ops.tsdf_raycast(Dd, wd, vs, origin, dims, TB.VOXEL, trunc, TB.K, C[views[:R]], H, W, [0] * R)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), img

    def sparse_route(R):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        img = ops.tsdf_raycast_sparse(Ds, ws, sv, trunc, TB.K, C[views[:R]], H, W, [0] * R)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), img

    say()
    say("the route of the parent commit, ops.tsdf_densify + ops.tsdf_raycast, against ops.tsdf_raycast_sparse; host "
        "clock around calls that end synchronised, medians of 3 (range) after a warm-up:")
    beats = True
    for R in (1, BATCH):
        parent_route(R), sparse_route(R)
        tp, ts = [], []
        for _ in range(3):
            a, img_p = parent_route(R)
            b, img_s = sparse_route(R)
            tp.append(a)
            ts.append(b)
        assert OB.same(img_p, img_s), "the sparse render is not the render of the densified pool"
        say("  %2d view%s: densify + raycast %9.2f ms (%.2f..%.2f); raycast_sparse %7.3f ms (%.3f..%.3f); bit-identical; "
            "%.0f x" % (R, " " if R == 1 else "s", np.median(tp), min(tp), max(tp), np.median(ts), min(ts), max(ts),
                        np.median(tp) / np.median(ts)))
        beats = beats and max(ts) < min(tp)
        del img_p, img_s
    say("  requirement (the sparse kernel beats densify + raycast on the same views): %s" % ("met" if beats else "MISSED"))
    torch.cuda.empty_cache()

    # -------------------------------------------------------------------------------- samples in absent bricks
    say()
    say("samples per ray (means over the 640 x 480 rays of a view; inside the lattice, up to the hit):")
    tot_in = tot_ab = 0.0
    for j in (0, BATCH // 2, BATCH - 1):
        inside, absent = absent_samples(sv, bi, Kv[j], Cv[j], H, W, float(st[0]), images[(BATCH, "skip on")][j], dev)
        say("  view of frame %2d: %.1f samples inside the lattice, %.1f of them in absent bricks (%.0f %%)"
            % (views[j], inside, absent, 100.0 * absent / max(inside, 1e-9)))
        tot_in, tot_ab = tot_in + inside / 3, tot_ab + absent / 3
    say("  mean of the three: %.1f samples per ray in absent bricks of %.1f: what a coarser second level could skip"
        % (tot_ab, tot_in))
    say()
    say("where the time goes (reasoned from the figures above, not from counters): a ray is a chain of dependent samples,")
    say("  one memory round trip each in the dense kernel (16 loads issued together).  The sparse kernel makes the same")
    say("  number of round trips in empty space (the table read replaces the 16 loads: fewer bytes, no fewer trips) and two")
    say("  where the brick is there (the table, then the rows), with more integer work per sample, so on a volume whose")
    say("  lines the dense kernel finds in the caches it cannot be faster: %.2f x the dense time on one view, %.2f x on %d."
        % (ms[names[(1, "skip off")]] / ms[names[(1, "dense")]],
           ms[names[(BATCH, "skip off")]] / ms[names[(BATCH, "dense")]], BATCH))
    say("  The brick skip does not pay at step = trunc / 2 = 2.5 voxels: its slab test runs on the %.0f %% of the samples that"
        % (100.0 * tot_ab / max(tot_in, 1e-9)))
    say("  land in absent bricks and a brick of 8 voxels holds about three samples, of which it can drop one: %.2f x the"
        % (ms[names[(1, "skip on")]] / ms[names[(1, "skip off")]]))
    say("  time of skip off; skip=False is the faster setting at this step.  What would pay is fewer samples: %.1f of %.1f"
        % (tot_ab, tot_in))
    say("  per ray lie in absent bricks, which a table over blocks of bricks could step over in a few reads.")
    say("  What the sparse kernel buys is memory (%.1f %% of the bytes) and the densify it replaces."
        % (100.0 * sparse_bytes / (8.0 * total)))
    del Ds, ws, images
    torch.cuda.empty_cache()

    # ------------------------------------------------------------------------------------------------ tracking
    sdepth, sK, sposes = OB.make_sequence(50, 640, 480)
    truth = np.linalg.inv(sposes[0]) @ sposes[-1]

    def track(model):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fr.track_sequence(sdepth, sK, model=model)
        return 1e3 * (time.perf_counter() - t0), res

    models = {"dense, voxel 0.01": MODEL, "sparse, voxel 0.01": dict(MODEL, sparse=True),
              "sparse, voxel 0.006": dict(MODEL, sparse=True, voxel=0.006)}
    times = {k: [] for k in models}
    results = {}
    for m in models.values():
        track(m)                                                # warm-up
    for _ in range(3):
        for k, m in models.items():
            t, results[k] = track(m)
            times[k].append(t)
    say()
    say("track_sequence on the 50 frames of odometry_bench.py (640 x 480, clean depth), model pass included, host clock, "
        "medians of 3 (range):")
    for k in models:
        say("  %-20s %8.1f ms  (%.1f..%.1f); frame 49 off by %.4f deg / %.3f mm; model_status != 0 on %d pairs"
            % ((k, np.median(times[k]), min(times[k]), max(times[k])) + OB.pose_error(results[k][0][-1], truth) +
               (int((results[k][2] != 0).sum()),)))
    say("  (a sparse step adds tsdf_extend to the dense step: mark, index, ONE more read-back -- the brick count -- and "
        "the move of the rows)")

    # ------------------------------------------------------------------------------------------------ the kernels
    say()
    no_scratch = None
    for model in ("Bricks", "Volumes"):             # raycast_kernel<Bricks, 0> and raycast_kernel<Volumes, 0>, mangled
        res = kernel_resources("raycast_kernelIN3d3f4tsdf%d%sELi0E" % (len(model), model))
        say("raycast_kernel<%s, 0> as compiled for gfx950: %s"
            % (model, ", ".join("%s %d" % kv for kv in res.items()) if res else "not measured (no hipcc here)"))
        if res and model == "Bricks":
            no_scratch = res.get("ScratchSize [bytes/lane]") == 0 and res.get("VGPRs Spill") == 0
    say("requirement (the sparse kernel uses no scratch): %s" % ("not measured" if no_scratch is None else
                                                                 "met" if no_scratch else "MISSED"))
    text = "\n".join(out) + "\n"
    dest = os.environ.get("TSDF_RAYCAST_SPARSE_BENCH_OUT", os.path.join(HERE, "tsdf_raycast_sparse_bench.txt"))
    with open(dest, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
