"""Times the tracking of a 640 x 480 depth sequence by ops.depth_odometry (d3f_depth_odometry) against its host twin and
the NumPy restatement, per pair and per iteration, and one pair alone against the batch:

    python profiles/odometry_bench.py [--frames 50] [--reps 7] [--out FILE]

Sequence: the analytic room of tests/tsdf_scene.py rendered at 640 x 480 (fx = fy = 480), depth in millimetres, F
cameras that move 10 mm and turn about 0.45 degrees per frame; the pairs are (f + 1, f), every one from the identity,
the default schedule (10, 5, 4) over three levels, max_distance 0.1.

* device -- events around back-to-back d3f_depth_odometry calls on buffers made beforehand, after a warm-up, medians
  over the repetitions; the pyramid (d3f_depth_pyramid) the same way on an uploaded sequence.
* one iteration of a level -- (t(K iterations at that level alone) - t(no iteration)) / K, K = 8: an association launch
  plus a fit launch over all pairs.
* one pair alone -- the same call with P = 1.
* host twin, NumPy -- host wall time of ops.depth_odometry_host / depth_odometry_numpy on the first pairs of the same
  pyramid (single thread), per pair.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import d3feat_pytorch_amd  # noqa: E402,F401
from d3feat_pytorch_amd import _native, ops  # noqa: E402
import tsdf_scene as S  # noqa: E402


def make_sequence(frames, width, height):
    """(depth uint16 [F,H,W], K [4], poses [F,4,4]) of the room at the given size."""
    k = np.array([0.75 * width, 0.75 * width, (width - 1) / 2.0, (height - 1) / 2.0])
    poses = np.stack([S.look_at((0.25 + 0.01 * i, 0.6 + 0.0025 * i, 0.25 + 0.0025 * i),
                                S.CENTER + np.array([0.0, 0.0025 * i, 0.0025 * i])) for i in range(frames)])
    depth = np.stack([S.to_raw(S.render(P, width, height, k)) for P in poses])
    return depth, k, poses


def pose_error(T, T_true):
    D = np.linalg.inv(T_true) @ T
    c = np.clip((np.trace(D[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.degrees(np.arccos(c))), float(np.linalg.norm(D[:3, 3]) * 1000.0)


def medians(arms, reps):
    """{name: median ms per call}: device events, the arms taking turns, after one warm-up call each."""
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(reps):
        for k, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: float(np.median(v)) for k, v in ms.items()}, {k: (min(v), max(v)) for k, v in ms.items()}


def iteration_bytes(H, W, level):
    """The bytes one association of ONE pair at a level must move: both level images once (4 bytes per pixel; the fixed
    image's five gathers per pixel hit lines another lane of the wave asked for) and 29 f64 sums per chunk of 1024."""
    pixels = (H >> level) * (W >> level)
    return 2 * 4 * pixels + 8 * ops.ODO_SUMS * ((pixels + 1023) // 1024)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=50)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--host-pairs', type=int, default=6)
    ap.add_argument('--numpy-pairs', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("odometry_bench.py measures on the GPU; there is none here")
    dev = torch.device('cuda')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    depth, K, poses = make_sequence(a.frames, a.width, a.height)
    F, H, W = depth.shape
    P = F - 1
    pairs = np.stack([np.arange(1, F), np.arange(0, F - 1)], axis=1).astype(np.int32)
    T_true = np.stack([np.linalg.inv(poses[b]) @ poses[a_] for a_, b in pairs])
    start = np.array([pose_error(np.eye(4), T_true[p]) for p in range(P)])
    props = torch.cuda.get_device_properties(0)
    say("# python profiles/odometry_bench.py  (%s, %d CUs)" % (props.gcnArchName, props.multi_processor_count))
    say("sequence: %d frames of %d x %d, %d pairs (f + 1, f) from the identity (up to %.2f deg / %.1f mm off); "
        "iterations %s, max_distance %.2f, depth_diff %.2f" % (F, W, H, P, start[:, 0].max(), start[:, 1].max(),
                                                              ops.ODO_ITERATIONS, ops.ODO_MAX_DISTANCE,
                                                              ops.ODO_DEPTH_DIFF))

    # ---- the answers first
    pyr = ops.depth_pyramid(depth, K, 3)
    T, count, rmse, status = (t.cpu().numpy() for t in ops.depth_odometry(pyr, pairs))
    err = np.array([pose_error(T[p], T_true[p]) for p in range(P)])
    say("device result: status != 0 on %d pairs; accepted pixels %d..%d; error against the analytic poses at most "
        "%.4f deg / %.3f mm" % (int((status != 0).sum()), count.min(), count.max(), err[:, 0].max(), err[:, 1].max()))

    # ---- the launches alone, buffers made beforehand
    L, stream, p_ = _native.lib(), torch.cuda.current_stream().cuda_stream, ops._p
    td = torch.from_numpy(depth.view(np.int16)).to(dev)
    tK = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(K.astype(np.float32), (F, 4)))).to(dev)
    data, KL = torch.empty_like(pyr.data), torch.empty_like(pyr.K)

    def pyramid():
        _native.check(L.d3f_depth_pyramid(p_(td), 0, F, H, W, p_(tK), 3, 1000.0, ops.TSDF_DEPTH_MAX, ops.ODO_DEPTH_DIFF,
                                          p_(data), p_(KL), stream), "d3f_depth_pyramid")

    tp = torch.from_numpy(pairs).to(dev)
    T0 = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(np.eye(4)[:3], (P, 3, 4)).reshape(P, 12))).to(dev)
    To = torch.empty((P, 4, 4), dtype=torch.float64, device=dev)
    oc, os_ = (torch.empty(P, dtype=torch.int32, device=dev) for _ in range(2))
    orm = torch.empty(P, dtype=torch.float64, device=dev)
    nbytes = L.d3f_depth_odometry_ws_bytes(P, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def odometry(iterations, n=P):
        counts = (ctypes.c_int32 * 3)(*iterations)
        _native.check(L.d3f_depth_odometry(p_(pyr.data), p_(pyr.K), F, H, W, 3, p_(tp), n, p_(T0),
                                           ctypes.cast(counts, ctypes.c_void_p), ops.ODO_MAX_DISTANCE,
                                           ops.ODO_DEPTH_DIFF, p_(To), p_(oc), p_(orm), p_(os_), None, p_(ws), nbytes,
                                           stream), "d3f_depth_odometry")

    arms = {"pyramid": pyramid, "batch": lambda: odometry(ops.ODO_ITERATIONS), "none": lambda: odometry((0, 0, 0)),
            "level 0 x 8": lambda: odometry((8, 0, 0)), "level 1 x 8": lambda: odometry((0, 8, 0)),
            "level 2 x 8": lambda: odometry((0, 0, 8)), "one pair": lambda: odometry(ops.ODO_ITERATIONS, 1)}
    ms, spread = medians(arms, a.reps)
    assert same(data, pyr.data)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    odometry(ops.ODO_ITERATIONS)
    torch.cuda.synchronize()
    wall = 1e3 * (time.perf_counter() - t0)
    fits = sum(ops.ODO_ITERATIONS)
    say("device, medians of %d (range):" % a.reps)
    say("  d3f_depth_pyramid, %d frames, 3 levels      %9.3f ms  (%.3f..%.3f) = %.1f us per frame" % (
        (F, ms["pyramid"]) + spread["pyramid"] + (1e3 * ms["pyramid"] / F,)))
    say("  d3f_depth_odometry, %d pairs, %d launches     %9.3f ms  (%.3f..%.3f; host wall of one call %.3f ms)" % (
        (P, 2 * fits + 3, ms["batch"]) + spread["batch"] + (wall,)))
    say("    per pair %.1f us; per pair and fit (%d fits) %.2f us" % (1e3 * ms["batch"] / P, fits,
                                                                       1e3 * ms["batch"] / P / fits))
    say("  no iteration (setup + final association)    %9.3f ms  (%.3f..%.3f)" % ((ms["none"],) + spread["none"]))
    for level in range(3):
        key = "level %d x 8" % level
        one = (ms[key] - ms["none"]) / 8
        nb = P * iteration_bytes(H, W, level)
        say("  one iteration at level %d (%3d x %3d), %d pairs %8.3f ms  = %.2f us per pair; %.2f MB to move = %.2f TB/s"
            % (level, W >> level, H >> level, P, one, 1e3 * one / P, nb / 1e6, nb / (one * 1e-3) / 1e12))
    say("  one pair alone, the same %d launches          %9.3f ms  (%.3f..%.3f): the batch of %d takes %.1f x one "
        "pair, %.1f x less per pair" % ((2 * fits + 3, ms["one pair"]) + spread["one pair"] +
                                        (P, ms["batch"] / ms["one pair"], P * ms["one pair"] / ms["batch"])))

    # ---- the host twin and the restatement on the first pairs (single thread)
    ph = ops.DepthPyramid(pyr.data.cpu(), pyr.K.cpu(), H, W, 3, ops.ODO_DEPTH_DIFF)
    nh, nn = min(a.host_pairs, P), min(a.numpy_pairs, P)
    t0 = time.perf_counter()
    Th = ops.depth_odometry_host(ph, pairs[:nh])[0].numpy()
    host_ms = 1e3 * (time.perf_counter() - t0) / nh
    t0 = time.perf_counter()
    Tn = ops.depth_odometry_numpy(ph, pairs[:nn])[0]
    numpy_ms = 1e3 * (time.perf_counter() - t0) / nn
    say("host twin  %9.1f ms per pair (%d pairs, host wall); |T - T_device| at most %.2e" % (
        host_ms, nh, np.abs(Th - T[:nh]).max()))
    say("NumPy      %9.1f ms per pair (%d pairs, host wall); |T - T_device| at most %.2e" % (
        numpy_ms, nn, np.abs(Tn - T[:nn]).max()))
    say("per pair: device (batched) %.4f ms, host twin %.0f x that, NumPy %.0f x" % (
        ms["batch"] / P, host_ms / (ms["batch"] / P), numpy_ms / (ms["batch"] / P)))
    say(json.dumps({"frames": F, "width": W, "height": H, "pairs": P, "pyramid_ms": ms["pyramid"],
                    "odometry_ms": ms["batch"], "one_pair_ms": ms["one pair"], "host_ms_per_pair": host_ms,
                    "numpy_ms_per_pair": numpy_ms,
                    "level_iteration_ms": [(ms["level %d x 8" % l] - ms["none"]) / 8 for l in range(3)],
                    "max_err_deg": err[:, 0].max(), "max_err_mm": err[:, 1].max()}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write("\n".join(lines) + "\n")


def same(a, b):
    return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


if __name__ == "__main__":
    main()
