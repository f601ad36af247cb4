"""Times the tracking of a 640 x 480 RGB-D sequence by ops.rgbd_odometry (d3f_rgbd_odometry) beside ops.depth_odometry
(d3f_depth_odometry) on the same frames in the same run, the arms taking turns:

    python profiles/rgbd_odometry_bench.py [--frames 50] [--reps 7] [--out FILE]

Sequence: that of profiles/odometry_bench.py (the analytic room of tests/tsdf_scene.py at 640 x 480, F cameras that move
10 mm and turn about 0.45 degrees per frame) painted with the analytic texture of tests/rgbd_cases.py; the pairs are
(f + 1, f), every one from the identity, the default schedule (10, 5, 4), max_distance 0.1, the default photo_weight.

* device -- events around back-to-back calls of the C entry points on buffers made beforehand, after a warm-up, medians
  and ranges over the repetitions; the intensity pyramid (d3f_rgbd_pyramid, from 8-bit colour and from f32) and the
  depth pyramid the same way on an uploaded sequence.
* one iteration of a level -- (t(K iterations at that level alone) - t(no iteration)) / K, K = 8: an association launch
  plus a fit launch over all pairs, for both trackers.
* one pair alone -- the same call with P = 1.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "profiles"))
import d3feat_pytorch_amd  # noqa: E402,F401
from d3feat_pytorch_amd import _native, ops  # noqa: E402
import rgbd_cases as RC  # noqa: E402
from odometry_bench import make_sequence, medians, pose_error, same  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=50)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rgbd_odometry_bench.py measures on the GPU; there is none here")
    dev = torch.device('cuda')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    depth, K, poses = make_sequence(a.frames, a.width, a.height)
    inten = RC.paint(depth, K, poses)
    rgb = RC.to_rgb8(inten)
    F, H, W = depth.shape
    P = F - 1
    pairs = np.stack([np.arange(1, F), np.arange(0, F - 1)], axis=1).astype(np.int32)
    T_true = np.stack([np.linalg.inv(poses[b]) @ poses[a_] for a_, b in pairs])
    props = torch.cuda.get_device_properties(0)
    w = ops.ODO_PHOTO_WEIGHT
    say("# python profiles/rgbd_odometry_bench.py  (%s, %d CUs)" % (props.gcnArchName, props.multi_processor_count))
    say("sequence: %d frames of %d x %d with an analytic texture, %d pairs (f + 1, f) from the identity; iterations %s, "
        "max_distance %.2f, photo_weight %.2f" % (F, W, H, P, ops.ODO_ITERATIONS, ops.ODO_MAX_DISTANCE, w))

    # ---- the answers first
    pyr = ops.rgbd_pyramid(depth, inten, K, 3)
    T, count, rmse, status, n_photo = (t.cpu().numpy() for t in ops.rgbd_odometry(pyr, pairs))
    Td = ops.depth_odometry(pyr, pairs)[0].cpu().numpy()
    err = np.array([pose_error(T[p], T_true[p]) for p in range(P)])
    errd = np.array([pose_error(Td[p], T_true[p]) for p in range(P)])
    say("device result: status != 0 on %d pairs; accepted pixels %d..%d, photometric rows %d..%d; error against the "
        "analytic poses at most %.4f deg / %.3f mm (depth only: %.4f deg / %.3f mm)" % (
            int((status != 0).sum()), count.min(), count.max(), n_photo.min(), n_photo.max(), err[:, 0].max(),
            err[:, 1].max(), errd[:, 0].max(), errd[:, 1].max()))

    # ---- the launches alone, buffers made beforehand
    L, stream, p_ = _native.lib(), torch.cuda.current_stream().cuda_stream, ops._p
    td = torch.from_numpy(depth.view(np.int16)).to(dev)
    tK = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(K.astype(np.float32), (F, 4)))).to(dev)
    trgb, tf32 = torch.from_numpy(rgb).to(dev), torch.from_numpy(inten).to(dev)
    data, KL, out_i = torch.empty_like(pyr.data), torch.empty_like(pyr.K), torch.empty_like(pyr.intensity)

    def depth_pyramid():
        _native.check(L.d3f_depth_pyramid(p_(td), 0, F, H, W, p_(tK), 3, 1000.0, ops.TSDF_DEPTH_MAX, ops.ODO_DEPTH_DIFF,
                                          p_(data), p_(KL), stream), "d3f_depth_pyramid")

    def intensity_pyramid(t, kind):
        _native.check(L.d3f_rgbd_pyramid(p_(t), kind, F, H, W, 3, p_(out_i), stream), "d3f_rgbd_pyramid")

    tp = torch.from_numpy(pairs).to(dev)
    T0 = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(np.eye(4)[:3], (P, 3, 4)).reshape(P, 12))).to(dev)
    To = torch.empty((P, 4, 4), dtype=torch.float64, device=dev)
    oc, os_, on = (torch.empty(P, dtype=torch.int32, device=dev) for _ in range(3))
    orm = torch.empty(P, dtype=torch.float64, device=dev)
    nbytes = L.d3f_rgbd_odometry_ws_bytes(P, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    assert nbytes >= L.d3f_depth_odometry_ws_bytes(P, H, W)

    def rgbd(iterations, n=P):
        counts = (ctypes.c_int32 * 3)(*iterations)
        _native.check(L.d3f_rgbd_odometry(p_(pyr.data), p_(pyr.intensity), p_(pyr.K), F, H, W, 3, p_(tp), n, p_(T0),
                                          ctypes.cast(counts, ctypes.c_void_p), ops.ODO_MAX_DISTANCE,
                                          ops.ODO_DEPTH_DIFF, w, p_(To), p_(oc), p_(orm), p_(os_), p_(on), None,
                                          p_(ws), nbytes, stream), "d3f_rgbd_odometry")

    def plain(iterations, n=P):
        counts = (ctypes.c_int32 * 3)(*iterations)
        _native.check(L.d3f_depth_odometry(p_(pyr.data), p_(pyr.K), F, H, W, 3, p_(tp), n, p_(T0),
                                           ctypes.cast(counts, ctypes.c_void_p), ops.ODO_MAX_DISTANCE,
                                           ops.ODO_DEPTH_DIFF, p_(To), p_(oc), p_(orm), p_(os_), None, p_(ws), nbytes,
                                           stream), "d3f_depth_odometry")

    it = ops.ODO_ITERATIONS
    arms = {"depth pyramid": depth_pyramid, "intensity rgb8": lambda: intensity_pyramid(trgb, 0),
            "intensity f32": lambda: intensity_pyramid(tf32, 2)}
    for name, fn in (("rgbd", rgbd), ("depth", plain)):
        arms[name + " batch"] = lambda fn=fn: fn(it)
        arms[name + " none"] = lambda fn=fn: fn((0, 0, 0))
        for level in range(3):
            arms["%s level %d x 8" % (name, level)] = lambda fn=fn, level=level: fn(
                tuple(8 if l == level else 0 for l in range(3)))
        arms[name + " one pair"] = lambda fn=fn: fn(it, 1)
    ms, spread = medians(arms, a.reps)
    assert same(out_i, pyr.intensity) and same(data, pyr.data)
    fits = sum(it)
    say("device, medians of %d (range), the arms taking turns:" % a.reps)
    for key, what in (("depth pyramid", "d3f_depth_pyramid"), ("intensity rgb8", "d3f_rgbd_pyramid from 8-bit colour"),
                      ("intensity f32", "d3f_rgbd_pyramid from f32")):
        say("  %-36s %d frames, 3 levels %9.3f ms  (%.3f..%.3f) = %.1f us per frame" % (
            (what + ",", F, ms[key]) + spread[key] + (1e3 * ms[key] / F,)))
    for name, what in (("rgbd", "d3f_rgbd_odometry"), ("depth", "d3f_depth_odometry")):
        key = name + " batch"
        say("  %s, %d pairs, %d launches  %9.3f ms  (%.3f..%.3f) = %.1f us per pair; per pair and fit (%d fits) "
            "%.2f us" % ((what, P, 2 * fits + 3, ms[key]) + spread[key] + (1e3 * ms[key] / P, fits,
                                                                           1e3 * ms[key] / P / fits)))
        key = name + " none"
        say("    no iteration (setup + final association)   %9.3f ms  (%.3f..%.3f)" % ((ms[key],) + spread[key]))
        key = name + " one pair"
        say("    one pair alone, the same launches          %9.3f ms  (%.3f..%.3f)" % ((ms[key],) + spread[key]))
    per_level = {}
    for level in range(3):
        one = {n: (ms["%s level %d x 8" % (n, level)] - ms[n + " none"]) / 8 for n in ("rgbd", "depth")}
        per_level[level] = one
        say("  one iteration at level %d (%3d x %3d), %d pairs: rgbd %8.3f ms = %.2f us per pair; depth only %8.3f ms = "
            "%.2f us per pair; ratio %.2f" % (level, W >> level, H >> level, P, one["rgbd"], 1e3 * one["rgbd"] / P,
                                              one["depth"], 1e3 * one["depth"] / P, one["rgbd"] / one["depth"]))
    ratio = ms["rgbd batch"] / ms["depth batch"]
    say("the photometric term costs %.2f x the depth-only tracker on the batch (%.3f ms against %.3f ms), %.2f x on one "
        "pair alone; the intensity pyramid adds %.3f ms (8-bit colour) to the %.3f ms of the depth pyramid" % (
            ratio, ms["rgbd batch"], ms["depth batch"], ms["rgbd one pair"] / ms["depth one pair"],
            ms["intensity rgb8"], ms["depth pyramid"]))
    say(json.dumps({"frames": F, "width": W, "height": H, "pairs": P, "photo_weight": w,
                    "depth_pyramid_ms": ms["depth pyramid"], "intensity_rgb8_ms": ms["intensity rgb8"],
                    "intensity_f32_ms": ms["intensity f32"], "rgbd_ms": ms["rgbd batch"],
                    "depth_ms": ms["depth batch"], "ratio": ratio, "rgbd_one_pair_ms": ms["rgbd one pair"],
                    "depth_one_pair_ms": ms["depth one pair"],
                    "rgbd_level_iteration_ms": [per_level[l]["rgbd"] for l in range(3)],
                    "depth_level_iteration_ms": [per_level[l]["depth"] for l in range(3)],
                    "max_err_deg": err[:, 0].max(), "max_err_mm": err[:, 1].max()}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
