"""Times the two FPFH passes (d3f_fpfh: the SPFH and the FPFH launch) next to d3f_estimate_normals over the SAME cell
list and radius -- the same walk with 10 integer sums per neighbour -- and next to the host twin on one thread:

    python profiles/fpfh_bench.py [--fragments 60] [--out profiles/fpfh_bench.txt]

Scene: that of profiles/colored_icp_bench.py (F fragments of ~25 k points at 0.03 m).  Radii after Open3D's examples:
normals at 2 voxels, FPFH at 5 voxels; one cell list at the FPFH radius.  Device times are events around single calls
after a warm-up, the arms taking turns in one process; medians and ranges of the windows.  The host twin is brute force
within a cloud, so it runs on the first fragment only and is scaled per point.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import d3feat_pytorch_amd  # noqa: E402,F401
from d3feat_pytorch_amd import _native, ops  # noqa: E402
from d3feat_pytorch_amd.datasets import preprocess as pp  # noqa: E402
from icp_bench import medians  # noqa: E402
from nearest_pairs_bench import VOXEL, make_scene  # noqa: E402

HBM_COPY_TBS = 6.29    # the float4 copy rate measured on the MI355X (profiles/tsdf_bench.py)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fragments', type=int, default=60)
    ap.add_argument('--raw', type=int, default=1200000)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda')
    rng = np.random.default_rng(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    frags, _ = make_scene(a.fragments, a.raw, rng)
    clouds = pp.subsample_fragments(frags, VOXEL, None, dev)
    lens = np.array([len(c) for c in clouds], dtype=np.int32)
    r_n, r_f = 2.0 * VOXEL, 5.0 * VOXEL
    props = torch.cuda.get_device_properties(0)
    say("# python profiles/fpfh_bench.py  (%s, %d CUs)" % (props.gcnArchName, props.multi_processor_count))
    say("scene: %d fragments, %d..%d points (mean %.0f) at %.3f m; normals at %.3f m, FPFH at %.3f m, one cell list at "
        "%.3f m" % (a.fragments, lens.min(), lens.max(), lens.mean(), VOXEL, r_n, r_f, r_f))
    pts = torch.as_tensor(np.concatenate(clouds, 0)).to(dev)
    grid = ops.CloudGrid(pts, lens, r_f)
    L, stream, p_ = _native.lib(), torch.cuda.current_stream().cuda_stream, ops._p
    B, N = len(lens), grid.Ns
    normals = ops.estimate_normals(grid, None, r_n)[0]
    yard = torch.empty((N, 3), dtype=torch.float32, device=dev)
    y_cnt, cnt = (torch.empty(N, dtype=torch.int32, device=dev) for _ in range(2))
    desc = torch.empty((N, 64), dtype=torch.float32, device=dev)
    nbytes = L.d3f_fpfh_ws_bytes(N)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def yardstick():
        _native.check(L.d3f_estimate_normals(p_(grid.ws), p_(pts), N, p_(grid.cloud_start), B, grid.radius, r_f, 3, None,
                                             p_(yard), p_(y_cnt), None, p_(grid.status.word), stream),
                      "d3f_estimate_normals")

    def passes(which):
        _native.check(L.d3f_fpfh_passes(p_(grid.ws), p_(pts), p_(normals), N, p_(grid.cloud_start), B, grid.radius, r_f,
                                        64, 1, p_(desc), p_(cnt), None, p_(grid.status.word), p_(ws), nbytes, which,
                                        stream), "d3f_fpfh_passes")

    passes(3)
    torch.cuda.synchronize()
    grid.status.raise_if_set()
    neighbours = int(cnt.long().sum())
    described = float((cnt > 0).double().mean())
    ms, spread = medians({"normals": yardstick, "spfh": lambda: passes(1), "fpfh": lambda: passes(2),
                          "both": lambda: passes(3)}, a.reps)
    per = neighbours / max(N, 1)
    say("%d points, %.1f neighbours per point at the FPFH radius, %.1f %% described:" % (N, per, 100 * described))
    say("  d3f_estimate_normals at the FPFH radius  %8.3f ms  (%.3f..%.3f); %.1f MB algorithmic = %.2f TB/s" % (
        ms["normals"], spread["normals"][0], spread["normals"][1], ops.estimate_normals_bytes(N, neighbours) / 1e6,
        1e-9 * ops.estimate_normals_bytes(N, neighbours) / ms["normals"]))
    for key, name in (("spfh", "the SPFH pass"), ("fpfh", "the FPFH pass"), ("both", "d3f_fpfh, both passes")):
        say("  %-40s %8.3f ms  (%.3f..%.3f)  = %.2f x the normals launch; %.2f ns per neighbour" % (
            name, ms[key], spread[key][0], spread[key][1], ms[key] / ms["normals"], 1e6 * ms[key] / max(neighbours, 1)))
    total = ops.fpfh_bytes(N, neighbours)
    say("algorithmic bytes of both passes: %.1f MB = %.2f TB/s at their time, %.1f %% of the %.2f TB/s HBM copy rate" % (
        total / 1e6, 1e-9 * total / ms["both"], 100 * 1e-9 * total / ms["both"] / HBM_COPY_TBS, HBM_COPY_TBS))
    # the host twin, one thread, the first fragment
    first = np.ascontiguousarray(clouds[0])
    nrm0 = normals[:len(first)].cpu().numpy()
    t0 = time.perf_counter()
    host = ops.fpfh_host(first, [len(first)], r_f, nrm0, row_width=64, unit=True)
    host_s = time.perf_counter() - t0
    same = bool(np.array_equal(host[0].numpy(), desc[:len(first)].cpu().numpy()))
    say("host twin, one thread, brute force over the first fragment (%d points): %.2f s = %.1f us per point; the device "
        "takes %.4f us per point; rows equal to the device's: %s" % (len(first), host_s, 1e6 * host_s / len(first),
                                                                    1e3 * ms["both"] / N, same))
    say(json.dumps({"fragments": a.fragments, "points": N, "neighbours_per_point": per, "normals_ms": ms["normals"],
                    "spfh_ms": ms["spfh"], "fpfh_ms": ms["fpfh"], "both_ms": ms["both"], "host_us_per_point":
                    1e6 * host_s / len(first), "host_equal": same}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
