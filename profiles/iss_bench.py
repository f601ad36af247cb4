"""Times the two ISS passes (d3f_iss_saliency, d3f_radius_nms) next to d3f_estimate_normals over the SAME cell list and
radius -- the same walk and the same ten integer sums per neighbour, with an eigenvector solve after them where the
saliency pass has eigenvalues only:

    python profiles/iss_bench.py [--fragments 60] [--out profiles/iss_bench.txt]

Scene: that of profiles/fpfh_bench.py (F fragments of ~25 k points at 0.03 m).  Radii in Open3D's proportion of 6 : 4
model resolutions, scaled to the cell list of the FPFH bench: salient radius 5 voxels, non-maximum radius 10 / 3 voxels,
one cell list at the salient radius.  Device times are events around single calls after a warm-up, the arms taking turns
in one process; medians and ranges of the windows.  The normals arm is measured TWICE in every round: the gap between its
two medians is the spread a ratio has to exceed before it means anything.  The compiler's resource report of the two
kernels is recorded beside the times.
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import d3feat_pytorch_amd  # noqa: E402,F401
from d3feat_pytorch_amd import _native, ops  # noqa: E402
from d3feat_pytorch_amd.datasets import preprocess as pp  # noqa: E402
from icp_bench import medians  # noqa: E402
from nearest_pairs_bench import VOXEL, make_scene  # noqa: E402


def resource_report(source="iss.hip", kernels=("iss_saliency_kernel", "radius_nms_kernel")):
    """{kernel: {VGPRs, ScratchSize, Occupancy, LDS Size}} from hipcc -Rpass-analysis=kernel-resource-usage with the
    flags of _native.build; {} when the compiler is not at hand."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-pass-failed", "-fPIC",
               "-I" + os.path.dirname(_native.HEADER), "-Rpass-analysis=kernel-resource-usage", "-c",
               os.path.join(_native.CSRC, source), "-o", os.path.join(tmp, "out.o")]
        try:
            text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
        except (OSError, subprocess.CalledProcessError):
            return {}
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            name = next((k for k in kernels if k in m.group(1)), None)
            continue
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)",
                      line)
        if m and name:
            out.setdefault(name, {})[m.group(1).split(" [")[0]] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fragments', type=int, default=60)
    ap.add_argument('--raw', type=int, default=1200000)
    ap.add_argument('--reps', type=int, default=9)
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
    r_s, r_n = 5.0 * VOXEL, 10.0 / 3.0 * VOXEL
    props = torch.cuda.get_device_properties(0)
    say("# python profiles/iss_bench.py  (%s, %d CUs)" % (props.gcnArchName, props.multi_processor_count))
    say("scene: %d fragments, %d..%d points (mean %.0f) at %.3f m; salient radius %.3f m, non-maximum radius %.3f m, one "
        "cell list at %.3f m; gammas 0.975, min_neighbors 5" % (a.fragments, lens.min(), lens.max(), lens.mean(), VOXEL,
                                                                 r_s, r_n, r_s))
    pts = torch.as_tensor(np.concatenate(clouds, 0)).to(dev)
    grid = ops.CloudGrid(pts, lens, r_s)
    L, stream, p_ = _native.lib(), torch.cuda.current_stream().cuda_stream, ops._p
    B, N = len(lens), grid.Ns
    yard = torch.empty((N, 3), dtype=torch.float32, device=dev)
    sal = torch.empty(N, dtype=torch.float32, device=dev)
    y_cnt, s_cnt, n_cnt = (torch.empty(N, dtype=torch.int32, device=dev) for _ in range(3))
    keep = torch.empty(N, dtype=torch.uint8, device=dev)
    dense = torch.as_tensor(1.0 - rng.random(N), dtype=torch.float32).to(dev)        # (0, 1]: every row walks

    def normals():
        _native.check(L.d3f_estimate_normals(p_(grid.ws), p_(pts), N, p_(grid.cloud_start), B, grid.radius, r_s, 3, None,
                                             p_(yard), p_(y_cnt), None, p_(grid.status.word), stream),
                      "d3f_estimate_normals")

    def saliency():
        _native.check(L.d3f_iss_saliency(p_(grid.ws), p_(pts), N, p_(grid.cloud_start), B, grid.radius, r_s, 0.975, 0.975,
                                         5, p_(sal), p_(s_cnt), None, p_(grid.status.word), stream), "d3f_iss_saliency")

    def nms(score):
        _native.check(L.d3f_radius_nms(p_(grid.ws), p_(pts), N, p_(grid.cloud_start), B, grid.radius, r_n, p_(score), 5,
                                       p_(keep), p_(n_cnt), p_(grid.status.word), stream), "d3f_radius_nms")

    saliency()
    nms(sal)
    torch.cuda.synchronize()
    grid.status.raise_if_set()
    neighbours = int(s_cnt.long().sum())
    salient = int((sal > 0).sum())
    walked = int(n_cnt.long().sum())
    kept = int(keep.sum())
    ms, spread = medians({"normals": normals, "saliency": saliency, "nms": lambda: nms(sal), "normals_again": normals,
                          "nms_dense": lambda: nms(dense)}, a.reps)
    walked_dense = int(n_cnt.long().sum())
    say("%d points, %.1f neighbours per point at the salient radius; %.1f %% salient, %d keypoints kept (%.1f per "
        "fragment), %.1f neighbours per walking row at the non-maximum radius:" % (
            N, neighbours / max(N, 1), 100.0 * salient / max(N, 1), kept, kept / max(B, 1), walked / max(salient, 1)))
    fmt = "  %-44s %8.3f ms  (%.3f..%.3f)"
    for key, name in (("normals", "d3f_estimate_normals at the salient radius"),
                      ("normals_again", "the same arm, measured again")):
        say((fmt + "; %.1f MB algorithmic = %.2f TB/s") % (
            name, ms[key], spread[key][0], spread[key][1], ops.estimate_normals_bytes(N, neighbours) / 1e6,
            1e-9 * ops.estimate_normals_bytes(N, neighbours) / ms[key]))
    yardstick = 0.5 * (ms["normals"] + ms["normals_again"])
    gap = abs(ms["normals"] - ms["normals_again"]) / yardstick
    ratio = ms["saliency"] / yardstick
    say((fmt + "  = %.3f x the normals launch (its two medians differ by %.3f of their mean); %.3f ns per neighbour") % (
        "d3f_iss_saliency", ms["saliency"], spread["saliency"][0], spread["saliency"][1], ratio, gap,
        1e6 * ms["saliency"] / max(neighbours, 1)))
    for key, name, rows, cand in (("nms", "d3f_radius_nms of that saliency", salient, walked),
                                  ("nms_dense", "d3f_radius_nms of a dense score in (0, 1]", N, walked_dense)):
        say((fmt + "  = %.3f x the normals launch; %d rows walk, %.3f ns per neighbour; %.1f MB algorithmic = %.2f "
             "TB/s") % (name, ms[key], spread[key][0], spread[key][1], ms[key] / yardstick, rows,
                        1e6 * ms[key] / max(cand, 1), ops.radius_nms_bytes(N, rows, cand) / 1e6,
                        1e-9 * ops.radius_nms_bytes(N, rows, cand) / ms[key]))
    res = resource_report()
    for kernel, r in res.items():
        say("  %s: %d VGPRs, %d B scratch per lane, %d B LDS, %d waves per SIMD" % (
            kernel, r.get("VGPRs", -1), r.get("ScratchSize", -1), r.get("LDS Size", -1), r.get("Occupancy", -1)))
    say(json.dumps({"fragments": a.fragments, "points": N, "neighbours_per_point": neighbours / max(N, 1),
                    "salient": salient, "kept": kept, "normals_ms": ms["normals"], "normals_again_ms": ms["normals_again"],
                    "saliency_ms": ms["saliency"], "saliency_over_normals": ratio, "normals_gap": gap,
                    "nms_ms": ms["nms"], "nms_dense_ms": ms["nms_dense"], "resources": res}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
