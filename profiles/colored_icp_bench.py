"""Times the coloured ICP (d3f_color_gradients, d3f_icp_rigid_color) next to the point-to-plane path it extends:

    python profiles/colored_icp_bench.py [--fragments 60] [--out profiles/colored_icp_bench.txt]

Scene and pairs: those of profiles/icp_bench.py (F fragments of ~25 k points at 0.03 m, every overlapping pair, every
pair 1 degree / 0.02 m off its ground truth, max_distance 1.25 voxels, one cell list at 2 max_distance), painted with
the smooth texture of tests/rgbd_cases.py at the world points.  Three comparisons, the yardstick of each being the
unchanged point-to-plane path in the SAME run:

* d3f_estimate_normals against d3f_color_gradients, one launch each over the scene;
* ONE search-and-fit iteration of the point-to-plane form against the coloured one, from runs whose tolerances are 0
  so that no pair stops early: (t(K = 8) - t(K = 0)) / 8, same cell list, rows and poses;
* the whole refinement of all pairs at the defaults (30 / 1e-6 / 1e-6) by each method -- the iteration counts differ,
  which is the point -- with the fits per pair and the end errors of both.

Device times are events around back-to-back calls after a warm-up, the arms taking turns in one process; medians and
ranges of the windows.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import d3feat_pytorch_amd  # noqa: E402,F401
from d3feat_pytorch_amd import _native, ops  # noqa: E402
from d3feat_pytorch_amd.datasets import preprocess as pp  # noqa: E402
from icp_bench import medians, rotation  # noqa: E402
from nearest_pairs_bench import RADIUS, VOXEL, make_scene  # noqa: E402


def tex(X, Y, Z):
    """The texture of tests/rgbd_cases.py: four sinusoids around 0.5, values inside [0.1, 0.9]."""
    return (0.5 + 0.14 * np.sin(17.0 * X + 0.3) + 0.13 * np.sin(19.0 * Y + 1.1) + 0.08 * np.sin(13.0 * Z + 0.7)
            + 0.05 * np.sin(11.0 * (X + Y + Z)))


def pose_errors(T, G):
    """(degrees, metres) per pair of T against G, both [P,4,4]."""
    D = np.linalg.inv(G) @ T
    c = np.clip((np.trace(D[:, :3, :3], axis1=1, axis2=2) - 1.0) / 2.0, -1.0, 1.0)
    return np.rad2deg(np.arccos(c)), np.linalg.norm(D[:, :3, 3], axis=1)


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

    frags, poses = make_scene(a.fragments, a.raw, rng)
    clouds = pp.subsample_fragments(frags, VOXEL, None, dev)
    lens = np.array([len(c) for c in clouds], dtype=np.int32)
    pairs, T = pp.candidate_pairs(clouds, poses, RADIUS)
    order = np.argsort(pairs[:, 1], kind='stable')
    pairs, T = pairs[order], T[order]
    T0 = T.copy()
    for p in range(len(pairs)):
        D = np.eye(4)
        D[:3, :3] = rotation(rng, np.deg2rad(1.0))
        v = rng.normal(size=3)
        D[:3, 3] = 0.02 * v / np.linalg.norm(v)
        T0[p] = T[p] @ D
    inten = []
    for c, P in zip(clouds, poses):
        w = np.asarray(c, dtype=np.float64) @ P[:3, :3].T + P[:3, 3]
        inten.append(tex(w[:, 0], w[:, 1], w[:, 2]).astype(np.float32))
    rows = int(lens[pairs[:, 0]].sum())
    props = torch.cuda.get_device_properties(0)
    say("# python profiles/colored_icp_bench.py  (%s, %d CUs, %s MHz shader clock reported by the runtime)"
        % (props.gcnArchName, props.multi_processor_count, getattr(props, 'clock_rate', 0) // 1000 or 'unknown'))
    say("scene: %d fragments, %d..%d points (mean %.0f) at %.3f m; %d pairs, %d moving rows; max_distance %.4f, normals "
        "and gradients at %.4f; start: ground truth perturbed by 1 deg / 0.02 m" % (
            a.fragments, lens.min(), lens.max(), lens.mean(), VOXEL, len(pairs), rows, RADIUS, 2.0 * RADIUS))
    pts = torch.as_tensor(np.concatenate(clouds, 0)).to(dev)
    I = torch.as_tensor(np.concatenate(inten)).to(dev)
    r_n = 2.0 * RADIUS
    grid = ops.CloudGrid(pts, lens, r_n)
    lens_dev = torch.as_tensor(lens.astype(np.int64)).to(dev)
    pr, Ti = torch.as_tensor(pairs.astype(np.int32)).to(dev), torch.as_tensor(T0).to(dev)
    L, stream, p_ = _native.lib(), torch.cuda.current_stream().cuda_stream, ops._p
    B, P, N = len(lens), len(pairs), grid.Ns
    tf12 = Ti[:, :3, :].contiguous()
    rs = torch.zeros(P + 1, dtype=torch.int64, device=dev)
    rs[1:] = torch.cumsum(lens_dev[pr[:, 0].long()], 0)
    normals = torch.empty((N, 3), dtype=torch.float32, device=dev)
    field = torch.empty((N, 4), dtype=torch.float32, device=dev)
    n_cnt, g_cnt = (torch.empty(N, dtype=torch.int32, device=dev) for _ in range(2))
    To = torch.empty((P, 4, 4), dtype=torch.float64, device=dev)
    oc, oi, os_, onc = (torch.empty(P, dtype=torch.int32, device=dev) for _ in range(4))
    orm, ocr = (torch.empty(P, dtype=torch.float64, device=dev) for _ in range(2))
    nb_p, nb_c = L.d3f_icp_rigid_plane_ws_bytes(P, rows), L.d3f_icp_rigid_color_ws_bytes(P, rows)
    ws_p, ws_c = (torch.empty(n, dtype=torch.uint8, device=dev) for n in (nb_p, nb_c))

    def estimate():
        _native.check(L.d3f_estimate_normals(p_(grid.ws), p_(pts), N, p_(grid.cloud_start), B, grid.radius, r_n, 3, None,
                                             p_(normals), p_(n_cnt), None, p_(grid.status.word), stream),
                      "d3f_estimate_normals")

    def gradients():
        _native.check(L.d3f_color_gradients(p_(grid.ws), p_(pts), N, p_(grid.cloud_start), B, grid.radius, r_n, 4,
                                            p_(normals), p_(I), p_(field), p_(g_cnt), None, p_(grid.status.word),
                                            stream), "d3f_color_gradients")

    def plane(K, rel):
        _native.check(L.d3f_icp_rigid_plane(
            p_(grid.ws), p_(pts), p_(normals), N, p_(grid.cloud_start), B, grid.radius, RADIUS, p_(pr), p_(rs), P, rows,
            p_(tf12), K, rel, rel, p_(To), p_(oc), p_(orm), p_(oi), p_(os_), None, p_(ws_p), nb_p, stream),
            "d3f_icp_rigid_plane")

    def colour(K, rel):
        _native.check(L.d3f_icp_rigid_color(
            p_(grid.ws), p_(pts), p_(normals), p_(field), N, p_(grid.cloud_start), B, grid.radius, RADIUS, p_(pr), p_(rs),
            P, rows, p_(tf12), 0.968, K, rel, rel, p_(To), p_(oc), p_(orm), p_(oi), p_(os_), p_(onc), p_(ocr), None,
            p_(ws_c), nb_c, stream), "d3f_icp_rigid_color")

    estimate()
    gradients()
    torch.cuda.synchronize()
    grid.status.raise_if_set()
    neighbours = int(n_cnt.long().sum())
    valid = float(torch.isfinite(field).all(1).double().mean())

    # ---- the two per-point launches
    ms, spread = medians({"normals": estimate, "gradients": gradients}, a.reps)
    say("per-point launches over %d points (%.1f neighbours per point, %.1f %% of the gradients valid):" % (
        N, neighbours / max(N, 1), 100 * valid))
    say("  d3f_estimate_normals  %8.3f ms  (%.3f..%.3f); %.1f MB algorithmic" % (
        ms["normals"], spread["normals"][0], spread["normals"][1], ops.estimate_normals_bytes(N, neighbours) / 1e6))
    say("  d3f_color_gradients   %8.3f ms  (%.3f..%.3f); %.1f MB algorithmic  = %.3f x the normals launch" % (
        ms["gradients"], spread["gradients"][0], spread["gradients"][1],
        ops.color_gradients_bytes(N, neighbours) / 1e6, ms["gradients"] / ms["normals"]))

    # ---- one iteration: tolerances 0, so every pair is searched every time
    arms = {"plane K=0": lambda: plane(0, 0.0), "plane K=8": lambda: plane(8, 0.0),
            "colour K=0": lambda: colour(0, 0.0), "colour K=8": lambda: colour(8, 0.0)}
    mi, si = medians(arms, a.reps)
    one_plane, one_colour = (mi["plane K=8"] - mi["plane K=0"]) / 8, (mi["colour K=8"] - mi["colour K=0"]) / 8
    say("one search-and-fit iteration (tolerances 0: all %d pairs searched every time):" % P)
    say("  point-to-plane  %8.3f ms  (K = 0: %.3f, K = 8: %.3f)" % (one_plane, mi["plane K=0"], mi["plane K=8"]))
    say("  coloured        %8.3f ms  (K = 0: %.3f, K = 8: %.3f)  = %.3f x point-to-plane" % (
        one_colour, mi["colour K=0"], mi["colour K=8"], one_colour / one_plane))
    say("  ranges: " + "; ".join("%s %.3f..%.3f" % ((k,) + si[k]) for k in mi))

    # ---- the whole refinement at the defaults
    mr, sr = medians({"plane": lambda: plane(30, 1e-6), "colour": lambda: colour(30, 1e-6)}, a.reps)
    plane(30, 1e-6)
    torch.cuda.synchronize()
    Tp, itp, stp = To.cpu().numpy().copy(), oi.cpu().numpy().copy(), os_.cpu().numpy().copy()
    colour(30, 1e-6)
    torch.cuda.synchronize()
    Tc, itc, stc, nc = To.cpu().numpy().copy(), oi.cpu().numpy().copy(), os_.cpu().numpy().copy(), onc.cpu().numpy()
    found = int(oc.sum())
    ep, ec = pose_errors(Tp, T), pose_errors(Tc, T)
    say("the whole refinement of %d pairs at the defaults (30 / 1e-6 / 1e-6, lambda_geometric 0.968):" % P)
    say("  point-to-plane  %8.3f ms  (%.3f..%.3f); fits per pair %d..%d (mean %.1f), %d pairs at the cap, status != 0 on "
        "%d; end error median %.3f deg / %.2f mm, worst %.3f deg / %.2f mm" % (
            mr["plane"], sr["plane"][0], sr["plane"][1], itp.min(), itp.max(), itp.mean(), int((itp == 30).sum()),
            int((stp != 0).sum()), np.median(ep[0]), 1e3 * np.median(ep[1]), ep[0].max(), 1e3 * ep[1].max()))
    say("  coloured        %8.3f ms  (%.3f..%.3f); fits per pair %d..%d (mean %.1f), %d pairs at the cap, status != 0 on "
        "%d; end error median %.3f deg / %.2f mm, worst %.3f deg / %.2f mm; colour rows %.1f %% of the matched" % (
            mr["colour"], sr["colour"][0], sr["colour"][1], itc.min(), itc.max(), itc.mean(), int((itc == 30).sum()),
            int((stc != 0).sum()), np.median(ec[0]), 1e3 * np.median(ec[1]), ec[0].max(), 1e3 * ec[1].max(),
            100.0 * nc.sum() / max(found, 1)))
    say("  (every launch of a call runs whatever the data: a pair that stopped returns at once, so the time follows the "
        "pairs still iterating)")
    say("algorithmic bytes per search at %d matched rows: point-to-plane %.1f MB, coloured %.1f MB" % (
        found, ops.icp_plane_bytes(rows, found) / 1e6, ops.icp_color_bytes(rows, found) / 1e6))
    say(json.dumps({"fragments": a.fragments, "pairs": P, "rows": rows, "normals_ms": ms["normals"],
                    "gradients_ms": ms["gradients"], "plane_iteration_ms": one_plane,
                    "colour_iteration_ms": one_colour, "plane_refine_ms": mr["plane"], "colour_refine_ms": mr["colour"],
                    "plane_mean_fits": float(itp.mean()), "colour_mean_fits": float(itc.mean())}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
