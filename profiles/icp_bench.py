"""Times ops.icp_rigid (d3f_icp_rigid) on one 3DMatch-sized scene against what the package offered before it:

    python profiles/icp_bench.py [--fragments 60] [--no-composed] [--out FILE]

Scene and pairs: those of profiles/nearest_pairs_bench.py (F fragments of ~25 k points at 0.03 m, every overlapping
pair, one cell list over the scene); every pair starts from its ground truth perturbed by 1 degree / 0.02 m and is
refined at max_distance = 1.25 voxels, the radius of the search floor.

* composed baseline -- the same ICP rule from the public operators that existed before: ops.nearest_pairs -> gather of
  the matched points -> f64 sums per pair (one index_add_ over all rows) -> batched torch.linalg.svd, the stopping rule
  on the host (one read-back per iteration; pairs that stopped leave the pair list).  Host wall time around a
  synchronise, because the host drives it.
* search floor -- one d3f_nearest_pairs launch over the same rows and radius; against it ONE fused iteration (search
  launch + fit launch), taken from runs whose tolerances are 0 so that no pair stops early: (t(K = 8) - t(K = 0)) / 8.

* point-to-plane -- one d3f_estimate_normals launch over the scene (cell list and radius of 2 max_distance), and ONE
  point-to-plane iteration (d3f_icp_rigid_plane, the same K = 8 / K = 0 difference) next to the point-to-point one on
  the same cell list, rows and poses.

Device times are events around back-to-back calls after a warm-up, medians over the repetitions, the arms of a
comparison taking turns in one process.  ``--no-composed`` leaves the composed baseline out (it takes most of the run).
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
from nearest_pairs_bench import RADIUS, VOXEL, make_scene  # noqa: E402


def rotation(rng, angle):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


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


def composed_icp(grid, lens_dev, pr, T0, radius, max_iters, rel_fitness, rel_rmse):
    """The rule of d3f_icp_rigid from ops.nearest_pairs and torch: returns (T [P,4,4], count, rmse, iterations) on the
    device.  Vectorised over the pairs; the stopping rule is evaluated on the host."""
    dev = pr.device
    P = int(pr.shape[0])
    pts = grid.supports
    start = grid.cloud_start.long()
    T = T0.clone()
    count = torch.zeros(P, dtype=torch.int64, device=dev)
    rmse = torch.zeros(P, dtype=torch.float64, device=dev)
    iters = torch.zeros(P, dtype=torch.int64, device=dev)
    prev_f = torch.zeros(P, dtype=torch.float64, device=dev)
    prev_r = torch.zeros(P, dtype=torch.float64, device=dev)
    live = torch.arange(P, device=dev)
    for k in range(max_iters + 1):
        sub = pr[live].contiguous()
        nn, cnt, row_start = ops.nearest_pairs(grid, None, sub, T[live].contiguous(), radius)
        n_rows = int(nn.shape[0])
        a, b = sub[:, 0].long(), sub[:, 1].long()
        seg = lens_dev[a]
        pid = torch.repeat_interleave(torch.arange(len(live), device=dev), seg, output_size=n_rows)
        src_row = torch.arange(n_rows, device=dev) - row_start[pid] + start[a][pid]
        hit = nn >= 0
        pid, src_row, tgt_row = pid[hit], src_row[hit], (nn.long() + start[b][torch.repeat_interleave(
            torch.arange(len(live), device=dev), seg, output_size=n_rows)])[hit]
        x = pts[src_row].double() - pts[start[a]][pid].double()
        y = pts[tgt_row].double() - pts[start[b]][pid].double()
        Tl = T[live][pid]
        q = (torch.einsum('nij,nj->ni', Tl[:, :3, :3], pts[src_row].double()) + Tl[:, :3, 3]).float()
        d = q - pts[tgt_row]
        d2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).double()
        feats = torch.cat([torch.ones_like(d2)[:, None], x, y, (x[:, :, None] * y[:, None, :]).reshape(-1, 9),
                           d2[:, None]], dim=1)
        sums = torch.zeros((len(live), 17), dtype=torch.float64, device=dev).index_add_(0, pid, feats)
        n = sums[:, 0]
        fitness = n / seg.double().clamp(min=1)
        r = torch.sqrt(sums[:, 16] / n.clamp(min=1))
        count[live], rmse[live] = n.long(), r
        stop = (n < 3)
        if k >= 1:
            stop |= ((fitness - prev_f[live]).abs() < rel_fitness) & ((r - prev_r[live]).abs() < rel_rmse)
        if k == max_iters:
            stop |= True
        go = ~stop
        nn_ = n.clamp(min=1)[:, None]
        cx, cy = sums[:, 1:4] / nn_, sums[:, 4:7] / nn_
        S = sums[:, 7:16].reshape(-1, 3, 3) - n[:, None, None] * cx[:, :, None] * cy[:, None, :]
        S = torch.where(go[:, None, None], S, torch.eye(3, dtype=torch.float64, device=dev).expand_as(S))
        U, _, Vh = torch.linalg.svd(S)
        V = Vh.transpose(1, 2)
        det = torch.linalg.det(V @ U.transpose(1, 2))
        D = torch.diag_embed(torch.stack([torch.ones_like(det), torch.ones_like(det), torch.sign(det)], 1))
        Rm = V @ D @ U.transpose(1, 2)
        px, py = pts[start[a]].double(), pts[start[b]].double()
        t = (cy + py) - torch.einsum('pij,pj->pi', Rm, cx + px)
        Tn = T[live].clone()
        Tn[:, :3, :3], Tn[:, :3, 3] = Rm, t
        T[live] = torch.where(go[:, None, None], Tn, T[live])
        prev_f[live], prev_r[live] = fitness, r
        iters[live] += go.long()
        live = live[go]                      # the host read-back of the iteration: how many pairs go on
        if live.numel() == 0:
            break
    return T, count, rmse, iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fragments', type=int, default=60)
    ap.add_argument('--raw', type=int, default=1200000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-composed', action='store_true')
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
    rows = int(lens[pairs[:, 0]].sum())
    props = torch.cuda.get_device_properties(0)
    say("# python profiles/icp_bench.py  (%s, %d CUs, %s MHz shader clock reported by the runtime)"
        % (props.gcnArchName, props.multi_processor_count, getattr(props, 'clock_rate', 0) // 1000 or 'unknown'))
    say("scene: %d fragments, %d..%d points (mean %.0f) at %.3f m; %d pairs, %d moving rows; max_distance %.4f; "
        "start: ground truth perturbed by 1 deg / 0.02 m" % (a.fragments, lens.min(), lens.max(), lens.mean(), VOXEL,
                                                            len(pairs), rows, RADIUS))
    pts = torch.as_tensor(np.concatenate(clouds, 0)).to(dev)
    grid = ops.CloudGrid(pts, lens, RADIUS)
    lens_dev = torch.as_tensor(lens.astype(np.int64)).to(dev)
    pr, Ti = torch.as_tensor(pairs.astype(np.int32)).to(dev), torch.as_tensor(T0).to(dev)
    kw = dict(rows=rows)

    # ---- the same answers first
    fused = ops.icp_rigid(grid, None, pr, Ti, RADIUS, **kw)
    torch.cuda.synchronize()
    grid.status.raise_if_set()
    it_f = fused[3].cpu().numpy()
    found = int(fused[1].sum())
    say("fits per pair %d..%d (mean %.1f), status != 0 on %d pairs; searched rows over the run (pairs that stopped "
        "leave): %.1f M in %d pair-searches" % (it_f.min(), it_f.max(), it_f.mean(), int((fused[4] != 0).sum()),
                                                float(((it_f + 1) * lens[pairs[:, 0]]).sum()) / 1e6,
                                                int((it_f + 1).sum())))
    ms, spread = medians({"fused": lambda: ops.icp_rigid(grid, None, pr, Ti, RADIUS, **kw)}, a.reps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ops.icp_rigid(grid, None, pr, Ti, RADIUS, **kw)
    torch.cuda.synchronize()
    fused_wall = 1e3 * (time.perf_counter() - t0)
    fused_ms, comp_ms = max(ms["fused"], fused_wall), None
    say("per scene, defaults (30 / 1e-6 / 1e-6):")
    say("  fused     %9.3f ms  (device events, median of %d, %.3f..%.3f; host wall of one call %.3f ms)" % (
        ms["fused"], a.reps, spread["fused"][0], spread["fused"][1], fused_wall))
    if not a.no_composed:
        comp = composed_icp(grid, lens_dev, pr, Ti, RADIUS, 30, 1e-6, 1e-6)
        it_c = comp[3].cpu().numpy()
        same = it_f == it_c
        dT = (fused[0] - comp[0]).abs().amax(dim=(1, 2)).cpu().numpy()
        say("fused against composed: %d of %d pairs stop after the same number of fits; max |T - T_composed| over "
            "those %.2e" % (same.sum(), len(same), dT[same].max() if same.any() else float('nan')))
        wall = []
        for _ in range(max(2, a.reps // 2)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            composed_icp(grid, lens_dev, pr, Ti, RADIUS, 30, 1e-6, 1e-6)
            torch.cuda.synchronize()
            wall.append(1e3 * (time.perf_counter() - t0))
        comp_ms = float(np.median(wall))
        say("  composed  %9.3f ms  (host wall incl. synchronise, median of %d, %.3f..%.3f)" % (
            comp_ms, len(wall), min(wall), max(wall)))
        say("  ratio composed / fused = %.2f  (fused taken at the larger of its two figures)" % (comp_ms / fused_ms))

    # ---- one fused iteration against the search floor (launches only, buffers made beforehand)
    L, stream, p_ = _native.lib(), torch.cuda.current_stream().cuda_stream, ops._p
    B, P = len(lens), len(pairs)
    tf12 = Ti[:, :3, :].contiguous()
    rs = torch.zeros(P + 1, dtype=torch.int64, device=dev)
    rs[1:] = torch.cumsum(lens_dev[pr[:, 0].long()], 0)
    out_nn = torch.empty(rows, dtype=torch.int32, device=dev)
    out_cnt = torch.zeros(P, dtype=torch.int32, device=dev)
    To = torch.empty((P, 4, 4), dtype=torch.float64, device=dev)
    oc, oi, os_ = (torch.empty(P, dtype=torch.int32, device=dev) for _ in range(3))
    orm = torch.empty(P, dtype=torch.float64, device=dev)
    nbytes = L.d3f_icp_rigid_ws_bytes(P, rows)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def floor():
        _native.check(L.d3f_nearest_pairs(p_(grid.ws), p_(pts), grid.Ns, p_(grid.cloud_start), B, grid.radius, RADIUS,
                                          p_(pr), p_(tf12), p_(rs), P, rows, p_(out_nn), p_(out_cnt),
                                          p_(grid.status.word), stream), "d3f_nearest_pairs")

    def icp(K):
        _native.check(L.d3f_icp_rigid(p_(grid.ws), p_(pts), grid.Ns, p_(grid.cloud_start), B, grid.radius, RADIUS,
                                      p_(pr), p_(rs), P, rows, p_(tf12), K, 0.0, 0.0, p_(To), p_(oc), p_(orm), p_(oi),
                                      p_(os_), None, p_(ws), nbytes, stream), "d3f_icp_rigid")

    ms, spread = medians({"floor": floor, "K=0": lambda: icp(0), "K=8": lambda: icp(8)}, max(a.reps, 7))
    assert int(oi.min()) == 8, "a pair stopped early although the tolerances are 0"
    one = (ms["K=8"] - ms["K=0"]) / 8
    say("one iteration against the search floor (tolerances 0: all %d pairs searched every time):" % P)
    say("  d3f_nearest_pairs, one launch      %8.3f ms  (%.3f..%.3f)" % ((ms["floor"],) + spread["floor"]))
    say("  d3f_icp_rigid, max_iters = 0       %8.3f ms  (%.3f..%.3f; setup + one search + one stopping launch)" % (
        (ms["K=0"],) + spread["K=0"]))
    say("  d3f_icp_rigid, max_iters = 8       %8.3f ms  (%.3f..%.3f)" % ((ms["K=8"],) + spread["K=8"]))
    say("  one fused iteration (search + fit) %8.3f ms  = %.3f x the search floor (target 1.15)" % (
        one, one / ms["floor"]))
    nb_floor, nb_icp = ops.nearest_pairs_bytes(rows, found), ops.icp_rigid_bytes(rows, found)
    say("algorithmic bytes per search at the final poses' %d matched rows: nearest_pairs %.1f MB, icp_rigid %.1f MB "
        "(no 4-byte index, 2 x 136 B of sums per %d rows); %.2f TB/s at the fused iteration's time" % (
            found, nb_floor / 1e6, nb_icp / 1e6, ops.ICP_BLOCK_ROWS, nb_icp / (one * 1e-3) / 1e12))

    # ---- point-to-plane: the normals launch, and one iteration next to the point-to-point one on the same cell list
    r_n = 2.0 * RADIUS
    grid_n = ops.CloudGrid(pts, lens, r_n)
    normals = torch.empty((grid_n.Ns, 3), dtype=torch.float32, device=dev)
    n_cnt = torch.empty(grid_n.Ns, dtype=torch.int32, device=dev)
    nbytes_p = L.d3f_icp_rigid_plane_ws_bytes(P, rows)
    ws_p = torch.empty(nbytes_p, dtype=torch.uint8, device=dev)

    def estimate():
        _native.check(L.d3f_estimate_normals(p_(grid_n.ws), p_(pts), grid_n.Ns, p_(grid_n.cloud_start), B, grid_n.radius,
                                             r_n, 3, None, p_(normals), p_(n_cnt), None, p_(grid_n.status.word),
                                             stream), "d3f_estimate_normals")

    def icp_on(K, plane):
        if plane:
            _native.check(L.d3f_icp_rigid_plane(
                p_(grid_n.ws), p_(pts), p_(normals), grid_n.Ns, p_(grid_n.cloud_start), B, grid_n.radius, RADIUS, p_(pr),
                p_(rs), P, rows, p_(tf12), K, 0.0, 0.0, p_(To), p_(oc), p_(orm), p_(oi), p_(os_), None, p_(ws_p),
                nbytes_p, stream), "d3f_icp_rigid_plane")
        else:
            _native.check(L.d3f_icp_rigid(
                p_(grid_n.ws), p_(pts), grid_n.Ns, p_(grid_n.cloud_start), B, grid_n.radius, RADIUS, p_(pr), p_(rs), P,
                rows, p_(tf12), K, 0.0, 0.0, p_(To), p_(oc), p_(orm), p_(oi), p_(os_), None, p_(ws), nbytes, stream),
                "d3f_icp_rigid")

    estimate()
    torch.cuda.synchronize()
    neighbours = int(n_cnt.long().sum())
    msp, spreadp = medians({"normals": estimate, "point K=0": lambda: icp_on(0, False),
                            "point K=8": lambda: icp_on(8, False), "plane K=0": lambda: icp_on(0, True),
                            "plane K=8": lambda: icp_on(8, True)}, max(a.reps, 7))
    grid_n.status.raise_if_set()
    one_point, one_plane = (msp["point K=8"] - msp["point K=0"]) / 8, (msp["plane K=8"] - msp["plane K=0"]) / 8
    plane_run = ops.icp_rigid(grid_n, None, pr, Ti, RADIUS, normals=normals, **kw)
    it_p = plane_run[3].cpu().numpy()
    say("point-to-plane, cell list and normals at %.4f m (%d points, %.1f neighbours per point):" % (
        r_n, grid_n.Ns, neighbours / max(grid_n.Ns, 1)))
    say("  d3f_estimate_normals, one launch          %8.3f ms  (%.3f..%.3f); %.1f MB algorithmic = %.2f TB/s" % (
        msp["normals"], spreadp["normals"][0], spreadp["normals"][1],
        ops.estimate_normals_bytes(grid_n.Ns, neighbours) / 1e6,
        ops.estimate_normals_bytes(grid_n.Ns, neighbours) / (msp["normals"] * 1e-3) / 1e12))
    say("  one point-to-point iteration on this list %8.3f ms  (K = 0: %.3f, K = 8: %.3f)" % (
        one_point, msp["point K=0"], msp["point K=8"]))
    say("  one point-to-plane iteration              %8.3f ms  (K = 0: %.3f, K = 8: %.3f) = %.3f x point-to-point" % (
        one_plane, msp["plane K=0"], msp["plane K=8"], one_plane / one_point))
    say("  ranges: " + "; ".join("%s %.3f..%.3f" % ((k,) + spreadp[k]) for k in msp if k != "normals"))
    say("  defaults (30 / 1e-6 / 1e-6): point-to-plane fits per pair %d..%d (mean %.1f) against %d..%d (mean %.1f); "
        "status != 0 on %d pairs" % (it_p.min(), it_p.max(), it_p.mean(), it_f.min(), it_f.max(), it_f.mean(),
                                     int((plane_run[4] != 0).sum())))
    say(json.dumps({"fragments": a.fragments, "pairs": P, "rows": rows, "fused_ms": fused_ms,
                    "composed_ms": comp_ms, "floor_ms": ms["floor"], "fused_iteration_ms": one,
                    "iteration_over_floor": one / ms["floor"], "normals_ms": msp["normals"],
                    "point_iteration_ms": one_point, "plane_iteration_ms": one_plane}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
