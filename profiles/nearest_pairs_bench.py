"""Times ops.nearest_pairs (d3f_nearest_pairs) on one 3DMatch-sized scene and compares it with what the package could do
before for one pair (a per-pair RadiusGrid + query(width=1)) and with scipy's cKDTree on 16 threads.

    python profiles/nearest_pairs_bench.py [--fragments 60] [--out FILE]

Scene: F fragments = independent noisy samplings of one indoor-like world (synthetic.raw_fragment at twice the usual
scale) cut to windows of half its length, each in a frame of its own, voxel-subsampled at 0.03 m on the device
(~25 k points each).  Pairs: every i < j the bounding-box prefilter of datasets/preprocess.py lets through.
Times are device events around back-to-back calls after a warm-up; every arm runs for at least a second and the two
arms of a comparison alternate in one process.  Bound: the algorithmic bytes of ops.nearest_pairs_bytes (12 B query,
27 bucket headers of 8 B, 24 B per candidate of the matched rows' own cell at the least, 4 B written) over the
6.3 TB/s the HBM achieves.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import d3feat_pytorch_amd  # noqa: E402,F401
from d3feat_pytorch_amd import _native, ops, synthetic  # noqa: E402
from d3feat_pytorch_amd.datasets import preprocess as pp  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
VOXEL = 0.03
RADIUS = 1.25 * VOXEL


def make_scene(F, raw_per_fragment, rng):
    scale = 2 * synthetic.SCENE_SCALE
    length = 3.0 * scale
    starts = np.sort(rng.uniform(0.0, length / 2, size=F))
    frags, poses = [], []
    for k, lo in enumerate(starts):
        w = synthetic.raw_fragment(1000 + k, n_raw=raw_per_fragment, scale=scale).astype(np.float64)
        w = w[(w[:, 0] >= lo) & (w[:, 0] < lo + length / 2)]
        a = rng.uniform(0, 2 * np.pi, size=3)
        c, s = np.cos(a), np.sin(a)
        R = np.array([[c[2], -s[2], 0], [s[2], c[2], 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, c[0], -s[0]], [0, s[0], c[0]]])
        P = np.eye(4)
        P[:3, :3], P[:3, 3] = R, rng.uniform(-1, 1, size=3)
        frags.append(((w - P[:3, 3]) @ P[:3, :3]).astype(np.float32))
        poses.append(P)
    return frags, np.stack(poses)


def timed(fn, min_seconds, min_reps=3):
    """ms per call of fn() (device events, back to back), over at least min_seconds."""
    fn()
    torch.cuda.synchronize()
    total, reps = 0.0, 0
    while total < 1e3 * min_seconds or reps < min_reps:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        total += e0.elapsed_time(e1)
        reps += 1
    return total / reps, reps


def alternate(arms, min_seconds):
    """{name: ms per call}: the arms take turns until each has run for min_seconds."""
    for fn in arms.values():
        fn()
    torch.cuda.synchronize()
    total = {k: 0.0 for k in arms}
    reps = {k: 0 for k in arms}
    while min(total.values()) < 1e3 * min_seconds:
        for k, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            total[k] += e0.elapsed_time(e1)
            reps[k] += 1
    return {k: total[k] / reps[k] for k in arms}, reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fragments', type=int, default=60)
    ap.add_argument('--raw', type=int, default=1200000)
    ap.add_argument('--subset', type=int, default=48, help="pairs of the per-pair comparison")
    ap.add_argument('--seconds', type=float, default=1.0)
    ap.add_argument('--no-kdtree', action='store_true')
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
    all_pairs = a.fragments * (a.fragments - 1) // 2
    order = np.argsort(pairs[:, 1], kind='stable')           # as mine_scene orders them: one target's pairs together
    pairs, T = pairs[order], T[order]
    rows = int(lens[pairs[:, 0]].sum())
    say("# python profiles/nearest_pairs_bench.py  (%s)" % torch.cuda.get_device_properties(0).gcnArchName)
    say("scene: %d fragments, %d..%d points (mean %.0f) at %.3f m, radius %.4f; %d of %d pairs pass the prefilter, "
        "%d query rows" % (a.fragments, lens.min(), lens.max(), lens.mean(), VOXEL, RADIUS, len(pairs), all_pairs, rows))
    pts = torch.as_tensor(np.concatenate(clouds, 0)).to(dev)

    build_ms, _ = timed(lambda: ops.CloudGrid(pts, lens, RADIUS), 0.3)
    grid = ops.CloudGrid(pts, lens, RADIUS)
    say("cell list over the scene (d3f_cloud_grid_build, %d points, %d clouds): %.3f ms" % (len(pts), len(lens), build_ms))
    pr, tf = torch.as_tensor(pairs.astype(np.int32)).to(dev), torch.as_tensor(T).to(dev)
    nn, count, _ = ops.nearest_pairs(grid, None, pr, tf, RADIUS)
    grid.status.raise_if_set()
    found = int(count.sum().item())
    nbytes = ops.nearest_pairs_bytes(rows, found)
    say("matched rows: %d (%.1f %%); algorithmic bytes %.1f MB (%.1f B per query)" % (found, 100.0 * found / rows,
                                                                                    nbytes / 1e6, nbytes / rows))

    # ---- lanes per query, the whole scene in one launch, taking turns
    arms = {("%d lanes" % g): (lambda g=g: ops.nearest_pairs(grid, None, pr, tf, RADIUS, lanes=g)) for g in (4, 8, 16, 32)}
    ms, reps = alternate(arms, a.seconds)
    arms_keys = list(arms)
    say("lanes per query (whole scene, one launch; operator time incl. its prefix sums and read-back of the row count):")
    res = {}
    for k in arms_keys:
        bound_ms = 1e3 * nbytes / HBM_BYTES_PER_S
        say("  %-8s %8.3f ms  %.3e queries/s  %5.1f %% of the byte bound (%.3f ms)  [%d calls]"
            % (k, ms[k], rows / ms[k] * 1e3, 100.0 * bound_ms / ms[k], bound_ms, reps[k]))
        res[k] = ms[k]
    default_ms = ms["8 lanes"]

    # ---- one pair at a time, old against new, on a subset of pairs with a good overlap
    ratio = (count.cpu().numpy() / lens[pairs[:, 0]])
    sub = np.argsort(-ratio, kind='stable')[:a.subset]
    sub_rows = int(lens[pairs[sub, 0]].sum())
    moved = [torch.as_tensor(pp.transform_points(clouds[i], T[k])).to(dev) for k, (i, j) in zip(sub, pairs[sub])]
    targets = [torch.as_tensor(clouds[j]).to(dev) for _, j in pairs[sub]]
    old_grids = [ops.RadiusGrid(t, [len(t)], RADIUS) for t in targets]
    sub_pr, sub_tf = pr[torch.as_tensor(sub).to(dev)].contiguous(), tf[torch.as_tensor(sub).to(dev)].contiguous()
    # launches only: every buffer is made beforehand, both arms go straight to the C ABI
    L, stream = _native.lib(), torch.cuda.current_stream().cuda_stream
    q_lens = [torch.tensor([q.shape[0]], dtype=torch.int32, device=dev) for q in moved]
    old_out = [torch.empty((q.shape[0], 1), dtype=torch.int32, device=dev) for q in moved]
    new_out = [torch.empty(q.shape[0], dtype=torch.int32, device=dev) for q in moved]
    new_cnt = torch.zeros(len(sub), dtype=torch.int32, device=dev)
    one_pr = [sub_pr[k:k + 1].contiguous() for k in range(len(sub))]
    one_tf = [sub_tf[k:k + 1, :3, :].contiguous() for k in range(len(sub))]
    one_rs = [torch.tensor([0, q.shape[0]], dtype=torch.int64, device=dev) for q in moved]
    all_tf = sub_tf[:, :3, :].contiguous()
    all_rs = torch.zeros(len(sub) + 1, dtype=torch.int64, device=dev)
    all_rs[1:] = torch.cumsum(torch.tensor([q.shape[0] for q in moved], device=dev), 0)
    all_out = torch.empty(sub_rows, dtype=torch.int32, device=dev)
    p_ = ops._p

    def old_query():
        for g, q, ql, o in zip(old_grids, moved, q_lens, old_out):
            L.d3f_radius_query_ex(p_(g.ws), p_(q), q.shape[0], p_(ql), g.Ns, p_(g.s_len), 1, g.radius, RADIUS, 1, p_(o),
                                  None, None, None, 0, None, 0, p_(g.status.word), stream)

    def old_build_query():
        for t, q in zip(targets, moved):
            ops.RadiusGrid(t, [t.shape[0]], RADIUS).query(q, [q.shape[0]], 1)

    def new_per_pair(lanes=0):
        for k in range(len(sub)):
            L.d3f_nearest_pairs_lanes(p_(grid.ws), p_(grid.supports), grid.Ns, p_(grid.cloud_start), len(lens),
                                      grid.radius, RADIUS, p_(one_pr[k]), p_(one_tf[k]), p_(one_rs[k]), 1,
                                      new_out[k].shape[0], p_(new_out[k]), p_(new_cnt[k:k + 1]), p_(grid.status.word),
                                      lanes, stream)

    def new_one_call():
        L.d3f_nearest_pairs(p_(grid.ws), p_(grid.supports), grid.Ns, p_(grid.cloud_start), len(lens), grid.radius,
                            RADIUS, p_(sub_pr), p_(all_tf), p_(all_rs), len(sub), sub_rows, p_(all_out), p_(new_cnt),
                            p_(grid.status.word), stream)

    # the same answers first
    old_query()
    new_per_pair()
    new_one_call()
    torch.cuda.synchronize()
    for k in range(len(sub)):
        old = old_out[k][:, 0]
        assert torch.equal(torch.where(old >= targets[k].shape[0], torch.full_like(old, -1), old), new_out[k])
    assert torch.equal(torch.cat(new_out), all_out)
    arms = {"old query": old_query, "old build+query": old_build_query, "new per pair": new_per_pair,
            "new one call": new_one_call}
    arms.update({"per pair, %d" % g: (lambda g=g: new_per_pair(g)) for g in (4, 8, 16, 32)})
    ms, reps = alternate(arms, a.seconds)
    say("one pair at a time, the %d best-overlapping pairs (%d rows); launches only, buffers made beforehand:"
        % (len(sub), sub_rows))
    for k, label in (("old query", "d3f_radius_query_ex(width=1) on a per-pair list, build and transform not counted"),
                     ("old build+query", "RadiusGrid(...).query(width=1) with the per-pair build (operator level)"),
                     ("new per pair", "d3f_nearest_pairs, one launch per pair on the scene's list"),
                     ("per pair, 4", "the same with 4 lanes per query forced"),
                     ("per pair, 8", "the same with 8 lanes"),
                     ("per pair, 16", "the same with 16 lanes"), ("per pair, 32", "the same with 32 lanes"),
                     ("new one call", "d3f_nearest_pairs, the %d pairs in one launch" % len(sub))):
        say("  %-16s %8.3f ms  %7.2f ns/query  %s" % (k, ms[k], 1e6 * ms[k] / sub_rows, label))
    say("  ratio old query / new per pair = %.2f; old query / new one call = %.2f; old build+query / new one call = %.2f"
        % (ms["old query"] / ms["new per pair"], ms["old query"] / ms["new one call"],
           ms["old build+query"] / ms["new one call"]))

    # ---- end to end: mine_scene on the device against cKDTree on 16 threads
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, corr = pp.mine_scene(clouds, poses, None, radius=RADIUS, device=dev)
    torch.cuda.synchronize()
    e2e = time.perf_counter() - t0
    say("mine_scene(device): %.3f s wall for %d pairs kept of %d (cell list, kernel, compaction, lists to the host)"
        % (e2e, len(corr), len(pairs)))
    out = {"fragments": a.fragments, "pairs": int(len(pairs)), "rows": rows, "ms_per_scene": default_ms,
           "queries_per_s": rows / default_ms * 1e3, "fraction_of_byte_bound": 1e3 * nbytes / HBM_BYTES_PER_S / default_ms,
           "ratio_old_query_over_new_per_pair": ms["old query"] / ms["new per pair"],
           "ratio_old_query_over_new_one_call": ms["old query"] / ms["new one call"], "mine_scene_s": e2e,
           "lanes_ms": res}
    if not a.no_kdtree:
        from scipy.spatial import cKDTree
        t0 = time.perf_counter()
        trees = {}
        hits = 0
        for k, (i, j) in enumerate(pairs):
            if j not in trees:
                trees[j] = cKDTree(clouds[j])
            d, _ = trees[j].query(pp.transform_points(clouds[i], T[k]), k=1, distance_upper_bound=RADIUS, workers=16)
            hits += int(np.isfinite(d).sum())
        kd = time.perf_counter() - t0
        say("cKDTree.query(workers=16), same pairs: %.3f s wall (%d matched rows; f64 distances, so a handful of rows "
            "may differ) -> %.1f x mine_scene, %.0f x the kernel alone" % (kd, hits, kd / e2e, kd / (default_ms / 1e3)))
        out["ckdtree_s"] = kd
    say(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
