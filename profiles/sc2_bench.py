"""Times ops.sc2_rigid against ops.ransac_rigid and ops.fgr_rigid (all at their defaults) on the same correspondences
and records what each recovers, at five synthetic inlier ratios: profiles/fgr_bench.py with an sc2_rigid column and
the ratio 0.02.  Writes profiles/sc2_bench.txt (--out).

    python profiles/sc2_bench.py [--fragments 60] [--reps 7] [--out profiles/sc2_bench.txt]

Batch: every pair of a 60-fragment scene, 1770 pairs, each with 2000..4000 correspondences (what mutual matching leaves
of 5000 keypoints), points in a 3 m cube, noise sigma = 1 cm on the inliers, the rest uniform outliers; delta = 5 cm.
Arms: sc2 (256 seeds, sets of 20, 3 refinements; max_count = the longest segment; the bit matrices of all pairs exceed
the default max_bytes, so the call runs in slices), fgr (defaults: tuple test on), fgr without the tuple test
(tuple_trials=0: no seed enters), ransac (50 000 hypotheses, 3 refinements).  The arms take turns inside one loop;
every call sits between two device events; medians
with (min .. max) of the repetitions after a warm-up round.  Timed once for all pairs in one call and once for the first
pair alone.  A pair counts as recovered when its pose is within 1 degree and 5 cm of the truth.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import d3feat_pytorch_amd  # noqa: E402,F401
from d3feat_pytorch_amd import ops  # noqa: E402

RATIOS = (0.5, 0.2, 0.1, 0.05, 0.02)
ROT_OK_DEG, TRANS_OK = 1.0, 0.05


def batch(P, inlier_ratio, rng):
    srcs, tgts, counts, truth = [], [], [], []
    for _ in range(P):
        M = int(rng.integers(2000, 4001))
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        t = rng.normal(size=3)
        tgt = rng.uniform(-1.5, 1.5, size=(M, 3))
        src = tgt @ q.T + t + rng.normal(scale=0.01, size=(M, 3))
        bad = rng.random(M) >= inlier_ratio
        src[bad] = rng.uniform(-1.5, 1.5, size=(int(bad.sum()), 3)) @ q.T + t
        srcs.append(src)
        tgts.append(tgt)
        counts.append(M)
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = q, t
        truth.append(T)
    offs = np.cumsum([0] + counts[:-1])
    seg = np.stack([offs, counts], axis=1).astype(np.int32)
    dev = torch.device('cuda')
    return (torch.from_numpy(np.concatenate(srcs).astype(np.float32)).to(dev),
            torch.from_numpy(np.concatenate(tgts).astype(np.float32)).to(dev),
            torch.from_numpy(seg).to(dev).contiguous(), np.array(counts), np.stack(truth))


def errors(T, truth):
    R = np.einsum('pji,pjk->pik', T[:, :3, :3], truth[:, :3, :3])
    c = np.clip((np.trace(R, axis1=1, axis2=2) - 1.0) / 2.0, -1.0, 1.0)
    return np.degrees(np.arccos(c)), np.linalg.norm(T[:, :3, 3] - truth[:, :3, 3], axis=1)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fragments', type=int, default=60)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'sc2_bench.txt'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sc2_bench.py measures on the GPU; there is none")
    P = a.fragments * (a.fragments - 1) // 2
    arms = (('sc2', lambda s, t, g: ops.sc2_rigid(s, t, g, max_count=4000)),
            ('fgr', lambda s, t, g: ops.fgr_rigid(s, t, g)),
            ('fgr tuple_trials=0', lambda s, t, g: ops.fgr_rigid(s, t, g, tuple_trials=0)),
            ('ransac', lambda s, t, g: ops.ransac_rigid(s, t, g)))
    lines = ["sc2_bench.py: %d fragments -> %d pairs, 2000..4000 correspondences each, sigma 0.01, delta 0.05, %s"
             % (a.fragments, P, torch.cuda.get_device_properties(0).gcnArchName),
             "times in ms per call from device events, median (min .. max) of %d alternating repetitions" % a.reps,
             "recovered: pose within %g degree and %g m of the truth; errors are medians over the recovered pairs"
             % (ROT_OK_DEG, TRANS_OK), ""]
    for ratio in RATIOS:
        src, tgt, seg, counts, truth = batch(P, ratio, np.random.default_rng(int(1000 * ratio)))
        one = seg[:1].clone()
        for shape, sg in (('all %d pairs in one call' % P, seg), ('one pair alone (%d rows)' % counts[0], one)):
            times = {name: [] for name, _ in arms}
            outs = {}
            for rep in range(a.reps + 1):                       # round 0 warms every arm up
                for name, fn in arms:
                    ms, outs[name] = timed(lambda: fn(src, tgt, sg))
                    if rep:
                        times[name].append(ms)
            lines.append("inlier ratio %.2f, %s (%d correspondences)" % (ratio, shape, int(sg[:, 1].sum())))
            for name, _ in arms:
                T = outs[name][0].cpu().numpy()
                st = outs[name][4].cpu().numpy()
                er, et = errors(T, truth[:len(T)])
                ok = (er < ROT_OK_DEG) & (et < TRANS_OK) & (st == 0)
                t = np.array(times[name])
                lines.append("  %-20s %9.3f ms (%.3f .. %.3f)   recovered %4d / %d = %5.1f %%   rot %.3f deg, trans %.4f m"
                             % (name, np.median(t), t.min(), t.max(), ok.sum(), len(ok), 100.0 * ok.mean(),
                                np.median(er[ok]) if ok.any() else float('nan'),
                                np.median(et[ok]) if ok.any() else float('nan')))
            lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text + "\n")


if __name__ == '__main__':
    main()
