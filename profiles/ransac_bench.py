"""Times ops.ransac_rigid (two launches: scoring + refinement) on a redkitchen-sized synthetic batch and compares the
scoring rate with the VALU bound of DESIGN.md's RANSAC section.

    python profiles/ransac_bench.py [--pairs 506] [--hyp 50000] [--reps 10]

Batch: P pairs of 1000..2000 correspondences (uniform), 30..95 % outliers, sigma = 1 cm, tau = 5 cm, edge ratio 0.9,
3 refinement iterations.  Time per batch from torch events around back-to-back calls after warm-up (median of reps).
tests = sum over pairs of count x H (every hypothesis of a block runs the full scan, valid or not).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import d3feat_pytorch_amd  # noqa: E402,F401
from d3feat_pytorch_amd import ops  # noqa: E402

# f32 VALU issue bound: 256 CUs x 4 SIMDs x 32 lanes/clk (a wave64 instruction takes 2 cycles) x 2.4 GHz = 7.86e13
# lane-instructions/s; one inlier test is 17 VALU instructions (9 fma + 3 sub, 1 mul + 2 fma, compare + add).
LANE_OPS_PER_S = 256 * 4 * 32 * 2.4e9
VALU_PER_TEST = 17
BOUND_TESTS_PER_S = LANE_OPS_PER_S / VALU_PER_TEST


def batch(P, rng):
    srcs, tgts, counts = [], [], []
    for _ in range(P):
        M = int(rng.integers(1000, 2001))
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        t = rng.normal(size=3)
        tgt = rng.uniform(-1.5, 1.5, size=(M, 3))
        src = tgt @ q.T + t + rng.normal(scale=0.01, size=(M, 3))
        bad = rng.random(M) < rng.uniform(0.3, 0.95)
        src[bad] = rng.uniform(-1.5, 1.5, size=(int(bad.sum()), 3)) @ q.T + t
        srcs.append(src)
        tgts.append(tgt)
        counts.append(M)
    offs = np.cumsum([0] + counts[:-1])
    seg = np.stack([offs, counts], axis=1).astype(np.int32)
    dev = torch.device('cuda')
    return (torch.from_numpy(np.concatenate(srcs).astype(np.float32)).to(dev),
            torch.from_numpy(np.concatenate(tgts).astype(np.float32)).to(dev),
            torch.from_numpy(seg).to(dev).contiguous(), np.array(counts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=506)      # redkitchen's gt.log
    ap.add_argument('--hyp', type=int, default=50000)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=2)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    src, tgt, seg, counts = batch(a.pairs, rng)
    kw = dict(num_hypotheses=a.hyp, distance_threshold=0.05, edge_ratio=0.9, refine_iters=3, seed=0)
    for _ in range(a.warmup):
        ops.ransac_rigid(src, tgt, seg, **kw)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = ops.ransac_rigid(src, tgt, seg, **kw)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    ms = float(np.median(times))
    tests = float(counts.sum()) * a.hyp
    st = out[4].cpu().numpy()
    res = {'pairs': a.pairs, 'hypotheses': a.hyp, 'correspondences': int(counts.sum()), 'ms_per_batch': round(ms, 3),
           'ms_min': round(float(np.min(times)), 3), 'ms_max': round(float(np.max(times)), 3),
           'tests_per_s': tests / (ms * 1e-3), 'bound_tests_per_s': BOUND_TESTS_PER_S,
           'fraction_of_bound': round(tests / (ms * 1e-3) / BOUND_TESTS_PER_S, 3),
           'pairs_ok': int((st == 0).sum()), 'device': torch.cuda.get_device_properties(0).gcnArchName}
    print("ransac_rigid: %d pairs x %d hypotheses, %d correspondences: %.3f ms per batch (min %.3f, max %.3f)" % (
        a.pairs, a.hyp, counts.sum(), ms, res['ms_min'], res['ms_max']))
    print("  %.3g tests/s = %.1f %% of the VALU bound %.3g tests/s (%d VALU instructions per test)" % (
        res['tests_per_s'], 100 * res['fraction_of_bound'], BOUND_TESTS_PER_S, VALU_PER_TEST))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
