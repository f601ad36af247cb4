"""Times ops.pair_information (d3f_pair_information) against the call that made the same search before it existed:

    python profiles/information_bench.py [--fragments 16] [--reps 21] [--out FILE]

Scene: ``--fragments`` fragments of the surface room of tests/icp_scene.py (~7 k points each), every pair i < j that
passes the bounding-box prefilter (preprocess.candidate_pairs), key i_j under its ground-truth pose: j moving, i fixed,
max_distance 0.075, one cell list over the scene.

* pair_information     -- setup launch, ONE search launch adding 20 f64 sums per lane, finishing launch;
* icp_rigid(max_iters=0) -- setup launch, the same search adding 17 f64 sums, fit launch that only evaluates T_init:
  what the package offered for "one search and its sums" before;
* information_numpy    -- the NumPy restatement (host wall time, once).

Device times are events around one call each after a warm-up, the two arms taking turns in one process, medians over the
repetitions with the range.  The moments are compared with the NumPy path before anything is timed.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
import d3feat_pytorch_amd  # noqa: E402,F401
from d3feat_pytorch_amd import ops  # noqa: E402
from d3feat_pytorch_amd.datasets import preprocess as pp  # noqa: E402
from d3feat_pytorch_amd.geometric_registration import registration as reg  # noqa: E402
import icp_scene as sc  # noqa: E402
from icp_bench import medians  # noqa: E402

RADIUS = 0.075


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fragments', type=int, default=16)
    ap.add_argument('--reps', type=int, default=21)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    dev = torch.device('cuda')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    clouds, poses = sc.make_scene(4, a.fragments)
    lens = np.array([len(c) for c in clouds], dtype=np.int64)
    ij, _ = pp.candidate_pairs(clouds, poses, RADIUS)
    pairs = ij[:, ::-1].copy()                                               # (moving j, fixed i)
    order = np.argsort(pairs[:, 1], kind='stable')
    pairs = pairs[order]
    T = np.stack([sc.gt_transform(poses, i, j) for j, i in pairs])
    rows = int(lens[pairs[:, 0]].sum())
    props = torch.cuda.get_device_properties(0)
    say("# python profiles/information_bench.py  (%s, %d CUs)" % (props.gcnArchName, props.multi_processor_count))
    say("scene: %d fragments, %d..%d points (mean %.0f); %d pairs, %d moving rows; max_distance %.3f; ground-truth "
        "poses" % (a.fragments, lens.min(), lens.max(), lens.mean(), len(pairs), rows, RADIUS))
    grid = ops.CloudGrid(torch.as_tensor(np.concatenate(clouds, 0)).to(dev), lens, RADIUS)
    pr, Ti = torch.as_tensor(pairs.astype(np.int32)).to(dev), torch.as_tensor(T).to(dev)

    # ---- the same answers first
    moments, count, status = ops.pair_information(grid, None, pr, Ti, RADIUS, rows=rows)
    icp = ops.icp_rigid(grid, None, pr, Ti, RADIUS, max_iters=0, rows=rows)
    torch.cuda.synchronize()
    grid.status.raise_if_set()
    t0 = time.perf_counter()
    want, cn = reg.information_numpy(clouds, pairs, T, RADIUS)
    numpy_ms = 1e3 * (time.perf_counter() - t0)
    m = moments.cpu().numpy()
    rel = max(np.abs(m[p] - want[p]).max() / max(np.abs(want[p]).max(), 1e-300) for p in range(len(pairs)))
    say("against information_numpy: counts equal %s, counts equal icp_rigid's %s, status != 0 on %d pairs, largest "
        "moment difference %.2e of the pair's largest moment; %d of %d rows accepted" % (
            np.array_equal(count.cpu().numpy(), cn), bool(torch.equal(count, icp[1])), int((status != 0).sum()), rel,
            int(cn.sum()), rows))

    # ---- times
    arms = {"pair_information": lambda: ops.pair_information(grid, None, pr, Ti, RADIUS, rows=rows),
            "icp_rigid(max_iters=0)": lambda: ops.icp_rigid(grid, None, pr, Ti, RADIUS, max_iters=0, rows=rows)}
    ms, spread = medians(arms, a.reps)
    for k in arms:
        say("  %-24s %8.3f ms  (device events, median of %d, %.3f..%.3f)" % (k, ms[k], a.reps, spread[k][0],
                                                                            spread[k][1]))
    say("  %-24s %8.1f ms  (host wall, one run)" % ("information_numpy", numpy_ms))
    say("ratio pair_information / icp_rigid(max_iters=0): %.3f" % (ms["pair_information"] / ms["icp_rigid(max_iters=0)"]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
