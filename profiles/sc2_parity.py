"""Measures d0, the largest entry difference of T between the host twin of the spatial-compatibility estimator
(ops.sc2_rigid_host) and the NumPy restatement (registration.sc2_numpy) over the pose cases of tests/fgr_cases.py with
num_seeds=64, on the CPU, and writes profiles/sc2_parity.txt.  tests/sc2_cases.py derives its tolerance from it:
max(1e-9, 100 d0).

    python profiles/sc2_parity.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import d3feat_pytorch_amd  # noqa: E402,F401
from d3feat_pytorch_amd import ops  # noqa: E402
from d3feat_pytorch_amd.geometric_registration import registration as reg  # noqa: E402
import fgr_cases as fc  # noqa: E402


def main():
    lines = ["sc2_parity.py: |T_host_twin - T_numpy| (largest entry) per case of tests/fgr_cases.py POSE_CASES, "
             "num_seeds=64, CPU", "case = (count, outlier share, sigma, input seed, unused)"]
    d0 = 0.0
    for case in fc.POSE_CASES:
        M, out, sigma, rng_seed, _ = case
        src, tgt, _, _ = fc.pose_pair(M, out, sigma, rng_seed)
        seg = np.array([[0, M]], dtype=np.int32)
        h = [x.numpy() for x in ops.sc2_rigid_host(src, tgt, seg, num_seeds=64)]
        n = reg.sc2_numpy(src, tgt, seg, num_seeds=64)
        same = all(np.array_equal(h[k], n[k]) for k in (1, 2, 3, 4))
        d = float(np.abs(h[0] - n[0]).max())
        d0 = max(d0, d)
        lines.append("  %-28s %.3e   integer outputs %s" % (case, d, "equal" if same else "DIFFER"))
    lines.append("d0 = %.3e   ->   bound max(1e-9, 100 d0) = %.3e" % (d0, max(1e-9, 100 * d0)))
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(ROOT, 'profiles', 'sc2_parity.txt'), 'w') as fh:
        fh.write(text + "\n")


if __name__ == '__main__':
    main()
