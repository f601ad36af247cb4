"""Measures d0, the largest entry difference of T between the host twin of the fast-global-registration kernel
(ops.fgr_rigid_host) and the NumPy restatement (registration.fgr_numpy) over the pose cases of tests/fgr_cases.py, on
the CPU, and writes profiles/fgr_parity.txt.  tests/fgr_cases.py derives its tolerance from it: max(1e-9, 100 d0).

    python profiles/fgr_parity.py
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
    lines = ["fgr_parity.py: |T_host_twin - T_numpy| (largest entry) per case of tests/fgr_cases.py POSE_CASES, CPU",
             "case = (count, outlier share, sigma, input seed, FGR seed)"]
    d0 = 0.0
    for case in fc.POSE_CASES:
        M, out, sigma, rng_seed, seed = case
        src, tgt, _, _ = fc.pose_pair(M, out, sigma, rng_seed)
        seg = np.array([[0, M]], dtype=np.int32)
        Th = ops.fgr_rigid_host(src, tgt, seg, seed=seed)[0].numpy()
        Tn = reg.fgr_numpy(src, tgt, seg, seed=seed)[0]
        d = float(np.abs(Th - Tn).max())
        d0 = max(d0, d)
        lines.append("  %-28s %.3e" % (case, d))
    lines.append("d0 = %.3e   ->   bound max(1e-9, 100 d0) = %.3e" % (d0, max(1e-9, 100 * d0)))
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(ROOT, 'profiles', 'fgr_parity.txt'), 'w') as fh:
        fh.write(text + "\n")


if __name__ == '__main__':
    main()
