"""Inputs and criteria that the CPU and GPU tests of the spatial-compatibility estimator share (test_sc2_cpu.py,
test_sc2_gpu.py).  The pose cases, their generator and the recovery criterion are fgr_cases'."""
import numpy as np

import fgr_cases as fc

# The largest entry difference of T between the host twin and the NumPy restatement over fgr_cases.POSE_CASES with
# num_seeds=64, measured on the CPU (profiles/sc2_parity.txt): d0 = 1.4e-15.  The bound is max(1e-9, 100 d0),
# FGR's convention: 1e-9 is what test_rigid_fit_matches_svd_kabsch allows a f64 fit against an independent evaluation
# (here Horn's quaternions against an SVD, and a fixed tree of partial sums against np.mean).
D0 = 1.4e-15
T_BOUND = max(1e-9, 100 * D0)

# the counts of the parity tests: below, at and above one and two 64-bit words, the 256-thread strides, a 32-row strip
COUNTS = (3, 4, 63, 64, 65, 127, 128, 129, 257, 1531)
# outlier share of each count: the small sets stay clean, the larger ones carry 0.3 .. 0.5
OUTLIERS = {3: 0.0, 4: 0.0, 63: 0.1, 64: 0.2, 65: 0.3, 127: 0.3, 128: 0.4, 129: 0.5, 257: 0.4, 1531: 0.5}
SETTINGS = ((64, 20), (7, 3))                              # (num_seeds, set_size)
LOW_INLIER = [(1500, 0.97, 0.01, 700 + d) for d in range(12)]   # pose_pair arguments: 3 % inliers
ROT_OK_DEG, TRANS_OK = 1.0, 0.05                           # the benchmark tables' "recovered"


def parity_pairs():
    """[(src, tgt)] of COUNTS, input seed 900 + position."""
    return [fc.pose_pair(M, OUTLIERS[M], 0.01, 900 + k)[:2] for k, M in enumerate(COUNTS)]


def next_multiple_of_64(n):
    return (n + 63) // 64 * 64


def compat_sqrt(src, tgt, tau):
    """The compatibility in its textbook form, with square roots: (C bool [n,n], margin f64 [n,n] = how far each entry
    is from the threshold)."""
    a, b = src.astype(np.float64), tgt.astype(np.float64)
    da = np.sqrt(((a[:, None] - a[None]) ** 2).sum(-1))
    db = np.sqrt(((b[:, None] - b[None]) ** 2).sum(-1))
    gap = np.abs(da - db)
    C = gap < tau
    np.fill_diagonal(C, False)
    return C, np.abs(gap - tau)


def unpack_rows(matrix, n):
    """int64 / uint64 [max_count, W] -> bool [n, n]; asserts that every bit and row >= n is 0."""
    m = np.ascontiguousarray(matrix).view(np.uint64)
    bits = np.unpackbits(m.view(np.uint8).reshape(m.shape[0], -1), axis=1, bitorder='little').astype(bool)
    assert not bits[n:].any() and not bits[:, n:].any()
    return bits[:n, :n]
