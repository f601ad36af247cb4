"""Inputs and criteria that the CPU and GPU tests of fast global registration share (test_fgr_cpu.py, test_fgr_gpu.py)."""
import numpy as np

from test_ransac_cpu import _rotation, kabsch_svd

# The largest entry difference of T between the host twin and the NumPy restatement over POSE_CASES, measured on the
# CPU (profiles/fgr_parity.txt): d0 = 1.7e-15.  The bound is max(1e-9, 100 d0): 1e-9 is what
# test_rigid_fit_matches_svd_kabsch allows a f64 fit against an independent evaluation; the factor 100 pays for the
# different summation order and the last bit of sin / cos over up to 128 steps.
D0 = 1.7e-15
T_BOUND = max(1e-9, 100 * D0)

# (count, outlier share, noise sigma, rng seed, FGR seed).  Outlier shares 0, 30 and 50 %: with these input
# seeds the NumPy restatement itself meets the recovery criterion below on every case (a condition on the inputs: an
# outlier that happens to land within delta of its true place keeps a large weight), so no share had to be lowered.
POSE_CASES = [(M, out, sigma, 100 + 50 * k, k)
              for k in range(2) for sigma in (0.0, 0.01) for out in (0.0, 0.3, 0.5) for M in (300, 1531)]

# The floor is the f32 rounding of the inputs: a coordinate below 4 m is off by up to 2^-22 m = 2.4e-7 m, a point by up
# to sqrt(3) times that = 4.1e-7 m -> 5e-7 m for the translation, and 5e-7 m over the 1.5 m half extent of the points
# is 3.3e-7 rad = 1.9e-5 degrees -> 2e-5 degrees for the rotation.
FLOOR_ROT_DEG, FLOOR_TRANS = 2e-5, 5e-7


def pose_pair(M, outliers, sigma, rng_seed):
    """M correspondences src ~ R0 tgt + t0 spread over a 3 m cube in all three directions, noise sigma, a share of
    uniform outliers -> (src f32, tgt f32, T0 [4,4], true-inlier mask)."""
    rng = np.random.default_rng(rng_seed)
    R0, t0 = _rotation(rng), rng.normal(size=3)
    tgt = rng.uniform(-1.5, 1.5, size=(M, 3))
    src = tgt @ R0.T + t0 + rng.normal(scale=sigma, size=(M, 3))
    bad = rng.random(M) < outliers
    src[bad] = rng.uniform(-1.5, 1.5, size=(int(bad.sum()), 3)) @ R0.T + t0
    T0 = np.eye(4)
    T0[:3, :3], T0[:3, 3] = R0, t0
    return src.astype(np.float32), tgt.astype(np.float32), T0, ~bad


def rot_err_deg(Ra, Rb):
    return float(np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1.0) / 2.0, -1.0, 1.0))))


def pose_errors(T, T0):
    return rot_err_deg(T[:3, :3], T0[:3, :3]), float(np.linalg.norm(T[:3, 3] - T0[:3, 3]))


def recovery_bounds(src, tgt, T0, good):
    """3x the errors of the Kabsch fit over the TRUE inliers (the best a least-squares estimator can do on this input)
    plus the floor: the margin 3 pays for the small weight the outliers keep at mu = delta^2."""
    R, t = kabsch_svd(src[good].astype(np.float64), tgt[good].astype(np.float64))
    K = np.eye(4)
    K[:3, :3], K[:3, 3] = R, t
    er, et = pose_errors(K, T0)
    return 3.0 * er + FLOOR_ROT_DEG, 3.0 * et + FLOOR_TRANS


def stack_host(pairs):
    """[(src, tgt), ...] -> stacked (src [rows,3] f32, tgt, seg int32 [P,2])."""
    src = np.concatenate([p[0] for p in pairs]).astype(np.float32).reshape(-1, 3)
    tgt = np.concatenate([p[1] for p in pairs]).astype(np.float32).reshape(-1, 3)
    lens = [len(p[0]) for p in pairs]
    offs = np.cumsum([0] + lens)[:-1]
    return src, tgt, np.stack([offs, lens], axis=1).astype(np.int32)
