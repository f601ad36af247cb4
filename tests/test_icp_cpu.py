"""CPU: the ICP fit from sums (d3f_icp_fit_host, csrc/rigid.hpp fit_from_sums) against a NumPy SVD fit, the NumPy
restatement of the whole ICP (registration.icp_numpy) on a surface scene, and the moving / fixed conventions of
registration.refine_transforms."""
import inspect

import numpy as np
import pytest

from d3feat_pytorch_amd import _native
from d3feat_pytorch_amd.datasets.preprocess import nearest_pairs_numpy
from d3feat_pytorch_amd.geometric_registration import registration as reg
import icp_scene as sc

SHIFT = (300.0, -200.0, 50.0)


def fit_host(sums, px, py):
    sums, px, py = (np.ascontiguousarray(v, dtype=np.float64) for v in (sums, px, py))
    out = np.zeros(16, dtype=np.float64)
    assert _native.lib().d3f_icp_fit_host(sums.ctypes.data, px.ctypes.data, py.ctypes.data, out.ctypes.data) == 0
    return out.reshape(4, 4)


def sums_of(x, y, px, py):
    """The 17 sums of include/d3feat_hip.h for moving points x matched to fixed points y, about pivots px, py."""
    xs, ys = x.astype(np.float64) - px, y.astype(np.float64) - py
    d2 = ((x.astype(np.float64) - y.astype(np.float64)) ** 2).sum()
    return np.concatenate([[len(x)], xs.sum(0), ys.sum(0), (xs.T @ ys).reshape(-1), [d2]])


def svd_fit(x, y):
    """4x4 of the least-squares y ~ R x + t (centred SVD, reflection fix), f64."""
    x, y = x.astype(np.float64), y.astype(np.float64)
    cx, cy = x.mean(0), y.mean(0)
    U, _, Vt = np.linalg.svd((x - cx).T @ (y - cy))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    T = np.eye(4)
    T[:3, :3] = Vt.T @ D @ U.T
    T[:3, 3] = cy - T[:3, :3] @ cx
    return T


def correspondences(rng, n, shift=(0.0, 0.0, 0.0)):
    """n moving points (f32) and their noisy images under a random pose (f32), both moved by ``shift``."""
    x = rng.uniform(-1.5, 1.5, size=(n, 3))
    G = sc.random_pose(rng)
    y = x @ G[:3, :3].T + G[:3, 3] + rng.normal(scale=0.004, size=(n, 3))
    s = np.asarray(shift)
    return (x + s).astype(np.float32), (y + s).astype(np.float32)


@pytest.mark.parametrize("n", [3, 4, 50, 10000])
def test_fit_from_sums_equals_svd_fit(n):
    rng = np.random.default_rng(100 + n)
    x, y = correspondences(rng, n)
    px, py = x[0].astype(np.float64), y[0].astype(np.float64)
    T = fit_host(sums_of(x, y, px, py), px, py)
    W = svd_fit(x, y)
    assert np.abs(T - W).max() < 1e-12, np.abs(T - W).max()
    R = T[:3, :3]
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-13 and abs(np.linalg.det(R) - 1.0) < 1e-13
    assert (T[3] == [0, 0, 0, 1]).all()


def test_fit_host_rejects_nonsense():
    z = np.zeros(3)
    out = np.zeros(16)
    L = _native.lib()
    assert L.d3f_icp_fit_host(None, z.ctypes.data, z.ctypes.data, out.ctypes.data) == -1
    bad = np.zeros(17)
    assert L.d3f_icp_fit_host(bad.ctypes.data, z.ctypes.data, z.ctypes.data, out.ctypes.data) == -1


@pytest.mark.parametrize("n", [3, 300, 300000])
def test_fit_from_sums_far_from_the_origin_needs_the_pivots(n):
    """Clouds at (300, -200, 50): with the pivots at row 0 of either cloud the fit agrees with a centred SVD fit to
    1e-10 in R and t.  (The raw second moment -- zero pivots -- is off by 3e-9 .. 2.6e-8 in t there, which the second
    half of the test shows, so a kernel that drops the pivots fails.)"""
    rng = np.random.default_rng(200 + n)
    x, y = correspondences(rng, n, SHIFT)
    W = svd_fit(x, y)
    px, py = x[0].astype(np.float64), y[0].astype(np.float64)
    T = fit_host(sums_of(x, y, px, py), px, py)
    err = np.abs(T - W).max()
    print("n = %d: |T - T_svd| = %.3g with pivots" % (n, err))
    assert err < 1e-10
    z = np.zeros(3)
    raw = np.abs(fit_host(sums_of(x, y, z, z), z, z) - W).max()
    print("n = %d: |T - T_svd| = %.3g with zero pivots" % (n, raw))


@pytest.fixture(scope="module")
def pair_scene():
    clouds, poses = sc.make_scene(1, 2)
    return clouds, sc.gt_transform(poses, 0, 1)


def test_icp_numpy_pulls_perturbed_poses_onto_the_geometry(pair_scene):
    clouds, G = pair_scene                      # G maps fragment 1 into fragment 0: moving 1, fixed 0
    rng = np.random.default_rng(5)
    for deg, shift in ((2, 0.03), (4, 0.05), (6, 0.08)):
        T0 = G @ sc.perturbation(rng, deg, shift)
        T, count, rmse, iters, status, trace = reg.icp_numpy(clouds, [(1, 0)], T0[None], 0.075, return_trace=True)
        r0, t0 = sc.pose_error(T0, G)
        r1, t1 = sc.pose_error(T[0], G)
        print("%g deg / %g -> %.3f deg / %.4f, count %d -> %d, %d fits, rmse %.4f" % (
            deg, shift, r1, t1, trace[0, 0, 0], count[0], iters[0], rmse[0]))
        assert status[0] == 0 and 1 <= iters[0] <= 30
        assert r1 < r0 and t1 < t0
        assert count[0] > trace[0, 0, 0]
        assert np.isnan(trace[0, iters[0] + 1:]).all() and not np.isnan(trace[0, :iters[0] + 1]).any()
        assert trace[0, iters[0], 0] == count[0]
        assert abs(rmse[0] - np.sqrt(trace[0, iters[0], 1] / count[0])) < 1e-15


@pytest.fixture(scope="module")
def small_scene():
    clouds, poses = sc.make_scene(2, 2, n=9000)
    return clouds, sc.gt_transform(poses, 0, 1)


def test_refine_transforms_conventions(small_scene):
    """gt.log-style (i, j) with T mapping j into i ("target onto source", what d3f_rigid_fit_host-style fits return)
    improves; the pair swapped with T NOT inverted ends FEW or farther from the truth than it began."""
    clouds, G = small_scene
    rng = np.random.default_rng(6)
    T0 = G @ sc.perturbation(rng, 3, 0.04)
    assert sc.pose_error(G, np.eye(4))[0] > 20          # random poses: T is far from the identity
    T, fitness, rmse, iters = reg.refine_transforms(clouds, [(0, 1)], T0[None], 0.075, device='cpu')
    r0, t0 = sc.pose_error(T0, G)
    r1, t1 = sc.pose_error(T[0], G)
    assert r1 < r0 and t1 < t0 and 0.3 < fitness[0] <= 1.0 and iters[0] >= 1
    # keys work like tuples
    Tk = reg.refine_transforms(clouds, ['0_1'], T0[None], 0.075, device='cpu')[0]
    assert np.array_equal(Tk, T)
    # the a/b mix-up: (1, 0) claims that T0 maps fragment 0 into fragment 1; the truth for that pair is inv(G)
    Gw = np.linalg.inv(G)
    rw0, tw0 = sc.pose_error(T0, Gw)
    Ts, fs, _, its = reg.refine_transforms(clouds, [(1, 0)], T0[None], 0.075, device='cpu')
    rs, ts = sc.pose_error(Ts[0], Gw)
    few = fs[0] * len(clouds[0]) < 3
    print("swapped: %.2f deg / %.3f -> %.2f deg / %.3f, fitness %.4f, %d fits" % (rw0, tw0, rs, ts, fs[0], its[0]))
    assert few or (rs >= rw0 and ts >= tw0)
    assert not (rs < r0 and ts < t0)                     # and nowhere near as good as the right way round


def test_max_iters_zero_only_evaluates(small_scene):
    clouds, G = small_scene
    rng = np.random.default_rng(7)
    T0 = G @ sc.perturbation(rng, 2, 0.03)
    T, count, rmse, iters, status = reg.icp_numpy(clouds, [(1, 0)], T0[None], 0.075, max_iters=0)
    assert np.array_equal(T[0, :3], T0[:3]) and iters[0] == 0 and status[0] == 0
    assert count[0] == nearest_pairs_numpy(clouds, [(1, 0)], T0[None], 0.075)[1][0]
    # [P,3,4] is taken like [P,4,4]
    T34 = reg.icp_numpy(clouds, [(1, 0)], T0[None, :3], 0.075, max_iters=0)[0]
    assert np.array_equal(T34, T)
    with pytest.raises(ValueError):
        reg.icp_numpy(clouds, [(1, 0)], T0[None], 0.075, max_iters=-1)
    with pytest.raises(ValueError):
        reg.icp_numpy(clouds, [(1, 0)], T0[None, :2], 0.075)


def test_few_and_bad_pairs_keep_their_pose():
    rng = np.random.default_rng(8)
    a = rng.uniform(0, 1, size=(200, 3)).astype(np.float32)
    b = (rng.uniform(0, 1, size=(300, 3)) + 10.0).astype(np.float32)          # nowhere near a
    T0 = np.tile(np.eye(4), (3, 1, 1))
    T0[2, 0, 3] = np.nan
    T, count, rmse, iters, status = reg.icp_numpy([a, b], [(0, 1), (0, 5), (1, 0)], T0, 0.075)
    assert list(status) == [reg.ICP_ST_FEW, reg.ICP_ST_PAIR, reg.ICP_ST_NONFINITE]
    assert np.array_equal(T[:2], T0[:2]) and (iters == 0).all() and (count == 0).all() and (rmse == 0).all()


def test_icp_keyword_defaults_leave_the_front_end_alone():
    for fn in (reg.estimate_transform, reg.register_scene):
        sig = inspect.signature(fn)
        assert sig.parameters['icp'].default is None
        assert sig.parameters['icp'].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    # the parameters that were there keep their order and defaults
    names = list(inspect.signature(reg.estimate_transform).parameters)
    assert names[:7] == ['source_keypts', 'source_desc', 'source_score', 'target_keypts', 'target_desc', 'target_score',
                         'num_points'] and names[-1] == 'ransac'
    names = list(inspect.signature(reg.register_scene).parameters)
    assert names[:7] == ['save_path', 'scene', 'gtpath', 'num_points', 'device', 'num_frag', 'out_log']
    with pytest.raises(ValueError):
        reg._icp_keywords(dict(max_iters=3))
