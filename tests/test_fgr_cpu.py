"""CPU: fast global registration -- the host twin of the kernel (ops.fgr_rigid_host; the rule of csrc/fgr.hpp compiled
for the CPU) against the NumPy restatement (registration.fgr_numpy), the recovery criterion, status bits, argument
checks and the estimator= routing.  Nothing here needs a GPU.

The tolerance of T is fgr_cases.T_BOUND = max(1e-9, 100 d0) with d0 = 1.7e-15 measured over POSE_CASES on the CPU
(profiles/fgr_parity.txt)."""
import numpy as np
import pytest
import torch

import d3feat_pytorch_amd  # noqa: F401
from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.geometric_registration import registration as reg
from test_ransac_cpu import sample_numpy
import fgr_cases as fc


def host(src, tgt, seg, **kw):
    return [x.numpy() for x in ops.fgr_rigid_host(src, tgt, np.asarray(seg, dtype=np.int32).reshape(-1, 2), **kw)]


def _passing(src, tgt, seed, p, trials, scale=0.95):
    """The trials h that pass the tuple test, by the restatement's parts."""
    idx = reg.fgr_draw(seed, p, np.arange(trials), len(src))
    ok = (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2])
    ok &= reg._fgr_triples_ok(src.astype(np.float64)[idx], tgt.astype(np.float64)[idx], scale)
    return np.nonzero(ok)[0]


@pytest.mark.parametrize("count", [3, 4, 257, 1531])
def test_tuple_test_matches_the_restatement(count):
    src, tgt, _, _ = fc.pose_pair(count, 0.3 if count > 4 else 0.0, 0.01, 7 + count)
    seed, p = 11, 5
    trials = 100 * count
    assert np.array_equal(reg.fgr_draw(seed, p, np.arange(trials), count), sample_numpy(seed, p, np.arange(trials), count))
    passing = _passing(src, tgt, seed, p, trials)
    assert len(passing) >= 8, "the input exercises the test"
    # a cap that is reached inside a chunk of 256 trials, in neither its first nor its last slot, past the first chunk
    inside = [c for c in range(1, len(passing)) if passing[c - 1] >= 256 and passing[c - 1] % 256 not in (0, 255)]
    cap = inside[len(inside) // 2]
    for kw, want_tuples in ((dict(max_tuples=0), len(passing)), (dict(max_tuples=cap), cap),
                            (dict(tuple_trials=0), 0)):
        h = host(src, tgt, [[0, count]], seed=seed, first_pair=p, return_debug=True, **kw)
        n = reg.fgr_numpy(src, tgt, [[0, count]], seed=seed, first_pair=p, return_debug=True, **kw)
        assert np.array_equal(h[5], n[5]) and h[5].dtype == np.int32, kw
        assert h[2][0] == n[2][0] == want_tuples, kw
        if 'tuple_trials' in kw:
            assert (h[5] == 1).all()
        else:
            used = passing[:want_tuples]
            want = np.bincount(sample_numpy(seed, p, used, count).reshape(-1), minlength=count)
            assert np.array_equal(h[5], want), kw


@pytest.mark.parametrize("case", fc.POSE_CASES, ids=lambda c: "M%d-out%g-sigma%g-s%d" % (c[0], c[1], c[2], c[4]))
def test_poses_match_the_restatement_and_recover_the_truth(case):
    M, out, sigma, rng_seed, seed = case
    src, tgt, T0, good = fc.pose_pair(M, out, sigma, rng_seed)
    seg = [[0, M]]
    h = host(src, tgt, seg, seed=seed, return_debug=True)
    n = reg.fgr_numpy(src, tgt, seg, seed=seed, return_debug=True)
    d = float(np.abs(h[0] - n[0]).max())
    print("case %s: |T_host - T_numpy| = %.3e" % (case, d))
    assert h[4][0] == n[4][0] == 0
    assert h[1][0] == n[1][0] and h[2][0] == n[2][0]
    assert d <= fc.T_BOUND
    assert abs(h[3][0] - n[3][0]) <= 1e-9 * max(1.0, n[3][0])
    assert np.array_equal(h[6][0, :, 0], n[6][0, :, 0])                       # mu per iteration: the same divisions
    assert np.nanmax(np.abs(h[6] - n[6])[..., 2:]) <= fc.T_BOUND
    assert np.array_equal(h[0][0, 3], [0, 0, 0, 1]) and abs(np.linalg.det(h[0][0, :3, :3]) - 1.0) < 1e-12
    # recovery: within 3x the inlier-only Kabsch fit plus the f32 floor -- first the restatement (a condition on the
    # input), then the host twin
    br, bt = fc.recovery_bounds(src, tgt, T0, good)
    for name, T in (("numpy", n[0][0]), ("host", h[0][0])):
        er, et = fc.pose_errors(T, T0)
        print("  %s: rot %.3e deg (bound %.3e), trans %.3e m (bound %.3e)" % (name, er, br, et, bt))
        assert er <= br and et <= bt, name
    assert h[1][0] >= 0.95 * good.sum()      # noise of sigma 0.01 stays far inside the 0.05 threshold


def test_annealing_reaches_delta_squared_by_iteration_96():
    """The header's arithmetic: a 3 m scene (D2 = 9) is at mu = delta^2 after the 25th division, before iteration 96."""
    src, tgt, _, _ = fc.pose_pair(300, 0.0, 0.0, 3)
    mu = host(src, tgt, [[0, 300]], return_debug=True)[6][0, :, 0]
    D2 = 1.4 * mu[0]
    assert 4.0 < D2 < 9.0                                   # centred points of a 3 m cube
    assert mu[-1] == 0.05 * 0.05 and (np.diff(mu) <= 0).all() and mu[96] == mu[-1] and mu[60] > mu[-1]


def test_status_bits_and_identity():
    src, tgt, _, _ = fc.pose_pair(50, 0.0, 0.0, 21)
    eye = np.eye(4)
    # count 2: FEW
    T, inl, tup, ws, st = host(src, tgt, [[0, 2]])
    assert st[0] == ops.FGR_ST_FEW and np.array_equal(T[0], eye) and inl[0] == 0 and ws[0] == 0
    # three collinear points / all rows on one line: the rotation about the line is free -> SINGULAR, the pose stays
    line = np.zeros((40, 3), np.float32)
    line[:, 0] = np.arange(40, dtype=np.float32) * 0.125
    for rows in (3, 40):
        for fn in (host, lambda *a, **k: list(reg.fgr_numpy(*a, **k))):
            T, inl, tup, ws, st = fn(line[:rows], line[:rows] + np.float32(0.5), [[0, rows]], tuple_trials=0)
            assert st[0] == ops.FGR_ST_SINGULAR, rows
            assert np.array_equal(T[0, :3, :3], np.eye(3)) and np.allclose(T[0, :3, 3], -0.5) and inl[0] == rows
    # with the tuple test on, every triple of a line is degenerate: nothing is live
    assert host(line, line.copy(), [[0, 40]])[4][0] == ops.FGR_ST_FEW
    # a segment past the rows, and a negative offset: SEGMENT
    for seg in ([[10, 41]], [[-1, 10]], [[0, ops.RANSAC_MAX_COUNT + 1]]):
        T, inl, tup, ws, st = host(src, tgt, seg)
        assert st[0] == ops.FGR_ST_SEGMENT and np.array_equal(T[0], eye) and inl[0] == 0 and tup[0] == 0
        assert reg.fgr_numpy(src, tgt, seg)[4][0] == ops.FGR_ST_SEGMENT
    # a NaN row: NONFINITE
    bad = src.copy()
    bad[7, 1] = np.nan
    for fn in (host, lambda *a, **k: list(reg.fgr_numpy(*a, **k))):
        T, inl, tup, ws, st = fn(bad, tgt, [[0, 50]], tuple_trials=0)
        assert st[0] == ops.FGR_ST_NONFINITE and np.array_equal(T[0], eye) and inl[0] == 0 and ws[0] == 0
    # pure outliers and a tiny number of trials: the tuple test leaves fewer than 3 live correspondences
    rng = np.random.default_rng(5)
    a, b = (rng.uniform(-1.5, 1.5, size=(200, 3)).astype(np.float32) for _ in range(2))
    n = reg.fgr_numpy(a, b, [[0, 200]], tuple_trials=4, seed=3, return_debug=True)
    assert n[4][0] == ops.FGR_ST_FEW and (n[5] > 0).sum() < 3          # the restatement says so for this seed
    h = host(a, b, [[0, 200]], tuple_trials=4, seed=3, return_debug=True)
    assert h[4][0] == ops.FGR_ST_FEW and np.array_equal(h[0][0], eye) and np.array_equal(h[5], n[5])
    # a batch: the pairs do not disturb each other
    s3, g3, seg3 = fc.stack_host([(src, tgt), (src[:2], tgt[:2]), (src[5:45], tgt[5:45])])
    T, inl, tup, ws, st = host(s3, g3, seg3)
    assert list(st) == [0, ops.FGR_ST_FEW, 0]
    assert np.array_equal(T[2], host(src[5:45], tgt[5:45], [[0, 40]], first_pair=2)[0][0])


def test_argument_checks_run_on_the_host():
    src, tgt, _, _ = fc.pose_pair(20, 0.0, 0.0, 1)
    seg = np.array([[0, 20]], dtype=np.int32)
    for kw in (dict(iterations=0), dict(iterations=ops.FGR_MAX_ITERS + 1), dict(division_factor=1.0),
               dict(division_factor=0.5), dict(distance_threshold=0.0), dict(distance_threshold=-1.0),
               dict(distance_threshold=float('inf')), dict(tuple_scale=0.0), dict(tuple_scale=1.01),
               dict(anneal_every=0), dict(tuple_trials=ops.FGR_MAX_TRIALS + 1), dict(max_tuples=-1),
               dict(first_pair=-1)):
        with pytest.raises(ValueError):
            ops.fgr_rigid_host(src, tgt, seg, **kw)
    for bad in ((src.astype(np.float64), tgt, seg), (src, tgt[:10], seg), (src.reshape(-1), tgt.reshape(-1), seg),
                (src, tgt, seg.astype(np.int64)), (src, tgt, seg.reshape(-1)), (src, tgt, seg[:0])):
        with pytest.raises(ValueError):
            ops.fgr_rigid_host(*bad)
    assert ops.fgr_rigid_host(torch.from_numpy(src), torch.from_numpy(tgt), torch.from_numpy(seg))[4][0] == 0
    assert ops.fgr_rigid_host(src, tgt, seg, tuple_scale=1.0, tuple_trials=0, iterations=1)[4][0] == 0   # the ends
    with pytest.raises(RuntimeError):            # the device entry takes no host tensor: no quiet CPU path
        ops.fgr_rigid(torch.from_numpy(src), torch.from_numpy(tgt), torch.from_numpy(seg))
    assert (ops.FGR_ST_FEW, ops.FGR_ST_SINGULAR, ops.FGR_ST_SEGMENT, ops.FGR_ST_NONFINITE) == (1, 2, 4, 8)
    assert reg.FGR_DEFAULTS['iterations'] == 128 and reg.FGR_MAX_TRIALS == ops.FGR_MAX_TRIALS


def test_an_unknown_estimator_raises_before_any_work(tmp_path):
    x = torch.zeros((4, 3))
    with pytest.raises(ValueError):
        reg.estimate_transform(x, x, x[:, 0], x, x, x[:, 0], estimator='nonsense')
    with pytest.raises(ValueError):
        reg.estimate_transforms_from_match(x, None, None, None, None, estimator='nonsense')
    with pytest.raises(ValueError):
        reg.register_scene(str(tmp_path), 'scene', str(tmp_path), estimator='nonsense')
    # the parameters of one estimator are not taken by the other
    with pytest.raises(ValueError):
        reg.register_scene(str(tmp_path), 'scene', str(tmp_path), estimator='fgr', num_hypotheses=10)
    with pytest.raises(ValueError):
        reg.register_scene(str(tmp_path), 'scene', str(tmp_path), fgr=dict(iterations=4))
