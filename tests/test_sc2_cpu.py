"""CPU: the spatial-compatibility estimator -- the host twin of the kernels (ops.sc2_rigid_host; the rule of csrc/sc2.hpp
compiled for the CPU) against the NumPy restatement (registration.sc2_numpy): the bits of the compatibility matrix,
degrees, seeds and consensus sets, the per-seed counts and the winner, recovery down to 3 % inliers, status bits,
argument checks and the estimator= routing.  Nothing here needs a GPU.

The tolerance of T is sc2_cases.T_BOUND = max(1e-9, 100 d0) with d0 = 1.4e-15 measured over fgr_cases.POSE_CASES on the
CPU (profiles/sc2_parity.txt)."""
import numpy as np
import pytest
import torch

import d3feat_pytorch_amd  # noqa: F401
from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.geometric_registration import registration as reg
from test_ransac_gpu import oracle_counts
import fgr_cases as fc
import sc2_cases as sc


def host(src, tgt, seg, **kw):
    return [x.numpy() for x in ops.sc2_rigid_host(src, tgt, np.asarray(seg, dtype=np.int32).reshape(-1, 2), **kw)]


@pytest.mark.parametrize("k", range(len(sc.COUNTS)), ids=lambda k: "n%d" % sc.COUNTS[k])
def test_bits_degrees_seeds_and_sets_equal_the_restatement(k):
    M = sc.COUNTS[k]
    src, tgt = sc.parity_pairs()[k]
    for max_count in (M, sc.next_multiple_of_64(M)):
        for seeds, size in sc.SETTINGS:
            kw = dict(num_seeds=seeds, set_size=size, max_count=max_count, return_debug=True)
            h = host(src, tgt, [[0, M]], **kw)
            n = reg.sc2_numpy(src, tgt, [[0, M]], **kw)
            assert h[10].shape == (1, max_count, (max_count + 63) // 64) and h[10].dtype == np.int64
            assert np.array_equal(h[10], n[10]), "bits of C"
            C = sc.unpack_rows(h[10][0], M)
            assert np.array_equal(C, C.T) and not C.diagonal().any()
            assert np.array_equal(h[5], C.sum(1)) and np.array_equal(h[5], n[5]), "degrees"
            assert np.array_equal(h[6], n[6]), "seed rows"
            assert np.array_equal(h[7], n[7]), "consensus sets"
            # the rule, spelled out once more on the unpacked bits: seeds, then the first set
            order = sorted(range(M), key=lambda i: (-int(h[5][i]), i))[:seeds]
            assert list(h[6][0, :len(order)]) == order and (h[6][0, len(order):] == -1).all()
            i = order[0]
            s2 = (C[i][None, :] & C).sum(1)
            cand = sorted(np.nonzero(C[i])[0], key=lambda j: (-int(s2[j]), j))[:size - 1]
            assert list(h[7][0, 0, :1 + len(cand)]) == [i] + [int(j) for j in cand]
            assert (h[7][0, 0, 1 + len(cand):] == -1).all()


def test_compatibility_against_the_square_root_form():
    tau = 0.1
    total = 0
    for args in ((1531, 0.5, 0.01, 7), (257, 0.3, 0.0, 8), (300, 0.0, 0.0, 9)):
        src, tgt, _, _ = fc.pose_pair(*args)
        C = reg.sc2_compatibility(src, tgt, tau)
        Cs, margin = sc.compat_sqrt(src, tgt, tau)
        diff = C != Cs
        total += C.size
        print("%s: %d of %d entries differ" % (args, diff.sum(), C.size))
        assert (margin[diff] <= 1e-12).all()                # a difference only where the gap IS the threshold
        if args[0] == 1531:
            assert not diff.any()
    assert total > 2e6


@pytest.mark.parametrize("k", [5, 8, 9], ids=lambda k: "n%d" % sc.COUNTS[k])
def test_counts_and_winner_match_the_restatement(k):
    M = sc.COUNTS[k]
    src, tgt = sc.parity_pairs()[k]
    exceptions = 0
    for seeds, size in sc.SETTINGS:
        kw = dict(num_seeds=seeds, set_size=size, return_debug=True)
        h = host(src, tgt, [[0, M]], **kw)
        n = reg.sc2_numpy(src, tgt, [[0, M]], **kw)
        valid = n[8][0] >= 0
        assert np.array_equal(h[8][0] >= 0, valid) and valid.sum() == min(seeds, M)
        rt = n[9][0][valid].astype(np.float64)
        assert np.abs(h[9][0][valid] - rt).max() <= 1e-6
        _, near = oracle_counts(src, tgt, rt[:, :9].reshape(-1, 3, 3), rt[:, 9:])
        diff = np.abs(h[8][0][valid] - n[8][0][valid])
        assert (diff <= near).all(), "a count difference no near-threshold correspondence explains"
        exceptions += int((diff > 0).sum())
        for name in (1, 2, 3, 4):                           # inliers, best_seed, best_count, status
            assert h[name][0] == n[name][0], name
        assert h[4][0] == 0 and h[2][0] == h[6][0, int(np.argmax(h[8][0]))]
        d = float(np.abs(h[0] - n[0]).max())
        print("n %d, %s: |T_host - T_numpy| = %.3e" % (M, (seeds, size), d))
        assert d <= sc.T_BOUND
        assert np.array_equal(h[0][0, 3], [0, 0, 0, 1]) and abs(np.linalg.det(h[0][0, :3, :3]) - 1.0) < 1e-12
    assert exceptions == 0          # these inputs were chosen so: no row sits within rounding reach of the threshold


@pytest.mark.parametrize("case", fc.POSE_CASES, ids=lambda c: "M%d-out%g-sigma%g-s%d" % (c[0], c[1], c[2], c[4]))
def test_pose_cases_recover_the_truth(case):
    M, out, sigma, rng_seed, _ = case
    src, tgt, T0, good = fc.pose_pair(M, out, sigma, rng_seed)
    n = reg.sc2_numpy(src, tgt, [[0, M]], num_seeds=64)
    h = host(src, tgt, [[0, M]], num_seeds=64)
    assert h[4][0] == n[4][0] == 0
    assert np.abs(h[0] - n[0]).max() <= sc.T_BOUND
    br, bt = fc.recovery_bounds(src, tgt, T0, good)
    for name, T in (("numpy", n[0][0]), ("host", h[0][0])):    # first the restatement (a condition on the input)
        er, et = fc.pose_errors(T, T0)
        print("  %s: rot %.3e deg (bound %.3e), trans %.3e m (bound %.3e)" % (name, er, br, et, bt))
        assert er <= br and et <= bt, name
    assert h[1][0] >= 0.95 * good.sum()


@pytest.mark.parametrize("args", sc.LOW_INLIER, ids=lambda a: "seed%d" % a[3])
def test_three_per_cent_inliers_recover_within_one_degree(args):
    src, tgt, T0, good = fc.pose_pair(*args)
    n = reg.sc2_numpy(src, tgt, [[0, args[0]]])
    h = host(src, tgt, [[0, args[0]]])
    for name, res in (("numpy", n), ("host", h)):
        er, et = fc.pose_errors(res[0][0], T0)
        print("  %s: %d true inliers, rot %.3f deg, trans %.4f m, inliers %d" % (name, good.sum(), er, et, res[1][0]))
        assert res[4][0] == 0 and er < sc.ROT_OK_DEG and et < sc.TRANS_OK, name
    assert h[1][0] == n[1][0] and h[2][0] == n[2][0]


def test_status_bits_and_identity():
    src, tgt, _, _ = fc.pose_pair(50, 0.0, 0.0, 21)
    eye = np.eye(4)
    both = (host, lambda *a, **k: list(reg.sc2_numpy(*a, **k)))
    for fn in both:
        # n = 0 and n = 2: FEW; n = 3: a pose
        for cnt in (0, 2):
            T, inl, bs, bc, st = fn(src, tgt, [[0, cnt]])
            assert st[0] == ops.SC2_ST_FEW and np.array_equal(T[0], eye) and inl[0] == 0 and bs[0] == -1 and bc[0] == 0
        T, inl, bs, bc, st = fn(src, tgt, [[4, 3]])
        assert st[0] == 0 and inl[0] == 3 and bc[0] == 3 and bs[0] == 0
        # a segment past the rows, a negative offset, count > max_count: SEGMENT
        for seg, kw in (([[10, 41]], {}), ([[-1, 10]], {}), ([[0, 50]], dict(max_count=49))):
            T, inl, bs, bc, st = fn(src, tgt, seg, **kw)
            assert st[0] == ops.SC2_ST_SEGMENT and np.array_equal(T[0], eye) and inl[0] == 0 and bs[0] == -1
        # all rows of one side identical: |a_i - a_j| = 0 against |b_i - b_j| > tau leaves the matrix empty
        same = np.repeat(src[:1], 50, axis=0)
        T, inl, bs, bc, st = fn(same, tgt, [[0, 50]])
        assert st[0] == ops.SC2_ST_NO_HYPOTHESIS and np.array_equal(T[0], eye) and inl[0] == 0 and bs[0] == -1
    # a NaN row takes no part: its row and column are empty, the pair still succeeds
    bad = src.copy()
    bad[7, 1] = np.nan
    h = host(bad, tgt, [[0, 50]], return_debug=True)
    n = reg.sc2_numpy(bad, tgt, [[0, 50]], return_debug=True)
    C = sc.unpack_rows(h[10][0], 50)
    assert not C[7].any() and not C[:, 7].any() and h[5][7] == 0 and np.array_equal(h[10], n[10])
    assert h[4][0] == n[4][0] == 0 and h[1][0] == n[1][0] == 49 and np.abs(h[0] - n[0]).max() <= sc.T_BOUND
    assert 7 not in h[7][0, :49]
    # a batch: the pairs do not disturb each other
    s3, g3, seg3 = fc.stack_host([(src, tgt), (src[:2], tgt[:2]), (src[5:45], tgt[5:45])])
    T, inl, bs, bc, st = host(s3, g3, seg3, max_count=50)
    assert list(st) == [0, ops.SC2_ST_FEW, 0]
    assert np.array_equal(T[2], host(src[5:45], tgt[5:45], [[0, 40]])[0][0])


def test_identical_rows():
    """All rows of ONE side identical: no two correspondences are compatible (0 against more than tau), the matrix is
    empty -> NO_HYPOTHESIS.  All rows identical on BOTH sides: by rule 1 every two are compatible (0 = 0), and the fit
    over coincident points is the pure translation between them (Horn's matrix is zero, the identity quaternion wins) --
    a pose that puts every row on its partner, not a failure."""
    one = np.ones((20, 3), np.float32)
    spread = (np.arange(60, dtype=np.float32).reshape(20, 3)) * np.float32(0.5)
    for s, g in ((one, spread), (spread, one)):
        h = host(s, g, [[0, 20]], return_debug=True)
        assert h[4][0] == ops.SC2_ST_NO_HYPOTHESIS and (h[5] == 0).all() and (h[8] == -1).all()
        assert np.array_equal(h[0][0], np.eye(4)) and h[1][0] == 0 and h[2][0] == -1
        assert reg.sc2_numpy(s, g, [[0, 20]])[4][0] == ops.SC2_ST_NO_HYPOTHESIS
    h = host(one, 3 * one, [[0, 20]], return_debug=True)
    assert h[4][0] == 0 and (h[5] == 19).all() and h[1][0] == 20 and h[2][0] == 0
    assert np.array_equal(h[0][0, :3, :3], np.eye(3)) and np.array_equal(h[0][0, :3, 3], [-2.0, -2.0, -2.0])


def test_argument_checks_run_on_the_host():
    src, tgt, _, _ = fc.pose_pair(20, 0.0, 0.0, 1)
    seg = np.array([[0, 20]], dtype=np.int32)
    for kw in (dict(max_count=0), dict(max_count=ops.SC2_MAX_COUNT + 1), dict(set_size=2),
               dict(set_size=ops.SC2_MAX_SET + 1), dict(num_seeds=0), dict(num_seeds=ops.SC2_MAX_SEEDS + 1),
               dict(refine_iters=-1), dict(refine_iters=ops.RANSAC_MAX_REFINE + 1), dict(distance_threshold=0.0),
               dict(distance_threshold=float('inf')), dict(compat_threshold=0.0), dict(compat_threshold=-0.1),
               dict(compat_threshold=float('inf')), dict(compat_threshold=float('nan'))):
        with pytest.raises(ValueError):
            ops.sc2_rigid_host(src, tgt, seg, **kw)
    for bad in ((src.astype(np.float64), tgt, seg), (src, tgt[:10], seg), (src.reshape(-1), tgt.reshape(-1), seg),
                (src, tgt, seg.astype(np.int64)), (src, tgt, seg.reshape(-1)), (src, tgt, seg[:0]),
                (src, tgt, np.zeros((65536, 2), np.int32))):
        with pytest.raises(ValueError):
            ops.sc2_rigid_host(*bad)
    # the ends of every limit
    for kw in (dict(max_count=20), dict(max_count=ops.SC2_MAX_COUNT, num_seeds=1), dict(set_size=3),
               dict(set_size=ops.SC2_MAX_SET), dict(num_seeds=1), dict(num_seeds=ops.SC2_MAX_SEEDS),
               dict(refine_iters=0), dict(refine_iters=ops.RANSAC_MAX_REFINE)):
        assert ops.sc2_rigid_host(src, tgt, seg, **kw)[4][0] == 0, kw
    assert ops.sc2_rigid_host(src, tgt, np.tile(seg, (65535, 1)), num_seeds=1, set_size=3, refine_iters=0)[4].sum() == 0
    assert ops.sc2_rigid_host(torch.from_numpy(src), torch.from_numpy(tgt), torch.from_numpy(seg))[4][0] == 0
    with pytest.raises(RuntimeError):            # the device entry takes no host tensor: no quiet CPU path
        ops.sc2_rigid(torch.from_numpy(src), torch.from_numpy(tgt), torch.from_numpy(seg))
    assert (ops.SC2_ST_FEW, ops.SC2_ST_NO_HYPOTHESIS, ops.SC2_ST_SEGMENT) == (1, 2, 4)
    assert (ops.SC2_MAX_COUNT, ops.SC2_MAX_SET, ops.SC2_MAX_SEEDS) == (8192, 64, 4096)
    assert (reg.SC2_ST_FEW, reg.SC2_ST_NO_HYPOTHESIS, reg.SC2_ST_SEGMENT) == (1, 2, 4)
    assert reg.SC2_MAX_COUNT == ops.SC2_MAX_COUNT
    assert reg.SC2_DEFAULTS == dict(distance_threshold=0.05, compat_threshold=0.1, num_seeds=256, set_size=20,
                                    refine_iters=3)


def test_estimator_keywords_are_checked_before_any_work(tmp_path):
    x = torch.zeros((4, 3))
    where = (str(tmp_path), 'scene', str(tmp_path))
    with pytest.raises(ValueError):               # RANSAC keywords with the other estimator
        reg.register_scene(*where, estimator='sc2', num_hypotheses=10)
    with pytest.raises(ValueError):
        reg.estimate_transform(x, x, x[:, 0], x, x, x[:, 0], estimator='sc2', seed=1)
    with pytest.raises(ValueError):
        reg.estimate_transforms_from_match(x, None, None, None, None, estimator='sc2', edge_ratio=0.5)
    for kw in (dict(sc2=dict(num_seeds=4)), dict(estimator='ransac', sc2={}), dict(estimator='fgr', sc2=dict(set_size=5)),
               dict(estimator='sc2', fgr=dict(iterations=4)), dict(estimator='sc2', sc2=[1, 2])):
        with pytest.raises(ValueError):
            reg.register_scene(*where, **kw)
        with pytest.raises(ValueError):
            reg.estimate_transform(x, x, x[:, 0], x, x, x[:, 0], **kw)
        with pytest.raises(ValueError):
            reg.estimate_transforms_from_match(x, None, None, None, None, **kw)
