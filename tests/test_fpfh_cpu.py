"""CPU: the FPFH rule (csrc/fpfh.hpp).  The NumPy restatement against an oracle written the way Open3D writes it, the
host twin against the restatement bit for bit, the edge cases against rows worked out by hand, and the dump that
``register_one_scene(desc_name='FPFH')`` reads."""
import os

import numpy as np
import pytest

from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.geometric_registration import evaluate as ev
from d3feat_pytorch_amd.geometric_registration import registration as reg
import fpfh_cases as fc
import icp_scene as sc

# f32 rounding of a value near 100 is 100 * 2^-24 = 6e-6; 1e-4 is the project's fp32 descriptor tolerance
ORACLE_TOL = 1e-4


@pytest.mark.parametrize("seed", fc.SEEDS)
def test_restatement_matches_the_independent_oracle(seed):
    clouds, _, normals, _ = fc.scene(seed)
    nrm = fc.zeroed(normals)
    desc, count, spfh = reg.fpfh_numpy(list(clouds), fc.R_FPFH, nrm, return_spfh=True)
    assert desc.dtype == np.float32 and desc.shape == (len(nrm), 33) and count.dtype == np.int32
    lo = 0
    for c in clouds:
        hi = lo + len(c)
        want_desc, want_count, want_spfh = fc.oracle(c, nrm[lo:hi], fc.R_FPFH)
        assert np.array_equal(count[lo:hi], want_count)
        assert np.array_equal(spfh[lo:hi], want_spfh)
        err = np.abs(desc[lo:hi].astype(np.float64) - want_desc).max()
        print("seed %d cloud of %d: up to %d neighbours, |desc - oracle| <= %.3g" % (seed, len(c), want_count.max(), err))
        assert err <= ORACLE_TOL
        # a point without a normal is skipped as a neighbour and has no descriptor
        dead = ~(nrm[lo:hi] != 0).any(1)
        assert dead.sum() > 10 and (count[lo:hi][dead] == 0).all() and (desc[lo:hi][dead] == 0).all()
        assert (desc[lo:hi][count[lo:hi] > 0].reshape(-1, 3, 11).sum(2) > 199.99).all()     # 100 + 100 per histogram
        lo = hi


def test_the_cap_is_part_of_the_rule():
    """Without the cap a neighbour within radius / 64 dominates the descriptor: the rows that have one move."""
    clouds, _, normals, _ = fc.scene(fc.SEEDS[0])
    c, nrm = clouds[0], normals[:len(clouds[0])]
    capped, uncapped = fc.oracle(c, nrm, fc.R_FPFH)[0], fc.oracle(c, nrm, fc.R_FPFH, cap=False)[0]
    moved = np.abs(capped - uncapped).max(1) > ORACLE_TOL
    assert 0 < moved.sum() < 100


@pytest.mark.parametrize("seed", fc.SEEDS)
def test_host_twin_equals_the_restatement_bit_for_bit(seed):
    clouds, _, normals, _ = fc.scene(seed)
    nrm = fc.zeroed(normals)
    want = reg.fpfh_numpy(list(clouds), fc.R_FPFH, nrm, return_spfh=True)
    got = ops.fpfh_host(np.concatenate(clouds), [len(c) for c in clouds], fc.R_FPFH, nrm, return_spfh=True)
    for g, w in zip(got, want):
        assert np.array_equal(g.numpy(), w)
    wide = ops.fpfh_host(np.concatenate(clouds), [len(c) for c in clouds], fc.R_FPFH, nrm, row_width=64)[0].numpy()
    assert wide.shape[1] == 64 and np.array_equal(wide[:, :33], want[0]) and (wide[:, 33:] == 0).all()
    # unit rows, what the matching kernel reads: the same bits, norm 1 to f32 rounding, zeros stay zeros
    unit = reg.fpfh_numpy(list(clouds), fc.R_FPFH, nrm, unit=True)[0]
    got = ops.fpfh_host(np.concatenate(clouds), [len(c) for c in clouds], fc.R_FPFH, nrm, row_width=64, unit=True)[0]
    assert np.array_equal(got.numpy()[:, :33], unit) and (got.numpy()[:, 33:] == 0).all()
    norms = np.linalg.norm(unit.astype(np.float64), axis=1)
    assert (np.abs(norms[want[1] > 0] - 1) < 1e-6).all() and (unit[want[1] == 0] == 0).all()
    scaled = want[0] / np.linalg.norm(want[0].astype(np.float64), axis=1, keepdims=True).clip(1e-30)
    assert np.abs(unit - scaled).max() < 1e-6


@pytest.mark.parametrize("case", fc.edge_cases(), ids=lambda c: c[0].replace(" ", "_"))
def test_edge_cases(case):
    _, pts, nrm, radius, count, spfh, desc = case
    for got in (reg.fpfh_numpy([pts], radius, nrm, return_spfh=True),
                tuple(t.numpy() for t in ops.fpfh_host(pts, [len(pts)], radius, nrm, return_spfh=True))):
        assert np.array_equal(got[1], count)
        assert np.array_equal(got[2], spfh)
        assert np.array_equal(got[0], desc)


def test_argument_checks():
    pts, nrm = np.zeros((2, 3), np.float32), np.ones((2, 3), np.float32)
    with pytest.raises(ValueError):
        ops.fpfh_host(pts, [2], 0.1, nrm, row_width=32)
    with pytest.raises(ValueError):
        ops.fpfh_host(pts, [2], 0.0, nrm)
    with pytest.raises(ValueError):
        ops.fpfh_host(pts, [3], 0.1, nrm)
    with pytest.raises(ValueError):
        ops.fpfh_host(pts, [2], 0.1, nrm[:1])
    with pytest.raises(ValueError):
        reg.fpfh_numpy([pts], 0.1, nrm[:1])
    assert ops.fpfh_bytes(10, 100) > ops.fpfh_bytes(10) > 0


def test_terrain_matches_are_inliers_often_enough():
    """What makes the end-to-end test on the device a test of the code and not of luck: on the fixture seeds at least
    0.15 of the restatement's mutual matches lie within 0.05 m of the truth.  The matches are those of the unit rows,
    which the matching kernel reads."""
    for seed in fc.SEEDS:
        clouds, poses, _, _ = fc.scene(seed)
        _, count, _, desc = fc.restated(seed)
        na = len(clouds[0])
        rows, cols = fc.mutual_numpy(desc[:na], desc[na:])
        keep = (count[:na][rows] > 0) & (count[na:][cols] > 0)
        rows, cols = rows[keep], cols[keep]
        G = sc.gt_transform(poses, 0, 1)
        moved = clouds[1][cols].astype(np.float64) @ G[:3, :3].T + G[:3, 3]
        ratio = (np.linalg.norm(clouds[0][rows] - moved, axis=1) < 0.05).mean()
        print("seed %d: %d mutual matches, %.3f within 0.05 m" % (seed, len(rows), ratio))
        assert ratio >= 0.15


def test_generate_fpfh_features_writes_the_registration_layout(tmp_path):
    clouds = fc.scene(fc.SEEDS[0])[0]
    frags = [c[:400] for c in clouds]      # (a thin sample: the normals need the descriptor's radius)
    out = []
    for run in ("a", "b", "other_seed"):
        root = str(tmp_path / run)
        ev.generate_fpfh_features({"terrain": frags}, root, fc.R_FPFH, fc.R_FPFH, seed=5 if run != "other_seed" else 6,
                                  device="cpu")
        dpath, kpath, spath = ev._paths(root, "terrain")
        assert sorted(os.listdir(dpath)) == ["cloud_bin_0.FPFH.npy", "cloud_bin_1.FPFH.npy"]
        got = []
        for k, c in enumerate(frags):
            name = "cloud_bin_%d" % k
            desc, pts, score = ev.get_desc(dpath, name, "FPFH"), ev.get_keypts(kpath, name), ev.get_scores(spath, name)
            assert desc.dtype == np.float32 and desc.shape == (len(c), 64) and (desc[:, 33:] == 0).all()
            assert np.array_equal(pts, c) and score.dtype == np.float32 and score.shape == (len(c), 1)
            described = (desc != 0).any(1)
            assert described.sum() > len(c) // 2
            assert ((score[:, 0] > 0) == described).all() and (score <= 1).all()
            got.append((desc, score))
        out.append(got)
    want = reg.describe_fpfh(frags, fc.R_FPFH, fc.R_FPFH, device="cpu")[0]
    for k in range(2):
        assert np.array_equal(out[0][k][0], want[k])
        assert np.array_equal(out[0][k][0], out[1][k][0]) and np.array_equal(out[0][k][1], out[1][k][1])
        assert not np.array_equal(out[0][k][1], out[2][k][1])
