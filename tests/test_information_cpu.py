"""CPU: the information matrix of a fragment pair (registration.information_numpy / information_from_moments) against a
brute-force sum of G^T G, the identities that tie its frame to transformation_error, the structure of the benchmark's
own gt.info blocks, the gt.info writer, and build_benchmark on the NumPy path -- nothing here needs a GPU."""
import os

import numpy as np
import pytest

import d3feat_pytorch_amd  # noqa: F401
from d3feat_pytorch_amd.datasets.preprocess import nearest_pairs_numpy
from d3feat_pytorch_amd.geometric_registration import evaluate as ev
from d3feat_pytorch_amd.geometric_registration import registration as reg
import icp_scene as sc

REF = "/root/reference"
R = 0.075
SHIFT = (300.0, -200.0, 50.0)


def cross_matrix(p):
    return np.array([[0.0, -p[2], p[1]], [p[2], 0.0, -p[0]], [-p[1], p[0], 0.0]])


def brute_information(points, rotation_first=False):
    """sum of G^T G over the f64 ``points``, one 6x6 product per point: G = [I | -[p]x], or [-[p]x | I] (Open3D's
    get_information_matrix_from_point_clouds, from its formula)."""
    out = np.zeros((6, 6))
    for p in np.asarray(points, dtype=np.float64):
        G = np.hstack([-cross_matrix(p), np.eye(3)] if rotation_first else [np.eye(3), -cross_matrix(p)])
        out += G.T @ G
    return out


def gt_pairs(shift=(0.0, 0.0, 0.0)):
    """The six pairs (moving j, fixed i), i < j, of make_scene(4, 4) under their ground-truth poses."""
    clouds, poses = sc.make_scene(4, 4)
    clouds = sc.shift_clouds(clouds, shift)
    pairs = np.asarray([(j, i) for i in range(4) for j in range(i + 1, 4)])
    G = np.stack([sc.shift_pose(sc.gt_transform(poses, i, j), shift) for j, i in pairs])
    return clouds, pairs, G


@pytest.fixture(scope="module")
def scene():
    clouds, pairs, G = gt_pairs()
    moments, count = reg.information_numpy(clouds, pairs, G, R)
    nn, want, row_start = nearest_pairs_numpy(clouds, pairs, G, R)
    return clouds, pairs, G, moments, count, (nn, want, row_start)


def test_information_equals_brute_force_sum_in_both_frames_and_orders(scene):
    """1e-12 * max|entry|: about 1e4 terms per sum in f64 (pairwise: error ~ log2(n) 2^-53) of exact products."""
    clouds, pairs, G, moments, count, (nn, want, row_start) = scene
    assert moments.shape == (6, 20) and np.array_equal(count, want) and np.array_equal(moments[:, 0], want)
    for p, (a, b) in enumerate(pairs):
        res = nn[row_start[p]:row_start[p + 1]]
        sel = res >= 0
        assert sel.sum() > 1000
        pts = {'moving': clouds[a][sel], 'fixed': clouds[b][res[sel]]}
        for frame in ('moving', 'fixed'):
            for order in ('translation_first', 'rotation_first'):
                got = reg.information_from_moments(moments[p:p + 1], frame, order)
                assert got.shape == (1, 6, 6) and got.dtype == np.float64
                ref = brute_information(pts[frame], order == 'rotation_first')
                err = np.abs(got[0] - ref).max() / np.abs(ref).max()
                print("pair %d %s %s: n = %d, rel. diff %.2e" % (p, frame, order, want[p], err))
                assert err <= 1e-12
    assert np.array_equal(reg.information_from_moments(np.zeros((2, 20))), np.zeros((2, 6, 6)))
    with pytest.raises(ValueError):
        reg.information_from_moments(moments, frame='world')
    with pytest.raises(ValueError):
        reg.information_from_moments(moments[:, :17])


def test_information_from_moments_takes_tensors():
    import torch
    m = np.random.default_rng(0).normal(size=(3, 20))
    for frame in ('moving', 'fixed'):
        for order in ('translation_first', 'rotation_first'):
            got = reg.information_from_moments(torch.from_numpy(m), frame, order)
            assert isinstance(got, torch.Tensor) and got.dtype == torch.float64
            assert np.array_equal(got.numpy(), reg.information_from_moments(m, frame, order))


@pytest.mark.parametrize("shift", [(0.0, 0.0, 0.0), SHIFT], ids=["as-generated", "shifted"])
def test_frame_identities_with_transformation_error(shift):
    """With the information matrix in the MOVING frame, transformation_error of a pure translation d is |d|^2, and of a
    pure rotation D (angle a about the unit axis u through the origin) it is sum |D x - x|^2 / (4 n), because
    |R x - x| = 2 sin(a/2) |u x x|.  The rotation identity fails by a wide margin with frame='fixed' (the fixed points
    are the same surface in ANOTHER frame, a rigid motion of order 1 away: a relative change of order 1 as generated
    and of order 1/360 at (300, -200, 50); asserted: more than 1e-4, a million times the tolerance).  The translation
    identity cannot tell the frames apart -- the top-left block is n I in both -- so it is asserted to hold in both."""
    clouds, pairs, G = gt_pairs(shift)
    p = 1
    a, b = pairs[p]
    moments, count = reg.information_numpy(clouds, pairs[p:p + 1], G[p:p + 1], R)
    nn = nearest_pairs_numpy(clouds, pairs[p:p + 1], G[p:p + 1], R)[0]
    x = clouds[a][nn >= 0].astype(np.float64)
    info = reg.information_from_moments(moments)[0]
    info_fixed = reg.information_from_moments(moments, frame='fixed')[0]
    assert info[0, 0] == len(x) == count[0]
    rng = np.random.default_rng(5)
    for d in ([0.25, 0.0, 0.0], [0.03, -0.11, 0.07]):
        D = np.eye(4)
        D[:3, 3] = d
        for mat in (info, info_fixed):
            e = reg.transformation_error(G[p] @ D, G[p], mat)
            print("translation %s: error %.15f, |d|^2 %.15f" % (d, e, np.dot(d, d)))
            assert abs(e - np.dot(d, d)) <= 1e-12
    for angle in (0.05, 0.4):
        D = np.eye(4)
        D[:3, :3] = sc.rotation(rng, angle)
        moved = ((x @ D[:3, :3].T - x) ** 2).sum()
        e = reg.transformation_error(G[p] @ D, G[p], info)
        rel = abs(moved - 4 * info[0, 0] * e) / moved
        e_fixed = reg.transformation_error(G[p] @ D, G[p], info_fixed)
        rel_fixed = abs(moved - 4 * info_fixed[0, 0] * e_fixed) / moved
        print("rotation %.2f rad: rel. diff %.2e (moving frame), %.2e (fixed frame)" % (angle, rel, rel_fixed))
        assert rel <= 1e-10
        assert rel_fixed > 1e-4


def assert_benchmark_structure(block, tol):
    """The four properties of a benchmark block: top-left n I; top-right -[s]x; symmetric; BR - (|s|^2 I - s s^T) / n
    positive semi-definite (Cauchy-Schwarz: sum |u x p|^2 >= |u x sum p|^2 / n).  Returns min eigenvalue / trace."""
    scale = np.abs(block).max()
    n = block[0, 0]
    assert n > 0 and np.abs(block[:3, :3] - n * np.eye(3)).max() <= tol * scale
    TR = block[:3, 3:]
    s = np.array([TR[1, 2], -TR[0, 2], TR[0, 1]])
    assert np.abs(TR + cross_matrix(s)).max() <= tol * scale
    assert np.abs(block - block.T).max() <= tol * scale
    rest = block[3:, 3:] - (np.dot(s, s) * np.eye(3) - np.outer(s, s)) / n
    w = np.linalg.eigvalsh(rest)
    assert w[0] > 0
    return w[0] / np.trace(block[3:, 3:])


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "geometric_registration", "gt_result")),
                    reason="reference benchmark files not mounted")
def test_shipped_gt_info_blocks_have_the_structure_of_the_moving_frame_form():
    """Every block of the eight gt.info files, to their nine printed digits (2e-8 of the block's largest entry)."""
    root = os.path.join(REF, "geometric_registration", "gt_result")
    blocks, least = 0, np.inf
    for scene_dir in sorted(os.listdir(root)):
        if not os.path.exists(os.path.join(root, scene_dir, 'gt.info')):
            continue
        for key, block in reg.loadinfo(os.path.join(root, scene_dir)).items():
            least = min(least, assert_benchmark_structure(block, 2e-8))
            blocks += 1
    print("%d blocks, smallest eigenvalue / trace %.2e" % (blocks, least))
    assert blocks == 1623


def test_information_numpy_blocks_have_the_benchmark_structure(scene):
    clouds, pairs, G, moments, count, _ = scene
    for block in reg.information_from_moments(moments):
        assert_benchmark_structure(block, 1e-15)


def test_writeinfo_round_trip(tmp_path, scene):
    moments = scene[3]
    mats = reg.information_from_moments(moments)
    info = {'2_11': mats[0], '0_3': mats[1], '0_12': mats[2], '10_11': mats[3]}
    reg.writeinfo(str(tmp_path / 'a'), info, 37)
    back = reg.loadinfo(str(tmp_path / 'a'))
    assert sorted(back) == sorted(info)
    for key in info:
        assert (np.abs(back[key] - info[key]) <= 1e-8 * np.abs(info[key])).all(), key
    with open(str(tmp_path / 'a' / 'gt.info')) as f:
        lines = f.read().splitlines()
    heads = [tuple(int(v) for v in ln.split()) for ln in lines[0::7]]
    assert heads == [(0, 3, 37), (0, 12, 37), (2, 11, 37), (10, 11, 37)]          # ordered by (i, j), num_frag kept
    assert lines[0] == '0\t 3\t 37\t' and len(lines) == 28
    assert lines[1] == ''.join(' % .8e\t ' % v for v in info['0_3'][0]).rstrip(' ')
    reg.writeinfo(str(tmp_path / 'b'), {}, 5)
    assert os.path.getsize(str(tmp_path / 'b' / 'gt.info')) == 0
    assert reg.loadinfo(str(tmp_path / 'b')) == {}
    with pytest.raises(ValueError):
        reg.writeinfo(str(tmp_path / 'c'), {'0_1': np.eye(4)}, 2)


def brute_overlap(moving, fixed, T, radius):
    """Share of the f64-moved ``moving`` points with a ``fixed`` point closer than ``radius``; also the number of points
    whose nearest distance lies within 1e-4 of the radius (where the f32 rule of the search may decide otherwise)."""
    q = moving.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    y = fixed.astype(np.float64)
    near = np.empty(len(q))
    for s in range(0, len(q), 256):
        near[s:s + 256] = np.sqrt(((q[s:s + 256, None, :] - y[None, :, :]) ** 2).sum(-1).min(1))
    return float((near < radius).mean()), int((np.abs(near - radius) < 1e-4).sum())


def five_fragments():
    """5 fragments whose view centres are 1.4 apart: overlaps from 0.03 to 1.0, fragments of 239 to 7857 points."""
    return sc.make_scene(4, 5, spacing=1.4)


def test_build_benchmark_on_the_numpy_path(tmp_path):
    clouds, poses = five_fragments()
    out = str(tmp_path / 'gt')
    gt, info, overlap = reg.build_benchmark(clouds, poses, out, None, radius=R, device='cpu')
    want = set()
    for i in range(5):
        for j in range(i + 1, 5):
            share, band = brute_overlap(clouds[j], clouds[i], sc.gt_transform(poses, i, j), R)
            key = '%d_%d' % (i, j)
            print("%s: brute-force overlap %.4f, built %s, %d rows at the radius" % (
                key, share, overlap.get(key), band))
            assert abs(share - 0.3) > (band + 1) / len(clouds[j])      # the scene decides every pair clearly
            if key in overlap:
                assert abs(overlap[key] - share) <= band / len(clouds[j])
            else:
                assert share == 0.0                                     # dropped by the box prefilter
            if share > 0.3:
                want.add(key)
    assert set(gt) == set(info) == want and 0 < len(want) < 10
    assert any(reg._far(k) for k in want)
    for key in gt:
        i, j = (int(v) for v in key.split('_'))
        assert np.array_equal(gt[key], np.linalg.inv(poses[i]) @ poses[j])
    # the files are what loadlog / loadinfo read
    log, inf = ev.loadlog(out), reg.loadinfo(out)
    assert sorted(log) == sorted(inf) == sorted(want)
    for key in want:
        assert np.abs(log[key] - gt[key]).max() <= 1e-8 * max(1.0, np.abs(gt[key]).max())
        assert np.abs(inf[key] - info[key]).max() <= 1e-8 * np.abs(info[key]).max()
    recall, precision, errs = reg.evaluate_registration(gt, gt, info)
    assert recall == 1.0 and precision == 1.0 and max(errs.values()) <= 1e-20
    D = np.eye(4)
    D[0, 3] = 0.25                                                       # in the moving frame: error |d|^2 = 0.0625
    recall, precision, errs = reg.evaluate_registration({k: T @ D for k, T in gt.items()}, gt, info)
    assert recall == 0.0 and len(errs) == sum(reg._far(k) for k in gt)
    for key in gt:
        assert abs(reg.transformation_error(gt[key] @ D, gt[key], info[key]) - 0.0625) <= 1e-12, key
    # symmetric never removes a key, and never lowers an overlap
    gs, infs, ovs = reg.build_benchmark(clouds, poses, str(tmp_path / 'sym'), None, radius=R, device='cpu',
                                        symmetric=True)
    assert set(gs) >= set(gt) and all(ovs[k] >= overlap[k] for k in overlap)
    for key in gt:
        assert np.array_equal(infs[key], info[key])
    # a different info_distance changes the matrices and not the keys
    g2, inf2, ov2 = reg.build_benchmark(clouds, poses, str(tmp_path / 'near'), None, radius=R, device='cpu',
                                        info_distance=0.02)
    assert set(g2) == set(gt) and ov2 == overlap
    assert all(inf2[k][0, 0] < info[k][0, 0] for k in gt)
    with pytest.raises(ValueError):
        reg.build_benchmark(clouds, poses[:4], out, None, radius=R, device='cpu')
    with pytest.raises(ValueError):
        reg.build_benchmark(clouds, poses, out, None, device='cpu')
