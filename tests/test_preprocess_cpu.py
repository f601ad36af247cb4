"""CPU: the writer of the 3DMatch training pickles (datasets/preprocess.py) on its NumPy path -- round trip through
``ThreeDMatchDataset``, the mining rule against an independent f64 kd-tree, the bounding-box prefilter, the file
readers and the degenerate scenes."""
import pickle
import random

import numpy as np
import pytest

from d3feat_pytorch_amd.datasets import ThreeDMatch as tdm
from d3feat_pytorch_amd.datasets import preprocess as pp
from preprocess_scene import make_scene, pose, write_scene

VOXEL = 0.03
RADIUS = 1.25 * VOXEL


@pytest.fixture(scope="module")
def subsample(native):
    def fn(points, voxel):
        p = np.ascontiguousarray(points, dtype=np.float32)
        return native.subsample_batch(p, np.array([p.shape[0]], dtype=np.int32), sampleDl=voxel)[0]
    return fn


@pytest.fixture(scope="module")
def scene():
    return make_scene(6)


def test_round_trip_through_the_dataset(tmp_path, scene, subsample):
    frags, poses = scene
    write_scene(tmp_path, 'synth-a', frags, poses, how='info')
    pts_file, key_file = pp.build_pickles(str(tmp_path), 'train', ['synth-a'], VOXEL, device='cpu', subsample=subsample)
    assert pts_file.endswith('3DMatch_train_0.030_points.pkl') and key_file.endswith('3DMatch_train_0.030_keypts.pkl')
    with open(key_file, 'rb') as f:
        keypts = pickle.load(f)
    with open(pts_file, 'rb') as f:
        points = pickle.load(f)
    assert list(points) == ['synth-a/cloud_bin_%d' % i for i in range(6)]
    assert all(v.dtype == np.float32 and v.ndim == 2 and v.shape[1] == 3 for v in points.values())
    # the neighbouring windows share 70 % of their extent, windows three apart 10 %: the structure is known
    for k in range(5):
        assert 'synth-a/cloud_bin_%d@synth-a/cloud_bin_%d' % (k, k + 1) in keypts
    assert not any('cloud_bin_0@synth-a/cloud_bin_%d' % k in key for key in keypts for k in (3, 4, 5))
    for key, c in keypts.items():
        src, tgt = key.split('@')
        assert c.ndim == 2 and c.shape[1] == 2 and c.dtype.kind == 'i'
        assert np.all(np.diff(c[:, 0]) > 0)                         # rows ascend in the source index, one per source
        assert c[:, 0].max() < len(points[src]) and c[:, 1].max() < len(points[tgt]) and c.min() >= 0
        assert len(c) > 0.3 * len(points[src])
    ds = tdm.ThreeDMatchDataset(str(tmp_path), 'train', num_node=64, downsample=VOXEL, augment_noise=0.0,
                                augment_rotation=0.0, augment_translation=0.0)
    assert len(ds) == len({k.split('@')[0] for k in keypts})
    ids = list(points)
    for index in range(len(ds)):
        random.seed(index)
        np.random.seed(index)
        item = ds[index]
        assert len(item) == 6
        src_pts, tgt_pts, feat0, feat1, sel, dist = item
        assert sel.shape == (64, 2) and dist.shape == (64, 64)
        assert sel[:, 0].max() < len(src_pts) and sel[:, 1].max() < len(tgt_pts) and sel.min() >= 0
        # which pair was drawn: the source is fixed by the index, the target by its point count and correspondences
        i = ids.index(ds._sources[index])
        hits = 0
        for j in range(6):
            key = '%s@%s' % (ids[i], ids[j])
            if key not in keypts or len(points[ids[j]]) != len(tgt_pts) or \
                    not np.array_equal(points[ids[j]].astype(np.float64), tgt_pts):
                continue
            T = np.linalg.inv(poses[j]) @ poses[i]
            moved = src_pts[sel[:, 0]] @ T[:3, :3].T + T[:3, 3]
            d = np.linalg.norm(moved - tgt_pts[sel[:, 1]], axis=1)
            assert d.max() < RADIUS * (1 + 1e-5), (key, d.max())
            hits += 1
        assert hits == 1


def _two_planes(rng, n=6000, edge=1.6):
    """Floor and wall of ``edge`` x ``edge`` with sigma 0.004 jitter, f32."""
    ab = rng.random((n, 2)) * edge
    pts = np.zeros((n, 3))
    pts[:n // 2, 0], pts[:n // 2, 1] = ab[:n // 2, 0], ab[:n // 2, 1]
    pts[n // 2:, 0], pts[n // 2:, 2] = ab[n // 2:, 0], ab[n // 2:, 1]
    return (pts + rng.normal(scale=0.004, size=pts.shape)).astype(np.float32)


def test_numpy_rule_against_f64_kdtree():
    """The f32 rule and an f64 kd-tree on the same rounded query positions may differ only where f32 and f64 disagree:
    rows whose nearest f64 distance lies within 1e-6 (relative) of the radius, or whose two nearest f64 distances lie
    within 1e-6 (relative) of each other, are left out -- at most 0.1 % of the rows -- and all others are equal."""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(11)
    total = left_out = 0
    for angle, shift in ((0.02, (0.35, 0.01, 0.0)), (-0.03, (0.6, -0.01, 0.01)), (0.05, (0.8, 0.0, -0.01)),
                         (0.01, (0.95, 0.02, 0.0))):
        src, tgt = _two_planes(rng), _two_planes(rng)
        T = pose(angle, shift)
        q = pp.transform_points(src, T)
        ref = (src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
        assert np.abs(q.astype(np.float64) - ref).max() < 1e-6      # the stated order against a plain f64 product
        nn = pp.nearest_within(q, tgt, RADIUS)
        d, idx = cKDTree(tgt.astype(np.float64)).query(q.astype(np.float64), k=2)
        near_radius = np.abs(d[:, 0] - RADIUS) <= 1e-6 * RADIUS
        near_tie = (d[:, 1] - d[:, 0]) <= 1e-6 * d[:, 1]
        skip = near_radius | near_tie
        want = np.where(d[:, 0] < RADIUS, idx[:, 0], -1)
        share = float((nn >= 0).mean())
        print("pair angle=%g shift=%s: matched %.1f %%, left out %d" % (angle, shift, 100 * share, int(skip.sum())))
        assert 0.3 < share < 0.9
        assert np.array_equal(nn[~skip], want[~skip])
        total += len(q)
        left_out += int(skip.sum())
    assert left_out <= 0.001 * total, (left_out, total)


def test_numpy_rule_ties_and_strict_radius():
    """Equal d2: the lowest target index; a point at exactly the radius is rejected; duplicates are legal."""
    tgt = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, 1, 0], [3, 0, 0]], dtype=np.float32)
    q = np.array([[0, 0, 0], [0.5, 0.5, 0], [4, 0, 0], [5, 0, 0], [0, 0.25, 0]], dtype=np.float32)
    assert pp.nearest_within(q, tgt, 1.0).tolist() == [-1, 0, -1, -1, 1]
    assert pp.nearest_within(q, tgt, np.float32(1.0000001)).tolist() == [0, 0, 4, -1, 1]
    nn, count, row_start = pp.nearest_pairs_numpy([q, tgt], [[0, 1], [1, 1]], np.stack([np.eye(4)] * 2), 1.0)
    assert row_start.tolist() == [0, 5, 10] and count.tolist() == [2, 5]
    assert nn[5:].tolist() == [0, 1, 2, 1, 4]                       # a duplicate finds the lower index of the two


def test_prefilter_drops_no_pair_with_a_match(scene, subsample):
    frags, poses = make_scene(8, window=0.3, stride=0.1)
    clouds = pp.subsample_fragments(frags, VOXEL, subsample, 'cpu')
    _, corr_f, ov_f = pp.mine_scene(clouds, poses, None, radius=RADIUS, min_overlap=0.0, device='cpu',
                                    return_overlap=True)
    _, corr_a, ov_a = pp.mine_scene(clouds, poses, None, radius=RADIUS, min_overlap=0.0, device='cpu', prefilter=False,
                                    return_overlap=True)
    assert len(ov_a) == 28 and len(ov_f) < 28                       # it does drop pairs ...
    assert all(ov_a[k] == 0.0 for k in ov_a if k not in ov_f)       # ... and only ones without a single match
    assert list(corr_f) == list(corr_a) and all(np.array_equal(corr_f[k], corr_a[k]) for k in corr_a)
    assert all(ov_f[k] == ov_a[k] for k in ov_f)


def test_symmetric_keeps_a_superset(scene, subsample):
    frags, poses = scene
    clouds = pp.subsample_fragments(frags, VOXEL, subsample, 'cpu')
    for thr in (0.3, 0.45):
        _, one = pp.mine_scene(clouds, poses, None, radius=RADIUS, min_overlap=thr, device='cpu')
        _, both, ov = pp.mine_scene(clouds, poses, None, radius=RADIUS, min_overlap=thr, symmetric=True, device='cpu',
                                    return_overlap=True)
        assert set(one) <= set(both)
        assert all(np.array_equal(one[k], both[k]) for k in one)    # the stored list is the i -> j one either way
        assert all(i < j for i, j in both)
    # the windows differ in size, so the two directions differ in their ratio: somewhere the reverse one decides
    _, fwd_ov = pp.mine_scene(clouds, poses, None, radius=RADIUS, device='cpu', return_overlap=True)[1:]
    assert any(ov[k] > fwd_ov[k] for k in ov)


def test_explicit_pairs_equal_the_scene_form(scene, subsample):
    frags, poses = scene
    clouds = pp.subsample_fragments(frags, VOXEL, subsample, 'cpu')
    _, corr = pp.mine_scene(clouds, poses, None, radius=RADIUS, device='cpu')
    pairs = [(i, j) for i in range(6) for j in range(i + 1, 6)]
    T = [np.linalg.inv(poses[j]) @ poses[i] for i, j in pairs]
    _, corr2 = pp.mine_pairs(clouds, pairs, T, radius=RADIUS, device='cpu')
    assert list(corr) == list(corr2) and all(np.array_equal(corr[k], corr2[k]) for k in corr)
    with pytest.raises(ValueError):
        pp.mine_pairs(clouds, [(0, 6)], [np.eye(4)], radius=RADIUS, device='cpu')
    with pytest.raises(ValueError):                                 # no CPU subsampler in the package
        pp.mine_scene(frags, poses, VOXEL, device='cpu')


def test_pose_readers_agree_and_degenerate_scenes_load(tmp_path, scene, subsample):
    frags, poses = scene
    write_scene(tmp_path / 'a', 's', frags, poses, how='info')
    write_scene(tmp_path / 'b', 's', frags, poses, how='npy')
    ids_a, pts_a, poses_a = pp.read_scene(str(tmp_path / 'a'), 's')
    ids_b, pts_b, poses_b = pp.read_scene(str(tmp_path / 'b'), 's')
    assert ids_a == ids_b == ['s/cloud_bin_%d' % i for i in range(6)]
    assert np.array_equal(poses_a, poses_b) and np.array_equal(poses_a, poses)
    assert all(np.array_equal(a, b) and np.array_equal(a, f.astype(np.float64)) for a, b, f in zip(pts_a, pts_b, frags))
    # one fragment: no pair; two fragments far apart: no surviving pair.  Both give valid pickles without a pair.
    write_scene(tmp_path / 'c', 'one', frags[:1], poses[:1])
    far = poses[:2].copy()
    far[1, :3, 3] += 50.0
    write_scene(tmp_path / 'c', 'far', frags[:2], far)
    pp.build_pickles(str(tmp_path / 'c'), 'val', ['one', 'far'], VOXEL, device='cpu', subsample=subsample)
    ds = tdm.ThreeDMatchDataset(str(tmp_path / 'c'), 'val', downsample=VOXEL)
    assert len(ds) == 0 and len(ds.points) == 3 and ds.correspondences == {}
    with pytest.warns(UserWarning, match="more than"):              # fragments the dataset will skip are counted
        big = np.random.default_rng(0).random((tdm.ThreeDMatchDataset.MAX_POINTS + 1, 3)).astype(np.float32) * 40
        write_scene(tmp_path / 'd', 'big', [big], poses[:1])
        pp.build_pickles(str(tmp_path / 'd'), 'train', ['big'], None, downsample=VOXEL, device='cpu')
