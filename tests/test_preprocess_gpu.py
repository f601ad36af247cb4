"""GPU: ``ops.nearest_pairs`` (d3f_nearest_pairs) and the device path of datasets/preprocess.py against the package's NumPy
restatement of the same contract -- exact equality of every index and count."""
import pickle
import random

import numpy as np
import pytest
import torch

from d3feat_pytorch_amd import config as cfgmod, ops
from d3feat_pytorch_amd.datasets import ThreeDMatch as tdm
from d3feat_pytorch_amd.datasets import preprocess as pp
from preprocess_scene import make_scene, pose, write_scene

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VOXEL = 0.03
RADIUS = 1.25 * VOXEL
ST_CELL_RANGE = 2


def _stack(clouds):
    pts = np.concatenate(clouds, 0) if sum(len(c) for c in clouds) else np.zeros((0, 3), np.float32)
    return torch.as_tensor(pts).to(DEV), np.array([len(c) for c in clouds], dtype=np.int32)


def _device(clouds, pairs, T, radius, lanes=0, grid=None):
    if grid is None:
        pts, lens = _stack(clouds)
        grid = ops.CloudGrid(pts, lens, radius)
    nn, count, row_start = ops.nearest_pairs(grid, None, pairs, T, radius, lanes=lanes)
    grid.status.raise_if_set()
    return nn.cpu().numpy(), count.cpu().numpy(), row_start.cpu().numpy()


def _same(got, want):
    for g, w, name in zip(got, want, ("nn", "count", "row_start")):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g, w), "%s differs in %d places" % (name, int((g != w).sum()))


@pytest.fixture(scope="module")
def scene12():
    frags, poses = make_scene(12, n_raw=90000, window=0.5, stride=0.06)
    return pp.subsample_fragments(frags, VOXEL, None, DEV), poses


def test_all_pairs_of_a_scene_equal_numpy(scene12):
    clouds, poses = scene12
    pairs = [(i, j) for i in range(12) for j in range(i + 1, 12)]
    assert len(pairs) == 66
    T = np.stack([np.linalg.inv(poses[j]) @ poses[i] for i, j in pairs])
    want = pp.nearest_pairs_numpy(clouds, pairs, T, RADIUS)
    share = want[1] / np.array([len(clouds[i]) for i, _ in pairs])
    assert share.max() > 0.8 and share.min() < 0.2                  # from nearly whole to nearly nothing
    pts, lens = _stack(clouds)
    grid = ops.CloudGrid(pts, lens, RADIUS)
    for lanes in (0, 4, 8, 16, 32):                                 # the result does not depend on the launch geometry
        _same(_device(clouds, pairs, T, RADIUS, lanes=lanes, grid=grid), want)
    # a long list (the 66 pairs nine times over): workgroups then serve several slices of rows and follow the pairs
    many = ops.nearest_pairs(grid, None, pairs * 9, np.concatenate([T] * 9), RADIUS)
    assert np.array_equal(many[0].cpu().numpy(), np.tile(want[0], 9))
    assert np.array_equal(many[1].cpu().numpy(), np.tile(want[1], 9))
    # [P,3,4] transforms and device pair tensors are the same call
    nn, count, _ = ops.nearest_pairs(grid, None, torch.as_tensor(pairs, device=DEV), T[:, :3, :], RADIUS)
    assert np.array_equal(nn.cpu().numpy(), want[0]) and np.array_equal(count.cpu().numpy(), want[1])


def test_ties_duplicates_and_the_strict_radius():
    """Integer-lattice targets with every point stored twice in shuffled order: many d2 are equal, the lowest index must
    win; queries at exactly the radius from their only candidate are rejected."""
    rng = np.random.default_rng(5)
    g = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing='ij'), -1).reshape(-1, 3)
    lattice = np.concatenate([g, g], 0).astype(np.float32)
    lattice = lattice[rng.permutation(len(lattice))]
    mids = np.concatenate([g + (0.5, 0, 0), g + (0.5, 0.5, 0), g + (0.5, 0.5, 0.5), g + (0.25, 0, 0), g],
                          0).astype(np.float32)
    lonely = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0]], dtype=np.float32)
    at_radius = np.array([[1, 0, 0], [9, 0, 0], [0, 11, 0], [0, 0, -1], [0.99999994, 0, 0], [1.0000001, 0, 0],
                          [0.6, 0.8, 0]], dtype=np.float32)
    clouds = [lattice, mids, lonely, at_radius]
    quarter = np.eye(4)
    quarter[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]            # exact in every format
    quarter[:3, 3] = [5, 0, 0]
    shift = np.eye(4)
    shift[:3, 3] = [1, -2, 3]
    pairs = [(1, 0), (1, 0), (1, 0), (3, 2), (0, 0)]
    T = np.stack([np.eye(4), quarter, shift, np.eye(4), np.eye(4)])
    want = pp.nearest_pairs_numpy(clouds, pairs, T, 1.0)
    for lanes in (0, 4, 16, 32):
        _same(_device(clouds, pairs, T, 1.0, lanes=lanes), want)
    nn, count, row_start = want
    # the expectation itself, independently: f64 brute force is exact on a lattice
    q = mids.astype(np.float64)
    d2 = ((q[:, None, :] - lattice.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    best = d2.min(1)
    first = np.array([np.nonzero(row == b)[0][0] for row, b in zip(d2, best)])
    assert np.array_equal(nn[:len(mids)], np.where(best < 1.0, first, -1))
    assert (d2 == best[:, None]).sum(1).max() >= 16                 # up to 8 lattice points, each stored twice
    # exactly at the radius: rejected; one ulp inside: accepted; (0.6, 0.8) has d2 >= 1 in f32: rejected too
    seg = nn[row_start[3]:row_start[4]]
    assert seg.tolist() == [-1, -1, -1, -1, 0, -1, -1] and count[3] == 1
    # a duplicated point looking for itself finds the lower of its two indices
    seg = nn[row_start[4]:row_start[5]]
    lower = np.array([np.nonzero((lattice == p).all(1))[0][0] for p in lattice])
    assert np.array_equal(seg, lower) and count[4] == len(lattice)


def test_edge_cases(scene12):
    clouds, poses = scene12
    rng = np.random.default_rng(9)
    a, b = clouds[0], clouds[1]
    one = a[:1].copy()
    # no pairs at all
    pts, lens = _stack([a, b, one])
    grid = ops.CloudGrid(pts, lens, RADIUS)
    nn, count, row_start = ops.nearest_pairs(grid, None, np.zeros((0, 2), np.int64), np.zeros((0, 4, 4)), RADIUS)
    assert nn.shape == (0,) and count.shape == (0,) and row_start.tolist() == [0]
    # no match / one-point cloud as source and as target / a cloud against itself under the identity
    away = np.eye(4)
    away[:3, 3] = [30.0, 0, 0]
    pairs = [(0, 1), (2, 0), (0, 2), (0, 0), (2, 2)]
    T = np.stack([away, np.eye(4), np.eye(4), np.eye(4), np.eye(4)])
    got = _device(None, pairs, T, RADIUS, grid=grid)
    _same(got, pp.nearest_pairs_numpy([a, b, one], pairs, T, RADIUS))
    nn, count, row_start = got
    assert count.tolist() == [0, 1, int((nn[row_start[2]:row_start[3]] == 0).sum()), len(a), 1]
    assert (nn[:len(a)] == -1).all() and count[2] >= 1
    assert np.array_equal(nn[row_start[3]:row_start[4]], np.arange(len(a)))
    # queries sent out of the addressable cells: the status says so and the rows are -1, never a wrong index
    out = np.eye(4)
    out[:3, 3] = [1.0e6, 0, 0]
    nn, count, _ = ops.nearest_pairs(grid, None, [(0, 0), (0, 0)], np.stack([out, np.eye(4)]), RADIUS)
    assert int(grid.status.word.item()) & ST_CELL_RANGE
    with pytest.raises(RuntimeError, match="outside the addressable cell grid"):
        grid.status.raise_if_set()
    assert (nn[:len(a)] == -1).all().item() and count.tolist() == [0, len(a)]
    assert np.array_equal(nn[len(a):].cpu().numpy(), np.arange(len(a)))
    grid.status.word.zero_()
    with pytest.raises(ValueError):
        ops.nearest_pairs(grid, None, [(0, 3)], np.eye(4)[None], RADIUS)
    with pytest.raises(RuntimeError, match="exceeds"):
        ops.nearest_pairs(grid, None, [(0, 1)], np.eye(4)[None], 2 * RADIUS)
    # a smaller radius on a shared cell list built by the radius search's own build
    T01 = (np.linalg.inv(poses[1]) @ poses[0])[None]
    rg = ops.RadiusGrid(pts, lens, 2.0 * RADIUS)
    for r in (2.0 * RADIUS, RADIUS, 0.4 * RADIUS):
        _same(_device(None, [(0, 1)], T01, r, grid=rg), pp.nearest_pairs_numpy([a, b, one], [(0, 1)], T01, r))
    # 200 small clouds in one cell list
    small = [(rng.random((int(n), 3)) * 0.3).astype(np.float32) for n in rng.integers(1, 150, size=200)]
    pairs = np.stack([rng.integers(0, 200, size=400), rng.integers(0, 200, size=400)], 1)
    T = np.stack([pose(rng.normal() * 0.2, rng.normal(size=3) * 0.03) for _ in range(400)])
    want = pp.nearest_pairs_numpy(small, pairs, T, RADIUS)
    assert 0.2 < (want[0] >= 0).mean() < 0.98
    _same(_device(small, pairs, T, RADIUS), want)
    with pytest.raises(RuntimeError):                               # the radius search's own build stops at 64 clouds
        ops.RadiusGrid(*_stack(small), RADIUS)


def test_device_pair_that_names_no_cloud(scene12):
    """Device pairs are not read on the host: a pair that names a cloud that is not there gets -1 rows (those of the
    clamped source cloud) and count 0 -- the kernel's own answer -- while its neighbours in the list are what the same
    pairs give from the host, and the grid's status word stays clear."""
    clouds, poses = scene12
    a, b, one = clouds[0], clouds[1], clouds[0][:1].copy()
    grid = ops.CloudGrid(*_stack([a, b, one]), RADIUS)
    T01 = np.linalg.inv(poses[1]) @ poses[0]
    T = np.stack([T01, np.eye(4), np.linalg.inv(T01)])
    pairs = torch.tensor([[0, 1], [9, 0], [1, 0]], dtype=torch.int32, device=DEV)
    nn, count, row_start = (t.cpu().numpy() for t in ops.nearest_pairs(grid, None, pairs, T, RADIUS))
    want_nn, want_count, want_start = _device(None, [(0, 1), (1, 0)], T[[0, 2]], RADIUS, grid=grid)
    assert row_start.tolist() == [0, len(a), len(a) + 1, len(a) + 1 + len(b)] and want_start[1] == len(a)
    assert np.array_equal(nn[:len(a)], want_nn[:len(a)]) and np.array_equal(nn[len(a) + 1:], want_nn[len(a):])
    assert count.tolist() == [want_count[0], 0, want_count[1]] and want_count.min() > 0
    assert nn[len(a)] == -1
    assert int(grid.status.word.item()) == 0


def _equal_dicts(x, y):
    return list(x) == list(y) and all(np.array_equal(x[k], y[k]) and x[k].dtype == y[k].dtype for k in x)


def test_chunking_and_determinism(scene12):
    clouds, poses = scene12
    runs = [pp.mine_scene(clouds, poses, None, radius=RADIUS, device=DEV, max_rows=m)[1]
            for m in (1, 20000, pp.DEFAULT_MAX_ROWS, pp.DEFAULT_MAX_ROWS)]
    assert len(runs[0]) > 10
    for r in runs[1:]:
        assert _equal_dicts(runs[0], r)
    cpu = pp.mine_scene(clouds, poses, None, radius=RADIUS, device='cpu')[1]
    assert _equal_dicts(runs[0], cpu)
    sym = [pp.mine_scene(clouds, poses, None, radius=RADIUS, min_overlap=0.5, symmetric=True, device=d, max_rows=m,
                         return_overlap=True)[1:] for d, m in ((DEV, 1), (DEV, pp.DEFAULT_MAX_ROWS), ('cpu', 1))]
    assert _equal_dicts(sym[0][0], sym[1][0]) and _equal_dicts(sym[0][0], sym[2][0])
    assert sym[0][1] == sym[1][1] == sym[2][1]                      # the overlap ratios, pair by pair
    # the device subsampler of the scene form: batched over the fragments == one fragment at a time
    frags, _ = make_scene(3, n_raw=30000)
    batched = pp.subsample_fragments(frags, VOXEL, None, DEV)
    assert all(np.array_equal(b, tdm._device_subsample(f, VOXEL)) for b, f in zip(batched, frags))


def test_pickles_equal_the_cpu_path_and_train(tmp_path):
    from d3feat_pytorch_amd.train import TrainStep
    frags, poses = make_scene(6, n_raw=120000, scale=0.5, window=0.7, stride=0.18)
    clouds = pp.subsample_fragments(frags, VOXEL, None, DEV)
    write_scene(tmp_path, 'synth-a', clouds, poses)                 # both sides read the same subsampled clouds
    files = {}
    for name, device in (('gpu', DEV), ('cpu', 'cpu')):
        files[name] = pp.build_pickles(str(tmp_path), 'train', ['synth-a'], None, out_dir=str(tmp_path / name),
                                       downsample=VOXEL, device=device)
    loaded = {name: [pickle.load(open(f, 'rb')) for f in fs] for name, fs in files.items()}
    assert _equal_dicts(loaded['gpu'][0], loaded['cpu'][0]) and _equal_dicts(loaded['gpu'][1], loaded['cpu'][1])
    assert len(loaded['gpu'][1]) >= 5
    cfg = cfgmod.default_config(first_features_dim=16, num_node=64)
    ds = tdm.ThreeDMatchDataset(str(tmp_path / 'gpu'), 'train', num_node=cfg.num_node, downsample=VOXEL)
    random.seed(0)
    np.random.seed(0)
    item = ds[0]
    ts = TrainStep(cfg, [30] * 5, torch.device(DEV), seed=0)
    loss = ts.step(item)[0]
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss).all())
