"""GPU: the raw moments of fragment pairs (ops.pair_information, the kInfo kind of csrc/icp.hip's search kernel) against
their NumPy restatement (registration.information_numpy); the edges of the launch geometry, batch independence,
determinism, graph capture; information_matrices, refine_transforms(return_information=True) and build_benchmark on the
device against their CPU paths; and register_scene scored against files that build_benchmark wrote."""
import os

import numpy as np
import pytest
import torch

from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.geometric_registration import evaluate as ev
from d3feat_pytorch_amd.geometric_registration import registration as reg
import icp_scene as sc

R = 0.075
SHIFT = (300.0, -200.0, 50.0)
PERTURBATIONS = ((2, 0.03), (4, 0.05), (6, 0.08))


def six_pairs(seed=4):
    """4 fragments of one room -> the 6 pairs (moving j, fixed i), i < j, each with its ground truth (maps j into i)
    perturbed by 2 deg / 0.03, 4 deg / 0.05 or 6 deg / 0.08 about random axes."""
    clouds, poses = sc.make_scene(seed, 4)
    rng = np.random.default_rng(seed + 1000)
    pairs, T0 = [], []
    for i in range(4):
        for j in range(i + 1, 4):
            pairs.append((j, i))
            T0.append(sc.gt_transform(poses, i, j) @ sc.perturbation(rng, *PERTURBATIONS[len(pairs) % 3]))
    return clouds, np.asarray(pairs), np.stack(T0)


def five_fragments():
    """5 fragments whose view centres are 1.4 apart: overlaps from 0.03 to 1.0, fragments of 239 to 7857 points."""
    return sc.make_scene(4, 5, spacing=1.4)


def device_grid(clouds, radius=R):
    pts = torch.from_numpy(np.concatenate(clouds)).cuda()
    return ops.CloudGrid(pts, [len(c) for c in clouds], radius)


@pytest.fixture(scope="module")
def scene():
    return six_pairs()


@pytest.fixture(scope="module")
def gpu_run(scene):
    clouds, pairs, T0 = scene
    grid = device_grid(clouds)
    outs = ops.pair_information(grid, None, pairs, T0, R)
    torch.cuda.synchronize()
    return grid, outs


@pytest.fixture(scope="module")
def benchmark_pair(tmp_path_factory):
    """build_benchmark of the 5-fragment scene on the device and on the NumPy path, once."""
    clouds, poses = five_fragments()
    root = tmp_path_factory.mktemp('benchmark')
    dev = reg.build_benchmark(clouds, poses, str(root / 'device'), None, radius=R)
    cpu = reg.build_benchmark(clouds, poses, str(root / 'cpu'), None, radius=R, device='cpu')
    return clouds, poses, root, dev, cpu


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [(0.0, 0.0, 0.0), SHIFT], ids=["as-generated", "shifted"])
def test_moments_match_information_numpy(scene, shift):
    """count equal (the search is bit-stated); every moment within 1e-11 of the pair's largest moment: about 2^13 exact
    products per sum, added in f64 in two different orders -- 2^15 terms x 2^-53 x a small constant."""
    clouds, pairs, T0 = scene
    clouds = sc.shift_clouds(clouds, shift)
    T0 = np.stack([sc.shift_pose(T, shift) for T in T0])
    moments, count, status = (t.cpu().numpy() for t in ops.pair_information(device_grid(clouds), None, pairs, T0, R))
    want, cn = reg.information_numpy(clouds, pairs, T0, R)
    assert moments.shape == (6, 20) and moments.dtype == np.float64
    assert np.array_equal(count, cn) and np.array_equal(moments[:, 0], cn.astype(np.float64)) and (status == 0).all()
    assert (cn > 1000).all()
    for p in range(6):
        err = np.abs(moments[p] - want[p]).max() / np.abs(want[p]).max()
        print("pair %d: n = %d, largest moment %.3e, rel. diff %.2e" % (p, cn[p], np.abs(want[p]).max(), err))
        assert err <= 1e-11


@pytest.mark.gpu
def test_edges_of_the_launch_geometry_in_one_call(scene):
    clouds, pairs, T0 = scene
    base = clouds[0]
    far = (base.astype(np.float64) + 50.0).astype(np.float32)
    stack = [base, base[:37].copy(), base[100:612].copy(), base[:513].copy(), far]
    assert [len(c) for c in stack[1:4]] == [37, 512, 513]
    grid = device_grid(stack)
    eye = np.eye(4)
    #           < one slice  one block  block + 1  self   50 m away  no such cloud  NaN pose
    dev_pairs = [(1, 0), (2, 0), (3, 0), (0, 0), (4, 0), (9, 0), (1, 0)]
    T = np.stack([eye] * 7)
    T[6, 1, 2] = np.nan
    rows = sum(len(stack[a]) if a < 5 else 0 for a, _ in dev_pairs) + len(base)
    moments, count, status = ops.pair_information(
        grid, None, torch.tensor(dev_pairs, dtype=torch.int32, device='cuda'), T, R, rows=rows)
    assert status.tolist() == [0, 0, 0, 0, 0, ops.ICP_ST_PAIR, ops.ICP_ST_NONFINITE]
    assert count.tolist() == [37, 512, 513, len(base), 0, 0, 0]
    m = moments.cpu().numpy()
    assert (m[4:] == 0).all()                                  # no accepted row / flagged: zero moments
    assert (m[:4, 19] == 0).all()                              # every point matched itself: sum d2 == 0
    assert np.array_equal(m[:4, 1:10], m[:4, 10:19])           # x moments == y moments, bit for bit
    want, cn = reg.information_numpy(stack, dev_pairs[:5], T[:5], R)
    assert np.array_equal(cn, count.cpu().numpy()[:5])
    for p in range(4):
        assert np.abs(m[p] - want[p]).max() <= 1e-11 * np.abs(want[p]).max(), p
    # the same five good pairs from the host give the same bits
    host = ops.pair_information(grid, None, dev_pairs[:5], T[:5], R)
    assert torch.equal(host[0], moments[:5]) and torch.equal(host[1], count[:5])


@pytest.mark.gpu
def test_a_pair_of_more_than_64_blocks(scene):
    """One pair of 64 * 512 + 1 moving rows: 65 block sums, so lane 0 of the wave that adds them (pair_sums in
    csrc/icp.hip, shared by the fit kernels and the information kernel) takes a second trip -- no other test has a
    fragment beyond 16 blocks.  The moving cloud repeats points of the fixed one under the identity: every row matches
    its own point at d2 == 0.  Moments within 1e-11 of the pair's largest against information_numpy (2^15 exact
    products per sum, added in f64 in two different orders); both fit kinds reduce the same count and sum of d2."""
    base = scene[0][0]
    moving = np.tile(base[:4097], (8, 1))[:32769]
    assert len(base) >= 4097 and len(moving) == 64 * ops.ICP_BLOCK_ROWS + 1
    stack, pairs, T = [moving, base], [(0, 1)], np.eye(4)[None]
    grid = device_grid(stack, 2 * R)
    moments, count, status = ops.pair_information(grid, None, pairs, T, R)
    m = moments.cpu().numpy()[0]
    assert count.tolist() == [32769] and status.tolist() == [0]
    assert m[19] == 0 and np.array_equal(m[1:10], m[10:19])
    want, cn = reg.information_numpy(stack, pairs, T, R)
    err = np.abs(m - want[0]).max() / np.abs(want[0]).max()
    print("n = %d, largest moment %.3e, rel. diff %.2e" % (cn[0], np.abs(want[0]).max(), err))
    assert cn.tolist() == [32769] and err <= 1e-11
    normals = ops.estimate_normals(grid, None, 2 * R)[0]
    for kw in ({}, {'normals': normals}):
        icp = ops.icp_rigid(grid, None, pairs, T, R, max_iters=0, return_trace=True, **kw)
        assert torch.equal(icp[1], count) and icp[4].tolist() == [0]
        assert torch.equal(icp[5][:, 0, 0], moments[:, 0]) and torch.equal(icp[5][:, 0, 1], moments[:, 19])


@pytest.mark.gpu
def test_batch_independent_and_deterministic(scene, gpu_run):
    clouds, pairs, T0 = scene
    grid, outs = gpu_run
    again = ops.pair_information(grid, None, pairs, T0, R)
    assert all(torch.equal(x, y) for x, y in zip(outs, again))
    back = ops.pair_information(grid, None, pairs[::-1].copy(), T0[::-1].copy(), R)
    assert all(torch.equal(x, y.flip(0)) for x, y in zip(outs, back))
    for p in range(len(pairs)):
        one = ops.pair_information(grid, None, pairs[p:p + 1], T0[p:p + 1], R)
        for x, y in zip(outs, one):
            assert torch.equal(x[p:p + 1], y), p
    # the search is icp_rigid's iteration 0
    icp = ops.icp_rigid(grid, None, pairs, T0, R, max_iters=0, return_trace=True)
    assert torch.equal(icp[1], outs[1]) and torch.equal(icp[5][:, 0, 1], outs[0][:, 19])


@pytest.mark.gpu
def test_graph_capture_replays_bit_identically(scene):
    clouds, pairs, T0 = scene
    grid = device_grid(clouds)
    dev_pairs = torch.from_numpy(pairs.astype(np.int32)).cuda()
    rows = int(sum(len(clouds[a]) for a, _ in pairs))
    Ti = torch.from_numpy(T0).cuda()
    ops.pair_information(grid, None, dev_pairs, Ti, R, rows=rows)            # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = ops.pair_information(grid, None, dev_pairs, Ti, R, rows=rows)
    rng = np.random.default_rng(77)
    Ti.copy_(torch.from_numpy(np.stack([T @ sc.perturbation(rng, 1, 0.01) for T in T0])).cuda())
    g.replay()
    torch.cuda.synchronize()
    want = ops.pair_information(grid, None, dev_pairs, Ti, R, rows=rows)
    assert all(torch.equal(x, y) for x, y in zip(outs, want))
    assert (want[2] == 0).all() and (want[1] > 1000).all()
    first = ops.pair_information(grid, None, dev_pairs, torch.from_numpy(T0).cuda(), R, rows=rows)
    assert not torch.equal(first[0], want[0])                                # the replay read the new poses


@pytest.mark.gpu
def test_argument_errors(scene):
    clouds, pairs, T0 = scene
    grid = device_grid(clouds, 0.05)
    with pytest.raises(RuntimeError):
        ops.pair_information(grid, None, pairs, T0, 0.075)           # above the cell list's radius
    with pytest.raises(ValueError):
        ops.pair_information(grid, None, pairs, T0[:, :2], 0.05)
    with pytest.raises(ValueError):
        ops.pair_information(grid, None, pairs, T0[:3], 0.05)
    with pytest.raises(ValueError):
        ops.pair_information(grid, None, [(0, 7)], T0[:1], 0.05)
    with pytest.raises(ValueError):
        ops.pair_information(torch.from_numpy(np.concatenate(clouds)).cuda(), None, pairs, T0, 0.05)
    a = ops.pair_information(grid, None, pairs[:2], T0[:2], 0.05)
    b = ops.pair_information(torch.from_numpy(np.concatenate(clouds)).cuda(), [len(c) for c in clouds], pairs[:2],
                             T0[:2, :3], 0.05)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert ops.pair_information_bytes(1024) == ops.icp_rigid_bytes(1024) + 2 * 2 * 24


@pytest.mark.gpu
def test_information_matrices_device_equals_cpu_path(scene):
    clouds, pairs, T0 = scene
    keys = ['%d_%d' % (i, j) for j, i in pairs]
    for frame, order in (('moving', 'translation_first'), ('fixed', 'rotation_first')):
        info, count, rmse = reg.information_matrices(clouds, keys, T0, R, frame=frame, order=order)
        want, cn, rn = reg.information_matrices(clouds, keys, T0, R, device='cpu', frame=frame, order=order)
        assert info.is_cuda and tuple(info.shape) == (6, 6, 6)
        assert np.array_equal(count.cpu().numpy(), cn)
        assert np.abs(rmse.cpu().numpy() - rn).max() <= 1e-12
        for p in range(6):
            assert np.abs(info[p].cpu().numpy() - want[p]).max() <= 1e-11 * np.abs(want[p]).max(), p


@pytest.mark.gpu
def test_refine_transforms_return_information_leaves_the_rest_alone(scene):
    clouds, pairs, T0 = scene
    keys = ['%d_%d' % (i, j) for j, i in pairs[:3]]
    plain = reg.refine_transforms(clouds, keys, T0[:3], R, max_iters=6)
    more = reg.refine_transforms(clouds, keys, T0[:3], R, max_iters=6, return_information=True)
    assert len(plain) == 4 and len(more) == 5
    assert all(torch.equal(x, y) for x, y in zip(plain, more))
    want = reg.information_matrices(clouds, keys, plain[0], R)[0]
    assert torch.equal(more[4], want)
    cpu = reg.refine_transforms(clouds[:2], ['0_1'], T0[:1], R, device='cpu', max_iters=2, return_information=True)
    assert cpu[4].shape == (1, 6, 6) and cpu[4][0, 0, 0] == round(cpu[1][0] * len(clouds[1]))


@pytest.mark.gpu
def test_build_benchmark_device_equals_cpu_path(benchmark_pair):
    """Same keys, identical gt.log text, parsed gt.info within 1e-8 of the block's largest entry (moments that differ in
    the twelfth digit can straddle one rounding boundary of the nine printed digits); three chunks write the same bytes
    as one."""
    clouds, poses, root, (gt, info, overlap), (gt_c, info_c, overlap_c) = benchmark_pair
    assert sorted(gt) == sorted(gt_c) == sorted(info) and 0 < len(gt) < 10
    assert overlap == overlap_c                                              # counts are equal, so the shares are
    read = lambda d, name: open(os.path.join(str(root / d), name)).read()
    assert read('device', 'gt.log') == read('cpu', 'gt.log')
    got, want = reg.loadinfo(str(root / 'device')), reg.loadinfo(str(root / 'cpu'))
    for key in gt:
        assert np.abs(got[key] - want[key]).max() <= 1e-8 * np.abs(want[key]).max(), key
        assert np.abs(info[key] - info_c[key]).max() <= 1e-11 * np.abs(info_c[key]).max(), key
    calls, real = [], ops.pair_information

    def spy(*args, **kw):
        calls.append(len(args[2]))
        return real(*args, **kw)
    # 25423 moving rows in 9 candidates, sorted by their fixed fragment: 7375 | 5616 + 2033 | the other six (10399)
    ops.pair_information = spy
    try:
        reg.build_benchmark(clouds, poses, str(root / 'chunked'), None, radius=R, max_rows=10500)
    finally:
        ops.pair_information = real
    print("pairs per call:", calls)
    assert len(calls) == 3 and sum(calls) == len(overlap)
    assert read('chunked', 'gt.log') == read('device', 'gt.log')
    assert read('chunked', 'gt.info') == read('device', 'gt.info')


@pytest.mark.gpu
def test_register_scene_scores_against_the_built_files(benchmark_pair, tmp_path):
    """register_scene consumes the gt.log / gt.info that build_benchmark wrote.  The recall is printed, not asserted:
    nobody has measured what these synthetic descriptors reach on this scene."""
    clouds, poses, root, (gt, info, overlap), _ = benchmark_pair
    num_frag, scene_name, save = 5, 'surface-room', str(tmp_path / 'dump')
    _, _, world, ids = sc.make_scene(4, 5, spacing=1.4, return_world=True)
    rng = np.random.default_rng(9)
    desc = sc.position_descriptors(rng, world, ids)
    score = [rng.permutation(len(c)).astype(np.float32)[:, None] / len(c) for c in clouds]
    dpath, kpath, spath = ev._paths(save, scene_name)
    for p in (dpath, kpath, spath):
        os.makedirs(p)
    for f in range(num_frag):
        np.save(os.path.join(dpath, 'cloud_bin_%d.D3Feat' % f), desc[f])
        np.save(os.path.join(kpath, 'cloud_bin_%d' % f), clouds[f])
        np.save(os.path.join(spath, 'cloud_bin_%d' % f), score[f])
    out = reg.register_scene(save, scene_name, str(root / 'device'), num_points=1000, num_hypotheses=20000,
                             distance_threshold=0.05, seed=0, icp=dict(max_distance=0.05))
    assert out is not None and len(out) == 3
    recall, precision, errs = out
    far = sorted(k for k in ev.loadlog(str(root / 'device')) if reg._far(k))
    assert far and sorted(errs) == far
    print("recall %.3f, precision %.3f over %d far pairs; errors %s" % (
        recall, precision, len(far), {k: float('%.3g' % v) for k, v in errs.items()}))
    assert 0.0 <= recall <= 1.0 and 0.0 <= precision <= 1.0
