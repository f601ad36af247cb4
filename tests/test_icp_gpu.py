"""GPU: batched ICP (ops.icp_rigid, csrc/icp.hip) against its NumPy restatement (registration.icp_numpy) on a surface
scene; batch independence, determinism, graph capture, and the refinement step of register_scene."""
import os

import numpy as np
import pytest
import torch

from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.datasets.preprocess import nearest_pairs_numpy, nearest_within, transform_points
from d3feat_pytorch_amd.geometric_registration import evaluate as ev
from d3feat_pytorch_amd.geometric_registration import registration as reg
import icp_scene as sc
from test_icp_cpu import svd_fit

R = 0.075
SHIFT = (300.0, -200.0, 50.0)
PERTURBATIONS = ((2, 0.03), (4, 0.05), (6, 0.08))


def six_pairs(seed=4):
    """4 fragments of one room -> the 6 pairs (moving j, fixed i), i < j, of different lengths, each with its ground
    truth (maps j into i) perturbed by 2 deg / 0.03, 4 deg / 0.05 or 6 deg / 0.08 about random axes."""
    clouds, poses = sc.make_scene(seed, 4)
    rng = np.random.default_rng(seed + 1000)
    pairs, G, T0 = [], [], []
    for i in range(4):
        for j in range(i + 1, 4):
            pairs.append((j, i))
            G.append(sc.gt_transform(poses, i, j))
            T0.append(G[-1] @ sc.perturbation(rng, *PERTURBATIONS[len(pairs) % 3]))
    return clouds, np.asarray(pairs), np.stack(G), np.stack(T0)


def device_grid(clouds, radius=R):
    pts = torch.from_numpy(np.concatenate(clouds)).cuda()
    return ops.CloudGrid(pts, [len(c) for c in clouds], radius)


def to_numpy(outs):
    return tuple(o.cpu().numpy() for o in outs)


@pytest.fixture(scope="module")
def scene():
    return six_pairs()


@pytest.fixture(scope="module")
def gpu_run(scene):
    clouds, pairs, G, T0 = scene
    grid = device_grid(clouds)
    outs = ops.icp_rigid(grid, None, pairs, T0, R)
    torch.cuda.synchronize()
    return grid, outs


@pytest.mark.gpu
def test_one_search_is_exact_and_one_fit_matches_numpy(scene):
    clouds, pairs, G, T0 = scene
    grid = device_grid(clouds)
    T, count, rmse, iters, status, trace = to_numpy(ops.icp_rigid(grid, None, pairs, T0, R, max_iters=0,
                                                                  return_trace=True))
    nn, want, row_start = nearest_pairs_numpy(clouds, pairs, T0, R)
    assert trace.shape == (6, 1, 2)
    assert np.array_equal(trace[:, 0, 0], want.astype(np.float64))           # bit-stated search: equality
    assert np.array_equal(count, want) and (iters == 0).all() and (status == 0).all()
    assert np.array_equal(T[:, :3], T0[:, :3]) and (T[:, 3] == [0, 0, 0, 1]).all()
    T1, count1, _, iters1, status1, trace1 = to_numpy(ops.icp_rigid(grid, None, pairs, T0, R, max_iters=1,
                                                                    return_trace=True))
    assert np.array_equal(trace1[:, 0], trace[:, 0]) and (iters1 == 1).all() and (status1 == 0).all()
    for p, (a, b) in enumerate(pairs):
        res = nn[row_start[p]:row_start[p + 1]]
        sel = res >= 0
        q, ym = transform_points(clouds[a], T0[p])[sel], clouds[b][res[sel]]
        d = q - ym
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]       # f32, the kernel's values
        sd2 = d2.astype(np.float64).sum()
        rel = abs(trace[p, 0, 1] - sd2) / sd2
        fit = np.abs(T1[p] - svd_fit(clouds[a][sel], ym)).max()
        print("pair %d: n0 = %d, sum d2 rel. diff %.2e, |T_1 - T_numpy| = %.2e" % (p, want[p], rel, fit))
        assert rel < 1e-12
        assert abs(rmse[p] - np.sqrt(sd2 / want[p])) < 1e-12
        assert fit < 1e-9


def band_rows(x, y, T, radius, origin):
    """Rows of x whose nearest point of y under T lies within rounding reach of the radius:
    |d2 - r^2| < 1e-6 (1 + |q - origin|^2)."""
    q = transform_points(x, T)
    nn = nearest_within(q, y, radius * 1.05)
    sel = nn >= 0
    d2 = ((q[sel].astype(np.float64) - y[nn[sel]].astype(np.float64)) ** 2).sum(1)
    q2 = ((q[sel].astype(np.float64) - np.asarray(origin)) ** 2).sum(1)
    r2 = float(np.float32(radius) * np.float32(radius))
    return int((np.abs(d2 - r2) < 1e-6 * (1.0 + q2)).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [(0.0, 0.0, 0.0), SHIFT], ids=["as-generated", "shifted"])
def test_full_run_matches_icp_numpy(scene, shift):
    """6 pairs of different lengths in one call against the NumPy restatement: iterations and status equal, T within
    1e-6, count equal -- except by at most the number of the pair's rows that lie within rounding reach of the radius
    under the oracle's final T, and those are at most 0.1 % of the pair's rows.  The reach is measured about the scene's
    own origin (1e-6 (1 + |q - shift|^2)): about the coordinate origin it would exceed r^2 itself for the scene at
    (300, -200, 50) and allow everything."""
    clouds, pairs, G, T0 = scene
    clouds = sc.shift_clouds(clouds, shift)
    T0 = np.stack([sc.shift_pose(T, shift) for T in T0])
    grid = device_grid(clouds)
    T, count, rmse, iters, status = to_numpy(ops.icp_rigid(grid, None, pairs, T0, R))
    Tn, cn, rn, itn, stn = reg.icp_numpy(clouds, pairs, T0, R)
    print("iterations", iters, itn, "status", status, stn)
    exceptions = 0
    for p, (a, b) in enumerate(pairs):
        band = band_rows(clouds[a], clouds[b], Tn[p], R, shift)
        diff = abs(int(count[p]) - int(cn[p]))
        exceptions += diff != 0
        print("pair %d (%d rows): |T - T_numpy| = %.2e, count %d / %d, band rows %d, rmse diff %.2e" % (
            p, len(clouds[a]), np.abs(T[p] - Tn[p]).max(), count[p], cn[p], band, abs(rmse[p] - rn[p])))
        assert band <= 1e-3 * len(clouds[a])
        assert diff <= band
    print("count exceptions: %d" % exceptions)
    assert np.array_equal(iters, itn) and np.array_equal(status, stn)
    assert np.abs(T - Tn).max() < 1e-6


@pytest.mark.gpu
def test_every_pair_improves_and_reports_its_own_pose(scene, gpu_run):
    clouds, pairs, G, T0 = scene
    grid, outs = gpu_run
    T, count, rmse, iters, status = outs
    for p in range(len(pairs)):
        r0, t0 = sc.pose_error(T0[p], G[p])
        r1, t1 = sc.pose_error(T[p].cpu().numpy(), G[p])
        print("pair %d: %.2f deg / %.3f -> %.3f deg / %.4f after %d fits" % (p, r0, t0, r1, t1, int(iters[p])))
        assert r1 < r0 and t1 < t0
    fresh = ops.icp_rigid(grid, None, pairs, T, R, max_iters=0)
    assert torch.equal(fresh[0], T) and torch.equal(fresh[1], count) and torch.equal(fresh[2], rmse)
    assert (status == 0).all() and (iters >= 1).all()


@pytest.mark.gpu
def test_batch_independent_and_deterministic(scene, gpu_run):
    clouds, pairs, G, T0 = scene
    grid, outs = gpu_run
    again = ops.icp_rigid(grid, None, pairs, T0, R)
    assert all(torch.equal(x, y) for x, y in zip(outs, again))
    for p in range(len(pairs)):
        one = ops.icp_rigid(grid, None, pairs[p:p + 1], T0[p:p + 1], R)
        for x, y in zip(outs, one):
            assert torch.equal(x[p:p + 1], y), p
    # a pair of fragments that do not meet: FEW, untouched, and nobody else notices
    far = (clouds[0].astype(np.float64) + 50.0).astype(np.float32)
    grid5 = device_grid(list(clouds) + [far])
    pairs5 = np.concatenate([pairs[:3], [[4, 0]], pairs[3:]])
    T5 = np.concatenate([T0[:3], np.eye(4)[None], T0[3:]])
    got = ops.icp_rigid(grid5, None, pairs5, T5, R)
    keep = [0, 1, 2, 4, 5, 6]
    for x, y in zip(outs, got):
        assert torch.equal(x, y[keep])
    assert int(got[4][3]) == ops.ICP_ST_FEW and int(got[3][3]) == 0 and int(got[1][3]) == 0
    assert torch.equal(got[0][3].cpu(), torch.eye(4, dtype=torch.float64))


@pytest.mark.gpu
def test_bad_pairs_and_poses_are_flagged_on_the_device(scene):
    clouds, pairs, G, T0 = scene
    grid = device_grid(clouds)
    dev_pairs = torch.tensor([[1, 0], [9, 0], [2, 0]], dtype=torch.int32, device='cuda')
    Ti = torch.from_numpy(np.stack([T0[0], T0[0], T0[1]])).cuda()
    Ti[2, 1, 1] = float('inf')
    T, count, rmse, iters, status = ops.icp_rigid(grid, None, dev_pairs, Ti, R, rows=3 * max(len(c) for c in clouds))
    assert status.tolist() == [0, ops.ICP_ST_PAIR, ops.ICP_ST_NONFINITE]
    assert torch.equal(T[1], Ti[1]) and iters.tolist()[1:] == [0, 0] and count.tolist()[1:] == [0, 0]
    alone = ops.icp_rigid(grid, None, pairs[:1], T0[:1], R)
    assert torch.equal(T[0], alone[0][0]) and int(count[0]) == int(alone[1][0])


@pytest.mark.gpu
def test_graph_capture_replays_bit_identically(scene):
    clouds, pairs, G, T0 = scene
    grid = device_grid(clouds)
    dev_pairs = torch.from_numpy(pairs.astype(np.int32)).cuda()
    rows = int(sum(len(clouds[a]) for a, _ in pairs))
    Ti = torch.from_numpy(T0).cuda()
    kw = dict(max_iters=12, rows=rows)
    ops.icp_rigid(grid, None, dev_pairs, Ti, R, **kw)              # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = ops.icp_rigid(grid, None, dev_pairs, Ti, R, **kw)
    rng = np.random.default_rng(77)
    other = np.stack([Gp @ sc.perturbation(rng, 3, 0.04) for Gp in G])
    Ti.copy_(torch.from_numpy(other).cuda())
    g.replay()
    torch.cuda.synchronize()
    want = ops.icp_rigid(grid, None, dev_pairs, Ti, R, **kw)
    assert all(torch.equal(x, y) for x, y in zip(outs, want))
    assert (want[4] == 0).all() and (want[3] >= 1).all()


@pytest.mark.gpu
def test_argument_errors(scene):
    clouds, pairs, G, T0 = scene
    grid = device_grid(clouds, 0.05)
    with pytest.raises(RuntimeError):
        ops.icp_rigid(grid, None, pairs, T0, 0.075)                  # above the cell list's radius
    with pytest.raises(ValueError):
        ops.icp_rigid(grid, None, pairs, T0[:, :2], 0.05)
    with pytest.raises(ValueError):
        ops.icp_rigid(grid, None, pairs, T0[:3], 0.05)
    with pytest.raises(ValueError):
        ops.icp_rigid(grid, None, pairs, T0, 0.05, max_iters=-1)
    with pytest.raises(ValueError):
        ops.icp_rigid(grid, None, [(0, 7)], T0[:1], 0.05)
    with pytest.raises(ValueError):
        ops.icp_rigid(torch.from_numpy(np.concatenate(clouds)).cuda(), None, pairs, T0, 0.05)
    # stacked points instead of a grid, and [P,3,4] poses, are the same call
    a = ops.icp_rigid(grid, None, pairs[:2], T0[:2], 0.05, max_iters=3)
    b = ops.icp_rigid(torch.from_numpy(np.concatenate(clouds)).cuda(), [len(c) for c in clouds], pairs[:2],
                      T0[:2, :3], 0.05, max_iters=3)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
def test_refine_transforms_device_equals_cpu_path(scene):
    clouds, pairs, G, T0 = scene
    keys = ['%d_%d' % (i, j) for j, i in pairs[:2]]
    T, fitness, rmse, iters = reg.refine_transforms(clouds, keys, T0[:2], R, max_iters=8)
    Tn, fn, rn, itn = reg.refine_transforms(clouds, keys, T0[:2], R, device='cpu', max_iters=8)
    assert np.abs(T.cpu().numpy() - Tn).max() < 1e-6 and np.array_equal(iters.cpu().numpy(), itn)
    assert np.abs(fitness.cpu().numpy() - fn).max() < 1e-3


@pytest.mark.gpu
def test_register_scene_refines_every_pair_in_one_call(tmp_path, monkeypatch):
    """register_scene(icp=...) == refine_transforms applied to what register_scene(icp=None) estimates (same seed), to
    1e-12; recall not lower; median transformation_error over the far pairs lower.  The estimates are compared as
    register_scene hands them to evaluate.writelog: the log file itself keeps 9 digits, so the files are only checked
    to agree with those estimates to the file's precision."""
    num_frag, scene_name, save = 6, 'surface-room', str(tmp_path / 'dump')
    clouds, poses, world, ids = sc.make_scene(3, num_frag, return_world=True)
    rng = np.random.default_rng(9)
    desc = sc.position_descriptors(rng, world, ids)
    score = [rng.permutation(len(c)).astype(np.float32)[:, None] / len(c) for c in clouds]
    gt = {'%d_%d' % (i, j): sc.gt_transform(poses, i, j) for i in range(num_frag) for j in range(i + 1, num_frag)}
    dpath, kpath, spath = ev._paths(save, scene_name)
    for p in (dpath, kpath, spath):
        os.makedirs(p)
    for f in range(num_frag):
        np.save(os.path.join(dpath, 'cloud_bin_%d.D3Feat' % f), desc[f])
        np.save(os.path.join(kpath, 'cloud_bin_%d' % f), clouds[f])
        np.save(os.path.join(spath, 'cloud_bin_%d' % f), score[f])
    gtdir = str(tmp_path / 'gt')
    ev.writelog(gtdir, gt, num_frag)
    with open(os.path.join(gtdir, 'gt.info'), 'w') as fh:
        for key in sorted(gt, key=lambda k: tuple(int(x) for x in k.split('_'))):
            i, j = (int(x) for x in key.split('_'))
            I6 = np.zeros((6, 6))
            for q in clouds[i][:500].astype(np.float64):
                px = np.array([[0, -q[2], q[1]], [q[2], 0, -q[0]], [-q[1], q[0], 0]])
                J = np.hstack([np.eye(3), -px])
                I6 += J.T @ J
            fh.write('%d\t %d\t %d\t\n' % (i, j, num_frag))
            for r in I6:
                fh.write(''.join(' % .8e\t ' % v for v in r).rstrip(' ') + '\n')
    written = []
    real_writelog = ev.writelog

    def spy(path, transforms, n):
        written.append({k: np.array(v) for k, v in transforms.items()})
        return real_writelog(path, transforms, n)
    monkeypatch.setattr(ev, 'writelog', spy)
    kw = dict(num_points=1000, num_hypotheses=20000, distance_threshold=0.05, seed=0)
    icp = dict(max_distance=0.04)
    rec0, prec0, errs0 = reg.register_scene(save, scene_name, gtdir, out_log=str(tmp_path / 'ransac'), **kw)
    rec1, prec1, errs1 = reg.register_scene(save, scene_name, gtdir, out_log=str(tmp_path / 'icp'), icp=icp, **kw)
    est0, est1 = written
    keys = sorted(gt, key=lambda k: tuple(int(x) for x in k.split('_')))
    assert sorted(est0) == sorted(est1) == sorted(keys)
    want = reg.refine_transforms(clouds, keys, np.stack([est0[k] for k in keys]), **icp)[0].cpu().numpy()
    for n, key in enumerate(keys):
        assert np.abs(est1[key] - want[n]).max() < 1e-12, key
    log1 = ev.loadlog(str(tmp_path / 'icp'))
    for key in keys:
        assert np.abs(log1[key] - est1[key]).max() < 1e-8 * max(1.0, np.abs(est1[key]).max())
    far = [k for k in keys if int(k.split('_')[1]) - int(k.split('_')[0]) > 1]
    m0, m1 = np.median([errs0[k] for k in far]), np.median([errs1[k] for k in far])
    print("recall %.3f -> %.3f, median transformation_error over %d far pairs %.3e -> %.3e" % (
        rec0, rec1, len(far), m0, m1))
    assert rec1 >= rec0
    assert m1 < m0
    # one pair through estimate_transform: the same refinement
    dev = [torch.from_numpy(a).cuda() for a in (clouds[0], desc[0], score[0], clouds[2], desc[2], score[2])]
    plain = reg.estimate_transform(*dev, num_points=1000, num_hypotheses=20000, seed=0)
    refined = reg.estimate_transform(*dev, num_points=1000, num_hypotheses=20000, seed=0, icp=icp)
    again = reg.refine_transforms([clouds[0], clouds[2]], [(0, 1)], plain[0][None], **icp)[0][0]
    assert torch.equal(refined[0], again) and torch.equal(refined[1], plain[1])
