"""GPU: surface normals (ops.estimate_normals, csrc/normals.hip) against a brute-force NumPy oracle -- integer moments
bit for bit -- and their independence of row order, stacking and cell size; point-to-plane ICP (ops.icp_rigid(normals=),
csrc/icp.hip) against its NumPy restatement (registration.icp_numpy(normals=)); batch independence, determinism, graph
capture, and the estimation='point_to_plane' option of the registration front end."""
import os

import numpy as np
import pytest
import torch

from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.geometric_registration import evaluate as ev
from d3feat_pytorch_amd.geometric_registration import registration as reg
import icp_scene as sc
from test_icp_gpu import band_rows, device_grid, to_numpy
from test_normals_plane_cpu import ANGLE, HEALTHY, R_NORMAL, SHIFT, check_normals, perturbed_pairs

R = 0.075
R_ICP_NORMAL = 0.1


def brute_moments(p, radius):
    """int64 [n,10]: the moments of include/d3feat_hip.h for one f32 cloud by an n x n computation."""
    p = np.ascontiguousarray(p, dtype=np.float32)
    e = p[:, None, :] - p[None, :, :]                                  # the search's p_i - p_j
    d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    inside = d2 < np.float32(radius) * np.float32(radius)
    d = p[None, :, :] - p[:, None, :]                                  # p_j - p_i: one f32 subtraction
    u = np.rint(d.astype(np.float64) * reg.normals_scale(radius)).astype(np.int64) * inside[..., None]
    cols = [inside.sum(1)] + [u[..., k].sum(1) for k in range(3)]
    cols += [(u[..., a] * u[..., b]).sum(1) for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    return np.stack(cols, 1).astype(np.int64)


def normals_of(clouds, radius, grid_radius=None, **kw):
    pts = torch.from_numpy(np.concatenate(clouds)).cuda()
    grid = ops.CloudGrid(pts, [len(c) for c in clouds], radius if grid_radius is None else grid_radius)
    out = ops.estimate_normals(grid, None, radius, return_moments=True, **kw)
    assert int(grid.status.word.item()) == 0
    return out


@pytest.fixture(scope="module")
def small():
    clouds, _ = sc.make_scene(4, 2, n=6000)
    outs = normals_of(clouds, R_NORMAL)
    torch.cuda.synchronize()
    return clouds, outs


@pytest.mark.gpu
def test_moments_are_exact_and_normals_match_eigh(small):
    clouds, (normals, count, moments) = small
    want = np.concatenate([brute_moments(c, R_NORMAL) for c in clouds])
    normals, count, moments = to_numpy((normals, count, moments))
    assert all(1500 < len(c) < 2500 for c in clouds)
    assert np.array_equal(count, want[:, 0]) and count.dtype == np.int32
    assert np.array_equal(moments, want)
    assert want[:, 0].min() >= 1 and want[:, 0].max() > 64
    pts = np.concatenate(clouds)
    few = want[:, 0] < 3
    assert (normals[few] == 0).all()
    worst, share = check_normals(normals, want, pts, np.nonzero(~few)[0])       # the gap is measured on the oracle
    print("%d rows: worst angle %.3g rad, %.2f %% below the gap, %d rows with fewer than 3 neighbours" % (
        len(pts), worst, 100 * share, int(few.sum())))
    assert worst < ANGLE
    assert share <= 0.01
    # the NumPy restatement holds the same integers
    assert np.array_equal(reg.estimate_normals_numpy(clouds, R_NORMAL, return_moments=True)[2], want)


@pytest.mark.gpu
def test_normals_do_not_depend_on_order_stacking_or_cell_size(small):
    clouds, (normals, count, moments) = small
    a, b = clouds
    na = len(a)
    rng = np.random.default_rng(21)
    perm = rng.permutation(na)
    inv = torch.from_numpy(np.argsort(perm)).cuda()
    n2, c2, m2 = normals_of([a[perm]], R_NORMAL)
    assert torch.equal(n2[inv], normals[:na]) and torch.equal(c2[inv], count[:na]) and torch.equal(m2[inv], moments[:na])
    # the same cloud as clouds 0 and 2 around another one that overlaps it in coordinates
    other = (a[rng.permutation(na)[:na // 2]].astype(np.float64) + rng.normal(scale=0.05, size=(na // 2, 3)))
    n3, c3, m3 = normals_of([a, other.astype(np.float32), a], R_NORMAL)
    for lo in (0, na + na // 2):
        assert torch.equal(n3[lo:lo + na], normals[:na]) and torch.equal(m3[lo:lo + na], moments[:na])
    assert not torch.equal(m3[:na], normals_of([np.concatenate([a, other.astype(np.float32)])], R_NORMAL)[2][:na])
    # a coarser cell list gives the same bits
    n4, c4, m4 = normals_of(clouds, R_NORMAL, grid_radius=0.3)
    assert torch.equal(n4, normals) and torch.equal(c4, count) and torch.equal(m4, moments)
    # and so does a second run
    n5, c5, m5 = normals_of(clouds, R_NORMAL)
    assert torch.equal(n5, normals) and torch.equal(m5, moments)


@pytest.mark.gpu
def test_small_corners(small):
    clouds, _ = small
    one = np.float32([[0.5, -0.25, 1.0]])
    two = np.float32([[0.0, 0.0, 0.0], [0.01, 0.0, 0.0]])
    n, c, m = to_numpy(normals_of([one, two, one], 0.1))
    assert (n == 0).all() and c.tolist() == [1, 2, 2, 1]
    assert m[2].tolist() == brute_moments(two, 0.1)[1].tolist()
    # min_neighbors = 2 lets the pair through: a line's smallest eigenvector is perpendicular to it
    n, c = to_numpy(ops.estimate_normals(torch.from_numpy(two).cuda(), [2], 0.1, min_neighbors=2))
    assert (np.abs(n[:, 0]) < 1e-7).all() and (np.abs(np.linalg.norm(n, axis=1) - 1) < 1e-6).all()
    # a cell holding more than 64 points: one point 100 times over
    a = clouds[0][:600]
    dense = np.concatenate([a, np.repeat(a[7:8], 100, 0)])
    n, c, m = to_numpy(normals_of([dense], 0.1))
    want = brute_moments(dense, 0.1)
    assert np.array_equal(m, want) and c[7] >= 101 and np.array_equal(n[600:], np.repeat(n[7:8], 100, 0))
    copies = np.repeat(np.float32([[0.25, 0.5, -1.0]]), 100, 0)        # nothing but copies: no extent, no normal
    n, c, m = to_numpy(normals_of([copies], 0.1))
    assert (n == 0).all() and (c == 100).all() and (m[:, 1:] == 0).all()
    # a plane z = const: exactly +-(0, 0, 1), the sign follows the viewpoint
    rng = np.random.default_rng(22)
    plane = np.concatenate([rng.uniform(-1, 1, size=(1500, 2)), np.full((1500, 1), 0.5)], 1).astype(np.float32)
    for view, sign in (((0.0, 0.0, 2.0), 1.0), (None, -1.0), ((5.0, 5.0, 0.25), -1.0)):
        n, c, _ = to_numpy(normals_of([plane], 0.2, viewpoint=view))
        assert (c >= 3).all()
        assert (n[:, :2] == 0).all() and (n[:, 2] == sign).all(), view
    n, _, _ = to_numpy(normals_of([plane], 0.2, viewpoint=(0.0, 0.0, 0.5)))        # in the plane: the first non-zero > 0
    assert (n[:, :2] == 0).all() and (n[:, 2] == 1.0).all()
    grid = device_grid(clouds, 0.1)
    with pytest.raises(RuntimeError):
        ops.estimate_normals(grid, None, 0.2)
    with pytest.raises(ValueError):
        ops.estimate_normals(grid, None, 0.1, min_neighbors=0)
    with pytest.raises(ValueError):
        ops.estimate_normals(grid, None, 0.1, viewpoint=(0.0, 1.0))
    with pytest.raises(ValueError):
        ops.estimate_normals(grid.supports, None, 0.1)


# ------------------------------------------------------------------------------------------------ point-to-plane ICP
@pytest.fixture(scope="module")
def scene():
    return perturbed_pairs()


def plane_setup(clouds, view=None):
    grid = device_grid(clouds, R_ICP_NORMAL)
    normals = ops.estimate_normals(grid, None, R_ICP_NORMAL, viewpoint=view)[0]
    return grid, normals


@pytest.fixture(scope="module")
def gpu_run(scene):
    clouds, keys, pairs, G, T0 = scene
    grid, normals = plane_setup(clouds)
    outs = ops.icp_rigid(grid, None, pairs, T0, R, normals=normals)
    torch.cuda.synchronize()
    return grid, normals, outs


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [(0.0, 0.0, 0.0), SHIFT], ids=["as-generated", "shifted"])
def test_plane_run_matches_icp_numpy(scene, shift):
    """The four pairs with healthy overlap in one call against the NumPy restatement, the same f32 normals handed to
    both: iterations and status equal, T within 1e-6, count equal except by at most the pair's rows within rounding
    reach of the radius under the oracle's final T, and those are at most 0.1 % of the pair's rows (the bounds of
    test_icp_gpu.test_full_run_matches_icp_numpy)."""
    clouds, keys, pairs, G, T0 = scene
    keep = [p for p, k in enumerate(keys) if k in HEALTHY]
    assert len(keep) == 4
    pairs, T0 = pairs[keep], T0[keep]
    clouds = sc.shift_clouds(clouds, shift)
    T0 = np.stack([sc.shift_pose(T, shift) for T in T0])
    grid, normals = plane_setup(clouds, view=shift)
    T, count, rmse, iters, status, trace = to_numpy(ops.icp_rigid(grid, None, pairs, T0, R, normals=normals,
                                                                  return_trace=True))
    Tn, cn, rn, itn, stn, trn = reg.icp_numpy(clouds, pairs, T0, R, normals=normals.cpu().numpy(), return_trace=True)
    print("iterations", iters, itn, "status", status, stn)
    for p, (a, b) in enumerate(pairs):
        band = band_rows(clouds[a], clouds[b], Tn[p], R, shift)
        diff = abs(int(count[p]) - int(cn[p]))
        print("pair %d (%d rows): |T - T_numpy| = %.2e, count %d / %d, band rows %d, rmse diff %.2e, n_k %s / %s" % (
            p, len(clouds[a]), np.abs(T[p] - Tn[p]).max(), count[p], cn[p], band, abs(rmse[p] - rn[p]),
            trace[p, :iters[p] + 1, 0].astype(int).tolist(), trn[p, :itn[p] + 1, 0].astype(int).tolist()))
        assert band <= 1e-3 * len(clouds[a])
        assert diff <= band
    assert np.array_equal(iters, itn) and np.array_equal(status, stn)
    assert np.abs(T - Tn).max() < 1e-6
    assert (status == 0).all() and (iters >= 1).all() and (iters <= 8).all()


@pytest.mark.gpu
def test_max_iters_zero_is_the_point_to_point_search(scene, gpu_run):
    clouds, keys, pairs, G, T0 = scene
    grid, normals, _ = gpu_run
    a = ops.icp_rigid(grid, None, pairs, T0, R, max_iters=0, return_trace=True, normals=normals)
    b = ops.icp_rigid(grid, None, pairs, T0, R, max_iters=0, return_trace=True)
    assert all(torch.equal(x, y) for x, y in zip(a[:5], b[:5]))
    assert torch.equal(a[5], b[5]) and (a[3] == 0).all() and (a[1] > 1000).all()
    with pytest.raises(ValueError):
        ops.icp_rigid(grid, None, pairs, T0, R, normals=normals[:-1])
    with pytest.raises(RuntimeError):
        ops.icp_rigid(grid, None, pairs, T0, R, normals=normals.cpu())


@pytest.mark.gpu
def test_plane_batch_independent_and_deterministic(scene, gpu_run):
    clouds, keys, pairs, G, T0 = scene
    grid, normals, outs = gpu_run
    T, count, rmse, iters, status = outs
    assert (status == 0).all() and (iters >= 1).all()
    again = ops.icp_rigid(grid, None, pairs, T0, R, normals=normals)
    assert all(torch.equal(x, y) for x, y in zip(outs, again))
    for p in range(len(pairs)):
        one = ops.icp_rigid(grid, None, pairs[p:p + 1], T0[p:p + 1], R, normals=normals)
        for x, y in zip(outs, one):
            assert torch.equal(x[p:p + 1], y), p
    # a pair of fragments that do not meet (FEW), and a fixed cloud that is one plane with the moving cloud lying in it
    # (SINGULAR: the pose is free to slide): both keep their pose, and nobody else notices
    rng = np.random.default_rng(23)
    far = (clouds[0].astype(np.float64) + 50.0).astype(np.float32)
    wall = np.concatenate([rng.uniform(0, 1, size=(2000, 2)), np.full((2000, 1), 0.5)], 1).astype(np.float32)
    tile = np.concatenate([rng.uniform(0.2, 0.8, size=(700, 2)), np.full((700, 1), 0.5)], 1).astype(np.float32)
    grid7, normals7 = plane_setup(list(clouds) + [far, wall, tile])
    n4 = sum(len(c) for c in clouds)
    assert torch.equal(normals7[:n4], normals)
    slide = np.eye(4)
    slide[:3, 3] = [0.01, -0.02, 0.0]
    pairs8 = np.concatenate([pairs[:3], [[4, 0]], pairs[3:], [[6, 5]]])
    T8 = np.concatenate([T0[:3], np.eye(4)[None], T0[3:], slide[None]])
    got = ops.icp_rigid(grid7, None, pairs8, T8, R, normals=normals7)
    keep = [0, 1, 2, 4, 5, 6]
    for x, y in zip(outs, got):
        assert torch.equal(x, y[keep])
    assert int(got[4][3]) == ops.ICP_ST_FEW and int(got[3][3]) == 0 and int(got[1][3]) == 0
    assert torch.equal(got[0][3].cpu(), torch.eye(4, dtype=torch.float64))
    assert ops.ICP_ST_SINGULAR == 16 and int(got[4][7]) == ops.ICP_ST_SINGULAR and int(got[3][7]) == 0
    assert torch.equal(got[0][7].cpu(), torch.from_numpy(slide)) and int(got[1][7]) == len(tile)
    alone = ops.icp_rigid(grid7, None, pairs8[7:], T8[7:], R, normals=normals7)
    assert all(torch.equal(x[7:], y) for x, y in zip(got, alone))
    # the NumPy restatement flags the same two pairs
    stn = reg.icp_numpy(list(clouds) + [far, wall, tile], pairs8[[3, 7]], T8[[3, 7]], R,
                        normals=normals7.cpu().numpy())[4]
    assert stn.tolist() == [reg.ICP_ST_FEW, reg.ICP_ST_SINGULAR]


@pytest.mark.gpu
def test_graph_capture_of_normals_and_plane_icp_replays_bit_identically(scene):
    clouds, keys, pairs, G, T0 = scene
    grid = device_grid(clouds, R_ICP_NORMAL)
    dev_pairs = torch.from_numpy(pairs.astype(np.int32)).cuda()
    rows = int(sum(len(clouds[a]) for a, _ in pairs))
    Ti = torch.from_numpy(T0).cuda()
    kw = dict(max_iters=12, rows=rows)

    def run():
        normals = ops.estimate_normals(grid, None, R_ICP_NORMAL)[0]
        return normals, ops.icp_rigid(grid, None, dev_pairs, Ti, R, normals=normals, **kw)
    run()                                                          # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        normals, outs = run()
    rng = np.random.default_rng(78)
    other = np.stack([Gp @ sc.perturbation(rng, 2, 0.03) for Gp in G])
    Ti.copy_(torch.from_numpy(other).cuda())
    normals.zero_()                                                # the replay has to estimate them again
    g.replay()
    torch.cuda.synchronize()
    want_normals, want = run()
    assert torch.equal(normals, want_normals) and bool((normals != 0).any())
    assert all(torch.equal(x, y) for x, y in zip(outs, want))
    assert (want[4] == 0).all() and (want[3] >= 1).all()


# ------------------------------------------------------------------------------------------------ the front end
@pytest.mark.gpu
def test_refine_transforms_point_to_plane_device_equals_cpu_path(scene):
    clouds, keys, pairs, G, T0 = scene
    sel = [keys.index('0_1'), keys.index('0_3')]
    T, fitness, rmse, iters = reg.refine_transforms(clouds, [keys[p] for p in sel], T0[sel], R, max_iters=8,
                                                    estimation='point_to_plane', normal_radius=R_ICP_NORMAL)
    Tn, fn, rn, itn = reg.refine_transforms(clouds, [keys[p] for p in sel], T0[sel], R, device='cpu', max_iters=8,
                                            estimation='point_to_plane', normal_radius=R_ICP_NORMAL)
    print("|T - T_cpu| = %.2e, iterations %s / %s" % (np.abs(T.cpu().numpy() - Tn).max(), iters.tolist(), itn.tolist()))
    assert np.abs(T.cpu().numpy() - Tn).max() < 1e-6 and np.array_equal(iters.cpu().numpy(), itn)
    assert np.abs(fitness.cpu().numpy() - fn).max() < 1e-3
    for n, p in enumerate(sel):
        assert sc.pose_error(T[n].cpu().numpy(), G[p])[0] < 0.1
    with pytest.raises(ValueError):
        reg.refine_transforms(clouds, [keys[0]], T0[:1], R, estimation='plane')


@pytest.mark.gpu
def test_refine_transforms_without_the_new_keywords_is_todays_call(scene):
    clouds, keys, pairs, G, T0 = scene
    T, fitness, rmse, iters = reg.refine_transforms(clouds, keys, T0, R, max_iters=5)
    want = ops.icp_rigid(device_grid(clouds, R), None, pairs, T0, R, max_iters=5)
    assert torch.equal(T, want[0]) and torch.equal(rmse, want[2]) and torch.equal(iters, want[3])
    lens = torch.tensor([len(clouds[a]) for a, _ in pairs], dtype=torch.float64, device='cuda')
    assert torch.equal(fitness, want[1].double() / lens)
    # the default normal_radius is 2 max_distance, on one cell list at that radius
    Tp = reg.refine_transforms(clouds, keys[:1], T0[:1], R, estimation='point_to_plane')
    grid = device_grid(clouds, 2 * R)
    normals = ops.estimate_normals(grid, None, 2 * R)[0]
    want = ops.icp_rigid(grid, None, pairs[:1], T0[:1], R, normals=normals)
    assert torch.equal(Tp[0], want[0]) and torch.equal(Tp[3], want[3])


@pytest.mark.gpu
def test_register_scene_point_to_plane_refines_every_pair_in_one_call(tmp_path, monkeypatch):
    """register_scene(icp=dict(..., estimation='point_to_plane')) == refine_transforms with the same keywords applied to
    what register_scene(icp=None) estimates (same seed), to 1e-12, compared as register_scene hands them to
    evaluate.writelog (the layout of test_icp_gpu.test_register_scene_refines_every_pair_in_one_call)."""
    num_frag, scene_name, save = 4, 'surface-room', str(tmp_path / 'dump')
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
    written = []
    real_writelog = ev.writelog

    def spy(path, transforms, n):
        written.append({k: np.array(v) for k, v in transforms.items()})
        return real_writelog(path, transforms, n)
    monkeypatch.setattr(ev, 'writelog', spy)
    kw = dict(num_points=1000, num_hypotheses=20000, distance_threshold=0.05, seed=0)
    icp = dict(max_distance=0.04, estimation='point_to_plane', normal_radius=0.1)
    assert reg.register_scene(save, scene_name, gtdir, out_log=str(tmp_path / 'ransac'), **kw) is None    # no gt.info
    reg.register_scene(save, scene_name, gtdir, out_log=str(tmp_path / 'plane'), icp=icp, **kw)
    est0, est1 = written
    keys = sorted(gt, key=lambda k: tuple(int(x) for x in k.split('_')))
    assert sorted(est0) == sorted(est1) == sorted(keys)
    want, _, _, iters = reg.refine_transforms(clouds, keys, np.stack([est0[k] for k in keys]), **icp)
    want = want.cpu().numpy()
    for n, key in enumerate(keys):
        assert np.abs(est1[key] - want[n]).max() < 1e-12, key
    assert (iters >= 1).any() and any(np.abs(est1[k] - est0[k]).max() > 1e-6 for k in keys)
    # one pair through estimate_transform: the same refinement
    dev = [torch.from_numpy(a).cuda() for a in (clouds[0], desc[0], score[0], clouds[1], desc[1], score[1])]
    plain = reg.estimate_transform(*dev, num_points=1000, num_hypotheses=20000, seed=0)
    refined = reg.estimate_transform(*dev, num_points=1000, num_hypotheses=20000, seed=0, icp=icp)
    again = reg.refine_transforms([clouds[0], clouds[1]], [(0, 1)], plain[0][None], **icp)[0][0]
    assert torch.equal(refined[0], again) and torch.equal(refined[1], plain[1])
