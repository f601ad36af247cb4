"""GPU: colour gradients (ops.color_gradients, csrc/normals.hip kColor) against the NumPy restatement -- integer moments
bit for bit -- and their independence of row order, stacking and cell size; coloured ICP (ops.icp_rigid(color_field=),
csrc/icp.hip kColor) against registration.icp_numpy(color_field=) on the plane slide and the room; the bit identities
with the point-to-plane form, batch independence, determinism, graph capture, and estimation='colored' of the front
end.  Cases: colored_icp_cases.py."""
import numpy as np
import pytest
import torch

from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.geometric_registration import registration as reg
import colored_icp_cases as cc
import icp_scene as sc
from test_icp_gpu import band_rows, device_grid, to_numpy
from test_normals_plane_cpu import HEALTHY, SHIFT

R, R_GRAD = cc.R_ICP, cc.R_GRAD


def gradients_of(clouds, cols, grid_radius=R_GRAD, normals=None, **kw):
    """(normals, field, count, moments) of the stacked clouds on the device."""
    grid = device_grid(clouds, grid_radius)
    if normals is None:
        normals = ops.estimate_normals(grid, None, R_GRAD)[0]
    inten = torch.from_numpy(np.concatenate(cols)).cuda()
    out = ops.color_gradients(grid, None, R_GRAD, normals, inten, return_moments=True, **kw)
    assert int(grid.status.word.item()) == 0
    return (normals,) + out


def check_against_numpy(clouds, cols, normals, field, count, moments):
    fn, cn, mn = reg.color_gradients_numpy(clouds, R_GRAD, normals.cpu().numpy(), np.concatenate(cols),
                                           return_moments=True)
    field, count, moments = to_numpy((field, count, moments))
    assert count.dtype == np.int32 and np.array_equal(count, cn)
    assert moments.dtype == np.int64 and np.array_equal(moments, mn)
    assert np.array_equal(np.isnan(field), np.isnan(fn))
    ok = np.isfinite(fn[:, 0])
    scale = np.maximum(1.0, np.abs(fn[ok, :3]).max(1))
    err = (np.abs(field[ok, :3].astype(np.float64) - fn[ok, :3]).max(1) / scale).max()
    assert np.array_equal(field[:, 3], fn[:, 3], equal_nan=True)
    return err, ok


@pytest.fixture(scope="module")
def small():
    clouds, cols = cc.small()
    outs = gradients_of(clouds, cols)
    torch.cuda.synchronize()
    return clouds, cols, outs


@pytest.mark.gpu
def test_moments_are_exact_and_gradients_match_numpy(small):
    clouds, cols, (normals, field, count, moments) = small
    assert all(1500 < len(c) < 2500 for c in clouds)                  # several workgroups of 256 rows and a ragged one
    err, ok = check_against_numpy(clouds, cols, normals, field, count, moments)
    print("small: %d rows, %d valid, worst |d - d_numpy| / max(1, |d|) = %.3g" % (len(ok), ok.sum(), err))
    assert err < 1e-6 and ok.mean() > 0.5 and not ok.all()      # (a sparse scene: both kinds)
    d = field[:, :3].double()
    dot = (d * normals.double()).sum(1)[torch.from_numpy(ok).cuda()].abs()
    assert float((dot / d[torch.from_numpy(ok).cuda()].abs().amax(1).clamp(min=1.0)).max()) < 1e-6
    # the ramp: 700 rows, two full workgroups and a partial one; the exact gradient comes back
    cloud, inten, normal, want = cc.ramp()
    nr, f, c, m = gradients_of([cloud], [inten])
    err, ok = check_against_numpy([cloud], [inten], nr, f, c, m)
    worst = np.abs(f.cpu().numpy()[:, :3].astype(np.float64) - want).max()
    print("ramp: worst |d - d_numpy| = %.3g, worst |d - exact| = %.3g" % (err, worst))
    assert err < 1e-6 and ok.all() and worst < 1e-4


@pytest.mark.gpu
def test_gradients_do_not_depend_on_order_stacking_or_cell_size(small):
    clouds, cols, (normals, field, count, moments) = small
    a, ia = clouds[0], cols[0]
    na = len(a)
    same = lambda x, y: torch.equal(x.view(torch.int32), y.view(torch.int32))    # bits: NaN compares equal to itself
    rng = np.random.default_rng(21)
    perm = rng.permutation(na)
    inv = torch.from_numpy(np.argsort(perm)).cuda()
    n2, f2, c2, m2 = gradients_of([a[perm]], [ia[perm]])
    assert torch.equal(n2[inv], normals[:na])
    assert same(f2[inv], field[:na]) and torch.equal(c2[inv], count[:na]) and torch.equal(m2[inv], moments[:na])
    # the same cloud as clouds 0 and 2 around another one that overlaps it in coordinates
    pick = rng.permutation(na)[:na // 2]
    other = (a[pick].astype(np.float64) + rng.normal(scale=0.05, size=(na // 2, 3))).astype(np.float32)
    n3, f3, c3, m3 = gradients_of([a, other, a], [ia, ia[pick], ia])
    for lo in (0, na + na // 2):
        assert same(f3[lo:lo + na], field[:na]) and torch.equal(m3[lo:lo + na], moments[:na])
    # coarser cell lists give the same bits, and so does a second run
    for cell in (0.2, 0.3):
        n4, f4, c4, m4 = gradients_of(clouds, cols, grid_radius=cell)
        assert same(f4, field) and torch.equal(c4, count) and torch.equal(m4, moments)
    n5, f5, c5, m5 = gradients_of(clouds, cols)
    assert same(f5, field) and torch.equal(m5, moments)


@pytest.mark.gpu
def test_gradient_corners(small):
    clouds, cols, (normals, field, count, moments) = small
    # intensities that are not usable: the row is not searched and counts for nobody else
    inten = np.concatenate(cols).copy()
    bad = np.random.default_rng(5).permutation(len(inten))[:60]
    inten[bad[:20]], inten[bad[20:40]], inten[bad[40:]] = np.nan, -0.1, 1.5
    split = np.cumsum([len(c) for c in clouds])[:-1]
    n1, f1, c1, m1 = gradients_of(clouds, np.split(inten, split), normals=normals)
    err, ok = check_against_numpy(clouds, np.split(inten, split), normals, f1, c1, m1)
    assert err < 1e-6
    assert bool(torch.isnan(f1[bad]).all()) and bool((c1[bad] == 0).all()) and bool((m1[bad] == 0).all())
    assert bool((c1 <= count).all()) and int((c1 < count).sum()) > 60
    # a zero normal, and min_neighbors above the neighbourhood: three NaNs, the intensity stays
    zero = normals.clone()
    zero[:100] = 0
    n2, f2, c2, m2 = gradients_of(clouds, cols, normals=zero)
    assert bool(torch.isnan(f2[:100, :3]).all()) and torch.equal(f2[:100, 3], field[:100, 3])
    assert torch.equal(m2, moments) and torch.equal(f2[100:].view(torch.int32), field[100:].view(torch.int32))
    n3, f3, c3, m3 = gradients_of(clouds, cols, normals=normals, min_neighbors=20)
    few = count < 20
    assert bool(few.any()) and bool((~few).any())
    assert bool(torch.isnan(f3[few, :3]).all()) and not bool(torch.isnan(f3[~few, 3]).any())
    assert torch.equal(f3[~few].view(torch.int32), field[~few].view(torch.int32))
    # rows beyond the clouds are NaN; a lone point has no gradient
    pts = torch.from_numpy(np.concatenate(clouds)).cuda()
    N = len(pts)
    grid = ops.CloudGrid(pts, [len(clouds[0]), len(clouds[1]) - 5], R_GRAD)
    f4, c4, m4 = ops.color_gradients(grid, None, R_GRAD, normals, torch.from_numpy(np.concatenate(cols)).cuda(),
                                     return_moments=True)
    assert bool(torch.isnan(f4[N - 5:]).all()) and bool((c4[N - 5:] == 0).all()) and bool((m4[N - 5:] == 0).all())
    assert torch.equal(m4[:len(clouds[0])], moments[:len(clouds[0])])
    one = torch.tensor([[0.5, -0.25, 1.0]], device='cuda')
    f5, c5 = ops.color_gradients(one, [1], 0.1, torch.tensor([[0.0, 0.0, 1.0]], device='cuda'),
                                 torch.tensor([0.5], device='cuda'))
    assert c5.tolist() == [1] and bool(torch.isnan(f5[0, :3]).all()) and float(f5[0, 3]) == 0.5
    grid = device_grid(clouds, R_GRAD)
    inten = torch.from_numpy(np.concatenate(cols)).cuda()
    with pytest.raises(RuntimeError):
        ops.color_gradients(grid, None, 0.2, normals, inten)
    with pytest.raises(ValueError):
        ops.color_gradients(grid, None, R_GRAD, normals, inten, min_neighbors=0)
    with pytest.raises(ValueError):
        ops.color_gradients(grid, None, R_GRAD, normals[:-1], inten)
    with pytest.raises(ValueError):
        ops.color_gradients(grid, None, R_GRAD, normals, inten[:-1])
    with pytest.raises(RuntimeError):
        ops.color_gradients(grid, None, R_GRAD, normals, inten.cpu())


# ------------------------------------------------------------------------------------------------ coloured ICP
@pytest.fixture(scope="module")
def scene():
    """The room's four fragments and the slide's two in one stack: seven pairs, the slide's last."""
    clouds, cols, keys, pairs, G, T0 = cc.room()
    sl_clouds, sl_cols, sl_G, sl_T0 = cc.plane_slide()
    assert all(7000 <= len(c) <= 8400 for c in clouds) and len(sl_clouds[1]) == 5000      # 5000 = 9 * 512 + 392
    return (list(clouds) + sl_clouds, list(cols) + sl_cols, list(keys) + ['slide'],
            np.concatenate([pairs, [[5, 4]]]), np.concatenate([G, sl_G[None]]), np.concatenate([T0, sl_T0[None]]))


def colour_setup(clouds, cols, view=None):
    grid = device_grid(clouds, R_GRAD)
    normals = ops.estimate_normals(grid, None, R_GRAD, viewpoint=view)[0]
    field = ops.color_gradients(grid, None, R_GRAD, normals, torch.from_numpy(np.concatenate(cols)).cuda())[0]
    return grid, normals, field


@pytest.fixture(scope="module")
def gpu_run(scene):
    clouds, cols, keys, pairs, G, T0 = scene
    grid, normals, field = colour_setup(clouds, cols)
    outs = ops.icp_rigid(grid, None, pairs, T0, R, normals=normals, color_field=field)
    torch.cuda.synchronize()
    return grid, normals, field, outs


def compare_with_oracle(clouds, pairs, T0, shift, grid, normals, field):
    """The bounds of test_normals_plane_gpu.test_plane_run_matches_icp_numpy, with n_color under count's bound and
    color_rmse within 1e-9."""
    T, count, rmse, iters, status, trace, n_color, color_rmse = to_numpy(ops.icp_rigid(
        grid, None, pairs, T0, R, normals=normals, color_field=field, return_trace=True))
    Tn, cn, rn, itn, stn, trn, ncn, crn = reg.icp_numpy(clouds, pairs, T0, R, normals=normals.cpu().numpy(),
                                                        color_field=field.cpu().numpy(), return_trace=True)
    print("iterations", iters, itn, "status", status, stn)
    for p, (a, b) in enumerate(pairs):
        band = band_rows(clouds[a], clouds[b], Tn[p], R, shift)
        print("pair %d (%d rows): |T - T_numpy| = %.2e, count %d / %d, n_color %d / %d, band rows %d, colour rmse diff "
              "%.2e" % (p, len(clouds[a]), np.abs(T[p] - Tn[p]).max(), count[p], cn[p], n_color[p], ncn[p], band,
                        abs(color_rmse[p] - crn[p])))
        assert band <= 1e-3 * len(clouds[a])
        assert abs(int(count[p]) - int(cn[p])) <= band
        assert abs(int(n_color[p]) - int(ncn[p])) <= band
    assert np.array_equal(iters, itn) and np.array_equal(status, stn)
    assert np.abs(T - Tn).max() < 1e-6
    assert np.abs(color_rmse - crn).max() < 1e-9
    assert (status == 0).all() and (iters >= 1).all() and (iters <= 10).all()
    return T, n_color


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [(0.0, 0.0, 0.0), SHIFT], ids=["as-generated", "shifted"])
def test_coloured_run_matches_icp_numpy(scene, shift):
    """The plane slide and the four room pairs with healthy overlap in one call against the NumPy restatement, the same
    f32 normals and field handed to both."""
    clouds, cols, keys, pairs, G, T0 = scene
    keep = [p for p, k in enumerate(keys) if k in HEALTHY or k == 'slide']
    assert len(keep) == 5
    pairs, G, T0 = pairs[keep], G[keep], T0[keep]
    clouds, T0 = cc.shifted(clouds, T0, shift)
    grid, normals, field = colour_setup(clouds, cols, view=shift)
    T, n_color = compare_with_oracle(clouds, pairs, T0, shift, grid, normals, field)
    assert (n_color > 3000).all()
    # the capability: the slide, which point-to-plane cannot hold, ends at the truth
    deg, off = sc.pose_error(sc.shift_pose(T[-1], [-v for v in shift]), G[-1])      # (about the scene's own origin)
    print("slide: %.4f deg / %.3f mm" % (deg, 1e3 * off))
    assert deg < 0.05 and off < 1e-3


@pytest.mark.gpu
def test_field_with_missing_rows_matches_icp_numpy(scene, gpu_run):
    clouds, cols, keys, pairs, G, T0 = scene
    grid, normals, field, outs = gpu_run
    keep = [p for p, k in enumerate(keys) if k in HEALTHY or k == 'slide']
    holes = field.clone()
    gone = torch.from_numpy(np.random.default_rng(3).uniform(size=len(field)) < 0.1).cuda()
    holes[gone] = float('nan')
    T, n_color = compare_with_oracle(clouds, pairs[keep], T0[keep], (0.0, 0.0, 0.0), grid, normals, holes)
    full = outs[5].cpu().numpy()[keep]
    assert (n_color < 0.9 * full).all() and (n_color > 0.7 * full).all()      # a row needs both of its ends


@pytest.mark.gpu
def test_bit_identities_with_the_other_forms(scene, gpu_run):
    clouds, cols, keys, pairs, G, T0 = scene
    grid, normals, field, outs = gpu_run
    plane = ops.icp_rigid(grid, None, pairs, T0, R, normals=normals, return_trace=True)
    # lambda_geometric = 1: sqrt(1) scales nothing and the colour rows add +-0
    one = ops.icp_rigid(grid, None, pairs, T0, R, normals=normals, color_field=field, lambda_geometric=1.0,
                        return_trace=True)
    assert len(one) == 8 and all(torch.equal(x, y) for x, y in zip(one[:5], plane[:5]))
    assert torch.equal(one[5].view(torch.int64), plane[5].view(torch.int64))           # the trace, NaNs included
    assert bool((one[6] > 1000).all()) and bool((one[7] > 0).all())
    # max_iters = 0 is the point-to-point search
    a = ops.icp_rigid(grid, None, pairs, T0, R, max_iters=0, return_trace=True, normals=normals, color_field=field)
    b = ops.icp_rigid(grid, None, pairs, T0, R, max_iters=0, return_trace=True)
    assert all(torch.equal(x, y) for x, y in zip(a[:6], b)) and bool((a[3] == 0).all()) and bool((a[6] > 1000).all())
    # a field that is NaN everywhere: no colour row.  At lambda_geometric = 1 that is point-to-plane bit for bit; at
    # the default every sum is point-to-plane's times lambda up to rounding (each J, r is scaled before the products
    # are formed), so the least-squares step is the same to rounding: the same iterations, T within 1e-9
    dark = torch.full_like(field, float('nan'))
    d1 = ops.icp_rigid(grid, None, pairs, T0, R, normals=normals, color_field=dark, lambda_geometric=1.0,
                       return_trace=True)
    assert all(torch.equal(x, y) for x, y in zip(d1[:5], plane[:5]))
    assert torch.equal(d1[5].view(torch.int64), plane[5].view(torch.int64))
    assert bool((d1[6] == 0).all()) and bool((d1[7] == 0).all())
    d2 = ops.icp_rigid(grid, None, pairs, T0, R, normals=normals, color_field=dark, return_trace=True)
    assert bool((d2[6] == 0).all()) and bool((d2[7] == 0).all())
    assert torch.equal(d2[3], plane[3]) and torch.equal(d2[4], plane[4])
    print("all-NaN field at the default lambda: |T - T_plane| = %.2e" % float((d2[0] - plane[0]).abs().max()))
    assert float((d2[0] - plane[0]).abs().max()) < 1e-9
    with pytest.raises(ValueError):
        ops.icp_rigid(grid, None, pairs, T0, R, color_field=field)
    with pytest.raises(ValueError):
        ops.icp_rigid(grid, None, pairs, T0, R, normals=normals, color_field=field[:-1])
    with pytest.raises(ValueError):
        ops.icp_rigid(grid, None, pairs, T0, R, normals=normals, color_field=field, lambda_geometric=-0.1)
    with pytest.raises(RuntimeError):
        ops.icp_rigid(grid, None, pairs, T0, R, normals=normals, color_field=field.cpu())


@pytest.mark.gpu
def test_coloured_batch_independent_and_deterministic(scene, gpu_run):
    clouds, cols, keys, pairs, G, T0 = scene
    grid, normals, field, outs = gpu_run
    assert len(outs) == 7 and bool((outs[4] == 0).all()) and bool((outs[3] >= 1).all())
    again = ops.icp_rigid(grid, None, pairs, T0, R, normals=normals, color_field=field)
    assert all(torch.equal(x, y) for x, y in zip(outs, again))
    for p in range(len(pairs)):
        one = ops.icp_rigid(grid, None, pairs[p:p + 1], T0[p:p + 1], R, normals=normals, color_field=field)
        for x, y in zip(outs, one):
            assert torch.equal(x[p:p + 1], y), p
    # every pair ends where the NumPy figures say: within 0.1 deg / 2.5 mm, the low-overlap pairs in at most 12 fits
    T, iters = outs[0].cpu().numpy(), outs[3].cpu().numpy()
    for p, key in enumerate(keys):
        deg, off = sc.pose_error(T[p], G[p])
        print("%s: %d fits, %.3f deg / %.2f mm" % (key, iters[p], deg, 1e3 * off))
        assert deg < 0.1 and off < 2.5e-3 and iters[p] <= 12, key
    # a pair the setup stops reports no colour
    bad = ops.icp_rigid(grid, None, pairs[:2], np.stack([T0[0], np.full((4, 4), np.nan)]), R, normals=normals,
                        color_field=field)
    assert int(bad[4][1]) == ops.ICP_ST_NONFINITE and int(bad[5][1]) == 0 and float(bad[6][1]) == 0.0
    assert all(torch.equal(x[:1], y[:1]) for x, y in zip(bad, outs))


@pytest.mark.gpu
def test_graph_capture_of_gradients_and_coloured_icp_replays_bit_identically(scene):
    clouds, cols, keys, pairs, G, T0 = scene
    grid = device_grid(clouds, R_GRAD)
    inten = torch.from_numpy(np.concatenate(cols)).cuda()
    dev_pairs = torch.from_numpy(pairs.astype(np.int32)).cuda()
    rows = int(sum(len(clouds[a]) for a, _ in pairs))
    Ti = torch.from_numpy(T0).cuda()
    kw = dict(max_iters=12, rows=rows)

    def run():
        normals = ops.estimate_normals(grid, None, R_GRAD)[0]
        field = ops.color_gradients(grid, None, R_GRAD, normals, inten)[0]
        return field, ops.icp_rigid(grid, None, dev_pairs, Ti, R, normals=normals, color_field=field, **kw)
    run()                                                          # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        field, outs = run()
    rng = np.random.default_rng(78)
    other = np.stack([Gp @ sc.perturbation(rng, 1, 0.02) for Gp in G])
    Ti.copy_(torch.from_numpy(other).cuda())
    field.zero_()                                                  # the replay has to compute it again
    g.replay()
    torch.cuda.synchronize()
    want_field, want = run()
    assert torch.equal(field.view(torch.int32), want_field.view(torch.int32)) and bool((field[:, 3] > 0).any())
    assert all(torch.equal(x, y) for x, y in zip(outs, want))
    assert bool((want[4] == 0).all()) and bool((want[3] >= 1).all()) and bool((want[5] > 1000).all())


# ------------------------------------------------------------------------------------------------ the front end
@pytest.mark.gpu
def test_refine_transforms_colored_device_equals_cpu_path(scene):
    clouds, cols, keys, pairs, G, T0 = scene
    frag_keys = ['0_1', '0_3', (4, 5)]                                 # two room pairs and the slide
    sel = [keys.index('0_1'), keys.index('0_3'), keys.index('slide')]
    kw = dict(max_iters=10, estimation='colored', normal_radius=R_GRAD, colors=[c[:, None] for c in cols])
    T, fitness, rmse, iters = reg.refine_transforms(clouds, frag_keys, T0[sel], R, **kw)
    Tn, fn, rn, itn = reg.refine_transforms(clouds, frag_keys, T0[sel], R, device='cpu', **kw)
    print("|T - T_cpu| = %.2e, iterations %s / %s" % (np.abs(T.cpu().numpy() - Tn).max(), iters.tolist(), itn.tolist()))
    assert np.abs(T.cpu().numpy() - Tn).max() < 1e-6 and np.array_equal(iters.cpu().numpy(), itn)
    assert np.abs(fitness.cpu().numpy() - fn).max() < 1e-3
    for n, p in enumerate(sel):
        assert sc.pose_error(T[n].cpu().numpy(), G[p])[0] < 0.1
    # it is one cell list, one normals launch, one gradients launch and one coloured call
    grid, normals, field = colour_setup(clouds, cols)
    want = ops.icp_rigid(grid, None, pairs[sel], T0[sel], R, max_iters=10, normals=normals, color_field=field)
    assert torch.equal(T, want[0]) and torch.equal(iters, want[3]) and torch.equal(rmse, want[2])
    with pytest.raises(ValueError):
        reg.refine_transforms(clouds, frag_keys, T0[sel], R, estimation='colored')
    # without the new keywords the call is today's
    Tp = reg.refine_transforms(clouds, frag_keys[:2], T0[sel[:2]], R, estimation='point_to_plane', normal_radius=R_GRAD)
    want = ops.icp_rigid(grid, None, pairs[sel[:2]], T0[sel[:2]], R, normals=normals)
    assert torch.equal(Tp[0], want[0]) and torch.equal(Tp[2], want[2]) and torch.equal(Tp[3], want[3])
    Tq = reg.refine_transforms(clouds, frag_keys[:2], T0[sel[:2]], R, max_iters=5)
    want = ops.icp_rigid(device_grid(clouds, R), None, pairs[sel[:2]], T0[sel[:2]], R, max_iters=5)
    assert torch.equal(Tq[0], want[0]) and torch.equal(Tq[2], want[2]) and torch.equal(Tq[3], want[3])


@pytest.mark.gpu
def test_register_scene_colored_reads_the_fragments_colours(tmp_path, monkeypatch):
    """register_scene(icp=dict(..., estimation='colored', colors=<folder of cloud_bin_<i>.ply>)) == refine_transforms
    with the colours read back from those files applied to what register_scene(icp=None) estimates (same seed), compared
    as register_scene hands them to evaluate.writelog; a fragment without colours is an error."""
    import os
    from d3feat_pytorch_amd.datasets import fragments as fr
    from d3feat_pytorch_amd.geometric_registration import evaluate as ev
    num_frag, scene_name, save = 3, 'painted-room', str(tmp_path / 'dump')
    clouds, poses, world, ids = sc.make_scene(3, num_frag, return_world=True)
    cols = cc.paint(world, ids)
    rng = np.random.default_rng(9)
    desc = sc.position_descriptors(rng, world, ids)
    score = [rng.permutation(len(c)).astype(np.float32)[:, None] / len(c) for c in clouds]
    gt = {'%d_%d' % (i, j): sc.gt_transform(poses, i, j) for i in range(num_frag) for j in range(i + 1, num_frag)}
    dpath, kpath, spath = ev._paths(save, scene_name)
    ply = str(tmp_path / 'ply')
    for p in (dpath, kpath, spath, ply):
        os.makedirs(p)
    for f in range(num_frag):
        np.save(os.path.join(dpath, 'cloud_bin_%d.D3Feat' % f), desc[f])
        np.save(os.path.join(kpath, 'cloud_bin_%d' % f), clouds[f])
        np.save(os.path.join(spath, 'cloud_bin_%d' % f), score[f])
        fr.write_ply_points(os.path.join(ply, 'cloud_bin_%d.ply' % f), clouds[f], colors=cols[f][:, None])
    gtdir = str(tmp_path / 'gt')
    ev.writelog(gtdir, gt, num_frag)
    written = []
    real_writelog = ev.writelog

    def spy(path, transforms, n):
        written.append({k: np.array(v) for k, v in transforms.items()})
        return real_writelog(path, transforms, n)
    monkeypatch.setattr(ev, 'writelog', spy)
    kw = dict(num_points=1000, num_hypotheses=20000, distance_threshold=0.05, seed=0)
    icp = dict(max_distance=0.04, estimation='colored', normal_radius=0.1)
    reg.register_scene(save, scene_name, gtdir, out_log=str(tmp_path / 'ransac'), **kw)
    reg.register_scene(save, scene_name, gtdir, out_log=str(tmp_path / 'colored'), icp=dict(icp, colors=ply), **kw)
    est0, est1 = written
    keys = sorted(gt, key=lambda k: tuple(int(x) for x in k.split('_')))
    back = [fr.read_ply_colors(os.path.join(ply, 'cloud_bin_%d.ply' % f)) for f in range(num_frag)]
    assert all(np.abs(b[:, 0] - c).max() <= 0.5 / 255 + 1e-7 for b, c in zip(back, cols))       # 8 bits per channel
    want, _, _, iters = reg.refine_transforms(clouds, keys, np.stack([est0[k] for k in keys]), colors=back, **icp)
    want = want.cpu().numpy()
    for n, key in enumerate(keys):
        assert np.abs(est1[key] - want[n]).max() < 1e-12, key
    assert (iters >= 1).any() and any(np.abs(est1[k] - est0[k]).max() > 1e-6 for k in keys)
    # a list of per-fragment arrays is taken as it is; a fragment without colours raises
    reg.register_scene(save, scene_name, gtdir, out_log=str(tmp_path / 'list'), icp=dict(icp, colors=back), **kw)
    assert all(np.array_equal(written[2][k], est1[k]) for k in keys)
    fr.write_ply_points(os.path.join(ply, 'cloud_bin_1.ply'), clouds[1])
    with pytest.raises(ValueError):
        reg.register_scene(save, scene_name, gtdir, out_log=str(tmp_path / 'none'), icp=dict(icp, colors=ply), **kw)
    with pytest.raises(ValueError):
        reg.register_scene(save, scene_name, gtdir, out_log=str(tmp_path / 'none'), icp=icp, **kw)
