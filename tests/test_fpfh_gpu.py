"""GPU: ops.fpfh (csrc/fpfh.hip) against the NumPy restatement bit for bit, its independence from anything that orders
the neighbours, the edge cases, a neighbourhood of thousands, graph capture, and FPFH through the registration chain."""
import numpy as np
import pytest
import torch

from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.geometric_registration import evaluate as ev
from d3feat_pytorch_amd.geometric_registration import registration as reg
import fpfh_cases as fc
import icp_scene as sc

SEED = fc.SEEDS[0]


def fpfh_of(clouds, normals, radius=fc.R_FPFH, grid_radius=None, **kw):
    pts = torch.from_numpy(np.concatenate(clouds)).cuda()
    grid = ops.CloudGrid(pts, [len(c) for c in clouds], radius if grid_radius is None else grid_radius)
    out = ops.fpfh(grid, None, radius, torch.from_numpy(np.ascontiguousarray(normals)).cuda(), return_spfh=True, **kw)
    assert int(grid.status.word.item()) == 0
    return out


@pytest.fixture(scope="module")
def terrain():
    clouds, _, normals, _ = fc.scene(SEED)
    nrm = fc.zeroed(normals)
    want = reg.fpfh_numpy(list(clouds), fc.R_FPFH, nrm, return_spfh=True)
    got = fpfh_of(clouds, nrm)
    torch.cuda.synchronize()
    return clouds, nrm, want, got


@pytest.mark.gpu
def test_device_equals_the_restatement_bit_for_bit(terrain):
    clouds, nrm, want, got = terrain
    desc, count, spfh = (t.cpu().numpy() for t in got)
    assert desc.dtype == np.float32 and count.dtype == np.int32 and spfh.dtype == np.int32
    assert np.array_equal(spfh, want[2])
    assert np.array_equal(count, want[1]) and count.max() > 90 and (count == 0).sum() > 20
    assert np.array_equal(desc, want[0])
    wide = fpfh_of(clouds, nrm, row_width=64)[0].cpu().numpy()
    assert wide.shape == (len(nrm), 64) and np.array_equal(wide[:, :33], desc) and (wide[:, 33:] == 0).all()
    unit = reg.fpfh_numpy(list(clouds), fc.R_FPFH, nrm, unit=True)[0]
    for width in (33, 64):
        got_unit = fpfh_of(clouds, nrm, row_width=width, unit=True)[0].cpu().numpy()
        assert np.array_equal(got_unit[:, :33], unit) and (got_unit[:, 33:] == 0).all()


@pytest.mark.gpu
def test_fpfh_does_not_depend_on_order_stacking_or_cell_size(terrain):
    clouds, nrm, _, got = terrain
    a, na = clouds[0], len(clouds[0])
    rng = np.random.default_rng(21)
    perm = rng.permutation(na)
    inv = torch.from_numpy(np.argsort(perm)).cuda()
    again = fpfh_of([a[perm]], nrm[:na][perm])
    assert all(torch.equal(x[inv], y[:na]) for x, y in zip(again, got))
    # the same cloud as clouds 0 and 2 around another one that overlaps it in coordinates
    half = rng.permutation(na)[:na // 2]
    other = (a[half].astype(np.float64) + rng.normal(scale=0.05, size=(na // 2, 3))).astype(np.float32)
    three = fpfh_of([a, other, a], np.concatenate([nrm[:na], nrm[:na][half], nrm[:na]]))
    for lo in (0, na + na // 2):
        assert all(torch.equal(x[lo:lo + na], y[:na]) for x, y in zip(three, got))
    mixed = fpfh_of([np.concatenate([a, other])], np.concatenate([nrm[:na], nrm[:na][half]]))
    assert not torch.equal(mixed[2][:na], got[2][:na])
    # a coarser cell list gives the same bits, and so does a second run
    for other_run in (fpfh_of(clouds, nrm, grid_radius=0.3), fpfh_of(clouds, nrm)):
        assert all(torch.equal(x, y) for x, y in zip(other_run, got))


@pytest.mark.gpu
def test_edge_cases_on_the_device():
    cases = fc.edge_cases()
    # every case alone, and all of them stacked as the clouds of one call
    for _, pts, nrm, radius, count, spfh, desc in cases:
        d, c, s = (t.cpu().numpy() for t in fpfh_of([pts], nrm, radius))
        assert np.array_equal(c, count) and np.array_equal(s, spfh) and np.array_equal(d, desc)
    d, c, s = (t.cpu().numpy() for t in fpfh_of([k[1] for k in cases], np.concatenate([k[2] for k in cases]), 0.1))
    assert np.array_equal(c, np.concatenate([k[4] for k in cases]))
    assert np.array_equal(s, np.concatenate([k[5] for k in cases]))
    assert np.array_equal(d, np.concatenate([k[6] for k in cases]))


@pytest.mark.gpu
def test_argument_checks_and_cell_range():
    pts = torch.zeros((4, 3), device="cuda")
    nrm = torch.ones((4, 3), device="cuda")
    with pytest.raises(ValueError):
        ops.fpfh(pts, [4], 0.1, nrm, row_width=32)
    with pytest.raises(ValueError):
        ops.fpfh(pts, [4], 0.1, nrm[:3])
    with pytest.raises(ValueError):
        ops.fpfh(pts, [4], float("inf"), nrm)
    with pytest.raises(RuntimeError):
        ops.fpfh(pts.cpu(), [4], 0.1, nrm)
    # a point whose cell cannot be addressed sets the grid's status word and has no descriptor
    far = torch.tensor([[0.0, 0, 0], [0.05, 0, 0], [1e6, 0, 0]], device="cuda")
    grid = ops.CloudGrid(far, [3], 0.1)
    desc, count = ops.fpfh(grid, None, 0.1, torch.tensor([[0.0, 0, 1]] * 3, device="cuda"))
    assert int(grid.status.word.item()) & 2
    assert count.tolist() == [1, 1, 0] and (desc[2] == 0).all() and (desc[0] != 0).any()


@pytest.mark.gpu
def test_a_neighbourhood_of_thousands():
    """3000 points inside one ball of half the radius: every point is every other's neighbour, far beyond what a cell, a
    lane's bucket or a 16-bit counter would hold."""
    rng = np.random.default_rng(3)
    n, radius = 3000, 0.2
    v = rng.normal(size=(n, 3))
    pts = (0.099 * v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(size=(n, 1)) ** (1 / 3)).astype(np.float32)
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    desc, count, spfh = (t.cpu().numpy() for t in fpfh_of([pts], nrm, radius))
    assert (count == n - 1).all()
    want = reg.fpfh_numpy([pts], radius, nrm, return_spfh=True)
    assert np.array_equal(spfh[:64], want[2][:64]) and np.array_equal(desc[:64], want[0][:64])
    assert np.array_equal(count, want[1])


@pytest.mark.gpu
def test_capture_in_a_graph_and_replay(terrain):
    clouds, nrm, _, got = terrain
    pts = torch.from_numpy(np.concatenate(clouds)).cuda()
    grid = ops.CloudGrid(pts, [len(c) for c in clouds], fc.R_FPFH)
    normals = torch.from_numpy(nrm).cuda()
    run = lambda: ops.fpfh(grid, None, fc.R_FPFH, normals, row_width=64, return_spfh=True)
    run()                                                              # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = run()
    for _ in range(2):
        for t in outs:
            t.fill_(7)                                                 # the replay has to compute it again
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(outs[0][:, :33], got[0]) and bool((outs[0][:, 33:] == 0).all())
        assert torch.equal(outs[1], got[1]) and torch.equal(outs[2], got[2])
    assert int(grid.status.word.item()) == 0


def seeded_scores(counts, seed):
    """The scores of evaluate.generate_fpfh_features: a uniform draw in (0, 1] for a described point, else 0."""
    rng = np.random.default_rng(seed)
    return [np.where(c > 0, 1.0 - rng.random(len(c)), 0.0).astype(np.float32) for c in counts]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", fc.SEEDS)
def test_fpfh_registers_the_terrain_fragments(seed):
    """describe_fpfh -> mutual_nn -> estimate_transform (RANSAC at its defaults) on the two terrain fragments: the
    descriptors and the mutual set are the restatement's bit for bit, and the pose lies within 1 deg / 0.02 m of the
    truth.  Measured on the MI355X: seed 5 -- 489 matches, 102 inliers, 0.51 deg, 0.013 m; seed 6 -- 544 matches, 142
    inliers, 0.32 deg, 0.012 m.  The rotation error is what ~100 matches that are each only within 0.05 m of their true
    partner give a fit over a 1 m patch (0.025 m / (0.4 m sqrt(100)) = 0.36 deg); the translation is measured at the
    frame's origin, so it carries that rotation error times the ~1.8 m from the origin to the overlap."""
    clouds, poses, _, views = fc.scene(seed)
    # (one call per fragment: describe_fpfh takes one viewpoint for all its clouds, and VIEW differs between the frames)
    each = [reg.describe_fpfh([np.array(c)], fc.R_FPFH, fc.R_NORMAL, viewpoint=v) for c, v in zip(clouds, views)]
    descs, counts = [e[0][0] for e in each], [e[1][0] for e in each]
    assert all(d.shape == (len(c), 64) and d.is_cuda for d, c in zip(descs, clouds))
    # the restatement over the normals the device estimated reproduces the descriptors bit for bit ...
    normals = np.concatenate([ops.estimate_normals(torch.from_numpy(np.array(c)).cuda(), [len(c)], fc.R_NORMAL,
                                                   viewpoint=v)[0].cpu().numpy() for c, v in zip(clouds, views)])
    want, want_count = reg.fpfh_numpy(list(clouds), fc.R_FPFH, normals, unit=True)
    na = len(clouds[0])
    assert np.array_equal(torch.cat(descs).cpu().numpy()[:, :33], want)
    assert np.array_equal(torch.cat(counts).cpu().numpy(), want_count)
    # ... and therefore the mutual set
    padded = np.zeros((len(want), 64), dtype=np.float32)
    padded[:, :33] = want
    row, _, mutual = ops.mutual_nn(descs[0].contiguous(), descs[1].contiguous())
    row_w, _, mutual_w = ops.mutual_nn(torch.from_numpy(padded[:na]).cuda(), torch.from_numpy(padded[na:]).cuda())
    assert torch.equal(mutual, mutual_w) and torch.equal(row[mutual.bool()], row_w[mutual_w.bool()])
    assert int(mutual.sum()) > 300
    scores = [torch.from_numpy(s).cuda() for s in seeded_scores([c.cpu().numpy() for c in counts], 0)]
    keypts = [torch.from_numpy(np.array(c)).cuda() for c in clouds]
    T, inliers, matches = reg.estimate_transform(keypts[0], descs[0], scores[0], keypts[1], descs[1], scores[1])
    rot, shift = sc.pose_error(T.cpu().numpy(), sc.gt_transform(poses, 0, 1))
    print("seed %d: %d matches, %d inliers, pose error %.3f deg %.4f m" % (seed, int(matches), int(inliers), rot, shift))
    assert rot < 1.0 and shift < 0.02


@pytest.mark.gpu
def test_register_scene_reads_the_fpfh_dump(tmp_path):
    """generate_fpfh_features -> build_benchmark's gt.log / gt.info -> register_scene(desc_name='FPFH'): the pair of
    terrain fragments is recalled.  Registration recall counts pairs with j - i > 1 only, so a small fragment far from
    both sits between the two."""
    clouds, poses = fc.shifted(SEED)              # generate_fpfh_features turns the normals towards each frame's origin
    away = np.eye(4)
    away[:3, 3] = (100.0, 0.0, 0.0)
    frags = [clouds[0], clouds[1][:200], clouds[1]]
    frag_poses = [poses[0], away @ poses[1], poses[1]]
    save, gtdir = str(tmp_path / "dump"), str(tmp_path / "gt")
    ev.generate_fpfh_features({"terrain": frags}, save, fc.R_FPFH, fc.R_NORMAL, seed=0)
    gt, _, overlap = reg.build_benchmark(frags, frag_poses, gtdir, None, radius=0.05, min_overlap=0.2)
    assert sorted(gt) == ["0_2"], overlap
    recall, precision, errs = reg.register_scene(save, "terrain", gtdir, num_points=2000, desc_name="FPFH")
    print("transformation error of 0_2: %.4g" % errs["0_2"])
    assert recall == 1.0 and precision == 1.0
    assert sorted(ev.loadlog(str(tmp_path / "dump" / "registration" / "terrain"))) == ["0_2"]
    rec = ev.register_one_scene(0.05, 0.05, save, "terrain", gtdir, num_points=2000, desc_name="FPFH")[0]
    assert rec == 100.0
