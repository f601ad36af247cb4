"""GPU: the spatial-compatibility estimator (ops.sc2_rigid; csrc/sc2.hip) against its host twin and the NumPy
restatement, alone and in batches, with a poisoned workspace, under graph capture, at 3 % inliers beside RANSAC and
FGR, and through registration.register_scene(estimator='sc2').  Small shapes on purpose: the counts cover one, two and
many 64-bit words per row, the 32-row strips of the matrix kernel and the 256-thread strides (sc2_cases.COUNTS)."""
import numpy as np
import pytest
import torch

from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.geometric_registration import evaluate as ev
from d3feat_pytorch_amd.geometric_registration import registration as reg
from test_ransac_gpu import _scene, stack, synthetic_pair
from test_fgr_gpu import _dump_scene
import fgr_cases as fc
import sc2_cases as sc

NAMES = ('T', 'inliers', 'best_seed', 'best_count', 'status', 'degree', 'seed_rows', 'consensus', 'hyp_count', 'hyp_rt',
         'matrix')


def _dev(src, tgt, seg):
    return (torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), torch.from_numpy(seg).cuda().contiguous())


@pytest.fixture(scope='module')
def parity_batch():
    """COUNTS stacked in one batch, and the host twin's outputs per setting (computed once, never changed)."""
    src, tgt, seg = fc.stack_host(sc.parity_pairs())
    host = {s: [x.numpy() for x in ops.sc2_rigid_host(src, tgt, seg, num_seeds=s[0], set_size=s[1], return_debug=True)]
            for s in sc.SETTINGS}
    return src, tgt, seg, host


def _assert_equal_to_host(d, h, what):
    for k in range(1, 9):                                   # every integer output
        assert np.array_equal(d[k], h[k]), (what, NAMES[k])
    assert np.array_equal(d[10], h[10]), (what, 'matrix')
    # the f32 images of the hypotheses: the fit is f64 on both sides, so the images differ by one f32 step at the most
    assert (np.abs(d[9] - h[9]) <= 2.0 ** -22 * np.maximum(1.0, np.abs(h[9]))).all(), what
    print("%s: max |T| diff %.3e, hyp_rt differs in %d entries" % (what, np.abs(d[0] - h[0]).max(), (d[9] != h[9]).sum()))
    assert np.abs(d[0] - h[0]).max() <= sc.T_BOUND, what


@pytest.mark.gpu
@pytest.mark.parametrize("setting", sc.SETTINGS, ids=lambda s: "seeds%d-set%d" % s)
def test_parity_with_the_host_twin(parity_batch, setting):
    src, tgt, seg, host = parity_batch
    d = [x.cpu().numpy() for x in ops.sc2_rigid(*_dev(src, tgt, seg), num_seeds=setting[0], set_size=setting[1],
                                                return_debug=True)]
    h = host[setting]
    assert (h[4] == 0).all() and (h[1] >= 3).all()
    for p, M in enumerate(sc.COUNTS):                       # the matrix is what its definition says
        sc.unpack_rows(d[10][p], M)
    _assert_equal_to_host(d, h, setting)


@pytest.mark.gpu
def test_a_poisoned_workspace_changes_no_bit(parity_batch):
    src, tgt, seg, host = parity_batch
    setting = sc.SETTINGS[0]
    kw = dict(num_seeds=setting[0], set_size=setting[1], return_debug=True)
    clean = ops.sc2_rigid(*_dev(src, tgt, seg), **kw)
    dirty = ops.sc2_rigid(*_dev(src, tgt, seg), _poison_ws=True, **kw)
    for k, (a, b) in enumerate(zip(clean, dirty)):
        assert torch.equal(a, b), NAMES[k]
    _assert_equal_to_host([x.cpu().numpy() for x in dirty], host[setting], 'poisoned')


@pytest.mark.gpu
def test_batching_and_determinism():
    good = [fc.pose_pair(M, 0.3, 0.01, 400 + M)[:2] for M in (300, 700, 257)]
    pairs = [(good[0][0][:0], good[0][1][:0]), (good[0][0][:2], good[0][1][:2]), good[0], good[1],
             (good[0][0][:5], good[0][1][:5]), good[2]]
    src, tgt, seg = fc.stack_host(pairs)
    rows = len(src)
    seg[4] = (rows - 2, 5)                                                # runs past the rows: invalid
    kw = dict(num_seeds=48, set_size=12, max_count=700, return_debug=True)
    out = ops.sc2_rigid(*_dev(src, tgt, seg), **kw)
    st = out[4].cpu().numpy()
    assert list(st) == [ops.SC2_ST_FEW, ops.SC2_ST_FEW, 0, 0, ops.SC2_ST_SEGMENT, 0]
    eye = torch.eye(4, dtype=torch.float64, device='cuda')
    for p in (0, 1, 4):
        assert torch.equal(out[0][p], eye) and int(out[1][p]) == 0 and int(out[2][p]) == -1
    per_pair = (0, 1, 2, 3, 4, 6, 7, 8, 9, 10)

    def degree_of(p, deg, sg):
        return deg[int(sg[p, 0]):int(sg[p, 0]) + int(sg[p, 1])]
    # every pair alone
    for p in range(6):
        if p == 4:
            s1, t1, g1 = src, tgt, seg[p:p + 1].copy()
        else:
            s1, t1, g1 = fc.stack_host([pairs[p]])
            if len(s1) == 0:
                s1, t1 = np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32)
        one = ops.sc2_rigid(*_dev(s1, t1, g1), **kw)
        for k in per_pair:
            assert torch.equal(out[k][p:p + 1], one[k]), (p, NAMES[k])
        if p != 4:
            assert torch.equal(degree_of(p, out[5], seg), one[5][:int(seg[p, 1])]), p
    # the batch reversed in memory: pair 5's rows first, every pair still at its own index of seg
    order = [5, 3, 2, 1, 0]
    rs, rt, rg = fc.stack_host([pairs[p] for p in order])
    rseg = seg.copy()
    for q, p in enumerate(order):
        rseg[p] = rg[q]
    rseg[4] = (rows - 2, 5)
    pad = np.zeros((rows - len(rs), 3), np.float32)                       # (pair 4's 5 rows: keeps `rows` the same)
    rev = ops.sc2_rigid(*_dev(np.concatenate([rs, pad]), np.concatenate([rt, pad]), rseg), **kw)
    for k in per_pair:
        assert torch.equal(out[k], rev[k]), NAMES[k]
    for p in order:
        assert torch.equal(degree_of(p, out[5], seg), degree_of(p, rev[5], rseg)), p
    # run to run
    again = ops.sc2_rigid(*_dev(src, tgt, seg), **kw)
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    # three slices of seg against the one call
    lib = ops._native.lib()
    two = lib.d3f_sc2_rigid_ws_bytes(2, 700, 48)
    assert lib.d3f_sc2_rigid_ws_bytes(3, 700, 48) > two
    sliced = ops.sc2_rigid(*_dev(src, tgt, seg), max_bytes=two, **kw)
    for k, (a, b) in enumerate(zip(out, sliced)):
        assert torch.equal(a, b), NAMES[k]
    with pytest.raises(ValueError):                                       # one pair alone does not fit
        ops.sc2_rigid(*_dev(src, tgt, seg), max_bytes=lib.d3f_sc2_rigid_ws_bytes(1, 700, 48) - 1, **kw)
    with pytest.raises(ValueError):
        ops.sc2_rigid(*_dev(src, tgt, seg), set_size=2)
    with pytest.raises(ValueError):
        ops.sc2_rigid(torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), torch.from_numpy(seg).cuda().long())


@pytest.mark.gpu
def test_graph_capture_replays_bit_identically():
    sets = [[fc.pose_pair(600, out, 0.01, 500 + 10 * r + k)[:2] for k in range(3)] for r, out in enumerate((0.2, 0.4, 0.5, 0.0))]
    src, tgt, seg = _dev(*fc.stack_host(sets[0]))
    kw = dict(num_seeds=32, max_count=600)
    ops.sc2_rigid(src, tgt, seg, **kw)                     # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = ops.sc2_rigid(src, tgt, seg, **kw)
    for r in (1, 2, 3):
        s2, t2, g2 = _dev(*fc.stack_host(sets[r]))
        src.copy_(s2)
        tgt.copy_(t2)
        seg.copy_(g2)
        g.replay()
        torch.cuda.synchronize()
        got = [x.clone() for x in outs]
        want = ops.sc2_rigid(src, tgt, seg, **kw)
        assert all(torch.equal(x, y) for x, y in zip(got, want)), r
        assert (want[4] == 0).all()


@pytest.mark.gpu
def test_recovery_under_outliers():
    """The CPU tests' criteria and inputs: fgr_cases.POSE_CASES at num_seeds=64 within fgr_cases.recovery_bounds, and
    sc2_cases.LOW_INLIER (3 % inliers) within 1 degree / 5 cm; each set stacked into one call."""
    cases = [fc.pose_pair(M, out, sigma, rng_seed) for M, out, sigma, rng_seed, _ in fc.POSE_CASES]
    src, tgt, seg = fc.stack_host([c[:2] for c in cases])
    T, inl, bs, bc, st = (x.cpu().numpy() for x in ops.sc2_rigid(*_dev(src, tgt, seg), num_seeds=64, max_count=1531))
    Th = ops.sc2_rigid_host(src, tgt, seg, num_seeds=64, max_count=1531)[0].numpy()
    assert (st == 0).all() and np.abs(T - Th).max() <= sc.T_BOUND
    for p, (s, g, T0, good) in enumerate(cases):
        br, bt = fc.recovery_bounds(s, g, T0, good)
        er, et = fc.pose_errors(T[p], T0)
        print("%s: rot %.3e deg (bound %.3e), trans %.3e m (bound %.3e)" % (fc.POSE_CASES[p], er, br, et, bt))
        assert er <= br and et <= bt, fc.POSE_CASES[p]
    low = [fc.pose_pair(*c) for c in sc.LOW_INLIER]
    src, tgt, seg = fc.stack_host([c[:2] for c in low])
    T, inl, bs, bc, st = (x.cpu().numpy() for x in ops.sc2_rigid(*_dev(src, tgt, seg), max_count=1500))
    assert (st == 0).all()
    for p, (s, g, T0, good) in enumerate(low):
        er, et = fc.pose_errors(T[p], T0)
        print("%s: %d true inliers, rot %.3f deg, trans %.4f m, inliers %d" % (sc.LOW_INLIER[p], good.sum(), er, et, inl[p]))
        assert er < sc.ROT_OK_DEG and et < sc.TRANS_OK, sc.LOW_INLIER[p]


@pytest.mark.gpu
def test_three_per_cent_inliers_beside_ransac_and_fgr():
    rng = np.random.default_rng(41)
    pairs = [synthetic_pair(rng, 1500, 0.97) for _ in range(3)]
    src, tgt, seg = stack(pairs)
    n = reg.sc2_numpy(src.cpu().numpy(), tgt.cpu().numpy(), seg.cpu().numpy(), max_count=1500)
    c = [x.cpu().numpy() for x in ops.sc2_rigid(src, tgt, seg, max_count=1500)]
    r = [x.cpu().numpy() for x in ops.ransac_rigid(src, tgt, seg)]
    f = [x.cpu().numpy() for x in ops.fgr_rigid(src, tgt, seg)]
    print("inliers: sc2 %s, sc2 numpy %s, ransac %s, fgr %s" % (c[1], n[1], r[1], f[1]))
    for p, (_, _, T0) in enumerate(pairs):                 # the restatement first
        assert n[4][p] == 0 and fc.pose_errors(n[0][p], T0)[0] < 1.0, p
    for p, (_, _, T0) in enumerate(pairs):
        assert c[4][p] == 0 and fc.pose_errors(c[0][p], T0)[0] < 1.0, p


@pytest.mark.gpu
def test_register_scene_with_sc2_end_to_end(tmp_path):
    rng = np.random.default_rng(15)        # test_register_scene_end_to_end's scene
    num_frag, k = 6, 1000
    scene, save, gtdir, gt, kp, desc, score = _dump_scene(tmp_path, rng, num_frag)
    keys = sorted(gt, key=lambda kk: tuple(int(x) for x in kk.split('_')))
    info = reg.loadinfo(gtdir)
    recall, precision, errs = reg.register_scene(save, scene, gtdir, num_points=k, out_log=str(tmp_path / 'est'),
                                                 estimator='sc2')
    est = ev.loadlog(str(tmp_path / 'est'))
    assert sorted(est) == sorted(gt)
    for key in keys:
        e = reg.transformation_error(est[key], gt[key], info[key])
        assert e <= 0.2 ** 2, (key, e)
    assert recall == 1.0 and precision == 1.0
    # the refinements after the pose estimate run through unchanged
    r2 = reg.register_scene(save, scene, gtdir, num_points=k, out_log=str(tmp_path / 'est_icp'), estimator='sc2',
                            icp=dict(max_distance=0.05))
    assert np.isfinite(r2[0]) and len(ev.loadlog(str(tmp_path / 'est_icp'))) == len(keys)
    r3, poses = reg.register_scene(save, scene, gtdir, num_points=k, out_log=str(tmp_path / 'est_pg'), estimator='sc2',
                                   sc2=dict(num_seeds=64), pose_graph=dict(max_distance=0.05))
    assert poses.shape == (num_frag, 4, 4) and np.isfinite(poses).all() and np.isfinite(r3[0])
    # estimator='ransac' is the call without the keyword
    kw = dict(num_hypotheses=4000, seed=2)
    a = reg.register_scene(save, scene, gtdir, num_points=k, out_log=str(tmp_path / 'ra'), **kw)
    b = reg.register_scene(save, scene, gtdir, num_points=k, out_log=str(tmp_path / 'rb'), estimator='ransac', **kw)
    assert a[:2] == b[:2] and a[2] == b[2]
    ea, eb = ev.loadlog(str(tmp_path / 'ra')), ev.loadlog(str(tmp_path / 'rb'))
    assert all(np.array_equal(ea[key], eb[key]) for key in keys)


@pytest.mark.gpu
def test_batched_inference_path_with_sc2_matches_single_pair_estimates():
    from d3feat_pytorch_amd.infer import InferStep
    rng = np.random.default_rng(16)
    poses, kp, desc, score = _scene(rng, 4, n_world=4000, n_frag=1500)
    item = tuple(torch.from_numpy(k).cuda() for k in kp)
    feats = torch.from_numpy(np.concatenate(desc)).cuda()
    scores = torch.from_numpy(np.concatenate(score)).cuda()
    k = 600
    step = InferStep.__new__(InferStep)                     # match() needs only the device and the item
    step.device = torch.device('cuda')
    seg = step.segments(item)
    row, mutual, sel = step.match(item, feats, scores, num_points=k)
    T, inl, n = reg.estimate_transforms_from_match(torch.cat(item), seg, row, mutual, sel, estimator='sc2',
                                                   sc2=dict(num_seeds=64))
    for p in range(2):
        i, j = 2 * p, 2 * p + 1
        o_i, o_j = int(seg[i, 0]), int(seg[j, 0])
        T1, inl1, n1 = reg.estimate_transform(item[i], feats[o_i:o_i + len(kp[i])], scores[o_i:o_i + len(kp[i])],
                                              item[j], feats[o_j:o_j + len(kp[j])], scores[o_j:o_j + len(kp[j])],
                                              num_points=k, estimator='sc2', sc2=dict(num_seeds=64))
        assert int(n[p]) == int(n1) > 30 and int(inl[p]) == int(inl1)
        assert torch.equal(T[p], T1), p
        Tgt = np.linalg.inv(poses[i]) @ poses[j]
        assert fc.pose_errors(T1.cpu().numpy(), Tgt)[0] < 1.0
    with pytest.raises(ValueError):
        reg.estimate_transforms_from_match(torch.cat(item), seg, row, mutual, sel, estimator='sc2', seed=4)
