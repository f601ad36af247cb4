"""GPU: fast global registration (ops.fgr_rigid; csrc/fgr.hip) against its host twin and the NumPy restatement, alone
and in batches, under graph capture, against RANSAC, and through registration.register_scene(estimator='fgr').
Small shapes on purpose: the kernel has ONE path for every count (the rows are streamed), so the counts only have to
cover the strided loop's trips (below, at and above 256, several odd trips)."""
import os

import numpy as np
import pytest
import torch

from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.geometric_registration import evaluate as ev
from d3feat_pytorch_amd.geometric_registration import registration as reg
from test_ransac_gpu import _scene, stack, synthetic_pair
import fgr_cases as fc


def _dev(src, tgt, seg):
    return (torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), torch.from_numpy(seg).cuda().contiguous())


@pytest.mark.gpu
def test_parity_with_the_host_twin():
    counts = (3, 4, 255, 256, 257, 1531, 4099)
    outliers = {256: 0.5, 1531: 0.5, 4099: 0.3}                            # the small sets stay clean
    pairs = [fc.pose_pair(M, outliers.get(M, 0.0), 0.01, 300 + k)[:2] for k, M in enumerate(counts)]
    src, tgt, seg = fc.stack_host(pairs)
    for kw in (dict(seed=9), dict(seed=9, max_tuples=137), dict(tuple_trials=0)):
        d = [x.cpu().numpy() for x in ops.fgr_rigid(*_dev(src, tgt, seg), return_debug=True, **kw)]
        h = [x.numpy() for x in ops.fgr_rigid_host(src, tgt, seg, return_debug=True, **kw)]
        assert np.array_equal(d[5], h[5]), kw                              # multiplicity
        for k in (1, 2, 4):                                                # inliers, tuples, status
            assert np.array_equal(d[k], h[k]), (kw, k, d[k], h[k])
        assert (h[4] == 0).all()
        # the trace localises a disagreement: mu exactly, weight_sum and steps to the bound, iteration by iteration
        assert np.array_equal(d[6][..., 0], h[6][..., 0]), kw
        step = np.abs(d[6][..., 2:] - h[6][..., 2:]).max(axis=(0, 2))
        wsum = (np.abs(d[6][..., 1] - h[6][..., 1]) / np.maximum(1.0, h[6][..., 1])).max(axis=0)
        first = np.nonzero((step > fc.T_BOUND) | (wsum > fc.T_BOUND))[0]
        print("%s: max |T| diff %.3e, max step diff %.3e" % (kw, np.abs(d[0] - h[0]).max(), step.max()))
        assert first.size == 0, "device and host part at iteration %d" % first[0]
        assert np.abs(d[0] - h[0]).max() <= fc.T_BOUND, kw
        assert np.abs(d[3] - h[3]).max() <= 1e-9 * max(1.0, h[3].max())


def _same(a, b):
    """Bit equality that takes the NaN rows of a trace (iterations that did not run) as equal."""
    return torch.equal(torch.nan_to_num(a, nan=-1.0), torch.nan_to_num(b, nan=-1.0))


@pytest.mark.gpu
def test_batching_and_determinism():
    good = [fc.pose_pair(M, 0.3, 0.01, 400 + M)[:2] for M in (300, 700, 257)]
    pairs = [(good[0][0][:0], good[0][1][:0]), (good[0][0][:2], good[0][1][:2]), good[0], good[1],
             (good[0][0][:5], good[0][1][:5]), good[2]]
    src, tgt, seg = fc.stack_host(pairs)
    rows = len(src)
    seg[4] = (rows - 2, 5)                                                # runs past the rows: invalid
    kw = dict(seed=21, max_tuples=300)
    out = ops.fgr_rigid(*_dev(src, tgt, seg), return_debug=True, **kw)
    st = out[4].cpu().numpy()
    assert list(st) == [ops.FGR_ST_FEW, ops.FGR_ST_FEW, 0, 0, ops.FGR_ST_SEGMENT, 0]
    eye = torch.eye(4, dtype=torch.float64, device='cuda')
    for p in (0, 1, 4):
        assert torch.equal(out[0][p], eye) and int(out[1][p]) == 0

    def mult_of(p, mult, sg):
        return mult[int(sg[p, 0]):int(sg[p, 0]) + int(sg[p, 1])]
    # every pair alone, with its own index as the hash index
    for p in range(6):
        if p == 4:
            s1, t1, g1 = src, tgt, seg[p:p + 1].copy()
        else:
            s1, t1, g1 = fc.stack_host([pairs[p]])
            if len(s1) == 0:
                s1, t1 = np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32)
        one = ops.fgr_rigid(*_dev(s1, t1, g1), first_pair=p, return_debug=True, **kw)
        for k in (0, 1, 2, 3, 4, 6):
            assert _same(out[k][p:p + 1], one[k]), (p, k)
        if p != 4:
            assert torch.equal(mult_of(p, out[5], seg), one[5][:int(seg[p, 1])]), p
    # the batch reversed in memory: pair 5's rows first, every pair still at its own index of seg (its hash index)
    order = [5, 3, 2, 1, 0]
    rs, rt, rg = fc.stack_host([pairs[p] for p in order])
    rseg = seg.copy()
    for q, p in enumerate(order):
        rseg[p] = rg[q]
    rseg[4] = (rows - 2, 5)
    pad = np.zeros((rows - len(rs), 3), np.float32)                       # (pair 4's 5 rows: keeps `rows` the same)
    rev = ops.fgr_rigid(*_dev(np.concatenate([rs, pad]), np.concatenate([rt, pad]), rseg), return_debug=True, **kw)
    for k in (0, 1, 2, 3, 4, 6):
        assert _same(out[k], rev[k]), k
    for p in order:
        assert torch.equal(mult_of(p, out[5], seg), mult_of(p, rev[5], rseg)), p
    # ... and the good pairs in another order of the batch, each call naming the hash index of its first pair
    for first, members in ((2, [2, 3]), (5, [5])):
        s1, t1, g1 = fc.stack_host([pairs[p] for p in members])
        part = ops.fgr_rigid(*_dev(s1, t1, g1), first_pair=first, **kw)
        for q, p in enumerate(members):
            for k in range(5):
                assert torch.equal(out[k][p], part[k][q]), (p, k)
    # run to run
    again = ops.fgr_rigid(*_dev(src, tgt, seg), return_debug=True, **kw)
    assert all(_same(a, b) for a, b in zip(out, again))
    # two seeds: other multiplicities with the tuple test on, identical results without it
    other = ops.fgr_rigid(*_dev(src, tgt, seg), return_debug=True, **dict(kw, seed=22))
    assert not torch.equal(other[5], out[5])
    a = ops.fgr_rigid(*_dev(src, tgt, seg), tuple_trials=0, seed=1, return_debug=True)
    b = ops.fgr_rigid(*_dev(src, tgt, seg), tuple_trials=0, seed=2, return_debug=True)
    assert all(_same(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError):
        ops.fgr_rigid(*_dev(src, tgt, seg), iterations=0)
    with pytest.raises(ValueError):
        ops.fgr_rigid(torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda(), torch.from_numpy(seg).cuda().long())


@pytest.mark.gpu
def test_graph_capture_replays_bit_identically():
    sets = [[fc.pose_pair(600, out, 0.01, 500 + 10 * r + k)[:2] for k in range(3)] for r, out in enumerate((0.2, 0.4, 0.5, 0.0))]
    src, tgt, seg = _dev(*fc.stack_host(sets[0]))
    kw = dict(seed=3, max_tuples=200)
    ops.fgr_rigid(src, tgt, seg, **kw)                     # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = ops.fgr_rigid(src, tgt, seg, **kw)
    for r in (1, 2, 3):
        s2, t2, g2 = _dev(*fc.stack_host(sets[r]))
        src.copy_(s2)
        tgt.copy_(t2)
        seg.copy_(g2)
        g.replay()
        torch.cuda.synchronize()
        got = [x.clone() for x in outs]
        want = ops.fgr_rigid(src, tgt, seg, **kw)
        assert all(torch.equal(x, y) for x, y in zip(got, want)), r
        assert (want[4] == 0).all()


@pytest.mark.gpu
def test_recovery_under_outliers():
    """The CPU test's criterion, cases and seeds (fgr_cases.POSE_CASES: 0 / 30 / 50 % outliers); one call per case, so
    that every case is pair 0 of its call as it is there."""
    for case in fc.POSE_CASES:
        M, out, sigma, rng_seed, seed = case
        s, g, T0, good = fc.pose_pair(M, out, sigma, rng_seed)
        seg = np.array([[0, M]], dtype=np.int32)
        T, inl, tup, ws, st = (x.cpu().numpy() for x in ops.fgr_rigid(*_dev(s, g, seg), seed=seed))
        Th = ops.fgr_rigid_host(s, g, seg, seed=seed)[0].numpy()
        assert st[0] == 0 and np.abs(T - Th).max() <= fc.T_BOUND, case
        br, bt = fc.recovery_bounds(s, g, T0, good)
        er, et = fc.pose_errors(T[0], T0)
        print("%s: rot %.3e deg (bound %.3e), trans %.3e m (bound %.3e)" % (case, er, br, et, bt))
        assert er <= br and et <= bt, case


@pytest.mark.gpu
def test_inliers_against_ransac_at_half_outliers():
    rng = np.random.default_rng(31)
    pairs = [synthetic_pair(rng, M, 0.5) for M in (400, 1500, 3000)]
    src, tgt, seg = stack(pairs)
    n = reg.fgr_numpy(src.cpu().numpy(), tgt.cpu().numpy(), seg.cpu().numpy())
    f = [x.cpu().numpy() for x in ops.fgr_rigid(src, tgt, seg)]
    r = [x.cpu().numpy() for x in ops.ransac_rigid(src, tgt, seg)]
    print("inliers: fgr %s, fgr numpy %s, ransac %s" % (f[1], n[1], r[1]))
    assert (f[4] == 0).all() and (r[4] == 0).all()
    assert (n[1] >= 0.9 * r[1]).all()                      # the restatement first
    assert (f[1] >= 0.9 * r[1]).all()
    for p, (_, _, T0) in enumerate(pairs):
        assert fc.pose_errors(f[0][p], T0)[0] < 1.0


def _dump_scene(tmp_path, rng, num_frag=6):
    scene, save = 'synthetic-room', str(tmp_path / 'dump')
    poses, kp, desc, score = _scene(rng, num_frag)
    gt = {'%d_%d' % (i, j): np.linalg.inv(poses[i]) @ poses[j] for i in range(num_frag) for j in range(i + 1, num_frag)}
    dpath, kpath, spath = ev._paths(save, scene)
    for p in (dpath, kpath, spath):
        os.makedirs(p)
    for f in range(num_frag):
        np.save(os.path.join(dpath, 'cloud_bin_%d.D3Feat' % f), desc[f])
        np.save(os.path.join(kpath, 'cloud_bin_%d' % f), kp[f])
        np.save(os.path.join(spath, 'cloud_bin_%d' % f), score[f])
    gtdir = str(tmp_path / 'gt')
    ev.writelog(gtdir, gt, num_frag)
    with open(os.path.join(gtdir, 'gt.info'), 'w') as fh:
        for key in sorted(gt, key=lambda k: tuple(int(x) for x in k.split('_'))):
            i, j = (int(x) for x in key.split('_'))
            I6 = np.zeros((6, 6))
            for q in kp[i][:500].astype(np.float64):
                px = np.array([[0, -q[2], q[1]], [q[2], 0, -q[0]], [-q[1], q[0], 0]])
                J = np.hstack([np.eye(3), -px])
                I6 += J.T @ J
            fh.write('%d\t %d\t %d\t\n' % (i, j, num_frag))
            for r in I6:
                fh.write(''.join(' % .8e\t ' % v for v in r).rstrip(' ') + '\n')
    return scene, save, gtdir, gt, kp, desc, score


@pytest.mark.gpu
def test_register_scene_with_fgr_end_to_end(tmp_path):
    rng = np.random.default_rng(15)        # test_register_scene_end_to_end's scene; the restatement is checked below
    num_frag, k = 6, 1000
    scene, save, gtdir, gt, kp, desc, score = _dump_scene(tmp_path, rng, num_frag)
    keys = sorted(gt, key=lambda kk: tuple(int(x) for x in kk.split('_')))
    info = reg.loadinfo(gtdir)
    # the restatement on the pipeline's own matches meets the benchmark's criterion on every listed pair
    for n, key in enumerate(keys):
        i, j = (int(x) for x in key.split('_'))
        dev = [torch.from_numpy(a).cuda() for a in (kp[i], desc[i], score[i], kp[j], desc[j], score[j])]
        mutual, sp, tp = reg._pair_points(*dev, k)
        m = mutual.bool().cpu().numpy()
        s, g = sp.cpu().numpy()[m], tp.cpu().numpy()[m]
        Tn = reg.fgr_numpy(s, g, [[0, len(s)]], first_pair=n)[0][0]
        assert reg.transformation_error(Tn, gt[key], info[key]) <= 0.04, key
    recall, precision, errs = reg.register_scene(save, scene, gtdir, num_points=k, out_log=str(tmp_path / 'est'),
                                                 estimator='fgr')
    est = ev.loadlog(str(tmp_path / 'est'))
    assert sorted(est) == sorted(gt)
    for key in keys:
        e = reg.transformation_error(est[key], gt[key], info[key])
        assert e <= 0.2 ** 2, (key, e)
    assert recall == 1.0 and precision == 1.0
    # the refinements after the pose estimate run through unchanged
    r2 = reg.register_scene(save, scene, gtdir, num_points=k, out_log=str(tmp_path / 'est_icp'), estimator='fgr',
                            icp=dict(max_distance=0.05))
    assert np.isfinite(r2[0]) and len(ev.loadlog(str(tmp_path / 'est_icp'))) == len(keys)
    r3, poses = reg.register_scene(save, scene, gtdir, num_points=k, out_log=str(tmp_path / 'est_pg'), estimator='fgr',
                                   fgr=dict(iterations=96), pose_graph=dict(max_distance=0.05))
    assert poses.shape == (num_frag, 4, 4) and np.isfinite(poses).all() and np.isfinite(r3[0])
    # estimator='ransac' is the call without the keyword
    kw = dict(num_hypotheses=4000, seed=2)
    a = reg.register_scene(save, scene, gtdir, num_points=k, out_log=str(tmp_path / 'ra'), **kw)
    b = reg.register_scene(save, scene, gtdir, num_points=k, out_log=str(tmp_path / 'rb'), estimator='ransac', **kw)
    assert a[:2] == b[:2] and a[2] == b[2]
    ea, eb = ev.loadlog(str(tmp_path / 'ra')), ev.loadlog(str(tmp_path / 'rb'))
    assert all(np.array_equal(ea[key], eb[key]) for key in keys)


@pytest.mark.gpu
def test_batched_inference_path_with_fgr_matches_single_pair_estimates():
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
    T, inl, n = reg.estimate_transforms_from_match(torch.cat(item), seg, row, mutual, sel, estimator='fgr',
                                                   fgr=dict(seed=4))
    for p in range(2):
        i, j = 2 * p, 2 * p + 1
        o_i, o_j = int(seg[i, 0]), int(seg[j, 0])
        T1, inl1, n1 = reg.estimate_transform(item[i], feats[o_i:o_i + len(kp[i])], scores[o_i:o_i + len(kp[i])],
                                              item[j], feats[o_j:o_j + len(kp[j])], scores[o_j:o_j + len(kp[j])],
                                              num_points=k, estimator='fgr', fgr=dict(seed=4, first_pair=p))
        assert int(n[p]) == int(n1) > 30 and int(inl[p]) == int(inl1)
        assert torch.equal(T[p], T1), p
        Tgt = np.linalg.inv(poses[i]) @ poses[j]
        assert fc.pose_errors(T1.cpu().numpy(), Tgt)[0] < 1.0
    with pytest.raises(ValueError):
        reg.estimate_transforms_from_match(torch.cat(item), seg, row, mutual, sel, estimator='fgr', seed=4)
