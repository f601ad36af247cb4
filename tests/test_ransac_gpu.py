"""GPU: batched RANSAC rigid registration (ops.ransac_rigid, geometric_registration.registration) against a NumPy f64
restatement of the whole algorithm with the same counter-based hash (csrc/rigid.hpp)."""
import os

import numpy as np
import pytest
import torch

from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.geometric_registration import evaluate as ev
from d3feat_pytorch_amd.geometric_registration import registration as reg
from test_ransac_cpu import sample_numpy, _rotation

TAU = 0.05
MIN_CROSS2 = 1e-12


# --------------------------------------------------------------------------------------------------- NumPy oracle
def kabsch_batch(S, G):
    """[B,n,3] source / target (f64) -> R [B,3,3], t [B,3] with src ~ R tgt + t (SVD, reflection fix)."""
    cs, ct = S.mean(axis=1), G.mean(axis=1)
    Hm = np.einsum('bia,bic->bac', G - ct[:, None], S - cs[:, None])
    U, _, Vt = np.linalg.svd(Hm)
    d = np.sign(np.linalg.det(np.einsum('bji,bkj->bik', Vt, U)))
    D = np.zeros((len(S), 3, 3))
    D[:, 0, 0] = D[:, 1, 1] = 1.0
    D[:, 2, 2] = d
    R = np.einsum('bji,bjk,blk->bil', Vt, D, U)
    return R, cs - np.einsum('bij,bj->bi', R, ct)


def oracle_hypotheses(src, tgt, H, seed, p, edge_ratio):
    """valid [H], R [H,3,3], t [H,3] (f64) of pair p's hypotheses."""
    n = len(src)
    idx = sample_numpy(seed, p, np.arange(H), n)
    s, g = src[idx].astype(np.float64), tgt[idx].astype(np.float64)          # [H,3,3]
    valid = (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2])
    for pts in (s, g):
        c = np.cross(pts[:, 1] - pts[:, 0], pts[:, 2] - pts[:, 0])
        valid &= (c * c).sum(axis=1) >= MIN_CROSS2
    if edge_ratio > 0:
        edge_ratio = float(np.float32(edge_ratio))              # the kernel's argument is f32
        for i, j in ((0, 1), (1, 2), (2, 0)):
            la2 = ((s[:, i] - s[:, j]) ** 2).sum(axis=1)
            lb2 = ((g[:, i] - g[:, j]) ** 2).sum(axis=1)
            valid &= np.minimum(la2, lb2) >= edge_ratio * edge_ratio * np.maximum(la2, lb2)
    R, t = kabsch_batch(s, g)
    return valid, R, t


def oracle_counts(src, tgt, R, t, chunk=512):
    """f64 inlier counts [H] and the number of correspondences within rounding reach of the threshold [H]."""
    s, g = src.astype(np.float64), tgt.astype(np.float64)
    band = 1e-5 * (1.0 + (s * s).sum(axis=1))
    cnt, near = [], []
    for a in range(0, len(R), chunk):
        d2 = ((np.einsum('hab,nb->hna', R[a:a + chunk], g) + t[a:a + chunk, None] - s) ** 2).sum(axis=2)
        cnt.append((d2 < TAU * TAU).sum(axis=1))
        near.append((np.abs(d2 - TAU * TAU) < band).sum(axis=1))
    return np.concatenate(cnt), np.concatenate(near)


def oracle_ransac(src, tgt, H, seed, p, edge_ratio=0.9, refine_iters=3):
    """(winner h or -1, its count, final T [4,4], final count, per-hypothesis (valid, R, t, count, near))."""
    valid, R, t = oracle_hypotheses(src, tgt, H, seed, p, edge_ratio)
    cnt, near = oracle_counts(src, tgt, R, t)
    if not valid.any():
        return -1, 0, np.eye(4), 0, (valid, R, t, cnt, near)
    score = np.where(valid, cnt, -1)
    h = int(np.argmax(score))                                   # first maximum: ties to the lowest index
    Rc, tc = R[h], t[h]
    s, g = src.astype(np.float64), tgt.astype(np.float64)
    for _ in range(refine_iters + 1):
        inl = (((g @ Rc.T + tc - s) ** 2).sum(axis=1) < TAU * TAU)
        fin = int(inl.sum())
        if _ == refine_iters or fin < 3:
            break
        Rb, tb = kabsch_batch(s[inl][None], g[inl][None])
        Rc, tc = Rb[0], tb[0]
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rc, tc
    return h, int(cnt[h]), T, fin, (valid, R, t, cnt, near)


# -------------------------------------------------------------------------------------------------------- data
def synthetic_pair(rng, M, outliers, sigma=0.01):
    """M correspondences src ~ R0 tgt + t0 (noise sigma) of which a fraction are random outliers; T0 [4,4]."""
    R0 = _rotation(rng)
    t0 = rng.normal(size=3)
    tgt = rng.uniform(-1.5, 1.5, size=(M, 3))
    src = tgt @ R0.T + t0 + rng.normal(scale=sigma, size=(M, 3))
    bad = rng.random(M) < outliers
    src[bad] = rng.uniform(-1.5, 1.5, size=(int(bad.sum()), 3)) @ R0.T + t0
    T0 = np.eye(4)
    T0[:3, :3], T0[:3, 3] = R0, t0
    return src.astype(np.float32), tgt.astype(np.float32), T0


def stack(pairs, dev='cuda'):
    src = np.concatenate([p[0] for p in pairs]) if pairs else np.zeros((0, 3), np.float32)
    tgt = np.concatenate([p[1] for p in pairs])
    offs = np.cumsum([0] + [len(p[0]) for p in pairs])[:-1]
    seg = np.stack([offs, [len(p[0]) for p in pairs]], axis=1).astype(np.int32)
    return (torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev), torch.from_numpy(seg).to(dev).contiguous())


def rot_err_deg(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1.0) / 2.0
    return float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


# ------------------------------------------------------------------------------------------------------- tests
@pytest.mark.gpu
def test_per_hypothesis_parity_with_the_oracle():
    rng = np.random.default_rng(11)
    pairs = [synthetic_pair(rng, M, 0.6) for M in (3, 700, 2000)]
    H, seed = 4096, 1234
    src, tgt, seg = stack(pairs)
    T, inl, bh, bc, st, hc, hr = ops.ransac_rigid(src, tgt, seg, num_hypotheses=H, distance_threshold=TAU,
                                                  edge_ratio=0.9, refine_iters=3, seed=seed, return_hypotheses=True)
    hc, hr, bh, bc = hc.cpu().numpy(), hr.cpu().numpy(), bh.cpu().numpy(), bc.cpu().numpy()
    exceptions = 0
    for p, (s, g, _) in enumerate(pairs):
        h, c, _, _, (valid, R, t, cnt, near) = oracle_ransac(s, g, H, seed, p)
        assert np.array_equal(hc[p] >= 0, valid), p
        v = np.nonzero(valid)[0]
        assert np.abs(hr[p, v, :9].reshape(-1, 3, 3) - R[v]).max(initial=0) < 1e-4, p
        assert np.abs(hr[p, v, 9:] - t[v]).max(initial=0) < 1e-4, p
        assert (hr[p, ~valid] == 0).all()
        diff = np.abs(hc[p, v] - cnt[v])
        assert (diff <= near[v]).all(), "a count difference no near-threshold correspondence explains"
        exceptions += int((diff > 0).sum())
        assert bh[p] == h and (h < 0 or bc[p] == c), (p, bh[p], h, bc[p], c)
    assert exceptions == 0
    assert valid.sum() > 100                             # the data exercises the scoring (M = 2000 pair)


@pytest.mark.gpu
def test_recovery_under_outliers():
    rng = np.random.default_rng(12)
    pairs = [synthetic_pair(rng, 1500, f) for f in (0.5, 0.8, 0.95)]
    H, seed = 50000, 7
    src, tgt, seg = stack(pairs)
    T, inl, bh, bc, st = ops.ransac_rigid(src, tgt, seg, num_hypotheses=H, distance_threshold=TAU, seed=seed)
    T, inl, bh, st = T.cpu().numpy(), inl.cpu().numpy(), bh.cpu().numpy(), st.cpu().numpy()
    assert (st == 0).all()
    for p, (s, g, T0) in enumerate(pairs):
        h, _, To, fin, _ = oracle_ransac(s, g, H, seed, p)
        assert rot_err_deg(T[p, :3, :3], T0[:3, :3]) < 1.0, p
        assert np.linalg.norm(T[p, :3, 3] - T0[:3, 3]) < 0.02, p
        assert bh[p] == h and inl[p] == fin, (p, bh[p], h, inl[p], fin)
        assert np.abs(T[p] - To).max() < 1e-6, p
        assert abs(np.linalg.det(T[p, :3, :3]) - 1.0) < 1e-9 and np.array_equal(T[p, 3], [0, 0, 0, 1])


@pytest.mark.gpu
def test_batching_edge_cases_and_determinism():
    rng = np.random.default_rng(13)
    good = [synthetic_pair(rng, M, 0.7) for M in (400, 900)]
    line = np.zeros((50, 3), np.float32)
    line[:, 0] = np.arange(50, dtype=np.float32) * 0.125          # collinear: every triangle is degenerate
    few = [(good[0][0][:n], good[0][1][:n]) for n in (0, 1, 2)]
    pairs = [(p[0], p[1]) for p in good] + few + [(line, line.copy())]
    src, tgt, seg = stack(pairs)
    kw = dict(num_hypotheses=3000, distance_threshold=TAU, seed=99)
    out = ops.ransac_rigid(src, tgt, seg, **kw)
    T, inl, bh, bc, st = (x.cpu().numpy() for x in out)
    assert list(st) == [0, 0, 1, 1, 1, 2]
    for p in range(2, 6):
        assert np.array_equal(T[p], np.eye(4)) and bh[p] == -1 and inl[p] == 0
    # P pairs in one call == P single-pair calls (each passing its pair index to the hash)
    for p in range(len(pairs)):
        s1, t1, g1 = stack([pairs[p]])
        one = ops.ransac_rigid(s1, t1, g1, first_pair=p, **kw)
        for a, b in zip(out, one):
            assert torch.equal(a[p:p + 1], b), p
    # same seed: bit-identical; another seed: other winners
    again = ops.ransac_rigid(src, tgt, seg, **kw)
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    other = ops.ransac_rigid(src, tgt, seg, **dict(kw, seed=100))
    assert not torch.equal(other[2][:2], out[2][:2])
    # edge_ratio = 0 turns the edge check off: validity exactly as the oracle says
    s, g = good[1][0], good[1][1]
    s1, t1, g1 = stack([(s, g)])
    for er in (0.0, 0.9):
        hc = ops.ransac_rigid(s1, t1, g1, num_hypotheses=2048, edge_ratio=er, seed=5, return_hypotheses=True)[5]
        valid = oracle_hypotheses(s, g, 2048, 5, 0, er)[0]
        assert np.array_equal(hc[0].cpu().numpy() >= 0, valid), er
    v0 = (ops.ransac_rigid(s1, t1, g1, num_hypotheses=2048, edge_ratio=0.0, seed=5, return_hypotheses=True)[5] >= 0)
    v9 = (ops.ransac_rigid(s1, t1, g1, num_hypotheses=2048, edge_ratio=0.9, seed=5, return_hypotheses=True)[5] >= 0)
    assert int(v0.sum()) > int(v9.sum()) and bool((v0 | ~v9).all())
    with pytest.raises(ValueError):
        ops.ransac_rigid(src, tgt, seg, num_hypotheses=0)
    with pytest.raises(ValueError):
        ops.ransac_rigid(src, tgt, seg.long())


@pytest.mark.gpu
def test_graph_capture_replays_bit_identically():
    rng = np.random.default_rng(14)
    a = [synthetic_pair(rng, 800, 0.7) for _ in range(3)]
    b = [synthetic_pair(rng, 800, 0.8) for _ in range(3)]
    src, tgt, seg = stack(a)
    kw = dict(num_hypotheses=5000, distance_threshold=TAU, seed=3)
    ops.ransac_rigid(src, tgt, seg, **kw)                  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = ops.ransac_rigid(src, tgt, seg, **kw)
    s2, t2, g2 = stack(b)
    src.copy_(s2)
    tgt.copy_(t2)
    seg.copy_(g2)
    g.replay()
    torch.cuda.synchronize()
    want = ops.ransac_rigid(src, tgt, seg, **kw)
    assert all(torch.equal(x, y) for x, y in zip(outs, want))
    assert (want[4] == 0).all()


def _scene(rng, num_frag=6, n_world=6000, n_frag=3000):
    world = rng.uniform(0, 2, size=(n_world, 3))
    wdesc = rng.normal(size=(n_world, 32))
    wdesc /= np.linalg.norm(wdesc, axis=1, keepdims=True)
    wscore = rng.permutation(n_world).astype(np.float32) / n_world
    poses = [np.eye(4)]
    for _ in range(num_frag - 1):
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = _rotation(rng), rng.normal(size=3)
        poses.append(T)
    kp, desc, score = [], [], []
    for f in range(num_frag):
        ids = rng.permutation(n_world)[:n_frag]
        inv = np.linalg.inv(poses[f])
        kp.append((world[ids] @ inv[:3, :3].T + inv[:3, 3] + rng.normal(scale=0.005, size=(n_frag, 3)))
                  .astype(np.float32))
        d = wdesc[ids] + rng.normal(scale=0.08, size=(n_frag, 32))
        desc.append((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32))
        score.append(wscore[ids][:, None])
    return poses, kp, desc, score


@pytest.mark.gpu
def test_register_scene_end_to_end(tmp_path):
    rng = np.random.default_rng(15)
    num_frag, scene, save = 6, 'synthetic-room', str(tmp_path / 'dump')
    poses, kp, desc, score = _scene(rng, num_frag)
    gt = {'%d_%d' % (i, j): np.linalg.inv(poses[i]) @ poses[j] for i in range(num_frag) for j in range(i + 1, num_frag)}
    useless = np.eye(4)
    useless[:3, :3], useless[:3, 3] = _rotation(rng), rng.normal(size=3)
    gt['1_4'] = useless                                     # a listed pair whose ground truth is wrong
    dpath, kpath, spath = ev._paths(save, scene)
    for p in (dpath, kpath, spath):
        os.makedirs(p)
    for f in range(num_frag):
        np.save(os.path.join(dpath, 'cloud_bin_%d.D3Feat' % f), desc[f])
        np.save(os.path.join(kpath, 'cloud_bin_%d' % f), kp[f])
        np.save(os.path.join(spath, 'cloud_bin_%d' % f), score[f])
    gtdir = str(tmp_path / 'gt')
    ev.writelog(gtdir, gt, num_frag)
    info = {}
    with open(os.path.join(gtdir, 'gt.info'), 'w') as fh:
        for key in sorted(gt, key=lambda k: tuple(int(x) for x in k.split('_'))):
            i, j = (int(x) for x in key.split('_'))
            I6 = np.zeros((6, 6))
            for q in kp[i][:500].astype(np.float64):
                px = np.array([[0, -q[2], q[1]], [q[2], 0, -q[0]], [-q[1], q[0], 0]])
                J = np.hstack([np.eye(3), -px])
                I6 += J.T @ J
            info[key] = I6
            fh.write('%d\t %d\t %d\t\n' % (i, j, num_frag))
            for r in I6:
                fh.write(''.join(' % .8e\t ' % v for v in r).rstrip(' ') + '\n')
    k = 1000
    kw = dict(num_hypotheses=20000, distance_threshold=0.05, seed=0)
    recall, precision, errs = reg.register_scene(save, scene, gtdir, num_points=k, out_log=str(tmp_path / 'est'), **kw)
    est = ev.loadlog(str(tmp_path / 'est'))
    assert sorted(est) == sorted(gt)
    far = [key for key in gt if int(key.split('_')[1]) - int(key.split('_')[0]) > 1]
    for key in far:
        if key == '1_4':
            assert errs[key] > 0.04
        else:
            assert errs[key] <= 0.04, (key, errs[key])
    # oracle: the pipeline's own matches (keypoint top-k + mutual NN, tested elsewhere), RANSAC restated in NumPy
    good, oracle_est = 0, {}
    keys = sorted(gt, key=lambda kk: tuple(int(x) for x in kk.split('_')))
    for n, key in enumerate(keys):
        i, j = (int(x) for x in key.split('_'))
        dev = [torch.from_numpy(a).cuda() for a in (kp[i], desc[i], score[i], kp[j], desc[j], score[j])]
        mutual, sp, tp = reg._pair_points(*dev, k)
        m = mutual.bool().cpu().numpy()
        s, g = sp.cpu().numpy()[m], tp.cpu().numpy()[m]
        oracle_est[key] = oracle_ransac(s, g, kw['num_hypotheses'], 0, n)[2]
    o_recall, o_precision, o_errs = reg.evaluate_registration(oracle_est, gt, info)
    assert (recall, precision) == (o_recall, o_precision)
    assert recall == (len(far) - 1) / len(far) and precision == recall
    for key in far:
        assert np.abs(est[key] - oracle_est[key]).max() < 1e-4, key


@pytest.mark.gpu
def test_batched_inference_path_matches_single_pair_estimates():
    """InferStep.match -> estimate_transforms_from_match on a 2-pair stacked item == estimate_transform per pair."""
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
    kw = dict(num_hypotheses=8000, seed=4)
    T, inl, n = reg.estimate_transforms_from_match(torch.cat(item), seg, row, mutual, sel, **kw)
    for p in range(2):
        i, j = 2 * p, 2 * p + 1
        o_i, o_j = int(seg[i, 0]), int(seg[j, 0])
        T1, inl1, n1 = reg.estimate_transform(item[i], feats[o_i:o_i + len(kp[i])], scores[o_i:o_i + len(kp[i])],
                                              item[j], feats[o_j:o_j + len(kp[j])], scores[o_j:o_j + len(kp[j])],
                                              num_points=k, first_pair=p, **kw)
        assert int(n[p]) == int(n1) > 30 and int(inl[p]) == int(inl1)
        assert torch.equal(T[p], T1), p
        Tgt = np.linalg.inv(poses[i]) @ poses[j]
        assert rot_err_deg(T1.cpu().numpy()[:3, :3], Tgt[:3, :3]) < 1.0
