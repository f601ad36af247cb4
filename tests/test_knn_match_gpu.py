"""csrc/knn_match.hip against the rule of csrc/knn_match.hpp, bit for bit: on the exact-lattice descriptors of
tests/knn_cases.py every float32 summation order gives the same products, so ``ops.knn_match`` must EQUAL
``registration.knn_match_numpy`` -- indices and distance bits, for every k, no tolerance, no share of rows left out --
with the best columns planted in one lane, across the lanes of a block, astride the column chunks, in the partial last
tile, in improving and worsening order, as distinct products, exact ties, rounding collisions and NaNs
(tests/test_knn_cases_cpu.py proves that they are there and that a wrong rule is seen).  Then slot 0 against
``ops.mutual_nn`` on descriptors that are NOT exact, the batched form, and the ``matches=`` plumbing of registration."""
import functools
import os

import numpy as np
import pytest
import torch

import knn_cases as kc
import matching_cases as mc
from d3feat_pytorch_amd import _native, ops
from d3feat_pytorch_amd.geometric_registration import evaluate as ev
from d3feat_pytorch_amd.geometric_registration import registration as reg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _device(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _host(pair):
    return tuple(x.cpu().numpy() for x in pair)


@functools.lru_cache(maxsize=None)
def _want(C, n, k):
    """The restatement on problem n of kc.problems(C), after asserting that its products are THE products; shared by the
    tests and never written to."""
    p = kc.problems(C)[n]
    mc.exact_products(p.S, p.T, p.bits)
    return reg.knn_match_numpy(p.S, p.T, k)


def _check_all(C, tag=""):
    for n, p in enumerate(kc.problems(C)):
        S, T = _device(p.S), _device(p.T)
        for k in kc.KS:
            got, want = _host(ops.knn_match(S, T, k)), _want(C, n, k)
            assert kc.same(got, want), "k=%d %s %s" % (k, tag, kc.missed(p, got, want))


@pytest.mark.parametrize("C", kc.WIDTHS)
def test_knn_match_equals_the_rule_on_exact_inputs(C):
    _check_all(C)


@pytest.mark.parametrize("wgs", (1, 0, 4096))
def test_knn_match_equals_the_rule_for_any_chunking(wgs):
    """match_wgs = 1: one column chunk; 0 and 4096: three."""
    old = _native.set_tunables(match_wgs=wgs)
    try:
        for C in kc.WIDTHS:
            _check_all(C, "match_wgs=%d" % wgs)
    finally:
        _native.set_tunables(**old)


@pytest.mark.parametrize("C", kc.WIDTHS)
def test_degenerate_shapes(C):
    for k in kc.KS:
        for name, S, T in kc.degenerate(C, k):
            mc.exact_products(S, T, 12)
            got, want = _host(ops.knn_match(_device(S), _device(T), k)), reg.knn_match_numpy(S, T, k)
            assert kc.same(got, want), "C=%d k=%d %s: %s" % (C, k, name, kc.missed(name, got, want))
            assert (got[0][:, len(T):] == -1).all() and np.isposinf(got[1][:, len(T):]).all(), (C, k, name)


@pytest.mark.parametrize("C", kc.WIDTHS)
def test_batched_form_equals_per_pair_calls_and_the_rule(C):
    D, seg, bits = mc.batched(C)
    dD, dseg = _device(D), _device(seg)
    for k in (1, 3, 8):
        idx, dist = _host(ops.knn_match_batched(dD, dD, dseg, mc.NS, mc.NT, k))
        assert idx.shape == (len(D), k) and dist.shape == (len(D), k)
        covered = np.zeros(len(D), bool)
        for (so, sn, to, tn), b in zip(seg.tolist(), bits):
            got = idx[so:so + sn], dist[so:so + sn]
            covered[so:so + sn] = True
            if tn == 0:                                   # an empty target: -1 / +inf in all of the pair's rows
                assert (got[0] == -1).all() and np.isposinf(got[1]).all()
                continue
            S, T = D[so:so + sn], D[to:to + tn]
            mc.exact_products(S, T, b)
            want = reg.knn_match_numpy(S, T, k)
            assert kc.same(got, want), "k=%d pair at %d: %s" % (k, so, kc.missed("batched", got, want))
            assert kc.same(got, _host(ops.knn_match(_device(S), _device(T), k))), (k, so)
        assert (idx[~covered] == -1).all() and np.isposinf(dist[~covered]).all() and (~covered).any()


def test_a_second_launch_gives_identical_tensors():
    p = kc.problem(32, 'collide')
    S, T = _device(p.S), _device(p.T)
    rng = np.random.default_rng(3)
    R = _device(rng.standard_normal((1500, 32)).astype(np.float32))
    R = R / R.norm(dim=1, keepdim=True)
    for a, b, k in ((S, T, 8), (R, R, 5)):
        one, two = ops.knn_match(a, b, k), ops.knn_match(a, b, k)
        assert torch.equal(one[0], two[0]) and torch.equal(one[1].view(torch.int32), two[1].view(torch.int32))


def _unit_rows(rng, n, C):
    x = rng.standard_normal((n, C)).astype(np.float32)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("Ns, Nt, C", [(300, 700, 16), (300, 700, 32), (300, 700, 64), (300, 700, 128), (3000, 5000, 32)])
def test_slot_0_is_mutual_nn_s_row_argmin_on_inexact_descriptors(Ns, Nt, C):
    """Random unit rows: the products are NOT exact, so only a kernel that forms them by the same instruction sequence
    and ranks them by the same rounded distance gives mutual_nn's arg-min in every row.  An equality."""
    rng = np.random.default_rng([Ns, C])
    S, T = _device(_unit_rows(rng, Ns, C)), _device(_unit_rows(rng, Nt, C))
    T[5:9] = S[7]                      # exact ties and near-ties among real-valued rows
    T[40] = S[7]
    row = ops.mutual_nn(S, T)[0]
    for k in (1, 2, 4, 8):
        idx, dist = ops.knn_match(S, T, k)
        assert torch.equal(idx[:, 0], row), "k=%d: %d rows differ" % (k, int((idx[:, 0] != row).sum()))
        key = dist.cpu().numpy()
        key = np.where(np.isnan(key), -np.inf, key)
        assert (key[:, 1:] >= key[:, :-1]).all()
        assert idx[7, :min(k, 5)].tolist() == [5, 6, 7, 8, 40][:k]


# ------------------------------------------------------------------------------------------------ plumbing
NUM_POINTS = 256


@functools.lru_cache(maxsize=None)
def _pair():
    """Exact-lattice descriptors on synthetic keypoints: the source keypoint of a selected row is its nearest target
    keypoint (by descriptor) under a known pose, plus noise.  Returns the arrays and the host-side selection."""
    S, T = kc.plumbing_pair(32)
    mc.exact_products(S, T, 12)
    rng = np.random.default_rng(11)
    s_score, t_score = rng.random(kc.NS).astype(np.float32), rng.random(kc.NT).astype(np.float32)
    si, ti = np.argsort(s_score, kind='stable')[-NUM_POINTS:], np.argsort(t_score, kind='stable')[-NUM_POINTS:]
    t_kp = rng.uniform(-1, 1, (kc.NT, 3)).astype(np.float32)
    w = np.array([0.3, -0.2, 0.5])
    Rm = reg._rodrigues(w)
    t = np.array([0.4, -0.1, 0.25])
    nearest = reg.knn_match_numpy(S[si], T[ti], 1)[0][:, 0]
    s_kp = rng.uniform(-1, 1, (kc.NS, 3)).astype(np.float32)
    s_kp[si] = (t_kp[ti][nearest] @ Rm.T + t + rng.normal(0, 0.003, (NUM_POINTS, 3))).astype(np.float32)
    return S, T, s_kp, t_kp, s_score, t_score, si, ti, Rm, t


def _host_correspondences(matches):
    """(src [n,3], tgt [n,3], slots): what the issue's rule keeps, built on the host from knn_match_numpy."""
    S, T, s_kp, t_kp, _, _, si, ti, _, _ = _pair()
    if 'ratio' in matches:
        idx, dist = reg.knn_match_numpy(S[si], T[ti], 2)
        keep = (idx[:, 1] >= 0) & (dist[:, 0] < np.float32(matches['ratio']) * dist[:, 1])
        return s_kp[si][keep], t_kp[ti][idx[keep, 0]], NUM_POINTS
    K = matches['k']
    idx = reg.knn_match_numpy(S[si], T[ti], K)[0]
    assert (idx >= 0).all()
    keep = np.ones(NUM_POINTS * K, bool)
    if matches.get('mutual'):                 # the column arg-min is the nearest source of a target: the transposed problem
        back = reg.knn_match_numpy(T[ti], S[si], 1)[0][:, 0]
        keep = back[idx.reshape(-1)] == np.repeat(np.arange(NUM_POINTS), K)
        assert 3 <= keep.sum() < keep.size
    return np.repeat(s_kp[si], K, axis=0)[keep], t_kp[ti][idx.reshape(-1)][keep], NUM_POINTS * K


@pytest.mark.parametrize("matches", [dict(k=3), dict(ratio=0.9), dict(k=3, mutual=True)], ids=["k3", "ratio", "k3mutual"])
def test_matches_keyword_hands_sc2_the_host_built_correspondences(matches, tmp_path):
    S, T, s_kp, t_kp, s_score, t_score, si, ti, Rm, t = _pair()
    src, tgt, slots = _host_correspondences(matches)
    assert len(src) >= 3
    seg = torch.tensor([[0, len(src)]], dtype=torch.int32, device=DEV)
    params = dict(reg.SC2_DEFAULTS, max_count=slots)
    wT, winl = ops.sc2_rigid(_device(src), _device(tgt), seg, **params)[:2]
    gT, ginl, gn = reg.estimate_transform(_device(s_kp), _device(S), _device(s_score), _device(t_kp), _device(T),
                                          _device(t_score), num_points=NUM_POINTS, estimator='sc2', matches=matches)
    assert int(gn) == len(src) and int(ginl) == int(winl[0])
    assert torch.equal(gT.view(torch.int64), wT[0].view(torch.int64))
    if matches == dict(k=3):                  # a third of the correspondences are right by construction
        assert int(ginl) >= 0.9 * NUM_POINTS
    assert np.abs(gT.cpu().numpy()[:3, :3] - Rm).max() < 0.01 and np.abs(gT.cpu().numpy()[:3, 3] - t).max() < 0.01
    # the same through register_scene on a two-fragment dump
    save, scene, gtdir = str(tmp_path / 'save'), 'scene', str(tmp_path / 'gt')
    dpath, kpath, spath = ev._paths(save, scene)
    for d in (dpath, kpath, spath):
        os.makedirs(d)
    for i, (kp, desc, score) in enumerate(((s_kp, S, s_score), (t_kp, T, t_score))):
        np.save(os.path.join(kpath, 'cloud_bin_%d.npy' % i), kp)
        np.save(os.path.join(dpath, 'cloud_bin_%d.%s.npy' % (i, ev.DESC_NAME)), desc)
        np.save(os.path.join(spath, 'cloud_bin_%d.npy' % i), score.reshape(-1, 1))
    truth = np.eye(4)
    truth[:3, :3], truth[:3, 3] = Rm, t
    ev.writelog(gtdir, {'0_1': truth}, 2)
    reg.register_scene(save, scene, gtdir, num_points=NUM_POINTS, out_log=str(tmp_path / 'est'), estimator='sc2',
                       matches=matches)
    est = ev.loadlog(str(tmp_path / 'est'))
    assert sorted(est) == ['0_1']
    assert np.allclose(est['0_1'], gT.cpu().numpy(), rtol=2e-8, atol=1e-12)      # (the log holds 9 digits)
    # matches=None is the call without the keyword, bit for bit
    a = reg.estimate_transform(_device(s_kp), _device(S), _device(s_score), _device(t_kp), _device(T), _device(t_score),
                               num_points=NUM_POINTS, estimator='sc2')
    b = reg.estimate_transform(_device(s_kp), _device(S), _device(s_score), _device(t_kp), _device(T), _device(t_score),
                               num_points=NUM_POINTS, estimator='sc2', matches=None)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_infer_step_match_knn_equals_knn_match_batched_on_the_selected_rows():
    from d3feat_pytorch_amd.infer import InferStep
    a, b = kc.problem(32, 'tie'), kc.problem(32, 'collide')
    clouds = [a.S, a.T, b.S[:200], b.T[:150]]                      # pair 1: fewer rows than keypoints asked for
    rng = np.random.default_rng(5)
    item = tuple(_device(rng.uniform(-1, 1, (len(c), 3)).astype(np.float32)) for c in clouds)
    feats = _device(np.concatenate(clouds))
    scores = _device(rng.random(len(feats)).astype(np.float32))
    step = InferStep.__new__(InferStep)                            # match_knn() needs only the device and the item
    step.device = torch.device(DEV)
    kp, k = 256, 3
    idx, dist, sel = step.match_knn(item, feats, scores, kp, k)
    assert idx.shape == (2, kp, k) and dist.shape == (2, kp, k) and sel.shape == (4, kp)
    seg = step.segments(item).cpu().numpy()
    sel_h, sc = sel.cpu().numpy(), scores.cpu().numpy()
    for p in range(2):
        rows = []
        for c in (2 * p, 2 * p + 1):
            off, n = seg[c]
            want_sel = np.argsort(sc[off:off + n], kind='stable')[-kp:]
            assert np.array_equal(sel_h[c][kp - len(want_sel):], want_sel) and (sel_h[c][:kp - len(want_sel)] == -1).all()
            rows.append(off + want_sel)
        F = feats.cpu().numpy()
        want = reg.knn_match_numpy(F[rows[0]], F[rows[1]], k)
        live = len(rows[0])
        got = idx[p].cpu().numpy(), dist[p].cpu().numpy()
        assert kc.same((got[0][kp - live:], got[1][kp - live:]), want), p
        assert (got[0][:kp - live] == -1).all() and np.isposinf(got[1][:kp - live]).all()
        direct = _host(ops.knn_match(_device(F[rows[0]]), _device(F[rows[1]]), k))
        assert kc.same((got[0][kp - live:], got[1][kp - live:]), direct), p
    # the [P,kp,K] tables go straight into the batched estimator entry
    T, inl, n = reg.estimate_transforms_from_match(torch.cat(item), step.segments(item), idx, idx >= 0, sel,
                                                   estimator='sc2')
    assert T.shape == (2, 4, 4) and n.tolist() == [kp * k, 200 * k]
