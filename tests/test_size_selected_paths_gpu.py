"""GPU: kernels whose code path is chosen by size, channel count or pointer alignment, on the paths the rest of the
suite never takes -- each against the project's own oracle (oracle/ops_ref.py, utils.loss in f64, torch.optim,
torch.nn.functional.batch_norm in f64):

A. csrc/loss.hip  loss_fwd_kernel / loss_bwd_kernel: the one-workgroup circle + detector loss that runs
   whenever cache_ok(M, C) = (M <= 128 && C <= 64) fails (every other test has M <= 128, C = 32: the tiled kernels).
B. csrc/loss.hip  contrastive_fwd_kernel / contrastive_bwd_kernel past one 64-channel chunk (acc[1..3], a partly filled
   last chunk) and past two 64-row ballot rounds, one round carrying many hits.
C. csrc/optimizer.hip  nonfinite_kernel / sgd_kernel / adam_kernel at a length where the launch is capped at 2048
   blocks: the 4-way unrolled round, the remainder rounds and the scalar tail all run, as they do on the 24.3 M
   parameters of the real model (the largest other optimizer test, n = 100003, needs 98 blocks: one round, no unroll).
D. csrc/pool.hip  the scalar kernels at C % 4 == 0 (taken only when a pointer is not 16-byte aligned) and ``width``
   against the oracle on the narrower table it stands for, in the plain, the _v4 and the grouped branch.
E. csrc/batchnorm.hip  bn_bwd_sum_kernel / bn_bwd_apply_kernel on a capacity buffer with ``n_live``.

Left out on purpose: the 64-bit-index kernels max_pool_bwd_kernel / closest_pool_bwd_kernel (and the `small == false`
forwards) need a matrix of 2^31 or more elements, 8 GiB or more each; no test allocates that.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from d3feat_pytorch_amd import ops
from oracle import ops_ref
from test_adam_contrastive_gpu import _check, _hyper, _inputs, _oracle
from util import rel_err

DEV = "cuda:0"
BWD_TOL = 2e-4          # test_gpu_ops.BWD_TOL
pytestmark = pytest.mark.gpu


def cu(a):
    return torch.as_tensor(a).to(DEV)


def _max_with_factor_4(existing, measured):
    """Bound of an M = 1024 case: the existing tolerance, or 4 x the error the SAME oracle makes in f32 against itself
    in f64 (computed by the case on the CPU, figures recorded in its docstring), whichever is larger -- the factor 4 is the margin for a
    different, equally valid summation order."""
    return {k: max(existing[k], 4.0 * measured[k]) for k in existing}


# ================================================================================================================
# A. circle + detector loss, one-workgroup kernels
# ================================================================================================================
def _circle_inputs(m, c):
    """The data of test_gpu_ops.test_circle_det_loss at any (M, C)."""
    rng = np.random.default_rng(1000 * m + c)
    a = rng.normal(size=(m, c)).astype(np.float32)
    p = (a + 0.3 * rng.normal(size=(m, c))).astype(np.float32)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    kp = rng.random((m, 3))
    dk = np.linalg.norm(kp[:, None] - kp[None], axis=-1)  # float64 like scipy cdist
    sa, sp = rng.random((m, 1)).astype(np.float32), rng.random((m, 1)).astype(np.float32)
    return a, p, dk, sa, sp


def _circle_oracle(a, p, dk, sa, sp, dtype=torch.float64):
    """ops_ref.circle_loss + ops_ref.det_loss on the CPU in ``dtype``, loss = 1.0 desc + 0.7 det, with autograd."""
    ta, tp, tsa, tsp = (torch.tensor(v, dtype=dtype, requires_grad=True) for v in (a, p, sa, sp))
    loss, acc, fp, an, dists = ops_ref.circle_loss(ta, tp, torch.from_numpy(dk))
    det = ops_ref.det_loss(dists, tsa, tsp)
    (1.0 * loss + 0.7 * det).backward()
    out = {'loss': loss, 'det': det, 'acc': acc, 'dists': dists, 'fp': fp, 'an': an, 'g_anchor': ta.grad,
           'g_positive': tp.grad, 'g_anc_score': tsa.grad, 'g_pos_score': tsp.grad}
    return {k: torch.as_tensor(v).detach().double().numpy() for k, v in out.items()}


def _circle_device(a, p, dk, sa, sp):
    ga, gp, gsa, gsp = (cu(v).requires_grad_(True) for v in (a, p, sa, sp))
    scalars, d, fp, an = ops.circle_det_loss(ga, gp, cu(dk), gsa, gsp)
    (1.0 * scalars[0] + 0.7 * scalars[1]).backward()
    torch.cuda.synchronize()
    s = scalars.detach().cpu().double().numpy()
    out = {'loss': s[0], 'det': s[1], 'acc': s[2], 'dists': d, 'fp': fp, 'an': an, 'g_anchor': ga.grad,
           'g_positive': gp.grad, 'g_anc_score': gsa.grad, 'g_pos_score': gsp.grad}
    return {k: torch.as_tensor(v).detach().cpu().double().numpy() for k, v in out.items()}, s


def _circle_errors(got, want):
    """The error measures of test_circle_det_loss, one per quantity."""
    err = {'loss': abs(float(got['loss']) - float(want['loss'])) / max(1.0, abs(float(want['loss']))),
           'det': abs(float(got['det']) - float(want['det'])), 'acc': abs(float(got['acc']) - float(want['acc']))}
    for k in ('dists', 'fp', 'an', 'g_anchor', 'g_positive', 'g_anc_score', 'g_pos_score'):
        err[k] = rel_err(got[k], want[k])
    return err


# test_circle_det_loss's tolerances, by quantity
CIRCLE_TOL = {'loss': 1e-5, 'det': 1e-5, 'acc': 1e-3, 'dists': 1e-5, 'fp': 1e-5, 'an': 1e-5, 'g_anchor': BWD_TOL,
              'g_positive': BWD_TOL, 'g_anc_score': 1e-5, 'g_pos_score': 1e-5}


def _assert_circle(shape, tol, min_gap=None):
    """``tol`` None: the M = 1024 rule, max(CIRCLE_TOL, 4 x the f32 oracle's error against the f64 oracle)."""
    inp = _circle_inputs(*shape)
    want = _circle_oracle(*inp)
    if min_gap is not None:
        assert float(_closest_negative(want)[1].min()) > min_gap
    if tol is None:
        f32_err = _circle_errors(_circle_oracle(*inp, dtype=torch.float32), want)
        print("circle oracle f32 vs f64", shape, {k: "%.3g" % v for k, v in f32_err.items()})
        tol = _max_with_factor_4(CIRCLE_TOL, f32_err)
        assert tol == CIRCLE_TOL, tol            # (the recorded outcome: no bound had to grow)
    got, s = _circle_device(*inp)
    err = _circle_errors(got, want)
    print("circle_det_loss", shape, {k: "%.3g" % v for k, v in err.items()})
    assert abs(s[5] - (s[0] + s[1])) <= 1e-5, shape
    for k, v in err.items():
        assert v < tol[k], (shape, k, v, tol[k])


@pytest.mark.parametrize("m,c", [(129, 32), (200, 32), (64, 65), (2, 80)])
def test_circle_det_loss_in_one_workgroup(m, c):
    """ops.circle_det_loss forward + backward where cache_ok(M, C) fails: loss_fwd_kernel and
    loss_bwd_kernel, one 1024-thread workgroup on the global buffers (distances in ``dists``, G in the
    workspace), against ops_ref.circle_loss + ops_ref.det_loss in f64 at test_circle_det_loss's tolerances.
    (129, 32): the first M past the tiled form.  (200, 32): M no multiple of 64, so the last round of line_stats has idle
    lanes.  (64, 65): the smallest C that leaves the tiled form, at a small M.  (2, 80): the smallest legal M -- 1020 of
    the 1024 threads own no distance and 14 of the 16 waves no line."""
    _assert_circle((m, c), CIRCLE_TOL)


def test_circle_det_loss_in_one_workgroup_at_the_largest_m():
    """(M, C) = (1024, 32), kMaxM: every thread of loss_fwd_kernel / loss_bwd_kernel walks 1024 of the
    M * M entries, every wave 64 rows and 64 columns of 1024 entries, every thread of the backward 32 sums of 1024 terms.
    The sums are 8 x longer than at M = 128, so every bound is max(test_circle_det_loss's, 4 x the error of the f32
    oracle against the f64 oracle), see _max_with_factor_4; the test computes them.  Measured f32-vs-f64 oracle errors:
        loss 2.1e-8, det 9.7e-9, accuracy 0, dists 1.4e-7, fp 6.6e-8, an 2.1e-7,
        grad anchor 5.7e-7, grad positive 6.3e-7, grad scores 1.9e-7
    Four times the largest of them is 2.5e-6, below every existing tolerance, so the bounds stay test_circle_det_loss's:
        1e-5 on loss, det, dists, fp, an and the score gradients, 1e-3 on accuracy, 2e-4 on the descriptor gradients.
    The two nearest negatives of every row of this input are at least 3.1e-5 apart in the f64 oracle (asserted above
    1e-5), so the detector term's arg-min is the same row in f32."""
    _assert_circle((1024, 32), None, min_gap=1e-5)


def test_train_loss_with_weights_at_a_size_that_is_not_tiled():
    """ops.train_loss at M = 200 with (w_desc, w_det) = (1.0, 0.5): the `plain and weights != (1, 1)` route of
    _TrainLossFn (total = dot(scalars[:2], gw), the backward hands both weighted gradients to loss_bwd_kernel)
    against the eager composition F.normalize + indexing + ops_ref in f64."""
    rng = np.random.default_rng(200)
    M, C, n0, n1 = 200, 32, 700, 650
    x = rng.normal(size=(n0 + n1, C)).astype(np.float32)
    sc = rng.random((n0 + n1, 1)).astype(np.float32)
    corr = np.stack([rng.choice(n0, M, replace=False), rng.choice(n1, M, replace=False)], 1).astype(np.int64)
    x[n0 + corr[:, 1]] = x[corr[:, 0]] + 0.3 * rng.normal(size=(M, C)).astype(np.float32)     # matching descriptors
    kp = rng.random((M, 3))
    dk = np.linalg.norm(kp[:, None] - kp[None], axis=-1)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    st = torch.tensor(sc, dtype=torch.float64, requires_grad=True)
    f = F.normalize(xt, p=2, dim=-1)
    c = torch.from_numpy(corr)
    desc, acc, fp, an, dists = ops_ref.circle_loss(f[c[:, 0]], f[c[:, 1] + n0], torch.from_numpy(dk))
    det = ops_ref.det_loss(dists, st[c[:, 0]], st[c[:, 1] + n0])
    (1.0 * desc + 0.5 * det).backward()
    gx, gs = cu(x).requires_grad_(True), cu(sc).requires_grad_(True)
    total, d1, e1, a1, f1, n1_ = ops.train_loss(gx, gs, cu(corr), n0, cu(dk), w_desc=1.0, w_det=0.5)
    total.backward()
    torch.cuda.synchronize()
    assert abs(float(d1) - float(desc)) < 1e-5 * max(1.0, abs(float(desc)))
    assert abs(float(e1) - float(det)) < 1e-5
    assert abs(float(total) - (float(desc) + 0.5 * float(det))) < 1e-5 * max(1.0, abs(float(desc)))
    assert abs(float(a1) - float(acc)) < 1e-3
    assert rel_err(f1.cpu().numpy(), fp.detach().numpy()) < 1e-5
    assert rel_err(n1_.cpu().numpy(), an.detach().numpy()) < 1e-5
    assert rel_err(gx.grad.cpu().numpy(), xt.grad.numpy()) < BWD_TOL
    assert rel_err(gs.grad.cpu().numpy(), st.grad.numpy()) < 1e-5


def test_stacked_circle_loss_still_refuses_more_than_128_rows():
    """The stacked form has the tiled kernels only: ops.train_loss_pairs at M = 129 raises instead of launching."""
    rng = np.random.default_rng(129)
    M, C = 129, 32
    x, sc = cu(rng.normal(size=(600, C)).astype(np.float32)), cu(rng.random((600, 1)).astype(np.float32))
    corr = cu(rng.integers(0, 250, size=(1, M, 2)).astype(np.int64))
    lens = torch.tensor([300, 300], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="M <= 128"):
        ops.train_loss_pairs(x, sc, corr, lens, cu(rng.random((1, M, M))))


# ================================================================================================================
# B. contrastive + detector loss, wide channels and many rows
# ================================================================================================================
def _contrastive_inputs(M, C, seed=0):
    """test_adam_contrastive_gpu._inputs (the forced near pair dk[3,5] included).  Its M = 64 / 128 are the recorded
    C = 32 vectors of the reference, so those two sizes restate its random recipe here for other channel counts."""
    if M not in (64, 128):
        return _inputs(M, C, seed)[:8]
    rng = np.random.RandomState(seed)
    a = rng.randn(M, C)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    p = a + 0.3 * rng.randn(M, C)
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    dk = rng.rand(M, M) * 0.4
    dk = np.minimum(dk, dk.T)
    dk[3, 5] = dk[5, 3] = 0.1
    return (a.astype(np.float32), p.astype(np.float32), dk, rng.rand(M).astype(np.float32),
            rng.rand(M).astype(np.float32), 0.1, 0.1, 1.4)


def _contrastive_device(a, p, dk, sa, sp, sr, pm, nm):
    ta, tp, tsa, tsp = (torch.tensor(v, device=DEV, requires_grad=True) for v in (a, p, sa, sp))
    scalars, dists, fp, an = ops.contrastive_det_loss(ta, tp, torch.tensor(dk, device=DEV), tsa, tsp, sr, pm, nm)
    (scalars[0] + scalars[1]).backward()
    torch.cuda.synchronize()
    out = {'desc': float(scalars[0]), 'det': float(scalars[1]), 'acc': float(scalars[2]),
           'dists': dists.double().cpu().numpy(), 'fp': fp.double().cpu().numpy(), 'an': an.double().cpu().numpy(),
           'g_anchor': ta.grad.double().cpu().numpy(), 'g_positive': tp.grad.double().cpu().numpy(),
           'g_anc_score': tsa.grad.double().cpu().numpy(), 'g_pos_score': tsp.grad.double().cpu().numpy()}
    assert abs(float(scalars[5]) - (out['desc'] + out['det'])) <= 1e-5
    return out


def _contrastive_errors(out, want):
    """The error measures of test_adam_contrastive_gpu._check, one per quantity."""
    err = {'desc': abs(out['desc'] - want['desc']) / max(1.0, abs(want['desc'])),
           'det': abs(out['det'] - want['det']) / max(1.0, abs(want['det'])), 'acc': abs(out['acc'] - want['acc'])}
    for k in ('dists', 'fp', 'an'):
        err[k] = float(np.abs(np.asarray(out[k], np.float64) - np.asarray(want[k], np.float64)).max())
    for k in ('g_anchor', 'g_positive', 'g_anc_score', 'g_pos_score'):
        ref = np.asarray(want[k], np.float64)
        err[k] = float(np.abs(out[k] - ref).max() / max(1e-12, np.abs(ref).max()))
    return err


# _check's bounds, by quantity (the gradients strictly below theirs)
CONTRASTIVE_TOL = {'desc': 2e-5, 'det': 2e-5, 'acc': 1e-3, 'dists': 2e-5, 'fp': 2e-5, 'an': 2e-5, 'g_anchor': 1e-4,
                   'g_positive': 1e-4, 'g_anc_score': 1e-4, 'g_pos_score': 1e-4}


def _closest_negative(want):
    """(argmin, gap to the runner-up) per row of the oracle's dists, the diagonal excluded."""
    d = np.array(want['dists'], np.float64)
    np.fill_diagonal(d, np.inf)
    two = np.sort(d, axis=1)[:, :2]
    return d.argmin(axis=1), two[:, 1] - two[:, 0]


@pytest.mark.parametrize("M,C", [(37, 65), (64, 130), (128, 256), (300, 32)])
def test_contrastive_det_loss_wide_channels_and_many_rows(M, C):
    """ops.contrastive_det_loss forward + backward against the f64 ContrastiveLoss + DetLoss at _check's bounds.  The
    positive-row wave of contrastive_bwd_kernel keeps acc[4], one slot per 64 channels, and scans `arg[i] == j` with one
    __ballot per 64 rows:  (37, 65) slot 1 with a single live channel;  (64, 130) three slots, the last partly filled;
    (128, 256) all four slots, the largest C the API takes;  (300, 32) five ballot rounds, the last with 44 live rows."""
    inp = _contrastive_inputs(M, C)
    _check(_contrastive_device(*inp), _oracle(*inp, torch.float64), 'f64 M=%d C=%d' % (M, C))


def test_contrastive_backward_with_many_rows_sharing_one_closest_negative():
    """(M, C) = (64, 130): 40 anchors (rows 10..49) have positive 7 as their closest negative, so the single ballot
    round of positive 7's wave carries 40 hits and adds them in ascending row order into three acc slots.
    Forty near-orthogonal unit vectors of the random recipe have no common neighbour (the best a unit vector reaches is
    a . p = 1/sqrt(40) with all of them, below the largest of 63 chance alignments), so these anchors are given a common
    component first (a_i <- normalise(a_i + u), |u| = 1; their positives are rebuilt from them by the recipe); positive
    7 is then the renormalised mean of anchors 10..49, and the keypoint distances of column 7 to those rows are put
    outside the safe radius so that none of the 40 entries is masked.  The oracle itself is asked whether the
    construction does its job: at least 32 rows with argmin == 7."""
    M, C = 64, 130
    a, p, dk, sa, sp, sr, pm, nm = _contrastive_inputs(M, C, seed=1)
    rng = np.random.RandomState(7)
    u = rng.randn(C)
    u /= np.linalg.norm(u)
    a64 = a.astype(np.float64)
    a64[10:50] += u
    a64[10:50] /= np.linalg.norm(a64[10:50], axis=1, keepdims=True)
    p64 = p.astype(np.float64)
    p64[10:50] = a64[10:50] + 0.3 * rng.randn(40, C)
    p64[10:50] /= np.linalg.norm(p64[10:50], axis=1, keepdims=True)
    p64[7] = a64[10:50].mean(axis=0)
    p64[7] /= np.linalg.norm(p64[7])
    dk[10:50, 7] = dk[7, 10:50] = 0.3
    inp = (a64.astype(np.float32), p64.astype(np.float32), dk, sa, sp, sr, pm, nm)
    want = _oracle(*inp, torch.float64)
    arg, _ = _closest_negative(want)
    assert int((arg == 7).sum()) >= 32, int((arg == 7).sum())
    _check(_contrastive_device(*inp), want, 'f64 shared closest negative')


def test_contrastive_det_loss_at_the_largest_m():
    """(M, C) = (1024, 48), the API's largest M: 256 workgroups of row waves forward, 512 backward, 16 ballot rounds per
    positive row, row sums of 1024 distances for average_negative.  Bounds: max(_check's, 4 x the error of the f32
    oracle against the f64 oracle), see _max_with_factor_4.  A row whose two nearest negatives are closer together than
    f32 resolves has no defined arg-min (its gradient moves to another row); the oracle is asked first that no row of
    this input is such a tie (gap > 1e-5; it is 2.9e-5).  Measured f32-vs-f64 oracle errors (the test computes them):
        desc 1.4e-8, det 2.8e-9, accuracy 0, dists 6.6e-7, fp 1.3e-7, an 1.1e-6,
        grad anchor 1.4e-7, grad positive 1.1e-7, grad scores 5.5e-7
    Four times the largest of them is 4.4e-6, below every bound of _check, so the bounds stay _check's:
        2e-5 on desc, det (relative to max(1, |.|)), dists, fp, an, 1e-3 on accuracy, 1e-4 on the four gradients."""
    inp = _contrastive_inputs(1024, 48)
    want = _oracle(*inp, torch.float64)
    assert float(_closest_negative(want)[1].min()) > 1e-5
    err = _contrastive_errors(_contrastive_device(*inp), want)
    f32_err = _contrastive_errors(_oracle(*inp, torch.float32), want)
    print("contrastive oracle f32 vs f64 (1024, 48)", {k: "%.3g" % v for k, v in f32_err.items()})
    tol = _max_with_factor_4(CONTRASTIVE_TOL, f32_err)
    assert tol == CONTRASTIVE_TOL, tol           # (the recorded outcome: no bound had to grow)
    print("contrastive_det_loss (1024, 48)", {k: "%.3g" % v for k, v in err.items()})
    for k, v in err.items():
        assert v < tol[k], (k, v, tol[k])


def test_stacked_contrastive_loss_past_128_rows_equals_the_single_pair_form():
    """ops.train_contrastive_loss_pairs with P = 2 pairs of M = 150 rows (three ballot rounds, blockIdx.y = pair) against
    ops.train_contrastive_loss on each pair alone, (w_desc, w_det) = (1.0, 0.5); pattern and bounds of
    test_training_forms_single_and_stacked_match_the_modular_loss."""
    P, M, C, sr, pm, nm = 2, 150, 32, 0.1, 0.1, 1.4
    sizes = [(300, 280), (250, 310)]
    pairs = []
    for q, (n0, n1) in enumerate(sizes):
        rng = np.random.RandomState(20 + q)
        x, s = rng.randn(n0 + n1, C).astype(np.float32), rng.rand(n0 + n1, 1).astype(np.float32)
        corr = np.stack([rng.choice(n0, M, replace=False), rng.choice(n1, M, replace=False)], 1).astype(np.int64)
        x[n0 + corr[:, 1]] = x[corr[:, 0]] + 0.2 * rng.randn(M, C).astype(np.float32)    # matching descriptors
        dk = rng.rand(M, M) * 0.3
        pairs.append((x, s, corr, np.minimum(dk, dk.T), n0))
    xt = torch.tensor(np.concatenate([p_[0] for p_ in pairs]), device=DEV, requires_grad=True)
    stt = torch.tensor(np.concatenate([p_[1] for p_ in pairs]), device=DEV, requires_grad=True)
    lens = torch.tensor([v for n in sizes for v in n], dtype=torch.int32, device=DEV)
    corr_all = torch.tensor(np.stack([p_[2] for p_ in pairs]), device=DEV)
    dk_all = torch.tensor(np.stack([p_[3] for p_ in pairs]), device=DEV)
    total, desc, det, acc, fp, an = ops.train_contrastive_loss_pairs(xt, stt, corr_all, lens, dk_all, sr, pm, nm,
                                                                     w_desc=1.0, w_det=0.5)
    total.backward()
    start, want_total = 0, 0.0
    for q, (x, s, corr, dk, n0) in enumerate(pairs):
        n = x.shape[0]
        xq = torch.tensor(x, device=DEV, requires_grad=True)
        sq = torch.tensor(s, device=DEV, requires_grad=True)
        t1, d1, e1, a1, f1, n1 = ops.train_contrastive_loss(xq, sq, torch.tensor(corr, device=DEV), n0,
                                                            torch.tensor(dk, device=DEV), sr, pm, nm, w_desc=1.0,
                                                            w_det=0.5)
        t1.backward()
        assert abs(float(desc[q]) - float(d1)) < 2e-5 and abs(float(det[q]) - float(e1)) < 2e-5, q
        assert abs(float(acc[q]) - float(a1)) < 1e-3, q
        assert float((fp[q] - f1).abs().max()) <= 2e-5 and float((an[q] - n1).abs().max()) <= 2e-5, q
        want_total += float(t1)
        assert float((xt.grad[start:start + n] - xq.grad).abs().max()) <= 1e-4 * float(xq.grad.abs().max()), q
        assert float((stt.grad[start:start + n] - sq.grad).abs().max()) <= 1e-4 * max(1e-6, float(sq.grad.abs().max()))
        start += n
    assert abs(float(total) - want_total) < 1e-4


# ================================================================================================================
# C. optimizer guard and update over every loop of the real launch
# ================================================================================================================
S = 2048 * 256                               # grid stride in float4: the launch is capped at 2048 blocks of 256
N_OPT = 4 * (4 * S + S // 2) + 3             # 9 437 187 floats, 38 MB per buffer


def test_optimizer_length_reaches_every_loop_of_the_capped_launch():
    """The arithmetic the cases below stand on, against the launch of d3f_sgd_guarded_step_lanes /
    d3f_adam_guarded_step: blocks = min(2048, ceil((n/4 + 1) / 256))."""
    n4 = N_OPT // 4
    assert N_OPT == 9437187 and min(2048, -(-(n4 + 1) // 256)) == 2048 and S == 524288
    assert n4 == 4 * S + S // 2              # every thread: one unrolled round (i + 3 S < n4 for all i < S) ...
    assert (S - 1) + 4 * S + 3 * S >= n4     # ... and no second one,
    assert n4 - 4 * S == S // 2              # then one remainder iteration in the first half of the threads,
    assert N_OPT % 4 == 3                    # and three scalars in the tail


def _guard_cases():
    q = [5, S + 5, 2 * S + 5, 3 * S + 5,     # the four loads a, b, c, d of the unrolled round
         S - 1, 4 * S - 1,                   # the last thread: its first and its last load
         4 * S + 5, 4 * S + S // 2 - 1]      # the remainder loop: an early thread and the last one that runs it
    idx = [4 * v + k % 4 for k, v in enumerate(q)] + [N_OPT - 1, N_OPT - 3]
    vals = [float('inf'), float('-inf'), float('nan')]
    return [(i, vals[k % 3], k // 2) for k, i in enumerate(idx)]


@pytest.mark.parametrize("lanes", [1, 4])
@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_guard_finds_one_nonfinite_value_in_every_loop(opt, lanes):
    """nonfinite_kernel at n = N_OPT: ONE non-finite value (+Inf, -Inf, NaN in turn) in one gradient lane, at a float4
    served by each of the four loads of the unrolled round, by the remainder loop and by the scalar tail, in every
    component of the float4 -- each such step must be skipped (state[1] + 1; parameters, moments / momentum buffer and
    Adam's step counter bit-unchanged).  Then +Inf and -Inf at the same place in two lanes, and an all-finite step, which
    must apply."""
    gen = torch.Generator(device=DEV).manual_seed(lanes)
    grads = [torch.randn(N_OPT, device=DEV, generator=gen) * 1e-2 for _ in range(lanes)]
    p = torch.randn(N_OPT, device=DEV, generator=gen)
    bufs = [torch.zeros_like(p) for _ in range(1 if opt == "sgd" else 2)]
    t = torch.zeros(1, device=DEV)
    state = torch.zeros(4, dtype=torch.int32, device=DEV)
    hyper = _hyper()
    keep = [x.clone() for x in [p] + bufs]

    def step():
        g = grads if lanes > 1 else grads[0]
        if opt == "sgd":
            ops.sgd_guarded_step(g, p, bufs[0], 0.01, 0.98, 1e-6, state)
        else:
            ops.adam_guarded_step(g, p, bufs[0], bufs[1], t, hyper, state)

    def unchanged():
        return all(torch.equal(x, y) for x, y in zip(keep, [p] + bufs)) and float(t) == 0.0

    skipped = 0
    for i, val, k in _guard_cases():
        lane = grads[k % lanes]
        old = float(lane[i])
        lane[i] = val
        step()
        skipped += 1
        assert int(state[1]) == skipped, (i, val, k % lanes)
        assert unchanged(), (i, val, k % lanes)
        lane[i] = old
    if lanes > 1:
        i = 4 * (2 * S + 77) + 2                                     # load c of the unrolled round
        old = float(grads[1][i]), float(grads[2][i])
        grads[1][i], grads[2][i] = float('inf'), float('-inf')
        step()
        skipped += 1
        assert int(state[1]) == skipped and unchanged()
        grads[1][i], grads[2][i] = old
    step()
    assert state.tolist() == [0, skipped, 0, 0]
    assert not torch.equal(keep[0], p) and (opt == "sgd" or float(t) == 1.0)


def _ends(x):
    """The whole buffer, the last 4 * 256 elements of the float4 range and the three tail scalars, each on its own: a
    defect at the end of the grid-stride range must not hide in a maximum over 9 M values."""
    return (("all", x), ("last float4s", x[N_OPT - 3 - 4 * 256:N_OPT - 3]), ("scalar tail", x[N_OPT - 3:]))


@pytest.mark.parametrize("lanes", [1, 3])
def test_adam_update_over_every_loop_matches_torch_adam(lanes):
    """adam_kernel at n = N_OPT (two and a half grid-stride rounds and the scalar tail), 3 steps against
    torch.optim.Adam(foreach=False) on the device at test_adam_step_matches_torch_adam's per-element bounds
    (1e-6 / 1e-7 / 1e-9 on p / m / v).

    This size also pins how adam1 forms g = grad + wd p.  Adam's first step is lr g / (|g| + eps), whose slope
    lr eps / (|g| + eps)^2 reaches lr / eps = 1e6 where |g| <= eps = 1e-8.  Among 9.4 M gradients of scale 1e-2 about a
    dozen fall below 1e-8 (among the 100003 of the existing test the smallest is ~2e-7), and there one f32 rounding of
    wd p on its own, instead of the fused multiply-add of torch's grad.add(param, alpha=wd), moves p by up to 2.1e-6:
    twice the bound.  adam1 therefore fuses that term (fmaf); with it every element agrees to 1e-6."""
    gen = torch.Generator(device=DEV).manual_seed(10 + lanes)
    p0 = torch.randn(N_OPT, device=DEV, generator=gen)
    ref_p = torch.nn.Parameter(p0.clone())
    ref = torch.optim.Adam([ref_p], lr=0.01, betas=(0.9, 0.999), weight_decay=1e-4, foreach=False)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    del p0
    t = torch.zeros(1, device=DEV)
    state = torch.zeros(4, dtype=torch.int32, device=DEV)
    gs = 1.0 / lanes
    hyper = _hyper(gs=gs)
    for s in range(3):
        gl = [torch.randn(N_OPT, device=DEV, generator=gen) * 1e-2 for _ in range(lanes)]
        total = gl[0].clone()
        for g in gl[1:]:
            total += g
        ref_p.grad = total.mul_(gs)
        ref.step()
        ops.adam_guarded_step(gl if lanes > 1 else gl[0], p, m, v, t, hyper, state)
    torch.cuda.synchronize()
    st = ref.state[ref_p]
    assert float(t) == 3.0 and state.tolist()[1:] == [0, 0, 0]
    for name, x, y, bound in (("p", p, ref_p.detach(), 1e-6), ("m", m, st['exp_avg'], 1e-7),
                              ("v", v, st['exp_avg_sq'], 1e-9)):
        errs = [(what, float((a - b).abs().max())) for (what, a), (_, b) in zip(_ends(x), _ends(y))]
        print("adam lanes=%d" % lanes, name, errs)
        for what, e in errs:
            assert e <= bound, (name, what, e)


def test_sgd_update_over_every_loop_matches_torch_sgd_and_the_lane_sum():
    """sgd_kernel at n = N_OPT, 3 steps: the single-buffer step on (g0 + g1) + g2 against torch.optim.SGD(momentum,
    weight_decay) to 1e-7 max(1, |p|max), and the three-lane step on g0, g1, g2 bit-identical to it (parameters and
    momentum buffer), as in test_guarded_sgd_on_gradient_lanes_steps_on_their_sum."""
    gen = torch.Generator(device=DEV).manual_seed(3)
    p0 = torch.randn(N_OPT, device=DEV, generator=gen)
    ref_p = torch.nn.Parameter(p0.clone())
    ref = torch.optim.SGD([ref_p], lr=0.01, momentum=0.98, weight_decay=1e-6)
    p1, b1, p3, b3 = p0.clone(), torch.zeros_like(p0), p0.clone(), torch.zeros_like(p0)
    del p0
    s1 = torch.zeros(4, dtype=torch.int32, device=DEV)
    s3 = torch.zeros(4, dtype=torch.int32, device=DEV)
    for s in range(3):
        gl = [torch.randn(N_OPT, device=DEV, generator=gen) for _ in range(3)]
        total = (gl[0] + gl[1]) + gl[2]
        ops.sgd_guarded_step(gl, p3, b3, 0.01, 0.98, 1e-6, s3)
        ops.sgd_guarded_step(total, p1, b1, 0.01, 0.98, 1e-6, s1)
        ref_p.grad = total
        ref.step()
        for (what, a), (_, b) in zip(_ends(p3) + _ends(b3), _ends(p1) + _ends(b1)):
            assert torch.equal(a, b), (s, what)
    assert s1.tolist() == [0, 0, 0, 0] and s3.tolist() == [0, 0, 0, 0]
    want = ref_p.detach()
    bound = 1e-7 * max(1.0, float(want.abs().max()))
    errs = [(what, float((a - b).abs().max())) for (what, a), (_, b) in zip(_ends(p1), _ends(want))]
    print("sgd p", errs, "bound", bound)
    for what, e in errs:
        assert e <= bound, (what, e, bound)


# ================================================================================================================
# D. pools off the vector path, and ``width`` against the oracle
# ================================================================================================================
NS, NQ, H = 500, 211, 17


def _pool_table(rng):
    """The index table of test_pools: shadow entries (== NS) anywhere, the first three rows all shadow."""
    idx = rng.integers(0, NS + 1, size=(NQ, H)).astype(np.int64)
    idx[:3] = NS
    return idx


def _one_float_in(a):
    """``a`` on the device as a contiguous view that starts one float into a larger buffer: 4 bytes off a 16-byte
    boundary, which is what sends a C % 4 == 0 matrix to the scalar kernels."""
    buf = torch.zeros(a.size + 8, dtype=torch.float32, device=DEV)
    v = buf[1:1 + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def test_pools_on_an_input_that_is_not_16_byte_aligned():
    """C = 64 with x one float off alignment: d3f_max_pool_forward / d3f_closest_pool_forward take max_pool_fwd_kernel /
    closest_pool_fwd_kernel (one channel per thread) although C % 4 == 0 -- every other test hands freshly allocated,
    aligned tensors, so with C % 4 == 0 only the _v4 kernels ran.  Forward equal to the oracle, backward within
    test_pools' 1e-6; then the concatenating closest_pool with a misaligned skip, and with Cs = 6 (Cs % 4 != 0)."""
    rng = np.random.default_rng(64)
    C = 64
    x = rng.normal(size=(NS, C)).astype(np.float32)
    idx = _pool_table(rng)
    for fn, ref_fn in ((ops.max_pool, ops_ref.max_pool), (ops.closest_pool, ops_ref.closest_pool)):
        tx = torch.from_numpy(x).requires_grad_(True)
        ref = ref_fn(tx, torch.from_numpy(idx))
        go = torch.from_numpy(rng.normal(size=ref.shape).astype(np.float32))
        ref.backward(go)
        gx = _one_float_in(x).requires_grad_(True)
        out = fn(gx, cu(idx))
        out.backward(cu(go))
        assert np.array_equal(out.detach().cpu().numpy(), ref.detach().numpy()), fn.__name__
        assert rel_err(gx.grad.cpu().numpy(), tx.grad.numpy()) < 1e-6, fn.__name__
    for cs, misaligned in ((24, True), (6, False)):
        skip = rng.normal(size=(NQ, cs)).astype(np.float32)
        wgt = rng.normal(size=(NQ, C + cs)).astype(np.float32)
        tx = torch.from_numpy(x).requires_grad_(True)
        ref_y = torch.cat([ops_ref.closest_pool(tx, torch.from_numpy(idx)), torch.from_numpy(skip)], dim=1)
        (ref_y * torch.from_numpy(wgt)).sum().backward()
        gx = cu(x).requires_grad_(True)
        gsk = (_one_float_in(skip) if misaligned else cu(skip)).requires_grad_(True)
        assert gx.data_ptr() % 16 == 0 and (misaligned or gsk.data_ptr() % 16 == 0)
        y = ops.closest_pool(gx, cu(idx), skip=gsk)
        assert np.array_equal(y.detach().cpu().numpy(), ref_y.detach().numpy()), cs
        (y * cu(wgt)).sum().backward()
        assert rel_err(gx.grad.cpu().numpy(), tx.grad.numpy()) < 1e-6, cs
        assert np.array_equal(gsk.grad.cpu().numpy(), wgt[:, C:]), cs


@pytest.mark.parametrize("C", [64, 33])
def test_max_pool_width_equals_the_oracle_on_the_narrower_table(C):
    """ops.max_pool(x, idx, width=[w]) == ops_ref.max_pool(x, idx[:, :min(w, H)]), output bit for bit and gradient, for
    w = 1, a width inside the table, the table's own width and one beyond it.  C = 64: max_pool_fwd_v4_kernel;
    C = 33: max_pool_fwd_kernel, whose loop bound is readfirstlane(*width).  Then the grouped branches: four clouds in
    two groups with widths (5, 12) through ``groups``, every group's rows against the oracle on its own truncated table
    (not against another call of the op)."""
    rng = np.random.default_rng(C)
    x = rng.normal(size=(NS, C)).astype(np.float32)
    x[::7] = -np.abs(x[::7])                 # rows whose maximum is the shadow's zero once their columns are trimmed
    idx = _pool_table(rng)
    go = rng.normal(size=(NQ, C)).astype(np.float32)
    for w in (1, 5, 17, 40):
        tx = torch.from_numpy(x).requires_grad_(True)
        ref = ops_ref.max_pool(tx, torch.from_numpy(idx[:, :min(w, H)]))
        ref.backward(torch.from_numpy(go))
        gx = cu(x).requires_grad_(True)
        out = ops.max_pool(gx, cu(idx), width=torch.tensor([w], dtype=torch.int32, device=DEV))
        out.backward(cu(go))
        assert np.array_equal(out.detach().cpu().numpy(), ref.detach().numpy()), w
        assert rel_err(gx.grad.cpu().numpy(), tx.grad.numpy()) < 1e-6, w
    lens_q = np.array([60, 51, 70, 30], np.int32)
    assert int(lens_q.sum()) == NQ
    widths = np.array([5, 12], np.int32)
    gx = cu(x).requires_grad_(True)
    out = ops.max_pool(gx, cu(idx), width=cu(widths), groups=(cu(lens_q), 2))
    out.backward(cu(go))
    tx = torch.from_numpy(x).requires_grad_(True)
    q0 = 0
    for g in range(2):
        q1 = q0 + int(lens_q[2 * g:2 * g + 2].sum())
        ref = ops_ref.max_pool(tx, torch.from_numpy(idx[q0:q1, :widths[g]]))
        ref.backward(torch.from_numpy(go[q0:q1]))
        assert np.array_equal(out[q0:q1].detach().cpu().numpy(), ref.detach().numpy()), g
        q0 = q1
    assert rel_err(gx.grad.cpu().numpy(), tx.grad.numpy()) < 1e-6


# ================================================================================================================
# E. batch norm backward on a capacity buffer
# ================================================================================================================
@pytest.mark.parametrize("C", [48, 300])
def test_batch_norm_backward_on_the_live_rows_of_a_capacity_buffer(C):
    """ops.batch_norm forward + backward with n_live = 500 of N = 700 rows; the rows past 500 of x AND of the incoming
    gradient are NaN, so one read of a dead row by bn_bwd_sum_kernel poisons dgamma / dbeta and everything behind them.
    Against torch.nn.functional.batch_norm (+ LeakyReLU 0.1) in f64 on x[:500] at test_batch_norm_matches_torch's
    bounds (1e-5, 2e-4 on the gradients); dx past the live rows is exactly zero.  C = 48: 64 columns x 4 row lanes per
    workgroup, 16 columns idle; C = 300: 256 columns x 1 lane, two column tiles, the second with 44 live columns."""
    N, n = 700, 500
    rng = np.random.default_rng(N + C)
    x = (rng.normal(size=(N, C)) * rng.uniform(0.5, 2.0, size=C)).astype(np.float32)
    w = rng.uniform(0.5, 1.5, size=C).astype(np.float32)
    b = rng.normal(size=C).astype(np.float32)
    go = rng.normal(size=(N, C)).astype(np.float32)
    xt = torch.tensor(x[:n], dtype=torch.float64, requires_grad=True)
    wt = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(b, dtype=torch.float64, requires_grad=True)
    ref = F.leaky_relu(F.batch_norm(xt.t().unsqueeze(0), None, None, wt, bt, True, 0.02, 1e-5).squeeze(0).t(), 0.1)
    ref.backward(torch.tensor(go[:n], dtype=torch.float64))
    x[n:], go[n:] = np.nan, np.nan
    gx, gw, gb = (cu(v).requires_grad_(True) for v in (x, w, b))
    y = ops.batch_norm(gx, gw, gb, None, None, True, momentum=0.02, eps=1e-5, slope=0.1,
                       n_live=torch.tensor([n], dtype=torch.int32, device=DEV))
    y.backward(cu(go))
    torch.cuda.synchronize()
    assert rel_err(y[:n].detach().cpu().numpy(), ref.detach().numpy()) < 1e-5
    assert float(y[n:].detach().abs().max()) == 0.0
    assert bool(torch.isfinite(gw.grad).all()) and bool(torch.isfinite(gb.grad).all())
    assert rel_err(gx.grad[:n].cpu().numpy(), xt.grad.numpy()) < 2e-4
    assert torch.equal(gx.grad[n:], torch.zeros_like(gx.grad[n:]))
    assert rel_err(gw.grad.cpu().numpy(), wt.grad.numpy()) < 2e-4
    assert rel_err(gb.grad.cpu().numpy(), bt.grad.numpy()) < 2e-4
