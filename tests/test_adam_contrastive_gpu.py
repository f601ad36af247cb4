"""GPU: the guarded Adam step and the fused contrastive + detector loss (reference optimizer 'ADAM' and desc_loss
'contrastive', training_3DMatch.py:62-76,119-132) -- kernels against torch.optim.Adam and the reference's recorded
loss, the graph-captured step, the training forms, the Trainer on the graph path with a snapshot resumed eagerly, and
a stacked lanes schedule."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from d3feat_pytorch_amd import config as cfgmod
from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.utils.loss import ContrastiveLoss, DetLoss

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contrastive.npz")
pytestmark = pytest.mark.gpu


def _item(g):
    n0, n1 = g['pts0'].shape[0], g['pts1'].shape[0]
    return (g['pts0'], g['pts1'], np.ones((n0, 1), np.float32), np.ones((n1, 1), np.float32), g['sel_corr'],
            g['dist_keypts_in'])


def _hyper(lr=0.01, betas=(0.9, 0.999), eps=1e-8, wd=1e-4, gs=1.0):
    return torch.tensor([lr, betas[0], betas[1], eps, wd, gs], dtype=torch.float64, device=DEV)


# ---- Adam kernel ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [1, 2, 3, 4])
def test_adam_step_matches_torch_adam(lanes):
    n = 100003                                       # not a multiple of 4: the tail path
    gen = torch.Generator(device=DEV).manual_seed(lanes)
    p0 = torch.randn(n, device=DEV, generator=gen)
    ref_p = torch.nn.Parameter(p0.clone())
    ref = torch.optim.Adam([ref_p], lr=0.01, betas=(0.9, 0.999), weight_decay=1e-4, foreach=False)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    t = torch.zeros(1, device=DEV)
    state = torch.zeros(4, dtype=torch.int32, device=DEV)
    gs = 1.0 / lanes
    hyper = _hyper(gs=gs)
    for s in range(6):
        gl = [torch.randn(n, device=DEV, generator=gen) * 1e-2 for _ in range(lanes)]
        total = gl[0].clone()
        for g in gl[1:]:
            total += g
        ref_p.grad = total * gs
        ref.step()
        ops.adam_guarded_step(gl if lanes > 1 else gl[0], p, m, v, t, hyper, state)
    torch.cuda.synchronize()
    st = ref.state[ref_p]
    assert float(t) == 6.0 and state.tolist()[1:] == [0, 0, 0]
    assert float((p - ref_p.detach()).abs().max()) <= 1e-6
    assert float((m - st['exp_avg']).abs().max()) <= 1e-7
    assert float((v - st['exp_avg_sq']).abs().max()) <= 1e-9

    # a NaN in one lane only, then a flagged pair status: nothing moves, both skips are counted
    keep = [x.clone() for x in (p, m, v, t)]
    gl = [torch.randn(n, device=DEV, generator=gen) * 1e-2 for _ in range(lanes)]
    gl[-1][n - 1] = float('nan')
    ops.adam_guarded_step(gl, p, m, v, t, hyper, state)
    gl = [torch.randn(n, device=DEV, generator=gen) * 1e-2 for _ in range(lanes)]
    ops.adam_guarded_step(gl, p, m, v, t, hyper, state,
                          pair_status=torch.tensor([4], dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    for a, b in zip(keep, (p, m, v, t)):
        assert torch.equal(a, b)
    assert state.tolist()[1:] == [2, 4, 1]


def test_adam_step_in_a_captured_graph_follows_lr_and_counts_on_the_device():
    n = 4097
    gen = torch.Generator(device=DEV).manual_seed(5)
    p = torch.randn(n, device=DEV, generator=gen)
    g = torch.randn(n, device=DEV, generator=gen) * 1e-2
    m, v, t = torch.zeros_like(p), torch.zeros_like(p), torch.zeros(1, device=DEV)
    state = torch.zeros(4, dtype=torch.int32, device=DEV)
    hyper = _hyper()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):           # (warm-up outside the capture, then put everything back)
        keep = [x.clone() for x in (p, m, v, t)]
        ops.adam_guarded_step(g, p, m, v, t, hyper, state)
        for dst, src in zip((p, m, v, t), keep):
            dst.copy_(src)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.adam_guarded_step(g, p, m, v, t, hyper, state)
    torch.cuda.synchronize()
    assert float(t) == 0.0                  # capturing ran nothing
    ref_p = torch.nn.Parameter(p.clone())
    ref = torch.optim.Adam([ref_p], lr=0.01, weight_decay=1e-4, foreach=False)
    for k in range(3):
        graph.replay()
        ref_p.grad = g.clone()
        ref.step()
    torch.cuda.synchronize()
    assert float(t) == 3.0
    assert float((p - ref_p.detach()).abs().max()) <= 1e-6
    hyper[0] = 0.005                        # the schedule reaches the captured launch
    ref.param_groups[0]['lr'] = 0.005
    graph.replay()
    ref_p.grad = g.clone()
    ref.step()
    torch.cuda.synchronize()
    assert float((p - ref_p.detach()).abs().max()) <= 1e-6
    hyper[0] = 0.0
    before, m0, v0 = p.clone(), m.clone(), v.clone()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(before, p) and not torch.equal(m0, m) and not torch.equal(v0, v)
    assert float(t) == 5.0 and int(state[1]) == 0


# ---- contrastive loss kernels ----------------------------------------------------------------------------------
def _oracle(a, p, dk, sa, sp, sr, pm, nm, dtype):
    """The package's plain-PyTorch ContrastiveLoss + DetLoss (pinned to the reference by the CPU test) with autograd."""
    ta = torch.tensor(a, dtype=dtype, requires_grad=True)
    tp = torch.tensor(p, dtype=dtype, requires_grad=True)
    tsa = torch.tensor(sa, dtype=dtype, requires_grad=True)
    tsp = torch.tensor(sp, dtype=dtype, requires_grad=True)
    desc, acc, fp, an, _, dists = ContrastiveLoss(pm, nm, 'euclidean', sr)(ta, tp, torch.tensor(dk))
    det = DetLoss('euclidean')(dists, tsa, tsp)
    (desc + det).backward()
    return {'desc': float(desc), 'det': float(det), 'acc': float(acc), 'dists': dists.detach().double().numpy(),
            'fp': np.asarray(list(fp)), 'an': np.asarray(list(an)), 'g_anchor': ta.grad.double().numpy(),
            'g_positive': tp.grad.double().numpy(), 'g_anc_score': tsa.grad.double().numpy(),
            'g_pos_score': tsp.grad.double().numpy()}


def _inputs(M, C=32, seed=0):
    if M in (128, 64):
        z = np.load(GOLDEN)
        k = 'm%d.' % M
        sr, pm, nm = [float(x) for x in z[k + 'params']]
        want = {n: z[k + n] for n in ('desc', 'det', 'acc', 'dists', 'fp', 'an', 'g_anchor', 'g_positive',
                                      'g_anc_score', 'g_pos_score')}
        return (z[k + 'anchor'], z[k + 'positive'], z[k + 'dist_keypts'], z[k + 'anc_score'], z[k + 'pos_score'],
                sr, pm, nm, want)
    rng = np.random.RandomState(seed)
    a = rng.randn(M, C)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    p = a + 0.3 * rng.randn(M, C)
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    dk = rng.rand(M, M) * 0.4
    dk = np.minimum(dk, dk.T)
    dk[3, 5] = dk[5, 3] = 0.1
    return (a.astype(np.float32), p.astype(np.float32), dk, rng.rand(M).astype(np.float32),
            rng.rand(M).astype(np.float32), 0.1, 0.1, 1.4, None)


def _check(out, want, what):
    assert abs(out['desc'] - float(want['desc'])) <= 2e-5 * max(1.0, abs(float(want['desc']))), what
    assert abs(out['det'] - float(want['det'])) <= 2e-5 * max(1.0, abs(float(want['det']))), what
    assert abs(out['acc'] - float(want['acc'])) <= 1e-3, what
    np.testing.assert_allclose(out['dists'], want['dists'], rtol=0, atol=2e-5, err_msg=what)
    np.testing.assert_allclose(out['fp'], want['fp'], rtol=0, atol=2e-5, err_msg=what)
    np.testing.assert_allclose(out['an'], want['an'], rtol=0, atol=2e-5, err_msg=what)
    for n in ('g_anchor', 'g_positive', 'g_anc_score', 'g_pos_score'):
        ref = np.asarray(want[n], np.float64)
        err = np.abs(out[n] - ref).max() / max(1e-12, np.abs(ref).max())
        assert err < 1e-4, (what, n, err)


@pytest.mark.parametrize("M", [128, 64, 37])
def test_contrastive_det_loss_matches_reference_and_f64(M):
    a, p, dk, sa, sp, sr, pm, nm, golden = _inputs(M)
    ta = torch.tensor(a, device=DEV, requires_grad=True)
    tp = torch.tensor(p, device=DEV, requires_grad=True)
    tsa = torch.tensor(sa, device=DEV, requires_grad=True)
    tsp = torch.tensor(sp, device=DEV, requires_grad=True)
    scalars, dists, fp, an = ops.contrastive_det_loss(ta, tp, torch.tensor(dk, device=DEV), tsa, tsp, sr, pm, nm)
    (scalars[0] + scalars[1]).backward()
    torch.cuda.synchronize()
    out = {'desc': float(scalars[0]), 'det': float(scalars[1]), 'acc': float(scalars[2]),
           'dists': dists.double().cpu().numpy(), 'fp': fp.double().cpu().numpy(), 'an': an.double().cpu().numpy(),
           'g_anchor': ta.grad.double().cpu().numpy(), 'g_positive': tp.grad.double().cpu().numpy(),
           'g_anc_score': tsa.grad.double().cpu().numpy(), 'g_pos_score': tsp.grad.double().cpu().numpy()}
    assert abs(float(scalars[5]) - (out['desc'] + out['det'])) <= 1e-5
    if golden is not None:
        _check(out, golden, 'golden M=%d' % M)
    _check(out, _oracle(a, p, dk, sa, sp, sr, pm, nm, torch.float64), 'f64 M=%d' % M)


def _clouds(seed, n0, n1, C=32):
    rng = np.random.RandomState(seed)
    return rng.randn(n0 + n1, C).astype(np.float32), rng.rand(n0 + n1, 1).astype(np.float32)


def _eager_reference(x, s, corr, off, dk, sr, pm, nm):
    """F.normalize + indexing (trainer.py:91-94) + ContrastiveLoss + DetLoss, on the device with autograd."""
    xt = torch.tensor(x, device=DEV, requires_grad=True)
    st = torch.tensor(s, device=DEV, requires_grad=True)
    f = F.normalize(xt, p=2, dim=-1)
    c = torch.tensor(corr, device=DEV)
    desc, acc, fp, an, _, dists = ContrastiveLoss(pm, nm, 'euclidean', sr)(f[c[:, 0]], f[c[:, 1] + off],
                                                                           torch.tensor(dk, device=DEV))
    det = DetLoss('euclidean')(dists, st[c[:, 0]], st[c[:, 1] + off])
    (desc + det).backward()
    return float(desc), float(det), float(acc), xt.grad, st.grad


def test_training_forms_single_and_stacked_match_the_modular_loss():
    M, sr, pm, nm = 64, 0.1, 0.1, 1.4
    sizes = [(300, 280), (250, 310), (400, 200)]
    pairs = []
    for q, (n0, n1) in enumerate(sizes):
        rng = np.random.RandomState(10 + q)
        x, s = _clouds(q, n0, n1)
        corr = np.stack([rng.choice(n0, M, replace=False), rng.choice(n1, M, replace=False)], 1).astype(np.int64)
        x[n0 + corr[:, 1]] = x[corr[:, 0]] + 0.2 * rng.randn(M, 32).astype(np.float32)    # matching descriptors
        dk = rng.rand(M, M) * 0.3
        dk = np.minimum(dk, dk.T)
        pairs.append((x, s, corr, dk, n0))
    # one pair
    x, s, corr, dk, n0 = pairs[0]
    xt = torch.tensor(x, device=DEV, requires_grad=True)
    stt = torch.tensor(s, device=DEV, requires_grad=True)
    total, desc, det, acc, fp, an = ops.train_contrastive_loss(xt, stt, torch.tensor(corr, device=DEV), n0,
                                                               torch.tensor(dk, device=DEV), sr, pm, nm)
    total.backward()
    rd, rt, ra, gx, gs = _eager_reference(x, s, corr, n0, dk, sr, pm, nm)
    assert abs(float(desc) - rd) < 2e-5 and abs(float(det) - rt) < 2e-5 and abs(float(acc) - ra) < 1e-3
    assert abs(float(total) - (rd + rt)) < 4e-5
    assert float((xt.grad - gx).abs().max()) <= 1e-4 * float(gx.abs().max())
    assert float((stt.grad - gs).abs().max()) <= 1e-4 * max(1e-6, float(gs.abs().max()))
    # three pairs stacked into one batch: clouds 2q, 2q + 1 = pair q, every pair its own problem, total = their sum
    xs = np.concatenate([p_[0] for p_ in pairs])
    ss = np.concatenate([p_[1] for p_ in pairs])
    lens = torch.tensor([v for n in sizes for v in n], dtype=torch.int32, device=DEV)
    corr_all = torch.tensor(np.stack([p_[2] for p_ in pairs]), device=DEV)
    dk_all = torch.tensor(np.stack([p_[3] for p_ in pairs]), device=DEV)
    xt = torch.tensor(xs, device=DEV, requires_grad=True)
    stt = torch.tensor(ss, device=DEV, requires_grad=True)
    total, desc, det, acc, fp, an = ops.train_contrastive_loss_pairs(xt, stt, corr_all, lens, dk_all, sr, pm, nm,
                                                                     w_desc=1.0, w_det=0.5)
    total.backward()
    start, want_total = 0, 0.0
    for q, (x, s, corr, dk, n0) in enumerate(pairs):
        n = x.shape[0]
        rd, rt, ra, gx, gs = _eager_reference(x, s, corr, n0, dk, sr, pm, nm)
        assert abs(float(desc[q]) - rd) < 2e-5 and abs(float(det[q]) - rt) < 2e-5 and abs(float(acc[q]) - ra) < 1e-3, q
        want_total += rd + 0.5 * rt
        # the stacked gradient of pair q's rows is pair q's own gradient with det weighted 0.5: re-derive it
        xq = torch.tensor(x, device=DEV, requires_grad=True)
        sq = torch.tensor(s, device=DEV, requires_grad=True)
        f = F.normalize(xq, p=2, dim=-1)
        c = torch.tensor(corr, device=DEV)
        d_, _, _, _, _, dists = ContrastiveLoss(pm, nm, 'euclidean', sr)(f[c[:, 0]], f[c[:, 1] + n0],
                                                                         torch.tensor(dk, device=DEV))
        (d_ + 0.5 * DetLoss('euclidean')(dists, sq[c[:, 0]], sq[c[:, 1] + n0])).backward()
        got = xt.grad[start:start + n]
        assert float((got - xq.grad).abs().max()) <= 1e-4 * float(xq.grad.abs().max()), q
        assert float((stt.grad[start:start + n] - sq.grad).abs().max()) <= 1e-4 * max(1e-6, float(sq.grad.abs().max()))
        start += n
    assert abs(float(total) - want_total) < 1e-4


# ---- training engine -------------------------------------------------------------------------------------------
def test_trainer_adam_contrastive_graph_then_eager_resume(golden_s0, tmp_path):
    """optimizer 'ADAM' + desc_loss 'contrastive' through the Trainer on the pipelined graphs for two epochs; the
    epoch-1 snapshot resumed on the EAGER engine reproduces epoch 2; the snapshot's optimizer loads into
    torch.optim.Adam."""
    from d3feat_pytorch_amd.train import GuardedAdam, TrainStep
    from d3feat_pytorch_amd.trainer import Trainer
    g = golden_s0
    item = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in _item(g))
    swapped = (item[1], item[0], item[3], item[2], item[4].flip(1).contiguous(), item[5].t().contiguous())
    sizes = [int(g['batch.points.%d' % l].shape[0]) for l in range(5)]

    class _Loader:
        dataset, batch_size, shuffle = [item, swapped, item, swapped], 1, False
        limits = [int(x) for x in g['limits']]

    def args(**kw):
        cfg = cfgmod.default_config(first_features_dim=16, num_node=64, optimizer='ADAM', desc_loss='contrastive',
                                    lr=1e-3)
        cfg.max_epoch, cfg.save_dir, cfg.tboard_dir, cfg.device = 2, str(tmp_path / 'snap'), str(tmp_path / 'tb'), DEV
        cfg.train_loader, cfg.val_max_iter, cfg.verbose, cfg.log_interval = _Loader(), 2, True, 2
        cfg.graph_capacities = TrainStep.capacities_for([sizes], slack=1.3)
        cfg.scheduler_gamma = 0.5
        for k, v in kw.items():
            setattr(cfg, k, v)
        return cfg

    tr = Trainer(args(graph=True))
    assert isinstance(tr.optimizer, GuardedAdam)
    tr.train()
    assert tr._captured and tr._get_lr() == 1e-3 * 0.25
    assert int(tr.optimizer.skipped) == 0 and float(tr.optimizer.t) == 8.0     # warm-up steps were put back
    files = sorted(p.name for p in (tmp_path / 'snap').iterdir())
    assert {'model_1.pth', 'model_2.pth'} <= set(files), files

    ref = Trainer(args(graph=False, pretrain=str(tmp_path / 'snap' / 'model_1.pth'), save_dir=str(tmp_path / 'snap2')))
    assert ref.start_epoch == 1 and float(ref.optimizer.t) == 4.0
    avg = ref.train_epoch(2)
    final = torch.load(tmp_path / 'snap' / 'model_2.pth', weights_only=True)
    worst = 0.0
    for k, v in ref.model.state_dict().items():
        worst = max(worst, float((v - final['state_dict'][k].to(DEV)).abs().max()))
    assert worst < 2e-4, worst
    assert 0.0 <= avg['accuracy'] <= 100.0 and avg['d_pos'] > 0 and avg['d_neg'] > 0
    res = ref.evaluate(2)
    assert np.isfinite(res['desc_loss']) and np.isfinite(res['det_loss'])

    model = ref.model
    adam = torch.optim.Adam(model.parameters(), lr=1.0)
    adam.load_state_dict(final['optimizer'])
    assert adam.param_groups[0]['lr'] == 1e-3 * 0.25
    assert all(float(adam.state[p]['step']) == 8.0 for p in model.parameters() if p.requires_grad)


def test_stacked_lanes_adam_update_is_adam_on_the_mean_gradient(golden_s0):
    """PairLanes, 2 lanes x 2 stacked pairs, optimizer 'ADAM' + contrastive: one joint update equals
    torch.optim.Adam applied to the mean of the four pairs' eager single-pair gradients."""
    from d3feat_pytorch_amd.train import PairLanes, TrainStep
    g = golden_s0
    item = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in _item(g))
    swapped = (item[1], item[0], item[3], item[2], item[4].flip(1).contiguous(), item[5].t().contiguous())
    cfg = cfgmod.default_config(first_features_dim=16, num_node=64, optimizer='ADAM', desc_loss='contrastive', lr=1e-3)
    limits = [int(x) for x in g['limits']]
    ts = TrainStep(cfg, limits, torch.device(DEV), seed=0)
    sizes = [int(t.shape[0]) for t in ts.build_batch(item)['points']]
    lanes = PairLanes(ts, 2, stack=2)
    lanes.enable_graph(TrainStep.capacities_for([[2 * n for n in sizes]], slack=1.3), num_corr=int(item[4].shape[0]))
    lanes.capture(item)
    lanes.synchronize()
    torch.cuda.synchronize()
    opt = ts.opt
    p0, m0, v0, t0 = (x.clone() for x in (ts.flat.data, opt.m, opt.v, opt.t))
    group = [item, swapped, swapped, item]
    grads = []
    for it in group:                         # eager single-pair gradients at p0, no update
        batch = ts.build_batch(it)
        batch['n0'] = int(it[0].shape[0])
        ts.flat.zero_grad()
        loss = ts.forward_loss(batch)[0]
        loss.backward()
        grads.append(ts.flat.gather_grads().clone())
    torch.cuda.synchronize()
    assert torch.equal(ts.flat.data, p0)
    mean = sum(grads[1:], grads[0].clone()) / 4
    lanes.step_graph(group, group)
    lanes.synchronize()
    torch.cuda.synchronize()
    assert lanes.check_status() == (0, 0) and int(opt.skipped) == 0 and float(opt.t) == float(t0) + 1
    ref_p = torch.nn.Parameter(p0.clone())
    ref = torch.optim.Adam([ref_p], lr=1e-3, betas=(0.9, 0.999), weight_decay=1e-6, foreach=False)
    ref.state[ref_p] = {'step': t0.cpu().reshape(()).clone(), 'exp_avg': m0.clone(), 'exp_avg_sq': v0.clone()}
    ref_p.grad = mean
    ref.step()
    moved = float((ref_p.detach() - p0).abs().max())
    assert moved > 1e-4
    # Adam's first steps normalise every coordinate (m / sqrt(v) ~ sign(g)): where the mean gradient is at the level of
    # float-atomic noise between the stacked graph and the eager passes, the two updates may differ by up to lr; every
    # coordinate with a gradient above that noise agrees
    diff = (ts.flat.data - ref_p.detach()).abs()
    sig = mean.abs() > 1e-4 * float(mean.abs().max())
    err = float(diff[sig].max())
    assert err < 2e-2 * moved, (err, moved)
    assert float((diff > 1e-2 * moved).float().mean()) < 1e-3
