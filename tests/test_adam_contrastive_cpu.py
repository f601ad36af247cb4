"""CPU: the reference's optimizer 'ADAM' and desc_loss 'contrastive' (config.py:51,63, training_3DMatch.py:62-76,
119-132) -- selection, the GuardedAdam host arithmetic against torch.optim.Adam, snapshot interchange in both
directions, and the plain-PyTorch ContrastiveLoss + DetLoss against the reference's recorded outputs."""
import os

import numpy as np
import pytest
import torch

from d3feat_pytorch_amd import config as cfgmod
from d3feat_pytorch_amd.models.architectures import KPFCNN
from d3feat_pytorch_amd.train import FlatParams, GuardedAdam, GuardedSGD, TrainStep
from d3feat_pytorch_amd.trainer import ExponentialLR, Trainer
from d3feat_pytorch_amd.utils.loss import ContrastiveLoss, DetLoss

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "contrastive.npz")
LIMITS = [5, 5, 5, 5, 5]


def _small_model(seed=0):
    np.random.seed(seed)
    torch.manual_seed(seed)
    return KPFCNN(cfgmod.default_config(first_features_dim=16))


def _fake_grads(model, seed, scale=1e-2):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(p.shape, generator=g) * scale if p.requires_grad else None for p in model.parameters()]


class _Loader:
    def __init__(self):
        self.dataset, self.batch_size, self.shuffle, self.limits = [], 1, False, LIMITS


def _args(tmp, **kw):
    cfg = cfgmod.default_config(first_features_dim=16)
    cfg.max_epoch, cfg.save_dir, cfg.tboard_dir, cfg.device, cfg.graph = 2, str(tmp / 'snap'), str(tmp / 'tb'), 'cpu', False
    cfg.train_loader = _Loader()
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _step(cfg, model=None):
    return TrainStep(cfg, LIMITS, torch.device('cpu'), model=model if model is not None else _small_model())


# ---- selection ------------------------------------------------------------------------------------------------
def test_configured_optimizer_and_loss_are_the_ones_trained_with():
    ts = _step(cfgmod.default_config(first_features_dim=16, optimizer='ADAM', desc_loss='contrastive', lr=0.003,
                                     weight_decay=1e-4))
    assert isinstance(ts.opt, GuardedAdam)
    assert ts.desc_loss == 'contrastive'
    assert ts.opt.lr == 0.003 and ts.opt.betas == (0.9, 0.999) and ts.opt.weight_decay == 1e-4 and ts.opt.eps == 1e-8
    assert ts.opt.param_groups[0]['betas'] == (0.9, 0.999)
    default = _step(cfgmod.default_config(first_features_dim=16))
    assert isinstance(default.opt, GuardedSGD) and default.desc_loss == 'circle'


def test_trainer_with_adam_config_holds_guarded_adam(tmp_path):
    tr = Trainer(_args(tmp_path, model=_small_model(), optimizer='ADAM', desc_loss='contrastive'))
    assert isinstance(tr.optimizer, GuardedAdam) and tr.engine.desc_loss == 'contrastive'
    assert isinstance(tr.scheduler, ExponentialLR) and tr._get_lr() == 0.01


@pytest.mark.parametrize("kw", [dict(optimizer='adam'), dict(optimizer='RMSprop'), dict(optimizer=3),
                                dict(desc_loss='triplet'), dict(desc_loss='Circle'),
                                dict(dist_type='cosine'), dict(dist_type='arccosine', desc_loss='circle')])
def test_unknown_choices_are_rejected(kw):
    with pytest.raises(ValueError):
        _step(cfgmod.default_config(first_features_dim=16, **kw))


def test_contrastive_ignores_dist_type_like_the_reference():
    ts = _step(cfgmod.default_config(first_features_dim=16, desc_loss='contrastive', dist_type='cosine'))
    assert ts.desc_loss == 'contrastive'


def test_torch_optimizer_instances_supply_the_hyper_parameters():
    model = _small_model()
    adam = torch.optim.Adam(model.parameters(), lr=0.02, betas=(0.9, 0.999), weight_decay=3e-5)
    ts = _step(cfgmod.default_config(first_features_dim=16, optimizer=adam, lr=0.5), model=model)
    assert isinstance(ts.opt, GuardedAdam)
    assert ts.opt.lr == 0.02 and ts.opt.betas == (0.9, 0.999) and ts.opt.weight_decay == 3e-5
    sgd = torch.optim.SGD(model.parameters(), lr=0.07, momentum=0.9, weight_decay=2e-6)
    ts = _step(cfgmod.default_config(first_features_dim=16, optimizer=sgd), model=model)
    assert isinstance(ts.opt, GuardedSGD) and (ts.opt.lr, ts.opt.momentum, ts.opt.weight_decay) == (0.07, 0.9, 2e-6)
    for bad in (torch.optim.Adam(model.parameters(), amsgrad=True), torch.optim.AdamW(model.parameters())):
        with pytest.raises(ValueError):
            _step(cfgmod.default_config(first_features_dim=16, optimizer=bad), model=model)


# ---- GuardedAdam host arithmetic --------------------------------------------------------------------------------
def _lane_grads(flat, seed, scale=1e-2):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(flat.numel, generator=g) * scale for _ in range(2)]


def _scatter(model, flat_vec):
    out, off = [], 0
    for p in model.parameters():
        if p.requires_grad:
            out.append(flat_vec[off:off + p.numel()].view_as(p).clone())
            off += p.numel()
        else:
            out.append(None)
    return out


def test_guarded_adam_host_path_matches_torch_adam_under_the_schedule():
    ref_model, our_model = _small_model(), _small_model()
    ref = torch.optim.Adam(ref_model.parameters(), lr=0.01, betas=(0.9, 0.999), weight_decay=1e-4)
    ref_sch = torch.optim.lr_scheduler.ExponentialLR(ref, gamma=0.99)
    flat = FlatParams(our_model)
    ours = GuardedAdam(flat, lr=0.01, betas=(0.9, 0.999), weight_decay=1e-4)
    ours.grad_scale = 0.5
    sch = ExponentialLR(ours, gamma=0.99)
    for s in range(200):
        lanes = _lane_grads(flat, s)
        for p, g in zip(ref_model.parameters(), _scatter(ref_model, (lanes[0] + lanes[1]) * 0.5)):
            p.grad = g
        ref.step()
        ok = ours.step(grads=lanes)
        assert bool(ok)
        if s % 10 == 9:
            ref_sch.step()
            sch.step()
    assert ours.lr == ref.param_groups[0]['lr']
    theirs = torch.cat([p.detach().reshape(-1) for p in ref_model.parameters() if p.requires_grad])
    assert float((flat.data - theirs).abs().max()) <= 1e-6
    assert float(ours.t) == 200.0 and int(ours.skipped) == 0


def test_guarded_adam_skips_non_finite_and_flagged_steps_bit_exactly():
    flat = FlatParams(_small_model())
    opt = GuardedAdam(flat, lr=0.01, weight_decay=1e-6)
    for s in range(3):
        assert bool(opt.step(grads=_lane_grads(flat, s)))
    keep = [t.clone() for t in (flat.data, opt.m, opt.v, opt.t)]
    bad = _lane_grads(flat, 7)
    bad[1][123] = float('nan')
    assert not bool(opt.step(grads=bad))
    bad = _lane_grads(flat, 8)
    bad[0][5] = float('inf')
    assert not bool(opt.step(grads=bad))
    assert not bool(opt.step(grads=_lane_grads(flat, 9), pair_status=torch.tensor([8], dtype=torch.int32)))
    for a, b in zip(keep, (flat.data, opt.m, opt.v, opt.t)):
        assert torch.equal(a, b)
    assert opt.state.tolist()[1:] == [3, 8, 1]
    assert float(opt.t) == 3.0


# ---- snapshots ----------------------------------------------------------------------------------------------
def _reference_adam(model, steps, gamma):
    """What the reference's training script builds for optimizer 'ADAM' (training_3DMatch.py:69-81)."""
    opt = torch.optim.Adam(model.parameters(), lr=0.01, betas=(0.9, 0.999), weight_decay=1e-6)
    sch = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=gamma)
    for s in range(steps):
        for p, g in zip(model.parameters(), _fake_grads(model, s)):
            p.grad = g
        opt.step()
        sch.step()
    return opt, sch


def _flat_grad_from(tr, grads):
    flat = tr.engine.flat
    off = 0
    for p, g in zip(tr.model.parameters(), grads):
        if p.requires_grad:
            flat.grad[off:off + p.numel()] = g.reshape(-1)
            off += p.numel()


def test_reference_adam_snapshot_resumes_identically(tmp_path):
    gamma = 0.1 ** (1 / 80)
    ref_model = _small_model()
    ref_opt, ref_sch = _reference_adam(ref_model, steps=3, gamma=gamma)
    path = tmp_path / 'model_3.pth'
    torch.save({'epoch': 3, 'state_dict': ref_model.state_dict(), 'optimizer': ref_opt.state_dict(),
                'scheduler': ref_sch.state_dict(), 'best_loss': 1.5}, path)
    tr = Trainer(_args(tmp_path, model=_small_model(seed=7), optimizer='ADAM', pretrain=str(path)))
    assert tr.start_epoch == 3 and isinstance(tr.optimizer, GuardedAdam) and float(tr.optimizer.t) == 3.0
    assert tr._get_lr() == ref_opt.param_groups[0]['lr']
    grads = _fake_grads(ref_model, 99)
    for p, g in zip(ref_model.parameters(), grads):
        p.grad = g
    ref_opt.step()
    _flat_grad_from(tr, grads)
    assert bool(tr.optimizer.step())
    for (k, a), b in zip(tr.model.state_dict().items(), ref_model.state_dict().values()):
        assert float((a - b).abs().max()) <= 1e-7, k


def test_our_adam_snapshot_continues_in_torch_adam(tmp_path):
    tr = Trainer(_args(tmp_path, model=_small_model(), optimizer='ADAM'))
    for s in range(2):
        _flat_grad_from(tr, _fake_grads(tr.model, s))
        tr.optimizer.step()
    tr.scheduler.step()
    path = tr._snapshot(1)
    state = torch.load(path, weights_only=True)
    ref_model = _small_model(seed=5)
    ref_model.load_state_dict(state['state_dict'])
    ref_opt = torch.optim.Adam(ref_model.parameters(), lr=0.01, betas=(0.9, 0.999), weight_decay=1e-6)
    ref_opt.load_state_dict(state['optimizer'])
    assert ref_opt.param_groups[0]['lr'] == tr._get_lr()
    assert all(float(ref_opt.state[p]['step']) == 2.0 for p in ref_model.parameters() if p.requires_grad)
    grads = _fake_grads(ref_model, 42)
    for p, g in zip(ref_model.parameters(), grads):
        p.grad = g
    ref_opt.step()
    _flat_grad_from(tr, grads)
    tr.optimizer.step()
    for (k, a), b in zip(tr.model.state_dict().items(), ref_model.state_dict().values()):
        assert float((a - b).abs().max()) <= 1e-7, k


def test_foreign_optimizer_layouts_are_rejected():
    model = _small_model()
    flat = FlatParams(model)
    opt = GuardedAdam(flat)
    sgd = torch.optim.SGD(model.parameters(), lr=0.01, momentum=0.98)
    for p, g in zip(model.parameters(), _fake_grads(model, 0)):
        p.grad = g
    sgd.step()
    with pytest.raises(ValueError):
        opt.load_state_dict(sgd.state_dict())
    for kw in (dict(amsgrad=True), dict(maximize=True)):
        other = torch.optim.Adam(model.parameters(), **kw)
        with pytest.raises(ValueError):
            opt.load_state_dict(other.state_dict())
    adamw = torch.optim.AdamW(model.parameters())
    with pytest.raises(ValueError):
        opt.load_state_dict(adamw.state_dict())
    good = torch.optim.Adam(model.parameters())
    good.step()
    sd = good.state_dict()
    opt.load_state_dict(sd)                         # the well-formed one loads
    first = next(iter(sd['state']))
    uneven = {'state': {k: dict(v) for k, v in sd['state'].items()}, 'param_groups': sd['param_groups']}
    uneven['state'][first]['step'] = torch.tensor(5.0)
    with pytest.raises(ValueError):
        opt.load_state_dict(uneven)
    shaped = {'state': {k: dict(v) for k, v in sd['state'].items()}, 'param_groups': sd['param_groups']}
    shaped['state'][first]['exp_avg'] = torch.zeros(3, 3, 3)
    with pytest.raises(ValueError):
        opt.load_state_dict(shaped)
    short = {'state': {}, 'param_groups': [dict(sd['param_groups'][0], params=[0, 1, 2])]}
    with pytest.raises(ValueError):
        opt.load_state_dict(short)


# ---- the contrastive loss's oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("M", [128, 64])
def test_contrastive_and_det_loss_equal_the_reference_recording(M):
    z = np.load(GOLDEN)
    k = 'm%d.' % M
    sr, pm, nm = [float(x) for x in z[k + 'params']]
    a = torch.tensor(z[k + 'anchor'], requires_grad=True)
    p = torch.tensor(z[k + 'positive'], requires_grad=True)
    sa = torch.tensor(z[k + 'anc_score'], requires_grad=True)
    sp = torch.tensor(z[k + 'pos_score'], requires_grad=True)
    desc, acc, fp, an, _, dists = ContrastiveLoss(pm, nm, 'euclidean', sr)(a, p, torch.tensor(z[k + 'dist_keypts']))
    det = DetLoss('euclidean')(dists, sa, sp)
    (desc + det).backward()
    assert abs(float(desc) - float(z[k + 'desc'])) <= 1e-6
    assert abs(float(det) - float(z[k + 'det'])) <= 1e-6
    assert float(acc) == float(z[k + 'acc'])
    np.testing.assert_allclose(dists.detach().numpy(), z[k + 'dists'], rtol=0, atol=1e-6)
    np.testing.assert_allclose(np.asarray(list(fp)), z[k + 'fp'], rtol=0, atol=1e-6)
    np.testing.assert_allclose(np.asarray(list(an)), z[k + 'an'], rtol=0, atol=1e-6)
    for name, t in (('g_anchor', a), ('g_positive', p), ('g_anc_score', sa), ('g_pos_score', sp)):
        np.testing.assert_allclose(t.grad.numpy(), z[k + name], rtol=0, atol=1e-7, err_msg=name)

