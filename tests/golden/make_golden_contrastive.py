#!/usr/bin/env python
"""The reference's batch-hard contrastive loss + detector loss, recorded (data only):

    python tests/golden/make_golden_contrastive.py REFERENCE_ROOT    ->  tests/golden/contrastive.npz

REFERENCE_ROOT is a checkout of the reference; its utils/loss.py is run on the CPU with autograd:
``ContrastiveLoss(pos_margin, neg_margin, metric='euclidean', safe_radius)`` (what training_3DMatch.py:119-125 builds
for desc_loss 'contrastive') and ``DetLoss('euclidean')`` on the contrastive's dists (trainer.py:96-98).

  m<M>.{anchor,positive}          [M,C] f32 unit descriptors (what F.normalize hands the loss)
  m<M>.{anc_score,pos_score}      [M] f32 detector scores
  m<M>.dist_keypts                [M,M] f64 keypoint distances; some entries are exactly safe_radius
  m<M>.params                     [safe_radius, pos_margin, neg_margin]
  m<M>.{desc,det,acc}             the two losses and the accuracy
  m<M>.{dists,fp,an}              dists [M,M] (with the +10s), furthest positive, average negative
  m<M>.{g_anchor,g_positive,g_anc_score,g_pos_score}   gradients of desc + det
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SAFE_RADIUS, POS_MARGIN, NEG_MARGIN = 0.1, 0.1, 1.4


def load_reference_loss(ref_root):
    spec = importlib.util.spec_from_file_location("ref_loss", os.path.join(ref_root, "utils", "loss.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_inputs(M, C, seed):
    rng = np.random.RandomState(seed)
    a = rng.randn(M, C)
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    # positives near their anchors, a few far (misses), a few anchors' neighbours close (hard negatives)
    p = a + rng.randn(M, C) * rng.choice([0.05, 0.3, 1.0], size=(M, 1), p=[0.5, 0.35, 0.15])
    p[M // 2:M // 2 + 4] = a[M // 2 + 1:M // 2 + 5] + 0.01 * rng.randn(4, C)
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    pts = rng.rand(M, 3) * 0.6
    dk = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1))
    dk = np.minimum(dk, dk.T)
    iu = np.triu_indices(M, 1)
    pick = rng.choice(len(iu[0]), size=12, replace=False)
    dk[iu[0][pick], iu[1][pick]] = SAFE_RADIUS          # exactly on the radius: not near (strict <)
    dk[iu[1][pick], iu[0][pick]] = SAFE_RADIUS
    np.fill_diagonal(dk, 0.0)
    sa = rng.rand(M).astype(np.float32) * 0.5 + 0.1
    sp = rng.rand(M).astype(np.float32) * 0.5 + 0.1
    return a.astype(np.float32), p.astype(np.float32), dk.astype(np.float64), sa, sp


def run(ref, a, p, dk, sa, sp):
    ta = torch.tensor(a, requires_grad=True)
    tp = torch.tensor(p, requires_grad=True)
    tsa = torch.tensor(sa, requires_grad=True)
    tsp = torch.tensor(sp, requires_grad=True)
    loss = ref.ContrastiveLoss(pos_margin=POS_MARGIN, neg_margin=NEG_MARGIN, metric='euclidean',
                               safe_radius=SAFE_RADIUS)
    desc, acc, fp, an, _, dists = loss(ta, tp, torch.tensor(dk))
    det = ref.DetLoss('euclidean')(dists, tsa, tsp)
    (desc + det).backward()
    return {'desc': np.float32(desc.item()), 'det': np.float32(det.item()), 'acc': np.float32(float(acc)),
            'dists': dists.detach().numpy().astype(np.float32), 'fp': np.asarray(fp, np.float32),
            'an': np.asarray(an, np.float32), 'g_anchor': ta.grad.numpy(), 'g_positive': tp.grad.numpy(),
            'g_anc_score': tsa.grad.numpy(), 'g_pos_score': tsp.grad.numpy()}


def main(ref_root):
    ref = load_reference_loss(ref_root)
    out = {}
    for M, seed in ((128, 1), (64, 2)):
        a, p, dk, sa, sp = make_inputs(M, 32, seed)
        res = run(ref, a, p, dk, sa, sp)
        key = 'm%d.' % M
        out.update({key + 'anchor': a, key + 'positive': p, key + 'anc_score': sa, key + 'pos_score': sp,
                    key + 'dist_keypts': dk, key + 'params': np.array([SAFE_RADIUS, POS_MARGIN, NEG_MARGIN])})
        out.update({key + k: v for k, v in res.items()})
    path = os.path.join(HERE, 'contrastive.npz')
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == '__main__':
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
