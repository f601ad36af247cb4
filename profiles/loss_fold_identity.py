"""Bit identity of the training loss across a change of its plumbing: a SHA-256 of every output and gradient of the seven
public loss functions of ops.py (circle_det_loss, contrastive_det_loss, select_normalize, train_loss, train_loss_pairs,
train_contrastive_loss, train_contrastive_loss_pairs) on fixed seeds.

    python profiles/loss_fold_identity.py [root of the tree to import, default: this file's]

Run it in two trees and compare the outputs line by line.  Dense scores; no row is sampled twice, so the float atomics
of the select backward add exactly one value to a cleared element and the gradients are reproducible bits.
Shapes (M, C): training (128, 32), validation (64, 32), the circle loss's one-workgroup route (200, 32) and (16, 96),
and the small case of tests/test_gpu_ops.py (9, 16; clouds of 37 and 41 rows); single pairs and P = 3 stacked (P = 1 for
the small case); weights (1, 1) and (1, 0.5)."""
import hashlib
import os
import sys

ROOT = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from d3feat_pytorch_amd import ops

DEV = "cuda:0"
WEIGHTS = ((1.0, 1.0), (1.0, 0.5))
SHAPES = [("train", 128, 32, [300, 280, 200, 260, 150, 310]), ("valid", 64, 32, [300, 280, 200, 260, 150, 310]),
          ("onewg200", 200, 32, [300, 280, 200, 260, 250, 310]), ("onewg96", 16, 96, [60, 50, 40, 70, 30, 45]),
          ("small", 9, 16, [37, 41])]


def cu(a):
    return torch.as_tensor(a).to(DEV)


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:32]


def report(tag, names, tensors):
    for n, t in zip(names, tensors):
        print("%-44s %-12s %s" % (tag, n, sha(t)))


def inputs(M, C, lens, seed):
    rng = np.random.default_rng(seed)
    P = len(lens) // 2
    N = int(np.sum(lens)) + 5
    x = rng.normal(size=(N, C)).astype(np.float32)
    sc = rng.random((N, 1)).astype(np.float32)
    corr = np.stack([np.stack([rng.permutation(lens[2 * p])[:M], rng.permutation(lens[2 * p + 1])[:M]], 1)
                     for p in range(P)]).astype(np.int64)
    dk = rng.random((P, M, M)) * 0.3
    dk = np.minimum(dk, dk.transpose(0, 2, 1))
    return x, sc, corr, dk


def fused(tag, f, x, sc, args, kw):
    tx, ts = cu(x).requires_grad_(True), cu(sc).requires_grad_(True)
    out = f(tx, ts, *args, **kw)
    out[0].backward()
    report(tag, ("total", "desc", "det", "accuracy", "fp", "an", "grad_x", "grad_scores"), out + (tx.grad, ts.grad))


def standalone(tag, f, a, p, dk, sa, sp):
    ta, tp = cu(a).requires_grad_(True), cu(p).requires_grad_(True)
    tsa, tsp = cu(sa).requires_grad_(True), cu(sp).requires_grad_(True)
    scalars, dists, fp, an = f(ta, tp, cu(dk), tsa, tsp)
    (scalars[0] + 0.5 * scalars[1]).backward()
    report(tag, ("scalars", "dists", "fp", "an", "grad_a", "grad_p", "grad_sa", "grad_sp"),
           (scalars, dists, fp, an, ta.grad, tp.grad, tsa.grad, tsp.grad))


def main():
    torch.zeros(1, device=DEV)
    for name, M, C, lens in SHAPES:
        x, sc, corr, dk = inputs(M, C, lens, 1000 * M + C)
        P, n0 = len(lens) // 2, int(lens[0])
        one = x[:lens[0] + lens[1]], sc[:lens[0] + lens[1]]
        # the standalone operators on the first pair
        tx, ts = cu(one[0]).requires_grad_(True), cu(one[1]).requires_grad_(True)
        c0 = cu(corr[0])
        outs = ops.select_normalize(tx, ts, c0[:, 0], c0[:, 1], n0)
        rng = np.random.default_rng(M)
        cot = [cu(rng.normal(size=tuple(o.shape)).astype(np.float32)) for o in outs]
        torch.autograd.backward(outs, cot)
        report("%s select_normalize" % name, ("out_a", "out_p", "sa", "sp", "grad_x", "grad_scores"),
               tuple(outs) + (tx.grad, ts.grad))
        a, p, sa, sp = [o.detach().cpu().numpy() for o in outs]
        standalone("%s circle_det_loss" % name, ops.circle_det_loss, a, p, dk[0], sa, sp)
        standalone("%s contrastive_det_loss" % name, ops.contrastive_det_loss, a, p, dk[0], sa, sp)
        for w in WEIGHTS:
            kw = dict(w_desc=w[0], w_det=w[1])
            wt = "w=%g,%g" % w
            fused("%s train_loss %s" % (name, wt), ops.train_loss, one[0], one[1], (c0, n0, cu(dk[0])), kw)
            fused("%s train_contrastive_loss %s" % (name, wt), ops.train_contrastive_loss, one[0], one[1],
                  (c0, n0, cu(dk[0])), kw)
            stacked = (cu(corr), cu(np.asarray(lens, np.int32)), cu(dk))
            if M <= 128 and C <= 64:
                fused("%s train_loss_pairs P=%d %s" % (name, P, wt), ops.train_loss_pairs, x, sc, stacked, kw)
            fused("%s train_contrastive_loss_pairs P=%d %s" % (name, P, wt), ops.train_contrastive_loss_pairs, x, sc,
                  stacked, kw)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
