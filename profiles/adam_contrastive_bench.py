"""Times the guarded Adam step against the guarded SGD step on a full-width model's flat buffer, the contrastive +
detector loss launches against the plain-PyTorch ContrastiveLoss + DetLoss at M = 128, and one pair per step
(Trainer defaults: the captured step) with ADAM + contrastive against SGD + circle.

    python profiles/adam_contrastive_bench.py [--reps 50]
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python profiles/adam_contrastive_bench.py --reps 20 --no-step

Optimizer times: torch events around back-to-back calls after warm-up (median of reps), one gradient lane.  Share of
the HBM bound: the byte counts of csrc/optimizer.hip (Adam 16 B read + 12 B written per parameter + 4 B guard; SGD
12 B + 8 B + 4 B) over the MI355X's 8 TB/s peak.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import d3feat_pytorch_amd  # noqa: E402,F401
from d3feat_pytorch_amd import config as cfgmod, ops, synthetic  # noqa: E402
from d3feat_pytorch_amd.datasets import dataloader as dl  # noqa: E402
from d3feat_pytorch_amd.models.architectures import KPFCNN  # noqa: E402
from d3feat_pytorch_amd.utils.loss import ContrastiveLoss, DetLoss  # noqa: E402

HBM_PEAK = 8.0e12
DEV = torch.device('cuda')


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out)), float(min(out))


def optimizer_steps(reps):
    n = sum(p.numel() for p in KPFCNN(cfgmod.default_config()).parameters() if p.requires_grad)
    g = torch.randn(n, device=DEV) * 1e-3
    p = torch.randn(n, device=DEV)
    buf, m, v = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    t = torch.zeros(1, device=DEV)
    state = torch.zeros(4, dtype=torch.int32, device=DEV)
    hs = torch.tensor([0.0, 0.98, 1e-6, 1.0], device=DEV)              # lr 0: the buffers stay finite over the reps
    ha = torch.tensor([0.0, 0.9, 0.999, 1e-8, 1e-6, 1.0], dtype=torch.float64, device=DEV)
    res = {'params': n}
    for name, fn, nbytes in (
            ('sgd', lambda: ops.sgd_guarded_step(g, p, buf, 0.0, 0.98, 1e-6, state, hyper=hs), 24 * n),
            ('adam', lambda: ops.adam_guarded_step(g, p, m, v, t, ha, state), 32 * n)):
        med, best = timed(fn, reps)
        res[name] = {'ms': med, 'ms_min': best, 'bytes': nbytes, 'GBps': nbytes / med * 1e-6,
                     'share_of_hbm_bound': nbytes / (med * 1e-3) / HBM_PEAK}
        print("%-4s step, %.1fM parameters: %.3f ms (min %.3f), %.2f GB -> %.0f GB/s = %.1f %% of the 8 TB/s bound"
              % (name, n * 1e-6, med, best, nbytes * 1e-9, nbytes / med * 1e-6, 100 * res[name]['share_of_hbm_bound']))
    return res


def losses(reps, M=128, C=32):
    rng = np.random.RandomState(0)
    a = torch.nn.functional.normalize(torch.tensor(rng.randn(M, C), dtype=torch.float32, device=DEV), dim=1)
    pp = torch.nn.functional.normalize(a + 0.3 * torch.randn(M, C, device=DEV), dim=1)
    dk = torch.tensor(rng.rand(M, M) * 0.4, dtype=torch.float64, device=DEV)
    sa, sp = torch.rand(M, device=DEV), torch.rand(M, device=DEV)
    ta, tp = a.clone().requires_grad_(True), pp.clone().requires_grad_(True)
    tsa, tsp = sa.clone().requires_grad_(True), sp.clone().requires_grad_(True)

    def fused():
        s = ops.contrastive_det_loss(ta, tp, dk, tsa, tsp, 0.1, 0.1, 1.4)[0]
        (s[0] + s[1]).backward()

    closs, dloss = ContrastiveLoss(0.1, 1.4, 'euclidean', 0.1), DetLoss('euclidean')

    def plain():
        desc, _, _, _, _, dists = closs(ta, tp, dk)
        (desc + dloss(dists, tsa, tsp)).backward()
    res = {}
    for name, fn in (('fused', fused), ('pytorch', plain)):
        med, best = timed(fn, reps)
        res[name] = {'ms': med, 'ms_min': best}
        print("contrastive + detector loss, M = %d, forward + backward, %-7s: %.3f ms (min %.3f)" % (M, name, med, best))
    return res


def one_pair_steps(reps):
    from d3feat_pytorch_amd.train import TrainStep

    def gpu_subsample(points, lengths, dlen):
        q, b = dl.batch_grid_subsampling_kpconv(torch.as_tensor(points).to(DEV), torch.as_tensor(lengths).to(DEV),
                                                sampleDl=dlen)
        return q.cpu().numpy(), b.cpu().numpy()
    raw = synthetic.make_pair(1, 2, gpu_subsample)
    item = tuple(torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in raw)
    limits = [40, 40, 40, 40, 30]
    res = {}
    for name, kw in (('sgd_circle', {}), ('adam_contrastive', dict(optimizer='ADAM', desc_loss='contrastive'))):
        cfg = cfgmod.default_config(**kw)
        ts = TrainStep(cfg, limits, DEV, seed=0)
        ts.opt.lr = 0.0
        sizes = [[int(x.shape[0]) for x in ts.build_batch(item)['points']]]
        ts.enable_graph(TrainStep.capacities_for(sizes, slack=1.0), num_corr=int(item[4].shape[0]))
        ts.capture(item)
        import time
        for _ in range(3):
            ts.step_graph(item, item)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):                # pipelined steps back to back (two streams): wall time per step
            ts.step_graph(item, item)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / reps
        ts.check_status()
        res[name] = {'ms': ms}
        print("one pair per step, captured step, %-16s: %.3f ms per step" % (name, ms))
        del ts
        torch.cuda.synchronize()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--no-step', action='store_true', help="skip the captured training steps (profiler runs)")
    a = ap.parse_args()
    out = {'device': torch.cuda.get_device_properties(0).gcnArchName}
    out['optimizer'] = optimizer_steps(a.reps)
    out['loss'] = losses(a.reps)
    if not a.no_step:
        out['step'] = one_pair_steps(a.reps)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
