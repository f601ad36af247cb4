"""What the deterministic mode costs, measured: the one-pair schedule and one stack of three pairs at the S1 size with the
mode off and on (graph replay, the arms taking turns in one run, device events, medians with ranges), and every replaced
launch beside the float-atomic form it replaces.  Writes profiles/deterministic_bench.txt.
Run on the GPU box: python profiles/deterministic_bench.py [--turns 7] [--steps 10]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from d3feat_pytorch_amd import _native, config as cfgmod, ops, synthetic
from d3feat_pytorch_amd.datasets import dataloader as dl
from d3feat_pytorch_amd.train import TrainStep

DEV = torch.device("cuda:0")
OUT = []


def say(line=""):
    print(line, flush=True)
    OUT.append(line)


def med_range(v):
    v = sorted(v)
    return "%8.3f  [%8.3f .. %8.3f]" % (v[len(v) // 2], v[0], v[-1])


def time_us(fn, inner=20, reps=9):
    """Median device time of one fn() in us: `inner` calls between two events, `reps` times."""
    for _ in range(3):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        out.append(1e3 * e0.elapsed_time(e1) / inner)
    return sorted(out)[len(out) // 2]


def gpu_subsample(points, lengths, dlen):
    p, b = dl.batch_grid_subsampling_kpconv(torch.as_tensor(points).to(DEV), torch.as_tensor(lengths).to(DEV), sampleDl=dlen)
    return p.cpu().numpy(), b.cpu().numpy()


def engine(cfg, limits, item, sizes, stack, deterministic):
    np.random.seed(0)
    torch.manual_seed(0)
    t = TrainStep(cfg, limits, DEV, seed=0, deterministic=deterministic)
    t.opt.lr = 0.0              # the parameters stay where they are: every replay does the same work
    caps = TrainStep.capacities_for([[stack * n for n in sizes]], slack=1.0)
    t.enable_graph(caps, num_corr=int(item[4].shape[0]), stack=stack)
    feed = tuple([item] * stack) if stack > 1 else item
    t.capture(feed)
    torch.cuda.synchronize()
    return t, feed


def step_times(arms, turns, steps):
    """{name: [ms per step]} -- the arms take turns; one figure per turn: `steps` replays between two device events."""
    res = {name: [] for name, _, _ in arms}
    for name, t, feed in arms:
        for _ in range(3):
            t.step_graph(feed, feed)
    torch.cuda.synchronize()
    for _ in range(turns):
        for name, t, feed in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                t.step_graph(feed, feed)
            e1.record()
            e1.synchronize()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) / steps)
    return res


def replaced_launches(cfg, limits, item):
    """Every launch the mode replaces, on the tables and shapes of the S1 pair's own pyramid, beside its atomic form."""
    L = _native.lib()
    s = torch.cuda.current_stream().cuda_stream
    p = ops._p
    np.random.seed(0)
    torch.manual_seed(0)
    t = TrainStep(cfg, limits, DEV, seed=0)
    batch = t.build_batch(item)
    say("%-44s %12s %12s" % ("launch (us, median of 9 x 20)", "atomic form", "ordered form"))
    width = cfg.first_features_dim
    for l, tab in enumerate(batch['pools']):
        if not tab.shape[0]:
            continue
        ns, nq, c = int(batch['points'][l].shape[0]), int(tab.shape[0]), width * 2 ** l
        go = torch.randn((nq, c), device=DEV)
        x = torch.randn((ns, c), device=DEV)
        out, arg = torch.empty((nq, c), device=DEV), torch.empty((nq, c), dtype=torch.int32, device=DEV)
        _native.check(L.d3f_max_pool_forward(p(x), ns, c, p(tab), nq, int(tab.shape[1]), p(out), p(arg), None, None, None, 0,
                                             0, s), "fwd")
        gx = torch.empty((ns, c), device=DEV)
        ptr, ent = ops._csr_of(tab, ns)
        a = time_us(lambda: L.d3f_max_pool_backward(p(go), p(arg), nq, c, ns, p(gx), 0, s))
        b = time_us(lambda: L.d3f_max_pool_backward_gather(p(go), p(arg), nq, c, ns, p(ptr), p(ent), None, p(gx), s))
        r = time_us(lambda: ops._csr_of(tab, ns), inner=5)
        say("%-44s %12.1f %12.1f   (+ %.1f transposing the table)" % ("max_pool bwd %d -> %d x %d" % (nq, ns, c), a, b, r))
    for l, tab in enumerate(batch['upsamples']):
        if not tab.shape[0]:
            continue
        nq, ns, c = int(tab.shape[0]), int(batch['points'][l + 1].shape[0]), width * 2 ** l
        go = torch.randn((nq, c), device=DEV)
        gx = torch.empty((ns, c), device=DEV)
        col0 = tab[:, :1].contiguous()
        ptr, ent = ops._csr_of(col0, ns)
        a = time_us(lambda: L.d3f_closest_pool_backward(p(go), c, p(tab), nq, int(tab.shape[1]), c, ns, p(gx), 0, s))
        b = time_us(lambda: L.d3f_closest_pool_backward_gather(p(go), c, nq, c, ns, p(ptr), p(ent), p(gx), s))
        r = time_us(lambda: ops._csr_of(tab[:, :1].contiguous(), ns), inner=5)
        say("%-44s %12.1f %12.1f   (+ %.1f transposing column 0)" % ("closest_pool bwd %d -> %d x %d" % (nq, ns, c), a, b, r))
    for l, pts in enumerate(batch['points']):
        n, c = int(pts.shape[0]), width * 2 ** l
        if n >= 4096:
            continue
        go, out = torch.randn((n, c), device=DEV), torch.randn((n, c), device=DEV)
        gm, gb = torch.empty((n, c), device=DEV), torch.zeros(c, device=DEV)
        nws = int(L.d3f_bias_act_backward_ordered_ws_bytes(n, c))
        ws = ops._ws(nws, DEV)
        a = time_us(lambda: L.d3f_bias_act_backward(p(go), p(out), 0.1, n, c, p(gm), p(gb), None, 1, None, None, 0, s))
        b = time_us(lambda: L.d3f_bias_act_backward_ordered(p(go), p(out), 0.1, n, c, p(gm), p(gb), None, None, p(ws), nws, s))
        say("%-44s %12.1f %12.1f" % ("bias_act bwd %d x %d" % (n, c), a, b))
    # the loss node's sparse backward and the few-point KPConv grad-inputs: the profiler regions of one eager step per mode
    rows = {}
    for mode in (False, True):
        np.random.seed(0)
        torch.manual_seed(0)
        eng = TrainStep(cfg, limits, DEV, seed=0, deterministic=mode)
        eng.opt.lr = 0.0
        for _ in range(2):
            eng.step(item)
        prof = ops.EventProfiler()
        ops.set_profiler(prof)
        for _ in range(5):
            eng.step(item)
        ops.set_profiler(None)
        rows[mode] = prof.summary()
    say()
    say("profiler regions of five eager steps per mode (us per call; a region is bracketed by events on the launch stream)")
    keys = ("kpconv_dx_scatter", "kpconv_dx_gather", "kpconv_agg_transposed", "kpconv_ordered", "detection_rows_bwd",
            "loss_rows_bwd_ordered", "max_pool_bwd_gather", "closest_pool_bwd_gather", "reverse_table")
    for mode in (False, True):
        say("  mode %s" % ("on" if mode else "off"))
        for label, d in sorted(rows[mode].items()):
            if label.startswith(keys):
                say("    %-52s calls %3d  %9.1f us" % (label, d["calls"], 1e3 * d["avg_ms"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--turns", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    args = ap.parse_args()
    g = np.load(os.path.join(ROOT, "tests", "golden", "s1_full.npz"), allow_pickle=False)
    limits = [int(x) for x in g['limits']]
    cfg = cfgmod.default_config()
    item = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in synthetic.make_pair(1, 2, gpu_subsample))
    probe = TrainStep(cfg, limits, DEV, seed=0)
    sizes = [int(t.shape[0]) for t in probe.build_batch(item)['points']]
    del probe
    say("deterministic mode at the S1 size: level sizes %s, %s" % (sizes, torch.cuda.get_device_name(0)))
    say("graph-replayed step, ms per step: median [min .. max] of %d turns of %d replays; the arms take turns" % (
        args.turns, args.steps))
    for stack in (1, 3):
        arms = []
        for name, mode in (("off", False), ("on", True), ("off (again)", False)):
            t, feed = engine(cfg, limits, item, sizes, stack, mode)
            arms.append((name, t, feed))
        res = step_times(arms, args.turns, args.steps)
        for name, _, _ in arms:
            say("  %d pair(s) per step, mode %-12s %s ms" % (stack, name, med_range(res[name])))
        off, on = sorted(res["off"])[len(res["off"]) // 2], sorted(res["on"])[len(res["on"]) // 2]
        say("  %d pair(s) per step: on / off = %.3f (medians)" % (stack, on / off))
        del arms
        torch.cuda.empty_cache()
    say()
    replaced_launches(cfg, limits, item)
    with open(os.path.join(ROOT, "profiles", "deterministic_bench.txt"), "w") as f:
        f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
