"""Times ops.knn_match (k = 1, 2, 4, 8) against ops.mutual_nn and against the only route to k nearest descriptors that
existed before it: torch.topk of the materialised 2 - 2 S T^T.  Writes profiles/knn_match_bench.txt (--out).

    python profiles/knn_match_bench.py [--windows 10] [--out profiles/knn_match_bench.txt]

Shapes: one pair of 19000 x 19000 x 32 (a whole 3DMatch fragment pair) and 8 pairs of 5000 x 5000 x 32 in one batched
call (the inference batch).  Descriptors are random unit rows.  A window is `calls` back-to-back calls between two
device events (20 for the kernels, 2 for the torch route, which is far slower); the arms take turns inside one loop, 3
warm-up rounds, then medians with (min .. max) of the windows, in ms per call.  The torch route needs the N x N matrix
(1.4 GB at 19000 x 19000); its time includes forming it.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import d3feat_pytorch_amd  # noqa: E402,F401
from d3feat_pytorch_amd import ops  # noqa: E402

WARMUP = 3


def unit_rows(n, C, seed):
    g = torch.Generator(device='cpu').manual_seed(seed)
    x = torch.randn((n, C), generator=g)
    return (x / x.norm(dim=1, keepdim=True)).cuda().contiguous()


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def measure(title, arms, windows, lines):
    times = {name: [] for name, _, _ in arms}
    for rnd in range(WARMUP + windows):
        for name, fn, calls in arms:
            ms = window(fn, calls)
            if rnd >= WARMUP:
                times[name].append(ms)
    lines.append(title)
    base = np.median(times['mutual_nn'])
    for name, _, calls in arms:
        t = np.array(times[name])
        lines.append("  %-28s %9.3f ms (%.3f .. %.3f)   %6.2f x mutual_nn   [%d calls per window]"
                     % (name, np.median(t), t.min(), t.max(), np.median(t) / base, calls))
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=10)
    ap.add_argument('--rows', type=int, default=19000)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'knn_match_bench.txt'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("knn_match_bench.py measures on the GPU; there is none")
    if a.windows < 10:
        raise SystemExit("at least 10 windows")
    lines = ["knn_match_bench.py on %s: ms per call from device events, median (min .. max) of %d windows after %d "
             "warm-up rounds, arms alternating" % (torch.cuda.get_device_properties(0).gcnArchName, a.windows, WARMUP), ""]
    N, C = a.rows, 32
    S, T = unit_rows(N, C, 1), unit_rows(N, C, 2)

    def torch_route(k):
        def run():
            d = 2.0 - 2.0 * (S @ T.t())
            return torch.topk(d, k, dim=1, largest=False)
        return run
    arms = [('mutual_nn', lambda: ops.mutual_nn(S, T), 20)]
    arms += [('knn_match k=%d' % k, (lambda k: lambda: ops.knn_match(S, T, k))(k), 20) for k in (1, 2, 4, 8)]
    arms += [('torch.topk(2 - 2 S T^T) k=%d' % k, torch_route(k), 2) for k in (1, 8)]
    measure("one pair, %d x %d x %d" % (N, N, C), arms, a.windows, lines)

    P, n = 8, 5000
    D = unit_rows(2 * P * n, C, 3)
    seg = torch.tensor([[2 * p * n, n, (2 * p + 1) * n, n] for p in range(P)], dtype=torch.int32).cuda().contiguous()
    Sb = torch.stack([D[2 * p * n:(2 * p + 1) * n] for p in range(P)])
    Tb = torch.stack([D[(2 * p + 1) * n:(2 * p + 2) * n] for p in range(P)])

    def torch_batched(k):
        def run():
            d = 2.0 - 2.0 * torch.bmm(Sb, Tb.transpose(1, 2))
            return torch.topk(d, k, dim=2, largest=False)
        return run
    arms = [('mutual_nn', lambda: ops.mutual_nn_batched(D, D, seg, n, n), 20)]
    arms += [('knn_match k=%d' % k, (lambda k: lambda: ops.knn_match_batched(D, D, seg, n, n, k))(k), 20) for k in (1, 2, 4, 8)]
    arms += [('torch.topk(2 - 2 S T^T) k=%d' % k, torch_batched(k), 2) for k in (1, 8)]
    measure("%d pairs of %d x %d x %d, one batched call" % (P, n, n, C), arms, a.windows, lines)

    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        fh.write(text + "\n")


if __name__ == '__main__':
    main()
