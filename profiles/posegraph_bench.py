"""Times the pose-graph optimisation (ops.pose_graph_optimize, csrc/posegraph.hip: one workgroup per graph) at the size
of a benchmark scene (tests/golden/posegraph_lab_hj.npz, 38 nodes / 77 edges, 15 % of the loop edges corrupted) and at
60 nodes / 500 edges (a synthetic ring with random chords, 10 % of them corrupted):

  * the device call for G = 1 and G = 8 stacked copies -- device events around REPEAT calls after a warm-up, and the
    host clock around one call that ends in a synchronise (what a caller waits for);
  * the host twin (the same text run by one CPU thread) and registration.pose_graph_numpy, host clock;
  * how the kernel's time splits between its phases, from the wave clock d3f_debug_set_phase_clock arms (shader-clock
    laps of wave 0 of the workgroup; a run of its own, the timed runs have the clock idle).

    python profiles/posegraph_bench.py            ->  profiles/posegraph_bench.txt

Needs the GPU; there is no fallback."""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

import posegraph_cases as pc  # noqa: E402
from d3feat_pytorch_amd import _native, ops  # noqa: E402
from d3feat_pytorch_amd.geometric_registration import registration as reg  # noqa: E402

REPEAT, WARMUP = 50, 5
PHASES = ['setup (checks, components, incidence, mu)', 'edge blocks and their energy', 'assembly of H and g',
          'factorisation (copy + damping + Cholesky)', 'forward and back substitution',
          'trial poses, their energy, the decision']


def dense_graph(N=60, E=500, seed=0, corrupt=0.1):
    """A ring of N nodes plus random chords up to E edges; ``corrupt`` of the chords get a gross error."""
    rng = np.random.default_rng(seed)
    truth = np.stack([pc.exp(rng.normal(0, 1.0, 3), rng.normal(0, 0.8, 3)) for _ in range(N)])
    pairs = {(k, k + 1) for k in range(N - 1)}
    while len(pairs) < E:
        i, j = sorted(rng.choice(N, 2, replace=False).tolist())
        pairs.add((i, j))
    edges = np.array(sorted(pairs), dtype=np.int64)
    unc = edges[:, 1] - edges[:, 0] > 1
    Z = np.stack([np.linalg.inv(truth[i]) @ truth[j] for i, j in edges])
    info = np.stack([pc.point_information(rng) for _ in edges])
    loops = np.nonzero(unc)[0]
    bad = sorted(rng.choice(loops, int(corrupt * len(loops)), replace=False).tolist())
    for e in bad:
        Z[e] = Z[e] @ pc.exp(rng.uniform(0.3, 1.0, 3) * rng.choice([-1.0, 1.0], 3), rng.normal(0, 0.5, 3))
    P0 = truth.copy()
    for k in range(1, N):
        P0[k] = P0[k] @ pc.exp(rng.normal(0, 0.05, 3), rng.normal(0, np.deg2rad(3), 3))
    return dict(N=N, edges=edges, Z=Z, info=info, unc=unc, truth=truth, poses0=P0, bad=bad)


def device_args(g, G):
    P0, edges, Z, info, unc, ns, es = pc.stack([g] * G)
    dev = torch.device('cuda')
    args = (torch.from_numpy(P0).to(dev), torch.from_numpy(edges.astype(np.int32)).to(dev), torch.from_numpy(Z).to(dev),
            torch.from_numpy(info).to(dev), torch.from_numpy(unc.astype(np.int32)).to(dev), pc.MAX_DISTANCE)
    kw = dict(node_start=torch.from_numpy(ns.astype(np.int32)).to(dev),
              edge_start=torch.from_numpy(es.astype(np.int32)).to(dev), max_nodes=g['N'], max_edges=len(g['edges']))
    return args, kw


def time_device(g, G):
    args, kw = device_args(g, G)
    for _ in range(WARMUP):
        out = ops.pose_graph_optimize(*args, **kw)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPEAT):
        out = ops.pose_graph_optimize(*args, **kw)
    e1.record()
    torch.cuda.synchronize()
    waits = []
    for _ in range(REPEAT):
        t = time.perf_counter()
        out = ops.pose_graph_optimize(*args, **kw)
        torch.cuda.synchronize()
        waits.append(time.perf_counter() - t)
    return e0.elapsed_time(e1) / REPEAT, 1e3 * float(np.median(waits)), 1e3 * float(np.min(waits)), out


def phase_shares(g):
    args, kw = device_args(g, 1)
    clk = torch.zeros(8 + 8 * 64, dtype=torch.int64, device='cuda')
    clk[1] = 64
    lib = _native.lib()
    lib.d3f_debug_set_phase_clock(clk.data_ptr())
    try:
        ops.pose_graph_optimize(*args, **kw)
        torch.cuda.synchronize()
    finally:
        lib.d3f_debug_set_phase_clock(None)
    rec = clk.cpu().numpy()
    laps = rec[8:8 + 8 * int(rec[0])].reshape(-1, 8)[:, :6].astype(np.float64)
    return laps.mean(0) / laps.mean(0).sum(), int(rec[0])


def main():
    assert torch.cuda.is_available(), "posegraph_bench.py needs the GPU"
    lines = ["pose-graph optimisation: %s, torch %s" % (torch.cuda.get_device_properties(0).gcnArchName,
                                                       torch.__version__),
             "device: mean of %d calls between device events after %d warm-up calls; 'wait' = host clock around one "
             "call + synchronise (median / min of %d)" % (REPEAT, WARMUP, REPEAT), ""]
    for name, g in (("fixture 38 nodes / 77 edges", pc.fixture_graph(0.15, 0)), ("ring 60 nodes / 500 edges",
                                                                                  dense_graph())):
        lines.append("%s, %d corrupted edges" % (name, len(g['bad'])))
        ref = None
        for G in (1, 8):
            ms, wait_med, wait_min, out = time_device(g, G)
            out = [t.cpu().numpy() for t in out]
            E = len(g['edges'])
            ok = np.nonzero(out[2][:E])[0].tolist() == g['bad'] and not out[6].any()
            lines.append("  device G=%d: %8.3f ms per call (%7.3f ms per graph), wait %7.3f / %7.3f ms, iterations %s, "
                         "pruned set %s" % (G, ms, ms / G, wait_med, wait_min, out[4][0].tolist(),
                                            "= corrupted set" if ok else "DIFFERS"))
            ref = out if ref is None else ref
        t = time.perf_counter()
        for _ in range(5):
            h = ops.pose_graph_optimize_host(g['poses0'], g['edges'], g['Z'], g['info'], g['unc'], pc.MAX_DISTANCE)
        host_ms = 1e3 * (time.perf_counter() - t) / 5
        t = time.perf_counter()
        n = reg.pose_graph_numpy(g['poses0'], g['edges'], g['Z'], g['info'], g['unc'], pc.MAX_DISTANCE)
        numpy_ms = 1e3 * (time.perf_counter() - t)
        lines.append("  host twin : %8.3f ms (one CPU thread), poses within %.2e of the device's" % (
            host_ms, np.abs(h[0].numpy() - ref[0][:g['N']]).max()))
        lines.append("  NumPy     : %8.3f ms, poses within %.2e of the device's" % (
            numpy_ms, np.abs(n[0] - ref[0][:g['N']]).max()))
        share, waves = phase_shares(g)
        lines.append("  shares of the kernel's time (wave clock, mean of %d waves):" % waves)
        for label, s in zip(PHASES, share):
            lines.append("    %5.1f %%  %s" % (100 * s, label))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(HERE, 'posegraph_bench.txt'), 'w') as f:
        f.write(text + "\n")


if __name__ == '__main__':
    main()
