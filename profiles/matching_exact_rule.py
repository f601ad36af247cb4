"""Cost of a change to the matching kernel's arg-min rule: two builds of libd3feat_hip.so (the parent's and the change's,
`_native.build(out=..., objdir=...)` of either checkout) run the 19k x 19k x 32 matching of tests/golden/s1_match.npz in
ONE process, alternating, RUNS runs each of LAUNCHES launches between device events after a warm-up.
python profiles/matching_exact_rule.py parent=PARENT.so change=CHANGE.so [name=OTHER.so ...]"""
import ctypes as C
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch
from d3feat_pytorch_amd import _native

RUNS, LAUNCHES = 7, 30


def load(path):
    lib = C.CDLL(path)
    for name in ("d3f_mutual_nn_ws_bytes", "d3f_mutual_nn"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _native.SIGNATURES[name]
    return lib


def main():
    names, paths = zip(*(a.split("=", 1) for a in sys.argv[1:]))
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    libs = [load(p) for p in paths]
    g = np.load(os.path.join(REPO, "tests", "golden", "s1_match.npz"), allow_pickle=False)
    n0 = int(g["n0"])
    S = torch.from_numpy(g["features_eval"][:n0]).to(dev).contiguous()
    T = torch.from_numpy(g["features_eval"][n0:]).to(dev).contiguous()
    Ns, Nt, ch = S.shape[0], T.shape[0], S.shape[1]
    out = [[torch.empty(n, dtype=torch.int32, device=dev) for n in (Ns, Nt, Ns)] for _ in libs]
    nbytes = libs[0].d3f_mutual_nn_ws_bytes(Ns, Nt)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def launch(k):
        ra, ca, mu = out[k]
        rc = libs[k].d3f_mutual_nn(S.data_ptr(), Ns, T.data_ptr(), Nt, ch, ra.data_ptr(), ca.data_ptr(), mu.data_ptr(),
                                   ws.data_ptr(), nbytes, stream)
        assert rc == 0, rc

    for k in range(len(libs)):
        for _ in range(10):
            launch(k)
    torch.cuda.synchronize()
    series = [[] for _ in libs]
    for _ in range(RUNS):
        for k in range(len(libs)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(LAUNCHES):
                launch(k)
            e1.record()
            torch.cuda.synchronize()
            series[k].append(e0.elapsed_time(e1) / LAUNCHES)
    print("mutual_nn %d x %d x %d, ms per call (fill + sweep + unpack), %d runs of %d launches, alternating:" % (
        Ns, Nt, ch, RUNS, LAUNCHES))
    for name, s in zip(names, series):
        print("%-6s %s   min %.4f median %.4f max %.4f" % (name, " ".join("%.4f" % x for x in s), min(s),
                                                           float(np.median(s)), max(s)))
    for name, o in zip(names[1:], out[1:]):
        diff = tuple(int((a != b).sum()) for a, b in zip(out[0], o))
        print("rows / columns / mutual flags of %s that differ from %s's on these descriptors: %d / %d / %d" % (
            (name, names[0]) + diff))


if __name__ == "__main__":
    main()
