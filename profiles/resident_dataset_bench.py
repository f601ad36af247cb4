"""Host dataset + upload against the device-resident dataset, side by side in one run (NOT bench.py: that one feeds the
step pre-made device items and so measures neither).

Builds synthetic pickles of 3DMatch-like size with synthetic.py (fragments of ~19k points after 0.03 m subsampling, a
few thousand correspondences per pair, num_node = 128) and measures
  (a) items/s of ``ThreeDMatchDataset.__getitem__`` + ``TrainStep.upload`` against ``ThreeDMatchResident.__getitem__``
      (and ``get_items`` of 12), alternating, wall clock around work that ends in a device synchronise;
  (b) pairs/s of ``Trainer.train_epoch`` with either dataset, on the reference schedule (one pair per step) and with
      ``fast_schedule`` (4 x 3 pairs per step); the first epoch (capture, warm-up) is not timed.
The host-dataset leg is the yardstick: it is what the Trainer did before the resident class existed.

Every leg that uses the GPU is a child process under its own time limit; after a leg that fails or runs out of time
nothing more is started.  Usage:  python profiles/resident_dataset_bench.py [--out profiles/resident_dataset_bench.txt]
"""
import argparse
import json
import os
import random
import shutil
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

DEV = "cuda:0"
NUM_NODE = 128
LEG_LIMITS = {"build": 240, "items": 240, "trainer": 360}     # seconds


def _datasets(root, which):
    from d3feat_pytorch_amd.datasets import ThreeDMatch as tdm
    if which == "host":
        return tdm.ThreeDMatchDataset(root, "train", num_node=NUM_NODE)
    return tdm.ThreeDMatchResident(root, "train", num_node=NUM_NODE, device=DEV)


def leg_build(root, args):
    """Pickles of args.pairs fragment pairs + the neighbour limits both Trainer legs share."""
    import pickle
    import numpy as np
    import torch
    from scipy.spatial import cKDTree
    from d3feat_pytorch_amd import config as cfgmod, synthetic
    from d3feat_pytorch_amd.datasets import ThreeDMatch as tdm, dataloader as dl

    def subsample(points, lengths, dlen):
        p, b = dl.batch_grid_subsampling_kpconv(torch.as_tensor(points).to(DEV), torch.as_tensor(lengths).to(DEV),
                                                sampleDl=dlen)
        return p.cpu().numpy(), b.cpu().numpy()
    clouds, tables = {}, {}
    for i in range(args.pairs):
        a = synthetic.make_fragment(2 * i + 1, subsample)
        b = synthetic.make_fragment(2 * i + 2, subsample)
        dist, nn = cKDTree(b).query(a, k=1, distance_upper_bound=0.0375)
        ok = np.nonzero(np.isfinite(dist))[0][::args.corr_stride]
        clouds["scene%02d/a" % i], clouds["scene%02d/b" % i] = a, b
        tables["scene%02d/a@scene%02d/b" % (i, i)] = np.stack([ok, nn[ok]], axis=1).astype(np.int64)
    with open(os.path.join(root, "3DMatch_train_0.030_points.pkl"), "wb") as f:
        pickle.dump(clouds, f)
    with open(os.path.join(root, "3DMatch_train_0.030_keypts.pkl"), "wb") as f:
        pickle.dump(tables, f)
    cfg = cfgmod.default_config(num_node=NUM_NODE)
    random.seed(0)
    np.random.seed(0)
    host = tdm.ThreeDMatchDataset(root, "train", num_node=NUM_NODE)
    limits = [int(x) for x in dl.calibrate_neighbors(host, cfg, samples_threshold=10 ** 9, device=DEV)]
    return {"pairs": args.pairs, "points_per_fragment": int(np.mean([c.shape[0] for c in clouds.values()])),
            "correspondences_per_pair": int(np.mean([t.shape[0] for t in tables.values()])), "limits": limits}


def leg_items(root, args, limits):
    import numpy as np
    import torch
    from d3feat_pytorch_amd import config as cfgmod
    from d3feat_pytorch_amd.train import TrainStep
    cfg = cfgmod.default_config(num_node=NUM_NODE)
    ts = TrainStep(cfg, limits, torch.device(DEV), seed=0)
    host, res = _datasets(root, "host"), _datasets(root, "resident")
    n = len(host)

    def run_host(count):
        for i in range(count):
            ts.upload(host[i % n])

    def run_resident(count):
        for i in range(count):
            ts.upload(res[i % n])

    def run_resident_12(count):
        for i in range(0, count, 12):
            for item in res.get_items([(i + k) % n for k in range(12)]):
                ts.upload(item)
    out = {"resident_bytes": res.resident_bytes}
    random.seed(0)
    np.random.seed(0)
    for name, fn in (("host", run_host), ("resident", run_resident), ("resident_get_items_12", run_resident_12)):
        fn(24)      # warm-up
    for rnd in range(args.rounds):
        for name, fn in (("host", run_host), ("resident", run_resident), ("resident_get_items_12", run_resident_12)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(args.items)
            torch.cuda.synchronize()
            out.setdefault(name, []).append(args.items / (time.perf_counter() - t0))
    return out


def leg_trainer(root, args, limits, which, fast):
    import numpy as np
    import torch
    from d3feat_pytorch_amd import config as cfgmod
    from d3feat_pytorch_amd.trainer import Trainer
    ds = _datasets(root, which)

    class _Epoch:      # args.epoch_pairs draws per epoch over the split's pairs, fresh augmentation every draw
        def __len__(self):
            return args.epoch_pairs

        def __getitem__(self, i):
            return ds[i % len(ds)]

    class _Loader:
        dataset, batch_size, shuffle = _Epoch(), 1, True
    _Loader.limits = limits
    cfg = cfgmod.default_config(num_node=NUM_NODE)
    cfg.max_epoch, cfg.save_dir, cfg.tboard_dir, cfg.device, cfg.graph = 1, None, None, DEV, True
    cfg.train_loader, cfg.val_max_iter, cfg.verbose, cfg.seed = _Loader(), 1, False, 0
    cfg.fast_schedule = bool(fast)
    random.seed(0)
    np.random.seed(0)
    tr = Trainer(cfg)
    tr.train_epoch(1)      # capture + warm-up
    torch.cuda.synchronize()
    rates = []
    for epoch in range(2, 2 + args.rounds):
        t0 = time.perf_counter()
        avg = tr.train_epoch(epoch)
        torch.cuda.synchronize()
        steps = args.epoch_pairs // tr.group
        rates.append(steps * tr.group / (time.perf_counter() - t0))
    return {"dataset": which, "pairs_per_step": tr.group, "pairs_per_s": rates, "skipped_steps": int(tr.optimizer.skipped),
            "rerun_pairs": int(getattr(tr, "rerun_pairs", 0)), "desc_loss": float(avg["desc_loss"])}


def child(args):
    shared = os.path.join(args.root, "build.json")
    limits = json.load(open(shared))["limits"] if os.path.exists(shared) else None
    if args.leg == "build":
        res = leg_build(args.root, args)
        json.dump(res, open(shared, "w"))
    elif args.leg == "items":
        res = leg_items(args.root, args, limits)
    else:
        _, which, schedule = args.leg.split(":")
        res = leg_trainer(args.root, args, limits, which, schedule == "fast")
    print("RESULT " + json.dumps(res))


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "resident_dataset_bench.txt"))
    ap.add_argument("--pairs", type=int, default=16, help="fragment pairs in the synthetic split")
    ap.add_argument("--corr-stride", type=int, default=3, help="keep every n-th mined correspondence")
    ap.add_argument("--items", type=int, default=240, help="items per timed round of (a)")
    ap.add_argument("--epoch-pairs", type=int, default=192, help="draws per epoch of (b)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leg", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--root", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        return child(args)
    root = tempfile.mkdtemp(prefix="resident_bench_")
    legs = ["build", "items", "trainer:host:reference", "trainer:resident:reference", "trainer:host:fast",
            "trainer:resident:fast"]
    results, lines = {}, []
    try:
        for leg in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--root", root] + [
                "--%s=%d" % (k, getattr(args, k.replace("-", "_"))) for k in ("pairs", "corr-stride", "items",
                                                                             "epoch-pairs", "rounds")]
            limit = LEG_LIMITS[leg.split(":")[0]]
            try:
                p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=limit, text=True)
            except subprocess.TimeoutExpired:
                lines.append("%s: no result within %d s; nothing more was started" % (leg, limit))
                break
            got = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
            if p.returncode != 0 or not got:
                lines.append("%s: exit status %d; nothing more was started\n%s" % (leg, p.returncode, p.stdout[-2000:]))
                break
            results[leg] = json.loads(got[-1][7:])
            print(leg, results[leg], flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    text = ["resident_dataset_bench.py: host dataset + upload against the resident dataset, one run",
            "arguments: %s" % {k: v for k, v in vars(args).items() if k not in ("leg", "root", "out")}]
    if "build" in results:
        text.append("split: %(pairs)d pairs, %(points_per_fragment)d points per fragment, %(correspondences_per_pair)d "
                    "correspondences per pair, num_node %(nn)d, neighbour limits %(limits)s"
                    % dict(results["build"], nn=NUM_NODE))
    if "items" in results:
        r = results["items"]
        h, d, g = _median(r["host"]), _median(r["resident"]), _median(r["resident_get_items_12"])
        text += ["(a) items/s, median of %d rounds of %d items (rounds: host %s | resident %s | get_items(12) %s)"
                 % (args.rounds, args.items, ["%.0f" % x for x in r["host"]], ["%.0f" % x for x in r["resident"]],
                    ["%.0f" % x for x in r["resident_get_items_12"]]),
                 "    host __getitem__ + upload      %9.1f items/s  (%.3f ms per item)" % (h, 1e3 / h),
                 "    resident __getitem__           %9.1f items/s  (%.3f ms per item)  x%.2f" % (d, 1e3 / d, d / h),
                 "    resident get_items(12)         %9.1f items/s  (%.3f ms per item)  x%.2f" % (g, 1e3 / g, g / h),
                 "    resident stores: %d bytes" % r["resident_bytes"]]
    for schedule in ("reference", "fast"):
        a, b = results.get("trainer:host:%s" % schedule), results.get("trainer:resident:%s" % schedule)
        if a and b:
            ha, hb = _median(a["pairs_per_s"]), _median(b["pairs_per_s"])
            text += ["(b) Trainer.train_epoch, %s schedule (%d pair(s) per step), median of %d epochs of %d pairs"
                     % (schedule, b["pairs_per_step"], args.rounds, args.epoch_pairs),
                     "    host dataset                   %9.1f pairs/s  (%.3f ms per pair)  epochs %s  skipped %d rerun %d"
                     % (ha, 1e3 / ha, ["%.0f" % x for x in a["pairs_per_s"]], a["skipped_steps"], a["rerun_pairs"]),
                     "    resident dataset               %9.1f pairs/s  (%.3f ms per pair)  epochs %s  skipped %d rerun %d"
                     "  x%.2f" % (hb, 1e3 / hb, ["%.0f" % x for x in b["pairs_per_s"]], b["skipped_steps"],
                                  b["rerun_pairs"], hb / ha)]
    text += lines
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text) + "\n")
    print("\n".join(text))
    return 1 if lines else 0


if __name__ == "__main__":
    sys.exit(main())
