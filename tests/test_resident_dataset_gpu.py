"""GPU: ``ops.augment_pairs`` (csrc/augment.hip) against its NumPy restatement bit for bit, the selection's stress
cases, and ``ThreeDMatchResident`` under ``calibrate_neighbors``, ``TrainStep`` and ``Trainer``."""
import random

import numpy as np
import pytest
import torch

from d3feat_pytorch_amd import config as cfgmod
from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.datasets import ThreeDMatch as tdm
from d3feat_pytorch_amd.datasets import dataloader as dl
import resident_cases as rc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_DEVICE_STORES = {}


def _device_stores(M):
    if M not in _DEVICE_STORES:
        points, corr = rc.stores(M)
        _DEVICE_STORES[M] = (torch.from_numpy(points.copy()).to(DEV), torch.from_numpy(corr.copy()).to(DEV))
    return _DEVICE_STORES[M]


def _host(item):
    return tuple(t.cpu().numpy() for t in item)


def _assert_item_is_the_restatement(got, ref, what):
    """Points, sel_corr exact; d2 recomputed from the RETURNED points exact; dist_keypts exact (f64 sqrt is correctly
    rounded on the device and nothing is contracted: 0 ulp observed over the whole case table)."""
    assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)), what
    assert np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32)), what
    assert got[2].dtype == np.int64 and np.array_equal(got[2], ref[2]), what
    d2 = tdm.keypoint_distances(got[0][got[2][:, 0]], squared=True)
    assert np.array_equal(d2.view(np.uint64), tdm.keypoint_distances(ref[0][ref[2][:, 0]], squared=True).view(np.uint64))
    ulp = np.abs(got[3].view(np.int64) - ref[3].view(np.int64)).max()
    print("%s: dist_keypts max ulp distance %d" % (what, ulp))
    assert got[3].shape == ref[3].shape and ulp == 0, (what, ulp)
    assert np.array_equal(got[3] > 0.1, ref[3] > 0.1)                      # the loss's > safe_radius mask


@pytest.mark.parametrize("k", rc.NODES)
def test_kernel_equals_the_restatement_bit_for_bit(k):
    """The CPU suite's case table: M in {1, k-1, k, k+1, 5000, 70000} (the last far beyond LDS as 64-bit keys), tables
    with duplicate rows, three keys, noise 0 and 0.005; clouds of 1000 and 777 points."""
    for M, key, noise in rc.all_cases(k):
        points, corr = _device_stores(M)
        got = _host(ops.augment_pairs(points, corr, [rc.job(M, key)], k, noise)[0])
        _assert_item_is_the_restatement(got, rc.restated(M, k, key, noise), (M, k, key, noise))


def _three_pairs():
    """Packed stores of three pairs of different sizes (each pair's indices local to its own two clouds)."""
    rng = np.random.RandomState(77)
    sizes = ((1000, 777, 5000), (333, 1200, 50), (64, 65, 70000))
    clouds, tables, jobs, at_p, at_c = [], [], [], 0, 0
    for p, (n0, n1, M) in enumerate(sizes):
        clouds += [rng.randn(n0, 3).astype(np.float32), rng.randn(n1, 3).astype(np.float32)]
        tables.append(np.stack([rng.randint(0, n0, M), rng.randint(0, n1, M)], axis=1).astype(np.int32))
        R, t = rc.transform(100 + p)
        jobs.append(ops.AugmentJob(at_p, n0, at_p + n0, n1, at_c, M, R, t, int(tdm.splitmix64(p)[0])))
        at_p, at_c = at_p + n0 + n1, at_c + M
    return np.concatenate(clouds), np.concatenate(tables), jobs


def test_a_batch_of_jobs_gives_the_bits_of_single_calls():
    points, corr, jobs = _three_pairs()
    dp, dc = torch.from_numpy(points).to(DEV), torch.from_numpy(corr).to(DEV)
    k, noise = 64, 0.005
    together = [_host(it) for it in ops.augment_pairs(dp, dc, jobs, k, noise)]
    single = [_host(ops.augment_pairs(dp, dc, [j], k, noise)[0]) for j in jobs]
    swapped = [_host(it) for it in ops.augment_pairs(dp, dc, jobs[::-1], k, noise)][::-1]
    ref = tdm.augment_items_numpy(points, corr, jobs, k, noise)
    assert [it[2].shape[0] for it in together] == [64, 50, 64]
    for a, b, c, r, j in zip(together, single, swapped, ref, jobs):
        assert all(rc.same_bits(x, y) for x, y in zip(a, b))
        assert all(rc.same_bits(x, y) for x, y in zip(a, c))
        _assert_item_is_the_restatement(a, r, j.corr_len)


def test_binding_rejects_what_the_kernel_cannot_take():
    points, corr = _device_stores(5000)
    j = rc.job(5000, 1)
    with pytest.raises(ValueError):
        ops.augment_pairs(points, corr, [], 16, 0.0)
    with pytest.raises(ValueError):
        ops.augment_pairs(points, corr, [j] * 17, 16, 0.0)
    with pytest.raises(ValueError):
        ops.augment_pairs(points, corr, [j], 1025, 0.0)
    with pytest.raises(ValueError):
        ops.augment_pairs(points, corr, [j._replace(corr_len=0)], 16, 0.0)
    with pytest.raises(RuntimeError):
        ops.augment_pairs(points.cpu(), corr, [j], 16, 0.0)
    with pytest.raises(RuntimeError):      # a segment outside the stores is refused on the host, before any launch
        ops.augment_pairs(points, corr, [j._replace(tgt_len=rc.N1 + 1)], 16, 0.0)
    with pytest.raises(RuntimeError):
        ops.augment_pairs(points, corr, [j._replace(corr_off=1)], 16, 0.0)


def _first_histogram(key, M, k):
    """(threshold bin, keys in it) of the kernel's first pass: 256 bins over the top 8 bits of z(7, j)."""
    z = tdm.augment_keys(key, 7, M)
    hist = np.bincount((z >> np.uint64(56)).astype(np.int64), minlength=256)
    b = int(np.argmax(np.cumsum(hist) >= k))
    return b, int(hist[b])


@pytest.mark.parametrize("k", (128, 1000))
def test_selection_with_a_crowded_threshold_bin(k):
    """M = 300000 rows: the first histogram's threshold bin (bin 0 of 256, ~1172 keys expected, 1181 for this key) holds
    more keys than the 1024 candidates the kernel sorts, so it must refine the bin on the next 8 bits; k = 1000 leaves
    the sort nearly full after that."""
    M, key = 300000, rc.KEYS[0]
    b, count = _first_histogram(key, M, k)
    assert count > 1024, (b, count)
    rng = np.random.RandomState(9)
    corr = np.stack([rng.randint(0, rc.N0, M), rng.randint(0, rc.N1, M)], axis=1).astype(np.int32)
    points = rc.stores(5000)[0]
    j = rc.job(M, key)
    ref = tdm.augment_items_numpy(points, corr, [j], k, 0.005)[0]
    got = _host(ops.augment_pairs(torch.from_numpy(points.copy()).to(DEV), torch.from_numpy(corr).to(DEV), [j], k,
                                  0.005)[0])
    rows = np.argsort(tdm.augment_keys(key, 7, M), kind='stable')[:k]
    assert np.array_equal(got[2], corr[rows].astype(np.int64))
    _assert_item_is_the_restatement(got, ref, (M, k))


def test_selection_far_beyond_lds():
    """M = 70000 with k = 128 (560 KB of 64-bit keys against 160 KB of LDS): exact, for every key of the table."""
    M, k = 70000, 128
    points, corr = _device_stores(M)
    for key in rc.KEYS + (7, 2 ** 63):
        got = _host(ops.augment_pairs(points, corr, [rc.job(M, key)], k, 0.0)[0])
        rows = np.argsort(tdm.augment_keys(key, 7, M), kind='stable')[:k]
        assert np.array_equal(got[2], rc.stores(M)[1][rows].astype(np.int64))
        assert np.unique(rows).size == k


# ------------------------------------------------------------------------------------------ ThreeDMatchResident
def _golden_split(golden_s0, folder):
    g = golden_s0
    rc.write_pickles(folder, {'room/a': g['pts0'].astype(np.float64), 'room/b': g['pts1'].astype(np.float64)},
                     {'room/a@room/b': g['sel_corr'].astype(np.int64)})
    return int(g['sel_corr'].shape[0])


def _synthetic_split(folder):
    rng = np.random.RandomState(5)
    clouds = {k: rng.rand(n, 3).astype(np.float32) for k, n in (('s/a', 300), ('s/b', 250), ('s/c', 120), ('s/d', 90))}
    tables = {}
    for s, t, M in (('s/a', 's/b', 400), ('s/a', 's/c', 10), ('s/c', 's/d', 40)):
        tables['%s@%s' % (s, t)] = np.stack([rng.randint(0, clouds[s].shape[0], M),
                                             rng.randint(0, clouds[t].shape[0], M)], axis=1).astype(np.int64)
    rc.write_pickles(folder, clouds, tables)


def test_get_items_equals_single_items_and_the_cpu_class(tmp_path):
    from d3feat_pytorch_amd.train import TrainStep
    _synthetic_split(tmp_path)
    res = tdm.ThreeDMatchResident(str(tmp_path), num_node=16, device=DEV)
    cpu = tdm.ThreeDMatchResident(str(tmp_path), num_node=16, device='cpu')
    assert res.resident_bytes == cpu.resident_bytes and len(res) == len(cpu) == 2
    out = []
    for ds, batched in ((res, True), (res, False), (cpu, False)):
        random.seed(3)
        np.random.seed(3)
        out.append(ds.get_items([0, 1, 0]) if batched else [ds[0], ds[1], ds[0]])
    for a, b, c in zip(*out):
        assert all(t.device == torch.device(DEV) and t.dtype == d for t, d in zip(a, TrainStep.ITEM_DTYPES))
        assert a[2].data_ptr() == a[3].data_ptr() == res._ones.data_ptr()       # views of the one resident buffer
        assert all(rc.same_bits(x, y) for x, y in zip(_host(a), _host(b)))
        assert all(rc.same_bits(x, y) for x, y in zip(_host(a), c))


def test_calibrate_neighbors_over_the_resident_set(golden_s0, tmp_path):
    k = _golden_split(golden_s0, tmp_path)
    res = tdm.ThreeDMatchResident(str(tmp_path), num_node=k, device=DEV)

    class _HostCopy:
        def __len__(self):
            return len(res)

        def __getitem__(self, i):
            return _host(res[i])
    cfg = cfgmod.default_config(first_features_dim=16, num_node=k)
    limits = []
    for ds in (res, _HostCopy()):
        random.seed(1)
        np.random.seed(1)
        limits.append(dl.calibrate_neighbors(ds, cfg, samples_threshold=0, device=DEV))
    assert np.array_equal(limits[0], limits[1]) and np.all(limits[0] > 0)


def test_trainer_consumes_the_resident_set(golden_s0, tmp_path):
    """One epoch of 5 draws and one evaluation under graph replay, as test_trainer_consumes_threedmatch_pickles does on
    the host class."""
    from d3feat_pytorch_amd.train import TrainStep
    from d3feat_pytorch_amd.trainer import Trainer
    g = golden_s0
    k = _golden_split(g, tmp_path)
    ds = tdm.ThreeDMatchResident(str(tmp_path), split='train', num_node=k, downsample=0.03, device=DEV)

    class _Many:   # one source fragment, visited several times per epoch with fresh augmentation draws
        def __len__(self):
            return 5

        def __getitem__(self, i):
            return ds[0]

    class _Loader:
        dataset, batch_size, shuffle = _Many(), 1, True
        limits = [int(x) for x in g['limits']]
    sizes = [int(g['batch.points.%d' % l].shape[0]) for l in range(5)]
    cfg = cfgmod.default_config(first_features_dim=16, num_node=k)
    cfg.max_epoch, cfg.save_dir, cfg.tboard_dir, cfg.device, cfg.graph = 1, None, None, DEV, True
    cfg.train_loader, cfg.val_max_iter = _Loader(), 1
    cfg.graph_capacities = TrainStep.capacities_for([sizes], slack=1.3)
    random.seed(0)
    np.random.seed(0)
    tr = Trainer(cfg)
    before = tr.engine.flat.data.clone()
    avg = tr.train_epoch(1)
    res = tr.evaluate(1)
    assert tr._captured and int(tr.optimizer.skipped) == 0
    assert all(np.isfinite(v) for v in avg.values()) and all(np.isfinite(v) for v in res.values())
    assert not torch.equal(before, tr.engine.flat.data)


def test_resident_item_trains_like_its_host_copy(golden_s0, tmp_path):
    """One eager forward: a resident item (passed through by upload) and the same item copied to host arrays and
    uploaded give exactly the same descriptor and detector loss at the same parameters."""
    from d3feat_pytorch_amd.train import TrainStep
    g = golden_s0
    k = _golden_split(g, tmp_path)
    ds = tdm.ThreeDMatchResident(str(tmp_path), num_node=k, device=DEV)
    cfg = cfgmod.default_config(first_features_dim=16, num_node=k)
    ts = TrainStep(cfg, [int(x) for x in g['limits']], torch.device(DEV), seed=3)
    random.seed(2)
    np.random.seed(2)
    item = ds[0]
    passed = ts.upload(item)
    assert all(a is b for a, b in zip(passed, item))
    copied = ts.upload(_host(item))
    assert all(a is not b and torch.equal(a, b) and a.dtype == b.dtype for a, b in zip(copied, item))
    losses = []
    for it in (passed, copied):
        batch = ts.build_batch(it)
        batch['n0'] = int(it[0].shape[0])
        _, desc, det, _ = ts.forward_loss(batch)
        losses.append((float(desc), float(det)))
    assert np.isfinite(losses[0]).all() and losses[0] == losses[1], losses
