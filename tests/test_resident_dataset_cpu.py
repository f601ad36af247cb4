"""CPU: the augmentation of the device-resident 3DMatch set through its host twin (d3f_augment_item_host, built from
the same csrc/augment.hpp functions as the kernels) against the NumPy restatement, the statistics of the restatement,
and ``ThreeDMatchResident(device='cpu')`` -- nothing here needs a GPU."""
import random

import numpy as np
import pytest

import d3feat_pytorch_amd  # noqa: F401
from d3feat_pytorch_amd import _native, ops
from d3feat_pytorch_amd.datasets import ThreeDMatch as tdm
import resident_cases as rc


def test_splitmix64_known_answer_through_the_host_twin():
    lib = _native.lib()
    assert lib.d3f_augment_key_host(0, 0, 0) == 0xE220A8397B1DCDAF
    assert int(tdm.splitmix64(0)[0]) == 0xE220A8397B1DCDAF
    for key, s, i in ((0x0123456789ABCDEF, 7, 5), (2 ** 64 - 1, 1, 2 ** 32 - 1), (42, 4, 69999)):
        z = int(tdm.splitmix64(np.uint64(key) ^ np.uint64((s << 32) | i))[0])
        assert lib.d3f_augment_key_host(key, s, i) == z
        if i < 10 ** 6:
            assert int(tdm.augment_keys(key, s, i + 1)[i]) == z


@pytest.mark.parametrize("k", rc.NODES)
def test_host_twin_equals_the_restatement_bit_for_bit(k):
    """Points (uint32 view), sel_corr and dist_keypts (uint64 view) over the case table: M in {1, k-1, k, k+1, 5000,
    70000} rows with duplicates, three keys, noise 0 and 0.005."""
    for M, key, noise in rc.all_cases(k):
        points, corr = rc.stores(M)
        ref = rc.restated(M, k, key, noise)
        got = rc.host_twin(points, corr, rc.job(M, key), k, noise)
        m = min(M, k)
        assert ref[2].shape == (m, 2) and ref[3].shape == (m, m)
        assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)), (M, key, noise)
        assert np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32)), (M, key, noise)
        assert np.array_equal(got[2], ref[2]), (M, key, noise)
        assert np.array_equal(got[3].view(np.uint64), ref[3].view(np.uint64)), (M, key, noise)


def test_host_twin_rejects_an_empty_table_and_bad_arguments():
    lib = _native.lib()
    points, corr = rc.stores(5000)
    import ctypes
    q = _native.AugmentJob()
    q.src_len, q.tgt_off, q.tgt_len, q.corr_len = rc.N0, rc.N0, rc.N1, 0
    out = [np.zeros((rc.N0, 3), np.float32), np.zeros((rc.N1, 3), np.float32), np.zeros((16, 2), np.int64),
           np.zeros((16, 16))]
    q.out_src, q.out_tgt, q.out_corr, q.out_dist = (a.ctypes.data for a in out)
    assert lib.d3f_augment_item_host(points.ctypes.data, corr.ctypes.data, ctypes.byref(q), 16, 0.0) == -1   # M < 1
    q.corr_len = 10
    assert lib.d3f_augment_item_host(points.ctypes.data, corr.ctypes.data, ctypes.byref(q), 0, 0.0) == -1
    assert lib.d3f_augment_item_host(points.ctypes.data, corr.ctypes.data, ctypes.byref(q), 16, -1.0) == -1
    assert lib.d3f_augment_item_host(None, corr.ctypes.data, ctypes.byref(q), 16, 0.0) == -1
    assert lib.d3f_augment_item_host(points.ctypes.data, corr.ctypes.data, ctypes.byref(q), 16, 0.0) == 10
    assert lib.d3f_augment_pairs(None, 1, None, 1, None, 1, 16, 0.0, None, 0, None) == -1    # checked before any launch
    assert lib.d3f_augment_pairs_ws_bytes(16, 128) == 0


def test_selection_is_the_k_smallest_keys_without_repeats():
    for k in rc.NODES:
        for M in (k + 1, 5000, 70000):
            for key in rc.KEYS:
                points, corr = rc.stores(M)
                z = tdm.augment_keys(key, 7, M)
                assert np.unique(z).size == M                              # distinct keys: no tie rule needed
                rows = np.argsort(z, kind='stable')[:k]
                assert np.unique(rows).size == k
                assert np.array_equal(rc.restated(M, k, key, 0.005)[2], corr[rows].astype(np.int64))
                got = rc.host_twin(points, corr, rc.job(M, key), k, 0.005)
                assert np.array_equal(got[2], corr[rows].astype(np.int64))


def test_key_decides_the_item():
    M, k = 5000, 64
    a, b = rc.restated(M, k, rc.KEYS[0], 0.005), rc.restated(M, k, rc.KEYS[2], 0.005)
    assert not np.array_equal(a[2], b[2])
    assert not np.array_equal(tdm.augment_uniform(rc.KEYS[0], 1, 100), tdm.augment_uniform(rc.KEYS[2], 1, 100))
    points, corr = rc.stores(M)
    again = tdm.augment_items_numpy(points, corr, [rc.job(M, rc.KEYS[0])], k, 0.005)[0]
    assert all(rc.same_bits(x, y) for x, y in zip(a, again))
    twice = rc.host_twin(points, corr, rc.job(M, rc.KEYS[0]), k, 0.005)
    assert all(rc.same_bits(x, y) for x, y in zip(a, twice))


def test_noise_is_uniform_in_the_unit_interval():
    """n = 4096 points x 3 coordinates x 2 clouds: every u in [0, 1); the mean of 3n uniforms has standard deviation
    1 / sqrt(12 * 3n) = 1 / sqrt(36 n), so six of them bound |mean - 0.5| by 6 / sqrt(36 n) = 0.0156."""
    n = 4096
    for key in rc.KEYS:
        for first in (1, 4):
            u = np.stack([tdm.augment_uniform(key, first + a, n) for a in range(3)])
            assert u.min() >= 0.0 and u.max() < 1.0
            assert abs(u.mean() - 0.5) < 6.0 / np.sqrt(36.0 * n)
    # and the points carry it: noise 1.0 on zero points IS u, rounded to float32
    points = np.zeros((2 * n, 3), np.float32)
    corr = np.zeros((1, 2), np.int32)
    j = ops.AugmentJob(0, n, n, n, 0, 1, np.eye(3), np.zeros(3), 99)
    p0, p1, _, _ = tdm.augment_items_numpy(points, corr, [j], 16, 1.0)[0]
    for a in range(3):
        assert np.array_equal(p0[:, a], tdm.augment_uniform(99, 1 + a, n).astype(np.float32))
        assert np.array_equal(p1[:, a], tdm.augment_uniform(99, 4 + a, n).astype(np.float32))


def test_every_row_is_sampled_equally_often():
    """M = 20 rows, k = 5, keys K_t = splitmix64(1000 + t) for t < 2000: each row is included with probability 1/4, a
    binomial frequency with standard deviation sqrt(0.25 * 0.75 / 2000); six of them = 0.058."""
    M, k, T = 20, 5, 2000
    keys = tdm.splitmix64(np.arange(1000, 1000 + T, dtype=np.uint64))
    counts = np.zeros(M)
    for K in keys:
        rows = np.argsort(tdm.augment_keys(int(K), 7, M), kind='stable')[:k]
        counts[rows] += 1
    f = counts / T
    assert np.all(np.abs(f - 0.25) < 6.0 * np.sqrt(0.25 * 0.75 / T)), f
    # the restatement's selection is that argsort
    corr = np.stack([np.arange(M), np.arange(M)], axis=1).astype(np.int32)
    j = ops.AugmentJob(0, M, M, M, 0, M, np.eye(3), np.zeros(3), int(keys[0]))
    sel = tdm.augment_items_numpy(np.zeros((2 * M, 3), np.float32), corr, [j], k, 0.0)[0][2]
    assert np.array_equal(sel[:, 0], np.argsort(tdm.augment_keys(int(keys[0]), 7, M), kind='stable')[:k])


# ------------------------------------------------------------------------------------------ ThreeDMatchResident
def _split(tmp_path, big=False):
    rng = np.random.RandomState(5)
    sizes = {'s/a': 300, 's/b': 250, 's/c': 120, 's/d': 90}
    clouds = {k: rng.rand(n, 3).astype(np.float32) for k, n in sizes.items()}
    if big:
        clouds['s/huge'] = rng.rand(tdm.ThreeDMatchResident.MAX_POINTS + 1, 3).astype(np.float32)
    pairs = [('s/a', 's/b', 400), ('s/a', 's/c', 10), ('s/c', 's/d', 40)] + ([('s/huge', 's/a', 50)] if big else [])
    tables = {}
    for s, t, M in pairs:
        tables['%s@%s' % (s, t)] = np.stack([rng.randint(0, clouds[s].shape[0], M),
                                             rng.randint(0, clouds[t].shape[0], M)], axis=1).astype(np.int64)
    rc.write_pickles(tmp_path, clouds, tables)
    return clouds, tables


def test_resident_cpu_items_have_the_host_class_structure(tmp_path):
    import torch
    from d3feat_pytorch_amd.train import TrainStep
    clouds, tables = _split(tmp_path)
    host = tdm.ThreeDMatchDataset(str(tmp_path), num_node=16)
    res = tdm.ThreeDMatchResident(str(tmp_path), num_node=16, device='cpu')
    assert len(res) == len(host) == 2 and res.ids_list == host.ids_list and res.src_to_tgt == host.src_to_tgt
    assert (res.num_node, res.__type__, res.MAX_POINTS, res.config) == (16, host.__type__, host.MAX_POINTS, None)
    assert res.resident_bytes == 4 * 3 * 760 + 4 * 2 * 450 + 4 * 300
    for index in range(len(res)):
        random.seed(index)
        np.random.seed(index)
        a = host[index]
        random.seed(index)
        np.random.seed(index)
        b = res[index]
        assert len(a) == len(b) == 6
        for x, y, dtype in zip(a, b, TrainStep.ITEM_DTYPES):      # same pair (first item of a seeded run), same shapes
            assert tuple(x.shape) == tuple(y.shape)
            assert torch.as_tensor(y).dtype == dtype               # already what upload() would convert the host's to
        assert np.all(b[2] == 1) and np.all(b[3] == 1) and b[2].shape == (b[0].shape[0], 1)
        j = res.last_jobs[0]
        table = tables['s/a@s/b' if j.corr_len == 400 else ('s/a@s/c' if j.corr_len == 10 else 's/c@s/d')]
        assert {tuple(r) for r in b[4]} <= {tuple(r) for r in table}
        assert np.array_equal(b[5], tdm.keypoint_distances(b[0][b[4][:, 0]]))
        # the noise is positive and below augment_noise on the source, which is not moved
        d = b[0].astype(np.float64) - res._points[j.src_off:j.src_off + j.src_len].astype(np.float64)
        assert d.min() >= 0.0 and d.max() < 0.005 + 1e-7
    with pytest.raises(ValueError):
        res.get_items([])
    with pytest.raises(ValueError):
        tdm.ThreeDMatchResident(str(tmp_path), num_node=16, device='cpu', max_bytes=1000)
    with pytest.raises(FileNotFoundError):
        tdm.ThreeDMatchResident(str(tmp_path), split='val', device='cpu')


def test_resident_get_items_draws_like_single_items(tmp_path):
    _split(tmp_path)
    res = tdm.ThreeDMatchResident(str(tmp_path), num_node=16, device='cpu')
    random.seed(3)
    np.random.seed(3)
    together = res.get_items([0, 1, 0])
    random.seed(3)
    np.random.seed(3)
    single = [res[0], res[1], res[0]]
    for a, b in zip(together, single):
        assert all(rc.same_bits(x, y) for x, y in zip(a, b))
    assert not rc.same_bits(single[0][0], single[2][0]) or not rc.same_bits(single[0][1], single[2][1])   # fresh keys


def test_resident_never_returns_oversized_pairs(tmp_path):
    _split(tmp_path, big=True)
    res = tdm.ThreeDMatchResident(str(tmp_path), num_node=16, device='cpu')
    huge = res._sources.index('s/huge')
    random.seed(0)
    np.random.seed(0)
    for _ in range(20):
        item = res[huge]
        assert item[0].shape[0] <= res.MAX_POINTS and item[1].shape[0] <= res.MAX_POINTS
        assert res.last_jobs[0].src_len <= res.MAX_POINTS


def test_resident_validates_its_tables_once(tmp_path):
    clouds, tables = _split(tmp_path)
    for column, value in ((0, 300), (1, 250), (0, -1)):
        bad = {k: v.copy() for k, v in tables.items()}
        bad['s/a@s/b'][7, column] = value
        rc.write_pickles(tmp_path, clouds, bad)
        with pytest.raises(ValueError):
            tdm.ThreeDMatchResident(str(tmp_path), num_node=16, device='cpu')
    rc.write_pickles(tmp_path, clouds, tables)
    with pytest.raises(ValueError):
        tdm.ThreeDMatchResident(str(tmp_path), num_node=16, self_augment=True, device='cpu')
    tdm.ThreeDMatchResident(str(tmp_path), num_node=16, device='cpu')


def test_resident_target_is_the_drawn_transform_without_noise(tmp_path):
    clouds, _ = _split(tmp_path)
    res = tdm.ThreeDMatchResident(str(tmp_path), num_node=16, augment_noise=0.0, augment_axis=3, device='cpu')
    random.seed(11)
    np.random.seed(11)
    for index in (0, 1, 0):
        item = res[index]
        j = res.last_jobs[0]
        R, t = j.R, j.t
        assert abs(np.linalg.det(R) - 1.0) < 1e-6 and np.all(t >= 0) and np.all(t < 0.001 + 1e-9)
        assert np.array_equal(R, R.astype(np.float32).astype(np.float64))      # rounded to float32 like the host class
        src = res._points[j.src_off:j.src_off + j.src_len]
        p = res._points[j.tgt_off:j.tgt_off + j.tgt_len].astype(np.float64)
        want = np.stack([((R[a, 0] * p[:, 0] + R[a, 1] * p[:, 1]) + R[a, 2] * p[:, 2]) + t[a] for a in range(3)], axis=1)
        assert np.array_equal(item[1], want.astype(np.float32))
        assert np.array_equal(item[0], src)                                     # the source is not moved
        assert np.allclose(item[1], p @ R.T + t, atol=1e-6)
