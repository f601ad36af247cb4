"""Shared by test_resident_dataset_cpu.py and test_resident_dataset_gpu.py: the case table of the augmentation kernel
and its NumPy restatement (datasets.ThreeDMatch.augment_items_numpy), computed once per case and never modified."""
import ctypes
import functools

import numpy as np

from d3feat_pytorch_amd import _native, ops
from d3feat_pytorch_amd.datasets import ThreeDMatch as tdm

N0, N1 = 1000, 777
NODES = (16, 64, 128)
KEYS = (0x0123456789ABCDEF, 0xFFFFFFFFFFFFFFFF, 42)
NOISES = (0.0, 0.005)


def corr_lengths(k):
    return (1, k - 1, k, k + 1, 5000, 70000)     # 70000 64-bit keys = 560 KB: beyond the 160 KB of LDS


@functools.lru_cache(maxsize=None)
def stores(M):
    """(points f32 [N0+N1,3], corr int32 [M,2] with duplicate rows): the source cloud first, then the target."""
    rng = np.random.RandomState(1000 + M % 997)
    points = (rng.rand(N0 + N1, 3) * 3.0 - 1.0).astype(np.float32)
    corr = np.stack([rng.randint(0, N0, M), rng.randint(0, N1, M)], axis=1).astype(np.int32)
    if M >= 2:
        corr[M // 2] = corr[0]                     # a duplicate row whatever the draw
    points.setflags(write=False)
    corr.setflags(write=False)
    return points, corr


def transform(key):
    rng = np.random.RandomState(key % (2 ** 31))
    q, _ = np.linalg.qr(rng.randn(3, 3))
    return q * np.sign(np.linalg.det(q)), rng.rand(3) * 0.5


def job(M, key):
    R, t = transform(key)
    return ops.AugmentJob(0, N0, N0, N1, 0, M, R, t, key)


@functools.lru_cache(maxsize=None)
def restated(M, k, key, noise):
    points, corr = stores(M)
    out = tdm.augment_items_numpy(points, corr, [job(M, key)], k, noise)[0]
    for a in out:
        a.setflags(write=False)
    return out


def all_cases(k):
    return [(M, key, noise) for M in corr_lengths(k) for key in KEYS for noise in NOISES]


def host_twin(points, corr, j, k, noise):
    """d3f_augment_item_host on NumPy stores -> (pts0, pts1, sel_corr, dist_keypts)."""
    m = min(int(j.corr_len), int(k))
    q = _native.AugmentJob()
    q.src_off, q.src_len, q.tgt_off, q.tgt_len = j.src_off, j.src_len, j.tgt_off, j.tgt_len
    q.corr_off, q.corr_len, q.key = j.corr_off, j.corr_len, j.key
    q.R[:] = [float(v) for v in np.asarray(j.R, dtype=np.float64).reshape(9)]
    q.t[:] = [float(v) for v in np.asarray(j.t, dtype=np.float64).reshape(3)]
    out = (np.zeros((j.src_len, 3), np.float32), np.zeros((j.tgt_len, 3), np.float32), np.zeros((m, 2), np.int64),
           np.zeros((m, m), np.float64))
    q.out_src, q.out_tgt, q.out_corr, q.out_dist = (a.ctypes.data for a in out)
    rc = _native.lib().d3f_augment_item_host(points.ctypes.data, corr.ctypes.data, ctypes.byref(q), int(k), float(noise))
    assert rc == m, rc
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def write_pickles(folder, clouds, tables, split='train', downsample=0.03):
    import os
    import pickle
    with open(os.path.join(str(folder), '3DMatch_%s_%.3f_points.pkl' % (split, downsample)), 'wb') as f:
        pickle.dump(clouds, f)
    with open(os.path.join(str(folder), '3DMatch_%s_%.3f_keypts.pkl' % (split, downsample)), 'wb') as f:
        pickle.dump(tables, f)
