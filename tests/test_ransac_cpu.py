"""CPU: the RANSAC sampler and rigid solver (csrc/rigid.hpp through their host-only C-ABI twins), the gt.info reader,
the benchmark's transformation error and registration recall -- nothing here needs a GPU."""
import ctypes
import os

import numpy as np
import pytest

import d3feat_pytorch_amd  # noqa: F401
from d3feat_pytorch_amd import _native
from d3feat_pytorch_amd.geometric_registration import evaluate as ev
from d3feat_pytorch_amd.geometric_registration import registration as reg

REF = "/root/reference"
M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _lib():
    if not os.path.exists(_native.LIB_PATH):
        _native.build()
    return _native.lib()


def splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over='ignore'):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def sample_numpy(seed, p, h, count):
    """[..., 3] indices of hypothesis h of pair p: the formula written in csrc/rigid.hpp."""
    key = splitmix64(splitmix64(np.uint64(seed)) ^ np.asarray(p, dtype=np.uint64))
    h = np.asarray(h, dtype=np.uint64)
    out = []
    for k in range(3):
        z = splitmix64(key ^ ((h << np.uint64(2)) | np.uint64(k)))
        with np.errstate(over='ignore'):
            out.append(((z >> np.uint64(32)) * np.asarray(count, dtype=np.uint64)) >> np.uint64(32))
    return np.stack(out, axis=-1).astype(np.int64)


def sample_host(seed, p, h, count):
    out = (ctypes.c_int32 * 3)()
    assert _lib().d3f_ransac_sample_host(int(seed), int(p), int(h), int(count), ctypes.addressof(out)) == 0
    return list(out)


def fit_host(src, tgt):
    src = np.ascontiguousarray(src, dtype=np.float64)
    tgt = np.ascontiguousarray(tgt, dtype=np.float64)
    out = np.zeros(16, dtype=np.float64)
    assert _lib().d3f_rigid_fit_host(src.ctypes.data, tgt.ctypes.data, int(src.shape[0]), out.ctypes.data) == 0
    return out.reshape(4, 4)


def kabsch_svd(src, tgt):
    """f64 least-squares rigid fit src ~ R tgt + t with the reflection fix."""
    cs, ct = src.mean(axis=0), tgt.mean(axis=0)
    Hm = (tgt - ct).T @ (src - cs)
    U, _, Vt = np.linalg.svd(Hm)
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return R, cs - R @ ct


def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def test_sampler_matches_the_documented_hash():
    rng = np.random.default_rng(0)
    n = 100000
    seeds = rng.integers(0, 2 ** 63, size=n, dtype=np.uint64)
    seeds[:1000] = 0
    seeds[1000:2000] = np.uint64(2 ** 64 - 1)
    ps = rng.integers(0, 600, size=n)
    hs = rng.integers(0, 50000, size=n)
    hs[2000:3000] = rng.integers(2 ** 23, 2 ** 24, size=1000)          # large h
    counts = rng.integers(1, 6145, size=n)
    counts[3000:4000] = 3
    counts[4000:5000] = 1531                                            # not a power of 2
    counts[5000:6000] = 4096
    want = sample_numpy(seeds, ps, hs, counts)
    assert (want >= 0).all() and (want < counts[:, None]).all()
    lib = _lib()
    out = (ctypes.c_int32 * 3)()
    addr = ctypes.addressof(out)
    fn = lib.d3f_ransac_sample_host
    got = np.empty((n, 3), dtype=np.int64)
    for i in range(n):
        fn(int(seeds[i]), int(ps[i]), int(hs[i]), int(counts[i]), addr)
        got[i] = out[:]
    assert np.array_equal(got, want)
    # count = 3 draws cover all three indices; the hash is not degenerate
    c3 = want[3000:4000]
    assert set(np.unique(c3)) == {0, 1, 2}
    assert lib.d3f_ransac_sample_host(0, 0, 0, 0, addr) == -1


def test_rigid_fit_matches_svd_kabsch():
    rng = np.random.default_rng(1)
    for n in (3, 500):
        for noise in (0.0, 0.01):
            for trial in range(20):
                R0 = _rotation(rng)
                t0 = rng.normal(size=3)
                tgt = rng.uniform(-1.5, 1.5, size=(n, 3))
                src = tgt @ R0.T + t0 + rng.normal(scale=noise, size=(n, 3))
                T = fit_host(src, tgt)
                R, t = kabsch_svd(src, tgt)
                assert np.abs(T[:3, :3] - R).max() < 1e-9 and np.abs(T[:3, 3] - t).max() < 1e-9, (n, noise, trial)
                assert abs(np.linalg.det(T[:3, :3]) - 1.0) < 1e-12
                assert np.array_equal(T[3], [0, 0, 0, 1])
                if noise == 0.0:
                    assert np.abs(T[:3, :3] - R0).max() < 1e-12 and np.abs(T[:3, 3] - t0).max() < 1e-12


def test_rigid_fit_never_reflects():
    """A mirrored point set: the unconstrained least-squares map is a reflection; the fit stays a proper rotation and
    equals the SVD solution with the reflection fix."""
    rng = np.random.default_rng(2)
    tgt = rng.uniform(-1, 1, size=(40, 3))
    src = tgt * np.array([1.0, 1.0, -1.0]) + np.array([0.3, -0.2, 0.1])
    Hm = (tgt - tgt.mean(0)).T @ (src - src.mean(0))
    U, _, Vt = np.linalg.svd(Hm)
    assert np.linalg.det(Vt.T @ U.T) < 0                  # the configuration does induce a reflection
    T = fit_host(src, tgt)
    R, t = kabsch_svd(src, tgt)
    assert abs(np.linalg.det(T[:3, :3]) - 1.0) < 1e-12
    assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 1e-12
    assert np.abs(T[:3, :3] - R).max() < 1e-9 and np.abs(T[:3, 3] - t).max() < 1e-9


INFO_SAMPLE = (
    "0\t 1\t 60\t\n"
    " 5.00000000e+03\t  0.00000000e+00\t  0.00000000e+00\t  0.00000000e+00\t  1.08436729e+04\t  1.26195044e+03\t\n"
    " 0.00000000e+00\t  5.00000000e+03\t  0.00000000e+00\t -1.08436729e+04\t  0.00000000e+00\t -1.24858826e+03\t\n"
    " 0.00000000e+00\t  0.00000000e+00\t  5.00000000e+03\t -1.26195044e+03\t  1.24858826e+03\t  0.00000000e+00\t\n"
    " 0.00000000e+00\t -1.08436729e+04\t -1.26195044e+03\t  2.66481113e+04\t -3.41289291e+01\t  2.59759790e+03\t\n"
    " 1.08436729e+04\t  0.00000000e+00\t  1.24858826e+03\t -3.41289291e+01\t  2.71010840e+04\t  3.71150854e+03\t\n"
    " 1.26195044e+03\t -1.24858826e+03\t  0.00000000e+00\t  2.59759790e+03\t  3.71150854e+03\t  3.56940430e+03\t\n"
    "2\t 7\t 60\t\n"
    " 1.00000000e+00\t  0.00000000e+00\t  0.00000000e+00\t  0.00000000e+00\t  0.00000000e+00\t  0.00000000e+00\t\n"
    " 0.00000000e+00\t  2.00000000e+00\t  0.00000000e+00\t  0.00000000e+00\t  0.00000000e+00\t  0.00000000e+00\t\n"
    " 0.00000000e+00\t  0.00000000e+00\t  3.00000000e+00\t  0.00000000e+00\t  0.00000000e+00\t  0.00000000e+00\t\n"
    " 0.00000000e+00\t  0.00000000e+00\t  0.00000000e+00\t  4.00000000e+00\t  0.00000000e+00\t  0.00000000e+00\t\n"
    " 0.00000000e+00\t  0.00000000e+00\t  0.00000000e+00\t  0.00000000e+00\t  5.00000000e+00\t  0.00000000e+00\t\n"
    " 0.00000000e+00\t  0.00000000e+00\t  0.00000000e+00\t  0.00000000e+00\t  0.00000000e+00\t -6.50000000e-01\t\n")


def test_loadinfo_reads_the_benchmark_layout(tmp_path):
    (tmp_path / 'gt.info').write_text(INFO_SAMPLE)
    got = reg.loadinfo(str(tmp_path))
    assert sorted(got) == ['0_1', '2_7']
    a = got['0_1']
    assert a.shape == (6, 6) and a.dtype == np.float64
    assert a[0, 0] == 5000.0 and a[0, 4] == 1.08436729e+04 and a[3, 4] == -3.41289291e+01 and a[5, 5] == 3.56940430e+03
    assert np.array_equal(a, a.T)
    assert np.array_equal(np.diag(got['2_7']), [1, 2, 3, 4, 5, -0.65])


def _info(rng, n=200):
    """Sum of [I, -[p]x]^T [I, -[p]x] over points p: the structure of the shipped gt.info matrices."""
    info = np.zeros((6, 6))
    for p in rng.uniform(-1, 1, size=(n, 3)):
        px = np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]])
        J = np.hstack([np.eye(3), -px])
        info += J.T @ J
    return info


def test_transformation_error_formula():
    rng = np.random.default_rng(3)
    info = _info(rng)
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = _rotation(rng), rng.normal(size=3)
    assert abs(reg.transformation_error(T, T, info)) < 1e-20
    d = np.array([0.03, -0.05, 0.02])
    Tt = T.copy()
    Tt[:3, 3] += T[:3, :3] @ d                             # inv(T) Tt = pure translation by d
    want = d @ info[:3, :3] @ d / info[0, 0]
    assert abs(reg.transformation_error(Tt, T, info) - want) < 1e-12 * max(1.0, want)
    # sign convention, by hand: Delta = rotation by +a about z plus translation d.  The benchmark's q is the
    # direction-cosine (dcm2quat) quaternion of Delta_R: (cos a/2, 0, 0, -sin a/2), so er = [d, 0, 0, +sin a/2];
    # p = er^T info er / info[0,0] -- the cross terms info[:3, 5] change sign with q_z
    a = 0.1
    D = np.eye(4)
    D[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    D[:3, 3] = d
    er = np.concatenate([d, [0, 0, np.sin(a / 2)]])
    want = er @ info @ er / info[0, 0]
    er_wrong = np.concatenate([d, [0, 0, -np.sin(a / 2)]])
    wrong = er_wrong @ info @ er_wrong / info[0, 0]
    got = reg.transformation_error(T @ D, T, info)
    assert abs(got - want) < 1e-12 and abs(got - wrong) > 1e-6
    # identity ground truth, small rotation about x, plain numbers: info = diag(1..6) -> p = 4 sin^2(a/2) / 1
    D = np.eye(4)
    D[:3, :3] = [[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]]
    got = reg.transformation_error(D, np.eye(4), np.diag([1.0, 2, 3, 4, 5, 6]))
    assert abs(got - 4 * np.sin(a / 2) ** 2) < 1e-15


def test_evaluate_registration_counts_only_far_pairs():
    gt = {'0_1': np.eye(4), '0_2': np.eye(4), '1_3': np.eye(4), '2_5': np.eye(4)}
    info = {k: np.eye(6) for k in gt}
    off = np.eye(4)
    off[0, 3] = 0.5                                        # error 0.25 > 0.04
    est = {'0_1': off, '0_2': np.eye(4), '1_3': off, '3_7': np.eye(4), '2_5': np.eye(4)}
    recall, precision, errs = reg.evaluate_registration(est, gt, info)
    assert recall == 2 / 3 and precision == 2 / 4          # 0_1 is consecutive; 3_7 is not listed
    assert sorted(errs) == ['0_2', '1_3', '2_5'] and abs(errs['1_3'] - 0.25) < 1e-15


SCENES = {  # scene directory: (good, gt pairs with j - i > 1, estimated pairs with j - i > 1)
    '7-scenes-redkitchen': (383, 449, 531),
    'sun3d-home_at-home_at_scan1_2013_jan_1': (83, 106, 236),
    'sun3d-home_md-home_md_scan9_2012_sep_30': (97, 159, 339),
    'sun3d-hotel_uc-scan3': (143, 182, 199),
    'sun3d-hotel_umd-maryland_hotel1': (46, 78, 111),
    'sun3d-hotel_umd-maryland_hotel3': (15, 26, 61),
    'sun3d-mit_76_studyroom-76-1studyroom2': (148, 234, 550),
    'sun3d-mit_lab_hj-lab_hj_tea_nov_2_2012_scan1_erika': (23, 45, 115),
}


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "geometric_registration", "gt_result")),
                    reason="reference benchmark files not mounted")
def test_registration_recall_of_the_3dmatch_logs():
    """The benchmark's own 3dmatch.log trajectories against its gt.log / gt.info: exact good-pair counts."""
    root = os.path.join(REF, "geometric_registration", "gt_result")
    for scene, (good, n_gt, n_est) in SCENES.items():
        d = os.path.join(root, scene + "-evaluation")
        gt, info = ev.loadlog(d), reg.loadinfo(d)
        est = _load_named(d)
        recall, precision, errs = reg.evaluate_registration(est, gt, info)
        assert round(recall * n_gt) == good and round(precision * n_est) == good, (scene, recall, precision)
        assert abs(recall - good / n_gt) < 1e-12 and abs(precision - good / n_est) < 1e-12, scene
        assert min(abs(e - 0.04) for e in errs.values()) > 1e-6, scene


def _load_named(d):
    """evaluate.loadlog reads <dir>/gt.log; the trajectory to score sits beside it as 3dmatch.log."""
    import shutil
    import tempfile
    tmp = tempfile.mkdtemp()
    try:
        shutil.copy(os.path.join(d, '3dmatch.log'), os.path.join(tmp, 'gt.log'))
        return ev.loadlog(tmp)
    finally:
        shutil.rmtree(tmp)
