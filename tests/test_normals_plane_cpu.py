"""CPU: the two solvers of the point-to-plane refinement through their host twins (d3f_normal_from_moments_host,
d3f_icp_plane_fit_host; csrc/plane.hpp) against NumPy, and the NumPy restatements of both contracts
(registration.estimate_normals_numpy, registration.icp_numpy(normals=...)) on the surface scene."""
import ctypes

import numpy as np
import pytest

from d3feat_pytorch_amd import _native
from d3feat_pytorch_amd.geometric_registration import registration as reg
import icp_scene as sc

SHIFT = (300.0, -200.0, 50.0)
R_NORMAL = 0.2
ANGLE = 1e-6          # rad: the f32 rounding of three components (~2e-7) with margin; the f64 solvers agree to ~1e-13
GAP = 1e-2            # (l1 - l0) / l2 below which the smallest eigenvector is ill-conditioned and not compared
HEALTHY, LOW_OVERLAP = ('0_1', '0_3', '1_2', '2_3'), ('0_2', '1_3')


def normal_host(m, Q, to_view):
    m = np.ascontiguousarray(m, dtype=np.int64)
    tv = np.ascontiguousarray(to_view, dtype=np.float64)
    out = np.full(3, np.nan, dtype=np.float32)
    assert _native.lib().d3f_normal_from_moments_host(m.ctypes.data, float(Q), tv.ctypes.data, out.ctypes.data) == 0
    return out


def eigh_of_moments(m):
    """(eigenvalues ascending, eigenvectors) of C = (S - s s^T / n) / n from the integer moments, f64."""
    n = float(m[0])
    s = m[1:4].astype(np.float64)
    S = m[[4, 5, 6, 5, 7, 8, 6, 8, 9]].astype(np.float64).reshape(3, 3)
    return np.linalg.eigh((S - np.outer(s, s) / n) / n)


def angle_between(a, b):
    """Angle of the LINES along a and b (sign-free), accurate for small angles."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.arctan2(np.linalg.norm(np.cross(a, b)), abs(a @ b)))


def check_normals(normals, moments, points, rows, view=(0.0, 0.0, 0.0)):
    """The angle bound on every row of ``rows`` whose gap (measured on the oracle's eigenvalues) exceeds GAP; at most
    1 % may fall below it.  Returns (worst angle, excluded share)."""
    worst, excluded = 0.0, 0
    for i in rows:
        w, V = eigh_of_moments(moments[i])
        assert w[2] > 0
        if (w[1] - w[0]) / w[2] <= GAP:
            excluded += 1
            continue
        worst = max(worst, angle_between(normals[i], V[:, 0]))
        assert abs(np.linalg.norm(normals[i].astype(np.float64)) - 1.0) < 1e-6
        to_view = np.asarray(view, dtype=np.float64) - points[i].astype(np.float64)
        assert normals[i].astype(np.float64) @ to_view >= -1e-6 * np.linalg.norm(to_view)
    return worst, excluded / max(len(rows), 1)


@pytest.fixture(scope="module")
def small_scene():
    clouds, _ = sc.make_scene(4, 2, n=6000)
    normals, count, moments = reg.estimate_normals_numpy(clouds, R_NORMAL, return_moments=True)
    return clouds, normals, count, moments


def test_normal_from_moments_host_matches_eigh(small_scene):
    clouds, _, count, moments = small_scene
    pts = np.concatenate(clouds)
    Q = reg.normals_scale(R_NORMAL)
    assert Q == 2.0 ** 22 and np.abs(moments[:, 1:4]).max() <= count.max() * 2 ** 20
    rows = np.arange(0, len(pts), 9)                       # a few hundred neighbourhoods of both fragments
    rows = rows[count[rows] >= 3]                          # (min_neighbors is the caller's test, not the solver's)
    assert len(rows) >= 300
    got = np.stack([normal_host(moments[i], Q, -pts[i].astype(np.float64)) for i in rows])
    full = np.zeros((len(pts), 3), dtype=np.float32)
    full[rows] = got
    worst, share = check_normals(full, moments, pts, rows)
    print("%d rows: worst angle %.3g rad, %.2f %% below the gap" % (len(rows), worst, 100 * share))
    assert worst < ANGLE
    assert share <= 0.01


def test_normal_sign_rule_and_zero_normals_are_exact():
    # 5 points of the plane z = 0 about the centre: u_z = 0 everywhere, the normal is +-(0, 0, 1) exactly
    u = np.array([[0, 0, 0], [100, 0, 0], [-100, 7, 0], [3, 90, 0], [5, -80, 0]], dtype=np.int64)
    m = np.array([len(u), *u.sum(0), (u[:, 0] ** 2).sum(), (u[:, 0] * u[:, 1]).sum(), 0, (u[:, 1] ** 2).sum(), 0, 0])
    assert normal_host(m, 1024.0, (0.3, -2.0, 5.0)).tolist() == [0.0, 0.0, 1.0]
    assert normal_host(m, 1024.0, (0.3, -2.0, -5.0)).tolist() == [0.0, 0.0, -1.0]
    assert normal_host(m, 1024.0, (1.0, 1.0, 0.0)).tolist() == [0.0, 0.0, 1.0]      # dot exactly 0: first non-zero > 0
    assert normal_host(m, 1024.0, (0.0, 0.0, 0.0)).tolist() == [0.0, 0.0, 1.0]
    # the same along x: the first non-zero component is x
    mx = m[[0, 3, 2, 1, 9, 8, 6, 7, 5, 4]]
    assert normal_host(mx, 1024.0, (0.0, 1.0, 0.0)).tolist() == [1.0, 0.0, 0.0]
    assert normal_host(mx, 1024.0, (-1.0, 1.0, 0.0)).tolist() == [-1.0, 0.0, 0.0]
    # no neighbour at all, and neighbours that all coincide with the point: zero normals
    assert normal_host(np.zeros(10, dtype=np.int64), 1024.0, (0, 0, 1)).tolist() == [0.0, 0.0, 0.0]
    same = np.zeros(10, dtype=np.int64)
    same[0] = 100
    assert normal_host(same, 1024.0, (0, 0, 1)).tolist() == [0.0, 0.0, 0.0]
    off = np.array([4, 8, -12, 20, 16, -24, 40, 36, -60, 100], dtype=np.int64)      # 4 copies of u = (2, -3, 5)
    assert normal_host(off, 1024.0, (0, 0, 1)).tolist() == [0.0, 0.0, 0.0]
    L = _native.lib()
    out = np.zeros(3, dtype=np.float32)
    assert L.d3f_normal_from_moments_host(None, 1.0, out.ctypes.data, out.ctypes.data) == -1
    assert L.d3f_normal_from_moments_host(m.ctypes.data, 0.0, np.zeros(3).ctypes.data, out.ctypes.data) == -1


def test_estimate_normals_numpy_is_permutation_invariant(small_scene):
    clouds, normals, count, moments = small_scene
    rng = np.random.default_rng(12)
    perm = rng.permutation(len(clouds[0]))
    n2, c2, m2 = reg.estimate_normals_numpy([clouds[0][perm]], R_NORMAL, return_moments=True)
    k = len(clouds[0])
    assert np.array_equal(m2, moments[:k][perm]) and np.array_equal(c2, count[:k][perm])
    assert np.array_equal(n2, normals[:k][perm])
    # and the count is the brute-force one
    p = clouds[0]
    e = p[:50, None, :] - p[None, :, :]
    d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    assert np.array_equal((d2 < np.float32(R_NORMAL) * np.float32(R_NORMAL)).sum(1), count[:50])
    with pytest.raises(ValueError):
        reg.estimate_normals_numpy(clouds, 0.0)


# ------------------------------------------------------------------------------------------------ the plane fit
def plane_sums(x, y, nrm, T, py):
    """The 29 sums of include/d3feat_hip.h and the stacked J, r they come from."""
    a = x.astype(np.float64) @ T[:3, :3].T + T[:3, 3] - py
    c = y.astype(np.float64) - py
    n = nrm.astype(np.float64)
    J = np.concatenate([np.cross(a, n), n], 1)
    r = ((a - c) * n).sum(1)
    A = J.T @ J
    d2 = ((a - c) ** 2).sum()
    return np.concatenate([[len(x)], A[np.triu_indices(6)], J.T @ r, [d2]]), J, r


def plane_fit_host(sums, py, T):
    sums, py = (np.ascontiguousarray(v, dtype=np.float64) for v in (sums, py))
    Tk = np.ascontiguousarray(T[:3], dtype=np.float64)
    out = np.full(16, np.nan)
    flag = ctypes.c_int(-1)
    assert _native.lib().d3f_icp_plane_fit_host(sums.ctypes.data, py.ctypes.data, Tk.ctypes.data, out.ctypes.data,
                                                ctypes.byref(flag)) == 0
    return out.reshape(4, 4), flag.value


def step_numpy(J, r, T, py):
    v = np.linalg.lstsq(J, -r, rcond=None)[0]
    Rx = np.array([[1, 0, 0], [0, np.cos(v[0]), -np.sin(v[0])], [0, np.sin(v[0]), np.cos(v[0])]])
    Ry = np.array([[np.cos(v[1]), 0, np.sin(v[1])], [0, 1, 0], [-np.sin(v[1]), 0, np.cos(v[1])]])
    Rz = np.array([[np.cos(v[2]), -np.sin(v[2]), 0], [np.sin(v[2]), np.cos(v[2]), 0], [0, 0, 1]])
    D = Rz @ Ry @ Rx
    out = np.eye(4)
    out[:3, :3] = D @ T[:3, :3]
    out[:3, 3] = D @ (T[:3, 3] - py) + py + v[3:]
    return out


def plane_correspondences(rng, n, shift=(0.0, 0.0, 0.0)):
    """n fixed points y with unit normals, the moving points x that a random pose G maps onto them (with noise), and a
    pose T_k 2 degrees / 0.03 off G, everything moved by ``shift``."""
    y = rng.uniform(-1.5, 1.5, size=(n, 3))
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    G = sc.random_pose(rng)
    x = (y + rng.normal(scale=0.004, size=(n, 3)) - G[:3, 3]) @ G[:3, :3]
    T = G @ sc.perturbation(rng, 2, 0.03)
    s = np.asarray(shift)
    return (x + s).astype(np.float32), (y + s).astype(np.float32), nrm.astype(np.float32), sc.shift_pose(T, shift)


@pytest.mark.parametrize("shift", [(0.0, 0.0, 0.0), SHIFT], ids=["as-generated", "shifted"])
@pytest.mark.parametrize("n", [6, 50, 10000])
def test_plane_fit_host_matches_lstsq(n, shift):
    rng = np.random.default_rng(300 + n)
    x, y, nrm, T = plane_correspondences(rng, n, shift)
    py = y[0].astype(np.float64)
    sums, J, r = plane_sums(x, y, nrm, T, py)
    got, singular = plane_fit_host(sums, py, T)
    want = step_numpy(J, r, T, py)
    err = np.abs(got - want).max()
    print("n = %d: |T_next - T_numpy| = %.3g" % (n, err))
    assert singular == 0
    assert err < 1e-9
    Rn = got[:3, :3]
    assert np.abs(Rn @ Rn.T - np.eye(3)).max() < 1e-13 and (got[3] == [0, 0, 0, 1]).all()
    # the step reduces the point-to-plane residual it linearised
    r1 = (((x.astype(np.float64) @ got[:3, :3].T + got[:3, 3]) - y.astype(np.float64)) * nrm.astype(np.float64)).sum(1)
    if n > 6:
        assert (r1 ** 2).sum() < 0.1 * (r ** 2).sum()


def test_plane_fit_host_flags_a_single_plane_and_zero_normals():
    rng = np.random.default_rng(31)
    y = np.concatenate([rng.uniform(-1, 1, size=(500, 2)), np.full((500, 1), 0.25)], 1).astype(np.float32)
    x = (y.astype(np.float64) + [0.01, -0.02, 0.0]).astype(np.float32)
    nrm = np.tile(np.float32([0, 0, 1]), (500, 1))
    T = np.eye(4)
    T[:3, 3] = [0.0, 0.0, 0.004]
    py = y[0].astype(np.float64)
    got, singular = plane_fit_host(plane_sums(x, y, nrm, T, py)[0], py, T)
    assert singular == 1 and np.array_equal(got, T)
    got, singular = plane_fit_host(plane_sums(x, y, np.zeros_like(nrm), T, py)[0], py, T)
    assert singular == 1 and np.array_equal(got, T)
    # three planes in general position are enough
    third = len(y) // 3
    y2, n2 = y.copy(), nrm.copy()
    y2[:third] = y[:third][:, [2, 0, 1]]
    n2[:third] = [1, 0, 0]
    y2[third:2 * third] = y[third:2 * third][:, [0, 2, 1]]
    n2[third:2 * third] = [0, 1, 0]
    got, singular = plane_fit_host(plane_sums(y2, y2, n2, T, py)[0], py, T)
    assert singular == 0 and np.abs(got[:3, 3]).max() < 1e-9 and np.abs(got[:3, :3] - np.eye(3)).max() < 1e-9
    flag = ctypes.c_int(0)
    assert _native.lib().d3f_icp_plane_fit_host(None, py.ctypes.data, py.ctypes.data, py.ctypes.data,
                                                ctypes.byref(flag)) == -1


# ------------------------------------------------------------------------------------------------ the whole ICP
def perturbed_pairs(seed=4, degrees=2, shift=0.03):
    """The 6 pairs (moving j, fixed i), i < j, of make_scene(seed, 4), every ground truth ``degrees`` / ``shift`` off."""
    clouds, poses = sc.make_scene(seed, 4)
    rng = np.random.default_rng(seed + 1000)
    keys, pairs, G, T0 = [], [], [], []
    for i in range(4):
        for j in range(i + 1, 4):
            keys.append('%d_%d' % (i, j))
            pairs.append((j, i))
            G.append(sc.gt_transform(poses, i, j))
            T0.append(G[-1] @ sc.perturbation(rng, degrees, shift))
    return clouds, keys, np.asarray(pairs), np.stack(G), np.stack(T0)


def test_icp_numpy_point_to_plane_converges_faster_and_closer():
    """Float64 figures of the contract's restatement, 2 deg / 0.03 off, max_distance 0.075, normals at 0.1:
    pairs with healthy overlap: point-to-plane stops after 4-5 fits at 0.03-0.05 deg, point-to-point after 9-24 at
    0.05-0.10 deg; the low-overlap pairs 0_2 and 1_3 (mostly one plane) use all 30 fits and end WORSE (0.99 / 0.41 deg
    against 0.12 / 0.19 deg): they are asserted only to terminate with a finite pose."""
    clouds, keys, pairs, G, T0 = perturbed_pairs()
    normals, count = reg.estimate_normals_numpy(clouds, 0.1)
    assert normals.shape == (sum(len(c) for c in clouds), 3) and (count >= 1).all()
    for p, key in enumerate(keys):
        one = slice(p, p + 1)
        Tp, cp, rp, ip, sp, tr = reg.icp_numpy(clouds, pairs[one], T0[one], 0.075, normals=normals, return_trace=True)
        ep = sc.pose_error(Tp[0], G[p])
        assert np.isfinite(Tp).all() and 0 <= ip[0] <= 30 and sp[0] == 0
        assert tr[0, ip[0], 0] == cp[0] and abs(rp[0] - np.sqrt(tr[0, ip[0], 1] / cp[0])) < 1e-15
        if key in LOW_OVERLAP:
            print("%s: point-to-plane %d fits, %.3f deg / %.4f" % (key, ip[0], *ep))
            continue
        Tq, cq, rq, iq, sq = reg.icp_numpy(clouds, pairs[one], T0[one], 0.075)
        eq = sc.pose_error(Tq[0], G[p])
        print("%s: point-to-plane %d fits, %.3f deg / %.4f; point-to-point %d fits, %.3f deg / %.4f" % (
            key, ip[0], *ep, iq[0], *eq))
        assert 1 <= ip[0] < iq[0]
        assert ep[0] < eq[0]
    # a list of per-cloud normals is the stacked array
    ends = np.cumsum([len(c) for c in clouds])
    split = [normals[e - len(c):e] for e, c in zip(ends, clouds)]
    a = reg.icp_numpy(clouds, pairs[:1], T0[:1], 0.075, normals=split, max_iters=2)
    b = reg.icp_numpy(clouds, pairs[:1], T0[:1], 0.075, normals=normals, max_iters=2)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    with pytest.raises(ValueError):
        reg.icp_numpy(clouds, pairs[:1], T0[:1], 0.075, normals=normals[:-1])


def test_icp_numpy_flags_a_singular_overlap_and_keeps_the_pose():
    rng = np.random.default_rng(41)
    fixed = np.concatenate([rng.uniform(0, 1, size=(800, 2)), np.full((800, 1), 0.5)], 1).astype(np.float32)
    moving = np.concatenate([rng.uniform(0.2, 0.8, size=(300, 2)), np.full((300, 1), 0.5)], 1).astype(np.float32)
    normals, _ = reg.estimate_normals_numpy([moving, fixed], 0.2)
    assert (np.abs(normals[:, 2]) == 1).all()
    T0 = np.eye(4)
    T0[:3, 3] = [0.01, -0.01, 0.0]
    T, count, rmse, iters, status = reg.icp_numpy([moving, fixed], [(0, 1)], T0[None], 0.075, normals=normals)
    assert status[0] == reg.ICP_ST_SINGULAR and iters[0] == 0 and np.array_equal(T[0], T0) and count[0] == 300


def test_refine_transforms_estimation_keyword():
    clouds, poses = sc.make_scene(2, 2, n=9000)
    G = sc.gt_transform(poses, 0, 1)
    T0 = (G @ sc.perturbation(np.random.default_rng(6), 2, 0.03))[None]
    with pytest.raises(ValueError):
        reg.refine_transforms(clouds, [(0, 1)], T0, 0.075, device='cpu', estimation='plane')
    T, fitness, rmse, iters = reg.refine_transforms(clouds, [(0, 1)], T0, 0.075, device='cpu',
                                                    estimation='point_to_plane')
    normals = reg.estimate_normals_numpy(clouds, 0.15)[0]                  # normal_radius defaults to 2 max_distance
    want = reg.icp_numpy(clouds, [(1, 0)], T0, 0.075, normals=normals)
    assert np.array_equal(T, want[0]) and np.array_equal(iters, want[3])
    r0, t0 = sc.pose_error(T0[0], G)
    r1, t1 = sc.pose_error(T[0], G)
    assert r1 < r0 and t1 < t0 and 0.3 < fitness[0] <= 1.0
    same = reg.refine_transforms(clouds, [(0, 1)], T0, 0.075, device='cpu', max_iters=3)
    explicit = reg.refine_transforms(clouds, [(0, 1)], T0, 0.075, device='cpu', max_iters=3,
                                     estimation='point_to_point')
    assert all(np.array_equal(u, v) for u, v in zip(same, explicit))
