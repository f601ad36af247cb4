"""CPU: coloured ICP.  The colour gradient through its host twin (d3f_color_gradient_from_moments_host;
csrc/color_icp.hpp) against a NumPy solve, and the NumPy restatements of both contracts
(registration.color_gradients_numpy, registration.icp_numpy(color_field=)) on the cases of colored_icp_cases.py: the
plane slide, which neither point-to-plane nor point-to-point ICP can hold, the room of the point-to-plane tests, a linear
intensity ramp and the small scene."""
import numpy as np
import pytest

from d3feat_pytorch_amd import _native
from d3feat_pytorch_amd.datasets import fragments as fr
from d3feat_pytorch_amd.datasets.ThreeDMatch import read_ply_points
from d3feat_pytorch_amd.geometric_registration import registration as reg
import colored_icp_cases as cc
import icp_scene as sc
from test_normals_plane_cpu import LOW_OVERLAP

R, R_GRAD = cc.R_ICP, cc.R_GRAD


def gradient_host(m, Q, nrm, intensity, min_neighbors=4):
    m = np.ascontiguousarray(m, dtype=np.int64)
    nrm = np.ascontiguousarray(nrm, dtype=np.float32)
    out = np.zeros(4, dtype=np.float32)
    assert _native.lib().d3f_color_gradient_from_moments_host(m.ctypes.data, float(Q), nrm.ctypes.data,
                                                              float(np.float32(intensity)), int(min_neighbors),
                                                              out.ctypes.data) == 0
    return out


def gradient_numpy(m, Q, nrm):
    """(d, valid): the contract's gradient with numpy.linalg.solve on the 2x2, and the contract's pivot test."""
    nv = nrm.astype(np.float64)
    k = int(np.argmin(np.abs(nv)))                                     # (argmin: the lowest index on ties)
    e1 = np.cross(nv, np.eye(3)[k])
    e1 /= np.linalg.norm(e1)
    E = np.stack([e1, np.cross(nv, e1)], 1)
    S = m[[4, 5, 6, 5, 7, 8, 6, 8, 9]].astype(np.float64).reshape(3, 3) / (Q * Q)
    h = m[10:13].astype(np.float64) / (Q * 2.0 ** 20)
    G = E.T @ S @ E
    if not np.linalg.det(G) > 1e-6 * max(G[0, 0], G[1, 1]) ** 2:
        return None, False
    return E @ np.linalg.solve(G, E.T @ h), True


@pytest.fixture(scope="module")
def small():
    clouds, cols = cc.small()
    normals = reg.estimate_normals_numpy(clouds, R_GRAD)[0]
    field, count, moments = reg.color_gradients_numpy(clouds, R_GRAD, normals, np.concatenate(cols),
                                                      return_moments=True)
    return clouds, cols, normals, field, count, moments


def test_gradient_host_matches_a_numpy_solve(small):
    clouds, cols, normals, field, count, moments = small
    inten = np.concatenate(cols)
    Q = reg.normals_scale(R_GRAD)
    assert Q == 2.0 ** 23 and int(np.abs(moments[:, 10:]).max()) <= int(count.max()) * 2 ** 40
    rows = np.arange(0, len(inten), 9)
    rows = rows[count[rows] >= 4]
    assert len(rows) >= 300
    worst, valid = 0.0, 0
    for i in rows:
        got = gradient_host(moments[i], Q, normals[i], inten[i])
        want, ok = gradient_numpy(moments[i], Q, normals[i])
        assert got[3] == inten[i]
        assert np.isfinite(got[:3]).all() == ok, i
        assert np.array_equal(np.isnan(got), np.isnan(field[i])), i    # the restatement states the same rule
        if ok:
            assert np.abs(got - field[i]).max() <= 1e-6 * max(1.0, np.abs(want).max()), i
            valid += 1
            err = np.abs(got[:3].astype(np.float64) - want).max() / max(1.0, np.abs(want).max())
            worst = max(worst, err)
            assert abs(got[:3].astype(np.float64) @ normals[i].astype(np.float64)) <= 1e-6 * max(1.0, np.abs(want).max())
    print("%d neighbourhoods, %d valid: worst |d - d_numpy| / max(1, |d|) = %.3g" % (len(rows), valid, worst))
    assert valid >= 250 and worst < 1e-6


def test_invalid_gradients_are_exactly_three_nans(small):
    clouds, cols, normals, field, count, moments = small
    Q = reg.normals_scale(R_GRAD)
    i = int(np.argmax(count))
    m, nrm, I = moments[i], normals[i], np.concatenate(cols)[i]
    good = gradient_host(m, Q, nrm, I)
    assert np.isfinite(good).all() and abs(good[:3].astype(np.float64) @ nrm.astype(np.float64)) < 1e-6

    def bad(out, w):
        return np.isnan(out[:3]).all() and (np.isnan(out[3]) if w is None else out[3] == np.float32(w))
    assert bad(gradient_host(m, Q, nrm, I, min_neighbors=int(m[0]) + 1), I)           # n < min_neighbors
    assert np.isfinite(gradient_host(m, Q, nrm, I, min_neighbors=int(m[0]))).all()
    assert bad(gradient_host(m, Q, np.zeros(3), I), I)                                # a zero normal
    u = np.array([[k * 1000, -k * 500, k * 250] for k in range(-5, 6)], dtype=np.int64)   # collinear neighbours
    c = np.arange(-5, 6, dtype=np.int64) * 777
    line = np.array([len(u), *u.sum(0), (u[:, 0] ** 2).sum(), (u[:, 0] * u[:, 1]).sum(), (u[:, 0] * u[:, 2]).sum(),
                     (u[:, 1] ** 2).sum(), (u[:, 1] * u[:, 2]).sum(), (u[:, 2] ** 2).sum(), *(u * c[:, None]).sum(0)])
    assert bad(gradient_host(line, Q, np.float32([0.0, 0.4472136, 0.8944272]), 0.5), 0.5)
    for own in (np.nan, -0.1, 1.5):                                                   # the point's own intensity
        assert bad(gradient_host(m, Q, nrm, own), None), own
    # the restatement agrees on each of them, and on the intensity rule of the moments
    f = reg.color_field_from_moments(np.stack([m, m, line, m]), Q, np.stack([nrm, np.zeros(3, np.float32),
                                     np.float32([0.0, 0.4472136, 0.8944272]), nrm]), np.float32([I, I, 0.5, 1.5]))
    assert np.isfinite(f[0]).all() and np.isnan(f[1:, :3]).all() and np.isnan(f[3, 3]) and f[2, 3] == 0.5
    cloud = clouds[0][:400]
    inten = cols[0][:400].copy()
    inten[[3, 50]] = [np.nan, 1.5]
    nr = reg.estimate_normals_numpy([cloud], R_GRAD)[0]
    f, n, mm = reg.color_gradients_numpy([cloud], R_GRAD, nr, inten, return_moments=True)
    assert np.isnan(f[[3, 50]]).all() and (n[[3, 50]] == 0).all() and (mm[[3, 50]] == 0).all()
    assert np.isfinite(f[np.isfinite(f[:, 0])]).all()
    base = reg.color_gradients_numpy([cloud], R_GRAD, nr, cols[0][:400])[1]
    assert (n <= base).all() and (n < base).sum() >= 2                # the two rows count for nobody else either
    L = _native.lib()
    out = np.zeros(4, dtype=np.float32)
    assert L.d3f_color_gradient_from_moments_host(None, 1.0, out.ctypes.data, 0.5, 4, out.ctypes.data) == -1
    assert L.d3f_color_gradient_from_moments_host(m.ctypes.data, 0.0, out.ctypes.data, 0.5, 4, out.ctypes.data) == -1


def test_color_gradients_numpy_is_permutation_invariant(small):
    clouds, cols, normals, field, count, moments = small
    k = len(clouds[0])
    perm = np.random.default_rng(12).permutation(k)
    f2, c2, m2 = reg.color_gradients_numpy([clouds[0][perm]], R_GRAD, normals[:k][perm], cols[0][perm],
                                           return_moments=True)
    assert np.array_equal(m2, moments[:k][perm]) and np.array_equal(c2, count[:k][perm])
    assert np.array_equal(f2, field[:k][perm], equal_nan=True)
    assert moments.dtype == np.int64 and moments.shape[1] == 13 and (moments[:, 10:] != 0).any()
    # a list of per-cloud arrays is the stacked array
    ends = np.cumsum([len(c) for c in clouds])
    split = [normals[e - len(c):e] for e, c in zip(ends, clouds)]
    f3 = reg.color_gradients_numpy(clouds, R_GRAD, split, cols)[0]
    assert np.array_equal(f3, field, equal_nan=True)
    with pytest.raises(ValueError):
        reg.color_gradients_numpy(clouds, R_GRAD, normals[:-1], np.concatenate(cols))
    with pytest.raises(ValueError):
        reg.color_gradients_numpy(clouds, 0.0, normals, np.concatenate(cols))


def test_ramp_gradient_is_exact():
    """A linear intensity over a noise-free plane: the least-squares slope is the exact gradient up to the quantisation
    of the intensity (2^-20 over a lever of ~0.05) and the f32 coordinates."""
    cloud, inten, normal, want = cc.ramp()
    nr = reg.estimate_normals_numpy([cloud], R_GRAD)[0]
    assert np.abs(np.abs(nr.astype(np.float64) @ normal) - 1).max() < 1e-5
    field, count = reg.color_gradients_numpy([cloud], R_GRAD, nr, inten)
    assert np.isfinite(field).all() and np.array_equal(field[:, 3], inten)
    worst = np.abs(field[:, :3].astype(np.float64) - want).max()
    print("ramp: %d..%d neighbours, worst |d - exact| = %.3g" % (count.min(), count.max(), worst))
    assert worst < 1e-4


# ------------------------------------------------------------------------------------------------ the whole ICP
@pytest.fixture(scope="module")
def slide():
    clouds, cols, G, T0 = cc.plane_slide()
    normals = reg.estimate_normals_numpy(clouds, R_GRAD)[0]
    field = reg.color_gradients_numpy(clouds, R_GRAD, normals, np.concatenate(cols))[0]
    return clouds, cols, G, T0, normals, field


def test_plane_slide_is_held_by_colour_alone(slide):
    """Two samples of ONE textured plane, 1.5 deg about the normal and 30 mm along the plane off: the point-to-plane
    residual does not see that error at all.  NumPy f64 figures: coloured 5 fits, 0.0086 deg / 0.31 mm; point-to-plane
    30 fits, 2.2 deg / 108 mm (it drifts further away)."""
    clouds, cols, G, T0, normals, field = slide
    T, count, rmse, iters, status, n_color, color_rmse = reg.icp_numpy(clouds, [(1, 0)], T0[None], R, normals=normals,
                                                                       color_field=field)
    deg, shift = sc.pose_error(T[0], G)
    print("coloured: %d fits, %.4f deg / %.3f mm, n_color %d of %d, colour rmse %.4f" % (
        iters[0], deg, 1e3 * shift, n_color[0], count[0], color_rmse[0]))
    assert status[0] == 0 and iters[0] <= 10
    assert deg < 0.05 and shift < 1e-3
    assert 0 < n_color[0] <= count[0] and 0 < color_rmse[0] < 0.05
    Tp, _, _, ip, sp = reg.icp_numpy(clouds, [(1, 0)], T0[None], R, normals=normals)
    degp, shiftp = sc.pose_error(Tp[0], G)
    print("point-to-plane: %d fits, status %d, %.3f deg / %.1f mm" % (ip[0], sp[0], degp, 1e3 * shiftp))
    assert degp > 1.0


def test_identities_of_the_coloured_restatement(slide):
    clouds, cols, G, T0, normals, field = slide
    kw = dict(max_iters=3, return_trace=True)
    # lambda_geometric = 1: the point-to-plane run, exactly
    a = reg.icp_numpy(clouds, [(1, 0)], T0[None], R, normals=normals, color_field=field, lambda_geometric=1.0, **kw)
    b = reg.icp_numpy(clouds, [(1, 0)], T0[None], R, normals=normals, **kw)
    assert all(np.array_equal(u, v, equal_nan=True) for u, v in zip(a[:6], b)) and a[6][0] > 0
    # max_iters = 0: the point-to-point search
    a = reg.icp_numpy(clouds, [(1, 0)], T0[None], R, normals=normals, color_field=field, max_iters=0, return_trace=True)
    b = reg.icp_numpy(clouds, [(1, 0)], T0[None], R, max_iters=0, return_trace=True)
    assert all(np.array_equal(u, v) for u, v in zip(a[:6], b)) and a[3][0] == 0 and a[6][0] > 0
    # no usable intensity anywhere: no colour row, and the point-to-plane trajectory (every row scaled by the same
    # sqrt(lambda) leaves the least-squares solution where it was, to rounding)
    dark = reg.color_gradients_numpy(clouds, R_GRAD, normals, np.full(len(field), np.nan, dtype=np.float32))[0]
    assert np.isnan(dark).all()
    a = reg.icp_numpy(clouds, [(1, 0)], T0[None], R, normals=normals, color_field=dark, **kw)
    b = reg.icp_numpy(clouds, [(1, 0)], T0[None], R, normals=normals, **kw)
    assert a[6][0] == 0 and a[7][0] == 0.0
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]) and np.array_equal(a[5][..., 0], b[5][..., 0],
                                                                                      equal_nan=True)
    assert np.abs(a[0] - b[0]).max() < 1e-9
    with pytest.raises(ValueError):
        reg.icp_numpy(clouds, [(1, 0)], T0[None], R, color_field=field)
    with pytest.raises(ValueError):
        reg.icp_numpy(clouds, [(1, 0)], T0[None], R, normals=normals, color_field=field, lambda_geometric=1.5)
    with pytest.raises(ValueError):
        reg.icp_numpy(clouds, [(1, 0)], T0[None], R, normals=normals, color_field=field[:-1])


def test_room_pairs_with_low_overlap_converge():
    """The six pairs of the point-to-plane tests, 2 deg / 0.03 off.  NumPy f64 figures (coloured against point-to-plane):
    0_1 0.025 deg / 0.44 mm in 5 fits (0.033 / 1.07, 5); 0_2 0.027 / 1.07, 7 (0.989 / 10.4, 30); 0_3 0.041 / 1.08, 4
    (0.034 / 0.62, 5); 1_2 0.031 / 0.54, 4 (0.051 / 0.64, 4); 1_3 0.047 / 1.50, 4 (0.408 / 7.4, 30); 2_3 0.050 / 1.23, 5
    (0.050 / 1.03, 4)."""
    clouds, cols, keys, pairs, G, T0 = cc.room()
    normals = reg.estimate_normals_numpy(clouds, R_GRAD)[0]
    field = reg.color_gradients_numpy(clouds, R_GRAD, normals, np.concatenate(cols))[0]
    assert np.isfinite(field).all(1).mean() > 0.99
    T, count, rmse, iters, status, n_color, color_rmse = reg.icp_numpy(clouds, pairs, T0, R, normals=normals,
                                                                       color_field=field)
    for p, key in enumerate(keys):
        deg, shift = sc.pose_error(T[p], G[p])
        line = "%s: coloured %d fits, %.3f deg / %.2f mm, n_color %d of %d" % (key, iters[p], deg, 1e3 * shift,
                                                                               n_color[p], count[p])
        if key in LOW_OVERLAP:
            Tp, _, _, ip, _ = reg.icp_numpy(clouds, pairs[p:p + 1], T0[p:p + 1], R, normals=normals)
            degp, shiftp = sc.pose_error(Tp[0], G[p])
            line += "; point-to-plane %d fits, %.3f deg / %.2f mm" % (ip[0], degp, 1e3 * shiftp)
        print(line)
        assert status[p] == 0 and deg < 0.1 and shift < 2.5e-3, key
        if key in LOW_OVERLAP:
            assert iters[p] <= 12 and deg < degp and shift < shiftp, key


# ------------------------------------------------------------------------------------------------ the front end
def test_refine_transforms_colored_on_the_cpu(slide):
    clouds, cols, G, T0, normals, field = slide
    want = reg.icp_numpy(clouds, [(1, 0)], T0[None], R, normals=normals, color_field=field)
    rgb = [np.repeat(c[:, None], 3, 1) for c in cols]                  # grey as RGB: the weights sum to 1 (to rounding)
    T, fitness, rmse, iters = reg.refine_transforms(clouds, [(0, 1)], T0[None], R, device='cpu', estimation='colored',
                                                    normal_radius=R_GRAD, colors=[c[:, None] for c in cols])
    assert np.array_equal(T, want[0]) and np.array_equal(iters, want[3]) and np.array_equal(rmse, want[2])
    assert fitness[0] == want[1][0] / len(clouds[1])
    T3 = reg.refine_transforms(clouds, [(0, 1)], T0[None], R, device='cpu', estimation='colored', normal_radius=R_GRAD,
                               colors=rgb)[0]
    assert sc.pose_error(T3[0], G)[0] < 0.05 and np.abs(T3 - T).max() < 1e-4
    one = reg.refine_transforms(clouds, [(0, 1)], T0[None], R, device='cpu', estimation='colored', normal_radius=R_GRAD,
                                colors=cols, lambda_geometric=1.0, max_iters=2)
    plane = reg.refine_transforms(clouds, [(0, 1)], T0[None], R, device='cpu', estimation='point_to_plane',
                                  normal_radius=R_GRAD, max_iters=2)
    assert all(np.array_equal(u, v) for u, v in zip(one, plane))
    with pytest.raises(ValueError):
        reg.refine_transforms(clouds, [(0, 1)], T0[None], R, device='cpu', estimation='colored')
    with pytest.raises(ValueError):
        reg.refine_transforms(clouds, [(0, 1)], T0[None], R, device='cpu', estimation='colored', colors=cols[:1])
    with pytest.raises(ValueError):
        reg.refine_transforms(clouds, [(0, 1)], T0[None], R, device='cpu', estimation='coloured', colors=cols)


def test_read_ply_colors_round_trips_write_ply_points(tmp_path):
    rng = np.random.default_rng(5)
    pts = rng.normal(size=(257, 3)).astype(np.float32)
    rgb8 = rng.integers(0, 256, size=(257, 3)).astype(np.uint8)
    colors = rgb8.astype(np.float32) / np.float32(255.0)
    name = str(tmp_path / 'c.ply')
    fr.write_ply_points(name, pts, colors=colors)
    got = fr.read_ply_colors(name)
    assert got.dtype == np.float32 and np.array_equal(got, colors)
    assert np.array_equal(read_ply_points(name), pts.astype(np.float64))
    fr.write_ply_points(name, pts, colors=colors[:, :1])               # one channel is written as grey
    assert np.array_equal(fr.read_ply_colors(name), np.repeat(colors[:, :1], 3, 1))
    fr.write_ply_points(name, pts)
    assert fr.read_ply_colors(name) is None
    with open(name, 'w') as f:                                         # an ascii file
        f.write("ply\nformat ascii 1.0\nelement vertex 2\nproperty float x\nproperty float y\nproperty float z\n"
                "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n"
                "0 0 0 255 0 51\n1 2 3 0 102 255\n")
    assert np.array_equal(fr.read_ply_colors(name), np.float32([[255, 0, 51], [0, 102, 255]]) / np.float32(255.0))
    with open(name, 'w') as f:
        f.write("not a ply\n")
    with pytest.raises(ValueError):
        fr.read_ply_colors(name)
    # register_scene's reader of a folder of fragments
    for i in range(2):
        fr.write_ply_points(str(tmp_path / ('cloud_bin_%d.ply' % i)), pts, colors=colors if i == 0 else None)
    assert np.array_equal(reg._scene_colors(str(tmp_path), [0], [257])[0], colors)
    with pytest.raises(ValueError):
        reg._scene_colors(str(tmp_path), [0, 1], [257, 257])           # fragment 1 has no colours
    with pytest.raises(ValueError):
        reg._scene_colors(str(tmp_path), [0], [256])
    with pytest.raises(ValueError):
        reg._scene_colors(None, [0], [257])


def test_intensity_of():
    import torch
    rng = np.random.default_rng(6)
    rgb = rng.uniform(size=(100, 3)).astype(np.float32)
    want = (np.float32(0.299) * rgb[:, 0] + np.float32(0.587) * rgb[:, 1]) + np.float32(0.114) * rgb[:, 2]
    got = reg.intensity_of(rgb)
    assert got.dtype == np.float32 and got.shape == (100,) and np.array_equal(got, want)
    assert np.array_equal(reg.intensity_of(rgb[:, :1]), rgb[:, 0]) and np.array_equal(reg.intensity_of(rgb[:, 0]), rgb[:, 0])
    rgb8 = rng.integers(0, 256, size=(100, 3)).astype(np.uint8)
    f = rgb8.astype(np.float32)
    want8 = ((np.float32(0.299) * f[:, 0] + np.float32(0.587) * f[:, 1]) + np.float32(0.114) * f[:, 2]) / np.float32(255)
    assert np.array_equal(reg.intensity_of(rgb8), want8)
    assert np.array_equal(reg.intensity_of(rgb8[:, :1]), f[:, 0] / np.float32(255))
    assert (reg.intensity_of(rgb8) <= 1.0).all() and reg.intensity_of(np.uint8([[255, 255, 255]]))[0] <= 1.0
    t = reg.intensity_of(torch.from_numpy(rgb))
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float32 and np.array_equal(t.numpy(), want)
    assert np.array_equal(reg.intensity_of(torch.from_numpy(rgb8)).numpy(), want8)
    nan = reg.intensity_of(np.float32([[np.nan, 0.5, 0.5]]))
    assert np.isnan(nan).all()
    with pytest.raises(ValueError):
        reg.intensity_of(rgb[:, :2])
