"""Fixtures of the FPFH tests (test_fpfh_cpu.py, test_fpfh_gpu.py): a bumpy terrain seen as two fragments -- FPFH is
weak on scenes that are mostly planes, so the room of icp_scene.py would test luck --, an oracle written independently
of the rule's construction (arctan2, arccos, float weights; the same acceptance and the same cap), and the edge cases
with their expected rows written out."""
import functools

import numpy as np

import icp_scene
from d3feat_pytorch_amd.geometric_registration import registration as reg

R_NORMAL, R_FPFH = 0.08, 0.2
# Seeds on which the restatement's mutual matches are inliers at 0.05 m often enough for RANSAC (0.21 and 0.26;
# test_fpfh_cpu.py asserts at least 0.15).  Of the seeds 1..7 the others draw 0.13 to 0.19: FPFH, not the code.
SEEDS = (5, 6)
VIEW = np.array([1.5, 1.0, 3.0])      # 3 m above the terrain, in the world


def terrain(rng, n=8000):
    """n points uniform on [0,3] x [0,2], z the sum of 12 sinusoids: bumps at every scale a 0.2 m descriptor sees."""
    xy = rng.uniform([0.0, 0.0], [3.0, 2.0], size=(n, 2))
    k = rng.uniform(4.0, 14.0, size=(12, 2)) * rng.choice([-1.0, 1.0], size=(12, 2))
    amp = 0.06 * rng.uniform(0.3, 1.0, size=12)
    phase = rng.uniform(0.0, 2.0 * np.pi, size=12)
    z = (amp * np.sin(xy @ k.T + phase)).sum(1)
    return np.concatenate([xy, z[:, None]], 1)


@functools.lru_cache(maxsize=None)
def scene(seed):
    """(clouds, poses, normals, views): two f32 fragments of one terrain around (1, 1, 0) and (2, 1, 0), each in its own
    frame, their fragment-to-world poses, the normals at R_NORMAL over the stacked rows (estimate_normals_numpy, one
    call per fragment: the normals are turned towards VIEW, which is a different point in each fragment's frame) and
    VIEW in each fragment's frame.  The frames stay where random_pose puts them, within ~2 m of the terrain: a pose error
    is measured at the frame's origin, and an origin moved to the viewpoint would multiply every rotation error by 3 m."""
    rng = np.random.default_rng(seed)
    world = terrain(rng)
    clouds, poses, views, normals = [], [], [], []
    for centre in ((1.0, 1.0, 0.0), (2.0, 1.0, 0.0)):
        pose = icp_scene.random_pose(rng)
        pose[:3, 3] *= 0.3
        clouds.append(icp_scene.fragment(rng, world, np.array(centre), pose, reach=1.0, keep=0.6, noise=0.002))
        inv = np.linalg.inv(pose)
        views.append((inv[:3, :3] @ VIEW + inv[:3, 3]).astype(np.float32))
        poses.append(pose)
        normals.append(reg.estimate_normals_numpy([clouds[-1]], R_NORMAL, viewpoint=views[-1])[0])
    normals = np.concatenate(normals)
    for c in clouds:
        c.setflags(write=False)
    normals.setflags(write=False)
    return clouds, poses, normals, views


def shifted(seed):
    """(clouds, poses) of scene(seed) with every fragment moved so that the viewpoint is its frame's origin: what a call
    that takes ONE viewpoint for all fragments (the origin) needs."""
    clouds, poses, _, views = scene(seed)
    out, moved = [], []
    for c, pose, view in zip(clouds, poses, views):
        out.append(icp_scene.shift_clouds([c], -view.astype(np.float64))[0])
        shift = np.eye(4)
        shift[:3, 3] = view
        moved.append(pose @ shift)
    return out, moved


@functools.lru_cache(maxsize=None)
def restated(seed):
    """(desc f32 [N,33], count, spfh, unit rows f32 [N,33]) of the stacked fragments at R_FPFH by the NumPy restatement;
    computed once."""
    clouds, _, normals, _ = scene(seed)
    out = reg.fpfh_numpy(list(clouds), R_FPFH, normals, return_spfh=True)
    out = out + (reg.fpfh_numpy(list(clouds), R_FPFH, normals, unit=True)[0],)
    for a in out:
        a.setflags(write=False)
    return out


def zeroed(normals, every=97):
    """The normals with every ``every``-th one set to zero: points without a descriptor among valid ones."""
    out = np.array(normals)
    out[::every] = 0.0
    return out


def oracle(cloud, normals, radius, cap=True):
    """(desc f64 [n,33], count [n], spfh int64 [n,33]) of ONE cloud the way Open3D's compute_fpfh_feature is written:
    arccos decides the role swap, arctan2 and a division bin the angle, the neighbours' histograms are normalised
    floats weighted by 1 / d2.  It shares with the rule only the acceptance of a neighbour and the cap on the weight."""
    p = np.asarray(cloud, dtype=np.float32)
    n = p.shape[0]
    nr = np.asarray(normals, dtype=np.float32)
    r32 = np.float32(radius)
    e = p[:, None, :] - p[None, :, :]
    d2f = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    P = p.astype(np.float64)
    dp = P[None, :, :] - P[:, None, :]                                   # [i, j] = p_j - p_i
    d2 = (dp[..., 0] * dp[..., 0] + dp[..., 1] * dp[..., 1]) + dp[..., 2] * dp[..., 2]
    usable = (nr != 0).any(1)
    ok = (d2f < r32 * r32) & (d2 != 0) & usable[:, None] & usable[None, :]
    ii, jj = np.nonzero(ok)
    N = nr.astype(np.float64)
    d, n1, n2 = dp[ii, jj], N[ii], N[jj]
    dist = np.linalg.norm(d, axis=1)
    a1, a2 = (n1 * d).sum(1) / dist, (n2 * d).sum(1) / dist
    swap = np.arccos(np.clip(np.abs(a1), 0, 1)) > np.arccos(np.clip(np.abs(a2), 0, 1))
    n1, n2 = np.where(swap[:, None], n2, n1), np.where(swap[:, None], n1, n2)
    d = np.where(swap[:, None], -d, d)
    f3 = np.where(swap, -a2, a1)
    v = np.cross(d, n1)
    vn = np.linalg.norm(v, axis=1)
    flat = vn == 0
    with np.errstate(all='ignore'):
        v = v / vn[:, None]
    w = np.cross(n1, v)
    f2 = (v * n2).sum(1)
    f1 = np.arctan2((w * n2).sum(1), (n1 * n2).sum(1))
    f1, f2, f3 = (np.where(flat, 0.0, f) for f in (f1, f2, f3))
    bins = [np.clip(np.floor(11 * (f1 + np.pi) / (2 * np.pi)), 0, 10), np.clip(np.floor(11 * (f2 + 1) * 0.5), 0, 10),
            np.clip(np.floor(11 * (f3 + 1) * 0.5), 0, 10)]
    spfh = np.zeros((n, 33), dtype=np.int64)
    for h in range(3):
        np.add.at(spfh, (ii, 11 * h + bins[h].astype(np.int64)), 1)
    count = ok.sum(1)
    with np.errstate(all='ignore'):
        hist = np.where(count[:, None] > 0, 100.0 * spfh / count[:, None], 0.0)     # Open3D's normalised SPFH
        ratio = float(r32) * float(r32) / d2
        wgt = np.where(ok, np.minimum(ratio, 4096.0) if cap else ratio, 0.0)
    acc = wgt @ hist
    desc = np.zeros((n, 33))
    for h in range(3):
        s = acc[:, 11 * h:11 * h + 11]
        tot = s.sum(1, keepdims=True)
        with np.errstate(all='ignore'):
            desc[:, 11 * h:11 * h + 11] = np.where(tot > 0, 100.0 * s / tot, 0.0) + hist[:, 11 * h:11 * h + 11]
    desc[count == 0] = 0.0
    return desc, count, spfh


def _row(theta, f2, f3):
    """A 33-wide row from {bin: value} per histogram."""
    out = np.zeros(33)
    for h, entries in enumerate((theta, f2, f3)):
        for b, v in entries.items():
            out[11 * h + b] = v
    return out


def _counts(theta, f2, f3):
    return _row(theta, f2, f3).astype(np.int32)


def edge_cases():
    """[(name, points f32 [n,3], normals f32 [n,3], radius, count [n], spfh [n,33], desc f32 [n,33])]: each one cloud,
    the expected values worked out by hand from the rule (csrc/fpfh.hpp)."""
    z, x0 = (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)
    none = np.zeros(33)
    f = lambda a: np.asarray(a, dtype=np.float32).reshape(-1, 3)
    cases = []
    cases.append(("one point", f([0.5, -0.25, 1.0]), f(z), 0.1, [0], [none], [none]))
    cases.append(("two coincident points", f([[0.25, 0.5, -1.0]] * 2), f([z, z]), 0.1, [0, 0], [none] * 2, [none] * 2))
    cases.append(("no neighbour in range", f([[0, 0, 0], [1, 0, 0]]), f([z, z]), 0.1, [0, 0], [none] * 2, [none] * 2))
    # A and C see each other, B between them has no normal.  A -> C: dp = (0, .05, 0) is perpendicular to both normals, so
    # a1 = a2 = 0, no swap, f3 = 0 (bin 5); v = dp x n_A = (1, 0, 0), f2 = v . n_C = 1 (bin 10); w = (0, 1, 0),
    # y = w . n_C = 0, x = n_A . n_C = 0 (bin 5).  C -> A gives the same bins.  One neighbour each: 100 + 100 per bin.
    pair = _row({5: 200.0}, {10: 200.0}, {5: 200.0})
    pair_c = _counts({5: 1}, {10: 1}, {5: 1})
    cases.append(("a zero normal among valid ones", f([[0, 0, 0], [0.05, 0, 0], [0, 0.05, 0]]), f([z, (0, 0, 0), x0]), 0.1,
                  [1, 0, 1], [pair_c, none, pair_c], [pair, none, pair]))
    # dp = (0, 0, .05) is parallel to the normals: v = dp x n = 0, all three bins are 5
    flat = _row({5: 200.0}, {5: 200.0}, {5: 200.0})
    flat_c = _counts({5: 1}, {5: 1}, {5: 1})
    cases.append(("a neighbour on dp parallel to n", f([[0, 0, 0], [0, 0, 0.05]]), f([z, z]), 0.1, [1, 1],
                  [flat_c] * 2, [flat] * 2))
    # The cap.  A = 0, B = (.001, 0, 0) (closer than radius / 64), C = (0, .05, 0); n_A = n_B = z, n_C = x.  A <-> B: bins
    # (5, 5, 5); A <-> C: (5, 10, 5) as above; B <-> C: a1 = 0, |a2| = .02: the roles swap, f3 = .02 (bin 5), v = (0, 0, 1),
    # f2 = 1 (bin 10), x = y = 0 (bin 5).  So c_A = c_B = {theta 5: 2, f2 5: 1, f2 10: 1, f3 5: 2}, c_C = {theta 5: 2,
    # f2 10: 2, f3 5: 2}, n = 2 everywhere.  Weights: W(A, B) = 2^32 2^12 / 2 = 2^43 (capped: radius^2 / d2 is 10^4);
    # W(A, C) = 2^32 4 / 2 = 2^33 (.1f is exactly twice .05f); W(B, C) = rint(2^32 (r2 / d2) / 2).
    r2 = float(np.float32(0.1)) * float(np.float32(0.1))
    d2_bc = float(np.float32(0.001)) * float(np.float32(0.001)) + float(np.float32(0.05)) * float(np.float32(0.05))
    w_ab, w_ac, w_bc = 2 ** 43, 2 ** 33, int(np.rint(2.0 ** 32 * (r2 / d2_bc) / 2.0))

    def f2_row(near, far):   # near: the weight of the neighbour with f2 counts {5: 1, 10: 1}; far: of C's {10: 2}
        s5, s10 = near, near + 2 * far
        return {5: 100.0 * s5 / (s5 + s10) + 50.0, 10: 100.0 * s10 / (s5 + s10) + 50.0}
    ab_c = _counts({5: 2}, {5: 1, 10: 1}, {5: 2})
    cases.append(("a pair closer than radius / 64", f([[0, 0, 0], [0.001, 0, 0], [0, 0.05, 0]]), f([z, z, x0]), 0.1,
                  [2, 2, 2], [ab_c, ab_c, _counts({5: 2}, {10: 2}, {5: 2})],
                  [_row({5: 200.0}, f2_row(w_ab, w_ac), {5: 200.0}), _row({5: 200.0}, f2_row(w_ab, w_bc), {5: 200.0}),
                   _row({5: 200.0}, {5: 50.0, 10: 150.0}, {5: 200.0})]))
    return [(name, p, nr, r, np.asarray(c, dtype=np.int32), np.stack(s).astype(np.int32),
             np.stack(d).astype(np.float32)) for name, p, nr, r, c, s, d in cases]


def mutual_numpy(a, b):
    """Mutual nearest neighbours of two descriptor blocks by L2 distance in f64: (rows of a, their rows of b)."""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    d = (a64 * a64).sum(1)[:, None] - 2.0 * (a64 @ b64.T) + (b64 * b64).sum(1)[None, :]
    ab, ba = d.argmin(1), d.argmin(0)
    rows = np.nonzero(ba[ab] == np.arange(a.shape[0]))[0]
    return rows, ab[rows]
