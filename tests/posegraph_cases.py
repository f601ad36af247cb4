"""Pose graphs for the multiway-registration tests (test_posegraph_cpu.py, test_posegraph_gpu.py): the benchmark scene
of tests/golden/posegraph_lab_hj.npz with seeded corruption of its loop edges, and synthetic ring-plus-chords graphs."""
import functools
import os

import numpy as np

from d3feat_pytorch_amd.geometric_registration import registration as reg

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_DISTANCE = 0.05            # the distance the benchmark's gt.info was computed at


def exp(t, w):
    """Exp([t, w]) = [[R(w), t], [0, 1]] (Rodrigues)."""
    w = np.asarray(w, dtype=np.float64)
    a = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    out = np.eye(4)
    out[:3, :3] = np.eye(3) + (K + K @ K / 2 if a < 1e-9 else np.sin(a) / a * K + (1 - np.cos(a)) / a ** 2 * K @ K)
    out[:3, 3] = t
    return out


def pose_errors(P, truth):
    """(largest translation error in metres, largest rotation error in degrees) of the poses P against truth."""
    dt = np.linalg.norm(P[:, :3, 3] - truth[:, :3, 3], axis=1).max()
    R = np.einsum('kab,kac->kbc', truth[:, :3, :3], P[:, :3, :3])
    v = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], 1)
    ang = np.arctan2(np.linalg.norm(v, axis=1) / 2, (np.trace(R, axis1=1, axis2=2) - 1) / 2)
    return float(dt), float(np.rad2deg(ang).max())


def components(N, edges, removed=()):
    active = np.ones(len(edges), dtype=bool)
    active[list(removed)] = False
    return reg._components_numpy(N, np.asarray(edges, dtype=np.int64), active)


@functools.lru_cache(maxsize=None)
def fixture():
    """(num_nodes, edges int64 [E,2], T, info, uncertain, truth): the scene as recorded; truth = the spanning-tree poses
    of the uncorrupted file, per component."""
    f = np.load(os.path.join(HERE, 'golden', 'posegraph_lab_hj.npz'))
    N, edges, T, info = int(f['num_nodes']), f['edges'].astype(np.int64), f['T'], f['info']
    unc = edges[:, 1] - edges[:, 0] > 1
    return N, edges, T, info, unc, reg.spanning_tree_poses(N, edges, T, unc)


@functools.lru_cache(maxsize=None)
def corrupted(fraction, seed):
    """The fixture with ``fraction`` of its loop edges replaced by gross errors and the initial poses disturbed.  Loop
    edges are tried in a random order and one is taken only if the components stay as they are without it and those
    already taken (a corrupted bridge contradicts nothing: no method can find it).  Z <- Z Exp([t, w]), |t_k| uniform
    in 0.3-1 m with random signs, |w| uniform in 20-90 degrees about a random axis; initial poses = truth Exp(N(0, 0.05
    m), N(0, 3 deg)) per axis with the gauge nodes exact.  Returns (Z, poses0, sorted corrupted edge indices)."""
    N, edges, T, info, unc, truth = fixture()
    rng = np.random.default_rng(seed)
    loops = np.nonzero(unc)[0]
    want = int(fraction * len(loops))
    base = components(N, edges)
    chosen = []
    for e in rng.permutation(loops):
        if len(chosen) == want:
            break
        if np.array_equal(components(N, edges, chosen + [int(e)]), base):
            chosen.append(int(e))
    assert len(chosen) == want
    Z = T.copy()
    for e in chosen:
        t = rng.uniform(0.3, 1.0, 3) * rng.choice([-1.0, 1.0], 3)
        axis = rng.normal(size=3)
        Z[e] = Z[e] @ exp(t, axis / np.linalg.norm(axis) * np.deg2rad(rng.uniform(20, 90)))
    P0 = truth.copy()
    for k in range(N):
        if base[k] != k:
            P0[k] = P0[k] @ exp(rng.normal(0, 0.05, 3), rng.normal(0, np.deg2rad(3), 3))
    return Z, P0, sorted(chosen)


def point_information(rng, count=60, spread=1.0):
    """An information matrix in the project's default form from ``count`` random points: sum G^T G, G = [I | -[p]x]."""
    p = rng.normal(scale=spread, size=(count, 3))
    L = np.zeros((6, 6))
    for q in p:
        G = np.concatenate([np.eye(3), -np.array([[0, -q[2], q[1]], [q[2], 0, -q[0]], [-q[1], q[0], 0]])], 1)
        L += G.T @ G
    return L


@functools.lru_cache(maxsize=None)
def ring(N, seed=0, corrupt=True, noise=True):
    """A ring of N nodes with chords: certain edges (k, k+1), uncertain closing edge and chords (k, k + 2 + k % 3) for
    every third k, every other chord given reversed as (j, i) with inv(Z), the first chord duplicated, and (with
    ``corrupt``, N >= 6) one chord replaced by a gross error.  Returns a dict: N, edges, Z, info, unc, truth, poses0
    (truth disturbed by 2 cm / 1 degree, node 0 exact), bad (indices of the corrupted edges)."""
    rng = np.random.default_rng(1000 * N + seed)
    truth = np.stack([exp(rng.normal(0, 1.0, 3), rng.normal(0, 0.8, 3)) for _ in range(N)])
    truth[0] = np.eye(4) if N else truth[0]
    pairs, unc = [], []
    for k in range(N - 1):
        pairs.append((k, k + 1))
        unc.append(False)
    if N >= 3:
        pairs.append((0, N - 1))
        unc.append(True)
    chords = [(k, k + 2 + k % 3) for k in range(0, N, 3) if k + 2 + k % 3 < N and (k, k + 2 + k % 3) != (0, N - 1)]
    for n, (i, j) in enumerate(chords):
        pairs.append((j, i) if n % 2 else (i, j))
        unc.append(True)
    if chords:
        pairs.append(chords[0])
        unc.append(True)
    edges = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    Z = np.stack([np.linalg.inv(truth[i]) @ truth[j] for i, j in edges]) if len(edges) else np.zeros((0, 4, 4))
    info = np.stack([point_information(rng) for _ in edges]) if len(edges) else np.zeros((0, 6, 6))
    bad = []
    if corrupt and N >= 6 and len(chords) >= 2:
        e = (N - 1) + 1 + 1                                    # the second chord
        Z[e] = Z[e] @ exp([0.6, -0.4, 0.5], [0.5, 0.3, -0.6])
        bad = [e]
    P0 = truth.copy()
    if noise:
        for k in range(1, N):
            P0[k] = P0[k] @ exp(rng.normal(0, 0.02, 3), rng.normal(0, np.deg2rad(1), 3))
    return dict(N=N, edges=edges, Z=Z, info=info, unc=np.asarray(unc, dtype=bool), truth=truth, poses0=P0, bad=bad)


def stack(graphs):
    """(poses0, edges, Z, info, unc, node_start, edge_start) of several ``ring``-style dicts stacked into one batch."""
    ns = np.cumsum([0] + [g['N'] for g in graphs])
    es = np.cumsum([0] + [len(g['edges']) for g in graphs])
    cat = lambda k, tail: np.concatenate([np.asarray(g[k]).reshape((-1,) + tail) for g in graphs])
    return (cat('poses0', (4, 4)), cat('edges', (2,)), cat('Z', (4, 4)), cat('info', (6, 6)), cat('unc', ()), ns, es)


def fixture_graph(fraction=0.15, seed=0):
    """The corrupted fixture as a ``ring``-style dict."""
    N, edges, T, info, unc, truth = fixture()
    Z, P0, bad = corrupted(fraction, seed)
    return dict(N=N, edges=edges, Z=Z, info=info, unc=unc, truth=truth, poses0=P0, bad=bad)
