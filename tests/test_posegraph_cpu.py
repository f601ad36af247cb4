"""CPU: robust pose-graph optimisation through the host twin of the kernel (d3f_pose_graph_optimize_host -- the text of
csrc/posegraph.hpp run by one worker) and through its NumPy restatement (registration.pose_graph_numpy): recovery of the
truth and of the exact corrupted set on a benchmark scene, the two against each other, the Jacobians against central
differences, the shapes where the block and incidence arithmetic can go wrong, the gauge, the spanning-tree start and
the front end on the CPU.

Bounds.  The fixture is consistent with itself to 2e-5 (the precision of its text), so poses are asked to come within
1e-3 m / 0.01 degrees of the truth, 50 times that.  Host twin and restatement solve the same normal equations in f64
by different routes and are asked to agree to 1e-6, the bound tests/test_icp_gpu.py sets between device and NumPy."""

import numpy as np
import pytest
import torch

import posegraph_cases as pc
from d3feat_pytorch_amd import _native, ops
from d3feat_pytorch_amd.geometric_registration import registration as reg

CASES = [(0.15, 0), (0.15, 1), (0.30, 0), (0.30, 1)]


def host(g, **kw):
    out = ops.pose_graph_optimize_host(g['poses0'], g['edges'], g['Z'], g['info'], g['unc'], pc.MAX_DISTANCE, **kw)
    return [t.numpy() for t in out]


def restated(g, **kw):
    return list(reg.pose_graph_numpy(g['poses0'], g['edges'], g['Z'], g['info'], g['unc'], pc.MAX_DISTANCE, **kw))


_RESULTS = {}


def fixture_result(which, fraction, seed):
    key = (which, fraction, seed)
    if key not in _RESULTS:
        _RESULTS[key] = (host if which == 'host' else restated)(pc.fixture_graph(fraction, seed))
    return _RESULTS[key]


def test_fixture_is_the_scene_the_issue_describes():
    N, edges, T, info, unc, truth = pc.fixture()
    assert (N, len(edges), int((~unc).sum())) == (38, 77, 32)
    assert len(set(pc.components(N, edges).tolist())) == 4
    assert [len(pc.corrupted(f, 0)[2]) for f in (0.15, 0.30)] == [6, 13]


@pytest.mark.parametrize("which", ["host", "numpy"])
@pytest.mark.parametrize("fraction,seed", CASES)
def test_truth_and_corrupted_set_are_recovered(which, fraction, seed):
    g = pc.fixture_graph(fraction, seed)
    P, weight, pruned, component, iterations, cost, status = fixture_result(which, fraction, seed)
    assert status.tolist() == [0]
    assert np.nonzero(pruned)[0].tolist() == g['bad']                     # exactly the corrupted set
    dt, deg = pc.pose_errors(P, g['truth'])
    good = np.ones(len(weight), dtype=bool)
    good[g['bad']] = False
    print("%s %.2f/%d: %.3g m %.3g deg, iterations %s, good weights >= %.6f, bad weights <= %.3g"
          % (which, fraction, seed, dt, deg, iterations.tolist(), weight[good].min(), weight[~good].max()))
    assert dt < 1e-3 and deg < 0.01
    assert weight[good].min() > 0.99 and weight[~good].max() < 0.01
    assert np.array_equal(component, pc.components(g['N'], g['edges']))  # no component was split
    assert cost[0, 2] < cost[0, 1] < cost[0, 0]


@pytest.mark.parametrize("fraction,seed", CASES)
def test_host_twin_agrees_with_the_restatement_on_the_fixture(fraction, seed):
    a, b = fixture_result('host', fraction, seed), fixture_result('numpy', fraction, seed)
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert np.abs(a[0] - b[0]).max() < 1e-6
    assert np.abs(a[1] - b[1]).max() < 1e-6


@pytest.mark.parametrize("N", [1, 2, 3, 11, 23])
def test_host_twin_agrees_with_the_restatement_on_rings(N):
    """Rings hold reversed edges (j, i), j > i, and a duplicated edge."""
    g = pc.ring(N)
    a, b = host(g), restated(g)
    assert a[6].tolist() == b[6].tolist() == [0]
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert np.nonzero(a[2])[0].tolist() == g['bad']
    assert np.abs(a[0] - b[0]).max() < 1e-6
    dt, deg = pc.pose_errors(a[0], g['truth'])
    assert dt < 1e-6 and deg < 1e-4                                      # the rings' good edges are exact


def edge_host(Pi, Pj, Z, L):
    r, c, Ji, Jj = np.zeros(6), np.zeros(1), np.zeros((6, 6)), np.zeros((6, 6))
    p = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data
    Pi, Pj, Z, L = (np.ascontiguousarray(a, dtype=np.float64) for a in (Pi, Pj, Z, L))
    assert _native.lib().d3f_pose_graph_edge_host(Pi.ctypes.data, Pj.ctypes.data, Z.ctypes.data, L.ctypes.data,
                                                  r.ctypes.data, c.ctypes.data, Ji.ctypes.data, Jj.ctypes.data) == 0
    return r, float(c[0]), Ji, Jj


@pytest.mark.parametrize("at_identity", [True, False])
def test_jacobians_against_central_differences(at_identity):
    """d r / d d_i and d r / d d_j of d3f_pose_graph_edge_host against central differences of its own residual under
    P <- P Exp(d), at D = I (where the issue asks for exactness) and at a D of 0.3 m / 40 degrees (the Jacobians are
    exact there too).  Step 1e-6: the truncation error is ~1e-12 and the rounding error ~1e-16 / 1e-6 = 1e-10 times
    the size of the poses, so 1e-7 holds with room."""
    rng = np.random.default_rng(5)
    for trial in range(6):
        Pi, Pj = (pc.exp(rng.normal(0, 1, 3), rng.normal(0, 1, 3)) for _ in range(2))
        Z = np.linalg.inv(Pi) @ Pj
        if not at_identity:
            Z = Z @ pc.exp(rng.normal(0, 0.3, 3), rng.normal(0, 0.4, 3))
        L = pc.point_information(rng)
        r, c, Ji, Jj = edge_host(Pi, Pj, Z, L)
        if at_identity:
            assert np.abs(r).max() < 1e-12
        assert abs(c - r @ L @ r) <= 1e-12 * max(1.0, c)
        h = 1e-6
        for J, which in ((Ji, 0), (Jj, 1)):
            num = np.zeros((6, 6))
            for q in range(6):
                d = np.zeros(6)
                d[q] = h
                plus, minus = ([Pi, Pj] for _ in range(2))
                plus[which] = plus[which] @ pc.exp(d[:3], d[3:])
                minus[which] = minus[which] @ pc.exp(-d[:3], -d[3:])
                num[:, q] = (edge_host(plus[0], plus[1], Z, L)[0] - edge_host(minus[0], minus[1], Z, L)[0]) / (2 * h)
            assert np.abs(J - num).max() < 1e-7, (which, trial)
        rn, cn, Jin, Jjn = reg.pose_graph_edge_numpy(Pi, Pj, Z, L)
        assert np.abs(r - rn).max() < 1e-12 and np.abs(Ji - Jin).max() < 1e-12 and np.abs(Jj - Jjn).max() < 1e-12


def small(poses0, edges, Z, info, unc):
    return dict(N=len(poses0), poses0=np.asarray(poses0, dtype=np.float64), edges=np.asarray(edges).reshape(-1, 2),
                Z=np.asarray(Z, dtype=np.float64).reshape(-1, 4, 4),
                info=np.asarray(info, dtype=np.float64).reshape(-1, 6, 6), unc=np.asarray(unc, dtype=bool))


@pytest.mark.parametrize("run", [host, restated])
def test_one_node_and_two_nodes(run):
    rng = np.random.default_rng(2)
    P0 = pc.exp([1, 2, 3], [0.1, 0.2, 0.3])
    out = run(small([P0], [], [], [], []))
    assert np.array_equal(out[0][0], P0) and out[3].tolist() == [0] and out[6].tolist() == [0]
    assert out[4].tolist() == [[0, 0]]
    Z = pc.exp([0.5, -1, 0.25], [0.3, -0.2, 0.9])
    for unc in (False, True):
        out = run(small([P0, np.eye(4)], [(0, 1)], [Z], [pc.point_information(rng)], [unc]))
        assert np.array_equal(out[0][0], P0)
        assert np.abs(out[0][1] - P0 @ Z).max() < 1e-9
        assert out[2].tolist() == [0] and out[3].tolist() == [0, 0] and out[6].tolist() == [0]
        out = run(small([P0, np.eye(4)], [(1, 0)], [Z], [pc.point_information(rng)], [unc]))   # the edge reversed
        assert np.abs(out[0][1] - P0 @ np.linalg.inv(Z)).max() < 1e-9


@pytest.mark.parametrize("run", [host, restated])
def test_isolated_node_and_zero_information_edge(run):
    """Node 3 has no edge; the only edge between {0, 1} and {2, 4} has no correspondences: it is reported pruned and
    the components stay apart, each with its lowest node fixed."""
    rng = np.random.default_rng(3)
    truth = np.stack([pc.exp(rng.normal(0, 1, 3), rng.normal(0, 0.5, 3)) for _ in range(5)])
    edges = [(0, 1), (2, 4), (1, 2), (1, 4)]
    Z = [np.linalg.inv(truth[i]) @ truth[j] for i, j in edges]
    info = [pc.point_information(rng), pc.point_information(rng), np.zeros((6, 6)), np.full((6, 6), np.nan)]
    P0 = truth.copy()
    for k in (1, 3, 4):
        P0[k] = P0[k] @ pc.exp(rng.normal(0, 0.05, 3), rng.normal(0, 0.05, 3))
    P, weight, pruned, component, iterations, cost, status = run(small(P0, edges, Z, info, [False, True, True, False]))
    assert status.tolist() == [0]
    assert pruned.tolist() == [0, 0, 1, 1] and weight[2:].tolist() == [0.0, 0.0]
    assert component.tolist() == [0, 0, 2, 3, 2]
    for k in (0, 2, 3):
        assert np.array_equal(P[k], P0[k])                               # the fixed nodes and the isolated one: bit-equal
    assert np.abs(P[1] - truth[1]).max() < 1e-8 and np.abs(P[4] - truth[4]).max() < 1e-8


@pytest.mark.parametrize("run", [host, restated])
def test_nonfinite_input_and_bad_edges_set_the_status(run):
    g = pc.ring(11)
    for what, want in (('Z', reg.PG_ST_NONFINITE), ('poses0', reg.PG_ST_NONFINITE)):
        bad = dict(g)
        bad[what] = g[what].copy()
        bad[what][3, 1, 2] = np.inf
        out = run(bad)
        assert out[6].tolist() == [want]
        assert np.array_equal(out[0], bad['poses0'], equal_nan=True) and out[4].tolist() == [[0, 0]]
    assert ops.PG_ST_NONFINITE == reg.PG_ST_NONFINITE and ops.PG_ST_GRAPH == reg.PG_ST_GRAPH


def test_host_twin_rejects_bad_edge_lists_and_arguments():
    """Host edge lists are checked by the wrapper; the kernel text's own check (device-side edge lists) is reached
    through the C entry.  Beyond the node cap: D3F_EINVAL; a workspace that is too small: D3F_EWORKSPACE."""
    g = pc.ring(6)
    for edges in ([(0, 6)], [(2, 2)], [(-1, 3)]):
        with pytest.raises(ValueError):
            ops.pose_graph_optimize_host(g['poses0'], edges, g['Z'][:1], g['info'][:1], [True], pc.MAX_DISTANCE)
    L = _native.lib()
    N, E = 6, len(g['edges'])
    ns, es = np.array([0, N], dtype=np.int32), np.array([0, E], dtype=np.int32)
    edges = g['edges'].astype(np.int32).copy()
    edges[2] = (1, 7)
    un = g['unc'].astype(np.int32)
    out = np.zeros((N, 4, 4))
    w, pr, comp = np.zeros(E), np.zeros(E, dtype=np.int32), np.zeros(N, dtype=np.int32)
    it, cost, st = np.zeros(2, dtype=np.int32), np.zeros(3), np.zeros(1, dtype=np.int32)
    nbytes = L.d3f_pose_graph_optimize_ws_bytes(1, N, E)
    ws = np.zeros(nbytes, dtype=np.uint8)
    p = lambda a: a.ctypes.data

    def call(max_nodes=N, nbytes=nbytes):
        return L.d3f_pose_graph_optimize_host(p(ns), p(es), 1, N, E, max_nodes, E, p(g['poses0']), p(edges), p(g['Z']),
                                              p(g['info']), p(un), 0.05, 2.0, 0.25, 100, 1e-9, 1e-9, p(out), p(w),
                                              p(pr), p(comp), p(it), p(cost), p(st), p(ws), nbytes, None)
    assert call() == 0 and st.tolist() == [ops.PG_ST_GRAPH] and np.array_equal(out, g['poses0'])
    assert call(max_nodes=5) == 0 and st.tolist() == [ops.PG_ST_GRAPH]   # a graph beyond the stated bound
    assert call(max_nodes=ops.PG_MAX_NODES + 1) == -1
    assert call(nbytes=nbytes - 256) == -2
    assert L.d3f_pose_graph_optimize_ws_bytes(1, ops.PG_MAX_NODES + 1, 10) == 0
    assert L.d3f_pose_graph_optimize_ws_bytes(2, 128, 500) >= 2 * 2 * 768 * 768 * 8
    with pytest.raises(ValueError):
        ops.pose_graph_optimize_host(np.tile(np.eye(4), (129, 1, 1)), [], np.zeros((0, 4, 4)), np.zeros((0, 6, 6)), [],
                                     pc.MAX_DISTANCE)


@pytest.mark.parametrize("run", [host, restated])
def test_duplicated_edge_counts_twice(run):
    """A certain edge listed twice equals the same edge with its information doubled (with certain edges only, so that
    mu -- a mean over the edges -- plays no part).  The measurements disagree, so the information matters.  Doubling is
    exact in floating point, so the two differ only by the order of a few sums: 1e-11 on poses of size 1."""
    rng = np.random.default_rng(4)
    truth = np.stack([pc.exp(rng.normal(0, 1, 3), rng.normal(0, 0.5, 3)) for _ in range(5)])
    edges = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 0), (1, 3)]
    Z = [np.linalg.inv(truth[i]) @ truth[j] @ pc.exp(rng.normal(0, 0.02, 3), rng.normal(0, 0.02, 3)) for i, j in edges]
    info = [pc.point_information(rng) for _ in edges]
    tight = dict(step_tol=1e-13, rel_cost=1e-15)     # the default rules stop within ~1e-9 of the minimum; go on to rounding
    twice = run(small(truth, edges + [edges[5]], Z + [Z[5]], info + [info[5]], [False] * 7), **tight)
    doubled = run(small(truth, edges, Z, info[:5] + [2 * info[5]], [False] * 6), **tight)
    once = run(small(truth, edges, Z, info, [False] * 6), **tight)
    assert np.abs(twice[0] - doubled[0]).max() < 1e-11
    assert np.abs(twice[0] - once[0]).max() > 1e-5


def test_reversed_edges_reach_the_same_poses():
    """The edge (i, j, Z) given as (j, i, inv(Z)).  Its residual is r' = -Ad(Z) r only to FIRST order in r (the
    translation part of [D_t ; log D_R] is not a group logarithm), so moving the information to the other frame,
    L' = Ad(Z)^-T L Ad(Z)^-1, gives the same cost to second order, not exactly: where the measurements are consistent
    both forms have the same minimum, and that is what is asked here; rings with reversed edges are compared with the
    restatement above, which treats every edge alike."""
    g = pc.ring(11, corrupt=False)
    flipped = dict(g)
    flipped['edges'] = g['edges'][:, ::-1].copy()
    flipped['Z'] = np.stack([np.linalg.inv(z) for z in g['Z']])
    info = []
    for z, L in zip(g['Z'], g['info']):
        Ad = np.zeros((6, 6))
        Ad[:3, :3] = Ad[3:, 3:] = z[:3, :3]
        t = z[:3, 3]
        Ad[:3, 3:] = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ z[:3, :3]
        Ai = np.linalg.inv(Ad)
        info.append(Ai.T @ L @ Ai)
    flipped['info'] = np.stack(info)
    a, b = host(g), host(flipped)
    assert a[6].tolist() == b[6].tolist() == [0] and not a[2].any() and not b[2].any()
    assert np.abs(a[0] - g['truth']).max() < 1e-8 and np.abs(b[0] - g['truth']).max() < 1e-8


@pytest.mark.parametrize("run", [host, restated])
def test_pruning_that_splits_a_component(run):
    """Two chains joined by two loop closures that are slightly off, with ``prune_threshold=1``: every uncertain edge
    with a residual is pruned after the first pass (the strain reaches the closures inside the chains too), the graph
    falls into two components and each keeps its lowest node fixed in the second pass.  (Gross errors do not serve here: a
    chain that hangs on contradicting closures alone can always satisfy one of them, and the line process finds it.)"""
    rng = np.random.default_rng(6)
    truth = np.stack([pc.exp(rng.normal(0, 1, 3), rng.normal(0, 0.5, 3)) for _ in range(8)])
    edges = [(0, 1), (1, 2), (2, 3), (4, 5), (5, 6), (6, 7), (1, 5), (2, 6), (0, 2), (4, 6)]
    Z = [np.linalg.inv(truth[i]) @ truth[j] for i, j in edges]
    Z[6] = Z[6] @ pc.exp([0.01, -0.005, 0.008], [0.01, 0.002, -0.005])
    Z[7] = Z[7] @ pc.exp([-0.006, 0.009, -0.004], [-0.004, 0.008, 0.003])
    info = [pc.point_information(rng) for _ in edges]
    unc = [False] * 6 + [True] * 4
    P0 = truth.copy()
    for k in range(1, 8):
        P0[k] = P0[k] @ pc.exp(rng.normal(0, 0.02, 3), rng.normal(0, 0.02, 3))
    P, weight, pruned, component, iterations, cost, status = run(small(P0, edges, Z, info, unc), prune_threshold=1.0)
    assert status.tolist() == [0]
    assert np.nonzero(pruned)[0].tolist() == [6, 7, 8, 9] and (weight[6:] < 1.0).all() and (weight[:6] == 1.0).all()
    assert component.tolist() == [0, 0, 0, 0, 4, 4, 4, 4]
    assert np.array_equal(P[0], P0[0])
    assert iterations[0, 1] >= 1 and cost[0, 2] < 1e-12 < cost[0, 1]
    for i, j in edges[:6] + edges[8:]:                                   # what is left is consistent: the truth
        assert np.abs(np.linalg.inv(P[i]) @ P[j] - np.linalg.inv(truth[i]) @ truth[j]).max() < 1e-7


def test_gauge():
    """Fixed nodes come back bit-equal; moving a component's initial poses by a rigid motion moves its result by the
    same motion (the residuals hold only inv(P_i) P_j), to 1e-9."""
    g = pc.fixture_graph(0.15, 0)
    a = fixture_result('host', 0.15, 0)
    comp = pc.components(g['N'], g['edges'])
    roots = sorted(set(comp.tolist()))
    assert len(roots) == 4
    for k in roots:
        assert np.array_equal(a[0][k], g['poses0'][k])
    rng = np.random.default_rng(9)
    moved = dict(g)
    moved['poses0'] = g['poses0'].copy()
    motion = {k: pc.exp(rng.normal(0, 2, 3), rng.normal(0, 1, 3)) for k in roots}
    for k in range(g['N']):
        moved['poses0'][k] = motion[comp[k]] @ g['poses0'][k]
    b = host(moved)
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    for k in range(g['N']):
        assert np.abs(b[0][k] - motion[comp[k]] @ a[0][k]).max() < 1e-9
    for k in roots:
        assert np.array_equal(b[0][k], moved['poses0'][k])


def test_spanning_tree_poses_reproduce_the_file():
    """Every pair pose of the uncorrupted file is met by the spanning-tree poses to the file's own precision; the tree
    takes certain edges first; tensors and arrays give the same poses."""
    N, edges, T, info, unc, truth = pc.fixture()
    parent, via, depth, root = reg.spanning_tree(N, edges, unc)
    assert np.array_equal(root, pc.components(N, edges))
    worst = max(np.abs(np.linalg.inv(truth[i]) @ truth[j] - T[e]).max() for e, (i, j) in enumerate(edges))
    print("largest entry of inv(P_i) P_j - T_ij: %.3g" % worst)
    assert worst < 2e-5
    for k in np.nonzero(root == np.arange(N))[0]:
        assert np.array_equal(truth[k], np.eye(4))
    # the tree holds as few uncertain edges as the graph allows
    certain_only = len(set(pc.components(N, edges, np.nonzero(unc)[0]).tolist()))
    assert int(unc[via[parent >= 0]].sum()) == certain_only - len(set(root.tolist()))
    keys = ['%d_%d' % (i, j) for i, j in edges]
    as_tensor = reg.spanning_tree_poses(N, keys, torch.from_numpy(T), unc)
    assert isinstance(as_tensor, torch.Tensor) and np.abs(as_tensor.numpy() - truth).max() < 1e-12


def test_multiway_registration_on_the_cpu():
    N, edges, T, info, unc, truth = pc.fixture()
    Z, P0, bad = pc.corrupted(0.15, 1)
    keys = ['%d_%d' % (i, j) for i, j in edges]
    poses, kept, weight, component, status = reg.multiway_registration(keys, Z, info, N, pc.MAX_DISTANCE, device='cpu')
    assert status.tolist() == [0]
    assert np.nonzero(~kept)[0].tolist() == bad                          # uncertain = j - i > 1, start = spanning tree
    dt, deg = pc.pose_errors(poses, truth)
    assert dt < 1e-3 and deg < 0.01
    assert np.array_equal(component, pc.components(N, edges))
    again = reg.multiway_registration(edges, Z, info, N, pc.MAX_DISTANCE, uncertain=unc, init=P0, device='cpu',
                                      max_iters=50)
    assert np.nonzero(~again[1])[0].tolist() == bad and np.abs(again[0] - poses).max() < 1e-6
