"""GPU: the pose-graph kernel (ops.pose_graph_optimize, csrc/posegraph.hip: one workgroup per graph) against its host
twin -- the same text run by one worker -- on the corrupted benchmark scene and on rings whose 6 N crosses 64, 256, the
workgroup's 512 threads and the 768 rows of the cap; batch independence, determinism, graph capture; and the front end:
multiway_registration over pair poses that refine_transforms made, register_scene(pose_graph=...).

Device and host run the same operations in the same order and differ only where the device's sin / cos / atan2 / sqrt
differ from the host's in the last place, so poses are asked to agree to 1e-6 (the bound tests/test_icp_gpu.py sets
between device and NumPy), pruned sets and components exactly."""
import os

import numpy as np
import pytest
import torch

import icp_scene as sc
import posegraph_cases as pc
from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.geometric_registration import evaluate as ev
from d3feat_pytorch_amd.geometric_registration import registration as reg


def device(g, **kw):
    out = ops.pose_graph_optimize(torch.from_numpy(g['poses0']).cuda(), g['edges'], g['Z'], g['info'], g['unc'],
                                  pc.MAX_DISTANCE, **kw)
    return [t.cpu().numpy() for t in out]


def host(g, **kw):
    out = ops.pose_graph_optimize_host(g['poses0'], g['edges'], g['Z'], g['info'], g['unc'], pc.MAX_DISTANCE, **kw)
    return [t.numpy() for t in out]


def check_against_host(g):
    a, b = device(g), host(g)
    assert a[6].tolist() == b[6].tolist() == [0]
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert np.nonzero(a[2])[0].tolist() == g['bad']
    assert np.abs(a[0] - b[0]).max() < 1e-6
    assert np.abs(a[1] - b[1]).max(initial=0.0) < 1e-6                    # (no edge at N = 1)
    assert np.abs(a[5] - b[5]).max() <= 1e-6 * max(1.0, np.abs(b[5]).max())
    for k in sorted(set(a[3].tolist())):
        assert np.array_equal(a[0][k], g['poses0'][k])                    # the gauge nodes: bit-equal
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("fraction,seed", [(0.15, 0), (0.30, 1)])
def test_device_equals_host_twin_on_the_fixture(fraction, seed):
    g = pc.fixture_graph(fraction, seed)
    a = check_against_host(g)
    dt, deg = pc.pose_errors(a[0], g['truth'])
    assert dt < 1e-3 and deg < 0.01


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 2, 3, 11, 43, 64, 65, 128])
def test_device_equals_host_twin_on_rings(N):
    g = pc.ring(N)
    a = check_against_host(g)
    dt, deg = pc.pose_errors(a[0], g['truth'])
    assert dt < 1e-6 and deg < 1e-4


@pytest.mark.gpu
def test_batch_is_bit_identical_to_each_graph_alone_and_from_run_to_run():
    rng = np.random.default_rng(1)
    two = dict(N=2, edges=np.array([[0, 1]]), Z=pc.exp([0.5, -1, 0.25], [0.3, -0.2, 0.9])[None],
               info=pc.point_information(rng)[None], unc=np.array([True]), poses0=np.tile(np.eye(4), (2, 1, 1)),
               bad=[])
    graphs = [pc.fixture_graph(0.15, 0), two, pc.ring(12)]
    assert graphs[2]['bad']
    P0, edges, Z, info, unc, ns, es = pc.stack(graphs)
    runs = [ops.pose_graph_optimize(torch.from_numpy(P0).cuda(), edges, Z, info, unc, pc.MAX_DISTANCE, node_start=ns,
                                    edge_start=es) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    batch = [t.cpu().numpy() for t in runs[0]]
    assert batch[6].tolist() == [0, 0, 0]
    for n, g in enumerate(graphs):
        alone = device(g)
        nodes, eds = slice(ns[n], ns[n + 1]), slice(es[n], es[n + 1])
        assert np.array_equal(batch[0][nodes], alone[0]) and np.array_equal(batch[1][eds], alone[1])
        assert np.array_equal(batch[2][eds], alone[2]) and np.array_equal(batch[3][nodes], alone[3])
        assert np.array_equal(batch[4][n], alone[4][0]) and np.array_equal(batch[5][n], alone[5][0])
        assert np.nonzero(alone[2])[0].tolist() == g['bad']
    # stacked the other way round: the same again
    P0r, edgesr, Zr, infor, uncr, nsr, esr = pc.stack(graphs[::-1])
    rev = [t.cpu().numpy() for t in ops.pose_graph_optimize(torch.from_numpy(P0r).cuda(), edgesr, Zr, infor, uncr,
                                                            pc.MAX_DISTANCE, node_start=nsr, edge_start=esr)]
    assert np.array_equal(rev[0][nsr[2]:nsr[3]], batch[0][ns[0]:ns[1]])
    assert np.array_equal(rev[1][esr[0]:esr[1]], batch[1][es[2]:es[3]])


@pytest.mark.gpu
def test_graph_capture_replays_bit_identically():
    g = pc.fixture_graph(0.30, 0)
    N, E = g['N'], len(g['edges'])
    dev = torch.device('cuda')
    P0 = torch.from_numpy(g['poses0']).to(dev)
    args = (torch.from_numpy(g['edges'].astype(np.int32)).to(dev), torch.from_numpy(g['Z']).to(dev),
            torch.from_numpy(g['info']).to(dev), torch.from_numpy(g['unc'].astype(np.int32)).to(dev), pc.MAX_DISTANCE)
    kw = dict(node_start=torch.tensor([0, N], dtype=torch.int32, device=dev),
              edge_start=torch.tensor([0, E], dtype=torch.int32, device=dev), max_nodes=N, max_edges=E)
    ops.pose_graph_optimize(P0, *args, **kw)                              # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = ops.pose_graph_optimize(P0, *args, **kw)
    P0.copy_(torch.from_numpy(pc.fixture_graph(0.30, 1)['poses0']).to(dev))   # other initial poses, same edges
    graph.replay()
    torch.cuda.synchronize()
    want = ops.pose_graph_optimize(P0, *args, **kw)
    for a, b in zip(outs, want):
        assert torch.equal(a, b)
    assert np.nonzero(outs[2].cpu().numpy())[0].tolist() == g['bad']
    first = [t.clone() for t in outs]
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, first):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_device_edge_lists_are_checked_by_the_kernel():
    g = pc.ring(11)
    edges = g['edges'].astype(np.int32).copy()
    edges[4] = (3, 11)
    dev = torch.device('cuda')
    out = ops.pose_graph_optimize(torch.from_numpy(g['poses0']).to(dev), torch.from_numpy(edges).to(dev), g['Z'],
                                  g['info'], g['unc'], pc.MAX_DISTANCE)
    assert out[6].tolist() == [ops.PG_ST_GRAPH] and np.array_equal(out[0].cpu().numpy(), g['poses0'])
    bad = g['Z'].copy()
    bad[2, 0, 3] = np.nan
    out = ops.pose_graph_optimize(torch.from_numpy(g['poses0']).to(dev), g['edges'], bad, g['info'], g['unc'],
                                  pc.MAX_DISTANCE)
    assert out[6].tolist() == [ops.PG_ST_NONFINITE] and np.array_equal(out[0].cpu().numpy(), g['poses0'])
    assert out[4].cpu().tolist() == [[0, 0]]


NUM_FRAG, ICP_DISTANCE = 7, 0.05


@pytest.fixture(scope="module")
def refined_scene():
    """Seven fragments of about 2000 points of one room, every pair of them overlapping; pair poses from
    refine_transforms started 1 degree / 1 cm from the truth, with their information matrices."""
    clouds, poses = sc.make_scene(11, NUM_FRAG, n=6500)
    pairs = [(i, j) for i in range(NUM_FRAG) for j in range(i + 1, NUM_FRAG)]
    rng = np.random.default_rng(3)
    gt = np.stack([sc.gt_transform(poses, i, j) for i, j in pairs])
    T0 = np.stack([G @ sc.perturbation(rng, 1.0, 0.01) for G in gt])
    T, fitness, rmse, iters, info = reg.refine_transforms(clouds, pairs, T0, ICP_DISTANCE, return_information=True)
    return clouds, pairs, gt, T, info


@pytest.mark.gpu
def test_multiway_registration_prunes_the_false_loop_closure(refined_scene):
    clouds, pairs, gt, T, info = refined_scene
    assert 1800 < np.mean([len(c) for c in clouds]) < 2400
    infos = info.cpu().numpy()
    refined = [reg.transformation_error(t, g, L) for t, g, L in zip(T.cpu().numpy(), gt, infos)]
    loops = [n for n, (i, j) in enumerate(pairs) if j - i > 1]
    bad = loops[1]
    Tb = T.clone()
    Tb[bad] = Tb[bad] @ torch.from_numpy(sc.perturbation(np.random.default_rng(4), 35, 0.5)).cuda()
    poses, kept, weight, component, status = reg.multiway_registration(pairs, Tb, info, NUM_FRAG, ICP_DISTANCE)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in (poses, kept, weight, component, status))
    assert status.tolist() == [0] and component.tolist() == [0] * NUM_FRAG
    assert np.nonzero(~kept.cpu().numpy())[0].tolist() == [bad]           # that pair and no other
    P = poses.cpu().numpy()
    after = [reg.transformation_error(np.linalg.inv(P[i]) @ P[j], gt[n], infos[n]) for n, (i, j) in enumerate(pairs)]
    print("transformation_error: refined pairs <= %.3g, pose graph <= %.3g (the pruned pair %.3g)"
          % (max(refined), max(after[n] for n in range(len(pairs)) if n != bad), after[bad]))
    assert max(after[n] for n in range(len(pairs)) if n != bad) <= max(refined)
    cpu = reg.multiway_registration(pairs, Tb.cpu().numpy(), infos, NUM_FRAG, ICP_DISTANCE, device='cpu')
    assert np.array_equal(cpu[1], kept.cpu().numpy()) and np.abs(cpu[0] - P).max() < 1e-6


@pytest.mark.gpu
def test_register_scene_with_a_pose_graph(tmp_path, monkeypatch):
    """register_scene(pose_graph=...) writes inv(P_i) P_j of the pairs multiway_registration kept and leaves the pruned
    ones out; without pose_graph it writes every pair as it did, and the file is what evaluate.writelog makes of them.
    The scene is that of test_icp_gpu's register_scene test; RANSAC's answer for the pair 1_4 is replaced by a gross
    error on its way out, the false loop closure a low overlap produces."""
    num_frag, scene_name, save = 6, 'surface-room', str(tmp_path / 'dump')
    clouds, poses, world, ids = sc.make_scene(3, num_frag, return_world=True)
    rng = np.random.default_rng(9)
    desc = sc.position_descriptors(rng, world, ids)
    score = [rng.permutation(len(c)).astype(np.float32)[:, None] / len(c) for c in clouds]
    gt = {'%d_%d' % (i, j): sc.gt_transform(poses, i, j) for i in range(num_frag) for j in range(i + 1, num_frag)}
    dpath, kpath, spath = ev._paths(save, scene_name)
    for p in (dpath, kpath, spath):
        os.makedirs(p)
    for f in range(num_frag):
        np.save(os.path.join(dpath, 'cloud_bin_%d.D3Feat' % f), desc[f])
        np.save(os.path.join(kpath, 'cloud_bin_%d' % f), clouds[f])
        np.save(os.path.join(spath, 'cloud_bin_%d' % f), score[f])
    gtdir = str(tmp_path / 'gt')
    ev.writelog(gtdir, gt, num_frag)
    written = []
    real_writelog = ev.writelog

    def spy(path, transforms, n):
        written.append({k: np.array(v) for k, v in transforms.items()})
        return real_writelog(path, transforms, n)
    monkeypatch.setattr(ev, 'writelog', spy)
    keys = sorted(gt, key=lambda k: tuple(int(x) for x in k.split('_')))
    false_key = '1_4'
    real_ransac = reg._ransac

    def spoiled(src, tgt, seg, params):
        out = list(real_ransac(src, tgt, seg, params))
        n = keys.index(false_key)
        out[0][n] = out[0][n] @ torch.from_numpy(sc.perturbation(np.random.default_rng(4), 40, 0.6)).to(out[0].device)
        return tuple(out)
    monkeypatch.setattr(reg, '_ransac', spoiled)
    kw = dict(num_points=1000, num_hypotheses=20000, distance_threshold=0.05, seed=0, icp=dict(max_distance=0.04))
    assert reg.register_scene(save, scene_name, gtdir, out_log=str(tmp_path / 'plain'), **kw) is None
    assert reg.register_scene(save, scene_name, gtdir, out_log=str(tmp_path / 'none'), pose_graph=None, **kw) is None
    result, P = reg.register_scene(save, scene_name, gtdir, out_log=str(tmp_path / 'graph'),
                                   pose_graph=dict(max_distance=0.04), **kw)
    plain, none, graph = written
    assert sorted(plain) == sorted(keys) and result is None and P.shape == (num_frag, 4, 4)
    read = lambda name: open(os.path.join(str(tmp_path / name), 'gt.log'), 'rb').read()
    real_writelog(str(tmp_path / 'again'), plain, num_frag)
    assert read('plain') == read('none') == read('again')
    # the same steps by hand: the pairs register_scene estimated, their information, the pose graph
    T = np.stack([plain[k] for k in keys])
    info = reg.information_matrices(clouds, keys, T, 0.04)[0]
    want_P, kept = (t.cpu().numpy() for t in reg.multiway_registration(keys, T, info, num_frag, 0.04)[:2])
    print("pruned pairs: %s" % [k for k, m in zip(keys, kept) if not m])
    assert sorted(graph) == sorted(k for k, m in zip(keys, kept) if m)
    assert false_key in plain and false_key not in graph and len(graph) >= len(keys) - 3
    assert np.abs(P - want_P).max() < 1e-9
    log = ev.loadlog(str(tmp_path / 'graph'))
    assert sorted(log) == sorted(graph)
    for key in graph:
        i, j = (int(x) for x in key.split('_'))
        assert np.abs(graph[key] - np.linalg.inv(P[i]) @ P[j]).max() < 1e-9
