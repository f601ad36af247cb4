"""GPU: ops.iss_saliency / ops.radius_nms / ops.iss_keypoints (csrc/iss.hip) against brute-force integers, the host twins
and the NumPy restatement bit for bit; the edge cases; independence of order, stacking, cell size and repetition; graph
capture; and the front ends (detect_iss, keypoint_repeatability, the FPFH + ISS dump and repeatability_scene) against
their device='cpu' forms."""
import os

import numpy as np
import pytest
import torch

from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.geometric_registration import evaluate as ev
from d3feat_pytorch_amd.geometric_registration import registration as reg
import fpfh_cases as fc
import iss_cases as ic

Q = reg.normals_scale(ic.R_SALIENT)
ST_CELL_RANGE = 2


def grid_of(clouds, radius, lens=None):
    pts = torch.from_numpy(np.concatenate(clouds)).cuda()
    return ops.CloudGrid(pts, [len(c) for c in clouds] if lens is None else lens, radius)


def saliency_of(clouds, grid_radius=None, **kw):
    grid = grid_of(clouds, ic.R_SALIENT if grid_radius is None else grid_radius)
    out = ops.iss_saliency(grid, None, ic.R_SALIENT, return_moments=True, **kw)
    assert int(grid.status.word.item()) == 0
    return out


def nms_of(clouds, score, radius=ic.R_NMS, min_neighbors=ic.MIN_NEIGHBORS, grid_radius=None, lens=None):
    grid = grid_of(clouds, radius if grid_radius is None else grid_radius, lens)
    score = score if isinstance(score, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(score)).cuda()
    out = ops.radius_nms(grid, None, radius, score, min_neighbors)
    assert int(grid.status.word.item()) == 0
    return out


def host(ts):
    return tuple(t.cpu().numpy() for t in ts)


@pytest.fixture(scope="module")
def device_run():
    """The fixture's fragments through both passes on the device, once."""
    clouds = ic.fixture()[0]
    saliency, count, moments = saliency_of(clouds)
    keep, count_nms = nms_of(clouds, saliency)
    torch.cuda.synchronize()
    return clouds, saliency, count, moments, keep, count_nms


@pytest.mark.gpu
def test_saliency_moments_are_exact_and_the_solve_is_the_host_twins(device_run):
    clouds, saliency, count, moments, _, _ = device_run
    _, want_m, want_s, _, _ = ic.fixture()
    saliency, count, moments = host((saliency, count, moments))
    assert saliency.dtype == np.float32 and count.dtype == np.int32 and moments.dtype == np.int64
    assert np.array_equal(moments, want_m) and np.array_equal(count, want_m[:, 0])
    # the same inline text on both sides, -ffp-contract=off on both: equal bits
    twin = ops.iss_saliency_from_moments_host(moments, Q, ic.G21, ic.G32, ic.MIN_NEIGHBORS).numpy()
    differ = np.nonzero(saliency != twin)[0]
    print("%d rows, device != host twin on %d" % (len(twin), len(differ)))
    assert np.array_equal(saliency, twin)
    # against eigvalsh as on the CPU
    near = ic.near_threshold(moments, Q)
    worst = int(ic.ulps(saliency[~near], want_s[~near]).max())
    print("%d rows within %.0e of a threshold, worst %d ulp against eigvalsh" % (near.sum(), ic.GAP, worst))
    assert near.mean() <= 0.01 and np.array_equal(saliency[~near] > 0, want_s[~near] > 0) and worst <= ic.MAX_ULP
    # the keywords reach the kernel
    open_gate = host(saliency_of(clouds, gamma_21=1.0, gamma_32=1.0, min_neighbors=1))[0]
    assert np.array_equal(open_gate, ops.iss_saliency_from_moments_host(moments, Q, 1.0, 1.0, 1).numpy())
    assert (open_gate > 0).sum() > (saliency > 0).sum()
    few = host(saliency_of(clouds, min_neighbors=40))[0]
    assert np.array_equal(few > 0, (saliency > 0) & (count >= 40)) and 0 < (few > 0).sum() < (saliency > 0).sum()


@pytest.mark.gpu
def test_nms_of_the_devices_saliency_equals_restatement_and_host_twin(device_run):
    clouds, saliency, _, _, keep, count = device_run
    sal = saliency.cpu().numpy()
    keep, count = host((keep, count))
    assert keep.dtype == np.bool_ and count.dtype == np.int32
    want = reg.radius_nms_numpy(list(clouds), sal, ic.R_NMS, ic.MIN_NEIGHBORS)
    twin = host(ops.radius_nms_host(np.concatenate(clouds), [len(c) for c in clouds], ic.R_NMS, sal, ic.MIN_NEIGHBORS))
    assert np.array_equal(keep, want[0]) and np.array_equal(count, want[1])
    assert np.array_equal(keep, twin[0]) and np.array_equal(count, twin[1])
    na = len(clouds[0])
    assert (int(keep[:na].sum()), int(keep[na:].sum())) == (74, 72)
    # [N,1] scores; a score positive on a single row: its count is right, every other row is 0
    assert torch.equal(nms_of(clouds, saliency.view(-1, 1))[0].cpu(), torch.from_numpy(keep))
    row = na + 17
    single = np.zeros(len(sal), dtype=np.float32)
    single[row] = 3.0
    k1, c1 = host(nms_of(clouds, single, min_neighbors=1))
    assert k1.sum() == 1 and k1[row] and c1[row] == ic.brute_nms(clouds[1], single[na:], ic.R_NMS)[1][17] > 1
    assert np.count_nonzero(c1) == 1


@pytest.mark.gpu
def test_hand_written_scores_and_a_crowded_cell(device_run):
    p, s, radius, want = ic.hand_case()
    for mn, (keep, count) in want.items():
        k, c = host(nms_of([p], s, radius, mn))
        assert np.array_equal(k, keep) and np.array_equal(c, count)
    # a cell holding more than 64 points, one point 100 times over with equal scores: kept together or beaten together
    a = ic.fixture()[0][0][:600]
    dense = np.concatenate([a, np.repeat(a[7:8], 100, 0)])
    for top in (5.0, 0.5):
        score = np.concatenate([np.linspace(1.0, 2.0, 600, dtype=np.float32), np.full(100, top, dtype=np.float32)])
        score[7] = top
        k, c = host(nms_of([dense], score, 0.1, 1))
        bk, bc = ic.brute_nms(dense, score, 0.1, 1)
        assert np.array_equal(k, bk) and np.array_equal(c, bc) and c[7] >= 101
        assert k[600:].all() == (top == 5.0) and k[600:].any() == (top == 5.0) and k[7] == k[600]
    # and through the saliency pass: the copies share the moments of the point they repeat
    sal, cnt, m = host(saliency_of([dense]))
    assert np.array_equal(m, ic.brute_moments(dense, ic.R_SALIENT))
    assert np.array_equal(sal[600:], np.repeat(sal[7:8], 100)) and np.array_equal(m[600:], np.repeat(m[7:8], 100, 0))
    copies = np.repeat(np.float32([[0.25, 0.5, -1.0]]), 100, 0)
    sal, cnt, m = host(saliency_of([copies]))
    assert (sal == 0).all() and (cnt == 100).all() and (m[:, 1:] == 0).all()
    rng = np.random.default_rng(31)
    plane = np.concatenate([rng.uniform(-1, 1, size=(1500, 2)), np.full((1500, 1), 0.5)], 1).astype(np.float32)
    sal, cnt, _ = host(saliency_of([plane]))
    assert (cnt >= 5).all() and (sal == 0).all()


@pytest.mark.gpu
def test_edge_cases(device_run):
    clouds = device_run[0]
    one = np.float32([[0.5, -0.25, 1.0]])
    # B = 1 with N = 1
    sal, cnt, m = host(saliency_of([one], min_neighbors=1))
    assert sal.tolist() == [0.0] and cnt.tolist() == [1] and m[0].tolist() == [1] + [0] * 9
    k, c = host(nms_of([one], np.float32([1.0]), min_neighbors=1))
    assert k.tolist() == [True] and c.tolist() == [1]
    k, c = host(nms_of([one], np.float32([1.0]), min_neighbors=2))
    assert k.tolist() == [False] and c.tolist() == [1]
    # a cloud of length 0 between two others
    a, b = clouds[0][:700], clouds[1][:600]
    empty = np.zeros((0, 3), dtype=np.float32)
    got = host(saliency_of([a, empty, b]))
    alone = [host(saliency_of([x])) for x in (a, b)]
    for g, x, y in zip(got, alone[0], alone[1]):
        assert np.array_equal(g, np.concatenate([x, y]))
    score = np.concatenate([alone[0][0], alone[1][0]])
    k, c = host(nms_of([a, empty, b], score))
    for lo, x, s in ((0, a, score[:700]), (700, b, score[700:])):
        bk, bc = ic.brute_nms(x, s, ic.R_NMS, ic.MIN_NEIGHBORS)
        assert np.array_equal(k[lo:lo + len(x)], bk) and np.array_equal(c[lo:lo + len(x)], bc)
    # lens that sum to fewer rows than N: the tail is 0
    grid = grid_of([a, b], ic.R_SALIENT, lens=[700, 100])
    sal, cnt, m = host(ops.iss_saliency(grid, None, ic.R_SALIENT, return_moments=True))
    assert np.array_equal(sal[:700], alone[0][0]) and not sal[800:].any() and not cnt[800:].any() and not m[800:].any()
    assert np.array_equal(m[700:800], ic.brute_moments(b[:100], ic.R_SALIENT))
    ones = torch.ones(1300, device="cuda")
    k, c = host(ops.radius_nms(grid, None, ic.R_NMS, ones, 1))
    assert k[:800].all() and not k[800:].any() and not c[800:].any() and (c[:800] >= 1).all()
    fused = host(ops.iss_keypoints(grid, None, ic.R_SALIENT, ic.R_NMS))
    assert not any(t[800:].any() for t in fused)
    assert int(grid.status.word.item()) == 0
    # a point outside the addressable grid: the status says so, its rows are 0, nothing faults
    far = a.copy()
    far[5] = [1.0e6, 0.0, 0.0]
    grid = grid_of([far], ic.R_SALIENT)
    sal, keep, cs, cn = host(ops.iss_keypoints(grid, None, ic.R_SALIENT, ic.R_NMS))
    assert int(grid.status.word.item()) & ST_CELL_RANGE
    assert sal[5] == 0 and not keep[5] and cs[5] == 0 and cn[5] == 0
    rest = np.delete(np.arange(700), 5)
    bk, bc = ic.brute_nms(far[rest], sal[rest], ic.R_NMS, ic.MIN_NEIGHBORS)      # the other rows do not notice
    assert np.array_equal(cs[rest], ic.brute_moments(far[rest], ic.R_SALIENT)[:, 0])
    assert np.array_equal(keep[rest], bk) and np.array_equal(cn[rest], bc) and bk.sum() > 5
    grid.status.word.zero_()
    k, c = host(ops.radius_nms(grid, None, ic.R_NMS, torch.ones(700, device="cuda"), 1))
    assert int(grid.status.word.item()) & ST_CELL_RANGE and not k[5] and c[5] == 0 and k[rest].all()
    # argument checks
    grid = grid_of([a], 0.1)
    with pytest.raises(RuntimeError):
        ops.iss_saliency(grid, None, ic.R_SALIENT)
    with pytest.raises(RuntimeError):
        ops.iss_keypoints(grid, None, ic.R_SALIENT, ic.R_NMS)
    with pytest.raises(RuntimeError):
        ops.radius_nms(grid, None, 0.1, np.ones(700, dtype=np.float32))
    for bad in (dict(gamma_21=0.0), dict(gamma_32=1.5), dict(min_neighbors=0)):
        with pytest.raises(ValueError):
            ops.iss_saliency(grid, None, 0.1, **bad)
    with pytest.raises(ValueError):
        ops.radius_nms(grid, None, 0.1, torch.ones(699, device="cuda"))
    with pytest.raises(ValueError):
        ops.radius_nms(grid, None, 0.0, torch.ones(700, device="cuda"))
    with pytest.raises(ValueError):
        ops.iss_saliency(grid.supports, None, 0.1)


@pytest.mark.gpu
def test_results_do_not_depend_on_order_stacking_cell_size_or_repetition(device_run):
    clouds, saliency, count, moments, keep, count_nms = device_run
    a, na = clouds[0], len(clouds[0])
    rng = np.random.default_rng(21)
    perm = rng.permutation(na)
    inv = torch.from_numpy(np.argsort(perm)).cuda()
    s2, c2, m2 = saliency_of([a[perm]])
    assert torch.equal(s2[inv], saliency[:na]) and torch.equal(c2[inv], count[:na]) and torch.equal(m2[inv], moments[:na])
    k2, n2 = nms_of([a[perm]], s2)
    assert torch.equal(k2[inv], keep[:na]) and torch.equal(n2[inv], count_nms[:na])
    # the same cloud as clouds 0 and 2 around another one that overlaps it in coordinates
    other = (a[rng.permutation(na)[:na // 2]].astype(np.float64) + rng.normal(scale=0.05, size=(na // 2, 3))).astype(np.float32)
    s3, c3, m3 = saliency_of([a, other, a])
    k3, n3 = nms_of([a, other, a], s3)
    for lo in (0, na + na // 2):
        assert torch.equal(s3[lo:lo + na], saliency[:na]) and torch.equal(m3[lo:lo + na], moments[:na])
        assert torch.equal(k3[lo:lo + na], keep[:na]) and torch.equal(n3[lo:lo + na], count_nms[:na])
    assert not torch.equal(saliency_of([np.concatenate([a, other])])[2][:na], moments[:na])
    # a coarser cell list gives the same bits, and so does a second run
    for grid_radius in (0.3, None):
        s4, c4, m4 = saliency_of(clouds, grid_radius=grid_radius)
        assert torch.equal(s4, saliency) and torch.equal(c4, count) and torch.equal(m4, moments)
        k4, n4 = nms_of(clouds, s4, grid_radius=grid_radius)
        assert torch.equal(k4, keep) and torch.equal(n4, count_nms)


@pytest.mark.gpu
def test_fused_entry_equals_its_parts_and_replays_in_a_graph(device_run):
    clouds, saliency, count, _, keep, count_nms = device_run
    grid = grid_of(clouds, ic.R_SALIENT)
    parts = (saliency, keep, count, count_nms)
    run = lambda: ops.iss_keypoints(grid, None, ic.R_SALIENT, ic.R_NMS)
    assert all(torch.equal(x, y) for x, y in zip(run(), parts))      # (and the warm-up outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = run()
    for _ in range(2):
        for t in outs:
            t.fill_(1)                                               # the replay has to compute it again
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(outs, parts))
    assert int(grid.status.word.item()) == 0
    # the non-maximum radius may be the larger one
    wide = ops.iss_keypoints(grid_of(clouds, 0.2), None, ic.R_SALIENT, 0.2)
    assert torch.equal(wide[0], saliency) and torch.equal(wide[1], nms_of(clouds, saliency, 0.2)[0])


@pytest.mark.gpu
def test_detect_iss_and_suppress_non_maxima_match_the_cpu_forms(device_run):
    clouds, saliency, _, moments, keep, _ = device_run
    assert not ic.near_threshold(moments.cpu().numpy(), Q).any()      # zero rows excluded
    clouds = [np.array(c) for c in clouds]                            # (writable copies: they become tensors)
    sal, rows = reg.detect_iss(clouds, ic.R_SALIENT, ic.R_NMS)
    sal_c, rows_c = reg.detect_iss(clouds, ic.R_SALIENT, ic.R_NMS, device="cpu")
    for k in range(2):
        assert rows[k].dtype == torch.int64 and np.array_equal(rows[k].cpu().numpy(), rows_c[k])
        assert np.array_equal(sal[k].cpu().numpy() > 0, sal_c[k] > 0)
        assert ic.ulps(sal[k].cpu().numpy(), sal_c[k]).max() <= ic.MAX_ULP
    assert [len(r) for r in rows] == [74, 72]
    na = len(clouds[0])
    scores = [saliency[:na], saliency[na:].cpu().numpy().reshape(-1, 1)]
    masks = reg.suppress_non_maxima(clouds, scores, ic.R_NMS, ic.MIN_NEIGHBORS)
    masks_c = reg.suppress_non_maxima(clouds, scores, ic.R_NMS, ic.MIN_NEIGHBORS, device="cpu")
    for k in range(2):
        assert masks[k].dtype == torch.bool and np.array_equal(masks[k].cpu().numpy(), masks_c[k])
    assert torch.equal(torch.cat(masks), keep)


@pytest.mark.gpu
def test_keypoint_repeatability_matches_the_cpu_form(device_run):
    clouds, _, _, _, keep, _ = device_run
    keep = keep.cpu().numpy()
    na = len(clouds[0])
    poses = fc.scene(ic.SEED)[1]
    G = np.linalg.inv(poses[0]) @ poses[1]
    kp = [clouds[0][keep[:na]], clouds[1][keep[na:]], np.zeros((0, 3), dtype=np.float32), np.array(clouds[0][:300])]
    keys = ["0_1", "0_2", "0_3", "1_3"]
    T = np.stack([G, np.eye(4), np.eye(4), np.linalg.inv(G)])
    for distance in (0.05, 0.1):
        got = reg.keypoint_repeatability(kp, keys, T, distance=distance)
        want = reg.keypoint_repeatability(kp, keys, T, distance=distance, device="cpu")
        for g, w in zip(got[:4], want[:4]):
            assert g.dtype == np.int64 and np.array_equal(g, w)
        assert got[4] == want[4]
    assert got[0][0] > 0 and got[0][1] == 0 and got[2][2] > 0
    empty = reg.keypoint_repeatability([kp[2], kp[2]], ["0_1"], np.eye(4)[None])
    assert empty[0].tolist() == [0] and np.isnan(empty[4])


@pytest.mark.gpu
def test_fpfh_iss_dump_and_repeatability_scene_match_the_cpu_forms(tmp_path):
    frags = ic.thin_fragments()
    poses = fc.scene(ic.SEED)[1]
    kw = dict(detector="iss", iss=dict(salient_radius=ic.R_SALIENT, non_max_radius=ic.R_NMS))
    out = {}
    for device in ("cuda", "cpu"):
        root = str(tmp_path / device)
        ev.generate_fpfh_features({"terrain": frags}, root, fc.R_FPFH, fc.R_FPFH, device=device, **kw)
        ev.writelog(os.path.join(root, "gt"), {"0_1": np.linalg.inv(poses[0]) @ poses[1]}, 2)
        _, kpath, spath = ev._paths(root, "terrain")
        scores = [ev.get_scores(spath, "cloud_bin_%d" % k) for k in range(2)]
        assert all(ev.get_keypts(kpath, "cloud_bin_%d" % k).shape == (1000, 3) for k in range(2))
        reps = [ev.repeatability_scene(root, "terrain", os.path.join(root, "gt"), num_points=(8, 64, 512), device=device,
                                       nms_radius=r) for r in (None, 0.2)]
        out[device] = (scores, reps)
    for a, b in zip(out["cuda"][0], out["cpu"][0]):
        assert np.array_equal(a > 0, b > 0) and (a > 0).sum() >= 10 and ic.ulps(a, b).max() <= ic.MAX_ULP
    for (rep_a, cnt_a), (rep_b, cnt_b) in zip(out["cuda"][1], out["cpu"][1]):
        assert rep_a == rep_b and all(np.array_equal(cnt_a[k], cnt_b[k]) for k in cnt_a)
    assert out["cuda"][1][0][1][512].sum() > out["cuda"][1][1][1][512].sum() > 0        # the suppression thinned them
