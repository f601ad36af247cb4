"""CPU: the ISS rule (csrc/iss.hpp).  The host twin of the saliency against ``eigvalsh``, the exact cases, the host twin
of the suppression against the NumPy restatement and an n x n statement bit for bit, independence of order and
stacking, repeatability against brute-force counts, and the dumps ``repeatability_scene`` reads."""
import os

import numpy as np
import pytest

from d3feat_pytorch_amd import _native, ops
from d3feat_pytorch_amd.geometric_registration import evaluate as ev
from d3feat_pytorch_amd.geometric_registration import registration as reg
import fpfh_cases as fc
import iss_cases as ic

Q = reg.normals_scale(ic.R_SALIENT)


def host_saliency(moments, q=Q, g21=ic.G21, g32=ic.G32, min_neighbors=ic.MIN_NEIGHBORS):
    return ops.iss_saliency_from_moments_host(moments, q, g21, g32, min_neighbors).numpy()


def lens_of(clouds):
    return [len(c) for c in clouds]


def test_fixture_is_the_one_the_bounds_were_measured_on():
    clouds, moments, saliency, keep, _ = ic.fixture()
    na = len(clouds[0])
    assert lens_of(clouds) == [2446, 2500]
    assert 38 < moments[:na, 0].mean() < 39 and 39 < moments[na:, 0].mean() < 40
    assert (saliency[:na] > 0).mean() > 0.99 and (saliency[na:] > 0).mean() > 0.99
    assert int(keep[:na].sum()) == 74 and int(keep[na:].sum()) == 72
    # equal positive f32 saliencies: the tie rule is exercised
    for c, s in zip(clouds, (saliency[:na], saliency[na:])):
        values, times = np.unique(s[s > 0], return_counts=True)
        assert (times > 1).sum() >= 3
        # and tied rows meet: some of them lie within the non-maximum radius of each other
        pairs = [np.nonzero(s == v)[0][:2] for v in values[times > 1]]
        assert min(np.linalg.norm(c[i] - c[j]) for i, j in pairs) < ic.R_NMS
    # the restatement holds the brute-force integers
    assert np.array_equal(reg.estimate_normals_numpy(list(clouds), ic.R_SALIENT, return_moments=True)[2], moments)


def test_host_saliency_matches_eigvalsh():
    clouds, moments, want, _, _ = ic.fixture()
    got = host_saliency(moments)
    assert got.dtype == np.float32 and got.shape == want.shape
    near = ic.near_threshold(moments, Q)
    worst = int(ic.ulps(got[~near], want[~near]).max())
    print("%d rows, %d within %.0e of a threshold, gate differs on %d, worst %d ulp" % (
        len(got), near.sum(), ic.GAP, ((got > 0) != (want > 0))[~near].sum(), worst))
    assert near.mean() <= 0.01
    assert np.array_equal(got[~near] > 0, want[~near] > 0)
    assert worst <= ic.MAX_ULP
    assert (got >= 0).all() and got.max() < ic.R_SALIENT ** 2


def test_saliency_exact_cases():
    rng = np.random.default_rng(31)
    plane = np.concatenate([rng.uniform(-1, 1, size=(1500, 2)), np.full((1500, 1), 0.5)], 1).astype(np.float32)
    m = ic.brute_moments(plane, 0.2)
    assert (m[:, 0] >= 5).all() and (m[:, [6, 8, 9]] == 0).all()
    assert (host_saliency(m, reg.normals_scale(0.2)) == 0).all()          # e3 is exactly 0: not positive
    copies = np.repeat(np.float32([[0.25, 0.5, -1.0]]), 100, 0)
    m = ic.brute_moments(copies, 0.1)
    assert (m[:, 0] == 100).all() and (host_saliency(m, reg.normals_scale(0.1)) == 0).all()
    # fewer than min_neighbors: a salient row of the fixture stops being one when more are asked for than it has
    _, moments, saliency, _, _ = ic.fixture()
    row = int(np.argmax(saliency))
    n = int(moments[row, 0])
    assert host_saliency(moments[row:row + 1], min_neighbors=n)[0] == host_saliency(moments[row:row + 1])[0] > 0
    assert host_saliency(moments[row:row + 1], min_neighbors=n + 1)[0] == 0
    assert (host_saliency(moments[moments[:, 0] < 5]) == 0).all()
    # gamma = 1 passes any strictly ordered triple: every row with distinct positive eigenvalues
    e = reg.iss_eigenvalues_numpy(moments, Q)
    ordered = (moments[:, 0] >= 5) & (e[:, 0] > e[:, 1] * (1 + 1e-9)) & (e[:, 1] > e[:, 2] * (1 + 1e-9)) & (e[:, 2] > 1e-12)
    assert ordered.mean() > 0.99
    open_gate = host_saliency(moments, g21=1.0, g32=1.0)
    assert (open_gate[ordered] > 0).all()
    assert ic.ulps(open_gate[ordered], e[ordered, 2].astype(np.float32)).max() <= ic.MAX_ULP
    strict = host_saliency(moments, g21=0.5, g32=0.5)
    assert 0 < (strict > 0).sum() < (open_gate > 0).sum() and (strict[strict > 0] == open_gate[strict > 0]).all()


def test_bad_arguments():
    lib = _native.lib()
    m = np.zeros(10, dtype=np.int64)
    out = np.zeros(1, dtype=np.float32)
    for q, g21, g32, mn in ((0.0, 0.9, 0.9, 5), (1.0, 0.0, 0.9, 5), (1.0, 0.9, 1.5, 5), (1.0, 0.9, 0.9, 0),
                            (1.0, float("nan"), 0.9, 5)):
        assert lib.d3f_iss_saliency_from_moments_host(m.ctypes.data, q, g21, g32, mn, out.ctypes.data) == -1
    assert lib.d3f_iss_saliency_from_moments_host(None, 1.0, 0.9, 0.9, 5, out.ctypes.data) == -1
    p = np.zeros((2, 3), dtype=np.float32)
    s = np.ones(2, dtype=np.float32)
    start = np.int32([0, 2])
    keep, count = np.zeros(2, dtype=np.uint8), np.zeros(2, dtype=np.int32)
    args = lambda r, mn, st=start: (p.ctypes.data, s.ctypes.data, 2, st.ctypes.data, 1, r, mn, keep.ctypes.data,
                                    count.ctypes.data)
    assert lib.d3f_radius_nms_host(*args(0.1, 1)) == 0 and keep.tolist() == [1, 1] and count.tolist() == [2, 2]
    assert lib.d3f_radius_nms_host(*args(0.0, 1)) == -1
    assert lib.d3f_radius_nms_host(*args(float("inf"), 1)) == -1
    assert lib.d3f_radius_nms_host(*args(0.1, 0)) == -1
    assert lib.d3f_radius_nms_host(*args(0.1, 1, np.int32([0, 3]))) == -1
    with pytest.raises(ValueError):
        ops.iss_saliency_from_moments_host(np.zeros((3, 9), dtype=np.int64), 1.0)
    with pytest.raises(ValueError):
        ops.iss_saliency_from_moments_host(np.zeros((3, 10), dtype=np.int64), 1.0, gamma_21=1.01)
    with pytest.raises(ValueError):
        ops.radius_nms_host(p, [2], 0.1, np.ones(3, dtype=np.float32))
    with pytest.raises(ValueError):
        ops.radius_nms_host(p, [3], 0.1, s)
    with pytest.raises(ValueError):
        reg.radius_nms_numpy([p], s, -1.0)
    with pytest.raises(ValueError):
        reg.iss_numpy([p], 0.1, 0.1, gamma_32=0.0)


def test_host_nms_equals_the_restatement_bit_for_bit():
    clouds, _, saliency, keep, count = ic.fixture()
    got = ops.radius_nms_host(np.concatenate(clouds), lens_of(clouds), ic.R_NMS, saliency, ic.MIN_NEIGHBORS)
    want = reg.radius_nms_numpy(list(clouds), saliency, ic.R_NMS, ic.MIN_NEIGHBORS)
    assert got[0].numpy().dtype == np.bool_ and got[1].numpy().dtype == np.int32
    for g, w, brute in zip(got, want, (keep, count)):
        assert np.array_equal(g.numpy(), w) and np.array_equal(w, brute)
    # [N,1] scores are the same scores
    col = ops.radius_nms_host(np.concatenate(clouds), lens_of(clouds), ic.R_NMS, saliency.reshape(-1, 1), ic.MIN_NEIGHBORS)
    assert np.array_equal(col[0].numpy(), keep) and np.array_equal(col[1].numpy(), count)


@pytest.mark.parametrize("min_neighbors", [1, 2])
def test_hand_written_ties_nan_and_lone_row(min_neighbors):
    p, s, radius, want = ic.hand_case()
    keep, count = want[min_neighbors]
    for got in (ops.radius_nms_host(p, [len(p)], radius, s, min_neighbors),
                reg.radius_nms_numpy([p], s, radius, min_neighbors), ic.brute_nms(p, s, radius, min_neighbors)):
        assert np.array_equal(np.asarray(got[0]), keep) and np.array_equal(np.asarray(got[1]), count)


def test_order_and_stacking_do_not_matter():
    clouds, _, saliency, keep, count = ic.fixture()
    a, b = clouds
    na = len(a)
    rng = np.random.default_rng(33)
    perm = rng.permutation(na)
    # a permuted fragment gives the permuted result
    sal_p, keep_p, cs_p, cn_p = reg.iss_numpy([a[perm]], ic.R_SALIENT, ic.R_NMS)
    assert np.array_equal(sal_p, saliency[:na][perm]) and np.array_equal(keep_p, keep[:na][perm])
    assert np.array_equal(cn_p, count[:na][perm])
    hk, hc = ops.radius_nms_host(a[perm], [na], ic.R_NMS, saliency[:na][perm], ic.MIN_NEIGHBORS)
    assert np.array_equal(hk.numpy(), keep[:na][perm]) and np.array_equal(hc.numpy(), count[:na][perm])
    # a fragment stacked between two others that overlap it in coordinates gives the bits it gives alone
    other = (a[rng.permutation(na)[:na // 2]].astype(np.float64) + rng.normal(scale=0.05, size=(na // 2, 3))).astype(np.float32)
    stacked = reg.iss_numpy([other, a, b[:500]], ic.R_SALIENT, ic.R_NMS)
    lo = len(other)
    assert np.array_equal(stacked[0][lo:lo + na], saliency[:na]) and np.array_equal(stacked[1][lo:lo + na], keep[:na])
    assert np.array_equal(stacked[3][lo:lo + na], count[:na])
    score = np.concatenate([np.ones(len(other), dtype=np.float32), saliency[:na], np.ones(500, dtype=np.float32)])
    hk, hc = ops.radius_nms_host(np.concatenate([other, a, b[:500]]), [len(other), na, 500], ic.R_NMS, score,
                                 ic.MIN_NEIGHBORS)
    assert np.array_equal(hk.numpy()[lo:lo + na], keep[:na]) and np.array_equal(hc.numpy()[lo:lo + na], count[:na])
    # rows beyond the lengths are not searched
    hk, hc = ops.radius_nms_host(np.concatenate(clouds), [na], ic.R_NMS, saliency, ic.MIN_NEIGHBORS)
    assert np.array_equal(hk.numpy()[:na], keep[:na]) and not hk.numpy()[na:].any() and not hc.numpy()[na:].any()


def test_detect_iss_and_suppress_non_maxima_on_the_cpu():
    clouds, _, saliency, keep, _ = ic.fixture()
    na = len(clouds[0])
    sal, rows = reg.detect_iss(list(clouds), ic.R_SALIENT, ic.R_NMS, device="cpu")
    assert np.array_equal(np.concatenate(sal), saliency)
    assert np.array_equal(rows[0], np.nonzero(keep[:na])[0]) and np.array_equal(rows[1], np.nonzero(keep[na:])[0])
    masks = reg.suppress_non_maxima(list(clouds), [saliency[:na], saliency[na:].reshape(-1, 1)], ic.R_NMS,
                                    ic.MIN_NEIGHBORS, device="cpu")
    assert np.array_equal(np.concatenate(masks), keep)
    with pytest.raises(ValueError):
        reg.suppress_non_maxima(list(clouds), [saliency[:na]], ic.R_NMS, device="cpu")


def exact_copy():
    """A keypoint set on a 2^-6 lattice and its copy under 90 degrees about z and a power-of-two shift: every
    coordinate of both, and of either moved onto the other, is exactly representable."""
    rng = np.random.default_rng(34)
    a = (rng.integers(-64, 64, size=(60, 3)) / 64.0).astype(np.float32)
    T = np.eye(4)
    T[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    T[:3, 3] = [4.0, -2.0, 0.5]                       # maps the copy's frame into a's
    inv = np.linalg.inv(T)
    b = (a.astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    return a, b, T


def test_keypoint_repeatability_on_the_cpu():
    clouds, _, _, keep, _ = ic.fixture()
    poses = fc.scene(ic.SEED)[1]
    na = len(clouds[0])
    kp = [clouds[0][keep[:na]], clouds[1][keep[na:]], np.zeros((0, 3), dtype=np.float32)]
    G = np.linalg.inv(poses[0]) @ poses[1]            # maps fragment 1 into fragment 0
    keys, T = ["0_1", "0_2"], np.stack([G, np.eye(4)])
    for distance in (0.05, 0.1):
        got = reg.keypoint_repeatability(kp, keys, T, distance=distance, device="cpu")
        want = ic.brute_repeatability(kp, keys, T, distance)
        for g, w in zip(got[:4], want[:4]):
            assert g.dtype == np.int64 and np.array_equal(g, w)
        assert got[4] == want[4]
        print("ISS keypoints %d / %d, repeated within %.2f m: %s of %s and %s of %s -> %.3f" % (
            len(kp[0]), len(kp[1]), distance, got[0], got[1], got[2], got[3], got[4]))
    # the empty fragment contributes 0 / 0: the scene's number is that of the pair 0_1 alone
    alone = reg.keypoint_repeatability(kp, ["0_1"], T[:1], distance=0.1, device="cpu")
    assert got[1].tolist() == [len(kp[1]), 0] and got[0][1] == 0 and got[2][1] == 0
    assert (got[0].sum() + got[2].sum()) / (got[1].sum() + got[3].sum()) == got[4]
    assert alone[4] == (alone[0][0] + alone[2][0]) / (len(kp[0]) + len(kp[1]))
    assert 0.0 < alone[4] < 1.0
    # a set and its exactly representable rigid copy repeat fully; apart by more than the distance, not at all
    a, b, Tab = exact_copy()
    full = reg.keypoint_repeatability([a, b], [(0, 1)], Tab[None], distance=0.01, device="cpu")
    assert full[0].tolist() == [60] and full[2].tolist() == [60] and full[4] == 1.0
    far = np.eye(4)
    far[:3, 3] = [10.0, 0, 0]
    none = reg.keypoint_repeatability([a, a], ["0_1"], far[None], distance=0.1, device="cpu")
    assert none[0].tolist() == [0] and none[2].tolist() == [0] and none[4] == 0.0
    assert np.isnan(reg.keypoint_repeatability([a[:0], a[:0]], ["0_1"], far[None], device="cpu")[4])
    with pytest.raises(ValueError):
        reg.keypoint_repeatability([a, a], ["0_2"], far[None], device="cpu")


def read_dump(root, scene="terrain", desc_name="FPFH"):
    dpath, kpath, spath = ev._paths(root, scene)
    out = []
    for k in range(len(os.listdir(kpath))):
        name = "cloud_bin_%d" % k
        out.append((ev.get_desc(dpath, name, desc_name), ev.get_keypts(kpath, name), ev.get_scores(spath, name)))
    return out


def file_bytes(root):
    out = {}
    for base, _, files in os.walk(root):
        for f in files:
            with open(os.path.join(base, f), "rb") as fh:
                out[os.path.relpath(os.path.join(base, f), root)] = fh.read()
    return out


def test_generate_fpfh_features_without_a_detector_is_unchanged(tmp_path):
    frags = [c[:400] for c in ic.thin_fragments()]
    a, b = str(tmp_path / "before"), str(tmp_path / "after")
    ev.generate_fpfh_features({"terrain": frags}, a, fc.R_FPFH, fc.R_FPFH, seed=5, device="cpu")
    ev.generate_fpfh_features({"terrain": frags}, b, fc.R_FPFH, fc.R_FPFH, seed=5, device="cpu", detector=None, iss=None)
    fa, fb = file_bytes(a), file_bytes(b)
    assert len(fa) == 6 and fa == fb
    # and the draw is the one it was: one uniform stream over the fragments in order
    rng = np.random.default_rng(5)
    for desc, _, score in read_dump(a):
        draw = 1.0 - rng.random(len(desc))
        assert np.array_equal(score[:, 0], np.where((desc != 0).any(1), draw, 0.0).astype(np.float32))
    for kw in (dict(detector="harris"), dict(detector="iss"), dict(iss=dict(salient_radius=0.1, non_max_radius=0.1)),
               dict(detector="iss", iss=dict(salient_radius=0.1))):
        with pytest.raises(ValueError):
            ev.generate_fpfh_features({"terrain": frags}, str(tmp_path / "bad"), fc.R_FPFH, device="cpu", **kw)


@pytest.fixture(scope="module")
def iss_dump(tmp_path_factory):
    """The FPFH + ISS dump of the two thin fragments on the CPU, and a hand-made gt.log beside it."""
    root = str(tmp_path_factory.mktemp("iss_dump"))
    frags = ic.thin_fragments()
    ev.generate_fpfh_features({"terrain": frags}, root, fc.R_FPFH, fc.R_FPFH, device="cpu", detector="iss",
                              iss=dict(salient_radius=ic.R_SALIENT, non_max_radius=ic.R_NMS))
    poses = fc.scene(ic.SEED)[1]
    G = np.linalg.inv(poses[0]) @ poses[1]
    ev.writelog(os.path.join(root, "gt"), {"0_1": G}, 2)
    return root, frags


def test_iss_scores_sit_exactly_on_the_detected_rows(iss_dump):
    root, frags = iss_dump
    sal, rows = reg.detect_iss(frags, ic.R_SALIENT, ic.R_NMS, device="cpu")
    for k, (desc, pts, score) in enumerate(read_dump(root)):
        assert np.array_equal(pts, frags[k]) and score.dtype == np.float32 and score.shape == (len(pts), 1)
        want = np.zeros(len(pts), dtype=np.float32)
        described = rows[k][(desc[rows[k]] != 0).any(1)]
        want[described] = sal[k][described]
        assert len(described) >= 10 and (want[described] > 0).all()
        assert np.array_equal(score[:, 0], want)


def test_repeatability_scene_reads_the_dump(iss_dump):
    root, frags = iss_dump
    dump = read_dump(root)
    positive = [int((s > 0).sum()) for _, _, s in dump]
    small, large = 8, max(positive) + 50              # the second is more than either fragment can fill
    assert min(positive) > small
    rep, counts = ev.repeatability_scene(root, "terrain", os.path.join(root, "gt"), num_points=(small, large),
                                         distance=0.1, device="cpu")
    gt = ev.loadlog(os.path.join(root, "gt"))
    assert counts[small].tolist() == [small, small] and counts[large].tolist() == positive
    for k in (small, large):
        sets = []
        for _, pts, s in dump:
            order = np.argsort(s[:, 0], kind="stable")
            top = order[-k:]
            sets.append(pts[top[s[top, 0] > 0]])
        want = ic.brute_repeatability(sets, ["0_1"], [gt["0_1"]], 0.1)[4]
        print("k = %d: %s keypoints, repeatability %.3f" % (k, counts[k].tolist(), rep[k]))
        assert rep[k] == want and 0.0 <= want <= 1.0
    # suppression at a radius that holds a whole fragment leaves its best point (and its ties) only
    rep1, counts1 = ev.repeatability_scene(root, "terrain", os.path.join(root, "gt"), num_points=(large,),
                                           nms_radius=10.0, device="cpu")
    assert counts1[large].tolist() == [1, 1]
    both, avg = ev.repeatability_scenes(root, {"terrain": os.path.join(root, "gt")}, num_points=(small, large),
                                        device="cpu")
    assert both["terrain"] == rep and avg == rep
