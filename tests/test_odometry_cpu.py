"""CPU: depth odometry (csrc/odometry.hpp) -- the host twins against the NumPy restatement (pyramid bit for bit, the
association index for index, the sums within the summation bound, the poses to 1e-6) and both against the analytic
poses of the room of ``tsdf_scene``; the statuses; ``track_sequence`` into ``fuse_fragments``; ``read_sequence`` without
pose files; and the C-ABI table."""
import os
import re

import numpy as np
import pytest

from d3feat_pytorch_amd import _native, ops
from d3feat_pytorch_amd.datasets import fragments as fr
import odometry_cases as OC
import tsdf_scene as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    a = a.numpy() if hasattr(a, 'numpy') else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return bits(a).shape == bits(b).shape and np.array_equal(bits(a), bits(b))


def arr(t):
    return t.numpy() if hasattr(t, 'numpy') else np.asarray(t)


@pytest.fixture(scope="module")
def room():
    """The room's pyramid by the host twin and by the restatement."""
    depth, K, _ = S.sequence()
    return ops.depth_pyramid_host(depth, K, OC.LEVELS), ops.depth_pyramid_numpy(depth, K, OC.LEVELS)


# ------------------------------------------------------------------------------------------------------- pyramid
def test_pyramid_twin_equals_restatement_on_the_room(room):
    ph, pn = room
    assert pn.table.tolist() == [[60, 80, 0], [30, 40, 4800], [15, 20, 6000]] and pn.data.shape == (12, 6300)
    assert same_bits(ph.data, pn.data) and same_bits(ph.K, pn.K)
    assert pn.K[0].tolist() == [[60.0, 60.0, 39.5, 29.5], [30.0, 30.0, 19.5, 14.5], [15.0, 15.0, 9.5, 7.0]]
    depth = S.sequence()[0]
    assert same_bits(pn.level(0), depth.astype(np.float32) / np.float32(1000.0))
    assert (pn.level(2) > 0).mean() > 0.8                      # most coarse pixels survive the depth_diff test
    assert (pn.level(1) == 0).any()                            # the sphere's silhouette does not


@pytest.mark.parametrize("name", sorted(OC.small_inputs()))
def test_pyramid_twin_equals_restatement_on_small_images(name):
    args = OC.small_inputs()[name]
    ph, pn = ops.depth_pyramid_host(**args), ops.depth_pyramid_numpy(**args)
    assert same_bits(ph.data, pn.data) and same_bits(ph.K, pn.K)
    H, W = args['depth'].shape[1:]
    assert pn.table[:, :2].tolist() == [[H >> l, W >> l] for l in range(3)]
    l0 = pn.level(0)
    if name == 'holes':
        assert not l0[:, 5:12, 10:20].any() and l0[0, 0, 0] == 0 and l0[1, 0, 0] > 0
        assert not pn.level(1)[:, 3:5, 5:10].any() and pn.level(1)[0, 0, 0] > 0   # k = 0 blocks; a block with k = 3
    if name == 'f32_nan':
        assert l0[0, 11, 18] == 0 and l0[1, 3, 30] == 0 and np.isfinite(pn.data).all()
        assert pn.level(1)[0, 5, 9] > 0                        # the NaN's block averages its three other pixels
    if name == 'depth_max':
        metres = args['depth'].astype(np.float32) / np.float32(1000.0)
        assert np.array_equal(l0 == 0, metres > np.float32(1.07)) and (l0 == 0).any() and (l0 > 0).any()
    if name == 'tiny_5x5':
        assert pn.table.tolist() == [[5, 5, 0], [2, 2, 25], [1, 1, 29]]


def test_pyramid_block_rule():
    """k valid pixels: their sequential f32 sum over (float)k; 0 when none is valid or when they span more than
    depth_diff."""
    img = np.array([[1.0, 1.02, 1.0, 1.0],
                    [0.0, 1.03, 1.0, 1.2],
                    [0.0, 0.0, 1.0, 1.05],
                    [0.0, 0.0, 1.04, 1.0]], dtype=np.float32)[None]
    for make in (ops.depth_pyramid_host, ops.depth_pyramid_numpy):
        p = make(img, [4.0, 4.0, 1.5, 1.5], levels=2, depth_diff=0.05)
        l1 = arr(p.level(1))[0]
        f32 = np.float32
        assert l1[0, 0] == ((f32(1.0) + f32(1.02)) + f32(1.03)) / f32(3.0)
        assert l1[0, 1] == 0                                   # 1.2 - 1.0 > 0.05
        assert l1[1, 0] == 0                                   # no valid pixel
        assert l1[1, 1] == (((f32(1.0) + f32(1.05)) + f32(1.04)) + f32(1.0)) / f32(4.0)   # 0.05 does not exceed 0.05
        assert arr(p.K)[0, 1].tolist() == [2.0, 2.0, 0.5, 0.5]


# ---------------------------------------------------------------------------------------------------------- step
@pytest.mark.parametrize("case", list(OC.step_cases()), ids=lambda c: c[0])
def test_step_twin_equals_restatement(case):
    """Per level, at the identity and at a second pose: the same target per pixel, the same count, the 29 sums within
    the summation bound 2 (n - 1) 2^-53 sum |term| per entry."""
    name, args, pairs, poses = case
    ph, pn = ops.depth_pyramid_host(**args), ops.depth_pyramid_numpy(**args)
    accepted = 0
    for level in range(OC.LEVELS):
        for T in poses:
            sh, ih = ops.depth_odometry_step_host(ph, pairs, T, level, return_index=True)
            sn, idx, terms = ops.depth_odometry_step_numpy(pn, pairs, T, level, return_index=True, return_terms=True)
            assert ih.dtype.is_floating_point is False and np.array_equal(arr(ih), idx)
            h, w = pn.table[level, :2]
            assert idx.shape == (len(pairs), h, w) and idx.max() < h * w
            for p in range(len(pairs)):
                n = int((idx[p] >= 0).sum())
                assert arr(sh)[p, 0] == n == sn[p, 0] == terms[p].shape[0]
                assert (np.abs(arr(sh)[p] - sn[p]) <= OC.sum_bound(terms[p])).all()
                accepted += n
    if name == 'tiny_5x5':
        sh, ih = ops.depth_odometry_step_host(ph, pairs, poses[0], 1, return_index=True)
        assert (arr(ih) == -1).all() and not arr(sh).any()     # 2 x 2: no pixel has four neighbours
    assert accepted > 0


def test_wide_case_fills_every_chunk_of_more_than_a_wave_of_chunks():
    """What the 'wide' case is for: at the identity both pairs have 65 chunks of 1024 raster pixels at level 0 (one
    more than the 64 lanes that add a pair's chunks, the last one of 832 pixels), and by the restatement's index every
    chunk holds accepted pixels, so no partial sum is trivially zero."""
    depth, K, _ = OC.wide()
    assert depth.shape[1] * depth.shape[2] == 64 * OC.CHUNK + 832
    _, idx = ops.depth_odometry_step_numpy(ops.depth_pyramid_numpy(depth, K, OC.LEVELS), OC.WIDE_PAIRS, None, 0,
                                           return_index=True)
    counts = OC.chunk_counts(idx)
    print("accepted per pair %s, fewest in a chunk %d" % (counts.sum(axis=1).tolist(), counts.min()))
    assert counts.shape == (2, 65) and counts.min() >= 1


def test_step_index_names_a_pixel_with_a_normal(room):
    """The index is a raster index of the fixed image, interior (a normal needs four neighbours), and the identity
    associates a static interior pixel of frame 0 with itself."""
    ph, pn = room
    _, idx = ops.depth_odometry_step_host(ph, [(0, 0)], None, 0, return_index=True)
    idx = arr(idx)[0]
    own = np.arange(60 * 80).reshape(60, 80)
    hit = idx >= 0
    assert hit.sum() > 4000 and np.array_equal(idx[hit], own[hit])
    assert not hit[0].any() and not hit[-1].any() and not hit[:, 0].any() and not hit[:, -1].any()


# ---------------------------------------------------------------------------------------------------------- room
@pytest.mark.parametrize("stride", [1, 2])
def test_room_pairs_are_recovered(stride):
    """All consecutive pairs of the room from the identity (stride 1: the start is up to 3.6 deg / 42 mm off; stride 2:
    6.9 deg / 85 mm).  Bounds: three times what an independent f64 prototype of the rule reached (0.032 deg / 0.31 mm
    and 0.021 deg / 0.20 mm; the depth is quantised to 1 mm and the f32 association may move a few boundary pixels):
    0.1 deg and 1 mm per pair.  The restatement reaches 0.0317 deg / 0.309 mm at stride 1 and 0.0207 deg / 0.205 mm at
    stride 2; the host twin the same to all digits shown."""
    depth, K, _ = S.sequence()
    pairs, Tt = OC.room_pairs(stride)
    Th, ch, rh, sh = ops.depth_odometry_host(depth, pairs, intrinsics=K)
    Tn, cn, rn, sn = ops.depth_odometry_numpy(depth, pairs, intrinsics=K)
    for who, T in (('twin', arr(Th)), ('restatement', Tn)):
        err = np.array([OC.pose_error(T[p], Tt[p]) for p in range(len(pairs))])
        print("stride %d, %s: max %.4f deg, %.4f mm" % (stride, who, err[:, 0].max(), err[:, 1].max()))
        assert err[:, 0].max() <= 0.1 and err[:, 1].max() <= 1.0
    assert np.abs(arr(Th) - Tn).max() < 1e-6
    assert arr(sh).tolist() == sn.tolist() == [0] * len(pairs)
    assert arr(ch).tolist() == cn.tolist() and arr(ch).min() > 3500
    assert np.allclose(arr(rh), rn, rtol=0, atol=1e-9) and 0 < arr(rh).max() < 0.02


def test_room_accumulated_pose_and_default_schedule_at_stride_3():
    """Frame 11 through the 11 chained pairs: bound 0.2 deg and 2 mm (three times the prototype's 0.058 deg / 0.57 mm);
    the restatement reaches 0.0580 deg / 0.567 mm.  The default schedule at stride 3 (10.1 deg / 127 mm off at the
    start): bound 0.1 deg and 1 mm (the prototype: 0.024 deg / 0.25 mm); the restatement and the host twin reach 0.0240 deg /
    0.253 mm."""
    depth, K, poses = S.sequence()
    tracked, status = fr.track_sequence(depth, K, device='cpu')
    assert status.tolist() == [0] * 11 and np.array_equal(tracked[0], np.eye(4))
    deg, mm = OC.pose_error(tracked[11], OC.relative(poses, 11, 0))
    print("frame 11: %.4f deg, %.4f mm" % (deg, mm))
    assert deg <= 0.2 and mm <= 2.0
    pairs, Tt = OC.room_pairs(3)
    for T in (arr(ops.depth_odometry_host(depth, pairs, intrinsics=K)[0]),
              ops.depth_odometry_numpy(depth, pairs, intrinsics=K)[0]):
        err = np.array([OC.pose_error(T[p], Tt[p]) for p in range(len(pairs))])
        print("stride 3: max %.4f deg, %.4f mm" % (err[:, 0].max(), err[:, 1].max()))
        assert err[:, 0].max() <= 0.1 and err[:, 1].max() <= 1.0


def test_information_is_the_sum_of_J_JT_rotation_first(room):
    ph, pn = room
    pairs, _ = OC.room_pairs(1)
    T, count, rmse, status, info = ops.depth_odometry_host(ph, pairs[:2], return_information=True)
    sums = arr(ops.depth_odometry_step_host(ph, pairs[:2], T, 0))
    iu = np.triu_indices(6)
    for p in range(2):
        assert np.array_equal(arr(info)[p][iu], sums[p, 1:22]) and np.array_equal(arr(info)[p], arr(info)[p].T)
        assert int(count[p]) == sums[p, 0] and float(rmse[p]) == np.sqrt(sums[p, 28] / sums[p, 0])
    In = ops.depth_odometry_numpy(pn, pairs[:2], return_information=True)[4]
    assert np.allclose(arr(info), In, rtol=1e-9)
    # rotation first: the translation block is sum n n^T, whose trace is the count (unit normals)
    assert np.allclose(np.trace(arr(info)[0][3:, 3:]), float(count[0]), rtol=1e-5)


# ------------------------------------------------------------------------------------------------------ statuses
def _both(pyr_args, pairs, T_init=None, **kw):
    ph, pn = ops.depth_pyramid_host(**pyr_args), ops.depth_pyramid_numpy(**pyr_args)
    h = [arr(t) for t in ops.depth_odometry_host(ph, pairs, T_init, **kw)]
    n = list(ops.depth_odometry_numpy(pn, pairs, T_init, **kw))
    assert h[3].tolist() == n[3].tolist() and h[1].tolist() == n[1].tolist()
    return h, n


def test_constant_depth_is_singular_and_leaves_the_pose():
    T0 = np.eye(4)
    T0[:3, 3] = [0.01, -0.02, 0.005]
    for res in _both(OC.constant_pair(), [(1, 0)], T0[None]):
        assert res[3].tolist() == [ops.ODO_ST_SINGULAR] and np.array_equal(res[0][0], T0)
        assert res[1].tolist() == [0] and res[2].tolist() == [0.0]


def test_an_empty_fixed_frame_gives_few():
    depth = S.sequence()[0][:2].copy()
    depth[0] = 0
    for res in _both(dict(depth=depth, intrinsics=S.K, levels=3), [(1, 0)]):
        assert res[3].tolist() == [ops.ODO_ST_FEW] and np.array_equal(res[0][0], np.eye(4)) and res[1].tolist() == [0]


def test_empty_coarse_levels_do_not_touch_the_pose():
    T0 = OC.small_pose()
    for res in _both(OC.small_inputs()['tiny_5x5'], [(1, 0)], T0[None]):
        assert res[3][0] in (ops.ODO_ST_FEW, ops.ODO_ST_SINGULAR) and np.array_equal(res[0][0], T0)
        assert res[1].tolist() == [0]


def test_bad_pairs_are_reported_and_leave_the_others_alone(room):
    ph, pn = room
    good = np.array([(1, 0), (4, 3)])
    Tg = [arr(t) for t in ops.depth_odometry_host(ph, good)]
    T0 = np.stack([np.eye(4)] * 5)
    T0[3, 1, 2] = np.nan
    T0[4, 0, 3] = np.inf
    pairs = np.array([(1, 0), (12, 0), (4, 3), (2, 1), (-1, 5)])
    for res in ([arr(t) for t in ops.depth_odometry_host(ph, pairs, T0)], ops.depth_odometry_numpy(pn, pairs, T0)):
        assert res[3].tolist() == [0, ops.ODO_ST_PAIR, 0, ops.ODO_ST_NONFINITE, ops.ODO_ST_PAIR | ops.ODO_ST_NONFINITE]
        assert res[1][[1, 3, 4]].tolist() == [0, 0, 0] and np.array_equal(res[0][1], np.eye(4))
        assert np.array_equal(res[0][3], T0[3], equal_nan=True) and np.array_equal(res[0][4], T0[4])
    res = [arr(t) for t in ops.depth_odometry_host(ph, pairs, T0)]
    for k, p in enumerate((0, 2)):                             # bit for bit what the pair gives without the bad ones
        assert np.array_equal(res[0][p], Tg[0][k]) and res[1][p] == Tg[1][k] and res[2][p] == Tg[2][k]
    sums, idx = ops.depth_odometry_step_host(ph, pairs, T0, 1, return_index=True)
    assert not arr(sums)[[1, 3, 4]].any() and (arr(idx)[[1, 3, 4]] == -1).all() and arr(sums)[0, 0] > 500


def test_arguments_are_checked(room):
    ph, pn = room
    with pytest.raises(ValueError):
        ops.depth_pyramid_host(S.sequence()[0], S.K, levels=7)          # 60 >> 6 = 0
    with pytest.raises(ValueError):
        ops.depth_odometry_host(ph, [(1, 0)], iterations=(10, 5))       # two counts for three levels
    with pytest.raises(ValueError):
        ops.depth_odometry_step_host(ph, [(1, 0)], None, 3)
    with pytest.raises(ValueError):
        ops.depth_odometry_host(ph, [(1, 0)], max_distance=0.0)
    with pytest.raises(RuntimeError):
        ops.depth_odometry_host(pn, [(1, 0)])                           # a NumPy pyramid is the restatement's
    assert ops.depth_odometry_host(ph, np.zeros((0, 2), dtype=int))[0].shape == (0, 4, 4)


# ---------------------------------------------------------------------------------------------------- end to end
def test_tracked_poses_fuse_into_fragments_on_the_surface():
    """``track_sequence`` then ``fuse_fragments``, no true pose inside a fragment: every point of both fragments within
    one voxel (0.02 m) of the analytic surface, the bound the TSDF tests apply with the true poses.  The restatement
    gives 0.0110 m and 0.0108 m for the two fragments."""
    depth, K, poses = S.sequence()
    tracked, status = fr.track_sequence(depth, K, device='cpu')
    assert not status.any()
    clouds, fposes = fr.fuse_fragments(depth, K, tracked, frames_per_fragment=S.PER_FRAGMENT, voxel=S.VOXEL,
                                       trunc=S.TRUNC, device='cpu')
    assert np.array_equal(fposes, tracked[[0, 6]]) and len(clouds) == 2
    for g, cloud in enumerate(clouds):                         # a fragment lives in the frame of its first camera
        dist = S.surface_distance(S.to_world(cloud, poses[g * S.PER_FRAGMENT]))
        print("fragment %d: %d points, max surface distance %.4f m" % (g, len(cloud), dist.max()))
        assert len(cloud) > 4500 and dist.max() <= 1.0 * S.VOXEL


def test_track_sequence_chunks_stride_and_failures():
    depth, K, poses = S.sequence()
    whole, _ = fr.track_sequence(depth[:6], K, device='cpu')
    chunked, status = fr.track_sequence(depth[:6], K, device='cpu', max_bytes=3 * 4 * 6300)   # three frames a chunk
    assert np.array_equal(whole, chunked) and status.shape == (5,)
    two, _ = fr.track_sequence(depth[:7], K, stride=2, device='cpu')
    assert two.shape == (4, 4, 4)
    deg, mm = OC.pose_error(two[1], OC.relative(poses, 2, 0))
    assert deg <= 0.1 and mm <= 1.0
    blind = depth[:4].copy()
    blind[2] = 0                                               # pairs (2, 1) and (3, 2) see nothing: reported, identity
    tracked, status = fr.track_sequence(blind, K, device='cpu')
    assert status.tolist() == [0, ops.ODO_ST_FEW, ops.ODO_ST_FEW]
    assert np.array_equal(tracked[2], tracked[1]) and np.array_equal(tracked[3], tracked[1])
    one, none = fr.track_sequence(depth[:1], K, device='cpu')
    assert one.shape == (1, 4, 4) and none.shape == (0,)


def test_read_sequence_without_pose_files(tmp_path):
    from PIL import Image
    depth, K, poses = S.sequence()
    folder = tmp_path / 'seq-01'
    folder.mkdir()
    np.savetxt(str(tmp_path / 'camera-intrinsics.txt'), [[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]])
    for i in range(3):
        Image.fromarray(depth[i].copy()).save(str(folder / ('frame-%06d.depth.png' % i)))
    d, k, p = fr.read_sequence(str(folder), require_poses=False)
    assert np.array_equal(d, depth[:3]) and np.array_equal(k, K) and p is None
    with pytest.raises(OSError):
        fr.read_sequence(str(folder))                          # the default still insists on the pose files
    for i in range(3):
        np.savetxt(str(folder / ('frame-%06d.pose.txt' % i)), poses[i], fmt='%.17g')
    assert np.array_equal(fr.read_sequence(str(folder), require_poses=False)[2], poses[:3])


# ----------------------------------------------------------------------------------------------------------- ABI
def test_every_odometry_entry_of_the_header_is_bound():
    src = open(os.path.join(REPO, "include", "d3feat_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = sorted(set(re.findall(r"\b(d3f_depth_[a-z0-9_]+)\s*\(", src)))
    assert declared == ["d3f_depth_odometry", "d3f_depth_odometry_host", "d3f_depth_odometry_step",
                        "d3f_depth_odometry_step_host", "d3f_depth_odometry_ws_bytes", "d3f_depth_pyramid",
                        "d3f_depth_pyramid_host", "d3f_depth_pyramid_pixels"]
    lib = _native.lib()
    for name in declared:
        assert name in _native.SIGNATURES and hasattr(lib, name)
    assert "odometry.hip" in _native.SOURCES
    assert lib.d3f_depth_pyramid_pixels(60, 80, 3) == 6300 == ops.depth_pyramid_pixels(60, 80, 3)
    assert lib.d3f_depth_pyramid_pixels(60, 80, 7) == 0
    assert lib.d3f_depth_odometry_ws_bytes(11, 60, 80) >= 11 * (12 * 8 + 5 * 29 * 8)
    for name, value in (("FEW", 1), ("PAIR", 4), ("NONFINITE", 8), ("SINGULAR", 16)):
        assert getattr(ops, "ODO_ST_" + name) == value
        assert re.search(r"#define D3F_ODO_ST_%s %d\b" % (name, value), src)
