"""CPU: ray-casting TSDF volumes (csrc/tsdf_raycast.hpp) -- the host twin against the NumPy restatement bit for bit,
depth and normals, clipped and unclipped, on the room, the small volumes and the edge views; the rule against the
analytic room; ``tsdf_integrate(..., into=)`` against one call over all frames; ``track_sequence(model=...)`` on the room,
clean and noisy; and the C-ABI table."""
import os
import re

import numpy as np
import pytest
import torch

from d3feat_pytorch_amd import _native, ops
from d3feat_pytorch_amd.datasets import fragments as fr
import odometry_cases as OC
import raycast_cases as RC
import tsdf_scene as S
from tsdf_entry_cases import REMOVED_ENTRIES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    a = a.numpy() if hasattr(a, 'numpy') else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return bits(a).shape == bits(b).shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def numpy_results():
    """name -> (depth, normals) of every case by the restatement, clipped: computed once."""
    return {name: ops.tsdf_raycast_numpy(normals=True, **case) for name, case in RC.cases().items()}


# ------------------------------------------------------------------------------------------- twin against NumPy
@pytest.mark.parametrize("name", list(RC.cases()))
def test_twin_equals_restatement_and_the_clip_changes_no_bit(name, numpy_results):
    case = RC.cases()[name]
    dn, nn = numpy_results[name]
    R = len(case['view_volume'])
    assert dn.shape == (R, case['height'], case['width']) and nn.shape == dn.shape + (3,)
    assert np.isfinite(dn).all() and np.isfinite(nn).all()
    dh, nh = ops.tsdf_raycast_host(normals=True, **case)
    assert same_bits(dh, dn) and same_bits(nh, nn)
    du, nu = ops.tsdf_raycast_host(normals=True, clip=False, **case)
    assert same_bits(du, dh) and same_bits(nu, nh)
    if name in ('room', 'small_dims_13x9x7', 'small_holes', 'two_volumes'):    # and the restatement's own switch
        du, nu = ops.tsdf_raycast_numpy(normals=True, clip=False, **case)
        assert same_bits(du, dn) and same_bits(nu, nn)
    assert same_bits(ops.tsdf_raycast_host(**case), dn)                          # without normals: the same depth
    if name in RC.ALL_ZERO:
        assert not dn.any() and not nn.any()
    elif R and name != 'small_last_plane':
        assert (dn > 0).any()
    unit = np.linalg.norm(nn.astype(np.float64), axis=-1)
    assert np.all((unit == 0) | (np.abs(unit - 1) < 1e-6)) and not nn[dn == 0].any()


def test_edge_views(numpy_results):
    d = {name: r[0] for name, r in numpy_results.items()}
    assert 0.1 < (d['camera_inside'] > 0).mean() < 1.0                           # the camera inside the volume
    assert d['no_views'].shape == (0, S.H, S.W)
    full = ops.tsdf_raycast_numpy(**dict(RC.cases()['depth_max'], depth_max=6.0))
    cut = d['depth_max']
    assert 0 < (cut > 0).sum() < (full > 0).sum() and cut.max() <= np.float32(1.0)
    assert same_bits(cut[cut > 0], full[cut > 0])                                # what is left is what it was
    assert not cut[full > np.float32(1.0)].any()
    one = ops.tsdf_raycast_numpy(**dict(RC.cases()['one_frame_min_weight_2'], min_weight=1.0))
    assert (one > 0).mean() > 0.5                                                # the same volume at min_weight = 1


def test_a_view_in_a_batch_is_that_view_alone(numpy_results):
    """Two volumes of different dims, four views in the order view_volume = [1, 0, 1, 0]."""
    vol, _ = RC.fragment_volumes()
    assert vol['dims'][0].tolist() != vol['dims'][1].tolist()
    dn, nn = numpy_results['two_volumes']
    frames, owner = (8, 2, 10, 4), (1, 0, 1, 0)
    for make in (ops.tsdf_raycast_host, ops.tsdf_raycast_numpy):
        for r in range(4):
            d1, n1 = make(normals=True, **RC.two_volumes(frames[r:r + 1], owner[r:r + 1]))
            assert same_bits(d1[0], dn[r]) and same_bits(n1[0], nn[r]) and (dn[r] > 0).mean() > 0.9


# ---------------------------------------------------------------------------------------- against the analytic room
def test_depth_against_the_analytic_room(numpy_results):
    """At step = trunc / 2 from frames 3 and 11 and a pose between the cameras: hit share at least 0.9, at least 0.97 of
    the hits within one voxel of ``S.render``, median error at most 2 mm.  The restatement gives hit shares 0.9956,
    0.9625, 0.9860, shares within a voxel 0.9831, 0.9859, 0.9814 and medians 0.66, 0.93, 0.63 mm; the outliers (up to
    1.06 m) are silhouette pixels of the sphere."""
    depth = numpy_results['room'][0]
    for r, pose in enumerate(RC.room_view_poses()):
        hit = depth[r] > 0
        err = np.abs(depth[r].astype(np.float64) - S.render(pose))[hit]
        print("view %d: hit %.4f, within a voxel %.4f, median %.3f mm, max %.3f m"
              % (r, hit.mean(), (err <= S.VOXEL).mean(), 1e3 * np.median(err), err.max()))
        assert hit.mean() >= 0.9 and (err <= S.VOXEL).mean() >= 0.97 and np.median(err) <= 0.002


def test_normals_on_the_walls(numpy_results):
    """At hits on the room's walls, 0.16 m (two truncation distances) from every other wall and from the sphere and with
    all eight neighbours on the same wall, the angle between the normal and the wall's inward normal: the restatement
    gives at most 7.52, 13.65 and 7.66 degrees for the three views (medians 1.52, 1.45, 1.46; the depth is quantised to
    1 mm and a voxel is 20 mm).  Asserted: twice the largest, 27.3 degrees, and twice the median, 3.05.  The normals
    face the camera, n . ray < 0: on every wall pixel, and on all but silhouette pixels elsewhere (the restatement
    leaves 0, 5 and 0 of about 4500; asserted: at most 1 %)."""
    depth, normals = numpy_results['room']
    for r, pose in enumerate(RC.room_view_poses()):
        mask, truth = RC.wall_pixels(pose)
        has = np.abs(normals[r]).sum(-1) > 0
        use = mask & (depth[r] > 0) & has
        assert mask.sum() > 1000 and use.sum() > 0.9 * mask.sum()
        cos = (normals[r][use].astype(np.float64) * truth[use]).sum(-1)
        angle = np.degrees(np.arccos(np.clip(cos, -1.0, 1.0)))
        print("view %d: %d wall pixels, max %.3f deg, median %.3f deg" % (r, use.sum(), angle.max(), np.median(angle)))
        assert angle.max() <= 27.3 and np.median(angle) <= 3.05
        u, v = np.meshgrid(np.arange(S.W), np.arange(S.H))
        ray = np.stack([(u - S.K[2]) / S.K[0], (v - S.K[3]) / S.K[1], np.ones(u.shape)], axis=-1)
        facing = (normals[r] * ray).sum(-1) < 0
        assert facing[use].all() and facing[has].mean() >= 0.99


# ------------------------------------------------------------------------------------------------------ into=
def _split_case(case, k):
    """(arguments of the frames [0, k), arguments of the frames [k, F)) of a one-volume case."""
    a, b = dict(case), dict(case)
    F = int(case['frame_start'][-1])
    a.update(depth=case['depth'][:k], frame_start=[0, min(k, F)], volume_to_camera=case['volume_to_camera'][:k])
    b.update(depth=case['depth'][k:], frame_start=[0, max(F - k, 0)], volume_to_camera=case['volume_to_camera'][k:])
    for c in (a, b):
        K = np.asarray(c['intrinsics'])
        if K.ndim == 2:
            c['intrinsics'] = K[:k] if c is a else K[k:]
    return a, b


def _integrate_numpy(**kw):
    return ops.tsdf_numpy(**kw)


@pytest.mark.parametrize("name", ['dims_13x9x7', 'f32_nan', 'holes', 'partly_outside', 'depth_max'])
def test_into_equals_one_call_on_small_volumes(name):
    """Frames [0, k) and then [k, F) ``into`` the result against one call over [0, F), bit for bit; F = 2, so k = 1 is
    both k = 1 and k = F - 1."""
    case = S.integrate_args(S.small_cases()[name])
    for make in (ops.tsdf_integrate_host, ops.tsdf_numpy):
        D, w, _ = make(**case)
        first, second = _split_case(case, 1)
        D1, w1, _ = make(**first)
        D2, w2, _ = make(into=(D1, w1), **second)
        assert D2 is D1 or np.shares_memory(bits(D2), bits(D1))              # in place
        assert same_bits(D2, D) and same_bits(w2, w) and float(np.asarray(w).max()) == 2.0


@pytest.mark.parametrize("k", [1, S.PER_FRAGMENT - 1])
def test_into_equals_one_call_on_the_room(k):
    """The two fragment volumes of the room: both get their frames [0, k) first and [k, 6) ``into`` the result; then a
    call in which the second volume owns no frame leaves it unchanged."""
    depth, fs, K, M, C = S.fragment_setup()
    vol, _ = RC.fragment_volumes()
    args = (vol['origin'], vol['dims'], S.VOXEL, S.TRUNC)
    n = S.PER_FRAGMENT
    head = np.r_[np.arange(0, k), np.arange(n, n + k)]
    tail = np.r_[np.arange(k, n), np.arange(n + k, 2 * n)]
    for make in (ops.tsdf_integrate_host, ops.tsdf_numpy):
        D1, w1, _ = make(depth[head], [0, k, 2 * k], K, M[head], *args)
        D2, w2, _ = make(depth[tail], [0, n - k, 2 * (n - k)], K, M[tail], *args, into=(D1, w1))
        assert same_bits(D2, vol['D']) and same_bits(w2, vol['w'])
    # a volume that owns no frame keeps its values; the other one goes on (its weight rises by the frames given)
    D1, w1, _ = ops.tsdf_integrate_host(depth, fs, K, M, *args)
    D2, w2, _ = ops.tsdf_numpy(depth, fs, K, M, *args)
    cut = int(vol['vol_start'][1])
    for make, D, w in ((ops.tsdf_integrate_host, D1, w1), (ops.tsdf_numpy, D2, w2)):
        make(depth[:2], [0, 2, 2], K, M[:2], *args, into=(D, w))
        assert same_bits(D[cut:], vol['D'][cut:]) and same_bits(w[cut:], vol['w'][cut:])
        assert float(np.asarray(w[:cut]).max()) == n + 2
    assert same_bits(D1, D2) and same_bits(w1, w2)


def test_into_checks_sizes_and_kind():
    case = S.integrate_args(S.small_cases()['dims_13x9x7'])
    D, w, _ = ops.tsdf_integrate_host(**case)
    with pytest.raises(ValueError):
        ops.tsdf_integrate_host(into=(D[:-1], w[:-1]), **case)
    with pytest.raises(ValueError):
        ops.tsdf_integrate_host(into=(D.double(), w), **case)
    with pytest.raises(ValueError):
        ops.tsdf_integrate_host(into=D, **case)
    with pytest.raises(ValueError):
        ops.tsdf_numpy(into=(D.numpy()[:-1], w.numpy()[:-1]), **case)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            ops.tsdf_integrate(into=(D, w), **case)                             # no fall-back to the CPU


def test_raycast_arguments_are_checked():
    case = dict(RC.cases()['room'])
    for bad in (dict(step=0.0), dict(step=1e-6), dict(view_volume=[0, 1, 0]), dict(depth_min=2.0, depth_max=1.0),
                dict(height=0), dict(camera_to_volume=case['camera_to_volume'][:2]), dict(D=case['D'][:-1])):
        for make in (ops.tsdf_raycast_host, ops.tsdf_raycast_numpy):
            with pytest.raises(ValueError):
                make(**dict(case, **bad))
    with pytest.raises(ValueError):
        ops.tsdf_raycast_host(**dict(case, trunc=None))                          # step=None needs trunc
    assert ops.tsdf_raycast_host(**dict(case, trunc=None, step=0.04)).shape == (3, S.H, S.W)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            ops.tsdf_raycast(**case)                                             # no fall-back to the CPU
    d = fr.render_views(case['D'], case['w'], case['vol_start'], case['origin'], case['dims'], S.VOXEL, S.TRUNC, S.K,
                        case['camera_to_volume'], S.H, S.W, view_volume=[0, 0, 0], device='cpu')
    assert same_bits(d, ops.tsdf_raycast_numpy(**case))


# ------------------------------------------------------------------------------------------------------ tracking
@pytest.fixture(scope="module")
def frame_to_frame():
    depth, K, _ = S.sequence()
    return fr.track_sequence(depth, K, device='cpu')


def frame_11_error(tracked):
    return OC.pose_error(tracked[11], OC.relative(S.sequence()[2], 11, 0))


def test_track_sequence_against_the_model_on_clean_depth(frame_to_frame):
    """12 frames, one fragment, voxel 0.01: frame 11 within 0.2 deg / 3 mm of the truth (frame to frame reaches 0.058
    deg / 0.57 mm: on clean depth the model's quantisation costs more than drift).  The restatement gives 0.077 deg /
    1.48 mm with the default trunc of 5 voxels."""
    depth, K, _ = S.sequence()
    tracked, status, model_status = fr.track_sequence(depth, K, device='cpu',
                                                      model=dict(frames_per_fragment=12, voxel=0.01))
    deg, mm = frame_11_error(tracked)
    print("clean, model at voxel 0.01: %.4f deg, %.4f mm" % (deg, mm))
    assert deg <= 0.2 and mm <= 3.0
    assert model_status.tolist() == [0] * 11 and status.tolist() == [0] * 11 and model_status.dtype == np.int32
    assert np.array_equal(tracked[0], np.eye(4)) and not np.array_equal(tracked, frame_to_frame[0])


def test_track_sequence_against_the_model_beats_frame_to_frame_on_noisy_depth():
    """Seeded Gaussian noise of 5 mm: frame 11 is closer to the truth against the model (voxel 0.01) than frame to
    frame, in degrees and in millimetres.  The restatement gives 0.564 deg / 3.65 mm frame to frame and 0.206 deg / 2.56
    mm against the model (default trunc of 5 voxels)."""
    K = S.K
    noisy = RC.noisy_depth()
    plain, _ = fr.track_sequence(noisy, K, device='cpu')
    tracked, status, model_status = fr.track_sequence(noisy, K, device='cpu',
                                                      model=dict(frames_per_fragment=12, voxel=0.01))
    ff, mo = frame_11_error(plain), frame_11_error(tracked)
    print("noisy: frame to frame %.4f deg, %.4f mm; model %.4f deg, %.4f mm" % (ff + mo))
    assert mo[0] < ff[0] and mo[1] < ff[1]
    assert model_status.tolist() == [0] * 11 and status.tolist() == [0] * 11


def test_track_sequence_model_restarts_per_fragment_and_none_is_unchanged(frame_to_frame):
    depth, K, poses = S.sequence()
    tracked, status, model_status = fr.track_sequence(depth, K, device='cpu',
                                                      model=dict(frames_per_fragment=6, voxel=0.02, trunc=0.08))
    assert model_status.tolist() == [0] * 5 + [-1] + [0] * 5 and status.tolist() == [0] * 11
    plain, plain_status = frame_to_frame
    # the pair that crosses the boundary chains by its frame-to-frame pose
    step = np.linalg.inv(tracked[5]) @ tracked[6]
    assert np.allclose(step, np.linalg.inv(plain[5]) @ plain[6], rtol=0, atol=1e-12)
    deg, mm = frame_11_error(tracked)
    assert deg <= 0.3 and mm <= 6.0                                             # still a chain of good poses
    # model=None is the function of before: two values, and the arithmetic of the frame-to-frame chain
    again = fr.track_sequence(depth, K, device='cpu', model=None)
    assert len(again) == 2 and np.array_equal(again[0], plain) and np.array_equal(again[1], plain_status)
    T = ops.depth_odometry_numpy(depth, np.stack([np.arange(1, 12), np.arange(0, 11)], 1), intrinsics=K)[0]
    chain = np.eye(4)
    for f in range(11):
        chain = chain @ T[f]
        assert np.array_equal(plain[f + 1], chain)
    with pytest.raises(ValueError):
        fr.track_sequence(depth[:3], K, device='cpu', model=dict(voxle=0.01))


def test_a_failed_model_pair_keeps_its_frame_to_frame_pose():
    """A frame without depth: the pairs around it fail both passes, the status says which, and the poses stay put."""
    depth, K, _ = S.sequence()
    blind = depth[:4].copy()
    blind[2] = 0
    tracked, status, model_status = fr.track_sequence(blind, K, device='cpu',
                                                      model=dict(frames_per_fragment=4, voxel=0.02, trunc=0.08))
    assert model_status[0] == 0 and model_status[1] == ops.ODO_ST_FEW and status[1] == ops.ODO_ST_FEW
    assert np.array_equal(tracked[2], tracked[1])


# ----------------------------------------------------------------------------------------------------------- ABI
def test_the_new_entries_of_the_header_are_bound():
    src = open(os.path.join(REPO, "include", "d3feat_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _native.lib()
    for name in ("d3f_tsdf_raycast", "d3f_tsdf_raycast_host", "d3f_tsdf_integrate", "d3f_tsdf_integrate_host"):
        assert re.search(r"\b%s\s*\(" % name, src) and name in _native.SIGNATURES and hasattr(lib, name)
    assert len(REMOVED_ENTRIES) == 16                      # folded into the entries above: `channels` and `into`
    for name in REMOVED_ENTRIES:
        assert not re.search(r"\b%s\s*\(" % name, src) and name not in _native.SIGNATURES and not hasattr(lib, name)
    assert "tsdf_raycast.hip" in _native.SOURCES
    assert re.search(r"#define D3F_RAYCAST_MAX_SAMPLES %d\b" % ops.RAYCAST_MAX_SAMPLES, src)
