"""CPU: RGB-D odometry (csrc/rgbd_odometry.hpp) -- the host twins and the NumPy restatement on the planar slide, where
the depth tracker is singular, and on the textured room; the intensity pyramid bit for bit; the association step within
the summation bound; ``photo_weight=0`` against the depth tracker bit for bit; the information matrix;
``track_sequence(color=)`` into ``fuse_fragments``; ``read_sequence(color=True)``; the argument checks."""
import numpy as np
import pytest

from d3feat_pytorch_amd import _native, ops
from d3feat_pytorch_amd.datasets import fragments as fr
import odometry_cases as OC
import rgbd_cases as RC
import tsdf_scene as S

HOST, NUMPY = RC.Backend('_host'), RC.Backend('_numpy')
arr = RC.arr


# --------------------------------------------------------------------------------------------- the reason for it all
@pytest.mark.parametrize("be", [HOST, NUMPY], ids=lambda b: b.name)
def test_planar_slide_is_singular_for_depth_and_tracked_with_colour(be):
    RC.check_slide(be)


@pytest.mark.parametrize("kind", ['f32', 'rgb8'])
@pytest.mark.parametrize("be", [HOST, NUMPY], ids=lambda b: b.name)
def test_textured_room_is_no_worse_than_twice_the_depth_tracker(be, kind):
    RC.check_room(be, kind)


def test_twin_and_restatement_agree_on_the_poses():
    """The poses of the host twin and of the restatement agree to 1e-6, on the room and on the slide."""
    depth, K, _, inten, _ = RC.room()
    pairs, _ = OC.room_pairs()
    a = HOST.odometry((depth, inten), pairs, intrinsics=K)
    b = NUMPY.odometry((depth, inten), pairs, intrinsics=K)
    assert np.abs(arr(a[0]) - b[0]).max() <= 1e-6 and np.array_equal(arr(a[1]), b[1]) and np.array_equal(arr(a[4]), b[4])
    sd, sK, si, sp, _ = RC.slide()
    a, b = HOST.odometry((sd, si), sp, intrinsics=sK), NUMPY.odometry((sd, si), sp, intrinsics=sK)
    assert np.abs(arr(a[0]) - b[0]).max() <= 1e-6 and np.array_equal(arr(a[4]), b[4])


# ------------------------------------------------------------------------------------------------------- pyramid
@pytest.mark.parametrize("name", sorted(RC.small_inputs()))
def test_pyramid_twin_equals_restatement_on_small_images(name):
    args, color = RC.small_inputs()[name]
    p, n = RC.check_pyramid(HOST, NUMPY, args, color)
    H, W = np.asarray(args['depth']).shape[1:]
    assert n.table[:, :2].tolist() == [[H >> l, W >> l] for l in range(3)]
    bad = ~np.isfinite(n.intensity)
    if name == 'raw_bad':                                      # the NaN and the infinity, and the pixels above them
        for l in range(3):
            want = np.zeros(n.intensity_level(l).shape, dtype=bool)
            for f, (u, v) in RC.BAD_PIXELS.items():
                want[f, v >> l, u >> l] = True
            assert np.array_equal(~np.isfinite(n.intensity_level(l)), want)
        assert np.isnan(n.intensity_level(2)[0, 0, 1]) and np.isposinf(n.intensity_level(2)[1, 0, 2])
    else:
        assert not bad.any()
    if name == 'tiny_5x5':
        assert n.table.tolist() == [[5, 5, 0], [2, 2, 25], [1, 1, 29]]


@pytest.mark.parametrize("kind", ['f32', 'rgb8', 'grey8'])
def test_pyramid_twin_equals_restatement_on_the_room(kind):
    depth, K, _, inten, rgb = RC.room()
    color = {'f32': inten, 'rgb8': rgb, 'grey8': np.ascontiguousarray(rgb[..., 1])}[kind]
    p, n = RC.check_pyramid(HOST, NUMPY, dict(depth=depth, intrinsics=K, levels=RC.LEVELS), color)
    assert n.intensity.shape == (12, 6300)
    if kind == 'f32':
        assert RC.same_bits(n.intensity_level(0), inten)
    if kind == 'grey8':
        assert RC.same_bits(n.intensity_level(0), color.astype(np.float32) / np.float32(255.0))


def test_intensity_rules():
    """Level 0 from colour in the written f32 order, and a coarser pixel as the raster-order f32 sum over 4."""
    f32 = np.float32
    rgb = np.array([[[10, 200, 30], [255, 255, 255]], [[0, 0, 0], [1, 2, 3]]], dtype=np.uint8)[None]
    depth = np.ones((1, 2, 2), dtype=np.float32)
    for be in (HOST, NUMPY):
        p = be.pyramid(depth, rgb, [2.0, 2.0, 0.5, 0.5], levels=2)
        l0, l1 = arr(p.intensity_level(0))[0], arr(p.intensity_level(1))[0]
        want = ((f32(0.299) * f32(10) + f32(0.587) * f32(200)) + f32(0.114) * f32(30)) / f32(255.0)
        assert l0[0, 0] == want and l0[1, 0] == 0 and abs(l0[0, 1] - 1.0) < 1e-6
        assert l1[0, 0] == (((l0[0, 0] + l0[0, 1]) + l0[1, 0]) + l0[1, 1]) / f32(4.0)


# ---------------------------------------------------------------------------------------------------------- step
@pytest.mark.parametrize("case", list(RC.step_cases()), ids=lambda c: c[0])
def test_step_twin_equals_restatement(case):
    photo = RC.check_step(HOST, NUMPY, case)
    if case[0] in ('room', 'raw', 'raw_bad', 'holes'):
        assert photo > 0


@pytest.mark.parametrize("be", [HOST, NUMPY], ids=lambda b: b.name)
def test_non_finite_intensity_in_the_footprint_gives_no_term(be):
    """The NaN of the fixed image (frame 0, pixel (7, 3)) lies in the footprint or the stencils of some accepted
    pixels: they add no photometric row, whatever non-finite value stands there; a finite value brings them back, and
    then the value matters."""
    args, bad = RC.small_inputs()['raw_bad']
    u, v = RC.BAD_PIXELS[0]
    sums = {}
    for key, value in (('nan', np.nan), ('inf', np.inf), ('-inf', -np.inf), ('0.5', 0.5), ('0.9', 0.9)):
        color = bad.copy()
        color[0, v, u] = value
        sums[key] = arr(be.step(RC.make_pyramid(be, args, color), [(1, 0)], None, 0))[0]
        assert np.isfinite(sums[key]).all()
    assert np.array_equal(sums['nan'], sums['inf']) and np.array_equal(sums['nan'], sums['-inf'])
    assert sums['0.5'][29] == sums['0.9'][29] > sums['nan'][29] > 0
    assert sums['0.5'][0] == sums['nan'][0] and sums['0.5'][28] == sums['nan'][28]       # the geometric part stays
    assert sums['0.5'][30] != sums['0.9'][30]
    assert sums['0.5'][29] - sums['nan'][29] <= 12                 # at most the 12 stencil positions of one pixel


# ------------------------------------------------------------------------------------------------- photo_weight 0
def test_weight_zero_is_the_depth_tracker_bit_for_bit():
    depth, K, _, inten, _ = RC.room()
    pairs, _ = OC.room_pairs()
    status = RC.check_weight_zero(HOST, HOST.pyramid(depth, inten, K, RC.LEVELS), pairs)
    assert not status.any()
    for name, (args, color) in RC.small_inputs().items():
        RC.check_weight_zero(HOST, RC.make_pyramid(HOST, args, color), [(1, 0), (0, 1)],
                             np.stack([np.eye(4), OC.small_pose()]))
    sd, sK, si, sp, _ = RC.slide()
    status = RC.check_weight_zero(HOST, HOST.pyramid(sd, si, sK, RC.LEVELS), sp)
    assert status.tolist() == [ops.ODO_ST_SINGULAR] * 2


# ---------------------------------------------------------------------------------------------------- information
def test_information_is_the_combined_sum_and_has_full_rank_on_the_slide():
    RC.check_information(HOST, exact=True)
    RC.check_information(NUMPY, exact=False)


# ---------------------------------------------------------------------------------------------------- end to end
def test_track_sequence_with_colour_chains_the_pair_poses_and_fuses():
    depth, K, poses, inten, rgb = RC.room()
    pairs, T_true = OC.room_pairs()
    T = NUMPY.odometry((depth, rgb), pairs, intrinsics=K)[0]
    tracked, status = fr.track_sequence(depth, K, device='cpu', color=rgb)
    assert not status.any() and np.array_equal(tracked[0], np.eye(4))
    for f in range(S.FRAMES - 1):
        assert np.array_equal(tracked[f + 1], tracked[f] @ T[f])
    chunked, _ = fr.track_sequence(depth, K, device='cpu', color=rgb, max_bytes=3 * 8 * 6300)   # three frames a chunk
    assert np.array_equal(chunked, tracked)
    clouds, fposes = fr.fuse_fragments(depth, K, tracked, frames_per_fragment=S.PER_FRAGMENT, voxel=S.VOXEL,
                                       trunc=S.TRUNC, device='cpu')
    assert np.array_equal(fposes, tracked[[0, 6]]) and len(clouds) == 2
    for g, cloud in enumerate(clouds):
        dist = S.surface_distance(S.to_world(cloud, poses[g * S.PER_FRAGMENT]))
        assert len(cloud) > 4500 and dist.max() <= 1.0 * S.VOXEL


def test_track_sequence_with_colour_tracks_the_slide():
    """Frames (fixed, moved) of the slide: pair (1, 0) is singular without colour and tracked with it."""
    sd, sK, si, _, T_true = RC.slide()
    plain, status = fr.track_sequence(sd[:2], sK, device='cpu')
    assert status.tolist() == [ops.ODO_ST_SINGULAR] and np.array_equal(plain[1], np.eye(4))
    tracked, status = fr.track_sequence(sd[:2], sK, device='cpu', color=si[:2])
    deg, mm = OC.pose_error(tracked[1], T_true[0])
    assert status.tolist() == [0] and deg < 0.1 and mm < 1.39
    zero, status = fr.track_sequence(sd[:2], sK, device='cpu', color=si[:2], photo_weight=0.0)
    assert status.tolist() == [ops.ODO_ST_SINGULAR]
    with pytest.raises(ValueError):
        fr.track_sequence(sd[:2], sK, device='cpu', photo_weight=0.1)
    with pytest.raises(ValueError):
        fr.track_sequence(sd[:2], sK, device='cpu', color=si[:2, :-1])


def test_read_sequence_with_colour(tmp_path):
    from PIL import Image
    depth, K, poses, _, rgb = RC.room()
    folder = tmp_path / 'seq-01'
    folder.mkdir()
    np.savetxt(str(tmp_path / 'camera-intrinsics.txt'), [[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]])
    for i in range(3):
        Image.fromarray(depth[i].copy()).save(str(folder / ('frame-%06d.depth.png' % i)))
        Image.fromarray(rgb[i].copy()).save(str(folder / ('frame-%06d.color.png' % i)))
        np.savetxt(str(folder / ('frame-%06d.pose.txt' % i)), poses[i], fmt='%.17g')
    d, k, p, c = fr.read_sequence(str(folder), color=True)
    assert np.array_equal(d, depth[:3]) and np.array_equal(p, poses[:3]) and np.array_equal(k, K)
    assert c.dtype == np.uint8 and np.array_equal(c, rgb[:3])
    assert len(fr.read_sequence(str(folder))) == 3                 # the default call is unchanged
    Image.fromarray(rgb[1, :-2].copy()).save(str(folder / 'frame-000001.color.png'))
    with pytest.raises(ValueError, match="registered"):
        fr.read_sequence(str(folder), color=True)
    (folder / 'frame-000001.color.png').unlink()
    with pytest.raises(ValueError, match="frame-000001.color.png"):
        fr.read_sequence(str(folder), color=True)
    assert len(fr.read_sequence(str(folder))) == 3


# ------------------------------------------------------------------------------------------------------ arguments
def test_arguments_are_checked():
    depth, K, _, inten, rgb = RC.room()
    for make in (ops.rgbd_pyramid_host, ops.rgbd_pyramid_numpy):
        with pytest.raises(ValueError):
            make(depth, inten[:, :-1], K)                          # not the depth's shape
        with pytest.raises(ValueError):
            make(depth, rgb[..., :2], K)
        with pytest.raises(ValueError):
            make(depth, inten.astype(np.float64), K)               # a wrong dtype
        with pytest.raises(ValueError):
            make(depth, inten[:5], K)
    ph, pn = ops.rgbd_pyramid_host(depth[:2], inten[:2], K), ops.rgbd_pyramid_numpy(depth[:2], inten[:2], K)
    for w in (-0.1, np.nan, np.inf, 1e39):
        with pytest.raises(ValueError):
            ops.rgbd_odometry_host(ph, [(1, 0)], photo_weight=w)
        with pytest.raises(ValueError):
            ops.rgbd_odometry_numpy(pn, [(1, 0)], photo_weight=w)
        with pytest.raises(ValueError):
            ops.rgbd_odometry_step_host(ph, [(1, 0)], None, 0, photo_weight=w)
    with pytest.raises(RuntimeError):
        ops.rgbd_odometry_host(ops.depth_pyramid_host(depth[:2], K), [(1, 0)])     # a pyramid without intensity
    with pytest.raises(ValueError):
        ops.rgbd_odometry_host((depth[:2], inten[:2]), [(1, 0)])                  # frames need intrinsics
    T, count, rmse, status, n_photo = ops.rgbd_odometry_host(ph, [(1, 0), (2, 0)], np.stack([np.eye(4)] * 2))
    assert arr(status).tolist() == [0, ops.ODO_ST_PAIR] and arr(n_photo)[1] == 0 and arr(n_photo)[0] > 0
    L = _native.lib()
    assert L.d3f_rgbd_odometry_ws_bytes(3, 60, 80) > L.d3f_depth_odometry_ws_bytes(3, 60, 80) > 0
    assert L.d3f_rgbd_odometry_ws_bytes(-1, 60, 80) == 0
