"""GPU: the RGB-D odometry kernels (csrc/odometry.hip) -- the planar slide and the textured room on the device;
the intensity pyramid against the host twin and the restatement bit for bit; the association step against both within
the summation bound; ``photo_weight=0`` against ``ops.depth_odometry`` bit for bit; a pair alone against the same pair
in a batch, in a reversed batch and from run to run bit for bit; the information matrix; ``track_sequence(color=)`` on
the device against ``device='cpu'``.  Images of 80 x 60 and smaller, and two of 272 x 244 (65 chunks)."""
import numpy as np
import pytest
import torch

from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.datasets import fragments as fr
import odometry_cases as OC
import rgbd_cases as RC
import tsdf_scene as S

pytestmark = pytest.mark.gpu

DEVICE, HOST, NUMPY = RC.Backend(''), RC.Backend('_host'), RC.Backend('_numpy')
arr = RC.arr


@pytest.fixture(scope="module")
def room():
    """The room's RGB-D pyramid on the device, the 11 consecutive pairs, and their result in one call."""
    depth, K, _, inten, _ = RC.room()
    pyr = ops.rgbd_pyramid(depth, inten, K, RC.LEVELS)
    pairs, _ = OC.room_pairs()
    return pyr, pairs, [arr(t) for t in ops.rgbd_odometry(pyr, pairs, return_information=True)]


def test_planar_slide_is_singular_for_depth_and_tracked_with_colour():
    T = RC.check_slide(DEVICE)
    sd, sK, si, sp, _ = RC.slide()
    assert np.abs(T - arr(HOST.odometry((sd, si), sp, intrinsics=sK)[0])).max() <= 1e-6


@pytest.mark.parametrize("kind", ['f32', 'rgb8'])
def test_textured_room_is_no_worse_than_twice_the_depth_tracker(kind):
    T = RC.check_room(DEVICE, kind)
    depth, K, _, inten, rgb = RC.room()
    pairs, _ = OC.room_pairs()
    Th = arr(HOST.odometry((depth, inten if kind == 'f32' else rgb), pairs, intrinsics=K)[0])
    assert np.abs(T - Th).max() <= 1e-6


@pytest.mark.parametrize("name", sorted(RC.small_inputs()))
def test_pyramid_equals_twin_and_restatement_on_small_images(name):
    args, color = RC.small_inputs()[name]
    p, n = RC.check_pyramid(DEVICE, NUMPY, args, color)
    assert p.intensity.is_cuda and p.data.is_cuda
    assert RC.same_intensity(p.intensity, RC.make_pyramid(HOST, args, color).intensity)
    if name == 'raw_bad':
        for l in range(3):
            want = np.zeros(n.intensity_level(l).shape, dtype=bool)
            for f, (u, v) in RC.BAD_PIXELS.items():
                want[f, v >> l, u >> l] = True
            assert np.array_equal(~np.isfinite(arr(p.intensity_level(l))), want)
    else:
        assert np.isfinite(arr(p.intensity)).all()


@pytest.mark.parametrize("kind", ['f32', 'rgb8', 'grey8'])
def test_pyramid_equals_twin_and_restatement_on_the_room(kind):
    depth, K, _, inten, rgb = RC.room()
    color = {'f32': inten, 'rgb8': rgb, 'grey8': np.ascontiguousarray(rgb[..., 1])}[kind]
    args = dict(depth=depth, intrinsics=K, levels=RC.LEVELS)
    p, n = RC.check_pyramid(DEVICE, NUMPY, args, color)
    assert RC.same_bits(p.intensity, RC.make_pyramid(HOST, args, color).intensity)
    if kind == 'f32':                                          # an f32 intensity already on the device is taken there
        q = ops.rgbd_pyramid(depth, torch.from_numpy(inten.copy()).cuda(), K, RC.LEVELS)
        assert RC.same_bits(q.intensity, p.intensity)


@pytest.mark.parametrize("case", list(RC.step_cases()), ids=lambda c: c[0])
def test_step_equals_twin_and_restatement(case):
    photo = RC.check_step(DEVICE, NUMPY, case, twin=HOST)
    if case[0] in ('room', 'raw', 'raw_bad', 'holes'):
        assert photo > 0


def test_non_finite_intensity_in_the_footprint_gives_no_term():
    args, bad = RC.small_inputs()['raw_bad']
    u, v = RC.BAD_PIXELS[0]
    sums = {}
    for key, value in (('nan', np.nan), ('inf', np.inf), ('0.5', 0.5), ('0.9', 0.9)):
        color = bad.copy()
        color[0, v, u] = value
        sums[key] = arr(ops.rgbd_odometry_step(RC.make_pyramid(DEVICE, args, color), [(1, 0)], None, 0))[0]
        assert np.isfinite(sums[key]).all()
    assert np.array_equal(sums['nan'], sums['inf'])
    assert sums['0.5'][29] == sums['0.9'][29] > sums['nan'][29] > 0
    assert sums['0.5'][0] == sums['nan'][0] and sums['0.5'][28] == sums['nan'][28]
    assert sums['0.5'][30] != sums['0.9'][30]


def test_weight_zero_is_the_depth_tracker_bit_for_bit(room):
    pyr, pairs, _ = room
    assert not RC.check_weight_zero(DEVICE, pyr, pairs).any()
    for name, (args, color) in RC.small_inputs().items():
        RC.check_weight_zero(DEVICE, RC.make_pyramid(DEVICE, args, color), [(1, 0), (0, 1)],
                             np.stack([np.eye(4), OC.small_pose()]))
    sd, sK, si, sp, _ = RC.slide()
    status = RC.check_weight_zero(DEVICE, ops.rgbd_pyramid(sd, si, sK, RC.LEVELS), sp)
    assert status.tolist() == [ops.ODO_ST_SINGULAR] * 2


def check_alone_in_a_batch_reversed_and_again(pyr, pairs, batch, alone_pairs):
    again = [arr(t) for t in ops.rgbd_odometry(pyr, pairs, return_information=True)]
    back = [arr(t)[::-1] for t in ops.rgbd_odometry(pyr, pairs[::-1].copy(), return_information=True)]
    for a, b, c in zip(batch, again, back):
        if a.dtype == np.float64:
            assert RC.same_bits(a, b, np.float64) and RC.same_bits(a, c, np.float64)
        else:
            assert np.array_equal(a, b) and np.array_equal(a, c)
    for p in alone_pairs:
        alone = [arr(t)[0] for t in ops.rgbd_odometry(pyr, pairs[p:p + 1], return_information=True)]
        for a, b in zip(alone, batch):
            assert RC.same_bits(a, b[p], np.float64) if b.dtype == np.float64 else a == b[p]


def test_a_pair_alone_in_a_batch_reversed_and_again_is_bit_identical(room):
    pyr, pairs, batch = room
    check_alone_in_a_batch_reversed_and_again(pyr, pairs, batch, (0, 4, 10))
    s_all = arr(ops.rgbd_odometry_step(pyr, pairs, batch[0], 0))
    s_one = arr(ops.rgbd_odometry_step(pyr, pairs[3:4], batch[0][3:4], 0))
    assert RC.same_bits(s_all[3], s_one[0], np.float64)
    # the wide views: 65 chunks per pair at level 0, one more than the lanes of the wave that adds them
    depth, K, _, inten = RC.wide()
    wide = ops.rgbd_pyramid(depth, inten, K, RC.LEVELS)
    batch = [arr(t) for t in ops.rgbd_odometry(wide, OC.WIDE_PAIRS, return_information=True)]
    check_alone_in_a_batch_reversed_and_again(wide, OC.WIDE_PAIRS, batch, (0, 1))
    assert not batch[3].any() and batch[1].min() > 55000 and batch[5].min() > 55000
    s_all = arr(ops.rgbd_odometry_step(wide, OC.WIDE_PAIRS, batch[0], 0))
    s_one = arr(ops.rgbd_odometry_step(wide, OC.WIDE_PAIRS[1:], batch[0][1:], 0))
    assert RC.same_bits(s_all[1], s_one[0], np.float64)


def test_information_is_the_combined_sum_and_has_full_rank_on_the_slide():
    RC.check_information(DEVICE, exact=True)


def test_track_sequence_with_colour_on_the_device():
    depth, K, poses, inten, rgb = RC.room()
    dev, status = fr.track_sequence(depth, K, color=rgb)
    cpu, status_cpu = fr.track_sequence(depth, K, device='cpu', color=rgb)
    assert not status.any() and np.array_equal(status, status_cpu) and np.abs(dev - cpu).max() <= 1e-6
    pairs, _ = OC.room_pairs()
    T = arr(ops.rgbd_odometry((depth, rgb), pairs, intrinsics=K)[0])
    for f in range(S.FRAMES - 1):
        assert np.array_equal(dev[f + 1], dev[f] @ T[f])
    clouds, fposes = fr.fuse_fragments(depth, K, dev, frames_per_fragment=S.PER_FRAGMENT, voxel=S.VOXEL, trunc=S.TRUNC)
    assert len(clouds) == 2 and np.array_equal(fposes, dev[[0, 6]])
    for g, cloud in enumerate(clouds):
        dist = S.surface_distance(S.to_world(arr(cloud), poses[g * S.PER_FRAGMENT]))
        assert len(cloud) > 4500 and dist.max() <= 1.0 * S.VOXEL
    sd, sK, si, _, T_true = RC.slide()
    plain, status = fr.track_sequence(sd[:2], sK)
    assert status.tolist() == [ops.ODO_ST_SINGULAR]
    tracked, status = fr.track_sequence(sd[:2], sK, color=si[:2])
    deg, mm = OC.pose_error(tracked[1], T_true[0])
    assert status.tolist() == [0] and deg < 0.1 and mm < 1.39
    cpu, _ = fr.track_sequence(sd[:2], sK, device='cpu', color=si[:2])
    assert np.abs(tracked - cpu).max() <= 1e-6


def test_arguments_are_checked_on_the_device():
    depth, K, _, inten, _ = RC.room()
    with pytest.raises(ValueError):
        ops.rgbd_pyramid(depth, inten[:, :-1], K)
    pyr = ops.rgbd_pyramid(depth[:2], inten[:2], K)
    for w in (-0.1, np.nan, np.inf):
        with pytest.raises(ValueError):
            ops.rgbd_odometry(pyr, [(1, 0)], photo_weight=w)
    with pytest.raises(RuntimeError):
        ops.rgbd_odometry(ops.depth_pyramid(depth[:2], K), [(1, 0)])
    with pytest.raises(RuntimeError):
        ops.rgbd_odometry(ops.rgbd_pyramid_host(depth[:2], inten[:2], K), [(1, 0)])
    T, count, rmse, status, n_photo = ops.rgbd_odometry(pyr, [(1, 0), (2, 0)], np.stack([np.eye(4)] * 2))
    assert arr(status).tolist() == [0, ops.ODO_ST_PAIR] and arr(n_photo)[1] == 0 and arr(n_photo)[0] > 0
