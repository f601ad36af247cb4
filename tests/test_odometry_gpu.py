"""GPU: the depth-odometry kernels (csrc/odometry.hip) against their host twins -- the pyramid bit for bit, the
association index for index and its sums within the summation bound, the poses to 1e-6 -- a pair alone against the same
pair in a batch, in a reversed batch and from run to run bit for bit, the statuses, and ``track_sequence`` into
``fuse_fragments`` on the device.  Images of 80 x 60 and smaller, and two of 272 x 244 (65 chunks)."""
import numpy as np
import pytest
import torch

from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.datasets import fragments as fr
import odometry_cases as OC
import tsdf_scene as S

pytestmark = pytest.mark.gpu


def arr(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def bits(a):
    return np.ascontiguousarray(arr(a), dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return bits(a).shape == bits(b).shape and np.array_equal(bits(a), bits(b))


def same_f64(a, b):
    a, b = (np.ascontiguousarray(arr(x), dtype=np.float64).view(np.uint64) for x in (a, b))
    return a.shape == b.shape and np.array_equal(a, b)


@pytest.fixture(scope="module")
def room():
    """The room's pyramid on the device and by the host twin."""
    depth, K, _ = S.sequence()
    return ops.depth_pyramid(depth, K, OC.LEVELS), ops.depth_pyramid_host(depth, K, OC.LEVELS)


@pytest.fixture(scope="module")
def room_batch(room):
    """The 11 consecutive pairs of the room in one call: (pairs, [T, count, rmse, status])."""
    pairs, _ = OC.room_pairs(1)
    return pairs, [arr(t) for t in ops.depth_odometry(room[0], pairs)]


def test_pyramid_equals_host_twin(room):
    pd, ph = room
    assert pd.data.is_cuda and pd.K.is_cuda and pd.data.shape == (12, 6300)
    assert same_bits(pd.data, ph.data) and same_bits(pd.K, ph.K)
    depth, K, _ = S.sequence()
    metres = depth.astype(np.float32) / np.float32(1000.0)     # f32 depth: the same pyramid from the other kernel
    assert same_bits(ops.depth_pyramid(metres, K, OC.LEVELS).data, ph.data)
    for name, args in OC.small_inputs().items():
        d, h = ops.depth_pyramid(**args), ops.depth_pyramid_host(**args)
        assert same_bits(d.data, h.data) and same_bits(d.K, h.K), name
        assert np.isfinite(arr(d.data)).all()


@pytest.mark.parametrize("case", list(OC.step_cases()), ids=lambda c: c[0])
def test_step_equals_host_twin(case):
    """Per level, at the identity and at a second pose: the target of every pixel and the count are the twin's; the 29
    sums agree within the summation bound 2 (n - 1) 2^-53 sum |term| per entry (the two add in different orders)."""
    name, args, pairs, poses = case
    pd, ph, pn = ops.depth_pyramid(**args), ops.depth_pyramid_host(**args), ops.depth_pyramid_numpy(**args)
    for level in range(OC.LEVELS):
        for T in poses:
            sd, idd = ops.depth_odometry_step(pd, pairs, T, level, return_index=True)
            sh, idh = ops.depth_odometry_step_host(ph, pairs, T, level, return_index=True)
            terms = ops.depth_odometry_step_numpy(pn, pairs, T, level, return_terms=True)[1]
            assert sd.is_cuda and idd.dtype == torch.int32 and np.array_equal(arr(idd), arr(idh))
            for p in range(len(pairs)):
                assert arr(sd)[p, 0] == arr(sh)[p, 0] == terms[p].shape[0]
                excess = np.abs(arr(sd)[p] - arr(sh)[p]) - OC.sum_bound(terms[p])
                print("%s level %d pair %d: n = %d, largest |device - twin| / bound = %.3g"
                      % (name, level, p, terms[p].shape[0],
                         (np.abs(arr(sd)[p] - arr(sh)[p]) / np.maximum(OC.sum_bound(terms[p]), 1e-300)).max()))
                assert (excess <= 0).all()
            assert same_f64(ops.depth_odometry_step(pd, pairs, T, level), sd)     # without the index: the same sums


def check_alone_in_a_batch_reversed_and_again(pd, pairs, batch):
    again = [arr(t) for t in ops.depth_odometry(pd, pairs)]
    back = [arr(t)[::-1] for t in ops.depth_odometry(pd, pairs[::-1].copy())]
    for other in (again, back):
        assert same_f64(other[0], batch[0]) and same_f64(other[2], batch[2])
        assert np.array_equal(other[1], batch[1]) and np.array_equal(other[3], batch[3])
    for p in range(len(pairs)):
        alone = [arr(t) for t in ops.depth_odometry(pd, pairs[p:p + 1])]
        assert same_f64(alone[0][0], batch[0][p]) and same_f64(alone[2], batch[2][p:p + 1])
        assert alone[1][0] == batch[1][p] and alone[3][0] == batch[3][p] == 0


def test_a_pair_alone_in_a_batch_reversed_and_again(room, room_batch):
    pd, _ = room
    pairs, batch = room_batch
    check_alone_in_a_batch_reversed_and_again(pd, pairs, batch)
    assert batch[1].min() > 3500
    # the wide views: 65 chunks per pair at level 0, one more than the lanes of the wave that adds them
    depth, K, _ = OC.wide()
    wide = ops.depth_pyramid(depth, K, OC.LEVELS)
    batch = [arr(t) for t in ops.depth_odometry(wide, OC.WIDE_PAIRS)]
    check_alone_in_a_batch_reversed_and_again(wide, OC.WIDE_PAIRS, batch)
    assert batch[1].min() > 55000


def test_odometry_equals_host_twin(room, room_batch):
    pd, ph = room
    pairs, (T, count, rmse, status) = room_batch
    Th, ch, rh, sh = (arr(t) for t in ops.depth_odometry_host(ph, pairs))
    print("largest |T - T_twin| = %.3g" % np.abs(T - Th).max())
    assert np.abs(T - Th).max() < 1e-6 and np.array_equal(status, sh) and not status.any()
    at_own = arr(ops.depth_odometry_step_host(ph, pairs, T, 0))   # the twin's association at the device's own final T
    assert np.array_equal(count, at_own[:, 0].astype(np.int32))
    assert np.allclose(rmse, np.sqrt(at_own[:, 28] / at_own[:, 0]), rtol=1e-12, atol=0)
    _, Tt = OC.room_pairs(1)
    err = np.array([OC.pose_error(T[p], Tt[p]) for p in range(len(pairs))])
    assert err[:, 0].max() <= 0.1 and err[:, 1].max() <= 1.0
    info = arr(ops.depth_odometry(pd, pairs[:2], return_information=True)[4])
    sums = arr(ops.depth_odometry_step(pd, pairs[:2], T[:2], 0))
    assert same_f64(info[:, np.triu_indices(6)[0], np.triu_indices(6)[1]], sums[:, 1:22])
    assert same_f64(info, info.transpose(0, 2, 1))
    # another schedule and another stride: two levels, stride 2
    pairs2, Tt2 = OC.room_pairs(2)
    depth, K, _ = S.sequence()
    Td, _, _, sd = (arr(t) for t in ops.depth_odometry(depth, pairs2, iterations=(8, 6), intrinsics=K))
    Tw, _, _, sw = (arr(t) for t in ops.depth_odometry_host(depth, pairs2, iterations=(8, 6), intrinsics=K))
    assert np.abs(Td - Tw).max() < 1e-6 and np.array_equal(sd, sw)


def test_statuses(room):
    pd, ph = room
    T0 = np.eye(4)
    T0[:3, 3] = [0.01, -0.02, 0.005]
    T, count, rmse, status = (arr(t) for t in ops.depth_odometry(ops.depth_pyramid(**OC.constant_pair()), [(1, 0)],
                                                                 T0[None]))
    assert status.tolist() == [ops.ODO_ST_SINGULAR] and np.array_equal(T[0], T0) and count.tolist() == [0]
    depth = S.sequence()[0][:2].copy()
    depth[0] = 0
    T, count, rmse, status = (arr(t) for t in ops.depth_odometry(depth, [(1, 0)], intrinsics=S.K))
    assert status.tolist() == [ops.ODO_ST_FEW] and np.array_equal(T[0], np.eye(4)) and count.tolist() == [0]
    tiny = OC.small_inputs()['tiny_5x5']
    Ts = OC.small_pose()
    T, count, rmse, status = (arr(t) for t in ops.depth_odometry(ops.depth_pyramid(**tiny), [(1, 0)], Ts[None]))
    Th, _, _, sh = (arr(t) for t in ops.depth_odometry_host(ops.depth_pyramid_host(**tiny), [(1, 0)], Ts[None]))
    assert status[0] in (ops.ODO_ST_FEW, ops.ODO_ST_SINGULAR) and status[0] == sh[0] and np.array_equal(T[0], Ts)
    # bad pairs in a batch: reported, and the others are what they are without them, bit for bit
    Tb = np.stack([np.eye(4)] * 5)
    Tb[3, 1, 2] = np.nan
    Tb[4, 0, 3] = np.inf
    pairs = np.array([(1, 0), (12, 0), (4, 3), (2, 1), (-1, 5)])
    T, count, rmse, status = (arr(t) for t in ops.depth_odometry(pd, pairs, Tb))
    assert status.tolist() == [0, ops.ODO_ST_PAIR, 0, ops.ODO_ST_NONFINITE, ops.ODO_ST_PAIR | ops.ODO_ST_NONFINITE]
    assert count[[1, 3, 4]].tolist() == [0, 0, 0] and np.array_equal(T[1], np.eye(4))
    assert np.array_equal(T[3], Tb[3], equal_nan=True) and np.array_equal(T[4], Tb[4])
    Tg, cg, rg, sg = (arr(t) for t in ops.depth_odometry(pd, pairs[[0, 2]]))
    assert same_f64(T[[0, 2]], Tg) and same_f64(rmse[[0, 2]], rg) and np.array_equal(count[[0, 2]], cg)
    sums, idx = ops.depth_odometry_step(pd, pairs, Tb, 1, return_index=True)
    assert not arr(sums)[[1, 3, 4]].any() and (arr(idx)[[1, 3, 4]] == -1).all() and arr(sums)[0, 0] > 500


def test_tracked_poses_fuse_into_fragments_on_the_surface():
    """``track_sequence`` then ``fuse_fragments``, both on the device: every point of both fragments within one voxel of
    the analytic surface."""
    depth, K, poses = S.sequence()
    tracked, status = fr.track_sequence(depth, K, device='cuda')
    assert not status.any() and np.array_equal(tracked[0], np.eye(4))
    host, _ = fr.track_sequence(depth, K, device='cpu')
    assert np.abs(tracked - host).max() < 11 * 3e-6             # eleven chained poses, each entry within 1e-6
    clouds, fposes = fr.fuse_fragments(depth, K, tracked, frames_per_fragment=S.PER_FRAGMENT, voxel=S.VOXEL,
                                       trunc=S.TRUNC, device='cuda')
    for g, cloud in enumerate(clouds):
        dist = S.surface_distance(S.to_world(cloud, poses[g * S.PER_FRAGMENT]))
        print("fragment %d: %d points, max surface distance %.4f m" % (g, len(cloud), dist.max()))
        assert len(cloud) > 4500 and dist.max() <= 1.0 * S.VOXEL
    chunked, _ = fr.track_sequence(depth[:6], K, device='cuda', max_bytes=3 * 4 * 6300)
    assert np.array_equal(chunked, tracked[:6])                # a pair's result does not depend on its chunk
