"""GPU: the ray-cast kernel (csrc/tsdf_raycast.hip) against its host twin bit for bit, depth and normals, clipped and
unclipped, on every input of the CPU tests; batches against single views and from run to run;
``tsdf_integrate(..., into=)`` on the device; a device tensor into ``depth_pyramid``; and ``track_sequence(model=...)``
on the device against the CPU path and the analytic poses.  Images of 80 x 60 at most, volumes under a million voxels
(the tracking volumes at voxel 0.01 aside)."""
import numpy as np
import pytest
import torch

from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.datasets import fragments as fr
import odometry_cases as OC
import raycast_cases as RC
import tsdf_scene as S

pytestmark = pytest.mark.gpu


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return bits(a).shape == bits(b).shape and np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("name", list(RC.cases()))
def test_device_equals_host_twin_and_the_clip_changes_no_bit(name):
    case = RC.cases()[name]
    dh, nh = ops.tsdf_raycast_host(normals=True, **case)
    dev = RC.on_device(case)
    dd, nd = ops.tsdf_raycast(normals=True, **dev)
    assert dd.is_cuda and nd.is_cuda and dd.dtype == torch.float32
    assert same_bits(dd, dh) and same_bits(nd, nh)
    du, nu = ops.tsdf_raycast(normals=True, clip=False, **dev)
    assert same_bits(du, dh) and same_bits(nu, nh)
    assert same_bits(ops.tsdf_raycast(**dev), dh)              # without the normal output
    assert bool(torch.isfinite(dd).all()) and bool(torch.isfinite(nd).all())
    if name in RC.ALL_ZERO:
        assert not bool(dd.any()) and not bool(nd.any())


def test_a_view_alone_in_a_batch_reversed_and_again():
    """Four views of two volumes of different dims, view_volume = [1, 0, 1, 0]: every view bit for bit alone, in the
    batch, in the reversed batch and from run to run."""
    frames, owner = (8, 2, 10, 4), (1, 0, 1, 0)
    batch = RC.on_device(RC.two_volumes(frames, owner))
    d, n = ops.tsdf_raycast(normals=True, **batch)
    d2, n2 = ops.tsdf_raycast(normals=True, **batch)
    assert same_bits(d, d2) and same_bits(n, n2)
    dr, nr = ops.tsdf_raycast(normals=True, **RC.on_device(RC.two_volumes(frames[::-1], owner[::-1])))
    assert same_bits(dr.flip(0), d) and same_bits(nr.flip(0), n)
    for r in range(4):
        d1, n1 = ops.tsdf_raycast(normals=True, **RC.on_device(RC.two_volumes(frames[r:r + 1], owner[r:r + 1])))
        assert same_bits(d1[0], d[r]) and same_bits(n1[0], n[r]) and float((d[r] > 0).float().mean()) > 0.9
    # render_views is the same call
    v = RC.two_volumes(frames, owner)
    again = fr.render_views(batch['D'], batch['w'], v['vol_start'], v['origin'], v['dims'], S.VOXEL, S.TRUNC, S.K,
                            v['camera_to_volume'], S.H, S.W, view_volume=owner)
    assert same_bits(again, d)


def test_the_volume_stays_on_the_device():
    case = RC.cases()['room']
    with pytest.raises(ValueError):
        ops.tsdf_raycast(**dict(case, D=torch.from_numpy(np.array(case['D'])), w=torch.from_numpy(np.array(case['w']))))
    dev = RC.on_device(RC.cases()['no_views'])
    d, n = ops.tsdf_raycast(normals=True, **dev)               # R = 0: empty tensors, no launch
    assert d.shape == (0, S.H, S.W) and n.shape == (0, S.H, S.W, 3) and d.is_cuda


# ------------------------------------------------------------------------------------------------------ into=
@pytest.mark.parametrize("name", ['dims_13x9x7', 'f32_nan', 'holes', 'partly_outside'])
def test_into_on_the_device_on_small_volumes(name):
    case = S.integrate_args(S.small_cases()[name])
    Dh, wh, _ = ops.tsdf_integrate_host(**case)
    first, second = dict(case), dict(case)
    first.update(depth=case['depth'][:1], frame_start=[0, 1], volume_to_camera=case['volume_to_camera'][:1])
    second.update(depth=case['depth'][1:], frame_start=[0, 1], volume_to_camera=case['volume_to_camera'][1:])
    D1, w1, _ = ops.tsdf_integrate(**first)
    H1, v1, _ = ops.tsdf_integrate_host(**first)
    assert same_bits(D1, H1) and same_bits(w1, v1)
    D2, w2, _ = ops.tsdf_integrate(into=(D1, w1), **second)
    H2, v2, _ = ops.tsdf_integrate_host(into=(H1, v1), **second)
    assert D2.data_ptr() == D1.data_ptr() and w2.data_ptr() == w1.data_ptr()        # in place
    assert same_bits(D2, H2) and same_bits(w2, v2)                                   # device equals twin
    assert same_bits(D2, Dh) and same_bits(w2, wh)                                   # split equals whole


@pytest.mark.parametrize("k", [1, S.PER_FRAGMENT - 1])
def test_into_on_the_device_on_the_room(k):
    depth, fs, K, M, C = S.fragment_setup()
    vol, _ = RC.fragment_volumes()
    args = (vol['origin'], vol['dims'], S.VOXEL, S.TRUNC)
    n = S.PER_FRAGMENT
    head = np.r_[np.arange(0, k), np.arange(n, n + k)]
    tail = np.r_[np.arange(k, n), np.arange(n + k, 2 * n)]
    D, w, _ = ops.tsdf_integrate(depth[head], [0, k, 2 * k], K, M[head], *args)
    ops.tsdf_integrate(depth[tail], [0, n - k, 2 * (n - k)], K, M[tail], *args, into=(D, w))
    assert same_bits(D, vol['D']) and same_bits(w, vol['w'])
    # the second volume owns no frame: unchanged; the first equals the twin's
    Dh, wh = torch.from_numpy(np.array(vol['D'])), torch.from_numpy(np.array(vol['w']))
    ops.tsdf_integrate(depth[:2], [0, 2, 2], K, M[:2], *args, into=(D, w))
    ops.tsdf_integrate_host(depth[:2], [0, 2, 2], K, M[:2], *args, into=(Dh, wh))
    cut = int(vol['vol_start'][1])
    assert same_bits(D, Dh) and same_bits(w, wh) and same_bits(D[cut:], vol['D'][cut:])
    assert float(w[:cut].max()) == n + 2
    with pytest.raises(ValueError):
        ops.tsdf_integrate(depth[:2], [0, 2, 2], K, M[:2], *args, into=(Dh, wh))     # host tensors into a device call
    with pytest.raises(ValueError):
        ops.tsdf_integrate(depth[:2], [0, 2, 2], K, M[:2], *args, into=(D[:-1], w[:-1]))


# --------------------------------------------------------------------------------------------------- device inputs
def test_depth_pyramid_takes_a_device_tensor():
    depth, K, _ = S.sequence()
    metres = (depth[:4].astype(np.float32) / np.float32(1000.0)).astype(np.float32)
    metres[1, 5, 7] = np.nan
    metres[2, 9, 3] = 7.5                                       # beyond depth_max
    host = ops.depth_pyramid(metres, K, 3)
    dev = ops.depth_pyramid(torch.from_numpy(metres).cuda(), K, 3)
    assert same_bits(dev.data, host.data) and same_bits(dev.K, host.K) and dev.table.tolist() == host.table.tolist()
    assert same_bits(ops.depth_pyramid(depth[:4], K, 3).data[[0, 3]], host.data[[0, 3]])   # and what uint16 gives
    render = ops.tsdf_raycast(**RC.on_device(RC.cases()['room']))
    pyr = ops.depth_pyramid(render, K, 3)                       # the ray-caster's output goes straight in
    assert same_bits(pyr.level(0), render) and same_bits(pyr.data, ops.depth_pyramid(render.cpu().numpy(), K, 3).data)


# ------------------------------------------------------------------------------------------------------ tracking
def frame_11_error(tracked):
    return OC.pose_error(tracked[11], OC.relative(S.sequence()[2], 11, 0))


def test_track_sequence_model_on_the_device_equals_the_cpu_path():
    """Voxel 0.02 so that the NumPy path stays short: the poses agree to 1e-6 (the odometry sums add in another
    order, as between ``depth_odometry`` and its restatement), the statuses exactly."""
    depth, K, _ = S.sequence()
    model = dict(frames_per_fragment=6, voxel=0.02, trunc=0.08)
    pc, sc, mc = fr.track_sequence(depth, K, device='cpu', model=model)
    pd, sd, md = fr.track_sequence(depth, K, device='cuda', model=model)
    print("device against CPU path: max |difference| %.3e" % np.abs(pd - pc).max())
    assert np.abs(pd - pc).max() <= 1e-6
    assert sd.tolist() == sc.tolist() and md.tolist() == mc.tolist() == [0] * 5 + [-1] + [0] * 5
    plain = fr.track_sequence(depth, K, device='cuda')
    assert len(plain) == 2 and len(fr.track_sequence(depth, K, device='cuda', model=None)) == 2


def test_track_sequence_model_on_the_device_accuracy_and_fusion():
    """The two conditions of the CPU test, on the device, at voxel 0.01: clean depth within 0.2 deg / 3 mm at frame 11;
    with the seeded 5 mm noise closer to the truth than frame to frame in degrees and in millimetres.  Then the poses
    go into ``fuse_fragments`` and give a cloud on the surface."""
    depth, K, poses = S.sequence()
    model = dict(frames_per_fragment=12, voxel=0.01)
    tracked, status, model_status = fr.track_sequence(depth, K, device='cuda', model=model)
    deg, mm = frame_11_error(tracked)
    print("clean, model at voxel 0.01: %.4f deg, %.4f mm" % (deg, mm))
    assert deg <= 0.2 and mm <= 3.0 and model_status.tolist() == [0] * 11 and status.tolist() == [0] * 11
    noisy = RC.noisy_depth()
    plain, _ = fr.track_sequence(noisy, K, device='cuda')
    against, _, noisy_status = fr.track_sequence(noisy, K, device='cuda', model=model)
    ff, mo = frame_11_error(plain), frame_11_error(against)
    print("noisy: frame to frame %.4f deg, %.4f mm; model %.4f deg, %.4f mm" % (ff + mo))
    assert mo[0] < ff[0] and mo[1] < ff[1] and noisy_status.tolist() == [0] * 11
    clouds, fposes = fr.fuse_fragments(depth, K, tracked, frames_per_fragment=S.PER_FRAGMENT, voxel=S.VOXEL,
                                       trunc=S.TRUNC, device='cuda')
    assert len(clouds) == 2 and np.array_equal(fposes, tracked[[0, 6]])
    for g, cloud in enumerate(clouds):
        dist = S.surface_distance(S.to_world(cloud, poses[g * S.PER_FRAGMENT]))
        assert len(cloud) > 4500 and dist.max() <= 1.0 * S.VOXEL
