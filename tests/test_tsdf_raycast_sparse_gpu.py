"""GPU: the sparse ray-cast kernel against its host twin bit for bit (the twin is checked against the dense twin on the
densified pool in test_tsdf_raycast_sparse_cpu.py), ``tsdf_integrate_sparse(..., into=)`` and ``tsdf_extend`` on the
device against their twins, and ``track_sequence(model=dict(sparse=True))`` against the CPU path."""
import numpy as np
import pytest
import torch

from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.datasets import fragments as fr
import raycast_sparse_cases as C
import tsdf_scene as S
import tsdf_sparse_cases as SC

pytestmark = pytest.mark.gpu
same_bits, host = SC.same_bits, SC.host


@pytest.fixture(scope="module")
def twins():
    """name -> (depth, normals) of the host twin, computed once."""
    return {name: ops.tsdf_raycast_sparse_host(**case, normals=True) for name, case in C.cases().items()}


@pytest.mark.parametrize("name", sorted(C.cases()))
def test_device_equals_host_twin_and_neither_skip_nor_clip_changes_a_bit(name, twins):
    dh, nh = twins[name]
    dev = C.on_device(C.cases()[name])
    for skip in (True, False):
        for clip in (True, False):
            dd, nd = ops.tsdf_raycast_sparse(**dev, normals=True, skip=skip, clip=clip)
            assert dd.is_cuda and nd.is_cuda and dd.dtype == torch.float32
            assert same_bits(dd, dh) and same_bits(nd, nh), (name, skip, clip)
            assert bool(torch.isfinite(dd).all()) and bool(torch.isfinite(nd).all())
    assert same_bits(ops.tsdf_raycast_sparse(**dev), dh)                  # without the normal output
    if name in C.ALL_ZERO:
        assert not bool(dd.any()) and not bool(nd.any())
    elif name in C.HITS:
        assert bool((dd > 0).any()) and bool(nd.any())


def test_a_view_alone_in_a_batch_reversed_and_again():
    """Four views of two sparse volumes of different dims, view_volume = [1, 0, 1, 0]: every view bit for bit alone, in
    the batch, in the reversed batch and from run to run."""
    frames, owner = (8, 2, 10, 4), (1, 0, 1, 0)
    batch = C.on_device(C.two_volumes(frames, owner))
    d, n = ops.tsdf_raycast_sparse(normals=True, **batch)
    d2, n2 = ops.tsdf_raycast_sparse(normals=True, **batch)
    assert same_bits(d, d2) and same_bits(n, n2)
    dr, nr = ops.tsdf_raycast_sparse(normals=True, **C.on_device(C.two_volumes(frames[::-1], owner[::-1])))
    assert same_bits(dr.flip(0), d) and same_bits(nr.flip(0), n)
    for r in range(4):
        d1, n1 = ops.tsdf_raycast_sparse(normals=True, **C.on_device(C.two_volumes(frames[r:r + 1], owner[r:r + 1])))
        assert same_bits(d1[0], d[r]) and same_bits(n1[0], n[r]) and float((d[r] > 0).float().mean()) > 0.9
    again = fr.render_views(batch['D'], batch['w'], None, None, None, None, S.TRUNC, S.K, batch['camera_to_volume'],
                            S.H, S.W, view_volume=owner, sv=batch['sv'])
    assert same_bits(again, d)


def test_the_pool_stays_on_the_device():
    case = C.cases()['room']
    with pytest.raises(ValueError):
        ops.tsdf_raycast_sparse(**dict(case, D=torch.from_numpy(np.array(case['D'])),
                                       w=torch.from_numpy(np.array(case['w']))))
    d, n = ops.tsdf_raycast_sparse(normals=True, **C.on_device(C.cases()['no_views']))       # R = 0: no launch
    assert d.shape == (0, S.H, S.W) and n.shape == (0, S.H, S.W, 3) and d.is_cuda
    dev = C.on_device(C.cases()['small_zero_frames'])                                        # B = 0: nothing to read
    assert dev['D'].shape == (0, 512)
    for min_weight in (1.0, 0.0):
        d, n = ops.tsdf_raycast_sparse(normals=True, min_weight=min_weight, **dev)
        assert d.shape == (2, S.SMALL_H, S.SMALL_W) and not bool(d.any()) and not bool(n.any())


# ---------------------------------------------------------------------------------------------------------- into=
@pytest.mark.parametrize("name", C.INTO_CASES)
def test_into_on_the_device(name):
    """Device equals twin, the split equals the whole, in place; a volume without a frame keeps its rows."""
    args = C.batch_args(name)
    sv = ops.tsdf_allocate_host(**SC.allocate_args(args))
    Dw, ww = ops.tsdf_integrate_sparse_host(**SC.sparse_args(args, sv))
    for k in (1, -1):
        head, tail = C.split_frames(args, k)
        D, w = ops.tsdf_integrate_sparse(**SC.sparse_args(head, sv))
        Dh, wh = ops.tsdf_integrate_sparse_host(**SC.sparse_args(head, sv))
        assert D.is_cuda and same_bits(D, Dh) and same_bits(w, wh)
        ptr = (D.data_ptr(), w.data_ptr())
        out = ops.tsdf_integrate_sparse(**SC.sparse_args(tail, sv), into=(D, w))
        ops.tsdf_integrate_sparse_host(**SC.sparse_args(tail, sv), into=(Dh, wh))
        assert out[0] is D and out[1] is w and (D.data_ptr(), w.data_ptr()) == ptr       # in place
        assert same_bits(D, Dh) and same_bits(w, wh)                                       # device equals twin
        assert same_bits(D, Dw) and same_bits(w, ww)                                       # split equals whole
    if name == 'room':
        bs = host(sv.brick_start)
        only_second = dict(args, depth=args['depth'][6:8], frame_start=[0, 0, 2],
                           volume_to_camera=args['volume_to_camera'][6:8])
        ops.tsdf_integrate_sparse(**SC.sparse_args(only_second, sv), into=(D, w))
        ops.tsdf_integrate_sparse_host(**SC.sparse_args(only_second, sv), into=(Dh, wh))
        assert same_bits(D, Dh) and same_bits(w, wh) and same_bits(D[:bs[1]], Dw[:bs[1]])
        assert float(w.max()) == 8.0
        with pytest.raises(ValueError):
            ops.tsdf_integrate_sparse(**SC.sparse_args(args, sv), into=(Dh, wh))           # host tensors, device call
        with pytest.raises(ValueError):
            ops.tsdf_integrate_sparse(**SC.sparse_args(args, sv), into=(D[:-1], w[:-1]))


# ---------------------------------------------------------------------------------------------------- tsdf_extend
@pytest.mark.parametrize("name", C.INTO_CASES + ('zero_frames',))
def test_extend_on_the_device(name):
    """Tables and pool equal the host twin's, and the tables those of one allocation over all frames."""
    args = S.small_cases()[name] if name == 'zero_frames' else C.batch_args(name)
    head, tail = C.split_frames(args, 1)
    sv = ops.tsdf_allocate(**SC.allocate_args(head))
    D, w = ops.tsdf_integrate_sparse(**SC.sparse_args(head, sv))
    svh = ops.tsdf_allocate_host(**SC.allocate_args(head))
    Dh, wh = ops.tsdf_integrate_sparse_host(**SC.sparse_args(head, svh))
    sv2, D2, w2 = ops.tsdf_extend(sv, D, w, **C.extend_args(tail))
    sh2, Dh2, wh2 = ops.tsdf_extend_host(svh, Dh, wh, **C.extend_args(tail))
    assert sv2.brick_index.is_cuda and D2.is_cuda and tuple(D2.shape) == (sv2.bricks, 512)
    assert SC.same_tables(sv2, sh2) and same_bits(D2, Dh2) and same_bits(w2, wh2)
    assert SC.same_tables(sv2, ops.tsdf_allocate_host(**SC.allocate_args(args)))
    # and the grown pool takes the frames: the device continues as the twin does
    ops.tsdf_integrate_sparse(**SC.sparse_args(tail, sv2), into=(D2, w2))
    ops.tsdf_integrate_sparse_host(**SC.sparse_args(tail, sh2), into=(Dh2, wh2))
    assert same_bits(D2, Dh2) and same_bits(w2, wh2)


# ------------------------------------------------------------------------------------------------------ tracking
def test_track_sequence_sparse_model_on_the_device_equals_the_cpu_path():
    """As the dense test asserts: the poses agree to 1e-6 (the odometry sums add in another order), the statuses
    exactly.  Voxel 0.02 so that the NumPy path stays short."""
    depth, K, _ = S.sequence()
    model = dict(frames_per_fragment=6, voxel=0.02, trunc=0.08, sparse=True)
    pc, sc, mc = fr.track_sequence(depth, K, device='cpu', model=model)
    pd, sd, md = fr.track_sequence(depth, K, device='cuda', model=model)
    print("device against CPU path: max |difference| %.3e" % np.abs(pd - pc).max())
    assert np.abs(pd - pc).max() <= 1e-6
    assert sd.tolist() == sc.tolist() and md.tolist() == mc.tolist() == [0] * 5 + [-1] + [0] * 5


def test_a_sparse_model_fits_on_the_device_where_the_dense_one_does_not():
    """The tracking model at voxel 0.01 (180 x 136 x 131 voxels, 25.6 MB dense) under a ``max_bytes`` of 12 MB."""
    depth, K, _ = S.sequence()
    model = dict(frames_per_fragment=4, voxel=0.01, max_bytes=12 << 20)
    with pytest.raises(ValueError):
        fr.track_sequence(depth[:4], K, device='cuda', model=model)
    tracked, status, model_status = fr.track_sequence(depth[:4], K, device='cuda', model=dict(model, sparse=True))
    assert model_status.tolist() == [0, 0, 0] and status.tolist() == [0, 0, 0]
