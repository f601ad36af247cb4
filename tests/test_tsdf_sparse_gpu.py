"""GPU: the sparse TSDF kernels (csrc/tsdf_sparse.hip, csrc/tsdf_integrate.hip) against their host twins bit for bit -- tables, pool, points and
point_start on the room of ``tsdf_scene`` (two fragments as one batch) and on every small volume -- batches against
single volumes and from run to run, uint16 against f32 depth, the capacity rule of the extraction, and
``fuse_fragments(sparse=True)`` on the device against the CPU path."""
import numpy as np
import pytest
import torch

from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.datasets import fragments as fr
import tsdf_scene as S
import tsdf_sparse_cases as SC
from tsdf_sparse_cases import host, same_bits, same_tables

pytestmark = pytest.mark.gpu


def host_twins(case):
    sv = ops.tsdf_allocate_host(**SC.allocate_args(case))
    D, w = ops.tsdf_integrate_sparse_host(**SC.sparse_args(case, sv))
    pts, ps = ops.tsdf_extract_sparse_host(D, w, sv)
    return sv, D, w, pts, ps


def device_equals_host(case):
    sv, D, w, pts, ps = host_twins(case)
    svd = ops.tsdf_allocate(**SC.allocate_args(case))
    assert svd.brick_index.is_cuda and svd.brick_coord.is_cuda and svd.brick_start.is_cuda
    assert same_tables(svd, sv)
    Dd, wd = ops.tsdf_integrate_sparse(**SC.sparse_args(case, svd))
    assert Dd.is_cuda and tuple(Dd.shape) == (sv.bricks, 512)
    assert same_bits(Dd, D) and same_bits(wd, w)
    pd, psd = ops.tsdf_extract_sparse(Dd, wd, svd)
    assert psd.tolist() == ps.tolist() and same_bits(pd, pts)              # equal and in the same order
    return sv, D, w, pts, ps


@pytest.fixture(scope="module")
def room():
    """The two fragments of the room as one batch, device checked against the host twins: (args, sv, D, w, pts, ps)."""
    args = SC.room_args()
    return (args,) + device_equals_host(args)


def test_device_equals_host_twin_on_the_room(room):
    args, sv, D, w, pts, ps = room
    # both scans cross a group of 1024: the flags of the lattice bricks, and the count blocks (two per brick)
    assert int(sv.lattice_start[-1]) == 2 * 891 > 1024 and 2 * sv.bricks > 1024
    assert int(ps[-1]) > 12000 and (host(sv.brick_index) < 0).any()
    svd = ops.tsdf_allocate(**SC.allocate_args(args))
    p2, ps2 = ops.tsdf_extract_sparse(D.cuda(), w.cuda(), svd, min_weight=2.0)
    h2, hs2 = ops.tsdf_extract_sparse_host(D, w, sv, min_weight=2.0)
    assert ps2.tolist() == hs2.tolist() and same_bits(p2, h2) and 0 < int(hs2[-1]) < int(ps[-1])


@pytest.mark.parametrize("name", sorted(SC.cases()))
def test_device_equals_host_twin_on_small_volumes(name):
    sv, D, w, pts, ps = device_equals_host(SC.cases()[name])
    assert (int(ps[-1]) == 0) == (sv.bricks == 0) == (name in ('zero_frames', 'behind_camera'))


@pytest.mark.parametrize("empty", sorted(SC.EMPTY_BETWEEN))
def test_a_batch_equals_its_volumes_alone_and_itself(empty):
    """Three volumes in one launch, the middle one without a brick."""
    names = SC.EMPTY_BETWEEN[empty]
    batch = SC.batch_of(names)
    sv, D, w, pts, ps = device_equals_host(batch)
    start, lattice = host(sv.brick_start).tolist(), sv.lattice_start.tolist()
    assert start[1] == start[2] and int(ps[1]) == int(ps[2]) and 0 < int(ps[1]) < int(ps[3])
    for run in range(2):                                       # from run to run
        svr = ops.tsdf_allocate(**SC.allocate_args(batch))
        Dr, wr = ops.tsdf_integrate_sparse(**SC.sparse_args(batch, svr))
        pr, psr = ops.tsdf_extract_sparse(Dr, wr, svr)
        assert same_tables(svr, sv) and same_bits(Dr, D) and same_bits(wr, w)
        assert same_bits(pr, pts) and psr.tolist() == ps.tolist()
    for v, name in enumerate(names):
        case = SC.cases()[name]
        sva = ops.tsdf_allocate(**SC.allocate_args(case))
        assert np.array_equal(host(sva.brick_index), host(sv.brick_index)[lattice[v]:lattice[v + 1]])
        assert np.array_equal(host(sva.brick_coord), host(sv.brick_coord)[start[v]:start[v + 1]])
        Da, wa = ops.tsdf_integrate_sparse(**SC.sparse_args(case, sva))
        assert same_bits(Da, D[start[v]:start[v + 1]]) and same_bits(wa, w[start[v]:start[v + 1]])
        pa, psa = ops.tsdf_extract_sparse(Da, wa, sva)
        assert same_bits(pa, pts[int(ps[v]):int(ps[v + 1])]) and int(psa[1]) == int(ps[v + 1] - ps[v])


def test_an_absent_neighbour_brick_on_the_device():
    sv, D, w = SC.absent_neighbour_pool()
    ph, psh = ops.tsdf_extract_sparse_host(D, w, sv)
    pd, psd = ops.tsdf_extract_sparse(D, w, sv)
    assert psd.tolist() == psh.tolist() == [0, 64] and same_bits(pd, ph)


def test_uint16_and_f32_depth_give_the_same_pool(room):
    args, sv, D, w, pts, ps = room
    metres = dict(args, depth=args['depth'].astype(np.float32) / np.float32(1000.0))
    svd = ops.tsdf_allocate(**SC.allocate_args(metres))
    assert same_tables(svd, sv)
    Dd, wd = ops.tsdf_integrate_sparse(**SC.sparse_args(metres, svd))
    assert same_bits(Dd, D) and same_bits(wd, w)


def test_capacity_sets_the_overflow_bit(room):
    args, sv, D, w, pts, ps = room
    cap = 1000
    p, s, status = ops.tsdf_extract_sparse(D.cuda(), w.cuda(), sv, capacity=cap, return_status=True)
    assert int(status.item()) == ops.TSDF_ST_OVERFLOW and s.tolist() == ps.tolist()
    assert tuple(p.shape) == (cap, 3) and same_bits(p, pts[:cap])
    p, s, status = ops.tsdf_extract_sparse(D.cuda(), w.cuda(), sv, capacity=int(ps[-1]), return_status=True)
    assert int(status.item()) == 0 and same_bits(p, pts) and s.tolist() == ps.tolist()


def test_capacity_is_enforced_inside_a_larger_buffer(room):
    """The raw entry point with a capacity smaller than the buffer: the rows past the capacity keep their content."""
    from d3feat_pytorch_amd import _native
    args, sv, D, w, pts, ps = room
    dev = torch.device('cuda')
    Dd, wd = ops._sparse_pool(D, w, sv, dev)
    tls, bs, bi, bc, to, tn, tvx = ops._sparse_tables(sv, dev)
    V, lattice, B = sv.volumes, int(sv.lattice_start[-1]), sv.bricks
    L = _native.lib()
    nbytes = L.d3f_tsdf_sparse_extract_ws_bytes(B)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    cap, rows = 777, 2000
    points = torch.full((rows, 3), -7.0, device=dev)
    point_start = torch.zeros(V + 1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = L.d3f_tsdf_sparse_extract(Dd.data_ptr(), wd.data_ptr(), tls.data_ptr(), bs.data_ptr(), bi.data_ptr(),
                                   bc.data_ptr(), to.data_ptr(), tn.data_ptr(), tvx.data_ptr(), V, lattice, B, 1.0, 0,
                                   cap, points.data_ptr(), point_start.data_ptr(), status.data_ptr(), ws.data_ptr(),
                                   nbytes, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert int(status.item()) == ops.TSDF_ST_OVERFLOW and point_start.tolist() == ps.tolist()
    assert same_bits(points[:cap], pts[:cap]) and bool((points[cap:] == -7.0).all())


def test_densify_on_the_device_is_the_dense_volume_inside_the_bricks(room):
    args, sv, D, w, pts, ps = room
    Dd, wd, vs = ops.tsdf_integrate(args['depth'], args['frame_start'], args['intrinsics'], args['volume_to_camera'],
                                    args['origin'], args['dims'], S.VOXEL, S.TRUNC)
    svd = ops.tsdf_allocate(**SC.allocate_args(args))
    ones = torch.ones((sv.bricks, 512), device='cuda')
    inside = ops.tsdf_densify(ones, ones, svd)[0] > 0
    Ds, ws_, vss = ops.tsdf_densify(D.cuda(), w.cuda(), svd)
    assert Ds.is_cuda and vss.tolist() == vs.tolist() and 0 < int(inside.sum()) < inside.numel()
    assert same_bits(Ds[inside], Dd[inside]) and same_bits(ws_[inside], wd[inside])
    assert not bool(Ds[~inside].any()) and not bool(ws_[~inside].any())
    valid = (wd >= 1) & (Dd.abs() < 1)
    assert not bool((valid & ~inside).any())                   # the superset, against the dense kernel's own volume


def test_fuse_fragments_sparse_on_the_device_equals_the_cpu_path():
    depth, K, poses = S.sequence()
    kw = dict(frames_per_fragment=S.PER_FRAGMENT, voxel=S.VOXEL, trunc=S.TRUNC, sparse=True)
    cpu, poses_cpu = fr.fuse_fragments(depth, K, poses, device='cpu', **kw)
    gpu, poses_gpu = fr.fuse_fragments(depth, K, poses, device='cuda', **kw)
    assert len(gpu) == 2 and all(same_bits(a, b) for a, b in zip(gpu, cpu)) and np.array_equal(poses_cpu, poses_gpu)
    scene_cpu = fr.fuse_scene(depth, K, poses, poses_cpu, S.PER_FRAGMENT, S.VOXEL, trunc=S.TRUNC, device='cpu',
                              sparse=True)
    scene_gpu = fr.fuse_scene(depth, K, poses, poses_cpu, S.PER_FRAGMENT, S.VOXEL, trunc=S.TRUNC, device='cuda',
                              sparse=True)
    assert same_bits(scene_gpu, scene_cpu) and S.surface_distance(scene_gpu).max() <= 1.0 * S.VOXEL
    with pytest.raises(ValueError, match="allocated bricks"):
        fr.fuse_fragments(depth, K, poses, device='cuda', max_bytes=1 << 16, **kw)
