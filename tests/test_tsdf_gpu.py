"""GPU: the TSDF kernels (csrc/tsdf.hip, csrc/tsdf_integrate.hip) against their host twins bit for bit -- bounds, D, w, points and point_start on
the analytic room of ``tsdf_scene`` and on every small volume -- batches against single volumes and from run to run, the
capacity rule of the extraction, uint16 against f32 depth, and ``fuse_fragments`` on the device against the CPU path."""
import numpy as np
import pytest
import torch

from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.datasets import fragments as fr
from d3feat_pytorch_amd.datasets import preprocess as pp
import tsdf_scene as S

pytestmark = pytest.mark.gpu


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return bits(a).shape == bits(b).shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def scene_host():
    """The two fragment volumes of the room by the host twins: (setup, origin, dims, D, w, points, point_start)."""
    depth, fs, K, M, C = S.fragment_setup()
    bounds = ops.tsdf_bounds_host(depth, fs, K, C)
    origin, dims = fr.place_volumes(bounds.numpy(), S.VOXEL)
    D, w, vs = ops.tsdf_integrate_host(depth, fs, K, M, origin, dims, S.VOXEL, S.TRUNC)
    pts, ps = ops.tsdf_extract_host(D, w, vs, origin, dims, S.VOXEL)
    return (depth, fs, K, M, C), bounds, origin, dims, D, w, pts, ps


def test_device_equals_host_twin_on_the_scene(scene_host):
    (depth, fs, K, M, C), bounds, origin, dims, D, w, pts, ps = scene_host
    assert same_bits(ops.tsdf_bounds(depth, fs, K, C), bounds)
    Dd, wd, vs = ops.tsdf_integrate(depth, fs, K, M, origin, dims, S.VOXEL, S.TRUNC)
    assert Dd.is_cuda and vs.tolist() == [0, 86 * 70 * 66, 86 * 70 * 66 + 83 * 66 * 67]
    assert same_bits(Dd, D) and same_bits(wd, w)
    pd, psd = ops.tsdf_extract(Dd, wd, vs, origin, dims, S.VOXEL)
    assert psd.tolist() == ps.tolist() and int(ps[-1]) > 12000
    assert same_bits(pd, pts)                                  # equal and in the same order
    # the voxel counts are no multiple of the extract block of 256, and whole blocks were never seen (no crossing there)
    n0 = 86 * 70 * 66
    assert n0 % 256 and (83 * 66 * 67) % 256 and bool((w[:n0 // 256 * 256].view(-1, 256).max(1).values == 0).any())
    pd2, psd2 = ops.tsdf_extract(Dd, wd, vs, origin, dims, S.VOXEL, min_weight=2.0)
    ph2, psh2 = ops.tsdf_extract_host(D, w, None, origin, dims, S.VOXEL, min_weight=2.0)
    assert psd2.tolist() == psh2.tolist() and same_bits(pd2, ph2) and 0 < int(psh2[-1]) < int(ps[-1])


@pytest.mark.parametrize("name", sorted(S.small_cases()))
def test_device_equals_host_twin_on_small_volumes(name):
    case = S.small_cases()[name]
    assert same_bits(ops.tsdf_bounds(**S.bounds_args(case)), ops.tsdf_bounds_host(**S.bounds_args(case)))
    Dh, wh, vsh = ops.tsdf_integrate_host(**S.integrate_args(case))
    Dd, wd, vsd = ops.tsdf_integrate(**S.integrate_args(case))
    assert same_bits(Dd, Dh) and same_bits(wd, wh) and vsd.tolist() == vsh.tolist()
    ph, psh = ops.tsdf_extract_host(Dh, wh, vsh, **S.extract_args(case))
    pd, psd = ops.tsdf_extract(Dd, wd, vsd, **S.extract_args(case))
    assert psd.tolist() == psh.tolist() and same_bits(pd, ph)
    assert (int(psh[-1]) == 0) == (name in ('zero_frames', 'behind_camera'))


def test_a_batch_equals_its_volumes_alone_and_itself(scene_host):
    """Three volumes with 6, 0 and 1 frames and different dims in one launch."""
    (depth, fs, K, M, C), bounds, origin, dims, D, w, pts, ps = scene_host
    o3 = np.array([origin[0], [0.1, -0.2, 0.4], origin[1]], dtype=np.float32)
    n3 = np.array([dims[0], [13, 9, 7], dims[1]])
    voxel3 = [S.VOXEL, 0.03, S.VOXEL]
    trunc3 = [S.TRUNC, 0.09, S.TRUNC]
    Db, wb, vsb = ops.tsdf_integrate(depth[:7], [0, 6, 6, 7], K, M[:7], o3, n3, voxel3, trunc3)
    pb, psb = ops.tsdf_extract(Db, wb, vsb, o3, n3, voxel3)
    vs = vsb.tolist()
    for run in range(2):                                       # from run to run
        Dr, wr, _ = ops.tsdf_integrate(depth[:7], [0, 6, 6, 7], K, M[:7], o3, n3, voxel3, trunc3)
        pr, psr = ops.tsdf_extract(Dr, wr, vsb, o3, n3, voxel3)
        assert same_bits(Dr, Db) and same_bits(wr, wb) and same_bits(pr, pb) and psr.tolist() == psb.tolist()
    alone = [(depth[:6], [0, 6], M[:6]), (depth[:0], [0, 0], M[:0]), (depth[6:7], [0, 1], M[6:7])]
    for v, (d, f, m) in enumerate(alone):
        Da, wa, vsa = ops.tsdf_integrate(d, f, K, m, o3[v:v + 1], n3[v:v + 1], voxel3[v], trunc3[v])
        assert same_bits(Da, Db[vs[v]:vs[v + 1]]) and same_bits(wa, wb[vs[v]:vs[v + 1]])
        pa, psa = ops.tsdf_extract(Da, wa, vsa, o3[v:v + 1], n3[v:v + 1], voxel3[v])
        assert same_bits(pa, pb[int(psb[v]):int(psb[v + 1])]) and int(psa[1]) == int(psb[v + 1] - psb[v])
    assert same_bits(Db[:vs[1]], D[:vs[1]])                    # the first volume is fragment 0
    assert not Db[vs[1]:vs[2]].any() and not wb[vs[1]:vs[2]].any() and int(psb[1]) == int(psb[2])
    assert float(wb[vs[2]:].max()) == 1.0 and int(psb[3]) > int(psb[2])


def test_capacity_sets_the_overflow_bit(scene_host):
    (depth, fs, K, M, C), bounds, origin, dims, D, w, pts, ps = scene_host
    cap = 1000
    Dd, wd = D.cuda(), w.cuda()
    p, s, status = ops.tsdf_extract(Dd, wd, None, origin, dims, S.VOXEL, capacity=cap, return_status=True)
    assert int(status.item()) == ops.TSDF_ST_OVERFLOW and s.tolist() == ps.tolist()
    assert tuple(p.shape) == (cap, 3) and same_bits(p, pts[:cap])
    p, s, status = ops.tsdf_extract(Dd, wd, None, origin, dims, S.VOXEL, capacity=int(ps[-1]), return_status=True)
    assert int(status.item()) == 0 and same_bits(p, pts) and s.tolist() == ps.tolist()


def test_capacity_is_enforced_inside_a_larger_buffer(scene_host):
    """The raw entry point with a capacity smaller than the buffer: the rows past the capacity keep their content."""
    from d3feat_pytorch_amd import _native
    (depth, fs, K, M, C), bounds, origin, dims, D, w, pts, ps = scene_host
    dev = torch.device('cuda')
    Dd, wd, V, total, to, tn, tvx, tvs = ops._tsdf_extract_inputs(D, w, origin, dims, S.VOXEL, dev)
    L = _native.lib()
    nbytes = L.d3f_tsdf_extract_ws_bytes(total)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    cap, rows = 777, 2000
    points = torch.full((rows, 3), -7.0, device=dev)
    point_start = torch.zeros(V + 1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = L.d3f_tsdf_extract(Dd.data_ptr(), wd.data_ptr(), tvs.data_ptr(), to.data_ptr(), tn.data_ptr(), tvx.data_ptr(),
                            V, total, 1.0, 0, cap, points.data_ptr(), point_start.data_ptr(), status.data_ptr(),
                            ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert int(status.item()) == ops.TSDF_ST_OVERFLOW and point_start.tolist() == ps.tolist()
    assert same_bits(points[:cap], pts[:cap]) and bool((points[cap:] == -7.0).all())


def test_uint16_and_f32_depth_give_the_same_volume(scene_host):
    (depth, fs, K, M, C), bounds, origin, dims, D, w, pts, ps = scene_host
    metres = depth.astype(np.float32) / np.float32(1000.0)
    assert same_bits(ops.tsdf_bounds(metres, fs, K, C), bounds)
    Dd, wd, _ = ops.tsdf_integrate(metres, fs, K, M, origin, dims, S.VOXEL, S.TRUNC)
    assert same_bits(Dd, D) and same_bits(wd, w)


def test_fuse_fragments_on_the_device_equals_the_cpu_path():
    depth, K, poses = S.sequence()
    kw = dict(frames_per_fragment=S.PER_FRAGMENT, voxel=S.VOXEL, trunc=S.TRUNC)
    cpu, poses_cpu = fr.fuse_fragments(depth, K, poses, device='cpu', **kw)
    gpu, poses_gpu = fr.fuse_fragments(depth, K, poses, device='cuda', **kw)
    assert len(gpu) == 2 and all(same_bits(a, b) for a, b in zip(gpu, cpu)) and np.array_equal(poses_cpu, poses_gpu)
    split = fr.fuse_fragments(depth, K, poses, device='cuda', max_bytes=8 * 86 * 70 * 66, **kw)[0]   # one per launch
    assert all(same_bits(a, b) for a, b in zip(split, cpu))
    with pytest.raises(ValueError, match="86 x 70 x 66"):
        fr.fuse_fragments(depth, K, poses, device='cuda', max_bytes=1 << 20, **kw)
    scene_cpu = fr.fuse_scene(depth, K, poses, poses_cpu, S.PER_FRAGMENT, S.VOXEL, trunc=S.TRUNC, device='cpu')
    scene_gpu = fr.fuse_scene(depth, K, poses, poses_cpu, S.PER_FRAGMENT, S.VOXEL, trunc=S.TRUNC, device='cuda')
    assert same_bits(scene_gpu, scene_cpu) and S.surface_distance(scene_gpu).max() <= 1.0 * S.VOXEL
    # the fragments enter the pipeline: the device miner keeps the pair at the project's threshold
    _, corr, overlap = pp.mine_scene(gpu, poses_gpu, 0.03, min_overlap=0.3, device='cuda', return_overlap=True)
    assert list(corr) == [(0, 1)] and overlap[(0, 1)] > 0.3
