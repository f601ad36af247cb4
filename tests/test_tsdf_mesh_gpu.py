"""GPU: the mesh kernels (csrc/tsdf_mesh.hip) against their host twin bit for bit, through the C ABI -- the room's two
volumes in one batch (face look-ups across blocks, scan groups and the volume boundary inside a block), every small
volume, batches against single volumes and from run to run, the capacity rule, and ``fuse_fragments`` / ``fuse_scene``
with ``mesh=True`` on the device against the CPU path."""
import numpy as np
import pytest
import torch

from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.datasets import fragments as fr
import tsdf_mesh_cases as MC
import tsdf_scene as S

pytestmark = pytest.mark.gpu

PARTS = ("vertices", "normals", "faces", "vertex_start", "face_start")


def same(a, b):
    """Equal dtype, shape and bits (f32 compared as words)."""
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    if a.dtype == np.float32 and b.dtype == np.float32:
        a, b = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


def assert_same_mesh(got, want):
    for g, w_, what in zip(got, want, PARTS):
        assert same(g, w_), what


@pytest.fixture(scope="module")
def room_host():
    """min_weight -> the host twin's mesh of the room's two volumes; computed once."""
    return {mw: ops.tsdf_mesh_host(min_weight=mw, **MC.room()) for mw in (1.0, 2.0)}


@pytest.mark.parametrize("mw", [1.0, 2.0])
def test_device_equals_host_twin_on_the_room(room_host, mw):
    args = MC.room()
    counts = np.diff(args['vol_start']).tolist()
    assert counts == [397320, 367026] and all(c % 256 for c in counts) and sum(counts) > 2 * 1024 * 256
    got = ops.tsdf_mesh(min_weight=mw, **args)
    assert all(t.is_cuda for t in got)
    want = room_host[mw]
    assert_same_mesh(got, want)
    assert int(want[3][1]) > 0 and int(want[3][2]) > int(want[3][1]) and int(want[4][2]) > int(want[4][1]) > 0
    if mw == 2.0:
        assert int(want[3][2]) < int(room_host[1.0][3][2])


@pytest.mark.parametrize("name", sorted(S.small_cases()))
def test_device_equals_host_twin_on_small_volumes(name):
    args = MC.small(name)
    want = ops.tsdf_mesh_host(**args)
    assert_same_mesh(ops.tsdf_mesh(**args), want)
    assert (int(want[3][-1]) == 0) == (name in ('dims_1x5x5', 'dims_5x1x1', 'zero_frames', 'behind_camera'))


def test_a_batch_equals_its_volumes_alone_and_itself():
    """Sphere 24^3, an empty 13 x 9 x 7 volume and the cut sphere 24^3 in one launch."""
    A = MC.analytic()
    parts = [A['sphere'], dict(D=np.full(13 * 9 * 7, 0.5, dtype=np.float32), w=np.ones(13 * 9 * 7, dtype=np.float32),
                               origin=[[0.1, -0.2, 0.4]], dims=[[13, 9, 7]], voxel=0.03), A['cut_sphere']]
    batch = dict(D=np.concatenate([p['D'] for p in parts]), w=np.concatenate([p['w'] for p in parts]), vol_start=None,
                 origin=np.concatenate([p['origin'] for p in parts]), dims=np.concatenate([p['dims'] for p in parts]),
                 voxel=[p['voxel'] for p in parts])
    first = ops.tsdf_mesh(**batch)
    for run in range(2):                                       # from run to run
        assert_same_mesh(ops.tsdf_mesh(**batch), first)
    v, n, f, vs, fs = (t.cpu() for t in first)
    assert int(vs[1]) == int(vs[2]) and int(fs[1]) == int(fs[2]) and int(vs[3]) > int(vs[2]) > 0
    for k, p in enumerate(parts):                              # the faces are local: the slices compare directly
        av, an, af, avs, afs = ops.tsdf_mesh(vol_start=None, **{key: p[key] for key in ('D', 'w', 'origin', 'dims', 'voxel')})
        assert same(av, v[vs[k]:vs[k + 1]]) and same(an, n[vs[k]:vs[k + 1]]) and same(af, f[fs[k]:fs[k + 1]])
        assert avs.tolist() == [0, int(vs[k + 1] - vs[k])] and afs.tolist() == [0, int(fs[k + 1] - fs[k])]
    assert_same_mesh(first, ops.tsdf_mesh_host(**batch))


def test_capacities_set_their_own_status_bits(room_host):
    args = MC.room()
    v, n, f, vs, fs = room_host[1.0]
    nv, nf = int(vs[-1]), int(fs[-1])
    out = ops.tsdf_mesh(vertex_capacity=1000, face_capacity=nf, return_status=True, **args)
    assert int(out[5].item()) == ops.TSDF_ST_OVERFLOW
    assert same(out[0], v[:1000]) and same(out[1], n[:1000]) and same(out[2], f) and same(out[3], vs) and same(out[4], fs)
    out = ops.tsdf_mesh(vertex_capacity=nv, face_capacity=1001, return_status=True, **args)
    assert int(out[5].item()) == ops.TSDF_ST_FACE_OVERFLOW
    assert same(out[0], v) and same(out[1], n) and same(out[2], f[:1001]) and same(out[3], vs) and same(out[4], fs)
    out = ops.tsdf_mesh(vertex_capacity=1000, face_capacity=1001, return_status=True, **args)
    assert int(out[5].item()) == ops.TSDF_ST_OVERFLOW | ops.TSDF_ST_FACE_OVERFLOW
    assert same(out[0], v[:1000]) and same(out[2], f[:1001]) and same(out[3], vs) and same(out[4], fs)
    out = ops.tsdf_mesh(vertex_capacity=nv, face_capacity=nf, return_status=True, **args)
    assert int(out[5].item()) == 0
    assert_same_mesh(out[:5], room_host[1.0])


@pytest.mark.parametrize("counted", [0, 1])
def test_capacities_are_enforced_inside_larger_buffers(room_host, counted):
    """The raw entry point with capacities smaller than the buffers: the rows past a capacity keep their content;
    after d3f_tsdf_mesh_count, counted = 1 gives the same."""
    from d3feat_pytorch_amd import _native
    args = MC.room()
    v, n, f, vs, fs = room_host[1.0]
    dev = torch.device('cuda')
    Dd, wd, V, total, to, tn, tvx, tvs = ops._tsdf_extract_inputs(args['D'], args['w'], args['origin'], args['dims'],
                                                                  args['voxel'], dev)
    L = _native.lib()
    nbytes = L.d3f_tsdf_mesh_ws_bytes(total)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    vcap, fcap, rows = 777, 1555, 3000
    vertices = torch.full((rows, 3), -7.0, device=dev)
    normals = torch.full((rows, 3), -7.0, device=dev)
    faces = torch.full((rows, 3), -7, dtype=torch.int32, device=dev)
    vertex_start = torch.zeros(V + 1, dtype=torch.int64, device=dev)
    face_start = torch.zeros(V + 1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    if counted:
        rc = L.d3f_tsdf_mesh_count(Dd.data_ptr(), wd.data_ptr(), tvs.data_ptr(), tn.data_ptr(), V, total, 1.0,
                                   vertex_start.data_ptr(), face_start.data_ptr(), ws.data_ptr(), nbytes, stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert int(vertex_start[V]) == int(vs[-1]) and int(face_start[V]) == int(fs[-1])
    rc = L.d3f_tsdf_mesh(Dd.data_ptr(), wd.data_ptr(), tvs.data_ptr(), to.data_ptr(), tn.data_ptr(), tvx.data_ptr(), V,
                         total, 1.0, counted, vcap, fcap, vertices.data_ptr(), normals.data_ptr(), faces.data_ptr(),
                         vertex_start.data_ptr(), face_start.data_ptr(), status.data_ptr(), ws.data_ptr(), nbytes, stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert int(status.item()) == ops.TSDF_ST_OVERFLOW | ops.TSDF_ST_FACE_OVERFLOW
    assert same(vertex_start, vs) and same(face_start, fs)
    assert same(vertices[:vcap], v[:vcap]) and bool((vertices[vcap:] == -7.0).all())
    assert same(normals[:vcap], n[:vcap]) and bool((normals[vcap:] == -7.0).all())
    assert same(faces[:fcap], f[:fcap]) and bool((faces[fcap:] == -7).all())     # an odd capacity cuts a quad in two


def test_fuse_fragments_and_scene_with_mesh_equal_the_cpu_path():
    depth, K, poses = S.sequence()
    kw = dict(frames_per_fragment=S.PER_FRAGMENT, voxel=S.VOXEL, trunc=S.TRUNC, mesh=True)
    cpu, poses_cpu, mesh_cpu = fr.fuse_fragments(depth, K, poses, device='cpu', **kw)
    gpu, poses_gpu, mesh_gpu = fr.fuse_fragments(depth, K, poses, device='cuda', **kw)
    assert len(gpu) == len(mesh_gpu) == 2 and np.array_equal(poses_cpu, poses_gpu)
    assert all(same(a, b) for a, b in zip(gpu, cpu))
    for a, b in zip(mesh_gpu, mesh_cpu):
        assert len(a) == 3 and a[0].shape[0] > 0 and a[2].shape[0] > 0
        assert same(a[0], b[0]) and same(a[1], b[1]) and same(a[2], b[2])
    skw = dict(trunc=S.TRUNC, mesh=True)
    cloud_cpu, scene_cpu = fr.fuse_scene(depth, K, poses, poses_cpu, S.PER_FRAGMENT, S.VOXEL, device='cpu', **skw)
    cloud_gpu, scene_gpu = fr.fuse_scene(depth, K, poses, poses_cpu, S.PER_FRAGMENT, S.VOXEL, device='cuda', **skw)
    assert same(cloud_gpu, cloud_cpu) and scene_gpu[0].shape[0] > 0
    assert same(scene_gpu[0], scene_cpu[0]) and same(scene_gpu[1], scene_cpu[1]) and same(scene_gpu[2], scene_cpu[2])
