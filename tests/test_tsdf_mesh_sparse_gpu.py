"""GPU: the sparse mesh kernels (csrc/tsdf_mesh_sparse.hip) against their host twin in order, bit for bit, and against
``tsdf_mesh_numpy`` of the densified pool up to order -- hand-made pools (an absent neighbour, a sphere through a brick
corner, a deleted brick, more than one scan group), every integrated small case, batches with a volume without bricks,
the room from run to run, the capacity rule with guard rows, and ``mesh_fragments`` / ``mesh_scene`` on the device
against the CPU path."""
import numpy as np
import pytest
import torch

from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.datasets import fragments as fr
import tsdf_mesh_cases as MC
import tsdf_mesh_sparse_cases as P
import tsdf_sparse_cases as SC
import tsdf_scene as S

pytestmark = pytest.mark.gpu


def device_mesh(name, min_weight=1.0, **kw):
    sv, D, w = P.named(name)
    got = ops.tsdf_mesh_sparse(D, w, sv, min_weight, **kw)
    assert all(t.is_cuda for t in got)
    return got


def test_absent_neighbour_gives_49_vertices_and_72_triangles():
    got = device_mesh('absent')
    assert tuple(got[0].shape) == (49, 3) and tuple(got[2].shape) == (72, 3)
    P.assert_in_order(got, P.host_mesh('absent'))
    P.assert_up_to_order(got, P.dense_mesh(P.named('absent')))


def test_sphere_through_a_brick_corner_is_closed():
    got = [P.host(t) for t in device_mesh('sphere')]
    assert got[0].shape == P.SPHERE_COUNTS[0] and got[2].shape == P.SPHERE_COUNTS[1]
    u_mult, d_mult = MC.edge_counts(got[2])
    assert (u_mult == 2).all() and (d_mult == 1).all() and MC.euler(got[0], got[2]) == 2
    P.assert_in_order(got, P.host_mesh('sphere'))
    P.assert_up_to_order(got, P.dense_mesh(P.sphere_pool()))


def test_a_deleted_brick_leaves_a_boundary():
    got = [P.host(t) for t in device_mesh('sphere_less')]
    P.assert_in_order(got, P.host_mesh('sphere_less'))
    P.assert_up_to_order(got, P.dense_mesh(P.named('sphere_less')))
    u_mult, _ = MC.edge_counts(got[2])
    assert (u_mult == 1).any() and 0 < got[2].shape[0] < P.SPHERE_COUNTS[1][0]


@pytest.mark.parametrize("name", sorted(SC.cases()))
def test_integrated_cases_equal_the_host_twin_and_the_dense_meshes(name):
    """Allocated and integrated on the device: against the host twin in order, the densified pool and the densely
    integrated volume up to order."""
    case = SC.cases()[name]
    sv = ops.tsdf_allocate(**SC.allocate_args(case))
    D, w = ops.tsdf_integrate_sparse(**SC.sparse_args(case, sv))
    got = ops.tsdf_mesh_sparse(D, w, sv)
    assert SC.same_tables(sv, P.integrated(name)[0])
    P.assert_in_order(got, P.host_mesh(name))
    P.assert_up_to_order(got, P.dense_mesh((sv, D, w)))
    Dd, wd, vs = ops.tsdf_numpy(**S.integrate_args(case))
    P.assert_up_to_order(got, ops.tsdf_mesh_numpy(Dd, wd, vs, [case['origin']], [case['dims']], case['voxel']))
    assert (int(got[3][-1]) == 0) == (name in ('dims_1x5x5', 'dims_5x1x1', 'zero_frames', 'behind_camera'))


@pytest.mark.parametrize("name", ['batch_' + k for k in sorted(SC.EMPTY_BETWEEN)])
def test_batches_with_a_volume_without_bricks(name):
    pool = P.integrated(name)
    got = device_mesh(name)
    P.assert_in_order(got, P.host_mesh(name))
    v, n, f, vs, fs = (P.host(t) for t in got)
    assert vs[0] == 0 and vs[1] == vs[2] and fs[1] == fs[2] and vs[3] > vs[2] > 0 and fs[3] > fs[2] > 0
    P.assert_up_to_order(got, P.dense_mesh(pool))
    for k in range(3):                                       # the faces are local: the slices compare directly
        one, Dk, wk = P.volume_of(pool, k)
        alone = ops.tsdf_mesh_sparse(Dk, wk, one)
        P.assert_in_order(alone, (v[vs[k]:vs[k + 1]], n[vs[k]:vs[k + 1]], f[fs[k]:fs[k + 1]],
                                  np.array([0, vs[k + 1] - vs[k]]), np.array([0, fs[k + 1] - fs[k]])))


@pytest.mark.parametrize("mw", [1.0, 2.0])
def test_the_room_in_one_call(mw):
    got = device_mesh('room', mw)
    assert got[3].tolist() == P.ROOM_COUNTS[mw][0] and got[4].tolist() == P.ROOM_COUNTS[mw][1]
    P.assert_in_order(got, P.host_mesh('room', mw))
    P.assert_up_to_order(got, P.dense_mesh(P.integrated('room'), mw))
    for run in range(2):                                     # from run to run
        P.assert_in_order(device_mesh('room', mw), got)


def test_more_than_one_scan_group():
    pool = P.plane_pool()
    assert pool[0].bricks == 1296
    got = [P.host(t) for t in device_mesh('plane')]
    P.assert_in_order(got, P.host_mesh('plane'))
    P.assert_up_to_order(got, P.dense_mesh(pool))
    rows = P.vertex_rows(pool)
    assert rows.size == got[0].shape[0] and (rows < 1024).any() and (rows >= 1024).any()
    face_rows = rows[got[2]]
    assert (face_rows.max(axis=1) < 1024).any() and (face_rows.min(axis=1) >= 1024).any()
    assert ((face_rows.min(axis=1) < 1024) & (face_rows.max(axis=1) >= 1024)).any()   # a quad that straddles row 1024


@pytest.mark.parametrize("vcap,fcap", [(0, 0), (1000, 20976), (11562, 1001), (777, 1555), (11562, 20976)])
def test_capacities_set_their_own_status_bits(vcap, fcap):
    v, n, f, vs, fs = P.host_mesh('room')
    out = device_mesh('room', vertex_capacity=vcap, face_capacity=fcap, return_status=True)
    want = (ops.TSDF_ST_OVERFLOW if vcap < vs[-1] else 0) | (ops.TSDF_ST_FACE_OVERFLOW if fcap < fs[-1] else 0)
    assert int(out[5].item()) == want
    P.assert_in_order(out[:5], (v[:vcap], n[:vcap], f[:fcap], vs, fs))


@pytest.mark.parametrize("counted", [0, 1])
def test_capacities_are_enforced_inside_larger_buffers(counted):
    """The raw entry point with capacities smaller than the buffers: the rows past a capacity keep their content;
    after d3f_tsdf_sparse_mesh_count, counted = 1 gives the same."""
    from d3feat_pytorch_amd import _native
    sv, D, w = P.integrated('room')
    v, n, f, vs, fs = P.host_mesh('room')
    dev = torch.device('cuda')
    Dd, wd = ops._sparse_pool(D, w, sv, dev)
    tls, bs, bi, bc, to, tn, tvx = ops._sparse_tables(sv, dev)
    V, lattice, B = sv.volumes, int(sv.lattice_start[-1]), sv.bricks
    L = _native.lib()
    nbytes = L.d3f_tsdf_sparse_mesh_ws_bytes(B)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    vcap, fcap, rows = 777, 1555, 3000
    vertices = torch.full((rows, 3), -7.0, device=dev)
    normals = torch.full((rows, 3), -7.0, device=dev)
    faces = torch.full((rows, 3), -7, dtype=torch.int32, device=dev)
    vertex_start = torch.zeros(V + 1, dtype=torch.int64, device=dev)
    face_start = torch.zeros(V + 1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    tables = (Dd.data_ptr(), wd.data_ptr(), tls.data_ptr(), bs.data_ptr(), bi.data_ptr(), bc.data_ptr())
    if counted:
        rc = L.d3f_tsdf_sparse_mesh_count(*tables, tn.data_ptr(), V, lattice, B, 1.0, vertex_start.data_ptr(),
                                          face_start.data_ptr(), ws.data_ptr(), nbytes, stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert vertex_start.tolist() == vs.tolist() and face_start.tolist() == fs.tolist()
    rc = L.d3f_tsdf_sparse_mesh(*tables, to.data_ptr(), tn.data_ptr(), tvx.data_ptr(), V, lattice, B, 1.0, counted, vcap,
                                fcap, vertices.data_ptr(), normals.data_ptr(), faces.data_ptr(), vertex_start.data_ptr(),
                                face_start.data_ptr(), status.data_ptr(), ws.data_ptr(), nbytes, stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert int(status.item()) == ops.TSDF_ST_OVERFLOW | ops.TSDF_ST_FACE_OVERFLOW
    P.assert_in_order((vertices[:vcap], normals[:vcap], faces[:fcap], vertex_start, face_start),
                      (v[:vcap], n[:vcap], f[:fcap], vs, fs))
    assert bool((vertices[vcap:] == -7.0).all()) and bool((normals[vcap:] == -7.0).all())
    assert bool((faces[fcap:] == -7).all())                  # an odd capacity cuts a quad in two


def test_no_bricks_launch_nothing():
    sv, D, w = P.integrated('zero_frames')
    assert sv.bricks == 0
    out = ops.tsdf_mesh_sparse(D, w, sv, return_status=True)
    assert tuple(out[0].shape) == (0, 3) and tuple(out[2].shape) == (0, 3) and out[2].dtype == torch.int32
    assert out[3].tolist() == [0, 0] and out[4].tolist() == [0, 0] and int(out[5].item()) == 0


def _as_batch(mesh):
    return tuple(mesh) + (np.array([0, mesh[0].shape[0]]), np.array([0, mesh[2].shape[0]]))


def test_mesh_fragments_and_scene_equal_the_cpu_path_and_the_dense_front_end():
    depth, K, poses = S.sequence()
    kw = dict(frames_per_fragment=S.PER_FRAGMENT, voxel=S.VOXEL, trunc=S.TRUNC)
    cpu, poses_cpu, mesh_cpu = fr.mesh_fragments(depth, K, poses, device='cpu', **kw)
    gpu, poses_gpu, mesh_gpu = fr.mesh_fragments(depth, K, poses, device='cuda', **kw)
    sparse, _ = fr.fuse_fragments(depth, K, poses, device='cuda', sparse=True, **kw)
    _, _, dense = fr.fuse_fragments(depth, K, poses, device='cuda', mesh=True, **kw)
    assert len(gpu) == len(mesh_gpu) == 2 and np.array_equal(poses_cpu, poses_gpu)
    assert all(SC.same_bits(a, b) for a, b in zip(gpu, cpu)) and all(SC.same_bits(a, b) for a, b in zip(gpu, sparse))
    for a, b, d in zip(mesh_gpu, mesh_cpu, dense):
        assert len(a) == 3 and a[0].shape[0] > 0 and a[2].shape[0] > 0
        P.assert_in_order(a, b)
        P.assert_up_to_order(_as_batch(a), _as_batch(d))
    skw = dict(trunc=S.TRUNC)
    cloud_cpu, scene_cpu = fr.mesh_scene(depth, K, poses, poses_cpu, S.PER_FRAGMENT, S.VOXEL, device='cpu', **skw)
    cloud_gpu, scene_gpu = fr.mesh_scene(depth, K, poses, poses_cpu, S.PER_FRAGMENT, S.VOXEL, device='cuda', **skw)
    _, scene_dense = fr.fuse_scene(depth, K, poses, poses_cpu, S.PER_FRAGMENT, S.VOXEL, device='cuda', mesh=True, **skw)
    assert SC.same_bits(cloud_gpu, cloud_cpu) and scene_gpu[0].shape[0] > 0
    assert SC.same_bits(cloud_gpu, fr.fuse_scene(depth, K, poses, poses_cpu, S.PER_FRAGMENT, S.VOXEL, device='cuda',
                                                 sparse=True, **skw))
    P.assert_in_order(scene_gpu, scene_cpu)
    P.assert_up_to_order(_as_batch(scene_gpu), _as_batch(scene_dense))


def test_mesh_front_end_writes_a_ply_and_handles_no_pose(tmp_path):
    from test_tsdf_mesh_cpu import _read_ply_mesh
    depth, K, poses = S.sequence()
    _, fragment_poses, meshes = fr.mesh_fragments(depth, K, poses, frames_per_fragment=S.PER_FRAGMENT, voxel=S.VOXEL,
                                                  trunc=S.TRUNC, device='cuda')
    v, n, f = meshes[1]
    path = str(tmp_path / 'fragment.ply')
    fr.write_ply_mesh(path, v, f, normals=n)
    names, vert, faces = _read_ply_mesh(path)
    assert names == ['x', 'y', 'z', 'nx', 'ny', 'nz']
    assert SC.same_bits(np.ascontiguousarray(vert[:, :3]), v) and SC.same_bits(np.ascontiguousarray(vert[:, 3:]), n)
    assert np.array_equal(faces.astype(np.int32), f)
    cloud, (v, n, f) = fr.mesh_scene(depth, K, poses, np.full_like(fragment_poses, np.nan), S.PER_FRAGMENT, S.VOXEL,
                                     device='cuda')
    assert cloud.shape == v.shape == n.shape == (0, 3) and f.shape == (0, 3) and f.dtype == np.int32
