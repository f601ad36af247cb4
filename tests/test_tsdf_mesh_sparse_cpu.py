"""CPU: the sparse mesh (csrc/tsdf_mesh_sparse.hpp) by its host twin and its NumPy restatement -- both in order, bit
for bit, and against ``tsdf_mesh_numpy`` of the densified pool up to order -- on hand-made pools (an absent neighbour,
a sphere through a brick corner, a deleted brick, more than one scan group), every integrated small case, batches with
a volume without bricks, the room, the capacity rule and the front end (``mesh_fragments`` / ``mesh_scene``)."""
import numpy as np
import pytest

from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.datasets import fragments as fr
import tsdf_mesh_cases as MC
import tsdf_mesh_sparse_cases as P
import tsdf_sparse_cases as SC
import tsdf_scene as S
from test_tsdf_mesh_cpu import _read_ply_mesh


def both(name, min_weight=1.0):
    """(host twin, NumPy) of a named pool, after checking that they agree in order."""
    sv, D, w = P.named(name)
    twin = P.host_mesh(name, min_weight)
    restated = ops.tsdf_mesh_sparse_numpy(D, w, sv, min_weight)
    P.assert_in_order(restated, twin)
    return twin, restated


def test_absent_neighbour_gives_49_vertices_and_72_triangles():
    """The plane between ix = 3 and 4: 7 x 7 active cells and 6 x 6 quads; nothing from ix = 7, whose cells reach the
    absent brick."""
    twin, _ = both('absent')
    assert twin[0].shape == (49, 3) and twin[2].shape == (72, 3)
    assert twin[3].tolist() == [0, 49] and twin[4].tolist() == [0, 72]
    dense = P.dense_mesh(P.named('absent'))
    assert dense[0].shape == (49, 3) and dense[2].shape == (72, 3)
    P.assert_up_to_order(twin, dense)
    assert np.array_equal(twin[1], np.tile(np.float32([1.0, 0.0, 0.0]), (49, 1)))     # towards positive D


def test_sphere_through_a_brick_corner_is_closed():
    """The dense restatement, which predates the sparse mesh, gives this sphere 376 vertices and 748 triangles (a closed
    surface of genus 0: V = F / 2 + 2); the counts are its, not the code's under test.  The sparse mesh must have the
    same, every undirected edge twice, every directed edge once, Euler 2."""
    sv, D, w = P.sphere_pool()
    assert sv.bricks == 8
    twin, _ = both('sphere')
    dense = P.dense_mesh((sv, D, w))
    for mesh in (dense, twin):
        assert mesh[0].shape == P.SPHERE_COUNTS[0] and mesh[2].shape == P.SPHERE_COUNTS[1]
        u_mult, d_mult = MC.edge_counts(mesh[2])
        assert (u_mult == 2).all() and (d_mult == 1).all()
        assert MC.euler(mesh[0], mesh[2]) == 2
    P.assert_up_to_order(twin, dense)
    # its quads take cells from several bricks: some face joins vertices of 4 different pool rows
    rows = P.vertex_rows((sv, D, w))
    assert rows.size == twin[0].shape[0]
    per_face = np.sort(rows[twin[2]], axis=1)
    assert (np.diff(per_face, axis=1) != 0).all(axis=1).any()                 # 3 rows in one triangle
    quads = np.concatenate([rows[twin[2][0::2]], rows[twin[2][1::2]]], axis=1)
    assert max(np.unique(q).size for q in quads) == 4


def test_a_deleted_brick_leaves_a_boundary():
    pool = P.named('sphere_less')
    assert pool[0].bricks == 7 and int(pool[0].brick_index[5]) == -1
    twin, _ = both('sphere_less')
    dense = P.dense_mesh(pool)
    P.assert_up_to_order(twin, dense)
    full = P.host_mesh('sphere')
    assert 0 < twin[2].shape[0] < full[2].shape[0] and 0 < twin[0].shape[0] < full[0].shape[0]
    u_mult, d_mult = MC.edge_counts(twin[2])
    assert (u_mult == 1).any() and u_mult.max() == 2 and (d_mult == 1).all()  # a boundary, and still oriented


@pytest.mark.parametrize("name", sorted(SC.cases()))
def test_integrated_cases_equal_the_dense_meshes(name):
    """Edge bricks and odd sizes: against the densified pool, and against the mesh of the densely integrated volume."""
    sv, D, w = P.integrated(name)
    twin, _ = both(name)
    P.assert_up_to_order(twin, P.dense_mesh((sv, D, w)))
    case = SC.cases()[name]
    Dd, wd, vs = ops.tsdf_numpy(**S.integrate_args(case))
    P.assert_up_to_order(twin, ops.tsdf_mesh_numpy(Dd, wd, vs, [case['origin']], [case['dims']], case['voxel']))
    if name in ('dims_1x5x5', 'dims_5x1x1', 'zero_frames', 'behind_camera'):
        assert twin[0].shape == (0, 3) and twin[2].shape == (0, 3)
    else:
        assert twin[0].shape[0] > 0
    if name in ('zero_frames', 'behind_camera'):
        assert sv.bricks == 0
    if name == 'partly_outside':
        assert sv.bricks == 6 and int(sv.lattice_start[-1]) == 48


@pytest.mark.parametrize("name", ['batch_' + k for k in sorted(SC.EMPTY_BETWEEN)])
def test_batches_with_a_volume_without_bricks(name):
    pool = P.integrated(name)
    sv = pool[0]
    assert np.diff(sv.brick_start)[1] == 0 and np.diff(sv.brick_start)[0] > 0 and np.diff(sv.brick_start)[2] > 0
    twin, _ = both(name)
    v, n, f, vs, fs = twin
    assert vs[1] == vs[2] and fs[1] == fs[2] and vs[3] > vs[2] > 0 and fs[3] > fs[2] > 0
    P.assert_up_to_order(twin, P.dense_mesh(pool))
    for k in range(3):                                       # the faces are local: the slices compare directly
        one, Dk, wk = P.volume_of(pool, k)
        alone = [P.host(a) for a in ops.tsdf_mesh_sparse_host(Dk, wk, one)]
        P.assert_in_order(alone, (v[vs[k]:vs[k + 1]], n[vs[k]:vs[k + 1]], f[fs[k]:fs[k + 1]],
                                  np.array([0, vs[k + 1] - vs[k]]), np.array([0, fs[k + 1] - fs[k]])))
        P.assert_in_order(ops.tsdf_mesh_sparse_numpy(Dk, wk, one), alone)


@pytest.mark.parametrize("mw", [1.0, 2.0])
def test_the_room_has_the_dense_counts(mw):
    sv = P.integrated('room')[0]
    assert sv.bricks == 663
    twin, _ = both('room', mw)
    assert twin[3].tolist() == P.ROOM_COUNTS[mw][0] and twin[4].tolist() == P.ROOM_COUNTS[mw][1]
    P.assert_up_to_order(twin, P.dense_mesh(P.integrated('room'), mw))
    P.assert_up_to_order(twin, ops.tsdf_mesh_numpy(min_weight=mw, **MC.room()))      # the densely integrated volumes
    P.assert_in_order(ops.tsdf_mesh_sparse_host(*P.integrated('room')[1:], sv, mw), twin)          # from run to run


def test_more_than_one_scan_group():
    sv, D, w = P.plane_pool()
    assert sv.bricks == 1296 > 1100
    twin, _ = both('plane')
    P.assert_up_to_order(twin, P.dense_mesh((sv, D, w)))
    rows = P.vertex_rows((sv, D, w))                                          # vertices come in pool-row order
    assert rows.size == twin[0].shape[0] and (rows >= 0).all()
    assert (rows < 1024).any() and (rows >= 1024).any()
    face_rows = rows[twin[2]]
    assert (face_rows.max(axis=1) < 1024).any() and (face_rows.min(axis=1) >= 1024).any()
    assert ((face_rows.min(axis=1) < 1024) & (face_rows.max(axis=1) >= 1024)).any()   # a quad that straddles row 1024
    # NumPy in chunks that split the rows differently gives the same
    P.assert_in_order(ops.tsdf_mesh_sparse_numpy(D, w, sv, chunk=500), twin)


def raw_host(pool, vcap, fcap, rows, min_weight=1.0):
    """d3f_tsdf_sparse_mesh_host with capacities smaller than its buffers of ``rows`` rows, which hold -7."""
    import torch
    from d3feat_pytorch_amd import _native
    sv, D, w = pool
    cpu = torch.device('cpu')
    Dt, wt = ops._sparse_pool(D, w, sv, cpu)
    tls, bs, bi, bc, to, tn, tvx = ops._sparse_tables(sv, cpu)
    V = sv.volumes
    vertices, normals = torch.full((rows, 3), -7.0), torch.full((rows, 3), -7.0)
    faces = torch.full((rows, 3), -7, dtype=torch.int32)
    vs, fs = torch.zeros(V + 1, dtype=torch.int64), torch.zeros(V + 1, dtype=torch.int64)
    status = torch.zeros(1, dtype=torch.int32)
    rc = _native.lib().d3f_tsdf_sparse_mesh_host(
        Dt.data_ptr(), wt.data_ptr(), tls.data_ptr(), bs.data_ptr(), bi.data_ptr(), bc.data_ptr(), to.data_ptr(),
        tn.data_ptr(), tvx.data_ptr(), V, int(sv.lattice_start[-1]), sv.bricks, min_weight, vcap, fcap,
        vertices.data_ptr(), normals.data_ptr(), faces.data_ptr(), vs.data_ptr(), fs.data_ptr(), status.data_ptr())
    assert rc == 0
    return vertices, normals, faces, vs, fs, int(status.item())


@pytest.mark.parametrize("vcap,fcap", [(0, 0), (777, 1555), (11562, 1001), (1000, 20976), (11562, 20976)])
def test_capacities(vcap, fcap):
    v, n, f, vs, fs = P.host_mesh('room')
    nv, nf = int(vs[-1]), int(fs[-1])
    vertices, normals, faces, gvs, gfs, status = raw_host(P.integrated('room'), vcap, fcap, 25000)
    assert status == (ops.TSDF_ST_OVERFLOW if vcap < nv else 0) | (ops.TSDF_ST_FACE_OVERFLOW if fcap < nf else 0)
    P.assert_in_order((vertices[:vcap], normals[:vcap], faces[:fcap], gvs, gfs), (v[:vcap], n[:vcap], f[:fcap], vs, fs))
    assert bool((vertices[vcap:] == -7.0).all()) and bool((normals[vcap:] == -7.0).all())
    assert bool((faces[fcap:] == -7).all())                        # an odd capacity cuts a quad in two
    # the wrapper: exactly the rows asked for
    sv, D, w = P.integrated('room')
    out = ops.tsdf_mesh_sparse_host(D, w, sv, vertex_capacity=vcap, face_capacity=fcap, return_status=True)
    assert int(out[5]) == status
    P.assert_in_order(out[:5], (v[:vcap], n[:vcap], f[:fcap], vs, fs))


def test_bytes_accounting():
    assert ops.tsdf_mesh_sparse_bytes(10, 100, 200, 48) == 16 * 512 * 10 + 8 * 48 + 64 * 10 + 24 * 100 + 12 * 200


# ------------------------------------------------------------------------------------------------------ front end
@pytest.fixture(scope="module")
def fragments_cpu():
    depth, K, poses = S.sequence()
    kw = dict(frames_per_fragment=S.PER_FRAGMENT, voxel=S.VOXEL, trunc=S.TRUNC, device='cpu')
    return fr.mesh_fragments(depth, K, poses, **kw), kw


def test_mesh_fragments_equal_the_dense_front_end(fragments_cpu):
    (clouds, poses_out, meshes), kw = fragments_cpu
    depth, K, poses = S.sequence()
    dense_clouds, dense_poses, dense_meshes = fr.fuse_fragments(depth, K, poses, mesh=True, **kw)
    sparse_clouds, sparse_poses = fr.fuse_fragments(depth, K, poses, sparse=True, **kw)
    assert len(clouds) == len(meshes) == 2 and np.array_equal(poses_out, dense_poses)
    for a, b in zip(clouds, sparse_clouds):
        assert SC.same_bits(a, b)
    for m, d in zip(meshes, dense_meshes):
        assert len(m) == 3 and m[0].shape[0] > 0 and m[2].shape[0] > 0 and m[2].dtype == np.int32
        P.assert_up_to_order(m + (np.array([0, m[0].shape[0]]), np.array([0, m[2].shape[0]])),
                             d + (np.array([0, d[0].shape[0]]), np.array([0, d[2].shape[0]])))
    assert [m[0].shape[0] for m in meshes] == np.diff(P.ROOM_COUNTS[1.0][0]).tolist()


def test_mesh_scene_equals_the_dense_front_end(fragments_cpu):
    (_, fragment_poses, _), kw = fragments_cpu
    depth, K, poses = S.sequence()
    skw = dict(trunc=S.TRUNC, device='cpu')
    cloud, mesh = fr.mesh_scene(depth, K, poses, fragment_poses, S.PER_FRAGMENT, S.VOXEL, **skw)
    dense_cloud, dense = fr.fuse_scene(depth, K, poses, fragment_poses, S.PER_FRAGMENT, S.VOXEL, mesh=True, **skw)
    assert SC.same_bits(cloud, fr.fuse_scene(depth, K, poses, fragment_poses, S.PER_FRAGMENT, S.VOXEL, sparse=True, **skw))
    assert mesh[0].shape[0] > 0 and mesh[2].shape[0] > 0
    P.assert_up_to_order(mesh + (np.array([0, mesh[0].shape[0]]), np.array([0, mesh[2].shape[0]])),
                         dense + (np.array([0, dense[0].shape[0]]), np.array([0, dense[2].shape[0]])))


def test_mesh_scene_without_a_finite_pose_is_empty(fragments_cpu):
    (_, fragment_poses, _), _ = fragments_cpu
    depth, K, poses = S.sequence()
    cloud, (v, n, f) = fr.mesh_scene(depth, K, poses, np.full_like(fragment_poses, np.nan), S.PER_FRAGMENT, S.VOXEL,
                                     device='cpu')
    assert cloud.shape == v.shape == n.shape == (0, 3) and cloud.dtype == v.dtype == np.float32
    assert f.shape == (0, 3) and f.dtype == np.int32
    clouds, poses_out, meshes = fr.mesh_fragments(depth[:0], K, poses[:0], device='cpu')
    assert clouds == [] and meshes == [] and poses_out.shape == (0, 4, 4)


def test_sparse_mesh_writes_a_ply(tmp_path, fragments_cpu):
    (_, _, meshes), _ = fragments_cpu
    v, n, f = meshes[0]
    path = str(tmp_path / 'fragment.ply')
    fr.write_ply_mesh(path, v, f, normals=n)
    names, vert, faces = _read_ply_mesh(path)
    assert names == ['x', 'y', 'z', 'nx', 'ny', 'nz']
    assert SC.same_bits(np.ascontiguousarray(vert[:, :3]), v) and SC.same_bits(np.ascontiguousarray(vert[:, 3:]), n)
    assert np.array_equal(faces.astype(np.int32), f)


def test_the_fuse_entry_points_name_the_new_functions():
    depth, K, poses = S.sequence()
    with pytest.raises(ValueError, match="sparse=True gives no mesh.*mesh_fragments"):
        fr.fuse_fragments(depth, K, poses, sparse=True, mesh=True, device='cpu')
