"""CPU: triangle meshes from TSDF volumes (csrc/tsdf_mesh.hpp) -- the host twin of the kernels against the NumPy
restatement bit for bit, the topology and geometry of the meshes of analytic volumes, the room of ``tsdf_scene``, the
tie to ``tsdf_extract``, and the front end (``fuse_fragments(mesh=True)``, ``write_ply_mesh``)."""
import numpy as np
import pytest

from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.datasets import fragments as fr
from d3feat_pytorch_amd.datasets.ThreeDMatch import read_ply_points
import tsdf_mesh_cases as MC
import tsdf_scene as S

CASES = MC.all_cases()
NAMES = [c[0] for c in CASES]
NO_SURFACE = ('empty', 'dims_1x5x5', 'dims_5x1x1', 'zero_frames', 'behind_camera')


def same(a, b):
    """Equal shape and equal bits (f32 compared as words, so -0 / +0 and NaN payloads count)."""
    a = a.numpy() if hasattr(a, 'numpy') else np.asarray(a)
    b = b.numpy() if hasattr(b, 'numpy') else np.asarray(b)
    if a.dtype == np.float32 and b.dtype == np.float32:
        a, b = np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


@pytest.fixture(scope="module")
def meshes():
    """name -> the mesh by the NumPy restatement; computed once."""
    return {name: ops.tsdf_mesh_numpy(min_weight=mw, **args) for name, args, mw in CASES}


# --------------------------------------------------------------------------------------- host twin == restatement
@pytest.mark.parametrize("name,args,mw", CASES, ids=NAMES)
def test_host_twin_equals_restatement(meshes, name, args, mw):
    got = ops.tsdf_mesh_host(min_weight=mw, **args)
    want = meshes[name]
    assert len(got) == len(want) == 5
    for g, w_, what in zip(got, want, ("vertices", "normals", "faces", "vertex_start", "face_start")):
        assert same(g, w_), what
    assert want[0].dtype == np.float32 and want[1].dtype == np.float32 and want[2].dtype == np.int32
    assert want[3].tolist()[-1] == want[0].shape[0] == want[1].shape[0] and want[4].tolist()[-1] == want[2].shape[0]
    if name in NO_SURFACE:
        assert want[0].shape == (0, 3) and want[1].shape == (0, 3) and want[2].shape == (0, 3)
        assert not want[3].any() and not want[4].any()
    else:
        assert want[0].shape[0] > 0


# ---------------------------------------------------------------------------------------- topology and geometry
def test_sphere_is_a_closed_oriented_surface_near_the_sphere(meshes):
    v, n, f, vs, fs = meshes['sphere']
    u_mult, d_mult = MC.edge_counts(f)
    assert (u_mult == 2).all() and (d_mult == 1).all()
    assert np.unique(f).size == v.shape[0]                                # every vertex is used
    assert v.shape[0] - u_mult.size + f.shape[0] == 2
    p = v.astype(np.float64)
    t0, t1, t2 = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    volume = float(np.einsum('ij,ij->i', t0, np.cross(t1, t2)).sum() / 6.0)
    exact = 4.0 * np.pi * MC.RADIUS ** 3 / 3.0
    print("V %d  E %d  F %d   signed volume %.5f (sphere %.5f, %+.1f %%)"
          % (v.shape[0], u_mult.size, f.shape[0], volume, exact, 100 * (volume / exact - 1)))
    assert volume > 0 and abs(volume / exact - 1) <= 0.05
    radial = p - np.array(MC.CENTER)
    dist = np.linalg.norm(radial, axis=1)
    print("vertex distance to the sphere / voxel: max %.3f" % (np.abs(dist - MC.RADIUS).max() / MC.VOXEL))
    assert np.abs(dist - MC.RADIUS).max() <= 0.25 * MC.VOXEL
    cos = np.einsum('ij,ij->i', n.astype(np.float64), radial / dist[:, None])
    print("vertex normals against the radial direction: max %.2f degrees" % np.degrees(np.arccos(cos.min())))
    assert cos.min() >= np.cos(np.radians(10.0))
    assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    fn = np.cross(t1 - t0, t2 - t0)
    fn /= np.linalg.norm(fn, axis=1)[:, None]
    centroid = (t0 + t1 + t2) / 3.0 - np.array(MC.CENTER)
    fcos = np.einsum('ij,ij->i', fn, centroid / np.linalg.norm(centroid, axis=1)[:, None])
    print("face normals against the radial direction: min cos %.3f" % fcos.min())
    assert fcos.min() > 0.8


def test_torus_is_closed_with_one_handle(meshes):
    v, n, f, vs, fs = meshes['torus']
    u_mult, d_mult = MC.edge_counts(f)
    assert f.shape[0] > 0 and (u_mult == 2).all() and (d_mult == 1).all()
    assert MC.euler(v, f) == 0


@pytest.mark.parametrize("name", ["cut_sphere", "holed_sphere"])
def test_a_cut_surface_is_a_disc(meshes, name):
    v, n, f, vs, fs = meshes[name]
    u_mult, d_mult = MC.edge_counts(f)
    assert set(u_mult.tolist()) == {1, 2}                                 # interior edges and a boundary, nothing else
    assert (d_mult == 1).all()
    assert MC.euler(v, f) == 1


# ------------------------------------------------------------------------------------------------------- the room
def test_room_mesh_lies_on_the_surface(meshes):
    v, n, f, vs, fs = meshes['room_w1']
    depth, K, poses = S.sequence()
    for k, first in enumerate((0, S.PER_FRAGMENT)):
        vk, fk = v[vs[k]:vs[k + 1]], f[fs[k]:fs[k + 1]]
        assert vk.shape[0] > 0 and fk.shape[0] > 0 and fk.shape[0] % 2 == 0
        assert fk.min() >= 0 and fk.max() < vk.shape[0]                   # local to the volume
        dist = S.surface_distance(S.to_world(vk, poses[first]))
        u_mult = MC.edge_counts(fk)[0]
        print("fragment %d: %d vertices, %d faces, max surface distance / voxel %.3f, edge multiplicities %s"
              % (k, vk.shape[0], fk.shape[0], dist.max() / S.VOXEL, np.bincount(u_mult).tolist()))
        assert dist.max() <= 1.0 * S.VOXEL
        assert u_mult.max() <= 4


# ---------------------------------------------------------------------------------------- the tie to tsdf_extract
@pytest.mark.parametrize("name,args,mw", CASES, ids=NAMES)
def test_every_quad_is_an_extracted_point_with_four_complete_cells(meshes, name, args, mw):
    fs = meshes[name][4]
    quads = MC.expected_quads(args['D'], args['w'], args['dims'], mw)
    assert (np.diff(fs) % 2 == 0).all() and (np.diff(fs) // 2).tolist() == quads
    points, ps = ops.tsdf_extract_numpy(args['D'], args['w'], args['vol_start'], args['origin'], args['dims'],
                                        args['voxel'], mw)
    assert (np.asarray(quads) <= np.diff(ps)).all()


def test_vertices_are_means_of_extracted_points():
    """2 x 2 x 2, one corner inside: one cell, three crossing edges, the vertex their mean and the normal (1,1,1)/sqrt 3
    away from the corner; no face, since no edge has four cells."""
    D = np.full(8, 0.5, dtype=np.float32)
    D[0] = -0.5
    args = dict(D=D, w=np.ones(8, np.float32), vol_start=None, origin=[[0, 0, 0]], dims=[[2, 2, 2]], voxel=1.0)
    v, n, f, vs, fs = ops.tsdf_mesh_host(**args)
    third = np.float32(0.5) / np.float32(3.0)
    assert same(v, np.array([[third] * 3], dtype=np.float32)) and f.shape == (0, 3)
    assert np.allclose(n.numpy(), 1 / np.sqrt(3), atol=1e-7) and vs.tolist() == [0, 1] and fs.tolist() == [0, 0]
    for got, want in zip(ops.tsdf_mesh_numpy(**args), (v, n, f, vs, fs)):
        assert same(got, want)


def test_host_capacities_set_their_own_bits(meshes):
    v, n, f, vs, fs = meshes['sphere']
    args = MC.analytic()['sphere']
    out = ops.tsdf_mesh_host(vertex_capacity=100, face_capacity=f.shape[0], return_status=True, **args)
    assert int(out[5]) == ops.TSDF_ST_OVERFLOW and same(out[0], v[:100]) and same(out[1], n[:100]) and same(out[2], f)
    out = ops.tsdf_mesh_host(vertex_capacity=v.shape[0], face_capacity=101, return_status=True, **args)
    assert int(out[5]) == ops.TSDF_ST_FACE_OVERFLOW and same(out[0], v) and same(out[2], f[:101])
    assert out[3].tolist() == vs.tolist() and out[4].tolist() == fs.tolist()
    out = ops.tsdf_mesh_host(vertex_capacity=v.shape[0] + 3, face_capacity=f.shape[0] + 3, return_status=True, **args)
    assert int(out[5]) == 0 and same(out[0][:v.shape[0]], v) and same(out[2][:f.shape[0]], f)


# --------------------------------------------------------------------------------------------- fragments and files
def test_fuse_fragments_with_mesh_returns_the_same_clouds_plus_meshes(meshes):
    depth, K, poses = S.sequence()
    kw = dict(frames_per_fragment=S.PER_FRAGMENT, voxel=S.VOXEL, trunc=S.TRUNC, device='cpu')
    clouds, fposes = fr.fuse_fragments(depth, K, poses, **kw)
    clouds_m, fposes_m, got = fr.fuse_fragments(depth, K, poses, mesh=True, **kw)
    assert len(clouds_m) == len(clouds) == 2 and all(same(a, b) for a, b in zip(clouds_m, clouds))
    assert np.array_equal(fposes_m, fposes)
    v, n, f, vs, fs = meshes['room_w1']                                   # the same two volumes, meshed directly
    for k in range(2):
        assert same(got[k][0], v[vs[k]:vs[k + 1]]) and same(got[k][1], n[vs[k]:vs[k + 1]])
        assert same(got[k][2], f[fs[k]:fs[k + 1]])
    cloud = fr.fuse_scene(depth, K, poses, fposes, S.PER_FRAGMENT, S.VOXEL, trunc=S.TRUNC, device='cpu')
    cloud_m, (sv, sn, sf) = fr.fuse_scene(depth, K, poses, fposes, S.PER_FRAGMENT, S.VOXEL, trunc=S.TRUNC, device='cpu',
                                          mesh=True)
    assert same(cloud_m, cloud) and sv.shape[0] > 0 and sf.shape[0] > 0 and sf.max() < sv.shape[0]
    assert S.surface_distance(sv).max() <= 1.0 * S.VOXEL
    none = fr.fuse_scene(depth, K, poses, np.full((2, 4, 4), np.nan), S.PER_FRAGMENT, S.VOXEL, device='cpu', mesh=True)
    assert none[0].shape == (0, 3) and [a.shape for a in none[1]] == [(0, 3)] * 3


def _read_ply_mesh(filename):
    """A small reader of exactly what ``write_ply_mesh`` writes."""
    with open(filename, 'rb') as f:
        header = []
        while not header or header[-1] != 'end_header':
            header.append(f.readline().decode('ascii').strip())
        counts = {h.split()[1]: int(h.split()[2]) for h in header if h.startswith('element')}
        names = [h.split()[2] for h in header if h.startswith('property float')]
        assert header[:2] == ['ply', 'format binary_little_endian 1.0']
        assert 'property list uchar int vertex_indices' in header
        vert = np.frombuffer(f.read(4 * len(names) * counts['vertex']), dtype='<f4').reshape(-1, len(names))
        rows = np.frombuffer(f.read(13 * counts['face']), dtype=[('n', 'u1'), ('i', '<i4', (3,))])
        assert f.read() == b'' and (rows['n'] == 3).all()
    return names, vert, rows['i']


def test_write_ply_mesh_round_trip(tmp_path, meshes):
    v, n, f, vs, fs = meshes['sphere']
    path = str(tmp_path / 'sphere.ply')
    fr.write_ply_mesh(path, v, f, normals=n)
    names, vert, faces = _read_ply_mesh(path)
    assert names == ['x', 'y', 'z', 'nx', 'ny', 'nz']
    assert same(np.ascontiguousarray(vert[:, :3]), v) and same(np.ascontiguousarray(vert[:, 3:]), n)
    assert same(faces.astype(np.int32), f)
    cloud = read_ply_points(path)                                         # the project's reader: the vertices, as a cloud
    assert cloud.dtype == np.float64 and np.array_equal(cloud, v.astype(np.float64))
    fr.write_ply_mesh(path, v, f)
    names, vert, faces = _read_ply_mesh(path)
    assert names == ['x', 'y', 'z'] and same(np.ascontiguousarray(vert), v) and same(faces.astype(np.int32), f)
    assert np.array_equal(read_ply_points(path), v.astype(np.float64))
    with pytest.raises(ValueError):
        fr.write_ply_mesh(path, v[:10], f)
