"""Pools and comparisons shared by the sparse mesh tests (csrc/tsdf_mesh_sparse.hpp): hand-made pools (a sphere through
a brick corner, the same with a brick deleted, a tilted plane over more than one scan group), the integrated pools of
``tsdf_sparse_cases``, and the two comparisons -- in order, bit for bit; and against the dense mesh up to order."""
import functools

import numpy as np

from d3feat_pytorch_amd import ops
import tsdf_sparse_cases as SC

PARTS = ("vertices", "normals", "faces", "vertex_start", "face_start")


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, 'detach') else np.asarray(a)


def words(a):
    """The array with f32 viewed as uint32: -0 / +0 and NaN payloads count."""
    a = np.ascontiguousarray(host(a))
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_in_order(got, want):
    """Identical arrays bit for bit: vertices, normals, faces, vertex_start, face_start."""
    for g, w_, what in zip(got, want, PARTS):
        g, w_ = host(g), host(w_)
        assert g.dtype == w_.dtype and g.shape == w_.shape, (what, g.dtype, w_.dtype, g.shape, w_.shape)
        assert np.array_equal(words(g), words(w_)), what


def _sorted(rows):
    return rows[np.lexsort(rows.T[::-1])]


def assert_up_to_order(got, want):
    """Per volume: equal counts, the same multiset of vertex rows (position + normal, 6 words) and the same multiset
    of faces with every index replaced by its vertex's 6 words (18 words, the corner order kept)."""
    v, n, f, vs, fs = (host(a) for a in got)
    V, N, F, VS, FS = (host(a) for a in want)
    assert np.array_equal(np.diff(vs), np.diff(VS)), (vs, VS)
    assert np.array_equal(np.diff(fs), np.diff(FS)), (fs, FS)
    for k in range(len(VS) - 1):
        a = np.concatenate([words(v[vs[k]:vs[k + 1]]).reshape(-1, 3), words(n[vs[k]:vs[k + 1]]).reshape(-1, 3)], 1)
        b = np.concatenate([words(V[VS[k]:VS[k + 1]]).reshape(-1, 3), words(N[VS[k]:VS[k + 1]]).reshape(-1, 3)], 1)
        assert np.array_equal(_sorted(a), _sorted(b)), "vertex rows of volume %d" % k
        fa, fb = f[fs[k]:fs[k + 1]], F[FS[k]:FS[k + 1]]
        if fa.size:
            assert fa.min() >= 0 and fa.max() < a.shape[0], "face entries of volume %d are not local" % k
        assert np.array_equal(_sorted(a[fa].reshape(-1, 18)), _sorted(b[fb].reshape(-1, 18))), "faces of volume %d" % k


def dense_mesh(pool, min_weight=1.0):
    """``tsdf_mesh_numpy`` of the densified pool: the dense restatement, which predates the sparse mesh."""
    sv, D, w = pool
    Dd, wd, vs = ops.tsdf_densify(np.asarray(host(D)), np.asarray(host(w)), sv)
    return ops.tsdf_mesh_numpy(Dd, wd, vs, sv.origin, sv.dims, sv.voxel, min_weight)


def _frozen(sv, D, w):
    for a in (D, w):
        a.setflags(write=False)
    return sv, D, w


def full_pool(dense, dims, voxel, origin=(0.0, 0.0, 0.0)):
    """A hand-made pool of one volume whose dims are multiples of 8, every brick allocated, w = 1: ``dense`` [nz,ny,nx]
    cut into rows in lattice order."""
    nx, ny, nz = dims
    nb = (nx // 8, ny // 8, nz // 8)
    B = nb[0] * nb[1] * nb[2]
    D = np.ascontiguousarray(np.asarray(dense, dtype=np.float32).reshape(nb[2], 8, nb[1], 8, nb[0], 8)
                             .transpose(0, 2, 4, 1, 3, 5)).reshape(B, 512)
    l = np.arange(B)
    coord = np.stack([l % nb[0], (l // nb[0]) % nb[1], l // (nb[0] * nb[1])], axis=1).astype(np.int32)
    sv = ops.SparseVolumes(np.arange(B, dtype=np.int32), coord, np.array([0, B], dtype=np.int64),
                           np.array([origin], dtype=np.float32), np.array([dims], dtype=np.int32),
                           np.array([voxel], dtype=np.float32))
    return sv, D, np.ones((B, 512), dtype=np.float32)


def without_brick(pool, l):
    """The one-volume pool with lattice brick ``l`` deleted: its row and its table entry."""
    sv, D, w = pool
    index = np.array(sv.brick_index)
    row = int(index[l])
    index[index > row] -= 1
    index[l] = -1
    keep = np.arange(sv.bricks) != row
    out = ops.SparseVolumes(index, np.ascontiguousarray(np.asarray(sv.brick_coord)[keep]),
                            np.array([0, sv.bricks - 1], dtype=np.int64), sv.origin, sv.dims, sv.voxel)
    return _frozen(out, np.ascontiguousarray(D[keep]), np.ascontiguousarray(w[keep]))


SPHERE_CENTER, SPHERE_RADIUS = (0.387, 0.391, 0.407), 0.22
SPHERE_COUNTS = ((376, 3), (748, 3))      # vertices, triangles: what tsdf_mesh_numpy gives the dense sphere


@functools.lru_cache(maxsize=None)
def sphere_pool():
    """16 x 16 x 16 voxels of 0.05 m, all 8 bricks: a sphere of radius 0.22 m about a point next to the corner the 8
    bricks share (0.4, 0.4, 0.4), truncated at 4 voxels; its quads take cells from up to 4 bricks on every axis pair."""
    i = np.arange(16, dtype=np.float64) * 0.05
    z, y, x = np.meshgrid(i, i, i, indexing='ij')
    sdf = np.sqrt((x - SPHERE_CENTER[0]) ** 2 + (y - SPHERE_CENTER[1]) ** 2 + (z - SPHERE_CENTER[2]) ** 2) - SPHERE_RADIUS
    return _frozen(*full_pool(np.clip(sdf / 0.2, -1.0, 1.0), (16, 16, 16), 0.05))


PLANE_DIMS = (96, 96, 72)          # 12 x 12 x 9 = 1296 bricks: two scan groups of 1024 rows


@functools.lru_cache(maxsize=None)
def plane_pool():
    """96 x 96 x 72 voxels of 0.01 m, all 1296 bricks: a tilted plane that crosses x = 31.7 voxels at (y, z) = (12, 60),
    between the bricks of the rows 1023 and 1024 (bx = 3 and 4, by = 1, bz = 7), truncated at 4 voxels."""
    nx, ny, nz = PLANE_DIMS
    z, y, x = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64),
                          np.arange(nx, dtype=np.float64), indexing='ij')
    sdf = ((x - 31.7) + 0.13 * (y - 12.0) + 0.21 * (z - 60.0)) / np.sqrt(1.0 + 0.13 ** 2 + 0.21 ** 2)
    return _frozen(*full_pool(np.clip(sdf / 4.0, -1.0, 1.0), PLANE_DIMS, 0.01, origin=(0.1, -0.2, 0.3)))


def vertex_rows(pool):
    """The pool row that owns each vertex of a one-volume pool, counted independently: the cells of the densified
    volume whose 8 corners are valid and differ in sign, per brick of their lowest voxel, in pool order (plain NumPy on
    D and w and the tables, no mesh code)."""
    sv, D, w = pool
    Dd, wd, _ = ops.tsdf_densify(np.asarray(D), np.asarray(w), sv)
    nx, ny, nz = (int(a) for a in sv.dims[0])
    Dd, ok = Dd.reshape(nz, ny, nx), (wd.reshape(nz, ny, nx) >= 1) & (np.abs(Dd.reshape(nz, ny, nx)) < 1)
    complete, inside, outside = (np.ones((nz - 1, ny - 1, nx - 1), dtype=bool) for _ in range(3))
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                at = (slice(dz, nz - 1 + dz), slice(dy, ny - 1 + dy), slice(dx, nx - 1 + dx))
                complete &= ok[at]
                inside &= Dd[at] < 0
                outside &= ~(Dd[at] < 0)
    iz, iy, ix = np.nonzero(complete & ~inside & ~outside)
    nb = (np.asarray(sv.dims[0], dtype=np.int64) + 7) // 8
    rows = np.asarray(sv.brick_index)[((iz >> 3) * nb[1] + (iy >> 3)) * nb[0] + (ix >> 3)].astype(np.int64)
    return np.sort(rows)


@functools.lru_cache(maxsize=None)
def integrated(name):
    """The pool of case ``name`` of ``tsdf_sparse_cases.cases()`` (or 'batch_' + the name of an ``EMPTY_BETWEEN`` batch, or 'room'):
    allocated and integrated in one go by the NumPy restatements.  ``(sv, D, w)``; shared, do not modify."""
    if name == 'room':
        case = SC.room_args()
    elif name.startswith('batch_'):
        case = SC.batch_of(SC.EMPTY_BETWEEN[name[6:]])
    else:
        case = SC.cases()[name]
    sv = ops.tsdf_allocate_numpy(**SC.allocate_args(case))
    D, w = ops.tsdf_sparse_numpy(**SC.sparse_args(case, sv))
    return _frozen(sv, D, w)


def volume_of(pool, v):
    """Volume ``v`` of a batch pool as a pool of its own."""
    sv, D, w = pool
    ls, bs = sv.lattice_start, np.asarray(sv.brick_start)
    rows = slice(int(bs[v]), int(bs[v + 1]))
    one = ops.SparseVolumes(np.asarray(sv.brick_index)[int(ls[v]):int(ls[v + 1])], np.asarray(sv.brick_coord)[rows],
                            np.array([0, rows.stop - rows.start], dtype=np.int64), sv.origin[v:v + 1], sv.dims[v:v + 1],
                            sv.voxel[v:v + 1])
    return one, D[rows], w[rows]


@functools.lru_cache(maxsize=None)
def host_mesh(name, min_weight=1.0):
    """The host twin's mesh of a named pool (``integrated`` names, 'sphere', 'sphere_less', 'plane', 'absent')."""
    sv, D, w = named(name)
    return tuple(host(a) for a in ops.tsdf_mesh_sparse_host(D, w, sv, min_weight))


def named(name):
    if name == 'sphere':
        return sphere_pool()
    if name == 'sphere_less':
        return without_brick(sphere_pool(), 5)
    if name == 'plane':
        return plane_pool()
    if name == 'absent':
        return SC.absent_neighbour_pool()
    return integrated(name)


ROOM_COUNTS = {1.0: ([0, 6996, 11562], [0, 12792, 20976]), 2.0: ([0, 6148, 9780], [0, 11074, 17470])}
