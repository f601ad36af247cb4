"""CPU: sparse TSDF volumes (csrc/tsdf_sparse.hpp) -- the host twins of the kernels against the NumPy restatement bit
for bit, and both against the dense path of csrc/tsdf.hpp: the allocated bricks cover every voxel the dense volume makes
valid, the pool holds the dense D and w, the points are the dense points as a set of rows.  No tolerance anywhere."""
import numpy as np
import pytest

from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.datasets import fragments as fr
import tsdf_scene as S
import tsdf_sparse_cases as SC
from tsdf_sparse_cases import host, same_bits, same_row_sets, same_tables


def dense_of(case):
    """The dense volumes of a case by the restatement: (D, w, vol_start, points, point_start)."""
    D, w, vs = ops.tsdf_numpy(**{k: v for k, v in case.items() if k != 'camera_to_volume'})
    pts, ps = ops.tsdf_extract_numpy(D, w, vs, case['origin'], case['dims'], case['voxel'])
    return D, w, vs, pts, ps


def allocated_voxels(sv):
    """bool [total]: the dense voxels that lie in an allocated brick."""
    ones = np.ones((sv.bricks, 512), dtype=np.float32)
    return ops.tsdf_densify(ones, ones, sv)[0] > 0


def check_case(case, expect_points=None):
    """Everything the issue asks of one batch; returns (sv, dense D, dense w, vol_start, sparse points, starts)."""
    sv = ops.tsdf_allocate_numpy(**SC.allocate_args(case))
    assert same_tables(ops.tsdf_allocate_host(**SC.allocate_args(case)), sv)             # allocation equality
    D, w, vs, pts, ps = dense_of(case)
    inside = allocated_voxels(sv)
    valid = (w >= 1) & (np.abs(D) < 1)
    assert not (valid & ~inside).any()                                                   # superset
    Dn, wn = ops.tsdf_sparse_numpy(**SC.sparse_args(case, sv))
    Dh, wh = ops.tsdf_integrate_sparse_host(**SC.sparse_args(case, sv))
    assert tuple(Dh.shape) == (sv.bricks, 512) and same_bits(Dh, Dn) and same_bits(wh, wn)   # pool equality
    Dd, wd, vsd = ops.tsdf_densify(Dn, wn, sv)
    assert vsd.tolist() == vs.tolist()
    assert same_bits(Dd[inside], D[inside]) and same_bits(wd[inside], w[inside])
    assert not Dd[~inside].any() and not wd[~inside].any()
    pn, psn = ops.tsdf_extract_sparse_numpy(Dn, wn, sv)
    ph, psh = ops.tsdf_extract_sparse_host(Dh, wh, sv)
    assert psh.tolist() == psn.tolist() and same_bits(ph, pn)                            # twin == restatement, in order
    assert same_row_sets(pn, psn, pts, ps) and int(psn[-1]) == int(ps[-1])               # the dense rows, per volume
    if expect_points is not None:
        assert (int(ps[-1]) > 0) == expect_points
    return sv, D, w, vs, pn, psn


@pytest.fixture(scope="module")
def room():
    """The two fragments of the room as one batch, checked: (args, sv, D, w, vol_start, points, point_start)."""
    args = SC.room_args()
    return (args,) + check_case(args, expect_points=True)


# ------------------------------------------------------------------------------------------------ the room
def test_the_room_allocates_a_superset_and_not_everything(room):
    args, sv, D, w, vs, pts, ps = room
    assert args['dims'].tolist() == [[86, 70, 66], [83, 66, 67]]
    lattice = sv.lattice_start.tolist()
    assert lattice == [0, 11 * 9 * 9, 11 * 9 * 9 + 11 * 9 * 9]
    start = host(sv.brick_start).tolist()
    print("allocated bricks: %s of %s" % (np.diff(start).tolist(), np.diff(lattice).tolist()))
    index = host(sv.brick_index)
    assert (index < 0).any()                     # a lattice brick is NOT allocated: no pass by allocating everything
    for v in range(2):
        assert 0 < start[v + 1] - start[v] < lattice[v + 1] - lattice[v]
        mine = index[lattice[v]:lattice[v + 1]]
        assert sorted(mine[mine >= 0].tolist()) == list(range(start[v + 1] - start[v]))
    assert int(ps[-1]) > 12000
    # no ratio is claimed for this tiny room (trunc = 4 voxels against bricks of 8): only that the figure is the tables'
    assert ops.tsdf_sparse_bytes(sv) == 4096 * sv.bricks + 4 * lattice[-1] + 12 * sv.bricks + 8 * 3
    assert ops.tsdf_sparse_bytes(sv, 0) + ops.tsdf_sparse_bytes(sv, 1) == ops.tsdf_sparse_bytes(sv) + 8


def test_the_room_has_crossings_between_bricks_on_every_axis(room):
    args, sv, D, w, vs, pts, ps = room
    nx, ny, nz = args['dims'][0]
    D0, w0 = D[:vs[1]].reshape(nz, ny, nx), w[:vs[1]].reshape(nz, ny, nx)
    ok = (w0 >= 1) & (np.abs(D0) < 1)
    for axis in range(3):                        # crossings whose two voxels sit in different bricks
        ok_a, D_a = np.moveaxis(ok, 2 - axis, 0), np.moveaxis(D0, 2 - axis, 0)
        last = ok_a.shape[0] - 1
        low, high = np.arange(7, last, 8), np.arange(8, last + 1, 8)[:len(np.arange(7, last, 8))]
        assert (ok_a[low] & ok_a[high] & ((D_a[low] < 0) != (D_a[high] < 0))).any()
    # a valid voxel whose +1 neighbour brick is absent cannot come out of the allocation rule (the neighbour of a voxel
    # inside a pixel's box lies inside the widened box): test_a_valid_voxel_before_an_absent_brick_emits_nothing_there
    # makes one by hand


# ------------------------------------------------------------------------------------------------ small volumes
@pytest.mark.parametrize("name", sorted(SC.cases()))
def test_small_volumes(name):
    case = SC.cases()[name]
    sv, D, w, vs, pts, ps = check_case(case, expect_points=name not in ('zero_frames', 'behind_camera'))
    if name in ('zero_frames', 'behind_camera'):
        assert sv.bricks == 0 and (host(sv.brick_index) == -1).all() and host(sv.brick_start).tolist() == [0, 0]
    if name in ('dims_1x5x5', 'dims_5x1x1', 'last_plane'):
        assert sv.lattice_start.tolist() == [0, 1] and sv.bricks == 1      # dims below 8 on every axis: one brick
    if name == 'dims_13x9x7':
        assert sv.lattice_start.tolist() == [0, 4]                        # no multiple of 8
    if name == 'partly_outside':
        assert 0 < sv.bricks < int(sv.lattice_start[-1])
    if name == 'brick_face_17x9x9':
        Dv, wv = D.reshape(9, 9, 17), w.reshape(9, 9, 17)
        ok = (wv >= 1) & (np.abs(Dv) < 1)
        face = ok[:, :, 7] & ok[:, :, 8] & ((Dv[:, :, 7] < 0) != (Dv[:, :, 8] < 0))
        assert face.any()                        # a sign change exactly between ix = 7 and ix = 8
        assert sv.lattice_start.tolist() == [0, 3 * 2 * 2]


@pytest.mark.parametrize("empty", sorted(SC.EMPTY_BETWEEN))
def test_a_volume_without_bricks_between_two_others(empty):
    names = SC.EMPTY_BETWEEN[empty]
    batch = SC.batch_of(names)
    sv, D, w, vs, pts, ps = check_case(batch, expect_points=True)
    start = host(sv.brick_start).tolist()
    assert start[1] == start[2] and 0 < start[1] < start[3]
    assert int(ps[1]) == int(ps[2]) and 0 < int(ps[1]) < int(ps[3])
    for v, name in enumerate(names):             # a batch equals its volumes alone
        alone = ops.tsdf_allocate_numpy(**SC.allocate_args(SC.cases()[name]))
        lo, hi = sv.lattice_start[v], sv.lattice_start[v + 1]
        assert np.array_equal(host(sv.brick_index)[lo:hi], alone.brick_index)
        assert np.array_equal(host(sv.brick_coord)[start[v]:start[v + 1]], alone.brick_coord)
        Da, wa = ops.tsdf_sparse_numpy(**SC.sparse_args(SC.cases()[name], alone))
        pa, psa = ops.tsdf_extract_sparse_numpy(Da, wa, alone)
        assert same_bits(pa, pts[ps[v]:ps[v + 1]])


def test_a_valid_voxel_before_an_absent_brick_emits_nothing_there():
    sv, D, w = SC.absent_neighbour_pool()
    pn, psn = ops.tsdf_extract_sparse_numpy(D, w, sv)
    ph, psh = ops.tsdf_extract_sparse_host(D, w, sv)
    assert same_bits(ph, pn) and psh.tolist() == psn.tolist() == [0, 64]
    assert (pn[:, 0] == np.float32(1.75)).all()                # between ix = 3 and ix = 4, nothing at ix = 7
    Dd, wd, vs = ops.tsdf_densify(D, w, sv)
    pd, psd = ops.tsdf_extract_numpy(Dd, wd, vs, sv.origin, sv.dims, sv.voxel)
    assert same_row_sets(pn, psn, pd, psd)
    assert np.array_equal(pn[:3], np.float32([[1.75, 0, 0], [1.75, 0.5, 0], [1.75, 1.0, 0]]))   # slot order: iy next


def test_min_weight_and_capacity(room):
    args, sv, D, w, vs, pts, ps = room
    Dn, wn = ops.tsdf_sparse_numpy(**SC.sparse_args(args, sv))
    p2, ps2 = ops.tsdf_extract_sparse_numpy(Dn, wn, sv, min_weight=2.0)
    h2, hs2 = ops.tsdf_extract_sparse_host(Dn, wn, sv, min_weight=2.0)
    d2, ds2 = ops.tsdf_extract_numpy(D, w, vs, args['origin'], args['dims'], S.VOXEL, min_weight=2.0)
    assert same_bits(h2, p2) and hs2.tolist() == ps2.tolist() and same_row_sets(p2, ps2, d2, ds2)
    assert 0 < int(ps2[-1]) < int(ps[-1])
    cap = 1000
    p, s, status = ops.tsdf_extract_sparse_host(Dn, wn, sv, capacity=cap, return_status=True)
    assert int(status) == ops.TSDF_ST_OVERFLOW and s.tolist() == ps.tolist() and same_bits(p, pts[:cap])
    p, s, status = ops.tsdf_extract_sparse_host(Dn, wn, sv, capacity=int(ps[-1]) + 5, return_status=True)
    assert int(status) == 0 and same_bits(p[:int(ps[-1])], pts)


def test_arguments_are_checked():
    case = SC.cases()['dims_13x9x7']
    for bad in (dict(dims=[13, 0, 7]), dict(frame_start=[0, 3]), dict(voxel=0.0), dict(trunc=-1.0)):
        with pytest.raises(ValueError):
            ops.tsdf_allocate_host(**dict(SC.allocate_args(case), **bad))
    sv = ops.tsdf_allocate_host(**SC.allocate_args(case))
    with pytest.raises(ValueError):
        ops.tsdf_extract_sparse_host(np.zeros(5), np.zeros(5), sv)
    with pytest.raises(ValueError):
        ops.tsdf_integrate_sparse_host(**dict(SC.sparse_args(case, sv), frame_start=[0, 1, 2]))
    short = ops.SparseVolumes(sv.brick_index[:-1], sv.brick_coord, sv.brick_start, sv.origin, sv.dims, sv.voxel)
    with pytest.raises(ValueError):
        ops.tsdf_integrate_sparse_host(**SC.sparse_args(case, short))


# ------------------------------------------------------------------------------------------------------ front end
def test_fuse_fragments_sparse_gives_the_same_rows_and_poses():
    depth, K, poses = S.sequence()
    kw = dict(frames_per_fragment=S.PER_FRAGMENT, voxel=S.VOXEL, trunc=S.TRUNC, device='cpu')
    dense, dense_poses = fr.fuse_fragments(depth, K, poses, **kw)
    sparse, sparse_poses = fr.fuse_fragments(depth, K, poses, sparse=True, **kw)
    assert np.array_equal(dense_poses, sparse_poses) and len(sparse) == len(dense) == 2
    for a, b in zip(sparse, dense):
        assert a.dtype == np.float32 and same_row_sets(a, [0, len(a)], b, [0, len(b)])
    # one volume per batch (the larger one's sparse bytes): the same clouds, in the same order
    sv = ops.tsdf_allocate_numpy(**SC.allocate_args(SC.room_args()))
    one = max(ops.tsdf_sparse_bytes(sv, v) for v in range(2))
    split = fr.fuse_fragments(depth, K, poses, sparse=True, max_bytes=one, **kw)[0]
    assert all(same_bits(a, b) for a, b in zip(split, sparse))
    with pytest.raises(ValueError, match=r"%d allocated bricks \(of 891\)" % int(host(sv.brick_start)[1])):
        fr.fuse_fragments(depth, K, poses, sparse=True, max_bytes=one // 2, **kw)


def test_a_scene_too_large_for_a_dense_volume_fits_as_a_sparse_one():
    depth, K, poses = SC.far_patches()
    voxel, trunc = 0.01, 0.05
    kw = dict(frames_per_fragment=2, voxel=voxel, trunc=trunc, device='cpu')
    C = poses                                                    # the scene frame is the world
    origin, dims = fr.place_volumes(ops.tsdf_bounds_numpy(depth, [0, 2], K, C), voxel)
    dense_bytes = 8 * int(np.prod(dims[0]))
    sv = ops.tsdf_allocate_numpy(depth, [0, 2], K, C, origin, dims, voxel, trunc)
    sparse_bytes = ops.tsdf_sparse_bytes(sv)
    max_bytes = 1 << 20
    print("dense %d bytes, sparse %d bytes (%d of %d bricks), max_bytes %d"
          % (dense_bytes, sparse_bytes, sv.bricks, int(sv.lattice_start[-1]), max_bytes))
    assert sparse_bytes < max_bytes < dense_bytes
    with pytest.raises(ValueError, match="more than max_bytes"):
        fr.fuse_scene(depth, K, poses, poses[:1], max_bytes=max_bytes, **kw)
    sparse = fr.fuse_scene(depth, K, poses, poses[:1], max_bytes=max_bytes, sparse=True, **kw)
    dense = fr.fuse_scene(depth, K, poses, poses[:1], max_bytes=2 * dense_bytes, **kw)
    assert len(dense) > 500 and same_row_sets(sparse, [0, len(sparse)], dense, [0, len(dense)])
    assert S.surface_distance(sparse).max() <= 1.0 * voxel


def test_sparse_with_mesh_raises():
    depth, K, poses = S.sequence()
    with pytest.raises(ValueError, match="sparse=True gives no mesh"):
        fr.fuse_fragments(depth, K, poses, frames_per_fragment=S.PER_FRAGMENT, voxel=S.VOXEL, device='cpu',
                          sparse=True, mesh=True)
    with pytest.raises(ValueError, match="sparse=True gives no mesh"):
        fr.fuse_scene(depth, K, poses, poses[[0, 6]], S.PER_FRAGMENT, S.VOXEL, device='cpu', sparse=True, mesh=True)
