"""CPU: TSDF fusion (csrc/tsdf.hpp) -- the host twins of the kernels against the NumPy restatement bit for bit, the
extraction rule on hand-made volumes, and the front end ``datasets/fragments.py`` on the analytic room of
``tsdf_scene`` (surface distance, overlap of the two fragments, files, the fused scene)."""
import numpy as np
import pytest

from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.datasets import fragments as fr
from d3feat_pytorch_amd.datasets import preprocess as pp
import tsdf_scene as S


def bits(a):
    a = a.numpy() if hasattr(a, 'numpy') else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return bits(a).shape == bits(b).shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def scene_volumes():
    """The two fragment volumes of the room by the restatement: (setup, origin, dims, D, w, vol_start, points, starts)."""
    depth, fs, K, M, C = S.fragment_setup()
    origin, dims = fr.place_volumes(ops.tsdf_bounds_numpy(depth, fs, K, C), S.VOXEL)
    D, w, vs = ops.tsdf_numpy(depth, fs, K, M, origin, dims, S.VOXEL, S.TRUNC)
    pts, ps = ops.tsdf_extract_numpy(D, w, vs, origin, dims, S.VOXEL)
    for a in (D, w, pts):
        a.setflags(write=False)
    return (depth, fs, K, M, C), origin, dims, D, w, vs, pts, ps


@pytest.fixture(scope="module")
def fragments():
    depth, K, poses = S.sequence()
    clouds, fposes = fr.fuse_fragments(depth, K, poses, frames_per_fragment=S.PER_FRAGMENT, voxel=S.VOXEL,
                                       trunc=S.TRUNC, device='cpu')
    return clouds, fposes


@pytest.fixture(scope="module")
def subsample(native):
    def fn(points, voxel):
        p = np.ascontiguousarray(points, dtype=np.float32)
        return native.subsample_batch(p, np.array([p.shape[0]], dtype=np.int32), sampleDl=voxel)[0]
    return fn


# --------------------------------------------------------------------------------------- host twin == restatement
def test_host_twin_equals_restatement_on_the_scene(scene_volumes):
    (depth, fs, K, M, C), origin, dims, D, w, vs, pts, ps = scene_volumes
    assert dims.tolist() == [[86, 70, 66], [83, 66, 67]]
    assert same_bits(ops.tsdf_bounds_host(depth, fs, K, C), ops.tsdf_bounds_numpy(depth, fs, K, C))
    Dh, wh, vsh = ops.tsdf_integrate_host(depth, fs, K, M, origin, dims, S.VOXEL, S.TRUNC)
    assert vsh.tolist() == vs.tolist()
    assert same_bits(Dh, D) and same_bits(wh, w)
    assert 0.1 < float((w > 0).mean()) < 0.5 and w.max() == 6.0
    ph, psh = ops.tsdf_extract_host(Dh, wh, vsh, origin, dims, S.VOXEL)
    assert psh.tolist() == ps.tolist()
    assert same_bits(ph, pts)                                  # equal and in the same order
    assert 7000 < ps[1] < 9000 and 4500 < ps[2] - ps[1] < 6000


@pytest.mark.parametrize("name", sorted(S.small_cases()))
def test_host_twin_equals_restatement_on_small_volumes(name):
    case = S.small_cases()[name]
    assert same_bits(ops.tsdf_bounds_host(**S.bounds_args(case)), ops.tsdf_bounds_numpy(**S.bounds_args(case)))
    Dh, wh, vs = ops.tsdf_integrate_host(**S.integrate_args(case))
    Dn, wn, vsn = ops.tsdf_numpy(**S.integrate_args(case))
    assert same_bits(Dh, Dn) and same_bits(wh, wn) and vs.tolist() == vsn.tolist()
    ph, psh = ops.tsdf_extract_host(Dh, wh, vs, **S.extract_args(case))
    pn, psn = ops.tsdf_extract_numpy(Dn, wn, vsn, **S.extract_args(case))
    assert psh.tolist() == psn.tolist() and same_bits(ph, pn)
    n = int(psn[-1])
    seen = float((wn > 0).mean())
    if name in ('zero_frames', 'behind_camera'):
        assert n == 0 and not Dn.any() and not wn.any()
        if name == 'zero_frames':
            assert np.isinf(ops.tsdf_bounds_numpy(**S.bounds_args(case))).all()
    else:
        assert n > 0 and np.isfinite(pn).all()
    if name == 'partly_outside':
        assert 0.0 < seen < 0.5                                # most of the lattice lies outside both frustums
    if name == 'dims_5x1x1':
        assert n <= 4 and (pn[:, 1:] == np.float32([0.0, 1.07])).all()
    if name == 'dims_1x5x5':
        assert (pn[:, 0] == 0).all()                           # no x neighbour: only the y and z axes emit
    if name == 'last_plane':                                   # planes at z = 0.95 .. 1.10: the crossing reaches the last one
        assert (pn[:, 2] > np.float32(1.05)).any() and (pn[:, 2] <= np.float32(0.95) + np.float32(0.05) * 3).all()
    if name in ('holes', 'depth_max', 'f32_nan'):
        full = ops.tsdf_numpy(**S.integrate_args(S.small_cases()['dims_13x9x7']))[1]
        assert wn.sum() < full.sum()                           # the dropped pixels were observations before


# ------------------------------------------------------------------------------------------------ extraction rule
def _extract_both(D, w, dims, origin=(0.0, 0.0, 0.0), voxel=0.5, **kw):
    D = np.asarray(D, dtype=np.float32)
    w = np.asarray(w, dtype=np.float32)
    pn, sn = ops.tsdf_extract_numpy(D, w, None, [origin], [dims], voxel, **kw)
    ph, sh = ops.tsdf_extract_host(D, w, None, [origin], [dims], voxel, **kw)
    assert same_bits(ph, pn) and sh.tolist() == sn.tolist()
    return pn


def test_zero_against_negative_emits_the_lattice_point_and_two_zeros_emit_nothing():
    p = _extract_both([0.0, -0.5], [1, 1], [2, 1, 1], origin=(1.0, 2.0, 3.0))
    assert p.tolist() == [[1.0, 2.0, 3.0]]
    assert _extract_both([0.0, 0.0], [1, 1], [2, 1, 1]).shape == (0, 3)
    assert _extract_both([0.0, 0.5], [1, 1], [2, 1, 1]).shape == (0, 3)      # 0 counts as not negative
    p = _extract_both([-0.25, 0.75], [1, 1], [1, 1, 2], origin=(1.0, 2.0, 3.0))
    assert p.tolist() == [[1.0, 2.0, 3.125]]
    assert _extract_both([-0.25, 1.0], [1, 1], [1, 2, 1]).shape == (0, 3)    # |D| = 1 is not valid
    assert _extract_both([-0.25, np.nan], [1, 1], [1, 2, 1]).shape == (0, 3)


def test_output_order_is_lattice_index_then_axis():
    # 2 x 2 x 2, the corner voxel negative and everything else positive: its three edges cross, in the order x, y, z
    D = np.full(8, 0.5, dtype=np.float32)
    D[0] = -0.5
    p = _extract_both(D, np.ones(8), [2, 2, 2], voxel=1.0)
    assert p.tolist() == [[0.5, 0.0, 0.0], [0.0, 0.5, 0.0], [0.0, 0.0, 0.5]]
    D = np.full(8, 0.5, dtype=np.float32)
    D[7] = -0.5                                                # the far corner: crossings of voxels 3 (z), 5 (y), 6 (x)
    p = _extract_both(D, np.ones(8), [2, 2, 2], voxel=1.0)
    assert p.tolist() == [[1.0, 1.0, 0.5], [1.0, 0.5, 1.0], [0.5, 1.0, 1.0]]


def test_min_weight_drops_voxels_seen_once(scene_volumes):
    _, origin, dims, D, w, vs, pts, ps = scene_volumes
    p1 = _extract_both([-0.5, 0.5, -0.5], [2, 2, 1], [3, 1, 1], min_weight=1.0)
    p2 = _extract_both([-0.5, 0.5, -0.5], [2, 2, 1], [3, 1, 1], min_weight=2.0)
    assert p1.shape == (2, 3) and p2.tolist() == [[0.25, 0.0, 0.0]]
    pn, psn = ops.tsdf_extract_numpy(D, w, vs, origin, dims, S.VOXEL, min_weight=2.0)
    ph, psh = ops.tsdf_extract_host(D, w, vs, origin, dims, S.VOXEL, min_weight=2.0)
    assert same_bits(ph, pn) and psh.tolist() == psn.tolist()
    assert 0 < psn[-1] < ps[-1]


def test_host_capacity_sets_the_overflow_bit_and_writes_nothing_past_it(scene_volumes):
    _, origin, dims, D, w, vs, pts, ps = scene_volumes
    cap = 1000
    p, s, status = ops.tsdf_extract_host(D, w, vs, origin, dims, S.VOXEL, capacity=cap, return_status=True)
    assert int(status) == ops.TSDF_ST_OVERFLOW and s.tolist() == ps.tolist()
    assert same_bits(p, pts[:cap])
    p, s, status = ops.tsdf_extract_host(D, w, vs, origin, dims, S.VOXEL, capacity=int(ps[-1]) + 5, return_status=True)
    assert int(status) == 0 and same_bits(p[:int(ps[-1])], pts)


def test_arguments_are_checked():
    case = S.integrate_args(S.small_cases()['dims_13x9x7'])
    for bad in (dict(dims=[13, 0, 7]), dict(frame_start=[0, 3]), dict(voxel=0.0), dict(trunc=-1.0),
                dict(depth=np.zeros((2, 23, 37), dtype=np.int32)), dict(volume_to_camera=np.zeros((3, 3, 4)))):
        with pytest.raises(ValueError):
            ops.tsdf_integrate_host(**dict(case, **bad))
    with pytest.raises(ValueError):
        ops.tsdf_extract_host(np.zeros(5), np.zeros(5), None, [[0, 0, 0]], [[2, 2, 2]], 0.1)
    with pytest.raises(ValueError):
        ops.tsdf_extract_host(np.zeros(8), np.zeros(8), [0, 7], [[0, 0, 0]], [[2, 2, 2]], 0.1)


# ------------------------------------------------------------------------------------------------------ front end
def test_fragments_lie_on_the_surface_and_overlap(fragments, subsample):
    clouds, fposes = fragments
    depth, K, poses = S.sequence()
    assert np.array_equal(fposes, poses[[0, S.PER_FRAGMENT]])
    assert [7000 < len(clouds[0]) < 9000, 4500 < len(clouds[1]) < 6000] == [True, True]
    for c, P in zip(clouds, fposes):
        assert c.dtype == np.float32
        dist = S.surface_distance(S.to_world(c, P))
        print("max surface distance / voxel: %.3f" % (dist.max() / S.VOXEL))
        assert dist.max() <= 1.0 * S.VOXEL
    sub, corr, overlap = pp.mine_scene(clouds, fposes, 0.03, min_overlap=0.3, device='cpu', subsample=subsample,
                                       return_overlap=True)
    # 0.559 with the oracle's barycentre subsampler (0.552 - 0.559 over three grid placements in the fragment frames,
    # 0.533 when the clouds are subsampled in the world frame): the figure moves by a few hundredths with the grid
    print("overlap of (0, 1): %.3f" % overlap[(0, 1)])
    assert list(corr) == [(0, 1)] and overlap[(0, 1)] > 0.3    # the pair is kept at the project's threshold


def test_write_fragments_round_trip(tmp_path, fragments):
    clouds, fposes = fragments
    path = fr.write_fragments(str(tmp_path), 'room', clouds, fposes, S.PER_FRAGMENT)
    assert open(path + '/cloud_bin_1.info.txt').readline() == "room\tseq-01\t6\t11\n"
    ids, points, poses = pp.read_scene(str(tmp_path), 'room')
    assert ids == ['room/cloud_bin_0', 'room/cloud_bin_1']
    for got, want in zip(points, clouds):
        assert same_bits(got.astype(np.float32), want) and np.array_equal(got, want.astype(np.float64))
    assert np.abs(poses - fposes).max() <= 1e-15 * np.abs(fposes).max()
    with pytest.raises(ValueError):
        fr.write_fragments(str(tmp_path), 'room', clouds, fposes[:1], S.PER_FRAGMENT)
    path = fr.write_fragments(str(tmp_path), 'short', clouds, fposes, S.PER_FRAGMENT, num_frames=8)
    assert open(path + '/cloud_bin_0.info.txt').readline() == "short\tseq-01\t0\t5\n"
    assert open(path + '/cloud_bin_1.info.txt').readline() == "short\tseq-01\t6\t7\n"     # the shorter last fragment


def test_fuse_scene_in_the_world_frame_and_without_a_fragment(fragments):
    depth, K, poses = S.sequence()
    _, fposes = fragments
    cloud = fr.fuse_scene(depth, K, poses, fposes, S.PER_FRAGMENT, S.VOXEL, trunc=S.TRUNC, device='cpu')
    dist = S.surface_distance(cloud)                           # true fragment poses: the scene frame is the world
    print("scene: %d points, max surface distance / voxel: %.3f" % (len(cloud), dist.max() / S.VOXEL))
    assert len(cloud) > 8000 and dist.max() <= 1.0 * S.VOXEL
    # a NaN row removes exactly that fragment's frames: what is left is the first six frames fused in the world frame
    gone = fposes.copy()
    gone[1] = np.nan
    only0 = fr.fuse_scene(depth, K, poses, gone, S.PER_FRAGMENT, S.VOXEL, trunc=S.TRUNC, device='cpu')
    want = fr.fuse_scene(depth[:6], K, poses[:6], fposes[:1], S.PER_FRAGMENT, S.VOXEL, trunc=S.TRUNC, device='cpu')
    assert same_bits(only0, want) and 0 < len(only0) < len(cloud)
    short = fr.fuse_scene(depth, K, poses, fposes[:1], S.PER_FRAGMENT, S.VOXEL, trunc=S.TRUNC, device='cpu')
    assert same_bits(short, want)                              # a fragment without a pose is left out too
    none = fr.fuse_scene(depth, K, poses, np.full((2, 4, 4), np.nan), S.PER_FRAGMENT, S.VOXEL, device='cpu')
    assert none.shape == (0, 3)


def test_a_volume_over_max_bytes_raises_before_anything_runs():
    depth, K, poses = S.sequence()
    with pytest.raises(ValueError, match=r"86 x 70 x 66 voxels.*extent 1\.72 x 1\.40 x 1\.32 m"):
        fr.fuse_fragments(depth, K, poses, frames_per_fragment=S.PER_FRAGMENT, voxel=S.VOXEL, device='cpu',
                          max_bytes=1 << 20)


def test_batches_by_max_bytes_give_the_same_fragments(fragments):
    depth, K, poses = S.sequence()
    one_by_one = fr.fuse_fragments(depth, K, poses, frames_per_fragment=S.PER_FRAGMENT, voxel=S.VOXEL, trunc=S.TRUNC,
                                   device='cpu', max_bytes=8 * 86 * 70 * 66)[0]
    assert all(same_bits(a, b) for a, b in zip(one_by_one, fragments[0])) and len(one_by_one) == 2
    short_last = fr.fuse_fragments(depth[:8], K, poses[:8], frames_per_fragment=S.PER_FRAGMENT, voxel=S.VOXEL,
                                   trunc=S.TRUNC, device='cpu')
    assert len(short_last[0]) == 2 and same_bits(short_last[0][0], fragments[0][0])
    assert np.array_equal(short_last[1][1], poses[6])


def test_read_sequence(tmp_path):
    from PIL import Image
    depth, K, poses = S.sequence()
    folder = tmp_path / 'seq-01'
    folder.mkdir()
    np.savetxt(str(tmp_path / 'camera-intrinsics.txt'), [[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]])
    for i in range(3):
        Image.fromarray(depth[i].copy()).save(str(folder / ('frame-%06d.depth.png' % i)))
        np.savetxt(str(folder / ('frame-%06d.pose.txt' % i)), poses[i], fmt='%.17g')
    d, k, p = fr.read_sequence(str(folder))
    assert d.dtype == np.uint16 and np.array_equal(d, depth[:3])
    assert np.array_equal(k, K) and np.array_equal(p, poses[:3])
    with pytest.raises(ValueError):
        fr.read_sequence(str(tmp_path))
