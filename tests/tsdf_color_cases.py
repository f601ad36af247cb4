"""Inputs and checks shared by the TSDF colour tests (csrc/tsdf_color.hpp): the small volumes of ``tsdf_scene`` and the
analytic room painted with ``rgbd_cases.tex``, hand-made lattices for ``color_at``, and a six-view planar slide.  The
same properties are asked of the host twins (CPU tests) and of the kernels (GPU tests): a ``Backend`` names the
functions of one of them; ``NUMPY`` is the restatement both are held against.  References are computed once by the host
twins or the restatement and shared; do not modify them."""
import functools

import numpy as np
import pytest
import torch

from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.datasets import fragments as fr
import odometry_cases as OC
import raycast_cases as RCC
import rgbd_cases as RC
import tsdf_scene as S
import tsdf_sparse_cases as SC

arr = RC.arr
SMALL = sorted(S.small_cases())
INTEGRATION_CASES = SMALL + ['room']


class Backend(object):
    """The colour functions of the device (''), the host twins ('_host') or the restatement ('_numpy')."""
    STEMS = dict(integrate=('tsdf_integrate', 'tsdf_numpy'), sparse=('tsdf_integrate_sparse', 'tsdf_sparse_numpy'),
                 allocate=('tsdf_allocate', None), extend=('tsdf_extend', None), raycast=('tsdf_raycast', None),
                 raycast_sparse=('tsdf_raycast_sparse', None), sample=('tsdf_sample_color', None),
                 sample_sparse=('tsdf_sample_color_sparse', None), extract=('tsdf_extract', None))

    def __init__(self, suffix):
        self.suffix = suffix
        self.name = suffix.strip('_') or 'device'
        for attr, (stem, numpy_name) in self.STEMS.items():
            setattr(self, attr, getattr(ops, numpy_name if suffix == '_numpy' and numpy_name else stem + suffix))

    @property
    def device(self):
        return 'cuda' if self.suffix == '' else 'cpu'

    def put(self, a):
        """An array where this backend's volumes live: a tensor on its device, or the array for the restatement."""
        a = np.array(arr(a))
        return a if self.suffix == '_numpy' else torch.from_numpy(a).to(self.device)


NUMPY = Backend('_numpy')
HOST = Backend('_host')


def same(a, b):
    """Bit-equal where not NaN, and a NaN where the other has one (a NaN's sign and payload are not part of the rule)."""
    return RC.same_intensity(np.asarray(arr(a), dtype=np.float32), np.asarray(arr(b), dtype=np.float32))


# ------------------------------------------------------------------------------------------------------- inputs
def f32_depth(depth):
    d = np.asarray(depth)
    return (d.astype(np.float32) / np.float32(1000.0)) if d.dtype == np.uint16 else d


@functools.lru_cache(maxsize=None)
def room_args():
    """Keyword arguments of ``ops.tsdf_integrate`` for the room fused into ONE volume in the frame of camera 0 (the
    volume of ``raycast_cases.room_volume``), and camera_to_volume."""
    depth, K, poses = S.sequence()
    vol = RCC.room_volume()
    M = np.stack([fr.rigid_inverse(P) @ poses[0] for P in poses])
    C = np.stack([fr.rigid_inverse(poses[0]) @ P for P in poses])
    return dict(depth=depth, frame_start=[0, S.FRAMES], intrinsics=K, volume_to_camera=M, origin=vol['origin'],
                dims=vol['dims'], voxel=S.VOXEL, trunc=S.TRUNC, depth_scale=1000.0, depth_max=6.0,
                camera_to_volume=C)


def case_args(name):
    return room_args() if name == 'room' else S.small_cases()[name]


def case_color(name, channels, bad=False):
    """The colour frames of a case: f32 intensity for one channel, uint8 RGB for three."""
    if name == 'room':
        return RC.room()[3] if channels == 1 else RC.room()[4]
    inten = RC.small_intensity(np.asarray(case_args(name)['depth']).shape, bad=bad)
    return inten if channels == 1 else RC.to_rgb8(inten)


def with_depth(args, f32):
    a = S.integrate_args(args)
    if f32:
        a = dict(a, depth=f32_depth(a['depth']))
    return a


@functools.lru_cache(maxsize=None)
def reference(name, channels, f32=False, bad=False):
    """(D, w, vol_start, Cv) of the restatement for a case; shared."""
    out = NUMPY.integrate(color=case_color(name, channels, bad), **with_depth(case_args(name), f32))
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------- 1. integration parity
def check_integration(be, name, channels, f32):
    args = with_depth(case_args(name), f32)
    D, w, vs, Cv = be.integrate(color=case_color(name, channels), **args)
    D0, w0, _ = be.integrate(**args)
    Dn, wn, _, Cn = reference(name, channels, f32)
    assert arr(Cv).shape == (arr(D).size, channels)
    assert RC.same_bits(D, D0) and RC.same_bits(w, w0), "colour changed D or w"
    assert same(D, Dn) and same(w, wn) and same(Cv, Cn)
    seen = arr(w) > 0
    if seen.any():
        c = arr(Cv)[seen]
        assert np.isfinite(c).all() and c.min() >= 0.0 and c.max() <= 1.0     # a mean of values in [0, 1]
    assert not arr(Cv)[~seen].any()
    return int(seen.sum())


PLANTED = {0: (18, 11, np.nan), 1: (20, 12, np.inf)}      # frame -> (u, v, value): pixels the 13 x 9 x 7 volume reads


def planted_color():
    c = np.array(case_color('dims_13x9x7', 1))
    for f, (u, v, value) in PLANTED.items():
        c[f, v, u] = value
    return c


def check_poison(be):
    """A NaN and an infinity planted in the colour frames reach exactly the voxels that read those pixels."""
    name = 'dims_13x9x7'
    args = with_depth(case_args(name), False)
    D, w, _, Cv = be.integrate(color=planted_color(), **args)
    Dn, wn, _, Cn = NUMPY.integrate(color=planted_color(), **args)
    clean = reference(name, 1)[3]
    bad, bad_n = ~np.isfinite(arr(Cv)), ~np.isfinite(Cn)
    assert np.array_equal(bad, bad_n) and bad.any() and not bad.all()
    assert np.isnan(arr(Cv)).any() and np.isinf(arr(Cv)).any()
    assert same(Cv, Cn) and same(D, Dn) and same(w, wn) and np.isfinite(arr(D)).all()
    assert np.array_equal(RC.bits(arr(Cv)[~bad]), RC.bits(clean[~bad])), "a voxel that read no planted pixel changed"
    # the voxels that read a planted pixel, found independently: those whose colour changes when that pixel does
    other = np.array(case_color(name, 1))
    for f, (u, v, _) in PLANTED.items():
        other[f, v, u] += np.float32(0.25)
    moved = NUMPY.integrate(color=other, **args)[3] != clean
    assert np.array_equal(moved, bad)
    return int(bad.sum())


# ------------------------------------------------------------------------------------------------------ 2. into=
def split_frames(args, lo, hi, frame_start):
    return dict(args, depth=args['depth'][lo:hi], volume_to_camera=args['volume_to_camera'][lo:hi],
                frame_start=frame_start)


def check_into(be, name, channels):
    args = with_depth(case_args(name), False)
    color = case_color(name, channels)
    F = args['depth'].shape[0]
    whole = be.integrate(color=color, **args)
    k = F // 2
    first = be.integrate(color=color[:k], **split_frames(args, 0, k, [0, k]))
    again = be.integrate(color=color[k:], into=(first[0], first[1], first[3]), **split_frames(args, k, F, [0, F - k]))
    assert same(first[0], whole[0]) and same(first[3], whole[3]), "into= must write in place"
    assert all(same(a, b) for a, b in zip(again, whole))
    before = [np.array(arr(t)) for t in (again[0], again[1], again[3])]
    be.integrate(color=color[:0], into=(again[0], again[1], again[3]), **split_frames(args, 0, 0, [0, 0]))
    assert all(RC.same_bits(a, b) or same(a, b) for a, b in zip(before, (again[0], again[1], again[3])))
    return whole


def check_into_errors(be):
    args = with_depth(case_args('dims_13x9x7'), False)
    color = case_color('dims_13x9x7', 3)
    D, w, _, Cv = be.integrate(color=color, **args)
    short = Cv[:-1].clone() if hasattr(Cv, 'clone') else np.array(Cv[:-1])
    wrong = Cv.double() if hasattr(Cv, 'double') else Cv.astype(np.float64)
    for into in ((D, w), (D, w, short), (D, w, wrong), (D, w, Cv, Cv)):
        with pytest.raises(ValueError):
            be.integrate(color=color, into=into, **args)
    with pytest.raises(ValueError):                                      # three channels into a one-channel call
        be.integrate(color=case_color('dims_13x9x7', 1), into=(D, w, Cv), **args)
    with pytest.raises(ValueError):                                      # a colour volume without colour frames
        be.integrate(into=(D, w, Cv), **args)
    if be.suffix == '':                                                  # the wrong device
        with pytest.raises(ValueError):
            be.integrate(color=color, into=(D, w, Cv.cpu()), **args)


# ---------------------------------------------------------- 2b. a batch of volumes, one of them frameless under into=
BATCH = ('dims_13x9x7', 'partly_outside', 'brick_face_17x9x9')      # 819, 11439 (45 workgroups) and 1377 voxels
BATCH_FIRST, BATCH_SECOND = ((0, 2, 3, 4), [0, 1, 3, 4]), ((1, 5), [0, 1, 1, 2])     # (frames, frame_start) of the split
BATCH_OBSERVED, BATCH_TWICE = (702, 542, 813), (689, 467, 809)      # voxels per volume with w > 0; seen by both frames


@functools.lru_cache(maxsize=None)
def batch_inputs(channels, f32):
    """(integrate arguments, colour, camera_to_volume) of the three volumes ``BATCH``, two frames of 37 x 23 each."""
    case = SC.batch_of(BATCH)
    inten = RC.small_intensity(np.asarray(case['depth']).shape)
    return with_depth(case, f32), (inten if channels == 1 else RC.to_rgb8(inten)), case['camera_to_volume']


def batch_frames(args, color, frames, frame_start):
    ix = list(frames)
    return dict(args, depth=args['depth'][ix], volume_to_camera=args['volume_to_camera'][ix],
                frame_start=frame_start), color[ix]


@functools.lru_cache(maxsize=None)
def batch_reference(channels, f32):
    """(D, w, vol_start, Cv) of the restatement for the whole call; shared."""
    args, color, _ = batch_inputs(channels, f32)
    return RCC.freeze(*NUMPY.integrate(color=color, **args))


@functools.lru_cache(maxsize=None)
def batch_host(channels, f32):
    """The whole call through the host twin; shared."""
    args, color, _ = batch_inputs(channels, f32)
    return HOST.integrate(color=color, **args)


def check_batch_into(be, channels, f32):
    """Colour over several volumes (v > 0 in the colour row's index) and a volume without a frame under ``into=``,
    dense and through the pool: the split call equals the whole call, which equals the restatement."""
    args, color, C = batch_inputs(channels, f32)
    whole = be.integrate(color=color, **args)
    plain = be.integrate(**args)
    ref = batch_reference(channels, f32)
    vs = [int(x) for x in arr(whole[2])]
    assert vs == [0, 819, 12258, 13635] and arr(whole[3]).shape == (vs[-1], channels)
    assert RC.same_bits(whole[0], plain[0]) and RC.same_bits(whole[1], plain[1]), "colour changed D or w"
    assert all(RC.same_bits(a, b) for a, b in zip((whole[0], whole[1], whole[3]), (ref[0], ref[1], ref[3])))
    w = arr(whole[1])
    assert tuple(int((w[a:b] > 0).sum()) for a, b in zip(vs, vs[1:])) == BATCH_OBSERVED
    assert tuple(int((w[a:b] == 2).sum()) for a, b in zip(vs, vs[1:])) == BATCH_TWICE
    a1, c1 = batch_frames(args, color, *BATCH_FIRST)
    a2, c2 = batch_frames(args, color, *BATCH_SECOND)
    first = be.integrate(color=c1, **a1)
    middle = [np.array(arr(t)[vs[1]:vs[2]]) for t in (first[0], first[1], first[3])]
    again = be.integrate(color=c2, into=(first[0], first[1], first[3]), **a2)
    for t, m in zip((again[0], again[1], again[3]), middle):
        assert RC.same_bits(arr(t)[vs[1]:vs[2]], m), "the volume without a frame changed"
    assert all(RC.same_bits(a, b) for a, b in zip((again[0], again[1], again[3]), (whole[0], whole[1], whole[3])))
    # the same through the pool
    frames, vol, rest = sparse_args(dict(args, camera_to_volume=C))
    sv = be.allocate(*frames, C, *vol)
    pool = be.sparse(*frames, args['volume_to_camera'], sv, *rest, color=color)
    p1 = be.sparse(a1['depth'], a1['frame_start'], frames[2], a1['volume_to_camera'], sv, *rest, color=c1)
    p2 = be.sparse(a2['depth'], a2['frame_start'], frames[2], a2['volume_to_camera'], sv, *rest, color=c2, into=p1)
    assert arr(pool[2]).shape == (sv.bricks, 512, channels)
    assert all(RC.same_bits(a, b) for a, b in zip(p2, pool))
    hs = host_tables(sv)
    dense = ops.tsdf_densify(np.array(arr(pool[0])), np.array(arr(pool[1])), hs, color=np.array(arr(pool[2])))
    inside = allocated_voxels(sv)
    assert inside.any() and not inside.all()
    assert (np.asarray(arr(sv.brick_coord)) * 8 + 7 >= np.repeat(sv.dims, np.diff(arr(sv.brick_start)), 0)).any(), \
        "no brick has a slot beyond dims"
    for got, want in zip((dense[0], dense[1], dense[3]), (ref[0], ref[1], ref[3])):
        assert RC.same_bits(got[inside], want[inside]) and not got[~inside].any()
    return whole, pool


# ----------------------------------------------------------------------------------------------------- 3. sparse
def sparse_args(args):
    a = S.integrate_args(args)
    frames = (a['depth'], a['frame_start'], a['intrinsics'])
    vol = (a['origin'], a['dims'], a['voxel'], a['trunc'], a['depth_scale'], a['depth_max'])
    return frames, vol, (a['trunc'], a['depth_scale'], a['depth_max'])


def allocated_voxels(sv):
    """bool [total]: the voxels of the dense layout that lie in an allocated brick."""
    ones = np.ones((sv.bricks, ops.TSDF_BRICK_VOXELS), dtype=np.float32)
    return ops.tsdf_densify(ones, ones, host_tables(sv))[0] > 0


def host_tables(sv):
    return ops.SparseVolumes(arr(sv.brick_index), arr(sv.brick_coord), arr(sv.brick_start), sv.origin, sv.dims,
                             sv.voxel)


def check_sparse(be, name, channels):
    args = case_args(name)
    frames, vol, rest = sparse_args(args)
    color = case_color(name, channels)
    sv = be.allocate(*frames, args['camera_to_volume'], *vol)
    D, w, Cp = be.sparse(*frames, args['volume_to_camera'], sv, *rest, color=color)
    D0, w0 = be.sparse(*frames, args['volume_to_camera'], sv, *rest)
    assert arr(Cp).shape == (sv.bricks, 512, channels) and RC.same_bits(D, D0) and RC.same_bits(w, w0)
    Dn, wn, _, Cn = reference(name, channels)
    hs = host_tables(sv)
    dense = ops.tsdf_densify(np.array(arr(D)), np.array(arr(w)), hs, color=np.array(arr(Cp)))
    inside = allocated_voxels(sv)
    assert same(dense[3][inside], Cn[inside]) and same(dense[1][inside], wn[inside])
    assert not dense[3][~inside].any()
    # the round trip through the dense layout, and the split over fixed tables
    ix = np.flatnonzero(inside)
    again = np.zeros_like(dense[3])
    again[ix] = Cn[ix]
    assert same(dense[3], again)
    F = frames[0].shape[0]
    if F >= 2 and sv.bricks:
        k = F // 2
        a = be.sparse(frames[0][:k], [0, k], frames[2], args['volume_to_camera'][:k], sv, *rest, color=color[:k])
        b = be.sparse(frames[0][k:], [0, F - k], frames[2], args['volume_to_camera'][k:], sv, *rest, color=color[k:],
                      into=a)
        assert all(same(x, y) for x, y in zip(b, (D, w, Cp)))
    return sv, D, w, Cp


def check_extend(be, name, channels):
    """The bricks of frame 0, then grown by frame 1: old rows move bit for bit, new rows are zero."""
    args = case_args(name)
    frames, vol, rest = sparse_args(args)
    color = case_color(name, channels)
    one = (frames[0][:1], [0, 1], frames[2])
    sv = be.allocate(*one, args['camera_to_volume'][:1], *vol)
    D, w, Cp = be.sparse(*one, args['volume_to_camera'][:1], sv, *rest, color=color[:1])
    sv2, D2, w2, Cp2 = be.extend(sv, D, w, frames[0][1:2], [0, 1], frames[2], args['camera_to_volume'][1:2], *rest,
                                 color=Cp)
    plain = be.extend(sv, D, w, frames[0][1:2], [0, 1], frames[2], args['camera_to_volume'][1:2], *rest)
    assert len(plain) == 3 and RC.same_bits(plain[1], D2) and RC.same_bits(plain[2], w2)
    assert arr(Cp2).shape == (sv2.bricks, 512, channels) and sv2.bricks >= sv.bricks
    old = ops.tsdf_densify(np.array(arr(D)), np.array(arr(w)), host_tables(sv), color=np.array(arr(Cp)))
    new = ops.tsdf_densify(np.array(arr(D2)), np.array(arr(w2)), host_tables(sv2), color=np.array(arr(Cp2)))
    assert same(old[3], new[3]) and same(old[1], new[1])          # zero outside the old bricks on both sides
    return sv.bricks, sv2.bricks


# --------------------------------------------------------------------------------------------------- 4. color_at
@functools.lru_cache(maxsize=None)
def lattice_case():
    """Two hand-made volumes -- 5 x 4 x 3 and 1 x 3 x 3 -- with seeded weights and colours, and hand-placed points.
    Returns (volume arguments, Cv [total,3], w [total], points f32 [N,3], point_start, what: name -> point index)."""
    rng = np.random.default_rng(7)
    dims = np.array([[5, 4, 3], [1, 3, 3]])
    origin = np.array([[0.05, -0.1, 0.2], [1.0, 1.0, 1.0]], dtype=np.float32)
    voxel = np.float32(0.1)
    total = 60 + 9
    w = rng.integers(1, 4, total).astype(np.float32)
    Cv = rng.uniform(0.0, 1.0, (total, 3)).astype(np.float32)
    at = lambda i, j, k: i + 5 * (j + 4 * k)
    for c in range(8):                                   # cell (3, 2, 1): only corner (4, 3, 2) keeps its weight
        i, j, k = 3 + (c & 1), 2 + ((c >> 1) & 1), 1 + (c >> 2)
        if c != 7:
            w[at(i, j, k)] = 0.0
    for c in range(8):                                   # cell (0, 0, 0): no corner has weight
        w[at(c & 1, (c >> 1) & 1, c >> 2)] = 0.0
    lat = lambda g, v=0: (origin[v] + voxel * np.asarray(g, dtype=np.float32)).astype(np.float32)
    pts, what = [], {}

    def add(name, p):
        what[name] = len(pts)
        pts.append(np.asarray(p, dtype=np.float32))
    add('vertex', lat((2, 1, 1)))
    add('inside', lat((1.3, 1.6, 0.4)))
    hi = np.array([4, 3, 2], dtype=np.float32)
    for a in range(3):
        g = np.array([1.5, 1.5, 0.5], dtype=np.float32)
        g[a] = hi[a]
        add('last_plane_%d' % a, lat(g))
        far = np.array(origin[0] + voxel * g, dtype=np.float64)
        far[a] = float(origin[0, a]) + float(voxel) * float(hi[a]) * (1.0 + 1e-5) + 1e-6
        add('outside_high_%d' % a, far)
        low = np.array(lat((1.5, 1.5, 0.5)))
        low[a] = np.nextafter(origin[0, a], np.float32(-np.inf))
        add('outside_low_%d' % a, low)
    add('one_corner', lat((3.4, 2.3, 1.6)))
    add('no_corner', lat((0.5, 0.5, 0.5)))
    add('nan', (np.nan, 0.1, 0.3))
    add('huge', (3e38, 0.1, 0.3))
    first = len(pts)
    add('flat_volume', lat((0, 1, 1), 1))
    pts = np.stack(pts).astype(np.float32)
    args = dict(origin=origin, dims=dims, voxel=voxel)
    for a in (w, Cv, pts):
        a.setflags(write=False)
    return args, Cv, w, pts, [0, first, len(pts)], what


def check_color_at(be, channels):
    args, Cv, w, pts, ps, what = lattice_case()
    Cv = np.ascontiguousarray(Cv[:, :channels])
    out = arr(be.sample(be.put(Cv), be.put(w), None, points=pts, point_start=ps, **args))
    ref = ops.tsdf_sample_color_numpy(Cv, w, None, points=pts, point_start=ps, **args)
    assert out.shape == (len(pts), channels) and same(out, ref)
    at = lambda i, j, k: i + 5 * (j + 4 * k)
    assert np.allclose(out[what['vertex']], Cv[at(2, 1, 1)], atol=1e-5)
    assert np.allclose(out[what['one_corner']], Cv[at(4, 3, 2)], atol=1e-6)
    for a in range(3):
        assert np.isfinite(out[what['last_plane_%d' % a]]).all()
        assert np.isnan(out[what['outside_high_%d' % a]]).all() and np.isnan(out[what['outside_low_%d' % a]]).all()
    for name in ('no_corner', 'nan', 'huge', 'flat_volume'):
        assert np.isnan(out[what[name]]).all(), name
    assert np.isfinite(out[what['inside']]).all()
    # min_weight above every weight: nothing has a colour
    none = arr(be.sample(be.put(Cv), be.put(w), None, points=pts, point_start=ps, min_weight=10.0, **args))
    assert np.isnan(none).all()
    return out


@functools.lru_cache(maxsize=None)
def brick_case():
    """A 20 x 20 x 20 lattice (3 x 3 x 3 bricks) with 5 of the 8 bricks around voxel (7, 7, 7) allocated and seeded
    pools, and points in the cells that straddle those bricks."""
    rng = np.random.default_rng(11)
    present = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 1), (1, 1, 1), (2, 2, 2)]
    index = np.full(27, -1, dtype=np.int32)
    coord = np.array(sorted(present, key=lambda b: b[0] + 3 * (b[1] + 3 * b[2])), dtype=np.int32)
    for rank, b in enumerate(coord):
        index[b[0] + 3 * (b[1] + 3 * b[2])] = rank
    sv = ops.SparseVolumes(index, coord, np.array([0, len(coord)], dtype=np.int64),
                           np.array([[-0.3, 0.1, 0.5]], dtype=np.float32), np.array([[20, 20, 20]], dtype=np.int32),
                           np.array([0.05], dtype=np.float32))
    w = rng.integers(0, 3, (len(coord), 512)).astype(np.float32)
    Cp = rng.uniform(0.0, 1.0, (len(coord), 512, 3)).astype(np.float32)
    g = np.concatenate([rng.uniform(6.5, 8.5, (40, 3)), rng.uniform(0.0, 19.0, (40, 3)),
                        [[7.5, 7.5, 7.5], [7.0, 7.0, 7.0], [19.0, 19.0, 19.0], [15.5, 15.5, 15.5]]])
    pts = (sv.origin[0] + sv.voxel[0] * g.astype(np.float32)).astype(np.float32)
    return sv, Cp, w, pts, [0, len(pts)]


def check_color_at_sparse(be, channels):
    sv, Cp, w, pts, ps = brick_case()
    Cp = np.ascontiguousarray(Cp[..., :channels])
    out = arr(be.sample_sparse(be.put(Cp), be.put(w), sv, pts, ps))
    _, wd, vs, Cv = ops.tsdf_densify(w, w, sv, color=Cp)
    ref = ops.tsdf_sample_color_numpy(Cv, wd, vs, sv.origin, sv.dims, sv.voxel, pts, ps)
    assert same(out, ref) and same(out, ops.tsdf_sample_color_sparse_numpy(Cp, w, sv, pts, ps))
    assert np.isfinite(out[:40]).all(1).any() and np.isnan(out).all(1).any()
    return out


# ---------------------------------------------------------------------------------------------------- 5. ray-cast
VOLUME_OF = {'room': 'room12', 'camera_inside': 'room12', 'misses': 'room12', 'nan_pose': 'room12',
             'depth_max': 'room12', 'no_views': 'room12', 'one_frame_min_weight_2': 'room1', 'two_volumes': 'fragments'}
THREE_CHANNELS = ('room', 'small_dims_13x9x7', 'two_volumes')


@functools.lru_cache(maxsize=None)
def painted_volume(key, channels):
    """The volume ``key`` fused with colour by the host twins, dense and sparse: dict(Cv, sv, Dp, wp, Cp, frames)."""
    if key.startswith('room'):
        frames = int(key[4:])
        a = dict(room_args())
        a.update(depth=a['depth'][:frames], volume_to_camera=a['volume_to_camera'][:frames],
                 camera_to_volume=a['camera_to_volume'][:frames], frame_start=[0, frames])
        vol = RCC.room_volume(frames)
        a.update(origin=vol['origin'], dims=vol['dims'])
        color = (RC.room()[3] if channels == 1 else RC.room()[4])[:frames]
    elif key == 'fragments':
        depth, fs, K, M, C = S.fragment_setup()
        vol = RCC.fragment_volumes()[0]
        a = dict(depth=depth, frame_start=fs, intrinsics=K, volume_to_camera=M, camera_to_volume=C,
                 origin=vol['origin'], dims=vol['dims'], voxel=S.VOXEL, trunc=S.TRUNC, depth_scale=1000.0, depth_max=6.0)
        color = RC.room()[3] if channels == 1 else RC.room()[4]
    else:
        a = S.small_cases()[key]
        vol = RCC.small_volume(key)
        color = case_color(key, channels)
    D, w, _, Cv = ops.tsdf_integrate_host(color=color, **S.integrate_args(a))
    assert RC.same_bits(D, vol['D']) and RC.same_bits(w, vol['w'])          # the volume of raycast_cases, painted
    frames, lattice, rest = sparse_args(a)
    sv = host_tables(ops.tsdf_allocate_host(*frames, a['camera_to_volume'], *lattice))
    Dp, wp, Cp = (arr(t) for t in ops.tsdf_integrate_sparse_host(*frames, a['volume_to_camera'], sv, *rest, color=color))
    return dict(Cv=RCC.freeze(Cv.numpy())[0], sv=sv, Dp=Dp, wp=wp, Cp=Cp)


def drop_brick(sv, row, *pools):
    """Host tables ``sv`` and their pools without pool row ``row``: the brick is absent, as if it had never been
    allocated."""
    index, coord, start = (np.array(arr(a)) for a in (sv.brick_index, sv.brick_coord, sv.brick_start))
    v = int(np.searchsorted(start, row, side='right')) - 1
    part = index[sv.lattice_start[v]:sv.lattice_start[v + 1]]           # a view: the volume's part of the table
    rank = row - start[v]
    part[part == rank] = -1
    part[part > rank] -= 1
    start[v + 1:] -= 1
    return (ops.SparseVolumes(index, np.delete(coord, row, axis=0), start, sv.origin, sv.dims, sv.voxel),) + \
        tuple(np.delete(arr(a), row, axis=0) for a in pools)


FOLD_CASES = ('fold_1', 'fold_3')          # names of fold_case(channels) among the ray-cast cases


@functools.lru_cache(maxsize=None)
def fold_case(channels):
    """The one case that drives every instantiation of the single ray-cast body and the single sampling body of
    csrc/tsdf_raycast.hip (dense and sparse; no colour, one channel, three) through the places a shared pixel prologue
    can go wrong.  Two volumes, 13 x 9 x 7 (2 x 2 x 1 bricks, their borders at index 7 | 8 on two axes) and 5 x 1 x 4
    (no cell along y), fused with colour by the host twins from the two small frames each; three views in the order
    1, 0, 1 of 19 x 21 pixels: two blocks of 16 x 16 each way, with partial 8 x 8 tiles in both; the sparse form with
    one allocated brick of the first volume taken out of the tables.  Returns (ray-cast arguments, dict(Cv, sv, Dp, wp,
    Cp), channels, points f32 [40,3], point_start): 32 points of the first volume, one of them outside its lattice
    and one NaN, and 8 of the second."""
    small = S.small_cases()['dims_13x9x7']
    twice = lambda a: np.concatenate([np.asarray(a)] * 2)
    a = dict(small, depth=twice(small['depth']), frame_start=[0, 2, 4], volume_to_camera=twice(small['volume_to_camera']),
             camera_to_volume=twice(small['camera_to_volume']),
             origin=np.array([[-0.3, -0.2, 0.9], [-0.1, 0.0, 0.95]], dtype=np.float32), dims=np.array([[13, 9, 7], [5, 1, 4]]))
    inten = RC.small_intensity(a['depth'].shape)
    color = inten if channels == 1 else RC.to_rgb8(inten)
    D, w, vs, Cv = (arr(t) for t in ops.tsdf_integrate_host(color=color, **S.integrate_args(a)))
    frames, lattice, rest = sparse_args(a)
    sv = host_tables(ops.tsdf_allocate_host(*frames, a['camera_to_volume'], *lattice))
    pools = ops.tsdf_integrate_sparse_host(*frames, a['volume_to_camera'], sv, *rest, color=color)
    assert int(arr(sv.brick_start)[1]) == 4, "the four lattice bricks of the first volume are allocated"
    sv, Dp, wp, Cp = drop_brick(sv, 3, *pools)        # brick (1, 1, 0): the voxels with ix >= 8 and iy = 8
    C = np.asarray(small['camera_to_volume'])
    case = dict(D=D, w=w, vol_start=vs, origin=a['origin'], dims=a['dims'], voxel=a['voxel'], trunc=a['trunc'],
                intrinsics=np.array([30.0, 30.0, 9.0, 15.0]), camera_to_volume=np.stack([C[0], C[1], C[0]]), height=21,
                width=19, view_volume=[1, 0, 1])
    rng = np.random.default_rng(5)
    g = np.concatenate([rng.uniform(0.0, 1.0, (29, 3)) * [12.0, 8.0, 6.0], [[10.5, 7.5, 3.5]], [[12.5, 4.0, 3.0], [np.nan, 1.0, 1.0]],
                        rng.uniform(0.0, 1.0, (8, 3)) * [4.0, 0.0, 3.0]])
    own = np.repeat([0, 1], [32, 8])
    pts = (a['origin'][own] + np.float32(a['voxel']) * g.astype(np.float32)).astype(np.float32)
    RCC.freeze(D, w, Cv, Dp, wp, Cp, pts)
    return case, dict(Cv=Cv, sv=sv, Dp=Dp, wp=wp, Cp=Cp), channels, pts, [0, 32, 40]


def check_fold_points(be, channels):
    """The points of ``fold_case`` through the dense and the sparse sampler: each equals the restatement."""
    case, vol, _, pts, ps = fold_case(channels)
    lattice = {k: case[k] for k in ('vol_start', 'origin', 'dims', 'voxel')}
    dense = arr(be.sample(be.put(vol['Cv']), be.put(case['w']), points=pts, point_start=ps, **lattice))
    sparse = arr(be.sample_sparse(be.put(vol['Cp']), be.put(vol['wp']), vol['sv'], pts, ps))
    assert dense.shape == sparse.shape == (40, channels)
    assert same(dense, ops.tsdf_sample_color_numpy(vol['Cv'], case['w'], points=pts, point_start=ps, **lattice))
    assert same(sparse, ops.tsdf_sample_color_sparse_numpy(vol['Cp'], vol['wp'], vol['sv'], pts, ps))
    assert np.isnan(dense[30:]).all() and np.isnan(sparse[30:]).all()      # outside, NaN, and the volume without a cell
    assert np.isfinite(dense[:30]).all(1).any() and np.isfinite(sparse[:30]).all(1).any()
    assert not same(dense, sparse), "the dropped brick holds none of the points"
    return dense, sparse


def raycast_case(name):
    if name in FOLD_CASES:
        return fold_case(int(name[-1]))[:3]
    channels = 3 if name in THREE_CHANNELS else 1
    key = VOLUME_OF.get(name) or name[len('small_'):]
    return RCC.cases()[name], painted_volume(key, channels), channels


@functools.lru_cache(maxsize=None)
def raycast_reference(name):
    """(depth, normals, colour) of the restatement for a case of ``raycast_cases.cases()``; shared."""
    case, vol, _ = raycast_case(name)
    return ops.tsdf_raycast_numpy(normals=True, color=vol['Cv'], **case)


def check_raycast(be, name):
    case, vol, channels = raycast_case(name)
    views = {k: v for k, v in case.items() if k not in ('D', 'w')}
    D, w, Cv = be.put(case['D']), be.put(case['w']), be.put(vol['Cv'])
    d0, n0 = be.raycast(D, w, normals=True, **views)
    d1, n1, c1 = be.raycast(D, w, normals=True, color=Cv, **views)
    d2, c2 = be.raycast(D, w, color=Cv, clip=False, **views)
    dn, nn, cn = raycast_reference(name)
    R = len(case['view_volume'])
    assert arr(c1).shape == (R, case['height'], case['width'], channels)
    assert RC.same_bits(d0, d1) and RC.same_bits(n0, n1), "colour changed depth or normals"
    assert same(d1, dn) and same(n1, nn) and same(c1, cn)
    assert same(d2, d1) and same(c2, c1), "the clip changed a bit"
    assert np.array_equal(np.isnan(arr(c1)).any(-1), arr(d1) == 0) and np.array_equal(np.isnan(arr(c1)).all(-1),
                                                                                    arr(d1) == 0)
    # sparse: the colour of the densified pool, skip on and off
    lattice = ('vol_start', 'origin', 'dims', 'voxel')
    sviews = {k: v for k, v in views.items() if k not in lattice}
    Dp, wp, Cp = be.put(vol['Dp']), be.put(vol['wp']), be.put(vol['Cp'])
    s0 = be.raycast_sparse(Dp, wp, vol['sv'], normals=True, **sviews)
    s1 = be.raycast_sparse(Dp, wp, vol['sv'], normals=True, color=Cp, **sviews)
    s2 = be.raycast_sparse(Dp, wp, vol['sv'], color=Cp, skip=False, **sviews)
    assert RC.same_bits(s0[0], s1[0]) and RC.same_bits(s0[1], s1[1]) and same(s2[0], s1[0]) and same(s2[1], s1[2])
    dense = ops.tsdf_densify(vol['Dp'], vol['wp'], vol['sv'], color=vol['Cp'])
    ref = ops.tsdf_raycast_numpy(dense[0], dense[1], color=dense[3], **views)
    assert same(s1[0], ref[0]) and same(s1[2], ref[1])
    assert np.array_equal(np.isnan(arr(s1[2])).all(-1), arr(s1[0]) == 0)
    return arr(d1), arr(c1)


def check_view_alone_batch_reversed_rerun(be):
    case, vol, _ = raycast_case('room')
    views = {k: v for k, v in case.items() if k not in ('D', 'w')}
    D, w, Cv = be.put(case['D']), be.put(case['w']), be.put(vol['Cv'])
    whole = arr(be.raycast(D, w, color=Cv, **views)[1])
    again = arr(be.raycast(D, w, color=Cv, **views)[1])
    back = arr(be.raycast(D, w, color=Cv, **dict(views, camera_to_volume=views['camera_to_volume'][::-1]))[1])
    assert same(whole, again) and same(whole, back[::-1])
    for r in range(3):
        one = dict(views, camera_to_volume=views['camera_to_volume'][r:r + 1], view_volume=[0])
        assert same(arr(be.raycast(D, w, color=Cv, **one)[1])[0], whole[r])


# ---------------------------------------------------------------------------------------------------- 6. accuracy
# the restatement's figures on the room, computed on the CPU (tests/test_tsdf_color_cpu.py checks them): the median and
# the maximum of |colour - tex| of the render and of the extracted cloud
RENDER_MEDIAN, RENDER_MAX = 0.00247, 0.16057
CLOUD_MEDIAN, CLOUD_MAX = 0.003135, 0.22351


def room_truth():
    """Per room view: (analytic depth f64 [H,W], tex at the analytic surface point f64 [H,W])."""
    out = []
    for P in RCC.room_view_poses():
        d = S.render(P)
        pts = S.to_world(RC.back_project(d, S.K).reshape(-1, 3), P)
        out.append((d, RC.tex(pts[:, 0], pts[:, 1], pts[:, 2]).reshape(d.shape)))
    return out


def render_errors(depth, colour):
    """(|rendered intensity - tex| at the hit pixels within one voxel of the analytic depth, the excluded fraction)."""
    errs, hits, kept = [], 0, 0
    for r, (d, t) in enumerate(room_truth()):
        hit = depth[r] > 0
        ok = hit & (np.abs(depth[r] - d) <= S.VOXEL)
        hits, kept = hits + int(hit.sum()), kept + int(ok.sum())
        errs.append(np.abs(colour[r, ..., 0].astype(np.float64) - t)[ok])
    return np.concatenate(errs), 1.0 - kept / float(hits)


def room_intensity_volume():
    return RCC.cases()['room'], painted_volume('room12', 1)


def check_render_accuracy(be, median_ref, max_ref):
    case, vol = room_intensity_volume()
    views = {k: v for k, v in case.items() if k not in ('D', 'w')}
    d, c = be.raycast(be.put(case['D']), be.put(case['w']), color=be.put(vol['Cv']), **views)
    err, excluded = render_errors(arr(d), arr(c))
    print("%s render: median %.5f max %.5f over %d pixels, %.2f %% excluded" % (be.name, np.median(err), err.max(),
                                                                               err.size, 100 * excluded))
    assert excluded < 0.03
    assert np.median(err) <= 1.5 * median_ref and err.max() <= 1.5 * max_ref
    return np.median(err), err.max(), excluded


def cloud_errors(be):
    case, vol = room_intensity_volume()
    lattice = dict(origin=case['origin'], dims=case['dims'], voxel=case['voxel'])
    D, w = be.put(case['D']), be.put(case['w'])
    pts, ps = be.extract(D, w, None, **lattice)
    col = arr(be.sample(be.put(vol['Cv']), w, None, points=pts, point_start=ps, **lattice))
    world = S.to_world(arr(pts).astype(np.float64), S.sequence()[2][0])
    assert np.isfinite(col).all()                        # an extracted point lies between two weighted voxels
    return np.abs(col[:, 0].astype(np.float64) - RC.tex(world[:, 0], world[:, 1], world[:, 2]))


def check_cloud_accuracy(be, median_ref, max_ref):
    err = cloud_errors(be)
    print("%s cloud: median %.5f max %.5f over %d points" % (be.name, np.median(err), err.max(), err.size))
    assert np.median(err) <= 1.5 * median_ref and err.max() <= 1.5 * max_ref
    return np.median(err), err.max()


# ---------------------------------------------------------------------------------------------------- 7. products
def rows_set(points, colors):
    both = np.concatenate([np.asarray(points, dtype=np.float32), np.asarray(colors, dtype=np.float32)], axis=1)
    return set(map(bytes, np.ascontiguousarray(both).view(np.uint32)))


def product_inputs():
    depth, K, poses, _, rgb = RC.room()
    return depth, K, poses, rgb


def check_products(device):
    depth, K, poses, rgb = product_inputs()
    kw = dict(frames_per_fragment=S.PER_FRAGMENT, voxel=S.VOXEL, trunc=S.TRUNC, device=device)
    plain = fr.fuse_fragments(depth, K, poses, **kw)
    clouds, fposes, colors = fr.fuse_fragments(depth, K, poses, color=rgb, **kw)
    assert len(plain) == 2 and len(clouds) == len(colors) == 2
    for a, b, c in zip(plain[0], clouds, colors):
        assert RC.same_bits(a, b) and c.shape == (b.shape[0], 3) and c.dtype == np.float32
        assert np.isfinite(c).all() and c.min() >= 0.0 and c.max() <= 1.0
    sc, _, scol = fr.fuse_fragments(depth, K, poses, color=rgb, sparse=True, **kw)
    for g in range(2):
        assert rows_set(clouds[g], colors[g]) == rows_set(sc[g], scol[g])
    _, _, meshes, mcol = fr.mesh_fragments(depth, K, poses, color=rgb, **kw)
    dm = fr.fuse_fragments(depth, K, poses, color=rgb, mesh=True, **kw)
    assert len(dm) == 4 and len(fr.mesh_fragments(depth, K, poses, **kw)[2][0]) == 3
    for g in range(2):
        assert len(meshes[g]) == 4 and meshes[g][3].shape == (meshes[g][0].shape[0], 3)
        assert rows_set(meshes[g][0], meshes[g][3]) == rows_set(dm[2][g][0], dm[2][g][3])
        assert rows_set(sc[g], scol[g]) == rows_set(sc[g], mcol[g])
    grey = fr.fuse_fragments(depth, K, poses, color=RC.room()[3], **kw)[2]
    assert grey[0].shape == (clouds[0].shape[0], 1)
    scene = fr.fuse_scene(depth, K, poses, fposes, color=rgb, **kw)
    assert len(scene) == 2 and scene[1].shape == (scene[0].shape[0], 3)
    return clouds, colors, meshes


def check_max_bytes(device):
    """One byte under ``8 + 4 Cc`` per voxel of the larger fragment raises before anything is launched."""
    depth, K, poses, rgb = product_inputs()
    dims = RCC.fragment_volumes()[0]['dims']
    voxels = int(max(int(n[0]) * int(n[1]) * int(n[2]) for n in dims))
    kw = dict(frames_per_fragment=S.PER_FRAGMENT, voxel=S.VOXEL, trunc=S.TRUNC, device=device)
    fr.fuse_fragments(depth, K, poses, max_bytes=8 * voxels, **kw)                    # the colourless volume fits
    fr.fuse_fragments(depth, K, poses, color=rgb, max_bytes=20 * voxels, **kw)
    with pytest.raises(ValueError, match="max_bytes"):
        fr.fuse_fragments(depth, K, poses, color=rgb, max_bytes=20 * voxels - 1, **kw)
    with pytest.raises(ValueError, match="max_bytes"):
        fr.fuse_fragments(depth, K, poses, color=RC.room()[3], max_bytes=12 * voxels - 1, **kw)


def check_ply(tmp_path, clouds, colors, meshes):
    from d3feat_pytorch_amd.datasets.ThreeDMatch import read_ply_points
    name = str(tmp_path / "cloud.ply")
    fr.write_ply_points(name, clouds[0], colors[0])
    assert np.array_equal(read_ply_points(name).astype(np.float32), clouds[0])
    head = open(name, 'rb').read(400)
    assert b"property uchar red" in head and b"property uchar blue" in head
    raw = np.fromfile(name, dtype=np.uint8)[-15 * clouds[0].shape[0]:].reshape(-1, 15)[:, 12:]
    assert np.array_equal(raw, np.rint(np.clip(colors[0].astype(np.float64), 0, 1) * 255).astype(np.uint8))
    vert, norm, face, vcol = meshes[0]
    fr.write_ply_mesh(name, vert, face, norm, colors=vcol)
    assert np.array_equal(read_ply_points(name).astype(np.float32), vert)
    fr.write_ply_points(name, clouds[0])
    assert b"red" not in open(name, 'rb').read(200)


# ---------------------------------------------------------------------------------------------------- 8. tracking
SLIDE_STEP = RC._rigid(0.5, (0.010, -0.006, 0.0))       # 0.5 degrees about the optical axis and (10, -6, 0) mm
SLIDE_MODEL = dict(frames_per_fragment=6, voxel=0.02)


@functools.lru_cache(maxsize=None)
def slide6():
    """(depth uint16 [6,48,64], K, intensity f32 [6,48,64], poses [6,4,4]): six views of the textured plane z = 1, each
    moved by ``SLIDE_STEP`` from the last; the depth is 1000 everywhere."""
    poses = [np.eye(4)]
    for _ in range(5):
        poses.append(poses[-1] @ SLIDE_STEP)
    depth = np.full((6, RC.SLIDE_H, RC.SLIDE_W), 1000, dtype=np.uint16)
    inten = RC.paint(depth, RC.SLIDE_K, poses)
    return RCC.freeze(depth, RC.SLIDE_K.copy(), inten, np.stack(poses))


@functools.lru_cache(maxsize=None)
def track_slide(device, sparse, color):
    depth, K, inten, _ = slide6()
    return fr.track_sequence(depth, K, color=inten, device=device, model=dict(SLIDE_MODEL, sparse=sparse, color=color))


@functools.lru_cache(maxsize=None)
def track_slide_pairs(device):
    depth, K, inten, _ = slide6()
    return fr.track_sequence(depth, K, color=inten, device=device)


def slide_errors(device, sparse):
    """((deg, mm) of the last frame under the colour model, the same under frame-to-frame RGB-D)."""
    truth = slide6()[3][5]
    model = OC.pose_error(track_slide(device, sparse, True)[0][5], truth)
    pairs = OC.pose_error(track_slide_pairs(device)[0][5], truth)
    print("%s slide (sparse=%s): colour model %.4f deg / %.4f mm; frame-to-frame RGB-D %.4f deg / %.4f mm" % (
        device, sparse, model[0], model[1], pairs[0], pairs[1]))
    return model, pairs


ROOM_MODEL = dict(frames_per_fragment=S.FRAMES, voxel=S.VOXEL)


@functools.lru_cache(maxsize=None)
def track_noisy_room(device, sparse):
    _, K, _, inten, _ = RC.room()
    return fr.track_sequence(RCC.noisy_depth(), K, color=inten, device=device, model=dict(ROOM_MODEL, sparse=sparse))


@functools.lru_cache(maxsize=None)
def track_noisy_room_pairs(device):
    _, K, _, inten, _ = RC.room()
    return fr.track_sequence(RCC.noisy_depth(), K, color=inten, device=device)


def room_errors(device, sparse):
    poses = S.sequence()[2]
    truth = fr.rigid_inverse(poses[0]) @ poses[11]
    model = OC.pose_error(track_noisy_room(device, sparse)[0][11], truth)
    pairs = OC.pose_error(track_noisy_room_pairs(device)[0][11], truth)
    print("%s noisy room (sparse=%s): colour model %.4f deg / %.4f mm; frame-to-frame RGB-D %.4f deg / %.4f mm" % (
        device, sparse, model[0], model[1], pairs[0], pairs[1]))
    return model, pairs
