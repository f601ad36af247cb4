"""Inputs shared by the RGB-D odometry tests: a smooth analytic texture of world coordinates; the room of
``tsdf_scene`` painted with it (as f32 intensity and as uint8 RGB); the planar slide -- two 64 x 48 views of the
fronto-parallel plane z = 1, whose depth-only normal equations are singular -- the small odd images of
``odometry_cases``, each with a deterministic intensity, and its two wide views of the room, painted."""
import functools

import numpy as np

import odometry_cases as OC
import tsdf_scene as S

LEVELS = OC.LEVELS
SLIDE_W, SLIDE_H = 64, 48
SLIDE_K = np.array([60.0, 60.0, 31.5, 23.5])


def tex(X, Y, Z):
    """A smooth texture of world coordinates (metres): four sinusoids whose amplitudes sum to 0.4 around 0.5, so the
    values stay inside [0.1, 0.9]."""
    return (0.5 + 0.14 * np.sin(17.0 * X + 0.3) + 0.13 * np.sin(19.0 * Y + 1.1) + 0.08 * np.sin(13.0 * Z + 0.7)
            + 0.05 * np.sin(11.0 * (X + Y + Z)))


def back_project(depth_m, K):
    """f64 [H,W,3]: camera-frame points of a depth image in metres."""
    h, w = depth_m.shape
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    return np.stack([(u - K[2]) / K[0] * depth_m, (v - K[3]) / K[1] * depth_m, depth_m], axis=-1)


def paint(depth_raw, K, poses):
    """f32 [F,H,W]: ``tex`` at the world point of every pixel's back-projected depth under the camera-to-world pose."""
    out = []
    for d, P in zip(depth_raw, poses):
        pts = S.to_world(back_project(d.astype(np.float64) / 1000.0, K).reshape(-1, 3), P)
        out.append(tex(pts[:, 0], pts[:, 1], pts[:, 2]).reshape(d.shape))
    return np.stack(out).astype(np.float32)


def to_rgb8(intensity):
    """uint8 [F,H,W,3]: a colour image whose channels differ a little, about as bright as ``intensity``."""
    v = np.clip(intensity.astype(np.float64), 0.0, 1.0)
    rgb = np.stack([v * 255.0, v * 250.0 + 3.0, v * 240.0 + 9.0], axis=-1)
    return np.rint(rgb).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def room():
    """(depth uint16 [12,60,80], K [4], poses, intensity f32 [12,60,80], rgb uint8 [12,60,80,3]); shared, do not
    modify."""
    depth, K, poses = S.sequence()
    inten = paint(depth, K, poses)
    rgb = to_rgb8(inten)
    inten.setflags(write=False)
    rgb.setflags(write=False)
    return depth, K, poses, inten, rgb


@functools.lru_cache(maxsize=None)
def wide():
    """(depth uint16 [2,244,272], K [4], T_true [2,4,4], intensity f32 [2,244,272]): ``odometry_cases.wide`` painted
    with ``tex``; shared, do not modify."""
    depth, K, T_true = OC.wide()
    inten = paint(depth, K, [S.camera(0), S.camera(1)])
    inten.setflags(write=False)
    return depth, K, T_true, inten


def _rigid(angle_deg, t):
    a = np.radians(angle_deg)
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T[:3, 3] = t
    return T


SLIDE_T = (_rigid(1.0, (0.012, -0.007, 0.0)),      # 1 degree about the optical axis and (12, -7, 0) mm
           _rigid(0.0, (-0.009, 0.011, 0.0)))      # a pure translation along the plane


@functools.lru_cache(maxsize=None)
def slide():
    """(depth uint16 [3,48,64], K [4], intensity f32 [3,48,64], pairs [2,2], T_true [2,4,4]): frame 0 is the fixed
    view of the plane z = 1 (depth quantised to 1 mm: 1000 everywhere), frames 1 and 2 the views moved by ``SLIDE_T``
    (T maps the moving camera's frame into frame 0's, the texture lives in frame 0's coordinates).  The plane stays
    fronto-parallel at z = 1 in every view, so the depth images are equal and only the texture moves."""
    depth = np.full((3, SLIDE_H, SLIDE_W), 1000, dtype=np.uint16)
    poses = [np.eye(4)] + list(SLIDE_T)
    inten = paint(depth, SLIDE_K, poses)
    inten.setflags(write=False)
    depth.setflags(write=False)
    return depth, SLIDE_K.copy(), inten, np.array([(1, 0), (2, 0)]), np.stack(SLIDE_T)


def small_intensity(shape, bad=False):
    """f32 [F,H,W]: a deterministic intensity for small images; ``bad`` plants a NaN in frame 0 and an infinity in
    frame 1 (at pixels (u, v) = (7, 3) and (9, 2) when the image is large enough, else at (1, 1) and (2, 2))."""
    F, h, w = shape
    f, v, u = np.meshgrid(np.arange(F, dtype=np.float64), np.arange(h, dtype=np.float64),
                          np.arange(w, dtype=np.float64), indexing='ij')
    img = (0.5 + 0.25 * np.sin(0.55 * u + 0.2 * f) * np.cos(0.4 * v) + 0.1 * np.sin(0.3 * (u + v) + f)).astype(np.float32)
    if bad:
        (u0, v0), (u1, v1) = ((7, 3), (9, 2)) if w > 9 and h > 3 else ((1, 1), (2, 2))
        img[0, v0, u0] = np.nan
        img[1, v1, u1] = np.inf
    return img


BAD_PIXELS = {0: (7, 3), 1: (9, 2)}     # frame -> (u, v) of the non-finite pixel of small_intensity(..., bad=True)


@functools.lru_cache(maxsize=None)
def small_inputs():
    """name -> (keyword arguments of ``ops.depth_pyramid``, colour) for the small images of ``odometry_cases``: f32
    intensity, uint8 grey for 'holes', uint8 RGB for 'depth_max', and 'raw_bad' = 'raw' with a NaN and an infinity in
    the intensity."""
    out = {}
    for name, args in OC.small_inputs().items():
        shape = np.asarray(args['depth']).shape
        inten = small_intensity(shape)
        if name == 'holes':
            color = np.rint(inten * 255.0).astype(np.uint8)
        elif name == 'depth_max':
            color = to_rgb8(inten)
        else:
            color = inten
        out[name] = (args, color)
    raw = OC.small_inputs()['raw']
    out['raw_bad'] = (raw, small_intensity(np.asarray(raw['depth']).shape, bad=True))
    return out


def step_cases():
    """(name, pyramid arguments, colour, pairs, list of T [P,4,4]): ``odometry_cases.step_cases`` with colour."""
    depth, K, poses, inten, _ = room()
    pairs = np.array([(1, 0), (3, 0)])
    Tt = np.stack([OC.relative(poses, a, b) for a, b in pairs])
    yield 'room', dict(depth=depth, intrinsics=K, levels=LEVELS), inten, pairs, [np.stack([np.eye(4)] * 2), Tt]
    for name, (args, color) in small_inputs().items():
        yield name, args, color, np.array([(1, 0)]), [np.eye(4)[None], OC.small_pose()[None]]
    wd, wK, wT, wi = wide()
    yield ('wide', dict(depth=wd, intrinsics=wK, levels=LEVELS), wi, OC.WIDE_PAIRS,
           [np.stack([np.eye(4)] * 2), wT])


# ---------------------------------------------------------------------------------------------------------- checks
# The same properties are asked of the host twins (CPU tests) and of the kernels (GPU tests): a Backend names the
# functions of one of them; NUMPY is the restatement both are held against.
class Backend(object):
    def __init__(self, suffix):
        from d3feat_pytorch_amd import ops
        pick = lambda stem: getattr(ops, stem + suffix)
        self.name = suffix.strip('_') or 'device'
        self.depth_pyramid, self.depth_step, self.depth_odometry = (pick(s) for s in (
            'depth_pyramid', 'depth_odometry_step', 'depth_odometry'))
        self.pyramid, self.step, self.odometry = (pick(s) for s in ('rgbd_pyramid', 'rgbd_odometry_step',
                                                                    'rgbd_odometry'))


def arr(t):
    return t.cpu().numpy() if hasattr(t, 'cpu') else np.asarray(t)


def bits(a, dtype=np.float32):
    return np.ascontiguousarray(arr(a), dtype=dtype).view(np.uint32 if dtype == np.float32 else np.uint64)


def same_bits(a, b, dtype=np.float32):
    return bits(a, dtype).shape == bits(b, dtype).shape and np.array_equal(bits(a, dtype), bits(b, dtype))


def same_intensity(a, b):
    """Bit-equal where finite, the same infinities, and a NaN where the other has a NaN (a NaN's sign and payload are
    not part of the rule)."""
    a, b = arr(a), arr(b)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a)[~nan], bits(b)[~nan])


def errors(T, T_true):
    """f64 [P,2]: (degrees, millimetres) of every pair."""
    return np.array([OC.pose_error(arr(T)[p], T_true[p]) for p in range(len(T_true))])


def upper_to_matrix(sums):
    """The 6x6 sum J J^T of one row of sums."""
    A = np.zeros((6, 6))
    k = 1
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = sums[k]
            k += 1
    return A


def make_pyramid(be, args, color):
    """The RGB-D pyramid of the keyword arguments of ``ops.depth_pyramid`` and a colour."""
    rest = {k: v for k, v in args.items() if k not in ('depth', 'intrinsics')}
    return be.pyramid(args['depth'], color, args['intrinsics'], **rest)


def check_slide(be):
    """Item 1: the depth tracker is singular on the slide and keeps the identity; the RGB-D tracker at the default
    weight ends within a tenth of the starting error -- 0.1 deg and 1.39 mm for the first pair; the second pair starts
    with no rotation error, so it takes the first pair's 0.1 deg and a tenth of its own 14.2 mm."""
    from d3feat_pytorch_amd import ops
    depth, K, inten, pairs, T_true = slide()
    pyr = be.pyramid(depth, inten, K, LEVELS)
    T, count, _, status = (arr(x) for x in be.depth_odometry(pyr, pairs))
    assert status.tolist() == [ops.ODO_ST_SINGULAR] * 2 and not count.any()
    assert np.array_equal(T, np.stack([np.eye(4)] * 2))
    T, count, rmse, status, n_photo = (arr(x) for x in be.odometry(pyr, pairs))
    start, end = errors(np.stack([np.eye(4)] * 2), T_true), errors(T, T_true)
    print("%s slide: start %s end %s (deg, mm); n_photo %s of %s" % (be.name, start.tolist(), end.tolist(),
                                                                   n_photo.tolist(), count.tolist()))
    assert status.tolist() == [0, 0] and (n_photo > 0).all() and (n_photo <= count).all()
    assert abs(start[0, 0] - 1.0) < 1e-9 and abs(start[0, 1] - 13.892) < 1e-3
    assert end[0, 0] < 0.1 and end[0, 1] < 1.39
    assert end[1, 0] < 0.1 and end[1, 1] < start[1, 1] / 10.0
    return T


def check_room(be, color_kind):
    """Item 2: all 11 consecutive pairs of the room have status 0 and none ends more than twice as far from the
    analytic pose as the depth tracker's worst pair on the same frames (computed here from the depth tracker)."""
    depth, K, _, inten, rgb = room()
    pairs, T_true = OC.room_pairs()
    pyr = be.pyramid(depth, inten if color_kind == 'f32' else rgb, K, LEVELS)
    worst = errors(be.depth_odometry(pyr, pairs)[0], T_true).max(axis=0)
    T, count, rmse, status, n_photo = (arr(x) for x in be.odometry(pyr, pairs))
    end = errors(T, T_true).max(axis=0)
    print("%s room (%s): depth-only worst %.4f deg / %.4f mm; RGB-D worst %.4f deg / %.4f mm" % (
        be.name, color_kind, worst[0], worst[1], end[0], end[1]))
    assert not status.any() and (n_photo > 0).all() and (n_photo <= count).all()
    assert end[0] <= 2.0 * worst[0] and end[1] <= 2.0 * worst[1]
    return T


def check_pyramid(be, numpy_be, args, color):
    """Item 3: the depth part is the depth pyramid's bit for bit; the intensity equals the restatement's."""
    p, d, n = make_pyramid(be, args, color), be.depth_pyramid(**args), make_pyramid(numpy_be, args, color)
    assert same_bits(p.data, d.data) and same_bits(p.K, d.K) and np.array_equal(p.table, d.table)
    assert arr(p.intensity).shape == arr(p.data).shape == n.intensity.shape
    assert same_intensity(p.intensity, n.intensity)
    return p, n


def check_step(be, numpy_be, case, twin=None):
    """Item 4, per level at the identity and at a second pose: the index is the depth step's; the 31 sums agree with
    the restatement's -- and with those of ``twin``, the host twin when ``be`` is the device -- within the summation
    bound of the restatement's per-pixel terms; n_photo <= n.  Returns the photometric rows seen."""
    name, args, color, pairs, poses = case
    pb, pn = make_pyramid(be, args, color), make_pyramid(numpy_be, args, color)
    pt = make_pyramid(twin, args, color) if twin is not None else None
    photo = 0
    for level in range(LEVELS):
        for T in poses:
            s, idx = be.step(pb, pairs, T, level, return_index=True)
            _, idx_d = be.depth_step(pb, pairs, T, level, return_index=True)
            sn, idx_n, terms = numpy_be.step(pn, pairs, T, level, return_index=True, return_terms=True)
            s = arr(s)
            assert np.array_equal(arr(idx), arr(idx_d)) and np.array_equal(arr(idx), idx_n)
            assert s.shape == (len(pairs), 31) and np.isfinite(s).all()
            for p in range(len(pairs)):
                assert s[p, 0] == sn[p, 0] == (idx_n[p] >= 0).sum() and s[p, 29] == sn[p, 29] <= s[p, 0]
                assert terms[p].shape == (int(sn[p, 0] + sn[p, 29]), 31)
                assert (np.abs(s[p] - sn[p]) <= OC.sum_bound(terms[p])).all(), (name, level, p)
                if pt is not None:
                    st = arr(twin.step(pt, pairs, T, level))
                    assert st[p, 0] == s[p, 0] and st[p, 29] == s[p, 29]
                    assert (np.abs(s[p] - st[p]) <= OC.sum_bound(terms[p])).all(), (name, level, p)
                photo += int(s[p, 29])
    return photo


def check_weight_zero(be, pyr, pairs, T_init=None):
    """Item 5: photo_weight = 0 gives the depth tracker's poses, counts, rmse and statuses bit for bit."""
    a = [arr(x) for x in be.depth_odometry(pyr, pairs, T_init)]
    b = [arr(x) for x in be.odometry(pyr, pairs, T_init, photo_weight=0.0)]
    assert same_bits(a[0], b[0], np.float64) and same_bits(a[2], b[2], np.float64)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3]) and not b[4].any()
    return a[3]


def check_information(be, exact=True):
    """Item 7: the information matrix is the combined sum J J^T of the association at level 0 under the final pose,
    symmetric, and of full rank on the slide, where the depth-only matrix has rank 3."""
    depth, K, inten, pairs, _ = slide()
    pyr = be.pyramid(depth, inten, K, LEVELS)
    T, _, _, status, info, n_photo = (arr(x) for x in be.odometry(pyr, pairs, return_information=True))
    assert not status.any() and info.shape == (2, 6, 6)
    sums = arr(be.step(pyr, pairs, T, 0))
    geo = arr(be.depth_step(pyr, pairs, T, 0))
    for p in range(2):
        A = upper_to_matrix(sums[p])
        assert np.array_equal(info[p], info[p].T) and sums[p, 29] == n_photo[p]
        assert np.array_equal(info[p], A) if exact else np.allclose(info[p], A, rtol=1e-9, atol=0.0)
        assert np.linalg.matrix_rank(info[p]) == 6 and np.linalg.matrix_rank(upper_to_matrix(geo[p])) == 3
