"""Inputs shared by the depth-odometry tests: the analytic room of ``tsdf_scene`` (12 frames of 80 x 60 with analytic
poses), its small images of 37 x 23 (odd dimensions: levels of 18 x 11 and 9 x 5, the 1024-pixel chunk not filled), a
5 x 5 image whose coarsest level is 1 x 1, a constant-depth pair whose normal equations are exactly singular, and two
views of the room at 272 x 244, whose level 0 has more chunks than a wave has lanes."""
import functools

import numpy as np

import tsdf_scene as S

LEVELS = 3
U53 = 2.0 ** -53


def relative(poses, a, b):
    """T that maps camera a's frame into camera b's, from camera-to-world poses."""
    return np.linalg.inv(poses[b]) @ poses[a]


def pose_error(T, T_true):
    """(degrees, millimetres) between two rigid 4x4."""
    D = np.linalg.inv(np.asarray(T_true, dtype=np.float64)) @ np.asarray(T, dtype=np.float64)
    c = np.clip((np.trace(D[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.degrees(np.arccos(c))), float(np.linalg.norm(D[:3, 3]) * 1000.0)


def room_pairs(stride=1):
    """(pairs [P,2] = (f + stride, f), T_true [P,4,4]) of the room."""
    _, _, poses = S.sequence()
    pairs = np.array([(f + stride, f) for f in range(S.FRAMES - stride)], dtype=np.int64)
    return pairs, np.stack([relative(poses, a, b) for a, b in pairs])


@functools.lru_cache(maxsize=None)
def small_inputs():
    """name -> keyword arguments of ``ops.depth_pyramid`` for the small images, and the pose they are evaluated at."""
    cases = S.small_cases()
    out = {}
    for name, key in (('raw', 'dims_13x9x7'), ('holes', 'holes'), ('f32_nan', 'f32_nan'), ('depth_max', 'depth_max')):
        c = cases[key]
        out[name] = dict(depth=c['depth'], intrinsics=S.SMALL_K, levels=LEVELS, depth_scale=c['depth_scale'],
                         depth_max=c['depth_max'])
    tiny = np.ascontiguousarray(cases['dims_13x9x7']['depth'][:, :5, :5])
    out['tiny_5x5'] = dict(depth=tiny, intrinsics=np.array([30.0, 30.0, 2.0, 2.0]), levels=LEVELS, depth_scale=1000.0,
                           depth_max=6.0)
    return out


def small_pose():
    """The camera-1-into-camera-0 pose of the small cases' two cameras (the images are not rendered from it: it is a
    second pose to associate under, not a pose to recover)."""
    C = S.small_cases()['dims_13x9x7']['camera_to_volume']
    return np.linalg.inv(C[0]) @ C[1]


def constant_pair():
    """Two f32 frames of 16 x 12 with d = 1.0 everywhere: normals exactly (0, 0, -1), so the columns of J for the
    rotation about z and the translations along x and y are exactly 0."""
    return dict(depth=np.ones((2, 12, 16), dtype=np.float32), intrinsics=np.array([20.0, 20.0, 7.5, 5.5]),
                levels=LEVELS)


WIDE_W, WIDE_H = 272, 244
WIDE_K = np.array([204.0, 204.0, 135.5, 121.5])
WIDE_PAIRS = np.array([(1, 0), (0, 1)])
CHUNK = 1024             # D3F_ODO_CHUNK: the consecutive raster pixels one workgroup sums


@functools.lru_cache(maxsize=None)
def wide():
    """(depth uint16 [2,244,272], K [4], T_true [2,4,4] of ``WIDE_PAIRS``): the room from its cameras 0 and 1 at
    272 x 244.  Level 0 has 66368 pixels = 64 chunks of 1024 and one of 832: a pair has more chunks than the 64 lanes
    that add them, and the last chunk is partly filled.  Shared, do not modify."""
    poses = [S.camera(0), S.camera(1)]
    depth = np.stack([S.to_raw(S.render(P, WIDE_W, WIDE_H, WIDE_K)) for P in poses])
    depth.setflags(write=False)
    return depth, WIDE_K.copy(), np.stack([relative(poses, a, b) for a, b in WIDE_PAIRS])


def chunk_counts(index):
    """int [P, chunks]: the accepted pixels (index >= 0) of every chunk of ``CHUNK`` raster pixels of an association
    index [P,H,W]."""
    ok = np.asarray(index).reshape(len(index), -1) >= 0
    pad = -ok.shape[1] % CHUNK
    return np.pad(ok, ((0, 0), (0, pad))).reshape(len(index), -1, CHUNK).sum(axis=2)


def step_cases():
    """(name, pyramid arguments, pairs, list of T [P,4,4]) for the association tests: at the identity and at a second
    pose, for every level."""
    depth, K, _ = S.sequence()
    pairs = np.array([(1, 0), (3, 0)])
    _, _, poses = S.sequence()
    Tt = np.stack([relative(poses, a, b) for a, b in pairs])
    yield 'room', dict(depth=depth, intrinsics=K, levels=LEVELS), pairs, [np.stack([np.eye(4)] * 2), Tt]
    for name, args in small_inputs().items():
        yield name, args, np.array([(1, 0)]), [np.eye(4)[None], small_pose()[None]]
    wd, wK, wT = wide()
    yield 'wide', dict(depth=wd, intrinsics=wK, levels=LEVELS), WIDE_PAIRS, [np.stack([np.eye(4)] * 2), wT]


def sum_bound(terms):
    """The summation bound of n f64 terms per entry, for TWO different orders: 2 (n - 1) 2^-53 sum |term|."""
    n = terms.shape[0]
    return 2.0 * max(n - 1, 0) * U53 * np.abs(terms).sum(axis=0)
