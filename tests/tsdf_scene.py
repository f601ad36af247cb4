"""An analytic room with an exact ray-cast depth renderer, shared by the TSDF tests: no mesh, no file.

The box [0,1.6] x [0,1.2] x [0,1.6] m seen from inside plus a sphere of radius 0.3 at C = (0.9, 0.45, 0.8); images of
80 x 60 with fx = fy = 60, cx = 39.5, cy = 29.5; depth = z-depth rounded to millimetres (uint16).  Twelve cameras
eye_i = (0.25 + 0.04 i, 0.6 + 0.01 i, 0.25 + 0.01 i) looking at C + (0, 0.01 i, 0.01 i), y up.  Two fragments of six
frames, voxel 0.02, trunc = 4 voxels."""
import functools

import numpy as np

BOX = np.array([1.6, 1.2, 1.6])
CENTER = np.array([0.9, 0.45, 0.8])
RADIUS = 0.3
W, H = 80, 60
K = np.array([60.0, 60.0, 39.5, 29.5])
FRAMES, PER_FRAGMENT = 12, 6
VOXEL = 0.02
TRUNC = 4 * VOXEL


def look_at(eye, target, up=(0.0, 1.0, 0.0)):
    """Camera-to-world pose: z forward, x right, y down (the image's v axis), world ``up`` up."""
    eye, target, up = (np.asarray(a, dtype=np.float64) for a in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    P = np.eye(4)
    P[:3, 0], P[:3, 1], P[:3, 2], P[:3, 3] = x, y, z, eye
    return P


def camera(i):
    return look_at((0.25 + 0.04 * i, 0.6 + 0.01 * i, 0.25 + 0.01 * i), CENTER + np.array([0.0, 0.01 * i, 0.01 * i]))


def render(pose, width=W, height=H, k=K, scale=1.0):
    """f64 [height, width] z-depth in metres of the room scaled by ``scale``, seen from the camera-to-world ``pose``."""
    u, v = np.meshgrid(np.arange(width, dtype=np.float64), np.arange(height, dtype=np.float64))
    d_cam = np.stack([(u - k[2]) / k[0], (v - k[3]) / k[1], np.ones_like(u)], axis=-1)
    d = d_cam @ pose[:3, :3].T                      # the ray's parameter is the z-depth
    eye = pose[:3, 3]
    with np.errstate(divide='ignore', invalid='ignore'):
        t_wall = np.where(d > 0, (BOX * scale - eye) / d, np.where(d < 0, (0.0 - eye) / d, np.inf))
    t = t_wall.min(axis=-1)
    oc = eye - CENTER * scale
    a = (d * d).sum(-1)
    b = 2.0 * (d * oc).sum(-1)
    c = (oc * oc).sum() - (RADIUS * scale) ** 2
    disc = b * b - 4.0 * a * c
    with np.errstate(invalid='ignore'):
        t_sphere = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0.0))) / (2.0 * a), np.inf)
    t_sphere = np.where(t_sphere > 0, t_sphere, np.inf)
    return np.minimum(t, t_sphere)


def to_raw(depth_m):
    return np.rint(depth_m * 1000.0).astype(np.uint16)


def surface_distance(points, scale=1.0):
    """f64 [N]: distance of world-frame points to the room's surface (nearest wall plane or the sphere)."""
    p = np.asarray(points, dtype=np.float64)
    wall = np.minimum(np.abs(p), np.abs(p - BOX * scale)).min(axis=1)
    sphere = np.abs(np.linalg.norm(p - CENTER * scale, axis=1) - RADIUS * scale)
    return np.minimum(wall, sphere)


@functools.lru_cache(maxsize=None)
def sequence():
    """(depth uint16 [12,60,80], intrinsics [4], poses f64 [12,4,4]); shared, do not modify."""
    poses = np.stack([camera(i) for i in range(FRAMES)])
    depth = np.stack([to_raw(render(P)) for P in poses])
    depth.setflags(write=False)
    poses.setflags(write=False)
    return depth, K.copy(), poses


def to_world(points, pose):
    p = np.asarray(points, dtype=np.float64)
    return p @ pose[:3, :3].T + pose[:3, 3]


# ------------------------------------------------------------------------------------------------- small volumes
SMALL_W, SMALL_H = 37, 23
SMALL_K = np.array([30.0, 30.0, 18.0, 11.0])


def _small_pose(k):
    """Camera-to-volume pose k of the small cases: near the origin, looking along +z, a little turned and moved."""
    return look_at((0.02 * k, -0.01 * k, 0.005 * k), (0.03 * k, 0.02 * k, 1.0), up=(0.0, -1.0, 0.0))


def _slanted(k):
    """f64 [23,37] depth in metres of frame k: a slanted surface about one metre away."""
    u, v = np.meshgrid(np.arange(SMALL_W, dtype=np.float64), np.arange(SMALL_H, dtype=np.float64))
    return 1.0 + 0.002 * u + 0.003 * v + 0.004 * k


def _rigid_inverse(P):
    out = np.eye(4)
    out[:3, :3] = P[:3, :3].T
    out[:3, 3] = -(P[:3, :3].T @ P[:3, 3])
    return out


@functools.lru_cache(maxsize=None)
def small_cases():
    """name -> keyword arguments of ``ops.tsdf_integrate`` (plus ``camera_to_volume`` for the bounds): one volume each,
    over images of 37 x 23, chosen where the indexing can go wrong."""
    poses = [_small_pose(k) for k in range(2)]
    M = np.stack([_rigid_inverse(P) for P in poses])
    C = np.stack(poses)
    raw = np.stack([to_raw(_slanted(k)) for k in range(2)])
    holes = raw.copy()
    holes[:, 5:12, 10:20] = 0
    holes[0, 0, 0] = 0
    metres = (raw.astype(np.float32) / np.float32(1000.0)).astype(np.float32)
    nan = metres.copy()
    nan[0, 11, 18] = np.nan
    nan[1, 3, 30] = np.inf
    base = dict(depth=raw, frame_start=[0, 2], intrinsics=SMALL_K, volume_to_camera=M, camera_to_volume=C, voxel=0.05,
                trunc=0.1, depth_scale=1000.0, depth_max=6.0)

    def case(**kw):
        c = dict(base)
        c.update(kw)
        return c
    return {
        'dims_13x9x7': case(origin=[-0.3, -0.2, 0.9], dims=[13, 9, 7]),
        'dims_1x5x5': case(origin=[0.0, -0.1, 0.95], dims=[1, 5, 5]),
        'dims_5x1x1': case(origin=[-0.2, 0.0, 1.07], dims=[5, 1, 1], voxel=0.1, trunc=0.2),
        'last_plane': case(origin=[-0.1, -0.1, 0.95], dims=[4, 4, 4]),
        'zero_frames': case(origin=[-0.3, -0.2, 0.9], dims=[13, 9, 7], frame_start=[0, 0]),
        'behind_camera': case(origin=[-0.3, -0.2, -2.0], dims=[13, 9, 7]),
        'partly_outside': case(origin=[-2.0, -1.5, 0.8], dims=[41, 31, 9], voxel=0.1, trunc=0.2),
        'holes': case(depth=holes, origin=[-0.3, -0.2, 0.9], dims=[13, 9, 7]),
        'depth_max': case(origin=[-0.3, -0.2, 0.9], dims=[13, 9, 7], depth_max=1.07),
        'f32_nan': case(depth=nan, origin=[-0.3, -0.2, 0.9], dims=[13, 9, 7]),
    }


def integrate_args(case):
    return {k: v for k, v in case.items() if k != 'camera_to_volume'}


def bounds_args(case):
    return dict(depth=case['depth'], frame_start=case['frame_start'], intrinsics=case['intrinsics'],
                camera_to_volume=case['camera_to_volume'], depth_scale=case['depth_scale'],
                depth_max=case['depth_max'])


def extract_args(case):
    return dict(origin=case['origin'], dims=case['dims'], voxel=case['voxel'])


def fragment_setup():
    """The scene as arguments of ``ops.tsdf_bounds`` / ``tsdf_integrate``: (depth, frame_start, K, M, C)."""
    depth, k, poses = sequence()
    first = (np.arange(FRAMES) // PER_FRAGMENT) * PER_FRAGMENT
    M = np.stack([_rigid_inverse(poses[f]) @ poses[first[f]] for f in range(FRAMES)])
    C = np.stack([_rigid_inverse(poses[first[f]]) @ poses[f] for f in range(FRAMES)])
    return depth, [0, PER_FRAGMENT, FRAMES], k, M, C
