"""Shared inputs of the ray-cast tests (csrc/tsdf_raycast.hpp), built from the analytic room and the small volumes of
``tsdf_scene``: name -> keyword arguments of ``ops.tsdf_raycast`` / ``tsdf_raycast_host`` / ``tsdf_raycast_numpy`` with D
and w as NumPy arrays (``on_device`` moves them).  Volumes are fused once by the host twin and shared; do not modify."""
import functools

import numpy as np

from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.datasets import fragments as fr
import tsdf_scene as S

MIDDLE = S.look_at((0.45, 0.66, 0.31), S.CENTER + np.array([0.0, 0.05, 0.05]))    # not a camera of the sequence


def freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def room_volume(frames=S.FRAMES):
    """The room fused from its first ``frames`` frames into ONE volume in the frame of camera 0, voxel 0.02, trunc
    0.08: dict(D, w, vol_start, origin, dims, voxel, trunc) and the sequence's poses."""
    depth, K, poses = S.sequence()
    depth, poses = depth[:frames], poses[:frames]
    M = np.stack([fr.rigid_inverse(P) @ poses[0] for P in poses])
    C = np.stack([fr.rigid_inverse(poses[0]) @ P for P in poses])
    origin, dims = fr.place_volumes(ops.tsdf_bounds_host(depth, [0, frames], K, C).numpy(), S.VOXEL)
    D, w, vs = ops.tsdf_integrate_host(depth, [0, frames], K, M, origin, dims, S.VOXEL, S.TRUNC)
    D, w, vs = freeze(D.numpy(), w.numpy(), vs.numpy())
    return dict(D=D, w=w, vol_start=vs, origin=origin, dims=dims, voxel=S.VOXEL, trunc=S.TRUNC)


def room_view_poses():
    """Camera-to-world poses of the three views of the room: frames 3 and 11 and one between the cameras."""
    poses = S.sequence()[2]
    return [poses[3], poses[11], MIDDLE]


def to_volume(world_poses):
    first = S.sequence()[2][0]
    return np.stack([fr.rigid_inverse(first) @ P for P in world_poses]) if len(world_poses) else np.zeros((0, 4, 4))


def room_views(world_poses, **kw):
    case = dict(room_volume(), intrinsics=S.K, camera_to_volume=to_volume(world_poses), height=S.H, width=S.W,
                view_volume=[0] * len(world_poses))
    case.update(kw)
    return case


@functools.lru_cache(maxsize=None)
def fragment_volumes():
    """The two fragment volumes of ``S.fragment_setup`` (different dims) and the camera-to-volume poses of all frames."""
    depth, fs, K, M, C = S.fragment_setup()
    origin, dims = fr.place_volumes(ops.tsdf_bounds_host(depth, fs, K, C).numpy(), S.VOXEL)
    D, w, vs = ops.tsdf_integrate_host(depth, fs, K, M, origin, dims, S.VOXEL, S.TRUNC)
    D, w, vs = freeze(D.numpy(), w.numpy(), vs.numpy())
    return dict(D=D, w=w, vol_start=vs, origin=origin, dims=dims, voxel=S.VOXEL, trunc=S.TRUNC), C


def two_volumes(frames=(8, 2, 10, 4), view_volume=(1, 0, 1, 0)):
    vol, C = fragment_volumes()
    return dict(vol, intrinsics=S.K, camera_to_volume=C[list(frames)], height=S.H, width=S.W,
                view_volume=list(view_volume))


@functools.lru_cache(maxsize=None)
def small_volume(name):
    case = S.small_cases()[name]
    D, w, vs = ops.tsdf_integrate_host(**S.integrate_args(case))
    D, w, vs = freeze(D.numpy(), w.numpy(), vs.numpy())
    return dict(D=D, w=w, vol_start=vs, origin=case['origin'], dims=case['dims'], voxel=case['voxel'],
                trunc=case['trunc'])


def small_views(name):
    """The small volume ``name`` seen from its own two cameras: images of 37 x 23, which fill no 8 x 8 tile."""
    return dict(small_volume(name), intrinsics=S.SMALL_K, camera_to_volume=S.small_cases()[name]['camera_to_volume'],
                height=S.SMALL_H, width=S.SMALL_W, view_volume=[0, 0])


def nan_pose():
    C = to_volume([S.sequence()[2][3]])
    C[0, 1, 2] = np.nan
    return C


@functools.lru_cache(maxsize=None)
def cases():
    """name -> arguments.  The room from three poses; every small volume (among them a 13 x 9 x 7 lattice, lattices with
    a dimension of 1, a volume without a frame); and the edge views."""
    poses = S.sequence()[2]
    out = {'room': room_views(room_view_poses())}
    for name in sorted(S.small_cases()):
        out['small_' + name] = small_views(name)
    inside = S.look_at((0.8, 0.6, 0.8), (1.6, 0.3, 1.6))                       # the camera in the middle of the volume
    away = S.look_at((0.25, 0.6, -3.0), (0.25, 0.6, -9.0))                     # behind the room, looking away from it
    out['camera_inside'] = room_views([inside])
    out['misses'] = room_views([away])
    out['nan_pose'] = dict(room_views([poses[3]]), camera_to_volume=nan_pose())
    out['depth_max'] = room_views([poses[3]], depth_max=1.0)
    out['one_frame_min_weight_2'] = dict(room_views([poses[0]]), **room_volume(1), min_weight=2.0)
    out['two_volumes'] = two_volumes()
    out['no_views'] = room_views([])
    return out


ALL_ZERO = ('small_dims_1x5x5', 'small_dims_5x1x1', 'small_zero_frames', 'small_behind_camera', 'misses', 'nan_pose',
            'one_frame_min_weight_2')


def on_device(case, device='cuda'):
    import torch
    out = dict(case)
    out['D'] = torch.from_numpy(np.array(case['D'])).to(device)
    out['w'] = torch.from_numpy(np.array(case['w'])).to(device)
    return out


# -------------------------------------------------------------------------------------------------------- walls
def wall_pixels(pose, clearance=0.16):
    """(mask bool [H,W], normals f64 [H,W,3] in the camera frame) of the pixels of the view ``pose`` (camera-to-world)
    whose ray meets a wall of the room at least ``clearance`` from every other wall and from the sphere, and whose
    eight neighbours meet the same wall: the wall's inward normal is then the surface normal there."""
    u, v = np.meshgrid(np.arange(S.W, dtype=np.float64), np.arange(S.H, dtype=np.float64))
    d = np.stack([(u - S.K[2]) / S.K[0], (v - S.K[3]) / S.K[1], np.ones_like(u)], axis=-1) @ pose[:3, :3].T
    eye = pose[:3, 3]
    with np.errstate(divide='ignore', invalid='ignore'):
        t_wall = np.where(d > 0, (S.BOX - eye) / d, np.where(d < 0, (0.0 - eye) / d, np.inf))
    axis = t_wall.argmin(axis=-1)
    t = t_wall.min(axis=-1)
    is_wall = S.render(pose) == t                                   # not the sphere
    p = eye + t[..., None] * d
    other = np.minimum(np.abs(p), np.abs(p - S.BOX))
    np.put_along_axis(other, axis[..., None], np.inf, axis=-1)
    wall_id = np.where(is_wall, 2 * axis + (np.take_along_axis(d, axis[..., None], -1)[..., 0] > 0), -1)
    same = np.zeros_like(is_wall)
    same[1:-1, 1:-1] = True
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            same[1:-1, 1:-1] &= wall_id[1 + dy:S.H - 1 + dy, 1 + dx:S.W - 1 + dx] == wall_id[1:-1, 1:-1]
    mask = (is_wall & same & (other.min(axis=-1) >= clearance)
            & (np.abs(np.linalg.norm(p - S.CENTER, axis=-1) - S.RADIUS) >= clearance))
    n_world = np.zeros(p.shape)
    np.put_along_axis(n_world, axis[..., None], -np.sign(np.take_along_axis(d, axis[..., None], -1)), axis=-1)
    return mask, n_world @ pose[:3, :3]


# ------------------------------------------------------------------------------------------------------ tracking
def noisy_depth():
    """The room's depth with seeded Gaussian noise of sigma = 5 raw units (5 mm)."""
    depth = S.sequence()[0]
    noise = np.random.default_rng(0).normal(0.0, 5.0, depth.shape)
    return np.clip(np.rint(depth.astype(np.float64) + noise), 0, 65535).astype(np.uint16)
