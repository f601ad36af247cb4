"""Shared inputs of the sparse ray-cast tests (csrc/tsdf_raycast_sparse.hpp): sparse pools of the analytic room and of
the small volumes of ``tsdf_scene``, allocated and fused once by the host twins and shared (do not modify), with the
views of ``raycast_cases``.  name -> keyword arguments of ``ops.tsdf_raycast_sparse`` / ``_host`` / ``_numpy`` with D
and w as NumPy arrays (``on_device`` moves them).  The oracle of every case is the DENSE host twin on the densified
pool: ``oracle(case)``."""
import functools

import numpy as np

from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.datasets import fragments as fr
import raycast_cases as R
import tsdf_scene as S
import tsdf_sparse_cases as SC

VIEW_KEYS = ('intrinsics', 'camera_to_volume', 'height', 'width', 'view_volume', 'step', 'depth_min', 'depth_max',
             'min_weight')


def pool_of(args):
    """``(sv, D, w)`` of the keyword arguments ``args`` of ``ops.tsdf_allocate`` plus ``volume_to_camera``: tables as
    CPU tensors, D and w as frozen arrays [B,512]."""
    sv = ops.tsdf_allocate_host(**SC.allocate_args(args))
    D, w = ops.tsdf_integrate_sparse_host(**SC.sparse_args(args, sv))
    D, w = R.freeze(D.numpy(), w.numpy())
    return sv, D, w


def room_args(voxel=S.VOXEL, trunc=S.TRUNC, frames=S.FRAMES):
    """The room's first ``frames`` frames into ONE volume in the frame of camera 0, placed as ``raycast_cases`` does."""
    depth, K, poses = S.sequence()
    depth, poses = depth[:frames], poses[:frames]
    M = np.stack([fr.rigid_inverse(P) @ poses[0] for P in poses])
    C = np.stack([fr.rigid_inverse(poses[0]) @ P for P in poses])
    origin, dims = fr.place_volumes(ops.tsdf_bounds_host(depth, [0, frames], K, C).numpy(), voxel)
    return dict(depth=depth, frame_start=[0, frames], intrinsics=K, volume_to_camera=M, camera_to_volume=C,
                origin=origin, dims=dims, voxel=voxel, trunc=trunc, depth_scale=1000.0, depth_max=6.0)


@functools.lru_cache(maxsize=None)
def room_pool(voxel=S.VOXEL, trunc=S.TRUNC, frames=S.FRAMES):
    sv, D, w = pool_of(room_args(voxel, trunc, frames))
    return dict(D=D, w=w, sv=sv, trunc=trunc)


@functools.lru_cache(maxsize=None)
def room_dense(voxel=S.VOXEL, trunc=S.TRUNC):
    """The same room integrated DENSELY by the host twin: the arguments of ``ops.tsdf_raycast_host``."""
    a = room_args(voxel, trunc)
    D, w, vs = ops.tsdf_integrate_host(a['depth'], a['frame_start'], a['intrinsics'], a['volume_to_camera'],
                                       a['origin'], a['dims'], voxel, trunc)
    D, w, vs = R.freeze(D.numpy(), w.numpy(), vs.numpy())
    return dict(D=D, w=w, vol_start=vs, origin=a['origin'], dims=a['dims'], voxel=voxel, trunc=trunc)


def inside_pose():
    return S.look_at((0.8, 0.6, 0.8), (1.6, 0.3, 1.6))           # the camera in the middle of the volume


def room_views(world_poses, pool=None, **kw):
    case = dict(pool or room_pool(), intrinsics=S.K, camera_to_volume=R.to_volume(world_poses), height=S.H, width=S.W,
                view_volume=[0] * len(world_poses))
    case.update(kw)
    return case


@functools.lru_cache(maxsize=None)
def small_pool(name):
    case = S.small_cases()[name]
    sv, D, w = pool_of(case)
    return dict(D=D, w=w, sv=sv, trunc=case['trunc'])


def small_views(name):
    return dict(small_pool(name), intrinsics=S.SMALL_K, camera_to_volume=S.small_cases()[name]['camera_to_volume'],
                height=S.SMALL_H, width=S.SMALL_W, view_volume=[0, 0])


@functools.lru_cache(maxsize=None)
def fragment_pool():
    """The two fragment volumes of the room (different dims) as one sparse batch, and the poses of all frames."""
    args = SC.room_args()
    sv, D, w = pool_of(args)
    return dict(D=D, w=w, sv=sv, trunc=S.TRUNC), args['camera_to_volume']


def two_volumes(frames=(8, 2, 10, 4), view_volume=(1, 0, 1, 0)):
    pool, C = fragment_pool()
    return dict(pool, intrinsics=S.K, camera_to_volume=C[list(frames)], height=S.H, width=S.W,
                view_volume=list(view_volume))


@functools.lru_cache(maxsize=None)
def cases():
    """name -> arguments: the room from the three views of ``raycast_cases`` plus the camera inside the volume, every
    small volume allocated and integrated with its own arguments, two volumes, and the edge views."""
    poses = S.sequence()[2]
    out = {'room': room_views(R.room_view_poses() + [inside_pose()])}
    for name in sorted(S.small_cases()):
        out['small_' + name] = small_views(name)
    out['two_volumes'] = two_volumes()
    out['nan_pose'] = dict(room_views([poses[3]]), camera_to_volume=R.nan_pose())
    out['one_frame_min_weight_2'] = room_views([poses[0]], room_pool(frames=1), min_weight=2.0)
    out['min_weight_0'] = room_views([poses[3], inside_pose()], min_weight=0.0)
    out['small_13x9x7_min_weight_0'] = dict(small_views('dims_13x9x7'), min_weight=0.0)
    out['no_views'] = room_views([])
    return out


ALL_ZERO = ('small_dims_1x5x5', 'small_dims_5x1x1', 'small_zero_frames', 'small_behind_camera', 'nan_pose',
            'one_frame_min_weight_2')
HITS = ('room', 'two_volumes', 'small_dims_13x9x7', 'small_holes', 'min_weight_0')
NO_BRICKS = ('small_zero_frames', 'small_behind_camera')


def oracle(case):
    """``(depth, normals)`` of the rule: the dense host twin on the densified pool, same views."""
    D, w, vs = ops.tsdf_densify(case['D'], case['w'], case['sv'])
    sv = case['sv']
    views = {k: case[k] for k in VIEW_KEYS if k in case}
    depth, nrm = ops.tsdf_raycast_host(D, w, vs, sv.origin, sv.dims, sv.voxel, case['trunc'], normals=True, **views)
    return depth.numpy(), nrm.numpy()


def on_device(case, device='cuda'):
    import torch
    out = dict(case)
    out['D'] = torch.from_numpy(np.array(case['D'])).to(device)
    out['w'] = torch.from_numpy(np.array(case['w'])).to(device)
    return out


# ------------------------------------------------------------------------------------------- into= and tsdf_extend
INTO_CASES = ('dims_13x9x7', 'f32_nan', 'holes', 'partly_outside', 'room')


@functools.lru_cache(maxsize=None)
def batch_args(name):
    """The keyword arguments (``tsdf_allocate``'s plus ``volume_to_camera``) of an ``into=`` / ``tsdf_extend`` case: a
    small case of one volume, or the room's two fragments."""
    return SC.room_args() if name == 'room' else S.small_cases()[name]


def split_frames(args, k):
    """``args`` cut into the frames every volume owns before and from its k-th frame on (k < 0: counted from its end):
    two argument dicts over the same volumes."""
    fs = np.asarray(args['frame_start'], dtype=np.int64)
    cut = np.array([min(max(a + k if k >= 0 else b + k, a), b) for a, b in zip(fs[:-1], fs[1:])])
    parts = []
    for lo, hi in ((fs[:-1], cut), (cut, fs[1:])):
        keep = np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)]).astype(np.int64)
        start = np.concatenate([[0], np.cumsum(hi - lo)])
        K = np.broadcast_to(np.asarray(args['intrinsics'], dtype=np.float64).reshape(-1, 4),
                            (args['depth'].shape[0], 4))
        parts.append(dict(args, depth=np.ascontiguousarray(args['depth'][keep]), frame_start=start,
                          intrinsics=K[keep], volume_to_camera=args['volume_to_camera'][keep],
                          camera_to_volume=args['camera_to_volume'][keep]))
    return parts


def extend_args(args):
    """The frame arguments of ``ops.tsdf_extend`` from an argument dict."""
    return dict(depth=args['depth'], frame_start=args['frame_start'], intrinsics=args['intrinsics'],
                camera_to_volume=args['camera_to_volume'], trunc=args['trunc'], depth_scale=args['depth_scale'],
                depth_max=args['depth_max'])


def old_rows_in_new(sv, sv2):
    """int64 [B]: the row in ``sv2``'s pool of every row of ``sv``'s, found through the tables on the host."""
    bi, bs = SC.host(sv.brick_index), SC.host(sv.brick_start)
    bi2, bs2 = SC.host(sv2.brick_index), SC.host(sv2.brick_start)
    ls = sv.lattice_start
    out = np.zeros(sv.bricks, dtype=np.int64)
    for v in range(sv.volumes):
        part, part2 = bi[ls[v]:ls[v + 1]], bi2[ls[v]:ls[v + 1]]
        assert (part2[part >= 0] >= 0).all(), "a brick was lost"
        out[bs[v] + part[part >= 0]] = bs2[v] + part2[part >= 0]
    return out
