"""Cases shared by the sparse TSDF tests (csrc/tsdf_sparse.hpp): the small volumes of ``tsdf_scene`` plus a volume whose
surface crosses a brick face, batches that put a volume without bricks between two others, a hand-made pool whose +1
neighbour brick is absent, and the helpers that compare a sparse result with the dense one."""
import functools

import numpy as np

from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.datasets import fragments as fr
import tsdf_scene as S


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, 'detach') else np.asarray(a)


def bits(a):
    return np.ascontiguousarray(host(a), dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    return bits(a).shape == bits(b).shape and np.array_equal(bits(a), bits(b))


def same_tables(a, b):
    """Two SparseVolumes hold the same tables (tensors or arrays)."""
    return all(host(getattr(a, k)).dtype == host(getattr(b, k)).dtype and
               np.array_equal(host(getattr(a, k)), host(getattr(b, k)))
               for k in ('brick_index', 'brick_coord', 'brick_start', 'origin', 'dims', 'voxel'))


def sorted_rows(points):
    """The rows of f32 [N,3] ordered by their uint32 views: a set of rows, bit for bit."""
    u = bits(points).reshape(-1, 3)
    return u[np.lexsort((u[:, 2], u[:, 1], u[:, 0]))]


def same_row_sets(sparse, sparse_start, dense, dense_start):
    """Per volume, the sparse cloud holds the dense cloud's rows bit for bit, in whatever order."""
    sparse_start, dense_start = host(sparse_start), host(dense_start)
    if not np.array_equal(np.diff(sparse_start), np.diff(dense_start)):
        return False
    return all(np.array_equal(sorted_rows(host(sparse)[sparse_start[v]:sparse_start[v + 1]]),
                              sorted_rows(host(dense)[dense_start[v]:dense_start[v + 1]]))
               for v in range(len(dense_start) - 1))


@functools.lru_cache(maxsize=None)
def brick_face_case():
    """17 x 9 x 9 voxels of 0.05 m seen along the volume's +x axis: the slanted surface of the small cases, about 1.07 m
    from the camera at the image centre, lies between ix = 7 and ix = 8 (origin_x + 7.5 voxels = 1.069 m), so its
    crossings on the x axis join the bricks bx = 0 and bx = 1."""
    base = S.small_cases()['dims_13x9x7']
    pose = S.look_at((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), up=(0.0, 0.0, 1.0))
    C = np.stack([pose, pose])
    M = np.stack([S._rigid_inverse(pose)] * 2)
    return dict(base, volume_to_camera=M, camera_to_volume=C, origin=[0.694, -0.2, -0.2], dims=[17, 9, 9])


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case: every small case of ``tsdf_scene`` and the brick-face volume; shared, do not modify."""
    out = dict(S.small_cases())
    out['brick_face_17x9x9'] = brick_face_case()
    return out


def allocate_args(case):
    return dict(depth=case['depth'], frame_start=case['frame_start'], intrinsics=case['intrinsics'],
                camera_to_volume=case['camera_to_volume'], origin=case['origin'], dims=case['dims'],
                voxel=case['voxel'], trunc=case['trunc'], depth_scale=case['depth_scale'], depth_max=case['depth_max'])


def sparse_args(case, sv):
    return dict(depth=case['depth'], frame_start=case['frame_start'], intrinsics=case['intrinsics'],
                volume_to_camera=case['volume_to_camera'], sv=sv, trunc=case['trunc'],
                depth_scale=case['depth_scale'], depth_max=case['depth_max'])


def batch_of(names):
    """The small cases ``names`` as ONE batch: a case of several volumes, each keeping its own frames."""
    picked = [cases()[n] for n in names]
    depth, M, C, frame_start = [], [], [], [0]
    for c in picked:
        f0, f1 = c['frame_start']
        depth.append(c['depth'][f0:f1])
        M.append(c['volume_to_camera'][f0:f1])
        C.append(c['camera_to_volume'][f0:f1])
        frame_start.append(frame_start[-1] + f1 - f0)
    return dict(depth=np.concatenate(depth), frame_start=frame_start, intrinsics=S.SMALL_K,
                volume_to_camera=np.concatenate(M), camera_to_volume=np.concatenate(C),
                origin=[c['origin'] for c in picked], dims=[c['dims'] for c in picked],
                voxel=[c['voxel'] for c in picked], trunc=[c['trunc'] for c in picked], depth_scale=1000.0,
                depth_max=6.0)


EMPTY_BETWEEN = {'behind_camera': ('dims_13x9x7', 'behind_camera', 'brick_face_17x9x9'),
                 'zero_frames': ('partly_outside', 'zero_frames', 'dims_13x9x7')}


def room_args():
    """The two fragments of the room as one batch: the keyword arguments of ``ops.tsdf_allocate`` plus
    ``volume_to_camera``, with the volumes placed as ``fuse_fragments`` places them."""
    depth, fs, K, M, C = S.fragment_setup()
    origin, dims = fr.place_volumes(ops.tsdf_bounds_numpy(depth, fs, K, C), S.VOXEL)
    return dict(depth=depth, frame_start=fs, intrinsics=K, volume_to_camera=M, camera_to_volume=C, origin=origin,
                dims=dims, voxel=S.VOXEL, trunc=S.TRUNC, depth_scale=1000.0, depth_max=6.0)


def absent_neighbour_pool():
    """A hand-made pool: one volume of 16 x 8 x 8 voxels (two lattice bricks along x) of which only brick 0 is
    allocated.  D = -0.5 for ix < 4 and +0.5 from there on, w = 1: the crossings between ix = 3 and ix = 4 are the only
    ones, and the valid voxels at ix = 7 have a +1 neighbour in the absent brick: no point there."""
    sv = ops.SparseVolumes(np.array([0, -1], dtype=np.int32), np.array([[0, 0, 0]], dtype=np.int32),
                           np.array([0, 1], dtype=np.int64), np.zeros((1, 3), dtype=np.float32),
                           np.array([[16, 8, 8]], dtype=np.int32), np.array([0.5], dtype=np.float32))
    ix = np.arange(512) & 7
    D = np.where(ix < 4, -0.5, 0.5).astype(np.float32).reshape(1, 512)
    return sv, D, np.ones((1, 512), dtype=np.float32)


def far_patches(width=24, height=18):
    """Two views from the middle of the room of two wall patches far apart (the wall x = 0 and the wall z = 1.6): the
    box around both is mostly empty space.  ``(depth uint16 [2,h,w], K [4], poses f64 [2,4,4])``."""
    k = np.array([60.0, 60.0, (width - 1) / 2.0, (height - 1) / 2.0])
    eye = (0.8, 0.6, 0.8)
    poses = np.stack([S.look_at(eye, (0.0, 0.6, 0.8)), S.look_at(eye, (0.8, 0.6, 1.6))])
    depth = np.stack([S.to_raw(S.render(P, width, height, k)) for P in poses])
    return depth, k, poses
