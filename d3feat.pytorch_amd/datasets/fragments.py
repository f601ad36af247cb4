"""Fragments and scenes from an RGB-D sequence: TSDF fusion of depth frames on the device (csrc/tsdf.hpp has the rule).

The upstream end of the 3DMatch pipeline -- a fragment is the fusion of ``frames_per_fragment`` (50) consecutive depth
frames, expressed in the frame of its first camera, whose pose is the fragment's ``.info.txt`` -- and its downstream
end: the fused scene, the same integration over all frames with the fragment poses of ``multiway_registration``
composed in.  The reference ships no code for either step (its fragments are the authors' download), so files made here
follow the rule of csrc/tsdf.hpp and are not claimed to equal that download.

``device='cuda'`` runs the HIP kernels (``ops.tsdf_bounds`` / ``tsdf_integrate`` / ``tsdf_extract``); ``device='cpu'``
runs their NumPy restatement, which gives the same clouds bit for bit.  ``mesh=True`` also gives the triangle mesh of
each volume with its vertex normals (``ops.tsdf_mesh``; csrc/tsdf_mesh.hpp has the rule).  ``sparse=True`` keeps D and w
only for the bricks of 8 x 8 x 8 voxels near a surface (``ops.tsdf_allocate`` / ``tsdf_integrate_sparse`` /
``tsdf_extract_sparse``; csrc/tsdf_sparse.hpp has the rule): the same points, in the sparse order, from a fraction of
the memory; ``mesh_fragments`` / ``mesh_scene`` give their meshes straight from the pools (``ops.tsdf_mesh_sparse``;
csrc/tsdf_mesh_sparse.hpp has the rule).  ``color=`` fuses the colour images beside D and w (csrc/tsdf_color.hpp has
the rule: one weight, ``c = (c w + c_pixel) / (w + 1)`` on the frames that update D) and returns the colour of every
point and mesh vertex, sampled from the colour volume (``ops.tsdf_sample_color``).

``track_sequence`` gives the camera poses of a sequence that comes without them: frame-to-frame depth odometry
(``ops.depth_odometry``; csrc/odometry.hpp has the rule), all frame pairs of a chunk in one launch sequence; with
``model=`` every frame is tracked against a ray-cast of its fragment's TSDF volume as well (``ops.tsdf_raycast``;
csrc/tsdf_raycast.hpp has the rule), which ``sparse=True`` keeps in bricks (``ops.tsdf_raycast_sparse`` / ``tsdf_extend``;
csrc/tsdf_raycast_sparse.hpp).  With ``color=`` the frame-to-frame pass is the RGB-D odometry (``ops.rgbd_odometry``;
csrc/rgbd_odometry.hpp), which also tracks views of a single plane; ``read_sequence(color=True)`` reads the colour
images, and with ``color=`` and ``model=`` together the model carries one intensity channel, every step renders depth
and intensity, and the model pass is RGB-D too.  ``render_views`` ray-casts volumes, dense or sparse, from 4x4 poses,
with ``color=`` their colour as well.
"""
import os
import re
from os.path import exists, join

import numpy as np

DEFAULT_MAX_BYTES = 1 << 33      # D and w of the volumes integrated in one launch (8 bytes per voxel, 4 more per
                                 # colour channel)
DEFAULT_DEPTH_MAX = 6.0          # metres (ops.TSDF_DEPTH_MAX)


def rigid_inverse(P):
    """f64 inverse [R^T, -R^T t] of the rigid 4x4 ``P``."""
    P = np.asarray(P, dtype=np.float64)
    out = np.eye(4)
    out[:3, :3] = P[:3, :3].T
    out[:3, 3] = -(P[:3, :3].T @ P[:3, 3])
    return out


def _is_cpu(device):
    return str(device).startswith('cpu')


def _frames(depth, intrinsics, poses):
    if hasattr(depth, 'detach'):
        from .. import ops
        depth = ops._tsdf_depth_array(depth)
    depth = np.asarray(depth)
    if depth.ndim != 3:
        raise ValueError("depth must be [F,H,W], got %s" % (depth.shape,))
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    if poses.shape[0] != depth.shape[0]:
        raise ValueError("%d poses for %d depth frames" % (poses.shape[0], depth.shape[0]))
    K = np.asarray(intrinsics, dtype=np.float64)
    if K.shape == (3, 3):
        K = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
    K = np.broadcast_to(K.reshape(-1, 4), (depth.shape[0], 4)).astype(np.float32)
    return depth, K, poses


def place_volumes(bounds, voxel):
    """``(origin f32 [V,3], dims int64 [V,3])`` from the [V,6] bounds of ``tsdf_bounds``: ``origin = voxel * (floor(min
    / voxel) - 1)`` and the lattice reaches one plane past the maximum.  A volume without a valid pixel gets one voxel."""
    b = np.asarray(bounds, dtype=np.float64).reshape(-1, 6)
    origin = np.zeros((b.shape[0], 3), dtype=np.float32)
    dims = np.ones((b.shape[0], 3), dtype=np.int64)
    for v in range(b.shape[0]):
        if not np.isfinite(b[v]).all():
            continue
        origin[v] = (voxel * (np.floor(b[v, :3] / voxel) - 1.0)).astype(np.float32)
        dims[v] = np.ceil((b[v, 3:] - origin[v].astype(np.float64)) / voxel).astype(np.int64) + 2
    return origin, dims


def _check_sparse(sparse, mesh):
    if sparse and mesh:
        raise ValueError("sparse=True gives no mesh here: mesh_fragments / mesh_scene fuse into sparse volumes and mesh "
                         "them (ops.tsdf_mesh_sparse)")


def _check_fits(dims, voxel, max_bytes, what, voxel_bytes=8):
    for v, n in enumerate(dims):
        nbytes = int(voxel_bytes) * int(n[0]) * int(n[1]) * int(n[2])
        if nbytes > max_bytes:
            raise ValueError("%s %d: a volume of %d x %d x %d voxels of %g m (extent %.2f x %.2f x %.2f m) takes %d "
                             "bytes, more than max_bytes = %d: raise max_bytes or the voxel size"
                             % (what, v, n[0], n[1], n[2], voxel, n[0] * voxel, n[1] * voxel, n[2] * voxel, nbytes,
                                max_bytes))


def _frame_groups(frame_start, frame_bytes, max_bytes):
    """(v, e) ranges of volumes whose frames fit ``max_bytes`` together (one volume's frames at least)."""
    V, v = frame_start.size - 1, 0
    while v < V:
        e = v + 1
        while e < V and int(frame_start[e + 1] - frame_start[v]) * frame_bytes <= int(max_bytes):
            e += 1
        yield v, e
        v = e


def _size_batches(sizes, max_bytes):
    """(v, e) ranges of volumes whose ``sizes`` fit ``max_bytes`` together (one volume at least)."""
    V, v = len(sizes), 0
    while v < V:
        e, used = v, 0
        while e < V and (e == v or used + int(sizes[e]) <= int(max_bytes)):
            used += int(sizes[e])
            e += 1
        yield v, e
        v = e


def _split_meshes(m, count, colors=None):
    """The per-volume (vertices, normals, faces) of a stacked mesh ``m`` of ``count`` volumes; with the stacked vertex
    ``colors`` a fourth entry, the volume's vertex colours."""
    vert, norm, face, vstart, fstart = m
    parts = (vert, norm) if colors is None else (vert, norm, colors)
    out = []
    for k in range(count):
        rows = [np.ascontiguousarray(a[vstart[k]:vstart[k + 1]]) for a in parts]
        out.append(tuple(rows[:2] + [np.ascontiguousarray(face[fstart[k]:fstart[k + 1]])] + rows[2:]))
    return out


def _fuse_sparse(depth, K, M, C, frame_start, origin, dims, voxel, trunc, depth_scale, depth_max, min_weight, cpu,
                 max_bytes, what, mesh=False, color=None):
    """``_fuse`` on sparse volumes: the bricks of every volume first (in the frame groups of the bounds), so that a
    volume whose pool and tables exceed ``max_bytes`` raises before any integration; then batches by the sparse
    sizes.  ``mesh``: also the meshes of the same pools (``ops.tsdf_mesh_sparse``), as ``_fuse`` returns them."""
    from .. import ops
    V = frame_start.size - 1
    allocate = ops.tsdf_allocate_numpy if cpu else ops.tsdf_allocate
    Cc = 0 if color is None else color.shape[-1]
    frame_bytes = (int(depth[0].nbytes) + (int(color[0].nbytes) if Cc else 0)) if depth.shape[0] else 0

    def tables(v, e):
        lo, hi = int(frame_start[v]), int(frame_start[e])
        return allocate(depth[lo:hi], frame_start[v:e + 1] - lo, K[lo:hi], C[lo:hi], origin[v:e], dims[v:e], voxel,
                        trunc, depth_scale, depth_max)
    sizes, kept = np.zeros(V, dtype=np.int64), {}
    for v, e in _frame_groups(frame_start, frame_bytes, max_bytes):
        sv = kept[(v, e)] = tables(v, e)                  # the tables are small: kept for a batch of the same volumes
        for k in range(v, e):
            sizes[k] = ops.tsdf_sparse_bytes(sv, k - v, Cc)
            if sizes[k] > max_bytes:
                n, start = dims[k], ops._host_array(sv.brick_start)
                raise ValueError("%s %d: the %d allocated bricks (of %d) of a volume of %d x %d x %d voxels of %g m "
                                 "take %d bytes, more than max_bytes = %d: raise max_bytes or the voxel size"
                                 % (what, k, start[k - v + 1] - start[k - v], np.diff(sv.lattice_start)[k - v], n[0],
                                    n[1], n[2], voxel, sizes[k], max_bytes))
    clouds, meshes, colors = [], [], []
    host = ops._host_array
    for v, e in _size_batches(sizes, max_bytes):
        lo, hi = int(frame_start[v]), int(frame_start[e])
        frames = (depth[lo:hi], frame_start[v:e + 1] - lo, K[lo:hi], M[lo:hi])
        sv = kept.pop((v, e), None) or tables(v, e)
        paint = dict(color=color[lo:hi]) if Cc else {}
        integrate, extract, mesher, sample = (
            (ops.tsdf_sparse_numpy, ops.tsdf_extract_sparse_numpy, ops.tsdf_mesh_sparse_numpy,
             ops.tsdf_sample_color_sparse_numpy) if cpu else
            (ops.tsdf_integrate_sparse, ops.tsdf_extract_sparse, ops.tsdf_mesh_sparse, ops.tsdf_sample_color_sparse))
        pool = integrate(*frames, sv, trunc, depth_scale, depth_max, **paint)
        D, w = pool[:2]
        pts, ps = extract(D, w, sv, min_weight)
        m = mesher(D, w, sv, min_weight) if mesh else None
        cols = host(sample(pool[2], w, sv, pts, ps, min_weight)) if Cc else None
        vcols = host(sample(pool[2], w, sv, m[0], m[3], min_weight)) if Cc and mesh else None
        pts, ps = host(pts), host(ps)
        m = [host(t) for t in m] if mesh else None
        del D, w, pool
        clouds.extend(np.ascontiguousarray(pts[ps[k]:ps[k + 1]]) for k in range(e - v))
        if Cc:
            colors.extend(np.ascontiguousarray(cols[ps[k]:ps[k + 1]]) for k in range(e - v))
        if mesh:
            meshes.extend(_split_meshes(m, e - v, vcols))
    return (clouds,) + ((meshes,) if mesh else ()) + ((colors,) if Cc else ())


def _fuse(depth, K, M, C, frame_start, voxel, trunc, depth_scale, depth_max, min_weight, device, max_bytes, what,
          mesh=False, sparse=False, color=None):
    """A tuple ``(clouds[, meshes][, colors])``: the clouds (list of f32 [N,3]) of the volumes that own the frame ranges
    ``frame_start`` of (depth, K, M, C); with ``mesh`` also their meshes, a list of (vertices f32 [Nv,3], normals f32
    [Nv,3], faces int32 [Nf,3]), from the same integrated volumes; with ``sparse`` from sparse volumes
    (``_fuse_sparse``).  ``color`` f32 [F,H,W,Cc] (``ops.tsdf_color_frames``): the colour is fused beside D and w, every
    mesh gains its vertex colours f32 [Nv,Cc] as a fourth entry and ``colors`` lists the clouds' colours f32 [N,Cc]."""
    from .. import ops
    cpu = _is_cpu(device)
    frame_start = np.asarray(frame_start, dtype=np.int64)
    V = frame_start.size - 1
    Cc = 0 if color is None else color.shape[-1]
    if V == 0:
        return ([],) + (([],) if mesh else ()) + (([],) if Cc else ())
    # the bounds in groups of volumes whose frames fit max_bytes too (one volume's frames at least): the depth frames
    # of a call (and its colour frames) are on the device next to its volumes
    frame_bytes = (int(depth[0].nbytes) + (int(color[0].nbytes) if Cc else 0)) if depth.shape[0] else 0
    bounds = []
    for v, e in _frame_groups(frame_start, frame_bytes, max_bytes):
        lo, hi = int(frame_start[v]), int(frame_start[e])
        args = (depth[lo:hi], frame_start[v:e + 1] - lo, K[lo:hi], C[lo:hi], depth_scale, depth_max)
        bounds.append(ops.tsdf_bounds_numpy(*args) if cpu else ops.tsdf_bounds(*args).cpu().numpy())
    bounds = np.concatenate(bounds, 0)
    origin, dims = place_volumes(bounds, voxel)
    if sparse:
        return _fuse_sparse(depth, K, M, C, frame_start, origin, dims, voxel, trunc, depth_scale, depth_max, min_weight,
                            cpu, int(max_bytes), what, mesh, color)
    _check_fits(dims, voxel, int(max_bytes), what, 8 + 4 * Cc)        # before anything is launched
    sizes = (8 + 4 * Cc) * dims[:, 0] * dims[:, 1] * dims[:, 2]
    clouds, meshes, colors = [], [], []
    host = ops._host_array
    integrate, extract, mesher, sample = (
        (ops.tsdf_numpy, ops.tsdf_extract_numpy, ops.tsdf_mesh_numpy, ops.tsdf_sample_color_numpy) if cpu else
        (ops.tsdf_integrate, ops.tsdf_extract, ops.tsdf_mesh, ops.tsdf_sample_color))
    for v, e in _size_batches(sizes, max_bytes):
        lo, hi = int(frame_start[v]), int(frame_start[e])
        args = (depth[lo:hi], frame_start[v:e + 1] - lo, K[lo:hi], M[lo:hi], origin[v:e], dims[v:e], voxel, trunc,
                depth_scale, depth_max)
        lattice = (origin[v:e], dims[v:e], voxel)
        fused = integrate(*args, **(dict(color=color[lo:hi]) if Cc else {}))
        D, w, vs = fused[:3]
        pts, ps = extract(D, w, vs, *lattice, min_weight)
        m = mesher(D, w, vs, *lattice, min_weight) if mesh else None
        cols = host(sample(fused[3], w, vs, *lattice, pts, ps, min_weight)) if Cc else None
        vcols = host(sample(fused[3], w, vs, *lattice, m[0], m[3], min_weight)) if Cc and mesh else None
        pts, ps = host(pts), host(ps)
        m = [host(t) for t in m] if mesh else None
        del D, w, fused
        clouds.extend(np.ascontiguousarray(pts[ps[k]:ps[k + 1]]) for k in range(e - v))
        if Cc:
            colors.extend(np.ascontiguousarray(cols[ps[k]:ps[k + 1]]) for k in range(e - v))
        if mesh:
            meshes.extend(_split_meshes(m, e - v, vcols))
    return (clouds,) + ((meshes,) if mesh else ()) + ((colors,) if Cc else ())


def fuse_fragments(depth, intrinsics, poses, frames_per_fragment=50, voxel=0.006, trunc=None, depth_scale=1000.0,
                   depth_max=DEFAULT_DEPTH_MAX, min_weight=1, device='cuda', max_bytes=DEFAULT_MAX_BYTES, mesh=False,
                   sparse=False, color=None):
    """``(clouds, fragment_poses)``: the fragments of a depth sequence, the 3DMatch way.

    ``depth`` [F,H,W] uint16 raw units (metres = raw / ``depth_scale``) or floating-point metres; ``intrinsics`` [4] =
    fx, fy, cx, cy, a 3x3 camera matrix, or [F,4]; ``poses`` [F,4,4] f64 camera-to-world.  Fragment g takes the frames
    ``[g k, (g + 1) k)`` (the last group may be shorter); its frame is its first camera's and its pose that camera's
    pose.  Frame f enters with ``M_f = inv(pose_f) @ pose_first`` (f64, rigid inverse, rounded to f32 once).  Every
    volume is placed from the back-projected extent of its frames (``place_volumes``); ``trunc`` defaults to ``5 *
    voxel``; a voxel counts with ``w >= min_weight``.  Fragments are integrated in batches whose volumes fit
    ``max_bytes``; one that does not fit alone raises ``ValueError`` before anything is launched.  The depth frames of
    a batch are uploaded with it (for the bounds, in groups that fit ``max_bytes`` as well): the device holds the
    volumes of one batch plus its frames, never the whole sequence.
    ``clouds``: list of f32 [N_g,3] in the fragments' own frames; ``fragment_poses`` f64 [G,4,4].  ``mesh=True``
    returns ``(clouds, fragment_poses, meshes)``: per fragment ``(vertices f32 [Nv,3], normals f32 [Nv,3], faces int32
    [Nf,3])`` in the fragment's frame, from the same integrated volume (``ops.tsdf_mesh``); the clouds and poses are
    those of ``mesh=False``.  ``sparse=True`` fuses into sparse volumes (csrc/tsdf_sparse.hpp): every volume's bricks
    are allocated first, ``max_bytes`` bounds the pools and tables of a batch (``ops.tsdf_sparse_bytes``) instead of the
    dense volumes, and each cloud holds the rows of ``sparse=False`` bit for bit in the sparse order (brick in lattice
    order, slot, axis).  ``sparse=True`` with ``mesh=True`` raises ``ValueError``: the mesh of sparse volumes comes
    from ``mesh_fragments``.

    ``color=`` uint8 [F,H,W,3] (R, G, B: three channels), uint8 [F,H,W] or floating point [F,H,W] (one), registered to
    the depth pixel by pixel (``ops.tsdf_color_frames``): the colour is fused beside D and w (csrc/tsdf_color.hpp: one
    weight, ``c = (c w + c_pixel) / (w + 1)`` on the frames that update D) and ``colors``, a list of f32 [N_g, Cc] with
    the colour of every point of every cloud in [0, 1], is appended last to what is returned; with ``mesh=True`` every
    mesh also gains its vertex colours f32 [Nv, Cc] as a fourth entry.  The colours are sampled from the colour volume
    at the points (``ops.tsdf_sample_color``: trilinear over the cell's corners that have weight).  ``max_bytes`` then
    counts ``8 + 4 Cc`` bytes per voxel (``ops.tsdf_sparse_bytes(..., channels=Cc)`` when sparse) and the colour frames
    beside the depth frames.  Without ``color`` nothing changes."""
    _check_sparse(sparse, mesh)
    return _fragments(depth, intrinsics, poses, frames_per_fragment, voxel, trunc, depth_scale, depth_max, min_weight,
                      device, max_bytes, mesh, sparse, color)


def _color_frames(color, depth):
    from .. import ops
    return None if color is None else ops.tsdf_color_frames(color, depth.shape)


def _fragments(depth, intrinsics, poses, frames_per_fragment, voxel, trunc, depth_scale, depth_max, min_weight, device,
               max_bytes, mesh, sparse, color=None):
    depth, K, poses = _frames(depth, intrinsics, poses)
    color = _color_frames(color, depth)
    k = int(frames_per_fragment)
    if k < 1:
        raise ValueError("frames_per_fragment must be at least 1")
    F = depth.shape[0]
    frame_start = np.asarray(list(range(0, F, k)) + [F], dtype=np.int64) if F else np.zeros(1, dtype=np.int64)
    first = np.repeat(frame_start[:-1], np.diff(frame_start))
    M = np.stack([rigid_inverse(poses[f]) @ poses[first[f]] for f in range(F)]) if F else np.zeros((0, 4, 4))
    C = np.stack([rigid_inverse(poses[first[f]]) @ poses[f] for f in range(F)]) if F else np.zeros((0, 4, 4))
    trunc = 5.0 * voxel if trunc is None else trunc
    fused = _fuse(depth, K, M, C, frame_start, float(voxel), float(trunc), depth_scale, depth_max, float(min_weight),
                  device, max_bytes, "fragment", mesh, sparse, color)
    fragment_poses = poses[frame_start[:-1]].copy()
    return (fused[0], fragment_poses) + tuple(fused[1:])


def fuse_scene(depth, intrinsics, poses, fragment_poses, frames_per_fragment, voxel, trunc=None, depth_scale=1000.0,
               depth_max=DEFAULT_DEPTH_MAX, min_weight=1, device='cuda', max_bytes=DEFAULT_MAX_BYTES, mesh=False,
               sparse=False, color=None):
    """One cloud f32 [N,3] in the scene frame: all frames fused into ONE volume, frame f of fragment g entering with the
    camera-to-scene pose ``fragment_poses[g] @ inv(poses[first_g]) @ poses[f]``.  ``fragment_poses`` [G',4,4] is what
    ``multiway_registration`` returns; the frames of a fragment whose pose is not finite, or that has none (g >= G'),
    are left out.  The one volume takes all kept frames in one launch, so they are on the device together with it.
    The other arguments are those of ``fuse_fragments``.  ``mesh=True`` returns ``(cloud, (vertices, normals, faces))``,
    the mesh of the same volume (empty arrays when no frame is kept).  ``sparse=True`` as for ``fuse_fragments``: the
    one volume is sparse, so a scene whose dense volume exceeds ``max_bytes`` fits when its allocated bricks do; its
    mesh comes from ``mesh_scene``.  ``color=`` as for ``fuse_fragments``: the cloud's colours f32 [N, Cc] are appended
    last -- ``(cloud, colors)``, or ``(cloud, (vertices, normals, faces, vertex_colors), colors)`` with a mesh."""
    _check_sparse(sparse, mesh)
    return _scene(depth, intrinsics, poses, fragment_poses, frames_per_fragment, voxel, trunc, depth_scale, depth_max,
                  min_weight, device, max_bytes, mesh, sparse, color)


def _scene(depth, intrinsics, poses, fragment_poses, frames_per_fragment, voxel, trunc, depth_scale, depth_max,
           min_weight, device, max_bytes, mesh, sparse, color=None):
    depth, K, poses = _frames(depth, intrinsics, poses)
    color = _color_frames(color, depth)
    Cc = 0 if color is None else color.shape[-1]
    k = int(frames_per_fragment)
    if k < 1:
        raise ValueError("frames_per_fragment must be at least 1")
    fp = np.asarray(fragment_poses, dtype=np.float64).reshape(-1, 4, 4)
    keep, S = [], []
    for f in range(depth.shape[0]):
        g = f // k
        if g >= fp.shape[0] or not np.isfinite(fp[g]).all():
            continue
        keep.append(f)
        S.append(fp[g] @ rigid_inverse(poses[g * k]) @ poses[f])
    if not keep:
        none = np.zeros((0, 3), dtype=np.float32)
        nocol = (np.zeros((0, Cc), dtype=np.float32),) if Cc else ()
        empty = (none.copy(), none.copy(), np.zeros((0, 3), dtype=np.int32)) + nocol
        out = (none,) + ((empty,) if mesh else ()) + nocol
        return out if len(out) > 1 else none
    S = np.stack(S)
    M = np.stack([rigid_inverse(s) for s in S])
    trunc = 5.0 * voxel if trunc is None else trunc
    fused = _fuse(np.ascontiguousarray(depth[keep]), K[keep], M, S, [0, len(keep)], float(voxel), float(trunc),
                  depth_scale, depth_max, float(min_weight), device, max_bytes, "scene", mesh, sparse,
                  None if color is None else np.ascontiguousarray(color[keep]))
    out = tuple(part[0] for part in fused)
    return out if len(out) > 1 else out[0]


def mesh_fragments(depth, intrinsics, poses, frames_per_fragment=50, voxel=0.006, trunc=None, depth_scale=1000.0,
                   depth_max=DEFAULT_DEPTH_MAX, min_weight=1, device='cuda', max_bytes=DEFAULT_MAX_BYTES, color=None):
    """``(clouds, fragment_poses, meshes)`` as ``fuse_fragments(mesh=True)`` returns them, fused into SPARSE volumes and
    meshed straight from their pools (``ops.tsdf_mesh_sparse``; csrc/tsdf_mesh_sparse.hpp has the rule): no dense volume
    is built, ``max_bytes`` bounds the pools and tables of a batch as for ``fuse_fragments(sparse=True)``, whose clouds
    these are.  Every mesh holds the vertices, normals and triangles of ``fuse_fragments(mesh=True)`` bit for bit, in
    the sparse order (pool row, slot, axis) and so with another vertex numbering.  ``device='cpu'`` runs the NumPy
    restatements, which work on the pools too.  ``color=`` as for ``fuse_fragments``: vertex colours as every mesh's
    fourth entry and ``colors`` appended last (``ops.tsdf_sample_color_sparse``)."""
    return _fragments(depth, intrinsics, poses, frames_per_fragment, voxel, trunc, depth_scale, depth_max, min_weight,
                      device, max_bytes, True, True, color)


def mesh_scene(depth, intrinsics, poses, fragment_poses, frames_per_fragment, voxel, trunc=None, depth_scale=1000.0,
               depth_max=DEFAULT_DEPTH_MAX, min_weight=1, device='cuda', max_bytes=DEFAULT_MAX_BYTES, color=None):
    """``(cloud, (vertices, normals, faces))`` as ``fuse_scene(mesh=True)`` returns them, from ONE sparse volume meshed
    straight from its pool (``ops.tsdf_mesh_sparse``): a scene whose dense volume exceeds ``max_bytes`` has a mesh when
    its allocated bricks fit.  The cloud is that of ``fuse_scene(sparse=True)``; empty arrays when no frame is kept.
    ``color=`` as for ``fuse_scene``."""
    return _scene(depth, intrinsics, poses, fragment_poses, frames_per_fragment, voxel, trunc, depth_scale, depth_max,
                  min_weight, device, max_bytes, True, True, color)


# --------------------------------------------------------------------------------------------------- tracking
DEFAULT_TRACK_BYTES = 1 << 30    # the depth pyramid of the frames tracked in one call (4 bytes per pixel, about 4/3 H W)


DEFAULT_MODEL = dict(frames_per_fragment=50, voxel=0.01, trunc=None, margin=None, step=None,
                     max_bytes=DEFAULT_MAX_BYTES, sparse=False, color=True)


def render_views(D, w, vol_start, origin, dims, voxel, trunc, intrinsics, poses, height, width, view_volume=None,
                 device='cuda', sv=None, **raycast):
    """Depth images f32 [R,H,W] in metres (0: no surface) of dense TSDF volumes seen from the camera-to-volume 4x4
    ``poses`` [R,4,4]: ``ops.tsdf_raycast`` (csrc/tsdf_raycast.hpp has the rule) on the device, where D and w are device
    tensors and so is the result; ``device='cpu'`` runs ``ops.tsdf_raycast_numpy`` on arrays.  ``view_volume`` [R] names
    every view's volume (None: one view per volume).  ``**raycast``: ``step``, ``depth_min``, ``depth_max``,
    ``min_weight``, ``normals`` (then ``(depth, normals f32 [R,H,W,3])``), ``clip``, and ``color=Cv`` (the colour volume
    of ``ops.tsdf_integrate(color=)``, or the colour pool with ``sv=``), which appends the colour render f32 [R,H,W,Cc]:
    NaN where the depth is 0.

    ``sv=``: the ``ops.SparseVolumes`` of a sparse pool ``D``, ``w`` [B,512] (``ops.tsdf_raycast_sparse``;
    csrc/tsdf_raycast_sparse.hpp has the rule: the render of the densified pool, bit for bit).  ``vol_start``,
    ``origin``, ``dims`` and ``voxel`` are then taken from ``sv`` and may be None; ``**raycast`` also takes ``skip``."""
    from .. import ops
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    if sv is not None:
        cast = ops.tsdf_raycast_sparse_numpy if _is_cpu(device) else ops.tsdf_raycast_sparse
        return cast(D, w, sv, trunc, intrinsics, poses, height, width, view_volume, **raycast)
    cast = ops.tsdf_raycast_numpy if _is_cpu(device) else ops.tsdf_raycast
    return cast(D, w, vol_start, origin, dims, voxel, trunc, intrinsics, poses, height, width, view_volume, **raycast)


def _track_pairs(depth, K, levels, iterations, cpu, max_bytes, depth_scale, depth_max, depth_diff, odometry,
                 color=None):
    """``(T f64 [F-1,4,4], status int32 [F-1])`` of the consecutive pairs (f+1, f), every pair from the identity, in
    chunks whose pyramid fits ``max_bytes``; with ``color`` by ``ops.rgbd_odometry``, whose intensity pyramid counts
    too."""
    from .. import ops
    F = depth.shape[0]
    frame_bytes = (4 if color is None else 8) * ops.depth_pyramid_pixels(depth.shape[1], depth.shape[2], levels)
    per_chunk = max(2, int(max_bytes) // max(frame_bytes, 1))
    T = np.broadcast_to(np.eye(4), (max(F - 1, 0), 4, 4)).copy()
    status = np.zeros(max(F - 1, 0), dtype=np.int32)
    pyramid, track = {(False, False): (ops.depth_pyramid, ops.depth_odometry),
                      (False, True): (ops.depth_pyramid_numpy, ops.depth_odometry_numpy),
                      (True, False): (ops.rgbd_pyramid, ops.rgbd_odometry),
                      (True, True): (ops.rgbd_pyramid_numpy, ops.rgbd_odometry_numpy)}[color is not None, bool(cpu)]
    for lo in range(0, F - 1, per_chunk - 1):
        hi = min(lo + per_chunk, F)                       # frames [lo, hi): the pairs (lo+1, lo) .. (hi-1, hi-2)
        pairs = np.stack([np.arange(1, hi - lo), np.arange(0, hi - lo - 1)], axis=1)
        frames = (depth[lo:hi],) if color is None else (depth[lo:hi], color[lo:hi])
        pyr = pyramid(*(frames + (K[lo:hi], levels, depth_scale, depth_max, depth_diff)))
        res = track(pyr, pairs, None, iterations, **odometry)
        T[lo:hi - 1], status[lo:hi - 1] = ops._host_array(res[0]), ops._host_array(res[3])
    return T, status


def _metres(frames, depth_scale):
    """f32 metres of depth frames, the conversion of csrc/tsdf.hpp's depth_value."""
    return frames.astype(np.float32) / np.float32(depth_scale) if frames.dtype == np.uint16 else frames


def _track_model(depth, K, T_ff, model, levels, iterations, cpu, depth_scale, depth_max, depth_diff, odometry,
                 inten=None, photo_weight=None):
    """The frame-to-model pass of ``track_sequence``: ``(T f64 [F-1,4,4], model_status int32 [F-1])``.  ``T_ff`` are the
    frame-to-frame poses actually used (the identity where that pass failed).  ``inten`` f32 [F,H,W]: the frames'
    intensity; unless ``model['color']`` is false the model carries it as one colour channel and the pass is RGB-D."""
    from .. import ops
    unknown = set(model) - set(DEFAULT_MODEL)
    if unknown:
        raise ValueError("model: unknown keys %s (known: %s)" % (sorted(unknown), sorted(DEFAULT_MODEL)))
    m = dict(DEFAULT_MODEL)
    m.update(model)
    k, voxel = int(m['frames_per_fragment']), float(m['voxel'])
    if k < 1:
        raise ValueError("model: frames_per_fragment must be at least 1")
    trunc = 5.0 * voxel if m['trunc'] is None else float(m['trunc'])
    margin = trunc if m['margin'] is None else float(m['margin'])
    max_bytes = int(m['max_bytes'])
    F, H, W = depth.shape
    frame_start = np.asarray(list(range(0, F, k)) + [F], dtype=np.int64)
    G = frame_start.size - 1
    T = T_ff.copy()
    model_status = np.zeros(max(F - 1, 0), dtype=np.int32)
    model_status[frame_start[1:-1] - 1] = -1              # the pairs that cross a fragment boundary
    # every camera in the frame of its fragment's first camera, chained frame to frame: where the volumes go
    L = np.broadcast_to(np.eye(4), (F, 4, 4)).copy()
    for g in range(G):
        for f in range(int(frame_start[g]) + 1, int(frame_start[g + 1])):
            L[f] = L[f - 1] @ T_ff[f - 1]
    frame_bytes = int(depth[0].nbytes)
    bounds = []
    for v, e in _frame_groups(frame_start, frame_bytes, max_bytes):
        lo, hi = int(frame_start[v]), int(frame_start[e])
        args = (depth[lo:hi], frame_start[v:e + 1] - lo, K[lo:hi], L[lo:hi], depth_scale, depth_max)
        bounds.append(ops.tsdf_bounds_numpy(*args) if cpu else ops.tsdf_bounds(*args).cpu().numpy())
    bounds = np.concatenate(bounds, 0).astype(np.float64)
    bounds[:, :3] -= margin
    bounds[:, 3:] += margin
    origin, dims = place_volumes(bounds, voxel)
    sparse = bool(m['sparse'])
    if inten is None or not m['color']:
        inten = None
    Cc = 0 if inten is None else 1
    eye = np.eye(4)
    if sparse:
        allocate = ops.tsdf_allocate_numpy if cpu else ops.tsdf_allocate
        extend = ops.tsdf_extend_numpy if cpu else ops.tsdf_extend
        integrate = ops.tsdf_sparse_numpy if cpu else ops.tsdf_integrate_sparse
        raycast = ops.tsdf_raycast_sparse_numpy if cpu else ops.tsdf_raycast_sparse

        def check_bytes(sv, v, e):
            nbytes = ops.tsdf_sparse_bytes(sv, channels=Cc)
            if nbytes > max_bytes:
                raise ValueError("model of fragments %d..%d: the %d allocated bricks (of %d) take %d bytes, more than "
                                 "max_bytes = %d: raise max_bytes or the voxel size"
                                 % (v, e - 1, sv.bricks, int(sv.lattice_start[-1]), nbytes, max_bytes))
        # the bricks of every fragment's first frame at the identity: the sizes the groups are made from
        first_all = frame_start[:-1]
        sizes = np.zeros(G, dtype=np.int64)
        for v, e in _frame_groups(np.arange(G + 1), frame_bytes, max_bytes):
            sv = allocate(depth[first_all[v:e]], np.arange(e - v + 1), K[first_all[v:e]],
                          np.broadcast_to(eye, (e - v, 4, 4)), origin[v:e], dims[v:e], voxel, trunc, depth_scale,
                          depth_max)
            for j in range(v, e):
                sizes[j] = ops.tsdf_sparse_bytes(sv, j - v, Cc)
    else:
        _check_fits(dims, voxel, max_bytes, "model of fragment", 8 + 4 * Cc)  # before anything is launched
        sizes = (8 + 4 * Cc) * dims[:, 0] * dims[:, 1] * dims[:, 2]
        integrate = ops.tsdf_numpy if cpu else ops.tsdf_integrate
        raycast = ops.tsdf_raycast_numpy if cpu else ops.tsdf_raycast
    for v, e in _size_batches(sizes, max_bytes):
        n = e - v
        first, count = frame_start[v:e], np.diff(frame_start[v:e + 1])
        vol = (origin[v:e], dims[v:e], voxel, trunc, depth_scale, depth_max)
        # step 0: the first frame of every fragment of the group, at the identity
        frames0 = (depth[first], np.arange(n + 1), K[first], np.broadcast_to(eye, (n, 4, 4)))
        paint = dict(color=inten[first]) if Cc else {}
        Cm = None                                              # the model's intensity: Cv, or the pool Cp
        if sparse:
            sv = allocate(*frames0, *vol)
            check_bytes(sv, v, e)
            D, w, Cm = (tuple(integrate(*frames0, sv, trunc, depth_scale, depth_max, **paint)) + (None,))[:3]
        else:
            D, w, vs, Cm = (tuple(integrate(*frames0, *vol, **paint)) + (None,))[:4]
        for s in range(1, int(count.max())):
            live = np.nonzero(count > s)[0]                # the fragments that have a frame s
            f = first[live] + s
            A = live.size
            views = (trunc, K[f - 1], L[f - 1], H, W, live)
            view = (D, w, sv) + views if sparse else (D, w, vs, origin[v:e], dims[v:e], voxel) + views
            frames = _metres(depth[f], depth_scale)
            pairs = np.stack([np.arange(A), A + np.arange(A)], axis=1)      # (frame s, the render of frame s - 1)
            K2 = np.concatenate([K[f], K[f - 1]])
            if Cc:
                # depth and intensity of the model in one launch; one RGB-D pyramid over the frames and the renders.  A
                # render's intensity is NaN where it has no depth: the tracker's finiteness test drops those pixels
                render, shade = raycast(*view, step=m['step'], depth_max=depth_max, color=Cm)
                rgbd = dict(odometry, photo_weight=photo_weight)
                if cpu:
                    pyr = ops.rgbd_pyramid_numpy(np.concatenate([frames, render]),
                                                 np.concatenate([inten[f], shade[..., 0]]), K2, levels, depth_scale,
                                                 depth_max, depth_diff)
                    res = ops.rgbd_odometry_numpy(pyr, pairs, T_ff[f - 1], iterations, **rgbd)
                else:
                    import torch
                    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(render.device)
                    pyr = ops.rgbd_pyramid(torch.cat([up(frames), render]), torch.cat([up(inten[f]), shade[..., 0]]),
                                           K2, levels, depth_scale, depth_max, depth_diff)
                    res = ops.rgbd_odometry(pyr, pairs, T_ff[f - 1], iterations, **rgbd)
                    res = (res[0].cpu().numpy(), None, None, res[3].cpu().numpy())   # the one read-back of the step
            elif cpu:
                both = np.concatenate([frames, raycast(*view, step=m['step'], depth_max=depth_max)])
                pyr = ops.depth_pyramid_numpy(both, K2, levels, depth_scale, depth_max, depth_diff)
                res = ops.depth_odometry_numpy(pyr, pairs, T_ff[f - 1], iterations, **odometry)
            else:
                import torch
                render = raycast(*view, step=m['step'], depth_max=depth_max)
                both = torch.cat([torch.from_numpy(np.ascontiguousarray(frames)).to(render.device), render])
                pyr = ops.depth_pyramid(both, K2, levels, depth_scale, depth_max, depth_diff)
                res = ops.depth_odometry(pyr, pairs, T_ff[f - 1], iterations, **odometry)
                res = (res[0].cpu().numpy(), None, None, res[3].cpu().numpy())   # the one read-back of the step
            for i in range(A):
                model_status[f[i] - 1] = res[3][i]
                if res[3][i] == 0:
                    T[f[i] - 1] = res[0][i]
                L[f[i]] = L[f[i] - 1] @ T[f[i] - 1]
            # frame s of every live fragment into its volume under inv(L): the others own no frame and keep theirs
            owns = np.zeros(n + 1, dtype=np.int64)
            owns[live + 1] = 1
            M = np.stack([rigid_inverse(L[j]) for j in f])
            paint = dict(color=inten[f]) if Cc else {}
            into = (D, w, Cm) if Cc else (D, w)
            if sparse:
                # the bricks the frame reaches under its refined pose first, then the frame into the grown pool
                grown = extend(sv, D, w, depth[f], np.cumsum(owns), K[f], L[f], trunc, depth_scale, depth_max,
                               **(dict(color=Cm) if Cc else {}))
                sv, into = grown[0], tuple(grown[1:])
                D, w, Cm = (into + (None,))[:3]
                check_bytes(sv, v, e)
                integrate(depth[f], np.cumsum(owns), K[f], M, sv, trunc, depth_scale, depth_max, into=into, **paint)
            else:
                integrate(depth[f], np.cumsum(owns), K[f], M, *vol, into=into, **paint)
        del D, w, Cm
    return T, model_status


def track_sequence(depth, intrinsics, stride=1, device='cuda', max_bytes=DEFAULT_TRACK_BYTES, depth_scale=1000.0,
                   depth_max=DEFAULT_DEPTH_MAX, depth_diff=0.05, model=None, color=None, photo_weight=None,
                   **odometry):
    """``(poses f64 [F,4,4], status int32 [F-1])``: camera poses of a depth sequence by frame-to-frame depth odometry
    (``ops.depth_odometry``: projective point-to-plane ICP over a depth pyramid, every pair from the identity).

    ``depth`` [F,H,W] and ``intrinsics`` as for ``fuse_fragments``.  ``stride`` takes every stride-th frame (F counts the
    frames taken).  ``poses[0] = I``; the pairs are ``(f+1, f)``, T_f maps camera f+1 into camera f, and
    ``poses[f+1] = poses[f] @ T_f``: camera-to-"world" poses in the frame of the first camera.  ``status[f]`` is the
    odometry's status of pair f (``ops.ODO_ST_*``); a pair whose status is not 0 keeps T_f = I -- reported, never
    repaired.  ``**odometry``: ``iterations`` (their number is the number of pyramid levels), ``max_distance``.
    Sequences whose pyramid exceeds ``max_bytes`` are tracked in chunks that overlap by one frame (two frames at
    least); a pair's result does not depend on its chunk.  ``device='cuda'`` runs the HIP kernels, ``device='cpu'``
    the NumPy restatement (equal to rounding).

    ``model=dict(frames_per_fragment=50, voxel=0.01, trunc=None, margin=None, step=None)`` (any subset; also
    ``max_bytes`` for the volumes of one group, as in ``fuse_fragments``) adds a frame-to-MODEL pass, KinectFusion's, and
    returns ``(poses, status, model_status)``.  Every fragment gets a dense volume in the frame of its first camera,
    placed from the frame-to-frame poses (``place_volumes``, widened by ``margin``, default ``trunc``, itself ``5 *
    voxel`` by default).  The first frame is integrated at the identity; then, frame by frame and for all fragments of a
    group at once, the volume is ray-cast from the refined pose of the previous frame (``ops.tsdf_raycast``, ``step``
    default ``trunc / 2``), the frame is tracked against that render by the same odometry, started from its
    frame-to-frame pose, and integrated into the volume under the result (``ops.tsdf_integrate(..., into=)``).  A pair
    tracked against the model with status 0 takes the model's pose; any other keeps its frame-to-frame pose.
    ``status`` is then the status of the pose actually used; ``model_status`` int32 [F-1] holds 0 where the model's pose
    was used, the tracker's ``ODO_ST_*`` where it failed against the render, and -1 for the pairs that cross a fragment
    boundary, which chain by their frame-to-frame pose: the model restarts with every fragment.  One read-back of poses
    and statuses per step.  Use it where the depth is noisy (the README has the figures): on clean depth the model's
    voxel quantisation costs more than the drift it removes.

    ``model=dict(sparse=True, ...)`` keeps the model in sparse volumes (csrc/tsdf_raycast_sparse.hpp): every fragment's
    bricks are allocated from its first frame at the identity; per step the pools are ray-cast directly
    (``ops.tsdf_raycast_sparse``), and after tracking every live fragment's bricks are grown by its new frame under the
    refined pose (``ops.tsdf_extend``) before the frame is integrated ``into`` the pool.  ``max_bytes`` then bounds
    ``ops.tsdf_sparse_bytes`` of a group instead of 8 bytes per voxel; it is checked after every growth and a group that
    outgrows it raises ``ValueError``.  A brick allocated late misses the free-space votes of the earlier frames, so the
    sparse model is not the dense one bit for bit; the README has the figures of both.

    ``color=`` uint8 [F,H,W,3] (``read_sequence(..., color=True)``), uint8 [F,H,W] or f32 [F,H,W], registered to the
    depth pixel by pixel: the frame-to-frame pass runs ``ops.rgbd_odometry`` instead (csrc/rgbd_odometry.hpp: a
    photometric row beside the point-to-plane row, scaled by ``photo_weight``, default ``ops.ODO_PHOTO_WEIGHT``), which
    tracks a view of a single plane where the depth-only pass reports ``ODO_ST_SINGULAR``; ``device='cpu'`` runs its
    NumPy restatement, and ``max_bytes`` counts the intensity pyramid too.  With ``model=`` the model of every
    fragment then carries ONE intensity channel beside D and w (csrc/tsdf_color.hpp; 12 bytes per voxel instead of 8):
    every step ray-casts depth AND intensity (``ops.tsdf_raycast(color=)``; the intensity is NaN where the render has
    no depth, which the tracker's finiteness test drops), builds one ``rgbd_pyramid`` over the frames and the renders,
    runs ``ops.rgbd_odometry`` against the render from the frame-to-frame pose, and integrates the frame with its
    intensity ``into`` the model -- dense or sparse, still one read-back per step.  The model pass therefore also holds
    on views that depth cannot (a pan along a wall).  ``model=dict(color=False, ...)`` keeps the depth-only model pass.

    ``fuse_fragments`` needs only the relative poses inside a fragment, so the result goes straight into it.  Without
    ``model`` drift accumulates from frame to frame; with it, from fragment to fragment; nothing closes a loop."""
    from .. import ops
    stride = int(stride)
    if stride < 1:
        raise ValueError("stride must be at least 1")
    depth = ops._tsdf_depth_array(depth)[::stride]
    F = depth.shape[0]
    if F < 1:
        raise ValueError("depth holds no frame")
    K = np.asarray(intrinsics, dtype=np.float64)
    if K.shape == (3, 3):
        K = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
    K = K.reshape(-1, 4)
    K = (K[::stride] if K.shape[0] > 1 else np.broadcast_to(K, (F, 4))).astype(np.float32)
    if K.shape[0] != F:
        raise ValueError("%d intrinsics rows for %d frames" % (K.shape[0], F))
    iterations = odometry.pop('iterations', ops.ODO_ITERATIONS)
    levels = len(ops._odo_iterations(iterations))
    cpu = _is_cpu(device)
    first = dict(odometry)
    if color is not None:
        color = ops._rgbd_color(np.asarray(ops._host_array(color))[::stride], depth.shape)[0]
        first['photo_weight'] = ops.ODO_PHOTO_WEIGHT if photo_weight is None else ops._rgbd_check_weight(photo_weight)
    elif photo_weight is not None:
        raise ValueError("photo_weight needs color")
    T, status = _track_pairs(depth, K, levels, iterations, cpu, max_bytes, depth_scale, depth_max, depth_diff, first,
                             color)
    for f in range(F - 1):
        if status[f] != 0:
            T[f] = np.eye(4)
    model_status = None
    if model is not None:
        inten = None if color is None else ops.tsdf_color_frames(color, depth.shape, channels=1)[..., 0]
        T, model_status = _track_model(np.ascontiguousarray(depth), K, T, dict(model), levels, iterations, cpu,
                                       depth_scale, depth_max, depth_diff, odometry, inten,
                                       first.get('photo_weight'))
        status = np.where(model_status == 0, 0, status).astype(np.int32)
    poses = np.broadcast_to(np.eye(4), (F, 4, 4)).copy()
    for f in range(F - 1):
        poses[f + 1] = poses[f] @ T[f]
    return (poses, status) if model is None else (poses, status, model_status)


# ------------------------------------------------------------------------------------------------------ files
def _ply_colors(colors, count):
    """uint8 [count,3] red, green, blue of colours f32 [count, 1 or 3] in [0, 1] (one channel is grey; a value outside
    [0, 1] is clipped, a NaN is 0)."""
    c = np.asarray(colors, dtype=np.float64).reshape(count, -1) if count else np.zeros((0, 3))
    if c.shape[1] not in (1, 3):
        raise ValueError("colors must hold 1 or 3 channels per vertex, got %d" % c.shape[1])
    c = np.broadcast_to(c, (count, 3)) if c.shape[1] == 1 else c
    return np.rint(np.clip(np.nan_to_num(c, nan=0.0), 0.0, 1.0) * 255.0).astype(np.uint8)


def _ply_vertex_rows(cols, names, colors):
    """(the packed vertex rows, their header lines): float columns ``cols`` named ``names``, then uchar red, green, blue
    when ``colors`` is given."""
    data = np.ascontiguousarray(np.concatenate(cols, axis=1))
    fields = [(n, '<f4') for n in names]
    header = "".join("property float %s\n" % n for n in names)
    if colors is None:
        return data.tobytes(), header
    rgb = _ply_colors(colors, data.shape[0])
    rows = np.zeros(data.shape[0], dtype=fields + [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')])
    for i, n in enumerate(names):
        rows[n] = data[:, i]
    rows['red'], rows['green'], rows['blue'] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    return rows.tobytes(), header + "property uchar red\nproperty uchar green\nproperty uchar blue\n"


def write_ply_points(filename, points, colors=None):
    """Binary little-endian PLY with the three float properties x, y, z; with ``colors`` f32 [N, 1 or 3] in [0, 1] (what
    ``fuse_fragments(color=)`` returns) also uchar red, green, blue.  ``read_ply_points`` reads either as a cloud."""
    p = np.ascontiguousarray(points, dtype='<f4').reshape(-1, 3)
    rows, header = _ply_vertex_rows([p], ['x', 'y', 'z'], colors)
    with open(filename, 'wb') as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\n%send_header\n"
                 % (p.shape[0], header)).encode('ascii'))
        f.write(rows)


def read_ply_colors(filename):
    """f32 [N,3] in [0, 1]: the uchar ``red green blue`` of the ``vertex`` element of a PLY file (what
    ``write_ply_points(colors=)`` writes; ascii or binary, the vertex element first), in the row order of
    ``read_ply_points``; None when the file carries no such colours."""
    from .ThreeDMatch import _PLY_TYPES
    with open(filename, 'rb') as f:
        if f.readline().strip() != b'ply':
            raise ValueError("%s: not a PLY file" % filename)
        fmt, n_vertex, props, element = None, None, [], None
        while True:
            line = f.readline()
            if not line:
                raise ValueError("%s: truncated PLY header" % filename)
            tok = line.decode('ascii', 'replace').split()
            if not tok or tok[0] in ('comment', 'obj_info'):
                continue
            if tok[0] == 'format':
                fmt = tok[1]
            elif tok[0] == 'element':
                element = tok[1]
                if element == 'vertex':
                    n_vertex = int(tok[2])
            elif tok[0] == 'property' and element == 'vertex':
                if tok[1] == 'list':
                    raise ValueError("%s: list property in the vertex element" % filename)
                props.append((tok[2], _PLY_TYPES[tok[1]]))
            elif tok[0] == 'end_header':
                break
        if n_vertex is None or fmt is None:
            raise ValueError("%s: no vertex element" % filename)
        kinds = dict(props)
        if any(kinds.get(c) != 'u1' for c in ('red', 'green', 'blue')):
            return None
        if fmt == 'ascii':
            rows = np.loadtxt(f, max_rows=n_vertex, ndmin=2) if n_vertex else np.zeros((0, len(props)))
            names = [n for n, _ in props]
            rgb = np.stack([rows[:, names.index(c)] for c in ('red', 'green', 'blue')], axis=1)
        else:
            order = {'binary_little_endian': '<', 'binary_big_endian': '>'}[fmt]
            dtype = np.dtype([(n, order + t) for n, t in props])
            data = np.frombuffer(f.read(n_vertex * dtype.itemsize), dtype=dtype, count=n_vertex)
            rgb = np.stack([data['red'], data['green'], data['blue']], axis=1)
        return rgb.astype(np.float32) / np.float32(255.0)


def write_ply_mesh(filename, vertices, faces, normals=None, colors=None):
    """Binary little-endian PLY of a triangle mesh: ``vertex`` with the float properties x, y, z (and nx, ny, nz when
    ``normals`` is given, and uchar red, green, blue when ``colors`` f32 [Nv, 1 or 3] in [0, 1] is) and ``face`` with
    ``list uchar int vertex_indices``.  ``read_ply_points`` of ``datasets/ThreeDMatch.py`` reads the vertices of such a
    file as a cloud."""
    cols = [np.ascontiguousarray(vertices, dtype='<f4').reshape(-1, 3)]
    names = ['x', 'y', 'z']
    if normals is not None:
        cols.append(np.ascontiguousarray(normals, dtype='<f4').reshape(-1, 3))
        names += ['nx', 'ny', 'nz']
        if cols[1].shape != cols[0].shape:
            raise ValueError("%d normals for %d vertices" % (cols[1].shape[0], cols[0].shape[0]))
    f3 = np.asarray(faces).reshape(-1, 3)
    if f3.size and (f3.min() < 0 or f3.max() >= cols[0].shape[0]):
        raise ValueError("face entries must be vertex indices in 0..%d" % (cols[0].shape[0] - 1))
    rows = np.zeros(f3.shape[0], dtype=[('n', 'u1'), ('i', '<i4', (3,))])
    rows['n'], rows['i'] = 3, f3
    vertex_rows, header = _ply_vertex_rows(cols, names, colors)
    with open(filename, 'wb') as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\n%selement face %d\n"
                 "property list uchar int vertex_indices\nend_header\n"
                 % (cols[0].shape[0], header, f3.shape[0])).encode('ascii'))
        f.write(vertex_rows)
        f.write(rows.tobytes())


def write_fragments(root, scene, clouds, poses, frames_per_fragment, seq='seq-01', num_frames=None):
    """``<root>/fragments/<scene>/cloud_bin_<i>.ply`` and ``cloud_bin_<i>.info.txt`` (header ``<scene>\\t<seq>\\t<first
    frame>\\t<last frame>``, then the 4x4 fragment-to-world pose with 17 significant digits), the layout
    ``preprocess.read_scene`` reads.  ``num_frames``: the length of the sequence, so that a shorter last fragment names
    its true last frame (None: every fragment is taken to be full).  Returns the folder."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    if poses.shape[0] != len(clouds):
        raise ValueError("%d poses for %d clouds" % (poses.shape[0], len(clouds)))
    path = join(root, 'fragments', scene)
    os.makedirs(path, exist_ok=True)
    k = int(frames_per_fragment)
    for i, (c, P) in enumerate(zip(clouds, poses)):
        write_ply_points(join(path, 'cloud_bin_%d.ply' % i), c)
        with open(join(path, 'cloud_bin_%d.info.txt' % i), 'w') as f:
            last = (i + 1) * k if num_frames is None else min((i + 1) * k, int(num_frames))
            f.write("%s\t%s\t%d\t%d\n" % (scene, seq, i * k, last - 1))
            for row in P:
                f.write("\t".join("%.17g" % x for x in row) + "\n")
    return path


def read_sequence(folder, require_poses=True, color=False):
    """``(depth uint16 [F,H,W], intrinsics f64 [4] = fx, fy, cx, cy, poses f64 [F,4,4])`` of a 3DMatch raw sequence
    folder: ``frame-%06d.depth.png`` (16-bit), ``frame-%06d.pose.txt`` (camera-to-world), and ``camera-intrinsics.txt``
    (3x3) in the folder or in its parent.  ``require_poses=False``: a sequence in which a pose file is missing gives
    ``poses = None`` (``track_sequence`` makes them) instead of an error.  ``color=True`` appends uint8 [F,H,W,3]
    (R, G, B) from ``frame-%06d.color.png`` next to every depth image (``track_sequence(color=)`` takes it); a missing
    colour file, or one whose size is not the depth's, raises ``ValueError``."""
    try:
        from PIL import Image
    except ImportError as e:
        raise RuntimeError("read_sequence needs Pillow to read the 16-bit depth PNGs (import PIL failed: %s)" % e)
    names = sorted(n for n in os.listdir(folder) if re.fullmatch(r'frame-\d+\.depth\.png', n))
    if not names:
        raise ValueError("%s: no frame-*.depth.png" % folder)
    for where in (folder, os.path.dirname(os.path.abspath(folder))):
        if exists(join(where, 'camera-intrinsics.txt')):
            Kmat = np.loadtxt(join(where, 'camera-intrinsics.txt'), dtype=np.float64)
            break
    else:
        raise ValueError("%s: no camera-intrinsics.txt here or one folder up" % folder)
    if Kmat.shape != (3, 3):
        raise ValueError("camera-intrinsics.txt: expected a 3x3 matrix, got %s" % (Kmat.shape,))
    depth, poses, rgb = [], [], []
    tracked = require_poses or all(exists(join(folder, n.replace('.depth.png', '.pose.txt'))) for n in names)
    for n in names:
        with Image.open(join(folder, n)) as im:
            a = np.array(im)
        if a.ndim != 2 or a.min() < 0 or a.max() > 65535:
            raise ValueError("%s: not a single-channel 16-bit image" % n)
        depth.append(a.astype(np.uint16))
        if color:
            cn = n.replace('.depth.png', '.color.png')
            if not exists(join(folder, cn)):
                raise ValueError("%s: no %s next to %s" % (folder, cn, n))
            with Image.open(join(folder, cn)) as im:
                c = np.array(im.convert('RGB'))
            if c.shape[:2] != a.shape:
                raise ValueError("%s is %d x %d, its depth image %d x %d: the colour must be registered to the depth"
                                 % (cn, c.shape[1], c.shape[0], a.shape[1], a.shape[0]))
            rgb.append(c.astype(np.uint8))
        if not tracked:
            continue
        P = np.loadtxt(join(folder, n.replace('.depth.png', '.pose.txt')), dtype=np.float64)
        if P.shape != (4, 4):
            raise ValueError("%s: expected a 4x4 pose" % n.replace('.depth.png', '.pose.txt'))
        poses.append(P)
    if len({d.shape for d in depth}) != 1:
        raise ValueError("%s: the depth images differ in size" % folder)
    res = (np.stack(depth), np.array([Kmat[0, 0], Kmat[1, 1], Kmat[0, 2], Kmat[1, 2]]),
           np.stack(poses) if tracked else None)
    return res + (np.stack(rgb),) if color else res
