"""Inputs and callers shared by the tests of the eight TSDF integrate and ray-cast entries of include/d3feat_hip.h
(test_tsdf_entries_cpu.py: the four host twins; test_tsdf_entries_gpu.py: the four device forms against them), which
are called directly through ``_native.lib()``, argument by argument as the header lists them.

Two dense volumes: dims (9, 5, 3), two bricks along x of which the second is partial, and (2, 2, 2), smaller than one
wave.  Two f32 depth frames of 8 x 6 look at a tilted plane through both.  ``FRAME_START`` gives both frames to the
first volume and none to the second.  The sparse tables come from ``ops.tsdf_allocate_host`` with a frame for each
volume, so that the second volume has a pool row although it owns no frame in the calls under test."""
import collections
import functools

import numpy as np
import torch

from d3feat_pytorch_amd import _native, ops

f32 = np.float32
EINVAL = _native.D3F_EINVAL
BAD_CHANNELS = (-1, 2, 4)

# the sixteen entries that `channels` and `into` replaced
REMOVED_ENTRIES = (["d3f_tsdf%s_integrate%s%s" % (kind, form, twin) for kind in ("", "_sparse")
                    for form in ("_color", "_into", "_color_into") for twin in ("", "_host")] +
                   ["d3f_tsdf_raycast%s_color%s" % (kind, twin) for kind in ("", "_sparse") for twin in ("", "_host")])

H, W, F, V = 6, 8, 2, 2
DIMS = np.array([[9, 5, 3], [2, 2, 2]], dtype=np.int32)
ORIGIN = np.array([[-0.2, -0.1, 0.45], [-0.05, -0.05, 0.46]], dtype=f32)
VOXEL = np.array([0.05, 0.05], dtype=f32)
TRUNC = np.array([0.1, 0.1], dtype=f32)
VOL_START = np.array([0, 135, 143], dtype=np.int64)
TOTAL, LARGEST = 143, 135
FRAME_START = np.array([0, 2, 2], dtype=np.int32)
ONE_FRAME = np.array([0, 1, 1], dtype=np.int32)              # of a one-frame call: the second volume again has none
DEPTH_SCALE, DEPTH_MAX = 1000.0, 6.0
K = np.tile(np.array([8.0, 8.0, 3.5, 2.5], dtype=f32), (F, 1))


def _scene():
    v, u = np.mgrid[0:H, 0:W].astype(f32)
    depth = np.stack([f32(0.5) + f32(0.01) * (u - f32(3.5)) + f32(0.008) * (v - f32(2.5)) + f32(0.004 * f)
                      for f in range(F)]).astype(f32)
    depth[0, 1, 2] = 0.0                                     # an invalid pixel
    M = np.zeros((F, 12), dtype=f32)                         # volume -> camera: frame 1 stands 1 cm to the side
    M[:, 0] = M[:, 5] = M[:, 10] = 1.0
    M[1, 3] = 0.01
    C = M.copy()                                             # camera -> volume, the inverse
    C[1, 3] = -0.01
    return np.ascontiguousarray(depth), M, C


DEPTH, M, C = _scene()


def colour(channels):
    """The colour frames f32 [F, H, W, channels]."""
    n = F * H * W * channels
    return (f32(0.5) + f32(0.4) * np.sin(f32(0.37) * np.arange(n, dtype=f32))).astype(f32).reshape(F, H, W, channels)


@functools.lru_cache(maxsize=None)
def sparse_volumes():
    """The tables, as arrays: frame 0 allocates the first volume's bricks and frame 1 the second's."""
    sv = ops.tsdf_allocate_host(DEPTH, [0, 1, 2], K, C.reshape(F, 3, 4), ORIGIN, DIMS, VOXEL, TRUNC,
                                depth_scale=DEPTH_SCALE, depth_max=DEPTH_MAX)
    sv = ops.SparseVolumes(*[np.ascontiguousarray(ops._host_array(a)) for a in
                             (sv.brick_index, sv.brick_coord, sv.brick_start)], sv.origin, sv.dims, sv.voxel)
    assert sv.brick_start.tolist() == [0, 2, 3], sv.brick_start      # both bricks of the first volume, the second's one
    return sv


def in_lattice(sv):
    """bool [B, 512]: the slots of the pool that are voxels of their volume."""
    s = np.arange(512)
    own = np.searchsorted(sv.brick_start, np.arange(sv.bricks), side='right') - 1
    i = sv.brick_coord[:, None, :] * 8 + np.stack([s & 7, (s >> 3) & 7, s >> 6], axis=-1)[None]
    return (i < sv.dims[own][:, None, :]).all(axis=-1)


class Side(object):
    """Where an entry's pointers live: host arrays for the twins, device tensors for the device forms."""

    def __init__(self, host):
        self.host, self.suffix = host, "_host" if host else ""

    def put(self, a):
        if a is None or self.host:
            return a
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def get(self, a):
        return a if a is None or self.host else a.cpu().numpy()

    def ptr(self, a):
        if a is None:
            return None
        return a.ctypes.data if self.host else a.data_ptr()

    def stream(self):
        return None if self.host else torch.cuda.current_stream().cuda_stream


HOST, DEVICE = Side(True), Side(False)


def call(side, stem, args):
    """The return code of entry `stem` (+ _host); ``args``: name -> array (input), tensor of ``side`` or scalar, in the
    header's order without the stream."""
    held = [side.put(a) if isinstance(a, np.ndarray) else a for a in args.values()]
    flat = [side.ptr(a) if a is None or isinstance(a, (np.ndarray, torch.Tensor)) else a for a in held]
    fn = getattr(_native.lib(), stem + side.suffix)
    assert len(flat) + 1 == len(_native.SIGNATURES[stem + side.suffix][1])
    rc = fn(*(flat + [side.stream()]))
    if not side.host:
        torch.cuda.synchronize()
    return rc


def integrate_args(sparse, channels, into, frames, frame_start, D, w, Cx, replace):
    """The argument list of d3f_tsdf_integrate / d3f_tsdf_sparse_integrate over ``frames`` (a slice) of the scene.
    ``D``, ``w``, ``Cx``: the outputs, already on their side.  ``replace``: {name: value}, to break arguments."""
    a = collections.OrderedDict()
    a['depth'] = DEPTH[frames]
    # bad channels: every pointer is there all the same
    a['color'] = np.ascontiguousarray(colour(abs(channels))[frames]) if channels else None
    a['channels'], a['depth_is_f32'] = channels, 1
    a['F'], a['H'], a['W'] = DEPTH[frames].shape
    a['frame_start'] = frame_start
    if sparse:
        sv = sparse_volumes()
        a['V'] = V
    else:
        a['vol_start'], a['V'], a['total_voxels'], a['max_volume_voxels'] = VOL_START, V, TOTAL, LARGEST
    a['intrinsics'], a['volume_to_camera'] = K[frames], M[frames]
    a['origin'], a['dims'], a['voxel'], a['trunc'] = ORIGIN, DIMS, VOXEL, TRUNC
    if sparse:
        a['brick_start'], a['brick_coord'], a['bricks'] = sv.brick_start, sv.brick_coord, sv.bricks
    a['depth_scale'], a['depth_max'], a['into'] = DEPTH_SCALE, DEPTH_MAX, into
    a['D'], a['w'], a['C'] = D, w, Cx
    assert set(replace) <= set(a), replace
    a.update(replace)
    return a


def cells(sparse):
    return sparse_volumes().bricks * 512 if sparse else TOTAL


def outputs(side, sparse, channels, fill=np.nan):
    """Fresh D, w and Cv / Cp (None without colour) on ``side``, holding ``fill``: NaN shows a cell that was not
    written."""
    n = cells(sparse)
    return (side.put(np.full(n, fill, dtype=f32)), side.put(np.full(n, fill, dtype=f32)),
            side.put(np.full((n, abs(channels)), fill, dtype=f32)) if channels else None)


def integrate(side, sparse, channels, into=0, frames=slice(0, F), frame_start=FRAME_START, out=None, **replace):
    """(rc, D, w, Cx) as host arrays; ``out``: the (D, w, Cx) on ``side`` to write into, fresh ones otherwise."""
    D, w, Cx = out if out is not None else outputs(side, sparse, channels)
    stem = "d3f_tsdf_sparse_integrate" if sparse else "d3f_tsdf_integrate"
    rc = call(side, stem, integrate_args(sparse, channels, into, frames, frame_start, D, w, Cx, replace))
    return rc, side.get(D), side.get(w), side.get(Cx)


# the views of the ray-casts: the first volume from both frame poses and the second, which holds nothing, once
VIEW_VOLUME = np.array([0, 1, 0], dtype=np.int32)
R = 3
VIEW_K = np.tile(K[0], (R, 1))
VIEW_C = np.ascontiguousarray(C[[0, 0, 1]])
STEP = np.array([0.025, 0.025], dtype=f32)
RAY = dict(depth_min=0.1, depth_max=DEPTH_MAX, min_weight=1.0, clip=1)


def raycast_args(sparse, channels, D, w, Cx, depth, normals, image, replace):
    a = collections.OrderedDict()
    a['D'], a['w'], a['C'], a['channels'] = D, w, Cx, channels
    if sparse:
        sv = sparse_volumes()
        a['lattice_start'], a['brick_start'], a['brick_index'] = sv.lattice_start, sv.brick_start, sv.brick_index
    else:
        a['vol_start'] = VOL_START
    a['origin'], a['dims'], a['voxel'], a['V'] = ORIGIN, DIMS, VOXEL, V
    if sparse:
        a['lattice_bricks'], a['bricks'] = int(sv.lattice_start[-1]), sv.bricks
    else:
        a['total_voxels'] = TOTAL
    a['view_volume'], a['R'], a['H'], a['W'] = VIEW_VOLUME, R, H, W
    a['intrinsics'], a['camera_to_volume'], a['step'] = VIEW_K, VIEW_C, STEP
    a['depth_min'], a['depth_max'], a['min_weight'], a['clip'] = (RAY[k] for k in ('depth_min', 'depth_max',
                                                                                      'min_weight', 'clip'))
    if sparse:
        a['skip'] = 1
    a['depth'], a['normals'], a['color'] = depth, normals, image
    assert set(replace) <= set(a), replace
    a.update(replace)
    return a


def raycast(side, sparse, channels, D, w, Cx, **replace):
    """(rc, depth [R,H,W], normals [R,H,W,3], colour image [R,H,W,channels] or None) of the model D, w, Cx (arrays)."""
    depth, normals = side.put(np.full((R, H, W), np.nan, dtype=f32)), side.put(np.full((R, H, W, 3), np.nan, dtype=f32))
    image = side.put(np.full((R, H, W, abs(channels)), 7.0, dtype=f32)) if channels else None
    stem = "d3f_tsdf_raycast_sparse" if sparse else "d3f_tsdf_raycast"
    rc = call(side, stem, raycast_args(sparse, channels, D, w, Cx, depth, normals, image, replace))
    return rc, side.get(depth), side.get(normals), side.get(image)


def same(a, b):
    """Bit for bit, NaN included."""
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------ references
@functools.lru_cache(maxsize=None)
def numpy_model(sparse, channels):
    """(D, w, Cx or None) of the restatement over both frames; computed once, do not modify."""
    col = dict(color=colour(channels)) if channels else {}
    kw = dict(depth_scale=DEPTH_SCALE, depth_max=DEPTH_MAX, **col)
    if sparse:
        out = ops.tsdf_sparse_numpy(DEPTH, FRAME_START, K, M.reshape(F, 3, 4), sparse_volumes(), TRUNC, **kw)
        out = tuple(a.reshape((-1,) + a.shape[2:]) for a in out)
    else:
        out = ops.tsdf_numpy(DEPTH, FRAME_START, K, M.reshape(F, 3, 4), ORIGIN, DIMS, VOXEL, TRUNC, **kw)
        out = (out[0], out[1]) + tuple(out[3:])
    assert (out[1] > 0).any() and (out[1][-8:] == 0).all()           # something is fused; the frameless volume is empty
    return tuple(out) + ((None,) if not channels else ())


@functools.lru_cache(maxsize=None)
def numpy_render(sparse, channels):
    """(depth, normals, colour image or None) of the restatement's ray-cast of numpy_model(sparse, channels)."""
    D, w, Cx = numpy_model(sparse, channels)
    kw = dict(view_volume=VIEW_VOLUME, step=STEP, depth_min=RAY['depth_min'], depth_max=RAY['depth_max'],
              min_weight=RAY['min_weight'], normals=True, clip=True, **(dict(color=Cx) if channels else {}))
    if sparse:
        sv = sparse_volumes()
        shape = (sv.bricks, 512)
        kw['color'] = None if Cx is None else Cx.reshape(shape + (channels,))
        out = ops.tsdf_raycast_sparse_numpy(D.reshape(shape), w.reshape(shape), sv, None, VIEW_K,
                                            VIEW_C.reshape(R, 3, 4), H, W, **kw)
    else:
        out = ops.tsdf_raycast_numpy(D, w, VOL_START, ORIGIN, DIMS, VOXEL, None, VIEW_K, VIEW_C.reshape(R, 3, 4), H, W,
                                     **kw)
    out = tuple(np.asarray(a) for a in out)
    assert (out[0][0] > 0).any() and (out[0][2] > 0).any() and not out[0][1].any()     # hits, and none in the empty one
    return out + ((None,) if not channels else ())


# ---------------------------------------------------------------------------------------------------------- checks
def check_bad_channels(side):
    """channels other than 0, 1, 3: D3F_EINVAL from all four entries, before anything else is looked at -- where
    channels = 0 with the same arguments is D3F_OK because the model is empty or there is no view -- and nothing is
    written."""
    for sparse in (False, True):
        empty = dict(bricks=0) if sparse else dict(total_voxels=0, max_volume_voxels=0)
        for channels in BAD_CHANNELS + (0,):
            want = 0 if channels == 0 else EINVAL
            nothing = dict(D=None, w=None, C=None, **empty)
            assert integrate(side, sparse, channels, **nothing)[0] == want, (sparse, channels)
            rc, D, w, _ = integrate(side, sparse, channels)
            assert rc == want and (channels == 0 or (np.isnan(D).all() and np.isnan(w).all())), (sparse, channels)
        D, w, _ = numpy_model(sparse, 0)
        for channels in BAD_CHANNELS + (0,):
            want = 0 if channels == 0 else EINVAL
            no_view = dict(R=0, depth=None, normals=None, color=None)
            assert raycast(side, sparse, channels, D, w, None, **no_view)[0] == want, (sparse, channels)
            rc, depth, _, _ = raycast(side, sparse, channels, D, w, None)
            assert rc == want and (channels == 0 or np.isnan(depth).all()), (sparse, channels)
            if channels:
                no_model = dict(depth=None, normals=None, color=None, **(empty if sparse else dict(total_voxels=0)))
                assert raycast(side, sparse, channels, None, None, None, **no_model)[0] == EINVAL, (sparse, channels)


def check_colour_pointers(side, sparse, channels):
    """channels 1 or 3: integrate needs color (F > 0) and Cv / Cp; a ray-cast needs the image and Cv / Cp."""
    assert integrate(side, sparse, channels, color=None)[0] == EINVAL
    assert integrate(side, sparse, channels, C=None)[0] == EINVAL
    D, w, Cx = numpy_model(sparse, channels)
    assert raycast(side, sparse, channels, D, w, Cx, color=None)[0] == EINVAL
    assert raycast(side, sparse, channels, D, w, None)[0] == EINVAL


def check_into(side, sparse, channels):
    """Frame 0 from zero, then frame 1 with into = 1: the cells of the first volume are those of one call over both
    frames, bit for bit; the second volume, which owns no frame, and the slots beyond dims keep the sentinels written
    before the second call.  Returns the (D, w, Cx) of the one call."""
    rc, *whole = integrate(side, sparse, channels)
    assert rc == 0
    out = outputs(side, sparse, channels)
    assert integrate(side, sparse, channels, 0, slice(0, 1), ONE_FRAME, out)[0] == 0
    n = cells(sparse)
    continued = (in_lattice(sparse_volumes()).reshape(-1) & (np.arange(n) < 2 * 512)) if sparse else np.arange(n) < 135
    for j, a in enumerate(out[:3 if channels else 2]):
        assert not side.get(a)[~continued].any()                      # from zero: written, and nothing fused there
        marks = np.broadcast_to(f32(-3.0 - j), a.shape)
        if side.host:
            a[~continued] = marks[~continued]
        else:
            a[torch.from_numpy(~continued).cuda()] = -3.0 - j
    rc, *split = integrate(side, sparse, channels, 1, slice(1, 2), ONE_FRAME, out)
    assert rc == 0
    for j, (a, b) in enumerate(zip(split, whole)):
        if a is not None:
            assert same(a[continued], b[continued]), (sparse, channels, j)
            assert (a[~continued] == f32(-3.0 - j)).all() and (~continued).sum() >= 8, (sparse, channels, j)
    return whole
