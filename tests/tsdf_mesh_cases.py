"""Volumes and measures shared by the TSDF mesh tests (csrc/tsdf_mesh.hpp): five analytic volumes, the room and the
small volumes of ``tsdf_scene`` as arguments of ``ops.tsdf_mesh*``, the topology of a triangle list, and an independent
NumPy count of the quads a volume must give."""
import functools

import numpy as np

import tsdf_scene as S

N, VOXEL = 24, 0.05                   # every analytic volume: a 24^3 lattice at the origin, w = 1
CENTER = (0.6, 0.55, 0.58)
RADIUS = 0.3
CUT_CENTER = (0.1, 0.55, 0.58)


def _lattice():
    i = np.arange(N, dtype=np.float64) * VOXEL
    z, y, x = np.meshgrid(i, i, i, indexing='ij')            # memory order: ix fastest
    return x, y, z


def _tsdf(sdf, trunc):
    return np.clip(sdf / trunc, -1.0, 1.0).astype(np.float32).reshape(-1)


def _sphere(center):
    x, y, z = _lattice()
    return np.sqrt((x - center[0]) ** 2 + (y - center[1]) ** 2 + (z - center[2]) ** 2) - RADIUS


def _volume(D, w=None, dims=(N, N, N), voxel=VOXEL):
    D = np.ascontiguousarray(D, dtype=np.float32).reshape(-1)
    w = np.ones_like(D) if w is None else np.ascontiguousarray(w, dtype=np.float32).reshape(-1)
    for a in (D, w):
        a.setflags(write=False)
    return dict(D=D, w=w, vol_start=None, origin=[[0.0, 0.0, 0.0]], dims=[list(dims)], voxel=voxel)


@functools.lru_cache(maxsize=None)
def analytic():
    """name -> keyword arguments of ``ops.tsdf_mesh`` (one volume each); shared, do not modify."""
    x, y, z = _lattice()
    torus = np.sqrt((np.sqrt((x - CENTER[0]) ** 2 + (y - CENTER[1]) ** 2) - 0.35) ** 2 + (z - CENTER[2]) ** 2) - 0.12
    holed_w = np.ones((N, N, N), dtype=np.float32)
    holed_w[14:] = 0.0                                       # iz >= 14
    return {
        'sphere': _volume(_tsdf(_sphere(CENTER), 0.2)),
        'torus': _volume(_tsdf(torus, 0.1)),
        'cut_sphere': _volume(_tsdf(_sphere(CUT_CENTER), 0.2)),
        'holed_sphere': _volume(_tsdf(_sphere(CENTER), 0.2), holed_w),
        'empty': _volume(np.full(N ** 3, 0.5, dtype=np.float32)),
    }


@functools.lru_cache(maxsize=None)
def room():
    """The two fragment volumes of the room in one batch, by the NumPy restatement (``min_weight`` is left open)."""
    from d3feat_pytorch_amd import ops
    from d3feat_pytorch_amd.datasets import fragments as fr
    depth, fs, K, M, C = S.fragment_setup()
    origin, dims = fr.place_volumes(ops.tsdf_bounds_numpy(depth, fs, K, C), S.VOXEL)
    D, w, vs = ops.tsdf_numpy(depth, fs, K, M, origin, dims, S.VOXEL, S.TRUNC)
    for a in (D, w):
        a.setflags(write=False)
    return dict(D=D, w=w, vol_start=vs, origin=origin, dims=dims, voxel=S.VOXEL)


@functools.lru_cache(maxsize=None)
def small(name):
    """The small volume ``name`` of ``tsdf_scene.small_cases()``, integrated by the NumPy restatement."""
    from d3feat_pytorch_amd import ops
    case = S.small_cases()[name]
    D, w, vs = ops.tsdf_numpy(**S.integrate_args(case))
    for a in (D, w):
        a.setflags(write=False)
    return dict(D=D, w=w, vol_start=vs, origin=[case['origin']], dims=[case['dims']], voxel=case['voxel'])


def all_cases():
    """(name, arguments, min_weight) of every volume the tests mesh."""
    out = [(name, args, 1.0) for name, args in analytic().items()]
    out += [('room_w%d' % mw, room(), float(mw)) for mw in (1, 2)]
    out += [(name, small(name), 1.0) for name in sorted(S.small_cases())]
    return out


# ------------------------------------------------------------------------------------------------------ topology
def edge_counts(faces):
    """(undirected multiplicities, directed multiplicities) of the edges of a triangle list [F,3]."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    directed = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], axis=0)
    span = int(f.max()) + 1 if f.size else 1
    d_mult = np.unique(directed[:, 0] * span + directed[:, 1], return_counts=True)[1]
    u_mult = np.unique(directed.min(1) * span + directed.max(1), return_counts=True)[1]
    return u_mult, d_mult


def euler(vertices, faces):
    """V - E + F over the vertices that a face uses."""
    f = np.asarray(faces).reshape(-1, 3)
    return int(np.unique(f).size) - int(edge_counts(f)[0].size) + int(f.shape[0])


# ------------------------------------------------------------------------------------- quads, counted independently
def expected_quads(D, w, dims, min_weight=1.0):
    """Per volume, the number of points ``tsdf_extract`` emits (valid lower and upper voxel, signs differ) whose edge has
    four COMPLETE cells around it: plain NumPy on D and w, no mesh code."""
    D = np.asarray(D, dtype=np.float32).reshape(-1)
    w = np.asarray(w, dtype=np.float32).reshape(-1)
    out, start = [], 0
    for nx, ny, nz in np.asarray(dims).reshape(-1, 3):
        count = int(nx) * int(ny) * int(nz)
        Dv = D[start:start + count].reshape(nz, ny, nx)
        ok = (w[start:start + count].reshape(nz, ny, nx) >= np.float32(min_weight)) & (np.abs(Dv) < 1)
        start += count
        # complete[z, y, x]: the cell of voxel (x, y, z), False where the cell does not exist; one plane of padding
        # below, so that index -1 + 1 = 0 is a cell that does not exist
        complete = np.zeros((nz + 1, ny + 1, nx + 1), dtype=bool)
        if min(nx, ny, nz) > 1:
            c = np.ones((nz - 1, ny - 1, nx - 1), dtype=bool)
            for dz in (0, 1):
                for dy in (0, 1):
                    for dx in (0, 1):
                        c &= ok[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
            complete[1:nz, 1:ny, 1:nx] = c
        quads = 0
        for z in range(nz):                                   # a plain loop over planes keeps this obviously right
            for a, (ex, ey, ez) in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))):
                if z + ez >= nz or ny - ey < 1 or nx - ex < 1:
                    continue
                lo = (z, slice(0, ny - ey), slice(0, nx - ex))
                hi = (z + ez, slice(ey, ny), slice(ex, nx))
                emit = ok[lo] & ok[hi] & ((Dv[lo] < 0) != (Dv[hi] < 0))
                around = np.ones_like(emit)
                others = [k for k in range(3) if k != a]
                for s0 in (-1, 0):
                    for s1 in (-1, 0):
                        off = [0, 0, 0]
                        off[others[0]], off[others[1]] = s0, s1
                        ox, oy, oz = off
                        around &= complete[z + 1 + oz, 1 + oy:1 + oy + ny - ey, 1 + ox:1 + ox + nx - ex]
                quads += int((emit & around).sum())
        out.append(quads)
    return out
