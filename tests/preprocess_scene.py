"""Seeded synthetic scenes for the preprocessing tests: ``synthetic.raw_fragment`` (one indoor-like cloud in the world
frame) cut into overlapping windows along x, every window handed out in a frame of its own with a known pose."""
import os

import numpy as np

from d3feat_pytorch_amd import synthetic


def pose(angle_z, t, angle_x=0.0):
    c, s = np.cos(angle_z), np.sin(angle_z)
    Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    c, s = np.cos(angle_x), np.sin(angle_x)
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Rx
    T[:3, 3] = t
    return T


def make_scene(n_frag=6, seed=3, n_raw=60000, scale=0.4, window=0.5, stride=0.15):
    """(fragments: list of f32 [N,3] in their own frames, poses [F,4,4] f64 fragment-to-world).  Windows k and k + d
    share ``window - d * stride`` of their extent, so the overlap structure is known from the geometry."""
    world = synthetic.raw_fragment(seed, n_raw=n_raw, scale=scale).astype(np.float64)
    frags, poses = [], []
    for k in range(n_frag):
        lo = stride * k
        P = pose(0.3 * k + 0.1, [0.1 * k, -0.2, 0.05 * k], angle_x=0.07 * k)
        w = world[(world[:, 0] >= lo) & (world[:, 0] < lo + window)]
        frags.append(((w - P[:3, 3]) @ P[:3, :3]).astype(np.float32))      # inv(P) applied
        poses.append(P)
    return frags, np.stack(poses)


def write_ply(path, pts):
    pts = np.asarray(pts, dtype=np.float32)
    with open(path, 'wb') as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\n"
                 "property float z\nend_header\n" % len(pts)).encode())
        f.write(pts.astype('<f4').tobytes())


def write_scene(root, scene, frags, poses, how='info'):
    """<root>/fragments/<scene>/cloud_bin_<i>.ply with the poses as cloud_bin_<i>.info.txt or as poses.npy."""
    path = os.path.join(str(root), 'fragments', scene)
    os.makedirs(path, exist_ok=True)
    for i, (pts, P) in enumerate(zip(frags, poses)):
        write_ply(os.path.join(path, 'cloud_bin_%d.ply' % i), pts)
        if how == 'info':
            with open(os.path.join(path, 'cloud_bin_%d.info.txt' % i), 'w') as f:
                f.write('%s\t0\t%d\t%d\n' % (scene, i * 50, i * 50 + 49))
                for row in P:
                    f.write('\t'.join('%.17g' % v for v in row) + '\n')
    if how == 'npy':
        np.save(os.path.join(path, 'poses.npy'), np.asarray(poses, dtype=np.float64))
    return path
