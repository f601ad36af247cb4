"""Cases of the coloured ICP tests (test_colored_icp_cpu.py, test_colored_icp_gpu.py): clouds painted with the smooth
texture ``rgbd_cases.tex`` at their world points.  Radius 0.1 for normals and gradients, max_distance 0.075 throughout."""
import numpy as np
import icp_scene as sc
from rgbd_cases import tex

R_ICP = 0.075          # max_distance
R_GRAD = 0.1           # radius of normals and gradients


def plane_slide(seed=7, n=5000, slide=0.03, deg=1.5, noise=0.002):
    """Two independent samples of the textured plane z = 0 over [0,1.5]^2, each in a random frame of its own;
    -> clouds, intensities, G (maps cloud 1 into cloud 0), T0 (G with an in-plane slide and a turn about the normal)."""
    rng = np.random.default_rng(seed)
    clouds, cols, poses = [], [], []
    for _ in range(2):
        w = np.stack([rng.uniform(0, 1.5, n), rng.uniform(0, 1.5, n), np.zeros(n)], 1)
        I = tex(w[:, 0], w[:, 1], w[:, 2]).astype(np.float32)
        pose = sc.random_pose(rng)
        inv = np.linalg.inv(pose)
        pts = w + rng.normal(scale=noise, size=w.shape)
        clouds.append((pts @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)); cols.append(I); poses.append(pose)
    a = np.deg2rad(deg)
    D = np.eye(4); D[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]; D[:3, 3] = [0.8 * slide, 0.6 * slide, 0]
    c = np.eye(4); c[:3, 3] = [0.75, 0.75, 0]
    return clouds, cols, sc.gt_transform(poses, 0, 1), np.linalg.inv(poses[0]) @ (c @ D @ np.linalg.inv(c)) @ poses[1]


def paint(world, ids):
    """f32 intensities of the fragments whose points are the rows ``ids`` of ``world``."""
    return [tex(world[r, 0], world[r, 1], world[r, 2]).astype(np.float32) for r in ids]


def room():
    """The clouds, keys, pairs, G, T0 of ``test_normals_plane_cpu.perturbed_pairs()`` and the fragments' intensities."""
    from test_normals_plane_cpu import perturbed_pairs
    clouds, keys, pairs, G, T0 = perturbed_pairs()
    same, _, world, ids = sc.make_scene(4, 4, return_world=True)
    assert all(np.array_equal(a, b) for a, b in zip(clouds, same))
    return clouds, paint(world, ids), keys, pairs, G, T0


def ramp():
    """700 points of a plane with the linear intensity 0.2 + 0.5 x + 0.4 y, in a random frame -> cloud, intensity, the
    plane's normal and the exact gradient in that frame."""
    rng = np.random.default_rng(11)
    x = rng.uniform(0, 0.6, 700)
    y = rng.uniform(0, 0.6, 700)
    w = np.stack([x, y, np.zeros(700)], 1)
    I = (0.2 + 0.5 * x + 0.4 * y).astype(np.float32)
    pose = sc.random_pose(rng)
    inv = np.linalg.inv(pose)
    cloud = (w @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    return cloud, I, inv[:3, :3] @ np.array([0.0, 0.0, 1.0]), inv[:3, :3] @ np.array([0.5, 0.4, 0.0])


def small():
    """``sc.make_scene(4, 2, n=6000)`` painted: clouds, intensities."""
    clouds, _, world, ids = sc.make_scene(4, 2, n=6000, return_world=True)
    return clouds, paint(world, ids)


def shifted(clouds, T, shift):
    """The clouds and the poses between them after every frame moved by ``shift``."""
    return sc.shift_clouds(clouds, shift), np.stack([sc.shift_pose(t, shift) for t in T])
