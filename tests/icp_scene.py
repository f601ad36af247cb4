"""Surface scene for the ICP tests (test_icp_cpu.py, test_icp_gpu.py): points ON walls, a floor, a sphere and a table
top -- not in a volume, because ICP on 3DMatch slides along planes -- seen as fragments around view centres, each in its
own random pose with its own noise."""
import numpy as np


def rotation(rng, angle=None):
    """Rotation about a random axis by ``angle`` radians (default: uniform in [0, pi))."""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = rng.uniform(0, np.pi) if angle is None else angle
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def random_pose(rng, shift=1.0):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = rotation(rng), rng.normal(scale=shift, size=3)
    return T


def perturbation(rng, degrees, shift):
    """A rigid motion of ``degrees`` about a random axis and ``shift`` in a random direction."""
    D = np.eye(4)
    D[:3, :3] = rotation(rng, np.deg2rad(degrees))
    v = rng.normal(size=3)
    D[:3, 3] = shift * v / np.linalg.norm(v)
    return D


def room(rng, n=24000):
    """n points on the four walls and the floor of a 3 x 2.5 x 2 room, a sphere of radius 0.4 and a table top."""
    parts = []
    k = n // 8
    u = lambda m, lo, hi: rng.uniform(lo, hi, size=m)
    parts.append(np.stack([u(2 * k, 0, 3), u(2 * k, 0, 2.5), np.zeros(2 * k)], 1))            # floor
    parts.append(np.stack([u(k, 0, 3), np.zeros(k), u(k, 0, 2)], 1))                          # wall y = 0
    parts.append(np.stack([u(k, 0, 3), np.full(k, 2.5), u(k, 0, 2)], 1))                      # wall y = 2.5
    parts.append(np.stack([np.zeros(k), u(k, 0, 2.5), u(k, 0, 2)], 1))                        # wall x = 0
    parts.append(np.stack([np.full(k, 3.0), u(k, 0, 2.5), u(k, 0, 2)], 1))                    # wall x = 3
    s = rng.normal(size=(k, 3))
    parts.append(np.array([1.0, 1.2, 0.4]) + 0.4 * s / np.linalg.norm(s, axis=1, keepdims=True))   # sphere
    m = n - 7 * k
    parts.append(np.stack([u(m, 1.8, 2.6), u(m, 0.8, 1.6), np.full(m, 0.75)], 1))            # table top
    return np.concatenate(parts)


def fragment(rng, world, centre, pose, reach=1.6, keep=0.6, noise=0.003, return_ids=False):
    """f32 [n,3]: the world points within ``reach`` of ``centre``, each kept with probability ``keep``, with Gaussian
    noise, expressed in the fragment's frame (``pose`` maps fragment coordinates to world coordinates); with
    ``return_ids`` also the rows of ``world`` they came from."""
    sel = (np.linalg.norm(world - centre, axis=1) < reach) & (rng.uniform(size=len(world)) < keep)
    pts = world[sel] + rng.normal(scale=noise, size=(int(sel.sum()), 3))
    inv = np.linalg.inv(pose)
    out = (pts @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)
    return (out, np.nonzero(sel)[0]) if return_ids else out


def view_centres(num, spacing=1.1):
    """``num`` view centres inside the room, consecutive ones ``spacing`` apart along a zig-zag."""
    out, c, d = [], np.array([0.9, 0.9, 1.0]), np.array([1.0, 0.0, 0.0])
    for k in range(num):
        out.append(c.copy())
        nxt = c + spacing * d
        if not (0.3 <= nxt[0] <= 2.7 and 0.3 <= nxt[1] <= 2.2):
            d = np.array([-d[1], d[0], 0.0]) if k % 2 == 0 else np.array([d[1], -d[0], 0.0])
            nxt = c + spacing * d
            if not (0.3 <= nxt[0] <= 2.7 and 0.3 <= nxt[1] <= 2.2):
                d = -d
                nxt = c + spacing * d
        c = nxt
    return out


def make_scene(seed, num_frag=2, n=24000, spacing=1.1, return_world=False):
    """(clouds, poses): ``num_frag`` f32 fragments of one room and their fragment-to-world poses; with ``return_world``
    also the room's points and, per fragment, the rows of them it holds."""
    rng = np.random.default_rng(seed)
    world = room(rng, n)
    clouds, poses, ids = [], [], []
    for c in view_centres(num_frag, spacing):
        pose = random_pose(rng)
        pts, rows = fragment(rng, world, c, pose, return_ids=True)
        clouds.append(pts)
        poses.append(pose)
        ids.append(rows)
    return (clouds, poses, world, ids) if return_world else (clouds, poses)


def position_descriptors(rng, world, ids, dim=32, wavelength=0.25, jitter=0.02):
    """Unit descriptors that are a smooth function of where a point lies in the room (random Fourier features of the
    world position, read at a position jittered per fragment point): the nearest descriptor of another fragment belongs
    to a NEARBY point, not to the same one -- keypoint matches with a localisation error, as real ones have."""
    W = rng.normal(scale=2 * np.pi / wavelength, size=(3, dim))
    phase = rng.uniform(0, 2 * np.pi, size=dim)
    out = []
    for rows in ids:
        pos = world[rows] + rng.normal(scale=jitter, size=(len(rows), 3))
        d = np.cos(pos @ W + phase)
        out.append((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32))
    return out


def shift_clouds(clouds, shift):
    """Every fragment's own frame moved away from the origin: f32(points + shift)."""
    return [(c.astype(np.float64) + np.asarray(shift, dtype=np.float64)).astype(np.float32) for c in clouds]


def shift_pose(T, shift):
    """The transform between two fragments after ``shift_clouds``: S T inv(S) with S the translation by ``shift``."""
    S = np.eye(4)
    S[:3, 3] = shift
    return S @ np.asarray(T, dtype=np.float64) @ np.linalg.inv(S)


def gt_transform(poses, i, j):
    """Maps fragment j into fragment i (the gt.log convention for key i_j)."""
    return np.linalg.inv(poses[i]) @ poses[j]


def pose_error(T, G):
    """(rotation error in degrees, translation error) of T against G."""
    D = np.linalg.inv(G) @ T
    c = np.clip((np.trace(D[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)
    return float(np.rad2deg(np.arccos(c))), float(np.linalg.norm(D[:3, 3]))
