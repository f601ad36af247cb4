"""Writer of the 3DMatch training pickles -- the files ``ThreeDMatchDataset`` reads (reference datasets/ThreeDMatch.py:68-90).

The reference ships no code for this step (its README points to the authors' download), so the rule is stated here
rather than copied: every fragment is voxel-subsampled with the pipeline's own barycentre operator; for a pair (i, j) of
fragments of one scene the points of i are moved into j's frame with ``T_ij = inv(P_j) @ P_i`` (f64, fragment-to-world
poses P) and each looks up its nearest point of j closer than ``radius``; the OVERLAP of (i, j) is the share of i's points
that have one; pairs whose overlap exceeds ``min_overlap`` are kept with their ``(source index, target index)`` list.
The defaults -- ``radius = 1.25 * voxel`` (0.0375 m at 0.03 m, what ``synthetic.make_pair`` uses) and ``min_overlap =
0.3`` (the "less than 30 % overlap" of the reference's test.py) -- are parameters.  Files made here follow THIS rule;
they are not claimed to equal the authors' download, which is not available to compare against.

Arithmetic (the same on both paths, so they agree bit for bit): the moved point is
``f32(((r0 x + r1 y) + r2 z) + t)`` per component in f64; ``d2 = ((dx dx) + (dy dy)) + (dz dz)`` in f32; accepted when
``d2 < f32(radius) * f32(radius)``; the lowest target index among equal d2.  ``device='cuda'`` runs the HIP kernel
``d3f_nearest_pairs`` over one cell list of the whole scene; ``device='cpu'`` is the NumPy restatement (blocked brute
force), the portable path and the oracle of the GPU tests.
"""
import os
import pickle
import re
import warnings
from os.path import exists, join

import numpy as np

from .ThreeDMatch import ThreeDMatchDataset, read_ply_points

SUBSAMPLE_GROUP = 64          # clouds per batched call of the subsampling operator (its D3F_MAX_BATCH)
DEFAULT_MAX_ROWS = 1 << 23    # query rows per kernel launch


# ------------------------------------------------------------------------------------------------------ the contract
def transform_points(points, T):
    """[N,3] f32 ``points`` moved by the 4x4 / 3x4 f64 ``T``: f64 products and sums in the stated order, rounded once."""
    p = np.asarray(points, dtype=np.float32)
    T = np.asarray(T, dtype=np.float64)
    x, y, z = (p[:, k].astype(np.float64) for k in range(3))
    out = np.empty((p.shape[0], 3), dtype=np.float32)
    for r in range(3):
        out[:, r] = (((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]).astype(np.float32)
    return out


def nearest_within(queries, targets, radius, block=1 << 22):
    """int32 [Nq]: per f32 query the index of the nearest f32 target with d2 < radius^2 (f32 rule above), else -1."""
    q = np.ascontiguousarray(queries, dtype=np.float32)
    t = np.ascontiguousarray(targets, dtype=np.float32)
    nn = np.full(q.shape[0], -1, dtype=np.int32)
    if q.shape[0] == 0 or t.shape[0] == 0:
        return nn
    r2 = np.float32(radius) * np.float32(radius)
    # exact shortcut: a point farther than the radius from the other cloud's bounding box in one axis has no partner
    m = float(radius) * 1.001 + 1e-6
    with np.errstate(invalid='ignore'):
        qsel = np.nonzero(np.all((q >= t.min(0).astype(np.float64) - m) & (q <= t.max(0).astype(np.float64) + m), 1))[0]
        if qsel.size == 0:
            return nn
        qq = q[qsel]
        tsel = np.nonzero(np.all((t >= qq.min(0).astype(np.float64) - m) & (t <= qq.max(0).astype(np.float64) + m), 1))[0]
    if tsel.size == 0:
        return nn
    tt = t[tsel]
    step = max(1, int(block) // tt.shape[0])
    for s in range(0, qq.shape[0], step):
        b = qq[s:s + step]
        dx = b[:, None, 0] - tt[None, :, 0]
        d2 = dx * dx
        dy = b[:, None, 1] - tt[None, :, 1]
        d2 = d2 + dy * dy
        dz = b[:, None, 2] - tt[None, :, 2]
        d2 = d2 + dz * dz
        k = np.argmin(d2, axis=1)                      # first occurrence: the lowest index among equal d2
        ok = d2[np.arange(b.shape[0]), k] < r2
        nn[qsel[s:s + step][ok]] = tsel[k[ok]]
    return nn


def nearest_pairs_numpy(clouds, pairs, transforms, radius):
    """The contract of ``ops.nearest_pairs`` in NumPy: ``(nn int32 [rows], count int32 [P], row_start int64 [P+1])``."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    T = np.asarray(transforms, dtype=np.float64)
    row_start = np.zeros(pairs.shape[0] + 1, dtype=np.int64)
    row_start[1:] = np.cumsum([clouds[a].shape[0] for a, _ in pairs])
    nn = np.full(int(row_start[-1]), -1, dtype=np.int32)
    count = np.zeros(pairs.shape[0], dtype=np.int32)
    for p, (a, b) in enumerate(pairs):
        res = nearest_within(transform_points(clouds[a], T[p]), clouds[b], radius)
        nn[row_start[p]:row_start[p + 1]] = res
        count[p] = int((res >= 0).sum())
    return nn, count, row_start


# ------------------------------------------------------------------------------------------------------ subsampling
def _as_clouds(fragments):
    return [np.ascontiguousarray(np.asarray(f, dtype=np.float32).reshape(-1, 3)) for f in fragments]


def subsample_fragments(fragments, voxel, subsample=None, device='cuda'):
    """The fragments as f32 clouds at ``voxel``: ``subsample(points, voxel) -> points`` per fragment when given (as in
    ``ThreeDMatchTestset``), else batched calls of the device barycentre operator; ``voxel=None`` takes them as they are."""
    if voxel is None:
        return _as_clouds(fragments)
    if subsample is not None:
        return _as_clouds([subsample(np.asarray(f), voxel) for f in fragments])
    if str(device).startswith('cpu'):
        raise ValueError("the package has no CPU voxel subsampler: pass subsample=, or voxel=None for clouds that are "
                         "subsampled already")
    import torch
    from .dataloader import batch_grid_subsampling_kpconv
    raw, out = _as_clouds(fragments), []
    for g in range(0, len(raw), SUBSAMPLE_GROUP):
        group = raw[g:g + SUBSAMPLE_GROUP]
        lens = torch.tensor([c.shape[0] for c in group], dtype=torch.int32)
        pts, out_len = batch_grid_subsampling_kpconv(torch.as_tensor(np.concatenate(group, 0)).to(device), lens,
                                                     sampleDl=float(voxel))
        pts, out_len = pts.cpu().numpy(), out_len.cpu().numpy()
        ends = np.cumsum(out_len)
        out.extend(np.ascontiguousarray(pts[e - n:e]) for e, n in zip(ends, out_len))
    return out


# ------------------------------------------------------------------------------------------------------ mining
def _chunks(units, rows_of, max_rows):
    """Consecutive groups of units (lists of pair numbers) of at most ``max_rows`` query rows, one unit at least."""
    out, cur, n = [], [], 0
    for u in units:
        r = sum(rows_of[p] for p in u)
        if cur and n + r > max_rows:
            out.append(cur)
            cur, n = [], 0
        cur.append(u)
        n += r
    if cur:
        out.append(cur)
    return out


def _directed_jobs(pairs, T, lens, symmetric, T_back=None):
    """The searches of a list of pairs: job (moving, fixed, T) = pair p with ``T[p]`` and, when ``symmetric``, the
    reverse direction right behind it with ``T_back[p]`` (default ``inv(T[p])``).  Returns ``(job_pairs int64 [J,2],
    job_T f64 [J,4,4], units, rows_of)``: ``units[p]`` lists the job numbers of pair p, forward first, and
    ``rows_of[j]`` is the length of job j's moving cloud."""
    job_pairs, job_T, units = [], [], []
    for p in range(len(pairs)):
        unit = [len(job_pairs)]
        job_pairs.append(pairs[p])
        job_T.append(T[p])
        if symmetric:
            unit.append(len(job_pairs))
            job_pairs.append(pairs[p, ::-1])
            job_T.append(np.linalg.inv(T[p]) if T_back is None else T_back[p])
        units.append(unit)
    job_pairs = np.asarray(job_pairs, dtype=np.int64).reshape(-1, 2)
    return job_pairs, np.asarray(job_T, dtype=np.float64).reshape(-1, 4, 4), units, lens[job_pairs[:, 0]]


def _by_fixed_cloud(units, job_pairs):
    """The units ordered by the fixed cloud of their first job: searches of one fixed cloud next to each other, so that
    the workgroups in flight together read the same part of the cell list."""
    return sorted(units, key=lambda u: (int(job_pairs[u[0], 1]), u[0]))


def _mine(clouds, pairs, transforms, radius, min_overlap, symmetric, device, max_rows):
    """{(i, j): int64 [M,2]} and {(i, j): overlap} for the explicit ``pairs`` with ``transforms`` source -> target."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    T = np.asarray(transforms, dtype=np.float64).reshape(-1, 4, 4) if len(pairs) else np.zeros((0, 4, 4))
    if T.shape[0] != pairs.shape[0]:
        raise ValueError("%d transforms for %d pairs" % (T.shape[0], pairs.shape[0]))
    if pairs.size and (pairs.min() < 0 or pairs.max() >= len(clouds)):
        raise ValueError("pairs name fragments outside 0..%d" % (len(clouds) - 1))
    if len(set(map(tuple, pairs.tolist()))) != pairs.shape[0]:
        raise ValueError("a pair is listed twice")
    lens = np.array([c.shape[0] for c in clouds], dtype=np.int64)
    job_pairs, job_T, units, rows_of = _directed_jobs(pairs, T, lens, symmetric)
    units = _by_fixed_cloud(units, job_pairs)
    corr, overlap = {}, {}
    on_cpu = str(device).startswith('cpu')
    if not on_cpu and pairs.shape[0]:
        import torch
        from .. import ops
        dev = torch.device(device)
        grid = ops.CloudGrid(torch.as_tensor(np.concatenate(clouds, 0) if lens.sum() else np.zeros((1, 3), np.float32))
                             .to(dev), lens.astype(np.int32), radius)
    for chunk in _chunks(units, rows_of, int(max_rows)):
        jobs = [j for u in chunk for j in u]
        jp, jt = job_pairs[jobs], job_T[jobs]
        if on_cpu:
            nn, count, row_start = nearest_pairs_numpy(clouds, jp, jt, radius)
        else:
            nn, count_d, row_start_d = ops.nearest_pairs(grid, None, jp, jt, radius)
            count, row_start = count_d.cpu().numpy(), row_start_d.cpu().numpy()   # (the chunk's one wait for the device)
        ratio = count / np.maximum(rows_of[jobs], 1)
        local = {j: k for k, j in enumerate(jobs)}
        kept = []                                          # chunk-local numbers of the forward jobs whose lists are kept
        for u in chunk:
            key = (int(job_pairs[u[0], 0]), int(job_pairs[u[0], 1]))
            overlap[key] = float(max(ratio[local[j]] for j in u))
            if overlap[key] > min_overlap and count[local[u[0]]] > 0:
                kept.append(local[u[0]])
        if not kept:
            continue
        if on_cpu:
            for k in kept:
                seg = nn[row_start[k]:row_start[k + 1]]
                src = np.nonzero(seg >= 0)[0]
                corr[(int(jp[k, 0]), int(jp[k, 1]))] = np.stack([src, seg[src]], 1).astype(np.int64)
        else:
            # compaction on the device; only the kept pairs' lists travel
            keep = torch.zeros(len(jobs), dtype=torch.bool, device=dev)
            keep[torch.as_tensor(kept, device=dev)] = True
            job_of_row = torch.repeat_interleave(torch.arange(len(jobs), device=dev),
                                                 torch.as_tensor(rows_of[jobs], device=dev))
            sel = torch.nonzero((nn >= 0) & keep[job_of_row]).squeeze(1)
            src = (sel - row_start_d[job_of_row[sel]]).cpu().numpy()
            tgt = nn[sel].cpu().numpy().astype(np.int64)
            kept.sort()                                     # the selected rows ascend: kept jobs in chunk order
            for k, e in zip(kept, np.cumsum(count[kept])):
                n = int(count[k])
                corr[(int(jp[k, 0]), int(jp[k, 1]))] = np.stack([src[e - n:e], tgt[e - n:e]], 1).astype(np.int64)
    if not on_cpu and pairs.shape[0]:
        grid.status.raise_if_set()
    order = {tuple(p): k for k, p in enumerate(pairs.tolist())}
    corr = {k: corr[k] for k in sorted(corr, key=order.get)}      # in the order the pairs were given
    return corr, overlap


def mine_pairs(fragments, pairs, transforms, voxel=None, radius=None, min_overlap=0.3, symmetric=False, device='cuda',
               max_rows=DEFAULT_MAX_ROWS, subsample=None, return_overlap=False):
    """Explicit pairs: ``pairs`` [P,2] (source, target) fragment numbers and ``transforms`` [P,4,4] f64 mapping source
    points into the target's frame.  (A ``gt.log`` entry ``i_j`` of ``geometric_registration.evaluate.loadlog`` maps j
    into i: pass it as pair (j, i).)  Returns ``(clouds, {(i, j): int64 [M,2]})``, rows ascending in the source index;
    ``return_overlap=True`` appends ``{(i, j): overlap}`` for every pair looked at."""
    if radius is None:
        if voxel is None:
            raise ValueError("radius is required when voxel is None")
        radius = 1.25 * voxel
    clouds = subsample_fragments(fragments, voxel, subsample, device)
    corr, overlap = _mine(clouds, pairs, transforms, float(radius), float(min_overlap), symmetric, device, max_rows)
    return (clouds, corr, overlap) if return_overlap else (clouds, corr)


def _box_gap(lo_a, hi_a, lo_b, hi_b):
    return float(np.sqrt((np.maximum(0.0, np.maximum(lo_a - hi_b, lo_b - hi_a)) ** 2).sum()))


def candidate_pairs(clouds, poses, radius, prefilter=True):
    """Pairs i < j whose world-frame bounding boxes are not farther apart than ``radius`` (those cannot overlap), and
    ``T_ij = inv(P_j) @ P_i``.  The margin covers the f32 rounding of the moved points."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    boxes = []
    for c, P in zip(clouds, poses):
        if c.shape[0] == 0:
            boxes.append(None)
            continue
        w = c.astype(np.float64) @ P[:3, :3].T + P[:3, 3]
        boxes.append((w.min(0), w.max(0)))
    pairs, T = [], []
    for i in range(len(clouds)):
        for j in range(i + 1, len(clouds)):
            if boxes[i] is None or boxes[j] is None:
                continue
            if prefilter:
                scale = max(np.abs(boxes[i][0]).max(), np.abs(boxes[i][1]).max(), np.abs(boxes[j][0]).max(),
                            np.abs(boxes[j][1]).max(), 1.0)
                if _box_gap(*boxes[i], *boxes[j]) > radius * 1.001 + 1e-5 * scale:
                    continue
            pairs.append((i, j))
            T.append(np.linalg.inv(poses[j]) @ poses[i])
    return np.asarray(pairs, dtype=np.int64).reshape(-1, 2), np.asarray(T, dtype=np.float64).reshape(-1, 4, 4)


def mine_scene(fragments, poses, voxel, radius=None, min_overlap=0.3, symmetric=False, device='cuda',
               max_rows=DEFAULT_MAX_ROWS, subsample=None, prefilter=True, return_overlap=False):
    """One scene: ``fragments`` a list of [N_i,3] arrays in their own frames, ``poses`` [F,4,4] f64 fragment-to-world.
    All pairs i < j are candidates.  Overlap of (i, j) is ``count / N_i``; with ``symmetric=True`` the direction j -> i is
    mined too and the larger ratio decides (the stored list is still the i -> j one).  Returns the subsampled clouds and
    ``{(i, j): int64 [M,2]}`` for the kept pairs."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    if poses.shape[0] != len(fragments):
        raise ValueError("%d poses for %d fragments" % (poses.shape[0], len(fragments)))
    if radius is None:
        if voxel is None:
            raise ValueError("radius is required when voxel is None")
        radius = 1.25 * voxel
    clouds = subsample_fragments(fragments, voxel, subsample, device)
    pairs, T = candidate_pairs(clouds, poses, float(radius), prefilter)
    corr, overlap = _mine(clouds, pairs, T, float(radius), float(min_overlap), symmetric, device, max_rows)
    return (clouds, corr, overlap) if return_overlap else (clouds, corr)


# ------------------------------------------------------------------------------------------------------ files
def read_pose(filename):
    """4x4 f64 fragment-to-world pose of a ``cloud_bin_<i>.info.txt``: one header line, then the matrix."""
    m = np.loadtxt(filename, skiprows=1, dtype=np.float64)
    if m.shape != (4, 4):
        raise ValueError("%s: expected a header line and a 4x4 matrix" % filename)
    return m


def read_scene(root, scene):
    """(fragment ids, [N,3] f64 points per fragment, poses [F,4,4]) of ``<root>/fragments/<scene>``: the fragments are
    ``cloud_bin_<i>.ply`` in the order of i, the poses come from ``poses.npy`` when the folder has one, else from the
    ``cloud_bin_<i>.info.txt`` files."""
    path = join(root, 'fragments', scene)
    names = sorted((f for f in os.listdir(path) if re.fullmatch(r'cloud_bin_\d+\.ply', f)),
                   key=lambda x: int(x[:-4].split('_')[-1]))
    ids = ['%s/%s' % (scene, n[:-4]) for n in names]
    points = [read_ply_points(join(path, n)) for n in names]
    if exists(join(path, 'poses.npy')):
        poses = np.load(join(path, 'poses.npy')).astype(np.float64).reshape(-1, 4, 4)
        if poses.shape[0] != len(names):
            raise ValueError("%s: poses.npy holds %d poses for %d fragments" % (path, poses.shape[0], len(names)))
    else:
        poses = np.stack([read_pose(join(path, n[:-4] + '.info.txt')) for n in names]) if names else np.zeros((0, 4, 4))
    return ids, points, poses


def pickle_names(out_dir, split, downsample):
    return (join(out_dir, '3DMatch_%s_%.3f_points.pkl' % (split, downsample)),
            join(out_dir, '3DMatch_%s_%.3f_keypts.pkl' % (split, downsample)))


def build_pickles(root, split, scenes, voxel, out_dir=None, downsample=None, radius=None, min_overlap=0.3,
                  symmetric=False, device='cuda', max_rows=DEFAULT_MAX_ROWS, subsample=None):
    """Writes ``3DMatch_<split>_<downsample:.3f>_points.pkl`` ({"<scene>/cloud_bin_<i>": float32 [N,3]}, each fragment
    in its OWN frame: the poses serve the mining only) and ``..._keypts.pkl`` ({"<src id>@<tgt id>": int64 [M,2]}) under
    ``out_dir`` (default ``root``) from ``<root>/fragments/<scene>/``.  ``downsample`` is the value in the file names
    (default ``voxel``; required with ``voxel=None``, which takes the PLY clouds as they are).  Returns the two paths."""
    downsample = voxel if downsample is None else downsample
    if downsample is None:
        raise ValueError("voxel=None needs downsample= for the file names")
    radius = 1.25 * downsample if radius is None else radius
    points, keypts, too_large = {}, {}, 0
    for scene in scenes:
        ids, raw, poses = read_scene(root, scene)
        clouds, corr = mine_scene(raw, poses, voxel, radius=radius, min_overlap=min_overlap, symmetric=symmetric,
                                  device=device, max_rows=max_rows, subsample=subsample)
        for ident, cloud in zip(ids, clouds):
            points[ident] = cloud
            too_large += cloud.shape[0] > ThreeDMatchDataset.MAX_POINTS
        for (i, j), c in corr.items():
            keypts['%s@%s' % (ids[i], ids[j])] = c
    if too_large:
        warnings.warn("%d fragments hold more than %d points: ThreeDMatchDataset skips them"
                      % (too_large, ThreeDMatchDataset.MAX_POINTS))
    out_dir = root if out_dir is None else out_dir
    os.makedirs(out_dir, exist_ok=True)
    pts_file, key_file = pickle_names(out_dir, split, downsample)
    with open(pts_file, 'wb') as f:
        pickle.dump(points, f)
    with open(key_file, 'wb') as f:
        pickle.dump(keypts, f)
    return pts_file, key_file
