"""3DMatch registration protocol around the matching kernel -- the reference's ``test.py`` (:20-128) re-cast for the GPU.

Same on-disk contract as the reference, so either side can read the other's dumps:

* ``generate_features``   (test.py:79-128): per fragment ``descriptors/<scene>/cloud_bin_<i>.D3Feat.npy`` [N,32] f32,
  ``keypoints/<scene>/cloud_bin_<i>.npy`` [N,3] f32, ``scores/<scene>/cloud_bin_<i>.npy`` [N,1] f32, eval mode
  (scores gated by the local-maximum mask).  The reference pushes a fragment through the network stacked with itself
  (datasets/ThreeDMatch.py:203 returns ``(pts, pts, ...)``) and keeps the first half (test.py:118-120); one copy gives
  the same rows (see ``describe_fragment``), so that is what runs.
* ``loadlog`` / ``writelog`` (geometric_registration/common.py:44-58): the ``gt.log`` trajectory format -- a
  ``id1 \\t id2 \\t n`` line followed by the 4x4 transform, tab separated.
* ``register_one_scene``  (test.py:20-76): for every fragment pair listed in ``gt.log``: top-k keypoints by score (or a
  random draw), mutual nearest neighbors in descriptor space, target keypoints moved by the ground-truth transform,
  inliers = matches closer than ``distance_threshold``; a pair is registered when its inlier ratio exceeds
  ``inlier_ratio_threshold``.  Returns ``(recall %, mean inlier count, mean inlier ratio)``.

Matching and inlier counting stay on the device (``ops.mutual_nn`` = the MFMA N x N kernel); per scene ONE read-back
of the per-pair counters.  The reference loops over pairs in NumPy/Open3D and one process per scene.
"""
import os

import numpy as np
import torch

from .. import ops
from ..datasets import dataloader as dl
from .common import select_keypoints

DESC_NAME = 'D3Feat'


# ------------------------------------------------------------------------------------------------- file formats
def loadlog(gtpath):
    """{'i_j': 4x4 float64} from ``<gtpath>/gt.log`` (common.py:44-58)."""
    with open(os.path.join(gtpath, 'gt.log')) as f:
        rows = [ln.rstrip('\n') for ln in f if ln.strip()]
    if len(rows) % 5:
        raise ValueError("gt.log: %d non-empty lines, expected blocks of 5" % len(rows))
    out = {}
    for i in range(0, len(rows), 5):
        head = rows[i].split('\t')[0:3]
        mat = np.array([[float(x) for x in rows[i + r].split('\t')[0:4]] for r in range(1, 5)], dtype=np.float64)
        out['%d_%d' % (int(head[0]), int(head[1]))] = mat
    return out


def writelog(gtpath, transforms, num_frag):
    """Inverse of :func:`loadlog` (used for synthetic scenes; the benchmark ships its own files)."""
    os.makedirs(gtpath, exist_ok=True)
    with open(os.path.join(gtpath, 'gt.log'), 'w') as f:
        for key in sorted(transforms, key=lambda k: tuple(int(x) for x in k.split('_'))):
            a, b = key.split('_')
            f.write('%d\t %d\t %d\t\n' % (int(a), int(b), num_frag))
            for row in np.asarray(transforms[key], dtype=np.float64):
                f.write(''.join(' % .8e\t ' % v for v in row).rstrip(' ') + '\n')


def _paths(save_path, scene):
    return (os.path.join(save_path, 'descriptors', scene), os.path.join(save_path, 'keypoints', scene),
            os.path.join(save_path, 'scores', scene))


def get_keypts(keyptspath, filename):
    return np.load(os.path.join(keyptspath, filename + '.npy'))


def get_desc(descpath, filename, desc_name=DESC_NAME):
    return np.load(os.path.join(descpath, filename + '.%s.npy' % desc_name))


def get_scores(scorepath, filename, desc_name=DESC_NAME):
    return np.load(os.path.join(scorepath, filename + '.npy'))


# ------------------------------------------------------------------------------------------ descriptor generation
@torch.no_grad()
def describe_fragment(model, points, config, neighborhood_limits, device=None, stacked=False, exact_width=True):
    """(keypoints [N,3], descriptors [N,32], scores [N,1]) of one fragment, device tensors (test.py:107-120).

    The reference feeds the fragment stacked with itself and keeps the first half.  Every operator of the network
    works per cloud (neighbor tables never cross clouds) and the detector's global maximum over two copies equals the
    maximum over one, so a single copy gives the same rows for half the work; ``stacked=True`` runs the literal
    two-copy batch (used by the test that checks the equivalence).  ``exact_width=False`` keeps every neighbor table at
    the full calibrated width instead of the reference's min(limit, max_count) -- what the static-shape graph engine
    (``infer.InferStep``) does; see the note on table widths in DESIGN.md section 3."""
    dev = torch.device(device) if device is not None else next(model.parameters()).device
    pts = torch.as_tensor(np.ascontiguousarray(points) if isinstance(points, np.ndarray) else points,
                          dtype=torch.float32, device=dev)
    n = int(pts.shape[0])
    feat = torch.ones((n, 1), dtype=torch.float32, device=dev)
    if stacked:
        empty = torch.zeros((0, 2), dtype=torch.int64, device=dev)
        batch = dl.collate_fn_descriptor([(pts, pts, feat, feat, empty, torch.zeros((0, 0), device=dev))], config,
                                         neighborhood_limits, device=dev)
    else:
        lengths = torch.tensor([n], dtype=torch.int32, device=dev)
        batch = dl.build_pyramid(pts, lengths, config, neighborhood_limits, exact_width=exact_width)
        batch.pop('_status')
        batch['features'] = feat
    was_training = model.training
    model.eval()
    try:
        features, scores = model(batch)
    finally:
        model.train(was_training)
    return batch['points'][0][:n], features[:n], scores[:n]


def generate_features(model, scenes, save_path, config, neighborhood_limits, device=None, verbose=False, engine=None):
    """``scenes``: {scene name: sequence of fragment point arrays [N,3]} (already voxel-subsampled at
    ``config.downsample`` like ThreeDMatchTestset does).  Writes the three .npy files per fragment.

    ``engine``: an ``infer.InferStep(model, ..., clouds=1)`` with graphs enabled -- fragments that fit its capacities
    go through the pipelined graph replay (the next fragment's pyramid is built under the current one's network),
    the others through the eager ``describe_fragment``."""
    for scene, fragments in scenes.items():
        dpath, kpath, spath = _paths(save_path, scene)
        for p in (dpath, kpath, spath):
            os.makedirs(p, exist_ok=True)
        frags = [np.ascontiguousarray(f, dtype=np.float32) for f in fragments]
        dev = torch.device(device) if device is not None else next(model.parameters()).device
        on_dev = [torch.from_numpy(f).to(dev) for f in frags] if engine is not None else None
        for ids, points in enumerate(frags):
            if engine is not None and engine.fits((on_dev[ids],)):
                nxt = (on_dev[ids + 1],) if ids + 1 < len(frags) and engine.fits((on_dev[ids + 1],)) else None
                features, scores = engine.describe((on_dev[ids],), nxt)
                pts = on_dev[ids]
            else:
                pts, features, scores = describe_fragment(model, points, config, neighborhood_limits, device)
            np.save(os.path.join(dpath, 'cloud_bin_%d.%s' % (ids, DESC_NAME)), features.cpu().numpy().astype(np.float32))
            np.save(os.path.join(kpath, 'cloud_bin_%d' % ids), pts.cpu().numpy().astype(np.float32))
            np.save(os.path.join(spath, 'cloud_bin_%d' % ids), scores.cpu().numpy().astype(np.float32))
            if verbose:
                print("Generate cloud_bin_%d for %s" % (ids, scene))
        if engine is not None:
            engine.check_status()


def generate_fpfh_features(scenes, save_path, radius, normal_radius=None, seed=0, desc_name='FPFH', device='cuda',
                           detector=None, iss=None):
    """``generate_features`` without a network: FPFH descriptors (``registration.describe_fpfh``: one cell list, one
    normals call and one ``ops.fpfh`` call per scene) in the same layout -- per fragment
    ``descriptors/<scene>/cloud_bin_<i>.<desc_name>.npy`` [N,64] f32 (33 columns scaled to unit rows and zero-padded: the
    norm and the width the matching kernel reads), ``keypoints/<scene>/cloud_bin_<i>.npy`` [N,3] f32 (the whole
    fragment, as the ICP path relies on) and
    ``scores/<scene>/cloud_bin_<i>.npy`` [N,1] f32.  FPFH has no detector: the score is a uniform draw in (0, 1] from
    ``numpy.random.default_rng(seed)`` for a point with a descriptor and 0 for one without, so the top-k selection of
    ``register_one_scene`` / ``registration.register_scene`` (with ``desc_name=``) is a reproducible uniform sample of
    the described points.  ``device='cpu'`` runs the NumPy restatement.

    ``detector='iss'`` with ``iss=dict(salient_radius=..., non_max_radius=...)`` (further keywords of
    ``registration.detect_iss``: the gammas, ``min_neighbors``) pairs FPFH with the ISS detector, as the published FPFH
    baselines do: the score is the ISS saliency for a point that survives the suppression AND has a descriptor, and 0
    for every other point; ``seed`` is not used.  Anything else than None / ``'iss'`` raises ``ValueError``."""
    from . import registration as reg
    if detector not in (None, 'iss') or (detector is None) != (iss is None):
        raise ValueError("detector must be None, or 'iss' with iss=dict(salient_radius=..., non_max_radius=...)")
    if detector == 'iss' and not (isinstance(iss, dict) and {'salient_radius', 'non_max_radius'} <= set(iss)):
        raise ValueError("iss must be a dict of detect_iss keywords with at least salient_radius and non_max_radius")
    rng = np.random.default_rng(seed)
    for scene, fragments in scenes.items():
        dpath, kpath, spath = _paths(save_path, scene)
        for p in (dpath, kpath, spath):
            os.makedirs(p, exist_ok=True)
        frags = [np.ascontiguousarray(f, dtype=np.float32).reshape(-1, 3) for f in fragments]
        descs, counts = reg.describe_fpfh(frags, radius, normal_radius, device=device)
        if detector == 'iss':
            saliency, kept = reg.detect_iss(frags, device=device, **iss)
        for ids, points in enumerate(frags):
            desc, count = descs[ids], counts[ids]
            if isinstance(desc, torch.Tensor):
                desc, count = desc.cpu().numpy(), count.cpu().numpy()
            if detector == 'iss':
                sal, rows = saliency[ids], kept[ids]
                if isinstance(sal, torch.Tensor):
                    sal, rows = sal.cpu().numpy(), rows.cpu().numpy()
                draw = np.zeros(points.shape[0], dtype=np.float32)
                draw[rows] = sal[rows]
            else:
                draw = 1.0 - rng.random(points.shape[0])                   # (0, 1]
            scores = np.where(count > 0, draw, 0.0).astype(np.float32).reshape(-1, 1)
            np.save(os.path.join(dpath, 'cloud_bin_%d.%s' % (ids, desc_name)), desc.astype(np.float32))
            np.save(os.path.join(kpath, 'cloud_bin_%d' % ids), points)
            np.save(os.path.join(spath, 'cloud_bin_%d' % ids), scores)


# ----------------------------------------------------------------------------------------------------- registration
def match_pair(source_keypts, source_desc, source_score, target_keypts, target_desc, target_score, gt_trans,
               num_points=250, distance_threshold=0.10, random_points=False, rng=None):
    """Device tensors in; returns device scalars ``(num_inliers, num_matches)`` of one fragment pair
    (test.py:47-70).  ``gt_trans`` maps the target fragment into the source frame."""
    if random_points:
        rng = rng if rng is not None else np.random
        si = torch.as_tensor(rng.choice(source_keypts.shape[0], num_points), device=source_desc.device)
        ti = torch.as_tensor(rng.choice(target_keypts.shape[0], num_points), device=source_desc.device)
    else:
        si = select_keypoints(source_score.reshape(-1), num_points)
        ti = select_keypoints(target_score.reshape(-1), num_points)
    sd = torch.nan_to_num(source_desc[si]).contiguous()
    td = torch.nan_to_num(target_desc[ti]).contiguous()
    row, _, mutual = ops.mutual_nn(sd, td)
    T = torch.as_tensor(gt_trans, dtype=torch.float64, device=sd.device)
    tgt = target_keypts[ti][row.long()].double() @ T[:3, :3].T + T[:3, 3]     # every source row's match, moved
    dist = torch.sqrt(((source_keypts[si].double() - tgt) ** 2).sum(dim=1))
    keep = mutual.bool()
    return ((dist < distance_threshold) & keep).sum(), keep.sum()


def register_one_scene(inlier_ratio_threshold, distance_threshold, save_path, scene, gtpath, num_frag=None,
                       num_points=250, random_points=False, device='cuda', seed=0, desc_name=DESC_NAME):
    """Recall / mean inlier count / mean inlier ratio of one scene from the dumped files (test.py:20-76).
    ``desc_name``: the descriptor whose dump is read (``'FPFH'``: ``generate_fpfh_features``)."""
    gt = loadlog(gtpath)
    dpath, kpath, spath = _paths(save_path, scene)
    if num_frag is None:
        num_frag = len([f for f in os.listdir(kpath) if f.endswith('.npy')])
    dev = torch.device(device)
    cache = {}

    def load(i):
        if i not in cache:
            name = 'cloud_bin_%d' % i
            cache[i] = tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in (
                get_keypts(kpath, name), get_desc(dpath, name, desc_name), get_scores(spath, name).reshape(-1)))
        return cache[i]
    rng = np.random.RandomState(seed)
    counts = []
    for id1 in range(num_frag):
        for id2 in range(id1 + 1, num_frag):
            key = '%d_%d' % (id1, id2)
            if key not in gt:   # pairs with less than 30% overlap are not part of the benchmark (test.py:38-42)
                continue
            sk, sd, ss = load(id1)
            tk, td, ts = load(id2)
            counts.append(torch.stack(match_pair(sk, sd, ss, tk, td, ts, gt[key], num_points, distance_threshold,
                                                 random_points, rng)))
    if not counts:
        raise ValueError("no fragment pair of %s is listed in %s" % (scene, os.path.join(gtpath, 'gt.log')))
    c = torch.stack(counts).cpu().numpy().astype(np.float64)      # the scene's only read-back
    inliers, matches = c[:, 0], c[:, 1]
    ratio = np.divide(inliers, matches, out=np.zeros_like(inliers), where=matches > 0)
    recall = float((ratio > inlier_ratio_threshold).sum()) * 100.0 / len(ratio)
    return recall, float(inliers.mean()), float(ratio.mean())


def evaluate_scenes(save_path, scenes_gt, inlier_ratio_threshold=0.05, distance_threshold=0.10, num_points=250,
                    random_points=False, device='cuda', desc_name=DESC_NAME):
    """{scene: gt directory} -> ({scene: [recall, inlier num, inlier ratio]}, averages) -- test.py:169-188."""
    out = {}
    for scene, gtpath in scenes_gt.items():
        out[scene] = list(register_one_scene(inlier_ratio_threshold, distance_threshold, save_path, scene, gtpath,
                                             num_points=num_points, random_points=random_points, device=device,
                                             desc_name=desc_name))
    avg = np.mean(np.array(list(out.values()), dtype=np.float64), axis=0)
    return out, {'recall': float(avg[0]), 'inlier_num': float(avg[1]), 'inlier_ratio': float(avg[2])}


# ---------------------------------------------------------------------------------------------------- repeatability
def repeatability_scene(save_path, scene, gtpath, num_points=(4, 8, 16, 32, 64, 128, 256, 512), distance=0.1,
                        nms_radius=None, device='cuda'):
    """Keypoint repeatability of one scene from the dumped keypoints and scores of any ``generate_*`` and the scene's
    ``gt.log`` (``registration.keypoint_repeatability`` has the convention).  For every k of ``num_points`` each
    fragment's keypoints are its ``select_keypoints`` top-k among the rows with a POSITIVE score -- a zero score is never
    a keypoint, so a fragment with fewer such rows gives what it has.  ``nms_radius``: the scores first go through
    ``registration.suppress_non_maxima`` at that radius (a suppressed row's score becomes 0).  One
    ``keypoint_repeatability`` call per k.  Returns ``({k: relative repeatability}, {k: int64 [num_frag] keypoints per
    fragment})``."""
    from . import registration as reg
    gt = loadlog(gtpath)
    _, kpath, spath = _paths(save_path, scene)
    num_frag = len([f for f in os.listdir(kpath) if f.endswith('.npy')])
    names = ['cloud_bin_%d' % i for i in range(num_frag)]
    keypts = [np.ascontiguousarray(get_keypts(kpath, n), dtype=np.float32).reshape(-1, 3) for n in names]
    scores = [np.ascontiguousarray(get_scores(spath, n), dtype=np.float32).reshape(-1) for n in names]
    if nms_radius is not None:
        masks = reg.suppress_non_maxima(keypts, scores, nms_radius, device=device)
        scores = [np.where(m.cpu().numpy() if isinstance(m, torch.Tensor) else m, s, np.float32(0.0))
                  for m, s in zip(masks, scores)]
    keys = sorted(gt, key=lambda k: tuple(int(x) for x in k.split('_')))
    if not keys:
        raise ValueError("no fragment pair is listed in %s" % os.path.join(gtpath, 'gt.log'))
    T = np.stack([gt[k] for k in keys])
    with np.errstate(invalid='ignore'):
        positive = [np.nonzero(s > 0)[0] for s in scores]
    rep, counts = {}, {}
    for k in num_points:
        sets = [p[rows[select_keypoints(torch.from_numpy(s[rows]), k).numpy()]]
                for p, s, rows in zip(keypts, scores, positive)]
        rep[int(k)] = reg.keypoint_repeatability(sets, keys, T, distance=distance, device=device)[4]
        counts[int(k)] = np.asarray([len(s) for s in sets], dtype=np.int64)
    return rep, counts


def repeatability_scenes(save_path, scenes_gt, num_points=(4, 8, 16, 32, 64, 128, 256, 512), distance=0.1,
                         nms_radius=None, device='cuda'):
    """{scene: gt directory} -> ({scene: {k: relative repeatability}}, {k: the mean over the scenes}), averaged over
    scenes the way ``evaluate_scenes`` averages recall."""
    out = {scene: repeatability_scene(save_path, scene, gtpath, num_points, distance, nms_radius, device)[0]
           for scene, gtpath in scenes_gt.items()}
    return out, {int(k): float(np.mean([r[int(k)] for r in out.values()])) for k in num_points}
