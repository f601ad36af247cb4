"""Rigid registration of fragment pairs and the 3DMatch registration recall -- the step after the correspondences.

The reference stops at the feature-match recall (``evaluate.register_one_scene``) and leaves pose estimation to Open3D
on the CPU.  Here it runs on the device: top-k keypoints by score, mutual nearest neighbours (``ops.mutual_nn``), then
RANSAC over the mutual matches of ALL pairs of a scene in one ``ops.ransac_rigid`` call (two launches) -- or, with
``estimator='fgr'``, fast global registration of the same matches in one ``ops.fgr_rigid`` call (one launch), or, with
``estimator='sc2'``, the spatial-compatibility estimator in one ``ops.sc2_rigid`` call (four launches, no sampling).

* ``estimate_transform``             one pair: keypoints / descriptors / scores -> (T, inliers, num_matches);
* ``estimate_transforms_from_match`` the batched inference path: ``infer.InferStep.match(item, feats, scores,
  num_points=k)`` output -> one transform per pair of the stacked item;
* ``fgr_numpy`` / ``fgr_multiplicities`` / ``fgr_draw``  the NumPy restatement of ``ops.fgr_rigid`` (csrc/fgr.hpp has
  the rule: tuple test, graduated non-convexity, Gauss-Newton on SE(3)) and of its tuple test and sampler;
  ``FGR_DEFAULTS`` are the parameters ``estimator='fgr'`` starts from;
* ``sc2_numpy`` / ``sc2_compatibility`` / ``sc2_pack_rows``  the NumPy restatement of ``ops.sc2_rigid`` (csrc/sc2.hpp
  has the rule: compatibility bits, degree seeds, second-order consensus sets) and of its bit matrix; ``SC2_DEFAULTS``
  are the parameters ``estimator='sc2'`` starts from;
* ``knn_match_numpy``  the NumPy restatement of ``ops.knn_match`` (csrc/knn_match.hpp has the rule: the k nearest
  target descriptors by rounded f32 distance, then index); ``matches=dict(k=K)`` / ``matches=dict(ratio=r)`` on
  ``estimate_transform`` / ``register_scene`` hand the estimator every keypoint's K nearest neighbours, or its nearest
  one where Lowe's ratio test holds, instead of the mutual ones;
* ``loadinfo`` / ``transformation_error`` / ``evaluate_registration``  the benchmark's ``gt.info`` files and its
  registration recall / precision (error p <= 0.2^2 under the 6x6 information matrix, pairs with j - i > 1);
* ``register_scene``                  every pair listed in ``gt.log`` from the dumped files, estimates written in the
  ``gt.log`` format (``evaluate.writelog``);
* ``refine_transforms`` / ``icp_numpy``  point-to-point ICP over the whole fragments after RANSAC (``ops.icp_rigid``, all
  pairs of a scene in one call) and its NumPy restatement -- ``estimate_transform`` / ``register_scene`` run it when
  given ``icp=dict(max_distance=...)``; ``estimation='point_to_plane'`` in that dict takes the point-to-plane form with
  normals from ``ops.estimate_normals`` (NumPy restatement: ``estimate_normals_numpy``), ``estimation='colored'``
  with ``colors=`` the coloured form (``ops.color_gradients``, ``ops.icp_rigid(color_field=)``; NumPy restatements:
  ``color_gradients_numpy``, ``icp_numpy(color_field=)``; ``intensity_of`` turns RGB into the intensity they take);
* ``information_matrices`` / ``information_from_moments`` / ``information_numpy`` / ``writeinfo``  the 6x6 information
  matrix of fragment pairs under given poses (``ops.pair_information``: one search, 20 raw moments per pair) -- the
  matrix ``gt.info`` holds and a pose graph takes per edge -- and the writer of ``gt.info``;
* ``build_benchmark`` / ``build_benchmark_files``  ``gt.log`` and ``gt.info`` of a scene from raw fragments with poses:
  what ``register_scene`` and ``evaluate_registration`` need to score registration recall on scenes of one's own;
* ``multiway_registration`` / ``spanning_tree_poses`` / ``pose_graph_numpy``  one consistent pose per fragment from the
  pair poses and their information matrices: robust pose-graph optimisation (``ops.pose_graph_optimize``, one launch)
  that prunes false loop closures, and its NumPy restatement -- ``register_scene`` runs it when given
  ``pose_graph=dict(max_distance=...)``;
* ``describe_fpfh`` / ``fpfh_numpy``  FPFH descriptors of fragments (``ops.fpfh``; csrc/fpfh.hpp has the rule) and their
  NumPy restatement: the training-free descriptor and the baseline column of the registration tables --
  ``evaluate.generate_fpfh_features`` dumps them and ``register_scene(desc_name='FPFH')`` reads them;
* ``detect_iss`` / ``suppress_non_maxima`` / ``iss_numpy`` / ``radius_nms_numpy``  ISS keypoints of fragments
  (``ops.iss_keypoints``; csrc/iss.hpp has the rule), radius non-maximum suppression of any score (``ops.radius_nms``)
  and their NumPy restatements; ``keypoint_repeatability`` the detector's metric over the pairs of a ``gt.log``.

Every transform maps the TARGET fragment into the SOURCE frame (src ~ R tgt + t), like ``gt.log``.  In ICP's terms the
target fragment j of a key ``i_j`` is the MOVING cloud and the source fragment i the FIXED one: ``ops.icp_rigid`` takes
``pairs = (j, i)`` with the ``gt.log`` matrix as it stands.
"""
import os

import numpy as np
import torch

from .. import ops
from . import evaluate as ev
from .common import select_keypoints

RANSAC_DEFAULTS = dict(num_hypotheses=50000, distance_threshold=0.05, edge_ratio=0.9, refine_iters=3, seed=0)
FGR_DEFAULTS = dict(distance_threshold=0.05, iterations=128, division_factor=1.4, anneal_every=4, tuple_scale=0.95,
                    tuple_trials=None, max_tuples=1000, seed=0)
FGR_ST_FEW, FGR_ST_SINGULAR, FGR_ST_SEGMENT, FGR_ST_NONFINITE = 1, 2, 4, 8                          # ops.FGR_ST_*
SC2_DEFAULTS = dict(distance_threshold=0.05, compat_threshold=0.1, num_seeds=256, set_size=20, refine_iters=3)
SC2_ST_FEW, SC2_ST_NO_HYPOTHESIS, SC2_ST_SEGMENT = 1, 2, 4                                          # ops.SC2_ST_*
SC2_MAX_COUNT = 8192           # ops.SC2_MAX_COUNT
RANSAC_MAX_COUNT = 65536       # ops.RANSAC_MAX_COUNT
KNN_MAX = 8                    # ops.KNN_MAX
FGR_MAX_TRIALS = 1 << 22       # ops.FGR_MAX_TRIALS
RANSAC_MIN_CROSS2 = 1e-12      # csrc/rigid.hpp kMinCross2
ICP_ST_FEW, ICP_ST_CELL_RANGE, ICP_ST_PAIR, ICP_ST_NONFINITE, ICP_ST_SINGULAR = 1, 2, 4, 8, 16      # ops.ICP_ST_*
PG_ST_ITER_CAP, PG_ST_NONFINITE, PG_ST_GRAPH, PG_ST_INDEFINITE = 1, 2, 4, 8                         # ops.PG_ST_*
PG_LAMBDA0, PG_LAMBDA_MIN, PG_LAMBDA_MAX = 1e-4, 1e-12, 1e8    # csrc/posegraph.hpp kLambda0 / kLambdaMin / kLambdaMax
PLANE_PIVOT = 1e-10            # csrc/plane.hpp kPlanePivot
GRADIENT_PIVOT = 1e-6          # csrc/color_icp.hpp kGradientPivot
INTENSITY_SCALE = 2.0 ** 20    # csrc/color_icp.hpp kIntensityScale
LAMBDA_GEOMETRIC = 0.968       # Open3D's default weight of the geometric term; not tuned here


def _compact(mutual, src_pts, tgt_pts):
    """[P,k] mutual flags + [P,k,3] source / matched target points -> stacked (src [P*k,3], tgt [P*k,3], seg [P,2]):
    pair p's mutual rows first, in slot order, at offset p*k.  On the device, no host synchronisation."""
    P, k = int(mutual.shape[0]), int(mutual.shape[1])
    m = mutual.reshape(P, k).to(torch.int64)
    n = m.sum(dim=1)
    pos = torch.cumsum(m, dim=1) - 1 + torch.arange(P, device=m.device).view(P, 1) * k
    dst = torch.where(m.bool(), pos, torch.full_like(pos, P * k)).reshape(-1)      # the others go to a spill row
    src = torch.zeros((P * k + 1, 3), dtype=torch.float32, device=m.device)
    tgt = torch.zeros((P * k + 1, 3), dtype=torch.float32, device=m.device)
    src.index_put_((dst,), src_pts.reshape(-1, 3).float())
    tgt.index_put_((dst,), tgt_pts.reshape(-1, 3).float())
    seg = torch.stack([torch.arange(P, device=m.device) * k, n], dim=1).to(torch.int32).contiguous()
    return src[:P * k].contiguous(), tgt[:P * k].contiguous(), seg, n


def _ransac(src, tgt, seg, params):
    p = dict(RANSAC_DEFAULTS)
    p.update(params)
    return ops.ransac_rigid(src, tgt, seg, **p)


def knn_match_numpy(S, T, k, block=1024):
    """The rule of ``ops.knn_match`` (csrc/knn_match.hpp) in NumPy: (idx int32 [Ns,k], dist f32 [Ns,k]), ascending
    (float32 distance, column) with NaN distances first; slots beyond Nt hold -1 / +inf.  Never holds more than ``block``
    rows of the matrix.  The products are the float32 images of the float64 ones: THE products where they are exact
    (tests/knn_cases.py), else within a rounding of the kernel's."""
    S, T, k = np.ascontiguousarray(S, np.float32), np.ascontiguousarray(T, np.float32), int(k)
    if not 1 <= k <= KNN_MAX:
        raise ValueError("k must be in 1..%d" % KNN_MAX)
    idx = np.full((len(S), k), -1, np.int32)
    dist = np.full((len(S), k), np.inf, np.float32)
    m, T64 = min(k, len(T)), T.astype(np.float64).T
    for b in range(0, len(S), int(block)):
        a = (S[b:b + block].astype(np.float64) @ T64).astype(np.float32)
        with np.errstate(invalid='ignore'):
            d = np.sqrt(np.float32(2) - np.float32(2) * a)
        key = np.where(np.isnan(d), -np.inf, d)
        order = np.argsort(key, axis=1, kind='stable')[:, :m]
        idx[b:b + block, :m] = order
        dist[b:b + block, :m] = np.take_along_axis(d, order, 1)
    return idx, dist


def _check_matches(matches, estimator, num_points):
    """The ``matches=`` keyword, checked before any work: None for the mutual rule (``None`` / ``'mutual'``), else
    ``(K, ratio, mutual)`` -- ``dict(k=K)``: ratio None; ``dict(ratio=r)``: K = 1; ``dict(k=K, mutual=True)``: the K
    nearest, mutual ones only."""
    if matches is None or matches == 'mutual':
        return None
    if not isinstance(matches, dict) or not matches:
        raise ValueError("matches must be None, 'mutual', dict(k=K), dict(k=K, mutual=True) or dict(ratio=r), got %r"
                         % (matches,))
    unknown = sorted(set(matches) - {'k', 'ratio', 'mutual'})
    if unknown:
        raise ValueError("matches takes the keys 'k', 'ratio' and 'mutual', not %s" % unknown)
    K, ratio, mutual = matches.get('k', 1), matches.get('ratio'), matches.get('mutual', False)
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= K <= KNN_MAX:
        raise ValueError("matches: k must be an integer in 1..%d, got %r" % (KNN_MAX, K))
    if not isinstance(mutual, bool):
        raise ValueError("matches: mutual must be True or False, got %r" % (mutual,))
    if ratio is not None:
        if K > 1:
            raise ValueError("matches takes k > 1 or ratio, not both")
        if mutual:
            raise ValueError("matches: mutual is taken with k, not with ratio")
        if isinstance(ratio, bool) or not isinstance(ratio, (int, float, np.floating)) or not 0.0 < ratio <= 1.0:
            raise ValueError("matches: ratio must be in (0, 1], got %r" % (ratio,))
        ratio = float(ratio)
    limit = _MATCH_LIMITS[estimator]
    if limit is not None and int(num_points) * int(K) > limit:
        raise ValueError("num_points * k = %d * %d = %d correspondences per pair, estimator=%r takes %d at most"
                         % (int(num_points), K, int(num_points) * int(K), estimator, limit))
    return int(K), ratio, mutual


def _knn_flags(idx, dist, ratio):
    """The kept slots of a ``knn_match`` result, flat in slot order i K + s: every filled slot, or (``ratio``, from a
    k = 2 result) the nearest neighbour of the rows that pass Lowe's test in f32 -- false on NaN and without a second."""
    if ratio is None:
        return (idx >= 0).reshape(-1), idx.reshape(-1)
    r = torch.tensor(ratio, dtype=torch.float32, device=dist.device)
    return (idx[:, 1] >= 0) & (dist[:, 0] < r * dist[:, 1]), idx[:, 0]


def _pair_points(source_keypts, source_desc, source_score, target_keypts, target_desc, target_score, num_points,
                 matches=None):
    """[k] mutual flags and the [k,3] source keypoints with their matched target keypoints (match_pair's selection).
    ``matches`` = (K, ratio, mutual) of ``_check_matches``: [k K] flags and points, correspondence (i, s) at slot
    i K + s."""
    si = select_keypoints(source_score.reshape(-1), num_points)
    ti = select_keypoints(target_score.reshape(-1), num_points)
    sd = torch.nan_to_num(source_desc[si]).contiguous()
    td = torch.nan_to_num(target_desc[ti]).contiguous()
    if matches is not None:
        K, ratio, mutual = matches
        idx, dist = ops.knn_match(sd, td, 2 if ratio is not None else K)
        keep, col = _knn_flags(idx, dist, ratio)
        if mutual:                           # slot (i, s) stays when source i is the nearest of its s-th target
            back = ops.mutual_nn(sd, td)[1][col.clamp(min=0).long()]
            keep = keep & (back == torch.arange(int(sd.shape[0]), device=back.device).repeat_interleave(K))
        return keep, source_keypts[si].repeat_interleave(K, dim=0), target_keypts[ti][col.clamp(min=0).long()]
    row, _, mutual = ops.mutual_nn(sd, td)
    return mutual, source_keypts[si], target_keypts[ti][row.long()]


def estimate_transform(source_keypts, source_desc, source_score, target_keypts, target_desc, target_score,
                       num_points=5000, icp=None, estimator='ransac', fgr=None, sc2=None, matches=None, **ransac):
    """One fragment pair (device tensors): top-k keypoints by score, mutual nearest neighbours, RANSAC.  Returns device
    tensors ``(T [4,4] f64, inliers, num_matches)``; T maps the target into the source frame.  ``ransac``: keywords of
    ``ops.ransac_rigid`` (defaults: RANSAC_DEFAULTS).  ``estimator='fgr'`` hands the same matches to ``ops.fgr_rigid``
    instead, with ``fgr`` a dict of its keywords (defaults: FGR_DEFAULTS); no ``ransac`` keyword is taken then.
    ``estimator='sc2'`` hands them to ``ops.sc2_rigid``, with ``sc2`` a dict of its keywords (defaults: SC2_DEFAULTS;
    ``max_count`` is filled in from ``num_points``).
    ``matches``: None (or ``'mutual'``): the mutual nearest neighbours; ``dict(k=K)``, 1 <= K <= 8: every selected source
    keypoint with each of its K nearest target keypoints (``ops.knn_match``), K = 1 the plain nearest neighbour;
    ``dict(ratio=r)``, 0 < r <= 1: its nearest neighbour where Lowe's test ``dist_1 < r dist_2`` holds;
    ``dict(k=K, mutual=True)``: of the K nearest only those whose own nearest source keypoint it is (one more
    ``ops.mutual_nn`` call).  ``num_points * K`` beyond what the estimator takes raises ``ValueError``.
    ``icp``: None, or a dict of ``refine_transforms`` keywords (at least ``max_distance``): the estimated pose is then
    refined by ICP over ALL points of the two fragments."""
    _check_estimator(estimator, dict(fgr=fgr, sc2=sc2), ransac)
    matches = _check_matches(matches, estimator, num_points)
    mutual, sp, tp = _pair_points(source_keypts, source_desc, source_score, target_keypts, target_desc, target_score,
                                  num_points, matches)
    src, tgt, seg, n = _compact(mutual.view(1, -1), sp.unsqueeze(0), tp.unsqueeze(0))
    T, inl = _estimate(estimator, dict(fgr=fgr, sc2=sc2), src, tgt, seg, ransac, int(mutual.numel()))
    if icp is not None:
        T = refine_transforms([source_keypts, target_keypts], [(0, 1)], T, device=source_keypts.device,
                              **_icp_keywords(icp))[0]
    return T[0], inl[0], n[0]


def estimate_transforms_from_match(points, seg, row, mutual, sel, estimator='ransac', fgr=None, sc2=None, **ransac):
    """The batched path: ``row, mutual, sel = InferStep.match(item, feats, scores, num_points=k)`` with ``points`` the
    item's stacked level-0 points [rows,3] and ``seg`` = ``InferStep.segments(item)`` [2P,2] (clouds 2p, 2p+1 are the
    source and target of pair p).  The mutual rows of every pair are compacted on the device and ONE ``ransac_rigid``
    call estimates all P transforms (``estimator='fgr'``, ``fgr=dict(...)``: one ``fgr_rigid`` call; ``estimator='sc2'``,
    ``sc2=dict(...)``: one ``sc2_rigid`` call with ``max_count`` = k; as in ``estimate_transform``).  Returns device tensors ``(T [P,4,4] f64, inliers [P], num_matches [P])``.
    ``row`` / ``mutual`` may also be [P,k,K]: K candidate targets per source keypoint and the flags of the ones to keep
    (``idx, dist, sel = InferStep.match_knn(...)``, ``mutual`` = ``idx >= 0`` or any filter of one's own); correspondence
    (i, s) of a pair then sits at slot i K + s and the estimator is told ``max_count`` = k K."""
    _check_estimator(estimator, dict(fgr=fgr, sc2=sc2), ransac)
    if row.dim() == 3:
        if tuple(mutual.shape) != tuple(row.shape):
            raise ValueError("row and mutual must have one shape, got %s and %s" % (tuple(row.shape), tuple(mutual.shape)))
        return _transforms_from_knn(points, seg, row, mutual, sel, estimator, fgr, sc2, ransac)
    P, k =int(row.shape[0]), int(row.shape[1])
    pts = points if points.dtype == torch.float32 else points.float()
    off = seg[:, 0].long()
    live = (sel >= 0)
    n_live = live.sum(dim=1)                                                  # keypoints per cloud (the tail of sel)
    src_rows = off[0::2].view(P, 1) + sel[0::2].clamp(min=0).long()           # [P,k] stacked rows of the sources
    tslot = (k - n_live[1::2]).view(P, 1) + row.long().clamp(min=0)           # target slot of each source's match
    tslot = tslot.clamp(max=k - 1)
    tgt_rows = off[1::2].view(P, 1) + torch.gather(sel[1::2].long(), 1, tslot).clamp(min=0)
    m = mutual.bool() & live[0::2]
    src, tgt, sg, n = _compact(m, pts[src_rows.reshape(-1)].view(P, k, 3), pts[tgt_rows.reshape(-1)].view(P, k, 3))
    T, inl = _estimate(estimator, dict(fgr=fgr, sc2=sc2), src, tgt, sg, ransac, k)
    return T, inl, n


def _transforms_from_knn(points, seg, idx, keep, sel, estimator, fgr, sc2, ransac):
    """``estimate_transforms_from_match`` on [P,k,K] tables."""
    P, k, K = (int(n) for n in idx.shape)
    limit = _MATCH_LIMITS[estimator]
    if limit is not None and k * K > limit:
        raise ValueError("num_points * k = %d * %d = %d correspondences per pair, estimator=%r takes %d at most"
                         % (k, K, k * K, estimator, limit))
    pts = points if points.dtype == torch.float32 else points.float()
    off = seg[:, 0].long()
    live = (sel >= 0)
    n_live = live.sum(dim=1)
    src_rows = off[0::2].view(P, 1) + sel[0::2].clamp(min=0).long()                          # [P,k]
    tslot = ((k - n_live[1::2]).view(P, 1, 1) + idx.long().clamp(min=0)).clamp(max=k - 1)    # [P,k,K]
    tsel = torch.gather(sel[1::2].long(), 1, tslot.view(P, k * K)).clamp(min=0)
    tgt_rows = off[1::2].view(P, 1) + tsel                                                   # [P,k K]
    m = (keep.bool() & (idx >= 0) & live[0::2].view(P, k, 1)).view(P, k * K)
    sp = pts[src_rows.reshape(-1)].view(P, k, 1, 3).expand(P, k, K, 3).reshape(P, k * K, 3)
    src, tgt, sg, n = _compact(m, sp, pts[tgt_rows.reshape(-1)].view(P, k * K, 3))
    T, inl = _estimate(estimator, dict(fgr=fgr, sc2=sc2), src, tgt, sg, ransac, k * K)
    return T, inl, n


# ------------------------------------------------------------------------------------------------- fast global registration
def _splitmix64(x):
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over='ignore'):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def fgr_draw(seed, p, h, count):
    """[..., 3] indices that trial h of pair p draws from ``count`` correspondences: the hash of csrc/rigid.hpp."""
    key = _splitmix64(_splitmix64(np.uint64(int(seed) & 0xffffffffffffffff)) ^ np.uint64(p))
    h = np.asarray(h, dtype=np.uint64)
    out = []
    for k in range(3):
        z = _splitmix64(key ^ ((h << np.uint64(2)) | np.uint64(k)))
        with np.errstate(over='ignore'):
            out.append(((z >> np.uint64(32)) * np.uint64(count)) >> np.uint64(32))
    return np.stack(out, axis=-1).astype(np.int64)


def _fgr_triples_ok(s, g, scale):
    """[H,3,3] f64 source / target triples -> [H] bool: rigid::triple_ok in its own order of operations."""
    def cross2(p):
        u, v = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        x = u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1]
        y = u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2]
        z = u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]
        return (x * x + y * y) + z * z

    def dist2(a, b):
        d = a - b
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    with np.errstate(invalid='ignore'):
        ok = ~(cross2(s) < RANSAC_MIN_CROSS2) & ~(cross2(g) < RANSAC_MIN_CROSS2)
        r2 = scale * scale
        for i, j in ((0, 1), (1, 2), (2, 0)):
            la2, lb2 = dist2(s[:, i], s[:, j]), dist2(g[:, i], g[:, j])
            lo, hi = np.where(la2 < lb2, la2, lb2), np.where(la2 < lb2, lb2, la2)
            ok &= lo >= r2 * hi
    return ok


def fgr_multiplicities(src, tgt, seed, p, tuple_scale=0.95, tuple_trials=None, max_tuples=1000, chunk=1 << 16):
    """The tuple test of csrc/fgr.hpp on one pair's [n,3] f32 correspondences -> ``(m int32 [n], tuples)``."""
    n = int(src.shape[0])
    trials = min(100 * n, FGR_MAX_TRIALS) if tuple_trials is None else int(tuple_trials)
    if trials == 0:
        return np.ones(n, dtype=np.int32), 0
    m, taken = np.zeros(n, dtype=np.int64), 0
    s64, g64 = src.astype(np.float64), tgt.astype(np.float64)
    for base in range(0, trials, chunk):
        idx = fgr_draw(seed, p, np.arange(base, min(base + chunk, trials)), n)
        ok = (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2])
        ok &= _fgr_triples_ok(s64[idx], g64[idx], float(tuple_scale))
        good = idx[ok]
        if max_tuples > 0:
            good = good[:max_tuples - taken]
        m += np.bincount(good.reshape(-1), minlength=n)
        taken += len(good)
        if max_tuples > 0 and taken >= max_tuples:
            break
    return m.astype(np.int32), taken


def _inliers_f32(T, src, tgt, tau):
    """The count of ``_inlier_mask_f32``."""
    return int(_inlier_mask_f32(T, src, tgt, tau).sum())


def _inlier_mask_f32(T, src, tgt, tau):
    """rigid::inlier_f32 over [n,3] f32 rows under the f32 image of T -> [n] bool.  A f32 fmaf is taken as the f32 rounding of the
    f64 ``a * b + c`` (the product is exact in f64): equal to the true fmaf except on double-rounding ties."""
    f32, f64 = np.float32, np.float64
    rt = T[:3].astype(f32)
    fma = lambda a, b, c: (f64(a) * b.astype(f64) + c.astype(f64)).astype(f32)
    x, y, z = tgt[:, 0], tgt[:, 1], tgt[:, 2]
    e = []
    for a in range(3):
        inner = fma(rt[a, 2], z, np.full(len(tgt), rt[a, 3], dtype=f32))
        e.append(fma(rt[a, 0], x, fma(rt[a, 1], y, inner)) - src[:, a])
    d2 = (e[2].astype(f64) * e[2].astype(f64)
          + ((e[1].astype(f64) * e[1].astype(f64) + (e[0] * e[0]).astype(f64)).astype(f32)).astype(f64)).astype(f32)
    return d2 < f32(tau) * f32(tau)


def fgr_numpy(src, tgt, seg, distance_threshold=0.05, iterations=128, division_factor=1.4, anneal_every=4,
              tuple_scale=0.95, tuple_trials=None, max_tuples=1000, seed=0, first_pair=0, return_debug=False):
    """The rule of ``ops.fgr_rigid`` (csrc/fgr.hpp) restated in NumPy f64 -- the independent witness of the device code
    and its host twin, not a transliteration: explicit 3x6 Jacobians, ``np.sum`` / ``einsum`` in their own order, a
    general linear solve behind the kernel's pivot test.  ``src`` / ``tgt`` [rows,3] f32 and ``seg`` [P,2] are host
    arrays.  Returns arrays ``(T [P,4,4], inliers [P], tuples [P], weight_sum [P], status [P])`` and, with
    ``return_debug``, ``(multiplicity int32 [rows], trace [P, iterations, 8])`` as ``ops.fgr_rigid`` does."""
    src = np.ascontiguousarray(src, dtype=np.float32).reshape(-1, 3)
    tgt = np.ascontiguousarray(tgt, dtype=np.float32).reshape(-1, 3)
    seg = np.asarray(seg, dtype=np.int64).reshape(-1, 2)
    P, rows, K = seg.shape[0], src.shape[0], int(iterations)
    T = np.tile(np.eye(4), (P, 1, 1))
    inl, tup, st = (np.zeros(P, dtype=np.int32) for _ in range(3))
    wsum = np.zeros(P)
    mult = np.zeros(rows, dtype=np.int32)
    trace = np.full((P, K, 8), np.nan)
    delta2 = float(distance_threshold) * float(distance_threshold)
    for p, (off, n) in enumerate(seg):
        if off < 0 or n < 0 or n > ops.RANSAC_MAX_COUNT or off + n > rows:
            st[p] = FGR_ST_SEGMENT
            continue
        if n < 3:
            st[p] = FGR_ST_FEW
            continue
        a32, b32 = src[off:off + n], tgt[off:off + n]
        m, tup[p] = fgr_multiplicities(a32, b32, seed, first_pair + p, tuple_scale, tuple_trials, int(max_tuples))
        mult[off:off + n] = m
        live = m > 0
        if live.sum() < 3:
            st[p] |= FGR_ST_FEW
            continue
        a, b, w0 = a32[live].astype(np.float64), b32[live].astype(np.float64), m[live].astype(np.float64)
        with np.errstate(all='ignore'):
            ca, cb = a.mean(0), b.mean(0)
            a, b = a - ca, b - cb
            mu = max(float((a * a).sum(1).max()), float((b * b).sum(1).max()))
        if not (np.isfinite(a).all() and np.isfinite(b).all()):
            st[p] |= FGR_ST_NONFINITE
            continue
        R, t = np.eye(3), np.zeros(3)
        for it in range(K):
            if it % int(anneal_every) == 0 and mu > delta2:
                mu = max(mu / float(division_factor), delta2)
            with np.errstate(all='ignore'):
                q = b @ R.T + t
                r = a - q
                w = w0 * (mu / ((r * r).sum(1) + mu)) ** 2
                J = np.zeros((len(q), 3, 6))
                J[:, 0, 1], J[:, 0, 2] = -q[:, 2], q[:, 1]                 # [q]x
                J[:, 1, 0], J[:, 1, 2] = q[:, 2], -q[:, 0]
                J[:, 2, 0], J[:, 2, 1] = -q[:, 1], q[:, 0]
                J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = -1.0
                A = np.einsum('n,nij,nik->jk', w, J, J)
                g = np.einsum('n,nij,ni->j', w, J, r)
            if not (np.isfinite(A).all() and np.isfinite(g).all() and np.isfinite(w.sum())):
                st[p] |= FGR_ST_NONFINITE
                break
            wsum[p] = w.sum()
            floor, U, singular = PLANE_PIVOT * A.diagonal().max(), np.zeros((6, 6)), False
            for i in range(6):
                d = A[i, i] - (U[:i, i] ** 2).sum()
                if not d > floor:
                    singular = True
                    break
                U[i, i] = np.sqrt(d)
                U[i, i + 1:] = (A[i, i + 1:] - U[:i, i] @ U[:i, i + 1:]) / U[i, i]
            step = np.zeros(6) if singular else np.linalg.solve(A, -g)
            trace[p, it] = np.concatenate([[mu, wsum[p]], step])
            if singular:
                st[p] |= FGR_ST_SINGULAR
                break
            E = _rodrigues(step[:3])
            R, t = E @ R, E @ t + step[3:]
        if st[p] & FGR_ST_NONFINITE:
            wsum[p] = 0.0
            continue
        T[p, :3, :3], T[p, :3, 3] = R, ca + t - R @ cb
        inl[p] = _inliers_f32(T[p], a32, b32, distance_threshold)
    res = (T, inl, tup, wsum, st)
    return res + (mult, trace) if return_debug else res


def _rodrigues(w):
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-8:
        return np.eye(3) + K
    return np.eye(3) + (np.sin(th) / th) * K + ((1.0 - np.cos(th)) / (th * th)) * (K @ K)


# ------------------------------------------------------------------------------------------------- spatial compatibility
def sc2_compatibility(src, tgt, compat_threshold=0.1):
    """Rule 1 of csrc/sc2.hpp on one pair's [n,3] f32 correspondences -> C [n,n] bool: only + - * in f64, in the
    header's order, so the bits are the kernel's."""
    a, b = np.asarray(src, dtype=np.float32).astype(np.float64), np.asarray(tgt, dtype=np.float32).astype(np.float64)

    def d2(p):
        d = p[:, None, :] - p[None, :, :]
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    with np.errstate(all='ignore'):
        A, B = d2(a), d2(b)
        s = (A + B) - float(compat_threshold) * float(compat_threshold)
        C = (s < 0.0) | (s * s < 4.0 * (A * B))
    np.fill_diagonal(C, False)
    return C


def sc2_pack_rows(C, W):
    """[n,n] bool -> uint64 [n,W]: bit l of word w is column 64 w + l."""
    n = C.shape[0]
    wide = np.zeros((n, 64 * W), dtype=bool)
    wide[:, :n] = C
    return np.ascontiguousarray(np.packbits(wide, axis=1, bitorder='little')).view('<u8').astype(np.uint64).reshape(n, W)


def _kabsch(s, g):
    """[n,3] f64 source / target -> (R, t) with src ~ R tgt + t (SVD, reflection fix)."""
    cs, ct = s.mean(0), g.mean(0)
    U, _, Vt = np.linalg.svd((g - ct).T @ (s - cs))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
    R = Vt.T @ D @ U.T
    return R, cs - R @ ct


def sc2_numpy(src, tgt, seg, distance_threshold=0.05, compat_threshold=0.1, num_seeds=256, set_size=20, refine_iters=3,
              max_count=None, return_debug=False):
    """The rule of ``ops.sc2_rigid`` (csrc/sc2.hpp) restated in NumPy -- the independent witness of the device code and
    its host twin: bit-packed rows and ``np.bitwise_count`` for everything integer (equal bit for bit), an SVD fit in
    place of Horn's quaternions and ``np.mean`` sums for everything f64 (equal to rounding).  ``src`` / ``tgt`` [rows,3]
    f32 and ``seg`` [P,2] are host arrays.  Returns arrays ``(T [P,4,4], inliers [P], best_seed [P], best_count [P],
    status [P])`` and, with ``return_debug``, ``(degree [rows], seed_rows [P,S], consensus [P,S,set_size], hyp_count
    [P,S], hyp_rt [P,S,12] f32, matrix int64 [P,max_count,W])`` as ``ops.sc2_rigid`` does."""
    src = np.ascontiguousarray(src, dtype=np.float32).reshape(-1, 3)
    tgt = np.ascontiguousarray(tgt, dtype=np.float32).reshape(-1, 3)
    seg = np.asarray(seg, dtype=np.int64).reshape(-1, 2)
    P, rows, S, K = seg.shape[0], src.shape[0], int(num_seeds), int(set_size)
    mc = max(1, min(rows, SC2_MAX_COUNT)) if max_count is None else int(max_count)
    W = (mc + 63) // 64
    T = np.tile(np.eye(4), (P, 1, 1))
    inl, bc, st = (np.zeros(P, dtype=np.int32) for _ in range(3))
    bs = np.full(P, -1, dtype=np.int32)
    degree = np.zeros(rows, dtype=np.int32)
    seed_rows = np.full((P, S), -1, dtype=np.int32)
    consensus = np.full((P, S, K), -1, dtype=np.int32)
    hyp_count = np.full((P, S), -1, dtype=np.int32)
    hyp_rt = np.zeros((P, S, 12), dtype=np.float32)
    matrix = np.zeros((P, mc, W), dtype=np.uint64)
    for p, (off, n) in enumerate(seg):
        if off < 0 or n < 0 or n > mc or off + n > rows:
            st[p] = SC2_ST_SEGMENT
            continue
        if n < 3:
            st[p] = SC2_ST_FEW
        a32, b32 = src[off:off + n], tgt[off:off + n]
        M = sc2_pack_rows(sc2_compatibility(a32, b32, compat_threshold), W)
        matrix[p, :n] = M
        deg = np.bitwise_count(M).sum(axis=1).astype(np.int64)
        degree[off:off + n] = deg
        order = np.lexsort((np.arange(n), -deg))[:min(S, n)]              # descending degree, ties to the lower row
        seed_rows[p, :len(order)] = order
        a64, b64 = a32.astype(np.float64), b32.astype(np.float64)
        best, best_T = (-1, 0), None
        for rank, i in enumerate(order):
            cand = np.nonzero((M[i, np.arange(n) >> 6] >> (np.arange(n) & 63).astype(np.uint64)) & np.uint64(1))[0]
            s2 = np.bitwise_count(M[i][None, :] & M[cand]).sum(axis=1).astype(np.int64)
            pick = cand[np.argsort(-s2, kind='stable')][:K - 1]           # descending s_ij, ties to the lower j
            rows_of_set = np.concatenate([[i], pick])
            consensus[p, rank, :len(rows_of_set)] = rows_of_set
            if deg[i] < 2:
                continue
            Th = np.eye(4)
            Th[:3, :3], Th[:3, 3] = _kabsch(a64[rows_of_set], b64[rows_of_set])
            c = _inliers_f32(Th, a32, b32, distance_threshold)
            hyp_count[p, rank] = c
            hyp_rt[p, rank] = np.concatenate([Th[:3, :3].reshape(-1), Th[:3, 3]]).astype(np.float32)
            if c > best[0]:                                                # first maximum: ties to the lowest rank
                best, best_T = (c, rank), Th
        if st[p]:
            continue
        if best_T is None:
            st[p] = SC2_ST_NO_HYPOTHESIS
            continue
        bs[p], bc[p] = order[best[1]], best[0]
        Tc = best_T
        for it in range(int(refine_iters) + 1):
            mask = _inlier_mask_f32(Tc, a32, b32, distance_threshold)
            inl[p] = int(mask.sum())
            if it == int(refine_iters) or inl[p] < 3:
                break
            Tc = np.eye(4)
            Tc[:3, :3], Tc[:3, 3] = _kabsch(a64[mask], b64[mask])
        T[p] = Tc
    res = (T, inl, bs, bc, st)
    return res + (degree, seed_rows, consensus, hyp_count, hyp_rt, matrix.view(np.int64)) if return_debug else res


def _fgr(src, tgt, seg, params, hint):
    p = dict(FGR_DEFAULTS)
    p.update(params or {})
    return ops.fgr_rigid(src, tgt, seg, **p)


def _sc2(src, tgt, seg, params, hint):
    p = dict(SC2_DEFAULTS)
    p.update(params or {})
    p.setdefault('max_count', hint)
    return ops.sc2_rigid(src, tgt, seg, **p)


def _ransac_entry(src, tgt, seg, params, hint):
    return _ransac(src, tgt, seg, params)


# estimator name -> (the keyword that carries its parameters, None: the entry point's own **keywords; its call).  A call
# takes (src, tgt, seg, parameters, the longest segment the compaction can produce) and returns (T, inliers, ...).
_ESTIMATORS = {'ransac': (None, _ransac_entry), 'fgr': ('fgr', _fgr), 'sc2': ('sc2', _sc2)}
# estimator name -> the longest correspondence set it takes (None: as long as the buffers are)
_MATCH_LIMITS = {'ransac': RANSAC_MAX_COUNT, 'fgr': None, 'sc2': SC2_MAX_COUNT}


def _check_estimator(estimator, given, ransac):
    """The ``estimator=`` / ``fgr=`` / ``sc2=`` / ``**ransac`` keywords of the three entry points, checked before any
    work.  ``given``: {keyword: value} of the estimators' own dicts."""
    if estimator not in _ESTIMATORS:
        raise ValueError("estimator must be one of %s, got %r" % (sorted(_ESTIMATORS), estimator))
    own = _ESTIMATORS[estimator][0]
    for name, value in given.items():
        if value is None:
            continue
        if name != own:
            raise ValueError("%s= is only taken with estimator=%r" % (name, name))
        if not isinstance(value, dict):
            raise ValueError("%s must be None or a dict of ops.%s_rigid keywords" % (name, name))
    if own is not None and ransac:
        raise ValueError("estimator=%r takes its parameters in %s=, not %s" % (estimator, own, sorted(ransac)))


def _estimate(estimator, given, src, tgt, seg, ransac, hint):
    """(T, inliers) of the compacted matches by the chosen estimator; ``hint``: no segment is longer than this."""
    own, call = _ESTIMATORS[estimator]
    return call(src, tgt, seg, ransac if own is None else given[own], hint)[:2]


# ------------------------------------------------------------------------------------------------- ICP refinement
def _pose44(T, P):
    T = np.asarray(T, dtype=np.float64)
    if T.shape not in ((P, 4, 4), (P, 3, 4)):
        raise ValueError("T must be [P,4,4] or [P,3,4] for the %d pairs, got %s" % (P, T.shape))
    out = np.tile(np.eye(4), (P, 1, 1))
    out[:, :3, :] = T[:, :3, :]
    return out


def normals_scale(radius):
    """Q = 2^floor(log2(2^20 / radius)) for the f32 ``radius``, in double (frexp is exact)."""
    return 2.0 ** (np.frexp(2.0 ** 20 / float(np.float32(radius)))[1] - 1)


def estimate_normals_numpy(clouds, radius, min_neighbors=3, viewpoint=None, return_moments=False, block=1 << 21):
    """The contract of ``ops.estimate_normals`` in NumPy (include/d3feat_hip.h): ``clouds`` a list of [n,3] f32 arrays,
    each searched on its own.  Returns ``(normals f32 [N,3], count int32 [N])`` over the stacked rows and, with
    ``return_moments``, ``moments int64 [N,10]`` -- the same integers the kernel adds, so counts and moments are equal
    to the device's bit for bit; the eigenvectors come from ``numpy.linalg.eigh`` in f64 and agree with the kernel's
    Jacobi solver to rounding.  Brute force within a window of the rows sorted by x: exact, and fast enough for
    fragments."""
    r32 = np.float32(radius)
    if not (0.0 < float(r32) < np.inf) or int(min_neighbors) < 1:
        raise ValueError("radius must be positive and finite, min_neighbors at least 1")
    r2, Q = r32 * r32, normals_scale(radius)
    view = np.zeros(3) if viewpoint is None else np.asarray(viewpoint, dtype=np.float32).astype(np.float64).reshape(3)
    normals, counts, moments = [], [], []
    for cloud in clouds:
        p = np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 3)
        n = p.shape[0]
        order = np.argsort(p[:, 0], kind='stable')
        ps = p[order]
        m = np.zeros((n, 10), dtype=np.int64)
        reach = float(r32) * 1.001 + 1e-6
        step = max(1, int(block) // max(n, 1))
        for s in range(0, n, step):
            q = ps[s:s + step]
            lo = np.searchsorted(ps[:, 0], float(q[0, 0]) - reach, 'left')
            hi = np.searchsorted(ps[:, 0], float(q[-1, 0]) + reach, 'right')
            t = ps[lo:hi]
            d = t[None, :, :] - q[:, None, :]                          # p_j - p_i: one f32 subtraction
            e = q[:, None, :] - t[None, :, :]                          # the search's p_i - p_j
            d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
            inside = d2 < r2
            u = np.where(inside[..., None], np.rint(d.astype(np.float64) * Q).astype(np.int64), 0)
            ux, uy, uz = u[..., 0], u[..., 1], u[..., 2]
            m[s:s + step] = np.stack([inside.sum(1), ux.sum(1), uy.sum(1), uz.sum(1), (ux * ux).sum(1),
                                      (ux * uy).sum(1), (ux * uz).sum(1), (uy * uy).sum(1), (uy * uz).sum(1),
                                      (uz * uz).sum(1)], 1)
        back = np.empty(n, dtype=np.int64)
        back[order] = np.arange(n)
        m = m[back]
        nrm = np.zeros((n, 3), dtype=np.float32)
        live = np.nonzero(m[:, 0] >= int(min_neighbors))[0]
        if live.size:
            k = m[live, 0].astype(np.float64)
            sm = m[live, 1:4].astype(np.float64)
            S = m[live][:, [4, 5, 6, 5, 7, 8, 6, 8, 9]].astype(np.float64).reshape(-1, 3, 3)
            C = (S - sm[:, :, None] * sm[:, None, :] / k[:, None, None]) / k[:, None, None] / (Q * Q)
            w, V = np.linalg.eigh(C)
            v = V[:, :, 0]
            dot = (v * (view - p[live].astype(np.float64))).sum(1)
            first = np.take_along_axis(v, np.argmax(v != 0.0, axis=1)[:, None], 1)[:, 0]
            v = np.where(((dot < 0) | ((dot == 0) & (first < 0)))[:, None], -v, v)
            nrm[live] = np.where((w[:, 2] > 0)[:, None], v, 0.0).astype(np.float32)
        normals.append(nrm)
        counts.append(m[:, 0].astype(np.int32))
        moments.append(m)
    cat = lambda xs, shape, dt: np.concatenate(xs) if xs else np.zeros(shape, dtype=dt)
    res = (cat(normals, (0, 3), np.float32), cat(counts, (0,), np.int32))
    return res + (cat(moments, (0, 10), np.int64),) if return_moments else res


def _plane_step(x, ym, nrm, T, py):
    """One point-to-plane fit (include/d3feat_hip.h): moving points x matched to fixed points ym with normals nrm under
    the 4x4 T, about the pivot py -> (T_next, singular).  The pivot test is the kernel's (Cholesky of the normal
    equations); the solution is a least-squares solve of the stacked system."""
    J, r = _plane_rows(x, ym, nrm, T, py)[:2]
    return _step_from_rows(J, r, T, py)


def _plane_rows(x, ym, nrm, T, py):
    """The stacked point-to-plane rows ``J [n,6]``, ``r [n]`` of include/d3feat_hip.h, and a, c."""
    R, t = T[:3, :3], T[:3, 3]
    x = x.astype(np.float64)
    a = np.stack([((R[r, 0] * x[:, 0] + R[r, 1] * x[:, 1]) + R[r, 2] * x[:, 2]) + t[r] for r in range(3)], 1) - py
    c = ym.astype(np.float64) - py
    n = nrm.astype(np.float64)
    return np.concatenate([np.cross(a, n), n], 1), ((a - c) * n).sum(1), a, c


def _color_rows(a, c, fy, ix):
    """The unweighted colour rows of the accepted correspondences (include/d3feat_hip.h): ``fy [n,4]`` the field rows of
    the matched fixed points, ``ix [n]`` the intensities of the moving points -> ``(J_C [m,6], r_C [m])`` over the m rows
    where ``fy`` is finite in all four entries and ``ix`` is finite."""
    ok = np.isfinite(fy).all(1) & np.isfinite(ix)
    d = fy[ok, :3].astype(np.float64)
    a, c = a[ok], c[ok]
    r = (fy[ok, 3].astype(np.float64) - ix[ok].astype(np.float64)) + ((a - c) * d).sum(1)
    return np.concatenate([np.cross(a, d), d], 1), r


def _step_from_rows(J, r, T, py):
    """The fit of ``_plane_step`` on the stacked rows J, r."""
    R, t = T[:3, :3], T[:3, 3]
    A = J.T @ J
    floor, U = PLANE_PIVOT * A.diagonal().max(), np.zeros((6, 6))
    for i in range(6):
        d = A[i, i] - (U[:i, i] ** 2).sum()
        if not d > floor:
            return T, True
        U[i, i] = np.sqrt(d)
        U[i, i + 1:] = (A[i, i + 1:] - U[:i, i] @ U[:i, i + 1:]) / U[i, i]
    v = np.linalg.lstsq(J, -r, rcond=None)[0]
    ca, sa, cb, sb, cg, sg = np.cos(v[0]), np.sin(v[0]), np.cos(v[1]), np.sin(v[1]), np.cos(v[2]), np.sin(v[2])
    D = np.array([[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa],
                  [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa],
                  [-sb, cb * sa, cb * ca]])                            # Rz(gamma) Ry(beta) Rx(alpha)
    out = np.eye(4)
    out[:3, :3] = D @ R
    out[:3, 3] = D @ (t - py) + py + v[3:]
    return out, False


def _per_cloud(rows, clouds, width, name):
    """A stacked f32 array [N, width] (or one array per cloud) -> one array per cloud."""
    if isinstance(rows, (list, tuple)):
        return [np.ascontiguousarray(r, dtype=np.float32).reshape(-1, width) for r in rows]
    rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, width)
    ends = np.cumsum([len(c) for c in clouds])
    if rows.shape[0] != (ends[-1] if len(ends) else 0):
        raise ValueError("%s must hold one row per stacked point" % name)
    return [rows[e - len(c):e] for e, c in zip(ends, clouds)]


def icp_numpy(clouds, pairs, T_init, max_distance, max_iters=30, rel_fitness=1e-6, rel_rmse=1e-6, return_trace=False,
              normals=None, color_field=None, lambda_geometric=LAMBDA_GEOMETRIC):
    """The contract of ``ops.icp_rigid`` in NumPy f64 (include/d3feat_hip.h): the ``device='cpu'`` path of
    ``refine_transforms`` and the oracle of the GPU tests.  ``clouds``: list of [n,3] f32 arrays; pair p = (moving cloud
    a, fixed cloud b), ``T_init[p]`` maps a into b's frame.  The search is ``preprocess.transform_points`` /
    ``nearest_within``; the fit is the SVD solution of the same least-squares problem the kernel solves with Horn's
    quaternions.  Returns ``(T [P,4,4], count int32 [P], rmse [P], iterations int32 [P], status int32 [P])`` and, with
    ``return_trace``, ``trace [P, max_iters+1, 2]`` = (n_k, sum d2_k), NaN beyond the stop.  ``normals``: None, or
    the f32 normals of the stacked clouds [N,3] (or one array per cloud): the point-to-plane form, whose fit follows
    ``_plane_step`` and which may end with ``ICP_ST_SINGULAR``.  ``color_field``: None, or the f32 field [N,4] of
    ``color_gradients_numpy`` / ``ops.color_gradients`` (or one array per cloud; requires ``normals``): the COLOURED
    form -- the point-to-plane rows times ``sqrt(lambda_geometric)`` stacked with the colour rows times
    ``sqrt(1 - lambda_geometric)`` (rows of weight zero are left out: they add nothing), the same pivot test and solve --
    and ``n_color int32 [P]``, ``color_rmse [P]`` of the returned poses are appended to the results."""
    from ..datasets.preprocess import nearest_within, transform_points
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    P, K = pairs.shape[0], int(max_iters)
    if K < 0:
        raise ValueError("max_iters must be >= 0")
    if normals is not None and not isinstance(normals, (list, tuple)):
        normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        ends = np.cumsum([len(c) for c in clouds])
        if normals.shape[0] != (ends[-1] if len(ends) else 0):
            raise ValueError("normals must hold one row per stacked point")
        normals = [normals[e - len(c):e] for e, c in zip(ends, clouds)]
    colored = color_field is not None
    if colored:
        if normals is None:
            raise ValueError("color_field requires normals")
        if not 0.0 <= float(lambda_geometric) <= 1.0:
            raise ValueError("lambda_geometric must be in [0, 1]")
        field = _per_cloud(color_field, clouds, 4, "color_field")
        sg, sc = np.sqrt(float(lambda_geometric)), np.sqrt(1.0 - float(lambda_geometric))
    n_color, color_rmse = np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.float64)
    T = _pose44(T_init, P)
    count, iters, status = (np.zeros(P, dtype=np.int32) for _ in range(3))
    rmse = np.zeros(P, dtype=np.float64)
    trace = np.full((P, K + 1, 2), np.nan)
    for p, (a, b) in enumerate(pairs):
        if not (0 <= a < len(clouds) and 0 <= b < len(clouds)):
            status[p] |= ICP_ST_PAIR
        if not np.isfinite(T[p, :3]).all():
            status[p] |= ICP_ST_NONFINITE
        if status[p]:
            continue
        x = np.ascontiguousarray(clouds[a], dtype=np.float32).reshape(-1, 3)
        y = np.ascontiguousarray(clouds[b], dtype=np.float32).reshape(-1, 3)
        prev = (0.0, 0.0)
        for k in range(K + 1):
            q = transform_points(x, T[p])
            nn = nearest_within(q, y, max_distance)
            sel = nn >= 0
            n = int(sel.sum())
            ym = y[nn[sel]]
            d = q[sel] - ym                                              # f32, the kernel's d2
            d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            sd2 = float(d2.astype(np.float64).sum())
            fitness = n / x.shape[0] if x.shape[0] else 0.0
            r = float(np.sqrt(sd2 / n)) if n else 0.0
            trace[p, k] = (n, sd2)
            count[p], rmse[p] = n, r
            if colored and n:
                Jg, rg, av, cv = _plane_rows(x[sel], ym, normals[b][nn[sel]], T[p], y[0].astype(np.float64))
                Jc, rc = _color_rows(av, cv, field[b][nn[sel]], field[a][sel, 3])
                n_color[p] = len(rc)
                color_rmse[p] = float(np.sqrt((rc * rc).sum() / len(rc))) if len(rc) else 0.0
            elif colored:
                n_color[p], color_rmse[p] = 0, 0.0
            if n < 3:
                status[p] |= ICP_ST_FEW
                break
            if k >= 1 and abs(fitness - prev[0]) < rel_fitness and abs(r - prev[1]) < rel_rmse:
                break
            if k == K:
                break
            px, py = x[0].astype(np.float64), y[0].astype(np.float64)    # pivots: row 0 of either cloud
            if normals is not None:
                if colored:
                    Jg, rg = sg * Jg, sg * rg
                    if sc > 0.0:
                        Jg, rg = np.concatenate([Jg, sc * Jc]), np.concatenate([rg, sc * rc])
                    T[p], singular = _step_from_rows(Jg, rg, T[p], py)
                else:
                    T[p], singular = _plane_step(x[sel], ym, normals[b][nn[sel]], T[p], py)
                if singular:
                    status[p] |= ICP_ST_SINGULAR
                    break
                prev = (fitness, r)
                iters[p] = k + 1
                continue
            xs, ys = x[sel].astype(np.float64) - px, ym.astype(np.float64) - py
            cx, cy = xs.mean(0), ys.mean(0)
            U, _, Vt = np.linalg.svd((xs - cx).T @ (ys - cy))            # S[a,b] = sum moving'_a fixed'_b
            D = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
            R = Vt.T @ D @ U.T                                           # y ~ R x + t
            T[p, :3, :3] = R
            T[p, :3, 3] = (cy + py) - R @ (cx + px)
            prev = (fitness, r)
            iters[p] = k + 1
    res = (T, count, rmse, iters, status)
    res = res + (trace,) if return_trace else res
    return res + (n_color, color_rmse) if colored else res


def intensity_of(colors):
    """The intensity the coloured ICP takes, f32 [N], from the colours ``fuse_fragments(color=)`` returns (array or
    tensor; the result is of the same kind): ``[N,1]`` (or ``[N]``) passes as it is; ``[N,3]`` f32 in [0, 1] becomes
    ``(0.299 R + 0.587 G) + 0.114 B`` in f32, the RGB-D tracker's weights; uint8 is divided by 255 as ``rgbd_pyramid``
    does.  NaN stays NaN: "no colour"."""
    tensor = isinstance(colors, torch.Tensor)
    c = colors if tensor else np.asarray(colors)
    eight = c.dtype == (torch.uint8 if tensor else np.uint8)
    c = c.to(torch.float32) if tensor else c.astype(np.float32)
    n = int(c.shape[0])
    c = c.reshape(n, -1)
    if c.shape[1] == 3:
        w = (torch.tensor if tensor else np.float32)([0.299, 0.587, 0.114])
        if tensor:
            w = w.to(c.device)
        I = (w[0] * c[:, 0] + w[1] * c[:, 1]) + w[2] * c[:, 2]
    elif c.shape[1] == 1:
        I = c[:, 0]
    else:
        raise ValueError("colors must be [N], [N,1] or [N,3], got %s" % (tuple(colors.shape),))
    if eight:
        I = I / 255.0 if tensor else I / np.float32(255.0)
    return I.contiguous() if tensor else np.ascontiguousarray(I, dtype=np.float32)


def color_gradients_numpy(clouds, radius, normals, intensity, min_neighbors=4, return_moments=False, block=1 << 21):
    """The contract of ``ops.color_gradients`` in NumPy (include/d3feat_hip.h): ``clouds`` a list of [n,3] f32 arrays,
    each searched on its own; ``normals`` f32 [N,3] and ``intensity`` f32 [N] over the stacked rows (or one array per
    cloud).  Returns ``(field f32 [N,4] = (d, I), count int32 [N])`` and, with ``return_moments``, ``moments int64
    [N,13]`` -- the integers the kernel adds, equal to the device's bit for bit; the 2x2 solve is the kernel's closed
    form in f64.  Brute force within a window of the rows sorted by x, as ``estimate_normals_numpy``."""
    r32 = np.float32(radius)
    if not (0.0 < float(r32) < np.inf) or int(min_neighbors) < 1:
        raise ValueError("radius must be positive and finite, min_neighbors at least 1")
    r2, Q = r32 * r32, normals_scale(radius)
    normals = _per_cloud(normals, clouds, 3, "normals")
    intensity = _per_cloud(intensity, clouds, 1, "intensity")
    fields, counts, moments = [], [], []
    for cloud, nrm, inten in zip(clouds, normals, intensity):
        p = np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 3)
        n = p.shape[0]
        I = inten.reshape(-1)
        if nrm.shape[0] != n or I.shape[0] != n:
            raise ValueError("normals and intensity must hold one row per point")
        with np.errstate(invalid='ignore'):
            usable = (I >= np.float32(0)) & (I <= np.float32(1))
        q = np.where(usable, np.rint(np.where(usable, I, 0).astype(np.float64) * INTENSITY_SCALE), 0).astype(np.int64)
        order = np.argsort(p[:, 0], kind='stable')
        ps, qs, us = p[order], q[order], usable[order]
        m = np.zeros((n, 13), dtype=np.int64)
        reach = float(r32) * 1.001 + 1e-6
        step = max(1, int(block) // max(n, 1))
        for s in range(0, n, step):
            qp = ps[s:s + step]
            lo = np.searchsorted(ps[:, 0], float(qp[0, 0]) - reach, 'left')
            hi = np.searchsorted(ps[:, 0], float(qp[-1, 0]) + reach, 'right')
            t = ps[lo:hi]
            d = t[None, :, :] - qp[:, None, :]                         # p_j - p_i: one f32 subtraction
            e = qp[:, None, :] - t[None, :, :]                         # the search's p_i - p_j
            d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
            inside = (d2 < r2) & us[None, lo:hi] & us[s:s + step, None]
            u = np.where(inside[..., None], np.rint(d.astype(np.float64) * Q).astype(np.int64), 0)
            ux, uy, uz = u[..., 0], u[..., 1], u[..., 2]
            c = np.where(inside, qs[None, lo:hi] - qs[s:s + step, None], 0)
            m[s:s + step] = np.stack([inside.sum(1), ux.sum(1), uy.sum(1), uz.sum(1), (ux * ux).sum(1),
                                      (ux * uy).sum(1), (ux * uz).sum(1), (uy * uy).sum(1), (uy * uz).sum(1),
                                      (uz * uz).sum(1), (ux * c).sum(1), (uy * c).sum(1), (uz * c).sum(1)], 1)
        back = np.empty(n, dtype=np.int64)
        back[order] = np.arange(n)
        m = m[back]
        fields.append(color_field_from_moments(m, Q, nrm, I, min_neighbors))
        counts.append(m[:, 0].astype(np.int32))
        moments.append(m)
    cat = lambda xs, shape, dt: np.concatenate(xs) if xs else np.zeros(shape, dtype=dt)
    res = (cat(fields, (0, 4), np.float32), cat(counts, (0,), np.int32))
    return res + (cat(moments, (0, 13), np.int64),) if return_moments else res


def color_field_from_moments(m, Q, nrm, intensity, min_neighbors=4):
    """Everything after the moments of ``color_gradients_numpy`` (csrc/color_icp.hpp gradient_from_moments, in the same
    order of operations): ``m int64 [n,13]``, ``nrm f32 [n,3]``, ``intensity f32 [n]`` -> ``field f32 [n,4]``."""
    m = np.asarray(m, dtype=np.int64).reshape(-1, 13)
    nv = np.asarray(nrm, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    I = np.asarray(intensity, dtype=np.float32).reshape(-1)
    n = m.shape[0]
    field = np.full((n, 4), np.nan, dtype=np.float32)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        usable = (I >= np.float32(0)) & (I <= np.float32(1))
        field[usable, 3] = I[usable]
        mag = np.abs(nv)
        ok = usable & (m[:, 0] >= int(min_neighbors)) & (mag.sum(1) > 0.0)
        use_y = mag[:, 1] < mag[:, 0]
        use_z = mag[:, 2] < np.where(use_y, mag[:, 1], mag[:, 0])
        k = np.where(use_z, 2, np.where(use_y, 1, 0))
        axis = np.eye(3)[k]
        e1 = np.cross(nv, axis)
        e1 = e1 / np.sqrt((e1[:, 0] * e1[:, 0] + e1[:, 1] * e1[:, 1]) + e1[:, 2] * e1[:, 2])[:, None]
        e2 = np.cross(nv, e1)
        S = m[:, [4, 5, 6, 5, 7, 8, 6, 8, 9]].astype(np.float64).reshape(-1, 3, 3) * (1.0 / (Q * Q))
        h = m[:, 10:13].astype(np.float64) * (1.0 / (Q * INTENSITY_SCALE))
        a1, a2 = np.einsum('nij,nj->ni', S, e1), np.einsum('nij,nj->ni', S, e2)
        g00, g01, g11 = (e1 * a1).sum(1), (e1 * a2).sum(1), (e2 * a2).sum(1)
        b0, b1 = (e1 * h).sum(1), (e2 * h).sum(1)
        det, top = g00 * g11 - g01 * g01, np.maximum(g00, g11)
        ok &= det > GRADIENT_PIVOT * (top * top)
        c0, c1 = (g11 * b0 - g01 * b1) / det, (g00 * b1 - g01 * b0) / det
        d = e1 * c0[:, None] + e2 * c1[:, None]
        field[ok, :3] = d[ok].astype(np.float32)
    return field


# ------------------------------------------------------------------------------------------------- FPFH descriptors
FPFH_MAX_NEIGHBORS = 1 << 18                     # csrc/fpfh.hpp kMaxNeighbors
FPFH_WEIGHT_SCALE, FPFH_WEIGHT_CAP = 2.0 ** 32, 2.0 ** 12
# cos and sin of theta_b = -pi + 2 pi b / 11, b = 1..10: the constants of csrc/fpfh.hpp, b = 11 - k mirrored from b = k
_FPFH_COS5 = [-0.8412535328311811, -0.4154150130018863, 0.14231483827328512, 0.6548607339452851, 0.9594929736144975]
_FPFH_SIN5 = [-0.5406408174555978, -0.9096319953545184, -0.9898214418809327, -0.7557495743542583, -0.2817325568414295]
FPFH_COS = np.array(_FPFH_COS5 + _FPFH_COS5[::-1], dtype=np.float64)
FPFH_SIN = np.array(_FPFH_SIN5 + [-s for s in _FPFH_SIN5[::-1]], dtype=np.float64)


def _fpfh_feature_bin(f):
    t = np.floor((11.0 * (f + 1.0)) * 0.5)
    return np.where(t >= 10.0, 10.0, np.where(t >= 0.0, t, 0.0)).astype(np.int64)


def fpfh_pair_bins(dp, d2, ni, nj):
    """The three bins (theta, f2, f3; each 0..10) of pairs (i, j) under the rule of csrc/fpfh.hpp: ``dp`` [m,3] f64 =
    p_j - p_i, ``d2`` [m] its squared length as the rule sums it (non-zero), ``ni`` / ``nj`` [m,3] f64 normals.
    Only + - * / sqrt and floor, in the header's order."""
    px, py, pz = dp[:, 0], dp[:, 1], dp[:, 2]
    with np.errstate(all='ignore'):
        dist = np.sqrt(d2)
        a1 = ((ni[:, 0] * px + ni[:, 1] * py) + ni[:, 2] * pz) / dist
        a2 = ((nj[:, 0] * px + nj[:, 1] * py) + nj[:, 2] * pz) / dist
        swap = np.abs(a1) < np.abs(a2)
        n1 = np.where(swap[:, None], nj, ni)
        n2 = np.where(swap[:, None], ni, nj)
        qx, qy, qz = np.where(swap, -px, px), np.where(swap, -py, py), np.where(swap, -pz, pz)
        f3 = np.where(swap, -a2, a1)
        vx, vy, vz = qy * n1[:, 2] - qz * n1[:, 1], qz * n1[:, 0] - qx * n1[:, 2], qx * n1[:, 1] - qy * n1[:, 0]
        vn = np.sqrt((vx * vx + vy * vy) + vz * vz)
        flat = vn == 0.0
        vx, vy, vz = vx / vn, vy / vn, vz / vn
        wx, wy, wz = n1[:, 1] * vz - n1[:, 2] * vy, n1[:, 2] * vx - n1[:, 0] * vz, n1[:, 0] * vy - n1[:, 1] * vx
        f2 = (vx * n2[:, 0] + vy * n2[:, 1]) + vz * n2[:, 2]
        y = (wx * n2[:, 0] + wy * n2[:, 1]) + wz * n2[:, 2]
        x = (n1[:, 0] * n2[:, 0] + n1[:, 1] * n2[:, 1]) + n1[:, 2] * n2[:, 2]
        reached = (y[:, None] * FPFH_COS[None, :] - x[:, None] * FPFH_SIN[None, :]) >= 0.0
    theta = np.where(y < 0.0, reached[:, :5].sum(1), 5 + reached[:, 5:].sum(1))
    theta = np.where((x == 0.0) & (y == 0.0), 5, theta)
    five = np.int64(5)
    return (np.where(flat, five, theta).astype(np.int64), np.where(flat, five, _fpfh_feature_bin(f2)),
            np.where(flat, five, _fpfh_feature_bin(f3)))


def _fpfh_blocks(ps, usable, r2f, reach, block):
    """Blocks of the rows of one cloud sorted by x: (s, lo, accepted [rows, window] bool, d [rows, window, 3] f64 =
    p_j - p_i, d2 [rows, window] f64) with the window ps[lo:lo + window] -- the neighbourhood test of csrc/fpfh.hpp."""
    n = ps.shape[0]
    step = max(1, int(block) // max(n, 1))
    for s in range(0, n, step):
        q = ps[s:s + step]
        lo = np.searchsorted(ps[:, 0], float(q[0, 0]) - reach, 'left')
        hi = np.searchsorted(ps[:, 0], float(q[-1, 0]) + reach, 'right')
        t = ps[lo:hi]
        e = q[:, None, :] - t[None, :, :]                              # the search's p_i - p_j, f32
        d2f = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
        d = t.astype(np.float64)[None, :, :] - q.astype(np.float64)[:, None, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        ok = (d2f < r2f) & (d2 != 0.0) & usable[s:s + step, None] & usable[None, lo:hi]
        yield s, lo, ok, d, d2


def fpfh_numpy(clouds, radius, normals, return_spfh=False, unit=False, block=1 << 20):
    """The contract of ``ops.fpfh`` in NumPy (csrc/fpfh.hpp): ``clouds`` a list of [n,3] f32 arrays, each searched on
    its own, ``normals`` f32 [N,3] over the stacked rows.  Returns ``(desc f32 [N,33], count int32 [N])`` and, with
    ``return_spfh``, ``spfh int32 [N,33]`` -- equal to the device's and the host twin's bit for bit: the rule uses only
    correctly rounded f64 operations and integer sums.  ``unit``: rows scaled to unit L2 norm by the rule's fixed-order
    sum of squares.  Brute force within a window of the rows sorted by x, like
    ``estimate_normals_numpy``."""
    r32 = np.float32(radius)
    if not (0.0 < float(r32) < np.inf):
        raise ValueError("radius must be positive and finite")
    r2f, r2 = r32 * r32, float(r32) * float(r32)
    reach = float(r32) * 1.001 + 1e-6
    nrm_all = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    descs, counts, spfhs = [], [], []
    row0 = 0
    for cloud in clouds:
        p = np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 3)
        n = p.shape[0]
        nrm = nrm_all[row0:row0 + n]
        if nrm.shape[0] != n:
            raise ValueError("normals must hold one row per point of every cloud")
        row0 += n
        order = np.argsort(p[:, 0], kind='stable')
        ps, ns = p[order], nrm[order].astype(np.float64)
        usable = (nrm[order] != 0).any(1)
        c = np.zeros((n, 33), dtype=np.int64)
        for s, lo, ok, d, d2 in _fpfh_blocks(ps, usable, r2f, reach, block):
            qi, tj = np.nonzero(ok)
            if not qi.size:
                continue
            bins = fpfh_pair_bins(d[qi, tj], d2[qi, tj], ns[s + qi], ns[lo + tj])
            rows = ok.shape[0]
            for h in range(3):
                c[s:s + rows, 11 * h:11 * h + 11] = np.bincount(qi * 11 + bins[h], minlength=rows * 11).reshape(rows, 11)
        cnt = c[:, :11].sum(1)
        S = np.zeros((n, 33), dtype=np.int64)
        for s, lo, ok, d, d2 in _fpfh_blocks(ps, usable, r2f, reach, block):
            nj = np.broadcast_to(cnt[None, lo:lo + ok.shape[1]], ok.shape)
            with np.errstate(all='ignore'):
                W = np.rint((FPFH_WEIGHT_SCALE * np.minimum(r2 / d2, FPFH_WEIGHT_CAP)) / nj.astype(np.float64))
            W = np.where(ok, W, 0.0).astype(np.int64)
            S[s:s + ok.shape[0]] = W @ c[lo:lo + ok.shape[1]]
        tot = np.repeat(S.reshape(n, 3, 11).sum(2), 11, axis=1)
        live = (cnt >= 1) & (cnt <= FPFH_MAX_NEIGHBORS)
        with np.errstate(all='ignore'):
            first = np.where(tot == 0, 0.0, (100.0 * S.astype(np.float64)) / tot.astype(np.float64))
            desc = first + (100.0 * c.astype(np.float64)) / cnt.astype(np.float64)[:, None]
        desc = np.where(live[:, None], desc, 0.0).astype(np.float32)
        if unit:
            wide, q = desc.astype(np.float64), np.zeros(n)
            for b in range(33):                                        # the rule's order of additions
                q = q + wide[:, b] * wide[:, b]
            with np.errstate(all='ignore'):
                desc = np.where(desc != 0, wide / np.sqrt(q)[:, None], 0.0).astype(np.float32)
        back = np.empty(n, dtype=np.int64)
        back[order] = np.arange(n)
        descs.append(desc[back])
        counts.append(cnt[back].astype(np.int32))
        spfhs.append(c[back].astype(np.int32))
    if row0 != nrm_all.shape[0]:
        raise ValueError("normals must hold one row per point of every cloud")
    cat = lambda xs, shape, dt: np.concatenate(xs) if xs else np.zeros(shape, dtype=dt)
    res = (cat(descs, (0, 33), np.float32), cat(counts, (0,), np.int32))
    return res + (cat(spfhs, (0, 33), np.int32),) if return_spfh else res


def describe_fpfh(clouds, radius, normal_radius=None, viewpoint=None, device='cuda'):
    """FPFH descriptors of fragments, the training-free stand-in for the network: ONE ``ops.CloudGrid`` at
    ``max(radius, normal_radius)`` over all fragments, one ``ops.estimate_normals`` call (``normal_radius`` defaults to
    ``0.4 * radius`` -- Open3D's examples use 2 and 5 voxels; ``viewpoint``: the same point in every fragment's own
    frame, default the origin) and one ``ops.fpfh`` call at ``radius``.  ``clouds``: list of [n,3] arrays / tensors.
    Returns ``(descriptors, counts)``: per fragment a [n,64] f32 block of zero-padded UNIT rows -- the width and the norm
    ``ops.mutual_nn`` reads: it ranks by the inner product, which for unit rows is the order of the L2 distance -- and
    the [n] int32 neighbour counts (0: no descriptor, a row of zeros); device tensors, or NumPy arrays from
    ``device='cpu'`` (``estimate_normals_numpy``, ``fpfh_numpy``)."""
    if normal_radius is None:
        normal_radius = 0.4 * float(radius)
    if not (0.0 < float(radius) < np.inf) or not (0.0 < float(normal_radius) < np.inf):
        raise ValueError("radius and normal_radius must be positive and finite")
    lens = [int(c.shape[0]) for c in clouds]
    ends = np.cumsum([0] + lens)
    if str(device).startswith('cpu'):
        arrs = _host_arrays(clouds)
        nrm = estimate_normals_numpy(arrs, normal_radius, viewpoint=viewpoint)[0]
        d33, cnt = fpfh_numpy(arrs, radius, nrm, unit=True)
        desc = np.zeros((d33.shape[0], 64), dtype=np.float32)
        desc[:, :33] = d33
    else:
        grid = _cloud_grid(clouds, max(float(radius), float(normal_radius)), torch.device(device))
        nrm = ops.estimate_normals(grid, None, normal_radius, viewpoint=viewpoint)[0]
        desc, cnt = ops.fpfh(grid, None, radius, nrm, row_width=64, unit=True)
    return ([desc[ends[k]:ends[k + 1]] for k in range(len(lens))], [cnt[ends[k]:ends[k + 1]] for k in range(len(lens))])


# ------------------------------------------------------------------------- ISS keypoints, suppression, repeatability
def iss_eigenvalues_numpy(moments, Q):
    """f64 [n,3] eigenvalues, descending, of the covariance of the integer ``moments`` [n,10] at scale ``Q``
    (include/d3feat_hip.h) by ``numpy.linalg.eigvalsh``; a row with n < 1 gives zeros."""
    m = np.asarray(moments, dtype=np.int64).reshape(-1, 10)
    e = np.zeros((m.shape[0], 3))
    live = np.nonzero(m[:, 0] >= 1)[0]
    if live.size:
        k = m[live, 0].astype(np.float64)
        sm = m[live, 1:4].astype(np.float64)
        S = m[live][:, [4, 5, 6, 5, 7, 8, 6, 8, 9]].astype(np.float64).reshape(-1, 3, 3)
        C = (S - sm[:, :, None] * sm[:, None, :] / k[:, None, None]) / k[:, None, None] / (float(Q) * float(Q))
        e[live] = np.linalg.eigvalsh(C)[:, ::-1]
    return e


def iss_saliency_numpy(moments, Q, gamma_21=0.975, gamma_32=0.975, min_neighbors=5):
    """Everything after the moments of ``ops.iss_saliency`` in NumPy (csrc/iss.hpp): f32 [n] saliency from the int64
    ``moments`` [n,10]; the eigenvalues come from ``eigvalsh`` and agree with the kernel's Jacobi solver to rounding."""
    m = np.asarray(moments, dtype=np.int64).reshape(-1, 10)
    e = iss_eigenvalues_numpy(m, Q)
    gate = ((m[:, 0] >= int(min_neighbors)) & (e[:, 0] > 0) & (e[:, 1] < float(gamma_21) * e[:, 0])
            & (e[:, 2] < float(gamma_32) * e[:, 1]))
    s = np.where(gate, e[:, 2], 0.0).astype(np.float32)
    return np.where(s > 0, s, np.float32(0.0)).astype(np.float32)


def radius_nms_numpy(clouds, scores, radius, min_neighbors=1, block=1 << 21):
    """The contract of ``ops.radius_nms`` in NumPy, exactly: ``clouds`` a list of [n,3] f32 arrays, ``scores`` the
    stacked f32 scores [N] / [N,1] (or one array per cloud).  Returns ``(keep bool [N], count int32 [N])`` over the
    stacked rows.  Brute force within a window of the rows sorted by x, as ``estimate_normals_numpy``."""
    r32 = np.float32(radius)
    if not (0.0 < float(r32) < np.inf) or int(min_neighbors) < 1:
        raise ValueError("radius must be positive and finite, min_neighbors at least 1")
    score_of = _per_cloud(scores, clouds, 1, "scores")
    r2 = r32 * r32
    keeps, counts = [], []
    for cloud, sc in zip(clouds, score_of):
        p = np.ascontiguousarray(cloud, dtype=np.float32).reshape(-1, 3)
        sc = sc.reshape(-1)
        n = p.shape[0]
        order = np.argsort(p[:, 0], kind='stable')
        ps, ss = p[order], sc[order]
        keep, cnt = np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int32)
        with np.errstate(invalid='ignore'):
            walking = np.nonzero(ss > 0)[0]                               # (a NaN is not > 0)
        reach = float(r32) * 1.001 + 1e-6
        step = max(1, int(block) // max(n, 1))
        for s in range(0, walking.size, step):
            rows = walking[s:s + step]
            q = ps[rows]
            lo = np.searchsorted(ps[:, 0], float(q[0, 0]) - reach, 'left')
            hi = np.searchsorted(ps[:, 0], float(q[-1, 0]) + reach, 'right')
            t, ts = ps[lo:hi], ss[lo:hi]
            e = q[:, None, :] - t[None, :, :]                              # the search's p_i - p_j
            d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
            inside = d2 < r2
            with np.errstate(invalid='ignore'):
                beaten = (inside & (ts[None, :] > ss[rows][:, None])).any(1)
            cnt[rows] = inside.sum(1)
            keep[rows] = ~beaten & (cnt[rows] >= int(min_neighbors))
        back = np.empty(n, dtype=np.int64)
        back[order] = np.arange(n)
        keeps.append(keep[back])
        counts.append(cnt[back])
    cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dtype=dt)
    return cat(keeps, bool), cat(counts, np.int32)


def iss_numpy(clouds, salient_radius, non_max_radius, gamma_21=0.975, gamma_32=0.975, min_neighbors=5):
    """The contract of ``ops.iss_keypoints`` in NumPy: ``(saliency f32 [N], keep bool [N], count_salient int32 [N],
    count_nms int32 [N])`` over the stacked rows of ``clouds``.  The moments are ``estimate_normals_numpy``'s -- the
    integers the kernel adds --, the eigenvalues ``numpy.linalg.eigvalsh``'s (they agree with the kernel's Jacobi solver
    to rounding, so a point whose gate ratio sits within rounding of its threshold may differ), the suppression exact."""
    for g in (gamma_21, gamma_32):
        if not (0.0 < float(g) <= 1.0):
            raise ValueError("gamma_21 and gamma_32 must lie in (0, 1], got %r" % (g,))
    arrs = [np.ascontiguousarray(c, dtype=np.float32).reshape(-1, 3) for c in clouds]
    _, count, moments = estimate_normals_numpy(arrs, salient_radius, min_neighbors=min_neighbors, return_moments=True)
    saliency = iss_saliency_numpy(moments, normals_scale(salient_radius), gamma_21, gamma_32, min_neighbors)
    keep, count_nms = radius_nms_numpy(arrs, saliency, non_max_radius, min_neighbors)
    return saliency, keep, count, count_nms


def _split(rows, lens):
    ends = np.cumsum([0] + list(lens))
    return [rows[ends[k]:ends[k + 1]] for k in range(len(lens))]


def detect_iss(clouds, salient_radius, non_max_radius, gamma_21=0.975, gamma_32=0.975, min_neighbors=5, device='cuda'):
    """ISS keypoints of the fragments of a scene: ONE ``ops.CloudGrid`` at the larger of the two radii over all
    fragments and one ``ops.iss_keypoints`` call.  ``clouds``: list of [n,3] arrays / tensors.  Returns ``(saliency,
    rows)``: per fragment the [n] f32 saliency (0: not salient) and the ascending row indices (int64) of the points that
    survive the suppression; device tensors, or NumPy arrays from ``device='cpu'`` (``iss_numpy``)."""
    lens = [int(c.shape[0]) for c in clouds]
    if str(device).startswith('cpu'):
        saliency, keep = iss_numpy(_host_arrays(clouds), salient_radius, non_max_radius, gamma_21, gamma_32,
                                   min_neighbors)[:2]
        return _split(saliency, lens), [np.nonzero(k)[0] for k in _split(keep, lens)]
    grid = _cloud_grid(clouds, max(float(salient_radius), float(non_max_radius)), torch.device(device))
    saliency, keep = ops.iss_keypoints(grid, None, salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors)[:2]
    return _split(saliency, lens), [torch.nonzero(k).view(-1) for k in _split(keep, lens)]


def suppress_non_maxima(clouds, scores, radius, min_neighbors=1, device='cuda'):
    """Radius non-maximum suppression of ANY per-point score over the fragments of a scene -- what a caller wraps around
    the learned detector's scores before ``select_keypoints``, whose plain top-k clusters.  ``scores``: one [n] / [n,1]
    array or tensor per fragment.  One ``ops.CloudGrid`` at ``radius`` and one ``ops.radius_nms`` call; returns the
    per-fragment keep masks (bool; device tensors, or NumPy arrays from ``device='cpu'``: ``radius_nms_numpy``)."""
    lens = [int(c.shape[0]) for c in clouds]
    if len(scores) != len(clouds) or any(int(np.prod(s.shape)) != n for s, n in zip(scores, lens)):
        raise ValueError("scores must hold one value per point of every fragment")
    if str(device).startswith('cpu'):
        flat = [np.asarray(s.detach().cpu().numpy() if isinstance(s, torch.Tensor) else s, dtype=np.float32).reshape(-1)
                for s in scores]
        return _split(radius_nms_numpy(_host_arrays(clouds), flat, radius, min_neighbors)[0], lens)
    dev = torch.device(device)
    grid = _cloud_grid(clouds, float(radius), dev)
    flat = [torch.as_tensor(s, dtype=torch.float32).reshape(-1).to(dev) for s in scores]
    score = torch.cat(flat) if flat else torch.zeros(0, dtype=torch.float32, device=dev)
    return _split(ops.radius_nms(grid, None, radius, score, min_neighbors)[0], lens)


def keypoint_repeatability(keypoints, keys_or_pairs, T, distance=0.1, device='cuda'):
    """Repeatability of a detector over the fragment pairs of a scene.  ``keypoints``: one [k_i,3] array / tensor per
    fragment, in the fragment's own frame (k_i may be 0); ``keys_or_pairs``: ``gt.log`` keys ``'i_j'`` or (i, j) tuples;
    ``T[e]`` the 4x4 ground truth that maps fragment j into fragment i.  For every pair, in BOTH directions, the number
    of keypoints of one fragment that have a keypoint of the other closer than ``distance`` after the ground-truth
    motion (strictly, ``ops.nearest_pairs``' rule; j's keypoints are moved by T[e], i's by its inverse).

    Returns ``(hits_ji, n_j, hits_ij, n_i, repeatability)``: int64 arrays over the pairs -- keypoints of j repeated in
    i, keypoints of j, and the other direction -- and the scene's relative repeatability ``sum hits / sum n`` over both
    directions.  A fragment without keypoints contributes 0 / 0 and so drops out of the sums; with no keypoint at all
    the repeatability is NaN.  One ``ops.CloudGrid`` over all keypoint sets and one ``ops.nearest_pairs`` call over the
    2P directed pairs, of which only the per-pair count is read; ``device='cpu'``: ``preprocess.nearest_pairs_numpy``.

    The evaluation script of the D3Feat paper was not at hand.  The convention taken here: both directions, and ALL
    keypoints of a fragment in the denominator, not only those that fall into the pair's overlap -- so the number is
    bounded by the overlap ratio and is comparable between detectors on the same pairs, not with the paper's table."""
    from ..datasets import preprocess as pp
    ji = _moving_fixed_pairs(keys_or_pairs, len(keypoints))                # rows (j, i): j moves into i under T
    P = ji.shape[0]
    Tji = _pose44(T, P) if P else np.zeros((0, 4, 4))
    if not (0.0 < float(distance) < np.inf):
        raise ValueError("distance must be positive and finite")
    pairs = np.concatenate([ji, ji[:, ::-1]])                              # then i moves into j under T^-1
    Ts = np.concatenate([Tji, np.linalg.inv(Tji) if P else Tji])
    lens = np.asarray([int(k.shape[0]) for k in keypoints], dtype=np.int64)
    if P == 0 or int(lens.sum()) == 0:
        count = np.zeros(2 * P, dtype=np.int64)
    elif str(device).startswith('cpu'):
        count = pp.nearest_pairs_numpy(_host_arrays([k.reshape(-1, 3) for k in keypoints]), pairs, Ts,
                                       distance)[1].astype(np.int64)
    else:
        grid = _cloud_grid(keypoints, float(distance), torch.device(device))
        count = ops.nearest_pairs(grid, None, pairs, Ts, distance)[1].cpu().numpy().astype(np.int64)
    hits_ji, hits_ij = count[:P], count[P:]
    n_j, n_i = lens[ji[:, 0]] if P else lens[:0], lens[ji[:, 1]] if P else lens[:0]
    total = int(n_j.sum() + n_i.sum())
    rep = float(hits_ji.sum() + hits_ij.sum()) / total if total else float('nan')
    return hits_ji, n_j, hits_ij, n_i, rep


def _icp_keywords(icp):
    if not isinstance(icp, dict) or 'max_distance' not in icp:
        raise ValueError("icp must be None or a dict of refine_transforms keywords with at least max_distance")
    return dict(icp)


def _moving_fixed_pairs(keys_or_pairs, num_clouds):
    """``gt.log`` keys ``'i_j'`` or (i, j) tuples -> int64 [P,2] rows (j, i) = (moving, fixed), what the ``ops`` entries
    take."""
    out = []
    for k in keys_or_pairs:
        i, j = (k.split('_') if isinstance(k, str) else k)
        out.append((int(i), int(j)))
    ij = np.asarray(out, dtype=np.int64).reshape(-1, 2)
    if ij.size and (ij.min() < 0 or ij.max() >= num_clouds):
        raise ValueError("pairs name fragments outside 0..%d" % (num_clouds - 1))
    return ij[:, ::-1].copy()


def _host_arrays(clouds):
    """The clouds (arrays or tensors) as contiguous f32 NumPy arrays."""
    return [np.ascontiguousarray(c.detach().cpu().numpy() if isinstance(c, torch.Tensor) else c, dtype=np.float32)
            for c in clouds]


def _cloud_grid(clouds, radius, dev):
    """One ``ops.CloudGrid`` at ``radius`` over the clouds stacked on ``dev``; the lengths stay known on the host."""
    pts = torch.cat([torch.as_tensor(c, dtype=torch.float32).reshape(-1, 3).to(dev) for c in clouds])
    return ops.CloudGrid(pts, np.asarray([int(c.shape[0]) for c in clouds], dtype=np.int64), float(radius))


def refine_transforms(clouds, keys_or_pairs, T, max_distance, device='cuda', estimation='point_to_point',
                      normal_radius=None, return_information=False, colors=None, lambda_geometric=LAMBDA_GEOMETRIC,
                      **icp):
    """ICP refinement of fragment-pair poses, all pairs in ONE ``ops.icp_rigid`` call over one ``ops.CloudGrid`` of the
    fragments.  ``estimation``: ``'point_to_point'``, or ``'point_to_plane'`` -- the cell list is then built at
    ``max(normal_radius, max_distance)`` (``normal_radius`` defaults to ``2 * max_distance``), the normals of all
    fragments are estimated once (``ops.estimate_normals``, viewpoint at each fragment's origin) and the fit minimises
    the point-to-plane residual: a handful of iterations from a good RANSAC pose, but it can stall on a low overlap that
    is mostly one plane and diverge from a poor start -- an option, not the default.  ``'colored'`` adds a colour term
    to that (``ops.color_gradients`` over the same cell list and radius, then the coloured ``ops.icp_rigid``) which
    holds the slide along a textured plane: ``colors`` is then required, one array / tensor per fragment -- ``[n,3]``
    RGB or ``[n,1]`` / ``[n]`` intensity, what ``intensity_of`` takes -- registered to the points; ``lambda_geometric``
    in [0, 1] weighs the geometric term (default: Open3D's 0.968, not tuned here).
    ``clouds``: list of [n,3] arrays / tensors, fragment k at index k;
    ``keys_or_pairs``: ``gt.log`` keys ``'i_j'`` or (i, j) tuples with ``T[p]`` ([P,4,4] / [P,3,4]; array or tensor)
    mapping fragment j into fragment i -- j is the moving cloud, i the fixed one.  ``icp``: ``max_iters``,
    ``rel_fitness``, ``rel_rmse`` of ``ops.icp_rigid``.  Returns ``(T [P,4,4] f64, fitness [P] = matched share of j's
    points under the returned T, rmse [P], iterations [P])``: device tensors, or NumPy arrays from ``device='cpu'``
    (``icp_numpy``).  A pair that ends with fewer than 3 matches keeps the pose it had then.
    ``return_information=True`` appends ``info [P,6,6]``, the benchmark-form information matrices of the RETURNED poses
    at ``max_distance`` (``information_matrices``): one more call on the cell list that is already built."""
    if estimation not in ('point_to_point', 'point_to_plane', 'colored'):
        raise ValueError("estimation must be 'point_to_point', 'point_to_plane' or 'colored', got %r" % (estimation,))
    colored = estimation == 'colored'
    plane = estimation == 'point_to_plane' or colored
    if colored:
        if colors is None:
            raise ValueError("estimation='colored' needs colors, one array per fragment")
        if len(colors) != len(clouds) or any(int(c.shape[0]) != int(p.shape[0]) for c, p in zip(colors, clouds)):
            raise ValueError("colors must hold one row per point of every fragment")
    if normal_radius is None:
        normal_radius = 2.0 * float(max_distance)
    ji = _moving_fixed_pairs(keys_or_pairs, len(clouds))
    lens = np.asarray([int(c.shape[0]) for c in clouds], dtype=np.int64)
    if str(device).startswith('cpu'):
        arrs = _host_arrays(clouds)
        Tn = T.detach().cpu().numpy() if isinstance(T, torch.Tensor) else T
        if plane:
            icp = dict(icp, normals=estimate_normals_numpy(arrs, normal_radius)[0])
        if colored:
            inten = np.concatenate([intensity_of(c.detach().cpu().numpy() if isinstance(c, torch.Tensor) else c)
                                    for c in colors])
            icp = dict(icp, color_field=color_gradients_numpy(arrs, normal_radius, icp['normals'], inten)[0],
                       lambda_geometric=lambda_geometric)
        Tr, count, rmse, iters = icp_numpy(arrs, ji, Tn, max_distance, **icp)[:4]
        res = (Tr, count / np.maximum(lens[ji[:, 0]], 1), rmse, iters)
        return res + (information_from_moments(information_numpy(arrs, ji, Tr, max_distance)[0]),) \
            if return_information else res
    dev = torch.device(device)
    grid = _cloud_grid(clouds, max(float(normal_radius), float(max_distance)) if plane else max_distance, dev)
    if plane:
        icp = dict(icp, normals=ops.estimate_normals(grid, None, normal_radius)[0])
    if colored:
        inten = torch.cat([torch.as_tensor(intensity_of(c)).to(dev) for c in colors])
        icp = dict(icp, color_field=ops.color_gradients(grid, None, normal_radius, icp['normals'], inten)[0],
                   lambda_geometric=lambda_geometric)
    Tr, count, rmse, iters = ops.icp_rigid(grid, None, ji, torch.as_tensor(T, dtype=torch.float64).to(dev),
                                           max_distance, **icp)[:4]
    fitness = count.double() / torch.as_tensor(np.maximum(lens[ji[:, 0]], 1), dtype=torch.float64, device=dev)
    if return_information:
        return Tr, fitness, rmse, iters, information_from_moments(ops.pair_information(grid, None, ji, Tr,
                                                                                        max_distance)[0])
    return Tr, fitness, rmse, iters


# ------------------------------------------------------------------------------------------------- information matrices
INFO_MOMENTS = 20              # ops.INFO_MOMENTS: n, sum x (3), sum x x^T (6), sum y (3), sum y y^T (6), sum d2


def information_from_moments(moments, frame='moving', order='translation_first'):
    """[P,6,6] f64 information matrices from the ``[P,20]`` raw moments of ``ops.pair_information`` /
    ``information_numpy`` (NumPy array or tensor; the result is of the same kind): sum of ``G^T G`` over the accepted
    rows with ``G = [I | -[p]x]``, i.e. ``[[n I, -[s]x], [[s]x, sum (|p|^2 I - p p^T)]]``, ``s = sum p``.
    ``frame='moving'`` takes p = x, the moving point in its own frame -- the frame ``transformation_error``'s
    ``D = inv(T_gt) T_est`` acts in, and with ``order='translation_first'`` the form of the benchmark's ``gt.info``
    (the defaults).  ``frame='fixed'`` takes p = y, the matched fixed point, and ``order='rotation_first'`` puts the
    rotation block first: together the form of Open3D's ``get_information_matrix_from_point_clouds`` -- stated from its
    formula and tested against a brute-force sum of it; Open3D itself was not available to compare with.  A pair with
    n = 0 gives zeros."""
    if frame not in ('moving', 'fixed') or order not in ('translation_first', 'rotation_first'):
        raise ValueError("frame must be 'moving' or 'fixed', order 'translation_first' or 'rotation_first'")
    tensor = isinstance(moments, torch.Tensor)
    m = moments.double() if tensor else np.asarray(moments, dtype=np.float64)
    if m.shape[-1] != INFO_MOMENTS:
        raise ValueError("moments must be [P,%d], got %s" % (INFO_MOMENTS, tuple(m.shape)))
    m = m.reshape(-1, INFO_MOMENTS)
    o = 1 if frame == 'moving' else 10
    n, sx, sy, sz = m[:, 0], m[:, o], m[:, o + 1], m[:, o + 2]
    xx, xy, xz, yy, yz, zz = (m[:, o + 3 + k] for k in range(6))
    z = torch.zeros_like(n) if tensor else np.zeros_like(n)
    rows = [[n, z, z, z, sz, -sy], [z, n, z, -sz, z, sx], [z, z, n, sy, -sx, z],
            [z, -sz, sy, yy + zz, -xy, -xz], [sz, z, -sx, -xy, xx + zz, -yz], [-sy, sx, z, -xz, -yz, xx + yy]]
    stack = torch.stack if tensor else np.stack
    info = stack([stack(r, -1) for r in rows], -2)
    if order == 'rotation_first':
        perm = [3, 4, 5, 0, 1, 2]
        info = info[:, perm][:, :, perm]
    return info


def information_numpy(clouds, pairs, T, max_distance):
    """The contract of ``ops.pair_information`` in NumPy (include/d3feat_hip.h): the search of
    ``preprocess.nearest_pairs_numpy`` and f64 sums over its accepted rows.  ``clouds``: list of [n,3] f32 arrays; pair
    p = (moving cloud a, fixed cloud b), ``T[p]`` maps a into b's frame.  Returns ``(moments f64 [P,20], count int32
    [P])``."""
    from ..datasets.preprocess import nearest_pairs_numpy, transform_points
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    T = _pose44(T, pairs.shape[0])
    arrs = [np.ascontiguousarray(c, dtype=np.float32).reshape(-1, 3) for c in clouds]
    nn, count, row_start = nearest_pairs_numpy(arrs, pairs, T, max_distance)
    moments = np.zeros((pairs.shape[0], INFO_MOMENTS), dtype=np.float64)
    iu = np.triu_indices(3)
    for p, (a, b) in enumerate(pairs):
        res = nn[row_start[p]:row_start[p + 1]]
        sel = res >= 0
        x32, y32 = arrs[a][sel], arrs[b][res[sel]]
        d = transform_points(x32, T[p]) - y32                                # f32, the kernel's d2
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        x, y = x32.astype(np.float64), y32.astype(np.float64)
        moments[p, 0] = x.shape[0]
        moments[p, 1:4], moments[p, 10:13] = x.sum(0), y.sum(0)
        moments[p, 4:10] = (x[:, iu[0]] * x[:, iu[1]]).sum(0)
        moments[p, 13:19] = (y[:, iu[0]] * y[:, iu[1]]).sum(0)
        moments[p, 19] = d2.astype(np.float64).sum()
    return moments, count


def _rmse_from_moments(moments):
    n, sd2 = moments[:, 0], moments[:, INFO_MOMENTS - 1]
    if isinstance(moments, torch.Tensor):
        return torch.where(n > 0, torch.sqrt(sd2 / n.clamp(min=1.0)), torch.zeros_like(n))
    return np.where(n > 0, np.sqrt(sd2 / np.maximum(n, 1.0)), 0.0)


def information_matrices(clouds, keys_or_pairs, T, max_distance, device='cuda', frame='moving',
                         order='translation_first'):
    """Information matrices of fragment pairs under the poses ``T``, all pairs in ONE ``ops.pair_information`` call
    over one ``ops.CloudGrid`` of the fragments.  ``clouds``, ``keys_or_pairs``, ``T``: as in ``refine_transforms`` --
    keys ``'i_j'`` or (i, j) tuples with ``T[p]`` mapping fragment j into fragment i; j is the moving cloud.  A moving
    point counts when its nearest point of i under ``T[p]`` is closer than ``max_distance``.  ``frame``, ``order``:
    ``information_from_moments`` (the defaults are the benchmark's ``gt.info`` form).  Returns ``(info [P,6,6] f64,
    count [P], rmse [P])``: device tensors, or NumPy arrays from ``device='cpu'`` (``information_numpy``)."""
    ji = _moving_fixed_pairs(keys_or_pairs, len(clouds))
    if str(device).startswith('cpu'):
        Tn = T.detach().cpu().numpy() if isinstance(T, torch.Tensor) else T
        moments, count = information_numpy(_host_arrays(clouds), ji, Tn, max_distance)
    else:
        dev = torch.device(device)
        moments, count, _ = ops.pair_information(_cloud_grid(clouds, max_distance, dev), None, ji,
                                                 torch.as_tensor(T, dtype=torch.float64).to(dev), max_distance)
    return information_from_moments(moments, frame, order), count, _rmse_from_moments(moments)


# ------------------------------------------------------------------------------------------------- gt.info, metric
def loadinfo(gtpath):
    """{'i_j': 6x6 float64} from ``<gtpath>/gt.info``: an ``i \\t j \\t n`` line, then 6 rows of 6 (like ``loadlog``)."""
    with open(os.path.join(gtpath, 'gt.info')) as f:
        rows = [ln.rstrip('\n') for ln in f if ln.strip()]
    if len(rows) % 7:
        raise ValueError("gt.info: %d non-empty lines, expected blocks of 7" % len(rows))
    out = {}
    for i in range(0, len(rows), 7):
        head = rows[i].split()[0:2]
        mat = np.array([[float(x) for x in rows[i + r].split()[0:6]] for r in range(1, 7)], dtype=np.float64)
        out['%d_%d' % (int(head[0]), int(head[1]))] = mat
    return out


def writeinfo(gtpath, info, num_frag):
    """Inverse of :func:`loadinfo`: ``{'i_j': 6x6}`` to ``<gtpath>/gt.info`` in the layout of the benchmark's files --
    per key, ordered by (i, j), an ``i \\t j \\t num_frag`` line and six rows in ``%.8e``."""
    os.makedirs(gtpath, exist_ok=True)
    with open(os.path.join(gtpath, 'gt.info'), 'w') as f:
        for key in sorted(info, key=lambda k: tuple(int(x) for x in k.split('_'))):
            a, b = key.split('_')
            mat = np.asarray(info[key], dtype=np.float64)
            if mat.shape != (6, 6):
                raise ValueError("info[%r] must be 6x6, got %s" % (key, mat.shape))
            f.write('%d\t %d\t %d\t\n' % (int(a), int(b), num_frag))
            for row in mat:
                f.write(''.join(' % .8e\t ' % v for v in row).rstrip(' ') + '\n')


def _quaternion(R):
    """Unit quaternion (w, x, y, z), w >= 0, of the active rotation R (R v = q v q*)."""
    R = np.asarray(R, dtype=np.float64)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = 2.0 * np.sqrt(tr + 1.0)
        q = np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = 2.0 * np.sqrt(1.0 + R[0, 0] - R[1, 1] - R[2, 2])
        q = np.array([(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s])
    elif R[1, 1] > R[2, 2]:
        s = 2.0 * np.sqrt(1.0 + R[1, 1] - R[0, 0] - R[2, 2])
        q = np.array([(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s])
    else:
        s = 2.0 * np.sqrt(1.0 + R[2, 2] - R[0, 0] - R[1, 1])
        q = np.array([(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s])
    q /= np.linalg.norm(q)
    return -q if q[0] < 0 else q


def transformation_error(T_est, T_gt, info):
    """The benchmark's error of an estimate: D = inv(T_gt) T_est, q = (w, x, y, z) the unit quaternion of D's rotation
    with w >= 0, er = [D_t, -q_xyz], p = er^T info er / info[0,0].

    Sign convention: q is the quaternion of D's rotation read as a direction-cosine matrix (what MATLAB's dcm2quat
    returns, the evaluation code of the benchmark), i.e. the active-rotation quaternion of D_R^T -- so for a rotation
    by +a about z, q_z = -sin(a/2) and er ends in +sin(a/2).  With the other sign the benchmark's own 3dmatch.log
    trajectories score 5-16 recall points lower on every scene (tests/test_ransac_cpu.py)."""
    D = np.linalg.inv(np.asarray(T_gt, dtype=np.float64)) @ np.asarray(T_est, dtype=np.float64)
    q = _quaternion(D[:3, :3].T)
    er = np.concatenate([D[:3, 3], -q[1:]])
    info = np.asarray(info, dtype=np.float64)
    return float(er @ info @ er / info[0, 0])


def _far(key):
    i, j = (int(x) for x in key.split('_'))
    return j - i > 1


def evaluate_registration(est, gt, info, err2=0.2 ** 2):
    """Registration recall / precision of estimates ``est`` against ``gt`` (``{'i_j': 4x4}``; ``info``: ``loadinfo``).
    Only pairs with j - i > 1 count (consecutive fragments overlap trivially).  A pair is good when it is listed in
    ``gt`` and its ``transformation_error`` is <= err2.  Returns ``(recall = good / #gt pairs, precision = good /
    #estimated pairs, {key: error})`` -- the error of every counted estimate that ``gt`` lists."""
    gt_keys = [k for k in gt if _far(k)]
    est_keys = [k for k in est if _far(k)]
    errs = {k: transformation_error(est[k], gt[k], info[k]) for k in est_keys if k in gt}
    good = sum(1 for e in errs.values() if e <= err2)
    recall = good / len(gt_keys) if gt_keys else 0.0
    precision = good / len(est_keys) if est_keys else 0.0
    return recall, precision, errs


def _scene_colors(colors, frags, rows):
    """The colours of the fragments ``frags`` (with ``rows`` points each) for ``register_scene``: ``colors`` a folder of
    ``cloud_bin_<i>.ply`` files or a sequence indexed by fragment number -> one array per fragment, in ``frags``'
    order."""
    from ..datasets.fragments import read_ply_colors
    if colors is None:
        raise ValueError("estimation='colored' needs colors: a folder of cloud_bin_<i>.ply files or per-fragment arrays")
    out = []
    for f, n in zip(frags, rows):
        if isinstance(colors, (str, os.PathLike)):
            name = os.path.join(colors, 'cloud_bin_%d.ply' % f)
            c = read_ply_colors(name) if os.path.exists(name) else None
        else:
            c = colors[f] if f < len(colors) else None
        if c is None:
            raise ValueError("fragment %d has no colours" % f)
        if int(c.shape[0]) != n:
            raise ValueError("fragment %d: %d colours for %d points" % (f, int(c.shape[0]), n))
        out.append(c)
    return out


def register_scene(save_path, scene, gtpath, num_points=5000, device='cuda', num_frag=None, out_log=None, icp=None,
                   pose_graph=None, desc_name=ev.DESC_NAME, estimator='ransac', fgr=None, sc2=None, matches=None,
                   **ransac):
    """Estimates the transform of every pair listed in ``<gtpath>/gt.log`` from the dumped keypoints / descriptors /
    scores (``evaluate``'s layout) with ONE batched ``ransac_rigid`` call, writes them with ``evaluate.writelog`` to
    ``out_log`` (a directory; default ``<save_path>/registration/<scene>``) and returns
    ``evaluate_registration(...)`` when ``<gtpath>/gt.info`` exists, else None.  ``icp``: None, or a dict of
    ``refine_transforms`` keywords (at least ``max_distance``): every pose is refined by ICP over the dumped keypoint
    files (they hold the whole subsampled fragment), all pairs in one call, before it is written and scored.  With
    ``estimation='colored'`` in that dict its ``colors`` names a folder of ``cloud_bin_<i>.ply`` files that hold one
    coloured vertex per row of fragment i's keypoint file (``fragments.write_ply_points(colors=)``; read with
    ``fragments.read_ply_colors``), or is a sequence of per-fragment colour arrays indexed by fragment number; a
    fragment without colours raises ``ValueError``.
    ``pose_graph``: None, or a dict of ``multiway_registration`` keywords (at least ``max_distance``): the information
    matrices of the estimated poses are taken (from the ICP call when ``icp`` is given, else from one
    ``information_matrices`` call over the keypoint files), ``multiway_registration`` gives one pose per fragment, and
    the log holds ``inv(P_i) P_j`` for every pair it kept -- the pairs it pruned are left out.  The return value is then
    ``(the usual result, poses [num_frag,4,4])``.  Still one read-back per scene.
    ``desc_name``: the descriptor whose dump is read (``cloud_bin_<i>.<desc_name>.npy``): ``'FPFH'`` for the files of
    ``evaluate.generate_fpfh_features``.
    ``estimator``: ``'ransac'`` (the default) or ``'fgr'``: one batched ``ops.fgr_rigid`` call on the same matches, with
    ``fgr`` a dict of its keywords (defaults: FGR_DEFAULTS); or ``'sc2'``: one batched ``ops.sc2_rigid`` call, with
    ``sc2`` a dict of its keywords (defaults: SC2_DEFAULTS, ``max_count`` = ``num_points``); everything after the pose
    estimate is the same.
    ``matches``: as in ``estimate_transform``: ``dict(k=K)`` / ``dict(ratio=r)`` replace the mutual rule by the K nearest
    neighbours / the ratio test (``ops.knn_match``), with K ``num_points`` slots per pair."""
    _check_estimator(estimator, dict(fgr=fgr, sc2=sc2), ransac)
    matches = _check_matches(matches, estimator, num_points)
    gt = ev.loadlog(gtpath)
    dpath, kpath, spath = ev._paths(save_path, scene)
    if num_frag is None:
        num_frag = len([f for f in os.listdir(kpath) if f.endswith('.npy')])
    dev = torch.device(device)
    cache = {}

    def load(i):
        if i not in cache:
            name = 'cloud_bin_%d' % i
            cache[i] = tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) for a in (
                ev.get_keypts(kpath, name), ev.get_desc(dpath, name, desc_name), ev.get_scores(spath, name).reshape(-1)))
        return cache[i]
    keys = sorted(gt, key=lambda k: tuple(int(x) for x in k.split('_')))
    if not keys:
        raise ValueError("no fragment pair is listed in %s" % os.path.join(gtpath, 'gt.log'))
    k = int(num_points) * (matches[0] if matches is not None else 1)     # slots per pair
    muts, sps, tps = [], [], []
    for key in keys:
        i, j = (int(x) for x in key.split('_'))
        mutual, sp, tp = _pair_points(*load(i), *load(j), int(num_points), matches)
        pad = k - int(mutual.shape[0])          # fragments with fewer than k points: pad with non-mutual rows
        if pad:
            mutual = torch.cat([mutual, mutual.new_zeros(pad)])
            sp = torch.cat([sp, sp.new_zeros((pad, 3))])
            tp = torch.cat([tp, tp.new_zeros((pad, 3))])
        muts.append(mutual)
        sps.append(sp)
        tps.append(tp)
    src, tgt, seg, _ = _compact(torch.stack(muts), torch.stack(sps), torch.stack(tps))
    T = _estimate(estimator, dict(fgr=fgr, sc2=sc2), src, tgt, seg, ransac, k)[0]
    frags = sorted(cache)
    slot = {f: n for n, f in enumerate(frags)}
    ij = [tuple(slot[int(x)] for x in key.split('_')) for key in keys]
    info = None
    if icp is not None:
        icp = _icp_keywords(icp)
        if icp.get('estimation') == 'colored':
            icp['colors'] = _scene_colors(icp.get('colors'), frags, [int(cache[f][0].shape[0]) for f in frags])
        res = refine_transforms([cache[f][0] for f in frags], ij, T, device=dev,
                                return_information=pose_graph is not None, **icp)
        T, info = res[0], (res[4] if pose_graph is not None else None)
    if pose_graph is None:
        T = T.cpu().numpy()                                      # the scene's only read-back
        est = {key: T[n] for n, key in enumerate(keys)}
        poses = None
    else:
        if not isinstance(pose_graph, dict) or 'max_distance' not in pose_graph:
            raise ValueError("pose_graph must be None or a dict of multiway_registration keywords with at least "
                             "max_distance")
        if info is None:
            info = information_matrices([cache[f][0] for f in frags], ij, T, pose_graph['max_distance'], device=dev)[0]
        P, kept = multiway_registration(keys, T, info, num_frag, device=dev, **pose_graph)[:2]
        i, j = (torch.as_tensor([int(k.split('_')[c]) for k in keys], device=dev) for c in (0, 1))
        rel = torch.matmul(_rigid_inverse(P[i]), P[j])
        flat = torch.cat([rel.reshape(-1), kept.double().reshape(-1), P.reshape(-1)]).cpu().numpy()   # the only read-back
        n = len(keys)
        rel, kept, poses = flat[:16 * n].reshape(n, 4, 4), flat[16 * n:17 * n] != 0, flat[17 * n:].reshape(-1, 4, 4)
        est = {key: rel[m] for m, key in enumerate(keys) if kept[m]}
    ev.writelog(out_log or os.path.join(save_path, 'registration', scene), est, num_frag)
    result = None
    if os.path.exists(os.path.join(gtpath, 'gt.info')):
        result = evaluate_registration(est, gt, loadinfo(gtpath))
    return result if pose_graph is None else (result, poses)


# ------------------------------------------------------------------------------------------------- multiway registration
def _edge_list(keys_or_pairs, num_nodes):
    """``gt.log`` keys ``'i_j'`` or (i, j) tuples -> int64 [E,2] rows (i, j), checked against ``num_nodes``."""
    out = []
    for k in keys_or_pairs:
        i, j = (k.split('_') if isinstance(k, str) else k)
        out.append((int(i), int(j)))
    ij = np.asarray(out, dtype=np.int64).reshape(-1, 2)
    if ij.size and (ij.min() < 0 or ij.max() >= num_nodes or (ij[:, 0] == ij[:, 1]).any()):
        raise ValueError("edges must join two different nodes in 0..%d" % (num_nodes - 1))
    return ij


def _rigid_inverse(T):
    """[..., 4, 4] rigid matrices (tensor or array) -> their inverses ``[R^T, -R^T t]``."""
    Rt = T[..., :3, :3].transpose(-1, -2) if isinstance(T, torch.Tensor) else np.swapaxes(T[..., :3, :3], -1, -2)
    out = T.clone() if isinstance(T, torch.Tensor) else np.array(T, dtype=np.float64)
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -(Rt @ T[..., :3, 3:4])[..., 0]
    return out


def spanning_tree(num_nodes, edges, uncertain=None):
    """The tree ``spanning_tree_poses`` composes along, decided on the host: for every component, from its lowest node,
    a breadth-first search over the CERTAIN edges (a node's edges in list order); when it runs dry, the first
    uncertain edge of the list that joins a reached node to an unreached one is taken and the search goes on from
    there.  Returns ``(parent [N] (-1 for a root), edge [N] (the edge to the parent), depth [N], root [N])``."""
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    unc = np.zeros(len(edges), dtype=bool) if uncertain is None else np.asarray(uncertain).astype(bool).reshape(-1)
    adj = [[] for _ in range(num_nodes)]
    for e, (i, j) in enumerate(edges):
        if not unc[e]:
            adj[i].append((e, j))
            adj[j].append((e, i))
    parent, via, depth, root = (np.full(num_nodes, -1, dtype=np.int64) for _ in range(4))
    loops = [e for e in range(len(edges)) if unc[e]]
    for r in range(num_nodes):
        if root[r] >= 0:
            continue
        root[r], depth[r] = r, 0
        queue = [r]
        while True:
            while queue:
                k = queue.pop(0)
                for e, m in adj[k]:
                    if root[m] < 0:
                        root[m], parent[m], via[m], depth[m] = r, k, e, depth[k] + 1
                        queue.append(m)
            for e in loops:
                i, j = edges[e]
                if (root[i] == r) != (root[j] == r) and min(root[i], root[j]) < 0:
                    k, m = (i, j) if root[i] == r else (j, i)
                    root[m], parent[m], via[m], depth[m] = r, k, e, depth[k] + 1
                    queue.append(m)
                    break
            if not queue:
                break
    return parent, via, depth, root


def spanning_tree_poses(num_nodes, keys_or_edges, T, uncertain=None):
    """Initial poses of a pose graph by composing the pair poses along ``spanning_tree``: the root (lowest node) of
    every component gets the identity and ``P_j = P_i T_ij`` (``P_i = P_j inv(T_ij)`` against the edge's direction).
    ``T`` [E,4,4]: a NumPy array gives a NumPy result; a tensor is composed in f64 on its device, one batched product
    per tree level, without a read-back (the tree itself depends on the key list alone)."""
    edges = _edge_list(keys_or_edges, num_nodes)
    parent, via, depth, _ = spanning_tree(num_nodes, edges, uncertain)
    tensor = isinstance(T, torch.Tensor)
    Z = T.double() if tensor else torch.as_tensor(np.asarray(T, dtype=np.float64))
    if tuple(Z.shape) != (len(edges), 4, 4):
        raise ValueError("T must be [E,4,4] for the %d edges, got %s" % (len(edges), tuple(Z.shape)))
    P = torch.eye(4, dtype=torch.float64, device=Z.device).repeat(num_nodes, 1, 1)
    if len(edges):
        step = torch.stack([Z, _rigid_inverse(Z)])                       # [2,E,4,4]: along / against the edge
        for level in range(1, int(depth.max()) + 1):
            kids = np.nonzero(depth == level)[0]
            against = (edges[via[kids], 0] == kids).astype(np.int64)     # the child is the edge's i
            idx = lambda a: torch.as_tensor(a, device=Z.device)
            P[idx(kids)] = torch.matmul(P[idx(parent[kids])], step[idx(against), idx(via[kids])])
    return P if tensor else P.numpy()


def _so3_log_numpy(R):
    """Rotation vector of R by the angle-axis formulas (not the kernel's quaternion route)."""
    c = min(1.0, max(-1.0, (np.trace(R) - 1.0) / 2.0))
    theta = np.arccos(c)
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    if theta < 1e-7:
        return v / 2.0
    if theta < np.pi - 1e-3:
        return v * (theta / (2.0 * np.sin(theta)))
    B = (R + np.eye(3)) / 2.0                                            # ~ a a^T near pi
    a = B[:, np.argmax(np.diag(B))].copy()
    a /= np.linalg.norm(a)
    if a @ v < 0:
        a = -a
    return a * theta


def _hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def _exp_numpy(d):
    """Exp([v, w]) = [[R(w), v], [0, 1]] by Rodrigues' formula."""
    w = d[3:]
    theta = np.linalg.norm(w)
    K = _hat(w)
    if theta < 1e-6:
        R = np.eye(3) + K + K @ K / 2.0
    else:
        R = np.eye(3) + np.sin(theta) / theta * K + (1.0 - np.cos(theta)) / theta ** 2 * K @ K
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = R, d[:3]
    return out


def pose_graph_edge_numpy(Pi, Pj, Z, L):
    """One edge of the pose graph in NumPy: ``(r [6], cost, Ji [6,6], Jj [6,6])`` -- ``D = inv(Z) inv(Pi) Pj``,
    ``r = [D_t ; log(D_R)]``, ``Jj = diag(D_R, Jr^-1(phi))``, ``Ji = -Jj Ad(inv(M))`` with ``M = inv(Pi) Pj``
    (include/d3feat_hip.h)."""
    M = _rigid_inverse(np.asarray(Pi, dtype=np.float64)) @ Pj
    D = _rigid_inverse(np.asarray(Z, dtype=np.float64)) @ M
    phi = _so3_log_numpy(D[:3, :3])
    r = np.concatenate([D[:3, 3], phi])
    theta = np.linalg.norm(phi)
    K = _hat(phi)
    C = 1.0 / 12.0 + theta ** 2 / 720.0 if theta < 1e-3 else (1.0 - 0.5 * theta / np.tan(0.5 * theta)) / theta ** 2
    Jj = np.zeros((6, 6))
    Jj[:3, :3], Jj[3:, 3:] = D[:3, :3], np.eye(3) + 0.5 * K + C * K @ K
    Ad = np.zeros((6, 6))
    Ad[:3, :3] = Ad[3:, 3:] = M[:3, :3].T
    Ad[:3, 3:] = -M[:3, :3].T @ _hat(M[:3, 3])
    return r, float(r @ L @ r), -Jj @ Ad, Jj


def _components_numpy(N, edges, active):
    label = np.arange(N)

    def find(k):
        while label[k] != k:
            label[k] = label[label[k]]
            k = label[k]
        return k
    for e in np.nonzero(active)[0]:
        a, b = find(edges[e, 0]), find(edges[e, 1])
        if a != b:
            label[max(a, b)] = min(a, b)
    return np.array([find(k) for k in range(N)], dtype=np.int32)


def _pose_graph_one(P, edges, Z, L, unc, max_distance, preference, prune_threshold, max_iters, step_tol, rel_cost):
    """One graph of ``pose_graph_numpy``."""
    N, E = len(P), len(edges)
    P = P.copy()
    weight, pruned = np.zeros(E), np.zeros(E, dtype=np.int32)
    iterations, cost, status = np.zeros(2, dtype=np.int32), np.zeros(3), 0
    component = np.arange(N, dtype=np.int32)
    bad = 0
    if not np.isfinite(P[:, :3]).all() or not np.isfinite(Z[:, :3]).all():
        bad |= PG_ST_NONFINITE
    if E and (edges.min() < 0 or edges.max() >= N or (edges[:, 0] == edges[:, 1]).any()):
        bad |= PG_ST_GRAPH
    active = np.array([np.isfinite(L[e]).all() and L[e, 0, 0] > 0 for e in range(E)], dtype=bool)
    pruned[~active] = 1
    if bad:
        return P, weight, pruned, component, iterations, cost, bad

    def energy_of(Q, mu):
        total, costs = 0.0, np.zeros(E)
        for e in np.nonzero(active)[0]:
            D = _rigid_inverse(Z[e]) @ _rigid_inverse(Q[edges[e, 0]]) @ Q[edges[e, 1]]
            r = np.concatenate([D[:3, 3], _so3_log_numpy(D[:3, :3])])
            costs[e] = r @ L[e] @ r
            total += mu * costs[e] / (mu + costs[e]) if unc[e] else costs[e]
        return total, costs

    for p in range(2):
        component = _components_numpy(N, edges, active)
        fixed = component == np.arange(N)
        live = np.nonzero(active)[0]
        mu = preference * max_distance ** 2 * L[live, 0, 0].mean() if live.size else 0.0
        energy, costs = energy_of(P, mu)
        if p == 0:
            cost[0] = energy
        lam, it, ended, system = PG_LAMBDA0, 0, live.size == 0, None
        while not ended and it < max_iters:
            if system is None:
                H, g = np.zeros((6 * N, 6 * N)), np.zeros(6 * N)
                for e in live:
                    i, j = edges[e]
                    r, c, Ji, Jj = pose_graph_edge_numpy(P[i], P[j], Z[e], L[e])
                    l = (mu / (mu + c)) ** 2 if unc[e] else 1.0
                    J = np.zeros((6, 6 * N))
                    J[:, 6 * i:6 * i + 6], J[:, 6 * j:6 * j + 6] = Ji, Jj
                    H += l * J.T @ L[e] @ J
                    g += l * J.T @ L[e] @ r
                for k in np.nonzero(fixed)[0]:
                    H[6 * k:6 * k + 6, :] = 0.0
                    H[:, 6 * k:6 * k + 6] = 0.0
                    H[6 * k:6 * k + 6, 6 * k:6 * k + 6] = np.eye(6)
                    g[6 * k:6 * k + 6] = 0.0
                system = (H, g)
            H, g = system
            it += 1
            A = H + lam * np.diag(np.diag(H))
            try:
                np.linalg.cholesky(A)
            except np.linalg.LinAlgError:
                lam *= 10.0
                if lam > PG_LAMBDA_MAX:
                    status |= PG_ST_INDEFINITE
                    ended = True
                continue
            d = -np.linalg.solve(A, g)
            maxd = np.abs(d).max()
            Q = P.copy()
            for k in np.nonzero(~fixed)[0]:
                Q[k] = P[k] @ _exp_numpy(d[6 * k:6 * k + 6])
            trial, trial_costs = energy_of(Q, mu)
            if trial < energy:
                P, costs, system = Q, trial_costs, None
                if maxd <= step_tol or energy - trial <= rel_cost * energy:
                    ended = True
                energy = trial
                lam = max(lam / 10.0, PG_LAMBDA_MIN)
            else:
                if maxd <= step_tol:
                    ended = True
                lam *= 10.0
                if lam > PG_LAMBDA_MAX:
                    ended = True
        if not ended:
            status |= PG_ST_ITER_CAP
        for e in live:
            weight[e] = (mu / (mu + costs[e])) ** 2 if unc[e] else 1.0
            if p == 0 and unc[e] and weight[e] < prune_threshold:
                active[e], pruned[e] = False, 1
        iterations[p], cost[1 + p] = it, energy
    return P, weight, pruned, component, iterations, cost, status


def pose_graph_numpy(poses, edges, T, info, uncertain, max_distance, node_start=None, edge_start=None,
                     preference_loop_closure=2.0, prune_threshold=0.25, max_iters=100, step_tol=1e-9, rel_cost=1e-9):
    """The contract of ``ops.pose_graph_optimize`` in NumPy f64 (include/d3feat_hip.h): the ``device='cpu'`` path of
    ``multiway_registration`` and the oracle of the tests.  It shares no code with the kernel: union-find components, a
    Python loop over the edges, dense ``numpy.linalg`` factorisation and solve, the rotation logarithm by the
    angle-axis formulas.  Arguments and the returned tuple ``(poses, weight, pruned, component, iterations, cost,
    status)`` are those of ``ops.pose_graph_optimize``, as NumPy arrays."""
    P = np.array(poses, dtype=np.float64).reshape(-1, 4, 4)
    edges = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    Z = np.asarray(T, dtype=np.float64).reshape(-1, 4, 4)
    L = np.asarray(info, dtype=np.float64).reshape(-1, 6, 6)
    unc = np.asarray(uncertain).astype(bool).reshape(-1)
    ns = np.asarray([0, len(P)] if node_start is None else node_start, dtype=np.int64)
    es = np.asarray([0, len(edges)] if edge_start is None else edge_start, dtype=np.int64)
    outs = [_pose_graph_one(P[ns[g]:ns[g + 1]], edges[es[g]:es[g + 1]], Z[es[g]:es[g + 1]], L[es[g]:es[g + 1]],
                            unc[es[g]:es[g + 1]], float(max_distance), float(preference_loop_closure),
                            float(prune_threshold), int(max_iters), float(step_tol), float(rel_cost))
            for g in range(len(ns) - 1)]
    cat = lambda k, shape, dt: np.concatenate([o[k] for o in outs]) if outs else np.zeros(shape, dtype=dt)
    return (cat(0, (0, 4, 4), np.float64), cat(1, (0,), np.float64), cat(2, (0,), np.int32), cat(3, (0,), np.int32),
            np.stack([o[4] for o in outs]).astype(np.int32) if outs else np.zeros((0, 2), dtype=np.int32),
            np.stack([o[5] for o in outs]) if outs else np.zeros((0, 3)),
            np.array([o[6] for o in outs], dtype=np.int32))


def multiway_registration(keys_or_pairs, T, info, num_nodes, max_distance, uncertain=None, init=None, device='cuda',
                          **options):
    """One consistent pose per fragment from the pair poses of a scene: robust pose-graph optimisation
    (``ops.pose_graph_optimize``, ONE launch; ``device='cpu'``: ``pose_graph_numpy``) that switches off and prunes the
    false loop closures.

    ``keys_or_pairs``: ``gt.log`` keys ``'i_j'`` or (i, j) tuples; ``T`` [E,4,4] maps fragment j into fragment i (what
    ``ransac_rigid`` / ``refine_transforms`` return); ``info`` [E,6,6] their information matrices in the default form
    of ``information_from_moments`` (``refine_transforms(..., return_information=True)``), computed at
    ``max_distance``; ``num_nodes`` fragments.  ``uncertain`` [E]: the edges the line process may switch off; None
    takes ``|j - i| > 1``, the benchmark's rule for "not consecutive".  ``init`` [N,4,4]: initial poses; None takes
    ``spanning_tree_poses``.  ``options``: ``preference_loop_closure``, ``prune_threshold``, ``max_iters``,
    ``step_tol``, ``rel_cost`` of ``ops.pose_graph_optimize``.

    Returns ``(poses [N,4,4] f64 -- fragment k into the frame of the lowest fragment of its component --, kept [E]
    bool, weight [E], component [N], status)``: device tensors (``status`` [1]), or NumPy arrays from ``device='cpu'``.
    ``inv(poses[i]) @ poses[j]`` is the consistent pose of a kept pair.  A false edge that is the ONLY link between two
    parts of the graph (a bridge) contradicts nothing and cannot be detected: it is kept."""
    edges = _edge_list(keys_or_pairs, num_nodes)
    unc = np.abs(edges[:, 1] - edges[:, 0]) > 1 if uncertain is None else np.asarray(
        uncertain.cpu() if isinstance(uncertain, torch.Tensor) else uncertain).astype(bool).reshape(-1)
    if unc.shape[0] != edges.shape[0]:
        raise ValueError("uncertain must hold one flag per edge")
    if str(device).startswith('cpu'):
        Tn, Ln = (np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
                  for a in (T, info))
        P0 = spanning_tree_poses(num_nodes, edges, Tn, unc) if init is None else np.asarray(
            init.detach().cpu().numpy() if isinstance(init, torch.Tensor) else init, dtype=np.float64)
        P, weight, pruned, component, _, _, status = pose_graph_numpy(P0, edges, Tn, Ln, unc, max_distance, **options)
        return P, pruned == 0, weight, component, status
    dev = torch.device(device)
    Td, Ld = (torch.as_tensor(a, dtype=torch.float64).to(dev) for a in (T, info))
    P0 = spanning_tree_poses(num_nodes, edges, Td, unc) if init is None else torch.as_tensor(
        init, dtype=torch.float64).to(dev)
    P, weight, pruned, component, _, _, status = ops.pose_graph_optimize(P0, edges, Td, Ld, unc, max_distance,
                                                                         **options)
    return P, pruned == 0, weight, component, status


# ------------------------------------------------------------------------------------------------- gt.log / gt.info
MAX_PAIRS = 65535              # pairs per ops.pair_information call


def _job_chunks(units, rows_of, max_rows):
    """``preprocess._chunks`` with the call's pair cap on top: consecutive groups of units of at most ``max_rows``
    moving rows and ``MAX_PAIRS`` jobs, one unit at least."""
    from ..datasets.preprocess import _chunks
    out = []
    for chunk in _chunks(units, rows_of, max_rows):
        cur, n = [], 0
        for u in chunk:
            if cur and n + len(u) > MAX_PAIRS:
                out.append(cur)
                cur, n = [], 0
            cur.append(u)
            n += len(u)
        out.append(cur)
    return out


def build_benchmark(fragments, poses, out_dir, voxel, radius=None, min_overlap=0.3, info_distance=None,
                    symmetric=False, device='cuda', max_rows=1 << 23, subsample=None):
    """Writes ``gt.log`` and ``gt.info`` of ONE scene into ``out_dir`` from raw fragments with poses -- the two files
    ``register_scene(save_path, scene, gtpath=out_dir)`` and ``evaluate_registration`` score registration recall with.

    The benchmark ships these files for its eight test scenes only and no code that makes them, so the rule is stated
    here rather than copied, as ``datasets/preprocess.py`` states the rule of the training pickles: ``fragments`` (a
    list of [N,3] arrays in their own frames) are voxel-subsampled at ``voxel`` (``preprocess.subsample_fragments``;
    ``voxel=None`` takes them as they are), ``poses`` [F,4,4] f64 map fragment to world.  Candidates are the pairs
    i < j of ``preprocess.candidate_pairs``.  For the key ``i_j``, ``T = inv(P_i) @ P_j`` maps j into i: j is the
    MOVING cloud, i the fixed one.  The OVERLAP of ``i_j`` is the share of j's points whose nearest point of i under T
    is closer than ``radius`` (default ``1.25 * voxel``, the training pickles' rule); with ``symmetric=True`` the
    direction i into j is searched too and the larger share decides.  Pairs whose overlap exceeds ``min_overlap`` (and
    that have a correspondence in the direction j into i) are kept.  The information matrix of a kept pair is the
    benchmark's form (``information_from_moments`` defaults) over the correspondences at ``info_distance`` (default
    ``radius``: one ``ops.pair_information`` call then serves both the overlap and the matrices).  Calls hold at most
    ``max_rows`` moving rows and 65535 pairs; a pair's result does not depend on the chunking.  ``device='cpu'`` is the
    NumPy path (``information_numpy``).

    Files made here follow THIS rule; they are not claimed to equal the benchmark's download, whose fragments are not
    available to compare against (its blocks hold at most 5000 points each, whatever sampling produced that).

    Returns ``(gt {'i_j': 4x4}, info {'i_j': 6x6}, overlap {'i_j': share})``; ``overlap`` lists every candidate."""
    from ..datasets.preprocess import _by_fixed_cloud, _directed_jobs, candidate_pairs, subsample_fragments
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
    if poses.shape[0] != len(fragments):
        raise ValueError("%d poses for %d fragments" % (poses.shape[0], len(fragments)))
    if radius is None:
        if voxel is None:
            raise ValueError("radius is required when voxel is None")
        radius = 1.25 * voxel
    radius = float(radius)
    info_distance = radius if info_distance is None else float(info_distance)
    clouds = subsample_fragments(fragments, voxel, subsample, device)
    lens = np.array([c.shape[0] for c in clouds], dtype=np.int64)
    ij, T_ij = candidate_pairs(clouds, poses, max(radius, info_distance))     # T_ij maps i into j
    # jobs (moving, fixed, T): j into i for every candidate and, when symmetric, i into j right behind it
    T_ji = [np.linalg.inv(poses[i]) @ poses[j] for i, j in ij]
    job_pairs, job_T, units, rows_of = _directed_jobs(ij[:, ::-1], T_ji, lens, symmetric, T_back=T_ij)
    on_cpu = str(device).startswith('cpu')
    grid = None
    if not on_cpu and len(job_pairs):
        grid = _cloud_grid(clouds, max(radius, info_distance), torch.device(device))

    def search(jobs, distance):
        """(moments [len(jobs),20], count) of the listed jobs, in chunks."""
        moments = np.zeros((len(jobs), INFO_MOMENTS))
        count = np.zeros(len(jobs), dtype=np.int64)
        at = {j: k for k, j in enumerate(jobs)}
        for chunk in _job_chunks(_by_fixed_cloud([[j] for j in jobs], job_pairs), rows_of, int(max_rows)):
            js = [u[0] for u in chunk]
            if on_cpu:
                m, c = information_numpy(clouds, job_pairs[js], job_T[js], distance)
            else:
                m, c, st = (t.cpu().numpy() for t in ops.pair_information(grid, None, job_pairs[js], job_T[js],
                                                                          distance))
                if st.any():
                    raise RuntimeError("pair_information flagged pairs %s with status %s"
                                       % (job_pairs[js][st != 0].tolist(), st[st != 0].tolist()))
            where = [at[j] for j in js]
            moments[where], count[where] = m, c
        return moments, count

    moments, count = search(list(range(len(job_pairs))), radius)
    share = count / np.maximum(rows_of, 1)
    gt, overlap, kept = {}, {}, []
    for u in units:
        j, i = (int(v) for v in job_pairs[u[0]])
        key = '%d_%d' % (i, j)
        overlap[key] = float(max(share[k] for k in u))
        if overlap[key] > min_overlap and count[u[0]] > 0:
            gt[key] = job_T[u[0]]
            kept.append(u[0])
    if info_distance != radius and kept:
        moments_kept = search(kept, info_distance)[0]
    else:
        moments_kept = moments[kept]
    if grid is not None:
        grid.status.raise_if_set()
    mats = information_from_moments(moments_kept.reshape(-1, INFO_MOMENTS))
    info = {'%d_%d' % (int(job_pairs[k, 1]), int(job_pairs[k, 0])): mats[n] for n, k in enumerate(kept)}
    ev.writelog(out_dir, gt, len(fragments))
    writeinfo(out_dir, info, len(fragments))
    return gt, info, overlap


def build_benchmark_files(root, scene, out_dir, voxel, **kw):
    """``build_benchmark`` over ``<root>/fragments/<scene>`` (``preprocess.read_scene``: ``cloud_bin_<i>.ply`` with
    ``poses.npy`` or ``cloud_bin_<i>.info.txt``).  The keys of the files are fragment numbers, so the folder must hold
    ``cloud_bin_0 .. cloud_bin_<F-1>`` without a gap.  The files follow ``build_benchmark``'s rule and are not claimed
    to equal the benchmark's download."""
    from ..datasets.preprocess import read_scene
    ids, points, poses = read_scene(root, scene)
    numbers = [int(i.rsplit('_', 1)[1]) for i in ids]
    if numbers != list(range(len(ids))):
        raise ValueError("%s: the fragments must be numbered 0..%d without a gap" % (scene, len(ids) - 1))
    return build_benchmark(points, poses, out_dir, voxel, **kw)
