"""Fixtures of the ISS tests (test_iss_cpu.py, test_iss_gpu.py): the two terrain fragments of fpfh_cases.scene(5) with
brute-force moments, an n x n statement of the suppression, the hand-written score cases with their expected rows, and a
brute-force repeatability count.  Everything is computed once and handed out read-only."""
import functools

import numpy as np

import fpfh_cases as fc
from d3feat_pytorch_amd.geometric_registration import registration as reg

SEED = 5
R_SALIENT, R_NMS = 0.15, 0.10
G21 = G32 = 0.975
MIN_NEIGHBORS = 5
GAP = 1e-9          # a gate ratio closer than this to its threshold may fall either way (measured on the oracle)
MAX_ULP = 2         # two f64 eigenvalues with an absolute error of order 1e-16 e1, each cast to f32 once


def brute_moments(p, radius):
    """int64 [n,10]: the moments of include/d3feat_hip.h for one f32 cloud by an n x n computation."""
    p = np.ascontiguousarray(p, dtype=np.float32)
    e = p[:, None, :] - p[None, :, :]                                  # the search's p_i - p_j
    d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    inside = d2 < np.float32(radius) * np.float32(radius)
    d = p[None, :, :] - p[:, None, :]                                  # p_j - p_i: one f32 subtraction
    u = np.rint(d.astype(np.float64) * reg.normals_scale(radius)).astype(np.int64) * inside[..., None]
    cols = [inside.sum(1)] + [u[..., k].sum(1) for k in range(3)]
    cols += [(u[..., a] * u[..., b]).sum(1) for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))]
    return np.stack(cols, 1).astype(np.int64)


def brute_nms(p, score, radius, min_neighbors=1):
    """(keep bool [n], count int32 [n]) of ONE cloud by an n x n computation, written from the contract."""
    p = np.ascontiguousarray(p, dtype=np.float32)
    s = np.asarray(score, dtype=np.float32).reshape(-1)
    e = p[:, None, :] - p[None, :, :]
    d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    inside = d2 < np.float32(radius) * np.float32(radius)
    with np.errstate(invalid='ignore'):
        walks = s > 0
        beaten = (inside & (s[None, :] > s[:, None])).any(1)
    count = np.where(walks, inside.sum(1), 0).astype(np.int32)
    return walks & ~beaten & (count >= min_neighbors), count


def ulps(a, b):
    """Distance of two f32 arrays of non-negative finite values in units in the last place."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def near_threshold(moments, Q, g21=G21, g32=G32):
    """bool [n]: rows one of whose gate ratios e2 / e1, e3 / e2 (``eigvalsh``) lies within GAP of its threshold."""
    e = reg.iss_eigenvalues_numpy(moments, Q)
    with np.errstate(all='ignore'):
        return (np.abs(e[:, 1] / e[:, 0] - g21) <= GAP) | (np.abs(e[:, 2] / e[:, 1] - g32) <= GAP)


@functools.lru_cache(maxsize=None)
def fixture():
    """(clouds, moments int64 [N,10], saliency f32 [N], keep bool [N], count_nms int32 [N]): the fragments, their
    brute-force moments at R_SALIENT, the restatement's saliency of them and the brute-force suppression of it at R_NMS."""
    clouds = fc.scene(SEED)[0]
    moments = np.concatenate([brute_moments(c, R_SALIENT) for c in clouds])
    saliency = reg.iss_saliency_numpy(moments, reg.normals_scale(R_SALIENT), G21, G32, MIN_NEIGHBORS)
    keep, count, lo = [], [], 0
    for c in clouds:
        k, n = brute_nms(c, saliency[lo:lo + len(c)], R_NMS, MIN_NEIGHBORS)
        keep.append(k)
        count.append(n)
        lo += len(c)
    out = (moments, saliency, np.concatenate(keep), np.concatenate(count))
    for a in out:
        a.setflags(write=False)
    return (clouds,) + out


def hand_case():
    """(points f32 [7,3], score f32 [7], radius, {min_neighbors: (keep, count)}) worked out by hand at radius 0.1:
    rows 0 and 1 tie at the top of their neighbourhood (0.04 apart) and both survive; row 2 (0.08 from row 0) is beaten;
    row 3 is a NaN 0.08 from row 2: never kept, not searched, and it beats nobody -- row 4, 0.04 from it and 0.12 from
    row 2, is kept with count 2; row 5 is alone: kept at min_neighbors 1, dropped at 2; row 6 has score 0: not searched,
    but it counts in the neighbourhoods of rows 0, 1 and 2 (0.057, 0.04, 0.057 away)."""
    p = np.float32([[0, 0, 0], [0.04, 0, 0], [0.08, 0, 0], [0.16, 0, 0], [0.2, 0, 0], [5, 5, 5], [0.04, 0.04, 0]])
    s = np.float32([2.0, 2.0, 1.0, np.nan, 0.5, 0.1, 0.0])
    count = np.int32([4, 4, 5, 0, 2, 1, 0])
    return p, s, 0.1, {1: (np.array([1, 1, 0, 0, 1, 1, 0], dtype=bool), count),
                       2: (np.array([1, 1, 0, 0, 1, 0, 0], dtype=bool), count)}


def brute_hits(a, b, T, distance):
    """The number of rows of the f32 keypoints ``b`` that, moved by the 4x4 ``T`` (``preprocess.transform_points``'
    rounding), have a row of ``a`` closer than ``distance`` (f32 rule, strict)."""
    from d3feat_pytorch_amd.datasets import preprocess as pp
    if len(a) == 0 or len(b) == 0:
        return 0
    q = pp.transform_points(b, T)
    e = q[:, None, :] - np.asarray(a, dtype=np.float32)[None, :, :]
    d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    return int((d2 < np.float32(distance) * np.float32(distance)).any(1).sum())


def brute_repeatability(keypoints, keys, T, distance):
    """(hits_ji, n_j, hits_ij, n_i, repeatability) of registration.keypoint_repeatability by n x n counts."""
    hji, nj, hij, ni = [], [], [], []
    for key, G in zip(keys, T):
        i, j = (int(x) for x in key.split('_'))
        hji.append(brute_hits(keypoints[i], keypoints[j], G, distance))
        hij.append(brute_hits(keypoints[j], keypoints[i], np.linalg.inv(G), distance))
        nj.append(len(keypoints[j]))
        ni.append(len(keypoints[i]))
    total = sum(nj) + sum(ni)
    rep = (sum(hji) + sum(hij)) / total if total else float('nan')
    return np.int64(hji), np.int64(nj), np.int64(hij), np.int64(ni), rep


def thin_fragments(n=1000):
    """The first n rows of each fragment: enough neighbours at R_SALIENT for a handful of keypoints, small enough for
    the NumPy FPFH restatement."""
    return [np.array(c[:n]) for c in fc.scene(SEED)[0]]
