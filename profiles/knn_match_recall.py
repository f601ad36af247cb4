"""What each matching rule hands the pose estimator on FPFH descriptors -- NOT a device measurement: everything here is
the NumPy restatements on the CPU (reg.fpfh_numpy, reg.knn_match_numpy, reg.sc2_numpy), and no test takes a threshold
from it.  Writes profiles/knn_match_recall.txt (--out).

    python profiles/knn_match_recall.py [--out profiles/knn_match_recall.txt]

Data: the terrain fragment pairs of tests/fpfh_cases.py (seeds 5 and 6; two overlapping fragments of a bumpy terrain,
FPFH at 0.2 m, unit rows).  Source keypoints: the rows of fragment 0 with a descriptor, every second one when there
are more than SC2_MAX_COUNT / 3 of them (so that k = 3 fits the estimator); targets: all rows of fragment 1 with a descriptor.
Per rule: the number of correspondences, how many lie within 0.05 m of their true partner, and whether reg.sc2_numpy
(defaults) recovers the pose within 1 degree and 5 cm.
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
import d3feat_pytorch_amd  # noqa: E402,F401
import fpfh_cases as fc  # noqa: E402
import icp_scene  # noqa: E402
from d3feat_pytorch_amd.geometric_registration import registration as reg  # noqa: E402

RULES = (('mutual', None), ('k=1', dict(k=1)), ('k=3', dict(k=3)), ('ratio=0.9', dict(ratio=0.9)),
         ('ratio=0.8', dict(ratio=0.8)))


def correspondences(S, T, rule):
    """(source rows, target rows) of the rule, as registration._pair_points keeps them."""
    if rule is None:
        row = reg.knn_match_numpy(S, T, 1)[0][:, 0]
        col = reg.knn_match_numpy(T, S, 1)[0][:, 0]
        keep = col[row] == np.arange(len(S))
        return np.nonzero(keep)[0], row[keep]
    if 'ratio' in rule:
        idx, dist = reg.knn_match_numpy(S, T, 2)
        keep = (idx[:, 1] >= 0) & (dist[:, 0] < np.float32(rule['ratio']) * dist[:, 1])
        return np.nonzero(keep)[0], idx[keep, 0]
    idx = reg.knn_match_numpy(S, T, rule['k'])[0]
    return np.repeat(np.arange(len(S)), rule['k']), idx.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'knn_match_recall.txt'))
    a = ap.parse_args()
    lines = ["knn_match_recall.py: NOT a device measurement -- NumPy restatements on the CPU, terrain pairs of "
             "tests/fpfh_cases.py, FPFH unit rows at %.2f m" % fc.R_FPFH,
             "inliers: correspondences within 0.05 m of the true partner; pose: reg.sc2_numpy at its defaults, recovered "
             "= within 1 degree and 0.05 m", ""]
    for seed in fc.SEEDS:
        clouds, poses, _, _ = fc.scene(seed)
        _, count, _, desc = fc.restated(seed)
        na = len(clouds[0])
        si = np.nonzero(count[:na] > 0)[0]
        if len(si) > reg.SC2_MAX_COUNT // 3:
            si = si[::2]
        ti = np.nonzero(count[na:] > 0)[0]
        S, T = np.ascontiguousarray(desc[:na][si]), np.ascontiguousarray(desc[na:][ti])
        G = icp_scene.gt_transform(poses, 0, 1)
        lines.append("seed %d: %d source keypoints, %d target keypoints" % (seed, len(si), len(ti)))
        for name, rule in RULES:
            r, c = correspondences(S, T, rule)
            src, tgt = clouds[0][si][r], clouds[1][ti][c]
            moved = tgt.astype(np.float64) @ G[:3, :3].T + G[:3, 3]
            inl = int((np.linalg.norm(src - moved, axis=1) < 0.05).sum())
            if len(r) >= 3:
                Tm = reg.sc2_numpy(src, tgt, np.array([[0, len(r)]]), max_count=len(r), **reg.SC2_DEFAULTS)[0][0]
                R = Tm[:3, :3].T @ G[:3, :3]
                rot = np.degrees(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0)))
                tr = np.linalg.norm(Tm[:3, 3] - G[:3, 3])
                pose = "rot %.3f deg, trans %.4f m: %s" % (rot, tr, "recovered" if rot < 1.0 and tr < 0.05 else "NOT recovered")
            else:
                pose = "fewer than 3 correspondences"
            lines.append("  %-10s %6d correspondences, %5d inliers (%5.1f %%)   %s"
                         % (name, len(r), inl, 100.0 * inl / max(len(r), 1), pose))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    with open(a.out, 'w') as fh:
        fh.write(text + "\n")


if __name__ == '__main__':
    main()
