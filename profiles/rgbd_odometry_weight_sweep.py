"""Chooses ops.ODO_PHOTO_WEIGHT: runs the NumPy restatement of the RGB-D odometry (ops.rgbd_odometry_numpy, CPU only)
over the photometric weights {0.01, 0.03, 0.1, 0.3, 1.0} on the two scenes of tests/rgbd_cases.py and writes the table

    python profiles/rgbd_odometry_weight_sweep.py [--out profiles/rgbd_odometry_weight_sweep.txt]

* planar slide -- two pairs of 64 x 48 views of the plane z = 1 (depth-only: singular).  Condition: status 0 and the
  final error within a tenth of the starting error (pair 1: 0.1 deg / 1.39 mm; pair 2 starts with no rotation error and
  takes pair 1's 0.1 deg).
* textured room -- the 11 consecutive pairs of the 80 x 60 room.  Condition: every status 0 and no pair further from the
  analytic pose than twice the worst pair of ops.depth_odometry_numpy on the same frames, in degrees and in millimetres.
The default is the largest weight that meets both.
"""
import argparse
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import d3feat_pytorch_amd  # noqa: E402,F401
from d3feat_pytorch_amd import ops  # noqa: E402
import odometry_cases as OC  # noqa: E402
import rgbd_cases as RC  # noqa: E402

WEIGHTS = (0.01, 0.03, 0.1, 0.3, 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    sd, sK, si, sp, sT = RC.slide()
    slide_pyr = ops.rgbd_pyramid_numpy(sd, si, sK, RC.LEVELS)
    start = np.array([OC.pose_error(np.eye(4), T) for T in sT])
    bound = np.stack([np.full(2, start[0, 0] / 10.0), start[:, 1] / 10.0], axis=1)
    depth, K, _, inten, _ = RC.room()
    pairs, T_true = OC.room_pairs()
    room_pyr = ops.rgbd_pyramid_numpy(depth, inten, K, RC.LEVELS)
    Td = ops.depth_odometry_numpy(room_pyr, pairs)[0]
    worst = np.array([OC.pose_error(Td[p], T_true[p]) for p in range(len(pairs))]).max(axis=0)
    say("# python profiles/rgbd_odometry_weight_sweep.py  (ops.rgbd_odometry_numpy, iterations %s)" % (ops.ODO_ITERATIONS,))
    say("slide: starts %.3f deg / %.2f mm and %.3f deg / %.2f mm off; bounds %.3f deg / %.3f mm and %.3f deg / %.3f mm"
        % (start[0, 0], start[0, 1], start[1, 0], start[1, 1], bound[0, 0], bound[0, 1], bound[1, 0], bound[1, 1]))
    say("room: depth-only worst pair %.4f deg / %.4f mm; bound twice that" % (worst[0], worst[1]))
    say("%8s | %-44s | %-34s | %s" % ("weight", "slide: status, deg / mm of pair 1, pair 2", "room: statuses != 0, worst deg / mm",
                                      "meets both"))
    best = None
    for w in WEIGHTS:
        T, _, _, st, n_photo = ops.rgbd_odometry_numpy(slide_pyr, sp, photo_weight=w)
        e = np.array([OC.pose_error(T[p], sT[p]) for p in range(2)])
        ok_slide = bool((st == 0).all() and (e < bound).all())
        Tr, _, _, sr, _ = ops.rgbd_odometry_numpy(room_pyr, pairs, photo_weight=w)
        er = np.array([OC.pose_error(Tr[p], T_true[p]) for p in range(len(pairs))]).max(axis=0)
        ok_room = bool((sr == 0).all() and (er <= 2.0 * worst).all())
        say("%8.2f | %s  %.4f / %.4f  %.4f / %.4f %s | %d  %.4f / %.4f %s | %s" % (
            w, [int(x) for x in st], e[0, 0], e[0, 1], e[1, 0], e[1, 1], "ok " if ok_slide else "NO ", int((sr != 0).sum()), er[0],
            er[1], "ok " if ok_room else "NO ", "yes" if ok_slide and ok_room else "no"))
        if ok_slide and ok_room:
            best = w
    say("largest weight that meets both: %s (ops.ODO_PHOTO_WEIGHT = %s)" % (best, ops.ODO_PHOTO_WEIGHT))
    if a.out:
        with open(a.out, 'w') as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
