#!/usr/bin/env python
"""The pose graph of one benchmark scene, recorded (data only):

    python tests/golden/make_golden_posegraph.py GT_RESULT_DIR    ->  tests/golden/posegraph_lab_hj.npz

GT_RESULT_DIR is the benchmark's ``gt_result`` folder (``geometric_registration/gt_result`` of the reference); the
``gt.log`` / ``gt.info`` of ``sun3d-mit_lab_hj-lab_hj_tea_nov_2_2012_scan1_erika`` are read with the project's own
``evaluate.loadlog`` / ``registration.loadinfo`` and stored as arrays, keys ordered by (i, j):

  num_nodes   int     fragments of the scene (the third number of every header line)
  edges       int32   [E,2]    (i, j) of the key ``i_j``, i < j
  T           f64     [E,4,4]  the ``gt.log`` matrix: maps fragment j into fragment i
  info        f64     [E,6,6]  the ``gt.info`` matrix (moving frame, translation block first)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
SCENE = 'sun3d-mit_lab_hj-lab_hj_tea_nov_2_2012_scan1_erika'


def main(gt_result):
    from d3feat_pytorch_amd.geometric_registration import evaluate as ev
    from d3feat_pytorch_amd.geometric_registration.registration import loadinfo
    gtpath = os.path.join(gt_result, SCENE + '-evaluation')
    log, info = ev.loadlog(gtpath), loadinfo(gtpath)
    with open(os.path.join(gtpath, 'gt.log')) as f:
        num_nodes = int(f.readline().split()[2])
    keys = sorted(log, key=lambda k: tuple(int(x) for x in k.split('_')))
    assert sorted(info) == sorted(log)
    edges = np.array([[int(x) for x in k.split('_')] for k in keys], dtype=np.int32)
    np.savez_compressed(os.path.join(HERE, 'posegraph_lab_hj.npz'), num_nodes=np.int64(num_nodes), edges=edges,
                        T=np.stack([np.asarray(log[k], dtype=np.float64) for k in keys]),
                        info=np.stack([info[k] for k in keys]))
    print("%s: %d nodes, %d edges, %d consecutive" % (SCENE, num_nodes, len(keys),
                                                      int((edges[:, 1] - edges[:, 0] == 1).sum())))


if __name__ == '__main__':
    main(sys.argv[1])
