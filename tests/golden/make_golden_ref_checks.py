#!/usr/bin/env python
"""What the reference itself returns in the tests that compare against it, recorded (data only):

    python tests/golden/make_golden_ref_checks.py REFERENCE_ROOT    ->  tests/golden/ref_checks.npz

REFERENCE_ROOT is a checkout of the reference.  Its native part is called through oracle/_ref/libd3f_ref.so, which
must have been built from that checkout (oracle/Makefile, target `ref`).

  nb.<trial>.<dl>.{pts,lens}      test_oracle_native.py::test_oracle_vs_compiled_reference: the reference's grid
  nb.<trial>.<dl>.nbr_{shape,sha}  subsampling of each case, and the shape and the SHA-256 of the canonical form
                                  (canonical_neighbors) of its radius search of the barycentres in the cloud
  ex.<case>.<form>.{0..3}         ::test_subsample_features_and_labels_vs_compiled_reference: the outputs of every call
                                  (the features-only and labels-only forms: the attribute output alone)
  loss.<metric>.{0..6}            test_host_logic.py::test_losses_with_the_other_cdist_metrics: the reference's
                                  utils/loss.py (losses, statistics, descriptor gradients)
  arch.{names,shapes,sha}         ::test_reference_architectures_runs_on_our_blocks_unchanged: the state dict of the
                                  reference's models/architectures.py built on this package's blocks
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)

import test_host_logic as thl  # noqa: E402
import test_oracle_native as ton  # noqa: E402
from oracle import native  # noqa: E402
from util import sha  # noqa: E402


def main(ref_root):
    if not native.have_ref():
        raise SystemExit("oracle/_ref/libd3f_ref.so is not built")
    out = {}
    for key, pts, lens, dl in ton.oracle_vs_reference_cases():
        b, bb, nbr = ton.reference_grid_and_radius(native, pts, lens, dl)
        out.update({key + '.pts': b, key + '.lens': bb, key + '.nbr_shape': np.array(nbr.shape, np.int64),
                    key + '.nbr_sha': np.array(sha(ton.canonical_neighbors(b, pts, nbr)))})
    for key, pts, lens, feats, labels, dl, mp in ton.attribute_cases():
        res = ton.reference_attributes(native, pts, lens, feats, labels, dl, mp)
        keep = range(len(res)) if isinstance(mp, int) else [2]    # (the test compares only these)
        out.update({'%s.%d' % (key, i): res[i] for i in keep})
    for metric in ["cosine", "arccosine", "sqeuclidean", "cityblock"]:
        res = thl.reference_loss_outputs(ref_root, metric)
        out.update({'loss.%s.%d' % (metric, i): r.detach().float().numpy() for i, r in enumerate(res)})
    sd, _ = thl.reference_architectures_state(ref_root)
    out['arch.names'] = np.array(list(sd))
    out['arch.shapes'] = np.array([','.join(str(d) for d in v.shape) for v in sd.values()])
    out['arch.sha'] = np.array([sha(v.numpy()) for v in sd.values()])
    path = os.path.join(HERE, 'ref_checks.npz')
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(os.path.abspath(sys.argv[1]))
