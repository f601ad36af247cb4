"""csrc/matching.hip against np.argmin, bit for bit: on the exact-lattice descriptors of tests/matching_cases.py every
float32 summation order gives the same products, so the kernel's row arg-min, column arg-min and mutual flag must EQUAL
the reference's -- no tolerance, no share of flips -- with exact ties, rounding collisions and negative 2 - 2a planted at
every structure of the kernel (tests/test_matching_cases_cpu.py proves that they are there and that a wrong rule is seen)."""
import numpy as np
import pytest
import torch

import matching_cases as mc
from d3feat_pytorch_amd import _native, ops
from d3feat_pytorch_amd.geometric_registration.common import build_correspondence
from oracle import ops_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _device(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _assert_equals_reference(S, T, bits, name, groups=()):
    """ops.mutual_nn == np.argmin on the exact products; a failure names the planted lines that came out wrong by the
    structure they straddle."""
    want = mc.reference(mc.exact_products(S, T, bits))
    got = [x.cpu().numpy() for x in ops.mutual_nn(_device(S), _device(T))]
    planted = [(g['side'], g['placement'], g['line'], g['members']) for g in groups
               if got[0 if g['side'] == 'row' else 1][g['line']] != g['expect']]
    for what, g, w in zip(("row_argmin", "col_argmin", "mutual"), got, want):
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, "%s: %s differs at %s: kernel %s, np.argmin %s; planted lines missed: %s" % (
            name, what, bad[:8], g[bad[:8]], w[bad[:8]], planted)
    return got


@pytest.mark.parametrize("C", mc.WIDTHS)
def test_mutual_nn_equals_np_argmin_on_exact_inputs(C):
    for p in mc.problems(C):
        got = _assert_equals_reference(p.S, p.T, p.bits, p.name, p.groups)
        assert np.array_equal(build_correspondence(p.S, p.T), ops_ref.build_correspondence(p.S, p.T)), p.name
        again = ops.mutual_nn(_device(p.S), _device(p.T))                       # a second launch: identical tensors
        assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(again, got)), p.name


@pytest.mark.parametrize("C", mc.WIDTHS)
@pytest.mark.parametrize("match_wgs", [1, 0, 4096])
def test_every_column_split_gives_the_same_exact_result(C, match_wgs):
    """match_wgs = 1: one chunk of 704 columns per row block; 0 (the default) and 4096: three chunks of 256."""
    old = _native.set_tunables(match_wgs=match_wgs)
    try:
        for p in mc.problems(C):
            _assert_equals_reference(p.S, p.T, p.bits, "%s, match_wgs = %d" % (p.name, match_wgs), p.groups)
    finally:
        _native.set_tunables(**old)


@pytest.mark.parametrize("C", mc.WIDTHS)
def test_degenerate_shapes_equal_np_argmin(C):
    for name, S, T in mc.degenerate(C):
        _assert_equals_reference(S, T, 12, "%s, C = %d" % (name, C))


@pytest.mark.parametrize("C", mc.WIDTHS)
def test_mutual_nn_batched_equals_np_argmin_of_every_pair(C):
    D, seg, bits = mc.batched(C)
    d = _device(D)
    out = ops.mutual_nn_batched(d, d, _device(seg), mc.NS, mc.NT)
    ra, ca, mu = (x.cpu().numpy() for x in out)
    again = ops.mutual_nn_batched(d, d, _device(seg), mc.NS, mc.NT)
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    for n, ((so, sn, to, tn), b) in enumerate(zip(seg.tolist(), bits)):
        if tn == 0:
            assert np.all(ra[so:so + sn] == -1) and not mu[so:so + sn].any(), n
            continue
        row, col, mutual = mc.reference(mc.exact_products(D[so:so + sn], D[to:to + tn], b))
        assert np.array_equal(ca[to:to + tn], col), (n, np.nonzero(ca[to:to + tn] != col)[0][:8])
        assert np.array_equal(ra[so:so + sn], row), (n, np.nonzero(ra[so:so + sn] != row)[0][:8])
        assert np.array_equal(mu[so:so + sn].astype(bool), mutual), n
