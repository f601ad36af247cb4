"""The inputs of the KPConv kernel tests, checked on the CPU: what the tables of tests/kpconv_cases.py give a kernel to
do.  These are conditions on INPUTS -- a shape that misses them gets another ns or h, never a lower bar."""
import numpy as np
import pytest
import torch

import kpconv_cases as kc
from oracle import ops_ref
from util import rel_err

FWD_TOL = 2e-5   # the bounds of test_gpu_ops.py
BWD_TOL = 2e-4


def _table_of(nq, ns, h, k, h_fill):
    q, s, idx, _, kp, _, ext = kc.dense_case(kc.dense_rng(nq, ns, h, k), nq, ns, h, 1, 1, k=k, h_fill=h_fill)
    return q, s, idx, kp, ext


@pytest.mark.parametrize("nq,ns,h,k,h_fill", kc.dense_geometries())
def test_dense_tables_make_every_sum_a_sum(nq, ns, h, k, h_fill):
    q, s, idx, kp, ext = _table_of(nq, ns, h, k, h_fill)
    st = kc.input_stats(q, s, idx, kp, ext)
    shadow = idx == ns
    full_rows = float((~shadow).all(axis=1).mean())
    print("dense (%d, %d, %d) K=%d: non-zero weights %.1f %%, zero rows %.1f %%, sums with >=1 / >=2 terms %.1f / %.1f %%, "
          "supports with >=2 contributions %.1f %%, shadow entries %.1f %%, full rows %.1f %%" % (
              nq, ns, h, k, 100 * st['nonzero'], 100 * st['zero_rows'], 100 * st['sums_ge1'], 100 * st['sums_ge2'],
              100 * st['supports_ge2'], 100 * shadow.mean(), 100 * full_rows))
    assert idx.dtype == np.int64 and idx.shape == (nq, h) and idx.min() >= 0 and idx.max() <= ns
    assert not (shadow[:, :-1] & ~shadow[:, 1:]).any()            # shadows only at row ends
    live = np.where(shadow, -1 - np.arange(h)[None, :], idx)      # no support twice in a row
    assert all(np.unique(r).size == h for r in live)
    assert st['nonzero'] >= 0.05
    if h > 1:
        assert st['zero_rows'] == 0.0
        assert st['sums_ge2'] >= 0.50
        assert st['supports_ge2'] >= 0.90
        assert 0.0 < full_rows < 1.0                              # both full rows and rows with shadows
    elif nq <= ns:
        # one column: no sum has two terms.  The one neighbour is the query's own support, at d = 0 or 0.01, so exactly
        # the kernel points inside the extent have their term: the centre and (0.48 / 0.66)^3 = 38 % of the others,
        # 43 % of 15 -- a third is asked for -- and every row has the centre's.  No support is named twice (distinct
        # queries): the collisions are the business of the nq > ns cases.
        assert st['zero_rows'] == 0.0
        assert st['sums_ge1'] >= 1.0 / 3.0
    else:
        # uniform queries, nq / ns = 2 per support: were the arrivals Poisson, 1 - 3 exp(-2) = 59 % of the supports
        # would be named twice; a third is asked for, since a nearest support beyond extent + 0.66 r contributes nothing
        assert st['supports_ge2'] >= 1.0 / 3.0


def test_shift_keeps_the_table_and_the_differences():
    """The far-away cases: same table, and s - q of neighbouring float32 points is exact, so the float64 oracle on the
    shifted float32 coordinates sees differences a float32 kernel can reproduce bit for bit."""
    nq, ns, h = kc.SHIFT_SHAPES['fused'][:3]
    q0, s0, idx0, _, kp0, _, e0 = kc.dense_case(kc.dense_rng(nq, ns, h), nq, ns, h, 1, 1)
    q, s, idx, _, kp, _, e = kc.dense_case(kc.dense_rng(nq, ns, h), nq, ns, h, 1, 1, shift=kc.SHIFT)
    assert np.array_equal(idx, idx0) and np.array_equal(kp, kp0) and e == e0
    assert q.dtype == np.float32 and s.dtype == np.float32 and abs(float(q[:, 0].mean()) - 300.5) < 0.1
    live = idx < ns
    rel32 = (s[np.minimum(idx, ns - 1)] - q[:, None, :])[live]
    rel64 = (s.astype(np.float64)[np.minimum(idx, ns - 1)] - q.astype(np.float64)[:, None, :])[live]
    assert np.array_equal(rel32.astype(np.float64), rel64)
    st = kc.input_stats(q, s, idx, kp, e)
    assert st['zero_rows'] == 0.0 and st['sums_ge2'] >= 0.50 and st['supports_ge2'] >= 0.90


def test_the_random_table_leaves_the_kernels_nothing_to_sum():
    """The finding the dense cases answer: on the generator the KPConv tests started with, under 1 % of the influence
    weights are non-zero, most output rows are exactly zero and next to no sum has two terms."""
    nq, ns, h, cin, cout = 1000, 1000, 42, 32, 32
    q, s, idx, x, kp, w = kc._kpconv_case(np.random.default_rng(nq + cin), nq, ns, h, cin, cout)
    st = kc.input_stats(q, s, idx, kp, kc.SPARSE_EXTENT)
    print("sparse (%d, %d, %d): non-zero weights %.2f %%, zero rows %.1f %%, sums with >=2 terms %.2f %%, supports with "
          ">=2 contributions %.2f %%" % (nq, ns, h, 100 * st['nonzero'], 100 * st['zero_rows'], 100 * st['sums_ge2'],
                                         100 * st['supports_ge2']))
    assert st['nonzero'] < 0.01
    assert st['zero_rows'] > 0.5 and st['sums_ge2'] < 0.01 and st['supports_ge2'] < 0.05


def _kpconv_losing_columns(q, s, idx, x, kp, w, extent, keep):
    """A float32 KPConv with a reduction defect: the neighbour columns h >= keep never reach the sums (the neighbour
    count, which a kernel takes from the features alone, stays that of the whole row)."""
    t = [torch.from_numpy(a) for a in (q, s, idx, x, kp, w)]
    x_pad = torch.cat([t[3], torch.zeros_like(t[3][:1])], 0)
    count = lambda table: torch.clamp((x_pad[table].sum(dim=-1) > 0).sum(dim=-1), min=1).float()
    cut = t[2][:, :keep]
    out = ops_ref.kpconv(t[0], t[1], cut, t[3], t[4], t[5], extent)
    return (out * (count(cut) / count(t[2]))[:, None]).numpy()


_DEFECT_SHAPES = [s for s in kc.FWD_BWD_SHAPES if s[2] > 32]


def test_a_reduction_that_loses_columns_is_seen_on_dense_tables_only():
    """What the dense inputs buy.  A KPConv that drops every neighbour column h >= 32, against the float64 oracle:
    on the dense table of every shape with h > 32 it exceeds FWD_TOL a thousandfold (rel_err 0.02 - 0.16) and is off in
    59 - 85 % of the rows that have more than 32 neighbours.  On the sparse tables a row's only live term sits in a
    dropped column now and then: measured, 13.6 % of the rows that have any output over the twelve shapes (3.9 % to
    30.4 % per shape, 2 to 20 rows) -- the other rows, and the 80 - 90 % of rows without output, cannot tell."""
    seen = total = 0
    for nq, ns, h, cin, cout in _DEFECT_SHAPES:
        q, s, idx, x, kp, w = kc._kpconv_case(np.random.default_rng(nq + cin), nq, ns, h, cin, cout)
        ref = kc.oracle64(q, s, idx, x, kp, w, kc.SPARSE_EXTENT)[0]
        got = _kpconv_losing_columns(q, s, idx, x, kp, w, kc.SPARSE_EXTENT, 32)
        rows = np.abs(ref).max(axis=1) > 0
        off = np.abs(got - ref).max(axis=1) > FWD_TOL * np.abs(ref).max()
        assert not off[~rows].any()
        print("sparse (%d, %d, %d, %d, %d): %d of %d rows with output see the defect (%.1f %%)" % (
            nq, ns, h, cin, cout, off.sum(), rows.sum(), 100.0 * off.sum() / max(rows.sum(), 1)))
        seen, total = seen + int(off.sum()), total + int(rows.sum())
    print("sparse, all shapes: %.1f %% of the rows with output" % (100.0 * seen / total))
    assert seen < 0.2 * total
    for nq, ns, h, cin, cout in _DEFECT_SHAPES:
        q, s, idx, x, kp, w, ext = kc.dense_case(kc.dense_rng(nq, ns, h), nq, ns, h, cin, cout)
        ref = kc.oracle64(q, s, idx, x, kp, w, ext)[0]
        got = _kpconv_losing_columns(q, s, idx, x, kp, w, ext, 32)
        err = rel_err(got, ref)
        off = np.abs(got - ref).max(axis=1) > FWD_TOL * np.abs(ref).max()
        long_rows = (idx[:, 32:] < ns).any(axis=1)
        print("dense (%d, %d, %d, %d, %d): rel_err %.2e, %.1f %% of all rows off, %.1f %% of the rows longer than 32" % (
            nq, ns, h, cin, cout, err, 100.0 * off.mean(), 100.0 * off[long_rows].mean()))
        assert err > 100 * FWD_TOL and off[long_rows].mean() > 0.5


@pytest.mark.parametrize("nq,ns,h,cin,cout", [(300, 400, 42, 32, 32), (97, 154, 23, 512, 512), (333, 1000, 37, 64, 64),
                                              (257, 300, 45, 128, 128), (700, 900, 42, 1, 64), (200, 260, 42, 24, 40),
                                              (300, 300, 17, 3, 8), (600, 300, 64, 32, 32)])
def test_float32_oracle_against_float64_on_dense_tables(nq, ns, h, cin, cout):
    """How far the float32 CPU oracle itself is from the float64 one on dense input (measured: 6.3e-7 at most on these
    tables, 7.3e-7 with other seeds; output and both gradients): the room FWD_TOL / BWD_TOL leave a kernel is more than
    25 times that."""
    q, s, idx, x, kp, w, ext = kc.dense_case(kc.dense_rng(nq, ns, h), nq, ns, h, cin, cout)
    go = np.random.default_rng(nq).normal(size=(nq, cout)).astype(np.float32)
    ref = kc.oracle64(q, s, idx, x, kp, w, ext, grad_out=go)
    tx, tw = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(w).requires_grad_(True)
    out = ops_ref.kpconv(torch.from_numpy(q), torch.from_numpy(s), torch.from_numpy(idx), tx, torch.from_numpy(kp), tw, ext)
    out.backward(torch.from_numpy(go))
    errs = [rel_err(a, b) for a, b in zip((out.detach().numpy(), tx.grad.numpy(), tw.grad.numpy()), ref[:3])]
    print("float32 oracle vs float64 (%d, %d, %d, %d, %d): out %.2e grad_x %.2e grad_w %.2e" % (nq, ns, h, cin, cout, *errs))
    assert errs[0] < FWD_TOL / 10 and errs[1] < BWD_TOL / 100 and errs[2] < BWD_TOL / 100


@pytest.mark.parametrize("mode", [("linear", "sum"), ("gaussian", "closest"), ("constant", "sum")], ids="-".join)
def test_float32_oracle_against_float64_at_the_modes_of_the_gather_test(mode):
    """The inputs of test_deterministic_gpu's gather test at ns = 37, 64 channels, for the influence / aggregation modes it
    runs: the float32 oracle stays inside FWD_TOL / BWD_TOL of the float64 one (no near-tie of the 'closest' arg-min flips
    between the two precisions on these inputs), so a miss on the GPU is the kernel's."""
    ns, ch, h = 37, 64, 12
    rng = np.random.default_rng([ns, ch])
    q, s, idx, x, kp, w = kc._kpconv_case(rng, ns, ns, h, ch, ch)
    rng.normal(size=ch)                                      # (the bias the test draws before the output gradient)
    go = rng.normal(size=(ns, ch)).astype(np.float32)
    res = []
    for dt in (torch.float32, torch.float64):
        t = [torch.from_numpy(a).to(dt) for a in (q, s, x, kp, w)]
        tx, tw = t[2].requires_grad_(True), t[4].requires_grad_(True)
        out = ops_ref.kpconv(t[0], t[1], torch.from_numpy(idx), tx, t[3], tw, kc.SPARSE_EXTENT, *mode)
        out.backward(torch.from_numpy(go).to(dt))
        res.append([a.detach().numpy() for a in (out, tx.grad, tw.grad)])
    errs = [rel_err(a, b) for a, b in zip(*res)]
    print("float32 oracle vs float64 at %s: out %.2e grad_x %.2e grad_w %.2e" % (mode, *errs))
    assert np.abs(res[1][0]).max() > 0 and np.abs(res[1][1]).max() > 0
    assert errs[0] < FWD_TOL and errs[1] < BWD_TOL and errs[2] < BWD_TOL
