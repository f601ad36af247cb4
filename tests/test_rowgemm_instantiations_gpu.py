"""Every instantiation of the row-streaming GEMM kernels of csrc/linear.hip, launched through the C entries and held to
float64 with ZERO tolerance on the exact inputs of rowgemm_cases.py (np.array_equal / torch.equal, whatever the order of
summation), and to float64 at the tolerances of test_gpu_ops.py on random inputs:

* rowgemm_kernel<MBW,CS,WT,EPI> (18), rowgemm_rt_kernel<MBW,CS,KT,0> (18) and the four pair kernels, one test per
  instantiation, at every row edge; rows at and beyond N untouched; zero_init cleared up to zero_n and not beyond;
* every epilogue combination; the guards of the pair entry;
* wide against narrow and rt against non-rt, bit for bit, on random inputs;
* the first form of A^T B (atb_partial_kernel<TI,TJ,U> and its three reducers) at every tile, partition count and ragged
  row count, and the grouped form on the same cases;
* ops.linear_bias_act / ops.linear_pair_bias_act through autograd, output and all gradients bit-equal to float64;
* the round-1 aggregation kept behind tunables().agg_through_lds against the direct one.

The tunables are process-global: every test restores them in a finally block."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from d3feat_pytorch_amd import _native, ops
import kpconv_cases as kc
import rowgemm_cases as rc
from util import rel_err

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FWD_TOL = 2e-5   # test_gpu_ops.py
BWD_TOL = 2e-4
SENT = rc.SENTINEL


@contextlib.contextmanager
def tunables(**kw):
    old = _native.set_tunables(**kw)
    try:
        yield
    finally:
        _native.set_tunables(**old)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV) if a is not None else None      # (a copy: the shared cases are read-only)


def _p(t):
    return t.data_ptr() if t is not None else None


def _stream():
    return torch.cuda.current_stream().cuda_stream


# operands and expected results live on the device once per shape; nothing writes to them
@functools.lru_cache(maxsize=None)
def unary_dev(kind, K, M, rows, exact=True):
    return tuple(dev(a) for a in rc.unary_operands(kind, K, M, rows, exact))


@functools.lru_cache(maxsize=None)
def unary_expected_dev(kind, K, M, rows, epi, slope):
    return dev(rc.unary_expected(kind, K, M, rows, epi, slope))


@functools.lru_cache(maxsize=None)
def pair_dev(K1, K2, M, rows, exact=True):
    return tuple(dev(a) for a in rc.pair_operands(K1, K2, M, rows, exact))


@functools.lru_cache(maxsize=None)
def pair_expected_dev(K1, K2, M, rows, on, slope):
    return dev(rc.pair_expected(K1, K2, M, rows, on, slope))


def _guarded(N, M):
    return torch.full((N + rc.GUARD_ROWS, M), SENT, dtype=torch.float32, device=DEV)


def _zero_buffer(M):
    """(buffer, zero_n): 3 M + 5 sentinels of which the launch is to clear the first 2 M."""
    return torch.full((3 * M + 5,), SENT, dtype=torch.float32, device=DEV), 2 * M


def launch_unary(kind, ops_dev, N, epi, slope, zero=None, zero_n=0):
    """One launch of N rows on the first N rows of the operands; returns the guarded output [N + GUARD_ROWS, M]."""
    x, w, b1, add, b2 = ops_dev
    L = _native.lib()
    if kind == "fwd":
        M, K = w.shape
        out = _guarded(N, M)
        code = L.d3f_linear_bias_act_forward(_p(x), _p(w), N, K, M, _p(b1) if epi[0] else None, _p(add) if epi[1] else None,
                                             _p(b2) if epi[2] else None, float(slope), _p(out), _p(zero), zero_n, _stream())
    else:
        K, M = w.shape                                   # weight [Cout, Cin] as stored: the reduction runs over Cout
        assert zero is None and not epi[0] and not epi[2] and slope == 1.0
        out = _guarded(N, M)
        code = L.d3f_linear_grad_input(_p(x), _p(w), N, M, K, _p(add) if epi[1] else None, _p(out), _stream())
    _native.check(code, "row-streaming launch %s" % kind)
    return out


def launch_pair(ops_dev, N, on, slope, zero=None, zero_n=0):
    x1, w1, x2, w2, *b = ops_dev
    M, K1, K2 = w1.shape[0], w1.shape[1], w2.shape[1]
    out = _guarded(N, M)
    bp = [_p(t) if use else None for t, use in zip(b, on)]
    code = _native.lib().d3f_linear_pair_bias_act_forward(_p(x1), _p(w1), K1, _p(x2), _p(w2), K2, N, M, bp[0], bp[1], bp[2],
                                                          bp[3], float(slope), _p(out), _p(zero), zero_n, _stream())
    _native.check(code, "d3f_linear_pair_bias_act_forward")
    return out


def mismatch(out, want, N):
    """None when rows [0, N) of ``out`` equal ``want`` bit for value and the guard rows still hold the sentinel; else a
    short description (how many elements differ, the first of them)."""
    if not bool((out[N:] == SENT).all()):
        rows = torch.nonzero((out[N:] != SENT).any(dim=1)).flatten().tolist()
        return "rows at and beyond N written: N + %s" % rows
    if torch.equal(out[:N], want[:N]):
        return None
    bad = torch.nonzero(out[:N] != want[:N])
    r, c = bad[0].tolist()
    return "%d of %d elements differ, first at [%d, %d]: got %r, want %r" % (
        bad.shape[0], N * out.shape[1], r, c, float(out[r, c]), float(want[r, c]))


def zero_mismatch(zero, zero_n):
    if not bool((zero[:zero_n] == 0.0).all()):
        return "zero_init: %d of the first %d entries not cleared" % (int((zero[:zero_n] != 0.0).sum()), zero_n)
    if not bool((zero[zero_n:] == SENT).all()):
        return "zero_init: entries at and beyond zero_n written"
    return None


def run_unary_case(c):
    """A case of rowgemm_cases under its tunables; returns a failure description or None."""
    rows = rc.rows_of(c)
    with tunables(rowgemm_wide=c.wide, rowgemm_rt=c.rt):
        zero, zero_n = _zero_buffer(c.M) if (c.kind == "fwd" and c.N > 64) else (None, 0)
        out = launch_unary(c.kind, unary_dev(c.kind, c.K, c.M, rows), c.N, c.epi, c.slope, zero, zero_n)
    bad = mismatch(out, unary_expected_dev(c.kind, c.K, c.M, rows, c.epi, c.slope), c.N)
    if bad is None and zero is not None:
        bad = zero_mismatch(zero, zero_n)
    return bad


def run_pair_case(c):
    with tunables(rowgemm_wide=c.wide):
        zero, zero_n = _zero_buffer(c.M)
        out = launch_pair(pair_dev(c.K1, c.K2, c.M, rc.RT_ROWS), c.N, c.biases, c.slope, zero, zero_n)
    return mismatch(out, pair_expected_dev(c.K1, c.K2, c.M, rc.RT_ROWS, c.biases, c.slope), c.N) or zero_mismatch(zero, zero_n)


def _report(failures):
    assert not failures, "%d case(s) differ from float64:\n%s" % (len(failures), "\n".join("%s: %s" % f for f in failures))


# ---- one test per instantiation -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", rc.ALL_INSTANTIATIONS)
def test_instantiation_is_exact_at_every_row_edge(kernel):
    """Every case that reaches ``kernel``: the exact output, nothing written at or beyond row N, zero_init cleared up to
    zero_n on the launches of more than one workgroup."""
    unary = [c for c in rc.ROWGEMM_CASES + rc.RT_CASES if c.kernel == kernel]
    pair = [c for c in rc.PAIR_CASES if c.kernel == kernel]
    assert unary or pair
    failures = [(c, bad) for c in unary for bad in [run_unary_case(c)] if bad]
    failures += [(c, bad) for c in pair for bad in [run_pair_case(c)] if bad]
    _report(failures)


def test_epilogue_combinations_of_the_unary_kernels():
    """none / b1 / add / b2 / all three / no activation, on rowgemm_kernel<2,2,T,T> and rowgemm_rt_kernel<4,2,2,0>."""
    assert {c.kernel for c in rc.EPILOGUE_CASES} == {"rowgemm_kernel<2,2,T,T>", "rowgemm_rt_kernel<4,2,2,0>"}
    _report([(c, bad) for c in rc.EPILOGUE_CASES for bad in [run_unary_case(c)] if bad])


def test_epilogue_combinations_of_the_pair_kernels():
    """Every subset of the four biases on rowgemm_rt_kernel<2,4,2,4>, no activation on rowgemm_rt_kernel<4,1,1,2>."""
    _report([(c, bad) for c in rc.PAIR_EPILOGUE_CASES for bad in [run_pair_case(c)] if bad])


def test_pair_entry_refuses_what_it_does_not_serve_and_writes_nothing():
    L = _native.lib()
    assert L.d3f_linear_pair_supported(4096, 32, 64, 128) == 1 and L.d3f_linear_pair_supported(4096, 16, 32, 64) == 1
    assert L.d3f_linear_pair_supported(4095, 32, 64, 128) == 0 and L.d3f_linear_pair_supported(4096, 32, 64, 64) == 0
    x1, w1, x2, w2, *b = pair_dev(32, 64, 128, rc.RT_ROWS)
    for N, M in ((4095, 128), (4096, 64)):
        out = _guarded(N, M)
        zero, zero_n = _zero_buffer(M)
        code = L.d3f_linear_pair_bias_act_forward(_p(x1), _p(w1), 32, _p(x2), _p(w2), 64, N, M, _p(b[0]), _p(b[1]), _p(b[2]),
                                                  _p(b[3]), rc.SLOPE, _p(out), _p(zero), zero_n, _stream())
        torch.cuda.synchronize()
        assert code == _native.D3F_EINVAL
        assert bool((out == SENT).all()) and bool((zero == SENT).all())


# ---- random tier: precision, and the dealings against each other ---------------------------------------------------------------
@pytest.mark.parametrize("M", rc.WIDTHS)
def test_random_tier_matches_float64_and_the_dealings_agree_bit_for_bit(M):
    """Random normal operands against float64 at FWD_TOL (forward) / BWD_TOL (grad-input), every kernel of this output
    width.  Wide and narrow, rt and non-rt run the same MFMA sequence per output element and the same epilogue, so their
    results are the same bits."""
    all_on = (True, True, True)
    for kind, Ks, tol in (("fwd", rc.FWD_K, FWD_TOL), ("gi_add", rc.FWD_K, BWD_TOL), ("gi", rc.GI_K, BWD_TOL)):
        epi = {"fwd": all_on, "gi_add": (False, True, False), "gi": (False, False, False)}[kind]
        slope = 0.1 if kind == "fwd" else 1.0
        for K in Ks:
            N, rows = rc.SMALL_ROWS, rc.SMALL_ROWS
            ref = rc.unary_expected(kind, K, M, rows, epi, slope, False)
            outs = []
            for wide in (1, 2):
                with tunables(rowgemm_wide=wide, rowgemm_rt=1):
                    outs.append(launch_unary(kind, unary_dev(kind, K, M, rows, False), N, epi, slope))
                err = rel_err(outs[-1][:N].cpu().numpy(), ref[:N])
                print("\nROWGEMM random %s N=%d K=%d M=%d wide=%d err=%.2e" % (kind, N, K, M, wide, err))
                assert err < tol, (kind, K, M, wide)
            assert torch.equal(outs[0], outs[1]), (kind, K, M, "wide vs narrow")
    for K in rc.RT_K:
        N, rows = rc.RT_MIN_ROWS + 47, rc.RT_ROWS
        ref = rc.unary_expected("fwd", K, M, rows, all_on, 0.1, False)
        outs = {}
        for wide in (1, 2):
            for rt in (0, 1):
                with tunables(rowgemm_wide=wide, rowgemm_rt=rt):
                    outs[wide, rt] = launch_unary("fwd", unary_dev("fwd", K, M, rows, False), N, all_on, 0.1)
                err = rel_err(outs[wide, rt][:N].cpu().numpy(), ref[:N])
                print("\nROWGEMM random fwd N=%d K=%d M=%d wide=%d rt=%d err=%.2e" % (N, K, M, wide, rt, err))
                assert err < FWD_TOL, (K, M, wide, rt)
        for key in ((1, 1), (2, 0), (2, 1)):
            assert torch.equal(outs[1, 0], outs[key]), (K, M, "(wide, rt) = (1, 0) vs", key)


@pytest.mark.parametrize("K1,K2,M", rc.PAIR_SHAPES)
def test_random_tier_of_the_pair_kernels(K1, K2, M):
    N = rc.RT_MIN_ROWS + 47
    ref = rc.pair_expected(K1, K2, M, rc.RT_ROWS, rc.ALL_BIASES, 0.1, False)
    outs = []
    for wide in (1, 2):
        with tunables(rowgemm_wide=wide):
            outs.append(launch_pair(pair_dev(K1, K2, M, rc.RT_ROWS, False), N, rc.ALL_BIASES, 0.1))
        err = rel_err(outs[-1][:N].cpu().numpy(), ref[:N])
        print("\nROWGEMM random pair %d|%d->%d wide=%d err=%.2e" % (K1, K2, M, wide, err))
        assert err < FWD_TOL
    assert torch.equal(outs[0], outs[1])


# ---- first form of A^T B ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def atb_dev(Cin, Cout, exact=True):
    return tuple(dev(a) for a in rc.atb_operands(Cin, Cout, exact))


@functools.lru_cache(maxsize=None)
def atb_expected_dev(R, Cin, Cout):
    return dev(rc.atb_expected(R, Cin, Cout))


def launch_grad_weight(x, go, R, bias=None):
    """d3f_linear_grad_weight[_bias] over the first R rows into a sentinel-filled target, the workspace poisoned with NaN
    (a slab the reducer reads without its having been written shows).  bias = (partials, gb, gb2 or None)."""
    L = _native.lib()
    Cin, Cout = x.shape[1], go.shape[1]
    gw = torch.full((Cout, Cin), SENT, dtype=torch.float32, device=DEV)
    nbytes = int(L.d3f_linear_grad_weight_ws_bytes(R, Cin, Cout))
    assert nbytes > 0
    ws = torch.full(((nbytes + 3) // 4,), float("nan"), dtype=torch.float32, device=DEV)
    if bias is None:
        code = L.d3f_linear_grad_weight(_p(x), _p(go), R, Cin, Cout, _p(gw), _p(ws), nbytes, _stream())
    else:
        part, gb, gb2 = bias
        code = L.d3f_linear_grad_weight_bias(_p(x), _p(go), R, Cin, Cout, _p(gw), _p(ws), nbytes, _p(part), part.shape[0],
                                             part.shape[1], _p(gb), _p(gb2), _stream())
    _native.check(code, "d3f_linear_grad_weight")
    return gw


def _equal_or_text(got, want):
    if torch.equal(got, want):
        return None
    bad = torch.nonzero(got != want)
    i = tuple(bad[0].tolist())
    return "%d of %d elements differ, first at %s: got %r, want %r" % (bad.shape[0], got.numel(), i, float(got[i]), float(want[i]))


@pytest.mark.parametrize("form,wgs", [(1, 0), (1, 3), (1, 512), (2, 0)])
def test_weight_gradient_is_exact_at_every_tile_and_partition_count(form, wgs):
    """grad_w = grad_out^T x == float64 with zero tolerance.  form 1: atb_partial_kernel<TI,TJ,U> for all nine (TI, TJ), one
    and three blocks a side, R from one row to ragged last partitions and partitions that start past R, summed by
    atb_reduce_kernel<16> and <4>; form 2: the grouped kernels on the same cases."""
    failures = []
    with tunables(atb_form=form, atb_first_form_wgs=wgs):
        for c in rc.ATB_CASES:
            if c.wgs != wgs:
                continue
            x, go = atb_dev(c.Cin, c.Cout)
            bad = _equal_or_text(launch_grad_weight(x, go, c.R), atb_expected_dev(c.R, c.Cin, c.Cout))
            if bad:
                failures.append((c, bad))
    _report(failures)


@pytest.mark.parametrize("form", [1, 2])
def test_weight_gradient_with_the_bias_sums_is_exact(form):
    """d3f_linear_grad_weight_bias: the weight gradient as above and grad_bias (grad_bias2) = the column sums of integer
    partials of 5 and of 70 rows, through atb_reduce_bias_kernel in both its slab-summing modes (form 1) and through the
    grouped second stage (form 2)."""
    failures = []
    for c in rc.ATB_BIAS_CASES:
        x, go = atb_dev(c.Cin, c.Cout)
        part_np, total_np = rc.bias_partials(c.bias_blocks, c.Cout)
        part, total = dev(part_np), dev(total_np)
        gb = torch.full((c.Cout,), SENT, dtype=torch.float32, device=DEV)
        gb2 = torch.full((c.Cout,), SENT, dtype=torch.float32, device=DEV) if c.gb2 else None
        with tunables(atb_form=form, atb_first_form_wgs=c.wgs):
            gw = launch_grad_weight(x, go, c.R, (part, gb, gb2))
        bad = _equal_or_text(gw, atb_expected_dev(c.R, c.Cin, c.Cout)) or _equal_or_text(gb, total) or \
            (_equal_or_text(gb2, total) if gb2 is not None else None)
        if bad:
            failures.append((c, bad))
    _report(failures)


def test_weight_gradient_random_tier():
    """Random normal operands against float64 at BWD_TOL: every tile of the first form, few and many partitions."""
    for wgs in (0, 3, 512):
        with tunables(atb_form=1, atb_first_form_wgs=wgs):
            for cout in (16, 32, 192):
                for cin in (16, 96, 64):
                    x, go = atb_dev(cin, cout, False)
                    for R in (65, 4099):
                        err = rel_err(launch_grad_weight(x, go, R).cpu().numpy(), rc.atb_expected(R, cin, cout, False))
                        print("\nATB random R=%d Cin=%d Cout=%d wgs=%d err=%.2e" % (R, cin, cout, wgs, err))
                        assert err < BWD_TOL, (R, cin, cout, wgs)


# ---- through autograd ----------------------------------------------------------------------------------------------------------------
def _unary_fn(t, slope):
    x, w, b1, add, b2 = t
    v = x @ w.t() + b1
    if add is not None:
        v = v + add
    return torch.nn.functional.leaky_relu(v + b2, slope)


def _pair_fn(t, slope):
    x1, w1, x2, w2, b1, b2, b3, b4 = t
    return torch.nn.functional.leaky_relu(x1 @ w1.t() + x2 @ w2.t() + b1 + b2 + b3 + b4, slope)


@functools.lru_cache(maxsize=None)
def autograd_problems():
    """[(name, operands, grad_out, float64 output, float64 gradients)] of the two unary shapes and the pair."""
    R = rc.AUTOGRAD_ROWS
    probs = []
    for cin, cout, with_add in rc.AUTOGRAD_UNARY:
        x, w, b1, add, b2 = rc.unary_operands("fwd", cin, cout, rc.RT_ROWS)
        operands = [x[:R], w, b1, add[:R] if with_add else None, b2]
        go = rc.autograd_grad_out(cout)
        probs.append(("unary %d->%d" % (cin, cout), operands, go) + rc.autograd_reference(lambda t: _unary_fn(t, rc.SLOPE), operands, go))
    k1, k2, m = rc.AUTOGRAD_PAIR
    x1, w1, x2, w2, *biases = rc.pair_operands(k1, k2, m, rc.RT_ROWS)
    operands = [x1[:R], w1, x2[:R], w2] + list(biases)
    go = rc.autograd_grad_out(m)
    probs.append(("pair %d|%d->%d" % (k1, k2, m), operands, go) + rc.autograd_reference(lambda t: _pair_fn(t, rc.SLOPE), operands, go))
    return probs


@pytest.mark.parametrize("setting", rc.AUTOGRAD_TUNABLES, ids=lambda s: "-".join("%s=%d" % kv for kv in s.items()))
def test_autograd_nodes_are_exact(setting):
    """ops.linear_bias_act (two shapes) and ops.linear_pair_bias_act at 4096 + 47 rows: output and every gradient -- inputs,
    weights, biases, the residual -- equal float64 autograd bit for bit, under the wide dealing and without the rt form."""
    failures = []
    with tunables(**setting):
        for name, operands, go, want_out, want_grads in autograd_problems():
            leaves = [dev(a).requires_grad_(True) if a is not None else None for a in operands]
            if name.startswith("unary"):
                x, w, b1, add, b2 = leaves
                out = ops.linear_bias_act(x, w, b1, add, b2, slope=rc.SLOPE)
                assert type(out.grad_fn).__name__.startswith("_LinearBiasActFn")     # the row-streaming node, not the library GEMM
            else:
                x1, w1, x2, w2, b1, b2, b3, b4 = leaves
                out = ops.linear_pair_bias_act(x1, w1, b1, b2, x2, w2, b3, b4, slope=rc.SLOPE)
            out.backward(dev(go))
            torch.cuda.synchronize()
            if not np.array_equal(out.detach().cpu().numpy(), want_out):
                failures.append((name, "output differs"))
            for k, (leaf, want) in enumerate(zip(leaves, want_grads)):
                if leaf is not None and not np.array_equal(leaf.grad.cpu().numpy(), want):
                    d = np.abs(leaf.grad.cpu().numpy().astype(np.float64) - want)
                    failures.append((name, "gradient of operand %d: %d elements differ, max %.3g" % (k, int((d > 0).sum()), d.max())))
    _report(failures)


# ---- the aggregation kept behind agg_through_lds ---------------------------------------------------------------------------------------
def _aggregate(q, s, idx, x, kp, extent):
    L = _native.lib()
    nq, h, ns, cin, k = q.shape[0], idx.shape[1], s.shape[0], x.shape[1], kp.shape[0]
    wf = torch.full((nq, k * cin), float("nan"), dtype=torch.float32, device=DEV)
    nn = torch.full((nq,), float("nan"), dtype=torch.float32, device=DEV)
    nbytes = int(L.d3f_kpconv_ws_bytes(nq, ns, h, k, cin, 64))
    ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=DEV)
    _native.check(L.d3f_kpconv_aggregate(_p(q), nq, _p(s), ns, _p(idx), h, _p(x), cin, _p(kp), k, float(extent), _p(wf), _p(nn),
                                         None, None, _p(ws), nbytes, _stream()), "d3f_kpconv_aggregate")
    torch.cuda.synchronize()
    return wf, nn


@pytest.mark.parametrize("geometry", ["dense", "shadow_heavy"])
def test_aggregation_through_lds_equals_the_direct_aggregation(geometry):
    """d3f_kpconv_aggregate under tunables().agg_through_lds = 1 (phase A of the fused kernel, through its LDS tile) gives
    the wf and nn of the direct kernel, and both give the float64 weighted features at FWD_TOL."""
    nq, ns, h, cin = 333, 1000, 37, 64
    if geometry == "dense":
        q, s, idx, x, kp, _, extent = kc.dense_case(kc.dense_rng(nq, ns, h), nq, ns, h, cin, 64)
    else:      # seven entries in ten are shadows, the supports lie around the queries
        q, s, idx, x, kp, _ = kc._kpconv_case(np.random.default_rng(7), nq, ns, h, cin, 64, shadow_frac=0.7)
        extent = 0.3
    infl = kc.influence_weights(q, s, idx, kp, extent)                                  # [nq, h, k] float64
    x_pad = np.concatenate([x.astype(np.float64), np.zeros((1, cin))], 0)
    ref = np.einsum("nhk,nhc->nkc", infl, x_pad[np.minimum(idx, ns)]).reshape(nq, -1)
    assert (ref != 0).mean() > 0.05 and ((idx == ns).mean() > 0.6) == (geometry == "shadow_heavy")
    args = (dev(q), dev(s), dev(idx.astype(np.int32)), dev(x), dev(kp), extent)
    wf_d, nn_d = _aggregate(*args)
    with tunables(agg_through_lds=1):
        wf_l, nn_l = _aggregate(*args)
    e_d, e_l = rel_err(wf_d.cpu().numpy(), ref), rel_err(wf_l.cpu().numpy(), ref)
    e_dl = rel_err(wf_l.cpu().numpy(), wf_d.cpu().numpy())
    print("\nAGG %s direct=%.2e through_lds=%.2e between=%.2e" % (geometry, e_d, e_l, e_dl))
    assert e_d < FWD_TOL and e_l < FWD_TOL and e_dl < FWD_TOL
    assert torch.equal(nn_d, nn_l) and bool((nn_d >= 1).all())
