"""The premises of test_rowgemm_instantiations_gpu.py, checked without a GPU: the exact tier of rowgemm_cases.py is
exact (float32 NumPy gives the bits of float64 on every case, so a kernel that sums in any order must too), both
LeakyReLU branches run, and the case lists reach every instantiation the dispatch of csrc/linear.hip can select."""
import numpy as np
import torch

import rowgemm_cases as rc


def _distinct(cases, key):
    seen = {}
    for c in cases:
        seen.setdefault(key(c), c)
    return list(seen.values())


def test_dispatch_rule_at_its_thresholds():
    """expected_kernel at the edges of the rule it restates, against instantiations written out by hand."""
    k = rc.expected_kernel
    assert k(4095, 32, 64, 0, 0, True, True) == "rowgemm_kernel<2,2,T,T>"          # below 4096 rows: never the rt form
    assert k(4096, 32, 64, 0, 0, True, True) == "rowgemm_rt_kernel<2,2,2,0>"
    assert k(4096, 32, 64, 0, 1, True, True) == "rowgemm_kernel<2,2,T,T>"          # rowgemm_rt = 1: never
    assert k(4096, 48, 64, 0, 0, True, True) == "rowgemm_kernel<2,2,T,T>"          # K / 16 = 3
    assert k(4096, 128, 64, 0, 0, True, True) == "rowgemm_kernel<2,2,T,T>"         # K / 16 = 8
    assert k(4096, 64, 64, 0, 0, False, True) == "rowgemm_kernel<2,2,F,T>"         # grad-input keeps rowgemm_kernel
    assert k(4096, 64, 64, 0, 0, False, False) == "rowgemm_kernel<2,2,F,F>"
    assert k(65535, 16, 128, 0, 0, True, True) == "rowgemm_rt_kernel<2,4,1,0>"     # wide from 65536 rows
    assert k(65536, 16, 128, 0, 0, True, True) == "rowgemm_rt_kernel<4,2,1,0>"
    assert k(65536, 16, 128, 1, 0, True, True) == "rowgemm_rt_kernel<2,4,1,0>"     # rowgemm_wide = 1: never
    assert k(1, 16, 64, 2, 0, True, True) == "rowgemm_kernel<4,1,T,T>"             # rowgemm_wide = 2: always
    assert k(1, 16, 32, 2, 0, True, True) == k(1, 16, 32, 1, 0, True, True) == "rowgemm_kernel<1,2,T,T>"
    assert k(1, 1024, 256, 2, 0, False, False) == "rowgemm_kernel<4,4,F,F>"
    assert k(4096, (32, 64), 128, 1, 0, True, True, pair=True) == "rowgemm_rt_kernel<2,4,2,4>"
    assert k(70000, (16, 32), 64, 0, 0, True, True, pair=True) == "rowgemm_rt_kernel<4,1,1,2>"
    assert not rc.pair_supported(4095, 32, 64, 128) and not rc.pair_supported(4096, 32, 64, 64)


def test_case_lists_reach_all_40_row_streaming_instantiations():
    assert len(rc.ALL_INSTANTIATIONS) == len(set(rc.ALL_INSTANTIATIONS)) == 40
    reached = {c.kernel for c in rc.UNARY_CASES + rc.PAIR_CASES + rc.PAIR_EPILOGUE_CASES}
    assert sorted(reached) == rc.ALL_INSTANTIATIONS
    # each list reaches what it is there for, on its own
    assert {c.kernel for c in rc.ROWGEMM_CASES} == {n for n in rc.ALL_INSTANTIATIONS if n.startswith("rowgemm_kernel")}
    assert {c.kernel for c in rc.RT_CASES} == {n for n in rc.ALL_INSTANTIATIONS if n.startswith("rowgemm_rt") and n.endswith(",0>")}
    assert {c.kernel for c in rc.PAIR_CASES} == {n for n in rc.ALL_INSTANTIATIONS if n.startswith("rowgemm_rt") and not n.endswith(",0>")}
    # every instantiation of rowgemm_kernel at every row edge, of rowgemm_rt_kernel at every tail
    for name in rc.ALL_INSTANTIATIONS:
        ns = {c.N for c in rc.ROWGEMM_CASES + rc.RT_CASES + rc.PAIR_CASES if c.kernel == name}
        assert ns >= set(rc.SMALL_N if name.startswith("rowgemm_kernel") else rc.RT_N), name
    # the tails: N just past a multiple of 16, of 32 and of 32 (4 / CS) for every CS
    assert {n % 16 for n in rc.RT_N} >= {0, 1, 15} and {n % 32 for n in rc.RT_N} >= {0, 1, 17}
    for cs in (1, 2, 4):
        rows_per_wg = 32 * (4 // cs)
        assert any(0 < n % rows_per_wg <= 16 for n in rc.RT_N) and any(n % rows_per_wg > rows_per_wg // 2 for n in rc.RT_N)
    # more than one workgroup where zero_init is checked: 130 rows at 16 (4 / CS) <= 64 rows a workgroup
    assert rc.SMALL_ROWS > 64


def test_first_form_cases_reach_every_tile_with_every_reducer():
    tiles = {"atb_partial_kernel<%d,%d>" % (i, j) for i in (1, 2, 4) for j in (1, 2, 4)}
    plain = {(c.plan["partial"], c.plan["reducer"]) for c in rc.ATB_CASES}
    assert plain == {(t, r) for t in tiles for r in ("atb_reduce_kernel<16>", "atb_reduce_kernel<4>")}
    bias = {(c.plan["partial"], c.plan["reducer"]) for c in rc.ATB_BIAS_CASES}
    assert bias == {(t, "atb_reduce_bias_kernel[fan16=%d]" % f) for t in tiles for f in (0, 1)}
    for t in tiles:     # one block and three blocks on either side, trailing partitions past the last row
        blocks = {c.plan["blocks"] for c in rc.ATB_CASES if c.plan["partial"] == t}
        assert blocks == {(1, 1), (1, 3), (3, 1), (3, 3)}
        assert any(c.plan["past_R"] for c in rc.ATB_CASES if c.plan["partial"] == t)
    assert {c.plan["P"] for c in rc.ATB_CASES} >= {1, 2, 3, 5, 57, 65}
    assert {c.bias_blocks for c in rc.ATB_BIAS_CASES} == {5, 70} and {c.gb2 for c in rc.ATB_BIAS_CASES} == {False, True}
    # the partition plan restated: a forced count is honoured up to one partition per 64 rows
    assert rc.atb_partitions(4099, 16, 16, 512) == 65 and rc.atb_partitions(4099, 16, 16, 3) == 3
    assert rc.atb_partitions(4099, 16, 16, 0) == 65 and rc.atb_partitions(4223, 192, 192, 512) == 57
    assert rc.atb_partitions(5, 64, 64, 0) == 1 and rc.atb_partitions(4099, 192, 192, 0) == 29


def test_exact_unary_cases_are_exact_in_float32():
    cases = _distinct(rc.UNARY_CASES, lambda c: (c.kind, c.K, c.M, rc.rows_of(c), c.epi, c.slope))
    assert {(4223, 1024, 256), (130, 64, 128), (4099, 16, 64)} <= {(c.N, c.K, c.M) for c in rc.UNARY_CASES}
    negative = []
    for c in cases:
        rows = rc.rows_of(c)
        x, w, b1, add, b2 = rc.unary_operands(c.kind, c.K, c.M, rows)
        for a, bound in ((x, rc.INT_X), (w, rc.INT_X), (b1, rc.INT_BIAS), (add, rc.INT_BIAS), (b2, rc.INT_BIAS)):
            assert a.dtype == np.float32 and np.array_equal(a, np.rint(a)) and np.abs(a).max() <= bound
        want = rc.unary_expected(c.kind, c.K, c.M, rows, c.epi, c.slope)
        got = rc.unary_product(c.kind, x, w, b1, add, b2, c.epi, c.slope, np.float32)
        assert got.dtype == np.float32 and want.dtype == np.float32
        assert np.array_equal(got, want), c
        ref64 = rc.unary_product(c.kind, x, w, b1, add, b2, c.epi, c.slope, np.float64)
        assert np.array_equal(want.astype(np.float64), ref64), c            # the cast lost nothing
        assert np.abs(ref64).max() < 2 ** 24 and not (want == rc.SENTINEL).any()
        if c.kind == "fwd" and c.slope != 1.0:
            negative.append(float((ref64 < 0).mean()))
            assert 0.4 < negative[-1] < 0.6, (c, negative[-1])              # both LeakyReLU branches run
    assert negative
    # the largest magnitude any order of summation can pass through
    assert rc.INT_X * rc.INT_X * 1024 + 3 * rc.INT_BIAS < 2 ** 24


def test_exact_pair_cases_are_exact_in_float32():
    for c in _distinct(rc.PAIR_CASES + rc.PAIR_EPILOGUE_CASES, lambda c: (c.K1, c.K2, c.M, c.biases, c.slope)):
        x1, w1, x2, w2, *biases = rc.pair_operands(c.K1, c.K2, c.M, rc.RT_ROWS)
        want = rc.pair_expected(c.K1, c.K2, c.M, rc.RT_ROWS, c.biases, c.slope)
        got = rc.pair_product(x1, w1, x2, w2, biases, c.biases, c.slope, np.float32)
        assert got.dtype == np.float32 and np.array_equal(got, want), c
        assert np.array_equal(want.astype(np.float64), rc.pair_product(x1, w1, x2, w2, biases, c.biases, c.slope, np.float64))
        if c.slope != 1.0:
            assert 0.4 < float((want < 0).mean()) < 0.6
    assert {c.biases for c in rc.PAIR_EPILOGUE_CASES} == {(a, b, c, d) for a in (False, True) for b in (False, True)
                                                          for c in (False, True) for d in (False, True)}


def test_exact_weight_gradient_cases_are_exact_in_float32_in_any_partition():
    assert max(rc.ATB_R) <= 4223 and rc.INT_ATB * rc.INT_ATB * max(rc.ATB_R) < 2 ** 24
    for c in _distinct(rc.ATB_CASES + rc.ATB_BIAS_CASES, lambda c: (c.R, c.Cin, c.Cout)):
        x, go = rc.atb_operands(c.Cin, c.Cout)
        assert np.array_equal(x, np.rint(x)) and np.abs(x).max() <= rc.INT_ATB and np.abs(go).max() <= rc.INT_ATB
        want = rc.atb_expected(c.R, c.Cin, c.Cout)
        assert want.shape == (c.Cout, c.Cin)
        assert np.array_equal((go[:c.R].T @ x[:c.R]).astype(np.float32), want), c
        assert np.array_equal(want.astype(np.float64), go[:c.R].astype(np.float64).T @ x[:c.R].astype(np.float64))
    # a 65-way split reduction over 4099 rows, summed in float32 slab by slab
    for cin, cout in ((16, 16), (64, 64), (192, 48)):
        x, go = rc.atb_operands(cin, cout)
        assert np.array_equal(rc.partitioned_sum32(go[:4099], x[:4099], 65), rc.atb_expected(4099, cin, cout))
    for blocks in (5, 70):
        part, total = rc.bias_partials(blocks, 64)
        assert np.array_equal(part.sum(0, dtype=np.float32), total) and np.array_equal(part[::-1].cumsum(0, dtype=np.float32)[-1], total)


def _unary_torch(t, slope):
    x, w, b1, add, b2 = t
    v = x @ w.t() + b1 + b2 + (add if add is not None else 0.0)
    return torch.nn.functional.leaky_relu(v, slope)


def _pair_torch(t, slope):
    x1, w1, x2, w2, b1, b2, b3, b4 = t
    return torch.nn.functional.leaky_relu(x1 @ w1.t() + x2 @ w2.t() + b1 + b2 + b3 + b4, slope)


def test_exact_autograd_cases_are_exact_in_float32():
    """Output and every gradient of the autograd cases: float32 autograd on the CPU gives the bits of float64."""
    R = rc.AUTOGRAD_ROWS
    problems = []
    for cin, cout, with_add in rc.AUTOGRAD_UNARY:
        x, w, b1, add, b2 = rc.unary_operands("fwd", cin, cout, rc.RT_ROWS)
        problems.append((_unary_torch, [x[:R], w, b1, add[:R] if with_add else None, b2], cout))
    k1, k2, m = rc.AUTOGRAD_PAIR
    x1, w1, x2, w2, *biases = rc.pair_operands(k1, k2, m, rc.RT_ROWS)
    problems.append((_pair_torch, [x1[:R], w1, x2[:R], w2] + list(biases), m))
    for fn, operands, cout in problems:
        go = rc.autograd_grad_out(cout)
        out, grads = rc.autograd_reference(lambda t: fn(t, rc.SLOPE), operands, go)
        leaves = [torch.from_numpy(np.array(a)).requires_grad_(True) if a is not None else None for a in operands]
        out32 = fn(leaves, rc.SLOPE)
        out32.backward(torch.from_numpy(np.array(go)))
        assert np.array_equal(out32.detach().numpy(), out)
        for leaf, g in zip(leaves, grads):
            if leaf is not None:
                assert leaf.grad.dtype == torch.float32 and np.array_equal(leaf.grad.numpy(), g)
                assert np.abs(g).max() * 4 < 2 ** 24 and np.array_equal(g * 4, np.rint(g * 4))     # whole quarter units
        # pre-activations that are exactly zero exist, so the gradient's choice of branch at 0 is part of the check
        assert (out == 0).any() and 0.4 < float((out < 0).mean()) < 0.6
