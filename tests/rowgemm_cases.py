"""Inputs for the tests of the row-streaming GEMM kernels of csrc/linear.hip (test_rowgemm_cases_cpu.py,
test_rowgemm_instantiations_gpu.py): plain NumPy, no GPU.

EXACT TIER.  Every operand is a small integer stored as float32, so that every product and every partial sum, taken in
ANY order, is an integer (or a multiple of 1/4) below 2^24 and therefore an exact float32:

  x, w, grad_out   integers in [-8, 8]          a product is at most 64
  bias*, add       integers in [-64, 64]
  slope            0.25                          a power of two: the LeakyReLU scaling is exact
  A^T B operands   integers in [-4, 4], R <= 4223 rows (16 * 4223 = 67 568)

The largest pre-activation is 64 * 1024 + 3 * 64 = 65 728 < 2^24.  Through autograd the masked gradient is a multiple
of 1/4 of magnitude <= 8, and the longest sum (a weight gradient over 4143 rows) stays below 4 * 64 * 4143 = 1 060 608
quarter units.  The expected result is the float64 product cast to float32, and a kernel is held to it with
np.array_equal: zero tolerance, whatever its summation order.  One dropped, duplicated or misplaced term changes an
integer by at least 1 (1/4 after the slope) and cannot hide.  test_rowgemm_cases_cpu.py proves the premise without a
GPU: float32 NumPy gives the same bits as float64 on every case.

RANDOM TIER.  Small integers cannot reveal a loss of precision (a product rounded to bf16, an accumulator narrower than
fp32), so the same shapes also run on random normal operands against float64 at the tolerances of test_gpu_ops.py.

DISPATCH.  ``expected_kernel`` restates, in pure Python, which of the 40 row-streaming instantiations
``rowgemm_launch`` / ``rowgemm_pair_launch`` select; ``atb_first_form`` restates the partition plan and the reducer of
the first form of A^T B.  Every case carries the instantiation it reaches, and the CPU test holds the case lists to
full coverage."""
import collections
import functools
import itertools

import numpy as np

SLOPE = 0.25          # a power of two
SENTINEL = -12345.0   # what the guard rows behind an output and a zero_init buffer hold before a launch
GUARD_ROWS = 8        # rows of sentinel behind every output
INT_X, INT_BIAS, INT_ATB = 8, 64, 4
RT_MIN_ROWS = 4096    # rowgemm_launch: the register-weights form from this many rows (linear.hip:1214)
WIDE_MIN_ROWS = 65536  # rowgemm_launch: the wide dealing from this many rows at rowgemm_wide = 0 (linear.hip:1210)


# ---- the dispatch rule ------------------------------------------------------------------------------------------------
def dealing(M, wide):
    """(MBW, CS) of an output width: MBW consecutive columns per lane, CS column groups per row tile; M = 16 MBW CS
    (the two switch statements of rowgemm_launch, linear.hip:1219-1224 and 1231-1236)."""
    return {32: (1, 2), 64: (4, 1) if wide else (2, 2), 128: (4, 2) if wide else (2, 4), 256: (4, 4)}[M]


def is_wide(N, rowgemm_wide):
    """linear.hip:1209-1210 (and 1253-1254 for the pair form): tunable 0 = by rows, 1 = never, 2 = always."""
    return rowgemm_wide == 2 or (rowgemm_wide == 0 and N >= WIDE_MIN_ROWS)


def pair_supported(N, K1, K2, M):
    """rowgemm_pair_supported, linear.hip:1245-1247."""
    return N >= RT_MIN_ROWS and ((M == 128 and K1 == 32 and K2 == 64) or (M == 64 and K1 == 16 and K2 == 32))


def expected_kernel(N, K, M, wide, rt, WT, EPI, pair=False):
    """The instantiation a launch reaches.  ``wide`` / ``rt``: the VALUES of tunables().rowgemm_wide / rowgemm_rt;
    (WT, EPI) = (True, True) forward, (False, True) grad-input with ``add``, (False, False) grad-input without;
    ``pair``: K is (K1, K2) and the launch is rowgemm_pair_launch (linear.hip:1249-1266), else rowgemm_launch
    (linear.hip:1199-1241)."""
    mbw, cs = dealing(M, is_wide(N, wide))
    if pair:
        K1, K2 = K
        assert pair_supported(N, K1, K2, M) and WT and EPI
        return "rowgemm_rt_kernel<%d,%d,%d,%d>" % (mbw, cs, K1 // 16, K2 // 16)                    # linear.hip:1258-1262
    assert N >= 1 and K >= 16 and K % 16 == 0 and K <= 1024                                         # linear.hip:1195-1197
    kt = K // 16
    if WT and EPI and rt != 1 and N >= RT_MIN_ROWS and kt in (1, 2, 4):                             # linear.hip:1214
        return "rowgemm_rt_kernel<%d,%d,%d,0>" % (mbw, cs, kt)
    return "rowgemm_kernel<%d,%d,%s,%s>" % (mbw, cs, "T" if WT else "F", "T" if EPI else "F")


# written out from the template arguments, not through expected_kernel: the six dealings, three (WT, EPI), three KT
DEALINGS = [(1, 2), (2, 2), (4, 1), (2, 4), (4, 2), (4, 4)]
ALL_INSTANTIATIONS = sorted(
    ["rowgemm_kernel<%d,%d,%s>" % (m, c, f) for m, c in DEALINGS for f in ("T,T", "F,T", "F,F")] +
    ["rowgemm_rt_kernel<%d,%d,%d,0>" % (m, c, kt) for m, c in DEALINGS for kt in (1, 2, 4)] +
    ["rowgemm_rt_kernel<2,4,2,4>", "rowgemm_rt_kernel<4,2,2,4>", "rowgemm_rt_kernel<2,2,1,2>", "rowgemm_rt_kernel<4,1,1,2>"])

KINDS = {"fwd": (True, True), "gi_add": (False, True), "gi": (False, False)}

# kind, N, K, M as the kernel sees them (grad-input: K = Cout is the reduction, M = Cin the output width); wide / rt: the
# tunable values the test sets; epi = (b1, add, b2) present; kernel: the instantiation reached
UnaryCase = collections.namedtuple("UnaryCase", "kind N K M wide rt epi slope kernel")
PairCase = collections.namedtuple("PairCase", "N K1 K2 M wide biases slope kernel")


def _unary(kind, N, K, M, wide, rt, epi=None, slope=SLOPE):
    WT, EPI = KINDS[kind]
    if epi is None:
        epi = {"fwd": (True, True, True), "gi_add": (False, True, False), "gi": (False, False, False)}[kind]
    if kind != "fwd":
        slope = 1.0               # d3f_linear_grad_input: no bias, no activation
    return UnaryCase(kind, N, K, M, wide, rt, epi, slope, expected_kernel(N, K, M, wide, rt, WT, EPI))


WIDTHS = (32, 64, 128, 256)
SMALL_N = (1, 15, 16, 17, 63, 130)          # one lane row, a tile less one / exact / plus one, a ragged workgroup, several
SMALL_ROWS = max(SMALL_N)
RT_N = tuple(RT_MIN_ROWS + d for d in (0, 1, 17, 47, 127))   # second tile absent, last wave empty, last workgroup partial
RT_ROWS = max(RT_N)
FWD_K = (16, 48, 1024)
GI_K = (32, 64, 256)
RT_K = (16, 32, 64)
PAIR_SHAPES = ((32, 64, 128), (16, 32, 64))
EPILOGUES = ((False, False, False), (True, False, False), (False, True, False), (False, False, True), (True, True, True))

# rowgemm_kernel (rowgemm_rt = 1): every dealing x every (WT, EPI) x reductions x row edges
ROWGEMM_CASES = [_unary(kind, N, K, M, wide, 1)
                 for kind in ("fwd", "gi_add", "gi") for M in WIDTHS for wide in (1, 2)
                 for K in (GI_K if kind == "gi" else FWD_K) for N in SMALL_N]
# the sizes the premise was worked out at: the longest reduction over many rows, and one K = 16 launch past 4096 rows
ROWGEMM_CASES += [_unary("fwd", 4223, 1024, 256, 1, 1), _unary("fwd", 4099, 16, 64, 1, 1), _unary("gi", 4099, 256, 64, 2, 1)]
# rowgemm_rt_kernel<.., 0> (rowgemm_rt = 0)
RT_CASES = [_unary("fwd", N, K, M, wide, 0) for M in WIDTHS for wide in (1, 2) for K in RT_K for N in RT_N]
# epilogue combinations, one dealing per kernel
EPILOGUE_CASES = [_unary("fwd", 130, 48, 64, 1, 1, epi) for epi in EPILOGUES] + \
                 [_unary("fwd", 130, 48, 64, 1, 1, (True, True, True), 1.0)] + \
                 [_unary("fwd", RT_MIN_ROWS + 47, 32, 128, 2, 0, epi) for epi in EPILOGUES] + \
                 [_unary("fwd", RT_MIN_ROWS + 47, 32, 128, 2, 0, (True, True, True), 1.0)]
UNARY_CASES = ROWGEMM_CASES + RT_CASES + EPILOGUE_CASES

ALL_BIASES = (True, True, True, True)


def _pair(N, K1, K2, M, wide, biases=ALL_BIASES, slope=SLOPE):
    return PairCase(N, K1, K2, M, wide, biases, slope, expected_kernel(N, (K1, K2), M, wide, 0, True, True, pair=True))


PAIR_CASES = [_pair(N, K1, K2, M, wide) for K1, K2, M in PAIR_SHAPES for wide in (1, 2) for N in RT_N]
# every subset of the four biases (none and all among them), and no activation
PAIR_EPILOGUE_CASES = [_pair(RT_MIN_ROWS + 47, 32, 64, 128, 1, b) for b in itertools.product((False, True), repeat=4)] + \
                      [_pair(RT_MIN_ROWS + 47, 16, 32, 64, 2, ALL_BIASES, 1.0)]


# ---- exact operands and their float64 results ---------------------------------------------------------------------------
def exact_ints(rng, shape, bound):
    return rng.integers(-bound, bound + 1, size=shape).astype(np.float32)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def unary_operands(kind, K, M, rows, exact=True):
    """x [rows, K], w, b1 [M], add [rows, M], b2 [M] of one (kind, K, M); a launch of N rows takes the first N rows.
    w is [M, K] for the forward (nn.Linear layout) and [K, M] for grad-input (x is then grad_out, w the layer's
    [Cout, Cin] weight as stored).  Read-only."""
    rng = np.random.default_rng([K, M, rows, len(kind), int(exact)])
    wshape = (M, K) if kind == "fwd" else (K, M)
    if exact:
        return _frozen(exact_ints(rng, (rows, K), INT_X), exact_ints(rng, wshape, INT_X), exact_ints(rng, M, INT_BIAS),
                       exact_ints(rng, (rows, M), INT_BIAS), exact_ints(rng, M, INT_BIAS))
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    return _frozen(f(rows, K), (f(*wshape) / np.sqrt(K)).astype(np.float32), f(M), f(rows, M), f(M))


def unary_product(kind, x, w, b1, add, b2, epi, slope, dtype):
    """act(x B + b1 + add + b2) in ``dtype`` arithmetic (B = w^T forward, w grad-input), the epilogue in the kernel's
    order; ``epi`` selects which of b1 / add / b2 are present."""
    t = lambda a: np.asarray(a, dtype)
    v = t(x) @ (t(w).T if kind == "fwd" else t(w))
    for on, term in zip(epi, (b1, add, b2)):
        if on:
            v = v + t(term)
    return np.where(v > 0, v, v * dtype(slope))


@functools.lru_cache(maxsize=None)
def unary_expected(kind, K, M, rows, epi, slope, exact=True):
    """[rows, M]: the float64 result (cast to float32 in the exact tier, where the cast is exact).  Read-only."""
    x, w, b1, add, b2 = unary_operands(kind, K, M, rows, exact)
    ref = unary_product(kind, x, w, b1, add, b2, epi, slope, np.float64)
    return _frozen(ref.astype(np.float32) if exact else ref)[0]


def rows_of(case):
    return SMALL_ROWS if case.N <= SMALL_ROWS else max(RT_ROWS, case.N)


@functools.lru_cache(maxsize=None)
def pair_operands(K1, K2, M, rows, exact=True):
    """x1 [rows, K1], w1 [M, K1], x2 [rows, K2], w2 [M, K2], four biases [M].  Read-only."""
    rng = np.random.default_rng([K1, K2, M, rows, int(exact)])
    if exact:
        return _frozen(exact_ints(rng, (rows, K1), INT_X), exact_ints(rng, (M, K1), INT_X),
                       exact_ints(rng, (rows, K2), INT_X), exact_ints(rng, (M, K2), INT_X),
                       *[exact_ints(rng, M, INT_BIAS) for _ in range(4)])
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    return _frozen(f(rows, K1), (f(M, K1) / np.sqrt(K1)).astype(np.float32), f(rows, K2),
                   (f(M, K2) / np.sqrt(K2)).astype(np.float32), f(M), f(M), f(M), f(M))


def pair_product(x1, w1, x2, w2, biases, on, slope, dtype):
    t = lambda a: np.asarray(a, dtype)
    v = t(x1) @ t(w1).T + t(x2) @ t(w2).T
    for use, b in zip(on, biases):
        if use:
            v = v + t(b)
    return np.where(v > 0, v, v * dtype(slope))


@functools.lru_cache(maxsize=None)
def pair_expected(K1, K2, M, rows, on, slope, exact=True):
    x1, w1, x2, w2, *biases = pair_operands(K1, K2, M, rows, exact)
    ref = pair_product(x1, w1, x2, w2, biases, on, slope, np.float64)
    return _frozen(ref.astype(np.float32) if exact else ref)[0]


# ---- first form of A^T B (the weight gradient, atb_form = 1) ----------------------------------------------------------------
def tile_width(n):
    """linear.hip:704."""
    return 4 if n % 64 == 0 else (2 if n % 32 == 0 else (1 if n % 16 == 0 else 0))


def atb_partitions(R, M, N, forced):
    """atb_partitions, linear.hip:709-724, for R <= 40000 rows (``forced`` = tunables().atb_first_form_wgs)."""
    assert R <= 40000
    nblocks = (M // (16 * tile_width(M))) * (N // (16 * tile_width(N)))
    target = forced if forced > 0 else (512 if (R >= 30000 and nblocks >= 8) else 256)
    wgs = (target + nblocks - 1) // nblocks
    return max(1, min(wgs, (R + 63) // 64, 512))


def atb_first_form(R, Cin, Cout, forced, bias):
    """What d3f_linear_grad_weight[_bias] launches at atb_form = 1 (atb_splitk_bias, linear.hip:926-961; A = grad_out so
    M = Cout, B = x so N = Cin): the partial kernel's tile, P partitions of rpw rows, the reducer, and whether trailing
    partitions start past the last row."""
    M, N = Cout, Cin
    P = atb_partitions(R, M, N, forced)
    rpw = (((R + P - 1) // P) + 3) // 4 * 4
    fan16 = P >= 64 and M * N <= 65536
    reducer = ("atb_reduce_bias_kernel[fan16=%d]" % fan16) if bias else ("atb_reduce_kernel<16>" if fan16 else "atb_reduce_kernel<4>")
    return {"partial": "atb_partial_kernel<%d,%d>" % (tile_width(M), tile_width(N)), "P": P, "rpw": rpw,
            "reducer": reducer, "past_R": (P - 1) * rpw >= R, "blocks": (M // (16 * tile_width(M)), N // (16 * tile_width(N)))}


ATB_CHANNELS = (16, 32, 64, 48, 96, 192)       # tile widths 1 / 2 / 4, one block and three blocks per side
ATB_R = (1, 5, 64, 65, 257, 4099, 4223)        # 4223: with 3 x 3 blocks and 512 forced workgroups the last of the 57
#                                                partitions of 76 rows starts at row 4256, past the operands' end
ATB_ROWS = max(ATB_R)
ATB_WGS = (0, 3, 512)
AtbCase = collections.namedtuple("AtbCase", "R Cin Cout wgs bias_blocks gb2 plan")


def _atb(R, Cin, Cout, wgs, bias_blocks=0, gb2=False):
    return AtbCase(R, Cin, Cout, wgs, bias_blocks, gb2, atb_first_form(R, Cin, Cout, wgs, bias_blocks > 0))


ATB_CASES = [_atb(R, cin, cout, wgs) for wgs in ATB_WGS for cout in ATB_CHANNELS for cin in ATB_CHANNELS for R in ATB_R]
# d3f_linear_grad_weight_bias: every tile pair, one block and three blocks a side, bias partials of 5 and of 70 rows (one
# and two trips of the 64-row column-sum loop), with and without the second bias target
ATB_BIAS_CASES = [_atb(R, cin, cout, wgs, blocks, gb2)
                  for wgs in (0, 512) for cout, cin in list(itertools.product((16, 32, 64), repeat=2)) + [(48, 192), (192, 96), (96, 48)]
                  for R in (5, 4099) for blocks, gb2 in ((5, False), (70, True), (70, False), (5, True))]


@functools.lru_cache(maxsize=None)
def atb_operands(Cin, Cout, exact=True):
    """x [ATB_ROWS, Cin], grad_out [ATB_ROWS, Cout]; a launch over R rows takes the first R.  Read-only."""
    rng = np.random.default_rng([Cin, Cout, int(exact)])
    if exact:
        return _frozen(exact_ints(rng, (ATB_ROWS, Cin), INT_ATB), exact_ints(rng, (ATB_ROWS, Cout), INT_ATB))
    return _frozen(rng.normal(size=(ATB_ROWS, Cin)).astype(np.float32), rng.normal(size=(ATB_ROWS, Cout)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def atb_expected(R, Cin, Cout, exact=True):
    """grad_w [Cout, Cin] = grad_out[:R]^T x[:R] in float64 (cast to float32 in the exact tier).  Read-only."""
    x, go = atb_operands(Cin, Cout, exact)
    ref = go[:R].astype(np.float64).T @ x[:R].astype(np.float64)
    return _frozen(ref.astype(np.float32) if exact else ref)[0]


@functools.lru_cache(maxsize=None)
def bias_partials(blocks, Cout):
    """Integer partial column sums [blocks, Cout] and their float64 column sum as float32.  Read-only."""
    part = exact_ints(np.random.default_rng([blocks, Cout]), (blocks, Cout), INT_BIAS)
    return _frozen(part, part.astype(np.float64).sum(0).astype(np.float32))


def partitioned_sum32(a, b, parts):
    """a^T b summed the way a split reduction does: ``parts`` float32 partial products over contiguous row slices,
    then added one after the other in float32."""
    edges = np.linspace(0, a.shape[0], parts + 1).astype(int)
    total = np.zeros((a.shape[1], b.shape[1]), np.float32)
    for lo, hi in zip(edges[:-1], edges[1:]):
        total = total + (a[lo:hi].T @ b[lo:hi]).astype(np.float32)
    return total


# ---- through autograd -------------------------------------------------------------------------------------------------------
AUTOGRAD_ROWS = RT_MIN_ROWS + 47
# (Cin, Cout, with add): K/16 = 2 and 4, a width with two dealings and one with a single dealing.  ops.linear_bias_act takes
# the row-streaming node only when the grad-input launch is served too (d3f_linear_fused_supported), i.e. Cin in
# {32, 64}: Cin = 16 reaches the kernels through the C entry alone
AUTOGRAD_UNARY = ((32, 64, True), (64, 256, False))
AUTOGRAD_PAIR = (32, 64, 128)
AUTOGRAD_TUNABLES = ({"rowgemm_wide": 2}, {"rowgemm_rt": 1})


@functools.lru_cache(maxsize=None)
def autograd_grad_out(M):
    """Integer upstream gradient [AUTOGRAD_ROWS, M] in [-8, 8].  Read-only."""
    return _frozen(exact_ints(np.random.default_rng([M, AUTOGRAD_ROWS]), (AUTOGRAD_ROWS, M), INT_X))[0]


def autograd_reference(fn, operands, grad_out):
    """float64 torch autograd on the CPU: ``fn`` maps a list of float64 leaves (None kept) to the output.  Returns the
    output and every leaf's gradient as float32 arrays (exact in the exact tier)."""
    import torch
    leaves = [torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(True) if a is not None else None for a in operands]
    out = fn(leaves)
    out.backward(torch.from_numpy(np.asarray(grad_out, np.float64)))
    return out.detach().numpy().astype(np.float32), [t.grad.numpy().astype(np.float32) if t is not None else None for t in leaves]
