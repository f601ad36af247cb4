"""Inputs for the KPConv kernel tests (test_gpu_ops.py, test_kpconv_cases_cpu.py).

``_kpconv_case`` is the generator the KPConv tests started with: a neighbour table of RANDOM supports.  With an extent of
0.05 in a unit cube almost every influence weight is zero (under 0.1 % are not), four output rows in five are exactly
zero and a non-zero row holds a single term: no sum over neighbours is ever a sum.  It is kept as it was, number for
number, because it covers what it covers (duplicate entries in a row, shadows in any proportion).

``dense_case`` builds what a radius search would: every row holds the nearest supports inside a ball whose expected
population is the table width, kernel points and extent in the proportions of the network (kernel points inside
0.66 r, extent 0.48 r).  About one weight in ten is non-zero, every output row is a sum of many terms and every support
receives gradient from many rows; ``input_stats`` measures that and test_kpconv_cases_cpu.py holds every shape of the
GPU tests to it.  The exception is the one-column table (h = 1, ball filled for ``H_FILL``): a row is then one
neighbour's term per kernel point at most, a row whose only neighbour lies beyond every kernel point's extent is zero
(8.8 % of the rows at (600, 300, 1)), and the CPU test asks of those tables what one column can give."""
import numpy as np
import torch

from oracle import ops_ref

SPARSE_EXTENT = 0.05
SHIFT = (300.0, -200.0, 50.0)    # the offset test_icp_gpu.py moves its scenes by

# ---- shapes (nq, ns, h, cin, cout) of the parametrised KPConv tests of test_gpu_ops.py, both geometries -------------
FWD_BWD_SHAPES = [(700, 900, 42, 1, 64), (1000, 1000, 42, 32, 32), (333, 1000, 37, 64, 64), (257, 300, 45, 128, 128),
                  (97, 154, 23, 512, 512), (500, 500, 9, 16, 8), (200, 260, 42, 24, 40), (300, 400, 42, 16, 16),
                  (300, 400, 40, 32, 64), (150, 160, 42, 256, 128), (2100, 2100, 42, 64, 32), (571, 2053, 42, 128, 128),
                  (900, 900, 42, 1, 32), (400, 500, 30, 2, 100), (300, 300, 42, 4, 64), (300, 300, 17, 3, 8)]
GATHER_SHAPES = [(1000, 1000, 42, 32, 32), (333, 1000, 37, 64, 64), (4500, 4500, 42, 64, 64), (257, 300, 45, 128, 128),
                 (97, 154, 23, 512, 512), (300, 400, 42, 16, 16), (300, 400, 40, 32, 64), (150, 160, 42, 256, 128),
                 (2100, 2100, 42, 64, 32), (571, 2053, 42, 128, 128), (5000, 900, 64, 32, 32)]
SAVED_WF_SHAPES = [(1000, 1000, 42, 32, 32), (97, 154, 23, 512, 512), (300, 400, 42, 16, 16), (150, 160, 42, 256, 128),
                   (200, 260, 42, 24, 40)]
BIAS_ACT_SHAPES = [(97, 154, 23, 512, 512), (150, 160, 42, 256, 128), (300, 400, 42, 16, 16), (257, 300, 45, 128, 128),
                   (571, 2053, 42, 64, 256)]
SHADOW_ROWS_SHAPE = (64, 80, 10, 32, 32)
# A table of 9 or 10 columns cannot give 15 kernel points two neighbours each (about one neighbour in nine lies within
# the extent of a kernel point): the dense twins of these two shapes are wider, the bar of the CPU test stays.
DENSE_TWIN = {(500, 500, 9, 16, 8): (500, 500, 17, 16, 8), SHADOW_ROWS_SHAPE: (64, 80, 20, 32, 32)}


# ---- dense geometry only: shapes the matrix lacked -------------------------------------------------------------------
K_VALUES = [1, 7, 16]
K_SHAPES = [(300, 400, 42, 32, 32),     # fused tile kernels
            (300, 400, 42, 2, 64),      # input-layer kernels, saved 16-slot wf
            (300, 300, 17, 3, 8),       # input-layer kernels, their own weight-gradient kernel
            (200, 260, 42, 24, 40)]     # general path
K1_WIDTH = 64   # K = 1 keeps the centre point: one neighbour in nine contributes, and only a table of 64 columns gives
#                 nine supports in ten their second contribution (measured at 42 columns: 88 - 90 %)
K_CASES = [(nq, ns, K1_WIDTH if k == 1 else h, cin, cout, k) for nq, ns, h, cin, cout in K_SHAPES for k in K_VALUES]
H_VALUES = [1, 64, 65, 70]              # 64: last width of the fused / input-layer kernels, 65: first of the general path
H_FILL = 8                              # population of the ball when the table keeps one neighbour (h = 1)
# (nq, ns, h, cin, cout).  With nq <= ns the queries sit on DISTINCT supports, so at h = 1 no support is named twice:
# the two 600-query cases (uniform queries, two per support) are there for the collisions of the scatter.
H_CASES = [(300, 400, h, cin, cout) for cin, cout in ((32, 32), (1, 64)) for h in H_VALUES] + \
          [(600, 300, 1, 32, 32), (600, 300, 1, 1, 64)]
WIDE_SHAPES = [(150, 200, 30, 192, 96),   # 4 channels per lane
               (97, 154, 23, 320, 48), (97, 154, 23, 500, 24),        # 8 channels per lane
               (150, 200, 30, 128, 96)]   # wide Cin the fused kernels serve, a Cout they do not
SMALL_EDGE_SHAPES = [(300, 400, 42, 2, 128),   # two outputs per lane, saved wf
                     (300, 400, 42, 4, 64),
                     (300, 400, 42, 4, 65), (300, 400, 42, 3, 128),   # just outside: general path
                     (300, 400, 42, 1, 33)]    # Cout no multiple of 16: weight gradient by the input-layer kernel
SHIFT_SHAPES = {'fused': (300, 400, 42, 32, 32), 'small': (300, 400, 42, 1, 64), 'general': (200, 260, 42, 24, 40),
                'gather': (300, 400, 42, 32, 32), 'aggregate_gemm': (300, 400, 42, 64, 64)}


def dense_geometries():
    """Every (nq, ns, h, k, h_fill) the dense GPU tests build a table for (the CPU test checks each once)."""
    geo = []
    for shapes in (FWD_BWD_SHAPES, GATHER_SHAPES, SAVED_WF_SHAPES, BIAS_ACT_SHAPES, [SHADOW_ROWS_SHAPE]):
        geo += [DENSE_TWIN.get(s, s)[:3] + (15, None) for s in shapes]
    for shapes in (WIDE_SHAPES, SMALL_EDGE_SHAPES, list(SHIFT_SHAPES.values())):
        geo += [s[:3] + (15, None) for s in shapes]
    geo += [(nq, ns, h, k, None) for nq, ns, h, _, _, k in K_CASES]
    geo += [(nq, ns, h, 15, H_FILL if h == 1 else None) for nq, ns, h, _, _ in H_CASES]
    return sorted(set(geo), key=lambda g: (g[0], g[1], g[2], g[3], g[4] or 0))


def _cloud(rng, n):
    return (rng.random((n, 3)) * np.asarray((1, 1, 1))).astype(np.float32)


def _kpconv_case(rng, nq, ns, h, cin, cout, shadow_frac=0.15, k=15):
    """q, s, idx(int64), x, kp, w: a table of random supports (extent to use: SPARSE_EXTENT)."""
    q, s = _cloud(rng, nq), _cloud(rng, ns)
    idx = rng.integers(0, ns, size=(nq, h))
    # supports near SOME query (not near the queries whose rows name them: see the module docstring)
    s_near = q[rng.integers(0, nq, size=ns)] + rng.normal(scale=0.03, size=(ns, 3)).astype(np.float32)
    s = s_near.astype(np.float32)
    shadow = rng.random((nq, h)) < shadow_frac
    idx[shadow] = ns
    idx.sort(axis=1)  # shadows (== ns) at the row end like real tables (not required by the kernel)
    x = rng.normal(size=(ns, cin)).astype(np.float32)
    x[rng.random(ns) < 0.1] = 0.0  # rows with zero feature sum exercise the neighbor_num rule
    kp = (rng.normal(size=(k, 3)) * 0.03).astype(np.float32)
    kp[0] = 0
    w = (rng.normal(size=(k, cin, cout)) / np.sqrt(cin * k)).astype(np.float32)
    return q, s, idx.astype(np.int64), x, kp, w


def dense_rng(nq, ns, h, k=15):
    """The generator of one dense case: the same table and kernel points wherever that geometry is built."""
    return np.random.default_rng([nq, ns, h, k])


def nearest_table(q, s, h, r, chunk=512):
    """[nq, h] int64: the h nearest supports of every query in ascending float64 distance (stable: equal distances keep
    the support order), entries at d >= r replaced by the shadow index ns.  Brute force, ``chunk`` queries at a time."""
    nq, ns = q.shape[0], s.shape[0]
    q64, s64 = q.astype(np.float64), s.astype(np.float64)
    idx = np.full((nq, h), ns, np.int64)
    w = min(h, ns)
    for a in range(0, nq, chunk):
        d2 = ((q64[a:a + chunk, None, :] - s64[None, :, :]) ** 2).sum(axis=2)
        if ns > 4 * w:   # the w nearest first, in support order, so that the stable sort of those few ends the same
            cand = np.sort(np.argpartition(d2, w - 1, axis=1)[:, :w], axis=1)
            order = np.take_along_axis(cand, np.argsort(np.take_along_axis(d2, cand, axis=1), axis=1, kind='stable'), axis=1)
        else:
            order = np.argsort(d2, axis=1, kind='stable')[:, :w]
        near = np.take_along_axis(d2, order, axis=1)
        idx[a:a + chunk, :w] = np.where(near < r * r, order, ns)
    return idx


def dense_case(rng, nq, ns, h, cin, cout, k=15, shift=(0, 0, 0), h_fill=None):
    """q, s, idx(int64), x, kp, w, extent: radius-search rows over uniform supports.  ``h_fill``: expected population of
    the ball (default: the table width h).  ``shift`` moves q and s AFTER the table is built."""
    s = rng.random((ns, 3)).astype(np.float32)
    if nq <= ns:
        # half the queries ARE supports (d = 0, the point itself leads its row), half lie 0.01 off one
        q = s[rng.permutation(ns)[:nq]].copy()
        q[nq // 2:] += rng.normal(scale=0.01, size=(nq - nq // 2, 3)).astype(np.float32)
    else:
        q = rng.random((nq, 3)).astype(np.float32)
    r = ((h_fill or h) / (ns * 4.0 * np.pi / 3.0)) ** (1.0 / 3.0)
    idx = nearest_table(q, s, h, r)
    d = rng.normal(size=(k, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    kp = (d * (0.66 * r * rng.random((k, 1)) ** (1.0 / 3.0))).astype(np.float32)
    kp[0] = 0
    x = rng.normal(size=(ns, cin)).astype(np.float32)
    x[rng.random(ns) < 0.1] = 0.0  # rows with zero feature sum exercise the neighbor_num rule
    w = (rng.normal(size=(k, cin, cout)) / np.sqrt(cin * k)).astype(np.float32)
    sh = np.asarray(shift, np.float64)
    q = (q.astype(np.float64) + sh).astype(np.float32)
    s = (s.astype(np.float64) + sh).astype(np.float32)
    return q, s, idx, x, kp, w, float(0.48 * r)


def influence_weights(q, s, idx, kp, extent):
    """[nq, h, k] float64 'linear' influence weights of a table, 0 at shadow entries."""
    ns = s.shape[0]
    s_pad = np.concatenate([s.astype(np.float64), np.full((1, 3), 1e6)], 0)
    rel = s_pad[np.minimum(idx, ns)] - q.astype(np.float64)[:, None, :]
    d = np.sqrt(((rel[:, :, None, :] - kp.astype(np.float64)[None, None]) ** 2).sum(axis=3))
    return np.where((idx < ns)[:, :, None], np.maximum(0.0, 1.0 - d / extent), 0.0)


def input_stats(q, s, idx, kp, extent):
    """What a table gives the kernels to do, in float64:
      nonzero      share of the nq * h * k influence weights that are > 0
      zero_rows    share of queries without any contributing neighbour (their output row is exactly zero)
      sums_ge1/2   share of (query, kernel point) sums over h with at least one / two non-zero terms
      supports_ge2 share of supports that receive a gradient contribution from at least two table entries"""
    ns = s.shape[0]
    live = influence_weights(q, s, idx, kp, extent) > 0
    terms = live.sum(axis=1)                                   # [nq, k]
    edges = idx[live.any(axis=2)]                              # table entries with some non-zero weight
    return {'nonzero': float(live.mean()), 'zero_rows': float((terms.sum(axis=1) == 0).mean()),
            'sums_ge1': float((terms >= 1).mean()), 'sums_ge2': float((terms >= 2).mean()),
            'supports_ge2': float((np.bincount(edges, minlength=ns)[:ns] >= 2).mean())}


def oracle64(q, s, idx, x, kp, w, extent, grad_out=None, bias=None, slope=None):
    """ops_ref.kpconv on float64 copies of float32 inputs (optionally LeakyReLU(. + bias) in float64 as well):
    (out, grad_x, grad_w, grad_bias) as float64 arrays, the gradients for a float64 copy of ``grad_out``."""
    t = lambda a: torch.from_numpy(np.asarray(a)).double()
    tx, tw = t(x).requires_grad_(True), t(w).requires_grad_(True)
    tb = t(bias).requires_grad_(True) if bias is not None else None
    out = ops_ref.kpconv(t(q), t(s), torch.from_numpy(idx), tx, t(kp), tw, float(extent))
    if tb is not None:
        out = torch.nn.functional.leaky_relu(out + tb, slope)
    if grad_out is None:
        return out.detach().numpy(), None, None, None
    out.backward(t(grad_out))
    return out.detach().numpy(), tx.grad.numpy(), tw.grad.numpy(), (tb.grad.numpy() if tb is not None else None)
