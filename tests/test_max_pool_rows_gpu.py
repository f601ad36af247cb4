"""max_pool_fwd_v4_kernel with rows mapped to waves: every lane mapping (many rows per wave, 4 and 2 rows per wave, a
second wave of a row with one live lane, 4 waves per row), the 64-column boundaries of the index chunk, every table
width, hostile index tables, the grouped form and the replay on the same buffers.

The comparison is oracle/ops_ref.max_pool on the table truncated to the counted columns (out-of-range entries are the
shadow there too): forward bit for bit, gradient rel_err < 1e-6 (the backward adds with float atomics)."""
import numpy as np
import pytest
import torch

from d3feat_pytorch_amd import _native, ops
from oracle import ops_ref
from util import rel_err

DEV = "cuda:0"
pytestmark = pytest.mark.gpu

NS, NQ = 300, 211
CHANNELS = [4, 64, 128, 260, 1024]      # C4 = 1, 16, 32, 65, 256
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def cu(a):
    return torch.as_tensor(a).to(DEV)


def _features(C, seed):
    """Five levels, so that equal maxima in different rows of x are common (the first in row order takes the gradient;
    the level 0 also ties with the shadow); every 7th row negative, so that the shadow's zero wins wherever such rows
    are all a query sees."""
    rng = np.random.default_rng(seed)
    x = (rng.integers(-2, 3, size=(NS, C)) * 0.5).astype(np.float32)
    x[::7] = -0.5 * rng.integers(1, 3, size=x[::7].shape).astype(np.float32)
    return x


def _table(H, seed):
    """Supports, shadows (== NS), negative and too-large entries anywhere; all-shadow rows at the start, in the middle
    and at the end; rows that see only negative features; a support listed twice in a row."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, NS + 1, size=(NQ, H)).astype(np.int64)
    bad = np.array([-1, -7, I32_MIN, NS + 1, NS + 64, I32_MAX], np.int64)
    hit = rng.random(size=idx.shape) < 0.08
    idx[hit] = bad[rng.integers(0, bad.size, size=int(hit.sum()))]
    idx[:3] = NS
    idx[100] = -1
    idx[NQ - 1] = I32_MAX
    idx[5::11] = 7 * rng.integers(0, (NS + 6) // 7, size=idx[5::11].shape)          # negative rows of x only
    if H > 1:
        idx[4::9, 1] = idx[4::9, 0]                                                  # twice, side by side
        idx[6::9, H - 1] = idx[6::9, 0]                                              # twice, at both ends
    return idx.astype(np.int32)


def _as_oracle_table(idx, w):
    """The first min(max(w, 1), H) columns, every entry outside [0, NS) named as the shadow row."""
    t = idx[:, :min(max(w, 1), idx.shape[1])].astype(np.int64)
    return torch.from_numpy(np.where((t < 0) | (t >= NS), NS, t))


_X = {}
_GO = {}


def _x(C):
    if C not in _X:
        _X[C] = _features(C, 1000 + C)
        _GO[C] = np.random.default_rng(2000 + C).normal(size=(NQ, C)).astype(np.float32)
    return _X[C], _GO[C]


def _oracle(x, table, go):
    tx = torch.from_numpy(x).requires_grad_(True)
    ref = ops_ref.max_pool(tx, table)
    ref.backward(torch.from_numpy(go))
    return ref.detach().numpy(), tx.grad.numpy()


@pytest.mark.parametrize("H", [1, 7, 64, 65, 96])
@pytest.mark.parametrize("C", CHANNELS)
def test_max_pool_rows_equal_the_oracle_for_every_mapping_chunk_and_width(C, H):
    """width = 1, H - 1, H and H + 3 (device int32[1]) on tables of 1, 7, 64, 65 and 96 columns: one group of 4 and
    of 8 gathers, the last column of the first 64-column load, the first of the second, and for C4 < 32 more than one
    pair of loads."""
    x, go = _x(C)
    idx = _table(H, 10 * H + 1)
    for w in sorted({1, max(H - 1, 1), H, H + 3}):
        want, want_gx = _oracle(x, _as_oracle_table(idx, w), go)
        gx = cu(x).requires_grad_(True)
        out = ops.max_pool(gx, cu(idx), width=torch.tensor([w], dtype=torch.int32, device=DEV))
        out.backward(cu(go))
        assert np.array_equal(out.detach().cpu().numpy(), want), w
        assert rel_err(gx.grad.cpu().numpy(), want_gx) < 1e-6, w
    want, want_gx = _oracle(x, _as_oracle_table(idx, H), go)                        # no width: the whole table
    gx = cu(x).requires_grad_(True)
    out = ops.max_pool(gx, cu(idx))
    out.backward(cu(go))
    assert np.array_equal(out.detach().cpu().numpy(), want)
    assert rel_err(gx.grad.cpu().numpy(), want_gx) < 1e-6


@pytest.mark.parametrize("C", CHANNELS)
def test_grouped_max_pool_rows_equal_the_oracle_on_each_group_s_table(C):
    """4 clouds in 2 groups with widths (5, 12) through ``groups``: the second cloud starts at row 60 and the second
    group at row 111, inside the row block of a wave for every mapping that has one (2, 4 and 64 rows per wave).
    Every group against the oracle on its own truncated table."""
    H = 17
    x, go = _x(C)
    idx = _table(H, 17)
    lens_q = np.array([60, 51, 70, 30], np.int32)
    assert int(lens_q.sum()) == NQ
    widths = np.array([5, 12], np.int32)
    gx = cu(x).requires_grad_(True)
    out = ops.max_pool(gx, cu(idx), width=cu(widths), groups=(cu(lens_q), 2))
    out.backward(cu(go))
    got = out.detach().cpu().numpy()
    want_gx = np.zeros_like(x)
    q0 = 0
    for g in range(2):
        q1 = q0 + int(lens_q[2 * g:2 * g + 2].sum())
        want, part = _oracle(x, _as_oracle_table(idx[q0:q1], int(widths[g])), go[q0:q1])
        assert np.array_equal(got[q0:q1], want), g
        want_gx += part
        q0 = q1
    assert rel_err(gx.grad.cpu().numpy(), want_gx) < 1e-6


@pytest.mark.parametrize("C", [128, 1024])
def test_max_pool_rows_replay_on_the_same_buffers(C):
    """Forward + backward twice through the C ABI on the same out / argmax / gradient buffers, the gradient buffer
    full of NaN before the first run and holding the first gradient before the second: the output repeats bit for
    bit and the gradient within 1e-6, which it can only do if the forward launch cleared the scatter target."""
    H = 65
    x, go = _x(C)
    idx = _table(H, 651)
    want, want_gx = _oracle(x, _as_oracle_table(idx, 40), go)
    dx, di, dgo = cu(x), cu(idx), cu(go)
    width = torch.tensor([40], dtype=torch.int32, device=DEV)
    out = torch.empty((NQ, C), dtype=torch.float32, device=DEV)
    arg = torch.empty((NQ, C), dtype=torch.int32, device=DEV)
    gx = torch.full((NS, C), float("nan"), dtype=torch.float32, device=DEV)
    lib, stream = _native.lib(), torch.cuda.current_stream().cuda_stream
    runs = []
    for _ in range(2):
        _native.check(lib.d3f_max_pool_forward(dx.data_ptr(), NS, C, di.data_ptr(), NQ, H, out.data_ptr(),
                                               arg.data_ptr(), gx.data_ptr(), width.data_ptr(), None, 0, 0, stream),
                      "d3f_max_pool_forward")
        _native.check(lib.d3f_max_pool_backward(dgo.data_ptr(), arg.data_ptr(), NQ, C, NS, gx.data_ptr(), 1, stream),
                      "d3f_max_pool_backward")
        runs.append((out.cpu().numpy(), gx.cpu().numpy()))
    assert np.array_equal(runs[0][0], want)
    assert rel_err(runs[0][1], want_gx) < 1e-6
    assert np.array_equal(runs[1][0], runs[0][0])
    assert rel_err(runs[1][1], runs[0][1]) < 1e-6
