"""The radius search where its cell table is SMALL: 64 or 128 buckets, so that the 27 cells of one query share buckets
with each other and with the cells of other clouds.  The kernel scans every distinct bucket once and accepts a candidate
iff it belongs to the query's cloud and d2 < r2 (csrc/radius_neighbors.hip, head of the file); the tests of
test_gpu_ops.py use >= 1500 supports (>= 4096 buckets), where two cells of a query almost never meet.

Every table is compared with np.array_equal against the CPU oracle and against a NumPy brute force in float32 with the
kernel's expression ((dx*dx)+(dy*dy))+(dz*dz) and its (d2 bits, index) order.  The conditions on the INPUTS (bucket
sharing, supports of other clouds inside the radius, row lengths around the cuts of the ranking networks) are
restated in NumPy from csrc/cell_list.hpp and asserted without a GPU."""
import functools

import numpy as np
import pytest
import torch

from d3feat_pytorch_amd import _native, ops

DEV = "cuda:0"
gpu = pytest.mark.gpu
U64 = np.uint64
NO_NEAREST = 32     # D3F_ST_NO_NEAREST of include/d3feat_hip.h


def cu(a):
    return torch.as_tensor(np.array(a)).to(DEV)      # (a copy: the shared inputs are read-only)


# ---------------------------------------------------------------------------------------- the search restated in NumPy
def _d2(q, s):
    """float32 ((dx*dx)+(dy*dy))+(dz*dz) of one query against rows of supports, no fused multiply-add"""
    d = (q[None, :] - s).astype(np.float32)
    return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float32)


def brute_keys(q, s, ql, sl, radius):
    """per query (rows past sum(ql): None) the uint64 keys (d2 bits << 32 | global support index) of the supports of
    the same cloud with d2 < float32(radius)^2, ascending"""
    r2 = np.float32(radius) * np.float32(radius)
    qo, so = np.concatenate([[0], np.cumsum(ql)]), np.concatenate([[0], np.cumsum(sl)])
    rows = [None] * q.shape[0]
    for b in range(len(ql)):
        sup = s[so[b]:so[b + 1]]
        for i in range(qo[b], qo[b + 1]):
            d2 = _d2(q[i], sup)
            keep = np.nonzero(d2 < r2)[0]
            keys = (d2[keep].view(np.uint32).astype(U64) << U64(32)) | (keep + so[b]).astype(U64)
            rows[i] = np.sort(keys)
    return rows


def table_of(rows, width, ns):
    out = np.full((len(rows), width), ns, np.int32)
    for i, k in enumerate(rows):
        if k is not None:
            n = min(width, k.size)
            out[i, :n] = (k[:n] & U64(0xffffffff)).astype(np.int32)
    return out


def counts_of(rows):
    return np.array([0 if k is None else k.size for k in rows], np.int32)


def last_keys_of(rows, width):
    """d3f_radius_query_ex's out_last_key: the key of the last entry a capped row keeps; ~0 when it keeps everything"""
    out = np.full(len(rows), ~U64(0), U64)
    for i, k in enumerate(rows):
        if k is not None and k.size > width:
            out[i] = k[width - 1]
    return out


def table_size_for(ns):
    m = 64
    while m < 2 * max(ns, 1):
        m <<= 1
    return m


def pack_key(b, cx, cy, cz):
    return (U64(b) << U64(48)) | (U64(cx + 32768) << U64(32)) | (U64(cy + 32768) << U64(16)) | U64(cz + 32768)


def bucket_of(key, mask):
    with np.errstate(over="ignore"):
        return int(((U64(key) * U64(0x9E3779B97F4A7C15)) >> U64(32)) & U64(mask))


def cell_of(p, inv_cell):
    return np.floor(p.astype(np.float64) * inv_cell).astype(np.int64)


def scanned_buckets(qpt, b, radius, mask):
    """[(bucket, cell)] of the cells of the 27 around `qpt` whose box lies within the radius (the kernel's pruning)"""
    cell = np.float64(np.float32(radius)) * (1.0 + 1e-4)
    inv_cell = 1.0 / cell
    cell = 1.0 / inv_cell
    c0 = cell_of(qpt, inv_cell)
    reach = np.float64(np.float32(radius)) * (1.0 + 1e-4)
    out = []
    for lane in range(27):
        c = c0 + np.array([lane % 3 - 1, (lane // 3) % 3 - 1, lane // 9 - 1])
        lo = c.astype(np.float64) * cell
        hi = lo + cell
        x = qpt.astype(np.float64)
        g = np.where(x < lo, lo - x, np.where(x > hi, x - hi, 0.0))
        if float((g * g).sum()) <= reach * reach:
            out.append((bucket_of(pack_key(b, int(c[0]), int(c[1]), int(c[2])), mask), tuple(int(v) for v in c)))
    return out


def input_conditions(q, s, ql, sl, radius):
    """(queries for which two different scanned cells share a bucket that holds an accepted support,
        supports of ANOTHER cloud within the radius of a query and inside a bucket the query scans,
        flat candidate totals per query = the supports stored in the distinct scanned buckets)"""
    ns = int(np.sum(sl))
    mask = table_size_for(s.shape[0]) - 1
    inv_cell = 1.0 / (np.float64(np.float32(radius)) * (1.0 + 1e-4))
    so = np.concatenate([[0], np.cumsum(sl)])
    cloud = np.repeat(np.arange(len(sl)), sl)
    cells = cell_of(s[:ns], inv_cell)
    sb = np.array([bucket_of(pack_key(int(cloud[i]), *[int(v) for v in cells[i]]), mask) for i in range(ns)], np.int64)
    r2 = np.float32(radius) * np.float32(radius)
    shared = foreign = 0
    totals = []
    qo = np.concatenate([[0], np.cumsum(ql)])
    for b in range(len(ql)):
        for i in range(qo[b], qo[b + 1]):
            sc = scanned_buckets(q[i], b, radius, mask)
            buckets = {}
            for bk, c in sc:
                buckets.setdefault(bk, []).append(c)
            d2 = _d2(q[i], s[:ns])
            inb = np.isin(sb, list(buckets))
            totals.append(int(inb.sum()))
            acc = (d2 < r2) & (cloud == b)
            if any(len(c) > 1 and bool((acc & (sb == bk)).any()) for bk, c in buckets.items()):
                shared += 1
            foreign += int(((d2 < r2) & (cloud != b) & inb).sum())
    return shared, foreign, np.array(totals)


# --------------------------------------------------------------------------------------------------------- tiny tables
# (supports per cloud, radius, seed): 27 .. 62 supports in all, i.e. tables of 64 or 128 buckets; the clouds overlap
TINY = [((7, 20), 0.30, 1), ((31, 31), 0.8, 2), ((1, 2, 31), 0.25, 3), ((31, 20, 7), 0.60, 4), ((2, 7), 0.9, 5),
        ((20, 31, 1), 0.16, 6)]


@functools.lru_cache(maxsize=None)
def tiny_case(k):
    sl, radius, seed = TINY[k]
    rng = np.random.default_rng(100 + seed)
    sl = np.array(sl, np.int32)
    s = (rng.random((int(sl.sum()), 3)) - 0.5).astype(np.float32)          # every cloud fills the same unit cube
    extra = np.array([40] * len(sl), np.int32)
    far = ((rng.random((int(extra.sum()), 3)) - 0.5) * 1.6).astype(np.float32)
    # per cloud: the supports themselves, then queries of their own (some outside the cube: short and empty rows)
    so, eo = np.concatenate([[0], np.cumsum(sl)]), np.concatenate([[0], np.cumsum(extra)])
    q = np.concatenate([np.concatenate([s[so[b]:so[b + 1]], far[eo[b]:eo[b + 1]]]) for b in range(len(sl))])
    ql = (sl + extra).astype(np.int32)
    rows = brute_keys(q, s, ql, sl, radius)
    for a in (q, s, ql, sl):
        a.setflags(write=False)
    return q, s, ql, sl, radius, rows


def test_tiny_inputs_share_buckets_and_meet_other_clouds():
    shared = foreign = 0
    longest, shortest = 0, 1 << 30
    for k in range(len(TINY)):
        q, s, ql, sl, radius, rows = tiny_case(k)
        assert table_size_for(s.shape[0]) in (64, 128)
        a, b, _ = input_conditions(q, s, ql, sl, radius)
        shared, foreign = shared + a, foreign + b
        c = counts_of(rows)
        longest, shortest = max(longest, int(c.max())), min(shortest, int(c[c > 0].min()))
    assert shared >= 20 and foreign >= 20
    assert shortest == 1 and longest >= 30


@gpu
@pytest.mark.parametrize("k", range(len(TINY)))
def test_tiny_tables_full_wide_and_transposed_forms(native, k):
    q, s, ql, sl, radius, rows = tiny_case(k)
    ns, cnt = s.shape[0], counts_of(rows)
    oracle = native.batch_query(q, s, ql, sl, radius=radius, max_neighbors=0)
    assert np.array_equal(oracle, table_of(rows, int(cnt.max()), ns))        # the two references agree
    grid = ops.RadiusGrid(cu(s), cu(sl), radius)
    for width in (3, int(cnt.max()), int(cnt.max()) + 5):
        tab, counts, mx, lkey = grid.query(cu(q), cu(ql), width, want_counts=True, want_max=True, want_last_key=True)
        assert np.array_equal(tab.cpu().numpy(), table_of(rows, width, ns)), width
        assert np.array_equal(counts.cpu().numpy(), cnt)
        assert mx.cpu().numpy().tolist() == [int(cnt.max())]
        assert np.array_equal(lkey.cpu().numpy().view(U64), last_keys_of(rows, width)), width
    tab, wide = grid.query(cu(q), cu(ql), 4, wide=int(cnt.max()))
    assert np.array_equal(tab.cpu().numpy(), table_of(rows, 4, ns))
    assert np.array_equal(wide.cpu().numpy(), oracle)
    _, mxg = grid.query(cu(q), cu(ql), 4, want_max=True, max_group=1)          # max count per cloud
    qo = np.concatenate([[0], np.cumsum(ql)])
    assert mxg.cpu().numpy().tolist() == [int(cnt[qo[b]:qo[b + 1]].max()) for b in range(len(ql))]
    # the pooling form: the same table, and per support the (d2 bits, query) keys of the queries that found it.  Queries
    # = the supports themselves (at most 31 per cloud: no list outgrows its 32 slots)
    srows = brute_keys(s, s, sl, sl, radius)
    width = max(1, int(counts_of(srows).max()) - 2)
    tab, mx, lkey, (tc, tk) = grid.query_pool_transposed(cu(s), cu(sl), width)
    assert np.array_equal(tab.cpu().numpy(), table_of(srows, width, ns))
    assert mx.cpu().numpy().tolist() == [int(counts_of(srows).max())]
    assert np.array_equal(lkey.cpu().numpy().view(U64), last_keys_of(srows, width))
    tc, tk = tc.cpu().numpy(), tk.cpu().numpy().view(U64).reshape(ns, 32)
    want = [[] for _ in range(ns)]
    for qi, keys in enumerate(srows):
        for key in keys:
            want[int(key & U64(0xffffffff))].append((key & U64(0xffffffff00000000)) | U64(qi))
    for f in range(ns):
        assert tc[f] == len(want[f]) <= 32
        assert np.array_equal(np.sort(tk[f, :tc[f]]), np.sort(np.array(want[f], U64))), f
    grid.status.raise_if_set()


@gpu
@pytest.mark.parametrize("k", range(len(TINY)))
def test_tiny_tables_prefix_form(k):
    q, s, ql, sl, radius, rows = tiny_case(k)
    ns = s.shape[0]
    prefix = 0.6 * radius
    p2 = np.float32(prefix) * np.float32(prefix)

    def expected(bound):
        within = rows if bound is None else brute_keys(q, s, ql, sl, bound)
        out = []
        for keys in within:
            d2 = (keys >> U64(32)).astype(np.uint32).view(np.float32)
            lead = keys[d2 < p2]
            out.append(lead if lead.size else keys[:1])
        return out

    for width in (2, 12):
        grid = ops.RadiusGrid(cu(s), cu(sl), radius)
        got = grid.query_prefix(cu(q), cu(ql), width, prefix).cpu().numpy()
        assert np.array_equal(got, table_of(expected(None), width, ns)), width
        grid.status.raise_if_set()
        bound = 0.8 * radius                      # with a nearest bound: nothing beyond it is looked at ...
        want = expected(bound)
        got = grid.query_prefix(cu(q), cu(ql), width, prefix, nearest_bound=bound).cpu().numpy()
        assert np.array_equal(got, table_of(want, width, ns)), width
        flagged = int(grid.status.word.item())     # ... and a query without a support inside it is reported
        assert flagged == (NO_NEAREST if any(k_.size == 0 for k_ in want) else 0)


# ------------------------------------------------------------------------------------ pass and network boundaries
@functools.lru_cache(maxsize=None)
def boundary_case():
    """One cloud of 600 points in a cube of side 2.5 r (+ 6 copies of one of them: equal d2, ordered by index), an EMPTY
    cloud, a third small cloud; queries = the supports and as many points around the cube; capacity rows past the live
    ones on both sides."""
    rng = np.random.default_rng(2025)
    radius = 0.2
    side = 2.5 * radius
    a = (rng.random((600, 3)) * side).astype(np.float32)
    a = np.concatenate([a, np.repeat(a[17:18], 6, 0)])
    c = (rng.random((45, 3)) * side).astype(np.float32)
    around = ((rng.random((600, 3)) * 2.2 - 0.6) * side).astype(np.float32)
    sl = np.array([a.shape[0], 0, c.shape[0]], np.int32)
    ql = np.array([a.shape[0] + around.shape[0], 0, c.shape[0]], np.int32)
    pad = np.full((9, 3), 0.25 * side, np.float32)
    s = np.concatenate([a, c, pad])
    q = np.concatenate([a, around, c, pad])
    rows = brute_keys(q, s, ql, sl, radius)
    for arr in (q, s, ql, sl):
        arr.setflags(write=False)
    return q, s, ql, sl, radius, rows


def test_boundary_inputs_straddle_the_passes_and_the_network_cuts():
    q, s, ql, sl, radius, rows = boundary_case()
    cnt = counts_of(rows)
    for n in (15, 16, 17, 31, 32, 33, 63, 64, 65):
        assert (cnt == n).any(), n
    assert cnt.max() > 128 and (cnt[:int(ql.sum())] == 0).any() and all(r is None for r in rows[int(ql.sum()):])
    dup = rows[17]                               # the copies of point 17: d2 == 0 seven times, ascending index
    assert np.array_equal(dup[:7], np.array([17, 600, 601, 602, 603, 604, 605], U64))
    _, _, totals = input_conditions(q[:int(ql[0])], s, ql[:1], sl, radius)
    for lo, hi in ((1, 64), (65, 128), (129, 192), (193, 1 << 30)):
        assert ((totals >= lo) & (totals <= hi)).any(), (lo, hi)


@gpu
def test_boundary_rows_in_registers_and_in_lds(native):
    q, s, ql, sl, radius, rows = boundary_case()
    ns, live = s.shape[0], int(ql.sum())
    cnt = counts_of(rows)
    oracle = native.batch_query(q[:live], s[:int(sl.sum())], ql, sl, radius=radius, max_neighbors=0)
    full = table_of(rows, int(cnt.max()), ns)
    assert np.array_equal(np.where(oracle == int(sl.sum()), ns, oracle), full[:live])
    grid = ops.RadiusGrid(cu(s), cu(sl), radius)
    for width in (16, 64, 70, int(cnt.max())):
        tab, counts, mx, lkey = grid.query(cu(q), cu(ql), width, want_counts=True, want_max=True, want_last_key=True)
        assert np.array_equal(tab.cpu().numpy(), full[:, :width]), width
        assert np.array_equal(counts.cpu().numpy(), cnt)
        assert mx.cpu().numpy().tolist() == [int(cnt.max())]
        assert np.array_equal(lkey.cpu().numpy().view(U64), last_keys_of(rows, width)), width
    wide = grid.query(cu(q), cu(ql), 8, wide=int(cnt.max()), table=False)
    assert np.array_equal(wide.cpu().numpy(), full)          # rows of more than 64 entries: ranked in LDS
    prefix = 0.5 * radius
    p2 = np.float32(prefix) * np.float32(prefix)
    want = []
    for keys in rows:
        if keys is None:
            want.append(None)
            continue
        lead = keys[(keys >> U64(32)).astype(np.uint32).view(np.float32) < p2]
        want.append(lead if lead.size else keys[:1])
    got = grid.query_prefix(cu(q), cu(ql), 40, prefix).cpu().numpy()
    assert np.array_equal(got, table_of(want, 40, ns))
    grid.status.raise_if_set()


# -------------------------------------------------------------------------------------------------- up_rank_kernel
@gpu
@pytest.mark.parametrize("width", [5, 32, 40])
def test_upsample_rows_rank_against_a_host_sort(width):
    rng = np.random.default_rng(31)
    sizes = [0, 1, 2, 31, 32, 33] * 3 + [7, 0, 33]           # (21 lists: the last workgroup is not full)
    nf, nc = len(sizes), 5000
    keys = np.zeros((nf, 32), U64)
    for f, n in enumerate(sizes):
        bits = rng.random(32).astype(np.float32)
        bits[rng.integers(0, 32, 12)] = bits[3]                # equal distance bits: ordered by the coarse index
        idx = rng.permutation(nc)[:32]
        keys[f] = (bits.view(np.uint32).astype(U64) << U64(32)) | idx.astype(U64)
    counts = cu(np.array(sizes, np.int32))
    up = torch.full((nf, width), -7, dtype=torch.int32, device=DEV)
    _native.check(_native.lib().d3f_upsample_rows_rank(counts.data_ptr(), cu(keys.view(np.int64)).data_ptr(), nf, nc,
                                                       width, up.data_ptr(), ops._stream()), "d3f_upsample_rows_rank")
    up, counts = up.cpu().numpy(), counts.cpu().numpy()
    for f, n in enumerate(sizes):
        if n == 0 or n > 32:                                   # left for the search that follows; an overlong list counts 0
            assert (up[f] == -7).all() and counts[f] == 0
            continue
        want = np.full(width, nc, np.int32)
        ranked = (np.sort(keys[f, :n]) & U64(0xffffffff)).astype(np.int32)
        want[:min(n, width)] = ranked[:width]
        assert np.array_equal(up[f], want) and counts[f] == n, f
