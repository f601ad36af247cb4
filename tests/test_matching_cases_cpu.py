"""The inputs of the exact matching tests, checked on the CPU: tests/matching_cases.py gives products that every float32
summation order reproduces bit for bit, holds the ties, rounding collisions and negative 2 - 2a it claims at every
structure of csrc/matching.hip, and tells a wrong arg-min rule from np.argmin's.  These are conditions on INPUTS -- a
fixture that misses them gets another placement, never a lower bar."""
import collections
import functools

import numpy as np
import pytest

import matching_cases as mc
from oracle import ops_ref


@functools.lru_cache(maxsize=None)
def _solved(C, regime, kind):
    p = mc.problem(C, regime, kind)
    dot = mc.exact_products(p.S, p.T, p.bits)
    return p, dot, mc.reference(dot)


def _pairs(row, mutual):
    i = np.nonzero(mutual)[0]
    return np.stack([i, row[i]], axis=1)


@pytest.mark.parametrize("C", mc.WIDTHS)
def test_every_summation_order_gives_the_same_products(C):
    """Lattice entries, bounded sums of magnitudes and a float64 product that float32 holds (asserted by the builder's
    exact_products) for every problem, degenerate shape and batched pair; BLAS sgemm then gives those bits, and the
    oracle's build_correspondence the reference pairs."""
    cases = [(p.name, p.S, p.T, p.bits) for p in mc.problems(C)]
    cases += [(name, S, T, 12) for name, S, T in mc.degenerate(C)]
    D, seg, bits = mc.batched(C)
    cases += [("pair %d" % n, D[so:so + sn], D[to:to + tn], b) for n, ((so, sn, to, tn), b) in enumerate(zip(seg, bits))
              if tn > 0]
    for name, S, T, b in cases:
        dot = mc.exact_products(S, T, b)
        assert np.array_equal(S @ T.T, dot), name
        row, col, mutual = mc.reference(dot)
        assert np.array_equal(ops_ref.build_correspondence(S, T), _pairs(row, mutual)), name
    assert np.isnan(mc.distances(mc.exact_products(D[seg[2, 0]:][:mc.NS], D[seg[2, 0]:][:mc.NS], 11))).any()


def test_the_collision_runs_are_found_not_assumed():
    """Four consecutive products share a distance next to -1 (3 steps of 2^-24 = 1.8e-7 apart, inside the kernel's 1e-6
    margin), two or three next to 0 and 0.375; above 0.5 a step of the product always moves the distance."""
    for a0, least in ((-4096 * 4094, 4), (512 * 512, 2), (3072 * 2048, 2)):
        lo, hi = mc.collision_run(a0)
        a = ((a0 + np.arange(lo - 1, hi + 2)) * 2.0 ** -24).astype(np.float32)
        d = mc.distances(a)
        assert hi - lo + 1 >= least and np.all(d[1:-1] == d[1]) and d[0] != d[1] and d[-1] != d[1], (a0, lo, hi)
    lo, hi = mc.collision_run(3 * 2 ** 22)
    assert lo == hi


@pytest.mark.parametrize("C", mc.WIDTHS)
def test_the_sweeps_put_a_bucket_boundary_on_every_line(C):
    """Every line's optimum is the last index's distance, shared by the 0 to 3 indices before it: the arg-min is the
    first of them, and all four run lengths occur on both sides."""
    for side, axis, n in (('row', 1, mc.NT), ('col', 0, mc.NT)):
        p = mc.sweep(C, side)
        dot = mc.exact_products(p.S, p.T)
        arg = mc.reference(dot)[0 if side == 'row' else 1]
        assert np.array_equal(np.argmax(dot, axis=axis), np.full(mc.NS, n - 1))
        runs = collections.Counter((n - arg).tolist())
        print("C = %d, %s sweep: lines by length of the optimum's run %s" % (C, side, dict(sorted(runs.items()))))
        assert set(runs) == {1, 2, 3, 4} and min(runs.values()) >= 10


def _structure(C, g):
    """Does the group's last pair of members straddle what its placement names?  Written out from the index maps of
    row_argmin_kernel: column j = chunk j / CPC, tile j / 64, block j / 16, lane j % 16; row i = workgroup i / 64RT,
    wave (i / 16RT) % 4, row tile (i / 16) % RT, lane quad (i % 16) / 4."""
    RT = mc.row_tiles(C)
    a, b = g['members'][-2:] if len(g['members']) > 1 else (g['members'][0],) * 2
    pl = g['placement']
    if g['side'] == 'row':
        same_chunk, lane_a, lane_b = a // mc.CPC == b // mc.CPC, a % 16, b % 16
        return {'lane': a // 16 == b // 16 and b == a + 1,
                'block': a // 64 == b // 64 and b // 16 == a // 16 + 1 and lane_a == lane_b,
                'tile': same_chunk and b // 64 == a // 64 + 1 and lane_a == lane_b,
                'tile5': same_chunk and b // 64 == a // 64 + 1 and lane_a != lane_b,
                'shared': same_chunk and a % mc.CPC // 64 == 0 and b % mc.CPC // 64 == 3 and lane_a != lane_b,
                'chunk256': a < 256 <= b < 512, 'chunk512': 256 <= a < 512 <= b,
                'last': mc.NT % 64 != 0 and mc.NT % 16 != 0 and mc.NT // 64 * 64 <= a < b and b >= mc.NT // 16 * 16}[pl]
    wg = lambda i: i // (64 * RT)
    wave = lambda i: i // (16 * RT)
    tile = lambda i: i // 16
    quad = lambda i: i % 16 // 4
    return {'lane': tile(a) == tile(b) and quad(a) == quad(b) and b == a + 1,
            'lk': tile(a) == tile(b) and quad(a) != quad(b),
            'rt': tile(a) != tile(b) and b == a + 16 and (wave(a) == wave(b)) == (RT == 2),
            'wave': wg(a) == wg(b) and wave(a) != wave(b),
            'wg': wg(a) != wg(b),
            'clamp': b == mc.NS - 1 and mc.NS % 16 != 0 and (a == b or tile(a) == tile(b) and quad(a) == quad(b))}[pl]


def _classify(products, members):
    """What the optimum of a line is made of, read from the reference's own numbers: ('tie' | 'single' | 'up' | 'down' |
    'nan', indices that share the optimum)."""
    d = mc.distances(products)
    if np.isnan(d).any():
        best = np.nonzero(np.isnan(d))[0]
        # several NaNs of different size, and a distance of exactly 0 below the first of them
        assert len(best) >= 2 and len(set(products[best].tolist())) == len(best)
        assert products[members[0]] == 1.0 and d[members[0]] == 0.0 and members[0] < best[0]
        return 'nan', best
    best = np.nonzero(d == d.min())[0]
    if len(best) == 1:
        return 'single', best
    a = products[best]
    if np.all(a == a[0]):
        return 'tie', best
    return ('up' if a[0] < a[-1] else 'down'), best


@pytest.mark.parametrize("C", mc.WIDTHS)
def test_every_class_is_planted_at_every_structure(C):
    seen = collections.Counter()
    for regime, kind in mc.REGIME_KINDS:
        p, dot, (row, col, _) = _solved(C, regime, kind)
        for g in p.groups:
            assert _structure(C, g), (p.name, g)
            products, arg = (dot[g['line']], row) if g['side'] == 'row' else (dot[:, g['line']], col)
            cls, best = _classify(products, g['members'])
            members = g['members'][1:] if cls == 'nan' else g['members']
            assert np.array_equal(best, members), (p.name, g, best)        # the planted members ARE the optimum
            assert arg[g['line']] == g['expect'] == best[0], (p.name, g)
            if cls == 'nan':     # 'up': the first NaN is the smaller product
                cls = 'nan-' + ('up' if products[best[0]] < products[best[1]] else 'down')
            want = {'nan': 'nan-' + kind, 'mid': kind, 'low': kind, 'anti': kind}[regime]
            if g['placement'] == 'clamp' and kind == 'tie':
                want = 'single'  # the last row alone: it ties with its own clamped copies, which only the kernel sees
            assert cls == want, (p.name, g, cls)
            seen[(g['side'], g['placement'], regime, cls)] += 1
    print("C = %d: %d planted lines in %d classes" % (C, sum(seen.values()), len(seen)))
    for side, placements in (('row', mc.ROW_PLACEMENTS), ('col', mc.COL_PLACEMENTS)):
        for pl in placements:
            tie = 'single' if pl == 'clamp' else 'tie'
            for regime, cls in (('mid', tie), ('mid', 'up'), ('mid', 'down'), ('low', 'up'), ('low', 'down'),
                                ('anti', 'up'), ('anti', 'down'), ('nan', 'nan-up'), ('nan', 'nan-down')):
                assert seen[(side, pl, regime, cls)] == 1, (side, pl, regime, cls)


# ------------------------------------------------------------------------------------------------ wrong rules
def _argmin_last(d, axis):
    n = d.shape[axis]
    return n - 1 - np.argmin(np.flip(d, axis), axis=axis)


def _later_block_wins(d, axis, block):
    """np.argmin inside blocks of `block` lines, merged with '<=': the later block keeps a tie."""
    d = np.where(np.isnan(d), -np.inf, d)
    d = d if axis == 1 else d.T
    arg, val = np.zeros(len(d), np.int64), np.full(len(d), np.inf, d.dtype)
    for b in range(0, d.shape[1], block):
        a = np.argmin(d[:, b:b + block], axis=1)
        v = d[np.arange(len(d)), b + a]
        arg, val = np.where(v <= val, b + a, arg), np.where(v <= val, v, val)
    return arg


def _largest_among_nans(dot, axis):
    d = mc.distances(dot)
    return np.where(np.isnan(d).any(axis=axis), np.argmax(dot, axis=axis), np.argmin(d, axis=axis))


def _mutants(C):
    dist = mc.distances
    clamped = lambda dot: np.sqrt(np.maximum(np.float32(2) - np.float32(2) * dot, np.float32(0)))
    nan_last = lambda dot: np.where(np.isnan(dist(dot)), np.inf, dist(dot))
    both = lambda f: (lambda dot: (f(dot, 1), f(dot, 0)))
    return {
        'arg-max of the product': both(lambda dot, ax: np.argmax(dot, axis=ax)),
        'last index on ties': both(lambda dot, ax: _argmin_last(dist(dot), ax)),
        'negative value clamped to 0': both(lambda dot, ax: np.argmin(clamped(dot), axis=ax)),
        'NaN ranked last': both(lambda dot, ax: np.argmin(nan_last(dot), axis=ax)),
        'largest product among the NaNs': both(_largest_among_nans),
        'later chunk / workgroup wins the merge': lambda dot: (_later_block_wins(dist(dot), 1, mc.CPC),
                                                               _later_block_wins(dist(dot), 0, 64 * mc.row_tiles(C))),
    }


@pytest.mark.parametrize("C", mc.WIDTHS)
def test_wrong_rules_are_caught_on_planted_rows_and_columns(C):
    for name, rule in _mutants(C).items():
        caught = collections.Counter()
        for regime, kind in mc.REGIME_KINDS:
            p, dot, (row, col, _) = _solved(C, regime, kind)
            m_row, m_col = rule(dot)
            for g in p.groups:
                ours, ref = (m_row, row) if g['side'] == 'row' else (m_col, col)
                if ours[g['line']] != ref[g['line']]:
                    caught[g['side']] += 1
                    caught[g['placement']] += 1
        print("C = %d, %s: wrong on %d planted rows and %d planted columns" % (C, name, caught['row'], caught['col']))
        assert caught['row'] >= 1 and caught['col'] >= 1, name
        if name.startswith('later'):
            assert caught['chunk256'] >= 1 and caught['chunk512'] >= 1 and caught['wg'] >= 1
