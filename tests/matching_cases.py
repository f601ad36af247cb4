"""Descriptor pairs on which mutual-NN matching has ONE right answer, bit for bit (NumPy only; shared by the CPU and GPU
tests of csrc/matching.hip).

Exact lattice: every entry is an integer multiple of 2^-12 and sum_c |S[i,c] T[j,c]| <= 1 for every pair of rows, so every
partial sum of a dot product, in any order, is a multiple of 2^-24 of magnitude <= 1: a float32.  BLAS, the MFMA chains
and float64 give the same product bits, and sqrt(2 - 2 a) of the reference is two correctly rounded operations.  (The
problems with products above 1 use multiples of 2^-11 and the bound 2, for the same reason.)  `exact_products` asserts all
of this for the pair it is given.

On such inputs ties, rounding collisions (different products, one rounded distance) and negative 2 - 2a can be PLANTED.
A group is one source row (or target column) -- its "line" -- whose optimum is two or three planted "members" at a
placement that straddles one structure of the kernel (lanes, 16-column blocks, 64-column tiles, filter sharing, column
chunks, row tiles, waves, workgroups, clamped rows).  Layout of a planted row: channel 0 carries the fine control (line 1
unit, member k units: + k lattice steps on the product), one private channel carries the product itself, everything else
is zero; background rows are random on the remaining channels and zero on the planted ones, so a planted row and a
background row have product 0.  Two groups share a private channel with opposite signs (their cross product is
negative).  In the anti-correlated regime (optimum near -1, where 4 consecutive products share one distance) every source
row holds 1 - 2^-12 on the column groups' channels and every target row -(1 - 2^-12) on the row groups', so that a line
sees -(1 - 2^-12) everywhere but at its members, which are one step of 2^-12 better."""
import functools

import numpy as np

WIDTHS = (16, 32, 64, 128)
NS, NT = 300, 700          # > 2 workgroups of rows at RT = 2; 3 column chunks of CPC by default, one at match_wgs = 1
CPC = 256                  # chunking() of matching.hip at this shape: cdiv(700, 256) = 3 chunks of 4 tiles
TILE = 64

REGIME_KINDS = (('mid', 'tie'), ('mid', 'up'), ('mid', 'down'), ('low', 'up'), ('low', 'down'), ('anti', 'up'),
                ('anti', 'down'), ('nan', 'up'), ('nan', 'down'))
ROW_PLACEMENTS = ('chunk256', 'chunk512', 'last', 'lane', 'block', 'tile', 'tile5', 'shared')
COL_PLACEMENTS = ('clamp', 'lane', 'lk', 'rt', 'wave', 'wg')


def row_tiles(C):
    """RT of run<C>() in matching.hip: a wave holds 16 RT source rows, a workgroup 64 RT."""
    return 2 if C <= 64 else 1


def distances(dot32):
    """The reference's float32 distance matrix, geometric_registration/common.py:9-10."""
    assert dot32.dtype == np.float32
    with np.errstate(invalid='ignore'):
        return np.sqrt(np.float32(2) - np.float32(2) * dot32)


def reference(dot32):
    """(row_argmin, col_argmin, mutual) of common.py:5-21 on the exact products."""
    d = distances(dot32)
    row, col = np.argmin(d, axis=1), np.argmin(d, axis=0)
    return row, col, col[row] == np.arange(len(row))


def exact_products(S, T, bits=12):
    """The float32 product matrix S T^T after asserting that it is the ONLY one: lattice entries, bounded sum of
    magnitudes (1 on the 2^-12 lattice, 2 on the 2^-11 one) and a float64 product that float32 holds unchanged."""
    unit = 2.0 ** bits
    for a in (S, T):
        assert a.dtype == np.float32 and np.array_equal(a * unit, np.rint(a * unit))
    S64, T64 = S.astype(np.float64), T.astype(np.float64)
    assert (np.abs(S64) @ np.abs(T64).T).max() <= 2.0 ** (12 - bits)
    dot64 = S64 @ T64.T
    dot32 = dot64.astype(np.float32)
    assert np.array_equal(dot32.astype(np.float64), dot64)
    return dot32


def collision_run(a0, bits=12, span=64):
    """(k_lo, k_hi): the longest run of lattice products (a0 + k) 2^-2bits, |k| <= span, that share one float32 distance
    (the run nearest k = 0 among equals)."""
    k = np.arange(-span, span + 1)
    d = distances(((a0 + k) * 2.0 ** (-2 * bits)).astype(np.float32))
    start = np.concatenate([[0], np.nonzero(d[1:] != d[:-1])[0] + 1])
    stop = np.concatenate([start[1:], [len(k)]])
    inner = (start > 0) & (stop < len(k))                    # runs cut by the window are not whole
    length = np.where(inner, stop - start, 0)
    best = np.nonzero(length == length.max())[0]
    b = best[np.argmin(np.abs(k[start[best]]))]
    return int(k[start[b]]), int(k[stop[b] - 1])


# placement -> (offset of the second member, condition on the first); columns for row groups, rows for column groups
def _row_second(name, j1):
    if name == 'lane':      # neighbouring lanes of one 16-column block
        return j1 + 1 if j1 % 16 <= 14 else None
    if name == 'block':     # same lane, next block of the tile
        return j1 + 16 if j1 % TILE < 48 else None
    if name == 'tile':      # same lane, next tile of the chunk
        return j1 + 64 if j1 % CPC < 192 else None
    if name == 'tile5':     # next tile, another lane
        return j1 + 69 if j1 % CPC < 187 and j1 % 16 < 11 else None
    if name == 'shared':    # tile 0 -> tile 3 of a chunk: the filter was shared among the lanes after tile 1
        return j1 + 195 if j1 % CPC < 61 and j1 % 16 < 13 else None
    raise KeyError(name)


def _col_second(name, i1, RT):
    if name == 'lane':      # rows 4 lk + r of one lane
        return i1 + 1 if i1 % 4 <= 2 else None
    if name == 'lk':        # same row tile, other lane quad
        return i1 + 4 if i1 % 16 < 12 else None
    if name == 'rt':        # other row tile of the wave (RT = 2); the next wave at RT = 1
        return i1 + 16 if i1 % 32 < 16 else None
    if name == 'wave':      # other wave of the workgroup
        return i1 + 16 * RT if i1 % (64 * RT) < 48 * RT else None
    if name == 'wg':        # other workgroup
        return i1 + 64 * RT
    raise KeyError(name)


class Problem:
    """S [NS, C], T [NT, C] float32 (the other way round in the column sweep), their lattice 2^-bits and the planted
    groups: dicts with side ('row' / 'col'), placement, kind, line (the row of S / T that owns the optimum), members
    (ascending rows of the other matrix) and expect (the member np.argmin returns)."""

    def __init__(self, C, regime, kind, S, T, bits, groups):
        self.C, self.regime, self.kind, self.S, self.T, self.bits, self.groups = C, regime, kind, S, T, bits, groups
        self.name = "%s/%s/C%d" % (regime, kind, C)


def _members(regime, kind, amp, a0, bits):
    """[(amplitude, k)] of the members in index order; the first of them that reaches the optimum is expected."""
    if regime == 'nan':
        # 1 (distance 0) at the lowest index, then 1 + 2^-20 and 1 + 2^-10: both NaN, np.argmin returns the first
        small, large = (amp, 4), (amp + 2, 0)
        return [(amp, 0)] + ([small, large] if kind == 'up' else [large, small])
    if kind == 'tie':
        return [(amp, 0), (amp, 0)]
    lo, hi = collision_run(a0, bits)
    assert hi > lo
    return [(amp, lo), (amp, hi)] if kind == 'up' else [(amp, hi), (amp, lo)]


@functools.lru_cache(maxsize=None)
def problem(C, regime, kind):
    RT = row_tiles(C)
    bits = 11 if regime == 'nan' else 12
    U = 1 << bits
    n_groups = len(ROW_PLACEMENTS) + len(COL_PLACEMENTS)
    anti = regime == 'anti'
    n_planted = 1 + (n_groups if anti else (n_groups + 1) // 2)
    n_bg = C - n_planted
    assert n_bg >= 1
    rng = np.random.default_rng([C, REGIME_KINDS.index((regime, kind))])
    R = int(U * np.sqrt(0.9 / n_bg))             # n_bg R^2 <= 0.9 U^2: the bound holds for ANY two background rows
    S = np.zeros((NS, C), np.int64)
    T = np.zeros((NT, C), np.int64)
    S[:, n_planted:] = rng.integers(-R, R + 1, size=(NS, n_bg))
    T[:, n_planted:] = rng.integers(-R, R + 1, size=(NT, n_bg))
    # (line amplitude, member amplitude) of a row group; a column group has them the other way round
    line_amp, member_amp = {'mid': (3072, 2048), 'low': (512, 512), 'nan': (U, U), 'anti': (U, -(U - 2))}[regime]
    if anti:
        row_ch = 1 + np.arange(len(ROW_PLACEMENTS))
        col_ch = 1 + len(ROW_PLACEMENTS) + np.arange(len(COL_PLACEMENTS))
        S[:, col_ch] = U - 1
        T[:, row_ch] = -(U - 1)

    used = {'row': set(), 'col': set()}        # 'row' groups use columns of T as members, 'col' groups rows of S

    def free_below(side, p):
        while p in used[side]:
            p -= 1
        assert p >= 0
        return p

    groups = []
    for g, (side, placement) in enumerate([('row', p) for p in ROW_PLACEMENTS] + [('col', p) for p in COL_PLACEMENTS]):
        n_lines, n_members = (NS, NT) if side == 'row' else (NT, NS)
        # the two members that straddle the structure
        if placement in ('chunk256', 'chunk512'):
            b = int(placement[5:])
            pair = (b - 3, b + 2)
        elif placement == 'clamp':               # the last row and its clamped copies (NS % 16 != 0)
            pair = (NS - 1,) if kind == 'tie' else (NS - 2, NS - 1)
        else:
            # 'last': both in the partial last tile, the second in the partial last block.  The others stay clear of it,
            # of the chunk boundaries' pairs and of the last rows.
            first = range(NT // TILE * TILE, NT // 16 * 16) if placement == 'last' else range(8, n_members)
            for p1 in rng.permutation(np.asarray(first)).tolist():
                if placement == 'last':
                    p2 = free_below(side, NT - 1)
                    p2 = p2 if p2 >= NT // 16 * 16 else None
                else:
                    p2 = _row_second(placement, p1) if side == 'row' else _col_second(placement, p1, RT)
                limit = NT // TILE * TILE if side == 'row' else NS - 3
                if p2 is not None and (placement == 'last' or p2 < limit) and not {p1, p2} & used[side] and \
                        not {p1 - 1, p1 - 2} & used[side]:
                    pair = (p1, p2)
                    break
            else:
                raise AssertionError("no room for %s %s" % (side, placement))
        used[side].update(pair)
        a0 = line_amp * member_amp
        spec = _members(regime, kind, member_amp if side == 'row' else line_amp, a0, bits)
        if len(pair) == 1:
            spec = spec[:1]
        if len(spec) == 3:                       # the zero-distance member goes below the pair
            pair = (free_below(side, pair[0] - 1),) + pair
            used[side].add(pair[0])
        # a free line (never one of the last rows: they belong to 'clamp')
        other = 'col' if side == 'row' else 'row'
        line = next(x for x in rng.permutation(n_lines - 3).tolist() if x not in used[other])
        used[other].add(line)
        ch, sign = (1 + g, 1) if anti else (1 + g // 2, 1 - 2 * (g % 2))
        L, M = (S, T) if side == 'row' else (T, S)
        L[line, n_planted:] = 0
        L[line, 0] = 1
        if anti and side == 'col':
            L[line, row_ch] = 0                  # (a target line is seen by the sources' column channels only)
            L[line, ch] = -U
        else:
            L[line, ch] = sign * (line_amp if side == 'row' else member_amp)
        for p, (amp, k) in zip(pair, spec):
            M[p, n_planted:] = 0
            M[p, 0] = k
            M[p, ch] = (U - 2) if (anti and side == 'col') else sign * amp
        groups.append(dict(side=side, placement=placement, kind=kind, line=line, members=pair,
                           expect=pair[1] if len(spec) == 3 else pair[0]))
    scale = np.float32(2.0 ** -bits)
    return Problem(C, regime, kind, (S * scale).astype(np.float32), (T * scale).astype(np.float32), bits, groups)


@functools.lru_cache(maxsize=None)
def sweep(C, side):
    """One bucket boundary of the rounded distance per line.  side 'row': source row i = (1, alpha_i, 0...), target
    column j = (j - (NT - 1), beta, 0...): the products of row i are alpha_i beta + k lattice steps, k = -(NT - 1) .. 0
    in column order, so np.argmin returns the FIRST column whose distance rounds to that of the last one -- 1 to 4 columns
    from the end, by where alpha_i beta lies in (-0.98, 0.98).  side 'col': the transposed problem (700 source rows)."""
    rng = np.random.default_rng([C, 99, side == 'col'])
    S = np.zeros((NS, C), np.int64)
    T = np.zeros((NT, C), np.int64)
    S[:, 0], S[:, 1] = 1, rng.integers(-4000, 4001, size=NS)
    T[:, 0], T[:, 1] = np.arange(NT) - (NT - 1), 4095
    S, T = ((x * np.float32(2.0 ** -12)).astype(np.float32) for x in (S, T))
    return Problem(C, 'sweep', side, *((S, T) if side == 'row' else (T, S)), 12, [])


def problems(C):
    return [problem(C, regime, kind) for regime, kind in REGIME_KINDS] + [sweep(C, 'row'), sweep(C, 'col')]


def degenerate(C):
    """[(name, S, T)]: one row, one column, less than one block of columns, one row past a row tile, one row past a
    workgroup -- cut from the tie problem, whose planted columns keep exact ties (product 0) over the background rows."""
    p = problem(C, 'mid', 'tie')
    n = 64 * row_tiles(C) + 1
    return [("Ns=1", p.S[:1], p.T), ("Nt=1", p.S, p.T[:1]), ("Nt=15", p.S, p.T[:15]), ("Ns=17", p.S[:17], p.T),
            ("Ns=%d" % n, p.S[:n], p.T)]


def batched(C):
    """(D, seg, bits): four pairs stacked in one matrix D at row offsets that are no multiples of 16; seg [4,4] =
    (src_off, src_len, tgt_off, tgt_len).  Pair 1 has an empty target; pair 2 matches the 2^-11 problem's source rows
    against themselves (self products of exactly 1 and above 1)."""
    a, b, c, d = (problem(C, *rk) for rk in (('mid', 'tie'), ('low', 'up'), ('nan', 'up'), ('anti', 'down')))
    parts = [np.zeros((5, C), np.float32), a.S, a.T, b.S, c.S, d.S, d.T]
    off = np.concatenate([[0], np.cumsum([len(x) for x in parts])])
    seg = np.array([[off[1], NS, off[2], NT], [off[3], NS, off[4], 0], [off[4], NS, off[4], NS],
                    [off[5], NS, off[6], NT]], np.int32)
    assert all(o % 16 for o in seg[:, 0]) and all(o % 16 for o in seg[:, 2])
    return np.concatenate(parts, 0), seg, (12, 12, 11, 12)
