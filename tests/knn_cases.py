"""Descriptor pairs on which k-nearest matching has ONE right answer for every k, bit for bit (NumPy only; shared by the
CPU and GPU tests of csrc/knn_match.hip).  Built on the exact lattice of tests/matching_cases.py: every product is a
float32 whatever the order of its sum (``mc.exact_products`` asserts it), so the rule of csrc/knn_match.hpp --
ascending (rounded distance, column), NaN first -- leaves no freedom.

A planted LINE is a source row whose 8 best columns are 8 planted MEMBERS at a placement that strains one structure of
the kernel; everything else has product 0 with the line (distance sqrt 2).  Layout as in matching_cases: channel 0
carries the fine control (line 1 unit, member m units: + m lattice steps on the product), one private channel the
product itself (two lines share one with opposite signs), background rows are zero on the planted channels.

Placements (columns of T; NT = 700 is three column chunks of 256, tiles of 64, blocks of 16, lane = column mod 16):
  lane      all 8 in ONE lane, over 8 successive blocks of two tiles: the lane's private list holds all k;
  block     8 different lanes of one 16-column block: only the cross-lane merge can rank them;
  chunk     astride the chunk boundaries at 256 and 512: only the chunk merge can rank them;
  last      in the partial last tile (640..699), four of them in the partial last block (688..699);
  improve   one per tile and lane, each better than all before it: every arrival evicts;
  worsen    the same, each worse than all before it: the filter must still admit the 2nd .. k-th.
``RANKS[placement][m]`` is the quality rank (0 = best) of member m in column order.

Forms (how the 8 qualities are realised):
  distinct  8 different products, 16 lattice steps apart: 8 different distances;
  tie       4 pairs of EQUAL products: the ascending column decides inside a pair;
  collide   4 pairs of DIFFERENT products that round to one distance (``mc.collision_run``), the larger product at the
            higher column: the column, not the product, decides;
  nan       ranks 0, 2, 4, 6 have products above 1 (2 - 2a < 0: NaN, of four different magnitudes), ranks 1, 3, 5, 7
            the product 1 (distance 0): the NaNs come first, in column order, then the zeros in column order.
"""
import functools

import numpy as np

import matching_cases as mc

WIDTHS, NS, NT, CPC, TILE = mc.WIDTHS, mc.NS, mc.NT, mc.CPC, mc.TILE
KS = (1, 2, 3, 5, 8)
KMAX = 8
FORMS = ('distinct', 'tie', 'collide', 'nan')

COLUMNS = {
    'lane': (259, 275, 291, 307, 323, 339, 355, 371),
    'block': (400, 402, 403, 405, 408, 411, 413, 415),
    'chunk': (254, 255, 256, 257, 510, 511, 512, 513),
    'last': (641, 650, 663, 672, 689, 690, 698, 699),
    'improve': (20, 47, 85, 110, 139, 172, 200, 230),
    'worsen': (21, 50, 90, 118, 151, 184, 211, 240),
}
RANKS = {
    'lane': (3, 0, 6, 1, 7, 2, 5, 4),
    'block': (5, 2, 7, 0, 4, 1, 6, 3),
    'chunk': (1, 6, 3, 4, 0, 7, 2, 5),
    'last': (2, 7, 0, 5, 3, 6, 1, 4),
    'improve': (7, 6, 5, 4, 3, 2, 1, 0),
    'worsen': (0, 1, 2, 3, 4, 5, 6, 7),
}
PLACEMENTS = tuple(COLUMNS)
# the lines: the first and the last row (whose clamped copies fill its row tile), rows of the second and third
# workgroup at either row tiling, one row past a row tile
LINES = dict(zip(PLACEMENTS, (5, 77, 130, 201, 272, NS - 1)))


def member_products(form, ranks, cols, bits):
    """[(amplitude, steps)] of the 8 members in column order, on the lattice 2^-bits."""
    U = 1 << bits
    if form == 'nan':
        return [(U + 2, 4 * r) if r % 2 == 0 else (U, 0) for r in ranks]
    amp, a0 = 2048, 3072 * 2048
    if form == 'distinct':
        return [(amp, 16 * (7 - r)) for r in ranks]
    if form == 'tie':
        return [(amp, 16 * (3 - r // 2)) for r in ranks]
    assert form == 'collide'
    out = [None] * 8
    for g in range(4):
        off = 200 * (3 - g)
        lo, hi = mc.collision_run(a0 + off, bits)
        assert hi > lo
        first, second = sorted((m for m in range(8) if ranks[m] // 2 == g), key=lambda m: cols[m])
        out[first], out[second] = (amp, off + lo), (amp, off + hi)
    return out


@functools.lru_cache(maxsize=None)
def problem(C, form):
    """mc.Problem whose ``groups`` are the six lines: dicts with placement, form, line (row of S), members (columns of T
    in column order) and ranks."""
    bits = 11 if form == 'nan' else 12
    U = 1 << bits
    n_planted = 1 + (len(PLACEMENTS) + 1) // 2
    n_bg = C - n_planted
    rng = np.random.default_rng([C, 7, FORMS.index(form)])
    R = int(U * np.sqrt(0.9 / n_bg))             # n_bg R^2 <= 0.9 U^2: the bound holds for ANY two background rows
    S = np.zeros((NS, C), np.int64)
    T = np.zeros((NT, C), np.int64)
    S[:, n_planted:] = rng.integers(-R, R + 1, size=(NS, n_bg))
    T[:, n_planted:] = rng.integers(-R, R + 1, size=(NT, n_bg))
    line_amp = U if form == 'nan' else 3072
    groups = []
    for g, placement in enumerate(PLACEMENTS):
        cols, ranks, line = COLUMNS[placement], RANKS[placement], LINES[placement]
        ch, sign = 1 + g // 2, 1 - 2 * (g % 2)
        S[line, :] = 0
        S[line, 0] = 1
        S[line, ch] = sign * line_amp
        for j, (amp, steps) in zip(cols, member_products(form, ranks, cols, bits)):
            T[j, :] = 0
            T[j, 0] = steps
            T[j, ch] = sign * amp
        groups.append(dict(placement=placement, form=form, line=line, members=cols, ranks=ranks))
    scale = np.float32(2.0 ** -bits)
    p = mc.Problem(C, 'knn', form, (S * scale).astype(np.float32), (T * scale).astype(np.float32), bits, groups)
    p.name = "knn/%s/C%d" % (form, C)
    return p


def problems(C):
    """The four planted problems, matching_cases' row sweep as it is (runs of 1-4 equal distances in DESCENDING column
    order of the product: ascending column inside a run) and its two 'nan' problems."""
    return [problem(C, form) for form in FORMS] + [mc.sweep(C, 'row'), mc.problem(C, 'nan', 'up'),
                                                    mc.problem(C, 'nan', 'down')]


def degenerate(C, k):
    """[(name, S, T)]: Nt in {1, k - 1, k, 15} and Ns in {1, 17, one past a workgroup at either row tiling}, cut from the
    tie problem."""
    p = problem(C, 'tie')
    out = [("Nt=%d" % n, p.S, p.T[:n]) for n in sorted({1, k - 1, k, 15} - {0})]
    return out + [("Ns=%d" % n, p.S[:n], p.T) for n in (1, 17, 65, 129)]


@functools.lru_cache(maxsize=None)
def plumbing_pair(C=32):
    """(S [NS,C], T [NT,C]) on the 2^-12 lattice for the tests of the ``matches=`` plumbing: every entry is +-R with
    C R^2 <= 0.9, so any two rows have an exact product; target row j < NS is source row j with j mod 8 signs flipped
    (products 0.90 down to 0.51 in steps of 0.056: some pass Lowe's test at 0.9, some do not), the others are random."""
    rng = np.random.default_rng([C, 23])
    R = int(4096 * np.sqrt(0.9 / C))
    S = R * rng.choice([-1, 1], size=(NS, C))
    T = R * rng.choice([-1, 1], size=(NT, C))
    for j in range(NS):
        T[j] = S[j]
        T[j, rng.permutation(C)[:j % 8]] *= -1
    scale = np.float32(2.0 ** -12)
    return (S * scale).astype(np.float32), (T * scale).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the rule, and wrong ones
def keys_of(dot32, nan_last=False, on_v=False):
    """The ranking key of every product: the rounded distance with NaN as -inf (the rule); ``on_v``: 2 - 2a itself (negative ones by magnitude);
    ``nan_last``: NaN as +inf."""
    with np.errstate(invalid='ignore'):
        v = np.float32(2) - np.float32(2) * dot32
        d = np.sqrt(v)
    if on_v:
        return np.where(np.isnan(v), -np.inf, v), d
    return np.where(np.isnan(d), np.inf if nan_last else -np.inf, d), d


def top_k(key, d, k, cols=None, high_column_first=False):
    """(idx, dist) of the k smallest (key, column) per row among ``cols`` (default: all); -1 / +inf where there are fewer."""
    cols = np.arange(key.shape[1]) if cols is None else np.asarray(cols)
    idx = np.full((len(key), k), -1, np.int32)
    dist = np.full((len(key), k), np.inf, np.float32)
    for i in range(len(key)):
        order = sorted(cols.tolist(), key=lambda j: (key[i, j], -j if high_column_first else j))[:k]
        idx[i, :len(order)] = order
        dist[i, :len(order)] = d[i, order]
    return idx, dist


def brute_force(dot32, k):
    """The rule by a plain Python sort of (key, column) pairs."""
    key, d = keys_of(dot32)
    return top_k(key, d, k)


def wrong_rule(name, dot32, k):
    """What a kernel with one of the named mistakes would return."""
    if name == 'rank_on_v':
        return top_k(*keys_of(dot32, on_v=True), k)
    if name == 'ties_to_higher_column':
        return top_k(*keys_of(dot32), k, high_column_first=True)
    if name == 'nan_last':
        return top_k(*keys_of(dot32, nan_last=True), k)
    key, d = keys_of(dot32)
    if name == 'chunks_not_merged':               # the first chunk's answer stands
        return top_k(key, d, k, cols=np.arange(min(CPC, key.shape[1])))
    assert name == 'lane_keeps_one'               # per chunk and lane only the best column survives
    idx = np.full((len(key), k), -1, np.int32)
    dist = np.full((len(key), k), np.inf, np.float32)
    n = key.shape[1]
    for i in range(len(key)):
        survivors = []
        for c0 in range(0, n, CPC):
            for lane in range(16):
                mine = [j for j in range(c0, min(c0 + CPC, n)) if j % 16 == lane]
                if mine:
                    survivors.append(min(mine, key=lambda j: (key[i, j], j)))
        a, b = top_k(key[i:i + 1], d[i:i + 1], k, cols=survivors)
        idx[i], dist[i] = a[0], b[0]
    return idx, dist


WRONG_RULES = ('rank_on_v', 'ties_to_higher_column', 'lane_keeps_one', 'chunks_not_merged', 'nan_last')


def _differs(a, b):
    """[rows] where idx differs or dist differs bitwise; a NaN equals a NaN (the sign and payload of a NaN are nobody's rule)."""
    da, db = np.asarray(a[1], np.float32), np.asarray(b[1], np.float32)
    both_nan = np.isnan(da) & np.isnan(db)
    return (np.asarray(a[0]) != np.asarray(b[0])).any(1) | ((da.view(np.uint32) != db.view(np.uint32)) & ~both_nan).any(1)


def same(a, b):
    """idx equal and dist bitwise equal (NaN equals NaN)."""
    return np.asarray(a[0]).shape == np.asarray(b[0]).shape and not _differs(a, b).any()


def missed(p, got, want):
    """The placements of ``p`` whose line differs, and the number of other rows that do: what a failure names."""
    bad = np.nonzero(_differs(got, want))[0]
    lines = {g['line']: g['placement'] for g in getattr(p, 'groups', ()) if g.get('side', 'row') == 'row'}
    return "%s: lines missed %s, other rows missed %d (first rows %s)" % (
        getattr(p, 'name', p), sorted(lines[i] for i in bad if i in lines), sum(i not in lines for i in bad),
        bad[:5].tolist())
