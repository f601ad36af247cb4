"""The inputs of the exact k-nearest matching tests, checked on the CPU: tests/knn_cases.py gives products that every
float32 summation order reproduces, holds every placement and form it claims (asserted from the data), and tells each of
five wrong rules from the right one; ``registration.knn_match_numpy`` is the rule; the ``matches=`` keyword is checked
before any work.  These are conditions on INPUTS -- a fixture that misses them gets another placement, never a lower bar."""
import functools
import inspect

import numpy as np
import pytest

import knn_cases as kc
import matching_cases as mc
from d3feat_pytorch_amd import _native
from d3feat_pytorch_amd.geometric_registration import registration as reg


@functools.lru_cache(maxsize=None)
def _dots(C):
    return [(p, mc.exact_products(p.S, p.T, p.bits)) for p in kc.problems(C)]


@pytest.mark.parametrize("C", kc.WIDTHS)
def test_the_restatement_is_a_brute_force_sort_on_every_problem(C):
    """exact_products asserts that there is ONE product matrix; knn_match_numpy on it equals a Python sort of (key, column)
    pairs for every k, blocked or not."""
    for p, dot in _dots(C):
        for k in kc.KS:
            want = kc.brute_force(dot, k)
            assert kc.same(reg.knn_match_numpy(p.S, p.T, k), want), kc.missed(p, reg.knn_match_numpy(p.S, p.T, k), want)
        assert kc.same(reg.knn_match_numpy(p.S, p.T, 8, block=37), kc.brute_force(dot, 8)), p.name
    for k in (1, 3, 8):
        for name, S, T in kc.degenerate(C, k):
            got = reg.knn_match_numpy(S, T, k)
            assert kc.same(got, kc.brute_force(mc.exact_products(S, T, 12), k)), name
            assert (got[0][:, len(T):] == -1).all() and np.isposinf(got[1][:, len(T):]).all(), name
    D, seg, bits = mc.batched(C)
    for (so, sn, to, tn), b in zip(seg.tolist(), bits):
        if tn:
            dot = mc.exact_products(D[so:so + sn], D[to:to + tn], b)
            assert kc.same(reg.knn_match_numpy(D[so:so + sn], D[to:to + tn], 5), kc.brute_force(dot, 5))


def test_the_restatement_takes_k_in_range_only():
    S = np.zeros((2, 16), np.float32)
    for k in (0, 9, -1):
        with pytest.raises(ValueError):
            reg.knn_match_numpy(S, S, k)
    assert reg.KNN_MAX == _native.D3F_KNN_MAX == kc.KMAX == 8


@pytest.mark.parametrize("C", kc.WIDTHS)
def test_every_placement_and_form_is_present(C):
    tiles = lambda cols: {j // kc.TILE for j in cols}
    chunks = lambda cols: {j // kc.CPC for j in cols}
    for form in kc.FORMS:
        p = kc.problem(C, form)
        dot = mc.exact_products(p.S, p.T, p.bits)
        idx, dist = kc.brute_force(dot, 8)
        assert sorted(g['placement'] for g in p.groups) == sorted(kc.PLACEMENTS)
        for g in p.groups:
            cols, line, where = np.array(g['members']), g['line'], (p.name, g['placement'])
            assert sorted(idx[line].tolist()) == cols.tolist(), where           # the 8 best ARE the members
            a, d = dot[line, cols], mc.distances(dot[line:line + 1, cols])[0]
            rest = np.delete(dot[line], cols)
            assert rest.max() < a.min() and (a.max() <= 1 or form == 'nan'), where
            # ---- placement
            if g['placement'] == 'lane':
                assert len(set(cols % 16)) == 1 and len(set(cols // 16)) == 8 and len(tiles(cols)) == 2 \
                    and len(chunks(cols)) == 1, where
            elif g['placement'] == 'block':
                assert len(set(cols // 16)) == 1 and len(set(cols % 16)) == 8, where
            elif g['placement'] == 'chunk':
                assert chunks(cols) == {0, 1, 2} and {255, 256, 511, 512} <= set(cols.tolist()), where
                assert {j // kc.CPC for j in idx[line, :3]} != {idx[line, 0] // kc.CPC} or form == 'nan', where
            elif g['placement'] == 'last':
                assert cols.min() >= kc.NT // kc.TILE * kc.TILE and (cols >= kc.NT // 16 * 16).sum() >= 2 \
                    and kc.NT - 1 in cols and kc.NT % kc.TILE and kc.NT % 16, where
            else:
                assert len(tiles(cols)) >= 4 and len(set(cols % 16)) == 8 and len(chunks(cols)) == 1, where
                if form != 'nan':
                    step = np.diff(d)
                    assert (step <= 0).all() if g['placement'] == 'improve' else (step >= 0).all(), where
                    if form == 'distinct':
                        assert (step != 0).all(), where
                    if g['placement'] == 'improve':          # every arrival (pair of arrivals) beats all before it
                        assert idx[line, 0] >= cols[-2], where
                    else:
                        assert idx[line, 0] == cols[0] and idx[line, 7] == cols[-1], where
            # ---- form
            if form == 'distinct':
                assert len(set(a.tolist())) == 8 and len(set(d.tolist())) == 8, where
            elif form == 'tie':
                assert len(set(a.tolist())) == 4 and all((a == x).sum() == 2 for x in a), where
            elif form == 'collide':
                assert len(set(a.tolist())) == 8 and len(set(d.tolist())) == 4, where
                for x in set(d.tolist()):
                    lo, hi = cols[d == x]
                    assert dot[line, hi] > dot[line, lo], where           # ranking on the product would swap them
            else:
                assert np.isnan(d).sum() == 4 and (d[~np.isnan(d)] == 0).all() and len(set(a[np.isnan(d)].tolist())) == 4, where
                assert np.isnan(dist[line, :4]).all() and (np.diff(idx[line, :4]) > 0).all() \
                    and (np.diff(idx[line, 4:]) > 0).all(), where
        # the lines sit in the first and last row, in several workgroups at either row tiling, and next to a tile edge
        lines = sorted(g['line'] for g in p.groups)
        assert lines[-1] == kc.NS - 1 and kc.NS % 16 and len({i // 128 for i in lines}) == 3 \
            and len({i // 64 for i in lines}) >= 4, p.name
    # the row sweep: runs of equal distances at the end of a row, which must come out in ascending column order
    p = mc.sweep(C, 'row')
    dot = mc.exact_products(p.S, p.T, p.bits)
    idx, dist = kc.brute_force(dot, 8)
    runs = collections_of_runs(dist)
    assert {1, 2, 3, 4} <= set(runs), sorted(set(runs))
    assert (idx[:, 0] >= kc.NT - 4).all() and ((np.diff(idx, axis=1) == 1) == (np.diff(dist, axis=1) == 0)).all()
    # matching_cases' own 'nan' problems: rows with several negative 2 - 2a
    for kind in ('up', 'down'):
        p = mc.problem(C, 'nan', kind)
        d = mc.distances(mc.exact_products(p.S, p.T, p.bits))
        assert (np.isnan(d).sum(1) >= 2).sum() >= len(mc.ROW_PLACEMENTS), p.name


def collections_of_runs(dist):
    """Lengths of the runs of equal distances over all rows."""
    out = []
    for row in dist:
        n = 1
        for a, b in zip(row[:-1], row[1:]):
            if a == b:
                n += 1
            else:
                out.append(n)
                n = 1
        out.append(n)
    return out


@pytest.mark.parametrize("C", (16, 128))
def test_each_wrong_rule_is_told_from_the_right_one(C):
    """On the planted lines alone (their rows of the product matrix), for k = 8 and for k = 2."""
    seen = {name: set() for name in kc.WRONG_RULES}
    for form in kc.FORMS:
        p = kc.problem(C, form)
        dot = mc.exact_products(p.S, p.T, p.bits)
        for g in p.groups:
            row = dot[g['line']:g['line'] + 1]
            for k in (2, 8):
                want = kc.brute_force(row, k)
                for name in kc.WRONG_RULES:
                    if not kc.same(kc.wrong_rule(name, row, k), want):
                        seen[name].add((form, g['placement'], k))
    assert all(seen.values()), seen
    flat = {name: {(f, pl) for f, pl, _ in hits} for name, hits in seen.items()}
    assert {('collide', pl) for pl in kc.PLACEMENTS} <= flat['rank_on_v']
    assert {('tie', pl) for pl in kc.PLACEMENTS} <= flat['ties_to_higher_column']
    assert {(f, 'lane') for f in kc.FORMS} <= flat['lane_keeps_one']
    assert {(f, 'chunk') for f in kc.FORMS} <= flat['chunks_not_merged']
    assert {('nan', pl) for pl in kc.PLACEMENTS} <= flat['nan_last']


def test_the_plumbing_pair_is_exact_and_splits_on_every_rule():
    """The descriptors of the GPU plumbing test: exact products, and each rule keeps some rows and drops others."""
    S, T = kc.plumbing_pair(32)
    mc.exact_products(S, T, 12)
    idx, dist = reg.knn_match_numpy(S, T, 3)
    ratio = dist[:, 0] < np.float32(0.9) * dist[:, 1]
    assert 30 <= ratio.sum() <= len(S) - 30
    back = reg.knn_match_numpy(T, S, 1)[0][:, 0]
    mutual = back[idx] == np.arange(len(S))[:, None]
    assert mutual[:, 0].sum() >= 30 and (~mutual[:, 0]).sum() >= 1 and mutual[:, 1:].sum() < mutual[:, 0].sum()


@pytest.mark.parametrize("matches", [dict(k=0), dict(k=9), dict(k=2.0), dict(k=True), dict(ratio=0.0), dict(ratio=1.5),
                                     dict(ratio='0.9'), dict(k=2, ratio=0.9), dict(knn=3), dict(k=3, mutual=1), dict(ratio=0.9, mutual=True), dict(),
                                     'knn', 3])
def test_matches_keyword_raises_before_any_work(matches):
    """Nothing here is a device tensor: a call that got past the check would fail with another error type."""
    for call in (lambda: reg.estimate_transform(None, None, None, None, None, None, matches=matches),
                 lambda: reg.register_scene('/nonexistent', 'scene', '/nonexistent', matches=matches),
                 lambda: reg._check_matches(matches, 'ransac', 5000)):
        with pytest.raises(ValueError, match="matches"):
            call()


def test_matches_keyword_counts_against_the_estimators_limit():
    assert reg._check_matches(dict(k=3), 'ransac', 5000) == (3, None, False)
    assert reg._check_matches(dict(ratio=0.9), 'sc2', 5000) == (1, 0.9, False)
    assert reg._check_matches(dict(k=1, ratio=1), 'sc2', 8192) == (1, 1.0, False)
    assert reg._check_matches(dict(k=8), 'fgr', 100000) == (8, None, False)
    assert reg._check_matches(dict(k=3, mutual=True), 'sc2', 2000) == (3, None, True)
    assert reg._check_matches(dict(k=np.int64(2)), 'sc2', 4096) == (2, None, False)
    with pytest.raises(ValueError) as e:
        reg._check_matches(dict(k=2), 'sc2', 5000)
    assert "10000" in str(e.value) and str(reg.SC2_MAX_COUNT) in str(e.value)
    with pytest.raises(ValueError) as e:
        reg.estimate_transform(None, None, None, None, None, None, num_points=10000, matches=dict(k=7))
    assert "70000" in str(e.value) and str(reg.RANSAC_MAX_COUNT) in str(e.value)
    assert (reg.SC2_MAX_COUNT, reg.RANSAC_MAX_COUNT) == (_native.D3F_SC2_MAX_COUNT, _native.D3F_RANSAC_MAX_COUNT)


def test_matches_none_takes_the_unchanged_path(monkeypatch):
    """None and 'mutual' never reach knn_match: _pair_points calls mutual_nn and hands back its flags and rows as before."""
    assert reg._check_matches(None, 'sc2', 10 ** 9) is None and reg._check_matches('mutual', 'sc2', 10 ** 9) is None
    for f in (reg.estimate_transform, reg.register_scene, reg._pair_points):
        assert inspect.signature(f).parameters['matches'].default is None
    import torch
    calls = []

    def mutual_nn(s, t):
        calls.append((s.clone(), t.clone()))
        return torch.tensor([2, 0, 1]), None, torch.tensor([1, 0, 1], dtype=torch.int32)

    def knn_match(*a):
        raise AssertionError("knn_match on the mutual path")
    monkeypatch.setattr(reg.ops, 'mutual_nn', mutual_nn)
    monkeypatch.setattr(reg.ops, 'knn_match', knn_match)
    kp = torch.arange(12.0).view(4, 3)
    desc = torch.eye(4)[:, :3].contiguous()
    score = torch.tensor([0.5, 0.1, 0.9, 0.7])
    for matches in ((), (None,)):
        mutual, sp, tp = reg._pair_points(kp, desc, score, kp + 100, desc, score, 3, *matches)
        si = reg.select_keypoints(score, 3)
        assert torch.equal(mutual, torch.tensor([1, 0, 1], dtype=torch.int32)) and torch.equal(sp, kp[si])
        assert torch.equal(tp, (kp + 100)[si][torch.tensor([2, 0, 1])])
    assert len(calls) == 2 and torch.equal(calls[0][0], desc[si])


def test_knn_flags_are_the_slots_the_issue_names():
    """dict(k=K): every filled slot, flat at i K + s; dict(ratio=r): f32 comparison, false on NaN and without a second."""
    import torch
    idx = torch.tensor([[4, 2], [1, -1], [0, 3], [5, 6], [7, 8]], dtype=torch.int32)
    dist = torch.tensor([[0.5, 1.0], [0.1, float('inf')], [float('nan'), 0.5], [0.9, 1.0], [0.25, 0.5]])
    keep, col = reg._knn_flags(idx, dist, None)
    assert keep.tolist() == [True, True, True, False, True, True, True, True, True, True] and col.tolist() == idx.reshape(-1).tolist()
    keep, col = reg._knn_flags(idx, dist, 0.9)
    assert keep.tolist() == [True, False, False, False, True] and col.tolist() == [4, 1, 0, 5, 7]
    assert reg._knn_flags(idx, dist, 0.5)[0].tolist() == [False, False, False, False, False]       # 0.25 < 0.5 * 0.5 is false
    r = np.float32(0.9)
    assert bool(np.float32(0.9) < r * np.float32(1.0)) is False


def test_ws_bytes_is_callable_from_the_built_library():
    lib = _native.lib()
    assert lib.d3f_knn_match_ws_bytes(300, 700, 8) >= 3 * 300 * 8 * 8
    assert lib.d3f_knn_match_ws_bytes(300, 700, 1) >= 3 * 300 * 8
    assert lib.d3f_knn_match_ws_bytes(300, 700, 9) == 0 == lib.d3f_knn_match_ws_bytes(0, 700, 1)
    assert lib.d3f_knn_match_batched_ws_bytes(1905, 4, 300, 700, 5) >= 3 * 1905 * 5 * 8
    old = _native.set_tunables(match_wgs=1)
    try:
        assert lib.d3f_knn_match_ws_bytes(300, 700, 8) == 300 * 8 * 8
    finally:
        _native.set_tunables(**old)
    # bad arguments are refused on the host, before any launch
    p = 0x10000
    assert lib.d3f_knn_match(p, 300, p, 700, 32, 0, p, p, p, 1 << 30, None) == _native.D3F_EINVAL
    assert lib.d3f_knn_match(p, 300, p, 700, 32, 9, p, p, p, 1 << 30, None) == _native.D3F_EINVAL
    assert lib.d3f_knn_match(p, 300, p, 700, 48, 3, p, p, p, 1 << 30, None) == _native.D3F_EINVAL
    assert lib.d3f_knn_match(p, 0, p, 700, 32, 3, p, p, p, 1 << 30, None) == _native.D3F_EINVAL
    assert lib.d3f_knn_match(p, 300, p, 700, 32, 3, None, p, p, 1 << 30, None) == _native.D3F_EINVAL
    assert lib.d3f_knn_match(p, 300, p, 700, 32, 3, p, p, p, 256, None) == _native.D3F_EWORKSPACE
    assert lib.d3f_knn_match_batched(p, 900, p, 900, p, 0, 300, 700, 32, 3, p, p, p, 1 << 30, None) == _native.D3F_EINVAL
    assert lib.d3f_knn_match_batched(p, 900, p, 900, p, 2, 300, 700, 32, 3, p, p, p, 256, None) == _native.D3F_EWORKSPACE
