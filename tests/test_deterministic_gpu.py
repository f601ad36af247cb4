"""GPU: the deterministic training mode (ops.set_deterministic / TrainStep(deterministic=True)) -- the order-fixed forms of
the backward scatters against NumPy restatements that add in float32, sequentially, in the order the kernels' header
comments state (bit for bit); against the float-atomic forms they replace within the rounding bound of a sum of that many
terms; and whole training steps replayed from the same parameters, bit for bit."""
import numpy as np
import pytest
import torch

from d3feat_pytorch_amd import config as cfgmod
from d3feat_pytorch_amd import _native, ops
from kpconv_cases import SPARSE_EXTENT, _kpconv_case
from oracle import ops_ref
from util import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U24 = 2.0 ** -24
BWD_TOL = 2e-4          # test_gpu_ops.test_kpconv_forward_backward's bound on the backward results


def cu(a, dtype=None):
    t = torch.as_tensor(a)
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV)


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def order_bound(n_terms, abs_sum):
    """|sum in one order - sum in another| of n float32 terms per element: each order is within gamma_(n-1) sum |term| of
    the exact sum (Higham, Accuracy and Stability, eq. 4.4), so the two differ by at most twice that.  Computed from the
    term count, as odometry_cases.sum_bound does for float64."""
    n = np.maximum(np.asarray(n_terms, np.float64) - 1.0, 0.0)
    return 2.0 * (n * U24 / (1.0 - n * U24)) * np.asarray(abs_sum, np.float64)


@pytest.fixture(autouse=True)
def _mode_off_afterwards():
    yield
    ops.set_deterministic(False)


# ------------------------------------------------------------------------------------------------ 1. pool backward
def _pool_table(rng, nq, ns, h, kind):
    """A pooling / upsampling table [nq, h] over ns supports: support 0 listed by more than 64 queries, support 1 by one,
    support 2 by none, a row that lists a support twice, shadow entries (== ns); 'shadow': every entry is shadow."""
    if kind == "shadow":
        return np.full((nq, h), ns, np.int32)
    idx = rng.integers(3, ns, size=(nq, h)).astype(np.int32)
    idx[rng.random((nq, h)) < 0.2] = ns
    if nq:
        idx[: min(nq, 100), 0] = 0
        idx[min(nq, 101) - 1, h - 1] = 1
        idx[nq // 2, 1] = idx[nq // 2, 2] = 5
    return idx


def _max_pool_restatement(go, arg, ns, base):
    """gx[s, c] = base[s, c] + go[q1, c] + go[q2, c] + ... over ascending q with arg[q, c] == s, added left to right in f32."""
    gx = np.zeros((ns, go.shape[1]), np.float32) if base is None else base.astype(np.float32).copy()
    cols = np.arange(go.shape[1])
    for q in range(go.shape[0]):
        live = arg[q] < ns
        gx[arg[q, live], cols[live]] = gx[arg[q, live], cols[live]] + go[q, live]
    return gx


def _closest_pool_restatement(go, idx0, ns, c):
    gx = np.zeros((ns, c), np.float32)
    for n in range(go.shape[0]):
        if 0 <= idx0[n] < ns:
            gx[idx0[n]] = gx[idx0[n]] + go[n, :c]
    return gx


POOL_SHAPES = [(150, 70, 5, 4, "mixed"), (150, 70, 5, 6, "mixed"), (150, 70, 5, 128, "mixed"), (150, 70, 5, 260, "mixed"),
               (40, 70, 5, 8, "shadow"), (0, 70, 5, 8, "mixed"), (1030, 300, 3, 64, "mixed")]


@pytest.mark.parametrize("nq,ns,h,c,kind", POOL_SHAPES)
@pytest.mark.parametrize("incoming", [False, True])
def test_max_pool_backward_gather(nq, ns, h, c, kind, incoming):
    L = _native.lib()
    rng = np.random.default_rng([nq, ns, c, int(incoming)])
    idx = _pool_table(rng, nq, ns, h, kind)
    pick = rng.integers(0, h, size=(nq, c))
    arg = np.take_along_axis(idx, pick, axis=1).astype(np.int32) if nq else np.zeros((0, c), np.int32)   # an entry of the row
    go = rng.normal(size=(nq, c)).astype(np.float32)
    base = rng.normal(size=(ns, c)).astype(np.float32) if incoming else None
    ptr, ent = ops._csr_of(cu(idx), ns)
    s = torch.cuda.current_stream().cuda_stream
    t_go, t_arg, t_base = cu(go), cu(arg), (cu(base) if incoming else None)
    outs = []
    for _ in range(2):
        gx = torch.full((ns, c), float("nan"), device=DEV)      # every row is written: no clear launch
        _native.check(L.d3f_max_pool_backward_gather(ops._p(t_go) if nq else None, ops._p(t_arg) if nq else None, nq, c,
                                                     ns, ops._p(ptr), ops._p(ent), ops._p(t_base), ops._p(gx), s), "gather")
        outs.append(gx)
    torch.cuda.synchronize()
    want = _max_pool_restatement(go, arg, ns, base)
    assert np.array_equal(bits(outs[0]), bits(want))
    assert np.array_equal(bits(outs[0]), bits(outs[1]))
    if incoming:    # in place on top of the incoming gradient, as _MaxPoolFn does when it adopts the collected tensor
        gx = t_base.clone()
        _native.check(L.d3f_max_pool_backward_gather(ops._p(t_go) if nq else None, ops._p(t_arg) if nq else None, nq, c,
                                                     ns, ops._p(ptr), ops._p(ent), ops._p(gx), ops._p(gx), s), "gather")
        assert np.array_equal(bits(gx), bits(want))
    if nq == 0:
        return
    # the float-atomic kernel it replaces: the same terms in arrival order
    at = t_base.clone() if incoming else torch.zeros((ns, c), device=DEV)
    _native.check(L.d3f_max_pool_backward(ops._p(t_go), ops._p(t_arg), nq, c, ns, ops._p(at), 1, s), "scatter")
    n_terms = np.zeros((ns, c)) + (1 if incoming else 0)
    abs_sum = np.abs(base).astype(np.float64) if incoming else np.zeros((ns, c))
    cols = np.arange(c)
    for q in range(nq):
        live = arg[q] < ns
        n_terms[arg[q, live], cols[live]] += 1
        abs_sum[arg[q, live], cols[live]] += np.abs(go[q, live])
    diff = np.abs(at.cpu().numpy().astype(np.float64) - want.astype(np.float64))
    assert (diff <= order_bound(n_terms, abs_sum)).all(), float(diff.max())


@pytest.mark.parametrize("nq,ns,h,c,kind", POOL_SHAPES)
@pytest.mark.parametrize("extra", [0, 12])       # ld > C: a column slice of a wider gradient is read in place
def test_closest_pool_backward_gather(nq, ns, h, c, kind, extra):
    L = _native.lib()
    rng = np.random.default_rng([nq, ns, c, extra])
    idx = _pool_table(rng, nq, ns, h, kind)
    if nq > 8 and kind == "mixed":
        idx[3, 0], idx[4, 0] = -1, ns + 7           # indices outside [0, ns)
    ld = c + extra
    wide = rng.normal(size=(nq, ld)).astype(np.float32)
    t_wide = cu(wide)
    ptr, ent = ops._csr_of(cu(np.ascontiguousarray(idx[:, :1])), ns)
    s = torch.cuda.current_stream().cuda_stream
    outs = []
    for _ in range(2):
        gx = torch.full((ns, c), float("nan"), device=DEV)
        _native.check(L.d3f_closest_pool_backward_gather(ops._p(t_wide) if nq else None, ld, nq, c, ns, ops._p(ptr),
                                                         ops._p(ent), ops._p(gx), s), "gather")
        outs.append(gx)
    torch.cuda.synchronize()
    want = _closest_pool_restatement(wide, idx[:, 0], ns, c)
    assert np.array_equal(bits(outs[0]), bits(want))
    assert np.array_equal(bits(outs[0]), bits(outs[1]))
    if nq == 0:
        return
    at = torch.zeros((ns, c), device=DEV)
    _native.check(L.d3f_closest_pool_backward(ops._p(t_wide), ld, ops._p(cu(idx)), nq, h, c, ns, ops._p(at), 1, s), "scatter")
    ok = (idx[:, 0] >= 0) & (idx[:, 0] < ns)
    n_terms = np.repeat(np.bincount(idx[ok, 0], minlength=ns)[:, None], c, axis=1)
    abs_sum = np.zeros((ns, c))
    np.add.at(abs_sum, idx[ok, 0], np.abs(wide[ok, :c]).astype(np.float64))
    diff = np.abs(at.cpu().numpy().astype(np.float64) - want.astype(np.float64))
    assert (diff <= order_bound(n_terms, abs_sum)).all(), float(diff.max())


def test_pool_nodes_follow_the_mode_of_their_forward():
    """ops.max_pool (with an incoming gradient and a deposit) and ops.closest_pool: the node takes the gather form when its
    FORWARD ran under the mode, whatever the mode is at backward time, and the scatter form otherwise."""
    rng = np.random.default_rng(11)
    nq, ns, h, c = 150, 70, 5, 32
    idx = _pool_table(rng, nq, ns, h, "mixed")
    x = rng.normal(size=(ns, c)).astype(np.float32)
    go = rng.normal(size=(nq, c)).astype(np.float32)
    inc = rng.normal(size=(ns, c)).astype(np.float32)
    res = {}
    for mode in (False, True):
        holder_in, holder_out = ops.GradHolder(), ops.GradHolder()
        assert holder_in.deposit(cu(inc).clone())
        tx = cu(x).requires_grad_(True)
        with ops.deterministic_mode(mode):
            y = ops.max_pool(tx, cu(idx), grad_deposit=holder_out, grad_incoming=holder_in)
            z = ops.closest_pool(tx, cu(idx))
        before = dict(ops.DISPATCH_COUNTS)
        y.backward(cu(go), retain_graph=True)
        pooled = holder_out.collect()
        gz, = torch.autograd.grad(z, tx, cu(go))
        torch.cuda.synchronize()
        kind, other = ('ordered', 'scatter') if mode else ('scatter', 'ordered')
        assert ops.DISPATCH_COUNTS[kind] == before[kind] + 2 and ops.DISPATCH_COUNTS[other] == before[other]
        res[mode] = (pooled.cpu().numpy(), gz.cpu().numpy())
    assert rel_err(res[True][0], res[False][0]) < 1e-6 and rel_err(res[True][1], res[False][1]) < 1e-6
    # the incoming gradient is the first term of every element
    arg = res[True][0] - inc
    assert np.abs(arg[2]).max() == 0.0      # support 2 is listed by nobody: its row is the incoming gradient itself


# ------------------------------------------------------------------------------------------------ 2. KPConv grad-input
def _check_grad_input_is_a_gather(ns, ch, block, mode=('linear', 'sum')):
    rng = np.random.default_rng([ns, ch])
    h = 12
    q, s, idx, x, kp, w = _kpconv_case(rng, ns, ns, h, ch, ch)
    bias = rng.normal(size=ch).astype(np.float32) * 0.1
    d = lambda a: torch.from_numpy(a).double()
    tx, tw = d(x).requires_grad_(True), d(w).requires_grad_(True)
    ref = ops_ref.kpconv(d(q), d(s), torch.from_numpy(idx), tx, d(kp), tw, SPARSE_EXTENT, *mode)
    if block:
        ref = torch.nn.functional.leaky_relu(ref + d(bias), 0.1)
    go = rng.normal(size=tuple(ref.shape)).astype(np.float32)
    ref.backward(d(go))

    class Prof:
        records = []
    tab = cu(idx, torch.int32)
    ops.build_reverse_table(tab, ns)
    grads = []
    for rep in range(2):
        gx, gw = cu(x).requires_grad_(True), cu(w).requires_grad_(True)
        before = dict(ops.DISPATCH_COUNTS)
        Prof.records = []
        ops.set_profiler(Prof)
        try:
            with ops.deterministic_mode(True):
                if block:
                    out = ops.kpconv_bias_act(cu(q), cu(s), tab, gx, cu(kp), gw, SPARSE_EXTENT, cu(bias))
                else:
                    out = ops.kpconv(cu(q), cu(s), tab, gx, cu(kp), gw, SPARSE_EXTENT, *mode)
            out.backward(cu(go))
        finally:
            ops.set_profiler(None)
        torch.cuda.synchronize()
        labels = [r[0] for r in Prof.records]
        assert not any(l.startswith("kpconv_dx_scatter") or l.startswith("kpconv_bwd[") for l in labels), labels
        assert any(l.startswith("kpconv_dx_gather" if block else "kpconv_ordered_dx") for l in labels), labels
        assert ops.DISPATCH_COUNTS['scatter'] == before['scatter']
        grads.append((gx.grad.clone(), gw.grad.clone()))
    assert rel_err(out.detach().cpu().numpy(), ref.detach().numpy()) < 2e-5
    assert rel_err(grads[0][0].cpu().numpy(), tx.grad.numpy()) < BWD_TOL
    assert rel_err(grads[0][1].cpu().numpy(), tw.grad.numpy()) < BWD_TOL
    assert np.array_equal(bits(grads[0][0]), bits(grads[1][0]))
    assert np.array_equal(bits(grads[0][1]), bits(grads[1][1]))


@pytest.mark.parametrize("ns", [37, 159])
@pytest.mark.parametrize("ch", [64, 512])
@pytest.mark.parametrize("block", [True, False])
def test_kpconv_grad_input_is_a_gather_at_few_rows(ns, ch, block):
    """Below ops.DX_GATHER_MIN_ROWS the default grad-input is the float-atomic scatter; under the mode the block's node
    (aggregation + GEMM, d3f_kpconv_grad_input_gather) and ops.kpconv's order-fixed node both gather.  Against float64."""
    _check_grad_input_is_a_gather(ns, ch, block)


@pytest.mark.parametrize("mode", [("gaussian", "closest"), ("constant", "sum")], ids="-".join)
def test_kpconv_grad_input_is_a_gather_at_a_non_default_mode(mode):
    """The block=False arm of the test above (ops.kpconv's general-path node, gather form) at the other influence /
    aggregation modes, against ops_ref.kpconv in float64 with the same bounds (tests/test_kpconv_cases_cpu.py holds the
    float32 oracle to them on these inputs)."""
    _check_grad_input_is_a_gather(37, 64, False, mode)


# ------------------------------------------------------------------------------------------------ 3. sparse loss backward
def _loss_case():
    """Two stacked pairs (two normaliser groups), M = 5, C = 32, H = 7, with the collisions the atomic form is sensitive to:
    pair 0 samples anchor row 3 twice; its anchor row 4 is a neighbor of anchor row 3 (and both are given the same winning
    channel: feature rows with their maximum at channel 9); the group's arg-max position is element (3, 9), a target of the
    c* terms of row 3 and of the neighbor term of row 4."""
    rng = np.random.default_rng(5)
    lens = np.array([40, 36, 44, 38], np.int32)
    n, c, h, m = int(lens.sum()), 32, 7, 5
    x = (rng.random((n, c)).astype(np.float32) * 0.5 + 0.1)
    x[3, 9], x[4, 9] = 3.0, 2.5          # (3, 9) is the maximum of group 0
    x[100, 17] = 2.75                     # the maximum of group 1
    off = np.concatenate([[0], np.cumsum(lens)])
    nb = np.empty((n, h), np.int32)
    for b in range(4):                    # neighbors inside the row's own cloud, itself first
        rows = np.arange(off[b], off[b + 1])
        nb[rows, 0] = rows
        nb[rows, 1:] = rng.integers(off[b], off[b + 1], size=(len(rows), h - 1))
    nb[:, h - 1] = n                      # a shadow entry in every row
    nb[3, 1], nb[4, 1] = 4, 3             # rows 3 and 4 are neighbors of each other
    corr = np.stack([np.stack([rng.permutation(lens[2 * p])[:m], rng.permutation(lens[2 * p + 1])[:m]], 1)
                     for p in range(2)]).astype(np.int64)          # cloud-local rows
    corr[0, 0, 0], corr[0, 1, 0], corr[0, 2, 0] = 3, 3, 4          # anchor row 3 twice, then its neighbor 4
    dk = rng.random((2, m, m)) * 0.5
    for p in range(2):
        np.fill_diagonal(dk[p], 0.0)
    return x, nb, lens, corr, (dk > 0.1).astype(np.uint8)


def _loss_backward(case, mode, debug=None, monkeypatch=None):
    x, nb, lens, corr, mask = case
    tx = cu(x).requires_grad_(True)
    t_lens = cu(lens)
    det = ops.DetectorRows(cu(nb), training=True, lens=t_lens, group=2)
    if debug is not None:
        monkeypatch.setattr(ops, "_LOSS_RECORDS", debug)
    with ops.deterministic_mode(mode):
        total = ops.train_loss_pairs(tx, det, cu(corr), t_lens, neg_mask=cu(mask))[0]
    total.backward()
    torch.cuda.synchronize()
    return tx.grad.detach().clone(), float(total.detach())


def test_sparse_loss_backward_is_the_ordered_sum_of_its_records(monkeypatch):
    case = _loss_case()
    x, nb, lens, corr, mask = case
    n, c = x.shape
    debug = {}
    g_det, loss_det = _loss_backward(case, True, debug, monkeypatch)
    monkeypatch.setattr(ops, "_LOSS_RECORDS", None)
    g_again, _ = _loss_backward(case, True)
    g_atomic, loss_atomic = _loss_backward(case, False)
    assert loss_det == loss_atomic
    assert np.array_equal(bits(g_det), bits(g_again))
    key, val, width = debug['key'].cpu().numpy(), debug['val'].cpu().numpy(), debug['width']
    tie = debug['tie_terms'].cpu().numpy()
    rows = 2 * 2 * 5
    assert width == c + 3 + nb.shape[1] and key.shape == (rows * width,)
    nrec = rows * width
    live = key != np.iinfo(np.int64).max
    rec = np.nonzero(live)[0]
    assert np.array_equal(key[live] % nrec, rec)        # record r carries its own index
    elem = key[live] // nrec
    # the header's order: ascending sampled row m2, inside a row normalise, c*, c', neighbors by slot == ascending record
    want = np.zeros(n * c, np.float32)
    n_terms, abs_sum = np.zeros(n * c), np.zeros(n * c)
    for r, e in zip(rec, elem):
        want[e] = want[e] + val[r]
        n_terms[e] += 1
        abs_sum[e] += abs(float(val[r]))
    off = np.concatenate([[0], np.cumsum(lens)])
    tie_at = []
    for gi in range(2):                                  # ... and the group's arg-max term last
        blk = x[off[2 * gi]:off[2 * gi + 2]]
        mx = max(float(blk.max()), 0.0)
        for e in np.nonzero(blk.reshape(-1) == np.float32(mx))[0] + off[2 * gi] * c:
            want[e] = want[e] + tie[gi]
            n_terms[e] += 1
            abs_sum[e] += abs(float(tie[gi]))
            tie_at.append(int(e))
    assert np.array_equal(bits(g_det.reshape(-1)), bits(want))
    # the constructed collisions are there
    assert tie_at[0] == 3 * c + 9 and n_terms[3 * c + 9] >= 5     # normalise x2, c* x2, neighbor of row 4, arg-max
    assert (n_terms.reshape(n, c)[3] >= 2).all()                  # row 3 is sampled twice
    diff = np.abs(g_atomic.cpu().numpy().astype(np.float64).reshape(-1) - want.astype(np.float64))
    bound = order_bound(n_terms, abs_sum)
    print("\nsparse loss backward: max |atomic - ordered| = %.3e, bound there %.3e, elements with > 1 term: %d" % (
        diff.max(), bound[diff.argmax()], int((n_terms > 1).sum())))
    assert (diff <= bound).all()


def test_select_normalize_ordered_without_the_rows_detector():
    """ops.select_normalize (dense scores: the score gradient takes the records' last slot) under the mode: the same
    values as the atomic form, the same bits twice."""
    rng = np.random.default_rng(9)
    n, c, m = 90, 32, 6
    x = rng.normal(size=(n, c)).astype(np.float32)
    sc = rng.random((n, 1)).astype(np.float32)
    ia = np.array([3, 3, 7, 11, 3, 20], np.int64)
    ip = np.array([5, 9, 5, 5, 30, 31], np.int64)
    w = [rng.normal(size=(m, c)).astype(np.float32), rng.normal(size=(m, c)).astype(np.float32),
         rng.normal(size=m).astype(np.float32), rng.normal(size=m).astype(np.float32)]
    res = {}
    for mode in (True, True, False):
        tx, ts = cu(x).requires_grad_(True), cu(sc).requires_grad_(True)
        with ops.deterministic_mode(mode):
            outs = ops.select_normalize(tx, ts, cu(ia), cu(ip), p_offset=40)
        sum((o * cu(v)).sum() for o, v in zip(outs, w)).backward()
        res.setdefault(mode, []).append((tx.grad.clone(), ts.grad.clone()))
    for k in range(2):
        assert np.array_equal(bits(res[True][0][k]), bits(res[True][1][k]))
        assert rel_err(res[True][0][k].cpu().numpy(), res[False][0][k].cpu().numpy()) < 1e-5


# ------------------------------------------------------------------------------------------------ 4. whole steps
def _s0(golden_s0):
    g = golden_s0
    n0, n1 = g['pts0'].shape[0], g['pts1'].shape[0]
    raw = (g['pts0'], g['pts1'], np.ones((n0, 1), np.float32), np.ones((n1, 1), np.float32), g['sel_corr'],
           g['dist_keypts_in'])
    item = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in raw)
    swapped = (item[1], item[0], item[3], item[2], item[4].flip(1).contiguous(), item[5].t().contiguous())
    limits = [int(x) for x in g['limits']]
    sizes = [int(g['batch.points.%d' % l].shape[0]) for l in range(5)]
    return item, swapped, limits, sizes


def _fresh(cfg, limits, deterministic=True):
    from d3feat_pytorch_amd.train import TrainStep
    np.random.seed(0)
    torch.manual_seed(0)
    return TrainStep(cfg, limits, torch.device(DEV), seed=0, deterministic=deterministic)


def _run(kind, cfg, item, swapped, limits, sizes):
    """Four steps of one schedule on a fresh engine: (parameters, losses) afterwards."""
    from d3feat_pytorch_amd.train import PairLanes, TrainStep
    t = _fresh(cfg, limits)
    seq = [item, swapped, item, swapped]
    m = int(item[4].shape[0])
    if kind == "eager":
        losses = [t.step(it)[0] for it in seq]
    elif kind == "graph":
        t.enable_graph(TrainStep.capacities_for([sizes], slack=1.3), num_corr=m)
        t.capture(item)
        losses = [t.step_graph(it, seq[k + 1] if k + 1 < 4 else None)[0] for k, it in enumerate(seq)]
        assert t.check_status() == (0, 0)
    elif kind == "stack2":
        t.enable_graph(TrainStep.capacities_for([[2 * v for v in sizes]], slack=1.3), num_corr=m, stack=2)
        t.capture((item, swapped))
        groups = [(item, swapped), (swapped, item), (item, item), (swapped, swapped)]
        losses = [t.step_graph(gr, groups[k + 1] if k + 1 < 4 else None)[0] for k, gr in enumerate(groups)]
        assert t.check_status() == (0, 0)
    else:
        lanes = PairLanes(t, 2)
        lanes.enable_graph(TrainStep.capacities_for([sizes], slack=1.3), num_corr=m)
        lanes.capture(item)
        groups = [[item, swapped], [swapped, item], [item, item], [swapped, swapped]]
        losses = []
        for k, gr in enumerate(groups):
            outs = lanes.step_graph(gr, groups[k + 1] if k + 1 < 4 else None)
            lanes.synchronize()
            losses += [o[0] for o in outs]
        assert lanes.check_status() == (0, 0)
    torch.cuda.synchronize()
    assert int(t.opt.skipped) == 0
    return t.flat.data.clone(), torch.stack([l.reshape(-1)[0].float() for l in losses]).cpu()


@pytest.mark.parametrize("kind", ["eager", "graph", "stack2", "lanes2"])
def test_two_runs_of_a_deterministic_schedule_agree_bit_for_bit(golden_s0, kind):
    """The S0 pair and configuration of profiles/determinism_check.py: two fresh engines, four steps each."""
    item, swapped, limits, sizes = _s0(golden_s0)
    cfg = cfgmod.default_config(first_features_dim=16, num_node=64)
    (pa, la), (pb, lb) = (_run(kind, cfg, item, swapped, limits, sizes) for _ in range(2))
    assert torch.isfinite(la).all() and float((pa - _fresh(cfg, limits).flat.data).abs().max()) > 0      # it trained
    assert np.array_equal(bits(la), bits(lb)), (la, lb)
    assert np.array_equal(bits(pa), bits(pb)), float((pa - pb).abs().max())


def test_adam_contrastive_steps_agree_bit_for_bit(golden_s0):
    item, swapped, limits, sizes = _s0(golden_s0)
    cfg = cfgmod.default_config(first_features_dim=16, num_node=64, optimizer='ADAM', desc_loss='contrastive', lr=1e-3)
    (pa, la), (pb, lb) = (_run("eager", cfg, item, swapped, limits, sizes) for _ in range(2))
    assert np.array_equal(bits(la), bits(lb)) and np.array_equal(bits(pa), bits(pb))


def _step_gradient(t, item):
    batch = t.build_batch(item)
    batch['n0'] = int(item[0].shape[0])
    t.flat.zero_grad()
    prof = type("Prof", (), {"records": []})
    ops.set_profiler(prof)
    try:
        loss = t.forward_loss(batch)[0]
        with ops.weight_grad_group():
            torch.autograd.backward(loss)
    finally:
        ops.set_profiler(None)
    torch.cuda.synchronize()
    return t.flat.gather_grads().clone(), float(loss), [r[0] for r in prof.records]


def test_deterministic_gradient_equals_the_default_gradient(golden_s0):
    """One step's gradient under the mode against the default mode's, within the bound test_graph_mode_matches_eager_step
    holds its two paths to (1e-4 of the largest entry; losses 2e-3); no scatter form is launched under the mode."""
    item, _, limits, _ = _s0(golden_s0)
    cfg = cfgmod.default_config(first_features_dim=16, num_node=64)
    before = dict(ops.DISPATCH_COUNTS)
    g_det, l_det, labels = _step_gradient(_fresh(cfg, limits, True), item)
    assert ops.DISPATCH_COUNTS['scatter'] == before['scatter'] and ops.DISPATCH_COUNTS['ordered'] > before['ordered']
    assert not any(l.startswith("kpconv_dx_scatter") or l.startswith("kpconv_bwd[") for l in labels)
    assert not ops.is_deterministic()
    g_def, l_def, _ = _step_gradient(_fresh(cfg, limits, False), item)
    assert abs(l_det - l_def) < 2e-3 * max(1.0, abs(l_def))
    assert float((g_det - g_def).abs().max()) < 1e-4 * float(g_def.abs().max())


# ------------------------------------------------------------------------------------------------ 5. no ordered form: raise
def test_operators_without_an_ordered_form_raise_under_the_mode():
    rng = np.random.default_rng(2)
    nq = ns = 60
    q, s, idx, x, kp, w = _kpconv_case(rng, nq, ns, 9, 16, 16)
    offsets = (rng.normal(size=(nq, 15, 3)) * 0.005).astype(np.float32)
    args = lambda: (cu(q), cu(s), cu(idx, torch.int32), cu(x).requires_grad_(True), cu(kp), cu(w).requires_grad_(True),
                    SPARSE_EXTENT, cu(offsets))
    out = ops.kpconv_deformable(*args())[0]         # runs as before without the mode
    out.sum().backward()
    feat = cu(np.abs(x[:, :16]) + 0.1).requires_grad_(True)
    ops.detection_scores(feat, cu(idx, torch.int32)).sum().backward()
    with ops.deterministic_mode(True):
        with pytest.raises(RuntimeError, match="kpconv_deformable does not have a deterministic implementation"):
            ops.kpconv_deformable(*args())
        with pytest.raises(RuntimeError, match="detection_scores .* does not have a deterministic implementation"):
            ops.detection_scores(cu(np.abs(x[:, :16]) + 0.1).requires_grad_(True), cu(idx, torch.int32))
        # inference (nothing to differentiate) is not affected
        with torch.no_grad():
            ops.kpconv_deformable(*args())
    assert not ops.is_deterministic()


# ------------------------------------------------------------------------------------------------ 6. mode off: as before
def test_mode_off_takes_the_scatter_forms_as_before(golden_s0):
    """With the mode off the step's dispatch is the parent's: below ops.DX_GATHER_MIN_ROWS support rows the KPConv
    grad-input is the scatter form (every level of the S0 pair but the first), no table of those levels is transposed, and
    no order-fixed form is launched."""
    item, _, limits, sizes = _s0(golden_s0)
    cfg = cfgmod.default_config(first_features_dim=16, num_node=64)
    t = _fresh(cfg, limits, False)
    batch = t.build_batch(item)
    for tab, pts in zip(batch['neighbors'], batch['points']):
        if tab.shape[0]:
            assert (getattr(tab, '_d3f_rev', None) is not None) == (pts.shape[0] >= ops.DX_GATHER_MIN_ROWS)
    before = dict(ops.DISPATCH_COUNTS)
    _, _, labels = _step_gradient(t, item)
    few = [n for n in sizes if n < ops.DX_GATHER_MIN_ROWS]
    assert few and ops.DISPATCH_COUNTS['ordered'] == before['ordered'] and ops.DISPATCH_COUNTS['scatter'] > before['scatter']
    scatters = [l for l in labels if l.startswith("kpconv_dx_scatter")]
    assert scatters and not any(l.startswith(("max_pool_bwd_gather", "closest_pool_bwd_gather", "loss_rows_bwd_ordered",
                                              "kpconv_ordered")) for l in labels)
    with ops.deterministic_mode(True):
        det_batch = t.build_batch(item)
    assert all(getattr(tab, '_d3f_rev', None) is not None for tab in det_batch['neighbors'] if tab.shape[0])
