"""GPU: the detector on the sampled rows of the training loss (ops.DetectorRows -> d3f_detection_rows_forward/backward).

The loss reads the scores of the 2 P M sampled correspondences only (reference trainer.py:90-97), so the fused loss node
scores those rows itself -- with the dense kernel's own device function -- and scatters their gradient into the one
[N, C] buffer the descriptor rows already use.  Checked here against the float64 autograd oracle (oracle.ops_ref), against
the dense path (the switch), stacked against single pairs, outside the rows form's domain, and under graph replay.

Shapes are the smallest at which the rows form can go wrong: 600 live rows + 37 capacity rows, C in {16, 32, 64} (the
three instantiations), H in {5, 37, 64} (a partial, an exact and several batches of G*SB neighbor slots), M = 16 rows per
side, one pair and three stacked pairs of unequal lengths."""
import numpy as np
import pytest
import torch

from d3feat_pytorch_amd import ops
from d3feat_pytorch_amd.utils.loss import ContrastiveLoss
from oracle import ops_ref
from util import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

FWD_TOL = 2e-5   # the project's tolerances (tests/test_gpu_ops.py)
BWD_TOL = 2e-4
M = 16
PAD = 37
LENS = {1: [320, 280], 3: [130, 90, 60, 140, 110, 70]}
MARGINS = (0.1, 0.1, 1.4)   # safe_radius, pos_margin, neg_margin


def cu(a, dtype=None):
    t = torch.as_tensor(a)
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV)


class Case(object):
    """Seeded inputs of one shape.  The index table keeps every pair's neighbors inside the pair (or shadow, == N), so
    the oracle can score each pair on its own sub-batch, as the reference does with its one-pair batches."""

    def __init__(self, C, H, P, variant="plain", seed=0):
        rng = np.random.default_rng(1000 * C + 10 * H + P + seed)
        self.C, self.H, self.P = C, H, P
        self.lens = np.array(LENS[P], np.int32)
        self.off = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)
        self.n_live = int(self.off[-1])
        self.N = N = self.n_live + PAD
        self.group = 2 if P > 1 else 0            # one pair: the capacity-shaped batch's lens without groups
        x = rng.normal(size=(N, C)).astype(np.float32)
        x[self.n_live:] *= 0.1                    # capacity rows: below every group's maximum
        idx = np.full((N, H), N, np.int32)
        corr = np.zeros((P, M, 2), np.int64)
        self.peak = []                            # (row, channel) of every group's planted maximum
        for p in range(P):
            a0, a1 = int(self.off[2 * p]), int(self.off[2 * p + 2])
            r = rng.integers(a0, a1 + (a1 - a0) // 3, size=(a1 - a0, H))
            idx[a0:a1] = np.where(r >= a1, N, r)                       # about a quarter shadow entries
            la, lp = int(self.lens[2 * p]), int(self.lens[2 * p + 1])
            # the group's maximum sits in a row that is neither sampled nor anybody's neighbor: its gradient entry is
            # the normaliser's term alone
            peak = a0 + 5
            tab = idx[a0:a1]
            tab[tab == peak] = N
            corr[p, :, 0] = rng.permutation(np.arange(6, la))[:M]
            corr[p, :, 1] = rng.permutation(lp)[:M]
            x[peak, 3 % C] = 7.0 + p
            self.peak.append((peak, 3 % C))
        idx[:, 0] = np.arange(N)                                       # column 0 is the row itself
        a = self.off[0] + corr[0, :, 0]
        idx[a[0], :] = N                                               # a sampled row with shadow neighbors only
        idx[a[1], min(1, H - 1)] = a[2]                                # a sampled row neighbors another sampled row
        corr[0, 4, 0] = corr[0, 3, 0]                                  # a row sampled twice
        g0 = slice(0, int(self.off[2])) if P > 1 else slice(0, N)
        if variant == "ties":                                          # group 0's maximum attained twice
            second = int(self.off[0]) + 4
            tab = idx[g0]
            tab[tab == second] = N
            idx[second, 0] = second
            x[second, 5 % C] = x[self.peak[0]]
            self.peak.append((second, 5 % C))
        elif variant == "nonpositive":                                 # mx = 0: the maximum is the shadow row's zero
            x[g0] = -(np.abs(x[g0]) + 0.1)                             # (no real row attains it: its term reaches no x)
            self.peak = self.peak[1:]
        elif variant in ("zeros1", "zeros40"):                         # mx = 0 attained by real elements as well
            x[g0] = -(np.abs(x[g0]) + 0.1)
            self.peak = self.peak[1:]
            zero_rows = [int(self.off[0]) + r for r in range(4)]       # never sampled (anchors start at local row 6)
            tab = idx[g0]
            tab[np.isin(tab, zero_rows)] = N                           # ... and nobody's neighbors
            idx[zero_rows, 0] = zero_rows
            cells = [(zero_rows[2], 7 % C)] if variant == "zeros1" else [(r, c) for r in zero_rows for c in range(10)]
            for r, c in cells:
                x[r, c] = 0.0
            self.zeros = cells
            self.peak = cells + self.peak
        self.x, self.idx, self.corr = x, idx, corr
        self.dk = rng.random((P, M, M)) * 0.3
        self.dk = np.minimum(self.dk, self.dk.transpose(0, 2, 1))

    # ---- rows of the stacked batch that the loss samples
    def rows(self):
        a = np.concatenate([self.off[2 * p] + self.corr[p, :, 0] for p in range(self.P)])
        b = np.concatenate([self.off[2 * p + 1] + self.corr[p, :, 1] for p in range(self.P)])
        return a, b

    def pair_range(self, p):
        if self.P == 1:
            return 0, self.n_live
        return int(self.off[2 * p]), int(self.off[2 * p + 2])

    def sub_table(self, p, table=None):
        a0, a1 = self.pair_range(p)
        tab = (self.idx if table is None else table)[a0:a1]
        return np.where(tab >= self.N, a1 - a0, tab - a0).astype(np.int64)

    def detector(self, table=None, training=True, width=None):
        return ops.DetectorRows(cu(self.idx if table is None else table), training=training, lens=cu(self.lens),
                                width=width, group=self.group)

    def dense_scores(self, x, table=None, training=True, width=None):
        return ops.detection_scores(x, cu(self.idx if table is None else table), training=training, lens=cu(self.lens),
                                    width=width, group=self.group)

    def loss(self, x, scores, kind):
        """(total, desc [P], det [P]) of the fused loss node in the form the training step uses for P pairs."""
        if self.P == 1:
            f = ops.train_loss if kind == "circle" else ops.train_contrastive_loss
            args = (10.0,) + MARGINS if kind == "circle" else MARGINS
            res = f(x, scores, cu(self.corr[0]), int(self.lens[0]), cu(self.dk[0]), *args)
            return res[0], res[1].reshape(1), res[2].reshape(1)
        f = ops.train_loss_pairs if kind == "circle" else ops.train_contrastive_loss_pairs
        args = (10.0,) + MARGINS if kind == "circle" else MARGINS
        res = f(x, scores, cu(self.corr), cu(self.lens), cu(self.dk), *args)
        return res[0], res[1], res[2]

    # ---- the float64 oracle: per pair ops_ref.detection_scores on its own sub-batch + the oracle's loss
    def oracle_scores(self, tx, training=True, table=None, widths=None):
        out = []
        for p in range(self.P):
            a0, a1 = self.pair_range(p)
            sub = self.sub_table(p, table)
            if widths is not None:
                sub = sub[:, :int(widths[p])]
            out.append(ops_ref.detection_scores(tx[a0:a1], torch.from_numpy(sub), training=training))
        return out

    def oracle(self, kind):
        tx = torch.from_numpy(self.x.astype(np.float64)).requires_grad_(True)
        scores = self.oracle_scores(tx)
        f = torch.nn.functional.normalize(tx, p=2, dim=-1)
        total, descs, dets = 0.0, [], []
        for p in range(self.P):
            a0, _ = self.pair_range(p)
            ia = torch.from_numpy(self.corr[p, :, 0])
            ip = torch.from_numpy(self.corr[p, :, 1] + int(self.lens[2 * p]))
            dk = torch.from_numpy(self.dk[p])
            if kind == "circle":
                desc, _, _, _, dists = ops_ref.circle_loss(f[a0 + ia], f[a0 + ip], dk, 10.0, *MARGINS)
            else:
                desc, _, _, _, _, dists = ContrastiveLoss(MARGINS[1], MARGINS[2], 'euclidean', MARGINS[0])(
                    f[a0 + ia], f[a0 + ip], dk)
            det = ops_ref.det_loss(dists, scores[p][ia], scores[p][ip])
            total = total + desc + det
            descs.append(float(desc.detach()))
            dets.append(float(det.detach()))
        total.backward()
        flat = torch.cat([s.detach().reshape(-1) for s in scores]).numpy()
        return flat, np.array(descs), np.array(dets), tx.grad.numpy()


def rows_scores(case, x, det):
    """sa, sp of the rows form alone (the launches _TrainLossFn makes before the loss kernels)."""
    P = case.P
    assert x.dtype == torch.float32 and x.is_contiguous()
    fmax = ops.global_max(x, det.lens, det.group)
    if P == 1:
        corr, off, lens = cu(case.corr[0]), ops._p_offset(int(case.lens[0]), x.device), None
    else:
        corr, off, lens = cu(case.corr).view(P * M, 2), None, cu(case.lens)
    _, _, sa, sp, saved, stride = ops._select_rows_fwd(x, None, corr, off, lens, P, M)
    ops._det_rows_fwd(x, det, fmax, saved, stride, P, M, sa, sp, False)
    return sa, sp


def run_both(case, kind):
    """Gradient of x through the rows form and through the dense path (the switch), plus the losses."""
    out = []
    for sparse in (True, False):
        gx = cu(case.x).requires_grad_(True)
        scores = case.detector() if sparse else case.dense_scores(gx)
        total, desc, det = case.loss(gx, scores, kind)
        total.backward()
        out.append((float(total), desc.detach().cpu().numpy(), det.detach().cpu().numpy(), gx.grad.cpu().numpy()))
    return out


def quiet_rows(case):
    """Rows that are neither sampled, nor neighbors of a sampled row, nor hold an arg-max of a normaliser."""
    touched = np.zeros(case.N + 1, bool)
    a, b = case.rows()
    rows = np.concatenate([a, b])
    touched[rows] = True
    touched[case.idx[rows].reshape(-1)] = True
    for r, _ in case.peak:
        touched[r] = True
    return ~touched[:case.N]


SHAPES = [(c, h, p) for c in (16, 32, 64) for h in (5, 37, 64) for p in (1, 3)]
VARIANTS = [(32, 37, 1, "ties"), (32, 37, 3, "ties"), (16, 5, 3, "ties"), (32, 37, 1, "nonpositive"),
            (64, 64, 3, "nonpositive"), (16, 37, 3, "nonpositive")]


@pytest.mark.parametrize("C,H,P,variant", [s + ("plain",) for s in SHAPES] + VARIANTS)
def test_rows_form_against_the_oracle_and_the_dense_path(C, H, P, variant):
    case = Case(C, H, P, variant)
    assert ops.DetectorRows.supported(C, H)
    # forward: the same device function as the dense kernel
    x = cu(case.x)
    sa, sp = rows_scores(case, x, case.detector())
    dense = case.dense_scores(x).reshape(-1)
    a, b = case.rows()
    assert torch.equal(sa, dense[cu(a)]) and torch.equal(sp, dense[cu(b)])
    for kind in ("circle", "contrastive"):
        ref_scores, ref_desc, ref_det, ref_grad = case.oracle(kind)
        if kind == "circle":
            err = rel_err(dense[:case.n_live].cpu().numpy(), ref_scores)
            print("scores vs oracle: %.3g" % err)
            assert err < FWD_TOL
        (tot_s, desc_s, det_s, g_s), (tot_d, desc_d, det_d, g_d) = run_both(case, kind)
        e_or, e_de = rel_err(g_s, ref_grad), rel_err(g_s, g_d)
        print("%s: grad vs oracle %.3g, vs dense %.3g, desc %.3g, det %.3g" % (
            kind, e_or, e_de, np.abs(desc_s - ref_desc).max(), np.abs(det_s - ref_det).max()))
        assert np.array_equal(desc_s, desc_d) and np.array_equal(det_s, det_d) and tot_s == tot_d
        assert np.abs(desc_s - ref_desc).max() < 1e-5 * max(1.0, np.abs(ref_desc).max())
        # det = mean (fp - cn)(sa + sp): the scores' tolerance on the scores' own scale (1e6 where the normaliser is 1e-6)
        assert np.abs(det_s - ref_det).max() < FWD_TOL * max(1.0, np.abs(ref_det).max(), np.abs(ref_scores).max())
        assert e_or < BWD_TOL
        assert e_de < 1e-5
        quiet = quiet_rows(case)
        assert quiet.sum() >= PAD             # (the capacity rows at least; most live rows at H = 5)
        assert np.all(g_s[quiet] == 0.0)
        for r, c in case.peak:
            assert g_s[r, c] != 0.0          # the normaliser's term reached the arg-max position


@pytest.mark.parametrize("C,H,P", [(32, 37, 1), (16, 64, 3), (64, 5, 3)])
def test_rows_form_in_evaluation_mode_with_a_table_width(C, H, P):
    """training = 0 adds the local-maximum gate; ``width`` trims a table kept wider than the reference would build it."""
    case = Case(C, H, P)
    rng = np.random.default_rng(C + H)
    groups = P if P > 1 else 1
    widths = np.array([max(2, H - 2 - 2 * g) for g in range(groups)], np.int32)
    table = case.idx.copy()
    for p in range(P):
        a0, a1 = case.pair_range(p)
        table[a0:a1, widths[p]:] = case.N
    table[case.n_live:, widths[-1]:] = case.N
    # mostly negative features: the shadow's zero is a live candidate of the gate
    x = cu((-np.abs(case.x) + (rng.random(case.x.shape) < 0.02)).astype(np.float32))
    width = cu(widths)
    sa, sp = rows_scores(case, x, case.detector(table, training=False, width=width))
    dense = case.dense_scores(x, table, training=False, width=width).reshape(-1)
    a, b = case.rows()
    assert torch.equal(sa, dense[cu(a)]) and torch.equal(sp, dense[cu(b)])
    tx = x.detach().cpu().double()
    ref = torch.cat([s.reshape(-1) for s in case.oracle_scores(tx, False, table, widths)]).numpy()
    got = dense[:case.n_live].cpu().numpy()
    assert np.array_equal(got != 0, ref != 0)
    assert rel_err(got, ref) < FWD_TOL
    # evaluation through the loss node: no backward, same losses as with the dense scores
    with torch.no_grad():
        t_rows = case.loss(x, case.detector(table, training=False, width=width), "circle")
        t_dense = case.loss(x, dense.reshape(-1, 1), "circle")
    assert all(torch.equal(u, v) for u, v in zip(t_rows, t_dense))


@pytest.mark.parametrize("kind", ["circle", "contrastive"])
def test_stacked_pairs_equal_the_single_pair_results(kind):
    case = Case(32, 37, 3)
    gx = cu(case.x).requires_grad_(True)
    total, desc, det = case.loss(gx, case.detector(), kind)
    total.backward()
    want_grad = torch.zeros_like(gx)
    want = 0.0
    for p in range(3):
        a0, a1 = case.pair_range(p)
        px = cu(case.x[a0:a1]).requires_grad_(True)
        one = ops.DetectorRows(cu(case.sub_table(p).astype(np.int32)), training=True)
        f = ops.train_loss if kind == "circle" else ops.train_contrastive_loss
        args = (10.0,) + MARGINS if kind == "circle" else MARGINS
        t1, d1, e1 = f(px, one, cu(case.corr[p]), int(case.lens[2 * p]), cu(case.dk[p]), *args)[:3]
        t1.backward()
        want_grad[a0:a1] += px.grad
        want += float(t1)
        assert abs(float(desc[p]) - float(d1)) < 1e-6 and abs(float(det[p]) - float(e1)) < 1e-6
    assert abs(float(total) - want) < 1e-5 * max(1.0, abs(want))
    assert float((gx.grad - want_grad).abs().max()) <= 1e-6 * float(want_grad.abs().max()) + 1e-9


def test_channel_count_outside_the_rows_form_takes_the_dense_path():
    case = Case(48, 37, 3)
    assert not ops.DetectorRows.supported(48, 37)
    for kind in ("circle", "contrastive"):
        _, ref_desc, ref_det, ref_grad = case.oracle(kind)
        gx = cu(case.x).requires_grad_(True)
        total, desc, det = case.loss(gx, case.detector(), kind)
        total.backward()
        assert np.abs(desc.detach().cpu().numpy() - ref_desc).max() < 1e-5 * max(1.0, np.abs(ref_desc).max())
        assert np.abs(det.detach().cpu().numpy() - ref_det).max() < FWD_TOL * max(1.0, np.abs(ref_det).max())
        assert rel_err(gx.grad.cpu().numpy(), ref_grad) < BWD_TOL


def test_graph_replays_agree_and_the_tie_term_keeps_its_bits():
    case = Case(32, 37, 3, "ties")
    gx = cu(case.x).requires_grad_(True)
    det = case.detector()
    corr, lens, dk = cu(case.corr), cu(case.lens), cu(case.dk)
    neg_mask = (dk > MARGINS[0]).to(torch.uint8).contiguous()

    def step():
        total = ops.train_loss_pairs(gx, det, corr, lens, None, 10.0, *MARGINS, neg_mask=neg_mask)[0]
        return total, torch.autograd.grad(total, gx)[0]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = step()[1].clone()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        total, grad = step()
    runs = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        runs.append(grad.clone())
    drift = float((runs[1] - runs[0]).abs().max())
    assert drift <= 2e-5 * float(runs[0].abs().max())
    assert float((runs[0] - eager).abs().max()) <= 2e-5 * float(eager.abs().max())
    for r, c in case.peak:      # rows nothing else writes: the entry IS the normaliser's term
        bits = [int(t[r:r + 1, c].view(torch.int32).item()) for t in (runs[0], runs[1], eager)]
        assert float(runs[0][r, c]) != 0.0 and bits[0] == bits[1] == bits[2]


@pytest.mark.parametrize("C,H,P,variant", [(32, 37, 3, "zeros1"), (16, 5, 1, "zeros1"), (32, 37, 3, "zeros40"),
                                           (64, 64, 1, "zeros40")])
def test_real_zeros_tie_with_the_shadow_row_as_the_dense_path_counts_them(C, H, P, variant):
    """A group without a positive feature: mx = 0 is attained by the zero shadow row and by every real element that is
    exactly 0.  The project counts the shadow row as ONE tie (det_reduce_kernel / det_finalize_kernel; the rows form keeps
    that meaning), so k real zeros share the normaliser's term as 1 / (k + 1) each.  torch's autograd of the oracle counts
    the shadow row's C zero elements separately (1 / (k + C)), so this case is compared with the dense path, not with the
    oracle.  k = 1 walks the arg-max list; k = 40 overflows its 32 entries and takes the rescan."""
    case = Case(C, H, P, variant)
    k = len(case.zeros)
    assert int((case.x[:case.pair_range(0)[1]] == 0.0).sum()) == k
    for kind in ("circle", "contrastive"):
        (tot_s, desc_s, det_s, g_s), (tot_d, desc_d, det_d, g_d) = run_both(case, kind)
        err = rel_err(g_s, g_d)
        print("%s %s: grad vs dense %.3g, tie entry %.6g (dense %.6g)" % (variant, kind, err, g_s[case.zeros[0]],
                                                                      g_d[case.zeros[0]]))
        assert tot_s == tot_d and np.array_equal(desc_s, desc_d) and np.array_equal(det_s, det_d)
        assert err < 1e-5
        tie = np.array([g_s[z] for z in case.zeros])
        assert tie[0] != 0.0 and np.all(tie == tie[0])       # nothing else writes these entries: the term itself
        want = np.array([g_d[z] for z in case.zeros], np.float64)
        assert np.abs(tie - want).max() <= 1e-5 * np.abs(want).max()
        assert np.all(g_s[quiet_rows(case)] == 0.0)
