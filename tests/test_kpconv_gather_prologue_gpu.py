"""The prologues of the KPConv gather kernels: index rows, query positions and kernel points are loaded unconditionally
from clamped addresses with the select on the value, and ``nn == NULL`` (a gradient that is already divided by nn) is a
compile-time case of the transposed kernels.  Held here, at the smallest shapes at which that can go wrong:

* forward aggregation (d3f_kpconv_aggregate): dead rows inside a wave, a partial workgroup, every step count, lanes
  >= H, the dead sixteenth kernel-point lane, CV 1 / 2 / 4 and two channel chunks, all-shadow rows, negative and
  oversized entries;
* transposed aggregation (d3f_kpconv_aggregate_transposed) and grad-input (d3f_kpconv_grad_input_gather, all three table
  forms): empty and full reverse rows, rows longer than 64 entries, the Cin slabs that select WK = 1 / 2 / 4, each with
  nn given and with nn = NULL on a pre-divided gradient;
* the input-layer kernels and the fused forward / grad-weights through ops.kpconv.

References: oracle/ops_ref.kpconv and its autograd at the tolerances of test_gpu_ops.py::test_kpconv_forward_backward;
every kernel bit-identical to itself on a second call, and bit-identical when every input is a slice of a larger
allocation whose neighbouring elements are poison (NaN features and positions, in-range but wrong indices): a read
outside a tensor shows as a changed bit, not as a fault."""
import functools

import numpy as np
import pytest
import torch

from d3feat_pytorch_amd import _native, ops
from oracle import ops_ref
from util import rel_err

DEV = "cuda:0"
FWD_TOL = 2e-5   # test_gpu_ops.py
BWD_TOL = 2e-4
PAD = 64         # poison elements on either side of an embedded input (a multiple of 4: float4 rows stay 16-byte aligned)
EXT = 0.06

# (Nq, H, K, Cin, Ns): Nq 1/3/17/65, H 1/15/16/17/42/64, K 1/15/16, Cin 16/32/64/128, Ns 1/40
FWD_CASES = [(1, 1, 1, 16, 1), (3, 15, 15, 32, 40), (17, 16, 16, 64, 40), (65, 17, 15, 128, 40), (17, 42, 15, 16, 40),
             (65, 64, 16, 32, 40), (3, 64, 1, 64, 1), (65, 42, 15, 128, 1), (17, 1, 15, 32, 40)]
# (W, Ns, Cout, Cin, K): W 1/7/64/65/130, Ns 1/5/18, Cout -> CV 1/2/4 and two chunks, Cin 64/32/16 -> WK 1/2/4
REV_CASES = [(1, 1, 16, 16, 1), (7, 5, 32, 32, 15), (64, 18, 64, 64, 16), (65, 5, 128, 16, 15), (130, 18, 32, 64, 15)]
REV_NQ = 150     # >= the widest row, so that full rows exist at every width


def cu(a):
    return torch.as_tensor(np.array(a)).to(DEV)      # (a copy: the shared cases are read-only)


def embedded(a, poison):
    """`a` as a slice inside a larger device allocation filled with `poison` (same dtype)."""
    a = np.ascontiguousarray(a)
    flat = np.full(a.size + 2 * PAD, poison, dtype=a.dtype) if not isinstance(poison, np.ndarray) else \
        np.resize(poison.astype(a.dtype), a.size + 2 * PAD)
    flat[PAD:PAD + a.size] = a.reshape(-1)
    whole = torch.as_tensor(flat).to(DEV)
    view = whole[PAD:PAD + a.size].view(a.shape)
    view._whole = whole
    return view


def bits(t):
    return t.detach().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ forward cases
@functools.lru_cache(maxsize=None)
def fwd_case(nq, h, k, cin, ns):
    rng = np.random.default_rng([nq, h, k, cin, ns])
    q = rng.uniform(0, 0.1, (nq, 3)).astype(np.float32)
    s = rng.uniform(0, 0.1, (ns, 3)).astype(np.float32)
    idx = rng.integers(0, ns + 1, (nq, h)).astype(np.int32)          # ns = the shadow index
    if nq >= 3:
        idx[1, :] = ns                                               # an all-shadow row
    hostile = idx.copy()                                             # negative and oversized entries: shadow too
    if nq >= 3:
        rows = rng.integers(0, nq, 6)
        cols = rng.integers(0, h, 6)
        hostile[rows, cols] = np.array([-1, -5, ns + 1, ns + 1000, 2 ** 31 - 1, -2 ** 31], np.int64).astype(np.int32)
    clean = np.where((hostile < 0) | (hostile > ns), ns, hostile).astype(np.int32)
    x = rng.normal(size=(ns, cin)).astype(np.float32)
    kp = (rng.normal(size=(k, 3)) * 0.03).astype(np.float32)
    cout = 8
    w = (rng.normal(size=(k, cin, cout)) / np.sqrt(k * cin)).astype(np.float32)
    ref = ops_ref.kpconv(torch.from_numpy(q), torch.from_numpy(s), torch.from_numpy(clean), torch.from_numpy(x),
                         torch.from_numpy(kp), torch.from_numpy(w), EXT).numpy()
    for a in (q, s, hostile, clean, x, kp, w, ref):
        a.setflags(write=False)
    return q, s, hostile, clean, x, kp, w, ref


def test_forward_cases_hold_the_conditions_they_are_chosen_for():
    """Restated in NumPy, no GPU: an all-shadow row, a partial last wave, lanes >= H, the dead sixteenth lane, negative
    and oversized entries are all present in the set (and the first three in every case of three rows or more)."""
    seen_neg = seen_big = False
    for nq, h, k, cin, ns in FWD_CASES:
        _, _, hostile, clean, _, _, _, _ = fwd_case(nq, h, k, cin, ns)
        assert nq % 4 != 0 and nq % 16 != 0                          # the last wave and the last workgroup are partial
        if nq >= 3:
            assert (clean == ns).all(axis=1).any()                   # an all-shadow row
            assert (clean < ns).any()
        seen_neg |= bool((hostile < 0).any())
        seen_big |= bool((hostile > ns).any())
        assert clean.min() >= 0 and clean.max() <= ns
    assert seen_neg and seen_big
    assert {(c[1] + 15) // 16 for c in FWD_CASES} == {1, 2, 3, 4}    # every step count
    assert any(c[1] % 16 for c in FWD_CASES) and {c[2] for c in FWD_CASES} == {1, 15, 16}
    assert {c[3] for c in FWD_CASES} == {16, 32, 64, 128} and {c[4] for c in FWD_CASES} == {1, 40}


def run_aggregate(q, s, idx, x, kp, k):
    L = _native.lib()
    nq, h, ns, cin = q.shape[0], idx.shape[1], s.shape[0], x.shape[1]
    wf = torch.full((nq, k * cin), float("nan"), dtype=torch.float32, device=DEV)
    nn = torch.full((nq,), float("nan"), dtype=torch.float32, device=DEV)
    nbytes = L.d3f_kpconv_ws_bytes(nq, ns, h, k, cin, 64)
    ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=DEV)
    _native.check(L.d3f_kpconv_aggregate(q.data_ptr(), nq, s.data_ptr(), ns, idx.data_ptr(), h, x.data_ptr(), cin,
                                         kp.data_ptr(), k, EXT, wf.data_ptr(), nn.data_ptr(), None, None, ws.data_ptr(),
                                         nbytes, torch.cuda.current_stream().cuda_stream), "d3f_kpconv_aggregate")
    torch.cuda.synchronize()
    return wf, nn


@pytest.mark.gpu
@pytest.mark.parametrize("nq,h,k,cin,ns", FWD_CASES)
def test_forward_aggregation(nq, h, k, cin, ns):
    q, s, hostile, clean, x, kp, w, ref = fwd_case(nq, h, k, cin, ns)
    wf, nn = run_aggregate(cu(q), cu(s), cu(hostile), cu(x), cu(kp), k)
    out = (wf.cpu().numpy().astype(np.float64) @ w.reshape(k * cin, -1).astype(np.float64)) / nn.cpu().numpy()[:, None]
    err = rel_err(out, ref)
    print("\nPROLOGUE fwd %s out=%.2e" % ((nq, h, k, cin, ns), err))
    assert err < FWD_TOL
    # negative / oversized entries behave like the shadow index, bit for bit
    wf_c, nn_c = run_aggregate(cu(q), cu(s), cu(clean), cu(x), cu(kp), k)
    assert torch.equal(bits(wf), bits(wf_c)) and torch.equal(bits(nn), bits(nn_c))
    # a second call gives the same bits
    wf2, nn2 = run_aggregate(cu(q), cu(s), cu(hostile), cu(x), cu(kp), k)
    assert torch.equal(bits(wf), bits(wf2)) and torch.equal(bits(nn), bits(nn2))
    # every input a slice of a larger allocation with poison around it: nothing outside the tensors reaches the result
    nanf = np.float32("nan")
    wf_p, nn_p = run_aggregate(embedded(q, nanf), embedded(s, nanf), embedded(hostile, np.int32(0)), embedded(x, nanf),
                               embedded(kp, nanf), k)
    assert torch.equal(bits(wf), bits(wf_p)) and torch.equal(bits(nn), bits(nn_p))


@pytest.mark.gpu
@pytest.mark.parametrize("nq,h,k,cin,cout,ns", [(17, 17, 15, 1, 32, 40), (3, 42, 16, 2, 64, 40), (65, 64, 15, 4, 16, 1),
                                                (17, 17, 15, 16, 16, 40), (65, 42, 16, 32, 32, 40), (3, 15, 1, 64, 64, 1)])
def test_input_layer_and_fused_kernels_through_ops(nq, h, k, cin, cout, ns):
    """ops.kpconv forward + backward (the input-layer kernels at Cin <= 4, the fused forward and grad-weights above)
    against the oracle and its autograd."""
    rng = np.random.default_rng([nq, h, k, cin, cout, ns])
    q = rng.uniform(0, 0.1, (nq, 3)).astype(np.float32)
    s = rng.uniform(0, 0.1, (ns, 3)).astype(np.float32)
    idx = rng.integers(0, ns + 1, (nq, h)).astype(np.int64)
    idx[1, :] = ns
    x = rng.normal(size=(ns, cin)).astype(np.float32)
    kp = (rng.normal(size=(k, 3)) * 0.03).astype(np.float32)
    w = (rng.normal(size=(k, cin, cout)) / np.sqrt(k * cin)).astype(np.float32)
    go = rng.normal(size=(nq, cout)).astype(np.float32)
    tx, tw = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(w).requires_grad_(True)
    ref = ops_ref.kpconv(torch.from_numpy(q), torch.from_numpy(s), torch.from_numpy(idx), tx, torch.from_numpy(kp), tw, EXT)
    ref.backward(torch.from_numpy(go))
    outs = []
    for _ in range(2):
        gx, gw = cu(x).requires_grad_(True), cu(w).requires_grad_(True)
        out = ops.kpconv(cu(q), cu(s), cu(idx), gx, cu(kp), gw, EXT)
        out.backward(cu(go))
        outs.append(out.detach())
    errs = (rel_err(out.detach().cpu().numpy(), ref.detach().numpy()), rel_err(gx.grad.cpu().numpy(), tx.grad.numpy()),
            rel_err(gw.grad.cpu().numpy(), tw.grad.numpy()))
    print("\nPROLOGUE ops %s out=%.2e grad_x=%.2e grad_w=%.2e" % (((nq, h, k, cin, cout, ns),) + errs))
    assert errs[0] < FWD_TOL
    assert errs[1] < BWD_TOL
    assert errs[2] < BWD_TOL
    if cin <= 4:      # (the fused forward may combine channel chunks with float atomics; the input-layer kernel does not)
        assert torch.equal(bits(outs[0]), bits(outs[1]))


# ------------------------------------------------------------------------------------------------ transposed cases
@functools.lru_cache(maxsize=None)
def rev_case(width, ns, cout, cin, k):
    """A reverse graph drawn directly: row s lists cnt[s] distinct queries (row 0 full, row 1 empty when there is one), a
    few of them `outsiders` that the search form lists without their being members.  Returns the inputs of all three
    table forms, the forward table they are the transpose of, and the oracle's grad_x for a gradient `go`."""
    nq = REV_NQ
    rng = np.random.default_rng([width, ns, cout, cin, k])
    q = rng.uniform(0, 0.1, (nq, 3)).astype(np.float32)
    s = rng.uniform(0, 0.1, (ns, 3)).astype(np.float32)
    cnt = rng.integers(0, width + 1, ns)
    cnt[0] = width
    if ns > 1:
        cnt[1] = 0
    outsider = np.zeros(nq, bool)
    outsider[rng.choice(nq, 9, replace=False)] = True
    listed = [np.sort(rng.choice(nq, c, replace=False)) for c in cnt]           # what the search form's rows hold
    members = [row[~outsider[row]] for row in listed]                            # what really lists s
    # exact form: float4 {q - s, bits of q}, compacted, padded with Nq
    rel = np.zeros((ns, width, 4), np.float32)
    rel[:, :, 3] = np.int32(nq).view(np.float32)
    for si, row in enumerate(members):
        rel[si, :row.size, :3] = q[row] - s[si]
        rel[si, :row.size, 3] = row.astype(np.int32).view(np.float32)
    # CSR form
    ptr = np.concatenate([[0], np.cumsum([m.size for m in members])]).astype(np.int32)
    ent_csr = (np.concatenate(members) if ptr[-1] else np.zeros(0, np.int64)).astype(np.int32)
    ent_csr = np.concatenate([ent_csr, np.full(1, nq, np.int32)])               # (never an empty allocation)
    # search form: every listed query, members or not; an outsider's last key admits nothing, a member's everything
    ent_tab = np.full((ns, width), nq, np.int32)
    for si, row in enumerate(listed):
        ent_tab[si, :row.size] = row
    last_key = np.where(outsider, np.uint64(0), np.uint64(2 ** 64 - 1)).astype(np.uint64)
    # the forward table this is the transpose of
    per_q = [[] for _ in range(nq)]
    for si, row in enumerate(members):
        for qi in row:
            per_q[qi].append(si)
    h = max(1, max(len(r) for r in per_q))
    idx = np.full((nq, h), ns, np.int64)
    for qi, r in enumerate(per_q):
        idx[qi, :len(r)] = r
    x = rng.normal(size=(ns, cin)).astype(np.float32)
    kp = (rng.normal(size=(k, 3)) * 0.03).astype(np.float32)
    w = (rng.normal(size=(k, cin, cout)) / np.sqrt(k * cin)).astype(np.float32)
    go = rng.normal(size=(nq, cout)).astype(np.float32)
    x_pad = np.concatenate([x, np.zeros((1, cin), np.float32)])
    nn = np.maximum((x_pad[idx].sum(-1) > 0).sum(-1), 1).astype(np.float32)     # blocks.py:377-379
    gon = (go / nn[:, None]).astype(np.float32)
    tx = torch.from_numpy(x).requires_grad_(True)
    ops_ref.kpconv(torch.from_numpy(q), torch.from_numpy(s), torch.from_numpy(idx), tx, torch.from_numpy(kp),
                   torch.from_numpy(w), EXT).backward(torch.from_numpy(go))
    case = dict(q=q, s=s, rel=rel, ptr=ptr, ent_csr=ent_csr, ent_tab=ent_tab, last_key=last_key, kp=kp, w=w, go=go,
                nn=nn, gon=gon, ref=tx.grad.numpy(), cnt=np.array([m.size for m in members]), listed=cnt)
    for v in case.values():
        v.setflags(write=False)
    return case


def test_reverse_cases_hold_the_conditions_they_are_chosen_for():
    """Restated in NumPy, no GPU: empty rows, full rows and a row longer than 64 entries are present."""
    longest = 0
    for width, ns, cout, cin, k in REV_CASES:
        c = rev_case(width, ns, cout, cin, k)
        assert c["listed"][0] == width                                          # a full row (of the search form)
        if ns > 1:
            assert c["cnt"][1] == 0                                             # an empty row
        assert ns % 4 != 0                                                      # the last wave is partial
        longest = max(longest, int(c["cnt"].max()))
    assert longest > 64 and max(c[0] for c in REV_CASES) > 128
    assert {c[0] for c in REV_CASES} == {1, 7, 64, 65, 130} and {c[1] for c in REV_CASES} == {1, 5, 18}


def device_inputs(c, poison):
    nanf = np.float32("nan")
    if not poison:
        d = {k: cu(c[k]) for k in ("q", "s", "rel", "ptr", "ent_csr", "ent_tab", "kp", "w", "go", "nn", "gon")}
        d["last_key"] = cu(c["last_key"].view(np.int64))
        return d
    rel_poison = np.array([nanf, nanf, nanf, 0.0], np.float32)                   # NaN offsets, query 0: in range, wrong
    d = dict(q=embedded(c["q"], nanf), s=embedded(c["s"], nanf), rel=embedded(c["rel"], rel_poison),
             ptr=embedded(c["ptr"], np.int32(0)), ent_csr=embedded(c["ent_csr"], np.int32(0)),
             ent_tab=embedded(c["ent_tab"], np.int32(0)),
             last_key=embedded(c["last_key"].view(np.int64), np.int64(-1)),      # (a key that admits everything)
             kp=embedded(c["kp"], nanf), w=embedded(c["w"], nanf), go=embedded(c["go"], nanf),
             nn=embedded(c["nn"], nanf), gon=embedded(c["gon"], nanf))
    return d


def run_transposed(d, width, ns, cout, k, with_nn):
    L = _native.lib()
    agg = torch.full((ns, k * cout), float("nan"), dtype=torch.float32, device=DEV)
    g = d["go"] if with_nn else d["gon"]
    _native.check(L.d3f_kpconv_aggregate_transposed(d["rel"].data_ptr(), width, ns, REV_NQ, d["kp"].data_ptr(), k, EXT,
                                                    d["nn"].data_ptr() if with_nn else None, g.data_ptr(), cout,
                                                    agg.data_ptr(), torch.cuda.current_stream().cuda_stream),
                  "d3f_kpconv_aggregate_transposed")
    torch.cuda.synchronize()
    return agg


def run_grad_input(d, form, width, ns, cin, cout, k, with_nn):
    L = _native.lib()
    gx = torch.full((ns, cin), float("nan"), dtype=torch.float32, device=DEV)
    g = d["go"] if with_nn else d["gon"]
    ptr = d["ptr"].data_ptr() if form == "csr" else None
    ent = d["ent_csr"].data_ptr() if form == "csr" else (d["ent_tab"].data_ptr() if form == "search" else None)
    lk = d["last_key"].data_ptr() if form == "search" else None
    rel = d["rel"].data_ptr() if form == "exact" else None
    _native.check(L.d3f_kpconv_grad_input_gather(d["q"].data_ptr(), REV_NQ, d["s"].data_ptr(), ns, ptr, ent, lk, width, 0.0,
                                                 rel, d["kp"].data_ptr(), k, d["w"].data_ptr(), cin, cout, EXT,
                                                 d["nn"].data_ptr() if with_nn else None, g.data_ptr(), gx.data_ptr(),
                                                 None, torch.cuda.current_stream().cuda_stream),
                  "d3f_kpconv_grad_input_gather")
    torch.cuda.synchronize()
    return gx


@pytest.mark.gpu
@pytest.mark.parametrize("with_nn", [True, False], ids=["nn", "prediv"])
@pytest.mark.parametrize("width,ns,cout,cin,k", REV_CASES)
def test_transposed_aggregation(width, ns, cout, cin, k, with_nn):
    c = rev_case(width, ns, cout, cin, k)
    d = device_inputs(c, poison=False)
    agg = run_transposed(d, width, ns, cout, k, with_nn)
    wt = np.transpose(c["w"], (0, 2, 1)).reshape(k * cout, cin).astype(np.float64)     # W'[k, o, c] = W[k, c, o]
    err = rel_err(agg.cpu().numpy().astype(np.float64) @ wt, c["ref"])
    print("\nPROLOGUE agg_rev %s nn=%s grad_x=%.2e" % ((width, ns, cout, cin, k), with_nn, err))
    assert err < BWD_TOL
    assert torch.equal(bits(agg), bits(run_transposed(d, width, ns, cout, k, with_nn)))
    assert torch.equal(bits(agg), bits(run_transposed(device_inputs(c, poison=True), width, ns, cout, k, with_nn)))


@pytest.mark.gpu
@pytest.mark.parametrize("with_nn", [True, False], ids=["nn", "prediv"])
@pytest.mark.parametrize("form", ["exact", "search", "csr"])
@pytest.mark.parametrize("width,ns,cout,cin,k", REV_CASES)
def test_grad_input_gather(width, ns, cout, cin, k, form, with_nn):
    c = rev_case(width, ns, cout, cin, k)
    d = device_inputs(c, poison=False)
    gx = run_grad_input(d, form, width, ns, cin, cout, k, with_nn)
    err = rel_err(gx.cpu().numpy(), c["ref"])
    print("\nPROLOGUE dx_gather %s %s nn=%s grad_x=%.2e" % ((width, ns, cout, cin, k), form, with_nn, err))
    assert err < BWD_TOL
    assert torch.equal(bits(gx), bits(run_grad_input(d, form, width, ns, cin, cout, k, with_nn)))
    assert torch.equal(bits(gx), bits(run_grad_input(device_inputs(c, poison=True), form, width, ns, cin, cout, k,
                                                     with_nn)))
