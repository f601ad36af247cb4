"""Tensor-level operators over the C ABI (device tensors in, device tensors out, autograd where the reference
has it).  Every function here launches hand-written HIP kernels from ``libd3feat_hip.so``; none has a PyTorch or
CPU fallback.  Reference locations are cited per operator.
"""
import collections
import numpy as np
import ctypes
import threading

import torch

from . import _native

ORDER_REFERENCE = _native.D3F_ORDER_REFERENCE    # row order of the reference's std::unordered_map iteration (grid_subsampling.cpp:85)
ORDER_FIRST_SEEN = _native.D3F_ORDER_FIRST_SEEN  # cells in order of their first input point


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------------------------
# optional per-operator HIP-event timing (bench.py): events are recorded on the stream the kernels are launched on
# ---------------------------------------------------------------------------------------------------------------
_PROFILER = None


def set_profiler(p):
    global _PROFILER
    _PROFILER = p


class _Region:
    def __init__(self, prof, label, nbytes):
        self.prof, self.label, self.nbytes = prof, label, nbytes

    def __enter__(self):
        if self.prof is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record(torch.cuda.current_stream())
        return self

    def __exit__(self, *exc):
        if self.prof is not None:
            self.e1.record(torch.cuda.current_stream())
            self.prof.records.append((self.label, self.nbytes, self.e0, self.e1))
        return False


def _region(label, nbytes=0):
    return _Region(_PROFILER, label, nbytes)


class EventProfiler:
    """Collects (label, algorithmic bytes, start event, end event) per C-ABI call; summary() after a sync."""

    def __init__(self):
        self.records = []

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for label, nbytes, e0, e1 in self.records:
            ms = e0.elapsed_time(e1)
            d = out.setdefault(label, {"calls": 0, "total_ms": 0.0, "bytes_per_call": nbytes})
            d["calls"] += 1
            d["total_ms"] += ms
        for d in out.values():
            d["avg_ms"] = d["total_ms"] / d["calls"]
        return out


def kpconv_fwd_bytes(Nq, Ns, H, K, Cin, Cout):
    """Algorithmic (gather-expanded, int32-index) bytes of one KPConv forward -- SURVEY.md section 8d."""
    return 12 * Nq + 4 * Nq * H + Nq * H * (12 + 4 * Cin) + 4 * K * Cin * Cout + 180 + 4 * Nq * Cout


def kpconv_bwd_bytes(Nq, Ns, H, K, Cin, Cout):
    return kpconv_fwd_bytes(Nq, Ns, H, K, Cin, Cout) + 4 * Nq * Cout + 4 * Ns * Cin + 4 * K * Cin * Cout


def _f32(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s must be a CUDA/HIP tensor (d3feat_pytorch_amd has no CPU path)" % name)
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _opt_f32(t, name):
    return _f32(t, name) if t is not None else None


def _i32(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s must be a CUDA/HIP tensor (d3feat_pytorch_amd has no CPU path)" % name)
    if t.dtype != torch.int32:
        t = t.to(torch.int32)  # the reference hands LongTensors (dataloader.py:161-163)
    return t.contiguous()


def _lens(t, device, name):
    """Stack lengths as an int32 device tensor (accepts lists / CPU tensors like the reference's q_batches)."""
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t, dtype=torch.int32)
    return t.to(device=device, dtype=torch.int32).contiguous().view(-1)


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _p(t):
    return t.data_ptr() if t is not None else None


SPACK_READY = 1   # D3F_SPACK_READY of the C ABI: "spack_keep already holds the packed supports"


class PackedSupports(object):
    """What the epilogue that produced a KPConv's input features left behind for it (d3f_bias_act_forward_pack): the
    packed supports {x, y, z, [row sum > 0]} of (s_pts, x) and, optionally, the cleared grad_x scatter target.  Rides on
    the feature tensor as ``x._d3f_spack``; the KPConv operators use it instead of launching their own packing kernel."""
    __slots__ = ("spack", "gx_buf", "s_ptr", "rows", "cols")

    def __init__(self, spack, gx_buf, s_pts, rows, cols):
        self.spack, self.gx_buf, self.s_ptr, self.rows, self.cols = spack, gx_buf, s_pts.data_ptr(), int(rows), int(cols)

    def fits(self, s_pts, x):
        return self.s_ptr == s_pts.data_ptr() and self.rows == int(x.shape[0]) == int(s_pts.shape[0]) and \
            self.cols == int(x.shape[1])


class DeviceStatus:
    """int32 device word the kernels OR error bits into; checked at the caller's next natural sync."""

    def __init__(self, device):
        self.word = torch.zeros(1, dtype=torch.int32, device=device)

    def raise_if_set(self):
        v = int(self.word.item())
        if v:
            raise RuntimeError(_native.status_message(v) or ("device status %d" % v))


# ---------------------------------------------------------------------------------------------------------------
# radius neighbors (cpp_wrappers/cpp_neighbors; datasets/dataloader.py:52-67)
# ---------------------------------------------------------------------------------------------------------------
class RadiusGrid:
    """Cell list of one support cloud for one radius; serves any number of query sets."""

    def __init__(self, supports, s_len, radius, status=None, ws=None):
        """``ws``: a workspace (``RadiusGrid.workspace(Ns, device)``) whose bucket counters the caller has cleared already
        (``zero_buffers``): a pyramid build clears all of its cell lists with one launch."""
        self.supports = _f32(supports, "supports")
        if self.supports.dim() != 2 or self.supports.shape[1] != 3:
            raise RuntimeError("Wrong dimensions : support.shape is not (N, 3)")
        dev = self.supports.device
        self.s_len = _lens(s_len, dev, "s_batches")
        self.radius = float(radius)
        self.status = status if status is not None else DeviceStatus(dev)
        L = _native.lib()
        self.Ns = int(self.supports.shape[0])
        nbytes = L.d3f_radius_grid_ws_bytes(self.Ns)
        build = L.d3f_radius_grid_build if ws is None else L.d3f_radius_grid_build_prezeroed
        if ws is not None and ws.numel() < nbytes:
            raise RuntimeError("cell-list workspace of %d bytes, %d needed" % (ws.numel(), nbytes))
        self.ws = _ws(nbytes, dev) if ws is None else ws
        with _region("radius_grid_build[Ns=%d]" % self.Ns, 12 * self.Ns + 24 * self.Ns):
            _native.check(build(_p(self.supports), self.Ns, _p(self.s_len), int(self.s_len.numel()), self.radius,
                                _p(self.ws), nbytes, _p(self.status.word), _stream()), "d3f_radius_grid_build")

    @staticmethod
    def workspace(Ns, device):
        """(workspace for a cell list over ``Ns`` supports, the leading part of it that must be cleared before the build)"""
        L = _native.lib()
        ws = _ws(L.d3f_radius_grid_ws_bytes(int(Ns)), device)
        return ws, ws[:int(L.d3f_radius_grid_zero_bytes(int(Ns)))]

    def query_prefix(self, queries, q_len, width, prefix_radius, radius=None, nearest_bound=0.0):
        """Prefix form (d3f_radius_query_prefix): int32 [Nq, width] rows = the supports within ``prefix_radius``, ranked as
        the leading part of the ``query`` row -- or the single nearest support within the search radius when there is
        none.  For tables of which only column 0 and the part within ``prefix_radius`` are ever read (the upsampling
        tables inside the training engine).  ``nearest_bound`` > 0: the caller guarantees a support within that distance
        of every query; cells beyond it are not scanned."""
        q = _f32(queries, "queries")
        q_len = _lens(q_len, q.device, "q_batches")
        Nq = int(q.shape[0])
        r = self.radius if radius is None else float(radius)
        out = torch.empty((Nq, int(width)), dtype=torch.int32, device=q.device)
        with _region("radius_query_prefix[Nq=%d,Ns=%d]" % (Nq, self.Ns), 12 * Nq + 12 * self.Ns + 4 * Nq * int(width)):
            _native.check(_native.lib().d3f_radius_query_prefix(
                _p(self.ws), _p(q), Nq, _p(q_len), self.Ns, _p(self.s_len), int(q_len.numel()), self.radius, r,
                float(prefix_radius), float(nearest_bound), int(width), _p(out), _p(self.status.word), _stream()),
                "d3f_radius_query_prefix")
        return out

    def query_pool_transposed(self, queries, q_len, width, max_group=0, mx_out=None, counts=None):
        """A pooling search over this (fine) cloud -- (table, device max count(s), last kept keys) as
        ``query(want_max=True, want_last_key=True)`` -- that also leaves its transpose behind: ``(counts [Ns] int32, keys
        [32 Ns] int64)``, per fine point the (d2 bits, coarse query) keys of the coarse queries that found it
        (d3f_radius_query_pool_transposed); ``RadiusGrid.prefix_rows_from_transposed`` ranks them into upsampling rows."""
        q = _f32(queries, "queries")
        q_len = _lens(q_len, q.device, "q_batches")
        if q_len.numel() != self.s_len.numel():
            raise RuntimeError("Wrong number of batch elements: different for queries and supports ")
        Nq = int(q.shape[0])
        out = torch.empty((Nq, int(width)), dtype=torch.int32, device=q.device)
        n_mx = -(-int(q_len.numel()) // int(max_group)) if max_group else 1
        mx = mx_out if mx_out is not None else torch.zeros(n_mx, dtype=torch.int32, device=q.device)
        if mx.numel() != n_mx or mx.dtype != torch.int32:
            raise RuntimeError("mx_out must hold %d int32 counters" % n_mx)
        lkey = torch.empty(Nq, dtype=torch.int64, device=q.device)
        if counts is None:          # (``counts``: [Ns] int32 the caller has cleared -- a pyramid build clears all at once)
            counts = torch.empty(self.Ns, dtype=torch.int32, device=q.device)
            zero_buffers([counts])
        elif counts.numel() != self.Ns or counts.dtype != torch.int32:
            raise RuntimeError("counts must hold %d int32 counters" % self.Ns)
        keys = torch.empty(32 * max(self.Ns, 1), dtype=torch.int64, device=q.device)
        with _region("radius_query_pool_transposed[Nq=%d,Ns=%d]" % (Nq, self.Ns), 12 * Nq + 12 * self.Ns + 4 * Nq * int(width)):
            _native.check(_native.lib().d3f_radius_query_pool_transposed(
                _p(self.ws), _p(q), Nq, _p(q_len), self.Ns, _p(self.s_len), int(q_len.numel()), self.radius, self.radius,
                int(width), _p(out), _p(mx), _p(lkey), int(max_group), _p(counts), _p(keys), _p(self.status.word),
                _stream()), "d3f_radius_query_pool_transposed")
        return out, mx, lkey, (counts, keys)

    def prefix_rows_from_transposed(self, queries, q_len, width, prefix_radius, transposed, nearest_bound=0.0):
        """The rows of ``query_prefix`` (this grid = the COARSE cloud, ``queries`` = the fine cloud) ranked from the lists a
        pooling search at ``prefix_radius`` left behind (``query_pool_transposed`` on the fine cloud's grid): the pairs are
        the same and so are the bits of their distances, so nothing is searched for a second time
        (d3f_upsample_rows_rank); the few fine points without a coarse point inside the radius -- and the padding rows --
        are searched as before (d3f_radius_query_prefix_missing)."""
        q = _f32(queries, "queries")
        q_len = _lens(q_len, q.device, "q_batches")
        counts, keys = transposed
        Nq = int(q.shape[0])
        if int(counts.numel()) != Nq:
            raise RuntimeError("transposed lists of %d points for %d queries" % (int(counts.numel()), Nq))
        L = _native.lib()
        out = torch.empty((Nq, int(width)), dtype=torch.int32, device=q.device)
        with _region("upsample_rows_rank[Nf=%d,Nc=%d]" % (Nq, self.Ns), 256 * Nq + 4 * Nq * int(width)):
            _native.check(L.d3f_upsample_rows_rank(_p(counts), _p(keys), Nq, self.Ns, int(width), _p(out), _stream()),
                          "d3f_upsample_rows_rank")
            _native.check(L.d3f_radius_query_prefix_missing(
                _p(self.ws), _p(q), Nq, _p(q_len), self.Ns, _p(self.s_len), int(q_len.numel()), self.radius, self.radius,
                float(prefix_radius), float(nearest_bound), int(width), _p(out), _p(counts), _p(self.status.word),
                _stream()), "d3f_radius_query_prefix_missing")
        return out

    def query(self, queries, q_len, width, want_counts=False, want_max=False, radius=None, wide=0, want_last_key=False,
              table=True, max_group=0, mx_out=None):
        """int32 [Nq, width] neighbor table (+ per-query uncapped counts, + device max count).

        ``radius`` (<= the grid's): search radius when it differs from the one the cell list was built for.
        ``wide`` > 0: additionally the whole ranked list of every query as an int32 [Nq, wide] table; ``want_last_key``:
        uint64 [Nq] rank key of the last entry each capped row keeps -- together the transposed form of a table for the
        gather-form KPConv grad-input (d3f_radius_query_ex).  ``table=False`` skips the capped table itself.
        ``max_group`` > 0: the max count comes per group of that many consecutive clouds (int32 [ceil(B/max_group)]).
        ``mx_out``: where the max count(s) go -- int32 counters the caller has cleared (``zero_buffers``)."""
        q = _f32(queries, "queries")
        if q.dim() != 2 or q.shape[1] != 3:
            raise RuntimeError("Wrong dimensions : query.shape is not (N, 3)")
        q_len = _lens(q_len, q.device, "q_batches")
        if q_len.numel() != self.s_len.numel():
            raise RuntimeError("Wrong number of batch elements: different for queries and supports ")
        Nq = int(q.shape[0])
        r = self.radius if radius is None else float(radius)
        if r > self.radius:
            raise RuntimeError("search radius %g exceeds the cell list's %g" % (r, self.radius))
        out = torch.empty((Nq, int(width)), dtype=torch.int32, device=q.device) if table else None
        counts = torch.empty(Nq, dtype=torch.int32, device=q.device) if want_counts else None
        n_mx = -(-int(q_len.numel()) // int(max_group)) if max_group else 1
        mx = None
        if want_max:
            mx = mx_out if mx_out is not None else torch.zeros(n_mx, dtype=torch.int32, device=q.device)
            if mx.numel() != n_mx or mx.dtype != torch.int32:
                raise RuntimeError("mx_out must hold %d int32 counters" % n_mx)
        wtab = torch.empty((Nq, int(wide)), dtype=torch.int32, device=q.device) if wide else None
        lkey = torch.empty(Nq, dtype=torch.int64, device=q.device) if want_last_key else None
        with _region("radius_query[Nq=%d,Ns=%d]" % (Nq, self.Ns), 12 * Nq + 12 * self.Ns + 4 * Nq * (int(width) + int(wide))):
            _native.check(_native.lib().d3f_radius_query_ex(_p(self.ws), _p(q), Nq, _p(q_len), self.Ns, _p(self.s_len),
                                                            int(q_len.numel()), self.radius, r, int(width), _p(out),
                                                            _p(counts), _p(mx), _p(wtab), int(wide), _p(lkey),
                                                            int(max_group), _p(self.status.word), _stream()),
                          "d3f_radius_query_ex")
        res = (out,) if table else ()
        for flag, t in ((want_counts, counts), (want_max, mx), (wide, wtab), (want_last_key, lkey)):
            if flag:
                res += (t,)
        return res if len(res) != 1 else res[0]


def copy_buffers(jobs, threshold=0.0):
    """``jobs`` = [(src, dst)] device-to-device copies of equal byte size, or (src float64, dst uint8, 'mask') for
    dst = src > threshold -- all in ONE launch per 24 jobs (d3f_copy_buffers).  The caller guarantees contiguous tensors."""
    import ctypes
    jobs = [j for j in jobs if j[0].numel()]
    for k in range(0, len(jobs), 24):
        part = jobs[k:k + 24]
        n = len(part)
        srcs = (ctypes.c_void_p * n)(*[j[0].data_ptr() for j in part])
        dsts = (ctypes.c_void_p * n)(*[j[1].data_ptr() for j in part])
        sizes = (ctypes.c_size_t * n)(*[j[0].numel() * j[0].element_size() for j in part])
        kinds = (ctypes.c_int * n)(*[1 if len(j) > 2 else 0 for j in part])
        _native.check(_native.lib().d3f_copy_buffers(srcs, dsts, sizes, kinds, n, float(threshold), _stream()),
                      "d3f_copy_buffers")


def zero_buffers(tensors):
    """Clear up to 8 device buffers (4-byte multiples) with ONE launch (d3f_zero_buffers)."""
    import ctypes
    ts = [t for t in tensors if t is not None and t.numel()]
    for k in range(0, len(ts), 8):
        part = ts[k:k + 8]
        ptrs = (ctypes.c_void_p * len(part))(*[t.data_ptr() for t in part])
        sizes = (ctypes.c_size_t * len(part))(*[t.numel() * t.element_size() for t in part])
        _native.check(_native.lib().d3f_zero_buffers(ptrs, sizes, len(part), _stream()), "d3f_zero_buffers")


# ---------------------------------------------------------------------------------------------------------------
# grid subsampling (cpp_wrappers/cpp_subsampling; datasets/dataloader.py:12-22)
# ---------------------------------------------------------------------------------------------------------------
def grid_subsample_raw(points, lens, sampleDl, max_p=0, order=ORDER_REFERENCE, status=None, out_cap=0, features=None,
                       labels=None):
    """Sync-free form: returns (out_points [capacity,3], out_len [B] int32, out_total [1] int32, status), followed by
    out_features [capacity,fdim] / out_labels [capacity,ldim] int32 when ``features`` / ``labels`` are given
    (reference grid_subsampling.cpp:89-102: member mean, majority vote).

    ``points`` may itself be a capacity buffer: only the first sum(lens) rows are read, so pyramid levels chain
    on the device without reading lengths back."""
    p = _f32(points, "points")
    if p.dim() != 2 or p.shape[1] != 3:
        raise RuntimeError("Wrong dimensions : points.shape is not (N, 3)")
    dev = p.device
    lens = _lens(lens, dev, "batches")
    status = status if status is not None else DeviceStatus(dev)
    N, B = int(p.shape[0]), int(lens.numel())
    f = c = None
    if features is not None:
        f = _f32(features, "features")
        if f.dim() != 2 or f.shape[0] != N:
            raise RuntimeError("Wrong dimensions : features.shape is not (N, d)")      # wrapper.cpp:172-215
    if labels is not None:
        c = labels
        if not (isinstance(c, torch.Tensor) and c.is_cuda and c.dtype == torch.int32):
            raise RuntimeError("classes must be an int32 device tensor")
        if c.dim() > 2 or c.shape[0] != N:
            raise RuntimeError("Wrong dimensions : classes.shape is not (N,) or (N, d)")  # wrapper.cpp:182-224
        c = c.reshape(N, -1).contiguous()
    L = _native.lib()
    nbytes = L.d3f_grid_subsample_ws_bytes(N, B)
    ws = _ws(nbytes, dev)
    cap = int(out_cap) if out_cap and out_cap > 0 else N
    out = torch.empty((cap, 3), dtype=torch.float32, device=dev)
    out_len = torch.empty(B, dtype=torch.int32, device=dev)
    total = torch.empty(1, dtype=torch.int32, device=dev)
    of = torch.empty((cap, f.shape[1]), dtype=torch.float32, device=dev) if f is not None else None
    oc = torch.empty((cap, c.shape[1]), dtype=torch.int32, device=dev) if c is not None else None
    with _region("grid_subsample[cap=%d]" % N, 24 * N):
        if f is None and c is None:
            _native.check(L.d3f_grid_subsample(_p(p), N, _p(lens), B, float(sampleDl), int(max_p), int(order), _p(out),
                                               cap, _p(out_len), _p(total), _p(ws), nbytes, _p(status.word), _stream()),
                          "d3f_grid_subsample")
        else:
            _native.check(L.d3f_grid_subsample_ex(
                _p(p), N, _p(lens), B, float(sampleDl), int(max_p), int(order), _p(f) if f is not None else None,
                int(f.shape[1]) if f is not None else 0, _p(c) if c is not None else None,
                int(c.shape[1]) if c is not None else 0, _p(out), cap, _p(out_len), _p(total),
                _p(of) if of is not None else None, _p(oc) if oc is not None else None, _p(ws), nbytes, _p(status.word),
                _stream()), "d3f_grid_subsample_ex")
    extra = tuple(t for t in (of, oc) if t is not None)
    return (out, out_len, total, status) + extra


# ---------------------------------------------------------------------------------------------------------------
# reverse neighbor tables (csrc/reverse_table.hip): CSR transpose of a table, for the gather-form KPConv grad-input
# ---------------------------------------------------------------------------------------------------------------
class ReverseTable(object):
    """The transpose of a neighbor table [Nq, H] over Ns supports, in one of two forms (int32 / int64 device tensors):
      CSR    ``ent[ptr[s] : ptr[s+1]]`` = the queries that list support s, ascending (build_reverse_table);
      search ``ent`` [Ns, width] = every query point within the radius of s, ranked, and ``last_key`` [Nq] = rank key of
             the last entry each table row kept: q lists s iff key(q, s) <= last_key[q] (RadiusGrid.query outputs)."""
    __slots__ = ("ptr", "ent", "last_key", "width", "Nq", "H", "Ns", "radius", "status", "rel")

    def __init__(self, ent, Nq, H, Ns, ptr=None, last_key=None, radius=0.0, status=None, rel=None):
        """``rel`` [Ns, width, 4] float32: the EXACT form (filter_reverse_table) -- row s = its true reverse neighbors
        compacted as {q - s, bits of q}; ``ent`` / ``ptr`` / ``last_key`` are then None."""
        if rel is not None:
            if ent is not None or ptr is not None or last_key is not None:
                raise ValueError("an exact-form reverse table carries only `rel`")
        elif (ptr is None) == (last_key is None):
            raise ValueError("a reverse table is either CSR (ptr) or search-form (last_key)")
        self.rel = rel
        self.ptr, self.ent, self.last_key = ptr, ent, last_key
        # radius > 0: `ent` comes from a search with a larger radius (an upsampling table); only its entries within
        # `radius` count.  status: DeviceStatus that receives D3F_ST_WIDE_OVERFLOW if such a row was cut short.
        self.radius, self.status = float(radius), status
        self.width = int(rel.shape[1]) if rel is not None else (int(ent.shape[1]) if ptr is None else 0)
        self.Nq, self.H, self.Ns = int(Nq), int(H), int(Ns)

    def matches(self, Nq, H, Ns):
        return (self.Nq, self.H, self.Ns) == (int(Nq), int(H), int(Ns))

    def tensors(self):
        return [t for t in (self.ptr, self.ent, self.last_key, self.rel) if t is not None]

    def edges(self):
        """Number of (query, support) pairs (one host read-back; measurement only)."""
        if self.rel is not None:
            return int((self.rel[:, :, 3].contiguous().view(torch.int32) < self.Nq).sum())
        if self.ptr is not None:
            return int(self.ptr[-1])
        return int((self.ent < self.Nq).sum())   # (search form: an upper bound -- the rows are supersets)


def filter_reverse_table(rev, q_pts, s_pts):
    """Search-form ReverseTable -> exact form (one launch, meant for the pyramid build): the membership test of every
    entry evaluated once, survivors compacted as {q - s, q}.  The search-form tensors are not kept."""
    if rev.rel is not None or rev.ptr is not None:
        return rev
    q, sp = _f32(q_pts, "q_pts"), _f32(s_pts, "s_pts")
    rel = torch.empty((rev.Ns, rev.width, 4), dtype=torch.float32, device=sp.device)
    with _region("reverse_table_filter[Ns=%d,W=%d]" % (rev.Ns, rev.width), 20 * rev.Ns * rev.width):
        _native.check(_native.lib().d3f_reverse_table_filter(
            _p(rev.ent), rev.width, _p(rev.last_key), _p(q), rev.Nq, _p(sp), rev.Ns, rev.radius, _p(rel),
            _p(rev.status.word) if rev.status is not None else None, _stream()), "d3f_reverse_table_filter")
    return ReverseTable(None, rev.Nq, rev.H, rev.Ns, rel=rel)


def attach_reverse_table(neighb_inds, rev):
    """Hand a table its transpose, so that operators given only the table (reference signatures) find it."""
    try:
        neighb_inds._d3f_rev = rev
    except AttributeError:  # pragma: no cover
        pass
    return rev


def build_reverse_table(neighb_inds, Ns):
    """CSR transpose of ``neighb_inds`` [Nq, H] (int32 device table, shadow entries >= Ns) over ``Ns`` supports, for
    tables that did not come with a search-form transpose.  Also attached to the table (``_d3f_rev``)."""
    idx = _i32(neighb_inds, "neighb_inds")
    Nq, H = int(idx.shape[0]), int(idx.shape[1])
    dev = idx.device
    ptr = torch.empty(int(Ns) + 1, dtype=torch.int32, device=dev)
    ent = torch.empty(max(Nq * H, 1), dtype=torch.int32, device=dev)
    L = _native.lib()
    nbytes = L.d3f_reverse_table_ws_bytes(Nq, H, int(Ns))
    ws = _ws(nbytes, dev)
    with _region("reverse_table[Nq=%d,H=%d,Ns=%d]" % (Nq, H, Ns), 12 * Nq * H + 8 * Ns):
        _native.check(L.d3f_reverse_table_build(_p(idx), Nq, H, int(Ns), _p(ptr), _p(ent), _p(ws), nbytes, _stream()),
                      "d3f_reverse_table_build")
    return attach_reverse_table(neighb_inds, ReverseTable(ent, Nq, H, Ns, ptr=ptr))


def reverse_table_of(neighb_inds, Nq, H, Ns, rev=None):
    """The reverse table to use for a table: the explicit one, else the one its builder attached; None otherwise."""
    if rev is None:
        rev = getattr(neighb_inds, "_d3f_rev", None)
    if rev is not None and not rev.matches(Nq, H, Ns):
        raise RuntimeError("reverse table of a [%d,%d] table over %d supports used with a [%d,%d] table over %d" % (
            rev.Nq, rev.H, rev.Ns, Nq, H, Ns))
    return rev


# KPConv layers whose grad-input runs as a gather over the reverse table: those with at least this many SUPPORT rows.
# Measured per layer of the S1 pair (profiles/r02b_timeline.txt vs r02a): 38k rows 177 -> 67 us, 8k rows x 64 ch
# 84 -> 36 us, the 8k -> 2k strided layer 43 -> 29 us.  Round 3 (exact-form tables, profiles/r03_dx_gather_threshold.txt):
# at the 2k-point level the two forms tie (4.096 vs 4.098 ms per step) -- the gather form is taken there too, it has no
# atomics and is bit-reproducible; below that (581 / 159 points x 256 / 512 channels) the scatter stays ahead (4.25 ms
# with the gather form at 581 points, 4.57 ms at 159: the chip is filled by splitting channels, which the gather form
# pays for with repeated aggregation).  Round 6 (3 stacked pairs: 114k / 24k / 6.2k / 1.7k / 0.5k rows; the wide layers
# now run the transposed aggregation + GEMM form, not the fused gather kernel): 1000 rows puts the 1.7k-row level on
# it as well -- 581.6 against 578.8 pairs/s at 2000, 575 / 574 at 300 / 100 -- and takes its float atomics away.
DX_GATHER_MIN_ROWS = 1000


# width of the search-form transpose of a conv table (the whole in-radius list of a point; S1: mean 41, max 68 at the
# 80 % limit of 42).  More than that sets D3F_ST_WIDE_OVERFLOW.  A pooling table's transpose is read off the
# upsampling table (coarse points within 2r of a fine point, nearest first: those within r -- mean 7, max 18 -- lead).
REV_WIDTH_CONV = 96
# the engine's upsampling rows ranked from the transpose the POOLING search leaves behind (RadiusGrid.query_pool_transposed
# / prefix_rows_from_transposed); False: the upsampling rows are searched for (rounds 4-6)
UPSAMPLES_FROM_POOL = True


def wants_reverse_table(Ns):
    """Whether a table over ``Ns`` supports is worth transposing (what the pyramid builders ask).  Under the deterministic
    mode every table is: the few-point levels' grad-input is a gather too."""
    if _DETERMINISTIC:
        return int(Ns) > 0
    return int(Ns) >= DX_GATHER_MIN_ROWS


# ---------------------------------------------------------------------------------------------------------------
# deterministic mode: a training step without float atomics
# ---------------------------------------------------------------------------------------------------------------
# Process-wide, off by default, and no environment variable.  An autograd node reads it when its FORWARD runs and keeps the
# choice on ``ctx``: its backward follows its forward, and a captured graph keeps the mode it was captured in.  Under it
# every float-atomic scatter of the step is replaced by an order-fixed form (the table in DESIGN section 5); an operator
# that has none raises instead of running.
_DETERMINISTIC = False
# how many launches of the scatter (atomic) forms a step has two forms for (pool backward, few-point KPConv grad-input,
# the loss node's sparse backward) / of the order-fixed replacements the dispatch made: tests assert on these that a mode
# did or did not reach a form
DISPATCH_COUNTS = {'scatter': 0, 'ordered': 0}


def set_deterministic(flag):
    """Switch the deterministic mode on or off for the process; returns the previous setting."""
    global _DETERMINISTIC
    old, _DETERMINISTIC = _DETERMINISTIC, bool(flag)
    return old


def is_deterministic():
    return _DETERMINISTIC


class deterministic_mode(object):
    """``with ops.deterministic_mode(True): ...`` -- the mode for the nodes whose forward runs inside (and for the pyramid
    built inside); restores the previous setting on exit.  The setting is the process's, not a thread's: scopes on different
    threads must not overlap (the training engines enter theirs one at a time)."""

    def __init__(self, flag=True):
        self.flag = bool(flag)

    def __enter__(self):
        self.old = set_deterministic(self.flag)
        return self

    def __exit__(self, exc_type, exc, tb):
        set_deterministic(self.old)
        return False


def _no_deterministic_form(op, why="its backward adds with float atomics"):
    """What torch does for an operator without a deterministic implementation."""
    raise RuntimeError("%s does not have a deterministic implementation (%s), but the deterministic mode is on "
                       "(ops.set_deterministic(True)).  Turn the mode off for this operation, or use an operator that has "
                       "an order-fixed form." % (op, why))


def _count(kind):
    DISPATCH_COUNTS[kind] += 1


def _csr_of(idx, Ns):
    """CSR transpose of a table for the gather-form pool backward: (ptr, ent), NOT attached to the table (a pooling table
    carries its KPConv transpose there).  Built where the node's forward runs: in a captured step the table's contents
    change from replay to replay, the build is part of the graph."""
    Nq, H = int(idx.shape[0]), int(idx.shape[1])
    if Nq * H == 0:     # no entry: every row of the transpose is empty
        return (torch.zeros(int(Ns) + 1, dtype=torch.int32, device=idx.device),
                torch.zeros(1, dtype=torch.int32, device=idx.device))
    ptr = torch.empty(int(Ns) + 1, dtype=torch.int32, device=idx.device)
    ent = torch.empty(max(Nq * H, 1), dtype=torch.int32, device=idx.device)
    L = _native.lib()
    nbytes = L.d3f_reverse_table_ws_bytes(Nq, H, int(Ns))
    ws = _ws(nbytes, idx.device)
    with _region("reverse_table[Nq=%d,H=%d,Ns=%d]" % (Nq, H, Ns), 12 * Nq * H + 8 * Ns):
        _native.check(L.d3f_reverse_table_build(_p(idx), Nq, H, int(Ns), _p(ptr), _p(ent), _p(ws), nbytes, _stream()),
                      "d3f_reverse_table_build")
    return ptr, ent



# ---------------------------------------------------------------------------------------------------------------
# KPConv (models/blocks.py:237-382)
# ---------------------------------------------------------------------------------------------------------------
def _adoptable(t, slot):
    """autograd adopts an incoming gradient as ``p.grad`` without a copy only when nobody else holds the tensor
    object: hand it a fresh view of the slot."""
    return t.view_as(t) if (slot is not None and t is slot) else t


def _grad_slot(param):
    """Where the weight gradient of ``param`` is to be written, when its owner (train.FlatParams) reserved a place for
    it in a flat gradient buffer; None otherwise (a fresh tensor is allocated)."""
    return getattr(param, "_d3f_grad_slot", None)


def _grad_target(slot, param):
    """The tensor a weight gradient is written to: the reserved slot, else a fresh tensor shaped like ``param``."""
    return slot if slot is not None else torch.empty_like(param)


def _bias_grad_buffer(want1, want2, Cout, device):
    """(gbuf, nb): one row [Cout] per bias that wants a gradient.  The node's forward launch clears the rows on the side
    (no fill launch in backward), and two bias parameters get separate rows (autograd would clone a shared one)."""
    nb = int(bool(want1)) + int(bool(want2))
    return (torch.empty((nb, Cout), dtype=torch.float32, device=device) if nb else None), nb


def _bias_grad_rows(ctx, want1, want2, Cout, device):
    """(g1, g2, first, second, pre): the bias-gradient rows of ``ctx.gbuf`` for the biases that want one, ``first`` /
    ``second`` = the same rows in the order the kernels fill them, ``pre`` = 1 when the forward cleared them."""
    g1 = g2 = None
    pre = 0
    if want1 or want2:
        gbuf, pre = ctx.gbuf, 1
        ctx.gbuf = None
        if gbuf is None:  # a second backward through the same node: fresh, not pre-cleared accumulators
            gbuf, pre = _bias_grad_buffer(want1, want2, Cout, device)[0], 0
        rows = list(gbuf.unbind(0))
        g1 = rows.pop(0) if want1 else None
        g2 = rows.pop(0) if want2 else None
    first, second = (g1, g2) if g1 is not None else (g2, None)
    return g1, g2, first, second, pre


# False: the backward pass recomputes the neighbor aggregation instead of reading it back (saves K*Cin*4 B/query)
SAVE_WEIGHTED_FEATURES = True
# below this many rows a weight gradient is a plain GEMM for the library; above, the reduction-parallel kernel
_SPLITK_MIN_ROWS = 4096
# below this many query points KPConv goes through library GEMMs (aggregate + wf@W forward; gW = (g/nn) W^T + scatter
# backward): measured better than the fused kernels up to the 2k-point level, not at 8k points
_GEMM_DX_MAX_ROWS = 4096
# ... and, whatever the row count, from this many input channels up (round 4): the contraction with W is then 60 % and
# more of a KPConv's arithmetic, and inside the fused kernels it runs on 16-row tiles against weights streamed from L2
# (0.15 - 0.2 of the f32 matrix rate, profiles/r04_step_timeline_stack4.txt); as aggregation kernel (registers -> HBM,
# csrc/kpconv_aggregate.hip) + tall GEMMs every contraction gets 128-row tiles.  Same split for the grad-input over
# the exact-form reverse table (transposed aggregation + GEMM with the permuted weights).
_GEMM_PATH_MIN_CIN = 32      # (round 6: 32 -- the level-0 layers' forward too: 266 -> 207 us alone, +1.2 % inside the 4 x 3 step)
_GEMM_DX_AGG_MIN_COUT = 64


_DW_LIBRARY_MIN_OUT = 1920 * 128
_DW_LIBRARY_MAX_ROWS = 16384


def _takes_gemm_path(Nq, Cin):
    return 0 < Nq < _GEMM_DX_MAX_ROWS or (Nq > 0 and Cin >= _GEMM_PATH_MIN_CIN)


def _csr_table(idx, Ns):
    """The CSR transpose of a table that came without a usable one, for the gather forms of the deterministic mode."""
    ptr, ent = _csr_of(idx, Ns)
    return ReverseTable(ent, int(idx.shape[0]), int(idx.shape[1]), Ns, ptr=ptr)


def _gather_table(rev, idx, Ns, K, Cin, Cout, always=False):
    """The reverse table the fused-path nodes' grad-input gathers over, None for the scatter form: the table's transpose
    from DX_GATHER_MIN_ROWS support rows up, for the channel counts the gather kernel covers.  ``always`` (a training call
    under the deterministic mode): at every row count, the CSR form built here when none came; other channel counts raise."""
    covered = _native.lib().d3f_kpconv_grad_input_gather_supported(Cin, Cout, K)
    if always:
        if not covered:
            _no_deterministic_form("KPConv grad-input for %d -> %d channels" % (Cin, Cout),
                                   "the gather form does not cover these channel counts")
        return rev if rev is not None else _csr_table(idx, Ns)
    return rev if (rev is not None and Ns >= DX_GATHER_MIN_ROWS and covered) else None


def _packed_supports(x, Ns, ready, packs, want_keep, need_clear):
    """(keep, gx_buf, clear): the packed supports a forward launch leaves for the backward pass, the scatter target it
    clears on the side (``need_clear``; the gather form writes every row: nothing to clear) and what the launch takes as
    its grad_x_clear argument.  The epilogue that produced x may have packed the supports already (``ready``, a
    PackedSupports): no packing launch then.  ``packs``: the launch works on packed supports at all; ``want_keep``: when
    the node allocates them itself."""
    keep = gx_buf = None
    use_ready = packs and ready is not None and (not need_clear or ready.gx_buf is not None)
    if use_ready:
        keep, gx_buf = ready.spack, (ready.gx_buf if need_clear else None)
    elif want_keep and packs:
        keep = torch.empty(16 * Ns, dtype=torch.uint8, device=x.device)
        if need_clear:
            gx_buf = torch.empty_like(x)
    return keep, gx_buf, SPACK_READY if use_ready else _p(gx_buf)


def _scatter_target(ctx, x):
    """(gx, pre): the buffer the node's forward cleared on the side (pre = 1); a second backward gets a fresh one."""
    gx, ctx.gx_buf = ctx.gx_buf, None
    return (gx, 1) if gx is not None else (torch.empty_like(x), 0)


def _kpconv_dx_gather(q_pts, s_pts, H, rev, kernel_points, weights, extent, nn, g, gx):
    """grad_x as a gather over the reverse table: aggregate g / nn around every support, then contract with W^T -- one
    launch instead of the gW GEMM + atomic scatter.  ``nn`` None: ``g`` is already divided."""
    Nq, Ns = int(q_pts.shape[0]), int(s_pts.shape[0])
    K, Cin, Cout = int(weights.shape[0]), int(weights.shape[1]), int(weights.shape[2])
    with _region("kpconv_dx_gather[Ns=%d,Cin=%d,Cout=%d]" % (Ns, Cin, Cout), kpconv_bwd_bytes(Nq, Ns, H, K, Cin, Cout)):
        _native.check(_native.lib().d3f_kpconv_grad_input_gather(
            _p(q_pts), Nq, _p(s_pts), Ns, _p(rev.ptr), _p(rev.ent), _p(rev.last_key), rev.width, rev.radius, _p(rev.rel),
            _p(kernel_points), K, _p(weights), Cin, Cout, extent, _p(nn), _p(g), _p(gx),
            _p(rev.status.word) if rev.status is not None else None, _stream()), "d3f_kpconv_grad_input_gather")


def _kpconv_dx_scatter(q_pts, s_pts, idx, x, kernel_points, weights, extent, gon, keep, pre, gx):
    """grad_x of the few-point layers: gW [Nq, K Cin] = (g / nn) [Nq, Cout] @ W^T (W viewed [K Cin, Cout]) over all
    queries is one library GEMM; the kernel only scatters it (float atomics)."""
    L = _native.lib()
    Nq, Ns, H = int(q_pts.shape[0]), int(s_pts.shape[0]), int(idx.shape[1])
    K, Cin, Cout = int(weights.shape[0]), int(weights.shape[1]), int(weights.shape[2])
    gwf = torch.mm(gon, weights.view(K * Cin, Cout).t())
    nbytes = L.d3f_kpconv_ws_bytes(Nq, Ns, H, K, Cin, 64)
    ws = _ws(nbytes, x.device)
    _count('scatter')
    with _region("kpconv_dx_scatter[Nq=%d,Cin=%d,H=%d]" % (Nq, Cin, H), 4 * Nq * K * Cin + 4 * Nq * H * (1 + Cin)):
        _native.check(L.d3f_kpconv_grad_input(_p(q_pts), Nq, _p(s_pts), Ns, _p(idx), H, _p(x), Cin, _p(kernel_points), K,
                                              extent, _p(gwf), _p(keep), pre, _p(gx), _p(ws), nbytes, _stream()),
                      "d3f_kpconv_grad_input")


class _KPConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q_pts, s_pts, idx, x, kernel_points, weights, extent, rev=None, ready=None):
        L = _native.lib()
        Nq, Ns, H = int(q_pts.shape[0]), int(s_pts.shape[0]), int(idx.shape[1])
        K, Cin, Cout = int(weights.shape[0]), int(weights.shape[1]), int(weights.shape[2])
        ctx.rev = rev = _gather_table(rev, idx, Ns, K, Cin, Cout)
        out = torch.empty((Nq, Cout), dtype=torch.float32, device=x.device)
        nn = torch.empty(Nq, dtype=torch.float32, device=x.device)
        nbytes = L.d3f_kpconv_ws_bytes(Nq, Ns, H, K, Cin, Cout)
        ws = _ws(nbytes, x.device)
        # training: keep the weighted features [Nq, K*Cin] for the backward pass (K*Cin*4 B per query of HBM) so the
        # weight gradient is one tall-skinny GEMM and the neighbor aggregation is not recomputed
        wf = None
        wf_row = L.d3f_kpconv_saves_wf(Cin, Cout, K, H)   # floats per query (the input-layer kernels pad K to 16 slots)
        if SAVE_WEIGHTED_FEATURES and ctx.needs_input_grad[5] and Nq > 0 and wf_row:
            wf = torch.empty((Nq, wf_row), dtype=torch.float32, device=x.device)
        # training: the packed supports are kept for the backward pass and its scatter target is cleared on the side
        packs = Nq > 0 and Ns > 0 and L.d3f_kpconv_packs_supports(Cin, Cout, K, H, Ns)
        keep, gx_buf, clear = _packed_supports(x, Ns, ready, packs, ctx.needs_input_grad[3] or ctx.needs_input_grad[5],
                                               ctx.needs_input_grad[3] and rev is None)
        with _region("kpconv_fwd[Nq=%d,Cin=%d,Cout=%d,H=%d]" % (Nq, Cin, Cout, H),
                     kpconv_fwd_bytes(Nq, Ns, H, K, Cin, Cout)):
            _native.check(L.d3f_kpconv_forward(_p(q_pts), Nq, _p(s_pts), Ns, _p(idx), H, _p(x), Cin,
                                               _p(kernel_points), K, _p(weights), Cout, float(extent), _p(out),
                                               _p(nn), _p(wf), _p(keep), clear, _p(ws), nbytes, _stream()),
                          "d3f_kpconv_forward")
        ctx.keep, ctx.gx_buf = keep, gx_buf
        ctx.gw_slot = _grad_slot(weights)
        ctx.has_wf = wf is not None
        ctx.save_for_backward(q_pts, s_pts, idx, x, kernel_points, weights, nn, *([wf] if wf is not None else []))
        ctx.extent = float(extent)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        q_pts, s_pts, idx, x, kernel_points, weights, nn = ctx.saved_tensors[:7]
        wf = ctx.saved_tensors[7] if ctx.has_wf else None
        L = _native.lib()
        Nq, Ns, H = int(q_pts.shape[0]), int(s_pts.shape[0]), int(idx.shape[1])
        K, Cin, Cout = int(weights.shape[0]), int(weights.shape[1]), int(weights.shape[2])
        need_x, need_w = ctx.needs_input_grad[3], ctx.needs_input_grad[5]
        keep, pre = ctx.keep, 0
        gx = None
        if need_x:
            gx, pre = _scatter_target(ctx, x)
        gw = _grad_target(ctx.gw_slot, weights) if need_w else None
        go = grad_out.contiguous().float() if (need_x or need_w) else None
        gw_native, gx_native = gw, gx
        # grad_W = wf^T (g / nn) over the saved weighted features: from _SPLITK_MIN_ROWS rows the reduction-parallel kernel
        # (tall-skinny upper levels; shapes it does not take stay with d3f_kpconv_backward), below an ordinary GEMM with a
        # short reduction -- a library call (few points, wide layers: bottom of the U-Net)
        wf_dw = need_w and wf is not None and wf.shape[1] == K * Cin
        big_dw = wf_dw and Nq >= _SPLITK_MIN_ROWS and L.d3f_linear_grad_weight_supported(Nq, Cout, K * Cin)
        gon = None

        def g_over_nn():
            # g / nn ONCE (one small elementwise launch), where its first consumer runs: inside the A^T B kernel the
            # division sat in every lane of every column block behind a dependent 4-byte load (round 4, bench per-launch
            # table: 23.9k x 480 x 32 in 63 us against 24 us without it), and the gather kernel divided once per edge
            nonlocal gon
            if gon is None:
                gon = go / nn.unsqueeze(1)
            return gon
        if need_x and ctx.rev is not None and Nq > 0:
            # (the gather divides by nn itself unless the A^T B kernel wants g / nn anyway)
            _kpconv_dx_gather(q_pts, s_pts, H, ctx.rev, kernel_points, weights, ctx.extent, None if big_dw else nn,
                              g_over_nn() if big_dw else go, gx)
            gx_native = None
        if big_dw or (wf_dw and Nq < _SPLITK_MIN_ROWS):
            # x := g / nn [Nq, Cout], grad_out := wf [Nq, K Cin]
            _weight_grad(g_over_nn(), wf, Nq, Cout, K * Cin, gw.view(K * Cin, Cout), big_dw, label="kpconv_dw_atb",
                         gemm_label="kpconv_dw_gemm[Nq=%d,Cin=%d,Cout=%d]" % (Nq, Cin, Cout))
            gw_native = None
        if gx_native is not None and 0 < Nq < _GEMM_DX_MAX_ROWS and L.d3f_kpconv_grad_input_supported(Cin, K, H, Ns):
            _kpconv_dx_scatter(q_pts, s_pts, idx, x, kernel_points, weights, ctx.extent, g_over_nn(), keep, pre, gx)
            gx_native = None
        if gx_native is not None or gw_native is not None:
            nbytes = L.d3f_kpconv_ws_bytes(Nq, Ns, H, K, Cin, Cout)
            ws = _ws(nbytes, x.device)
            with _region("kpconv_bwd[Nq=%d,Cin=%d,Cout=%d,H=%d]" % (Nq, Cin, Cout, H),
                         kpconv_bwd_bytes(Nq, Ns, H, K, Cin, Cout)):
                _native.check(L.d3f_kpconv_backward(_p(q_pts), Nq, _p(s_pts), Ns, _p(idx), H, _p(x), Cin,
                                                    _p(kernel_points), K, _p(weights), Cout, ctx.extent, _p(nn),
                                                    _p(go), _p(wf), _p(keep), pre, _p(gx_native), _p(gw_native),
                                                    _p(ws), nbytes, _stream()),
                              "d3f_kpconv_backward")
        return None, None, None, gx, None, _adoptable(gw, ctx.gw_slot), None, None, None


# The transposed-aggregation grad-input contracts with the permuted weights W'[k, o, c] = W[k, c, o].  One
# permute + copy launch per layer (9 per 3-pair stack, 63 us) became ONE launch per backward pass: the forward of every
# such layer queues its weights, the first grad-input that needs a permuted matrix launches d3f_permute_kpconv_weights
# for the whole queue.  The queue is process-wide, not per thread: a forward on the calling thread is followed by its
# backward on autograd's device thread (or, for a lane, on the lane's capture thread); steps are recorded / run one at a
# time, the lock only keeps the two dictionaries consistent.  A shape the launch does not serve is permuted on its own.
_WPERM = {'queue': {}, 'ready': {}}
_WPERM_LOCK = threading.Lock()


def _wperm_state():
    return _WPERM


def _queue_weight_permute(weights):
    st = _wperm_state()
    key = weights.data_ptr()
    with _WPERM_LOCK:
        st['ready'].pop(key, None)          # (a new forward: whatever an earlier backward left behind is stale)
        if len(st['queue']) >= 64:          # forwards without a backward: start over
            st['queue'].clear()
        st['queue'][key] = weights


def _permuted_weights(weights):
    """W' [K * Cout, Cin] of ``weights`` [K, Cin, Cout]."""
    K, Cin, Cout = int(weights.shape[0]), int(weights.shape[1]), int(weights.shape[2])
    st = _wperm_state()
    key = weights.data_ptr()
    with _WPERM_LOCK:
        wp = st['ready'].pop(key, None)
        jobs = []
        if wp is None and key in st['queue']:
            jobs = [w for w in st['queue'].values()
                    if w.shape[1] % 32 == 0 and w.shape[2] % 32 == 0 and w.is_contiguous() and w.device == weights.device]
            st['queue'].clear()
            st['ready'].clear()
    if jobs:
        for j0 in range(0, len(jobs), 16):
            part = jobs[j0:j0 + 16]
            outs = [torch.empty((w.shape[0] * w.shape[2], w.shape[1]), dtype=torch.float32, device=w.device) for w in part]
            n = len(part)
            srcs = (ctypes.c_void_p * n)(*[w.data_ptr() for w in part])
            dsts = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
            ks = (ctypes.c_int * n)(*[int(w.shape[0]) for w in part])
            cis = (ctypes.c_int * n)(*[int(w.shape[1]) for w in part])
            cos = (ctypes.c_int * n)(*[int(w.shape[2]) for w in part])
            _native.check(_native.lib().d3f_permute_kpconv_weights(srcs, dsts, ks, cis, cos, n, _stream()),
                          "d3f_permute_kpconv_weights")
            with _WPERM_LOCK:
                for w, o in zip(part, outs):
                    st['ready'][w.data_ptr()] = o
        with _WPERM_LOCK:
            wp = st['ready'].pop(key, None)
    if wp is None:
        wp = weights.permute(0, 2, 1).contiguous().view(K * Cout, Cin)
    return wp


class _KPConvGemmBiasActFn(torch.autograd.Function):
    """act(KPConv(x) + bias) for the few-point / wide layers (bottom of the U-Net), as
        aggregation kernel -> wf [Nq, K*Cin], nn      library GEMM  raw = wf @ W       epilogue  act(raw/nn + bias)
    and backward   epilogue backward -> g/nn, bias gradient      GEMMs  grad_W = wf^T (g/nn),  gW = (g/nn) W^T
                   scatter kernel -> grad_x.
    The fused forward kernel would run its contraction on 10..40 workgroups there (58-71 us); this is ~40 us and the
    backward saves the separate g/nn pass."""

    @staticmethod
    def forward(ctx, q_pts, s_pts, idx, x, kernel_points, weights, bias, extent, slope, rev=None, ready=None):
        L = _native.lib()
        Nq, Ns, H = int(q_pts.shape[0]), int(s_pts.shape[0]), int(idx.shape[1])
        K, Cin, Cout = int(weights.shape[0]), int(weights.shape[1]), int(weights.shape[2])
        det = ctx.det = _DETERMINISTIC
        # (under the mode: the gather form at EVERY row count)
        ctx.rev = rev = _gather_table(rev, idx, Ns, K, Cin, Cout, always=det and ctx.needs_input_grad[3])
        dev = x.device
        wf = torch.empty((Nq, K * Cin), dtype=torch.float32, device=dev)
        nn = torch.empty(Nq, dtype=torch.float32, device=dev)
        nbytes = L.d3f_kpconv_ws_bytes(Nq, Ns, H, K, Cin, 64)
        ws = _ws(nbytes, dev)
        # (the aggregation kernel always works on packed supports; they are kept only for the scatter kernel)
        need_clear = ctx.needs_input_grad[3] and rev is None
        keep, gx_buf, clear = _packed_supports(x, Ns, ready, True, need_clear, need_clear)
        with _region("kpconv_aggregate[Nq=%d,Cin=%d,H=%d]" % (Nq, Cin, H), 4 * Nq * H * (4 + Cin) + 4 * Nq * K * Cin):
            _native.check(L.d3f_kpconv_aggregate(_p(q_pts), Nq, _p(s_pts), Ns, _p(idx), H, _p(x), Cin,
                                                 _p(kernel_points), K, float(extent), _p(wf), _p(nn), _p(keep), clear,
                                                 _p(ws), nbytes, _stream()), "d3f_kpconv_aggregate")
        ctx.keep, ctx.gx_buf = keep, gx_buf
        want_b = bias is not None and ctx.needs_input_grad[6]
        gbuf, _ = _bias_grad_buffer(want_b, False, Cout, dev)
        if _own_gemm(wf, weights, Nq, K * Cin, Cout, bias):
            # contraction + / nn + bias + LeakyReLU in one launch (csrc/gemm_epilogue.hip)
            out = gemm_epilogue(wf, weights, GEMM_NN, Nq, K * Cin, Cout, row_div=nn, bias1=bias, slope=slope,
                                zero_init=gbuf if want_b else None)
        else:
            raw = torch.mm(wf, weights.view(K * Cin, Cout))
            out = torch.empty_like(raw)
            _native.check(L.d3f_bias_act_forward(_p(raw), _p(bias), None, None, float(slope), Nq, Cout, _p(out), _p(gbuf),
                                                 Cout if want_b else 0, _p(nn), None, 0, 0, _stream()),
                          "d3f_bias_act_forward")
        ctx.save_for_backward(q_pts, s_pts, idx, x, kernel_points, weights, nn, wf, out)
        ctx.gbuf, ctx.extent, ctx.slope, ctx.want_b = gbuf, float(extent), float(slope), want_b
        ctx.gw_slot = _grad_slot(weights)
        if ctx.needs_input_grad[3] and rev is not None and rev.rel is not None and \
                Cout >= _GEMM_DX_AGG_MIN_COUT and L.d3f_kpconv_aggregate_transposed_supported(Cout, K):
            _queue_weight_permute(weights)      # (its grad-input contracts with W': one launch for all such layers)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        q_pts, s_pts, idx, x, kernel_points, weights, nn, wf, out = ctx.saved_tensors
        L = _native.lib()
        Nq, Ns, H = int(q_pts.shape[0]), int(s_pts.shape[0]), int(idx.shape[1])
        K, Cin, Cout = int(weights.shape[0]), int(weights.shape[1]), int(weights.shape[2])
        go = grad_out.contiguous()
        gb, _, _, _, pre = _bias_grad_rows(ctx, ctx.want_b, False, Cout, go.device)
        gon = torch.empty_like(go)  # masked gradient / nn
        # many rows: the reduction over the points is what has to be spread over the chip (csrc/linear.hip); a large
        # output over a few thousand rows (1920 x 128 and up) is an ordinary GEMM again: 36 against 58 us at 6159 rows
        # (profiles/r04_dw_library_vs_atb.txt)
        atb = (ctx.needs_input_grad[5] and Nq >= _SPLITK_MIN_ROWS
               and bool(L.d3f_linear_grad_weight_supported(Nq, Cout, K * Cin))
               and not (K * Cin * Cout >= _DW_LIBRARY_MIN_OUT and Nq <= _DW_LIBRARY_MAX_ROWS))
        bias_part, bias_blocks = _epilogue_backward(go, out, ctx.slope, Nq, Cout, gon, gb, None, pre, nn, atb, ctx.det)
        gx = gw = None
        if ctx.needs_input_grad[5]:
            gw = _grad_target(ctx.gw_slot, weights)
            # x := g / nn [Nq, Cout], grad_out := wf [Nq, K Cin]: grad_W [K Cin, Cout] = wf^T (g / nn)
            _weight_grad(gon, wf, Nq, Cout, K * Cin, gw.view(K * Cin, Cout), atb, bias_part, bias_blocks, gb, None,
                         label="kpconv_dw_atb")
        rev = ctx.rev
        if ctx.needs_input_grad[3] and rev is not None and rev.rel is not None and Cout >= _GEMM_DX_AGG_MIN_COUT \
                and L.d3f_kpconv_aggregate_transposed_supported(Cout, K):
            # transposed aggregation (registers -> HBM) + one tall GEMM with the permuted weights W'[k, o, c] = W[k, c, o]:
            # every row of grad_x written once, no atomics (gon is already / nn)
            agg = torch.empty((Ns, K * Cout), dtype=torch.float32, device=x.device)
            with _region("kpconv_agg_transposed[Ns=%d,Cout=%d]" % (Ns, Cout), 4 * Ns * K * Cout + 16 * Ns * rev.width):
                _native.check(L.d3f_kpconv_aggregate_transposed(_p(rev.rel), rev.width, Ns, Nq, _p(kernel_points), K,
                                                                ctx.extent, None, _p(gon), Cout, _p(agg), _stream()),
                              "d3f_kpconv_aggregate_transposed")
            gx = torch.mm(agg, _permuted_weights(weights))
        elif ctx.needs_input_grad[3] and rev is not None:
            gx = torch.empty_like(x)
            _kpconv_dx_gather(q_pts, s_pts, H, rev, kernel_points, weights, ctx.extent, None, gon, gx)
        elif ctx.needs_input_grad[3]:
            gx, pre = _scatter_target(ctx, x)
            _kpconv_dx_scatter(q_pts, s_pts, idx, x, kernel_points, weights, ctx.extent, gon, ctx.keep, pre, gx)
        return None, None, None, gx, None, _adoptable(gw, ctx.gw_slot), gb, None, None, None, None


def _ready_supports(x, s_pts):
    """The PackedSupports the producer of ``x`` left on it, if they belong to exactly this (s_pts, x)."""
    ready = getattr(x, '_d3f_spack', None)
    return ready if (ready is not None and ready.fits(s_pts, x)) else None


def _kpconv_operands(q_pts, s_pts, neighb_inds, x, kernel_points, weights, offsets=None):
    """(q_pts, s_pts, idx, x, kp, w) as the kernels take them (contiguous float32 / int32 device tensors), their shapes
    checked against each other -- and ``offsets`` [Nq, K, 3] of a deformable KPConv against them."""
    q_pts, s_pts, x = _f32(q_pts, "q_pts"), _f32(s_pts, "s_pts"), _f32(x, "x")
    idx = _i32(neighb_inds, "neighb_inds")
    kp, w = _f32(kernel_points, "kernel_points"), _f32(weights, "weights")
    ok = x.shape[0] == s_pts.shape[0] and x.shape[1] == w.shape[1] and idx.shape[0] == q_pts.shape[0]
    if offsets is not None:
        ok = ok and tuple(offsets.shape) == (q_pts.shape[0], w.shape[0], 3)
    if not ok:
        text = "KPConv: inconsistent shapes q%s s%s idx%s x%s W%s" % tuple(
            tuple(t.shape) for t in (q_pts, s_pts, idx, x, w))
        raise RuntimeError(text if offsets is None else "deformable %s offsets%s" % (text, tuple(offsets.shape)))
    return q_pts, s_pts, idx, x, kp, w


def kpconv_bias_act(q_pts, s_pts, neighb_inds, x, kernel_points, weights, extent, bias, slope=0.1, influence='linear',
                    aggregation='sum', rev=None):
    """LeakyReLU(KPConv(x) + bias): KPConv + the bias/activation that follows it in every block
    (reference blocks.py:594-598, 668-676)."""
    if kpconv_mode(influence, aggregation) != 0:
        return bias_act(kpconv(q_pts, s_pts, neighb_inds, x, kernel_points, weights, extent, influence, aggregation),
                        bias, slope=slope)
    q_pts, s_pts, x = _f32(q_pts, "q_pts"), _f32(s_pts, "s_pts"), _f32(x, "x")
    Nq, H = int(q_pts.shape[0]), int(neighb_inds.shape[1])
    K, Cin = int(weights.shape[0]), int(weights.shape[1])
    gemm_path = _takes_gemm_path(Nq, Cin)
    if _DETERMINISTIC and torch.is_grad_enabled() and Nq > 0:
        # deterministic mode: the aggregation + GEMM node at every row count (its grad-input is the gather form); the
        # channel counts the gather kernel does not cover go through the general-path node's gather form (ops.kpconv below)
        gemm_path = not x.requires_grad or bool(
            _native.lib().d3f_kpconv_grad_input_gather_supported(Cin, int(weights.shape[2]), K))
    elif _DETERMINISTIC and not torch.is_grad_enabled() and x.requires_grad:
        x = x.detach()      # (no graph is recorded: the node must not ask for a grad-input form it will never run)
    if gemm_path and s_pts.shape[0] > 0 and \
            _native.lib().d3f_kpconv_grad_input_supported(Cin, K, H, int(s_pts.shape[0])):
        q_pts, s_pts, idx, x, kp, w = _kpconv_operands(q_pts, s_pts, neighb_inds, x, kernel_points, weights)
        b = _opt_f32(bias, "bias")
        rev = reverse_table_of(neighb_inds, Nq, H, int(s_pts.shape[0]), rev) if x.requires_grad else None
        return _KPConvGemmBiasActFn.apply(q_pts, s_pts, idx, x, kp, w, b, float(extent), float(slope), rev,
                                          _ready_supports(x, s_pts))
    return bias_act(kpconv(q_pts, s_pts, neighb_inds, x, kernel_points, weights, extent, rev=rev), bias, slope=slope)


KP_INFLUENCES = {'linear': 0, 'constant': 1, 'gaussian': 2}
KP_AGGREGATIONS = {'sum': 0, 'closest': 4}


def kpconv_mode(influence='linear', aggregation='sum'):
    """Mode word of the C ABI; the reference's error messages for unknown names (blocks.py:344,352)."""
    if influence not in KP_INFLUENCES:
        raise ValueError('Unknown influence function type (config.KP_influence)')
    if aggregation not in KP_AGGREGATIONS:
        raise ValueError("Unknown convolution mode. Should be 'closest' or 'sum'")
    return KP_INFLUENCES[influence] | KP_AGGREGATIONS[aggregation]


class _KPConvGeneralFn(torch.autograd.Function):
    """KPConv of ANY channel count and influence / aggregation mode (blocks.py:327-352) on the general path: the
    mode-aware aggregation kernel (a gather, one wave per query) -> wf, nn; the contraction with the kernel weights by
    library GEMMs; grad_W = wf^T (g / nn) on the weight-gradient routes of the other nodes; grad_x from
    gW = (g / nn) W^T, as a float-atomic scatter over the table (``rev`` None: the non-default modes) or as a GATHER over
    its transpose (``rev``: the ReverseTable in CSR or exact form; every training call under the deterministic mode, in
    place of the scatters of this node and of _KPConvFn)."""

    @staticmethod
    def forward(ctx, q_pts, s_pts, idx, x, kp, weights, extent, mode, rev):
        Nq, Ns, H = int(q_pts.shape[0]), int(s_pts.shape[0]), int(idx.shape[1])
        K, Cin, Cout = (int(v) for v in weights.shape)
        wf = torch.empty((Nq, K * Cin), dtype=torch.float32, device=x.device)
        nn_ = torch.empty((Nq,), dtype=torch.float32, device=x.device)
        with _region("kpconv_%s_fwd[Nq=%d,Cin=%d,H=%d,mode=%d]" % ("modes" if rev is None else "ordered", Nq, Cin, H, mode),
                     4 * Nq * H * (4 + Cin)):
            _native.check(_native.lib().d3f_kpconv_aggregate_modes(
                _p(q_pts), Nq, _p(s_pts), Ns, _p(idx), H, _p(x), Cin, _p(kp), K, extent, mode, _p(wf), _p(nn_),
                _stream()), "d3f_kpconv_aggregate_modes")
        out = torch.mm(wf, weights.reshape(K * Cin, Cout)) / nn_[:, None]
        ctx.save_for_backward(q_pts, s_pts, idx, kp, weights, wf, nn_)
        ctx.extent, ctx.mode, ctx.rev, ctx.gw_slot = extent, mode, rev, _grad_slot(weights)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        q_pts, s_pts, idx, kp, weights, wf, nn_ = ctx.saved_tensors
        L = _native.lib()
        Nq, Ns, H = int(q_pts.shape[0]), int(s_pts.shape[0]), int(idx.shape[1])
        K, Cin, Cout = (int(v) for v in weights.shape)
        g = grad_out.contiguous() / nn_[:, None]
        gx = gw = None
        if ctx.needs_input_grad[5]:
            gw = _grad_target(ctx.gw_slot, weights)
            atb = Nq >= _SPLITK_MIN_ROWS and bool(L.d3f_linear_grad_weight_supported(Nq, Cout, K * Cin))
            _weight_grad(g, wf, Nq, Cout, K * Cin, gw.view(K * Cin, Cout), atb, label="kpconv_dw_atb",
                         gemm_label="kpconv_dw_gemm[Nq=%d,Cin=%d,Cout=%d]" % (Nq, Cin, Cout))
        if ctx.needs_input_grad[3]:
            rev = ctx.rev
            gwf = torch.mm(g, weights.reshape(K * Cin, Cout).t()).contiguous()
            gx = torch.empty((Ns, Cin), dtype=torch.float32, device=g.device)
            if rev is None:
                with _region("kpconv_modes_dx[Nq=%d,Cin=%d,H=%d,mode=%d]" % (Nq, Cin, H, ctx.mode), 8 * Nq * H * Cin):
                    _native.check(L.d3f_kpconv_grad_input_modes(_p(q_pts), Nq, _p(s_pts), Ns, _p(idx), H, Cin, _p(kp), K,
                                                                ctx.extent, ctx.mode, _p(gwf), _p(gx), _stream()),
                                  "d3f_kpconv_grad_input_modes")
            else:
                _count('ordered')
                with _region("kpconv_ordered_dx[Ns=%d,Cin=%d,mode=%d]" % (Ns, Cin, ctx.mode), 8 * Nq * K * Cin):
                    _native.check(L.d3f_kpconv_grad_input_modes_gather(
                        _p(q_pts), Nq, _p(s_pts), Ns, _p(rev.ptr), _p(rev.ent) if rev.ptr is not None else None,
                        _p(rev.rel), rev.width, Cin, _p(kp), K, ctx.extent, ctx.mode, _p(gwf), _p(gx), _stream()),
                        "d3f_kpconv_grad_input_modes_gather")
        return None, None, None, gx, None, _adoptable(gw, ctx.gw_slot), None, None, None


def kpconv(q_pts, s_pts, neighb_inds, x, kernel_points, weights, extent, influence='linear', aggregation='sum',
           rev=None):
    """Rigid KPConv.  Shapes as KPConv.forward (blocks.py:237); 'linear' / 'sum' (the D3Feat configuration) runs on
    the fused kernels, the other modes of blocks.py:327-352 on the general path.  ``rev``: the table's ReverseTable
    (build_reverse_table; found on the table itself when its builder attached it): grad_x is then a gather."""
    mode = kpconv_mode(influence, aggregation)
    q_pts, s_pts, idx, x, kp, w = _kpconv_operands(q_pts, s_pts, neighb_inds, x, kernel_points, weights)
    Nq, Ns, H = int(q_pts.shape[0]), int(s_pts.shape[0]), int(idx.shape[1])
    # a training call under the deterministic mode: every mode and channel count through the general node's gather form
    # (_KPConvFn's kernels combine channel chunks, waves and weight-gradient partials with float atomics, and both nodes'
    # other grad-input forms scatter)
    ordered = _DETERMINISTIC and torch.is_grad_enabled() and (x.requires_grad or w.requires_grad)
    if (ordered or mode != 0) and (Nq == 0 or Ns == 0):
        return x.new_zeros((Nq, w.shape[2])) + 0.0 * (x.sum() + w.sum())
    # ... but the input layer (features without gradient) on the input-layer kernels: their forward has no atomic and,
    # where they save the weighted features (16-slot rows: Cout % 16 == 0), grad_W is the A^T B kernel over them
    # (asked at K = 1, where the 16-slot rows cannot be mistaken for K * Cin)
    if ordered and mode == 0 and not x.requires_grad and SAVE_WEIGHTED_FEATURES and \
            _native.lib().d3f_kpconv_saves_wf(int(w.shape[1]), int(w.shape[2]), 1, H) == 16 * int(w.shape[1]):
        return _KPConvFn.apply(q_pts, s_pts, idx, x, kp, w, float(extent), None, None)
    if x.requires_grad and (ordered or mode == 0):
        rev = reverse_table_of(neighb_inds, Nq, H, Ns, rev)
    else:
        rev = None
    if not ordered and mode == 0:
        return _KPConvFn.apply(q_pts, s_pts, idx, x, kp, w, float(extent), rev, _ready_supports(x, s_pts))
    if ordered and x.requires_grad and (rev is None or (rev.ptr is None and rev.rel is None)):
        rev = _csr_table(idx, Ns)       # (no transpose, or a search-form one: not one of the gather kernel's two forms)
    return _KPConvGeneralFn.apply(q_pts, s_pts, idx, x, kp, w, float(extent), mode, rev)


class _KPConvDeformAggFn(torch.autograd.Function):
    """wf, nn, min-distance bookkeeping of a deformable KPConv (csrc/kpconv_deform.hip); differentiable w.r.t. the
    features and the deformed kernel points."""

    @staticmethod
    def forward(ctx, q_pts, s_pts, idx, x, kp_def, extent, extent_sq, mode):
        L = _native.lib()
        Nq, Ns, H = int(q_pts.shape[0]), int(s_pts.shape[0]), int(idx.shape[1])
        K, Cin = int(kp_def.shape[1]), int(x.shape[1])
        wf = torch.empty((Nq, K, Cin), dtype=torch.float32, device=x.device)
        nn_ = torch.empty((Nq,), dtype=torch.float32, device=x.device)
        min_idx = torch.empty((Nq, K), dtype=torch.int32, device=x.device)
        with _region("kpconv_deform_fwd[Nq=%d,Cin=%d,H=%d]" % (Nq, Cin, H), 4 * Nq * H * (4 + Cin)):
            _native.check(L.d3f_kpconv_deform_aggregate(_p(q_pts), Nq, _p(s_pts), Ns, _p(idx), H, _p(x), Cin,
                                                        _p(kp_def), K, extent, extent_sq, mode, _p(wf), _p(nn_), None,
                                                        _p(min_idx), _stream()), "d3f_kpconv_deform_aggregate")
        ctx.save_for_backward(q_pts, s_pts, idx, x, kp_def)
        ctx.extent, ctx.extent_sq, ctx.mode = extent, extent_sq, mode
        ctx.mark_non_differentiable(nn_, min_idx)
        ctx.set_materialize_grads(False)
        return wf, nn_, min_idx

    @staticmethod
    def backward(ctx, gwf, _gnn, _gidx):
        if gwf is None:
            return (None,) * 8
        q_pts, s_pts, idx, x, kp_def = ctx.saved_tensors
        L = _native.lib()
        Nq, Ns, H = int(q_pts.shape[0]), int(s_pts.shape[0]), int(idx.shape[1])
        K, Cin = int(kp_def.shape[1]), int(x.shape[1])
        gx = torch.empty((Ns, Cin), dtype=torch.float32, device=x.device) if ctx.needs_input_grad[3] else None
        gkp = torch.empty((Nq, K, 3), dtype=torch.float32, device=x.device) if ctx.needs_input_grad[4] else None
        if gx is None and gkp is None:
            return (None,) * 8
        gwf = gwf.contiguous()
        with _region("kpconv_deform_bwd[Nq=%d,Cin=%d,H=%d]" % (Nq, Cin, H), 12 * Nq * H * Cin):
            _native.check(L.d3f_kpconv_deform_grad(_p(q_pts), Nq, _p(s_pts), Ns, _p(idx), H, _p(x), Cin, _p(kp_def), K,
                                                   ctx.extent, ctx.extent_sq, ctx.mode, _p(gwf), _p(gx), _p(gkp),
                                                   _stream()), "d3f_kpconv_deform_grad")
        return None, None, None, gx, gkp, None, None, None


def kpconv_deformable(q_pts, s_pts, neighb_inds, x, kernel_points, weights, extent, offsets, modulations=None,
                      influence='linear', aggregation='sum'):
    """Deformable (and modulated) KPConv, the deformable=True branch of KPConv.forward (blocks.py:243-387).

    ``offsets`` [Nq,K,3] are the SCALED kernel-point shifts (unscaled offsets * KP_extent, :256), ``modulations``
    [Nq,K] the 2*sigmoid factors (:250) or None.  Returns (out [Nq,Cout], min_d2 [Nq,K], deformed_KP [Nq,K,3]) --
    the last two are what the reference keeps on the module for its fitting / repulsive regulariser
    (architectures.py:22-55); min_d2 carries its gradient to the offsets."""
    mode = kpconv_mode(influence, aggregation)
    q_pts, s_pts, idx, x, kp, w = _kpconv_operands(q_pts, s_pts, neighb_inds, x, kernel_points, weights, offsets)
    K, Cin, Cout = (int(v) for v in w.shape)
    Nq = int(q_pts.shape[0])
    if _DETERMINISTIC and torch.is_grad_enabled() and x.requires_grad:
        _no_deterministic_form("kpconv_deformable")
    deformed = offsets + kp                                              # blocks.py:287
    extent = float(extent)
    extent_sq = float(np.float32(extent ** 2))                           # the float32 scalar of `sq_distances < ext**2`
    wf, nn_, min_idx = _KPConvDeformAggFn.apply(q_pts, s_pts, idx, x, deformed.contiguous(), extent, extent_sq, mode)
    # min over the neighbors of d2 (blocks.py:301), re-evaluated at the arg-min support so that autograd carries its
    # gradient to the offsets (the selection itself has none); the shadow support sits at 1e6 like the reference's
    s_pad = torch.cat((s_pts, torch.zeros_like(s_pts[:1, :]) + 1e6), 0)
    nearest = s_pad[min_idx.long()] - q_pts.unsqueeze(1)                 # [Nq,K,3]
    min_d2 = torch.sum((nearest - deformed) ** 2, dim=2)
    if modulations is not None:
        wf = wf * modulations.unsqueeze(2)                               # :365-366
    out = torch.mm(wf.reshape(Nq, K * Cin), w.reshape(K * Cin, Cout)) / nn_[:, None]
    return out, min_d2, deformed


# ---------------------------------------------------------------------------------------------------------------
class GradHolder(object):
    __slots__ = ("tensor", "closed")

    def __init__(self):
        self.tensor, self.closed = None, False

    def deposit(self, g):
        """True when `g` was taken (the caller then returns None as its gradient)."""
        if self.closed or self.tensor is not None or g is None:
            return False
        self.tensor = g
        return True

    def collect(self):
        self.closed = True
        g, self.tensor = self.tensor, None
        return g


class _GradTapFn(torch.autograd.Function):
    """Identity whose backward deposits the gradient (the identity shortcut of a bottleneck block)."""

    @staticmethod
    def forward(ctx, x, holder):
        ctx.holder = holder
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return (None if ctx.holder.deposit(g) else g), None


def grad_tap(x, holder):
    return _GradTapFn.apply(x, holder) if holder is not None else x


def _add_deposited(holder, go, weight):
    """grad_x = go @ weight (+ the sibling branch's deposited gradient, accumulated by the GEMM itself)."""
    c = holder.collect() if holder is not None else None
    if c is None:
        return torch.mm(go, weight)
    if c.is_contiguous() and c.dtype == go.dtype and c.shape == (go.shape[0], weight.shape[1]):
        if _WG_GROUP is not None:
            # the deposited buffer may be a queued operand of a weight gradient that has not run yet (the masked gradient
            # of the block's last unary layer IS the shortcut's gradient): accumulate out of place -- on the row-streaming
            # kernel where it serves the shape (it reads `add` and writes a separate output anyway: no extra traffic; the
            # library's out-of-place addmm first copies c, 58 MB at level 0)
            N, Cout, Cin = int(go.shape[0]), int(go.shape[1]), int(weight.shape[1])
            L = _native.lib()
            if go.is_contiguous() and weight.is_contiguous() and L.d3f_linear_fused_supported(N, Cin, Cout):
                gx = torch.empty_like(c)
                _native.check(L.d3f_linear_grad_input(_p(go), _p(weight), N, Cin, Cout, _p(c), _p(gx), _stream()),
                              "d3f_linear_grad_input")
                return gx
            return torch.addmm(c, go, weight)
        return c.addmm_(go, weight)      # beta = 1, in place: the deposited buffer has no other reader left
    return torch.mm(go, weight).add_(c)


# ---------------------------------------------------------------------------------------------------------------
# Own f32-MFMA GEMM with the block's epilogue fused (csrc/gemm_epilogue.hip): the contractions of the wide / few-row
# layers -- KPConv's wf @ W (models/blocks.py:362-374) with / nn + bias + LeakyReLU, nn.Linear of the unary blocks
# (:481-541) with bias + residual + LeakyReLU, and their grad-input products
# ---------------------------------------------------------------------------------------------------------------
GEMM_NT, GEMM_NN = 0, 1


def _al16(*ts):
    return all(t is None or t.data_ptr() % 16 == 0 for t in ts)


def gemm_epilogue_ok(x, w, mode, R, K, N, kblock=0, ldx=None, ldw=None, *others):
    """True when d3f_gemm_epilogue serves this product (shape, alignment, leading dimensions)."""
    if R < 1:
        return False
    ldx = K if ldx is None else ldx
    ldw = (K if mode == GEMM_NT else N) if ldw is None else ldw
    if (ldx | ldw) & 3 or not _al16(x, w, *others):
        return False
    return bool(_native.lib().d3f_gemm_epilogue_supported(int(R), int(K), int(N), int(mode), int(kblock)))


def gemm_epilogue(x, w, mode, R, K, N, kblock=0, ldx=None, ldw=None, row_div=None, bias1=None, add=None, bias2=None,
                  slope=1.0, zero_init=None, out=None):
    """out [R, N] = act(x [R, K] . B / row_div + bias1 + add + bias2) in one launch (two when the reduction is split).
    mode GEMM_NT: B = w [N, ldw] (y = x w^T); kblock > 0: w is [K / kblock][N][kblock] (KPConv weights read as the
    permuted matrix of the transposed-aggregation grad-input).  mode GEMM_NN: B = w [K, ldw].  ``out`` may be a
    row-strided view.  Raises RuntimeError when the product is not supported (callers ask gemm_epilogue_ok first)."""
    L = _native.lib()
    ldx = K if ldx is None else int(ldx)
    ldw = (K if mode == GEMM_NT else N) if ldw is None else int(ldw)
    if out is None:
        out = torch.empty((R, N), dtype=torch.float32, device=x.device)
    ldy = int(out.stride(0)) if out.dim() == 2 else N
    ldadd = int(add.stride(0)) if add is not None else 0
    nbytes = int(L.d3f_gemm_epilogue_ws_bytes(int(R), int(K), int(N)))
    ws = _ws(nbytes, x.device)
    zn = int(zero_init.numel()) if zero_init is not None else 0
    with _region("gemm_epilogue[R=%d,K=%d,N=%d,mode=%d]" % (R, K, N, mode), 4 * (R * K + K * N + R * N)):
        _native.check(L.d3f_gemm_epilogue(_p(x), ldx, _p(w), ldw, int(mode), int(kblock), int(R), int(K), int(N),
                                          _p(row_div), _p(bias1), _p(add), ldadd, _p(bias2), float(slope), _p(out), ldy,
                                          _p(zero_init), zn, _p(ws), nbytes, _stream()), "d3f_gemm_epilogue")
    return out


# Which products go to the own kernel: KPConv's forward contraction only (every other product is a library GEMM).
# Measured per shape against the library GEMM + its epilogue launch (profiles/gemm_epilogue_bench.py ->
# profiles/r06_gemm_epilogue_bench.txt) and per kind of product inside the 4 x 3 step
# (profiles/calls/r06_gemm_kinds_ab.sh): the own kernel wins where the library's pick is poor or the fused epilogue is
# a large share -- KPConv contractions of the bottom levels (<= 1024 rows x 3840 / 7680: split reduction) and of the
# many-row levels -- and loses on the mid-size square-ish products of levels 2-3 and the decoder, where the library's
# shared-panel tiles reach 0.65-0.75 of the matrix rate.  Inside the step only the KPConv forward pays (+1.0 %); the
# unary blocks' forward and grad-input (from 16k rows), KPConv's grad-input products (transposed-aggregation GEMM up to
# 1024 rows, gW = (g/nn) W^T) and the decoder's four products measured 0 ... -1.4 % (profiles/r06_ab_log.txt) and are
# library GEMMs at their call sites.  The kernel serves them all (GEMM_NT / GEMM_NN, the ``kblock`` form, leading
# dimensions: tests/test_gpu_ops.py::test_gemm_epilogue_matches_float64), so taking one up again is a call-site edit.
def _own_gemm(x, w, R, K, N, *others):
    """Policy + capability: True when KPConv's forward contraction wf [R, K] @ W [K, N] runs on d3f_gemm_epilogue."""
    if not (R <= 1024 or 4096 <= R < 16384):
        return False       # (levels 1 and 3 of a 3-pair stack: 43 vs 33 + 5 us and 45 vs 38 + 5 us inside the step)
    return gemm_epilogue_ok(x, w, GEMM_NN, R, K, N, 0, None, None, *others)


# ---------------------------------------------------------------------------------------------------------------
# 1x1 convolution of the unary blocks (models/blocks.py:481-515): library GEMMs for y = x W^T and grad_x, own
# reduction-parallel kernel for grad_W (tall-skinny: the reduction runs over the points)
# ---------------------------------------------------------------------------------------------------------------
class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, holder=None, deposit=None):
        ctx.save_for_backward(x, weight)
        ctx.gw_slot = _grad_slot(weight)
        ctx.holder, ctx.dep = holder, deposit
        return torch.mm(x, weight.t())

    @staticmethod
    def backward(ctx, grad_out):
        x, weight = ctx.saved_tensors
        go = grad_out.contiguous()
        gx = _add_deposited(ctx.holder, go, weight) if ctx.needs_input_grad[0] else None
        if gx is not None and ctx.dep is not None and ctx.dep.deposit(gx):
            gx = None
        gw = None
        if ctx.needs_input_grad[1]:
            N, Cin, Cout = int(x.shape[0]), int(x.shape[1]), int(weight.shape[0])
            atb = N >= _SPLITK_MIN_ROWS and bool(_native.lib().d3f_linear_grad_weight_supported(N, Cin, Cout))
            gw = _grad_target(ctx.gw_slot, weight)
            _weight_grad(x, go, N, Cin, Cout, gw, atb)
        return gx, _adoptable(gw, ctx.gw_slot), None, None


class _LinearBiasActFn(torch.autograd.Function):
    """act(x W^T + b1 + add + b2) in ONE launch (d3f_linear_bias_act_forward) for the many-row / narrow layers; the
    backward is the epilogue's backward kernel followed by grad_x = g W (row-streaming kernel) and grad_W = g^T x
    (reduction-parallel kernel)."""

    @staticmethod
    def forward(ctx, x, weight, b1, add, b2, slope, holder=None, deposit=None):
        L = _native.lib()
        ctx.holder, ctx.dep = holder, deposit
        N, Cin, Cout = int(x.shape[0]), int(x.shape[1]), int(weight.shape[0])
        out = torch.empty((N, Cout), dtype=torch.float32, device=x.device)
        gbuf, nb = _bias_grad_buffer(b1 is not None and ctx.needs_input_grad[2],
                                     b2 is not None and ctx.needs_input_grad[4], Cout, x.device)
        with _region("linear_fused_fwd[N=%d,Cin=%d,Cout=%d]" % (N, Cin, Cout), 4 * N * (Cin + Cout) + 4 * Cin * Cout):
            _native.check(L.d3f_linear_bias_act_forward(_p(x), _p(weight), N, Cin, Cout, _p(b1), _p(add), _p(b2),
                                                        float(slope), _p(out), _p(gbuf), nb * Cout, _stream()),
                          "d3f_linear_bias_act_forward")
        ctx.save_for_backward(x, weight, out)
        ctx.gbuf = gbuf
        ctx.gw_slot = _grad_slot(weight)
        ctx.slope = float(slope)
        ctx.has = (b1 is not None, add is not None, b2 is not None)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, weight, out = ctx.saved_tensors
        L = _native.lib()
        N, Cin, Cout = int(x.shape[0]), int(x.shape[1]), int(weight.shape[0])
        go = grad_out.contiguous()
        want1 = ctx.has[0] and ctx.needs_input_grad[2]
        want2 = ctx.has[2] and ctx.needs_input_grad[4]
        g1, g2, first, second, pre = _bias_grad_rows(ctx, want1, want2, Cout, go.device)
        atb = ctx.needs_input_grad[1] and bool(L.d3f_linear_grad_weight_supported(N, Cin, Cout))
        bias_part, bias_blocks = None, 0
        if ctx.slope == 1.0 and not (want1 or want2):
            gm = go
        else:
            gm = go if ctx.slope == 1.0 else torch.empty_like(go)
            bias_part, bias_blocks = _epilogue_backward(go, out, ctx.slope, N, Cout, gm if ctx.slope != 1.0 else None,
                                                        first, second, pre, None, atb)
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty_like(x)
            c = ctx.holder.collect() if ctx.holder is not None else None
            if c is not None and not (c.is_contiguous() and c.shape == gx.shape and c.dtype == gx.dtype):
                c = c.contiguous().float().reshape(gx.shape)
            with _region("linear_dx[N=%d,Cin=%d,Cout=%d]" % (N, Cin, Cout), 4 * N * (Cin + Cout) + 4 * Cin * Cout):
                _native.check(L.d3f_linear_grad_input(_p(gm), _p(weight), N, Cin, Cout, _p(c), _p(gx), _stream()),
                              "d3f_linear_grad_input")
            if ctx.dep is not None and ctx.dep.deposit(gx):
                gx = None
        if ctx.needs_input_grad[1]:
            gw = _grad_target(ctx.gw_slot, weight)
            _weight_grad(x, gm, N, Cin, Cout, gw, atb, bias_part, bias_blocks, first, second)
        return (gx, _adoptable(gw, ctx.gw_slot), g1, gm if ctx.has[1] and ctx.needs_input_grad[3] else None, g2,
                None, None, None)


class _LinearPairBiasActFn(torch.autograd.Function):
    """act(x1 W1^T + x2 W2^T + b1a + b1b + b2a + b2b) in ONE launch (d3f_linear_pair_bias_act_forward): the last unary
    block of a bottleneck and its shortcut unary (reference blocks.py:658-686) -- the shortcut tensor is never formed.
    Backward: ONE epilogue pass (masked gradient + the column sums all four biases share), grad_x1 = g W1 and
    grad_x2 = g W2 on the row-streaming kernel, both weight gradients queued / launched on the reduction-parallel kernel."""

    @staticmethod
    def forward(ctx, x1, w1, b1a, b1b, x2, w2, b2a, b2b, slope, deposit2=None):
        L = _native.lib()
        ctx.dep2 = deposit2
        N, C1, C2, Cout = int(x1.shape[0]), int(x1.shape[1]), int(x2.shape[1]), int(w1.shape[0])
        out = torch.empty((N, Cout), dtype=torch.float32, device=x1.device)
        ctx.want = tuple(b is not None and ctx.needs_input_grad[i] for b, i in ((b1a, 2), (b1b, 3), (b2a, 6), (b2b, 7)))
        # (two rows whenever any of the four biases wants a gradient: the epilogue pass fills both)
        gbuf, nb = _bias_grad_buffer(any(ctx.want), any(ctx.want), Cout, x1.device)
        with _region("linear_pair_fwd[N=%d,Cin=%d|%d,Cout=%d]" % (N, C1, C2, Cout),
                     4 * N * (C1 + C2 + Cout) + 4 * (C1 + C2) * Cout):
            _native.check(L.d3f_linear_pair_bias_act_forward(_p(x1), _p(w1), C1, _p(x2), _p(w2), C2, N, Cout, _p(b1a),
                                                             _p(b1b), _p(b2a), _p(b2b), float(slope), _p(out), _p(gbuf),
                                                             nb * Cout, _stream()), "d3f_linear_pair_bias_act_forward")
        ctx.save_for_backward(x1, w1, x2, w2, out)
        ctx.gbuf, ctx.slope = gbuf, float(slope)
        ctx.slots = (_grad_slot(w1), _grad_slot(w2))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x1, w1, x2, w2, out = ctx.saved_tensors
        L = _native.lib()
        N, C1, C2, Cout = int(x1.shape[0]), int(x1.shape[1]), int(x2.shape[1]), int(w1.shape[0])
        go = grad_out.contiguous()
        first, second, _, _, pre = _bias_grad_rows(ctx, any(ctx.want), any(ctx.want), Cout, go.device)
        # Both weight gradients run on the A^T B kernel: it serves every row count >= 1 with channel counts that are
        # multiples of 16 (atb_supported, csrc/linear.hip), which the pairs the forward launch accepts all are
        # (rowgemm_pair_supported: >= 4096 rows, 32 | 64 -> 128 or 16 | 32 -> 64 channels)
        need_w1, need_w2 = ctx.needs_input_grad[1], ctx.needs_input_grad[5]
        fold = need_w1 and need_w2 and _WG_GROUP is not None
        gm = torch.empty_like(go) if ctx.slope != 1.0 else go
        bias_part, bias_blocks = None, 0
        if ctx.slope != 1.0 or first is not None:
            bias_part, bias_blocks = _epilogue_backward(go, out, ctx.slope, N, Cout, gm if ctx.slope != 1.0 else None, first,
                                                        second, pre, None, fold and first is not None)
        third = fourth = None
        if first is not None:
            third, fourth = torch.empty_like(first), torch.empty_like(first)
        gx1 = gx2 = None
        if ctx.needs_input_grad[0]:
            gx1 = torch.empty_like(x1)
            _native.check(L.d3f_linear_grad_input(_p(gm), _p(w1), N, C1, Cout, None, _p(gx1), _stream()),
                          "d3f_linear_grad_input")
        if ctx.needs_input_grad[4]:
            gx2 = torch.empty_like(x2)
            _native.check(L.d3f_linear_grad_input(_p(gm), _p(w2), N, C2, Cout, None, _p(gx2), _stream()),
                          "d3f_linear_grad_input")
            if ctx.dep2 is not None and ctx.dep2.deposit(gx2):
                gx2 = None
        gw1 = gw2 = None
        if need_w1:
            gw1 = _grad_target(ctx.slots[0], w1)
            _weight_grad(x1, gm, N, C1, Cout, gw1, True, bias_part, bias_blocks, first, second)
        if need_w2:
            gw2 = _grad_target(ctx.slots[1], w2)
            # (the second problem finishes the same bias partials into the shortcut's two bias gradients)
            _weight_grad(x2, gm, N, C2, Cout, gw2, True, bias_part, bias_blocks, third, fourth)
        if first is not None and bias_part is None:     # (no fold: the epilogue pass finished first / second itself)
            third.copy_(first)
            fourth.copy_(first)
        g = [first if ctx.want[0] else None, second if ctx.want[1] else None, third if ctx.want[2] else None,
             fourth if ctx.want[3] else None]
        return (gx1, _adoptable(gw1, ctx.slots[0]), g[0], g[1], gx2, _adoptable(gw2, ctx.slots[1]), g[2], g[3],
                None, None)


def linear_pair_supported(N, C1, C2, Cout, *tensors):
    """Whether linear_pair_bias_act serves a pair of these dimensions (the level-0 bottleneck's: (32 | 64) -> 128 from 4096
    rows); ``tensors``: operands already at hand, checked for device / dtype / layout."""
    for t in tensors:
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0):
            return False
    L = _native.lib()
    N, C1, C2, Cout = int(N), int(C1), int(C2), int(Cout)
    return bool(L.d3f_linear_pair_supported(N, C1, C2, Cout)) and bool(L.d3f_linear_fused_supported(N, C1, Cout)) \
        and bool(L.d3f_linear_fused_supported(N, C2, Cout))


def linear_pair_bias_act(x1, w1, b1a, b1b, x2, w2, b2a, b2b, slope=0.1, grad_deposit2=None):
    """act(x1 @ w1^T + b1a + b1b + x2 @ w2^T + b2a + b2b): unary2(x1) + unary_shortcut(x2) + LeakyReLU of a bottleneck
    block in one launch (reference blocks.py:658-686).  grad_deposit2: x2's gradient is handed to a sibling branch
    (GradHolder) instead of being returned."""
    f = _opt_f32
    if not linear_pair_supported(x1.shape[0], x1.shape[1], x2.shape[1], w1.shape[0], x1, x2, w1, w2):
        raise RuntimeError("linear_pair_bias_act: unsupported operands x1%s x2%s w1%s w2%s" % (
            tuple(x1.shape), tuple(x2.shape), tuple(w1.shape), tuple(w2.shape)))
    return _LinearPairBiasActFn.apply(_f32(x1, "x1"), _f32(w1, "w1"), f(b1a, "bias"), f(b1b, "bias"), _f32(x2, "x2"),
                                      _f32(w2, "w2"), f(b2a, "bias"), f(b2b, "bias"), float(slope), grad_deposit2)


# The bias gradient's second pass rides in the weight gradient's second-stage launch (csrc/linear.hip,
# atb_reduce_bias_kernel) whenever both are two-pass forms: N >= 4096 rows for the epilogue's backward and the A^T B
# kernel for grad_W -- the nodes pass ``fold`` = "this node's weight gradient takes the A^T B path".
def _epilogue_backward(go, out, slope, N, C, gm, first, second, pre, row_div, fold, det=False):
    """grad through act(. + biases): masked gradient into ``gm`` (None: not wanted) and the bias gradient(s).  With
    ``fold`` only the first pass runs; returns (partials, blocks) for d3f_linear_grad_weight_bias, else (None, 0).
    ``det``: the node ran its forward under the deterministic mode -- the two-pass form at every row count."""
    L = _native.lib()
    wsb, nws = _bias_bwd_ws(N, C, go.device) if first is not None else (None, 0)
    nblk = int(L.d3f_bias_act_backward_blocks(N, C)) if (fold and first is not None and wsb is not None) else 0
    if nblk > 0:
        _native.check(L.d3f_bias_act_backward_partial(_p(go), _p(out), float(slope), N, C, _p(gm), _p(row_div), _p(wsb),
                                                      nws, _stream()), "d3f_bias_act_backward_partial")
        return wsb, nblk
    if det and first is not None:
        _bias_act_backward_ordered(go, out, slope, N, C, gm, first, second, row_div)
        return None, 0
    _native.check(L.d3f_bias_act_backward(_p(go), _p(out), float(slope), N, C, _p(gm), _p(first), _p(second),
                                          pre if first is not None else 0, _p(row_div), _p(wsb), nws, _stream()),
                  "d3f_bias_act_backward")
    return None, 0


def _bias_act_backward_ordered(go, out, slope, N, C, gm, first, second, row_div):
    """d3f_bias_act_backward without its float atomics (deterministic mode): column sums per row block, added in block
    order; ``first`` / ``second`` are overwritten."""
    L = _native.lib()
    nws = int(L.d3f_bias_act_backward_ordered_ws_bytes(N, C))
    ws = _ws(nws, go.device)
    _count('ordered')
    _native.check(L.d3f_bias_act_backward_ordered(_p(go), _p(out), float(slope), N, C, _p(gm), _p(first), _p(second),
                                                  _p(row_div), _p(ws), nws, _stream()), "d3f_bias_act_backward_ordered")


class WeightGradGroup(object):
    """The weight gradients of ONE backward stage, queued by the autograd nodes and computed together when the stage
    ends (d3f_linear_grad_weight_group: one launch over every problem's tasks + one that sums all slabs and finishes
    the queued bias gradients).  A weight gradient has no consumer before the optimizer (reference trainer.py:103-111),
    so nothing orders it between the grad-input kernels; queued, the 27 problems of a stacked step share one launch's
    ramp-up and tail and the memory-bound ones run beside the matrix-bound ones.

        with ops.weight_grad_group():
            torch.autograd.backward(loss, ...)
        # <- here every p.grad / flat-buffer slot is final

    The queue keeps every operand alive until the flush (under hipGraph capture a freed block would be handed to a
    later allocation of the same capture) and the nodes never modify a queued operand in place (``_add_deposited``).
    Backward runs on autograd's worker thread: the active group is a module global, one backward at a time."""

    def __init__(self):
        self.problems, self.keep = [], []

    def add(self, x, gm, N, Cin, Cout, gw, bias_part, bias_blocks, first, second):
        ldw = int(gw.stride(0)) if gw.dim() == 2 else int(Cin)
        if gw.dim() == 2 and (gw.stride(1) != 1 or gw.shape[0] != Cout or gw.shape[1] != Cin):
            raise RuntimeError("weight-gradient target of shape %s (strides %s) for a [%d, %d] gradient" % (
                tuple(gw.shape), tuple(gw.stride()), Cout, Cin))
        self.problems.append((_p(x), _p(gm), _p(gw), int(N), int(Cin), int(Cout), ldw,
                              _p(bias_part), int(bias_blocks) if bias_part is not None else 0,
                              int(first.numel()) if bias_part is not None else 0,
                              _p(first) if bias_part is not None else None,
                              _p(second) if bias_part is not None else None))
        # held through FRESH tensor objects on the same storage: autograd adopts an incoming gradient as p.grad without a
        # copy only while nobody else holds the tensor object -- a second reference to gw / first / second would make it
        # clone them here, before the flush has written them
        self.keep.append(tuple(t.detach() if t is not None else None for t in (x, gm, gw, bias_part, first, second)))

    def flush(self):
        """Launch the queued problems on the current stream and empty the queue."""
        n = len(self.problems)
        if n == 0:
            return 0
        L = _native.lib()
        arr = (_native.AtbProblem * n)()
        for q, t in zip(arr, self.problems):
            (q.x, q.grad_out, q.grad_w, q.N, q.Cin, q.Cout, q.ldw, q.bias_part, q.bias_blocks, q.bias_cols,
             q.grad_bias, q.grad_bias2) = t
        nbytes = int(L.d3f_linear_grad_weight_group_ws_bytes(arr, n))
        if nbytes == 0:
            raise RuntimeError("d3f_linear_grad_weight_group: unsupported problem in the queue")
        dev = self.keep[0][0].device
        ws = _ws(nbytes, dev)
        flops = sum(2 * t[3] * t[4] * t[5] for t in self.problems)
        with _region("weight_grad_group[n=%d,GFLOP=%.2f]" % (n, flops * 1e-9),
                     sum(4 * t[3] * (t[4] + t[5]) + 4 * t[4] * t[5] for t in self.problems)):
            _native.check(L.d3f_linear_grad_weight_group(arr, n, _p(ws), nbytes, _stream()),
                          "d3f_linear_grad_weight_group")
        self.problems, self.keep = [], []
        return n


_WG_GROUP = None
# False: every weight gradient is launched where autograd reaches it (rounds 1-5; experiments and A/B tests)
GROUP_WEIGHT_GRADS = True


class weight_grad_group(object):
    """Context manager around ONE backward pass (or one stage of a split backward): see WeightGradGroup."""

    def __enter__(self):
        global _WG_GROUP
        if _WG_GROUP is not None:
            raise RuntimeError("weight_grad_group: a backward stage is already collecting weight gradients")
        self.group = WeightGradGroup() if GROUP_WEIGHT_GRADS else None
        _WG_GROUP = self.group
        return self.group

    def __exit__(self, exc_type, exc, tb):
        global _WG_GROUP
        g, _WG_GROUP = _WG_GROUP, None
        if g is not None and exc_type is None:
            g.flush()
        return False


def _queue_small_weight_grad(x, gm, N, Cin, Cout, gw):
    """Few-row weight gradients (the bottom levels: 462 / 1713 rows against 512 ... 7680 x 512 outputs) are library
    GEMMs when launched where autograd reaches them; inside a weight_grad_group they join the stage's grouped launch
    (undivided reduction, one task per 64 x 64 output block, written straight to the target).  True when queued."""
    g = _WG_GROUP
    if g is None or N < 1 or Cin % 16 or Cout % 16:
        return False
    if x.data_ptr() % 16 or gm.data_ptr() % 16 or not x.is_contiguous() or not gm.is_contiguous():
        return False
    g.add(x, gm, N, Cin, Cout, gw, None, 0, None, None)
    return True


def _grad_weight_atb(x, gm, N, Cin, Cout, gw, bias_part, bias_blocks, first, second, label):
    """grad_W [Cout, Cin] = gm^T x on the reduction-parallel kernels; with ``bias_part`` the second stage also sums the
    bias partials into ``first`` (/ ``second``).  Inside a weight_grad_group the problem is only queued."""
    L = _native.lib()
    g = _WG_GROUP
    if g is not None and x.data_ptr() % 16 == 0 and gm.data_ptr() % 16 == 0:
        g.add(x, gm, N, Cin, Cout, gw, bias_part, bias_blocks, first, second)
        return
    if gw.dim() == 2 and not gw.is_contiguous():      # (a column block of a wider matrix: only the group writes in place)
        tmp = torch.empty((Cout, Cin), dtype=torch.float32, device=x.device)
        _grad_weight_atb(x, gm, N, Cin, Cout, tmp, bias_part, bias_blocks, first, second, label)
        gw.copy_(tmp)
        return
    nbytes = L.d3f_linear_grad_weight_ws_bytes(N, Cin, Cout)
    ws = _ws(nbytes, x.device)
    with _region("%s[N=%d,Cin=%d,Cout=%d]" % (label, N, Cin, Cout), 4 * N * (Cin + Cout) + 4 * Cin * Cout):
        if bias_part is not None:
            _native.check(L.d3f_linear_grad_weight_bias(_p(x), _p(gm), N, Cin, Cout, _p(gw), _p(ws), nbytes,
                                                        _p(bias_part), int(bias_blocks), int(first.numel()),
                                                        _p(first), _p(second), _stream()), "d3f_linear_grad_weight_bias")
        else:
            _native.check(L.d3f_linear_grad_weight(_p(x), _p(gm), N, Cin, Cout, _p(gw), _p(ws), nbytes, _stream()),
                          "d3f_linear_grad_weight")


def _weight_grad(x, gm, N, Cin, Cout, gw, use_atb, bias_part=None, bias_blocks=0, first=None, second=None,
                 label="linear_dw", gemm_label=None):
    """grad_W = gm^T x into ``gw`` [Cout, Cin] the way every node does it: the reduction-parallel kernels when the node
    decided ``use_atb`` (they also finish the bias partials, see _grad_weight_atb), else as one of the stage's grouped
    small problems, else a library GEMM (under the profiler region ``gemm_label`` when given)."""
    if use_atb:
        _grad_weight_atb(x, gm, N, Cin, Cout, gw, bias_part, bias_blocks, first, second, label)
    elif not _queue_small_weight_grad(x, gm, N, Cin, Cout, gw):
        with _Region(_PROFILER if gemm_label else None, gemm_label, 4 * N * (Cin + Cout)):
            torch.mm(gm.t(), x, out=gw)


class _LinearLibBiasActFn(torch.autograd.Function):
    """act(x W^T + b1 + add + b2) as library GEMM + one epilogue launch, as ONE autograd node (round 5; it used to be
    _LinearFn followed by _BiasActFn): the backward runs the epilogue's backward, grad_x = g W (library; a sibling
    branch's deposited gradient accumulated by the GEMM) and grad_W = g^T x, and because both live in one node the bias
    gradient's second pass is folded into grad_W's second-stage launch.  ``pack``: see bias_act."""

    @staticmethod
    def forward(ctx, x, weight, b1, add, b2, slope, holder=None, deposit=None, pack=None):
        L = _native.lib()
        ctx.holder, ctx.dep = holder, deposit
        N, C = int(x.shape[0]), int(weight.shape[0])
        gbuf, nb = _bias_grad_buffer(b1 is not None and ctx.needs_input_grad[2],
                                     b2 is not None and ctx.needs_input_grad[4], C, x.device)
        ctx.gbuf, ctx.slope = gbuf, float(slope)
        ctx.has = (b1 is not None, add is not None, b2 is not None)
        ctx.gw_slot = _grad_slot(weight)
        ctx.det = _DETERMINISTIC
        raw = torch.mm(x, weight.t())
        out = torch.empty_like(raw)
        if pack is not None:
            s_pts, want_clear = pack
            spack = torch.empty(16 * N, dtype=torch.uint8, device=x.device)
            gx_clear = torch.empty_like(raw) if want_clear else None
            _native.check(L.d3f_bias_act_forward_pack(
                _p(raw), _p(b1), _p(add), _p(b2), float(slope), N, C, _p(out), _p(gbuf), nb * C, None, None, 0, 0,
                _p(s_pts), _p(spack), _p(gx_clear), _stream()), "d3f_bias_act_forward_pack")
            ctx.save_for_backward(x, weight, out)
            ctx.mark_non_differentiable(spack)
            if gx_clear is not None:
                ctx.mark_non_differentiable(gx_clear)
            ctx.set_materialize_grads(False)
            return out, spack, gx_clear
        _native.check(L.d3f_bias_act_forward(_p(raw), _p(b1), _p(add), _p(b2), float(slope), N, C, _p(out), _p(gbuf),
                                             nb * C, None, None, 0, 0, _stream()), "d3f_bias_act_forward")
        ctx.save_for_backward(x, weight, out)
        return out

    @staticmethod
    def backward(ctx, grad_out, *_unused):
        x, weight, out = ctx.saved_tensors
        none = (None,) * 9
        if grad_out is None:
            return none
        L = _native.lib()
        N, Cin, Cout = int(x.shape[0]), int(x.shape[1]), int(weight.shape[0])
        go = grad_out.contiguous()
        want1 = ctx.has[0] and ctx.needs_input_grad[2]
        want2 = ctx.has[2] and ctx.needs_input_grad[4]
        g1, g2, first, second, pre = _bias_grad_rows(ctx, want1, want2, Cout, go.device)
        need_w = ctx.needs_input_grad[1]
        atb = need_w and N >= _SPLITK_MIN_ROWS and bool(L.d3f_linear_grad_weight_supported(N, Cin, Cout))
        bias_part, bias_blocks = None, 0
        identity = ctx.slope == 1.0
        if identity and first is None:
            gm = go
        else:
            gm = go if identity else torch.empty_like(go)
            bias_part, bias_blocks = _epilogue_backward(go, out, ctx.slope, N, Cout, None if identity else gm, first,
                                                        second, pre, None, atb, ctx.det)
        gx = _add_deposited(ctx.holder, gm, weight) if ctx.needs_input_grad[0] else None
        if gx is not None and ctx.dep is not None and ctx.dep.deposit(gx):
            gx = None
        gw = None
        if need_w:
            gw = _grad_target(ctx.gw_slot, weight)
            _weight_grad(x, gm, N, Cin, Cout, gw, atb, bias_part, bias_blocks, first, second)
        return (gx, _adoptable(gw, ctx.gw_slot), g1, gm if ctx.has[1] and ctx.needs_input_grad[3] else None, g2,
                None, None, None, None)


class _UpsampleLinearFn(torch.autograd.Function):
    """Decoder unary block on [nearest_upsample(x_coarse) | skip] (reference architectures.py:311-314 + blocks.py:481):
        act( [x_c[idx] | skip] W^T + b )  =  act( (x_c W1^T)[idx] + skip W2^T + b ),   W = [W1 | W2].
    A row gather commutes with a row-wise linear map, so the wide half of the product (the 2048/1024/512-channel
    upsampled features) is computed on the COARSE rows -- 3.3x .. 4.8x fewer -- and upsampled inside the epilogue; the
    backward pools the masked gradient back to the coarse rows before the two GEMMs that involve W1."""

    @staticmethod
    def forward(ctx, xc, idx, skip, weight, b1, b2, slope, skip_deposit=None):
        L = _native.lib()
        ctx.skip_dep = skip_deposit
        Nc, Cc = int(xc.shape[0]), int(xc.shape[1])
        N, Cs = int(skip.shape[0]), int(skip.shape[1])
        Cout, H = int(weight.shape[0]), int(idx.shape[1])
        w1, w2 = weight[:, :Cc], weight[:, Cc:]
        t = torch.mm(xc, w1.t())                  # [Nc, Cout] on the coarse rows
        y = torch.mm(skip, w2.t())                # [N, Cout]
        out = torch.empty_like(y)
        nb = int(b1 is not None and ctx.needs_input_grad[4]) + int(b2 is not None and ctx.needs_input_grad[5])
        # backward targets, cleared by the forward launch on the side: bias-gradient rows + the pooled gradient [Nc, Cout]
        zbuf = torch.empty((nb + Nc) * Cout, dtype=torch.float32, device=xc.device)
        gbuf = zbuf[:nb * Cout].view(nb, Cout) if nb else None
        gt_buf = zbuf[nb * Cout:].view(Nc, Cout)
        _native.check(L.d3f_bias_act_forward(_p(y), _p(b1), _p(t), _p(b2), float(slope), N, Cout, _p(out), _p(zbuf),
                                             int(zbuf.numel()), None, _p(idx), H, Nc, _stream()), "d3f_bias_act_forward")
        ctx.save_for_backward(xc, idx, skip, weight, out)
        ctx.gbuf, ctx.gt_buf, ctx.slope = gbuf, gt_buf, float(slope)
        ctx.has = (b1 is not None, b2 is not None)
        ctx.gw_slot = _grad_slot(weight)
        # deterministic mode: the pooled gradient is a gather over the transpose of the table's column 0
        ctx.det = _DETERMINISTIC
        ctx.csr = _csr_of(idx[:, :1].contiguous(), Nc) if ctx.det else None
        return out

    @staticmethod
    def backward(ctx, grad_out):
        xc, idx, skip, weight, out = ctx.saved_tensors
        L = _native.lib()
        Nc, Cc = int(xc.shape[0]), int(xc.shape[1])
        N, Cs = int(skip.shape[0]), int(skip.shape[1])
        Cout, H = int(weight.shape[0]), int(idx.shape[1])
        go = grad_out.contiguous()
        want1 = ctx.has[0] and ctx.needs_input_grad[4]
        want2 = ctx.has[1] and ctx.needs_input_grad[5]
        g1, g2, first, second, pre = _bias_grad_rows(ctx, want1, want2, Cout, go.device)
        gm = torch.empty_like(go)
        atb = (ctx.needs_input_grad[3] and N >= _SPLITK_MIN_ROWS
               and bool(L.d3f_linear_grad_weight_supported(N, Cs, Cout)))
        bias_part, bias_blocks = _epilogue_backward(go, out, ctx.slope, N, Cout, gm, first, second, pre, None, atb,
                                                    ctx.det)
        # pooled gradient of the coarse product: g_t[m] = sum_{n: idx[n,0] = m} gm[n]
        gt, ctx.gt_buf = ctx.gt_buf, None
        pre_t = 1 if gt is not None else 0
        if gt is None:
            gt = torch.empty((Nc, Cout), dtype=torch.float32, device=go.device)
        if ctx.det:
            _closest_pool_backward_gather(gm, Cout, N, Cout, Nc, ctx.csr, gt)
        else:
            _count('scatter')
            _native.check(L.d3f_closest_pool_backward(_p(gm), Cout, _p(idx), N, H, Cout, Nc, _p(gt), pre_t, _stream()),
                          "d3f_closest_pool_backward")
        w1, w2 = weight[:, :Cc], weight[:, Cc:]
        gxc = torch.mm(gt, w1) if ctx.needs_input_grad[0] else None
        gskip = torch.mm(gm, w2) if ctx.needs_input_grad[2] else None
        if gskip is not None and ctx.skip_dep is not None and ctx.skip_dep.deposit(gskip):
            gskip = None    # handed to the encoder block that consumes the same skip tensor (GradHolder)
        gw = None
        if ctx.needs_input_grad[3]:
            gw = _grad_target(ctx.gw_slot, weight)
            # the GEMMs and the grouped second stage write their column block of W's gradient in place (row stride
            # Cc + Cs); the coarse half (few rows) never takes the A^T B path
            _weight_grad(xc, gt, Nc, Cc, Cout, gw[:, :Cc], False)
            _weight_grad(skip, gm, N, Cs, Cout, gw[:, Cc:], atb, bias_part, bias_blocks, first, second)
        return gxc, None, gskip, _adoptable(gw, ctx.gw_slot), g1, g2, None, None


def upsample_linear_bias_act(x_coarse, inds, skip, weight, bias1=None, bias2=None, slope=0.1, skip_grad_deposit=None):
    """act([x_coarse[inds[:,0]] | skip] @ weight^T + bias1 + bias2) without forming the upsampled matrix."""
    xc, sk, w = _f32(x_coarse, "x_coarse"), _f32(skip, "skip"), _f32(weight, "weight")
    idx = _i32(inds, "inds")
    if idx.dim() == 1:
        idx = idx.view(-1, 1)
    if w.shape[1] != xc.shape[1] + sk.shape[1] or idx.shape[0] != sk.shape[0]:
        raise RuntimeError("upsample_linear: shapes x_c%s skip%s W%s idx%s" % (
            tuple(xc.shape), tuple(sk.shape), tuple(w.shape), tuple(idx.shape)))
    return _UpsampleLinearFn.apply(xc, idx, sk, w, _opt_f32(bias1, "bias1"), _opt_f32(bias2, "bias2"), float(slope),
                                   skip_grad_deposit)


# rows from which the unary blocks use the fused row-streaming kernels instead of library GEMM + epilogue launch
_FUSED_LINEAR_MIN_ROWS = 4096
_FUSED_LINEAR_MAX_CIN = 64     # (wider inputs: the library GEMM's deeper tiling + an epilogue launch wins, re-measured in round 6)


def linear_bias_act(x, weight, bias1=None, add=None, bias2=None, slope=0.1, grad_holder=None, grad_deposit=None,
                    pack_for=None):
    """act(x @ weight^T + bias1 + add + bias2) -- the whole unary block (reference blocks.py:481-541,686).
    grad_holder: the gradient a sibling branch deposited for `x` is added by this op's grad-input GEMM;
    grad_deposit: this op hands its own grad_x to the sibling instead of returning it (see GradHolder);
    pack_for: see bias_act (honoured on the library-GEMM + epilogue path)."""
    x, weight = _f32(x, "x"), _f32(weight, "weight")
    N, Cin, Cout = int(x.shape[0]), int(x.shape[1]), int(weight.shape[0])
    # measured (profiles/unary_gemm_microbench.py): the fused kernel beats library GEMM + epilogue launch for
    # Cin <= 64 (7-21 us vs 10-27 us at 38k rows), not for Cin >= 128 where the library's deeper tiling wins
    fused = N >= _FUSED_LINEAR_MIN_ROWS and Cin <= _FUSED_LINEAR_MAX_CIN and \
        _native.lib().d3f_linear_fused_supported(N, Cin, Cout)
    if fused or (x.dim() == 2 and x.is_cuda and (add is None or add.shape == (N, Cout))):
        b1, b2, a = _opt_f32(bias1, "bias1"), _opt_f32(bias2, "bias2"), _opt_f32(add, "add")
        if fused:
            return _LinearBiasActFn.apply(x, weight, b1, a, b2, float(slope), grad_holder, grad_deposit)
        # library GEMM + epilogue as ONE autograd node
        if pack_for is not None and N > 0 and _native.lib().d3f_bias_act_packs(Cout) and N * Cout < 2 ** 32 and \
                int(pack_for[0].shape[0]) == N:
            s_pts = _f32(pack_for[0], "s_pts")
            out, spack, gx_clear = _LinearLibBiasActFn.apply(x, weight, b1, a, b2, float(slope), grad_holder,
                                                             grad_deposit, (s_pts, bool(pack_for[1])))
            out._d3f_spack = PackedSupports(spack, gx_clear, s_pts, N, Cout)
            return out
        return _LinearLibBiasActFn.apply(x, weight, b1, a, b2, float(slope), grad_holder, grad_deposit)
    return bias_act(linear_nobias(x, weight, grad_holder, grad_deposit), bias1, add, bias2, slope=slope,
                    pack_for=pack_for)


def linear_nobias(x, weight, grad_holder=None, grad_deposit=None):
    """x [N, Cin] @ weight[Cout, Cin]^T on the device (fp32)."""
    return _LinearFn.apply(_f32(x, "x"), _f32(weight, "weight"), grad_holder, grad_deposit)


# ---------------------------------------------------------------------------------------------------------------
# pools (models/blocks.py:79-110)
# ---------------------------------------------------------------------------------------------------------------
class _MaxPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, idx, deposit=None, incoming=None, width=None, groups=None):
        ctx.dep, ctx.incoming = deposit, incoming
        g_len, g_n = groups if groups is not None else (None, 0)
        Ns, C = int(x.shape[0]), int(x.shape[1])
        Nq, H = int(idx.shape[0]), int(idx.shape[1])
        out = torch.empty((Nq, C), dtype=torch.float32, device=x.device)
        arg = torch.empty((Nq, C), dtype=torch.int32, device=x.device)
        # cleared by the forward launch (the deterministic mode's gather writes every row: nothing to clear)
        gx_buf = torch.empty_like(x) if (ctx.needs_input_grad[0] and not _DETERMINISTIC) else None
        with _region("max_pool_fwd[Nq=%d,C=%d]" % (Nq, C), 4 * Nq * H + 4 * Nq * H * C + 4 * Nq * C):
            _native.check(_native.lib().d3f_max_pool_forward(_p(x), Ns, C, _p(idx), Nq, H, _p(out), _p(arg),
                                                             _p(gx_buf), _p(width), _p(g_len),
                                                             int(g_len.numel()) if g_len is not None else 0, int(g_n),
                                                             _stream()), "d3f_max_pool_forward")
        ctx.save_for_backward(arg)
        ctx.shape = (Ns, C)
        ctx.gx_buf = gx_buf
        # deterministic mode: the backward gathers over the CSR transpose of the pooling table
        ctx.det = _DETERMINISTIC
        ctx.csr = _csr_of(idx, Ns) if (ctx.det and ctx.needs_input_grad[0]) else None
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (arg,) = ctx.saved_tensors
        Ns, C = ctx.shape
        go = grad_out.contiguous().float()
        gx, ctx.gx_buf = ctx.gx_buf, None
        pre = 1 if gx is not None else 0
        # a gradient an older consumer of x already produced (the decoder, for a skip tensor): scatter on top of it
        c = ctx.incoming.collect() if ctx.incoming is not None else None
        if ctx.det:
            # order per element: the incoming gradient FIRST, then the queries that list the row, ascending
            base = None
            if c is not None and tuple(c.shape) == (Ns, C):
                base, c = c.contiguous().float(), None
            if gx is None:
                gx = torch.empty((Ns, C), dtype=torch.float32, device=go.device)
            ptr, ent = ctx.csr
            _count('ordered')
            with _region("max_pool_bwd_gather[Ns=%d,C=%d]" % (Ns, C), 8 * int(arg.shape[0]) * C + 4 * Ns * C):
                _native.check(_native.lib().d3f_max_pool_backward_gather(_p(go), _p(arg), int(arg.shape[0]), C, Ns,
                                                                         _p(ptr), _p(ent), _p(base), _p(gx), _stream()),
                              "d3f_max_pool_backward_gather")
            if c is not None:
                gx.add_(c)
            if ctx.dep is not None and ctx.dep.deposit(gx):
                gx = None
            return gx, None, None, None, None, None
        if c is not None and c.is_contiguous() and c.dtype == torch.float32 and tuple(c.shape) == (Ns, C):
            gx, pre, c = c, 1, None
        if gx is None:
            gx = torch.empty((Ns, C), dtype=torch.float32, device=go.device)
        _count('scatter')
        _native.check(_native.lib().d3f_max_pool_backward(_p(go), _p(arg), int(arg.shape[0]), C, Ns, _p(gx), pre,
                                                          _stream()), "d3f_max_pool_backward")
        if c is not None:
            gx.add_(c)
        if ctx.dep is not None and ctx.dep.deposit(gx):
            gx = None
        return gx, None, None, None, None, None


def _check_groups(width, groups, what):
    """(q_lens int32 [B] on the device, clouds per group) of a batch that stacks several reference batches; ``width``
    then holds one entry per group."""
    if groups is None:
        if width is not None and not (width.is_cuda and width.dtype == torch.int32 and width.numel() == 1):
            raise ValueError("width must be a device int32[1] tensor")
        return None
    g_len, g_n = groups
    if not (isinstance(g_len, torch.Tensor) and g_len.is_cuda and g_len.dtype == torch.int32) or int(g_n) < 1:
        raise ValueError("%s: groups = (device int32 stack lengths, clouds per group)" % what)
    n_groups = -(-int(g_len.numel()) // int(g_n))
    if width is not None and not (width.is_cuda and width.dtype == torch.int32 and width.numel() == n_groups):
        raise ValueError("%s: width must hold one device int32 per group (%d)" % (what, n_groups))
    return g_len, int(g_n)


def max_pool(x, inds, grad_deposit=None, grad_incoming=None, width=None, groups=None):
    """max over the neighbors of every query row, zero shadow row included (blocks.py:94-110).  ``width``: device
    int32[1] = the table's max neighbor count; only the first min(H, width) columns count -- the table the reference
    would have built (dataloader.py:64-66) when ``inds`` is kept at a wider, static width.  ``groups`` = (stack lengths
    of the QUERY level, clouds per group): the batch stacks several reference batches (8 pairs: groups of 2) and
    ``width`` holds one entry per group."""
    groups = _check_groups(width, groups, "max_pool")
    return _MaxPoolFn.apply(_f32(x, "x"), _i32(inds, "inds"), grad_deposit, grad_incoming, width, groups)


class _ClosestPoolFn(torch.autograd.Function):
    """closest_pool, optionally concatenated with a skip tensor ([upsampled | skip]) by the same launch."""

    @staticmethod
    def forward(ctx, x, idx, skip):
        Ns, C = int(x.shape[0]), int(x.shape[1])
        Nq, H = int(idx.shape[0]), int(idx.shape[1])
        Cs = int(skip.shape[1]) if skip is not None else 0
        out = torch.empty((Nq, C + Cs), dtype=torch.float32, device=x.device)
        # cleared by the forward launch (the deterministic mode's gather writes every row: nothing to clear)
        gx_buf = torch.empty_like(x) if (ctx.needs_input_grad[0] and not _DETERMINISTIC) else None
        _native.check(_native.lib().d3f_closest_pool_forward(_p(x), Ns, C, _p(idx), Nq, H, _p(skip), Cs, _p(out),
                                                             _p(gx_buf), _stream()), "d3f_closest_pool_forward")
        ctx.save_for_backward(idx)
        ctx.shape = (Ns, C, Cs)
        ctx.gx_buf = gx_buf
        # deterministic mode: the backward gathers over the CSR transpose of the table's column 0
        ctx.det = _DETERMINISTIC
        ctx.csr = _csr_of(idx[:, :1].contiguous(), Ns) if (ctx.det and ctx.needs_input_grad[0]) else None
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        Ns, C, Cs = ctx.shape
        go = grad_out if grad_out.dtype == torch.float32 else grad_out.float()
        # a column slice of a wider row-major matrix (the [upsampled | skip] gradient) is read in place
        if not (go.dim() == 2 and go.stride(1) == 1 and go.stride(0) >= C + Cs):
            go = go.contiguous()
        ld = int(go.stride(0)) if go.shape[0] > 1 else C + Cs
        gx = None
        if ctx.needs_input_grad[0]:
            gx, ctx.gx_buf = ctx.gx_buf, None
            pre = 1 if gx is not None else 0
            if gx is None:
                gx = torch.empty((Ns, C), dtype=torch.float32, device=go.device)
            if ctx.det:
                _closest_pool_backward_gather(go, ld, int(idx.shape[0]), C, Ns, ctx.csr, gx)
            else:
                _count('scatter')
                _native.check(_native.lib().d3f_closest_pool_backward(_p(go), ld, _p(idx), int(idx.shape[0]),
                                                                      int(idx.shape[1]), C, Ns, _p(gx), pre, _stream()),
                              "d3f_closest_pool_backward")
        g_skip = go[:, C:] if (Cs and ctx.needs_input_grad[2]) else None
        return gx, None, g_skip


def _closest_pool_backward_gather(go, ld, Nq, C, Ns, csr, gx):
    """gx [Ns, C] = per coarse row the sum of the ``go`` rows (stride ``ld``) of the fine rows that point to it, ascending:
    the gather form of d3f_closest_pool_backward (deterministic mode)."""
    ptr, ent = csr
    _count('ordered')
    with _region("closest_pool_bwd_gather[Ns=%d,C=%d]" % (Ns, C), 4 * Nq * C + 4 * Ns * C):
        _native.check(_native.lib().d3f_closest_pool_backward_gather(_p(go), int(ld), int(Nq), int(C), int(Ns), _p(ptr),
                                                                     _p(ent), _p(gx), _stream()),
                      "d3f_closest_pool_backward_gather")


def closest_pool(x, inds, skip=None):
    """x'[inds[:, 0]] (reference blocks.py:79-91); with ``skip`` [Nq, Cs] the result is torch.cat([pooled, skip], 1)."""
    idx = _i32(inds, "inds")
    if idx.dim() == 1:
        idx = idx.view(-1, 1)
    sk = _opt_f32(skip, "skip")
    if sk is not None and (sk.dim() != 2 or sk.shape[0] != idx.shape[0]):
        raise RuntimeError("closest_pool: skip %s does not match %d query rows" % (tuple(sk.shape), idx.shape[0]))
    return _ClosestPoolFn.apply(_f32(x, "x"), idx, sk)


# ---------------------------------------------------------------------------------------------------------------
# block epilogue: bias (+ residual) (+ LeakyReLU) (models/blocks.py:473,497,598,676,686)
# ---------------------------------------------------------------------------------------------------------------
def _bias_bwd_ws(N, C, device):
    nb = int(_native.lib().d3f_bias_act_backward_ws_bytes(N, C))
    return (_ws(nb, device), nb) if nb else (None, 0)


class _BiasActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, b1, add, b2, slope, pack=None):
        N, C = int(x.shape[0]), int(x.shape[1])
        out = torch.empty_like(x)
        # the backward's bias-gradient accumulators [2, C] are cleared by the forward kernel on the side: no fill
        # launch in backward, and the two bias parameters get separate buffers (autograd would clone a shared one)
        gbuf, nb = _bias_grad_buffer(b1 is not None and ctx.needs_input_grad[1],
                                     b2 is not None and ctx.needs_input_grad[3], C, x.device)
        ctx.gbuf, ctx.slope = gbuf, float(slope)
        ctx.has = (b1 is not None, add is not None, b2 is not None)
        ctx.det = _DETERMINISTIC
        if pack is not None:
            s_pts, want_clear = pack
            spack = torch.empty(16 * N, dtype=torch.uint8, device=x.device)
            gx_clear = torch.empty_like(x) if want_clear else None
            _native.check(_native.lib().d3f_bias_act_forward_pack(
                _p(x), _p(b1), _p(add), _p(b2), float(slope), N, C, _p(out), _p(gbuf), nb * C, None, None, 0, 0,
                _p(s_pts), _p(spack), _p(gx_clear), _stream()), "d3f_bias_act_forward_pack")
            ctx.save_for_backward(out)
            ctx.mark_non_differentiable(spack)
            if gx_clear is not None:
                ctx.mark_non_differentiable(gx_clear)
            # (without this autograd hands backward zero-FILLED gradients for the two by-products: two fill launches
            # per packed layer and step, visible in the step timeline as FillFunctor pairs)
            ctx.set_materialize_grads(False)
            return out, spack, gx_clear
        _native.check(_native.lib().d3f_bias_act_forward(_p(x), _p(b1), _p(add), _p(b2), float(slope), N, C, _p(out),
                                                         _p(gbuf), nb * C, None, None, 0, 0, _stream()),
                      "d3f_bias_act_forward")
        ctx.save_for_backward(out)
        return out

    @staticmethod
    def backward(ctx, grad_out, *_unused):
        (out,) = ctx.saved_tensors
        N, C = int(out.shape[0]), int(out.shape[1])
        if grad_out is None:     # (only by-products were used: possible with set_materialize_grads(False))
            return None, None, None, None, None, None
        go = grad_out.contiguous()
        need_gx = ctx.needs_input_grad[0] or (ctx.has[1] and ctx.needs_input_grad[2])
        want1 = ctx.has[0] and ctx.needs_input_grad[1]
        want2 = ctx.has[2] and ctx.needs_input_grad[3]
        identity = ctx.slope == 1.0
        gx = None
        g1, g2, first, second, pre = _bias_grad_rows(ctx, want1, want2, C, go.device)
        if identity and not (want1 or want2):
            gx = go
        elif need_gx or want1 or want2:
            if need_gx and not identity:
                gx = torch.empty_like(go)
            wsb, nws = _bias_bwd_ws(N, C, go.device) if first is not None else (None, 0)
            if ctx.det and first is not None:
                _bias_act_backward_ordered(go, out, ctx.slope, N, C, gx, first, second, None)
            else:
                _native.check(_native.lib().d3f_bias_act_backward(_p(go), _p(out), ctx.slope, N, C, _p(gx), _p(first),
                                                                  _p(second), pre if first is not None else 0, None,
                                                                  _p(wsb), nws, _stream()), "d3f_bias_act_backward")
            if identity:
                gx = go
        return (gx if ctx.needs_input_grad[0] else None, g1, gx if ctx.has[1] and ctx.needs_input_grad[2] else None,
                g2, None, None)


def bias_act(x, bias1=None, add=None, bias2=None, slope=0.1, pack_for=None):
    """act(x + bias1 + add + bias2) with act = LeakyReLU(slope) (slope = 1.0: no activation); one launch each way.
    ``pack_for`` = (s_pts, want_clear): the result is the feature matrix of a KPConv over the supports ``s_pts``; the
    same launch leaves that KPConv's packed supports (and, with ``want_clear``, its cleared grad_x target) behind as
    ``result._d3f_spack`` (PackedSupports) -- one launch less per KPConv layer."""
    x = _f32(x, "x")
    if x.dim() != 2:
        raise RuntimeError("bias_act expects [N, C]")
    b1, b2, a = _opt_f32(bias1, "bias1"), _opt_f32(bias2, "bias2"), _opt_f32(add, "add")
    if a is not None and a.shape != x.shape:
        raise RuntimeError("bias_act: residual shape %s != %s" % (tuple(a.shape), tuple(x.shape)))
    if pack_for is not None and x.shape[0] > 0 and _native.lib().d3f_bias_act_packs(int(x.shape[1])) and \
            x.numel() < 2 ** 32 and int(pack_for[0].shape[0]) == int(x.shape[0]):
        s_pts = _f32(pack_for[0], "s_pts")
        out, spack, gx_clear = _BiasActFn.apply(x, b1, a, b2, float(slope), (s_pts, bool(pack_for[1])))
        out._d3f_spack = PackedSupports(spack, gx_clear, s_pts, x.shape[0], x.shape[1])
        return out
    return _BiasActFn.apply(x, b1, a, b2, float(slope))


# ---------------------------------------------------------------------------------------------------------------
# batch normalisation over the stacked points (models/blocks.py:454-471, use_bn=True) -- csrc/batchnorm.hip
# ---------------------------------------------------------------------------------------------------------------
class _BatchNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, training, momentum, eps, slope, n_live):
        N, C = int(x.shape[0]), int(x.shape[1])
        L = _native.lib()
        y = torch.empty_like(x)
        mean = torch.empty(C, dtype=torch.float32, device=x.device)
        invstd = torch.empty(C, dtype=torch.float32, device=x.device)
        nbytes = L.d3f_batchnorm_ws_bytes(N, C)
        ws = _ws(nbytes, x.device)
        with _region("batchnorm_fwd[N=%d,C=%d]" % (N, C), 16 * N * C):
            _native.check(L.d3f_batchnorm_forward(_p(x), N, C, _p(n_live), _p(weight), _p(bias), _p(running_mean),
                                                  _p(running_var), float(momentum), float(eps), 1 if training else 0,
                                                  float(slope), _p(y), _p(mean), _p(invstd), _p(ws), nbytes, _stream()),
                          "d3f_batchnorm_forward")
        ctx.save_for_backward(x, weight, bias, mean, invstd)
        ctx.n_live, ctx.slope, ctx.training = n_live, float(slope), bool(training)
        ctx.mark_non_differentiable(mean, invstd)
        ctx.set_materialize_grads(False)
        return y, mean, invstd

    @staticmethod
    def backward(ctx, gy, _gm, _gi):
        if gy is None:
            return (None,) * 10
        x, weight, bias, mean, invstd = ctx.saved_tensors
        N, C = int(x.shape[0]), int(x.shape[1])
        L = _native.lib()
        gy = gy.contiguous()
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gw = torch.empty(C, dtype=torch.float32, device=x.device) if weight is not None else None
        gb = torch.empty(C, dtype=torch.float32, device=x.device) if bias is not None else None
        nbytes = L.d3f_batchnorm_ws_bytes(N, C)
        ws = _ws(nbytes, x.device)
        with _region("batchnorm_bwd[N=%d,C=%d]" % (N, C), 20 * N * C):
            _native.check(L.d3f_batchnorm_backward(_p(x), N, C, _p(ctx.n_live), _p(weight), _p(bias), _p(mean),
                                                   _p(invstd), ctx.slope, 1 if ctx.training else 0, _p(gy), _p(gx),
                                                   _p(gw), _p(gb), _p(ws), nbytes, _stream()),
                          "d3f_batchnorm_backward")
        return gx, gw, gb, None, None, None, None, None, None, None


def batch_norm(x, weight, bias, running_mean, running_var, training, momentum=0.1, eps=1e-5, slope=1.0, n_live=None):
    """nn.BatchNorm1d over the N stacked points of x [N, C] (the reference's BatchNormBlock, blocks.py:465-471) with an
    optional LeakyReLU(slope) fused behind it.  Training mode normalises with the batch statistics and updates
    ``running_mean`` / ``running_var`` in place (momentum, unbiased variance); eval mode uses the running statistics.
    ``n_live`` (int32 device scalar) bounds the live rows when x is a capacity-shaped buffer."""
    x = _f32(x, "x")
    if x.dim() != 2:
        raise RuntimeError("batch_norm expects [N, C]")
    if not training and (running_mean is None or running_var is None):
        raise RuntimeError("batch_norm in eval mode needs running statistics")
    if momentum is None:
        raise RuntimeError("batch_norm: cumulative-average momentum (None) is not supported")
    w, b = _opt_f32(weight, "weight"), _opt_f32(bias, "bias")
    return _BatchNormFn.apply(x, w, b, running_mean, running_var, bool(training), float(momentum), float(eps),
                              float(slope), n_live)[0]


# ---------------------------------------------------------------------------------------------------------------
# detector score (models/architectures.py:322-368)
# ---------------------------------------------------------------------------------------------------------------
def global_max(x, lens=None, group=0):
    """max(x) as a device scalar; with ``lens`` (int32 stack lengths) only the first sum(lens) rows count; with
    ``group`` > 0 one maximum per group of that many consecutive clouds (float32 [ceil(B/group)])."""
    x = _f32(x, "x")
    if group:
        G = -(-int(lens.numel()) // int(group))
        out = torch.empty(G, dtype=torch.float32, device=x.device)
        ws = _ws(4 * G, x.device)
        _native.check(_native.lib().d3f_global_max_groups(_p(x), int(x.shape[0]), int(x.shape[1]), _p(lens),
                                                          int(lens.numel()), int(group), _p(out), _p(ws),
                                                          max(4 * G, 256), _stream()), "d3f_global_max_groups")
        return out
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    ws = _ws(256, x.device)
    if lens is None:
        _native.check(_native.lib().d3f_global_max(_p(x), x.numel(), _p(out), _p(ws), 256, _stream()),
                      "d3f_global_max")
    else:
        _native.check(_native.lib().d3f_global_max_rows(_p(x), int(x.shape[0]), int(x.shape[1]), _p(lens),
                                                        int(lens.numel()), _p(out), _p(ws), 256, _stream()),
                      "d3f_global_max_rows")
    return out


class _DetScoreFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, idx, training, lens=None, width=None, group=0):
        N, C, H = int(feat.shape[0]), int(feat.shape[1]), int(idx.shape[1])
        if group and lens is None:
            raise RuntimeError("detection_scores: the grouped form needs the stack lengths")
        fmax = global_max(feat, lens, group)
        scores = torch.empty((N, 1), dtype=torch.float32, device=feat.device)
        na = _native.lib().d3f_detection_scores_aux_floats(C) if (training and ctx.needs_input_grad[0] and H <= 64) else 0
        aux = torch.empty((N, na), dtype=torch.float32, device=feat.device) if na else None
        with _region("detection_fwd[N=%d]" % N, 4 * N * H + 4 * N * H * C + 4 * N * C + 4 * N):
            _native.check(_native.lib().d3f_detection_scores_forward(_p(feat), N, C, _p(idx), H, _p(fmax),
                                                                     1 if training else 0, _p(scores), _p(aux),
                                                                     _p(width), _p(lens) if group else None,
                                                                     int(lens.numel()) if group else 0, int(group),
                                                                     _stream()), "d3f_detection_scores_forward")
        ctx.aux = aux
        ctx.save_for_backward(feat, idx, fmax)
        ctx.training = bool(training)
        ctx.groups = (lens, int(group)) if group else None
        return scores

    @staticmethod
    def backward(ctx, grad_scores):
        feat, idx, fmax = ctx.saved_tensors
        if not ctx.training:
            raise RuntimeError("detection_scores: backward is defined for training mode only")
        N, C, H = int(feat.shape[0]), int(feat.shape[1]), int(idx.shape[1])
        gs = grad_scores.contiguous().float()
        gf = torch.empty_like(feat)
        nws = int(_native.lib().d3f_detection_scores_ws_bytes(N, C))
        ws = _ws(nws, feat.device)
        with _region("detection_bwd[N=%d]" % N, 4 * N * H + 4 * N * H * C + 12 * N * C + 4 * N):
            if ctx.groups is not None:   # stacked pairs: the normaliser's gradient stays inside each pair
                lens, group = ctx.groups
                _native.check(_native.lib().d3f_detection_scores_backward_groups(
                    _p(feat), N, C, _p(idx), H, _p(fmax), _p(gs), _p(ctx.aux), _p(gf), _p(lens), int(lens.numel()),
                    group, _p(ws), nws, _stream()), "d3f_detection_scores_backward_groups")
            else:
                _native.check(_native.lib().d3f_detection_scores_backward(_p(feat), N, C, _p(idx), H, _p(fmax), _p(gs),
                                                                          _p(ctx.aux), _p(gf), _p(ws), nws, _stream()),
                              "d3f_detection_scores_backward")
        return gf, None, None, None, None, None


def detection_scores(features, neighbors, training=True, lens=None, width=None, group=0):
    """scores [N,1] from un-normalised descriptors [N,C] and the layer-0 neighbor table.  ``lens`` (device int32
    stack lengths) restricts the global-max normaliser to the live rows of a capacity-shaped batch; ``width`` (device
    int32[1], the table's max neighbor count) makes a table kept at the full limit behave like the reference's
    min(limit, max_count)-column table in the eval-mode local-maximum gate (as for max_pool).  ``group`` > 0: the batch
    stacks several reference batches of that many clouds (8 pairs: 2); the normaliser (architectures.py:342 takes the
    maximum of ONE pair) and ``width`` are then per group, in forward and backward."""
    _check_groups(width, (lens, group) if group else None, "detection_scores")
    if _DETERMINISTIC and training and torch.is_grad_enabled() and features.requires_grad:
        # (the training step scores the sampled rows inside the loss node, ops.DetectorRows, which has an ordered form)
        _no_deterministic_form("detection_scores (the dense detector's backward)")
    return _DetScoreFn.apply(_f32(features, "features"), _i32(neighbors, "neighbors"), bool(training), lens, width,
                             int(group))


class DetectorRows(object):
    """The arguments of ``detection_scores`` without the features: handed to ``train_loss`` and its siblings in place
    of a ``scores`` tensor, it makes the loss node score the 2 P M sampled rows itself (d3f_detection_rows_forward: the
    dense kernel's own body, one wave per sampled row) -- the reference's loss reads no other score (trainer.py:90-97).
    The node is then differentiable with respect to ``x`` alone and returns the one merged gradient."""

    def __init__(self, neighbors, training=True, lens=None, width=None, group=0):
        _check_groups(width, (lens, group) if group else None, "DetectorRows")
        if group and lens is None:
            raise RuntimeError("DetectorRows: the grouped form needs the stack lengths")
        self.neighbors = _i32(neighbors, "neighbors")
        self.training, self.lens, self.width, self.group = bool(training), lens, width, int(group)

    @staticmethod
    def supported(C, H):
        """The rows form's domain (the aux path's own: C in {16, 32, 64}, H <= 64); others keep the dense detector."""
        return bool(_native.lib().d3f_detection_rows_supported(int(C), int(H)))


# ---------------------------------------------------------------------------------------------------------------
# circle + detector loss (utils/loss.py:8-44,111-141,149-158)
# ---------------------------------------------------------------------------------------------------------------
def _loss_outputs(oa, P, M, with_total):
    """(scalars [P,6], total or None, dists [P,M,M], fp [P*M], an [P*M], stats) for either loss's forward entry."""
    dev = oa.device
    return (torch.empty((P, 6), dtype=torch.float32, device=dev),
            torch.empty((), dtype=torch.float32, device=dev) if with_total else None,
            torch.empty((P, M, M), dtype=torch.float32, device=dev),
            torch.empty(P * M, dtype=torch.float32, device=dev), torch.empty(P * M, dtype=torch.float32, device=dev),
            torch.empty(P * _native.lib().d3f_circle_det_loss_stats_floats(M), dtype=torch.float32, device=dev))


def _circle_tiled(M, C):
    """The strips route of d3f_circle_det_loss_*; beyond it one workgroup serves one pair, without weights or total."""
    return M <= 128 and C <= 64


def _circle_fwd(oa, op, sa, sp, neg_mask, P, M, params, weights=(1.0, 1.0), with_total=False):
    """Forward launches on selected rows oa/op [P*M,C]: (scalars [P,6], total, dists [P,M,M], fp, an, stats) with
    total = sum_p (w_desc desc_p + w_det det_p), or None."""
    C = int(oa.shape[1])
    s, sr, pm, nm = params
    out = scalars, total, dists, fp, an, stats = _loss_outputs(oa, P, M, with_total)
    _native.check(_native.lib().d3f_circle_det_loss_forward(
        _p(oa), _p(op), M, C, P, _p(neg_mask), _p(sa), _p(sp), s, sr, pm, nm, weights[0], weights[1], _p(dists), _p(fp),
        _p(an), _p(scalars), _p(total), _p(stats), _stream()), "d3f_circle_det_loss_forward")
    return out


def _circle_bwd(oa, op, sa, sp, neg_mask, dists, stats, P, M, params, weights, g_ptrs):
    """(ga, gp, gsa, gsp) of _circle_fwd.  ``g_ptrs``: device addresses of d / d desc and d / d det (the same address
    twice for d / d total: the kernel applies ``weights``)."""
    L = _native.lib()
    C = int(oa.shape[1])
    s, sr, pm, nm = params
    ga, gp = torch.empty_like(oa), torch.empty_like(op)
    gsa, gsp = torch.empty_like(sa), torch.empty_like(sp)
    nbytes = 0 if _circle_tiled(M, C) else L.d3f_circle_det_loss_ws_bytes(M)
    ws = _ws(nbytes, oa.device) if nbytes else None
    _native.check(L.d3f_circle_det_loss_backward(
        _p(oa), _p(op), M, C, P, _p(neg_mask), _p(sa), _p(sp), s, sr, pm, nm, weights[0], weights[1], _p(dists),
        _p(stats), g_ptrs[0], g_ptrs[1], _p(ga), _p(gp), _p(gsa), _p(gsp), _p(ws), nbytes, _stream()),
        "d3f_circle_det_loss_backward")
    return ga, gp, gsa, gsp


class _CircleDetFn(torch.autograd.Function):
    """Returns (scalars[6], dists[M,M], furthest_positive[M], average_negative[M]); scalars[0] = desc loss,
    scalars[1] = det loss are differentiable wrt anchor / positive / scores."""

    @staticmethod
    def forward(ctx, anchor, positive, neg_mask, anc_score, pos_score, log_scale, safe_radius, pos_margin,
                neg_margin):
        M = int(anchor.shape[0])
        ctx.params = (float(log_scale), float(safe_radius), float(pos_margin), float(neg_margin))
        scalars, _, dists, fp, an, stats = _circle_fwd(anchor, positive, anc_score, pos_score, neg_mask, 1, M, ctx.params)
        scalars, dists = scalars.view(6), dists.view(M, M)
        ctx.save_for_backward(anchor, positive, neg_mask, anc_score, pos_score, dists, stats)
        ctx.mark_non_differentiable(dists, fp, an)
        ctx.set_materialize_grads(False)
        return scalars, dists, fp, an

    @staticmethod
    def backward(ctx, g_scalars, g_dists, g_fp, g_an):
        if g_scalars is None:
            return (None,) * 9
        anchor, positive, neg_mask, anc_score, pos_score, dists, stats = ctx.saved_tensors
        g = g_scalars.contiguous().float()
        ga, gp, gsa, gsp = _circle_bwd(anchor, positive, anc_score, pos_score, neg_mask, dists, stats, 1,
                                       int(anchor.shape[0]), ctx.params, (1.0, 1.0), (g.data_ptr(), g.data_ptr() + 4))
        return ga, gp, None, gsa, gsp, None, None, None, None


def _neg_mask_of(dist_keypts, safe_radius):
    if dist_keypts is None or not dist_keypts.is_cuda:
        raise RuntimeError("dist_keypts must be a CUDA/HIP tensor")
    return (dist_keypts > safe_radius).to(torch.uint8).contiguous()  # evaluated in the caller's dtype (f64)


def circle_det_loss(anchor, positive, dist_keypts, anc_score, pos_score, log_scale=10.0, safe_radius=0.1,
                    pos_margin=0.1, neg_margin=1.4):
    anchor, positive = _f32(anchor, "anchor"), _f32(positive, "positive")
    neg_mask = _neg_mask_of(dist_keypts, safe_radius)
    sa = _f32(anc_score, "anc_score").reshape(-1)
    sp = _f32(pos_score, "pos_score").reshape(-1)
    return _CircleDetFn.apply(anchor, positive, neg_mask, sa, sp, log_scale, safe_radius, pos_margin, neg_margin)


def _sampled_rows(idx_a, idx_p, p_offset=None, lens=None):
    """(saved, stride): the sampled rows of a training step as the select + normalise and detector entries take them
    ("The sampled rows" in include/d3feat_hip.h).  ``saved`` = (ia, ip, p_offset, lens), what a backward keeps: int64 index
    vectors read with ``stride``; one pair has global rows, ``p_offset`` (device int32 [1]) or None and ``lens`` None; P
    stacked pairs have cloud-local rows and ``lens`` device int32 [2P].  The two columns of one contiguous [T,2] int64
    table (``corr[:, 0]``, ``corr[:, 1]``) are read in place with stride 2; anything else is compacted."""
    if (idx_a.dtype == torch.int64 and idx_p.dtype == torch.int64 and idx_a.dim() == 1 and idx_p.dim() == 1
            and idx_a.stride(0) == 2 and idx_p.stride(0) == 2 and idx_p.data_ptr() == idx_a.data_ptr() + 8
            and idx_a.shape == idx_p.shape):
        return (idx_a, idx_p, p_offset, lens), 2
    ia, ip = idx_a.contiguous(), idx_p.contiguous()
    if ia.dtype != torch.int64 or ip.dtype != torch.int64:
        ia, ip = ia.long(), ip.long()
    return (ia, ip, p_offset, lens), 1


def _select_rows_fwd(x, scores, corr, p_offset, lens, P, M):
    """The 2 P M sampled rows of corr [P*M,2], gathered and normalised by one launch: (oa, op [P*M,C], sa, sp [P*M], saved,
    stride), the last two as _sampled_rows gives them.  ``scores`` None: sa / sp are left for the detector's rows form to
    fill (_det_rows_fwd)."""
    saved, stride = _sampled_rows(corr[:, 0], corr[:, 1], p_offset, lens)
    return _select_normalize_fwd(x, scores, saved, stride, P, M) + (saved, stride)


def _select_normalize_fwd(x, scores, saved, stride, P, M):
    N, C, T, dev = int(x.shape[0]), int(x.shape[1]), P * M, x.device
    ia, ip, p_offset, lens = saved
    oa = torch.empty((T, C), dtype=torch.float32, device=dev)
    op = torch.empty((T, C), dtype=torch.float32, device=dev)
    sa = torch.empty(T, dtype=torch.float32, device=dev)
    sp = torch.empty(T, dtype=torch.float32, device=dev)
    _native.check(_native.lib().d3f_select_normalize_forward(
        _p(x), _p(scores), N, C, _p(ia), _p(ip), stride, M, P, _p(p_offset), _p(lens), _p(oa), _p(op), _p(sa), _p(sp),
        _stream()), "d3f_select_normalize_forward")
    return oa, op, sa, sp


def _select_rows_bwd(x, saved, stride, P, M, g_a, g_p, g_sa, g_sp, with_scores=True):
    """(grad_x [N,C], grad_scores [N,1]) of _select_normalize_fwd: one allocation, cleared by one fill.  ``with_scores``
    False: (grad_x, None), the score gradients go through _det_rows_bwd instead."""
    N, C = int(x.shape[0]), int(x.shape[1])
    ia, ip, p_offset, lens = saved
    if with_scores:
        buf = torch.empty(N * (C + 1), dtype=torch.float32, device=x.device)
        gx, gs = buf[:N * C].view(N, C), buf[N * C:].view(N, 1)
    else:
        gx, gs, g_sa, g_sp = torch.empty((N, C), dtype=torch.float32, device=x.device), None, None, None
    cont = [g.contiguous() if g is not None else None for g in (g_a, g_p, g_sa, g_sp)]
    _native.check(_native.lib().d3f_select_normalize_backward(
        _p(x), N, C, _p(ia), _p(ip), stride, M, P, _p(p_offset), _p(lens), _p(cont[0]), _p(cont[1]), _p(cont[2]),
        _p(cont[3]), _p(gx), _p(gs), _stream()), "d3f_select_normalize_backward")
    return gx, gs


_LOSS_RECORDS = None     # tests: a dict here receives the records of the next ordered loss backward (its ``debug``)


def _loss_rows_bwd_ordered(x, saved, stride, P, M, g_a, g_p, g_sa, g_sp, with_scores=True, det=None, debug=None):
    """_select_rows_bwd (and, with ``det`` = (DetectorRows, fmax, aux), _det_rows_bwd on top of it) without float atomics,
    for the deterministic mode: every contribution is stored as a record, the record keys are sorted, and each element of
    the gradient is the float32 sum of its records in key order -- ascending sampled row (anchors, then positives), inside a
    row the normalisation's term, the detector's c* and c' terms, the neighbors by slot -- with the group's arg-max term
    last (d3f_loss_rows_backward_records / _apply).  Returns (grad_x [N,C], grad_scores [N,1] or None).  ``debug``: a dict
    that receives the records (key, val), their width and the arg-max terms (tests restate the sums from them)."""
    L = _native.lib()
    N, C = int(x.shape[0]), int(x.shape[1])
    ia, ip, p_offset, lens = saved
    rows = 2 * P * M
    if debug is None:
        debug = _LOSS_RECORDS
    if det is not None:
        rows_det, fmax, aux = det
        head, groups = _det_rows_args(x, rows_det, fmax, lens)
        H, with_scores = int(rows_det.neighbors.shape[1]), False
        n_groups = int(fmax.numel())
    else:
        head, groups, fmax, aux, H, n_groups = (_p(x), N, C, None, 0, None), (None, 0, 0), None, None, 0, 1
    R = int(L.d3f_loss_rows_record_width(C, H))
    key = torch.empty(rows * R, dtype=torch.int64, device=x.device)
    val = torch.empty(rows * R, dtype=torch.float32, device=x.device)
    nws = int(L.d3f_detection_rows_ws_bytes(rows))
    ws = _ws(nws, x.device)     # (part / pgroup of the first call are read by the second: ONE buffer)
    cont = [g.contiguous() if g is not None else None for g in (g_a, g_p, g_sa, g_sp)]
    if with_scores:
        buf = torch.empty(N * (C + 1), dtype=torch.float32, device=x.device)
        gx, gs = buf[:N * C].view(N, C), buf[N * C:].view(N, 1)
    else:
        gx, gs = torch.empty((N, C), dtype=torch.float32, device=x.device), None
    tie = torch.zeros(n_groups, dtype=torch.float32, device=x.device) if debug is not None else None
    _count('ordered')
    with _region("loss_rows_bwd_ordered[T=%d]" % (P * M)):
        feat, _, _, nb, _, fm = head
        g_len, g_b, g_group = groups
        _native.check(L.d3f_loss_rows_backward_records(
            feat, N, C, nb, H, fm, g_len, g_b, g_group, _p(ia), _p(ip), stride, M, P, _p(p_offset), _p(lens), _p(aux),
            _p(cont[0]), _p(cont[1]), _p(cont[2]), _p(cont[3]), 1 if with_scores else 0, _p(key), _p(val), _p(ws), nws,
            _stream()), "d3f_loss_rows_backward_records")
        skey = torch.sort(key)[0]       # (keys are unique: element * records + record index)
        _native.check(L.d3f_loss_rows_backward_apply(
            feat, N, C, H, fm, g_len, g_b, g_group, rows, 1 if det is not None else 0, 1 if with_scores else 0, _p(skey),
            _p(val), _p(gx), _p(tie), _p(ws), nws, _stream()), "d3f_loss_rows_backward_apply")
    if debug is not None:
        debug.update(key=key, val=val, width=R, tie_terms=tie, sorted_key=skey)
    return gx, gs


class _SelectNormalizeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scores, saved, stride):
        ctx.save_for_backward(x, *saved)
        ctx.stride, ctx.ordered = stride, _DETERMINISTIC
        return _select_normalize_fwd(x, scores, saved, stride, 1, int(saved[0].shape[0]))

    @staticmethod
    def backward(ctx, g_a, g_p, g_sa, g_sp):
        x, *saved = ctx.saved_tensors
        bwd = _loss_rows_bwd_ordered if ctx.ordered else _select_rows_bwd
        gx, gs = bwd(x, saved, ctx.stride, 1, int(saved[0].shape[0]), g_a, g_p, g_sa, g_sp)
        return gx, gs, None, None


def _p_offset(p_offset, device):
    if p_offset is None:
        return None
    off = p_offset if isinstance(p_offset, torch.Tensor) else torch.tensor([int(p_offset)], device=device)
    return off.reshape(-1)[:1].to(torch.int32).contiguous()


def select_normalize(x, scores, idx_a, idx_p, p_offset=None):
    """(normalize(x)[idx_a], normalize(x)[idx_p + p_offset], scores[idx_a], scores[idx_p + p_offset]) without
    normalising or differentiating through the other N - 2M rows.  idx_*: int64 [M] (the two columns of a [M,2] table
    are read in place); p_offset: device int32 scalar."""
    x = _f32(x, "x")
    sc = _f32(scores, "scores").reshape(-1, 1)
    return _SelectNormalizeFn.apply(x, sc, *_sampled_rows(idx_a, idx_p, _p_offset(p_offset, x.device)))


# ---------------------------------------------------------------------------------------------------------------
# contrastive + detector loss (utils/loss.py:47-97 with metric 'euclidean', :149-158; desc_loss 'contrastive')
# ---------------------------------------------------------------------------------------------------------------
def _dk64(dist_keypts, shape, device):
    dk = dist_keypts.to(device=device, dtype=torch.float64).contiguous()
    if tuple(dk.shape) != tuple(shape):
        raise ValueError("dist_keypts must be [%s], got %s" % (",".join(map(str, shape)), tuple(dk.shape)))
    return dk


def _contrastive_fwd(oa, op, sa, sp, dk, P, M, params, weights=(1.0, 1.0), with_total=False):
    """Forward launches on selected rows oa/op [P*M,C]: (scalars [P,6], total or None, dists, fp, an, stats)."""
    C = int(oa.shape[1])
    sr, pm, nm = params
    out = scalars, total, dists, fp, an, stats = _loss_outputs(oa, P, M, with_total)
    _native.check(_native.lib().d3f_contrastive_det_loss_forward(
        _p(oa), _p(op), M, C, P, _p(dk), _p(sa), _p(sp), sr, pm, nm, weights[0], weights[1], _p(dists), _p(fp), _p(an),
        _p(scalars), _p(total), _p(stats), _stream()), "d3f_contrastive_det_loss_forward")
    return out


def _contrastive_bwd(oa, op, sa, sp, stats, P, M, params, weights, g_ptrs):
    C = int(oa.shape[1])
    _, pm, nm = params
    ga, gp = torch.empty_like(oa), torch.empty_like(op)
    gsa, gsp = torch.empty_like(sa), torch.empty_like(sp)
    _native.check(_native.lib().d3f_contrastive_det_loss_backward(
        _p(oa), _p(op), M, C, P, _p(sa), _p(sp), pm, nm, weights[0], weights[1], _p(stats), g_ptrs[0], g_ptrs[1],
        _p(ga), _p(gp), _p(gsa), _p(gsp), _stream()), "d3f_contrastive_det_loss_backward")
    return ga, gp, gsa, gsp


class _ContrastiveDetFn(torch.autograd.Function):
    """Returns (scalars[6], dists[M,M], furthest_positive[M], average_negative[M]); scalars[0] = desc loss,
    scalars[1] = det loss are differentiable wrt anchor / positive / scores."""

    @staticmethod
    def forward(ctx, anchor, positive, dk, anc_score, pos_score, params):
        M = int(anchor.shape[0])
        scalars, _, dists, fp, an, stats = _contrastive_fwd(anchor, positive, anc_score, pos_score, dk, 1, M, params)
        scalars, dists = scalars.view(6), dists.view(M, M)
        ctx.save_for_backward(anchor, positive, anc_score, pos_score, stats)
        ctx.params = params
        ctx.mark_non_differentiable(dists, fp, an)
        ctx.set_materialize_grads(False)
        return scalars, dists, fp, an

    @staticmethod
    def backward(ctx, g_scalars, g_dists, g_fp, g_an):
        if g_scalars is None:
            return (None,) * 6
        anchor, positive, anc_score, pos_score, stats = ctx.saved_tensors
        g = g_scalars.contiguous().float()
        ga, gp, gsa, gsp = _contrastive_bwd(anchor, positive, anc_score, pos_score, stats, 1, int(anchor.shape[0]),
                                            ctx.params, (1.0, 1.0), (g.data_ptr(), g.data_ptr() + 4))
        return ga, gp, None, gsa, gsp, None


def contrastive_det_loss(anchor, positive, dist_keypts, anc_score, pos_score, safe_radius=0.1, pos_margin=0.1,
                         neg_margin=1.4):
    """The reference's ``ContrastiveLoss(pos_margin, neg_margin, 'euclidean', safe_radius)`` followed by ``DetLoss`` on
    its ``dists``, in two launches (d3f_contrastive_det_loss_forward).  ``dist_keypts`` [M,M] is read as float64.
    Returns (scalars[6] = desc, det, accuracy, mean furthest positive, mean average negative, desc + det;
    dists [M,M] with the +10s; furthest_positive [M]; average_negative [M]); desc and det carry gradient."""
    anchor, positive = _f32(anchor, "anchor"), _f32(positive, "positive")
    M = int(anchor.shape[0])
    if not 2 <= M <= 1024 or tuple(positive.shape) != tuple(anchor.shape) or not 1 <= int(anchor.shape[1]) <= 256:
        raise ValueError("anchor / positive must both be [M,C] with 2 <= M <= 1024, C <= 256")
    dk = _dk64(dist_keypts, (M, M), anchor.device)
    sa = _f32(anc_score, "anc_score").reshape(-1)
    sp = _f32(pos_score, "pos_score").reshape(-1)
    return _ContrastiveDetFn.apply(anchor, positive, dk, sa, sp,
                                   (float(safe_radius), float(pos_margin), float(neg_margin)))


# ---------------------------------------------------------------------------------------------------------------
# the whole loss of one training step (trainer.py:91-98) as ONE autograd node
# ---------------------------------------------------------------------------------------------------------------
def _det_rows_args(x, det, fmax, pair_lens):
    """Leading arguments of the d3f_detection_rows_* entries and their normaliser groups (len, B, group); stacked pairs
    hand their own lengths (group 0: one normaliser for all of them, as the dense form without groups)."""
    N, C, H = int(x.shape[0]), int(x.shape[1]), int(det.neighbors.shape[1])
    if int(det.neighbors.shape[0]) != N:
        raise ValueError("DetectorRows: the neighbor table must have one row per descriptor")
    lens = pair_lens if pair_lens is not None else (det.lens if det.group else None)
    if pair_lens is not None and det.group and (det.lens is None or det.lens.numel() != pair_lens.numel()):
        raise ValueError("DetectorRows: lens must be the stacked pairs' own level-0 lengths")
    if int(fmax.numel()) != (-(-int(lens.numel()) // det.group) if det.group else 1):
        raise ValueError("DetectorRows: one normaliser per group of clouds expected")
    return ((_p(x), N, C, _p(det.neighbors), H, _p(fmax)),
            (_p(lens), int(lens.numel()) if lens is not None else 0, det.group))


def _det_rows_fwd(x, det, fmax, saved, stride, P, M, sa, sp, want_aux):
    """Scores of the sampled rows into sa / sp; returns the compact aux [2 P M, 8] (None when no backward follows)."""
    ia, ip, p_offset, lens = saved
    head, groups = _det_rows_args(x, det, fmax, lens)
    aux = torch.empty((2 * P * M, 8), dtype=torch.float32, device=x.device) if want_aux else None
    with _region("detection_rows_fwd[T=%d]" % (P * M)):
        _native.check(_native.lib().d3f_detection_rows_forward(
            *head, 1 if det.training else 0, _p(det.width), *groups, _p(ia), _p(ip), stride, M, P, _p(p_offset),
            _p(lens), _p(sa), _p(sp), _p(aux), _stream()), "d3f_detection_rows_forward")
    return aux


def _det_rows_bwd(x, det, fmax, saved, stride, P, M, aux, gsa, gsp, gx):
    """Adds the detector's gradient of the sampled rows (and the normaliser's arg-max term) to ``gx``."""
    L = _native.lib()
    ia, ip, p_offset, lens = saved
    head, groups = _det_rows_args(x, det, fmax, lens)
    nws = int(L.d3f_detection_rows_ws_bytes(2 * P * M))
    ws = _ws(nws, x.device)
    with _region("detection_rows_bwd[T=%d]" % (P * M)):
        _native.check(L.d3f_detection_rows_backward(
            *head, *groups, _p(ia), _p(ip), stride, M, P, _p(p_offset), _p(lens), _p(aux), _p(gsa), _p(gsp), _p(gx),
            _p(ws), nws, _stream()), "d3f_detection_rows_backward")


class _TrainLossFn(torch.autograd.Function):
    """x [N,C] raw descriptors, scores [N,1], corr [P*M,2] -> (total, scalars [P,6], dists [P,M,M], furthest_positive
    [P*M], average_negative [P*M]) with total = sum over the pairs of w_desc * desc + w_det * det.  ``lens`` None: one
    pair with ``p_offset``; otherwise every pair's own cloud-local table and lens int32 [2P] on the device.
    Same kernels as select_normalize + circle_det_loss / contrastive_det_loss; what disappears is the autograd glue
    between them (index selects and their zero-filled backward, the weighted sum and its backward: ~12 sub-5-us launches
    per step).  ``aux``: the circle loss's neg_mask (uint8) or the contrastive loss's keypoint distances (f64),
    [M,M] / [P,M,M]; ``params`` = the loss's scalars, led by log_scale for the circle loss.
    ``gw``: (w_desc, w_det) on the device for the circle loss's one-workgroup route (one pair beyond M = 128 or C = 64),
    whose kernel knows no weights; None everywhere else.
    ``scores`` may be a ``DetectorRows`` instead of a tensor: the node then scores the sampled rows itself, is
    differentiable with respect to x only and returns the single merged grad_x (one fill, no dense score gradient)."""

    @staticmethod
    def forward(ctx, x, scores, corr, p_offset, lens, aux, circle, P, params, weights, gw):
        M = int(aux.shape[-1])
        det = scores if isinstance(scores, DetectorRows) else None
        oa, op, sa, sp, saved, stride = _select_rows_fwd(x, None if det else scores, corr, p_offset, lens, P, M)
        if det is not None:
            fmax = global_max(x, det.lens, det.group)
            ctx.det = (det, fmax, _det_rows_fwd(x, det, fmax, saved, stride, P, M, sa, sp,
                                                det.training and ctx.needs_input_grad[0]))
        else:
            ctx.det = None
        # the one-workgroup circle kernel knows no weights: unit weights (config.py:58-59) take its own desc + det
        # (scalars[5]; no launch for the sum), others go through ``gw``; every other form weights inside the kernel
        plain = circle and not _circle_tiled(M, int(x.shape[1]))
        if plain:
            scalars, _, dists, fp, an, stats = _circle_fwd(oa, op, sa, sp, aux, P, M, params)
            total = scalars[0, 5] if weights == (1.0, 1.0) else torch.dot(scalars[0, :2], gw)
        else:
            scalars, total, dists, fp, an, stats = (_circle_fwd if circle else _contrastive_fwd)(
                oa, op, sa, sp, aux, P, M, params, weights, True)
        ctx.save_for_backward(x, *saved, oa, op, sa, sp, stats, *((aux, dists, gw) if circle else ()))
        ctx.meta = (stride, circle, plain, P, M, params, weights)
        ctx.ordered = _DETERMINISTIC
        ctx.mark_non_differentiable(scalars, dists, fp, an)
        ctx.set_materialize_grads(False)   # (else four zero-fill launches per step for the by-products' gradients)
        return total, scalars, dists, fp, an

    @staticmethod
    def backward(ctx, g_total, g_scalars, g_dists, g_fp, g_an):
        if g_total is None:
            return (None,) * 11
        x, oa, op, sa, sp, stats = ctx.saved_tensors[:1] + ctx.saved_tensors[5:10]
        saved = ctx.saved_tensors[1:5]
        stride, circle, plain, P, M, params, weights = ctx.meta
        if plain and weights != (1.0, 1.0):
            g = (ctx.saved_tensors[12] * g_total).contiguous()
            g_ptrs, weights = (g.data_ptr(), g.data_ptr() + 4), (1.0, 1.0)
        else:      # d total / d desc = d total / d det = g_total: both pointers read the same scalar
            g = g_total.contiguous().float().reshape(1)
            g_ptrs = (g.data_ptr(), g.data_ptr())
        if circle:
            neg_mask, dists = ctx.saved_tensors[10:12]
            grads = _circle_bwd(oa, op, sa, sp, neg_mask, dists, stats, P, M, params, weights, g_ptrs)
        else:
            grads = _contrastive_bwd(oa, op, sa, sp, stats, P, M, params, weights, g_ptrs)
        if ctx.det is None:
            return (_loss_rows_bwd_ordered if ctx.ordered else _select_rows_bwd)(x, saved, stride, P, M, *grads) + \
                (None,) * 9
        det, fmax, aux8 = ctx.det
        if aux8 is None:
            raise RuntimeError("train loss: the detector's backward is defined for training mode only")
        if ctx.ordered:     # normalisation + detector + arg-max terms in ONE order-fixed sum per element
            gx, _ = _loss_rows_bwd_ordered(x, saved, stride, P, M, *grads, with_scores=False, det=ctx.det)
            return (gx,) + (None,) * 10
        _count('scatter')
        gx, _ = _select_rows_bwd(x, saved, stride, P, M, *grads, with_scores=False)
        _det_rows_bwd(x, det, fmax, saved, stride, P, M, aux8, grads[2], grads[3], gx)
        return (gx,) + (None,) * 10


def _loss_inputs(x, scores):
    """(x, scores [N,1]); a ``DetectorRows`` outside the rows form's domain becomes the dense scores here."""
    x = _f32(x, "x")
    if isinstance(scores, DetectorRows):
        if DetectorRows.supported(x.shape[1], scores.neighbors.shape[1]):
            return x, scores
        scores = detection_scores(x, scores.neighbors, scores.training, scores.lens, scores.width, scores.group)
    return x, _f32(scores, "scores").reshape(-1, 1)


def _train_loss(x, scores, corr, p_offset, lens, table, limit, circle, params, w_desc, w_det, gw_cache=None):
    """The four train_* front ends behind their own arguments.  ``lens`` None: one pair, corr int64 [M,2] with
    ``p_offset``; returns (total, desc, det, accuracy, furthest_positive [M], average_negative [M]).  Otherwise P stacked
    pairs, corr [P,M,2] / [P*M,2] and lens device int32 [2P]; desc, det, accuracy are [P], the two vectors [P,M].
    ``table(device, M)`` checks and returns the loss's neg_mask / keypoint distances (M None: stacked, its own [P,M,M]
    gives P and M); ``limit`` = (lowest M, highest M, highest C, message) or None."""
    x, sc = _loss_inputs(x, scores)
    if lens is None:
        if not (corr.is_cuda and corr.dtype == torch.int64 and corr.dim() == 2 and corr.shape[1] == 2):
            raise ValueError("corr must be an int64 [M,2] device tensor")
        P, M = 1, int(corr.shape[0])
        aux = table(x.device, M)
    else:
        aux = table(x.device, None)
        P, M = int(aux.shape[0]), int(aux.shape[1])
        if not (corr.is_cuda and corr.dtype == torch.int64 and corr.numel() == 2 * P * M and corr.shape[-1] == 2):
            raise ValueError("corr must be an int64 [P,M,2] device tensor (P = %d, M = %d)" % (P, M))
        if not (isinstance(lens, torch.Tensor) and lens.is_cuda and lens.dtype == torch.int32 and lens.numel() == 2 * P):
            raise ValueError("lens must hold the 2P level-0 stack lengths as device int32")
        lens = lens.contiguous()
    C = int(x.shape[1])
    if limit is not None and (not limit[0] <= M <= limit[1] or C > limit[2] or P > 32):
        raise ValueError(limit[3])
    weights, gw = (float(w_desc), float(w_det)), None
    if circle and not _circle_tiled(M, C) and weights != (1.0, 1.0):
        key = (x.device,) + weights
        if key not in gw_cache:
            gw_cache[key] = torch.tensor(weights, dtype=torch.float32, device=x.device)
        gw = gw_cache[key]
    total, scalars, dists, fp, an = _TrainLossFn.apply(x, sc, corr.contiguous().view(P * M, 2), _p_offset(p_offset, x.device),
                                                       lens, aux, circle, P, params, weights, gw)
    if lens is None:
        return total, scalars[0, 0], scalars[0, 1], scalars[0, 2], fp, an
    return total, scalars[:, 0], scalars[:, 1], scalars[:, 2], fp.view(P, M), an.view(P, M)


def train_loss(x, scores, corr, p_offset, dist_keypts, log_scale=10.0, safe_radius=0.1, pos_margin=0.1, neg_margin=1.4,
               w_desc=1.0, w_det=1.0, neg_mask=None, _gw_cache={}):
    """Loss of one training step on the un-normalised network output (trainer.py:91-98):
    ``w_desc * CircleLoss(normalize(x)[corr[:,0]], normalize(x)[corr[:,1] + p_offset]) + w_det * DetLoss(...)``.
    Returns (total, desc, det, accuracy, furthest_positive [M], average_negative [M]); only ``total`` carries
    gradient.  ``neg_mask``: ``dist_keypts > safe_radius`` as uint8 when the caller already has it (the pipelined step
    evaluates it with the pair's upload, off the training stream).  ``scores``: the [N,1] scores, or a ``DetectorRows``
    (here and in the three sibling forms): the detector then runs on the 2M sampled rows only, inside this node."""
    def table(device, M):
        if neg_mask is None:
            return _neg_mask_of(dist_keypts, safe_radius)
        if not (neg_mask.is_cuda and neg_mask.dtype == torch.uint8 and neg_mask.is_contiguous()
                and tuple(neg_mask.shape) == (M, M)):
            raise ValueError("neg_mask must be a contiguous uint8 [M,M] device tensor (dist_keypts > safe_radius)")
        return neg_mask

    return _train_loss(x, scores, corr, p_offset, None, table, None, True,
                       (float(log_scale), float(safe_radius), float(pos_margin), float(neg_margin)), w_desc, w_det,
                       _gw_cache)


def train_loss_pairs(x, scores, corr, lens, dist_keypts=None, log_scale=10.0, safe_radius=0.1, pos_margin=0.1,
                     neg_margin=1.4, w_desc=1.0, w_det=1.0, neg_mask=None):
    """Loss of one training step on P fragment pairs STACKED into one batch (clouds 2p, 2p+1 = pair p): per pair the
    reference's ``CircleLoss`` + ``DetLoss`` on its own M sampled correspondences (trainer.py:91-98; the reference
    trains one pair per step, dataloader.py:73), ``total`` = their sum -- its gradient is the sum of the pairs'
    gradients, the optimizer's gradient scale makes the mean.  ``corr`` int64 [P,M,2] / [P*M,2] cloud-local rows as the
    dataset yields them, ``lens`` device int32 [2P] (level-0 stack lengths), ``dist_keypts`` [P,M,M] or ``neg_mask``
    uint8 [P,M,M] = dist_keypts > safe_radius.  Three launches forward (select + normalise, strips of all pairs,
    finalize), two backward.
    Returns (total, desc [P], det [P], accuracy [P], furthest_positive [P,M], average_negative [P,M])."""
    def table(device, _):
        mask = _neg_mask_of(dist_keypts, safe_radius) if neg_mask is None else neg_mask
        if not (mask.is_cuda and mask.dtype == torch.uint8 and mask.is_contiguous() and mask.dim() == 3
                and mask.shape[1] == mask.shape[2]):
            raise ValueError("neg_mask must be a contiguous uint8 [P,M,M] device tensor (dist_keypts > safe_radius)")
        return mask

    return _train_loss(x, scores, corr, None, lens, table,
                       (0, 128, 64, "stacked loss: M <= 128 correspondences, C <= 64 channels, P <= 32 pairs"), True,
                       (float(log_scale), float(safe_radius), float(pos_margin), float(neg_margin)), w_desc, w_det)


def train_contrastive_loss(x, scores, corr, p_offset, dist_keypts, safe_radius=0.1, pos_margin=0.1, neg_margin=1.4,
                           w_desc=1.0, w_det=1.0):
    """``train_loss`` with the reference's desc_loss 'contrastive' (training_3DMatch.py:119-125):
    ``w_desc * ContrastiveLoss(normalize(x)[corr[:,0]], normalize(x)[corr[:,1] + p_offset], dist_keypts) + w_det *
    DetLoss(dists, ...)``.  Returns (total, desc, det, accuracy, furthest_positive [M], average_negative [M]); only
    ``total`` carries gradient."""
    def table(device, M):
        return _dk64(dist_keypts, (1, M, M) if dist_keypts.dim() == 3 else (M, M), device)

    return _train_loss(x, scores, corr, p_offset, None, table,
                       (2, 1024, 256, "contrastive loss: 2 <= M <= 1024 correspondences, C <= 256 channels"), False,
                       (float(safe_radius), float(pos_margin), float(neg_margin)), w_desc, w_det)


def train_contrastive_loss_pairs(x, scores, corr, lens, dist_keypts, safe_radius=0.1, pos_margin=0.1, neg_margin=1.4,
                                 w_desc=1.0, w_det=1.0):
    """``train_loss_pairs`` with the contrastive loss: P stacked pairs, ``dist_keypts`` [P,M,M] (read as float64),
    total = sum_p (w_desc desc_p + w_det det_p).
    Returns (total, desc [P], det [P], accuracy [P], furthest_positive [P,M], average_negative [P,M])."""
    def table(device, _):
        if dist_keypts.dim() != 3 or dist_keypts.shape[1] != dist_keypts.shape[2]:
            raise ValueError("dist_keypts must be [P,M,M]")
        return _dk64(dist_keypts, tuple(dist_keypts.shape), device)

    return _train_loss(x, scores, corr, None, lens, table,
                       (2, 1024, 256, "stacked contrastive loss: 2 <= M <= 1024, C <= 256 channels, P <= 32 pairs"), False,
                       (float(safe_radius), float(pos_margin), float(neg_margin)), w_desc, w_det)


# ---------------------------------------------------------------------------------------------------------------
# dense mutual-NN matching (geometric_registration/common.py:5-21)
# ---------------------------------------------------------------------------------------------------------------
def mutual_nn(source_desc, target_desc):
    """(row_argmin [Ns], col_argmin [Nt], mutual [Ns]) int32 device tensors."""
    s, t = _f32(source_desc, "source_desc"), _f32(target_desc, "target_desc")
    Ns, Nt, C = int(s.shape[0]), int(t.shape[0]), int(s.shape[1])
    ra = torch.empty(Ns, dtype=torch.int32, device=s.device)
    ca = torch.empty(Nt, dtype=torch.int32, device=s.device)
    mu = torch.empty(Ns, dtype=torch.int32, device=s.device)
    nbytes = _native.lib().d3f_mutual_nn_ws_bytes(Ns, Nt)
    ws = _ws(nbytes, s.device)
    _native.check(_native.lib().d3f_mutual_nn(_p(s), Ns, _p(t), Nt, C, _p(ra), _p(ca), _p(mu), _p(ws), nbytes,
                                              _stream()), "d3f_mutual_nn")
    return ra, ca, mu


def mutual_nn_batched(source_desc, target_desc, seg, max_src, max_tgt):
    """P matchings by one pair of launches.  ``seg`` int32 [P,4] on the device = (src_off, src_len, tgt_off, tgt_len) per
    pair into the rows of the (possibly identical) stacked descriptor matrices; ``max_src`` / ``max_tgt`` host upper
    bounds of the lengths.  Returns (row_argmin [src rows], col_argmin [tgt rows], mutual [src rows]) indexed by stacked
    row, holding pair-local indices; rows outside every segment hold -1 / 0."""
    s, t = _f32(source_desc, "source_desc"), _f32(target_desc, "target_desc")
    if not (seg.is_cuda and seg.dtype == torch.int32 and seg.dim() == 2 and seg.shape[1] == 4 and seg.is_contiguous()):
        raise ValueError("seg must be a contiguous device int32 [P,4] tensor")
    Ns, Nt, C, P = int(s.shape[0]), int(t.shape[0]), int(s.shape[1]), int(seg.shape[0])
    ra = torch.full((Ns,), -1, dtype=torch.int32, device=s.device)
    ca = torch.full((Nt,), -1, dtype=torch.int32, device=s.device)
    mu = torch.zeros(Ns, dtype=torch.int32, device=s.device)
    nbytes = _native.lib().d3f_mutual_nn_batched_ws_bytes(Ns, Nt)
    ws = _ws(nbytes, s.device)
    _native.check(_native.lib().d3f_mutual_nn_batched(_p(s), Ns, _p(t), Nt, _p(seg), P, int(max_src), int(max_tgt), C,
                                                      _p(ra), _p(ca), _p(mu), _p(ws), nbytes, _stream()),
                  "d3f_mutual_nn_batched")
    return ra, ca, mu


KNN_MAX = _native.D3F_KNN_MAX


def _knn_k(k):
    if not 1 <= int(k) <= KNN_MAX:
        raise ValueError("k must be in 1..%d" % KNN_MAX)
    return int(k)


def knn_match(source_desc, target_desc, k):
    """(idx int32 [Ns,k], dist f32 [Ns,k]): the k nearest target descriptors of every source descriptor by the rule of
    csrc/knn_match.hpp -- ascending (float32 distance sqrt(2 - 2 S T^T), target index), a NaN distance first like
    ``np.argmin``; slots beyond Nt hold -1 / +inf.  ``idx[:, 0]`` is ``mutual_nn``'s row arg-min."""
    s, t = _f32(source_desc, "source_desc"), _f32(target_desc, "target_desc")
    Ns, Nt, C, k = int(s.shape[0]), int(t.shape[0]), int(s.shape[1]), _knn_k(k)
    idx = torch.empty((Ns, k), dtype=torch.int32, device=s.device)
    dist = torch.empty((Ns, k), dtype=torch.float32, device=s.device)
    nbytes = _native.lib().d3f_knn_match_ws_bytes(Ns, Nt, k)
    ws = _ws(nbytes, s.device)
    _native.check(_native.lib().d3f_knn_match(_p(s), Ns, _p(t), Nt, C, k, _p(idx), _p(dist), _p(ws), nbytes, _stream()),
                  "d3f_knn_match")
    return idx, dist


def knn_match_batched(source_desc, target_desc, seg, max_src, max_tgt, k):
    """P ``knn_match`` problems by one pair of launches; ``seg`` / ``max_src`` / ``max_tgt`` as in ``mutual_nn_batched``.
    Returns (idx [src rows,k], dist [src rows,k]) indexed by stacked source row, holding pair-local indices; rows outside
    every segment and the rows of a pair with an empty target hold -1 / +inf."""
    s, t = _f32(source_desc, "source_desc"), _f32(target_desc, "target_desc")
    if not (seg.is_cuda and seg.dtype == torch.int32 and seg.dim() == 2 and seg.shape[1] == 4 and seg.is_contiguous()):
        raise ValueError("seg must be a contiguous device int32 [P,4] tensor")
    Ns, Nt, C, P, k = int(s.shape[0]), int(t.shape[0]), int(s.shape[1]), int(seg.shape[0]), _knn_k(k)
    idx = torch.full((Ns, k), -1, dtype=torch.int32, device=s.device)
    dist = torch.full((Ns, k), float('inf'), dtype=torch.float32, device=s.device)
    nbytes = _native.lib().d3f_knn_match_batched_ws_bytes(Ns, P, int(max_src), int(max_tgt), k)
    ws = _ws(nbytes, s.device)
    _native.check(_native.lib().d3f_knn_match_batched(_p(s), Ns, _p(t), Nt, _p(seg), P, int(max_src), int(max_tgt), C, k,
                                                      _p(idx), _p(dist), _p(ws), nbytes, _stream()),
                  "d3f_knn_match_batched")
    return idx, dist


TOPK_MAX = _native.D3F_TOPK_MAX


def topk_scores(scores, seg, k):
    """int32 [P,k]: the k highest-scoring rows of every cloud (cloud-local indices), ascending (score, index) like the
    tail of a stable argsort (test.py:56-57); ``seg`` int32 [P,2] on the device = (offset, length) per cloud; a cloud
    with fewer than k rows leads with -1."""
    sc = _f32(scores, "scores").reshape(-1)
    if not (seg.is_cuda and seg.dtype == torch.int32 and seg.dim() == 2 and seg.shape[1] == 2 and seg.is_contiguous()):
        raise ValueError("seg must be a contiguous device int32 [P,2] tensor")
    if not 1 <= int(k) <= TOPK_MAX:
        raise ValueError("k must be in 1..%d" % TOPK_MAX)
    out = torch.empty((int(seg.shape[0]), int(k)), dtype=torch.int32, device=sc.device)
    _native.check(_native.lib().d3f_topk_scores(_p(sc), int(sc.numel()), _p(seg), int(seg.shape[0]), int(k), _p(out),
                                                _stream()), "d3f_topk_scores")
    return out


# ---------------------------------------------------------------------------------------------------------------
# rigid registration (what the reference leaves to Open3D's RANSAC on the CPU)
# ---------------------------------------------------------------------------------------------------------------
RANSAC_MAX_HYPOTHESES = _native.D3F_RANSAC_MAX_HYPOTHESES
RANSAC_MAX_COUNT = _native.D3F_RANSAC_MAX_COUNT
RANSAC_MAX_REFINE = _native.D3F_RANSAC_MAX_REFINE
RANSAC_ST_FEW, RANSAC_ST_NO_HYPOTHESIS = _native.D3F_RANSAC_ST_FEW, _native.D3F_RANSAC_ST_NO_HYPOTHESIS
RANSAC_ST_SEGMENT = _native.D3F_RANSAC_ST_SEGMENT


def ransac_rigid(src, tgt, seg, num_hypotheses=50000, distance_threshold=0.05, edge_ratio=0.9, refine_iters=3, seed=0,
                 return_hypotheses=False, first_pair=0):
    """RANSAC rigid registration of P correspondence sets in two launches (d3f_ransac_rigid).

    ``src`` / ``tgt`` [rows,3] (row i of one matches row i of the other); ``seg`` int32 [P,2] on the device =
    (offset, count) per pair.  Returns device tensors ``(T [P,4,4] f64, inliers [P], best_hypothesis [P],
    best_count [P], status [P])``: T maps the TARGET onto the SOURCE (src ~ R tgt + t, the gt.log convention) and is the
    identity where ``status`` is non-zero (RANSAC_ST_* bits).  ``return_hypotheses=True`` appends every hypothesis'
    inlier count [P,H] int32 (-1 when invalid) and f32 (R row-major, t) [P,H,12].  ``first_pair``: the hash index of
    pair 0 (a batch split over several calls draws what one call would)."""
    s, t = _f32(src, "src"), _f32(tgt, "tgt")
    if s.dim() != 2 or s.shape[1] != 3 or tuple(t.shape) != tuple(s.shape):
        raise ValueError("src and tgt must be [rows,3] tensors of the same shape")
    if not (isinstance(seg, torch.Tensor) and seg.is_cuda and seg.dtype == torch.int32 and seg.dim() == 2
            and seg.shape[1] == 2 and seg.shape[0] >= 1 and seg.is_contiguous()):
        raise ValueError("seg must be a contiguous device int32 [P,2] tensor")
    H, P = int(num_hypotheses), int(seg.shape[0])
    if not 1 <= H <= RANSAC_MAX_HYPOTHESES:
        raise ValueError("num_hypotheses must be in 1..%d" % RANSAC_MAX_HYPOTHESES)
    if not 0 <= int(refine_iters) <= RANSAC_MAX_REFINE:
        raise ValueError("refine_iters must be in 0..%d" % RANSAC_MAX_REFINE)
    if not (0.0 <= float(edge_ratio) <= 1.0) or not (0.0 < float(distance_threshold) < float("inf")):
        raise ValueError("edge_ratio must be in [0, 1] and distance_threshold positive")
    dev = s.device
    T = torch.empty((P, 4, 4), dtype=torch.float64, device=dev)
    out = [torch.empty(P, dtype=torch.int32, device=dev) for _ in range(4)]
    hc = torch.empty((P, H), dtype=torch.int32, device=dev) if return_hypotheses else None
    hr = torch.empty((P, H, 12), dtype=torch.float32, device=dev) if return_hypotheses else None
    nbytes = _native.lib().d3f_ransac_rigid_ws_bytes(P, H)
    ws = _ws(nbytes, dev)
    _native.check(_native.lib().d3f_ransac_rigid(
        _p(s), _p(t), int(s.shape[0]), _p(seg), P, int(first_pair), H, float(distance_threshold), float(edge_ratio),
        int(refine_iters), int(seed) & 0xffffffffffffffff, _p(T), _p(out[0]), _p(out[1]), _p(out[2]), _p(out[3]),
        _p(hc), _p(hr), _p(ws), nbytes, _stream()), "d3f_ransac_rigid")
    res = (T,) + tuple(out)
    return res + (hc, hr) if return_hypotheses else res


# fast global registration: the RANSAC-free estimator on the same correspondences (csrc/fgr.hpp has the rule)
FGR_MAX_PAIRS = _native.D3F_FGR_MAX_PAIRS
FGR_MAX_ITERS = _native.D3F_FGR_MAX_ITERS
FGR_MAX_TRIALS = _native.D3F_FGR_MAX_TRIALS
FGR_ST_FEW, FGR_ST_SINGULAR = _native.D3F_FGR_ST_FEW, _native.D3F_FGR_ST_SINGULAR
FGR_ST_SEGMENT, FGR_ST_NONFINITE = _native.D3F_FGR_ST_SEGMENT, _native.D3F_FGR_ST_NONFINITE


def _fgr_scalars(P, distance_threshold, iterations, division_factor, anneal_every, tuple_scale, tuple_trials,
                 max_tuples, seed, first_pair):
    """The checked scalar arguments of d3f_fgr_rigid / d3f_fgr_rigid_host, in the header's order."""
    if not 1 <= P <= FGR_MAX_PAIRS:
        raise ValueError("seg must hold 1..%d pairs" % FGR_MAX_PAIRS)
    if not 1 <= int(iterations) <= FGR_MAX_ITERS:
        raise ValueError("iterations must be in 1..%d" % FGR_MAX_ITERS)
    if not (0.0 < float(distance_threshold) < float("inf")):
        raise ValueError("distance_threshold must be positive and finite")
    if not (1.0 < float(division_factor) < float("inf")) or int(anneal_every) < 1:
        raise ValueError("division_factor must be > 1 and anneal_every at least 1")
    if not (0.0 < float(tuple_scale) <= 1.0):
        raise ValueError("tuple_scale must be in (0, 1]")
    trials = -1 if tuple_trials is None else int(tuple_trials)
    if not -1 <= trials <= FGR_MAX_TRIALS or int(max_tuples) < 0 or int(first_pair) < 0:
        raise ValueError("tuple_trials must be None or in 0..%d, max_tuples and first_pair non-negative" % FGR_MAX_TRIALS)
    return (int(first_pair), float(distance_threshold), int(iterations), float(division_factor), int(anneal_every),
            float(tuple_scale), trials, int(max_tuples), int(seed) & 0xffffffffffffffff)


def fgr_rigid(src, tgt, seg, distance_threshold=0.05, iterations=128, division_factor=1.4, anneal_every=4,
              tuple_scale=0.95, tuple_trials=None, max_tuples=1000, seed=0, first_pair=0, return_debug=False):
    """Fast global registration of P correspondence sets in one launch (d3f_fgr_rigid; csrc/fgr.hpp has the rule).

    ``src`` / ``tgt`` / ``seg`` as in ``ransac_rigid`` (the segments must not overlap).  Returns device tensors
    ``(T [P,4,4] f64, inliers [P], tuples [P], weight_sum [P] f64, status [P])``: T maps the TARGET onto the SOURCE and
    is the identity where ``status`` has FGR_ST_FEW, FGR_ST_SEGMENT or FGR_ST_NONFINITE; ``inliers`` counts ALL
    correspondences within ``distance_threshold`` under T, the number ``ransac_rigid`` reports.  ``tuple_trials``: None
    = min(100 count, FGR_MAX_TRIALS) per pair, 0 = no tuple test (then the result does not depend on ``seed``).
    ``return_debug=True`` appends ``multiplicity [rows] int32`` (0 for rows of no segment) and ``trace [P, iterations,
    8] f64`` = (mu, weight_sum, omega, v) per iteration, NaN for iterations that did not run."""
    s, t = _f32(src, "src"), _f32(tgt, "tgt")
    if s.dim() != 2 or s.shape[1] != 3 or tuple(t.shape) != tuple(s.shape):
        raise ValueError("src and tgt must be [rows,3] tensors of the same shape")
    if not (isinstance(seg, torch.Tensor) and seg.is_cuda and seg.dtype == torch.int32 and seg.dim() == 2
            and seg.shape[1] == 2 and seg.shape[0] >= 1 and seg.is_contiguous()):
        raise ValueError("seg must be a contiguous device int32 [P,2] tensor")
    P, rows = int(seg.shape[0]), int(s.shape[0])
    scalars = _fgr_scalars(P, distance_threshold, iterations, division_factor, anneal_every, tuple_scale, tuple_trials,
                           max_tuples, seed, first_pair)
    dev = s.device
    T = torch.empty((P, 4, 4), dtype=torch.float64, device=dev)
    inl, tup, st = (torch.empty(P, dtype=torch.int32, device=dev) for _ in range(3))
    wsum = torch.empty(P, dtype=torch.float64, device=dev)
    mult = torch.zeros(rows, dtype=torch.int32, device=dev) if return_debug else None
    trace = torch.full((P, int(iterations), 8), float("nan"), dtype=torch.float64, device=dev) if return_debug else None
    nbytes = _native.lib().d3f_fgr_rigid_ws_bytes(rows)
    ws = _ws(nbytes, dev)
    _native.check(_native.lib().d3f_fgr_rigid(
        _p(s), _p(t), rows, _p(seg), P, scalars[0], scalars[1], scalars[2], scalars[3], scalars[4], scalars[5],
        scalars[6], scalars[7], scalars[8], _p(T), _p(inl), _p(tup), _p(wsum), _p(st), _p(mult), _p(trace), _p(ws),
        nbytes, _stream()), "d3f_fgr_rigid")
    res = (T, inl, tup, wsum, st)
    return res + (mult, trace) if return_debug else res


def fgr_rigid_host(src, tgt, seg, distance_threshold=0.05, iterations=128, division_factor=1.4, anneal_every=4,
                   tuple_scale=0.95, tuple_trials=None, max_tuples=1000, seed=0, first_pair=0, return_debug=False):
    """The host twin of ``fgr_rigid`` (d3f_fgr_rigid_host): the same rule compiled for the CPU, one thread, the same
    summation order.  ``src`` / ``tgt`` / ``seg`` are host arrays (or CPU tensors); returns CPU tensors.  No GPU
    call."""
    s, t, g = _host_array(src), _host_array(tgt), _host_array(seg)
    if s.dtype != np.float32 or t.dtype != np.float32:
        raise ValueError("src and tgt must be float32")
    s, t = np.ascontiguousarray(s), np.ascontiguousarray(t)
    if s.ndim != 2 or s.shape[1] != 3 or t.shape != s.shape:
        raise ValueError("src and tgt must be [rows,3] arrays of the same shape")
    if g.dtype != np.int32 or g.ndim != 2 or g.shape[1] != 2 or g.shape[0] < 1:
        raise ValueError("seg must be an int32 [P,2] array")
    g = np.ascontiguousarray(g)
    P, rows, K = int(g.shape[0]), int(s.shape[0]), int(iterations)
    scalars = _fgr_scalars(P, distance_threshold, iterations, division_factor, anneal_every, tuple_scale, tuple_trials,
                           max_tuples, seed, first_pair)
    T = np.zeros((P, 4, 4), dtype=np.float64)
    inl, tup, st = (np.zeros(P, dtype=np.int32) for _ in range(3))
    wsum = np.zeros(P, dtype=np.float64)
    mult = np.zeros(rows, dtype=np.int32) if return_debug else None
    trace = np.full((P, K, 8), np.nan, dtype=np.float64) if return_debug else None
    _native.check(_native.lib().d3f_fgr_rigid_host(
        s.ctypes.data if rows else None, t.ctypes.data if rows else None, rows, g.ctypes.data, P, scalars[0], scalars[1],
        scalars[2], scalars[3], scalars[4], scalars[5], scalars[6], scalars[7], scalars[8], T.ctypes.data,
        inl.ctypes.data, tup.ctypes.data, wsum.ctypes.data, st.ctypes.data,
        mult.ctypes.data if return_debug else None, trace.ctypes.data if return_debug else None), "d3f_fgr_rigid_host")
    res = tuple(torch.from_numpy(x) for x in (T, inl, tup, wsum, st))
    return res + (torch.from_numpy(mult), torch.from_numpy(trace)) if return_debug else res


# spatial compatibility of second order: the estimator without sampling (csrc/sc2.hpp has the rule)
SC2_MAX_COUNT = _native.D3F_SC2_MAX_COUNT
SC2_MAX_SET = _native.D3F_SC2_MAX_SET
SC2_MAX_SEEDS = _native.D3F_SC2_MAX_SEEDS
SC2_ST_FEW, SC2_ST_NO_HYPOTHESIS = _native.D3F_SC2_ST_FEW, _native.D3F_SC2_ST_NO_HYPOTHESIS
SC2_ST_SEGMENT = _native.D3F_SC2_ST_SEGMENT


def _sc2_scalars(P, rows, max_count, distance_threshold, compat_threshold, num_seeds, set_size, refine_iters):
    """The checked scalar arguments of d3f_sc2_rigid / d3f_sc2_rigid_host, in the header's order."""
    if not 1 <= P <= 65535:
        raise ValueError("seg must hold 1..65535 pairs")
    mc = max(1, min(rows, SC2_MAX_COUNT)) if max_count is None else int(max_count)
    if not 1 <= mc <= SC2_MAX_COUNT:
        raise ValueError("max_count must be in 1..%d" % SC2_MAX_COUNT)
    if not (0.0 < float(distance_threshold) < float("inf")) or not (0.0 < float(compat_threshold) < float("inf")):
        raise ValueError("distance_threshold and compat_threshold must be positive and finite")
    if not 1 <= int(num_seeds) <= SC2_MAX_SEEDS:
        raise ValueError("num_seeds must be in 1..%d" % SC2_MAX_SEEDS)
    if not 3 <= int(set_size) <= SC2_MAX_SET:
        raise ValueError("set_size must be in 3..%d" % SC2_MAX_SET)
    if not 0 <= int(refine_iters) <= RANSAC_MAX_REFINE:
        raise ValueError("refine_iters must be in 0..%d" % RANSAC_MAX_REFINE)
    return mc, float(distance_threshold), float(compat_threshold), int(num_seeds), int(set_size), int(refine_iters)


def sc2_rigid(src, tgt, seg, distance_threshold=0.05, compat_threshold=0.1, num_seeds=256, set_size=20, refine_iters=3,
              max_count=None, max_bytes=2 << 30, return_debug=False, _poison_ws=False):
    """Spatial-compatibility (SC2) pose estimation of P correspondence sets in four launches (d3f_sc2_rigid; csrc/sc2.hpp
    has the rule): no sampling, no seed.

    ``src`` / ``tgt`` / ``seg`` as in ``ransac_rigid`` (the segments must not overlap).  Returns device tensors ``(T
    [P,4,4] f64, inliers [P], best_seed [P], best_count [P], status [P])``: T maps the TARGET onto the SOURCE and is the
    identity where ``status`` is non-zero (SC2_ST_* bits); ``best_seed`` is the winning seed's row inside its pair.
    ``max_count``: the longest segment the call takes (None: min(rows, SC2_MAX_COUNT)); the bit matrices cost
    ``max_count * ceil(max_count / 64) * 8`` bytes per pair.  When the workspace of all P pairs exceeds ``max_bytes`` the
    pairs are processed in slices of ``seg`` (device slices, no read-back) and the outputs concatenated: the same bits as
    one call.  One pair that alone exceeds ``max_bytes`` raises ``ValueError``.
    ``return_debug=True`` appends ``degree [rows] int32`` (0 for rows of no segment), ``seed_rows [P,num_seeds]``,
    ``consensus [P,num_seeds,set_size]``, ``hyp_count [P,num_seeds]``, ``hyp_rt [P,num_seeds,12] f32`` and the bit
    matrices ``int64 [P, max_count, W]`` -- a view of the workspace (of the slices' workspaces, concatenated, when the
    call was sliced)."""
    s, t = _f32(src, "src"), _f32(tgt, "tgt")
    if s.dim() != 2 or s.shape[1] != 3 or tuple(t.shape) != tuple(s.shape):
        raise ValueError("src and tgt must be [rows,3] tensors of the same shape")
    if not (isinstance(seg, torch.Tensor) and seg.is_cuda and seg.dtype == torch.int32 and seg.dim() == 2
            and seg.shape[1] == 2 and seg.shape[0] >= 1 and seg.is_contiguous()):
        raise ValueError("seg must be a contiguous device int32 [P,2] tensor")
    P, rows = int(seg.shape[0]), int(s.shape[0])
    mc, dt, ct, S, K, iters = _sc2_scalars(P, rows, max_count, distance_threshold, compat_threshold, num_seeds, set_size,
                                           refine_iters)
    L = _native.lib()
    if L.d3f_sc2_rigid_ws_bytes(1, mc, S) > int(max_bytes):
        raise ValueError("one pair needs %d bytes of workspace at max_count=%d, more than max_bytes=%d"
                         % (L.d3f_sc2_rigid_ws_bytes(1, mc, S), mc, int(max_bytes)))
    step = P
    while L.d3f_sc2_rigid_ws_bytes(step, mc, S) > int(max_bytes):      # the parts are aligned: no closed form
        step = (step + 1) // 2
    dev, W = s.device, (mc + 63) // 64
    T = torch.empty((P, 4, 4), dtype=torch.float64, device=dev)
    out = [torch.empty(P, dtype=torch.int32, device=dev) for _ in range(4)]
    deg = sr = cons = hc = hr = None
    mats = []
    if return_debug:
        deg = torch.zeros(rows, dtype=torch.int32, device=dev)
        sr = torch.empty((P, S), dtype=torch.int32, device=dev)
        cons = torch.empty((P, S, K), dtype=torch.int32, device=dev)
        hc = torch.empty((P, S), dtype=torch.int32, device=dev)
        hr = torch.empty((P, S, 12), dtype=torch.float32, device=dev)
    for a in range(0, P, step):
        b = min(a + step, P)
        nbytes = L.d3f_sc2_rigid_ws_bytes(b - a, mc, S)
        ws = _ws(nbytes, dev)
        if _poison_ws:
            ws.fill_(0xFF)
        _native.check(L.d3f_sc2_rigid(
            _p(s), _p(t), rows, _p(seg[a:b]), b - a, mc, dt, ct, S, K, iters, _p(T[a:b]), _p(out[0][a:b]),
            _p(out[1][a:b]), _p(out[2][a:b]), _p(out[3][a:b]), _p(deg), _p(sr[a:b]) if return_debug else None,
            _p(cons[a:b]) if return_debug else None, _p(hc[a:b]) if return_debug else None,
            _p(hr[a:b]) if return_debug else None, _p(ws), nbytes, _stream()), "d3f_sc2_rigid")
        if return_debug:
            mats.append(ws[:8 * (b - a) * mc * W].view(torch.int64).view(b - a, mc, W))
    res = (T,) + tuple(out)
    if return_debug:
        res = res + (deg, sr, cons, hc, hr, mats[0] if len(mats) == 1 else torch.cat(mats))
    return res


def sc2_rigid_host(src, tgt, seg, distance_threshold=0.05, compat_threshold=0.1, num_seeds=256, set_size=20,
                   refine_iters=3, max_count=None, return_debug=False):
    """The host twin of ``sc2_rigid`` (d3f_sc2_rigid_host): the same rule compiled for the CPU, one thread.  ``src`` /
    ``tgt`` / ``seg`` are host arrays (or CPU tensors); returns CPU tensors, with ``return_debug`` the same extra
    outputs as ``sc2_rigid``.  No GPU call."""
    s, t, g = _host_array(src), _host_array(tgt), _host_array(seg)
    if s.dtype != np.float32 or t.dtype != np.float32:
        raise ValueError("src and tgt must be float32")
    s, t = np.ascontiguousarray(s), np.ascontiguousarray(t)
    if s.ndim != 2 or s.shape[1] != 3 or t.shape != s.shape:
        raise ValueError("src and tgt must be [rows,3] arrays of the same shape")
    if g.dtype != np.int32 or g.ndim != 2 or g.shape[1] != 2 or g.shape[0] < 1:
        raise ValueError("seg must be an int32 [P,2] array")
    g = np.ascontiguousarray(g)
    P, rows = int(g.shape[0]), int(s.shape[0])
    mc, dt, ct, S, K, iters = _sc2_scalars(P, rows, max_count, distance_threshold, compat_threshold, num_seeds, set_size,
                                           refine_iters)
    T = np.zeros((P, 4, 4), dtype=np.float64)
    out = [np.zeros(P, dtype=np.int32) for _ in range(4)]
    dbg = []
    if return_debug:
        dbg = [np.zeros(rows, dtype=np.int32), np.zeros((P, S), dtype=np.int32), np.zeros((P, S, K), dtype=np.int32),
               np.zeros((P, S), dtype=np.int32), np.zeros((P, S, 12), dtype=np.float32),
               np.zeros((P, mc, (mc + 63) // 64), dtype=np.int64)]
    ptr = [x.ctypes.data for x in dbg] if return_debug else [None] * 6
    _native.check(_native.lib().d3f_sc2_rigid_host(
        s.ctypes.data if rows else None, t.ctypes.data if rows else None, rows, g.ctypes.data, P, mc, dt, ct, S, K, iters,
        T.ctypes.data, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, out[3].ctypes.data, ptr[0], ptr[1],
        ptr[2], ptr[3], ptr[4], ptr[5]), "d3f_sc2_rigid_host")
    return tuple(torch.from_numpy(x) for x in [T] + out + dbg)


# ---------------------------------------------------------------------------------------------------------------
# training items from a device-resident split (datasets.ThreeDMatch.ThreeDMatchResident)
# ---------------------------------------------------------------------------------------------------------------
AUGMENT_MAX_JOBS = _native.D3F_AUGMENT_MAX_JOBS
AUGMENT_MAX_NODE = _native.D3F_AUGMENT_MAX_NODE
# one item: rows of its clouds in the packed point store, rows of its table in the packed correspondence store, the
# target's rigid transform (R [3,3], t [3]; float64) and the 64-bit item key
AugmentJob = collections.namedtuple('AugmentJob', 'src_off src_len tgt_off tgt_len corr_off corr_len R t key')


def augment_pairs(points, corr, jobs, num_node, noise):
    """Up to 16 training items in one call of two launches (d3f_augment_pairs; arithmetic in csrc/augment.hpp).

    ``points`` f32 [sumN,3] and ``corr`` int32 [sumM,2] are the packed device stores, ``jobs`` a sequence of
    ``AugmentJob``.  Returns one ``(pts0 f32 [n0,3], pts1 f32 [n1,3], sel_corr int64 [m,2], dist_keypts f64 [m,m])`` per
    job, m = min(corr_len, num_node), launched on the current stream (no copy, no host synchronisation)."""
    if not (isinstance(points, torch.Tensor) and points.is_cuda and points.dtype == torch.float32 and points.dim() == 2
            and points.shape[1] == 3 and points.is_contiguous()):
        raise RuntimeError("points must be a contiguous CUDA/HIP float32 [sumN,3] tensor (no CPU path)")
    if not (isinstance(corr, torch.Tensor) and corr.is_cuda and corr.dtype == torch.int32 and corr.dim() == 2
            and corr.shape[1] == 2 and corr.is_contiguous()):
        raise RuntimeError("corr must be a contiguous CUDA/HIP int32 [sumM,2] tensor (no CPU path)")
    B, k = len(jobs), int(num_node)
    if not 1 <= B <= AUGMENT_MAX_JOBS:
        raise ValueError("1..%d jobs per call" % AUGMENT_MAX_JOBS)
    if not 1 <= k <= AUGMENT_MAX_NODE:
        raise ValueError("num_node must be in 1..%d" % AUGMENT_MAX_NODE)
    dev = points.device
    arr = (_native.AugmentJob * B)()
    out = []
    for q, j in zip(arr, jobs):
        if int(j.corr_len) < 1:
            raise ValueError("a pair without correspondences cannot be sampled")
        m = min(int(j.corr_len), k)
        o = (torch.empty((int(j.src_len), 3), dtype=torch.float32, device=dev),
             torch.empty((int(j.tgt_len), 3), dtype=torch.float32, device=dev),
             torch.empty((m, 2), dtype=torch.int64, device=dev), torch.empty((m, m), dtype=torch.float64, device=dev))
        q.src_off, q.src_len, q.tgt_off, q.tgt_len = int(j.src_off), int(j.src_len), int(j.tgt_off), int(j.tgt_len)
        q.corr_off, q.corr_len, q.key = int(j.corr_off), int(j.corr_len), int(j.key) & 0xffffffffffffffff
        q.R[:] = [float(v) for v in np.asarray(j.R, dtype=np.float64).reshape(9)]
        q.t[:] = [float(v) for v in np.asarray(j.t, dtype=np.float64).reshape(3)]
        q.out_src, q.out_tgt, q.out_corr, q.out_dist = (t.data_ptr() for t in o)
        out.append(o)
    L = _native.lib()
    nbytes = L.d3f_augment_pairs_ws_bytes(B, k)
    ws = _ws(nbytes, dev) if nbytes else None
    with _region("augment_pairs"):
        _native.check(L.d3f_augment_pairs(_p(points), int(points.shape[0]), _p(corr), int(corr.shape[0]), arr, B, k,
                                          float(noise), _p(ws), nbytes, _stream()), "d3f_augment_pairs")
    return out


# ---------------------------------------------------------------------------------------------------------------
# nearest neighbour over a list of cloud pairs (mining of the 3DMatch training pickles, datasets/preprocess.py)
# ---------------------------------------------------------------------------------------------------------------
MAX_CLOUDS = 65535   # the cell key keeps the cloud index in 16 bits


def _cloud_start(s_len):
    """int32 [B+1] device prefix of the cloud lengths."""
    start = torch.zeros(int(s_len.numel()) + 1, dtype=torch.int32, device=s_len.device)
    start[1:] = torch.cumsum(s_len, 0)
    return start


class CloudGrid:
    """One cell list over MANY stacked clouds (up to ``MAX_CLOUDS``; ``RadiusGrid`` takes 64) for ``nearest_pairs``:
    d3f_cloud_grid_build finds a point's cloud in a prefix of the lengths and keeps every cloud's buckets and points
    contiguous, which the radius search's queries do not read -- hence a class of its own."""

    def __init__(self, points, lens, radius, status=None):
        self.supports = _f32(points, "points")
        if self.supports.dim() != 2 or self.supports.shape[1] != 3:
            raise RuntimeError("Wrong dimensions : points.shape is not (N, 3)")
        dev = self.supports.device
        self.s_len = _lens(lens, dev, "lens")
        # lengths that came from the host stay known there: nearest_pairs then sizes its output without a read-back
        self.lens_host = None if isinstance(lens, torch.Tensor) and lens.is_cuda else \
            np.asarray(lens.cpu() if isinstance(lens, torch.Tensor) else lens, dtype=np.int64).reshape(-1)
        if self.lens_host is not None and (self.lens_host.min(initial=0) < 0 or
                                           int(self.lens_host.sum()) > int(self.supports.shape[0])):
            raise ValueError("lens must be non-negative and sum to at most the %d stacked points"
                             % int(self.supports.shape[0]))
        if not 1 <= int(self.s_len.numel()) <= MAX_CLOUDS:
            raise ValueError("1..%d clouds per cell list, got %d" % (MAX_CLOUDS, int(self.s_len.numel())))
        self.radius = float(radius)
        self.status = status if status is not None else DeviceStatus(dev)
        self.cloud_start = _cloud_start(self.s_len)
        L = _native.lib()
        self.Ns = int(self.supports.shape[0])
        nbytes = L.d3f_radius_grid_ws_bytes(self.Ns)
        self.ws = _ws(nbytes, dev)
        with _region("cloud_grid_build[Ns=%d]" % self.Ns, 12 * self.Ns + 24 * self.Ns):
            _native.check(L.d3f_cloud_grid_build(_p(self.supports), self.Ns, _p(self.cloud_start),
                                                 int(self.s_len.numel()), self.radius, _p(self.ws), nbytes,
                                                 _p(self.status.word), _stream()), "d3f_cloud_grid_build")


def _resolve_grid(grid_or_points, lens, radius, what):
    """The cell list of the geometry entries: ``grid_or_points`` itself when it is a ``RadiusGrid`` / ``CloudGrid`` (its
    radius must cover ``radius``; a ``RadiusGrid`` gets its ``cloud_start`` prefix on first use), else a ``CloudGrid``
    built over the stacked points with their ``lens``.  ``what`` names the radius in the error."""
    if isinstance(grid_or_points, (RadiusGrid, CloudGrid)):
        grid = grid_or_points
        if float(radius) > grid.radius:
            raise RuntimeError("%s %g exceeds the cell list's %g" % (what, float(radius), grid.radius))
        if getattr(grid, "cloud_start", None) is None:
            grid.cloud_start = _cloud_start(grid.s_len)
        return grid
    if lens is None:
        raise ValueError("lens is required with stacked points")
    return CloudGrid(grid_or_points, lens, radius)


def _pair_list(grid, pairs, T, name, rows=None, max_pairs=None):
    """The pair list of ``nearest_pairs`` / ``icp_rigid`` / ``pair_information`` -> ``(pairs int32 [P,2], P, T f64
    [P,12], row_start int64 [P+1], rows)``.  ``pairs``: host values (checked against the grid's clouds) or a device
    tensor (not read: the kernels answer a pair that names no cloud, and ``row_start`` takes the length of the clamped
    cloud).  ``T`` (``name`` in the error): [P,3,4], [P,4,4] or [P,12].  ``row_start`` is the prefix of the moving clouds'
    lengths; it and ``rows`` come from the host when pairs and lengths are known there, else ``rows`` is the caller's
    bound or the one read-back of this form.  ``max_pairs``: None for any number of pairs, none included, else
    1..max_pairs."""
    dev = grid.supports.device
    B = int(grid.s_len.numel())
    host = None
    if isinstance(pairs, torch.Tensor) and pairs.is_cuda:
        pr = pairs.to(torch.int32).contiguous().view(-1, 2)
    else:
        host = np.asarray(pairs.cpu() if isinstance(pairs, torch.Tensor) else pairs, dtype=np.int64).reshape(-1, 2)
        if host.size and (host.min() < 0 or host.max() >= B):
            raise ValueError("pairs name clouds outside 0..%d" % (B - 1))
        pr = torch.as_tensor(host.astype(np.int32), device=dev)
    P = int(pr.shape[0])
    if max_pairs is not None and not 1 <= P <= max_pairs:
        raise ValueError("1..%d pairs per call, got %d" % (max_pairs, P))
    tf = torch.as_tensor(T, dtype=torch.float64).to(dev)
    if tuple(tf.shape) not in ((P, 3, 4), (P, 4, 4), (P, 12)):
        raise ValueError("%s must be [P,3,4] or [P,4,4] for the %d pairs, got %s" % (name, P, tuple(tf.shape)))
    tf = tf.reshape(P, 16 if tuple(tf.shape[1:]) == (4, 4) else 12)[:, :12].contiguous()
    lens_host = getattr(grid, "lens_host", None)
    if host is not None and lens_host is not None:
        rs = np.zeros(P + 1, dtype=np.int64)
        rs[1:] = np.cumsum(lens_host[host[:, 0]])
        return pr, P, tf, torch.as_tensor(rs, device=dev), int(rs[-1])
    row_start = torch.zeros(P + 1, dtype=torch.int64, device=dev)
    if P:
        row_start[1:] = torch.cumsum(grid.s_len.long()[pr[:, 0].long().clamp(0, B - 1)], 0)
    if rows is None:
        rows = row_start[-1].item() if P else 0   # sizes the output: the one read-back of this form
    return pr, P, tf, row_start, int(rows)


def nearest_pairs_bytes(rows, found=None):
    """Algorithmic bytes of ``rows`` queries: the source point (12), the (start, end) headers of 27 buckets (216), the
    stored point and cell key of every candidate the accepted cells hold (24 each; ``found`` of them, by default one
    per query, the least a matched row reads) and the index written (4)."""
    rows = int(rows)
    return rows * (12 + 27 * 8 + 4) + 24 * (rows if found is None else int(found))


def nearest_pairs(grid_or_points, lens, pairs, transforms, radius, lanes=0):
    """Nearest neighbour within ``radius`` for every point of the source cloud of every pair (d3f_nearest_pairs).

    ``grid_or_points``: a ``RadiusGrid`` / ``CloudGrid`` over the stacked clouds (several chunks of pairs then share one
    cell list; ``lens`` may be None), or the stacked points [N,3] themselves, each cloud in its own frame, with ``lens``
    their lengths.  ``pairs`` int [P,2] = (source cloud, target cloud), ``transforms`` f64 [P,3,4] or [P,4,4] mapping
    source points into the target's frame.  Returns ``(nn int32 [rows], count int32 [P], row_start int64 [P+1])``:
    rows ``row_start[p] .. row_start[p+1]`` are the points of pair p's source in order, ``nn`` the index inside the target
    cloud (-1: none within the radius), ``count[p]`` the rows of pair p with a neighbour.  Arithmetic and tie rule:
    include/d3feat_hip.h.  Host ``pairs`` are checked against the clouds; a device tensor is not read, and a pair of it
    that names a cloud that is not there gets -1 rows and count 0 (its rows: those of the clamped source cloud).
    ``lanes``: lanes per query (measurements; the result does not depend on it)."""
    grid = _resolve_grid(grid_or_points, lens, radius, "search radius")
    dev = grid.supports.device
    pr, P, tf, row_start, rows = _pair_list(grid, pairs, transforms, "transforms")
    nn = torch.empty(rows, dtype=torch.int32, device=dev)
    count = torch.zeros(P, dtype=torch.int32, device=dev)
    if rows == 0:
        return nn, count, row_start
    with _region("nearest_pairs[P=%d,rows=%d]" % (P, rows), nearest_pairs_bytes(rows)):
        _native.check(_native.lib().d3f_nearest_pairs_lanes(
            _p(grid.ws), _p(grid.supports), grid.Ns, _p(grid.cloud_start), int(grid.s_len.numel()), grid.radius,
            float(radius), _p(pr), _p(tf), _p(row_start), P, rows, _p(nn), _p(count), _p(grid.status.word), int(lanes),
            _stream()),
            "d3f_nearest_pairs")
    return nn, count, row_start


# ---------------------------------------------------------------------------------------------------------------
# point-to-point ICP over a list of cloud pairs (the refinement after RANSAC; Open3D's registration_icp)
# ---------------------------------------------------------------------------------------------------------------
ICP_MAX_ITERS = _native.D3F_ICP_MAX_ITERS
ICP_BLOCK_ROWS = _native.D3F_ICP_BLOCK_ROWS
ICP_ST_FEW, ICP_ST_CELL_RANGE = _native.D3F_ICP_ST_FEW, _native.D3F_ICP_ST_CELL_RANGE
ICP_ST_PAIR, ICP_ST_NONFINITE = _native.D3F_ICP_ST_PAIR, _native.D3F_ICP_ST_NONFINITE
ICP_ST_SINGULAR = _native.D3F_ICP_ST_SINGULAR   # point-to-plane: singular normal equations (one plane's free slide, zero normals)
PG_ST_ITER_CAP, PG_ST_NONFINITE = _native.D3F_PG_ST_ITER_CAP, _native.D3F_PG_ST_NONFINITE   # pose_graph_optimize
PG_ST_GRAPH, PG_ST_INDEFINITE = _native.D3F_PG_ST_GRAPH, _native.D3F_PG_ST_INDEFINITE
PG_MAX_NODES = _native.D3F_PG_MAX_NODES     # nodes of one graph
PG_MAX_ITERS = _native.D3F_PG_MAX_ITERS


def icp_rigid_bytes(rows, found=None):
    """Algorithmic bytes of ONE search of ``rows`` rows: ``nearest_pairs_bytes`` without the 4-byte index, plus the 136
    bytes of sums a workgroup of ``ICP_BLOCK_ROWS`` rows writes and the fit reads back."""
    rows = int(rows)
    return nearest_pairs_bytes(rows, found) - 4 * rows + 2 * 136 * (-(-rows // ICP_BLOCK_ROWS))


def icp_plane_bytes(rows, found=None):
    """Algorithmic bytes of ONE point-to-plane search of ``rows`` rows: ``icp_rigid_bytes`` with 232 bytes of sums (29
    f64) per workgroup in place of 136, plus the 12-byte normal of every matched row (``found`` of them, by default one
    per row)."""
    rows = int(rows)
    return (icp_rigid_bytes(rows, found) + 2 * (232 - 136) * (-(-rows // ICP_BLOCK_ROWS))
            + 12 * (rows if found is None else int(found)))


def icp_color_bytes(rows, found=None):
    """Algorithmic bytes of ONE coloured search of ``rows`` rows: ``icp_plane_bytes`` with 248 bytes of sums (31 f64) per
    workgroup in place of 232, plus the 16-byte field row of the matched fixed point and the 4-byte intensity of the
    moving point of every matched row (``found`` of them, by default one per row)."""
    rows = int(rows)
    return (icp_plane_bytes(rows, found) + 2 * (248 - 232) * (-(-rows // ICP_BLOCK_ROWS))
            + 20 * (rows if found is None else int(found)))


def pair_information_bytes(rows, found=None):
    """Algorithmic bytes of the ONE search of ``pair_information``: ``icp_rigid_bytes`` with 160 bytes of sums (20 f64)
    per workgroup in place of 136."""
    rows = int(rows)
    return icp_rigid_bytes(rows, found) + 2 * (160 - 136) * (-(-rows // ICP_BLOCK_ROWS))


def estimate_normals_bytes(n, neighbors=None):
    """Algorithmic bytes of the normals of ``n`` points: the point (12), the (start, end) headers of 27 buckets (216),
    the stored point and cell key of every candidate the accepted cells hold (24 each; ``neighbors`` of them in all, by
    default the point itself), the normal (12) and the count (4)."""
    n = int(n)
    return n * (12 + 27 * 8 + 12 + 4) + 24 * (n if neighbors is None else int(neighbors))


def estimate_normals(grid_or_points, lens, radius, min_neighbors=3, viewpoint=None, return_moments=False):
    """Surface normal of every point of the stacked clouds (d3f_estimate_normals): the eigenvector of the smallest
    eigenvalue of the covariance of the point's neighbours within ``radius`` IN ITS OWN CLOUD (itself included), turned
    towards ``viewpoint`` (3 numbers, the same point in every cloud's own frame; default the origin).

    ``grid_or_points``, ``lens``: as in ``nearest_pairs`` -- a ``RadiusGrid`` / ``CloudGrid`` with ``radius`` at most
    its own, or the stacked points with their lengths.  Returns device tensors ``(normals [N,3] f32, count [N] int32)``
    in input row order and, with ``return_moments``, ``moments [N,10] int64``.  A point with fewer than
    ``min_neighbors`` neighbours, or whose neighbours coincide, gets the normal (0, 0, 0).  The moments are integer sums
    (include/d3feat_hip.h), so the result does not depend on the order in which the cell list holds the points: it is
    bit-identical from run to run, for a cloud alone or stacked among others, and for any cell size."""
    if not (0.0 < float(radius) < float("inf")) or int(min_neighbors) < 1:
        raise ValueError("radius must be positive and finite, min_neighbors at least 1")
    grid = _resolve_grid(grid_or_points, lens, radius, "radius")
    dev = grid.supports.device
    view = None
    if viewpoint is not None:
        view = np.ascontiguousarray(np.asarray(viewpoint, dtype=np.float32).reshape(-1))
        if view.shape != (3,) or not np.isfinite(view).all():
            raise ValueError("viewpoint must be 3 finite numbers")
    N = grid.Ns
    normals = torch.empty((N, 3), dtype=torch.float32, device=dev)
    count = torch.empty(N, dtype=torch.int32, device=dev)
    moments = torch.empty((N, 10), dtype=torch.int64, device=dev) if return_moments else None
    if N:
        with _region("estimate_normals[N=%d]" % N, estimate_normals_bytes(N)):
            _native.check(_native.lib().d3f_estimate_normals(
                _p(grid.ws), _p(grid.supports), N, _p(grid.cloud_start), int(grid.s_len.numel()), grid.radius,
                float(radius), int(min_neighbors), view.ctypes.data if view is not None else None, _p(normals),
                _p(count), _p(moments), _p(grid.status.word), _stream()), "d3f_estimate_normals")
    return (normals, count, moments) if return_moments else (normals, count)


def color_gradients_bytes(n, neighbors=None):
    """Algorithmic bytes of the colour gradients of ``n`` points: ``estimate_normals_bytes`` with the point's normal (12)
    and intensity (4) read, the 4-byte intensity of every neighbour (``neighbors`` of them in all, by default the point
    itself) and a 16-byte field row written in place of the 12-byte normal."""
    n = int(n)
    return estimate_normals_bytes(n, neighbors) + n * (12 + 4 + 4) + 4 * (n if neighbors is None else int(neighbors))


def color_gradients(grid_or_points, lens, radius, normals, intensity, min_neighbors=4, return_moments=False):
    """Colour gradient of every point of the stacked clouds on its tangent plane (d3f_color_gradients) -- what the
    coloured form of ``icp_rigid`` reads per matched fixed point.

    ``grid_or_points``, ``lens``, ``radius``: as in ``estimate_normals`` (the same neighbourhood: the point's own cloud,
    itself included).  ``normals`` f32 [N,3] (``estimate_normals``) and ``intensity`` f32 [N] or [N,1] in input row
    order; an intensity is usable when ``0 <= I <= 1``, anything else (NaN included) means "no colour"
    (``registration.intensity_of`` makes one from RGB).  The gradient is the least-squares slope of the intensity over
    the neighbours with a usable intensity, restricted to the tangent plane (rule: include/d3feat_hip.h).  Returns device
    tensors ``(field [N,4] f32 = (d_x, d_y, d_z, I), count [N] int32)`` and, with ``return_moments``, ``moments [N,13]
    int64``.  Three NaNs mark an invalid gradient (own intensity not usable, fewer than ``min_neighbors`` usable
    neighbours, a zero normal, neighbours on one line), a NaN in ``.w`` an unusable intensity.  The moments are integer
    sums, so the result is bit-identical from run to run, for a cloud alone or stacked, and for any cell size."""
    if not (0.0 < float(radius) < float("inf")) or int(min_neighbors) < 1:
        raise ValueError("radius must be positive and finite, min_neighbors at least 1")
    grid = _resolve_grid(grid_or_points, lens, radius, "radius")
    dev = grid.supports.device
    N = grid.Ns
    nrm = _f32(normals, "normals")
    if tuple(nrm.shape) != (N, 3) or nrm.device != dev:
        raise ValueError("normals must be [%d,3] on the points' device, got %s" % (N, tuple(nrm.shape)))
    inten = _f32(intensity, "intensity")
    if tuple(inten.shape) not in ((N,), (N, 1)) or inten.device != dev:
        raise ValueError("intensity must be [%d] or [%d,1] on the points' device, got %s" % (N, N, tuple(inten.shape)))
    field = torch.empty((N, 4), dtype=torch.float32, device=dev)
    count = torch.empty(N, dtype=torch.int32, device=dev)
    moments = torch.empty((N, 13), dtype=torch.int64, device=dev) if return_moments else None
    if N:
        with _region("color_gradients[N=%d]" % N, color_gradients_bytes(N)):
            _native.check(_native.lib().d3f_color_gradients(
                _p(grid.ws), _p(grid.supports), N, _p(grid.cloud_start), int(grid.s_len.numel()), grid.radius,
                float(radius), int(min_neighbors), _p(nrm), _p(inten), _p(field), _p(count), _p(moments),
                _p(grid.status.word), _stream()), "d3f_color_gradients")
    return (field, count, moments) if return_moments else (field, count)


# ---------------------------------------------------------------------------------------------------------------
# FPFH descriptors (csrc/fpfh.hpp has the rule; Open3D's compute_fpfh_feature)
# ---------------------------------------------------------------------------------------------------------------
FPFH_WIDTH = 33          # 3 histograms of 11 bins
FPFH_ROW = 36            # int32 per row of the SPFH table between the two passes (33 counts, n, two zeros)
FPFH_WIDTHS = (33, 64)   # row widths d3f_fpfh writes; 64 is zero-padded, the width mutual_nn reads


def fpfh_bytes(n, neighbors=None):
    """Algorithmic bytes of the FPFH descriptors of ``n`` points at row width 33, both passes: each pass reads the point
    (12), the (start, end) headers of 27 buckets (216) and the stored point and cell key of every candidate the accepted
    cells hold (24 each; ``neighbors`` of them in all, by default one per point).  The SPFH pass also reads the point's
    normal (12) and the 12-byte normal of every neighbour and writes a 144-byte table row and the count (4); the FPFH
    pass reads the point's own table row (144) and that of every neighbour (144 each) and writes the descriptor (132)."""
    n = int(n)
    m = n if neighbors is None else int(neighbors)
    return n * (2 * (12 + 27 * 8) + 12 + 4 + 4 * FPFH_ROW + 4 * FPFH_ROW + 4 * FPFH_WIDTH) + m * (2 * 24 + 12 + 4 * FPFH_ROW)


def _fpfh_width(row_width):
    if int(row_width) not in FPFH_WIDTHS:
        raise ValueError("row_width must be 33 or 64, got %r" % (row_width,))
    return int(row_width)


def fpfh(grid_or_points, lens, radius, normals, row_width=33, return_spfh=False, unit=False):
    """FPFH descriptor of every point of the stacked clouds (d3f_fpfh; what Open3D's compute_fpfh_feature computes on the
    CPU): three 11-bin histograms of the pair features of the point's neighbours within ``radius`` IN ITS OWN CLOUD, each
    the sum of the point's own histogram and the distance-weighted histograms of its neighbours, scaled to 100.

    ``grid_or_points``, ``lens``, ``radius``: as in ``estimate_normals``.  ``normals`` f32 [N,3] in input row order
    (``estimate_normals``); a point whose normal is (0, 0, 0) has no descriptor and is nobody's neighbour.  Returns device
    tensors ``(desc [N,row_width] f32, count [N] int32)`` and, with ``return_spfh``, ``spfh [N,33] int32`` (the
    neighbour counts per bin).  ``row_width`` 33, or 64 for zero-padded rows: zero columns do not change an L2 distance,
    so that is what ``mutual_nn`` reads with no copy -- with ``unit=True``, which scales every row to unit L2 norm in
    the kernel (f64, a fixed order: csrc/fpfh.hpp): ``mutual_nn`` ranks by the inner product of UNIT rows, which for
    them is the order of the L2 distance.  ``count`` is the number of neighbours; a point with count 0 has
    no descriptor and a row of zeros.  Every sum over neighbours is an integer (csrc/fpfh.hpp), so the result is
    bit-identical from run to run, for any row order, for a cloud alone or stacked, and for any cell size.  Two
    launches, no read-back, capturable in a graph."""
    if not (0.0 < float(radius) < float("inf")):
        raise ValueError("radius must be positive and finite")
    width = _fpfh_width(row_width)
    grid = _resolve_grid(grid_or_points, lens, radius, "radius")
    dev = grid.supports.device
    N = grid.Ns
    nrm = _f32(normals, "normals")
    if tuple(nrm.shape) != (N, 3) or nrm.device != dev:
        raise ValueError("normals must be [%d,3] on the points' device, got %s" % (N, tuple(nrm.shape)))
    desc = torch.empty((N, width), dtype=torch.float32, device=dev)
    count = torch.empty(N, dtype=torch.int32, device=dev)
    spfh = torch.empty((N, FPFH_WIDTH), dtype=torch.int32, device=dev) if return_spfh else None
    if N:
        L = _native.lib()
        nbytes = L.d3f_fpfh_ws_bytes(N)
        ws = _ws(nbytes, dev)
        with _region("fpfh[N=%d]" % N, fpfh_bytes(N)):
            _native.check(L.d3f_fpfh(
                _p(grid.ws), _p(grid.supports), _p(nrm), N, _p(grid.cloud_start), int(grid.s_len.numel()), grid.radius,
                float(radius), width, int(bool(unit)), _p(desc), _p(count), _p(spfh), _p(grid.status.word), _p(ws), nbytes,
                _stream()),
                "d3f_fpfh")
    return (desc, count, spfh) if return_spfh else (desc, count)


def fpfh_host(points, lens, radius, normals, row_width=33, return_spfh=False, unit=False):
    """The host twin of ``fpfh`` (d3f_fpfh_host): the same inline rule compiled for the CPU, brute force within each
    cloud, one thread.  ``points`` [N,3], ``lens`` and ``normals`` [N,3] are host arrays (or CPU tensors); returns CPU
    tensors.  No GPU call."""
    if not (0.0 < float(radius) < float("inf")):
        raise ValueError("radius must be positive and finite")
    width = _fpfh_width(row_width)
    pts = np.ascontiguousarray(_host_array(points), dtype=np.float32)
    nrm = np.ascontiguousarray(_host_array(normals), dtype=np.float32)
    ln = np.asarray(_host_array(lens), dtype=np.int64).reshape(-1)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError("points must be [N,3], got %s" % (pts.shape,))
    N = int(pts.shape[0])
    if nrm.shape != (N, 3):
        raise ValueError("normals must be [%d,3], got %s" % (N, nrm.shape))
    if not 1 <= ln.size <= MAX_CLOUDS or ln.min() < 0 or int(ln.sum()) > N:
        raise ValueError("lens must be 1..%d non-negative lengths that sum to at most the %d stacked points"
                         % (MAX_CLOUDS, N))
    start = np.zeros(ln.size + 1, dtype=np.int32)
    start[1:] = np.cumsum(ln)
    desc = np.zeros((N, width), dtype=np.float32)
    count = np.zeros(N, dtype=np.int32)
    spfh = np.zeros((N, FPFH_WIDTH), dtype=np.int32) if return_spfh else None
    _native.check(_native.lib().d3f_fpfh_host(
        pts.ctypes.data, nrm.ctypes.data, N, start.ctypes.data, int(ln.size), float(radius), width, int(bool(unit)),
        desc.ctypes.data,
        count.ctypes.data, spfh.ctypes.data if return_spfh else None), "d3f_fpfh_host")
    out = (torch.from_numpy(desc), torch.from_numpy(count))
    return out + (torch.from_numpy(spfh),) if return_spfh else out


# ---------------------------------------------------------------------------------------------------------------
# ISS keypoints and radius non-maximum suppression (csrc/iss.hpp has the rule; Open3D's compute_iss_keypoints)
# ---------------------------------------------------------------------------------------------------------------
def iss_saliency_bytes(n, neighbors=None):
    """Algorithmic bytes of the ISS saliency of ``n`` points: ``estimate_normals_bytes`` with a 4-byte saliency written
    in place of the 12-byte normal."""
    return estimate_normals_bytes(n, neighbors) - 8 * int(n)


def radius_nms_bytes(n, walking=None, neighbors=None):
    """Algorithmic bytes of the suppression of ``n`` rows of which ``walking`` (default all) have a positive score: every
    row reads its score (4) and writes keep and count (5); a walking row reads its point (12), the (start, end) headers
    of 27 buckets (216), and the stored point, cell key and score of every candidate (28 each; ``neighbors`` of them in
    all, by default the row itself)."""
    n = int(n)
    w = n if walking is None else int(walking)
    return n * (4 + 5) + w * (12 + 27 * 8) + 28 * (w if neighbors is None else int(neighbors))


def _iss_checks(radius, min_neighbors, gammas=()):
    if not (0.0 < float(radius) < float("inf")) or int(min_neighbors) < 1:
        raise ValueError("radius must be positive and finite, min_neighbors at least 1")
    for g in gammas:
        if not (0.0 < float(g) <= 1.0):
            raise ValueError("gamma_21 and gamma_32 must lie in (0, 1], got %r" % (g,))


def _score_rows(score, N, dev):
    s = _f32(score, "score")
    if tuple(s.shape) not in ((N,), (N, 1)) or s.device != dev:
        raise ValueError("score must be [%d] or [%d,1] on the points' device, got %s" % (N, N, tuple(s.shape)))
    return s


def iss_saliency(grid_or_points, lens, radius, gamma_21=0.975, gamma_32=0.975, min_neighbors=5, return_moments=False):
    """ISS saliency of every point of the stacked clouds (d3f_iss_saliency): with e1 >= e2 >= e3 the eigenvalues of the
    covariance of the point's neighbours within ``radius`` IN ITS OWN CLOUD (itself included; the neighbourhood and the
    integer moments of ``estimate_normals``), a point is salient when it has at least ``min_neighbors`` neighbours,
    ``e2 < gamma_21 e1`` and ``e3 < gamma_32 e2``; its saliency is e3 (f32, squared length units), 0 when not salient.
    The defaults are Open3D's.

    ``grid_or_points``, ``lens``, ``radius``: as in ``estimate_normals``.  Returns device tensors ``(saliency [N] f32,
    count [N] int32)`` in input row order and, with ``return_moments``, ``moments [N,10] int64``.  The result is
    bit-identical from run to run, for any row order, for a cloud alone or stacked, and for any cell size."""
    _iss_checks(radius, min_neighbors, (gamma_21, gamma_32))
    grid = _resolve_grid(grid_or_points, lens, radius, "radius")
    dev = grid.supports.device
    N = grid.Ns
    saliency = torch.empty(N, dtype=torch.float32, device=dev)
    count = torch.empty(N, dtype=torch.int32, device=dev)
    moments = torch.empty((N, 10), dtype=torch.int64, device=dev) if return_moments else None
    if N:
        with _region("iss_saliency[N=%d]" % N, iss_saliency_bytes(N)):
            _native.check(_native.lib().d3f_iss_saliency(
                _p(grid.ws), _p(grid.supports), N, _p(grid.cloud_start), int(grid.s_len.numel()), grid.radius,
                float(radius), float(gamma_21), float(gamma_32), int(min_neighbors), _p(saliency), _p(count),
                _p(moments), _p(grid.status.word), _stream()), "d3f_iss_saliency")
    return (saliency, count, moments) if return_moments else (saliency, count)


def radius_nms(grid_or_points, lens, radius, score, min_neighbors=1):
    """Radius non-maximum suppression of any per-point score (d3f_radius_nms): row i is kept when ``score[i] > 0`` (a NaN
    is not), no neighbour within ``radius`` IN ITS OWN CLOUD has a strictly larger score -- equal scores both survive,
    so the row order does not matter -- and the neighbourhood, i included, holds at least ``min_neighbors`` points.

    ``grid_or_points``, ``lens``, ``radius``: as in ``estimate_normals``; ``score`` f32 [N] or [N,1] in input row order.
    Returns device tensors ``(keep [N] bool, count [N] int32)``: ``count`` is the size of the neighbourhood of a row
    with a positive score and 0 for every other row (those are not searched).  One launch, no read-back."""
    _iss_checks(radius, min_neighbors)
    grid = _resolve_grid(grid_or_points, lens, radius, "radius")
    dev = grid.supports.device
    N = grid.Ns
    s = _score_rows(score, N, dev)
    keep = torch.empty(N, dtype=torch.uint8, device=dev)
    count = torch.empty(N, dtype=torch.int32, device=dev)
    if N:
        with _region("radius_nms[N=%d]" % N, radius_nms_bytes(N)):
            _native.check(_native.lib().d3f_radius_nms(
                _p(grid.ws), _p(grid.supports), N, _p(grid.cloud_start), int(grid.s_len.numel()), grid.radius,
                float(radius), _p(s), int(min_neighbors), _p(keep), _p(count), _p(grid.status.word), _stream()),
                "d3f_radius_nms")
    return keep.view(torch.bool), count


def iss_keypoints(grid_or_points, lens, salient_radius, non_max_radius, gamma_21=0.975, gamma_32=0.975,
                  min_neighbors=5):
    """ISS keypoints of the stacked clouds (d3f_iss_keypoints): ``iss_saliency`` at ``salient_radius``, then
    ``radius_nms`` of that saliency at ``non_max_radius`` with the same ``min_neighbors``, over ONE cell list whose
    radius covers both.  Returns device tensors ``(saliency [N] f32, keep [N] bool, count_salient [N] int32, count_nms
    [N] int32)``, bit for bit what the two calls return.  Two launches, no read-back, capturable in a graph."""
    _iss_checks(salient_radius, min_neighbors, (gamma_21, gamma_32))
    _iss_checks(non_max_radius, min_neighbors)
    grid = _resolve_grid(grid_or_points, lens, max(float(salient_radius), float(non_max_radius)), "radius")
    dev = grid.supports.device
    N = grid.Ns
    saliency = torch.empty(N, dtype=torch.float32, device=dev)
    keep = torch.empty(N, dtype=torch.uint8, device=dev)
    count_salient = torch.empty(N, dtype=torch.int32, device=dev)
    count_nms = torch.empty(N, dtype=torch.int32, device=dev)
    if N:
        with _region("iss_keypoints[N=%d]" % N, iss_saliency_bytes(N) + radius_nms_bytes(N)):
            _native.check(_native.lib().d3f_iss_keypoints(
                _p(grid.ws), _p(grid.supports), N, _p(grid.cloud_start), int(grid.s_len.numel()), grid.radius,
                float(salient_radius), float(non_max_radius), float(gamma_21), float(gamma_32), int(min_neighbors),
                _p(saliency), _p(keep), _p(count_salient), _p(count_nms), _p(grid.status.word), _stream()),
                "d3f_iss_keypoints")
    return saliency, keep.view(torch.bool), count_salient, count_nms


def iss_saliency_from_moments_host(moments, Q, gamma_21=0.975, gamma_32=0.975, min_neighbors=5):
    """The host twin of everything after the moments of ``iss_saliency`` (d3f_iss_saliency_from_moments_host, the same
    inline code compiled for the CPU): ``moments`` int64 [n,10] host rows, ``Q`` their scale
    (``registration.normals_scale(radius)``) -> f32 [n] CPU tensor.  No GPU call."""
    _iss_checks(1.0, min_neighbors, (gamma_21, gamma_32))
    m = np.ascontiguousarray(_host_array(moments), dtype=np.int64)
    if m.ndim != 2 or m.shape[1] != 10 or not float(Q) > 0.0:
        raise ValueError("moments must be [n,10] and Q positive, got %s and %r" % (m.shape, Q))
    out = np.zeros(m.shape[0], dtype=np.float32)
    fn = _native.lib().d3f_iss_saliency_from_moments_host
    for k in range(m.shape[0]):
        _native.check(fn(m[k].ctypes.data, float(Q), float(gamma_21), float(gamma_32), int(min_neighbors),
                         out[k:].ctypes.data), "d3f_iss_saliency_from_moments_host")
    return torch.from_numpy(out)


def radius_nms_host(points, lens, radius, score, min_neighbors=1):
    """The host twin of ``radius_nms`` (d3f_radius_nms_host): the same rule compiled for the CPU, brute force within
    each cloud, one thread.  ``points`` [N,3], ``lens`` and ``score`` [N] or [N,1] are host arrays (or CPU tensors);
    returns CPU tensors ``(keep bool [N], count int32 [N])``.  No GPU call."""
    _iss_checks(radius, min_neighbors)
    pts = np.ascontiguousarray(_host_array(points), dtype=np.float32)
    ln = np.asarray(_host_array(lens), dtype=np.int64).reshape(-1)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError("points must be [N,3], got %s" % (pts.shape,))
    N = int(pts.shape[0])
    sc = np.ascontiguousarray(_host_array(score), dtype=np.float32)
    if sc.shape not in ((N,), (N, 1)):
        raise ValueError("score must be [%d] or [%d,1], got %s" % (N, N, sc.shape))
    if not 1 <= ln.size <= MAX_CLOUDS or ln.min() < 0 or int(ln.sum()) > N:
        raise ValueError("lens must be 1..%d non-negative lengths that sum to at most the %d stacked points"
                         % (MAX_CLOUDS, N))
    start = np.zeros(ln.size + 1, dtype=np.int32)
    start[1:] = np.cumsum(ln)
    keep = np.zeros(N, dtype=np.uint8)
    count = np.zeros(N, dtype=np.int32)
    _native.check(_native.lib().d3f_radius_nms_host(
        pts.ctypes.data, sc.ctypes.data, N, start.ctypes.data, int(ln.size), float(radius), int(min_neighbors),
        keep.ctypes.data, count.ctypes.data), "d3f_radius_nms_host")
    return torch.from_numpy(keep.astype(np.bool_)), torch.from_numpy(count)


def icp_rigid(grid_or_points, lens, pairs, T_init, max_distance, max_iters=30, rel_fitness=1e-6, rel_rmse=1e-6,
              return_trace=False, rows=None, normals=None, color_field=None, lambda_geometric=0.968):
    """Point-to-point ICP of P cloud pairs, all advancing together on the device (d3f_icp_rigid).

    ``grid_or_points``, ``lens``, ``pairs``: as in ``nearest_pairs`` -- pair p = (MOVING cloud a, FIXED cloud b) and
    ``T_init`` f64 [P,4,4] or [P,3,4] maps points of a into b's frame.  (For a ``gt.log`` key i_j, whose matrix maps j
    into i -- what ``ransac_rigid`` returns -- the pair is (j, i) and the matrix is a valid ``T_init`` as it stands.)
    Each iteration matches every moving point to its nearest fixed point closer than ``max_distance`` (arithmetic and tie
    rule of ``nearest_pairs``) and fits the rigid motion to the matches in f64; a pair stops when fitness and RMSE both
    change by less than ``rel_fitness`` / ``rel_rmse`` (absolute differences, Open3D's ICPConvergenceCriteria), after
    ``max_iters`` fits, or with fewer than 3 matches (``ICP_ST_FEW``).  Returns device tensors ``(T [P,4,4] f64, count
    [P] int32, rmse [P] f64, iterations [P] int32, status [P] int32)``: ``count`` / ``rmse`` are those of the returned
    ``T``; ``return_trace=True`` appends ``trace [P, max_iters+1, 2]`` f64 = (n_k, sum d2_k) per search (NaN beyond the
    stop).  Bit-identical from run to run and for a pair alone or inside any batch.  No read-back when the lengths and
    pairs are known on the host, or when ``rows`` -- a host bound on the moving rows of all pairs together -- comes with
    device ``pairs`` (the form a captured graph takes; a pair reaching beyond it gets ``ICP_ST_PAIR``).

    ``normals``: None, or the f32 [N,3] normals of the stacked points (``estimate_normals``) -- the fit then minimises
    the POINT-TO-PLANE residual against the fixed cloud's normals (d3f_icp_rigid_plane; Open3D's
    TransformationEstimationPointToPlane).  Search, count, rmse, stopping rule and trace keep their meaning; a pair
    whose 6x6 normal equations are singular (the overlap is one plane, or has only zero normals) stops at its current
    pose with ``ICP_ST_SINGULAR``.  It converges in a handful of iterations from a good pose and can stall or diverge
    where point-to-point does not -- on a low overlap that is mostly one plane, or from a poor start.

    ``color_field``: None, or the f32 [N,4] field of ``color_gradients`` (requires ``normals``) -- COLOURED ICP
    (d3f_icp_rigid_color; Open3D's registration_colored_icp): the point-to-plane rows weighted by
    ``sqrt(lambda_geometric)`` plus, per matched row whose fixed point has a valid gradient and whose moving point has
    an intensity, a colour row weighted by ``sqrt(1 - lambda_geometric)``, so that texture holds the pose where a
    single plane lets it slide.  ``n_color [P] int32`` and ``color_rmse [P] f64`` of the returned pose are then
    appended to the results (after ``trace``); ``n_color == 0`` means that colour took no part.  ``lambda_geometric=1``
    gives the point-to-plane results bit for bit.  The default 0.968 is Open3D's; it has not been tuned here."""
    if not 0 <= int(max_iters) <= ICP_MAX_ITERS:
        raise ValueError("max_iters must be in 0..%d" % ICP_MAX_ITERS)
    if not float(rel_fitness) >= 0.0 or not float(rel_rmse) >= 0.0:
        raise ValueError("rel_fitness and rel_rmse must be non-negative")
    grid = _resolve_grid(grid_or_points, lens, max_distance, "max_distance")
    if not (0.0 < float(max_distance) < float("inf")):
        raise ValueError("max_distance must be positive and finite")
    dev = grid.supports.device
    pr, P, tf, row_start, rows = _pair_list(grid, pairs, T_init, "T_init", rows, MAX_CLOUDS)
    K = int(max_iters)
    T = torch.empty((P, 4, 4), dtype=torch.float64, device=dev)
    count, iterations, status = (torch.empty(P, dtype=torch.int32, device=dev) for _ in range(3))
    rmse = torch.empty(P, dtype=torch.float64, device=dev)
    trace = torch.empty((P, K + 1, 2), dtype=torch.float64, device=dev) if return_trace else None
    L = _native.lib()
    nrm = None
    if normals is not None:
        nrm = _f32(normals, "normals")
        if tuple(nrm.shape) != (grid.Ns, 3) or nrm.device != dev:
            raise ValueError("normals must be [%d,3] on the points' device, got %s" % (grid.Ns, tuple(nrm.shape)))
    plane = nrm is not None
    if color_field is not None:
        if not plane:
            raise ValueError("color_field requires normals")
        if not 0.0 <= float(lambda_geometric) <= 1.0:
            raise ValueError("lambda_geometric must be in [0, 1]")
        field = _f32(color_field, "color_field")
        if tuple(field.shape) != (grid.Ns, 4) or field.device != dev:
            raise ValueError("color_field must be [%d,4] on the points' device, got %s" % (grid.Ns, tuple(field.shape)))
        n_color = torch.empty(P, dtype=torch.int32, device=dev)
        color_rmse = torch.empty(P, dtype=torch.float64, device=dev)
        nbytes = L.d3f_icp_rigid_color_ws_bytes(P, rows)
        ws = _ws(nbytes, dev)
        with _region("icp_rigid_color[P=%d,rows=%d,iters<=%d]" % (P, rows, K), (K + 1) * icp_color_bytes(rows)):
            _native.check(L.d3f_icp_rigid_color(
                _p(grid.ws), _p(grid.supports), _p(nrm), _p(field), grid.Ns, _p(grid.cloud_start),
                int(grid.s_len.numel()), grid.radius, float(max_distance), _p(pr), _p(row_start), P, rows, _p(tf),
                float(lambda_geometric), K, float(rel_fitness), float(rel_rmse), _p(T), _p(count), _p(rmse),
                _p(iterations), _p(status), _p(n_color), _p(color_rmse), _p(trace), _p(ws), nbytes, _stream()),
                "d3f_icp_rigid_color")
        res = (T, count, rmse, iterations, status)
        return (res + (trace,) if return_trace else res) + (n_color, color_rmse)
    name = "d3f_icp_rigid_plane" if plane else "d3f_icp_rigid"
    nbytes = getattr(L, name + "_ws_bytes")(P, rows)
    ws = _ws(nbytes, dev)
    head = (_p(grid.ws), _p(grid.supports)) + ((_p(nrm),) if plane else ())
    with _region("%s[P=%d,rows=%d,iters<=%d]" % (name[4:], P, rows, K),
                 (K + 1) * (icp_plane_bytes if plane else icp_rigid_bytes)(rows)):
        _native.check(getattr(L, name)(
            *head, grid.Ns, _p(grid.cloud_start), int(grid.s_len.numel()), grid.radius, float(max_distance), _p(pr),
            _p(row_start), P, rows, _p(tf), K, float(rel_fitness), float(rel_rmse), _p(T), _p(count), _p(rmse),
            _p(iterations), _p(status), _p(trace), _p(ws), nbytes, _stream()), name)
    res = (T, count, rmse, iterations, status)
    return res + (trace,) if return_trace else res


INFO_MOMENTS = _native.D3F_INFO_MOMENTS   # n, sum x (3), sum x x^T (6), sum y (3), sum y y^T (6), sum d2


def pair_information(grid_or_points, lens, pairs, T, max_distance, rows=None):
    """Raw moments of the correspondences of P cloud pairs under the GIVEN poses (d3f_pair_information) -- what the 6x6
    information matrix of a pair is made of (``registration.information_from_moments``; the benchmark's ``gt.info``).

    Arguments as in ``icp_rigid``: pair p = (MOVING cloud a, FIXED cloud b), ``T`` f64 [P,4,4] or [P,3,4] maps points
    of a into b's frame; host or device ``pairs``; ``rows`` for the captured form.  ONE search -- ``icp_rigid``'s
    iteration 0, bit for bit -- and over its accepted rows, in f64, ``moments [P,20]`` = n, sum x (3), the upper
    triangle of sum x x^T (xx, xy, xz, yy, yz, zz), sum y (3), the upper triangle of sum y y^T (6), sum d2: x the moving
    point in its OWN frame, y the matched fixed point, raw (no pivots).  Returns device tensors ``(moments, count [P]
    int32, status [P] int32)``; a pair flagged ``ICP_ST_PAIR`` / ``ICP_ST_NONFINITE`` has zero moments.  Three
    launches, bit-identical from run to run and for a pair alone or inside any batch; no read-back when the lengths and
    pairs are known on the host, or when ``rows`` comes with device ``pairs``."""
    grid = _resolve_grid(grid_or_points, lens, max_distance, "max_distance")
    if not (0.0 < float(max_distance) < float("inf")):
        raise ValueError("max_distance must be positive and finite")
    dev = grid.supports.device
    pr, P, tf, row_start, rows = _pair_list(grid, pairs, T, "T", rows, MAX_CLOUDS)
    moments = torch.empty((P, INFO_MOMENTS), dtype=torch.float64, device=dev)
    count, status = (torch.empty(P, dtype=torch.int32, device=dev) for _ in range(2))
    L = _native.lib()
    nbytes = L.d3f_pair_information_ws_bytes(P, rows)
    ws = _ws(nbytes, dev)
    with _region("pair_information[P=%d,rows=%d]" % (P, rows), pair_information_bytes(rows)):
        _native.check(L.d3f_pair_information(
            _p(grid.ws), _p(grid.supports), grid.Ns, _p(grid.cloud_start), int(grid.s_len.numel()), grid.radius,
            float(max_distance), _p(pr), _p(row_start), P, rows, _p(tf), _p(moments), _p(count), _p(status), _p(ws),
            nbytes, _stream()), "d3f_pair_information")
    return moments, count, status


# ---------------------------------------------------------------------------------------------------------------
# multiway registration: robust pose-graph optimisation over the fragments of a scene (Open3D's global_optimization)
# ---------------------------------------------------------------------------------------------------------------
def _graph_starts(start, count, device, name):
    """``node_start`` / ``edge_start`` -> (int32 device tensor [G+1], host array or None).  None: one graph."""
    if isinstance(start, torch.Tensor) and start.is_cuda:
        return start.to(torch.int32).contiguous().view(-1), None
    host = np.asarray([0, count] if start is None else (start.cpu() if isinstance(start, torch.Tensor) else start),
                      dtype=np.int64).reshape(-1)
    if host.size < 2 or host[0] != 0 or host[-1] != count or (np.diff(host) < 0).any():
        raise ValueError("%s must rise from 0 to %d, got %s" % (name, count, host.tolist()))
    return torch.as_tensor(host.astype(np.int32), device=device), host


def _pose_graph_inputs(poses, edges, T, info, uncertain, node_start, edge_start, max_nodes, max_edges, device):
    """The arguments of d3f_pose_graph_optimize on ``device`` (a torch device; the host twin takes 'cpu')."""
    ps = torch.as_tensor(poses, dtype=torch.float64).to(device).contiguous()
    if ps.dim() != 3 or tuple(ps.shape[1:]) != (4, 4):
        raise ValueError("poses must be [N,4,4], got %s" % (tuple(ps.shape),))
    N = int(ps.shape[0])
    on_device = isinstance(edges, torch.Tensor) and edges.is_cuda
    if on_device:
        ed = edges.to(torch.int32).contiguous().view(-1, 2)
    else:
        host = np.asarray(edges.cpu() if isinstance(edges, torch.Tensor) else edges, dtype=np.int64).reshape(-1, 2)
        ed = torch.as_tensor(host.astype(np.int32)).to(device)
    E = int(ed.shape[0])
    Z = torch.as_tensor(T, dtype=torch.float64).to(device).contiguous()
    L = torch.as_tensor(info, dtype=torch.float64).to(device).contiguous()
    if tuple(Z.shape) != (E, 4, 4) or tuple(L.shape) != (E, 6, 6):
        raise ValueError("T must be [E,4,4] and info [E,6,6] for the %d edges, got %s and %s"
                         % (E, tuple(Z.shape), tuple(L.shape)))
    un = torch.as_tensor(uncertain).to(device).to(torch.int32).contiguous().view(-1)
    if int(un.numel()) != E:
        raise ValueError("uncertain must hold one flag per edge")
    ns, ns_host = _graph_starts(node_start, N, device, "node_start")
    es, es_host = _graph_starts(edge_start, E, device, "edge_start")
    G = int(ns.numel()) - 1
    if int(es.numel()) - 1 != G:
        raise ValueError("node_start and edge_start must delimit the same number of graphs")
    if max_nodes is None:
        if ns_host is None:
            raise ValueError("max_nodes is required with a device node_start")
        max_nodes = int(np.diff(ns_host).max())
    if max_edges is None:
        if es_host is None:
            raise ValueError("max_edges is required with a device edge_start")
        max_edges = int(np.diff(es_host).max())
    if int(max_nodes) > PG_MAX_NODES:
        raise ValueError("a graph holds at most %d nodes, got %d" % (PG_MAX_NODES, int(max_nodes)))
    if not on_device and ns_host is not None and es_host is not None:    # host edges are checked here
        for g in range(G):
            e = host[es_host[g]:es_host[g + 1]]
            n = int(ns_host[g + 1] - ns_host[g])
            if e.size and (e.min() < 0 or e.max() >= n or (e[:, 0] == e[:, 1]).any()):
                raise ValueError("graph %d: edges must join two different nodes in 0..%d" % (g, n - 1))
    return ps, ed, Z, L, un, ns, es, G, N, E, int(max_nodes), int(max_edges)


def _pose_graph_call(fn, name, device, stream, poses, edges, T, info, uncertain, max_distance, node_start, edge_start,
                     preference_loop_closure, prune_threshold, max_iters, step_tol, rel_cost, max_nodes, max_edges):
    if not (0.0 < float(max_distance) < float("inf")):
        raise ValueError("max_distance must be positive and finite")
    if not 0 <= int(max_iters) <= PG_MAX_ITERS:
        raise ValueError("max_iters must be in 0..%d" % PG_MAX_ITERS)
    if not (0.0 < float(preference_loop_closure) < float("inf")) or not 0.0 <= float(prune_threshold) <= 1.0:
        raise ValueError("preference_loop_closure must be positive and finite, prune_threshold in 0..1")
    if not float(step_tol) >= 0.0 or not float(rel_cost) >= 0.0:
        raise ValueError("step_tol and rel_cost must be non-negative")
    ps, ed, Z, L, un, ns, es, G, N, E, max_nodes, max_edges = _pose_graph_inputs(
        poses, edges, T, info, uncertain, node_start, edge_start, max_nodes, max_edges, device)
    out = torch.empty_like(ps)
    weight = torch.empty(E, dtype=torch.float64, device=device)
    pruned = torch.empty(E, dtype=torch.int32, device=device)
    component = torch.empty(N, dtype=torch.int32, device=device)
    iterations = torch.empty((G, 2), dtype=torch.int32, device=device)
    cost = torch.empty((G, 3), dtype=torch.float64, device=device)
    status = torch.empty(G, dtype=torch.int32, device=device)
    nbytes = _native.lib().d3f_pose_graph_optimize_ws_bytes(G, max_nodes, max_edges)
    ws = _ws(nbytes, device)
    with _region("%s[G=%d,N=%d,E=%d]" % (name[4:], G, N, E)):
        _native.check(fn(_p(ns), _p(es), G, N, E, max_nodes, max_edges, _p(ps), _p(ed), _p(Z), _p(L), _p(un),
                         float(max_distance), float(preference_loop_closure), float(prune_threshold), int(max_iters),
                         float(step_tol), float(rel_cost), _p(out), _p(weight), _p(pruned), _p(component),
                         _p(iterations), _p(cost), _p(status), _p(ws), nbytes, stream), name)
    return out, weight, pruned, component, iterations, cost, status


def pose_graph_optimize(poses, edges, T, info, uncertain, max_distance, node_start=None, edge_start=None,
                        preference_loop_closure=2.0, prune_threshold=0.25, max_iters=100, step_tol=1e-9, rel_cost=1e-9,
                        max_nodes=None, max_edges=None):
    """Robust pose-graph optimisation of G stacked fragment graphs, each carried by one workgroup
    (d3f_pose_graph_optimize): one consistent pose per fragment from the pair poses of a scene, with the false loop
    closures switched off by a line process and pruned.

    ``poses`` f64 [N,4,4]: initial pose of every node (fragment k into the frame of its component's reference node);
    ``edges`` [E,2] = (i, j) LOCAL to their graph -- host values (checked here) or a device int32 tensor (checked by
    the kernel: ``PG_ST_GRAPH``); ``T`` f64 [E,4,4] maps fragment j into fragment i (a ``gt.log`` key i_j, what
    ``ransac_rigid`` / ``icp_rigid`` with pairs (j, i) return); ``info`` f64 [E,6,6] in the project's default form
    (``registration.information_from_moments``); ``uncertain`` [E] flags the edges under the line process;
    ``max_distance``: the distance the information was computed at.  ``node_start`` / ``edge_start`` [G+1] delimit the
    graphs (None: one graph); as device tensors they come with the host bounds ``max_nodes`` / ``max_edges`` on one
    graph's size -- with device ``edges`` too that is the form a captured graph takes.  At most ``PG_MAX_NODES`` nodes
    per graph.

    Residual ``[D_t ; log(D_R)]`` of ``D = inv(T) inv(P_i) P_j`` under ``info``; uncertain edges weigh
    ``(mu / (mu + c))^2`` with ``mu = preference_loop_closure * max_distance^2 * mean info[0,0]``; Levenberg-Marquardt,
    then every uncertain edge below ``prune_threshold`` is pruned, the components are taken again and a second pass
    runs -- all in ONE launch (include/d3feat_hip.h has the damping schedule and the stopping rules ``step_tol``,
    ``rel_cost``, ``max_iters``).  The lowest node of every component of the active edges is fixed.

    Returns device tensors ``(poses [N,4,4] f64, weight [E] f64, pruned [E] int32, component [N] int32, iterations
    [G,2] int32, cost [G,3] f64 (initial, after pass 1, final), status [G] int32 (PG_ST_* bits))``.  An edge without
    correspondences (``info[0,0] <= 0``) or with a non-finite matrix is reported pruned.  Bit-identical from run to run
    and for a graph alone or inside any batch; no read-back, no floating-point atomics."""
    dev = poses.device if isinstance(poses, torch.Tensor) and poses.is_cuda else torch.device("cuda")
    if not torch.cuda.is_available():
        raise RuntimeError("pose_graph_optimize needs the GPU (d3feat_pytorch_amd has no CPU path; the host twin is "
                           "pose_graph_optimize_host)")
    return _pose_graph_call(_native.lib().d3f_pose_graph_optimize, "d3f_pose_graph_optimize", dev, _stream(), poses,
                            edges, T, info, uncertain, max_distance, node_start, edge_start, preference_loop_closure,
                            prune_threshold, max_iters, step_tol, rel_cost, max_nodes, max_edges)


def pose_graph_optimize_host(poses, edges, T, info, uncertain, max_distance, node_start=None, edge_start=None,
                             preference_loop_closure=2.0, prune_threshold=0.25, max_iters=100, step_tol=1e-9,
                             rel_cost=1e-9, max_nodes=None, max_edges=None):
    """The host twin of ``pose_graph_optimize`` (d3f_pose_graph_optimize_host): the same text as the kernel run by one
    worker on the CPU, for tests -- host arrays / CPU tensors in, CPU tensors out, no GPU call."""
    global _PROFILER
    prof, _PROFILER = _PROFILER, None      # a region records device events
    try:
        return _pose_graph_call(_native.lib().d3f_pose_graph_optimize_host, "d3f_pose_graph_optimize_host",
                                torch.device("cpu"), None, poses, edges, T, info, uncertain, max_distance, node_start,
                                edge_start, preference_loop_closure, prune_threshold, max_iters, step_tol, rel_cost,
                                max_nodes, max_edges)
    finally:
        _PROFILER = prof


# ---------------------------------------------------------------------------------------------------------------
# TSDF fusion of depth frames into dense volumes, and their zero crossings as point clouds (csrc/tsdf.hpp)
# ---------------------------------------------------------------------------------------------------------------
TSDF_DEPTH_MAX = 6.0          # default depth_max in metres: farther pixels are not fused
TSDF_ST_OVERFLOW = _native.D3F_TSDF_ST_OVERFLOW
TSDF_MAX_VOLUMES = _native.D3F_TSDF_MAX_VOLUMES


def _tsdf_depth_array(depth, device_ok=False):
    """Depth frames as a host array [F,H,W], uint16 raw units or f32 metres (other floats become f32).  With
    ``device_ok`` a device f32 tensor [F,H,W] is passed through as it is (no copy to the host): what ``tsdf_raycast``
    returns goes straight into ``depth_pyramid``."""
    if device_ok and isinstance(depth, torch.Tensor) and depth.is_cuda and depth.dtype == torch.float32:
        if depth.dim() != 3:
            raise ValueError("depth must be [F,H,W], got %s" % (tuple(depth.shape),))
        return depth.detach().contiguous()
    if isinstance(depth, torch.Tensor):
        t = depth.detach().cpu()
        depth = t.view(torch.int16).numpy().view(np.uint16) if t.dtype in (torch.int16, torch.uint16) else t.numpy()
    a = np.asarray(depth)
    if a.dtype != np.uint16:
        if a.dtype.kind != 'f':
            raise ValueError("depth must be uint16 raw units or floating-point metres, got %s" % a.dtype)
        a = a.astype(np.float32, copy=False)
    if a.ndim != 3:
        raise ValueError("depth must be [F,H,W], got %s" % (a.shape,))
    return np.ascontiguousarray(a)


def _tsdf_frames(depth, frame_start, intrinsics, matrices):
    """Host form of the frame arguments: (depth [F,H,W], frame_start int32 [V+1], K f32 [F,4], matrices f32 [F,12])."""
    d = _tsdf_depth_array(depth)
    F = d.shape[0]
    fs = np.asarray(frame_start, dtype=np.int64).reshape(-1)
    if fs.size < 2 or fs[0] < 0 or fs[-1] > F or (np.diff(fs) < 0).any():
        raise ValueError("frame_start must rise within 0..%d, got %s" % (F, fs.tolist()))
    if fs.size - 1 > TSDF_MAX_VOLUMES:
        raise ValueError("at most %d volumes per call" % TSDF_MAX_VOLUMES)
    K = np.asarray(intrinsics.cpu() if isinstance(intrinsics, torch.Tensor) else intrinsics, dtype=np.float32)
    K = np.ascontiguousarray(np.broadcast_to(K.reshape(-1, 4), (F, 4)))
    m = np.asarray(matrices.cpu() if isinstance(matrices, torch.Tensor) else matrices)
    if m.ndim == 3 and m.shape[1:] in ((4, 4), (3, 4)):
        m = m[:, :3, :]
    m = np.ascontiguousarray(m.astype(np.float32).reshape(-1, 12))        # rounded to f32 once, here
    if m.shape[0] != F:
        raise ValueError("%d frame matrices for %d frames" % (m.shape[0], F))
    return d, fs.astype(np.int32), K, m


def _tsdf_volumes(origin, dims, voxel, V, trunc=None):
    """Host form of the volume arguments: (origin f32 [V,3], dims int32 [V,3], voxel f32 [V], trunc f32 [V] or None,
    vol_start int64 [V+1])."""
    def host(a):
        return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    o = np.ascontiguousarray(np.asarray(host(origin), dtype=np.float32).reshape(-1, 3))
    n = np.ascontiguousarray(np.asarray(host(dims), dtype=np.int64).reshape(-1, 3))
    if o.shape[0] != V or n.shape[0] != V:
        raise ValueError("origin and dims must hold one row per volume (%d)" % V)
    if (n < 1).any() or (n > 0x7fffffff).any():
        raise ValueError("every lattice dimension must be at least 1, got %s" % n.tolist())
    vx = np.ascontiguousarray(np.broadcast_to(np.asarray(host(voxel), dtype=np.float32).reshape(-1), (V,)))
    if not (vx > 0).all():
        raise ValueError("voxel sizes must be positive")
    tr = None
    if trunc is not None:
        tr = np.ascontiguousarray(np.broadcast_to(np.asarray(host(trunc), dtype=np.float32).reshape(-1), (V,)))
        if not (tr > 0).all():
            raise ValueError("truncation distances must be positive")
    vol_start = np.zeros(V + 1, dtype=np.int64)
    vol_start[1:] = np.cumsum([int(a) * int(b) * int(c) for a, b, c in n])
    return o, n.astype(np.int32), vx, tr, vol_start


def _on(device, *arrays):
    out = []
    for a in arrays:
        a = a if a.flags.writeable else a.copy()
        t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)
        out.append(t.to(device).contiguous())
    return out


def _tsdf_device():
    if not torch.cuda.is_available():
        raise RuntimeError("the TSDF kernels need the GPU (d3feat_pytorch_amd has no CPU path; the host twins are "
                           "tsdf_*_host, the NumPy restatement tsdf_numpy)")
    return torch.device("cuda")


def _tsdf_bounds(fn, name, device, stream, depth, frame_start, intrinsics, camera_to_volume, depth_scale, depth_max):
    d, fs, K, C = _tsdf_frames(depth, frame_start, intrinsics, camera_to_volume)
    V = fs.size - 1
    if d.shape[0] > 65535:
        raise ValueError("at most 65535 frames per call")
    td, tfs, tK, tC = _on(device, d, fs, K, C)
    bounds = torch.empty((V, 6), dtype=torch.float32, device=device)
    _native.check(fn(_p(td), int(d.dtype != np.uint16), d.shape[0], d.shape[1], d.shape[2], _p(tfs), V, _p(tK), _p(tC),
                     float(depth_scale), float(depth_max), _p(bounds), stream), name)
    return bounds


def tsdf_bounds(depth, frame_start, intrinsics, camera_to_volume, depth_scale=1000.0, depth_max=TSDF_DEPTH_MAX):
    """f32 [V,6] on the device: per volume the minimum (3) and maximum (3), in the volume's frame, of the back-projected
    valid pixels of its frames (d3f_tsdf_bounds; +inf / -inf for a volume without one).  ``camera_to_volume`` [F,3,4] /
    [F,4,4]: the inverses of ``tsdf_integrate``'s matrices, rounded to f32 here.  Exact (integer-ordered min / max)."""
    dev = _tsdf_device()
    with _region("tsdf_bounds"):
        return _tsdf_bounds(_native.lib().d3f_tsdf_bounds, "d3f_tsdf_bounds", dev, _stream(), depth, frame_start,
                            intrinsics, camera_to_volume, depth_scale, depth_max)


def tsdf_bounds_host(depth, frame_start, intrinsics, camera_to_volume, depth_scale=1000.0, depth_max=TSDF_DEPTH_MAX):
    """The host twin of ``tsdf_bounds`` (d3f_tsdf_bounds_host): CPU tensor out, no GPU call."""
    return _tsdf_bounds(_native.lib().d3f_tsdf_bounds_host, "d3f_tsdf_bounds_host", torch.device("cpu"), None, depth,
                        frame_start, intrinsics, camera_to_volume, depth_scale, depth_max)


def tsdf_color_frames(color, shape, channels=None):
    """The colour frames of depth frames of ``shape`` [F,H,W] as the TSDF kernels read them (csrc/tsdf_color.hpp): a host
    f32 array [F,H,W,Cc].  ``color``: uint8 [F,H,W,3] (R, G, B) gives Cc = 3, ``f32(c) / 255`` per channel, or with
    ``channels=1`` the intensity ``((0.299 R + 0.587 G) + 0.114 B) / 255``; uint8 [F,H,W] gives ``v / 255``, Cc = 1;
    floating point [F,H,W], [F,H,W,1] or [F,H,W,3] is taken as it is (f32).  The Cc = 1 forms are level 0 of
    ``rgbd_pyramid(...).intensity`` bit for bit: a model fused from them holds what the tracker compares."""
    c = color.detach().cpu().numpy() if isinstance(color, torch.Tensor) else np.asarray(color)
    shape = tuple(int(a) for a in shape)
    f32 = np.float32
    if c.dtype == np.uint8 and c.shape == shape + (3,):
        c = c.astype(f32)
        if channels == 1:
            c = (((f32(0.299) * c[..., 0] + f32(0.587) * c[..., 1]) + f32(0.114) * c[..., 2]) / f32(255.0))[..., None]
        else:
            c = c / f32(255.0)
    elif c.dtype == np.uint8 and c.shape == shape:
        c = (c.astype(f32) / f32(255.0))[..., None]
    elif c.dtype.kind == 'f' and c.shape == shape:
        c = c.astype(f32, copy=False)[..., None]
    elif c.dtype.kind == 'f' and c.shape in (shape + (1,), shape + (3,)):
        c = c.astype(f32, copy=False)
    else:
        raise ValueError("color must be uint8 [F,H,W,3] (R, G, B), uint8 [F,H,W] or floating point [F,H,W], [F,H,W,1] "
                         "or [F,H,W,3] for depth frames of shape %s, got %s of shape %s" % (shape, c.dtype, c.shape))
    if channels is not None and c.shape[-1] != int(channels):
        raise ValueError("the colour frames give %d channels, %d were asked for" % (c.shape[-1], int(channels)))
    return np.ascontiguousarray(c)


def _tsdf_into(into, total, device, channels=0, what="voxels"):
    """The (D, w) of ``into=``: f32 tensors of ``total`` voxels on ``device``, contiguous -- they are written in place.
    ``channels`` > 0: the triple (D, w, Cv), Cv holding ``channels`` values per voxel."""
    if channels:
        if not isinstance(into, (tuple, list)) or len(into) != 3:
            raise ValueError("into must be the triple (D, w, Cv) of an earlier integration with color=")
    elif not isinstance(into, (tuple, list)) or len(into) != 2:
        raise ValueError("into must be the pair (D, w) of an earlier integration")
    for name, t, per in zip(("D", "w", "Cv"), into, (1, 1, channels)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("into: %s must be a contiguous float32 tensor" % name)
        if t.device.type != torch.device(device).type:
            raise ValueError("into: %s is on %s, the call runs on %s" % (name, t.device, device))
        if int(t.numel()) != total * per:
            raise ValueError("into: %s holds %d values, the %d %s give %d" % (name, t.numel(), total, what, total * per))
    return tuple(into)


def _tsdf_integrate(host, device, depth, frame_start, intrinsics, volume_to_camera, volumes, trunc, depth_scale,
                    depth_max, into, color):
    """Every integrate form: d3f_tsdf[_sparse]_integrate[_host], its ``channels`` and its ``into``.  ``volumes``:
    ``(origin, dims, voxel)`` of dense volumes, or a ``SparseVolumes``; what depends on which is the tables in the
    argument list and the shape of the outputs."""
    d, fs, K, M = _tsdf_frames(depth, frame_start, intrinsics, volume_to_camera)
    V = fs.size - 1
    sparse = isinstance(volumes, SparseVolumes)
    if sparse and V != volumes.volumes:
        raise ValueError("frame_start names %d volumes, the sparse volumes are %d" % (V, volumes.volumes))
    origin, dims, voxel = (volumes.origin, volumes.dims, volumes.voxel) if sparse else volumes
    o, n, vx, tr, vol_start = _tsdf_volumes(origin, dims, voxel, V, trunc)
    c = None if color is None else tsdf_color_frames(color, d.shape)
    Cc = 0 if c is None else c.shape[-1]
    td, tfs, tK, tM, ttr = _on(device, d, fs, K, M, tr)
    if sparse:
        _, bs, _, bc, to, tn, tvx = _sparse_tables(volumes, device)
        B = volumes.bricks
        shape, what = (B, TSDF_BRICK_VOXELS), "slots of the allocated bricks"
        head, tail = (V,), (_p(bs), _p(bc) if B else None, B)
    else:
        to, tn, tvx, tvs = _on(device, o, n, vx, vol_start)
        shape, what = (int(vol_start[-1]),), "voxels"
        head, tail = (_p(tvs), V, shape[0], int(np.diff(vol_start).max())), ()
    cells = int(np.prod(shape))
    if into is None:
        D = torch.empty(shape, dtype=torch.float32, device=device)
        w = torch.empty(shape, dtype=torch.float32, device=device)
        Cv = torch.empty(shape + (Cc,), dtype=torch.float32, device=device) if Cc else None
    else:
        D, w, Cv = (_tsdf_into(into, cells, device, Cc, what) + (None,))[:3]
    ptr = _p if cells else (lambda t: None)
    name = "d3f_tsdf" + ("_sparse" if sparse else "") + "_integrate" + ("_host" if host else "")
    tc = _on(device, c)[0] if Cc else None                     # Cc = 0: null colour pointers, which are not looked at
    args = ((_p(td), _p(tc), Cc, int(d.dtype != np.uint16), d.shape[0], d.shape[1], d.shape[2], _p(tfs)) + head +
            (_p(tK), _p(tM), _p(to), _p(tn), _p(tvx), _p(ttr)) + tail +
            (float(depth_scale), float(depth_max), int(into is not None), ptr(D), ptr(w), ptr(Cv),
             None if host else _stream()))
    _native.check(getattr(_native.lib(), name)(*args), name)
    return (D, w) + (() if sparse else (tvs,)) + ((Cv,) if Cc else ())


def tsdf_integrate(depth, frame_start, intrinsics, volume_to_camera, origin, dims, voxel, trunc, depth_scale=1000.0,
                   depth_max=TSDF_DEPTH_MAX, into=None, color=None):
    """Fuse depth frames into V dense volumes in ONE launch (d3f_tsdf_integrate; the rule is csrc/tsdf.hpp).

    ``depth`` [F,H,W] uint16 raw units (metres = raw / ``depth_scale``) or f32 metres; ``frame_start`` [V+1]: volume v
    owns the frames ``[frame_start[v], frame_start[v+1])``; ``intrinsics`` [4] or [F,4] = fx, fy, cx, cy;
    ``volume_to_camera`` [F,3,4] / [F,4,4] (f64 is rounded to f32 once, here); ``origin`` [V,3], ``dims`` [V,3] = nx,
    ny, nz (host values), ``voxel`` and ``trunc`` a number or [V].  Returns device tensors ``(D f32 [total], w f32
    [total], vol_start int64 [V+1])``: volume v is ``D[vol_start[v]:vol_start[v+1]].view(nz, ny, nx)``.  One thread owns
    a voxel for all frames: written once, no atomics, bit-identical from run to run and to the host twin.

    ``into=(D, w)``: device tensors of an earlier call over the same ``origin`` / ``dims`` / ``voxel`` / ``trunc``; the
    frames are integrated into them IN PLACE (d3f_tsdf_integrate, into = 1) and the same tensors are returned.  The
    running mean is sequential over frames, so the frames [0, k) and then [k, F) ``into`` the result give the volume of
    one call over [0, F) bit for bit.  A volume that owns no frame in the call keeps its values.

    ``color=frames`` (what ``tsdf_color_frames`` takes: uint8 RGB gives 3 channels, uint8 grey or f32 [F,H,W] one)
    fuses the colour beside D and w (d3f_tsdf_integrate, channels = Cc; the rule is csrc/tsdf_color.hpp) and returns
    ``(D, w, vol_start, Cv f32 [total, Cc])``.  There is ONE weight: on exactly the frames that update a voxel's D and
    w, with the w from before the increment, ``c = (c w + c_pixel) / (w + 1)`` per channel, ``c_pixel`` read bilinearly
    over the 2 x 2 pixels around the voxel's projection (the depth is read at the nearest of them); D and w are the
    colourless call's bit for bit.  A non-finite colour value propagates into the voxels that have it among their four.  ``into=(D, w, Cv)`` continues all three."""
    dev = _tsdf_device()
    with _region("tsdf_integrate"):
        return _tsdf_integrate(False, dev, depth, frame_start, intrinsics, volume_to_camera, (origin, dims, voxel),
                               trunc, depth_scale, depth_max, into, color)


def tsdf_integrate_host(depth, frame_start, intrinsics, volume_to_camera, origin, dims, voxel, trunc,
                        depth_scale=1000.0, depth_max=TSDF_DEPTH_MAX, into=None, color=None):
    """The host twin of ``tsdf_integrate`` (d3f_tsdf_integrate_host): CPU tensors out (``into``: CPU tensors, written
    in place), no GPU call."""
    return _tsdf_integrate(True, torch.device("cpu"), depth, frame_start, intrinsics, volume_to_camera,
                           (origin, dims, voxel), trunc, depth_scale, depth_max, into, color)


def _pool_tensors(D, w, device):
    """D and w as the extract and mesh functions take them -- tensors, arrays or lists, wherever they are -- as flat
    float32 tensors on ``device``, named as ``_dense_model`` / ``_sparse_model`` want them."""
    D, w = (torch.from_numpy(np.array(a, dtype=np.float32)) if isinstance(a, np.ndarray) else
            torch.as_tensor(a, dtype=torch.float32) for a in (D, w))
    return ("D", D.to(device).contiguous().view(-1)), ("w", w.to(device).contiguous().view(-1))


def _tsdf_extract_inputs(D, w, origin, dims, voxel, device):
    (_, D), (_, w) = _pool_tensors(D, w, device)
    V = int(np.asarray(dims.cpu() if isinstance(dims, torch.Tensor) else dims).reshape(-1, 3).shape[0])
    o, n, vx, _, vol_start = _tsdf_volumes(origin, dims, voxel, V)
    total = int(vol_start[-1])
    if int(D.numel()) != total or int(w.numel()) != total:
        raise ValueError("D and w must hold the %d voxels of dims, got %d and %d" % (total, D.numel(), w.numel()))
    if total == 0 or V > TSDF_MAX_VOLUMES:
        raise ValueError("between 1 and %d volumes per call" % TSDF_MAX_VOLUMES)
    return (D, w, V, total) + tuple(_on(device, o, n, vx, vol_start))


def _check_vol_start(vol_start, expected):
    """A host ``vol_start`` is compared with the prefix of dims; a device one is not read back."""
    if vol_start is None or (isinstance(vol_start, torch.Tensor) and vol_start.is_cuda):
        return
    if not np.array_equal(np.asarray(vol_start, dtype=np.int64).reshape(-1), expected.cpu().numpy()):
        raise ValueError("vol_start is not the voxel prefix of dims")


def tsdf_extract(D, w, vol_start, origin, dims, voxel, min_weight=1.0, capacity=None, return_status=False):
    """The zero crossings of V volumes as one stacked cloud (d3f_tsdf_extract): ``(points f32 [M,3], point_start int64
    [V+1])`` on the device, in the order volume, lattice index of the lower voxel, axis -- a pure function of the
    volumes.  ``D``, ``w``, ``vol_start`` as ``tsdf_integrate`` returns them (a device ``vol_start`` is taken to be the
    prefix of ``dims``, which are host values).  A voxel counts when ``w >= min_weight`` and ``|D| < 1``.

    ONE read-back: the count pass and the scan run first, the number of points is read from the device, exactly that
    many rows are allocated and the emit pass fills them.  With ``capacity`` given nothing is read back: the three steps
    run back to back into ``capacity`` rows, points beyond it are dropped and TSDF_ST_OVERFLOW is set in the status word
    (``return_status=True`` appends it as a device int32 [1] tensor; ``point_start`` is complete either way)."""
    dev = _tsdf_device()
    return _tsdf_extract(False, dev, _dense_model(False, dev, _pool_tensors(D, w, dev), vol_start, origin, dims, voxel),
                         min_weight, capacity, return_status)


def tsdf_extract_host(D, w, vol_start, origin, dims, voxel, min_weight=1.0, capacity=None, return_status=False):
    """The host twin of ``tsdf_extract`` (d3f_tsdf_extract_host): CPU tensors out, no GPU call."""
    cpu = torch.device("cpu")
    return _tsdf_extract(True, cpu, _dense_model(True, cpu, _pool_tensors(D, w, cpu), vol_start, origin, dims, voxel),
                         min_weight, capacity, return_status)


def _lattice_axes(local, n, o, vx):
    """f32 lattice coordinates (x, y, z) and integer (ix, iy, iz) of the local voxel indices ``local`` of a lattice."""
    nx, ny = int(n[0]), int(n[1])
    ix, row = local % nx, local // nx
    iy, iz = row % ny, row // ny
    xyz = tuple(np.float32(o[a]) + np.float32(vx) * i.astype(np.float32) for a, i in enumerate((ix, iy, iz)))
    return xyz, (ix, iy, iz)


def _tsdf_fuse_numpy(xyz, d, K, M, f0, f1, trunc, depth_scale, depth_max, start=None, colour=None):
    """integrate_voxel of csrc/tsdf.hpp for the f32 lattice points ``xyz = (x, y, z)`` over the frames [f0, f1), from
    zero; ``start = (D, w)``: continuing from these values.  ``colour`` f32 [F,H,W,Cc]: integrate_voxel<Cc> (the
    colour rule is csrc/tsdf_color.hpp), ``start = (D, w, c)``, and (D, w, c [n,Cc]) is returned."""
    x, y, z = xyz
    H, W = d.shape[1:]
    f32 = np.float32
    scale, dmax, half, one = f32(depth_scale), f32(depth_max), f32(0.5), f32(1.0)
    c = None
    if start is None:
        D = np.zeros(x.shape, dtype=f32)
        w = np.zeros(x.shape, dtype=f32)
        if colour is not None:
            c = np.zeros(x.shape + (colour.shape[-1],), dtype=f32)
    elif colour is not None:
        D, w, c = start
    else:
        D, w = start
    with np.errstate(all='ignore'):
        for f in range(f0, f1):
            m = M[f]
            px = ((m[0] * x + m[1] * y) + m[2] * z) + m[3]
            py = ((m[4] * x + m[5] * y) + m[6] * z) + m[7]
            pz = ((m[8] * x + m[9] * y) + m[10] * z) + m[11]
            ok = pz > 0
            u = np.floor(((K[f, 0] * px) / pz + K[f, 2]) + half)
            r = np.floor(((K[f, 1] * py) / pz + K[f, 3]) + half)
            ok &= (u >= 0) & (u < f32(W)) & (r >= 0) & (r < f32(H))
            rr, uu = np.where(ok, r, 0).astype(np.int64), np.where(ok, u, 0).astype(np.int64)
            raw = d[f][rr, uu]
            dm = raw.astype(f32) / scale if raw.dtype == np.uint16 else raw
            ok &= (dm > 0) & ~(dm > dmax)
            sdf = dm - pz
            ok &= ~(sdf < -trunc)
            t = np.minimum(one, sdf / trunc)
            if c is not None:       # with the w from before the increment; bilinear at the unrounded projection
                uf = np.where(ok, (K[f, 0] * px) / pz + K[f, 2], 0).astype(f32)
                vf = np.where(ok, (K[f, 1] * py) / pz + K[f, 3], 0).astype(f32)
                u0, v0 = np.floor(uf), np.floor(vf)
                a, b = (uf - u0)[..., None], (vf - v0)[..., None]
                iu, iv = u0.astype(np.int64), v0.astype(np.int64)
                c0, c1 = np.maximum(iu, 0), np.minimum(iu + 1, W - 1)
                r0, r1 = np.maximum(iv, 0), np.minimum(iv + 1, H - 1)
                im = colour[f]
                cp = ((im[r0, c0] * (one - a) + im[r0, c1] * a) * (one - b)
                      + (im[r1, c0] * (one - a) + im[r1, c1] * a) * b)
                c = np.where(ok[..., None], (c * w[..., None] + cp) / (w + one)[..., None], c)
            D = np.where(ok, (D * w + t) / (w + one), D)
            w = np.where(ok, w + one, w)
    return (D, w) if c is None else (D, w, c.astype(f32, copy=False))


def tsdf_numpy(depth, frame_start, intrinsics, volume_to_camera, origin, dims, voxel, trunc, depth_scale=1000.0,
               depth_max=TSDF_DEPTH_MAX, chunk=1 << 21, into=None, color=None):
    """The contract of ``tsdf_integrate`` in NumPy: ``(D f32 [total], w f32 [total], vol_start int64 [V+1])``.  Every
    product and sum is spelled out in f32 in the order of csrc/tsdf.hpp (no ``@``), so the result equals the kernel's
    bit for bit.  ``chunk`` voxels are swept at a time.  ``into=(D, w)``: contiguous f32 arrays of an earlier call,
    written in place and returned, as ``tsdf_integrate`` does with its tensors.  ``color=``: the colour of
    csrc/tsdf_color.hpp beside them, ``(D, w, vol_start, Cv f32 [total, Cc])``; ``into=(D, w, Cv)``."""
    d, fs, K, M = _tsdf_frames(depth, frame_start, intrinsics, volume_to_camera)
    V = fs.size - 1
    o, n, vx, tr, vol_start = _tsdf_volumes(origin, dims, voxel, V, trunc)
    total = int(vol_start[-1])
    c = None if color is None else tsdf_color_frames(color, d.shape)
    Cc = 0 if c is None else c.shape[-1]
    if into is None:
        arrays = [np.zeros(total, dtype=np.float32), np.zeros(total, dtype=np.float32)]
        if Cc:
            arrays.append(np.zeros((total, Cc), dtype=np.float32))
    else:
        arrays = _numpy_into(into, total, Cc, "voxels")
    for v in range(V):
        if into is not None and fs[v + 1] <= fs[v]:
            continue
        first, last = int(vol_start[v]), int(vol_start[v + 1])
        for s in range(first, last, int(chunk)):
            e = min(s + int(chunk), last)
            xyz, _ = _lattice_axes(np.arange(s, e, dtype=np.int64) - vol_start[v], n[v], o[v], vx[v])
            start = None if into is None else tuple(a[s:e].copy() for a in arrays)
            out = _tsdf_fuse_numpy(xyz, d, K, M, int(fs[v]), int(fs[v + 1]), tr[v], depth_scale, depth_max, start, c)
            for a, b in zip(arrays, out):
                a[s:e] = b
    return (arrays[0], arrays[1], vol_start) + ((arrays[2],) if Cc else ())


def _numpy_into(into, total, channels, what):
    """The arrays of a NumPy ``into=``, flat views [total] (and [total, channels]) of (D, w) or (D, w, Cv)."""
    if channels:
        if not isinstance(into, (tuple, list)) or len(into) != 3:
            raise ValueError("into must be the triple (D, w, Cv) of an earlier integration with color=")
    elif not isinstance(into, (tuple, list)) or len(into) != 2:
        raise ValueError("into must be the pair (D, w) of an earlier integration")
    for name, a, per in zip(("D", "w", "Cv"), into, (1, 1, channels)):
        if not isinstance(a, np.ndarray) or a.dtype != np.float32 or not a.flags.c_contiguous or \
                not a.flags.writeable or a.size != total * per:
            raise ValueError("into: %s must be a writeable contiguous float32 array of %d values (%d %s)"
                             % (name, total * per, total, what))
    out = [into[0].reshape(-1), into[1].reshape(-1)]
    if channels:
        out.append(into[2].reshape(total, channels))
    return out


def _order_keys(a):
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def _order_values(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7fffffff), ~k).astype(np.uint32).view(np.float32)


def tsdf_bounds_numpy(depth, frame_start, intrinsics, camera_to_volume, depth_scale=1000.0, depth_max=TSDF_DEPTH_MAX):
    """The contract of ``tsdf_bounds`` in NumPy: f32 [V,6], equal to the kernel's bit for bit."""
    d, fs, K, C = _tsdf_frames(depth, frame_start, intrinsics, camera_to_volume)
    V = fs.size - 1
    H, W = d.shape[1:]
    f32 = np.float32
    rows, cols = np.meshgrid(np.arange(H, dtype=f32), np.arange(W, dtype=f32), indexing='ij')
    lo = np.full((V, 3), 0xff800000, dtype=np.uint32)
    hi = np.full((V, 3), 0x007fffff, dtype=np.uint32)
    with np.errstate(all='ignore'):
        for v in range(V):
            for f in range(int(fs[v]), int(fs[v + 1])):
                dm = d[f].astype(f32) / f32(depth_scale) if d.dtype == np.uint16 else d[f]
                ok = (dm > 0) & ~(dm > f32(depth_max))
                if not ok.any():
                    continue
                X = ((cols - K[f, 2]) * dm) / K[f, 0]
                Y = ((rows - K[f, 3]) * dm) / K[f, 1]
                c = C[f]
                for r in range(3):
                    q = ((c[4 * r] * X + c[4 * r + 1] * Y) + c[4 * r + 2] * dm) + c[4 * r + 3]
                    keys = _order_keys(q[ok])
                    lo[v, r] = min(lo[v, r], keys.min())
                    hi[v, r] = max(hi[v, r], keys.max())
    return np.concatenate([_order_values(lo), _order_values(hi)], axis=1)


def tsdf_extract_numpy(D, w, vol_start, origin, dims, voxel, min_weight=1.0):
    """The contract of ``tsdf_extract`` in NumPy: ``(points f32 [M,3], point_start int64 [V+1])``, equal to the
    kernel's bit for bit and in order."""
    D = np.ascontiguousarray(D, dtype=np.float32).reshape(-1)
    w = np.ascontiguousarray(w, dtype=np.float32).reshape(-1)
    V = int(np.asarray(dims).reshape(-1, 3).shape[0])
    o, n, vx, _, vs = _tsdf_volumes(origin, dims, voxel, V)
    if D.size != int(vs[-1]) or w.size != D.size:
        raise ValueError("D and w must hold the %d voxels of dims" % int(vs[-1]))
    out, point_start = [], np.zeros(V + 1, dtype=np.int64)
    with np.errstate(all='ignore'):
        for v in range(V):
            nx, ny, nz = (int(a) for a in n[v])
            Dv = D[vs[v]:vs[v + 1]].reshape(nz, ny, nx)
            ok = (w[vs[v]:vs[v + 1]].reshape(nz, ny, nx) >= np.float32(min_weight)) & (np.abs(Dv) < np.float32(1.0))
            neg = Dv < 0
            emit = np.zeros((nz, ny, nx, 3), dtype=bool)
            frac = np.zeros((nz, ny, nx, 3), dtype=np.float32)
            for a, (low, high) in enumerate(((np.s_[:, :, :-1], np.s_[:, :, 1:]), (np.s_[:, :-1, :], np.s_[:, 1:, :]),
                                             (np.s_[:-1, :, :], np.s_[1:, :, :]))):
                emit[low + (a,)] = ok[low] & ok[high] & (neg[low] != neg[high])
                a0, a1 = np.abs(Dv[low]), np.abs(Dv[high])
                frac[low + (a,)] = a0 / (a0 + a1)
            local, axis = np.nonzero(emit.reshape(-1, 3))          # row-major: lattice index, then axis
            xyz, _ = _lattice_axes(local.astype(np.int64), n[v], o[v], vx[v])
            pts = np.stack(xyz, axis=1).astype(np.float32)
            rows = np.arange(local.size)
            pts[rows, axis] = pts[rows, axis] + vx[v] * frac.reshape(-1, 3)[local, axis]
            out.append(pts)
            point_start[v + 1] = point_start[v] + local.size
    return (np.concatenate(out, 0) if out else np.zeros((0, 3), np.float32)), point_start


# ---------------------------------------------------------------------------------------------------------------
# sparse TSDF volumes: bricks of 8 x 8 x 8 voxels allocated only near a surface (csrc/tsdf_sparse.hpp)
# ---------------------------------------------------------------------------------------------------------------
TSDF_BRICK = 8                # voxels along a brick's edge
TSDF_BRICK_VOXELS = 512


class SparseVolumes(object):
    """The tables of a batch of sparse volumes, as ``tsdf_allocate`` returns them: ``brick_index`` int32 [L] (per lattice
    brick, bx fastest, volume after volume: its rank among the allocated bricks of its volume, or -1), ``brick_coord``
    int32 [B,3] = (bx, by, bz) of the allocated bricks in pool order, ``brick_start`` int64 [V+1] (the prefix of the
    allocated bricks over the volumes) -- device tensors from ``tsdf_allocate``, CPU tensors from the host twin, arrays
    from the restatement -- and the host arrays ``origin`` f32 [V,3], ``dims`` int32 [V,3], ``voxel`` f32 [V].  The pool
    row of lattice brick l of volume v is ``brick_start[v] + brick_index[lattice_start[v] + l]``."""
    __slots__ = ('brick_index', 'brick_coord', 'brick_start', 'origin', 'dims', 'voxel')

    def __init__(self, brick_index, brick_coord, brick_start, origin, dims, voxel):
        self.brick_index, self.brick_coord, self.brick_start = brick_index, brick_coord, brick_start
        self.origin, self.dims, self.voxel = origin, dims, voxel

    @property
    def volumes(self):
        return int(self.dims.shape[0])

    @property
    def bricks(self):
        return int(self.brick_coord.shape[0])

    @property
    def lattice_start(self):
        """int64 [V+1] (host): the prefix of the volumes' brick lattices ceil(n / 8)^3."""
        return _lattice_start(self.dims)


def _lattice_start(dims):
    nb = (np.asarray(dims, dtype=np.int64) + (TSDF_BRICK - 1)) // TSDF_BRICK
    out = np.zeros(nb.shape[0] + 1, dtype=np.int64)
    out[1:] = np.cumsum(nb[:, 0] * nb[:, 1] * nb[:, 2])
    return out


def _host_array(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def tsdf_sparse_bytes(sv, volume=None, channels=0):
    """The bytes of a batch of sparse volumes: the pool (D and w, 8 bytes per slot of an allocated brick, and 4 more per
    colour channel with ``channels``) plus the tables (``brick_index``, ``brick_coord``, ``brick_start``).  ``volume``:
    of that volume alone."""
    lattice, bricks, V = int(sv.lattice_start[-1]), sv.bricks, sv.volumes
    if volume is not None:
        lattice = int(np.diff(sv.lattice_start)[volume])
        bricks, V = int(np.diff(_host_array(sv.brick_start))[volume]), 1
    return (2 + int(channels)) * 4 * TSDF_BRICK_VOXELS * bricks + 4 * lattice + 12 * bricks + 8 * (V + 1)


def _tsdf_allocate(host, device, stream, depth, frame_start, intrinsics, camera_to_volume, origin, dims, voxel, trunc,
                   depth_scale, depth_max, existing=None):
    """``existing``: an int32 [L] ``brick_index`` on ``device`` whose bricks (entries >= 0) are flagged too, between the
    mark and the index launches (``tsdf_extend``)."""
    d, fs, K, C = _tsdf_frames(depth, frame_start, intrinsics, camera_to_volume)
    V = fs.size - 1
    o, n, vx, tr, _ = _tsdf_volumes(origin, dims, voxel, V, trunc)
    ls = _lattice_start(n)
    lattice = int(ls[-1])
    if lattice > 0x7fffffff:
        raise ValueError("the brick lattices of a call hold %d bricks, more than 2^31 - 1" % lattice)
    if not host and d.shape[0] > 65535:
        raise ValueError("at most 65535 frames per call")
    td, tfs, tK, tC, to, tn, tvx, ttr, tls = _on(device, d, fs, K, C, o, n, vx, tr, ls)
    flags = torch.empty(lattice, dtype=torch.int32, device=device)
    brick_index = torch.empty(lattice, dtype=torch.int32, device=device)
    coord = torch.empty((lattice, 3), dtype=torch.int32, device=device)
    brick_start = torch.zeros(V + 1, dtype=torch.int64, device=device)
    L = _native.lib()
    frames = (_p(td), int(d.dtype != np.uint16), d.shape[0], d.shape[1], d.shape[2], _p(tfs), V, _p(tK), _p(tC),
              _p(to), _p(tn), _p(tvx), _p(ttr), _p(tls), lattice, float(depth_scale), float(depth_max), _p(flags))
    if host:
        _native.check(L.d3f_tsdf_sparse_mark_host(*frames), "d3f_tsdf_sparse_mark_host")
        if existing is not None:
            flags.copy_(torch.maximum(flags, (existing >= 0).to(torch.int32)))
        _native.check(L.d3f_tsdf_sparse_index_host(_p(flags), _p(tls), _p(tn), V, lattice, _p(brick_index), _p(coord),
                                                   _p(brick_start)), "d3f_tsdf_sparse_index_host")
    else:
        nbytes = L.d3f_tsdf_sparse_index_ws_bytes(lattice)
        ws = _ws(nbytes, device)
        _native.check(L.d3f_tsdf_sparse_mark(*(frames + (stream,))), "d3f_tsdf_sparse_mark")
        if existing is not None:
            flags.copy_(torch.maximum(flags, (existing >= 0).to(torch.int32)))      # in place: same stream, no sync
        _native.check(L.d3f_tsdf_sparse_index(_p(flags), _p(tls), _p(tn), V, lattice, _p(brick_index), _p(coord),
                                              _p(brick_start), _p(ws), nbytes, stream), "d3f_tsdf_sparse_index")
    bricks = int(brick_start[V].item())                    # the one read-back: the number of allocated bricks
    return SparseVolumes(brick_index, coord[:bricks].clone(), brick_start, o, n, vx)


def tsdf_allocate(depth, frame_start, intrinsics, camera_to_volume, origin, dims, voxel, trunc, depth_scale=1000.0,
                  depth_max=TSDF_DEPTH_MAX):
    """The bricks of V sparse volumes (d3f_tsdf_sparse_mark, d3f_tsdf_sparse_index; the rule is csrc/tsdf_sparse.hpp): a
    ``SparseVolumes`` with device tables.  Every valid pixel of a volume's frames flags the bricks of 8 x 8 x 8 voxels
    that the box of its footprint over ``[max(d - trunc, 0), d + trunc]``, widened by one voxel, touches; the flags are
    scanned in lattice order.  The frame arguments are those of ``tsdf_bounds``, the volume arguments those of
    ``tsdf_integrate``.  ONE read-back: the number of allocated bricks."""
    dev = _tsdf_device()
    with _region("tsdf_allocate"):
        return _tsdf_allocate(False, dev, _stream(), depth, frame_start, intrinsics, camera_to_volume, origin, dims,
                              voxel, trunc, depth_scale, depth_max)


def tsdf_allocate_host(depth, frame_start, intrinsics, camera_to_volume, origin, dims, voxel, trunc,
                       depth_scale=1000.0, depth_max=TSDF_DEPTH_MAX):
    """The host twin of ``tsdf_allocate`` (d3f_tsdf_sparse_mark_host, d3f_tsdf_sparse_index_host): CPU tensors, no GPU
    call."""
    return _tsdf_allocate(True, torch.device("cpu"), None, depth, frame_start, intrinsics, camera_to_volume, origin,
                          dims, voxel, trunc, depth_scale, depth_max)


def _sparse_tables(sv, device):
    """(lattice_start, brick_start, brick_index, brick_coord, origin, dims, voxel) of ``sv`` as tensors on ``device``."""
    def tensor(a, dtype):
        a = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
        return a.to(device=device, dtype=dtype).contiguous()
    tls, to, tn, tvx = _on(device, sv.lattice_start, sv.origin, sv.dims, sv.voxel)
    bi, bc, bs = tensor(sv.brick_index, torch.int32), tensor(sv.brick_coord, torch.int32), tensor(sv.brick_start,
                                                                                                  torch.int64)
    if (int(bi.numel()) != int(sv.lattice_start[-1]) or tuple(bc.shape) != (sv.bricks, 3) or
            int(bs.numel()) != sv.volumes + 1):
        raise ValueError("the tables of the sparse volumes do not fit their dims")
    return tls, bs, bi, bc, to, tn, tvx


def tsdf_integrate_sparse(depth, frame_start, intrinsics, volume_to_camera, sv, trunc, depth_scale=1000.0,
                          depth_max=TSDF_DEPTH_MAX, into=None, color=None):
    """Fuse depth frames into the allocated bricks of ``sv`` in ONE launch (d3f_tsdf_sparse_integrate): device tensors
    ``(D f32 [B,512], w f32 [B,512])``, row b the brick ``sv.brick_coord[b]``, voxel (ix, iy, iz) at slot ``(ix & 7) + 8
    (iy & 7) + 64 (iz & 7)``.  Every slot inside the lattice holds what ``tsdf_integrate`` gives that voxel, bit for
    bit; a slot beyond ``dims`` holds 0.  The frame arguments and ``trunc`` are those of ``tsdf_integrate``.

    ``into=(D, w)``: the device pool of an earlier call over the same ``sv`` and ``trunc``; the frames are integrated
    into it IN PLACE (d3f_tsdf_sparse_integrate, into = 1; csrc/tsdf_raycast_sparse.hpp) and the same tensors are
    returned.  The frames [0, k) and then [k, F) ``into`` the result give the pool of one call over [0, F) bit for bit;
    the rows of a volume that owns no frame in the call keep their values.

    ``color=frames`` as for ``tsdf_integrate``: the colour pool ``Cp f32 [B,512,Cc]`` is fused beside D and w
    (d3f_tsdf_sparse_integrate, channels = Cc; csrc/tsdf_color.hpp) and ``(D, w, Cp)`` is returned; every slot inside
    the lattice holds the dense ``Cv`` of that voxel bit for bit, every other slot 0.  ``into=(D, w, Cp)`` continues all
    three."""
    dev = _tsdf_device()
    with _region("tsdf_integrate_sparse"):
        return _tsdf_integrate(False, dev, depth, frame_start, intrinsics, volume_to_camera, sv, trunc, depth_scale,
                               depth_max, into, color)


def tsdf_integrate_sparse_host(depth, frame_start, intrinsics, volume_to_camera, sv, trunc, depth_scale=1000.0,
                               depth_max=TSDF_DEPTH_MAX, into=None, color=None):
    """The host twin of ``tsdf_integrate_sparse`` (d3f_tsdf_sparse_integrate_host):
    CPU tensors out (``into``: CPU tensors, written in place), no GPU call."""
    return _tsdf_integrate(True, torch.device("cpu"), depth, frame_start, intrinsics, volume_to_camera, sv, trunc,
                           depth_scale, depth_max, into, color)


def _sparse_pool(D, w, sv, device):
    (_, D), (_, w) = _pool_tensors(D, w, device)
    if int(D.numel()) != sv.bricks * TSDF_BRICK_VOXELS or int(w.numel()) != int(D.numel()):
        raise ValueError("D and w must hold the %d x 512 slots of the allocated bricks, got %d and %d"
                         % (sv.bricks, D.numel(), w.numel()))
    return D, w


def tsdf_extract_sparse(D, w, sv, min_weight=1.0, capacity=None, return_status=False):
    """The zero crossings of sparse volumes as one stacked cloud (d3f_tsdf_sparse_extract): ``(points f32 [M,3],
    point_start int64 [V+1])`` on the device, in the order volume, brick in lattice order, slot, axis.  As a set of rows
    they are ``tsdf_extract``'s points of the dense volumes, bit for bit.  ``D``, ``w`` as ``tsdf_integrate_sparse``
    returns them; ``capacity``, ``return_status`` and the one read-back as for ``tsdf_extract``."""
    dev = _tsdf_device()
    return _tsdf_extract(False, dev, _sparse_model(False, dev, _pool_tensors(D, w, dev), sv), min_weight, capacity,
                         return_status)


def tsdf_extract_sparse_host(D, w, sv, min_weight=1.0, capacity=None, return_status=False):
    """The host twin of ``tsdf_extract_sparse`` (d3f_tsdf_sparse_extract_host): CPU tensors out, no GPU call."""
    cpu = torch.device("cpu")
    return _tsdf_extract(True, cpu, _sparse_model(True, cpu, _pool_tensors(D, w, cpu), sv), min_weight, capacity,
                         return_status)


def _slot_voxels(coord):
    """int64 [B,512] x 3: the voxel (ix, iy, iz) of every slot of the bricks ``coord`` [B,3]."""
    s = np.arange(TSDF_BRICK_VOXELS, dtype=np.int64)
    inside = (s & 7, (s >> 3) & 7, s >> 6)
    return tuple(coord[:, a, None].astype(np.int64) * TSDF_BRICK + inside[a][None, :] for a in range(3))


def tsdf_densify(D, w, sv, color=None):
    """A pool scattered into the dense layout of ``tsdf_integrate``: ``(D f32 [total], w f32 [total], vol_start int64
    [V+1])``, zero outside the allocated bricks, by plain indexing (tensors in, tensors on the same device out; arrays
    in, arrays out).  For tests, and for ``tsdf_mesh`` on a volume that fits.  ``color=Cp`` [B,512,Cc]: the dense colour
    ``Cv`` [total, Cc] is returned too, last."""
    arrays = isinstance(D, np.ndarray)
    dev = torch.device("cpu") if arrays else D.device
    Dp, wp = _sparse_pool(D, w, sv, dev)
    n = np.asarray(sv.dims, dtype=np.int64)
    vol_start = np.zeros(sv.volumes + 1, dtype=np.int64)
    vol_start[1:] = np.cumsum(n[:, 0] * n[:, 1] * n[:, 2])
    coord, bs = _host_array(sv.brick_coord), _host_array(sv.brick_start)
    vol = np.repeat(np.arange(sv.volumes), np.diff(bs))
    ix, iy, iz = _slot_voxels(coord)
    nv = n[vol]
    exists = (ix < nv[:, 0, None]) & (iy < nv[:, 1, None]) & (iz < nv[:, 2, None])
    at = vol_start[vol][:, None] + (iz * nv[:, 1, None] + iy) * nv[:, 0, None] + ix
    src = torch.from_numpy(np.flatnonzero(exists.reshape(-1))).to(dev)
    dst = torch.from_numpy(at[exists]).to(dev)
    out = []
    for pool in (Dp, wp):
        dense = torch.zeros(int(vol_start[-1]), dtype=torch.float32, device=dev)
        dense[dst] = pool[src]
        out.append(dense.numpy() if arrays else dense)
    res = (out[0], out[1], (vol_start if arrays else torch.from_numpy(vol_start).to(dev)))
    if color is not None:
        Cp = _sparse_color_pool(color, sv, dev)
        dense = torch.zeros((int(vol_start[-1]), Cp.shape[-1]), dtype=torch.float32, device=dev)
        dense[dst] = Cp.view(-1, Cp.shape[-1])[src]
        res += (dense.numpy() if arrays else dense,)
    return res


def _sparse_color_pool(Cp, sv, device):
    """A colour pool as a contiguous f32 tensor [B, 512, Cc] on ``device`` ([B,512] is one channel)."""
    Cp = torch.from_numpy(np.array(Cp, dtype=np.float32)) if isinstance(Cp, np.ndarray) else \
        torch.as_tensor(Cp, dtype=torch.float32)
    Cp = Cp.to(device).contiguous()
    slots = sv.bricks * TSDF_BRICK_VOXELS
    Cc = Cp.shape[-1] if Cp.dim() == 3 else 1
    if Cc not in (1, 3) or int(Cp.numel()) != slots * Cc:
        raise ValueError("the colour pool must be [%d, 512, 1 or 3], got %s" % (sv.bricks, tuple(Cp.shape)))
    return Cp.view(sv.bricks, TSDF_BRICK_VOXELS, Cc)


def tsdf_allocate_numpy(depth, frame_start, intrinsics, camera_to_volume, origin, dims, voxel, trunc,
                        depth_scale=1000.0, depth_max=TSDF_DEPTH_MAX):
    """The contract of ``tsdf_allocate`` in NumPy: a ``SparseVolumes`` of arrays, equal to the kernels' tables.  Every
    product and sum is spelled out in f32 in the order of csrc/tsdf_sparse.hpp."""
    d, fs, K, C = _tsdf_frames(depth, frame_start, intrinsics, camera_to_volume)
    V = fs.size - 1
    o, n, vx, tr, _ = _tsdf_volumes(origin, dims, voxel, V, trunc)
    H, W = d.shape[1:]
    f32 = np.float32
    half, one, zero = f32(0.5), f32(1.0), f32(0.0)
    rows, cols = np.meshgrid(np.arange(H, dtype=f32), np.arange(W, dtype=f32), indexing='ij')
    index, coords, brick_start = [], [], np.zeros(V + 1, dtype=np.int64)
    with np.errstate(all='ignore'):
        for v in range(V):
            nb = (n[v].astype(np.int64) + (TSDF_BRICK - 1)) // TSDF_BRICK
            flags = np.zeros((int(nb[2]), int(nb[1]), int(nb[0])), dtype=bool)
            for f in range(int(fs[v]), int(fs[v + 1])):
                dm = d[f].astype(f32) / f32(depth_scale) if d.dtype == np.uint16 else d[f]
                ok = (dm > 0) & ~(dm > f32(depth_max))
                near = dm - tr[v]
                z = (np.where(near > 0, near, zero), dm + tr[v])
                su = ((cols - half) - K[f, 2], (cols + half) - K[f, 2])
                sv = ((rows - half) - K[f, 3], (rows + half) - K[f, 3])
                c, lo, hi = C[f], None, None
                for corner in range(8):
                    zz = z[corner >> 2]
                    X = (su[corner & 1] * zz) / K[f, 0]
                    Y = (sv[(corner >> 1) & 1] * zz) / K[f, 1]
                    q = [((c[4 * r] * X + c[4 * r + 1] * Y) + c[4 * r + 2] * zz) + c[4 * r + 3] for r in range(3)]
                    lo = q if lo is None else [np.where(q[r] < lo[r], q[r], lo[r]) for r in range(3)]
                    hi = q if hi is None else [np.where(q[r] > hi[r], q[r], hi[r]) for r in range(3)]
                box = []
                for r in range(3):
                    last = f32(int(n[v, r]) - 1)
                    flo = np.floor((lo[r] - o[v, r]) / vx[v]) - one
                    fhi = np.floor((hi[r] - o[v, r]) / vx[v]) + one
                    ok &= (fhi >= 0) & (flo <= last)
                    box += [np.where(flo <= 0, zero, np.where(flo >= last, last, flo)),
                            np.where(fhi <= 0, zero, np.where(fhi >= last, last, fhi))]
                if not ok.any():
                    continue
                box = np.stack([b[ok] for b in box], axis=1).astype(np.int64)
                box = np.minimum(box, n[v].astype(np.int64).repeat(2)[None, :] - 1) >> 3    # f32(n - 1) may round up
                for x0, x1, y0, y1, z0, z1 in np.unique(box, axis=0):
                    flags[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1] = True
            flat = flags.reshape(-1)
            index.append(np.where(flat, np.cumsum(flat) - 1, -1).astype(np.int32))
            bz, by, bx = np.nonzero(flags)                          # row-major: lattice order
            coords.append(np.stack([bx, by, bz], axis=1).astype(np.int32))
            brick_start[v + 1] = brick_start[v] + bx.size
    return SparseVolumes(np.concatenate(index), np.concatenate(coords, 0).reshape(-1, 3), brick_start, o, n, vx)


def tsdf_sparse_numpy(depth, frame_start, intrinsics, volume_to_camera, sv, trunc, depth_scale=1000.0,
                      depth_max=TSDF_DEPTH_MAX, chunk=1 << 12, into=None, color=None):
    """The contract of ``tsdf_integrate_sparse`` in NumPy: ``(D f32 [B,512], w f32 [B,512])``, equal to the kernel's bit
    for bit: ``tsdf_numpy``'s arithmetic on the slots of the allocated bricks, ``chunk`` bricks at a time.
    ``into=(D, w)``: writeable contiguous f32 arrays [B,512] of an earlier call, continued in place and returned.
    ``color=``: ``(D, w, Cp f32 [B,512,Cc])`` (csrc/tsdf_color.hpp); ``into=(D, w, Cp)``."""
    d, fs, K, M = _tsdf_frames(depth, frame_start, intrinsics, volume_to_camera)
    V = fs.size - 1
    if V != sv.volumes:
        raise ValueError("frame_start names %d volumes, the sparse volumes are %d" % (V, sv.volumes))
    o, n, vx, tr, _ = _tsdf_volumes(sv.origin, sv.dims, sv.voxel, V, trunc)
    coord, bs = _host_array(sv.brick_coord), _host_array(sv.brick_start)
    c = None if color is None else tsdf_color_frames(color, d.shape)
    Cc = 0 if c is None else c.shape[-1]
    B = sv.bricks
    if into is None:
        pools = [np.zeros((B, TSDF_BRICK_VOXELS), dtype=np.float32), np.zeros((B, TSDF_BRICK_VOXELS), dtype=np.float32)]
        if Cc:
            pools.append(np.zeros((B, TSDF_BRICK_VOXELS, Cc), dtype=np.float32))
    else:
        pools = _numpy_into(into, B * TSDF_BRICK_VOXELS, Cc, "slots of the allocated bricks")
        pools = [a.reshape((B, TSDF_BRICK_VOXELS) + a.shape[1:]) for a in pools]
    for v in range(V):
        if into is not None and fs[v + 1] <= fs[v]:
            continue
        for s in range(int(bs[v]), int(bs[v + 1]), int(chunk)):
            e = min(s + int(chunk), int(bs[v + 1]))
            i = _slot_voxels(coord[s:e])
            exists = (i[0] < n[v, 0]) & (i[1] < n[v, 1]) & (i[2] < n[v, 2])
            xyz = tuple(np.float32(o[v, a]) + np.float32(vx[v]) * i[a][exists].astype(np.float32) for a in range(3))
            start = None if into is None else tuple(a[s:e][exists] for a in pools)
            out = _tsdf_fuse_numpy(xyz, d, K, M, int(fs[v]), int(fs[v + 1]), tr[v], depth_scale, depth_max, start, c)
            for a, b in zip(pools, out):
                a[s:e][exists] = b
    return tuple(pools) if into is None else tuple(into)


def tsdf_extract_sparse_numpy(D, w, sv, min_weight=1.0):
    """The contract of ``tsdf_extract_sparse`` in NumPy: ``(points f32 [M,3], point_start int64 [V+1])``, equal to the
    kernel's bit for bit and in order."""
    B, V = sv.bricks, sv.volumes
    D = np.ascontiguousarray(_host_array(D), dtype=np.float32).reshape(-1)
    w = np.ascontiguousarray(_host_array(w), dtype=np.float32).reshape(-1)
    if D.size != B * TSDF_BRICK_VOXELS or w.size != D.size:
        raise ValueError("D and w must hold the %d x 512 slots of the allocated bricks" % B)
    o, n, vx, _, _ = _tsdf_volumes(sv.origin, sv.dims, sv.voxel, V)
    index, coord, bs = (_host_array(a) for a in (sv.brick_index, sv.brick_coord, sv.brick_start))
    ls = sv.lattice_start
    out, point_start = [], np.zeros(V + 1, dtype=np.int64)
    face = (np.s_[:, :, :, 7], np.s_[:, :, 7, :], np.s_[:, 7, :, :]), (np.s_[:, :, :, 0], np.s_[:, :, 0, :],
                                                                       np.s_[:, 0, :, :])
    inner = ((np.s_[:, :, :, :-1], np.s_[:, :, :, 1:]), (np.s_[:, :, :-1, :], np.s_[:, :, 1:, :]),
             (np.s_[:, :-1, :, :], np.s_[:, 1:, :, :]))
    with np.errstate(all='ignore'):
        for v in range(V):
            rows = slice(int(bs[v]), int(bs[v + 1]))
            Bv = rows.stop - rows.start
            c = coord[rows].astype(np.int64)
            nb = (n[v].astype(np.int64) + (TSDF_BRICK - 1)) // TSDF_BRICK
            i = _slot_voxels(c)
            exists = ((i[0] < n[v, 0]) & (i[1] < n[v, 1]) & (i[2] < n[v, 2])).reshape(Bv, 8, 8, 8)
            Dv = D[rows.start * TSDF_BRICK_VOXELS:rows.stop * TSDF_BRICK_VOXELS].reshape(Bv, 8, 8, 8)   # [b, iz, iy, ix]
            wv = w[rows.start * TSDF_BRICK_VOXELS:rows.stop * TSDF_BRICK_VOXELS].reshape(Bv, 8, 8, 8)
            ok = exists & (wv >= np.float32(min_weight)) & (np.abs(Dv) < np.float32(1.0))
            emit = np.zeros((Bv, 8, 8, 8, 3), dtype=bool)
            frac = np.zeros((Bv, 8, 8, 8, 3), dtype=np.float32)
            for a in range(3):
                D1, ok1 = np.zeros_like(Dv), np.zeros_like(ok)     # the +1 neighbour on axis a, and whether it is valid
                low, high = inner[a]
                D1[low], ok1[low] = Dv[high], ok[high]
                beyond = c.copy()                                  # across the face: the brick that brick_index names
                beyond[:, a] += 1
                inside = beyond[:, a] < nb[a]
                at = ls[v] + (beyond[:, 2] * nb[1] + beyond[:, 1]) * nb[0] + beyond[:, 0]
                rank = np.where(inside, index[np.where(inside, at, 0)], -1)
                has = np.flatnonzero(rank >= 0)
                D1[face[0][a]][has] = Dv[face[1][a]][rank[has]]
                ok1[face[0][a]][has] = ok[face[1][a]][rank[has]]
                emit[..., a] = ok & ok1 & ((Dv < 0) != (D1 < 0))
                a0, a1 = np.abs(Dv), np.abs(D1)
                frac[..., a] = a0 / (a0 + a1)
            slot, axis = np.nonzero(emit.reshape(-1, 3))           # row-major: brick, slot, then axis
            xyz = tuple(np.float32(o[v, a]) + np.float32(vx[v]) * i[a].reshape(-1)[slot].astype(np.float32)
                        for a in range(3))
            pts = np.stack(xyz, axis=1).astype(np.float32)
            r = np.arange(slot.size)
            pts[r, axis] = pts[r, axis] + vx[v] * frac.reshape(-1, 3)[slot, axis]
            out.append(pts)
            point_start[v + 1] = point_start[v] + slot.size
    return (np.concatenate(out, 0) if out else np.zeros((0, 3), np.float32)), point_start


# ---------------------------------------------------------------------------------------------------------------
# triangle meshes with normals from the TSDF volumes: dual contouring of the lattice (csrc/tsdf_mesh.hpp)
# ---------------------------------------------------------------------------------------------------------------
TSDF_ST_FACE_OVERFLOW = _native.D3F_TSDF_ST_FACE_OVERFLOW


def tsdf_mesh_bytes(total_voxels, vertices, faces):
    """The bytes ``tsdf_mesh`` must move: D and w read by the count pass and again by the emit pass (8 bytes per voxel
    each), the ballot word of every wave written once, and the rows written (vertices and normals 12 bytes each, a
    triangle 12).  The neighbourhood reads are taken to come from cache and the scans are left out."""
    return 16 * int(total_voxels) + (int(total_voxels) + 63) // 64 * 8 + 24 * int(vertices) + 12 * int(faces)


def tsdf_mesh(D, w, vol_start, origin, dims, voxel, min_weight=1.0, vertex_capacity=None, face_capacity=None,
              return_status=False):
    """Triangle meshes of V volumes by dual contouring of the lattice (d3f_tsdf_mesh; the rule is csrc/tsdf_mesh.hpp):
    ``(vertices f32 [Nv,3], normals f32 [Nv,3], faces int32 [Nf,3], vertex_start int64 [V+1], face_start int64 [V+1])``
    on the device.  A cell whose 8 corners are valid (``w >= min_weight`` and ``|D| < 1``) and that has a crossing edge
    owns one vertex, the mean of the points ``tsdf_extract`` emits for its crossing edges; its normal is the normalised
    gradient of D over the cell and points to positive D (free space).  A crossing lattice edge whose four cells are
    complete gives two triangles, counter-clockwise seen from outside.  Vertices come in the order volume, cell index;
    faces in the order volume, lattice index of the edge's lower voxel, axis; face entries are vertex indices LOCAL to
    their volume (global row = entry + ``vertex_start[v]``).  A pure function of the volumes, bit-identical from run to
    run and to the host twin.  The arguments are those of ``tsdf_extract``.

    ONE read-back: the count pass and the scans run first, the two totals are read from the device, exactly that many
    rows are allocated and the emit pass fills them.  With BOTH capacities given nothing is read back; rows beyond a
    capacity are dropped and TSDF_ST_OVERFLOW (vertices) / TSDF_ST_FACE_OVERFLOW (faces) is set in the status word
    (``return_status=True`` appends it as a device int32 [1] tensor; both starts are complete either way)."""
    dev = _tsdf_device()
    return _tsdf_mesh(False, dev, _dense_model(False, dev, _pool_tensors(D, w, dev), vol_start, origin, dims, voxel),
                      min_weight, vertex_capacity, face_capacity, return_status)


def tsdf_mesh_host(D, w, vol_start, origin, dims, voxel, min_weight=1.0, vertex_capacity=None, face_capacity=None,
                   return_status=False):
    """The host twin of ``tsdf_mesh`` (d3f_tsdf_mesh_host): CPU tensors out, no GPU call."""
    cpu = torch.device("cpu")
    return _tsdf_mesh(True, cpu, _dense_model(True, cpu, _pool_tensors(D, w, cpu), vol_start, origin, dims, voxel),
                      min_weight, vertex_capacity, face_capacity, return_status)


_MESH_QUAD = ((-1, -1), (0, -1), (0, 0), (-1, 0))       # the cells q0..q3 around an edge, offsets on the axes (b, c)


def tsdf_mesh_numpy(D, w, vol_start, origin, dims, voxel, min_weight=1.0):
    """The contract of ``tsdf_mesh`` in NumPy: ``(vertices f32 [Nv,3], normals f32 [Nv,3], faces int32 [Nf,3],
    vertex_start int64 [V+1], face_start int64 [V+1])``, equal to the kernel's bit for bit and in order.  Every sum is
    spelled out in f32 in the order of csrc/tsdf_mesh.hpp."""
    f32 = np.float32
    D = np.ascontiguousarray(D, dtype=f32).reshape(-1)
    w = np.ascontiguousarray(w, dtype=f32).reshape(-1)
    V = int(np.asarray(dims).reshape(-1, 3).shape[0])
    o, n, vx, _, vs = _tsdf_volumes(origin, dims, voxel, V)
    if D.size != int(vs[-1]) or w.size != D.size:
        raise ValueError("D and w must hold the %d voxels of dims" % int(vs[-1]))
    if vol_start is not None and not np.array_equal(np.asarray(vol_start, dtype=np.int64).reshape(-1), vs):
        raise ValueError("vol_start is not the voxel prefix of dims")
    verts, norms, faces = [], [], []
    vertex_start, face_start = np.zeros(V + 1, dtype=np.int64), np.zeros(V + 1, dtype=np.int64)
    with np.errstate(all='ignore'):
        for v in range(V):
            nx, ny, nz = (int(a) for a in n[v])
            Dv = D[vs[v]:vs[v + 1]].reshape(nz, ny, nx)
            ok = (w[vs[v]:vs[v + 1]].reshape(nz, ny, nx) >= f32(min_weight)) & (np.abs(Dv) < f32(1.0))
            neg = Dv < 0
            lat3 = [np.broadcast_to((f32(o[v][a]) + f32(vx[v]) * np.arange(m).astype(f32)).reshape(shape), (nz, ny, nx))
                    for a, (m, shape) in enumerate(((nx, (1, 1, -1)), (ny, (1, -1, 1)), (nz, (-1, 1, 1))))]

            def corner(A, c):           # A at the corner c (bits 0..2 = offsets on x, y, z) of every cell
                dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
                return A[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
            cells = (max(nz - 1, 0), max(ny - 1, 0), max(nx - 1, 0))
            complete = np.ones(cells, dtype=bool)
            for c in range(8):
                complete &= corner(ok, c)
            k = np.zeros(cells, dtype=np.int64)
            s = [np.zeros(cells, dtype=f32) for _ in range(3)]
            g = []
            for a in range(3):
                a1, a2 = (1 if a == 0 else 0), (1 if a == 2 else 2)
                total = None
                for j in range(4):
                    c0 = ((j & 1) << a1) | (((j >> 1) & 1) << a2)
                    c1 = c0 | (1 << a)
                    d0, d1 = corner(Dv, c0), corner(Dv, c1)
                    diff = d1 - d0
                    total = diff if total is None else total + diff
                    cross = corner(neg, c0) != corner(neg, c1)
                    a0, a1_ = np.abs(d0), np.abs(d1)
                    p = [corner(lat3[r], c0) for r in range(3)]
                    p[a] = p[a] + f32(vx[v]) * (a0 / (a0 + a1_))
                    for r in range(3):
                        s[r] = np.where(cross, np.where(k == 0, p[r], s[r] + p[r]), s[r])
                    k = k + cross
                g.append(total)
            active = complete & (k > 0)
            length = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
            good = (length > 0) & np.isfinite(length)
            sel = np.nonzero(active)                                  # row-major: the cell index
            kf = k[sel].astype(f32)
            verts.append(np.stack([s[r][sel] / kf for r in range(3)], axis=1).astype(f32).reshape(-1, 3))
            norms.append(np.stack([np.where(good[sel], g[r][sel] / length[sel], f32(0.0)) for r in range(3)],
                                  axis=1).astype(f32).reshape(-1, 3))
            vertex_start[v + 1] = vertex_start[v] + sel[0].size
            # faces: the complete cells and their vertex indices on the whole lattice, then the quads of every edge
            C = np.zeros((nz, ny, nx), dtype=bool)
            C[:cells[0], :cells[1], :cells[2]] = complete
            index = np.full((nz, ny, nx), -1, dtype=np.int64)
            act = np.zeros((nz, ny, nx), dtype=bool)
            act[:cells[0], :cells[1], :cells[2]] = active
            index[act] = np.arange(int(act.sum()))
            local = np.arange(nz * ny * nx, dtype=np.int64).reshape(nz, ny, nx)
            keys, tris = [], []
            for a in range(3):
                b, c = (a + 1) % 3, (a + 2) % 3
                n_abc = (nx, ny, nz)
                rng = [slice(0, None)] * 3                            # the voxels e that can have all four cells
                rng[b], rng[c] = slice(1, None), slice(1, None)
                rng[a] = slice(0, n_abc[a] - 1)
                e = (rng[2], rng[1], rng[0])                          # arrays are [z, y, x]

                def shifted(A, db, dc):
                    r = list(rng)
                    r[b] = slice(1 + db, n_abc[b] + db)
                    r[c] = slice(1 + dc, n_abc[c] + dc)
                    return A[r[2], r[1], r[0]]
                up = list(rng)
                up[a] = slice(1, n_abc[a])
                quad = neg[e] != neg[up[2], up[1], up[0]]
                for db, dc in _MESH_QUAD:
                    quad = quad & shifted(C, db, dc)
                q = np.stack([shifted(index, db, dc)[quad] for db, dc in _MESH_QUAD], axis=1)      # [m, 4]
                inside = neg[e][quad][:, None]
                tris.append(np.where(inside, q[:, [0, 1, 2, 0, 2, 3]], q[:, [3, 2, 1, 3, 1, 0]]))
                keys.append(local[e][quad] * 3 + a)
            order = np.argsort(np.concatenate(keys), kind='stable')          # lattice index of e, then axis
            faces.append(np.concatenate(tris, 0)[order].reshape(-1, 3).astype(np.int32))
            face_start[v + 1] = face_start[v] + faces[-1].shape[0]
    cat = np.concatenate
    return cat(verts, 0), cat(norms, 0), cat(faces, 0), vertex_start, face_start


# ---------------------------------------------------------------------------------------------------------------
# triangle meshes straight from a sparse pool (csrc/tsdf_mesh_sparse.hpp has the rule; csrc/tsdf_mesh_sparse.hip the
# kernels)
# ---------------------------------------------------------------------------------------------------------------
def tsdf_mesh_sparse_bytes(bricks, vertices, faces, lattice_bricks=0):
    """The bytes ``tsdf_mesh_sparse`` must move: the pool's D and w read by the count pass and again by the emit pass
    (8 bytes per slot each), ``brick_index`` read once per pass, the 8 ballot words of every row written once, and the
    rows written (vertices and normals 12 bytes each, a triangle 12).  The halo voxels a row takes from its neighbours
    (488 of 1000) are taken to come from cache, and the scans are left out."""
    return (16 * TSDF_BRICK_VOXELS * int(bricks) + 8 * int(lattice_bricks) + 64 * int(bricks) + 24 * int(vertices) +
            12 * int(faces))


def tsdf_mesh_sparse(D, w, sv, min_weight=1.0, vertex_capacity=None, face_capacity=None, return_status=False):
    """Triangle meshes of sparse volumes straight from the pool (d3f_tsdf_sparse_mesh; the rule is
    csrc/tsdf_mesh_sparse.hpp): ``(vertices f32 [Nv,3], normals f32 [Nv,3], faces int32 [Nf,3], vertex_start int64
    [V+1], face_start int64 [V+1])`` on the device, and no dense array on the way.  The rule is ``tsdf_mesh``'s with a
    voxel's D and w taken from its brick's pool row; a voxel of an absent brick is never valid.  The result is
    ``tsdf_mesh`` of ``tsdf_densify(D, w, sv)`` -- the same vertices, normals and faces bit for bit -- in another order:
    vertices by volume, pool row (brick in lattice order) and slot of the cell's lowest voxel; faces by volume, pool row
    and slot of the edge's lower voxel, then axis; face entries are vertex indices LOCAL to their volume.  For a pool
    allocated and integrated over the same frames in one go that is the mesh of the densely integrated volume; bricks
    added late by ``tsdf_extend`` hold only the later frames.  ``D``, ``w`` as ``tsdf_integrate_sparse`` returns them;
    the capacities, ``return_status`` and the one read-back as for ``tsdf_mesh``."""
    dev = _tsdf_device()
    return _tsdf_mesh(False, dev, _sparse_model(False, dev, _pool_tensors(D, w, dev), sv), min_weight, vertex_capacity,
                      face_capacity, return_status)


def tsdf_mesh_sparse_host(D, w, sv, min_weight=1.0, vertex_capacity=None, face_capacity=None, return_status=False):
    """The host twin of ``tsdf_mesh_sparse`` (d3f_tsdf_sparse_mesh_host): CPU tensors out, no GPU call."""
    cpu = torch.device("cpu")
    return _tsdf_mesh(True, cpu, _sparse_model(True, cpu, _pool_tensors(D, w, cpu), sv), min_weight, vertex_capacity,
                      face_capacity, return_status)


def _brick_rows27(sv, v, index, coord, bs):
    """int64 [Bv,27]: the pool rows of the 27 bricks around every row of volume v, entry ``(dx + 1) + 3 (dy + 1) + 9
    (dz + 1)``, -1 where the brick is absent or outside the lattice (brick_neighbour() of csrc/tsdf_mesh_sparse.hpp)."""
    lo, hi = int(bs[v]), int(bs[v + 1])
    c = coord[lo:hi].astype(np.int64)
    nb = (np.asarray(sv.dims[v], dtype=np.int64) + (TSDF_BRICK - 1)) // TSDF_BRICK
    ls, L, B = sv.lattice_start, int(index.size), int(coord.shape[0])
    rows = np.full((hi - lo, 27), -1, dtype=np.int64)
    for j in range(27):
        off = np.array([j % 3 - 1, (j // 3) % 3 - 1, j // 9 - 1], dtype=np.int64)
        if j == 13:
            rows[:, j] = np.arange(lo, hi)
            continue
        n = c + off[None, :]
        inside = ((n >= 0) & (n < nb[None, :])).all(axis=1)
        at = int(ls[v]) + (n[:, 2] * nb[1] + n[:, 1]) * nb[0] + n[:, 0]
        inside &= (at >= 0) & (at < L)
        rank = np.where(inside, index[np.where(inside, at, 0)], -1).astype(np.int64)
        row = lo + rank
        rows[:, j] = np.where((rank >= 0) & (row >= 0) & (row < B), row, -1)
    return rows


def _brick_halo(A, rows27, lo, hi, fill):
    """``A`` [B,8,8,8] (any dtype, [row, z, y, x]) gathered around the n rows of ``rows27`` [n,27] into [n, m, m, m], m = hi - lo
    + 1: the in-brick coordinates lo..hi (lo in (-1, 0), hi in (7, 8)) per axis, with ``fill`` where a neighbour
    brick is missing."""
    n, m = rows27.shape[0], hi - lo + 1
    out = np.full((n, m, m, m), fill, dtype=A.dtype)
    parts = [(d, dst, src) for d, dst, src in ((-1, slice(0, 1), slice(7, 8)), (0, slice(-lo, 8 - lo), slice(0, 8)),
                                               (1, slice(8 - lo, 9 - lo), slice(0, 1)))
             if (d != -1 or lo < 0) and (d != 1 or hi > 7)]
    for dz, tz, sz in parts:
        for dy, ty, sy in parts:
            for dx, tx, sx in parts:
                row = rows27[:, (dx + 1) + 3 * (dy + 1) + 9 * (dz + 1)]
                has = np.flatnonzero(row >= 0)
                if has.size:
                    out[has, tz, ty, tx] = A[row[has], sz, sy, sx]
    return out


def tsdf_mesh_sparse_numpy(D, w, sv, min_weight=1.0, chunk=1 << 10):
    """The contract of ``tsdf_mesh_sparse`` in NumPy: ``(vertices f32 [Nv,3], normals f32 [Nv,3], faces int32 [Nf,3],
    vertex_start int64 [V+1], face_start int64 [V+1])``, equal to the kernel's bit for bit and in order.  It works on
    the pool, ``chunk`` bricks at a time: every brick gathers its 10 x 10 x 10 halo from the rows around it, and no
    dense volume is built.  Every sum is spelled out in f32 in the order of csrc/tsdf_mesh.hpp."""
    f32 = np.float32
    B, V = sv.bricks, sv.volumes
    D = np.ascontiguousarray(_host_array(D), dtype=f32).reshape(-1)
    w = np.ascontiguousarray(_host_array(w), dtype=f32).reshape(-1)
    if D.size != B * TSDF_BRICK_VOXELS or w.size != D.size:
        raise ValueError("D and w must hold the %d x 512 slots of the allocated bricks" % B)
    o, n, vx, _, _ = _tsdf_volumes(sv.origin, sv.dims, sv.voxel, V)
    index, coord, bs = (_host_array(a) for a in (sv.brick_index, sv.brick_coord, sv.brick_start))
    coord = coord.reshape(-1, 3)
    Dp = D.reshape(B, 8, 8, 8)                                       # [row, iz, iy, ix]
    vol = np.repeat(np.arange(V), np.diff(bs))
    i = _slot_voxels(coord)
    nv_ = n[vol].astype(np.int64)
    exists = ((i[0] < nv_[:, 0, None]) & (i[1] < nv_[:, 1, None]) & (i[2] < nv_[:, 2, None])).reshape(B, 8, 8, 8)
    ok = exists & (w.reshape(B, 8, 8, 8) >= f32(min_weight)) & (np.abs(Dp) < f32(1.0))
    neg = ok & (Dp < 0)
    rows27 = (np.concatenate([_brick_rows27(sv, v, index, coord, bs) for v in range(V)], 0) if B
              else np.zeros((0, 27), dtype=np.int64))

    def corner(A, c, lo=0):     # A [n, m, m, m] over the in-brick coordinates lo..: A at corner c of the cells lo..7
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        m = 8 - lo
        return A[:, dz:m + dz, dy:m + dy, dx:m + dx]
    # pass 1: the ACTIVE cells of every row, hence every cell's vertex index in its volume
    active = np.zeros((B, 8, 8, 8), dtype=bool)
    for s in range(0, B, int(chunk)):
        e = min(s + int(chunk), B)
        hok = _brick_halo(ok, rows27[s:e], 0, 8, False)
        hneg = _brick_halo(neg, rows27[s:e], 0, 8, False)
        complete = np.ones((e - s, 8, 8, 8), dtype=bool)
        crossing = np.zeros((e - s, 8, 8, 8), dtype=bool)
        for c in range(8):
            complete &= corner(hok, c)
            crossing |= corner(hneg, c) != corner(hneg, 0)
        active[s:e] = complete & crossing
    order = np.cumsum(active.reshape(-1)) - 1
    vertex_start = np.zeros(V + 1, dtype=np.int64)
    for v in range(V):
        vertex_start[v + 1] = int(active[:int(bs[v + 1])].sum())
    vindex = np.where(active, order.reshape(B, 8, 8, 8) - vertex_start[vol][:, None, None, None], -1).astype(np.int64)
    # pass 2: vertices, normals and faces, in the order row, slot (, axis)
    verts, norms, faces = [], [], []
    face_start = np.zeros(V + 1, dtype=np.int64)
    face_rows = np.zeros(B, dtype=np.int64)
    with np.errstate(all='ignore'):
        for s in range(0, B, int(chunk)):
            e = min(s + int(chunk), B)
            r27 = rows27[s:e]
            hD = _brick_halo(Dp, r27, 0, 8, f32(0.0))
            hneg = _brick_halo(neg, r27, 0, 8, False)
            vox = f32(vx[vol[s:e]])[:, None, None, None]
            org = o[vol[s:e]].astype(f32)
            lat = [(org[:, a, None] + f32(vx[vol[s:e]])[:, None] *
                    (coord[s:e, a, None].astype(np.int64) * 8 + np.arange(9)[None, :]).astype(f32)).astype(f32)
                   for a in range(3)]
            lat3 = [np.broadcast_to(lat[0][:, None, None, :], (e - s, 9, 9, 9)),
                    np.broadcast_to(lat[1][:, None, :, None], (e - s, 9, 9, 9)),
                    np.broadcast_to(lat[2][:, :, None, None], (e - s, 9, 9, 9))]
            cells = (e - s, 8, 8, 8)
            k = np.zeros(cells, dtype=np.int64)
            sums = [np.zeros(cells, dtype=f32) for _ in range(3)]
            g = []
            for a in range(3):
                a1, a2 = (1 if a == 0 else 0), (1 if a == 2 else 2)
                total = None
                for j in range(4):
                    c0 = ((j & 1) << a1) | (((j >> 1) & 1) << a2)
                    c1 = c0 | (1 << a)
                    d0, d1 = corner(hD, c0), corner(hD, c1)
                    diff = d1 - d0
                    total = diff if total is None else total + diff
                    cross = corner(hneg, c0) != corner(hneg, c1)
                    b0, b1 = np.abs(d0), np.abs(d1)
                    p = [corner(lat3[r], c0) for r in range(3)]
                    p[a] = p[a] + vox * (b0 / (b0 + b1))
                    for r in range(3):
                        sums[r] = np.where(cross, np.where(k == 0, p[r], sums[r] + p[r]), sums[r])
                    k = k + cross
                g.append(total)
            length = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
            good = (length > 0) & np.isfinite(length)
            sel = np.nonzero(active[s:e])                              # row-major: row, slot
            kf = k[sel].astype(f32)
            verts.append(np.stack([sums[r][sel] / kf for r in range(3)], axis=1).astype(f32).reshape(-1, 3))
            norms.append(np.stack([np.where(good[sel], g[r][sel] / length[sel], f32(0.0)) for r in range(3)],
                                  axis=1).astype(f32).reshape(-1, 3))
            # faces: the COMPLETE cells and the vertex indices of the cells -1..7 around every row
            hok = _brick_halo(ok, r27, -1, 8, False)
            hneg = _brick_halo(neg, r27, -1, 8, False)
            hidx = _brick_halo(vindex, r27, -1, 7, -1)
            C = np.ones((e - s, 9, 9, 9), dtype=bool)                  # the cells of the voxels -1..7
            for c in range(8):
                C &= corner(hok, c, -1)
            quad = np.zeros(cells + (3,), dtype=bool)
            tri = np.zeros(cells + (3, 6), dtype=np.int64)
            here = hneg[:, 1:9, 1:9, 1:9]
            for a in range(3):
                b, c = (a + 1) % 3, (a + 2) % 3

                def shifted(A, db, dc):                                # A over -1..7 at e + (db, dc) on the axes (b, c)
                    r = [slice(1, 9)] * 3
                    r[b], r[c] = slice(1 + db, 9 + db), slice(1 + dc, 9 + dc)
                    return A[:, r[2], r[1], r[0]]
                up = [slice(1, 9)] * 3
                up[a] = slice(2, 10)
                q = hok[:, 1:9, 1:9, 1:9] & hok[:, up[2], up[1], up[0]] & (here != hneg[:, up[2], up[1], up[0]])
                for db, dc in _MESH_QUAD:
                    q = q & shifted(C, db, dc)
                quad[..., a] = q
                idx = np.stack([shifted(hidx, db, dc) for db, dc in _MESH_QUAD], axis=-1)      # [.., 4]
                tri[..., a, :] = np.where(here[..., None], idx[..., [0, 1, 2, 0, 2, 3]], idx[..., [3, 2, 1, 3, 1, 0]])
            faces.append(tri[quad].reshape(-1, 3).astype(np.int32))    # row-major: row, slot, axis
            face_rows[s:e] = 2 * quad.reshape(e - s, -1).sum(axis=1)
    for v in range(V):
        face_start[v + 1] = int(face_rows[:int(bs[v + 1])].sum())
    cat = np.concatenate
    none = np.zeros((0, 3), dtype=f32)
    return (cat(verts, 0) if verts else none, cat(norms, 0) if norms else none.copy(),
            cat(faces, 0) if faces else np.zeros((0, 3), dtype=np.int32), vertex_start, face_start)


# ---------------------------------------------------------------------------------------------------------------
# Ray-casting TSDF volumes, dense and sparse: a volume plus a camera pose gives a depth image (csrc/tsdf_raycast.hpp has
# the rule; csrc/tsdf_raycast.hip the kernel, for both kinds of model)
# ---------------------------------------------------------------------------------------------------------------
RAYCAST_MAX_SAMPLES = _native.D3F_RAYCAST_MAX_SAMPLES   # samples of one ray at most
RAYCAST_DEPTH_MIN = 0.1       # default depth_min in metres: where every ray starts
RAYCAST_MAX_VIEWS = 65535


def _raycast_views(V, trunc, intrinsics, camera_to_volume, height, width, view_volume, step, depth_min, depth_max):
    """Host form of the view arguments: (view_volume int32 [R], K f32 [R,4], C f32 [R,12], step f32 [V])."""
    def host(a):
        return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    H, W = int(height), int(width)
    if H < 1 or W < 1 or H * W > 1 << 30:
        raise ValueError("height and width must be positive and hold at most 2^30 pixels, got %d x %d" % (H, W))
    vv = np.arange(V, dtype=np.int64) if view_volume is None else np.asarray(host(view_volume), dtype=np.int64).reshape(-1)
    R = vv.size
    if R > RAYCAST_MAX_VIEWS:
        raise ValueError("at most %d views per call, got %d" % (RAYCAST_MAX_VIEWS, R))
    if R and (vv.min() < 0 or vv.max() >= V):
        raise ValueError("view_volume must name volumes in 0..%d, got %s" % (V - 1, vv.tolist()))
    K = np.asarray(host(intrinsics), dtype=np.float32)
    K = np.ascontiguousarray(np.broadcast_to(K.reshape(-1, 4), (R, 4)))
    c = np.asarray(host(camera_to_volume))
    if c.ndim == 2 and c.shape in ((4, 4), (3, 4)) and R == 1:
        c = c[None]
    if c.ndim == 3 and c.shape[1:] in ((4, 4), (3, 4)):
        c = c[:, :3, :]
    c = np.ascontiguousarray(c.astype(np.float32).reshape(-1, 12))        # rounded to f32 once, here
    if c.shape[0] != R:
        raise ValueError("%d camera_to_volume matrices for %d views" % (c.shape[0], R))
    dmin, dmax = np.float32(depth_min), np.float32(depth_max)
    if not (dmin >= 0 and dmax >= dmin and np.isfinite(dmax)):
        raise ValueError("0 <= depth_min <= depth_max (finite) is required, got %g and %g" % (depth_min, depth_max))
    if step is None:
        if trunc is None:
            raise ValueError("step=None takes trunc / 2: give trunc or step")
        st = np.broadcast_to(np.asarray(host(trunc), dtype=np.float32).reshape(-1), (V,)) / np.float32(2.0)
    else:
        st = np.broadcast_to(np.asarray(host(step), dtype=np.float32).reshape(-1), (V,))
    st = np.ascontiguousarray(st, dtype=np.float32)
    if not (st > 0).all() or not ((dmax - dmin) / st <= np.float32(RAYCAST_MAX_SAMPLES)).all():
        raise ValueError("every step must be positive and give at most %d samples between depth_min and depth_max, "
                         "got %s" % (RAYCAST_MAX_SAMPLES, st.tolist()))
    return vv.astype(np.int32), K, c, st, H, W


def _color_volume(Cv, total, what):
    """A colour volume / pool as a contiguous tensor [total, Cc] ([total] is one channel)."""
    Cc = int(Cv.shape[-1]) if Cv.dim() >= 2 else 1
    if Cc not in (1, 3) or int(Cv.numel()) != total * Cc:
        raise ValueError("color must hold 1 or 3 channels for each of the %d %s, got %s" % (total, what, tuple(Cv.shape)))
    return Cv.contiguous().view(total, Cc), Cc


# A fused TSDF model as the entry points of csrc/tsdf_raycast.hip read it, dense or sparse: ``tensors`` (D, w and the
# colour as given, checked to be float32 on the device), ``stem`` of the entry points' names, ``V``, ``cells`` (the voxels
# or slots that D, w and the colours must hold), ``stored`` (False: an empty pool, whose pointers go in as NULL), the
# words of the error messages (``holds``, ``limit``), ``color(c)`` -> (the checked colour tensor, Cc) and ``tables()`` ->
# (the C arguments between the colour and the views / points, the tensors behind them).  ``tables(surface=True)`` gives
# the pair of argument lists of the extract and mesh entry points instead: those of the emit forms and the twins, which
# take ``brick_coord`` too (NULL for an empty pool), and those of the count forms, which take no origin and no voxel.
# The last argument of either is the size that the ``_ws_bytes`` functions take.
_FusedModel = collections.namedtuple("_FusedModel", "tensors stem V cells stored holds limit color tables")


def _model_tensors(host, device, kind, named):
    """``named`` = ((name, float32 tensor or None), ...) of a ``kind`` ("volume" / "pool"): the tensors, checked to be
    on ``device`` (a host twin takes arrays too)."""
    out = [torch.from_numpy(np.array(t, dtype=np.float32)) if host and isinstance(t, np.ndarray) else t
           for _, t in named]
    for (name, _), t in zip(named, out):
        if name == "color" and t is None:
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device.type != device.type:
            raise ValueError("%s must be a float32 tensor on %s: the %s stays where it is" % (name, device, kind))
    return out


def _dense_model(host, device, named, vol_start, origin, dims, voxel):
    tensors = _model_tensors(host, device, "volume", named)
    V = int(np.asarray(_host_array(dims)).reshape(-1, 3).shape[0])
    o, n, vx, _, vs = _tsdf_volumes(origin, dims, voxel, V)
    total = int(vs[-1])

    def tables(surface=False):
        held = _on(device, vs, o, n, vx)
        _check_vol_start(vol_start, held[0])
        args = tuple(_p(t) for t in held) + (V, total)
        return ((args, (args[0], args[2], V, total)) if surface else args), held

    return _FusedModel(tensors=tensors, stem="", V=V, cells=total, stored=True, holds="the %d voxels of dims" % total,
                       limit=" (at most %d volumes)" % TSDF_MAX_VOLUMES,
                       color=lambda c: _color_volume(c, total, "voxels"), tables=tables)


def _sparse_model(host, device, named, sv):
    tensors = _model_tensors(host, device, "pool", named)
    B = sv.bricks

    def color(c):
        Cp = _sparse_color_pool(c, sv, device)
        return Cp, int(Cp.shape[-1])

    def tables(surface=False):
        tls, bs, bi, bc, to, tn, tvx = held = _sparse_tables(sv, device)
        rows, sizes = (_p(tls), _p(bs), _p(bi)), (sv.volumes, int(sv.lattice_start[-1]), B)
        if surface:
            rows += (_p(bc) if B else None,)
        args = rows + (_p(to), _p(tn), _p(tvx)) + sizes
        return ((args, rows + (_p(tn),) + sizes) if surface else args), held

    return _FusedModel(tensors=tensors, stem="_sparse", V=sv.volumes, cells=B * TSDF_BRICK_VOXELS, stored=bool(B),
                       holds="the %d x 512 slots of the allocated bricks" % B, limit="", color=color, tables=tables)


def _tsdf_surface(host, device, model, what, min_weight, capacities, outputs, return_status):
    """Every extract and mesh form, d3f_tsdf[_sparse]_{extract,mesh}{_count, , _host}.  ``model``: ``_dense_model`` /
    ``_sparse_model`` of (D, w); ``what``: "extract" / "mesh"; ``capacities``: one per kind of row (points; vertices and
    faces), None for "as many as there are"; ``outputs``: (dtype, index of its capacity) per output of rows [n,3].
    Returns the outputs, one start [V+1] per capacity and, with ``return_status``, the status word.

    The capacity rule, once: with every capacity given nothing is read back, rows beyond a capacity are dropped and
    leave a bit in the status.  Otherwise the device forms count and scan first, read the totals (the ONE read-back),
    and emit into exactly that many rows; a twin is run twice, first into no rows at all."""
    D, w = model.tensors
    if int(D.numel()) != model.cells or int(w.numel()) != model.cells:
        raise ValueError("D and w must hold %s, got %d and %d" % (model.holds, D.numel(), w.numel()))
    if not model.stem and (model.cells == 0 or model.V > TSDF_MAX_VOLUMES):
        raise ValueError("between 1 and %d volumes per call" % TSDF_MAX_VOLUMES)
    (emit_tables, count_tables), _held = model.tables(surface=True)
    V, name = model.V, "d3f_tsdf%s_%s" % (model.stem, what)
    starts = torch.zeros((len(capacities), V + 1), dtype=torch.int64, device=device)
    status = torch.zeros(1, dtype=torch.int32, device=device)

    def rows(capacities):
        return tuple(torch.empty((int(capacities[j]), 3), dtype=dtype, device=device) for dtype, j in outputs)

    def returned(out):
        out += tuple(starts)
        return out + (status,) if return_status else out

    if not host and not model.stored:                          # nothing allocated: no kernel has anything to do
        return returned(rows([c or 0 for c in capacities]))
    L = _native.lib()
    pool = (_p(D), _p(w)) if model.stored else (None, None)
    known = all(c is not None for c in capacities)

    def emit(fn, head, capacities, out, status, tail):
        capacities = tuple(int(c) for c in capacities)
        _native.check(fn(*(pool + emit_tables + head + capacities + tuple(_p(t) if t.numel() else None for t in out) +
                           tuple(_p(s) for s in starts) + (_p(status),) + tail)), fn.__name__)

    if host:
        fn = getattr(L, name + "_host")
        if not known:                                          # the totals
            emit(fn, (float(min_weight),), [0] * len(capacities), rows([0] * len(capacities)),
                 torch.zeros(1, dtype=torch.int32), ())
            capacities = [int(s[V]) if c is None else c for c, s in zip(capacities, starts)]
        out = rows(capacities)
        emit(fn, (float(min_weight),), capacities, out, status, ())
        return returned(out)
    nbytes = getattr(L, name + "_ws_bytes")(emit_tables[-1])
    ws = _ws(nbytes, device)
    tail = (_p(ws), nbytes, _stream())
    with _region("tsdf_" + what + model.stem):
        if not known:
            _native.check(getattr(L, name + "_count")(*(pool + count_tables + (float(min_weight),) +
                                                        tuple(_p(s) for s in starts) + tail)), name + "_count")
            totals = starts[:, V].tolist()                     # the one read-back: the sizes of the result
            capacities = [t if c is None else c for c, t in zip(capacities, totals)]
        out = rows(capacities)
        emit(getattr(L, name), (float(min_weight), int(not known)), capacities, out, status, tail)
    return returned(out)


def _tsdf_extract(host, device, model, min_weight, capacity, return_status):
    """(points f32 [M,3], point_start int64 [V+1]) of ``model``, on ``device``."""
    return _tsdf_surface(host, device, model, "extract", min_weight, [capacity], ((torch.float32, 0),), return_status)


def _tsdf_mesh(host, device, model, min_weight, vertex_capacity, face_capacity, return_status):
    """(vertices f32 [Nv,3], normals f32 [Nv,3], faces int32 [Nf,3], vertex_start, face_start) of ``model``."""
    return _tsdf_surface(host, device, model, "mesh", min_weight, [vertex_capacity, face_capacity],
                         ((torch.float32, 0), (torch.float32, 0), (torch.int32, 1)), return_status)


def _tsdf_raycast(host, device, model, trunc, intrinsics, camera_to_volume, height, width, view_volume, step, depth_min,
                  depth_max, min_weight, normals, clip, skip=None):
    """Every ray-cast form.  ``model``: ``_dense_model`` / ``_sparse_model`` of (D, w, color); ``skip``: None for the
    dense entry points, which take none."""
    D, w, color = model.tensors
    D, w = D.contiguous().view(-1), w.contiguous().view(-1)
    if int(D.numel()) != model.cells or int(w.numel()) != model.cells:
        raise ValueError("D and w must hold %s, got %d and %d" % (model.holds, D.numel(), w.numel()))
    if model.V > TSDF_MAX_VOLUMES:
        raise ValueError("at most %d volumes per call" % TSDF_MAX_VOLUMES)
    vv, K, C, st, H, W = _raycast_views(model.V, trunc, intrinsics, camera_to_volume, height, width, view_volume, step,
                                        depth_min, depth_max)
    R = vv.size
    Cv, Cc = (None, 0) if color is None else model.color(color)
    depth = torch.empty((R, H, W), dtype=torch.float32, device=device)
    nrm = torch.empty((R, H, W, 3), dtype=torch.float32, device=device) if normals else None
    col = torch.empty((R, H, W, Cc), dtype=torch.float32, device=device) if Cc else None
    if R:
        tables, _held = model.tables()
        tvv, tK, tC, tst = _on(device, vv, K, C, st)
        ptr = _p if model.stored else (lambda t: None)
        name = "d3f_tsdf_raycast" + model.stem + ("_host" if host else "")
        args = ((ptr(D), ptr(w), ptr(Cv), Cc) + tables +         # Cc = 0: null colour pointers, which are not looked at
                (_p(tvv), R, H, W, _p(tK), _p(tC), _p(tst), float(depth_min), float(depth_max), float(min_weight),
                 int(bool(clip))) + (() if skip is None else (int(bool(skip)),)) +
                (_p(depth), _p(nrm), _p(col), None if host else _stream()))
        _native.check(getattr(_native.lib(), name)(*args), name)
    out = (depth,) + ((nrm,) if normals else ()) + ((col,) if Cc else ())
    return out if len(out) > 1 else depth


def tsdf_raycast(D, w, vol_start, origin, dims, voxel, trunc, intrinsics, camera_to_volume, height, width,
                 view_volume=None, step=None, depth_min=RAYCAST_DEPTH_MIN, depth_max=TSDF_DEPTH_MAX, min_weight=1.0,
                 normals=False, clip=True, color=None):
    """Ray-cast R views of V dense TSDF volumes in ONE launch (d3f_tsdf_raycast; the rule is csrc/tsdf_raycast.hpp):
    ``depth`` f32 [R,H,W] on the device, the camera z-depth in metres of the surface along every pixel's ray, 0 where
    the ray meets none -- what ``depth_pyramid`` takes as f32 metres.  ``normals=True`` returns ``(depth, normals f32
    [R,H,W,3])``: unit normals in the camera frame, towards positive D (out of the surface, facing the camera: the sign
    of ``tsdf_mesh``'s normals and of the odometry's), zeros where there is no hit or the gradient is not defined.

    ``D``, ``w``, ``vol_start``, ``origin``, ``dims``, ``voxel`` as ``tsdf_integrate`` returns and takes them; D and w
    are device tensors and stay where they are.  ``intrinsics`` [4] or [R,4] = fx, fy, cx, cy; ``camera_to_volume``
    [R,3,4] / [R,4,4] maps a view's camera into the frame of its volume (f64 is rounded to f32 once, here);
    ``view_volume`` [R]: the volume of every view, in any order, a volume any number of times (None: R = V, one view per
    volume).  A ray samples the trilinear D at ``depth_min + step k <= depth_max``; ``step`` (a number or [V]) defaults
    to ``trunc / 2``.  A sample counts when all 8 corners of its cell have ``w >= min_weight``; |D| < 1 is not asked
    for.  A positive sample followed by a non-positive one is a hit at the interpolated zero; a ray that first meets a
    surface from behind (a negative sample not preceded by a positive one) ends without a hit.  ``clip=False`` turns
    off the clipping of every ray's sample range to the volume's box, which changes the time and no bit.

    One thread per ray, a wave per 8 x 8 pixels; no atomics, nothing read back: a view's image is bit-identical alone,
    in any batch, from run to run, and to ``tsdf_raycast_host`` and ``tsdf_raycast_numpy``.  R = 0 returns empty
    tensors without a launch.

    ``color=Cv`` (the colour volume [total, Cc] of ``tsdf_integrate(color=)``, a device tensor) appends the colour
    image f32 [R,H,W,Cc] to whatever is returned (d3f_tsdf_raycast, channels = Cc; csrc/tsdf_color.hpp): at a hit the
    trilinear mean of the colours of the hit cell's corners with ``w >= min_weight``, renormalised over those corners
    (so a hit in a partly observed cell still has a colour); NaN in every channel where depth is 0 -- NaN, not 0, so
    the render goes into ``rgbd_pyramid`` as f32 intensity and the tracker's finiteness test drops those pixels.
    Depth and normals are untouched, bit for bit."""
    dev = _tsdf_device()
    with _region("tsdf_raycast"):
        model = _dense_model(False, dev, (("D", D), ("w", w), ("color", color)), vol_start, origin, dims, voxel)
        return _tsdf_raycast(False, dev, model, trunc, intrinsics, camera_to_volume, height, width, view_volume, step,
                             depth_min, depth_max, min_weight, normals, clip)


def tsdf_raycast_host(D, w, vol_start, origin, dims, voxel, trunc, intrinsics, camera_to_volume, height, width,
                      view_volume=None, step=None, depth_min=RAYCAST_DEPTH_MIN, depth_max=TSDF_DEPTH_MAX,
                      min_weight=1.0, normals=False, clip=True, color=None):
    """The host twin of ``tsdf_raycast`` (d3f_tsdf_raycast_host): CPU tensors (or arrays)
    in, CPU tensors out, no GPU call."""
    cpu = torch.device("cpu")
    model = _dense_model(True, cpu, (("D", D), ("w", w), ("color", color)), vol_start, origin, dims, voxel)
    return _tsdf_raycast(True, cpu, model, trunc, intrinsics, camera_to_volume, height, width, view_volume, step,
                         depth_min, depth_max, min_weight, normals, clip)


def _raycast_lerp(a, b, t):
    return a + t * (b - a)


def _raycast_sample_numpy(Dv, wv, n, o, vx, qx, qy, qz, min_weight):
    """sample() of csrc/tsdf_raycast.hpp for the f32 points (qx, qy, qz): (valid bool, value f32)."""
    f32 = np.float32
    nx, ny, nz = (int(a) for a in n)
    one = f32(1.0)
    gx, gy, gz = (qx - o[0]) / vx, (qy - o[1]) / vx, (qz - o[2]) / vx
    ix, iy, iz = np.floor(gx), np.floor(gy), np.floor(gz)
    inside = ((ix >= 0) & (ix + one < f32(nx)) & (iy >= 0) & (iy + one < f32(ny)) & (iz >= 0) & (iz + one < f32(nz)))
    zero = f32(0.0)
    i = (np.where(inside, ix, zero).astype(np.int64) + nx * np.where(inside, iy, zero).astype(np.int64)
         + nx * ny * np.where(inside, iz, zero).astype(np.int64))
    if nx < 2 or ny < 2 or nz < 2:                    # no cell: nothing is inside, and nothing is read
        return np.zeros(i.shape, dtype=bool), np.zeros(i.shape, dtype=f32)
    sy, sz = nx, nx * ny
    corners = (0, 1, sy, sy + 1, sz, sz + 1, sz + sy, sz + sy + 1)
    d000, d100, d010, d110, d001, d101, d011, d111 = (Dv[i + c] for c in corners)
    weighted = np.ones(i.shape, dtype=bool)
    for c in corners:
        weighted &= wv[i + c] >= min_weight
    fx, fy, fz = gx - ix, gy - iy, gz - iz
    e00, e10 = _raycast_lerp(d000, d100, fx), _raycast_lerp(d010, d110, fx)
    e01, e11 = _raycast_lerp(d001, d101, fx), _raycast_lerp(d011, d111, fx)
    value = _raycast_lerp(_raycast_lerp(e00, e10, fy), _raycast_lerp(e01, e11, fy), fz)
    return inside & weighted, value.astype(f32)


def _color_at_numpy(Cv, wv, n, o, vx, q, min_weight):
    """color_at() of csrc/tsdf_color.hpp for the f32 points q = (qx, qy, qz) in a dense lattice with colours Cv
    [count, Cc] and weights wv [count]: f32 [N, Cc], NaN where the rule gives none."""
    f32 = np.float32
    Cc = Cv.shape[1]
    N = q[0].shape[0]
    out = np.full((N, Cc), np.nan, dtype=f32)
    nn = [int(a) for a in n]
    if min(nn) < 2 or N == 0:
        return out
    one, zero = f32(1.0), f32(0.0)
    g = [(q[a] - o[a]) / vx for a in range(3)]
    inside = np.ones(N, dtype=bool)
    for a in range(3):
        inside &= (g[a] >= zero) & (g[a] <= f32(nn[a] - 1))
    base = [np.minimum(np.floor(np.where(inside, g[a], zero)), f32(nn[a] - 2)) for a in range(3)]
    f = [np.where(inside, g[a], zero) - base[a] for a in range(3)]
    i = [b.astype(np.int64) for b in base]
    sy, sz = nn[0], nn[0] * nn[1]
    at = i[0] + sy * i[1] + sz * i[2]
    tx, ty, tz = (one - f[0], f[0]), (one - f[1], f[1]), (one - f[2], f[2])
    s = np.zeros(N, dtype=f32)
    acc = np.zeros((N, Cc), dtype=f32)
    for c in range(8):
        t = (tx[c & 1] * ty[(c >> 1) & 1]) * tz[c >> 2]
        j = at + (c & 1) + sy * ((c >> 1) & 1) + sz * (c >> 2)
        weighted = wv[j] >= min_weight
        s = np.where(weighted, s + t, s)
        acc = np.where(weighted[:, None], acc + t[:, None] * Cv[j], acc)
    ok = inside & (s > zero)
    return np.where(ok[:, None], acc / s[:, None], f32(np.nan)).astype(f32)


def _raycast_point_numpy(C, x, y, z):
    """ray_point() of csrc/tsdf_raycast.hpp."""
    X, Y = x * z, y * z
    return tuple(((C[4 * r] * X + C[4 * r + 1] * Y) + C[4 * r + 2] * z) + C[4 * r + 3] for r in range(3))


def _raycast_clip_numpy(n, o, vx, C, x, y, step, dmin, dmax):
    """clip_range() of csrc/tsdf_raycast.hpp: (k0, k1) int64 per ray."""
    f32 = np.float32
    zin = np.full(x.shape, dmin, dtype=f32)
    zout = np.full(x.shape, dmax, dtype=f32)
    empty = np.zeros(x.shape, dtype=bool)
    for a in range(3):
        d = (C[4 * a] * x + C[4 * a + 1] * y) + C[4 * a + 2]
        oa = C[4 * a + 3]
        lo, hi = o[a] - vx, o[a] + vx * f32(n[a])
        still = d == 0
        empty |= still & ((oa < lo) | (oa > hi))
        ta, tb = (lo - oa) / d, (hi - oa) / d
        zin = np.where(still, zin, np.fmax(zin, np.fmin(ta, tb)))      # fmin / fmax drop a NaN, as fminf / fmaxf do
        zout = np.where(still, zout, np.fmin(zout, np.fmax(ta, tb)))
    lo = np.floor((zin - dmin) / step) - f32(1.0)
    hi = np.ceil((zout - dmin) / step) + f32(1.0)
    lo = np.fmin(np.fmax(lo, f32(0.0)), f32(RAYCAST_MAX_SAMPLES + 1))
    hi = np.fmax(np.fmin(hi, f32(RAYCAST_MAX_SAMPLES)), f32(-1.0))
    return lo.astype(np.int64), np.where(empty, -1, hi.astype(np.int64))


def _raycast_view_numpy(Dv, wv, n, o, vx, K, C, H, W, step, dmin, dmax, min_weight, clip, normals, Cv=None):
    """cast_ray() of csrc/tsdf_raycast.hpp for every pixel of one view: (depth f32 [H,W], normals f32 [H,W,3] | None);
    with the volume's colours ``Cv`` [count, Cc] also hit_color() of csrc/tsdf_color.hpp, f32 [H,W,Cc], third."""
    f32 = np.float32
    P = H * W
    depth = np.zeros(P, dtype=f32)
    nrm = np.zeros((P, 3), dtype=f32) if normals else None
    u = np.broadcast_to(np.arange(W, dtype=f32)[None, :], (H, W)).reshape(-1)
    v = np.broadcast_to(np.arange(H, dtype=f32)[:, None], (H, W)).reshape(-1)
    x, y = (u - K[2]) / K[0], (v - K[3]) / K[1]
    if clip:
        k0, k1 = _raycast_clip_numpy(n, o, vx, C, x, y, step, dmin, dmax)
    else:
        k0, k1 = np.zeros(P, dtype=np.int64), np.full(P, RAYCAST_MAX_SAMPLES, dtype=np.int64)
    positive = np.zeros(P, dtype=bool)
    t0 = np.zeros(P, dtype=f32)
    done = k1 < k0
    for k in range(int(k0.min()) if P else 0, (int(k1.max()) if P else -1) + 1):
        z = dmin + step * f32(k)
        if not z <= dmax or done.all():
            break
        idx = np.nonzero(~done & (k0 <= k) & (k <= k1))[0]
        if idx.size == 0:
            continue
        q = _raycast_point_numpy(C, x[idx], y[idx], z)
        valid, t1 = _raycast_sample_numpy(Dv, wv, n, o, vx, q[0], q[1], q[2], min_weight)
        hit = valid & positive[idx] & ~(t1 > 0)
        a0, a1 = t0[idx][hit], t1[hit]
        depth[idx[hit]] = (z - step) + step * (a0 / (a0 - a1))
        end = valid & ~hit & (t1 < 0)
        done[idx[hit | end]] = True
        positive[idx] = valid & (t1 > 0)
        t0[idx] = np.where(valid, t1, t0[idx])
    depth = np.where((depth > 0) & (depth <= dmax), depth, f32(0.0)).astype(f32)
    if normals:
        idx = np.nonzero(depth > 0)[0]
        q = _raycast_point_numpy(C, x[idx], y[idx], depth[idx])
        ok = np.ones(idx.size, dtype=bool)
        g = []
        for a in range(3):
            p, m = list(q), list(q)
            p[a], m[a] = q[a] + vx, q[a] - vx
            okp, vp = _raycast_sample_numpy(Dv, wv, n, o, vx, p[0], p[1], p[2], min_weight)
            okm, vm = _raycast_sample_numpy(Dv, wv, n, o, vx, m[0], m[1], m[2], min_weight)
            ok &= okp & okm
            g.append(vp - vm)
        nc = [(C[j] * g[0] + C[4 + j] * g[1]) + C[8 + j] * g[2] for j in range(3)]
        ln = np.sqrt((nc[0] * nc[0] + nc[1] * nc[1]) + nc[2] * nc[2])
        ok &= (ln > 0) & (ln <= np.finfo(f32).max)
        for j in range(3):
            nrm[idx, j] = np.where(ok, nc[j] / ln, f32(0.0))
    if Cv is not None:
        col = np.full((P, Cv.shape[1]), np.nan, dtype=f32)
        idx = np.nonzero(depth > 0)[0]
        q = _raycast_point_numpy(C, x[idx], y[idx], depth[idx])
        col[idx] = _color_at_numpy(Cv, wv, n, o, vx, q, min_weight)
        return depth.reshape(H, W), (nrm.reshape(H, W, 3) if normals else None), col.reshape(H, W, -1)
    return depth.reshape(H, W), (nrm.reshape(H, W, 3) if normals else None)


def tsdf_raycast_numpy(D, w, vol_start, origin, dims, voxel, trunc, intrinsics, camera_to_volume, height, width,
                       view_volume=None, step=None, depth_min=RAYCAST_DEPTH_MIN, depth_max=TSDF_DEPTH_MAX,
                       min_weight=1.0, normals=False, clip=True, color=None):
    """The contract of ``tsdf_raycast`` in NumPy: ``depth`` f32 [R,H,W] (and ``normals`` f32 [R,H,W,3], and with
    ``color=Cv`` the colour image f32 [R,H,W,Cc]), every f32 operation in the order of csrc/tsdf_raycast.hpp and
    csrc/tsdf_color.hpp, so the result equals the kernel's bit for bit."""
    D = np.ascontiguousarray(_host_array(D), dtype=np.float32).reshape(-1)
    w = np.ascontiguousarray(_host_array(w), dtype=np.float32).reshape(-1)
    V = int(np.asarray(_host_array(dims)).reshape(-1, 3).shape[0])
    o, n, vx, _, vs = _tsdf_volumes(origin, dims, voxel, V)
    if D.size != int(vs[-1]) or w.size != int(vs[-1]):
        raise ValueError("D and w must hold the %d voxels of dims, got %d and %d" % (vs[-1], D.size, w.size))
    vv, K, C, st, H, W = _raycast_views(V, trunc, intrinsics, camera_to_volume, height, width, view_volume, step,
                                        depth_min, depth_max)
    f32 = np.float32
    Cv = None
    if color is not None:
        Cv = np.ascontiguousarray(_host_array(color), dtype=f32)
        Cv = Cv.reshape(D.size, -1)
        if Cv.shape[1] not in (1, 3):
            raise ValueError("color must hold 1 or 3 channels for each of the %d voxels" % D.size)
    depth = np.zeros((vv.size, H, W), dtype=f32)
    nrm = np.zeros((vv.size, H, W, 3), dtype=f32) if normals else None
    col = np.zeros((vv.size, H, W, Cv.shape[1]), dtype=f32) if Cv is not None else None
    with np.errstate(all='ignore'):
        for r, vol in enumerate(vv):
            a, b = int(vs[vol]), int(vs[vol + 1])
            res = _raycast_view_numpy(D[a:b], w[a:b], n[vol], o[vol], vx[vol], K[r], C[r], H, W, st[vol],
                                      f32(depth_min), f32(depth_max), f32(min_weight), clip, normals,
                                      None if Cv is None else Cv[a:b])
            depth[r] = res[0]
            if normals:
                nrm[r] = res[1]
            if Cv is not None:
                col[r] = res[2]
    out = (depth,) + ((nrm,) if normals else ()) + ((col,) if Cv is not None else ())
    return out if len(out) > 1 else depth


def _sample_points(points, point_start, V):
    """Host form of the points of ``tsdf_sample_color``: (f32 [N,3], int64 [V+1])."""
    pts = np.ascontiguousarray(_host_array(points), dtype=np.float32).reshape(-1, 3)
    ps = np.ascontiguousarray(_host_array(point_start), dtype=np.int64).reshape(-1)
    if ps.size != V + 1 or ps[0] < 0 or ps[-1] > pts.shape[0] or (np.diff(ps) < 0).any():
        raise ValueError("point_start must be the rising prefix [V+1] of the %d points over %d volumes, got %s"
                         % (pts.shape[0], V, ps.tolist()))
    return pts, ps


def _sample_inputs(points, point_start, V, device):
    """(points f32 [N,3], point_start int64 [V+1]) on ``device``; device tensors stay where they are (nothing is read
    back), host values are checked."""
    if isinstance(points, torch.Tensor) and isinstance(point_start, torch.Tensor) and points.is_cuda and \
            device.type == "cuda":
        tp = points.to(torch.float32).contiguous().view(-1, 3)
        tps = point_start.to(device=device, dtype=torch.int64).contiguous().view(-1)
        if int(tps.numel()) != V + 1:
            raise ValueError("point_start must hold %d entries, got %d" % (V + 1, tps.numel()))
        return tp, tps
    pts, ps = _sample_points(points, point_start, V)
    return tuple(_on(device, pts, ps))


def _tsdf_sample_color(host, device, model, points, point_start, min_weight):
    """Every point-sampling form.  ``model``: ``_dense_model`` / ``_sparse_model`` of (the colours, w)."""
    Cv, w = model.tensors
    w = w.contiguous().view(-1)
    if int(w.numel()) != model.cells or model.V > TSDF_MAX_VOLUMES:
        raise ValueError("w must hold %s%s, got %d" % (model.holds, model.limit, w.numel()))
    Cv, Cc = model.color(Cv)
    tp, tps = _sample_inputs(points, point_start, model.V, device)
    N = int(tp.shape[0])
    out = torch.empty((N, Cc), dtype=torch.float32, device=device)
    if N:
        tables, _held = model.tables()
        ptr = _p if model.stored else (lambda t: None)
        name = "d3f_tsdf_sample_color" + model.stem + ("_host" if host else "")
        _native.check(getattr(_native.lib(), name)(*((ptr(Cv), ptr(w), Cc) + tables + (
            _p(tp), _p(tps), N, float(min_weight), _p(out), None if host else _stream()))), name)
    return out


def tsdf_sample_color(Cv, w, vol_start, origin, dims, voxel, points, point_start, min_weight=1.0):
    """The colour of dense colour volumes at arbitrary points (d3f_tsdf_sample_color; ``color_at`` of
    csrc/tsdf_color.hpp): f32 [N, Cc] on the device.  ``Cv`` [total, Cc], ``w``, ``vol_start``, ``origin``, ``dims``,
    ``voxel`` as ``tsdf_integrate(color=)`` returns and takes them; ``points`` f32 [N,3] in the frame of their volume
    and ``point_start`` [V+1] as ``tsdf_extract`` / ``tsdf_mesh`` (its vertex_start) return them -- device tensors are
    used where they are.  A point's colour is the trilinear mean of its cell's corners with ``w >= min_weight``,
    renormalised over those corners; a point on the last lattice plane is inside; NaN in every channel where the point
    is outside the lattice (a NaN coordinate is), where some dimension is 1, or where no corner has weight.  One thread
    per point; equal to the host twin and ``tsdf_sample_color_numpy`` bit for bit."""
    dev = _tsdf_device()
    with _region("tsdf_sample_color"):
        model = _dense_model(False, dev, (("Cv", Cv), ("w", w)), vol_start, origin, dims, voxel)
        return _tsdf_sample_color(False, dev, model, points, point_start, min_weight)


def tsdf_sample_color_host(Cv, w, vol_start, origin, dims, voxel, points, point_start, min_weight=1.0):
    """The host twin of ``tsdf_sample_color`` (d3f_tsdf_sample_color_host): CPU tensors (or arrays) in, a CPU tensor
    out, no GPU call."""
    cpu = torch.device("cpu")
    model = _dense_model(True, cpu, (("Cv", Cv), ("w", w)), vol_start, origin, dims, voxel)
    return _tsdf_sample_color(True, cpu, model, points, point_start, min_weight)


def tsdf_sample_color_numpy(Cv, w, vol_start, origin, dims, voxel, points, point_start, min_weight=1.0):
    """The contract of ``tsdf_sample_color`` in NumPy: f32 [N, Cc], every f32 operation in the order of
    csrc/tsdf_color.hpp."""
    f32 = np.float32
    w = np.ascontiguousarray(_host_array(w), dtype=f32).reshape(-1)
    V = int(np.asarray(_host_array(dims)).reshape(-1, 3).shape[0])
    o, n, vx, _, vs = _tsdf_volumes(origin, dims, voxel, V)
    Cv = np.ascontiguousarray(_host_array(Cv), dtype=f32).reshape(w.size, -1)
    if w.size != int(vs[-1]) or Cv.shape[1] not in (1, 3):
        raise ValueError("w and Cv must hold the %d voxels of dims, Cv with 1 or 3 channels" % int(vs[-1]))
    pts, ps = _sample_points(points, point_start, V)
    out = np.full((pts.shape[0], Cv.shape[1]), np.nan, dtype=f32)
    with np.errstate(all='ignore'):
        for v in range(V):
            a, b, p0, p1 = int(vs[v]), int(vs[v + 1]), int(ps[v]), int(ps[v + 1])
            q = tuple(pts[p0:p1, k] for k in range(3))
            out[p0:p1] = _color_at_numpy(Cv[a:b], w[a:b], n[v], o[v], vx[v], q, f32(min_weight))
    return out


# ---------------------------------------------------------------------------------------------------------------
# Ray-casting, growing and continuing SPARSE TSDF volumes (csrc/tsdf_raycast_sparse.hpp has the rule;
# csrc/tsdf_raycast.hip the kernel: _tsdf_raycast and _tsdf_sample_color above, with a _sparse_model)
# ---------------------------------------------------------------------------------------------------------------
def tsdf_raycast_sparse(D, w, sv, trunc, intrinsics, camera_to_volume, height, width, view_volume=None, step=None,
                        depth_min=RAYCAST_DEPTH_MIN, depth_max=TSDF_DEPTH_MAX, min_weight=1.0, normals=False,
                        clip=True, skip=True, color=None):
    """Ray-cast R views of V SPARSE TSDF volumes in ONE launch (d3f_tsdf_raycast_sparse; the rule is
    csrc/tsdf_raycast_sparse.hpp): ``depth`` f32 [R,H,W] on the device, and ``(depth, normals f32 [R,H,W,3])`` with
    ``normals=True`` -- the outputs, conventions and view arguments of ``tsdf_raycast``.  ``D``, ``w``: the pool [B,512]
    of ``tsdf_integrate_sparse``, device tensors that stay where they are; ``sv`` their ``SparseVolumes``.

    The rule is ``tsdf_raycast``'s with one thing replaced: a corner voxel's D and w come from its brick's pool row, and
    a voxel of an absent brick is D = 0, w = 0.  The render is therefore ``tsdf_raycast`` of ``tsdf_densify(D, w, sv)``
    bit for bit, depth and normals, without the dense volume ever existing.  ``skip=False`` turns off the skipping of the
    samples that stay inside an absent brick (used only when ``min_weight > 0``), which, like ``clip=False``, changes
    the time and no bit (at the default step of 2.5 voxels ``skip=False`` was measured the faster of the two:
    profiles/tsdf_raycast_sparse_bench.txt).  One thread per ray, no atomics, nothing read back: a view's image is
    bit-identical alone, in any batch, from run to run, and to ``tsdf_raycast_sparse_host`` and
    ``tsdf_raycast_sparse_numpy``.  R = 0 returns empty tensors without a launch; B = 0 gives images of zeros.

    ``color=Cp`` (the colour pool [B,512,Cc] of ``tsdf_integrate_sparse(color=)``) appends the colour image f32
    [R,H,W,Cc] (d3f_tsdf_raycast_sparse, channels = Cc), NaN where depth is 0: ``tsdf_raycast(color=)`` of the densified
    pool bit for bit, a corner in an absent brick being w = 0 with colour 0."""
    dev = _tsdf_device()
    with _region("tsdf_raycast_sparse"):
        model = _sparse_model(False, dev, (("D", D), ("w", w), ("color", color)), sv)
        return _tsdf_raycast(False, dev, model, trunc, intrinsics, camera_to_volume, height, width, view_volume, step,
                             depth_min, depth_max, min_weight, normals, clip, bool(skip))


def tsdf_raycast_sparse_host(D, w, sv, trunc, intrinsics, camera_to_volume, height, width, view_volume=None, step=None,
                             depth_min=RAYCAST_DEPTH_MIN, depth_max=TSDF_DEPTH_MAX, min_weight=1.0, normals=False,
                             clip=True, skip=True, color=None):
    """The host twin of ``tsdf_raycast_sparse`` (d3f_tsdf_raycast_sparse_host): CPU tensors (or arrays)
    in, CPU tensors out, no GPU call."""
    cpu = torch.device("cpu")
    model = _sparse_model(True, cpu, (("D", D), ("w", w), ("color", color)), sv)
    return _tsdf_raycast(True, cpu, model, trunc, intrinsics, camera_to_volume, height, width, view_volume, step,
                         depth_min, depth_max, min_weight, normals, clip, bool(skip))


def tsdf_raycast_sparse_numpy(D, w, sv, trunc, intrinsics, camera_to_volume, height, width, view_volume=None,
                              step=None, depth_min=RAYCAST_DEPTH_MIN, depth_max=TSDF_DEPTH_MAX, min_weight=1.0,
                              normals=False, clip=True, skip=True, color=None):
    """The contract of ``tsdf_raycast_sparse`` in NumPy, and the statement of its rule: ``tsdf_raycast_numpy`` of the
    densified pool (colour pool included).  ``skip`` changes no bit and is not restated."""
    dense = tsdf_densify(np.ascontiguousarray(_host_array(D), dtype=np.float32),
                         np.ascontiguousarray(_host_array(w), dtype=np.float32), sv,
                         None if color is None else np.ascontiguousarray(_host_array(color), dtype=np.float32))
    return tsdf_raycast_numpy(dense[0], dense[1], dense[2], sv.origin, sv.dims, sv.voxel, trunc, intrinsics,
                              camera_to_volume, height, width, view_volume, step, depth_min, depth_max, min_weight,
                              normals, clip, dense[3] if color is not None else None)


def tsdf_sample_color_sparse(Cp, w, sv, points, point_start, min_weight=1.0):
    """``tsdf_sample_color`` for sparse volumes (d3f_tsdf_sample_color_sparse): ``Cp`` [B,512,Cc] and ``w`` [B,512] the
    pool of ``tsdf_integrate_sparse(color=)``, ``sv`` its ``SparseVolumes``; ``points`` / ``point_start`` as
    ``tsdf_extract_sparse`` / ``tsdf_mesh_sparse`` return them.  A corner in an absent brick is w = 0 with colour 0, so
    the result is ``tsdf_sample_color`` of the densified pool bit for bit."""
    dev = _tsdf_device()
    with _region("tsdf_sample_color_sparse"):
        return _tsdf_sample_color(False, dev, _sparse_model(False, dev, (("Cp", Cp), ("w", w)), sv), points,
                                  point_start, min_weight)


def tsdf_sample_color_sparse_host(Cp, w, sv, points, point_start, min_weight=1.0):
    """The host twin of ``tsdf_sample_color_sparse`` (d3f_tsdf_sample_color_sparse_host): no GPU call."""
    cpu = torch.device("cpu")
    return _tsdf_sample_color(True, cpu, _sparse_model(True, cpu, (("Cp", Cp), ("w", w)), sv), points, point_start,
                              min_weight)


def tsdf_sample_color_sparse_numpy(Cp, w, sv, points, point_start, min_weight=1.0):
    """The contract of ``tsdf_sample_color_sparse`` in NumPy, and the statement of its rule:
    ``tsdf_sample_color_numpy`` of the densified pool."""
    w = np.ascontiguousarray(_host_array(w), dtype=np.float32)
    _, wd, vs, Cv = tsdf_densify(w, w, sv, np.ascontiguousarray(_host_array(Cp), dtype=np.float32))
    return tsdf_sample_color_numpy(Cv, wd, vs, sv.origin, sv.dims, sv.voxel, points, point_start, min_weight)


def _extend_rows(sv, sv2, D, w, device, color=None):
    """The pool of ``sv2`` (a superset of ``sv``'s bricks over the same lattices) holding the rows of (D, w) -- and of
    the colour pool, when given: every old row at its new place, zeros elsewhere.  Plain tensor indexing on ``device``;
    nothing is read back."""
    B, B2 = sv.bricks, sv2.bricks
    D, w = _sparse_pool(D, w, sv, device)
    out = [torch.zeros((B2, TSDF_BRICK_VOXELS), dtype=torch.float32, device=device) for _ in range(2)]
    if color is not None:
        Cp = _sparse_color_pool(color, sv, device)
        out.append(torch.zeros((B2, TSDF_BRICK_VOXELS, Cp.shape[-1]), dtype=torch.float32, device=device))
    if B:
        def tensor(a, dtype):
            a = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
            return a.to(device=device, dtype=dtype)
        nb = (np.asarray(sv.dims, dtype=np.int64) + (TSDF_BRICK - 1)) // TSDF_BRICK
        tls, tnb = _on(device, sv.lattice_start, nb)
        bs, bs2 = tensor(sv.brick_start, torch.int64), tensor(sv2.brick_start, torch.int64)
        bc, bi2 = tensor(sv.brick_coord, torch.int64), tensor(sv2.brick_index, torch.int64)
        rows = torch.arange(B, dtype=torch.int64, device=device)
        vol = torch.searchsorted(bs[1:].contiguous(), rows, right=True).clamp_(max=sv.volumes - 1)   # the row's volume
        l = tls[vol] + (bc[:, 2] * tnb[vol, 1] + bc[:, 1]) * tnb[vol, 0] + bc[:, 0]
        dst = bs2[vol] + bi2[l]
        out[0][dst] = D.view(B, TSDF_BRICK_VOXELS)
        out[1][dst] = w.view(B, TSDF_BRICK_VOXELS)
        if color is not None:
            out[2][dst] = Cp
    return tuple(out)


def _tsdf_extend(host, device, stream, sv, D, w, depth, frame_start, intrinsics, camera_to_volume, trunc, depth_scale,
                 depth_max, color=None):
    fs = np.asarray(frame_start).reshape(-1)
    if fs.size - 1 != sv.volumes:
        raise ValueError("frame_start names %d volumes, the sparse volumes are %d" % (fs.size - 1, sv.volumes))
    bi = sv.brick_index if isinstance(sv.brick_index, torch.Tensor) else torch.from_numpy(
        np.ascontiguousarray(sv.brick_index))
    bi = bi.to(device=device, dtype=torch.int32)
    if int(bi.numel()) != int(sv.lattice_start[-1]):
        raise ValueError("the tables of the sparse volumes do not fit their dims")
    sv2 = _tsdf_allocate(host, device, stream, depth, frame_start, intrinsics, camera_to_volume, sv.origin, sv.dims,
                         sv.voxel, trunc, depth_scale, depth_max, existing=bi)
    return (sv2,) + _extend_rows(sv, sv2, D, w, device, color)


def tsdf_extend(sv, D, w, depth, frame_start, intrinsics, camera_to_volume, trunc, depth_scale=1000.0,
                depth_max=TSDF_DEPTH_MAX, color=None):
    """Grow the sparse volumes ``sv`` with pool ``(D, w)`` by the bricks that further frames flag: ``(sv2, D2, w2)`` on
    the device (csrc/tsdf_raycast_sparse.hpp).  ``sv2`` holds the bricks of ``sv`` united with those the frames flag
    under ``tsdf_allocate``'s rule -- origin, dims and voxel unchanged, tables in lattice order, so ``sv2`` equals
    ``tsdf_allocate`` over all the frames seen so far, table for table.  Rows that existed are copied to their new place
    bit for bit; new rows hold D = 0, w = 0.  The frame arguments are those of ``tsdf_allocate``; a volume may own no
    frame.  The mark and index launches of ``tsdf_allocate`` do the work, with the flags OR-ed with ``brick_index >= 0``
    between them; the rows move by plain tensor indexing.  ONE read-back: the number of bricks.

    A brick allocated late holds only the frames integrated after it appeared: where earlier frames saw that space as
    free, it is not what the dense volume holds.  ``color=Cp``: the colour pool moves with its rows, new rows hold
    colour 0, and ``(sv2, D2, w2, Cp2)`` is returned; a late brick's colour, like its D, holds only the frames
    integrated after it appeared."""
    dev = _tsdf_device()
    with _region("tsdf_extend"):
        return _tsdf_extend(False, dev, _stream(), sv, D, w, depth, frame_start, intrinsics, camera_to_volume, trunc,
                            depth_scale, depth_max, color)


def tsdf_extend_host(sv, D, w, depth, frame_start, intrinsics, camera_to_volume, trunc, depth_scale=1000.0,
                     depth_max=TSDF_DEPTH_MAX, color=None):
    """The host twin of ``tsdf_extend`` (d3f_tsdf_sparse_mark_host, d3f_tsdf_sparse_index_host): CPU tensors, no GPU
    call."""
    return _tsdf_extend(True, torch.device("cpu"), None, sv, D, w, depth, frame_start, intrinsics, camera_to_volume,
                        trunc, depth_scale, depth_max, color)


def tsdf_extend_numpy(sv, D, w, depth, frame_start, intrinsics, camera_to_volume, trunc, depth_scale=1000.0,
                      depth_max=TSDF_DEPTH_MAX, color=None):
    """The contract of ``tsdf_extend`` in NumPy: ``(sv2, D2, w2)`` of arrays, equal to the device's tables and pool."""
    new = tsdf_allocate_numpy(depth, frame_start, intrinsics, camera_to_volume, sv.origin, sv.dims, sv.voxel, trunc,
                              depth_scale, depth_max)
    old_index, old_start = _host_array(sv.brick_index), _host_array(sv.brick_start).astype(np.int64)
    ls = sv.lattice_start
    n = np.asarray(sv.dims, dtype=np.int64)
    index, coords, brick_start = [], [], np.zeros(sv.volumes + 1, dtype=np.int64)
    for v in range(sv.volumes):
        flat = (old_index[ls[v]:ls[v + 1]] >= 0) | (new.brick_index[ls[v]:ls[v + 1]] >= 0)
        nb = (n[v] + (TSDF_BRICK - 1)) // TSDF_BRICK
        index.append(np.where(flat, np.cumsum(flat) - 1, -1).astype(np.int32))
        local = np.flatnonzero(flat)                                # lattice order
        coords.append(np.stack([local % nb[0], (local // nb[0]) % nb[1], local // (nb[0] * nb[1])],
                               axis=1).astype(np.int32))
        brick_start[v + 1] = brick_start[v] + local.size
    sv2 = SparseVolumes(np.concatenate(index), np.concatenate(coords, 0).reshape(-1, 3), brick_start, sv.origin,
                        sv.dims, sv.voxel)
    B = sv.bricks
    D = np.ascontiguousarray(_host_array(D), dtype=np.float32).reshape(-1)
    w = np.ascontiguousarray(_host_array(w), dtype=np.float32).reshape(-1)
    if D.size != B * TSDF_BRICK_VOXELS or w.size != D.size:
        raise ValueError("D and w must hold the %d x 512 slots of the allocated bricks" % B)
    D2 = np.zeros((sv2.bricks, TSDF_BRICK_VOXELS), dtype=np.float32)
    w2 = np.zeros((sv2.bricks, TSDF_BRICK_VOXELS), dtype=np.float32)
    Cp = Cp2 = None
    if color is not None:
        Cp = np.ascontiguousarray(_host_array(color), dtype=np.float32).reshape(B, TSDF_BRICK_VOXELS, -1)
        Cp2 = np.zeros((sv2.bricks, TSDF_BRICK_VOXELS, Cp.shape[-1]), dtype=np.float32)
    for v in range(sv.volumes):
        kept = np.flatnonzero(old_index[ls[v]:ls[v + 1]] >= 0)
        src = old_start[v] + old_index[ls[v]:ls[v + 1]][kept]
        dst = brick_start[v] + sv2.brick_index[ls[v]:ls[v + 1]][kept]
        D2[dst] = D.reshape(B, TSDF_BRICK_VOXELS)[src]
        w2[dst] = w.reshape(B, TSDF_BRICK_VOXELS)[src]
        if Cp is not None:
            Cp2[dst] = Cp[src]
    return (sv2, D2, w2) + ((Cp2,) if Cp is not None else ())


# ---------------------------------------------------------------------------------------------------------------
# Depth odometry: camera poses of a depth sequence by projective point-to-plane ICP over a depth pyramid
# (csrc/odometry.hpp has the rule; csrc/odometry.hip the kernels, of this section and the next)
# ---------------------------------------------------------------------------------------------------------------
ODO_ST_FEW = _native.D3F_ODO_ST_FEW               # the final association has fewer than 6 accepted pixels
ODO_ST_PAIR = _native.D3F_ODO_ST_PAIR             # a frame index outside [0, F)
ODO_ST_NONFINITE = _native.D3F_ODO_ST_NONFINITE   # T_init holds a non-finite value
ODO_ST_SINGULAR = _native.D3F_ODO_ST_SINGULAR     # the last fit at level 0 was singular (e.g. a view of a single plane)
ODO_MAX_LEVELS = _native.D3F_ODO_MAX_LEVELS
ODO_MAX_ITERS = _native.D3F_ODO_MAX_ITERS
ODO_MAX_PAIRS = 65535
ODO_SUMS = _native.D3F_ODO_SUMS                   # n, the 21 upper entries of sum J J^T, sum J r (6), sum d2
ODO_MIN_PIXELS = 6
ODO_ITERATIONS = (10, 5, 4)
ODO_MAX_DISTANCE = 0.1
ODO_DEPTH_DIFF = 0.05


def depth_pyramid_pixels(H, W, levels):
    """Pixels of one frame's packed pyramid: the sum of ``(H >> l) * (W >> l)`` over the levels."""
    return sum((int(H) >> l) * (int(W) >> l) for l in range(int(levels)))


class DepthPyramid(object):
    """The packed depth pyramid of F frames and its level table (``depth_pyramid``).  ``data`` f32 [F, pixels]: the
    levels of a frame one after another, level l being ``(H >> l) x (W >> l)`` pixels in raster order (metres, 0 where
    invalid); ``K`` f32 [F, levels, 4] the intrinsics of every level; ``table`` int64 [levels, 3] = rows, columns and
    pixel offset of a level inside a frame (host values); ``depth_diff`` what the levels were built with (the normals
    use it again).  ``data`` and ``K`` are device tensors, CPU tensors (host twin) or NumPy arrays (restatement)."""

    def __init__(self, data, K, H, W, levels, depth_diff):
        self.data, self.K, self.H, self.W, self.levels = data, K, int(H), int(W), int(levels)
        self.depth_diff = float(depth_diff)
        self.frames = int(data.shape[0])
        off = np.cumsum([0] + [(self.H >> l) * (self.W >> l) for l in range(self.levels)])
        self.table = np.array([[self.H >> l, self.W >> l, off[l]] for l in range(self.levels)], dtype=np.int64)

    def level(self, l):
        """Level ``l`` of all frames as a view [F, H_l, W_l]."""
        h, w, off = (int(x) for x in self.table[l])
        return self.data[:, off:off + h * w].reshape(self.frames, h, w)


def _odo_check_levels(H, W, levels):
    levels = int(levels)
    if not 1 <= levels <= ODO_MAX_LEVELS or (H >> (levels - 1)) < 1 or (W >> (levels - 1)) < 1:
        raise ValueError("levels must be in 1..%d and leave every level of a %d x %d image a pixel, got %d"
                         % (ODO_MAX_LEVELS, W, H, levels))
    return levels


def _odo_frames(depth, intrinsics, device_ok=False):
    """Host form of the frames: (depth [F,H,W] uint16 / f32, K f32 [F,4]); with ``device_ok`` a device f32 tensor stays
    one."""
    d = _tsdf_depth_array(depth, device_ok)
    if d.shape[0] < 1:
        raise ValueError("depth holds no frame")
    K = np.asarray(intrinsics.cpu() if isinstance(intrinsics, torch.Tensor) else intrinsics, dtype=np.float32)
    return d, np.ascontiguousarray(np.broadcast_to(K.reshape(-1, 4), (d.shape[0], 4)))


def _depth_pyramid(host, device, depth, intrinsics, levels, depth_scale, depth_max, depth_diff):
    d, K = _odo_frames(depth, intrinsics, device_ok=not host)
    F, H, W = (int(k) for k in d.shape)
    levels = _odo_check_levels(H, W, levels)
    if isinstance(d, torch.Tensor):                   # f32 metres already on the device: no round trip
        td, is_f32 = d, 1
        tK, = _on(device, K)
    else:
        td, tK = _on(device, d, K)
        is_f32 = int(d.dtype != np.uint16)
    data = torch.empty((F, depth_pyramid_pixels(H, W, levels)), dtype=torch.float32, device=device)
    KL = torch.empty((F, levels, 4), dtype=torch.float32, device=device)
    L = _native.lib()
    args = (_p(td), is_f32, F, H, W, _p(tK), levels, float(depth_scale), float(depth_max),
            float(depth_diff), _p(data), _p(KL))
    if host:
        _native.check(L.d3f_depth_pyramid_host(*args), "d3f_depth_pyramid_host")
    else:
        _native.check(L.d3f_depth_pyramid(*(args + (_stream(),))), "d3f_depth_pyramid")
    return DepthPyramid(data, KL, H, W, levels, depth_diff)


def depth_pyramid(depth, intrinsics, levels=3, depth_scale=1000.0, depth_max=TSDF_DEPTH_MAX, depth_diff=ODO_DEPTH_DIFF):
    """The depth pyramid of F frames on the device (d3f_depth_pyramid; the rule is csrc/odometry.hpp): a
    ``DepthPyramid`` -- the packed pyramid ``.data`` f32 [F, pixels], the level table ``.table`` and the intrinsics of
    every level ``.K``.  ``depth`` [F,H,W] uint16 raw units (metres = raw / ``depth_scale``) or f32 metres (a device
    f32 tensor, such as ``tsdf_raycast``'s, is taken where it is);
    ``intrinsics`` [4] or [F,4] = fx, fy, cx, cy.  Level 0 is the depth in metres, 0 where invalid (not ``d > 0``, or
    ``d > depth_max``: a NaN and an infinity too); level l+1 halves level l (an odd last row or column is dropped),
    a pixel being the mean of the valid pixels of its 2x2 block and 0 when there is none or when they span more than
    ``depth_diff``.  Equal to the host twin and ``depth_pyramid_numpy`` bit for bit."""
    dev = _tsdf_device()
    with _region("depth_pyramid"):
        return _depth_pyramid(False, dev, depth, intrinsics, levels, depth_scale, depth_max, depth_diff)


def depth_pyramid_host(depth, intrinsics, levels=3, depth_scale=1000.0, depth_max=TSDF_DEPTH_MAX,
                       depth_diff=ODO_DEPTH_DIFF):
    """The host twin of ``depth_pyramid`` (d3f_depth_pyramid_host): CPU tensors, no GPU call."""
    return _depth_pyramid(True, torch.device("cpu"), depth, intrinsics, levels, depth_scale, depth_max, depth_diff)


def _odo_pairs(pairs, T, name):
    """Host form of a pair list: (pairs int32 [P,2], T f64 [P,12]); ``T`` None gives identities."""
    pr = np.ascontiguousarray(np.asarray(_host_array(pairs), dtype=np.int64).reshape(-1, 2))
    P = pr.shape[0]
    if P > ODO_MAX_PAIRS:
        raise ValueError("at most %d pairs per call, got %d" % (ODO_MAX_PAIRS, P))
    if (np.abs(pr) > 0x7fffffff).any():
        raise ValueError("%s: frame indices must fit an int32" % name)
    if T is None:
        T = np.broadcast_to(np.eye(4), (P, 4, 4))
    t = np.asarray(_host_array(T), dtype=np.float64)
    if t.ndim == 2 and P == 1:
        t = t[None]
    if t.ndim != 3 or t.shape[0] != P or t.shape[1:] not in ((4, 4), (3, 4)):
        raise ValueError("%s: T must be [%d,4,4] or [%d,3,4], got %s" % (name, P, P, t.shape))
    return pr.astype(np.int32), np.ascontiguousarray(t[:, :3, :].reshape(P, 12))


def _odo_check_distance(max_distance):
    if not float(max_distance) > 0.0:
        raise ValueError("max_distance must be positive")
    return float(max_distance)


def _odo_check_level(level, pyr):
    if not 0 <= int(level) < pyr.levels:
        raise ValueError("level must be in 0..%d, got %d" % (pyr.levels - 1, int(level)))
    return int(level)


def _odo_call(stem, what, host, pyr, pr, t, rest):
    """Calls d3f_<stem>_odometry<what> (with its workspace, on the stream) or its ``_host`` twin: the pyramid, the
    pairs and their poses, then ``rest``.  ``stem`` 'rgbd' passes the intensity too."""
    device = pyr.data.device
    tp, tt = _on(device, pr, t)
    L = _native.lib()
    P = pr.shape[0]
    name = "d3f_%s_odometry%s" % (stem, what)
    args = ((_p(pyr.data),) + ((_p(pyr.intensity),) if stem == "rgbd" else ())
            + (_p(pyr.K), pyr.frames, pyr.H, pyr.W, pyr.levels, _p(tp), P, _p(tt)) + rest)
    if host:
        _native.check(getattr(L, name + "_host")(*args), name + "_host")
    else:
        nbytes = getattr(L, "d3f_%s_odometry_ws_bytes" % stem)(P, pyr.H, pyr.W)
        ws = _ws(nbytes, device)
        _native.check(getattr(L, name)(*(args + (_p(ws), nbytes, _stream()))), name)


def _odo_step(host, pyr, pairs, T, level, max_distance, photo_weight, return_index):
    """One association on the host or the device; ``photo_weight`` None: the depth entry points, else the RGB-D
    ones."""
    stem = "depth" if photo_weight is None else "rgbd"
    device = pyr.data.device
    pr, t = _odo_pairs(pairs, T, stem + "_odometry_step")
    level, P = _odo_check_level(level, pyr), pr.shape[0]
    weight = () if photo_weight is None else (_rgbd_check_weight(photo_weight),)
    h, w = int(pyr.table[level, 0]), int(pyr.table[level, 1])
    sums = torch.zeros((P, RGBD_SUMS if weight else ODO_SUMS), dtype=torch.float64, device=device)
    index = torch.full((P, h, w), -1, dtype=torch.int32, device=device) if return_index else None
    if P:
        _odo_call(stem, "_step", host, pyr, pr, t, (level, _odo_check_distance(max_distance), pyr.depth_diff) + weight
                  + (_p(sums), _p(index)))
    return (sums, index) if return_index else sums


def _odo_checked_pyramid(pyr, what, cls, host):
    """``pyr`` when it is a ``cls`` (DepthPyramid or RgbdPyramid) of CPU tensors (``host``) or of device tensors."""
    if isinstance(pyr, cls) and isinstance(pyr.data, torch.Tensor) and pyr.data.is_cuda != host:
        return pyr
    made_by = "ops.rgbd_pyramid" if cls is RgbdPyramid else "ops.depth_pyramid"
    if host:
        raise RuntimeError("%s takes the %s of %s_host (CPU tensors)" % (what, cls.__name__, made_by))
    raise RuntimeError("%s takes the %s of %s (on the device); the host twin is %s_host, "
                       "the NumPy restatement %s_numpy" % (what, cls.__name__, made_by, what, what))


def depth_odometry_step(pyr, pairs, T, level, max_distance=ODO_MAX_DISTANCE, return_index=False):
    """ONE association of P frame pairs at ``level`` under ``T`` (d3f_depth_odometry_step): ``sums`` f64 [P,29] on the
    device -- n, the 21 upper entries of sum J J^T row by row, sum J r (6), sum d2 of the accepted pixels, with
    ``J = [a x n, n]`` and ``r = (a - y) . n``.  ``pairs`` [P,2] = (moving frame a, fixed frame b), ``T`` [P,4,4] maps
    a's camera frame into b's.  ``return_index=True`` appends int32 [P, H_l, W_l]: per moving pixel the raster index of
    the accepted fixed pixel, or -1.  A pair that names a frame outside the pyramid, or whose T is not finite, gives
    zero sums and -1 everywhere."""
    _odo_checked_pyramid(pyr, "depth_odometry_step", DepthPyramid, False)
    with _region("depth_odometry_step"):
        return _odo_step(False, pyr, pairs, T, level, max_distance, None, return_index)


def depth_odometry_step_host(pyr, pairs, T, level, max_distance=ODO_MAX_DISTANCE, return_index=False):
    """The host twin of ``depth_odometry_step`` (d3f_depth_odometry_step_host): the same rule pixel by pixel in raster
    order, CPU tensors, no GPU call."""
    return _odo_step(True, _odo_checked_pyramid(pyr, "depth_odometry_step_host", DepthPyramid, True), pairs, T, level,
                     max_distance, None, return_index)


def _odo_iterations(iterations, levels=None):
    it = [int(k) for k in np.asarray(iterations).reshape(-1)]
    if not it or len(it) > ODO_MAX_LEVELS or min(it) < 0 or max(it) > ODO_MAX_ITERS:
        raise ValueError("iterations must hold 1..%d counts in 0..%d (finest level first), got %s"
                         % (ODO_MAX_LEVELS, ODO_MAX_ITERS, it))
    if levels is not None and len(it) != levels:
        raise ValueError("%d iteration counts for a pyramid of %d levels" % (len(it), levels))
    return it


def _odometry(host, pyr, pairs, T_init, iterations, max_distance, photo_weight, return_information):
    """The whole odometry on the host or the device; ``photo_weight`` None: the depth entry points, else the RGB-D
    ones, whose ``n_photo`` ends the result."""
    stem = "depth" if photo_weight is None else "rgbd"
    device = pyr.data.device
    pr, t = _odo_pairs(pairs, T_init, stem + "_odometry")
    it = _odo_iterations(iterations, pyr.levels)
    weight = () if photo_weight is None else (_rgbd_check_weight(photo_weight),)
    P = pr.shape[0]
    T = torch.zeros((P, 4, 4), dtype=torch.float64, device=device)
    count = torch.zeros(P, dtype=torch.int32, device=device)
    rmse = torch.zeros(P, dtype=torch.float64, device=device)
    status = torch.zeros(P, dtype=torch.int32, device=device)
    n_photo = (torch.zeros(P, dtype=torch.int32, device=device),) if weight else ()
    info = torch.zeros((P, 6, 6), dtype=torch.float64, device=device) if return_information else None
    if P:
        counts = (ctypes.c_int32 * len(it))(*it)
        _odo_call(stem, "", host, pyr, pr, t,
                  (ctypes.cast(counts, ctypes.c_void_p), _odo_check_distance(max_distance), pyr.depth_diff) + weight
                  + (_p(T), _p(count), _p(rmse), _p(status)) + tuple(_p(n) for n in n_photo) + (_p(info),))
    return (T, count, rmse, status) + ((info,) if return_information else ()) + n_photo


def depth_odometry(pyr_or_depth, pairs, T_init=None, iterations=ODO_ITERATIONS, max_distance=ODO_MAX_DISTANCE,
                   return_information=False, intrinsics=None, depth_scale=1000.0, depth_max=TSDF_DEPTH_MAX,
                   depth_diff=ODO_DEPTH_DIFF):
    """Relative poses of P frame pairs by projective point-to-plane ICP over the depth pyramid, all pairs in one launch
    sequence (d3f_depth_odometry; the rule is csrc/odometry.hpp -- KinectFusion's tracker, frame to frame).

    ``pyr_or_depth``: the ``DepthPyramid`` of ``depth_pyramid``, or depth frames [F,H,W] with ``intrinsics`` (the
    pyramid of ``len(iterations)`` levels is then built here with ``depth_scale``, ``depth_max``, ``depth_diff``).
    ``pairs`` [P,2] = (moving frame a, fixed frame b) and T maps a's camera frame into b's -- the (source, target,
    transform) convention of ``icp_rigid``; with camera-to-world poses, ``T = inv(pose_b) @ pose_a``.  ``T_init``
    [P,4,4] f64 (None: identities).  ``iterations[l]`` fits at level l (0 the finest), coarsest level first, fixed
    counts: no host synchronisation, nothing read back.  An iteration projects every valid pixel of a into b, takes
    b's pixel there with the normal computed from b's depth, accepts within ``max_distance`` and solves the 6x6
    point-to-plane system; fewer than 6 accepted pixels or a singular system leave T as it is.

    Returns device tensors ``(T f64 [P,4,4], count int32 [P], rmse f64 [P], status int32 [P])``: count and rmse of one
    more association at level 0 under the final T.  ``status``: ODO_ST_FEW (that association has fewer than 6 pixels),
    ODO_ST_SINGULAR (the last fit at level 0 was singular: a view of a single plane), ODO_ST_PAIR (a frame outside the
    pyramid), ODO_ST_NONFINITE (a non-finite T_init); each leaves T = T_init and gives count 0.
    ``return_information=True`` appends f64 [P,6,6] = sum J J^T of that association, ``J = [a x n, n]``: ROTATION
    FIRST, in the FIXED frame b, point-to-plane -- not the point-to-point form of
    ``registration.information_from_moments``, whose default is translation first in the moving frame; its
    ``frame='fixed', order='rotation_first'`` has the same layout.  A pair's result is bit-identical alone, in any
    batch, and from run to run."""
    if isinstance(pyr_or_depth, DepthPyramid):
        pyr = _odo_checked_pyramid(pyr_or_depth, "depth_odometry", DepthPyramid, False)
    else:
        if intrinsics is None:
            raise ValueError("depth frames need intrinsics")
        pyr = depth_pyramid(pyr_or_depth, intrinsics, len(_odo_iterations(iterations)), depth_scale, depth_max,
                            depth_diff)
    with _region("depth_odometry"):
        return _odometry(False, pyr, pairs, T_init, iterations, max_distance, None, return_information)


def depth_odometry_host(pyr_or_depth, pairs, T_init=None, iterations=ODO_ITERATIONS, max_distance=ODO_MAX_DISTANCE,
                        return_information=False, intrinsics=None, depth_scale=1000.0, depth_max=TSDF_DEPTH_MAX,
                        depth_diff=ODO_DEPTH_DIFF):
    """The host twin of ``depth_odometry`` (d3f_depth_odometry_host): CPU tensors, no GPU call.  It sums in raster
    order, so T agrees with the device's to rounding (1e-6), not bit for bit."""
    if isinstance(pyr_or_depth, DepthPyramid):
        pyr = _odo_checked_pyramid(pyr_or_depth, "depth_odometry_host", DepthPyramid, True)
    else:
        if intrinsics is None:
            raise ValueError("depth frames need intrinsics")
        pyr = depth_pyramid_host(pyr_or_depth, intrinsics, len(_odo_iterations(iterations)), depth_scale, depth_max,
                                 depth_diff)
    return _odometry(True, pyr, pairs, T_init, iterations, max_distance, None, return_information)


# ------------------------------------------------------------------------------------------- NumPy restatement
def depth_pyramid_numpy(depth, intrinsics, levels=3, depth_scale=1000.0, depth_max=TSDF_DEPTH_MAX,
                        depth_diff=ODO_DEPTH_DIFF):
    """The contract of ``depth_pyramid`` in NumPy: a ``DepthPyramid`` of NumPy arrays, equal to the kernel's bit for
    bit (every f32 operation in the order of csrc/odometry.hpp)."""
    d, K = _odo_frames(depth, intrinsics)
    F, H, W = d.shape
    levels = _odo_check_levels(H, W, levels)
    f32 = np.float32
    dd = f32(depth_diff)
    data = np.zeros((F, depth_pyramid_pixels(H, W, levels)), dtype=f32)
    with np.errstate(all='ignore'):
        dm = d.astype(f32) / f32(depth_scale) if d.dtype == np.uint16 else d
        cur = np.where((dm > 0) & ~(dm > f32(depth_max)), dm, f32(0.0)).astype(f32)
        off = 0
        for l in range(levels):
            h, w = cur.shape[1:]
            data[:, off:off + h * w] = cur.reshape(F, -1)
            off += h * w
            if l + 1 == levels:
                break
            hn, wn = h >> 1, w >> 1
            total = np.zeros((F, hn, wn), dtype=f32)
            k = np.zeros((F, hn, wn), dtype=np.int32)
            lo = np.full((F, hn, wn), np.inf, dtype=f32)
            hi = np.full((F, hn, wn), -np.inf, dtype=f32)
            for dy in range(2):
                for dx in range(2):
                    b = cur[:, dy:2 * hn:2, dx:2 * wn:2]
                    ok = b > 0
                    total = np.where(ok, total + b, total)
                    lo = np.where(ok, np.minimum(lo, b), lo)
                    hi = np.where(ok, np.maximum(hi, b), hi)
                    k += ok
            cur = np.where((k == 0) | (hi - lo > dd), f32(0.0), total / k.astype(f32)).astype(f32)
    KL = np.zeros((F, levels, 4), dtype=f32)
    KL[:, 0] = K
    for l in range(1, levels):
        KL[:, l, 0] = KL[:, l - 1, 0] / f32(2.0)
        KL[:, l, 1] = KL[:, l - 1, 1] / f32(2.0)
        KL[:, l, 2] = (KL[:, l - 1, 2] - f32(0.5)) / f32(2.0)
        KL[:, l, 3] = (KL[:, l - 1, 3] - f32(0.5)) / f32(2.0)
    return DepthPyramid(data, KL, H, W, levels, depth_diff)


def _odo_numpy_pyramid(pyr):
    if not isinstance(pyr, DepthPyramid):
        raise ValueError("expected a DepthPyramid")
    if isinstance(pyr.data, np.ndarray):
        return pyr
    return DepthPyramid(_host_array(pyr.data), _host_array(pyr.K), pyr.H, pyr.W, pyr.levels, pyr.depth_diff)


def _odo_vertices(img, K):
    """(X, Y, Z) f32 [H,W] of a level image: vertex() of csrc/odometry.hpp for every pixel."""
    h, w = img.shape
    u = np.arange(w, dtype=np.float32)[None, :]
    v = np.arange(h, dtype=np.float32)[:, None]
    return ((u - K[2]) * img) / K[0], ((v - K[3]) * img) / K[1], img


def _odo_normals(img, K, depth_diff):
    """normal_at() of csrc/odometry.hpp for every pixel of a level image: (has bool [H,W], n f32 [3,H,W], V f32
    [3,H,W])."""
    f32 = np.float32
    h, w = img.shape
    V = np.stack(_odo_vertices(img, K)).astype(f32)
    has = np.zeros((h, w), dtype=bool)
    n = np.zeros((3, h, w), dtype=f32)
    if h < 3 or w < 3:
        return has, n, V
    dd = f32(depth_diff)
    c, le, ri, up, dn = img[1:-1, 1:-1], img[1:-1, :-2], img[1:-1, 2:], img[:-2, 1:-1], img[2:, 1:-1]
    ok = (c > 0) & (le > 0) & (ri > 0) & (up > 0) & (dn > 0)
    for nb in (le, ri, up, dn):
        ok &= np.abs(nb - c) <= dd
    e1 = [A[1:-1, 2:] - A[1:-1, :-2] for A in V]
    e2 = [A[2:, 1:-1] - A[:-2, 1:-1] for A in V]
    c0 = e1[1] * e2[2] - e1[2] * e2[1]
    c1 = e1[2] * e2[0] - e1[0] * e2[2]
    c2 = e1[0] * e2[1] - e1[1] * e2[0]
    ln = np.sqrt((c0 * c0 + c1 * c1) + c2 * c2)
    ok &= (ln > 0) & np.isfinite(ln)
    nn = [c0 / ln, c1 / ln, c2 / ln]
    Vc = V[:, 1:-1, 1:-1]
    flip = (nn[0] * Vc[0] + nn[1] * Vc[1]) + nn[2] * Vc[2] > 0
    for r in range(3):
        n[r, 1:-1, 1:-1] = np.where(ok, np.where(flip, -nn[r], nn[r]), f32(0.0))
    has[1:-1, 1:-1] = ok
    return has, n, V


def _odo_associate_numpy(A_img, Ka, fixed, Kb, T12, max_distance):
    """associate() of csrc/odometry.hpp for every pixel of the moving level image: (index int32 [H,W], a, y, n f32
    [3,m] of the accepted pixels in raster order).  ``fixed`` = ``_odo_normals`` of the fixed image."""
    f32 = np.float32
    has, nb, Vb = fixed
    h, w = A_img.shape
    M = np.asarray(T12, dtype=np.float64).reshape(12).astype(f32)
    md = f32(max_distance)
    X, Y, Z = _odo_vertices(A_img, Ka)
    ok = A_img > 0
    a = [((M[4 * r] * X + M[4 * r + 1] * Y) + M[4 * r + 2] * Z) + M[4 * r + 3] for r in range(3)]
    ok &= a[2] > 0
    up = np.floor(((Kb[0] * a[0]) / a[2] + Kb[2]) + f32(0.5))
    vp = np.floor(((Kb[1] * a[1]) / a[2] + Kb[3]) + f32(0.5))
    ok &= (up >= 0) & (up < f32(w)) & (vp >= 0) & (vp < f32(h))
    ui = np.where(ok, up, 0).astype(np.int64)
    vi = np.where(ok, vp, 0).astype(np.int64)
    ok &= has[vi, ui]
    y = [Vb[r][vi, ui] for r in range(3)]
    e = [a[r] - y[r] for r in range(3)]
    ok &= (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] <= md * md
    index = np.where(ok, vi * w + ui, -1).astype(np.int32)
    pick = lambda rows: np.stack([np.asarray(x, dtype=f32)[ok] for x in rows])
    return index, pick(a), pick(y), np.stack([nb[r][vi, ui][ok] for r in range(3)])


_ODO_UPPER = [(i, j) for i in range(6) for j in range(i, 6)]


def _odo_terms(a, y, n):
    """add_pixel() of csrc/odometry.hpp: f64 [m,29], what every accepted pixel adds to the sums."""
    a, y, n = (x.astype(np.float64) for x in (a, y, n))
    e = a - y
    J = [a[1] * n[2] - a[2] * n[1], a[2] * n[0] - a[0] * n[2], a[0] * n[1] - a[1] * n[0], n[0], n[1], n[2]]
    r = (e[0] * n[0] + e[1] * n[1]) + e[2] * n[2]
    cols = [np.ones_like(r)] + [J[i] * J[j] for i, j in _ODO_UPPER] + [J[i] * r for i in range(6)]
    cols.append((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
    return np.stack(cols, axis=1) if r.size else np.zeros((0, ODO_SUMS))


def _odo_pair_ok(pr, t, F):
    return 0 <= pr[0] < F and 0 <= pr[1] < F and bool(np.isfinite(t).all())


def _odo_pair_terms(pyr, level, a, b, t, md, normals=None):
    """(index int32 [H_l,W_l], a f32 [3,m], terms f64 [m,29]) of one association of the pair (a, b), the accepted
    pixels in raster order.  ``normals``: a cache of ``_odo_normals`` by (fixed frame, level)."""
    imgs = pyr.level(level)
    key = (b, level)
    fixed = normals.get(key) if normals is not None else None
    if fixed is None:
        fixed = _odo_normals(imgs[b], pyr.K[b, level], pyr.depth_diff)
        if normals is not None:
            normals[key] = fixed
    index, av, yv, nv = _odo_associate_numpy(imgs[a], pyr.K[a, level], fixed, pyr.K[b, level], t, md)
    return index, av, _odo_terms(av, yv, nv)


def _odo_step_numpy(pyr, pr, t, level, n_sums, pair_terms, return_index, return_terms):
    """The per-pair loop of the ``*_odometry_step_numpy`` functions: ``pair_terms(a, b, t)`` gives the index and the
    f64 [rows, n_sums] terms of one valid pair."""
    h, w = int(pyr.table[level, 0]), int(pyr.table[level, 1])
    sums = np.zeros((pr.shape[0], n_sums))
    index = np.full((pr.shape[0], h, w), -1, dtype=np.int32)
    terms = []
    with np.errstate(all='ignore'):
        for p in range(pr.shape[0]):
            terms.append(np.zeros((0, n_sums)))
            if not _odo_pair_ok(pr[p], t[p], pyr.frames):
                continue
            index[p], terms[-1] = pair_terms(int(pr[p, 0]), int(pr[p, 1]), t[p])
            sums[p] = terms[-1].sum(axis=0)
    res = (sums,) + ((index,) if return_index else ()) + ((terms,) if return_terms else ())
    return res if len(res) > 1 else sums


def depth_odometry_step_numpy(pyr, pairs, T, level, max_distance=ODO_MAX_DISTANCE, return_index=False,
                              return_terms=False):
    """The contract of ``depth_odometry_step`` in NumPy: ``sums`` f64 [P,29] (NumPy's own summation order: equal to
    the kernel's within the summation bound, not bit for bit) and, with ``return_index``, the index int32 [P,H_l,W_l],
    which is equal.  ``return_terms=True`` appends the list of the f64 [m_p,29] terms the sums are made of."""
    pyr = _odo_numpy_pyramid(pyr)
    pr, t = _odo_pairs(pairs, T, "depth_odometry_step_numpy")
    level = _odo_check_level(level, pyr)

    def pair_terms(a, b, tp):
        index, _, terms = _odo_pair_terms(pyr, level, a, b, tp, _odo_check_distance(max_distance))
        return index, terms

    return _odo_step_numpy(pyr, pr, t, level, ODO_SUMS, pair_terms, return_index, return_terms)


_ODO_PLANE_PIVOT = 1e-10      # kPlanePivot of csrc/plane.hpp


def _odo_plane_step(sums, T12):
    """fit() of csrc/odometry.hpp (plane_step of csrc/plane.hpp with a zero pivot) -> (T_next [12], moved, singular):
    the pivot test is the kernel's Cholesky; the solution is NumPy's solve of the same system."""
    if sums[0] < ODO_MIN_PIXELS:
        return T12, False, False
    A = np.zeros((6, 6))
    for k, (i, j) in enumerate(_ODO_UPPER):
        A[i, j] = A[j, i] = sums[1 + k]
    floor, U = _ODO_PLANE_PIVOT * A.diagonal().max(), np.zeros((6, 6))
    for i in range(6):
        d = A[i, i] - (U[:i, i] ** 2).sum()
        if not d > floor:
            return T12, False, True
        U[i, i] = np.sqrt(d)
        U[i, i + 1:] = (A[i, i + 1:] - U[:i, i] @ U[:i, i + 1:]) / U[i, i]
    v = np.linalg.solve(A, -sums[22:28])
    ca, sa, cb, sb, cg, sg = np.cos(v[0]), np.sin(v[0]), np.cos(v[1]), np.sin(v[1]), np.cos(v[2]), np.sin(v[2])
    D = np.array([[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa],
                  [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa],
                  [-sb, cb * sa, cb * ca]])                            # Rz(gamma) Ry(beta) Rx(alpha)
    Tk = T12.reshape(3, 4)
    out = np.empty((3, 4))
    out[:, :3] = D @ Tk[:, :3]
    out[:, 3] = D @ Tk[:, 3] + v[3:]
    return out.reshape(12), True, False


def _odo_march_numpy(pyr, pr, t0, it, sums_at, return_information, photo=False):
    """The coarse-to-fine march of the ``*_odometry_numpy`` functions over P pairs from the poses ``t0`` [P,12]:
    ``sums_at(p, level, t)`` gives the sums of one association of pair p: 29 of them, or with ``photo`` 31, and
    ``n_photo`` then ends the result."""
    P = pr.shape[0]
    T = np.zeros((P, 4, 4))
    T[:, 3, 3] = 1.0
    T[:, :3, :] = t0.reshape(P, 3, 4)
    count = np.zeros(P, dtype=np.int32)
    rmse = np.zeros(P)
    status = np.zeros(P, dtype=np.int32)
    n_photo = np.zeros(P, dtype=np.int32)
    info = np.zeros((P, 6, 6))
    with np.errstate(all='ignore'):
        for p in range(P):
            if not (0 <= pr[p, 0] < pyr.frames and 0 <= pr[p, 1] < pyr.frames):
                status[p] |= ODO_ST_PAIR
            if not np.isfinite(t0[p]).all():
                status[p] |= ODO_ST_NONFINITE
            if status[p]:
                continue
            t, singular = t0[p].copy(), False
            for level in range(pyr.levels - 1, -1, -1):
                for _ in range(it[level]):
                    t, _moved, s = _odo_plane_step(sums_at(p, level, t), t)
                    if level == 0:
                        singular = s
            sums = sums_at(p, 0, t)
            if sums[0] < ODO_MIN_PIXELS:
                status[p] = ODO_ST_FEW
            elif singular:
                status[p] = ODO_ST_SINGULAR
            else:
                T[p, :3, :] = t.reshape(3, 4)
                count[p] = int(sums[0])
                rmse[p] = np.sqrt(sums[28] / sums[0])
                if photo:
                    n_photo[p] = int(sums[29])
                for k, (i, j) in enumerate(_ODO_UPPER):
                    info[p, i, j] = info[p, j, i] = sums[1 + k]
    return (T, count, rmse, status) + ((info,) if return_information else ()) + ((n_photo,) if photo else ())


def depth_odometry_numpy(pyr_or_depth, pairs, T_init=None, iterations=ODO_ITERATIONS, max_distance=ODO_MAX_DISTANCE,
                         return_information=False, intrinsics=None, depth_scale=1000.0, depth_max=TSDF_DEPTH_MAX,
                         depth_diff=ODO_DEPTH_DIFF):
    """The contract of ``depth_odometry`` in NumPy: ``(T f64 [P,4,4], count int32 [P], rmse f64 [P], status int32 [P])``
    (and the information matrices [P,6,6]); T agrees with the kernel's to rounding, not bit for bit."""
    it = _odo_iterations(iterations)
    if isinstance(pyr_or_depth, DepthPyramid):
        pyr = _odo_numpy_pyramid(pyr_or_depth)
        _odo_iterations(iterations, pyr.levels)
    else:
        if intrinsics is None:
            raise ValueError("depth frames need intrinsics")
        pyr = depth_pyramid_numpy(pyr_or_depth, intrinsics, len(it), depth_scale, depth_max, depth_diff)
    pr, t0 = _odo_pairs(pairs, T_init, "depth_odometry_numpy")
    md = _odo_check_distance(max_distance)
    normals = {}
    sums_at = lambda p, level, t: _odo_pair_terms(pyr, level, int(pr[p, 0]), int(pr[p, 1]), t, md,
                                                  normals)[2].sum(axis=0)
    return _odo_march_numpy(pyr, pr, t0, it, sums_at, return_information)


# ---------------------------------------------------------------------------------------------------------------
# RGB-D odometry: the depth odometry with a photometric term (csrc/rgbd_odometry.hpp has the rule; the kernels and
# the helpers that take ``photo_weight`` are the depth odometry's)
# ---------------------------------------------------------------------------------------------------------------
RGBD_SUMS = _native.D3F_RGBD_SUMS   # the 29 of the depth odometry (both kinds of rows in sum J J^T and sum J r), n_photo, sum r_I^2
ODO_PHOTO_WEIGHT = 0.3   # profiles/rgbd_odometry_weight_sweep.txt: the largest of the swept weights that meets both
#                          conditions of the sweep (the planar slide recovered, the textured room no worse than twice
#                          the depth tracker's worst pair)
_RGBD_KINDS = {'rgb8': _native.D3F_RGBD_COLOR_RGB8, 'grey8': _native.D3F_RGBD_COLOR_GREY8,
               'f32': _native.D3F_RGBD_COLOR_F32}


class RgbdPyramid(DepthPyramid):
    """A ``DepthPyramid`` with the intensity pyramid beside it (``rgbd_pyramid``): ``intensity`` f32 [F, pixels] has
    the layout of ``data`` (``intensity_level(l)`` is the view [F, H_l, W_l]).  ``data``, ``K`` and ``table`` are
    ``depth_pyramid``'s bit for bit, so every ``depth_*`` function takes this object as it is."""

    def __init__(self, data, K, H, W, levels, depth_diff, intensity):
        DepthPyramid.__init__(self, data, K, H, W, levels, depth_diff)
        self.intensity = intensity

    def intensity_level(self, l):
        h, w, off = (int(x) for x in self.table[l])
        return self.intensity[:, off:off + h * w].reshape(self.frames, h, w)


def _rgbd_color(color, shape, device_ok=False):
    """Host form of the colour frames of depth frames of ``shape`` [F,H,W]: (array, kind) with kind 'rgb8' (uint8
    [F,H,W,3]), 'grey8' (uint8 [F,H,W]) or 'f32' (f32 [F,H,W]; with ``device_ok`` a device f32 tensor stays one)."""
    if isinstance(color, torch.Tensor):
        if device_ok and color.is_cuda and color.dtype == torch.float32:
            c = color.contiguous()
        else:
            c = color.detach().cpu().numpy()
    else:
        c = np.asarray(color)
    if isinstance(c, torch.Tensor) or c.dtype == np.float32:
        kind = 'f32'
    elif c.dtype == np.uint8:
        kind = 'rgb8' if c.ndim == 4 else 'grey8'
    else:
        raise ValueError("color must be uint8 [F,H,W,3] (R, G, B), uint8 [F,H,W] or float32 [F,H,W], got %s"
                         % (c.dtype,))
    want = tuple(shape) + ((3,) if kind == 'rgb8' else ())
    if tuple(c.shape) != want:
        raise ValueError("color of shape %s for depth frames of shape %s: expected %s"
                         % (tuple(c.shape), tuple(shape), want))
    return (c if isinstance(c, torch.Tensor) else np.ascontiguousarray(c)), kind


def _rgbd_check_weight(photo_weight):
    w = float(photo_weight)
    if not 0.0 <= w <= float(np.finfo(np.float32).max):       # (a NaN fails; the kernels take it as f32)
        raise ValueError("photo_weight must be a finite number >= 0, got %r" % (photo_weight,))
    return w


def _rgbd_pyramid(host, device, depth, color, intrinsics, levels, depth_scale, depth_max, depth_diff):
    d = _tsdf_depth_array(depth, not host)
    c, kind = _rgbd_color(color, d.shape, device_ok=not host)
    base = _depth_pyramid(host, device, depth, intrinsics, levels, depth_scale, depth_max, depth_diff)
    tc = c if isinstance(c, torch.Tensor) else _on(device, c)[0]
    inten = torch.empty_like(base.data)
    L = _native.lib()
    args = (_p(tc), _RGBD_KINDS[kind], base.frames, base.H, base.W, base.levels, _p(inten))
    if host:
        _native.check(L.d3f_rgbd_pyramid_host(*args), "d3f_rgbd_pyramid_host")
    else:
        _native.check(L.d3f_rgbd_pyramid(*(args + (_stream(),))), "d3f_rgbd_pyramid")
    return RgbdPyramid(base.data, base.K, base.H, base.W, base.levels, base.depth_diff, inten)


def rgbd_pyramid(depth, color, intrinsics, levels=3, depth_scale=1000.0, depth_max=TSDF_DEPTH_MAX,
                 depth_diff=ODO_DEPTH_DIFF):
    """The depth and intensity pyramids of F frames on the device (d3f_depth_pyramid and d3f_rgbd_pyramid; the rule is
    csrc/rgbd_odometry.hpp): an ``RgbdPyramid`` whose ``data``, ``table`` and ``K`` are ``depth_pyramid``'s bit for
    bit, with ``.intensity`` f32 [F, pixels] in the same layout.  ``color``: uint8 [F,H,W,3] (R, G, B;
    I = ((0.299 R + 0.587 G) + 0.114 B) / 255 in f32), uint8 [F,H,W] (I = v / 255) or f32 [F,H,W] (as it is; a device
    tensor is taken where it is), H and W the depth's, registered to the depth pixel by pixel.  A coarser pixel is the
    f32 sum of its 2x2 block in raster order divided by 4; an odd last row or column is dropped.  Intensity has no
    validity: a non-finite f32 value propagates into the coarser pixels above it and is excluded where the tracker
    reads it.  Equal to the host twin and ``rgbd_pyramid_numpy`` bit for bit."""
    dev = _tsdf_device()
    with _region("rgbd_pyramid"):
        return _rgbd_pyramid(False, dev, depth, color, intrinsics, levels, depth_scale, depth_max, depth_diff)


def rgbd_pyramid_host(depth, color, intrinsics, levels=3, depth_scale=1000.0, depth_max=TSDF_DEPTH_MAX,
                      depth_diff=ODO_DEPTH_DIFF):
    """The host twin of ``rgbd_pyramid`` (d3f_depth_pyramid_host, d3f_rgbd_pyramid_host): CPU tensors, no GPU call."""
    return _rgbd_pyramid(True, torch.device("cpu"), depth, color, intrinsics, levels, depth_scale, depth_max,
                         depth_diff)


def rgbd_odometry_step(pyr, pairs, T, level, max_distance=ODO_MAX_DISTANCE, photo_weight=ODO_PHOTO_WEIGHT,
                       return_index=False):
    """ONE association of P frame pairs at ``level`` under ``T`` with both terms (d3f_rgbd_odometry_step): ``sums`` f64
    [P,31] on the device.  The first 29 are ``depth_odometry_step``'s, where sum J J^T and sum J r also hold the
    photometric rows ``photo_weight * [a x q, q]`` and ``photo_weight * r_I`` (n and sum d2 stay geometric); then
    n_photo and sum r_I^2 (unweighted).  The association, and with it the index of ``return_index=True``, is
    ``depth_odometry_step``'s.  An accepted pixel has a photometric row when the 2x2 bilinear footprint of its
    unrounded projection and the central differences at it lie inside the fixed image and every intensity read is
    finite.  ``photo_weight=0`` skips the term (n_photo = 0)."""
    _odo_checked_pyramid(pyr, "rgbd_odometry_step", RgbdPyramid, False)
    with _region("rgbd_odometry_step"):
        return _odo_step(False, pyr, pairs, T, level, max_distance, photo_weight, return_index)


def rgbd_odometry_step_host(pyr, pairs, T, level, max_distance=ODO_MAX_DISTANCE, photo_weight=ODO_PHOTO_WEIGHT,
                            return_index=False):
    """The host twin of ``rgbd_odometry_step`` (d3f_rgbd_odometry_step_host): the same rule pixel by pixel in raster
    order, CPU tensors, no GPU call."""
    return _odo_step(True, _odo_checked_pyramid(pyr, "rgbd_odometry_step_host", RgbdPyramid, True), pairs, T, level,
                     max_distance, photo_weight, return_index)


def _rgbd_frames(pyr_or_frames, intrinsics):
    if intrinsics is None:
        raise ValueError("(depth, color) frames need intrinsics")
    if not isinstance(pyr_or_frames, (tuple, list)) or len(pyr_or_frames) != 2:
        raise ValueError("expected an RgbdPyramid or the pair (depth, color) of frames")
    return pyr_or_frames


def rgbd_odometry(pyr_or_frames, pairs, T_init=None, iterations=ODO_ITERATIONS, max_distance=ODO_MAX_DISTANCE,
                  photo_weight=ODO_PHOTO_WEIGHT, return_information=False, intrinsics=None, depth_scale=1000.0,
                  depth_max=TSDF_DEPTH_MAX, depth_diff=ODO_DEPTH_DIFF):
    """Relative poses of P frame pairs from depth AND intensity, all pairs in one launch sequence (d3f_rgbd_odometry;
    the rule is csrc/rgbd_odometry.hpp): ``depth_odometry`` with a photometric row per pixel beside the point-to-plane
    row -- the hybrid objective of Park, Zhou, Koltun 2017 after Steinbruecker et al. 2011, what Open3D's
    ``compute_rgbd_odometry`` minimises.  The intensity residual ``r_I = I_b(projection of a) - I_a(pixel)`` constrains
    the three motions a view of one plane leaves free, so such a pair is tracked where ``depth_odometry`` reports
    ``ODO_ST_SINGULAR``.

    ``pyr_or_frames``: the ``RgbdPyramid`` of ``rgbd_pyramid``, or ``(depth, color)`` frames with ``intrinsics``.
    Everything else is ``depth_odometry``'s: pairs, T, iterations, ``max_distance``, the statuses (``ODO_ST_FEW`` by
    the geometric count, ``ODO_ST_SINGULAR`` by the combined system), count and rmse (geometric).  ``photo_weight``
    is a plain scale between the two residuals: intensity is in [0, 1], the geometric residual in metres, and the
    photometric row and residual are multiplied by it (its square weighs the squared term).  The default
    ``ODO_PHOTO_WEIGHT`` comes from profiles/rgbd_odometry_weight_sweep.txt.  ``photo_weight=0`` gives
    ``depth_odometry``'s results bit for bit.  The colour must be registered to the depth and keep a surface's
    brightness from frame to frame (no auto-exposure).

    Returns device tensors ``(T f64 [P,4,4], count int32 [P], rmse f64 [P], status int32 [P], n_photo int32 [P])``;
    ``return_information=True`` inserts f64 [P,6,6] = the combined sum J J^T of the final association (rotation first,
    fixed frame) before ``n_photo``, which is the number of photometric rows of that association.  A pair's result is
    bit-identical alone, in any batch, and from run to run."""
    if isinstance(pyr_or_frames, DepthPyramid):
        pyr = _odo_checked_pyramid(pyr_or_frames, "rgbd_odometry", RgbdPyramid, False)
    else:
        d, c = _rgbd_frames(pyr_or_frames, intrinsics)
        pyr = rgbd_pyramid(d, c, intrinsics, len(_odo_iterations(iterations)), depth_scale, depth_max, depth_diff)
    with _region("rgbd_odometry"):
        return _odometry(False, pyr, pairs, T_init, iterations, max_distance, photo_weight, return_information)


def rgbd_odometry_host(pyr_or_frames, pairs, T_init=None, iterations=ODO_ITERATIONS, max_distance=ODO_MAX_DISTANCE,
                       photo_weight=ODO_PHOTO_WEIGHT, return_information=False, intrinsics=None, depth_scale=1000.0,
                       depth_max=TSDF_DEPTH_MAX, depth_diff=ODO_DEPTH_DIFF):
    """The host twin of ``rgbd_odometry`` (d3f_rgbd_odometry_host): CPU tensors, no GPU call.  It sums in raster
    order, so T agrees with the device's to rounding (1e-6), not bit for bit."""
    if isinstance(pyr_or_frames, DepthPyramid):
        pyr = _odo_checked_pyramid(pyr_or_frames, "rgbd_odometry_host", RgbdPyramid, True)
    else:
        d, c = _rgbd_frames(pyr_or_frames, intrinsics)
        pyr = rgbd_pyramid_host(d, c, intrinsics, len(_odo_iterations(iterations)), depth_scale, depth_max, depth_diff)
    return _odometry(True, pyr, pairs, T_init, iterations, max_distance, photo_weight, return_information)


# ------------------------------------------------------------------------------------------- NumPy restatement
def rgbd_pyramid_numpy(depth, color, intrinsics, levels=3, depth_scale=1000.0, depth_max=TSDF_DEPTH_MAX,
                       depth_diff=ODO_DEPTH_DIFF):
    """The contract of ``rgbd_pyramid`` in NumPy: an ``RgbdPyramid`` of NumPy arrays, equal to the kernels' bit for bit
    (every f32 operation in the order of csrc/rgbd_odometry.hpp)."""
    f32 = np.float32
    base = depth_pyramid_numpy(depth, intrinsics, levels, depth_scale, depth_max, depth_diff)
    c, kind = _rgbd_color(color, (base.frames, base.H, base.W))
    with np.errstate(all='ignore'):
        if kind == 'rgb8':
            c = c.astype(f32)
            cur = ((f32(0.299) * c[..., 0] + f32(0.587) * c[..., 1]) + f32(0.114) * c[..., 2]) / f32(255.0)
        elif kind == 'grey8':
            cur = c.astype(f32) / f32(255.0)
        else:
            cur = c
        inten = np.zeros_like(base.data)
        for l in range(base.levels):
            h, w, off = (int(x) for x in base.table[l])
            inten[:, off:off + h * w] = cur.reshape(base.frames, -1)
            hn, wn = h >> 1, w >> 1
            blk = lambda dy, dx: cur[:, dy:2 * hn:2, dx:2 * wn:2]
            cur = (((blk(0, 0) + blk(0, 1)) + blk(1, 0)) + blk(1, 1)) / f32(4.0)
    return RgbdPyramid(base.data, base.K, base.H, base.W, base.levels, base.depth_diff, inten)


def _rgbd_numpy_pyramid(pyr):
    if not isinstance(pyr, RgbdPyramid):
        raise ValueError("expected an RgbdPyramid")
    if isinstance(pyr.data, np.ndarray):
        return pyr
    return RgbdPyramid(_host_array(pyr.data), _host_array(pyr.K), pyr.H, pyr.W, pyr.levels, pyr.depth_diff,
                       _host_array(pyr.intensity))


def _rgbd_photometric_numpy(index, a, IA, IB, Kb):
    """photometric() of csrc/rgbd_odometry.hpp for the accepted pixels of one association (``index`` int32 [H,W] and
    ``a`` f32 [3,m] of ``_odo_associate_numpy``): (has bool [m], r f32 [m], q f32 [3,m])."""
    f32 = np.float32
    h, w = IA.shape
    Ia = IA[index >= 0]
    m = Ia.shape[0]
    if m == 0 or h < 4 or w < 4:
        return np.zeros(m, dtype=bool), np.zeros(m, dtype=f32), np.zeros((3, m), dtype=f32)
    two = f32(2.0)
    px = (Kb[0] * a[0]) / a[2] + Kb[2]
    py = (Kb[1] * a[1]) / a[2] + Kb[3]
    x0f, y0f = np.floor(px), np.floor(py)
    has = (x0f >= 1) & (x0f <= f32(w - 3)) & (y0f >= 1) & (y0f <= f32(h - 3))
    x0 = np.where(has, x0f, 1).astype(np.int64)
    y0 = np.where(has, y0f, 1).astype(np.int64)
    wx, wy = px - x0f, py - y0f
    at = lambda dx, dy: IB[y0 + dy, x0 + dx]
    u0, u1 = at(0, -1), at(1, -1)
    m0, m1, m2, m3 = at(-1, 0), at(0, 0), at(1, 0), at(2, 0)
    n0, n1, n2, n3 = at(-1, 1), at(0, 1), at(1, 1), at(2, 1)
    d0, d1 = at(0, 2), at(1, 2)
    for x in (Ia, u0, u1, m0, m1, m2, m3, n0, n1, n2, n3, d0, d1):
        has &= np.isfinite(x)

    def bilinear(c00, c10, c01, c11):
        t = c00 + wx * (c10 - c00)
        b = c01 + wx * (c11 - c01)
        return t + wy * (b - t)

    Ib = bilinear(m1, m2, n1, n2)
    gx = bilinear((m2 - m0) / two, (m3 - m1) / two, (n2 - n0) / two, (n3 - n1) / two)
    gy = bilinear((n1 - u0) / two, (n2 - u1) / two, (d0 - m1) / two, (d1 - m2) / two)
    g0, g1 = gx * Kb[0], gy * Kb[1]
    q = np.stack([g0 / a[2], g1 / a[2], -((g0 * a[0] + g1 * a[1]) / (a[2] * a[2]))]).astype(f32)
    has &= np.isfinite(q).all(axis=0)
    return has, (Ib - Ia).astype(f32), q


def _rgbd_terms(a, q, r, w):
    """add_photometric() of csrc/rgbd_odometry.hpp: f64 [m,31], what every photometric row adds to the sums."""
    a, q, r = a.astype(np.float64), q.astype(np.float64), r.astype(np.float64)
    J = [w * (a[1] * q[2] - a[2] * q[1]), w * (a[2] * q[0] - a[0] * q[2]), w * (a[0] * q[1] - a[1] * q[0]),
         w * q[0], w * q[1], w * q[2]]
    rw = w * r
    zero = np.zeros_like(r)
    cols = [zero] + [J[i] * J[j] for i, j in _ODO_UPPER] + [J[i] * rw for i in range(6)] + [zero, np.ones_like(r), r * r]
    return np.stack(cols, axis=1) if r.size else np.zeros((0, RGBD_SUMS))


def _rgbd_pair_terms(pyr, level, a, b, t, md, w, normals=None):
    """(index int32 [H_l,W_l], terms f64 [m + m_photo, 31]) of one association of the pair (a, b): the geometric rows
    (zero in the last two columns), then the photometric rows, each in raster order."""
    index, av, geo = _odo_pair_terms(pyr, level, a, b, t, md, normals)
    geo = np.concatenate([geo, np.zeros((av.shape[1], 2))], axis=1)
    if w == 0.0:
        return index, geo
    inten = pyr.intensity_level(level)
    has, r, q = _rgbd_photometric_numpy(index, av, inten[a], inten[b], pyr.K[b, level])
    return index, np.concatenate([geo, _rgbd_terms(av[:, has], q[:, has], r[has], w)], axis=0)


def rgbd_odometry_step_numpy(pyr, pairs, T, level, max_distance=ODO_MAX_DISTANCE, photo_weight=ODO_PHOTO_WEIGHT,
                             return_index=False, return_terms=False):
    """The contract of ``rgbd_odometry_step`` in NumPy: ``sums`` f64 [P,31] (NumPy's own summation order: equal to the
    kernel's within the summation bound, not bit for bit) and, with ``return_index``, the index int32 [P,H_l,W_l],
    which is equal.  ``return_terms=True`` appends the list of the f64 [m_p + m_photo_p, 31] rows the sums are made
    of: the geometric terms, then the photometric ones."""
    pyr = _rgbd_numpy_pyramid(pyr)
    pr, t = _odo_pairs(pairs, T, "rgbd_odometry_step_numpy")
    level = _odo_check_level(level, pyr)
    w = float(np.float32(_rgbd_check_weight(photo_weight)))
    md = _odo_check_distance(max_distance)
    pair_terms = lambda a, b, tp: _rgbd_pair_terms(pyr, level, a, b, tp, md, w)
    return _odo_step_numpy(pyr, pr, t, level, RGBD_SUMS, pair_terms, return_index, return_terms)


def rgbd_odometry_numpy(pyr_or_frames, pairs, T_init=None, iterations=ODO_ITERATIONS, max_distance=ODO_MAX_DISTANCE,
                        photo_weight=ODO_PHOTO_WEIGHT, return_information=False, intrinsics=None, depth_scale=1000.0,
                        depth_max=TSDF_DEPTH_MAX, depth_diff=ODO_DEPTH_DIFF):
    """The contract of ``rgbd_odometry`` in NumPy: ``(T f64 [P,4,4], count int32 [P], rmse f64 [P], status int32 [P],
    [information f64 [P,6,6],] n_photo int32 [P])``; T agrees with the kernel's to rounding, not bit for bit."""
    it = _odo_iterations(iterations)
    if isinstance(pyr_or_frames, DepthPyramid):
        pyr = _rgbd_numpy_pyramid(pyr_or_frames)
        _odo_iterations(iterations, pyr.levels)
    else:
        d, c = _rgbd_frames(pyr_or_frames, intrinsics)
        pyr = rgbd_pyramid_numpy(d, c, intrinsics, len(it), depth_scale, depth_max, depth_diff)
    pr, t0 = _odo_pairs(pairs, T_init, "rgbd_odometry_numpy")
    md = _odo_check_distance(max_distance)
    w = float(np.float32(_rgbd_check_weight(photo_weight)))
    normals = {}
    sums_at = lambda p, level, t: _rgbd_pair_terms(pyr, level, int(pr[p, 0]), int(pr[p, 1]), t, md, w,
                                                   normals)[1].sum(axis=0)
    return _odo_march_numpy(pyr, pr, t0, it, sums_at, return_information, photo=True)


# ---------------------------------------------------------------------------------------------------------------
# guarded SGD step on flat buffers (trainer.py:104-111 + training_3DMatch.py:62-76)
# ---------------------------------------------------------------------------------------------------------------
def sgd_guarded_step(grad, params, momentum_buf, lr, momentum, weight_decay, state, hyper=None, pair_status=None):
    """In place: params/momentum_buf updated unless grad holds a non-finite value (then state[1] += 1).
    ``grad``: the gradient buffer, or a list of up to four of them (one per pair in flight on this GPU,
    train.PairLanes): the step then uses their sum (d3f_sgd_guarded_step_lanes).  ``hyper``: optional fp32[4] device tensor {lr, momentum, weight_decay, grad_scale} read by the kernel when it
    runs.  ``pair_status``: optional device int32[1], the status word of the pair the gradient came from: non-zero
    skips the update too (state[2] |= flags, state[3] += 1)."""
    lanes = list(grad) if isinstance(grad, (list, tuple)) else [grad]
    if not 1 <= len(lanes) <= 4:
        raise ValueError("1..4 gradient buffers, got %d" % len(lanes))
    grad = lanes[0]
    for t, name in [(g, "grad") for g in lanes] + [(params, "params"), (momentum_buf, "momentum_buf")]:
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == grad.numel()):
            raise ValueError("%s must be a contiguous fp32 device tensor of %d elements" % (name, grad.numel()))
    if not (state.is_cuda and state.dtype == torch.int32 and state.numel() >= 4):
        raise ValueError("state must be an int32[4] device tensor")
    if hyper is not None and not (hyper.is_cuda and hyper.dtype == torch.float32 and hyper.numel() == 4
                                  and hyper.is_contiguous()):
        raise ValueError("hyper must be a contiguous fp32[4] device tensor")
    with _region("sgd", (12 + 8 * len(lanes)) * grad.numel()):
        if len(lanes) == 1:
            _native.check(_native.lib().d3f_sgd_guarded_step(_p(grad), _p(params), _p(momentum_buf), grad.numel(),
                                                             float(lr), float(momentum), float(weight_decay),
                                                             _p(hyper) if hyper is not None else None, _p(state),
                                                             _p(pair_status), _stream()), "d3f_sgd_guarded_step")
        else:
            import ctypes
            ptrs = (ctypes.c_void_p * len(lanes))(*[g.data_ptr() for g in lanes])
            _native.check(_native.lib().d3f_sgd_guarded_step_lanes(
                ctypes.cast(ptrs, ctypes.c_void_p), len(lanes), _p(params), _p(momentum_buf), grad.numel(), float(lr),
                float(momentum), float(weight_decay), _p(hyper) if hyper is not None else None, _p(state),
                _p(pair_status), _stream()), "d3f_sgd_guarded_step_lanes")


def adam_guarded_step(grad, params, exp_avg, exp_avg_sq, step, hyper, state, pair_status=None):
    """In place, torch.optim.Adam's step (amsgrad off, L2 weight decay) on flat buffers unless a gradient holds a
    non-finite value or ``pair_status`` is set (then nothing changes but state[1] += 1; see sgd_guarded_step).
    ``grad``: one gradient buffer or a list of up to four (summed in order).  ``step``: device fp32[1], applied steps so
    far (advanced by an applied step).  ``hyper``: device fp64[6] {lr, beta1, beta2, eps, weight_decay, grad_scale},
    read when the kernels run."""
    lanes = list(grad) if isinstance(grad, (list, tuple)) else [grad]
    if not 1 <= len(lanes) <= 4:
        raise ValueError("1..4 gradient buffers, got %d" % len(lanes))
    n = lanes[0].numel()
    for t, name in [(g, "grad") for g in lanes] + [(params, "params"), (exp_avg, "exp_avg"),
                                                   (exp_avg_sq, "exp_avg_sq")]:
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n):
            raise ValueError("%s must be a contiguous fp32 device tensor of %d elements" % (name, n))
    if not (step.is_cuda and step.dtype == torch.float32 and step.numel() == 1):
        raise ValueError("step must be an fp32[1] device tensor")
    if not (hyper.is_cuda and hyper.dtype == torch.float64 and hyper.numel() == 6 and hyper.is_contiguous()):
        raise ValueError("hyper must be a contiguous fp64[6] device tensor")
    if not (state.is_cuda and state.dtype == torch.int32 and state.numel() >= 4):
        raise ValueError("state must be an int32[4] device tensor")
    import ctypes
    ptrs = (ctypes.c_void_p * len(lanes))(*[g.data_ptr() for g in lanes])
    with _region("adam", (24 + 8 * len(lanes)) * n):
        _native.check(_native.lib().d3f_adam_guarded_step(
            ctypes.cast(ptrs, ctypes.c_void_p), len(lanes), _p(params), _p(exp_avg), _p(exp_avg_sq), _p(step), n,
            _p(hyper), _p(state), _p(pair_status), _stream()), "d3f_adam_guarded_step")


def poison_gradient_if_status(grad, pair_status, state):
    """Data-parallel form of the pair-status gate (before the gradient exchange): see d3f_poison_gradient_if_status."""
    _native.check(_native.lib().d3f_poison_gradient_if_status(_p(grad), _p(pair_status), _p(state), _stream()),
                  "d3f_poison_gradient_if_status")
