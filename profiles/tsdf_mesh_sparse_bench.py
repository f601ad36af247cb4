"""Times the mesh straight from a sparse pool (ops.tsdf_mesh_sparse, csrc/tsdf_mesh_sparse.hip) on the fragment of
profiles/tsdf_bench.py -- 50 synthetic depth frames of 640 x 480, voxel 0.006 m, trunc 5 voxels -- fused once into a
sparse pool and once into the dense volume:

    python profiles/tsdf_mesh_sparse_bench.py            ->  profiles/tsdf_mesh_sparse_bench.txt

  * d3f_tsdf_sparse_mesh_count (count + two scans + starts), d3f_tsdf_sparse_mesh counted (emit) and uncounted (both)
    against d3f_tsdf_mesh on the dense volume and d3f_tsdf_sparse_extract on the same pool: device events on the stream
    around INNER back-to-back C-ABI calls on buffers made beforehand, the arms taking turns, REPEAT windows after WARMUP
    rounds; median, minimum and maximum of the time per call;
  * ops.tsdf_densify + ops.tsdf_mesh, the only route to a mesh of a pool before, against ops.tsdf_mesh_sparse: host clock
    around calls that end synchronised, after a warm-up;
  * the sparse mesh against the dense mesh of the same fragment: equal counts, and the same vertex rows (position and
    normal) bit for bit as a set;
  * the bytes the sparse mesh must move (ops.tsdf_mesh_sparse_bytes) over its time, as a share of the HBM copy rate
    measured in MI355X_MICROARCH.md;
  * the kernels' register, scratch and LDS figures as the compiler reports them, when hipcc is there.

Needs the GPU; there is no fallback."""
import datetime
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import tsdf_bench as TB  # noqa: E402  (puts the repository and tests/ on the path)
from tsdf_raycast_sparse_bench import kernel_resources  # noqa: E402
from d3feat_pytorch_amd import _native, ops  # noqa: E402
from d3feat_pytorch_amd.datasets import fragments as fr  # noqa: E402

REPEAT, WARMUP, INNER = 15, 3, 10
ROUTE_RUNS = 3


def timed_alternating(fns):
    """Milliseconds per call [len(fns), REPEAT]: device events around INNER calls of each of ``fns``, taken in turn,
    after WARMUP rounds."""
    for _ in range(WARMUP):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(REPEAT):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(INNER):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1) / INNER)
    return np.array(out)


def sorted_rows(v, n):
    rows = np.concatenate([v.cpu().numpy().view(np.uint32), n.cpu().numpy().view(np.uint32)], axis=1)
    return rows[np.lexsort(rows.T[::-1])]


def main():
    assert torch.cuda.is_available(), "tsdf_mesh_sparse_bench needs the GPU"
    dev = torch.device('cuda')
    L, p, stream = _native.lib(), ops._p, torch.cuda.current_stream().cuda_stream
    out = []

    def say(s=""):
        print(s, flush=True)
        out.append(s)

    F, voxel = TB.FRAMES, TB.VOXEL
    trunc = 5 * voxel
    say("Meshing the fragment of tsdf_bench.py straight from its sparse pool: %d frames of %d x %d, voxel %g m, trunc %g m"
        % (F, TB.WIDTH, TB.HEIGHT, voxel, trunc))
    say("device: %s (%s)   date: %s" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName,
                                        datetime.date.today().isoformat()))
    say()
    depth, poses = TB.make_sequence()
    M = np.stack([fr.rigid_inverse(P) @ poses[0] for P in poses])
    C = np.stack([fr.rigid_inverse(poses[0]) @ P for P in poses])
    origin, dims = fr.place_volumes(ops.tsdf_bounds(depth, [0, F], TB.K, C).cpu().numpy(), voxel)
    sv = ops.tsdf_allocate(depth, [0, F], TB.K, C, origin, dims, voxel, trunc)
    Ds, ws = ops.tsdf_integrate_sparse(depth, [0, F], TB.K, M, sv, trunc)
    D, w, tvs = ops.tsdf_integrate(depth, [0, F], TB.K, M, origin, dims, voxel, trunc)
    total, B, lattice = int(D.numel()), sv.bricks, int(sv.lattice_start[-1])
    sparse_bytes = ops.tsdf_sparse_bytes(sv)
    say("volume: %d x %d x %d = %d voxels; %d of %d bricks allocated (%.1f %%)"
        % (dims[0, 0], dims[0, 1], dims[0, 2], total, B, lattice, 100.0 * B / lattice))
    say("bytes: dense D and w %.3f GB; sparse pool and tables %.1f MB (%.1f %% of the dense bytes)"
        % (8e-9 * total, 1e-6 * sparse_bytes, 100.0 * sparse_bytes / (8.0 * total)))

    # sizes and results through the public operators
    sm = ops.tsdf_mesh_sparse(Ds, ws, sv)
    dm = ops.tsdf_mesh(D, w, tvs, origin, dims, voxel)
    points, point_start = ops.tsdf_extract_sparse(Ds, ws, sv)
    nv, nf, npts = int(sm[0].shape[0]), int(sm[2].shape[0]), int(points.shape[0])
    same_counts = (nv, nf) == (int(dm[0].shape[0]), int(dm[2].shape[0]))
    same_rows = same_counts and np.array_equal(sorted_rows(sm[0], sm[1]), sorted_rows(dm[0], dm[1]))
    say("mesh: %d vertices, %d triangles from the pool; %d vertices, %d triangles from the dense volume; the same vertex "
        "rows (position and normal) bit for bit as a set: %s;   cloud: %d points"
        % (nv, nf, dm[0].shape[0], dm[2].shape[0], same_rows, npts))
    assert same_counts and same_rows, "the sparse mesh is not the dense mesh"

    o, n, vx, _, _ = ops._tsdf_volumes(origin, dims, voxel, 1)
    to, tn, tvx = ops._on(dev, o, n, vx)
    tls, bs, bi, bc, _, _, _ = ops._sparse_tables(sv, dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    vertices, normals, faces, vertex_start, face_start = sm
    dvertices, dnormals, dfaces, dvertex_start, dface_start = dm
    sm_bytes = L.d3f_tsdf_sparse_mesh_ws_bytes(B)
    sm_ws = torch.empty(sm_bytes, dtype=torch.uint8, device=dev)
    dm_bytes = L.d3f_tsdf_mesh_ws_bytes(total)
    dm_ws = torch.empty(dm_bytes, dtype=torch.uint8, device=dev)
    ex_bytes = L.d3f_tsdf_sparse_extract_ws_bytes(B)
    ex_ws = torch.empty(ex_bytes, dtype=torch.uint8, device=dev)
    pool = (p(Ds), p(ws), p(tls), p(bs), p(bi), p(bc))

    def sparse_count():
        _native.check(L.d3f_tsdf_sparse_mesh_count(*pool, p(tn), 1, lattice, B, 1.0, p(vertex_start), p(face_start),
                                                   p(sm_ws), sm_bytes, stream), "d3f_tsdf_sparse_mesh_count")

    def sparse_mesh(counted):
        _native.check(L.d3f_tsdf_sparse_mesh(*pool, p(to), p(tn), p(tvx), 1, lattice, B, 1.0, counted, nv, nf,
                                             p(vertices), p(normals), p(faces), p(vertex_start), p(face_start),
                                             p(status), p(sm_ws), sm_bytes, stream), "d3f_tsdf_sparse_mesh")

    def dense_mesh():
        _native.check(L.d3f_tsdf_mesh(p(D), p(w), p(tvs), p(to), p(tn), p(tvx), 1, total, 1.0, 0, nv, nf, p(dvertices),
                                      p(dnormals), p(dfaces), p(dvertex_start), p(dface_start), p(status), p(dm_ws),
                                      dm_bytes, stream), "d3f_tsdf_mesh")

    def sparse_extract():
        _native.check(L.d3f_tsdf_sparse_extract(*pool, p(to), p(tn), p(tvx), 1, lattice, B, 1.0, 0, npts, p(points),
                                                p(point_start), p(status), p(ex_ws), ex_bytes, stream),
                      "d3f_tsdf_sparse_extract")

    ms_c, = timed_alternating([sparse_count])                              # the counts stay in the workspace
    ms_e, = timed_alternating([lambda: sparse_mesh(1)])
    ms_s, ms_d, ms_x = timed_alternating([lambda: sparse_mesh(0), dense_mesh, sparse_extract])
    assert int(status.item()) == 0 and int(vertex_start[1]) == nv and int(face_start[1]) == nf

    def line(name, ms):
        return "  %-58s median %8.3f ms   min %8.3f   max %8.3f" % (name, np.median(ms), ms.min(), ms.max())
    say()
    say("time per call: device events around %d back-to-back calls, %d windows after %d warm-up rounds, the arms of a "
        "group taking turns" % (INNER, REPEAT, WARMUP))
    say(line("d3f_tsdf_sparse_mesh_count (count + 2 scans + starts)", ms_c))
    say(line("d3f_tsdf_sparse_mesh, counted (emit)", ms_e))
    say(line("d3f_tsdf_sparse_mesh (count + scans + emit)", ms_s))
    say(line("d3f_tsdf_mesh on the dense volume (count + scans + emit)", ms_d))
    say(line("d3f_tsdf_sparse_extract on the pool (count + scan + emit)", ms_x))
    t_s, t_d, t_x = float(np.median(ms_s)), float(np.median(ms_d)), float(np.median(ms_x))
    say("  sparse mesh / dense mesh = %.3f (%s); sparse mesh / sparse extract = %.2f"
        % (t_s / t_d, "faster than the dense mesh" if ms_s.max() < ms_d.min() else
           "NOT faster than the dense mesh: a finding" if t_s >= t_d else "faster in the median, the ranges overlap",
           t_s / t_x))
    moved = ops.tsdf_mesh_sparse_bytes(B, nv, nf, lattice)
    say("  tsdf_mesh_sparse: %.0f bytes (tsdf_mesh_sparse_bytes) in %.3f ms = %.1f GB/s = %.1f %% of the %.2f TB/s HBM copy "
        "rate (the pool fits the 256 MB Infinity Cache, so this is no HBM figure: it says how far the pass is from a copy)"
        % (moved, t_s, moved / t_s * 1e-6, 100 * moved / t_s * 1e-9 / TB.HBM_COPY_TBS, TB.HBM_COPY_TBS))

    # ------------------------------------------------------------------------- the only route there was before
    del D, w, dm, dvertices, dnormals, dfaces, dm_ws
    torch.cuda.empty_cache()

    def old_route():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        Dd, wd, vs = ops.tsdf_densify(Ds, ws, sv)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        mesh = ops.tsdf_mesh(Dd, wd, vs, origin, dims, voxel)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), 1e3 * (t1 - t0), mesh[3][1].item()

    def new_route():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mesh = ops.tsdf_mesh_sparse(Ds, ws, sv)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), mesh[3][1].item()

    old_route(), new_route()
    t_old, t_den, t_new = [], [], []
    for _ in range(ROUTE_RUNS):
        a, d, count_old = old_route()
        b, count_new = new_route()
        assert count_old == count_new == nv
        t_old.append(a)
        t_den.append(d)
        t_new.append(b)
    say()
    say("the route to a mesh of a pool before, ops.tsdf_densify + ops.tsdf_mesh, against ops.tsdf_mesh_sparse (allocation of "
        "the result and the one read-back included); host clock around calls that end synchronised, medians of %d (range) "
        "after a warm-up:" % ROUTE_RUNS)
    say("  densify + mesh %9.2f ms (%.2f..%.2f), of which densify %.2f ms;   tsdf_mesh_sparse %7.3f ms (%.3f..%.3f);   %.0f x"
        % (np.median(t_old), min(t_old), max(t_old), np.median(t_den), np.median(t_new), min(t_new), max(t_new),
           np.median(t_old) / np.median(t_new)))

    say()
    for kernel in ("sparse_mesh_count_kernel", "sparse_mesh_emit_kernel"):
        res = kernel_resources(kernel, "tsdf_mesh_sparse.hip")
        say("%s as compiled for gfx950: %s" % (kernel, ", ".join("%s %d" % kv for kv in res.items()) if res else
                                                "not measured (no hipcc here)"))
    text = "\n".join(out) + "\n"
    dest = os.environ.get("TSDF_MESH_SPARSE_BENCH_OUT", os.path.join(HERE, "tsdf_mesh_sparse_bench.txt"))
    with open(dest, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
