"""CPU: ray-casting sparse TSDF volumes (csrc/tsdf_raycast_sparse.hpp) -- the host twin against the dense host twin on
the densified pool, which is the rule; ``tsdf_integrate_sparse(..., into=)`` against one call over all frames;
``tsdf_extend`` against one allocation over all frames; ``track_sequence(model=dict(sparse=True))`` on the room."""
import os
import re

import numpy as np
import pytest
import torch

import d3feat_pytorch_amd  # noqa: F401
from d3feat_pytorch_amd import _native, ops
from d3feat_pytorch_amd.datasets import fragments as fr
import odometry_cases as OC
import raycast_cases as RC
import raycast_sparse_cases as C
import tsdf_scene as S
import tsdf_sparse_cases as SC
from tsdf_entry_cases import REMOVED_ENTRIES

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
same_bits, host = SC.same_bits, SC.host


@pytest.fixture(scope="module")
def oracles():
    """name -> (depth, normals) of the dense host twin on the densified pool, computed once."""
    return {name: C.oracle(case) for name, case in C.cases().items()}


# ------------------------------------------------------------------------------------------------------- ray-cast
@pytest.mark.parametrize("name", sorted(C.cases()))
def test_twin_equals_the_dense_twin_on_the_densified_pool(name, oracles):
    """The rule: bit for bit, depth and normals, with the brick skip and the box clip on and off."""
    case = C.cases()[name]
    depth, nrm = oracles[name]
    R = len(case['view_volume'])
    for skip in (True, False):
        for clip in (True, False):
            d, n = ops.tsdf_raycast_sparse_host(**case, normals=True, skip=skip, clip=clip)
            assert d.shape == (R, case['height'], case['width']) and n.shape == d.shape + (3,)
            assert same_bits(d, depth), (name, skip, clip)
            assert same_bits(n, nrm), (name, skip, clip)
    assert same_bits(ops.tsdf_raycast_sparse_host(**case), depth)          # without the normal output
    if name in C.ALL_ZERO:
        assert not depth.any() and not nrm.any()
    elif name in C.HITS:
        assert (depth > 0).any() and nrm.any()
    if name in C.NO_BRICKS:
        assert case['sv'].bricks == 0


def test_the_cases_are_what_they_say():
    cases = C.cases()
    sv = cases['room']['sv']
    assert (sv.bricks, int(sv.lattice_start[-1])) == (420, 972)
    assert cases['small_partly_outside']['sv'].bricks == 6 and int(cases['small_partly_outside']['sv'].lattice_start[-1]) == 48
    assert cases['two_volumes']['sv'].volumes == 2 and cases['two_volumes']['view_volume'] == [1, 0, 1, 0]
    assert host(cases['two_volumes']['sv'].brick_start)[1] > 0          # the second volume's rows do not start at 0
    # min_weight = 0: absent bricks count as a valid D = 0, so the image differs from that of min_weight = 1
    zero = ops.tsdf_raycast_sparse_host(**cases['min_weight_0'])
    one = ops.tsdf_raycast_sparse_host(**dict(cases['min_weight_0'], min_weight=1.0))
    assert not same_bits(zero, one)


def test_restatement_and_render_views(oracles):
    for name in ('room', 'small_dims_13x9x7', 'two_volumes', 'small_zero_frames'):
        case = C.cases()[name]
        d, n = ops.tsdf_raycast_sparse_numpy(**case, normals=True)
        assert same_bits(d, oracles[name][0]) and same_bits(n, oracles[name][1]), name
    case = C.cases()['two_volumes']
    d = fr.render_views(case['D'], case['w'], None, None, None, None, case['trunc'], S.K, case['camera_to_volume'],
                        S.H, S.W, view_volume=case['view_volume'], device='cpu', sv=case['sv'], skip=False)
    assert same_bits(d, oracles['two_volumes'][0])


@pytest.mark.parametrize("voxel,trunc,bricks", [(0.02, 0.08, (420, 972)), (0.01, 0.05, (1551, 6647))])
def test_sparse_equals_the_dense_integrated_volume_on_the_room(voxel, trunc, bricks):
    """NOT a property of the rule, which only promises the render of the densified pool: for THESE inputs the voxels
    the pool lacks are never needed by a ray (free space before the last positive sample, unseen space behind the
    crossing), so the render also equals that of the densely integrated volume bit for bit."""
    pool, dense = C.room_pool(voxel, trunc), C.room_dense(voxel, trunc)
    assert (pool['sv'].bricks, int(pool['sv'].lattice_start[-1])) == bricks
    poses = RC.room_view_poses() + ([C.inside_pose()] if voxel == 0.01 else [])
    views = dict(intrinsics=S.K, camera_to_volume=RC.to_volume(poses), height=S.H, width=S.W,
                 view_volume=[0] * len(poses), normals=True)
    sd, sn = ops.tsdf_raycast_sparse_host(**pool, **views)
    dd, dn = ops.tsdf_raycast_host(**dense, **views)
    assert same_bits(sd, dd) and same_bits(sn, dn) and (host(sd) > 0).mean() > 0.5


def test_raycast_arguments_are_checked():
    case = C.cases()['room']
    for bad in (dict(D=case['D'][:-1]), dict(view_volume=[0, 0, 0, 1]), dict(camera_to_volume=np.zeros((2, 4, 4))),
                dict(step=0.0), dict(depth_max=0.05), dict(height=0)):
        with pytest.raises(ValueError):
            ops.tsdf_raycast_sparse_host(**dict(case, **bad))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            ops.tsdf_raycast_sparse(**case)                                      # no fall-back to the CPU
    empty = ops.tsdf_raycast_sparse_host(**C.cases()['no_views'], normals=True)
    assert empty[0].shape == (0, S.H, S.W) and empty[1].shape == (0, S.H, S.W, 3)


# ---------------------------------------------------------------------------------------------------------- into=
def whole_pool(args):
    sv = ops.tsdf_allocate_host(**SC.allocate_args(args))
    D, w = ops.tsdf_integrate_sparse_host(**SC.sparse_args(args, sv))
    return sv, D, w


@pytest.mark.parametrize("name", C.INTO_CASES)
def test_into_equals_one_call(name):
    """For fixed tables the frames before k and then the frames from k on ``into`` the result give the pool of one call
    bit for bit, split after every volume's first frame and before its last; in place; host twin and NumPy."""
    args = C.batch_args(name)
    sv, D, w = whole_pool(args)
    assert sv.bricks > 0
    for k in (1, -1):
        head, tail = C.split_frames(args, k)
        Dh, wh = ops.tsdf_integrate_sparse_host(**SC.sparse_args(head, sv))
        ptr = (Dh.data_ptr(), wh.data_ptr())
        out = ops.tsdf_integrate_sparse_host(**SC.sparse_args(tail, sv), into=(Dh, wh))
        assert out[0] is Dh and out[1] is wh and (Dh.data_ptr(), wh.data_ptr()) == ptr
        assert same_bits(Dh, D) and same_bits(wh, w), (name, k)
        Dn, wn = ops.tsdf_sparse_numpy(**SC.sparse_args(head, sv))
        out = ops.tsdf_sparse_numpy(**SC.sparse_args(tail, sv), into=(Dn, wn))
        assert out[0] is Dn and out[1] is wn
        assert same_bits(Dn, D) and same_bits(wn, w), (name, k)


def test_into_leaves_a_volume_without_a_frame_alone_and_checks_its_arguments():
    args = C.batch_args('room')                                           # two volumes of six frames
    sv, D, w = whole_pool(args)
    bs = host(sv.brick_start)
    only_second = dict(args, depth=args['depth'][6:8], frame_start=[0, 0, 2], volume_to_camera=args['volume_to_camera'][6:8])
    for integrate, pool in ((ops.tsdf_integrate_sparse_host, (D.clone(), w.clone())),
                            (ops.tsdf_sparse_numpy, (D.numpy().copy(), w.numpy().copy()))):
        integrate(**SC.sparse_args(only_second, sv), into=pool)
        assert same_bits(host(pool[0])[:bs[1]], host(D)[:bs[1]]) and same_bits(host(pool[1])[:bs[1]], host(w)[:bs[1]])
        assert not same_bits(host(pool[1])[bs[1]:], host(w)[bs[1]:])
        assert host(pool[1]).max() == 8.0
    # without into the function returns what it did: the pool of a fresh call, whatever the tensors held
    again = ops.tsdf_integrate_sparse_host(**SC.sparse_args(args, sv))
    assert same_bits(again[0], D) and same_bits(again[1], w)
    for bad in ((D, w[:-1]), (D.double(), w), (D.numpy(), w.numpy()), (D,), D):
        with pytest.raises(ValueError):
            ops.tsdf_integrate_sparse_host(**SC.sparse_args(args, sv), into=bad)
    with pytest.raises(ValueError):
        ops.tsdf_sparse_numpy(**SC.sparse_args(args, sv), into=(D, w))           # tensors where arrays are due


# ---------------------------------------------------------------------------------------------------- tsdf_extend
@pytest.mark.parametrize("name", C.INTO_CASES)
def test_extend_equals_one_allocation(name):
    """Allocate from the frames before k, extend with the rest: the tables of one allocation over all frames, array
    for array; old rows at their new place bit for bit, new rows zero; host twin equals NumPy."""
    args = C.batch_args(name)
    whole = ops.tsdf_allocate_host(**SC.allocate_args(args))
    for k in (1, -1):
        head, tail = C.split_frames(args, k)
        sv = ops.tsdf_allocate_host(**SC.allocate_args(head))
        D, w = ops.tsdf_integrate_sparse_host(**SC.sparse_args(head, sv))
        sv2, D2, w2 = ops.tsdf_extend_host(sv, D, w, **C.extend_args(tail))
        assert SC.same_tables(sv2, whole), (name, k)
        assert D2.shape == (whole.bricks, 512) and w2.shape == D2.shape and D2.dtype == torch.float32
        at = C.old_rows_in_new(sv, sv2)
        assert same_bits(host(D2)[at], D) and same_bits(host(w2)[at], w)
        fresh = np.setdiff1d(np.arange(sv2.bricks), at)
        assert not host(D2)[fresh].any() and not host(w2)[fresh].any()
        if name == 'room':
            assert fresh.size > 0                                          # later frames do reach new bricks
        svn, Dn, wn = ops.tsdf_extend_numpy(ops.tsdf_allocate_numpy(**SC.allocate_args(head)), D.numpy(), w.numpy(),
                                            **C.extend_args(tail))
        assert SC.same_tables(svn, sv2) and same_bits(Dn, D2) and same_bits(wn, w2)
        # frames that flag nothing new: equal tables, an equal pool
        sv3, D3, w3 = ops.tsdf_extend_host(sv2, D2, w2, **C.extend_args(head))
        assert SC.same_tables(sv3, sv2) and same_bits(D3, D2) and same_bits(w3, w2)


@pytest.mark.parametrize("name", ['zero_frames', 'behind_camera'])
def test_extend_without_bricks(name):
    """B = 0 before and B = 0 after; and B = 0 before, bricks after."""
    args = S.small_cases()[name]
    sv = ops.tsdf_allocate_host(**SC.allocate_args(args))
    D, w = ops.tsdf_integrate_sparse_host(**SC.sparse_args(args, sv))
    assert sv.bricks == 0
    for extend, tables in ((ops.tsdf_extend_host, sv), (ops.tsdf_extend_numpy, ops.tsdf_allocate_numpy(
            **SC.allocate_args(args)))):
        sv2, D2, w2 = extend(tables, host(D), host(w), **C.extend_args(args))
        assert sv2.bricks == 0 and tuple(D2.shape) == (0, 512) and tuple(w2.shape) == (0, 512)
        assert SC.same_tables(sv2, tables)
    if name == 'zero_frames':
        seen = S.small_cases()['dims_13x9x7']
        sv2, D2, w2 = ops.tsdf_extend_host(sv, D, w, **C.extend_args(seen))
        assert SC.same_tables(sv2, ops.tsdf_allocate_host(**SC.allocate_args(seen))) and not host(D2).any()
    with pytest.raises(ValueError):
        ops.tsdf_extend_host(sv, D, w, **dict(C.extend_args(args), frame_start=[0, 1, 2]))    # two volumes for one


# ------------------------------------------------------------------------------------------------------ tracking
def frame_11_error(tracked):
    return OC.pose_error(tracked[11], OC.relative(S.sequence()[2], 11, 0))


# What the sparse model pass may lose against the dense one at frame 11, in degrees and millimetres.  Measured with the
# NumPy restatements on the room (two fragments of six frames, voxel 0.02, trunc 0.1): see the docstring below.  The
# two passes differ only where a brick was allocated late, so the slack covers that difference with head-room for f32
# reordering between the restatement and the kernels (1e-6 in a pose entry: 1e-4 deg, 1e-3 mm) and no more.
SLACK_DEG, SLACK_MM = 1e-4, 1e-3


@pytest.mark.parametrize("label", ["clean", "noisy"])
def test_track_sequence_against_a_sparse_model(label):
    """Two fragments of six frames at voxel 0.02 (trunc 0.1): every pair inside a fragment is tracked against the
    sparse model, and frame 11 is no farther from the analytic pose than with the dense model pass on the same input,
    run here by the existing code, plus the slack above.  Measured with the NumPy restatements (deg / mm at frame 11,
    dense model = sparse model to the digits shown):
        clean  voxel 0.02: 0.3950 / 4.8607 (6 per fragment), 0.2332 / 3.3135 (12)   voxel 0.01: 0.0678 / 0.8300, 0.0774 / 1.4769
        noisy  voxel 0.02: 0.3256 / 4.1549 (6 per fragment), 0.2622 / 4.3017 (12)   voxel 0.01: 0.4398 / 3.1188, 0.2064 / 2.5551
    On this sequence no ray needs a voxel whose brick arrived late, so the late bricks' missing free-space votes do not
    show; the slack is the f32 head-room alone."""
    depth = S.sequence()[0] if label == "clean" else RC.noisy_depth()
    model = dict(frames_per_fragment=6, voxel=0.02)
    dense = fr.track_sequence(depth, S.K, device='cpu', model=model)
    sparse = fr.track_sequence(depth, S.K, device='cpu', model=dict(model, sparse=True))
    assert sparse[2].tolist() == [0] * 5 + [-1] + [0] * 5 and sparse[1].tolist() == [0] * 11
    assert sparse[2].dtype == np.int32 and np.array_equal(sparse[0][0], np.eye(4))
    de, sp = frame_11_error(dense[0]), frame_11_error(sparse[0])
    print("%s, voxel 0.02: dense model %.4f deg, %.4f mm; sparse model %.4f deg, %.4f mm" % ((label,) + de + sp))
    assert sp[0] <= de[0] + SLACK_DEG and sp[1] <= de[1] + SLACK_MM


def test_a_sparse_model_fits_where_the_dense_one_does_not():
    """The room's model at voxel 0.01 (180 x 136 x 131 voxels: 25.6 MB dense, about 7 MB of bricks): a ``max_bytes``
    between the two raises for the dense model before anything runs, and the sparse one tracks."""
    depth, K, _ = S.sequence()
    model = dict(frames_per_fragment=4, voxel=0.01, max_bytes=12 << 20)
    with pytest.raises(ValueError):
        fr.track_sequence(depth[:4], K, device='cpu', model=model)
    tracked, status, model_status = fr.track_sequence(depth[:4], K, device='cpu', model=dict(model, sparse=True))
    assert model_status.tolist() == [0, 0, 0] and status.tolist() == [0, 0, 0]
    with pytest.raises(ValueError):                                              # and a group that outgrows it raises
        fr.track_sequence(depth[:4], K, device='cpu', model=dict(model, sparse=True, max_bytes=3 << 20))


# ----------------------------------------------------------------------------------------------------------- ABI
def test_the_new_entries_of_the_header_are_bound():
    src = open(os.path.join(REPO, "include", "d3feat_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _native.lib()
    for name in ("d3f_tsdf_raycast_sparse", "d3f_tsdf_raycast_sparse_host", "d3f_tsdf_sparse_integrate",
                 "d3f_tsdf_sparse_integrate_host"):
        assert re.search(r"\b%s\s*\(" % name, src) and name in _native.SIGNATURES and hasattr(lib, name)
    assert len(REMOVED_ENTRIES) == 16                      # folded into the entries above: `channels` and `into`
    for name in REMOVED_ENTRIES:
        assert not re.search(r"\b%s\s*\(" % name, src) and name not in _native.SIGNATURES and not hasattr(lib, name)
    assert fr.DEFAULT_MODEL['sparse'] is False
