"""CPU: the entry points of the training loss's four stages (select + normalise, the detector's rows form, circle and
contrastive loss) reject null or inconsistent arguments on the host (D3F_EINVAL, or D3F_EWORKSPACE for a short
workspace) before any launch -- no device is touched.  The addresses below are never read."""
import os
import subprocess
import sys

from d3feat_pytorch_amd import _native

EINVAL, EWORKSPACE = -1, -2
A = 0x10000        # a non-null "device address": the checks only compare it with NULL
STACKED = dict(len=A, B=6, group=2, pairs=3, pair_len=A)    # three stacked pairs, their clouds the normaliser groups


def _fwd(**kw):
    a = dict(feat=A, N=600, C=32, idx=A, H=40, fmax=A, training=1, width=None, len=None, B=0, group=0, idx_a=A, idx_p=A,
             stride=2, M=16, pairs=1, p_offset=None, pair_len=None, sa=A, sp=A, aux=A)
    a.update(kw)
    return _native.lib().d3f_detection_rows_forward(
        a['feat'], a['N'], a['C'], a['idx'], a['H'], a['fmax'], a['training'], a['width'], a['len'], a['B'], a['group'],
        a['idx_a'], a['idx_p'], a['stride'], a['M'], a['pairs'], a['p_offset'], a['pair_len'], a['sa'], a['sp'], a['aux'],
        None)


def _bwd(**kw):
    a = dict(feat=A, N=600, C=32, idx=A, H=40, fmax=A, len=None, B=0, group=0, idx_a=A, idx_p=A, stride=2, M=16, pairs=1,
             p_offset=None, pair_len=None, aux=A, g_sa=A, g_sp=A, grad_x=A, ws=A, ws_bytes=1 << 20)
    a.update(kw)
    return _native.lib().d3f_detection_rows_backward(
        a['feat'], a['N'], a['C'], a['idx'], a['H'], a['fmax'], a['len'], a['B'], a['group'], a['idx_a'], a['idx_p'],
        a['stride'], a['M'], a['pairs'], a['p_offset'], a['pair_len'], a['aux'], a['g_sa'], a['g_sp'], a['grad_x'],
        a['ws'], a['ws_bytes'], None)


def _select_fwd(**kw):
    a = dict(x=A, scores=A, N=600, C=32, idx_a=A, idx_p=A, stride=2, M=16, pairs=1, p_offset=None, pair_len=None,
             out_a=A, out_p=A, sa=A, sp=A)
    a.update(kw)
    return _native.lib().d3f_select_normalize_forward(
        a['x'], a['scores'], a['N'], a['C'], a['idx_a'], a['idx_p'], a['stride'], a['M'], a['pairs'], a['p_offset'],
        a['pair_len'], a['out_a'], a['out_p'], a['sa'], a['sp'], None)


def _select_bwd(**kw):
    a = dict(x=A, N=600, C=32, idx_a=A, idx_p=A, stride=2, M=16, pairs=1, p_offset=None, pair_len=None, g_a=A, g_p=A,
             g_sa=None, g_sp=None, grad_x=A, grad_scores=None)
    a.update(kw)
    return _native.lib().d3f_select_normalize_backward(
        a['x'], a['N'], a['C'], a['idx_a'], a['idx_p'], a['stride'], a['M'], a['pairs'], a['p_offset'], a['pair_len'],
        a['g_a'], a['g_p'], a['g_sa'], a['g_sp'], a['grad_x'], a['grad_scores'], None)


def _circle_fwd(**kw):
    a = dict(M=16, C=32, pairs=1, w=(1.0, 1.0), out_total=None)
    a.update(kw)
    return _native.lib().d3f_circle_det_loss_forward(A, A, a['M'], a['C'], a['pairs'], A, A, A, 10.0, 0.1, 0.1, 1.4,
                                                     a['w'][0], a['w'][1], A, A, A, A, a['out_total'], A, None)


def _circle_bwd(**kw):
    a = dict(M=16, C=32, pairs=1, w=(1.0, 1.0), ws=A, ws_bytes=1 << 30)
    a.update(kw)
    return _native.lib().d3f_circle_det_loss_backward(A, A, a['M'], a['C'], a['pairs'], A, A, A, 10.0, 0.1, 0.1, 1.4,
                                                      a['w'][0], a['w'][1], A, A, A, A, A, A, A, A, a['ws'],
                                                      a['ws_bytes'], None)


def _contrastive_fwd(**kw):
    a = dict(M=16, C=32, pairs=1, anchor=A, out_total=None)
    a.update(kw)
    return _native.lib().d3f_contrastive_det_loss_forward(a['anchor'], A, a['M'], a['C'], a['pairs'], A, A, A, 0.1, 0.1,
                                                          1.4, 1.0, 1.0, A, A, A, A, a['out_total'], A, None)


def _contrastive_bwd(**kw):
    a = dict(M=16, C=32, pairs=1, stats=A)
    a.update(kw)
    return _native.lib().d3f_contrastive_det_loss_backward(A, A, a['M'], a['C'], a['pairs'], A, A, 0.1, 1.4, 1.0, 1.0,
                                                           a['stats'], A, A, A, A, A, A, None)


ROWS_STAGES = (_select_fwd, _select_bwd, _fwd, _bwd)
LOSS_STAGES = (_circle_fwd, _circle_bwd, _contrastive_fwd, _contrastive_bwd)


def test_domain_and_workspace_are_host_computations():
    lib = _native.lib()
    assert [lib.d3f_detection_rows_supported(c, 40) for c in (16, 32, 64, 48, 8, 128)] == [1, 1, 1, 0, 0, 0]
    assert [lib.d3f_detection_rows_supported(32, h) for h in (1, 64, 65, 0)] == [1, 1, 0, 0]
    small, large = lib.d3f_detection_rows_ws_bytes(32), lib.d3f_detection_rows_ws_bytes(768)
    assert small >= 8 * 32 and large >= small + 8 * (768 - 32)
    assert lib.d3f_detection_rows_ws_bytes(0) > 0


def test_forward_entries_reject_bad_arguments_on_the_host():
    for bad in (dict(feat=None), dict(idx=None), dict(fmax=None), dict(idx_a=None), dict(idx_p=None), dict(sa=None),
                dict(sp=None), dict(N=0), dict(M=0), dict(stride=0), dict(C=48), dict(C=0), dict(H=65), dict(H=0),
                dict(training=0),                      # aux is a training-mode output
                dict(len=A, B=0, group=2), dict(len=A, B=65, group=2), dict(len=A, B=2, group=-1)):
        assert _fwd(**bad) == EINVAL, bad
    # the stacked form: the correspondence table (both columns), the pairs' lengths, the pair count, B = 2 pairs
    for bad in (dict(idx_a=None, idx_p=None), dict(pair_len=None), dict(pairs=0), dict(pairs=33), dict(M=0), dict(B=4),
                dict(C=24), dict(H=100), dict(group=-1), dict(sa=None), dict(feat=None)):
        assert _fwd(**dict(STACKED, **bad)) == EINVAL, bad


def test_backward_entries_reject_bad_arguments_on_the_host():
    need = _native.lib().d3f_detection_rows_ws_bytes(2 * 16)
    for bad in (dict(feat=None), dict(idx=None), dict(fmax=None), dict(idx_a=None), dict(idx_p=None), dict(aux=None),
                dict(grad_x=None), dict(ws=None), dict(N=0), dict(M=0), dict(stride=0), dict(C=48), dict(H=65),
                dict(len=A, B=0, group=2)):
        assert _bwd(**bad) == EINVAL, bad
    assert _bwd(ws_bytes=need - 1) == EWORKSPACE
    need = _native.lib().d3f_detection_rows_ws_bytes(2 * 3 * 16)
    for bad in (dict(idx_a=None, idx_p=None), dict(pair_len=None), dict(pairs=0), dict(pairs=33), dict(B=5), dict(C=20),
                dict(H=65), dict(aux=None), dict(grad_x=None), dict(ws=None)):
        assert _bwd(**dict(STACKED, **bad)) == EINVAL, bad
    assert _bwd(**dict(STACKED, ws_bytes=need - 1)) == EWORKSPACE


def test_select_normalize_without_scores_still_checks_its_buffers():
    # scores given but no place for them; a score gradient that is not the tail of grad_x
    stacked = dict(pairs=3, pair_len=A)
    assert _select_fwd(sa=None, sp=None) == EINVAL
    assert _select_bwd(grad_scores=A + 4) == EINVAL
    assert _select_fwd(sp=None, **stacked) == EINVAL
    assert _select_bwd(grad_scores=A + 4, **stacked) == EINVAL
    assert _select_bwd(grad_x=None, grad_scores=A, **stacked) == EINVAL


def test_every_stage_checks_its_pair_count():
    for f in ROWS_STAGES + LOSS_STAGES:
        assert f(pairs=0) == EINVAL, f.__name__
        assert f(pairs=33) == EINVAL, f.__name__
    for f in ROWS_STAGES:
        assert f(pairs=33, pair_len=A) == EINVAL, f.__name__
        assert f(pairs=2, pair_len=None) == EINVAL, f.__name__              # global rows: one pair
        assert f(pairs=1, p_offset=A, pair_len=A) == EINVAL, f.__name__     # an offset AND cloud-local rows
        assert f(pairs=2, p_offset=A, pair_len=A) == EINVAL, f.__name__


def test_the_one_workgroup_circle_route_serves_one_plain_pair():
    """M = 129 leaves the tiled kernels: one pair, no total, unit weights, and a workspace for the backward."""
    assert _circle_fwd(M=129, pairs=2) == EINVAL
    assert _circle_bwd(M=129, pairs=2) == EINVAL
    assert _circle_fwd(M=129, out_total=A) == EINVAL
    assert _circle_fwd(M=16, C=65, out_total=A) == EINVAL
    assert _circle_fwd(M=129, w=(1.0, 0.5)) == EINVAL
    assert _circle_bwd(M=129, w=(1.0, 0.5)) == EINVAL
    assert _circle_bwd(M=129, ws=None) == EINVAL
    need = _native.lib().d3f_circle_det_loss_ws_bytes(129)
    assert need == 4 * 129 * 129
    assert _circle_bwd(M=129, ws_bytes=need - 1) == EWORKSPACE
    for f in LOSS_STAGES:
        assert f(M=1) == EINVAL and f(M=1025) == EINVAL and f(C=0) == EINVAL, f.__name__
    assert _contrastive_fwd(C=257) == EINVAL and _contrastive_bwd(C=257) == EINVAL
    assert _contrastive_fwd(anchor=None) == EINVAL and _contrastive_bwd(stats=None) == EINVAL


def test_the_tiled_circle_backward_needs_no_workspace():
    """M = 16, C = 32 with ws = NULL passes the argument check.  Past the check stands the launch, which must not
    happen with these addresses: the call is made in a child process that sees no device, and only there."""
    child = ("import torch\n"
             "assert not torch.cuda.is_available(), 'a device is visible: the call is not made'\n"
             "import test_sparse_detector_abi as t\n"
             "print('rc', t._circle_bwd(M=16, C=32, ws=None, ws_bytes=0))\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    here = os.path.dirname(os.path.abspath(__file__))
    env["PYTHONPATH"] = os.pathsep.join([here, os.path.dirname(here)] + env.get("PYTHONPATH", "").split(os.pathsep))
    out = subprocess.run([sys.executable, "-c", child], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    rc = int(out.stdout.split("rc")[-1])
    assert rc not in (EINVAL, EWORKSPACE), rc
