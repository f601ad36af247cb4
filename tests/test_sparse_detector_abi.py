"""CPU: the entry points of the detector's rows form reject null or inconsistent arguments on the host (D3F_EINVAL, or
D3F_EWORKSPACE for a short workspace) before any launch -- no device is touched.  The addresses below are never read."""
from d3feat_pytorch_amd import _native

EINVAL, EWORKSPACE = -1, -2
A = 0x10000        # a non-null "device address": the checks only compare it with NULL


def _fwd(**kw):
    a = dict(feat=A, N=600, C=32, idx=A, H=40, fmax=A, training=1, width=None, len=None, B=0, group=0, idx_a=A, idx_p=A,
             stride=2, M=16, p_offset=None, sa=A, sp=A, aux=A)
    a.update(kw)
    return _native.lib().d3f_detection_rows_forward(
        a['feat'], a['N'], a['C'], a['idx'], a['H'], a['fmax'], a['training'], a['width'], a['len'], a['B'], a['group'],
        a['idx_a'], a['idx_p'], a['stride'], a['M'], a['p_offset'], a['sa'], a['sp'], a['aux'], None)


def _fwd_pairs(**kw):
    a = dict(feat=A, N=600, C=32, idx=A, H=40, fmax=A, training=1, width=None, len=A, B=6, group=2, corr=A, M=16, pairs=3,
             sa=A, sp=A, aux=A)
    a.update(kw)
    return _native.lib().d3f_detection_rows_forward_pairs(
        a['feat'], a['N'], a['C'], a['idx'], a['H'], a['fmax'], a['training'], a['width'], a['len'], a['B'], a['group'],
        a['corr'], a['M'], a['pairs'], a['sa'], a['sp'], a['aux'], None)


def _bwd(**kw):
    a = dict(feat=A, N=600, C=32, idx=A, H=40, fmax=A, len=None, B=0, group=0, idx_a=A, idx_p=A, stride=2, M=16,
             p_offset=None, aux=A, g_sa=A, g_sp=A, grad_x=A, ws=A, ws_bytes=1 << 20)
    a.update(kw)
    return _native.lib().d3f_detection_rows_backward(
        a['feat'], a['N'], a['C'], a['idx'], a['H'], a['fmax'], a['len'], a['B'], a['group'], a['idx_a'], a['idx_p'],
        a['stride'], a['M'], a['p_offset'], a['aux'], a['g_sa'], a['g_sp'], a['grad_x'], a['ws'], a['ws_bytes'], None)


def _bwd_pairs(**kw):
    a = dict(feat=A, N=600, C=32, idx=A, H=40, fmax=A, len=A, B=6, group=2, corr=A, M=16, pairs=3, aux=A, g_sa=A, g_sp=A,
             grad_x=A, ws=A, ws_bytes=1 << 20)
    a.update(kw)
    return _native.lib().d3f_detection_rows_backward_pairs(
        a['feat'], a['N'], a['C'], a['idx'], a['H'], a['fmax'], a['len'], a['B'], a['group'], a['corr'], a['M'], a['pairs'],
        a['aux'], a['g_sa'], a['g_sp'], a['grad_x'], a['ws'], a['ws_bytes'], None)


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
    for bad in (dict(corr=None), dict(len=None), dict(pairs=0), dict(pairs=33), dict(M=0), dict(B=4), dict(C=24),
                dict(H=100), dict(group=-1), dict(sa=None), dict(feat=None)):
        assert _fwd_pairs(**bad) == EINVAL, bad


def test_backward_entries_reject_bad_arguments_on_the_host():
    need = _native.lib().d3f_detection_rows_ws_bytes(2 * 16)
    for bad in (dict(feat=None), dict(idx=None), dict(fmax=None), dict(idx_a=None), dict(idx_p=None), dict(aux=None),
                dict(grad_x=None), dict(ws=None), dict(N=0), dict(M=0), dict(stride=0), dict(C=48), dict(H=65),
                dict(len=A, B=0, group=2)):
        assert _bwd(**bad) == EINVAL, bad
    assert _bwd(ws_bytes=need - 1) == EWORKSPACE
    need = _native.lib().d3f_detection_rows_ws_bytes(2 * 3 * 16)
    for bad in (dict(corr=None), dict(len=None), dict(pairs=0), dict(pairs=33), dict(B=5), dict(C=20), dict(H=65),
                dict(aux=None), dict(grad_x=None), dict(ws=None)):
        assert _bwd_pairs(**bad) == EINVAL, bad
    assert _bwd_pairs(ws_bytes=need - 1) == EWORKSPACE


def test_select_normalize_without_scores_still_checks_its_buffers():
    lib = _native.lib()
    # scores given but no place for them; a score gradient that is not the tail of grad_x
    assert lib.d3f_select_normalize_forward(A, A, 600, 32, A, A, 2, 16, None, A, A, None, None, None) == EINVAL
    assert lib.d3f_select_normalize_backward(A, 600, 32, A, A, 2, 16, None, A, A, None, None, A, A + 4, None) == EINVAL
    assert lib.d3f_select_normalize_forward_pairs(A, A, 600, 32, A, 16, 3, A, A, A, A, None, None) == EINVAL
    assert lib.d3f_select_normalize_backward_pairs(A, 600, 32, A, 16, 3, A, A, A, None, None, None, A, None) == EINVAL
