"""CPU: the plumbing of the deterministic training mode -- the flag from the config / the Trainer's args to TrainStep, the
process-wide switch and its scope, what the pyramid builders are told, and the new entry points in the C header."""
import re

import numpy as np
import pytest
import torch

from d3feat_pytorch_amd import config as cfgmod
from d3feat_pytorch_amd import _native, ops
from d3feat_pytorch_amd.models.architectures import KPFCNN
from d3feat_pytorch_amd.train import TrainStep
from d3feat_pytorch_amd.trainer import Trainer

LIMITS = [5, 5, 5, 5, 5]
NEW_ENTRIES = ("d3f_max_pool_backward_gather", "d3f_closest_pool_backward_gather", "d3f_kpconv_grad_input_modes_gather",
               "d3f_bias_act_backward_ordered_ws_bytes", "d3f_bias_act_backward_ordered", "d3f_loss_rows_record_width",
               "d3f_loss_rows_backward_records", "d3f_loss_rows_backward_apply")


@pytest.fixture(autouse=True)
def _mode_off_afterwards():
    assert not ops.is_deterministic()
    yield
    ops.set_deterministic(False)


def _small_model():
    np.random.seed(0)
    torch.manual_seed(0)
    return KPFCNN(cfgmod.default_config(first_features_dim=16))


class _Loader:
    def __init__(self):
        self.dataset, self.batch_size, self.shuffle, self.limits = [], 1, False, LIMITS


def _args(tmp, **kw):
    cfg = cfgmod.default_config(first_features_dim=16)
    cfg.max_epoch, cfg.save_dir, cfg.tboard_dir, cfg.device, cfg.graph = 2, str(tmp / 'snap'), str(tmp / 'tb'), 'cpu', False
    cfg.train_loader, cfg.model = _Loader(), _small_model()
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def test_the_mode_is_off_by_default_and_scoped():
    assert cfgmod.default_config().deterministic is False
    assert ops.set_deterministic(True) is False and ops.is_deterministic()
    assert ops.set_deterministic(False) is True and not ops.is_deterministic()
    with ops.deterministic_mode(True):
        assert ops.is_deterministic()
        with ops.deterministic_mode(False):
            assert not ops.is_deterministic()
        assert ops.is_deterministic()
    assert not ops.is_deterministic()
    with pytest.raises(ValueError):
        with ops.deterministic_mode(True):
            raise ValueError("inside")
    assert not ops.is_deterministic()


def test_wants_reverse_table_follows_the_mode():
    few, many = ops.DX_GATHER_MIN_ROWS - 1, ops.DX_GATHER_MIN_ROWS
    assert not ops.wants_reverse_table(few) and ops.wants_reverse_table(many)
    with ops.deterministic_mode(True):
        assert ops.wants_reverse_table(1) and ops.wants_reverse_table(few) and ops.wants_reverse_table(many)
        assert not ops.wants_reverse_table(0)
    assert not ops.wants_reverse_table(few)


def test_flag_reaches_trainstep_from_config_and_argument():
    model = _small_model()
    dev = torch.device('cpu')
    assert TrainStep(cfgmod.default_config(first_features_dim=16), LIMITS, dev, model=model).deterministic is False
    on = TrainStep(cfgmod.default_config(first_features_dim=16, deterministic=True), LIMITS, dev, model=model)
    assert on.deterministic is True
    # the argument outranks the config, both ways
    assert TrainStep(cfgmod.default_config(first_features_dim=16), LIMITS, dev, model=model, deterministic=True).deterministic
    assert not TrainStep(cfgmod.default_config(first_features_dim=16, deterministic=True), LIMITS, dev, model=model,
                         deterministic=False).deterministic
    # the engine's scope: the mode holds inside and the process-wide setting comes back
    with on._mode():
        assert ops.is_deterministic()
    assert not ops.is_deterministic()
    off = TrainStep(cfgmod.default_config(first_features_dim=16), LIMITS, dev, model=model)
    ops.set_deterministic(True)
    with off._mode():                  # an engine that does not ask leaves a mode the user set alone
        assert ops.is_deterministic()
    assert ops.is_deterministic()
    # lanes and capacity classes are copies of the engine: they keep its choice
    import copy
    assert copy.copy(on).deterministic is True


def test_flag_reaches_trainstep_from_trainer_args(tmp_path):
    assert Trainer(_args(tmp_path)).engine.deterministic is False
    tr = Trainer(_args(tmp_path, deterministic=True))
    assert tr.deterministic is True and tr.engine.deterministic is True


def test_new_entry_points_are_declared_and_say_what_they_replace():
    with open(_native.HEADER) as f:
        text = f.read()
    for name in NEW_ENTRIES:
        assert name in _native.SIGNATURES, name
        # the comment block in front of the prototype names the scatter it replaces
        head = text[:text.index(name + "(")]
        comment = head[head.rindex("/*"):]
        assert re.search(r"replaces", comment), name
    res, args = _native.SIGNATURES["d3f_max_pool_backward_gather"]
    assert res is _native.C.c_int and len(args) == 10
    assert _native.SIGNATURES["d3f_bias_act_backward_ordered_ws_bytes"][0] is _native.C.c_size_t


def test_new_entry_points_bind():
    L = _native.lib()
    for name in NEW_ENTRIES:
        assert getattr(L, name).argtypes == _native.SIGNATURES[name][1], name
    assert L.d3f_loss_rows_record_width(32, 7) == 32 + 3 + 7 and L.d3f_loss_rows_record_width(0, 7) == 0
    # argument checks run before anything touches a device
    assert L.d3f_max_pool_backward_gather(None, None, 4, 8, 4, None, None, None, None, None) == _native.D3F_EINVAL
    assert L.d3f_closest_pool_backward_gather(None, 4, 4, 8, 4, None, None, None, None) == _native.D3F_EINVAL
    assert L.d3f_bias_act_backward_ordered_ws_bytes(100, 64) >= 4 * 64 * ((100 + 15) // 16)
    assert L.d3f_bias_act_backward_ordered_ws_bytes(5000, 64) == L.d3f_bias_act_backward_ws_bytes(5000, 64)


def test_unconverted_operators_name_themselves():
    with pytest.raises(RuntimeError, match=r"my_op does not have a deterministic implementation .*set_deterministic"):
        ops._no_deterministic_form("my_op")
