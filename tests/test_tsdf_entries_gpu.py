"""The four device entries d3f_tsdf[_sparse]_integrate and d3f_tsdf_raycast[_sparse], called directly on the small
volumes of tsdf_entry_cases and held against their host twins bit for bit, for channels 0, 1, 3 and into 0 / 1."""
import functools

import pytest

import d3feat_pytorch_amd  # noqa: F401
import tsdf_entry_cases as E

pytestmark = pytest.mark.gpu
HOST, DEVICE = E.HOST, E.DEVICE
MODELS = [pytest.param(False, id="dense"), pytest.param(True, id="sparse")]


@functools.lru_cache(maxsize=None)
def twin_model(sparse, channels):
    rc, *model = E.integrate(HOST, sparse, channels)
    assert rc == 0
    return model


def test_bad_channels_are_einval_and_nothing_is_written():
    E.check_bad_channels(DEVICE)


@pytest.mark.parametrize("channels", [0, 1, 3])
@pytest.mark.parametrize("sparse", MODELS)
def test_integrate_equals_the_twin_from_zero_and_into(sparse, channels):
    whole = E.check_into(DEVICE, sparse, channels)               # into = 0, then into = 1, against one call
    for got, want in zip(whole, twin_model(sparse, channels)):
        assert (got is None and want is None) or E.same(got, want)
    if channels:
        E.check_colour_pointers(DEVICE, sparse, channels)


@pytest.mark.parametrize("channels", [0, 1, 3])
@pytest.mark.parametrize("sparse", MODELS)
def test_raycast_equals_the_twin(sparse, channels):
    model = twin_model(sparse, channels)
    rc, *want = E.raycast(HOST, sparse, channels, *model)
    assert rc == 0 and (want[0] > 0).any()
    rc, *got = E.raycast(DEVICE, sparse, channels, *model)
    assert rc == 0
    for a, b in zip(got, want):
        assert (a is None and b is None) or E.same(a, b)
