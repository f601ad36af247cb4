"""The four host twins d3f_tsdf[_sparse]_integrate_host and d3f_tsdf_raycast[_sparse]_host, called directly: what
`channels` and `into` select, which pointers each form looks at, and the bytes against the NumPy restatement.
No GPU."""
import pytest

import d3feat_pytorch_amd  # noqa: F401
import tsdf_entry_cases as E

HOST = E.HOST
MODELS = [pytest.param(False, id="dense"), pytest.param(True, id="sparse")]


def test_bad_channels_are_einval_before_anything_else():
    E.check_bad_channels(HOST)


@pytest.mark.parametrize("sparse", MODELS)
def test_channels_0_is_the_colourless_form_with_null_colour_pointers(sparse):
    rc, D, w, Cx = E.integrate(HOST, sparse, 0)                  # color, Cv / Cp null
    assert rc == 0 and Cx is None
    want = E.numpy_model(sparse, 0)
    assert E.same(D, want[0]) and E.same(w, want[1])
    rc, depth, normals, image = E.raycast(HOST, sparse, 0, D, w, None)       # Cv / Cp and the colour image null
    assert rc == 0 and image is None
    want = E.numpy_render(sparse, 0)
    assert E.same(depth, want[0]) and E.same(normals, want[1])


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("sparse", MODELS)
def test_channels_1_and_3_need_their_pointers_and_equal_the_restatement(sparse, channels):
    E.check_colour_pointers(HOST, sparse, channels)
    rc, *model = E.integrate(HOST, sparse, channels)
    assert rc == 0
    for got, want in zip(model, E.numpy_model(sparse, channels)):
        assert E.same(got, want)
    plain = E.numpy_model(sparse, 0)
    assert E.same(model[0], plain[0]) and E.same(model[1], plain[1])         # D and w are the colourless call's
    rc, *render = E.raycast(HOST, sparse, channels, *model)
    assert rc == 0
    for got, want in zip(render, E.numpy_render(sparse, channels)):
        assert E.same(got, want)


@pytest.mark.parametrize("channels", [0, 1, 3])
@pytest.mark.parametrize("sparse", MODELS)
def test_into_continues_and_leaves_the_frameless_volume_alone(sparse, channels):
    whole = E.check_into(HOST, sparse, channels)
    for got, want in zip(whole, E.numpy_model(sparse, channels)):
        assert (got is None and want is None) or E.same(got, want)
