"""GPU: colour in TSDF volumes (csrc/tsdf_color.hpp) through the kernels -- integration, ``into=``, the sparse pool,
``color_at`` at hand-placed points, the ray-cast colour, the accuracy against the analytic texture, the coloured
products and the RGB-D model tracker on the device -- against the host twins and the NumPy restatement bit for bit.
Images of 80 x 60 and smaller; tests/tsdf_color_cases.py has the inputs and the checks."""
import numpy as np
import pytest

from d3feat_pytorch_amd import ops
import raycast_cases as RCC
import tsdf_color_cases as CC

pytestmark = pytest.mark.gpu

DEVICE = CC.Backend('')
RENDER_MEDIAN, RENDER_MAX, CLOUD_MEDIAN, CLOUD_MAX = CC.RENDER_MEDIAN, CC.RENDER_MAX, CC.CLOUD_MEDIAN, CC.CLOUD_MAX


@pytest.mark.parametrize("f32", [False, True], ids=['uint16', 'f32'])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("name", CC.INTEGRATION_CASES)
def test_integration_equals_restatement_and_leaves_D_and_w_alone(name, channels, f32):
    CC.check_integration(DEVICE, name, channels, f32)


def test_integration_equals_the_host_twin():
    for name, channels in (('dims_13x9x7', 3), ('room', 1)):
        args = CC.with_depth(CC.case_args(name), False)
        color = CC.case_color(name, channels)
        assert CC.same(DEVICE.integrate(color=color, **args)[3], CC.HOST.integrate(color=color, **args)[3])


def test_planted_nan_and_infinity_poison_exactly_the_voxels_that_read_them():
    assert CC.check_poison(DEVICE) > 0


@pytest.mark.parametrize("name,channels", [('dims_13x9x7', 1), ('partly_outside', 3), ('room', 1), ('room', 3)])
def test_into_continues_colour_bit_for_bit(name, channels):
    whole = CC.check_into(DEVICE, name, channels)
    assert whole[3].is_cuda and CC.same(whole[3], CC.reference(name, channels)[3])


def test_into_rejects_a_wrong_colour_volume():
    CC.check_into_errors(DEVICE)


@pytest.mark.parametrize("f32", [False, True], ids=['uint16', 'f32'])
@pytest.mark.parametrize("channels", [1, 3])
def test_colour_batch_with_a_frameless_volume_under_into(channels, f32):
    whole, pool = CC.check_batch_into(DEVICE, channels, f32)
    assert whole[3].is_cuda and pool[2].is_cuda
    host = CC.batch_host(channels, f32)
    assert all(CC.RC.same_bits(a, b) for a, b in zip((whole[0], whole[1], whole[3]), (host[0], host[1], host[3])))


@pytest.mark.parametrize("name,channels", [(n, 1 + 2 * (i % 2)) for i, n in enumerate(CC.INTEGRATION_CASES)])
def test_sparse_pool_holds_the_dense_colour(name, channels):
    sv, D, w, Cp = CC.check_sparse(DEVICE, name, channels)
    assert Cp.is_cuda


def test_extend_moves_colour_rows_and_zero_fills_new_ones():
    old, new = CC.check_extend(DEVICE, 'room', 1)
    assert new > old > 0
    CC.check_extend(DEVICE, 'partly_outside', 3)


@pytest.mark.parametrize("channels", [1, 3])
def test_color_at_edge_cases(channels):
    assert CC.same(CC.check_color_at(DEVICE, channels), CC.check_color_at(CC.HOST, channels))
    assert CC.same(CC.check_color_at_sparse(DEVICE, channels), CC.check_color_at_sparse(CC.HOST, channels))
    for device, host in zip(CC.check_fold_points(DEVICE, channels), CC.check_fold_points(CC.HOST, channels)):
        assert CC.same(device, host)


@pytest.mark.parametrize("name", sorted(RCC.cases()) + list(CC.FOLD_CASES))
def test_raycast_colour(name):
    depth, colour = CC.check_raycast(DEVICE, name)
    if name in RCC.ALL_ZERO:
        assert not depth.any() and np.isnan(colour).all()
    else:
        assert np.isfinite(colour).any() == bool(depth.any())
    if name in CC.FOLD_CASES:       # the middle view hits in each of its four blocks of 16 x 16; its neighbours see no cell
        halves = (slice(0, 16), slice(16, None))
        assert all(depth[1, v, u].any() for v in halves for u in halves) and not depth[0].any() and not depth[2].any()


def test_a_view_is_identical_alone_in_a_batch_reversed_and_rerun():
    CC.check_view_alone_batch_reversed_rerun(DEVICE)


def test_rendered_intensity_against_the_analytic_texture():
    """As on the CPU: the restatement's median 0.00247 and maximum 0.1606 over the hit pixels within one voxel of the
    analytic depth (under 3 % are not); the device within 1.5 x of both."""
    CC.check_render_accuracy(DEVICE, RENDER_MEDIAN, RENDER_MAX)


def test_cloud_colour_against_the_analytic_texture():
    """As on the CPU: the restatement's median 0.00313 and maximum 0.2235 at the extracted points; the device within
    1.5 x of both."""
    CC.check_cloud_accuracy(DEVICE, CLOUD_MEDIAN, CLOUD_MAX)


def test_products_carry_colours_and_equal_the_cpu_path(tmp_path):
    clouds, colors, meshes = CC.check_products('cuda')
    cpu = CC.check_products('cpu')
    for g in range(2):
        assert CC.same(clouds[g], cpu[0][g]) and CC.same(colors[g], cpu[1][g])
        assert CC.same(meshes[g][0], cpu[2][g][0]) and CC.same(meshes[g][3], cpu[2][g][3])
    CC.check_max_bytes('cuda')
    CC.check_ply(tmp_path, clouds, colors, meshes)


@pytest.mark.parametrize("sparse", [False, True], ids=['dense', 'sparse'])
def test_slide_model_pass_is_singular_without_colour_and_tracks_with_it(sparse):
    """As on the CPU, on the device; and the device's poses against the CPU path's to 1e-6 with equal statuses."""
    poses, status, model_status = CC.track_slide('cuda', sparse, False)
    assert model_status.tolist() == [ops.ODO_ST_SINGULAR] * 5 and not status.any()
    poses, status, model_status = CC.track_slide('cuda', sparse, True)
    assert model_status.tolist() == [0] * 5 and not status.any()
    cpu = CC.track_slide('cpu', sparse, True)
    assert np.abs(poses - cpu[0]).max() <= 1e-6
    assert np.array_equal(status, cpu[1]) and np.array_equal(model_status, cpu[2])


@pytest.mark.parametrize("sparse", [False, True], ids=['dense', 'sparse'])
def test_slide_colour_model_within_twice_the_frame_to_frame_error(sparse):
    """The bound of the CPU test of the same name, on the device (there 0.0089 deg / 0.136 mm against 0.0071 deg /
    0.114 mm); the device agrees with the CPU path to 1e-6."""
    model, pairs = CC.slide_errors('cuda', sparse)
    assert model[0] <= 2.0 * pairs[0] and model[1] <= 2.0 * pairs[1]


@pytest.mark.parametrize("sparse", [False, True], ids=['dense', 'sparse'])
def test_noisy_room_colour_model_ends_closer_in_rotation(sparse):
    """As on the CPU (0.1821 against 0.2467 degrees; 3.678 against 2.788 mm, not asserted), and the device's poses against
    the CPU path's to 1e-6 with equal statuses."""
    poses, status, model_status = CC.track_noisy_room('cuda', sparse)
    assert model_status.tolist() == [0] * 11 and not status.any()
    model, pairs = CC.room_errors('cuda', sparse)
    assert model[0] < pairs[0]
    cpu = CC.track_noisy_room('cpu', sparse)
    assert np.abs(poses - cpu[0]).max() <= 1e-6
    assert np.array_equal(status, cpu[1]) and np.array_equal(model_status, cpu[2])
