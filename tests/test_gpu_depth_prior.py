"""The monocular depth prior on the MI355X (CPU twin: test_depth_prior.py; cases, references and bars: depth_prior_cases.py).  The
references are computed on the CPU here as well.  Where the emulator run compares two training runs bit for bit, the device run
holds them to pose_grad_cases.DEVICE_RERUN_TOL: the rasterizer's backward is not bit-reproducible from run to run there."""
import pytest
import torch

import depth_prior_cases as dp
from photo_slam_amd import capi

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    assert capi.load().gsr_backend() == b"hip-gfx950"
    return torch.device("cuda:0")


def _host():
    from test_cpp_host import load_host
    return load_host("hip")


@pytest.mark.parametrize("mode", dp.MODES, ids=dp.mode_id)
@pytest.mark.parametrize("content", dp.CONTENTS)
def test_depth_prior_group_against_float64_on_gpu(content, mode):
    dp.check_group(_dev(), content, mode, tag="gpu")


@pytest.mark.parametrize("mode", dp.MODES, ids=dp.mode_id)
def test_depth_prior_full_hd_on_gpu(mode):
    dp.check_full_hd(_dev(), mode)


def test_depth_prior_is_invariant_to_an_affine_map_of_the_prior_on_gpu():
    dp.check_affine_invariance(_dev())


def test_depth_prior_degenerate_input_gives_exact_zeros_on_gpu():
    dp.check_degenerate(_dev())


def test_depth_prior_nan_in_invalid_pixels_changes_no_bit_on_gpu():
    dp.check_nan_in_invalid_pixels(_dev())


def test_depth_prior_scalar_path_equals_vector_path_on_gpu():
    dp.check_scalar_path(_dev())


def test_depth_prior_fit_only_call_on_gpu():
    dp.check_fit_only(_dev())


def test_depth_prior_guard_bands_stay_untouched_on_gpu():
    dp.check_guard_bands(_dev())


def test_depth_prior_ten_runs_give_the_same_bits_on_gpu():
    dp.check_determinism(_dev(), 97, 132, 10)


def test_depth_prior_upstream_gradient_on_gpu():
    dp.check_upstream_gradient(_dev())


def test_depth_prior_cpp_op_equals_python_wrapper_on_gpu():
    dev = _dev()
    dp.check_cpp_host(_host(), dev)


def test_depth_prior_apply_against_float64_and_in_place_on_gpu():
    dp.check_apply(_dev())


def test_depth_prior_descent_raises_the_correlation_on_gpu():
    dp.check_descent(_dev())


def test_depth_prior_gradients_through_the_rasterizer_on_gpu():
    dp.check_through_rasterizer(_dev())


def test_train_step_with_a_depth_prior_python_on_gpu():
    dp.check_train_python(None, _dev())


def test_train_step_with_a_depth_prior_cpp_on_gpu():
    dev = _dev()
    dp.check_train_cpp(_host(), None, dev)


def test_align_depth_prior_and_seed_python_on_gpu():
    dp.check_align_and_seed_python(None, _dev())


def test_align_depth_prior_and_seed_cpp_on_gpu():
    dev = _dev()
    dp.check_align_and_seed_cpp(_host(), None, dev)
