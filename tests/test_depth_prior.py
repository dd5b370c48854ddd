"""The monocular depth prior on the emulator build (depth_prior_cases.py): the aligned L1 and the Pearson loss in both spaces against
float64 references group by group, the properties (affine invariance, the degenerate rule, NaN in invalid pixels), the hygiene
checks of the other loss kernels (scalar path, guarded buffers, determinism, the upstream gradient, the C++ op),
gsr_depth_prior_apply, descent at the loss level, the gradients through the rasterizer, and TrainStep / alignDepthPrior on both
hosts.  (GPU twin: test_gpu_depth_prior.py.)"""
import pytest
import torch

import depth_prior_cases as dp
from photo_slam_amd import rasterize_points as rp

CPU = torch.device("cpu")


@pytest.fixture()
def emu(emu_lib_path, monkeypatch):
    monkeypatch.setattr(rp, "_LIB_OVERRIDE", emu_lib_path)
    return emu_lib_path


def _host():
    from test_cpp_host import load_host
    return load_host("emu")


@pytest.mark.parametrize("mode", dp.MODES, ids=dp.mode_id)
@pytest.mark.parametrize("content", dp.CONTENTS)
def test_depth_prior_group_against_float64(emu, content, mode):
    dp.check_group(CPU, content, mode, tag="emu")


def test_depth_prior_is_invariant_to_an_affine_map_of_the_prior(emu):
    dp.check_affine_invariance(CPU)


def test_depth_prior_degenerate_input_gives_exact_zeros(emu):
    dp.check_degenerate(CPU)


def test_depth_prior_nan_in_invalid_pixels_changes_no_bit(emu):
    dp.check_nan_in_invalid_pixels(CPU)


def test_depth_prior_scalar_path_equals_vector_path(emu):
    dp.check_scalar_path(CPU)


def test_depth_prior_fit_only_call(emu):
    dp.check_fit_only(CPU)


def test_depth_prior_guard_bands_stay_untouched(emu):
    dp.check_guard_bands(CPU)


def test_depth_prior_two_runs_give_the_same_bits(emu):
    dp.check_determinism(CPU, 97, 132, 2)


def test_depth_prior_upstream_gradient(emu):
    dp.check_upstream_gradient(CPU)


def test_depth_prior_cpp_op_equals_python_wrapper(emu):
    dp.check_cpp_host(_host(), CPU)


def test_depth_prior_apply_against_float64_and_in_place(emu):
    dp.check_apply(CPU)


def test_depth_prior_descent_raises_the_correlation(emu):
    dp.check_descent(CPU)


def test_depth_prior_gradients_through_the_rasterizer(emu):
    dp.check_through_rasterizer(CPU)


def test_train_step_with_a_depth_prior_python(emu):
    dp.check_train_python(emu, CPU)


def test_train_step_with_a_depth_prior_cpp(emu):
    dp.check_train_cpp(_host(), emu, CPU)


def test_depth_prior_with_a_process_group_throws_cpp(emu, tmp_path):
    dp.check_process_group_cpp(_host(), CPU, tmp_path)


def test_align_depth_prior_and_seed_python(emu):
    dp.check_align_and_seed_python(emu, CPU)


def test_align_depth_prior_and_seed_cpp(emu):
    dp.check_align_and_seed_cpp(_host(), emu, CPU)
