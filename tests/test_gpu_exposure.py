"""Per-keyframe exposure compensation on the MI355X (CPU twin: test_exposure.py; cases, references and bars: exposure_cases.py).
The references are computed on the CPU here as well.  The identity-exposure train step (exposure_cases.check_identity_train_*)
compares two training runs bit for bit and runs on the emulator only: on the device the backward pass of the rasterizer is not
bit-reproducible from run to run (pose_grad_cases.py: DEVICE_RERUN_TOL).  The refinement against a darkened target
(check_refine_*) runs there too: its float64 reference loop alone takes minutes, and on the device it would exercise nothing
beyond the exposure loss (tested here class by class) behind the host code the emulator run covers."""
import pytest
import torch

import exposure_cases as ec
import loss_cases as lc
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


@pytest.mark.parametrize("map_name", list(ec.MAPS))
@pytest.mark.parametrize("cls", lc.CLASSES)
def test_exposure_loss_class_against_float64_on_gpu(cls, map_name):
    ec.check_group(_dev(), cls, map_name, tag="gpu")


@pytest.mark.parametrize("map_name", list(ec.MAPS))
@pytest.mark.parametrize("lam", [0.0, 1.0])
@pytest.mark.parametrize("cls", ec.BRANCH_CLASSES)
def test_exposure_loss_single_branch_on_gpu(cls, lam, map_name):
    ec.check_group(_dev(), cls, map_name, lam, tag="gpu")


def test_exposure_loss_full_hd_on_gpu():
    ec.check_full_hd(_dev(), "mixing")


def test_identity_exposure_equals_plain_loss_on_gpu():
    ec.check_identity(_dev())


def test_exposure_scalar_staging_equals_vector_staging_on_gpu():
    ec.check_scalar_staging(_dev())


def test_exposure_poisoned_buffers_do_not_reach_the_results_on_gpu():
    ec.check_poisoned_buffers(_dev())


def test_exposure_guard_bands_stay_untouched_on_gpu():
    ec.check_guard_bands(_dev())


def test_exposure_ten_runs_give_the_same_bits_on_gpu():
    ec.check_determinism(_dev(), 97, 132, 10)


def test_exposure_upstream_gradient_and_is_root_on_gpu():
    ec.check_upstream_gradient(_dev())


def test_exposure_cpp_op_equals_python_wrapper_on_gpu():
    dev = _dev()
    ec.check_cpp_host(_host(), dev)


def test_apply_exposure_against_float64_and_in_place_on_gpu():
    ec.check_apply(_dev())


def test_exposure_converges_at_the_loss_level_on_gpu():
    ec.check_convergence(_dev())


def test_train_step_optimizes_keyframe_exposures_python_on_gpu():
    ec.check_train_python(None, _dev())


def test_train_step_optimizes_keyframe_exposures_cpp_on_gpu():
    dev = _dev()
    ec.check_train_cpp(_host(), dev)


def test_exposure_with_a_process_group_throws_python_on_gpu():
    ec.check_process_group_python(None, _dev())
