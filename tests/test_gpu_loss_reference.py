"""The fused L1+SSIM loss, Adam and the depth loss on the MI355X against float64 references (CPU twin: test_loss_reference.py; the
cases, references and bars: loss_cases.py).  Both references are computed on the CPU here as well.  The device build contracts
a * b + c to FMA, the emulator build does not: the class bars are the same."""
import pytest
import torch

import loss_cases as lc
from photo_slam_amd import capi

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    assert capi.load().gsr_backend() == b"hip-gfx950"
    return torch.device("cuda:0")


@pytest.mark.parametrize("cls", lc.CLASSES)
def test_loss_class_against_float64_on_gpu(cls):
    lc.check_group(_dev(), cls, tag="gpu")


@pytest.mark.parametrize("lam", [0.0, 1.0])    # the L1 branch alone, the SSIM branch alone
@pytest.mark.parametrize("cls", lc.CLASSES)
def test_loss_class_single_branch_on_gpu(cls, lam):
    lc.check_group(_dev(), cls, lam, tag="gpu")


def test_equal_images_have_exactly_zero_l1_gradient_on_gpu():
    lc.check_equal_images(_dev())


def test_scalar_staging_equals_vector_staging_on_gpu():
    lc.check_scalar_staging(_dev())


def test_poisoned_buffers_do_not_reach_the_results_on_gpu():
    lc.check_poisoned_buffers(_dev())


def test_guard_bands_stay_untouched_on_gpu():
    lc.check_guard_bands(_dev())


def test_ten_runs_give_the_same_bits_on_gpu():
    lc.check_determinism(_dev(), 97, 132, 10)


def test_upstream_gradient_and_is_root_on_gpu():
    lc.check_upstream_gradient(_dev())


def test_cpp_host_loss_equals_python_wrapper_on_gpu():
    dev = _dev()
    from test_cpp_host import load_host
    lc.check_cpp_host(load_host("hip"), dev)


def test_adam_sizes_against_float64_on_gpu():
    lc.check_adam_sizes(_dev())


def test_adam_misaligned_pointers_on_gpu():
    lc.check_adam_misaligned(_dev())


def test_adam_row_periods_against_float64_on_gpu():
    lc.check_adam_periods(_dev())


def test_adam_multi_equals_single_steps_at_every_size_on_gpu():
    lc.check_adam_multi(_dev())


def test_depth_loss_capped_grid_and_one_pixel_on_gpu():
    dev = _dev()
    lc.check_depth_loss64(dev, 1449, 1449, seed=2, w=0.05, lo=1e-10, hi=40.0)   # H W > 1024 x 2048: the grid is capped
    lc.check_depth_loss64(dev, 1, 1)
    lc.check_depth_loss64(dev, 37, 53)
