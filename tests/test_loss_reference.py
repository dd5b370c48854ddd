"""The fused L1+SSIM loss, Adam and the depth loss (csrc/train_ops.hip) on the emulator build against float64 references
(loss_cases.py): the content training sees -- converged, flat, black, equal, out-of-range and impulse images, with masks -- at
the sizes where a tiled kernel goes wrong, judged class by class against the error of the float32 ATen formulation; the scalar
staging path, poisoned and guarded buffers, determinism, the upstream gradient, the C++ host; Adam's scalar tail, misaligned
pointers and row periods; the capped grid of the depth loss.  (GPU twin: test_gpu_loss_reference.py.)"""
import pytest
import torch

import loss_cases as lc
from photo_slam_amd import rasterize_points as rp

CPU = torch.device("cpu")


@pytest.fixture()
def emu(emu_lib_path, monkeypatch):
    monkeypatch.setattr(rp, "_LIB_OVERRIDE", emu_lib_path)
    return emu_lib_path


@pytest.mark.parametrize("cls", lc.CLASSES)
def test_loss_class_against_float64(emu, cls):
    lc.check_group(CPU, cls, tag="emu")


@pytest.mark.parametrize("lam", [0.0, 1.0])    # the L1 branch alone, the SSIM branch alone
@pytest.mark.parametrize("cls", lc.CLASSES)
def test_loss_class_single_branch(emu, cls, lam):
    lc.check_group(CPU, cls, lam, tag="emu")


def test_equal_images_have_exactly_zero_l1_gradient(emu):
    lc.check_equal_images(CPU)


def test_scalar_staging_equals_vector_staging(emu):
    lc.check_scalar_staging(CPU)


def test_poisoned_buffers_do_not_reach_the_results(emu):
    lc.check_poisoned_buffers(CPU)


def test_guard_bands_stay_untouched(emu):
    lc.check_guard_bands(CPU)


def test_two_runs_give_the_same_bits(emu):
    lc.check_determinism(CPU, 97, 132, 2)
    lc.check_determinism(CPU, 40, 75, 2)


def test_upstream_gradient_and_is_root(emu):
    lc.check_upstream_gradient(CPU)


def test_cpp_host_loss_equals_python_wrapper(emu):
    from test_cpp_host import load_host
    lc.check_cpp_host(load_host("emu"), CPU)


def test_adam_sizes_against_float64(emu):
    lc.check_adam_sizes(CPU)


def test_adam_misaligned_pointers(emu):
    lc.check_adam_misaligned(CPU)


def test_adam_row_periods_against_float64(emu):
    lc.check_adam_periods(CPU)


def test_adam_multi_equals_single_steps_at_every_size(emu):
    lc.check_adam_multi(CPU)


def test_depth_loss_capped_grid_and_one_pixel(emu):
    lc.check_depth_loss64(CPU, 1449, 1449, seed=2, w=0.05, lo=1e-10, hi=40.0)   # H W > 1024 x 2048: the grid is capped
    lc.check_depth_loss64(CPU, 1, 1)
    lc.check_depth_loss64(CPU, 37, 53)
