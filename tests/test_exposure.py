"""Per-keyframe exposure compensation on the emulator build (exposure_cases.py): the fused loss behind a [3,4] colour map against
float64 references class by class, the identity map against the plain entry bit for bit, the hygiene checks of the plain loss
(staging paths, poisoned and guarded buffers, determinism, the upstream gradient, the C++ op), gsr_apply_exposure, convergence of
the map at the loss level, and TrainStep on both hosts.  (GPU twin: test_gpu_exposure.py.)"""
import pytest
import torch

import exposure_cases as ec
import loss_cases as lc
from photo_slam_amd import rasterize_points as rp

CPU = torch.device("cpu")


@pytest.fixture()
def emu(emu_lib_path, monkeypatch):
    monkeypatch.setattr(rp, "_LIB_OVERRIDE", emu_lib_path)
    return emu_lib_path


def _host():
    from test_cpp_host import load_host
    return load_host("emu")


@pytest.mark.parametrize("map_name", list(ec.MAPS))
@pytest.mark.parametrize("cls", lc.CLASSES)
def test_exposure_loss_class_against_float64(emu, cls, map_name):
    ec.check_group(CPU, cls, map_name, tag="emu")


@pytest.mark.parametrize("map_name", list(ec.MAPS))
@pytest.mark.parametrize("lam", [0.0, 1.0])
@pytest.mark.parametrize("cls", ec.BRANCH_CLASSES)
def test_exposure_loss_single_branch(emu, cls, lam, map_name):
    ec.check_group(CPU, cls, map_name, lam, tag="emu")


def test_identity_exposure_equals_plain_loss(emu):
    ec.check_identity(CPU)


def test_exposure_scalar_staging_equals_vector_staging(emu):
    ec.check_scalar_staging(CPU)


def test_exposure_poisoned_buffers_do_not_reach_the_results(emu):
    ec.check_poisoned_buffers(CPU)


def test_exposure_guard_bands_stay_untouched(emu):
    ec.check_guard_bands(CPU)


def test_exposure_two_runs_give_the_same_bits(emu):
    ec.check_determinism(CPU, 97, 132, 2)


def test_exposure_upstream_gradient_and_is_root(emu):
    ec.check_upstream_gradient(CPU)


def test_exposure_cpp_op_equals_python_wrapper(emu):
    ec.check_cpp_host(_host(), CPU)


def test_apply_exposure_against_float64_and_in_place(emu):
    ec.check_apply(CPU)


def test_exposure_converges_at_the_loss_level(emu):
    ec.check_convergence(CPU)


def test_train_step_optimizes_keyframe_exposures_python(emu):
    ec.check_train_python(emu, CPU)


def test_train_step_optimizes_keyframe_exposures_cpp(emu):
    ec.check_train_cpp(_host(), CPU)


def test_identity_exposures_leave_the_train_step_unchanged_python(emu):
    ec.check_identity_train_python(emu, CPU)


def test_identity_exposures_leave_the_train_step_unchanged_cpp(emu):
    ec.check_identity_train_cpp(_host(), CPU)


def test_refine_pose_applies_the_keyframe_exposure_python(emu, oracle):
    ec.check_refine_python(emu, CPU, oracle)


def test_refine_pose_applies_the_keyframe_exposure_cpp(emu, oracle):
    ec.check_refine_cpp(_host(), CPU, oracle)


def test_exposure_with_a_process_group_throws_python(emu):
    ec.check_process_group_python(emu, CPU)


def test_exposure_with_a_process_group_throws_cpp(emu, tmp_path):
    ec.check_process_group_cpp(_host(), CPU, tmp_path)
