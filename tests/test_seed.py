"""Seeding Gaussians from an RGB-D frame (gsr_seed_select, gsr_seed_emit; GaussianModel.seedFromDepth, TrainStep.seedFromDepth) on the
emulator build: the selection, its order, the counts and the median's bits as integers against numpy in float32; the written rows
against float64; thinning, strides, corner values, read-nothing-else, determinism, the API contract and the Python host.
Shared checks: seed_cases.py; GPU twin: test_gpu_seed.py; the C++ host's: test_cpp_host_seed.py.

Measured on the emulator build (every case of this file): written values (xyz relative to the larger of |p_c| and |t|, scaling, the
DC colour and the logit relative to max(1, |value|)) largest relative error 2.95e-7 (xyz, at 1025 x 1024), the MI355X the same
2.95e-7: bar 1e-5 (seed_cases.BAR_VALUES: the next power of ten above ten times the larger).  Host scene (229 x 131, 4000 Gaussians,
the 596 whose means project into the central rectangle pruned): the first seedFromDepth appends 9911 rows (all by the unseen rule;
29 999 valid pixels), the mean alpha over the rectangle rises from 0.195 to 0.958, and the second call selects 0.  The train step
after seeding against the same step after _append_rows: identical bits."""
import pytest
import torch

import seed_cases as sc

CPU = torch.device("cpu")


@pytest.mark.parametrize("W,H", sc.SIZES)
def test_select_and_emit_at_every_size(emu_lib_path, W, H):
    sc.check_case(emu_lib_path, CPU, W, H, seed=W + H)


def test_past_one_chunk_of_the_spine_scan(emu_lib_path):
    """(the absolute threshold alone: the four radix passes over a million emulated pixels belong to the GPU twin)"""
    W, H = sc.PAST_ONE_CHUNK
    sc.check_case(emu_lib_path, CPU, W, H, seed=1, n_emit=lambda s: s // 3, depth_error_abs=0.4, depth_error_median_factor=0.0)


def test_median_bits(emu_lib_path):
    sc.check_median(emu_lib_path, CPU)


def test_strides_and_offsets(emu_lib_path):
    sc.check_strides(emu_lib_path, CPU)


def test_thinning(emu_lib_path):
    sc.check_thinning(emu_lib_path, CPU)


def test_corner_values_and_options(emu_lib_path):
    sc.check_corners(emu_lib_path, CPU)


def test_same_bits_on_every_run(emu_lib_path):
    sc.check_determinism(emu_lib_path, CPU)


def test_api_contract(emu_lib_path):
    sc.check_api_contract(emu_lib_path, CPU)


def test_python_host_seeds_what_the_rule_selects(emu_lib_path):
    sc.check_host_python(emu_lib_path, CPU)


def test_python_host_empty_model_caps_and_process_group(emu_lib_path):
    sc.check_host_empty_and_caps(emu_lib_path, CPU)


def test_python_train_step_after_seeding(emu_lib_path):
    sc.check_host_train_step_after_seeding(emu_lib_path, CPU)
