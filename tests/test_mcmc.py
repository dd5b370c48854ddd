"""3DGS-MCMC relocation, growth and position noise (gsr_mcmc_relocate, gsr_mcmc_add_noise) on the emulator build: weights, exact
sampling, the new values against the float64 definition, read-before-write, determinism, the API contract and the Python host.
Shared checks: mcmc_cases.py; GPU twin: test_gpu_mcmc.py; the C++ host's: test_cpp_host_mcmc.py.

Measured on the emulator build (every case of this file): weights at most 1 unit from round(sigmoid64 * 2^24) (bar 4); new values
(o', scale', the stored logit and log-scale against the float64 definition) largest relative error 1.65e-5, the MI355X the same
1.65e-5: bar 1e-3; the noise step's displacement 8.01e-5 of the row's largest component (at P = 262 444), the MI355X the same: bar
1e-3; out_alpha at the centre before / after a relocation: relative difference exactly 0 in all four cases on both builds, bar 1e-6
(mcmc_cases.py says how each bar follows from its measurements)."""
import pytest
import torch

import mcmc_cases as mc

CPU = torch.device("cpu")


@pytest.mark.parametrize("P", mc.SIZES + [mc.PAST_ONE_CHUNK])
def test_relocate_at_every_size(emu_lib_path, P):
    mc.check_relocate(emu_lib_path, CPU, P, seed=P)


@pytest.mark.parametrize("M", [1, 16])
def test_relocate_other_sh_rows(emu_lib_path, M):
    mc.check_relocate(emu_lib_path, CPU, 257, M=M, seed=2)


def test_relocate_without_moments_and_extras(emu_lib_path):
    mc.check_relocate(emu_lib_path, CPU, 1025, moments=False, extras=False, seed=4)


def test_edge_draws_and_prefix_boundaries(emu_lib_path):
    mc.check_edge_draws(emu_lib_path, CPU)


def test_all_rows_dead(emu_lib_path):
    mc.check_all_dead(emu_lib_path, CPU)


def test_no_row_dead(emu_lib_path):
    mc.check_none_dead(emu_lib_path, CPU)


def test_fewer_draws_than_dead_rows(emu_lib_path):
    mc.check_fewer_draws_than_dead(emu_lib_path, CPU)


def test_one_source_drawn_60_times(emu_lib_path):
    mc.check_one_source_60_times(emu_lib_path, CPU)


@pytest.mark.parametrize("P,n_add", [(1, 1), (64, 3), (257, 12), (1025, 51), (33000, 1650), (mc.PAST_ONE_CHUNK, 13122)])
def test_growth(emu_lib_path, P, n_add):
    mc.check_growth(emu_lib_path, CPU, P, n_add, seed=P)


@pytest.mark.parametrize("P", mc.SIZES + [mc.PAST_ONE_CHUNK])
def test_noise_at_every_size(emu_lib_path, P):
    mc.check_noise(emu_lib_path, CPU, P, seed=P)


def test_noise_corner_cases(emu_lib_path):
    mc.check_noise_corners(emu_lib_path, CPU)


def test_same_bits_on_every_run(emu_lib_path):
    mc.check_determinism(emu_lib_path, CPU)


def test_api_contract(emu_lib_path):
    mc.check_api_contract(emu_lib_path, CPU)


@pytest.mark.parametrize("o", [0.3, 0.9])
@pytest.mark.parametrize("k", [1, 4])
def test_relocation_keeps_the_alpha_at_the_centre(emu_lib_path, o, k):
    mc.check_alpha_is_kept(emu_lib_path, CPU, o, k)


def test_python_model_calls(emu_lib_path):
    mc.check_host_model_calls(emu_lib_path, CPU)


def test_python_train_step_grows_to_the_cap_and_stays(emu_lib_path):
    mc.check_host_training(emu_lib_path, CPU)


def test_python_train_step_adds_noise_every_step(emu_lib_path):
    mc.check_host_noise_runs_every_step(emu_lib_path, CPU)


def test_python_train_step_off_is_off(emu_lib_path):
    mc.check_host_off_is_off(emu_lib_path, CPU)


def test_python_train_step_refuses_a_process_group(emu_lib_path):
    mc.check_process_group_is_refused(emu_lib_path, CPU)
