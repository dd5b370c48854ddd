"""3DGS-MCMC relocation, growth and position noise on the MI355X (GPU twin of test_mcmc.py; shared checks and their bars:
mcmc_cases.py).  The sizes are the workgroup and wave boundaries of the per-row kernels plus the first size past one chunk of the
spine scan (1024 block totals of 256 rows), which the emulator file leaves to this one.

Measured on the MI355X (every case of this file): weights at most 1 unit from round(sigmoid64 * 2^24) (bar 4);
new values (o', scale', the stored logit and log-scale against the float64 definition) largest relative error 1.65e-5, the emulator
build the same 1.65e-5: bar 1e-3; the noise step's displacement 8.01e-5 of the row's largest component (at P = 262 444), the emulator
build the same: bar 1e-3; out_alpha at the centre before / after a relocation: relative difference exactly 0 in all four cases on both
builds, bar 1e-6; C++ host against Python host after 22 steps with mcmc on: largest parameter difference 6.0e-7 (emulator build
4.4e-6).  A whole train step is NOT the same bits on every run here (the backward blend adds with float atomics), so the off-is-off
check compares calls, not bits; the kernels of this feature are the same bits on every run (test_same_bits_on_every_run)."""
import pytest
import torch

import mcmc_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device (MI355X)")
    return torch.device("cuda:0")


@pytest.mark.parametrize("P", mc.SIZES + [mc.PAST_ONE_CHUNK])
def test_relocate_at_every_size(dev, P):
    mc.check_relocate(None, dev, P, seed=P)


@pytest.mark.parametrize("M", [1, 16])
def test_relocate_other_sh_rows(dev, M):
    mc.check_relocate(None, dev, 257, M=M, seed=2)


def test_relocate_without_moments_and_extras(dev):
    mc.check_relocate(None, dev, 1025, moments=False, extras=False, seed=4)


def test_edge_draws_and_prefix_boundaries(dev):
    mc.check_edge_draws(None, dev)


def test_all_rows_dead(dev):
    mc.check_all_dead(None, dev)


def test_no_row_dead(dev):
    mc.check_none_dead(None, dev)


def test_fewer_draws_than_dead_rows(dev):
    mc.check_fewer_draws_than_dead(None, dev)


def test_one_source_drawn_60_times(dev):
    mc.check_one_source_60_times(None, dev)


@pytest.mark.parametrize("P,n_add", [(1, 1), (64, 3), (257, 12), (1025, 51), (33000, 1650), (mc.PAST_ONE_CHUNK, 13122)])
def test_growth(dev, P, n_add):
    mc.check_growth(None, dev, P, n_add, seed=P)


@pytest.mark.parametrize("P", mc.SIZES + [mc.PAST_ONE_CHUNK])
def test_noise_at_every_size(dev, P):
    mc.check_noise(None, dev, P, seed=P)


def test_noise_corner_cases(dev):
    mc.check_noise_corners(None, dev)


def test_same_bits_on_every_run(dev):
    mc.check_determinism(None, dev)


def test_api_contract(dev):
    mc.check_api_contract(None, dev)


@pytest.mark.parametrize("o", [0.3, 0.9])
@pytest.mark.parametrize("k", [1, 4])
def test_relocation_keeps_the_alpha_at_the_centre(dev, o, k):
    mc.check_alpha_is_kept(None, dev, o, k)


def test_python_model_calls(dev):
    mc.check_host_model_calls(None, dev)


def test_python_train_step_grows_to_the_cap_and_stays(dev):
    mc.check_host_training(None, dev)


def test_python_train_step_adds_noise_every_step(dev):
    mc.check_host_noise_runs_every_step(None, dev)


def test_python_train_step_off_is_off(dev):
    mc.check_host_off_is_off(None, dev)


def test_python_train_step_refuses_a_process_group(dev):
    mc.check_process_group_is_refused(None, dev)
