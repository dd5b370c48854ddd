"""Per-Gaussian contribution statistics of a render (GSR_CONTRIBUTION: out_weight_sum / out_weight_max / out_n_touched) and the
pruning by them, on the emulator build (contribution_cases.py; GPU twin: test_gpu_contribution.py): the statistics against the
oracle in both binning arrangements with and without a weight map, their invariants, the render's outputs unchanged, determinism,
accumulation over views, gsr_backward behind a forward with the bit, argument errors, and score_contribution /
prune_uncontributing / covisibility of both hosts.

test_reference_input_condition asserts the condition the reference check puts on its inputs: the Gaussians with a pixel whose
decisions sit inside rounding noise are at most 40 % of the visible ones (the oracle alone: 20 % / 16 % at scale_k = 0.2 without /
with a weight map, 15 % / 14 % at 0.6)."""
import pytest
import torch

import contribution_cases as cc

CPU = torch.device("cpu")
KS = [0.2, 0.6]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("k", KS)
def test_reference_input_condition(oracle, k, weighted):
    cc.check_input_condition(oracle, k, weighted)


@pytest.mark.parametrize("flags", [32, 64])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("k", KS)
def test_against_reference(emu_lib_path, oracle, k, weighted, flags):
    print(cc.check_reference(emu_lib_path, CPU, oracle, k, weighted, flags))


@pytest.mark.parametrize("flags", [32, 64])
@pytest.mark.parametrize("k", KS)
def test_invariants(emu_lib_path, k, flags):
    print(cc.check_invariants(emu_lib_path, CPU, k, flags))


@pytest.mark.parametrize("k", KS)
def test_bit_identity(emu_lib_path, k):
    cc.check_bit_identity(emu_lib_path, CPU, k)


@pytest.mark.parametrize("flags", [32, 64 | 8])
def test_accumulate(emu_lib_path, flags):
    cc.check_accumulate(emu_lib_path, CPU, 0.6, flags)


@pytest.mark.parametrize("flags", [32, 64])
def test_backward_after_contribution_forward(emu_lib_path, flags):
    cc.check_backward_after(emu_lib_path, CPU, 0.6, flags, exact=True)


def test_options(emu_lib_path):
    cc.check_options(emu_lib_path, CPU)


def test_argument_errors(emu_lib_path, monkeypatch):
    cc.check_argument_errors(emu_lib_path, CPU)


def test_hosts_python(emu_lib_path, monkeypatch):
    from photo_slam_amd import rasterize_points as rp
    monkeypatch.setattr(rp, "_LIB_OVERRIDE", emu_lib_path)
    cc.check_host_python(CPU)


def test_hosts_cpp(emu_lib_path):
    from tests.test_cpp_host import load_host
    cc.check_host_cpp(load_host("emu"), emu_lib_path, CPU)


def test_hosts_agree(emu_lib_path):
    from tests.test_cpp_host import load_host
    cc.check_hosts_agree(load_host("emu"), emu_lib_path, CPU)
