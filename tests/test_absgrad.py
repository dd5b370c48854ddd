"""Absolute screen-space gradients (gsr_backward_args.dL_dmean2D_abs, AbsGS / gsplat's absgrad) on the emulator build: the [P,2]
array against the per-pixel reference formed from the unchanged CPU oracle (absgrad_cases.py), in both binning arrangements and
both forms of the backward blend; the bound and the single-pixel equality against dL_dmean2D; every other output bit for bit that
of the call without the field; the fused statistics and gsr_densify_stats_abs; the fused optimizers, anti-aliasing, the
regularisers and the pose outputs; the API contract.  (GPU twin: test_gpu_absgrad.py.)"""
import pytest
import torch

import absgrad_cases as ac

CPU = torch.device("cpu")


@pytest.mark.parametrize("form", ac.FORMS)
@pytest.mark.parametrize("flags", ac.FLAGS)
@pytest.mark.parametrize("name", ac.CASES)
def test_against_per_pixel_reference(emu_lib_path, oracle, monkeypatch, name, flags, form):
    monkeypatch.setenv("GSR_BWD_HALF_TILES", form)
    ac.check_case(emu_lib_path, CPU, name, flags, exact=True)


@pytest.mark.parametrize("form", ac.FORMS)
@pytest.mark.parametrize("flags", ac.FLAGS)
def test_single_pixel_equality(emu_lib_path, monkeypatch, flags, form):
    monkeypatch.setenv("GSR_BWD_HALF_TILES", form)
    ac.check_single_pixel(emu_lib_path, CPU, flags)


@pytest.mark.parametrize("form", ac.FORMS)
@pytest.mark.parametrize("flags", ac.FLAGS)
def test_fused_statistics_and_separate_pass(emu_lib_path, monkeypatch, flags, form):
    monkeypatch.setenv("GSR_BWD_HALF_TILES", form)
    ac.check_fused_stats(emu_lib_path, CPU, flags, exact=True)


@pytest.mark.parametrize("antialias", [False, True])
@pytest.mark.parametrize("form", ac.FORMS)
def test_fused_optimizer_and_antialiasing(emu_lib_path, monkeypatch, form, antialias):
    monkeypatch.setenv("GSR_BWD_HALF_TILES", form)
    ac.check_fused_optimizer_and_antialias(emu_lib_path, CPU, 64 if antialias else 32, True, antialias)


@pytest.mark.parametrize("form", ac.FORMS)
def test_regularisers_and_pose_outputs(emu_lib_path, monkeypatch, form):
    monkeypatch.setenv("GSR_BWD_HALF_TILES", form)
    ac.check_with_regulariser_and_pose(emu_lib_path, CPU, 32, exact=True)


def test_api_contract(emu_lib_path):
    ac.check_api_contract(emu_lib_path, CPU)
