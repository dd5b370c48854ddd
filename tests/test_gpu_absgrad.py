"""Absolute screen-space gradients (gsr_backward_args.dL_dmean2D_abs) on the MI355X: the cases of test_absgrad.py against the same
per-pixel references (absgrad_cases.py), both binning arrangements, both forms of the backward blend -- other outputs held to the
rerun tolerance of pose_grad_cases.same_or_rerun_close, since two runs of the device's backward blend differ in the order of their
LDS adds -- and one call each at C1, at C2 (one wave per quad) and at a full C3 view (half tiles) for the bound and for "nothing
else moves", which need no per-pixel reference."""
import pytest
import torch

import absgrad_cases as ac
from photo_slam_amd import capi
from photo_slam_amd import scene

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    assert capi.load().gsr_backend() == b"hip-gfx950"
    return torch.device("cuda:0")


@pytest.mark.parametrize("form", ac.FORMS)
@pytest.mark.parametrize("flags", ac.FLAGS)
@pytest.mark.parametrize("name", ac.CASES)
def test_against_per_pixel_reference_on_gpu(oracle, monkeypatch, name, flags, form):
    dev = _dev()
    monkeypatch.setenv("GSR_BWD_HALF_TILES", form)
    ac.check_case(None, dev, name, flags, exact=False)


@pytest.mark.parametrize("form", ac.FORMS)
@pytest.mark.parametrize("flags", ac.FLAGS)
def test_single_pixel_equality_on_gpu(monkeypatch, flags, form):
    dev = _dev()
    monkeypatch.setenv("GSR_BWD_HALF_TILES", form)
    ac.check_single_pixel(None, dev, flags)


@pytest.mark.parametrize("form", ac.FORMS)
@pytest.mark.parametrize("flags", ac.FLAGS)
def test_fused_statistics_and_separate_pass_on_gpu(monkeypatch, flags, form):
    dev = _dev()
    monkeypatch.setenv("GSR_BWD_HALF_TILES", form)
    ac.check_fused_stats(None, dev, flags, exact=False)


@pytest.mark.parametrize("antialias", [False, True])
@pytest.mark.parametrize("form", ac.FORMS)
def test_fused_optimizer_and_antialiasing_on_gpu(monkeypatch, form, antialias):
    dev = _dev()
    monkeypatch.setenv("GSR_BWD_HALF_TILES", form)
    ac.check_fused_optimizer_and_antialias(None, dev, 64 if antialias else 32, False, antialias)


@pytest.mark.parametrize("form", ac.FORMS)
def test_regularisers_and_pose_outputs_on_gpu(monkeypatch, form):
    dev = _dev()
    monkeypatch.setenv("GSR_BWD_HALF_TILES", form)
    ac.check_with_regulariser_and_pose(None, dev, 32, exact=False)


def test_api_contract_on_gpu():
    ac.check_api_contract(None, _dev())


@pytest.mark.parametrize("config,flags", [("C1", 32), ("C2", 64), ("C3", 32)])
def test_bound_and_unchanged_outputs_at_baseline_shapes(config, flags):
    """C1 and C2 take the quad form of the backward blend, a full C3 view the half tiles (gsr_api.hip: blend_bwd_half_tiles)"""
    dev = _dev()
    cl = scene.make_config(config, seed=1)
    ac.check_bound_only(None, dev, cl, cl.cameras[0], flags)
