"""The walk over the kernel variants of the backward pass (variant_cases.py) on the MI355X: the cases of
test_variant_dispatch.py -- 16 of 48 combinations accepted per case -- with the outputs of a toggled feature's neighbours held to
the rerun tolerance of pose_grad_cases.same_or_rerun_close, since the device's backward blend adds with float atomics."""
import pytest
import torch

import variant_cases as vc
from photo_slam_amd import capi

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("form", vc.FORMS)
@pytest.mark.parametrize("antialias", [False, True])
@pytest.mark.parametrize("rows_ok", [True, False])
def test_every_combination_is_launched_or_refused_on_gpu(monkeypatch, rows_ok, antialias, form):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    assert capi.load().gsr_backend() == b"hip-gfx950"
    monkeypatch.setenv("GSR_BWD_HALF_TILES", form)
    assert vc.walk(None, torch.device("cuda:0"), rows_ok, antialias, exact=False) == vc.ACCEPTED
