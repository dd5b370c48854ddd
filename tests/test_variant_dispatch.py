"""The walk over the kernel variants of the backward pass (variant_cases.py) on the emulator build: per case (rows_ok, antialias,
form of the backward blend) all 48 combinations of depth, pose, geom_reg, absgrad, factored and packed through lib.gsr_backward --
16 accepted, 32 refused with the status include/gsr.h names; outputs of a toggled feature's neighbours bit for bit.  (GPU twin:
test_gpu_variant_dispatch.py.)"""
import pytest
import torch

import variant_cases as vc

CPU = torch.device("cpu")


@pytest.mark.parametrize("form", vc.FORMS)
@pytest.mark.parametrize("antialias", [False, True])
@pytest.mark.parametrize("rows_ok", [True, False])
def test_every_combination_is_launched_or_refused(emu_lib_path, monkeypatch, rows_ok, antialias, form):
    monkeypatch.setenv("GSR_BWD_HALF_TILES", form)
    assert vc.walk(emu_lib_path, CPU, rows_ok, antialias, exact=True) == vc.ACCEPTED
