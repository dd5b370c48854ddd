"""Opacity / scale / isotropy regularisers inside the backward pass (gsr_backward_args.geom_reg) on the emulator build: the term in
isolation against a float64 evaluation of its definition at every workgroup boundary, the isotropy corner cases, the term added to
a real gradient, the loss values and their reproducibility, the fused geom_adam step, off-is-off, the API contract, and the Python
host's TrainStep.  Shared checks: geom_reg_cases.py; GPU twin: test_gpu_geom_reg.py; the C++ host's: test_cpp_host_geom_reg.py."""
import pytest
import torch

import geom_reg_cases as gr

CPU = torch.device("cpu")


@pytest.mark.parametrize("P", gr.SIZES)
def test_term_in_isolation_at_every_size(emu_lib_path, P):
    gr.check_isolated(emu_lib_path, CPU, P, raw=gr.ALL_RAW)


@pytest.mark.parametrize("raw", [0, 1, 2, 3, 4, 7])
def test_term_in_isolation_raw_on_and_off(emu_lib_path, raw):
    gr.check_isolated(emu_lib_path, CPU, 330, raw=raw, flags=gr.TILE_FIRST)


@pytest.mark.parametrize("kw", [dict(scale_modifier=1.7), dict(scale_modifier=0.6, raw=gr.ALL_RAW), dict(path="compact"),
                                dict(path="compact", raw=gr.ALL_RAW), dict(path="colors"), dict(path="colors", raw=2),
                                dict(aa=True), dict(aa=True, raw=gr.ALL_RAW), dict(aa=True, path="compact", raw=1)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_term_in_isolation_configurations(emu_lib_path, kw):
    gr.check_isolated(emu_lib_path, CPU, 330, **kw)


def test_term_in_isolation_without_the_loss(emu_lib_path):
    gr.check_isolated(emu_lib_path, CPU, 330, raw=gr.ALL_RAW, want_loss=False)


def test_isotropy_corner_cases(emu_lib_path):
    gr.check_isotropy_corners(emu_lib_path, CPU)


@pytest.mark.parametrize("kw", [dict(), dict(raw=gr.ALL_RAW), dict(raw=gr.ALL_RAW, maps=True), dict(aa=True, raw=1),
                                dict(path="compact", maps=True), dict(path="colors", raw=2)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()) or "plain")
def test_added_to_a_real_gradient(emu_lib_path, kw):
    gr.check_added(emu_lib_path, CPU, 330, **kw)


@pytest.mark.parametrize("P,aa", [(129, False), (330, True), (33000, False)])
def test_loss_values_and_their_bits(emu_lib_path, P, aa):
    gr.check_loss_values(emu_lib_path, CPU, P, aa=aa)


@pytest.mark.parametrize("mode", ["geom-only", "sh-eager", "sh-lazy"])
def test_fused_step(emu_lib_path, mode):
    gr.check_fused(emu_lib_path, CPU, lazy=mode == "sh-lazy", sh_adam=mode != "geom-only")


@pytest.mark.parametrize("raw", [0, gr.ALL_RAW])
def test_off_is_off(emu_lib_path, raw):
    gr.check_off_is_off(emu_lib_path, CPU, raw=raw)


def test_api_contract(emu_lib_path):
    gr.check_api_contract(emu_lib_path, CPU)


def test_python_host_isotropy_rounds_needles(emu_lib_path):
    gr.check_host_isotropy(emu_lib_path, CPU)


def test_python_host_opacity_fades_hidden_gaussians(emu_lib_path):
    gr.check_host_opacity(emu_lib_path, CPU)


def test_python_host_loss_terms(emu_lib_path):
    gr.check_host_losses(emu_lib_path, CPU)
