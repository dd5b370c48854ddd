"""Opacity / scale / isotropy regularisers inside the backward pass on the MI355X (GPU twin of test_geom_reg.py; shared checks and
their bars: geom_reg_cases.py).  Small scenes only (96 x 64 and smaller): the per-Gaussian kernel goes wrong at workgroup
boundaries, not at scale.

Measured on the MI355X: the term alone <= 1.5e-6 element-wise (bar 1e-5); added to a real gradient <= 7.0e-8 of
the L1 mass (bar 1e-4); the loss values <= 8.4e-8 (bar 1e-5), bit-identical between reruns and binning arrangements; needles after
30 steps: mean max / min scale 7.987 without and 7.172 with isotropic_reg_ = 10; hidden Gaussians: mean activated opacity 0.500
without and 0.190 with opacity_reg_ = 0.01."""
import pytest
import torch

import geom_reg_cases as gr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device (MI355X)")
    return torch.device("cuda:0")


@pytest.mark.parametrize("P", gr.SIZES)
def test_term_in_isolation_at_every_size(dev, P):
    gr.check_isolated(None, dev, P, raw=gr.ALL_RAW)


@pytest.mark.parametrize("raw", [0, 1, 2, 3, 4, 7])
def test_term_in_isolation_raw_on_and_off(dev, raw):
    gr.check_isolated(None, dev, 330, raw=raw, flags=gr.TILE_FIRST)


@pytest.mark.parametrize("kw", [dict(scale_modifier=1.7), dict(scale_modifier=0.6, raw=gr.ALL_RAW), dict(path="compact"),
                                dict(path="compact", raw=gr.ALL_RAW), dict(path="colors"), dict(path="colors", raw=2),
                                dict(aa=True), dict(aa=True, raw=gr.ALL_RAW), dict(aa=True, path="compact", raw=1)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_term_in_isolation_configurations(dev, kw):
    gr.check_isolated(None, dev, 330, **kw)


def test_term_in_isolation_without_the_loss(dev):
    gr.check_isolated(None, dev, 330, raw=gr.ALL_RAW, want_loss=False)


def test_isotropy_corner_cases(dev):
    gr.check_isotropy_corners(None, dev)


@pytest.mark.parametrize("kw", [dict(), dict(raw=gr.ALL_RAW), dict(raw=gr.ALL_RAW, maps=True), dict(aa=True, raw=1),
                                dict(path="compact", maps=True), dict(path="colors", raw=2)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()) or "plain")
def test_added_to_a_real_gradient(dev, kw):
    gr.check_added(None, dev, 330, **kw)


@pytest.mark.parametrize("P,aa", [(129, False), (330, True), (33000, False)])
def test_loss_values_and_their_bits(dev, P, aa):
    gr.check_loss_values(None, dev, P, aa=aa)


@pytest.mark.parametrize("mode", ["geom-only", "sh-eager", "sh-lazy"])
def test_fused_step(dev, mode):
    gr.check_fused(None, dev, lazy=mode == "sh-lazy", sh_adam=mode != "geom-only")


@pytest.mark.parametrize("raw", [0, gr.ALL_RAW])
def test_off_is_off(dev, raw):
    gr.check_off_is_off(None, dev, raw=raw)


def test_api_contract(dev):
    gr.check_api_contract(None, dev)


def test_python_host_isotropy_rounds_needles(dev):
    gr.check_host_isotropy(None, dev)


def test_python_host_opacity_fades_hidden_gaussians(dev):
    gr.check_host_opacity(None, dev)


def test_python_host_loss_terms(dev):
    gr.check_host_losses(None, dev)
