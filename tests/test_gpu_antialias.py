"""Anti-aliased rendering (GSR_ANTIALIAS) on the MI355X (CPU twin: test_antialias.py): the forward pass against the oracle's render
with opacities o h32 and against the library's own render without the bit, the backward pass against the oracle's gradients plus
the h term, at C1 and at C2 (a mid-size view), in both binning arrangements and both backward forms; the maps' gradients, the fused
geometry step, the pose gradients, the clamp, the energy of an isolated Gaussian, level consistency, the autograd node and both
hosts at C1.  Gradients are compared with tolerances (two runs of one program differ in the last bits of a gradient on the device);
the forward pass's bit-exact checks hold."""
import numpy as np
import pytest
import torch

import antialias_cases as aa
import forward_only_cases as fo
from photo_slam_amd import capi
from photo_slam_amd import scene

pytestmark = pytest.mark.gpu
BG = np.array([0.2, 0.5, 0.1], np.float32)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    assert capi.load().gsr_backend() == b"hip-gfx950"
    return torch.device("cuda:0")


@pytest.mark.parametrize("flags", [32, 64 | 8, 64 | fo.FORWARD_ONLY, 32 | 8 | fo.FORWARD_ONLY])
@pytest.mark.parametrize("config", ["C1", "C2"])
def test_forward_on_gpu(oracle, config, flags):
    dev = _dev()
    cl = scene.make_config(config, seed=1)
    aa.check_forward(None, dev, oracle, cl, cl.cameras[0], BG, flags)


@pytest.mark.parametrize("kw", [dict(raw=True), dict(use_colors_precomp=True), dict(use_cov3D_precomp=True)])
def test_forward_with_raw_and_precomputed_inputs_on_gpu(oracle, kw):
    dev = _dev()
    cl = scene.make_config("C1", seed=2)
    aa.check_forward(None, dev, oracle, cl, cl.cameras[0], BG, 64 | 8, **kw)


@pytest.mark.parametrize("form", ["0", "1"])   # GSR_BWD_HALF_TILES
@pytest.mark.parametrize("config,flags", [("C1", 64), ("C1", 32 | 8), ("C2", 64)])
def test_backward_on_gpu(oracle, monkeypatch, config, flags, form):
    dev = _dev()
    monkeypatch.setenv("GSR_BWD_HALF_TILES", form)
    cl = scene.make_config(config, seed=1)
    aa.check_backward(None, dev, oracle, cl, cl.cameras[0], BG, flags, seed=1, maps=True)


def test_backward_of_sub_pixel_gaussians_on_gpu(oracle):
    dev = _dev()
    cl = scene.make_config("C1", seed=9, scale_k=0.01)   # (sigma ~ 0.2 px at 3 m)
    aa.check_backward(None, dev, oracle, cl, cl.cameras[0], BG, 64, seed=9, maps=True, h_term_min=1e-3)   # ten times the aggregate bar


def test_backward_with_precomputed_covariance_on_gpu(oracle):
    dev = _dev()
    cl = scene.make_config("C1", seed=2)
    aa.check_backward(None, dev, oracle, cl, cl.cameras[0], BG, 32, seed=4, use_cov3D_precomp=True)


def test_mismatch_guard_fused_step_and_pose_on_gpu(oracle):
    dev = _dev()
    cl = scene.make_config("C1", seed=3)
    cam = cl.cameras[0]
    aa.check_mismatch_guard(None, dev, cl, cam, BG)
    aa.check_fused_geom_adam(None, dev, cl, cam, BG)
    aa.check_pose(None, dev, oracle, cl, cam, BG)


def test_clamp_energy_and_levels_on_gpu(oracle):
    dev = _dev()
    aa.check_clamp(None, dev, oracle, BG)
    aa.check_energy(None, dev, oracle)
    d_with, d_without, sub, means = aa.level_consistency(None, dev)
    print("measured: |mean alpha fine - coarse| with the bit", d_with, "without", d_without, "ratio", d_without / max(d_with, 1e-30))
    assert sub > 0.5 and d_with < d_without


def test_autograd_node_and_hosts_on_gpu():
    dev = _dev()
    from tests.test_cpp_host import load_host
    cl = scene.make_config("C1", seed=4)
    aa.check_autograd(None, dev, cl)
    aa.check_hosts(load_host("hip"), None, dev, cl, steps=6, exact=False)
