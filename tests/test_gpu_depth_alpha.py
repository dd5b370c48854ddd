"""Depth and alpha maps with gradients on the MI355X (CPU twin: test_depth_alpha.py): the maps against the oracle with the image,
radii and instance count unchanged, the backward pass against the oracle, and zero upstream gradients, at C1, C2 (the one-wave-per-
quad backward form) and a full C3 view (half tiles), in both binning arrangements; the depth loss and the train step of both hosts at C1.
Gradients are compared with tolerances: two runs of the same program differ in the last bits of a gradient on the device (the
order of the LDS adds in blend_bwd, test_gpu_forward_only.py); the forward pass has no such adds, its bit-exact checks hold."""
import numpy as np
import pytest
import torch

import depth_alpha_cases as da
from photo_slam_amd import capi
from photo_slam_amd import scene

pytestmark = pytest.mark.gpu
BG = np.array([0.2, 0.5, 0.1], np.float32)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    assert capi.load().gsr_backend() == b"hip-gfx950"
    return torch.device("cuda:0")


CONFIGS = ["C1", "C2", "C3"]


@pytest.mark.parametrize("flags", [32, 64])   # GSR_BINNING_DEPTH_FIRST / TILE_FIRST
@pytest.mark.parametrize("config", CONFIGS)
def test_forward_maps_on_gpu(oracle, config, flags):
    dev = _dev()
    cl = scene.make_config(config, seed=1)
    print(da.check_forward(None, dev, oracle, cl, cl.cameras[0], BG, flags))


def test_forward_maps_culled_and_forward_only_on_gpu(oracle):
    dev = _dev()
    cl = scene.make_config("C1", seed=2)
    print(da.check_forward(None, dev, oracle, cl, cl.cameras[0], BG, 32 | 8 | capi.FORWARD_ONLY))


@pytest.mark.parametrize("flags", [32, 64])
@pytest.mark.parametrize("config", CONFIGS)
def test_backward_on_gpu(oracle, config, flags):
    dev = _dev()
    cl = scene.make_config(config, seed=1)
    print(da.check_backward(None, dev, oracle, cl, cl.cameras[0], BG, flags, seed=1))


@pytest.mark.parametrize("flags", [32, 64])
@pytest.mark.parametrize("config", CONFIGS)
def test_zero_upstream_on_gpu(config, flags):
    dev = _dev()
    cl = scene.make_config(config, seed=1)
    da.check_zero_upstream(None, dev, cl, cl.cameras[0], BG, flags, exact=False)


def test_fused_geom_adam_with_depth_gradient_on_gpu():
    dev = _dev()
    cl = scene.make_config("C1", seed=3)
    da.check_fused_geom_adam(None, dev, cl, cl.cameras[0], BG)


def test_depth_loss_autograd_and_train_step_on_gpu():
    dev = _dev()
    da.check_depth_loss(dev)
    da.check_depth_loss(dev, H=1080, W=1920, seed=1, w=0.05, lo=1e-10, hi=40.0)
    cl = scene.make_config("C1", seed=4)
    da.check_autograd(dev, cl)
    da.check_train_step_python(dev, cl, steps=4, exact=False)


def test_train_step_cpp_host_on_gpu():
    """the C++ host's train step with gt_depth, and the two hosts against each other, at C1 (tolerances: two runs of the same
    program differ in the last bits of a gradient on the device)"""
    dev = _dev()
    from tests.test_cpp_host import load_host
    ops = load_host("hip")
    cl = scene.make_config("C1", seed=4)
    da.check_train_step_cpp(ops, None, dev, cl, steps=4, exact=False)
    da.check_train_step_hosts(ops, None, dev, cl, steps=3, exact=False)
    da.check_train_step_fused_unfused(dev, cl, steps=3, exact=False)
