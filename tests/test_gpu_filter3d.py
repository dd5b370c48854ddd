"""The 3-D smoothing filter (GSR_FILTER_3D and gsr_filter3d_compute) on the MI355X (CPU twin: test_filter3d.py): the filter against
its numpy restatement bit for bit (division and square root are the correctly rounded ones on the device), the forward pass against
the oracle's render of (s', o') at C1 and C2, the backward pass against the oracle's gradients pushed through the filter's chain
rule at C1 (both binning arrangements, both backward forms), once at C2 and on the sub-pixel scene; the all-zero filter, the error
rules, the fused geometry step, the pose gradients, the autograd node, both hosts and the PLY forms at C1 size or below.  Gradients
are compared with tolerances (two runs of one program differ in the last bits of a gradient on the device); the forward pass's
bit-exact checks hold."""
import numpy as np
import pytest
import torch

import filter3d_cases as f3
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


@pytest.mark.parametrize("K", [0, 1, 3])
@pytest.mark.parametrize("P", [0, 40, 1500, 30000])
def test_compute_on_gpu(P, K):
    dev = _dev()
    cl = scene.make_cloud(max(P, 1), 64, 48, 51.2, 51.2, seed=3, scale_k=0.35, n_views=3)
    filt, obs = f3.check_compute(None, dev, cl, f3.camera_rows(cl.cameras[:K]), P=P)
    if P and not K:
        assert not filt.any()


def test_compute_beyond_one_grid_pyramid_and_upstream_on_gpu():
    """300 000 Gaussians: more rows than the capped grid has threads, so every thread strides; K = 40 cameras; a pyramid against
    the float64 definition; equal cameras against upstream's compute_3D_filter; a camera that sees nothing"""
    dev = _dev()
    cl = scene.make_cloud(300_000, 64, 48, 51.2, 51.2, seed=3, scale_k=0.35, n_views=40)
    f3.check_compute(None, dev, cl, f3.camera_rows(cl.cameras))
    cl = scene.make_cloud(1500, 64, 48, 51.2, 51.2, seed=3, scale_k=0.35, n_views=3)
    rows = f3.camera_rows(cl.cameras, levels=[1, 2, 4])
    got, obs = f3.check_compute(None, dev, cl, rows)
    want, obs64 = f3.filter64(cl.xyz, rows)
    assert np.array_equal(obs, obs64) and (np.abs(got - want) / want).max() <= 1e-6
    rows = f3.camera_rows(cl.cameras)
    got = f3.compute(None, dev, cl.xyz, rows)
    want = f3.upstream_filter(cl.xyz, rows)
    assert (np.abs(got - want) / want).max() <= 1e-6
    rows = rows[:1].copy()
    rows[0, 14] -= 100.0
    got, obs = f3.check_compute(None, dev, cl, rows)
    assert not obs.any() and not got.any()


@pytest.mark.parametrize("flags", [32, 64 | 8, 64 | fo.FORWARD_ONLY, 32 | 8 | fo.FORWARD_ONLY])
def test_forward_on_gpu(oracle, flags):
    dev = _dev()
    cl = scene.make_config("C1", seed=1, n_views=3)
    f3.check_forward(None, dev, oracle, cl, cl.cameras[0], BG, flags)


def test_forward_at_c2_on_gpu(oracle):
    dev = _dev()
    cl = scene.make_config("C2", seed=1)
    f3.check_forward(None, dev, oracle, cl, cl.cameras[0], BG, 64 | 8)


@pytest.mark.parametrize("kw", [dict(raw=True), dict(use_colors_precomp=True), dict(antialias=True, maps=True)])
def test_forward_with_raw_inputs_colours_maps_and_antialiasing_on_gpu(oracle, kw):
    dev = _dev()
    cl = scene.make_config("C1", seed=2, n_views=3)
    f3.check_forward(None, dev, oracle, cl, cl.cameras[0], BG, 64 | 8, **kw)


def test_forward_of_sub_pixel_gaussians_on_gpu(oracle):
    dev = _dev()
    cl = scene.make_config("C1", seed=9, scale_k=0.01, n_views=3)
    rep = f3.check_forward(None, dev, oracle, cl, cl.cameras[0], BG, 64)
    assert rep["c_mean"] < 0.2, rep   # the filter dominates


@pytest.mark.parametrize("form", ["0", "1"])   # GSR_BWD_HALF_TILES
@pytest.mark.parametrize("flags,maps", [(64, True), (32 | 8, False)])
def test_backward_on_gpu(oracle, monkeypatch, flags, maps, form):
    dev = _dev()
    monkeypatch.setenv("GSR_BWD_HALF_TILES", form)
    cl = scene.make_config("C1", seed=1, n_views=3)
    f3.check_backward(None, dev, oracle, cl, cl.cameras[0], BG, flags, seed=1, maps=maps)


def test_backward_at_c2_on_gpu(oracle):
    dev = _dev()
    cl = scene.make_config("C2", seed=1)
    f3.check_backward(None, dev, oracle, cl, cl.cameras[0], BG, 64, seed=1)


@pytest.mark.parametrize("kw", [dict(raw=True), dict(raw=True, antialias=True, maps=True)])
def test_backward_with_raw_parameters_and_antialiasing_on_gpu(oracle, kw):
    dev = _dev()
    cl = scene.make_config("C1", seed=2, n_views=3)
    f3.check_backward(None, dev, oracle, cl, cl.cameras[0], BG, 64, seed=3, **kw)


def test_backward_of_sub_pixel_gaussians_on_gpu(oracle):
    dev = _dev()
    cl = scene.make_config("C1", seed=9, scale_k=0.01, n_views=3)
    f3.check_backward(None, dev, oracle, cl, cl.cameras[0], BG, 64, seed=9, maps=True, opacity_term_min=1e-3)   # ten times the aggregate bar


def test_zero_filter_error_rules_fused_step_and_pose_on_gpu(oracle):
    dev = _dev()
    cl = scene.make_config("C1", seed=3, n_views=3)
    cam = cl.cameras[0]
    f3.check_zero_filter(None, dev, cl, cam, BG, 64)
    f3.check_zero_filter(None, dev, cl, cam, BG, 32, raw=True, antialias=True)
    f3.check_errors(None, dev, cl, cam, BG)
    f3.check_fused_geom_adam(None, dev, cl, cam, BG)
    f3.check_fused_geom_adam(None, dev, cl, cam, BG, reg=True)
    f3.check_pose(None, dev, oracle, cl, cam, BG)


def test_autograd_node_hosts_and_ply_on_gpu(oracle, tmp_path):
    dev = _dev()
    from tests.test_cpp_host import load_host
    ops = load_host("hip")
    cl = scene.make_cloud(600, 64, 48, 51.2, 51.2, seed=1, scale_k=0.35, n_views=3)
    f3.check_autograd(None, dev, oracle, cl)
    f3.check_recompute_python(None, dev, cl)
    f3.check_recompute_cpp(ops, dev, cl)
    f3.check_ply(ops, None, dev, oracle, cl, tmp_path)
    cl = scene.make_config("C1", seed=4, n_views=3)
    f3.check_hosts(ops, None, dev, cl, steps=6, exact=False)
