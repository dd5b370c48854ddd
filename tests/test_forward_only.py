"""Forward-only rendering (GSR_FORWARD_ONLY, include/gsr.h) on the emulator build: the same image and radii as the training
forward, bit for bit, on every scene shape of the tile-first parity test, in both binning arrangements and with
GSR_CULL_EMPTY_TILES; the smaller scratch sizes; the backward guard; the read-only lazy SH rows; and the automatic switch of
both hosts (C++ host: its emulator build; Python host: the mirror)."""
import numpy as np
import pytest
import torch

import forward_only_cases as fo
import parity
from photo_slam_amd import capi
from photo_slam_amd import scene

CPU = torch.device("cpu")
BG = np.array([0.2, 0.5, 0.1], np.float32)


def small_scene(P, W, H, seed, scale_k=0.35):
    return scene.make_cloud(P, W, H, 0.8 * W, 0.8 * W, seed=seed, scale_k=scale_k)


SHAPES = [
    (600, 64, 48, 1, 0.35), (1500, 80, 70, 2, 0.35),
    (300, 96, 64, 5, 1.5),      # large splats: long runs of instance slots
    (40, 16, 16, 7, 0.35),      # a one-tile image: a tile sort of zero passes
    (6000, 64, 64, 3, 0.5),     # lists of ~1 000 entries
    (30000, 32, 32, 4, 0.3),    # lists of more than 2 048 entries
]


@pytest.mark.parametrize("flags", [32, 64, 32 | 8, 64 | 8])   # GSR_BINNING_DEPTH_FIRST / TILE_FIRST, with GSR_CULL_EMPTY_TILES
@pytest.mark.parametrize("P,W,H,seed,scale_k", SHAPES)
def test_forward_only_equals_training_forward(emu_lib_path, oracle, P, W, H, seed, scale_k, flags):
    cl = small_scene(P, W, H, seed, scale_k)
    cam = cl.cameras[0]
    R, color, radii = fo.check_parity(emu_lib_path, CPU, cl, cam, BG, flags)
    ores, ocolor, oradii, _ = parity.run_oracle(oracle, cl, cam, BG, do_backward=False)
    assert np.array_equal(radii.numpy(), oradii)
    assert R == ores.R
    assert float(np.abs(color.numpy() - ocolor).mean()) <= parity.RGB_L1_TOL


@pytest.mark.parametrize("flags", [32, 64])
def test_forward_only_with_more_than_128k_gaussians(emu_lib_path, flags):
    cl = small_scene(150000, 96, 64, 6, 0.5)
    fo.check_parity(emu_lib_path, CPU, cl, cl.cameras[0], BG, flags)


@pytest.mark.parametrize("kw", [dict(use_colors_precomp=True), dict(use_cov3D_precomp=True),
                                dict(use_colors_precomp=True, use_cov3D_precomp=True)])
@pytest.mark.parametrize("flags", [32, 64 | 8])
def test_forward_only_with_precomputed_inputs(emu_lib_path, flags, kw):
    cl = small_scene(1500, 80, 70, 2)
    fo.check_parity(emu_lib_path, CPU, cl, cl.cameras[0], BG, flags, **kw)


def test_forward_only_with_raw_parameters(emu_lib_path):
    """GSR_RAW_*: the model's raw opacity / scaling / rotation, activated in-kernel"""
    cl = small_scene(1500, 80, 70, 2)
    cam = cl.cameras[0]
    a = fo.inputs(cl, cam, BG, CPU)
    a.update(opacity=fo._t(cl.opacity, CPU), scales=fo._t(cl.scaling, CPU), rotations=fo._t(cl.rotation, CPU))
    for flags in (7 | 32, 7 | 64 | 8):
        R0, c0, r0, _, _ = fo.render(emu_lib_path, a, flags)
        R1, c1, r1, _, f = fo.render(emu_lib_path, a, flags | fo.FORWARD_ONLY)
        assert f == 1 and R0 == R1 and torch.equal(c0, c1) and torch.equal(r0, r1)


def test_scratch_sizes(emu_lib_path):
    fo.check_sizes(capi.load(emu_lib_path))


def test_backward_refuses_forward_only_buffers(emu_lib_path):
    cl = small_scene(600, 64, 48, 1)
    fo.check_backward_guard(emu_lib_path, CPU, cl, cl.cameras[0], BG)


@pytest.mark.parametrize("window", [2, 4, 7])
def test_lazy_rows_are_read_only(emu_lib_path, window):
    cl, cams = fo.lazy_scene(400, 48, 32, seed=11)
    fo.check_lazy_read_only(emu_lib_path, CPU, cl, cams, BG, window=window)


def test_host_layers_switch_to_forward_only(emu_lib_path):
    from tests.test_cpp_host import load_host
    cl = small_scene(600, 64, 48, 1)
    fo.check_host_modes(load_host("emu"), emu_lib_path, CPU, cl, cl.cameras[0], BG)


def test_render_view_between_train_steps_python(emu_lib_path):
    cl, cams = fo.lazy_scene(300, 48, 32, seed=21)
    a = fo.run_python_interleaved(emu_lib_path, CPU, cl, cams, True, iterations=12)
    b = fo.run_python_interleaved(emu_lib_path, CPU, cl, cams, False, iterations=12)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_render_view_between_train_steps_cpp(emu_lib_path):
    from tests.test_cpp_host import load_host
    ops = load_host("emu")
    cl, cams = fo.lazy_scene(300, 48, 32, seed=21)
    a = fo.run_cpp_interleaved(ops, CPU, cl, cams, True, iterations=12)
    b = fo.run_cpp_interleaved(ops, CPU, cl, cams, False, iterations=12)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_render_view_keeps_the_training_workspace(emu_lib_path):
    cl, cams = fo.lazy_scene(300, 48, 32, seed=22)
    fo.check_workspace(emu_lib_path, CPU, cl, cams)
