"""Depth and alpha maps with gradients (gsr_forward_args.out_depth / out_alpha, gsr_backward_args.dL_ddepth / dL_dalpha) and the
RGB-D depth loss, on the emulator build: the maps and the gradients against the CPU oracle (depth_alpha_cases.py), in both binning
arrangements, with and without GSR_CULL_EMPTY_TILES / GSR_FORWARD_ONLY, both backward forms; zero upstream gradients change
nothing; the fused geometry step; gsr_depth_l1_loss; autograd; and the train step of both hosts.  (GPU twin:
test_gpu_depth_alpha.py.)"""
import numpy as np
import pytest
import torch

import depth_alpha_cases as da
import forward_only_cases as fo
from photo_slam_amd import scene

CPU = torch.device("cpu")
BG = np.array([0.2, 0.5, 0.1], np.float32)
from test_forward_only import SHAPES, small_scene   # noqa: E402  (the shapes of the forward-only tests)


@pytest.mark.parametrize("flags", [32, 64 | 8, 64 | fo.FORWARD_ONLY, 32 | 8 | fo.FORWARD_ONLY])
@pytest.mark.parametrize("P,W,H,seed,scale_k", SHAPES)
def test_forward_maps(emu_lib_path, oracle, P, W, H, seed, scale_k, flags):
    cl = small_scene(P, W, H, seed, scale_k)
    print(da.check_forward(emu_lib_path, CPU, oracle, cl, cl.cameras[0], BG, flags))


@pytest.mark.parametrize("kw", [dict(use_colors_precomp=True), dict(use_cov3D_precomp=True)])
@pytest.mark.parametrize("flags", [32, 64 | 8])
def test_forward_maps_with_precomputed_inputs(emu_lib_path, oracle, flags, kw):
    cl = small_scene(1500, 80, 70, 2)
    da.check_forward(emu_lib_path, CPU, oracle, cl, cl.cameras[0], BG, flags, **kw)


def test_forward_maps_with_raw_parameters(emu_lib_path):
    cl = small_scene(1500, 80, 70, 2)
    cam = cl.cameras[0]
    a = fo.inputs(cl, cam, BG, CPU)
    ref = da.render(emu_lib_path, a, 32)
    a.update(opacity=fo._t(cl.opacity, CPU), scales=fo._t(cl.scaling, CPU), rotations=fo._t(cl.rotation, CPU))
    for flags in (7 | 32, 7 | 64 | 8, 7 | 64 | fo.FORWARD_ONLY):
        R, c, r, d, al, _ = da.render(emu_lib_path, a, flags)
        assert R == ref[0] and torch.equal(r, ref[2])
        assert float((d - ref[3]).abs().max()) <= 1e-4 * float(ref[3].abs().max()) and float((al - ref[4]).abs().max()) <= 1e-5


def test_empty_model_leaves_the_maps_untouched(emu_lib_path):
    cl = small_scene(10, 32, 32, 1)
    a = fo.inputs(cl, cl.cameras[0], BG, CPU)
    for k in ("means3D", "opacity", "scales", "rotations", "sh"):
        a[k] = a[k][:0]
    R, _, _, d, al, _ = da.render(emu_lib_path, a, 0)
    assert R == 0 and bool((d == -7).all()) and bool((al == -7).all())


@pytest.mark.parametrize("form", ["0", "1"])   # GSR_BWD_HALF_TILES: quads / half tiles
@pytest.mark.parametrize("P,W,H,seed,scale_k", [SHAPES[0], SHAPES[2], SHAPES[5]])
def test_backward_against_oracle(emu_lib_path, oracle, monkeypatch, form, P, W, H, seed, scale_k):
    monkeypatch.setenv("GSR_BWD_HALF_TILES", form)
    cl = small_scene(P, W, H, seed, scale_k)
    print(da.check_backward(emu_lib_path, CPU, oracle, cl, cl.cameras[0], BG, 64, seed=seed))


@pytest.mark.parametrize("form", ["0", "1"])
@pytest.mark.parametrize("P,W,H,fx,seed", [(20000, 189, 125, 150.0, 12), (8000, 9, 200, 160.0, 14)])
def test_backward_at_image_edges(emu_lib_path, oracle, monkeypatch, form, P, W, H, fx, seed):
    """the edge cases of test_blend_bwd_half_tiles.py: partial quads, right quads / bottom halves outside the image"""
    monkeypatch.setenv("GSR_BWD_HALF_TILES", form)
    cl = scene.make_cloud(P, W, H, fx, fx, seed=seed, scale_k=0.2)
    print(da.check_backward(emu_lib_path, CPU, oracle, cl, cl.cameras[0], BG, 32 | 8, seed=seed))


@pytest.mark.parametrize("which", ["depth", "alpha"])
@pytest.mark.parametrize("form", ["0", "1"])
def test_backward_with_one_map(emu_lib_path, oracle, monkeypatch, which, form):
    monkeypatch.setenv("GSR_BWD_HALF_TILES", form)
    cl = small_scene(1500, 80, 70, 2)
    da.check_backward(emu_lib_path, CPU, oracle, cl, cl.cameras[0], BG, 64, seed=3, use_depth=which == "depth",
                      use_alpha=which == "alpha")


@pytest.mark.parametrize("kw", [dict(use_colors_precomp=True), dict(use_cov3D_precomp=True)])
def test_backward_with_precomputed_inputs(emu_lib_path, oracle, kw):
    cl = small_scene(1500, 80, 70, 2)
    da.check_backward(emu_lib_path, CPU, oracle, cl, cl.cameras[0], BG, 32, seed=4, **kw)


@pytest.mark.parametrize("form", ["0", "1"])
@pytest.mark.parametrize("P,W,H,seed,scale_k", [SHAPES[1], SHAPES[2]])
def test_zero_upstream_equals_plain_backward(emu_lib_path, monkeypatch, form, P, W, H, seed, scale_k):
    monkeypatch.setenv("GSR_BWD_HALF_TILES", form)
    cl = small_scene(P, W, H, seed, scale_k)
    da.check_zero_upstream(emu_lib_path, CPU, cl, cl.cameras[0], BG, 64)


def test_fused_geom_adam_with_depth_gradient(emu_lib_path):
    cl = small_scene(1500, 80, 70, 2)
    da.check_fused_geom_adam(emu_lib_path, CPU, cl, cl.cameras[0], BG)


def test_depth_l1_loss(emu_lib_path, monkeypatch):
    from photo_slam_amd import rasterize_points as rp
    monkeypatch.setattr(rp, "_LIB_OVERRIDE", emu_lib_path)
    da.check_depth_loss(CPU)
    da.check_depth_loss(CPU, H=480, W=640, seed=1, w=0.05, lo=1e-10, hi=40.0)


def test_autograd_depth_and_alpha(emu_lib_path, monkeypatch):
    from photo_slam_amd import rasterize_points as rp
    monkeypatch.setattr(rp, "_LIB_OVERRIDE", emu_lib_path)
    da.check_autograd(CPU, small_scene(600, 64, 48, 1))


def test_train_step_python(emu_lib_path, monkeypatch):
    from photo_slam_amd import rasterize_points as rp
    monkeypatch.setattr(rp, "_LIB_OVERRIDE", emu_lib_path)
    da.check_train_step_python(CPU, small_scene(600, 64, 48, 1))



def test_train_step_fused_and_dense_optimizer_agree(emu_lib_path, monkeypatch):
    from photo_slam_amd import rasterize_points as rp
    monkeypatch.setattr(rp, "_LIB_OVERRIDE", emu_lib_path)
    da.check_train_step_fused_unfused(CPU, small_scene(600, 64, 48, 1))


def test_train_step_cpp(emu_lib_path):
    from tests.test_cpp_host import load_host
    da.check_train_step_cpp(load_host("emu"), emu_lib_path, CPU, small_scene(600, 64, 48, 1))


def test_train_step_cpp_and_python_agree(emu_lib_path):
    from tests.test_cpp_host import load_host
    da.check_train_step_hosts(load_host("emu"), emu_lib_path, CPU, small_scene(600, 64, 48, 1))
