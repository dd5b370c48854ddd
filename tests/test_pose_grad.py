"""Camera pose gradients in the backward pass (gsr_backward_args.dL_dviewmatrix / dL_dprojmatrix / dL_dcampos) and pose refinement
(TrainStep.refinePose), on the emulator build: the raw gradients against float64 autograd of the independent renderer at every SH
degree, the rigid-motion identity through the CPU oracle's gradients, unchanged behaviour of everything else, bit-reproducibility,
both binning arrangements, and convergence of the refinement.  Shared checks: pose_grad_cases.py; GPU twin: test_gpu_pose_grad.py.

Refinement (scene pose_grad_cases.REFINE_SCENE at SH degree 1, 60 Adam steps, lr 2e-3, plain L1; errors as % of the mean depth /
degrees): start 1.75 % / 1.12 deg, bound 0.175 % / 0.112 deg (a tenth of the start; twice the reference's final error is smaller).
  RGB alone:        float64 reference loop 0.021 % / 0.014 deg; refinePose (Python host) emulator 0.021 % / 0.019 deg, MI355X 0.021 % / 0.024 deg
  with depth, 0.01: float64 reference loop 0.016 % / 0.016 deg; refinePose (Python host) emulator 0.017 % / 0.013 deg, MI355X 0.016 % / 0.011 deg
(the C++ host's: test_cpp_host_pose.py)"""
import numpy as np
import pytest
import torch

import pose_grad_cases as pg
from photo_slam_amd import scene
from test_forward_only import small_scene

CPU = torch.device("cpu")
BG = np.array([0.2, 0.5, 0.1], np.float32)


@pytest.mark.parametrize("seed,deg", pg.AUTOGRAD_CASES)
def test_raw_gradients_match_float64_autograd(emu_lib_path, oracle, seed, deg):
    pg.check_against_autograd(emu_lib_path, CPU, oracle, seed, deg)


@pytest.mark.parametrize("flags", [pg.DEPTH_FIRST, pg.TILE_FIRST | 8])
@pytest.mark.parametrize("mode", ["sh0", "colors", "cov"])
def test_rigid_motion_identity_random_upstream(emu_lib_path, oracle, mode, flags):
    cl = small_scene(4000, 160, 120, 3)
    pg.check_rigid_identity(emu_lib_path, CPU, oracle, cl, cl.cameras[0], BG, flags, mode=mode, upstream="random", seed=3)


@pytest.mark.parametrize("mode", ["sh0", "cov"])
def test_rigid_motion_identity_coherent_upstream(emu_lib_path, oracle, mode):
    cl = small_scene(4000, 160, 120, 3)
    pg.check_rigid_identity(emu_lib_path, CPU, oracle, cl, cl.cameras[0], BG, pg.TILE_FIRST, mode=mode, upstream="coherent")


@pytest.mark.parametrize("kw", [dict(), dict(deg=1), dict(deg=0), dict(use_colors_precomp=True), dict(use_cov3D_precomp=True),
                                dict(sh_coeffs=4, deg=1), dict(sh_coeffs=9, deg=2), dict(maps=True), dict(stats=True),
                                dict(maps=True, sh_coeffs=4, deg=1)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()) or "plain")
def test_other_outputs_unchanged_and_sums_reproducible(emu_lib_path, kw):
    cl = small_scene(1500, 80, 70, 2)
    one = pg.check_unchanged(emu_lib_path, CPU, cl, cl.cameras[0], BG, pg.DEPTH_FIRST, **kw)
    other = pg.check_unchanged(emu_lib_path, CPU, cl, cl.cameras[0], BG, pg.TILE_FIRST, **kw)
    pg.pose_same_or_close(one, other, "depth-first and tile-first binning gave different pose gradients", True)
    a = torch.cat([t.reshape(-1) for t in one[8:]]).numpy()
    assert np.abs(a[:32]).sum() > 0
    if kw.get("deg", 3) == 0 or kw.get("use_colors_precomp"):
        assert not a[32:].any()
    else:
        assert a[32:].any()


@pytest.mark.parametrize("lazy", [False, True])
def test_fused_steps_unchanged_and_sums_use_positions_before_the_step(emu_lib_path, lazy):
    cl = small_scene(1500, 80, 70, 2)
    pg.check_unchanged_fused(emu_lib_path, CPU, cl, cl.cameras[0], BG, pg.DEPTH_FIRST, lazy=lazy)


@pytest.mark.parametrize("seed", [1, 2, 4])
def test_depth_upstream_matches_float64_autograd(emu_lib_path, oracle, seed):
    pg.check_depth_against_autograd(emu_lib_path, CPU, oracle, seed)


def test_depth_gradient_reaches_the_pose(emu_lib_path):
    """a loss on the depth map alone reaches the camera (through dL/dz and through the alphas' positions); no loss, no gradient"""
    import forward_only_cases as fo
    cl = small_scene(1500, 80, 70, 2)
    cam = cl.cameras[0]
    a = fo.inputs(cl, cam, BG, CPU)
    zero = torch.zeros((3, cam.H, cam.W))
    out, _ = pg.backward_pose(emu_lib_path, a, cam, 0, zero, dD=torch.ones((cam.H, cam.W)))
    assert float(out[8][3, 2]) != 0 and bool(out[9].any()) and torch.isfinite(out[8]).all()
    out, _ = pg.backward_pose(emu_lib_path, a, cam, 0, zero)
    assert not bool(out[8].any()) and not bool(out[9].any()) and not bool(out[10].any())


def test_api_contract(emu_lib_path):
    cl = scene.make_cloud(1, 96, 64, 80.0, 80.0, seed=0)
    cam = scene.make_camera(96, 64, 80.0, 80.0, np.eye(3), np.zeros(3))
    cl.xyz[:] = [0.0, 0.0, 3.0]
    pg.check_api_contract(emu_lib_path, CPU, cl, cam, BG)


@pytest.mark.parametrize("with_depth", [False, True])
def test_refine_pose_converges_python(emu_lib_path, oracle, with_depth):
    pg.check_refine_python(emu_lib_path, CPU, oracle, with_depth=with_depth)
