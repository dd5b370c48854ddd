"""Camera pose gradients and pose refinement on the MI355X (GPU twin of test_pose_grad.py; shared checks: pose_grad_cases.py):
(a) the raw gradients against float64 autograd, (b) the rigid-motion identity through the oracle's gradients at full size -- C1, C2,
C3 and a C5 view, both binning arrangements, a random and a coherent upstream gradient -- (c) unchanged behaviour and
bit-reproducible sums at C3, (d) refinePose on the Python host (the C++ host's: test_cpp_host_pose.py).

Measured on the MI355X (DESIGN.md section 5 has the tables): (a) <= 4.2e-6; (b) random <= 2.7e-6 of the mass, coherent <= 2.5e-6 of
|sum|; (d) refinePose 0.021 % of the mean depth / 0.024 deg, with depth 0.016 % / 0.011 deg (reference loop 0.021 % / 0.014 deg and
0.016 % / 0.016 deg; bound 0.175 % / 0.112 deg)."""
import numpy as np
import pytest
import torch

import pose_grad_cases as pg
from photo_slam_amd import scene

pytestmark = pytest.mark.gpu
BG = np.array([0.2, 0.5, 0.1], np.float32)
BOTH = (pg.DEPTH_FIRST, pg.TILE_FIRST)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device (MI355X)")
    return torch.device("cuda:0")


@pytest.mark.parametrize("seed,deg", pg.AUTOGRAD_CASES)
def test_raw_gradients_match_float64_autograd(oracle, dev, seed, deg):
    pg.check_against_autograd(None, dev, oracle, seed, deg)


@pytest.mark.parametrize("seed", [1, 2, 4])
def test_depth_upstream_matches_float64_autograd(oracle, dev, seed):
    pg.check_depth_against_autograd(None, dev, oracle, seed)


@pytest.mark.parametrize("upstream", ["random", "coherent"])
@pytest.mark.parametrize("cfg,mode", [("C1", "sh0"), ("C1", "cov"), ("C2", "colors"), ("C3", "sh0"), ("C5", "sh0")])
def test_rigid_motion_identity_at_full_size(oracle, dev, cfg, mode, upstream):
    cl = scene.make_config(cfg, seed=0)
    pg.check_rigid_identity(None, dev, oracle, cl, cl.cameras[0], BG, BOTH, mode=mode, upstream=upstream)


@pytest.mark.parametrize("kw", [dict(), dict(maps=True, stats=True), dict(use_colors_precomp=True), dict(sh_coeffs=9, deg=2)],
                         ids=["plain", "maps-stats", "colors", "compact-sh"])
def test_other_outputs_unchanged_and_sums_reproducible_at_C3(dev, kw):
    cl = scene.make_config("C3", seed=0)
    one = pg.check_unchanged(None, dev, cl, cl.cameras[0], BG, pg.DEPTH_FIRST, **kw)
    other = pg.check_unchanged(None, dev, cl, cl.cameras[0], BG, pg.TILE_FIRST, **kw)
    same = pg.pose_same_or_close(one, other, "depth-first and tile-first binning gave different pose gradients", False)
    print("measured: per-Gaussian gradients of the two arrangements bit-identical:", same)
    assert float(one[8].abs().sum()) > 0 and float(one[9].abs().sum()) > 0


@pytest.mark.parametrize("lazy", [False, True])
def test_fused_steps_unchanged(dev, lazy):
    cl = scene.make_config("C3", seed=0)
    pg.check_unchanged_fused(None, dev, cl, cl.cameras[0], BG, pg.DEPTH_FIRST, lazy=lazy)


def test_api_contract(dev):
    cl = scene.make_cloud(1, 96, 64, 80.0, 80.0, seed=0)
    cam = scene.make_camera(96, 64, 80.0, 80.0, np.eye(3), np.zeros(3))
    cl.xyz[:] = [0.0, 0.0, 3.0]
    pg.check_api_contract(None, dev, cl, cam, BG)


@pytest.mark.parametrize("with_depth", [False, True])
def test_refine_pose_converges_python(oracle, dev, with_depth):
    pg.check_refine_python(None, dev, oracle, with_depth=with_depth)
