"""Anti-aliased rendering (GSR_ANTIALIAS, include/gsr.h) on the emulator build: the forward pass against the CPU oracle's render with
opacities o h32 and against the library's own render without the bit; the backward pass against the oracle's gradients plus the
h term (antialias_cases.py), both backward forms, with the maps' gradients, precomputed colours / covariances, the fused geometry
step and the pose gradients; the clamp; the energy of an isolated Gaussian; level consistency; the untouched default; the autograd
node; both hosts; two gloo replicas.  (GPU twin: test_gpu_antialias.py.)"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import antialias_cases as aa
import forward_only_cases as fo
from test_forward_only import SHAPES, small_scene

CPU = torch.device("cpu")
BG = np.array([0.2, 0.5, 0.1], np.float32)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [32, 64 | 8, 64 | fo.FORWARD_ONLY, 32 | 8 | fo.FORWARD_ONLY])
@pytest.mark.parametrize("P,W,H,seed,scale_k", SHAPES)
def test_forward_against_oracle(emu_lib_path, oracle, P, W, H, seed, scale_k, flags):
    cl = small_scene(P, W, H, seed, scale_k)
    aa.check_forward(emu_lib_path, CPU, oracle, cl, cl.cameras[0], BG, flags)


@pytest.mark.parametrize("kw", [dict(raw=True), dict(use_colors_precomp=True), dict(use_cov3D_precomp=True),
                                dict(use_colors_precomp=True, use_cov3D_precomp=True)])
@pytest.mark.parametrize("flags", [32, 64 | 8, 64 | fo.FORWARD_ONLY, 32 | 8 | fo.FORWARD_ONLY])
def test_forward_with_raw_and_precomputed_inputs(emu_lib_path, oracle, flags, kw):
    cl = small_scene(1500, 80, 70, 2)
    aa.check_forward(emu_lib_path, CPU, oracle, cl, cl.cameras[0], BG, flags, **kw)


@pytest.mark.parametrize("P,W,H,seed,scale_k", SHAPES)
def test_restatements_of_h_agree(P, W, H, seed, scale_k):
    """the float32-numpy and the float64 restatement of h, neither the code under test: the gap recorded in antialias_cases.py"""
    cl = small_scene(P, W, H, seed, scale_k)
    gap = aa.restatement_gap(cl, cl.cameras[0])
    print("measured: h32 vs h64 relative L1", gap)
    assert gap <= aa.RESTATEMENT_GAP["factor"] * aa.RESTATEMENT_GAP["h_rel_l1_measured"]


@pytest.mark.parametrize("form", ["0", "1"])   # GSR_BWD_HALF_TILES: quads / half tiles
@pytest.mark.parametrize("maps", [False, True])
@pytest.mark.parametrize("P,W,H,seed,scale_k", [SHAPES[0], SHAPES[2], SHAPES[5]])
def test_backward_against_oracle(emu_lib_path, oracle, monkeypatch, form, maps, P, W, H, seed, scale_k):
    monkeypatch.setenv("GSR_BWD_HALF_TILES", form)
    cl = small_scene(P, W, H, seed, scale_k)
    # (SHAPES[2] is a scene of large splats, h ~ 1: there the h term is below the bars; on the other two its absence would miss them)
    aa.check_backward(emu_lib_path, CPU, oracle, cl, cl.cameras[0], BG, 64, seed=seed, maps=maps,
                      h_term_min=0.0 if scale_k > 1 else 1e-3)


@pytest.mark.parametrize("form", ["0", "1"])
def test_backward_of_sub_pixel_gaussians(emu_lib_path, oracle, monkeypatch, form):
    """a cloud whose Gaussians are mostly smaller than a pixel: the h term is a hundred times the aggregate bar of the position gradient"""
    monkeypatch.setenv("GSR_BWD_HALF_TILES", form)
    cl = small_scene(3000, 64, 48, 9, 0.05)
    aa.check_backward(emu_lib_path, CPU, oracle, cl, cl.cameras[0], BG, 64, seed=9, maps=True, h_term_min=0.01)


@pytest.mark.parametrize("flags", [32, 32 | 8])
def test_backward_depth_first_and_culled_tiles(emu_lib_path, oracle, flags):
    cl = small_scene(1500, 80, 70, 2)
    aa.check_backward(emu_lib_path, CPU, oracle, cl, cl.cameras[0], BG, flags, seed=3, maps=True)


@pytest.mark.parametrize("kw", [dict(use_colors_precomp=True), dict(use_cov3D_precomp=True)])
def test_backward_with_precomputed_inputs(emu_lib_path, oracle, kw):
    """cov3D_precomp: the h term lands in dL_dcov3D"""
    cl = small_scene(1500, 80, 70, 2)
    aa.check_backward(emu_lib_path, CPU, oracle, cl, cl.cameras[0], BG, 32, seed=4, **kw)


def test_backward_refuses_a_mismatched_bit(emu_lib_path):
    cl = small_scene(600, 64, 48, 1)
    aa.check_mismatch_guard(emu_lib_path, CPU, cl, cl.cameras[0], BG)


def test_fused_geom_adam(emu_lib_path):
    cl = small_scene(1500, 80, 70, 2)
    aa.check_fused_geom_adam(emu_lib_path, CPU, cl, cl.cameras[0], BG)


@pytest.mark.parametrize("cov", [False, True])
def test_pose_gradients(emu_lib_path, oracle, cov):
    cl = small_scene(1500, 80, 70, 2)
    aa.check_pose(emu_lib_path, CPU, oracle, cl, cl.cameras[0], BG, cov=cov)


def test_clamp(emu_lib_path, oracle):
    aa.check_clamp(emu_lib_path, CPU, oracle, BG)


def test_energy_of_an_isolated_gaussian(emu_lib_path, oracle):
    aa.check_energy(emu_lib_path, CPU, oracle)


def test_level_consistency(emu_lib_path):
    d_with, d_without, sub, means = aa.level_consistency(emu_lib_path, CPU)
    print("measured: |mean alpha fine - coarse| with the bit", d_with, "without", d_without, "ratio", d_without / max(d_with, 1e-30),
          "sub-pixel share at the coarse level", sub, means)
    assert sub > 0.5, "most Gaussians must be sub-pixel at the coarse level"
    assert d_with < d_without


def test_default_is_untouched(emu_lib_path):
    """the bit clear through the new keyword == the parent's calling convention, hash for hash (image, radii, every gradient), C1 size"""
    from photo_slam_amd import scene
    cl = scene.make_config("C1", seed=0)
    cam = cl.cameras[0]
    new = aa.default_hashes(emu_lib_path, CPU, cl, cam, BG, parent_convention=False)
    old = aa.default_hashes(emu_lib_path, CPU, cl, cam, BG, parent_convention=True)
    assert new == old and len(new) >= 9


def test_autograd_node(emu_lib_path):
    aa.check_autograd(emu_lib_path, CPU, small_scene(600, 64, 48, 1))


def test_python_and_cpp_hosts_agree(emu_lib_path):
    from tests.test_cpp_host import load_host
    aa.check_hosts(load_host("emu"), emu_lib_path, CPU, small_scene(600, 64, 48, 1))


WORKER = r'''
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
import __graft_entry__ as entry
entry.load_package()
from photo_slam_amd import rasterize_points as rp, scene
from photo_slam_amd.gaussian_model import GaussianModel, GaussianOptimizationParams
from photo_slam_amd.gaussian_renderer import GaussianKeyframe, GaussianPipelineParams
from photo_slam_amd.trainer import TrainStep
rp._LIB_OVERRIDE = sys.argv[2]
dist.init_process_group("gloo")
rank, ws = dist.get_rank(), dist.get_world_size()
cl = scene.make_cloud(300, 48, 32, 40.0, 40.0, seed=3, scale_k=0.35, n_views=ws)
opt = GaussianOptimizationParams()
g = GaussianModel.from_cloud(cl, device="cpu"); g.trainingSetup(opt)
kf = GaussianKeyframe.from_camera(cl.cameras[rank], "cpu")
torch.manual_seed(100 + rank); gt = torch.rand(3, 32, 48)
ts = TrainStep(g, opt, GaussianPipelineParams(), torch.zeros(3), world_size=ws, factored_exchange=True,
               cameras_extent=float(cl.extent), seed=7, antialiasing=sys.argv[4] == "1")
for _ in range(3): ts.trainForOneIteration(kf, gt, torch.ones(3, 32, 48))
g.sync_features()
out = {n: p.detach().numpy() for n, p in zip(["xyz","features","opacity","scaling","rotation"], g.params())}
np.savez(os.path.join(sys.argv[3], f"rank{rank}_aa{sys.argv[4]}.npz"), **out)
dist.barrier()
'''


def test_view_factored_exchange_replicas_identical_gloo(emu_lib_path, tmp_path):
    """world size 2, the view-factored exchange, the bit set: replicas bit-identical (the geometry gradients are all-reduced as they
    are), and not the parameters of the run without the bit"""
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    runs = {}
    for aa_on, port in (("1", 29561), ("0", 29563)):
        subprocess.check_call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
                               "127.0.0.1", "--master-port", str(port), str(script), ROOT, emu_lib_path, str(tmp_path), aa_on],
                              env=env, timeout=900)
        runs[aa_on] = [np.load(tmp_path / f"rank{r}_aa{aa_on}.npz") for r in range(2)]
    for k in ("xyz", "features", "opacity", "scaling", "rotation"):
        assert np.array_equal(runs["1"][0][k], runs["1"][1][k]), f"replicas diverged on {k}"
    assert not np.array_equal(runs["1"][0]["xyz"], runs["0"][0]["xyz"]), "the bit did not reach the data-parallel step"
