"""Absolute screen-space gradients through the hosts: the autograd functions of both hosts hand out the [P,2] array of the C-ABI
(Python: `.absgrad` on the viewspace tensor, as upstream; C++: GaussianRasterizationExtensions::absgrad_), the Python and the C++
TrainStep with absgrad_ agree over six steps with one densification, the fused statistics equal the separate pass, and
densifyAndPrune takes densify_abs_grad_threshold_ with the switch on.  Emulator build here, the MI355X at C1 with 2 000 Gaussians
in the gpu-marked twin."""
import copy
import math

import numpy as np
import pytest
import torch

import absgrad_cases as ac
import forward_only_cases as fo
import parity
import pose_grad_cases as pg
from photo_slam_amd import rasterize_points as rp
from photo_slam_amd import scene
from photo_slam_amd.gaussian_model import GaussianModel, GaussianOptimizationParams
from photo_slam_amd.gaussian_rasterizer import GaussianRasterizationSettings, GaussianRasterizer
from photo_slam_amd.gaussian_renderer import GaussianKeyframe, GaussianPipelineParams, GaussianRenderer
from photo_slam_amd.trainer import TrainStep
from test_cpp_host import load_host

BG = ac.BG


def _cam_args(c, dev):
    t = lambda x: fo._t(x, dev)
    return (t(c.viewmatrix), t(c.projmatrix), t(c.campos), 2 * math.atan(c.tanfovx), 2 * math.atan(c.tanfovy), c.H, c.W)


def check_autograd_paths(ops, dev, lib_path, cl, exact):
    """`.absgrad` of the Python autograd path and absgrad_ of the C++ one == the C-ABI output"""
    cam = cl.cameras[0]
    P = cl.xyz.shape[0]
    dpix = np.random.default_rng(2).standard_normal((3, cam.H, cam.W)).astype(np.float32)
    out, _, direct = ac.run(lib_path, dev, cl, cam, 0, dpix)
    t = lambda x: fo._t(x, dev)
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        s = GaussianRasterizationSettings(cam.H, cam.W, cam.tanfovx, cam.tanfovy, t(BG), 1.0, t(cam.viewmatrix), t(cam.projmatrix), 3,
                                          t(cam.campos), False, absgrad_=True)
        leaf = lambda x: t(x).clone().requires_grad_(True)
        means2D = torch.zeros((P, 3), device=dev, requires_grad=True)
        color, _ = GaussianRasterizer(s)(leaf(cl.xyz), means2D, leaf(cl.get_opacity()), True, False, True, True, False,
                                         shs=leaf(cl.get_features()), scales=leaf(cl.get_scaling()), rotations=leaf(cl.get_rotation()))
        assert not hasattr(means2D, "absgrad")
        (color * t(dpix)).sum().backward()
    finally:
        rp._LIB_OVERRIDE = prev
    assert means2D.absgrad.shape == (P, 2)
    pg.same_or_rerun_close("means2D.absgrad", means2D.absgrad, direct, exact)
    pg.same_or_rerun_close("means2D.grad", means2D.grad, out[0], exact)
    ac.check_bound(means2D.absgrad.cpu().numpy(), means2D.grad.cpu().numpy())
    e = torch.empty(0, device=dev)
    m2 = torch.zeros((P, 3), device=dev, requires_grad=True)
    ab = torch.full((P, 2), float("nan"), device=dev)
    color, _ = ops.rasterize_gaussians_absgrad(leaf(cl.xyz), m2, leaf(cl.get_features()), e, leaf(cl.get_opacity()), leaf(cl.get_scaling()),
                                               leaf(cl.get_rotation()), e, t(BG), 1.0, t(cam.viewmatrix), t(cam.projmatrix), cam.tanfovx,
                                               cam.tanfovy, cam.H, cam.W, 3, t(cam.campos), 0, ab)
    (color * t(dpix)).sum().backward()
    pg.same_or_rerun_close("absgrad_ (C++)", ab, direct, exact)
    pg.same_or_rerun_close("means2D.grad (C++)", m2.grad, out[0], exact)


def _trainers(ops, dev, cl, options):
    """(C++ handle, Python model, Python TrainStep) with the same options (keys of trainer_set_options)"""
    g = GaussianModel.from_cloud(copy.deepcopy(cl), device=dev)
    bg = torch.zeros(3, device=dev)
    h = ops.trainer_create(g.xyz_.detach(), g.features_.detach(), g.opacity_.detach(), g.scaling_.detach(), g.rotation_.detach(), 3,
                           float(cl.extent), bg)
    ops.trainer_set_options(h, dict({"densify": 1.0, "cameras_extent": float(cl.extent), "seed": 7.0, "densify_from_iter": 1.0,
                                     "densification_interval": 4.0, "opacity_reset_interval": 3000.0}, **options))
    opt = GaussianOptimizationParams()
    opt.densify_from_iter_, opt.densification_interval_ = 1, 4
    g.trainingSetup(opt)
    ts = TrainStep(g, opt, GaussianPipelineParams(), bg, cameras_extent=float(cl.extent), densify=True, seed=7)
    ts.absgrad_ = bool(options.get("absgrad", 0.0))
    if "densify_abs_grad_threshold" in options:
        ts.densify_abs_grad_threshold_ = options["densify_abs_grad_threshold"]
    return h, g, ts


def check_train_step_hosts(ops, dev, lib_path, cl, exact):
    """six steps, densification at the fourth: the hosts agree (the bars of test_cpp_host.run_densify_schedule_checks); the fused
    statistics of the first step equal the separate pass on that step's array"""
    cams = cl.cameras
    torch.manual_seed(0)
    gts = [torch.rand(3, c.H, c.W).to(dev) for c in cams]
    mask = torch.ones(3, cams[0].H, cams[0].W, device=dev)
    kfs = [GaussianKeyframe.from_camera(c, dev) for c in cams]
    # (a threshold the scene's random images reach: the step must split or clone something)
    h, g, ts = _trainers(ops, dev, cl, {"absgrad": 1.0, "densify_abs_grad_threshold": 2e-5})
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        assert ops.trainer_last_absgrad(h).shape == (0, 2)
        for it in range(1, 7):
            k = (it - 1) % len(cams)
            if it == 1:   # the separate statistics pass on a twin model: render with absgrad, then addViewStats
                g2 = GaussianModel.from_cloud(copy.deepcopy(cl), device=dev)
                from photo_slam_amd import loss_utils
                img, vsp, _, radii = GaussianRenderer.render(kfs[k], cams[k].H, cams[k].W, g2, GaussianPipelineParams(), torch.zeros(3, device=dev),
                                                             absgrad=True)
                loss_utils.fused_l1_ssim_loss(img, gts[k], None, 0.2, is_root=True).backward()
                g2.addViewStats(vsp, radii, absgrad=vsp.absgrad)
            l_py = float(ts.trainForOneIteration(kfs[k], gts[k], mask))
            l_cpp = float(ops.trainer_render_and_backward(h, *_cam_args(cams[k], dev), gts[k], mask))
            if it == 1:
                for name, a, b, c in zip(("accum", "denom", "max_radii"), ops.trainer_stats(h), (g.xyz_gradient_accum_, g.denom_, g.max_radii2D_),
                                         (g2.xyz_gradient_accum_, g2.denom_, g2.max_radii2D_)):
                    # (the two hosts form the image gradient with their own loss code: exact=False, as the depth tests compare them)
                    pg.same_or_rerun_close("fused statistics, C++ against Python: " + name, a.reshape(-1), b.reshape(-1), False)
                    pg.same_or_rerun_close("fused against separate statistics: " + name, b.reshape(-1), c.reshape(-1), exact)
                ab = ops.trainer_last_absgrad(h)
                assert ab.shape == (cl.xyz.shape[0], 2) and bool((ab >= 0).all())
                norm = ab.norm(dim=1)
                pg.same_or_rerun_close("the statistic is the norm of the pair", ops.trainer_stats(h)[0].reshape(-1), norm * (norm > 0), False)
            ops.trainer_finish(h)
            assert np.isclose(l_py, l_cpp, rtol=2e-4), (it, l_py, l_cpp)
            assert ops.trainer_params(h)[0].shape == g.xyz_.shape, it
            if it == 4:
                d = ts.last_densify_
                assert list(ops.trainer_last_densify(h)) == [d["cloned"], d["split"], d["pruned"], d["points"]], it
                assert d["cloned"] + d["split"] > 0, d
        for a, b in zip(ops.trainer_params(h), g.params()):
            if exact:
                assert torch.allclose(a, b.detach(), rtol=1e-3, atol=1e-5)
            else:
                assert parity.rel_l1(a.detach().cpu().numpy(), b.detach().cpu().numpy()) <= 1e-3
    finally:
        rp._LIB_OVERRIDE = prev
        ops.trainer_destroy(h)


def check_threshold_switch(ops, dev, lib_path, cl):
    """hand-built accumulators, mean statistic per Gaussian: 1e-4 (a signed norm below densify_grad_threshold_ = 0.0002) is not
    densified with the switch off, 1e-3 (an absolute norm above densify_abs_grad_threshold_ = 0.0008) is with it on; and 5e-4,
    between the two defaults, is densified by the signed threshold only"""
    cam = cl.cameras[0]
    torch.manual_seed(0)
    gt = torch.rand(3, cam.H, cam.W).to(dev)
    mask = torch.ones(3, cam.H, cam.W, device=dev)
    kf = GaussianKeyframe.from_camera(cam, dev)
    want = {(0.0, 1e-4): False, (1.0, 1e-3): True, (0.0, 5e-4): True, (1.0, 5e-4): False}
    for (switch, mean), grows in want.items():
        h, g, ts = _trainers(ops, dev, cl, {"absgrad": switch, "densification_interval": 1.0, "densify_from_iter": 0.0})
        ts.opt_.densification_interval_, ts.opt_.densify_from_iter_ = 1, 0
        assert ts.densify_abs_grad_threshold_ == 0.0008 and ts.opt_.densify_grad_threshold_ == 0.0002
        prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
        try:
            denom = 1.0e6   # (this step's own view adds one observation in a million to the hand-built mean)
            for stats in (ops.trainer_stats(h), (g.xyz_gradient_accum_, g.denom_, g.max_radii2D_)):
                stats[0].fill_(mean * denom)
                stats[1].fill_(denom)
            ts.trainForOneIteration(kf, gt, mask)
            ops.trainer_render_and_backward(h, *_cam_args(cam, dev), gt, mask)
            ops.trainer_finish(h)
            d = ts.last_densify_
            assert (d["cloned"] + d["split"] > 0) == grows, (switch, mean, d)
            assert list(ops.trainer_last_densify(h)) == [d["cloned"], d["split"], d["pruned"], d["points"]], (switch, mean)
        finally:
            rp._LIB_OVERRIDE = prev
            ops.trainer_destroy(h)


def test_autograd_paths_hand_out_the_c_abi_array(emu_lib_path):
    check_autograd_paths(load_host("emu"), torch.device("cpu"), emu_lib_path, scene.make_cloud(300, 48, 32, 30, 30, seed=1), exact=True)


def test_train_step_of_both_hosts(emu_lib_path):
    check_train_step_hosts(load_host("emu"), torch.device("cpu"), emu_lib_path,
                           scene.make_cloud(300, 48, 32, 40.0, 40.0, seed=3, scale_k=0.35, n_views=2), exact=True)


def test_threshold_follows_the_switch(emu_lib_path):
    check_threshold_switch(load_host("emu"), torch.device("cpu"), emu_lib_path, scene.make_cloud(250, 48, 32, 40.0, 40.0, seed=3, scale_k=0.35))


@pytest.mark.gpu
def test_hosts_at_c1_on_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    ops, dev = load_host("hip"), torch.device("cuda:0")
    cl = scene.make_config("C1", seed=1, n_views=2, P=2000)
    check_autograd_paths(ops, dev, None, cl, exact=False)
    check_train_step_hosts(ops, dev, None, cl, exact=False)
    check_threshold_switch(ops, dev, None, cl)
