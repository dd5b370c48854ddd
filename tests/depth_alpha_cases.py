"""Shared checks of the depth and alpha maps (gsr_forward_args.out_depth / out_alpha, gsr_backward_args.dL_ddepth / dL_dalpha,
include/gsr.h) for the emulator tests (test_depth_alpha.py) and the GPU tests (test_gpu_depth_alpha.py).

The CPU oracle serves as the reference unchanged, because the blend is linear in the colours: the depth map is channel 0 of a
render with colours (z, z, z) and no background, the alpha map the same render with colours (1, 1, 1); the gradient of
<dpix, C> + <dD, D> + <dA, A> is the sum of three oracle backward passes (the SH render with dpix, the z render with (dD, 0, 0),
the ones render with (dA, 0, 0)) plus dL/dz (V[2], V[6], V[10]) in dL_dmeans3D, dL/dz = the z render's dL_dcolors[:, 0]."""
import numpy as np
import torch

import forward_only_cases as fo
import parity
from photo_slam_amd import capi
from photo_slam_amd import rasterize_points as rp

GRAD_NAMES = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations")
ROW_CHECKED = ("dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dscales", "dL_drotations")


def view_z(cl, cam):
    """transformPoint4x3(mean, view).z in float32, in its operation order (no contraction)"""
    V = cam.viewmatrix.reshape(-1).astype(np.float32)
    x, y, z = (cl.xyz[:, i].astype(np.float32) for i in range(3))
    return ((V[2] * x + V[6] * y) + V[10] * z) + V[14]


def _np(t):
    return None if t is None or t.numel() == 0 else t.detach().cpu().numpy()


def oracle_forward(oracle, a, cl, cam, colors, bg):
    """one oracle render of the inputs `a` (fo.inputs) with the given per-Gaussian colours and background"""
    cov = _np(a["cov3D_precomp"])
    return oracle.forward(bg, cl.xyz, _np(a["opacity"]).reshape(-1), cam.viewmatrix, cam.projmatrix, cam.campos, cam.tanfovx,
                          cam.tanfovy, cam.H, cam.W, shs=None, sh_degree=3, colors_precomp=np.ascontiguousarray(colors, np.float32),
                          scales=None if cov is not None else _np(a["scales"]), rotations=None if cov is not None else _np(a["rotations"]),
                          cov3D_precomp=cov)


def oracle_maps(oracle, a, cl, cam):
    """(depth, alpha, z) of the oracle"""
    z = view_z(cl, cam)
    P = z.shape[0]
    zero = np.zeros(3, np.float32)
    _, cz, _ = oracle_forward(oracle, a, cl, cam, np.repeat(z[:, None], 3, 1), zero)
    _, c1, _ = oracle_forward(oracle, a, cl, cam, np.ones((P, 3), np.float32), zero)
    return cz[0], c1[0], z


def render(lib_path, a, flags, depth=True, alpha=True, workspace=None):
    """(R, image, radii, depth, alpha, buffers) of one gsr_forward through the Python boundary"""
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        dev = a["means3D"].device
        H, W = a["image_height"], a["image_width"]
        d = torch.full((H, W), -7.0, device=dev) if depth else None   # (every pixel must be written)
        al = torch.full((H, W), -7.0, device=dev) if alpha else None
        R, color, radii, g, b, i = rp.RasterizeGaussiansCUDA(**a, raw_params=flags, out_depth=d, out_alpha=al, workspace=workspace)
        return R, color, radii, d, al, (g, b, i)
    finally:
        rp._LIB_OVERRIDE = prev


def check_forward(lib_path, dev, oracle, cl, cam, bg, flags, **kw):
    """The maps against the oracle; image, radii and instance count bit-identical to the call without them; either map alone is
    the same as both together.  Returns the report."""
    a = fo.inputs(cl, cam, bg, dev, **kw)
    R0, c0, r0, _, _, _ = render(lib_path, a, flags, depth=False, alpha=False)
    R1, c1, r1, d1, al1, _ = render(lib_path, a, flags)
    assert R0 == R1 and torch.equal(c0, c1) and torch.equal(r0, r1), "the maps changed the image, the radii or the instance count"
    _, c2, _, d2, _, _ = render(lib_path, a, flags, alpha=False)
    _, c3, _, _, al3, _ = render(lib_path, a, flags, depth=False)
    assert torch.equal(d1, d2) and torch.equal(al1, al3) and torch.equal(c0, c2) and torch.equal(c0, c3)
    od, oa, z = oracle_maps(oracle, a, cl, cam)
    vis = r0.cpu().numpy() > 0
    zmean = float(z[vis].mean()) if vis.any() else 1.0
    d, al = d1.cpu().numpy(), al1.cpu().numpy()
    rep = dict(depth_L1=float(np.abs(d - od).mean()) / zmean, alpha_L1=float(np.abs(al - oa).mean()), R=R0,
               covered=float((oa > 0).mean()))
    assert rep["depth_L1"] <= parity.RGB_L1_TOL and rep["alpha_L1"] <= parity.RGB_L1_TOL, rep
    assert np.all(al >= 0.0) and np.all(al <= 1.0) and np.all(d[al == 0] == 0), rep
    if flags & fo.FORWARD_ONLY == 0:
        # forward-only and training forms render the same maps, bit for bit
        _, cf, _, df, alf, _ = render(lib_path, a, flags | fo.FORWARD_ONLY)
        assert torch.equal(cf, c0) and torch.equal(df, d1) and torch.equal(alf, al1)
    return rep


def backward(lib_path, a, cam, flags, dpix, dD, dA, raw=0, **bkw):
    """forward (training) + backward with the given upstream gradients (dD / dA None = not passed); returns the tuple of
    RasterizeGaussiansBackwardCUDA and the radii"""
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        R, _, radii, g, b, i = rp.RasterizeGaussiansCUDA(**a, raw_params=flags | raw)
        out = rp.RasterizeGaussiansBackwardCUDA(a["background"], a["means3D"], radii, a["colors"], a["scales"], a["rotations"], 1.0,
                                                a["cov3D_precomp"], a["viewmatrix"], a["projmatrix"], cam.tanfovx, cam.tanfovy, dpix,
                                                a["sh"], 3, a["campos"], g, R, b, i, raw_params=raw, dL_ddepth=dD, dL_dalpha=dA, **bkw)
        if a["means3D"].is_cuda:
            torch.cuda.synchronize()
        return out, radii
    finally:
        rp._LIB_OVERRIDE = prev


def oracle_grads(oracle, a, cl, cam, bg, dpix, dD, dA):
    """oracle gradients of <dpix, C> + <dD, D> + <dA, A> (module docstring)"""
    P = cl.xyz.shape[0]
    colors = _np(a["colors"])
    cov = _np(a["cov3D_precomp"])
    res, _, oradii, g = parity.run_oracle(oracle, cl, cam, bg, dL_dpix=dpix, use_colors_precomp=colors is not None, colors=colors,
                                          use_cov3D_precomp=cov is not None, cov3D=cov)
    g = {k: v.astype(np.float64) for k, v in g.items()}
    z = view_z(cl, cam)
    zero = np.zeros(3, np.float32)
    for is_depth, col, up in ((True, np.repeat(z[:, None], 3, 1), dD), (False, np.ones((P, 3), np.float32), dA)):
        if up is None:
            continue
        r2, _, _ = oracle_forward(oracle, a, cl, cam, col, zero)
        dp = np.zeros((3, cam.H, cam.W), np.float32)
        dp[0] = up
        g2 = oracle.backward(r2, dp)
        for k in ("dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dscales", "dL_drotations"):
            g[k] += g2[k]
        if is_depth:
            V = cam.viewmatrix.reshape(-1).astype(np.float64)
            g["dL_dmeans3D"] += g2["dL_dcolors"][:, :1].astype(np.float64) * np.array([V[2], V[6], V[10]])[None, :]
    return g, oradii


def check_backward(lib_path, dev, oracle, cl, cam, bg, flags, seed=0, use_depth=True, use_alpha=True, **kw):
    """backward with random dpix, dD, dA against the oracle: aggregate rel-L1 and the per-row bars"""
    rng = np.random.default_rng(seed)
    a = fo.inputs(cl, cam, bg, dev, **kw)
    dpix = rng.standard_normal((3, cam.H, cam.W)).astype(np.float32)
    dD = rng.standard_normal((cam.H, cam.W)).astype(np.float32) if use_depth else None
    dA = rng.standard_normal((cam.H, cam.W)).astype(np.float32) if use_alpha else None
    t = lambda x: None if x is None else fo._t(x, dev)
    out, radii = backward(lib_path, a, cam, flags, t(dpix), t(dD), t(dA))
    ref, oradii = oracle_grads(oracle, a, cl, cam, bg, dpix, dD, dA)
    assert np.array_equal(radii.cpu().numpy(), oradii)
    vis = oradii > 0
    rep = {}
    for name, gt in zip(GRAD_NAMES, out):
        if gt is None or gt.numel() == 0 or name not in ref or not np.abs(ref[name]).sum():
            continue
        g = gt.cpu().numpy()
        assert np.isfinite(g).all(), name
        rep[name] = parity.rel_l1(g, ref[name])
        assert rep[name] <= parity.GRAD_REL_L1_TOL, (name, rep)
        assert not np.any(g.reshape(g.shape[0], -1)[~vis]), f"{name} non-zero on culled Gaussians"
        if name in ROW_CHECKED:
            e = parity.row_errors(g, ref[name])[vis]
            row = dict(p9999=float(np.quantile(e, 0.9999)), max=float(e.max()), beyond=int((e > parity.ROW_OUTLIER).sum()))
            rep["rows_" + name] = row
            assert row["p9999"] <= parity.ROW_P9999_TOL and row["max"] <= parity.ROW_MAX_TOL, (name, row)
            assert row["beyond"] <= max(3, parity.ROW_OUTLIER_FRAC * e.size), (name, row)
    return rep


def check_zero_upstream(lib_path, dev, cl, cam, bg, flags, exact=True, seed=0, **kw):
    """dD = dA = 0 passed as tensors: the gradients of the plain backward (equal on the emulator, to rounding on the device)"""
    rng = np.random.default_rng(seed)
    a = fo.inputs(cl, cam, bg, dev, **kw)
    dpix = fo._t(rng.standard_normal((3, cam.H, cam.W)).astype(np.float32), dev)
    zero = torch.zeros((cam.H, cam.W), device=dev)
    plain, _ = backward(lib_path, a, cam, flags, dpix, None, None)
    with_zero, _ = backward(lib_path, a, cam, flags, dpix, zero, zero.clone())
    for name, x, y in zip(GRAD_NAMES, plain, with_zero):
        if x is None or x.numel() == 0:
            continue
        if exact:
            assert torch.equal(x, y), name
        else:
            assert parity.rel_l1(y.cpu().numpy(), x.cpu().numpy()) <= 1e-5, name


def check_fused_geom_adam(lib_path, dev, cl, cam, bg, seed=0):
    """raw_params = 7 + geom_adam with a depth gradient: the parameters after the fused step match the unfused gradients +
    gsr_adam_step, to the bar of parity.check_fused_geom_adam"""
    lib = capi.load(lib_path)
    rng = np.random.default_rng(seed)
    P = cl.xyz.shape[0]
    raw = capi.RAW_OPACITY | capi.RAW_SCALING | capi.RAW_ROTATION
    dpix = fo._t(rng.standard_normal((3, cam.H, cam.W)).astype(np.float32), dev)
    dD = fo._t(rng.standard_normal((cam.H, cam.W)).astype(np.float32), dev)
    dA = fo._t(rng.standard_normal((cam.H, cam.W)).astype(np.float32), dev)
    names = ("xyz", "opacity", "scaling", "rotation")
    init = dict(xyz=cl.xyz, opacity=cl.opacity.reshape(P, 1), scaling=cl.scaling, rotation=cl.rotation)
    lrs = dict(xyz=1.6e-4, opacity=0.05, scaling=0.005, rotation=0.001)
    steps = dict(xyz=4, opacity=2, scaling=4, rotation=7)
    mom = {n: ((0.01 * rng.standard_normal(init[n].shape)).astype(np.float32), (1e-4 * rng.random(init[n].shape)).astype(np.float32))
           for n in names}

    def run(fused):
        st = {n: [fo._t(init[n].copy(), dev).clone(), fo._t(mom[n][0].copy(), dev).clone(), fo._t(mom[n][1].copy(), dev).clone()]
              for n in names}
        a = fo.inputs(cl, cam, bg, dev)
        a.update(means3D=st["xyz"][0], opacity=st["opacity"][0], scales=st["scaling"][0], rotations=st["rotation"][0])
        ga = dict(tensors=[(st[n][0], st[n][1], st[n][2], lrs[n], steps[n]) for n in names], beta1=0.9, beta2=0.999,
                  eps=1e-15) if fused else None
        out, radii = backward(lib_path, a, cam, 0, dpix, dD, dA, raw=raw, geom_adam=ga, training_outputs_only=fused)
        return st, out, radii.cpu().numpy()

    st_ref, g_ref, radii = run(False)
    grads = dict(xyz=g_ref[3], opacity=g_ref[2], scaling=g_ref[6], rotation=g_ref[7])
    for n in names:
        p_, m_, v_ = st_ref[n]
        gr = grads[n].contiguous()
        capi.check(lib, lib.gsr_adam_step(p_.data_ptr(), gr.data_ptr(), m_.data_ptr(), v_.data_ptr(), p_.numel(), lrs[n], 0.9, 0.999,
                                          1e-15, steps[n], 0, 0, lrs[n], None), "gsr_adam_step")
    if dev.type != "cpu":
        torch.cuda.synchronize()
    st_fus, _, _ = run(True)
    exact = dev.type == "cpu"
    vis = radii > 0
    assert vis.any()
    for n in names:
        for k in range(3):
            x, y = st_fus[n][k].cpu().numpy(), st_ref[n][k].cpu().numpy()
            tol = max(lrs[n] * (2e-6 if exact else 2e-3), 1.2e-7 * np.abs(y).max()) if k == 0 else (1e-6 if exact else 2e-4) * np.abs(y).max()
            assert np.abs(x - y).max() <= tol, (n, k, np.abs(x - y).max(), tol)
    # the depth term reached the xyz step: without it the positions would have moved differently
    assert float(grads["xyz"].abs().sum()) > 0


def depth_loss_reference(depth, gt, w, lo, hi):
    """the torch expression of gsr_depth_l1_loss: (loss, gradient)"""
    with torch.enable_grad():
        d = depth.detach().clone().requires_grad_(True)
        valid = (gt > lo) & (gt < hi)
        H, W = d.shape
        loss = w * ((d - gt).abs() * valid).sum() / (H * W)
        loss.backward()
    return loss.detach(), d.grad


def check_depth_loss(dev, H=37, W=53, seed=0, w=0.7, lo=0.1, hi=5.0):
    from photo_slam_amd import loss_utils
    rng = np.random.default_rng(seed)
    gt = rng.uniform(0.0, 6.0, (H, W)).astype(np.float32)
    gt[0, :4] = [lo, hi, 0.0, np.nextafter(np.float32(lo), np.float32(1))]   # on the bounds (invalid), 0, just inside
    depth = gt + rng.standard_normal((H, W)).astype(np.float32)
    depth[1, :6] = gt[1, :6]                                   # D == gt: sign 0
    gt_t, d_t = fo._t(gt, dev), fo._t(depth, dev).requires_grad_(True)
    loss = loss_utils.depth_l1_loss(d_t, gt_t, w, lo, hi)
    loss.backward()
    ref_loss, ref_grad = depth_loss_reference(fo._t(depth, dev), gt_t, w, lo, hi)
    assert abs(loss.item() - ref_loss.item()) <= 1e-6 * abs(ref_loss.item()) + 1e-7, (loss.item(), ref_loss.item())
    assert torch.allclose(d_t.grad, ref_grad, rtol=1e-6, atol=0), float((d_t.grad - ref_grad).abs().max())
    assert torch.equal(d_t.grad == 0, ref_grad == 0)
    assert float(d_t.grad[0, 0]) == 0 and float(d_t.grad[0, 1]) == 0 and float(d_t.grad[1, 0]) == 0
    # deterministic: the same bits again
    loss2 = loss_utils.depth_l1_loss(d_t.detach(), gt_t, w, lo, hi)
    assert loss2.item() == loss.item()


def _settings(cl, cam, dev, render_depth=True, forward_only=False):
    from photo_slam_amd.gaussian_rasterizer import GaussianRasterizationSettings
    t = lambda x: fo._t(x, dev)
    return GaussianRasterizationSettings(cam.H, cam.W, cam.tanfovx, cam.tanfovy, t(np.array([0.2, 0.5, 0.1], np.float32)), 1.0,
                                         t(cam.viewmatrix), t(cam.projmatrix), 3, t(cam.campos), False,
                                         forward_only_=forward_only, render_depth_=render_depth)


def check_autograd(dev, cl):
    """A loss on depth alone, and one on alpha alone, back-propagates through GaussianRasterizer (settings.render_depth_) to the
    gradients of the direct backward call; under torch.no_grad() the maps equal the training forward's bit for bit"""
    from photo_slam_amd.gaussian_rasterizer import GaussianRasterizer
    cam = cl.cameras[0]
    rng = np.random.default_rng(5)
    w = fo._t(rng.standard_normal((cam.H, cam.W)).astype(np.float32), dev)

    def leaves():
        t = lambda x: fo._t(x, dev).clone().requires_grad_(True)
        return dict(means3D=t(cl.xyz), means2D=torch.zeros((cl.xyz.shape[0], 3), device=dev, requires_grad=True),
                    opacities=t(cl.get_opacity()), shs=t(cl.get_features()), scales=t(cl.get_scaling()),
                    rotations=t(cl.get_rotation()))

    def run(which):
        L = leaves()
        r = GaussianRasterizer(_settings(cl, cam, dev))
        color, radii, depth, alpha = r(L["means3D"], L["means2D"], L["opacities"], True, False, True, True, False, shs=L["shs"],
                                       scales=L["scales"], rotations=L["rotations"])
        assert depth.requires_grad and alpha.requires_grad and depth.shape == (cam.H, cam.W)
        ((depth if which == "depth" else alpha) * w).sum().backward()
        return L, (color.detach(), radii, depth.detach(), alpha.detach())

    for which in ("depth", "alpha"):
        L, outs = run(which)
        a = fo.inputs(cl, cam, np.array([0.2, 0.5, 0.1], np.float32), dev)
        zero = torch.zeros((3, cam.H, cam.W), device=dev)
        ref, _ = backward(None if dev.type != "cpu" else rp._LIB_OVERRIDE, a, cam, 0, zero, w if which == "depth" else None,
                          w if which == "alpha" else None)
        got = dict(dL_dmeans3D=L["means3D"].grad, dL_dmeans2D=L["means2D"].grad, dL_dopacity=L["opacities"].grad,
                   dL_dscales=L["scales"].grad, dL_drotations=L["rotations"].grad, dL_dsh=L["shs"].grad)
        for name, g in zip(GRAD_NAMES, ref):
            if name not in got:
                continue
            x = got[name]
            assert x is not None and torch.isfinite(x).all(), name
            if dev.type == "cpu":
                assert torch.equal(x.reshape(g.shape), g), (which, name)
            else:
                assert parity.rel_l1(x.reshape(g.shape).cpu().numpy(), g.cpu().numpy()) <= 1e-5, (which, name)
        assert float(L["means3D"].grad.abs().sum()) > 0 and float(L["shs"].grad.abs().sum()) == 0
        # the no-grad path renders the same maps (forward-only)
        with torch.no_grad():
            L2 = leaves()
            c2, r2, d2, a2 = GaussianRasterizer(_settings(cl, cam, dev))(L2["means3D"], L2["means2D"], L2["opacities"], True, False,
                                                                          True, True, False, shs=L2["shs"], scales=L2["scales"],
                                                                          rotations=L2["rotations"])
        assert rp.lastForwardOnly() == 1
        assert torch.equal(c2, outs[0]) and torch.equal(r2, outs[1]) and torch.equal(d2, outs[2]) and torch.equal(a2, outs[3])


def _python_trainer(cl, dev, weight=0.0, lo=0.1, hi=100.0):
    import copy
    from photo_slam_amd.gaussian_model import GaussianModel, GaussianOptimizationParams
    from photo_slam_amd.gaussian_renderer import GaussianPipelineParams
    from photo_slam_amd.trainer import TrainStep
    g = GaussianModel.from_cloud(copy.deepcopy(cl), device=dev)
    opt = GaussianOptimizationParams()
    g.trainingSetup(opt)
    ts = TrainStep(g, opt, GaussianPipelineParams(), torch.zeros(3, device=dev), cameras_extent=float(cl.extent), seed=7)
    ts.depth_loss_weight_, ts.depth_min_, ts.depth_max_ = weight, lo, hi
    return g, ts


def train_data(cl, dev, seed=0):
    """(keyframes, gt images, gt depths, mask) for the cloud's cameras: the sensor depth is the oracle-free expected depth of the
    initial model, perturbed, with holes"""
    from photo_slam_amd.gaussian_renderer import GaussianKeyframe
    torch.manual_seed(seed)
    cams = cl.cameras
    kfs = [GaussianKeyframe.from_camera(c, dev) for c in cams]
    gts = [torch.rand(3, c.H, c.W).to(dev) for c in cams]
    rng = np.random.default_rng(seed)
    depths = []
    for c in cams:
        z = rng.uniform(1.0, 8.0, (c.H, c.W)).astype(np.float32)
        z[rng.random((c.H, c.W)) < 0.1] = 0.0   # holes: invalid
        depths.append(fo._t(z, dev))
    return kfs, gts, depths, torch.ones(3, cams[0].H, cams[0].W, device=dev)


def check_train_step_python(dev, cl, steps=5, exact=True):
    """weight 0 with gt_depth == no gt_depth bit for bit (exact: the emulator; on the device two runs of the same program differ in
    the last bits of a gradient -- the first step's loss, a forward quantity, is still compared bit for bit); with weight > 0 the
    loss is the RGB loss plus the torch-formed depth loss of the same render, and the parameters move differently"""
    from photo_slam_amd import loss_utils
    from photo_slam_amd.gaussian_renderer import GaussianRenderer
    kfs, gts, depths, mask = train_data(cl, dev)
    n = len(kfs)
    runs, first = [], []
    for with_depth in (False, True):
        g, ts = _python_trainer(cl, dev, weight=0.0)
        for it in range(steps):
            l = ts.trainForOneIteration(kfs[it % n], gts[it % n], mask, sync_loss=False, gt_depth=depths[it % n] if with_depth else None)
            if it == 0:
                first.append(l.item())
        runs.append([p.detach().clone() for p in g.params()])
    assert first[0] == first[1]
    for x, y in zip(*runs):
        if exact:
            assert torch.equal(x, y), "depth_loss_weight_ = 0 with gt_depth changed the trajectory"
        else:
            assert parity.rel_l1(y.cpu().numpy(), x.cpu().numpy()) <= 1e-3
    # weight > 0: the loss of the first step against the torch expression on the same render
    w, lo, hi = 0.3, 0.5, 6.0
    g, ts = _python_trainer(cl, dev, weight=w, lo=lo, hi=hi)
    with torch.no_grad():
        img, _, _, _, depth, alpha = GaussianRenderer.render(kfs[0], kfs[0].image_height_, kfs[0].image_width_, g, ts.pipe_, ts.background_,
                                                             render_depth=True)
        rgb = loss_utils.fused_l1_ssim_loss(img, gts[0], None, ts.opt_.lambda_dssim_)
        dl, _ = depth_loss_reference(depth, depths[0], w, lo, hi)
    loss = ts.trainForOneIteration(kfs[0], gts[0], mask, sync_loss=False, gt_depth=depths[0])
    want = rgb.item() + dl.item()
    assert abs(loss.item() - want) <= 2e-6 * abs(want), (loss.item(), want, rgb.item(), dl.item())
    assert float(dl) > 0
    for it in range(1, steps):
        ts.trainForOneIteration(kfs[it % n], gts[it % n], mask, sync_loss=False, gt_depth=depths[it % n])
    moved = [p.detach() for p in g.params()]
    assert not torch.equal(moved[0], runs[0][0]), "the depth loss did not reach the positions"
    # render_view with depth: (image, depth, alpha), forward-only
    img, d, a = ts.render_view(kfs[0], with_depth=True)
    assert d.shape == (kfs[0].image_height_, kfs[0].image_width_) and a.shape == d.shape and rp.lastForwardOnly() == 1
    return [p.detach().clone() for p in g.params()]


def _cam_args(c, dev):
    import math
    t = lambda x: fo._t(x, dev)
    return (t(c.viewmatrix), t(c.projmatrix), t(c.campos), 2 * math.atan(c.tanfovx), 2 * math.atan(c.tanfovy), c.H, c.W)


def _cpp_trainer(ops, cl, dev, weight=0.0, lo=0.1, hi=100.0):
    import copy
    from photo_slam_amd.gaussian_model import GaussianModel
    g0 = GaussianModel.from_cloud(copy.deepcopy(cl), device=dev)
    h = ops.trainer_create(g0.xyz_.detach(), g0.features_.detach(), g0.opacity_.detach(), g0.scaling_.detach(), g0.rotation_.detach(),
                           3, float(cl.extent), torch.zeros(3, device=dev))
    ops.trainer_set_options(h, {"seed": 7.0, "cameras_extent": float(cl.extent), "depth_loss_weight": float(weight),
                                "depth_min": float(lo), "depth_max": float(hi)})
    return h


def check_train_step_cpp(ops, lib_path, dev, cl, steps=5, exact=True):
    """The C++ host (TrainStep::renderAndBackward with gt_depth, op trainer_render_and_backward_depth): weight 0 with gt_depth ==
    no gt_depth (bit for bit on the emulator; the first step's loss on the device); with weight > 0 the loss of a step is the RGB
    loss plus the torch-formed depth loss of the same render (renderViewWithDepth), and the positions move differently"""
    from photo_slam_amd import loss_utils
    kfs, gts, depths, mask = train_data(cl, dev)
    cams = [_cam_args(c, dev) for c in cl.cameras]
    n = len(cams)
    runs, first = [], []
    for with_depth in (False, True):
        h = _cpp_trainer(ops, cl, dev)
        try:
            for it in range(steps):
                if with_depth:
                    l = ops.trainer_render_and_backward_depth(h, *cams[it % n], gts[it % n], mask, depths[it % n])
                else:
                    l = ops.trainer_render_and_backward(h, *cams[it % n], gts[it % n], mask)
                ops.trainer_finish(h)
                if it == 0:
                    first.append(l.item())
            runs.append([p.detach().clone() for p in ops.trainer_params(h)])
        finally:
            ops.trainer_destroy(h)
    assert first[0] == first[1]
    for x, y in zip(*runs):
        assert torch.equal(x, y) if exact else parity.rel_l1(y.cpu().numpy(), x.cpu().numpy()) <= 1e-3
    w, lo, hi = 0.3, 0.5, 6.0
    h = _cpp_trainer(ops, cl, dev, w, lo, hi)
    try:
        img, depth, alpha = ops.trainer_render_view_depth(h, *cams[0])
        assert img.grad_fn is None and depth.shape == (cl.cameras[0].H, cl.cameras[0].W) and alpha.shape == depth.shape
        assert float(alpha.min()) >= 0 and float(alpha.max()) <= 1 and float(depth.abs().sum()) > 0
        prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
        try:
            with torch.no_grad():
                rgb = loss_utils.fused_l1_ssim_loss(img, gts[0], None, 0.2)
        finally:
            rp._LIB_OVERRIDE = prev
        dl, _ = depth_loss_reference(depth, depths[0], w, lo, hi)
        loss = ops.trainer_render_and_backward_depth(h, *cams[0], gts[0], mask, depths[0])
        ops.trainer_finish(h)
        want = rgb.item() + dl.item()
        assert abs(loss.item() - want) <= 2e-6 * abs(want), (loss.item(), want, rgb.item(), dl.item())
        for it in range(1, steps):
            ops.trainer_render_and_backward_depth(h, *cams[it % n], gts[it % n], mask, depths[it % n])
            ops.trainer_finish(h)
        assert not torch.equal(ops.trainer_params(h)[0], runs[0][0]), "the depth loss did not reach the positions"
    finally:
        ops.trainer_destroy(h)


def check_train_step_hosts(ops, lib_path, dev, cl, steps=3, exact=True):
    """C++ and Python hosts with the depth loss (weight > 0) agree on the parameters after `steps` steps (the bar of the colour
    train step's cross-host check, tests/test_cpp_host.py)"""
    kfs, gts, depths, mask = train_data(cl, dev)
    cams = [_cam_args(c, dev) for c in cl.cameras]
    n = len(cams)
    w, lo, hi = 0.3, 0.5, 6.0
    h = _cpp_trainer(ops, cl, dev, w, lo, hi)
    try:
        losses_cpp = []
        for it in range(steps):
            losses_cpp.append(ops.trainer_render_and_backward_depth(h, *cams[it % n], gts[it % n], mask, depths[it % n]).item())
            ops.trainer_finish(h)
        cpp = [p.detach().clone() for p in ops.trainer_params(h)]
    finally:
        ops.trainer_destroy(h)
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        g, ts = _python_trainer(cl, dev, weight=w, lo=lo, hi=hi)
        losses_py = [ts.trainForOneIteration(kfs[it % n], gts[it % n], mask, sync_loss=False, gt_depth=depths[it % n]).item()
                     for it in range(steps)]
        g.sync_features()   # (lazy SH Adam: the rows that are behind catch up while the same library is selected)
    finally:
        rp._LIB_OVERRIDE = prev
    assert np.allclose(losses_cpp, losses_py, rtol=1e-5), (losses_cpp, losses_py)
    for a, b in zip(cpp, g.params()):
        if exact:
            assert torch.allclose(a, b.detach(), rtol=1e-4, atol=1e-6)
        else:
            assert parity.rel_l1(a.cpu().numpy(), b.detach().cpu().numpy()) <= 1e-3


def check_train_step_fused_unfused(dev, cl, steps=3, exact=True):
    """The depth loss through the fused optimizer steps (SH and geometry Adam inside backward: dL/dz reaches the xyz step inside
    preprocess_bwd) against the dense path (autograd gradients of the four tensors + the separate Adam steps): the same
    parameters after `steps` steps, to the bar of parity.check_fused_geom_adam per step"""
    kfs, gts, depths, mask = train_data(cl, dev)
    n = len(kfs)
    out = []
    for fused in (True, False):
        g, ts = _python_trainer(cl, dev, weight=0.3, lo=0.5, hi=6.0)
        init = [p.detach().clone() for p in g.params()]
        ts.fused_geom_adam_ = ts.fused_sh_adam_ = fused
        for it in range(steps):
            ts.trainForOneIteration(kfs[it % n], gts[it % n], mask, sync_loss=False, gt_depth=depths[it % n])
        g.sync_features()
        out.append([p.detach() - p0 for p, p0 in zip(g.params(), init)])   # (the steps taken: a missing term shows in full)
    for a, b in zip(*out):
        assert float(b.abs().sum()) > 0
        err = parity.rel_l1(a.cpu().numpy(), b.cpu().numpy())
        assert err <= (1e-5 if exact else 1e-3), err
