"""Shared checks of the opacity / scale / isotropy regularisers inside the backward pass (gsr_backward_args.geom_reg, include/gsr.h)
for the emulator tests (test_geom_reg.py), the GPU tests (test_gpu_geom_reg.py) and the C++ host's (test_cpp_host_geom_reg.py).

The reference is reference() below: a float64 evaluation of the definitions in include/gsr.h on the fp32 inputs the kernel sees
(the weights as the fp32 values the struct carries).  It shares no code with the kernels.

Bars:
  * the term alone (dL_dpix = 0): element-wise relative REG_TOL = 1e-5 on the visible rows -- a handful of fp32 roundings of exp,
    sigmoid and two or three multiplies, nothing cancels.  The scenes keep the logits in [-3, 3], so that 1 - sigmoid(x) >= 0.047
    and the rounding of sigmoid (6e-8) is at most 1.3e-6 of o (1 - o); under GSR_ANTIALIAS the activated opacity is recovered from
    the record with two more roundings (at most 4e-6).  Culled rows and every other output: exactly 0.
  * added to a real gradient g: on the emulator |out - (g + r)| <= 2^-23 |g + r| + REG_TOL |r| (one fp32 rounding of the sum, r to
    its own bar), every other output bit-identical; on the device parity.GRAD_REL_L1_TOL = 1e-4 of the L1 mass, the other outputs to
    the rerun bar of pose_grad_cases (the parent's backward pass is not bit-reproducible there, pose_grad_cases.py:137).
  * the three loss values: relative REG_TOL of the float64 sums (non-negative terms, 128-wide fp32 partials, then a double
    accumulation); a rerun and the other binning arrangement give the same bits, on the emulator and on the device (the sums read
    only the forward pass's record and the inputs, both deterministic).
  * the fused step: the bar of parity.check_fused_geom_adam."""
import copy
import ctypes as C

import numpy as np
import torch

import forward_only_cases as fo
import parity
import pose_grad_cases as pg
from photo_slam_amd import capi, scene
from photo_slam_amd import rasterize_points as rp

REG_TOL = 1e-5
DEPTH_FIRST, TILE_FIRST = pg.DEPTH_FIRST, pg.TILE_FIRST
ALL_RAW = capi.RAW_OPACITY | capi.RAW_SCALING | capi.RAW_ROTATION
WEIGHTS = dict(w_opacity=0.013, w_scale=0.0071, w_isotropic=0.029)
LARGE = 40000   # (see check_isolated)
SIZES = (1, 127, 128, 129, 330, 33000, LARGE)
W, H, FX = 96, 64, 80.0
BG = np.array([0.2, 0.5, 0.1], np.float32)
OUT_NAMES = pg.GRAD_NAMES
K_OPACITY, K_SCALE = 2, 6

_clouds = {}


def cloud(P, seed=3, scale_k=0.2, size=(W, H, FX)):
    """scene.make_cloud at 96 x 64 with the logits clipped to [-3, 3] (module docstring) and the last three Gaussians moved in front
    of the camera, so that the last rows of the last workgroup are visible ones; P == 1: one Gaussian straight ahead"""
    key = (P, seed, scale_k, size)
    if key not in _clouds:
        cl = scene.make_cloud(P, size[0], size[1], size[2], size[2], seed=seed, scale_k=scale_k)
        cl.opacity = np.clip(cl.opacity, -3.0, 3.0).astype(np.float32)
        cam = cl.cameras[0]
        ahead = cam.campos + 2.5 * cam.viewmatrix[:3, 2]
        side = cam.viewmatrix[:3, 0]
        for k in range(min(3, P)):
            cl.xyz[P - 1 - k] = ahead + 0.3 * (k - 1) * side
        _clouds[key] = cl
    return copy.deepcopy(_clouds[key])


def away_camera(cam):
    """a camera far behind the scene looking away from it: sees nothing"""
    return scene.make_camera(cam.W, cam.H, FX, FX, np.eye(3), np.array([0.0, 0.0, 500.0]))


# ---------------------------------------------------------------------------------------------------- the float64 reference
def reference(opacity_in, scales_in, radii, w, raw):
    """(dL_dopacity [P,1], dL_dscale [P,3], loss [3]) of the definitions in include/gsr.h, float64.  opacity_in / scales_in: the fp32
    arrays the kernel is given (raw or activated, by `raw`); scales_in None = cov3D_precomp"""
    vis = np.asarray(radii) > 0
    wo, ws, wi = (float(np.float32(w.get(k, 0.0))) for k in ("w_opacity", "w_scale", "w_isotropic"))
    x = np.asarray(opacity_in, np.float64).reshape(-1)
    o = 1.0 / (1.0 + np.exp(-x)) if raw & capi.RAW_OPACITY else x
    go = np.where(vis, wo * (o * (1.0 - o) if raw & capi.RAW_OPACITY else np.ones_like(o)), 0.0)
    loss = [wo * o[vis].sum(), 0.0, 0.0]
    gs = np.zeros((x.shape[0], 3))
    if scales_in is not None:
        y = np.asarray(scales_in, np.float64)
        s = np.exp(y) if raw & capi.RAW_SCALING else y
        d = s - s.mean(1, keepdims=True)
        same = (s[:, :1] == s).all(1)   # (three equal scales: d is exactly 0 by definition, whatever the mean's rounding)
        d[same] = 0.0
        sg = np.sign(d)
        gs = ws + wi * (sg - sg.mean(1, keepdims=True))
        if raw & capi.RAW_SCALING:
            gs = gs * s
        gs = np.where(vis[:, None], gs, 0.0)
        loss[1] = ws * s[vis].sum()
        loss[2] = wi * np.abs(d[vis]).sum()
    return go.reshape(-1, 1), gs, np.array(loss)


# ---------------------------------------------------------------------------------------------------- the library
def model_inputs(cl, cam, dev, raw=0, sh_coeffs=None, **kw):
    """fo.inputs with the raw tensors where `raw` says so, or a compact [P,M,3] SH tensor"""
    sh = fo._t(np.ascontiguousarray(cl.get_features()[:, :sh_coeffs]), dev) if sh_coeffs else None
    a = fo.inputs(cl, cam, BG, dev, sh=sh, **kw)
    if raw & capi.RAW_OPACITY:
        a["opacity"] = fo._t(cl.opacity, dev)
    if raw & capi.RAW_SCALING and a["scales"].numel():
        a["scales"] = fo._t(cl.scaling, dev)
    if raw & capi.RAW_ROTATION and a["rotations"].numel():
        a["rotations"] = fo._t(cl.rotation, dev)
    return a


def backward(lib_path, a, cam, dpix, flags=0, raw=0, deg=3, scale_modifier=1.0, aa=False, reg=None, want_loss=False, dD=None, dA=None,
             **bkw):
    """forward (training) + backward; returns (the tuple of eight, radii, the [3] loss tensor or None)"""
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        a = dict(a, degree=deg, scale_modifier=scale_modifier)
        dev = a["means3D"].device
        R, _, radii, g, b, i = rp.RasterizeGaussiansCUDA(**a, raw_params=flags | raw, antialiasing=aa)
        loss = torch.full((3,), 7.0, device=dev) if want_loss else None
        if reg is not None:
            reg = dict(reg, loss=loss)
        out = rp.RasterizeGaussiansBackwardCUDA(a["background"], a["means3D"], radii, a["colors"], a["scales"], a["rotations"],
                                                scale_modifier, a["cov3D_precomp"], a["viewmatrix"], a["projmatrix"], cam.tanfovx,
                                                cam.tanfovy, dpix, a["sh"], deg, a["campos"], g, R, b, i, raw_params=raw,
                                                dL_ddepth=dD, dL_dalpha=dA, antialiasing=aa, geom_reg=reg, **bkw)
        if dev.type != "cpu":
            torch.cuda.synchronize()
        return out, radii.cpu().numpy(), loss
    finally:
        rp._LIB_OVERRIDE = prev


def _np(t):
    return t.detach().cpu().numpy()


def _elementwise(name, got, want, vis):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert not got[~vis].any(), f"{name}: a culled row is not exactly 0"
    err = np.abs(got[vis] - want[vis]) / np.maximum(np.abs(want[vis]), 1e-300)
    err = np.where(want[vis] == 0, np.abs(got[vis]) != 0, err)
    worst = float(err.max()) if err.size else 0.0
    print(f"measured: {name} worst element-wise relative error {worst:.3g} over {int(vis.sum())} visible rows")
    assert worst <= REG_TOL, (name, worst)
    return worst


def _check_loss(loss, want):
    got = _np(loss).astype(np.float64)
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    err = np.where(want == 0, got != 0, err)
    print("measured: loss", got, "float64", want, "relative error", err)
    assert (err <= REG_TOL).all(), (got, want, err)


# ---------------------------------------------------------------------------------------------------- 1. the term in isolation
def check_isolated(lib_path, dev, P, raw=0, scale_modifier=1.0, aa=False, path="rows", flags=0, weights=WEIGHTS, want_loss=True):
    """dL_dpix = 0: what the pass writes is the regulariser's gradient alone.  path: "rows" (16-byte aligned [P,16,3] SH), "compact"
    ([P,9,3] SH, degree 2), "colors" (colors_precomp)"""
    cl = cloud(P)
    cam = cl.cameras[0]
    kw = dict(use_colors_precomp=True) if path == "colors" else {}
    a = model_inputs(cl, cam, dev, raw, sh_coeffs=9 if path == "compact" else None, **kw)
    dpix = torch.zeros((3, cam.H, cam.W), device=dev)
    out, radii, loss = backward(lib_path, a, cam, dpix, flags=flags, raw=raw, deg=2 if path == "compact" else 3,
                                scale_modifier=scale_modifier, aa=aa, reg=weights, want_loss=want_loss)
    vis = radii > 0
    assert vis.any(), "the scene has no visible Gaussian"
    if P >= 128:
        assert (~vis).any(), "the scene has no culled Gaussian"
    if P == 330:
        assert 0 < vis[:64].sum() < 64, "no wave holds both culled and visible rows"
    if P >= 33000:
        # 33 000 Gaussians are 258 workgroups of 128: more than the 256 threads of the final sum, so its strided loop runs twice --
        # but fewer than the 300 workgroups with a visible row the issue asks for, which no scene of that size can have.  So 33 000
        # must have a visible row in more than 256 workgroups, and LARGE = 40 000 (313 workgroups) carries the bar of 300.
        groups = np.add.reduceat(vis, np.arange(0, P, 128)) > 0
        print("measured: workgroups with a visible row", int(groups.sum()), "of", groups.size)
        assert groups.sum() >= (300 if P >= LARGE else 257)
    go, gs, want_loss64 = reference(_np(a["opacity"]), _np(a["scales"]), radii, weights, raw)
    rep = dict(opacity=_elementwise("dL_dopacity", _np(out[K_OPACITY]), go, vis),
               scale=_elementwise("dL_dscales", _np(out[K_SCALE]), gs, vis))
    for k, name in enumerate(OUT_NAMES):
        if k not in (K_OPACITY, K_SCALE) and out[k] is not None:
            assert not bool(out[k].any()), f"{name} is not exactly 0 under a zero upstream gradient"
    if want_loss:
        _check_loss(loss, want_loss64)
    return rep


# ---------------------------------------------------------------------------------------------------- 2. isotropy corner cases
def check_isotropy_corners(lib_path, dev):
    """three equal scales: gradient and loss contribution exactly 0; two equal and one larger: w (-2/3, -2/3, +4/3), activated inputs"""
    cl = cloud(129)
    cam = cl.cameras[0]
    P = cl.xyz.shape[0]
    rng = np.random.default_rng(5)
    base = np.exp(cl.scaling[:, :1]).astype(np.float32)   # every mantissa pattern the cloud has
    wi = np.float32(0.029)
    a = model_inputs(cl, cam, dev, 0)
    dpix = torch.zeros((3, cam.H, cam.W), device=dev)
    # (a) all equal
    a["scales"] = fo._t(np.repeat(base, 3, 1), dev)
    out, radii, loss = backward(lib_path, a, cam, dpix, reg=dict(w_isotropic=float(wi)), want_loss=True)
    assert (radii > 0).any()
    assert not bool(out[K_SCALE].any()), "three equal scales must give a gradient of exactly 0"
    assert not bool(loss.any()), "three equal scales must contribute exactly 0 to the loss"
    # (b) two equal, one larger, the larger one in a random position
    pos = rng.integers(0, 3, P)
    s = np.repeat(base, 3, 1)
    s[np.arange(P), pos] *= np.float32(1.75)
    a["scales"] = fo._t(s, dev)
    out, radii, loss = backward(lib_path, a, cam, dpix, reg=dict(w_isotropic=float(wi)), want_loss=True)
    vis = radii > 0
    assert vis.any()
    # fp32, as the definition is evaluated: w (sgn - mean sgn), mean sgn = (-1 - 1 + 1) / 3
    mean = (np.float32(-1.0)) / np.float32(3.0)
    small, large = wi * (np.float32(-1.0) - mean), wi * (np.float32(1.0) - mean)
    want = np.where(np.arange(3)[None, :] == pos[:, None], large, small).astype(np.float32)
    want[~vis] = 0.0
    got = _np(out[K_SCALE])
    assert np.array_equal(got, want), (np.abs(got - want).max(), "two equal scales and one larger: w (-2/3, -2/3, +4/3)")
    assert abs(float(large) / float(wi) - 4.0 / 3.0) < 2e-7 and abs(float(small) / float(wi) + 2.0 / 3.0) < 2e-7
    _check_loss(loss, reference(_np(a["opacity"]), s, radii, dict(w_isotropic=float(wi)), 0)[2])


# ---------------------------------------------------------------------------------------------------- 3. added to a real gradient
def check_added(lib_path, dev, P, raw=0, maps=False, aa=False, path="rows", seed=0):
    """a random dL_dpix (maps: depth and alpha gradients too): the result with the struct = the result without it + the float64
    term; the other outputs unchanged"""
    cl = cloud(P)
    cam = cl.cameras[0]
    rng = np.random.default_rng(seed)
    kw = dict(use_colors_precomp=True) if path == "colors" else {}
    a = model_inputs(cl, cam, dev, raw, sh_coeffs=9 if path == "compact" else None, **kw)
    dpix = fo._t(rng.standard_normal((3, cam.H, cam.W)).astype(np.float32), dev)
    dD = fo._t(rng.standard_normal((cam.H, cam.W)).astype(np.float32), dev) if maps else None
    dA = fo._t(rng.standard_normal((cam.H, cam.W)).astype(np.float32), dev) if maps else None
    run = lambda reg: backward(lib_path, a, cam, dpix, raw=raw, deg=2 if path == "compact" else 3, aa=aa, reg=reg, dD=dD, dA=dA)
    plain, radii, _ = run(None)
    with_, radii2, _ = run(WEIGHTS)
    assert np.array_equal(radii, radii2)
    vis = radii > 0
    go, gs, _ = reference(_np(a["opacity"]), _np(a["scales"]), radii, WEIGHTS, raw)
    exact = dev.type == "cpu"
    rep = {}
    for k, r in ((K_OPACITY, go), (K_SCALE, gs)):
        g, h = _np(plain[k]).astype(np.float64), _np(with_[k]).astype(np.float64)
        assert float(np.abs(g).sum()) > 0, "the upstream gradient reached nothing"
        want = g + r
        if exact:
            tol = 2.0 ** -23 * np.abs(want) + REG_TOL * np.abs(r)
            worst = float((np.abs(h - want) / np.maximum(tol, 1e-300)).max())
            print(f"measured: {OUT_NAMES[k]} worst |out - (g + r)| / tolerance {worst:.3g}")
            assert (np.abs(h - want) <= tol).all(), (OUT_NAMES[k], worst)
            assert np.array_equal(h[~vis], g[~vis])
        else:
            rep[OUT_NAMES[k]] = parity.rel_l1(h, want)
            print(f"measured: {OUT_NAMES[k]} rel L1 of out against g + r {rep[OUT_NAMES[k]]:.3g}")
            assert rep[OUT_NAMES[k]] <= parity.GRAD_REL_L1_TOL, rep
            assert not np.abs(h[~vis]).any()
    for k, name in enumerate(OUT_NAMES):
        if k not in (K_OPACITY, K_SCALE):
            assert (plain[k] is None) == (with_[k] is None)
            if plain[k] is not None:
                pg.same_or_rerun_close(name + " with the regularisers on", with_[k], plain[k], exact)
    return rep


# ---------------------------------------------------------------------------------------------------- 4. the loss values
def check_loss_values(lib_path, dev, P, raw=ALL_RAW, aa=False):
    """the three floats against float64 sums; a rerun and the other binning arrangement give the same bits; a camera that sees
    nothing and P == 0 give zeros"""
    cl = cloud(P)
    cam = cl.cameras[0]
    a = model_inputs(cl, cam, dev, raw)
    dpix = fo._t(np.random.default_rng(1).standard_normal((3, cam.H, cam.W)).astype(np.float32), dev)
    first = None
    # (at the large size the rerun is left to the smaller ones: one run per arrangement)
    for flags in ((DEPTH_FIRST, DEPTH_FIRST, TILE_FIRST) if P < 33000 else (DEPTH_FIRST, TILE_FIRST)):
        _, radii, loss = backward(lib_path, a, cam, dpix, flags=flags, raw=raw, aa=aa, reg=WEIGHTS, want_loss=True)
        _check_loss(loss, reference(_np(a["opacity"]), _np(a["scales"]), radii, WEIGHTS, raw)[2])
        assert bool((loss > 0).all())
        if first is None:
            first = loss
        else:
            assert torch.equal(first, loss), ("a rerun or the other binning arrangement gave different loss bits", first, loss)
    if P >= 33000:
        return
    away = away_camera(cam)
    _, radii, loss = backward(lib_path, model_inputs(cl, away, dev, raw), away, dpix, raw=raw, reg=WEIGHTS, want_loss=True)
    assert not (radii > 0).any()
    assert bool((loss == 0).all()), "a view that sees nothing must write three zeros"
    e = model_inputs(cl, cam, dev, raw)
    for k in ("means3D", "opacity", "scales", "rotations", "sh"):
        e[k] = e[k][:0]
    _, _, loss = backward(lib_path, e, cam, dpix, raw=raw, reg=WEIGHTS, want_loss=True)
    assert bool((loss == 0).all()), "P == 0 must write three zeros"


# ---------------------------------------------------------------------------------------------------- 5. the fused step
def check_fused(lib_path, dev, lazy=False, sh_adam=True, P=330, seed=0):
    """raw_params = 7 + geom_adam + the struct (+ sh_adam, eager or lazy): parameters and moments afterwards = the unfused gradients,
    struct included, followed by gsr_adam_step; the bar of parity.check_fused_geom_adam"""
    cl = cloud(P)
    cam = cl.cameras[0]
    lib = capi.load(lib_path)
    rng = np.random.default_rng(seed)
    dpix = fo._t(rng.standard_normal((3, cam.H, cam.W)).astype(np.float32), dev)
    names = ("xyz", "opacity", "scaling", "rotation")
    init = dict(xyz=cl.xyz, opacity=cl.opacity.reshape(P, 1), scaling=cl.scaling, rotation=cl.rotation, sh=cl.get_features())
    mom = {n: ((0.01 * rng.standard_normal(init[n].shape)).astype(np.float32), (1e-4 * rng.random(init[n].shape)).astype(np.float32))
           for n in init}
    lrs = dict(xyz=1.6e-4, opacity=0.05, scaling=0.005, rotation=0.001)
    steps = dict(xyz=4, opacity=2, scaling=4, rotation=7)
    row_step0 = np.full(P, 3, np.int32)   # (every row up to date: the lazy forward pass changes no SH row)

    def run(fused):
        st = {n: [fo._t(init[n].copy(), dev).clone(), fo._t(mom[n][0].copy(), dev).clone(), fo._t(mom[n][1].copy(), dev).clone()]
              for n in init}
        a = fo.inputs(cl, cam, BG, dev, sh=st["sh"][0])
        a.update(means3D=st["xyz"][0], opacity=st["opacity"][0], scales=st["scaling"][0], rotations=st["rotation"][0])
        bkw = {}
        if fused:
            bkw["geom_adam"] = dict(tensors=[(st[n][0], st[n][1], st[n][2], lrs[n], steps[n]) for n in names], beta1=0.9, beta2=0.999, eps=1e-15)
            if sh_adam:
                sa = dict(exp_avg=st["sh"][1], exp_avg_sq=st["sh"][2], lr=0.0025, lr_tail=0.000125, beta1=0.9, beta2=0.999, eps=1e-15, step=4)
                if lazy:
                    sa.update(row_step=fo._t(row_step0.copy(), dev), window=4, lr_past=[0.0025] * 3, lr_tail_past=[0.000125] * 3)
                bkw["sh_adam"] = sa
            bkw["training_outputs_only"] = True
        prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
        try:
            R, _, radii, g, b, i = rp.RasterizeGaussiansCUDA(**a, raw_params=ALL_RAW, sh_adam=bkw.get("sh_adam") if lazy else None)
            loss = torch.full((3,), 7.0, device=dev)
            out = rp.RasterizeGaussiansBackwardCUDA(a["background"], a["means3D"], radii, a["colors"], a["scales"], a["rotations"], 1.0,
                                                    a["cov3D_precomp"], a["viewmatrix"], a["projmatrix"], cam.tanfovx, cam.tanfovy, dpix,
                                                    a["sh"], 3, a["campos"], g, R, b, i, raw_params=ALL_RAW,
                                                    geom_reg=dict(WEIGHTS, loss=loss), **bkw)
            if dev.type != "cpu":
                torch.cuda.synchronize()
        finally:
            rp._LIB_OVERRIDE = prev
        return st, out, radii.cpu().numpy(), loss

    st_ref, g_ref, radii, loss_ref = run(False)
    grads = dict(xyz=g_ref[3], opacity=g_ref[2], scaling=g_ref[6], rotation=g_ref[7])
    go, gs, want_loss = reference(cl.opacity, cl.scaling, radii, WEIGHTS, ALL_RAW)
    vis = radii > 0
    assert float(np.abs(gs[vis]).min()) > 0 and float(np.abs(_np(g_ref[6])[vis]).sum()) > 0
    for n in names:   # the separate passes
        p_, m_, v_ = st_ref[n]
        gr = grads[n].contiguous()
        capi.check(lib, lib.gsr_adam_step(p_.data_ptr(), gr.data_ptr(), m_.data_ptr(), v_.data_ptr(), p_.numel(), lrs[n], 0.9, 0.999,
                                          1e-15, steps[n], 0, 0, lrs[n], None), "gsr_adam_step")
    if dev.type != "cpu":
        torch.cuda.synchronize()
    st_fus, g_fus, _, loss_fus = run(True)
    assert g_fus[2] is None and g_fus[6] is None
    _check_loss(loss_fus, want_loss)
    assert torch.equal(loss_fus, loss_ref), "the loss values of the fused and the unfused call differ"
    exact = dev.type == "cpu"
    assert vis.any() and (~vis).any()
    for n in names:
        for k, what in enumerate(("param", "exp_avg", "exp_avg_sq")):
            x, y = _np(st_fus[n][k]), _np(st_ref[n][k])
            tol = max(lrs[n] * (2e-6 if exact else 2e-3), 1.2e-7 * np.abs(y).max()) if k == 0 else (1e-6 if exact else 2e-4) * np.abs(y).max()
            print(f"measured: fused {n} {what} max difference {np.abs(x - y).max():.3g} (bar {tol:.3g})")
            assert np.abs(x - y).max() <= tol, (n, what, np.abs(x - y).max(), tol)


# ---------------------------------------------------------------------------------------------------- 6. off is off
def check_off_is_off(lib_path, dev, P=330, raw=0):
    """a struct with zero weights and loss == NULL gives the outputs of NULL"""
    cl = cloud(P)
    cam = cl.cameras[0]
    a = model_inputs(cl, cam, dev, raw)
    dpix = fo._t(np.random.default_rng(2).standard_normal((3, cam.H, cam.W)).astype(np.float32), dev)
    plain, _, _ = backward(lib_path, a, cam, dpix, raw=raw)
    off, _, _ = backward(lib_path, a, cam, dpix, raw=raw, reg=dict(w_opacity=0.0, w_scale=0.0, w_isotropic=0.0))
    for name, x, y in zip(OUT_NAMES, plain, off):
        pg.same_or_rerun_close(name + " with an all-zero struct", y, x, dev.type == "cpu")


# ---------------------------------------------------------------------------------------------------- 7. the API contract
def check_api_contract(lib_path, dev):
    """every error of include/gsr.h: gsr_geom_reg"""
    lib = capi.load(lib_path)
    assert int(lib.gsr_geom_reg_scratch_bytes(0)) >= 0 and int(lib.gsr_geom_reg_scratch_bytes(1000)) >= 4 * 3 * 8
    cl = cloud(129)
    cam = cl.cameras[0]
    P = cl.xyz.shape[0]
    a = model_inputs(cl, cam, dev, 0)
    dpix = torch.ones((3, cam.H, cam.W), device=dev)

    def status(reg, want_loss=False, **kw):
        try:
            backward(lib_path, kw.pop("inputs", a), cam, dpix, reg=reg, want_loss=want_loss, **kw)
        except capi.GsrError as e:
            return e.status
        return 0

    assert status(WEIGHTS, True) == 0
    for bad in (-1e-3, float("nan"), float("inf"), -float("inf")):
        for k in WEIGHTS:
            assert status(dict(WEIGHTS, **{k: bad})) == -1, (k, bad, "a negative or non-finite weight: GSR_ERR_INVALID_ARG")
    cov = model_inputs(cl, cam, dev, 0, use_cov3D_precomp=True)
    assert status(dict(w_opacity=0.1), True, inputs=cov) == 0, "the opacity term works with cov3D_precomp"
    assert status(dict(w_scale=0.1), inputs=cov) == -1 and status(dict(w_isotropic=0.1), inputs=cov) == -1, "no scales to regularise"
    assert status(WEIGHTS, dL_dcolor_view=torch.zeros((P, 3), device=dev)) == -4, "with dL_dcolor_view: GSR_ERR_UNSUPPORTED"
    assert status(WEIGHTS, pose_grad=True) == -4, "with the pose outputs: GSR_ERR_UNSUPPORTED"
    assert status(dict(w_opacity=0.0), pose_grad=True) == 0, "an all-zero struct behaves as NULL"
    # loss without scratch: the C-ABI directly
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        R, _, radii, g, b, i = rp.RasterizeGaussiansCUDA(**a, raw_params=0)
        grads = [torch.empty((P, n), device=dev) for n in (3, 4, 1, 3, 3, 6, 48, 3, 4)]
        loss = torch.full((3,), 7.0, device=dev)
        ba = capi.BackwardArgs()
        ba.P, ba.D, ba.M, ba.R, ba.width, ba.height = P, 3, 16, R, cam.W, cam.H
        ba.scale_modifier, ba.tan_fovx, ba.tan_fovy = 1.0, cam.tanfovx, cam.tanfovy
        for n in ("background", "means3D", "scales", "rotations", "viewmatrix", "projmatrix", "campos"):
            setattr(ba, n, a[n].data_ptr())
        ba.shs, ba.radii, ba.dL_dpix = a["sh"].data_ptr(), radii.data_ptr(), dpix.data_ptr()
        ba.geom_buffer, ba.binning_buffer, ba.image_buffer = g.data_ptr(), b.data_ptr(), i.data_ptr()
        for n, t in zip(("dL_dmean2D", "dL_dconic", "dL_dopacity", "dL_dcolor", "dL_dmean3D", "dL_dcov3D", "dL_dsh", "dL_dscale", "dL_drot"), grads):
            setattr(ba, n, t.data_ptr())
        gr = capi.GeomReg(0.1, 0.1, 0.1, loss.data_ptr(), None)
        ba.geom_reg = C.pointer(gr)
        assert lib.gsr_backward(C.byref(ba), rp._stream_ptr(a["means3D"])) == -1, "loss without scratch was accepted"
        if dev.type != "cpu":
            torch.cuda.synchronize()
        assert bool((loss == 7.0).all())
        scratch = torch.empty((int(lib.gsr_geom_reg_scratch_bytes(P)),), dtype=torch.uint8, device=dev)
        gr.scratch = scratch.data_ptr()
        ba.P = 0
        capi.check(lib, lib.gsr_backward(C.byref(ba), rp._stream_ptr(a["means3D"])), "P == 0")
        if dev.type != "cpu":
            torch.cuda.synchronize()
        assert bool((loss == 0.0).all()), "P == 0 must write three zeros"
    finally:
        rp._LIB_OVERRIDE = prev


# ---------------------------------------------------------------------------------------------------- 8. the hosts
HOST_STEPS = 30
LAMBDA_ISOTROPIC = 10.0   # (MonoGS's value)
LAMBDA_OPACITY = 0.01     # (3DGS-MCMC's value)


def needle_cloud(P=300):
    """about 300 Gaussians at 96 x 64, each started as a needle: one scale (a random axis) 8 times the other two"""
    cl = cloud(P, seed=4, scale_k=0.05)   # (small: a needle is then 0.3 m long, a handful of tiles)
    rng = np.random.default_rng(11)
    cl.scaling = np.repeat(cl.scaling[:, :1], 3, 1)
    cl.scaling[np.arange(P), rng.integers(0, 3, P)] += np.float32(np.log(8.0))
    return cl


def wall_cloud():
    """an opaque wall of 8 x 6 large Gaussians 2 m in front of the camera and 200 small ones 1.5 m behind it: those are inside the
    frustum (radii > 0) and explain nothing.  Returns (cloud, the hidden ones' indices)."""
    cl = cloud(248, seed=6, size=(48, 32, 40.0))   # (the same field of view at a quarter of the pixels: the wall covers every tile)
    cam = cl.cameras[0]
    right, up, fwd = cam.viewmatrix[:3, 0], cam.viewmatrix[:3, 1], cam.viewmatrix[:3, 2]
    rng = np.random.default_rng(12)
    n = 0
    for j in range(6):
        for i in range(8):
            u, v = (i - 3.5) / 3.5 * 1.3 * 2.0 * cam.tanfovx, (j - 2.5) / 2.5 * 1.3 * 2.0 * cam.tanfovy
            cl.xyz[n] = cam.campos + 2.0 * fwd + u * right + v * up
            cl.scaling[n] = np.log(0.3)
            cl.opacity[n] = 6.0
            n += 1
    hidden = np.arange(n, 248)
    for k in hidden:
        u, v = (rng.random(2) * 2 - 1) * 0.7 * 3.5 * np.array([cam.tanfovx, cam.tanfovy])
        cl.xyz[k] = cam.campos + 3.5 * fwd + u * right + v * up
        cl.scaling[k] = np.log(0.05)
        cl.opacity[k] = 0.0
    return cl, hidden


def _train(lib_path, dev, cl, steps, gt_from=None, **lambdas):
    """`steps` train steps of a Python TrainStep on cl against the render of gt_from (default: cl itself) from cl's camera; returns
    (model, trainer, the losses returned)"""
    from photo_slam_amd.gaussian_renderer import GaussianKeyframe
    cam = cl.cameras[0]
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        kf = GaussianKeyframe.from_camera(cam, dev)
        g0, ts0 = pg.python_trainer(gt_from if gt_from is not None else cl, dev, deg=3)
        gt = ts0.render_view(kf).clone()
        g, ts = pg.python_trainer(cl, dev, deg=3)
        for k, v in lambdas.items():
            setattr(ts, k, v)
        mask = torch.ones_like(gt)
        losses = [ts.trainForOneIteration(kf, gt, mask, sync_loss=(i == 0)) for i in range(steps)]
        if dev.type != "cpu":
            torch.cuda.synchronize()
        return g, ts, losses
    finally:
        rp._LIB_OVERRIDE = prev


def check_host_isotropy(lib_path, dev, trainer=_train):
    """needles, 30 steps against the render of the round cloud: the mean of max-scale / min-scale is strictly lower with
    isotropic_reg_ on.  Returns (off, on)."""
    cl = needle_cloud()
    round_ = cloud(300, seed=4, scale_k=0.05)
    round_.scaling = np.repeat(round_.scaling[:, :1], 3, 1)
    ratio = {}
    for name, lam in (("off", 0.0), ("on", LAMBDA_ISOTROPIC)):
        g, _, _ = trainer(lib_path, dev, copy.deepcopy(cl), HOST_STEPS, gt_from=round_, isotropic_reg_=lam)
        sc = np.exp(_np(g.scaling_).astype(np.float64))
        ratio[name] = float((sc.max(1) / sc.min(1)).mean())
    print("measured: mean max-scale / min-scale after", HOST_STEPS, "steps: regulariser off", ratio["off"], "on", ratio["on"], "(start 8)")
    assert ratio["on"] < ratio["off"], ratio
    return ratio["off"], ratio["on"]


def check_host_opacity(lib_path, dev, trainer=_train):
    """Gaussians behind an opaque wall, 30 steps against the model's own render: their mean activated opacity is strictly lower with
    opacity_reg_ on.  Returns (off, on)."""
    cl, hidden = wall_cloud()
    mean = {}
    for name, lam in (("off", 0.0), ("on", LAMBDA_OPACITY)):
        g, _, _ = trainer(lib_path, dev, copy.deepcopy(cl), HOST_STEPS, opacity_reg_=lam)
        o = 1.0 / (1.0 + np.exp(-_np(g.opacity_).astype(np.float64).reshape(-1)))
        mean[name] = float(o[hidden].mean())
    print("measured: mean activated opacity of the hidden Gaussians after", HOST_STEPS, "steps: regulariser off", mean["off"], "on",
          mean["on"], "(start 0.5)")
    assert mean["on"] < mean["off"], mean
    return mean["off"], mean["on"]


def check_host_losses(lib_path, dev):
    """last_reg_losses = the definitions evaluated on the model before the step, with the hosts' normalisation by the visible
    count; the returned loss = the loss of the same step without the regularisers + the three terms; None when nobody reads it"""
    cl = needle_cloud()
    cam = cl.cameras[0]
    lam = dict(opacity_reg_=LAMBDA_OPACITY, scale_reg_=0.02, isotropic_reg_=LAMBDA_ISOTROPIC)
    _, ts, losses = _train(lib_path, dev, copy.deepcopy(cl), 2, **lam)
    assert ts.last_reg_losses is None, "a step whose loss nobody reads must not form the three terms"
    _, ts1, losses1 = _train(lib_path, dev, copy.deepcopy(cl), 1, **lam)
    _, _, plain = _train(lib_path, dev, copy.deepcopy(cl), 1)
    a = model_inputs(cl, cam, dev, ALL_RAW)
    _, radii, _ = backward(lib_path, a, cam, torch.zeros((3, cam.H, cam.W), device=dev), raw=ALL_RAW)
    V = max(int((radii > 0).sum()), 1)
    w = dict(w_opacity=LAMBDA_OPACITY / V, w_scale=0.02 / (3.0 * V), w_isotropic=LAMBDA_ISOTROPIC / (3.0 * V))
    want = reference(cl.opacity, cl.scaling, radii, w, ALL_RAW)[2]
    assert ts1.last_reg_losses is not None and tuple(ts1.last_reg_losses.shape) == (3,)
    _check_loss(ts1.last_reg_losses, want)
    total, base = float(losses1[0].detach()), float(plain[0].detach())
    print("measured: returned loss", total, "photometric", base, "terms", want)
    assert abs(total - (base + want.sum())) <= 1e-5 * abs(total), (total, base, want)
    return want


def check_host_cpp(ops, lib_path, dev, steps=5):
    """the C++ host (TrainStep::opacity_reg_ / scale_reg_ / isotropic_reg_ through ops_register.cpp) against the Python host on the
    needle scene: the same losses, the same three terms and -- after 5 steps -- the same parameters, to the bars tests/test_cpp_host.py
    uses for that comparison (losses rtol 1e-5; parameters rtol 1e-4, atol 1e-6); and the regularisers moved the model"""
    from photo_slam_amd.gaussian_renderer import GaussianKeyframe
    cl = needle_cloud()
    cam = cl.cameras[0]
    lam = dict(opacity_reg=LAMBDA_OPACITY, scale_reg=0.02, isotropic_reg=LAMBDA_ISOTROPIC)
    h = pg.cpp_trainer(ops, cl, dev, deg=3)
    try:
        # (a target that is NOT the model's own render: at a zero residual the L1 gradient is the sign of rounding noise, which
        # Adam turns into full steps -- two hosts then part ways for reasons that have nothing to do with the regularisers)
        gt = torch.rand(3, cam.H, cam.W, generator=torch.Generator().manual_seed(0)).to(dev)
        mask = torch.ones_like(gt)
        ops.trainer_set_options(h, {k: float(v) for k, v in lam.items()})
        losses_cpp, terms_cpp = [], []
        for _ in range(steps):
            losses_cpp.append(float(ops.trainer_render_and_backward(h, *pg._cam_args(cam, dev), gt, mask)))
            terms_cpp.append(ops.trainer_last_reg_losses(h).clone())
            ops.trainer_finish(h)
        ops.trainer_set_options(h, {"read_reg_losses": 0.0})
        ops.trainer_render_and_backward(h, *pg._cam_args(cam, dev), gt, mask)
        assert ops.trainer_last_reg_losses(h).numel() == 0, "read_reg_losses = 0 must not form the three terms"
        ops.trainer_finish(h)
        ops.trainer_set_options(h, {"read_reg_losses": 1.0})
        params_cpp = [p.detach().clone() for p in ops.trainer_params(h)]
    finally:
        ops.trainer_destroy(h)
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        kf = GaussianKeyframe.from_camera(cam, dev)
        runs = {}
        for name, on in (("on", True), ("off", False)):
            g, ts = pg.python_trainer(cl, dev, deg=3)
            if on:
                ts.opacity_reg_, ts.scale_reg_, ts.isotropic_reg_ = lam["opacity_reg"], lam["scale_reg"], lam["isotropic_reg"]
            losses, terms = [], []
            for _ in range(steps):
                losses.append(float(ts.trainForOneIteration(kf, gt, mask, sync_loss=True).detach()))
                terms.append(ts.last_reg_losses)
            ts.trainForOneIteration(kf, gt, mask, sync_loss=False)
            g.sync_features()
            runs[name] = (g, losses, terms)
    finally:
        rp._LIB_OVERRIDE = prev
    g, losses_py, terms_py = runs["on"]
    print("measured: losses C++", losses_cpp, "Python", losses_py)
    assert np.allclose(losses_cpp, losses_py, rtol=1e-5), (losses_cpp, losses_py)
    for a, b in zip(terms_cpp, terms_py):
        assert a.shape == (3,) and torch.allclose(a, b, rtol=1e-5, atol=0), (a, b)
    worst = 0.0
    for a, b in zip(params_cpp, g.params()):
        worst = max(worst, float((a - b.detach()).abs().max()))
        assert torch.allclose(a, b.detach(), rtol=1e-4, atol=1e-6)
    print("measured: largest parameter difference C++ / Python after", steps + 1, "steps", worst)
    moved = float((runs["on"][0].scaling_.detach() - runs["off"][0].scaling_.detach()).abs().max())
    assert moved > 1e-3, "the regularisers did not move the scales"
