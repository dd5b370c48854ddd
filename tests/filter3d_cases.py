"""Shared checks of the 3-D smoothing filter (GSR_FILTER_3D and gsr_filter3d_compute, include/gsr.h) for the emulator tests
(test_filter3d.py) and the GPU tests (test_gpu_filter3d.py).

The CPU oracle serves as the reference unchanged: the filter is an input transform, so the render with the bit is the oracle's render
of the activated inputs (s', o').  s' and o' are restated twice here -- filtered32() in numpy float32 in the operation order gsr.h
documents, filtered64() in float64 torch with autograd -- and the filter itself twice as well (filter32(), filter64()); upstream's
compute_3D_filter is transcribed in upstream_filter().  None of them shares code with the kernels.

Backward: the oracle's backward pass on (s'32, o'32) gives g_s' and g_o' with both held independent; with the bit the library must
return them pushed through the chain rule of gsr.h, which filtered64()'s autograd applies in float64.  Every other gradient is the
oracle's on (s', o').

Bars: the aggregate and per-row bars of tests/parity.py, unchanged, for everything.  The gap between the two RESTATEMENTS (neither
is the code under test) was measured on the visible Gaussians of test_forward_only.SHAPES with camera 0's filter: relative L1 of s'
at most 2.9e-8, of c at most 6.3e-8.  Times 4 for operation-order freedom that is 2.6e-7, far inside parity.GRAD_REL_L1_TOL = 1e-4 and
the row bars, so no bar of its own was needed.  RESTATEMENT_GAP records the measurement; test_filter3d.py re-measures it and holds
it to 4 x that figure."""
import copy
import hashlib

import numpy as np
import torch

import antialias_cases as aa
import depth_alpha_cases as da
import forward_only_cases as fo
import parity
import pose_grad_cases as pg
from photo_slam_amd import capi
from photo_slam_amd import rasterize_points as rp

F3 = capi.FILTER_3D
VARIANCE = 0.2
RESTATEMENT_GAP = dict(s_rel_l1_measured=2.9e-8, c_rel_l1_measured=6.3e-8, factor=4)
GRAD_NAMES = da.GRAD_NAMES
_np = aa._np


# ---------------------------------------------------------------------------------------------------- the filter, restated
def camera_rows(cams, levels=None):
    """[K, 20] float32 rows of gsr_filter3d_camera from scene.Cameras: the view matrix, focal lengths W / (2 tan), the size.
    levels: per camera a divisor d -- the camera at pyramid level W / d x H / d with focal / d"""
    f = np.float32
    rows = np.zeros((len(cams), 20), f)
    for k, c in enumerate(cams):
        d = f(1 if levels is None else levels[k])
        rows[k, :16] = c.viewmatrix.reshape(-1).astype(f)
        rows[k, 16] = f(c.W) / (f(2) * f(c.tanfovx)) / d
        rows[k, 17] = f(c.H) / (f(2) * f(c.tanfovy)) / d
        rows[k, 18] = f(c.W) / d
        rows[k, 19] = f(c.H) / d
    return rows


def filter32(xyz, rows, variance=VARIANCE):
    """gsr_filter3d_compute in numpy float32, the operation order of include/gsr.h; returns (filter [P], observed [P])"""
    f = np.float32
    P = xyz.shape[0]
    x, y, z = (xyz[:, i].astype(f) for i in range(3))
    T = np.zeros(P, f)
    obs = np.zeros(P, bool)
    with np.errstate(all="ignore"):
        for row in rows.astype(f):
            V, fx, fy, w, h = row[:16], row[16], row[17], row[18], row[19]
            X = ((V[0] * x + V[4] * y) + V[8] * z) + V[12]
            Y = ((V[1] * x + V[5] * y) + V[9] * z) + V[13]
            Z = ((V[2] * x + V[6] * y) + V[10] * z) + V[14]
            u = (X / Z) * fx + f(0.5) * w
            v = (Y / Z) * fy + f(0.5) * h
            sees = (Z > f(0.2)) & (u >= f(-0.15) * w) & (u <= f(1.15) * w) & (v >= f(-0.15) * h) & (v <= f(1.15) * h)
            t = (Z / np.maximum(fx, fy)).astype(f)
            T = np.where(sees, np.where(obs, np.minimum(T, t), t), T).astype(f)
            obs |= sees
    sv = np.sqrt(f(variance))
    out = (sv * T).astype(f)
    out[~obs] = sv * (T[obs].max() if obs.any() else f(0))
    assert out.dtype == f
    return out, obs


def filter64(xyz, rows, variance=VARIANCE):
    """the definition in float64: sqrt(variance) times the smallest sampling interval z / max(fx, fy) over the cameras that observe
    the Gaussian; the largest such value for the Gaussians nobody observes"""
    x = xyz.astype(np.float64)
    P = x.shape[0]
    T = np.full(P, np.inf)
    for row in rows.astype(np.float64):
        Wc = row[:16].reshape(4, 4).T   # W2C
        t = x @ Wc[:3, :3].T + Wc[:3, 3]
        fx, fy, w, h = row[16:]
        with np.errstate(all="ignore"):
            u, v = t[:, 0] / t[:, 2] * fx + 0.5 * w, t[:, 1] / t[:, 2] * fy + 0.5 * h
        sees = (t[:, 2] > np.float64(np.float32(0.2))) & (u >= -0.15 * w) & (u <= 1.15 * w) & (v >= -0.15 * h) & (v <= 1.15 * h)
        T = np.where(sees, np.minimum(T, t[:, 2] / max(fx, fy)), T)
    obs = np.isfinite(T)
    out = np.sqrt(variance) * np.where(obs, T, T[obs].max() if obs.any() else 0.0)
    return out, obs


def upstream_filter(xyz, rows):
    """Mip-Splatting's GaussianModel.compute_3D_filter transcribed to numpy float32 (scene/gaussian_model.py of the public
    repository): the smallest depth over the observing cameras and the largest focal_x, separately; both axes are projected with
    focal_x, as upstream does"""
    f = np.float32
    xyz = xyz.astype(f)
    distance = np.ones(xyz.shape[0], f) * f(100000.0)
    valid_points = np.zeros(xyz.shape[0], bool)
    focal_length = f(0.0)
    for row in rows.astype(f):
        Wc = row[:16].reshape(4, 4).T
        R, T = Wc[:3, :3].T, Wc[:3, 3]        # upstream keeps R = C2W rotation^T ... xyz_cam = xyz @ R + T
        xyz_cam = xyz @ R + T[None, :]
        valid_depth = xyz_cam[:, 2] > f(0.2)
        x, y, z = xyz_cam[:, 0], xyz_cam[:, 1], xyz_cam[:, 2]
        z = np.maximum(z, f(0.001))
        x = x / z * row[16] + row[18] / f(2.0)
        y = y / z * row[16] + row[19] / f(2.0)
        in_screen = (x >= f(-0.15) * row[18]) & (x <= row[18] * f(1.15)) & (y >= f(-0.15) * row[19]) & (y <= f(1.15) * row[19])
        valid = valid_depth & in_screen
        distance[valid] = np.minimum(distance[valid], z[valid])
        valid_points |= valid
        if focal_length < row[16]:
            focal_length = row[16]
    distance[~valid_points] = distance[valid_points].max()
    return distance / focal_length * f(0.2 ** 0.5)


def compute(lib_path, dev, xyz, rows, variance=VARIANCE):
    """gsr_filter3d_compute through the Python boundary"""
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        out = rp.filter3D(fo._t(xyz, dev), fo._t(rows.reshape(-1, 20), dev), variance)
        if dev.type != "cpu":
            torch.cuda.synchronize()
        return out.cpu().numpy()
    finally:
        rp._LIB_OVERRIDE = prev


def check_compute(lib_path, dev, cl, rows, variance=VARIANCE, P=None):
    """the library's filter against filter32, bit for bit; twice the same bits; returns (filter, observed)"""
    xyz = cl.xyz if P is None else cl.xyz[:P]
    got = compute(lib_path, dev, xyz, rows, variance)
    want, obs = filter32(xyz, rows, variance)
    assert got.shape == want.shape and got.dtype == np.float32
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, (bad[:5], got[bad[:5]], want[bad[:5]])
    again = compute(lib_path, dev, xyz, rows, variance)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), "two runs gave different bits"
    return got, obs


# ---------------------------------------------------------------------------------------------------- s', o', restated twice
def filtered32(s, o, filt):
    """(s', o', c) in numpy float32, in the operation order of include/gsr.h (GSR_FILTER_3D)"""
    f = np.float32
    s, o, filt = s.astype(f), o.reshape(-1).astype(f), filt.astype(f)
    F = filt * filt
    a = s * s + F[:, None]
    sp = np.sqrt(a).astype(f)
    r = (s / sp).astype(f)
    c = (r[:, 0] * r[:, 1]) * r[:, 2]
    op = o * c
    assert sp.dtype == f and op.dtype == f
    return sp, op, c


def filtered64(s, o, filt):
    """(s', o', c) as float64 torch expressions of s [P,3], o [P], filt [P]"""
    sp = torch.sqrt(s * s + (filt * filt)[:, None])
    r = s / sp
    c = r[:, 0] * r[:, 1] * r[:, 2]
    return sp, o * c, c


def restatement_gap(cl, cam):
    """relative L1 of s' and of c between the two restatements over the visible (z > 0.2) Gaussians, camera `cam`'s filter"""
    filt, _ = filter32(cl.xyz, camera_rows([cam]))
    sp32, _, c32 = filtered32(cl.get_scaling(), cl.get_opacity(), filt)
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))
    sp64, _, c64 = filtered64(t64(cl.get_scaling()), t64(cl.get_opacity().reshape(-1)), t64(filt))
    vis = da.view_z(cl, cam) > 0.2
    return parity.rel_l1(sp32[vis], sp64.numpy()[vis]), parity.rel_l1(c32[vis], c64.numpy()[vis])


def filtered_cloud(cl, filt):
    """a view of the cloud whose ACTIVATED scales and opacities are (s'32, o'32): what the oracle, and the library without the bit,
    are given"""
    sp, op, c = filtered32(cl.get_scaling(), cl.get_opacity(), filt)
    clf = copy.copy(cl)
    op = np.ascontiguousarray(op.reshape(-1, 1))
    clf.get_scaling = lambda: sp
    clf.get_opacity = lambda: op
    return clf, c


def scene_filter(cl, n_views=None):
    """the filter of the cloud's first n_views cameras (all by default), by the numpy restatement"""
    cams = cl.cameras if n_views is None else cl.cameras[:n_views]
    return filter32(cl.xyz, camera_rows(cams))


# ---------------------------------------------------------------------------------------------------- the library
def forward(lib_path, a, flags, filt=None, depth=False, alpha=False, **kw):
    """(R, image, radii, depth, alpha, buffers) of one gsr_forward through the Python boundary; filt: the filter tensor"""
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        dev = a["means3D"].device
        H, W = a["image_height"], a["image_width"]
        d = torch.full((H, W), -7.0, device=dev) if depth else None
        al = torch.full((H, W), -7.0, device=dev) if alpha else None
        R, color, radii, g, b, i = rp.RasterizeGaussiansCUDA(**a, raw_params=flags, out_depth=d, out_alpha=al, filter_3D=filt, **kw)
        return R, color, radii, d, al, (g, b, i)
    finally:
        rp._LIB_OVERRIDE = prev


def lists(lib_path, a, flags, filt, W, H):
    """(image, point list, tile ranges) of a training forward through the test-suite's view into the buffers"""
    import ctypes as C
    devapi = parity.devapi
    lib, dlib = capi.load(lib_path), devapi.load(lib_path)
    R, color, radii, _, _, (g, binning, img) = forward(lib_path, a, flags, filt)
    bv, iv = devapi.BinningView(), devapi.ImageView()
    capi.check(lib, dlib.gsr_view_image(C.c_void_p(img.data_ptr()), W, H, C.byref(iv)), "view_image")
    T = ((W + 15) // 16) * ((H + 15) // 16)
    ranges = parity._slice(img, iv.ranges, 2 * T, np.uint32)
    pl = np.zeros(0, np.uint32)
    if R:
        capi.check(lib, dlib.gsr_view_binning(C.c_void_p(binning.data_ptr()), R, W, H, C.byref(bv)), "view_binning")
        pl = parity._slice(binning, bv.point_list, R, np.uint32)
    return color, pl, ranges


def backward(lib_path, a, cam, flags, dpix, dD=None, dA=None, raw=0, filt=None, fwd_filt="same", **bkw):
    """forward (training) + backward with the filter; returns the tuple of RasterizeGaussiansBackwardCUDA and the radii"""
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        R, _, radii, g, b, i = rp.RasterizeGaussiansCUDA(**a, raw_params=flags | raw, filter_3D=filt if isinstance(fwd_filt, str) else fwd_filt)
        out = rp.RasterizeGaussiansBackwardCUDA(a["background"], a["means3D"], radii, a["colors"], a["scales"], a["rotations"], 1.0,
                                                a["cov3D_precomp"], a["viewmatrix"], a["projmatrix"], cam.tanfovx, cam.tanfovy, dpix,
                                                a["sh"], a["degree"], a["campos"], g, R, b, i, raw_params=raw, dL_ddepth=dD, dL_dalpha=dA,
                                                filter_3D=filt, **bkw)
        if a["means3D"].is_cuda:
            torch.cuda.synchronize()
        return out, radii
    finally:
        rp._LIB_OVERRIDE = prev


def raw_inputs(a, cl, dev):
    a = dict(a)
    a.update(opacity=fo._t(cl.opacity, dev), scales=fo._t(cl.scaling, dev), rotations=fo._t(cl.rotation, dev))
    return a


# ---------------------------------------------------------------------------------------------------- forward
def check_forward(lib_path, dev, oracle, cl, cam, bg, flags, filt=None, raw=False, antialias=False, maps=False, **kw):
    """The render with the bit against the oracle's render of (s'32, o'32) (radii and instance count equal, parity.RGB_L1_TOL);
    against the library's own render of the pre-filtered activated inputs without the bit (bit for bit on the emulator: image,
    radii, point list, ranges); and the image differs from the unfiltered render.  raw: the model's raw parameters with GSR_RAW_*;
    antialias: with GSR_ANTIALIAS, the reference then antialias_cases' route applied to (s', o'); maps: depth and alpha maps too."""
    if filt is None:
        filt, _ = scene_filter(cl)
    clf, c = filtered_cloud(cl, filt)
    a = fo.inputs(cl, cam, bg, dev, **kw)
    a_f = fo.inputs(clf, cam, bg, dev, **kw)
    ft = fo._t(filt, dev)
    lib_flags = flags | (aa.AA if antialias else 0)
    a_lib = raw_inputs(a, cl, dev) if raw else a
    if raw:
        lib_flags |= 7
    op = clf.get_opacity().reshape(-1)
    if antialias:
        op = op * aa.h32(clf, cam)
    ores, ocolor, oradii = aa.oracle_forward(oracle, a_f, clf, cam, bg, op)
    R1, c1, r1, d1, al1, _ = forward(lib_path, a_lib, lib_flags, ft, depth=maps, alpha=maps)
    R0, c0, r0, _, _, _ = forward(lib_path, a_lib, lib_flags)
    vis = oradii > 0
    rep = dict(rgb_L1=float(np.abs(c1.cpu().numpy() - ocolor).mean()), R=R1, changed=float((c1 - c0).abs().mean()),
               c_mean=float(c[vis].mean()) if vis.any() else 1.0)
    assert np.array_equal(r1.cpu().numpy(), oradii) and R1 == ores.R, rep
    assert rep["rgb_L1"] <= parity.RGB_L1_TOL, rep
    assert not torch.equal(c0, c1), "the bit did not change the image"
    if maps:
        od, oa, z = da.oracle_maps(oracle, dict(a_f, opacity=fo._t(op.reshape(-1, 1), torch.device("cpu"))), clf, cam)
        zmean = float(z[vis].mean()) if vis.any() else 1.0
        rep.update(depth_L1=float(np.abs(d1.cpu().numpy() - od).mean()) / zmean, alpha_L1=float(np.abs(al1.cpu().numpy() - oa).mean()))
        assert rep["depth_L1"] <= parity.RGB_L1_TOL and rep["alpha_L1"] <= parity.RGB_L1_TOL, rep
    # the library's own render of the pre-filtered ACTIVATED inputs, bit clear
    flags2 = flags | (aa.AA if antialias else 0)
    R2, c2, r2, _, _, _ = forward(lib_path, a_f, flags2)
    assert R2 == R1 and torch.equal(r2, r1), "radii or instance count differ from the render of the pre-filtered inputs"
    if dev.type == "cpu" and not raw:
        assert torch.equal(c2, c1), "the image differs from the render of the pre-filtered inputs"
        if not flags & fo.FORWARD_ONLY:
            i1, pl1, rg1 = lists(lib_path, a_lib, lib_flags, ft, cam.W, cam.H)
            i2, pl2, rg2 = lists(lib_path, a_f, flags2, None, cam.W, cam.H)
            # (GSR_CULL_EMPTY_TILES shortens the internal lists: the words of the R-entry buffer behind them are not written)
            assert flags & 8 or (np.array_equal(pl1, pl2) and np.array_equal(rg1, rg2)), "the lists differ"
            assert torch.equal(i1, i2)
    else:
        rep["own_L1"] = float((c2 - c1).abs().mean())
        assert rep["own_L1"] <= parity.RGB_L1_TOL, rep
    if not flags & fo.FORWARD_ONLY:
        _, cf, rf, _, _, _ = forward(lib_path, a_lib, lib_flags | fo.FORWARD_ONLY, ft)
        assert torch.equal(cf, c1) and torch.equal(rf, r1), "the forward-only form renders another image"
    print("measured:", rep)
    return rep


def check_zero_filter(lib_path, dev, cl, cam, bg, flags, raw=False, antialias=False, seed=0):
    """an all-zero filter with the bit set equals the bit clear: image, radii and every gradient (bit for bit; the gradients of two
    runs on the device differ in their last bits, there they are compared as two runs of one program are)"""
    rng = np.random.default_rng(seed)
    a = fo.inputs(cl, cam, bg, dev)
    rawbits = (7 if raw else 0) | (aa.AA if antialias else 0)
    if raw:
        a = raw_inputs(a, cl, dev)
    dpix = fo._t(rng.standard_normal((3, cam.H, cam.W)).astype(np.float32), dev)
    zero = torch.zeros(cl.xyz.shape[0], device=dev)
    R0, c0, r0, _, _, _ = forward(lib_path, a, flags | rawbits)
    R1, c1, r1, _, _, _ = forward(lib_path, a, flags | rawbits, zero)
    assert R0 == R1 and torch.equal(c0, c1) and torch.equal(r0, r1)
    g0, _ = backward(lib_path, a, cam, flags, dpix, raw=rawbits)
    g1, _ = backward(lib_path, a, cam, flags, dpix, raw=rawbits, filt=zero)
    for name, x, y in zip(GRAD_NAMES, g0, g1):
        if x is None or x.numel() == 0:
            continue
        if dev.type == "cpu":
            assert torch.equal(x, y), name
        else:
            assert parity.rel_l1(y.cpu().numpy(), x.cpu().numpy()) <= pg.DEVICE_RERUN_TOL, name


# ---------------------------------------------------------------------------------------------------- backward
def chain_rule64(s, o, filt, g_sp, g_op):
    """(dL/ds [P,3], dL/do [P], the part of dL/ds that comes through the opacity factor c) from the gradients of the filtered
    scale and opacity, by float64 autograd of filtered64()"""
    t64 = lambda x: torch.tensor(np.asarray(x, np.float64))
    S = t64(s).requires_grad_(True)
    O = t64(o.reshape(-1)).requires_grad_(True)
    sp, op, c = filtered64(S, O, t64(filt))
    gs, go = t64(g_sp), t64(g_op.reshape(-1))
    ds_scale, = torch.autograd.grad((sp * gs).sum(), S, retain_graph=True)
    ds_opac, do = torch.autograd.grad((op * go).sum(), (S, O))
    return (ds_scale + ds_opac).numpy(), do.numpy(), ds_opac.numpy()


def expected_grads(oracle, cl, cam, bg, filt, dpix, dD=None, dA=None, raw=False, antialias=False, **kw):
    """the gradients the library must return with the bit (module docstring), float64; the oracle's radii; the opacity-term part
    of dL_dscales"""
    clf, c = filtered_cloud(cl, filt)
    cpu = torch.device("cpu")
    a_f = fo.inputs(clf, cam, bg, cpu, **kw)
    if antialias:
        g, oradii, h, w, jt = aa.expected_grads(oracle, a_f, clf, cam, bg, dpix, dD, dA)
    else:
        g, oradii = da.oracle_grads(oracle, a_f, clf, cam, bg, dpix, dD, dA)
    vis = oradii > 0
    s, o = cl.get_scaling().astype(np.float64), cl.get_opacity().reshape(-1).astype(np.float64)
    g_sp = np.where(vis[:, None], g["dL_dscales"], 0.0)
    g_op = np.where(vis, g["dL_dopacity"].reshape(-1), 0.0)
    ds, do, ds_opac = chain_rule64(s, o, filt, g_sp, g_op)
    exp = dict(g)
    if raw:
        ds, ds_opac = ds * s, ds_opac * s
        do = do * o * (1 - o)
        # the rotation: the oracle differentiates the unit quaternion; the raw one adds the normalisation's Jacobian
        q = cl.rotation.astype(np.float64)
        n = np.linalg.norm(q, axis=1, keepdims=True)
        u, gq = q / n, g["dL_drotations"].astype(np.float64)
        exp["dL_drotations"] = (gq - u * (u * gq).sum(1, keepdims=True)) / n
    exp["dL_dscales"] = ds
    exp["dL_dopacity"] = do.reshape(g["dL_dopacity"].shape)
    return exp, oradii, ds_opac


def check_backward(lib_path, dev, oracle, cl, cam, bg, flags, filt=None, seed=0, maps=False, raw=False, antialias=False,
                   opacity_term_min=0.0):
    """backward with the bit (random dpix; maps: random dL_ddepth / dL_dalpha too) against expected_grads.  opacity_term_min: the
    share of the expected dL_dscales that comes through the opacity factor (g_o' o dc/ds) must be at least this -- where it is,
    a kernel that forgot the term could not pass the aggregate bar"""
    rng = np.random.default_rng(seed)
    if filt is None:
        filt, _ = scene_filter(cl)
    a = fo.inputs(cl, cam, bg, dev)
    if raw:
        a = raw_inputs(a, cl, dev)
    dpix = rng.standard_normal((3, cam.H, cam.W)).astype(np.float32)
    dD = rng.standard_normal((cam.H, cam.W)).astype(np.float32) if maps else None
    dA = rng.standard_normal((cam.H, cam.W)).astype(np.float32) if maps else None
    t = lambda x: None if x is None else fo._t(x, dev)
    rawbits = (7 if raw else 0) | (aa.AA if antialias else 0)
    out, radii = backward(lib_path, a, cam, flags, t(dpix), t(dD), t(dA), raw=rawbits, filt=t(filt))
    ref, oradii, ds_opac = expected_grads(oracle, cl, cam, bg, filt, dpix, dD, dA, raw=raw, antialias=antialias)
    assert np.array_equal(radii.cpu().numpy(), oradii)
    vis = oradii > 0
    rep = aa.compare_grads(out, ref, vis)
    rep["opacity_term_share_scales"] = float(np.abs(ds_opac).sum() / (np.abs(ref["dL_dscales"]).sum() + 1e-30))
    print("measured:", rep)
    assert rep["opacity_term_share_scales"] >= opacity_term_min, rep
    return rep


def check_errors(lib_path, dev, cl, cam, bg):
    """the error rules of gsr.h: the bit without the pointer, the bit with cov3D_precomp (forward and backward), a backward bit that
    differs from the forward call's, the bit through the multi-GPU exchange"""
    P = cl.xyz.shape[0]
    filt = torch.full((P,), 0.01, device=dev)
    dpix = torch.ones((3, cam.H, cam.W), device=dev)

    def refused(status, fn, what):
        try:
            fn()
        except capi.GsrError as e:
            assert e.status == status, (what, e.status)
        else:
            raise AssertionError(what + " was accepted")
    a = fo.inputs(cl, cam, bg, dev)
    refused(-1, lambda: forward(lib_path, a, F3), "GSR_FILTER_3D without a filter")
    a_cov = fo.inputs(cl, cam, bg, dev, use_cov3D_precomp=True)
    refused(-1, lambda: forward(lib_path, a_cov, 0, filt), "GSR_FILTER_3D with cov3D_precomp")
    refused(-1, lambda: backward(lib_path, a_cov, cam, 0, dpix, filt=filt, fwd_filt=None), "GSR_FILTER_3D with cov3D_precomp (backward)")
    refused(-1, lambda: backward(lib_path, a, cam, 0, dpix, raw=F3, fwd_filt=filt), "gsr_backward with the bit and no filter")
    # a mismatched bit, both ways
    refused(-1, lambda: backward(lib_path, a, cam, 0, dpix, filt=None, fwd_filt=filt), "a backward pass without the forward pass's bit")
    refused(-1, lambda: backward(lib_path, a, cam, 0, dpix, filt=filt, fwd_filt=None), "a backward pass with a bit the forward pass had not")
    view = torch.zeros((P, 3), device=dev)
    refused(-4, lambda: backward(lib_path, a, cam, 0, dpix, filt=filt, dL_dcolor_view=view), "the filter through the exchange")
    # ... and the matching pair runs
    out, _ = backward(lib_path, a, cam, 0, dpix, filt=filt)
    assert torch.isfinite(out[6]).all() and torch.isfinite(out[2]).all()


# ---------------------------------------------------------------------------------------------------- fused paths
def check_fused_geom_adam(lib_path, dev, cl, cam, bg, reg=False, seed=0):
    """raw_params = 7 | GSR_FILTER_3D + geom_adam with depth / alpha gradients: parameters and moments after the fused step match
    the unfused gradients (with the bit) + gsr_adam_step, to the bar of antialias_cases.check_fused_geom_adam.  reg: with non-zero
    geom_reg weights (the regulariser stays on the unfiltered values: the unfused gradients with it equal those without it plus
    its own terms of gsr.h)"""
    lib = capi.load(lib_path)
    rng = np.random.default_rng(seed)
    P = cl.xyz.shape[0]
    raw = capi.RAW_OPACITY | capi.RAW_SCALING | capi.RAW_ROTATION
    filt, _ = scene_filter(cl)
    ft = fo._t(filt, dev)
    dpix = fo._t(rng.standard_normal((3, cam.H, cam.W)).astype(np.float32), dev)
    dD = fo._t(rng.standard_normal((cam.H, cam.W)).astype(np.float32), dev)
    dA = fo._t(rng.standard_normal((cam.H, cam.W)).astype(np.float32), dev)
    names = ("xyz", "opacity", "scaling", "rotation")
    init = dict(xyz=cl.xyz, opacity=cl.opacity.reshape(P, 1), scaling=cl.scaling, rotation=cl.rotation)
    lrs = dict(xyz=1.6e-4, opacity=0.05, scaling=0.005, rotation=0.001)
    steps = dict(xyz=4, opacity=2, scaling=4, rotation=7)
    mom = {n: ((0.01 * rng.standard_normal(init[n].shape)).astype(np.float32), (1e-4 * rng.random(init[n].shape)).astype(np.float32))
           for n in names}
    greg = dict(w_opacity=0.01, w_scale=0.02, w_isotropic=0.03) if reg else None

    def run(fused, with_reg=True):
        st = {n: [fo._t(init[n].copy(), dev).clone(), fo._t(mom[n][0].copy(), dev).clone(), fo._t(mom[n][1].copy(), dev).clone()]
              for n in names}
        a = fo.inputs(cl, cam, bg, dev)
        a.update(means3D=st["xyz"][0], opacity=st["opacity"][0], scales=st["scaling"][0], rotations=st["rotation"][0])
        ga = dict(tensors=[(st[n][0], st[n][1], st[n][2], lrs[n], steps[n]) for n in names], beta1=0.9, beta2=0.999,
                  eps=1e-15) if fused else None
        out, radii = backward(lib_path, a, cam, 0, dpix, dD, dA, raw=raw, filt=ft, geom_adam=ga, training_outputs_only=fused,
                              geom_reg=greg if with_reg else None)
        return st, out, radii.cpu().numpy()

    st_ref, g_ref, radii = run(False)
    grads = dict(xyz=g_ref[3], opacity=g_ref[2], scaling=g_ref[6], rotation=g_ref[7])
    vis = radii > 0
    assert vis.any()
    if reg:
        # the regulariser's own terms, on the UNfiltered activated values (gsr.h: gsr_geom_reg), float64
        _, g_plain, _ = run(False, with_reg=False)
        o = cl.get_opacity().reshape(-1).astype(np.float64)
        s = cl.get_scaling().astype(np.float64)
        d = s - s.mean(1, keepdims=True)
        sg = np.sign(d)
        add_o = np.where(vis, greg["w_opacity"] * o * (1 - o), 0.0)
        add_s = np.where(vis[:, None], (greg["w_scale"] + greg["w_isotropic"] * (sg - sg.mean(1, keepdims=True))) * s, 0.0)
        e_o = parity.rel_l1(g_ref[2].cpu().numpy().reshape(-1), g_plain[2].cpu().numpy().reshape(-1).astype(np.float64) + add_o)
        e_s = parity.rel_l1(g_ref[6].cpu().numpy(), g_plain[6].cpu().numpy().astype(np.float64) + add_s)
        print("measured: geom_reg terms on the unfiltered values:", e_o, e_s)
        assert e_o <= parity.GRAD_REL_L1_TOL and e_s <= parity.GRAD_REL_L1_TOL, (e_o, e_s)
    for n in names:
        p_, m_, v_ = st_ref[n]
        gr = grads[n].contiguous()
        capi.check(lib, lib.gsr_adam_step(p_.data_ptr(), gr.data_ptr(), m_.data_ptr(), v_.data_ptr(), p_.numel(), lrs[n], 0.9, 0.999,
                                          1e-15, steps[n], 0, 0, lrs[n], None), "gsr_adam_step")
    if dev.type != "cpu":
        torch.cuda.synchronize()
    st_fus, _, _ = run(True)
    exact = dev.type == "cpu"
    for n in names:
        for k in range(3):
            x, y = st_fus[n][k].cpu().numpy(), st_ref[n][k].cpu().numpy()
            tol = max(lrs[n] * (2e-6 if exact else 2e-3), 1.2e-7 * np.abs(y).max()) if k == 0 else (1e-6 if exact else 2e-4) * np.abs(y).max()
            assert np.abs(x - y).max() <= tol, (n, k, np.abs(x - y).max(), tol)


def check_pose(lib_path, dev, oracle, cl, cam, bg, flags=(32, 64), seed=0):
    """The pose gradients with the bit by the rigid-motion identity of pose_grad_cases.py (its method (b), view-independent colour,
    random upstream gradient) on (s', o'): the identity's per-Gaussian gradients are the oracle's on the filtered inputs (the filter
    does not depend on the pose), the bar parity.GRAD_REL_L1_TOL on the mass-normalised error, as there"""
    filt, _ = scene_filter(cl)
    clf, _ = filtered_cloud(cl, filt)
    a = fo.inputs(cl, cam, bg, dev, use_colors_precomp=True)
    a_f = fo.inputs(clf, cam, bg, torch.device("cpu"), use_colors_precomp=True)
    dpix = np.random.default_rng(seed).standard_normal((3, cam.H, cam.W)).astype(np.float32)
    g, oradii = da.oracle_grads(oracle, a_f, clf, cam, bg, dpix, None, None)
    vis = oradii > 0
    terms = pg.identity_terms(cam, cl.xyz[vis], g["dL_dmeans3D"][vis], h_rot=g["dL_drotations"][vis], rot=cl.get_rotation()[vis])
    total, mass = terms.sum(0), np.abs(terms).sum(0)
    reps = []
    for f in flags:
        out, radii = backward(lib_path, a, cam, f, fo._t(dpix, dev), filt=fo._t(filt, dev), pose_grad=True)
        assert np.array_equal(radii.cpu().numpy(), oradii)
        gv, gp, gc = (t.cpu().numpy() for t in out[8:])
        assert not gc.any() and not gv.reshape(-1)[pg.VIEW_DEAD].any() and not gp.reshape(-1)[pg.PROJ_DEAD].any()
        err = np.abs(pg.chain_to_xi(gv, gp, gc, cam) - total) / mass
        rep = dict(flags=f, err=[float(e) for e in err], visible=int(vis.sum()))
        print("measured:", rep)
        assert (err <= parity.GRAD_REL_L1_TOL).all(), rep
        reps.append(rep)
    return reps


# ---------------------------------------------------------------------------------------------------- default untouched
def default_hashes(lib_path, dev, cl, cam, bg, parent_convention, seed=0):
    """sha256 of image, radii and every gradient of a run with the bit clear.  parent_convention: the calls exactly as before this
    feature existed (no filter_3D argument); otherwise filter_3D=None passed through the new keyword"""
    rng = np.random.default_rng(seed)
    a = fo.inputs(cl, cam, bg, dev)
    dpix = fo._t(rng.standard_normal((3, cam.H, cam.W)).astype(np.float32), dev)
    kw = {} if parent_convention else dict(filter_3D=None)
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        R, color, radii, g, b, i = rp.RasterizeGaussiansCUDA(**a, **kw)
        out = rp.RasterizeGaussiansBackwardCUDA(a["background"], a["means3D"], radii, a["colors"], a["scales"], a["rotations"], 1.0,
                                                a["cov3D_precomp"], a["viewmatrix"], a["projmatrix"], cam.tanfovx, cam.tanfovy, dpix,
                                                a["sh"], 3, a["campos"], g, R, b, i, **kw)
    finally:
        rp._LIB_OVERRIDE = prev
    hs = {"R": R}
    for name, t in zip(("image", "radii") + GRAD_NAMES, (color, radii) + tuple(out)):
        if t is not None:
            hs[name] = hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
    return hs


# ---------------------------------------------------------------------------------------------------- autograd node and the hosts
def check_autograd(lib_path, dev, oracle, cl, seed=5):
    """The autograd node (GaussianRasterizer with filter_3D_): the filter is a non-differentiable input (it gets no gradient even
    when it requires one), and a loss on the image back-propagates to the gradients of the float64 restatement -- the oracle's on
    (s', o') through chain_rule64 -- within parity.GRAD_REL_L1_TOL; under torch.no_grad() the forward-only path renders the same
    image"""
    from photo_slam_amd.gaussian_rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    cam = cl.cameras[0]
    bg = np.array([0.2, 0.5, 0.1], np.float32)
    rng = np.random.default_rng(seed)
    t = lambda x: fo._t(x, dev)
    filt, _ = scene_filter(cl)
    dpix = rng.standard_normal((3, cam.H, cam.W)).astype(np.float32)
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        ft = t(filt).requires_grad_(True)

        def settings(f):
            return GaussianRasterizationSettings(cam.H, cam.W, cam.tanfovx, cam.tanfovy, t(bg), 1.0, t(cam.viewmatrix), t(cam.projmatrix),
                                                 3, t(cam.campos), False, filter_3D_=f)
        leaf = lambda x: t(x).clone().requires_grad_(True)
        L = dict(means3D=leaf(cl.xyz), means2D=torch.zeros((cl.xyz.shape[0], 3), device=dev, requires_grad=True),
                 opacities=leaf(cl.get_opacity()), shs=leaf(cl.get_features()), scales=leaf(cl.get_scaling()),
                 rotations=leaf(cl.get_rotation()))
        color, radii = GaussianRasterizer(settings(ft))(L["means3D"], L["means2D"], L["opacities"], True, False, True, True, False,
                                                        shs=L["shs"], scales=L["scales"], rotations=L["rotations"])
        (color * t(dpix)).sum().backward()
        assert ft.grad is None, "the filter received a gradient"
        ref, oradii, _ = expected_grads(oracle, cl, cam, bg, filt, dpix)
        assert np.array_equal(radii.cpu().numpy(), oradii)
        got = dict(dL_dmeans3D=L["means3D"].grad, dL_dmeans2D=L["means2D"].grad, dL_dopacity=L["opacities"].grad,
                   dL_dscales=L["scales"].grad, dL_drotations=L["rotations"].grad, dL_dsh=L["shs"].grad)
        rep = {}
        for name, x in got.items():
            assert x is not None and torch.isfinite(x).all(), name
            rep[name] = parity.rel_l1(x.cpu().numpy().reshape(ref[name].shape), ref[name])
            assert rep[name] <= parity.GRAD_REL_L1_TOL, (name, rep)
        print("measured:", rep)
        with torch.no_grad():
            c2 = GaussianRasterizer(settings(ft))(L["means3D"], L["means2D"], L["opacities"], True, False, True, True, False,
                                                  shs=L["shs"], scales=L["scales"], rotations=L["rotations"])[0]
            c3 = GaussianRasterizer(settings(None))(L["means3D"], L["means2D"], L["opacities"], True, False, True, True, False,
                                                    shs=L["shs"], scales=L["scales"], rotations=L["rotations"])[0]
        assert rp.lastForwardOnly() == 1
        assert torch.equal(c2, color.detach()) and not torch.equal(c3, c2)
    finally:
        rp._LIB_OVERRIDE = prev


def camera_tuples(rows):
    """the rows as the (viewmatrix, focal_x, focal_y, width, height) tuples TrainStep.setFilterCameras takes"""
    return [(torch.from_numpy(np.ascontiguousarray(r[:16].reshape(4, 4))), float(r[16]), float(r[17]), float(r[18]), float(r[19])) for r in rows]


def _python_trainer(cl, dev, rows, filter3d=True, interval=4, **kw):
    from photo_slam_amd.gaussian_model import GaussianModel, GaussianOptimizationParams
    from photo_slam_amd.gaussian_renderer import GaussianPipelineParams
    from photo_slam_amd.trainer import TrainStep
    g = GaussianModel.from_cloud(copy.deepcopy(cl), device=dev)
    opt = GaussianOptimizationParams()
    for k, v in kw.pop("opt", {}).items():
        setattr(opt, k, v)
    g.trainingSetup(opt)
    ts = TrainStep(g, opt, GaussianPipelineParams(), torch.zeros(3, device=dev), cameras_extent=float(cl.extent), seed=7,
                   filter3d=filter3d, **kw)
    ts.filter3d_interval_ = interval
    if rows is not None:
        ts.setFilterCameras(camera_tuples(rows))
    return g, ts


def _cpp_trainer(ops, cl, dev, rows, filter3d=True, interval=4, options=None):
    from photo_slam_amd.gaussian_model import GaussianModel
    g0 = GaussianModel.from_cloud(copy.deepcopy(cl), device=dev)
    h = ops.trainer_create(g0.xyz_.detach(), g0.features_.detach(), g0.opacity_.detach(), g0.scaling_.detach(), g0.rotation_.detach(),
                           3, float(cl.extent), torch.zeros(3, device=dev))
    o = {"seed": 7.0, "cameras_extent": float(cl.extent), "filter3d": 1.0 if filter3d else 0.0, "filter3d_interval": float(interval)}
    o.update(options or {})
    ops.trainer_set_options(h, o)
    if rows is not None:
        ops.trainer_set_filter_cameras(h, fo._t(rows, dev))
    return h


# The two hosts on the emulator: the loss sequences and the filters are bit-identical, the parameters after the steps and a rendered
# view are not -- WITHOUT the filter either.  Measured on the emulator, 600 Gaussians, 6 steps on the mixed-resolution pair, filter3d_
# OFF in both hosts: the largest absolute difference of a parameter tensor 2.4e-7 (xyz 1.2e-7, features 7.5e-9, opacity 2.4e-7,
# scaling 2.4e-7, rotation 6.0e-8: one unit in the last place of single entries), of the rendered view 1.2e-7; with it ON 1.2e-7 and
# 6.0e-8.  The gap predates this feature (tests/test_cpp_host.py holds the hosts to rtol 1e-4 for it), so "exactly" is asserted for
# what IS exact -- losses and filter -- and parameters and view are held to HOST_GAP: 4 x the figures measured with the filter off,
# which check_hosts re-measures (the off pair must stay inside the same bar: the bar is not the filter's).
HOST_GAP = dict(param_abs_max_measured=2.4e-7, view_abs_max_measured=1.2e-7, factor=4)


def check_hosts(ops, lib_path, dev, cl, steps=6, exact=True):
    """Python TrainStep(filter3d=True) and the C++ TrainStep (option filter3d) over `steps` steps on a mixed-resolution pair of
    keyframes, the filter recomputed every 4 iterations.  exact (the emulator): the same loss sequence and the same filter, bit for
    bit; parameters and render_view / renderView within HOST_GAP, the gap the hosts have without the filter (re-measured here).
    Not exact (the device): the tolerances antialias_cases.check_hosts holds the hosts to.  The filter is really on in both (the
    first loss differs from the run without it)."""
    cams, kfs, gts, masks = aa.mixed_resolution_data(cl, dev)
    args = [da._cam_args(c, dev) for c in cams]
    rows = camera_rows(cl.cameras)   # (the finest level each keyframe is trained at)
    n = len(cams)

    def cpp(on):
        h = _cpp_trainer(ops, cl, dev, rows, filter3d=on)
        try:
            losses = []
            for it in range(steps):
                losses.append(ops.trainer_render_and_backward(h, *args[it % n], gts[it % n], masks[it % n]).item())
                ops.trainer_finish(h)
            view = ops.trainer_render_view(h, *args[1])
            return losses, [p.detach().clone() for p in ops.trainer_params(h)], view, ops.trainer_filter_3d(h).clone()
        finally:
            ops.trainer_destroy(h)

    def py(on):
        prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
        try:
            g, ts = _python_trainer(cl, dev, rows, filter3d=on)
            losses = [ts.trainForOneIteration(kfs[it % n], gts[it % n], masks[it % n], sync_loss=False).item() for it in range(steps)]
            view = ts.render_view(kfs[1])
            g.sync_features()
            return losses, [p.detach().clone() for p in g.params()], view, g.filter_3D_
        finally:
            rp._LIB_OVERRIDE = prev

    runs = {on: (cpp(on), py(on)) for on in (True, False)}
    (losses_cpp, params_cpp, view_cpp, filt_cpp), (losses_py, params_py, view_py, filt_py) = runs[True]
    (losses_cpp_off, _, _, filt_off), (losses_py_off, _, _, filt_py_off) = runs[False]
    assert filt_off.numel() == 0 and filt_py_off is None and filt_cpp.numel() == cl.xyz.shape[0]
    assert losses_cpp[0] != losses_cpp_off[0], "the C++ host's option did not reach the rasterizer"
    assert losses_py[0] != losses_py_off[0], "TrainStep(filter3d=True) did not reach the rasterizer"
    print("measured: losses", losses_cpp, losses_py)
    if exact:
        assert losses_cpp == losses_py, (losses_cpp, losses_py)
        assert torch.equal(filt_cpp, filt_py)
        for on in (False, True):
            (lc, pc, vc, _), (lp, pp, vp, _) = runs[on]
            assert lc == lp, (on, lc, lp)
            gap_p = max(float((x - y).abs().max()) for x, y in zip(pc, pp))
            gap_v = float((vc - vp).abs().max())
            print("measured: hosts, filter", on, "parameters max abs", gap_p, "view max abs", gap_v)
            assert gap_p <= HOST_GAP["factor"] * HOST_GAP["param_abs_max_measured"], (on, gap_p)
            assert gap_v <= HOST_GAP["factor"] * HOST_GAP["view_abs_max_measured"], (on, gap_v)
    else:
        assert np.allclose(losses_cpp, losses_py, rtol=1e-5), (losses_cpp, losses_py)
        for x, y in zip(params_cpp, params_py):
            assert parity.rel_l1(x.cpu().numpy(), y.cpu().numpy()) <= 1e-3
        assert float((view_cpp - view_py).abs().max()) <= 1e-3
        assert parity.rel_l1(filt_cpp.cpu().numpy(), filt_py.cpu().numpy()) <= 1e-3


def check_recompute_python(lib_path, dev, cl):
    """Python host: the filter has P entries at every render and is recomputed -- against filter32 at the positions of that moment,
    bit for bit -- after a densification and after increasePcd; filter3d_ on without cameras throws, and so does a process group"""
    cams, kfs, gts, masks = aa.mixed_resolution_data(cl, dev)
    rows = camera_rows(cl.cameras)
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    real_forward, real_filter = rp.RasterizeGaussiansCUDA, rp.filter3D
    renders, computes = [], []

    def forward(*a, **kw):
        f = kw.get("filter_3D")
        assert f is not None and f.shape[0] == a[1].shape[0], "a render without a filter of P entries"
        renders.append(int(f.shape[0]))
        return real_forward(*a, **kw)

    def filter3d(means3D, cameras, variance=0.2, out=None):
        got = real_filter(means3D, cameras, variance, out)
        want, _ = filter32(means3D.detach().cpu().numpy(), cameras.cpu().numpy(), variance)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), "the recomputed filter differs from the restatement"
        computes.append(int(means3D.shape[0]))
        return got
    rp.RasterizeGaussiansCUDA, rp.filter3D = forward, filter3d
    try:
        g, ts = _python_trainer(cl, dev, rows, interval=100, densify=True,
                                opt=dict(densify_from_iter_=1, densification_interval_=3, opacity_reset_interval_=1000,
                                         densify_grad_threshold_=2e-5))
        P0 = g.xyz_.shape[0]
        for it in range(5):
            ts.trainForOneIteration(kfs[it % 2], gts[it % 2], masks[it % 2], sync_loss=False)
        assert ts.last_densify_ is not None and g.xyz_.shape[0] != P0, "no densification happened"
        assert computes == [P0, g.xyz_.shape[0]], computes   # once at first use, once after the densification
        assert g.filter_3D_ is not None and g.filter_3D_.shape[0] == g.xyz_.shape[0]
        rng = np.random.default_rng(0)
        pts = torch.from_numpy((cl.xyz[:50] + 0.01 * rng.standard_normal((50, 3))).astype(np.float32)).to(dev)
        g.increasePcd(pts, torch.rand(50, 3).to(dev), 6)
        assert g.filter_3D_ is None, "increasePcd left a stale filter"
        ts.render_view(kfs[1])
        assert computes[-1] == g.xyz_.shape[0] and len(computes) == 3 and renders[-1] == g.xyz_.shape[0]
        assert len(renders) == 6
        # on without cameras; with a process group
        g2, ts2 = _python_trainer(cl, dev, None)
        for bad, what in ((ts2, "no cameras"), (_python_trainer(cl, dev, rows, world_size=2)[1], "process group")):
            try:
                bad.trainForOneIteration(kfs[0], gts[0], masks[0], sync_loss=False)
            except RuntimeError as e:
                assert what in str(e), str(e)
            else:
                raise AssertionError("filter3d_ " + what + ": no error")
        # a model without tensors yet (the start-up of seedFromDepth): the cameras are taken, nothing is dereferenced
        from photo_slam_amd.gaussian_model import GaussianModel, GaussianOptimizationParams
        from photo_slam_amd.gaussian_renderer import GaussianPipelineParams
        from photo_slam_amd.trainer import TrainStep
        ts3 = TrainStep(GaussianModel(3, dev), GaussianOptimizationParams(), GaussianPipelineParams(), torch.zeros(3, device=dev),
                        cameras_extent=float(cl.extent), filter3d=True)
        ts3.setFilterCameras(camera_tuples(rows))
        assert ts3.filter_cameras_.shape == (len(rows), 20) and ts3.viewFilter3D() is None
    finally:
        rp.RasterizeGaussiansCUDA, rp.filter3D = real_forward, real_filter
        rp._LIB_OVERRIDE = prev


def check_recompute_cpp(ops, dev, cl):
    """C++ host: after a densification and after increasePcd the model's filter is undefined, the next render recomputes it with P
    entries -- against filter32 at the positions of that moment, bit for bit.  Every render is counted (TrainStep::filter3d_renders_:
    the renders that were handed the filter; RasterizeGaussiansCUDA itself refuses a filter whose row count is not P) and followed
    by a look at the filter's size; filter3d on without cameras throws, and so does the exchange; setFilterCameras on a model
    without tensors works"""
    cams, kfs, gts, masks = aa.mixed_resolution_data(cl, dev)
    args = [da._cam_args(c, dev) for c in cams]
    rows = camera_rows(cl.cameras)

    renders = [0]

    def rendered(h):
        """one more render was handed a filter, and the filter has P entries"""
        renders[0] += 1
        assert ops.trainer_filter3d_renders(h) == renders[0], (ops.trainer_filter3d_renders(h), renders[0])
        assert ops.trainer_filter_3d(h).numel() == ops.trainer_params(h)[0].shape[0]

    def same(h, xyz):
        rendered(h)
        got = ops.trainer_filter_3d(h).cpu().numpy()
        want, _ = filter32(xyz.detach().cpu().numpy(), rows)
        assert got.shape == want.shape, (got.shape, want.shape)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), float(np.abs(got - want).max())
    h = _cpp_trainer(ops, cl, dev, rows, interval=100)
    try:
        xyz = ops.trainer_params(h)[0].detach().clone()
        ops.trainer_render_and_backward(h, *args[0], gts[0], masks[0])
        same(h, xyz)
        ops.trainer_finish(h)
        for k in range(2):   # (steps that neither recompute nor invalidate: the filter of P entries is carried on)
            ops.trainer_render_and_backward(h, *args[k], gts[k], masks[k])
            rendered(h)
            ops.trainer_finish(h)
        ops.trainer_render_view_depth(h, *args[0])
        rendered(h)
        ops.trainer_densify_and_prune(h, 2e-5, 0.005, float(cl.extent), 0, 7)
        assert ops.trainer_filter_3d(h).numel() == 0, "densifyAndPrune left a stale filter"
        xyz = ops.trainer_params(h)[0].detach().clone()
        assert xyz.shape[0] != cl.xyz.shape[0]
        ops.trainer_render_view(h, *args[1])
        same(h, xyz)
        rng = np.random.default_rng(0)
        pts = torch.from_numpy((cl.xyz[:50] + 0.01 * rng.standard_normal((50, 3))).astype(np.float32)).to(dev)
        ops.trainer_increase_pcd(h, pts, torch.rand(50, 3).to(dev), 6, False)
        assert ops.trainer_filter_3d(h).numel() == 0, "increasePcd left a stale filter"
        xyz = ops.trainer_params(h)[0].detach().clone()
        ops.trainer_render_and_backward(h, *args[0], gts[0], masks[0])
        same(h, xyz)
    finally:
        ops.trainer_destroy(h)
    # a model without tensors yet (the start-up of seedFromDepth): the cameras are taken, nothing is dereferenced
    h = ops.trainer_create_empty(3, torch.zeros(3, device=dev))
    try:
        ops.trainer_set_options(h, {"filter3d": 1.0})
        ops.trainer_set_filter_cameras(h, fo._t(rows, dev))
        assert ops.trainer_filter_3d(h).numel() == 0
    finally:
        ops.trainer_destroy(h)
    for options, what in ((None, "no cameras"), ("exchange", "process group")):
        h = _cpp_trainer(ops, cl, dev, None if options is None else rows)
        try:
            if options:
                ops.trainer_set_factored_exchange(h, True)
            try:
                ops.trainer_render_and_backward(h, *args[0], gts[0], masks[0])
            except RuntimeError as e:
                assert what in str(e), str(e)
            else:
                raise AssertionError("filter3d " + what + ": no error")
        finally:
            ops.trainer_destroy(h)


# ---------------------------------------------------------------------------------------------------- PLY
def check_ply(ops, lib_path, dev, oracle, cl, tmp_path):
    """Round trip with and without the property in both hosts and across them; with the filter undefined the bytes are those of a
    model that never had one; the fused export, loaded and rendered WITHOUT the bit, matches the filtered render within
    parity.RGB_L1_TOL"""
    from photo_slam_amd import ply_io
    from photo_slam_amd.gaussian_model import GaussianModel
    rows = camera_rows(cl.cameras)
    cam = cl.cameras[0]
    bg = np.array([0.2, 0.5, 0.1], np.float32)
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        g = GaussianModel.from_cloud(copy.deepcopy(cl), device=dev)
        plain, with_f, fused = (str(tmp_path / n) for n in ("plain.ply", "filter.ply", "fused.ply"))
        g.savePly(plain)
        filt = g.computeFilter3D(fo._t(rows, dev))
        g.savePly(with_f)
        g.savePly(fused, fused=True)
        g.filter_3D_ = None
        again = str(tmp_path / "plain2.ply")
        g.savePly(again)
        assert open(plain, "rb").read() == open(again, "rb").read()
        n = lambda t: t.detach().cpu().numpy()
        parent = str(tmp_path / "parent.ply")
        ply_io.save_ply(parent, n(g.xyz_), n(g.features_), n(g.opacity_), n(g.scaling_), n(g.rotation_))   # the call as it was
        assert open(plain, "rb").read() == open(parent, "rb").read()
        assert b"filter_3D" not in open(plain, "rb").read(4096) and b"filter_3D" not in open(fused, "rb").read(4096)
        assert len(open(with_f, "rb").read()) - len(open(plain, "rb").read()) == 4 * cl.xyz.shape[0] + len("property float filter_3D\n")
        g1, g2 = GaussianModel.loadPly(plain, device=dev), GaussianModel.loadPly(with_f, device=dev)
        assert g1.filter_3D_ is None and torch.equal(g2.filter_3D_, filt)
        for a, b in zip(g2.params(), g.params()):
            assert torch.equal(a.detach(), b.detach())
        # the C++ host: reads the property, writes the same bytes back, and drops it with the filter
        h = ops.trainer_create_from_ply(with_f, 3, float(cl.extent), torch.zeros(3, device=dev))
        try:
            assert torch.equal(ops.trainer_filter_3d(h), filt)
            back, back_fused = str(tmp_path / "cpp.ply"), str(tmp_path / "cpp_fused.ply")
            ops.trainer_save_ply(h, back)
            assert open(back, "rb").read() == open(with_f, "rb").read()
            ops.trainer_save_ply_fused(h, back_fused)
            sp, op = ops.trainer_filtered_activations(h)
            with torch.no_grad():
                assert torch.allclose(sp, g2.getScalingWithFilter3D(), rtol=1e-6) and torch.allclose(op, g2.getOpacityWithFilter3D(), rtol=1e-6)
        finally:
            ops.trainer_destroy(h)
        h = ops.trainer_create_from_ply(plain, 3, float(cl.extent), torch.zeros(3, device=dev))
        try:
            assert ops.trainer_filter_3d(h).numel() == 0
            back = str(tmp_path / "cpp_plain.ply")
            ops.trainer_save_ply(h, back)
            assert open(back, "rb").read() == open(plain, "rb").read()
        finally:
            ops.trainer_destroy(h)
        # the fused export rendered WITHOUT the bit against the filtered render (raw parameters in the rasterizer, both)
        a = raw_inputs(fo.inputs(cl, cam, bg, dev), cl, dev)
        _, want, r_want, _, _, _ = forward(lib_path, a, 7, filt)
        for path in (fused, back_fused):
            gf = GaussianModel.loadPly(path, device=dev)
            assert gf.filter_3D_ is None
            af = dict(a, opacity=gf.opacity_.detach(), scales=gf.scaling_.detach(), rotations=gf.rotation_.detach())
            _, got, r_got, _, _, _ = forward(lib_path, af, 7)
            err = float((got - want).abs().mean())
            print("measured: fused export against the filtered render, RGB L1", err)
            assert err <= parity.RGB_L1_TOL, err
    finally:
        rp._LIB_OVERRIDE = prev
