"""Shared checks of anti-aliased rendering (GSR_ANTIALIAS, include/gsr.h) for the emulator tests (test_antialias.py) and the GPU tests
(test_gpu_antialias.py).

The CPU oracle serves as the reference unchanged: the bit multiplies the activated opacity by h = sqrt(max(0.000025, det Sigma /
det(Sigma + 0.3 I))) and changes nothing else, so the render with the bit is the oracle's render with opacities o h.  h32() restates
h in numpy float32 in the operation order gsr.h documents; h64() restates it in float64 torch with autograd, including the
frustum clamp of computeCov2D and its gradient rule.  Neither shares code with the kernels.

Backward: the oracle's backward pass on (o' = o h32) gives g' = dL/do' and every gradient with o' held independent.  With the
bit the library must return dL_dopacity = g' h and, for the geometry, the oracle's values plus J_h^T (g' o), J_h from autograd of
h64().

Bars: the aggregate and per-row bars of tests/parity.py, unchanged, for everything.  det Sigma = a c - b b cancels for
needle-shaped Gaussians, so float32 and float64 may disagree on h there.  The gap between the two RESTATEMENTS (neither is the code
under test) was measured on the scenes of test_forward_only.SHAPES: relative L1 of h over the visible Gaussians 3.5e-8 ... 6.3e-8.
Times 4 for operation-order freedom that is 2.5e-7, far inside parity.GRAD_REL_L1_TOL = 1e-4 and the row bars, so no bar of its
own was needed: every comparison below uses the existing bars (measured on the emulator: aggregates <= 1.5e-6, rows <= 2e-3 at
the maximum).  RESTATEMENT_GAP records the measurement; test_antialias.py re-measures it and holds it to that figure."""
import hashlib

import numpy as np
import torch

import depth_alpha_cases as da
import forward_only_cases as fo
import parity
import pose_grad_cases as pg
from photo_slam_amd import capi
from photo_slam_amd import rasterize_points as rp

AA = capi.ANTIALIAS
H2_MIN = 0.000025
LOWPASS = 0.3
# the measured float32-numpy / float64 gap of the two restatements of h over test_forward_only.SHAPES (relative L1, visible
# Gaussians): at most 6.3e-8; held to 4 x that (operation-order freedom)
RESTATEMENT_GAP = dict(h_rel_l1_measured=6.3e-8, factor=4)
GRAD_NAMES = da.GRAD_NAMES
ROW_CHECKED = da.ROW_CHECKED


def _np(t):
    return None if t is None or t.numel() == 0 else t.detach().cpu().numpy()


# ---------------------------------------------------------------------------------------------------- h, restated twice
def cov3d32(scales, rots):
    """computeCov3D (forward.cu:118-152) in float32, its operation order, from activated scales / unit quaternions"""
    f = np.float32
    s = scales.astype(f)
    q = rots.astype(f)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    one, two = f(1), f(2)
    R = [[one - two * (y * y + z * z), two * (x * y - r * z), two * (x * z + r * y)],
         [two * (x * y + r * z), one - two * (x * x + z * z), two * (y * z - r * x)],
         [two * (x * z - r * y), two * (y * z + r * x), one - two * (x * x + y * y)]]
    M = [[f(1) * s[:, k] * R[c][k] for k in range(3)] for c in range(3)]
    dot = lambda a, b: (M[a][0] * M[b][0] + M[a][1] * M[b][1]) + M[a][2] * M[b][2]
    return np.stack([dot(0, 0), dot(1, 0), dot(2, 0), dot(1, 1), dot(2, 1), dot(2, 2)], 1)


def cov2d32(cl, cam, cov3D=None):
    """(a, b, c) of the projected covariance BEFORE the low-pass, computeCov2D (forward.cu:74-113) in float32, its operation order"""
    f = np.float32
    V = cam.viewmatrix.reshape(-1).astype(f)
    x, y, z = (cl.xyz[:, i].astype(f) for i in range(3))
    c3 = cov3d32(cl.get_scaling(), cl.get_rotation()) if cov3D is None else cov3D.astype(f)
    with np.errstate(all="ignore"):
        tx = ((V[0] * x + V[4] * y) + V[8] * z) + V[12]
        ty = ((V[1] * x + V[5] * y) + V[9] * z) + V[13]
        tz = ((V[2] * x + V[6] * y) + V[10] * z) + V[14]
        limx, limy = f(1.3) * f(cam.tanfovx), f(1.3) * f(cam.tanfovy)
        fx, fy = f(cam.W) / (f(2) * f(cam.tanfovx)), f(cam.H) / (f(2) * f(cam.tanfovy))
        tx = np.minimum(limx, np.maximum(-limx, tx / tz)) * tz
        ty = np.minimum(limy, np.maximum(-limy, ty / tz)) * tz
        J00, J02 = fx / tz, -(fx * tx) / (tz * tz)
        J11, J12 = fy / tz, -(fy * ty) / (tz * tz)
        T00, T01, T02 = V[0] * J00 + V[2] * J02, V[4] * J00 + V[6] * J02, V[8] * J00 + V[10] * J02
        T10, T11, T12 = V[1] * J11 + V[2] * J12, V[5] * J11 + V[6] * J12, V[9] * J11 + V[10] * J12
        A00 = (T00 * c3[:, 0] + T01 * c3[:, 1]) + T02 * c3[:, 2]
        A10 = (T00 * c3[:, 1] + T01 * c3[:, 3]) + T02 * c3[:, 4]
        A20 = (T00 * c3[:, 2] + T01 * c3[:, 4]) + T02 * c3[:, 5]
        A01 = (T10 * c3[:, 0] + T11 * c3[:, 1]) + T12 * c3[:, 2]
        A11 = (T10 * c3[:, 1] + T11 * c3[:, 3]) + T12 * c3[:, 4]
        A21 = (T10 * c3[:, 2] + T11 * c3[:, 4]) + T12 * c3[:, 5]
        a = (A00 * T00 + A10 * T01) + A20 * T02
        b = (A01 * T00 + A11 * T01) + A21 * T02
        c = (A01 * T10 + A11 * T11) + A21 * T12
    return a, b, c


def h32(cl, cam, cov3D=None):
    """h per Gaussian in numpy float32, in the operation order of include/gsr.h (GSR_ANTIALIAS); 1 where it is not a number (such a
    Gaussian is culled)"""
    f = np.float32
    a, b, c = cov2d32(cl, cam, cov3D)
    with np.errstate(all="ignore"):
        a1, c1 = a + f(LOWPASS), c + f(LOWPASS)
        det1 = a1 * c1 - b * b
        det0 = a * c - b * b
        h2 = np.maximum(f(H2_MIN), det0 / det1)
        h = np.sqrt(h2).astype(f)
    return np.where(np.isfinite(h), h, f(1))


def h64(xyz, view, cam, scales=None, rots=None, cov3D=None):
    """h per Gaussian as a float64 torch expression of (xyz [P,3], view [16] or [4,4], scales + rots or cov3D [P,6]).  The frustum
    clamp of tx / tz, ty / tz at +-1.3 tanfov follows the reference's gradient rule (backward.cu:185-190): a clamped coordinate is a
    constant (nothing flows to the mean through it), the unclamped one is the variable."""
    V = view.reshape(-1)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if cov3D is None:
        r, qx, qy, qz = rots[:, 0], rots[:, 1], rots[:, 2], rots[:, 3]
        R = torch.stack([1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - r * qz), 2 * (qx * qz + r * qy),
                         2 * (qx * qy + r * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - r * qx),
                         2 * (qx * qz - r * qy), 2 * (qy * qz + r * qx), 1 - 2 * (qx * qx + qy * qy)], 1).reshape(-1, 3, 3)
        M = R * scales[:, None, :]
        S = M @ M.transpose(1, 2)
    else:
        c = cov3D
        S = torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], 1).reshape(-1, 3, 3)
    tx = V[0] * x + V[4] * y + V[8] * z + V[12]
    ty = V[1] * x + V[5] * y + V[9] * z + V[13]
    tz = V[2] * x + V[6] * y + V[10] * z + V[14]
    limx, limy = 1.3 * float(np.float32(cam.tanfovx)), 1.3 * float(np.float32(cam.tanfovy))
    fx, fy = cam.W / (2.0 * float(np.float32(cam.tanfovx))), cam.H / (2.0 * float(np.float32(cam.tanfovy)))

    def clamp(t, lim):   # t' = clamp(t / tz) * tz; clamped: a constant
        ratio = t / tz
        out = ratio.detach().clamp(-lim, lim) * tz.detach()
        return torch.where((ratio.detach() < -lim) | (ratio.detach() > lim), out, t)
    tx, ty = clamp(tx, limx), clamp(ty, limy)
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -(fx * tx) / (tz * tz), zero, fy / tz, -(fy * ty) / (tz * tz)], 1).reshape(-1, 2, 3)
    Wm = V.reshape(4, 4)[:3, :3].T    # W2C rotation: W(r, c) = V[4c + r]
    T = J @ Wm                        # [P,2,3]
    C2 = T @ S @ T.transpose(1, 2)
    a, b, c = C2[:, 0, 0], C2[:, 0, 1], C2[:, 1, 1]
    det0 = a * c - b * b
    det1 = (a + LOWPASS) * (c + LOWPASS) - b * b
    ratio = det0 / det1
    return torch.sqrt(torch.where(ratio > H2_MIN, ratio, torch.full_like(ratio, H2_MIN)))


def h_jacobian_term(cl, cam, weight, cov3D=None):
    """J_h^T weight: dict of float64 numpy gradients of sum_i weight_i h_i with respect to xyz, scales, rots (or cov3D) and view [4,4]
    (weight: [P], zero on culled Gaussians)"""
    g64 = lambda a: torch.tensor(np.asarray(a, np.float64), requires_grad=True)
    xyz, view = g64(cl.xyz), g64(cam.viewmatrix)
    if cov3D is None:
        s, q = g64(cl.get_scaling()), g64(cl.get_rotation())
        h = h64(xyz, view, cam, scales=s, rots=q)
    else:
        c = g64(cov3D)
        h = h64(xyz, view, cam, cov3D=c)
    w = torch.tensor(np.asarray(weight, np.float64))
    live = w != 0
    (h[live] * w[live]).sum().backward()
    z = lambda t: np.zeros(t.shape) if t.grad is None else t.grad.numpy()
    out = dict(dL_dmeans3D=z(xyz), view=z(view))
    if cov3D is None:
        out.update(dL_dscales=z(s), dL_drotations=z(q))
    else:
        out.update(dL_dcov3D=z(c))
    return out


def restatement_gap(cl, cam, seed=0):
    """the float32-numpy / float64 gap of the two restatements on the visible (z > 0.2) Gaussians: relative L1 of h"""
    with torch.no_grad():
        t64 = lambda a: torch.tensor(np.asarray(a, np.float64))
        h_64 = h64(t64(cl.xyz), t64(cam.viewmatrix), cam, scales=t64(cl.get_scaling()), rots=t64(cl.get_rotation())).numpy()
    z = da.view_z(cl, cam)
    vis = z > 0.2
    return parity.rel_l1(h32(cl, cam)[vis], h_64[vis])


# ---------------------------------------------------------------------------------------------------- forward
def oracle_forward(oracle, a, cl, cam, bg, opacity):
    """the oracle's render of the inputs `a` (fo.inputs) with the given activated opacities"""
    cov, colors = _np(a["cov3D_precomp"]), _np(a["colors"])
    return oracle.forward(bg, cl.xyz, np.ascontiguousarray(opacity, np.float32), cam.viewmatrix, cam.projmatrix, cam.campos, cam.tanfovx,
                          cam.tanfovy, cam.H, cam.W, shs=None if colors is not None else _np(a["sh"]), sh_degree=3,
                          colors_precomp=colors, scales=None if cov is not None else cl.get_scaling(),
                          rotations=None if cov is not None else cl.get_rotation(), cov3D_precomp=cov)


def lists(lib_path, dev, a, flags, P, W, H):
    """(R, image, radii, point list, tile ranges) of a training forward through the test-suite's view into the buffers"""
    import ctypes as C
    devapi = parity.devapi
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        lib, dlib = capi.load(lib_path), devapi.load(lib_path)
        R, color, radii, geom, binning, img = rp.RasterizeGaussiansCUDA(**a, raw_params=flags)
        bv, iv = devapi.BinningView(), devapi.ImageView()
        capi.check(lib, dlib.gsr_view_image(C.c_void_p(img.data_ptr()), W, H, C.byref(iv)), "view_image")
        T = ((W + 15) // 16) * ((H + 15) // 16)
        ranges = parity._slice(img, iv.ranges, 2 * T, np.uint32)
        pl = np.zeros(0, np.uint32)
        if R:
            capi.check(lib, dlib.gsr_view_binning(C.c_void_p(binning.data_ptr()), R, W, H, C.byref(bv)), "view_binning")
            pl = parity._slice(binning, bv.point_list, R, np.uint32)
        return R, color, radii, pl, ranges
    finally:
        rp._LIB_OVERRIDE = prev


def check_forward(lib_path, dev, oracle, cl, cam, bg, flags, raw=False, **kw):
    """The render with the bit against the oracle's render with o h32 (parity.RGB_L1_TOL; radii and instance count equal); against
    the library's own render without the bit: radii, R, point list and ranges equal, the image differs.  raw: the model's raw
    parameters with GSR_RAW_* (activated in-kernel)."""
    a = fo.inputs(cl, cam, bg, dev, **kw)
    cov = _np(a["cov3D_precomp"])
    if raw:
        a.update(opacity=fo._t(cl.opacity, dev), scales=fo._t(cl.scaling, dev), rotations=fo._t(cl.rotation, dev))
        flags |= 7
    h = h32(cl, cam, cov)
    ores, ocolor, oradii = oracle_forward(oracle, a, cl, cam, bg, cl.get_opacity().reshape(-1) * h)
    R0, c0, r0, _, _ = fo.render(lib_path, a, flags)
    R1, c1, r1, _, _ = fo.render(lib_path, a, flags | AA)
    rep = dict(rgb_L1=float(np.abs(c1.cpu().numpy() - ocolor).mean()), R=R1,
               changed=float((c1 - c0).abs().mean()), h_mean=float(h[oradii > 0].mean()) if (oradii > 0).any() else 1.0)
    print("measured:", rep)
    assert np.array_equal(r1.cpu().numpy(), oradii) and R1 == ores.R
    assert rep["rgb_L1"] <= parity.RGB_L1_TOL, rep
    assert R0 == R1 and torch.equal(r0, r1), "the bit changed the radii or the instance count"
    assert not torch.equal(c0, c1), "the bit did not change the image"
    if not flags & fo.FORWARD_ONLY:
        P = cl.xyz.shape[0]
        _, _, _, pl0, rg0 = lists(lib_path, dev, a, flags, P, cam.W, cam.H)
        _, c2, _, pl1, rg1 = lists(lib_path, dev, a, flags | AA, P, cam.W, cam.H)
        if not flags & 8:   # (GSR_CULL_EMPTY_TILES drops instances by a bound on the COMPENSATED opacity: its internal lists may be shorter)
            assert np.array_equal(pl0, pl1) and np.array_equal(rg0, rg1), "the bit changed the lists"
        assert torch.equal(c2, c1)
        # the forward-only form renders the same image, bit for bit
        _, cf, rf, _, _ = fo.render(lib_path, a, flags | AA | fo.FORWARD_ONLY)
        assert torch.equal(cf, c1) and torch.equal(rf, r1)
    return rep


# ---------------------------------------------------------------------------------------------------- backward
def expected_grads(oracle, a, cl, cam, bg, dpix, dD=None, dA=None):
    """the gradients the library must return with the bit (module docstring), float64; and the oracle's radii, h32 and g' o"""
    cov = _np(a["cov3D_precomp"])
    h = h32(cl, cam, cov)
    o = cl.get_opacity().reshape(-1)

    # depth_alpha_cases.oracle_grads runs the colour pass through parity.run_oracle, which takes the activated opacity from the
    # cloud, and the map passes through the inputs `a`: both get o' = o h32, which the oracle then holds independent
    import copy
    op = np.ascontiguousarray((o * h).reshape(-1, 1), np.float32)
    a2 = dict(a, opacity=fo._t(op, torch.device("cpu")))
    cl2 = copy.copy(cl)
    cl2.get_opacity = lambda: op
    g, oradii = da.oracle_grads(oracle, a2, cl2, cam, bg, dpix, dD, dA)
    vis = oradii > 0
    gp = g["dL_dopacity"].reshape(-1)
    w = np.where(vis, gp * o.astype(np.float64), 0.0)
    jt = h_jacobian_term(cl, cam, w, cov)
    exp = dict(g)
    exp["dL_dopacity"] = (gp * h.astype(np.float64)).reshape(g["dL_dopacity"].shape)
    for k in ("dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dcov3D"):
        if k in jt and k in exp and exp[k] is not None and np.size(exp[k]):
            exp[k] = exp[k] + jt[k].reshape(exp[k].shape)
    if cov is None:
        # dL_dcov3D with scales / rotations: the library writes the gradient of the covariance it computed; the h term through cov3D
        exp.pop("dL_dcov3D", None)
    return exp, oradii, h, w, jt


def compare_grads(out, ref, vis, what=""):
    rep = {}
    for name, gt in zip(GRAD_NAMES, out):
        if gt is None or gt.numel() == 0 or name not in ref or ref[name] is None or not np.abs(ref[name]).sum():
            continue
        g = gt.cpu().numpy()
        assert np.isfinite(g).all(), name
        rep[name] = parity.rel_l1(g, ref[name].reshape(g.shape))
        assert rep[name] <= parity.GRAD_REL_L1_TOL, (what, name, rep)
        assert not np.any(g.reshape(g.shape[0], -1)[~vis]), f"{name} non-zero on culled Gaussians"
        if name in ROW_CHECKED:
            e = parity.row_errors(g, ref[name].reshape(g.shape))[vis]
            row = dict(p9999=float(np.quantile(e, 0.9999)), max=float(e.max()), beyond=int((e > parity.ROW_OUTLIER).sum()))
            rep["rows_" + name] = row
            assert row["p9999"] <= parity.ROW_P9999_TOL and row["max"] <= parity.ROW_MAX_TOL, (what, name, row)
            assert row["beyond"] <= max(3, parity.ROW_OUTLIER_FRAC * e.size), (what, name, row)
    return rep


def check_backward(lib_path, dev, oracle, cl, cam, bg, flags, seed=0, maps=False, h_term_min=0.0, **kw):
    """backward with the bit (random dpix; maps: random dL_ddepth / dL_dalpha too) against expected_grads.  h_term_min: the share
    of the expected dL_dmeans3D that is the h term must be at least this (a scene of small splats: there its absence could not
    pass the bars)"""
    rng = np.random.default_rng(seed)
    a = fo.inputs(cl, cam, bg, dev, **kw)
    dpix = rng.standard_normal((3, cam.H, cam.W)).astype(np.float32)
    dD = rng.standard_normal((cam.H, cam.W)).astype(np.float32) if maps else None
    dA = rng.standard_normal((cam.H, cam.W)).astype(np.float32) if maps else None
    t = lambda x: None if x is None else fo._t(x, dev)
    out, radii = da.backward(lib_path, a, cam, flags, t(dpix), t(dD), t(dA), raw=AA)
    ref, oradii, h, w, jt = expected_grads(oracle, a, cl, cam, bg, dpix, dD, dA)
    assert np.array_equal(radii.cpu().numpy(), oradii)
    vis = oradii > 0
    rep = compare_grads(out, ref, vis)
    # how much of the geometry gradient is the h term (a test that could not tell its absence shows nothing)
    rep["h_term_share_means3D"] = float(np.abs(jt["dL_dmeans3D"]).sum() / (np.abs(ref["dL_dmeans3D"]).sum() + 1e-30))
    print("measured:", rep)
    assert rep["h_term_share_means3D"] >= h_term_min, rep
    return rep


def check_mismatch_guard(lib_path, dev, cl, cam, bg):
    """gsr_backward refuses the buffers of a forward pass whose GSR_ANTIALIAS bit differs from its own"""
    a = fo.inputs(cl, cam, bg, dev)
    dpix = torch.ones((3, cam.H, cam.W), device=dev)
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        for fwd, bwd in ((AA, 0), (0, AA)):
            R, _, radii, g, b, i = rp.RasterizeGaussiansCUDA(**a, raw_params=fwd)
            try:
                rp.RasterizeGaussiansBackwardCUDA(a["background"], a["means3D"], radii, a["colors"], a["scales"], a["rotations"], 1.0,
                                                  a["cov3D_precomp"], a["viewmatrix"], a["projmatrix"], cam.tanfovx, cam.tanfovy, dpix,
                                                  a["sh"], 3, a["campos"], g, R, b, i, raw_params=bwd)
            except capi.GsrError as e:
                assert e.status == -1
            else:
                raise AssertionError("gsr_backward accepted a GSR_ANTIALIAS bit that differs from the forward pass's")
        # the keyword and the bit say the same
        R, c1, radii, g, b, i = rp.RasterizeGaussiansCUDA(**a, antialiasing=True)
        out = rp.RasterizeGaussiansBackwardCUDA(a["background"], a["means3D"], radii, a["colors"], a["scales"], a["rotations"], 1.0,
                                                a["cov3D_precomp"], a["viewmatrix"], a["projmatrix"], cam.tanfovx, cam.tanfovy, dpix,
                                                a["sh"], 3, a["campos"], g, R, b, i, antialiasing=True)
        _, c2, _, _, _, _ = rp.RasterizeGaussiansCUDA(**a, raw_params=AA)
        assert torch.equal(c1, c2) and torch.isfinite(out[3]).all()
    finally:
        rp._LIB_OVERRIDE = prev


def check_fused_geom_adam(lib_path, dev, cl, cam, bg, seed=0):
    """raw_params = 7 | GSR_ANTIALIAS + geom_adam with depth / alpha gradients: the parameters after the fused step match the unfused
    gradients (with the bit) + gsr_adam_step, to the bar of depth_alpha_cases.check_fused_geom_adam; and the unfused raw-parameter
    gradients follow the activated ones through the activations' chain rule"""
    lib = capi.load(lib_path)
    rng = np.random.default_rng(seed)
    P = cl.xyz.shape[0]
    raw = capi.RAW_OPACITY | capi.RAW_SCALING | capi.RAW_ROTATION | AA
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
        out, radii = da.backward(lib_path, a, cam, 0, dpix, dD, dA, raw=raw, geom_adam=ga, training_outputs_only=fused)
        return st, out, radii.cpu().numpy()

    st_ref, g_ref, radii = run(False)
    grads = dict(xyz=g_ref[3], opacity=g_ref[2], scaling=g_ref[6], rotation=g_ref[7])
    # the raw opacity gradient: the activated one (same bit, activated inputs) times o (1 - o)
    a_act = fo.inputs(cl, cam, bg, dev)
    g_act, _ = da.backward(lib_path, a_act, cam, 0, dpix, dD, dA, raw=AA)
    o = cl.get_opacity().reshape(-1).astype(np.float64)
    want = g_act[2].cpu().numpy().reshape(-1).astype(np.float64) * o * (1 - o)
    err = parity.rel_l1(grads["opacity"].cpu().numpy().reshape(-1), want)
    print("measured: raw opacity gradient against activated * o (1 - o):", err)
    assert err <= parity.GRAD_REL_L1_TOL, err
    for n in names:
        p_, m_, v_ = st_ref[n]
        gr = grads[n].contiguous()
        capi.check(lib, lib.gsr_adam_step(p_.data_ptr(), gr.data_ptr(), m_.data_ptr(), v_.data_ptr(), p_.numel(), lrs[n], 0.9, 0.999,
                                          1e-15, steps[n], 0, 0, lrs[n], None), "gsr_adam_step")
    if dev.type != "cpu":
        torch.cuda.synchronize()
    st_fus, _, _ = run(True)
    exact = dev.type == "cpu"
    assert (radii > 0).any()
    for n in names:
        for k in range(3):
            x, y = st_fus[n][k].cpu().numpy(), st_ref[n][k].cpu().numpy()
            tol = max(lrs[n] * (2e-6 if exact else 2e-3), 1.2e-7 * np.abs(y).max()) if k == 0 else (1e-6 if exact else 2e-4) * np.abs(y).max()
            assert np.abs(x - y).max() <= tol, (n, k, np.abs(x - y).max(), tol)


def check_pose(lib_path, dev, oracle, cl, cam, bg, flags=(32, 64), seed=0, cov=False):
    """The pose gradients with the bit by the rigid-motion identity of pose_grad_cases.py (its method (b), view-independent colour,
    random upstream gradient): the identity's per-Gaussian gradients are expected_grads (the oracle's with o h plus the h term), the
    bar parity.GRAD_REL_L1_TOL on the mass-normalised error, as there"""
    kw = dict(use_colors_precomp=True, use_cov3D_precomp=cov)
    a = fo.inputs(cl, cam, bg, dev, **kw)
    dpix = np.random.default_rng(seed).standard_normal((3, cam.H, cam.W)).astype(np.float32)
    ref, oradii, h, w, jt = expected_grads(oracle, a, cl, cam, bg, dpix)
    vis = oradii > 0
    if cov:
        terms = pg.identity_terms(cam, cl.xyz[vis], ref["dL_dmeans3D"][vis], g_cov=ref["dL_dcov3D"][vis], cov=_np(a["cov3D_precomp"])[vis])
        plain = pg.identity_terms(cam, cl.xyz[vis], (ref["dL_dmeans3D"] - jt["dL_dmeans3D"])[vis],
                                  g_cov=(ref["dL_dcov3D"] - jt["dL_dcov3D"])[vis], cov=_np(a["cov3D_precomp"])[vis])
    else:
        terms = pg.identity_terms(cam, cl.xyz[vis], ref["dL_dmeans3D"][vis], h_rot=ref["dL_drotations"][vis], rot=cl.get_rotation()[vis])
        plain = pg.identity_terms(cam, cl.xyz[vis], (ref["dL_dmeans3D"] - jt["dL_dmeans3D"])[vis],
                                  h_rot=(ref["dL_drotations"] - jt["dL_drotations"])[vis], rot=cl.get_rotation()[vis])
    total, mass = terms.sum(0), np.abs(terms).sum(0)
    reps = []
    for f in flags:
        out, radii = pg.backward_pose(lib_path, a, cam, f, fo._t(dpix, dev), raw=AA)
        assert np.array_equal(radii.cpu().numpy(), oradii)
        gv, gp, gc = (t.cpu().numpy() for t in out[8:])
        assert not gc.any() and not gv.reshape(-1)[pg.VIEW_DEAD].any() and not gp.reshape(-1)[pg.PROJ_DEAD].any()
        got = pg.chain_to_xi(gv, gp, gc, cam)
        err = np.abs(got - total) / mass
        miss = np.abs(got - plain.sum(0)) / mass   # against the identity WITHOUT the h term: must be told apart
        rep = dict(flags=f, err=[float(e) for e in err], without_h_term=[float(e) for e in miss], visible=int(vis.sum()))
        print("measured:", rep)
        assert (err <= parity.GRAD_REL_L1_TOL).all(), rep
        reps.append(rep)
    return reps


# ---------------------------------------------------------------------------------------------------- clamp
def clamp_scene(W=64, H=48):
    """one crafted Gaussian with det Sigma / det Sigma' < 0.000025 in front of the camera (a needle far thinner than a pixel, seen
    side-on, so that it still covers pixels), among a few ordinary ones"""
    from photo_slam_amd import scene
    cl = scene.make_cloud(40, W, H, 0.8 * W, 0.8 * W, seed=21, scale_k=0.6)
    cam = cl.cameras[0]
    Wc = cam.viewmatrix.astype(np.float64).T   # W2C
    c2w = np.linalg.inv(Wc)
    centre = (c2w @ np.array([0.05, -0.03, 2.0, 1.0]))[:3]
    cl.xyz[0] = centre.astype(np.float32)
    # the long axis along the camera's x: rotation = the camera's rotation (world <- camera axes)
    Rcw = c2w[:3, :3]
    cl.rotation[0] = _quat(Rcw).astype(np.float32)
    cl.scaling[0] = np.log(np.array([0.4, 1e-7, 1e-7], np.float32))
    cl.opacity[0] = 8.0    # (0.005 o must stay above the blend's 1 / 255)
    return cl, cam


def _quat(R):
    """(r, x, y, z) of a rotation matrix"""
    r = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    if r > 1e-6:
        return np.array([r, (R[2, 1] - R[1, 2]) / (4 * r), (R[0, 2] - R[2, 0]) / (4 * r), (R[1, 0] - R[0, 1]) / (4 * r)])
    x = np.sqrt(max(0.0, 1 + R[0, 0] - R[1, 1] - R[2, 2])) / 2
    return np.array([(R[2, 1] - R[1, 2]) / (4 * x), x, (R[0, 1] + R[1, 0]) / (4 * x), (R[0, 2] + R[2, 0]) / (4 * x)])


def check_clamp(lib_path, dev, oracle, bg, seed=0):
    """the crafted Gaussian's compensated opacity is 0.005 o, and its h term is exactly absent: its gradients equal the oracle's
    with o' (opacity: g' * 0.005)"""
    cl, cam = clamp_scene()
    a = fo.inputs(cl, cam, bg, dev)
    h = h32(cl, cam)
    assert h[0] == np.float32(np.sqrt(np.float32(H2_MIN))), h[0]
    a0, b0, c0 = (float(v[0]) for v in cov2d32(cl, cam))
    assert (a0 * c0 - b0 * b0) / ((a0 + 0.3) * (c0 + 0.3) - b0 * b0) < H2_MIN
    dpix = np.random.default_rng(seed).standard_normal((3, cam.H, cam.W)).astype(np.float32)
    out, radii = da.backward(lib_path, a, cam, 64, fo._t(dpix, dev), None, None, raw=AA)
    ref, oradii, h, w, jt = expected_grads(oracle, a, cl, cam, bg, dpix)
    assert oradii[0] > 0 and np.array_equal(radii.cpu().numpy(), oradii)
    assert not jt["dL_dmeans3D"][0].any() and not jt["dL_dscales"][0].any() and not jt["dL_drotations"][0].any()
    compare_grads(out, ref, oradii > 0, "clamp scene")
    # the crafted row on its own, against the oracle with o' (no h term): the bar of a row
    for name, k in (("dL_dmeans3D", 3), ("dL_dscales", 6), ("dL_drotations", 7), ("dL_dopacity", 2)):
        g = out[k].cpu().numpy().reshape(cl.xyz.shape[0], -1)[0].astype(np.float64)
        r = ref[name].reshape(cl.xyz.shape[0], -1)[0]
        assert np.abs(r).sum() > 0, name
        e = np.abs(g - r).sum() / np.abs(r).sum()
        print("measured: clamped row", name, e)
        assert e <= parity.ROW_P9999_TOL, (name, e)
    # the record holds 0.005 o: the forward image equals the oracle's with that opacity (checked by check_forward's bar)
    ores, ocolor, _ = oracle_forward(oracle, a, cl, cam, bg, cl.get_opacity().reshape(-1) * h)
    _, c1, _, _, _ = fo.render(lib_path, a, 64 | AA)
    assert float(np.abs(c1.cpu().numpy() - ocolor).mean()) <= parity.RGB_L1_TOL


# ---------------------------------------------------------------------------------------------------- energy
ENERGY_SIGMAS = (0.25, 0.5, 1.0, 2.0)
ENERGY_TOL = 0.03   # derived: the 3-sigma cut loses <= exp(-4.5) = 1.1 %, unit sampling of a sigma' >= 0.55 px Gaussian errs <= 0.6 %


def energy_scene(sigma_px, W=64, H=64):
    """one isolated isotropic Gaussian in front of a camera at the origin, of projected sigma `sigma_px` pixels, opacity chosen so
    that o h = 0.5; returns (cloud, camera, o, det Sigma)"""
    from photo_slam_amd import scene
    fxy = 0.8 * W
    cam = scene.make_camera(W, H, fxy, fxy, np.eye(3), np.zeros(3))
    z = 4.0
    s = sigma_px * z / fxy     # on the optical axis J = diag(f / z): the projected sigma is f s / z
    det0 = sigma_px ** 4
    h = np.sqrt(det0 / (sigma_px ** 2 + LOWPASS) ** 2)
    o = 0.5 / h            # (an ACTIVATED opacity, passed as such: it exceeds 1 below sigma = 0.6 px, where 1 / h > 2)
    # a little off the pixel centre, well inside the image
    x = np.array([[0.013 * z, -0.021 * z, z]], np.float32)
    cl = scene.Cloud(x, np.zeros((1, 1, 3), np.float32), np.zeros((1, 15, 3), np.float32), np.log(np.full((1, 3), s, np.float32)),
                     np.array([[1.0, 0, 0, 0]], np.float32), np.zeros((1, 1), np.float32), [cam], 1.0)
    return cl, cam, float(o), float(det0)


def check_energy(lib_path, dev, oracle):
    """Sum over the pixels of the alpha map of one isolated isotropic Gaussian whose activated opacity o is chosen so that o h = 0.5:
    with the bit it is 2 pi o sqrt(det Sigma) within ENERGY_TOL (the oracle with o h32 first).  Without the bit the sum exceeds
    2 pi o sqrt(det Sigma) by 1 / h -- checked at o = 0.5 instead: with o h = 0.5 the uncompensated o is 2.9 at sigma = 0.25 and 1.1
    at 0.5, where the blend's alpha <= 0.99 saturates the peak and the sum is no longer linear in o."""
    rep = {}
    for sigma in ENERGY_SIGMAS:
        cl, cam, o, _ = energy_scene(sigma)
        bg = np.zeros(3, np.float32)
        a = fo.inputs(cl, cam, bg, dev, use_colors_precomp=True)
        a["colors"] = torch.ones((1, 3), device=dev)
        h = h32(cl, cam)
        a0, b0, c0 = (float(v[0]) for v in cov2d32(cl, cam))   # (det Sigma of the restatement: sigma^4 up to the off-axis term)
        root = np.sqrt(a0 * c0 - b0 * b0)
        assert abs(root / sigma ** 2 - 1) < 1e-3
        want = 2 * np.pi * o * root
        a["opacity"] = torch.full((1, 1), o, device=dev)
        _, ocolor, _ = oracle_forward(oracle, a, cl, cam, bg, np.array([o], np.float32) * h)
        e_or = float(ocolor[0].astype(np.float64).sum())
        assert abs(e_or / want - 1) <= ENERGY_TOL, ("the oracle with o h32", sigma, e_or, want)
        _, _, _, _, al1, _ = da.render(lib_path, a, 64 | AA, depth=False)
        e1 = float(al1.double().sum())
        a["opacity"] = torch.full((1, 1), 0.5, device=dev)
        _, _, _, _, al0, _ = da.render(lib_path, a, 64, depth=False)
        e0 = float(al0.double().sum()) / (2 * np.pi * 0.5 * root)
        rep[sigma] = dict(with_bit=e1 / want, without=e0, one_over_h=float(1 / h[0]))
        print("measured: energy", sigma, rep[sigma])
        assert abs(e1 / want - 1) <= ENERGY_TOL, (sigma, rep[sigma])
        assert abs(e0 * float(h[0]) - 1) <= ENERGY_TOL, (sigma, rep[sigma])
    assert rep[0.25]["one_over_h"] > 5.5   # 5.9x at sigma = 0.25
    return rep


# ---------------------------------------------------------------------------------------------------- level consistency
def level_consistency(lib_path, dev, P=4000, W=256, H=192, scale_k=0.02, seed=8):
    """mean alpha map of one cloud at W x H and at W/4 x H/4 with the same camera, with and without the bit: (|difference| with,
    |difference| without, visible share of Gaussians that are sub-pixel at the coarse level)"""
    from photo_slam_amd import scene
    fine = scene.make_cloud(P, W, H, 0.8 * W, 0.8 * W, seed=seed, scale_k=scale_k)
    coarse = scene.make_cloud(P, W // 4, H // 4, 0.8 * W / 4, 0.8 * W / 4, seed=seed, scale_k=scale_k)
    assert np.array_equal(fine.xyz, coarse.xyz) and np.array_equal(fine.cameras[0].viewmatrix, coarse.cameras[0].viewmatrix)
    bg = np.zeros(3, np.float32)
    means = {}
    for name, cl in (("fine", fine), ("coarse", coarse)):
        cam = cl.cameras[0]
        a = fo.inputs(cl, cam, bg, dev)
        for bit in (0, AA):
            _, _, _, _, al, _ = da.render(lib_path, a, bit, depth=False)
            means[name, bit] = float(al.double().mean())
    a0, b0, c0 = cov2d32(coarse, coarse.cameras[0])
    vis = da.view_z(coarse, coarse.cameras[0]) > 0.2
    sub = float((np.sqrt(np.maximum(a0, c0))[vis] < 1.0).mean())
    d_with = abs(means["fine", AA] - means["coarse", AA])
    d_without = abs(means["fine", 0] - means["coarse", 0])
    return d_with, d_without, sub, means


# ---------------------------------------------------------------------------------------------------- default untouched
def default_hashes(lib_path, dev, cl, cam, bg, parent_convention, seed=0):
    """sha256 of image, radii and every gradient of a run with the bit clear.  parent_convention: the calls exactly as before this
    feature existed (no antialiasing argument, no bit); otherwise antialiasing=False passed through the new keyword"""
    rng = np.random.default_rng(seed)
    a = fo.inputs(cl, cam, bg, dev)
    dpix = fo._t(rng.standard_normal((3, cam.H, cam.W)).astype(np.float32), dev)
    kw = {} if parent_convention else dict(antialiasing=False)
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
def check_autograd(lib_path, dev, cl):
    """The autograd node (GaussianRasterizer with antialiasing_) against the C-ABI gradients of the direct call with the bit: a loss
    on colour + depth + alpha back-propagates to the same gradients (bit for bit on the emulator); under torch.no_grad() the
    forward-only path renders the same image"""
    from photo_slam_amd.gaussian_rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    cam = cl.cameras[0]
    bg = np.array([0.2, 0.5, 0.1], np.float32)
    rng = np.random.default_rng(5)
    t = lambda x: fo._t(x, dev)
    wc = t(rng.standard_normal((3, cam.H, cam.W)).astype(np.float32))
    wd = t(rng.standard_normal((cam.H, cam.W)).astype(np.float32))
    wa = t(rng.standard_normal((cam.H, cam.W)).astype(np.float32))
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        def settings(aa):
            return GaussianRasterizationSettings(cam.H, cam.W, cam.tanfovx, cam.tanfovy, t(bg), 1.0, t(cam.viewmatrix), t(cam.projmatrix),
                                                 3, t(cam.campos), False, render_depth_=True, antialiasing_=aa)
        leaf = lambda x: t(x).clone().requires_grad_(True)
        L = dict(means3D=leaf(cl.xyz), means2D=torch.zeros((cl.xyz.shape[0], 3), device=dev, requires_grad=True),
                 opacities=leaf(cl.get_opacity()), shs=leaf(cl.get_features()), scales=leaf(cl.get_scaling()),
                 rotations=leaf(cl.get_rotation()))
        color, radii, depth, alpha = GaussianRasterizer(settings(True))(L["means3D"], L["means2D"], L["opacities"], True, False, True,
                                                                          True, False, shs=L["shs"], scales=L["scales"],
                                                                          rotations=L["rotations"])
        ((color * wc).sum() + (depth * wd).sum() + (alpha * wa).sum()).backward()
        a = fo.inputs(cl, cam, bg, dev)
        ref, _ = da.backward(lib_path, a, cam, 0, wc, wd, wa, raw=AA)
        got = dict(dL_dmeans3D=L["means3D"].grad, dL_dmeans2D=L["means2D"].grad, dL_dopacity=L["opacities"].grad,
                   dL_dscales=L["scales"].grad, dL_drotations=L["rotations"].grad, dL_dsh=L["shs"].grad)
        for name, g in zip(GRAD_NAMES, ref):
            if name not in got:
                continue
            x = got[name]
            assert x is not None and torch.isfinite(x).all(), name
            if dev.type == "cpu":
                assert torch.equal(x.reshape(g.shape), g), name
            else:
                assert parity.rel_l1(x.reshape(g.shape).cpu().numpy(), g.cpu().numpy()) <= 1e-5, name
        with torch.no_grad():
            c2, r2, d2, a2 = GaussianRasterizer(settings(True))(L["means3D"], L["means2D"], L["opacities"], True, False, True, True, False,
                                                                 shs=L["shs"], scales=L["scales"], rotations=L["rotations"])
            c3 = GaussianRasterizer(settings(False))(L["means3D"], L["means2D"], L["opacities"], True, False, True, True, False,
                                                     shs=L["shs"], scales=L["scales"], rotations=L["rotations"])[0]
        assert rp.lastForwardOnly() == 1
        assert torch.equal(c2, color.detach()) and torch.equal(d2, depth.detach()) and torch.equal(a2, alpha.detach())
        assert not torch.equal(c3, c2)
    finally:
        rp._LIB_OVERRIDE = prev


def mixed_resolution_data(cl, dev, seed=0):
    """two keyframes of one camera pose at two pyramid levels (full and half resolution), their targets and masks"""
    from photo_slam_amd import scene
    from photo_slam_amd.gaussian_renderer import GaussianKeyframe
    cam = cl.cameras[0]
    half = scene.Camera(cam.W // 2, cam.H // 2, cam.tanfovx, cam.tanfovy, cam.viewmatrix, cam.projmatrix, cam.campos)
    torch.manual_seed(seed)
    cams = [cam, half]
    kfs = [GaussianKeyframe.from_camera(c, dev) for c in cams]
    gts = [torch.rand(3, c.H, c.W).to(dev) for c in cams]
    masks = [torch.ones(3, c.H, c.W, device=dev) for c in cams]
    return cams, kfs, gts, masks


def _python_trainer(cl, dev, antialiasing):
    import copy
    from photo_slam_amd.gaussian_model import GaussianModel, GaussianOptimizationParams
    from photo_slam_amd.gaussian_renderer import GaussianPipelineParams
    from photo_slam_amd.trainer import TrainStep
    g = GaussianModel.from_cloud(copy.deepcopy(cl), device=dev)
    opt = GaussianOptimizationParams()
    g.trainingSetup(opt)
    ts = TrainStep(g, opt, GaussianPipelineParams(), torch.zeros(3, device=dev), cameras_extent=float(cl.extent), seed=7,
                   antialiasing=antialiasing)
    return g, ts


def check_hosts(ops, lib_path, dev, cl, steps=6, exact=True):
    """Python TrainStep(antialiasing=True) and the C++ TrainStep (option antialiasing) over `steps` steps on a mixed-resolution pair
    of keyframes: the same loss sequence and parameters, to the tolerance tests/test_cpp_host.py holds the hosts to; the bit is
    really on in both (the first loss differs from the run without it); render_view / renderView agree too"""
    import copy
    from photo_slam_amd.gaussian_model import GaussianModel
    cams, kfs, gts, masks = mixed_resolution_data(cl, dev)
    args = [da._cam_args(c, dev) for c in cams]
    n = len(cams)

    def cpp(aa):
        g0 = GaussianModel.from_cloud(copy.deepcopy(cl), device=dev)
        h = ops.trainer_create(g0.xyz_.detach(), g0.features_.detach(), g0.opacity_.detach(), g0.scaling_.detach(), g0.rotation_.detach(),
                               3, float(cl.extent), torch.zeros(3, device=dev))
        ops.trainer_set_options(h, {"seed": 7.0, "cameras_extent": float(cl.extent), "antialiasing": 1.0 if aa else 0.0})
        try:
            losses = []
            for it in range(steps):
                losses.append(ops.trainer_render_and_backward(h, *args[it % n], gts[it % n], masks[it % n]).item())
                ops.trainer_finish(h)
            view = ops.trainer_render_view(h, *args[1])
            return losses, [p.detach().clone() for p in ops.trainer_params(h)], view
        finally:
            ops.trainer_destroy(h)

    losses_cpp, params_cpp, view_cpp = cpp(True)
    losses_off, _, _ = cpp(False)
    assert losses_cpp[0] != losses_off[0], "the C++ host's option did not reach the rasterizer"
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        g, ts = _python_trainer(cl, dev, True)
        losses_py = [ts.trainForOneIteration(kfs[it % n], gts[it % n], masks[it % n], sync_loss=False).item() for it in range(steps)]
        view_py = ts.render_view(kfs[1])
        g.sync_features()
        g_off, ts_off = _python_trainer(cl, dev, False)
        first_off = ts_off.trainForOneIteration(kfs[0], gts[0], masks[0], sync_loss=False).item()
    finally:
        rp._LIB_OVERRIDE = prev
    assert losses_py[0] != first_off, "TrainStep(antialiasing=True) did not reach the rasterizer"
    print("measured: losses", losses_cpp, losses_py)
    assert np.allclose(losses_cpp, losses_py, rtol=1e-5), (losses_cpp, losses_py)
    for x, y in zip(params_cpp, g.params()):
        if exact:
            assert torch.allclose(x, y.detach(), rtol=1e-4, atol=1e-6)
        else:
            assert parity.rel_l1(x.cpu().numpy(), y.detach().cpu().numpy()) <= 1e-3
    assert float((view_cpp - view_py).abs().max()) <= (1e-5 if exact else 1e-3)
