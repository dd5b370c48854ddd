"""Shared checks of the camera pose gradients (gsr_backward_args.dL_dviewmatrix / dL_dprojmatrix / dL_dcampos, include/gsr.h) and of
pose refinement (TrainStep.refinePose) for the emulator tests (test_pose_grad.py), the GPU tests (test_gpu_pose_grad.py) and the
C++ host's (test_cpp_host_pose.py).

Two references, neither shares code with the kernels:
  (a) float64 autograd of test_oracle_pinning.torch_render with respect to its view_t, proj_t and campos arguments -- the
      DEFINITION of the three gradients -- at every SH degree, on the small scenes of that file whose pixels are not
      threshold-fragile;
  (b) the rigid-motion identity through the CPU oracle's own gradients, for view-independent colour at any size: moving the
      camera by exp(xi^) on the left is moving every Gaussian rigidly the other way, so with W2C = [R | tau], t_i = R x_i + tau,
      g_i = dL_dmeans3D_i, q_i = (r, v), h_i = dL_drotations_i over the rows with radii > 0
          dL/drho   = sum_i R g_i
          dL/dtheta = sum_i [ t_i x (R g_i) + R w_i ],   w_i[k] = 1/2 h_i . (-v_k, r e_k + e_k x v)
      (cov3D_precomp: w_i = 2 (M_12, M_20, M_01), M = C_i G_i - G_i C_i, G_i the symmetric matrix of dL_dcov3D_i).
Bars: (a) AUTOGRAD_TOL = 2e-3, the bar test_oracle_pinning.py applies to fp32-vs-float64 gradients (measured on the emulator:
<= 2.6e-6 for the matrices, <= 6e-7 for the camera centre); (b) with a random upstream gradient the error is normalised by the
mass sum_i |term_i| of each component (a sum of a million mixed-sign terms cancels), bar parity.GRAD_REL_L1_TOL = 1e-4; with a
coherent one (the gradient of the L1 distance to the oracle's render at a perturbed pose) by |sum|, bar COHERENT_TOL = 2e-3, after
asserting on the oracle alone that |sum| >= 1e-2 mass in every component."""
import math

import numpy as np
import torch

import forward_only_cases as fo
import parity
from photo_slam_amd import capi, scene
from photo_slam_amd import rasterize_points as rp
from test_oracle_pinning import torch_render

DEPTH_FIRST, TILE_FIRST = 32, 64      # GSR_BINNING_DEPTH_FIRST / GSR_BINNING_TILE_FIRST
AUTOGRAD_CASES = [(1, 1), (2, 3), (3, 2), (4, 3), (5, 0)]   # (seed, degree) of test_oracle_matches_independent_float64_autograd without fragile pixels
AUTOGRAD_TOL = 2e-3
COHERENT_TOL = 2e-3
COHERENT_MIN_SIGNAL = 1e-2
# the perturbation of the coherent upstream gradient: 0.5 degrees about COHERENT_AXIS, 1 % of the mean depth along
# COHERENT_DIRECTION (mostly backwards: a sideways step leaves the z component of the oracle's sum below the signal bar on the
# small scenes).  Chosen on the ORACLE ALONE: its |sum| / mass is >= 0.033 in every component at C1, C2, C3, a C5 view and the
# emulator scenes (C3: 0.22 0.19 0.35 0.09 0.12 0.09).
COHERENT_AXIS = (0.5, -0.7, 0.5)
COHERENT_DIRECTION = (-0.3, 0.25, -0.92)
VIEW_DEAD = [3, 7, 11, 15]            # row 3 of W2C
PROJ_DEAD = [2, 6, 10, 14]            # the z row of the projection
GRAD_NAMES = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations")


# ---------------------------------------------------------------------------------------------------- poses in float64
def exp64(xi):
    """exp(xi^), xi = (rho, theta), as a float64 [4,4] torch matrix (differentiable at 0)"""
    z = xi.new_zeros(())
    tw = torch.stack([torch.stack([z, -xi[5], xi[4], xi[0]]), torch.stack([xi[5], z, -xi[3], xi[1]]),
                      torch.stack([-xi[4], xi[3], z, xi[2]]), xi.new_zeros(4)])
    return torch.linalg.matrix_exp(tw)


def base_of(cam):
    """(W2C_0, P^T) in float64 from a scene.Camera: projmatrix = view . P^T"""
    view = torch.tensor(cam.viewmatrix.astype(np.float64))
    return view.T.contiguous(), torch.linalg.solve(view, torch.tensor(cam.projmatrix.astype(np.float64)))


def camera_tensors64(xi, w2c0, projT):
    """the three camera tensors of the pose exp(xi^) W2C_0, built as the hosts' PoseDelta builds them"""
    view = (exp64(xi) @ w2c0).T
    return view, view @ projT, torch.linalg.inv(view)[3, :3]


def chain_to_xi(Gv, Gp, Gc, cam):
    """the 6-vector dL/dxi at xi = 0 from the three raw gradients, through the pose's construction (float64 autograd)"""
    w2c0, projT = base_of(cam)
    xi = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    v, p, c = camera_tensors64(xi, w2c0, projT)
    t64 = lambda g: torch.tensor(np.asarray(g, np.float64))
    ((v * t64(Gv).reshape(4, 4)).sum() + (p * t64(Gp).reshape(4, 4)).sum() + (c * t64(Gc)).sum()).backward()
    return xi.grad.numpy()


def moved_camera(cam, xi):
    """scene.Camera at exp(xi^) W2C (float64 construction, rounded once)"""
    w2c0, projT = base_of(cam)
    with torch.no_grad():
        v, p, c = camera_tensors64(torch.tensor(np.asarray(xi, np.float64)), w2c0, projT)
    f = lambda t: np.ascontiguousarray(t.numpy().astype(np.float32))
    return scene.Camera(cam.W, cam.H, cam.tanfovx, cam.tanfovy, f(v), f(p), f(c))


def pose_error(w2c, w2c_true, zbar):
    """(translation error / mean depth, rotation error in degrees) between two W2C matrices"""
    d = np.asarray(w2c, np.float64) @ np.linalg.inv(np.asarray(w2c_true, np.float64))
    ang = math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(d[:3, :3]) - 1.0) / 2.0))))
    return float(np.linalg.norm(d[:3, 3]) / zbar), ang


def mean_depth(cl, cam, radii=None):
    z = cl.xyz.astype(np.float64) @ cam.viewmatrix.astype(np.float64)[:3, 2] + float(cam.viewmatrix[3, 2])
    z = z[radii > 0] if radii is not None else z[z > 0.2]
    return float(z.mean())


# ---------------------------------------------------------------------------------------------------- the library
def backward_pose(lib_path, a, cam, flags, dpix, deg=3, raw=0, pose=True, dD=None, dA=None, **bkw):
    """forward (training) + backward with the pose outputs; returns (the tuple of RasterizeGaussiansBackwardCUDA, radii)"""
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        a = dict(a, degree=deg)
        R, _, radii, g, b, i = rp.RasterizeGaussiansCUDA(**a, raw_params=flags | raw)
        out = rp.RasterizeGaussiansBackwardCUDA(a["background"], a["means3D"], radii, a["colors"], a["scales"], a["rotations"], 1.0,
                                                a["cov3D_precomp"], a["viewmatrix"], a["projmatrix"], cam.tanfovx, cam.tanfovy, dpix,
                                                a["sh"], deg, a["campos"], g, R, b, i, raw_params=raw, dL_ddepth=dD, dL_dalpha=dA,
                                                pose_grad=pose, **bkw)
        if a["means3D"].is_cuda:
            torch.cuda.synchronize()
        return out, radii
    finally:
        rp._LIB_OVERRIDE = prev


def member_from_oracle(res, H, W, P):
    """tile membership per pixel from the oracle's sorted lists (test_oracle_pinning.py)"""
    member = np.zeros((H * W, P), bool)
    gx = res.grid[0]
    for t in range(res.T):
        lst = res.point_list[res.ranges[t, 0]:res.ranges[t, 1]]
        ty, tx = divmod(t, gx)
        for yy in range(ty * 16, min(H, ty * 16 + 16)):
            member[yy * W + tx * 16: yy * W + min(W, tx * 16 + 16), :][:, lst] = True
    return member


def _rel(x, y, live=None):
    x, y = np.asarray(x, np.float64).reshape(-1), np.asarray(y, np.float64).reshape(-1)
    if live is not None:
        x, y = x[live], y[live]
    return float(np.abs(x - y).sum() / (np.abs(y).sum() + 1e-30))


# Deviation from the issue, which asks for bit-identity on the GPU too: on the MI355X the PARENT's backward pass is not
# bit-reproducible.  blend_bwd merges some of its sums with LDS float atomics whose order varies from run to run (measured: two
# plain passes at C3 differ in 25 000 elements of dL_dopacity by 4e-8 relative and in nothing else; at C1, the quad form, in
# thousands of elements of every gradient by 2e-8 ... 9e-8).  So on the device
#   * another output of a call with the pose outputs is held to DEVICE_RERUN_TOL of the call without them, the bar
#     tests/test_gpu_parity.py (test_forward_is_deterministic_and_backward_is_stable) applies to two runs of one program;
#   * the 35 floats of two calls must be bit-identical whenever every per-Gaussian gradient the sums are formed from is
#     bit-identical between THOSE SAME two calls (all of the eight but dL_dopacity: the sums read none of its terms) -- that is
#     the determinism of the new reduction, tested whenever its inputs allow -- and are held to DEVICE_RERUN_TOL otherwise.
# On the emulator everything is asserted bit for bit, unconditionally.
DEVICE_RERUN_TOL = 1e-5


def same_or_rerun_close(name, x, y, exact):
    if exact:
        assert torch.equal(x, y), f"{name} differs"
    else:
        assert parity.rel_l1(x.cpu().numpy(), y.cpu().numpy()) <= DEVICE_RERUN_TOL, f"{name} differs by more than two runs of one program may"


def pose_same_or_close(out_a, out_b, what, exact):
    """out_a, out_b: the tuples of eleven of two calls (see the comment above).  Returns whether the two calls' per-Gaussian
    gradients were bit-identical (then the 35 floats were asserted bit-identical too)."""
    inputs_same = all(torch.equal(x, y) for k, (x, y) in enumerate(zip(out_a[:8], out_b[:8])) if k != 2 and x is not None and y is not None)
    if exact:
        assert inputs_same, what + " (the per-Gaussian gradients differ)"
    for x, y in zip(out_a[8:], out_b[8:]):
        if inputs_same:
            assert torch.equal(x, y), what
        elif bool(y.any()):
            assert parity.rel_l1(x.cpu().numpy(), y.cpu().numpy()) <= DEVICE_RERUN_TOL, what
    return inputs_same


def check_against_autograd(lib_path, dev, oracle, seed, deg):
    """(a): the three raw gradients and the 6-vector at xi = 0 against float64 autograd of torch_render, both binning arrangements;
    the entries the render does not depend on exactly 0; the autograd route through GaussianRasterizer gives the same 6-vector"""
    from photo_slam_amd.gaussian_rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    from photo_slam_amd.gaussian_renderer import GaussianKeyframe, PoseDelta
    W, H, P = 32, 24, 60
    cl = scene.make_cloud(P, W, H, 30.0, 30.0, seed=seed, scale_k=0.5)
    cam = cl.cameras[0]
    bg = np.array([0.3, 0.1, 0.6], np.float32)
    dpix = np.random.default_rng(seed).standard_normal((3, H, W)).astype(np.float32)
    scales, rots, opac, sh = cl.get_scaling(), cl.get_rotation(), cl.get_opacity(), cl.get_features()
    res, img, radii = oracle.forward(bg, cl.xyz, opac, cam.viewmatrix, cam.projmatrix, cam.campos, cam.tanfovx, cam.tanfovy, H, W,
                                     shs=sh, sh_degree=deg, scales=scales, rotations=rots)
    assert (res.fragile == 0).all(), "the scene has threshold-fragile pixels: not one of the cases the issue lists"
    member = torch.tensor(member_from_oracle(res, H, W, P))
    c64 = lambda x: torch.tensor(np.asarray(x, np.float64))
    g64 = lambda x: c64(x).requires_grad_(True)

    def render64(view_t, proj_t, campos):
        out = torch_render(c64(cl.xyz), c64(scales), c64(rots), c64(opac), c64(sh), view_t, proj_t, campos, float(cam.tanfovx),
                           float(cam.tanfovy), W, H, c64(bg), member, deg)
        return (out * c64(dpix)).sum()

    tv, tp, tc = g64(cam.viewmatrix), g64(cam.projmatrix), g64(cam.campos)
    render64(tv, tp, tc).backward()
    ref_c = tc.grad.numpy() if tc.grad is not None else np.zeros(3)
    w2c0, projT = base_of(cam)
    xi = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    render64(*camera_tensors64(xi, w2c0, projT)).backward()
    ref_xi = xi.grad.numpy()
    live_v = np.setdiff1d(np.arange(16), VIEW_DEAD)
    live_p = np.setdiff1d(np.arange(16), PROJ_DEAD)
    assert not tv.grad.numpy().reshape(-1)[VIEW_DEAD].any() and not tp.grad.numpy().reshape(-1)[PROJ_DEAD].any()
    rep = {}
    first = None
    for flags in (DEPTH_FIRST, TILE_FIRST):
        a = fo.inputs(cl, cam, bg, dev)
        out, lradii = backward_pose(lib_path, a, cam, flags, fo._t(dpix, dev), deg=deg)
        assert np.array_equal(lradii.cpu().numpy(), radii)
        gv, gp, gc = (t.cpu().numpy() for t in out[8:])
        assert gv.shape == (4, 4) and gp.shape == (4, 4) and gc.shape == (3,)
        assert not gv.reshape(-1)[VIEW_DEAD].any() and not gp.reshape(-1)[PROJ_DEAD].any(), "an entry the render does not depend on is not 0"
        r = dict(view=_rel(gv, tv.grad.numpy(), live_v), proj=_rel(gp, tp.grad.numpy(), live_p),
                 xi=_rel(chain_to_xi(gv, gp, gc, cam), ref_xi))
        if not ref_c.any():
            assert not gc.any(), "dL_dcampos must be exactly 0 where the reference's is"
        else:
            r["campos"] = _rel(gc, ref_c)
        print("measured:", seed, deg, flags, r)
        assert max(r.values()) <= AUTOGRAD_TOL, r
        if first is None:
            first = out
        else:   # depth-first and tile-first: the same 35 floats
            same = pose_same_or_close(first, out, "the binning arrangements gave different pose gradients", dev.type == "cpu")
            print("measured: per-Gaussian gradients of the two arrangements bit-identical:", same)
        rep[flags] = r
    # the autograd route: a PoseDelta at xi = 0 through GaussianRasterizer
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        pose = PoseDelta.from_keyframe(GaussianKeyframe.from_camera(cam, dev))
        kf = pose.keyframe()
        s = GaussianRasterizationSettings(H, W, cam.tanfovx, cam.tanfovy, fo._t(bg, dev), 1.0, kf.world_view_transform_,
                                          kf.full_proj_transform_, deg, kf.camera_center_, False)
        a = fo.inputs(cl, cam, bg, dev)
        outs = GaussianRasterizer(s)(a["means3D"], torch.zeros_like(a["means3D"]), a["opacity"], True, False, True, True, False,
                                     shs=a["sh"], scales=a["scales"], rotations=a["rotations"])
        assert outs[0].requires_grad, "a render in which only the camera requires grad must take the training path"
        (outs[0] * fo._t(dpix, dev)).sum().backward()
        assert pose.xi_.grad is not None
        rep["xi_autograd"] = _rel(pose.xi_.grad.cpu().numpy(), ref_xi)
        print("measured: xi through autograd", rep["xi_autograd"])
        assert rep["xi_autograd"] <= AUTOGRAD_TOL, rep
    finally:
        rp._LIB_OVERRIDE = prev
    return rep


def check_depth_against_autograd(lib_path, dev, oracle, seed):
    """POSE x DEPTH: a loss <dD, depth map> alone.  dL_dviewmatrix (dL/dz joins dL/dt_z) and dL_dprojmatrix against float64
    autograd of the depth render of the independent renderer (_depth64: colours z(view), no background); bar AUTOGRAD_TOL"""
    W, H, P = 32, 24, 60
    cl = scene.make_cloud(P, W, H, 30.0, 30.0, seed=seed, scale_k=0.5)
    cam = cl.cameras[0]
    bg = np.array([0.3, 0.1, 0.6], np.float32)
    dD = np.random.default_rng(seed + 100).standard_normal((H, W)).astype(np.float32)
    res, _, radii = oracle.forward(bg, cl.xyz, cl.get_opacity(), cam.viewmatrix, cam.projmatrix, cam.campos, cam.tanfovx, cam.tanfovy,
                                   H, W, shs=cl.get_features(), sh_degree=0, scales=cl.get_scaling(), rotations=cl.get_rotation())
    assert (res.fragile == 0).all()
    member = torch.tensor(member_from_oracle(res, H, W, P))
    g64 = lambda x: torch.tensor(np.asarray(x, np.float64)).requires_grad_(True)
    tv, tp = g64(cam.viewmatrix), g64(cam.projmatrix)
    d = _depth64(cl, tv, tp, float(cam.tanfovx), float(cam.tanfovy), W, H, member)
    (d * torch.tensor(dD.astype(np.float64))).sum().backward()
    a = fo.inputs(cl, cam, bg, dev)
    out, _ = backward_pose(lib_path, a, cam, 0, torch.zeros((3, H, W), device=dev), deg=0, dD=fo._t(dD, dev))
    gv, gp, gc = (t.cpu().numpy() for t in out[8:])
    live_v, live_p = np.setdiff1d(np.arange(16), VIEW_DEAD), np.setdiff1d(np.arange(16), PROJ_DEAD)
    r = dict(view=_rel(gv, tv.grad.numpy(), live_v), proj=_rel(gp, tp.grad.numpy(), live_p))
    print("measured: depth upstream", seed, r)
    assert not gc.any() and not gv.reshape(-1)[VIEW_DEAD].any() and not gp.reshape(-1)[PROJ_DEAD].any()
    assert max(r.values()) <= AUTOGRAD_TOL, r
    return r


# ---------------------------------------------------------------------------------------------------- (b) the rigid-motion identity
def identity_terms(cam, xyz, g_mean, h_rot=None, rot=None, g_cov=None, cov=None):
    """per-Gaussian terms [V, 6] of the identity (module docstring), float64"""
    Wc = cam.viewmatrix.astype(np.float64).T
    R, tau = Wc[:3, :3], Wc[:3, 3]
    x, g = xyz.astype(np.float64), g_mean.astype(np.float64)
    t = x @ R.T + tau
    Rg = g @ R.T
    if g_cov is not None:
        c, d = cov.astype(np.float64), g_cov.astype(np.float64)
        sym = lambda m, off: np.stack([m[:, 0], off * m[:, 1], off * m[:, 2], off * m[:, 1], m[:, 3], off * m[:, 4], off * m[:, 2],
                                       off * m[:, 4], m[:, 5]], 1).reshape(-1, 3, 3)
        C, G = sym(c, 1.0), sym(d, 0.5)
        M = C @ G - G @ C
        w = 2.0 * np.stack([M[:, 1, 2], M[:, 2, 0], M[:, 0, 1]], 1)
    else:
        q, h = rot.astype(np.float64), h_rot.astype(np.float64)
        r, v = q[:, 0], q[:, 1:]
        w = np.zeros_like(v)
        for k in range(3):
            e = np.zeros(3)
            e[k] = 1.0
            w[:, k] = 0.5 * (-h[:, 0] * v[:, k] + (h[:, 1:] * (r[:, None] * e[None, :] + np.cross(e[None, :], v))).sum(1))
    return np.concatenate([Rg, np.cross(t, Rg) + w @ R.T], 1)


def check_rigid_identity(lib_path, dev, oracle, cl, cam, bg, flags, mode="colors", upstream="random", seed=0):
    """(b) for one view.  mode: "sh0" (SH degree 0), "colors" (colors_precomp), "cov" (colors_precomp + cov3D_precomp).
    upstream: "random" or "coherent".  Returns the measured errors per component."""
    kw = dict(use_colors_precomp=mode != "sh0", use_cov3D_precomp=mode == "cov")
    deg = 0 if mode == "sh0" else 3
    a = fo.inputs(cl, cam, bg, dev, **kw)
    npy = lambda t: None if t is None or t.numel() == 0 else t.cpu().numpy()
    okw = dict(sh_degree=deg, use_colors_precomp=kw["use_colors_precomp"], colors=npy(a["colors"]),
               use_cov3D_precomp=kw["use_cov3D_precomp"], cov3D=npy(a["cov3D_precomp"]))
    if upstream == "random":
        dpix = np.random.default_rng(seed).standard_normal((3, cam.H, cam.W)).astype(np.float32)
    else:
        zbar = mean_depth(cl, cam)
        th = math.radians(0.5) * np.array(COHERENT_AXIS) / np.linalg.norm(COHERENT_AXIS)
        rho = 0.01 * zbar * np.array(COHERENT_DIRECTION) / np.linalg.norm(COHERENT_DIRECTION)
        _, target, _, _ = parity.run_oracle(oracle, cl, moved_camera(cam, np.concatenate([rho, th])), bg, do_backward=False, **okw)
        _, here, _, _ = parity.run_oracle(oracle, cl, cam, bg, do_backward=False, **okw)
        dpix = (np.sign(here - target) / here.size).astype(np.float32)
    res, _, oradii, og = parity.run_oracle(oracle, cl, cam, bg, dL_dpix=dpix, **okw)
    vis = oradii > 0
    if mode == "cov":
        terms = identity_terms(cam, cl.xyz[vis], og["dL_dmeans3D"][vis], g_cov=og["dL_dcov3D"][vis], cov=npy(a["cov3D_precomp"])[vis])
    else:
        terms = identity_terms(cam, cl.xyz[vis], og["dL_dmeans3D"][vis], h_rot=og["dL_drotations"][vis], rot=cl.get_rotation()[vis])
    total, mass = terms.sum(0), np.abs(terms).sum(0)
    if upstream == "coherent":
        signal = np.abs(total) / mass
        print("measured: oracle |sum| / mass", signal)
        assert (signal >= COHERENT_MIN_SIGNAL).all(), ("the oracle's own sum is not coherent in every component: pick another perturbation", signal)
    reps, first = [], None
    for f in (flags if isinstance(flags, (tuple, list)) else (flags,)):   # (one oracle run serves every binning arrangement)
        out, radii = backward_pose(lib_path, a, cam, f, fo._t(dpix, dev), deg=deg)
        assert np.array_equal(radii.cpu().numpy(), oradii)
        gv, gp, gc = (t.cpu().numpy() for t in out[8:])
        assert not gc.any(), "dL_dcampos must be exactly 0 for view-independent colour"
        assert not gv.reshape(-1)[VIEW_DEAD].any() and not gp.reshape(-1)[PROJ_DEAD].any()
        got = chain_to_xi(gv, gp, gc, cam)
        err = np.abs(got - total) / (mass if upstream == "random" else np.abs(total))
        rep = dict(mode=mode, upstream=upstream, flags=f, err=[float(e) for e in err], visible=int(vis.sum()))
        print("measured:", rep)
        assert (err <= (parity.GRAD_REL_L1_TOL if upstream == "random" else COHERENT_TOL)).all(), rep
        if first is None:
            first = out
        else:
            same = pose_same_or_close(first, out, "the binning arrangements gave different pose gradients", dev.type == "cpu")
            print("measured: per-Gaussian gradients of the two arrangements bit-identical:", same)
        reps.append(rep)
    return reps if isinstance(flags, (tuple, list)) else reps[0]


# ---------------------------------------------------------------------------------------------------- (c) unchanged behaviour
def check_unchanged(lib_path, dev, cl, cam, bg, flags, deg=3, raw=0, sh_coeffs=None, maps=False, stats=False, seed=0, **kw):
    """Every other output of the backward pass bit-identical with and without the pose outputs; two calls with them give the same
    35 floats bit for bit; returns the 35 floats.  sh_coeffs: a compact [P,M,3] SH tensor (the in-kernel SH backward)."""
    rng = np.random.default_rng(seed)
    P = cl.xyz.shape[0]
    dpix = fo._t(rng.standard_normal((3, cam.H, cam.W)).astype(np.float32), dev)
    dD = fo._t(rng.standard_normal((cam.H, cam.W)).astype(np.float32), dev) if maps else None
    dA = fo._t(rng.standard_normal((cam.H, cam.W)).astype(np.float32), dev) if maps else None

    def run(pose):
        sh = fo._t(np.ascontiguousarray(cl.get_features()[:, :sh_coeffs]), dev) if sh_coeffs else None
        a = fo.inputs(cl, cam, bg, dev, sh=sh, **kw)
        vs = tuple(torch.full((P,), 0.25, device=dev) for _ in range(3)) if stats else None
        out, radii = backward_pose(lib_path, a, cam, flags, dpix, deg=deg, raw=raw, pose=pose, dD=dD, dA=dA, view_stats=vs)
        return out, vs

    exact = dev.type == "cpu"
    plain, vs0 = run(False)
    one, vs1 = run(True)
    two, _ = run(True)
    assert len(plain) == 8 and len(one) == 11
    for name, x, y in zip(GRAD_NAMES, plain, one):
        assert (x is None) == (y is None), name
        if x is not None:
            same_or_rerun_close(name + " with the pose outputs requested", y, x, exact)
    if stats:
        for x, y in zip(vs0, vs1):
            same_or_rerun_close("a fused statistic with the pose outputs requested", y, x, exact)
    same = pose_same_or_close(one, two, "two calls on the same inputs gave different pose gradients", exact)
    assert all(torch.isfinite(x).all() for x in one[8:])
    print("measured: per-Gaussian gradients of the two calls bit-identical:", same)
    return one


def check_unchanged_fused(lib_path, dev, cl, cam, bg, flags, lazy=False, seed=0):
    """raw parameters + sh_adam (eager or lazy) + geom_adam + the fused statistics: parameters, moments, row_step and statistics
    after the step are bit-identical with and without the pose outputs, and the pose gradients equal those of the unfused call
    on the same (pre-step) inputs bit for bit -- the sums use the positions as they were before the fused xyz step"""
    rng = np.random.default_rng(seed)
    P = cl.xyz.shape[0]
    raw = capi.RAW_OPACITY | capi.RAW_SCALING | capi.RAW_ROTATION
    dpix = fo._t(rng.standard_normal((3, cam.H, cam.W)).astype(np.float32), dev)
    names = ("xyz", "opacity", "scaling", "rotation")
    init = dict(xyz=cl.xyz, opacity=cl.opacity.reshape(P, 1), scaling=cl.scaling, rotation=cl.rotation, sh=cl.get_features())
    mom = {n: ((0.01 * rng.standard_normal(init[n].shape)).astype(np.float32), (1e-4 * rng.random(init[n].shape)).astype(np.float32))
           for n in init}
    lrs = dict(xyz=1.6e-4, opacity=0.05, scaling=0.005, rotation=0.001)
    row_step0 = np.full(P, 3, np.int32)   # (every row up to date: the lazy forward pass then changes no SH row, and the unfused call renders the same model)

    def run(pose, fused=True):
        st = {n: [fo._t(init[n].copy(), dev).clone(), fo._t(mom[n][0].copy(), dev).clone(), fo._t(mom[n][1].copy(), dev).clone()]
              for n in init}
        a = fo.inputs(cl, cam, bg, dev, sh=st["sh"][0])
        a.update(means3D=st["xyz"][0], opacity=st["opacity"][0], scales=st["scaling"][0], rotations=st["rotation"][0])
        bkw = {}
        row_step = fo._t(row_step0.copy(), dev)
        if fused:
            bkw["geom_adam"] = dict(tensors=[(st[n][0], st[n][1], st[n][2], lrs[n], 4) for n in names], beta1=0.9, beta2=0.999, eps=1e-15)
            sa = dict(exp_avg=st["sh"][1], exp_avg_sq=st["sh"][2], lr=0.0025, lr_tail=0.000125, beta1=0.9, beta2=0.999, eps=1e-15, step=4)
            if lazy:
                sa.update(row_step=row_step, window=4, lr_past=[0.0025] * 3, lr_tail_past=[0.000125] * 3)
            bkw["sh_adam"] = sa
            bkw["view_stats"] = tuple(torch.full((P,), 0.25, device=dev) for _ in range(3))
            bkw["training_outputs_only"] = True
        prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
        try:
            R, _, radii, g, b, i = rp.RasterizeGaussiansCUDA(**a, raw_params=flags | raw, sh_adam=bkw.get("sh_adam") if lazy else None)
            out = rp.RasterizeGaussiansBackwardCUDA(a["background"], a["means3D"], radii, a["colors"], a["scales"], a["rotations"], 1.0,
                                                    a["cov3D_precomp"], a["viewmatrix"], a["projmatrix"], cam.tanfovx, cam.tanfovy, dpix,
                                                    a["sh"], 3, a["campos"], g, R, b, i, raw_params=raw, pose_grad=pose, **bkw)
        finally:
            rp._LIB_OVERRIDE = prev
        state = [t for n in init for t in st[n]] + [row_step] + list(bkw.get("view_stats", ()))
        return out, state

    exact = dev.type == "cpu"
    o0, s0 = run(False)
    o1, s1 = run(True)
    for k, (x, y) in enumerate(zip(s0, s1)):
        same_or_rerun_close(f"state tensor {k} of the fused step, with the pose outputs requested,", y, x, exact)
    assert not torch.equal(s1[0], fo._t(init["xyz"], dev)), "the fused xyz step did not happen"
    # the fused call returns no per-Gaussian gradients to condition on: its 35 floats are compared with the unfused call's bit for
    # bit on the emulator, to the rerun bar on the device
    o2, _ = run(True, fused=False)
    for x, y in zip(o1[8:], o2[8:]):
        if exact or bool(y.any()):
            same_or_rerun_close("the pose gradients of the fused step against the unfused call's:", x, y, exact)
    return o1[8:]


def check_api_contract(lib_path, dev, cl, cam, bg):
    """all four pointers or none; refused together with dL_dcolor_view; P == 0 and a view that sees nothing write zeros"""
    import ctypes as C
    lib = capi.load(lib_path)
    assert int(lib.gsr_pose_grad_scratch_bytes(0)) >= 0 and int(lib.gsr_pose_grad_scratch_bytes(1000)) >= 4 * (24 * 8 + 3 * 16)
    a = fo.inputs(cl, cam, bg, dev)
    dpix = torch.ones((3, cam.H, cam.W), device=dev)
    P = cl.xyz.shape[0]
    try:
        backward_pose(lib_path, a, cam, 0, dpix, dL_dcolor_view=torch.zeros((P, 3), device=dev))
        raise AssertionError("pose_grad together with dL_dcolor_view was accepted")
    except RuntimeError:
        pass
    # the C-ABI directly: three of the four pointers
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        R, _, radii, g, b, i = rp.RasterizeGaussiansCUDA(**a, raw_params=0)
        grads = [torch.empty((P, n), device=dev) for n in (3, 4, 1, 3, 3, 6, 48, 3, 4)]
        pose = torch.full((35,), 7.0, device=dev)
        scratch = torch.empty((int(lib.gsr_pose_grad_scratch_bytes(P)),), dtype=torch.uint8, device=dev)
        ba = capi.BackwardArgs()
        ba.P, ba.D, ba.M, ba.R, ba.width, ba.height = P, 3, 16, R, cam.W, cam.H
        ba.scale_modifier, ba.tan_fovx, ba.tan_fovy = 1.0, cam.tanfovx, cam.tanfovy
        for n in ("background", "means3D", "scales", "rotations", "viewmatrix", "projmatrix", "campos"):
            setattr(ba, n, a[n].data_ptr())
        ba.shs, ba.radii, ba.dL_dpix = a["sh"].data_ptr(), radii.data_ptr(), dpix.data_ptr()
        ba.geom_buffer, ba.binning_buffer, ba.image_buffer = g.data_ptr(), b.data_ptr(), i.data_ptr()
        for n, t in zip(("dL_dmean2D", "dL_dconic", "dL_dopacity", "dL_dcolor", "dL_dmean3D", "dL_dcov3D", "dL_dsh", "dL_dscale", "dL_drot"), grads):
            setattr(ba, n, t.data_ptr())
        ba.dL_dviewmatrix, ba.dL_dprojmatrix, ba.dL_dcampos = pose.data_ptr(), pose.data_ptr() + 64, pose.data_ptr() + 128
        assert lib.gsr_backward(C.byref(ba), rp._stream_ptr(a["means3D"])) == -1, "three of the four pose pointers were accepted"
        assert bool((pose == 7.0).all())
        ba.pose_scratch = scratch.data_ptr()
        ba.dL_dcolor_view = grads[0].data_ptr()
        assert lib.gsr_backward(C.byref(ba), rp._stream_ptr(a["means3D"])) == -4, "pose outputs with dL_dcolor_view: GSR_ERR_UNSUPPORTED"
        ba.dL_dcolor_view = None
        ba.P = 0
        capi.check(lib, lib.gsr_backward(C.byref(ba), rp._stream_ptr(a["means3D"])), "P == 0")
        if dev.type != "cpu":
            torch.cuda.synchronize()
        assert bool((pose == 0.0).all()), "P == 0 must write 35 zeros"
    finally:
        rp._LIB_OVERRIDE = prev
    # a view that sees nothing: the camera turned away from the one Gaussian
    away = scene.make_camera(cam.W, cam.H, 80.0, 80.0, np.eye(3), np.array([0.0, 0.0, 50.0]))
    out, radii = backward_pose(lib_path, fo.inputs(cl, away, bg, dev), away, 0, dpix)
    assert not bool((radii > 0).any())
    assert all(not bool(t.any()) for t in out[8:])
    # the Python boundary at P == 0
    e = fo.inputs(cl, cam, bg, dev)
    for k in ("means3D", "opacity", "scales", "rotations", "sh"):
        e[k] = e[k][:0]
    out, _ = backward_pose(lib_path, e, cam, 0, dpix)
    assert len(out) == 11 and all(not bool(t.any()) for t in out[8:])


# ---------------------------------------------------------------------------------------------------- (d) refinement
REFINE_SCENE = dict(P=600, W=96, H=64, fx=90.0, fy=90.0, seed=2, scale_k=0.5)
REFINE_ITERS, REFINE_LR = 60, 2e-3
# The scene and the active SH degree were chosen by the float64 reference loop below (reference_refine, tile membership from the
# oracle's lists at every iterate): at degree 1 it ends at 0.021 % of the mean depth / 0.014 deg from a start of 1.75 % / 1.12 deg.
# At degree 3 the same scene does not serve: a large Gaussian at the near plane enters and leaves the lists as the pose moves (the
# loss jumps between 0.0015 and 0.028) and the loop ends where it began; seeds 0, 1, 3 ... 8 at degree 3 end above a tenth of the
# start in rotation within 60 steps.  Degree 1 keeps the view-direction term (dL_dcampos) in the refinement.
REFINE_DEGREE = 1
REFINE_DEPTH_RANGE = (0.1, 100.0)
# the depth case's weight, chosen by the same reference loop with its depth term: at 0.01 it ends at 0.016 % / 0.016 deg; at 0.1 at
# 0.073 % / 0.200 deg and at 0.3 at 0.51 % / 1.12 deg within the 60 steps (the library follows it: 0.073 % / 0.200 deg at 0.1) -- the
# sign gradients of the depth L1 then dominate Adam's normalised step, whose jitter at lr 2e-3 rad is the size of the bound
REFINE_DEPTH_WEIGHT = 0.01
REFINE_START = ((0.010, -0.008, 0.012), (0.6, -0.8, 0.5))   # rho / mean depth, theta in degrees


def refine_setup():
    """(cloud, true camera, start camera, mean depth, target image of the float64 renderer at the true pose) of the refinement
    test: the start pose is the true one moved by REFINE_START"""
    cl = scene.make_cloud(**REFINE_SCENE)
    cam = cl.cameras[0]
    zbar = mean_depth(cl, cam)
    xi0 = np.concatenate([np.array(REFINE_START[0]) * zbar, np.radians(REFINE_START[1])])
    return cl, cam, moved_camera(cam, xi0), zbar


def _oracle_member(oracle, cl, cam, deg):
    res, img, radii = oracle.forward(np.zeros(3, np.float32), cl.xyz, cl.get_opacity(), cam.viewmatrix, cam.projmatrix, cam.campos,
                                     cam.tanfovx, cam.tanfovy, cam.H, cam.W, shs=cl.get_features(), sh_degree=deg,
                                     scales=cl.get_scaling(), rotations=cl.get_rotation())
    return torch.tensor(member_from_oracle(res, cam.H, cam.W, cl.xyz.shape[0])), img


def _depth64(cl, view_t, proj_t, tanx, tany, W, H, member):
    """the depth map sum z alpha T of the float64 renderer: a render with the colours (z, z, z), z = the view-space depth of the
    mean (a function of the pose), and no background -- the blend is linear in the colours (depth_alpha_cases.py)"""
    c64 = lambda x: torch.tensor(np.asarray(x, np.float64))
    xyz = c64(cl.xyz)
    z = xyz @ view_t[:3, 2] + view_t[3, 2]
    sh = torch.zeros(xyz.shape[0], 16, 3, dtype=torch.float64)
    sh = torch.cat([((z - 0.5) / 0.28209479177387814)[:, None, None].expand(-1, 1, 3), sh[:, 1:]], 1)
    out = torch_render(xyz, c64(cl.get_scaling()), c64(cl.get_rotation()), c64(cl.get_opacity()), sh, view_t, proj_t,
                       torch.zeros(3, dtype=torch.float64), tanx, tany, W, H, torch.zeros(3, dtype=torch.float64), member, 0)
    return out[0]


def reference_refine(oracle, cl, cam_true, cam_start, zbar, deg=REFINE_DEGREE, iterations=REFINE_ITERS, lr=REFINE_LR, depth_weight=0.0):
    """The float64 reference loop: Adam on xi, plain L1 to the oracle's render at the true pose, torch_render with the oracle's
    tile lists at the current pose; depth_weight != 0 adds depth_weight * the L1 distance of the depth map to the one at the true
    pose over the pixels with REFINE_DEPTH_RANGE, divided by H W (loss_utils.depth_l1_loss).  Returns (initial errors, final
    errors, losses)."""
    c64 = lambda x: torch.tensor(np.asarray(x, np.float64))
    member_true, target = _oracle_member(oracle, cl, cam_true, deg)
    target = c64(target)
    tanx, tany = float(cam_true.tanfovx), float(cam_true.tanfovy)
    if depth_weight:
        with torch.no_grad():
            gt_depth = _depth64(cl, c64(cam_true.viewmatrix), c64(cam_true.projmatrix), tanx, tany, cam_true.W, cam_true.H, member_true)
        valid = (gt_depth > REFINE_DEPTH_RANGE[0]) & (gt_depth < REFINE_DEPTH_RANGE[1])
    w2c0, projT = base_of(cam_start)
    xi = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([xi], lr=lr)
    w2c_true = cam_true.viewmatrix.T
    first = pose_error(w2c0.numpy(), w2c_true, zbar)
    losses = []
    for _ in range(iterations):
        with torch.no_grad():
            here = moved_camera(cam_start, xi.numpy())
        member, _ = _oracle_member(oracle, cl, here, deg)
        v, p, c = camera_tensors64(xi, w2c0, projT)
        img = torch_render(c64(cl.xyz), c64(cl.get_scaling()), c64(cl.get_rotation()), c64(cl.get_opacity()), c64(cl.get_features()),
                           v, p, c, float(cam_true.tanfovx), float(cam_true.tanfovy), cam_true.W, cam_true.H,
                           torch.zeros(3, dtype=torch.float64), member, deg)
        loss = (img - target).abs().mean()
        if depth_weight:
            d = _depth64(cl, v, p, tanx, tany, cam_true.W, cam_true.H, member)
            loss = loss + depth_weight * ((d - gt_depth).abs() * valid).sum() / d.numel()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        last = pose_error((exp64(xi) @ w2c0).numpy(), w2c_true, zbar)
    return first, last, losses


def refine_bound(first, ref_last):
    """the bound of the issue: twice the reference loop's final error or a tenth of the initial error, whichever is larger -- and
    the reference itself must end below the tenth"""
    assert ref_last[0] <= first[0] / 10 and ref_last[1] <= first[1] / 10, ("the reference loop does not converge on this scene", first, ref_last)
    return max(2 * ref_last[0], first[0] / 10), max(2 * ref_last[1], first[1] / 10)


def python_trainer(cl, dev, deg=REFINE_DEGREE):
    import copy
    from photo_slam_amd.gaussian_model import GaussianModel, GaussianOptimizationParams
    from photo_slam_amd.gaussian_renderer import GaussianPipelineParams
    from photo_slam_amd.trainer import TrainStep
    g = GaussianModel.from_cloud(copy.deepcopy(cl), device=dev)
    g.active_sh_degree_ = deg
    opt = GaussianOptimizationParams()
    opt.lambda_dssim_ = 0.0
    g.trainingSetup(opt)
    return g, TrainStep(g, opt, GaussianPipelineParams(), torch.zeros(3, device=dev), cameras_extent=float(cl.extent), seed=7)


def _snapshot(g, ts):
    o = g.optimizer_
    t = [p.detach().clone() for p in g.params_raw()]
    for p in g.params_raw():
        st = o.state.get(id(p), {})
        t += [v.clone() for k, v in sorted(st.items()) if torch.is_tensor(v)]
    t += [b.clone() for b in ts.workspace_.bufs if b is not None]
    return t


def check_refine_python(lib_path, dev, oracle, with_depth=False, train_steps=3):
    """(d) on the Python host: after a few train steps (so that Adam moments, lazy rows and the training workspace exist),
    refinePose from the start pose reaches the bound; model, moments, row_step and training workspace are bit-identical before
    and after"""
    from photo_slam_amd.gaussian_renderer import GaussianKeyframe
    cl, cam, start, zbar = refine_setup()
    first, ref_last, ref_losses = reference_refine(oracle, cl, cam, start, zbar, depth_weight=REFINE_DEPTH_WEIGHT if with_depth else 0.0)
    bound = refine_bound(first, ref_last)
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        g, ts = python_trainer(cl, dev)
        kf_true, kf_start = GaussianKeyframe.from_camera(cam, dev), GaussianKeyframe.from_camera(start, dev)
        with torch.no_grad():
            gt, gt_depth, _ = ts.render_view(kf_true, with_depth=True)
        gt, gt_depth = gt.clone(), gt_depth.clone()
        mask = torch.ones_like(gt)
        if train_steps:   # (against its own render: the model barely moves, but every piece of optimizer state comes to life)
            for _ in range(train_steps):
                ts.trainForOneIteration(kf_true, gt, mask, sync_loss=False)
            with torch.no_grad():
                gt, gt_depth, _ = ts.render_view(kf_true, with_depth=True)
            gt, gt_depth = gt.clone(), gt_depth.clone()
        if with_depth:
            ts.depth_loss_weight_, ts.depth_min_, ts.depth_max_ = (REFINE_DEPTH_WEIGHT,) + REFINE_DEPTH_RANGE
        before = _snapshot(g, ts)
        w2c, losses = ts.refinePose(kf_start, gt, mask, REFINE_ITERS, REFINE_LR, REFINE_LR, gt_depth=gt_depth if with_depth else None)
        after = _snapshot(g, ts)
    finally:
        rp._LIB_OVERRIDE = prev
    assert len(before) == len(after) and all(torch.equal(x, y) for x, y in zip(before, after)), "refinePose touched the map or its optimizer state"
    assert len(losses) == REFINE_ITERS and losses[-1] < losses[0]
    last = pose_error(w2c.cpu().numpy(), cam.viewmatrix.T, zbar)
    rep = dict(initial=first, reference_final=ref_last, library_final=last, bound=bound, loss=(losses[0], losses[-1]))
    print("measured:", rep)
    assert last[0] <= bound[0] and last[1] <= bound[1], rep
    return rep


# ---------------------------------------------------------------------------------------------------- the C++ host
def _cam_args(c, dev):
    t = lambda x: fo._t(x, dev)
    return (t(c.viewmatrix), t(c.projmatrix), t(c.campos), 2 * math.atan(c.tanfovx), 2 * math.atan(c.tanfovy), c.H, c.W)


def cpp_trainer(ops, cl, dev, deg=REFINE_DEGREE, depth_weight=0.0):
    import copy
    from photo_slam_amd.gaussian_model import GaussianModel
    g0 = GaussianModel.from_cloud(copy.deepcopy(cl), device=dev)
    h = ops.trainer_create(g0.xyz_.detach(), g0.features_.detach(), g0.opacity_.detach(), g0.scaling_.detach(), g0.rotation_.detach(),
                           3, float(cl.extent), torch.zeros(3, device=dev))
    ops.trainer_set_options(h, {"seed": 7.0, "cameras_extent": float(cl.extent), "lambda_dssim": 0.0, "active_sh_degree": float(deg),
                                "depth_loss_weight": float(depth_weight), "depth_min": 0.1, "depth_max": 100.0})
    return h


def check_refine_cpp(ops, lib_path, dev, oracle, with_depth=False, train_steps=3):
    """(d) on the C++ host (TrainStep::refinePose, op trainer_refine_pose): the bound of the reference loop; every tensor of
    trainer_state bit-identical before and after; the first iteration's loss equals the Python host's on the same model"""
    cl, cam, start, zbar = refine_setup()
    first, ref_last, _ = reference_refine(oracle, cl, cam, start, zbar, depth_weight=REFINE_DEPTH_WEIGHT if with_depth else 0.0)
    bound = refine_bound(first, ref_last)
    h = cpp_trainer(ops, cl, dev)
    try:
        gt, gt_depth, _ = ops.trainer_render_view_depth(h, *_cam_args(cam, dev))
        mask = torch.ones_like(gt)
        for _ in range(train_steps):
            ops.trainer_render_and_backward(h, *_cam_args(cam, dev), gt, mask)
            ops.trainer_finish(h)
        gt, gt_depth, _ = ops.trainer_render_view_depth(h, *_cam_args(cam, dev))
        gt, gt_depth = gt.clone(), gt_depth.clone()
        if with_depth:
            ops.trainer_set_options(h, {"depth_loss_weight": REFINE_DEPTH_WEIGHT})
        before = [t.clone() for t in ops.trainer_state(h)]
        w2c, losses = ops.trainer_refine_pose(h, *_cam_args(start, dev), gt, mask, REFINE_ITERS, REFINE_LR, REFINE_LR,
                                              gt_depth if with_depth else torch.empty(0, device=dev))
        after = ops.trainer_state(h)
        assert len(before) == len(after) and len(before) >= 15
        assert all(torch.equal(x, y) for x, y in zip(before, after)), "refinePose touched the map or its optimizer state"
        # the Python host on the same (trained) model, same images: the same first loss, and both within the bound
        prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
        try:
            from photo_slam_amd.gaussian_renderer import GaussianKeyframe
            g, ts = python_trainer(cl, dev)
            with torch.no_grad():
                for p, q in zip(g.params(), ops.trainer_params(h)):
                    p.copy_(q)
            if with_depth:
                ts.depth_loss_weight_, ts.depth_min_, ts.depth_max_ = (REFINE_DEPTH_WEIGHT,) + REFINE_DEPTH_RANGE
            w2c_py, losses_py = ts.refinePose(GaussianKeyframe.from_camera(start, dev), gt, mask, REFINE_ITERS, REFINE_LR, REFINE_LR,
                                              gt_depth=gt_depth if with_depth else None)
        finally:
            rp._LIB_OVERRIDE = prev
    finally:
        ops.trainer_destroy(h)
    losses = [float(x) for x in losses.cpu()]
    assert len(losses) == REFINE_ITERS and losses[-1] < losses[0]
    assert abs(losses[0] - losses_py[0]) <= 1e-5 * abs(losses_py[0]), (losses[0], losses_py[0])
    last = pose_error(w2c.cpu().numpy(), cam.viewmatrix.T, zbar)
    last_py = pose_error(w2c_py.cpu().numpy(), cam.viewmatrix.T, zbar)
    rep = dict(initial=first, reference_final=ref_last, cpp_final=last, python_final=last_py, bound=bound)
    print("measured:", rep)
    assert last[0] <= bound[0] and last[1] <= bound[1], rep
    assert last_py[0] <= bound[0] and last_py[1] <= bound[1], rep
    return rep


def check_pose_gradient_cpp(ops, lib_path, dev, exact=True):
    """dL/dxi at xi = 0 through the C++ host's autograd node (GaussianRasterizerFunctionPose behind GaussianRasterizerEx, op
    trainer_pose_gradient: only the camera requires grad) against the Python host's on the same model"""
    from photo_slam_amd.gaussian_rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    from photo_slam_amd.gaussian_renderer import GaussianKeyframe, PoseDelta
    cl = scene.make_cloud(600, 64, 48, 60.0, 60.0, seed=1)
    cam = cl.cameras[0]
    dpix = fo._t(np.random.default_rng(2).standard_normal((3, cam.H, cam.W)).astype(np.float32), dev)
    h = cpp_trainer(ops, cl, dev, deg=3)
    try:
        got = ops.trainer_pose_gradient(h, *_cam_args(cam, dev), dpix)
        params = [p.detach().clone() for p in ops.trainer_params(h)]
    finally:
        ops.trainer_destroy(h)
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        pose = PoseDelta.from_keyframe(GaussianKeyframe.from_camera(cam, dev))
        kf = pose.keyframe()
        s = GaussianRasterizationSettings(cam.H, cam.W, kf.tanfovx_, kf.tanfovy_, torch.zeros(3, device=dev), 1.0, kf.world_view_transform_,
                                          kf.full_proj_transform_, 3, kf.camera_center_, False, 7)
        xyz, sh, op, sc, rot = params
        out = GaussianRasterizer(s)(xyz, torch.zeros_like(xyz), op, True, False, True, True, False, sh, None, sc, rot, None)
        (out[0] * dpix).sum().backward()
    finally:
        rp._LIB_OVERRIDE = prev
    want = pose.xi_.grad
    assert got.shape == (6,) and float(want.abs().sum()) > 0
    err = parity.rel_l1(got.cpu().numpy(), want.cpu().numpy())
    print("measured: C++ vs Python dL/dxi", err)
    assert err <= (1e-6 if exact else 1e-4), err
