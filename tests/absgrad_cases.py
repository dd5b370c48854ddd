"""Shared checks of the absolute screen-space gradients (gsr_backward_args.dL_dmean2D_abs, gsr_densify_stats_abs; include/gsr.h)
for the emulator tests (test_absgrad.py) and the GPU tests (test_gpu_absgrad.py).

The reference is the CPU oracle, unchanged.  The backward blend is independent per pixel, so pixel p's own contribution g_p to
dL_dmeans2D is one oracle backward with a one-hot upstream gradient, and
    abs[g] = sum_p |oracle.backward(res, dpix * delta_p)["dL_dmeans2D"][g]|.
With depth / alpha upstream gradients the z-colour and the ones-colour renders of depth_alpha_cases.oracle_grads are added per
pixel, before the absolute value.  A reference is computed once per process and case (reference_abs) and shared, read-only.

Bars.  (a) is parity's: the aggregate relative L1 of dL_dmeans2D (GRAD_REL_L1_TOL) and the per-row bars parity.compare applies to
that tensor -- absolute sums have no cancellation, they need nothing looser.  (b), (c): REL_BAR = 1e-5 of the values themselves,
per component -- in every referenced case, for the single pixels and in the host tests (measured: <= 2e-7 and <= 3.1e-6, emulator
and MI355X).  Only check_bound_only, at the BASELINE shapes, has to allow for what hundreds of thousands of Gaussians bring: the two
sides come from different float32 arithmetic -- sum(w dx) A + sum(w dy) B against sum |w (2 A' dx + B' dy)| with the prescaled conic --
so each is within a few roundings of the magnitude of its two TERMS, o W/2 (|sum w dx A| + |sum w dy B|), not of their sum; for a
Gaussian that one or two pixels blend, on the line where A dx = -B dy, the terms cancel and the sum is small next to its own rounding
error (C2: 3 components of 10^6 short by up to 1.8e-5 of their value; a full C3 view: 6 of 4 10^6, up to 9e-4).  There the strict bar
is asserted for all but at most CANCEL_CAP of the components, and those few must still be within REL_BAR of the magnitude of their
terms (term_scale)."""
import functools

import numpy as np
import torch

import depth_alpha_cases as da
import forward_only_cases as fo
import parity
import pose_grad_cases as pg
from photo_slam_amd import capi
from photo_slam_amd import rasterize_points as rp
from photo_slam_amd import scene

BG = np.array([0.2, 0.5, 0.1], np.float32)
REL_BAR = 1e-5
# check_bound_only: the share of the components that may miss REL_BAR of their own value because their two terms cancel (module
# docstring) -- one in 100 000, i.e. at most 1 at C1, 10 at C2 and 40 at a C3 view
CANCEL_CAP = 1e-5
GSR_ERR_UNSUPPORTED = -4
FLAGS = (32, 64)            # GSR_BINNING_*: both arrangements
FORMS = ("0", "1")          # GSR_BWD_HALF_TILES: quads (four waves, 256-entry segments) / half tiles (two waves, 128-entry segments)
CASES = ("dense", "segments", "ragged", "long", "depth_alpha")
# (c): one pixel in each quad position of a pair of the half-tile form -- left quad, right quad -- and one in the lower half of
# the tile, all in tile 0
SINGLE_PIXELS = ((3, 2), (11, 5), (6, 12))   # (x, y)


def _scene(name):
    if name in ("dense", "depth_alpha"):
        return scene.make_cloud(300, 48, 32, 30, 30, seed=1)
    if name == "segments":
        # The dense scene's tile lists hold 65 ... 100 entries (300 Gaussians, half of them in view, cannot fill a 256-entry segment):
        # this one -- larger Gaussians, every tile's list longer than 300 entries, random upstream on every pixel like the dense
        # case -- takes both forms of the kernel across a segment boundary in every tile, with both pixels of every lane live
        return scene.make_cloud(500, 48, 32, 30, 30, seed=1, scale_k=1.0)
    if name == "ragged":
        return scene.make_cloud(300, 40, 24, 30, 30, seed=1)
    if name == "long":
        return scene.make_cloud(60, 160, 144, 100, 100, seed=5, scale_k=0.6)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name):
    """(cloud, camera, dpix, dD, dA) of a case; the arrays are shared: do not write to them"""
    cl = _scene(name)
    cam = cl.cameras[0]
    rng = np.random.default_rng(7)
    dpix = rng.standard_normal((3, cam.H, cam.W)).astype(np.float32)
    dD = dA = None
    if name == "long":
        # three whole tiles and 200 scattered pixels: per-pixel independence keeps the reference exact at about 1 000 oracle calls
        live = np.zeros((cam.H, cam.W), bool)
        gx = (cam.W + 15) // 16
        for t in (0, gx + 4, 5 * gx + 7):
            ty, tx = divmod(t, gx)
            live[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16] = True
        pick = rng.choice(cam.H * cam.W, 200, replace=False)
        live.reshape(-1)[pick] = True
        dpix = dpix * live[None]
    if name == "depth_alpha":
        dD = rng.standard_normal((cam.H, cam.W)).astype(np.float32)
        dA = rng.standard_normal((cam.H, cam.W)).astype(np.float32)
    return cl, cam, dpix, dD, dA


@functools.lru_cache(maxsize=None)
def _reference(name):
    from oracle import oracle
    cl, cam, dpix, dD, dA = case(name)
    threads = oracle.get_threads()
    oracle.set_threads(1)   # a one-pixel backward has nothing to share out
    try:
        a = fo.inputs(cl, cam, BG, torch.device("cpu"))
        res, _, oradii, full = parity.run_oracle(oracle, cl, cam, BG, dL_dpix=dpix)
        P = cl.xyz.shape[0]
        zero = np.zeros(3, np.float32)
        rz = r1 = None
        if dD is not None:
            rz, _, _ = da.oracle_forward(oracle, a, cl, cam, np.repeat(da.view_z(cl, cam)[:, None], 3, 1), zero)
        if dA is not None:
            r1, _, _ = da.oracle_forward(oracle, a, cl, cam, np.ones((P, 3), np.float32), zero)
        live = np.abs(dpix).sum(0) != 0
        for up in (dD, dA):
            if up is not None:
                live |= up != 0
        ab, signed = np.zeros((P, 2)), np.zeros((P, 2))
        dp = np.zeros((3, cam.H, cam.W), np.float32)
        for y, x in zip(*np.nonzero(live)):
            dp[:, y, x] = dpix[:, y, x]
            g = oracle.backward(res, dp)["dL_dmeans2D"][:, :2].astype(np.float64)
            dp[:, y, x] = 0
            for r2, up in ((rz, dD), (r1, dA)):
                if up is not None:
                    dp[0, y, x] = up[y, x]
                    g += oracle.backward(r2, dp)["dL_dmeans2D"][:, :2]
                    dp[0, y, x] = 0
            ab += np.abs(g)
            signed += g
        # the one-hot sums reproduce the oracle's own gradient (the premise of the reference); with depth / alpha: of the colour
        # render plus the two others, depth_alpha_cases.oracle_grads
        want = da.oracle_grads(oracle, a, cl, cam, BG, dpix, dD, dA)[0]["dL_dmeans2D"][:, :2] if (dD is not None or dA is not None) \
            else full["dL_dmeans2D"][:, :2]
        assert parity.rel_l1(signed, want) <= 1e-6, parity.rel_l1(signed, want)
        assert np.all(ab >= np.abs(signed) * (1 - 1e-12))
        ab.setflags(write=False)
        return ab, oradii, res.tiles_touched.copy(), res.ranges.copy()
    finally:
        oracle.set_threads(threads)


def reference_abs(name):
    """(abs [P,2] float64, oracle radii, tiles_touched, tile ranges) of a case: computed once, shared, read-only"""
    return _reference(name)


def _t(x, dev):
    return None if x is None else fo._t(x, dev)


def run(lib_path, dev, cl, cam, flags, dpix, dD=None, dA=None, absgrad=True, raw=0, **bkw):
    """forward + backward through the Python boundary; returns (the tuple of RasterizeGaussiansBackwardCUDA, radii, abs [P,2])"""
    a = fo.inputs(cl, cam, BG, dev)
    if raw:
        a.update(opacity=_t(cl.opacity, dev).clone(), scales=_t(cl.scaling, dev).clone(), rotations=_t(cl.rotation, dev).clone(),
                 means3D=a["means3D"].clone(), sh=a["sh"].clone())
    ab = torch.full((cl.xyz.shape[0], 2), float("nan"), device=dev) if absgrad else None   # (every row must be written)
    out, radii = da.backward(lib_path, a, cam, flags, _t(dpix, dev), _t(dD, dev), _t(dA, dev), raw=raw, absgrad=ab, **bkw)
    return out, radii, ab


def term_scale(lib_path, dev, cl, cam, flags, g2d, raw=0):
    """[P,2]: the magnitude of the two terms whose sum a component of dL_dmean2D is, o W/2 (|u A| + |v B|) and o H/2 (|u B| + |v C|)
    with (u, v) = (sum w dx, sum w dy) recovered from dL_dmean2D itself and the conic and opacity of the library's own blend
    records (module docstring: what REL_BAR is relative to where the two terms cancel)."""
    import ctypes as C
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        a = fo.inputs(cl, cam, BG, dev)
        if raw:
            a.update(opacity=_t(cl.opacity, dev), scales=_t(cl.scaling, dev), rotations=_t(cl.rotation, dev))
        P = cl.xyz.shape[0]
        _, _, _, geom, _, _ = rp.RasterizeGaussiansCUDA(**a, raw_params=flags | raw)
        lib, dlib = capi.load(lib_path), parity.devapi.load(lib_path)
        gv = parity.devapi.GeometryView()
        capi.check(lib, dlib.gsr_view_geometry(C.c_void_p(geom.data_ptr()), P, C.byref(gv)), "view_geometry")
        rec = parity._slice(geom, gv.rec, 12 * P, np.float32).reshape(P, 12).astype(np.float64)
    finally:
        rp._LIB_OVERRIDE = prev
    A, B, Cc, o = rec[:, 2], rec[:, 3], rec[:, 4], rec[:, 5]
    hw, hh = 0.5 * cam.W, 0.5 * cam.H
    with np.errstate(all="ignore"):
        gx, gy = g2d[:, 0].astype(np.float64) / (o * hw), g2d[:, 1].astype(np.float64) / (o * hh)
        det = A * Cc - B * B
        u, v = -(Cc * gx - B * gy) / det, -(A * gy - B * gx) / det
        scale = np.stack([o * hw * (np.abs(u * A) + np.abs(v * B)), o * hh * (np.abs(u * B) + np.abs(v * Cc))], 1)
    return np.nan_to_num(scale, nan=0.0, posinf=0.0, neginf=0.0)


def component_bar(ab, signed):
    """REL_BAR of the values themselves (the larger of the two sides), per component"""
    return REL_BAR * np.maximum(np.abs(ab), np.abs(signed))


def check_bound(ab, g2d, scale=None):
    """(b) abs >= |dL_dmean2D| componentwise, to REL_BAR of the values.  scale (check_bound_only alone: term_scale): at most
    CANCEL_CAP of the components may miss that bar, and those must be within REL_BAR of the magnitude of their terms."""
    ab, s = ab.astype(np.float64), np.abs(g2d[:, :2].astype(np.float64))
    short = s - ab
    worst = float((short / np.maximum(s, 1e-300)).max(initial=0.0))
    over = short > component_bar(ab, s)
    print(f"bound: worst relative shortfall {worst:.3e}; components beyond {REL_BAR:g} of their own value: {int(over.sum())} of {over.size}")
    if scale is None:
        assert not over.any(), (worst, int(over.sum()))
    else:
        assert over.sum() <= CANCEL_CAP * over.size, (worst, int(over.sum()), over.size)
        assert np.all(short[over] <= REL_BAR * scale[over]), worst
    return worst


def check_unchanged(out_abs, out_plain, exact):
    """(d) every other output equals the call without the field: bit for bit on the emulator, to the rerun tolerance on the device"""
    for name, x, y in zip(da.GRAD_NAMES, out_abs, out_plain):
        assert (x is None) == (y is None), name
        if x is not None and x.numel():
            pg.same_or_rerun_close(name, x, y, exact)


def check_case(lib_path, dev, name, flags, exact):
    """(a), (b), (d) of a case against its reference, and what the case is there to cover; returns the report"""
    check_shape_of_case(name)
    cl, cam, dpix, dD, dA = case(name)
    ref, oradii, tiles_touched, ranges = reference_abs(name)
    out, radii, ab_t = run(lib_path, dev, cl, cam, flags, dpix, dD, dA)
    ab = ab_t.cpu().numpy()
    assert np.array_equal(radii.cpu().numpy(), oradii)
    vis = oradii > 0
    assert np.isfinite(ab).all() and np.all(ab >= 0) and not ab[~vis].any(), "a row is not written, negative, or non-zero for a culled Gaussian"
    rep = dict(rel_l1=parity.rel_l1(ab, ref))
    e = parity.row_errors(ab, ref)
    ev, el = e[vis], e[vis & (tiles_touched > 64)]
    rep.update(p9999=float(np.quantile(ev, 0.9999)), max=float(ev.max()), beyond=int((ev > parity.ROW_OUTLIER).sum()),
               long_rows=int(el.size), long_max=float(el.max(initial=0.0)), long_beyond=int((el > parity.ROW_OUTLIER).sum()))
    print(name, flags, rep)
    assert rep["rel_l1"] <= parity.GRAD_REL_L1_TOL, rep
    assert rep["p9999"] <= parity.ROW_P9999_TOL and rep["max"] <= parity.ROW_MAX_TOL, rep
    assert rep["beyond"] <= max(3, parity.ROW_OUTLIER_FRAC * ev.size), rep
    assert rep["long_beyond"] <= max(2, parity.ROW_SUBSET_OUTLIER_FRAC * el.size), rep
    rep["bound"] = check_bound(ab, out[0].cpu().numpy())
    plain, _, _ = run(lib_path, dev, cl, cam, flags, dpix, dD, dA, absgrad=False)
    check_unchanged(out, plain, exact)
    return rep


def check_shape_of_case(name):
    """what a case is there to cover, asserted from the oracle's lists"""
    cl, cam, dpix, _, _ = case(name)
    _, oradii, tiles_touched, ranges = reference_abs(name)
    n = ranges[:, 1].astype(np.int64) - ranges[:, 0]
    if name in ("dense", "depth_alpha"):
        assert bool((np.abs(dpix).sum(0) != 0).all())   # both pixels of every lane are live
    if name == "segments":
        assert n.min() > 256, n   # every tile: both forms cross a segment boundary (128 / 256 entries) ...
        assert bool((np.abs(dpix).sum(0) != 0).all())   # ... with both pixels of every lane live
    if name == "ragged":
        assert cam.W % 16 and cam.H % 16 and cam.H % 16 <= 8   # out-of-image lanes; the last tile row has only its upper half
    if name == "long":
        assert (tiles_touched > 64).any(), tiles_touched.max()   # long_run_sums_kernel
        assert ((tiles_touched > 0) & (tiles_touched <= 64)).any()   # ... and the per-lane run sum
        assert 0 < (np.abs(dpix).sum(0) != 0).sum() <= 3 * 256 + 200


def check_single_pixel(lib_path, dev, flags):
    """(c) with the upstream gradient non-zero at one pixel only, abs == |dL_dmean2D|"""
    cl, cam, dpix, _, _ = case("dense")
    worst = 0.0
    for x, y in SINGLE_PIXELS:
        dp = np.zeros_like(dpix)
        dp[:, y, x] = dpix[:, y, x]
        out, _, ab = run(lib_path, dev, cl, cam, flags, dp)
        g2d = out[0].cpu().numpy()
        ab, s = ab.cpu().numpy().astype(np.float64), np.abs(g2d[:, :2].astype(np.float64))
        assert s.any(), "the pixel blends nothing"
        d = np.abs(ab - s)
        worst = max(worst, float((d / np.maximum(np.maximum(ab, s), 1e-300)).max()))
        assert np.all(d <= component_bar(ab, s)), (x, y, worst)
    print(f"single pixel: worst relative difference {worst:.3e}")
    return worst


def check_fused_stats(lib_path, dev, flags, exact):
    """(e) stat_grad_accum after two views == the sum of the row norms of the two absolute arrays; gsr_densify_stats_abs: the same
    bits; stat_denom / stat_max_radii: those of the call without the field"""
    lib = capi.load(lib_path)
    cl = scene.make_cloud(300, 48, 32, 30, 30, seed=1, n_views=2)
    P = cl.xyz.shape[0]
    rng = np.random.default_rng(3)
    init = [rng.random(P).astype(np.float32), rng.integers(0, 5, P).astype(np.float32), rng.integers(0, 12, P).astype(np.float32)]
    fused = [_t(x.copy(), dev) for x in init]
    apart = [_t(x.copy(), dev) for x in init]
    plain = [_t(x.copy(), dev) for x in init]
    want = init[0].copy()
    seen = np.zeros(P, bool)
    for cam in cl.cameras:
        dpix = rng.standard_normal((3, cam.H, cam.W)).astype(np.float32)
        _, radii, ab = run(lib_path, dev, cl, cam, flags, dpix, view_stats=fused)
        run(lib_path, dev, cl, cam, flags, dpix, absgrad=False, view_stats=plain)
        capi.check(lib, lib.gsr_densify_stats_abs(P, ab.data_ptr(), radii.data_ptr(), apart[0].data_ptr(), apart[1].data_ptr(),
                                                  apart[2].data_ptr(), None), "gsr_densify_stats_abs")
        if dev.type != "cpu":
            torch.cuda.synchronize()
        a, vis = ab.cpu().numpy(), radii.cpu().numpy() > 0
        norm = np.sqrt(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1])   # float32, one rounding per operation: the kernels' arithmetic
        want = np.where(vis, want + norm, want).astype(np.float32)
        seen |= vis
    assert seen.any() and (~seen).any()
    for k in range(3):
        assert torch.equal(fused[k], apart[k]), f"gsr_densify_stats_abs differs from the fused statistics in output {k}"
    assert torch.equal(fused[1], plain[1]) and torch.equal(fused[2], plain[2])
    got = fused[0].cpu().numpy()
    if exact:
        assert np.array_equal(got, want)
    else:   # (the device's square root may differ from the host's in the last bit)
        assert np.allclose(got, want, rtol=1e-6, atol=0)
    assert (got[seen] > plain[0].cpu().numpy()[seen]).mean() > 0.5   # ... and it is not the signed statistic


def _adam_dicts(cl, dev, rng, a):
    P = cl.xyz.shape[0]
    names = ("means3D", "opacity", "scales", "rotations")
    lrs = (1.6e-4, 0.05, 0.005, 0.001)
    tensors = []
    for n, lr in zip(names, lrs):
        p = a[n]
        tensors.append((p, _t((0.01 * rng.standard_normal(tuple(p.shape))).astype(np.float32), dev),
                        _t((1e-4 * rng.random(tuple(p.shape))).astype(np.float32), dev), lr, 3))
    sh = a["sh"]
    sh_adam = dict(exp_avg=_t((0.01 * rng.standard_normal(tuple(sh.shape))).astype(np.float32), dev),
                   exp_avg_sq=_t((1e-4 * rng.random(tuple(sh.shape))).astype(np.float32), dev), lr=0.0025, lr_tail=0.0025 / 20,
                   beta1=0.9, beta2=0.999, eps=1e-15, step=3)
    return dict(tensors=tensors, beta1=0.9, beta2=0.999, eps=1e-15), sh_adam


def check_fused_optimizer_and_antialias(lib_path, dev, flags, exact, antialias):
    """(f) with geom_adam + sh_adam the absolute array equals the plain run's (rule of (d)), with and without GSR_ANTIALIAS"""
    cl, cam, dpix, _, _ = case("dense")
    raw = capi.RAW_OPACITY | capi.RAW_SCALING | capi.RAW_ROTATION
    fl = flags | (capi.ANTIALIAS if antialias else 0)
    _, _, plain = run(lib_path, dev, cl, cam, fl, dpix, raw=raw, antialiasing=antialias)
    assert bool(plain.isfinite().all()) and bool((plain > 0).any())

    a = fo.inputs(cl, cam, BG, dev)
    a.update(opacity=_t(cl.opacity, dev).clone(), scales=_t(cl.scaling, dev).clone(), rotations=_t(cl.rotation, dev).clone(),
             means3D=a["means3D"].clone(), sh=a["sh"].clone())
    before = a["means3D"].clone()
    ga, sa = _adam_dicts(cl, dev, np.random.default_rng(5), a)
    ab = torch.full((cl.xyz.shape[0], 2), float("nan"), device=dev)
    da.backward(lib_path, a, cam, fl, _t(dpix, dev), None, None, raw=raw, absgrad=ab, geom_adam=ga, sh_adam=sa,
                training_outputs_only=True, antialiasing=antialias)
    assert not torch.equal(before, a["means3D"]), "the fused step did not happen"
    pg.same_or_rerun_close("dL_dmean2D_abs", ab, plain, exact)
    if antialias:   # (and the compensated opacity is the one that scales it: not the array of the render without the bit)
        _, _, off = run(lib_path, dev, cl, cam, flags, dpix, raw=raw)
        assert not torch.equal(off, plain)


def check_with_regulariser_and_pose(lib_path, dev, flags, exact):
    """the absolute array next to geom_reg and next to the pose outputs: that of the plain run (rule of (d)), and theirs unchanged"""
    cl, cam, dpix, _, _ = case("dense")
    _, _, plain = run(lib_path, dev, cl, cam, flags, dpix)
    reg = dict(w_opacity=1e-3, w_scale=2e-3, w_isotropic=5e-4)
    out_r, _, ab_r = run(lib_path, dev, cl, cam, flags, dpix, geom_reg=reg)
    out_r0, _, _ = run(lib_path, dev, cl, cam, flags, dpix, geom_reg=reg, absgrad=False)
    pg.same_or_rerun_close("dL_dmean2D_abs (geom_reg)", ab_r, plain, exact)
    check_unchanged(out_r, out_r0, exact)
    out_p, _, ab_p = run(lib_path, dev, cl, cam, flags, dpix, pose_grad=True)
    out_p0, _, _ = run(lib_path, dev, cl, cam, flags, dpix, pose_grad=True, absgrad=False)
    pg.same_or_rerun_close("dL_dmean2D_abs (pose)", ab_p, plain, exact)
    check_unchanged(out_p[:8], out_p0[:8], exact)
    pg.pose_same_or_close(out_p, out_p0, "the pose gradients changed with dL_dmean2D_abs", exact)


def check_api_contract(lib_path, dev):
    """(g) a culled view writes zeros; P == 0 is accepted; the multi-GPU combination returns GSR_ERR_UNSUPPORTED"""
    cl, cam, dpix, _, _ = case("dense")
    # a camera outside the room that looks away from it: nothing is visible
    away = scene.make_camera(cam.W, cam.H, 30.0, 30.0, scene.look_rotation(np.pi / 2, 0.0), np.array([100.0, 0.0, 0.0]))
    out, radii, ab = run(lib_path, dev, cl, away, 0, dpix)
    assert not bool((radii > 0).any()) and bool((ab == 0).all()), "a culled view must write zeros"
    empty = scene.make_cloud(4, cam.W, cam.H, 30, 30, seed=1)
    for k in ("xyz", "features_dc", "features_rest", "scaling", "rotation", "opacity"):
        setattr(empty, k, getattr(empty, k)[:0])
    _, _, ab0 = run(lib_path, dev, empty, cam, 0, dpix)
    assert ab0.shape == (0, 2)
    view = torch.zeros((cl.xyz.shape[0], 3), device=dev)
    try:
        run(lib_path, dev, cl, cam, 0, dpix, dL_dcolor_view=view)
    except capi.GsrError as e:
        assert e.status == GSR_ERR_UNSUPPORTED, e
    else:
        raise AssertionError("dL_dmean2D_abs together with dL_dcolor_view was accepted")
    # the separate statistics pass validates its arguments like gsr_densify_stats
    lib = capi.load(lib_path)
    assert lib.gsr_densify_stats_abs(0, None, None, None, None, None, None) == 0
    assert lib.gsr_densify_stats_abs(4, None, None, None, None, None, None) == -1


def check_bound_only(lib_path, dev, cl, cam, flags, seed=0):
    """(b) and (d) at a BASELINE shape: no per-pixel reference.  The one place where the bound is not asserted for every component:
    REL_BAR of the values themselves for all but at most CANCEL_CAP of the components, and REL_BAR of the magnitude of their terms
    (term_scale) for those few -- one- and two-pixel Gaussians whose two terms cancel (module docstring)."""
    rng = np.random.default_rng(seed)
    dpix = rng.standard_normal((3, cam.H, cam.W)).astype(np.float32)
    out, radii, ab = run(lib_path, dev, cl, cam, flags, dpix)
    a = ab.cpu().numpy()
    vis = radii.cpu().numpy() > 0
    assert np.isfinite(a).all() and not a[~vis].any() and a[vis].any()
    g2d = out[0].cpu().numpy()
    worst = check_bound(a, g2d, term_scale(lib_path, dev, cl, cam, flags, g2d))
    plain, _, _ = run(lib_path, dev, cl, cam, flags, dpix, absgrad=False)
    check_unchanged(out, plain, exact=False)
    return worst
