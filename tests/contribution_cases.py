"""Shared checks of the per-Gaussian contribution statistics (GSR_CONTRIBUTION, include/gsr.h: out_weight_sum / out_weight_max /
out_n_touched of gsr_forward_args) for the emulator tests (test_contribution.py) and the GPU tests (test_gpu_contribution.py).

Nothing in the reference corresponds to the statistics; the CPU oracle serves unchanged:
  weight_sum   the blend is linear in the colours: a render with colours (1, 1, 1) and the oracle's backward pass with
               dL_dpix = (w, 0, 0) leaves sum_p w alpha T in dL_dcolors[:, 0].
  weight_max, n_touched   a float32 numpy re-walk of the oracle's render_tile_fwd over the oracle's lists, one tile at a time.  For
               every Gaussian it yields solid (pixels with w != 0 that blend it on every walk the device may take, with the
               oracle's T), maybe (pixels with w != 0 that MAY blend it, or blend it with another T: decisions inside rounding noise
               -- the oracle's three tests and their bands -- may fall either way on the device) and the maximum of w alpha T over
               the pixels the oracle's decisions blend.  Only pixels the oracle flags fragile hold such decisions (asserted).  A
               fragile pixel is walked with an interval for T: a Gaussian in front of its first uncertain decision is solid, one
               behind a stop that every possible walk takes is not blended at all, the ones in between are maybe.  (Counting
               every Gaussian a fragile pixel's tile lists as maybe, wherever it sits in the walk, is sound too but leaves 80 % of
               the visible Gaussians of the saturated k = 0.6 cloud out of the exact comparisons; this leaves 14-20 %.)
Inputs: scene.make_cloud(3000, 229, 131, 183.2, 183.2, seed=1, scale_k=k, n_views=2), k = 0.2 and 0.6 -- 15 x 9 tiles with partial
quads on the right and bottom edges, lists of up to 536 entries, 211 Gaussians over more than 64 tiles, 23 214 saturated pixels at
k = 0.6, P no multiple of 64."""
import copy

import numpy as np
import torch

import depth_alpha_cases as da
import forward_only_cases as fo
import parity
from photo_slam_amd import capi
from photo_slam_amd import rasterize_points as rp
from photo_slam_amd import scene

BG = np.array([0.2, 0.5, 0.1], np.float32)
W, H, FX, P = 229, 131, 183.2, 3000
WEIGHT_MAX_TOL = 2e-5    # absolute: the parity suite's final_T bar is 1e-5 absolute, and alpha <= 0.99 carries a relative error of that order
MAYBE_MAX_FRAC = 0.40    # condition on the inputs: Gaussians with a fragile pixel among the visible ones (the reference alone: 18-20 %)

_clouds, _refs = {}, {}


def cloud(k):
    if k not in _clouds:
        _clouds[k] = scene.make_cloud(P, W, H, FX, FX, seed=1, scale_k=k, n_views=2)
    return _clouds[k]


def weight_map(seed=0):
    """random w in [0, 1) with 30 % of the pixels set to 0"""
    rng = np.random.default_rng(100 + seed)
    w = rng.random((H, W)).astype(np.float32)
    w[rng.random((H, W)) < 0.3] = 0.0
    return w


def reference(oracle, k, weighted, view=0):
    """dict(sum, max, solid, maybe, radii) of the oracle for the cloud's view (computed once, shared, never modified)"""
    key = (k, weighted, view)
    if key in _refs:
        return _refs[key]
    cl = cloud(k)
    cam = cl.cameras[view]
    w = weight_map() if weighted else np.ones((H, W), np.float32)
    a = fo.inputs(cl, cam, BG, torch.device("cpu"))
    res, _, radii = da.oracle_forward(oracle, a, cl, cam, np.ones((P, 3), np.float32), np.zeros(3, np.float32))
    dp = np.zeros((3, H, W), np.float32)
    dp[0] = w
    wsum = oracle.backward(res, dp)["dL_dcolors"][:, 0].astype(np.float64)
    solid, maybe, wmax = np.zeros(P, np.int64), np.zeros(P, np.int64), np.zeros(P, np.float32)
    f32 = np.float32
    gx, gy = res.grid
    m2d, co = res.means2D, res.conic_opacity
    for ty in range(gy):
        for tx in range(gx):
            rs, re = (int(v) for v in res.ranges[ty * gx + tx])
            if re <= rs:
                continue
            ys, xs = np.meshgrid(np.arange(ty * 16, min(H, ty * 16 + 16)), np.arange(tx * 16, min(W, tx * 16 + 16)), indexing="ij")
            ys, xs = ys.reshape(-1), xs.reshape(-1)
            pxf, pyf = xs.astype(f32), ys.astype(f32)
            wv = w[ys, xs]
            counted = wv != 0
            # A fragile pixel is walked with an INTERVAL [T_lo, T_hi] for the transmittance the device may hold, split wherever a
            # decision sits inside rounding noise (the oracle's own three tests and their bands): an uncertain skip leaves T_hi
            # alone and lowers T_lo; a stop test is certain only if it falls the same way for the whole interval.  may_done: some
            # of these walks have stopped; done_all: all of them have -- behind that no Gaussian is blended whatever the device did.
            T_lo, T_hi = np.ones(xs.size, f32), np.ones(xs.size, f32)
            may_done, done_all = np.zeros(xs.size, bool), np.zeros(xs.size, bool)
            T = np.ones(xs.size, f32)
            done = np.zeros(xs.size, bool)
            for e in range(rs, re):
                g = int(res.point_list[e])
                c0, c1, c2, op = (f32(v) for v in co[g])
                dx, dy = f32(m2d[g, 0]) - pxf, f32(m2d[g, 1]) - pyf
                power = f32(-0.5) * (c0 * dx * dx + c2 * dy * dy) - c1 * dx * dy
                mag = np.abs(f32(0.5) * c0 * dx * dx) + np.abs(f32(0.5) * c2 * dy * dy) + np.abs(c1 * dx * dy)
                alpha = np.minimum(f32(0.99), op * np.exp(np.minimum(power, f32(0))))
                # the oracle's walk
                skip = (power > 0) | (alpha < f32(1.0 / 255.0))
                test_T = T * (f32(1) - alpha)
                stop = ~done & ~skip & (test_T < f32(0.0001))
                blend = ~done & ~skip & ~stop
                # every walk the device may take
                unsure_skip = ((np.abs(power) <= f32(1e-5) * mag + f32(1e-30)) & (op >= f32(1.0 / 255.0 * 0.999))) | \
                    (~(power > 0) & (np.abs(alpha * f32(255.0) - f32(1.0)) <= f32(1e-4)))
                can_pass, can_skip = ~skip | unsure_skip, skip | unsure_skip   # (past the skips / skipped)
                lo, hi = T_lo * (f32(1) - alpha), T_hi * (f32(1) - alpha)
                must_stop = hi * f32(10000.0) < f32(1.0 - 2e-4)
                can_stop = lo * f32(10000.0) <= f32(1.0 + 2e-4)
                can_blend = ~done_all & can_pass & ~must_stop
                exact = ~may_done & (T_lo == T_hi) & ~unsure_skip & ~(can_stop & ~must_stop)   # one walk, the oracle's, with the oracle's T
                assert not np.any(blend & ~can_blend)
                solid[g] += int((blend & exact & counted).sum())
                maybe[g] += int((can_blend & ~(blend & exact) & counted).sum())
                if blend.any():
                    wmax[g] = max(wmax[g], f32((alpha * T * wv)[blend].max()))
                live = ~done_all
                T_hi = np.where(live & can_pass & ~can_skip & ~can_stop, hi, T_hi)       # surely blended: the upper end moves too
                T_lo = np.where(live & can_blend, lo, T_lo)
                done_all |= live & ~can_skip & must_stop
                may_done |= live & can_pass & can_stop
                T = np.where(blend, test_T, T)
                done |= stop
            unsure_px = may_done & ~done_all | (T_lo != T_hi)
            assert not np.any(unsure_px & (res.fragile[ys, xs] == 0)), "an uncertain decision on a pixel the oracle did not flag fragile"
            assert np.allclose(T, res.final_T[ys, xs], rtol=1e-5, atol=0), "the re-walk and the oracle disagree on final T"
    _refs[key] = dict(sum=wsum, max=wmax, solid=solid, maybe=maybe, radii=radii.copy())
    return _refs[key]


def check_input_condition(oracle, k, weighted):
    """the condition check 1 puts on its inputs: the Gaussians with a fragile pixel (maybe > 0), which the exact comparisons of
    n_touched and weight_max leave out, are at most 40 % of the visible ones"""
    ref = reference(oracle, k, weighted)
    vis = ref["radii"] > 0
    frac = float((ref["maybe"][vis] > 0).mean())
    print(dict(k=k, weighted=weighted, visible=int(vis.sum()), maybe_frac=frac))
    assert frac <= MAYBE_MAX_FRAC, frac


def stats(lib_path, a, flags, w=None, which=(True, True, True), accumulate=False, into=None, depth=False, workspace=None):
    """one gsr_forward with the statistics through the Python boundary: dict(R, color, radii, sum, max, cnt, depth, alpha, bufs).
    into: (sum, max, cnt) tensors to use (accumulate / prefilled); otherwise filled with garbage first -- every element must be
    written"""
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        dev = a["means3D"].device
        n = a["means3D"].shape[0]
        if into is None:
            into = (torch.full((n,), -3.5, device=dev), torch.full((n,), -2.5, device=dev), torch.full((n,), -9, dtype=torch.int32, device=dev))
        s, m, c = (t if use else None for t, use in zip(into, which))
        d = torch.full((a["image_height"], a["image_width"]), -7.0, device=dev) if depth else None
        al = torch.full((a["image_height"], a["image_width"]), -7.0, device=dev) if depth else None
        R, color, radii, g, b, i = rp.RasterizeGaussiansCUDA(**a, raw_params=flags, out_depth=d, out_alpha=al, workspace=workspace,
                                                             pixel_weight=None if w is None else fo._t(w, dev), out_weight_sum=s,
                                                             out_weight_max=m, out_n_touched=c, contribution_accumulate=accumulate)
        if dev.type != "cpu":
            torch.cuda.synchronize()
        return dict(R=R, color=color, radii=radii, sum=s, max=m, cnt=c, depth=d, alpha=al, bufs=(g, b, i))
    finally:
        rp._LIB_OVERRIDE = prev


def _same(x, y, names=("sum", "max", "cnt")):
    return all(torch.equal(x[n], y[n]) for n in names)


def check_reference(lib_path, dev, oracle, k, weighted, flags):
    """check 1: the three statistics against the reference.  Returns the report."""
    cl = cloud(k)
    ref = reference(oracle, k, weighted)
    w = weight_map() if weighted else None
    r = stats(lib_path, fo.inputs(cl, cl.cameras[0], BG, dev), flags, w=w)
    radii = r["radii"].cpu().numpy()
    assert np.array_equal(radii, ref["radii"])
    vis = radii > 0
    s, m, c = r["sum"].cpu().numpy(), r["max"].cpu().numpy(), r["cnt"].cpu().numpy().astype(np.int64)
    assert np.isfinite(s).all() and np.isfinite(m).all()
    rep = dict(visible=int(vis.sum()), maybe_frac=float((ref["maybe"][vis] > 0).mean()), sum_rel_l1=parity.rel_l1(s, ref["sum"]))
    assert rep["sum_rel_l1"] <= parity.GRAD_REL_L1_TOL, rep
    e = parity.row_errors(s[:, None], ref["sum"][:, None])[vis]
    row = dict(p9999=float(np.quantile(e, 0.9999)), max=float(e.max()), beyond=int((e > parity.ROW_OUTLIER).sum()))
    rep["rows_sum"] = row
    assert row["p9999"] <= parity.ROW_P9999_TOL and row["max"] <= parity.ROW_MAX_TOL, row
    assert row["beyond"] <= max(3, parity.ROW_OUTLIER_FRAC * e.size), row
    sure = ref["maybe"] == 0
    assert np.array_equal(c[sure], ref["solid"][sure]), int((c[sure] != ref["solid"][sure]).sum())
    assert np.all(c >= ref["solid"]) and np.all(c <= ref["solid"] + ref["maybe"])
    rep["max_abs_err"] = float(np.abs(m[sure] - ref["max"][sure]).max())
    print(rep)
    assert rep["max_abs_err"] <= WEIGHT_MAX_TOL, rep
    return rep


def check_invariants(lib_path, dev, k, flags):
    """check 2: what must hold without any reference"""
    cl = cloud(k)
    a = fo.inputs(cl, cl.cameras[0], BG, dev)
    r = stats(lib_path, a, flags, depth=True)
    s, m, c = (r[n].cpu().numpy().astype(np.float64) for n in ("sum", "max", "cnt"))
    radii = r["radii"].cpu().numpy()
    alpha_total = float(r["alpha"].cpu().numpy().astype(np.float64).sum())
    rep = dict(sum_total=float(s.sum()), alpha_total=alpha_total, visible=int((radii > 0).sum()),
               visible_untouched=int(((radii > 0) & (c == 0)).sum()))
    print(rep)
    assert abs(rep["sum_total"] - alpha_total) <= 1e-5 * alpha_total, rep
    assert np.array_equal(c == 0, s == 0) and np.array_equal(c == 0, m == 0)
    assert np.all(m <= 0.99) and np.all(m >= 0) and np.all(c >= 0)
    assert np.all(m <= s) and np.all(s <= c * m * (1 + 1e-6))
    assert not s[radii == 0].any() and not m[radii == 0].any() and not c[radii == 0].any()
    assert rep["visible_untouched"] >= 1, rep
    wmap = weight_map(1)
    rw = stats(lib_path, a, flags, w=wmap)
    sw, mw, cw = (rw[n].cpu().numpy().astype(np.float64) for n in ("sum", "max", "cnt"))
    assert np.all(mw <= 0.99 * float(wmap.max())) and np.all(cw <= c) and np.all(sw <= s)
    assert np.array_equal(cw == 0, sw == 0) and np.array_equal(cw == 0, mw == 0)
    assert np.all(mw <= sw) and np.all(sw <= cw * mw * (1 + 1e-6))
    return rep


def check_bit_identity(lib_path, dev, k, weighted=True):
    """check 3: the outputs of the render are those of the call without the bit; any subset of the statistics equals the full call;
    forward-only equals the training form; two runs and both binning arrangements give the same bits; GSR_CULL_EMPTY_TILES leaves
    counts and maxima equal and the sums to 1e-6 per row"""
    cl = cloud(k)
    a = fo.inputs(cl, cl.cameras[0], BG, dev)
    w = weight_map(2) if weighted else None
    full = {}
    for flags in (32, 64):
        R0, c0, r0, d0, al0, _ = da.render(lib_path, a, flags)
        f = full[flags] = stats(lib_path, a, flags, w=w, depth=True)
        assert f["R"] == R0 and torch.equal(f["color"], c0) and torch.equal(f["radii"], r0)
        assert torch.equal(f["depth"], d0) and torch.equal(f["alpha"], al0), "the statistics changed the depth or alpha map"
        again = stats(lib_path, a, flags, w=w)
        assert _same(f, again) and torch.equal(again["color"], c0), "two runs differ"
        for which in ((True, False, False), (False, True, True)) if flags == 32 else ((False, False, True), (True, True, False)):
            part = stats(lib_path, a, flags, w=w, which=which)
            assert _same(f, part, [n for n, use in zip(("sum", "max", "cnt"), which) if use]) and torch.equal(part["color"], c0)
        fwd = stats(lib_path, a, flags | fo.FORWARD_ONLY, w=w, depth=True)
        assert _same(f, fwd) and torch.equal(fwd["color"], c0) and torch.equal(fwd["depth"], d0) and torch.equal(fwd["alpha"], al0)
        for extra in ((8,) if flags == 32 else (8 | fo.FORWARD_ONLY,)):
            cu = stats(lib_path, a, flags | extra, w=w)
            assert torch.equal(cu["color"], c0) and _same(f, cu, ("max", "cnt"))
            x, y = cu["sum"].cpu().numpy().astype(np.float64), f["sum"].cpu().numpy().astype(np.float64)
            assert np.all(np.abs(x - y) <= 1e-6 * np.abs(y))
    assert _same(full[32], full[64]), "the two binning arrangements differ"


def check_accumulate(lib_path, dev, k, flags):
    """check 4: views 0 and 1 accumulated equal a + b, maximum(a, b), a + b of the separate calls, bit for bit"""
    cl = cloud(k)
    w = weight_map(3)
    a0, a1 = (fo.inputs(cl, cam, BG, dev) for cam in cl.cameras[:2])
    x, y = stats(lib_path, a0, flags, w=w), stats(lib_path, a1, flags | fo.FORWARD_ONLY, w=w)   # (garbage-prefilled: mode 0 writes everything)
    assert float(x["sum"].min()) >= 0 and float(x["max"].min()) >= 0 and int(x["cnt"].min()) >= 0
    assert not torch.equal(x["cnt"], y["cnt"])
    n = cl.xyz.shape[0]
    acc = (torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))
    stats(lib_path, a0, flags, w=w, accumulate=True, into=acc)
    stats(lib_path, a1, flags | fo.FORWARD_ONLY, w=w, accumulate=True, into=acc)
    assert torch.equal(acc[0], x["sum"] + y["sum"]) and torch.equal(acc[1], torch.maximum(x["max"], y["max"]))
    assert torch.equal(acc[2], x["cnt"] + y["cnt"])


def check_backward_after(lib_path, dev, k, flags, exact):
    """check 5: gsr_backward on the buffers of a training-form forward with the bit gives the gradients of a plain forward"""
    cl = cloud(k)
    cam = cl.cameras[0]
    a = fo.inputs(cl, cam, BG, dev)
    dpix = fo._t(np.random.default_rng(4).standard_normal((3, H, W)).astype(np.float32), dev)
    plain, _ = da.backward(lib_path, a, cam, flags, dpix, None, None)
    r = stats(lib_path, a, flags, w=weight_map(4))
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        g, b, i = r["bufs"]
        out = rp.RasterizeGaussiansBackwardCUDA(a["background"], a["means3D"], r["radii"], a["colors"], a["scales"], a["rotations"], 1.0,
                                                a["cov3D_precomp"], a["viewmatrix"], a["projmatrix"], cam.tanfovx, cam.tanfovy, dpix,
                                                a["sh"], 3, a["campos"], g, r["R"], b, i)
        if dev.type != "cpu":
            torch.cuda.synchronize()
    finally:
        rp._LIB_OVERRIDE = prev
    checked = 0
    for name, x, y in zip(da.GRAD_NAMES, plain, out):
        if x is None or x.numel() == 0:
            continue
        checked += 1
        if exact:
            assert torch.equal(x, y), name
        else:
            assert parity.rel_l1(y.cpu().numpy(), x.cpu().numpy()) <= 1e-5, name
    assert checked >= 6 and float(plain[3].abs().sum()) > 0


def check_options(lib_path, dev):
    """the bit with GSR_ANTIALIAS, GSR_RAW_*, colors_precomp and cov3D_precomp: the render unchanged, the invariants hold, and the
    statistics do not depend on the colours"""
    cl = cloud(0.2)
    cam = cl.cameras[0]
    base = stats(lib_path, fo.inputs(cl, cam, BG, dev), 32)
    for kw, flags in ((dict(use_colors_precomp=True), 32), (dict(use_cov3D_precomp=True), 64), ({}, 32 | capi.ANTIALIAS)):
        a = fo.inputs(cl, cam, BG, dev, **kw)
        _, c0, r0, _, _, _ = da.render(lib_path, a, flags, depth=False, alpha=False)
        r = stats(lib_path, a, flags, depth=True)
        assert torch.equal(r["color"], c0) and torch.equal(r["radii"], r0)
        s, al = float(r["sum"].double().sum()), float(r["alpha"].double().sum())
        assert abs(s - al) <= 1e-5 * al
        if "use_colors_precomp" in kw:
            assert _same(base, r), "the statistics depend on the colours"
    a = fo.inputs(cl, cam, BG, dev)
    a.update(opacity=fo._t(cl.opacity, dev), scales=fo._t(cl.scaling, dev), rotations=fo._t(cl.rotation, dev))
    raw = stats(lib_path, a, 7 | 32)
    # (the activations are then taken in-kernel: equal to rounding)
    assert torch.equal(raw["radii"], base["radii"])
    assert parity.rel_l1(raw["sum"].cpu().numpy(), base["sum"].cpu().numpy()) <= parity.GRAD_REL_L1_TOL


def check_argument_errors(lib_path, dev):
    """check 6: the bit without an output, an output without the bit: GSR_ERR_INVALID_ARG; wrong dtype / shape raise on the host;
    P == 0 leaves the outputs untouched"""
    import pytest
    cl = cloud(0.2)
    a = fo.inputs(cl, cl.cameras[0], BG, dev)
    n = cl.xyz.shape[0]
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        with pytest.raises(capi.GsrError) as e:
            rp.RasterizeGaussiansCUDA(**a, raw_params=32 | capi.CONTRIBUTION)
        assert e.value.status == -1
        bit, capi.CONTRIBUTION = capi.CONTRIBUTION, 0   # (the host then passes the outputs without setting the bit)
        try:
            with pytest.raises(capi.GsrError) as e:
                rp.RasterizeGaussiansCUDA(**a, raw_params=32, out_weight_sum=torch.zeros(n, device=dev))
            assert e.value.status == -1
        finally:
            capi.CONTRIBUTION = bit
        for kw in (dict(out_weight_sum=torch.zeros(n, dtype=torch.float64, device=dev)), dict(out_weight_max=torch.zeros(n + 1, device=dev)),
                   dict(out_n_touched=torch.zeros(n, device=dev)), dict(out_n_touched=torch.zeros((n, 1), dtype=torch.int32, device=dev)),
                   dict(out_weight_sum=torch.zeros(2 * n, device=dev)[::2]),
                   dict(out_weight_sum=torch.zeros(n, device=dev), pixel_weight=torch.zeros((W, H), device=dev)),
                   dict(pixel_weight=torch.zeros((H, W), device=dev)), dict(contribution_accumulate=True)):
            with pytest.raises(RuntimeError):
                rp.RasterizeGaussiansCUDA(**a, raw_params=32, **kw)
        for key in ("means3D", "opacity", "scales", "rotations", "sh"):
            a[key] = a[key][:0]
        keep = torch.full((0,), 1.0, device=dev)
        R = rp.RasterizeGaussiansCUDA(**a, raw_params=32, out_weight_sum=keep)[0]
        assert R == 0
    finally:
        rp._LIB_OVERRIDE = prev


# ---- check 7: the hosts, on the k = 0.6 cloud with its two cameras ----------------------------------------------------------
# The pruning threshold: 1/255 does not hold the render bar on this cloud -- nearly every pixel saturates, most blended weights
# alpha T lie below 1/255, and 2 011 of the 2 081 Gaussians the two keyframes see go; many small terms add up.  Halved until the
# ORACLE's renders of the pruned cloud hold parity.RGB_L1_TOL against those of the full cloud (mean absolute difference, views 0
# and 1): 1/255: 1.7e-3 / 1.7e-3;  /2: 4.9e-4 / 9.4e-4;  /4: 1.9e-4 / 3.7e-4;  /8: 6.6e-5 / 1.6e-4;  /16: 3.9e-5 / 6.8e-5 (1 898
# removed) -- the first that holds.
PRUNE_THRESHOLD = 1.0 / 255.0 / 16.0


def _direct_accumulated(tensors, cl, dev, weights, cull=False, antialiasing=False):
    """the accumulated direct calls score_contribution must equal: (sum, max, cnt, views_seen) of the raw model tensors (xyz,
    opacity, scaling, rotation) over the cloud's cameras.  The statistics do not depend on the colours: ones stand in."""
    xyz, opacity, scaling, rotation = (t.detach() for t in tensors)
    n = xyz.shape[0]
    acc = (torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))
    seen = torch.zeros(n, dtype=torch.int32, device=dev)
    empty = torch.empty(0, device=dev)
    for cam, w in zip(cl.cameras, weights):
        t = lambda a: fo._t(a, dev)
        _, _, radii, _, _, _ = rp.RasterizeGaussiansCUDA(
            torch.zeros(3, device=dev), xyz, torch.ones((n, 3), device=dev), opacity, scaling, rotation, 1.0, empty, t(cam.viewmatrix),
            t(cam.projmatrix), cam.tanfovx, cam.tanfovy, cam.H, cam.W, empty, 3, t(cam.campos), False,
            raw_params=7 | fo.FORWARD_ONLY | (8 if cull else 0), antialiasing=antialiasing, pixel_weight=w, out_weight_sum=acc[0],
            out_weight_max=acc[1], out_n_touched=acc[2], contribution_accumulate=True)
        seen += (radii > 0).to(torch.int32)
    return acc + (seen,)


def _host_weights(dev):
    return [fo._t(weight_map(5), dev), None]


def check_host_python(dev, exact=True, train_steps=1):
    """TrainStep.score_contribution equals the accumulated direct calls and touches nothing (parameters, Adam moments, row_step,
    training workspace; a train step behind it equals one without it); rp.lastForwardOnly() == 1; prune_uncontributing removes
    exactly the rows its score names, keeps the unseen ones and leaves the renders within parity.RGB_L1_TOL; a train step runs
    afterwards on an optimizer state of the new length; covisibility.  Returns the positions after pruning."""
    import pose_grad_cases as pg
    cl = cloud(0.6)
    kfs, gts, _, mask = da.train_data(cl, dev)
    weights = _host_weights(dev)
    finals = []
    for score in (True, False):
        g, ts = da._python_trainer(cl, dev)
        for it in range(train_steps):   # (optimizer state, lazily stepped SH rows and the training workspace come to life)
            ts.trainForOneIteration(kfs[it % 2], gts[it % 2], mask, sync_loss=False)
        if score:
            before = pg._snapshot(g, ts)
            got = ts.score_contribution(kfs, weights)
            assert rp.lastForwardOnly() == 1
            after = pg._snapshot(g, ts)
            assert len(before) == len(after) and all(torch.equal(x, y) for x, y in zip(before, after)), "scoring touched the model"
            assert g.optimizer_.lazy_view_args(1) is not None, "the model has no lazily stepped SH rows: the read-only path was not exercised"
            want = _direct_accumulated(g.params_raw()[:1] + g.params_raw()[2:], cl, dev, weights)
            for name, x, y in zip(("weight_sum", "weight_max", "n_touched", "views_seen"), got, want):
                assert x.dtype == y.dtype and torch.equal(x, y), name
            assert all(not t.requires_grad for t in got)
            assert int(got[2].sum()) > 0 and int(got[3].max()) == 2
        ts.trainForOneIteration(kfs[0], gts[0], mask, sync_loss=False)
        g.sync_features()
        finals.append([p.detach().clone() for p in g.params()])
    for x, y in zip(*finals):
        if exact:
            assert torch.equal(x, y), "a train step behind score_contribution differs from one without it"
        else:
            assert parity.rel_l1(x.cpu().numpy(), y.cpu().numpy()) <= 1e-3
    # options of the object: cull_empty_tiles_ / antialiasing_ are honoured
    g, ts = da._python_trainer(cl, dev)
    ts.cull_empty_tiles_, ts.antialiasing_ = True, True
    got = ts.score_contribution(kfs)
    want = _direct_accumulated(g.params_raw()[:1] + g.params_raw()[2:], cl, dev, [None, None], cull=True, antialiasing=True)
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    plain = _direct_accumulated(g.params_raw()[:1] + g.params_raw()[2:], cl, dev, [None, None])
    assert not torch.equal(got[0], plain[0]), "antialiasing_ did not reach the scoring renders"
    # covisibility
    a = ts.score_contribution(kfs[:1])[2]
    b = ts.score_contribution(kfs[1:])[2]
    assert ts.covisibility(a, a) == 1.0 and 0.0 < ts.covisibility(a, b) < 1.0
    assert ts.covisibility(torch.zeros_like(a), torch.zeros_like(a)) == 0.0
    # pruning
    g, ts = da._python_trainer(cl, dev)
    _, wmax, _, seen = ts.score_contribution(kfs)
    expect = (seen >= 1) & (wmax < PRUNE_THRESHOLD)
    assert int(expect.sum()) > 0 and int((seen == 0).sum()) > 0 and not bool((expect & (seen == 0)).any())
    rows = [p.detach().clone() for p in g.params()]
    views = [ts.render_view(kf).clone() for kf in kfs]
    n = ts.prune_uncontributing(kfs, PRUNE_THRESHOLD)
    assert n == int(expect.sum()) and g.xyz_.shape[0] == rows[0].shape[0] - n
    for p, old in zip(g.params(), rows):
        assert torch.equal(p.detach(), old[~expect]), "prune_uncontributing removed other rows than its score names"
    rep = dict(removed=n, of=int(rows[0].shape[0]), unseen_kept=int((seen == 0).sum()))
    for i, kf in enumerate(kfs):
        rep[f"view{i}_mean_abs_diff"] = float((ts.render_view(kf) - views[i]).abs().mean())
    print(rep)
    assert all(rep[f"view{i}_mean_abs_diff"] <= parity.RGB_L1_TOL for i in range(len(kfs))), rep
    ts.trainForOneIteration(kfs[0], gts[0], mask, sync_loss=False)
    for p in g.params_raw():
        st = g.optimizer_.state.get(id(p), {})
        assert st and all(v.shape[0] == p.shape[0] for v in st.values() if torch.is_tensor(v) and v.dim() > 0)
    assert ts.prune_uncontributing(kfs, PRUNE_THRESHOLD, min_views=3) == 0   # (no Gaussian is seen by three of two keyframes)
    ts.world_size_ = 2
    import pytest
    with pytest.raises(RuntimeError):
        ts.prune_uncontributing(kfs, PRUNE_THRESHOLD)
    return rows[0][~expect]


def _stacked_cams(cl, dev):
    t = lambda name: torch.stack([fo._t(getattr(c, name), dev) for c in cl.cameras])
    import math
    c = cl.cameras[0]
    return (t("viewmatrix"), t("projmatrix"), t("campos"), 2 * math.atan(c.tanfovx), 2 * math.atan(c.tanfovy), c.H, c.W)


def check_host_cpp(ops, lib_path, dev, exact=True, train_steps=1):
    """the same on the C++ host (ops trainer_score_contribution / trainer_prune_uncontributing / rasterize_gaussians_contribution /
    covisibility).  Returns the positions after pruning."""
    import pytest
    cl = cloud(0.6)
    kfs, gts, _, mask = da.train_data(cl, dev)
    cams = [da._cam_args(c, dev) for c in cl.cameras]
    stacked = _stacked_cams(cl, dev)
    weights = _host_weights(dev)
    wlist = [w if w is not None else torch.empty(0, device=dev) for w in weights]
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        finals = []
        for score in (True, False):
            h = da._cpp_trainer(ops, cl, dev)
            try:
                for it in range(train_steps):
                    ops.trainer_render_and_backward(h, *cams[it % 2], gts[it % 2], mask)
                    ops.trainer_finish(h)
                if score:
                    before = [t.clone() for t in ops.trainer_state(h)]
                    got = ops.trainer_score_contribution(h, *stacked, wlist)
                    assert rp.lastForwardOnly() == 1
                    after = ops.trainer_state(h)
                    assert len(before) == len(after) and len(before) >= 15
                    assert all(torch.equal(x, y) for x, y in zip(before, after)), "scoreContribution touched the model"
                    xyz, opacity, scaling, rotation = (before[0], before[2], before[3], before[4])
                    want = _direct_accumulated((xyz, opacity, scaling, rotation), cl, dev, weights)
                    for name, x, y in zip(("weight_sum", "weight_max", "n_touched", "views_seen"), got, want):
                        assert x.dtype == y.dtype and torch.equal(x, y), name
                ops.trainer_render_and_backward(h, *cams[0], gts[0], mask)
                ops.trainer_finish(h)
                finals.append([p.detach().clone() for p in ops.trainer_params(h)])
            finally:
                ops.trainer_destroy(h)
        for x, y in zip(*finals):
            assert torch.equal(x, y) if exact else parity.rel_l1(x.cpu().numpy(), y.cpu().numpy()) <= 1e-3
        # pruning
        h = da._cpp_trainer(ops, cl, dev)
        try:
            _, wmax, touched, seen = ops.trainer_score_contribution(h, *stacked, [])
            expect = (seen >= 1) & (wmax < PRUNE_THRESHOLD)
            rows = [p.detach().clone() for p in ops.trainer_params(h)]
            views = [ops.trainer_render_view(h, *c).clone() for c in cams]
            n = ops.trainer_prune_uncontributing(h, *stacked, PRUNE_THRESHOLD, 1)
            assert n == int(expect.sum()) and n > 0
            for p, old in zip(ops.trainer_params(h), rows):
                assert torch.equal(p.detach(), old[~expect])
            for c, v in zip(cams, views):
                assert float((ops.trainer_render_view(h, *c) - v).abs().mean()) <= parity.RGB_L1_TOL
            ops.trainer_render_and_backward(h, *cams[0], gts[0], mask)
            ops.trainer_finish(h)
            state = ops.trainer_state(h)
            assert all(t.shape[0] == rows[0].shape[0] - n for t in state[:5])
            assert ops.trainer_prune_uncontributing(h, *stacked, PRUNE_THRESHOLD, 3) == 0
            one = [x[:1] for x in stacked[:3]] + list(stacked[3:])
            two = [x[1:] for x in stacked[:3]] + list(stacked[3:])
            a, b = ops.trainer_score_contribution(h, *one, [])[2], ops.trainer_score_contribution(h, *two, [])[2]
            assert ops.covisibility(a, a) == 1.0 and 0.0 < ops.covisibility(a, b) < 1.0
            assert ops.covisibility(torch.zeros_like(a), torch.zeros_like(a)) == 0.0
            kept = ops.trainer_params(h)[0].shape[0]
        finally:
            ops.trainer_destroy(h)
        # the extension fields of GaussianRasterizerEx against the Python boundary, and their argument checks
        cam = cl.cameras[0]
        a = fo.inputs(cl, cam, BG, dev)
        r = stats(lib_path, a, fo.FORWARD_ONLY, w=weight_map(5))
        m = cl.xyz.shape[0]
        out = [torch.full((m,), -1.0, device=dev), torch.full((m,), -1.0, device=dev), torch.full((m,), -1, dtype=torch.int32, device=dev)]
        e = torch.empty(0, device=dev)
        args = (a["means3D"], torch.zeros_like(a["means3D"]), a["sh"], e, a["opacity"], a["scales"], a["rotations"], e, a["background"], 1.0,
                a["viewmatrix"], a["projmatrix"], cam.tanfovx, cam.tanfovy, cam.H, cam.W, 3, a["campos"], 0, True)
        color, radii = ops.rasterize_gaussians_contribution(*args, [fo._t(weight_map(5), dev)] + out, False)
        assert torch.equal(color, r["color"]) and torch.equal(radii, r["radii"])
        assert torch.equal(out[0], r["sum"]) and torch.equal(out[1], r["max"]) and torch.equal(out[2], r["cnt"])
        for bad in ([e, out[0].double(), e, e], [e, e, out[1][:-1], e], [e, e, e, out[0]], [fo._t(weight_map(5), dev).t().contiguous(), out[0], e, e],
                    [fo._t(weight_map(5), dev), e, e, e]):
            with pytest.raises(RuntimeError):
                ops.rasterize_gaussians_contribution(*args, bad, False)
        return rows[0][~expect]
    finally:
        rp._LIB_OVERRIDE = prev


def check_hosts_agree(ops, lib_path, dev):
    """the C++ and the Python host remove the same rows"""
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        cl = cloud(0.6)
        kfs, _, _, _ = da.train_data(cl, dev)
        g, ts = da._python_trainer(cl, dev)
        py_score = ts.score_contribution(kfs)
        n_py = ts.prune_uncontributing(kfs, PRUNE_THRESHOLD)
        h = da._cpp_trainer(ops, cl, dev)
        try:
            cpp_score = ops.trainer_score_contribution(h, *_stacked_cams(cl, dev), [])
            n_cpp = ops.trainer_prune_uncontributing(h, *_stacked_cams(cl, dev), PRUNE_THRESHOLD, 1)
            assert all(torch.equal(x, y) for x, y in zip(py_score, cpp_score))
            assert n_py == n_cpp and n_py > 0
            for p, q in zip(g.params(), ops.trainer_params(h)):
                assert torch.equal(p.detach(), q.detach())
        finally:
            ops.trainer_destroy(h)
    finally:
        rp._LIB_OVERRIDE = prev
