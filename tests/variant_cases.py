"""Shared walk over the kernel variants of the backward pass for the emulator test (test_variant_dispatch.py) and the GPU test
(test_gpu_variant_dispatch.py): every combination of the optional features of gsr_backward (include/gsr.h) goes through the
C-ABI entry itself -- lib.gsr_backward on a capi.BackwardArgs, so the library decides and not the Python boundary -- and is
either accepted or refused with the status gsr.h names.  The feature suites pin the numbers of the variants; this walk pins the
SELECTION: a launcher that picked a sibling instantiation would write an output nobody asked for, leave one unwritten, or change
an output that the toggled feature must not touch.

Scene: 129 Gaussians (two workgroups of preprocess_bwd_kernel's 128 threads, the second with one live lane; three of
sh_bwd_rows_kernel's 64), a 40 x 24 image (3 x 2 tiles, ragged right and bottom edges), some Gaussians culled, R > 0.
One forward pass per case (rows_ok, antialias, form); the backward pass leaves the forward pass's buffers as it found them, so the
48 combinations of a case share them.

Per case 16 of the 48 combinations are accepted and 32 refused (expected_status; the same at every case)."""
import ctypes as C
import itertools

import numpy as np
import torch

import forward_only_cases as fo
import pose_grad_cases as pg
from photo_slam_amd import capi
from photo_slam_amd import rasterize_points as rp
from photo_slam_amd import scene

P, W, H = 129, 40, 24
BG = np.array([0.2, 0.5, 0.1], np.float32)
GSR_OK, GSR_ERR_UNSUPPORTED = 0, -4
FORMS = ("0", "1")   # GSR_BWD_HALF_TILES: quads / half tiles
# rows_ok -> (active degree, M): [P,16,3] aligned rows at degree 3 (preprocess_bwd_kernel<true> + sh_bwd_rows_kernel); nine
# coefficients at degree 2, a row length for which kernels.h: sh_rows_path is false (preprocess_bwd_kernel<false> alone)
LAYOUTS = {True: (3, 16), False: (2, 9)}
FEATURES = ("depth", "pose", "geom_reg", "absgrad", "factored", "packed")
TOGGLED = ("pose", "absgrad", "packed")
ACCEPTED, REFUSED = 16, 32
REG = dict(w_opacity=1e-3, w_scale=2e-3, w_isotropic=5e-4)


def combinations():
    """the 48 combinations of FEATURES: the full product, packed with factored only (a message rides next to dL_dcolor_view)"""
    out = [dict(zip(FEATURES, bits)) for bits in itertools.product((False, True), repeat=len(FEATURES))]
    return [c for c in out if c["factored"] or not c["packed"]]


def expected_status(c):
    """include/gsr.h: geom_reg, the pose outputs and dL_dmean2D_abs each are GSR_ERR_UNSUPPORTED together with dL_dcolor_view /
    packed_view (the multi-GPU exchange), and geom_reg also with the pose outputs; everything else is accepted"""
    exchange = c["factored"] or c["packed"]
    if c["geom_reg"] and (exchange or c["pose"]):
        return GSR_ERR_UNSUPPORTED
    if (c["pose"] or c["absgrad"]) and exchange:
        return GSR_ERR_UNSUPPORTED
    return GSR_OK


def key(c):
    return tuple(c[f] for f in FEATURES)


class Forward:
    """one training forward pass of the scene and what every backward call of a case shares"""

    def __init__(self, lib_path, dev, rows_ok, antialias):
        self.lib_path, self.dev = lib_path, dev
        self.lib = capi.load(lib_path)
        self.degree, self.M = LAYOUTS[rows_ok]
        self.raw = capi.ANTIALIAS if antialias else 0
        cl = scene.make_cloud(P, W, H, 30, 30, seed=3)   # (the seed: Gaussian 128, the second workgroup's one lane, is visible)
        self.cam = cam = cl.cameras[0]
        sh = fo._t(cl.get_features()[:, :self.M], dev)
        self.a = a = dict(fo.inputs(cl, cam, BG, dev, sh=sh), degree=self.degree)
        rng = np.random.default_rng(7)
        self.dpix = fo._t(rng.standard_normal((3, H, W)).astype(np.float32), dev)
        self.dD = fo._t(rng.standard_normal((H, W)).astype(np.float32), dev)
        prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
        try:
            self.R, _, self.radii, self.geom, self.binning, self.img = rp.RasterizeGaussiansCUDA(**a, raw_params=self.raw)
            self.capacity = (P + 3) & ~3
            self.plan = rp.packViewPlan(self.radii, self.capacity,
                                        message=torch.zeros(rp.packedViewWords(P, self.capacity), dtype=torch.int32, device=dev))
        finally:
            rp._LIB_OVERRIDE = prev
        vis = self.radii.cpu().numpy() > 0
        # the shapes the scene is there for: a ragged tile grid, visible and culled Gaussians inside one wave, instances to blend
        assert W % 16 and H % 16 and self.R > 0
        assert vis[:64].any() and not vis[:64].all() and vis[128], "vis must differ inside a wave, and the last lane be live"
        assert rows_ok == (3 * self.M == 48 and sh.data_ptr() % 16 == 0)

    def backward(self, c):
        """gsr_backward with the features of c; returns (status, outputs by name, the packed message before the call or None).
        Every float output holds NaN before the call."""
        dev, M = self.dev, self.M
        nan = lambda *shape: torch.full(shape, float("nan"), device=dev)
        out = dict(dL_dmean2D=nan(P, 3), dL_dconic=nan(P, 2, 2), dL_dopacity=nan(P, 1), dL_dcolor=nan(P, 3), dL_dmean3D=nan(P, 3),
                   dL_dcov3D=nan(P, 6), dL_dscale=nan(P, 3), dL_drot=nan(P, 4))
        a, x = capi.BackwardArgs(), self.a
        a.P, a.D, a.M, a.R, a.width, a.height = P, self.degree, M, int(self.R), W, H
        a.scale_modifier, a.tan_fovx, a.tan_fovy, a.raw_params = 1.0, float(self.cam.tanfovx), float(self.cam.tanfovy), self.raw
        for name, t in (("background", x["background"]), ("means3D", x["means3D"]), ("shs", x["sh"]), ("scales", x["scales"]),
                        ("rotations", x["rotations"]), ("viewmatrix", x["viewmatrix"]), ("projmatrix", x["projmatrix"]),
                        ("campos", x["campos"]), ("radii", self.radii), ("geom_buffer", self.geom),
                        ("binning_buffer", self.binning), ("image_buffer", self.img), ("dL_dpix", self.dpix)):
            setattr(a, name, t.data_ptr())
        if c["factored"]:
            out["dL_dcolor_view"] = nan(P, 3)
            a.dL_dcolor_view = out["dL_dcolor_view"].data_ptr()
        else:
            out["dL_dsh"] = nan(P, M, 3)
        plan = None
        if c["packed"]:
            plan, out["packed_view"] = self.plan, self.plan.clone()
            a.packed_view, a.packed_capacity_rows = out["packed_view"].data_ptr(), self.capacity
        if c["depth"]:
            a.dL_ddepth = self.dD.data_ptr()
        keep = []
        if c["pose"]:
            out["pose"] = nan(35)
            keep.append(torch.empty(int(self.lib.gsr_pose_grad_scratch_bytes(P)), dtype=torch.uint8, device=dev))
            p0 = out["pose"].data_ptr()
            a.dL_dviewmatrix, a.dL_dprojmatrix, a.dL_dcampos, a.pose_scratch = p0, p0 + 64, p0 + 128, keep[-1].data_ptr()
        if c["geom_reg"]:
            out["reg_loss"] = nan(3)
            keep.append(torch.empty(int(self.lib.gsr_geom_reg_scratch_bytes(P)), dtype=torch.uint8, device=dev))
            gr = capi.GeomReg(REG["w_opacity"], REG["w_scale"], REG["w_isotropic"], out["reg_loss"].data_ptr(), keep[-1].data_ptr())
            a.geom_reg = C.pointer(gr)
        if c["absgrad"]:
            out["dL_dmean2D_abs"] = nan(P, 2)
        for name in ("dL_dmean2D", "dL_dconic", "dL_dopacity", "dL_dcolor", "dL_dmean3D", "dL_dcov3D", "dL_dsh", "dL_dscale",
                     "dL_drot", "dL_dmean2D_abs"):
            if name in out:
                setattr(a, name, out[name].data_ptr())
        status = int(self.lib.gsr_backward(C.byref(a), rp._stream_ptr(x["means3D"])))
        if dev.type != "cpu":
            torch.cuda.synchronize()
        return status, out, plan


def _same(what, name, x, y, exact):
    if name == "pose":
        # (the 35 floats are sums with cancellation: on the device the rule of pose_grad_cases.pose_same_or_close, per array)
        for k, (lo, hi) in enumerate(((0, 16), (16, 32), (32, 35))):
            if exact or bool(y[lo:hi].any()):
                pg.same_or_rerun_close(f"{what}: {name}[{lo}:{hi}]", x[lo:hi], y[lo:hi], exact)
    elif x.numel():
        pg.same_or_rerun_close(f"{what}: {name}", x, y, exact)


def walk(lib_path, dev, rows_ok, antialias, exact):
    """all 48 combinations of one case: the status of each; accepted: every requested output written and finite; refused: every
    output as the test filled it; pose, absgrad and packed each leave every other output as the combination without it has it
    (absgrad_cases.check_unchanged's sense: bit for bit with `exact`, the rerun tolerance of the device otherwise).  Returns the
    number of accepted combinations."""
    fw = Forward(lib_path, dev, rows_ok, antialias)
    results = {}
    for c in combinations():
        status, out, plan = fw.backward(c)
        assert status == expected_status(c), (c, status)
        for name, t in out.items():
            if status != GSR_OK:
                untouched = torch.equal(t, plan) if name == "packed_view" else bool(torch.isnan(t).all())
                assert untouched, f"{c}: refused, but {name} was written"
            elif name != "packed_view":
                assert bool(torch.isfinite(t).all()), f"{c}: {name} has elements that are not written or not finite"
        if status == GSR_OK:
            if c["packed"]:
                assert not torch.equal(out["packed_view"], plan), f"{c}: the message was not written"
            results[key(c)] = out
    for k, out in results.items():
        c = dict(zip(FEATURES, k))
        for f in TOGGLED:
            if c[f]:
                base = results[key(dict(c, **{f: False}))]   # (accepted: the rules only ever refuse MORE features)
                for name, y in base.items():
                    _same(f"{c} against the call without {f}", name, out[name], y, exact)
    assert len(results) == ACCEPTED and len(combinations()) == ACCEPTED + REFUSED
    return len(results)
