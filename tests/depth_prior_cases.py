"""The monocular depth prior (gsr_depth_prior_loss, gsr_depth_prior_apply, TrainStep.depth_prior_weight_ / alignDepthPrior) against
float64 references.  Shared by test_depth_prior.py (emulator build) and test_gpu_depth_prior.py (MI355X).

References (on the CPU, neither involves the library under test): the expressions of include/gsr.h in torch -- validity, r = D / A
or A / D, the closed-form fit from centred sums, the aligned L1 or 1 - Pearson, gradients by autograd -- in float64 (the truth) and
the same expression in float32 (the yardstick).  Per case
    E_L = |loss - loss64|,   E_G = H W max over both gradient maps |grad - grad64|,   E_s, E_t, E_rho = |fit - fit64|
and B_* the same for the float32 expression; per group of cases (one content, one space, one mode: every size, with and without
the alpha map and the mask)
    max E_L <= 2 max B_L + 2^-22,  max E_G <= 2 max B_G + 2^-20   (the floors of loss_cases.py),
    max E_x <= 2 max B_x + 2^-22 max(1, |x64|)  for x in s, t, rho  (four float32 ulps of the value: fit[] is float32), n exact.
Sign pixels of the aligned L1 -- |r - s q - t| < 2^-18 (|r| + |s q| + |t|) in float64 -- are left out of E_G and B_G, at most 0.5 %
of a case's valid pixels; the exact-affine content is checked by its loss and fit only in that mode."""
import functools
import math
import zlib

import numpy as np
import torch

import loss_cases as lc
import parity
import pose_grad_cases as pg
from photo_slam_amd import capi, loss_utils, scene
from photo_slam_amd import rasterize_points as rp

FLOOR_L, FLOOR_G, FLOOR_FIT = lc.FLOOR_L, lc.FLOOR_G, 2.0 ** -22
SIZES = [(1, 1), (1, 40), (5, 33), (45, 70), (40, 75), (97, 132)]
FULL_HD = (1080, 1920)
MODES = [(False, False), (True, False), (False, True), (True, True)]     # (inverse, pearson)
CONTENTS = ["affine", "noisy", "anti", "invalid"]
ALPHA_MIN = 0.5
WEIGHT = 0.7
SIGN_REL = 2.0 ** -18
SIGN_CAP = 0.005
NOISE_SALT = 0        # chosen so that the float64 reference of every case stays inside SIGN_CAP (small maps: no sign pixel at all)


def mode_id(mode):
    return ("inverse" if mode[0] else "depth") + "-" + ("pearson" if mode[1] else "l1")


class Case:
    def __init__(self, name, inverse, pearson, D, A, q, valid):
        self.name, self.inverse, self.pearson = name, inverse, pearson
        self.D, self.A, self.q, self.valid = D, A, q, valid
        self.H, self.W = D.shape

    def __repr__(self):
        return f"{self.name}[{self.H}x{self.W} {mode_id((self.inverse, self.pearson))} A={self.A is not None} valid={self.valid is not None}]"


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


@functools.lru_cache(maxsize=None)
def maps(H, W):
    """(D, A) float32: an expected depth z in [1.2, 4] (smooth, plus pixel noise), alpha in [0.6, 1], D = z A"""
    y = torch.arange(H, dtype=torch.float64).view(H, 1)
    x = torch.arange(W, dtype=torch.float64).view(1, W)
    z = 2.5 + 0.8 * torch.sin(0.21 * x + 0.13 * y) + 0.4 * torch.sin(0.31 * y - 0.07 * x + 1.0)
    z = z + 0.1 * torch.rand(H, W, generator=_gen("z", H, W), dtype=torch.float64)
    A = (0.6 + 0.4 * torch.rand(H, W, generator=_gen("A", H, W), dtype=torch.float64)).float()
    return (z * A.double()).float(), A


def rendered64(D, A, inverse):
    a = torch.ones_like(D, dtype=torch.float64) if A is None else A.double()
    return a / D.double() if inverse else D.double() / a


def make_case(content, mode, H, W, with_alpha, with_valid):
    inverse, pearson = mode
    D, A = maps(H, W)
    D, A = D.clone(), A.clone()
    r = rendered64(D, A if with_alpha else None, inverse)
    noise = torch.randn(H, W, generator=_gen("noise", NOISE_SALT, content, H, W), dtype=torch.float64)
    scale = float(r.std()) if r.numel() > 1 else 1.0
    if content == "affine":
        q = 0.5 * r + 0.3
    elif content == "noisy":
        q = 0.5 * r + 0.3 + 0.15 * scale * noise
    elif content == "anti":
        q = 3.5 - 0.5 * r + 0.3 * scale * noise
    else:
        assert content == "invalid"
        q = 0.8 * r + 0.1 + 0.2 * scale * noise
    q = q.float()
    assert bool((q > 0).all())
    valid = None
    if with_valid:
        valid = (torch.rand(H, W, generator=_gen("valid", H, W)) > 0.15).to(torch.uint8) * 3   # (any non-zero byte is "set")
    if content == "invalid":
        g = _gen("invalid", H, W)
        pick = lambda p: torch.rand(H, W, generator=g) < p
        bad = [0.0, -1.0, float("nan"), float("inf"), float("-inf")]
        for k, v in enumerate(bad):            # scattered pixels
            q[pick(0.02)] = v
        A[pick(0.03)] = 0.3
        A[pick(0.01)] = 0.0
        D[pick(0.02)] = 0.0
        D[pick(0.02)] = -1.5
        if H >= 40:                            # whole rows
            q[3, :] = 0.0
            q[7, :] = float("nan")
            q[11, : W // 2] = float("inf")
            q[11, W // 2:] = -1.0
            A[15, :] = float(np.nextafter(np.float32(ALPHA_MIN), np.float32(0)))   # just below alpha_min
            A[16, :] = ALPHA_MIN                                             # on it: valid
            D[19, :] = 0.0
            D[23, :] = -2.0
    return Case(content, inverse, pearson, D, A if with_alpha else None, q, valid)


_cases = {}


def get(content, mode, H, W, with_alpha=True, with_valid=False):
    key = (content, mode, H, W, with_alpha, with_valid)
    if key not in _cases:
        _cases[key] = make_case(*key)
    return _cases[key]


def group(content, mode):
    return [get(content, mode, H, W, a, v) for (H, W) in SIZES for a in (True, False) for v in (False, True)]


# ---------------------------------------------------------------------------------------------------------------- references
def valid_mask(case):
    """the validity rule on the float32 inputs"""
    D, q = case.D, case.q
    ok = (D > 0) & torch.isfinite(q) & (q > 0)
    if case.A is not None:
        ok &= case.A >= np.float32(ALPHA_MIN)
    if case.valid is not None:
        ok &= case.valid != 0
    return ok


def reference(case, dtype, weight=WEIGHT):
    """dict(loss, gD, gA, s, t, rho, n, sign) of the torch expression in `dtype`, results in float64.  sign: the sign pixels of the
    aligned L1 (None in the Pearson mode)."""
    ok = valid_mask(case)
    H, W = case.H, case.W
    one = torch.ones((), dtype=dtype)
    D = torch.where(ok, case.D.to(dtype), one).requires_grad_(True)
    A = torch.where(ok, case.A.to(dtype) if case.A is not None else one, one).requires_grad_(True)
    q = torch.where(ok, case.q.to(dtype), one)
    n = int(ok.sum())
    zero = dict(loss=0.0, gD=torch.zeros(H, W, dtype=torch.float64), gA=torch.zeros(H, W, dtype=torch.float64), s=0.0, t=0.0, rho=0.0,
                n=n, sign=None if case.pearson else torch.zeros(H, W, dtype=torch.bool))
    if n < 2:
        return zero
    with torch.enable_grad():
        r = A / D if case.inverse else D / A
        m = ok.to(dtype)
        qm, rm = (q * m).sum() / n, (r * m).sum() / n
        dq, dr = (q - qm) * m, (r - rm) * m
        sqq, sqr, srr = (dq * dq).sum(), (dq * dr).sum(), (dr * dr).sum()
        q_ok = bool(sqq > 1e-12 * (q * q * m).sum())
        r_ok = bool(srr > 1e-12 * (r * r * m).sum())
        if not q_ok or (case.pearson and not r_ok):
            return zero
        s, t = (sqr / sqq).detach(), None
        t = (rm - s * qm).detach()
        rho = sqr / torch.sqrt(sqq * srr) if r_ok else torch.zeros((), dtype=dtype)
        res = (r - (s * q + t)) * m
        loss = weight * (1.0 - rho) if case.pearson else weight * res.abs().sum() / (H * W)
        gD, gA = torch.autograd.grad(loss, (D, A))
    assert loss.dtype == dtype and gD.dtype == dtype
    sign = None
    if not case.pearson:
        sign = ok & (res.detach().abs() < SIGN_REL * (r.detach().abs() + (s * q).abs() + t.abs()))
    gD, gA = gD.double() * ok, gA.double() * ok
    return dict(loss=float(loss.detach().double()), gD=gD, gA=gA if case.A is not None else torch.zeros_like(gD), s=float(s.double()),
                t=float(t.double()), rho=float(rho.detach().double().clamp(-1.0, 1.0)), n=n, sign=sign)


_refs = {}


def references(case):
    if id(case) not in _refs:
        _refs[id(case)] = (case, reference(case, torch.float64), reference(case, torch.float32))
    return _refs[id(case)][1:]


def _on(dev, case):
    t = lambda x: None if x is None else x.to(dev).contiguous()
    return t(case.D), t(case.A), t(case.q), t(case.valid)


def run_fused(dev, case, weight=WEIGHT):
    """the kernels through the Python wrapper: dict like reference(), in float64 on the CPU"""
    D, A, q, v = _on(dev, case)
    D.requires_grad_(True)
    if A is not None:
        A.requires_grad_(True)
    loss, fit = loss_utils.depth_prior_loss(D, A, q, weight, inverse=case.inverse, pearson=case.pearson, alpha_min=ALPHA_MIN, valid=v,
                                            return_fit=True)
    grads = torch.autograd.grad(loss, (D,) if A is None else (D, A))
    f = fit.detach().cpu().double()
    return dict(loss=float(loss.detach().cpu().double()), gD=grads[0].cpu().double(),
                gA=grads[1].cpu().double() if A is not None else torch.zeros(case.H, case.W, dtype=torch.float64),
                s=float(f[0]), t=float(f[1]), rho=float(f[2]), n=int(f[3]))


def _finite(out, case):
    assert math.isfinite(out["loss"]) and bool(torch.isfinite(out["gD"]).all()) and bool(torch.isfinite(out["gA"]).all()), f"{case}: NaN or Inf"
    assert all(math.isfinite(out[k]) for k in ("s", "t", "rho")), f"{case}: NaN or Inf in fit"


def errors(got, r64, r32, case, keep=None, grads=True):
    """one row of E_* / B_* (module docstring).  keep: the pixels that count for the gradients"""
    n = case.H * case.W
    row = dict(case=case, E_L=abs(got["loss"] - r64["loss"]), B_L=abs(r32["loss"] - r64["loss"]), E_G=0.0, B_G=0.0, worst=None)
    for k in ("s", "t", "rho"):
        row["E_" + k], row["B_" + k], row["V_" + k] = abs(got[k] - r64[k]), abs(r32[k] - r64[k]), abs(r64[k])
    if grads:
        keep = torch.ones(case.H, case.W, dtype=torch.bool) if keep is None else keep
        for k in ("gD", "gA"):
            e = (got[k] - r64[k]).abs() * keep
            if n * float(e.max()) >= row["E_G"]:
                row["E_G"], row["worst"] = n * float(e.max()), (k,) + tuple(lc.worst_pixel(e.unsqueeze(0)))[1:3]
            row["B_G"] = max(row["B_G"], n * float(((r32[k] - r64[k]).abs() * keep).max()))
    return row


def measure(dev, case):
    r64, r32 = references(case)
    got = run_fused(dev, case)
    _finite(got, case)
    assert got["n"] == r64["n"], (case, got["n"], r64["n"])
    invalid = ~valid_mask(case)
    assert not bool(got["gD"][invalid].any()) and not bool(got["gA"][invalid].any()), f"{case}: a gradient on an invalid pixel"
    keep = None
    if not case.pearson:
        share = float(r64["sign"].sum()) / max(r64["n"], 1)
        if case.name != "affine":
            assert share <= SIGN_CAP, f"{case}: {share:.3g} of the valid pixels are sign pixels in float64 (the inputs, not the code)"
        keep = ~r64["sign"]
    return errors(got, r64, r32, case, keep, grads=case.pearson or case.name != "affine")


def check_rows(rows, what):
    failures = []
    report = []
    for k, floor in (("L", FLOOR_L), ("G", FLOOR_G), ("s", None), ("t", None), ("rho", None)):
        w = max(rows, key=lambda r: r["E_" + k])
        E, B = w["E_" + k], max(r["B_" + k] for r in rows)
        if floor is None:
            floor = FLOOR_FIT * max(1.0, max(r["V_" + k] for r in rows))
        report.append(f"E_{k}={E:.3g} B_{k}={B:.3g}")
        if not E <= 2.0 * B + floor:
            failures.append(f"{k}: {E:.4g} at {w['case']} {w['worst'] if k == 'G' else ''} > 2 x {B:.4g} + {floor:.3g}")
    print(f"DEPTH_PRIOR {what} cases={len(rows)} " + " ".join(report))
    assert not failures, what + ": " + "; ".join(failures)


def check_group(dev, content, mode, tag=""):
    check_rows([measure(dev, c) for c in group(content, mode)], f"{tag} {content} {mode_id(mode)}")


def check_full_hd(dev, mode):
    """1080 x 1920: the grid is capped, every thread walks several groups of four pixels"""
    check_rows([measure(dev, get("invalid", mode, *FULL_HD, True, True))], f"gpu invalid 1080x1920 {mode_id(mode)}")


# ------------------------------------------------------------------------------------------------------------------- properties
def check_affine_invariance(dev):
    """q -> a q + b (a > 0): the loss and both gradients stay inside the bars of the float64 reference of the ORIGINAL prior, and
    (s, t) -> (s / a, t - s b / a).  The prior is quantised to 2^-12 and a = 2, b = 0.75, so that a q + b is exact in float32."""
    a, b = 2.0, 0.75
    for mode in MODES:
        rows = []
        for (H, W) in ((5, 33), (40, 75), (97, 132)):
            base = get("noisy", mode, H, W)
            q0 = torch.round(base.q * 4096.0) / 4096.0
            c0 = Case("noisy-quantised", mode[0], mode[1], base.D, base.A, q0, None)
            c1 = Case("noisy-mapped", mode[0], mode[1], base.D, base.A, a * q0 + b, None)
            assert bool(((c1.q.double() - (a * q0.double() + b)) == 0).all())
            r64, r32 = reference(c0, torch.float64), reference(c1, torch.float32)
            got = run_fused(dev, c1)
            _finite(got, c1)
            # in the units of the original prior
            got["s"], got["t"] = got["s"] * a, got["t"] + got["s"] * b
            r32["s"], r32["t"] = r32["s"] * a, r32["t"] + r32["s"] * b
            rows.append(errors(got, r64, r32, c1, None if mode[1] else ~r64["sign"]))
        check_rows(rows, f"affine invariance {mode_id(mode)}")


def _raw_zero(out, n, what):
    loss, gd, ga, fit = out
    assert float(loss) == 0.0 and not bool(gd.any()) and (ga is None or not bool(ga.any())), what
    assert fit.cpu().tolist() == [0.0, 0.0, 0.0, float(n)], (what, fit.cpu().tolist())


def check_degenerate(dev):
    """n < 2, a constant prior, and -- Pearson -- a constant render: loss 0, gradients all zero, fit = {0, 0, 0, n}, exactly"""
    H, W = 40, 75
    D, A = (t.to(dev) for t in maps(H, W))
    q = (0.5 * rendered64(D.cpu(), A.cpu(), False) + 0.3).float().to(dev)
    for flags in range(4):
        pearson = bool(flags & capi.DEPTH_PRIOR_PEARSON)
        none = torch.zeros(H, W, dtype=torch.uint8, device=dev)
        _raw_zero(raw_prior(D, A, q, none, flags), 0, ("n = 0", flags))
        one = none.clone()
        one[17, 31] = 1
        _raw_zero(raw_prior(D, A, q, one, flags), 1, ("n = 1", flags))
        _raw_zero(raw_prior(D, A, torch.full_like(q, 0.75), None, flags), H * W, ("constant prior", flags))
        _raw_zero(raw_prior(D, A, torch.full_like(q, float("nan")), None, flags), 0, ("NaN prior", flags))
        _raw_zero(raw_prior(D[:1, :1].contiguous(), None, q[:1, :1].contiguous(), None, flags), 1, ("1 x 1", flags))
        flat = raw_prior(torch.full_like(D, 2.0), None, q, None, flags)      # r constant, q not
        if pearson:
            _raw_zero(flat, H * W, ("constant render", flags))
        else:
            assert float(flat[3][2]) == 0.0 and float(flat[3][3]) == H * W and all(bool(torch.isfinite(t).all()) for t in flat if t is not None)


def check_nan_in_invalid_pixels(dev):
    """NaN planted in D and A where the pixel is invalid for another reason changes no output bit"""
    for mode in MODES:
        case = get("invalid", mode, 97, 132, True, True)
        D, A, q, v = _on(dev, case)
        flags = (1 if mode[0] else 0) | (2 if mode[1] else 0)
        base = raw_prior(D, A, q, v, flags)
        bad_q = ~(torch.isfinite(q) & (q > 0)) | (v == 0)
        D2, A2 = D.clone(), A.clone()
        D2[bad_q | (A < ALPHA_MIN)] = float("nan")
        A2[bad_q | ~(D > 0)] = float("nan")
        assert int(torch.isnan(D2).sum()) > 100 and int(torch.isnan(A2).sum()) > 100
        _same(raw_prior(D2, A2, q, v, flags), base, f"{case} NaN planted")
        assert all(bool(torch.isfinite(t).all()) for t in base)


# ------------------------------------------------------------------------------------------------- the C ABI with own buffers
def _lib():
    return rp._lib()


def raw_prior(D, A, q, valid, flags, weight=WEIGHT, alpha_min=ALPHA_MIN, gd=None, ga=None, fit=None, scratch=None, grads=True):
    """gsr_depth_prior_loss on the caller's tensors.  Returns (loss [1], grad_depth, grad_alpha or None, fit [4])."""
    lib = _lib()
    H, W = D.shape
    for t in (D, A, q):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous())
    assert valid is None or (valid.dtype == torch.uint8 and valid.is_contiguous())
    nb = int(lib.gsr_depth_prior_scratch_bytes(W, H))
    dev = D.device
    nan = lambda n: torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    if grads:
        gd = nan(H * W) if gd is None else gd
        ga = (nan(H * W) if ga is None else ga) if A is not None else None
    fit = nan(4) if fit is None else fit
    scratch = torch.empty(nb, dtype=torch.uint8, device=dev) if scratch is None else scratch
    assert scratch.numel() >= nb and scratch.data_ptr() % 8 == 0
    loss = nan(1) if grads else None
    ptr = lambda t: None if t is None else t.data_ptr()
    args = capi.DepthPriorArgs(W, H, ptr(D), ptr(A), ptr(q), ptr(valid), int(flags), float(alpha_min), float(weight), ptr(gd), ptr(ga),
                               ptr(loss), ptr(fit))
    import ctypes
    capi.check(lib, lib.gsr_depth_prior_loss(ctypes.byref(args), scratch.data_ptr(), rp._stream_ptr(D)), "gsr_depth_prior_loss")
    shape = lambda t: None if t is None else t[:H * W].view(H, W)
    return loss, shape(gd), shape(ga), fit


def _same(a, b, what):
    for x, y, name in zip(a, b, ("loss", "grad_depth", "grad_alpha", "fit")):
        assert (x is None) == (y is None), (what, name)
        if x is not None:
            assert torch.equal(x.cpu(), y.cpu()), f"{what}: {name} differs by {float((x.cpu() - y.cpu()).abs().max()):.3g}"


def _flags(mode):
    return (capi.DEPTH_PRIOR_INVERSE if mode[0] else 0) | (capi.DEPTH_PRIOR_PEARSON if mode[1] else 0)


def misaligned(t):
    """loss_cases.misaligned for a float32 map; a uint8 mask lands one byte past a 16-byte boundary"""
    if t.dtype == torch.float32:
        return lc.misaligned(t)
    buf = torch.empty(t.numel() + 16, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 1
    return v


def check_scalar_path(dev):
    """any pointer four bytes (the mask: one byte) past a 16-byte boundary takes the scalar path: the same bits"""
    for mode in MODES:
        for (H, W) in ((40, 75), (97, 132)):
            case = get("invalid", mode, H, W, True, True)
            D, A, q, v = _on(dev, case)
            assert all(t.data_ptr() % 16 == 0 for t in (D, A, q, v))
            base = raw_prior(D, A, q, v, _flags(mode))
            planes = dict(D=D, A=A, q=q, v=v)
            for which in [(k,) for k in planes] + [tuple(planes)]:
                d1, a1, q1, v1 = (misaligned(t) if k in which else t for k, t in planes.items())
                _same(raw_prior(d1, a1, q1, v1, _flags(mode)), base, f"{case}, {which} misaligned")
            gd = lc.misaligned(torch.empty(H, W, device=dev)).view(-1)
            _same(raw_prior(D, A, q, v, _flags(mode), gd=gd), base, f"{case}, grad_depth misaligned")
            _same(raw_prior(D, None, q, None, _flags(mode), gd=gd), raw_prior(D, None, q, None, _flags(mode)), f"{case}, no alpha, misaligned")


def check_fit_only(dev):
    """grad_depth == NULL && loss == NULL: fit alone, the bits of the full call, in both spaces"""
    for mode in MODES:
        case = get("invalid", mode, 97, 132, True, True)
        D, A, q, v = _on(dev, case)
        full = raw_prior(D, A, q, v, _flags(mode))
        only = raw_prior(D, A, q, v, _flags(mode), grads=False)
        assert only[0] is None and only[1] is None and torch.equal(only[3].cpu(), full[3].cpu())
        if not mode[1]:
            assert torch.equal(loss_utils.depth_prior_fit(D, A, q, inverse=mode[0], alpha_min=ALPHA_MIN, valid=v).cpu(), full[3].cpu())


def check_guard_bands(dev, sizes=((1, 1), (5, 33), (40, 75), (97, 132))):
    """4096 bytes of a byte pattern on either side of the scratch region, both gradient maps and fit"""
    lib = _lib()
    pad = 4 * lc.GUARD_FLOATS
    for mode in MODES:
        for (H, W) in sizes:
            case = get("noisy", mode, H, W)
            D, A, q, v = _on(dev, case)
            nb, n = int(lib.gsr_depth_prior_scratch_bytes(W, H)), H * W
            regions = (("scratch", nb), ("grad_depth", 4 * n), ("grad_alpha", 4 * n), ("fit", 16))
            bufs = {name: torch.full((pad + size + pad,), lc.GUARD_BYTE, dtype=torch.uint8, device=dev) for name, size in regions}
            inner = lambda name, size: bufs[name][pad:pad + size]
            out = raw_prior(D, A, q, v, _flags(mode), gd=inner("grad_depth", 4 * n).view(torch.float32),
                            ga=inner("grad_alpha", 4 * n).view(torch.float32), fit=inner("fit", 16).view(torch.float32),
                            scratch=inner("scratch", nb))
            for name, size in regions:
                buf = bufs[name].cpu()
                for side, band in (("before", buf[:pad]), ("after", buf[pad + size:])):
                    hit = torch.nonzero(band != lc.GUARD_BYTE).flatten()
                    assert hit.numel() == 0, f"{case}: {hit.numel()} bytes written {side} the {name} region, the first at offset {int(hit[0])}"
            _same(out, raw_prior(D, A, q, v, _flags(mode)), f"{case} guarded buffers")


def check_determinism(dev, H, W, runs):
    for mode in MODES:
        case = get("invalid", mode, H, W, True, True)
        D, A, q, v = _on(dev, case)
        first = None
        for _ in range(runs):
            res = [t.cpu() for t in raw_prior(D, A, q, v, _flags(mode))]
            first = first or res
            _same(res, first, f"{case} rerun")


def check_upstream_gradient(dev):
    """both gradients times the upstream gradient"""
    for mode in MODES:
        case = get("noisy", mode, 45, 70)
        D, A, q, v = _on(dev, case)

        def grads_of(scale):
            d, a = D.clone().requires_grad_(True), A.clone().requires_grad_(True)
            out = loss_utils.depth_prior_loss(d, a, q, WEIGHT, inverse=mode[0], pearson=mode[1], alpha_min=ALPHA_MIN)
            return torch.autograd.grad(out * scale if scale is not None else out, (d, a))

        plain = grads_of(None)
        assert bool(plain[0].any()) and bool(plain[1].any())
        got = grads_of(3.0)
        assert torch.equal(got[0], plain[0] * 3.0) and torch.equal(got[1], plain[1] * 3.0)


def check_cpp_host(ops, dev):
    """ops.depth_prior_loss / depth_prior_fit / depth_prior_apply of the C++ host and the Python wrappers: the same bits"""
    none_f, none_b = torch.empty(0, device=dev), torch.empty(0, dtype=torch.uint8, device=dev)
    for mode in MODES:
        for case in (get("invalid", mode, 40, 75, True, True), get("noisy", mode, 97, 132, False, False)):
            D, A, q, v = _on(dev, case)
            leaves = lambda: (D.clone().requires_grad_(True), None if A is None else A.clone().requires_grad_(True))
            d, a = leaves()
            out, fit = loss_utils.depth_prior_loss(d, a, q, WEIGHT, inverse=mode[0], pearson=mode[1], alpha_min=ALPHA_MIN, valid=v, return_fit=True)
            g = torch.autograd.grad(out, (d,) if a is None else (d, a))
            d2, a2 = leaves()
            out2, fit2 = ops.depth_prior_loss(d2, none_f if a2 is None else a2, q, WEIGHT, mode[0], mode[1], ALPHA_MIN, none_b if v is None else v)
            g2 = torch.autograd.grad(out2 * 1.0, (d2,) if a2 is None else (d2, a2))
            assert torch.equal(out2.detach(), out.detach()) and torch.equal(fit2, fit) and all(torch.equal(x, y) for x, y in zip(g2, g)), case
            f3 = ops.depth_prior_fit(D, none_f if A is None else A, q, mode[0], ALPHA_MIN, none_b if v is None else v)
            if not mode[1]:
                assert torch.equal(f3, fit)
            assert torch.equal(ops.depth_prior_apply(q, f3, mode[0], False), loss_utils.depth_prior_apply(q, f3, inverse=mode[0]))


# -------------------------------------------------------------------------------------------------------- gsr_depth_prior_apply
def check_apply(dev):
    """s q + t or 1 / (s q + t) against float64 with the float32 expression as the yardstick; zeros where q is invalid or the
    result is not positive; in place"""
    lib = _lib()
    for inverse in (False, True):
        for (H, W) in ((1, 1), (5, 33), (40, 75), (97, 132)):
            case = get("invalid", (inverse, False), H, W)
            q = case.q.to(dev).contiguous()
            for s, t in ((0.5, 0.3), (-0.4, 1.0), (0.0, 0.0), (1.0, 0.0)):
                fit = torch.tensor([s, t, 0.9, 5.0], dtype=torch.float32, device=dev)

                def expr(dtype):
                    qq, f = case.q.to(dtype), fit.cpu().to(dtype)
                    ok = torch.isfinite(qq) & (qq > 0)
                    m = f[0] * torch.where(ok, qq, torch.ones((), dtype=dtype)) + f[1]
                    o = 1.0 / m if inverse else m
                    return torch.where(ok & torch.isfinite(o) & (o > 0) & (m > 0), o, torch.zeros((), dtype=dtype)).double()

                want, yard = expr(torch.float64), expr(torch.float32)
                got = loss_utils.depth_prior_apply(q, fit, inverse=inverse)
                assert got.shape == q.shape and bool(torch.isfinite(got).all()) and bool((got >= 0).all())
                g = got.cpu().double()
                # (a result within rounding of 0 may land on either side: compare where the float64 value is clearly positive)
                sure = (want == 0) | (want > 1e-6)
                assert torch.equal((g == 0) & sure, (want == 0) & sure), (inverse, H, W, s, t)
                E, B = float(((g - want).abs() * sure).max()), float(((yard - want).abs() * sure).max())
                floor = FLOOR_FIT * max(1.0, float(want.max()))
                assert E <= 2.0 * B + floor, (inverse, H, W, s, t, E, B)
                bad = ~(torch.isfinite(case.q) & (case.q > 0))
                assert not bool(g[bad].any())
                if s == 0.0:
                    assert not bool(g.any())
                buf = q.clone()
                capi.check(lib, lib.gsr_depth_prior_apply(buf.data_ptr(), fit.data_ptr(), 1 if inverse else 0, W, H, buf.data_ptr(),
                                                          rp._stream_ptr(buf)), "gsr_depth_prior_apply")
                assert torch.equal(buf, got), (inverse, H, W, "in place")


# ------------------------------------------------------------------------------------------------------ descent at the loss level
DESCENT_STEPS = 40


def check_descent(dev):
    """plain gradient descent on D (A fixed) from a noisy start raises rho above its starting value in either mode; a step may
    lower rho by no more than the float32 yardstick's own distance from float64 at that point (+ the floor of rho)"""
    H, W = 40, 75
    D0, A = maps(H, W)
    for inverse in (False, True):
        r_true = rendered64(D0, A, inverse)
        q = (0.5 * r_true + 0.3).float()
        noise = torch.randn(H, W, generator=_gen("descent", inverse), dtype=torch.float64)
        start = (D0.double() * (1.0 + 0.15 * noise)).clamp_min(0.3).float()
        for pearson in (False, True):
            D = start.to(dev)
            Ad, qd = A.to(dev), q.to(dev)
            n = H * W
            # a step of a twentieth of the map's scale per unit of H W |grad|, shrinking: the L1 gradient has constant size
            rhos = []
            for k in range(DESCENT_STEPS):
                d = D.clone().requires_grad_(True)
                loss, fit = loss_utils.depth_prior_loss(d, Ad, qd, 1.0, inverse=inverse, pearson=pearson, alpha_min=ALPHA_MIN, return_fit=True)
                g = torch.autograd.grad(loss, d)[0]
                rhos.append(float(fit[2]))
                step = 0.05 / (1.0 + 0.25 * k)
                D = (D - step * n * g / float((n * g).abs().max().clamp_min(1e-12))).clamp_min(0.05)
            case = Case("descent", inverse, pearson, D.cpu(), A, q, None)
            noise_floor = abs(reference(case, torch.float32)["rho"] - reference(case, torch.float64)["rho"]) + FLOOR_FIT
            drops = [a - b for a, b in zip(rhos, rhos[1:])]
            print(f"DEPTH_PRIOR descent {mode_id((inverse, pearson))}: rho {rhos[0]:.6f} -> {rhos[-1]:.6f}, largest drop {max(drops):.3g}, "
                  f"yardstick noise {noise_floor:.3g}")
            assert rhos[-1] > rhos[0], (inverse, pearson, rhos[0], rhos[-1])
            assert max(drops) <= noise_floor, (inverse, pearson, max(drops), noise_floor)


# --------------------------------------------------------------------------------------------------------- through the rasterizer
def small_cloud():
    """the smallest cloud of depth_alpha_cases' tests"""
    return scene.make_cloud(600, 64, 48, 0.8 * 64, 0.8 * 64, seed=1, scale_k=0.35)


def prior_for(H, W):
    return (0.6 + 0.5 * lc.textured(H, W)[0]).contiguous()


def torch_prior_loss(depth, alpha, q, weight, inverse, pearson):
    """the float32 torch expression on device tensors (no mask), differentiable in depth and alpha"""
    ok = (alpha >= ALPHA_MIN) & (depth > 0) & torch.isfinite(q) & (q > 0)
    one = torch.ones((), dtype=depth.dtype, device=depth.device)
    d, a, qq = torch.where(ok, depth, one), torch.where(ok, alpha, one), torch.where(ok, q, one)
    r = a / d if inverse else d / a
    m = ok.to(depth.dtype)
    n = m.sum()
    qm, rm = (qq * m).sum() / n, (r * m).sum() / n
    dq, dr = (qq - qm) * m, (r - rm) * m
    sqq, sqr, srr = (dq * dq).sum(), (dq * dr).sum(), (dr * dr).sum()
    if pearson:
        return weight * (1.0 - sqr / torch.sqrt(sqq * srr))
    s = (sqr / sqq).detach()
    t = (rm - s * qm).detach()
    return weight * ((r - (s * qq + t)) * m).abs().sum() / depth.numel()


def check_through_rasterizer(dev):
    """render -> depth_prior_loss -> backward against render -> the float32 torch expression -> backward: the parameter gradients
    inside the gradient bars of depth_alpha_cases (parity.py)"""
    import depth_alpha_cases as da
    import forward_only_cases as fo
    from photo_slam_amd.gaussian_rasterizer import GaussianRasterizer
    cl = small_cloud()
    cam = cl.cameras[0]
    q = prior_for(cam.H, cam.W).to(dev)

    def run(loss_fn):
        t = lambda x: fo._t(x, dev).clone().requires_grad_(True)
        L = dict(means3D=t(cl.xyz), means2D=torch.zeros((cl.xyz.shape[0], 3), device=dev, requires_grad=True), opacities=t(cl.get_opacity()),
                 shs=t(cl.get_features()), scales=t(cl.get_scaling()), rotations=t(cl.get_rotation()))
        color, radii, depth, alpha = GaussianRasterizer(da._settings(cl, cam, dev))(
            L["means3D"], L["means2D"], L["opacities"], True, False, True, True, False, shs=L["shs"], scales=L["scales"], rotations=L["rotations"])
        loss_fn(depth, alpha).backward()
        return {k: v.grad.detach().cpu().numpy() for k, v in L.items() if k != "shs"}, radii.cpu().numpy() > 0

    for mode in MODES:
        got, vis = run(lambda d, a: loss_utils.depth_prior_loss(d, a, q, WEIGHT, inverse=mode[0], pearson=mode[1], alpha_min=ALPHA_MIN))
        ref, _ = run(lambda d, a: torch_prior_loss(d, a, q, WEIGHT, *mode))
        for name in got:
            assert np.isfinite(got[name]).all() and np.abs(ref[name]).sum() > 0, (mode, name)
            err = parity.rel_l1(got[name], ref[name])
            e = parity.row_errors(got[name], ref[name])[vis]
            row = dict(rel_l1=err, p9999=float(np.quantile(e, 0.9999)), max=float(e.max()), beyond=int((e > parity.ROW_OUTLIER).sum()))
            print(f"DEPTH_PRIOR rasterizer {mode_id(mode)} {name}: {row}")
            assert err <= parity.GRAD_REL_L1_TOL, (mode, name, row)
            assert row["p9999"] <= parity.ROW_P9999_TOL and row["max"] <= parity.ROW_MAX_TOL, (mode, name, row)
            assert row["beyond"] <= max(3, parity.ROW_OUTLIER_FRAC * e.size), (mode, name, row)


# ---------------------------------------------------------------------------------------------------------- TrainStep, both hosts
TRAIN_WEIGHT = 0.3
TRAIN_STEPS = 3


def _train_data(cl, dev):
    import depth_alpha_cases as da
    kfs, gts, _, mask = da.train_data(cl, dev)
    return kfs, gts, [prior_for(c.H, c.W).to(dev) for c in cl.cameras], mask


def _python_trainer(cl, dev, weight=0.0, pearson=False, inverse=True, fused=True):
    import depth_alpha_cases as da
    g, ts = da._python_trainer(cl, dev)
    ts.depth_prior_weight_, ts.depth_prior_pearson_, ts.depth_prior_inverse_ = weight, pearson, inverse
    ts.fused_sh_adam_ = ts.fused_geom_adam_ = fused
    return g, ts


def _params(g):
    g.sync_features()
    return [p.detach().clone() for p in g.params()]


def _same_params(a, b, exact, what):
    for k, (x, y) in enumerate(zip(a, b)):
        pg.same_or_rerun_close(f"{what}: tensor {k}", x, y, exact)


def check_train_python(lib_path, dev):
    """weight 0 with a prior, and a weight without a prior, are the parent's step; with a weight every step's loss is the RGB loss
    plus the term on a forward-only render of the same model, the step equals the hand-composed one (render with maps, the two
    losses, backward, the optimizer's step) and the fused optimizer steps agree with the dense ones; a process group throws"""
    from photo_slam_amd.gaussian_renderer import GaussianRenderer
    exact = dev.type == "cpu"
    cl = small_cloud()
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        kfs, gts, priors, mask = _train_data(cl, dev)
        n = len(kfs)

        def steps(weight, with_prior, pearson=False, fused=True, check_loss=False):
            g, ts = _python_trainer(cl, dev, weight, pearson, fused=fused)
            losses = []
            for it in range(TRAIN_STEPS):
                k = it % n
                if check_loss:
                    g.sync_features()
                    img, depth, alpha = ts.render_view(kfs[k], with_depth=True)
                    rgb = loss_utils.fused_l1_ssim_loss(img, gts[k], None, ts.opt_.lambda_dssim_)
                    term, fit = loss_utils.depth_prior_loss(depth, alpha, priors[k], weight, inverse=True, pearson=pearson,
                                                            alpha_min=ts.depth_prior_alpha_min_, return_fit=True)
                    assert float(term) > 0
                l = ts.trainForOneIteration(kfs[k], gts[k], mask, sync_loss=False, prior_depth=priors[k] if with_prior else None)
                if check_loss:
                    assert torch.equal(l.detach(), (rgb + term).detach()), (it, float(l), float(rgb), float(term))
                    assert torch.equal(ts.last_depth_prior_fit_, fit)
                elif not (with_prior and weight):
                    assert ts.last_depth_prior_fit_ is None
                losses.append(l.detach().clone())
            return losses, _params(g), ts

        parent_l, parent_p, _ = steps(0.0, False)
        for weight, with_prior in ((0.0, True), (TRAIN_WEIGHT, False)):
            l, p, _ = steps(weight, with_prior)
            assert torch.equal(l[0], parent_l[0])
            _same_params(p, parent_p, exact, f"weight {weight}, prior {with_prior}")
        for pearson in (False, True):
            _, fused_p, ts = steps(TRAIN_WEIGHT, True, pearson, check_loss=True)
            assert not torch.equal(fused_p[0], parent_p[0]), "the depth prior did not reach the positions"
            _, dense_p, _ = steps(TRAIN_WEIGHT, True, pearson, fused=False)
            # ---- the hand-composed step
            g, ts = _python_trainer(cl, dev, 0.0, fused=False)
            for it in range(TRAIN_STEPS):
                k = it % n
                g.updateLearningRate(it + 1)
                out = GaussianRenderer.render(kfs[k], kfs[k].image_height_, kfs[k].image_width_, g, ts.pipe_, ts.background_,
                                              training_outputs_only=True, cull_empty_tiles=ts.cull_empty_tiles_, render_depth=True,
                                              antialiasing=ts.antialiasing_)
                loss = loss_utils.fused_l1_ssim_loss(out[0], gts[k], None, ts.opt_.lambda_dssim_) + loss_utils.depth_prior_loss(
                    out[4], out[5], priors[k], TRAIN_WEIGHT, inverse=True, pearson=pearson, alpha_min=0.5)
                loss.backward()
                with torch.no_grad():
                    g.optimizer_.step()
                    g.optimizer_.zero_grad(set_to_none=True)
            _same_params(dense_p, _params(g), exact, f"hand-composed step, pearson={pearson}")
            for a, b, p0 in zip(fused_p, dense_p, parent_p):
                err = parity.rel_l1((a - p0).cpu().numpy(), (b - p0).cpu().numpy()) if float((b - p0).abs().sum()) else 0.0
                assert err <= (1e-5 if exact else 1e-3), ("fused against dense optimizer steps", pearson, err)
        # ---- a process group
        g, ts = _python_trainer(cl, dev, TRAIN_WEIGHT)
        ts.world_size_ = 2
        try:
            ts.trainForOneIteration(kfs[0], gts[0], mask, sync_loss=False, prior_depth=priors[0])
        except RuntimeError as e:
            assert "depth prior" in str(e)
        else:
            raise AssertionError("a depth prior with a process group was accepted")
        assert ts.iteration_ == 0
    finally:
        rp._LIB_OVERRIDE = prev


def _cpp_trainer(ops, cl, dev, weight=0.0, pearson=False):
    import depth_alpha_cases as da
    h = da._cpp_trainer(ops, cl, dev)
    ops.trainer_set_options(h, {"depth_prior_weight": float(weight), "depth_prior_pearson": 1.0 if pearson else 0.0,
                                "depth_prior_inverse": 1.0, "depth_prior_alpha_min": 0.5})
    return h


def check_train_cpp(ops, lib_path, dev):
    """the C++ host: weight 0 with a prior and a weight without one are the parent's step; with a weight the loss is the RGB loss
    plus the term on the same render, the fit is reported, and the parameters agree with the Python host's"""
    import depth_alpha_cases as da
    exact = dev.type == "cpu"
    cl = small_cloud()
    kfs, gts, priors, mask = _train_data(cl, dev)
    cams = [da._cam_args(c, dev) for c in cl.cameras]
    n = len(cams)
    none = torch.empty(0, device=dev)

    def steps(weight, with_prior, pearson=False, check_loss=False):
        h = _cpp_trainer(ops, cl, dev, weight, pearson)
        try:
            losses = []
            for it in range(TRAIN_STEPS):
                k = it % n
                if check_loss:
                    img, depth, alpha = ops.trainer_render_view_depth(h, *cams[k])
                    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
                    try:
                        rgb = loss_utils.fused_l1_ssim_loss(img, gts[k], None, 0.2)
                        term, fit = loss_utils.depth_prior_loss(depth, alpha, priors[k], weight, inverse=True, pearson=pearson, alpha_min=0.5,
                                                                return_fit=True)
                    finally:
                        rp._LIB_OVERRIDE = prev
                l = ops.trainer_train_depth_prior(h, *cams[k], gts[k], mask, none, priors[k] if with_prior else none)
                if check_loss:
                    assert torch.equal(l, (rgb + term).detach()), (it, float(l), float(rgb), float(term))
                    assert torch.equal(ops.trainer_last_depth_prior_fit(h), fit)
                elif not (with_prior and weight):
                    assert ops.trainer_last_depth_prior_fit(h).numel() == 0
                losses.append(l.clone())
            return losses, [p.detach().clone() for p in ops.trainer_params(h)]
        finally:
            ops.trainer_destroy(h)

    parent_l, parent_p = steps(0.0, False)
    for weight, with_prior in ((0.0, True), (TRAIN_WEIGHT, False)):
        l, p = steps(weight, with_prior)
        assert torch.equal(l[0], parent_l[0])
        _same_params(p, parent_p, exact, f"C++ weight {weight}, prior {with_prior}")
    for pearson in (False, True):
        cpp_l, cpp_p = steps(TRAIN_WEIGHT, True, pearson, check_loss=True)
        assert not torch.equal(cpp_p[0], parent_p[0]), "the depth prior did not reach the positions"
        prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
        try:
            g, ts = _python_trainer(cl, dev, TRAIN_WEIGHT, pearson)
            py_l = [ts.trainForOneIteration(kfs[it % n], gts[it % n], mask, sync_loss=False, prior_depth=priors[it % n]).item()
                    for it in range(TRAIN_STEPS)]
            py_p = _params(g)
        finally:
            rp._LIB_OVERRIDE = prev
        # (the bars of depth_alpha_cases.check_train_step_hosts)
        assert np.allclose([float(x) for x in cpp_l], py_l, rtol=1e-5), (cpp_l, py_l)
        for a, b in zip(cpp_p, py_p):
            if exact:
                assert torch.allclose(a, b, rtol=1e-4, atol=1e-6)
            else:
                assert parity.rel_l1(a.cpu().numpy(), b.cpu().numpy()) <= 1e-3


def check_process_group_cpp(ops, dev, tmp_path):
    import torch.distributed as dist
    import depth_alpha_cases as da
    cl = small_cloud()
    dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "store"), rank=0, world_size=1)
    h = _cpp_trainer(ops, cl, dev, TRAIN_WEIGHT)
    try:
        ops.trainer_set_process_group(h, dist.group.WORLD.group_name, True)
        c = cl.cameras[0]
        gt = torch.zeros(3, c.H, c.W, device=dev)
        try:
            ops.trainer_train_depth_prior(h, *da._cam_args(c, dev), gt, torch.ones_like(gt), torch.empty(0, device=dev), prior_for(c.H, c.W).to(dev))
        except RuntimeError as e:
            assert "depth prior" in str(e)
        else:
            raise AssertionError("a depth prior with a process group was accepted")
    finally:
        ops.trainer_destroy(h)
        dist.destroy_process_group()


# ------------------------------------------------------------------------------------------------------ alignment and seeding
def _align_reference(depth, alpha, q, dtype):
    """the float64 / float32 restatement of alignDepthPrior on the given render (inverse space, alpha_min 0.5): (map, fit)"""
    case = Case("align", True, False, depth.cpu(), alpha.cpu(), q.cpu(), None)
    ref = reference(case, dtype)
    qq = case.q.to(dtype)
    m = ref["s"] * qq + ref["t"]
    out = torch.where((qq > 0) & (m > 0), 1.0 / m, torch.zeros((), dtype=dtype))
    return out.double(), ref


def check_align_and_seed_python(lib_path, dev):
    """alignDepthPrior against the float64 restatement fed the same render; seedFromDepth(aligned) appends the rows
    GaussianModel.seedFromDepth gives for that tensor; an empty model throws"""
    import seed_cases as sc
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        cl, kf, gt_image, gt_depth, inside, rect = sc.host_frame(dev)
        g, ts = sc.python_trainer(cl, dev)
        g.prunePoints(inside)
        P = int(g.xyz_.shape[0])
        # a relative inverse-depth prior of the scene: an affine map of 1 / depth of the full model, with a little noise
        noise = torch.randn(gt_depth.shape, generator=torch.Generator().manual_seed(3)).to(dev)
        prior = torch.where(gt_depth > 0, 0.8 / gt_depth.clamp_min(1e-3) + 0.05 + 0.002 * noise, torch.zeros_like(gt_depth)).contiguous()
        _, depth, alpha = ts.render_view(kf, with_depth=True)
        aligned, fit = ts.alignDepthPrior(kf, prior)
        want, r64 = _align_reference(depth, alpha, prior, torch.float64)
        yard, r32 = _align_reference(depth, alpha, prior, torch.float32)
        f = fit.cpu().double().tolist()
        assert f[3] == r64["n"] > 100
        for k, name in enumerate(("s", "t", "rho")):
            assert abs(f[k] - r64[name]) <= 2.0 * abs(r32[name] - r64[name]) + FLOOR_FIT * max(1.0, abs(r64[name])), (name, f[k], r64[name])
        E, B = float((aligned.cpu().double() - want).abs().max()), float((yard - want).abs().max())
        print(f"DEPTH_PRIOR align: fit {f}, float64 {[r64[k] for k in ('s', 't', 'rho')]}, E={E:.3g} B={B:.3g}")
        assert E <= 2.0 * B + FLOOR_FIT * max(1.0, float(want.max())), (E, B)
        assert torch.equal(aligned == 0, prior <= 0)
        assert r64["rho"] > 0.5   # (the prior is an affine map of the full model, the render is the pruned one: related, not equal)
        # ---- seeding from the aligned map: the trainer's call against the model's own on a twin
        g2, ts2 = sc.python_trainer(cl, dev)
        g2.prunePoints(inside)
        n = ts.seedFromDepth(kf, gt_image, aligned, 17, want_pixels=True)
        W, H = kf.image_width_, kf.image_height_
        n2 = g2.seedFromDepth(aligned, gt_image, alpha, depth, kf.world_view_transform_, W / (2.0 * kf.tanfovx_), H / (2.0 * kf.tanfovy_),
                              (W - 1) / 2.0, (H - 1) / 2.0, 17, int(ts2.seed_max_new_), min_depth=ts2.depth_min_, max_depth=ts2.depth_max_,
                              alpha_threshold=ts2.seed_alpha_threshold_, depth_error_abs=ts2.seed_depth_error_abs_,
                              depth_median_factor=ts2.seed_depth_median_factor_, stride=ts2.seed_stride_, scale_factor=ts2.seed_scale_factor_,
                              init_opacity=ts2.seed_init_opacity_, want_pixels=True)
        assert n == n2 > 0 and torch.equal(g.last_seed_pixels_, g2.last_seed_pixels_)
        for a, b in zip(g.params(), g2.params()):
            assert a.shape[0] == P + n and torch.equal(a.detach(), b.detach())
        # ---- an empty model
        from photo_slam_amd.gaussian_model import GaussianModel
        _, ts3 = sc.python_trainer(None, dev)
        try:
            ts3.alignDepthPrior(kf, prior)
        except RuntimeError as e:
            assert "empty" in str(e)
        else:
            raise AssertionError("alignDepthPrior on an empty model was accepted")
        return aligned, fit, prior, n
    finally:
        rp._LIB_OVERRIDE = prev


def check_align_and_seed_cpp(ops, lib_path, dev):
    """the C++ host's alignDepthPrior and the seeding from its map against the Python host's"""
    import seed_cases as sc
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        cl, _, gt_image, gt_depth, inside, rect = sc.host_frame(dev)
        kf = sc._cpp_keyframe(cl.cameras[0], dev)
        g, ts = sc.python_trainer(cl, dev)
        g.prunePoints(inside)
        noise = torch.randn(gt_depth.shape, generator=torch.Generator().manual_seed(3)).to(dev)
        prior = torch.where(gt_depth > 0, 0.8 / gt_depth.clamp_min(1e-3) + 0.05 + 0.002 * noise, torch.zeros_like(gt_depth)).contiguous()
        aligned_py, fit_py = ts.alignDepthPrior(kf, prior)
        n_py = ts.seedFromDepth(kf, gt_image, aligned_py, 17, want_pixels=True)
    finally:
        rp._LIB_OVERRIDE = prev
    args = pg._cam_args(cl.cameras[0], dev)
    h = pg.cpp_trainer(ops, cl, dev, deg=3)
    try:
        ops.trainer_prune_points(h, inside)
        aligned, fit = ops.trainer_align_depth_prior(h, *args, prior)
        assert torch.equal(fit, fit_py) and torch.equal(aligned, aligned_py)
        n = ops.trainer_seed_from_depth(h, *args, gt_image, aligned, 17)
        assert n == n_py > 0
        for a, b in zip(ops.trainer_params(h), g.params()):
            assert a.shape == b.shape and torch.equal(a.detach(), b.detach())
    finally:
        ops.trainer_destroy(h)
    h = ops.trainer_create_empty(3, torch.zeros(3, device=dev))
    try:
        try:
            ops.trainer_align_depth_prior(h, *args, prior)
        except RuntimeError as e:
            assert "empty" in str(e)
        else:
            raise AssertionError("alignDepthPrior on an empty model was accepted")
    finally:
        ops.trainer_destroy(h)
