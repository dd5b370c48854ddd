"""The fused L1+SSIM loss, Adam and the depth loss (csrc/train_ops.hip) against float64 references, on the image content training
sees.  Shared by test_loss_reference.py (emulator build) and test_gpu_loss_reference.py (MI355X).

References (both on the CPU, neither involves the library under test):
  * float64: loss_utils.l1_loss / ssim on .double() copies of the float32 inputs -- the truth;
  * float32: the same ATen expression in float32 -- the yardstick: the reference project's own formulation, whose distance from
    the float64 result is what "as accurate as the reference" means.

Per case   E_L = |loss - loss64|,  E_G = 3 H W max_pixels |grad - grad64|  (the gradient in units of its natural scale 1/N: it
stays meaningful where the true gradient is zero);  B_L, B_G the same for float32 ATen.  Per content class (every size and mask
variant of one kind of content at one lambda)

    max_class E <= 2 max_class B + floor,   floor_L = 2^-22, floor_G = 2^-20.

A class maximum, because the float32 biases are signed and cancel by chance in single cases; a margin of 2, because the kernel
evaluates the same float32 E[x^2] - mu^2 as ATen; floor_L = four float32 ulps of the mean S ~ 1 the loss is subtracted from,
floor_G the same with a factor for the 121-tap transposed filter: they only keep classes with B ~ 0 from dividing by nothing."""
import ctypes
import functools
import math
import zlib

import numpy as np
import torch

from photo_slam_amd import capi, loss_utils
from photo_slam_amd import rasterize_points as rp

LAM = 0.2
FLOOR_L, FLOOR_G = 2.0 ** -22, 2.0 ** -20
FULL_SIZES = [(45, 70), (40, 72), (64, 64)]          # every content class
EDGE_SIZES = ([(1, 1), (1, 40), (40, 1), (5, 33),                                   # smaller than a window
               (10, 12), (11, 11), (12, 10),                                         # window half width +- 1 ... window
               (31, 33), (32, 32), (33, 31), (63, 65), (64, 64), (65, 63),           # around one and two tiles
               (40, 72), (40, 73), (40, 74), (40, 75)]                               # W % 4 = 0, 1, 2, 3
              + [(8, 32 * k - 3) for k in range(1, 9)]                               # 3 gx gy = 3, 6, ..., 24 workgroups
              + [(97, 132)])                                                         # a non-square grid of several rows
CLASSES = ["noise", "textured", "flat", "black", "equal", "range", "impulse"]
FLAT_LEVELS = [0.05, 0.25, 0.5, 0.75, 0.97]
MASKS = ["binary", "tile", "soft"]


class Case:
    def __init__(self, cls, name, lam, rendered, gt, mask):
        self.cls, self.name, self.lam = cls, name, lam
        self.rendered, self.gt, self.mask = rendered, gt, mask
        self.H, self.W = rendered.shape[1:]

    def __repr__(self):
        return f"{self.name}[{self.H}x{self.W}, lambda={self.lam}]"


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def textured(H, W):
    """a smooth sinusoid pattern in [0.1, 0.9] with periods of 17 to 27 pixels, different in every channel"""
    y = torch.arange(H, dtype=torch.float64).view(1, H, 1)
    x = torch.arange(W, dtype=torch.float64).view(1, 1, W)
    c = torch.arange(3, dtype=torch.float64).view(3, 1, 1)
    v = 0.5 + 0.2 * torch.sin(0.37 * x + 0.11 * y + 0.9 * c) + 0.2 * torch.sin(0.23 * y - 0.05 * x + 1.7 * c)
    return v.float()


def make_mask(kind, H, W):
    g = _gen("mask", kind, H, W)
    if kind == "binary":                      # 80 % ones
        return (torch.rand(3, H, W, generator=g) > 0.2).float()
    if kind == "soft":                        # not binary
        return torch.rand(3, H, W, generator=g)
    assert kind == "tile"                     # zero on the whole tile (ty, tx) = (0, 1) and its 5-pixel halo
    m = torch.ones(3, H, W)
    m[:, 0:32 + 5, 32 - 5:64 + 5] = 0.0
    return m


def impulse_positions(H, W):
    """(y, x): the image corners, the four pixels around the corner shared by tiles (0,0) (0,1) (1,0) (1,1), and the last row /
    column whose 11-tap window still reaches tile 0 -- the 21 x 21 footprint of the gradient then crosses the tile corner"""
    return [(0, 0), (H - 1, W - 1), (31, 31), (32, 32), (31, 32), (36, 27), (27, 36)]


@functools.lru_cache(maxsize=None)
def content(cls, H, W):
    """[(variant name, rendered, gt)] of one content class at one size (shared: nobody writes to these tensors)"""
    tex = textured(H, W)
    n = lambda *key: torch.randn(3, H, W, generator=_gen(cls, H, W, *key))
    if cls == "noise":                        # the pair of tests/test_train_ops.py
        g = _gen(cls, H, W)
        return [("noise", torch.rand(3, H, W, generator=g), torch.rand(3, H, W, generator=g))]
    if cls == "textured":                     # a converged view
        return [("textured", tex + 1e-3 * n(), tex)]
    if cls == "flat":
        out = []
        for level in FLAT_LEVELS:
            gt = torch.full((3, H, W), level)
            for sigma in (1e-3, 1e-2):
                out.append((f"flat{level}s{sigma:g}", gt + sigma * n(level, sigma), gt))
        gt = torch.full((3, H, W), 0.75)
        step = W // 2 + 1                     # 36, 37, 33: not on a tile boundary
        assert step % 32 != 0
        gt[:, :, step:] = 0.25
        out.append(("flatsplit", gt + 1e-3 * n("split"), gt))
        return out
    if cls == "black":                        # the first iterations
        return [("black", torch.zeros(3, H, W), tex)]
    if cls == "equal":
        return [("equal", tex.clone(), tex)]
    if cls == "range":                        # negative values and values above 1
        return [("range", 4.0 * tex - 1.0, tex)]
    assert cls == "impulse"
    out = []
    for (y, x) in impulse_positions(H, W):
        r = tex.clone()
        r[:, y, x] += 0.1
        out.append((f"impulse{y}_{x}", r, tex))
    return out


_cases = {}


def get(cls, name, H, W, lam=LAM):
    """The case `name` (a content variant of class cls, "+binary" / "+tile" / "+soft" appended for a mask) at H x W: built once,
    so that its references are computed once."""
    key = (cls, name, H, W, lam)
    if key not in _cases:
        for variant, r, gt in content(cls, H, W):
            _cases[(cls, variant, H, W, lam)] = Case(cls, variant, lam, r, gt, None)
            for kind in MASKS:
                _cases[(cls, f"{variant}+{kind}", H, W, lam)] = Case(cls, f"{variant}+{kind}", lam, r, gt, make_mask(kind, H, W))
    return _cases[key]


def group(cls, lam=LAM):
    """The cases of one content class at one lambda: at lambda = 0.2 every content variant on FULL_SIZES -- `textured` on EDGE_SIZES
    as well, `textured` and `flat` with every mask on FULL_SIZES too; at lambda = 0 and 1 (the L1 and the SSIM branch alone)
    every content variant at 45 x 70."""
    sizes = list(FULL_SIZES) if lam == LAM else FULL_SIZES[:1]
    if cls == "textured" and lam == LAM:
        sizes += [s for s in EDGE_SIZES if s not in sizes]
    cases = []
    for (H, W) in sizes:
        for name, _, _ in content(cls, H, W):
            cases.append(get(cls, name, H, W, lam))
            if cls in ("textured", "flat") and lam == LAM and (H, W) in FULL_SIZES:
                cases += [get(cls, f"{name}+{kind}", H, W, lam) for kind in MASKS]
    return cases


# ---------------------------------------------------------------------------------------------------------------- references
def reference(case, dtype):
    """(loss, gradient) of the ATen expression in `dtype` on the CPU, both returned in float64"""
    x = case.rendered.detach().cpu().to(dtype).requires_grad_(True)
    gt = case.gt.detach().cpu().to(dtype)
    xm = x if case.mask is None else x * case.mask.detach().cpu().to(dtype)
    with torch.enable_grad():
        loss = (1.0 - case.lam) * loss_utils.l1_loss(xm, gt) + case.lam * (1.0 - loss_utils.ssim(xm.unsqueeze(0), gt.unsqueeze(0)))
        (grad,) = torch.autograd.grad(loss, x)
    assert loss.dtype == dtype and grad.dtype == dtype
    return float(loss.detach().double()), grad.detach().double()


_refs = {}


def references(case):
    """float64 and float32 references of a case, computed once and shared by every test that needs them"""
    if id(case) not in _refs:
        _refs[id(case)] = (case, reference(case, torch.float64), reference(case, torch.float32))
    return _refs[id(case)][1:]


def run_fused(dev, case):
    """(loss, gradient) of the fused kernels through the Python wrapper, in float64 on the CPU"""
    r = case.rendered.to(dev).requires_grad_(True)
    mask = None if case.mask is None else case.mask.to(dev)
    out = loss_utils.fused_l1_ssim_loss(r, case.gt.to(dev), mask, case.lam)
    (g,) = torch.autograd.grad(out, r)
    return out.detach().cpu().double().item(), g.detach().cpu().double()


def worst_pixel(err):
    """(channel, y, x, y % 32, x % 32) of the largest entry of a [3,H,W] error map"""
    _, H, W = err.shape
    i = int(torch.argmax(err))
    c, y, x = i // (H * W), (i // W) % H, i % W
    return (c, y, x, y % 32, x % 32)


def measure(dev, case):
    (l64, g64), (l32, g32) = references(case)
    loss, grad = run_fused(dev, case)
    n = 3 * case.H * case.W
    eg = (grad - g64).abs()
    assert math.isfinite(loss) and bool(torch.isfinite(grad).all()), f"{case}: the kernels returned NaN or Inf"
    return dict(case=case, loss64=l64, bias=loss - l64, bias32=l32 - l64, E_L=abs(loss - l64), B_L=abs(l32 - l64),
                E_G=n * float(eg.max()), B_G=n * float((g32 - g64).abs().max()), worst=worst_pixel(eg))


def check_group(dev, cls, lam=LAM, tag=""):
    """max_class E <= 2 max_class B + floor for the loss and for the gradient; every case runs, every pixel counts.  Prints
    the figures of the class (pytest -s)."""
    rows = [measure(dev, c) for c in group(cls, lam)]
    wl = max(rows, key=lambda r: r["E_L"])
    wg = max(rows, key=lambda r: r["E_G"])
    EL, EG = wl["E_L"], wg["E_G"]
    BL, BG = max(r["B_L"] for r in rows), max(r["B_G"] for r in rows)
    sb = max(rows, key=lambda r: abs(r["bias"]))
    line = (f"LOSSREF {tag} {cls} lambda={lam:g} cases={len(rows)} E_L={EL:.3g} B_L={BL:.3g} E_G={EG:.3g} B_G={BG:.3g} "
            f"bias={sb['bias']:+.3g} (ATen {sb['bias32']:+.3g}) at {sb['case']} worst_grad={wg['case']} (c,y,x,y%32,x%32)={wg['worst']}")
    print(line)
    failures = []
    if not EL <= 2.0 * BL + FLOOR_L:
        failures.append(f"loss: |fused - f64| = {EL:.4g} at {wl['case']} (signed {wl['bias']:+.4g}, ATen f32 {wl['bias32']:+.4g}, "
                        f"loss {wl['loss64']:.6g}) > 2 x {BL:.4g} + {FLOOR_L:.3g}")
    if not EG <= 2.0 * BG + FLOOR_G:
        failures.append(f"gradient: 3HW max|fused - f64| = {EG:.4g} > 2 x {BG:.4g} + {FLOOR_G:.3g}")
    # (the worst gradient pixel goes into every message: it is what places a fault in the tile)
    assert not failures, (f"class {cls}, lambda {lam:g}: " + "; ".join(failures) + f"; worst gradient pixel: {wg['case']}, "
                          f"3HW |fused - f64| = {EG:.4g} at (channel, y, x, y % 32, x % 32) = {wg['worst']}")


def check_equal_images(dev):
    """rendered == gt bit for bit: sign(0) = 0 in the L1 term, so with lambda = 0 the loss and every gradient entry are exactly 0"""
    for (H, W) in FULL_SIZES:
        tex = textured(H, W)
        for mask in (None, make_mask("binary", H, W)):
            gt = tex if mask is None else tex * mask          # (binary mask: x * m == gt exactly)
            loss, grad = run_fused(dev, Case("equal", "equal", 0.0, tex.clone(), gt, mask))
            assert loss == 0.0 and not bool(grad.any()), (H, W, loss, float(grad.abs().max()), worst_pixel(grad.abs()))


# ------------------------------------------------------------------------------------------------- the C ABI with own buffers
def _lib():
    return rp._lib()


def misaligned(t):
    """a contiguous copy of t at a storage offset of one float: 4 bytes past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def misaligned_vector_loads(lib):
    """The emulator build counts the 16-byte staging loads that were not 16-byte aligned (train_ops.hip: LOSS_LOAD_F4) -- the CPU
    and the device both take them, so the results cannot tell; reading resets the count.  The device build has no counter: 0."""
    if not hasattr(lib, "gsr_emu_loss_misaligned_loads"):
        return 0
    lib.gsr_emu_loss_misaligned_loads.restype = ctypes.c_longlong
    return int(lib.gsr_emu_loss_misaligned_loads())


def raw_loss(r, gt, mask, lam, grad=None, scratch=None):
    """gsr_l1_ssim_loss on the caller's tensors; `grad` (float32, >= 3 H W) and `scratch` (uint8) may be the caller's own.
    Returns (loss [1], grad)."""
    lib = _lib()
    _, H, W = r.shape
    for t in (r, gt, mask):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous())
    if grad is None:
        grad = torch.empty(3 * H * W, dtype=torch.float32, device=r.device)
    if scratch is None:
        scratch = torch.empty(int(lib.gsr_loss_scratch_bytes(W, H)), dtype=torch.uint8, device=r.device)
    assert grad.numel() >= 3 * H * W and scratch.numel() >= lib.gsr_loss_scratch_bytes(W, H) and scratch.data_ptr() % 16 == 0
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device=r.device)
    misaligned_vector_loads(lib)
    capi.check(lib, lib.gsr_l1_ssim_loss(r.data_ptr(), gt.data_ptr(), None if mask is None else mask.data_ptr(), W, H, float(lam),
                                         grad.data_ptr(), loss.data_ptr(), scratch.data_ptr(), rp._stream_ptr(r)), "gsr_l1_ssim_loss")
    assert misaligned_vector_loads(lib) == 0, "the vector staging path ran on a plane that is not 16-byte aligned"
    return loss, grad


def _on(dev, case):
    return case.rendered.to(dev).contiguous(), case.gt.to(dev).contiguous(), None if case.mask is None else case.mask.to(dev).contiguous()


def staging_cases():
    return [get("textured", "textured+soft", 40, 72), get("flat", "flat0.97s0.001+binary", 64, 64), get("noise", "noise", 40, 72),
            get("textured", "textured", 64, 64)]


def check_scalar_staging(dev):
    """W % 4 == 0 with a plane that does not start on a 16-byte boundary takes the scalar staging path (vec = 0): the arithmetic
    behind the staging is the same code, so the loss and the gradient equal the aligned run's bit for bit."""
    for case in staging_cases():
        assert case.W % 4 == 0
        r, gt, m = _on(dev, case)
        assert all(t is None or t.data_ptr() % 16 == 0 for t in (r, gt, m))
        loss0, grad0 = raw_loss(r, gt, m, case.lam)
        planes = dict(rendered=r, gt=gt, mask=m)
        names = [k for k, t in planes.items() if t is not None]
        for which in [(k,) for k in names] + [tuple(names)]:      # each plane on its own, then all together
            r1, g1, m1 = (misaligned(t) if k in which else t for k, t in planes.items())
            loss1, grad1 = raw_loss(r1, g1, m1, case.lam)
            d = (grad1 - grad0).abs().view(3, case.H, case.W)
            assert torch.equal(loss1, loss0) and torch.equal(grad1, grad0), \
                (f"{case}, {which} misaligned: loss {loss1.item()!r} / {loss0.item()!r}, gradient differs by {float(d.max()):.3g} at "
                 f"(channel, y, x, y % 32, x % 32) = {worst_pixel(d)}")


def check_poisoned_buffers(dev):
    """nothing of what the scratch region and the gradient buffer held before the call reaches the results"""
    lib = _lib()
    for case in [get("textured", "textured", 33, 31), get("textured", "textured+binary", 40, 72), get("textured", "textured", 40, 75),
                 get("textured", "textured", 8, 93), get("textured", "textured", 1, 1)]:
        r, gt, m = _on(dev, case)
        nb, n = int(lib.gsr_loss_scratch_bytes(case.W, case.H)), 3 * case.H * case.W
        assert nb % 4 == 0
        res = []
        for fill in (0.0, float("nan")):
            scratch = torch.full((nb // 4,), fill, dtype=torch.float32, device=dev)
            grad = torch.full((n,), fill, dtype=torch.float32, device=dev)
            loss, grad = raw_loss(r, gt, m, case.lam, grad=grad, scratch=scratch.view(torch.uint8))
            res.append((loss.cpu(), grad.cpu()))
        (l0, g0), (l1, g1) = res
        assert not bool(torch.isnan(l1).any()) and not bool(torch.isnan(g1).any()), case
        assert torch.equal(l0, l1) and torch.equal(g0, g1), case


GUARD_FLOATS = 1024
GUARD_BYTE = 0xA5


def check_guard_bands(dev, sizes=((1, 1), (33, 31), (40, 75))):
    """The kernels write inside gsr_loss_scratch_bytes(W, H) bytes of scratch and 3 H W floats of gradient, nowhere else: both lie
    inside larger buffers of the test's own, 4096 bytes of a byte pattern on either side, which are read back afterwards."""
    lib = _lib()
    pad = 4 * GUARD_FLOATS
    for (H, W) in sizes:
        case = get("textured", "textured", H, W)
        r, gt, m = _on(dev, case)
        nb, n = int(lib.gsr_loss_scratch_bytes(W, H)), 3 * H * W
        sbuf = torch.full((pad + nb + pad,), GUARD_BYTE, dtype=torch.uint8, device=dev)
        gbuf = torch.full((pad + 4 * n + pad,), GUARD_BYTE, dtype=torch.uint8, device=dev)
        loss, grad = raw_loss(r, gt, m, case.lam, grad=gbuf[pad:pad + 4 * n].view(torch.float32), scratch=sbuf[pad:pad + nb])
        for name, buf, size in (("scratch", sbuf.cpu(), nb), ("gradient", gbuf.cpu(), 4 * n)):
            for side, band in (("before", buf[:pad]), ("after", buf[pad + size:])):
                hit = torch.nonzero(band != GUARD_BYTE).flatten()
                assert hit.numel() == 0, f"{H}x{W}: {hit.numel()} bytes written {side} the {name} region, the first at offset {int(hit[0])}"
        # and the results are those of plain buffers
        loss0, grad0 = raw_loss(r, gt, m, case.lam)
        assert torch.equal(loss, loss0) and torch.equal(grad.cpu(), grad0.cpu())


def check_determinism(dev, H, W, runs):
    case = get("textured", "textured", H, W)
    r, gt, m = _on(dev, case)
    first = None
    for _ in range(runs):
        loss, grad = raw_loss(r, gt, m, case.lam)
        res = (loss.cpu(), grad.cpu())
        if first is None:
            first = res
        assert torch.equal(res[0], first[0]) and torch.equal(res[1], first[1])


def check_upstream_gradient(dev):
    """the stored gradient times the upstream gradient -- handed on unchanged, whatever the upstream gradient, with is_root=True"""
    case = get("textured", "textured+soft", 45, 70)
    r, gt, m = _on(dev, case)

    def grad_of(scale, is_root):
        x = r.clone().requires_grad_(True)
        out = loss_utils.fused_l1_ssim_loss(x, gt, m, case.lam, is_root)
        (g,) = torch.autograd.grad(out * scale if scale is not None else out, x)
        return g

    plain = grad_of(None, False)
    assert bool(plain.any())
    assert torch.equal(grad_of(3.0, False), plain * 3.0)
    assert torch.equal(grad_of(None, True), plain)
    assert torch.equal(grad_of(3.0, True), plain)


def check_cpp_host(ops, dev):
    """ops.l1_ssim_loss of the C++ host and the Python wrapper sit on the same C entry point: the same bits"""
    for case in [get("textured", "textured+binary", 45, 70), get("flat", "flat0.97s0.001", 40, 72), get("noise", "noise", 33, 31)]:
        r, gt, m = _on(dev, case)
        x = r.clone().requires_grad_(True)
        out = loss_utils.fused_l1_ssim_loss(x, gt, m, case.lam)
        (g,) = torch.autograd.grad(out, x)
        y = r.clone().requires_grad_(True)
        out2 = ops.l1_ssim_loss(y, gt, m if m is not None else torch.empty(0, device=dev), case.lam)
        (g2,) = torch.autograd.grad(out2, y)
        assert torch.equal(out2.detach(), out.detach()) and torch.equal(g2, g), (case, out.item(), out2.item(), float((g - g2).abs().max()))


# ------------------------------------------------------------------------------------------------------------------------ Adam
B1, B2, EPS = 0.9, 0.999, 1e-15
ADAM_STEPS = 3
ADAM_NS = [1, 2, 3, 5, 1023, 1024, 1025, 4099]
ADAM_PERIODS = [(3, 3), (12, 3), (27, 3), (48, 3)]     # SH degree 0, 1, 2, 3: [P, (d+1)^2, 3] rows, features_dc = the first 3


def adam_inputs(n, tag=""):
    g = _gen("adam", n, tag)
    p = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * (10.0 ** -k) for k in range(ADAM_STEPS)]   # (gradients of falling size: v remembers)
    return p, grads


def adam64(p, grads, lr):
    """Adam in float64 on the float32 inputs (numpy); lr: a scalar or one learning rate per element.  Returns p, m, v."""
    p = p.numpy().astype(np.float64)
    lr = np.asarray(lr, np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    for t, g in enumerate(grads, 1):
        g = g.numpy().astype(np.float64)
        m = B1 * m + (1.0 - B1) * g
        v = B2 * v + (1.0 - B2) * g * g
        p = p - (lr / (1.0 - B1 ** t)) * m / (np.sqrt(v) / math.sqrt(1.0 - B2 ** t) + EPS)
    return p, m, v


def adam_torch(p, grads, lr):
    """torch.optim.Adam in float32 on the CPU -- the yardstick; lr: a scalar, or [(index tensor, lr)] for separate groups"""
    groups = lr if isinstance(lr, list) else [(torch.arange(p.numel()), lr)]
    leaves = [p[idx].clone().requires_grad_(True) for idx, _ in groups]
    opt = torch.optim.Adam([dict(params=[x], lr=l) for x, (_, l) in zip(leaves, groups)], betas=(B1, B2), eps=EPS)
    for g in grads:
        for x, (idx, _) in zip(leaves, groups):
            x.grad = g[idx].clone()
        opt.step()
    out = p.clone()
    for x, (idx, _) in zip(leaves, groups):
        out[idx] = x.detach()
    return out.numpy().astype(np.float64)


def adam_kernel(dev, p, grads, lr, period=0, split=0, lr_tail=None, misalign=None):
    """gsr_adam_step, ADAM_STEPS times; misalign: the index (param, grad, exp_avg, exp_avg_sq) of the pointer that sits one float
    past a 16-byte boundary.  Returns p, m, v (CPU tensors)."""
    lib = _lib()
    place = lambda t, k: misaligned(t.to(dev)) if misalign == k else t.to(dev).clone()
    pp, m, v = place(p, 0), place(torch.zeros_like(p), 2), place(torch.zeros_like(p), 3)
    for k, t in enumerate((pp, None, m, v)):
        assert t is None or (t.data_ptr() % 16 == 0) == (misalign != k)
    for step, g in enumerate(grads, 1):
        gg = place(g, 1)
        capi.check(lib, lib.gsr_adam_step(pp.data_ptr(), gg.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), float(lr), B1, B2, EPS,
                                          step, period, split, float(lr if lr_tail is None else lr_tail), rp._stream_ptr(pp)),
                   "gsr_adam_step")
    return pp.cpu(), m.cpu(), v.cpu()


def _ulp(x):
    return float(np.spacing(np.float32(np.abs(x).max())))


def assert_adam(what, got, p64, m64, v64, p32, grads):
    """The parameter: max error against float64 <= 2 x that of torch.optim.Adam in float32 + one float32 ulp of the (largest)
    parameter -- the same recurrence.  The moments: 3 steps of at most 3 roundings (1.5 ulp) + the float32 betas (0.5 ulp) each, in
    units of the largest term that enters them: 6 ulps of max |g| and of max g^2."""
    p, m, v = (t.numpy().astype(np.float64) for t in got)
    e, b = np.abs(p - p64).max(), np.abs(p32 - p64).max()
    assert e <= 2.0 * b + _ulp(p64), (what, "param", e, b, _ulp(p64), int(np.abs(p - p64).argmax()))
    gmax = max(float(g.abs().max()) for g in grads)
    assert np.abs(m - m64).max() <= 6 * _ulp(np.float64(gmax)), (what, "exp_avg", np.abs(m - m64).max(), int(np.abs(m - m64).argmax()))
    assert np.abs(v - v64).max() <= 6 * _ulp(np.float64(gmax * gmax)), (what, "exp_avg_sq", np.abs(v - v64).max(), int(np.abs(v - v64).argmax()))


def check_adam_sizes(dev):
    """the vector body, the scalar tail (n % 4 != 0), n < 4, and one workgroup more than full ones"""
    for n in ADAM_NS:
        p, grads = adam_inputs(n)
        p64, m64, v64 = adam64(p, grads, 1e-2)
        assert_adam(f"n={n}", adam_kernel(dev, p, grads, 1e-2), p64, m64, v64, adam_torch(p, grads, 1e-2), grads)


def check_adam_misaligned(dev):
    """each pointer in turn one float past a 16-byte boundary: the scalar path over the whole tensor, the vector path's bits"""
    for n in (1025, 4099):
        p, grads = adam_inputs(n)
        p64, m64, v64 = adam64(p, grads, 1e-2)
        p32 = adam_torch(p, grads, 1e-2)
        aligned = adam_kernel(dev, p, grads, 1e-2)
        for k, name in enumerate(("param", "grad", "exp_avg", "exp_avg_sq")):
            got = adam_kernel(dev, p, grads, 1e-2, misalign=k)
            assert_adam(f"n={n}, {name} misaligned", got, p64, m64, v64, p32, grads)
            for a, b in zip(got, aligned):
                assert torch.equal(a, b), (n, name)


def check_adam_periods(dev):
    """[split, period) of every period-element row steps with lr_tail: head and tail against two plain Adam groups"""
    lr, lr_tail = 2e-3, 1e-4
    for period, split in ADAM_PERIODS:
        n = 257 * period
        p, grads = adam_inputs(n, period)
        col = torch.arange(n) % period
        head, tail = torch.nonzero(col < split).flatten(), torch.nonzero(col >= split).flatten()
        assert head.numel() == 257 * split and tail.numel() == 257 * (period - split)
        lrs = np.where(col.numpy() < split, lr, lr_tail)
        p64, m64, v64 = adam64(p, grads, lrs)
        p32 = adam_torch(p, grads, [(head, lr), (tail, lr_tail)] if tail.numel() else [(head, lr)])
        got = adam_kernel(dev, p, grads, lr, period=period, split=split, lr_tail=lr_tail)
        for name, idx in (("head", head), ("tail", tail)):
            if idx.numel():
                i = idx.numpy()
                assert_adam(f"period={period}, {name}", [t[idx] for t in got], p64[i], m64[i], v64[i], p32[i], [g[idx] for g in grads])
        # the two learning rates are told apart: the tail moved 20 times less than the head
        if tail.numel():
            moved = (got[0] - p).abs()
            assert float(moved[tail].median()) < 0.1 * float(moved[head].median())


def check_adam_multi(dev):
    """gsr_adam_step_multi == gsr_adam_step per tensor, bit for bit (the code promises it: adam_update), for the sizes of
    ADAM_NS as the tensors of one launch with an empty tensor (n = 0, null pointers) among them.  A launch takes at most 8
    tensors, the empty one included: two launches."""
    lib = _lib()
    for ns in ([1, 2, 0, 3, 5, 1023], [1024, 0, 1025, 4099]):
        arr = (capi.AdamMultiTensor * len(ns))()
        keep, want = [], []
        for k, n in enumerate(ns):
            if n == 0:
                arr[k] = capi.AdamMultiTensor(None, None, None, None, 0, 1e-2, 1, 0.0)
                continue
            p, grads = adam_inputs(n, "multi")
            lr, step = 1e-2 / (k + 1), k + 1
            m0, v0 = 0.1 * grads[1], grads[2] ** 2 + 1e-6
            one = [p.to(dev).clone(), m0.to(dev).clone(), v0.to(dev).clone()]
            g = grads[0].to(dev)
            capi.check(lib, lib.gsr_adam_step(one[0].data_ptr(), g.data_ptr(), one[1].data_ptr(), one[2].data_ptr(), n, lr, B1, B2, EPS,
                                              step, 0, 0, lr, rp._stream_ptr(g)), "gsr_adam_step")
            multi = [p.to(dev).clone(), m0.to(dev).clone(), v0.to(dev).clone()]
            arr[k] = capi.AdamMultiTensor(multi[0].data_ptr(), g.data_ptr(), multi[1].data_ptr(), multi[2].data_ptr(), n, lr, step, 0.0)
            keep.append((g, multi))
            want.append((n, one, multi, p))
        capi.check(lib, lib.gsr_adam_step_multi(len(ns), arr, B1, B2, EPS, rp._stream_ptr(keep[0][0])), "gsr_adam_step_multi")
        for n, one, multi, p in want:
            for a, b, name in zip(one, multi, ("param", "exp_avg", "exp_avg_sq")):
                assert torch.equal(a, b), (n, name)
            assert not torch.equal(multi[0].cpu(), p)


# ------------------------------------------------------------------------------------------------------------------ depth loss
def check_depth_loss64(dev, H, W, seed=0, w=0.7, lo=0.1, hi=5.0):
    """gsr_depth_l1_loss against a float64 sum: the loss to 1e-6 relative, the gradient's zero pattern exactly and its values to
    1e-6 relative, the same bits from a second run"""
    rng = np.random.default_rng(seed)
    gt = rng.uniform(0.0, 6.0, (H, W)).astype(np.float32)
    if H * W <= 8:
        gt = np.clip(gt, 1.0, 4.0)                    # (valid, whatever the draw)
    depth = gt + rng.standard_normal((H, W)).astype(np.float32)
    if H * W > 8:
        gt.flat[0:3] = [lo, hi, 0.0]                  # on the bounds, and 0: invalid
        depth.flat[3:6] = gt.flat[3:6]                # D == gt: sign 0
    valid = (gt > np.float32(lo)) & (gt < np.float32(hi))
    diff = depth.astype(np.float64) - gt.astype(np.float64)
    ref_loss = w * np.abs(diff)[valid].sum() / (H * W)
    ref_grad = np.where(valid, np.sign(diff), 0.0) * (w / (H * W))
    d_t = torch.from_numpy(depth).to(dev).requires_grad_(True)
    gt_t = torch.from_numpy(gt).to(dev)
    loss = loss_utils.depth_l1_loss(d_t, gt_t, w, lo, hi)
    (grad,) = torch.autograd.grad(loss, d_t)
    grad = grad.cpu().numpy().astype(np.float64)
    assert abs(loss.item() - ref_loss) <= 1e-6 * abs(ref_loss), (H, W, loss.item(), ref_loss)
    assert np.array_equal(grad == 0, ref_grad == 0)
    assert np.allclose(grad, ref_grad, rtol=1e-6, atol=0), float(np.abs(grad - ref_grad).max())
    assert valid.any() and (H * W <= 8 or (grad.flat[0:6] == 0).all())
    loss2 = loss_utils.depth_l1_loss(d_t.detach(), gt_t, w, lo, hi)
    assert loss2.item() == loss.item()
    return loss.item(), ref_loss
