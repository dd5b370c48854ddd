"""Per-keyframe exposure compensation (gsr_l1_ssim_loss_exposure, gsr_apply_exposure, TrainStep.optimize_exposure_) against float64
references.  Shared by test_exposure.py (emulator build) and test_gpu_exposure.py (MI355X).

The map (include/gsr.h): x_c = (r_0 E[0][c] + r_1 E[1][c] + r_2 E[2][c] + E[c][3]) m_c, the loss of loss_cases on x.  References are
torch autograd on the CPU of x = einsum("khw,kc->chw", r, E[:, :3]) + E[:, 3] behind loss_cases' own loss expression: float64 is
the truth, the same expression in float32 the yardstick.  Per case
    E_L = |loss - loss64|,  E_G = 3 H W max |grad_rendered - grad64|,  E_X = max over the 12 entries |grad_exposure - f64|
and B_L, B_G, B_X the same for float32 ATen; per content class and map
    max E_L <= 2 max B_L + 2^-22,   max E_G <= 2 max B_G + 2^-20,   max E_X <= 2 max B_X + 2^-20
(loss_cases' bars; the floor of E_X: sixteen float32 ulps of sums of magnitude <= 1)."""
import math

import numpy as np
import torch

import loss_cases as lc
from photo_slam_amd import capi, loss_utils
from photo_slam_amd import rasterize_points as rp

FLOOR_L, FLOOR_G, FLOOR_X = 2.0 ** -22, 2.0 ** -20, 2.0 ** -20
MAPS = {
    "gain": [[1.25, 0.0, 0.0, -0.04], [0.0, 0.8, 0.0, 0.03], [0.0, 0.0, 1.1, 0.01]],
    "mixing": [[0.9, 0.08, -0.03, 0.02], [0.05, 1.1, 0.04, -0.03], [-0.02, 0.06, 0.85, 0.05]],
}
EXTRA_TEXTURED = [(1, 1), (5, 33), (33, 31), (40, 73), (40, 75), (8, 93), (97, 132)]
BRANCH_CLASSES = ["textured", "flat"]          # lambda = 0 and lambda = 1, at 45 x 70


def exposure(name, dev="cpu"):
    return torch.tensor(MAPS[name], dtype=torch.float32, device=dev)


def identity(dev="cpu"):
    return torch.eye(3, 4, dtype=torch.float32, device=dev)


def map64(r, E):
    """the map in the dtype of its arguments (the expression of the issue)"""
    return torch.einsum("khw,kc->chw", r, E[:, :3]) + E[:, 3].view(3, 1, 1)


def group(cls, lam=lc.LAM):
    """the cases of one content class: loss_cases.group at FULL_SIZES (with the masks it has there), `textured` at EXTRA_TEXTURED
    as well; at lambda = 0 and 1 every content variant at 45 x 70"""
    cases = [c for c in lc.group(cls, lam) if (c.H, c.W) in lc.FULL_SIZES]
    if cls == "textured" and lam == lc.LAM:
        cases += [lc.get("textured", "textured", H, W, lam) for (H, W) in EXTRA_TEXTURED]
    return cases


# ---------------------------------------------------------------------------------------------------------------- references
def reference(case, E, dtype):
    """(loss, grad_rendered, grad_exposure) of the ATen expression in `dtype` on the CPU, returned in float64"""
    r = case.rendered.detach().cpu().to(dtype).requires_grad_(True)
    e = E.detach().cpu().to(dtype).requires_grad_(True)
    gt = case.gt.detach().cpu().to(dtype)
    with torch.enable_grad():
        x = map64(r, e)
        xm = x if case.mask is None else x * case.mask.detach().cpu().to(dtype)
        loss = (1.0 - case.lam) * loss_utils.l1_loss(xm, gt) + case.lam * (1.0 - loss_utils.ssim(xm.unsqueeze(0), gt.unsqueeze(0)))
        gr, ge = torch.autograd.grad(loss, (r, e))
    assert loss.dtype == dtype and gr.dtype == dtype and ge.dtype == dtype
    return float(loss.detach().double()), gr.detach().double(), ge.detach().double()


_refs = {}


def references(case, map_name):
    key = (id(case), map_name)
    if key not in _refs:
        E = exposure(map_name)
        _refs[key] = (case, reference(case, E, torch.float64), reference(case, E, torch.float32))
    return _refs[key][1:]


def run_fused(dev, case, E):
    """(loss, grad_rendered, grad_exposure) of the fused kernels through the Python wrapper, in float64 on the CPU"""
    r = case.rendered.to(dev).requires_grad_(True)
    e = E.to(dev).requires_grad_(True)
    mask = None if case.mask is None else case.mask.to(dev)
    out = loss_utils.fused_l1_ssim_loss(r, case.gt.to(dev), mask, case.lam, exposure=e)
    gr, ge = torch.autograd.grad(out, (r, e))
    return out.detach().cpu().double().item(), gr.detach().cpu().double(), ge.detach().cpu().double()


def measure(dev, case, map_name):
    (l64, g64, x64), (l32, g32, x32) = references(case, map_name)
    loss, grad, gexp = run_fused(dev, case, exposure(map_name))
    assert math.isfinite(loss) and bool(torch.isfinite(grad).all()) and bool(torch.isfinite(gexp).all()), f"{case}: NaN or Inf"
    n = 3 * case.H * case.W
    eg = (grad - g64).abs()
    return dict(case=case, E_L=abs(loss - l64), B_L=abs(l32 - l64), E_G=n * float(eg.max()), B_G=n * float((g32 - g64).abs().max()),
                E_X=float((gexp - x64).abs().max()), B_X=float((x32 - x64).abs().max()), dE=float(x64.abs().max()),
                worst=lc.worst_pixel(eg))


def check_rows(rows, what):
    wl, wg, wx = (max(rows, key=lambda r: r[k]) for k in ("E_L", "E_G", "E_X"))
    EL, EG, EX = wl["E_L"], wg["E_G"], wx["E_X"]
    BL, BG, BX = (max(r[k] for r in rows) for k in ("B_L", "B_G", "B_X"))
    print(f"EXPOSURE {what} cases={len(rows)} E_L={EL:.3g} B_L={BL:.3g} E_G={EG:.3g} B_G={BG:.3g} E_X={EX:.3g} B_X={BX:.3g} "
          f"max|dE|={max(r['dE'] for r in rows):.3g} worst_grad={wg['case']} {wg['worst']} worst_dE={wx['case']}")
    failures = []
    if not EL <= 2.0 * BL + FLOOR_L:
        failures.append(f"loss: {EL:.4g} at {wl['case']} > 2 x {BL:.4g} + {FLOOR_L:.3g}")
    if not EG <= 2.0 * BG + FLOOR_G:
        failures.append(f"grad_rendered: 3HW max = {EG:.4g} at {wg['case']} {wg['worst']} > 2 x {BG:.4g} + {FLOOR_G:.3g}")
    if not EX <= 2.0 * BX + FLOOR_X:
        failures.append(f"grad_exposure: {EX:.4g} at {wx['case']} > 2 x {BX:.4g} + {FLOOR_X:.3g}")
    assert not failures, what + ": " + "; ".join(failures)


def check_group(dev, cls, map_name, lam=lc.LAM, tag=""):
    check_rows([measure(dev, c, map_name) for c in group(cls, lam)], f"{tag} {cls} map={map_name} lambda={lam:g}")


def check_full_hd(dev, map_name):
    """1080 x 1920: the grid of the mix pass is capped, every thread of it walks several pixels"""
    case = lc.Case("textured", "textured", lc.LAM, *lc.content("textured", 1080, 1920)[0][1:], None)
    check_rows([measure(dev, case, map_name)], f"gpu textured 1080x1920 map={map_name}")


# ------------------------------------------------------------------------------------------------- the C ABI with own buffers
def _lib():
    return rp._lib()


def raw_exposure_loss(r, gt, mask, lam, E, grad=None, grad_e=None, scratch=None):
    """gsr_l1_ssim_loss_exposure on the caller's tensors.  Returns (loss [1], grad_rendered, grad_exposure [12])."""
    lib = _lib()
    _, H, W = r.shape
    for t in (r, gt, mask, E):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous())
    nb = int(lib.gsr_loss_exposure_scratch_bytes(W, H))
    assert nb >= int(lib.gsr_loss_scratch_bytes(W, H)) + 4 * 4 * 3 * ((W + 31) // 32) * ((H + 31) // 32)
    if grad is None:
        grad = torch.empty(3 * H * W, dtype=torch.float32, device=r.device)
    if grad_e is None:
        grad_e = torch.full((12,), float("nan"), dtype=torch.float32, device=r.device)
    if scratch is None:
        scratch = torch.empty(nb, dtype=torch.uint8, device=r.device)
    assert grad.numel() >= 3 * H * W and grad_e.numel() == 12 and scratch.numel() >= nb and scratch.data_ptr() % 16 == 0
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device=r.device)
    lc.misaligned_vector_loads(lib)
    capi.check(lib, lib.gsr_l1_ssim_loss_exposure(r.data_ptr(), gt.data_ptr(), None if mask is None else mask.data_ptr(), W, H,
                                                  float(lam), E.data_ptr(), grad.data_ptr(), grad_e.data_ptr(), loss.data_ptr(),
                                                  scratch.data_ptr(), rp._stream_ptr(r)), "gsr_l1_ssim_loss_exposure")
    assert lc.misaligned_vector_loads(lib) == 0, "the vector staging path ran on a plane that is not 16-byte aligned"
    return loss, grad, grad_e


def _same(a, b, what):
    for x, y, name in zip(a, b, ("loss", "grad_rendered", "grad_exposure")):
        assert torch.equal(x.cpu(), y.cpu()), f"{what}: {name} differs by {float((x.cpu() - y.cpu()).abs().max()):.3g}"


def check_identity(dev):
    """E = eye(3,4): loss and grad_rendered are gsr_l1_ssim_loss's bit for bit (r 1 + g 0 + b 0 + 0 is exact)"""
    E = identity(dev)
    for (H, W, mis) in ((45, 70, False), (40, 72, False), (40, 72, True)):
        for kind in (None, "binary", "soft"):
            case = lc.get("textured", "textured" if kind is None else f"textured+{kind}", H, W)
            r, gt, m = lc._on(dev, case)
            if mis:
                r, gt, m = lc.misaligned(r), lc.misaligned(gt), None if m is None else lc.misaligned(m)
            loss0, grad0 = lc.raw_loss(r, gt, m, case.lam)
            loss1, grad1, ge = raw_exposure_loss(r, gt, m, case.lam, E)
            _same((loss1, grad1), (loss0, grad0), f"{case} misaligned={mis}")
            assert bool(torch.isfinite(ge).all()) and bool(ge.any())


def check_scalar_staging(dev):
    """a plane one float past a 16-byte boundary takes the scalar staging path: the same bits in all three results"""
    E = exposure("mixing", dev)
    for case in lc.staging_cases():
        r, gt, m = lc._on(dev, case)
        base = raw_exposure_loss(r, gt, m, case.lam, E)
        planes = dict(rendered=r, gt=gt, mask=m)
        names = [k for k, t in planes.items() if t is not None]
        for which in [(k,) for k in names] + [tuple(names)]:
            r1, g1, m1 = (lc.misaligned(t) if k in which else t for k, t in planes.items())
            _same(raw_exposure_loss(r1, g1, m1, case.lam, E), base, f"{case}, {which} misaligned")


def check_poisoned_buffers(dev):
    lib = _lib()
    E = exposure("mixing", dev)
    for case in [lc.get("textured", "textured", 33, 31), lc.get("textured", "textured+binary", 40, 72), lc.get("textured", "textured", 40, 75),
                 lc.get("textured", "textured", 1, 1)]:
        r, gt, m = lc._on(dev, case)
        nb, n = int(lib.gsr_loss_exposure_scratch_bytes(case.W, case.H)), 3 * case.H * case.W
        assert nb % 4 == 0
        res = []
        for fill in (0.0, float("nan")):
            scratch = torch.full((nb // 4,), fill, dtype=torch.float32, device=dev)
            out = raw_exposure_loss(r, gt, m, case.lam, E, grad=torch.full((n,), fill, dtype=torch.float32, device=dev),
                                    grad_e=torch.full((12,), fill, dtype=torch.float32, device=dev), scratch=scratch.view(torch.uint8))
            res.append([t.cpu() for t in out])
        assert not any(bool(torch.isnan(t).any()) for t in res[1]), case
        _same(res[1], res[0], f"{case} poisoned")


def check_guard_bands(dev, sizes=((1, 1), (33, 31), (40, 75))):
    """4096 bytes of a byte pattern on either side of the scratch region, grad_rendered and the 12 floats of grad_exposure"""
    lib = _lib()
    pad = 4 * lc.GUARD_FLOATS
    E = exposure("mixing", dev)
    for (H, W) in sizes:
        case = lc.get("textured", "textured", H, W)
        r, gt, m = lc._on(dev, case)
        nb, n = int(lib.gsr_loss_exposure_scratch_bytes(W, H)), 3 * H * W
        bufs = {name: torch.full((pad + size + pad,), lc.GUARD_BYTE, dtype=torch.uint8, device=dev)
                for name, size in (("scratch", nb), ("grad_rendered", 4 * n), ("grad_exposure", 48))}
        inner = lambda name, size: bufs[name][pad:pad + size]
        out = raw_exposure_loss(r, gt, m, case.lam, E, grad=inner("grad_rendered", 4 * n).view(torch.float32),
                                grad_e=inner("grad_exposure", 48).view(torch.float32), scratch=inner("scratch", nb))
        for name, size in (("scratch", nb), ("grad_rendered", 4 * n), ("grad_exposure", 48)):
            buf = bufs[name].cpu()
            for side, band in (("before", buf[:pad]), ("after", buf[pad + size:])):
                hit = torch.nonzero(band != lc.GUARD_BYTE).flatten()
                assert hit.numel() == 0, f"{H}x{W}: {hit.numel()} bytes written {side} the {name} region, the first at offset {int(hit[0])}"
        _same(out, raw_exposure_loss(r, gt, m, case.lam, E), f"{H}x{W} guarded buffers")


def check_determinism(dev, H, W, runs):
    case = lc.get("textured", "textured", H, W)
    r, gt, m = lc._on(dev, case)
    E = exposure("mixing", dev)
    first = None
    for _ in range(runs):
        res = [t.cpu() for t in raw_exposure_loss(r, gt, m, case.lam, E)]
        first = first or res
        _same(res, first, f"{H}x{W} rerun")


def check_upstream_gradient(dev):
    """both gradients times the upstream gradient -- handed on unchanged, whatever it is, with is_root=True"""
    case = lc.get("textured", "textured+soft", 45, 70)
    r, gt, m = lc._on(dev, case)
    E = exposure("gain", dev)

    def grads_of(scale, is_root):
        x, e = r.clone().requires_grad_(True), E.clone().requires_grad_(True)
        out = loss_utils.fused_l1_ssim_loss(x, gt, m, case.lam, is_root, exposure=e)
        return torch.autograd.grad(out * scale if scale is not None else out, (x, e))

    plain = grads_of(None, False)
    assert bool(plain[0].any()) and bool(plain[1].any()) and plain[1].shape == (3, 4)
    for got, want in ((grads_of(3.0, False), [g * 3.0 for g in plain]), (grads_of(None, True), plain), (grads_of(3.0, True), plain)):
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def check_cpp_host(ops, dev):
    """ops.l1_ssim_loss_exposure / ops.apply_exposure of the C++ host and the Python wrappers: the same bits"""
    E = exposure("mixing", dev)
    for case in [lc.get("textured", "textured+binary", 45, 70), lc.get("flat", "flat0.97s0.001", 40, 72), lc.get("noise", "noise", 33, 31)]:
        r, gt, m = lc._on(dev, case)
        x, e = r.clone().requires_grad_(True), E.clone().requires_grad_(True)
        out = loss_utils.fused_l1_ssim_loss(x, gt, m, case.lam, exposure=e)
        g = torch.autograd.grad(out, (x, e))
        y, f = r.clone().requires_grad_(True), E.clone().requires_grad_(True)
        out2 = ops.l1_ssim_loss_exposure(y, gt, m if m is not None else torch.empty(0, device=dev), case.lam, f, False)
        g2 = torch.autograd.grad(out2, (y, f))
        assert torch.equal(out2.detach(), out.detach()) and torch.equal(g2[0], g[0]) and torch.equal(g2[1], g[1]), case
        assert torch.equal(ops.apply_exposure(r, E), loss_utils.apply_exposure(r, E))


# ----------------------------------------------------------------------------------------------------------- gsr_apply_exposure
def check_apply(dev):
    """the float64 expression to 4 ulps of the largest |x|; in place through the C entry point"""
    lib = _lib()
    for name in MAPS:
        E = exposure(name, dev)
        for (H, W) in ((1, 1), (33, 31), (40, 75), (97, 132)):
            r = lc.content("range", H, W)[0][1].to(dev).contiguous()
            want = map64(r.cpu().double(), E.cpu().double())
            tol = 4.0 * float(np.spacing(np.float32(want.abs().max())))
            got = loss_utils.apply_exposure(r, E)
            assert got.shape == r.shape and float((got.cpu().double() - want).abs().max()) <= tol, (name, H, W)
            buf = r.clone()
            capi.check(lib, lib.gsr_apply_exposure(buf.data_ptr(), E.data_ptr(), W, H, buf.data_ptr(), rp._stream_ptr(buf)), "gsr_apply_exposure")
            assert torch.equal(buf, got), (name, H, W, "in place")
    eye_in = lc.textured(40, 75).to(dev)
    assert torch.equal(loss_utils.apply_exposure(eye_in, identity(dev)), eye_in)


# ------------------------------------------------------------------------------------------------ convergence at the loss level
CONV_STEPS, CONV_LR0, CONV_LR1, CONV_LAM = 200, 0.01, 0.001, 0.2
CONV_START_ERROR = 0.15      # max |eye(3,4) - mixing map|


def _conv_lr(k):
    t = k / float(CONV_STEPS)
    return math.exp(math.log(CONV_LR0) * (1.0 - t) + math.log(CONV_LR1) * t)


def _adam_loop(E, grad_fn):
    """CONV_STEPS Adam steps (betas 0.9 / 0.999, eps 1e-15) on E in its own dtype, gradients from grad_fn(E)"""
    m, v = torch.zeros_like(E), torch.zeros_like(E)
    for k in range(1, CONV_STEPS + 1):
        g = grad_fn(E)
        m = 0.9 * m + 0.1 * g
        v = 0.999 * v + 0.001 * g * g
        E = E - (_conv_lr(k) / (1.0 - 0.9 ** k)) * m / (v.sqrt() / math.sqrt(1.0 - 0.999 ** k) + 1e-15)
    return E


def check_convergence(dev):
    """R = textured + noise, gt = the mixing map of R: from the identity, Adam through the fused loss recovers the map to
    max(2 x the float64 loop's final error, a tenth of the initial 0.15); the float64 loop itself ends below the tenth"""
    H, W = 64, 96
    R = lc.textured(H, W) + 0.05 * torch.randn(3, H, W, generator=torch.Generator().manual_seed(1))
    E_true = exposure("mixing")
    assert abs(float((identity() - E_true).abs().max()) - CONV_START_ERROR) < 1e-6
    gt = map64(R.double(), E_true.double()).float()

    def grad64(E):
        e = E.detach().requires_grad_(True)
        x = map64(R.double(), e)
        g = gt.double()
        with torch.enable_grad():
            loss = (1.0 - CONV_LAM) * loss_utils.l1_loss(x, g) + CONV_LAM * (1.0 - loss_utils.ssim(x.unsqueeze(0), g.unsqueeze(0)))
        return torch.autograd.grad(loss, e)[0]

    ref_err = float((_adam_loop(identity().double(), grad64) - E_true.double()).abs().max())
    assert ref_err <= CONV_START_ERROR / 10, ("the float64 loop does not converge", ref_err)
    Rd, gtd = R.to(dev), gt.to(dev)

    def grad_fused(E):
        e = E.detach().requires_grad_(True)
        return torch.autograd.grad(loss_utils.fused_l1_ssim_loss(Rd, gtd, None, CONV_LAM, exposure=e), e)[0]

    err = float((_adam_loop(identity(dev), grad_fused).cpu() - E_true).abs().max())
    bound = max(2.0 * ref_err, CONV_START_ERROR / 10)
    print(f"EXPOSURE convergence: float64 loop {ref_err:.3g}, fused loop {err:.3g}, bound {bound:.3g}")
    assert err <= bound, (err, ref_err, bound)


# ---------------------------------------------------------------------------------------------------------- TrainStep, both hosts
import pose_grad_cases as pg   # noqa: E402
from photo_slam_amd import scene   # noqa: E402

TRAIN_LAM = 0.2
TRAIN_LR_STEPS = 10          # exposure_lr_max_steps_: the schedule moves visibly within the keyframes' two steps
ADAM_TOL = 2.0 ** -20        # eight float32 ulps of 1.25 over three steps


def train_scene():
    """REFINE_SCENE with three views: keyframes A and B are trained on, C carries an exposure and is never used"""
    return scene.make_cloud(**dict(pg.REFINE_SCENE, n_views=3))


def _targets(render, cams, dev):
    """per keyframe the model's own render behind a per-keyframe gain/offset: something for the exposures to learn"""
    out = []
    for k, cam in enumerate(cams):
        img = render(cam).clone()
        E = exposure("gain", dev).clone()
        E[:, :3] *= 1.0 - 0.1 * k
        out.append(loss_utils.apply_exposure(img, E).clone())
    return out


def lr_schedule(step, lr0=0.01, lr1=0.001, max_steps=TRAIN_LR_STEPS):
    t = min(max(step / float(max_steps), 0.0), 1.0)
    return math.exp(math.log(lr0) * (1.0 - t) + math.log(lr1) * t)


def adam_replay64(E0, grads, lrs):
    """float64 Adam (betas 0.9 / 0.999, eps 1e-15) on E0 with the given gradients and learning rates, one step each"""
    p = E0.double().cpu().clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for k, (g, lr) in enumerate(zip(grads, lrs), 1):
        g = g.double().cpu()
        m = 0.9 * m + 0.1 * g
        v = 0.999 * v + 0.001 * g * g
        p = p - (lr / (1.0 - 0.9 ** k)) * m / (v.sqrt() / math.sqrt(1.0 - 0.999 ** k) + 1e-15)
    return p


def _expected(img, gt, mask, E):
    """the fused loss with exposure E on a forward-only render, and the library's own grad_exposure"""
    e = E.detach().clone().requires_grad_(True)
    loss = loss_utils.fused_l1_ssim_loss(img, gt, mask, TRAIN_LAM, exposure=e)
    return loss.detach(), torch.autograd.grad(loss, e)[0]


def _check_replay(name, E_final, E0, grads, steps_taken):
    assert steps_taken == len(grads), (name, steps_taken, len(grads))
    want = adam_replay64(E0, grads, [lr_schedule(k) for k in range(1, len(grads) + 1)])
    err = float((E_final.cpu().double() - want).abs().max())
    moved = float((E_final.cpu() - E0.cpu()).abs().max())
    print(f"EXPOSURE keyframe {name}: {len(grads)} steps, |E - replay| = {err:.3g}, moved {moved:.3g}")
    assert moved >= 1e-3, (name, "the exposure did not move")
    assert err <= ADAM_TOL, (name, err)


def python_trainer(cl, dev, optimize=True, lr=None):
    g, ts = pg.python_trainer(cl, dev)
    ts.opt_.lambda_dssim_ = TRAIN_LAM
    ts.optimize_exposure_ = optimize
    ts.exposure_lr_max_steps_ = TRAIN_LR_STEPS
    if lr is not None:
        ts.exposure_lr_init_ = ts.exposure_lr_final_ = lr
    return g, ts


def check_train_python(lib_path, dev):
    """(a) on the Python host: iterations over A, B, A"""
    from photo_slam_amd.gaussian_renderer import GaussianKeyframe
    cl = train_scene()
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        g, ts = python_trainer(cl, dev)
        kfs = [GaussianKeyframe.from_camera(c, dev) for c in cl.cameras]
        gts = _targets(ts.render_view, kfs, dev)
        mask = torch.ones_like(gts[0])
        unused = exposure("mixing", dev)
        kfs[2].exposure_ = unused.clone()
        grads, start = {0: [], 1: []}, {}
        for k in (0, 1, 0):
            kf = kfs[k]
            E = identity(dev) if kf.exposure_ is None else kf.exposure_.clone()
            start.setdefault(k, E)
            img = ts.render_view(kf)
            assert torch.equal(ts.render_view(kf, apply_exposure=True), loss_utils.apply_exposure(img, E))
            want, ge = _expected(img, gts[k], None, E)
            loss = ts.trainForOneIteration(kf, gts[k], mask, sync_loss=False)
            assert torch.equal(loss.detach(), want), (k, float(loss), float(want))
            grads[k].append(ge)
        for k, name in ((0, "A"), (1, "B")):
            _check_replay(name, kfs[k].exposure_, start[k], grads[k], kfs[k].exposure_step_)
        assert torch.equal(kfs[2].exposure_, unused) and kfs[2].exposure_step_ == 0 and kfs[2].exposure_exp_avg_ is None
        assert abs(ts.exposureLearningRate(1) - lr_schedule(1)) <= 1e-6 * lr_schedule(1)
    finally:
        rp._LIB_OVERRIDE = prev


def _py_state(g):
    o = g.optimizer_
    t = [p.detach().clone() for p in g.params_raw()]
    for p in g.params_raw():
        st = o.state.get(id(p), {})
        t += [v.clone() for k, v in sorted(st.items()) if torch.is_tensor(v)]
    return t


def check_identity_train_python(lib_path, dev):
    """(b): identity exposures at learning rate 0 against no exposures: the same model, moments and row_step bit for bit"""
    from photo_slam_amd.gaussian_renderer import GaussianKeyframe
    cl = train_scene()
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        states = []
        gts = None
        for with_exposure in (False, True):
            g, ts = python_trainer(cl, dev, optimize=with_exposure, lr=0.0)
            kfs = [GaussianKeyframe.from_camera(c, dev) for c in cl.cameras]
            if gts is None:
                gts = _targets(ts.render_view, kfs, dev)
            mask = torch.ones_like(gts[0])
            losses = [ts.trainForOneIteration(kfs[k], gts[k], mask, sync_loss=False).detach().clone() for k in (0, 1, 0)]
            if with_exposure:
                assert all(torch.equal(kfs[k].exposure_, identity(dev)) for k in (0, 1)) and kfs[0].exposure_step_ == 2
            states.append(losses + _py_state(g))
        assert len(states[0]) == len(states[1]) and len(states[0]) >= 3 + 15
        for i, (x, y) in enumerate(zip(*states)):
            assert torch.equal(x, y), f"tensor {i} differs with identity exposures"
    finally:
        rp._LIB_OVERRIDE = prev


def check_process_group_python(lib_path, dev):
    """(d): a process group with an exposure throws before anything is rendered or exchanged"""
    from photo_slam_amd.gaussian_renderer import GaussianKeyframe
    cl = train_scene()
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        g, ts = python_trainer(cl, dev, optimize=False)
        ts.world_size_ = 2
        kf = GaussianKeyframe.from_camera(cl.cameras[0], dev)
        kf.exposure_ = identity(dev)
        gt = torch.zeros(3, kf.image_height_, kf.image_width_, device=dev)
        try:
            ts.trainForOneIteration(kf, gt, torch.ones_like(gt), sync_loss=False)
        except RuntimeError as e:
            assert "exposure" in str(e)
        else:
            raise AssertionError("an exposure with a process group was accepted")
        assert ts.iteration_ == 0
    finally:
        rp._LIB_OVERRIDE = prev


# ---- the C++ host: the ops build a keyframe per call, its exposure state travels as arguments (ops_register.cpp)
def cpp_trainer(ops, cl, dev, optimize=True, lr=None):
    h = pg.cpp_trainer(ops, cl, dev)
    o = {"lambda_dssim": TRAIN_LAM, "optimize_exposure": 1.0 if optimize else 0.0, "exposure_lr_max_steps": float(TRAIN_LR_STEPS)}
    if lr is not None:
        o.update({"exposure_lr_init": lr, "exposure_lr_final": lr})
    ops.trainer_set_options(h, o)
    return h


def check_train_cpp(ops, dev):
    """(a) on the C++ host"""
    cl = train_scene()
    none = torch.empty(0, device=dev)
    h = cpp_trainer(ops, cl, dev)
    try:
        args = [pg._cam_args(c, dev) for c in cl.cameras]
        gts = _targets(lambda a: ops.trainer_render_view(h, *a), args, dev)
        mask = torch.ones_like(gts[0])
        state = {k: ([none, none, none], 0) for k in (0, 1)}
        grads, start = {0: [], 1: []}, {}
        for k in (0, 1, 0):
            (E_t, m_t, v_t), step = state[k]
            E = identity(dev) if E_t.numel() == 0 else E_t.clone()
            start.setdefault(k, E)
            img = ops.trainer_render_view(h, *args[k])
            assert torch.equal(ops.trainer_render_view_exposure(h, *args[k], E, True), loss_utils.apply_exposure(img, E))
            want, ge = _expected(img, gts[k], None, E)
            loss, E_t, m_t, v_t, step = ops.trainer_train_exposure(h, *args[k], gts[k], mask, [E_t, m_t, v_t], step)
            assert torch.equal(loss, want), (k, float(loss), float(want))
            state[k] = ([E_t, m_t, v_t], step)
            grads[k].append(ge)
        for k, name in ((0, "A"), (1, "B")):
            _check_replay(name, state[k][0][0], start[k], grads[k], state[k][1])
        assert abs(ops.trainer_exposure_lr(h, 1) - lr_schedule(1)) <= 1e-6 * lr_schedule(1)
    finally:
        ops.trainer_destroy(h)


def check_identity_train_cpp(ops, dev):
    """(b) on the C++ host: the leaves, moments and row_step of trainer_state, and the losses"""
    cl = train_scene()
    none = torch.empty(0, device=dev)
    states, gts = [], None
    for with_exposure in (False, True):
        h = cpp_trainer(ops, cl, dev, optimize=with_exposure, lr=0.0)
        try:
            args = [pg._cam_args(c, dev) for c in cl.cameras]
            if gts is None:
                gts = _targets(lambda a: ops.trainer_render_view(h, *a), args, dev)
            mask = torch.ones_like(gts[0])
            kf = {k: ([none, none, none], 0) for k in (0, 1)}
            losses = []
            for k in (0, 1, 0):
                loss, E_t, m_t, v_t, step = ops.trainer_train_exposure(h, *args[k], gts[k], mask, kf[k][0], kf[k][1])
                kf[k] = ([E_t, m_t, v_t], step)
                losses.append(loss.clone())
            if with_exposure:
                assert torch.equal(kf[0][0][0], identity(dev)) and kf[0][1] == 2 and kf[1][1] == 1
            else:
                assert kf[0][0][0].numel() == 0 and kf[0][1] == 0
            # (trainer_state ends with the training workspace, uint8 buffers whose padding is whatever the allocator left)
            states.append(losses + [t.clone() for t in ops.trainer_state(h) if t.dtype != torch.uint8])
        finally:
            ops.trainer_destroy(h)
    assert len(states[0]) == len(states[1]) and len(states[0]) >= 3 + 15
    for i, (x, y) in enumerate(zip(*states)):
        assert torch.equal(x, y), f"tensor {i} differs with identity exposures"


def check_process_group_cpp(ops, dev, tmp_path):
    """(d) on the C++ host: a one-rank gloo group of this process"""
    import torch.distributed as dist
    cl = train_scene()
    dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "store"), rank=0, world_size=1)
    h = cpp_trainer(ops, cl, dev, optimize=False)
    try:
        ops.trainer_set_process_group(h, dist.group.WORLD.group_name, True)
        a = pg._cam_args(cl.cameras[0], dev)
        gt = torch.zeros(3, cl.cameras[0].H, cl.cameras[0].W, device=dev)
        none = torch.empty(0, device=dev)
        try:
            ops.trainer_train_exposure(h, *a, gt, torch.ones_like(gt), [identity(dev), none, none], 0)
        except RuntimeError as e:
            assert "exposure" in str(e)
        else:
            raise AssertionError("an exposure with a process group was accepted")
    finally:
        ops.trainer_destroy(h)
        dist.destroy_process_group()


# ---- (c) refinePose on a darkened target
# The target is the true pose's render behind REFINE_MAP and the keyframe carries that map: the loss then compares map(render)
# with map(target render), and a refinement that ignored the exposure would chase the brightness change instead.  The reference
# is the float64 loop of pose_grad_cases.reference_refine with the map applied to its render and to its target.
REFINE_MAP = "gain"


def reference_refine(oracle, cl, cam_true, cam_start, zbar):
    c64 = lambda x: torch.tensor(np.asarray(x, np.float64))
    deg = pg.REFINE_DEGREE
    E = exposure(REFINE_MAP).double()
    _, target = pg._oracle_member(oracle, cl, cam_true, deg)
    target = map64(c64(target), E)
    w2c0, projT = pg.base_of(cam_start)
    xi = torch.zeros(6, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([xi], lr=pg.REFINE_LR)
    w2c_true = cam_true.viewmatrix.T
    first = pg.pose_error(w2c0.numpy(), w2c_true, zbar)
    for _ in range(pg.REFINE_ITERS):
        with torch.no_grad():
            here = pg.moved_camera(cam_start, xi.numpy())
        member, _ = pg._oracle_member(oracle, cl, here, deg)
        v, p, c = pg.camera_tensors64(xi, w2c0, projT)
        img = pg.torch_render(c64(cl.xyz), c64(cl.get_scaling()), c64(cl.get_rotation()), c64(cl.get_opacity()), c64(cl.get_features()),
                              v, p, c, float(cam_true.tanfovx), float(cam_true.tanfovy), cam_true.W, cam_true.H,
                              torch.zeros(3, dtype=torch.float64), member, deg)
        loss = (map64(img, E) - target).abs().mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
    with torch.no_grad():
        last = pg.pose_error((pg.exp64(xi) @ w2c0).numpy(), w2c_true, zbar)
    return first, last


_refine_ref = {}


def refine_reference(oracle):
    """(cloud, true camera, start camera, mean depth, initial errors, bound): the reference loop runs once per session"""
    if "ref" not in _refine_ref:
        cl, cam, start, zbar = pg.refine_setup()
        first, ref_last = reference_refine(oracle, cl, cam, start, zbar)
        print("EXPOSURE refine reference: initial", first, "final", ref_last)
        _refine_ref["ref"] = (cl, cam, start, zbar, first, pg.refine_bound(first, ref_last))
    return _refine_ref["ref"]


def check_refine_python(lib_path, dev, oracle):
    from photo_slam_amd.gaussian_renderer import GaussianKeyframe
    cl, cam, start, zbar, first, bound = refine_reference(oracle)
    prev, rp._LIB_OVERRIDE = rp._LIB_OVERRIDE, lib_path
    try:
        g, ts = pg.python_trainer(cl, dev)          # (lambda_dssim 0: the reference loop's plain L1)
        E = exposure(REFINE_MAP, dev)
        gt = loss_utils.apply_exposure(ts.render_view(GaussianKeyframe.from_camera(cam, dev)).clone(), E)
        kf = GaussianKeyframe.from_camera(start, dev)
        kf.exposure_ = E.clone()
        w2c, losses = ts.refinePose(kf, gt, torch.ones_like(gt), pg.REFINE_ITERS, pg.REFINE_LR, pg.REFINE_LR)
        assert torch.equal(kf.exposure_, E) and kf.exposure_step_ == 0, "refinePose must not optimise the exposure"
    finally:
        rp._LIB_OVERRIDE = prev
    last = pg.pose_error(w2c.cpu().numpy(), cam.viewmatrix.T, zbar)
    print("EXPOSURE refine (Python):", dict(initial=first, final=last, bound=bound, loss=(losses[0], losses[-1])))
    assert losses[-1] < losses[0] and last[0] <= bound[0] and last[1] <= bound[1], (last, bound)


def check_refine_cpp(ops, dev, oracle):
    cl, cam, start, zbar, first, bound = refine_reference(oracle)
    h = pg.cpp_trainer(ops, cl, dev)
    try:
        E = exposure(REFINE_MAP, dev)
        gt = loss_utils.apply_exposure(ops.trainer_render_view(h, *pg._cam_args(cam, dev)).clone(), E)
        w2c, losses = ops.trainer_refine_pose_exposure(h, *pg._cam_args(start, dev), gt, torch.ones_like(gt), pg.REFINE_ITERS,
                                                       pg.REFINE_LR, pg.REFINE_LR, E.clone())
    finally:
        ops.trainer_destroy(h)
    last = pg.pose_error(w2c.cpu().numpy(), cam.viewmatrix.T, zbar)
    print("EXPOSURE refine (C++):", dict(initial=first, final=last, bound=bound, loss=(float(losses[0]), float(losses[-1]))))
    assert float(losses[-1]) < float(losses[0]) and last[0] <= bound[0] and last[1] <= bound[1], (last, bound)
