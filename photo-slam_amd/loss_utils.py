"""include/loss_utils.h:28-124: L1, PSNR, SSIM (11x11 Gaussian window, sigma 1.5, grouped conv2d)."""
import math

import torch
import torch.nn.functional as F


def l1_loss(network_output, gt):
    return torch.abs(network_output - gt).mean()


def psnr(img1, img2):
    mse = torch.pow(img1 - img2, 2).mean()
    return 10.0 * torch.log10(1.0 / mse)


def gaussian(window_size, sigma, device):
    g = torch.tensor([math.exp(-(x - window_size // 2) ** 2 / (2.0 * sigma * sigma)) for x in range(window_size)],
                     dtype=torch.float32, device=device)
    return g / g.sum()


_window_cache = {}


def create_window(window_size, channel, device):
    key = (window_size, channel, str(device))
    if key not in _window_cache:
        w1 = gaussian(window_size, 1.5, device).unsqueeze(1)
        w2 = w1.mm(w1.t()).float().unsqueeze(0).unsqueeze(0)
        _window_cache[key] = w2.expand(channel, 1, window_size, window_size).contiguous()
    return _window_cache[key]


def _ssim(img1, img2, window, window_size, channel, size_average=True):
    pad = window_size // 2
    mu1 = F.conv2d(img1, window, padding=pad, groups=channel)
    mu2 = F.conv2d(img2, window, padding=pad, groups=channel)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = F.conv2d(img1 * img1, window, padding=pad, groups=channel) - mu1_sq
    sigma2_sq = F.conv2d(img2 * img2, window, padding=pad, groups=channel) - mu2_sq
    sigma12 = F.conv2d(img1 * img2, window, padding=pad, groups=channel) - mu1_mu2
    C1, C2 = 0.01 * 0.01, 0.03 * 0.03
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    return ssim_map.mean() if size_average else ssim_map.mean(1).mean(1).mean(1)


def ssim(img1, img2, window_size=11, size_average=True):
    channel = img1.size(-3)
    window = create_window(window_size, channel, img1.device).type_as(img1)
    return _ssim(img1, img2, window, window_size, channel, size_average)


# ---------------------------------------------------------------------------------------------
# Fused HIP version of the train-step loss (csrc/train_ops.hip, gsr_l1_ssim_loss):
#   loss = (1 - lambda) * l1_loss(rendered * mask, gt) + lambda * (1 - ssim(rendered * mask, gt))
# (src/gaussian_mapper.cpp:692-698) with its gradient w.r.t. `rendered`, in two LDS-tiled kernels.
import ctypes as _C

from . import rasterize_points as _rp


class _FusedL1SSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rendered, gt, mask, lambda_dssim, is_root=False):
        ctx.is_root = bool(is_root)
        lib = _rp._lib()
        _rp._check_device(lib, rendered, gt)
        r = rendered.contiguous().float()
        g = gt.contiguous().float()
        m = None if mask is None else mask.contiguous().float()
        _, H, W = r.shape
        grad = torch.empty_like(r)
        loss = torch.empty(1, dtype=torch.float32, device=r.device)
        scratch = torch.empty(int(lib.gsr_loss_scratch_bytes(W, H)), dtype=torch.uint8, device=r.device)
        st = lib.gsr_l1_ssim_loss(r.data_ptr(), g.data_ptr(), None if m is None else m.data_ptr(), W, H,
                                  float(lambda_dssim), grad.data_ptr(), loss.data_ptr(), scratch.data_ptr(),
                                  _rp._stream_ptr(r))
        from . import capi
        capi.check(lib, st, "gsr_l1_ssim_loss")
        ctx.save_for_backward(grad)
        return loss[0]

    @staticmethod
    def backward(ctx, grad_out):
        (grad,) = ctx.saved_tensors
        if ctx.is_root:
            return grad, None, None, None, None
        return grad * grad_out, None, None, None, None


class _FusedL1SSIMExposure(torch.autograd.Function):
    """gsr_l1_ssim_loss_exposure: the loss behind a [3,4] exposure map, with the gradients of the rendered image and of the map"""
    @staticmethod
    def forward(ctx, rendered, gt, mask, lambda_dssim, is_root, exposure):
        ctx.is_root = bool(is_root)
        lib = _rp._lib()
        _rp._check_device(lib, rendered, gt)
        if tuple(exposure.shape) != (3, 4) or exposure.device != rendered.device:
            raise RuntimeError("exposure must be a [3, 4] tensor on the device of the rendered image")
        r = rendered.contiguous().float()
        g = gt.contiguous().float()
        m = None if mask is None else mask.contiguous().float()
        e = exposure.contiguous().float()
        _, H, W = r.shape
        grad = torch.empty_like(r)
        grad_e = torch.empty_like(e)
        loss = torch.empty(1, dtype=torch.float32, device=r.device)
        scratch = torch.empty(int(lib.gsr_loss_exposure_scratch_bytes(W, H)), dtype=torch.uint8, device=r.device)
        st = lib.gsr_l1_ssim_loss_exposure(r.data_ptr(), g.data_ptr(), None if m is None else m.data_ptr(), W, H,
                                           float(lambda_dssim), e.data_ptr(), grad.data_ptr(), grad_e.data_ptr(),
                                           loss.data_ptr(), scratch.data_ptr(), _rp._stream_ptr(r))
        from . import capi
        capi.check(lib, st, "gsr_l1_ssim_loss_exposure")
        ctx.save_for_backward(grad, grad_e)
        return loss[0]

    @staticmethod
    def backward(ctx, grad_out):
        grad, grad_e = ctx.saved_tensors
        if ctx.is_root:
            return grad, None, None, None, None, grad_e
        return grad * grad_out, None, None, None, None, grad_e * grad_out


def fused_l1_ssim_loss(rendered, gt, mask, lambda_dssim, is_root=False, exposure=None):
    """is_root: the caller promises to call .backward() on this very value (upstream gradient exactly 1, as the train step
    does): backward then hands the stored gradient on without the [3,H,W] multiply by one.
    exposure: a keyframe's [3,4] affine colour map (include/gsr.h, gsr_l1_ssim_loss_exposure), applied to the rendered image
    inside the loss kernels; autograd then returns gradients for `rendered` and `exposure`."""
    if exposure is not None:
        return _FusedL1SSIMExposure.apply(rendered, gt, mask, lambda_dssim, is_root, exposure)
    return _FusedL1SSIM.apply(rendered, gt, mask, lambda_dssim, is_root)


def apply_exposure(image, exposure):
    """image_0 E[0][c] + image_1 E[1][c] + image_2 E[2][c] + E[c][3] per pixel of a [3,H,W] image (gsr_apply_exposure): what the
    loss compares with the target, for evaluation renders of a keyframe with an exposure.  No clamping, no gradient."""
    lib = _rp._lib()
    _rp._check_device(lib, image, exposure)
    if tuple(exposure.shape) != (3, 4) or image.dim() != 3 or image.size(0) != 3:
        raise RuntimeError("apply_exposure takes a [3, H, W] image and a [3, 4] exposure")
    r = image.detach().contiguous().float()
    e = exposure.detach().contiguous().float()
    out = torch.empty_like(r)
    st = lib.gsr_apply_exposure(r.data_ptr(), e.data_ptr(), r.size(2), r.size(1), out.data_ptr(), _rp._stream_ptr(r))
    from . import capi
    capi.check(lib, st, "gsr_apply_exposure")
    return out


# Depth L1 loss of an RGB-D keyframe (csrc/train_ops.hip, gsr_depth_l1_loss):
#   loss = weight * sum_{min_depth < gt < max_depth} |depth - gt| / (H W)
# with its gradient w.r.t. the rendered depth map, deterministic (two launches).
class _DepthL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, gt_depth, weight, min_depth, max_depth):
        lib = _rp._lib()
        _rp._check_device(lib, depth, gt_depth)
        d = depth.contiguous().float()
        g = gt_depth.contiguous().float()
        if d.dim() != 2 or g.shape != d.shape:
            raise RuntimeError("depth and gt_depth must be [H, W] tensors of the same shape")
        H, W = d.shape
        grad = torch.empty_like(d)
        loss = torch.empty(1, dtype=torch.float32, device=d.device)
        scratch = torch.empty(int(lib.gsr_depth_loss_scratch_bytes(W, H)), dtype=torch.uint8, device=d.device)
        st = lib.gsr_depth_l1_loss(d.data_ptr(), g.data_ptr(), W, H, float(min_depth), float(max_depth), float(weight),
                                   grad.data_ptr(), loss.data_ptr(), scratch.data_ptr(), _rp._stream_ptr(d))
        from . import capi
        capi.check(lib, st, "gsr_depth_l1_loss")
        ctx.save_for_backward(grad)
        return loss[0]

    @staticmethod
    def backward(ctx, grad_out):
        (grad,) = ctx.saved_tensors
        return grad * grad_out, None, None, None, None


def depth_l1_loss(depth, gt_depth, weight, min_depth, max_depth):
    """weight * sum over the pixels with min_depth < gt_depth < max_depth of |depth - gt_depth|, divided by H W (a scalar
    tensor; differentiable in depth)"""
    return _DepthL1.apply(depth, gt_depth, weight, min_depth, max_depth)


# Monocular depth prior (csrc/train_ops.hip, gsr_depth_prior_loss; the semantics: include/gsr.h): a relative-depth map that is right
# up to a scale and a shift against r = depth / alpha (inverse: alpha / depth) -- the aligned L1 after a closed-form per-frame fit,
# or 1 - Pearson correlation -- with its gradients w.r.t. the rendered depth and alpha maps, deterministic, nothing read on the host.
def _depth_prior_flags(inverse, pearson):
    from . import capi
    return (capi.DEPTH_PRIOR_INVERSE if inverse else 0) | (capi.DEPTH_PRIOR_PEARSON if pearson else 0)


def _depth_prior_maps(lib, depth, alpha, prior, valid):
    _rp._check_device(lib, depth, prior)
    d = depth.contiguous().float()
    q = prior.contiguous().float()
    if d.dim() != 2 or q.shape != d.shape:
        raise RuntimeError("depth and prior must be [H, W] tensors of the same shape")
    a = None
    if alpha is not None:
        a = alpha.contiguous().float()
        if a.shape != d.shape or a.device != d.device:
            raise RuntimeError("alpha must be an [H, W] tensor like depth")
    v = None
    if valid is not None:
        v = valid.contiguous()
        if v.dtype == torch.bool:
            v = v.view(torch.uint8)
        if v.dtype != torch.uint8 or v.shape != d.shape or v.device != d.device:
            raise RuntimeError("valid must be an [H, W] uint8 or bool tensor on the device of depth")
    return d, a, q, v


def _depth_prior_call(lib, d, a, q, v, weight, flags, alpha_min, with_grads):
    from . import capi
    H, W = d.shape
    fit = torch.empty(4, dtype=torch.float32, device=d.device)
    grad_d = torch.empty_like(d) if with_grads else None
    grad_a = torch.empty_like(d) if with_grads and a is not None else None
    loss = torch.empty(1, dtype=torch.float32, device=d.device) if with_grads else None
    scratch = torch.empty(int(lib.gsr_depth_prior_scratch_bytes(W, H)), dtype=torch.uint8, device=d.device)
    ptr = lambda t: None if t is None else t.data_ptr()
    args = capi.DepthPriorArgs(W, H, ptr(d), ptr(a), ptr(q), ptr(v), int(flags), float(alpha_min), float(weight),
                               ptr(grad_d), ptr(grad_a), ptr(loss), ptr(fit))
    st = lib.gsr_depth_prior_loss(_C.byref(args), scratch.data_ptr(), _rp._stream_ptr(d))
    capi.check(lib, st, "gsr_depth_prior_loss")
    return loss, grad_d, grad_a, fit


class _DepthPrior(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, alpha, prior, weight, flags, alpha_min, valid):
        lib = _rp._lib()
        d, a, q, v = _depth_prior_maps(lib, depth, alpha, prior, valid)
        loss, grad_d, grad_a, fit = _depth_prior_call(lib, d, a, q, v, weight, flags, alpha_min, True)
        ctx.has_alpha = a is not None
        ctx.save_for_backward(*([grad_d, grad_a] if a is not None else [grad_d]))
        ctx.mark_non_differentiable(fit)
        return loss[0], fit

    @staticmethod
    def backward(ctx, grad_out, _grad_fit):
        saved = ctx.saved_tensors
        return (saved[0] * grad_out, saved[1] * grad_out if ctx.has_alpha else None, None, None, None, None, None)


def depth_prior_loss(depth, alpha, prior, weight, inverse=True, pearson=False, alpha_min=0.5, valid=None, return_fit=False):
    """The monocular depth-prior term of one view (a scalar tensor; differentiable in depth and alpha): depth and alpha are the
    rendered [H,W] maps (alpha None = all ones), prior the network's [H,W] map, valid an optional [H,W] uint8 / bool mask.
    inverse: the prior is an inverse depth (compared with alpha / depth); pearson: 1 - correlation instead of the aligned L1.
    return_fit: (loss, fit) with fit = [s, t, rho, n] on the device."""
    loss, fit = _DepthPrior.apply(depth, alpha, prior, weight, _depth_prior_flags(inverse, pearson), alpha_min, valid)
    return (loss, fit) if return_fit else loss


def depth_prior_fit(depth, alpha, prior, inverse=True, alpha_min=0.5, valid=None):
    """fit = [s, t, rho, n] of prior against the rendered maps alone (two launches, no gradient)"""
    lib = _rp._lib()
    d, a, q, v = _depth_prior_maps(lib, depth.detach(), None if alpha is None else alpha.detach(), prior, valid)
    return _depth_prior_call(lib, d, a, q, v, 0.0, _depth_prior_flags(inverse, False), alpha_min, False)[3]


def depth_prior_apply(prior, fit, inverse=True, out=None):
    """The prior in the units of the render it was fitted to (gsr_depth_prior_apply): s q + t, or 1 / (s q + t) with inverse; 0
    where the prior is invalid or the result is not finite and positive.  out may be prior itself (contiguous float32)."""
    from . import capi
    lib = _rp._lib()
    _rp._check_device(lib, prior, fit)
    q = prior.detach().contiguous().float()
    f = fit.detach().contiguous().float()
    if q.dim() != 2 or f.numel() != 4:
        raise RuntimeError("depth_prior_apply takes an [H, W] prior and a [4] fit")
    if out is None:
        out = torch.empty_like(q)
    elif out.shape != q.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != q.device:
        raise RuntimeError("depth_prior_apply: out must be a contiguous float32 tensor like prior")
    st = lib.gsr_depth_prior_apply(q.data_ptr(), f.data_ptr(), _depth_prior_flags(inverse, False), q.size(1), q.size(0),
                                   out.data_ptr(), _rp._stream_ptr(q))
    capi.check(lib, st, "gsr_depth_prior_apply")
    return out
