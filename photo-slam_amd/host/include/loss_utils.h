// loss_utils.h -- the reference's include/loss_utils.h:24-126 with the SAME names and signatures, for a maintainer who swaps the
// header along with the two GPU libraries: l1_loss() and ssim() -- the two calls of the train step,
// src/gaussian_mapper.cpp:692-698 = src/gaussian_trainer.cpp:82-84 -- run the fused HIP kernels of gsr_l1_ssim_loss (value and
// gradient in two launches instead of 5 + 10 grouped 11x11 convolutions and ~20 elementwise ATen kernels per call: 10 of the
// 15.4 ms a step of the reference's unchanged host code takes at 2 M Gaussians @ 1080p on MI355X are MIOpen convolutions).
// Same results to 1e-6 (tests/test_train_ops.py against the reference's own header compiled, tests/test_reference_pinning.py).
// Everything else in the header -- psnr, psnr_gaussian_splatting, gaussian, create_window, _ssim -- keeps the reference's names,
// signatures and values (tests/test_cpp_host.py pins them to the reference's header compiled) and is computed this library's way
// in ATen: separable windows, the five local statistics of an image pair in one grouped convolution pair.  ssim() falls back to
// it for the calls the kernels do not cover (another window, no size average, a batch, a target that requires a gradient, host tensors).
// The definitions live in lib cuda_rasterizer (host/src/loss_utils.cpp); the reference's header is all-inline.
#pragma once
#include <vector>

#include <torch/torch.h>

namespace loss_utils
{

torch::Tensor l1_loss(torch::Tensor &network_output, torch::Tensor &gt);

torch::Tensor psnr(torch::Tensor &img1, torch::Tensor &img2);

torch::Tensor psnr_gaussian_splatting(torch::Tensor &img1, torch::Tensor &img2);

torch::Tensor gaussian(
    int window_size,
    float sigma,
    torch::DeviceType device_type = torch::kCUDA);

torch::autograd::Variable create_window(
    int window_size,
    int64_t channel,
    torch::DeviceType device_type = torch::kCUDA);

torch::Tensor _ssim(
    torch::Tensor &img1,
    torch::Tensor &img2,
    torch::autograd::Variable &window,
    int window_size,
    int64_t channel,
    bool size_average = true);

torch::Tensor ssim(
    torch::Tensor &img1,
    torch::Tensor &img2,
    torch::DeviceType device_type = torch::kCUDA,
    int window_size = 11,
    bool size_average = true);

// (extension, not in the reference's header) the whole loss of the train step in ONE pass of the kernels:
//   (1 - lambda_dssim) * l1_loss(rendered * mask, gt) + lambda_dssim * (1 - ssim(rendered * mask, gt))
// mask: undefined / empty = all ones.  is_root: the caller promises to call backward() on this very value.
torch::Tensor fused_l1_ssim(torch::Tensor rendered, torch::Tensor gt, torch::Tensor mask, float lambda_dssim, bool is_root = false);
// (extension) ... behind a keyframe's exposure: a [3,4] float32 affine colour map on the device, applied to the rendered image inside
// the loss kernels (include/gsr.h: gsr_l1_ssim_loss_exposure); differentiable in rendered AND exposure.
torch::Tensor fused_l1_ssim_exposure(torch::Tensor rendered, torch::Tensor gt, torch::Tensor mask, float lambda_dssim,
                                     torch::Tensor exposure, bool is_root = false);
// (extension) image_0 E[0][c] + image_1 E[1][c] + image_2 E[2][c] + E[c][3] per pixel of a [3,H,W] image (gsr_apply_exposure): what
// the loss compares with the target, for evaluation renders of a keyframe with an exposure.  No clamping, no gradient.
torch::Tensor apply_exposure(torch::Tensor image, torch::Tensor exposure);
// (extension) the depth L1 loss of an RGB-D keyframe (csrc/train_ops.hip, gsr_depth_l1_loss; deterministic):
//   weight * sum over the pixels with min_depth < gt_depth < max_depth of |depth - gt_depth|, divided by H W
// depth, gt_depth: [H,W] float32 on one device; differentiable in depth.
torch::Tensor depth_l1(torch::Tensor depth, torch::Tensor gt_depth, float weight, float min_depth, float max_depth);
// (extension) the monocular depth-prior term of one view (csrc/train_ops.hip, gsr_depth_prior_loss; the semantics: include/gsr.h;
// deterministic): prior is a network's relative [H,W] map, right up to a scale and a shift, compared with depth / alpha (inverse:
// alpha / depth) over the pixels with alpha >= alpha_min, depth > 0, a finite positive prior and valid != 0 -- the aligned L1 after a
// closed-form per-frame fit, divided by H W, or weight * (1 - Pearson correlation) with pearson.  depth, alpha, prior: float32 [H,W] on
// one device; alpha undefined / empty = all ones; valid: uint8 / bool [H,W] or undefined / empty.  Differentiable in depth and alpha.
// fit: if given, receives [s, t, rho, n] (device).
torch::Tensor depth_prior(torch::Tensor depth, torch::Tensor alpha, torch::Tensor prior, float weight, bool inverse = true,
                          bool pearson = false, float alpha_min = 0.5f, torch::Tensor valid = torch::Tensor(),
                          torch::Tensor* fit = nullptr);
// (extension) [s, t, rho, n] of the fit alone (two launches, no gradient)
torch::Tensor depth_prior_fit(torch::Tensor depth, torch::Tensor alpha, torch::Tensor prior, bool inverse = true, float alpha_min = 0.5f,
                              torch::Tensor valid = torch::Tensor());
// (extension) the prior in the units of the render it was fitted to (gsr_depth_prior_apply): s q + t, or 1 / (s q + t) with inverse; 0
// where the prior is invalid or the result is not finite and positive.  in_place: written over prior (contiguous), which is returned.
torch::Tensor depth_prior_apply(torch::Tensor prior, torch::Tensor fit, bool inverse = true, bool in_place = false);

}
