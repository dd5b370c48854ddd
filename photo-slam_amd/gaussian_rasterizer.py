"""GaussianRasterizationSettings / GaussianRasterizerFunction / GaussianRasterizer.

Mirror of include/gaussian_rasterizer.h:25-127 and src/gaussian_rasterizer.cpp:18-234: same
member names, argument order, saved tensors, gradient order and std::runtime_error texts.
"""
from dataclasses import dataclass

import torch

from . import capi
from . import rasterize_points as rp


@dataclass
class GaussianRasterizationSettings:
    """include/gaussian_rasterizer.h:25-55"""
    image_height_: int
    image_width_: int
    tanfovx_: float
    tanfovy_: float
    bg_: torch.Tensor
    scale_modifier_: float
    viewmatrix_: torch.Tensor
    projmatrix_: torch.Tensor
    sh_degree_: int
    campos_: torch.Tensor
    prefiltered_: bool
    raw_params_: int = 0   # extension: GSR_RAW_* mask, activations fused into the rasterizer (include/gsr.h)
    # extension: a [P,3] tensor that receives the clamp-masked colour gradient in backward; the SH gradient is then left
    # to the view-factored exchange (trainer.ViewFactoredExchange) and autograd gets None for sh
    sh_grad_view_: torch.Tensor = None
    # extension, optimizer-in-backward for the SH tensor: dict(exp_avg, exp_avg_sq, lr, lr_tail, beta1, beta2, eps, step) --
    # backward applies this Adam step to sh in place instead of returning its gradient (gsr_backward_args.sh_adam)
    sh_adam_: dict = None
    # extension: (xyz_gradient_accum, denom, max_radii2D) -- backward adds this view's densification statistics itself
    view_stats_: tuple = None
    # extension, optimizer-in-backward for xyz / opacity / scaling / rotation: dict(tensors=[(param, exp_avg, exp_avg_sq, lr,
    # step)] x 4, beta1, beta2, eps) -- backward applies their Adam steps in place (gsr_backward_args.geom_adam) and autograd
    # gets None for the four; training_outputs_only_: the viewspace gradient and dL_dcov3D are not written either
    geom_adam_: dict = None
    training_outputs_only_: bool = False
    # extension (GSR_CULL_EMPTY_TILES, include/gsr.h): instances of tiles in which no pixel can blend the Gaussian are dropped
    # in front of the tile sort -- same image, same gradients, shorter internal lists
    cull_empty_tiles_: bool = False
    # extension: rasterize_points.RasterWorkspace -- the caller's persistent scratch buffers (None = fresh buffers per call, as the
    # reference)
    workspace_: object = None
    # extension (GSR_FORWARD_ONLY, include/gsr.h): render without preparing a backward pass even with grad mode on (a viewer's
    # renderFromPose).  GaussianRasterizer.forward also takes that path by itself under torch.no_grad() and when no input
    # requires grad; the outputs then carry no grad_fn.
    forward_only_: bool = False
    # extension: GaussianRasterizer.forward also renders the depth map sum z alpha T and the alpha map 1 - T_final (include/gsr.h:
    # gsr_forward_args.out_depth / out_alpha) and returns (color, radii, depth, alpha); both maps are differentiable
    render_depth_: bool = False
    # extension (GSR_ANTIALIAS, include/gsr.h): the opacity is compensated for the 0.3 px low-pass of the projected covariance
    # (upstream's `antialiasing`); forward and backward get the same value
    antialiasing_: bool = False
    # extension (GSR_CONTRIBUTION, include/gsr.h), forward-only renders: dict(out_weight_sum, out_weight_max, out_n_touched -- [P]
    # float32 / float32 / int32 tensors or None --, pixel_weight -- [H,W] or None --, accumulate) -- the render also leaves the
    # per-Gaussian contribution statistics in the caller's tensors.  Not differentiable; nothing enters the autograd graph.
    contribution_: dict = None
    # extension (gsr_backward_args.geom_reg, include/gsr.h): dict(lambda_opacity, lambda_scale, lambda_isotropic, loss) -- backward adds
    # the gradients of the opacity / scale / isotropy regularisers on the Gaussians this view sees to the opacity and scale gradients
    # inside the pass (in front of the fused geom_adam_ step, if any).  The lambdas are those of a MEAN over the visible Gaussians:
    # the per-Gaussian weights are lambda_opacity / V and lambda_scale / (3 V), lambda_isotropic / (3 V), V = max(visible count of
    # the forward pass, 1).  loss: a float32 [3] tensor that receives the three loss values, or None (they are not formed).
    geom_reg_: dict = None
    # extension (gsr_backward_args.dL_dmean2D_abs, include/gsr.h; AbsGS, gsplat's `absgrad`): backward also forms the absolute
    # screen-space gradients -- per Gaussian the sums over its pixels of |d/dmean2D.x| and |d/dmean2D.y| of each pixel's own term --
    # and leaves them, as upstream does, in a `.absgrad` attribute ([P,2]) of the means2D / viewspace tensor the forward was given.
    # With view_stats_ the fused statistics accumulate the norm of that pair.  Not together with sh_grad_view_.
    absgrad_: bool = False
    # extension (GSR_FILTER_3D, include/gsr.h): the [P] float32 3-D smoothing filter of every Gaussian (Mip-Splatting; GaussianModel.
    # computeFilter3D) -- scales and opacity are filtered inside the rasterizer, forward and backward get the same tensor, the
    # gradients are those of the unfiltered leaves.  A non-differentiable input; not with cov3D_precomp or sh_grad_view_.  None = off
    filter_3D_: torch.Tensor = None


def _filter_arg(s):
    """settings.filter_3D_ as the rasterizer takes it: detached (the filter has no gradient), None = off"""
    return None if s.filter_3D_ is None else s.filter_3D_.detach()


def _forward(ctx, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, s, depth=None, alpha=None, means2D=None):
    """the forward of both autograd Functions (depth / alpha: [H,W] tensors the maps are rendered into, or None; means2D: the
    viewspace tensor, which receives `.absgrad` in backward with settings.absgrad_)"""
    if s.absgrad_ and s.sh_grad_view_ is not None:
        raise RuntimeError("absgrad_ is not available through the view-factored exchange (sh_grad_view_)")
    ctx.viewspace = means2D if s.absgrad_ else None
    num_rendered, color, radii, geomBuffer, binningBuffer, imgBuffer = rp.RasterizeGaussiansCUDA(
        s.bg_, means3D, colors_precomp, opacities, scales, rotations, s.scale_modifier_, cov3Ds_precomp,
        s.viewmatrix_, s.projmatrix_, s.tanfovx_, s.tanfovy_, s.image_height_, s.image_width_, sh, s.sh_degree_,
        s.campos_, s.prefiltered_, s.raw_params_ | (capi.CULL_EMPTY_TILES if s.cull_empty_tiles_ else 0), s.sh_adam_,   # sh_adam_: lazy mode brings visible rows up to date first
        s.workspace_, out_depth=depth, out_alpha=alpha, antialiasing=s.antialiasing_, filter_3D=_filter_arg(s))
    ctx.set_materialize_grads(False)   # (no zero tensor for the unused gradient of `radii`)
    ctx.num_rendered = num_rendered
    # (the forward pass's one host synchronisation has produced the visible count: the regularisers' mean needs it)
    ctx.visible_count = rp.lastVisibleCount() if s.geom_reg_ is not None else 0
    ctx.raster_settings = s
    ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geomBuffer,
                          binningBuffer, imgBuffer)
    ctx.mark_non_differentiable(radii)
    return color, radii


def _backward(ctx, grad_out_color, grad_depth=None, grad_alpha=None, pose=False):
    """the backward of the autograd Functions: any subset of the image gradients (None = that image took no part in the loss;
    a missing colour gradient next to a map's is zeros).  pose: the gradients of viewmatrix, projmatrix and campos follow the
    eight of the Gaussians' inputs (GaussianRasterizerPoseFunction): twelve values"""
    if grad_out_color is None and grad_depth is None and grad_alpha is None:   # (set_materialize_grads(False)): no gradients
        return (None,) * (12 if pose else 9)
    s = ctx.raster_settings
    colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geomBuffer, binningBuffer, imgBuffer = \
        ctx.saved_tensors
    if grad_out_color is None:
        grad_out_color = torch.zeros((3, int(s.image_height_), int(s.image_width_)), dtype=torch.float32, device=means3D.device)
    cont = lambda t: None if t is None else t.contiguous().float()
    geom_reg = None
    if s.geom_reg_ is not None:
        V = float(max(int(ctx.visible_count), 1))
        geom_reg = dict(w_opacity=float(s.geom_reg_.get("lambda_opacity", 0.0)) / V,
                        w_scale=float(s.geom_reg_.get("lambda_scale", 0.0)) / (3.0 * V),
                        w_isotropic=float(s.geom_reg_.get("lambda_isotropic", 0.0)) / (3.0 * V), loss=s.geom_reg_.get("loss"))
    absgrad = torch.empty((means3D.size(0), 2), dtype=torch.float32, device=means3D.device) if s.absgrad_ else None
    (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales,
     dL_drotations, *dL_dcamera) = rp.RasterizeGaussiansBackwardCUDA(
        s.bg_, means3D, radii, colors_precomp, scales, rotations, s.scale_modifier_, cov3Ds_precomp, s.viewmatrix_,
        s.projmatrix_, s.tanfovx_, s.tanfovy_, grad_out_color, sh, s.sh_degree_, s.campos_, geomBuffer,
        ctx.num_rendered, binningBuffer, imgBuffer, s.raw_params_, s.sh_grad_view_,
        # view-factored mode: the SH step follows the exchange (gsr_sh_adam_from_views); sh_adam_ -- its lazy form -- served
        # the forward pass (rows this view sees caught up) and lets backward run this step's slice of the rotating
        # catch-up next to the blend kernel
        s.sh_adam_ if (s.sh_grad_view_ is None or (s.sh_adam_ or {}).get("row_step") is not None) else None, s.view_stats_,
        s.geom_adam_, s.training_outputs_only_, dL_ddepth=cont(grad_depth), dL_dalpha=cont(grad_alpha),
        pose_grad=pose, workspace=s.workspace_ if (pose or geom_reg is not None) else None, antialiasing=s.antialiasing_,
        geom_reg=geom_reg, absgrad=absgrad, filter_3D=_filter_arg(s))
    if absgrad is not None and ctx.viewspace is not None:
        ctx.viewspace.absgrad = absgrad   # (as upstream: next to .grad on the viewspace tensor)
    # order of src/gaussian_rasterizer.cpp:159-179
    def g(t, like):   # (None where an extension took the gradient's place)
        return t if like.numel() and t is not None else None
    grads = (dL_dmeans3D, dL_dmeans2D, g(dL_dsh, sh), g(dL_dcolors, colors_precomp), dL_dopacity,
             g(dL_dscales, scales), g(dL_drotations, rotations), g(dL_dcov3D, cov3Ds_precomp))
    if pose:
        needs = ctx.needs_input_grad
        return grads + tuple(t if needs[8 + k] else None for k, t in enumerate(dL_dcamera)) + (None,)
    return grads + (None,)


class GaussianRasterizerFunction(torch.autograd.Function):
    """src/gaussian_rasterizer.cpp:28-180"""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings):
        return _forward(ctx, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings,
                        means2D=means2D)

    @staticmethod
    def backward(ctx, grad_out_color, _grad_radii):
        return _backward(ctx, grad_out_color)


class GaussianRasterizerDepthFunction(torch.autograd.Function):
    """GaussianRasterizerFunction with the depth and alpha maps (settings.render_depth_): returns (color, radii, depth, alpha).
    Backward takes any subset of the three image gradients (a missing colour gradient is zeros, a missing depth / alpha gradient
    is left out of the call: gsr_backward_args.dL_ddepth / dL_dalpha)."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings):
        s = raster_settings
        depth = torch.zeros((int(s.image_height_), int(s.image_width_)), dtype=torch.float32, device=means3D.device)
        alpha = torch.zeros_like(depth)
        color, radii = _forward(ctx, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, s, depth, alpha, means2D=means2D)
        return color, radii, depth, alpha

    @staticmethod
    def backward(ctx, grad_out_color, _grad_radii, grad_depth, grad_alpha):
        return _backward(ctx, grad_out_color, grad_depth, grad_alpha)


class GaussianRasterizerPoseFunction(torch.autograd.Function):
    """The rasterizer with the camera as a differentiable input: viewmatrix, projmatrix and campos (the settings' three tensors,
    passed as inputs so that their graph -- a pose built with torch ops, PoseDelta -- continues behind them) get the gradients of
    gsr_backward_args.dL_dviewmatrix / dL_dprojmatrix / dL_dcampos.  GaussianRasterizer.forward takes this Function when one of
    the three requires grad.  Returns (color, radii), with settings.render_depth_ (color, radii, depth, alpha)."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, viewmatrix, projmatrix,
                campos, raster_settings):
        s = raster_settings
        if s.sh_grad_view_ is not None:
            raise RuntimeError("camera gradients are not available through the view-factored exchange (sh_grad_view_)")
        if not s.render_depth_:
            return _forward(ctx, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, s, means2D=means2D)
        depth = torch.zeros((int(s.image_height_), int(s.image_width_)), dtype=torch.float32, device=means3D.device)
        alpha = torch.zeros_like(depth)
        color, radii = _forward(ctx, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, s, depth, alpha, means2D=means2D)
        return color, radii, depth, alpha

    @staticmethod
    def backward(ctx, grad_out_color, _grad_radii, grad_depth=None, grad_alpha=None):
        return _backward(ctx, grad_out_color, grad_depth, grad_alpha, pose=True)


def _rasterize_forward_only(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, s):
    """The forward pass alone (GSR_FORWARD_ONLY): RasterizeGaussiansCUDA directly, no autograd node, no buffers kept.  Only the
    lazy form of sh_adam_ concerns a forward pass (its rows are then read, not written).  With s.render_depth_ the depth and alpha
    maps are rendered too: (color, radii, depth, alpha)."""
    lazy = s.sh_adam_ if s.sh_adam_ is not None and s.sh_adam_.get("row_step") is not None else None
    depth = alpha = None
    if s.render_depth_:
        depth = torch.zeros((int(s.image_height_), int(s.image_width_)), dtype=torch.float32, device=means3D.device)
        alpha = torch.zeros_like(depth)
    c = s.contribution_ or {}
    with torch.no_grad():
        _, color, radii, _, _, _ = rp.RasterizeGaussiansCUDA(
            s.bg_, means3D, colors_precomp, opacities, scales, rotations, s.scale_modifier_, cov3Ds_precomp,
            s.viewmatrix_, s.projmatrix_, s.tanfovx_, s.tanfovy_, s.image_height_, s.image_width_, sh, s.sh_degree_,
            s.campos_, s.prefiltered_,
            s.raw_params_ | (capi.CULL_EMPTY_TILES if s.cull_empty_tiles_ else 0) | capi.FORWARD_ONLY, lazy, s.workspace_,
            out_depth=depth, out_alpha=alpha, antialiasing=s.antialiasing_, pixel_weight=c.get("pixel_weight"),
            out_weight_sum=c.get("out_weight_sum"), out_weight_max=c.get("out_weight_max"), out_n_touched=c.get("out_n_touched"),
            contribution_accumulate=bool(c.get("accumulate", False)), filter_3D=_filter_arg(s))
    if s.render_depth_:
        return color, radii, depth, alpha
    return color, radii


def rasterizeGaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings):
    """include/gaussian_rasterizer.h:78-100"""
    return GaussianRasterizerFunction.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                            cov3Ds_precomp, raster_settings)


class GaussianRasterizer(torch.nn.Module):
    """include/gaussian_rasterizer.h:102-127, src/gaussian_rasterizer.cpp:18-26,182-234"""

    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings_ = raster_settings

    def markVisibleGaussians(self, positions):
        with torch.no_grad():
            s = self.raster_settings_
            return rp.markVisible(positions, s.viewmatrix_, s.projmatrix_)

    def forward(self, means3D, means2D, opacities, has_shs, has_colors_precomp, has_scales, has_rotations,
                has_cov3D_precomp, shs=None, colors_precomp=None, scales=None, rotations=None, cov3D_precomp=None):
        if (not has_shs and not has_colors_precomp) or (has_shs and has_colors_precomp):
            raise RuntimeError("Please provide excatly one of either SHs or precomputed colors!")
        if ((not has_scales or not has_rotations) and not has_cov3D_precomp) or \
                ((has_scales or has_rotations) and has_cov3D_precomp):
            raise RuntimeError("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        empty = torch.empty(0, device=means3D.device)
        shs = shs if has_shs else empty
        colors_precomp = colors_precomp if has_colors_precomp else empty
        scales = scales if has_scales else empty
        rotations = rotations if has_rotations else empty
        cov3D_precomp = cov3D_precomp if has_cov3D_precomp else empty
        # no backward pass can follow (grad mode off, or nothing to differentiate), or the caller says none will: the forward pass
        # alone (GSR_FORWARD_ONLY -- the same image and radii, no scratch for a backward pass, no autograd node)
        s = self.raster_settings_
        if s.contribution_ is not None and not (s.forward_only_ or not torch.is_grad_enabled()):
            raise RuntimeError("contribution_ is an extension of forward-only renders (forward_only_, or torch.no_grad())")
        if s.forward_only_ or not torch.is_grad_enabled() or not any(
                t is not None and t.requires_grad
                for t in (means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                          s.viewmatrix_, s.projmatrix_, s.campos_)):
            return _rasterize_forward_only(means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, s)
        if any(t is not None and t.requires_grad for t in (s.viewmatrix_, s.projmatrix_, s.campos_)):
            # the camera is being differentiated (pose refinement): its three tensors enter as inputs
            return GaussianRasterizerPoseFunction.apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                                        cov3D_precomp, s.viewmatrix_, s.projmatrix_, s.campos_, s)
        if s.render_depth_:   # (color, radii, depth, alpha)
            return GaussianRasterizerDepthFunction.apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                                         cov3D_precomp, s)
        color, radii = rasterizeGaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                          cov3D_precomp, self.raster_settings_)
        return color, radii
