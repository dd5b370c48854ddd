"""GaussianRenderer::render (include/gaussian_renderer.h:29-42, src/gaussian_renderer.cpp:23-149)."""
import os
from dataclasses import dataclass
from typing import Optional

import torch

from .gaussian_rasterizer import GaussianRasterizationSettings, GaussianRasterizer


@dataclass
class GaussianPipelineParams:
    """include/gaussian_parameters.h (pipeline flags)"""
    convert_SHs_: bool = False
    compute_cov3D_: bool = False


@dataclass
class GaussianKeyframe:
    """The per-view tensors render() consumes (include/gaussian_keyframe.h): transposed view
    matrix, transposed full projection, camera centre, FoV -- see scene.make_camera."""
    image_height_: int
    image_width_: int
    tanfovx_: float   # the reference stores FoVx_/FoVy_ and takes tan(FoV/2) in render()
    tanfovy_: float
    world_view_transform_: torch.Tensor
    full_proj_transform_: torch.Tensor
    camera_center_: torch.Tensor
    # Exposure compensation (include/gsr.h: gsr_l1_ssim_loss_exposure): the keyframe's [3,4] affine colour map between render and
    # loss, float32 on the device; None = no compensation, the plain loss kernels.  It belongs to the keyframe, not to the map:
    # its Adam moments and its own step count travel with it (TrainStep.optimize_exposure_).
    exposure_: Optional[torch.Tensor] = None
    exposure_exp_avg_: Optional[torch.Tensor] = None
    exposure_exp_avg_sq_: Optional[torch.Tensor] = None
    exposure_step_: int = 0

    @classmethod
    def from_camera(cls, cam, device):
        t = lambda a: torch.from_numpy(a).to(device).contiguous()
        return cls(cam.H, cam.W, cam.tanfovx, cam.tanfovy, t(cam.viewmatrix), t(cam.projmatrix), t(cam.campos))


class PoseDelta:
    """A keyframe pose under refinement: a fixed base W2C_0 and a 6-vector xi = (rho, theta), W2C = exp(xi^) W2C_0 (left
    perturbation, exp = the matrix exponential of the 4x4 twist [[theta^, rho], [0, 0]]).  keyframe() builds the three tensors
    the renderer consumes with torch ops, as the reference builds them (GaussianKeyframe::computeTransformTensors,
    src/gaussian_keyframe.cpp:119-141): world_view_transform_ = W2C^T, full_proj_transform_ = view . projection_matrix_,
    camera_center_ = inverse(view)[3, :3] -- so the rasterizer's camera gradients (GaussianRasterizerPoseFunction) chain back to
    xi_ by autograd.  retract() folds xi into the base and zeroes it."""

    def __init__(self, w2c, projection_matrix, image_height, image_width, tanfovx, tanfovy):
        self.base_ = w2c.detach().clone().float()                            # [4,4] W2C_0 (not transposed)
        self.projection_matrix_ = projection_matrix.detach().clone().float()  # [4,4] P^T, as the reference keeps it
        self.xi_ = torch.zeros(6, dtype=torch.float32, device=self.base_.device, requires_grad=True)
        self.image_height_, self.image_width_, self.tanfovx_, self.tanfovy_ = image_height, image_width, tanfovx, tanfovy

    @classmethod
    def from_keyframe(cls, kf):
        """the pose of a GaussianKeyframe; its projection P^T = inverse(view) . full_proj (in double, rounded once)"""
        view = kf.world_view_transform_.detach().double()
        proj = torch.linalg.solve(view, kf.full_proj_transform_.detach().double()).float()
        return cls(kf.world_view_transform_.detach().t(), proj, kf.image_height_, kf.image_width_, kf.tanfovx_, kf.tanfovy_)

    @staticmethod
    def exp(xi):
        """exp(xi^) as a [4,4] matrix, differentiable at xi = 0"""
        rho, th = xi[:3], xi[3:]
        z = xi.new_zeros(())
        twist = torch.stack([torch.stack([z, -th[2], th[1], rho[0]]), torch.stack([th[2], z, -th[0], rho[1]]),
                             torch.stack([-th[1], th[0], z, rho[2]]), xi.new_zeros(4)])
        return torch.linalg.matrix_exp(twist)

    def w2c(self):
        return PoseDelta.exp(self.xi_) @ self.base_

    def keyframe(self):
        view = self.w2c().t()
        return GaussianKeyframe(self.image_height_, self.image_width_, self.tanfovx_, self.tanfovy_, view,
                                view @ self.projection_matrix_, torch.linalg.inv(view)[3, :3])

    def retract(self):
        with torch.no_grad():
            self.base_ = (PoseDelta.exp(self.xi_) @ self.base_).contiguous()
            self.xi_.zero_()
        return self.base_


def pose_delta(kf):
    """PoseDelta.from_keyframe"""
    return PoseDelta.from_keyframe(kf)


class GaussianRenderer:
    @staticmethod
    def render(viewpoint_camera, image_height, image_width, pc, pipe, bg_color, override_color=None,
               scaling_modifier=1.0, use_override_color=False, fuse_activations=True, sh_grad_view=None, sh_adam=None, view_stats=None,
               geom_adam=None, training_outputs_only=False, cull_empty_tiles=False, workspace=None, forward_only=False,
               render_depth=False, antialiasing=False, contribution=None, geom_reg=None, absgrad=False, filter_3D=None):
        """returns (render, viewspace_points, visibility_filter, radii), with render_depth (render, viewspace_points,
        visibility_filter, radii, depth, alpha)

        fuse_activations (extension; False = the reference data flow): hand the raw opacity / scaling / rotation
        leaves to the rasterizer, which applies sigmoid / exp / normalize in preprocess and their chain rule in the
        backward preprocess -- same result, ~13 fewer elementwise launches and 3 fewer [P,*] temporaries per step.

        sh_grad_view, sh_adam, view_stats, geom_adam (extensions; None = the reference data flow): see
        GaussianRasterizationSettings.  training_outputs_only: the viewspace gradient and dL_dcov3D are not computed (for a caller
        whose densification statistics are fused: view_stats); implied by geom_adam.  cull_empty_tiles: instances of tiles in which
        no pixel can blend the Gaussian leave the list (same image and gradients; off by default -- measured a wash, DESIGN.md
        section 10); the environment variable GSR_CULL_EMPTY_TILES=0/1, when set, overrides the argument (an A/B handle).

        forward_only (extension): no backward pass follows (a viewer's or an evaluation render; implied under torch.no_grad()) --
        the rasterizer prepares nothing for one (GSR_FORWARD_ONLY), screenspace_points is a plain tensor, and on a model whose SH
        rows are stepped lazily the rows are read as they are and caught up in registers only: the model is neither flushed nor
        changed, and its lazy state survives for the next train step.

        render_depth (extension): the depth map sum z alpha T and the alpha map 1 - T_final ([H, W] each, include/gsr.h:
        gsr_forward_args.out_depth / out_alpha) are appended to the tuple; both are differentiable (a depth or alpha loss
        reaches the positions, opacities, scales and rotations).

        antialiasing (extension; False = the reference's render): the opacity of every Gaussian is compensated for the 0.3 px
        low-pass of its projected covariance (GSR_ANTIALIAS, include/gsr.h; upstream's `antialiasing`), so that a Gaussian keeps
        its brightness across the resolutions a map is trained and viewed at.  A map is rendered with the value it was trained
        with.

        contribution (extension, forward-only renders): GaussianRasterizationSettings.contribution_ -- the per-Gaussian
        contribution statistics of this render, left in the caller's tensors (TrainStep.score_contribution).

        geom_reg (extension): GaussianRasterizationSettings.geom_reg_ -- the opacity / scale / isotropy regularisers on the Gaussians
        this view sees, added to the gradients inside the rasterizer's backward (TrainStep.opacity_reg_ ...).

        absgrad (extension): GaussianRasterizationSettings.absgrad_ -- backward leaves the [P,2] absolute screen-space gradients
        in viewspace_points.absgrad (as upstream's absgrad does), and fused view_stats accumulate their norm (TrainStep.absgrad_).

        filter_3D (extension; None = off): GaussianRasterizationSettings.filter_3D_ -- the [P] 3-D smoothing filter of Mip-Splatting
        (GSR_FILTER_3D, include/gsr.h; pc.computeFilter3D leaves it in pc.filter_3D_), applied to scales and opacity inside the
        rasterizer.  A map is rendered with the filter it was trained with.  Not with pipe.compute_cov3D_."""
        env = os.environ.get("GSR_CULL_EMPTY_TILES")
        if env:
            cull_empty_tiles = env == "1"
        forward_only = bool(forward_only) or not torch.is_grad_enabled()
        # (with the fused geometry step nobody reads its gradient and the rasterizer never reads its values: no zero fill then)
        slim = geom_adam is not None or training_outputs_only
        if forward_only:
            screenspace_points = torch.zeros_like(pc.getXYZ())
        else:
            screenspace_points = (torch.empty_like if slim else torch.zeros_like)(pc.getXYZ(), requires_grad=True)
            try:
                screenspace_points.retain_grad()
            except Exception:
                pass
        # a model whose SH rows are stepped lazily: a forward-only render reads the tensor as it is (no flush) and hands the lazy
        # state over read-only -- the rows it sees are caught up in registers (gsr.h: GSR_FORWARD_ONLY with sh_adam->lazy)
        lazy_view = None
        if forward_only and sh_adam is None and not use_override_color and not pipe.convert_SHs_ and \
                getattr(pc, "optimizer_", None) is not None and getattr(pc, "_features", None) is not None:
            from .trainer import FEATURES_GROUP
            lazy_view = pc.optimizer_.lazy_view_args(FEATURES_GROUP)
            if lazy_view is not None:
                sh_adam = lazy_view
        # SH evaluated in torch (convert_SHs_) or colours given: the rasterizer sees no SH tensor, so the SH extensions are off
        sh_in_rasterizer = not use_override_color and not pipe.convert_SHs_
        raw = 7 if fuse_activations and not pipe.compute_cov3D_ else 0
        raster_settings = GaussianRasterizationSettings(
            image_height, image_width, viewpoint_camera.tanfovx_, viewpoint_camera.tanfovy_, bg_color, scaling_modifier,
            viewpoint_camera.world_view_transform_, viewpoint_camera.full_proj_transform_, pc.active_sh_degree_,
            viewpoint_camera.camera_center_, False, raw,
            sh_grad_view if sh_in_rasterizer else None, sh_adam if sh_in_rasterizer else None, view_stats,
            geom_adam if raw == 7 else None, bool((geom_adam is not None or training_outputs_only) and raw == 7),
            cull_empty_tiles_=bool(cull_empty_tiles), workspace_=workspace, forward_only_=forward_only,
            render_depth_=bool(render_depth), antialiasing_=bool(antialiasing), contribution_=contribution,
            geom_reg_=None if forward_only else geom_reg, absgrad_=bool(absgrad) and not forward_only, filter_3D_=filter_3D)
        rasterizer = GaussianRasterizer(raster_settings)
        means3D = pc.getXYZ()
        means2D = screenspace_points
        opacity = pc.opacity_ if raw else pc.getOpacityActivation()
        scales = rotations = cov3D_precomp = None
        if pipe.compute_cov3D_:                                        # src/gaussian_renderer.cpp:78-86
            cov3D_precomp = pc.getCovarianceActivation()
        else:
            scales = pc.scaling_ if raw else pc.getScalingActivation()
            rotations = pc.rotation_ if raw else pc.getRotationActivation()
        has_shs = has_color_precomp = False
        shs = colors_precomp = None
        if use_override_color:
            colors_precomp, has_color_precomp = override_color, True
        elif pipe.convert_SHs_:                                        # :106-113: SH -> RGB in torch
            from . import sh_utils
            K = (pc.max_sh_degree_ + 1) ** 2
            shs_view = pc.getFeatures().transpose(1, 2).reshape(-1, 3, K)
            dir_pp = pc.getXYZ() - viewpoint_camera.camera_center_.reshape(1, 3)
            dir_pp_normalized = dir_pp / torch.norm(dir_pp, dim=1, keepdim=True)
            sh2rgb = sh_utils.eval_sh(pc.active_sh_degree_, shs_view, dir_pp_normalized)
            colors_precomp, has_color_precomp = torch.clamp_min(sh2rgb + 0.5, 0.0), True
        elif lazy_view is not None:
            shs, has_shs = pc._features, True   # (raw: getFeatures() would flush the lazy rows)
        else:
            shs, has_shs = pc.getFeatures(), True
        has_sr = not pipe.compute_cov3D_
        out = rasterizer(means3D, means2D, opacity, has_shs, has_color_precomp, has_sr, has_sr,
                         pipe.compute_cov3D_, shs, colors_precomp, scales, rotations, cov3D_precomp)
        rendered_image, radii = out[0], out[1]
        # (visibility_filter is one more launch: with the fused geometry step its consumers are fused too -- None then)
        if render_depth:
            return rendered_image, screenspace_points, (None if slim else radii > 0), radii, out[2], out[3]
        return rendered_image, screenspace_points, (None if slim else radii > 0), radii
