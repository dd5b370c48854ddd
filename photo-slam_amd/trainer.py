"""The measured train step: GaussianMapper::trainForOneIteration (src/gaussian_mapper.cpp:614-774)
without the SLAM keyframe scheduling -- render -> mask -> L1 + lambda*(1-SSIM) -> backward ->
densification statistics -> Adam -- plus the keyframe-batch data parallelism of SURVEY.md 8(e):
one keyframe per rank, mean of the five leaf gradients over the ranks (ViewFactoredExchange, or the plain
all-reduce of GradientReduction), SUM/MAX of the statistics."""
import os

import torch
import torch.distributed as dist

from . import loss_utils
from .gaussian_renderer import GaussianRenderer


FEATURES_GROUP = 1   # position of features_ in GaussianModel.params() and in the optimizer's groups


def _one_buffer(tensors):
    """A flat view over the storage the given contiguous tensors tile exactly and without gaps (the rasterizer's backward
    hands the gradients of the four small parameter tensors out as slices of one buffer), or None."""
    if len(tensors) < 2 or any(t is None or not t.is_contiguous() or t.dtype != torch.float32 for t in tensors):
        return None
    base = tensors[0].untyped_storage()
    if any(t.untyped_storage().data_ptr() != base.data_ptr() for t in tensors):
        return None
    spans = sorted((t.storage_offset(), t.numel()) for t in tensors)
    end = spans[0][0]
    for off, n in spans:
        if off != end:
            return None
        end = off + n
    if spans[0][0] != 0 or end * 4 != base.nbytes():
        return None
    return torch.empty(0, dtype=torch.float32, device=tensors[0].device).set_(base, 0, (end,))


class GradientReduction:
    """Mean of the per-view gradients over the ranks, overlapped with the optimizer: every tensor's all-reduce is issued
    asynchronously right after backward, largest first (the [P,16,3] SH gradient is 81 % of the 472 MB), and wait(i) blocks
    only the compute stream, only for tensor i -- so Adam on the SH tensor runs while the small reductions are still on the
    links, and their Adam follows.  Tensors that tile one buffer (the four small gradients, see _one_buffer) travel as ONE
    collective.  RCCL averages inside the collective (ncclAvg); gloo (the CPU test path) has no AVG: it sums, and wait()
    scales."""

    def __init__(self, tensors, world_size, sum_only=False):
        """sum_only: the collective SUMS and nothing scales -- the consumer multiplies by grad_scale() = 1/N as it reads the
        gradient (FusedAdam.step_groups): no averaging pass over the buffer (ncclAvg = pre-multiply + sum: with ONE rank a
        whole extra kernel)"""
        self.tensors_, self.world_size_ = tensors, world_size
        self.sum_only_ = sum_only
        self.avg_ = not sum_only and dist.get_backend() == "nccl"
        op = dist.ReduceOp.AVG if self.avg_ else dist.ReduceOp.SUM
        self.order_ = sorted(range(len(tensors)), key=lambda i: -tensors[i].numel())
        # members of one buffer share a single collective: group -> [tensor to reduce, work, scaled?]
        self.group_of_, self.groups_ = {}, []
        by_storage = {}
        for i in self.order_:
            by_storage.setdefault(tensors[i].untyped_storage().data_ptr(), []).append(i)
        for members in by_storage.values():
            flat = _one_buffer([tensors[i] for i in members])
            if flat is not None:
                for i in members:
                    self.group_of_[i] = len(self.groups_)
                self.groups_.append([flat, None, False])
        for i in self.order_:
            if i not in self.group_of_:
                self.group_of_[i] = len(self.groups_)
                self.groups_.append([tensors[i], None, False])
        issued = set()
        for i in self.order_:   # issue in size order; a shared buffer goes out when its first member comes up
            k = self.group_of_[i]
            if k not in issued:
                issued.add(k)
                self.groups_[k][1] = dist.all_reduce(self.groups_[k][0], op=op, async_op=True)

    def collectives(self):
        return len(self.groups_)

    def order(self):
        return self.order_

    def wait(self, i):
        grp = self.groups_[self.group_of_[i]]
        grp[1].wait()
        if not self.avg_ and not self.sum_only_ and not grp[2]:
            grp[0].mul_(1.0 / self.world_size_)
            grp[2] = True

    def grad_scale(self):
        return 1.0 / self.world_size_ if self.sum_only_ else 1.0

    def scale_now(self):
        """sum_only mode after all: average in place (a consumer that cannot apply the scale itself)"""
        if self.sum_only_:
            self.wait_all()
            for grp in self.groups_:
                if not grp[2]:
                    grp[0].mul_(1.0 / self.world_size_)
                    grp[2] = True
            self.sum_only_ = False

    def wait_all(self):
        for i in self.order_:
            self.wait(i)


class ViewFactoredExchange:
    """The same batch mean with 2.6x (8 ranks) to 4.2x (2 ranks) fewer bytes on the links.  81 % of
    the gradient is the [P,16,3] SH tensor, and one view's SH gradient is rank one per Gaussian: basis(dir) x dL_dcolor, with dir known to every rank.
    So the ranks ALL-GATHER the 3-float colour gradients (rasterizer backward with sh_grad_view_; in PARTS row ranges) and
    the camera centres, each rebuilds the mean SH gradient locally (gsr_sh_grad_from_views), and only the other four tensors
    (11 floats per Gaussian) are all-reduced.  Per Gaussian a rank sends (N-1) * 12 + 2 (N-1)/N * 44 B instead of 2 (N-1)/N * 236 B.

    Usage: send, color_view = ViewFactoredExchange.send_buffer(P, device) before the render; color_view ([P,3], rows 0..P-1 of
    send) is handed to the backward (row P receives the camera centre: one gather carries both); others =
    [(index, grad), ...] of the remaining parameters (one all-reduce when they share a buffer, GradientReduction); after
    construction everything is in flight.  sh_gradient() / sh_adam_step() wait for the gather; they read means3D, so call
    them BEFORE Adam moves the positions."""

    @staticmethod
    def send_buffer(P, device):
        send = torch.empty((P + 1, 3), dtype=torch.float32, device=device)
        return send, send[:P]

    PARTS = 1   # ONE all-gather: the colour gradients with the camera centre as row P (every collective costs a launch on
                # RCCL's stream and two cross-stream hand-offs: at one rank four collectives per step cost ~0.1 ms more than two)

    def __init__(self, send, camera_center, others, world_size):
        self.world_size_ = world_size
        P = send.size(0) - 1
        dev = send.device
        self.P_ = P
        self.nccl_ = dist.get_backend() == "nccl"
        send[P].copy_(camera_center.detach().reshape(3).to(torch.float32))
        gathered = torch.empty((world_size, P + 1, 3), dtype=torch.float32, device=dev)
        if self.nccl_:
            work = dist.all_gather_into_tensor(gathered, send.unsqueeze(0), async_op=True)
        else:
            # gloo (the CPU test path) gathers host tensors
            host = gathered.cpu()
            dist.all_gather_into_tensor(host, send.unsqueeze(0).cpu().contiguous())
            gathered.copy_(host)
            work = None
        self.centre_work_ = None
        self.centres_ = gathered[:, P]            # [N, 3], stride (P + 1) * 3
        self.parts_ = [[0, gathered[:, :P], work]]   # [row0, views [N, P, 3] (strided over the views), work or None]
        self.indices_ = [i for i, _ in others]
        # (summed, not averaged: the Adam launch of the four small tensors multiplies by 1/N as it reads the gradients)
        self.reduction_ = GradientReduction([t for _, t in others], world_size, sum_only=True)

    def gathered_parts(self):
        """Yields (first row, camera centres [N,3], colour gradients [N,rows,3]) part by part, each once ITS all-gather has
        landed (stream-side wait: the host keeps queueing)."""
        if self.centre_work_ is not None:
            self.centre_work_.wait()
            self.centre_work_ = None
        for part in self.parts_:
            if part[2] is not None:
                part[2].wait()
                part[2] = None
            yield part[0], self.centres_, part[1]

    def gathered(self):
        """(camera centres [N,3], colour gradients [N,P,3]) of all ranks in one tensor (a copy when the gather ran in parts)"""
        parts = [v for _, _, v in self.gathered_parts()]
        return self.centres_, parts[0] if len(parts) == 1 else torch.cat(parts, 1)

    def sh_gradient(self, means3D, degree, M, out=None):
        from . import rasterize_points as rp
        centres, views = self.gathered()
        return rp.shGradFromViews(means3D.detach(), centres, views, degree, M, 1.0 / self.world_size_, out)

    def sh_adam_step(self, means3D, degree, sh, sh_adam):
        """The rebuild and the Adam step of the SH tensor in one pass per part (gsr_sh_adam_from_views): the mean gradient
        never reaches HBM.  sh_adam: FusedAdam.begin_fused_step(FEATURES_GROUP)."""
        from . import rasterize_points as rp
        m3, shd = means3D.detach(), sh.detach()
        lazy = sh_adam.get("row_step") is not None
        if lazy and int(sh_adam["window"]) < 3:
            raise RuntimeError("lazy rows in the view-factored step need a window of at least 3")
        for row0, centres, views in self.gathered_parts():
            n = views.size(1)
            part = dict(sh_adam, exp_avg=sh_adam["exp_avg"][row0:row0 + n], exp_avg_sq=sh_adam["exp_avg_sq"][row0:row0 + n])
            if lazy:
                part["row_step"] = sh_adam["row_step"][row0:row0 + n]
            rp.shAdamFromViews(m3[row0:row0 + n], centres, views, degree, 1.0 / self.world_size_, shd[row0:row0 + n], part)
        # (lazy rows, gsr_sh_adam_lazy: the rows no view of the batch lights were left alone above; the rotating catch-up that
        # bounds their lag ran inside the rasterizer's backward, next to the blend kernel -- gsr_backward_args.sh_adam together
        # with dL_dcolor_view)

    def order(self):
        """parameter indices of the all-reduced tensors in completion order"""
        return [self.indices_[j] for j in self.reduction_.order()]

    def wait(self, index):
        self.reduction_.wait(self.indices_.index(index))

    def wait_all(self):
        for _ in self.gathered_parts():
            pass
        self.reduction_.wait_all()


def allreduce_mean(tensors, world_size):
    """In-place mean over the ranks, all reductions in flight together."""
    GradientReduction(tensors, world_size).wait_all()


class TrainStep:
    def __init__(self, gaussians, opt, pipe, background, world_size=1, cameras_extent=None, densify=False,
                 densify_min_opacity=0.005, prune_big_point_after_iter=30000, seed=0, factored_exchange=True, fused_sh_adam=True,
                 lazy_sh_adam_window=32, fused_geom_adam=True, cull_empty_tiles=False, antialiasing=False, filter3d=False):
        # the rasterizer's scratch buffers, kept across iterations and grown with headroom (rasterize_points.RasterWorkspace);
        # persistent_workspace_ = False: fresh buffers per call, as the reference's resizeFunctional
        from . import rasterize_points as rp
        self.persistent_workspace_ = True
        self.workspace_ = rp.RasterWorkspace()
        # ... and a second set for render_view(): a view between a training forward and its backward must not overwrite the
        # buffers that forward saved
        self.view_workspace_ = rp.RasterWorkspace()
        # anti-aliased rendering (GSR_ANTIALIAS, include/gsr.h): every render of this object -- the train step at whatever H x W the
        # keyframe's pyramid level has, render_view, refinePose -- compensates the opacity for the 0.3 px low-pass.  Densification and
        # pruning keep their thresholds on the uncompensated sigmoid(opacity), as upstream does.
        self.antialiasing_ = bool(antialiasing)
        # Mip-Splatting's 3-D smoothing filter (GSR_FILTER_3D, include/gsr.h), the other half of antialiasing_: every Gaussian is
        # bounded from below by the sampling interval of the keyframes that observe it.  With filter3d_ on, the model's filter_3D_
        # is recomputed from the cameras of setFilterCameras whenever it is undefined (a densification, increasePcd, a loop closure
        # ... reset it) and every filter3d_interval_ iterations (100: upstream's value, a default to override), before that
        # iteration's render, and EVERY render of this object carries it.  Densification and pruning thresholds, the MCMC moves
        # and the regularisers stay on the unfiltered parameters, as upstream.
        self.filter3d_ = bool(filter3d)
        self.filter3d_interval_ = 100
        self.filter3d_variance_ = 0.2
        self.filter_cameras_ = None     # [K, 20] float32 rows of gsr_filter3d_camera on the model's device (setFilterCameras)
        self.cull_empty_tiles_ = bool(cull_empty_tiles)   # option of this object; GSR_CULL_EMPTY_TILES only overrides (gaussian_renderer.py)
        self.gaussians_, self.opt_, self.pipe_, self.background_ = gaussians, opt, pipe, background
        self.cameras_extent_ = cameras_extent if cameras_extent is not None else gaussians.spatial_lr_scale_
        self.densify_, self.densify_min_opacity_ = densify, densify_min_opacity
        self.prune_big_point_after_iter_ = prune_big_point_after_iter
        # every rank draws the same split samples: identical replicas without a broadcast
        # (a model without a single Gaussian yet -- seedFromDepth makes the first ones -- names its device itself)
        self.generator_ = torch.Generator(device=gaussians.xyz_.device if getattr(gaussians, "xyz_", None) is not None else gaussians.device_).manual_seed(seed)
        self.last_densify_ = None
        self.iteration_ = 0
        self.world_size_ = world_size
        # world_size > 1: ViewFactoredExchange (default) or the plain all-reduce of all five gradients
        self.factored_exchange_ = factored_exchange
        # world_size == 1: the Adam step of the SH tensor runs inside the rasterizer's backward (its 192 B/Gaussian gradient
        # row never reaches HBM); same arithmetic, same result as the separate pass
        self.fused_sh_adam_ = fused_sh_adam
        # ... and the zero-gradient steps of the culled Gaussians' rows taken lazily, at most this many at a time (0 = every
        # row at every step): TrainStep::lazy_sh_adam_window_ of the C++ host
        self.lazy_sh_adam_window_ = lazy_sh_adam_window
        # ... and the Adam steps of xyz / opacity / scaling / rotation inside the backward kernels that hold their gradients
        # (TrainStep::fused_geom_adam_ of the C++ host), on the same iterations
        self.fused_geom_adam_ = fused_geom_adam
        self.ema_loss_for_log_ = 0.0
        # RGB-D keyframes: trainForOneIteration(..., gt_depth) adds depth_loss_weight_ * the L1 distance of the rendered depth map
        # to the sensor's over the pixels with depth_min_ < gt < depth_max_ (RGBD.min_depth / RGBD.max_depth), divided by H W
        # (loss_utils.depth_l1_loss).  0 = the RGB loss alone, gt_depth ignored.
        self.depth_loss_weight_ = 0.0
        self.depth_min_ = 0.0
        self.depth_max_ = float("inf")
        # Monocular keyframes: trainForOneIteration(..., prior_depth) adds depth_prior_weight_ * the depth-prior term of
        # loss_utils.depth_prior_loss (include/gsr.h: gsr_depth_prior_loss) on the rendered depth and alpha maps: the aligned L1
        # after a per-frame scale-and-shift fit, or 1 - Pearson correlation with depth_prior_pearson_; depth_prior_inverse_: the
        # prior is an inverse depth (MiDaS / Depth Anything); pixels with alpha < depth_prior_alpha_min_ take no part.
        # 0 = off, prior_depth ignored.  last_depth_prior_fit_: [s, t, rho, n] of the last step with the term (device), else None.
        self.depth_prior_weight_ = 0.0
        self.depth_prior_pearson_ = False
        self.depth_prior_inverse_ = True
        self.depth_prior_alpha_min_ = 0.5
        self.last_depth_prior_fit_ = None
        # Per-keyframe exposure compensation (upstream 3DGS's per-image exposure): a keyframe that carries exposure_ -- a [3,4]
        # affine colour map -- has it applied between render and loss, inside the loss kernels (gsr_l1_ssim_loss_exposure), in
        # trainForOneIteration and refinePose.  optimize_exposure_: the keyframe of a train step gets the identity at first use
        # and takes one Adam step on its 12 floats after every backward pass (gsr_adam_step, the model's betas and eps), at a
        # learning rate that falls log-linearly from exposure_lr_init_ to exposure_lr_final_ over exposure_lr_max_steps_ of the
        # keyframe's OWN steps.  refinePose applies a keyframe's exposure and never optimises it.
        # Regularisers on the Gaussians a view sees, added to the opacity and scale gradients inside the rasterizer's backward
        # (gsr_backward_args.geom_reg; with fused_geom_adam_ in front of the fused step, so nothing reaches HBM for them):
        #   opacity_reg_ * mean_V sigmoid(opacity) + scale_reg_ * mean_V,k exp(scaling) (the L1 terms of 3DGS-MCMC, which push
        #   Gaussians that explain nothing towards the pruning thresholds) + isotropic_reg_ * mean_V,k |s_k - mean_k s| (MonoGS)
        # over the V Gaussians with radii > 0 in the view.  All 0 = off: no struct is passed and the kernels are those without it.
        # last_reg_losses: the three terms of the last step whose loss was read (sync_loss), a [3] tensor, else None.
        self.opacity_reg_ = 0.0
        self.scale_reg_ = 0.0
        self.isotropic_reg_ = 0.0
        self.last_reg_losses = None
        # Densification by absolute screen-space gradients (AbsGS; gsplat's absgrad): the backward pass sums |d/dmean2D| per pixel
        # before the reduction over a Gaussian's pixels (gsr_backward_args.dL_dmean2D_abs), the fused statistics accumulate the norm
        # of those sums, and densifyAndPrune compares their mean with densify_abs_grad_threshold_ instead of the model's
        # densify_grad_threshold_.  0.0008 is gsplat's recommended value with absgrad: a default for the caller to override, not
        # a tuned number.  Off = the signed statistic and threshold of the reference.
        self.absgrad_ = False
        self.densify_abs_grad_threshold_ = 0.0008
        # Fixed-budget maps (3DGS-MCMC, the other half of opacity_reg_ / scale_reg_): with mcmc_ on and densify set, the iterations
        # that rebuild today run relocateDead + addNew instead of densifyAndPrune -- the count grows by 5 % per event to exactly
        # mcmc_cap_max_ and then stays, no tensor is rebuilt on a relocation and the opacity is never reset -- and every step adds
        # position noise of scale mcmc_noise_lr_ * the current xyz learning rate after the optimizer update.
        self.mcmc_ = False
        self.mcmc_cap_max_ = 0
        self.mcmc_noise_lr_ = 5e5       # (upstream's noise_lr)
        self.mcmc_min_opacity_ = 0.005
        self.last_mcmc_counts_ = None   # the device counts of the last relocateDead
        # Seeding from an RGB-D frame (seedFromDepth; GaussianModel.seedFromDepth, include/gsr.h: gsr_seed_*): SplaTAM's values.
        # seed_max_new_ bounds one call's rows when mcmc_ is off (with mcmc_ on the bound is mcmc_cap_max_ - P).  Nothing calls
        # seedFromDepth by itself.
        self.seed_alpha_threshold_ = 0.5
        self.seed_depth_median_factor_ = 50.0
        self.seed_depth_error_abs_ = 0.0
        self.seed_stride_ = 1
        self.seed_scale_factor_ = 1.0
        self.seed_init_opacity_ = 0.5
        self.seed_max_new_ = 1 << 30
        self.optimize_exposure_ = False
        self.exposure_lr_init_ = 0.01
        self.exposure_lr_final_ = 0.001
        self.exposure_lr_max_steps_ = opt.iterations_

    def exposureLearningRate(self, step):
        """the learning rate of a keyframe's `step`-th exposure step (1-based): log-linear, float arithmetic as exponLrFunc"""
        import numpy as _np
        f32 = _np.float32
        lr_init, lr_final = f32(self.exposure_lr_init_), f32(self.exposure_lr_final_)
        if step < 0 or lr_init <= 0.0 or lr_final <= 0.0:
            return 0.0
        t = min(max(f32(step) / f32(max(int(self.exposure_lr_max_steps_), 1)), f32(0.0)), f32(1.0))
        return float(_np.exp(_np.log(lr_init) * (f32(1) - t) + _np.log(lr_final) * t))

    def _exposure_of(self, viewpoint_cam, create):
        """the keyframe's exposure ([3,4] float32 on the model's device) or None; create: the identity at first use"""
        e = getattr(viewpoint_cam, "exposure_", None)
        if e is None and create:
            e = viewpoint_cam.exposure_ = torch.eye(3, 4, dtype=torch.float32, device=self.gaussians_.xyz_.device)
        if e is not None and (tuple(e.shape) != (3, 4) or e.dtype != torch.float32 or not e.is_contiguous()):
            raise RuntimeError("a keyframe's exposure_ must be a contiguous float32 [3, 4] tensor")
        return e

    def _exposure_adam_step(self, viewpoint_cam, grad):
        """one Adam step of the keyframe's exposure on its own moments and step count"""
        from . import capi
        from . import rasterize_points as rp
        kf, e = viewpoint_cam, viewpoint_cam.exposure_
        if kf.exposure_exp_avg_ is None:
            kf.exposure_exp_avg_, kf.exposure_exp_avg_sq_ = torch.zeros_like(e), torch.zeros_like(e)
        kf.exposure_step_ += 1
        lr = self.exposureLearningRate(kf.exposure_step_)
        lib = rp._lib()
        g = grad.contiguous()
        capi.check(lib, lib.gsr_adam_step(e.data_ptr(), g.data_ptr(), kf.exposure_exp_avg_.data_ptr(), kf.exposure_exp_avg_sq_.data_ptr(),
                                          12, lr, 0.9, 0.999, 1e-15, kf.exposure_step_, 0, 0, lr, rp._stream_ptr(e)),
                   "gsr_adam_step")

    def setFilterCameras(self, cameras):
        """The keyframes the 3-D smoothing filter is derived from: a list of GaussianKeyframes (focal lengths W / (2 tanfovx),
        H / (2 tanfovy) and the size of the keyframe as given: pass it at the finest level it is trained at) or of (viewmatrix,
        focal_x, focal_y, width, height) tuples.  The model's filter is recomputed before the next render.  An empty list and a
        negative filter3d_variance_ are refused by the first render, not here.  Works on a model that has no tensors yet
        (seedFromDepth's start-up): the rows then go to the model's device_."""
        from . import rasterize_points as rp
        rows = []
        for c in cameras:
            if isinstance(c, (tuple, list)):
                rows.append(tuple(c))
            else:
                W, H = int(c.image_width_), int(c.image_height_)
                rows.append((c.world_view_transform_, W / (2.0 * c.tanfovx_), H / (2.0 * c.tanfovy_), W, H))
        g = self.gaussians_
        self.filter_cameras_ = rp.filter3DCameras(rows, g.xyz_.device if getattr(g, "xyz_", None) is not None else g.device_)
        g.filter_3D_ = None

    def viewFilter3D(self, recompute=False):
        """the filter every render of this object carries: None with filter3d_ off; else the model's filter_3D_, computed first when
        it is undefined (or `recompute`)"""
        if not self.filter3d_:
            return None
        if self.world_size_ > 1:
            raise RuntimeError("TrainStep: filter3d_ is not supported with a process group")
        if self.filter_cameras_ is None or self.filter_cameras_.shape[0] == 0:
            raise RuntimeError("TrainStep: filter3d_ is on and no cameras are registered (setFilterCameras)")
        g = self.gaussians_
        if getattr(g, "xyz_", None) is None:   # (no Gaussian yet: nothing is rendered)
            return None
        if self.filter_cameras_.device != g.xyz_.device:
            self.filter_cameras_ = self.filter_cameras_.to(g.xyz_.device)
        f = g.filter_3D_
        if recompute or f is None or f.shape[0] != g.xyz_.shape[0]:
            with torch.no_grad():
                f = g.computeFilter3D(self.filter_cameras_, self.filter3d_variance_)
        return f

    def render_view(self, viewpoint_cam, with_depth=False, apply_exposure=False):
        """A viewer / evaluation render of the current model (GaussianMapper::renderFromPose, renderAndRecordKeyframe):
        forward-only (GSR_FORWARD_ONLY), into the trainer's second workspace, with lazily stepped SH rows read as they are --
        no flush, no counter advanced, nothing of the model or the training workspace touched.  Returns the [3,H,W] image;
        with_depth: (image, depth, alpha), the [H,W] depth map sum z alpha T and alpha map 1 - T_final.  apply_exposure: the
        image behind the keyframe's exposure_ (what the loss compares with the target), if it has one."""
        with torch.no_grad():
            out = GaussianRenderer.render(
                viewpoint_cam, viewpoint_cam.image_height_, viewpoint_cam.image_width_, self.gaussians_, self.pipe_,
                self.background_, cull_empty_tiles=self.cull_empty_tiles_,
                workspace=self.view_workspace_ if self.persistent_workspace_ else None, forward_only=True,
                render_depth=bool(with_depth), antialiasing=self.antialiasing_, filter_3D=self.viewFilter3D())
        image = out[0]
        if apply_exposure and getattr(viewpoint_cam, "exposure_", None) is not None:
            image = loss_utils.apply_exposure(image, viewpoint_cam.exposure_)
        if with_depth:
            return image, out[4], out[5]
        return image

    def score_contribution(self, keyframes, pixel_weights=None):
        """What every Gaussian puts into the given keyframes' images (include/gsr.h: GSR_CONTRIBUTION): one forward-only render per
        keyframe through the second workspace, exactly as render_view -- lazily stepped SH rows read as they are, nothing of the
        model or the training workspace touched, cull_empty_tiles_ and antialiasing_ honoured -- with the three statistics
        accumulating over the keyframes inside the rasterizer.  pixel_weights: one [H,W] float32 map (finite, >= 0) or None per
        keyframe.  Returns (weight_sum, weight_max, n_touched, views_seen): the sum and the maximum over all pixels of all
        keyframes of w alpha T, the number of blending pixels with w != 0, and the number of keyframes with radii > 0."""
        dev = self.gaussians_.xyz_.device
        P = self.gaussians_.xyz_.shape[0]
        wsum, wmax = torch.zeros(P, device=dev), torch.zeros(P, device=dev)
        touched, seen = torch.zeros(P, dtype=torch.int32, device=dev), torch.zeros(P, dtype=torch.int32, device=dev)
        if pixel_weights is not None and len(pixel_weights) != len(keyframes):
            raise RuntimeError("score_contribution: one pixel weight map (or None) per keyframe")
        for i, kf in enumerate(keyframes):
            c = dict(out_weight_sum=wsum, out_weight_max=wmax, out_n_touched=touched, accumulate=True,
                     pixel_weight=pixel_weights[i] if pixel_weights is not None else None)
            with torch.no_grad():
                out = GaussianRenderer.render(kf, kf.image_height_, kf.image_width_, self.gaussians_, self.pipe_, self.background_,
                                              cull_empty_tiles=self.cull_empty_tiles_,
                                              workspace=self.view_workspace_ if self.persistent_workspace_ else None,
                                              forward_only=True, antialiasing=self.antialiasing_, contribution=c,
                                              filter_3D=self.viewFilter3D())
                seen += (out[3] > 0).to(torch.int32)
        return wsum, wmax, touched, seen

    def prune_uncontributing(self, keyframes, min_weight_max, min_views=1):
        """Scores the keyframes (score_contribution) and removes, through prunePoints, the Gaussians that at least min_views of them
        have in their frustum (radii > 0) and whose largest blending weight alpha T at any pixel of any of them stays below
        min_weight_max.  A Gaussian no given keyframe sees is kept: not observed is not useless.  Returns the number removed."""
        if self.world_size_ > 1:
            raise RuntimeError("TrainStep: prune_uncontributing is not supported with a process group")
        _, wmax, _, seen = self.score_contribution(keyframes)
        mask = (seen >= int(min_views)) & (wmax < float(min_weight_max))
        n = int(mask.sum())
        if n:
            with torch.no_grad():
                self.gaussians_.prunePoints(mask)
        return n

    def alignDepthPrior(self, viewpoint_cam, prior, valid=None):
        """A monocular network's relative [H,W] map in the units of the map: one forward-only render with its depth and alpha maps
        (render_view), the scale-and-shift fit of the depth-prior loss against it (depth_prior_inverse_, depth_prior_alpha_min_),
        then gsr_depth_prior_apply.  Returns (metric [H,W] map -- 0 where the prior is invalid --, fit = [s, t, rho, n] on the
        device); the map is what seedFromDepth takes as gt_depth.  A degenerate fit (include/gsr.h) gives an all-zero map, which
        seeds nothing.  An empty model has no render to align to: that throws."""
        g = self.gaussians_
        if getattr(g, "xyz_", None) is None or int(g.xyz_.shape[0]) == 0:
            raise RuntimeError("TrainStep: alignDepthPrior needs a render to align to, and the model is empty "
                               "(seed the first frame from a metric depth map)")
        _, depth, alpha = self.render_view(viewpoint_cam, with_depth=True)
        fit = loss_utils.depth_prior_fit(depth, alpha, prior, inverse=self.depth_prior_inverse_,
                                         alpha_min=self.depth_prior_alpha_min_, valid=valid)
        return loss_utils.depth_prior_apply(prior, fit, inverse=self.depth_prior_inverse_), fit

    def seedFromDepth(self, viewpoint_cam, gt_image, gt_depth, iteration, want_pixels=False):
        """The mapper's "where does the map fail to explain this frame, and what do I put there" step (SplaTAM's add_new_gaussians,
        MonoGS's unexplored-region insertion): one forward-only render of the map with its depth and alpha maps (render_view; none
        while the model is empty -- the first frame of a session initialises the map this way), then GaussianModel.seedFromDepth
        with the seed_* options, the valid range depth_min_ < gt < depth_max_ of the depth loss, and the rasterizer's own
        pixel-centre convention fx = W / (2 tanfovx), cx = (W - 1) / 2 (likewise y), so that a seed projects onto the centre of
        its pixel.  At most mcmc_cap_max_ - P rows with mcmc_ on, seed_max_new_ otherwise.  Returns the number of rows appended."""
        if self.world_size_ > 1:
            raise RuntimeError("TrainStep: seedFromDepth is not supported with a process group")
        g = self.gaussians_
        P = 0 if getattr(g, "xyz_", None) is None else int(g.xyz_.shape[0])
        alpha = depth = None
        if P > 0:
            _, depth, alpha = self.render_view(viewpoint_cam, with_depth=True)
        H, W = int(viewpoint_cam.image_height_), int(viewpoint_cam.image_width_)
        max_new = (int(self.mcmc_cap_max_) - P) if self.mcmc_ else int(self.seed_max_new_)
        return g.seedFromDepth(gt_depth, gt_image, alpha, depth, viewpoint_cam.world_view_transform_,
                               W / (2.0 * viewpoint_cam.tanfovx_), H / (2.0 * viewpoint_cam.tanfovy_), (W - 1) / 2.0, (H - 1) / 2.0,
                               iteration, max_new, min_depth=self.depth_min_, max_depth=self.depth_max_,
                               alpha_threshold=self.seed_alpha_threshold_, depth_error_abs=self.seed_depth_error_abs_,
                               depth_median_factor=self.seed_depth_median_factor_, stride=self.seed_stride_,
                               scale_factor=self.seed_scale_factor_, init_opacity=self.seed_init_opacity_, want_pixels=want_pixels)

    @staticmethod
    def covisibility(n_touched_a, n_touched_b):
        """rasterize_points.covisibility: |A & B| / |A | B| over the Gaussians two views blend"""
        from . import rasterize_points as rp
        return rp.covisibility(n_touched_a, n_touched_b)

    def _frozen_map(self):
        """The model's tensors for a render that must not touch the model (refinePose): detached, and with lazily stepped SH rows
        a caught-up COPY of the SH tensor (the zero-gradient steps the rows are behind, taken on clones: neither the tensor, its
        moments nor row_step change).  One copy per call, nothing per iteration."""
        g = self.gaussians_
        sh = g._features.detach()
        o = g.optimizer_
        st = o.state.get(id(g._features)) if o is not None else None
        if st is not None and "row_step" in st and st["lr_hist"]:
            hist = st["lr_hist"]
            sh = sh.clone()
            from . import rasterize_points as rp_
            rp_.shAdamFlush(sh, dict(exp_avg=st["exp_avg"].clone(), exp_avg_sq=st["exp_avg_sq"].clone(), lr=hist[0][0], lr_tail=hist[0][1],
                                     beta1=o.betas[0], beta2=o.betas[1], eps=o.eps, step=st["step"], row_step=st["row_step"].clone(),
                                     window=st["window"], lr_past=[a for a, _ in hist[1:]], lr_tail_past=[b for _, b in hist[1:]]))
        return g.xyz_.detach(), sh, g.opacity_.detach(), g.scaling_.detach(), g.rotation_.detach()

    def refinePose(self, viewpoint_cam, gt_image, mask, iterations, lr_translation, lr_rotation, gt_depth=None):
        """Photometric refinement of one keyframe's pose against the frozen map: `iterations` Adam steps (betas 0.9 / 0.999,
        eps 1e-8, learning rates lr_translation for rho and lr_rotation for theta) on the xi of a PoseDelta started at
        viewpoint_cam, minimising the train step's loss -- fused L1 + lambda_dssim_ (1 - SSIM), plus depth_l1_loss with gt_depth
        when depth_loss_weight_ != 0.  The camera gradients come from the rasterizer's backward (gsr_backward_args.dL_dviewmatrix
        ...) and reach xi through the pose's construction by autograd.  The map is frozen: its tensors enter detached, no
        optimizer or lazy-row state is touched, and the render uses the second workspace, as render_view does -- a refinement
        between a training forward and its backward disturbs nothing.  Returns (W2C [4,4], [loss per iteration])."""
        from .gaussian_rasterizer import GaussianRasterizationSettings, GaussianRasterizer
        from .gaussian_renderer import PoseDelta
        from . import capi
        use_depth = gt_depth is not None and self.depth_loss_weight_ != 0.0
        g, opt = self.gaussians_, self.opt_
        if self.pipe_.convert_SHs_ or self.pipe_.compute_cov3D_:
            raise RuntimeError("refinePose renders the raw model (convert_SHs_ / compute_cov3D_ must be off)")
        xyz, sh, opacity, scaling, rotation = self._frozen_map()
        filter_3D = self.viewFilter3D()
        pose = PoseDelta.from_keyframe(viewpoint_cam)
        dev = xyz.device
        lr = torch.tensor([lr_translation] * 3 + [lr_rotation] * 3, dtype=torch.float32, device=dev)
        m, v = torch.zeros(6, device=dev), torch.zeros(6, device=dev)
        b1, b2, eps = 0.9, 0.999, 1e-8
        env = os.environ.get("GSR_CULL_EMPTY_TILES")
        cull = (env == "1") if env else self.cull_empty_tiles_
        means2D = torch.zeros_like(xyz)
        eff_mask = self._effective_mask(mask)
        exposure = self._exposure_of(viewpoint_cam, create=False)   # applied, not optimised
        if exposure is not None:
            exposure = exposure.detach()
        losses = []
        for it in range(1, int(iterations) + 1):
            kf = pose.keyframe()
            s = GaussianRasterizationSettings(
                kf.image_height_, kf.image_width_, kf.tanfovx_, kf.tanfovy_, self.background_, 1.0, kf.world_view_transform_,
                kf.full_proj_transform_, g.active_sh_degree_, kf.camera_center_, False, 7, cull_empty_tiles_=cull,
                workspace_=self.view_workspace_ if self.persistent_workspace_ else None, render_depth_=use_depth,
                antialiasing_=self.antialiasing_, filter_3D_=filter_3D)
            out = GaussianRasterizer(s)(xyz, means2D, opacity, True, False, True, True, False, sh, None, scaling, rotation, None)
            loss = loss_utils.fused_l1_ssim_loss(out[0], gt_image, eff_mask, opt.lambda_dssim_, is_root=True, exposure=exposure)
            if use_depth:
                loss = loss + loss_utils.depth_l1_loss(out[2], gt_depth, self.depth_loss_weight_, self.depth_min_, self.depth_max_)
            (grad,) = torch.autograd.grad(loss, pose.xi_)
            with torch.no_grad():
                m.mul_(b1).add_(grad, alpha=1 - b1)
                v.mul_(b2).addcmul_(grad, grad, value=1 - b2)
                step = lr / (1 - b1 ** it)
                pose.xi_.sub_(step * m / (v.sqrt() / (1 - b2 ** it) ** 0.5 + eps))
            losses.append(loss.detach())
        w2c = pose.retract()
        return w2c, [float(x) for x in torch.stack(losses).cpu()] if losses else []

    def _effective_mask(self, mask):
        """rendered * mask with a mask of ones is the identity (src/gaussian_mapper.cpp:692-693; most keyframes carry a full
        mask): such a mask is recognised ONCE per mask tensor (one reduction + host read when a keyframe's mask is first seen)
        and the loss kernels then skip its 2 x 25 MB of reads at 1080p.  Remembered per tensor OBJECT through a weak reference
        (an address or id alone could be reused by another tensor after this one is freed) together with its version counter
        (in-place writes invalidate the entry)."""
        if mask is None:
            return None
        import weakref
        cache = self.__dict__.setdefault("_mask_is_ones", {})
        entry = cache.get(id(mask))
        if entry is None or entry[0]() is not mask or entry[1] != mask._version:
            if len(cache) >= 64:
                cache.clear()
            with torch.no_grad():
                entry = cache[id(mask)] = (weakref.ref(mask), mask._version, bool((mask == 1).all().item()))
        return None if entry[2] else mask

    def trainForOneIteration(self, viewpoint_cam, gt_image, mask, sync_loss=True, position_lr_step=None, gt_depth=None,
                             prior_depth=None):
        """position_lr_step: the step of the position learning-rate schedule -- None = the iteration (src/gaussian_mapper.cpp:672-674,
        the COLMAP flavour); a SLAM session passes the keyframe's use count (:663-671, capped at position_lr_max_steps_).
        gt_depth: the keyframe's [H,W] sensor depth (an RGB-D session's img_auxiliary_undist_); with depth_loss_weight_ != 0 the
        depth L1 loss joins the RGB loss before the one backward pass (its gradient reaches the positions through the depth map).
        prior_depth: a monocular network's relative [H,W] map of the keyframe; with depth_prior_weight_ != 0 the depth-prior term
        joins the loss in the same way (through the depth AND alpha maps); both may be given."""
        use_depth = gt_depth is not None and self.depth_loss_weight_ != 0.0
        if use_depth and self.world_size_ > 1:
            raise RuntimeError("TrainStep: the depth loss is not supported with a process group (depth_loss_weight_ must be 0)")
        use_prior = prior_depth is not None and self.depth_prior_weight_ != 0.0
        if use_prior and self.world_size_ > 1:
            raise RuntimeError("TrainStep: the depth prior is not supported with a process group (depth_prior_weight_ must be 0)")
        exposure = self._exposure_of(viewpoint_cam, create=self.optimize_exposure_)
        if exposure is not None and self.world_size_ > 1:
            raise RuntimeError("TrainStep: exposure compensation is not supported with a process group")
        g, opt = self.gaussians_, self.opt_
        if self.mcmc_ and self.world_size_ > 1:
            raise RuntimeError("TrainStep: mcmc_ is not supported with a process group")
        geom_reg = None
        if self.opacity_reg_ or self.scale_reg_ or self.isotropic_reg_:
            if self.world_size_ > 1:
                raise RuntimeError("TrainStep: the opacity / scale / isotropy regularisers are not supported with a process group")
            # (the loss values are formed only on steps whose loss somebody reads)
            geom_reg = dict(lambda_opacity=float(self.opacity_reg_), lambda_scale=float(self.scale_reg_),
                            lambda_isotropic=float(self.isotropic_reg_),
                            loss=torch.zeros(3, dtype=torch.float32, device=g.xyz_.device) if sync_loss else None)
        self.last_reg_losses = None
        self.last_depth_prior_fit_ = None
        if self.absgrad_ and self.world_size_ > 1:
            raise RuntimeError("TrainStep: absgrad_ is not supported with a process group")
        if self.filter3d_:
            self.viewFilter3D()   # (refuses a process group and a missing camera list before anything of the step happens)
        self.iteration_ += 1
        it = self.iteration_
        g.updateLearningRate(it if position_lr_step is None else min(int(position_lr_step), opt.position_lr_max_steps_))   # :661-674
        sh_send = sh_view = sh_adam = geom_adam = sh_adam_views = None
        if self.world_size_ > 1 and self.factored_exchange_:
            sh_send, sh_view = ViewFactoredExchange.send_buffer(g.xyz_.size(0), g.xyz_.device)
        # this iteration densifies (src/gaussian_mapper.cpp:720-721; the fresh leaves have no gradient, so the reference's
        # optimizer step skips every group)
        rebuilds = bool(self.densify_ and it < opt.densify_until_iter_ and it > opt.densify_from_iter_ and
                        opt.densification_interval_ and it % opt.densification_interval_ == 0)
        # The fused optimizer steps advance their step counters HERE, so they are taken only when render() will really hand
        # them to the rasterizer: with convert_SHs_ the rasterizer sees colours, not the SH tensor (no SH step to fuse), and
        # with compute_cov3D_ it sees a covariance, not the raw scaling / rotation leaves (no geometry step to fuse) --
        # autograd then leaves dense gradients and the ordinary optimizer step below takes those groups.
        if self.world_size_ == 1 and self.fused_sh_adam_ and it < opt.iterations_ and not rebuilds and \
                g._features.size(1) == 16 and g.optimizer_ is not None and not self.pipe_.convert_SHs_:
            sh_adam = g.optimizer_.begin_fused_step(FEATURES_GROUP, self.lazy_sh_adam_window_)
            # (an iteration that resets the opacity replaces that leaf AFTER backward: the reference's optimizer step then
            # skips it -- no gradient -- while a step fused into backward would already have been taken: src/gaussian_mapper.cpp:732-735)
            resets = bool(self.densify_ and not self.mcmc_ and it < opt.densify_until_iter_ and opt.opacity_reset_interval_ and
                          it % opt.opacity_reset_interval_ == 0)
            if self.fused_geom_adam_ and len(g.optimizer_.param_groups) == 5 and not self.pipe_.compute_cov3D_ and not resets:
                # xyz, opacity, scaling, rotation = groups 0, 2, 3, 4 (GaussianModel.trainingSetup)
                tensors = []
                for gi in (0, 2, 3, 4):
                    d = g.optimizer_.begin_fused_step(gi)
                    tensors.append((g.optimizer_.param_groups[gi]["params"][0].detach(), d["exp_avg"], d["exp_avg_sq"], d["lr"], d["step"]))
                geom_adam = dict(tensors=tensors, beta1=sh_adam["beta1"], beta2=sh_adam["beta2"], eps=sh_adam["eps"])
        # Data-parallel step with the view-factored exchange: the SH rows step AFTER the exchange (gsr_sh_adam_from_views), and
        # lazily there too -- a row no view of the batch lights takes a zero-gradient step, i.e. it may take it later; the
        # forward pass gets the same struct so that the rows THIS view sees are up to date before they are evaluated.
        if sh_view is not None and self.lazy_sh_adam_window_ >= 3 and it < opt.iterations_ and not rebuilds and \
                g._features.size(1) == 16 and g.optimizer_ is not None and not self.pipe_.convert_SHs_ and \
                g._features.is_contiguous():
            sh_adam_views = g.optimizer_.begin_fused_step(FEATURES_GROUP, self.lazy_sh_adam_window_)
        # this view's densification statistics (:714-719) are added by the backward kernel that holds dL_dmean2D.  With
        # several ranks they accumulate PER RANK and are reduced only when densification consumes them (below): SUM and MAX
        # commute with the accumulation over iterations, so nothing crosses the links for them on the other 99 of 100 steps
        view_stats = (g.xyz_gradient_accum_, g.denom_, g.max_radii2D_) if it < opt.densify_until_iter_ else None
        fwd_adam = sh_adam if sh_adam is not None else sh_adam_views
        g._in_lazy_step = fwd_adam is not None and fwd_adam.get("row_step") is not None
        try:
            out = GaussianRenderer.render(
                viewpoint_cam, viewpoint_cam.image_height_, viewpoint_cam.image_width_, g, self.pipe_, self.background_,
                sh_grad_view=sh_view, sh_adam=fwd_adam, view_stats=view_stats, geom_adam=geom_adam,
                training_outputs_only=True,   # the statistics are fused (or over): nobody reads the viewspace gradient
                cull_empty_tiles=self.cull_empty_tiles_, workspace=self.workspace_ if self.persistent_workspace_ else None,
                render_depth=use_depth or use_prior, antialiasing=self.antialiasing_, geom_reg=geom_reg,
                absgrad=bool(self.absgrad_) and view_stats is not None,   # (only the statistics read it)
                filter_3D=self.viewFilter3D(recompute=bool(self.filter3d_interval_) and it % int(self.filter3d_interval_) == 0))
            rendered_image, viewspace_point_tensor, visibility_filter, radii = out[:4]
        finally:
            g._in_lazy_step = False
        # :692-698  masked L1 + lambda * (1 - SSIM), fused with its gradient (csrc/train_ops.hip)
        exposure_leaf = None
        if exposure is not None:   # (a leaf of this step's graph: the keyframe's tensor itself is stepped in place below)
            exposure_leaf = exposure.detach().requires_grad_(self.optimize_exposure_)
        loss = loss_utils.fused_l1_ssim_loss(rendered_image, gt_image, self._effective_mask(mask), opt.lambda_dssim_, is_root=True,
                                             exposure=exposure_leaf)
        if use_depth:   # (the sum's backward hands both terms the root's exact 1: is_root stays valid)
            loss = loss + loss_utils.depth_l1_loss(out[4], gt_depth, self.depth_loss_weight_, self.depth_min_, self.depth_max_)
        if use_prior:
            prior_loss, self.last_depth_prior_fit_ = loss_utils.depth_prior_loss(
                out[4], out[5], prior_depth, self.depth_prior_weight_, inverse=self.depth_prior_inverse_,
                pearson=self.depth_prior_pearson_, alpha_min=self.depth_prior_alpha_min_, return_fit=True)
            loss = loss + prior_loss
        # :699 (the root gradient: a cached 1 instead of the ones_like fill autograd launches per backward())
        if getattr(self, "_root_grad", None) is None or self._root_grad.device != loss.device:
            self._root_grad = torch.ones_like(loss).detach()
        loss.backward(self._root_grad)
        if geom_reg is not None and geom_reg["loss"] is not None:
            # the returned loss = photometric (+ depth) + the three terms the backward pass has just written
            self.last_reg_losses = geom_reg["loss"]
            loss = loss.detach() + geom_reg["loss"].sum()
        if sh_adam is not None:
            g.optimizer_.end_fused_step(FEATURES_GROUP, sh_adam)
        with torch.no_grad():
            reduction = None
            if self.world_size_ > 1:
                # keyframe-batch data parallelism: mean of the per-view gradients over RCCL, in flight from here on
                if sh_view is not None:
                    reduction = ViewFactoredExchange(sh_send, viewpoint_cam.camera_center_,
                                                     [(i, p.grad) for i, p in enumerate(g.params_raw()) if i != FEATURES_GROUP],
                                                     self.world_size_)
                else:
                    reduction = GradientReduction([p.grad for p in g.params()], self.world_size_)
            if it < opt.densify_until_iter_:
                if self.densify_:
                    if reduction is not None and rebuilds:
                        # every tensor is about to be rebuilt and this step's update is skipped: the exchange only has to
                        # finish.  (An opacity reset alone replaces ONE leaf: the other groups keep their gradients and
                        # step below through the reduction, the reset opacity has no gradient and is skipped -- :732-735.)
                        reduction.wait_all()
                        reduction = None
                    if rebuilds:                                                                    # :721-730
                        if self.world_size_ > 1:
                            # the batch's statistics since the last densification: norm sums and counts SUM, radii MAX
                            dist.all_reduce(g.xyz_gradient_accum_, op=dist.ReduceOp.SUM)
                            dist.all_reduce(g.denom_, op=dist.ReduceOp.SUM)
                            dist.all_reduce(g.max_radii2D_, op=dist.ReduceOp.MAX)
                        size_threshold = 20 if it > self.prune_big_point_after_iter_ else 0   # :723
                        g.optimizer_.zero_grad(set_to_none=True)   # shapes change; this step's update is skipped
                        if self.mcmc_:
                            self.last_mcmc_counts_ = g.relocateDead(self.mcmc_min_opacity_, generator=self.generator_)
                            g.addNew(self.mcmc_cap_max_, generator=self.generator_, min_opacity=self.mcmc_min_opacity_)
                        else:
                            max_grad = self.densify_abs_grad_threshold_ if self.absgrad_ else opt.densify_grad_threshold_
                            self.last_densify_ = g.densifyAndPrune(max_grad, self.densify_min_opacity_,
                                                                   self.cameras_extent_, size_threshold,
                                                                   generator=self.generator_)
                    if not self.mcmc_ and opt.opacity_reset_interval_ and it % opt.opacity_reset_interval_ == 0:      # :732-735
                        g.resetOpacity()
            if it < opt.iterations_:                                       # :769-772
                if reduction is None:
                    g.optimizer_.step()
                else:
                    # each tensor is updated as soon as ITS reduction has landed (largest first): Adam on the SH tensor
                    # overlaps the four small reductions still on the links
                    g.optimizer_.begin_step()
                    if sh_view is not None:
                        # the SH gradient is rebuilt from the gathered views (reads xyz_: before ITS update) and applied
                        # while the all-reduces of the other four tensors are on the links
                        if sh_adam_views is not None:   # rebuild + Adam in one pass, lazy rows
                            g._in_lazy_step = True
                            try:
                                reduction.sh_adam_step(g.xyz_, g.active_sh_degree_, g._features, sh_adam_views)
                            finally:
                                g._in_lazy_step = False
                            g.optimizer_.end_fused_step(FEATURES_GROUP, sh_adam_views)
                            sh_adam_views = None
                        elif g.features_.size(1) == 16:   # rebuild + Adam in one pass
                            reduction.sh_adam_step(g.xyz_, g.active_sh_degree_, g.features_,
                                                   g.optimizer_.begin_fused_step(FEATURES_GROUP))
                        else:
                            g.features_.grad = reduction.sh_gradient(g.xyz_, g.active_sh_degree_, g.features_.size(1))
                            g.optimizer_.step_group(FEATURES_GROUP)
                    small = [i for i in reduction.order() if i != FEATURES_GROUP]
                    if sh_view is not None:
                        # the small gradients arrived SUMMED (in ONE all-reduce when they share a buffer): one Adam launch for
                        # the four tensors, which applies the 1/N as it reads them
                        for i in small:
                            reduction.wait(i)
                        g.optimizer_.step_groups(small, reduction.reduction_.grad_scale())
                    else:
                        for i in reduction.order():
                            reduction.wait(i)
                            g.optimizer_.step_group(i)
                g.optimizer_.zero_grad(set_to_none=True)
                if self.mcmc_:
                    g.addPositionNoise(self.mcmc_noise_lr_ * g.optimizer_.param_groups[0]["lr"] * g.optimizer_.lr_scale,
                                       generator=self.generator_)
            elif reduction is not None:
                reduction.wait_all()
            # the keyframe's exposure: its own Adam step, on densifying iterations too (it is not rebuilt)
            if self.optimize_exposure_ and exposure_leaf is not None and it < opt.iterations_:
                self._exposure_adam_step(viewpoint_cam, exposure_leaf.grad)
            if sync_loss:
                # :705 (the reference's per-iteration host sync for the loss EMA) -- moved behind the optimizer launches, so
                # that Adam is already queued behind backward while the host waits
                self.ema_loss_for_log_ = 0.4 * loss.item() + 0.6 * self.ema_loss_for_log_
        return loss
