// gaussian_renderer.h -- GaussianRenderer::render (include/gaussian_renderer.h:29-42).
//
// Inside the Photo-SLAM tree this header is used with the reference's own gaussian_model.h /
// gaussian_keyframe.h / gaussian_parameters.h (define PHOTOSLAM_TREE).  Stand-alone (this repo:
// no OpenCV / Eigen / ORB-SLAM3 available) render() is a template over the model and keyframe
// types and touches exactly the members the reference implementation touches
// (src/gaussian_renderer.cpp:41-148): FoVx_, FoVy_, world_view_transform_, full_proj_transform_,
// camera_center_ ; getXYZ(), getOpacityActivation(), getScalingActivation(),
// getRotationActivation(), getCovarianceActivation(), getFeatures(), active_sh_degree_.
#pragma once
#include <torch/torch.h>

#include <cmath>
#include <cstdlib>
#include <memory>
#include <stdexcept>
#include <tuple>

#include "gaussian_rasterizer.h"
#include "sh_utils.h"

#ifdef PHOTOSLAM_TREE
#include "gaussian_keyframe.h"
#include "gaussian_model.h"
#include "gaussian_parameters.h"
#elif !defined(GSR_HAVE_PIPELINE_PARAMS)
#define GSR_HAVE_PIPELINE_PARAMS
struct GaussianPipelineParams {   // include/gaussian_parameters.h:41-49
	bool convert_SHs_ = false;
	bool compute_cov3D_ = false;
};
#endif

namespace gsr_renderer_detail {
// A model whose SH rows are stepped lazily (this repository's GaussianModel, gaussian_model_lite.h: features_row_step_ defined):
// the lazy state handed to a FORWARD-ONLY render read-only -- step = the next one, lr_past[0] = the learning rates of the last
// one taken, so that the rows the view sees are caught up in registers to the steps taken so far (include/gsr.h:
// GSR_FORWARD_ONLY) -- and the SH tensor as it is (in_lazy_step_ around getFeatures(): no flush).  false for any other model
// (the reference's GaussianModel has no lazy rows).
template <class Model>
auto lazy_view(Model& m, ShAdamStep& s, torch::Tensor& shs, int)
    -> decltype((void)m.features_row_step_, (void)m.features_lr_hist_, (void)m.in_lazy_step_, (void)m.groups_, bool())
{
	if (!m.features_row_step_.defined() || m.groups_.size() < 2) return false;
	s = m.featuresAdamStep(Model::ShStep::Lazy);
	s.step++;   // (the counter names the last step taken; the next one is only described, not taken: its rates = lr_past[0])
	if (!m.features_lr_hist_.empty()) {
		s.lr = m.features_lr_hist_[0].first;
		s.lr_tail = m.features_lr_hist_[0].second;
	}
	const bool was = m.in_lazy_step_;
	m.in_lazy_step_ = true;
	shs = m.getFeatures();
	m.in_lazy_step_ = was;
	return true;
}
template <class Model>
bool lazy_view(Model&, ShAdamStep&, torch::Tensor&, long)
{
	return false;
}
}  // namespace gsr_renderer_detail

// A keyframe pose under refinement: a fixed base W2C_0 and a 6-vector xi = (rho, theta), W2C = exp(xi^) W2C_0 (left perturbation,
// exp = the matrix exponential of the 4x4 twist [[theta^, rho], [0, 0]]).  apply() builds the three tensors render() consumes with
// torch ops, as the reference builds them (GaussianKeyframe::computeTransformTensors, src/gaussian_keyframe.cpp:119-141):
// world_view_transform_ = W2C^T, full_proj_transform_ = view . projection_matrix_, camera_center_ = inverse(view)[3, :3] -- so the
// rasterizer's camera gradients (GaussianRasterizerFunctionPose) chain back to xi_ by autograd.  retract() folds xi into the base
// and zeroes it.
struct PoseDelta {
	torch::Tensor base_;                // [4,4] W2C_0 (not transposed)
	torch::Tensor projection_matrix_;   // [4,4] P^T, as the reference keeps it
	torch::Tensor xi_;                  // [6] leaf, requires grad
	// from a keyframe's world_view_transform_ and full_proj_transform_: P^T = inverse(view) . full_proj (in double, rounded once)
	PoseDelta(const torch::Tensor& world_view_transform, const torch::Tensor& full_proj_transform)
	{
		torch::NoGradGuard ng;
		auto view = world_view_transform.detach().to(torch::kFloat64);
		projection_matrix_ = at::linalg_solve(view, full_proj_transform.detach().to(torch::kFloat64)).to(torch::kFloat32);
		base_ = world_view_transform.detach().t().contiguous().to(torch::kFloat32).clone();
		xi_ = torch::zeros({6}, base_.options()).set_requires_grad(true);
	}
	// exp(xi^) as a [4,4] matrix, differentiable at xi = 0
	static torch::Tensor exp(const torch::Tensor& xi)
	{
		auto z = xi.new_zeros({});
		auto row = [&](const torch::Tensor& a, const torch::Tensor& b, const torch::Tensor& c, const torch::Tensor& d) { return torch::stack({a, b, c, d}); };
		auto twist = torch::stack({row(z, -xi[5], xi[4], xi[0]), row(xi[5], z, -xi[3], xi[1]), row(-xi[4], xi[3], z, xi[2]), xi.new_zeros({4})});
		return at::linalg_matrix_exp(twist);
	}
	torch::Tensor w2c() const { return torch::matmul(exp(xi_), base_); }
	template <class Keyframe>
	void apply(Keyframe& kf) const
	{
		auto view = w2c().t();
		kf.world_view_transform_ = view;
		kf.full_proj_transform_ = torch::matmul(view, projection_matrix_);
		kf.camera_center_ = torch::inverse(view)[3].slice(0, 0, 3);
	}
	torch::Tensor retract()
	{
		torch::NoGradGuard ng;
		base_ = torch::matmul(exp(xi_), base_).contiguous();
		xi_.zero_();
		return base_;
	}
};

class GaussianRenderer {
public:
	// returns (render, viewspace_points, visibility_filter, radii).  The reference's parameters, then this repository's
	// extensions as ONE struct (gaussian_rasterizer.h; the default = the reference's data flow).  What the pipeline flags rule
	// out is masked here: with compute_cov3D_ the rasterizer sees a covariance, not the raw leaves (raw_params_ and geom_adam_
	// are cleared), with convert_SHs_ or override colours it sees no SH tensor (sh_grad_view_ and sh_adam_ are cleared).
	// raw_params_ == 7 hands the raw opacity_/scaling_/rotation_ leaves to the rasterizer, which applies sigmoid / exp /
	// normalize and their chain rule in-kernel (include/gsr.h raw_params); render_depth_ is renderWithDepth's to set.
	template <class Keyframe, class Model>
	static std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor> render(
	    std::shared_ptr<Keyframe> viewpoint_camera, int image_height, int image_width, std::shared_ptr<Model> pc,
	    GaussianPipelineParams& pipe, torch::Tensor& bg_color, torch::Tensor& override_color,
	    float scaling_modifier = 1.0f, bool use_override_color = false,
	    const GaussianRasterizationExtensions& extensions = GaussianRasterizationExtensions())
	{
		auto r = render_impl(false, viewpoint_camera, image_height, image_width, pc, pipe, bg_color, override_color, scaling_modifier,
		                     use_override_color, extensions);
		return std::make_tuple(std::get<0>(r), std::get<1>(r), std::get<2>(r), std::get<3>(r));
	}

	// render() with the depth map sum z alpha T and the alpha map 1 - T_final ([H,W] each; include/gsr.h:
	// gsr_forward_args.out_depth / out_alpha) appended: (render, viewspace_points, visibility_filter, radii, depth, alpha).  Both
	// maps are differentiable: a depth or alpha loss reaches the positions, opacities, scales and rotations.
	template <class Keyframe, class Model>
	static std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor> renderWithDepth(
	    std::shared_ptr<Keyframe> viewpoint_camera, int image_height, int image_width, std::shared_ptr<Model> pc,
	    GaussianPipelineParams& pipe, torch::Tensor& bg_color, torch::Tensor& override_color,
	    float scaling_modifier = 1.0f, bool use_override_color = false,
	    const GaussianRasterizationExtensions& extensions = GaussianRasterizationExtensions())
	{
		return render_impl(true, viewpoint_camera, image_height, image_width, pc, pipe, bg_color, override_color, scaling_modifier,
		                   use_override_color, extensions);
	}

private:
	// the body of both: with_depth selects GaussianRasterizerEx::forwardWithDepth (depth and alpha undefined otherwise)
	template <class Keyframe, class Model>
	static std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor> render_impl(
	    bool with_depth, std::shared_ptr<Keyframe> viewpoint_camera, int image_height, int image_width, std::shared_ptr<Model> pc,
	    GaussianPipelineParams& pipe, torch::Tensor& bg_color, torch::Tensor& override_color, float scaling_modifier,
	    bool use_override_color, const GaussianRasterizationExtensions& extensions)
	{
		GaussianRasterizationExtensions ext = extensions;   // (the rasterizer's: masked below)
		// forward_only_: no backward pass follows (a viewer's or an evaluation render) -- the rasterizer prepares
		// nothing for one (GSR_FORWARD_ONLY), screenspace_points is a plain tensor, and on a model whose SH rows are stepped lazily
		// the rows are read as they are and caught up in registers only: the model is neither flushed nor changed
		ext.forward_only_ = ext.forward_only_ || !torch::GradMode::is_enabled();
		// dummy input whose gradient is dL/dmean2D (the densification statistic)
		// (with training_outputs_only_ nobody reads its gradient and the rasterizer never reads its values: the 12 P
		// bytes are then not even zero-filled)
		const bool training_outputs_only = extensions.training_outputs_only_;
		torch::Tensor screenspace_points;
		if (ext.forward_only_) {
			screenspace_points = torch::zeros_like(pc->getXYZ(), torch::TensorOptions().requires_grad(false));
		} else {
			screenspace_points = training_outputs_only ? torch::empty_like(pc->getXYZ(), torch::TensorOptions().requires_grad(true))
			                                           : torch::zeros_like(pc->getXYZ(), torch::TensorOptions().requires_grad(true));
			screenspace_points.retain_grad();
		}

		const float tanfovx = std::tan(viewpoint_camera->FoVx_ * 0.5f);
		const float tanfovy = std::tan(viewpoint_camera->FoVy_ * 0.5f);
		GaussianRasterizationSettings raster_settings(image_height, image_width, tanfovx, tanfovy, bg_color,
		                                              scaling_modifier, viewpoint_camera->world_view_transform_,
		                                              viewpoint_camera->full_proj_transform_, pc->active_sh_degree_,
		                                              viewpoint_camera->camera_center_, false);
		if (ext.raw_params_ != 0 && ext.raw_params_ != 7)
			throw std::runtime_error("GaussianRenderer::render: raw_params_ must be 0 (activations in torch) or 7 (all three in the rasterizer)");
		if (pipe.compute_cov3D_) ext.raw_params_ = 0;
		ext.render_depth_ = with_depth;
		// SH evaluated in torch (convert_SHs_) or colours given: the rasterizer sees no SH tensor, so the SH extensions are off
		const bool sh_in_rasterizer = !use_override_color && !pipe.convert_SHs_;
		if (!sh_in_rasterizer) {
			ext.sh_grad_view_ = torch::Tensor();
			ext.sh_adam_ = ShAdamStep();
		}
		torch::Tensor lazy_shs;
		bool lazy_rows = false;
		if (ext.forward_only_ && sh_in_rasterizer && !ext.sh_adam_.row_step.defined())
			lazy_rows = gsr_renderer_detail::lazy_view(*pc, ext.sh_adam_, lazy_shs, 0);
		// (the same image and gradients either way; off by default: measured a wash, DESIGN.md section 10.  The caller's
		// cull_empty_tiles_ decides; the environment variable GSR_CULL_EMPTY_TILES=0/1, when set, overrides it -- an A/B handle)
		static const int cull_env = [] { const char* e = std::getenv("GSR_CULL_EMPTY_TILES"); return (e && *e) ? (e[0] == '1' ? 1 : 0) : -1; }();
		if (cull_env >= 0) ext.cull_empty_tiles_ = cull_env != 0;
		// the fused geometry step needs the raw leaves in the rasterizer (it steps opacity_ / scaling_ / rotation_ themselves)
		if (ext.raw_params_ != 7) {
			ext.geom_adam_ = GeomAdamStep();
			ext.training_outputs_only_ = false;
		}
		GaussianRasterizerEx rasterizer(raster_settings, ext);

		auto means3D = pc->getXYZ();
		auto opacity = ext.raw_params_ ? pc->opacity_ : pc->getOpacityActivation();
		bool has_scales = false, has_rotations = false, has_cov3D_precomp = false;
		torch::Tensor scales, rotations, cov3D_precomp;
		if (pipe.compute_cov3D_) {
			cov3D_precomp = pc->getCovarianceActivation();
			has_cov3D_precomp = true;
		} else {
			scales = ext.raw_params_ ? pc->scaling_ : pc->getScalingActivation();
			rotations = ext.raw_params_ ? pc->rotation_ : pc->getRotationActivation();
			has_scales = has_rotations = true;
		}
		bool has_shs = false, has_color_precomp = false;
		torch::Tensor shs, colors_precomp;
		if (use_override_color) {
			colors_precomp = override_color;
			has_color_precomp = true;
		} else if (pipe.convert_SHs_) {
			// src/gaussian_renderer.cpp:106-113: SH -> RGB in torch, handed to the rasterizer as colors_precomp
			const int max_coeffs = (pc->max_sh_degree_ + 1) * (pc->max_sh_degree_ + 1);
			auto shs_view = pc->getFeatures().transpose(1, 2).reshape({-1, 3, max_coeffs});
			auto dir_pp = pc->getXYZ() - viewpoint_camera->camera_center_.reshape({1, 3});
			auto dir_pp_normalized = dir_pp / torch::norm(dir_pp, 2, {1}, /*keepdim=*/true);
			auto sh2rgb = sh_utils::eval_sh(pc->active_sh_degree_, shs_view, dir_pp_normalized);
			colors_precomp = torch::clamp_min(sh2rgb + 0.5, 0.0);
			has_color_precomp = true;
		} else {
			shs = lazy_rows ? lazy_shs : pc->getFeatures();
			has_shs = true;
		}
		torch::Tensor rendered_image, radii, depth, alpha;
		if (with_depth) {
			std::tie(rendered_image, radii, depth, alpha) =
			    rasterizer.forwardWithDepth(means3D, screenspace_points, opacity, has_shs, has_color_precomp, has_scales,
			                                has_rotations, has_cov3D_precomp, shs, colors_precomp, scales, rotations, cov3D_precomp);
		} else {
			std::tie(rendered_image, radii) =
			    rasterizer.forward(means3D, screenspace_points, opacity, has_shs, has_color_precomp, has_scales, has_rotations,
			                       has_cov3D_precomp, shs, colors_precomp, scales, rotations, cov3D_precomp);
		}
		// (visibility_filter = radii > 0 is one more launch: a caller that fused everything that consumes it -- the statistics,
		// training_outputs_only_ -- gets an undefined tensor and derives it from radii if it ever wants it)
		return std::make_tuple(rendered_image, screenspace_points, training_outputs_only ? torch::Tensor() : (radii > 0), radii, depth,
		                       alpha);
	}
};
