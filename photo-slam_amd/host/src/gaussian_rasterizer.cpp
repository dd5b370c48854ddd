// gaussian_rasterizer.cpp -- autograd glue, counterpart of src/gaussian_rasterizer.cpp:18-234.
#include "gaussian_rasterizer.h"

#include <initializer_list>
#include <stdexcept>

#include "../../../include/gsr.h"

torch::Tensor GaussianRasterizer::markVisibleGaussians(torch::Tensor& positions)
{
	torch::NoGradGuard no_grad;
	return markVisible(positions, raster_settings_.viewmatrix_, raster_settings_.projmatrix_);
}

namespace {

// What backward needs besides the saved tensors: the settings and the extensions of the call, kept whole
// (ctx->saved_data["state"]) -- backward_impl reads whatever field it wants, no field is packed or unpacked by name
struct SavedState : torch::CustomClassHolder {
	SavedState(GaussianRasterizationSettings&& s, GaussianRasterizationExtensions&& e) : settings(std::move(s)), extensions(std::move(e)) {}
	GaussianRasterizationSettings settings;
	GaussianRasterizationExtensions extensions;
	int num_rendered = 0;
	int visible_count = 0;   // the regularisers' mean is over the Gaussians the forward pass saw
};

// RasterizeGaussiansCUDA as both paths below call it.  more_raw_params: GSR_FORWARD_ONLY or 0; depth / alpha: defined = the
// maps are rendered into them (render_depth_).  Only the lazy form of sh_adam_ concerns a forward pass (visible rows are
// brought up to date first; forward-only: read at their caught-up values, not written) -- RasterizeGaussiansCUDA looks at no other.
auto rasterize_forward(const torch::Tensor& means3D, const torch::Tensor& sh, const torch::Tensor& colors_precomp,
                       const torch::Tensor& opacities, const torch::Tensor& scales, const torch::Tensor& rotations,
                       const torch::Tensor& cov3Ds_precomp, const GaussianRasterizationSettings& s,
                       const GaussianRasterizationExtensions& e, int more_raw_params, const torch::Tensor& depth,
                       const torch::Tensor& alpha)
{
	RasterForwardExtensions f;
	f.raw_params = e.raw_params_ | (e.cull_empty_tiles_ ? GSR_CULL_EMPTY_TILES : 0) | more_raw_params;
	f.sh_adam = &e.sh_adam_;
	f.workspace = e.workspace_;
	f.out_depth = depth;
	f.out_alpha = alpha;
	f.antialiasing_ = e.antialiasing_;
	if (e.filter_3D_.defined()) f.filter_3D_ = e.filter_3D_.detach();   // (an input without a gradient)
	f.pixel_weight = e.pixel_weight_;
	f.out_weight_sum = e.out_weight_sum_;
	f.out_weight_max = e.out_weight_max_;
	f.out_n_touched = e.out_n_touched_;
	f.contribution_accumulate = e.contribution_accumulate_;
	return RasterizeGaussiansCUDA(s.bg_, means3D, colors_precomp, opacities, scales, rotations, s.scale_modifier_, cov3Ds_precomp,
	                              s.viewmatrix_, s.projmatrix_, s.tanfovx_, s.tanfovy_, s.image_height_, s.image_width_, sh,
	                              s.sh_degree_, s.campos_, s.prefiltered_, f);
}

// shared by GaussianRasterizerFunction (the reference's contract: no extensions) and GaussianRasterizerFunctionEx; the node
// takes the two structs over (moved, not copied again)
torch::autograd::tensor_list forward_impl(torch::autograd::AutogradContext* ctx, torch::Tensor means3D, torch::Tensor sh,
                                          torch::Tensor colors_precomp, torch::Tensor opacities, torch::Tensor scales,
                                          torch::Tensor rotations, torch::Tensor cov3Ds_precomp,
                                          GaussianRasterizationSettings&& settings, GaussianRasterizationExtensions&& extensions)
{
	auto state = c10::make_intrusive<SavedState>(std::move(settings), std::move(extensions));
	const GaussianRasterizationSettings& s = state->settings;
	const GaussianRasterizationExtensions& e = state->extensions;
	torch::Tensor depth, alpha;   // (render_depth_: the two maps, written for every pixel)
	if (e.render_depth_) {
		depth = torch::zeros({s.image_height_, s.image_width_}, means3D.options().dtype(torch::kFloat32));
		alpha = torch::zeros({s.image_height_, s.image_width_}, means3D.options().dtype(torch::kFloat32));
	}
	auto r = rasterize_forward(means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, s, e, 0, depth, alpha);
	state->num_rendered = std::get<0>(r);
	// (the forward pass's one host synchronisation has produced the count)
	if (e.hasGeomReg()) state->visible_count = lastVisibleCount();
	// (no zero tensor for the unused gradient of `radii`: autograd would otherwise fill P ints per backward)
	ctx->set_materialize_grads(false);
	ctx->saved_data["state"] = c10::IValue::make_capsule(state);
	auto color = std::get<1>(r);
	auto radii = std::get<2>(r);
	// same 14 tensors, same order as the reference (src/gaussian_rasterizer.cpp:87-100)
	ctx->save_for_backward({s.bg_, s.viewmatrix_, s.projmatrix_, s.campos_, colors_precomp, means3D, scales, rotations,
	                        cov3Ds_precomp, radii, sh, std::get<3>(r), std::get<4>(r), std::get<5>(r)});
	ctx->mark_non_differentiable({radii});
	if (e.render_depth_) return {color, radii, depth, alpha};
	return {color, radii};
}

// n_extra: undefined gradients for the trailing non-tensor inputs (raster_settings [, extensions])
// pose: the gradients of viewmatrix, projmatrix and campos follow the eight (GaussianRasterizerFunctionPose)
torch::autograd::tensor_list backward_impl(torch::autograd::AutogradContext* ctx, torch::autograd::tensor_list grad_outputs,
                                           int n_extra, bool pose = false)
{
	const int n_camera = pose ? 3 : 0;
	// render_depth_: (color, radii, depth, alpha) -- the gradients of the two maps, either undefined (not in the loss)
	const torch::Tensor dL_ddepth = grad_outputs.size() > 2 ? grad_outputs[2] : torch::Tensor();
	const torch::Tensor dL_dalpha = grad_outputs.size() > 3 ? grad_outputs[3] : torch::Tensor();
	// no image took part in the loss (set_materialize_grads(false)): no gradients
	if (!grad_outputs[0].defined() && !dL_ddepth.defined() && !dL_dalpha.defined()) {
		torch::autograd::tensor_list none(static_cast<size_t>(8 + n_camera + n_extra));
		return none;
	}
	const auto state = c10::static_intrusive_pointer_cast<SavedState>(ctx->saved_data["state"].toCapsule());
	const GaussianRasterizationSettings& s = state->settings;
	const GaussianRasterizationExtensions& e = state->extensions;
	torch::Tensor dL_dcolor = grad_outputs[0];
	if (!dL_dcolor.defined())   // (a loss on the maps alone: the colour gradient is zeros)
		dL_dcolor = torch::zeros({3, s.image_height_, s.image_width_}, dL_ddepth.defined() ? dL_ddepth.options() : dL_dalpha.options());
	auto map_grad = [](const torch::Tensor& t) { return t.defined() ? t.contiguous().to(torch::kFloat32) : t; };
	RasterBackwardExtensions b;
	b.raw_params = e.raw_params_;
	b.antialiasing_ = e.antialiasing_;
	if (e.filter_3D_.defined()) b.filter_3D_ = e.filter_3D_.detach();
	b.dL_dcolor_view = e.sh_grad_view_;
	// view-factored mode: the SH step follows the exchange (gsr_sh_adam_from_views); sh_adam_ -- its lazy form only -- served
	// the forward pass (rows this view sees caught up) and lets backward run this step's slice of the rotating catch-up
	if (!e.sh_grad_view_.defined() || e.sh_adam_.row_step.defined()) b.sh_adam = &e.sh_adam_;
	b.view_stats = &e.view_stats_;
	b.geom_adam = &e.geom_adam_;
	b.training_outputs_only = e.training_outputs_only_;
	b.dL_ddepth = map_grad(dL_ddepth);
	b.dL_dalpha = map_grad(dL_dalpha);
	b.color_view_ready_stream = e.color_view_ready_stream_;
	b.packed_view = e.packed_view_;
	b.packed_capacity = e.packed_capacity_;
	b.absgrad = e.absgrad_;
	PoseGradients camera;
	if (pose) {
		b.pose_grad = &camera;
		b.workspace = e.workspace_;
	}
	GeomRegStep reg;
	if (e.hasGeomReg()) {
		// (double, then one rounding: the arithmetic of the Python host)
		const double V = static_cast<double>(state->visible_count > 1 ? state->visible_count : 1);
		reg.w_opacity = static_cast<float>(e.opacity_reg_ / V);
		reg.w_scale = static_cast<float>(e.scale_reg_ / (3.0 * V));
		reg.w_isotropic = static_cast<float>(e.isotropic_reg_ / (3.0 * V));
		reg.loss = e.reg_loss_;
		b.geom_reg = &reg;
		b.workspace = e.workspace_;
	}
	auto v = ctx->get_saved_variables();
	auto g = RasterizeGaussiansBackwardCUDA(v[0] /*bg*/, v[5] /*means3D*/, v[9] /*radii*/, v[4] /*colors_precomp*/,
	                                        v[6] /*scales*/, v[7] /*rotations*/, s.scale_modifier_, v[8] /*cov3Ds*/,
	                                        v[1] /*view*/, v[2] /*proj*/, s.tanfovx_, s.tanfovy_, dL_dcolor, v[10] /*sh*/,
	                                        s.sh_degree_, v[3] /*campos*/, v[11], state->num_rendered, v[12], v[13], b);
	// gradient order of the forward inputs (src/gaussian_rasterizer.cpp:159-179); absent optionals get none
	auto opt = [](const torch::Tensor& grad, const torch::Tensor& input) {
		return (input.defined() && input.numel() != 0 && grad.defined()) ? grad : torch::Tensor();
	};
	// (undefined where an extension took the gradient's place: fused optimizer steps, training_outputs_only_)
	torch::autograd::tensor_list out = {std::get<3>(g) /*means3D*/,
	                                    std::get<0>(g) /*means2D*/,
	                                    opt(std::get<5>(g), v[10]) /*sh*/,
	                                    opt(std::get<1>(g), v[4]) /*colors_precomp*/,
	                                    std::get<2>(g) /*opacities*/,
	                                    opt(std::get<6>(g), v[6]) /*scales*/,
	                                    opt(std::get<7>(g), v[7]) /*rotations*/,
	                                    opt(std::get<4>(g), v[8]) /*cov3Ds_precomp*/};
	if (pose) {
		out.push_back(camera.dL_dviewmatrix);
		out.push_back(camera.dL_dprojmatrix);
		out.push_back(camera.dL_dcampos);
	}
	for (int i = 0; i < n_extra; i++) out.push_back(torch::Tensor());
	return out;
}

// GaussianRasterizer::forward, src/gaussian_rasterizer.cpp:182-234: the XOR validation and the empty optionals
void validate_and_fill(const torch::Tensor& means3D, bool has_shs, bool has_colors_precomp, bool has_scales, bool has_rotations,
                       bool has_cov3D_precomp, torch::Tensor& shs, torch::Tensor& colors_precomp, torch::Tensor& scales,
                       torch::Tensor& rotations, torch::Tensor& cov3D_precomp)
{
	if (has_shs == has_colors_precomp)
		throw std::runtime_error("Please provide excatly one of either SHs or precomputed colors!");
	if (((!has_scales || !has_rotations) && !has_cov3D_precomp) || ((has_scales || has_rotations) && has_cov3D_precomp))
		throw std::runtime_error(
		    "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
	auto empty = torch::empty({0}, means3D.options().dtype(torch::kFloat32));
	if (!has_shs) shs = empty;
	if (!has_colors_precomp) colors_precomp = empty;
	if (!has_scales) scales = empty;
	if (!has_rotations) rotations = empty;
	if (!has_cov3D_precomp) cov3D_precomp = empty;
}

// No backward pass can follow: grad mode is off, or none of the differentiable inputs requires grad
bool no_backward(const std::initializer_list<const torch::Tensor*> inputs)
{
	if (!torch::GradMode::is_enabled()) return true;
	for (const torch::Tensor* t : inputs)
		if (t->defined() && t->requires_grad()) return false;
	return true;
}

// The body of GaussianRasterizer::forward, GaussianRasterizerEx::forward and forwardWithDepth.  ext == nullptr: the reference's
// rasterizer (its own autograd node, GaussianRasterizerFunction).  (color, radii, depth, alpha): the maps only with_depth.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor> rasterizer_forward(
    GaussianRasterizationSettings& s, const GaussianRasterizationExtensions* ext, bool with_depth, torch::Tensor means3D,
    torch::Tensor means2D, torch::Tensor opacities, bool has_shs, bool has_colors_precomp, bool has_scales, bool has_rotations,
    bool has_cov3D_precomp, torch::Tensor shs, torch::Tensor colors_precomp, torch::Tensor scales, torch::Tensor rotations,
    torch::Tensor cov3D_precomp)
{
	validate_and_fill(means3D, has_shs, has_colors_precomp, has_scales, has_rotations, has_cov3D_precomp, shs, colors_precomp,
	                  scales, rotations, cov3D_precomp);
	static const GaussianRasterizationExtensions none;
	const GaussianRasterizationExtensions& e = ext ? *ext : none;
	// forward_only_, or a render no backward pass can follow (NoGradGuard, or nothing to differentiate): the forward pass alone
	// (GSR_FORWARD_ONLY) -- RasterizeGaussiansCUDA directly with the bit, no autograd node, no buffers kept
	// (the camera counts only where a node exists that differentiates it: the reference-signature rasterizer, ext == nullptr, has
	// none -- GaussianRasterizerFunction keeps its nine inputs -- and decides as before)
	const bool camera_grad = ext && !no_backward({&s.viewmatrix_, &s.projmatrix_, &s.campos_});
	if (e.forward_only_ ||
	    (!camera_grad && no_backward({&means3D, &means2D, &shs, &colors_precomp, &opacities, &scales, &rotations, &cov3D_precomp}))) {
		torch::NoGradGuard no_grad;
		torch::Tensor depth, alpha;
		if (with_depth) {
			const auto opts = means3D.options().dtype(torch::kFloat32);
			depth = torch::zeros({s.image_height_, s.image_width_}, opts);
			alpha = torch::zeros({s.image_height_, s.image_width_}, opts);
		}
		auto r = rasterize_forward(means3D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, s, e, GSR_FORWARD_ONLY,
		                           depth, alpha);
		return std::make_tuple(std::get<1>(r), std::get<2>(r), depth, alpha);
	}
	// the camera is being differentiated (pose refinement): its three tensors enter the node as inputs
	if (camera_grad) {
		if (e.sh_grad_view_.defined())
			throw std::runtime_error("camera gradients are not available through the view-factored exchange (sh_grad_view_)");
		GaussianRasterizationExtensions node_ext = e;
		if (with_depth) node_ext.render_depth_ = true;
		auto result = GaussianRasterizerFunctionPose::apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
		                                                    cov3D_precomp, s.viewmatrix_, s.projmatrix_, s.campos_, s, std::move(node_ext));
		if (!with_depth) return std::make_tuple(result[0], result[1], torch::Tensor(), torch::Tensor());
		return std::make_tuple(result[0], result[1], result[2], result[3]);
	}
	if (!ext) {
		auto result = rasterizeGaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp, s);
		return std::make_tuple(result[0], result[1], torch::Tensor(), torch::Tensor());
	}
	GaussianRasterizationExtensions node_ext = e;   // the one copy of a forward pass: the autograd node takes it over
	if (with_depth) node_ext.render_depth_ = true;
	auto result = GaussianRasterizerFunctionEx::apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
	                                                  cov3D_precomp, s, std::move(node_ext));
	if (!with_depth) return std::make_tuple(result[0], result[1], torch::Tensor(), torch::Tensor());
	return std::make_tuple(result[0], result[1], result[2], result[3]);
}

}  // namespace

torch::autograd::tensor_list GaussianRasterizerFunction::forward(
    torch::autograd::AutogradContext* ctx, torch::Tensor means3D, torch::Tensor means2D, torch::Tensor sh,
    torch::Tensor colors_precomp, torch::Tensor opacities, torch::Tensor scales, torch::Tensor rotations,
    torch::Tensor cov3Ds_precomp, GaussianRasterizationSettings s)
{
	(void)means2D;  // only its gradient slot matters
	return forward_impl(ctx, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, std::move(s),
	                    GaussianRasterizationExtensions());
}

torch::autograd::tensor_list GaussianRasterizerFunction::backward(torch::autograd::AutogradContext* ctx,
                                                                  torch::autograd::tensor_list grad_outputs)
{
	return backward_impl(ctx, grad_outputs, 1);
}

torch::autograd::tensor_list GaussianRasterizerFunctionEx::forward(
    torch::autograd::AutogradContext* ctx, torch::Tensor means3D, torch::Tensor means2D, torch::Tensor sh,
    torch::Tensor colors_precomp, torch::Tensor opacities, torch::Tensor scales, torch::Tensor rotations,
    torch::Tensor cov3Ds_precomp, GaussianRasterizationSettings s, GaussianRasterizationExtensions e)
{
	(void)means2D;
	return forward_impl(ctx, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, std::move(s), std::move(e));
}

torch::autograd::tensor_list GaussianRasterizerFunctionEx::backward(torch::autograd::AutogradContext* ctx,
                                                                    torch::autograd::tensor_list grad_outputs)
{
	return backward_impl(ctx, grad_outputs, 2);
}

torch::autograd::tensor_list GaussianRasterizerFunctionPose::forward(
    torch::autograd::AutogradContext* ctx, torch::Tensor means3D, torch::Tensor means2D, torch::Tensor sh,
    torch::Tensor colors_precomp, torch::Tensor opacities, torch::Tensor scales, torch::Tensor rotations,
    torch::Tensor cov3Ds_precomp, torch::Tensor viewmatrix, torch::Tensor projmatrix, torch::Tensor campos,
    GaussianRasterizationSettings s, GaussianRasterizationExtensions e)
{
	(void)means2D;
	// (the values come from the settings, which hold the same three tensors; as inputs they give the node its edges)
	(void)viewmatrix; (void)projmatrix; (void)campos;
	return forward_impl(ctx, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, std::move(s), std::move(e));
}

torch::autograd::tensor_list GaussianRasterizerFunctionPose::backward(torch::autograd::AutogradContext* ctx,
                                                                      torch::autograd::tensor_list grad_outputs)
{
	return backward_impl(ctx, grad_outputs, 2, true);
}

std::tuple<torch::Tensor, torch::Tensor> GaussianRasterizer::forward(
    torch::Tensor means3D, torch::Tensor means2D, torch::Tensor opacities, bool has_shs, bool has_colors_precomp,
    bool has_scales, bool has_rotations, bool has_cov3D_precomp, torch::Tensor shs, torch::Tensor colors_precomp,
    torch::Tensor scales, torch::Tensor rotations, torch::Tensor cov3D_precomp)
{
	auto r = rasterizer_forward(raster_settings_, nullptr, false, means3D, means2D, opacities, has_shs, has_colors_precomp, has_scales,
	                            has_rotations, has_cov3D_precomp, shs, colors_precomp, scales, rotations, cov3D_precomp);
	return std::make_tuple(std::get<0>(r), std::get<1>(r));
}

std::tuple<torch::Tensor, torch::Tensor> GaussianRasterizerEx::forward(
    torch::Tensor means3D, torch::Tensor means2D, torch::Tensor opacities, bool has_shs, bool has_colors_precomp,
    bool has_scales, bool has_rotations, bool has_cov3D_precomp, torch::Tensor shs, torch::Tensor colors_precomp,
    torch::Tensor scales, torch::Tensor rotations, torch::Tensor cov3D_precomp)
{
	auto r = rasterizer_forward(raster_settings_, &extensions_, false, means3D, means2D, opacities, has_shs, has_colors_precomp,
	                            has_scales, has_rotations, has_cov3D_precomp, shs, colors_precomp, scales, rotations, cov3D_precomp);
	return std::make_tuple(std::get<0>(r), std::get<1>(r));
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor> GaussianRasterizerEx::forwardWithDepth(
    torch::Tensor means3D, torch::Tensor means2D, torch::Tensor opacities, bool has_shs, bool has_colors_precomp,
    bool has_scales, bool has_rotations, bool has_cov3D_precomp, torch::Tensor shs, torch::Tensor colors_precomp,
    torch::Tensor scales, torch::Tensor rotations, torch::Tensor cov3D_precomp)
{
	return rasterizer_forward(raster_settings_, &extensions_, true, means3D, means2D, opacities, has_shs, has_colors_precomp,
	                          has_scales, has_rotations, has_cov3D_precomp, shs, colors_precomp, scales, rotations, cov3D_precomp);
}
