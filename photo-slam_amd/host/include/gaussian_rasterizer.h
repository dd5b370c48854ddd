// gaussian_rasterizer.h -- GaussianRasterizationSettings / GaussianRasterizerFunction / rasterizeGaussians /
// GaussianRasterizer declared EXACTLY as the reference declares them (include/gaussian_rasterizer.h:25-127): same members
// in the same order (= the same object layout), same signatures (= the same mangled symbols), so that
// GaussianRenderer::render and the mapper call sites (src/gaussian_renderer.cpp:51-66,129-148) compile unchanged AND an
// object compiled against the reference's header links and runs against libphotoslam_host.so
// (tests/test_reference_link.py).  This repository's extensions live in the separate *Ex types below.
#pragma once
#include <torch/torch.h>

#include <tuple>
#include <vector>

#include "rasterize_points.h"

struct GaussianRasterizationSettings {
	GaussianRasterizationSettings(int image_height, int image_width, float tanfovx, float tanfovy, torch::Tensor& bg,
	                              float scale_modifier, torch::Tensor& viewmatrix, torch::Tensor& projmatrix,
	                              int sh_degree, torch::Tensor& campos, bool prefiltered)
	    : image_height_(image_height), image_width_(image_width), tanfovx_(tanfovx), tanfovy_(tanfovy), bg_(bg),
	      scale_modifier_(scale_modifier), viewmatrix_(viewmatrix), projmatrix_(projmatrix), sh_degree_(sh_degree),
	      campos_(campos), prefiltered_(prefiltered)
	{
	}
	int image_height_;
	int image_width_;
	float tanfovx_;
	float tanfovy_;
	torch::Tensor bg_;
	float scale_modifier_;
	torch::Tensor viewmatrix_;
	torch::Tensor projmatrix_;
	int sh_degree_;
	torch::Tensor campos_;
	bool prefiltered_;
};

class GaussianRasterizerFunction : public torch::autograd::Function<GaussianRasterizerFunction> {
public:
	static torch::autograd::tensor_list forward(torch::autograd::AutogradContext* ctx, torch::Tensor means3D,
	                                            torch::Tensor means2D, torch::Tensor sh, torch::Tensor colors_precomp,
	                                            torch::Tensor opacities, torch::Tensor scales, torch::Tensor rotations,
	                                            torch::Tensor cov3Ds_precomp,
	                                            GaussianRasterizationSettings raster_settings);
	static torch::autograd::tensor_list backward(torch::autograd::AutogradContext* ctx,
	                                             torch::autograd::tensor_list grad_out_color);
};

inline torch::autograd::tensor_list rasterizeGaussians(torch::Tensor& means3D, torch::Tensor& means2D, torch::Tensor& sh,
                                                       torch::Tensor& colors_precomp, torch::Tensor& opacities,
                                                       torch::Tensor& scales, torch::Tensor& rotations,
                                                       torch::Tensor& cov3Ds_precomp,
                                                       GaussianRasterizationSettings& raster_settings)
{
	return GaussianRasterizerFunction::apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
	                                         cov3Ds_precomp, raster_settings);
}

class GaussianRasterizer : public torch::nn::Module {
public:
	GaussianRasterizer(GaussianRasterizationSettings& raster_settings) : raster_settings_(raster_settings) {}

	torch::Tensor markVisibleGaussians(torch::Tensor& positions);

	std::tuple<torch::Tensor, torch::Tensor> forward(torch::Tensor means3D, torch::Tensor means2D, torch::Tensor opacities,
	                                                 bool has_shs, bool has_colors_precomp, bool has_scales,
	                                                 bool has_rotations, bool has_cov3D_precomp, torch::Tensor shs,
	                                                 torch::Tensor colors_precomp, torch::Tensor scales,
	                                                 torch::Tensor rotations, torch::Tensor cov3D_precomp);

public:
	GaussianRasterizationSettings raster_settings_;
};

// ---- extensions of this repository (none of them alters the types above) ------------------------------------------------
struct GaussianRasterizationExtensions {
	int raw_params_ = 0;   // GSR_RAW_* mask (activations fused into the rasterizer), see include/gsr.h
	// a [P,3] tensor that receives the clamp-masked colour gradient in backward; sh then gets no gradient from autograd --
	// the view-factored exchange of the data-parallel step rebuilds it (shGradFromViews)
	torch::Tensor sh_grad_view_;
	// optimizer-in-backward for the SH tensor (rasterize_points.h): set exp_avg to enable
	ShAdamStep sh_adam_;
	// {xyz_gradient_accum, denom, max_radii2D} -- backward adds this view's densification statistics itself
	std::vector<torch::Tensor> view_stats_;
	// optimizer-in-backward for xyz / opacity / scaling / rotation (rasterize_points.h): fill param to enable; those four then
	// get no gradient from autograd
	GeomAdamStep geom_adam_;
	// dL_dmeans2D and dL_dcov3D are not written either (means2D and cov3Ds_precomp get no gradient) -- for a caller that fuses
	// the densification statistics (view_stats_)
	bool training_outputs_only_ = false;
	// with sh_grad_view_ only (rasterize_points.h: RasterBackwardExtensions): the hipStream_t that waits for the point inside
	// backward at which sh_grad_view_ is complete, and the packed message backward writes next to it
	void* color_view_ready_stream_ = nullptr;
	torch::Tensor packed_view_;
	int64_t packed_capacity_ = 0;
	// GSR_CULL_EMPTY_TILES (include/gsr.h): instances of tiles in which no pixel can blend the Gaussian are dropped in front of
	// the tile sort -- the same image and the same gradients from shorter internal lists
	bool cull_empty_tiles_ = false;
	// persistent scratch buffers of a caller that renders iteration after iteration (rasterize_points.h: RasterWorkspace; the
	// caller owns it and keeps it alive until the backward pass has run); nullptr = fresh buffers per call, as the reference
	RasterWorkspace* workspace_ = nullptr;
	// GSR_FORWARD_ONLY (include/gsr.h): render without preparing a backward pass even with grad mode on -- for code shaped like
	// the reference's GaussianMapper::renderFromPose.  GaussianRasterizer(Ex)::forward also takes that path by itself when grad
	// mode is off or no input requires grad; the outputs then carry no grad_fn.
	bool forward_only_ = false;
	// the depth map sum z alpha T and the alpha map 1 - T_final (include/gsr.h: gsr_forward_args.out_depth / out_alpha) as two
	// more outputs of GaussianRasterizerFunctionEx -- (color, radii, depth, alpha), both maps differentiable; its backward takes
	// any subset of the three image gradients.  Set by GaussianRasterizerEx::forwardWithDepth (forward() renders no maps).
	bool render_depth_ = false;
	// GSR_ANTIALIAS (include/gsr.h): anti-aliased rendering -- the opacity of every Gaussian is multiplied by
	// sqrt(det Sigma / det(Sigma + 0.3 I)) of its projected covariance (upstream's `antialiasing`), in the forward pass, the
	// forward-only path and the backward pass alike
	bool antialiasing_ = false;
	// GSR_FILTER_3D (include/gsr.h): Mip-Splatting's 3-D smoothing filter, a float32 [P] tensor (GaussianModel::computeFilter3D) --
	// scales and opacity are filtered inside the rasterizer, in the forward pass, the forward-only path and the backward pass alike;
	// the gradients are those of the unfiltered leaves and the filter gets none (a non-differentiable input: it is not an
	// argument of the autograd nodes).  Not with cov3D_precomp or sh_grad_view_.  Undefined = off.
	torch::Tensor filter_3D_;
	// GSR_CONTRIBUTION (include/gsr.h; rasterize_points.h: RasterForwardExtensions): the per-Gaussian contribution statistics of the
	// render, left in the caller's [P] tensors (float32 / float32 / int32; any subset), with an optional [H,W] pixel weight map.
	// Not differentiable: nothing enters the autograd graph.
	torch::Tensor pixel_weight_, out_weight_sum_, out_weight_max_, out_n_touched_;
	bool contribution_accumulate_ = false;
	// the opacity / scale / isotropy regularisers on the Gaussians this view sees (gsr_backward_args.geom_reg, include/gsr.h): backward
	// adds their gradients to the opacity and scale gradients inside the pass (in front of the fused geom_adam_ step, if any).  The
	// lambdas are those of a MEAN over the visible Gaussians: the per-Gaussian weights are opacity_reg_ / V, scale_reg_ / (3 V) and
	// isotropic_reg_ / (3 V), V = max(visible count of the forward pass, 1).  All 0 and no loss = off.  reg_loss_: a float32 [3]
	// tensor that receives the three loss values; undefined = they are not formed.
	double opacity_reg_ = 0.0, scale_reg_ = 0.0, isotropic_reg_ = 0.0;
	torch::Tensor reg_loss_;
	bool hasGeomReg() const { return opacity_reg_ != 0.0 || scale_reg_ != 0.0 || isotropic_reg_ != 0.0 || reg_loss_.defined(); }
	// the absolute screen-space gradients (gsr_backward_args.dL_dmean2D_abs; AbsGS, gsplat's absgrad): a float32 [P,2] tensor of
	// the caller's that backward() fills -- what upstream leaves in `.absgrad` of the viewspace tensor (a C++ tensor carries no
	// attributes; the Python host does attach it there).  With view_stats_ the fused statistics accumulate the norm of this pair.
	// Undefined = off.  Not together with sh_grad_view_.
	torch::Tensor absgrad_;
};

class GaussianRasterizerFunctionEx : public torch::autograd::Function<GaussianRasterizerFunctionEx> {
public:
	static torch::autograd::tensor_list forward(torch::autograd::AutogradContext* ctx, torch::Tensor means3D,
	                                            torch::Tensor means2D, torch::Tensor sh, torch::Tensor colors_precomp,
	                                            torch::Tensor opacities, torch::Tensor scales, torch::Tensor rotations,
	                                            torch::Tensor cov3Ds_precomp, GaussianRasterizationSettings raster_settings,
	                                            GaussianRasterizationExtensions extensions);
	static torch::autograd::tensor_list backward(torch::autograd::AutogradContext* ctx,
	                                             torch::autograd::tensor_list grad_out_color);
};

// The rasterizer with the camera as a differentiable input: viewmatrix, projmatrix and campos (the settings' three tensors, passed
// as inputs so that their graph -- a pose built with torch ops, PoseDelta of gaussian_renderer.h -- continues behind them) get the
// gradients of gsr_backward_args.dL_dviewmatrix / dL_dprojmatrix / dL_dcampos.  GaussianRasterizerEx takes this node when one of
// the three requires grad; the reference-signature GaussianRasterizerFunction keeps its nine inputs and nine gradients.
class GaussianRasterizerFunctionPose : public torch::autograd::Function<GaussianRasterizerFunctionPose> {
public:
	static torch::autograd::tensor_list forward(torch::autograd::AutogradContext* ctx, torch::Tensor means3D,
	                                            torch::Tensor means2D, torch::Tensor sh, torch::Tensor colors_precomp,
	                                            torch::Tensor opacities, torch::Tensor scales, torch::Tensor rotations,
	                                            torch::Tensor cov3Ds_precomp, torch::Tensor viewmatrix, torch::Tensor projmatrix,
	                                            torch::Tensor campos, GaussianRasterizationSettings raster_settings,
	                                            GaussianRasterizationExtensions extensions);
	static torch::autograd::tensor_list backward(torch::autograd::AutogradContext* ctx,
	                                             torch::autograd::tensor_list grad_out_color);
};

// GaussianRasterizer with the extensions: same forward() contract and exception texts
class GaussianRasterizerEx : public GaussianRasterizer {
public:
	GaussianRasterizerEx(GaussianRasterizationSettings& raster_settings, const GaussianRasterizationExtensions& extensions)
	    : GaussianRasterizer(raster_settings), extensions_(extensions)
	{
	}
	std::tuple<torch::Tensor, torch::Tensor> forward(torch::Tensor means3D, torch::Tensor means2D, torch::Tensor opacities,
	                                                 bool has_shs, bool has_colors_precomp, bool has_scales,
	                                                 bool has_rotations, bool has_cov3D_precomp, torch::Tensor shs,
	                                                 torch::Tensor colors_precomp, torch::Tensor scales,
	                                                 torch::Tensor rotations, torch::Tensor cov3D_precomp);
	// forward() with the depth and alpha maps: (color, radii, depth, alpha), [H,W] each (extensions_.render_depth_); under
	// NoGradGuard / forward_only_ / no input requiring grad the forward-only path renders the same maps
	std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor> forwardWithDepth(
	    torch::Tensor means3D, torch::Tensor means2D, torch::Tensor opacities, bool has_shs, bool has_colors_precomp,
	    bool has_scales, bool has_rotations, bool has_cov3D_precomp, torch::Tensor shs, torch::Tensor colors_precomp,
	    torch::Tensor scales, torch::Tensor rotations, torch::Tensor cov3D_precomp);
	GaussianRasterizationExtensions extensions_;
};
