// ops_register.cpp -- exposes the C++ host layer to Python (torch.ops.photoslam_amd.*) so that the
// test-suite and bench.py can drive the very code a C++ caller (gaussian_mapper) would link against.
#include <torch/library.h>
#include "loss_utils.h"
#include <torch/torch.h>

#include <map>
#include <mutex>

#include "gaussian_model_lite.h"
#include "gaussian_renderer.h"
#include "keyframe_scheduler.h"
#include <torch/csrc/distributed/c10d/GroupRegistry.hpp>
#include "operate_points.h"
#include "spatial.h"
#include "stereo_vision.h"

namespace {

// ---- what the four rasterize_gaussians* ops share: the extensions their raw_params argument names (GSR_RAW_* in bits 1|2|4,
// GSR_CULL_EMPTY_TILES in 8, GSR_ANTIALIAS in 256), their eighteen leading arguments, and the forward call on them (a tensor without
// elements = not given; ext null = the reference's GaussianRasterizer)
GaussianRasterizationExtensions decode_raw_params(int64_t raw_params)
{
	GaussianRasterizationExtensions e;
	e.raw_params_ = (int)raw_params & 7;
	e.cull_empty_tiles_ = (raw_params & 8) != 0;
	e.antialiasing_ = (raw_params & 256) != 0;
	return e;
}
bool has(const torch::Tensor& t) { return t.defined() && t.numel() != 0; }
struct RasterArgs {
	torch::Tensor means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, bg;
	double scale_modifier;
	torch::Tensor viewmatrix, projmatrix;
	double tanfovx, tanfovy;
	int64_t image_height, image_width, sh_degree;
	torch::Tensor campos;
};
std::tuple<torch::Tensor, torch::Tensor> forward(RasterArgs in, const GaussianRasterizationExtensions* ext, bool prefiltered = false)
{
	GaussianRasterizationSettings s((int)in.image_height, (int)in.image_width, (float)in.tanfovx, (float)in.tanfovy, in.bg, (float)in.scale_modifier,
	                                in.viewmatrix, in.projmatrix, (int)in.sh_degree, in.campos, prefiltered);
	auto call = [&](auto&& r) {
		return r.forward(in.means3D, in.means2D, in.opacities, has(in.sh), has(in.colors_precomp), has(in.scales), has(in.rotations),
		                 has(in.cov3Ds_precomp), in.sh, in.colors_precomp, in.scales, in.rotations, in.cov3Ds_precomp);
	};
	return ext ? call(GaussianRasterizerEx(s, *ext)) : call(GaussianRasterizer(s));
}

std::tuple<torch::Tensor, torch::Tensor> rasterize_gaussians(
    torch::Tensor means3D, torch::Tensor means2D, torch::Tensor sh, torch::Tensor colors_precomp, torch::Tensor opacities,
    torch::Tensor scales, torch::Tensor rotations, torch::Tensor cov3Ds_precomp, torch::Tensor bg, double scale_modifier,
    torch::Tensor viewmatrix, torch::Tensor projmatrix, double tanfovx, double tanfovy, int64_t image_height, int64_t image_width,
    int64_t sh_degree, torch::Tensor campos, bool prefiltered)
{
	return forward({means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, bg, scale_modifier, viewmatrix, projmatrix,
	                tanfovx, tanfovy, image_height, image_width, sh_degree, campos}, nullptr, prefiltered);
}

// GaussianRasterizer(Ex)::forward as a caller of the forward-only path reaches it: ex = GaussianRasterizerEx with raw_params /
// GSR_CULL_EMPTY_TILES / forward_only_ (extension_forward_only), otherwise the reference's GaussianRasterizer; no_grad = under
// torch::NoGradGuard.  (image, radii)
std::tuple<torch::Tensor, torch::Tensor> rasterize_gaussians_modes(
    torch::Tensor means3D, torch::Tensor means2D, torch::Tensor sh, torch::Tensor colors_precomp, torch::Tensor opacities,
    torch::Tensor scales, torch::Tensor rotations, torch::Tensor cov3Ds_precomp, torch::Tensor bg, double scale_modifier,
    torch::Tensor viewmatrix, torch::Tensor projmatrix, double tanfovx, double tanfovy, int64_t image_height, int64_t image_width,
    int64_t sh_degree, torch::Tensor campos, bool ex, int64_t raw_params, bool extension_forward_only, bool no_grad)
{
	c10::optional<torch::NoGradGuard> guard;
	if (no_grad) guard.emplace();
	GaussianRasterizationExtensions e = decode_raw_params(raw_params);
	e.forward_only_ = extension_forward_only;
	return forward({means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, bg, scale_modifier, viewmatrix, projmatrix,
	                tanfovx, tanfovy, image_height, image_width, sh_degree, campos}, ex ? &e : nullptr);
}

// rasterize_gaussians_modes (ex) with the contribution statistics (GaussianRasterizationExtensions::out_weight_sum_ ...): stats =
// {pixel_weight, out_weight_sum, out_weight_max, out_n_touched}, a tensor without elements = not given.  (image, radii)
std::tuple<torch::Tensor, torch::Tensor> rasterize_gaussians_contribution(
    torch::Tensor means3D, torch::Tensor means2D, torch::Tensor sh, torch::Tensor colors_precomp, torch::Tensor opacities,
    torch::Tensor scales, torch::Tensor rotations, torch::Tensor cov3Ds_precomp, torch::Tensor bg, double scale_modifier,
    torch::Tensor viewmatrix, torch::Tensor projmatrix, double tanfovx, double tanfovy, int64_t image_height, int64_t image_width,
    int64_t sh_degree, torch::Tensor campos, int64_t raw_params, bool extension_forward_only, std::vector<torch::Tensor> stats,
    bool accumulate)
{
	TORCH_CHECK(stats.size() == 4, "stats: {pixel_weight, out_weight_sum, out_weight_max, out_n_touched}");
	torch::NoGradGuard guard;
	GaussianRasterizationExtensions e = decode_raw_params(raw_params);
	e.forward_only_ = extension_forward_only;
	if (has(stats[0])) e.pixel_weight_ = stats[0];
	if (has(stats[1])) e.out_weight_sum_ = stats[1];
	if (has(stats[2])) e.out_weight_max_ = stats[2];
	if (has(stats[3])) e.out_n_touched_ = stats[3];
	e.contribution_accumulate_ = accumulate;
	return forward({means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, bg, scale_modifier, viewmatrix, projmatrix,
	                tanfovx, tanfovy, image_height, image_width, sh_degree, campos}, &e);
}
// rasterize_gaussians_modes (ex) with the absolute screen-space gradients: backward() of the returned image fills `absgrad`
// ([P,2], GaussianRasterizationExtensions::absgrad_).  (image, radii)
std::tuple<torch::Tensor, torch::Tensor> rasterize_gaussians_absgrad(
    torch::Tensor means3D, torch::Tensor means2D, torch::Tensor sh, torch::Tensor colors_precomp, torch::Tensor opacities,
    torch::Tensor scales, torch::Tensor rotations, torch::Tensor cov3Ds_precomp, torch::Tensor bg, double scale_modifier,
    torch::Tensor viewmatrix, torch::Tensor projmatrix, double tanfovx, double tanfovy, int64_t image_height, int64_t image_width,
    int64_t sh_degree, torch::Tensor campos, int64_t raw_params, torch::Tensor absgrad)
{
	GaussianRasterizationExtensions e = decode_raw_params(raw_params);
	e.absgrad_ = absgrad;
	return forward({means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, bg, scale_modifier, viewmatrix, projmatrix,
	                tanfovx, tanfovy, image_height, image_width, sh_degree, campos}, &e);
}
double covisibility_op(torch::Tensor a, torch::Tensor b) { return covisibility(a, b); }

torch::Tensor mark_visible(torch::Tensor means3D, torch::Tensor viewmatrix, torch::Tensor projmatrix)
{
	return markVisible(means3D, viewmatrix, projmatrix);
}
torch::Tensor dist_cuda2(torch::Tensor points) { return distCUDA2(points); }
torch::Tensor l1_ssim_loss(torch::Tensor rendered, torch::Tensor gt, torch::Tensor mask, double lambda_dssim)
{
	return fusedL1SSIMLoss(rendered, gt, mask, (float)lambda_dssim);
}
torch::Tensor l1_ssim_loss_exposure(torch::Tensor rendered, torch::Tensor gt, torch::Tensor mask, double lambda_dssim,
                                    torch::Tensor exposure, bool is_root)
{
	return loss_utils::fused_l1_ssim_exposure(rendered, gt, mask, (float)lambda_dssim, exposure, is_root);
}
torch::Tensor apply_exposure(torch::Tensor image, torch::Tensor exposure) { return loss_utils::apply_exposure(image, exposure); }
// loss_utils::depth_prior and its companions (alpha, valid with no elements = not given): (loss, fit [4])
std::tuple<torch::Tensor, torch::Tensor> depth_prior_loss(torch::Tensor depth, torch::Tensor alpha, torch::Tensor prior, double weight,
                                                          bool inverse, bool pearson, double alpha_min, torch::Tensor valid)
{
	torch::Tensor fit;
	auto loss = loss_utils::depth_prior(depth, alpha, prior, (float)weight, inverse, pearson, (float)alpha_min, valid, &fit);
	return std::make_tuple(loss, fit);
}
torch::Tensor depth_prior_fit(torch::Tensor depth, torch::Tensor alpha, torch::Tensor prior, bool inverse, double alpha_min, torch::Tensor valid)
{
	return loss_utils::depth_prior_fit(depth, alpha, prior, inverse, (float)alpha_min, valid);
}
torch::Tensor depth_prior_apply(torch::Tensor prior, torch::Tensor fit, bool inverse, bool in_place)
{
	return loss_utils::depth_prior_apply(prior, fit, inverse, in_place);
}

torch::Tensor transform_points(torch::Tensor points, torch::Tensor transformmatrix)
{
	transformPoints(points, transformmatrix);
	return points;
}
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, int64_t> scale_transform_mark_visible(
    torch::Tensor points, torch::Tensor rots, torch::Tensor not_transformed, torch::Tensor unstable, torch::Tensor transform,
    torch::Tensor view, torch::Tensor proj, int64_t num_transformed, double scale)
{
	int n = (int)num_transformed;
	scaleAndTransformThenMarkVisiblePoints(points, rots, not_transformed, unstable, transform, view, proj, n, (float)scale);
	return std::make_tuple(points, rots, not_transformed, (int64_t)n);
}
torch::Tensor reproject_depth_pinhole(torch::Tensor depth, torch::Tensor mask, std::vector<double> intr, int64_t width)
{
	std::vector<float> f(intr.begin(), intr.end());
	return reprojectDepthPinhole(depth, mask, f, (int)width);
}
std::tuple<torch::Tensor, torch::Tensor> neighborhood_keypoints(torch::Tensor px, torch::Tensor has, torch::Tensor p3,
                                                                torch::Tensor colors, double max_dist, std::vector<double> intr,
                                                                int64_t width)
{
	std::vector<float> f(intr.begin(), intr.end());
	return monocularPinholeInactiveGeoDensifyBySearchingNeighborhoodKeypoints(px, has, p3, colors, (float)max_dist, f, (int)width);
}

// ---- a C++ TrainStep behind an integer handle
std::mutex g_mu;
std::map<int64_t, std::shared_ptr<TrainStep>> g_trainers;
int64_t g_next = 1;

// a TrainStep around the model behind a new handle
int64_t adopt(std::shared_ptr<GaussianModel> model, torch::Tensor background)
{
	std::lock_guard<std::mutex> lk(g_mu);
	g_trainers[g_next] = std::make_shared<TrainStep>(model, background);
	return g_next++;
}
// an op returns no undefined tensor: an empty one of the given dtype on `like`'s device stands for it
torch::Tensor or_empty(const torch::Tensor& t, const torch::Tensor& like, c10::optional<torch::ScalarType> dtype = c10::nullopt,
                       at::IntArrayRef shape = {0})
{
	return t.defined() ? t : torch::empty(shape, like.options().dtype(dtype.value_or(like.scalar_type())).requires_grad(false));
}

int64_t trainer_create(torch::Tensor xyz, torch::Tensor features, torch::Tensor opacity, torch::Tensor scaling,
                       torch::Tensor rotation, int64_t sh_degree, double spatial_lr_scale, torch::Tensor background)
{
	auto model = std::make_shared<GaussianModel>((int)sh_degree, xyz, features, opacity, scaling, rotation,
	                                             (float)spatial_lr_scale);
	model->trainingSetup(GaussianOptimizationParams());
	return adopt(model, background);
}
int64_t trainer_create_from_pcd(torch::Tensor points, torch::Tensor colors, int64_t sh_degree, double spatial_lr_scale,
                                torch::Tensor background)
{
	auto model = std::make_shared<GaussianModel>((int)sh_degree);
	model->createFromPcd(points, colors, (float)spatial_lr_scale);
	model->trainingSetup(GaussianOptimizationParams());
	return adopt(model, background);
}
// a generator of the tensors' device seeded like torch.Generator(device).manual_seed(seed)
at::Generator make_generator(const torch::Device& device, int64_t seed)
{
	auto gen = at::globalContext().defaultGenerator(device).clone();
	gen.set_current_seed(static_cast<uint64_t>(seed));
	return gen;
}
std::shared_ptr<TrainStep> get(int64_t h)
{
	std::lock_guard<std::mutex> lk(g_mu);
	auto it = g_trainers.find(h);
	TORCH_CHECK(it != g_trainers.end(), "unknown trainer handle");
	return it->second;
}
std::shared_ptr<GaussianKeyframe> make_kf(torch::Tensor view, torch::Tensor proj, torch::Tensor campos, double fovx,
                                          double fovy, int64_t H, int64_t W)
{
	auto kf = std::make_shared<GaussianKeyframe>();
	kf->image_height_ = (int)H;
	kf->image_width_ = (int)W;
	kf->FoVx_ = (float)fovx;
	kf->FoVy_ = (float)fovy;
	kf->world_view_transform_ = view;
	kf->full_proj_transform_ = proj;
	kf->camera_center_ = campos;
	return kf;
}
torch::Tensor trainer_render_and_backward(int64_t h, torch::Tensor view, torch::Tensor proj, torch::Tensor campos,
                                          double fovx, double fovy, int64_t H, int64_t W, torch::Tensor gt,
                                          torch::Tensor mask)
{
	return get(h)->renderAndBackward(make_kf(view, proj, campos, fovx, fovy, H, W), gt, mask).detach();
}
// ... for an RGB-D keyframe: the depth loss (depth_loss_weight / depth_min / depth_max of trainer_set_options) joins the RGB loss
torch::Tensor trainer_render_and_backward_depth(int64_t h, torch::Tensor view, torch::Tensor proj, torch::Tensor campos, double fovx,
                                                double fovy, int64_t H, int64_t W, torch::Tensor gt, torch::Tensor mask,
                                                torch::Tensor gt_depth)
{
	return get(h)->renderAndBackward(make_kf(view, proj, campos, fovx, fovy, H, W), gt, mask, gt_depth).detach();
}
// TrainStep::trainForOneIteration with a sensor depth and / or a monocular prior (no elements = not given)
torch::Tensor trainer_train_depth_prior(int64_t h, torch::Tensor view, torch::Tensor proj, torch::Tensor campos, double fovx, double fovy,
                                        int64_t H, int64_t W, torch::Tensor gt, torch::Tensor mask, torch::Tensor gt_depth,
                                        torch::Tensor prior_depth)
{
	return get(h)->trainForOneIteration(make_kf(view, proj, campos, fovx, fovy, H, W), gt, mask, gt_depth.numel() ? gt_depth : torch::Tensor(),
	                                    prior_depth.numel() ? prior_depth : torch::Tensor()).detach();
}
// TrainStep::lastDepthPriorFit: [s, t, rho, n] of the last step with the depth-prior term, or an empty tensor
torch::Tensor trainer_last_depth_prior_fit(int64_t h)
{
	auto t = get(h);
	return or_empty(t->lastDepthPriorFit(), t->gaussians_->xyz_);
}
// TrainStep::alignDepthPrior: (the metric map, fit)
std::tuple<torch::Tensor, torch::Tensor> trainer_align_depth_prior(int64_t h, torch::Tensor view, torch::Tensor proj, torch::Tensor campos,
                                                                   double fovx, double fovy, int64_t H, int64_t W, torch::Tensor prior)
{
	return get(h)->alignDepthPrior(make_kf(view, proj, campos, fovx, fovy, H, W), prior);
}
// TrainStep::lastAbsgrad: the [P,2] absolute screen-space gradients of the last step that formed them, or an empty tensor
torch::Tensor trainer_last_absgrad(int64_t h)
{
	auto t = get(h);
	return or_empty(t->lastAbsgrad(), t->gaussians_->xyz_, c10::nullopt, {0, 2});
}
// TrainStep::lastRegLosses: the three regulariser terms of the last step ([3]), or an empty tensor when they were not formed
torch::Tensor trainer_last_reg_losses(int64_t h)
{
	auto t = get(h);
	return or_empty(t->lastRegLosses(), t->gaussians_->xyz_);
}
// the extensions of the two ops that call GaussianRenderer::render themselves: the trainer's antialiasing_ and filter, neither its
// cull_empty_tiles_ nor a workspace
GaussianRasterizationExtensions render_extensions(TrainStep& t, int raw_params)
{
	GaussianRasterizationExtensions ext;
	ext.raw_params_ = raw_params;
	ext.antialiasing_ = t.antialiasing_;
	ext.filter_3D_ = t.viewFilter3D();
	return ext;
}
// GaussianRenderer::render on the trainer's model with the pipeline flags of GaussianPipelineParams (convert_SHs_,
// compute_cov3D_: src/gaussian_renderer.cpp:78-113): (image, radii); the image is attached to the model's leaves
std::tuple<torch::Tensor, torch::Tensor> trainer_render(int64_t h, torch::Tensor view, torch::Tensor proj, torch::Tensor campos,
                                                        double fovx, double fovy, int64_t H, int64_t W, bool convert_SHs,
                                                        bool compute_cov3D, bool fuse_activations)
{
	auto t = get(h);
	GaussianPipelineParams pipe;
	pipe.convert_SHs_ = convert_SHs;
	pipe.compute_cov3D_ = compute_cov3D;
	torch::Tensor override_color;
	auto pkg = GaussianRenderer::render(make_kf(view, proj, campos, fovx, fovy, H, W), (int)H, (int)W, t->gaussians_, pipe,
	                                    t->background_, override_color, 1.0f, false, render_extensions(*t, fuse_activations ? 7 : 0));
	return std::make_tuple(std::get<0>(pkg), std::get<3>(pkg));
}
// TrainStep::renderView: a forward-only render of the current model into the trainer's second workspace (the image, detached)
torch::Tensor trainer_render_view(int64_t h, torch::Tensor view, torch::Tensor proj, torch::Tensor campos, double fovx, double fovy,
                                  int64_t H, int64_t W)
{
	return get(h)->renderView(make_kf(view, proj, campos, fovx, fovy, H, W));
}
// ---- keyframes that carry an exposure.  The ops build a keyframe per call, so its exposure state travels as arguments:
// state = {exposure [3,4], exp_avg, exp_avg_sq}, each possibly empty (= undefined), and the keyframe's step count; tensors given are
// updated in place, and the state after the call comes back (an exposure created at first use among it).
std::shared_ptr<GaussianKeyframe> with_exposure(std::shared_ptr<GaussianKeyframe> kf, const std::vector<torch::Tensor>& state, int64_t step)
{
	TORCH_CHECK(state.size() == 3, "exposure state: {exposure, exp_avg, exp_avg_sq}");
	if (state[0].numel()) kf->exposure_ = state[0];
	if (state[1].numel()) kf->exposure_exp_avg_ = state[1];
	if (state[2].numel()) kf->exposure_exp_avg_sq_ = state[2];
	kf->exposure_step_ = (int)step;
	return kf;
}
// TrainStep::trainForOneIteration on such a keyframe: (loss, exposure, exp_avg, exp_avg_sq, [step])
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, int64_t> trainer_train_exposure(
    int64_t h, torch::Tensor view, torch::Tensor proj, torch::Tensor campos, double fovx, double fovy, int64_t H, int64_t W,
    torch::Tensor gt, torch::Tensor mask, std::vector<torch::Tensor> state, int64_t step)
{
	auto kf = with_exposure(make_kf(view, proj, campos, fovx, fovy, H, W), state, step);
	auto loss = get(h)->trainForOneIteration(kf, gt, mask).detach();
	return std::make_tuple(loss, or_empty(kf->exposure_, gt), or_empty(kf->exposure_exp_avg_, gt), or_empty(kf->exposure_exp_avg_sq_, gt),
	                       (int64_t)kf->exposure_step_);
}
torch::Tensor trainer_render_view_exposure(int64_t h, torch::Tensor view, torch::Tensor proj, torch::Tensor campos, double fovx,
                                           double fovy, int64_t H, int64_t W, torch::Tensor exposure, bool apply_exposure)
{
	auto kf = make_kf(view, proj, campos, fovx, fovy, H, W);
	if (exposure.numel()) kf->exposure_ = exposure;
	return get(h)->renderView(kf, apply_exposure);
}
std::tuple<torch::Tensor, torch::Tensor> trainer_refine_pose_exposure(int64_t h, torch::Tensor view, torch::Tensor proj,
                                                                      torch::Tensor campos, double fovx, double fovy, int64_t H,
                                                                      int64_t W, torch::Tensor gt, torch::Tensor mask,
                                                                      int64_t iterations, double lr_translation, double lr_rotation,
                                                                      torch::Tensor exposure)
{
	auto kf = make_kf(view, proj, campos, fovx, fovy, H, W);
	if (exposure.numel()) kf->exposure_ = exposure;
	return get(h)->refinePose(kf, gt, mask, (int)iterations, lr_translation, lr_rotation);
}
// the keyframes of the two ops below: views / projs [K,4,4], campos [K,3], one field of view and size for all
std::vector<std::shared_ptr<GaussianKeyframe>> make_kfs(const torch::Tensor& views, const torch::Tensor& projs, const torch::Tensor& campos,
                                                        double fovx, double fovy, int64_t H, int64_t W)
{
	std::vector<std::shared_ptr<GaussianKeyframe>> kfs;
	for (int64_t i = 0; i < views.size(0); i++) kfs.push_back(make_kf(views[i].contiguous(), projs[i].contiguous(), campos[i].contiguous(), fovx, fovy, H, W));
	return kfs;
}
// TrainStep::scoreContribution: (weight_sum, weight_max, n_touched, views_seen); pixel_weights: empty, or one map per keyframe (a
// tensor without elements = ones)
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor> trainer_score_contribution(
    int64_t h, torch::Tensor views, torch::Tensor projs, torch::Tensor campos, double fovx, double fovy, int64_t H, int64_t W,
    std::vector<torch::Tensor> pixel_weights)
{
	return get(h)->scoreContribution(make_kfs(views, projs, campos, fovx, fovy, H, W), pixel_weights);
}
// TrainStep::pruneUncontributing: the number of Gaussians removed
int64_t trainer_prune_uncontributing(int64_t h, torch::Tensor views, torch::Tensor projs, torch::Tensor campos, double fovx, double fovy,
                                     int64_t H, int64_t W, double min_weight_max, int64_t min_views)
{
	return get(h)->pruneUncontributing(make_kfs(views, projs, campos, fovx, fovy, H, W), (float)min_weight_max, (int)min_views);
}
double trainer_exposure_lr(int64_t h, int64_t step) { return get(h)->exposureLearningRate((int)step); }
// TrainStep::renderViewWithDepth: (image, depth, alpha) of a forward-only render into the second workspace
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> trainer_render_view_depth(int64_t h, torch::Tensor view, torch::Tensor proj,
                                                                                  torch::Tensor campos, double fovx, double fovy,
                                                                                  int64_t H, int64_t W)
{
	return get(h)->renderViewWithDepth(make_kf(view, proj, campos, fovx, fovy, H, W));
}
// TrainStep::refinePose: (the refined W2C [4,4], the loss per iteration); gt_depth with no elements = none
std::tuple<torch::Tensor, torch::Tensor> trainer_refine_pose(int64_t h, torch::Tensor view, torch::Tensor proj, torch::Tensor campos,
                                                             double fovx, double fovy, int64_t H, int64_t W, torch::Tensor gt,
                                                             torch::Tensor mask, int64_t iterations, double lr_translation,
                                                             double lr_rotation, torch::Tensor gt_depth)
{
	return get(h)->refinePose(make_kf(view, proj, campos, fovx, fovy, H, W), gt, mask, (int)iterations, lr_translation, lr_rotation,
	                          gt_depth.numel() ? gt_depth : torch::Tensor());
}
// every tensor a refinement must leave alone: the five leaves as they are, their Adam moments, the lazy rows' counters, the
// training workspace
std::vector<torch::Tensor> trainer_state(int64_t h)
{
	auto t = get(h);
	std::vector<torch::Tensor> out = t->gaussians_->paramsRaw();
	for (auto& grp : t->gaussians_->groups_) {
		out.push_back(grp.exp_avg);
		out.push_back(grp.exp_avg_sq);
	}
	if (t->gaussians_->features_row_step_.defined()) out.push_back(t->gaussians_->features_row_step_);
	for (const torch::Tensor* b : {&t->workspace_.geom, &t->workspace_.binning, &t->workspace_.img})
		if (b->defined()) out.push_back(*b);
	return out;
}
// the camera gradients of a loss <dL_dpix, image> through GaussianRasterizerEx with a PoseDelta at xi = 0 on the trainer's model:
// dL/dxi [6] (the autograd route of the C++ host)
torch::Tensor trainer_pose_gradient(int64_t h, torch::Tensor view, torch::Tensor proj, torch::Tensor campos, double fovx, double fovy,
                                    int64_t H, int64_t W, torch::Tensor dL_dpix)
{
	auto t = get(h);
	auto kf = make_kf(view, proj, campos, fovx, fovy, H, W);
	PoseDelta pose(kf->world_view_transform_, kf->full_proj_transform_);
	pose.apply(*kf);
	torch::Tensor override_color;
	const GaussianRasterizationExtensions ext = render_extensions(*t, 7);
	// (the map frozen for this render: only the camera requires grad; the leaves get their flags back on every way out of it)
	auto frozen = t->gaussians_;
	auto leaves = frozen->paramsRaw();
	std::vector<bool> was;
	for (auto& p : leaves) { was.push_back(p.requires_grad()); p.set_requires_grad(false); }
	std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor> pkg;
	{
		ScopeExit restore{[&] { for (size_t i = 0; i < leaves.size(); i++) leaves[i].set_requires_grad(was[i]); }};
		pkg = GaussianRenderer::render(kf, (int)H, (int)W, frozen, t->pipe_, t->background_, override_color, 1.0f, false, ext);
	}
	TORCH_CHECK(std::get<0>(pkg).requires_grad(), "a render in which only the camera requires grad must take the training path");
	return torch::autograd::grad({(std::get<0>(pkg) * dL_dpix).sum()}, {pose.xi_})[0];
}
void trainer_finish(int64_t h) { get(h)->finishOneIteration(); }
void trainer_finish_begin(int64_t h) { get(h)->finishBegin(); }
void trainer_adam_group(int64_t h, int64_t group) { get(h)->finishAdamGroup(static_cast<int>(group)); }
void trainer_finish_end(int64_t h) { get(h)->finishEnd(); }
std::vector<torch::Tensor> trainer_params(int64_t h) { return get(h)->gaussians_->params(); }
std::vector<torch::Tensor> trainer_grads(int64_t h)
{
	std::vector<torch::Tensor> g;
	// (features_ has no gradient yet in the factored mode: an empty tensor keeps the positions)
	for (auto& p : get(h)->gaussians_->paramsRaw()) g.push_back(or_empty(p.grad(), p));
	return g;
}
// densification: options of the schedule (names of GaussianOptimizationParams / GaussianMapper without the trailing
// underscore; unknown keys are refused), and the single operations for the parity tests
void trainer_set_options(int64_t h, c10::Dict<std::string, double> o)
{
	auto t = get(h);
	auto& p = t->gaussians_->opt_;
	for (const auto& kv : o) {
		const std::string& k = kv.key();
		const double v = kv.value();
		if (k == "densify") t->densify_ = v != 0.0;
		else if (k == "fused_sh_adam") t->fused_sh_adam_ = v != 0.0;
		else if (k == "lazy_sh_adam_window") t->lazy_sh_adam_window_ = (int)v;
		else if (k == "fused_geom_adam") t->fused_geom_adam_ = v != 0.0;
		else if (k == "active_sh_degree") t->gaussians_->active_sh_degree_ = std::min((int)v, t->gaussians_->max_sh_degree_);
		else if (k == "cull_empty_tiles") t->cull_empty_tiles_ = v != 0.0;
		else if (k == "antialiasing") t->antialiasing_ = v != 0.0;
		else if (k == "filter3d") t->filter3d_ = v != 0.0;
		else if (k == "filter3d_interval") t->filter3d_interval_ = static_cast<int>(v);
		else if (k == "filter3d_variance") t->filter3d_variance_ = static_cast<float>(v);
		else if (k == "optimize_exposure") t->optimize_exposure_ = v != 0.0;
		else if (k == "exposure_lr_init") t->exposure_lr_init_ = static_cast<float>(v);
		else if (k == "exposure_lr_final") t->exposure_lr_final_ = static_cast<float>(v);
		else if (k == "exposure_lr_max_steps") t->exposure_lr_max_steps_ = (int)v;
		else if (k == "opacity_reg") t->opacity_reg_ = v;
		else if (k == "scale_reg") t->scale_reg_ = v;
		else if (k == "isotropic_reg") t->isotropic_reg_ = v;
		else if (k == "read_reg_losses") t->read_reg_losses_ = v != 0.0;
		else if (k == "absgrad") t->absgrad_ = v != 0.0;
		else if (k == "densify_abs_grad_threshold") t->densify_abs_grad_threshold_ = (float)v;
		else if (k == "mcmc") t->mcmc_ = v != 0.0;
		else if (k == "mcmc_cap_max") t->mcmc_cap_max_ = (int64_t)v;
		else if (k == "mcmc_noise_lr") t->mcmc_noise_lr_ = v;
		else if (k == "mcmc_min_opacity") t->mcmc_min_opacity_ = (float)v;
		else if (k == "seed_alpha_threshold") t->seed_alpha_threshold_ = (float)v;
		else if (k == "seed_depth_median_factor") t->seed_depth_median_factor_ = (float)v;
		else if (k == "seed_depth_error_abs") t->seed_depth_error_abs_ = (float)v;
		else if (k == "seed_stride") t->seed_stride_ = (int)v;
		else if (k == "seed_scale_factor") t->seed_scale_factor_ = (float)v;
		else if (k == "seed_init_opacity") t->seed_init_opacity_ = (float)v;
		else if (k == "seed_max_new") t->seed_max_new_ = (int64_t)v;
		else if (k == "depth_loss_weight") t->depth_loss_weight_ = static_cast<float>(v);
		else if (k == "depth_min") t->depth_min_ = static_cast<float>(v);
		else if (k == "depth_max") t->depth_max_ = static_cast<float>(v);
		else if (k == "depth_prior_weight") t->depth_prior_weight_ = static_cast<float>(v);
		else if (k == "depth_prior_pearson") t->depth_prior_pearson_ = v != 0.0;
		else if (k == "depth_prior_inverse") t->depth_prior_inverse_ = v != 0.0;
		else if (k == "depth_prior_alpha_min") t->depth_prior_alpha_min_ = static_cast<float>(v);
		else if (k == "persistent_workspace") t->persistent_workspace_ = v != 0.0;
		else if (k == "early_gather") t->early_gather_ = v != 0.0;
		else if (k == "packed_exchange") t->packed_exchange_ = v != 0.0;
		else if (k == "pack_in_backward") t->pack_in_backward_ = v != 0.0;
		else if (k == "lazy_slice_late") t->lazy_slice_late_ = v != 0.0;
		else if (k == "no_side_stream") t->no_side_stream_ = v != 0.0;
		else if (k == "profile_exchange") t->profile_exchange_ = v != 0.0;
		else if (k == "convert_SHs") t->pipe_.convert_SHs_ = v != 0.0;
		else if (k == "compute_cov3D") t->pipe_.compute_cov3D_ = v != 0.0;
		else if (k == "cameras_extent") t->cameras_extent_ = (float)v;
		else if (k == "position_lr_step") t->position_lr_step_ = (int)v;
		else if (k == "morton_reindex") t->gaussians_->morton_reindex_ = v != 0.0;
		else if (k == "lr_scale") t->gaussians_->lr_scale_ = v;
		else if (k == "densify_min_opacity") t->densify_min_opacity_ = (float)v;
		else if (k == "prune_big_point_after_iter") t->prune_big_point_after_iter_ = (int)v;
		else if (k == "seed") t->generator_ = make_generator(t->gaussians_->xyz_.device(), (int64_t)v);
		else if (k == "iterations") p.iterations_ = (int)v;
		else if (k == "densify_from_iter") p.densify_from_iter_ = (int)v;
		else if (k == "densify_until_iter") p.densify_until_iter_ = (int)v;
		else if (k == "densification_interval") p.densification_interval_ = (int)v;
		else if (k == "opacity_reset_interval") p.opacity_reset_interval_ = (int)v;
		else if (k == "densify_grad_threshold") p.densify_grad_threshold_ = (float)v;
		else if (k == "percent_dense") p.percent_dense_ = (float)v;
		else if (k == "lambda_dssim") p.lambda_dssim_ = (float)v;
		else TORCH_CHECK(false, "unknown trainer option: ", k);
	}
}
std::vector<int64_t> trainer_densify_and_prune(int64_t h, double max_grad, double min_opacity, double extent,
                                               int64_t max_screen_size, int64_t seed)
{
	auto g = get(h)->gaussians_;
	auto r = g->densifyAndPrune((float)max_grad, (float)min_opacity, (float)extent, (int)max_screen_size,
	                            make_generator(g->xyz_.device(), seed));
	return {r.cloned, r.split, r.pruned, r.points};
}
// GaussianModel::relocateDead / addNew / addPositionNoise with a generator seeded as given; TrainStep::last_mcmc_counts_
torch::Tensor trainer_relocate_dead(int64_t h, double min_opacity, int64_t seed)
{
	auto g = get(h)->gaussians_;
	return g->relocateDead((float)min_opacity, make_generator(g->xyz_.device(), seed));
}
int64_t trainer_add_new(int64_t h, int64_t cap_max, int64_t seed)
{
	auto g = get(h)->gaussians_;
	return g->addNew(cap_max, make_generator(g->xyz_.device(), seed));
}
void trainer_add_position_noise(int64_t h, double noise_scale, int64_t seed)
{
	auto g = get(h)->gaussians_;
	g->addPositionNoise((float)noise_scale, make_generator(g->xyz_.device(), seed));
}
torch::Tensor trainer_last_mcmc_counts(int64_t h)
{
	auto t = get(h);
	return or_empty(t->last_mcmc_counts_, t->gaussians_->xyz_, torch::kInt32);
}
// TrainStep::seedFromDepth (the pixels of the new rows are kept: trainer_last_seed_pixels); GaussianModel::last_seed_counts_ / _pixels_
int64_t trainer_seed_from_depth(int64_t h, torch::Tensor view, torch::Tensor proj, torch::Tensor campos, double fovx, double fovy,
                                int64_t H, int64_t W, torch::Tensor gt_image, torch::Tensor gt_depth, int64_t iteration)
{
	return get(h)->seedFromDepth(make_kf(view, proj, campos, fovx, fovy, H, W), gt_image, gt_depth, (int)iteration, true);
}
// GaussianModel::appendRows: the five row tensors join the model as increasePcd's rows do
void trainer_append_rows(int64_t h, std::vector<torch::Tensor> rows, int64_t iteration)
{
	TORCH_CHECK(rows.size() == 5, "trainer_append_rows: xyz, features, opacity, scaling, rotation");
	get(h)->gaussians_->appendRows({rows[0], rows[1], rows[2], rows[3], rows[4]}, (int)iteration);
}
// a trainer around a model that has no tensors yet (no optimizer either): seedFromDepth makes the first Gaussians
int64_t trainer_create_empty(int64_t sh_degree, torch::Tensor background)
{
	auto model = std::make_shared<GaussianModel>((int)sh_degree);
	model->device_ = background.device();
	return adopt(model, background);
}
std::vector<int64_t> trainer_last_seed_counts(int64_t h) { return get(h)->gaussians_->last_seed_counts_; }
torch::Tensor trainer_last_seed_pixels(int64_t h)
{
	auto g = get(h)->gaussians_;
	return or_empty(g->last_seed_pixels_, g->xyz_, torch::kInt32);
}
torch::Tensor trainer_reorder_along_z_curve(int64_t h) { return get(h)->gaussians_->reorderAlongZCurve(); }
std::vector<int64_t> trainer_last_densify(int64_t h)
{
	auto r = get(h)->last_densify_;
	return {r.cloned, r.split, r.pruned, r.points};
}
void trainer_save_ply(int64_t h, std::string path) { get(h)->gaussians_->savePly(path); }
// GaussianModel::savePly(path, fused = true): the 3-D smoothing filter folded into the stored scales and opacities
void trainer_save_ply_fused(int64_t h, std::string path) { get(h)->gaussians_->savePly(path, true); }
// TrainStep::setFilterCameras with the [K, 20] rows of gsr_filter3d_camera; the model's filter_3D_ ([0] while it is undefined);
// GaussianModel::computeFilter3D; getScalingWithFilter3D / getOpacityWithFilter3D
void trainer_set_filter_cameras(int64_t h, torch::Tensor cameras) { get(h)->setFilterCameras(cameras); }
torch::Tensor trainer_filter_3d(int64_t h)
{
	auto t = get(h);
	return or_empty(t->gaussians_->filter_3D_, t->background_, torch::kFloat32);
}
int64_t trainer_filter3d_renders(int64_t h) { return get(h)->filter3d_renders_; }
torch::Tensor trainer_compute_filter_3d(int64_t h, torch::Tensor cameras, double variance)
{
	auto g = get(h)->gaussians_;
	return g->computeFilter3D(cameras.to(g->xyz_.device(), torch::kFloat32).contiguous(), static_cast<float>(variance));
}
std::vector<torch::Tensor> trainer_filtered_activations(int64_t h)
{
	auto g = get(h)->gaussians_;
	torch::NoGradGuard ng;
	return {g->getScalingWithFilter3D(), g->getOpacityWithFilter3D()};
}
// a fresh trainer from a PLY checkpoint (GaussianModel::loadPly): the tensors land on the device of `bg`
int64_t trainer_create_from_ply(std::string path, int64_t sh_degree, double spatial_lr_scale, torch::Tensor bg)
{
	auto g = std::make_shared<GaussianModel>((int)sh_degree);
	g->device_ = bg.device();
	g->loadPly(path);
	g->spatial_lr_scale_ = (float)spatial_lr_scale;
	g->trainingSetup(GaussianOptimizationParams());
	return adopt(g, bg);
}
void trainer_reset_opacity(int64_t h) { get(h)->gaussians_->resetOpacity(); }
void trainer_apply_scaled_transformation(int64_t h, double s, torch::Tensor T) { get(h)->gaussians_->applyScaledTransformation((float)s, T); }
// -> (flags after the call, number of points moved)
std::tuple<torch::Tensor, int64_t> trainer_scaled_transform_visible(int64_t h, torch::Tensor flags, torch::Tensor diff_pose,
                                                                    torch::Tensor view, torch::Tensor proj, int64_t kf_creation_iter,
                                                                    int64_t stable_num_iter_existence, double scale)
{
	int moved = 0;
	auto f = flags.clone();
	get(h)->gaussians_->scaledTransformVisiblePointsOfKeyframe(f, diff_pose, view, proj, (int)kf_creation_iter, (int)stable_num_iter_existence,
	                                                          moved, (float)scale);
	return {f, (int64_t)moved};
}
void trainer_prune_points(int64_t h, torch::Tensor mask) { get(h)->gaussians_->prunePoints(mask); }
void trainer_one_up_sh_degree(int64_t h) { get(h)->gaussians_->oneUpShDegree(); }
std::vector<torch::Tensor> trainer_moments(int64_t h)   // exp_avg of the five groups, then exp_avg_sq
{
	std::vector<torch::Tensor> out;
	get(h)->gaussians_->syncFeatures();
	for (auto& g : get(h)->gaussians_->groups_) out.push_back(g.exp_avg);
	for (auto& g : get(h)->gaussians_->groups_) out.push_back(g.exp_avg_sq);
	return out;
}

// lazy SH Adam: the step every row of the SH tensor has taken (empty = every row is up to date), WITHOUT bringing them up to date
torch::Tensor trainer_features_row_step(int64_t h)
{
	auto& r = get(h)->gaussians_->features_row_step_;
	return r.defined() ? r.clone() : torch::empty({0}, torch::kInt32);
}

// Adam step counters of the five groups (torch::optim::AdamParamState::step of the reference's six: features_dc and
// features_rest share one counter here, as they always carry a gradient together)
std::vector<int64_t> trainer_steps(int64_t h)
{
	std::vector<int64_t> out;
	for (auto& g : get(h)->gaussians_->groups_) out.push_back(g.step);
	return out;
}
void trainer_set_steps(int64_t h, std::vector<int64_t> steps)
{
	auto& groups = get(h)->gaussians_->groups_;
	TORCH_CHECK(steps.size() == groups.size(), "one step counter per parameter group");
	for (size_t i = 0; i < groups.size(); i++) groups[i].step = (int)steps[i];
}

bool trainer_densify_due(int64_t h) { return get(h)->densifyDue(); }

// view-factored exchange of the data-parallel step (bench.py --gpus N, trainer.ViewFactoredExchange)
void trainer_set_factored_exchange(int64_t h, bool on) { get(h)->factored_exchange_ = on; }
torch::Tensor trainer_sh_grad_view(int64_t h) { return get(h)->sh_grad_view_; }
torch::Tensor trainer_sh_send_buffer(int64_t h) { return get(h)->sh_send_; }
std::vector<double> trainer_exchange_wait_ms(int64_t h) { return get(h)->exchangeWaitMs(); }
void trainer_features_grad_from_views(int64_t h, torch::Tensor campos_views, torch::Tensor views)
{
	get(h)->setFeaturesGradFromViews(campos_views, views);
}
void trainer_features_step_from_views(int64_t h, torch::Tensor campos_views, torch::Tensor views, int64_t row0, bool first_part)
{
	get(h)->stepFeaturesFromViews(campos_views, views, row0, first_part);
}
// GaussianModel::increasePcd (src/gaussian_model.cpp:188-376): the tensor overload, or -- vector_overload -- the std::vector one
void trainer_increase_pcd(int64_t h, torch::Tensor points, torch::Tensor colors, int64_t iteration, bool vector_overload)
{
	auto g = get(h)->gaussians_;
	if (vector_overload) {
		auto p = points.detach().to(torch::kCPU).to(torch::kFloat32).contiguous(), c = colors.detach().to(torch::kCPU).to(torch::kFloat32).contiguous();
		std::vector<float> pv(p.data_ptr<float>(), p.data_ptr<float>() + p.numel()), cv(c.data_ptr<float>(), c.data_ptr<float>() + c.numel());
		g->increasePcd(pv, cv, (int)iteration);
	} else {
		g->increasePcd(points, colors, (int)iteration);
	}
}
torch::Tensor trainer_exist_since_iter(int64_t h) { return get(h)->gaussians_->exist_since_iter_; }
void trainer_set_exist_since_iter(int64_t h, torch::Tensor v)
{
	auto g = get(h)->gaussians_;
	g->exist_since_iter_ = v.to(g->xyz_.device()).to(torch::kInt32).contiguous().clone();
}
void trainer_release_arena(int64_t h) { get(h)->gaussians_->releaseArena(); }
// Data-parallel keyframe batches driven from C++: the process group Python created (torch.distributed's default group, or any
// other) is resolved by its registered name; from then on trainer_train_one_iteration() issues every collective itself.
// the host-side group (gloo) over which the packed exchange agrees on its message capacity; empty name = none
void trainer_set_count_group(int64_t h, std::string group_name)
{
	if (group_name.empty()) get(h)->setCountGroup(nullptr);
	else get(h)->setCountGroup(c10d::resolve_process_group(group_name));
}
void trainer_set_process_group(int64_t h, std::string group_name, bool factored)
{
	if (group_name.empty()) get(h)->setProcessGroup(nullptr, factored);
	else get(h)->setProcessGroup(c10d::resolve_process_group(group_name), factored);
}
torch::Tensor trainer_train_one_iteration(int64_t h, torch::Tensor view, torch::Tensor proj, torch::Tensor campos, double fovx, double fovy,
                                          int64_t height, int64_t width, torch::Tensor gt, torch::Tensor mask)
{
	return get(h)->trainForOneIteration(make_kf(view, proj, campos, fovx, fovy, height, width), gt, mask).detach();
}
void trainer_features_finish_from_views(int64_t h) { get(h)->finishFeaturesFromViews(); }
void trainer_geom_adam(int64_t h, double grad_scale) { get(h)->finishGeomAdam((float)grad_scale); }
torch::Tensor sh_grad_from_views(torch::Tensor means3D, torch::Tensor campos_views, torch::Tensor views, int64_t degree,
                                 int64_t M, double scale)
{
	return shGradFromViews(means3D, campos_views, views, (int)degree, (int)M, (float)scale);
}
std::vector<torch::Tensor> trainer_stats(int64_t h)
{
	auto g = get(h)->gaussians_;
	return {g->xyz_gradient_accum_, g->denom_, g->max_radii2D_};
}
// KeyframeScheduler (host/include/keyframe_scheduler.h) behind handles, for the tests and for a Python driver of a keyframe batch
std::map<int64_t, std::shared_ptr<KeyframeScheduler>> g_schedulers;
int64_t g_next_scheduler = 1;
std::shared_ptr<KeyframeScheduler> scheduler(int64_t h)
{
	std::lock_guard<std::mutex> lk(g_mu);
	auto it = g_schedulers.find(h);
	TORCH_CHECK(it != g_schedulers.end(), "unknown keyframe scheduler handle ", h);
	return it->second;
}
int64_t keyframe_scheduler_create(int64_t seed)
{
	std::lock_guard<std::mutex> lk(g_mu);
	g_schedulers[g_next_scheduler] = std::make_shared<KeyframeScheduler>((uint64_t)seed);
	return g_next_scheduler++;
}
void keyframe_scheduler_destroy(int64_t h)
{
	std::lock_guard<std::mutex> lk(g_mu);
	g_schedulers.erase(h);
}
int64_t keyframe_scheduler_add(int64_t h, int64_t times_of_use) { return scheduler(h)->addKeyframe((int)times_of_use); }
void keyframe_scheduler_increase(int64_t h, int64_t keyframe, int64_t times) { scheduler(h)->increaseTimesOfUse((int)keyframe, (int)times); }
int64_t keyframe_scheduler_use_one(int64_t h) { return scheduler(h)->useOne(); }
std::vector<int64_t> keyframe_scheduler_use_batch(int64_t h, int64_t B)
{
	const auto b = scheduler(h)->useBatch((int)B);
	return std::vector<int64_t>(b.begin(), b.end());
}
std::vector<int64_t> keyframe_scheduler_use_batch_on_ranks(int64_t h, std::string group_name)
{
	const auto b = scheduler(h)->useBatchOnRanks(c10d::resolve_process_group(group_name));
	return std::vector<int64_t>(b.begin(), b.end());
}
// [used times, remaining times of use] of every keyframe
std::vector<int64_t> keyframe_scheduler_state(int64_t h)
{
	auto s = scheduler(h);
	std::vector<int64_t> out;
	for (int k = 0; k < s->size(); k++) out.push_back(s->usedTimes(k));
	for (int k = 0; k < s->size(); k++) out.push_back(s->remainingTimesOfUse(k));
	return out;
}
void trainer_destroy(int64_t h)
{
	std::lock_guard<std::mutex> lk(g_mu);
	g_trainers.erase(h);
}

}  // namespace

TORCH_LIBRARY(photoslam_amd, m)
{
	m.def("rasterize_gaussians", &rasterize_gaussians);
	m.def("rasterize_gaussians_modes", &rasterize_gaussians_modes);
	m.def("rasterize_gaussians_contribution", &rasterize_gaussians_contribution);
	m.def("rasterize_gaussians_absgrad", &rasterize_gaussians_absgrad);
	m.def("trainer_last_absgrad", &trainer_last_absgrad);
	m.def("covisibility", &covisibility_op);
	m.def("trainer_score_contribution", &trainer_score_contribution);
	m.def("trainer_prune_uncontributing", &trainer_prune_uncontributing);
	m.def("mark_visible", &mark_visible);
	m.def("dist_cuda2", &dist_cuda2);
	m.def("l1_ssim_loss", &l1_ssim_loss);
	m.def("l1_ssim_loss_exposure", &l1_ssim_loss_exposure);
	m.def("apply_exposure", &apply_exposure);
	m.def("depth_prior_loss", &depth_prior_loss);
	m.def("depth_prior_fit", &depth_prior_fit);
	m.def("depth_prior_apply", &depth_prior_apply);
	m.def("trainer_train_depth_prior", &trainer_train_depth_prior);
	m.def("trainer_last_depth_prior_fit", &trainer_last_depth_prior_fit);
	m.def("trainer_align_depth_prior", &trainer_align_depth_prior);
	m.def("trainer_train_exposure", &trainer_train_exposure);
	m.def("trainer_render_view_exposure", &trainer_render_view_exposure);
	m.def("trainer_refine_pose_exposure", &trainer_refine_pose_exposure);
	m.def("trainer_exposure_lr", &trainer_exposure_lr);
	// host/include/loss_utils.h, the functions behind the reference's names (tests pin them to the reference's header compiled)
	m.def("loss_ssim", +[](torch::Tensor a, torch::Tensor b, int64_t window_size, bool size_average) {
		return loss_utils::ssim(a, b, a.device().type(), (int)window_size, size_average);
	});
	m.def("loss_ssim_with_window", +[](torch::Tensor a, torch::Tensor b, torch::Tensor window, int64_t window_size, bool size_average) {
		torch::autograd::Variable w = window;
		return loss_utils::_ssim(a, b, w, (int)window_size, a.size(-3), size_average);
	});
	m.def("loss_psnr", +[](torch::Tensor a, torch::Tensor b) { return loss_utils::psnr(a, b); });
	m.def("loss_psnr_gaussian_splatting", +[](torch::Tensor a, torch::Tensor b) { return loss_utils::psnr_gaussian_splatting(a, b); });
	m.def("loss_create_window", +[](int64_t window_size, int64_t channel, torch::Tensor like) {
		return loss_utils::create_window((int)window_size, channel, like.device().type());
	});
	m.def("loss_l1", +[](torch::Tensor a, torch::Tensor b) { return loss_utils::l1_loss(a, b); });
	m.def("transform_points", &transform_points);
	m.def("scale_transform_mark_visible", &scale_transform_mark_visible);
	m.def("reproject_depth_pinhole", &reproject_depth_pinhole);
	m.def("neighborhood_keypoints", &neighborhood_keypoints);
	m.def("trainer_create", &trainer_create);
	m.def("trainer_render_and_backward", &trainer_render_and_backward);
	m.def("trainer_render", &trainer_render);
	m.def("trainer_render_view", &trainer_render_view);
	m.def("trainer_render_and_backward_depth", &trainer_render_and_backward_depth);
	m.def("trainer_render_view_depth", &trainer_render_view_depth);
	m.def("trainer_finish", &trainer_finish);
	m.def("trainer_finish_begin", &trainer_finish_begin);
	m.def("trainer_adam_group", &trainer_adam_group);
	m.def("trainer_finish_end", &trainer_finish_end);
	m.def("trainer_params", &trainer_params);
	m.def("trainer_refine_pose", &trainer_refine_pose);
	m.def("trainer_state", &trainer_state);
	m.def("trainer_pose_gradient", &trainer_pose_gradient);
	m.def("trainer_last_reg_losses", &trainer_last_reg_losses);
	m.def("trainer_grads", &trainer_grads);
	m.def("trainer_stats", &trainer_stats);
	m.def("trainer_create_from_pcd", &trainer_create_from_pcd);
	m.def("trainer_set_options", &trainer_set_options);
	m.def("trainer_densify_and_prune", &trainer_densify_and_prune);
	m.def("trainer_reorder_along_z_curve", &trainer_reorder_along_z_curve);
	m.def("trainer_relocate_dead", &trainer_relocate_dead);
	m.def("trainer_add_new", &trainer_add_new);
	m.def("trainer_add_position_noise", &trainer_add_position_noise);
	m.def("trainer_last_mcmc_counts", &trainer_last_mcmc_counts);
	m.def("trainer_seed_from_depth", &trainer_seed_from_depth);
	m.def("trainer_last_seed_counts", &trainer_last_seed_counts);
	m.def("trainer_append_rows", &trainer_append_rows);
	m.def("trainer_create_empty", &trainer_create_empty);
	m.def("trainer_last_seed_pixels", &trainer_last_seed_pixels);
	m.def("trainer_last_densify", &trainer_last_densify);
	m.def("trainer_save_ply", &trainer_save_ply);
	m.def("trainer_save_ply_fused", &trainer_save_ply_fused);
	m.def("trainer_set_filter_cameras", &trainer_set_filter_cameras);
	m.def("trainer_filter_3d", &trainer_filter_3d);
	m.def("trainer_filter3d_renders", &trainer_filter3d_renders);
	m.def("trainer_compute_filter_3d", &trainer_compute_filter_3d);
	m.def("trainer_filtered_activations", &trainer_filtered_activations);
	m.def("trainer_create_from_ply", &trainer_create_from_ply);
	m.def("trainer_reset_opacity", &trainer_reset_opacity);
	m.def("trainer_apply_scaled_transformation", &trainer_apply_scaled_transformation);
	m.def("trainer_scaled_transform_visible", &trainer_scaled_transform_visible);
	m.def("trainer_prune_points", &trainer_prune_points);
	m.def("trainer_one_up_sh_degree", &trainer_one_up_sh_degree);
	m.def("trainer_moments", &trainer_moments);
	m.def("trainer_steps", &trainer_steps);
	m.def("trainer_features_row_step", &trainer_features_row_step);
	m.def("trainer_set_steps", &trainer_set_steps);
	m.def("trainer_densify_due", &trainer_densify_due);
	m.def("trainer_set_factored_exchange", &trainer_set_factored_exchange);
	m.def("trainer_sh_grad_view", &trainer_sh_grad_view);
	m.def("trainer_sh_send_buffer", &trainer_sh_send_buffer);
	m.def("trainer_exchange_wait_ms", &trainer_exchange_wait_ms);
	m.def("trainer_features_grad_from_views", &trainer_features_grad_from_views);
	m.def("trainer_features_step_from_views", &trainer_features_step_from_views);
	m.def("trainer_increase_pcd", &trainer_increase_pcd);
	m.def("trainer_exist_since_iter", &trainer_exist_since_iter);
	m.def("trainer_set_exist_since_iter", &trainer_set_exist_since_iter);
	m.def("trainer_release_arena", &trainer_release_arena);
	m.def("trainer_set_process_group", &trainer_set_process_group);
	m.def("trainer_set_count_group", &trainer_set_count_group);
	m.def("trainer_train_one_iteration", &trainer_train_one_iteration);
	m.def("trainer_features_finish_from_views", &trainer_features_finish_from_views);
	m.def("trainer_geom_adam", &trainer_geom_adam);
	m.def("sh_grad_from_views", &sh_grad_from_views);
	m.def("trainer_destroy", &trainer_destroy);
	m.def("keyframe_scheduler_create", &keyframe_scheduler_create);
	m.def("keyframe_scheduler_destroy", &keyframe_scheduler_destroy);
	m.def("keyframe_scheduler_add", &keyframe_scheduler_add);
	m.def("keyframe_scheduler_increase", &keyframe_scheduler_increase);
	m.def("keyframe_scheduler_use_one", &keyframe_scheduler_use_one);
	m.def("keyframe_scheduler_use_batch", &keyframe_scheduler_use_batch);
	m.def("keyframe_scheduler_use_batch_on_ranks", &keyframe_scheduler_use_batch_on_ranks);
	m.def("keyframe_scheduler_state", &keyframe_scheduler_state);
}
