// train_step.cpp -- LibTorch host code of the measured train step (see gaussian_model_lite.h).
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "../../../include/gsr.h"
#include "gaussian_model_lite.h"
#include "gaussian_renderer.h"
#include "loss_utils.h"

#ifndef GSR_HOST_NO_HIP
#include <c10/hip/HIPStream.h>
#endif

namespace {
void* stream_of(const torch::Tensor& t)
{
#ifndef GSR_HOST_NO_HIP
	if (t.is_cuda()) return c10::hip::getCurrentHIPStream(t.device().index()).stream();
#endif
	return nullptr;
}
void check(int status, const char* where)
{
	if (status != GSR_OK) throw std::runtime_error(std::string(where) + ": " + gsr_strerror(status));
}

// (render, viewspace_points, visibility_filter, radii, depth, alpha) of GaussianRenderer::renderWithDepth
using RenderPackage = std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>;

// THE render call of a TrainStep: the keyframe at its own size, the step's pipeline flags and background, no override colours;
// with_depth appends the depth and alpha maps (undefined tensors otherwise).  Model: GaussianModel, or refinePose's frozen copy
template <class Model>
RenderPackage renderModel(TrainStep& t, const std::shared_ptr<GaussianKeyframe>& kf, const std::shared_ptr<Model>& model,
                          const GaussianRasterizationExtensions& ext, bool with_depth)
{
	torch::Tensor none;
	const int H = kf->image_height_, W = kf->image_width_;
	if (with_depth) return GaussianRenderer::renderWithDepth(kf, H, W, model, t.pipe_, t.background_, none, 1.0f, false, ext);
	auto p = GaussianRenderer::render(kf, H, W, model, t.pipe_, t.background_, none, 1.0f, false, ext);
	return RenderPackage(std::get<0>(p), std::get<1>(p), std::get<2>(p), std::get<3>(p), none, none);
}
}  // namespace

torch::Tensor fusedL1SSIMLoss(torch::Tensor rendered, torch::Tensor gt, torch::Tensor mask, float lambda_dssim, bool is_root)
{
	return loss_utils::fused_l1_ssim(rendered, gt, mask, lambda_dssim, is_root);   // (lib cuda_rasterizer: host/src/loss_utils.cpp)
}

GaussianModel::GaussianModel(int sh_degree, torch::Tensor xyz, torch::Tensor features, torch::Tensor opacity,
                             torch::Tensor scaling, torch::Tensor rotation, float spatial_lr_scale)
    : max_sh_degree_(sh_degree), active_sh_degree_(sh_degree), spatial_lr_scale_(spatial_lr_scale)
{
	auto leaf = [](torch::Tensor t) { return t.detach().clone().contiguous().set_requires_grad(true); };
	xyz_ = leaf(xyz);
	features_ = leaf(features);
	opacity_ = leaf(opacity);
	scaling_ = leaf(scaling);
	rotation_ = leaf(rotation);
	const auto P = xyz_.size(0);
	max_radii2D_ = torch::zeros({P}, xyz_.options());
	xyz_gradient_accum_ = torch::zeros({P, 1}, xyz_.options());
	denom_ = torch::zeros({P, 1}, xyz_.options());
	exist_since_iter_ = torch::zeros({P}, xyz_.options().dtype(torch::kInt32).requires_grad(false));
}

// src/gaussian_model.cpp:73-96: Sigma = (R S)(R S)^T with R = build_rotation(rotation_) (include/general_utils.h:33-57: the
// quaternion is normalised there), S = diag(scaling_modifier * exp(scaling_)); the six entries xx xy xz yy yz zz
torch::Tensor GaussianModel::getCovarianceActivation(int scaling_modifier)
{
	auto q = rotation_ / torch::sqrt((rotation_ * rotation_).sum(1, /*keepdim=*/true));
	auto r = q.select(1, 0), x = q.select(1, 1), y = q.select(1, 2), z = q.select(1, 3);
	auto R = torch::stack({1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
	                       2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
	                       2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)}, 1).reshape({-1, 3, 3});
	auto L = R * (scaling_modifier * getScalingActivation()).unsqueeze(1);   // R diag(s): column j scaled by s_j
	auto cov = torch::bmm(L, L.transpose(1, 2));
	return torch::stack({cov.select(1, 0).select(1, 0), cov.select(1, 0).select(1, 1), cov.select(1, 0).select(1, 2),
	                     cov.select(1, 1).select(1, 1), cov.select(1, 1).select(1, 2), cov.select(1, 2).select(1, 2)}, 1);
}

// Mip-Splatting's 3-D smoothing filter (include/gsr.h: GSR_FILTER_3D, gsr_filter3d_compute)
torch::Tensor GaussianModel::computeFilter3D(const torch::Tensor& cameras, float variance)
{
	filter_3D_ = filter3D(xyz_.detach(), cameras, variance);
	return filter_3D_;
}

torch::Tensor GaussianModel::getScalingWithFilter3D()
{
	if (!filter_3D_.defined() || filter_3D_.size(0) != xyz_.size(0))
		throw std::runtime_error("filter_3D_ is not defined for this model (computeFilter3D)");
	auto s = getScalingActivation();
	return torch::sqrt(s * s + (filter_3D_ * filter_3D_).unsqueeze(1));
}

torch::Tensor GaussianModel::getOpacityWithFilter3D()
{
	auto sp = getScalingWithFilter3D();
	auto r = getScalingActivation() / sp;
	return getOpacityActivation() * ((r.select(1, 0) * r.select(1, 1)) * r.select(1, 2)).unsqueeze(1);
}

void GaussianModel::trainingSetup(const GaussianOptimizationParams& opt)
{
	opt_ = opt;
	groups_.clear();
	auto add = [&](torch::Tensor& p, double lr, int period = 0, int split = 0, double lr_tail = 0.0) {
		AdamGroup g;
		g.param = p;
		g.exp_avg = torch::zeros_like(p);
		g.exp_avg_sq = torch::zeros_like(p);
		g.lr = lr;
		g.lr_tail = lr_tail;
		g.period = period;
		g.split = split;
		groups_.push_back(g);
	};
	add(xyz_, opt.position_lr_init_ * spatial_lr_scale_);
	// features_dc (lr) | features_rest (lr / 20) share the [P,16,3] buffer
	add(features_, opt.feature_lr_, 3 * (max_sh_degree_ + 1) * (max_sh_degree_ + 1), 3, opt.feature_lr_ / 20.0);   // double division, :495
	add(opacity_, opt.opacity_lr_);
	add(scaling_, opt.scaling_lr_);
	add(rotation_, opt.rotation_lr_);
	preloadMaintenanceKernels();
}

// The HIP runtime loads a code object of LibTorch the first time one of its kernels is launched.  The train step itself uses
// none of ATen's elementwise kernels, so the first resetOpacity (sigmoid, minimum) or loop-closure call (integer abs / compare)
// in the middle of a mapping session would pay for that: 25 ms on a warm box, 110 ms on a cold one, measured as ONE iteration of
// bench.py --mapper-loop (the second reset of the same run costs nothing measurable).  They are touched here, on four elements,
// when the optimizer is set up -- a session pays at its start, not at iteration opacity_reset_interval.
void GaussianModel::preloadMaintenanceKernels()
{
	if (!xyz_.defined() || !xyz_.is_cuda()) return;
	torch::NoGradGuard ng;
	const auto o = xyz_.options().requires_grad(false);
	auto x = torch::full({4, 1}, 0.25f, o);
	auto act = torch::sigmoid(x);
	auto bound = torch::ones_like(act * 0.01);
	auto y = torch::log(torch::min(act, bound) / (1 - torch::min(act, torch::ones_like(act) * 0.01)));   // resetOpacity, both forms
	auto age = torch::zeros({4}, o.dtype(torch::kInt32));
	auto young = torch::abs(age - 3) < 2;                                                               // scaledTransformVisiblePointsOfKeyframe
	auto z = (x * 1.5f).contiguous().clone().zero_();
	(void)y; (void)young; (void)z;
}

float GaussianModel::updateLearningRate(int step)
{
	const float lr_init = opt_.position_lr_init_ * spatial_lr_scale_, lr_final = opt_.position_lr_final_ * spatial_lr_scale_;
	float lr = 0.f;
	if (!(step < 0 || (lr_init == 0.0f && lr_final == 0.0f))) {
		float t = static_cast<float>(step) / static_cast<float>(opt_.position_lr_max_steps_);
		t = std::min(std::max(t, 0.0f), 1.0f);
		lr = std::exp(std::log(lr_init) * (1 - t) + std::log(lr_final) * t);
	}
	groups_[0].lr = lr;
	return lr;
}

ShAdamStep GaussianModel::featuresAdamStep(ShStep which) const
{
	const AdamGroup& grp = groups_.at(1);
	const bool taken = which == ShStep::LazyTaken;
	ShAdamStep s;
	s.exp_avg = grp.exp_avg;
	s.exp_avg_sq = grp.exp_avg_sq;
	s.step = grp.step;
	s.lr = taken ? features_lr_hist_.at(0).first : grp.lr * lr_scale_;
	s.lr_tail = taken ? features_lr_hist_.at(0).second : grp.lr_tail * lr_scale_;
	if (which == ShStep::Eager) return s;
	s.row_step = features_row_step_;
	s.window = features_lazy_window_;
	for (size_t k = taken ? 1 : 0; k < features_lr_hist_.size(); k++) {
		s.lr_past.push_back(features_lr_hist_[k].first);
		s.lr_tail_past.push_back(features_lr_hist_[k].second);
	}
	return s;
}

ShAdamStep GaussianModel::beginFeaturesStep(bool lazy, int window)
{
	AdamGroup& grp = groups_.at(1);
	if (lazy && features_row_step_.defined() && features_lazy_window_ != window) syncFeatures();
	if (lazy && !features_row_step_.defined()) {   // every row has taken the grp.step steps so far
		features_row_step_ = torch::full({features_.size(0)}, grp.step, features_.options().dtype(torch::kInt32).requires_grad(false));
		features_lazy_window_ = window;
		features_lr_hist_.clear();
	}
	grp.step++;   // the caller takes the step; optimizerStepGroup(1) then finds no gradient
	return featuresAdamStep(lazy ? ShStep::Lazy : ShStep::Eager);
}

void GaussianModel::endFeaturesStep(const ShAdamStep& taken)
{
	features_lr_hist_.insert(features_lr_hist_.begin(), {taken.lr, taken.lr_tail});
	if (static_cast<int>(features_lr_hist_.size()) > features_lazy_window_) features_lr_hist_.pop_back();
}

void GaussianModel::syncFeatures()
{
	if (!features_row_step_.defined()) return;
	torch::NoGradGuard ng;
	const bool behind = !features_lr_hist_.empty() && groups_.size() > 1;
	const ShAdamStep s = behind ? featuresAdamStep(ShStep::LazyTaken) : ShAdamStep();
	features_row_step_ = torch::Tensor();   // (before the flush: the calls below may come back here)
	if (behind) {
		auto sh = features_.detach();
		shAdamFlush(sh, s);
	}
	features_lr_hist_.clear();
}

void GaussianModel::optimizerStepGroup(int group)
{
	torch::NoGradGuard ng;
	auto& g = groups_.at(static_cast<size_t>(group));
	auto grad = g.param.grad();
	if (!grad.defined()) return;
	if (group == 1) syncFeatures();   // a dense step of the SH tensor: every row must be up to date first
	grad = grad.contiguous();
	g.step++;
	check(gsr_adam_step(g.param.data_ptr<float>(), grad.data_ptr<float>(), g.exp_avg.data_ptr<float>(),
	                    g.exp_avg_sq.data_ptr<float>(), g.param.numel(), g.lr * lr_scale_, 0.9, 0.999, 1e-15, g.step, g.period,
	                    g.split, (g.period ? g.lr_tail : g.lr) * lr_scale_, stream_of(g.param)),
	      "gsr_adam_step");
}

void GaussianModel::optimizerStep()
{
	beginOptimizerStep();
	for (int i = 0; i < static_cast<int>(groups_.size()); i++) optimizerStepGroup(i);
}

void GaussianModel::zeroGrad()
{
	for (auto& g : groups_) g.param.mutable_grad() = torch::Tensor();
}

void GaussianModel::addDensificationStats(torch::Tensor& viewspace_point_tensor, torch::Tensor& update_filter)
{
	addDensificationStats(viewspace_point_tensor, update_filter, viewspace_point_tensor.grad());
}

void GaussianModel::addDensificationStats(torch::Tensor& viewspace_point_tensor, torch::Tensor& update_filter, const torch::Tensor& absgrad)
{
	const torch::Tensor g = absgrad.defined() ? absgrad : viewspace_point_tensor.grad();
	auto n = torch::norm(g.index({update_filter}).slice(1, 0, 2), 2, {-1}, true);
	xyz_gradient_accum_.index_put_({update_filter}, xyz_gradient_accum_.index({update_filter}) + n);
	denom_.index_put_({update_filter}, denom_.index({update_filter}) + 1);
}

void TrainStep::requireSingleProcess(const char* what, bool factored_counts, const char* suffix) const
{
	if (process_group_ || (factored_counts && factored_exchange_))
		throw std::runtime_error(std::string("TrainStep: ") + what + " not supported with a process group" + suffix);
}

GaussianRasterizationExtensions TrainStep::baseExtensions(RasterWorkspace* workspace) const
{
	GaussianRasterizationExtensions ext;
	ext.raw_params_ = 7;
	ext.cull_empty_tiles_ = cull_empty_tiles_;
	ext.antialiasing_ = antialiasing_;
	ext.workspace_ = persistent_workspace_ ? workspace : nullptr;
	return ext;
}

// a viewer's render: forward-only, into the second workspace
GaussianRasterizationExtensions TrainStep::viewExtensions()
{
	GaussianRasterizationExtensions ext = baseExtensions(&view_workspace_);
	ext.filter_3D_ = viewFilter3D();
	ext.forward_only_ = true;
	return ext;
}

torch::Tensor TrainStep::trainForOneIteration(std::shared_ptr<GaussianKeyframe> kf, torch::Tensor gt_image, torch::Tensor mask,
                                              torch::Tensor gt_depth, torch::Tensor prior_depth)
{
	if (process_group_) {
		if (usesDepthLoss(gt_depth)) requireSingleProcess("the depth loss is", false, " (depth_loss_weight_ must be 0)");
		if (usesDepthPrior(prior_depth)) requireSingleProcess("the depth prior is", false, " (depth_prior_weight_ must be 0)");
		if (kf->exposure_.defined() || optimize_exposure_) requireSingleProcess("exposure compensation is", false);
		return trainForOneIterationDataParallel(kf, gt_image, mask);
	}
	auto loss = renderAndBackward(kf, gt_image, mask, gt_depth, prior_depth);
	finishOneIteration();
	return loss;
}

void TrainStep::setFilterCameras(const std::vector<std::shared_ptr<GaussianKeyframe>>& keyframes)
{
	std::vector<torch::Tensor> rows;
	for (const auto& kf : keyframes) {
		// the rasterizer's own tan(FoV / 2) (GaussianRenderer::render): focal = size / (2 tan)
		const double tanfovx = std::tan(kf->FoVx_ * 0.5f), tanfovy = std::tan(kf->FoVy_ * 0.5f);
		const int W = kf->image_width_, H = kf->image_height_;
		rows.push_back(filter3DCameraRow(kf->world_view_transform_, static_cast<float>(W / (2.0 * tanfovx)), static_cast<float>(H / (2.0 * tanfovy)),
		                                 static_cast<float>(W), static_cast<float>(H)));
	}
	setFilterCameras(rows.empty() ? torch::zeros({0, 20}, torch::kFloat32) : torch::stack(rows));
}

void TrainStep::setFilterCameras(const torch::Tensor& cameras)
{
	if (cameras.dim() != 2 || cameras.size(1) != 20) throw std::runtime_error("setFilterCameras: a [K, 20] tensor of gsr_filter3d_camera rows");
	// (a model without tensors yet -- seedFromDepth makes the first ones -- names its device itself)
	const torch::Device dev = gaussians_->xyz_.defined() ? gaussians_->xyz_.device() : gaussians_->device_;
	filter_cameras_ = cameras.detach().to(dev, torch::kFloat32).contiguous();
	gaussians_->filter_3D_ = torch::Tensor();
}

void TrainStep::checkFilter3D() const
{
	if (!filter3d_) return;
	requireSingleProcess("filter3d_ is", true);
	if (!filter_cameras_.defined() || filter_cameras_.size(0) == 0)
		throw std::runtime_error("TrainStep: filter3d_ is on and no cameras are registered (setFilterCameras)");
}

torch::Tensor TrainStep::viewFilter3D(bool recompute)
{
	if (!filter3d_) return torch::Tensor();
	checkFilter3D();
	auto& g = gaussians_;
	if (!g->xyz_.defined()) return torch::Tensor();   // (no Gaussian yet: nothing is rendered)
	if (filter_cameras_.device() != g->xyz_.device()) filter_cameras_ = filter_cameras_.to(g->xyz_.device());
	if (recompute || !g->filter_3D_.defined() || g->filter_3D_.size(0) != g->xyz_.size(0)) g->computeFilter3D(filter_cameras_, filter3d_variance_);
	filter3d_renders_++;
	return g->filter_3D_;
}

torch::Tensor TrainStep::renderView(std::shared_ptr<GaussianKeyframe> kf, bool apply_exposure)
{
	torch::NoGradGuard no_grad;
	auto pkg = renderModel(*this, kf, gaussians_, viewExtensions(), false);
	if (apply_exposure && kf->exposure_.defined()) return loss_utils::apply_exposure(std::get<0>(pkg), kf->exposure_);
	return std::get<0>(pkg);
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor> TrainStep::scoreContribution(
    const std::vector<std::shared_ptr<GaussianKeyframe>>& keyframes, const std::vector<torch::Tensor>& pixel_weights)
{
	torch::NoGradGuard no_grad;
	if (!pixel_weights.empty() && pixel_weights.size() != keyframes.size())
		throw std::runtime_error("scoreContribution: one pixel weight map (or an undefined tensor) per keyframe");
	const auto& xyz = gaussians_->xyz_;
	const int64_t P = xyz.size(0);
	const auto f32 = xyz.options().dtype(torch::kFloat32).requires_grad(false), i32 = xyz.options().dtype(torch::kInt32).requires_grad(false);
	auto wsum = torch::zeros({P}, f32), wmax = torch::zeros({P}, f32);
	auto touched = torch::zeros({P}, i32), seen = torch::zeros({P}, i32);
	for (size_t i = 0; i < keyframes.size(); i++) {
		const auto& kf = keyframes[i];
		GaussianRasterizationExtensions ext = viewExtensions();
		ext.out_weight_sum_ = wsum;
		ext.out_weight_max_ = wmax;
		ext.out_n_touched_ = touched;
		ext.contribution_accumulate_ = true;
		if (!pixel_weights.empty() && pixel_weights[i].defined() && pixel_weights[i].numel()) ext.pixel_weight_ = pixel_weights[i];
		auto pkg = renderModel(*this, kf, gaussians_, ext, false);
		seen += (std::get<3>(pkg) > 0).to(torch::kInt32);
	}
	return std::make_tuple(wsum, wmax, touched, seen);
}

int64_t TrainStep::pruneUncontributing(const std::vector<std::shared_ptr<GaussianKeyframe>>& keyframes, float min_weight_max, int min_views)
{
	requireSingleProcess("pruneUncontributing is", false);
	torch::NoGradGuard no_grad;
	auto score = scoreContribution(keyframes);
	torch::Tensor mask = (std::get<3>(score) >= min_views) & (std::get<1>(score) < min_weight_max);
	const int64_t n = mask.sum().item<int64_t>();
	if (n) gaussians_->prunePoints(mask);
	return n;
}

double TrainStep::exposureLearningRate(int step) const
{
	const float lr_init = exposure_lr_init_, lr_final = exposure_lr_final_;
	if (step < 0 || lr_init <= 0.0f || lr_final <= 0.0f) return 0.0;
	const int max_steps = exposure_lr_max_steps_ >= 0 ? exposure_lr_max_steps_ : gaussians_->opt_.iterations_;
	float t = static_cast<float>(step) / static_cast<float>(std::max(max_steps, 1));
	t = std::min(std::max(t, 0.0f), 1.0f);
	return std::exp(std::log(lr_init) * (1 - t) + std::log(lr_final) * t);   // float arithmetic, as updateLearningRate
}

// one Adam step of the last backward pass's keyframe exposure, on the keyframe's own moments and step count
void TrainStep::finishExposure()
{
	auto kf = std::move(exposure_kf_);
	auto grad = std::move(exposure_grad_);
	exposure_kf_.reset();
	exposure_grad_ = torch::Tensor();
	if (!kf || !grad.defined() || iteration_ >= gaussians_->opt_.iterations_) return;
	torch::NoGradGuard ng;
	auto& e = kf->exposure_;
	if (!kf->exposure_exp_avg_.defined()) {
		kf->exposure_exp_avg_ = torch::zeros_like(e);
		kf->exposure_exp_avg_sq_ = torch::zeros_like(e);
	}
	kf->exposure_step_++;
	const double lr = exposureLearningRate(kf->exposure_step_);
	grad = grad.contiguous();
	check(gsr_adam_step(e.data_ptr<float>(), grad.data_ptr<float>(), kf->exposure_exp_avg_.data_ptr<float>(),
	                    kf->exposure_exp_avg_sq_.data_ptr<float>(), 12, lr, 0.9, 0.999, 1e-15, kf->exposure_step_, 0, 0, lr, stream_of(e)),
	      "gsr_adam_step");
}

std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> TrainStep::renderViewWithDepth(std::shared_ptr<GaussianKeyframe> kf)
{
	torch::NoGradGuard no_grad;
	auto pkg = renderModel(*this, kf, gaussians_, viewExtensions(), true);
	return std::make_tuple(std::get<0>(pkg), std::get<4>(pkg), std::get<5>(pkg));
}

std::tuple<torch::Tensor, torch::Tensor> TrainStep::alignDepthPrior(std::shared_ptr<GaussianKeyframe> viewpoint_cam, torch::Tensor prior,
                                                                    torch::Tensor valid)
{
	if (!gaussians_->xyz_.defined() || gaussians_->xyz_.size(0) == 0)
		throw std::runtime_error("TrainStep: alignDepthPrior needs a render to align to, and the model is empty "
		                         "(seed the first frame from a metric depth map)");
	torch::NoGradGuard no_grad;
	auto maps = renderViewWithDepth(viewpoint_cam);
	auto fit = loss_utils::depth_prior_fit(std::get<1>(maps), std::get<2>(maps), prior, depth_prior_inverse_, depth_prior_alpha_min_, valid);
	return std::make_tuple(loss_utils::depth_prior_apply(prior, fit, depth_prior_inverse_), fit);
}

int64_t TrainStep::seedFromDepth(std::shared_ptr<GaussianKeyframe> viewpoint_cam, torch::Tensor gt_image, torch::Tensor gt_depth,
                                 int iteration, bool want_pixels)
{
	requireSingleProcess("seedFromDepth is", true);
	auto& g = gaussians_;
	const int64_t P = g->xyz_.defined() ? g->xyz_.size(0) : 0;
	torch::Tensor alpha, depth;
	if (P > 0) {
		auto maps = renderViewWithDepth(viewpoint_cam);
		depth = std::get<1>(maps);
		alpha = std::get<2>(maps);
	}
	const int H = viewpoint_cam->image_height_, W = viewpoint_cam->image_width_;
	// the rasterizer's own tan(FoV / 2) (GaussianRenderer::render) and its pixel-centre convention
	const float tanfovx = std::tan(viewpoint_cam->FoVx_ * 0.5f), tanfovy = std::tan(viewpoint_cam->FoVy_ * 0.5f);
	GaussianModel::SeedOptions o;
	o.min_depth_ = depth_min_;
	o.max_depth_ = depth_max_;
	o.alpha_threshold_ = seed_alpha_threshold_;
	o.depth_error_abs_ = seed_depth_error_abs_;
	o.depth_median_factor_ = seed_depth_median_factor_;
	o.stride_ = seed_stride_;
	o.scale_factor_ = seed_scale_factor_;
	o.init_opacity_ = seed_init_opacity_;
	o.want_pixels_ = want_pixels;
	const int64_t max_new = mcmc_ ? mcmc_cap_max_ - P : seed_max_new_;
	return g->seedFromDepth(gt_depth, gt_image, alpha, depth, viewpoint_cam->world_view_transform_,
	                        static_cast<float>(W / (2.0 * static_cast<double>(tanfovx))), static_cast<float>(H / (2.0 * static_cast<double>(tanfovy))),
	                        static_cast<float>((W - 1) / 2.0), static_cast<float>((H - 1) / 2.0), iteration, max_new, o);
}

namespace {
// the frozen map of refinePose: exactly the members GaussianRenderer::render touches, detached tensors
struct FrozenModel {
	torch::Tensor xyz_, features_, opacity_, scaling_, rotation_;
	int active_sh_degree_ = 0, max_sh_degree_ = 0;
	torch::Tensor getXYZ() { return xyz_; }
	torch::Tensor getFeatures() { return features_; }
	torch::Tensor getOpacityActivation() { return torch::sigmoid(opacity_); }
	torch::Tensor getScalingActivation() { return torch::exp(scaling_); }
	torch::Tensor getRotationActivation() { return torch::nn::functional::normalize(rotation_); }
	torch::Tensor getCovarianceActivation() { throw std::runtime_error("refinePose renders the raw model (compute_cov3D_ must be off)"); }
};
}  // namespace

std::tuple<torch::Tensor, torch::Tensor> TrainStep::refinePose(std::shared_ptr<GaussianKeyframe> viewpoint_cam, torch::Tensor gt_image,
                                                              torch::Tensor mask, int iterations, double lr_translation,
                                                              double lr_rotation, torch::Tensor gt_depth)
{
	if (pipe_.convert_SHs_ || pipe_.compute_cov3D_)
		throw std::runtime_error("refinePose renders the raw model (convert_SHs_ / compute_cov3D_ must be off)");
	const bool use_depth = usesDepthLoss(gt_depth);
	auto& g = gaussians_;
	auto frozen = std::make_shared<FrozenModel>();
	frozen->xyz_ = g->xyz_.detach();
	frozen->opacity_ = g->opacity_.detach();
	frozen->scaling_ = g->scaling_.detach();
	frozen->rotation_ = g->rotation_.detach();
	frozen->features_ = g->features_.detach();
	frozen->active_sh_degree_ = g->active_sh_degree_;
	frozen->max_sh_degree_ = g->max_sh_degree_;
	if (g->features_row_step_.defined() && !g->features_lr_hist_.empty() && g->groups_.size() > 1) {
		// lazily stepped SH rows: the zero-gradient steps the rows are behind are taken on COPIES (one copy per call, nothing per
		// iteration) -- neither the tensor, its moments nor row_step change
		torch::NoGradGuard ng;
		ShAdamStep s = g->featuresAdamStep(GaussianModel::ShStep::LazyTaken);
		s.exp_avg = s.exp_avg.clone();
		s.exp_avg_sq = s.exp_avg_sq.clone();
		s.row_step = s.row_step.clone();
		frozen->features_ = frozen->features_.clone();
		shAdamFlush(frozen->features_, s);
	}
	PoseDelta pose(viewpoint_cam->world_view_transform_, viewpoint_cam->full_proj_transform_);
	auto kf = std::make_shared<GaussianKeyframe>(*viewpoint_cam);
	const auto opts = pose.xi_.options().requires_grad(false);
	auto lr = torch::cat({torch::full({3}, lr_translation, opts), torch::full({3}, lr_rotation, opts)});
	auto m = torch::zeros({6}, opts), v = torch::zeros({6}, opts);
	const double b1 = 0.9, b2 = 0.999, eps = 1e-8;
	const torch::Tensor eff_mask = effectiveMask(mask);
	GaussianRasterizationExtensions ext = baseExtensions(&view_workspace_);
	ext.filter_3D_ = viewFilter3D();   // (one call per refinement, not per iteration)
	// (a keyframe's exposure is applied, not optimised)
	const torch::Tensor exposure = viewpoint_cam->exposure_.defined() ? viewpoint_cam->exposure_.detach() : torch::Tensor();
	std::vector<torch::Tensor> losses;
	for (int it = 1; it <= iterations; it++) {
		pose.apply(*kf);
		auto pkg = renderModel(*this, kf, frozen, ext, use_depth);
		auto loss = stepLoss(std::get<0>(pkg), std::get<4>(pkg), exposure, gt_image, eff_mask, gt_depth, use_depth);
		auto grad = torch::autograd::grad({loss}, {pose.xi_})[0];
		{
			torch::NoGradGuard ng;
			m.mul_(b1).add_(grad, 1.0 - b1);
			v.mul_(b2).addcmul_(grad, grad, 1.0 - b2);
			auto step = lr / (1.0 - std::pow(b1, it));
			pose.xi_.sub_(step * m / (v.sqrt() / std::sqrt(1.0 - std::pow(b2, it)) + eps));
		}
		losses.push_back(loss.detach());
	}
	auto w2c = pose.retract();
	return std::make_tuple(w2c, losses.empty() ? torch::zeros({0}, opts) : torch::stack(losses));
}

// ---- the stages of renderAndBackward, in the order it runs them
// Every refusal of a step, before anything of it happens (iteration_ has not advanced); what the last step left for its readers (the
// pending exposure step, lastRegLosses(), lastAbsgrad()) is dropped at the points it always was: a refused call leaves the same state
void TrainStep::checkStepSupported(const std::shared_ptr<GaussianKeyframe>& kf, bool use_depth, bool use_prior)
{
	if (use_depth) requireSingleProcess("the depth loss is", false, " (depth_loss_weight_ must be 0)");
	if (use_prior) requireSingleProcess("the depth prior is", false, " (depth_prior_weight_ must be 0)");
	exposure_kf_.reset();
	exposure_grad_ = torch::Tensor();
	if (kf->exposure_.defined() || optimize_exposure_) requireSingleProcess("exposure compensation is", false);
	if (usesGeomReg()) requireSingleProcess("the opacity / scale / isotropy regularisers are", true);
	if (mcmc_) requireSingleProcess("mcmc_ is", true);
	if (absgrad_) requireSingleProcess("absgrad_ is", true);
	checkFilter3D();   // (refuses a process group and a missing camera list)
	last_reg_losses_ = torch::Tensor();
	last_absgrad_ = torch::Tensor();
	last_depth_prior_fit_ = torch::Tensor();
	if (optimize_exposure_ && !kf->exposure_.defined())   // the identity at first use (created before the check it always passes)
		kf->exposure_ = torch::eye(3, 4, gaussians_->xyz_.options().requires_grad(false));
	if (kf->exposure_.defined() && (kf->exposure_.dim() != 2 || kf->exposure_.size(0) != 3 || kf->exposure_.size(1) != 4 ||
	                                kf->exposure_.scalar_type() != torch::kFloat32 || !kf->exposure_.is_contiguous()))
		throw std::runtime_error("a keyframe's exposure_ must be a contiguous float32 [3, 4] tensor");
}

// the buffers of the view-factored exchange (none without it): this view's message and what the gather of this step writes
void TrainStep::prepareExchangeBuffers(const std::shared_ptr<GaussianKeyframe>& kf)
{
	auto& g = gaussians_;
	if (!factored_exchange_) {
		sh_send_ = torch::Tensor();
		sh_grad_view_ = torch::Tensor();
		sh_gathered_ = torch::Tensor();
		packed_this_step_ = false;
		return;
	}
	const auto P = g->xyz_.size(0);
	sh_send_ = torch::empty({P + 1, 3}, g->xyz_.options().requires_grad(false));
	sh_grad_view_ = sh_send_.narrow(0, 0, P);
	sh_send_.select(0, P).copy_(kf->camera_center_.detach().reshape({3}));
	// the packed form needs the fused [P,16,3] step of the views (the other layouts take the dense route)
	packed_this_step_ = packed_exchange_ && process_group_ && g->features_.size(1) == 16 && g->groups_.size() > 1 &&
	                    g->features_.is_contiguous() && !pipe_.convert_SHs_;
	if (process_group_ && !packed_this_step_) {
		const int64_t N = process_group_->getSize();
		if (!sh_gathered_.defined() || sh_gathered_.size(0) != N || sh_gathered_.size(1) != P + 1 ||
		    sh_gathered_.device() != sh_send_.device())
			sh_gathered_ = torch::empty({N, P + 1, 3}, sh_send_.options());
	}
	if (packed_this_step_) {
		// persistent message buffers sized for the worst case (every Gaussian visible), allocated HERE -- before the passes
		// are enqueued, like sh_gathered_
		const int64_t N = process_group_->getSize(), words = packedViewWords(P, (P + 3) / 4 * 4);
		const auto io = sh_send_.options().dtype(torch::kInt32);
		if (!sh_packed_send_.defined() || sh_packed_send_.numel() != words || sh_packed_send_.device() != sh_send_.device()) {
			sh_packed_send_ = torch::empty({words}, io);
			sh_packed_gathered_ = torch::empty({N * words}, io);
			sh_gathered_ = torch::Tensor();
		}
		if (sh_packed_gathered_.numel() != N * words) sh_packed_gathered_ = torch::empty({N * words}, io);
	}
}

// the three regularisers; returns the [3] tensor their loss values are written to (formed only when somebody reads them)
torch::Tensor TrainStep::planRegularisers(GaussianRasterizationExtensions& ext) const
{
	if (!usesGeomReg()) return torch::Tensor();
	ext.opacity_reg_ = opacity_reg_;
	ext.scale_reg_ = scale_reg_;
	ext.isotropic_reg_ = isotropic_reg_;
	if (read_reg_losses_) ext.reg_loss_ = torch::zeros({3}, gaussians_->xyz_.options().dtype(torch::kFloat32).requires_grad(false));
	return ext.reg_loss_;
}

// The Adam step of the SH tensor this iteration takes outside optimizerStepGroup(1), if any; returns whether its rows step lazily.
// The step counter advances HERE, so the step is planned only when render() will really hand it to the rasterizer
// (gaussian_renderer.h: sh_in_rasterizer): with convert_SHs_ the rasterizer sees colours, not the SH tensor -- autograd then leaves
// a dense gradient and optimizerStepGroup() takes the step.
bool TrainStep::planFeaturesStep(GaussianRasterizationExtensions& ext, bool rebuilds)
{
	auto& g = gaussians_;
	auto steppable = [&] {
		return !rebuilds && iteration_ < g->opt_.iterations_ && g->groups_.size() > 1 && g->features_.size(1) == 16 && !pipe_.convert_SHs_;
	};
	bool lazy = false;
	if (fused_sh_adam_ && !factored_exchange_ && steppable()) {   // the step happens inside backward
		lazy = lazy_sh_adam_window_ >= 2 && g->features_.is_contiguous();
		ext.sh_adam_ = g->beginFeaturesStep(lazy, lazy_sh_adam_window_);
	}
	// Data-parallel step with the view-factored exchange: the SH rows step AFTER the exchange (stepFeaturesFromViews), and lazily
	// there too -- a row no view of the batch lights takes a zero-gradient step, i.e. it may take it later.  The forward pass
	// gets the same struct, so that the rows THIS view sees are up to date before they are evaluated; backward (factored mode)
	// uses it only to run this step's slice of the rows' rotating catch-up next to the blend kernel.
	views_adam_ = ShAdamStep();
	views_adam_pending_ = false;
	if (factored_exchange_ && lazy_sh_adam_window_ >= 3 && steppable() && g->features_.is_contiguous()) {
		lazy = true;
		ext.sh_adam_ = g->beginFeaturesStep(true, lazy_sh_adam_window_);
		views_adam_ = ext.sh_adam_;
		views_adam_pending_ = true;
	}
	if (!lazy) g->syncFeatures();   // the render reads every visible row as it is
	return lazy;
}

// how the passes overlap with the exchange: the gather's own stream, the SH step's two scheduling switches, the prepacked message
void TrainStep::planExchangeOverlap(GaussianRasterizationExtensions& ext)
{
	auto& g = gaussians_;
#ifndef GSR_HOST_NO_HIP
	// early_gather_ (GSR_EARLY_GATHER=0/1 overrides): off = the gather is issued on the compute stream behind the whole backward pass
	static const int early_env = [] { const char* e = getenv("GSR_EARLY_GATHER"); return (e && *e) ? (atoi(e) != 0 ? 1 : 0) : -1; }();
	const bool early_gather = early_env >= 0 ? early_env != 0 : early_gather_;
	gather_stream_in_use_ = false;
	if (early_gather && factored_exchange_ && process_group_ && g->xyz_.is_cuda()) {
		// the exchange's gather waits for the colour gradients only, not for the whole backward pass (keyframe_batch_exchange.cpp)
		if (!gather_stream_) gather_stream_ = c10::hip::getStreamFromPool(/*isHighPriority=*/false, g->xyz_.device().index()).stream();
		ext.color_view_ready_stream_ = gather_stream_;
		gather_stream_in_use_ = true;
	}
#endif
	ext.sh_adam_.no_side_stream = no_side_stream_;
	ext.sh_adam_.lazy_slice_late = lazy_slice_late_;
	// packed exchange: the backward pass writes this view's message itself (rows + header; the mask / prefix sections are
	// planned from the radii right behind the forward pass) -- no pack launches between the backward pass and the gather
	static const int pack_env = [] { const char* e = getenv("GSR_PACK_IN_BACKWARD"); return (e && *e) ? (atoi(e) != 0 ? 1 : 0) : -1; }();
	prepacked_this_step_ = packed_this_step_ && (pack_env >= 0 ? pack_env != 0 : pack_in_backward_);
	if (prepacked_this_step_) {
		ext.packed_view_ = sh_packed_send_;
		ext.packed_capacity_ = (g->xyz_.size(0) + 3) / 4 * 4;
	}
}

// The Adam steps of xyz, opacity, scaling, rotation = groups 0, 2, 3, 4 (trainingSetup) inside backward, on the iterations the SH
// step is fused on; optimizerStepGroup() then finds no gradient on them.  With compute_cov3D_ the rasterizer sees a covariance,
// not the raw scaling / rotation leaves, and the groups take their dense steps.
// (resets: an iteration that resets the opacity replaces that leaf AFTER backward: the reference's optimizer step then skips it --
// no gradient -- while a step fused into backward would already have been taken: src/gaussian_mapper.cpp:732-735)
void TrainStep::planGeomStep(GaussianRasterizationExtensions& ext, bool resets)
{
	auto& g = gaussians_;
	if (!(fused_geom_adam_ && !factored_exchange_ && ext.sh_adam_.exp_avg.defined() && g->groups_.size() == 5 && !pipe_.compute_cov3D_ && !resets))
		return;
	GeomAdamStep& geom_adam = ext.geom_adam_;
	for (int gi : {0, 2, 3, 4}) {
		auto& grp = g->groups_[static_cast<size_t>(gi)];
		grp.step++;
		geom_adam.param.push_back(grp.param.detach());
		geom_adam.exp_avg.push_back(grp.exp_avg);
		geom_adam.exp_avg_sq.push_back(grp.exp_avg_sq);
		geom_adam.lr.push_back(grp.lr * g->lr_scale_);
		geom_adam.step.push_back(grp.step);
	}
}

void TrainStep::planStatistics(GaussianRasterizationExtensions& ext)
{
	auto& g = gaussians_;
	// the statistics are fused (or over) in every mode of this step: nobody reads the viewspace gradient or dL_dcov3D
	ext.training_outputs_only_ = true;
	// the densification statistics of this view (:714-719) are added by the backward kernel that holds dL_dmean2D in registers
	if (iteration_ < g->opt_.densify_until_iter_) ext.view_stats_ = {g->xyz_gradient_accum_, g->denom_, g->max_radii2D_};
	// AbsGS: the statistics accumulate the norm of the absolute pair (only they read it)
	if (absgrad_ && !ext.view_stats_.empty())
		ext.absgrad_ = last_absgrad_ = torch::empty({g->xyz_.size(0), 2}, g->xyz_.options().requires_grad(false));
}

// rendered * mask with a mask of ones is the identity (src/gaussian_mapper.cpp:692-693; most keyframes carry a full mask):
// recognised ONCE per mask tensor (one reduction + host read when a keyframe's mask is first seen); the loss kernels then skip its
// 2 x 25 MB of reads at 1080p.  Returns the mask, or an empty tensor for one of ones (= none: FusedL1SSIMFunction::forward).
torch::Tensor TrainStep::effectiveMask(const torch::Tensor& mask)
{
	if (!mask.defined() || !mask.numel()) return mask;
	// remembered per TensorImpl through a weak pointer (it keeps the object's address from being reused by another tensor
	// after this one is freed) together with the version counter (in-place writes invalidate the entry)
	auto* impl = mask.unsafeGetTensorImpl();
	const int64_t version = static_cast<int64_t>(mask._version());
	auto it = mask_is_ones_.find(impl);
	if (it == mask_is_ones_.end() || it->second.self.expired() || it->second.version != version) {
		if (mask_is_ones_.size() >= 64) mask_is_ones_.clear();
		torch::NoGradGuard ng;
		MaskEntry e;
		e.self = c10::weak_intrusive_ptr<c10::TensorImpl, c10::UndefinedTensorImpl>(mask.getIntrusivePtr());
		e.version = version;
		e.ones = (mask == 1).all().item<bool>();
		it = mask_is_ones_.insert_or_assign(impl, std::move(e)).first;
	}
	return it->second.ones ? torch::empty({0}, mask.options()) : mask;
}

// the loss of a step and of a pose refinement: fused L1 + lambda_dssim_ (1 - SSIM) behind `exposure` (if defined), plus the depth L1
// term.  The caller calls backward() on this very value (is_root; the sum's backward hands both terms the root's exact 1).
torch::Tensor TrainStep::stepLoss(const torch::Tensor& rendered, const torch::Tensor& depth, const torch::Tensor& exposure, const torch::Tensor& gt_image,
                                  const torch::Tensor& eff_mask, const torch::Tensor& gt_depth, bool use_depth) const
{
	const float lambda_dssim = gaussians_->opt_.lambda_dssim_;
	auto loss = exposure.defined() ? loss_utils::fused_l1_ssim_exposure(rendered, gt_image, eff_mask, lambda_dssim, exposure, /*is_root=*/true)
	                               : fusedL1SSIMLoss(rendered, gt_image, eff_mask, lambda_dssim, /*is_root=*/true);
	if (use_depth) loss = loss + loss_utils::depth_l1(depth, gt_depth, depth_loss_weight_, depth_min_, depth_max_);
	return loss;
}

torch::Tensor TrainStep::renderAndBackward(std::shared_ptr<GaussianKeyframe> kf, torch::Tensor gt_image, torch::Tensor mask,
                                           torch::Tensor gt_depth, torch::Tensor prior_depth)
{
	const bool use_depth = usesDepthLoss(gt_depth), use_prior = usesDepthPrior(prior_depth);
	checkStepSupported(kf, use_depth, use_prior);
	auto& g = gaussians_;
	iteration_++;
	// the position learning rate follows the iteration (src/gaussian_mapper.cpp:672-674) or -- a SLAM session -- the number of
	// times THIS keyframe has been used (:663-671): the caller says which through position_lr_step_
	g->updateLearningRate(position_lr_step_ >= 0 ? std::min(position_lr_step_, g->opt_.position_lr_max_steps_) : iteration_);
	prepareExchangeBuffers(kf);
	// the extensions of this step's render, and what the stages below switch on
	GaussianRasterizationExtensions ext = baseExtensions(&workspace_);
	ext.sh_grad_view_ = sh_grad_view_;
	// the 3-D smoothing filter: recomputed when undefined and every filter3d_interval_ iterations, before this iteration's render
	ext.filter_3D_ = viewFilter3D(filter3d_interval_ > 0 && iteration_ % filter3d_interval_ == 0);
	const torch::Tensor reg_loss = planRegularisers(ext);
	const bool lazy = planFeaturesStep(ext, densifyDue());
	planExchangeOverlap(ext);
	planGeomStep(ext, opacityResetDue());
	planStatistics(ext);
	// (with the depth loss: the same render with the depth and alpha maps appended, GaussianRenderer::renderWithDepth)
	RenderPackage pkg;
	{
		g->in_lazy_step_ = lazy;
		ScopeExit clear{[&] { g->in_lazy_step_ = false; }};   // (on every way out of the render)
		pkg = renderModel(*this, kf, g, ext, use_depth || use_prior);
	}
	if (factored_exchange_ && packed_this_step_) beginCountExchange();   // (the forward pass has left this view's visible count)
	if (prepacked_this_step_) planPackedView(std::get<3>(pkg));
	last_viewspace_ = std::get<1>(pkg);
	last_visibility_ = std::get<2>(pkg);
	last_radii_ = std::get<3>(pkg);
	const torch::Tensor eff_mask = effectiveMask(mask);
	torch::Tensor exposure_leaf;   // (a leaf of this step's graph: the keyframe's tensor itself is stepped in place afterwards)
	if (kf->exposure_.defined()) exposure_leaf = kf->exposure_.detach().set_requires_grad(optimize_exposure_);
	auto loss = stepLoss(std::get<0>(pkg), std::get<4>(pkg), exposure_leaf, gt_image, eff_mask, gt_depth, use_depth);
	if (use_prior)   // (not in stepLoss: refinePose shares that and takes no prior)
		loss = loss + loss_utils::depth_prior(std::get<4>(pkg), std::get<5>(pkg), prior_depth, depth_prior_weight_, depth_prior_inverse_,
		                                      depth_prior_pearson_, depth_prior_alpha_min_, torch::Tensor(), &last_depth_prior_fit_);
	// the root gradient: a cached 1 instead of the ones_like fill autograd launches per backward()
	if (!root_grad_.defined() || root_grad_.device() != loss.device()) root_grad_ = torch::ones_like(loss).detach();
	loss.backward(root_grad_);
	if (reg_loss.defined()) {
		// the returned loss = photometric (+ depth) + the three terms the backward pass has just written
		last_reg_losses_ = reg_loss;
		loss = loss.detach() + reg_loss.sum();
	}
	if (optimize_exposure_ && exposure_leaf.defined()) {
		exposure_kf_ = kf;
		exposure_grad_ = exposure_leaf.grad();
	}
	// the step is taken: its learning rates join the history the later catch-ups need (the factored step: finishFeaturesFromViews)
	if (lazy && !views_adam_pending_) g->endFeaturesStep(ext.sh_adam_);
	return loss;
}

void TrainStep::finishOneIteration()
{
	finishBegin();
	if (iteration_ < gaussians_->opt_.iterations_)
		for (int i = 0; i < static_cast<int>(gaussians_->groups_.size()); i++) gaussians_->optimizerStepGroup(i);
	finishEnd();
}

void TrainStep::setFeaturesGradFromViews(torch::Tensor campos_views, torch::Tensor dL_dcolor_views)
{
	torch::NoGradGuard ng;
	auto& g = gaussians_;
	if (views_adam_pending_) {
		// the dense route after all: the lazy step renderAndBackward() announced is withdrawn (its counter, not yet its learning
		// rates, had been recorded) and every row catches up to the steps really taken
		views_adam_pending_ = false;
		views_adam_ = ShAdamStep();
		g->groups_[1].step--;
	}
	g->syncFeatures();
	g->features_.mutable_grad() =
	    shGradFromViews(g->xyz_.detach(), campos_views, dL_dcolor_views, g->active_sh_degree_,
	                    static_cast<int>(g->features_.size(1)), 1.0f / static_cast<float>(dL_dcolor_views.size(0)));
}

void TrainStep::stepFeaturesFromViews(torch::Tensor campos_views, torch::Tensor dL_dcolor_views, int64_t row0, bool first_part)
{
	torch::NoGradGuard ng;
	auto& g = gaussians_;
	if (iteration_ >= g->opt_.iterations_) return;
	const int64_t P = g->xyz_.size(0), n = dL_dcolor_views.size(1);
	if (row0 < 0 || row0 + n > P) throw std::runtime_error("stepFeaturesFromViews: the part exceeds the Gaussians");
	if (!views_adam_pending_) {
		g->syncFeatures();
		if (g->features_.size(1) != 16 || g->groups_.size() < 2) {   // other layouts: gradient tensor + separate pass (whole batch only)
			if (row0 != 0 || n != P) throw std::runtime_error("stepFeaturesFromViews: parts need the [P,16,3] SH layout");
			setFeaturesGradFromViews(campos_views, dL_dcolor_views);
			finishAdamGroup(1);
			return;
		}
	}
	// lazy rows: renderAndBackward() advanced the step counter and prepared the struct; rows no view lights stay behind.  Otherwise
	// the eager step of every row, whose counter advances with the first part only
	ShAdamStep a = views_adam_pending_ ? views_adam_ : first_part ? g->beginFeaturesStep(false, 0) : g->featuresAdamStep(GaussianModel::ShStep::Eager);
	a.exp_avg = a.exp_avg.narrow(0, row0, n);
	a.exp_avg_sq = a.exp_avg_sq.narrow(0, row0, n);
	if (a.row_step.defined()) a.row_step = a.row_step.narrow(0, row0, n);
	auto sh = g->features_.detach().narrow(0, row0, n);
	shAdamFromViews(g->xyz_.detach().narrow(0, row0, n), campos_views, dL_dcolor_views, g->active_sh_degree_,
	                1.0f / static_cast<float>(dL_dcolor_views.size(0)), sh, a);
}

void TrainStep::stepFeaturesFromPackedViews(torch::Tensor messages, int64_t msg_stride, int64_t n_views)
{
	torch::NoGradGuard ng;
	auto& g = gaussians_;
	if (iteration_ >= g->opt_.iterations_) return;
	const float scale = 1.0f / static_cast<float>(n_views);
	auto sh = g->features_.detach();
	if (views_adam_pending_) {   // lazy rows: renderAndBackward() advanced the step counter and prepared the struct
		shAdamFromPackedViews(g->xyz_.detach(), messages, msg_stride, n_views, g->active_sh_degree_, scale, sh, views_adam_);
		return;
	}
	g->syncFeatures();
	shAdamFromPackedViews(g->xyz_.detach(), messages, msg_stride, n_views, g->active_sh_degree_, scale, sh, g->beginFeaturesStep(false, 0));
}

void TrainStep::finishFeaturesFromViews()
{
	if (!views_adam_pending_) return;
	torch::NoGradGuard ng;
	views_adam_pending_ = false;
	// (the rotating catch-up that bounds the lag of the rows no view lights ran inside the rasterizer's backward, next to the
	// blend kernel: gsr_backward_args.sh_adam together with dL_dcolor_view)
	gaussians_->endFeaturesStep(views_adam_);   // the step is taken: its learning rates join the history the later catch-ups need
	views_adam_ = ShAdamStep();
}

void TrainStep::finishGeomAdam(float grad_scale)
{
	torch::NoGradGuard ng;
	auto& g = gaussians_;
	if (iteration_ >= g->opt_.iterations_) return;
	if (g->groups_.size() != 5) {
		// another parameter layout than trainingSetup()'s five groups: every group but the SH tensor's (stepped from the views)
		// takes its own pass, the 1/N of the summed gradients applied first -- never a silent return: in the factored
		// data-parallel step this function is the ONLY consumer of those gradients
		for (int gi = 0; gi < static_cast<int>(g->groups_.size()); gi++) {
			if (gi == 1) continue;
			auto grad = g->groups_[static_cast<size_t>(gi)].param.grad();
			if (!grad.defined()) continue;
			if (grad_scale != 1.0f) grad.mul_(grad_scale);
			finishAdamGroup(gi);
		}
		return;
	}
	std::vector<AdamMultiEntry> entries;
	for (int gi : {0, 2, 3, 4}) {
		auto& grp = g->groups_[static_cast<size_t>(gi)];
		auto grad = grp.param.grad();
		if (!grad.defined()) continue;   // (the iteration that rebuilt the tensors: no gradient, the step counter rests)
		grp.step++;
		AdamMultiEntry e;
		e.param = grp.param.detach();
		e.grad = grad.contiguous();
		e.exp_avg = grp.exp_avg;
		e.exp_avg_sq = grp.exp_avg_sq;
		e.lr = grp.lr * g->lr_scale_;
		e.step = grp.step;
		e.grad_scale = grad_scale;
		entries.push_back(e);
	}
	adamStepMulti(entries, 0.9, 0.999, 1e-15);
	for (int gi : {0, 2, 3, 4}) g->groups_[static_cast<size_t>(gi)].param.mutable_grad() = torch::Tensor();
}

void TrainStep::finishAdamGroup(int group)
{
	if (iteration_ < gaussians_->opt_.iterations_) gaussians_->optimizerStepGroup(group);
}

void TrainStep::finishEnd()
{
	finishFeaturesFromViews();   // (a driver that forgot the slice: the lazy state stays consistent)
	if (iteration_ < gaussians_->opt_.iterations_) gaussians_->zeroGrad();
	if (mcmc_ && iteration_ < gaussians_->opt_.iterations_ && !gaussians_->groups_.empty())
		gaussians_->addPositionNoise(static_cast<float>(mcmc_noise_lr_ * gaussians_->groups_[0].lr * gaussians_->lr_scale_), generator_);
	finishExposure();   // the keyframe's exposure takes its own step, on densifying iterations too (it is not rebuilt)
}

bool TrainStep::densifyDue() const
{
	const auto& o = gaussians_->opt_;
	return densify_ && iteration_ < o.densify_until_iter_ && iteration_ > o.densify_from_iter_ && o.densification_interval_ &&
	       iteration_ % o.densification_interval_ == 0;
}

void TrainStep::finishBegin()
{
	torch::NoGradGuard ng;
	auto& g = gaussians_;
	// (the statistics of :714-719 were added inside backward: view_stats)
	if (densifyDue()) {
		const int size_threshold = iteration_ > prune_big_point_after_iter_ ? 20 : 0;   // src/gaussian_mapper.cpp:723
		g->zeroGrad();   // shapes change; this step's update is skipped
		last_absgrad_ = torch::Tensor();   // (its rows are those of the model before the rebuild)
		if (mcmc_) {
			last_mcmc_counts_ = g->relocateDead(mcmc_min_opacity_, generator_);
			g->addNew(mcmc_cap_max_, generator_, mcmc_min_opacity_);
		} else {
			// (AbsGS: the accumulator holds the absolute statistic, which has its own threshold)
			const float max_grad = absgrad_ ? densify_abs_grad_threshold_ : g->opt_.densify_grad_threshold_;
			last_densify_ = g->densifyAndPrune(max_grad, densify_min_opacity_, cameras_extent_, size_threshold, generator_);
		}
	}
	if (opacityResetDue()) g->resetOpacity();
	if (iteration_ < g->opt_.iterations_) g->beginOptimizerStep();
}
