// gaussian_model_lite.h -- the slice of GaussianModel / GaussianKeyframe the measured train step
// needs (include/gaussian_model.h:59-193, include/gaussian_keyframe.h:36-136 of the reference),
// LibTorch only -- the reference classes pull in OpenCV, Eigen, Sophus and ORB-SLAM3, none of which
// exist in this environment.  Member names follow the reference so GaussianRenderer::render is the
// same code for both.
#pragma once
#include <torch/torch.h>
#include <torch/csrc/distributed/c10d/ProcessGroup.hpp>

#include <array>
#include <cmath>
#include <limits>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "gaussian_rasterizer.h"   // GaussianRasterizationExtensions; rasterize_points.h: ShAdamStep, RasterWorkspace

struct GaussianOptimizationParams {  // include/gaussian_parameters.h:61-96 defaults
	int iterations_ = 30000;
	float position_lr_init_ = 0.00016f, position_lr_final_ = 0.0000016f, position_lr_delay_mult_ = 0.01f;
	int position_lr_max_steps_ = 30000;
	float feature_lr_ = 0.0025f, opacity_lr_ = 0.05f, scaling_lr_ = 0.005f, rotation_lr_ = 0.001f;
	float percent_dense_ = 0.01f, lambda_dssim_ = 0.2f;
	int densification_interval_ = 100, opacity_reset_interval_ = 3000, densify_from_iter_ = 500,
	    densify_until_iter_ = 15000;
	float densify_grad_threshold_ = 0.0002f;
};

#ifndef GSR_HAVE_PIPELINE_PARAMS
#define GSR_HAVE_PIPELINE_PARAMS
struct GaussianPipelineParams {   // include/gaussian_parameters.h:41-49
	bool convert_SHs_ = false;
	bool compute_cov3D_ = false;
};
#endif

struct GaussianKeyframe {
	int image_height_ = 0, image_width_ = 0;
	float FoVx_ = 0.f, FoVy_ = 0.f;
	torch::Tensor world_view_transform_, full_proj_transform_, camera_center_;
	// Exposure compensation (include/gsr.h: gsr_l1_ssim_loss_exposure): the keyframe's [3,4] affine colour map between render and
	// loss, float32 on the device; undefined = no compensation, the plain loss kernels.  It belongs to the keyframe, not to the
	// map: its Adam moments and its own step count travel with it (TrainStep::optimize_exposure_).
	torch::Tensor exposure_, exposure_exp_avg_, exposure_exp_avg_sq_;
	int exposure_step_ = 0;
};

// One Adam parameter group of the fused optimizer (gsr_adam_step)
struct AdamGroup {
	torch::Tensor param, exp_avg, exp_avg_sq;
	double lr = 0.0, lr_tail = 0.0;   // torch::optim::AdamOptions::lr is double (set_lr(float) widens: src/gaussian_model.cpp:489-502)
	int period = 0, split = 0;
	int step = 0;   // per parameter, as torch::optim::AdamParamState: advances only when the parameter has a gradient
};

// runs f on every way out of the scope it is declared in, an exception's included
template <class F> struct ScopeExit { F f; ~ScopeExit() { f(); } };
template <class F> ScopeExit(F) -> ScopeExit<F>;

class GaussianModel {
public:
	GaussianModel(int sh_degree, torch::Tensor xyz, torch::Tensor features, torch::Tensor opacity, torch::Tensor scaling,
	              torch::Tensor rotation, float spatial_lr_scale);
	explicit GaussianModel(int sh_degree);   // empty model: createFromPcd() next

	// map maintenance (src/gaussian_model_densify.cpp; include/gaussian_model.h:72-137 of the reference)
	void createFromPcd(torch::Tensor points, torch::Tensor colors, float spatial_lr_scale);
	// src/gaussian_model.cpp:188-376, both overloads: new SLAM map points join the model (colours -> SH DC term, scales from
	// distCUDA2 AMONG THE NEW POINTS, identity rotations, opacity 0.1, exist_since_iter = iteration) through
	// densificationPostfix (:644-712): appended behind the existing rows, zero Adam moments for the new rows, step counters
	// carried, all three statistics arrays reset to zero.  The append is O(new points) while the arena has room (the reference
	// re-cats every tensor and moment and then empties the allocator cache).
	void increasePcd(std::vector<float> points, std::vector<float> colors, const int iteration);
	void increasePcd(torch::Tensor& new_point_cloud, torch::Tensor& new_colors, const int iteration);
	void oneUpShDegree();
	// Loop closure (src/gaussian_model.cpp:379-475; callers: src/gaussian_mapper.cpp loop-closure handling).
	// applyScaledTransformation: every point p <- s R p + t (transformPoints on the scaled positions), then -- exactly as
	// shipped -- `scaling_ *= s` on the LOG-scales (:395; not log(s) added: mirrored, not fixed), and the Adam moments of xyz and
	// scaling are zeroed, their step counters kept (scaledTransformationPostfix -> replaceTensorToOptimizer :567-586).
	// T: the 4x4 matrix [R t; 0 1], row-major (the reference takes a Sophus::SE3f and hands its matrix on).
	void applyScaledTransformation(const float s, torch::Tensor T);
	// The points a keyframe sees and that exist for fewer than stable_num_iter_existence iterations around its creation are
	// moved by diff_pose (scaleAndTransformThenMarkVisiblePoints: positions AND rotations), flags of moved points are cleared,
	// rotation_ becomes the NORMALISED (and rotated) quaternions, moments of xyz and rotation are zeroed (:408-475).
	void scaledTransformVisiblePointsOfKeyframe(torch::Tensor& point_not_transformed_flags, torch::Tensor& diff_pose,
	                                            torch::Tensor& kf_world_view_transform, torch::Tensor& kf_full_proj_transform,
	                                            const int kf_creation_iter, const int stable_num_iter_existence, int& num_transformed,
	                                            const float scale = 1.0f);
	void resetOpacity();
	bool intended_opacity_reset_ = false;   // see resetOpacity(): false = the reference as shipped
	void prunePoints(torch::Tensor& mask);
	// the whole model laid out along a Z-order curve of the positions (gaussian_model_densify.cpp); returns the permutation
	torch::Tensor reorderAlongZCurve();
	struct DensifyResult {
		int64_t cloned = 0, split = 0, pruned = 0, points = 0;
	};
	// generator: the sampler of the split children's positions (every data-parallel rank seeds it identically)
	DensifyResult densifyAndPrune(float max_grad, float min_opacity, float extent, int max_screen_size,
	                              c10::optional<at::Generator> generator = c10::nullopt);

	// Fixed-budget maps: 3DGS-MCMC (include/gsr.h: gsr_mcmc_relocate / gsr_mcmc_add_noise), the other half of the method whose L1
	// terms are TrainStep::opacity_reg_ / scale_reg_.
	// relocateDead: every dead Gaussian (sigmoid(opacity) <= min_opacity) becomes a copy of a live one drawn in proportion to its
	// opacity; the source and its copies share the opacity and scale that leave the render unchanged, their Adam moments are zeroed.
	// IN PLACE: no leaf is replaced and no count is read.  Returns the DEVICE counts (int32 [8]: dead rows, destinations written,
	// sources drawn, the largest N).
	torch::Tensor relocateDead(float min_opacity = 0.005f, c10::optional<at::Generator> generator = c10::nullopt);
	// addNew: the model grows to min(cap_max, floor(1.05 P)) rows (105 P / 100 in integers), the new rows drawn like relocateDead's
	// but over ALL rows; appended through the arena as increasePcd's rows are.  The count is formed on the host, nothing is read
	// back.  Returns the number of rows added (0: nothing happened).
	int64_t addNew(int64_t cap_max, c10::optional<at::Generator> generator = c10::nullopt, float min_opacity = 0.005f);
	// addPositionNoise: xyz += Sigma (z sigmoid(100 ((1 - o) - 0.995)) noise_scale), z ~ N(0, 1) from the generator, in place
	void addPositionNoise(float noise_scale, c10::optional<at::Generator> generator = c10::nullopt);

	// Seeding from an RGB-D frame (include/gsr.h: gsr_seed_select / gsr_seed_emit; SplaTAM's add_new_gaussians, MonoGS's
	// unexplored-region insertion): the pixels of the sensor depth map gt_depth [H,W] that the map does not explain -- alpha <
	// alpha_threshold_ in the map's own render, or the render puts a surface in front of the measured one by more than
	// max(depth_error_abs_, depth_median_factor_ * the median depth error) -- are back-projected through the camera (viewmatrix:
	// world_view_transform_; fx, fy, cx, cy in pixels) and appended as Gaussians of one pixel's footprint, coloured from gt_image
	// [3,H,W] (undefined: DC 0).  alpha / depth: out_alpha / out_depth of a forward-only render of the current map, or undefined
	// for a map that does not exist yet.  gsr_seed_select, ONE read of the counts, room through the arena path of increasePcd /
	// addNew, gsr_seed_emit; at most max_new rows, thinned evenly over the image.  sparse_points_* are not touched.  Returns the
	// number of rows appended; last_seed_counts_ holds the counts read (selected, by the unseen rule, by the depth rule alone,
	// valid pixels, the median's bits) and, with want_pixels_, last_seed_pixels_ the pixel v * W + u of every new row.
	struct SeedOptions {
		float min_depth_ = 0.0f, max_depth_ = std::numeric_limits<float>::infinity();
		float alpha_threshold_ = 0.5f, depth_error_abs_ = 0.0f, depth_median_factor_ = 50.0f;
		int stride_ = 1, offset_x_ = 0, offset_y_ = 0;
		float scale_factor_ = 1.0f, init_opacity_ = 0.5f;
		bool want_pixels_ = false;
	};
	int64_t seedFromDepth(torch::Tensor gt_depth, torch::Tensor gt_image, torch::Tensor alpha, torch::Tensor depth, torch::Tensor viewmatrix,
	                      float fx, float fy, float cx, float cy, int iteration, int64_t max_new, const SeedOptions& options);
	std::vector<int64_t> last_seed_counts_;
	torch::Tensor last_seed_pixels_;

	// activations, src/gaussian_model.cpp:48-71
	torch::Tensor getXYZ() { return xyz_; }
	torch::Tensor getScalingActivation() { return torch::exp(scaling_); }
	torch::Tensor getRotationActivation() { return torch::nn::functional::normalize(rotation_); }
	torch::Tensor getOpacityActivation() { return torch::sigmoid(opacity_); }
	// one [P,16,3] leaf instead of cat(features_dc.clone(), features_rest.clone()) (gaussian_model.cpp:63-66)
	// (lazy SH Adam: outside the fused train step the rows are brought up to date first, see syncFeatures())
	torch::Tensor getFeatures()
	{
		if (!in_lazy_step_) syncFeatures();
		return features_;
	}
	torch::Tensor getCovarianceActivation(int scaling_modifier = 1);   // :73-96

	void trainingSetup(const GaussianOptimizationParams& opt);   // src/gaussian_model.cpp:477-510
	float updateLearningRate(int step);                          // :1118-1131 (exponLrFunc)
	void optimizerStep();                                        // torch::optim::Adam semantics, fused
	// the same step one parameter group at a time (xyz, features, opacity, scaling, rotation), so that a data-parallel
	// driver can update a tensor as soon as ITS gradient reduction has landed
	void beginOptimizerStep() {}   // (the step counters are per group and advance in optimizerStepGroup)
	void optimizerStepGroup(int group);
	void zeroGrad();
	void addDensificationStats(torch::Tensor& viewspace_point_tensor, torch::Tensor& update_filter);  // :817-831
	// ... from the view's [P,2] absolute screen-space gradients instead of the viewspace tensor's gradient (AbsGS:
	// GaussianRasterizationExtensions::absgrad_)
	void addDensificationStats(torch::Tensor& viewspace_point_tensor, torch::Tensor& update_filter, const torch::Tensor& absgrad);
	std::vector<torch::Tensor> params()
	{
		syncFeatures();
		return {xyz_, features_, opacity_, scaling_, rotation_};
	}
	// the five leaves as they are (no catch-up of lazily stepped SH rows): for code that only needs their .grad() inside a step
	std::vector<torch::Tensor> paramsRaw() { return {xyz_, features_, opacity_, scaling_, rotation_}; }

	// Lazy Adam steps for the SH rows of culled Gaussians (gsr_sh_adam_lazy, include/gsr.h; TrainStep::lazy_sh_adam_window_).
	// While features_row_step_ is defined, rows of features_ and of its two moment tensors may be up to `window` zero-gradient
	// steps behind (row i has taken features_row_step_[i] of groups_[1].step steps).  syncFeatures() takes the missing steps
	// (gsr_sh_adam_flush: the same arithmetic, bit-identical to the eager update) and drops the state; everything that reads
	// or rewrites features_ or its moments outside the fused train step calls it first (getFeatures(), params(), the dense
	// optimizer step, densify / prune, savePly, the data-parallel exchange).
	void syncFeatures();
	// The Adam state of the SH tensor (groups_[1], the learning rates scaled by lr_scale_) as the ShAdamStep the rasterizer and
	// the shAdam* functions take (rasterize_points.h); step = the group's counter in every form:
	//   Eager      the step the counter names, every row
	//   Lazy       the same step with the lazy rows' state (row_step, window, the history of the earlier steps' rates)
	//   LazyTaken  the counter's step has been taken: its rates are the newest entry of the history (what shAdamFlush wants)
	enum class ShStep { Eager, Lazy, LazyTaken };
	ShAdamStep featuresAdamStep(ShStep which) const;
	// A step of the SH tensor taken outside optimizerStepGroup(1) (the Python optimizer's begin_fused_step / end_fused_step).  begin:
	// with lazy, the rows' state is created if there is none (a state of another window is flushed first); the counter advances;
	// returns featuresAdamStep(Lazy or Eager).  end (lazy, the step taken): its learning rates join the history, trimmed to the window.
	ShAdamStep beginFeaturesStep(bool lazy, int window);
	void endFeaturesStep(const ShAdamStep& taken);
	torch::Tensor features_row_step_;                            // [P] int32 or undefined (= every row is up to date)
	std::vector<std::pair<double, double>> features_lr_hist_;    // (lr, lr_tail) of the Adam steps since the state exists, newest first
	int features_lazy_window_ = 0;
	bool in_lazy_step_ = false;                                  // set by TrainStep around its own render call

	int max_sh_degree_, active_sh_degree_;
	float spatial_lr_scale_;
	// Multiplies every learning rate where it is consumed.  1 = training.  0 = a STATIONARY workload for throughput
	// measurements: every kernel runs and the Adam moments update, the parameters do not move (bench.py).
	double lr_scale_ = 1.0;
	torch::Tensor xyz_, features_, opacity_, scaling_, rotation_;
	torch::Tensor max_radii2D_, xyz_gradient_accum_, denom_;
	// include/gaussian_model.h:169: the iteration each Gaussian has existed since ([P] int32; read by the loop-closure transform,
	// src/gaussian_model.cpp:433); carried through prune / clone / split (:636, :744, :782) and set by increasePcd (:255)
	torch::Tensor exist_since_iter_;
	torch::Tensor sparse_points_xyz_, sparse_points_color_;   // :182-183: the points handed to increasePcd so far
	GaussianOptimizationParams opt_;
	std::vector<AdamGroup> groups_;

	// arena of the rebuilds (gaussian_model_densify.cpp): optional, created on the first rebuild otherwise
	void reserve(int64_t capacity);
	// checkpoint interchange with the reference and with Inria viewers (src/ply_io.cpp; src/gaussian_model.cpp:838-1047)
	// With filter_3D_ defined a `filter_3D` float property follows the reference's (upstream Mip-Splatting's layout; loadPly takes it
	// when present); without it the file is the reference's, byte for byte.  fused (needs filter_3D_): log(s') and logit(o') of
	// getScalingWithFilter3D / getOpacityWithFilter3D are stored instead and no filter_3D property, so that a viewer without the
	// filter shows the map as it was trained.
	void savePly(const std::string& result_path, bool fused = false);
	void loadPly(const std::string& ply_path);

	// Mip-Splatting's 3-D smoothing filter (include/gsr.h: GSR_FILTER_3D): a [P] float32 tensor, undefined by default.  It belongs to
	// the rows and positions it was computed for: every member that changes the row count, the row order or moves positions
	// wholesale (densifyAndPrune, prunePoints, reorderAlongZCurve, increasePcd, seedFromDepth, relocateDead, addNew, the loop-closure
	// transforms, createFromPcd, loadPly of a file without the property) resets it to undefined -- a stale filter must never be
	// rendered; TrainStep recomputes it (filter3d_).
	torch::Tensor filter_3D_;
	// filter_3D_ from the keyframes that observe each Gaussian (gsr_filter3d_compute): cameras = a float32 [K, 20] tensor of
	// gsr_filter3d_camera rows on the model's device (rasterize_points.h: filter3DCameraRow)
	torch::Tensor computeFilter3D(const torch::Tensor& cameras, float variance = 0.2f);
	// the contract of GSR_FILTER_3D in torch, for export and for callers outside the rasterizer: s'_k = sqrt(s_k^2 + f^2) [P,3] and
	// o' = o (s_0 / s'_0)(s_1 / s'_1)(s_2 / s'_2) [P,1]; throw while filter_3D_ is undefined
	torch::Tensor getScalingWithFilter3D();
	torch::Tensor getOpacityWithFilter3D();
	torch::Device device_ = torch::kCPU;   // where loadPly() / createFromPcd() put a model that has no tensors yet

	// densifyAndPrune lays the new set out along a Z-order curve of the Gaussians' positions (include/gsr.h:
	// gsr_densify_gather_args.morton_scratch): the same Gaussians, values, moments and statistics in another row order -- the
	// per-Gaussian kernels of the following steps then find a view's Gaussians in shared 128-byte lines.  Off by default (the
	// reference's order: kept originals, clones, children).
	bool morton_reindex_ = false;

private:
	torch::Tensor& paramByIndex(int i);
	void replaceParam(int group, torch::Tensor fresh, torch::Tensor exp_avg, torch::Tensor exp_avg_sq, bool rows_kept = false);
	void preloadMaintenanceKernels();   // first-use code-object loads of the ATen kernels behind resetOpacity / loop closure, paid in trainingSetup
	void replaceParamValues(int group, torch::Tensor fresh);   // same shape, zero moments: in place while the leaf lives in the arena
	// gsr_densify_select + one host read + gsr_densify_gather; returns kept, clones, child parents, split, clone-selected, rows
	std::array<int64_t, 6> compact(struct gsr_densify_select_args& sel, c10::optional<at::Generator> generator, bool morton_reindex = false);
	static void* hostStream(const torch::Tensor& t);   // the current HIP stream of the tensor's device (null on the host)
	struct Arena {
		int64_t capacity = 0;
		int cur = 0;
		std::array<std::array<torch::Tensor, 3>, 5> params[2];   // [set][tensor][parameter, exp_avg, exp_avg_sq]
		std::array<torch::Tensor, 3> stats[2];
		torch::Tensor exist[2];   // exist_since_iter_ ([capacity] int32)
	} arena_;
public:
	// densificationPostfix as an append into the arena: what increasePcd and addNew end in (public for the host tests, which hand a
	// model the rows another one was seeded with)
	void appendRows(const std::array<torch::Tensor, 5>& rows, int iteration);
private:
	// the append itself: n rows behind the live ones -- zero moments, exist_since_iter = iteration, the statistics reset; rows
	// null: the parameter rows are left for a kernel to write (seedFromDepth)
	void growRows(int64_t n, int iteration, const std::array<torch::Tensor, 5>* rows);
public:
	// The arena keeps two sets of 1.25-1.5x (parameters + moments) resident (~2 kB per Gaussian) so that rebuilds allocate
	// nothing.  LIFETIME CONTRACT: after a rebuild xyz_, features_, ..., the Adam moments and the statistics are narrow() views
	// into one of the two sets; a tensor obtained BEFORE rebuild N (getXYZ(), a moment, xyz_gradient_accum_ held by a viewer or
	// mapper thread) is overwritten by rebuild N + 2 -- clone() what has to outlive a rebuild (the reference hands out fresh
	// tensors).  releaseArena(): the live tensors move into allocations of their own and both sets are freed (what the
	// reference's emptyCache() after densification achieves, :814) -- call it when densification ends
	// (iteration >= densify_until_iter_) or whenever stable tensors are needed; the next rebuild creates a new arena.
	void releaseArena();
private:
	torch::Tensor densify_scratch_;
	torch::Tensor mcmc_scratch_;
	torch::Tensor seed_scratch_;
	torch::Tensor mcmcCall(int64_t P, int64_t n_add, const torch::Tensor& draws, float min_opacity);
};

// GaussianMapper::trainForOneIteration (src/gaussian_mapper.cpp:614-774) without the SLAM keyframe
// scheduling: render -> masked L1 + lambda (1 - SSIM) -> backward -> statistics -> Adam.
class TrainStep {
public:
	TrainStep(std::shared_ptr<GaussianModel> g, torch::Tensor background) : gaussians_(g), background_(background) {}
	~TrainStep();                                  // releases the HIP events of the data-parallel step (keyframe_batch_exchange.cpp)
	TrainStep(const TrainStep&) = delete;          // (it owns them)
	TrainStep& operator=(const TrainStep&) = delete;
	// ---- 1. calls (then: 2. options, 3. results of the last step, 4. data-parallel state, 5. internal state of a step)
	// forward + backward only (gradients left on the leaves, statistics gathered): lets a data-parallel
	// driver all-reduce before finishOneIteration()
	torch::Tensor renderAndBackward(std::shared_ptr<GaussianKeyframe> kf, torch::Tensor gt_image, torch::Tensor mask)
	{ return renderAndBackward(kf, gt_image, mask, torch::Tensor()); }
	// ... with the keyframe's [H,W] sensor depth (an RGB-D session's img_auxiliary_undist_): with depth_loss_weight_ != 0 the depth
	// L1 loss (loss_utils::depth_l1 over depth_min_ < gt < depth_max_) joins the RGB loss before the one backward pass; undefined
	// gt_depth or weight 0 = the RGB loss alone
	// prior_depth: a monocular network's relative [H,W] map of the keyframe: with depth_prior_weight_ != 0 the depth-prior term
	// (loss_utils::depth_prior on the rendered depth AND alpha maps) joins the loss in the same way; both maps may be given
	torch::Tensor renderAndBackward(std::shared_ptr<GaussianKeyframe> kf, torch::Tensor gt_image, torch::Tensor mask,
	                                torch::Tensor gt_depth, torch::Tensor prior_depth = torch::Tensor());
	void finishOneIteration();
	// finishOneIteration() in three pieces for the overlapped data-parallel step (bench.py): statistics, then Adam per
	// group as the reductions complete, then the gradient reset
	void finishBegin();
	void finishAdamGroup(int group);
	void finishEnd();
	// Keyframe batches over several ranks: every rank accumulates the statistics of ITS views (they are added inside
	// backward); SUM / MAX commute with that accumulation, so the driver reduces xyz_gradient_accum_ and denom_ (SUM) and
	// max_radii2D_ (MAX) over the ranks only before a finishBegin() that will densify -- densifyDue() says when.
	bool densifyDue() const;
	bool opacityResetDue() const   // this iteration's finishBegin() resets the opacity (never with mcmc_)
	{
		const auto& o = gaussians_->opt_;
		return densify_ && !mcmc_ && iteration_ < o.densify_until_iter_ && o.opacity_reset_interval_ && iteration_ % o.opacity_reset_interval_ == 0;
	}
	// renderAndBackward + finishOneIteration; with a process group set, the data-parallel step (trainForOneIterationDataParallel).
	// gt_depth: an RGB-D keyframe, the depth loss of renderAndBackward (not with a process group: throws when the weight is non-zero)
	torch::Tensor trainForOneIteration(std::shared_ptr<GaussianKeyframe> kf, torch::Tensor gt_image, torch::Tensor mask)
	{ return trainForOneIteration(kf, gt_image, mask, torch::Tensor()); }
	// prior_depth: a monocular keyframe, the depth-prior term of renderAndBackward (likewise not with a process group)
	torch::Tensor trainForOneIteration(std::shared_ptr<GaussianKeyframe> kf, torch::Tensor gt_image, torch::Tensor mask,
	                                   torch::Tensor gt_depth, torch::Tensor prior_depth = torch::Tensor());
	// A viewer / evaluation render of the current model (GaussianMapper::renderFromPose, renderAndRecordKeyframe): forward-only
	// (GSR_FORWARD_ONLY) into a second workspace of its own -- a view between a training forward and its backward must not
	// overwrite the buffers that forward saved -- with lazily stepped SH rows read as they are: no flush, no counter advanced,
	// nothing of the model touched.  Returns the [3,H,W] image.
	// apply_exposure: the image behind the keyframe's exposure_ (what the loss compares with the target), if it has one
	torch::Tensor renderView(std::shared_ptr<GaussianKeyframe> kf, bool apply_exposure = false);
	// ... with the depth and alpha maps: (image, depth, alpha), [H,W] each (GaussianRenderer::renderWithDepth)
	std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> renderViewWithDepth(std::shared_ptr<GaussianKeyframe> kf);
	GaussianRasterizationExtensions viewExtensions();   // what the two calls above hand to GaussianRenderer
	// what every render starts from: raw leaves, cull_empty_tiles_, antialiasing_, the workspace; not the filter (viewFilter3D counts)
	GaussianRasterizationExtensions baseExtensions(RasterWorkspace* workspace) const;
	// Photometric refinement of one keyframe's pose against the FROZEN map: `iterations` Adam steps (betas 0.9 / 0.999, eps 1e-8,
	// learning rates lr_translation for rho and lr_rotation for theta) on the xi of a PoseDelta (gaussian_renderer.h) started at
	// viewpoint_cam, minimising the train step's loss -- fused L1 + lambda_dssim_ (1 - SSIM), plus the depth L1 loss with gt_depth
	// when depth_loss_weight_ != 0.  The camera gradients come from the rasterizer's backward (gsr_backward_args.dL_dviewmatrix ...)
	// and reach xi through the pose's construction by autograd.  The map's tensors enter detached, no optimizer or lazy-row state is
	// touched (lazily stepped SH rows: a caught-up copy is rendered), and the render uses the second workspace as renderView does.
	// Returns (the refined W2C [4,4], the loss of every iteration [iterations]).
	std::tuple<torch::Tensor, torch::Tensor> refinePose(std::shared_ptr<GaussianKeyframe> viewpoint_cam, torch::Tensor gt_image,
	                                                    torch::Tensor mask, int iterations, double lr_translation, double lr_rotation,
	                                                    torch::Tensor gt_depth = torch::Tensor());
	// What every Gaussian puts into the given keyframes' images (include/gsr.h: GSR_CONTRIBUTION): one forward-only render per keyframe
	// through the second workspace, exactly as renderView -- lazily stepped SH rows read as they are, nothing of the model or the
	// training workspace touched, cull_empty_tiles_ and antialiasing_ honoured -- with the three statistics accumulating over the
	// keyframes inside the rasterizer.  pixel_weights: empty, or one [H,W] float32 map (finite, >= 0; undefined = ones) per keyframe.
	// Returns (weight_sum, weight_max, n_touched, views_seen): the sum and the maximum over all pixels of all keyframes of
	// w alpha T, the number of blending pixels with w != 0, and the number of keyframes with radii > 0.
	std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor> scoreContribution(
	    const std::vector<std::shared_ptr<GaussianKeyframe>>& keyframes, const std::vector<torch::Tensor>& pixel_weights = {});
	// Scores the keyframes and removes, through prunePoints, the Gaussians that at least min_views of them have in their frustum
	// (radii > 0) and whose largest blending weight alpha T at any pixel of any of them stays below min_weight_max.  A Gaussian no
	// given keyframe sees is kept: not observed is not useless.  Returns the number removed.  Not with a process group: throws.
	int64_t pruneUncontributing(const std::vector<std::shared_ptr<GaussianKeyframe>>& keyframes, float min_weight_max, int min_views = 1);
	// Seeding from an RGB-D frame: the mapper's "where does the map fail to explain this frame, and what do I put there" step.
	// seedFromDepth makes one forward-only render of the map with its depth and alpha maps (renderViewWithDepth; none while the
	// model is empty -- the first frame of a session initialises the map this way) and calls GaussianModel::seedFromDepth with the
	// seed_* options (SplaTAM's values), the valid range depth_min_ < gt < depth_max_ of the depth loss and the rasterizer's
	// own pixel-centre convention fx = W / (2 tanfovx), cx = (W - 1) / 2 (likewise y), so that a seed projects onto the centre of
	// its pixel.  At most mcmc_cap_max_ - P rows with mcmc_ on, seed_max_new_ otherwise.  Returns the number of rows appended.
	// Not with a process group: throws.  Nothing calls it by itself.
	int64_t seedFromDepth(std::shared_ptr<GaussianKeyframe> viewpoint_cam, torch::Tensor gt_image, torch::Tensor gt_depth, int iteration,
	                      bool want_pixels = false);
	// A monocular network's relative [H,W] map in the units of the map: one forward-only render with its depth and alpha maps
	// (renderViewWithDepth), the scale-and-shift fit of the depth-prior loss against it (depth_prior_inverse_, depth_prior_alpha_min_;
	// valid: an optional uint8 / bool [H,W] mask), then gsr_depth_prior_apply.  Returns (the metric [H,W] map -- 0 where the prior is
	// invalid --, fit = [s, t, rho, n] on the device); the map is what seedFromDepth takes as gt_depth.  A degenerate fit
	// (include/gsr.h) gives an all-zero map, which seeds nothing.  An empty model has no render to align to: throws.
	std::tuple<torch::Tensor, torch::Tensor> alignDepthPrior(std::shared_ptr<GaussianKeyframe> viewpoint_cam, torch::Tensor prior,
	                                                         torch::Tensor valid = torch::Tensor());
	// THE refusal of the single-process-only features: throws "TrainStep: <what> not supported with a process group<suffix>" (what =
	// the feature and its verb, "mcmc_ is") with a process group set or -- factored_counts -- with the view-factored exchange on
	void requireSingleProcess(const char* what, bool factored_counts, const char* suffix = "") const;
	// ---- 2. options
	// The depth loss of RGB-D keyframes: depth_loss_weight_ * the L1 distance of the rendered depth map (sum z alpha T) to the
	// sensor's over the pixels with depth_min_ < gt < depth_max_ (RGBD.min_depth / RGBD.max_depth), divided by H W.  0 = off.
	float depth_loss_weight_ = 0.0f;
	float depth_min_ = 0.0f;
	float depth_max_ = std::numeric_limits<float>::infinity();
	bool usesDepthLoss(const torch::Tensor& gt_depth) const { return gt_depth.defined() && depth_loss_weight_ != 0.0f; }
	// Monocular keyframes: depth_prior_weight_ * the depth-prior term (include/gsr.h: gsr_depth_prior_loss) of prior_depth against the
	// rendered depth and alpha maps: the aligned L1 after a per-frame scale-and-shift fit, or 1 - Pearson correlation with
	// depth_prior_pearson_; depth_prior_inverse_: the prior is an inverse depth (MiDaS / Depth Anything); pixels with alpha <
	// depth_prior_alpha_min_ take no part.  0 = off.  lastDepthPriorFit(): [s, t, rho, n] of the last step with the term (device).
	float depth_prior_weight_ = 0.0f;
	bool depth_prior_pearson_ = false;
	bool depth_prior_inverse_ = true;
	float depth_prior_alpha_min_ = 0.5f;
	bool usesDepthPrior(const torch::Tensor& prior_depth) const { return prior_depth.defined() && depth_prior_weight_ != 0.0f; }
	torch::Tensor lastDepthPriorFit() const { return last_depth_prior_fit_; }
	torch::Tensor last_depth_prior_fit_;
	// Per-keyframe exposure compensation (upstream 3DGS's per-image exposure): a keyframe that carries exposure_ has it applied
	// between render and loss, inside the loss kernels, in renderAndBackward and refinePose.  optimize_exposure_: the keyframe of a
	// train step gets the identity at first use and takes one Adam step on its 12 floats in finishEnd() (gsr_adam_step,
	// the model's betas and eps; densifying iterations included), at a learning rate that falls log-linearly from exposure_lr_init_
	// to exposure_lr_final_ over exposure_lr_max_steps_ (< 0: opt_.iterations_) of the keyframe's OWN steps.  refinePose applies
	// a keyframe's exposure and never optimises it.  Not with a process group: throws.
	bool optimize_exposure_ = false;
	float exposure_lr_init_ = 0.01f, exposure_lr_final_ = 0.001f;
	int exposure_lr_max_steps_ = -1;
	double exposureLearningRate(int step) const;   // of a keyframe's `step`-th exposure step (1-based)
	// Regularisers on the Gaussians a view sees, added to the opacity and scale gradients inside the rasterizer's backward
	// (gsr_backward_args.geom_reg; with fused_geom_adam_ in front of the fused step, so nothing reaches HBM for them):
	//   opacity_reg_ * mean_V sigmoid(opacity) + scale_reg_ * mean_V,k exp(scaling)  (the L1 terms of 3DGS-MCMC, which push Gaussians
	//   that explain nothing towards the pruning thresholds) + isotropic_reg_ * mean_V,k |s_k - mean_k s|  (MonoGS)
	// over the V Gaussians with radii > 0 in the view.  All 0 = off: no struct is passed and the kernels are those without it.  Not
	// with a process group: throws.  read_reg_losses_ (the C++ form of the Python host's sync_loss): the three loss values are
	// formed and added to the loss renderAndBackward returns, and lastRegLosses() gives them ([3]; undefined otherwise).  refinePose
	// ignores the three.
	double opacity_reg_ = 0.0, scale_reg_ = 0.0, isotropic_reg_ = 0.0;
	bool read_reg_losses_ = true;
	bool usesGeomReg() const { return opacity_reg_ != 0.0 || scale_reg_ != 0.0 || isotropic_reg_ != 0.0; }
	// Densification by absolute screen-space gradients (AbsGS; gsplat's absgrad): the backward pass sums |d/dmean2D| per pixel
	// before the reduction over a Gaussian's pixels (gsr_backward_args.dL_dmean2D_abs), the fused statistics accumulate the norm of
	// those sums, and densifyAndPrune compares their mean with densify_abs_grad_threshold_ instead of densify_grad_threshold_.
	// 0.0008 is gsplat's recommended value with absgrad: a default for the caller to override, not a tuned number.  Off = the
	// signed statistic and threshold of the reference.  lastAbsgrad(): the [P,2] array of the last step, undefined when that
	// step formed none or rebuilt the model (its rows would be those of the model before the rebuild).  Not
	// with a process group: throws.
	bool absgrad_ = false;
	float densify_abs_grad_threshold_ = 0.0008f;
	// Fixed-budget maps (3DGS-MCMC): with mcmc_ on and densify_ set, the iterations that rebuild today run relocateDead + addNew
	// instead of densifyAndPrune -- the count grows by 5 % per event to exactly mcmc_cap_max_ and then stays, no tensor is rebuilt
	// on a relocation, that iteration's update is skipped as a rebuild's is, and the opacity is never reset -- and every step adds
	// position noise of scale mcmc_noise_lr_ * the current xyz learning rate behind the optimizer update (finishEnd()).  Not with
	// a process group: throws.  Off = nothing changes.
	bool mcmc_ = false;
	int64_t mcmc_cap_max_ = 0;
	double mcmc_noise_lr_ = 5e5;   // (upstream's noise_lr)
	float mcmc_min_opacity_ = 0.005f;
	// the options of seedFromDepth
	float seed_alpha_threshold_ = 0.5f, seed_depth_median_factor_ = 50.0f, seed_depth_error_abs_ = 0.0f;
	int seed_stride_ = 1;
	float seed_scale_factor_ = 1.0f, seed_init_opacity_ = 0.5f;
	int64_t seed_max_new_ = int64_t(1) << 30;
	// Densification schedule of GaussianMapper::trainForOneIteration (src/gaussian_mapper.cpp:711-735), off by default:
	// every densification_interval_ iterations after densify_from_iter_, and the opacity reset.  Runs inside
	// finishBegin(); an iteration that rebuilt the tensors skips its optimizer step exactly as the reference does (the
	// fresh leaves have no gradient).
	bool densify_ = false;
	float cameras_extent_ = 1.0f, densify_min_opacity_ = 0.005f;
	int prune_big_point_after_iter_ = 30000;   // Optimization.prune_big_point_after_iter of the shipped Replica / EuRoC configs (no in-code default in the reference)
	c10::optional<at::Generator> generator_;
	// The step of the position learning-rate schedule for the NEXT iteration(s): -1 = the iteration count (the COLMAP flavour,
	// src/gaussian_mapper.cpp:672-674); a SLAM session sets the keyframe's use count before every iteration (:663-671:
	// kfs_used_times_[fid], capped at position_lr_max_steps_)
	int position_lr_step_ = -1;
	// The Adam step of the SH tensor inside the rasterizer's backward (gsr_backward_args.sh_adam: its gradient rows never
	// reach HBM, 0.13 ms of a 2.3 ms step at C3); same arithmetic as the separate pass.  Not used on an iteration that
	// densifies (the reference skips that optimizer step) nor with the factored exchange.
	bool fused_sh_adam_ = true;
	// ... and the zero-gradient steps of the culled Gaussians' rows taken lazily, at most this many at a time (2 .. 32; 0 = every
	// row at every step): one HBM round trip of a culled row per `window` steps instead of one per step (1.2 GB per step at
	// C3), results bit-identical (GaussianModel::syncFeatures, tests/test_lazy_sh_adam.py)
	int lazy_sh_adam_window_ = 32;
	// The Adam steps of xyz / opacity / scaling / rotation inside the backward kernels that hold their gradients
	// (gsr_backward_args.geom_adam): the 88 B per Gaussian gradient round trip and four optimizer launches disappear; on the
	// same iterations as fused_sh_adam_.  The viewspace gradient and dL_dcov3D are then not written either.
	bool fused_geom_adam_ = true;
	// Scheduling / list-building switches, each at its measured-best value; none changes a result.  They
	// are options of THIS object -- a SLAM process that links the library decides per TrainStep -- and the environment variables
	// of the bench sessions (GSR_CULL_EMPTY_TILES, GSR_EARLY_GATHER, GSR_LAZY_SLICE_EARLY, GSR_SH_ADAM_SIDE_STREAM) only override.
	bool cull_empty_tiles_ = false;   // instances of tiles no pixel of which can blend the Gaussian leave the list (a wash on MI355X)
	bool early_gather_ = true;        // the exchange's all-gather waits for the colour gradients only, not for the whole backward pass
	bool lazy_slice_late_ = false;    // the lazy SH rows' slice behind the backward blend instead of next to it
	bool no_side_stream_ = false;     // no second stream inside gsr_forward / gsr_backward
	// the rasterizer's three scratch buffers are kept across iterations and grown with headroom (workspace_, view_workspace_);
	// false: fresh buffers per call, as the reference's resizeFunctional
	bool persistent_workspace_ = true;
	// Anti-aliased rendering (GSR_ANTIALIAS, include/gsr.h): every render of this object -- the train step at whatever H x W the
	// keyframe's pyramid level has, renderView, refinePose -- compensates the opacity for the 0.3 px low-pass of the projected
	// covariance.  Unlike the switches above it CHANGES the result; densification and pruning keep their thresholds on the
	// uncompensated sigmoid(opacity), as upstream does.
	bool antialiasing_ = false;
	// Mip-Splatting's 3-D smoothing filter (GSR_FILTER_3D, include/gsr.h), the other half of antialiasing_: every Gaussian is bounded
	// from below by the sampling interval of the keyframes that observe it.  With filter3d_ on, the model's filter_3D_ is recomputed
	// from the cameras of setFilterCameras whenever it is undefined (a densification, increasePcd, a loop closure ... reset it) and
	// every filter3d_interval_ iterations (100: upstream's value, a default to override), before that iteration's render, and EVERY
	// render of this object carries it through viewExtensions(): renderAndBackward, renderView, renderViewWithDepth, refinePose,
	// scoreContribution and seedFromDepth's render.  On without cameras: throws.  With a process group: throws.  Densification and
	// pruning thresholds, the MCMC moves and the regularisers stay on the unfiltered parameters, as upstream.
	bool filter3d_ = false;
	int filter3d_interval_ = 100;
	float filter3d_variance_ = 0.2f;
	torch::Tensor filter_cameras_;   // [K, 20] float32 rows of gsr_filter3d_camera on the model's device
	// the keyframes' view matrices with the focal lengths size / (2 tan(FoV / 2)) and the size of each keyframe AS GIVEN: pass it at
	// the finest level it is trained at.  The model's filter is recomputed before the next render.
	// K == 0 and a negative filter3d_variance_ are refused by the first render (viewFilter3D, gsr_filter3d_compute), not here.
	// Works on a model that has no tensors yet (seedFromDepth's start-up): the rows then go to the model's device_.
	void setFilterCameras(const std::vector<std::shared_ptr<GaussianKeyframe>>& keyframes);
	void setFilterCameras(const torch::Tensor& cameras);   // ... or the rows themselves (rasterize_points.h: filter3DCameraRow)
	// the filter every render of this object carries: undefined with filter3d_ off; else the model's filter_3D_, computed first
	// when it is undefined (or `recompute`)
	torch::Tensor viewFilter3D(bool recompute = false);
	void checkFilter3D() const;   // the two refusals of viewFilter3D alone (a process group; no cameras): throws or does nothing
	// pipeline flags of the render call (include/gaussian_parameters.h; every shipped config leaves both off).  The fused
	// optimizer paths above are taken only when render() keeps the tensors they step inside the rasterizer.
	GaussianPipelineParams pipe_;
	// ---- 3. results of the last step
	torch::Tensor lastRegLosses() const { return last_reg_losses_; }
	torch::Tensor last_reg_losses_;
	torch::Tensor lastAbsgrad() const { return last_absgrad_; }
	torch::Tensor last_absgrad_;
	torch::Tensor last_mcmc_counts_;   // the device counts of the last relocateDead
	GaussianModel::DensifyResult last_densify_;
	torch::Tensor last_viewspace_, last_visibility_ /* undefined when the step fused its consumers: last_radii_ > 0 */, last_radii_;
	// renders of this object that were handed the filter (every call of viewFilter3D that returned one; RasterizeGaussiansCUDA
	// refuses a filter whose row count is not the model's): lets a test see that no render went without
	int64_t filter3d_renders_ = 0;
	// exposed communication of the data-parallel step: the time the compute stream spent waiting for a collective (HIP events
	// around every Work::wait(), recorded only while profile_exchange_ is set); read with exchangeWaitMs()
	bool profile_exchange_ = false;
	std::vector<double> exchangeWaitMs();
	void markWait(int k);   // {all-gather wait, all-reduce wait} of the last data-parallel step, in ms
	// ---- 4. data-parallel state
	// Keyframe batches, one keyframe per rank: with a process group set, trainForOneIteration() is the
	// data-parallel step -- render + backward of THIS rank's keyframe, the gradient exchange over c10d (RCCL on the GPU boxes:
	// ViewFactoredExchange by default, the plain GradientReduction otherwise; host/include/keyframe_batch_exchange.h), the
	// optimizer on the batch-mean gradient, and before a densification the SUM / MAX of the per-rank statistics.  Every rank
	// holds a replica; replicas stay bit-identical (identical Adam on identical gradients, identically seeded split samples).
	// No collective is issued from anywhere but here.  A C++ mapper creates c10d::TCPStore + ProcessGroupNCCL and hands the
	// group over; under Python the default group is resolved by name (ops_register.cpp: trainer_set_process_group).
	void setProcessGroup(c10::intrusive_ptr<c10d::ProcessGroup> pg, bool factored = true);
	torch::Tensor trainForOneIterationDataParallel(std::shared_ptr<GaussianKeyframe> kf, torch::Tensor gt_image, torch::Tensor mask);
	c10::intrusive_ptr<c10d::ProcessGroup> process_group_;
	bool factored_exchange_ = false;
	// Data-parallel keyframe batches with the view-factored exchange (include/gsr.h, gsr_sh_grad_from_views): backward
	// then leaves the clamp-masked colour gradient of this view in sh_grad_view_ and no gradient on features_; after the
	// driver has gathered the views of all ranks, setFeaturesGradFromViews() installs the batch-mean SH gradient.  It reads
	// xyz_, so it must run before finishAdamGroup(0).
	torch::Tensor sh_grad_view_;
	void setFeaturesGradFromViews(torch::Tensor campos_views, torch::Tensor dL_dcolor_views);
	// ... or rebuilds it and takes the Adam step of features_ in the same pass (gsr_sh_adam_from_views): the mean gradient
	// never reaches HBM.  Replaces setFeaturesGradFromViews() + finishAdamGroup(1); same ordering constraint.
	// row0 / first_part: the gathered views may arrive in parts (rows [row0, row0 + views.size(1)) of the Gaussians): each
	// part is applied as soon as ITS all-gather has landed, while the next one is still on the links; the Adam step counter
	// advances with the first part only.
	void stepFeaturesFromViews(torch::Tensor campos_views, torch::Tensor dL_dcolor_views, int64_t row0 = 0, bool first_part = true);
	// With lazy_sh_adam_window_ >= 2 the factored step is as lean as the single-GPU one: a row no gathered view lights takes a
	// zero-gradient step, i.e. it may take it LATER (gsr_sh_adam_from_views with sh_adam->lazy) -- renderAndBackward() then
	// advances the SH step counter itself and hands the lazy struct to the forward pass, stepFeaturesFromViews() steps only the
	// lit rows, and finishFeaturesFromViews() -- after the last part -- runs this step's slice of the rotating catch-up and
	// records the step's learning rates.  (finishEnd() calls it if the driver did not.)
	void finishFeaturesFromViews();
	ShAdamStep views_adam_;
	bool views_adam_pending_ = false;
	// xyz / opacity / scaling / rotation in ONE Adam launch (gsr_adam_step_multi): the data-parallel step's four small
	// gradients arrive together from one all-reduce.  Replaces finishAdamGroup(0 / 2 / 3 / 4).  grad_scale: the gradients are
	// multiplied by it as they are read (the 1/N of a batch mean whose all-reduce summed).
	void finishGeomAdam(float grad_scale = 1.0f);
	// The all-gather of the view-factored exchange is issued on a stream of its own that waits only for the point inside
	// backward at which the colour gradients are complete (gsr_backward_args.color_view_ready_stream): it overlaps the SH
	// backward kernel instead of following it.  A hipStream_t from LibTorch's pool, created on first use; null on the host.
	void* gather_stream_ = nullptr;
	bool gather_stream_in_use_ = false;   // this step hands gather_stream_ to the exchange (early_gather_)
	torch::Tensor sh_send_;        // [P + 1, 3]: rows 0 .. P-1 = sh_grad_view_, row P = this view's camera centre (one all-gather)
	// [N, P + 1, 3]: what the all-gather writes.  PERSISTENT (re-allocated only when P or N changes) and sized in
	// renderAndBackward() BEFORE the forward and backward passes are enqueued: the early gather writes it from a second stream
	// that is ordered only behind "the colour gradients are complete", i.e. while the tail of the backward pass still runs -- a
	// buffer taken from the caching allocator at that point could be a block the pass has just released and still writes
	// (record_stream protects the free side, not the first use on a foreign stream).
	torch::Tensor sh_gathered_;
	// The view-factored exchange in its PACKED form (include/gsr.h: gsr_pack_color_view): every rank sends only the rows its
	// view sees -- 11.7 MB instead of 24 MB per rank and link at 2 M Gaussians.  The ranks agree on the message capacity by
	// exchanging their views' visible counts (one int each, host values) over a host-side group (setCountGroup: gloo) right behind
	// the forward pass; the host picks the result up after it has queued the backward pass (keyframe_batch_exchange.cpp:
	// beginCountExchange).  Off by default until a multi-GPU node has measured it (bench.py picks the faster form in a guarded
	// trial); bit-identical results (tests/test_packed_views.py, tests/test_train_step.py).
	bool packed_exchange_ = false;
	// packed form: the message buffers (int32; persistent like sh_gathered_), the pack kernels' scratch and the count exchange
	torch::Tensor sh_packed_send_, sh_packed_gathered_, sh_pack_scratch_;
	// counts_host_: every rank's visible count, on the host (pinned only on the RCCL route, whose copies need it)
	torch::Tensor count_own_pinned_, count_own_dev_, counts_dev_, counts_host_, count_own_host_;
	// the visible counts travel host-side over this group when it is set (gloo next to the RCCL group of the gradients):
	// keyframe_batch_exchange.cpp: beginCountExchange
	c10::intrusive_ptr<c10d::ProcessGroup> count_group_;
	void setCountGroup(c10::intrusive_ptr<c10d::ProcessGroup> pg) { count_group_ = std::move(pg); }
	c10::intrusive_ptr<c10d::Work> count_work_;
	bool counts_on_device_route_ = false;
	void* counts_event_ = nullptr;     // hipEvent_t behind the counts' copy to the host
	bool packed_this_step_ = false;
	// the gathered messages' headers are read back and verified (checkPackedViews: a host wait) on the first packed steps of this
	// object -- a capacity the ranks did not agree on shows there, loudly, instead of as rows silently read as zero
	int check_packed_first_steps_ = 3;
	int packed_steps_checked_ = 0;
	// On = the backward pass writes the message itself (gsr_backward_args.packed_view; mask + prefix planned from the radii on the
	// gather stream behind the forward pass): no pack launches between the backward pass and the gather.  Off (default) = the
	// message is packed from the dense view behind the backward pass (gsr_pack_color_view, four launches on the gather stream next
	// to the SH backward kernel).  Measured on one box at one rank (profiles/r04_r): writing the message inside the backward pass
	// costs the compute stream +26 us, packing behind it costs +3 us there (it hides next to the SH kernel) -- the same step time
	// either way, so the simpler arrangement is the default.  GSR_PACK_IN_BACKWARD overrides.
	bool pack_in_backward_ = false;
	bool prepacked_this_step_ = false;
	void planPackedView(const torch::Tensor& radii);
	void beginCountExchange();         // behind the forward pass: this view's visible count to every rank
	int64_t finishCountExchange();     // -> the capacity every rank uses (max count, rounded up to 4 rows)
	void stepFeaturesFromPackedViews(torch::Tensor messages, int64_t msg_stride, int64_t n_views);
	// hipEvent_t: before / after the gather wait, before / after the reduce wait, start and end of the data-parallel step
	void* wait_events_[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
	// ---- 5. internal state of a step
	std::shared_ptr<GaussianModel> gaussians_;
	torch::Tensor background_;
	int iteration_ = 0;
	RasterWorkspace workspace_;        // of the train step's render (rasterize_points.h: RasterWorkspace; persistent_workspace_)
	RasterWorkspace view_workspace_;   // of the forward-only renders and refinePose
	std::shared_ptr<GaussianKeyframe> exposure_kf_;   // the keyframe of the last backward pass and the gradient of its exposure,
	torch::Tensor exposure_grad_;                     // until finishEnd() has taken the step
	void finishExposure();
	torch::Tensor root_grad_;   // the constant 1 handed to loss.backward()
	struct MaskEntry {
		c10::weak_intrusive_ptr<c10::TensorImpl, c10::UndefinedTensorImpl> self{c10::intrusive_ptr<c10::TensorImpl, c10::UndefinedTensorImpl>()};
		int64_t version = 0;
		bool ones = false;
	};
	std::map<const void*, MaskEntry> mask_is_ones_;   // masks seen so far: all ones? (effectiveMask)
	// the stages of renderAndBackward, in the order it runs them (train_step.cpp); effectiveMask and stepLoss serve refinePose too
	void checkStepSupported(const std::shared_ptr<GaussianKeyframe>& kf, bool use_depth, bool use_prior = false);
	void prepareExchangeBuffers(const std::shared_ptr<GaussianKeyframe>& kf);
	torch::Tensor planRegularisers(GaussianRasterizationExtensions& ext) const;
	bool planFeaturesStep(GaussianRasterizationExtensions& ext, bool rebuilds);   // -> the SH rows step lazily
	void planExchangeOverlap(GaussianRasterizationExtensions& ext);
	void planGeomStep(GaussianRasterizationExtensions& ext, bool resets);
	void planStatistics(GaussianRasterizationExtensions& ext);
	torch::Tensor effectiveMask(const torch::Tensor& mask);   // the mask, or an empty tensor for a mask of ones
	torch::Tensor stepLoss(const torch::Tensor& rendered, const torch::Tensor& depth, const torch::Tensor& exposure, const torch::Tensor& gt_image,
	                       const torch::Tensor& eff_mask, const torch::Tensor& gt_depth, bool use_depth) const;
};

// loss = (1-lambda) L1 + lambda (1-SSIM) with its gradient in two HIP kernels (gsr_l1_ssim_loss)
// is_root: the caller promises to call backward() on this very value (upstream gradient exactly 1, as TrainStep does):
// backward then hands the stored gradient on without the [3,H,W] multiply by one
torch::Tensor fusedL1SSIMLoss(torch::Tensor rendered, torch::Tensor gt, torch::Tensor mask, float lambda_dssim,
                              bool is_root = false);
