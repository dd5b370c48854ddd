// loss_utils.cpp -- see host/include/loss_utils.h: the reference's loss functions (include/loss_utils.h:24-126) with l1_loss / ssim
// on the fused HIP kernels (csrc/train_ops.hip, gsr_l1_ssim_loss) behind a torch::autograd::Function.
#include "loss_utils.h"

#include <cmath>
#include <stdexcept>
#include <string>

#include "../../../include/gsr.h"

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

// value = (1 - lambda) L1 + lambda (1 - SSIM) of (rendered * mask, gt); the gradient with respect to `rendered` is produced by
// the same pass and handed on in backward (times the upstream gradient unless the value is the root of the graph)
class FusedL1SSIMFunction : public torch::autograd::Function<FusedL1SSIMFunction> {
public:
	static torch::Tensor forward(torch::autograd::AutogradContext* ctx, torch::Tensor rendered, torch::Tensor gt,
	                             torch::Tensor mask, double lambda_dssim, bool is_root)
	{
		ctx->saved_data["is_root"] = is_root;
		auto r = rendered.contiguous(), g = gt.contiguous();
		torch::Tensor m = mask.defined() && mask.numel() ? mask.contiguous() : torch::Tensor();
		const int H = static_cast<int>(r.size(-2)), W = static_cast<int>(r.size(-1));
		auto grad = torch::empty_like(r);
		auto loss = torch::empty({1}, r.options());
		auto scratch = torch::empty({static_cast<int64_t>(gsr_loss_scratch_bytes(W, H))}, r.options().dtype(torch::kByte));
		check(gsr_l1_ssim_loss(r.data_ptr<float>(), g.data_ptr<float>(), m.defined() ? m.data_ptr<float>() : nullptr, W,
		                       H, static_cast<float>(lambda_dssim), grad.data_ptr<float>(), loss.data_ptr<float>(),
		                       reinterpret_cast<char*>(scratch.data_ptr()), stream_of(r)),
		      "gsr_l1_ssim_loss");
		ctx->save_for_backward({grad});
		return loss[0];
	}
	static torch::autograd::tensor_list backward(torch::autograd::AutogradContext* ctx, torch::autograd::tensor_list go)
	{
		auto grad = ctx->get_saved_variables()[0];
		if (ctx->saved_data["is_root"].toBool()) return {grad, torch::Tensor(), torch::Tensor(), torch::Tensor(), torch::Tensor()};
		return {grad * go[0], torch::Tensor(), torch::Tensor(), torch::Tensor(), torch::Tensor()};
	}
};

// the same value behind a [3,4] exposure map; gradients for `rendered` and `exposure`
class FusedL1SSIMExposureFunction : public torch::autograd::Function<FusedL1SSIMExposureFunction> {
public:
	static torch::Tensor forward(torch::autograd::AutogradContext* ctx, torch::Tensor rendered, torch::Tensor gt,
	                             torch::Tensor mask, double lambda_dssim, bool is_root, torch::Tensor exposure)
	{
		ctx->saved_data["is_root"] = is_root;
		if (exposure.dim() != 2 || exposure.size(0) != 3 || exposure.size(1) != 4 || exposure.scalar_type() != torch::kFloat32 ||
		    exposure.device() != rendered.device())
			throw std::runtime_error("fused_l1_ssim_exposure: exposure must be a float32 [3, 4] tensor on the device of the rendered image");
		auto r = rendered.contiguous(), g = gt.contiguous(), e = exposure.contiguous();
		torch::Tensor m = mask.defined() && mask.numel() ? mask.contiguous() : torch::Tensor();
		const int H = static_cast<int>(r.size(-2)), W = static_cast<int>(r.size(-1));
		auto grad = torch::empty_like(r);
		auto grad_e = torch::empty_like(e);
		auto loss = torch::empty({1}, r.options());
		auto scratch = torch::empty({static_cast<int64_t>(gsr_loss_exposure_scratch_bytes(W, H))}, r.options().dtype(torch::kByte));
		check(gsr_l1_ssim_loss_exposure(r.data_ptr<float>(), g.data_ptr<float>(), m.defined() ? m.data_ptr<float>() : nullptr, W, H,
		                                static_cast<float>(lambda_dssim), e.data_ptr<float>(), grad.data_ptr<float>(),
		                                grad_e.data_ptr<float>(), loss.data_ptr<float>(), reinterpret_cast<char*>(scratch.data_ptr()),
		                                stream_of(r)),
		      "gsr_l1_ssim_loss_exposure");
		ctx->save_for_backward({grad, grad_e});
		return loss[0];
	}
	static torch::autograd::tensor_list backward(torch::autograd::AutogradContext* ctx, torch::autograd::tensor_list go)
	{
		auto saved = ctx->get_saved_variables();
		const torch::Tensor none;
		if (ctx->saved_data["is_root"].toBool()) return {saved[0], none, none, none, none, saved[1]};
		return {saved[0] * go[0], none, none, none, none, saved[1] * go[0]};
	}
};

class DepthL1Function : public torch::autograd::Function<DepthL1Function> {
public:
	static torch::Tensor forward(torch::autograd::AutogradContext* ctx, torch::Tensor depth, torch::Tensor gt_depth, double weight,
	                             double min_depth, double max_depth)
	{
		auto d = depth.contiguous(), g = gt_depth.contiguous();
		if (d.dim() != 2 || g.sizes() != d.sizes() || d.scalar_type() != torch::kFloat32 || g.scalar_type() != torch::kFloat32)
			throw std::runtime_error("depth_l1: depth and gt_depth must be float32 [H, W] tensors of the same shape");
		const int H = static_cast<int>(d.size(0)), W = static_cast<int>(d.size(1));
		auto grad = torch::empty_like(d);
		auto loss = torch::empty({1}, d.options());
		auto scratch = torch::empty({static_cast<int64_t>(gsr_depth_loss_scratch_bytes(W, H))}, d.options().dtype(torch::kByte));
		check(gsr_depth_l1_loss(d.data_ptr<float>(), g.data_ptr<float>(), W, H, static_cast<float>(min_depth),
		                        static_cast<float>(max_depth), static_cast<float>(weight), grad.data_ptr<float>(),
		                        loss.data_ptr<float>(), reinterpret_cast<char*>(scratch.data_ptr()), stream_of(d)),
		      "gsr_depth_l1_loss");
		ctx->save_for_backward({grad});
		return loss[0];
	}
	static torch::autograd::tensor_list backward(torch::autograd::AutogradContext* ctx, torch::autograd::tensor_list go)
	{
		auto grad = ctx->get_saved_variables()[0];
		return {grad * go[0], torch::Tensor(), torch::Tensor(), torch::Tensor(), torch::Tensor()};
	}
};

// ---- the monocular depth prior (include/gsr.h: gsr_depth_prior_loss).  An empty tensor stands for "not given" (alpha, valid).
struct DepthPriorMaps {
	torch::Tensor d, a, q, v;
};
DepthPriorMaps depth_prior_maps(const torch::Tensor& depth, const torch::Tensor& alpha, const torch::Tensor& prior, const torch::Tensor& valid)
{
	DepthPriorMaps m;
	m.d = depth.contiguous();
	m.q = prior.contiguous();
	if (m.d.dim() != 2 || m.q.sizes() != m.d.sizes() || m.d.scalar_type() != torch::kFloat32 || m.q.scalar_type() != torch::kFloat32 ||
	    m.q.device() != m.d.device())
		throw std::runtime_error("depth_prior: depth and prior must be float32 [H, W] tensors of the same shape on one device");
	if (alpha.defined() && alpha.numel()) {
		m.a = alpha.contiguous();
		if (m.a.sizes() != m.d.sizes() || m.a.scalar_type() != torch::kFloat32 || m.a.device() != m.d.device())
			throw std::runtime_error("depth_prior: alpha must be a float32 [H, W] tensor like depth");
	}
	if (valid.defined() && valid.numel()) {
		m.v = valid.contiguous();
		if (m.v.scalar_type() == torch::kBool) m.v = m.v.view(torch::kByte);
		if (m.v.sizes() != m.d.sizes() || m.v.scalar_type() != torch::kByte || m.v.device() != m.d.device())
			throw std::runtime_error("depth_prior: valid must be a uint8 or bool [H, W] tensor on the device of depth");
	}
	return m;
}
int depth_prior_flags(bool inverse, bool pearson) { return (inverse ? GSR_DEPTH_PRIOR_INVERSE : 0) | (pearson ? GSR_DEPTH_PRIOR_PEARSON : 0); }

// {loss [1], grad_depth, grad_alpha, fit [4]}; with_grads false: the fit alone (the others undefined)
std::vector<torch::Tensor> depth_prior_call(const DepthPriorMaps& m, float weight, int flags, float alpha_min, bool with_grads)
{
	const int H = static_cast<int>(m.d.size(0)), W = static_cast<int>(m.d.size(1));
	torch::Tensor loss, grad_d, grad_a;
	auto fit = torch::empty({4}, m.d.options());
	if (with_grads) {
		loss = torch::empty({1}, m.d.options());
		grad_d = torch::empty_like(m.d);
		if (m.a.defined()) grad_a = torch::empty_like(m.d);
	}
	auto scratch = torch::empty({static_cast<int64_t>(gsr_depth_prior_scratch_bytes(W, H))}, m.d.options().dtype(torch::kByte));
	gsr_depth_prior_args a{};
	a.width = W; a.height = H;
	a.depth = m.d.data_ptr<float>();
	a.alpha = m.a.defined() ? m.a.data_ptr<float>() : nullptr;
	a.prior = m.q.data_ptr<float>();
	a.valid = m.v.defined() ? m.v.data_ptr<uint8_t>() : nullptr;
	a.flags = flags; a.alpha_min = alpha_min; a.weight = weight;
	a.grad_depth = grad_d.defined() ? grad_d.data_ptr<float>() : nullptr;
	a.grad_alpha = grad_a.defined() ? grad_a.data_ptr<float>() : nullptr;
	a.loss = loss.defined() ? loss.data_ptr<float>() : nullptr;
	a.fit = fit.data_ptr<float>();
	check(gsr_depth_prior_loss(&a, reinterpret_cast<char*>(scratch.data_ptr()), stream_of(m.d)), "gsr_depth_prior_loss");
	return {loss, grad_d, grad_a, fit};
}

class DepthPriorFunction : public torch::autograd::Function<DepthPriorFunction> {
public:
	static torch::autograd::tensor_list forward(torch::autograd::AutogradContext* ctx, torch::Tensor depth, torch::Tensor alpha,
	                                            torch::Tensor prior, double weight, int64_t flags, double alpha_min, torch::Tensor valid)
	{
		const auto m = depth_prior_maps(depth, alpha, prior, valid);
		auto r = depth_prior_call(m, static_cast<float>(weight), static_cast<int>(flags), static_cast<float>(alpha_min), true);
		ctx->saved_data["has_alpha"] = m.a.defined();
		if (m.a.defined()) ctx->save_for_backward({r[1], r[2]});
		else ctx->save_for_backward({r[1]});
		ctx->mark_non_differentiable({r[3]});
		return {r[0][0], r[3]};
	}
	static torch::autograd::tensor_list backward(torch::autograd::AutogradContext* ctx, torch::autograd::tensor_list go)
	{
		auto saved = ctx->get_saved_variables();
		const torch::Tensor none;
		return {saved[0] * go[0], ctx->saved_data["has_alpha"].toBool() ? saved[1] * go[0] : none, none, none, none, none, none};
	}
};

// what the kernels cover: one float32 [3,H,W] (or [1,3,H,W]) image pair on one device, the target without a gradient
bool fused_applies(const torch::Tensor& a, const torch::Tensor& b)
{
	if (!a.defined() || !b.defined() || a.sizes() != b.sizes() || a.scalar_type() != torch::kFloat32 || b.scalar_type() != torch::kFloat32 ||
	    a.device() != b.device() || b.requires_grad())
		return false;
	if (a.dim() == 4 && a.size(0) != 1) return false;
	if (a.dim() != 3 && a.dim() != 4) return false;
	if (a.size(-3) != 3) return false;
#ifndef GSR_HOST_NO_HIP
	return a.is_cuda();
#else
	return !a.is_cuda();   // the emulator build of the test-suite runs the kernels on host tensors
#endif
}
}  // namespace

namespace loss_utils
{

torch::Tensor fused_l1_ssim(torch::Tensor rendered, torch::Tensor gt, torch::Tensor mask, float lambda_dssim, bool is_root)
{
	if (!mask.defined()) mask = torch::empty({0}, gt.options());   // (autograd::Function::apply needs every tensor argument defined)
	return FusedL1SSIMFunction::apply(rendered, gt, mask, static_cast<double>(lambda_dssim), is_root);
}

torch::Tensor fused_l1_ssim_exposure(torch::Tensor rendered, torch::Tensor gt, torch::Tensor mask, float lambda_dssim,
                                     torch::Tensor exposure, bool is_root)
{
	if (!mask.defined()) mask = torch::empty({0}, gt.options());
	return FusedL1SSIMExposureFunction::apply(rendered, gt, mask, static_cast<double>(lambda_dssim), is_root, exposure);
}

torch::Tensor apply_exposure(torch::Tensor image, torch::Tensor exposure)
{
	if (image.dim() != 3 || image.size(0) != 3 || exposure.dim() != 2 || exposure.size(0) != 3 || exposure.size(1) != 4 ||
	    image.scalar_type() != torch::kFloat32 || exposure.scalar_type() != torch::kFloat32 || image.device() != exposure.device())
		throw std::runtime_error("apply_exposure: a float32 [3, H, W] image and a float32 [3, 4] exposure on one device");
	auto r = image.detach().contiguous(), e = exposure.detach().contiguous();
	auto out = torch::empty_like(r);
	check(gsr_apply_exposure(r.data_ptr<float>(), e.data_ptr<float>(), static_cast<int>(r.size(2)), static_cast<int>(r.size(1)),
	                         out.data_ptr<float>(), stream_of(r)),
	      "gsr_apply_exposure");
	return out;
}

torch::Tensor depth_l1(torch::Tensor depth, torch::Tensor gt_depth, float weight, float min_depth, float max_depth)
{
	return DepthL1Function::apply(depth, gt_depth, static_cast<double>(weight), static_cast<double>(min_depth),
	                              static_cast<double>(max_depth));
}

torch::Tensor depth_prior(torch::Tensor depth, torch::Tensor alpha, torch::Tensor prior, float weight, bool inverse, bool pearson,
                          float alpha_min, torch::Tensor valid, torch::Tensor* fit)
{
	if (!alpha.defined()) alpha = torch::empty({0}, depth.options());   // (autograd::Function::apply needs every tensor argument defined)
	if (!valid.defined()) valid = torch::empty({0}, depth.options().dtype(torch::kByte));
	auto out = DepthPriorFunction::apply(depth, alpha, prior, static_cast<double>(weight),
	                                     static_cast<int64_t>(depth_prior_flags(inverse, pearson)), static_cast<double>(alpha_min), valid);
	if (fit) *fit = out[1];
	return out[0];
}

torch::Tensor depth_prior_fit(torch::Tensor depth, torch::Tensor alpha, torch::Tensor prior, bool inverse, float alpha_min,
                              torch::Tensor valid)
{
	const auto m = depth_prior_maps(depth.detach(), alpha.defined() ? alpha.detach() : alpha, prior.detach(), valid);
	return depth_prior_call(m, 0.0f, depth_prior_flags(inverse, false), alpha_min, false)[3];
}

torch::Tensor depth_prior_apply(torch::Tensor prior, torch::Tensor fit, bool inverse, bool in_place)
{
	if (prior.dim() != 2 || prior.scalar_type() != torch::kFloat32 || fit.numel() != 4 || fit.scalar_type() != torch::kFloat32 ||
	    prior.device() != fit.device())
		throw std::runtime_error("depth_prior_apply: a float32 [H, W] prior and a float32 [4] fit on one device");
	if (in_place && !prior.is_contiguous()) throw std::runtime_error("depth_prior_apply: in place needs a contiguous prior");
	auto q = prior.detach().contiguous(), f = fit.detach().contiguous();
	auto out = in_place ? q : torch::empty_like(q);
	check(gsr_depth_prior_apply(q.data_ptr<float>(), f.data_ptr<float>(), depth_prior_flags(inverse, false), static_cast<int>(q.size(1)),
	                            static_cast<int>(q.size(0)), out.data_ptr<float>(), stream_of(q)),
	      "gsr_depth_prior_apply");
	return out;
}

torch::Tensor l1_loss(torch::Tensor &network_output, torch::Tensor &gt)
{
	if (fused_applies(network_output, gt)) return FusedL1SSIMFunction::apply(network_output, gt, torch::empty({0}, gt.options()), 0.0, false);   // (an empty mask = none)
	return torch::abs(network_output - gt).mean();
}

// ---- the calls the kernels do not cover (another window, no size average, a batch, a target with a gradient, host tensors).
// Same names, signatures and values as the reference's header (the drop-in contract: include/loss_utils.h:33-108), computed this
// library's way: the SSIM window is the outer product of one normalised 1-D Gaussian, so every local statistic is TWO 1-D
// convolutions (11 + 11 taps per pixel instead of 121), and the five statistics of a pair of images -- means, second moments, the
// mixed moment -- ride in ONE grouped convolution pair over a 5C-channel stack.

torch::Tensor psnr(torch::Tensor &img1, torch::Tensor &img2)
{
	// 10 log10(1 / mse), mse over the whole tensor
	return -10.0f * torch::log10(torch::mse_loss(img1, img2));
}

torch::Tensor psnr_gaussian_splatting(torch::Tensor &img1, torch::Tensor &img2)
{
	// the Inria evaluation's form: per image of the batch 20 log10(1 / rmse), then the mean over the batch
	const auto per_image = (img1 - img2).square().flatten(1).mean(1, /*keepdim=*/true);
	return (-10.0f * torch::log10(per_image)).mean();
}

torch::Tensor gaussian(int window_size, float sigma, torch::DeviceType device_type)
{
	// taps exp(-(x - window_size / 2)^2 / (2 sigma^2)), x = 0 .. window_size - 1 (integer centre), normalised to sum 1
	const auto x = torch::arange(window_size, torch::TensorOptions().dtype(torch::kFloat32).device(device_type)) - static_cast<float>(window_size / 2);
	const auto w = torch::exp(x.square() * (-1.0f / (2.0f * sigma * sigma)));
	return w / w.sum();
}

torch::autograd::Variable create_window(int window_size, int64_t channel, torch::DeviceType device_type)
{
	// [channel, 1, k, k]: the same 2-D window for every channel (a grouped convolution's weight)
	const auto taps = gaussian(window_size, 1.5f, device_type);
	return torch::outer(taps, taps).to(torch::kFloat).expand({channel, 1, window_size, window_size}).contiguous();
}

namespace {
// local window sums of every channel of x [N, C, H, W] (zero padding, as conv2d with padding k / 2): separable when the window is
// the outer product of its marginals (any window create_window makes), the plain grouped 2-D convolution otherwise
torch::Tensor window_filter(const torch::Tensor& x, const torch::Tensor& window2d, int window_size)
{
	namespace F = torch::nn::functional;
	const int64_t C = x.size(1);
	const int pad = window_size / 2;
	const auto k2 = window2d.select(0, 0).select(0, 0);                     // [k, k] (the same for every channel)
	const auto col = k2.sum(1), row = k2.sum(0);                            // marginals: vertical and horizontal taps
	const auto total = k2.sum();
	const bool separable = torch::allclose(torch::outer(col, row), k2 * total, 1e-6, 1e-9);
	if (!separable)
		return F::conv2d(x, k2.reshape({1, 1, window_size, window_size}).expand({C, 1, window_size, window_size}), F::Conv2dFuncOptions().padding(pad).groups(C));
	const auto horizontal = (row / total).reshape({1, 1, 1, window_size}).expand({C, 1, 1, window_size});
	const auto vertical = col.reshape({1, 1, window_size, 1}).expand({C, 1, window_size, 1});
	const auto h = F::conv2d(x, horizontal, F::Conv2dFuncOptions().padding({0, pad}).groups(C));
	return F::conv2d(h, vertical, F::Conv2dFuncOptions().padding({pad, 0}).groups(C));
}
}  // namespace

torch::Tensor _ssim(torch::Tensor &img1, torch::Tensor &img2, torch::autograd::Variable &window, int window_size, int64_t channel,
                    bool size_average)
{
	const bool batched = img1.dim() == 4;
	const auto a = batched ? img1 : img1.unsqueeze(0), b = batched ? img2 : img2.unsqueeze(0);
	// one filter pass over [a | b | a a | b b | a b]
	const auto stats = window_filter(torch::cat({a, b, a * a, b * b, a * b}, 1), window, window_size).split(channel, 1);
	const auto& mean_a = stats[0];
	const auto& mean_b = stats[1];
	const auto cross = mean_a * mean_b, energy = mean_a.square() + mean_b.square();
	const auto spread = stats[2] + stats[3] - energy;      // var(a) + var(b)
	const auto covariance = stats[4] - cross;
	const double c1 = 1e-4, c2 = 9e-4;                      // (0.01 L)^2, (0.03 L)^2 with a dynamic range L of 1
	auto map = ((2 * cross + c1) * (2 * covariance + c2)) / ((energy + c1) * (spread + c2));
	if (!batched) map = map.squeeze(0);
	if (size_average) return map.mean();
	return map.mean(1).mean(1).mean(1);   // (the reference's reduction order: dims 1, 1, 1 of what is left)
}

torch::Tensor ssim(torch::Tensor &img1, torch::Tensor &img2, torch::DeviceType device_type, int window_size, bool size_average)
{
	// the train step's call (11 x 11 window, sigma 1.5, mean over the map): 1 - [(1 - lambda) L1 + lambda (1 - SSIM)] at lambda = 1
	if (window_size == 11 && size_average && fused_applies(img1, img2))
		return 1.0 - FusedL1SSIMFunction::apply(img1, img2, torch::empty({0}, img2.options()), 1.0, false);
	const int64_t channels = img1.size(-3);
	torch::autograd::Variable window = create_window(window_size, channels, img1.device().type()).to(img1.scalar_type());
	return _ssim(img1, img2, window, window_size, channels, size_average);
}

}
