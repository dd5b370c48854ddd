// train_ops.hip -- the two largest non-rasterizer costs of the measured train step
// (GaussianMapper::trainForOneIteration, src/gaussian_mapper.cpp:692-699,769-772), fused:
//
//  * masked L1 + SSIM loss with its gradient w.r.t. the rendered image.  The reference builds it
//    from 5 grouped 11x11 conv2d + ~20 elementwise ATen ops and lets autograd run 10 more convs
//    backward (include/loss_utils.h:28-124); on MI355X MIOpen spends ~12 ms per step on those
//    depthwise convolutions at 1080p.  Here: two LDS-tiled passes with a separable 11-tap window
//    (window2D = g (x) g, loss_utils.h:49-74), ~0.4 GB of HBM traffic in total.
//  * Adam (torch::optim::Adam semantics, eps 1e-15, src/gaussian_model.cpp:477-510) as one
//    streaming pass per tensor: 7 x 4 bytes per parameter instead of ~10 elementwise launches
//    per parameter group.
#include "kernels.h"
#include "state.h"
#include "wave64.h"
#include <type_traits>
#ifdef GSR_EMU
#include <atomic>
#endif

namespace gsr {

constexpr int LT = 32;                  // output tile width
constexpr int LTY = 32;                 // output tile height (8 row groups per column: LTY / 8 outputs per thread)
constexpr int LH = 5;                   // window half width (11 taps)
constexpr int LRY = LTY + 2 * LH;       // 42 input rows with halo
// Staged input tile: columns x0-8 .. x0+39 (the halo x0-5 .. x0+36 padded to 16-byte vectors: with W % 4 == 0 every vector
// lies inside or outside the image as a whole and is moved by one global_load_dwordx4 + one ds_write_b128)
constexpr int SX0 = 8;
constexpr int SW4 = 12;                 // float4 per staged row
constexpr int SP4 = 13;                 // staged row pitch in float4 (52 floats)
constexpr int HP4 = 9;                  // pitch of a horizontally filtered row in float4 (36 floats for 32 columns)
constexpr int HP = 4 * HP4;

struct LossParams {
	const float* rendered;  // [3,H,W]
	const float* gt;        // [3,H,W]
	const float* mask;      // [3,H,W] or null
	int W, H;
	int vec;                // W % 4 == 0 and every plane 16-byte aligned: stage with 16-byte vectors
	float lambda_dssim;
	float g[11];            // normalised 1-D window
	float* dmaps;           // [3][3,H,W]: dL/dmu1, dL/de11, dL/de12 (already scaled by -lambda/N)
	float* partial;         // [2][nblocks]: L1 sums, SSIM sums
	float* grad;            // [3,H,W] dL/d rendered
	float* loss;            // [1]
	int nblocks;
	int gx, gy;             // tile grid per channel: nblocks = 3 gx gy
};

// Workgroup -> (channel, tile) with the same XCD banding as the blend kernels (blend.h: tile_assignment): workgroup b runs on
// XCD b % 8, and every XCD gets a contiguous run of the row-major tile order, so that the 5-pixel halo a tile shares with its
// neighbours (1.72x the tile's own pixels at 32 x 32) is found in THAT XCD's L2 instead of being fetched once per XCD.  The
// launch is 1-D, padded to a multiple of 8; returns false for a padding workgroup.
__device__ __forceinline__ bool loss_tile(const LossParams& p, int& t, int& ch, int& x0, int& y0)
{
	const int per = (p.nblocks + 7) >> 3;
	const int b = (int)blockIdx.x, in_xcd = b >> 3;
	t = (b & 7) * per + in_xcd;
	if (in_xcd >= per || t >= p.nblocks) return false;
	const int per_ch = p.gx * p.gy;
	ch = t / per_ch;
	const int r = t - ch * per_ch, ty = r / p.gx;
	x0 = (r - ty * p.gx) * LT;
	y0 = ty * LTY;
	return true;
}
static inline int loss_grid(int nblocks) { return ((nblocks + 7) >> 3) * 8; }

__device__ __forceinline__ float block_sum_256(float v, float* s4)
{
	// wave sum by shuffles-free DPP is overkill here; LDS tree over 4 wave partials
	float w = v;
#ifdef GSR_EMU
	{
		uint32_t b; memcpy(&b, &w, 4);
		const uint64_t* s = ::hipemu::wave_exchange(b);
		float acc = 0.f;
		for (int i = 0; i < 64; i++) { uint32_t u = (uint32_t)s[i]; float f; memcpy(&f, &u, 4); acc += f; }
		::hipemu::wave_sync();
		w = acc;
	}
#else
	w = wave_sum_f32_lane63(w);
	w = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, w), 63));
#endif
	__syncthreads();
	if (lane_id() == 0) s4[wave_id()] = w;
	__syncthreads();
	return s4[0] + s4[1] + s4[2] + s4[3];
}

// Both passes are separable 11-tap convolutions over a 32x32 output tile with a 5-pixel halo.  Every thread produces
// FOUR consecutive outputs of a row (horizontal pass: 42 rows x 8 groups = 336 units over 256 threads) or of a column
// (vertical pass) from 14 inputs held in registers.  Both kernels are bound by VALU + LDS issue with little overlap between
// the two (few resident waves, three barrier-separated phases), so the LDS side is kept short: rows are staged and read back
// as 16-byte vectors (a unit's 14-float window = the aligned 20 floats around it), the horizontally filtered rows are written
// as 16-byte vectors INTO THE MEMORY OF THE STAGED TILE (behind a barrier: every unit has read its inputs by then;
// 30 KB instead of 42 KB per workgroup: 5 resident workgroups per CU instead of 3), and products / reciprocals that do not
// depend on the tap or output are hoisted.
constexpr int LG = 4;              // outputs per thread in the horizontal pass
constexpr int LGV = LTY / 8;       // outputs per thread in the vertical pass (256 threads = 32 columns x 8 row groups)
constexpr int LWV = LGV + 2 * LH;
constexpr int H_UNITS = LRY * (LT / LG);   // 336
static_assert(H_UNITS > 256 && H_UNITS <= 512, "two horizontal units per thread at most");

// A 16-byte load of the vector staging path.  `vec` in gsr_l1_ssim_loss promises that every one of them is 16-byte aligned; a host
// CPU and the device both take a load that is not, so no result would show a broken promise: the emulator build counts them
// (gsr_emu_loss_misaligned_loads, tests/loss_cases.py).
#ifdef GSR_EMU
static std::atomic<long long> g_loss_misaligned_loads{0};
static inline float4 loss_load_f4_counted(const float* p)
{
	if (reinterpret_cast<uintptr_t>(p) & 15) g_loss_misaligned_loads++;
	return *reinterpret_cast<const float4*>(p);
}
#define LOSS_LOAD_F4(p) loss_load_f4_counted(p)
#else
#define LOSS_LOAD_F4(p) (*reinterpret_cast<const float4*>(p))
#endif

// Stage NA planes (row pitch W) of the tile at (x0, y0) into s[a][LRY][SP4]; plane 0 is multiplied by mask if given.
// EXPO: the same code as an instantiation of its own for loss_bwd_kernel<true> -- with ONE instantiation inlined into both backward
// kernels the compiler schedules the plain kernel's staging differently from the code without the exposure feature.
template <int NA, bool EXPO = false>
__device__ __forceinline__ void loss_stage_tile(const float* const (&src)[NA], const float* mask, int W, int H, int vec, int x0,
                                                int y0, float4* s, int tid)
{
	if (vec) {
		for (int i = tid; i < LRY * SW4; i += 256) {
			const int r = i / SW4, q = i - r * SW4;
			const int gx = x0 - SX0 + 4 * q, gy = y0 - LH + r;
			const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;
			const size_t o = in ? (size_t)gy * W + gx : 0;
#pragma unroll
			for (int a = 0; a < NA; a++) {
				float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
				if (in) {
					v = LOSS_LOAD_F4(src[a] + o);
					if (a == 0 && mask) {
						const float4 m = LOSS_LOAD_F4(mask + o);
						v.x *= m.x; v.y *= m.y; v.z *= m.z; v.w *= m.w;
					}
				}
				s[(a * LRY + r) * SP4 + q] = v;
			}
		}
	} else {
		float* sf = reinterpret_cast<float*>(s);
		for (int i = tid; i < LRY * SW4 * 4; i += 256) {
			const int r = i / (SW4 * 4), c = i - r * (SW4 * 4);
			const int gx = x0 - SX0 + c, gy = y0 - LH + r;
			const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;
			const size_t o = in ? (size_t)gy * W + gx : 0;
#pragma unroll
			for (int a = 0; a < NA; a++) {
				float v = 0.f;
				if (in) {
					v = src[a][o];
					if (a == 0 && mask) v *= mask[o];
				}
				sf[(a * LRY + r) * (SP4 * 4) + c] = v;
			}
		}
	}
}

// ---- per-keyframe exposure (gsr_l1_ssim_loss_exposure): x_c = (r_0 E[0][c] + r_1 E[1][c] + r_2 E[2][c] + E[c][3]) m_c, E [3,4]
// row-major on the device.  Instantiations of their own (loss_fwd_kernel<true>, loss_bwd_kernel<true>; their parameters: LossParams
// with three pointers behind it), so that the plain kernels are the same code with the same arguments as without the feature.
struct LossExposureParams : LossParams {
	const float* E;          // [12]
	float* xpartial;         // [4][nblocks]: per workgroup (channel c) sum r_0 G_c, sum r_1 G_c, sum r_2 G_c, sum G_c
	float* grad_exposure;    // [12]
};
template <bool EXPO> using LossKernelParams = std::conditional_t<EXPO, LossExposureParams, LossParams>;

// One element of the map, in the order of the contract and without contraction: pass 1 (both staging paths), pass 2 and
// gsr_apply_exposure produce the same bits from the same inputs, whatever surrounds the call (see adam_update).
__device__ __forceinline__ float exposure_map(float r0, float r1, float r2, float e0, float e1, float e2, float e3)
{
#pragma clang fp contract(off)
	return r0 * e0 + r1 * e1 + r2 * e2 + e3;
}

// loss_stage_tile<2> for the exposure kernels: plane 0 is the mapped (and masked) rendered image of channel ch -- three rendered
// loads per element, ONE staged plane (a fourth staged plane would not fit the 30 KB region) -- plane 1 is gt.
__device__ __forceinline__ void loss_stage_tile_exposure(const float* rendered, const float* gt, const float* mask, size_t plane,
                                                         const float (&e)[4], int W, int H, int vec, int x0, int y0, float4* s, int tid)
{
	const float* r0 = rendered;
	const float* r1 = rendered + plane;
	const float* r2 = rendered + 2 * plane;
	if (vec) {
		for (int i = tid; i < LRY * SW4; i += 256) {
			const int r = i / SW4, q = i - r * SW4;
			const int gx = x0 - SX0 + 4 * q, gy = y0 - LH + r;
			const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;
			const size_t o = in ? (size_t)gy * W + gx : 0;
			float4 v = make_float4(0.f, 0.f, 0.f, 0.f), y = make_float4(0.f, 0.f, 0.f, 0.f);
			if (in) {
				const float4 a = LOSS_LOAD_F4(r0 + o), b = LOSS_LOAD_F4(r1 + o), c = LOSS_LOAD_F4(r2 + o);
				y = LOSS_LOAD_F4(gt + o);
				v.x = exposure_map(a.x, b.x, c.x, e[0], e[1], e[2], e[3]);
				v.y = exposure_map(a.y, b.y, c.y, e[0], e[1], e[2], e[3]);
				v.z = exposure_map(a.z, b.z, c.z, e[0], e[1], e[2], e[3]);
				v.w = exposure_map(a.w, b.w, c.w, e[0], e[1], e[2], e[3]);
				if (mask) {
					const float4 m = LOSS_LOAD_F4(mask + o);
					v.x *= m.x; v.y *= m.y; v.z *= m.z; v.w *= m.w;
				}
			}
			s[r * SP4 + q] = v;
			s[(LRY + r) * SP4 + q] = y;
		}
	} else {
		float* sf = reinterpret_cast<float*>(s);
		for (int i = tid; i < LRY * SW4 * 4; i += 256) {
			const int r = i / (SW4 * 4), c = i - r * (SW4 * 4);
			const int gx = x0 - SX0 + c, gy = y0 - LH + r;
			const bool in = gx >= 0 && gx < W && gy >= 0 && gy < H;
			const size_t o = in ? (size_t)gy * W + gx : 0;
			float v = 0.f, y = 0.f;
			if (in) {
				v = exposure_map(r0[o], r1[o], r2[o], e[0], e[1], e[2], e[3]);
				if (mask) v *= mask[o];
				y = gt[o];
			}
			sf[r * (SP4 * 4) + c] = v;
			sf[(LRY + r) * (SP4 * 4) + c] = y;
		}
	}
}

// the aligned 20 floats around the 14-float window of horizontal unit (r, g): window element t sits at [3 + t]
__device__ __forceinline__ void loss_load_window(const float4* plane, int r, int g, float (&w)[20])
{
#pragma unroll
	for (int k = 0; k < 5; k++) {
		const float4 v = plane[r * SP4 + g + k];
		w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
	}
}

// Pass 1: window statistics -> SSIM map value + the three derivative maps, and L1 / SSIM partial sums.
// EXPO: the staging applies the exposure map as it loads (loss_stage_tile_exposure); everything behind it is the same code.
template <bool EXPO>
__global__ void __launch_bounds__(256)
loss_fwd_kernel(const LossKernelParams<EXPO> p)
{
	// staged x, y: 2 x 42 x 13 float4; then the five filtered maps: 5 x 42 x 9 float4 in the same memory
	__shared__ float4 s_mem[5 * LRY * HP4];
	static_assert(5 * LRY * HP4 >= 2 * LRY * SP4, "the filtered maps cover the staged tile");
	__shared__ float s_red[4];
	int t, ch, x0, y0;
	if (!loss_tile(p, t, ch, x0, y0)) return;   // (workgroup-uniform)
	const size_t plane = (size_t)p.W * p.H;
	const int tid = (int)threadIdx.x;
	if constexpr (EXPO) {
		const float e[4] = {p.E[ch], p.E[4 + ch], p.E[8 + ch], p.E[4 * ch + 3]};
		loss_stage_tile_exposure(p.rendered, p.gt + ch * plane, p.mask ? p.mask + ch * plane : nullptr, plane, e, p.W, p.H, p.vec,
		                         x0, y0, s_mem, tid);
	} else {
		const float* const src[2] = {p.rendered + ch * plane, p.gt + ch * plane};
		loss_stage_tile<2>(src, p.mask ? p.mask + ch * plane : nullptr, p.W, p.H, p.vec, x0, y0, s_mem, tid);
	}
	__syncthreads();
	float l1_sum = 0.f, ssim_sum = 0.f;
	// horizontal pass: unit u = (row r, group g of LG columns)
	auto h_unit = [&](const float (&xw)[20], const float (&yw)[20], int r, int g, float4 (&out)[5]) {
		float xx[14], yy[14], xy[14];
#pragma unroll
		for (int t = 0; t < 14; t++) {
			const float x = xw[3 + t], y = yw[3 + t];
			xx[t] = x * x; yy[t] = y * y; xy[t] = x * y;
		}
		float acc[5][LG];
#pragma unroll
		for (int o = 0; o < LG; o++) {
			float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
			for (int t = 0; t < 11; t++) {
				const float gw = p.g[t];
				a0 += gw * xw[3 + o + t];
				a1 += gw * yw[3 + o + t];
				a2 += gw * xx[o + t];
				a3 += gw * yy[o + t];
				a4 += gw * xy[o + t];
			}
			acc[0][o] = a0; acc[1][o] = a1; acc[2][o] = a2; acc[3][o] = a3; acc[4][o] = a4;
		}
#pragma unroll
		for (int k = 0; k < 5; k++) out[k] = make_float4(acc[k][0], acc[k][1], acc[k][2], acc[k][3]);
		// L1 term of the four output pixels of this unit (interior rows only): output column c is staged column c + 8
		const int gy = y0 + r - LH;
		if (r >= LH && r < LH + LTY && gy < p.H) {
#pragma unroll
			for (int o = 0; o < LG; o++)
				if (x0 + 4 * g + o < p.W) l1_sum += fabsf(xw[SX0 + o] - yw[SX0 + o]);
		}
	};
	{
		const float4* s_x = s_mem;
		const float4* s_y = s_mem + LRY * SP4;
		float xw[20], yw[20];
		float4 out1[5], out2[5];
		const int r1 = tid >> 3, g1 = tid & 7;
		loss_load_window(s_x, r1, g1, xw);
		loss_load_window(s_y, r1, g1, yw);
		h_unit(xw, yw, r1, g1, out1);
		const bool two = tid + 256 < H_UNITS;
		const int r2 = (tid + 256) >> 3;
		if (two) {
			loss_load_window(s_x, r2, g1, xw);
			loss_load_window(s_y, r2, g1, yw);
		}
		// every unit has read its inputs: the filtered maps may overwrite the staged tile.  (The second unit's inputs cross the
		// barrier, not its results: 126 instead of 138 VGPRs, i.e. 4 instead of 3 waves per SIMD.)
		__syncthreads();
#pragma unroll
		for (int k = 0; k < 5; k++) s_mem[(k * LRY + r1) * HP4 + g1] = out1[k];
		if (two) {
			h_unit(xw, yw, r2, g1, out2);
#pragma unroll
			for (int k = 0; k < 5; k++) s_mem[(k * LRY + r2) * HP4 + g1] = out2[k];
		}
	}
	__syncthreads();
	const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
	const float inv_n = 1.0f / (3.0f * (float)plane);
	{
		// vertical pass: thread = (column c, group of LGV rows)
		const float* s_h = reinterpret_cast<const float*>(s_mem);
		const int c = tid & (LT - 1), r0 = (tid >> 5) * LGV;
		float st[5][LGV];
#pragma unroll
		for (int k = 0; k < 5; k++) {
			float col[LWV];
#pragma unroll
			for (int t = 0; t < LWV; t++) col[t] = s_h[(k * LRY + r0 + t) * HP + c];
#pragma unroll
			for (int o = 0; o < LGV; o++) {
				float a = 0.f;
#pragma unroll
				for (int t = 0; t < 11; t++) a += p.g[t] * col[o + t];
				st[k][o] = a;
			}
		}
		const int gx = x0 + c;
		const float gS = -p.lambda_dssim * inv_n;   // dL/dS = -lambda / N ; chain to (mu1, e11, e12)
#pragma unroll
		for (int o = 0; o < LGV; o++) {
			const int gy = y0 + r0 + o;
			if (gx < p.W && gy < p.H) {
				const float mu1 = st[0][o], mu2 = st[1][o], e11 = st[2][o], e22 = st[3][o], e12 = st[4][o];
				const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
				const float sig1 = e11 - mu1_sq, sig2 = e22 - mu2_sq, sig12 = e12 - mu12;
				const float A = 2.f * mu12 + C1, B = 2.f * sig12 + C2, Cc = mu1_sq + mu2_sq + C1, D = sig1 + sig2 + C2;
				const float invCD = 1.0f / (Cc * D);
				const float invC = D * invCD, invD = Cc * invCD;   // one division per pixel
				const float S = A * B * invCD;
				ssim_sum += S;
				const float dmu1 = 2.f * mu2 * (B - A) * invCD - 2.f * mu1 * S * (invC - invD);
				const size_t oo = (size_t)gy * p.W + gx;
				p.dmaps[(0 * 3 + ch) * plane + oo] = gS * dmu1;
				p.dmaps[(1 * 3 + ch) * plane + oo] = gS * (-S * invD);
				p.dmaps[(2 * 3 + ch) * plane + oo] = gS * (2.f * A * invCD);
			}
		}
	}
	const float t1 = block_sum_256(l1_sum, s_red);
	const float t2 = block_sum_256(ssim_sum, s_red);
	if (tid == 0) {
		p.partial[t] = t1;   // (indexed by tile: the final sum's order does not depend on the workgroup mapping)
		p.partial[p.nblocks + t] = t2;
	}
}

// The loss value from the per-workgroup partial sums of pass 1, in a fixed order.  Run by ONE workgroup of pass 2 (pass 1 is
// complete by then): a launch of its own cost 9 us for 3 us of work.
__device__ __forceinline__ void loss_finalize(const LossParams& p, float* s_red)
{
	float a = 0.f, b = 0.f;
	for (int i = (int)threadIdx.x; i < p.nblocks; i += 256) {
		a += p.partial[i];
		b += p.partial[p.nblocks + i];
	}
	const float l1 = block_sum_256(a, s_red);
	const float ss = block_sum_256(b, s_red);
	if (threadIdx.x == 0) {
		const float inv_n = 1.0f / (3.0f * (float)p.W * (float)p.H);
		p.loss[0] = (1.0f - p.lambda_dssim) * (l1 * inv_n) + p.lambda_dssim * (1.0f - ss * inv_n);
	}
}

// Pass 2: dL/dx = G*(dL/dmu1) + 2x G*(dL/de11) + y G*(dL/de12) + (1-lambda)/N sign(x-y), times mask.
// EXPO: x is recomputed from the three rendered planes at the thread's pixel, G_c = dL/dx_c m_c is written instead of the final
// gradient (exposure_mix_kernel mixes it per pixel), and the workgroup leaves its four partial sums of grad_exposure's column c.
template <bool EXPO>
__global__ void __launch_bounds__(256)
loss_bwd_kernel(const LossKernelParams<EXPO> p)
{
	// staged derivative maps: 3 x 42 x 13 float4; then their filtered rows: 3 x 42 x 9 float4 in the same memory
	__shared__ float4 s_mem[3 * LRY * SP4];
	__shared__ float s_red[4];
	int t, ch, x0, y0;
	if (!loss_tile(p, t, ch, x0, y0)) return;   // (workgroup-uniform)
	const size_t plane = (size_t)p.W * p.H;
	const int tid = (int)threadIdx.x;
	{
		const float* const src[3] = {p.dmaps + (0 * 3 + ch) * plane, p.dmaps + (1 * 3 + ch) * plane, p.dmaps + (2 * 3 + ch) * plane};
		loss_stage_tile<3, EXPO>(src, nullptr, p.W, p.H, p.vec, x0, y0, s_mem, tid);
	}
	__syncthreads();
	auto h_unit = [&](const float (&w)[20], float4& out) {
		float a[LG];
#pragma unroll
		for (int o = 0; o < LG; o++) {
			float acc = 0.f;
#pragma unroll
			for (int t = 0; t < 11; t++) acc += p.g[t] * w[3 + o + t];
			a[o] = acc;
		}
		out = make_float4(a[0], a[1], a[2], a[3]);
	};
	{
		float w[20];
		float4 out1[3], out2[3];
		const int r1 = tid >> 3, g1 = tid & 7;
#pragma unroll
		for (int k = 0; k < 3; k++) {
			loss_load_window(s_mem + k * LRY * SP4, r1, g1, w);
			h_unit(w, out1[k]);
		}
		const bool two = tid + 256 < H_UNITS;
		const int r2 = (tid + 256) >> 3;
		if (two) {
#pragma unroll
			for (int k = 0; k < 3; k++) {
				loss_load_window(s_mem + k * LRY * SP4, r2, g1, w);
				h_unit(w, out2[k]);
			}
		}
		__syncthreads();   // every unit has read its inputs: the filtered rows may overwrite the staged maps
#pragma unroll
		for (int k = 0; k < 3; k++) s_mem[(k * LRY + r1) * HP4 + g1] = out1[k];
		if (two) {
#pragma unroll
			for (int k = 0; k < 3; k++) s_mem[(k * LRY + r2) * HP4 + g1] = out2[k];
		}
	}
	__syncthreads();
	const float inv_n = 1.0f / (3.0f * (float)plane);
	{
		const float* s_h = reinterpret_cast<const float*>(s_mem);
		const int c = tid & (LT - 1), r0 = (tid >> 5) * LGV;
		float cv[3][LGV];
#pragma unroll
		for (int k = 0; k < 3; k++) {
			float col[LWV];
#pragma unroll
			for (int t = 0; t < LWV; t++) col[t] = s_h[(k * LRY + r0 + t) * HP + c];
#pragma unroll
			for (int o = 0; o < LGV; o++) {
				float a = 0.f;
#pragma unroll
				for (int t = 0; t < 11; t++) a += p.g[t] * col[o + t];
				cv[k][o] = a;
			}
		}
		const int gx = x0 + c;
		const float l1w = (1.0f - p.lambda_dssim) * inv_n;
		if constexpr (EXPO) {
			const float e0 = p.E[ch], e1 = p.E[4 + ch], e2 = p.E[8 + ch], e3 = p.E[4 * ch + 3];
			float xs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
			for (int o = 0; o < LGV; o++) {
				const int gy = y0 + r0 + o;
				if (gx < p.W && gy < p.H) {
					const size_t po = (size_t)gy * p.W + gx, oo = ch * plane + po;
					const float m = p.mask ? p.mask[oo] : 1.f;
					const float ra = p.rendered[po], rb = p.rendered[plane + po], rc = p.rendered[2 * plane + po];
					const float xv = exposure_map(ra, rb, rc, e0, e1, e2, e3) * m, yv = p.gt[oo];   // (the mask as the plain kernel applies it)
					const float d = xv - yv;
					const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
					const float gx_ = cv[0][o] + 2.f * xv * cv[1][o] + yv * cv[2][o] + l1w * sgn;
					const float G = gx_ * m;
					p.grad[oo] = G;
					xs[0] += ra * G; xs[1] += rb * G; xs[2] += rc * G; xs[3] += G;
				}
			}
#pragma unroll
			for (int k = 0; k < 4; k++) {
				const float sk = block_sum_256(xs[k], s_red);
				if (tid == 0) p.xpartial[k * p.nblocks + t] = sk;   // (indexed by tile, as p.partial)
			}
		} else {
#pragma unroll
			for (int o = 0; o < LGV; o++) {
				const int gy = y0 + r0 + o;
				if (gx < p.W && gy < p.H) {
					const size_t oo = ch * plane + (size_t)gy * p.W + gx;
					const float m = p.mask ? p.mask[oo] : 1.f;
					const float xv = p.rendered[oo] * m, yv = p.gt[oo];
					const float d = xv - yv;
					const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
					const float gx_ = cv[0][o] + 2.f * xv * cv[1][o] + yv * cv[2][o] + l1w * sgn;
					p.grad[oo] = gx_ * m;
				}
			}
		}
	}
	if (t == 0) loss_finalize(p, s_red);
}

// Pass 3 of the exposure loss, element-wise: grad_rendered_k(p) = sum_c E[k][c] G_c(p), in place over G (a thread reads the three
// G of its pixels before it writes them).  Workgroup 0 then adds the [4][nblocks] partial sums of pass 2 to the 12 entries of
// grad_exposure in tile order, as loss_finalize does for the loss: [k][c] (c < 3) and [c][3] come from the tiles of channel c.
constexpr int MIX_MAX_BLOCKS = 2048;
static inline int stream_blocks(size_t n) { return (int)((n + 255) / 256 < (size_t)MIX_MAX_BLOCKS ? (n + 255) / 256 : (size_t)MIX_MAX_BLOCKS); }
__global__ void __launch_bounds__(256)
exposure_mix_kernel(float* __restrict__ grad, size_t plane, const float* __restrict__ E, const float* __restrict__ xpartial,
                    float* __restrict__ grad_exposure, int nblocks)
{
	__shared__ float s_red[4];
	float e[9];
#pragma unroll
	for (int k = 0; k < 3; k++)
#pragma unroll
		for (int c = 0; c < 3; c++) e[3 * k + c] = E[4 * k + c];
	const size_t stride = (size_t)gridDim.x * 256;
	for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < plane; i += stride) {
		const float g0 = grad[i], g1 = grad[plane + i], g2 = grad[2 * plane + i];
		grad[i] = exposure_map(g0, g1, g2, e[0], e[1], e[2], 0.f);
		grad[plane + i] = exposure_map(g0, g1, g2, e[3], e[4], e[5], 0.f);
		grad[2 * plane + i] = exposure_map(g0, g1, g2, e[6], e[7], e[8], 0.f);
	}
	if (blockIdx.x == 0) {
		const int per_ch = nblocks / 3;
		for (int c = 0; c < 3; c++)
			for (int k = 0; k < 4; k++) {
				float a = 0.f;
				for (int i = (int)threadIdx.x; i < per_ch; i += 256) a += xpartial[k * nblocks + c * per_ch + i];
				const float sum = block_sum_256(a, s_red);
				if (threadIdx.x == 0) grad_exposure[k < 3 ? 4 * k + c : 4 * c + 3] = sum;
			}
	}
}

// gsr_apply_exposure: out_c = r_0 E[0][c] + r_1 E[1][c] + r_2 E[2][c] + E[c][3] per pixel, no clamping; out may be the image.
__global__ void __launch_bounds__(256)
apply_exposure_kernel(const float* image, const float* __restrict__ E, size_t plane, float* out)
{
	float e[12];
#pragma unroll
	for (int k = 0; k < 12; k++) e[k] = E[k];
	const size_t stride = (size_t)gridDim.x * 256;
	for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < plane; i += stride) {
		const float r0 = image[i], r1 = image[plane + i], r2 = image[2 * plane + i];
		out[i] = exposure_map(r0, r1, r2, e[0], e[4], e[8], e[3]);
		out[plane + i] = exposure_map(r0, r1, r2, e[1], e[5], e[9], e[7]);
		out[2 * plane + i] = exposure_map(r0, r1, r2, e[2], e[6], e[10], e[11]);
	}
}

// ------------------------------------------------------------------ Adam
// torch.optim.Adam / torch::optim::Adam step (no amsgrad, no weight decay):
//   m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ; p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
// One element of the step.  Contraction is switched off inside: the two kernels below must produce the same bits from the same
// inputs (tests compare them with torch.equal), and with -ffp-contract=fast the compiler forms different FMAs in different
// surroundings (found on the GPU when adam_multi_kernel gained its gradient scale).
__device__ __forceinline__ void adam_update(float& p, float& m, float& v, float g, float b1, float omb1, float b2, float omb2,
                                            float step_size, float inv_sqrt_bc2, float eps)
{
#pragma clang fp contract(off)
	m = b1 * m + omb1 * g;
	v = b2 * v + omb2 * g * g;
	p -= step_size * m / (sqrtf(v) * inv_sqrt_bc2 + eps);
}

__global__ void __launch_bounds__(256)
adam_kernel(float* __restrict__ param, const float* __restrict__ grad, float* __restrict__ exp_avg,
            float* __restrict__ exp_avg_sq, long long n, const AdamScalars a, int period, int split)
{
	const float step_size = a.step_size, step_size_tail = a.step_size_tail, b1 = a.b1, b2 = a.b2, omb1 = a.omb1, omb2 = a.omb2,
	            eps = a.eps, inv_sqrt_bc2 = a.inv_sqrt_bc2;
	// period/split: elements [split, period) of every `period`-element row use step_size_tail (the SH buffer
	// keeps features_dc (lr) and features_rest (lr/20) in one [P,16,3] tensor); period == 0: uniform.
	const long long stride = (long long)gridDim.x * blockDim.x * 4;
	const long long i0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
	const bool aligned = ((reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(exp_avg) |
	                       reinterpret_cast<uintptr_t>(exp_avg_sq)) & 15) == 0;
	// position inside the `period`-element row, carried in 32 bits (one 64-bit modulo per thread, not per element)
	const uint32_t per = (uint32_t)period;
	uint32_t r = per ? (uint32_t)(i0 % (long long)per) : 0u;
	const uint32_t dr = per ? (uint32_t)(stride % (long long)per) : 0u;
	for (long long i = i0; i < n; i += stride) {
		if (i + 3 < n && aligned) {
			// every access is streaming (non-temporal): nothing here is reused before 3 GB of other traffic has passed
			// (measured 604 -> 531 us per step at C3 against default-cached accesses)
			float4 pv = load_stream_f4(reinterpret_cast<const float4*>(param + i));
			const float4 gv = load_stream_f4(reinterpret_cast<const float4*>(grad + i));
			float4 mv = load_stream_f4(reinterpret_cast<const float4*>(exp_avg + i));
			float4 vv = load_stream_f4(reinterpret_cast<const float4*>(exp_avg_sq + i));
			float* pp = &pv.x; const float* gp = &gv.x; float* mp = &mv.x; float* vp = &vv.x;
#pragma unroll
			for (int k = 0; k < 4; k++) {
				uint32_t rk = r + (uint32_t)k;
				if (rk >= per) rk -= per;
				const float ss = (per && rk >= (uint32_t)split) ? step_size_tail : step_size;
				adam_update(pp[k], mp[k], vp[k], gp[k], b1, omb1, b2, omb2, ss, inv_sqrt_bc2, eps);
			}
			store_stream_f4(reinterpret_cast<float4*>(param + i), pv);
			store_stream_f4(reinterpret_cast<float4*>(exp_avg + i), mv);
			store_stream_f4(reinterpret_cast<float4*>(exp_avg_sq + i), vv);
		} else {
			for (long long k = i; k < n && k < i + 4; k++) {
				uint32_t rk = r + (uint32_t)(k - i);
				if (rk >= per) rk -= per;
				const float ss = (per && rk >= (uint32_t)split) ? step_size_tail : step_size;
				float pk = param[k], mk = exp_avg[k], vk = exp_avg_sq[k];
				adam_update(pk, mk, vk, grad[k], b1, omb1, b2, omb2, ss, inv_sqrt_bc2, eps);
				exp_avg[k] = mk;
				exp_avg_sq[k] = vk;
				param[k] = pk;
			}
		}
		r += dr;
		if (r >= per) r -= per;
	}
}

// Densification statistics of one view (src/gaussian_mapper.cpp:714-719, src/gaussian_model.cpp:817-831):
//   max_radii2D[vis] = max(max_radii2D[vis], radii[vis]); xyz_gradient_accum[vis] += |dL/dmean2D.xy|; denom[vis] += 1
// with vis = radii > 0.  The reference does this with boolean-mask gathers/scatters (nonzero + index_put_:
// 8 partition kernels and a host sync per step); one pass over P here.
__global__ void __launch_bounds__(256)
densify_stats_kernel(int P, const float* __restrict__ dL_dmean2D, const int* __restrict__ radii,
                     float* __restrict__ accum, float* __restrict__ denom, float* __restrict__ max_radii)
{
	const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	if (i >= P) return;
	const int r = radii[i];
	if (r > 0) {
		const float gx = dL_dmean2D[3 * (size_t)i], gy = dL_dmean2D[3 * (size_t)i + 1];
		accum[i] += sqrtf(gx * gx + gy * gy);
		denom[i] += 1.0f;
		max_radii[i] = fmaxf(max_radii[i], (float)r);
	}
}

}  // namespace gsr

using namespace gsr;

extern "C" {

#ifdef GSR_EMU
// (emulator build only) the number of misaligned 16-byte staging loads since the last call
long long gsr_emu_loss_misaligned_loads() { return g_loss_misaligned_loads.exchange(0); }
#endif

size_t gsr_loss_scratch_bytes(int width, int height)
{
	if (width <= 0 || height <= 0) return 0;
	const size_t plane = (size_t)width * height;
	const size_t nb = (size_t)div_up(width, LT) * div_up(height, LTY) * 3;
	return (9 * plane + 2 * nb + 64) * sizeof(float);
}

// the kernel parameters both loss entries share
static void loss_params(LossParams& p, const float* rendered, const float* gt, const float* mask, int width, int height,
                        float lambda_dssim, float* grad_rendered, float* loss, char* scratch)
{
	p.rendered = rendered; p.gt = gt; p.mask = mask; p.W = width; p.H = height; p.lambda_dssim = lambda_dssim;
	// 16-byte staging: every row of every plane (inputs and the derivative maps in `scratch`) starts on a 16-byte boundary
	p.vec = (width % 4 == 0) && !((reinterpret_cast<uintptr_t>(rendered) | reinterpret_cast<uintptr_t>(gt) |
	                              reinterpret_cast<uintptr_t>(mask) | reinterpret_cast<uintptr_t>(scratch)) & 15);
	// gaussian(11, 1.5) normalised, include/loss_utils.h:49-62.  The normaliser is torch's gauss.sum(): the correctly rounded
	// sum of the eleven floats (a sequential float sum is one ulp lower: the weights then sum to 1 + 6e-8 instead of the
	// reference's 1 - 1.6e-8, and sigma = E[x^2] - mu^2 -- a difference of two numbers ~0.25 that is itself ~1e-3 -- inherits
	// mu^2 * 1.5e-7 with ONE sign over the whole image: a 2e-5 relative bias of the loss on a near-converged view, 150x the
	// reference's own float error against float64; found by tests/test_train_sequence_reference.py)
	double sum = 0.0;
	for (int x = 0; x < 11; x++) {
		const int t = x - 5;
		p.g[x] = expf(-(float)(t * t) / (2.0f * 1.5f * 1.5f));
		sum += (double)p.g[x];
	}
	const float fsum = (float)sum;
	for (int x = 0; x < 11; x++) p.g[x] /= fsum;
	const size_t plane = (size_t)width * height;
	const int gx = div_up(width, LT), gy = div_up(height, LTY);
	p.nblocks = gx * gy * 3;
	p.gx = gx; p.gy = gy;
	p.dmaps = reinterpret_cast<float*>(scratch);
	p.partial = p.dmaps + 9 * plane;
	p.grad = grad_rendered;
	p.loss = loss;
}

int gsr_l1_ssim_loss(const float* rendered, const float* gt, const float* mask, int width, int height, float lambda_dssim,
                     float* grad_rendered, float* loss, char* scratch, void* stream_)
{
	if (!rendered || !gt || !grad_rendered || !loss || !scratch || width <= 0 || height <= 0) return GSR_ERR_INVALID_ARG;
	hipStream_t stream = (hipStream_t)stream_;
	LossParams p;
	loss_params(p, rendered, gt, mask, width, height, lambda_dssim, grad_rendered, loss, scratch);
	GSR_LAUNCH(loss_fwd_kernel<false>, loss_grid(p.nblocks), 256, stream, p);
	GSR_LAUNCH(loss_bwd_kernel<false>, loss_grid(p.nblocks), 256, stream, p);
	GSR_CHECK_LAUNCH();
	return GSR_OK;
}

size_t gsr_loss_exposure_scratch_bytes(int width, int height)
{
	if (width <= 0 || height <= 0) return 0;
	const size_t nb = (size_t)div_up(width, LT) * div_up(height, LTY) * 3;
	return gsr_loss_scratch_bytes(width, height) + 4 * nb * sizeof(float);
}

int gsr_l1_ssim_loss_exposure(const float* rendered, const float* gt, const float* mask, int width, int height, float lambda_dssim,
                              const float* exposure, float* grad_rendered, float* grad_exposure, float* loss, char* scratch,
                              void* stream_)
{
	if (!rendered || !gt || !exposure || !grad_rendered || !grad_exposure || !loss || !scratch || width <= 0 || height <= 0)
		return GSR_ERR_INVALID_ARG;
	hipStream_t stream = (hipStream_t)stream_;
	LossExposureParams p;
	loss_params(p, rendered, gt, mask, width, height, lambda_dssim, grad_rendered, loss, scratch);
	p.E = exposure;
	// behind the plain entry's region: 9 planes, [2][nblocks] partial sums and its 64 floats of slack
	p.xpartial = reinterpret_cast<float*>(scratch + gsr_loss_scratch_bytes(width, height));
	p.grad_exposure = grad_exposure;
	const size_t plane = (size_t)width * height;
	const int mix_blocks = stream_blocks(plane);
	GSR_LAUNCH(loss_fwd_kernel<true>, loss_grid(p.nblocks), 256, stream, p);
	GSR_LAUNCH(loss_bwd_kernel<true>, loss_grid(p.nblocks), 256, stream, p);
	GSR_LAUNCH(exposure_mix_kernel, mix_blocks, 256, stream, grad_rendered, plane, p.E, p.xpartial, p.grad_exposure, p.nblocks);
	GSR_CHECK_LAUNCH();
	return GSR_OK;
}

int gsr_apply_exposure(const float* image, const float* exposure, int width, int height, float* out, void* stream_)
{
	if (!image || !exposure || !out || width <= 0 || height <= 0) return GSR_ERR_INVALID_ARG;
	hipStream_t stream = (hipStream_t)stream_;
	const size_t plane = (size_t)width * height;
	const int blocks = stream_blocks(plane);
	GSR_LAUNCH(apply_exposure_kernel, blocks, 256, stream, image, exposure, plane, out);
	GSR_CHECK_LAUNCH();
	return GSR_OK;
}

int gsr_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long long n, double lr, double beta1,
                  double beta2, double eps, int step, int period, int split, double lr_tail, void* stream_)
{
	if (n < 0 || step < 1) return GSR_ERR_INVALID_ARG;
	if (n == 0) return GSR_OK;
	if (!param || !grad || !exp_avg || !exp_avg_sq) return GSR_ERR_INVALID_ARG;
	hipStream_t stream = (hipStream_t)stream_;
	const AdamScalars as = adam_scalars(lr, lr_tail, beta1, beta2, eps, step);
	long long blocks = (n / 4 + 255) / 256;
	// one float4 per thread: measured 609 us per step at C3 against 729 us for an 8192-block grid-stride loop
	if (blocks > 0x7FFFFFFFll) blocks = 0x7FFFFFFFll;
	if (blocks < 1) blocks = 1;
	GSR_LAUNCH(adam_kernel, (int)blocks, 256, stream, param, grad, exp_avg, exp_avg_sq, n, as, period, split);
	GSR_CHECK_LAUNCH();
	return GSR_OK;
}

// Several tensors in ONE launch (gsr_adam_step_multi): block b works on the tensor whose block range holds it, one float4 per
// thread, the arithmetic of adam_kernel (uniform learning rate per tensor).
constexpr int ADAM_MULTI_MAX = 8;
struct AdamMultiParams {
	float* param[ADAM_MULTI_MAX];
	const float* grad[ADAM_MULTI_MAX];
	float* exp_avg[ADAM_MULTI_MAX];
	float* exp_avg_sq[ADAM_MULTI_MAX];
	long long n[ADAM_MULTI_MAX];
	int first_block[ADAM_MULTI_MAX + 1];
	AdamScalars s[ADAM_MULTI_MAX];
	float grad_scale[ADAM_MULTI_MAX];
	int count;
};
}  // extern "C"
namespace gsr {
__global__ void __launch_bounds__(256)
adam_multi_kernel(const AdamMultiParams q)
{
	int t = 0;
#pragma unroll
	for (int k = 1; k < ADAM_MULTI_MAX; k++)
		if (k < q.count && (int)blockIdx.x >= q.first_block[k]) t = k;
	float* __restrict__ param = q.param[t];
	const float* __restrict__ grad = q.grad[t];
	float* __restrict__ exp_avg = q.exp_avg[t];
	float* __restrict__ exp_avg_sq = q.exp_avg_sq[t];
	const long long n = q.n[t];
	const AdamScalars a = q.s[t];
	const float gs = q.grad_scale[t];
	const long long i = ((long long)((int)blockIdx.x - q.first_block[t]) * 256 + threadIdx.x) * 4;
	if (i >= n) return;
	const bool aligned = ((reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(exp_avg) |
	                       reinterpret_cast<uintptr_t>(exp_avg_sq)) & 15) == 0;
	if (i + 3 < n && aligned) {
		float4 pv = load_stream_f4(reinterpret_cast<const float4*>(param + i));
		const float4 gv = load_stream_f4(reinterpret_cast<const float4*>(grad + i));
		float4 mv = load_stream_f4(reinterpret_cast<const float4*>(exp_avg + i));
		float4 vv = load_stream_f4(reinterpret_cast<const float4*>(exp_avg_sq + i));
		float* pp = &pv.x; const float* gp = &gv.x; float* mp = &mv.x; float* vp = &vv.x;
#pragma unroll
		for (int k = 0; k < 4; k++) {
			const float g = gs == 1.0f ? gp[k] : gp[k] * gs;
			adam_update(pp[k], mp[k], vp[k], g, a.b1, a.omb1, a.b2, a.omb2, a.step_size, a.inv_sqrt_bc2, a.eps);
		}
		store_stream_f4(reinterpret_cast<float4*>(param + i), pv);
		store_stream_f4(reinterpret_cast<float4*>(exp_avg + i), mv);
		store_stream_f4(reinterpret_cast<float4*>(exp_avg_sq + i), vv);
	} else {
		for (long long k = i; k < n && k < i + 4; k++) {
			const float g = gs == 1.0f ? grad[k] : grad[k] * gs;
			float pk = param[k], mk = exp_avg[k], vk = exp_avg_sq[k];
			adam_update(pk, mk, vk, g, a.b1, a.omb1, a.b2, a.omb2, a.step_size, a.inv_sqrt_bc2, a.eps);
			exp_avg[k] = mk;
			exp_avg_sq[k] = vk;
			param[k] = pk;
		}
	}
}
}  // namespace gsr
extern "C" {

int gsr_adam_step_multi(int count, const gsr_adam_multi_tensor* tensors, double beta1, double beta2, double eps, void* stream_)
{
	if (count < 0 || count > ADAM_MULTI_MAX || (count && !tensors)) return GSR_ERR_INVALID_ARG;
	AdamMultiParams q{};
	long long blocks = 0;
	int used = 0;
	for (int k = 0; k < count; k++) {
		const gsr_adam_multi_tensor& t = tensors[k];
		if (t.n < 0 || t.step < 1) return GSR_ERR_INVALID_ARG;
		if (t.n == 0) continue;
		if (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq) return GSR_ERR_INVALID_ARG;
		q.param[used] = t.param; q.grad[used] = t.grad; q.exp_avg[used] = t.exp_avg; q.exp_avg_sq[used] = t.exp_avg_sq;
		q.n[used] = t.n;
		q.s[used] = adam_scalars(t.lr, t.lr, beta1, beta2, eps, t.step);
		// (a zero-initialised struct -- the idiom of every gsr struct -- means "no scaling", not "multiply the gradient by 0")
		if (!(t.grad_scale >= 0.0f) || t.grad_scale > 3.0e38f) return GSR_ERR_INVALID_ARG;   // negative, NaN, Inf
		q.grad_scale[used] = t.grad_scale == 0.0f ? 1.0f : t.grad_scale;
		q.first_block[used] = (int)blocks;
		blocks += (t.n + 1023) / 1024;
		if (blocks > 0x7FFFFFFFll) return GSR_ERR_UNSUPPORTED;
		used++;
	}
	if (!used) return GSR_OK;
	q.first_block[used] = (int)blocks;
	q.count = used;
	hipStream_t stream = (hipStream_t)stream_;
	GSR_LAUNCH(adam_multi_kernel, (int)blocks, 256, stream, q);
	GSR_CHECK_LAUNCH();
	return GSR_OK;
}

int gsr_densify_stats(int P, const float* dL_dmean2D, const int* radii, float* xyz_gradient_accum, float* denom,
                      float* max_radii2D, void* stream_)
{
	if (P < 0) return GSR_ERR_INVALID_ARG;
	if (P == 0) return GSR_OK;
	if (!dL_dmean2D || !radii || !xyz_gradient_accum || !denom || !max_radii2D) return GSR_ERR_INVALID_ARG;
	hipStream_t stream = (hipStream_t)stream_;
	GSR_LAUNCH(densify_stats_kernel, div_up(P, 256), 256, stream, P, dL_dmean2D, radii, xyz_gradient_accum, denom, max_radii2D);
	GSR_CHECK_LAUNCH();
	return GSR_OK;
}

}  // extern "C"

// ---- depth L1 loss of an RGB-D keyframe (gsr_depth_l1_loss): pass 1 writes the gradient and one partial sum per workgroup (a
// fixed grid over a fixed element order), pass 2 -- one workgroup -- sums the partials in index order: the same bits every run.
namespace gsr {
constexpr int DL_THREADS = 256;
constexpr int DL_MAX_BLOCKS = 1024;
static inline int depth_loss_blocks(size_t n) { return (int)(n / (DL_THREADS * 8) + 1 < (size_t)DL_MAX_BLOCKS ? n / (DL_THREADS * 8) + 1 : DL_MAX_BLOCKS); }

__global__ void __launch_bounds__(DL_THREADS)
depth_l1_partial_kernel(const float* __restrict__ depth, const float* __restrict__ gt, size_t n, float min_depth, float max_depth,
                        float scale, float* __restrict__ grad, float* __restrict__ partial)
{
	__shared__ float s4[4];
	const size_t stride = (size_t)gridDim.x * DL_THREADS;
	float acc = 0.f;
	for (size_t i = (size_t)blockIdx.x * DL_THREADS + threadIdx.x; i < n; i += stride) {
		const float d = depth[i], g = gt[i];
		const bool valid = g > min_depth && g < max_depth;
		const float diff = d - g;
		const float sgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
		if (valid) acc += fabsf(diff);
		grad[i] = valid ? sgn * scale : 0.f;
	}
	const float s = block_sum_256(acc, s4);
	if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ void __launch_bounds__(DL_THREADS)
depth_l1_final_kernel(const float* __restrict__ partial, int nblocks, float scale, float* __restrict__ loss)
{
	__shared__ float s4[4];
	float a = 0.f;
	for (int i = (int)threadIdx.x; i < nblocks; i += DL_THREADS) a += partial[i];
	const float s = block_sum_256(a, s4);
	if (threadIdx.x == 0) loss[0] = s * scale;
}
}  // namespace gsr
extern "C" {

size_t gsr_depth_loss_scratch_bytes(int width, int height)
{
	if (width <= 0 || height <= 0) return 0;
	return (size_t)depth_loss_blocks((size_t)width * height) * sizeof(float);
}

int gsr_depth_l1_loss(const float* depth, const float* gt_depth, int width, int height, float min_depth, float max_depth,
                      float weight, float* grad_depth, float* loss, char* scratch, void* stream_)
{
	if (!depth || !gt_depth || !grad_depth || !loss || !scratch || width <= 0 || height <= 0) return GSR_ERR_INVALID_ARG;
	hipStream_t stream = (hipStream_t)stream_;
	const size_t n = (size_t)width * height;
	const int blocks = depth_loss_blocks(n);
	// d loss / d depth of the valid pixels: weight / (H W) times the sign, the factor autograd forms for weight * sum / (H W)
	const float scale = (1.0f / (float)n) * weight;
	float* partial = reinterpret_cast<float*>(scratch);
	GSR_LAUNCH(depth_l1_partial_kernel, blocks, DL_THREADS, stream, depth, gt_depth, n, min_depth, max_depth, scale, grad_depth, partial);
	GSR_LAUNCH(depth_l1_final_kernel, 1, DL_THREADS, stream, partial, blocks, scale, loss);
	GSR_CHECK_LAUNCH();
	return GSR_OK;
}

}  // extern "C"

// ---- monocular depth prior (gsr_depth_prior_loss, gsr_depth_prior_apply): a relative-depth map q that is right only up to a scale
// and a shift, against the rendered quantity r = D / A (or A / D).  Pass 1 leaves six fp64 moment sums per workgroup, pass 2 -- one
// workgroup -- sums them in index order and solves the fit, pass 3 writes the gradients (and, for the aligned L1, one fp64 partial
// sum per workgroup), pass 4 -- one workgroup -- sums those.  Fixed grids over a fixed element order, no atomics: the same bits every
// run.  A thread owns whole groups of four consecutive pixels; the 16-byte and the scalar path differ in how a group is loaded and
// stored and in nothing else, so they give the same bits.
namespace gsr {
constexpr int DP_THREADS = 256;
constexpr int DP_MAX_BLOCKS = 1024;
constexpr int DP_MOMENTS = 6;   // n, sum q, sum r, sum qq, sum qr, sum rr
// coefficients pass 2 leaves for pass 3 and 4 (fp64, in scratch)
enum { DP_S = 0, DP_T, DP_QM, DP_RM, DP_CA, DP_CB, DP_OK, DP_COEFS = 8 };
static inline int depth_prior_blocks(size_t n)
{
	const size_t groups = (n + 3) / 4, b = (groups + DP_THREADS - 1) / DP_THREADS;
	return (int)(b < (size_t)DP_MAX_BLOCKS ? b : (size_t)DP_MAX_BLOCKS);
}

struct DepthPriorParams {
	const float* depth;
	const float* alpha;      // or null: all ones
	const float* prior;
	const uint8_t* valid;    // or null: all set
	size_t n;                // H W
	int vec;                 // every pointer 16-byte aligned: groups move as 16-byte vectors
	int inverse, pearson;
	float alpha_min;
	double weight;
	float* grad_depth;
	float* grad_alpha;       // null exactly when alpha is
	float* loss;             // or null (with grad_depth): the fit only
	float* fit;              // [4]
	double* partial;         // [nblocks][DP_MOMENTS]
	double* coef;            // [DP_COEFS]
	double* lpartial;        // [nblocks]
	int nblocks;
};

// group g = pixels 4 g .. 4 g + 3 (the last group may be short: its missing pixels come back with v = 0)
__device__ __forceinline__ void depth_prior_load4(const DepthPriorParams& p, size_t g, float (&D)[4], float (&A)[4], float (&q)[4],
                                                  unsigned (&v)[4])
{
	const size_t i = 4 * g;
	if (p.vec && i + 3 < p.n) {
		const float4 d4 = *reinterpret_cast<const float4*>(p.depth + i), q4 = *reinterpret_cast<const float4*>(p.prior + i);
		D[0] = d4.x; D[1] = d4.y; D[2] = d4.z; D[3] = d4.w;
		q[0] = q4.x; q[1] = q4.y; q[2] = q4.z; q[3] = q4.w;
		if (p.alpha) {
			const float4 a4 = *reinterpret_cast<const float4*>(p.alpha + i);
			A[0] = a4.x; A[1] = a4.y; A[2] = a4.z; A[3] = a4.w;
		} else {
			A[0] = A[1] = A[2] = A[3] = 1.f;
		}
		const uint32_t m = p.valid ? *reinterpret_cast<const uint32_t*>(p.valid + i) : 0x01010101u;
		v[0] = m & 0xffu; v[1] = (m >> 8) & 0xffu; v[2] = (m >> 16) & 0xffu; v[3] = m >> 24;
	} else {
#pragma unroll
		for (int k = 0; k < 4; k++) {
			const bool in = i + k < p.n;
			D[k] = in ? p.depth[i + k] : 0.f;
			q[k] = in ? p.prior[i + k] : 0.f;
			A[k] = in && p.alpha ? p.alpha[i + k] : 1.f;
			v[k] = in ? (p.valid ? (unsigned)p.valid[i + k] : 1u) : 0u;
		}
	}
}

// The validity rule and the rendered quantity of one pixel (r in fp64 from the fp32 maps).  Every comparison is false for a NaN.  A
// pixel whose r is not a positive finite float (alpha 0 under an alpha_min <= 0, a depth of +Inf) is left out like an invalid one:
// nothing that is not finite enters a sum.
__device__ __forceinline__ bool depth_prior_pixel(float D, float A, float q, unsigned v, float alpha_min, int inverse, double& r)
{
	const bool ok = A >= alpha_min && D > 0.f && q > 0.f && q <= 3.4028234663852886e38f && v != 0u;
	const double num = inverse ? (double)A : (double)D, den = inverse ? (double)D : (double)A;
	r = ok ? num / den : 0.0;
	const bool fin = r > 0.0 && r <= 3.4028234663852886e38;
	if (!fin) r = 0.0;
	return ok && fin;
}

__device__ __forceinline__ void depth_prior_accumulate(double (&m)[DP_MOMENTS], double q, double r)
{
#pragma clang fp contract(off)
	m[0] += 1.0;
	m[1] += q;
	m[2] += r;
	m[3] += q * q;
	m[4] += q * r;
	m[5] += r * r;
}

// K sums over the workgroup in a fixed tree, valid in every thread (fp64 has no DPP form here: through LDS)
template <int K>
__device__ __forceinline__ void block_sum_f64(double (&v)[K], double* s /*[K][DP_THREADS]*/)
{
	const int tid = (int)threadIdx.x;
	__syncthreads();   // s reuse across calls
#pragma unroll
	for (int k = 0; k < K; k++) s[k * DP_THREADS + tid] = v[k];
	__syncthreads();
	for (int off = DP_THREADS / 2; off > 0; off >>= 1) {
		if (tid < off) {
#pragma unroll
			for (int k = 0; k < K; k++) s[k * DP_THREADS + tid] += s[k * DP_THREADS + tid + off];
		}
		__syncthreads();
	}
#pragma unroll
	for (int k = 0; k < K; k++) v[k] = s[k * DP_THREADS];
}

__global__ void __launch_bounds__(DP_THREADS)
depth_prior_moments_kernel(const DepthPriorParams p)
{
	__shared__ double s_red[DP_MOMENTS * DP_THREADS];
	double m[DP_MOMENTS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
	const size_t groups = (p.n + 3) / 4, stride = (size_t)gridDim.x * DP_THREADS;
	for (size_t g = (size_t)blockIdx.x * DP_THREADS + threadIdx.x; g < groups; g += stride) {
		float D[4], A[4], q[4];
		unsigned v[4];
		depth_prior_load4(p, g, D, A, q, v);
#pragma unroll
		for (int k = 0; k < 4; k++) {
			double r;
			if (depth_prior_pixel(D[k], A[k], q[k], v[k], p.alpha_min, p.inverse, r)) depth_prior_accumulate(m, (double)q[k], r);
		}
	}
	block_sum_f64<DP_MOMENTS>(m, s_red);
	if (threadIdx.x == 0) {
#pragma unroll
		for (int k = 0; k < DP_MOMENTS; k++) p.partial[(size_t)blockIdx.x * DP_MOMENTS + k] = m[k];
	}
}

// One workgroup: the moments from the partial sums in index order, the closed-form fit, rho and the degenerate rule.
__global__ void __launch_bounds__(DP_THREADS)
depth_prior_fit_kernel(const DepthPriorParams p)
{
	__shared__ double s_red[DP_MOMENTS * DP_THREADS];
	double m[DP_MOMENTS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
	for (int i = (int)threadIdx.x; i < p.nblocks; i += DP_THREADS)
#pragma unroll
		for (int k = 0; k < DP_MOMENTS; k++) m[k] += p.partial[(size_t)i * DP_MOMENTS + k];
	block_sum_f64<DP_MOMENTS>(m, s_red);
	if (threadIdx.x != 0) return;
	const double n = m[0];
	double s = 0.0, t = 0.0, rho = 0.0, qm = 0.0, rm = 0.0, ca = 0.0, cb = 0.0;
	bool ok = false;
	if (n >= 2.0) {
		qm = m[1] / n;
		rm = m[2] / n;
		const double sqq = m[3] - m[1] * qm, sqr = m[4] - m[1] * rm, srr = m[5] - m[2] * rm;
		const bool q_ok = sqq > 1e-12 * m[3], r_ok = srr > 1e-12 * m[5];
		if (q_ok && r_ok) {
			rho = sqr / sqrt(sqq * srr);
			rho = rho > 1.0 ? 1.0 : (rho < -1.0 ? -1.0 : rho);
			ca = 1.0 / sqrt(sqq * srr);   // 1 / (S_q S_r)
			cb = rho / srr;               // rho / S_r^2
		}
		ok = p.pearson ? (q_ok && r_ok) : q_ok;
		if (ok) {
			s = sqr / sqq;
			t = rm - s * qm;
		} else {
			rho = 0.0;
		}
	}
	p.fit[0] = (float)s; p.fit[1] = (float)t; p.fit[2] = (float)rho; p.fit[3] = (float)n;
	p.coef[DP_S] = s; p.coef[DP_T] = t; p.coef[DP_QM] = qm; p.coef[DP_RM] = rm; p.coef[DP_CA] = ca; p.coef[DP_CB] = cb;
	p.coef[DP_OK] = ok ? 1.0 : 0.0;
	if (p.loss && p.pearson) p.loss[0] = ok ? (float)(p.weight * (1.0 - rho)) : 0.f;
}

// one pixel's dloss/dr, and for the aligned L1 its |residual|
__device__ __forceinline__ double depth_prior_dr(const DepthPriorParams& p, const double (&c)[DP_COEFS], double wl, double q, double r,
                                                 double& abs_res)
{
#pragma clang fp contract(off)
	if (p.pearson) return -p.weight * ((q - c[DP_QM]) * c[DP_CA] - c[DP_CB] * (r - c[DP_RM]));
	const double res = r - (c[DP_S] * q + c[DP_T]);
	abs_res += fabs(res);
	return res > 0.0 ? wl : (res < 0.0 ? -wl : 0.0);
}
__device__ __forceinline__ float depth_prior_finite(double g)
{
	const float f = (float)g;
	return f >= -3.4028234663852886e38f && f <= 3.4028234663852886e38f ? f : 0.f;
}

__global__ void __launch_bounds__(DP_THREADS)
depth_prior_grad_kernel(const DepthPriorParams p)
{
	__shared__ double s_red[DP_THREADS];
	double c[DP_COEFS];
#pragma unroll
	for (int k = 0; k < DP_COEFS; k++) c[k] = p.coef[k];
	const bool ok = c[DP_OK] != 0.0;
	const double wl = p.weight / (double)p.n;
	double acc[1] = {0.0};
	const size_t groups = (p.n + 3) / 4, stride = (size_t)gridDim.x * DP_THREADS;
	for (size_t g = (size_t)blockIdx.x * DP_THREADS + threadIdx.x; g < groups; g += stride) {
		float D[4], A[4], q[4], gd[4], ga[4];
		unsigned v[4];
		depth_prior_load4(p, g, D, A, q, v);
#pragma unroll
		for (int k = 0; k < 4; k++) {
			double r;
			gd[k] = 0.f;
			ga[k] = 0.f;
			if (depth_prior_pixel(D[k], A[k], q[k], v[k], p.alpha_min, p.inverse, r) && ok) {
				const double dr = depth_prior_dr(p, c, wl, (double)q[k], r, acc[0]);
				// default: dr/dD = 1/A, dr/dA = -D/A^2 = -r/A;  inverse: dr/dD = -A/D^2 = -r/D, dr/dA = 1/D
				const double den = p.inverse ? (double)D[k] : (double)A[k];
				const double direct = dr / den, cross = -(dr * r) / den;
				gd[k] = depth_prior_finite(p.inverse ? cross : direct);
				ga[k] = depth_prior_finite(p.inverse ? direct : cross);
			}
		}
		const size_t i = 4 * g;
		if (p.vec && i + 3 < p.n) {
			*reinterpret_cast<float4*>(p.grad_depth + i) = make_float4(gd[0], gd[1], gd[2], gd[3]);
			if (p.grad_alpha) *reinterpret_cast<float4*>(p.grad_alpha + i) = make_float4(ga[0], ga[1], ga[2], ga[3]);
		} else {
#pragma unroll
			for (int k = 0; k < 4; k++)
				if (i + k < p.n) {
					p.grad_depth[i + k] = gd[k];
					if (p.grad_alpha) p.grad_alpha[i + k] = ga[k];
				}
		}
	}
	if (p.pearson) return;   // (workgroup-uniform) its loss left pass 2
	block_sum_f64<1>(acc, s_red);
	if (threadIdx.x == 0) p.lpartial[blockIdx.x] = acc[0];
}

__global__ void __launch_bounds__(DP_THREADS)
depth_prior_final_kernel(const DepthPriorParams p)
{
	__shared__ double s_red[DP_THREADS];
	double a[1] = {0.0};
	for (int i = (int)threadIdx.x; i < p.nblocks; i += DP_THREADS) a[0] += p.lpartial[i];
	block_sum_f64<1>(a, s_red);
	if (threadIdx.x == 0) p.loss[0] = depth_prior_finite(a[0] * (p.weight / (double)p.n));
}

// gsr_depth_prior_apply: the fitted map, 0 where the prior is invalid or the result is not a positive finite float; out may be prior
__global__ void __launch_bounds__(DP_THREADS)
depth_prior_apply_kernel(const float* prior, const float* __restrict__ fit, int inverse, size_t n, float* out)
{
	const double s = (double)fit[0], t = (double)fit[1];
	const size_t stride = (size_t)gridDim.x * DP_THREADS;
	for (size_t i = (size_t)blockIdx.x * DP_THREADS + threadIdx.x; i < n; i += stride) {
		const float q = prior[i];
		float o = 0.f;
		if (q > 0.f && q <= 3.4028234663852886e38f) {
			double m = s * (double)q + t;
			if (inverse) m = m > 0.0 ? 1.0 / m : 0.0;
			const float f = (float)m;
			if (f > 0.f && f <= 3.4028234663852886e38f) o = f;
		}
		out[i] = o;
	}
}
}  // namespace gsr
extern "C" {

size_t gsr_depth_prior_scratch_bytes(int width, int height)
{
	if (width <= 0 || height <= 0) return 0;
	const size_t nb = (size_t)depth_prior_blocks((size_t)width * height);
	return (nb * (DP_MOMENTS + 1) + DP_COEFS) * sizeof(double);
}

int gsr_depth_prior_loss(const gsr_depth_prior_args* a, char* scratch, void* stream_)
{
	if (!a || !scratch || (reinterpret_cast<uintptr_t>(scratch) & 7) || !a->depth || !a->prior || !a->fit || a->width <= 0 ||
	    a->height <= 0)
		return GSR_ERR_INVALID_ARG;
	if (a->flags & ~(GSR_DEPTH_PRIOR_INVERSE | GSR_DEPTH_PRIOR_PEARSON)) return GSR_ERR_INVALID_ARG;
	const bool grads = a->grad_depth != nullptr;
	if (grads != (a->loss != nullptr)) return GSR_ERR_INVALID_ARG;   // both or neither (neither: the fit only)
	if (grads ? (a->grad_alpha != nullptr) != (a->alpha != nullptr) : a->grad_alpha != nullptr) return GSR_ERR_INVALID_ARG;
	hipStream_t stream = (hipStream_t)stream_;
	DepthPriorParams p;
	p.depth = a->depth; p.alpha = a->alpha; p.prior = a->prior; p.valid = a->valid;
	p.n = (size_t)a->width * a->height;
	p.vec = !((reinterpret_cast<uintptr_t>(a->depth) | reinterpret_cast<uintptr_t>(a->alpha) | reinterpret_cast<uintptr_t>(a->prior) |
	           reinterpret_cast<uintptr_t>(a->valid) | reinterpret_cast<uintptr_t>(a->grad_depth) |
	           reinterpret_cast<uintptr_t>(a->grad_alpha)) & 15);
	p.inverse = (a->flags & GSR_DEPTH_PRIOR_INVERSE) ? 1 : 0;
	p.pearson = (a->flags & GSR_DEPTH_PRIOR_PEARSON) ? 1 : 0;
	p.alpha_min = a->alpha_min;
	p.weight = (double)a->weight;
	p.grad_depth = a->grad_depth; p.grad_alpha = a->grad_alpha; p.loss = a->loss; p.fit = a->fit;
	p.nblocks = depth_prior_blocks(p.n);
	p.partial = reinterpret_cast<double*>(scratch);
	p.coef = p.partial + (size_t)p.nblocks * DP_MOMENTS;
	p.lpartial = p.coef + DP_COEFS;
	GSR_LAUNCH(depth_prior_moments_kernel, p.nblocks, DP_THREADS, stream, p);
	GSR_LAUNCH(depth_prior_fit_kernel, 1, DP_THREADS, stream, p);
	if (grads) {
		GSR_LAUNCH(depth_prior_grad_kernel, p.nblocks, DP_THREADS, stream, p);
		if (!p.pearson) GSR_LAUNCH(depth_prior_final_kernel, 1, DP_THREADS, stream, p);
	}
	GSR_CHECK_LAUNCH();
	return GSR_OK;
}

int gsr_depth_prior_apply(const float* prior, const float* fit, int flags, int width, int height, float* out_depth, void* stream_)
{
	if (!prior || !fit || !out_depth || width <= 0 || height <= 0 || (flags & ~(GSR_DEPTH_PRIOR_INVERSE | GSR_DEPTH_PRIOR_PEARSON)))
		return GSR_ERR_INVALID_ARG;
	hipStream_t stream = (hipStream_t)stream_;
	const size_t n = (size_t)width * height;
	GSR_LAUNCH(depth_prior_apply_kernel, stream_blocks(n), DP_THREADS, stream, prior, fit, (flags & GSR_DEPTH_PRIOR_INVERSE) ? 1 : 0, n,
	           out_depth);
	GSR_CHECK_LAUNCH();
	return GSR_OK;
}

}  // extern "C"
