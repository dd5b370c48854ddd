// points.hip -- Photo-SLAM's point-cloud kernels next to the rasterizer:
//   transform_points / scale_and_transform_points         src/operate_points.cu:38-71
//   (helpers transform_point, scale_and_transform_point, transfrom_quaternion_using_matrix,
//    insert_rot_to_rots                                    cuda_rasterizer/operate_points.h:39-179)
//   reproject_depths_pinhole / search_neighborhood_...     src/stereo_vision.cu:39-136
// Small streaming kernels (12-28 B per point); compiled -ffp-contract=off so results are bit-identical
// to the CPU oracle.  The reference's quirks are kept where a caller could observe them and are
// switchable where they are plain bugs (see gsr.h).
#include "state.h"
#include "wave64.h"

#include <float.h>

namespace gsr {

__device__ __forceinline__ void xform4x3(const float* m, float x, float y, float z, float& ox, float& oy, float& oz)
{
	// transformPoint4x3, auxiliary.h:58-66
	ox = m[0] * x + m[4] * y + m[8] * z + m[12];
	oy = m[1] * x + m[5] * y + m[9] * z + m[13];
	oz = m[2] * x + m[6] * y + m[10] * z + m[14];
}

__global__ void __launch_bounds__(256)
transform_points_kernel(int P, const float* __restrict__ pts, const float* __restrict__ m, float* __restrict__ out)
{
	const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	if (i >= P) return;
	float x, y, z;
	xform4x3(m, pts[3 * (size_t)i], pts[3 * (size_t)i + 1], pts[3 * (size_t)i + 2], x, y, z);
	out[3 * (size_t)i] = x;
	out[3 * (size_t)i + 1] = y;
	out[3 * (size_t)i + 2] = z;
}

__global__ void __launch_bounds__(256)
scale_transform_points_kernel(int P, float scale, const float* __restrict__ pts, const float* __restrict__ rots,
                              const float* __restrict__ m, const uint8_t* __restrict__ mask, float* __restrict__ out_pts,
                              float* __restrict__ out_rots, int reference_rot_layout)
{
	const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	if (i >= P || !mask[i]) return;
	float x, y, z;
	xform4x3(m, pts[3 * (size_t)i] * scale, pts[3 * (size_t)i + 1] * scale, pts[3 * (size_t)i + 2] * scale, x, y, z);
	out_pts[3 * (size_t)i] = x;
	out_pts[3 * (size_t)i + 1] = y;
	out_pts[3 * (size_t)i + 2] = z;

	// transfrom_quaternion_using_matrix, operate_points.h:72-156: stored order is (w, x, y, z)
	const float qw = rots[4 * (size_t)i], qx = rots[4 * (size_t)i + 1], qy = rots[4 * (size_t)i + 2], qz = rots[4 * (size_t)i + 3];
	const float tx = 2.0f * qx, ty = 2.0f * qy, tz = 2.0f * qz;
	const float twx = tx * qw, twy = ty * qw, twz = tz * qw;
	const float txx = tx * qx, txy = ty * qx, txz = tz * qx;
	const float tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
	const float R00 = 1.0f - (tyy + tzz), R01 = txy - twz, R02 = txz + twy;
	const float R10 = txy + twz, R11 = 1.0f - (txx + tzz), R12 = tyz - twx;
	const float R20 = txz - twy, R21 = tyz + twx, R22 = 1.0f - (txx + tyy);
	float R[3][3];
	R[0][0] = m[0] * R00 + m[4] * R10 + m[8] * R20;
	R[0][1] = m[0] * R01 + m[4] * R11 + m[8] * R21;
	R[0][2] = m[0] * R02 + m[4] * R12 + m[8] * R22;
	R[1][0] = m[1] * R00 + m[5] * R10 + m[9] * R20;
	R[1][1] = m[1] * R01 + m[5] * R11 + m[9] * R21;
	R[1][2] = m[1] * R02 + m[5] * R12 + m[9] * R22;
	R[2][0] = m[2] * R00 + m[6] * R10 + m[10] * R20;
	R[2][1] = m[2] * R01 + m[6] * R11 + m[10] * R21;
	R[2][2] = m[2] * R02 + m[6] * R12 + m[10] * R22;
	float ow, ox, oy, oz;
	float t = R[0][0] + R[1][1] + R[2][2];
	if (t > 0.0f) {  // Shoemake, "Quaternion Calculus and Fast Animation"
		t = sqrtf(t + 1.0f);
		ow = 0.5f * t;
		t = 0.5f / t;
		ox = (R[2][1] - R[1][2]) * t;
		oy = (R[0][2] - R[2][0]) * t;
		oz = (R[1][0] - R[0][1]) * t;
	} else {
		int a = 0;
		if (R[1][1] > R[0][0]) a = 1;
		if (R[2][2] > R[a][a]) a = 2;
		const int b = (a + 1) % 3, c = (b + 1) % 3;
		t = sqrtf(R[a][a] - R[b][b] - R[c][c] + 1.0f);
		float xyz[3];
		xyz[a] = 0.5f * t;
		t = 0.5f / t;
		ow = (R[c][b] - R[b][c]) * t;
		xyz[b] = (R[b][a] + R[a][b]) * t;
		xyz[c] = (R[c][a] + R[a][c]) * t;
		ox = xyz[0];
		oy = xyz[1];
		oz = xyz[2];
	}
	out_rots[4 * (size_t)i] = ow;
	out_rots[4 * (size_t)i + 1] = ox;
	if (reference_rot_layout) {
		// insert_rot_to_rots writes index +2 twice and never +3 (operate_points.h:175-178): (w, x, z, <untouched>)
		out_rots[4 * (size_t)i + 2] = oz;
	} else {
		out_rots[4 * (size_t)i + 2] = oy;
		out_rots[4 * (size_t)i + 3] = oz;
	}
}

// reproject_depths_pinhole, stereo_vision.cu:39-61 (+ reproject_depth_pinhole, stereo_vision.h:39-53)
__global__ void __launch_bounds__(256)
reproject_depth_kernel(int P, int width, float fx, float fy, float cx, float cy, const float* __restrict__ depths,
                       const uint8_t* __restrict__ mask, float* __restrict__ points)
{
	const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	if (i >= P || !mask[i]) return;
	const int v = i / width, u = i - v * width;
	const float d = depths[i];
	points[3 * (size_t)i] = (u - cx) * d / fx;
	points[3 * (size_t)i + 1] = (v - cy) * d / fy;
	points[3 * (size_t)i + 2] = d;
}

// search_neighborhood_to_estimate_depth_and_reproject_pinhole, stereo_vision.cu:63-136.  Thread = keypoint;
// candidates are staged through LDS in tiles of 256 and scanned in index order, so the first nearest
// candidate wins exactly as in the reference's serial loop.
__global__ void __launch_bounds__(256)
neighborhood_depth_kernel(int N, int width, float fx, float fy, float cx, float cy, float max_pixel_dist,
                          const float* __restrict__ pixels, const uint8_t* __restrict__ has3D,
                          const float* __restrict__ p3d, const float* __restrict__ colors, float* __restrict__ out_p,
                          float* __restrict__ out_c)
{
	__shared__ float s_u[256], s_v[256], s_z[256];
	__shared__ uint8_t s_has[256];
	const int idx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	const bool valid = idx < N;
	const float u = valid ? pixels[2 * (size_t)idx] : 0.f, v = valid ? pixels[2 * (size_t)idx + 1] : 0.f;
	const bool mine3d = valid && has3D[idx];
	float min_dist = FLT_MAX, depth = -1.0f;   // MAXFLOAT
	for (int base = 0; base < N; base += 256) {
		const int j = base + (int)threadIdx.x;
		__syncthreads();
		if (j < N) {
			s_u[threadIdx.x] = pixels[2 * (size_t)j];
			s_v[threadIdx.x] = pixels[2 * (size_t)j + 1];
			s_z[threadIdx.x] = p3d[3 * (size_t)j + 2];
			s_has[threadIdx.x] = has3D[j];
		}
		__syncthreads();
		if (valid && !mine3d) {
			const int n = min(256, N - base);
			for (int k = 0; k < n; k++) {
				if (!s_has[k] || base + k == idx) continue;
				const float du = u - s_u[k], dv = v - s_v[k];
				const float dist = du * du + dv * dv;
				if (dist > max_pixel_dist || dist >= min_dist) continue;
				min_dist = dist;
				depth = s_z[k];
			}
		}
	}
	if (!valid) return;
	const size_t pt = 3 * (size_t)idx;
	const int px_in_image = (int)(v * width + u);   // float arithmetic truncated, as the reference
	if (mine3d) {
		out_p[pt] = p3d[pt];
		out_p[pt + 1] = p3d[pt + 1];
		out_p[pt + 2] = p3d[pt + 2];
		out_c[pt] = colors[px_in_image];
		out_c[pt + 1] = colors[px_in_image + 1];
		out_c[pt + 2] = colors[px_in_image + 2];
		return;
	}
	if (depth > 0.0f) {
		const int ui = (int)u, vi = (int)v;   // reproject_depth_pinhole takes int u, v
		out_p[pt] = (ui - cx) * depth / fx;
		out_p[pt + 1] = (vi - cy) * depth / fy;
		out_p[pt + 2] = depth;
		out_c[pt] = colors[px_in_image];
		out_c[pt + 1] = colors[px_in_image + 1];
		out_c[pt + 2] = colors[px_in_image + 2];
	} else {
		out_p[pt + 2] = -1.0f;
	}
}

// ---------------------------------------------------------------------------------------------------------------------
// Seeding Gaussians from an RGB-D frame (include/gsr.h: gsr_seed_select / gsr_seed_emit).  Per pixel over up to 1920 x 1080; a
// workgroup of 256 threads owns a tile of 1024 consecutive pixels, four per thread, so the three maps are read with 16-byte loads
// and a thread's pixels are consecutive in row-major order.
//
//   seed_hist_kernel  : (median only) one pass of the radix select: e = |gt - depth| of the valid pixels whose upper bits equal the
//                       prefix found so far, counted by the next eight bits in an LDS histogram (integer LDS adds: the counts do
//                       not depend on the order); one histogram per workgroup, the workgroups stride over the tiles
//   seed_pick_kernel  : sums the histograms per bin in workgroup order, scans the 256 bins and extends the prefix by the bin that
//                       holds the wanted rank.  Four pairs of launches leave the median's bits in the state.
//   seed_count_kernel : the flags of every pixel; per tile the number selected, selected by the unseen rule, by the depth rule
//                       alone, and valid
//   seed_spine_kernel : exclusive scan of the tile totals (one workgroup, chunks of 1024 as densify_spine_kernel), counts[0..4]
//   seed_plan_kernel  : the flags again, ranks from a block scan of the per-thread counts -> plan[rank] = pixel
//   seed_emit_kernel  : one work item per unit of a destination row (as mcmc_move_kernel): row P + j takes the pixel of rank
//                       ceil((j+1) n_selected / n_emit) - 1
constexpr int SEED_BLOCK = 256;
constexpr int SEED_TILE = 4 * SEED_BLOCK;   // pixels per workgroup
constexpr int SEED_HIST_BLOCKS = 256;       // workgroups (and histograms) of a radix pass
constexpr uint32_t SF_VALID = 1u, SF_SEL = 2u, SF_UNSEEN = 4u, SF_DEPTH = 8u;

struct SeedState {
	uint32_t prefix;    // the median's upper bits found so far; after the last pass the median's bits
	uint32_t k;         // the wanted rank among the elements that share the prefix
	uint32_t n_valid;
	uint32_t pad;
};

struct SeedSelect {
	int N, width;
	const float* alpha;
	const float* depth;
	const float* gt;
	float min_depth, max_depth, alpha_threshold, err_abs, err_factor;
	int stride, offset_x, offset_y;
	int rule;   // 0: the depth rule is off, 1: T = err_abs, 2: T = max(err_abs, err_factor * median)
	int vec;    // every map's base is 16-byte aligned
	// scratch
	SeedState* state;
	uint32_t* tile_counts;   // [4][ntiles]: selected, by the unseen rule, by the depth rule alone, valid; row 0 becomes offsets
	uint32_t* blk_hist;      // [SEED_HIST_BLOCKS][256]
	uint32_t* plan;          // [N]
};

struct SeedPixels {
	float g[4], a[4], d[4];
};

__device__ __forceinline__ float seed_load1(const float* map, int i, int n, float fill) { return (map && i < n) ? map[i] : fill; }

// the four pixels [i0, i0 + 4) of the three maps; pixels past the end read as gt = NaN (not valid)
__device__ __forceinline__ SeedPixels seed_load(const SeedSelect& p, int i0)
{
	const float nan = __uint_as_float(0x7FC00000u);
	float4 g, a = make_float4(0.f, 0.f, 0.f, 0.f), d = make_float4(0.f, 0.f, 0.f, 0.f);
	if (p.vec && i0 + 3 < p.N) {
		g = *reinterpret_cast<const float4*>(p.gt + i0);
		if (p.alpha) {
			a = *reinterpret_cast<const float4*>(p.alpha + i0);
			d = *reinterpret_cast<const float4*>(p.depth + i0);
		}
	} else {
		g = make_float4(seed_load1(p.gt, i0, p.N, nan), seed_load1(p.gt, i0 + 1, p.N, nan), seed_load1(p.gt, i0 + 2, p.N, nan),
		                seed_load1(p.gt, i0 + 3, p.N, nan));
		a = make_float4(seed_load1(p.alpha, i0, p.N, 0.f), seed_load1(p.alpha, i0 + 1, p.N, 0.f), seed_load1(p.alpha, i0 + 2, p.N, 0.f),
		                seed_load1(p.alpha, i0 + 3, p.N, 0.f));
		d = make_float4(seed_load1(p.depth, i0, p.N, 0.f), seed_load1(p.depth, i0 + 1, p.N, 0.f), seed_load1(p.depth, i0 + 2, p.N, 0.f),
		                seed_load1(p.depth, i0 + 3, p.N, 0.f));
	}
	return SeedPixels{{g.x, g.y, g.z, g.w}, {a.x, a.y, a.z, a.w}, {d.x, d.y, d.z, d.w}};
}

__device__ __forceinline__ bool seed_valid(const SeedSelect& p, float g) { return g > p.min_depth && g < p.max_depth; }

__device__ __forceinline__ float seed_threshold(const SeedSelect& p)
{
	return p.rule == 2 ? fmaxf(p.err_abs, p.err_factor * __uint_as_float(p.state->prefix)) : p.err_abs;
}

__device__ __forceinline__ uint32_t seed_flags(const SeedSelect& p, int i, float g, float a, float d, float T)
{
	if (!seed_valid(p, g)) return 0u;
	if (p.stride > 1) {
		const int v = i / p.width, u = i - v * p.width;
		if (u % p.stride != p.offset_x || v % p.stride != p.offset_y) return SF_VALID;
	}
	const bool unseen = a < p.alpha_threshold;
	const bool in_front = p.rule != 0 && d > g && fabsf(g - d) > T;
	if (unseen) return SF_VALID | SF_SEL | SF_UNSEEN;
	if (in_front) return SF_VALID | SF_SEL | SF_DEPTH;
	return SF_VALID;
}

__global__ void __launch_bounds__(SEED_BLOCK)
seed_hist_kernel(const SeedSelect p, int ntiles, int pass)
{
	__shared__ uint32_t s_hist[256];
	s_hist[threadIdx.x] = 0u;
	__syncthreads();
	const int shift = 24 - 8 * pass;
	const uint32_t prefix = pass ? p.state->prefix : 0u;
	for (int tile = (int)blockIdx.x; tile < ntiles; tile += (int)gridDim.x) {
		const SeedPixels px = seed_load(p, tile * SEED_TILE + 4 * (int)threadIdx.x);
#pragma unroll
		for (int j = 0; j < 4; j++) {
			const uint32_t key = __float_as_uint(fabsf(px.g[j] - px.d[j]));
			// (pass 0: every valid pixel; later: those whose bits above the digit equal the prefix -- shift + 8 <= 24 there)
			const bool active = seed_valid(p, px.g[j]) && (pass == 0 || (key >> (shift + 8)) == prefix);
			if (active) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
		}
	}
	__syncthreads();
	p.blk_hist[(size_t)blockIdx.x * 256 + threadIdx.x] = s_hist[threadIdx.x];
}

// thread = bin.  nblocks histograms summed in workgroup order; the bin whose range of ranks holds k extends the prefix.
__global__ void __launch_bounds__(256)
seed_pick_kernel(const SeedSelect p, int nblocks, int pass)
{
	__shared__ uint32_t s_wave[4];
	uint32_t sum = 0;
	for (int b = 0; b < nblocks; b++) sum += p.blk_hist[(size_t)b * 256 + threadIdx.x];
	const uint32_t prefix = pass ? p.state->prefix : 0u;
	const uint32_t k_in = pass ? p.state->k : 0u;
	uint32_t total;
	const uint32_t excl = block_excl_scan_256(sum, &total, s_wave);   // (its barriers stand between the reads above and the writes below)
	const uint32_t k = pass ? k_in : (total ? (total - 1u) / 2u : 0u);
	if (total == 0u) {   // no valid pixel: the median's bits stay 0
		if (threadIdx.x == 0) {
			p.state->prefix = 0u;
			p.state->k = 0u;
			if (pass == 0) p.state->n_valid = 0u;
		}
		return;
	}
	if (pass == 0 && threadIdx.x == 0) p.state->n_valid = total;
	if (sum != 0u && excl <= k && k - excl < sum) {
		p.state->prefix = (prefix << 8) | threadIdx.x;
		p.state->k = k - excl;
	}
}

__global__ void __launch_bounds__(SEED_BLOCK)
seed_count_kernel(const SeedSelect p, int ntiles)
{
	__shared__ uint32_t s_cnt[SEED_BLOCK / 64][2];
	const float T = seed_threshold(p);
	const int i0 = (int)blockIdx.x * SEED_TILE + 4 * (int)threadIdx.x;
	const SeedPixels px = seed_load(p, i0);
	// four counters of at most 1024 per tile: two to a word
	uint32_t c01 = 0, c23 = 0;
#pragma unroll
	for (int j = 0; j < 4; j++) {
		const uint32_t f = seed_flags(p, i0 + j, px.g[j], px.a[j], px.d[j], T);
		c01 += ((f & SF_SEL) ? 1u : 0u) + ((f & SF_UNSEEN) ? 0x10000u : 0u);
		c23 += ((f & SF_DEPTH) ? 1u : 0u) + ((f & SF_VALID) ? 0x10000u : 0u);
	}
	c01 = wave_sum_u32(c01);
	c23 = wave_sum_u32(c23);
	if (lane_id() == 0) {
		s_cnt[wave_id()][0] = c01;
		s_cnt[wave_id()][1] = c23;
	}
	__syncthreads();
	if (threadIdx.x < 2) {
		uint32_t t = 0;
		for (int k = 0; k < SEED_BLOCK / 64; k++) t += s_cnt[k][threadIdx.x];
		p.tile_counts[(size_t)(2 * threadIdx.x) * ntiles + blockIdx.x] = t & 0xFFFFu;
		p.tile_counts[(size_t)(2 * threadIdx.x + 1) * ntiles + blockIdx.x] = t >> 16;
	}
}

// exclusive scan of the selected counts over the tiles, totals of all four (one workgroup; the loop of densify_spine_kernel)
__global__ void __launch_bounds__(1024)
seed_spine_kernel(const SeedSelect p, int ntiles, int* __restrict__ counts)
{
	__shared__ uint32_t s_wave[16];
	__shared__ uint32_t s_carry;
	__shared__ uint32_t s_tot[4];
	for (int b = 0; b < 4; b++) {
		if (threadIdx.x == 0) s_carry = 0;
		__syncthreads();
		uint32_t* row = p.tile_counts + (size_t)b * ntiles;
		for (int base = 0; base < ntiles; base += 1024) {
			const int i = base + (int)threadIdx.x;
			const uint32_t v = i < ntiles ? row[i] : 0u;
			const uint32_t incl = wave_incl_scan_u32(v);
			if (lane_id() == 63) s_wave[wave_id()] = incl;
			__syncthreads();
			uint32_t off = s_carry;
			for (int k = 0; k < wave_id(); k++) off += s_wave[k];
			if (i < ntiles) row[i] = off + incl - v;
			__syncthreads();
			if (threadIdx.x == 1023) s_carry = off + incl;
			__syncthreads();
		}
		if (threadIdx.x == 0) s_tot[b] = s_carry;
		__syncthreads();
	}
	if (threadIdx.x == 0) {
		for (int b = 0; b < 4; b++) counts[b] = (int)s_tot[b];
		counts[4] = (p.rule == 2 && p.state->n_valid) ? (int)p.state->prefix : 0;
		counts[5] = 0;
		counts[6] = 0;
		counts[7] = 0;
	}
}

__global__ void __launch_bounds__(SEED_BLOCK)
seed_plan_kernel(const SeedSelect p)
{
	__shared__ uint32_t s_wave[SEED_BLOCK / 64];
	const float T = seed_threshold(p);
	const int i0 = (int)blockIdx.x * SEED_TILE + 4 * (int)threadIdx.x;
	const SeedPixels px = seed_load(p, i0);
	uint32_t sel = 0;
#pragma unroll
	for (int j = 0; j < 4; j++)
		if (seed_flags(p, i0 + j, px.g[j], px.a[j], px.d[j], T) & SF_SEL) sel |= 1u << j;
	uint32_t total;
	uint32_t rank = p.tile_counts[blockIdx.x] + block_excl_scan_256((uint32_t)__popcll((unsigned long long)sel), &total, s_wave);
#pragma unroll
	for (int j = 0; j < 4; j++)
		if (sel & (1u << j)) p.plan[rank++] = (uint32_t)(i0 + j);   // (rank < counts[0] <= N; a selected pixel is < N)
}

struct SeedEmit {
	int width, n_plane;          // n_plane = width * height: the stride of the image's channels
	uint32_t n_selected, n_emit;
	int P;
	int row_floats[5];
	float* param[5];
	float* m1[5];
	float* m2[5];
	int* exist;
	int iteration;
	float* stats[3];
	int* out_pixel;
	const float* gt;
	const float* image;
	const float* vm;
	float fx, fy, cx, cy;
	float scale_mul;             // scale_factor * stride
	float opacity_logit;
	const uint32_t* plan;
	long long items_before[7];   // work items per destination row: t[0..4], statistics + exist + out_pixel, end
};

__global__ void __launch_bounds__(256)
seed_emit_kernel(const SeedEmit p)
{
	const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
	const long long per_row = p.items_before[6];
	const long long j = item / per_row;
	if (j >= (long long)p.n_emit) return;
	const long long e = item - j * per_row;
	// the rank written to row P + j: the last r with floor(r n_emit / n_selected) == j
	const unsigned long long r = ((unsigned long long)(j + 1) * p.n_selected + p.n_emit - 1ull) / p.n_emit - 1ull;
	const int pix = (int)p.plan[r];
	const size_t dst = (size_t)p.P + (size_t)j;
	if (e >= p.items_before[5]) {
		const int a = (int)(e - p.items_before[5]);
		if (a == 3) {
			if (p.exist) p.exist[dst] = p.iteration;
		} else if (a == 4) {
			if (p.out_pixel) p.out_pixel[j] = pix;
		} else if (p.stats[a]) {
			p.stats[a][dst] = 0.f;
		}
		return;
	}
	int ti = 0;
#pragma unroll
	for (int k = 1; k < 5; k++) ti += e >= p.items_before[k];
	const int u = (int)(e - p.items_before[ti]);
	const int rf = p.row_floats[ti];
	if ((rf & 3) == 0) {   // rows of whole float4s: features, rotation
		float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
		if (ti == 4) {
			val.x = 1.0f;
		} else if (u == 0 && p.image) {
			const float C0 = 0.28209479177387814f;   // RGB2SH with the float constant, as increasePcd
			val.x = (p.image[pix] - 0.5f) / C0;
			val.y = (p.image[(size_t)p.n_plane + pix] - 0.5f) / C0;
			val.z = (p.image[2 * (size_t)p.n_plane + pix] - 0.5f) / C0;
		}
		const size_t dn = dst * (size_t)(rf / 4) + u;
		reinterpret_cast<float4*>(p.param[ti])[dn] = val;
		if (p.m1[ti]) {
			const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
			reinterpret_cast<float4*>(p.m1[ti])[dn] = zero;
			reinterpret_cast<float4*>(p.m2[ti])[dn] = zero;
		}
		return;
	}
	float val = 0.f;
	if (ti == 0) {
		const int v = pix / p.width, uu = pix - v * p.width;
		const float z = p.gt[pix];
		const float d0 = (uu - p.cx) * z / p.fx - p.vm[12], d1 = (v - p.cy) * z / p.fy - p.vm[13], d2 = z - p.vm[14];
		val = p.vm[4 * u] * d0 + p.vm[4 * u + 1] * d1 + p.vm[4 * u + 2] * d2;
	} else if (ti == 1) {   // an SH row that is no multiple of four floats (M = 1): the DC term, then zeros
		if (u < 3 && p.image) val = (p.image[(size_t)u * p.n_plane + pix] - 0.5f) / 0.28209479177387814f;
	} else if (ti == 2) {
		val = p.opacity_logit;
	} else if (ti == 3) {
		val = logf(p.scale_mul * p.gt[pix] / (0.5f * (p.fx + p.fy)));
	} else {
		val = u == 0 ? 1.0f : 0.f;   // (a rotation row is always a float4; kept for completeness of the table)
	}
	const size_t dn = dst * (size_t)rf + u;
	p.param[ti][dn] = val;
	if (p.m1[ti]) {
		p.m1[ti][dn] = 0.f;
		p.m2[ti][dn] = 0.f;
	}
}

static inline int seed_tiles(long long n) { return (int)((n + SEED_TILE - 1) / SEED_TILE); }

struct SeedScratch {
	SeedState* state;
	uint32_t* tile_counts;
	uint32_t* blk_hist;
	uint32_t* plan;
};
static inline SeedScratch seed_carve(char* scratch, long long n)
{
	Carver c(scratch);
	SeedScratch s;
	s.state = c.take<SeedState>(1);
	s.tile_counts = c.take<uint32_t>((size_t)4 * seed_tiles(n));
	s.blk_hist = c.take<uint32_t>((size_t)SEED_HIST_BLOCKS * 256);
	s.plan = c.take<uint32_t>((size_t)n);
	return s;
}

// ---------------------------------------------------------------------------------------------------------------------
// Mip-Splatting's 3-D smoothing filter from the keyframes that observe a Gaussian (include/gsr.h: gsr_filter3d_compute).
//
//   filter3d_kernel      : one Gaussian per lane, its mean in registers, a loop over the K cameras.  The camera index is
//                          wave-uniform and the array is const __restrict__: the 80 bytes of a camera arrive through scalar loads
//                          (s_load_dwordx16 + x4 in the ISA), once per wave and camera, not per lane.  The means are read once for all
//                          K cameras: 12 B in and 4 B out per Gaussian.  An observed Gaussian leaves sqrt(variance) T, T = its
//                          smallest sampling interval z / max(fx, fy); an unobserved one leaves F3D_UNOBSERVED (a negative number:
//                          every observed value is positive).  The grid is capped at F3D_MAX_BLOCKS workgroups that stride over
//                          the rows, and every workgroup leaves the largest T it saw in `block_max` with a plain store.
//   filter3d_fill_kernel : every workgroup takes the maximum of the (at most F3D_MAX_BLOCKS) entries and gives the unobserved rows
//                          of its stride sqrt(variance) times that -- upstream's rule; 0 when nothing is observed.
// T >= 0, so the maxima are taken on the bit patterns (the integer order of non-negative floats is their order): no float atomics,
// no order dependence -- the same inputs give the same bits.
constexpr int F3D_THREADS = 256;
constexpr int F3D_MAX_BLOCKS = 1024;
constexpr float F3D_UNOBSERVED = -1.0f;

__global__ void __launch_bounds__(F3D_THREADS)
filter3d_kernel(int P, const float* __restrict__ means3D, int K, const gsr_filter3d_camera* __restrict__ cams, float sqrt_variance,
                float* __restrict__ filter_3D, uint32_t* __restrict__ block_max)
{
	__shared__ uint32_t s_max[F3D_THREADS / 64];
	uint32_t t_max = 0u;   // bits of the largest T of an observed Gaussian of this thread
	// (every thread of the workgroup runs the same number of rounds: the wave maximum below needs whole waves)
	for (long long base = (long long)blockIdx.x * F3D_THREADS; base < (long long)P; base += (long long)gridDim.x * F3D_THREADS) {
		const long long i = base + threadIdx.x;
		if (i >= (long long)P) continue;
		const float px = means3D[3 * (size_t)i], py = means3D[3 * (size_t)i + 1], pz = means3D[3 * (size_t)i + 2];
		float T = 0.f;
		bool observed = false;
		for (int k = 0; k < K; k++) {
			const float* V = cams[k].viewmatrix;
			const float fx = cams[k].focal_x, fy = cams[k].focal_y, w = cams[k].width, h = cams[k].height;
			const float x = V[0] * px + V[4] * py + V[8] * pz + V[12];
			const float y = V[1] * px + V[5] * py + V[9] * pz + V[13];
			const float z = V[2] * px + V[6] * py + V[10] * pz + V[14];   // vz of preprocess_fwd_kernel: z > 0.2f is its near test
			const float u = (x / z) * fx + 0.5f * w;
			const float v = (y / z) * fy + 0.5f * h;
			const bool sees = z > 0.2f && u >= -0.15f * w && u <= 1.15f * w && v >= -0.15f * h && v <= 1.15f * h;
			const float t = z / fmaxf(fx, fy);
			if (sees) {
				T = observed ? fminf(T, t) : t;
				observed = true;
			}
		}
		filter_3D[i] = observed ? sqrt_variance * T : F3D_UNOBSERVED;
		if (observed && T > 0.f) {   // (a NaN or a negative T -- a caller's camera without a focal length -- never becomes the maximum)
			const uint32_t b = __float_as_uint(T);
			t_max = b > t_max ? b : t_max;
		}
	}
	const uint32_t w_max = wave_max_u32(t_max);
	if (lane_id() == 0) s_max[wave_id()] = w_max;
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t m = s_max[0];
#pragma unroll
		for (int k = 1; k < F3D_THREADS / 64; k++) m = s_max[k] > m ? s_max[k] : m;
		block_max[blockIdx.x] = m;
	}
}

__global__ void __launch_bounds__(F3D_THREADS)
filter3d_fill_kernel(int P, int n_blocks, const uint32_t* __restrict__ block_max, float sqrt_variance, float* __restrict__ filter_3D)
{
	__shared__ uint32_t s_max[F3D_THREADS / 64];
	uint32_t m = 0u;
	for (int b = (int)threadIdx.x; b < n_blocks; b += F3D_THREADS) m = block_max[b] > m ? block_max[b] : m;
	m = wave_max_u32(m);
	if (lane_id() == 0) s_max[wave_id()] = m;
	__syncthreads();
	m = s_max[0];
#pragma unroll
	for (int k = 1; k < F3D_THREADS / 64; k++) m = s_max[k] > m ? s_max[k] : m;
	const float fill = sqrt_variance * __uint_as_float(m);
	for (long long i = (long long)blockIdx.x * F3D_THREADS + threadIdx.x; i < (long long)P; i += (long long)gridDim.x * F3D_THREADS)
		if (filter_3D[i] < 0.f) filter_3D[i] = fill;
}

static inline int filter3d_blocks(int P)
{
	const int b = div_up(P, F3D_THREADS);
	return b < F3D_MAX_BLOCKS ? b : F3D_MAX_BLOCKS;
}

}  // namespace gsr

using namespace gsr;

extern "C" {

size_t gsr_filter3d_scratch_bytes(int P)
{
	(void)P;   // one word per workgroup of filter3d_kernel, whose grid is capped
	return (size_t)F3D_MAX_BLOCKS * sizeof(uint32_t);
}

int gsr_filter3d_compute(int P, const float* means3D, int K, const gsr_filter3d_camera* cameras, float variance, float* filter_3D,
                         char* scratch, void* stream_)
{
	if (P < 0 || K < 0 || !(variance >= 0.f) || !(variance <= FLT_MAX)) return GSR_ERR_INVALID_ARG;
	if (P == 0) return GSR_OK;
	if (!means3D || !filter_3D || !scratch || (K > 0 && !cameras) || (reinterpret_cast<uintptr_t>(scratch) & 3)) return GSR_ERR_INVALID_ARG;
	hipStream_t stream = (hipStream_t)stream_;
	const int blocks = filter3d_blocks(P);
	const float sqrt_variance = sqrtf(variance);
	uint32_t* block_max = reinterpret_cast<uint32_t*>(scratch);
	GSR_LAUNCH(filter3d_kernel, blocks, F3D_THREADS, stream, P, means3D, K, cameras, sqrt_variance, filter_3D, block_max);
	GSR_LAUNCH(filter3d_fill_kernel, blocks, F3D_THREADS, stream, P, blocks, (const uint32_t*)block_max, sqrt_variance, filter_3D);
	GSR_CHECK_LAUNCH();
	return GSR_OK;
}

size_t gsr_seed_scratch_bytes(int width, int height)
{
	const long long n = (width > 0 && height > 0) ? (long long)width * height : 0;
	return align_up(sizeof(SeedState), 128) + align_up((size_t)4 * seed_tiles(n) * sizeof(uint32_t), 128) +
	       align_up((size_t)SEED_HIST_BLOCKS * 256 * sizeof(uint32_t), 128) + align_up((size_t)n * sizeof(uint32_t), 128) + 256;
}

int gsr_seed_select(const gsr_seed_select_args* a, char* scratch, int* counts, void* stream_)
{
	if (!a || !counts || a->width < 0 || a->height < 0) return GSR_ERR_INVALID_ARG;
	if (a->stride < 1 || a->offset_x < 0 || a->offset_x >= a->stride || a->offset_y < 0 || a->offset_y >= a->stride) return GSR_ERR_INVALID_ARG;
	if ((a->alpha == nullptr) != (a->depth == nullptr)) return GSR_ERR_INVALID_ARG;
	hipStream_t stream = (hipStream_t)stream_;
	const long long n = (long long)a->width * a->height;
	if (n == 0) {
		GSR_HIP(hipMemsetAsync(counts, 0, 8 * sizeof(int), stream));
		return GSR_OK;
	}
	if (!scratch || !a->gt_depth) return GSR_ERR_INVALID_ARG;
	if (n > 0x7FFFFFFFll - SEED_TILE) return GSR_ERR_UNSUPPORTED;   // pixel indices are int32
	SeedSelect p;
	p.N = (int)n; p.width = a->width;
	p.alpha = a->alpha; p.depth = a->depth; p.gt = a->gt_depth;
	p.min_depth = a->min_depth; p.max_depth = a->max_depth; p.alpha_threshold = a->alpha_threshold;
	p.err_abs = a->depth_error_abs; p.err_factor = a->depth_error_median_factor;
	p.stride = a->stride; p.offset_x = a->offset_x; p.offset_y = a->offset_y;
	p.rule = a->depth_error_median_factor != 0.f ? 2 : (a->depth_error_abs != 0.f ? 1 : 0);
	p.vec = ((reinterpret_cast<uintptr_t>(a->alpha) | reinterpret_cast<uintptr_t>(a->depth) | reinterpret_cast<uintptr_t>(a->gt_depth)) & 15) == 0;
	const SeedScratch s = seed_carve(scratch, n);
	p.state = s.state; p.tile_counts = s.tile_counts; p.blk_hist = s.blk_hist; p.plan = s.plan;
	const int ntiles = seed_tiles(n);
	if (p.rule == 2) {
		const int hb = ntiles < SEED_HIST_BLOCKS ? ntiles : SEED_HIST_BLOCKS;
		for (int pass = 0; pass < 4; pass++) {
			GSR_LAUNCH(seed_hist_kernel, hb, SEED_BLOCK, stream, p, ntiles, pass);
			GSR_LAUNCH(seed_pick_kernel, 1, 256, stream, p, hb, pass);
		}
	}
	GSR_LAUNCH(seed_count_kernel, ntiles, SEED_BLOCK, stream, p, ntiles);
	GSR_LAUNCH(seed_spine_kernel, 1, 1024, stream, p, ntiles, counts);
	GSR_LAUNCH(seed_plan_kernel, ntiles, SEED_BLOCK, stream, p);
	GSR_CHECK_LAUNCH();
	return GSR_OK;
}

int gsr_seed_emit(const gsr_seed_emit_args* a, const char* scratch, void* stream_)
{
	if (!a || a->width < 0 || a->height < 0 || a->stride < 1 || a->P < 0) return GSR_ERR_INVALID_ARG;
	if (a->n_selected < 0 || a->n_emit < 0 || a->n_emit > a->n_selected) return GSR_ERR_INVALID_ARG;
	if (!(a->init_opacity > 0.f && a->init_opacity < 1.f)) return GSR_ERR_INVALID_ARG;
	const long long n = (long long)a->width * a->height;
	if (n == 0 || a->n_emit == 0) return GSR_OK;
	if (n > 0x7FFFFFFFll - SEED_TILE) return GSR_ERR_UNSUPPORTED;
	if (!scratch || !a->gt_depth || !a->viewmatrix || a->n_selected > n) return GSR_ERR_INVALID_ARG;
	static const int row_floats[5] = {3, 0, 1, 3, 4};
	SeedEmit p;
	p.width = a->width; p.n_plane = (int)n;
	p.n_selected = (uint32_t)a->n_selected; p.n_emit = (uint32_t)a->n_emit;
	p.P = a->P;
	int n_moments = 0;
	long long items = 0;
	for (int i = 0; i < 5; i++) {
		p.row_floats[i] = i == 1 ? a->features_row_floats : row_floats[i];
		if (p.row_floats[i] <= 0) return GSR_ERR_INVALID_ARG;
		p.param[i] = a->param[i]; p.m1[i] = a->exp_avg[i]; p.m2[i] = a->exp_avg_sq[i];
		if (!p.param[i]) return GSR_ERR_INVALID_ARG;
		n_moments += (p.m1[i] != nullptr) + (p.m2[i] != nullptr);
		if ((p.row_floats[i] & 3) == 0) {   // float4 rows need 16-byte aligned bases
			const uintptr_t m = reinterpret_cast<uintptr_t>(p.param[i]) | reinterpret_cast<uintptr_t>(p.m1[i]) | reinterpret_cast<uintptr_t>(p.m2[i]);
			if (m & 15) return GSR_ERR_UNSUPPORTED;
		}
		p.items_before[i] = items;
		items += (p.row_floats[i] & 3) == 0 ? p.row_floats[i] / 4 : p.row_floats[i];
	}
	if (n_moments != 0 && n_moments != 10) return GSR_ERR_INVALID_ARG;   // all ten moments or none
	p.items_before[5] = items;
	items += 5;   // the three statistics, exist_since_iter and out_pixel
	p.items_before[6] = items;
	p.exist = a->exist_since_iter; p.iteration = a->iteration;
	for (int k = 0; k < 3; k++) p.stats[k] = a->stats[k];
	p.out_pixel = a->out_pixel;
	p.gt = a->gt_depth; p.image = a->image; p.vm = a->viewmatrix;
	p.fx = a->fx; p.fy = a->fy; p.cx = a->cx; p.cy = a->cy;
	p.scale_mul = a->scale_factor * (float)a->stride;
	const double o = (double)a->init_opacity;
	p.opacity_logit = (float)log(o / (1.0 - o));
	p.plan = seed_carve(const_cast<char*>(scratch), n).plan;
	const long long blocks = ((long long)a->n_emit * items + 255) / 256;
	if (blocks > 0x7FFFFFFFll) return GSR_ERR_UNSUPPORTED;
	GSR_LAUNCH(seed_emit_kernel, (int)blocks, 256, (hipStream_t)stream_, p);
	GSR_CHECK_LAUNCH();
	return GSR_OK;
}

int gsr_transform_points(int P, const float* points, const float* transformmatrix, float* out_points, void* stream_)
{
	if (P < 0) return GSR_ERR_INVALID_ARG;
	if (P == 0) return GSR_OK;
	if (!points || !transformmatrix || !out_points) return GSR_ERR_INVALID_ARG;
	hipStream_t stream = (hipStream_t)stream_;
	GSR_LAUNCH(transform_points_kernel, div_up(P, 256), 256, stream, P, points, transformmatrix, out_points);
	GSR_CHECK_LAUNCH();
	return GSR_OK;
}

int gsr_scale_transform_points(int P, float scale, const float* points, const float* rots, const float* transformmatrix,
                               const uint8_t* mask, float* out_points, float* out_rots, int reference_rot_layout,
                               void* stream_)
{
	if (P < 0) return GSR_ERR_INVALID_ARG;
	if (P == 0) return GSR_OK;
	if (!points || !rots || !transformmatrix || !mask || !out_points || !out_rots) return GSR_ERR_INVALID_ARG;
	hipStream_t stream = (hipStream_t)stream_;
	GSR_LAUNCH(scale_transform_points_kernel, div_up(P, 256), 256, stream, P, scale, points, rots, transformmatrix, mask,
	           out_points, out_rots, reference_rot_layout);
	GSR_CHECK_LAUNCH();
	return GSR_OK;
}

int gsr_reproject_depth_pinhole(int P, int width, float fx, float fy, float cx, float cy, const float* depths,
                                const uint8_t* mask, float* out_points, void* stream_)
{
	if (P < 0 || width <= 0) return GSR_ERR_INVALID_ARG;
	if (P == 0) return GSR_OK;
	if (!depths || !mask || !out_points) return GSR_ERR_INVALID_ARG;
	hipStream_t stream = (hipStream_t)stream_;
	GSR_LAUNCH(reproject_depth_kernel, div_up(P, 256), 256, stream, P, width, fx, fy, cx, cy, depths, mask, out_points);
	GSR_CHECK_LAUNCH();
	return GSR_OK;
}

int gsr_neighborhood_depth_pinhole(int N, int width, float fx, float fy, float cx, float cy, float max_pixel_dist,
                                   const float* pixels, const uint8_t* has3D, const float* point3D, const float* colors,
                                   float* out_points, float* out_colors, void* stream_)
{
	if (N < 0 || width <= 0) return GSR_ERR_INVALID_ARG;
	if (N == 0) return GSR_OK;
	if (!pixels || !has3D || !point3D || !colors || !out_points || !out_colors) return GSR_ERR_INVALID_ARG;
	hipStream_t stream = (hipStream_t)stream_;
	GSR_LAUNCH(neighborhood_depth_kernel, div_up(N, 256), 256, stream, N, width, fx, fy, cx, cy, max_pixel_dist, pixels,
	           has3D, point3D, colors, out_points, out_colors);
	GSR_CHECK_LAUNCH();
	return GSR_OK;
}

}  // extern "C"
