// densify.hip -- GaussianModel::densifyAndPrune / prunePoints as stream compaction.
//
// Reference: src/gaussian_model.cpp:588-815.  densifyAndClone appends the clones (cat), densifyAndSplit appends 2 children
// per selected Gaussian (cat) and prunes the parents (boolean-mask index of all six tensors + both Adam moments), the
// final prune masks everything again -- every tensor and moment is copied 4-6 times, each step syncs on a mask count,
// and emptyCache() drops the allocator blocks.  The RESULT is a pure function of per-Gaussian decisions:
//
//   new arrays = [ originals that are neither split nor pruned | clones that survive the prune |
//                  first children that survive | second children that survive ],   every block in source order
//
// (clones carry their source's opacity and scale, so they are pruned iff the source is; both children of a parent share
// its opacity and its scale / 1.6, so they survive or go together; max_radii2D is zeroed by densificationPostfix BEFORE the
// final prune, so the screen-size term of :808 never fires).  Hence:
//
//   gsr_densify_select : one pass over (accum, denom, scaling, opacity) -> five flags per Gaussian, block totals, a spine
//                        scan, and a second pass that ranks every flag with wave ballots (deterministic: no atomics) and
//                        writes the GATHER PLAN: for every row of the new arrays its source row and kind, for every
//                        surviving child its row in the [2k,3] normal-sample matrix.  Counts stay on the device; the host
//                        reads them once (it has to size the new tensors).
//   gsr_densify_gather : one launch rebuilds all five parameter tensors and their ten Adam moment tensors from the plan
//                        (rows copied once; new rows get zero moments), computes the children's positions
//                        R(q) * (z * exp(s)) + xyz and scales log(exp(s) / 1.6) in place of the copy, and zeroes the three
//                        statistics arrays.  708 B read + 708 B written per surviving Gaussian: HBM-bound.
//
// prunePoints(mask) is the same plan with keep = !mask and nothing else.
#include "kernels.h"
#include "wave64.h"

namespace gsr {

constexpr int DS_BLOCK = 256;
// flag bits
constexpr uint32_t F_KEEP = 1u, F_CLONE_KEPT = 2u, F_CHILD_KEPT = 4u, F_SPLIT = 8u, F_CLONE_SEL = 16u;

struct DensifySelect {
	int P;
	const float* accum;
	const float* denom;
	const float* scaling;        // [P,3] log-scales
	const float* opacity;        // [P] logits
	const uint8_t* prune_mask;   // non-null: prunePoints(mask) -- keep = !mask, nothing else
	float max_grad, min_opacity, thr_dense, thr_world;
	int use_world;               // max_screen_size != 0: also prune scale > 0.1 extent (:809)
};

// scale / (0.8 * N) of densifyAndSplit (:738) as ATen evaluates `tensor / 1.6` on the device (multiplication by the fp32
// reciprocal, BinaryDivTrueKernel.cu) resp. on the host (a true division)
__device__ __forceinline__ float child_scale(float s)
{
#ifdef GSR_EMU
	return s / 1.6f;
#else
	return s * (1.0f / 1.6f);
#endif
}

__device__ __forceinline__ uint32_t densify_flags(const DensifySelect& p, int i)
{
	if (p.prune_mask) return p.prune_mask[i] ? 0u : F_KEEP;
	// grads = accum / denom, nan -> 0 (:800-802)
	float g = p.accum[i] / p.denom[i];
	if (g != g) g = 0.f;
	const float s0 = expf(p.scaling[3 * (size_t)i + 0]), s1 = expf(p.scaling[3 * (size_t)i + 1]), s2 = expf(p.scaling[3 * (size_t)i + 2]);
	const float smax = fmaxf(fmaxf(s0, s1), s2);
	const bool big = smax > p.thr_dense;
	// densifyAndClone (:768-773): frobenius_norm over the last dimension of [P,1], i.e. |g| (ATen's norm kernel scales by the
	// maximum: no overflow / underflow of g*g for |g| outside 1e-19 .. 1.8e19); densifyAndSplit (:723-730): g itself
	const bool clone_sel = (fabsf(g) >= p.max_grad) && !big;
	const bool split_sel = (g >= p.max_grad) && big;
	// the final prune (:805-813) on the would-be rows
	const float op = 1.0f / (1.0f + expf(-p.opacity[i]));
	bool prune_self = op < p.min_opacity;
	bool prune_child = prune_self;
	if (p.use_world) {
		prune_self = prune_self || (smax > p.thr_world);
		// the children's activated scale is exp(log(s / 1.6)) (:738 stores the log, :809 activates it again)
		const float c = fmaxf(fmaxf(expf(logf(child_scale(s0))), expf(logf(child_scale(s1)))), expf(logf(child_scale(s2))));
		prune_child = prune_child || (c > p.thr_world);
	}
	uint32_t f = 0;
	if (!split_sel && !prune_self) f |= F_KEEP;
	if (clone_sel) f |= F_CLONE_SEL;
	if (clone_sel && !prune_self) f |= F_CLONE_KEPT;
	if (split_sel) f |= F_SPLIT;
	if (split_sel && !prune_child) f |= F_CHILD_KEPT;
	return f;
}

// pass 1: totals of the five flags per block of 256 Gaussians -> block_counts[5][nblocks]
__global__ void __launch_bounds__(DS_BLOCK)
densify_count_kernel(const DensifySelect p, uint32_t* __restrict__ block_counts, int nblocks)
{
	__shared__ uint32_t s_cnt[DS_BLOCK / 64][5];
	const int i = (int)blockIdx.x * DS_BLOCK + (int)threadIdx.x;
	const uint32_t f = i < p.P ? densify_flags(p, i) : 0u;
	const int w = wave_id();
#pragma unroll
	for (int b = 0; b < 5; b++) {
		const unsigned long long m = wave_ballot((f >> b) & 1u);
		if (lane_id() == 0) s_cnt[w][b] = (uint32_t)__popcll(m);
	}
	__syncthreads();
	if (threadIdx.x < 5) {
		uint32_t t = 0;
		for (int k = 0; k < DS_BLOCK / 64; k++) t += s_cnt[k][threadIdx.x];
		block_counts[(size_t)threadIdx.x * nblocks + blockIdx.x] = t;
	}
}

// pass 2: exclusive scan of every counter over the blocks (one workgroup; nblocks = P / 256), totals -> counts[0..4],
// counts[5] = rows of the new arrays
__global__ void __launch_bounds__(1024)
densify_spine_kernel(uint32_t* __restrict__ block_counts, int nblocks, int* __restrict__ counts)
{
	__shared__ uint32_t s_wave[16];
	__shared__ uint32_t s_carry;
	__shared__ uint32_t s_tot[5];
	for (int b = 0; b < 5; b++) {
		if (threadIdx.x == 0) s_carry = 0;
		__syncthreads();
		uint32_t* row = block_counts + (size_t)b * nblocks;
		for (int base = 0; base < nblocks; base += 1024) {
			const int i = base + (int)threadIdx.x;
			const uint32_t v = i < nblocks ? row[i] : 0u;
			const uint32_t incl = wave_incl_scan_u32(v);
			if (lane_id() == 63) s_wave[wave_id()] = incl;
			__syncthreads();
			uint32_t off = s_carry;
			for (int k = 0; k < wave_id(); k++) off += s_wave[k];
			if (i < nblocks) row[i] = off + incl - v;
			__syncthreads();
			if (threadIdx.x == 1023) s_carry = off + incl;
			__syncthreads();
		}
		if (threadIdx.x == 0) s_tot[b] = s_carry;
		__syncthreads();
	}
	if (threadIdx.x == 0) {
		for (int b = 0; b < 5; b++) counts[b] = (int)s_tot[b];
		counts[5] = (int)(s_tot[0] + s_tot[1] + 2u * s_tot[2]);
		counts[6] = 0;
		counts[7] = 0;
	}
}

// pass 3: ranks -> the gather plan.  src_of[row] = source | kind << 30 (0 kept original, 1 clone, 2 first child, 3 second
// child); child_sample[c] = row of child c (counted from the first child row) in the [2k,3] sample matrix: the reference
// draws samples for ALL selected parents, k = counts[3], parent-major within each copy (repeat({N,1}), :732-735).
__global__ void __launch_bounds__(DS_BLOCK)
densify_plan_kernel(const DensifySelect p, const uint32_t* __restrict__ block_offs, int nblocks, const int* __restrict__ counts,
                    uint32_t* __restrict__ src_of, uint32_t* __restrict__ child_sample)
{
	__shared__ uint32_t s_cnt[DS_BLOCK / 64][4];
	const int i = (int)blockIdx.x * DS_BLOCK + (int)threadIdx.x;
	const uint32_t f = i < p.P ? densify_flags(p, i) : 0u;
	const int w = wave_id();
	uint32_t rank[4];
#pragma unroll
	for (int b = 0; b < 4; b++) {
		const unsigned long long m = wave_ballot((f >> b) & 1u);
		rank[b] = (uint32_t)__popcll(m & lanemask_lt());
		if (lane_id() == 0) s_cnt[w][b] = (uint32_t)__popcll(m);
	}
	__syncthreads();
#pragma unroll
	for (int b = 0; b < 4; b++) {
		uint32_t off = block_offs[(size_t)b * nblocks + blockIdx.x];
		for (int k = 0; k < w; k++) off += s_cnt[k][b];
		rank[b] += off;
	}
	if (i >= p.P) return;
	const uint32_t n_keep = (uint32_t)counts[0], n_clone = (uint32_t)counts[1], n_child = (uint32_t)counts[2], k_split = (uint32_t)counts[3];
	if (f & F_KEEP) src_of[rank[0]] = (uint32_t)i;
	if (f & F_CLONE_KEPT) src_of[n_keep + rank[1]] = (uint32_t)i | (1u << 30);
	if (f & F_CHILD_KEPT) {
		const uint32_t c = rank[2];
		src_of[n_keep + n_clone + c] = (uint32_t)i | (2u << 30);
		src_of[n_keep + n_clone + n_child + c] = (uint32_t)i | (3u << 30);
		child_sample[c] = rank[3];
		child_sample[n_child + c] = k_split + rank[3];
	}
}

// ---------------------------------------------------------------------------------------------------------------------
// gather: one launch, work item = one 16-byte (or 4-byte) unit of one destination row of one tensor.  The five tensors are
// laid out as consecutive ranges of work items; each item copies parameter, exp_avg and exp_avg_sq.
struct GatherTensor {
	const float* src[3];   // parameter, exp_avg, exp_avg_sq (moments may be null: no optimizer state)
	float* dst[3];
	int row_floats;        // 3, 48, 1, 3, 4
};
struct DensifyGather {
	int n_new, n_first_child;     // rows; first row of the children block = n_keep + n_clone_kept
	const uint32_t* src_of;
	const uint32_t* child_sample;
	const uint32_t* row_perm;     // null, or: row r of the new set is row row_perm[r] of the plan (gsr_densify_gather_args.morton_scratch)
	const float* samples;         // [2k,3] standard normal draws (at::normal's randn before the scale), null if no children
	GatherTensor t[5];            // xyz, features, opacity, scaling, rotation
	float* stats[3];              // xyz_gradient_accum, denom, max_radii2D of the new set: zero-filled (may be null)
	const int* exist_in;          // exist_since_iter_ [P] (nullable, with exist_out): every new row inherits its source's value
	int* exist_out;               //   (prunePoints :636, densifyAndSplit :744, densifyAndClone :782)
	long long items_before[7];    // prefix sums of the work items: t[0..4], then the statistics (+ exist_since_iter), then the end
};

__device__ __forceinline__ void quat_rotate(const float* q, float sx, float sy, float sz, float& ox, float& oy, float& oz)
{
	// general_utils::build_rotation (include/general_utils.h:33-57) + bmm(R, s)
	const float norm = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
	const float r = q[0] / norm, x = q[1] / norm, y = q[2] / norm, z = q[3] / norm;
	const float R00 = 1.f - 2.f * (y * y + z * z), R01 = 2.f * (x * y - r * z), R02 = 2.f * (x * z + r * y);
	const float R10 = 2.f * (x * y + r * z), R11 = 1.f - 2.f * (x * x + z * z), R12 = 2.f * (y * z - r * x);
	const float R20 = 2.f * (x * z - r * y), R21 = 2.f * (y * z + r * x), R22 = 1.f - 2.f * (x * x + y * y);
	ox = R00 * sx + R01 * sy + R02 * sz;
	oy = R10 * sx + R11 * sy + R12 * sz;
	oz = R20 * sx + R21 * sy + R22 * sz;
}

__global__ void __launch_bounds__(256)
densify_gather_kernel(const DensifyGather p)
{
	const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
	if (item >= p.items_before[6]) return;
	if (item >= p.items_before[5]) {   // statistics of the new set start from zero (densificationPostfix :709-711)
		const long long e = item - p.items_before[5];
		const int a = (int)(e / p.n_new);
		const long long row = e - (long long)a * p.n_new;
		if (a == 3) {
			if (p.exist_out) p.exist_out[row] = p.exist_in[p.src_of[p.row_perm ? p.row_perm[row] : (uint32_t)row] & 0x3FFFFFFFu];
		} else if (p.stats[a]) {
			p.stats[a][row] = 0.f;
		}
		return;
	}
	int ti = 0;
#pragma unroll
	for (int k = 1; k < 5; k++) ti += item >= p.items_before[k];
	const GatherTensor& t = p.t[ti];
	const long long local = item - p.items_before[ti];
	const bool vec = (t.row_floats & 3) == 0;            // rows of whole float4s: features (12), rotation (1)
	const int units = vec ? t.row_floats / 4 : t.row_floats;
	const int row = (int)(local / units), u = (int)(local - (long long)row * units);
	const int prow = p.row_perm ? (int)p.row_perm[row] : row;   // the plan's row (its position decides a child's sample)
	const uint32_t code = p.src_of[prow];
	const uint32_t src = code & 0x3FFFFFFFu, kind = code >> 30;
	if (vec) {
		const size_t so = ((size_t)src * units + u), dn = ((size_t)row * units + u);
		reinterpret_cast<float4*>(t.dst[0])[dn] = reinterpret_cast<const float4*>(t.src[0])[so];
		const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
		if (t.dst[1]) reinterpret_cast<float4*>(t.dst[1])[dn] = kind ? zero : reinterpret_cast<const float4*>(t.src[1])[so];
		if (t.dst[2]) reinterpret_cast<float4*>(t.dst[2])[dn] = kind ? zero : reinterpret_cast<const float4*>(t.src[2])[so];
		return;
	}
	const size_t so = (size_t)src * units + u, dn = (size_t)row * units + u;
	float v = t.src[0][so];
	if (kind >= 2u && (ti == 0 || ti == 3)) {
		// a split child (:731-738): position sampled from the parent, scale / 1.6
		const float* ps = p.t[3].src[0] + 3 * (size_t)src;     // the parent's log-scales
		if (ti == 3) {
			v = logf(child_scale(expf(v)));
		} else {
			const float* z = p.samples + 3 * (size_t)p.child_sample[prow - p.n_first_child];
			// at::normal(mean 0, std): randn * std (+ 0)
			const float sx = z[0] * expf(ps[0]), sy = z[1] * expf(ps[1]), sz = z[2] * expf(ps[2]);
			float o[3];
			quat_rotate(p.t[4].src[0] + 4 * (size_t)src, sx, sy, sz, o[0], o[1], o[2]);
			v = o[u] + v;
		}
	}
	t.dst[0][dn] = v;
	if (t.dst[1]) t.dst[1][dn] = kind ? 0.f : t.src[1][so];
	if (t.dst[2]) t.dst[2][dn] = kind ? 0.f : t.src[2][so];
}

// the position every row of the plan is ordered by: its source's (a child: its parent's)
__global__ void __launch_bounds__(256)
densify_plan_positions_kernel(int n_new, const uint32_t* __restrict__ src_of, const float* __restrict__ xyz, float* __restrict__ pos)
{
	const int r = (int)blockIdx.x * 256 + (int)threadIdx.x;
	if (r >= n_new) return;
	const size_t s = (size_t)(src_of[r] & 0x3FFFFFFFu);
	pos[3 * (size_t)r] = xyz[3 * s];
	pos[3 * (size_t)r + 1] = xyz[3 * s + 1];
	pos[3 * (size_t)r + 2] = xyz[3 * s + 2];
}

static inline int densify_blocks(int P) { return div_up(P, DS_BLOCK); }

// ---------------------------------------------------------------------------------------------------------------------
// 3DGS-MCMC relocation / growth (include/gsr.h).  Sampling in proportion to opacity is made exact and order-independent by
// integer weights w = lrintf(o * 2^24) and their uint64 prefix C: a draw's source is a binary search in C.
//
//   mcmc_weight_kernel : o, dead flag, w per row; block totals of w (uint64) and of the dead flags
//   mcmc_spine_kernel  : exclusive scan of both over the blocks (one workgroup, chunks of 1024 as densify_spine_kernel),
//                        counts[0] = dead rows, counts[1] = destinations
//   mcmc_prefix_kernel : C per row; the dead rows ranked with ballots -> dest_of[k] (as densify_plan_kernel ranks its flags)
//   mcmc_sample_kernel : one thread per destination: t, binary search, src_of[k]; draws per source counted with an integer
//                        atomicAdd (the totals do not depend on the order)
//   mcmc_source_kernel : every source with N > 1: o', D in double, opacity and scale rewritten, its moments zeroed
//   mcmc_move_kernel   : one work item per unit of a destination row: copies xyz / SH / rotation and the source's NEW opacity
//                        and scale (destinations and sources are disjoint: relocating, dead rows have weight 0; growing, the
//                        destinations are rows >= P), zero moments and statistics, exist_since_iter of the source
//   mcmc_finish_kernel : counts[2], counts[3] from the per-block results of mcmc_source_kernel
constexpr int MCMC_NMAX = 51;

struct McmcBinom {
	double c[MCMC_NMAX][MCMC_NMAX];   // c[n][k] = C(n, k), n < 51: exact in double (C(50,25) = 1.26e14 < 2^53)
};
constexpr McmcBinom mcmc_make_binom()
{
	McmcBinom b{};
	for (int n = 0; n < MCMC_NMAX; n++) {
		b.c[n][0] = 1.0;
		for (int k = 1; k <= n; k++) b.c[n][k] = b.c[n - 1][k - 1] + (k <= n - 1 ? b.c[n - 1][k] : 0.0);
	}
	return b;
}
#ifdef GSR_EMU
static const McmcBinom mcmc_binom = mcmc_make_binom();
#else
__constant__ McmcBinom mcmc_binom = mcmc_make_binom();
#endif

struct McmcRelocate {
	int P, n_add, n_draws;
	float min_opacity;
	int row_floats[5];
	float* param[5];
	float* m1[5];
	float* m2[5];
	const float* draws;
	int* exist;
	float* stats[3];
	uint32_t* out_weights;
	// scratch
	uint32_t* w;           // [P]
	unsigned long long* C; // [P]
	uint32_t* cnt;         // [P] draws per source (zeroed by the host call)
	uint32_t* dest_of;     // [P] k-th dead row (relocating)
	uint32_t* src_of;      // [n_draws]
	unsigned long long* blk_w;   // [nblocks] block totals of w -> exclusive offsets
	uint32_t* blk_dead;    // [nblocks] likewise for the dead flags
	uint32_t* blk_nsrc;    // [nblocks] sources with N > 1
	uint32_t* blk_maxn;    // [nblocks] largest N
	long long items_before[7];   // work items of mcmc_move_kernel per destination row: t[0..4], statistics + exist, end
};

__device__ __forceinline__ float mcmc_opacity(float logit) { return 1.0f / (1.0f + expf(-logit)); }

__global__ void __launch_bounds__(DS_BLOCK)
mcmc_weight_kernel(const McmcRelocate p)
{
	__shared__ unsigned long long s_w[DS_BLOCK / 64];
	__shared__ uint32_t s_dead[DS_BLOCK / 64];
	const int i = (int)blockIdx.x * DS_BLOCK + (int)threadIdx.x;
	uint32_t w = 0;
	bool dead = false;
	if (i < p.P) {
		const float o = mcmc_opacity(p.param[2][i]);
		dead = o <= p.min_opacity;
		w = (dead && p.n_add == 0) ? 0u : (uint32_t)lrintf(o * 16777216.0f);
		p.w[i] = w;
		if (p.out_weights) p.out_weights[i] = w;
	}
	// 64 weights of at most 2^24: the wave's total fits 32 bits, the block's needs 33
	const uint32_t wsum = wave_sum_u32(w);
	const unsigned long long m = wave_ballot(dead);
	if (lane_id() == 0) {
		s_w[wave_id()] = wsum;
		s_dead[wave_id()] = (uint32_t)__popcll(m);
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		unsigned long long t = 0;
		uint32_t d = 0;
		for (int k = 0; k < DS_BLOCK / 64; k++) {
			t += s_w[k];
			d += s_dead[k];
		}
		p.blk_w[blockIdx.x] = t;
		p.blk_dead[blockIdx.x] = d;
	}
}

// exclusive scan over the blocks.  A block total of w is at most 2^32: it is scanned inside a wave as two 32-bit halves of 16
// and 17 bits (64 lanes: no overflow), and across the waves and the chunks in 64 bits.
__global__ void __launch_bounds__(1024)
mcmc_spine_kernel(const McmcRelocate p, int nblocks, int* __restrict__ counts)
{
	__shared__ unsigned long long s_wave_w[16];
	__shared__ uint32_t s_wave_d[16];
	__shared__ unsigned long long s_carry_w;
	__shared__ uint32_t s_carry_d;
	if (threadIdx.x == 0) {
		s_carry_w = 0;
		s_carry_d = 0;
	}
	__syncthreads();
	for (int base = 0; base < nblocks; base += 1024) {
		const int i = base + (int)threadIdx.x;
		const unsigned long long v = i < nblocks ? p.blk_w[i] : 0ull;
		const uint32_t d = i < nblocks ? p.blk_dead[i] : 0u;
		const uint32_t lo = wave_incl_scan_u32((uint32_t)(v & 0xFFFFull)), hi = wave_incl_scan_u32((uint32_t)(v >> 16));
		const unsigned long long incl_w = ((unsigned long long)hi << 16) + lo;
		const uint32_t incl_d = wave_incl_scan_u32(d);
		if (lane_id() == 63) {
			s_wave_w[wave_id()] = incl_w;
			s_wave_d[wave_id()] = incl_d;
		}
		__syncthreads();
		unsigned long long off_w = s_carry_w;
		uint32_t off_d = s_carry_d;
		for (int k = 0; k < wave_id(); k++) {
			off_w += s_wave_w[k];
			off_d += s_wave_d[k];
		}
		if (i < nblocks) {
			p.blk_w[i] = off_w + incl_w - v;
			p.blk_dead[i] = off_d + incl_d - d;
		}
		__syncthreads();
		if (threadIdx.x == 1023) {
			s_carry_w = off_w + incl_w;
			s_carry_d = off_d + incl_d;
		}
		__syncthreads();
	}
	if (threadIdx.x == 0) {
		const uint32_t dead = s_carry_d;
		uint32_t n_dest = p.n_add > 0 ? (uint32_t)p.n_add : min(dead, (uint32_t)p.n_draws);
		if (s_carry_w == 0) n_dest = 0;   // no weight anywhere: nothing moves
		counts[0] = (int)dead;
		counts[1] = (int)n_dest;
		for (int k = 2; k < 8; k++) counts[k] = 0;
	}
}

__global__ void __launch_bounds__(DS_BLOCK)
mcmc_prefix_kernel(const McmcRelocate p)
{
	__shared__ uint32_t s_w[DS_BLOCK / 64];
	__shared__ uint32_t s_dead[DS_BLOCK / 64];
	const int i = (int)blockIdx.x * DS_BLOCK + (int)threadIdx.x;
	const bool in = i < p.P;
	const uint32_t w = in ? p.w[i] : 0u;
	const bool dead = in && mcmc_opacity(p.param[2][i]) <= p.min_opacity;
	const uint32_t incl = wave_incl_scan_u32(w);
	const unsigned long long m = wave_ballot(dead);
	if (lane_id() == 63) s_w[wave_id()] = incl;
	if (lane_id() == 0) s_dead[wave_id()] = (uint32_t)__popcll(m);
	__syncthreads();
	unsigned long long off = p.blk_w[blockIdx.x];
	uint32_t rank = p.blk_dead[blockIdx.x] + (uint32_t)__popcll(m & lanemask_lt());
	for (int k = 0; k < wave_id(); k++) {
		off += s_w[k];
		rank += s_dead[k];
	}
	if (!in) return;
	p.C[i] = off + incl;
	if (dead && p.n_add == 0) p.dest_of[rank] = (uint32_t)i;
}

__global__ void __launch_bounds__(256)
mcmc_sample_kernel(const McmcRelocate p, const int* __restrict__ counts)
{
	const int k = (int)blockIdx.x * 256 + (int)threadIdx.x;
	if (k >= counts[1]) return;
	const unsigned long long total = p.C[p.P - 1];
	unsigned long long t = (unsigned long long)((double)p.draws[k] * (double)total);
	if (t > total - 1) t = total - 1;
	// the first s with C[s] > t (C[P-1] = total > t: it exists)
	int lo = 0, hi = p.P - 1;
	while (lo < hi) {
		const int mid = lo + ((hi - lo) >> 1);
		if (p.C[mid] > t) hi = mid; else lo = mid + 1;
	}
	p.src_of[k] = (uint32_t)lo;
	atomicAdd(&p.cnt[lo], 1u);
}

// o' and scale' of a source drawn n - 1 times (n >= 2), from its fp32 activated opacity: logit(o') and log(scale' / scale)
__device__ __forceinline__ void mcmc_new_values(float o_f, uint32_t n_draws_of, float min_opacity, float& new_logit, double& log_ratio)
{
	const int N = (int)min(n_draws_of, (uint32_t)MCMC_NMAX);
	const double o = (double)o_f;
	double on = 1.0 - pow(1.0 - o, 1.0 / (double)N);
	on = fmin(fmax(on, (double)min_opacity), 1.0 - 1.0 / 16777216.0);
	double D = 0.0;
	for (int i = 1; i <= N; i++) {
		double pw = on, sgn = 1.0;
		for (int k = 0; k < i; k++) {
			D += mcmc_binom.c[i - 1][k] * sgn * pw / sqrt((double)(k + 1));
			pw *= on;
			sgn = -sgn;
		}
	}
	new_logit = (float)log(on / (1.0 - on));
	log_ratio = log(o / D);
}

__global__ void __launch_bounds__(DS_BLOCK)
mcmc_source_kernel(const McmcRelocate p)
{
	__shared__ uint32_t s_n[DS_BLOCK / 64], s_max[DS_BLOCK / 64];
	const int i = (int)blockIdx.x * DS_BLOCK + (int)threadIdx.x;
	const uint32_t n = i < p.P ? p.cnt[i] + 1u : 0u;
	const bool src = n > 1u;
	if (src) {
		float nl;
		double lr;
		mcmc_new_values(mcmc_opacity(p.param[2][i]), n, p.min_opacity, nl, lr);
		p.param[2][i] = nl;
		float* s = p.param[3] + 3 * (size_t)i;
		// log(exp(s) * o / D) = s + log(o / D), summed in double and rounded once
		for (int c = 0; c < 3; c++) s[c] = (float)((double)s[c] + lr);
		if (p.m1[0]) {
			for (int t = 0; t < 5; t++) {
				float* a = p.m1[t] + (size_t)p.row_floats[t] * i;
				float* b = p.m2[t] + (size_t)p.row_floats[t] * i;
				for (int c = 0; c < p.row_floats[t]; c++) {
					a[c] = 0.f;
					b[c] = 0.f;
				}
			}
		}
	}
	const unsigned long long m = wave_ballot(src);
	const uint32_t mx = wave_max_u32(src ? n : 0u);
	if (lane_id() == 0) {
		s_n[wave_id()] = (uint32_t)__popcll(m);
		s_max[wave_id()] = mx;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t a = 0, b = 0;
		for (int k = 0; k < DS_BLOCK / 64; k++) {
			a += s_n[k];
			b = max(b, s_max[k]);
		}
		p.blk_nsrc[blockIdx.x] = a;
		p.blk_maxn[blockIdx.x] = b;
	}
}

__global__ void __launch_bounds__(256)
mcmc_move_kernel(const McmcRelocate p, const int* __restrict__ counts)
{
	const long long item = (long long)blockIdx.x * 256 + threadIdx.x;
	const long long per_row = p.items_before[6];
	const long long k = item / per_row;
	if (k >= (long long)counts[1]) return;
	const long long e = item - k * per_row;
	const size_t src = p.src_of[k];
	const size_t dst = p.n_add > 0 ? (size_t)p.P + (size_t)k : (size_t)p.dest_of[k];
	if (e >= p.items_before[5]) {
		const int a = (int)(e - p.items_before[5]);
		if (a == 3) {
			if (p.exist) p.exist[dst] = p.exist[src];
		} else if (p.stats[a]) {
			p.stats[a][dst] = 0.f;
		}
		return;
	}
	int ti = 0;
#pragma unroll
	for (int j = 1; j < 5; j++) ti += e >= p.items_before[j];
	const int u = (int)(e - p.items_before[ti]);
	const int rf = p.row_floats[ti];
	if ((rf & 3) == 0) {   // rows of whole float4s: features, rotation
		const int units = rf / 4;
		const size_t so = src * units + u, dn = dst * units + u;
		reinterpret_cast<float4*>(p.param[ti])[dn] = reinterpret_cast<const float4*>(p.param[ti])[so];
		if (p.m1[ti]) {
			const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
			reinterpret_cast<float4*>(p.m1[ti])[dn] = zero;
			reinterpret_cast<float4*>(p.m2[ti])[dn] = zero;
		}
		return;
	}
	const size_t so = src * rf + u, dn = dst * rf + u;
	p.param[ti][dn] = p.param[ti][so];
	if (p.m1[ti]) {
		p.m1[ti][dn] = 0.f;
		p.m2[ti][dn] = 0.f;
	}
}

__global__ void __launch_bounds__(256)
mcmc_finish_kernel(const McmcRelocate p, int nblocks, int* __restrict__ counts)
{
	__shared__ uint32_t s_n[4], s_max[4];
	uint32_t a = 0, b = 0;
	for (int i = (int)threadIdx.x; i < nblocks; i += 256) {
		a += p.blk_nsrc[i];
		b = max(b, p.blk_maxn[i]);
	}
	a = wave_sum_u32(a);
	b = wave_max_u32(b);
	if (lane_id() == 0) {
		s_n[wave_id()] = a;
		s_max[wave_id()] = b;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		counts[2] = (int)(s_n[0] + s_n[1] + s_n[2] + s_n[3]);
		counts[3] = (int)max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
	}
}

// The Langevin position noise (include/gsr.h: gsr_mcmc_add_noise).  One thread per Gaussian, 56 bytes read and 12 written; the
// fourteen loads are independent and stand in front of the first use.
__global__ void __launch_bounds__(256)
mcmc_noise_kernel(int P, float* __restrict__ xyz, const float* __restrict__ opacity, const float* __restrict__ scaling,
                  const float* __restrict__ rotation, const float* __restrict__ z, float noise_scale)
{
	const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
	if (i >= P) return;
	const size_t i3 = 3 * (size_t)i;
	const float px = xyz[i3], py = xyz[i3 + 1], pz = xyz[i3 + 2];
	const float zx = z[i3], zy = z[i3 + 1], zz = z[i3 + 2];
	const float lo = opacity[i];
	float c3[6];
	compute_cov3D(scaling, rotation, (size_t)i, 1.0f, GSR_RAW_SCALING | GSR_RAW_ROTATION, c3);
	const float o = mcmc_opacity(lo);
	// expf overflows to +inf for an opaque Gaussian: the quotient is then exactly 0
	const float g = 1.0f / (1.0f + expf(100.0f * (o - 0.005f)));
	const float f = g * noise_scale;
	const float vx = zx * f, vy = zy * f, vz = zz * f;
	xyz[i3] = px + (c3[0] * vx + c3[1] * vy + c3[2] * vz);
	xyz[i3 + 1] = py + (c3[1] * vx + c3[3] * vy + c3[4] * vz);
	xyz[i3 + 2] = pz + (c3[2] * vx + c3[4] * vy + c3[5] * vz);
}

static inline int mcmc_move_units(int row_floats) { return (row_floats & 3) == 0 ? row_floats / 4 : row_floats; }

// The densification statistics of one view from the absolute screen-space pair (gsr_backward_args.dL_dmean2D_abs, [P,2]): the
// arithmetic of densify_stats_kernel (train_ops.hip) on the norm of that pair.  It lives in this translation unit because it is
// built without FMA contraction like preprocess_bwd.hip, whose fused form (stat_* next to dL_dmean2D_abs) it has to match bit for bit.
__global__ void __launch_bounds__(256)
densify_stats_abs_kernel(int P, const float* __restrict__ abs2, const int* __restrict__ radii, float* __restrict__ accum,
                         float* __restrict__ denom, float* __restrict__ max_radii)
{
	const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
	if (i >= P) return;
	const int r = radii[i];
	if (r > 0) {
		const float gx = abs2[2 * (size_t)i], gy = abs2[2 * (size_t)i + 1];
		accum[i] += sqrtf(gx * gx + gy * gy);
		denom[i] += 1.0f;
		max_radii[i] = fmaxf(max_radii[i], (float)r);
	}
}

}  // namespace gsr

using namespace gsr;

extern "C" {

int gsr_densify_stats_abs(int P, const float* dL_dmean2D_abs, const int* radii, float* xyz_gradient_accum, float* denom,
                          float* max_radii2D, void* stream_)
{
	if (P < 0) return GSR_ERR_INVALID_ARG;
	if (P == 0) return GSR_OK;
	if (!dL_dmean2D_abs || !radii || !xyz_gradient_accum || !denom || !max_radii2D) return GSR_ERR_INVALID_ARG;
	hipStream_t stream = (hipStream_t)stream_;
	GSR_LAUNCH(densify_stats_abs_kernel, div_up(P, 256), 256, stream, P, dL_dmean2D_abs, radii, xyz_gradient_accum, denom, max_radii2D);
	GSR_CHECK_LAUNCH();
	return GSR_OK;
}

size_t gsr_densify_morton_scratch_bytes(int n_new) { return knn_scratch_bytes(n_new < 0 ? 0 : n_new); }

size_t gsr_densify_scratch_bytes(int P)
{
	if (P < 0) P = 0;
	// block counters [5][nblocks], src_of [2P] (the new set has at most P + P rows), child_sample [2P]
	return align_up((size_t)5 * densify_blocks(P) * sizeof(uint32_t), 128) + 2 * align_up((size_t)2 * P * sizeof(uint32_t), 128) + 256;
}

int gsr_densify_select(const gsr_densify_select_args* a, char* scratch, int* counts, void* stream_)
{
	if (!a || !counts || a->P < 0) return GSR_ERR_INVALID_ARG;
	hipStream_t stream = (hipStream_t)stream_;
	if (a->P == 0) {
		GSR_HIP(hipMemsetAsync(counts, 0, 8 * sizeof(int), stream));
		return GSR_OK;
	}
	if (!scratch) return GSR_ERR_INVALID_ARG;
	if (!a->prune_mask && (!a->xyz_gradient_accum || !a->denom || !a->scaling || !a->opacity)) return GSR_ERR_INVALID_ARG;
	DensifySelect p;
	p.P = a->P;
	p.accum = a->xyz_gradient_accum; p.denom = a->denom; p.scaling = a->scaling; p.opacity = a->opacity;
	p.prune_mask = a->prune_mask;
	p.max_grad = a->max_grad; p.min_opacity = a->min_opacity;
	p.thr_dense = a->percent_dense * a->extent;   // float products, as src/gaussian_model.cpp:729,772,809
	p.thr_world = 0.1f * a->extent;
	p.use_world = a->max_screen_size != 0;
	const int nb = densify_blocks(a->P);
	Carver c(scratch);
	uint32_t* block_counts = c.take<uint32_t>((size_t)5 * nb);
	uint32_t* src_of = c.take<uint32_t>((size_t)2 * a->P);
	uint32_t* child_sample = c.take<uint32_t>((size_t)2 * a->P);
	GSR_LAUNCH(densify_count_kernel, nb, DS_BLOCK, stream, p, block_counts, nb);
	GSR_LAUNCH(densify_spine_kernel, 1, 1024, stream, block_counts, nb, counts);
	GSR_LAUNCH(densify_plan_kernel, nb, DS_BLOCK, stream, p, (const uint32_t*)block_counts, nb, (const int*)counts, src_of,
	           child_sample);
	GSR_CHECK_LAUNCH();
	return GSR_OK;
}

int gsr_densify_gather(const gsr_densify_gather_args* a, const char* scratch, void* stream_)
{
	if (!a || a->P < 0 || a->n_new < 0 || a->n_keep < 0 || a->n_clone < 0 || a->n_child < 0 || a->n_split < 0) return GSR_ERR_INVALID_ARG;
	if ((long long)a->n_keep + a->n_clone + 2ll * a->n_child != a->n_new || a->n_new > 2ll * a->P) return GSR_ERR_INVALID_ARG;
	if (a->n_new == 0) return GSR_OK;
	if (!scratch || a->P == 0) return GSR_ERR_INVALID_ARG;
	if (a->n_child && !a->samples) return GSR_ERR_INVALID_ARG;
	static const int row_floats[5] = {3, 0, 1, 3, 4};
	DensifyGather p;
	p.n_new = a->n_new;
	p.n_first_child = a->n_keep + a->n_clone;
	Carver c(const_cast<char*>(scratch));
	const int nb = densify_blocks(a->P);
	(void)c.take<uint32_t>((size_t)5 * nb);
	p.src_of = c.take<uint32_t>((size_t)2 * a->P);
	p.child_sample = c.take<uint32_t>((size_t)2 * a->P);
	p.samples = a->samples;
	long long items = 0;
	for (int i = 0; i < 5; i++) {
		GatherTensor& t = p.t[i];
		t.row_floats = i == 1 ? a->features_row_floats : row_floats[i];
		if (t.row_floats <= 0) return GSR_ERR_INVALID_ARG;
		t.src[0] = a->param_in[i]; t.src[1] = a->exp_avg_in[i]; t.src[2] = a->exp_avg_sq_in[i];
		t.dst[0] = a->param_out[i]; t.dst[1] = a->exp_avg_out[i]; t.dst[2] = a->exp_avg_sq_out[i];
		if (!t.src[0] || !t.dst[0]) return GSR_ERR_INVALID_ARG;
		if ((t.src[1] == nullptr) != (t.dst[1] == nullptr) || (t.src[2] == nullptr) != (t.dst[2] == nullptr)) return GSR_ERR_INVALID_ARG;
		if ((t.row_floats & 3) == 0) {   // float4 rows need 16-byte aligned bases
			uintptr_t m = 0;
			for (int k = 0; k < 3; k++) m |= reinterpret_cast<uintptr_t>(t.src[k]) | reinterpret_cast<uintptr_t>(t.dst[k]);
			if (m & 15) return GSR_ERR_UNSUPPORTED;
		}
		p.items_before[i] = items;
		items += (long long)a->n_new * ((t.row_floats & 3) == 0 ? t.row_floats / 4 : t.row_floats);
	}
	p.items_before[5] = items;
	for (int k = 0; k < 3; k++) p.stats[k] = a->stats_out[k];
	if ((a->exist_since_iter_in == nullptr) != (a->exist_since_iter_out == nullptr)) return GSR_ERR_INVALID_ARG;
	p.exist_in = a->exist_since_iter_in; p.exist_out = a->exist_since_iter_out;
	items += 4ll * a->n_new;
	p.items_before[6] = items;
	const long long blocks = (items + 255) / 256;
	if (blocks > 0x7FFFFFFFll) return GSR_ERR_UNSUPPORTED;
	p.row_perm = nullptr;
	if (a->morton_scratch) {
		// the plan's rows along the Z-order curve of their sources' positions (the simple-knn front half: bounding box, Morton codes,
		// radix sort); the gather below then reads the plan through the permutation
		float* pos = morton_points_buffer(a->n_new, a->morton_scratch);
		GSR_LAUNCH(densify_plan_positions_kernel, div_up(a->n_new, 256), 256, (hipStream_t)stream_, a->n_new, p.src_of, a->param_in[0], pos);
		uint32_t* perm = nullptr;
		const int st = launch_morton_order(a->n_new, pos, &perm, a->morton_scratch, (hipStream_t)stream_);
		if (st != GSR_OK) return st;
		p.row_perm = perm;
	}

	GSR_LAUNCH(densify_gather_kernel, (int)blocks, 256, (hipStream_t)stream_, p);
	GSR_CHECK_LAUNCH();
	return GSR_OK;
}

size_t gsr_mcmc_scratch_bytes(int P, int n_draws)
{
	if (P < 0) P = 0;
	if (n_draws < 0) n_draws = 0;
	const size_t nb = (size_t)densify_blocks(P);
	// w, cnt, dest_of [P], C [P] (64-bit), src_of [n_draws], four per-block arrays (one of them 64-bit)
	return 3 * align_up((size_t)P * sizeof(uint32_t), 128) + align_up((size_t)P * sizeof(unsigned long long), 128) +
	       align_up((size_t)n_draws * sizeof(uint32_t), 128) + align_up(nb * sizeof(unsigned long long), 128) +
	       3 * align_up(nb * sizeof(uint32_t), 128) + 256;
}

int gsr_mcmc_relocate(const gsr_mcmc_relocate_args* a, char* scratch, int* counts, void* stream_)
{
	if (!a || !counts || a->P < 0 || a->n_add < 0 || a->n_draws < 0 || a->n_add > a->n_draws) return GSR_ERR_INVALID_ARG;
	if (!(a->min_opacity > 0.f && a->min_opacity < 1.f)) return GSR_ERR_INVALID_ARG;
	hipStream_t stream = (hipStream_t)stream_;
	if (a->P == 0) {
		GSR_HIP(hipMemsetAsync(counts, 0, 8 * sizeof(int), stream));
		return GSR_OK;
	}
	if (!scratch || (a->n_draws > 0 && !a->draws)) return GSR_ERR_INVALID_ARG;
	static const int row_floats[5] = {3, 0, 1, 3, 4};
	McmcRelocate p;
	p.P = a->P; p.n_add = a->n_add; p.n_draws = a->n_draws;
	p.min_opacity = a->min_opacity;
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
		items += mcmc_move_units(p.row_floats[i]);
	}
	if (n_moments != 0 && n_moments != 10) return GSR_ERR_INVALID_ARG;   // all ten moments or none
	p.items_before[5] = items;
	items += 4;   // the three statistics and exist_since_iter
	p.items_before[6] = items;
	p.draws = a->draws;
	p.exist = a->exist_since_iter;
	for (int k = 0; k < 3; k++) p.stats[k] = a->stats[k];
	p.out_weights = a->out_weights;
	const int nb = densify_blocks(a->P);
	Carver c(scratch);
	p.w = c.take<uint32_t>((size_t)a->P);
	p.cnt = c.take<uint32_t>((size_t)a->P);
	p.dest_of = c.take<uint32_t>((size_t)a->P);
	p.C = c.take<unsigned long long>((size_t)a->P);
	p.src_of = c.take<uint32_t>((size_t)a->n_draws);
	p.blk_w = c.take<unsigned long long>((size_t)nb);
	p.blk_dead = c.take<uint32_t>((size_t)nb);
	p.blk_nsrc = c.take<uint32_t>((size_t)nb);
	p.blk_maxn = c.take<uint32_t>((size_t)nb);
	// the most destinations there can be: every draw, and when relocating no more than the rows
	const int max_dest = a->n_add > 0 ? a->n_add : (a->n_draws < a->P ? a->n_draws : a->P);
	const long long move_blocks = ((long long)max_dest * items + 255) / 256;
	if (move_blocks > 0x7FFFFFFFll) return GSR_ERR_UNSUPPORTED;
	GSR_HIP(hipMemsetAsync(p.cnt, 0, (size_t)a->P * sizeof(uint32_t), stream));
	GSR_LAUNCH(mcmc_weight_kernel, nb, DS_BLOCK, stream, p);
	GSR_LAUNCH(mcmc_spine_kernel, 1, 1024, stream, p, nb, counts);
	GSR_LAUNCH(mcmc_prefix_kernel, nb, DS_BLOCK, stream, p);
	if (max_dest > 0) GSR_LAUNCH(mcmc_sample_kernel, div_up(max_dest, 256), 256, stream, p, (const int*)counts);
	GSR_LAUNCH(mcmc_source_kernel, nb, DS_BLOCK, stream, p);
	if (max_dest > 0) GSR_LAUNCH(mcmc_move_kernel, (int)move_blocks, 256, stream, p, (const int*)counts);
	GSR_LAUNCH(mcmc_finish_kernel, 1, 256, stream, p, nb, counts);
	GSR_CHECK_LAUNCH();
	return GSR_OK;
}

int gsr_mcmc_add_noise(int P, float* xyz, const float* opacity, const float* scaling, const float* rotation, const float* z,
                       float noise_scale, void* stream_)
{
	if (P < 0) return GSR_ERR_INVALID_ARG;
	if (P == 0) return GSR_OK;
	if (!xyz || !opacity || !scaling || !rotation || !z) return GSR_ERR_INVALID_ARG;
	if (reinterpret_cast<uintptr_t>(rotation) & 15) return GSR_ERR_UNSUPPORTED;   // read as float4 rows
	GSR_LAUNCH(mcmc_noise_kernel, div_up(P, 256), 256, (hipStream_t)stream_, P, xyz, opacity, scaling, rotation, z, noise_scale);
	GSR_CHECK_LAUNCH();
	return GSR_OK;
}

}  // extern "C"
