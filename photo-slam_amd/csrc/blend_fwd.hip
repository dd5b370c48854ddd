// blend_fwd.hip -- forward alpha blending, one wave per 8x8 pixel quad.
//
// Per-pixel semantics are renderCUDA's (cuda_rasterizer/forward.cu:261-374): walk the tile's
// depth-sorted list front to back, skip pairs with power > 0 or alpha < 1/255, stop a pixel
// once T*(1-alpha) < 1e-4 (that entry is not blended), write C + T*bg in CHW, final T and
// the index of the last contributor.
//
// Structure: see blend.h.  The per-pair arithmetic is branch-free (select instead of the
// reference's nested continues), the next batch's list entries are prefetched while the current
// batch is blended, and a wave leaves as soon as all its pixels are saturated.
//
// FWD_ONLY (GSR_FORWARD_ONLY, a render no backward pass follows): the same image from the same visits, without what only the
// backward pass reads -- no contribution flags per (quad, entry), no final T and last contributor per pixel, and no scalar
// bookkeeping of the flags (contrib_m) inside the visit loop.
//
// DEPTH (gsr_forward_args.out_depth / out_alpha, either form): the depth map sum_j z_j alpha_j T_j and the alpha map 1 - T from
// the same visits.  z_j, the view-space depth the lists are sorted by, is gathered at staging into the spare word of the LDS
// record; the visit adds ONE v_fmac under the same EXEC mask as the colour channels.
//
// CONTRIB (GSR_CONTRIBUTION, either form, with or without DEPTH): per-Gaussian contribution statistics.  A (quad, list entry) pair
// is visited exactly once, so the visit reduces wgt = [w(p)] alpha T over the lanes of upd_m to (sum, max, count of pixels with
// w != 0) -- a DPP sum, a max on the bit patterns (non-negative floats order like their bits), one s_bcnt1 -- and parks the
// triple in the registers of lane `bit`; at the end of the batch lane j stores entry j's triple to the entry's instance slot
// (blend.h: slot = first + (ty - miny) w + (tx - minx), quad q at [slot][q]) with plain stores, if any pixel counted.  Slots nobody
// writes were zeroed by the caller; contribution_reduce_kernel sums every Gaussian's run.  1 = all weights one, 2 = weight map.
#include "blend.h"
#include "kernels.h"
#include "variant.h"

namespace gsr {

// the instantiations that exist (variant.h): 2 x 2 x 3 = 12
constexpr bool blend_fwd_variant(bool FWD_ONLY, bool DEPTH, int CONTRIB) { return CONTRIB >= 0 && CONTRIB <= 2; }
template <bool FWD_ONLY, bool DEPTH, int CONTRIB = 0>
__global__ void __launch_bounds__(64)
blend_fwd_kernel(const BlendFwdParams p)
{
	__shared__ float4 s_rec[64][3];   // per staged entry: (x, y, A', B') (C', opacity, r, g) (b, z (DEPTH), -, -)

	int tile, quad;
	quad_assignment((int)blockIdx.x, p.deal, tile, quad);
	if (tile >= p.tiles) return;
	const int tile_x = tile % p.grid_x, tile_y = tile / p.grid_x;
	const int l = lane_id();
	const int qx0 = tile_x * TILE + (quad & 1) * 8, qy0 = tile_y * TILE + (quad >> 1) * 8;
	const int px = qx0 + (l & 7), py = qy0 + (l >> 3);
	const bool inside = px < p.W && py < p.H;
	const float pxf = (float)px, pyf = (float)py;
	const uint2 range = p.ranges[tile];
	const int n = (int)(range.y - range.x);

	float T = 1.0f;
	typedef float v2f __attribute__((vector_size(8)));
#ifdef GSR_EMU
	v2f Crg = {0.f, 0.f};
#else
	float Cr = 0.f, Cg = 0.f;
#endif
	float Cb = 0.f;
	float Cd = 0.f;   // DEPTH: sum z alpha T
	uint32_t last_contributor = 0;
	// pixel state predicates live as 64-bit lane masks in SGPR pairs; their logic is scalar
	unsigned long long done_m = wave_ballot(!inside);

	// CONTRIB: the pixel's weight, the lanes whose weight counts (one ballot per wave), and the triple of the entry this lane staged
	float wpix = 1.f;
	unsigned long long wnz_m = ~0ull;
	float acc_sum = 0.f;
	uint32_t acc_max = 0u, acc_cnt = 0u, my_slot = 0u;
	if constexpr (CONTRIB == 2) {
		wpix = inside ? p.pixel_weight[(size_t)py * p.W + px] : 0.f;
		wnz_m = wave_ballot(wpix != 0.f);
	}

	uint32_t gid_next = (l < n) ? p.point_list[range.x + (uint32_t)l] : 0u;
	for (int base = 0; base < n; base += 64) {
		if (~done_m == 0ull) break;
		const bool have = base + l < n;
		const uint32_t gid = gid_next;
		const int e_next = base + 64 + l;
		gid_next = (e_next < n) ? p.point_list[range.x + (uint32_t)e_next] : 0u;
		bool keep = false;
		if (have) {
			const float4 q0 = p.rec[3 * (size_t)gid + 0];
			const float4 q1 = p.rec[3 * (size_t)gid + 1];
			float cb;
			if constexpr (CONTRIB != 0) {
				const float4 q2 = p.rec[3 * (size_t)gid + 2];
				const uint32_t rmin = __float_as_uint(q2.y), rmax = __float_as_uint(q2.z);
				const uint32_t minx = rmin & 0xFFFFu, miny = rmin >> 16, maxx = rmax & 0xFFFFu;
				cb = q2.x;
				my_slot = __float_as_uint(q2.w) + ((uint32_t)tile_y - miny) * (maxx - minx) + ((uint32_t)tile_x - minx);
				acc_sum = 0.f; acc_max = 0u; acc_cnt = 0u;
			} else {
				cb = p.rec[3 * (size_t)gid + 2].x;
			}
			keep = quad_keep(q0, q1, (float)qx0, (float)qy0);
			s_rec[l][0] = prescale_q0(q0);
			s_rec[l][1] = make_float4(prescale_c(q1.x), q1.y, q1.z, q1.w);
			s_rec[l][2].x = cb;
			if constexpr (DEPTH) s_rec[l][2].y = p.depth[gid];
		}
		unsigned long long m = wave_ballot(keep);
		wave_fence();
		unsigned long long contrib_m = 0ull;   // entries of this batch that some pixel of the quad blends (scalar; training form only)
		// The visit loop is bound by VALU issue AND by scalar issue (one scalar unit serves the CU's four SIMDs: ~4 SIMD cycles
		// per scalar instruction against ~75 of VALU issue per visit; three more scalar instructions per visit cost 12 us per
		// launch): its control flow is one scalar mask, the surviving entries not yet visited, cleared bit by bit with
		// s_bitset0_b64 (the compiler's m &= m - 1 is three instructions) and tested once per iteration.
		while (m) {
			const int bit = __ffsll((long long)m) - 1;
#ifdef GSR_EMU
			m &= m - 1ull;
#else
			asm volatile("s_bitset0_b64 %0, %1" : "+s"(m) : "s"(bit));
#endif
			const float4 g0 = s_rec[bit][0];
			const float4 g1 = s_rec[bit][1];
			float gb, gz = 0.f;
			if constexpr (DEPTH) {
				const float2 bz = *reinterpret_cast<const float2*>(&s_rec[bit][2]);
				gb = bz.x;
				gz = bz.y;
			} else {
				gb = s_rec[bit][2].x;
			}
			const float dx = g0.x - pxf, dy = g0.y - pyf;
			const float pw = g0.z * dx * dx + g1.x * dy * dy + g0.w * dx * dy;   // log2(e) * power
			const float alpha = fminf(0.99f, g1.y * __builtin_amdgcn_exp2f(pw));
			const unsigned long long ok_m = wave_ballot(!(pw > 0.0f)) & wave_ballot(!(alpha < 1.0f / 255.0f)) & ~done_m;
			const float test_T = T * (1.f - alpha);
			const unsigned long long below_m = wave_ballot(test_T < 0.0001f);
			unsigned long long upd_m;
			if constexpr (FWD_ONLY) {
				upd_m = ok_m & ~below_m;   // (one s_andn2_b64: nobody wants the flags)
			} else {
#ifdef GSR_EMU
			upd_m = ok_m & ~below_m;
			if (upd_m) contrib_m |= 1ull << bit;
#else
			// upd_m = ok_m & ~below_m, and contrib_m |= upd_m ? 1 << bit : 0 off the SCC that s_andn2_b64 leaves (three scalar
			// instructions for both; the compiler's select form of the second alone takes five)
			asm volatile("s_andn2_b64 %[upd], %[ok], %[below]\n\ts_cbranch_scc0 1f\n\ts_bitset1_b64 %[c], %[bit]\n1:"
			             : [upd] "=&s"(upd_m), [c] "+s"(contrib_m) : [ok] "s"(ok_m), [below] "s"(below_m), [bit] "s"(bit) : "scc");
#endif
			}
			done_m |= ok_m & below_m;
			float cw = 0.f;   // CONTRIB: this lane's [w(p)] alpha T, formed before T moves on
			if constexpr (CONTRIB != 0) cw = alpha * T;
			if constexpr (CONTRIB == 2) cw *= wpix;
#ifdef GSR_EMU
			const float wgt = mask_select0_f32(upd_m, alpha * T);
			Crg += (v2f){g1.z, g1.w} * (v2f){wgt, wgt};
			Cb += gb * wgt;
			if constexpr (DEPTH) Cd += gz * wgt;
			T = mask_select_f32(upd_m, test_T, T);
			last_contributor = mask_select_u32(upd_m, (uint32_t)(base + bit + 1), last_contributor);
#else
			// The state of the pixels that blend this entry is updated UNDER EXEC = upd_m: three v_fmac and two v_mov (17 issue
			// cycles) instead of a multiply-by-select, a packed fma, and two selects each behind a v_mov (27 of the visit's 85);
			// costs two scalar instructions.
			{
				const float wgt = alpha * T;
				const uint32_t contributor = (uint32_t)(base + bit + 1);
				unsigned long long saved_exec;
				if constexpr (DEPTH) {   // (the same block with the depth channel's v_fmac)
				asm volatile("s_and_saveexec_b64 %[save], %[upd]\n\t"
				             "v_fmac_f32 %[cr], %[gr], %[w]\n\t"
				             "v_fmac_f32 %[cg], %[gg], %[w]\n\t"
				             "v_fmac_f32 %[cb], %[gbv], %[w]\n\t"
				             "v_fmac_f32 %[cd], %[gzv], %[w]\n\t"
				             "v_mov_b32 %[t], %[tt]\n\t"
				             "v_mov_b32 %[last], %[c]\n\t"
				             "s_mov_b64 exec, %[save]"
				             : [save] "=&s"(saved_exec), [cr] "+v"(Cr), [cg] "+v"(Cg), [cb] "+v"(Cb), [cd] "+v"(Cd), [t] "+v"(T),
				               [last] "+v"(last_contributor)
				             : [upd] "s"(upd_m), [gr] "v"(g1.z), [gg] "v"(g1.w), [gbv] "v"(gb), [gzv] "v"(gz), [w] "v"(wgt), [tt] "v"(test_T),
				               [c] "s"(contributor)
				             : "scc");
				} else {
				asm volatile("s_and_saveexec_b64 %[save], %[upd]\n\t"
				             "v_fmac_f32 %[cr], %[gr], %[w]\n\t"
				             "v_fmac_f32 %[cg], %[gg], %[w]\n\t"
				             "v_fmac_f32 %[cb], %[gbv], %[w]\n\t"
				             "v_mov_b32 %[t], %[tt]\n\t"
				             "v_mov_b32 %[last], %[c]\n\t"
				             "s_mov_b64 exec, %[save]"
				             : [save] "=&s"(saved_exec), [cr] "+v"(Cr), [cg] "+v"(Cg), [cb] "+v"(Cb), [t] "+v"(T), [last] "+v"(last_contributor)
				             : [upd] "s"(upd_m), [gr] "v"(g1.z), [gg] "v"(g1.w), [gbv] "v"(gb), [w] "v"(wgt), [tt] "v"(test_T), [c] "s"(contributor)
				             : "scc");
				}
			}
#endif
			if constexpr (CONTRIB != 0) {
				cw = mask_select0_f32(upd_m, cw);
				const float vsum = wave_readlane_f32(wave_sum_f32_lane63(cw), 63);
				const uint32_t vmax = wave_max_u32(__float_as_uint(cw));
				const uint32_t vcnt = (uint32_t)__popcll(CONTRIB == 2 ? (upd_m & wnz_m) : upd_m);
				const bool mine = l == bit;
				acc_sum = mine ? vsum : acc_sum;
				acc_max = mine ? vmax : acc_max;
				acc_cnt = mine ? vcnt : acc_cnt;
			}
			// (No test for "every pixel saturated" here: the rest of the batch then changes nothing -- ok_m excludes the saturated
			// pixels -- and is at most a few dozen visits once per quad; the test cost every visit two scalar instructions.
			// Tried and rejected: reading the NEXT entry's record from LDS while the current one is blended, unrolled by two so
			// that the register sets alternate -- 22 instead of 15 scalar instructions per visit, 0.212 instead of 0.188 ms.)
		}
		const bool wave_done = ~done_m == 0ull;
		// the backward pass walks the same batches: it visits only the entries flagged here (15 % of the entries that survive the
		// quad rejection blend into no pixel -- alpha below 1/255 at every pixel centre, or every such pixel saturated)
		if (!FWD_ONLY && have) p.contrib[(size_t)quad * p.contrib_stride + range.x + (uint32_t)(base + l)] = (uint8_t)((contrib_m >> l) & 1ull);
		if constexpr (CONTRIB != 0) {
			// (an entry no pixel of the quad counts keeps the zeros its slot was given; my_slot < R by construction, checked anyway)
			if (have && acc_cnt != 0u && my_slot < p.stats_slots) {
				float* dst = p.stats + ((size_t)my_slot * QUADS_PER_TILE + (size_t)quad) * CONTRIB_WORDS;
				dst[0] = acc_sum;
				dst[1] = __uint_as_float(acc_max);
				dst[2] = __uint_as_float(acc_cnt);
			}
		}
		if (wave_done) break;
		wave_fence();  // all lanes have read this batch before the next one overwrites the slice
	}
	if (inside) {
		const size_t pix = (size_t)py * p.W + px;
		const size_t plane = (size_t)p.H * p.W;
		if constexpr (!FWD_ONLY) {
			p.final_T[pix] = T;
			p.n_contrib[pix] = last_contributor;
		}
#ifdef GSR_EMU
		const float Cr = Crg[0], Cg = Crg[1];
#endif
		p.out_color[pix] = Cr + T * p.bg[0];
		p.out_color[plane + pix] = Cg + T * p.bg[1];
		p.out_color[2 * plane + pix] = Cb + T * p.bg[2];
		if constexpr (DEPTH) {
			if (p.out_depth) p.out_depth[pix] = Cd;
			if (p.out_alpha) p.out_alpha[pix] = 1.f - T;
		}
	}
}

// The per-Gaussian end of the contribution statistics: sum each Gaussian's contiguous run of instance slots in a fixed order --
// slots ascending, quads 0..3 inside a slot -- and write or accumulate the three outputs.  Lane = Gaussian for runs of up to
// LONG_RUN slots; a longer run (a screen-filling splat) is then summed by the whole wave, lane l the k = ceil(cnt / 64) consecutive
// slots [l k, (l + 1) k) and a fixed butterfly over the lanes, so that no lane walks thousands of slots alone (partials.h).  The
// order depends on the run's length alone: the same bits in both binning arrangements, whose first slots differ.
struct ContribTriple {
	float sum;
	uint32_t max, cnt;
};
__device__ __forceinline__ void contrib_add_slot(const float4* __restrict__ s4, ContribTriple& t)
{
	const float4 a = s4[0], b = s4[1], c = s4[2];   // (s0 m0 c0 s1) (m1 c1 s2 m2) (c2 s3 m3 c3)
	t.sum += a.x; t.sum += a.w; t.sum += b.z; t.sum += c.y;
	t.max = max(max(t.max, __float_as_uint(a.y)), max(__float_as_uint(b.x), max(__float_as_uint(b.w), __float_as_uint(c.z))));
	t.cnt += __float_as_uint(a.z) + __float_as_uint(b.y) + __float_as_uint(c.x) + __float_as_uint(c.w);
}

__global__ void __launch_bounds__(64)
contribution_reduce_kernel(const ContributionParams p)
{
	const int l = lane_id();
	const int idx = (int)blockIdx.x * 64 + l;
	const bool live = idx < p.P;
	uint32_t cnt = live ? p.tiles_touched[idx] : 0u;
	uint32_t first = cnt ? __float_as_uint(p.rec[3 * (size_t)idx + 2].w) : 0u;
	if ((unsigned long long)first + cnt > (unsigned long long)p.stats_slots) cnt = 0u;   // (cannot happen: the emission's own layout)
	const float4* s4 = reinterpret_cast<const float4*>(p.stats);
	ContribTriple t = {0.f, 0u, 0u};
	if (cnt <= LONG_RUN)
		for (uint32_t k = 0; k < cnt; k++) contrib_add_slot(s4 + 3 * (size_t)(first + k), t);
	unsigned long long long_m = wave_ballot(cnt > LONG_RUN);
	while (long_m) {
		const int src = __ffsll((long long)long_m) - 1;
		long_m &= long_m - 1ull;
		const uint32_t rf = wave_readlane_u32(first, src), rc = wave_readlane_u32(cnt, src);
		const uint32_t k = (rc + 63u) >> 6;
		const uint32_t lo = min(rc, (uint32_t)l * k), hi = min(rc, lo + k);
		ContribTriple u = {0.f, 0u, 0u};
		for (uint32_t j = lo; j < hi; j++) contrib_add_slot(s4 + 3 * (size_t)(rf + j), u);
		const float rs = wave_readlane_f32(wave_sum_f32_lane63(u.sum), 63);
		const uint32_t rm = wave_max_u32(u.max);
		const uint32_t rn = wave_sum_u32(u.cnt);
		if (l == src) { t.sum = rs; t.max = rm; t.cnt = rn; }
	}
	if (!live) return;
	const float vmax = __uint_as_float(t.max);
	if (p.accumulate) {
		if (p.out_sum) p.out_sum[idx] += t.sum;
		if (p.out_max) p.out_max[idx] = fmaxf(p.out_max[idx], vmax);
		if (p.out_cnt) p.out_cnt[idx] += (int)t.cnt;
	} else {
		if (p.out_sum) p.out_sum[idx] = t.sum;
		if (p.out_max) p.out_max[idx] = vmax;
		if (p.out_cnt) p.out_cnt[idx] = (int)t.cnt;
	}
}

int launch_contribution_reduce(const ContributionParams& p, hipStream_t stream)
{
	if (p.P <= 0) return GSR_OK;
	GSR_LAUNCH(contribution_reduce_kernel, div_up(p.P, 64), 64, stream, p);
	GSR_CHECK_LAUNCH();
	return GSR_OK;
}

int launch_blend_fwd(const BlendFwdParams& p, hipStream_t stream)
{
	const bool depth = p.out_depth || p.out_alpha;
	if (depth && !p.depth) return GSR_ERR_INVALID_ARG;
	const int st = with_int<0, 2>([&](auto contrib) {
		return with_flags([&](auto fo, auto dp) -> int {
			constexpr int CONTRIB = decltype(contrib)::value;
			constexpr bool FWD_ONLY = decltype(fo)::value, DEPTH = decltype(dp)::value, EXISTS = blend_fwd_variant(FWD_ONLY, DEPTH, CONTRIB);
			if constexpr (EXISTS) GSR_LAUNCH((blend_fwd_kernel<FWD_ONLY, DEPTH, CONTRIB>), quad_grid(p.deal), 64, stream, p);
			return EXISTS ? GSR_OK : GSR_ERR_UNSUPPORTED;
		}, p.forward_only != 0, depth);
	}, p.stats ? (p.pixel_weight ? 2 : 1) : 0, GSR_ERR_UNSUPPORTED);
	if (st != GSR_OK) return st;
	GSR_CHECK_LAUNCH();
	return GSR_OK;
}

}  // namespace gsr
