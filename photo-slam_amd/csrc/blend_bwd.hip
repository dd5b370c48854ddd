// blend_bwd.hip -- backward of the alpha blend: per-pixel loss gradients -> per-instance
// gradients of colour, 2D mean, conic and opacity.  One wave per 16x8 half tile, two halves = one 128-thread workgroup per tile:
// lane l of wave h holds TWO pixels, (l & 7, 8h + (l >> 3)) in the half's left quad 2h and the pixel 8 columns to its right in
// its right quad 2h + 1 (the quads of the forward blend, blend.h, whose flags say which quads blend an entry).  Views with
// fewer tiles than keep the machine busy that way run the same kernel with one wave per 8x8 quad (four waves, 256 threads and
// 256-entry segments per tile; below, in front of the kernel).  What follows describes the half tiles.
//
// Per-pixel semantics are renderCUDA's backward (cuda_rasterizer/backward.cu:399-557): walk
// the tile list back to front starting at each pixel's last contributor, recompute alpha,
// un-blend T, and accumulate the nine partial derivatives.
//
// The reference issues nine global float atomics per contributing (pixel, Gaussian) pair
// (backward.cu:523-554).  Here there are none (see blend.h):
//   * entries behind the deepest last-contributor of the tile are never loaded; a segment of 128 list entries is staged once
//     per tile by all 128 threads, and only the entries the forward blend flagged as blended by some quad of the tile
//     (state.h: contrib); every half-tile wave then walks the union of the entries flagged for its two quads and evaluates,
//     per entry, only the flagged quad(s) -- a wave-uniform branch on the two flag bits;
//   * where both quads of a half blend an entry (three quarters of the quad visits at C3, 70 % at C2: tools/quad_pair_probe.py,
//     profiles/r07_a_*) the nine products of the lane's two pixels are summed in the lane and reduced ONCE: one butterfly and
//     one ds_add_f32 per (half tile, entry) instead of one per (quad, entry);
//   * the per-pair arithmetic is branch-free; 1/(1-alpha) is one v_rcp_f32 shared by the two
//     divisions of the reference;
//   * "everything behind entry j, dotted with the pixel's loss gradient" is ONE running scalar per pixel (below) instead of
//     the reference's three-channel accum_rec;
//   * the nine terms are summed across the wave's 64 lanes with a butterfly packed from the
//     top through v_permlane32_swap / v_permlane16_swap (wave64.h, 19 VALU) that leaves eight
//     totals in one register (one per 8-lane group) and the ninth as four row sums; ONE ds_add_f32
//     with twelve active lanes adds them to the tile's LDS accumulators, where the two halves
//     of a tile meet;
//   * the two mean2D terms are reduced as sum(dL_dG*G*dx), sum(dL_dG*G*dy); their conic
//     combination (backward.cu:539-546) is linear in them and applied once per Gaussian in
//     preprocess_bwd (partials.h);
//   * at the end of a segment of 128 list entries the workgroup writes every touched entry's
//     nine sums to that instance's private 48-byte slot with plain stores.
//
// The running scalar.  The reference keeps accum_rec = the colour blended BEHIND entry j, normalised by the transmittance
// there (A_{j+1}), and forms dL/dalpha_j = T_j (c_j - A_{j+1}) . dpix - T_final / (1 - alpha_j) (bg . dpix)
// (backward.cu:505-534).  With the un-normalised suffix S_{j+1} = sum_{k > j} c_k alpha_k T_k = T_{j+1} A_{j+1} and
// T_{j+1} = T_j (1 - alpha_j) this is   dL/dalpha_j = T_j (c_j . dpix) - B_{j+1} / (1 - alpha_j),
//   B_{j+1} = S_{j+1} . dpix + T_final (bg . dpix),     B_j = B_{j+1} + (c_j . dpix) alpha_j T_j,
// one scalar recurrence instead of three (six VALU per visit instead of eleven), no division by a small transmittance -- and a
// state that could be re-created at any list position from T before the position and the colour blended behind it.  (Round 6
// built that: the forward blend left both per pixel at every 256- / 1 024-entry boundary and the backward blend ran one workgroup
// per (tile, group of segments) -- parity green, -7 % of this kernel at 500 k @ 1200 x 680 and 2 M @ 640 x 480, nothing elsewhere,
// +4 us in the forward blend and 16 bytes per instance: removed, commit 2e10ed9, EXPERIMENTS.md R6.)
//
// DEPTH (gsr_backward_args.dL_ddepth / dL_dalpha): the depth map D = sum_j z_j alpha_j T_j is one more colour channel and the alpha
// map A = 1 - T_final moves only the start of the running scalar:
//   B_final = T_final (bg . dpix - dA),   B_j = B_{j+1} + (c_j . dpix + z_j dD) alpha_j T_j,
// and dL/dz_j = sum over the pixels of alpha_j T_j dD, a tenth sum.  It costs no LDS: z rides in the spare word s_rec[i][2].y and
// the tenth sum is accumulated in s_rec[i][2].z (zeroed at staging), reduced like the ninth -- row sums of 16 lanes, merged by four
// more lanes of the same ds_add_f32 -- and written to slot word [9].
//
// ABS (gsr_backward_args.dL_dmean2D_abs): the absolute screen-space gradients of AbsGS.  The mean2D pair above is reduced as
// sum(w dx), sum(w dy) and gets its conic per Gaussian; a sum of ABSOLUTE values does not factor that way, so it is formed here, per
// pixel: two more products per visit, |w (2 A' dx + B' dy)| and |w (B' dx + 2 C' dy)| with w = dL_dG G and the prescaled conic of
// s_rec (the positive constants -- opacity, ln 2 for the prescale, W/2 and H/2 -- factor out of the absolute value: preprocess_bwd),
// the two pixels of a lane summed in the lane, reduced like the ninth and tenth -- row sums, delivered by eight more lanes of the
// same ds_add_f32 -- and written to slot words [10], [11].  The colour-only form keeps the two sums in s_rec[i][2].w and .y: no
// LDS.  ABS x DEPTH needs four values for the three spare words: that instantiation alone carries s_absy (+ 4 bytes per entry:
// 11.9 / 23.8 KB, 13 / 6 workgroups per CU against 14 / 7).  An instantiation of its own: the kernels without it stay the same code.
//
#include "blend.h"
#include "kernels.h"
#include "variant.h"

namespace gsr {

// Two forms of one kernel, WAVES waves per tile:
//   WAVES == 2  wave h owns the tile's half h (rows 8h .. 8h+7): quads 2h and 2h+1, two pixels per lane (the header above);
//   WAVES == 4  wave q owns quad q, one pixel per lane: twice the waves for the same work -- the form for views whose half-tile
//               grid does not fill the machine (BlendBwdParams::half_tiles, chosen in gsr_api.hip: blend_bwd_half_tiles).
// A segment holds one list entry per thread (LDS 11.4 / 22.8 KB per workgroup of two / four waves: 7 waves per SIMD either way).

// One pixel of a lane: its position, loss gradient, last contributor and the backward state (T, B: file header).
struct BwdPixel {
	typedef float v2f __attribute__((vector_size(8)));
	v2f pxy, dprg;
	float dpb, T, B;
	float dD;   // DEPTH: the pixel's dL/ddepth
	uint32_t last;
};

// the instantiations that exist (variant.h): half tiles or quads, 2 x 2 x 2 = 8
constexpr bool blend_bwd_variant(int WAVES, bool DEPTH, bool ABS) { return WAVES == 2 || WAVES == 4; }
template <int WAVES, bool DEPTH, bool ABS = false>
__global__ void __launch_bounds__(64 * WAVES)
blend_bwd_kernel(const BlendBwdParams p)
{
	static_assert(WAVES == 2 || WAVES == 4, "half tiles or quads");
	constexpr bool PAIRS = WAVES == 2;          // two pixels per lane
	constexpr int BWD_THREADS = 64 * WAVES;
	constexpr int BWD_SEG = BWD_THREADS;        // list entries accumulated in LDS per segment; thread i stages entry i of the segment
	__shared__ float4 s_rec[BWD_SEG][3];   // per entry of the segment: (x, y, A', B') (C', opacity, r, g) (b, z, sum dL/dz, -)
	                                       // (DEPTH only: z and the tenth sum)
	__shared__ float s_acc[9][BWD_SEG];
	__shared__ float s_absy[ABS && DEPTH ? BWD_SEG : 1];   // ABS x DEPTH only: the one sum s_rec has no spare word for (file header)
	__shared__ uint32_t s_slot[BWD_SEG];
	__shared__ uint8_t s_flag[BWD_SEG];    // bit q: quad q of the tile blends the entry
	__shared__ uint32_t s_wmax[QUADS_PER_TILE];

	const int tile = tile_assignment((int)blockIdx.x, p.deal);
	if (tile >= p.tiles) return;
	const int tile_x = tile % p.grid_x, tile_y = tile / p.grid_x;
	const int w = (int)wave_uniform_u32((uint32_t)wave_id());   // scalar: the LDS record address is SGPR arithmetic
	const int qa = PAIRS ? 2 * w : w, qb = qa + 1;              // the wave's (left) quad and, in pairs, the right one
	const int l = lane_id(), tid = (int)threadIdx.x;
	typedef float v2f __attribute__((vector_size(8)));
	const uint2 range = p.ranges[tile];
	const size_t plane = (size_t)p.H * p.W;

	// lane l: pixel (l & 7, l >> 3) of quad qa (pixel a) and, in pairs, the pixel 8 columns to its right, in quad qb (pixel b)
	auto load_pixel = [&](int px, int py, BwdPixel& s) {
		const bool inside = px < p.W && py < p.H;
		const size_t pix = (size_t)py * p.W + px;
		s.pxy = (v2f){(float)px, (float)py};
		s.last = inside ? p.n_contrib[pix] : 0u;
		const float T_final = inside ? p.final_T[pix] : 0.f;
		float dpr = 0.f, dpg = 0.f, dpb = 0.f;
		if (inside) {
			dpr = p.dL_dpix[pix];
			dpg = p.dL_dpix[plane + pix];
			dpb = p.dL_dpix[2 * plane + pix];
		}
		s.dprg = (v2f){dpr, dpg};
		s.dpb = dpb;
		// the pixel's state behind its last contributor: T = the final transmittance, B = (everything blended behind, i.e. the
		// background) . dpix
		s.T = T_final;
		if constexpr (DEPTH) {   // (+ the alpha map's -dA: file header)
			s.dD = (inside && p.dL_ddepth) ? p.dL_ddepth[pix] : 0.f;
			const float dA = (inside && p.dL_dalpha) ? p.dL_dalpha[pix] : 0.f;
			s.B = T_final * ((p.bg[0] * dpr + p.bg[1] * dpg + p.bg[2] * dpb) - dA);
		} else {
			s.B = T_final * (p.bg[0] * dpr + p.bg[1] * dpg + p.bg[2] * dpb);
		}
	};
	const int pxa = tile_x * TILE + (qa & 1) * 8 + (l & 7), py = tile_y * TILE + (qa >> 1) * 8 + (l >> 3);
	BwdPixel A, Bp;
	load_pixel(pxa, py, A);
	if (PAIRS) load_pixel(pxa + 8, py, Bp);

	// entries at or behind s_wmax[q] touch no pixel of quad q; bmax: none of the tile
	const uint32_t wmax_a = wave_uniform_u32(wave_max_u32(A.last));
	const uint32_t wmax_b = PAIRS ? wave_uniform_u32(wave_max_u32(Bp.last)) : 0u;
	if (l == 0) {
		s_wmax[qa] = wmax_a;
		if (PAIRS) s_wmax[qb] = wmax_b;
	}
	__syncthreads();
	const uint32_t bmax = wave_uniform_u32(max(max(s_wmax[0], s_wmax[1]), max(s_wmax[2], s_wmax[3])));

	// lanes 0, 8, .., 56 deliver the eight packed totals, lanes 1, 17, 33, 49 the four row sums of the ninth
	// (wave_reduce9_swap_f32): one ds_add_f32 with twelve active lanes
	const bool red_ninth = (l & 15) == 1;
	const bool red_lane = ((l & 7) == 0) || red_ninth;
	const int red_off = (red_ninth ? 8 : wave_swap9_component(l)) * BWD_SEG;
	// DEPTH: lanes 2, 18, 34, 50 add the four row sums of the tenth to s_rec[entry][2].z (12 floats per entry)
	const bool red_tenth = DEPTH && (l & 15) == 2;
	float* const red_base = red_tenth ? &s_rec[0][2].z : &s_acc[0][0] + red_off;
	const int red_stride = red_tenth ? 12 : 1;
	// ABS: lanes 3, 19, 35, 51 add the four row sums of sum |g_p.x| to s_rec[entry][2].w, lanes 4, 20, 36, 52 those of sum |g_p.y| to
	// s_rec[entry][2].y (with DEPTH, where z sits there: to s_absy[entry])
	const bool red_ax = ABS && (l & 15) == 3, red_ay = ABS && (l & 15) == 4;
	float* const red_abs_base = red_ax ? &s_rec[0][2].w : (red_ay ? (DEPTH ? &s_absy[0] : &s_rec[0][2].y) : red_base);
	const int red_abs_stride = red_ax ? 12 : (red_ay ? (DEPTH ? 1 : 12) : red_stride);

	const int seg_first = (int)((bmax + BWD_SEG - 1) / BWD_SEG) - 1, seg_last = 0;
	// The segment's records are staged ONCE per tile, by all the workgroup's threads (thread i: list entry seg_lo + i), and only
	// for the entries some quad of the tile blended (the forward blend's flags: a quarter of the entries of a 1080p view, a tenth
	// at 640 x 480 with 2 M Gaussians).  The list entries and flags of the NEXT segment are asked for while this one is walked.
	auto seg_flags = [&](int seg_) -> uint32_t {
		const uint32_t e = (uint32_t)seg_ * BWD_SEG + (uint32_t)tid;
		uint32_t f = 0u;
		if (e < bmax) {
#pragma unroll
			for (int q = 0; q < QUADS_PER_TILE; q++)
				// (behind a quad's deepest last contributor the forward blend may not have walked: no flags were written there)
				if (e < s_wmax[q] && p.contrib[(size_t)q * p.contrib_stride + range.x + e] != 0) f |= 1u << q;
		}
		return f;
	};
	auto seg_gid = [&](int seg_) -> uint32_t {
		const uint32_t e = (uint32_t)seg_ * BWD_SEG + (uint32_t)tid;
		return e < bmax ? p.point_list[range.x + e] : 0u;
	};

	// The alpha test of one pixel.  `ok` = the lanes whose pixel blends the entry (okl: this lane's).  In pairs it is the AND of
	// three ballots of compares, a lane mask in an SGPR pair that the selects below take as their scalar operand (a ballot of the
	// combined predicate, carried across the pair's branches, costs a v_cndmask + v_cmp per test); with one pixel per lane the
	// plain predicate gives the shorter visit (one select less).
	struct Hit {
		v2f dxy;
		float G, alpha;
		unsigned long long ok;
		bool okl;
	};
	auto test = [](const BwdPixel& s, const float4 g0, const float4 g1, uint32_t pos) -> Hit {
		Hit h;
		h.dxy = (v2f){g0.x, g0.y} - s.pxy;
		const float dx = h.dxy[0], dy = h.dxy[1];
		const float pw = g0.z * dx * dx + g1.x * dy * dy + g0.w * dx * dy;
		h.G = __builtin_amdgcn_exp2f(pw);
		h.alpha = fminf(0.99f, g1.y * h.G);
		h.okl = (pos < s.last) && !(pw > 0.0f) && !(h.alpha < 1.0f / 255.0f);
		h.ok = PAIRS ? wave_ballot(pos < s.last) & wave_ballot(!(pw > 0.0f)) & wave_ballot(!(h.alpha < 1.0f / 255.0f)) : wave_ballot(h.okl);
		return h;
	};
	// ... and its gradient terms: the nine products of the pixel (order of the LDS accumulators below) and its state update.
	// Lanes whose pixel does not blend the entry contribute exact zeros and keep their state.  The per-Gaussian constants
	// (opacity, -1/2, W/2, H/2, the conic in the mean2D terms) are applied after the reduction (preprocess_bwd, partials.h);
	// pairs of products ride in v_pk_mul_f32.
	struct Terms {
		v2f c01, t, m56;
		float c3, t7, wG;
		float z9;   // DEPTH: alpha T dL/ddepth
		float ax, ay;   // ABS: |w G (2 A' dx + B' dy)|, |w G (B' dx + 2 C' dy)|
	};
	auto terms = [](BwdPixel& s, const Hit& h, const float4 g1, float gb, float gz, float a2, float bp) -> Terms {
		const float rinv = __builtin_amdgcn_rcpf(1.f - h.alpha);
		const float Tn = s.T * rinv;   // the transmittance in FRONT of this entry
		// dL/dalpha = T_j (c_j . dpix) - B_{j+1} / (1 - alpha_j)   (the running scalar: file header; DEPTH: z_j dD is one more channel)
		float cdp = g1.z * s.dprg[0] + g1.w * s.dprg[1] + gb * s.dpb;
		if constexpr (DEPTH) cdp += gz * s.dD;
		const float dL_dalpha = cdp * Tn - s.B * rinv;
		const float am = PAIRS ? mask_select0_f32(h.ok, h.alpha) : (h.okl ? h.alpha : 0.f);
		const float dLm = PAIRS ? mask_select0_f32(h.ok, dL_dalpha) : (h.okl ? dL_dalpha : 0.f);
		const float dcol = am * Tn;
		Terms r;
		r.wG = dLm * h.G;
		r.c01 = s.dprg * (v2f){dcol, dcol};
		r.t = h.dxy * (v2f){r.wG, r.wG};            // w dx, w dy
		r.m56 = h.dxy * (v2f){r.t[0], r.t[0]};      // w dx dx, w dx dy
		r.c3 = dcol * s.dpb;
		r.t7 = r.t[1] * h.dxy[1];                    // w dy dy
		if constexpr (DEPTH) r.z9 = dcol * s.dD;
		if constexpr (ABS) {   // a2 = 2 A', bp = B', g1.x = C': the pixel's own mean2D terms, before their signs can cancel
			r.ax = fabsf(r.wG * (a2 * h.dxy[0] + bp * h.dxy[1]));
			r.ay = fabsf(r.wG * (bp * h.dxy[0] + (g1.x + g1.x) * h.dxy[1]));
		}
		s.T = PAIRS ? mask_select_f32(h.ok, Tn, s.T) : (h.okl ? Tn : s.T);
		s.B += dcol * cdp;   // (dcol is zero where the entry is not blended)
		return r;
	};

	uint32_t flags_next = seg_first >= 0 ? seg_flags(seg_first) : 0u, gid_next = seg_first >= 0 ? seg_gid(seg_first) : 0u;
	for (int seg = seg_first; seg >= seg_last; seg--) {
		const uint32_t seg_lo = (uint32_t)seg * BWD_SEG;
		const uint32_t seg_hi = min(bmax, seg_lo + BWD_SEG);
		for (int i = tid; i < 9 * BWD_SEG; i += BWD_THREADS) (&s_acc[0][0])[i] = 0.f;
		{
			const uint32_t f = flags_next, gid = gid_next;
			uint32_t slot = 0xFFFFFFFFu;
			float4 q0 = make_float4(0.f, 0.f, 0.f, 0.f), q1 = q0, q2 = q0;
			float z = 0.f;
			if (f) {
				q0 = p.rec[3 * (size_t)gid + 0];
				q1 = p.rec[3 * (size_t)gid + 1];
				q2 = p.rec[3 * (size_t)gid + 2];
				if constexpr (DEPTH) z = p.depth[gid];
			}
			if (seg > seg_last) {   // (asked for in front of the wait for the records)
				flags_next = seg_flags(seg - 1);
				gid_next = seg_gid(seg - 1);
			}
			if (f) {
				s_rec[tid][0] = prescale_q0(q0);
				s_rec[tid][1] = make_float4(prescale_c(q1.x), q1.y, q1.z, q1.w);
				s_rec[tid][2].x = q2.x;
				if constexpr (DEPTH) s_rec[tid][2].y = z;
				const uint32_t rlo = __float_as_uint(q2.y), rhi = __float_as_uint(q2.z);
				const uint32_t minx = rlo & 0xFFFFu, miny = rlo >> 16, maxx = rhi & 0xFFFFu;
				slot = __float_as_uint(q2.w) + ((uint32_t)tile_y - miny) * (maxx - minx) + ((uint32_t)tile_x - minx);
			}
			s_slot[tid] = slot;
			s_flag[tid] = (uint8_t)f;
			if constexpr (DEPTH) s_rec[tid][2].z = 0.f;   // the tenth sum
			if constexpr (ABS) {                          // the two absolute sums
				s_rec[tid][2].w = 0.f;
				if constexpr (DEPTH) s_absy[tid] = 0.f;
				else s_rec[tid][2].y = 0.f;
			}
		}
		__syncthreads();

		for (int b = (int)((seg_hi - seg_lo - 1u) >> 6); b >= 0; b--) {
			const uint32_t fl = s_flag[b * 64 + l];
			// per quad of the half the entries of this batch it blends; the wave walks their union
			const unsigned long long ma = wave_ballot(((fl >> qa) & 1u) != 0u), mb = PAIRS ? wave_ballot(((fl >> qb) & 1u) != 0u) : 0ull;
			unsigned long long m = ma | mb;
			const int base = (int)seg_lo + b * 64;
			const float4(*rec_b)[3] = &s_rec[b * 64];
			while (m) {
				const int bit = 63 - __clzll((long long)m);
#ifdef GSR_EMU
				m &= ~(1ull << bit);
#else
				asm volatile("s_bitset0_b64 %0, %1" : "+s"(m) : "s"(bit));   // (one scalar instruction instead of shift + andn2)
#endif
				const uint32_t pos = (uint32_t)(base + bit);
				const float4 g0 = rec_b[bit][0];
				const float4 g1 = rec_b[bit][1];
				float gb, gz = 0.f;
				if constexpr (DEPTH) {
					const float2 bz = *reinterpret_cast<const float2*>(&rec_b[bit][2]);
					gb = bz.x;
					gz = bz.y;
				} else {
					gb = rec_b[bit][2].x;
				}
				// only the flagged quads of the pair are tested (wave-uniform branches on the two flag bits)
				const float a2 = ABS ? g0.z + g0.z : 0.f, bp = g0.w;
				Hit ha, hb;
				unsigned long long oka = 0ull, okb = 0ull;
				if ((ma >> bit) & 1ull) {
					ha = test(A, g0, g1, pos);
					oka = ha.ok;
				}
				if (PAIRS && ((mb >> bit) & 1ull)) {
					hb = test(Bp, g0, g1, pos);
					okb = hb.ok;
				}
				// order of the nine sums in the LDS accumulators: 0 colour r, 1 w dx, 2 w dx dx, 3 colour b, 4 colour g, 5 w dy,
				// 6 w dx dy, 7 w dy dy, 8 w -- chosen so that the halves of each packed product sit four apart: the
				// butterfly's first level then adds (v0, v4) + (v1, v5) and (v2, v6) + (v3, v7) as register pairs
				// without a move (wave_reduce9_swap_f32); the segment write-out below restores the slot order.
				// Where both pixels of the lane blend the entry their products are summed in the lane: ONE reduction per
				// (half tile, entry).
				Terms r;
				if (PAIRS && oka && okb) {
					const Terms ra = terms(A, ha, g1, gb, gz, a2, bp), rb = terms(Bp, hb, g1, gb, gz, a2, bp);
					r.c01 = ra.c01 + rb.c01;
					r.t = ra.t + rb.t;
					r.m56 = ra.m56 + rb.m56;
					r.c3 = ra.c3 + rb.c3;
					r.t7 = ra.t7 + rb.t7;
					r.wG = ra.wG + rb.wG;
					if constexpr (DEPTH) r.z9 = ra.z9 + rb.z9;
					if constexpr (ABS) {
						r.ax = ra.ax + rb.ax;
						r.ay = ra.ay + rb.ay;
					}
				} else if (oka) {
					r = terms(A, ha, g1, gb, gz, a2, bp);
				} else if (PAIRS && okb) {
					r = terms(Bp, hb, g1, gb, gz, a2, bp);
				} else {
					continue;   // wave-uniform
				}
				float v[9];
				v[0] = r.c01[0];
				v[4] = r.c01[1];
				v[1] = r.t[0];
				v[5] = r.t[1];
				v[2] = r.m56[0];
				v[6] = r.m56[1];
				v[3] = r.c3;
				v[7] = r.t7;
				v[8] = r.wG;
				float packed, ninth_row;
				if constexpr (ABS) {   // the two absolute sums (behind the tenth, with DEPTH) are reduced like the ninth: row sums,
				                       // delivered by further lanes of the same ds_add_f32
					constexpr int K = DEPTH ? 3 : 2;
					float e[K], e_row[K];
					if constexpr (DEPTH) e[0] = r.z9;
					e[K - 2] = r.ax;
					e[K - 1] = r.ay;
					wave_reduce9_rows_swap_f32<K>(v, e, packed, ninth_row, e_row);
					GSR_OPAQUE_F32(packed);
					GSR_OPAQUE_F32(ninth_row);
#pragma unroll
					for (int k = 0; k < K; k++) GSR_OPAQUE_F32(e_row[k]);
					float val = red_ninth ? ninth_row : packed;
					if constexpr (DEPTH) val = red_tenth ? e_row[0] : val;
					val = red_ax ? e_row[K - 2] : (red_ay ? e_row[K - 1] : val);
					if (red_lane || red_tenth || red_ax || red_ay) atomicAdd(red_abs_base + ((int)pos - (int)seg_lo) * red_abs_stride, val);
				} else if constexpr (DEPTH) {   // the tenth (dL/dz) is reduced like the ninth: row sums, four more lanes of the same ds_add_f32
					float v10[10];
#pragma unroll
					for (int c = 0; c < 9; c++) v10[c] = v[c];
					v10[9] = r.z9;
					float tenth_row;
					wave_reduce10_swap_f32(v10, packed, ninth_row, tenth_row);
					GSR_OPAQUE_F32(packed);
					GSR_OPAQUE_F32(ninth_row);
					GSR_OPAQUE_F32(tenth_row);
					if (red_lane || red_tenth)
						atomicAdd(red_base + ((int)pos - (int)seg_lo) * red_stride, red_tenth ? tenth_row : (red_ninth ? ninth_row : packed));
				} else {
					wave_reduce9_swap_f32(v, packed, ninth_row);
					GSR_OPAQUE_F32(packed);      // keep the last butterfly adds fused with their DPP moves (the compiler otherwise
					GSR_OPAQUE_F32(ninth_row);   // sinks them into the 12-lane branch as mov_dpp + add)
					if (red_lane) atomicAdd(&(&s_acc[0][0])[red_off + ((int)pos - (int)seg_lo)], red_ninth ? ninth_row : packed);
				}
			}
		}
		__syncthreads();

		// write every touched entry of the segment to its instance slot
		for (int i = tid; i < (int)(seg_hi - seg_lo); i += BWD_THREADS) {
			const uint32_t slot = s_slot[i];
			float any = 0.f;
#pragma unroll
			for (int c = 0; c < 9; c++) any += fabsf(s_acc[c][i]);
			if constexpr (DEPTH) any += fabsf(s_rec[i][2].z);
			float abs_x = 0.f, abs_y = 0.f;
			if constexpr (ABS) {   // (an entry whose only non-zero sums are these is touched too)
				abs_x = s_rec[i][2].w;
				abs_y = DEPTH ? s_absy[i] : s_rec[i][2].y;
				any += abs_x + abs_y;
			}
			if (slot != 0xFFFFFFFFu && any != 0.f) {   // untouched / all-zero entries stay unflagged: the per-Gaussian sum skips them
				p.touched[slot] = 1;
				float4* dst = reinterpret_cast<float4*>(p.partials + (size_t)slot * (4 * SLOT_F4));
				// slot order (partials.h): colour r g b, w dx, w dy, w dx dx, w dx dy, w dy dy, w
				dst[0] = make_float4(s_acc[0][i], s_acc[4][i], s_acc[3][i], s_acc[1][i]);
				dst[1] = make_float4(s_acc[5][i], s_acc[2][i], s_acc[6][i], s_acc[7][i]);
				if constexpr (ABS) dst[2] = make_float4(s_acc[8][i], DEPTH ? s_rec[i][2].z : 0.f, abs_x, abs_y);   // + [10], [11]: the absolute sums
				else if constexpr (DEPTH) *reinterpret_cast<float2*>(dst + 2) = make_float2(s_acc[8][i], s_rec[i][2].z);   // + [9] dL/dz
				else reinterpret_cast<float*>(dst + 2)[0] = s_acc[8][i];
			}
		}
		if (seg > seg_last) __syncthreads();
	}
}

int launch_blend_bwd(const BlendBwdParams& p, hipStream_t stream)
{
	const bool depth = p.dL_ddepth || p.dL_dalpha;
	if (depth && !p.depth) return GSR_ERR_INVALID_ARG;
	const int st = with_int<2, 4>([&](auto waves) {
		return with_flags([&](auto dp, auto ab) -> int {
			constexpr int WAVES = decltype(waves)::value;
			constexpr bool DEPTH = decltype(dp)::value, ABS = decltype(ab)::value, EXISTS = blend_bwd_variant(WAVES, DEPTH, ABS);
			if constexpr (EXISTS) GSR_LAUNCH((blend_bwd_kernel<WAVES, DEPTH, ABS>), tile_grid(p.deal), 64 * WAVES, stream, p);
			return EXISTS ? GSR_OK : GSR_ERR_UNSUPPORTED;
		}, depth, p.abs_sums != 0);
	}, p.half_tiles ? 2 : 4, GSR_ERR_UNSUPPORTED);
	if (st != GSR_OK) return st;
	GSR_CHECK_LAUNCH();
	return GSR_OK;
}

}  // namespace gsr
