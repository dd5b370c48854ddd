// partials.h -- the per-Gaussian end of the atomic-free gradient hand-off (blend.h): sum a Gaussian's contiguous run of
// per-instance gradient slots, written and flagged by the backward blend, in a fixed order (bit-reproducible).
// Lane = Gaussian.  Runs of up to LONG_RUN (64) slots are summed by their owner lane -- 16 flag bytes per load, squeezed to a
// bit mask, then the TOUCHED slots only (about 1 in 5: the rest lie behind their tile's last contributor or blend into no
// pixel), two per trip.  Longer runs (screen-filling splats; listed by the forward pass) are summed beforehand by
// long_run_sums_kernel, one WAVE per run, which leaves the total in the run's first slot: wherever such Gaussians sit in the
// arrays -- densification appends the children of split Gaussians consecutively -- no wave of the backward preprocess inherits
// their work.
//   a[0..2] dL_dcolor   a[3], a[4] sum w dx, sum w dy   a[5..7] sum w dx dx, w dx dy, w dy dy   a[8] sum w
//   a[9] dL/dz (the depth / alpha maps' backward, blend_bwd.hip: DEPTH) -- carried by the forms over float[10] / DEPTH only
//   a[10], a[11] sum |w (2 A' dx + B' dy)|, sum |w (B' dx + 2 C' dy)| per pixel (blend_bwd.hip: ABS) -- carried by the forms over
//   float[12] / ABS only, which take words [8..11] as one 16-byte load (the ABS blend writes word [9] too, zero without DEPTH)
#pragma once
#include "state.h"
#include "wave64.h"

namespace gsr {

// U touched slots of a run in one trip: the loads first, the sums in slot order.  N = 10: word [9] too (one 8-byte load);
// N = 12: words [9..11] too (one 16-byte load)
template <int U, int N>
__device__ __forceinline__ void sum_slots_trip(const float4* src, unsigned long long& live, float (&a)[N])
{
	static_assert(N == 9 || N == 10 || N == 12, "nine sums, ten with dL/dz, or twelve with the absolute mean2D sums");
	int idx[U];
	float4 x[U], y[U];
	float z[U], zd[U];
	float zx[U], zy[U];   // N == 12
#pragma unroll
	for (int j = 0; j < U; j++) {
		idx[j] = __ffsll((long long)live) - 1;
		live &= live - 1ull;
	}
#pragma unroll
	for (int j = 0; j < U; j++) {
		x[j] = src[SLOT_F4 * (size_t)idx[j]];
		y[j] = src[SLOT_F4 * (size_t)idx[j] + 1];
		if constexpr (N == 12) {
			const float4 t = src[SLOT_F4 * (size_t)idx[j] + 2];
			z[j] = t.x;
			zd[j] = t.y;
			zx[j] = t.z;
			zy[j] = t.w;
		} else if constexpr (N == 10) {
			const float2 t = *reinterpret_cast<const float2*>(src + SLOT_F4 * (size_t)idx[j] + 2);
			z[j] = t.x;
			zd[j] = t.y;
		} else {
			z[j] = src[SLOT_F4 * (size_t)idx[j] + 2].x;
		}
	}
#pragma unroll
	for (int j = 0; j < U; j++) {
		a[0] += x[j].x; a[1] += x[j].y; a[2] += x[j].z; a[3] += x[j].w;
		a[4] += y[j].x; a[5] += y[j].y; a[6] += y[j].z; a[7] += y[j].w;
		a[8] += z[j];
		if constexpr (N >= 10) a[9] += zd[j];
		if constexpr (N == 12) {
			a[10] += zx[j];
			a[11] += zy[j];
		}
	}
}

// 16 flag bytes (0 / 1 each) at p, squeezed to 16 bits (bit i = byte i)
__device__ __forceinline__ uint32_t squeeze_flags16(const uint8_t* p)
{
	uint4 f;
	__builtin_memcpy(&f, p, 16);   // unaligned 16-byte load
	return (((f.x * 0x01020408u) >> 24) & 0xFu) | ((((f.y * 0x01020408u) >> 24) & 0xFu) << 4) | ((((f.z * 0x01020408u) >> 24) & 0xFu) << 8) |
	       ((((f.w * 0x01020408u) >> 24) & 0xFu) << 12);
}

template <int N>
__device__ __forceinline__ void wave_sum_partial_runs(uint32_t cnt, uint32_t first, const float* __restrict__ partials,
                                                      const uint8_t* __restrict__ touched, float (&a)[N])
{
	const float4* part4 = reinterpret_cast<const float4*>(partials);
#pragma unroll
	for (int c = 0; c < N; c++) a[c] = 0.f;
	if (cnt != 0u && cnt <= LONG_RUN) {
		// the run's flags, 16 bytes per load, squeezed to one bit per slot: the loops below then run over the TOUCHED slots
		// only (~1 in 5) and their loads do not wait for one another (a byte-flag test per slot serialises on memory latency)
		unsigned long long live = 0ull;
#pragma unroll
		for (int c = 0; c < 4; c++)
			if (16u * c < cnt) live |= (unsigned long long)squeeze_flags16(touched + first + 16 * c) << (16 * c);
		if (cnt < 64u) live &= (1ull << cnt) - 1ull;
		const float4* src = part4 + SLOT_F4 * (size_t)first;
		// two touched slots per trip: their loads leave together, the sums follow in slot order (a lane's chain of dependent round
		// trips is what this HBM-latency-bound phase waits for: one slot per trip -> two: the stage 0.463 -> 0.452 ms at C3; four: equal)
		while (live & (live - 1ull)) sum_slots_trip<2>(src, live, a);
		while (live) sum_slots_trip<1>(src, live, a);
	}
	// a longer run was summed by long_run_sums_kernel (one wave per run), which left the total in the run's FIRST slot
	if (cnt > LONG_RUN && touched[first]) {
		const float4 x = part4[SLOT_F4 * (size_t)first], y = part4[SLOT_F4 * (size_t)first + 1];
		float z;
		if constexpr (N == 12) {
			const float4 t = part4[SLOT_F4 * (size_t)first + 2];
			z = t.x;
			a[9] = t.y; a[10] = t.z; a[11] = t.w;
		} else {
			z = part4[SLOT_F4 * (size_t)first + 2].x;
		}
		a[0] = x.x; a[1] = x.y; a[2] = x.z; a[3] = x.w;
		a[4] = y.x; a[5] = y.y; a[6] = y.z; a[7] = y.w;
		a[8] = z;
		if constexpr (N == 10) a[9] = part4[SLOT_F4 * (size_t)first + 2].y;
	}
}

// One wave per listed run: sum its touched slots in a fixed order, store the total in the run's first slot and flag it.  Lane l owns
// the k = ceil(cnt / 64) CONSECUTIVE slots [l k, (l + 1) k): 16-byte flag loads, then only the touched slots, four per trip.
// (Rounds 2-5 also carried two lane-strided forms behind GSR_LRS_MODE; this one measured fastest -- 20 -> 14 us at C3 -- and stayed.)
// DEPTH: word [9] (dL/dz) too, summed by a tenth full-wave reduction.  ABS: words [9..11], three more reductions.
template <bool DEPTH, bool ABS = false>
__device__ __forceinline__ void wave_sum_long_run(uint32_t first, uint32_t cnt, float* __restrict__ partials, uint8_t* __restrict__ touched)
{
	constexpr int N = ABS ? 12 : (DEPTH ? 10 : 9);
	const int l = lane_id();
	float4* part4 = reinterpret_cast<float4*>(partials);
	float v[N];
#pragma unroll
	for (int c = 0; c < N; c++) v[c] = 0.f;
	bool any = false;
	const uint32_t k = (cnt + 63u) >> 6;
	const uint32_t lo = (uint32_t)l * k, hi = min(cnt, lo + k);
	for (uint32_t g0 = lo; g0 < hi; g0 += 64u) {   // (one pass for runs of up to 4 096 slots)
		const uint32_t n = min(64u, hi - g0);
		unsigned long long live = 0ull;
#pragma unroll
		for (int c = 0; c < 4; c++)
			if (16u * c < n) live |= (unsigned long long)squeeze_flags16(touched + first + g0 + 16 * c) << (16 * c);   // (the array is padded by 64 bytes)
		if (n < 64u) live &= (1ull << n) - 1ull;
		any = any || live != 0ull;
		const float4* src = part4 + SLOT_F4 * (size_t)(first + g0);
		while (__popcll(live) >= 4) sum_slots_trip<4>(src, live, v);
		while (live & (live - 1ull)) sum_slots_trip<2>(src, live, v);
		while (live) sum_slots_trip<1>(src, live, v);
	}
	const bool some = wave_ballot(any) != 0ull;
	float v9 = 0.f;
	// (ABS without DEPTH: word [9] rides in the 16-byte load of words [8..11] and is zero -- the ABS blend writes it -- so it is
	// neither reduced nor needed: v9 stays 0)
	if constexpr (DEPTH) v9 = wave_sum_f32_lane63(v[9]);
	float v10 = 0.f, v11 = 0.f;
	if constexpr (ABS) {
		v10 = wave_sum_f32_lane63(v[10]);
		v11 = wave_sum_f32_lane63(v[11]);
	}
	float (&v_nine)[9] = *reinterpret_cast<float (*)[9]>(&v[0]);
	wave_reduce9_f32(v_nine);  // totals in lane 63; every lane has read its slots by now (the reduction is a rendezvous)
	if (l == 63) {
		part4[SLOT_F4 * (size_t)first] = make_float4(v[0], v[1], v[2], v[3]);
		part4[SLOT_F4 * (size_t)first + 1] = make_float4(v[4], v[5], v[6], v[7]);
		if constexpr (ABS) part4[SLOT_F4 * (size_t)first + 2] = make_float4(v[8], v9, v10, v11);
		else if constexpr (DEPTH) *reinterpret_cast<float2*>(part4 + SLOT_F4 * (size_t)first + 2) = make_float2(v[8], v9);
		else reinterpret_cast<float*>(part4 + SLOT_F4 * (size_t)first + 2)[0] = v[8];
		touched[first] = some ? 1 : 0;
	}
}

}  // namespace gsr
