// kernels_hals_dyn.hip -- accelerated HALS with per-column dynamic stopping of the inner sweeps (docs/HALS.md, "Dynamic stopping"), in one launch.
//
// k_sweeps_hals_dyn is a kernel of its own with the mapping (hals_geom.h), the prologue and the epilogue of k_sweeps_hals (kernels_hals_multi.hip); `sweeps` is
// the MAXIMUM number of passes.  For fixed G and a the columns of a panel are independent NNLS problems, so the rule is per column: with
// d_t = sum_k (p_k^(t) - p_k^(t-1))^2 a column is frozen after sweep t when d_t <= tol2 d_1 (tol2 = delta^2 rounded to T by the launcher), and a frozen column is
// never stepped again.  The lane that makes coordinate step k adds (new - old)^2 to its own partial sum; at the end of the sweep a butterfly over the L lanes of
// the column group forms d_t, the same bits in every lane of the group, so that the column state (threshold, count, frozen) stays uniform over the group.
//
// Leaving the sweep loop is a WORKGROUP-uniform decision: each wave votes "one of my columns is still live" into LDS, a barrier follows, and every thread reads
// the same four votes.  The streamed-G form has barriers inside the sweep; no wave leaves on its own.  No atomics: a repeated launch is bit-identical.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "hals_geom.h"
#include "kernels.h"
#include "split3.h"

namespace nmfamd {

constexpr int HALS_WAVES = HALS_THREADS / 64;

template <typename T, int RP, bool PEN>
__global__ __launch_bounds__(HALS_THREADS) void k_sweeps_hals_dyn(T* __restrict__ P, const T* __restrict__ slabs, int S, long slab_stride, const T* __restrict__ G,
                                                                  int r, int len_valid, T* __restrict__ ps, T* __restrict__ sumsq_part, T l1_arg, T l2_arg, int sweeps,
                                                                  T tol2_arg, int* __restrict__ counts) {
	using Gm = HalsGeom<T, RP>;
	constexpr int L = Gm::L, C = Gm::C, E = Gm::E, GROUPS = Gm::GROUPS, COLS = Gm::COLS, KC = Gm::KC;
	__shared__ __attribute__((aligned(16))) T sG[KC * RP];
	__shared__ int s_live[2][HALS_WAVES];            // the waves' votes, by the parity of the sweep
	// the state of a column beside `live`: thr = tol2 d_1 and cnt = sweeps applied, in LDS and not in registers (fp64 RP 256 and 512 have none to spare).  thr is
	// written by lane 0 of the column group at the end of sweep 0 and read by the group from sweep 1 on, behind the barrier of the vote; cnt is written and read
	// by that lane alone.
	__shared__ T s_thr[COLS];
	__shared__ int s_cnt[COLS];
	const int tid = threadIdx.x, lane = tid % L, grp = tid / L;
	const long y0 = (long)blockIdx.x * COLS;

	// (VGPRs: a uniform argument meets per-lane values below, split3.h)
	const T l1 = PEN ? in_vgpr(l1_arg) : T(0), l2 = PEN ? in_vgpr(l2_arg) : T(0);
	const T tol2 = in_vgpr(tol2_arg);
	T h[C][E], a[C][E], inv[E];
	// live = not frozen, uniform over the L lanes of a column.  A padding column is frozen at entry with count 0: its slabs may hold anything and must not keep
	// the workgroup in the loop.
	bool live[C];
#pragma unroll
	for (int c = 0; c < C; ++c) {
		const long y = y0 + c * GROUPS + grp;
		const long base = y * RP;
		const bool valid = y < len_valid;
		live[c] = valid;
		if (lane == 0) s_cnt[c * GROUPS + grp] = 0;
#pragma unroll
		for (int e = 0; e < E; ++e) {
			const int l = e * L + lane;
			T s = slabs[base + l];
			for (int k = 1; k < S; ++k) s += slabs[(long)k * slab_stride + base + l];
			a[c][e] = s;
			h[c][e] = (valid && l < r) ? P[base + l] : T(0);
		}
	}
#pragma unroll
	for (int e = 0; e < E; ++e) {
		const int k = e * L + lane;
		T d = k < r ? G[(long)k * RP + k] : T(0);
		if constexpr (PEN) { if (k < r) d += l2; }
		inv[e] = d > T(0) ? T(1) / d : T(0);        // 0: the coordinate is skipped (G(k, k) [+ l2] <= 0, or padding)
	}

	int k_lo = 0, k_hi = 0;
	for (int t = 0; t < sweeps; ++t) {               // (uniform, 1 ... 64; left early only by the uniform break at the bottom)
		// streamed G: LDS holds the last chunk of the sweep before; restage from row 0.  Resident G (r <= KC): staged by sweep 0, kept.
		if (r > KC) { k_lo = 0; k_hi = 0; }
		T acc[C];                                    // this lane's part of d_t
#pragma unroll
		for (int c = 0; c < C; ++c) acc[c] = T(0);
#pragma unroll
		for (int e = 0; e < E; ++e) {
			for (int q = 0; q < L; ++q) {
				const int k = e * L + q;
				if (k >= r) break;                       // (uniform)
				if (k >= k_hi) {
					__syncthreads();
					k_lo = k;
					k_hi = k + KC < r ? k + KC : r;
					const int count = (k_hi - k_lo) * RP;
					for (int i = tid; i < count; i += HALS_THREADS) sG[i] = G[(long)k_lo * RP + i];
					__syncthreads();
				}
				const T* gk = sG + (k - k_lo) * RP;
				T gv[E];
#pragma unroll
				for (int ee = 0; ee < E; ++ee) gv[ee] = gk[ee * L + lane];
#pragma unroll
				for (int c = 0; c < C; ++c) {
					T dot = 0;
#pragma unroll
					for (int ee = 0; ee < E; ++ee) dot += gv[ee] * h[c][ee];
#pragma unroll
					for (int off = L / 2; off > 0; off >>= 1) dot += __shfl_xor(dot, off, L);
					if (lane == q && inv[e] > T(0) && live[c]) {      // (a frozen column: the dot product was formed, the step is not made)
						T v;
						if constexpr (PEN) v = h[c][e] - ((dot - a[c][e]) + (l2 * h[c][e] + l1)) * inv[e];
						else v = h[c][e] - (dot - a[c][e]) * inv[e];
						v = v > T(0) ? v : T(0);
						const T moved = v - h[c][e];
						acc[c] += moved * moved;
						h[c][e] = v;
					}
				}
			}
		}
		// the end of sweep t: d_t per column (an xor butterfly: the same bits in all L lanes), the rule, the votes
		bool mine = false;
#pragma unroll
		for (int c = 0; c < C; ++c) {
			T d = acc[c];
#pragma unroll
			for (int off = L / 2; off > 0; off >>= 1) d += __shfl_xor(d, off, L);
			if (live[c]) {
				const int col = c * GROUPS + grp;
				T thr;
				if (t == 0) {
					thr = tol2 * d;
					if (lane == 0) s_thr[col] = thr;
				} else thr = s_thr[col];
				if (lane == 0) s_cnt[col] = t + 1;
				if (d <= thr) live[c] = false;           // (at t = 0 and tol2 < 1: only where the sweep moved nothing)
			}
			mine = mine || live[c];
		}
		const bool wave_live = __any(mine);
		if ((tid & 63) == 0) s_live[t & 1][tid >> 6] = wave_live ? 1 : 0;
		__syncthreads();                             // (the votes of sweep t + 2 reuse this row: every wave has passed the barrier of t + 1 by then, behind its reads here)
		int any_live = 0;
#pragma unroll
		for (int w = 0; w < HALS_WAVES; ++w) any_live |= s_live[t & 1][w];
		if (any_live == 0) break;                    // (uniform: every thread of the workgroup read the same votes)
	}

#pragma unroll
	for (int c = 0; c < C; ++c) {
		const long y = y0 + c * GROUPS + grp;
		const long base = y * RP;
		if (y >= len_valid) {                        // (h of a padding column was never stepped; its a may be anything)
#pragma unroll
			for (int e = 0; e < E; ++e) h[c][e] = T(0);
		}
#pragma unroll
		for (int e = 0; e < E; ++e) P[base + e * L + lane] = h[c][e];
		if (counts != nullptr && lane == 0) counts[y] = s_cnt[c * GROUPS + grp];      // (0 on padding)
		if (ps != nullptr) {
			T s = 0;
#pragma unroll
			for (int e = 0; e < E; ++e) s += h[c][e] * a[c][e];
#pragma unroll
			for (int off = L / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, L);
			if (lane == 0 && y < len_valid) ps[y] = s;
		}
	}
	if (sumsq_part == nullptr) return;
	__syncthreads();                                 // (sG: the last chunk of the last sweep has been read)
#pragma unroll
	for (int c = 0; c < C; ++c)
#pragma unroll
		for (int e = 0; e < E; ++e) sG[(c * GROUPS + grp) * RP + e * L + lane] = h[c][e] * h[c][e];
	__syncthreads();
	for (int cc = tid; cc < RP; cc += HALS_THREADS) {
		T s = 0;
		for (int col = 0; col < COLS; ++col) s += sG[col * RP + cc];
		sumsq_part[(long)blockIdx.x * RP + cc] = s;
	}
}

template <typename T, int RP>
static hipError_t sweeps_dyn_at(T* P, const T* slabs, int S, long slab_stride, const T* G, int r, int len_pad, int len_valid, T* ps, T* sumsq_part, hipStream_t stream, T l1,
                                T l2, int sweeps, T tol2, int* counts) {
	const dim3 grid(len_pad / HalsGeom<T, RP>::COLS);
	if (l1 != T(0) || l2 != T(0))
		hipLaunchKernelGGL((k_sweeps_hals_dyn<T, RP, true>), grid, dim3(HALS_THREADS), 0, stream, P, slabs, S, slab_stride, G, r, len_valid, ps, sumsq_part, l1, l2, sweeps, tol2, counts);
	else
		hipLaunchKernelGGL((k_sweeps_hals_dyn<T, RP, false>), grid, dim3(HALS_THREADS), 0, stream, P, slabs, S, slab_stride, G, r, len_valid, ps, sumsq_part, T(0), T(0), sweeps, tol2,
		                   counts);
	return hipGetLastError();
}

template <typename T>
hipError_t launch_panel_sweeps_hals_dyn(T* P, const T* slabs, int S, long slab_stride, const T* G, int RP, int r, int len_pad, int len_valid, T* ps, T* sumsq_part,
                                        hipStream_t stream, T l1, T l2, int sweeps, double tol, int* counts) {
	if (sweeps < HALS_SWEEPS_MIN || sweeps > HALS_SWEEPS_MAX) return hipErrorInvalidValue;
	if (!(tol > 0.0 && tol < 1.0)) return hipErrorInvalidValue;      // (NaN included; 0 is launch_panel_sweeps_hals, the caller's choice)
	if (!panel_sweep_hals_available(RP, sizeof(T)) || S < 1 || r < 1 || r > RP || len_pad % 128 != 0 || len_valid > len_pad) return hipErrorInvalidValue;
	if (!(l1 >= T(0)) || !(l2 >= T(0)) || !std::isfinite(l1) || !std::isfinite(l2)) return hipErrorInvalidValue;
	const T tol2 = (T)(tol * tol);                   // delta^2, rounded once to the engine's precision (0 where it underflows: only a sweep that moves nothing freezes)
	switch (RP) {
	case 64: return sweeps_dyn_at<T, 64>(P, slabs, S, slab_stride, G, r, len_pad, len_valid, ps, sumsq_part, stream, l1, l2, sweeps, tol2, counts);
	case 128: return sweeps_dyn_at<T, 128>(P, slabs, S, slab_stride, G, r, len_pad, len_valid, ps, sumsq_part, stream, l1, l2, sweeps, tol2, counts);
	case 192: if constexpr (sizeof(T) == 8) return sweeps_dyn_at<T, 192>(P, slabs, S, slab_stride, G, r, len_pad, len_valid, ps, sumsq_part, stream, l1, l2, sweeps, tol2, counts); break;      // (fp64 only)
	case 256: return sweeps_dyn_at<T, 256>(P, slabs, S, slab_stride, G, r, len_pad, len_valid, ps, sumsq_part, stream, l1, l2, sweeps, tol2, counts);
	case 320: if constexpr (sizeof(T) == 8) return sweeps_dyn_at<T, 320>(P, slabs, S, slab_stride, G, r, len_pad, len_valid, ps, sumsq_part, stream, l1, l2, sweeps, tol2, counts); break;      // (fp64 only)
	case 384: return sweeps_dyn_at<T, 384>(P, slabs, S, slab_stride, G, r, len_pad, len_valid, ps, sumsq_part, stream, l1, l2, sweeps, tol2, counts);
	case 448: if constexpr (sizeof(T) == 8) return sweeps_dyn_at<T, 448>(P, slabs, S, slab_stride, G, r, len_pad, len_valid, ps, sumsq_part, stream, l1, l2, sweeps, tol2, counts); break;      // (fp64 only)
	case 512: return sweeps_dyn_at<T, 512>(P, slabs, S, slab_stride, G, r, len_pad, len_valid, ps, sumsq_part, stream, l1, l2, sweeps, tol2, counts);
	}
	return hipErrorInvalidValue;
}
template hipError_t launch_panel_sweeps_hals_dyn<float>(float*, const float*, int, long, const float*, int, int, int, int, float*, float*, hipStream_t, float, float, int, double, int*);
template hipError_t launch_panel_sweeps_hals_dyn<double>(double*, const double*, int, long, const double*, int, int, int, int, double*, double*, hipStream_t, double, double, int, double,
                                                         int*);

} // namespace nmfamd
