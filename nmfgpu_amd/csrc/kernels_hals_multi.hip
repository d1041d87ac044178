// kernels_hals_multi.hip -- accelerated HALS (Gillis & Glineur 2012): several Gauss-Seidel sweeps of a panel against the SAME Gram matrix G and the SAME
// summed slabs a, in one launch.  docs/HALS.md, "Inner sweeps", states the semantics; kernels_hals.hip has the single sweep and describes the mapping, which
// this kernel shares (hals_geom.h).
//
// k_sweeps_hals is k_sweep_hals with its pass over k = 0 .. r - 1 repeated `sweeps` times: the prologue (slab sums into a, the old column into h, the
// reciprocals of the diagonal) runs once, h and a stay in registers between the sweeps, and the epilogue (panel, ps, partial sums of squares) runs once from
// the final h.  Per sweep after the first that saves a launch, S reads of the slabs and a read and a write of the panel.  Where all of G fits one LDS chunk
// (r <= KC) it is staged once; where it is streamed in chunks of KC rows, every sweep starts again from chunk 0 behind a barrier, because the chunk left in LDS
// by the end of a sweep holds the LAST rows of G.  `sweeps` is a uniform argument bounded by the launcher (1 ... 64).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "hals_geom.h"
#include "kernels.h"
#include "split3.h"

namespace nmfamd {

template <typename T, int RP, bool PEN>
__global__ __launch_bounds__(HALS_THREADS) void k_sweeps_hals(T* __restrict__ P, const T* __restrict__ slabs, int S, long slab_stride, const T* __restrict__ G,
                                                              int r, int len_valid, T* __restrict__ ps, T* __restrict__ sumsq_part, T l1_arg, T l2_arg, int sweeps) {
	using Gm = HalsGeom<T, RP>;
	constexpr int L = Gm::L, C = Gm::C, E = Gm::E, GROUPS = Gm::GROUPS, COLS = Gm::COLS, KC = Gm::KC;
	__shared__ __attribute__((aligned(16))) T sG[KC * RP];
	const int tid = threadIdx.x, lane = tid % L, grp = tid / L;
	const long y0 = (long)blockIdx.x * COLS;

	// (VGPRs: a uniform argument meets per-lane values below, split3.h)
	const T l1 = PEN ? in_vgpr(l1_arg) : T(0), l2 = PEN ? in_vgpr(l2_arg) : T(0);
	T h[C][E], a[C][E], inv[E];
#pragma unroll
	for (int c = 0; c < C; ++c) {
		const long y = y0 + c * GROUPS + grp;
		const long base = y * RP;
		const bool valid = y < len_valid;
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
	for (int t = 0; t < sweeps; ++t) {               // (uniform, 1 ... 64)
		// streamed G: LDS holds the last chunk of the sweep before; restage from row 0 (the barrier in front of the staging keeps that chunk until every wave has
		// finished with it).  Resident G (r <= KC): staged by sweep 0 as [0, r), which no k of a later sweep leaves.
		if (r > KC) { k_lo = 0; k_hi = 0; }
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
					if (lane == q && inv[e] > T(0)) {
						T v;
						if constexpr (PEN) v = h[c][e] - ((dot - a[c][e]) + (l2 * h[c][e] + l1)) * inv[e];
						else v = h[c][e] - (dot - a[c][e]) * inv[e];
						h[c][e] = v > T(0) ? v : T(0);
					}
				}
			}
		}
	}

#pragma unroll
	for (int c = 0; c < C; ++c) {
		const long y = y0 + c * GROUPS + grp;
		const long base = y * RP;
		if (y >= len_valid) {                        // (the slabs of a padding column need not be 0: its sweeps are discarded)
#pragma unroll
			for (int e = 0; e < E; ++e) h[c][e] = T(0);
		}
#pragma unroll
		for (int e = 0; e < E; ++e) P[base + e * L + lane] = h[c][e];
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
static hipError_t sweeps_at(T* P, const T* slabs, int S, long slab_stride, const T* G, int r, int len_pad, int len_valid, T* ps, T* sumsq_part, hipStream_t stream, T l1, T l2,
                            int sweeps) {
	const dim3 grid(len_pad / HalsGeom<T, RP>::COLS);
	if (l1 != T(0) || l2 != T(0))
		hipLaunchKernelGGL((k_sweeps_hals<T, RP, true>), grid, dim3(HALS_THREADS), 0, stream, P, slabs, S, slab_stride, G, r, len_valid, ps, sumsq_part, l1, l2, sweeps);
	else hipLaunchKernelGGL((k_sweeps_hals<T, RP, false>), grid, dim3(HALS_THREADS), 0, stream, P, slabs, S, slab_stride, G, r, len_valid, ps, sumsq_part, T(0), T(0), sweeps);
	return hipGetLastError();
}

template <typename T>
hipError_t launch_panel_sweeps_hals(T* P, const T* slabs, int S, long slab_stride, const T* G, int RP, int r, int len_pad, int len_valid, T* ps, T* sumsq_part,
                                    hipStream_t stream, T l1, T l2, int sweeps) {
	if (sweeps < HALS_SWEEPS_MIN || sweeps > HALS_SWEEPS_MAX) return hipErrorInvalidValue;
	// one sweep: the single-sweep kernel through its own launcher, as before the counts existed
	if (sweeps == 1) return launch_panel_sweep_hals<T>(P, slabs, S, slab_stride, G, RP, r, len_pad, len_valid, ps, sumsq_part, stream, l1, l2);
	if (!panel_sweep_hals_available(RP, sizeof(T)) || S < 1 || r < 1 || r > RP || len_pad % 128 != 0 || len_valid > len_pad) return hipErrorInvalidValue;
	if (!(l1 >= T(0)) || !(l2 >= T(0)) || !std::isfinite(l1) || !std::isfinite(l2)) return hipErrorInvalidValue;
	switch (RP) {
	case 64: return sweeps_at<T, 64>(P, slabs, S, slab_stride, G, r, len_pad, len_valid, ps, sumsq_part, stream, l1, l2, sweeps);
	case 128: return sweeps_at<T, 128>(P, slabs, S, slab_stride, G, r, len_pad, len_valid, ps, sumsq_part, stream, l1, l2, sweeps);
	case 192: if constexpr (sizeof(T) == 8) return sweeps_at<T, 192>(P, slabs, S, slab_stride, G, r, len_pad, len_valid, ps, sumsq_part, stream, l1, l2, sweeps); break;      // (fp64 only)
	case 256: return sweeps_at<T, 256>(P, slabs, S, slab_stride, G, r, len_pad, len_valid, ps, sumsq_part, stream, l1, l2, sweeps);
	case 320: if constexpr (sizeof(T) == 8) return sweeps_at<T, 320>(P, slabs, S, slab_stride, G, r, len_pad, len_valid, ps, sumsq_part, stream, l1, l2, sweeps); break;      // (fp64 only)
	case 384: return sweeps_at<T, 384>(P, slabs, S, slab_stride, G, r, len_pad, len_valid, ps, sumsq_part, stream, l1, l2, sweeps);
	case 448: if constexpr (sizeof(T) == 8) return sweeps_at<T, 448>(P, slabs, S, slab_stride, G, r, len_pad, len_valid, ps, sumsq_part, stream, l1, l2, sweeps); break;      // (fp64 only)
	case 512: return sweeps_at<T, 512>(P, slabs, S, slab_stride, G, r, len_pad, len_valid, ps, sumsq_part, stream, l1, l2, sweeps);
	}
	return hipErrorInvalidValue;
}
template hipError_t launch_panel_sweeps_hals<float>(float*, const float*, int, long, const float*, int, int, int, int, float*, float*, hipStream_t, float, float, int);
template hipError_t launch_panel_sweeps_hals<double>(double*, const double*, int, long, const double*, int, int, int, int, double*, double*, hipStream_t, double, double, int);

} // namespace nmfamd
