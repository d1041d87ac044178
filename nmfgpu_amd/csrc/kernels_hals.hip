// kernels_hals.hip -- HALS (hierarchical alternating least squares, coordinate descent; Cichocki & Phan 2009): the Gauss-Seidel sweep over the r
// coordinates of every panel column, and the column normalisation that keeps W H unchanged.  docs/HALS.md states the semantics and the mapping.
//
// Panel layout of the engine: column y of H (or row y of W) is RP contiguous elements at P[y * RP].  For each column, with
// a = sum of the split-K slabs (W^T V, or (V H^T)^T) and the r x r Gram matrix G (W^T W, or H H^T):
//   for k = 0 .. r - 1, skipping k where G(k, k) <= 0:   p(k) <- max(0, p(k) - (G(k, :) . p - a(k)) / G(k, k))
// with the entries l < k already updated (Gauss-Seidel).  Coordinates k >= r and columns y >= len_valid are written as 0, whatever the padding of P,
// the slabs and G holds, and add nothing to ps or sumsq_part (an invalid column is swept like the others and masked when it is written).
//
// Mapping: L lanes per column, lane j holds the entries l = e * L + j (e = 0 .. E - 1, E = RP / L) of the column and of a in registers; a
// workgroup of 256 threads takes 256 / L groups times C columns.  At step k every lane forms its part of G(k, :) . p from the row k of G
// (staged in LDS in chunks of KC rows, shared by every column of the workgroup), the L parts are summed by a butterfly inside the group,
// and the owning lane (j = k % L, register e = k / L -- a compile-time index, the loop over e is unrolled) applies the step.  The
// reciprocals 1 / G(k, k) live in the owner's registers.  Optional outputs as k_panel_update's: ps(y) = sum_k p_new(k) a(k) and per-workgroup
// partial sums of squares of the new entries.
//
// Penalised form (PEN; scikit-learn's coordinate descent with an L1 and an L2 penalty on the swept factor, l1, l2 >= 0): with d(k) = G(k, k) + l2,
//   skipping k where d(k) <= 0:   p(k) <- max(0, p(k) - (G(k, :) . p + l2 p(k) - a(k) + l1) / d(k))
// G and a stay unpenalised: ps is formed from the raw a, and the engine's trace reads the raw Gram matrix.  The launcher picks the plain instantiation
// when both penalties are 0, so that form is the same code as before the penalties existed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "hals_geom.h"
#include "kernels.h"
#include "split3.h"

namespace nmfamd {

template <typename T, int RP, bool PEN>
__global__ __launch_bounds__(HALS_THREADS) void k_sweep_hals(T* __restrict__ P, const T* __restrict__ slabs, int S, long slab_stride, const T* __restrict__ G,
                                                             int r, int len_valid, T* __restrict__ ps, T* __restrict__ sumsq_part, T l1_arg, T l2_arg) {
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

#pragma unroll
	for (int c = 0; c < C; ++c) {
		const long y = y0 + c * GROUPS + grp;
		const long base = y * RP;
		if (y >= len_valid) {                        // (the slabs of a padding column need not be 0: its sweep is discarded)
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
	__syncthreads();                                 // (sG: the last chunk has been read)
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
static hipError_t sweep_at(T* P, const T* slabs, int S, long slab_stride, const T* G, int r, int len_pad, int len_valid, T* ps, T* sumsq_part, hipStream_t stream, T l1, T l2) {
	const dim3 grid(len_pad / HalsGeom<T, RP>::COLS);
	if (l1 != T(0) || l2 != T(0)) hipLaunchKernelGGL((k_sweep_hals<T, RP, true>), grid, dim3(HALS_THREADS), 0, stream, P, slabs, S, slab_stride, G, r, len_valid, ps, sumsq_part, l1, l2);
	else hipLaunchKernelGGL((k_sweep_hals<T, RP, false>), grid, dim3(HALS_THREADS), 0, stream, P, slabs, S, slab_stride, G, r, len_valid, ps, sumsq_part, T(0), T(0));
	return hipGetLastError();
}

template <typename T>
static int sweep_cols(int RP) {
	switch (RP) {
	case 64: return HalsGeom<T, 64>::COLS;
	case 128: return HalsGeom<T, 128>::COLS;
	case 192: return HalsGeom<T, 192>::COLS;
	case 256: return HalsGeom<T, 256>::COLS;
	case 320: return HalsGeom<T, 320>::COLS;
	case 384: return HalsGeom<T, 384>::COLS;
	case 448: return HalsGeom<T, 448>::COLS;
	case 512: return HalsGeom<T, 512>::COLS;
	}
	return 0;
}

bool panel_sweep_hals_available(int RP, size_t elem) {
	if (elem == 4) return RP == 64 || RP == 128 || RP == 256 || RP == 384 || RP == 512;
	return elem == 8 && RP % 64 == 0 && RP >= 64 && RP <= 512;
}

int panel_sweep_hals_parts(int RP, size_t elem, int len_pad) {
	if (!panel_sweep_hals_available(RP, elem)) return 0;
	const int cols = elem == 8 ? sweep_cols<double>(RP) : sweep_cols<float>(RP);
	return len_pad / cols;
}

template <typename T>
hipError_t launch_panel_sweep_hals(T* P, const T* slabs, int S, long slab_stride, const T* G, int RP, int r, int len_pad, int len_valid, T* ps, T* sumsq_part,
                                   hipStream_t stream, T l1, T l2) {
	if (!panel_sweep_hals_available(RP, sizeof(T)) || r < 1 || r > RP || len_pad % 128 != 0 || len_valid > len_pad) return hipErrorInvalidValue;
	if (!(l1 >= T(0)) || !(l2 >= T(0)) || !std::isfinite(l1) || !std::isfinite(l2)) return hipErrorInvalidValue;
	switch (RP) {
	case 64: return sweep_at<T, 64>(P, slabs, S, slab_stride, G, r, len_pad, len_valid, ps, sumsq_part, stream, l1, l2);
	case 128: return sweep_at<T, 128>(P, slabs, S, slab_stride, G, r, len_pad, len_valid, ps, sumsq_part, stream, l1, l2);
	case 192: if constexpr (sizeof(T) == 8) return sweep_at<T, 192>(P, slabs, S, slab_stride, G, r, len_pad, len_valid, ps, sumsq_part, stream, l1, l2); break;      // (fp64 only)
	case 256: return sweep_at<T, 256>(P, slabs, S, slab_stride, G, r, len_pad, len_valid, ps, sumsq_part, stream, l1, l2);
	case 320: if constexpr (sizeof(T) == 8) return sweep_at<T, 320>(P, slabs, S, slab_stride, G, r, len_pad, len_valid, ps, sumsq_part, stream, l1, l2); break;      // (fp64 only)
	case 384: return sweep_at<T, 384>(P, slabs, S, slab_stride, G, r, len_pad, len_valid, ps, sumsq_part, stream, l1, l2);
	case 448: if constexpr (sizeof(T) == 8) return sweep_at<T, 448>(P, slabs, S, slab_stride, G, r, len_pad, len_valid, ps, sumsq_part, stream, l1, l2); break;      // (fp64 only)
	case 512: return sweep_at<T, 512>(P, slabs, S, slab_stride, G, r, len_pad, len_valid, ps, sumsq_part, stream, l1, l2);
	}
	return hipErrorInvalidValue;
}
template hipError_t launch_panel_sweep_hals<float>(float*, const float*, int, long, const float*, int, int, int, int, float*, float*, hipStream_t, float, float);
template hipError_t launch_panel_sweep_hals<double>(double*, const double*, int, long, const double*, int, int, int, int, double*, double*, hipStream_t, double, double);

// ------------------------------------------------------------------------------------------
// Column normalisation of W that keeps W H: d(c) = ||W(:, c)|| from the summed squares; where d(c) > 0, W(:, c) <- W(:, c) / d(c) and
// H(c, :) <- H(c, :) d(c) (the sum > 0 guard of kernel::normalizeColumns).  One launch over both panels, four consecutive entries per thread.
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_hals_rescale(T* __restrict__ Wt, long w_quads, T* __restrict__ H, long h_quads, int RP, const T* __restrict__ colsq) {
	typedef T T4 __attribute__((ext_vector_type(4)));
	const long e = (long)blockIdx.x * 256 + threadIdx.x;
	const bool on_w = e < w_quads;
	if (!on_w && e >= w_quads + h_quads) return;
	T* p = on_w ? Wt + 4 * e : H + 4 * (e - w_quads);
	const int c0 = (int)((4 * (on_w ? e : e - w_quads)) % RP);
	T4 v = *reinterpret_cast<const T4*>(p);
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		const T s = colsq[c0 + k];
		if (s > T(0)) {
			const T d = (T)sqrt(s);
			v[k] = on_w ? v[k] / d : v[k] * d;
		}
	}
	*reinterpret_cast<T4*>(p) = v;
}

template <typename T>
hipError_t launch_hals_normalize(T* Wt, int RP, int mpad, T* H, int npad, T* sumsq_part, int parts, hipStream_t stream) {
	// the r sums into the scratch behind the partials (RP elements of the 16 * RP every sum-of-squares buffer carries), one order for both panels
	T* colsq = sumsq_part + (long)parts * RP;
	if (hipError_t err = launch_reduce_partials<T>(sumsq_part, parts, RP, colsq, RP, stream); err != hipSuccess) return err;
	const long wq = (long)mpad * RP / 4, hq = (long)npad * RP / 4;
	hipLaunchKernelGGL((k_hals_rescale<T>), dim3((unsigned)((wq + hq + 255) / 256)), dim3(256), 0, stream, Wt, wq, H, hq, RP, (const T*)colsq);
	return hipGetLastError();
}
template hipError_t launch_hals_normalize<float>(float*, int, int, float*, int, float*, int, hipStream_t);
template hipError_t launch_hals_normalize<double>(double*, int, int, double*, int, double*, int, hipStream_t);

} // namespace nmfamd
