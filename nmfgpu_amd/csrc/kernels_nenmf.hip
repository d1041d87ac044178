// kernels_nenmf.hip -- NeNMF (Guan, Tao, Luo, Yuan 2012): Nesterov-accelerated projected-gradient steps on the non-negative least-squares problem of one
// factor, in the slot of the HALS sweeps.  docs/NENMF.md states the semantics; kernels_hals.hip describes the arrays (panel layout, slabs, ps, sumsq_part).
//
// For the panel P (r x len), the Gram matrix G, a = the summed slabs and the penalties (l1, l2):
//   L = max_k sum_l G(k, l) + l2                                  (one value per launch, every workgroup computes it the same way from its staged G)
//   Y_0 = P_0;   P_{t+1} = max(0, Y_t - (G Y_t + l2 Y_t - a + l1) / L);   Y_{t+1} = P_{t+1} + c_t (P_{t+1} - P_t),   t = 0 .. steps - 1;   result P_steps
// with the momentum coefficients c_t = (alpha_t - 1) / alpha_{t+1} handed over by the launcher.  L <= 0 or not finite: no step is taken.
//
// Mapping: a workgroup of four waves owns COLS panel columns for all steps.  G (rows and columns >= r stored as 0) is staged once into LDS and is the A operand of
// v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64, whose operand maps are the same in both precisions; Y goes through LDS once per step as the B operand ([column][k],
// so a lane fetches VEC consecutive k of its column with one 16-byte read, as it does from its row of G -- the k order inside a block of 4 VEC is permuted the same
// way on both sides).  Wave w computes the rows [w RP / 4, (w + 1) RP / 4) of G Y for all COLS columns; a, P_t, Y_t and the product live in registers in the
// accumulator layout (column on the lane, rows in the registers), so the step and the extrapolation are lane-local.  Both LDS images have a row stride of RP
// elements + 32 bytes: the 16-byte reads of a lane group then fall on distinct banks.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <limits>

#include "kernels.h"
#include "split3.h"

namespace nmfamd {

constexpr int APG_THREADS = 256;

template <typename T>
struct ApgCoef { T c[APG_STEPS_MAX]; };      // c[t]: the extrapolation after step t (the last one is not used)

template <typename T, int RP>
struct ApgGeom {
	static constexpr int COLS = sizeof(T) == 4 ? 32 : 16;            // panel columns per workgroup
	static constexpr int VEC = 16 / (int)sizeof(T);                  // elements per 16-byte LDS read
	static constexpr int KB = 4 * VEC;                               // k per block: VEC MFMAs of k = 4
	static constexpr int LD = RP + 32 / (int)sizeof(T);              // row stride of both LDS images
	static constexpr int RW = RP / 64, CT = COLS / 16;               // 16 x 16 tiles per wave: RW down, CT across
	static constexpr int NBUF = (RP + 2 * COLS) * LD * (int)sizeof(T) <= 160 * 1024 ? 2 : 1;      // images of Y: two save the barrier behind the product
	static_assert(RP % 64 == 0 && RP <= APG_THREADS && 128 % COLS == 0 && COLS * LD >= RP && COLS * LD >= 16 * COLS, "tile shape");
	static_assert((RP + NBUF * COLS) * LD * (int)sizeof(T) <= 160 * 1024, "G and Y fit LDS");
};

template <typename T> struct ApgAcc;
template <> struct ApgAcc<float> { typedef float V4 __attribute__((ext_vector_type(4))); };
template <> struct ApgAcc<double> { typedef double V4 __attribute__((ext_vector_type(4))); };

__device__ inline ApgAcc<float>::V4 apg_mfma(float a, float b, ApgAcc<float>::V4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ inline ApgAcc<double>::V4 apg_mfma(double a, double b, ApgAcc<double>::V4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// row inside a 16 x 16 result tile of register e in lane group q (the f64 instruction has its own map)
template <typename T>
__device__ inline int apg_row(int q, int e) { return sizeof(T) == 4 ? 4 * q + e : q + 4 * e; }

template <typename T, int RP, bool PEN>
__global__ __launch_bounds__(APG_THREADS) void k_apg_steps(T* __restrict__ P, const T* __restrict__ slabs, int S, long slab_stride, const T* __restrict__ G, int r,
                                                           int len_valid, T* __restrict__ ps, T* __restrict__ sumsq_part, T l1_arg, T l2_arg, int steps, ApgCoef<T> coef) {
	using Gm = ApgGeom<T, RP>;
	constexpr int COLS = Gm::COLS, VEC = Gm::VEC, KB = Gm::KB, LD = Gm::LD, RW = Gm::RW, CT = Gm::CT, NBUF = Gm::NBUF;
	typedef T TV __attribute__((ext_vector_type(VEC)));
	typedef typename ApgAcc<T>::V4 V4;
	__shared__ __attribute__((aligned(16))) T sG[RP * LD];
	__shared__ __attribute__((aligned(16))) T sY[NBUF * COLS * LD];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, c16 = lane & 15;
	const long y0 = (long)blockIdx.x * COLS;

	// (VGPRs: a uniform argument meets per-lane values below, split3.h)
	const T l1 = PEN ? in_vgpr(l1_arg) : T(0), l2 = PEN ? in_vgpr(l2_arg) : T(0);

	// G into LDS, rows and columns >= r as 0 whatever the padding holds
	for (int i = tid; i < RP * (RP / VEC); i += APG_THREADS) {
		const int k = i / (RP / VEC), l = (i % (RP / VEC)) * VEC;
		TV v;
#pragma unroll
		for (int e = 0; e < VEC; ++e) v[e] = T(0);
		if (k < r && l < r) {
			v = *reinterpret_cast<const TV*>(G + (long)k * RP + l);
#pragma unroll
			for (int e = 0; e < VEC; ++e) { if (l + e >= r) v[e] = T(0); }
		}
		*reinterpret_cast<TV*>(sG + k * LD + l) = v;
	}

	// the summed slabs and the old columns, in the accumulator layout; 0 on coordinates >= r and on padding columns
	T a[RW][CT][4], p[RW][CT][4], y[RW][CT][4];
#pragma unroll
	for (int i = 0; i < RW; ++i)
#pragma unroll
		for (int j = 0; j < CT; ++j) {
			const long col = y0 + 16 * j + c16;
#pragma unroll
			for (int e = 0; e < 4; ++e) {
				const int row = 16 * (wave * RW + i) + apg_row<T>(q, e);
				T s = 0, v = 0;
				if (col < len_valid && row < r) {
					const long at = col * RP + row;
					s = slabs[at];
					for (int k = 1; k < S; ++k) s += slabs[(long)k * slab_stride + at];
					v = P[at];
				}
				a[i][j][e] = s; p[i][j][e] = v; y[i][j][e] = v;
			}
		}

	// L: the row sums of G in the order of l, their maximum, + l2 -- from the staged G, the same in every workgroup
	__syncthreads();
	if (tid < RP) {
		T s = 0;
		if (tid < r) {
			for (int l = 0; l < r; l += VEC) {
				const TV v = *reinterpret_cast<const TV*>(sG + tid * LD + l);
#pragma unroll
				for (int e = 0; e < VEC; ++e) s += v[e];
			}
		}
		sY[tid] = s;
	}
	__syncthreads();
	T lip = sY[0];
	for (int k = 1; k < r; ++k) {
		const T v = sY[k];
		lip = (v > lip || v != v) ? v : lip;         // (a NaN stays)
	}
	lip += l2;
	const bool take = lip > T(0) && lip <= std::numeric_limits<T>::max() && steps > 0;      // (uniform)
	const T inv = T(1) / lip;
	__syncthreads();                                 // (sY: the row sums have been read)

	if (take) {
		const int kblocks = (r + KB - 1) / KB;
		for (int t = 0; t < steps; ++t) {            // (uniform, 1 ... APG_STEPS_MAX)
			T* buf = sY + (NBUF == 2 ? (t & 1) * COLS * LD : 0);
#pragma unroll
			for (int i = 0; i < RW; ++i)
#pragma unroll
				for (int j = 0; j < CT; ++j)
#pragma unroll
					for (int e = 0; e < 4; ++e) buf[(16 * j + c16) * LD + 16 * (wave * RW + i) + apg_row<T>(q, e)] = y[i][j][e];
			__syncthreads();
			V4 acc[RW][CT];
#pragma unroll
			for (int i = 0; i < RW; ++i)
#pragma unroll
				for (int j = 0; j < CT; ++j)
#pragma unroll
					for (int e = 0; e < 4; ++e) acc[i][j][e] = T(0);
			for (int kb = 0; kb < kblocks; ++kb) {
				TV av[RW], bv[CT];
#pragma unroll
				for (int i = 0; i < RW; ++i) av[i] = *reinterpret_cast<const TV*>(sG + (16 * (wave * RW + i) + c16) * LD + kb * KB + VEC * q);
#pragma unroll
				for (int j = 0; j < CT; ++j) bv[j] = *reinterpret_cast<const TV*>(buf + (16 * j + c16) * LD + kb * KB + VEC * q);
#pragma unroll
				for (int s = 0; s < VEC; ++s)
#pragma unroll
					for (int i = 0; i < RW; ++i)
#pragma unroll
						for (int j = 0; j < CT; ++j) acc[i][j] = apg_mfma(av[i][s], bv[j][s], acc[i][j]);
			}
			if (NBUF == 1) __syncthreads();          // (one image of Y: the next step writes the one this product read)
			const bool last = t + 1 == steps;
			const T c = in_vgpr(coef.c[t]);
#pragma unroll
			for (int i = 0; i < RW; ++i)
#pragma unroll
				for (int j = 0; j < CT; ++j)
#pragma unroll
					for (int e = 0; e < 4; ++e) {
						const T yv = y[i][j][e];
						T g;
						if constexpr (PEN) g = (acc[i][j][e] - a[i][j][e]) + (l2 * yv + l1);
						else g = acc[i][j][e] - a[i][j][e];
						const T v = yv - g * inv;
						const T pn = v > T(0) ? v : T(0);
						if (!last) y[i][j][e] = pn + c * (pn - p[i][j][e]);
						p[i][j][e] = pn;
					}
		}
	}

	// the panel; per column the parts of ps of this lane's rows
	T part[CT];
#pragma unroll
	for (int j = 0; j < CT; ++j) {
		const long col = y0 + 16 * j + c16;
		T s = 0;
#pragma unroll
		for (int i = 0; i < RW; ++i)
#pragma unroll
			for (int e = 0; e < 4; ++e) {
				P[col * RP + 16 * (wave * RW + i) + apg_row<T>(q, e)] = p[i][j][e];
				s += p[i][j][e] * a[i][j][e];
			}
		part[j] = s;
	}
	if (ps != nullptr) {
		__syncthreads();                             // (sY: the last product has been read)
#pragma unroll
		for (int j = 0; j < CT; ++j) sY[(wave * 4 + q) * COLS + 16 * j + c16] = part[j];
		__syncthreads();
		if (tid < COLS && y0 + tid < len_valid) {
			T s = 0;
			for (int k = 0; k < 16; ++k) s += sY[k * COLS + tid];
			ps[y0 + tid] = s;
		}
	}
	if (sumsq_part == nullptr) return;
	__syncthreads();
#pragma unroll
	for (int i = 0; i < RW; ++i)
#pragma unroll
		for (int j = 0; j < CT; ++j)
#pragma unroll
			for (int e = 0; e < 4; ++e) sY[(16 * j + c16) * LD + 16 * (wave * RW + i) + apg_row<T>(q, e)] = p[i][j][e] * p[i][j][e];
	__syncthreads();
	if (tid < RP) {
		T s = 0;
		for (int col = 0; col < COLS; ++col) s += sY[col * LD + tid];
		sumsq_part[(long)blockIdx.x * RP + tid] = s;
	}
}

template <typename T, int RP>
static hipError_t apg_at(T* P, const T* slabs, int S, long slab_stride, const T* G, int r, int len_pad, int len_valid, T* ps, T* sumsq_part, hipStream_t stream, T l1, T l2,
                         int steps, const ApgCoef<T>& coef) {
	const dim3 grid(len_pad / ApgGeom<T, RP>::COLS);
	if (l1 != T(0) || l2 != T(0))
		hipLaunchKernelGGL((k_apg_steps<T, RP, true>), grid, dim3(APG_THREADS), 0, stream, P, slabs, S, slab_stride, G, r, len_valid, ps, sumsq_part, l1, l2, steps, coef);
	else hipLaunchKernelGGL((k_apg_steps<T, RP, false>), grid, dim3(APG_THREADS), 0, stream, P, slabs, S, slab_stride, G, r, len_valid, ps, sumsq_part, T(0), T(0), steps, coef);
	return hipGetLastError();
}

bool panel_steps_apg_available(int RP, size_t elem) { return (elem == 4 || elem == 8) && (RP == 64 || RP == 128); }

int panel_steps_apg_parts(int RP, size_t elem, int len_pad) {
	if (!panel_steps_apg_available(RP, elem)) return 0;
	return len_pad / (elem == 8 ? ApgGeom<double, 64>::COLS : ApgGeom<float, 64>::COLS);
}

void apg_momentum(int steps, double* out) {
	double alpha = 1;
	for (int t = 0; t < steps; ++t) {
		const double next = (1 + std::sqrt(4 * alpha * alpha + 1)) / 2;
		out[t] = (alpha - 1) / next;
		alpha = next;
	}
}

template <typename T>
hipError_t launch_panel_steps_apg(T* P, const T* slabs, int S, long slab_stride, const T* G, int RP, int r, int len_pad, int len_valid, T* ps, T* sumsq_part,
                                  hipStream_t stream, T l1, T l2, int steps) {
	if (steps < APG_STEPS_MIN || steps > APG_STEPS_MAX) return hipErrorInvalidValue;
	if (!panel_steps_apg_available(RP, sizeof(T)) || S < 1 || r < 1 || r > RP || len_pad < 128 || len_pad % 128 != 0 || len_valid < 0 || len_valid > len_pad) return hipErrorInvalidValue;
	if (!(l1 >= T(0)) || !(l2 >= T(0)) || !std::isfinite(l1) || !std::isfinite(l2)) return hipErrorInvalidValue;
	// the momentum coefficients do not depend on the data: in double here, rounded to T for the kernel
	double c[APG_STEPS_MAX];
	apg_momentum(steps, c);
	ApgCoef<T> coef;
	for (int t = 0; t < APG_STEPS_MAX; ++t) coef.c[t] = t < steps ? (T)c[t] : T(0);
	switch (RP) {
	case 64: return apg_at<T, 64>(P, slabs, S, slab_stride, G, r, len_pad, len_valid, ps, sumsq_part, stream, l1, l2, steps, coef);
	case 128: return apg_at<T, 128>(P, slabs, S, slab_stride, G, r, len_pad, len_valid, ps, sumsq_part, stream, l1, l2, steps, coef);
	}
	return hipErrorInvalidValue;
}
template hipError_t launch_panel_steps_apg<float>(float*, const float*, int, long, const float*, int, int, int, int, float*, float*, hipStream_t, float, float, int);
template hipError_t launch_panel_steps_apg<double>(double*, const double*, int, long, const double*, int, int, int, int, double*, double*, hipStream_t, double, double, int);

} // namespace nmfamd
