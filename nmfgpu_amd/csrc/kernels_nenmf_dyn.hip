// kernels_nenmf_dyn.hip -- NeNMF with per-column dynamic stopping of the projected-gradient steps (docs/NENMF.md, "Dynamic stopping"), in one launch.
//
// k_apg_steps_dyn is a kernel of its own with the geometry, the prologue, the L computation, the product loop and the epilogue of k_apg_steps (kernels_nenmf.hip,
// which stays as it is: the geometry is restated here word for word); `steps` is the MAXIMUM number of steps.  For fixed G, a, L and momentum coefficients the
// columns of a panel are independent problems, so the rule is per column: with d_t = sum_k (P_{t+1}[k] - Y_t[k])^2 (L sqrt(d_t) is the norm of the gradient
// mapping at Y_t) a column is frozen after step t when d_t <= tol2 d_0 (tol2 = delta^2 rounded to T by the launcher); its result is P_{t+1}, and it is never
// stepped again.  The step arithmetic is that of k_apg_steps in its order: a column that is never frozen carries the bits of the static launch.
//
// d_t: a column is spread over the four waves and the four lane groups q of each.  A lane sums the squares of its own rows, an xor butterfly over q forms the
// wave's partial (the same bits in its four lanes), and the lanes of q = 0 leave it in s_d[t & 1][wave][column].  Behind the barrier that step t + 1 has anyway
// (the one after the write of Y_{t+1}) every thread adds the four partials of its columns in wave order: the same bits in every thread that holds a part of the
// column, so threshold, count and `live` are per-thread registers that agree without being exchanged.  The rule for step t is therefore applied inside step
// t + 1, before its update: a column frozen by d_t had its Y_{t+1} extrapolated and written, which nothing reads but the product whose result is dropped.
// The row of parity t is written again at the end of step t + 2, which a wave reaches only behind the barrier of t + 2, that is behind every wave's reads in t + 1.
//
// Leaving the loop is a WORKGROUP-uniform decision without a vote: every wave holds a part of all COLS columns, so each computes the same `live` bits from the
// same LDS words and `__any` is the same in all four.  The exit lags the last freeze by the write of one Y and one barrier; no product is formed for it.
// No barrier is added to those of k_apg_steps, and no atomics: a repeated launch is bit-identical.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <limits>

#include "kernels.h"
#include "split3.h"

namespace nmfamd {

// (from here to apg_row: the text of kernels_nenmf.hip)
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

constexpr int APG_WAVES = APG_THREADS / 64;

template <typename T, int RP, bool PEN>
__global__ __launch_bounds__(APG_THREADS) void k_apg_steps_dyn(T* __restrict__ P, const T* __restrict__ slabs, int S, long slab_stride, const T* __restrict__ G, int r,
                                                               int len_valid, T* __restrict__ ps, T* __restrict__ sumsq_part, T l1_arg, T l2_arg, int steps, ApgCoef<T> coef,
                                                               T tol2_arg, int* __restrict__ counts) {
	using Gm = ApgGeom<T, RP>;
	constexpr int COLS = Gm::COLS, VEC = Gm::VEC, KB = Gm::KB, LD = Gm::LD, RW = Gm::RW, CT = Gm::CT, NBUF = Gm::NBUF;
	typedef T TV __attribute__((ext_vector_type(VEC)));
	typedef typename ApgAcc<T>::V4 V4;
	__shared__ __attribute__((aligned(16))) T sG[RP * LD];
	__shared__ __attribute__((aligned(16))) T sY[NBUF * COLS * LD];
	__shared__ T s_d[2][APG_WAVES][COLS];            // the waves' parts of d_t per column, by the parity of t
	static_assert((RP + NBUF * COLS) * LD * (int)sizeof(T) + (int)sizeof(T) * 2 * APG_WAVES * COLS <= 160 * 1024, "G, Y and the parts of d fit LDS");
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, c16 = lane & 15;
	const long y0 = (long)blockIdx.x * COLS;

	// (VGPRs: a uniform argument meets per-lane values below, split3.h)
	const T l1 = PEN ? in_vgpr(l1_arg) : T(0), l2 = PEN ? in_vgpr(l2_arg) : T(0);
	const T tol2 = in_vgpr(tol2_arg);

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
	// the state of this thread's columns: live = not frozen, thr = tol2 d_0, cnt = steps applied.  A padding column is frozen at entry with count 0: its slabs
	// and panel rows were not read and must not keep the workgroup in the loop.
	bool live[CT];
	T thr[CT];
	int cnt[CT];
#pragma unroll
	for (int j = 0; j < CT; ++j) { live[j] = false; thr[j] = T(0); cnt[j] = 0; }

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
#pragma unroll
		for (int j = 0; j < CT; ++j) live[j] = y0 + 16 * j + c16 < len_valid;
		const int kblocks = (r + KB - 1) / KB;
		int t = 0;
		for (; t < steps; ++t) {                     // (uniform, 1 ... APG_STEPS_MAX; left early only by the uniform break below)
			T* buf = sY + (NBUF == 2 ? (t & 1) * COLS * LD : 0);
#pragma unroll
			for (int i = 0; i < RW; ++i)
#pragma unroll
				for (int j = 0; j < CT; ++j)
#pragma unroll
					for (int e = 0; e < 4; ++e) buf[(16 * j + c16) * LD + 16 * (wave * RW + i) + apg_row<T>(q, e)] = y[i][j][e];
			__syncthreads();
			if (t > 0) {
				// the rule for step t - 1: d in wave order, the same bits in every thread of the column
				bool mine = false;
#pragma unroll
				for (int j = 0; j < CT; ++j) {
					const T* part = &s_d[(t - 1) & 1][0][16 * j + c16];
					T d = part[0];
#pragma unroll
					for (int w = 1; w < APG_WAVES; ++w) d += part[w * COLS];
					if (live[j]) {
						if (t == 1) thr[j] = tol2 * d;
						if (d <= thr[j]) { live[j] = false; cnt[j] = t; }      // (at d_0 and tol2 < 1: only where the step moved nothing)
					}
					mine = mine || live[j];
				}
				if (!__any(mine)) break;                 // (uniform: every wave holds all COLS columns and read the same words)
			}
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
			for (int j = 0; j < CT; ++j) {
				T dsum = T(0);                           // this lane's part of d_t
#pragma unroll
				for (int i = 0; i < RW; ++i)
#pragma unroll
					for (int e = 0; e < 4; ++e) {
						const T yv = y[i][j][e];
						T g;
						if constexpr (PEN) g = (acc[i][j][e] - a[i][j][e]) + (l2 * yv + l1);
						else g = acc[i][j][e] - a[i][j][e];
						const T v = yv - g * inv;
						const T pn = v > T(0) ? v : T(0);
						const T moved = pn - yv;
						dsum += moved * moved;
						if (live[j]) {                       // (a frozen column: the product was formed, the step is not made)
							if (!last) y[i][j][e] = pn + c * (pn - p[i][j][e]);
							p[i][j][e] = pn;
						}
					}
				if (!last) {                             // (the count of a column that reaches the last step is `steps` whatever d is)
					dsum += __shfl_xor(dsum, 16, 64);
					dsum += __shfl_xor(dsum, 32, 64);
					if (q == 0) s_d[t & 1][wave][16 * j + c16] = dsum;
				}
			}
		}
#pragma unroll
		for (int j = 0; j < CT; ++j) { if (live[j]) cnt[j] = steps; }      // (live here: the loop ran to its end)
	}
	if (counts != nullptr && wave == 0 && q == 0) {
#pragma unroll
		for (int j = 0; j < CT; ++j) counts[y0 + 16 * j + c16] = cnt[j];      // (0 on padding, and where no step was taken)
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
static hipError_t apg_dyn_at(T* P, const T* slabs, int S, long slab_stride, const T* G, int r, int len_pad, int len_valid, T* ps, T* sumsq_part, hipStream_t stream, T l1,
                             T l2, int steps, const ApgCoef<T>& coef, T tol2, int* counts) {
	const dim3 grid(len_pad / ApgGeom<T, RP>::COLS);
	if (l1 != T(0) || l2 != T(0))
		hipLaunchKernelGGL((k_apg_steps_dyn<T, RP, true>), grid, dim3(APG_THREADS), 0, stream, P, slabs, S, slab_stride, G, r, len_valid, ps, sumsq_part, l1, l2, steps, coef, tol2,
		                   counts);
	else
		hipLaunchKernelGGL((k_apg_steps_dyn<T, RP, false>), grid, dim3(APG_THREADS), 0, stream, P, slabs, S, slab_stride, G, r, len_valid, ps, sumsq_part, T(0), T(0), steps, coef,
		                   tol2, counts);
	return hipGetLastError();
}

template <typename T>
hipError_t launch_panel_steps_apg_dyn(T* P, const T* slabs, int S, long slab_stride, const T* G, int RP, int r, int len_pad, int len_valid, T* ps, T* sumsq_part,
                                      hipStream_t stream, T l1, T l2, int steps, T tol, int* counts) {
	if (steps < APG_STEPS_MIN || steps > APG_STEPS_MAX) return hipErrorInvalidValue;
	if (!(tol > T(0) && tol < T(1))) return hipErrorInvalidValue;      // (NaN included; 0 is launch_panel_steps_apg, the caller's choice)
	if (!panel_steps_apg_available(RP, sizeof(T)) || S < 1 || r < 1 || r > RP || len_pad < 128 || len_pad % 128 != 0 || len_valid < 0 || len_valid > len_pad) return hipErrorInvalidValue;
	if (!(l1 >= T(0)) || !(l2 >= T(0)) || !std::isfinite(l1) || !std::isfinite(l2)) return hipErrorInvalidValue;
	// the momentum coefficients as launch_panel_steps_apg hands them over: in double, rounded to T for the kernel
	double c[APG_STEPS_MAX];
	apg_momentum(steps, c);
	ApgCoef<T> coef;
	for (int t = 0; t < APG_STEPS_MAX; ++t) coef.c[t] = t < steps ? (T)c[t] : T(0);
	const T tol2 = (T)((double)tol * (double)tol);   // delta^2, rounded once to the engine's precision (0 where it underflows: only a step that moves nothing freezes)
	switch (RP) {
	case 64: return apg_dyn_at<T, 64>(P, slabs, S, slab_stride, G, r, len_pad, len_valid, ps, sumsq_part, stream, l1, l2, steps, coef, tol2, counts);
	case 128: return apg_dyn_at<T, 128>(P, slabs, S, slab_stride, G, r, len_pad, len_valid, ps, sumsq_part, stream, l1, l2, steps, coef, tol2, counts);
	}
	return hipErrorInvalidValue;
}
template hipError_t launch_panel_steps_apg_dyn<float>(float*, const float*, int, long, const float*, int, int, int, int, float*, float*, hipStream_t, float, float, int, float, int*);
template hipError_t launch_panel_steps_apg_dyn<double>(double*, const double*, int, long, const double*, int, int, int, int, double*, double*, hipStream_t, double, double, int, double,
                                                       int*);

} // namespace nmfamd
