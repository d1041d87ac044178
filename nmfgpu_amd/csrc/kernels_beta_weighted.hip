// kernels_beta_weighted.hip -- the weighted form of the fused dense beta-divergence half-step (docs/DIVERGENCE.md, "Weighted update"): the objective is
// sum_ij w_ij d_beta(v_ij | P_ij), so with OX the image of the weights in the layout of X
//     num(o, c) = sum_k w(k, o) X(k, o) P(k, o)^(beta - 2) B(k, c),    den(o, c) = sum_k w(k, o) P(k, o)^(beta - 1) B(k, c)
// The kernels are those of kernels_beta.hip with one more image: the weight tile is loaded into the accumulator's layout exactly as the V tile is,
// an entry with weight 0 is selected out like padding (whatever V holds there, NaN included), every other entry's q, r and error terms are scaled by its weight,
// and the denominator is a second product at every beta (beta = 1: r = w, so it is no longer the column sums of B).  Same slab plan, same fixed summation order:
// a repeated run is bit-identical, and with every weight 1 the partial panels are those of the unweighted launch bit for bit (beta != 1).
// Kernels of their own, in a translation unit of their own: the unweighted launch keeps its argument list and its code object instruction for instruction (a
// body shared through a template flag was tried and rescheduled every unweighted kernel, docs/DIVERGENCE.md).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "kernels.h"
#include "split3.h"

namespace nmfamd {

typedef float betaw_f32x16 __attribute__((ext_vector_type(16)));

constexpr int BETAW_GENERAL = 2;      // (the value of the BETA template parameter that takes beta at run time)

// p^y = exp2(y log2 p) for p > 0.  fp32: the hardware's log2 and exp2 (v_log_f32, v_exp_f32; P >= eps and V is not denormal where it matters, so their flush of
// denormals costs nothing) -- the relative error is about |y log2 p| 2^-24, which on factors of ordinary size is a few ulp (docs/DIVERGENCE.md)
__device__ inline float betaw_log2(float p) { return __builtin_amdgcn_logf(p); }
__device__ inline double betaw_log2(double p) { return log2(p); }
__device__ inline float betaw_exp2(float y) { return __builtin_amdgcn_exp2f(y); }
__device__ inline double betaw_exp2(double y) { return exp2(y); }

// the element-wise map and the error terms of one entry (x = v, w = its weight, p = (W H) + eps), kernels_beta.hip's beta_entry with the weight: entries on the padding
// or with weight 0 (the caller folds w > 0 into `valid`) are selected out -- zeros and no terms, whatever x holds; the terms are added as w times the unweighted
// term and q and rr leave scaled by w (beta = 1: rr = w).  With w = 1 every value is the unweighted one bit for bit (a product with 1 is exact).
template <typename T, int BETA, bool TERMS>
__device__ inline void betaw_entry(T x, T w, T p, bool valid, T be, T& q, T& rr, T& tf, T& td) {
	q = 0; rr = 0;
	if (!valid) return;
	if (BETA == 1) {
		q = x / p;
		if (TERMS) {
			const T d = x - p;
			tf += (w * d) * d;
			td += w * ((x > T(0) ? x * log(q) : T(0)) - x + p);
		}
		q *= w; rr = w;
	} else if (BETA == BETAW_GENERAL) {
		// t = p^(beta - 2); the divergence term (x^beta + (beta - 1) p^beta - beta x p^(beta - 1)) is left unscaled: the kernel divides the row sums by beta (beta - 1)
		const T t = betaw_exp2((be - T(2)) * betaw_log2(p));
		q = x * t;
		rr = t * p;
		if (TERMS) {
			const T d = x - p;
			tf += (w * d) * d;
			const T xb = x > T(0) ? betaw_exp2(be * betaw_log2(x)) : T(0);
			td += w * (xb + (be - T(1)) * (rr * p) - be * (x * rr));
		}
		q *= w; rr *= w;
	} else {
		const T ip = T(1) / p;
		rr = ip;
		q = x * ip * ip;
		if (TERMS) {
			const T d = x - p, ratio = x * ip;
			tf += (w * d) * d;
			td += w * (ratio - log(ratio) - T(1));
		}
		q *= w; rr *= w;
	}
}

// WO x WK waves: WO tiles of 32 output columns, WK tiles of 32 reduction rows per step (WO * WK = 4)
template <int RP, int BETA, bool UPDATE, bool TERMS, int WO, int WK>
__global__ __launch_bounds__(256) void k_beta_fused_w_f32(const float* __restrict__ X, const float* __restrict__ OX, long ldx, const float* __restrict__ A,
                                                    const float* __restrict__ B, float eps, float bexp,
                                                    float* __restrict__ num_part, float* __restrict__ den_part, long part_stride,
                                                    float* __restrict__ tf_part, float* __restrict__ td_part, long t_stride,
                                                    int out_valid, int red_valid, int tiles_total, int tiles_per_slab) {
	constexpr int LD = RP + 2, BO = 32 * WO, KT = 32 * WK, NC = RP / 32;
	static_assert(WO * WK == 4, "four waves");
	static_assert(BO * RP <= KT * LD, "the combine region lies over the B tile");
	extern __shared__ float betaw_smem[];
	float* As = betaw_smem;              // [BO][LD]
	float* Bs = betaw_smem + BO * LD;    // [KT][LD]
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int wo = wave % WO, wk = wave / WO;
	const int li = lane & 31, h = lane >> 5;
	const int o0 = blockIdx.x * BO, slab = blockIdx.y;
	const int tile_begin = slab * tiles_per_slab, tile_end = min(tile_begin + tiles_per_slab, tiles_total);
	const int o = o0 + 32 * wo + li;
	const float e_v = in_vgpr(eps);     // (a uniform argument meets vector values below: split3.h)
	const float b_v = BETA == BETAW_GENERAL ? in_vgpr(bexp) : 0.f;

	for (int idx = threadIdx.x * 4; idx < BO * RP; idx += 1024) {
		const int row = idx / RP, col = idx % RP;
		const float4 v = *reinterpret_cast<const float4*>(A + (long)(o0 + row) * RP + col);
		float* d = As + row * LD + col;
		d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
	}

	betaw_f32x16 num[NC], den[NC];
#pragma unroll
	for (int ct = 0; ct < NC; ++ct)
#pragma unroll
		for (int v = 0; v < 16; ++v) { num[ct][v] = 0.f; den[ct][v] = 0.f; }
	float tf = 0.f, td = 0.f;

	for (int tile = tile_begin; tile < tile_end; ++tile) {
		const int kt = tile * KT;
		__syncthreads();      // (the previous tile's readers are done; the first pass: As is complete below)
		for (int idx = threadIdx.x * 4; idx < KT * RP; idx += 1024) {
			const int row = idx / RP, col = idx % RP;
			const float4 v = *reinterpret_cast<const float4*>(B + (long)(kt + row) * RP + col);
			float* d = Bs + row * LD + col;
			d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
		}
		// the V tile in the accumulator's layout: x[4 g + e] = X(o, kt + 32 wk + 8 g + 4 h + e)
		float x[16];
		{
			const float* xr = X + (long)o * ldx + kt + 32 * wk + 4 * h;
#pragma unroll
			for (int g = 0; g < 4; ++g) {
				const float4 v = *reinterpret_cast<const float4*>(xr + 8 * g);
				x[4 * g] = v.x; x[4 * g + 1] = v.y; x[4 * g + 2] = v.z; x[4 * g + 3] = v.w;
			}
		}
		// ... and the weight tile, the same way
		float wx[16];
		{
			const float* wr = OX + (long)o * ldx + kt + 32 * wk + 4 * h;
#pragma unroll
			for (int g = 0; g < 4; ++g) {
				const float4 v = *reinterpret_cast<const float4*>(wr + 8 * g);
				wx[4 * g] = v.x; wx[4 * g + 1] = v.y; wx[4 * g + 2] = v.z; wx[4 * g + 3] = v.w;
			}
		}
		__syncthreads();
		// P(k, o) = sum_c B(k, c) A(o, c), c ascending
		betaw_f32x16 P;
#pragma unroll
		for (int v = 0; v < 16; ++v) P[v] = 0.f;
		{
			const float* bs = Bs + (32 * wk + li) * LD + h;
			const float* as = As + (32 * wo + li) * LD + h;
#pragma unroll 16
			for (int t = 0; t < RP / 2; ++t) P = __builtin_amdgcn_mfma_f32_32x32x2f32(bs[2 * t], as[2 * t], P, 0, 0, 0);
		}
		float q[16], rr[16];
#pragma unroll
		for (int v = 0; v < 16; ++v) {
			const int kk = kt + 32 * wk + (v & 3) + 8 * (v >> 2) + 4 * h;
			betaw_entry<float, BETA, TERMS>(x[v], wx[v], P[v] + e_v, kk < red_valid && o < out_valid && wx[v] > 0.f, b_v, q[v], rr[v], tf, td);
		}
		if (UPDATE) {
			const float* b2 = Bs + (32 * wk + 4 * h) * LD + li;
#pragma unroll
			for (int v = 0; v < 16; ++v) {
#pragma unroll
				for (int ct = 0; ct < NC; ++ct) {
					const float bop = b2[((v & 3) + 8 * (v >> 2)) * LD + 32 * ct];
					num[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(q[v], bop, num[ct], 0, 0, 0);
					den[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(rr[v], bop, den[ct], 0, 0, 0);
				}
			}
		}
	}
	__syncthreads();
	if (UPDATE) {
		// the WK waves of an output tile in wave order, through the region of the B tile; then the slab's partial panel rows, coalesced
		float* R = Bs;
#pragma unroll
		for (int pass = 0; pass < 2; ++pass) {
			for (int w = 0; w < WK; ++w) {
				if (wk == w) {
#pragma unroll
					for (int ct = 0; ct < NC; ++ct)
#pragma unroll
						for (int v = 0; v < 16; ++v) {
							const int idx = (32 * wo + (v & 3) + 8 * (v >> 2) + 4 * h) * RP + 32 * ct + li;
							const float mine = pass == 0 ? num[ct][v] : den[ct][v];
							R[idx] = w == 0 ? mine : R[idx] + mine;
						}
				}
				__syncthreads();
			}
			float* dst = (pass == 0 ? num_part : den_part) + (long)slab * part_stride + (long)o0 * RP;
			for (int idx = threadIdx.x; idx < BO * RP; idx += 256) dst[idx] = R[idx];
			__syncthreads();
		}
	}
	if (TERMS) {
		if (BETA == BETAW_GENERAL) td *= 1.f / (b_v * (b_v - 1.f));
		// lane halves (h = 0 then 1), then the WK waves in order
		const float of = __shfl_xor(tf, 32), od = __shfl_xor(td, 32);
		const float sf = h == 0 ? tf + of : of + tf, sd = h == 0 ? td + od : od + td;
		float* Ts = As;      // [WK][BO][2]
		if (h == 0) { Ts[(wk * BO + 32 * wo + li) * 2] = sf; Ts[(wk * BO + 32 * wo + li) * 2 + 1] = sd; }
		__syncthreads();
		if ((int)threadIdx.x < BO) {
			float a = 0.f, b = 0.f;
			for (int w = 0; w < WK; ++w) { a += Ts[(w * BO + threadIdx.x) * 2]; b += Ts[(w * BO + threadIdx.x) * 2 + 1]; }
			tf_part[(long)slab * t_stride + o0 + threadIdx.x] = a;
			td_part[(long)slab * t_stride + o0 + threadIdx.x] = b;
		}
	}
}

// The same half-step with plain FMAs (fp64: the parity form).  A workgroup owns 8 output columns and walks tiles of 32 reduction rows: thread (k, o) forms
// P(k, o) and the map, thread (o, c mod 32) then accumulates its RP / 32 numerators (and denominators) over the tile's rows in ascending k.
template <typename T, int RP, int BETA, bool UPDATE, bool TERMS>
__global__ __launch_bounds__(256) void k_beta_fused_w_valu(const T* __restrict__ X, const T* __restrict__ OX, long ldx, const T* __restrict__ A, const T* __restrict__ B,
                                                     T eps, T bexp, T* __restrict__ num_part, T* __restrict__ den_part, long part_stride,
                                                     T* __restrict__ tf_part, T* __restrict__ td_part, long t_stride,
                                                     int out_valid, int red_valid, int tiles_total, int tiles_per_slab) {
	constexpr int LD = RP + 1, BO = 8, KT = 32, NACC = RP / 32;
	extern __shared__ double betaw_smem_d[];
	T* As = reinterpret_cast<T*>(betaw_smem_d);      // [BO][LD]
	T* Bs = As + BO * LD;                           // [KT][LD]
	T* Qs = Bs + KT * LD;                           // [KT][BO]
	T* Rs = Qs + KT * BO;                           // [KT][BO]
	const int o0 = blockIdx.x * BO, slab = blockIdx.y;
	const int tile_begin = slab * tiles_per_slab, tile_end = min(tile_begin + tiles_per_slab, tiles_total);
	const int k1 = threadIdx.x & 31, o1 = threadIdx.x >> 5;      // both phases: o1 = the thread's output column
	const T e_v = in_vgpr(eps);
	const T b_v = BETA == BETAW_GENERAL ? in_vgpr(bexp) : T(0);
	for (int idx = threadIdx.x; idx < BO * RP; idx += 256) As[(idx / RP) * LD + idx % RP] = A[(long)o0 * RP + idx];
	T num[NACC], den[NACC];
#pragma unroll
	for (int u = 0; u < NACC; ++u) { num[u] = 0; den[u] = 0; }
	T tf = 0, td = 0;
	for (int tile = tile_begin; tile < tile_end; ++tile) {
		const int kt = tile * KT;
		__syncthreads();
		for (int idx = threadIdx.x; idx < KT * RP; idx += 256) Bs[(idx / RP) * LD + idx % RP] = B[(long)kt * RP + idx];
		const T x = X[(long)(o0 + o1) * ldx + kt + k1];
		const T wx = OX[(long)(o0 + o1) * ldx + kt + k1];
		__syncthreads();
		{
			T p = 0;
			const T* bs = Bs + k1 * LD;
			const T* as = As + o1 * LD;
			for (int c = 0; c < RP; ++c) p += bs[c] * as[c];
			T q, rr;
			betaw_entry<T, BETA, TERMS>(x, wx, p + e_v, kt + k1 < red_valid && o0 + o1 < out_valid && wx > T(0), b_v, q, rr, tf, td);
			Qs[k1 * BO + o1] = q;
			Rs[k1 * BO + o1] = rr;
		}
		__syncthreads();
		if (UPDATE) {
			for (int k = 0; k < KT; ++k) {
				const T q = Qs[k * BO + o1], rr = Rs[k * BO + o1];
#pragma unroll
				for (int u = 0; u < NACC; ++u) {
					const T b = Bs[k * LD + k1 + 32 * u];
					num[u] += q * b;
					den[u] += rr * b;
				}
			}
		}
	}
	if (UPDATE) {
#pragma unroll
		for (int u = 0; u < NACC; ++u) {
			const long at = (long)slab * part_stride + (long)(o0 + o1) * RP + k1 + 32 * u;
			num_part[at] = num[u];
			den_part[at] = den[u];
		}
	}
	if (TERMS) {
		// a column's 32 row residues in ascending order
		__syncthreads();
		Qs[k1 * BO + o1] = tf;
		Rs[k1 * BO + o1] = BETA == BETAW_GENERAL ? td / (b_v * (b_v - T(1))) : td;
		__syncthreads();
		if ((int)threadIdx.x < BO) {
			T a = 0, b = 0;
			for (int k = 0; k < KT; ++k) { a += Qs[k * BO + threadIdx.x]; b += Rs[k * BO + threadIdx.x]; }
			tf_part[(long)slab * t_stride + o0 + threadIdx.x] = a;
			td_part[(long)slab * t_stride + o0 + threadIdx.x] = b;
		}
	}
}

template <typename T>
hipError_t launch_beta_fused_weighted(const T* X, const T* OX, long ldx, const T* A, const T* B, int RP, double beta_value, bool update, bool terms, T eps,
                                      const BetaPlan& plan, T* num_part, T* den_part, long part_stride, T* tf_part, T* td_part, long t_stride,
                                      int out_pad, int out_valid, int red_valid, hipStream_t stream) {
	// (the checks of launch_beta_fused; the denominator panel is needed at every beta)
	const T bexp = (T)beta_value;
	const int beta = bexp == T(1) ? 1 : bexp == T(0) ? 0 : BETAW_GENERAL;
	if (X == nullptr || OX == nullptr || !beta_half_step_available(RP) || !std::isfinite((double)bexp) || (!update && !terms) || out_pad <= 0 || out_pad % 128 != 0 ||
	    plan.slabs < 1 || out_valid > out_pad || red_valid > (long)plan.tiles * plan.kt || ldx < (long)plan.tiles * plan.kt || ldx % 4 != 0)
		return hipErrorInvalidValue;
	if (update && (num_part == nullptr || den_part == nullptr)) return hipErrorInvalidValue;
	if (terms && (tf_part == nullptr || td_part == nullptr)) return hipErrorInvalidValue;
	const dim3 grid((unsigned)(out_pad / plan.bo), (unsigned)plan.slabs), block(256);
	hipError_t e = hipSuccess;
#define NMFAMD_BETAW_GO(KERNEL, BYTES)                                                                                                                     \
	do {                                                                                                                                                   \
		static std::atomic<unsigned long long> done{0};                                                                                                    \
		e = allow_dynamic_lds(reinterpret_cast<const void*>(&KERNEL), (int)(BYTES), done);                                                                 \
		if (e != hipSuccess) return e;                                                                                                                     \
		hipLaunchKernelGGL(KERNEL, grid, block, (size_t)(BYTES), stream, X, OX, ldx, A, B, eps, bexp, num_part, den_part, part_stride, tf_part, td_part,   \
		                   t_stride, out_valid, red_valid, plan.tiles, plan.tiles_per_slab);                                                               \
	} while (0)
#define NMFAMD_BETAW_FORMS(KERNEL_OF, BYTES)                                                                                                               \
	do {                                                                                                                                                   \
		if (beta == 1) {                                                                                                                                   \
			if (update && terms) NMFAMD_BETAW_GO((KERNEL_OF(1, true, true)), BYTES);                                                                       \
			else if (update) NMFAMD_BETAW_GO((KERNEL_OF(1, true, false)), BYTES);                                                                          \
			else NMFAMD_BETAW_GO((KERNEL_OF(1, false, true)), BYTES);                                                                                      \
		} else if (beta == BETAW_GENERAL) {                                                                                                                 \
			if (update && terms) NMFAMD_BETAW_GO((KERNEL_OF(BETAW_GENERAL, true, true)), BYTES);                                                            \
			else if (update) NMFAMD_BETAW_GO((KERNEL_OF(BETAW_GENERAL, true, false)), BYTES);                                                               \
			else NMFAMD_BETAW_GO((KERNEL_OF(BETAW_GENERAL, false, true)), BYTES);                                                                           \
		} else {                                                                                                                                           \
			if (update && terms) NMFAMD_BETAW_GO((KERNEL_OF(0, true, true)), BYTES);                                                                       \
			else if (update) NMFAMD_BETAW_GO((KERNEL_OF(0, true, false)), BYTES);                                                                          \
			else NMFAMD_BETAW_GO((KERNEL_OF(0, false, true)), BYTES);                                                                                      \
		}                                                                                                                                                  \
	} while (0)
	if constexpr (sizeof(T) == 4) {
		if (plan.bo != (RP == 256 ? 64 : 32) || plan.kt != (RP == 256 ? 64 : 128)) return hipErrorInvalidValue;
#define NMFAMD_BETAW_F32_64(B_, U_, T_) k_beta_fused_w_f32<64, B_, U_, T_, 1, 4>
#define NMFAMD_BETAW_F32_128(B_, U_, T_) k_beta_fused_w_f32<128, B_, U_, T_, 1, 4>
#define NMFAMD_BETAW_F32_256(B_, U_, T_) k_beta_fused_w_f32<256, B_, U_, T_, 2, 2>
		// (the LDS of the unweighted launch: the weight tile lives in registers)
		switch (RP) {
		case 64: NMFAMD_BETAW_FORMS(NMFAMD_BETAW_F32_64, sizeof(float) * (size_t)(32 * 1 + 32 * 4) * (64 + 2)); break;
		case 128: NMFAMD_BETAW_FORMS(NMFAMD_BETAW_F32_128, sizeof(float) * (size_t)(32 * 1 + 32 * 4) * (128 + 2)); break;
		default: NMFAMD_BETAW_FORMS(NMFAMD_BETAW_F32_256, sizeof(float) * (size_t)(32 * 2 + 32 * 2) * (256 + 2)); break;
		}
#undef NMFAMD_BETAW_F32_64
#undef NMFAMD_BETAW_F32_128
#undef NMFAMD_BETAW_F32_256
	} else {
		if (plan.bo != 8 || plan.kt != 32) return hipErrorInvalidValue;
#define NMFAMD_BETAW_F64_64(B_, U_, T_) k_beta_fused_w_valu<T, 64, B_, U_, T_>
#define NMFAMD_BETAW_F64_128(B_, U_, T_) k_beta_fused_w_valu<T, 128, B_, U_, T_>
#define NMFAMD_BETAW_F64_256(B_, U_, T_) k_beta_fused_w_valu<T, 256, B_, U_, T_>
		switch (RP) {
		case 64: NMFAMD_BETAW_FORMS(NMFAMD_BETAW_F64_64, sizeof(T) * (size_t)((8 + 32) * (64 + 1) + 2 * 32 * 8)); break;
		case 128: NMFAMD_BETAW_FORMS(NMFAMD_BETAW_F64_128, sizeof(T) * (size_t)((8 + 32) * (128 + 1) + 2 * 32 * 8)); break;
		default: NMFAMD_BETAW_FORMS(NMFAMD_BETAW_F64_256, sizeof(T) * (size_t)((8 + 32) * (256 + 1) + 2 * 32 * 8)); break;
		}
#undef NMFAMD_BETAW_F64_64
#undef NMFAMD_BETAW_F64_128
#undef NMFAMD_BETAW_F64_256
	}
#undef NMFAMD_BETAW_FORMS
#undef NMFAMD_BETAW_GO
	return hipGetLastError();
}
template hipError_t launch_beta_fused_weighted<float>(const float*, const float*, long, const float*, const float*, int, double, bool, bool, float, const BetaPlan&, float*, float*,
                                                      long, float*, float*, long, int, int, int, hipStream_t);
template hipError_t launch_beta_fused_weighted<double>(const double*, const double*, long, const double*, const double*, int, double, bool, bool, double, const BetaPlan&, double*,
                                                       double*, long, double*, double*, long, int, int, int, hipStream_t);

} // namespace nmfamd
