// kernels_beta.hip -- dense beta-divergence NMF: the multiplicative update at beta = 1 (generalised KL), beta = 0 (Itakura-Saito) and any other real beta (the
// general form), with optional L1 / L2 penalties, on a dense resident V (docs/DIVERGENCE.md).
//
// One half-step, written once for both sides.  A is the panel that is updated ([out_pad][RP]: H in the H step, Wt in the W step), B the other panel
// ([red_pad][RP]), X the image of V with the output index as its row ([out_pad][ldx]: the column-major V in the H step, its transpose in the W step):
//     P(k, o) = sum_c B(k, c) A(o, c) + eps
//     beta = 1:  Q = X ./ P                      num(o, c) = sum_k Q(k, o) B(k, c)                                   den(c) = sum_k B(k, c)  (a vector: the caller's)
//     beta = 0:  Q = X ./ P^2,  R = 1 ./ P       num(o, c) = sum_k Q(k, o) B(k, c),  den(o, c) = sum_k R(k, o) B(k, c)
//     general:   Q = X .* P^(beta - 2),  R = P^(beta - 1)   the same two products as beta = 0
//     A(o, c) <- A(o, c) (num / (den + eps + l1 + l2 A(o, c)))^gamma,   gamma = 1 / (2 - beta) below beta = 1, 1 up to beta = 2, 1 / (beta - 1) above
// The template parameter BETA names the element-wise map: 1, 0, or BETA_GENERAL with beta a kernel argument.
// k_beta_fused_* forms P tile by tile, applies the element-wise map with the V tile in registers and accumulates num (and den): P, Q and R never reach HBM and V is
// read once.  The reduction index is cut into slabs (blockIdx.y) so that a launch has a few hundred workgroups whatever the shape; every slab writes its own partial
// panels and k_beta_update adds them in slab order, applies the update, zeroes the padding and leaves the per-workgroup sums the normalisation and the other
// side's KL denominator need.  Fixed order everywhere, no atomics: a repeated run is bit-identical.
//
// fp32 (k_beta_fused_f32): both products on the matrix pipe with the exact fp32 MFMA (v_mfma_f32_32x32x2_f32).  The first product is oriented so that its
// accumulator IS the second product's A operand: D(k, o) of the 32 x 32 tile puts, in lane l, column o = l & 31 and rows k = (v & 3) + 8 (v >> 2) + 4 (l >> 5),
// v = 0 .. 15; the second product's A operand wants, in lane l, row o = l & 31 and the K index l >> 5 -- so its sixteen K-steps take register v of the mapped
// accumulator as it is, with B rows k(v, l >> 5) as the other operand.  No LDS round trip for Q.
// fp64 (k_beta_fused_valu): plain FMAs, the parity form.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "kernels.h"
#include "split3.h"

namespace nmfamd {

typedef float beta_f32x16 __attribute__((ext_vector_type(16)));

constexpr int BETA_GENERAL = 2;      // (the value of the BETA template parameter that takes beta at run time)

// p^y = exp2(y log2 p) for p > 0.  fp32: the hardware's log2 and exp2 (v_log_f32, v_exp_f32; P >= eps and V is not denormal where it matters, so their flush of
// denormals costs nothing) -- the relative error is about |y log2 p| 2^-24, which on factors of ordinary size is a few ulp (docs/DIVERGENCE.md)
__device__ inline float beta_log2(float p) { return __builtin_amdgcn_logf(p); }
__device__ inline double beta_log2(double p) { return log2(p); }
__device__ inline float beta_exp2(float y) { return __builtin_amdgcn_exp2f(y); }
__device__ inline double beta_exp2(double y) { return exp2(y); }

// the element-wise map and the error terms of one entry (x = v, p = (W H) + eps); padding entries (valid = false) give zeros and no terms
template <typename T, int BETA, bool TERMS>
__device__ inline void beta_entry(T x, T p, bool valid, T be, T& q, T& rr, T& tf, T& td) {
	q = 0; rr = 0;
	if (!valid) return;
	if (BETA == 1) {
		q = x / p;
		if (TERMS) {
			const T d = x - p;
			tf += d * d;
			td += (x > T(0) ? x * log(q) : T(0)) - x + p;
		}
	} else if (BETA == BETA_GENERAL) {
		// t = p^(beta - 2); the divergence term (x^beta + (beta - 1) p^beta - beta x p^(beta - 1)) is left unscaled: the kernel divides the row sums by beta (beta - 1)
		const T t = beta_exp2((be - T(2)) * beta_log2(p));
		q = x * t;
		rr = t * p;
		if (TERMS) {
			const T d = x - p;
			tf += d * d;
			const T xb = x > T(0) ? beta_exp2(be * beta_log2(x)) : T(0);
			td += xb + (be - T(1)) * (rr * p) - be * (x * rr);
		}
	} else {
		const T ip = T(1) / p;
		rr = ip;
		q = x * ip * ip;
		if (TERMS) {
			const T d = x - p, ratio = x * ip;
			tf += d * d;
			td += ratio - log(ratio) - T(1);
		}
	}
}

// WO x WK waves: WO tiles of 32 output columns, WK tiles of 32 reduction rows per step (WO * WK = 4)
template <int RP, int BETA, bool UPDATE, bool TERMS, int WO, int WK>
__global__ __launch_bounds__(256) void k_beta_fused_f32(const float* __restrict__ X, long ldx, const float* __restrict__ A, const float* __restrict__ B, float eps, float bexp,
                                                        float* __restrict__ num_part, float* __restrict__ den_part, long part_stride,
                                                        float* __restrict__ tf_part, float* __restrict__ td_part, long t_stride,
                                                        int out_valid, int red_valid, int tiles_total, int tiles_per_slab) {
	constexpr int LD = RP + 2, BO = 32 * WO, KT = 32 * WK, NC = RP / 32;
	static_assert(WO * WK == 4, "four waves");
	static_assert(BO * RP <= KT * LD, "the combine region lies over the B tile");
	extern __shared__ float beta_smem[];
	float* As = beta_smem;              // [BO][LD]
	float* Bs = beta_smem + BO * LD;    // [KT][LD]
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int wo = wave % WO, wk = wave / WO;
	const int li = lane & 31, h = lane >> 5;
	const int o0 = blockIdx.x * BO, slab = blockIdx.y;
	const int tile_begin = slab * tiles_per_slab, tile_end = min(tile_begin + tiles_per_slab, tiles_total);
	const int o = o0 + 32 * wo + li;
	const float e_v = in_vgpr(eps);     // (a uniform argument meets vector values below: split3.h)
	const float b_v = BETA == BETA_GENERAL ? in_vgpr(bexp) : 0.f;

	for (int idx = threadIdx.x * 4; idx < BO * RP; idx += 1024) {
		const int row = idx / RP, col = idx % RP;
		const float4 v = *reinterpret_cast<const float4*>(A + (long)(o0 + row) * RP + col);
		float* d = As + row * LD + col;
		d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
	}

	beta_f32x16 num[NC], den[NC];
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
		__syncthreads();
		// P(k, o) = sum_c B(k, c) A(o, c), c ascending
		beta_f32x16 P;
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
			beta_entry<float, BETA, TERMS>(x[v], P[v] + e_v, kk < red_valid && o < out_valid, b_v, q[v], rr[v], tf, td);
		}
		if (UPDATE) {
			const float* b2 = Bs + (32 * wk + 4 * h) * LD + li;
#pragma unroll
			for (int v = 0; v < 16; ++v) {
#pragma unroll
				for (int ct = 0; ct < NC; ++ct) {
					const float bop = b2[((v & 3) + 8 * (v >> 2)) * LD + 32 * ct];
					num[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(q[v], bop, num[ct], 0, 0, 0);
					if (BETA != 1) den[ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(rr[v], bop, den[ct], 0, 0, 0);
				}
			}
		}
	}
	__syncthreads();
	if (UPDATE) {
		// the WK waves of an output tile in wave order, through the region of the B tile; then the slab's partial panel rows, coalesced
		float* R = Bs;
#pragma unroll
		for (int pass = 0; pass < (BETA != 1 ? 2 : 1); ++pass) {
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
		if (BETA == BETA_GENERAL) td *= 1.f / (b_v * (b_v - 1.f));
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
__global__ __launch_bounds__(256) void k_beta_fused_valu(const T* __restrict__ X, long ldx, const T* __restrict__ A, const T* __restrict__ B, T eps, T bexp,
                                                         T* __restrict__ num_part, T* __restrict__ den_part, long part_stride,
                                                         T* __restrict__ tf_part, T* __restrict__ td_part, long t_stride,
                                                         int out_valid, int red_valid, int tiles_total, int tiles_per_slab) {
	constexpr int LD = RP + 1, BO = 8, KT = 32, NACC = RP / 32;
	extern __shared__ double beta_smem_d[];
	T* As = reinterpret_cast<T*>(beta_smem_d);      // [BO][LD]
	T* Bs = As + BO * LD;                           // [KT][LD]
	T* Qs = Bs + KT * LD;                           // [KT][BO]
	T* Rs = Qs + KT * BO;                           // [KT][BO]
	const int o0 = blockIdx.x * BO, slab = blockIdx.y;
	const int tile_begin = slab * tiles_per_slab, tile_end = min(tile_begin + tiles_per_slab, tiles_total);
	const int k1 = threadIdx.x & 31, o1 = threadIdx.x >> 5;      // both phases: o1 = the thread's output column
	const T e_v = in_vgpr(eps);
	const T b_v = BETA == BETA_GENERAL ? in_vgpr(bexp) : T(0);
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
		__syncthreads();
		{
			T p = 0;
			const T* bs = Bs + k1 * LD;
			const T* as = As + o1 * LD;
			for (int c = 0; c < RP; ++c) p += bs[c] * as[c];
			T q, rr;
			beta_entry<T, BETA, TERMS>(x, p + e_v, kt + k1 < red_valid && o0 + o1 < out_valid, b_v, q, rr, tf, td);
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
					if (BETA != 1) den[u] += rr * b;
				}
			}
		}
	}
	if (UPDATE) {
#pragma unroll
		for (int u = 0; u < NACC; ++u) {
			const long at = (long)slab * part_stride + (long)(o0 + o1) * RP + k1 + 32 * u;
			num_part[at] = num[u];
			if (BETA != 1) den_part[at] = den[u];
		}
	}
	if (TERMS) {
		// a column's 32 row residues in ascending order
		__syncthreads();
		Qs[k1 * BO + o1] = tf;
		Rs[k1 * BO + o1] = BETA == BETA_GENERAL ? td / (b_v * (b_v - T(1))) : td;
		__syncthreads();
		if ((int)threadIdx.x < BO) {
			T a = 0, b = 0;
			for (int k = 0; k < KT; ++k) { a += Qs[k * BO + threadIdx.x]; b += Rs[k * BO + threadIdx.x]; }
			tf_part[(long)slab * t_stride + o0 + threadIdx.x] = a;
			td_part[(long)slab * t_stride + o0 + threadIdx.x] = b;
		}
	}
}

// The slabs in order, then A(o, c) <- A(o, c) (num / (den + eps + l1 + l2 A(o, c)))^gamma on the valid coordinates and 0 on the padding; one workgroup per 128
// panel rows, which leaves its sums of squares and sums of the new values (sumsq_part, sum_part: [out_pad / 128][RP]) and, on error iterations, the rows' error terms.
// vec_den: the denominator is the vector dsum (beta = 1), else the slabs' den_part.  power: 0 gamma = 1, 1 gamma = 1/2 (a square root), 2 any other gamma (a zero
// quotient stays 0).  EXT = false is the launch beta = 0 and beta = 1 always had (no penalty, power 0 or 1: the same instructions, so the same bits and the same
// time); EXT = true carries the penalties and the general power, whose code would otherwise sit in that launch's row loop.
template <typename T, bool EXT>
__global__ __launch_bounds__(256) void k_beta_update(T* __restrict__ A, const T* __restrict__ num_part, const T* __restrict__ den_part, long part_stride, int slabs,
                                                     const T* __restrict__ dsum, int RP, int r, int out_valid, T eps, int vec_den, int power, T gamma,
                                                     int penalised, T l1, T l2, int update, T* __restrict__ sumsq_part, T* __restrict__ sum_part,
                                                     const T* __restrict__ tf_part, const T* __restrict__ td_part, long t_stride, T* __restrict__ t_frob, T* __restrict__ t_div) {
	__shared__ T s_sq[256], s_sm[256];
	const int G = 256 / RP, c = threadIdx.x % RP, g = threadIdx.x / RP;
	const int row0 = blockIdx.x * 128;
	const T e_v = in_vgpr(eps);
	const T g_v = EXT ? in_vgpr(gamma) : T(0), l1_v = EXT ? in_vgpr(l1) : T(0), l2_v = EXT ? in_vgpr(l2) : T(0);
	if (update) {
		T sq = 0, sm = 0;
		const T dvec = vec_den ? dsum[c] : T(0);
		for (int row = row0 + g; row < row0 + 128; row += G) {
			const long idx = (long)row * RP + c;
			T nu = 0, de = 0;
			for (int s = 0; s < slabs; ++s) {
				nu += num_part[(long)s * part_stride + idx];
				if (!vec_den) de += den_part[(long)s * part_stride + idx];
			}
			if (vec_den) de = dvec;
			T v = 0;
			if (row < out_valid && c < r) {
				if (!EXT) {
					const T quo = nu / (de + e_v);
					v = A[idx] * (power == 1 ? sqrt(quo) : quo);
				} else {
					const T a = A[idx];
					const T quo = penalised ? nu / (de + e_v + l1_v + l2_v * a) : nu / (de + e_v);
					T f = quo;
					if (power == 1) f = sqrt(quo);
					else if (power == 2) f = quo > T(0) ? exp2(g_v * log2(quo)) : T(0);
					v = a * f;
				}
			}
			A[idx] = v;
			sq += v * v;
			sm += v;
		}
		s_sq[threadIdx.x] = sq; s_sm[threadIdx.x] = sm;
		__syncthreads();
		if ((int)threadIdx.x < RP) {
			T a = s_sq[c], b = s_sm[c];
			for (int k = 1; k < G; ++k) { a += s_sq[k * RP + c]; b += s_sm[k * RP + c]; }
			if (sumsq_part != nullptr) sumsq_part[(long)blockIdx.x * RP + c] = a;
			if (sum_part != nullptr) sum_part[(long)blockIdx.x * RP + c] = b;
		}
	}
	if (t_frob != nullptr && (int)threadIdx.x < 128) {
		const int row = row0 + threadIdx.x;
		T a = 0, b = 0;
		for (int s = 0; s < slabs; ++s) { a += tf_part[(long)s * t_stride + row]; b += td_part[(long)s * t_stride + row]; }
		t_frob[row] = a;
		t_div[row] = b;
	}
}

bool beta_half_step_available(int RP) { return RP == 64 || RP == 128 || RP == 256; }

BetaPlan plan_beta_half_step(long out_pad, long red_pad, int RP, size_t elem_bytes, int num_cus, int force_slabs) {
	BetaPlan p;
	if (elem_bytes == 4) { p.bo = RP == 256 ? 64 : 32; p.kt = RP == 256 ? 64 : 128; }
	else { p.bo = 8; p.kt = 32; }
	p.tiles = (int)(red_pad / p.kt);
	const long oblocks = out_pad / p.bo;
	// The slab count, a function of the shape and the CU count only.  Residency is limited by the LDS (fp32: 42 KB per workgroup at RP = 64, three to a CU; 83 KB at
	// RP = 128 and 132 KB at RP = 256, one to a CU), but resident workgroups share the CU's one matrix pipe, so whether a CU's workgroups run side by side or one
	// after the other, a launch lasts about as long as the matrix-pipe work of its most loaded CU: the count is chosen for the largest share of useful work in the CU-rounds of the launch -- workgroups / (rounds x CUs),
	// times the tiles that do work over the tiles of the longest slab (uneven slabs), times per / (per + 1) for a workgroup's prologue and epilogue (about one
	// tile's time).  With fewer workgroups than CUs this prefers more slabs; with many it prefers counts whose workgroups fill whole rounds.
	long best = 1;
	if (force_slabs > 0) best = std::max<long>(1, std::min<long>(force_slabs, std::min<long>(p.tiles, BETA_MAX_SLABS)));
	else {
		double best_share = -1.0;
		for (long s = 1; s <= std::min<long>(p.tiles, BETA_MAX_SLABS); ++s) {
			const long per = (p.tiles + s - 1) / s;
			if ((p.tiles + per - 1) / per != s) continue;      // (this count collapses to a smaller one)
			const double wgs = (double)oblocks * (double)s;
			const double rounds = (double)((oblocks * s + num_cus - 1) / num_cus);
			const double share = wgs / (rounds * num_cus) * ((double)p.tiles / (double)(per * s)) * ((double)per / (double)(per + 1));
			if (share > best_share + 1e-9) { best_share = share; best = s; }
		}
	}
	p.tiles_per_slab = (int)((p.tiles + best - 1) / best);
	p.slabs = (p.tiles + p.tiles_per_slab - 1) / p.tiles_per_slab;
	return p;
}

template <typename T>
hipError_t launch_beta_fused(const T* X, long ldx, const T* A, const T* B, int RP, double beta_value, bool update, bool terms, T eps, const BetaPlan& plan,
                             T* num_part, T* den_part, long part_stride, T* tf_part, T* td_part, long t_stride,
                             int out_pad, int out_valid, int red_valid, hipStream_t stream) {
	// (beta is taken in the precision of T; 1 and 0 have their own element-wise maps, every other finite value runs the general one)
	const T bexp = (T)beta_value;
	const int beta = bexp == T(1) ? 1 : bexp == T(0) ? 0 : BETA_GENERAL;
	if (!beta_half_step_available(RP) || !std::isfinite((double)bexp) || (!update && !terms) || out_pad <= 0 || out_pad % 128 != 0 || plan.slabs < 1 ||
	    out_valid > out_pad || red_valid > (long)plan.tiles * plan.kt || ldx < (long)plan.tiles * plan.kt || ldx % 4 != 0)
		return hipErrorInvalidValue;
	if (update && (num_part == nullptr || (beta != 1 && den_part == nullptr))) return hipErrorInvalidValue;
	if (terms && (tf_part == nullptr || td_part == nullptr)) return hipErrorInvalidValue;
	const dim3 grid((unsigned)(out_pad / plan.bo), (unsigned)plan.slabs), block(256);
	hipError_t e = hipSuccess;
#define NMFAMD_BETA_GO(KERNEL, BYTES)                                                                                                                      \
	do {                                                                                                                                                   \
		static std::atomic<unsigned long long> done{0};                                                                                                    \
		e = allow_dynamic_lds(reinterpret_cast<const void*>(&KERNEL), (int)(BYTES), done);                                                                 \
		if (e != hipSuccess) return e;                                                                                                                     \
		hipLaunchKernelGGL(KERNEL, grid, block, (size_t)(BYTES), stream, X, ldx, A, B, eps, bexp, num_part, den_part, part_stride, tf_part, td_part, t_stride,   \
		                   out_valid, red_valid, plan.tiles, plan.tiles_per_slab);                                                                         \
	} while (0)
	if constexpr (sizeof(T) == 4) {
#define NMFAMD_BETA_F32(RPV, WO, WK)                                                                                                                       \
	do {                                                                                                                                                   \
		constexpr size_t bytes = sizeof(float) * (size_t)(32 * WO + 32 * WK) * (RPV + 2);                                                                  \
		if (beta == 1) {                                                                                                                                   \
			if (update && terms) NMFAMD_BETA_GO((k_beta_fused_f32<RPV, 1, true, true, WO, WK>), bytes);                                                    \
			else if (update) NMFAMD_BETA_GO((k_beta_fused_f32<RPV, 1, true, false, WO, WK>), bytes);                                                       \
			else NMFAMD_BETA_GO((k_beta_fused_f32<RPV, 1, false, true, WO, WK>), bytes);                                                                   \
		} else if (beta == BETA_GENERAL) { \
			if (update && terms) NMFAMD_BETA_GO((k_beta_fused_f32<RPV, BETA_GENERAL, true, true, WO, WK>), bytes); \
			else if (update) NMFAMD_BETA_GO((k_beta_fused_f32<RPV, BETA_GENERAL, true, false, WO, WK>), bytes); \
			else NMFAMD_BETA_GO((k_beta_fused_f32<RPV, BETA_GENERAL, false, true, WO, WK>), bytes); \
		} else {                                                                                                                                           \
			if (update && terms) NMFAMD_BETA_GO((k_beta_fused_f32<RPV, 0, true, true, WO, WK>), bytes);                                                    \
			else if (update) NMFAMD_BETA_GO((k_beta_fused_f32<RPV, 0, true, false, WO, WK>), bytes);                                                       \
			else NMFAMD_BETA_GO((k_beta_fused_f32<RPV, 0, false, true, WO, WK>), bytes);                                                                   \
		}                                                                                                                                                  \
	} while (0)
		if (plan.bo != (RP == 256 ? 64 : 32) || plan.kt != (RP == 256 ? 64 : 128)) return hipErrorInvalidValue;
		switch (RP) {
		case 64: NMFAMD_BETA_F32(64, 1, 4); break;
		case 128: NMFAMD_BETA_F32(128, 1, 4); break;
		default: NMFAMD_BETA_F32(256, 2, 2); break;
		}
#undef NMFAMD_BETA_F32
	} else {
#define NMFAMD_BETA_F64(RPV)                                                                                                                               \
	do {                                                                                                                                                   \
		constexpr size_t bytes = sizeof(T) * (size_t)((8 + 32) * (RPV + 1) + 2 * 32 * 8);                                                                  \
		if (beta == 1) {                                                                                                                                   \
			if (update && terms) NMFAMD_BETA_GO((k_beta_fused_valu<T, RPV, 1, true, true>), bytes);                                                        \
			else if (update) NMFAMD_BETA_GO((k_beta_fused_valu<T, RPV, 1, true, false>), bytes);                                                           \
			else NMFAMD_BETA_GO((k_beta_fused_valu<T, RPV, 1, false, true>), bytes);                                                                       \
		} else if (beta == BETA_GENERAL) { \
			if (update && terms) NMFAMD_BETA_GO((k_beta_fused_valu<T, RPV, BETA_GENERAL, true, true>), bytes); \
			else if (update) NMFAMD_BETA_GO((k_beta_fused_valu<T, RPV, BETA_GENERAL, true, false>), bytes); \
			else NMFAMD_BETA_GO((k_beta_fused_valu<T, RPV, BETA_GENERAL, false, true>), bytes); \
		} else {                                                                                                                                           \
			if (update && terms) NMFAMD_BETA_GO((k_beta_fused_valu<T, RPV, 0, true, true>), bytes);                                                        \
			else if (update) NMFAMD_BETA_GO((k_beta_fused_valu<T, RPV, 0, true, false>), bytes);                                                           \
			else NMFAMD_BETA_GO((k_beta_fused_valu<T, RPV, 0, false, true>), bytes);                                                                       \
		}                                                                                                                                                  \
	} while (0)
		if (plan.bo != 8 || plan.kt != 32) return hipErrorInvalidValue;
		switch (RP) {
		case 64: NMFAMD_BETA_F64(64); break;
		case 128: NMFAMD_BETA_F64(128); break;
		default: NMFAMD_BETA_F64(256); break;
		}
#undef NMFAMD_BETA_F64
	}
#undef NMFAMD_BETA_GO
	return hipGetLastError();
}
template hipError_t launch_beta_fused<float>(const float*, long, const float*, const float*, int, double, bool, bool, float, const BetaPlan&, float*, float*, long, float*, float*,
                                             long, int, int, int, hipStream_t);
template hipError_t launch_beta_fused<double>(const double*, long, const double*, const double*, int, double, bool, bool, double, const BetaPlan&, double*, double*, long, double*,
                                              double*, long, int, int, int, hipStream_t);

template <typename T>
hipError_t launch_beta_update(T* A, const T* num_part, const T* den_part, long part_stride, int slabs, const T* dsum, int RP, int r, int out_pad, int out_valid, T eps,
                              double beta_value, T l1, T l2, bool update, T* sumsq_part, T* sum_part, const T* tf_part, const T* td_part, long t_stride, T* t_frob,
                              T* t_div, hipStream_t stream, bool weighted) {
	// gamma: scikit-learn's rule (the majorise-minimise exponent of Fevotte & Idier 2011)
	const double b = (double)(T)beta_value;      // (in the precision of T, as launch_beta_fused takes it)
	const bool vec_den = b == 1.0 && !weighted;      // (weighted: the beta = 1 denominator is a panel like any other, and the launch is the EXT one at every beta)
	const double gamma = b < 1.0 ? 1.0 / (2.0 - b) : b <= 2.0 ? 1.0 : 1.0 / (b - 1.0);
	const int power = gamma == 1.0 ? 0 : gamma == 0.5 ? 1 : 2;
	const bool penalised = l1 != T(0) || l2 != T(0);
	if (!beta_half_step_available(RP) || !std::isfinite(b) || !(l1 >= T(0)) || !(l2 >= T(0)) || !std::isfinite((double)l1) || !std::isfinite((double)l2) ||
	    out_pad <= 0 || out_pad % 128 != 0 || slabs < 1 || r < 1 || r > RP)
		return hipErrorInvalidValue;
	if (update && (num_part == nullptr || (vec_den ? dsum == nullptr : den_part == nullptr))) return hipErrorInvalidValue;
	if ((t_frob == nullptr) != (t_div == nullptr) || (t_frob != nullptr && (tf_part == nullptr || td_part == nullptr)) || (!update && t_frob == nullptr)) return hipErrorInvalidValue;
	if (penalised || power == 2 || weighted)
		hipLaunchKernelGGL((k_beta_update<T, true>), dim3((unsigned)(out_pad / 128)), dim3(256), 0, stream, A, num_part, den_part, part_stride, slabs, dsum, RP, r, out_valid,
		                   eps, vec_den ? 1 : 0, power, (T)gamma, penalised ? 1 : 0, l1, l2, update ? 1 : 0, sumsq_part, sum_part, tf_part, td_part, t_stride, t_frob, t_div);
	else
		hipLaunchKernelGGL((k_beta_update<T, false>), dim3((unsigned)(out_pad / 128)), dim3(256), 0, stream, A, num_part, den_part, part_stride, slabs, dsum, RP, r, out_valid,
		                   eps, vec_den ? 1 : 0, power, (T)gamma, 0, T(0), T(0), update ? 1 : 0, sumsq_part, sum_part, tf_part, td_part, t_stride, t_frob, t_div);
	return hipGetLastError();
}
template hipError_t launch_beta_update<float>(float*, const float*, const float*, long, int, const float*, int, int, int, int, float, double, float, float, bool, float*, float*, const float*,
                                              const float*, long, float*, float*, hipStream_t, bool);
template hipError_t launch_beta_update<double>(double*, const double*, const double*, long, int, const double*, int, int, int, int, double, double, double, double, bool, double*, double*,
                                               const double*, const double*, long, double*, double*, hipStream_t, bool);

} // namespace nmfamd
