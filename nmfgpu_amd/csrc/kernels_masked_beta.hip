// kernels_masked_beta.hip -- missing-value NMF under the beta-divergence: the multiplicative update of docs/DIVERGENCE.md ("Weighted update", 0 / 1 weights) with
// both sums over the OBSERVED entries of V only (docs/MISSING.md, "Beta-divergence").
//
// Omega = the stored entries of the sparse images (CSR + CSC, built once per upload).  Per output row, with p = A(row, :) . B(idx_p, :) + eps over the row's
// stored entries:
//     num = sum_p v_p p^(beta - 2) B(idx_p, :),   den = sum_p p^(beta - 1) B(idx_p, :),   A(row, :) <- A(row, :) .* (num ./ (den + eps + l1 + l2 A(row, :)))^gamma
//     H step (CSC image, A = H,  B = Wt), W step (CSR image, A = Wt, B = H); gamma = 1 / (2 - beta) below beta = 1, 1 up to beta = 2, 1 / (beta - 1) above
// Layout and the order of every sum are k_masked_fused's (kernels_masked.hip): one wave per output row, a group of 16 lanes owns one stored entry (two per group in
// flight), each lane SEG = RP / 16 contiguous factor rows, a 4-step butterfly forms the dot product, per-group running sums in entry order, groups
// (g0 + g1) + (g2 + g3); no atomics -- a repeated run is bit-identical.  After the butterfly the group forms the element-wise map once per entry:
//     BETA_KL       q = v / p                                  r = 1
//     BETA_IS       ip = 1 / p, q = v ip ip                    r = ip
//     BETA_GENERAL  t = exp2((beta - 2) log2 p), q = v t       r = t p
// and accumulates num += q B(idx_p, :), den += r B(idx_p, :) while the gathered row sits in registers.  An entry slot past the end of a row is SELECTED out (q = r = 0
// by selection, never a product with zero: p = eps there makes p^(beta - 2) huge).  The owning wave applies the quotient, the penalties and gamma in place: no
// other wave of the launch reads that row, so no numerator or denominator panel exists.
// An empty row has num = den = 0 and becomes 0 (a zero quotient stays 0 at every gamma); padding coordinates (c >= r) are 0 in A and in B and stay 0; padding rows
// are not touched.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "kernels.h"
#include "split3.h"

namespace nmfamd {

constexpr int BETA_IS = 0, BETA_KL = 1, BETA_GENERAL = 2;      // the element-wise map (BETA_GENERAL takes beta at run time), numbered as in kernels_beta.hip

// p^y = exp2(y log2 p) for p > 0, as k_beta_fused_* has it: fp32 on the hardware's log2 and exp2 (v_log_f32, v_exp_f32; p >= eps, so their flush of denormals is
// never met), fp64 on log2 / exp2
__device__ inline float mb_log2(float p) { return __builtin_amdgcn_logf(p); }
__device__ inline double mb_log2(double p) { return log2(p); }
__device__ inline float mb_exp2(float y) { return __builtin_amdgcn_exp2f(y); }
__device__ inline double mb_exp2(double y) { return exp2(y); }

// The map of one entry (x = v_p, p = the dot product + eps) and, with TERMS, its two error terms: (x - p)^2 and d_beta(x | p) -- the general form UNSCALED
// (x^beta + (beta - 1) p^beta - beta x p^(beta - 1), x^beta = 0 at x = 0): the wave divides the row sum by beta (beta - 1) once.
template <typename T, int BETA, bool TERMS>
__device__ inline void masked_beta_entry(T x, T p, T be, T& q, T& rr, T& tf, T& td) {
	if (BETA == BETA_KL) {
		q = x / p;
		rr = T(1);
		if (TERMS) {
			const T d = x - p;
			tf = d * d;
			td = (x > T(0) ? x * log(q) : T(0)) - x + p;
		}
	} else if (BETA == BETA_GENERAL) {
		const T t = mb_exp2((be - T(2)) * mb_log2(p));
		q = x * t;
		rr = t * p;
		if (TERMS) {
			const T d = x - p;
			tf = d * d;
			const T xb = x > T(0) ? mb_exp2(be * mb_log2(x)) : T(0);
			td = xb + (be - T(1)) * (rr * p) - be * (x * rr);
		}
	} else {
		const T ip = T(1) / p;
		rr = ip;
		q = x * ip * ip;
		if (TERMS) {
			const T d = x - p, ratio = x * ip;
			tf = d * d;
			td = ratio - log(ratio) - T(1);
		}
	}
}

// UPDATE: write the updated rows of A (false: the terms-only form of the errors under constant W).  TERMS: t_frob(row) = sum_p (v_p - p)^2 and t_div(row) =
// sum_p d_beta(v_p | p) with the OLD row of A.  power: 0 gamma = 1, 1 gamma = 1/2 (a square root), 2 any other gamma.  sumsq_part != nullptr (UPDATE only):
// per-workgroup partial sums of squares of the new rows, one RP vector per workgroup -- the workgroups then stride over the row groups, so the count of partials is
// the grid, a function of the row count only (masked_norm_parts).
template <typename T, int VEC, int BETA, bool UPDATE, bool TERMS>
__global__ __launch_bounds__(256) void k_masked_beta_fused(const int* __restrict__ ptr, const int* __restrict__ idx, const T* __restrict__ val,
                                                           T* __restrict__ A, const T* __restrict__ B, T eps, T bexp, T l1, T l2, T gamma, int power,
                                                           T* __restrict__ t_frob, T* __restrict__ t_div, T* __restrict__ sumsq_part, int rows, int row_groups) {
	constexpr int RP = 64 * VEC, SEG = 4 * VEC;
	__shared__ T s_sq[4][RP];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int g = lane >> 4, sl = lane & 15;
	// (uniform arguments meet vector values below: split3.h)
	const T e_v = in_vgpr(eps), b_v = BETA == BETA_GENERAL ? in_vgpr(bexp) : T(0);
	const T l1_v = in_vgpr(l1), l2_v = in_vgpr(l2), g_v = in_vgpr(gamma);
	T sq[SEG];
#pragma unroll
	for (int e = 0; e < SEG; ++e) sq[e] = 0;
	for (int rg = blockIdx.x; rg < row_groups; rg += gridDim.x) {
		const int row = rg * 4 + wave;
		if (row >= rows) continue;     // (wave-uniform)
		T a[SEG], num[SEG], den[SEG];
#pragma unroll
		for (int e = 0; e < SEG; ++e) { a[e] = A[(long)row * RP + sl * SEG + e]; num[e] = 0; den[e] = 0; }
		T s_frob = 0, s_div = 0;
		const int p_begin = ptr[row], p_end = ptr[row + 1];
		for (int p0 = p_begin; p0 < p_end; p0 += 8) {
			const int pa = p0 + g, pb = p0 + 4 + g;
			const bool va = pa < p_end, vb = pb < p_end;
			const int ja = idx[va ? pa : p_begin], jb = idx[vb ? pb : p_begin];
			// (a slot past the end reads the row's first entry and the value 1: finite arithmetic whose result is selected out below)
			const T xa = va ? val[pa] : T(1), xb = vb ? val[pb] : T(1);
			const T* ba = B + (long)ja * RP + sl * SEG;
			const T* bb = B + (long)jb * RP + sl * SEG;
			T ra[SEG], rb[SEG];
#pragma unroll
			for (int e = 0; e < SEG; ++e) { ra[e] = ba[e]; rb[e] = bb[e]; }
			T da = 0, db = 0;
#pragma unroll
			for (int e = 0; e < SEG; ++e) { da += a[e] * ra[e]; db += a[e] * rb[e]; }
#pragma unroll
			for (int w = 8; w > 0; w >>= 1) { da += __shfl_xor(da, w, 16); db += __shfl_xor(db, w, 16); }
			T qa, wa, fa = 0, ka = 0, qb, wb, fb = 0, kb = 0;
			masked_beta_entry<T, BETA, TERMS>(xa, da + e_v, b_v, qa, wa, fa, ka);
			masked_beta_entry<T, BETA, TERMS>(xb, db + e_v, b_v, qb, wb, fb, kb);
			// an entry past the end: no share of either sum, by selection
			qa = va ? qa : T(0); wa = va ? wa : T(0);
			qb = vb ? qb : T(0); wb = vb ? wb : T(0);
			if (UPDATE) {
#pragma unroll
				for (int e = 0; e < SEG; ++e) { num[e] += qa * ra[e]; den[e] += wa * ra[e]; }
#pragma unroll
				for (int e = 0; e < SEG; ++e) { num[e] += qb * rb[e]; den[e] += wb * rb[e]; }
			}
			if (TERMS && sl == 0) {
				if (va) { s_frob += fa; s_div += ka; }
				if (vb) { s_frob += fb; s_div += kb; }
			}
		}
		if (UPDATE) {
			// groups 0 .. 3 in order: (g0 + g1) + (g2 + g3) on every lane, then lanes 0 .. 15 hold the row
#pragma unroll
			for (int e = 0; e < SEG; ++e) {
				const T on = __shfl_xor(num[e], 16), od = __shfl_xor(den[e], 16);
				const T ln = (g & 1) ? on + num[e] : num[e] + on, ld = (g & 1) ? od + den[e] : den[e] + od;
				const T pn = __shfl_xor(ln, 32), pd = __shfl_xor(ld, 32);
				num[e] = (g & 2) ? pn + ln : ln + pn;
				den[e] = (g & 2) ? pd + ld : ld + pd;
			}
			if (g == 0) {
				T* dst = A + (long)row * RP + sl * SEG;
#pragma unroll
				for (int e = 0; e < SEG; ++e) {
					const T quo = num[e] / (den[e] + e_v + l1_v + l2_v * a[e]);
					T f = quo;
					if (power == 1) f = sqrt(quo);
					else if (power == 2) f = quo > T(0) ? exp2(g_v * log2(quo)) : T(0);      // (a zero quotient stays 0)
					const T v = a[e] * f;
					dst[e] = v;
					sq[e] += v * v;
				}
			}
		}
		if (TERMS) {
			const T f0 = __shfl(s_frob, 0), f1 = __shfl(s_frob, 16), f2 = __shfl(s_frob, 32), f3 = __shfl(s_frob, 48);
			const T d0 = __shfl(s_div, 0), d1 = __shfl(s_div, 16), d2 = __shfl(s_div, 32), d3 = __shfl(s_div, 48);
			if (lane == 0) {
				const T td = ((d0 + d1) + d2) + d3;
				t_frob[row] = ((f0 + f1) + f2) + f3;
				t_div[row] = BETA == BETA_GENERAL ? td / (b_v * (b_v - T(1))) : td;
			}
		}
	}
	if (UPDATE && sumsq_part != nullptr) {
		// the four waves' sums in wave order (a wave's rows were added in row order above)
		if (g == 0) {
#pragma unroll
			for (int e = 0; e < SEG; ++e) s_sq[wave][sl * SEG + e] = sq[e];
		}
		__syncthreads();
		if ((int)threadIdx.x < RP) {
			const int c = threadIdx.x;
			sumsq_part[(long)blockIdx.x * RP + c] = ((s_sq[0][c] + s_sq[1][c]) + s_sq[2][c]) + s_sq[3][c];
		}
	}
}

template <typename T>
hipError_t launch_masked_beta_half_step(const int* ptr, const int* idx, const T* val, T* A, const T* B, int RP, T eps, double beta_value, T l1, T l2, bool update,
                                        T* t_frob, T* t_div, T* sumsq_part, int rows, hipStream_t stream) {
	const bool terms = t_frob != nullptr;
	const double b = (double)(T)beta_value;      // (in the precision of T: a value that rounds to 0 or 1 there runs the Itakura-Saito or the KL map)
	if ((RP != 64 && RP != 128 && RP != 256) || rows <= 0 || (t_frob == nullptr) != (t_div == nullptr) || (!update && !terms) || (!update && sumsq_part != nullptr) || !std::isfinite(b) || !(l1 >= T(0)) ||
	    !(l2 >= T(0)) || !std::isfinite((double)l1) || !std::isfinite((double)l2))
		return hipErrorInvalidValue;
	// gamma: scikit-learn's rule (the majorise-minimise exponent of Fevotte & Idier 2011), as launch_beta_update
	const double gamma = b < 1.0 ? 1.0 / (2.0 - b) : b <= 2.0 ? 1.0 : 1.0 / (b - 1.0);
	const int power = gamma == 1.0 ? 0 : gamma == 0.5 ? 1 : 2;
	const int map = b == 1.0 ? BETA_KL : b == 0.0 ? BETA_IS : BETA_GENERAL;
	const int row_groups = (rows + 3) / 4;
	const dim3 grid((unsigned)(sumsq_part != nullptr ? masked_norm_parts(rows) : row_groups)), block(256);
#define NMFAMD_MB_GO(VEC, MAP, U, TR)                                                                                                                       \
	hipLaunchKernelGGL((k_masked_beta_fused<T, VEC, MAP, U, TR>), grid, block, 0, stream, ptr, idx, val, A, B, eps, (T)b, l1, l2, (T)gamma, power, t_frob, t_div, \
	                   sumsq_part, rows, row_groups)
#define NMFAMD_MB_FORM(VEC, MAP)                                   \
	if (update && terms) NMFAMD_MB_GO(VEC, MAP, true, true);        \
	else if (update) NMFAMD_MB_GO(VEC, MAP, true, false);           \
	else NMFAMD_MB_GO(VEC, MAP, false, true)
#define NMFAMD_MB_MAP(VEC)                                         \
	if (map == BETA_KL) { NMFAMD_MB_FORM(VEC, BETA_KL); }           \
	else if (map == BETA_IS) { NMFAMD_MB_FORM(VEC, BETA_IS); }      \
	else { NMFAMD_MB_FORM(VEC, BETA_GENERAL); }                     \
	break
	switch (RP / 64) {
	case 1: NMFAMD_MB_MAP(1);
	case 2: NMFAMD_MB_MAP(2);
	case 4: NMFAMD_MB_MAP(4);
	default: return hipErrorInvalidValue;      // padded ranks 64, 128, 256
	}
#undef NMFAMD_MB_MAP
#undef NMFAMD_MB_FORM
#undef NMFAMD_MB_GO
	return hipGetLastError();
}
template hipError_t launch_masked_beta_half_step<float>(const int*, const int*, const float*, float*, const float*, int, float, double, float, float, bool, float*, float*,
                                                        float*, int, hipStream_t);
template hipError_t launch_masked_beta_half_step<double>(const int*, const int*, const double*, double*, const double*, int, double, double, double, double, bool, double*,
                                                         double*, double*, int, hipStream_t);

} // namespace nmfamd
