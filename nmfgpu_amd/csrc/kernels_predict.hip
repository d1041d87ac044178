// kernels_predict.hip -- the value of W H at coordinates the caller names, and the error over them (docs/PREDICT.md).
//
// A coordinate list of nnz entries (i_p, j_p), unsorted, duplicates counted once per copy; Wt (element (k, i) at [i * RP + k]) and H (element (k, j) at [j * RP + k])
// are the engine's padded panels.  Per entry
//     out[p] = sum_{k < r} W(i_p, k) H(k, j_p)                                       (no eps)
// and, with values v_p, the terms (v_p - out[p])^2, d_beta(v_p | out[p] + eps) and the sum of the absolute values of the summands of d_beta.
// Layout of k_masked_fused (kernels_masked.hip) without a CSR: 256 threads are sixteen groups of 16 lanes, a group owns one entry at a time with two in flight;
// per entry it gathers row i of Wt and column j of H -- RP contiguous elements each -- in 16-byte loads, lane q of the group taking chunk 16 c + q in round c.
// Coordinates k >= r are SELECTED out of the dot product (never multiplied by zero: the padding may hold anything), then a 4-step butterfly inside the group.
// Order of every sum: a lane's chunks in round order, the butterfly, per-group running sums of the terms in DOUBLE in entry order, the sixteen groups of a
// workgroup in group order; one triple of doubles per workgroup, which the host adds in workgroup order.  The grid is a function of nnz only and there are no
// float atomics: a repeated launch is bit-identical.
// An entry slot past nnz gathers entry 0 (nnz >= 1) and is selected out.  No index is checked here: k_predict_validate runs first, and the gather is launched
// only when it found every coordinate inside the matrix.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "kernels.h"
#include "split3.h"

namespace nmfamd {

// the element-wise map of an entry's divergence term, numbered as in kernels_masked_beta.hip; PREDICT_NONE: the squared error only
constexpr int PREDICT_IS = 0, PREDICT_KL = 1, PREDICT_GENERAL = 2, PREDICT_NONE = 3;

// p^y = exp2(y log2 p) for p > 0, as masked_beta_entry has it: fp32 on the hardware's log2 and exp2 (p >= eps, so their flush of denormals is never met), fp64 on
// log2 / exp2
__device__ inline float pe_log2(float p) { return __builtin_amdgcn_logf(p); }
__device__ inline double pe_log2(double p) { return log2(p); }
__device__ inline float pe_exp2(float y) { return __builtin_amdgcn_exp2f(y); }
__device__ inline double pe_exp2(double y) { return exp2(y); }
__device__ inline float pe_abs(float x) { return fabsf(x); }
__device__ inline double pe_abs(double x) { return fabs(x); }

// The terms of one entry (x = v_p, p = the prediction + eps), masked_beta_entry's TERMS arithmetic: td = d_beta(x | p), ta = the sum of the absolute values of its
// summands.  The general form is x^beta + (beta - 1) p^beta - beta x p^(beta - 1) over beta (beta - 1), x^beta = 0 at x = 0; beta = 2 runs it as it is.
template <typename T>
__device__ inline void predict_entry_terms(int map, T x, T p, T be, T& td, T& ta) {
	if (map == PREDICT_KL) {
		const T q = x / p;
		const T a = x > T(0) ? x * log(q) : T(0);
		td = a - x + p;
		ta = pe_abs(a) + pe_abs(x) + pe_abs(p);
	} else if (map == PREDICT_GENERAL) {
		const T t = pe_exp2((be - T(2)) * pe_log2(p));
		const T rr = t * p;
		const T xb = x > T(0) ? pe_exp2(be * pe_log2(x)) : T(0);
		const T s1 = (be - T(1)) * (rr * p), s2 = be * (x * rr), c = be * (be - T(1));
		td = (xb + s1 - s2) / c;
		ta = (pe_abs(xb) + pe_abs(s1) + pe_abs(s2)) / pe_abs(c);
	} else {
		const T ratio = x * (T(1) / p), l = log(ratio);
		td = ratio - l - T(1);
		ta = pe_abs(ratio) + pe_abs(l) + T(1);
	}
}

template <typename T> struct PredictChunk;
template <> struct PredictChunk<float> { typedef float type __attribute__((ext_vector_type(4))); };
template <> struct PredictChunk<double> { typedef double type __attribute__((ext_vector_type(2))); };

// ROUNDS: 16-byte chunks per lane and gathered row, RP = ROUNDS * 256 / sizeof(T).  TERMS: values are given; part[3 * blockIdx.x + {0, 1, 2}] = this workgroup's sums
// of (v - out)^2, of d_beta and of its absolute summands (map = PREDICT_NONE: the first only, the others 0).  out may be null with TERMS.  passes = ceil(nnz / 32).
template <typename T, int ROUNDS, bool TERMS>
__global__ __launch_bounds__(256) void k_predict_entries(const int* __restrict__ rows, const int* __restrict__ cols, const T* __restrict__ vals, long nnz, int base,
                                                         const T* __restrict__ Wt, const T* __restrict__ H, int r, T eps, T bexp, int map, T* __restrict__ out,
                                                         double* __restrict__ part, long passes) {
	typedef typename PredictChunk<T>::type chunk_t;
	constexpr int EL = 16 / (int)sizeof(T), RP = ROUNDS * 16 * EL;
	constexpr int UNROLL = ROUNDS <= 8 ? ROUNDS : 4;
	__shared__ double s_part[16][3];
	const int group = threadIdx.x >> 4, sl = threadIdx.x & 15;
	// (uniform arguments meet vector values below: split3.h)
	const T e_v = in_vgpr(eps), b_v = in_vgpr(bexp);
	double s_sq = 0, s_div = 0, s_abs = 0;
	for (long pass = blockIdx.x; pass < passes; pass += gridDim.x) {
		const long pa = pass * 32 + group, pb = pa + 16;
		const bool va = pa < nnz, vb = pb < nnz;
		const long qa = va ? pa : 0, qb = vb ? pb : 0;
		const long ia = (long)rows[qa] - base, ja = (long)cols[qa] - base, ib = (long)rows[qb] - base, jb = (long)cols[qb] - base;
		const chunk_t* wa = reinterpret_cast<const chunk_t*>(Wt + ia * RP) + sl;
		const chunk_t* ha = reinterpret_cast<const chunk_t*>(H + ja * RP) + sl;
		const chunk_t* wb = reinterpret_cast<const chunk_t*>(Wt + ib * RP) + sl;
		const chunk_t* hb = reinterpret_cast<const chunk_t*>(H + jb * RP) + sl;
		T da = 0, db = 0;
#pragma unroll UNROLL
		for (int c = 0; c < ROUNDS; ++c) {
			const chunk_t xwa = wa[16 * c], xha = ha[16 * c], xwb = wb[16 * c], xhb = hb[16 * c];
			const int k0 = (16 * c + sl) * EL;
#pragma unroll
			for (int e = 0; e < EL; ++e) {
				// a coordinate of the padding has no share, by selection
				const bool in = k0 + e < r;
				const T fa = xwa[e] * xha[e] + da, fb = xwb[e] * xhb[e] + db;
				da = in ? fa : da;
				db = in ? fb : db;
			}
		}
#pragma unroll
		for (int w = 8; w > 0; w >>= 1) { da += __shfl_xor(da, w, 16); db += __shfl_xor(db, w, 16); }
		if (out != nullptr && sl == 0) {
			if (va) out[pa] = da;
			if (vb) out[pb] = db;
		}
		if (TERMS) {
			// (an entry slot past the end takes the value 1: finite arithmetic whose result is selected out)
			const T xa = va ? vals[pa] : T(1), xb = vb ? vals[pb] : T(1);
			const T ra = xa - da, rb = xb - db;
			T ka = 0, aa = 0, kb = 0, ab = 0;
			if (map != PREDICT_NONE) {      // (uniform)
				predict_entry_terms<T>(map, xa, da + e_v, b_v, ka, aa);
				predict_entry_terms<T>(map, xb, db + e_v, b_v, kb, ab);
			}
			if (va) { s_sq += (double)(ra * ra); s_div += (double)ka; s_abs += (double)aa; }
			if (vb) { s_sq += (double)(rb * rb); s_div += (double)kb; s_abs += (double)ab; }
		}
	}
	if (TERMS) {
		// the sixteen groups in group order (a group's entries were added in entry order above)
		if (sl == 0) { s_part[group][0] = s_sq; s_part[group][1] = s_div; s_part[group][2] = s_abs; }
		__syncthreads();
		if (threadIdx.x < 3) {
			double s = 0;
			for (int g = 0; g < 16; ++g) s += s_part[g][threadIdx.x];
			part[3 * (long)blockIdx.x + threadIdx.x] = s;
		}
	}
}

// first_bad[0] = the smallest p whose coordinate lies outside [base, base + m) x [base, base + n), first_bad[1] = the smallest p whose value breaks `rule`
// (0 none, 1 finite and >= 0, 2 finite, 3 finite and > 0); both start at 0xffffffff (the caller's fill) and are lowered by integer atomics: independent of order.
// Reads rows, cols (and vals under a rule) below nnz only.
template <typename T>
__global__ __launch_bounds__(256) void k_predict_validate(const int* __restrict__ rows, const int* __restrict__ cols, const T* __restrict__ vals, long nnz, int base,
                                                          int m, int n, int rule, unsigned* __restrict__ first_bad) {
	const long stride = (long)gridDim.x * blockDim.x;
	for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += stride) {
		const long i = (long)rows[p] - base, j = (long)cols[p] - base;
		if (i < 0 || i >= m || j < 0 || j >= n) atomicMin(&first_bad[0], (unsigned)p);
		if (rule != 0) {
			const T v = vals[p];
			const bool finite = v - v == T(0);
			const bool ok = finite && (rule == 1 ? v >= T(0) : rule == 3 ? v > T(0) : true);
			if (!ok) atomicMin(&first_bad[1], (unsigned)p);
		}
	}
}

int predict_entry_parts(long nnz) { return (int)std::max(1l, std::min((nnz + PREDICT_PASS_ENTRIES - 1) / PREDICT_PASS_ENTRIES, (long)PREDICT_MAX_PARTS)); }

bool predict_rank_instantiated(int RP, size_t elem_bytes) {
	if (elem_bytes == 4) return RP == 64 || RP == 128 || RP == 256 || RP == 384 || RP == 512;
	return elem_bytes == 8 && RP >= 64 && RP <= 512 && RP % 64 == 0;
}

template <typename T>
hipError_t launch_predict_validate(const int* rows, const int* cols, const T* vals, long nnz, int base, int m, int n, int rule, unsigned* first_bad, hipStream_t stream) {
	if (rows == nullptr || cols == nullptr || first_bad == nullptr || nnz < 1 || nnz > PREDICT_MAX_ENTRIES || m < 1 || n < 1 || rule < 0 || rule > 3 ||
	    (rule != 0 && vals == nullptr))
		return hipErrorInvalidValue;
	const unsigned grid = (unsigned)std::min((nnz + 255) / 256, 2048l);
	hipLaunchKernelGGL((k_predict_validate<T>), dim3(grid), dim3(256), 0, stream, rows, cols, vals, nnz, base, m, n, rule, first_bad);
	return hipGetLastError();
}
template hipError_t launch_predict_validate<float>(const int*, const int*, const float*, long, int, int, int, int, unsigned*, hipStream_t);
template hipError_t launch_predict_validate<double>(const int*, const int*, const double*, long, int, int, int, int, unsigned*, hipStream_t);

template <typename T>
hipError_t launch_predict_entries(const int* rows, const int* cols, const T* vals, long nnz, int base, const T* Wt, const T* H, int RP, int r, T eps, double beta,
                                  T* out, double* part, hipStream_t stream) {
	const bool terms = vals != nullptr;
	if (rows == nullptr || cols == nullptr || Wt == nullptr || H == nullptr || nnz < 1 || nnz > PREDICT_MAX_ENTRIES || !predict_rank_instantiated(RP, sizeof(T)) ||
	    r < 1 || r > RP || (base != 0 && base != 1) || (!terms && out == nullptr) || (terms && part == nullptr))
		return hipErrorInvalidValue;
	const double b = (double)(T)beta;      // (in the precision of T: a value that rounds to 0 or 1 there runs the Itakura-Saito or the KL map; NaN: no divergence)
	if (terms && std::isinf(b)) return hipErrorInvalidValue;
	const int map = !terms || b != b ? PREDICT_NONE : b == 1.0 ? PREDICT_KL : b == 0.0 ? PREDICT_IS : PREDICT_GENERAL;
	const long passes = (nnz + PREDICT_PASS_ENTRIES - 1) / PREDICT_PASS_ENTRIES;
	const dim3 grid((unsigned)predict_entry_parts(nnz)), block(256);
	const T bexp = map == PREDICT_GENERAL ? (T)b : T(0);
	const int rounds = RP * (int)sizeof(T) / 256;
#define NMFAMD_PREDICT(ROUNDS)                                                                                                                              \
	if (rounds == ROUNDS) {                                                                                                                                  \
		if (terms) hipLaunchKernelGGL((k_predict_entries<T, ROUNDS, true>), grid, block, 0, stream, rows, cols, vals, nnz, base, Wt, H, r, eps, bexp, map, out, part, passes); \
		else hipLaunchKernelGGL((k_predict_entries<T, ROUNDS, false>), grid, block, 0, stream, rows, cols, vals, nnz, base, Wt, H, r, eps, bexp, map, out, part, passes);   \
	}
	// fp32: padded ranks 64, 128, 256, 384, 512 (1, 2, 4, 6, 8 rounds); fp64: 64 ... 512 in steps of 64 (2 ... 16 rounds)
	NMFAMD_PREDICT(2) NMFAMD_PREDICT(4) NMFAMD_PREDICT(6) NMFAMD_PREDICT(8)
	if constexpr (sizeof(T) == 4) { NMFAMD_PREDICT(1) }
	else { NMFAMD_PREDICT(10) NMFAMD_PREDICT(12) NMFAMD_PREDICT(14) NMFAMD_PREDICT(16) }
#undef NMFAMD_PREDICT
	return hipGetLastError();
}
template hipError_t launch_predict_entries<float>(const int*, const int*, const float*, long, int, const float*, const float*, int, int, float, double, float*, double*,
                                                  hipStream_t);
template hipError_t launch_predict_entries<double>(const int*, const int*, const double*, long, int, const double*, const double*, int, int, double, double, double*,
                                                   double*, hipStream_t);

} // namespace nmfamd
