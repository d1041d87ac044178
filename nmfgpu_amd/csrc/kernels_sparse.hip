// kernels_sparse.hip -- sparse-V compute path (extension; the reference densifies sparse input with
// cuSPARSE and runs the dense algorithm, source/common/Matrix.h:145-232).
//
// V stays in HBM as CSR (rows of V) and CSC (= CSR of V^T), 0-based int32 indices, built once on
// the host from the caller's CSR / CSC / COO arrays with the caller's index base applied exactly.
// The two products against V become row-gather SpMMs over the factor panels (whose rows are
// contiguous: panel layout [y][RP]):
//     W^T V      out(:, j) = sum_{i in column j} V(i, j) Wt(:, i)      CSC + Wt panel
//     (V H^T)^T  out(:, i) = sum_{j in row i}    V(i, j) H(:, j)       CSR + H panel
// and the KL-divergence update adds an SDDMM (W H evaluated at the stored entries only).
// One wave owns one output row ("wavefront-segmented" reduction: the 64 lanes hold the RP factor
// rows of the running sum, the stored entries of the row are walked in index order), so every
// sum has a fixed order and the result is deterministic.
//
// Every launcher of this file but launch_permute has a test entry that runs it once on caller-built arrays (nmfamd_op_kl_fused_*, _kl_update_*, _kl_sums_*,
// _panel_rowsum_*, _spmm_rows_*, _sddmm_quotient_*: amd_api.cpp); tests/test_gpu_sparse_kl_ops.py compares each launch with the restatements of
// tests/sparse_kl_reference.py, which are written from the formulas in the comments below.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "split3.h"

namespace nmfamd {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// broadcast of lane `src` (wave-uniform index) through v_readlane: no LDS crossbar round trip
__device__ inline int bcast(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ inline float bcast(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }
__device__ inline double bcast(double v, int src) {
	const long long b = __double_as_longlong(v);
	const int lo = __builtin_amdgcn_readlane((int)(b & 0xffffffffll), src), hi = __builtin_amdgcn_readlane((int)(b >> 32), src);
	return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// out(row, :) = sum_p val[p] * P(idx[p], :), p in [ptr[row], ptr[row+1]); rows >= `rows` are zeroed.
// VEC = RP / 64 factor rows per lane (contiguous: one gathered panel row is one coalesced access).
template <typename T, int VEC>
__global__ __launch_bounds__(256) void k_spmm_rows(const int* __restrict__ ptr, const int* __restrict__ idx, const T* __restrict__ val,
                                                   const T* __restrict__ P, T* __restrict__ out, int rows, int rows_pad) {
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int row = blockIdx.x * 4 + wave;
	if (row >= rows_pad) return;
	constexpr int RP = 64 * VEC;
	T acc[VEC];
#pragma unroll
	for (int v = 0; v < VEC; ++v) acc[v] = 0;
	if (row < rows) {
		const int p_begin = ptr[row], p_end = ptr[row + 1];
		for (int p0 = p_begin; p0 < p_end; p0 += 64) {
			const int cnt = min(64, p_end - p0);
			int my_idx = 0; T my_val = 0;
			if (lane < cnt) { my_idx = idx[p0 + lane]; my_val = val[p0 + lane]; }
			int u = 0;
			for (; u + 4 <= cnt; u += 4) {
				T g[4][VEC]; T v[4];
#pragma unroll
				for (int k = 0; k < 4; ++k) {
					const int i = bcast(my_idx, u + k);
					v[k] = bcast(my_val, u + k);
					const T* src = P + (long)i * RP + lane * VEC;
#pragma unroll
					for (int e = 0; e < VEC; ++e) g[k][e] = src[e];
				}
#pragma unroll
				for (int k = 0; k < 4; ++k)
#pragma unroll
					for (int e = 0; e < VEC; ++e) acc[e] += v[k] * g[k][e];
			}
			for (; u < cnt; ++u) {
				const int i = bcast(my_idx, u);
				const T v = bcast(my_val, u);
				const T* src = P + (long)i * RP + lane * VEC;
#pragma unroll
				for (int e = 0; e < VEC; ++e) acc[e] += v * src[e];
			}
		}
	}
	T* dst = out + (long)row * RP + lane * VEC;
#pragma unroll
	for (int e = 0; e < VEC; ++e) dst[e] = acc[e];
}

template <typename T>
hipError_t launch_spmm_rows(const int* ptr, const int* idx, const T* val, const T* P, int RP, T* out, int rows, int rows_pad, hipStream_t stream) {
	dim3 grid((rows_pad + 3) / 4), block(256);
	switch (RP / 64) {
	case 1: hipLaunchKernelGGL((k_spmm_rows<T, 1>), grid, block, 0, stream, ptr, idx, val, P, out, rows, rows_pad); break;
	case 2: hipLaunchKernelGGL((k_spmm_rows<T, 2>), grid, block, 0, stream, ptr, idx, val, P, out, rows, rows_pad); break;
	case 4: hipLaunchKernelGGL((k_spmm_rows<T, 4>), grid, block, 0, stream, ptr, idx, val, P, out, rows, rows_pad); break;
	default: return hipErrorInvalidValue;   // padded ranks 64, 128, 256
	}
	return hipGetLastError();
}
template hipError_t launch_spmm_rows<float>(const int*, const int*, const float*, const float*, int, float*, int, int, hipStream_t);
template hipError_t launch_spmm_rows<double>(const int*, const int*, const double*, const double*, int, double*, int, int, hipStream_t);

// SDDMM + quotient for the KL update: for every stored entry p = (row, idx[p]):
//     wh   = A(row, :) . B(idx[p], :)          (both panel rows, RP contiguous values)
//     q[p] = val[p] / (wh + eps)
// and per row the partial sums the error evaluation needs:
//     t_vwh(row) = sum_p val * wh              (terms of tr(H^T W^T V))
//     t_kl(row)  = sum_p val * log(val / wh)   (first term of the generalised KL divergence)
// One wave per row, FOUR stored entries per step: a group of 16 lanes owns one entry, each lane
// covers RP/16 contiguous factor rows of the dot product (one gathered panel row = one coalesced
// access of the group) and the dot is finished with four butterfly steps inside the group.
// Fixed summation order: lane segments, then the butterfly, then groups 0..3.
// TERMS = false: quotients only (every iteration needs those; the double-precision logarithm of the divergence term
// on one lane in sixteen was half of the kernel's time).
template <typename T, int VEC, bool TERMS>
__global__ __launch_bounds__(256) void k_sddmm_quotient(const int* __restrict__ ptr, const int* __restrict__ idx, const T* __restrict__ val,
                                                        const T* __restrict__ A, const T* __restrict__ B, T eps,
                                                        T* __restrict__ q, T* __restrict__ t_vwh, T* __restrict__ t_kl, int rows) {
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int row = blockIdx.x * 4 + wave;
	if (row >= rows) return;
	constexpr int RP = 64 * VEC, SEG = 4 * VEC;
	const int g = lane >> 4, sl = lane & 15;
	T a[SEG];
#pragma unroll
	for (int e = 0; e < SEG; ++e) a[e] = A[(long)row * RP + sl * SEG + e];
	const int p_begin = ptr[row], p_end = ptr[row + 1];
	T s_vwh = 0, s_kl = 0;
	for (int p0 = p_begin; p0 < p_end; p0 += 8) {
		// two entries per group in flight
		const int pa = p0 + g, pb = p0 + 4 + g;
		const bool va = pa < p_end, vb = pb < p_end;
		const int ja = idx[va ? pa : p_begin], jb = idx[vb ? pb : p_begin];
		const T* ba = B + (long)ja * RP + sl * SEG;
		const T* bb = B + (long)jb * RP + sl * SEG;
		T da = 0, db = 0;
#pragma unroll
		for (int e = 0; e < SEG; ++e) { da += a[e] * ba[e]; db += a[e] * bb[e]; }
#pragma unroll
		for (int w = 8; w > 0; w >>= 1) { da += __shfl_xor(da, w, 16); db += __shfl_xor(db, w, 16); }
		if (sl == 0) {
			if (va) {
				const T v = val[pa];
				q[pa] = v / (da + eps);
				if (TERMS) {
					s_vwh += v * da;
					if (v > T(0)) s_kl += v * (T)log((double)v / (double)(da + eps));
				}
			}
			if (vb) {
				const T v = val[pb];
				q[pb] = v / (db + eps);
				if (TERMS) {
					s_vwh += v * db;
					if (v > T(0)) s_kl += v * (T)log((double)v / (double)(db + eps));
				}
			}
		}
	}
	if (!TERMS) return;
	// group partials sit in lanes 0, 16, 32, 48
	const T v0 = __shfl(s_vwh, 0), v1 = __shfl(s_vwh, 16), v2 = __shfl(s_vwh, 32), v3 = __shfl(s_vwh, 48);
	const T k0 = __shfl(s_kl, 0), k1 = __shfl(s_kl, 16), k2 = __shfl(s_kl, 32), k3 = __shfl(s_kl, 48);
	if (lane == 0) { t_vwh[row] = ((v0 + v1) + v2) + v3; t_kl[row] = ((k0 + k1) + k2) + k3; }
}

// t_vwh == nullptr: no per-row error terms (quotients only)
template <typename T>
hipError_t launch_sddmm_quotient(const int* ptr, const int* idx, const T* val, const T* A, const T* B, int RP, T eps,
                                 T* q, T* t_vwh, T* t_kl, int rows, hipStream_t stream) {
	dim3 grid((rows + 3) / 4), block(256);
	const bool terms = t_vwh != nullptr && t_kl != nullptr;
#define NMFAMD_SDDMM(VEC)                                                                                                                  \
	if (terms) hipLaunchKernelGGL((k_sddmm_quotient<T, VEC, true>), grid, block, 0, stream, ptr, idx, val, A, B, eps, q, t_vwh, t_kl, rows); \
	else hipLaunchKernelGGL((k_sddmm_quotient<T, VEC, false>), grid, block, 0, stream, ptr, idx, val, A, B, eps, q, t_vwh, t_kl, rows);      \
	break
	switch (RP / 64) {
	case 1: NMFAMD_SDDMM(1);
	case 2: NMFAMD_SDDMM(2);
	case 4: NMFAMD_SDDMM(4);
	default: return hipErrorInvalidValue;
	}
#undef NMFAMD_SDDMM
	return hipGetLastError();
}
template hipError_t launch_sddmm_quotient<float>(const int*, const int*, const float*, const float*, const float*, int, float, float*, float*, float*, int, hipStream_t);
template hipError_t launch_sddmm_quotient<double>(const int*, const int*, const double*, const double*, const double*, int, double, double*, double*, double*, int, hipStream_t);

// KL half-step in ONE pass over the stored entries of a row: quotient and numerator together,
//     out(row, :) = sum_p  val[p] / (A(row, :) . B(idx[p], :) + eps)  *  B(idx[p], :)
// H step: CSC arrays, A = H (the column's own factor row), B = Wt;  W step: CSR arrays, A = Wt, B = H.
// The gathered row B(idx[p], :) serves the dot product AND the accumulation while it sits in registers, so an iteration
// gathers 2 x nnz factor rows instead of 4 x nnz, the quotients are never stored, and nothing has to be permuted
// between the CSR and the CSC order (round 1: SDDMM, permute, SpMM per half-step; 4.70 -> 2.9 ms per iteration at BASELINE
// config 3 -- the gathers were, and are, at the cache levels' row-gather rates).
// One wave per row; a group of 16 lanes owns one entry, each lane RP / 16 contiguous factor rows; two entries per group in
// flight.  Fixed order: lane segments, butterfly inside the group (dot), per-group running sums, groups 0 .. 3 at the end.
// TERMS: the per-row error terms t_vwh(row) = sum val * wh, t_kl(row) = sum val * log(val / wh) (W step of error iterations).
// BLOCKED form (blocks > 1): the gathered index range is cut into `blocks` blocks whose rows of B fit an XCD's L2 (the verdict of round 2:
// 70 % of the gathered rows missed L2 and came from the memory-side cache at its rate).  The grid runs block-major -- all rows' entries
// of block 0, then block 1, ... -- so that at any time the workgroups in flight gather from one or two blocks; a row's entries are
// sorted by index, hence its entries of block b are the range [bptr[row * (blocks + 1) + b], bptr[row * (blocks + 1) + b + 1]).
// One partial numerator panel (and one vector of error terms) per block, added in block order by the update kernel: deterministic.
__device__ inline float kl_log(float x) { return logf(x); }
__device__ inline double kl_log(double x) { return log(x); }

template <typename T, int VEC, bool TERMS>
__global__ __launch_bounds__(256) void k_kl_fused(const int* __restrict__ ptr, const int* __restrict__ idx, const T* __restrict__ val,
                                                  const T* __restrict__ A, const T* __restrict__ B, T eps,
                                                  T* __restrict__ out, T* __restrict__ t_vwh, T* __restrict__ t_kl, int rows, int rows_pad,
                                                  int blocks, long out_stride, const T* __restrict__ a_scale) {
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int per_block = (rows_pad + 3) >> 2;            // workgroups per block
	// Which (block, row group) this workgroup is.  blocks % 8 == 0 (the engine cuts long factors that way): workgroup i runs on XCD i % 8, and XCD x takes
	// the blocks x, x + 8, ... one after the other for all rows -- every L2 then holds ONE block at a time and fetches only ITS blocks (1 / 8 of the
	// gathered factor per launch instead of all of it: the factor left the memory-side cache eight times per launch in block-major order).
	// Otherwise block-major: all XCDs gather from the same block at a time.
	int blk = 0, rg = (int)blockIdx.x;
	if (blocks > 1) {
		if ((blocks & 7) == 0) {
			const int xcd = (int)(blockIdx.x & 7), j = (int)(blockIdx.x >> 3);
			blk = xcd + 8 * (j / per_block);
			rg = j % per_block;
		} else {
			blk = (int)(blockIdx.x / per_block);
			rg = (int)(blockIdx.x - (unsigned)blk * per_block);
		}
	}
	const int row = rg * 4 + wave;
	if (row >= rows_pad) return;
	out += (long)blk * out_stride;
	if (TERMS) { t_vwh += (long)blk * rows_pad; t_kl += (long)blk * rows_pad; }
	const int pstride = blocks > 1 ? blocks + 1 : 1;
	constexpr int RP = 64 * VEC, SEG = 4 * VEC;
	const int g = lane >> 4, sl = lane & 15;
	T acc[SEG];
#pragma unroll
	for (int e = 0; e < SEG; ++e) acc[e] = 0;
	T s_vwh = 0, s_kl = 0;
	if (row < rows) {
		T a[SEG];
#pragma unroll
		for (int e = 0; e < SEG; ++e) a[e] = A[(long)row * RP + sl * SEG + e];
		// a_scale (round 6): W is carried with a pending column scale d -- W = Wt D -- and every dot product W(i, :) . H(:, j) takes d once, on the row that is
		// loaded once per output row (the H step's own row of H, the W step's own row of Wt); the gathered rows stay as they lie
		if (a_scale != nullptr) {
#pragma unroll
			for (int e = 0; e < SEG; ++e) a[e] *= a_scale[sl * SEG + e];
		}
		const int p_begin = ptr[(long)row * pstride + blk], p_end = ptr[(long)row * pstride + blk + 1];
		for (int p0 = p_begin; p0 < p_end; p0 += 8) {
			const int pa = p0 + g, pb = p0 + 4 + g;
			const bool va = pa < p_end, vb = pb < p_end;
			const int ja = idx[va ? pa : p_begin], jb = idx[vb ? pb : p_begin];
			const T xa = va ? val[pa] : T(0), xb = vb ? val[pb] : T(0);
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
			// (an entry past the end has value 0: quotient 0, nothing accumulated)
			const T qa = xa / (da + eps), qb = xb / (db + eps);
#pragma unroll
			for (int e = 0; e < SEG; ++e) acc[e] += qa * ra[e];
#pragma unroll
			for (int e = 0; e < SEG; ++e) acc[e] += qb * rb[e];
			if (TERMS && sl == 0) {
				// (the logarithm in T: round 3 took it in double for float entries too -- a software routine on a quarter-rate pipe, run by four lanes of a
				//  divergent wave per pair of entries: the error-term form of this launch took 1.31 ms against 0.61; the term is rounded to T anyway)
				if (va) { s_vwh += xa * da; if (xa > T(0)) s_kl += xa * kl_log(xa / (da + eps)); }
				if (vb) { s_vwh += xb * db; if (xb > T(0)) s_kl += xb * kl_log(xb / (db + eps)); }
			}
		}
	}
	// groups 0 .. 3 in order: (g0 + g1) + (g2 + g3) on every lane, then lanes 0 .. 15 hold the row
#pragma unroll
	for (int e = 0; e < SEG; ++e) {
		const T o = __shfl_xor(acc[e], 16);
		const T lo = (g & 1) ? o + acc[e] : acc[e] + o;          // pair sum, lower group first
		const T p2 = __shfl_xor(lo, 32);
		acc[e] = (g & 2) ? p2 + lo : lo + p2;
	}
	if (g == 0) {
		T* dst = out + (long)row * RP + sl * SEG;
#pragma unroll
		for (int e = 0; e < SEG; ++e) dst[e] = acc[e];
	}
	if (TERMS && row < rows) {
		const T v0 = __shfl(s_vwh, 0), v1 = __shfl(s_vwh, 16), v2 = __shfl(s_vwh, 32), v3 = __shfl(s_vwh, 48);
		const T k0 = __shfl(s_kl, 0), k1 = __shfl(s_kl, 16), k2 = __shfl(s_kl, 32), k3 = __shfl(s_kl, 48);
		if (lane == 0) { t_vwh[row] = ((v0 + v1) + v2) + v3; t_kl[row] = ((k0 + k1) + k2) + k3; }
	}
}

// out: rows_pad x RP numerator panel (rows in [rows, rows_pad) zeroed); t_vwh == nullptr: no per-row error terms
template <typename T>
hipError_t launch_kl_fused(const int* ptr, const int* idx, const T* val, const T* A, const T* B, int RP, T eps,
                           T* out, T* t_vwh, T* t_kl, int rows, int rows_pad, hipStream_t stream, int blocks, long out_stride, const T* a_scale) {
	if (blocks < 1) return hipErrorInvalidValue;
	dim3 grid((unsigned)(((rows_pad + 3) / 4) * blocks)), block(256);
	const bool terms = t_vwh != nullptr && t_kl != nullptr;
#define NMFAMD_KLF(VEC)                                                                                                                        \
	if (terms) hipLaunchKernelGGL((k_kl_fused<T, VEC, true>), grid, block, 0, stream, ptr, idx, val, A, B, eps, out, t_vwh, t_kl, rows, rows_pad, blocks, out_stride, a_scale); \
	else hipLaunchKernelGGL((k_kl_fused<T, VEC, false>), grid, block, 0, stream, ptr, idx, val, A, B, eps, out, t_vwh, t_kl, rows, rows_pad, blocks, out_stride, a_scale);      \
	break
	switch (RP / 64) {
	case 1: NMFAMD_KLF(1);
	case 2: NMFAMD_KLF(2);
	case 4: NMFAMD_KLF(4);
	default: return hipErrorInvalidValue;
	}
#undef NMFAMD_KLF
	return hipGetLastError();
}
template hipError_t launch_kl_fused<float>(const int*, const int*, const float*, const float*, const float*, int, float, float*, float*, float*, int, int, hipStream_t, int, long, const float*);
template hipError_t launch_kl_fused<double>(const int*, const int*, const double*, const double*, const double*, int, double, double*, double*, double*, int, int, hipStream_t, int, long, const double*);

// dst[p] = src[perm[p]]: the quotients in the other storage order
template <typename T>
__global__ void k_permute(const T* __restrict__ src, const int* __restrict__ perm, T* __restrict__ dst, long count) {
	const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
	if (p < count) dst[p] = src[perm[p]];
}

template <typename T>
hipError_t launch_permute(const T* src, const int* perm, T* dst, long count, hipStream_t stream) {
	if (count == 0) return hipSuccess;
	hipLaunchKernelGGL((k_permute<T>), dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, src, perm, dst, count);
	return hipGetLastError();
}
template hipError_t launch_permute<float>(const float*, const int*, float*, long, hipStream_t);
template hipError_t launch_permute<double>(const double*, const int*, double*, long, hipStream_t);

// partial(wg, c) = sum of P(c, y) over the workgroup's 128 panel columns (row sums of the factor
// matrix: the KL denominators); reduced in order by launch_reduce_partials.
template <typename T>
__global__ __launch_bounds__(256) void k_panel_rowsum_partial(const T* __restrict__ P, int RP, T* __restrict__ partial) {
	const long base = (long)blockIdx.x * 128 * RP;
	for (int c = threadIdx.x; c < RP; c += 256) {
		T s = 0;
		for (int y = 0; y < 128; ++y) s += P[base + (long)y * RP + c];
		partial[(long)blockIdx.x * RP + c] = s;
	}
}

template <typename T>
hipError_t launch_panel_rowsum(const T* P, int RP, int len_pad, T* partial, T* sums, hipStream_t stream) {
	const int parts = len_pad / 128;
	hipLaunchKernelGGL((k_panel_rowsum_partial<T>), dim3(parts), dim3(256), 0, stream, P, RP, partial);
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) return e;
	return launch_reduce_partials<T>(partial, parts, RP, sums, RP, stream);
}
template hipError_t launch_panel_rowsum<float>(const float*, int, int, float*, float*, hipStream_t);
template hipError_t launch_panel_rowsum<double>(const double*, int, int, double*, double*, hipStream_t);

// KL multiplicative update: P(c, y) <- P(c, y) * num(c, y) / (den(c) + eps), plus the per-workgroup
// sums of squares of the result (for the column normalisation of W).  One workgroup = 128 panel columns.
// One workgroup = 128 panel columns; a thread owns four consecutive factor rows c (one 16-byte access) and every (1024 / RP)-th
// panel column; the `parts` partial numerators (the blocks of the blocked KL step) are added in block order, eight loads in flight.
template <typename T>
__global__ __launch_bounds__(256) void k_kl_update(T* __restrict__ P, const T* __restrict__ num, const T* __restrict__ den, int RP, T eps,
                                                   T* __restrict__ sumsq_part, int parts, long part_stride, T* __restrict__ sum_part, const T* __restrict__ scale) {
	typedef T T4 __attribute__((ext_vector_type(4)));
	__shared__ T s_ss[256 * 4], s_sv[256 * 4];
	const long base = (long)blockIdx.x * 128 * RP;
	const int per_row = RP / 4, c4 = threadIdx.x % per_row, yy = threadIdx.x / per_row, ystep = 256 / per_row;
	T4 d = *reinterpret_cast<const T4*>(den + 4 * c4);
	d += in_vgpr(eps);      // (a scalar operand of a packed add otherwise: split3.h)
	// scale (round 6, W's pending column scale d): the H update's numerator is D (Wt^T Q), the W update's old value is Wt D -- either way one more factor per element
	T4 sc = {1, 1, 1, 1};
	if (scale != nullptr) sc = *reinterpret_cast<const T4*>(scale + 4 * c4);
	T4 ss = {0, 0, 0, 0}, sv = {0, 0, 0, 0};
	for (int y = yy; y < 128; y += ystep) {
		const long e = base + (long)y * RP + 4 * c4;
		T4 nm = *reinterpret_cast<const T4*>(num + e);
		// batches of eight requested together; the remainder as ONE batch of its own size (round 3's tail loop took the last parts % 8 panels one dependent
		// load at a time -- seven of config 3's sixteen H-side panels; clamped duplicates instead re-read whole panels: 56 -> 71 us)
		int b = 1;
		for (; b + 8 <= parts; b += 8) {
			T4 t[8];
#pragma unroll
			for (int u = 0; u < 8; ++u) t[u] = *reinterpret_cast<const T4*>(num + (long)(b + u) * part_stride + e);
#pragma unroll
			for (int u = 0; u < 8; ++u) nm += t[u];
		}
#define NMFAMD_KL_TAIL(N) case N: { T4 t[N]; _Pragma("unroll") for (int u = 0; u < N; ++u) t[u] = *reinterpret_cast<const T4*>(num + (long)(b + u) * part_stride + e); \
                                   _Pragma("unroll") for (int u = 0; u < N; ++u) nm += t[u]; break; }
		switch (parts - b) {
			NMFAMD_KL_TAIL(1) NMFAMD_KL_TAIL(2) NMFAMD_KL_TAIL(3) NMFAMD_KL_TAIL(4) NMFAMD_KL_TAIL(5) NMFAMD_KL_TAIL(6) NMFAMD_KL_TAIL(7)
			default: break;
		}
#undef NMFAMD_KL_TAIL
		const T4 p = *reinterpret_cast<const T4*>(P + e);
		const T4 v = (p * sc) * nm / d;
		*reinterpret_cast<T4*>(P + e) = v;
		ss += v * v;
		sv += v;
	}
	if (sumsq_part || sum_part) {
		// the panel columns of one factor row in ascending order of the thread's start column (fixed order); sums of squares (the column normalisation of W)
		// and plain sums (the row sums of the factor matrix: the other half-step's denominators -- round 3 read the panel again for them) in one exchange
#pragma unroll
		for (int i = 0; i < 4; ++i) { s_ss[threadIdx.x * 4 + i] = ss[i]; s_sv[threadIdx.x * 4 + i] = sv[i]; }
		__syncthreads();
		if ((int)threadIdx.x < RP) {
			const int c = threadIdx.x;
			T acc = 0, acv = 0;
			for (int g = 0; g < ystep; ++g) { acc += s_ss[(g * per_row + c / 4) * 4 + (c & 3)]; acv += s_sv[(g * per_row + c / 4) * 4 + (c & 3)]; }
			if (sumsq_part) sumsq_part[(long)blockIdx.x * RP + c] = acc;
			if (sum_part) sum_part[(long)blockIdx.x * RP + c] = acv;
		}
	}
}

// sums(c) = (sum over parts of sum_part(., c)) * (1 / sqrt(sum over parts of sumsq_part(., c)), or 1 where that is 0: kernel::normalizeColumns' guard) -- the
// column sums of the panel AFTER its column normalisation, from the two vectors of per-workgroup partials its update left (sumsq_part == nullptr: plain sums).
// One workgroup of 1024 threads per 16 columns (16 columns x 64 groups of parts, eight loads in flight, groups added in order): a single workgroup pulled the
// 800 KB of config 3's W-side partials through one CU in 8.4 us.
template <typename T>
__global__ __launch_bounds__(1024) void k_kl_sums(const T* __restrict__ sum_part, const T* __restrict__ sumsq_part, int parts, int RP, T* __restrict__ sums, T* __restrict__ scale_out) {
	__shared__ T s_a[1024], s_b[1024];
	const int cl = threadIdx.x & 15, g = threadIdx.x >> 4, c = blockIdx.x * 16 + cl;
	T a = 0, b = 0;
	for (int p = g; p < parts; p += 8 * 64) {
		T va[8], vb[8];
#pragma unroll
		for (int u = 0; u < 8; ++u) {
			const int q = p + u * 64;
			va[u] = q < parts ? sum_part[(long)q * RP + c] : T(0);
			vb[u] = (sumsq_part != nullptr && q < parts) ? sumsq_part[(long)q * RP + c] : T(0);
		}
#pragma unroll
		for (int u = 0; u < 8; ++u) { a += va[u]; b += vb[u]; }
	}
	s_a[threadIdx.x] = a; s_b[threadIdx.x] = b;
	__syncthreads();
	if (threadIdx.x < 16) {
		T sa = 0, sb = 0;
		for (int k = 0; k < 64; ++k) { sa += s_a[k * 16 + cl]; sb += s_b[k * 16 + cl]; }
		sums[c] = sumsq_part == nullptr ? sa : (sb > T(0) ? sa / (T)sqrt((double)sb) : sa);
		// the pending column scale itself (kernel::normalizeColumns as a factor, KernelNormalizeColumns.cu:37-58): 1 / sqrt(sum of squares), 1 for an all-zero column
		if (scale_out != nullptr) scale_out[c] = sb > T(0) ? (T)(1.0 / sqrt((double)sb)) : T(1);
	}
}

template <typename T>
hipError_t launch_kl_sums(const T* sum_part, const T* sumsq_part, int parts, int RP, T* sums, hipStream_t stream, T* scale_out) {
	if (RP < 64 || RP > 256 || RP % 16 != 0) return hipErrorInvalidValue;
	hipLaunchKernelGGL((k_kl_sums<T>), dim3(RP / 16), dim3(1024), 0, stream, sum_part, sumsq_part, parts, RP, sums, scale_out);
	return hipGetLastError();
}
template hipError_t launch_kl_sums<float>(const float*, const float*, int, int, float*, hipStream_t, float*);
template hipError_t launch_kl_sums<double>(const double*, const double*, int, int, double*, hipStream_t, double*);

template <typename T>
hipError_t launch_kl_update(T* P, const T* num, const T* den, int RP, int len_pad, T eps, T* sumsq_part, hipStream_t stream, int parts, long part_stride, T* sum_part, const T* scale) {
	// padded ranks 64, 128, 256, as in the gather launchers: k_kl_update's thread mapping needs RP / 4 to divide 256 (at 192 the last of its six thread groups
	// would repeat the rows of the first, and the exchange would read five groups of six)
	if ((RP != 64 && RP != 128 && RP != 256) || parts < 1) return hipErrorInvalidValue;
	hipLaunchKernelGGL((k_kl_update<T>), dim3(len_pad / 128), dim3(256), 0, stream, P, num, den, RP, eps, sumsq_part, parts, part_stride, sum_part, scale);
	return hipGetLastError();
}
template hipError_t launch_kl_update<float>(float*, const float*, const float*, int, int, float, float*, hipStream_t, int, long, float*, const float*);
template hipError_t launch_kl_update<double>(double*, const double*, const double*, int, int, double, double*, hipStream_t, int, long, double*, const double*);

} // namespace nmfamd
