// kernels_masked.hip -- missing-value NMF: the multiplicative update over the OBSERVED entries of V only (docs/MISSING.md).
//
// Omega = the stored entries of the sparse images (kernels_sparse.hip's CSR + CSC, built once per upload).  W H inside the two denominators of the
// reference's multiplicative update is restricted to Omega, so each half-step needs, per output row, one SDDMM value per stored entry and two
// accumulations with the gathered factor row:
//     H step (CSC image, A = H,  B = Wt):  a_j <- a_j .* (sum_p v_p B(i_p, :)) ./ (sum_p (a_j . B(i_p, :)) B(i_p, :) + eps)
//     W step (CSR image, A = Wt, B = H):   a_i <- a_i .* (sum_p v_p B(j_p, :)) ./ (sum_p (a_i . B(j_p, :)) B(j_p, :) + eps)
// Layout of k_kl_fused: one wave per output row, a group of 16 lanes owns one stored entry (two per group in flight), each lane SEG = RP / 16 contiguous
// factor rows; the gathered row B(idx[p], :) serves the dot product and both accumulations while it sits in registers, so a half-step gathers nnz factor rows.
// The owning wave writes its row of A in place: no other wave of the launch reads that row (the gathered panel is the other factor), so no numerator or
// denominator panel exists.  Fixed order everywhere: lane segments, butterfly inside the group, per-group running sums in entry order, groups
// (g0 + g1) + (g2 + g3); no atomics -- a repeated run is bit-identical.
// An empty row (no stored entry) has num = den = 0 and becomes 0; padding factor rows (c >= r) are 0 in A and in B and stay 0; padding rows are not touched.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "split3.h"

namespace nmfamd {

// UPDATE: write the updated rows of A (false: the residual-only form of the error under constant W).  TERMS: t_res(row) = sum_p (v_p - A(row, :) . B(idx[p], :))^2
// with the OLD row of A.  sumsq_part != nullptr (UPDATE only): per-workgroup partial sums of squares of the new rows, one RP vector per workgroup -- the workgroups
// then stride over the row groups (workgroup w takes row groups w, w + gridDim, ...), so the count of partials is the grid, a function of the row count only.
template <typename T, int VEC, bool UPDATE, bool TERMS>
__global__ __launch_bounds__(256) void k_masked_fused(const int* __restrict__ ptr, const int* __restrict__ idx, const T* __restrict__ val,
                                                      T* __restrict__ A, const T* __restrict__ B, T eps,
                                                      T* __restrict__ t_res, T* __restrict__ sumsq_part, int rows, int row_groups) {
	constexpr int RP = 64 * VEC, SEG = 4 * VEC;
	__shared__ T s_sq[4][RP];
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int g = lane >> 4, sl = lane & 15;
	const T e_v = in_vgpr(eps);        // (a uniform argument meets vector values below: split3.h)
	T sq[SEG];
#pragma unroll
	for (int e = 0; e < SEG; ++e) sq[e] = 0;
	for (int rg = blockIdx.x; rg < row_groups; rg += gridDim.x) {
		const int row = rg * 4 + wave;
		if (row >= rows) continue;     // (wave-uniform)
		T a[SEG], num[SEG], den[SEG];
#pragma unroll
		for (int e = 0; e < SEG; ++e) { a[e] = A[(long)row * RP + sl * SEG + e]; num[e] = 0; den[e] = 0; }
		T s_res = 0;
		const int p_begin = ptr[row], p_end = ptr[row + 1];
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
			// an entry past the end: value 0 and no share of the denominator
			if (!va) da = 0;
			if (!vb) db = 0;
			if (UPDATE) {
#pragma unroll
				for (int e = 0; e < SEG; ++e) { num[e] += xa * ra[e]; den[e] += da * ra[e]; }
#pragma unroll
				for (int e = 0; e < SEG; ++e) { num[e] += xb * rb[e]; den[e] += db * rb[e]; }
			}
			if (TERMS && sl == 0) {
				if (va) { const T d = xa - da; s_res += d * d; }
				if (vb) { const T d = xb - db; s_res += d * d; }
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
					const T v = a[e] * num[e] / (den[e] + e_v);      // the reference's value * upper / (lower + eps)
					dst[e] = v;
					sq[e] += v * v;
				}
			}
		}
		if (TERMS) {
			const T v0 = __shfl(s_res, 0), v1 = __shfl(s_res, 16), v2 = __shfl(s_res, 32), v3 = __shfl(s_res, 48);
			if (lane == 0) t_res[row] = ((v0 + v1) + v2) + v3;
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

int masked_norm_parts(int rows) { return std::max(1, std::min((rows + 3) / 4, MASKED_NORM_PARTS)); }

template <typename T>
hipError_t launch_masked_half_step(const int* ptr, const int* idx, const T* val, T* A, const T* B, int RP, T eps, bool update,
                                   T* t_res, T* sumsq_part, int rows, hipStream_t stream) {
	if (rows <= 0 || (!update && t_res == nullptr) || (!update && sumsq_part != nullptr)) return hipErrorInvalidValue;
	const int row_groups = (rows + 3) / 4;
	const dim3 grid((unsigned)(sumsq_part != nullptr ? masked_norm_parts(rows) : row_groups)), block(256);
	const bool terms = t_res != nullptr;
#define NMFAMD_MASKED(VEC)                                                                                                                                  \
	if (update && terms) hipLaunchKernelGGL((k_masked_fused<T, VEC, true, true>), grid, block, 0, stream, ptr, idx, val, A, B, eps, t_res, sumsq_part, rows, row_groups);        \
	else if (update) hipLaunchKernelGGL((k_masked_fused<T, VEC, true, false>), grid, block, 0, stream, ptr, idx, val, A, B, eps, t_res, sumsq_part, rows, row_groups);         \
	else hipLaunchKernelGGL((k_masked_fused<T, VEC, false, true>), grid, block, 0, stream, ptr, idx, val, A, B, eps, t_res, sumsq_part, rows, row_groups);                      \
	break
	switch (RP / 64) {
	case 1: NMFAMD_MASKED(1);
	case 2: NMFAMD_MASKED(2);
	case 4: NMFAMD_MASKED(4);
	default: return hipErrorInvalidValue;      // padded ranks 64, 128, 256
	}
#undef NMFAMD_MASKED
	return hipGetLastError();
}
template hipError_t launch_masked_half_step<float>(const int*, const int*, const float*, float*, const float*, int, float, bool, float*, float*, int, hipStream_t);
template hipError_t launch_masked_half_step<double>(const int*, const int*, const double*, double*, const double*, int, double, bool, double*, double*, int, hipStream_t);

} // namespace nmfamd
