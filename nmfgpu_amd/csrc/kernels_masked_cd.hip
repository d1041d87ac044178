// kernels_masked_cd.hip -- missing-value NMF by coordinate descent over the OBSERVED entries of V (docs/MISSING.md, "Coordinate descent").
//
// A half-step solves, for every row i of the panel A (the CSR image with A = Wt, B = H, or the CSC image with A = H, B = Wt), the row's own normal equations
//     G_i = sum_p b_p b_p^T   (RP x RP),   c_i = sum_p v_p b_p,       p over the row's stored entries in STORED order, b_p = B(idx[p], :) with coordinates >= r selected to 0
// with `sweeps` Gauss-Seidel sweeps of docs/HALS.md started at the old row: for k = 0 .. r - 1, d_k = G_i[k][k] + l2 (the step is skipped where d_k <= 0),
//     a[k] <- max(0, a[k] - (G_i[k, :] . a + l2 a[k] - c_i[k] + l1) / d_k).
// One workgroup of four waves per row at a time (the workgroups stride over the rows; a long row stays on its workgroup):
//   * the row's gathered B rows stream through LDS in tiles of TK entries, gathered in whole 128-byte lines (consecutive lanes take consecutive 16 bytes of a row);
//   * G_i is formed on the matrix pipe -- v_mfma_f32_32x32x2_f32 / v_mfma_f64_16x16x4_f64, an exact fma chain over the entries in stored order (a tile's unused
//     tail holds zeros, which add nothing) -- only the blocks on or above the diagonal, dealt to the waves round robin; the accumulators hold G_i while the row streams;
//   * c_i beside it, one coordinate per thread of the waves with the fewest blocks, entries in stored order;
//   * G_i then goes to LDS OVER the dead staging tile (the mirror of an off-diagonal block is exact: b_k b_l and b_l b_k round alike), and wave 0 sweeps: the
//     gradient g = G a - c lives across its lanes (coordinate l + 64 e on lane l, in double) and step k adds delta_k G[k][:] to it -- row k = column k of G,
//     contiguous in LDS --, so a coordinate costs one LDS row and two lane reads, no reduction.
// No atomics, nothing outside a row's own workgroup: a row's bits depend on that row alone.  An empty row becomes exactly 0; coordinates >= r come out exactly 0
// whatever the padding of A and B holds.  NORMAL: the launch also writes G_i and c_i (the kernel-level entry's view of the normal equations).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>

#include "kernels.h"
#include "split3.h"

namespace nmfamd {

namespace {

// the matrix-pipe form of a precision: block edge BS, entries per instruction KS, accumulator registers NACC, and where accumulator register e of a lane sits
template <typename T> struct CdPipe;
template <> struct CdPipe<float> {
	static constexpr int BS = 32, KS = 2, NACC = 16;
	typedef float acc_t __attribute__((ext_vector_type(16)));
	typedef float4 line_t;
	__device__ static inline acc_t mfma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
	__device__ static inline int row(int e, int lane) { return (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5); }
};
template <> struct CdPipe<double> {
	static constexpr int BS = 16, KS = 4, NACC = 4;
	typedef double acc_t __attribute__((ext_vector_type(4)));
	typedef double2 line_t;
	__device__ static inline acc_t mfma(double a, double b, acc_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
	__device__ static inline int row(int e, int lane) { return (lane >> 4) + 4 * e; }
};

constexpr int CD_TK = 32;      // entries per staging tile

template <typename T, int RP> struct CdGeom {
	static constexpr int LD = RP + (sizeof(T) == 8 ? 2 : 0);      // row stride of the staging tile (fp64: 16 bytes of padding, the four k rows of an operand read then miss each other's banks)
	static constexpr int AREA = RP * RP > CD_TK * LD ? RP * RP : CD_TK * LD;      // G over the tile
	static constexpr int LDS_BYTES = (int)sizeof(T) * (AREA + 2 * RP + CD_TK);
};

template <typename T, int RP, bool NORMAL>
__global__ __launch_bounds__(256) void k_masked_cd(const int* __restrict__ ptr, const int* __restrict__ idx, const T* __restrict__ val, T* __restrict__ A,
                                                   const T* __restrict__ B, int r, int rows, int sweeps, T l1_arg, T l2_arg, T* __restrict__ G_out, T* __restrict__ c_out) {
	using P = CdPipe<T>;
	using Geo = CdGeom<T, RP>;
	using line_t = typename P::line_t;
	using acc_t = typename P::acc_t;
	constexpr int BS = P::BS, KS = P::KS, NACC = P::NACC, NB = RP / BS, NU = NB * (NB + 1) / 2, MAXB = (NU + 3) / 4;
	constexpr int TK = CD_TK, LD = Geo::LD, V16 = 16 / (int)sizeof(T), CH = RP / V16, VEC = RP / 64;
	extern __shared__ __attribute__((aligned(16))) unsigned char cd_smem[];
	T* const s_g = reinterpret_cast<T*>(cd_smem);      // [RP][RP] once the row has streamed; the staging tile [TK][LD] until then
	T* const s_c = s_g + Geo::AREA;                    // [RP]
	T* const s_p = s_c + RP;                           // [RP] the old row, coordinates >= r as 0
	T* const s_val = s_p + RP;                         // [TK]
	const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
	const int oi = lane & (BS - 1), ok = lane / BS;    // operand element of this lane: coordinate oi of its block, entry ok of the k-step
	const int cj = tid - (256 - RP);                   // c_i: coordinate of this thread (the last RP threads: the waves with the fewest blocks)
	const T l1 = in_vgpr(l1_arg), l2 = in_vgpr(l2_arg);
	// the blocks of this wave: upper-triangle block u = wave + 4 s in row-major order
	int bi[MAXB], bj[MAXB];
#pragma unroll
	for (int s = 0; s < MAXB; ++s) {
		int i = 0, rem = wave + 4 * s;
		while (i < NB - 1 && rem >= NB - i) { rem -= NB - i; ++i; }
		bi[s] = i;
		bj[s] = i + rem;      // (>= NB where the wave has no block s)
	}
	for (int row = blockIdx.x; row < rows; row += gridDim.x) {
		const int p_begin = ptr[row], p_end = ptr[row + 1];
		if (p_begin >= p_end) {      // (workgroup-uniform) no stored entry: the row becomes 0, its normal equations are 0
			if (tid < RP) A[(long)row * RP + tid] = 0;
			if (NORMAL) {
				for (int x = tid; x < RP * RP; x += 256) G_out[(long)row * RP * RP + x] = 0;
				if (tid < RP) c_out[(long)row * RP + tid] = 0;
			}
			continue;
		}
		acc_t acc[MAXB];
#pragma unroll
		for (int s = 0; s < MAXB; ++s)
#pragma unroll
			for (int e = 0; e < NACC; ++e) acc[s][e] = 0;
		T c_acc = 0;
		for (int p0 = p_begin; p0 < p_end; p0 += TK) {
			__syncthreads();      // the tile's readers, or the sweep of the row before, are done
			for (int x = tid; x < TK * CH; x += 256) {
				const int e = x / CH, q = x % CH;
				const bool has = p0 + e < p_end;
				const int j = idx[has ? p0 + e : p_begin];
				line_t v = *reinterpret_cast<const line_t*>(B + (long)j * RP + q * V16);
				T* comp = reinterpret_cast<T*>(&v);
#pragma unroll
				for (int y = 0; y < V16; ++y)
					if (!has || q * V16 + y >= r) comp[y] = 0;      // selected, not multiplied: the padding may hold anything
				*reinterpret_cast<line_t*>(s_g + e * LD + q * V16) = v;
			}
			if (tid < TK) s_val[tid] = p0 + tid < p_end ? val[p0 + tid] : T(0);
			__syncthreads();
			const int cnt = min(TK, p_end - p0), ksteps = (cnt + KS - 1) / KS;
#pragma unroll
			for (int s = 0; s < MAXB; ++s) {
				if (bj[s] < NB) {      // (wave-uniform)
					const T* pa = s_g + ok * LD + bi[s] * BS + oi;
					const T* pb = s_g + ok * LD + bj[s] * BS + oi;
					for (int kk = 0; kk < ksteps; ++kk) acc[s] = P::mfma(pa[kk * KS * LD], pb[kk * KS * LD], acc[s]);
				}
			}
			if (cj >= 0)
				for (int e = 0; e < cnt; ++e) c_acc += s_val[e] * s_g[e * LD + cj];
		}
		__syncthreads();      // the last tile is dead: G over it
#pragma unroll
		for (int s = 0; s < MAXB; ++s) {
			if (bj[s] < NB) {
				const int cc = bj[s] * BS + oi;
#pragma unroll
				for (int e = 0; e < NACC; ++e) {
					const int rr = bi[s] * BS + P::row(e, lane);
					s_g[rr * RP + cc] = acc[s][e];
					if (bi[s] != bj[s]) s_g[cc * RP + rr] = acc[s][e];
				}
			}
		}
		if (cj >= 0) s_c[cj] = c_acc;
		if (tid < RP) s_p[tid] = tid < r ? A[(long)row * RP + tid] : T(0);
		__syncthreads();
		if (NORMAL) {
			for (int x = tid; x < RP * RP; x += 256) G_out[(long)row * RP * RP + x] = s_g[x];
			if (tid < RP) c_out[(long)row * RP + tid] = s_c[tid];
		}
		if (wave == 0) {
			// (g in double in either precision: it is carried through every step of every sweep and never formed afresh, so what it loses it loses for good -- in
			//  fp32 a row with fewer entries than coordinates, whose G_i is singular, ended 10 ... 100 times further from the fp64 result than a sweep that forms
			//  each dot product afresh; the step itself, quotient included, stays in T)
			T pv[VEC];
			double g[VEC];
#pragma unroll
			for (int e = 0; e < VEC; ++e) { pv[e] = s_p[lane + 64 * e]; g[e] = 0; }
			for (int k = 0; k < r; ++k) {
				const double pk = (double)s_p[k];
#pragma unroll
				for (int e = 0; e < VEC; ++e) g[e] += (double)s_g[k * RP + lane + 64 * e] * pk;
			}
#pragma unroll
			for (int e = 0; e < VEC; ++e) g[e] -= (double)s_c[lane + 64 * e];
			for (int sw = 0; sw < sweeps; ++sw) {
				for (int k = 0; k < r; ++k) {
					const int ek = k >> 6, lk = k & 63;
					T pk = pv[0];
					double gk = g[0];
#pragma unroll
					for (int e = 1; e < VEC; ++e)
						if (e == ek) { pk = pv[e]; gk = g[e]; }
					pk = __shfl(pk, lk);
					gk = __shfl(gk, lk);
					const T d = s_g[k * RP + k] + l2;
					if (d > 0) {      // (wave-uniform; a coordinate no entry of the row touches keeps its value at l2 = 0)
						const T num = (T)(gk + (double)l2 * (double)pk + (double)l1);
						const T nw = max(T(0), pk - num / d);
						const double dl = (double)nw - (double)pk;
#pragma unroll
						for (int e = 0; e < VEC; ++e) {
							g[e] += dl * (double)s_g[k * RP + lane + 64 * e];
							if (e == ek && lane == lk) pv[e] = nw;
						}
					}
				}
			}
#pragma unroll
			for (int e = 0; e < VEC; ++e) A[(long)row * RP + lane + 64 * e] = lane + 64 * e < r ? pv[e] : T(0);
		}
	}
}

template <typename T, int RP, bool NORMAL>
hipError_t launch_cd(const int* ptr, const int* idx, const T* val, T* A, const T* B, int r, int rows, int sweeps, T l1, T l2, T* G_out, T* c_out, hipStream_t stream) {
	static std::atomic<unsigned long long> lds_done{0};
	constexpr int bytes = CdGeom<T, RP>::LDS_BYTES;
	if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void*>(&k_masked_cd<T, RP, NORMAL>), bytes, lds_done); e != hipSuccess) return e;
	const dim3 grid((unsigned)std::min(rows, MASKED_CD_MAX_GRID)), block(256);
	hipLaunchKernelGGL((k_masked_cd<T, RP, NORMAL>), grid, block, bytes, stream, ptr, idx, val, A, B, r, rows, sweeps, l1, l2, G_out, c_out);
	return hipGetLastError();
}

} // namespace

template <typename T>
hipError_t launch_masked_cd_half_step(const int* ptr, const int* idx, const T* val, T* A, const T* B, int RP, int r, int rows, int sweeps, T l1, T l2, T* G_out, T* c_out,
                                      hipStream_t stream) {
	if (!masked_cd_rank_instantiated(RP) || r < 1 || r > RP || rows <= 0 || sweeps < 1 || sweeps > MASKED_CD_MAX_SWEEPS || !(l1 >= 0) || !(l2 >= 0) || !std::isfinite((double)l1) ||
	    !std::isfinite((double)l2) || (G_out == nullptr) != (c_out == nullptr))
		return hipErrorInvalidValue;
	const bool normal = G_out != nullptr;
	if (RP == 64) return normal ? launch_cd<T, 64, true>(ptr, idx, val, A, B, r, rows, sweeps, l1, l2, G_out, c_out, stream)
	                            : launch_cd<T, 64, false>(ptr, idx, val, A, B, r, rows, sweeps, l1, l2, G_out, c_out, stream);
	return normal ? launch_cd<T, 128, true>(ptr, idx, val, A, B, r, rows, sweeps, l1, l2, G_out, c_out, stream)
	              : launch_cd<T, 128, false>(ptr, idx, val, A, B, r, rows, sweeps, l1, l2, G_out, c_out, stream);
}
template hipError_t launch_masked_cd_half_step<float>(const int*, const int*, const float*, float*, const float*, int, int, int, int, float, float, float*, float*, hipStream_t);
template hipError_t launch_masked_cd_half_step<double>(const int*, const int*, const double*, double*, const double*, int, int, int, int, double, double, double*, double*, hipStream_t);

} // namespace nmfamd
