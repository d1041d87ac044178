// kernels_beta_online.hip -- the update launch of the minibatch (online) dense beta-divergence update (docs/DIVERGENCE.md, "Minibatch update").
//
// The fused half-step launches of kernels_beta.hip serve a block of columns as they are (offset pointers, a padded output length, valid counts).  Their companion
// k_beta_update does not: it runs one workgroup per 128 panel rows -- 79 workgroups for W at m = 10 000 -- and a minibatch pass runs an update launch twice per
// batch, not twice per pass.  k_beta_update_rows does the same work on a fine grid: a workgroup owns BETA_ROWS_PER_WG = 16 panel rows, thread (g, c) column c of
// every (256 / RP)-th of them.  It adds the slabs' partial panels in slab order and then
//     ONLINE = false:  P(o, c) <- P(o, c) (num / den)^gamma                                                  the ordinary update (the batch's H step)
//     ONLINE = true:   A <- rho A + P^(1 / gamma) num,  B <- rho B + den,  P <- (A / B)^gamma                the online update (the W step; A, B: the accumulators)
// with den = (den_part's sum, or dsum(c) at the unweighted beta = 1) + eps + l1 + l2 P(o, c), sets values below eps to 0 when asked to, zeroes the padding
// (o >= out_valid or c >= r; A and B are not touched there) and leaves the column sums of its 16 rows (sum_part: [out_pad / 16][RP]) for launch_kl_sums, which adds
// any number of parts in a fixed order.  No atomics anywhere: a repeated run is bit-identical.
// power: 0 gamma = 1, 1 gamma = 1/2 (a square root; P^(1 / gamma) is a square), 2 any other gamma (exp2(gamma log2 x), exp2(log2(x) / gamma); 0 stays 0).
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernels.h"
#include "split3.h"

namespace nmfamd {

template <typename T, bool ONLINE>
__global__ __launch_bounds__(256) void k_beta_update_rows(T* __restrict__ P, T* __restrict__ Aacc, T* __restrict__ Bacc, const T* __restrict__ num_part,
                                                          const T* __restrict__ den_part, long part_stride, int slabs, const T* __restrict__ dsum, int RP, int r,
                                                          int out_valid, T eps, int vec_den, int power, T gamma, T inv_gamma, T l1, T l2, T rho, int flush,
                                                          T* __restrict__ sum_part) {
	__shared__ T s_sm[256];
	const int G = 256 / RP, c = threadIdx.x % RP, g = threadIdx.x / RP;
	const int row0 = blockIdx.x * BETA_ROWS_PER_WG;
	// (uniform arguments that meet vector values: split3.h)
	const T e_v = in_vgpr(eps), g_v = in_vgpr(gamma), ig_v = in_vgpr(inv_gamma), l1_v = in_vgpr(l1), l2_v = in_vgpr(l2), rho_v = in_vgpr(rho);
	const T dvec = vec_den ? dsum[c] : T(0);
	T sm = 0;
	for (int row = row0 + g; row < row0 + BETA_ROWS_PER_WG; row += G) {
		const long idx = (long)row * RP + c;
		T v = 0;
		if (row < out_valid && c < r) {
			T nu = 0, de = 0;
			for (int s = 0; s < slabs; ++s) {
				nu += num_part[(long)s * part_stride + idx];
				if (!vec_den) de += den_part[(long)s * part_stride + idx];
			}
			if (vec_den) de = dvec;
			const T a = P[idx];
			const T d = de + e_v + l1_v + l2_v * a;
			T quo;
			if (ONLINE) {
				T ap = a;
				if (power == 1) ap = a * a;
				else if (power == 2) ap = a > T(0) ? exp2(ig_v * log2(a)) : T(0);
				const T an = rho_v * Aacc[idx] + ap * nu;
				const T bn = rho_v * Bacc[idx] + d;
				Aacc[idx] = an;
				Bacc[idx] = bn;
				quo = an / bn;
			} else {
				quo = nu / d;
			}
			T f = quo;
			if (power == 1) f = sqrt(quo);
			else if (power == 2) f = quo > T(0) ? exp2(g_v * log2(quo)) : T(0);
			v = ONLINE ? f : a * f;
			if (flush && v < e_v) v = T(0);
		}
		P[idx] = v;
		sm += v;
	}
	if (sum_part != nullptr) {
		// the workgroup's rows of one column in ascending order of the thread's first row
		s_sm[threadIdx.x] = sm;
		__syncthreads();
		if ((int)threadIdx.x < RP) {
			T b = s_sm[c];
			for (int k = 1; k < G; ++k) b += s_sm[k * RP + c];
			sum_part[(long)blockIdx.x * RP + c] = b;
		}
	}
}

template <typename T>
hipError_t launch_beta_update_rows(T* P, T* Aacc, T* Bacc, const T* num_part, const T* den_part, long part_stride, int slabs, const T* dsum, int RP, int r, int out_pad,
                                   int out_valid, T eps, double beta_value, T l1, T l2, bool online, T rho, bool flush, T* sum_part, hipStream_t stream) {
	// gamma: launch_beta_update's rule
	const double b = (double)(T)beta_value;
	const bool vec_den = b == 1.0;
	const double gamma = b < 1.0 ? 1.0 / (2.0 - b) : b <= 2.0 ? 1.0 : 1.0 / (b - 1.0);
	const int power = gamma == 1.0 ? 0 : gamma == 0.5 ? 1 : 2;
	if (!beta_half_step_available(RP) || !std::isfinite(b) || !(l1 >= T(0)) || !(l2 >= T(0)) || !std::isfinite((double)l1) || !std::isfinite((double)l2) ||
	    out_pad <= 0 || out_pad % 128 != 0 || out_valid < 0 || out_valid > out_pad || slabs < 1 || r < 1 || r > RP || P == nullptr || num_part == nullptr ||
	    (vec_den ? dsum == nullptr : den_part == nullptr) || part_stride < (long)out_pad * RP)
		return hipErrorInvalidValue;
	if (online && (Aacc == nullptr || Bacc == nullptr || !(rho >= T(0)) || !(rho <= T(1)))) return hipErrorInvalidValue;
	const dim3 grid((unsigned)(out_pad / BETA_ROWS_PER_WG)), block(256);
	if (online)
		hipLaunchKernelGGL((k_beta_update_rows<T, true>), grid, block, 0, stream, P, Aacc, Bacc, num_part, den_part, part_stride, slabs, dsum, RP, r, out_valid, eps,
		                   vec_den ? 1 : 0, power, (T)gamma, (T)(1.0 / gamma), l1, l2, rho, flush ? 1 : 0, sum_part);
	else
		hipLaunchKernelGGL((k_beta_update_rows<T, false>), grid, block, 0, stream, P, (T*)nullptr, (T*)nullptr, num_part, den_part, part_stride, slabs, dsum, RP, r,
		                   out_valid, eps, vec_den ? 1 : 0, power, (T)gamma, (T)(1.0 / gamma), l1, l2, T(0), flush ? 1 : 0, sum_part);
	return hipGetLastError();
}
template hipError_t launch_beta_update_rows<float>(float*, float*, float*, const float*, const float*, long, int, const float*, int, int, int, int, float, double, float, float,
                                                   bool, float, bool, float*, hipStream_t);
template hipError_t launch_beta_update_rows<double>(double*, double*, double*, const double*, const double*, long, int, const double*, int, int, int, int, double, double, double,
                                                    double, bool, double, bool, double*, hipStream_t);

// A <- P, B <- 1 on whole panels of `count` elements: the accumulators of a minibatch engine whenever its factors are set
template <typename T>
__global__ __launch_bounds__(256) void k_beta_online_reset(const T* __restrict__ P, T* __restrict__ Aacc, T* __restrict__ Bacc, long count) {
	const long i = (long)blockIdx.x * 256 + threadIdx.x;
	if (i < count) { Aacc[i] = P[i]; Bacc[i] = T(1); }
}

template <typename T>
hipError_t launch_beta_online_reset(const T* P, T* Aacc, T* Bacc, long count, hipStream_t stream) {
	if (P == nullptr || Aacc == nullptr || Bacc == nullptr || count <= 0) return hipErrorInvalidValue;
	hipLaunchKernelGGL((k_beta_online_reset<T>), dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, P, Aacc, Bacc, count);
	return hipGetLastError();
}
template hipError_t launch_beta_online_reset<float>(const float*, float*, float*, long, hipStream_t);
template hipError_t launch_beta_online_reset<double>(const double*, double*, double*, long, hipStream_t);

} // namespace nmfamd
