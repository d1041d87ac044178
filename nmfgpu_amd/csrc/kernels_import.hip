// kernels_import.hip -- device-resident input and output (docs/DEVICE_IO.md): a caller's matrix in HBM, column-major or row-major with a leading dimension,
// into the column-major staging image of the upload (with the value rules of the host upload evaluated in the same pass), and the factor panels in both directions.
//
// One tile form serves every kernel here.  A workgroup of 256 threads moves a 64 x 64 tile through LDS:
//   phase 1  reads the tile along the SOURCE's contiguous index ("inner"; the other one is "outer") -- 16 bytes per lane where the pointer, the leading dimension and
//            the position allow it, element by element where they do not (an element-aligned pointer, an odd ld, the ragged edge) -- and stores it at
//                tile[outer * S + inner + (inner >> PS)]         one pad element after every 128 bytes of a row, S odd
//   phase 2  reads it with the lanes of a wave along the DESTINATION's contiguous index and stores 256 contiguous bytes (fp32) per wave instruction.
// Bank arithmetic (64 banks of 4 bytes; a ds_write_b32 / ds_read_b32 is serviced in two groups of 32 lanes, banks mod 32; ds_write_b64 in groups of 16 lanes;
// ds_read_b64 in two groups of 32 lanes, banks mod 64):
//   fp32, S = 65, PS = 5.  Phase 1, 16-byte form: 16 lanes cover one row, word k of lane l goes to outer * 65 + 4 l + k + (l >= 8): banks of residue k (l < 8) and
//     k + 1 (l >= 8) modulo 4, sixteen different ones; the other 16 lanes of the group take the row two further on (+130 = +2 modulo 32): residues k + 2 and k + 3.
//     Element form: 32 consecutive words of one row.  Phase 2 across the outer index: lane * 65 + c = lane + c modulo 32; along the inner index: consecutive words.
//   fp64, S = 67, PS = 4.  Phase 1: 16 lanes cover half a row, element k of lane l at dword 2 (outer * 67 + 2 l + k + (l >= 8)): 4 l + 2 k and 4 (l - 8) + 2 k + 2
//     modulo 32, sixteen different banks.  Phase 2 across the outer index: dword 2 (lane * 67 + c), 2 * 67 lane modulo 64 takes 32 different even values.
// So neither the store nor the transposed read has a bank conflict, in either precision.  The one exception is the UNtransposed read in fp64 (lanes along the inner
// index): dwords 2 (lane + (lane >> 4)) of 32 lanes span 66 dwords, so the last lane of a group meets the first one's bank (one two-way pair per group).
//
// Nothing here adds floating-point numbers with atomics: violations of a value rule are bits OR-ed into one int (order-independent), the sum of the weights is one
// double per workgroup, added by a fixed butterfly over the lanes and then over the four waves in order, and the caller adds the workgroups' partials in index
// order.  Sources are const and never written.
#include <hip/hip_runtime.h>

#include "io_tile.h"
#include "kernels.h"

namespace nmfamd {

namespace {

// rule: 0 none, 1 finite and >= 0, 2 finite and > 0.  One workgroup per 64 x 64 tile of the PADDED image (rows_pad x cols_pad, multiples of 64): what lies beyond
// rows x cols is written as 0.
template <typename T>
__global__ __launch_bounds__(256) void k_import_dense(const T* __restrict__ src, long ld, int row_major, int vec, int rows, int cols, T* __restrict__ dst, long ldd,
                                                       unsigned tiles_i, int rule, int* __restrict__ flags) {
	__shared__ T tile[64 * IoTile<T>::S];
	const long i0 = (long)(blockIdx.x % tiles_i) * 64, j0 = (long)(blockIdx.x / tiles_i) * 64;
	if (row_major) io_tile_load<T>(tile, src, ld, vec != 0, i0, j0, rows, cols);
	else io_tile_load<T>(tile, src, ld, vec != 0, j0, i0, cols, rows);
	__syncthreads();
	const int il = threadIdx.x & 63, w = threadIdx.x >> 6;
	bool bad = false;
#pragma unroll 4
	for (int q = 0; q < 16; ++q) {
		const int jl = w + 4 * q;
		const T v = io_tile_read<T>(tile, row_major != 0, il, jl);
		if (rule != 0 && i0 + il < rows && j0 + jl < cols) bad |= !io_finite(v) || v < T(0) || (rule == 2 && v == T(0));
		dst[(j0 + jl) * ldd + i0 + il] = v;
	}
	if (__any(bad) && il == 0) atomicOr(flags, IMPORT_BAD_VALUE);
}

// The joint rule of the weighted upload.  positive_rule: V > 0 (beta <= 0) instead of V >= 0 under a weight > 0.
template <typename T>
__global__ __launch_bounds__(256) void k_import_weighted(const T* __restrict__ V, long ldv, int v_row_major, int v_vec, const T* __restrict__ Om, long ldo, int o_row_major,
                                                          int o_vec, int rows, int cols, T* __restrict__ Vdst, T* __restrict__ Odst, long ldd, unsigned tiles_i,
                                                          int positive_rule, int* __restrict__ flags, double* __restrict__ wsum_part) {
	__shared__ T tile[64 * IoTile<T>::S];
	__shared__ double red[4];
	const long i0 = (long)(blockIdx.x % tiles_i) * 64, j0 = (long)(blockIdx.x / tiles_i) * 64;
	const int il = threadIdx.x & 63, w = threadIdx.x >> 6;
	T wv[16];
	if (o_row_major) io_tile_load<T>(tile, Om, ldo, o_vec != 0, i0, j0, rows, cols);
	else io_tile_load<T>(tile, Om, ldo, o_vec != 0, j0, i0, cols, rows);
	__syncthreads();
#pragma unroll
	for (int q = 0; q < 16; ++q) wv[q] = io_tile_read<T>(tile, o_row_major != 0, il, w + 4 * q);
	__syncthreads();
	if (v_row_major) io_tile_load<T>(tile, V, ldv, v_vec != 0, i0, j0, rows, cols);
	else io_tile_load<T>(tile, V, ldv, v_vec != 0, j0, i0, cols, rows);
	__syncthreads();
	bool bad_w = false, bad_v = false, some = false;
	double sum = 0;
#pragma unroll
	for (int q = 0; q < 16; ++q) {
		const int jl = w + 4 * q;
		const T wt = wv[q];
		T v = T(0);
		if (i0 + il < rows && j0 + jl < cols) {
			if (!io_finite(wt) || wt < T(0)) bad_w = true;
			else if (wt > T(0)) {
				v = io_tile_read<T>(tile, v_row_major != 0, il, jl);
				bad_v |= !io_finite(v) || v < T(0) || (positive_rule != 0 && v == T(0));
				some = true;
				sum += (double)wt;
			}
		}
		Vdst[(j0 + jl) * ldd + i0 + il] = v;      // (0 wherever the weight is 0, whatever V holds there)
		Odst[(j0 + jl) * ldd + i0 + il] = wt;
	}
	const int f = (__any(bad_w) ? IMPORT_BAD_WEIGHT : 0) | (__any(bad_v) ? IMPORT_BAD_VALUE : 0) | (__any(some) ? IMPORT_SOME_WEIGHT : 0);
	// (IMPORT_SOME_WEIGHT is every wave's news: one atomic per wave on one address would outlast the copy, so a wave adds only bits the word does not show yet --
	//  a stale read costs a redundant atomic, never a bit)
	if (f != 0 && il == 0 && (f & ~__atomic_load_n(flags, __ATOMIC_RELAXED)) != 0) atomicOr(flags, f);
	// the workgroup's sum: a butterfly inside each wave (the pairing is fixed by the lane numbers), then the four waves in order
#pragma unroll
	for (int s = 32; s > 0; s >>= 1) sum += __shfl_xor(sum, s, 64);
	if (il == 0) red[w] = sum;
	__syncthreads();
	if (threadIdx.x == 0) wsum_part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// Panel [len_pad][RP] (coordinate c of entry j at panel[j * RP + c]) -> the caller's r x len block: dst(c, j) at dst[j * ld + c] (along_c) or dst[c * ld + j].
// Nothing is written outside the block.
template <typename T>
__global__ __launch_bounds__(256) void k_export_panel(const T* __restrict__ panel, int RP, int r, int len, T* __restrict__ dst, long ld, int along_c, unsigned tiles_c) {
	__shared__ T tile[64 * IoTile<T>::S];
	const long c0 = (long)(blockIdx.x % tiles_c) * 64, j0 = (long)(blockIdx.x / tiles_c) * 64;
	io_tile_load<T>(tile, panel, RP, true, j0, c0, len, r);
	__syncthreads();
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll 4
	for (int q = 0; q < 16; ++q) {
		const int f = w + 4 * q;
		if (along_c) {
			const long c = c0 + lane, j = j0 + f;
			if (c < r && j < len) dst[j * ld + c] = tile[IoTile<T>::at(f, lane)];
		} else {
			const long j = j0 + lane, c = c0 + f;
			if (c < r && j < len) dst[c * ld + j] = tile[IoTile<T>::at(lane, f)];
		}
	}
}

} // namespace

template <typename T>
hipError_t launch_import_dense(const T* src, long ld, int layout, int rows, int cols, T* dst, long ldd, long rows_pad, long cols_pad, int rule, int* flags, hipStream_t stream) {
	if (rows_pad % 64 != 0 || cols_pad % 64 != 0 || rows > rows_pad || cols > cols_pad || ldd < rows_pad || (layout != 0 && layout != 1) || rule < 0 || rule > 2) return hipErrorInvalidValue;
	const unsigned long long ti = (unsigned long long)(rows_pad / 64), tj = (unsigned long long)(cols_pad / 64);
	if (ti * tj == 0) return hipSuccess;
	if (ti * tj > 0x7fffffffull) return hipErrorInvalidValue;
	hipLaunchKernelGGL((k_import_dense<T>), dim3((unsigned)(ti * tj)), dim3(256), 0, stream, src, ld, layout, aligned16(src, ld, sizeof(T)) ? 1 : 0, rows, cols, dst, ldd,
	                   (unsigned)ti, rule, flags);
	return hipGetLastError();
}
template hipError_t launch_import_dense<float>(const float*, long, int, int, int, float*, long, long, long, int, int*, hipStream_t);
template hipError_t launch_import_dense<double>(const double*, long, int, int, int, double*, long, long, long, int, int*, hipStream_t);

long import_weighted_parts(long rows_pad, long cols_pad) { return (rows_pad / 64) * (cols_pad / 64); }

template <typename T>
hipError_t launch_import_weighted(const T* V, long ldv, int layoutV, const T* Omega, long ldo, int layoutO, int rows, int cols, T* Vdst, T* Odst, long ldd, long rows_pad,
                                  long cols_pad, int positive_rule, int* flags, double* wsum_part, hipStream_t stream) {
	if (rows_pad % 64 != 0 || cols_pad % 64 != 0 || rows > rows_pad || cols > cols_pad || ldd < rows_pad || (layoutV != 0 && layoutV != 1) || (layoutO != 0 && layoutO != 1)) return hipErrorInvalidValue;
	const unsigned long long ti = (unsigned long long)(rows_pad / 64), tj = (unsigned long long)(cols_pad / 64);
	if (ti * tj == 0) return hipSuccess;
	if (ti * tj > 0x7fffffffull) return hipErrorInvalidValue;
	hipLaunchKernelGGL((k_import_weighted<T>), dim3((unsigned)(ti * tj)), dim3(256), 0, stream, V, ldv, layoutV, aligned16(V, ldv, sizeof(T)) ? 1 : 0, Omega, ldo, layoutO,
	                   aligned16(Omega, ldo, sizeof(T)) ? 1 : 0, rows, cols, Vdst, Odst, ldd, (unsigned)ti, positive_rule, flags, wsum_part);
	return hipGetLastError();
}
template hipError_t launch_import_weighted<float>(const float*, long, int, const float*, long, int, int, int, float*, float*, long, long, long, int, int*, double*, hipStream_t);
template hipError_t launch_import_weighted<double>(const double*, long, int, const double*, long, int, int, int, double*, double*, long, long, long, int, int*, double*, hipStream_t);

// The panel is the column-major RP x len_pad matrix P(c, j); a factor given as W (len x r) is its transpose, so its layout changes sides.
template <typename T>
hipError_t launch_import_panel(const T* src, long ld, int layout, bool is_w, int r, int len, T* panel, int RP, long len_pad, hipStream_t stream) {
	if (layout != 0 && layout != 1) return hipErrorInvalidValue;
	return launch_import_dense<T>(src, ld, is_w ? 1 - layout : layout, r, len, panel, RP, RP, len_pad, 0, nullptr, stream);
}
template hipError_t launch_import_panel<float>(const float*, long, int, bool, int, int, float*, int, long, hipStream_t);
template hipError_t launch_import_panel<double>(const double*, long, int, bool, int, int, double*, int, long, hipStream_t);

template <typename T>
hipError_t launch_export_panel(const T* panel, int RP, long len_pad, bool is_w, int r, int len, T* dst, long ld, int layout, hipStream_t stream) {
	if ((layout != 0 && layout != 1) || RP % 64 != 0 || r > RP || len > len_pad || len_pad % 64 != 0) return hipErrorInvalidValue;
	const unsigned long long tc = (unsigned long long)((r + 63) / 64), tj = (unsigned long long)((len + 63) / 64);
	if (tc * tj == 0) return hipSuccess;
	if (tc * tj > 0x7fffffffull) return hipErrorInvalidValue;
	// H (r x len): column-major = contiguous along c; W (len x r): row-major = contiguous along c
	const int along_c = (is_w ? layout == 1 : layout == 0) ? 1 : 0;
	hipLaunchKernelGGL((k_export_panel<T>), dim3((unsigned)(tc * tj)), dim3(256), 0, stream, panel, RP, r, len, dst, ld, along_c, (unsigned)tc);
	return hipGetLastError();
}
template hipError_t launch_export_panel<float>(const float*, int, long, bool, int, int, float*, long, int, hipStream_t);
template hipError_t launch_export_panel<double>(const double*, int, long, bool, int, int, double*, long, int, hipStream_t);

} // namespace nmfamd
