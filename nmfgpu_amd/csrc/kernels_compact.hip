// kernels_compact.hip -- device-resident input of the sparse engines (docs/DEVICE_IO.md): a caller's DENSE matrix in HBM, column-major or row-major with a leading
// dimension, compacted straight into the CSR and the CSC image of its stored entries (missing values: every entry that is not NaN, zeros included; otherwise every
// entry != 0), and the value rules of a sparse upload evaluated over the caller's value array where it lies.
//
// The tile is the one of kernels_import.hip (io_tile.h): a workgroup of 256 threads loads a 64 x 64 tile along the source's contiguous index into LDS with the
// padded stride derived there, and then reads it BOTH ways -- a wave with its 64 lanes along the columns of one tile row, and with its lanes along the rows of one
// tile column (conflict-free in fp32 either way; in fp64 the read along the source's contiguous index has the one two-way pair per 32-lane group that file names).
// A wave's ballot of "this lane's entry is stored" is the occupancy mask of a tile row (or column); its popcount is the count, the popcount below a lane the rank.
//   1. k_compact_count    rowcnt[i][tile column] and colcnt[j][tile row]: every count has exactly one writer.  The tile's total goes into one 64-bit counter.
//   2. exclusive scans of the two flattened count arrays (k_sp_scan of kernels_sparse_setup.hip, launch_sp_scan): off_r[i][tc] is where the entries of row i
//      inside tile column tc start in the CSR image, so csr_ptr[i] = off_r[i][0] (k_compact_pointers); likewise off_c and the CSC image.
//   3. k_compact_scatter  the same tile again: csr_idx / csr_val at off_r[i][tc] + rank along the row, csc_idx / csc_val at off_c[j][tr] + rank along the column.
// Stored coordinates are unique, so the images are determined by the set of stored entries alone: CSR rows ascend in their columns (tile columns in order, ranks
// inside a tile in lane order), CSC columns in their rows -- what the host's stable sorts give (Engine::upload_triplets).  No sort, so no segment length limit.
// The only atomics are integer ones (flag bits, the 64-bit total): nothing depends on the order workgroups run in.  Sources are const and never written.
#include <hip/hip_runtime.h>

#include "io_tile.h"
#include "kernels.h"

namespace nmfamd {

namespace {

// the tile element at matrix coordinates (il, jl) relative to the tile's corner (il a row, jl a column)
template <typename T>
__device__ __forceinline__ T compact_at(const T* __restrict__ tile, bool row_major, int il, int jl) {
	return tile[row_major ? IoTile<T>::at(il, jl) : IoTile<T>::at(jl, il)];
}

// masked: stored = not NaN (an infinite entry is reported through *inf); otherwise stored = != 0 (-0 is a zero, NaN is stored: the host loop's `v != 0`)
template <typename T>
__device__ __forceinline__ bool compact_stored(T v, int masked, bool inside, bool* inf) {
	if (!inside) return false;
	if (masked) {
		if (v != v) return false;
		if (!io_finite(v)) *inf = true;
		return true;
	}
	return v != T(0);
}

__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }

template <typename T>
__device__ __forceinline__ void compact_tile_load(T* __restrict__ tile, const T* __restrict__ src, long ld, int row_major, int vec, long i0, long j0, int rows, int cols) {
	if (row_major) io_tile_load<T>(tile, src, ld, vec != 0, i0, j0, rows, cols);
	else io_tile_load<T>(tile, src, ld, vec != 0, j0, i0, cols, rows);
}

// One workgroup per 64 x 64 tile (tile row ti = blockIdx.x % tiles_i).  rowcnt: [rows][tiles_j], colcnt: [cols][tiles_i].
template <typename T>
__global__ __launch_bounds__(256) void k_compact_count(const T* __restrict__ src, long ld, int row_major, int vec, int rows, int cols, int masked, unsigned tiles_i, unsigned tiles_j,
                                                        int* __restrict__ rowcnt, int* __restrict__ colcnt, int* __restrict__ flags, unsigned long long* __restrict__ total) {
	__shared__ T tile[64 * IoTile<T>::S];
	__shared__ int wave_total[4];
	const unsigned ti = blockIdx.x % tiles_i, tj = blockIdx.x / tiles_i;
	const long i0 = (long)ti * 64, j0 = (long)tj * 64;
	compact_tile_load<T>(tile, src, ld, row_major, vec, i0, j0, rows, cols);
	__syncthreads();
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	bool inf = false;
	int sum = 0;      // (wave-uniform: the entries of this wave's tile rows)
#pragma unroll 4
	for (int q = 0; q < 16; ++q) {
		const int f = w + 4 * q;
		// tile row f, the lanes along its columns
		const bool sr = compact_stored(compact_at<T>(tile, row_major != 0, f, lane), masked, i0 + f < rows && j0 + lane < cols, &inf);
		const int cr = __popcll(__ballot(sr));
		if (lane == 0 && i0 + f < rows) rowcnt[(i0 + f) * tiles_j + tj] = cr;
		sum += cr;
		// tile column f, the lanes along its rows
		const bool sc = compact_stored(compact_at<T>(tile, row_major != 0, lane, f), masked, i0 + lane < rows && j0 + f < cols, &inf);
		const int cc = __popcll(__ballot(sc));
		if (lane == 0 && j0 + f < cols) colcnt[(j0 + f) * tiles_i + ti] = cc;
	}
	if (__any(inf) && lane == 0) atomicOr(flags, IMPORT_BAD_VALUE);
	if (lane == 0) wave_total[w] = sum;
	__syncthreads();
	if (threadIdx.x == 0) {
		const int t = wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
		if (t != 0) atomicAdd(total, (unsigned long long)t);
	}
}

// off_r: the scanned rowcnt ([rows][tiles_j] and the total behind it), off_c likewise.  Positions are checked against nnz before every store: the source is the
// caller's memory, and a count that no longer fits it must not become a store outside the images.  from_csr (or null): the CSR position of every CSC entry.
template <typename T>
__global__ __launch_bounds__(256) void k_compact_scatter(const T* __restrict__ src, long ld, int row_major, int vec, int rows, int cols, int masked, unsigned tiles_i, unsigned tiles_j,
                                                          const int* __restrict__ off_r, const int* __restrict__ off_c, long nnz, int* __restrict__ csr_idx, T* __restrict__ csr_val,
                                                          int* __restrict__ csc_idx, T* __restrict__ csc_val, int* __restrict__ from_csr) {
	__shared__ T tile[64 * IoTile<T>::S];
	__shared__ unsigned long long rowmask[64];
	const unsigned ti = blockIdx.x % tiles_i, tj = blockIdx.x / tiles_i;
	const long i0 = (long)ti * 64, j0 = (long)tj * 64;
	compact_tile_load<T>(tile, src, ld, row_major, vec, i0, j0, rows, cols);
	__syncthreads();
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	bool inf = false;      // (reported by the count; not looked at here)
#pragma unroll 4
	for (int q = 0; q < 16; ++q) {
		const int f = w + 4 * q;
		const T v = compact_at<T>(tile, row_major != 0, f, lane);
		const bool s = compact_stored(v, masked, i0 + f < rows && j0 + lane < cols, &inf);
		const unsigned long long mask = __ballot(s);
		if (lane == 0) rowmask[f] = mask;
		if (s) {
			const long pos = (long)off_r[(i0 + f) * tiles_j + tj] + __popcll(mask & lanes_below(lane));
			if (pos >= 0 && pos < nnz) { csr_idx[pos] = (int)(j0 + lane); csr_val[pos] = v; }
		}
	}
	__syncthreads();
#pragma unroll 4
	for (int q = 0; q < 16; ++q) {
		const int f = w + 4 * q;
		const T v = compact_at<T>(tile, row_major != 0, lane, f);
		const bool s = compact_stored(v, masked, i0 + lane < rows && j0 + f < cols, &inf);
		const unsigned long long mask = __ballot(s);
		if (s) {
			const long pos = (long)off_c[(j0 + f) * tiles_i + ti] + __popcll(mask & lanes_below(lane));
			if (pos >= 0 && pos < nnz) {
				csc_idx[pos] = (int)(i0 + lane); csc_val[pos] = v;
				if (from_csr != nullptr) from_csr[pos] = off_r[(i0 + lane) * tiles_j + tj] + __popcll(rowmask[lane] & lanes_below(f));
			}
		}
	}
}

// ptr[s] = off[s * per] for s < segments, ptr[segments] = off[segments * per] (the total the scan wrote behind its last element)
__global__ __launch_bounds__(256) void k_compact_pointers(const int* __restrict__ off, int segments, unsigned per, int* __restrict__ ptr) {
	const long s = (long)blockIdx.x * 256 + threadIdx.x;
	if (s <= segments) ptr[s] = off[s * per];
}

// rule 1: finite and >= 0, rule 2: finite, rule 3: finite and > 0
template <typename T>
__global__ __launch_bounds__(256) void k_sparse_value_rule(const T* __restrict__ values, long nnz, int rule, int* __restrict__ flags) {
	const long p = (long)blockIdx.x * 256 + threadIdx.x;
	bool bad = false;
	if (p < nnz) { const T v = values[p]; bad = !io_finite(v) || (rule == 1 && v < T(0)) || (rule == 3 && !(v > T(0))); }
	if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flags, IMPORT_BAD_VALUE);
}

bool compact_grid(int rows, int cols, unsigned long long* ti, unsigned long long* tj) {
	if (rows <= 0 || cols <= 0) return false;
	*ti = ((unsigned long long)rows + 63) / 64; *tj = ((unsigned long long)cols + 63) / 64;
	// (the flattened count arrays are scanned by one launch whose length is an int)
	return *ti * *tj <= 0x7fffffffull && (unsigned long long)rows * *tj < 0x7fffffffull && (unsigned long long)cols * *ti < 0x7fffffffull;
}

} // namespace

long compact_row_counts(int rows, int cols) { return (long)rows * (((long)cols + 63) / 64); }
long compact_col_counts(int rows, int cols) { return (long)cols * (((long)rows + 63) / 64); }

template <typename T>
hipError_t launch_compact_count(const T* src, long ld, int layout, int rows, int cols, int masked, int* rowcnt, int* colcnt, int* flags, unsigned long long* total, hipStream_t stream) {
	unsigned long long ti = 0, tj = 0;
	if ((layout != 0 && layout != 1) || !compact_grid(rows, cols, &ti, &tj)) return hipErrorInvalidValue;
	hipLaunchKernelGGL((k_compact_count<T>), dim3((unsigned)(ti * tj)), dim3(256), 0, stream, src, ld, layout, aligned16(src, ld, sizeof(T)) ? 1 : 0, rows, cols, masked, (unsigned)ti,
	                   (unsigned)tj, rowcnt, colcnt, flags, total);
	return hipGetLastError();
}
template hipError_t launch_compact_count<float>(const float*, long, int, int, int, int, int*, int*, int*, unsigned long long*, hipStream_t);
template hipError_t launch_compact_count<double>(const double*, long, int, int, int, int, int*, int*, int*, unsigned long long*, hipStream_t);

hipError_t launch_compact_pointers(const int* off_r, const int* off_c, int rows, int cols, int* csr_ptr, int* csc_ptr, hipStream_t stream) {
	unsigned long long ti = 0, tj = 0;
	if (!compact_grid(rows, cols, &ti, &tj)) return hipErrorInvalidValue;
	hipLaunchKernelGGL(k_compact_pointers, dim3((unsigned)(rows / 256 + 1)), dim3(256), 0, stream, off_r, rows, (unsigned)tj, csr_ptr);
	hipLaunchKernelGGL(k_compact_pointers, dim3((unsigned)(cols / 256 + 1)), dim3(256), 0, stream, off_c, cols, (unsigned)ti, csc_ptr);
	return hipGetLastError();
}

template <typename T>
hipError_t launch_compact_scatter(const T* src, long ld, int layout, int rows, int cols, int masked, const int* off_r, const int* off_c, long nnz, int* csr_idx, T* csr_val,
                                  int* csc_idx, T* csc_val, int* from_csr, hipStream_t stream) {
	unsigned long long ti = 0, tj = 0;
	if ((layout != 0 && layout != 1) || nnz < 0 || !compact_grid(rows, cols, &ti, &tj)) return hipErrorInvalidValue;
	if (nnz == 0) return hipSuccess;
	hipLaunchKernelGGL((k_compact_scatter<T>), dim3((unsigned)(ti * tj)), dim3(256), 0, stream, src, ld, layout, aligned16(src, ld, sizeof(T)) ? 1 : 0, rows, cols, masked, (unsigned)ti,
	                   (unsigned)tj, off_r, off_c, nnz, csr_idx, csr_val, csc_idx, csc_val, from_csr);
	return hipGetLastError();
}
template hipError_t launch_compact_scatter<float>(const float*, long, int, int, int, int, const int*, const int*, long, int*, float*, int*, float*, int*, hipStream_t);
template hipError_t launch_compact_scatter<double>(const double*, long, int, int, int, int, const int*, const int*, long, int*, double*, int*, double*, int*, hipStream_t);

template <typename T>
hipError_t launch_sparse_value_rule(const T* values, long nnz, int rule, int* flags, hipStream_t stream) {
	if (rule < 1 || rule > 3) return hipErrorInvalidValue;
	if (nnz <= 0) return hipSuccess;
	hipLaunchKernelGGL((k_sparse_value_rule<T>), dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, stream, values, nnz, rule, flags);
	return hipGetLastError();
}
template hipError_t launch_sparse_value_rule<float>(const float*, long, int, int*, hipStream_t);
template hipError_t launch_sparse_value_rule<double>(const double*, long, int, int*, hipStream_t);

} // namespace nmfamd
