// io_tile.h -- the 64 x 64 tile of the device-resident input and output kernels (kernels_import.hip has the layout and its bank arithmetic; kernels_compact.hip
// moves the same tile): the padded LDS stride, phase 1 (the load along the source's contiguous index) and the read of phase 2.  Internal header, device code.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nmfamd {

namespace {

template <typename T>
struct IoTile {
	static constexpr int VEC = 16 / (int)sizeof(T);            // elements per 16-byte load
	static constexpr int PS = sizeof(T) == 4 ? 5 : 4;          // one pad element after every 128 bytes
	static constexpr int S = 64 + (63 >> PS);                  // 65 / 67: odd
	static constexpr int LPR = 64 / VEC;                       // lanes per tile row in the 16-byte form
	struct alignas(16) Vec { T v[VEC]; };
	__device__ static int at(int outer, int inner) { return outer * S + inner + (inner >> PS); }
};

template <typename T>
__device__ __forceinline__ bool io_finite(T v) { return v - v == T(0); }

// Phase 1: the tile [outer0, outer0 + 64) x [inner0, inner0 + 64) of src (element (outer, inner) at src[outer * ld + inner]) into LDS, zeros outside
// outer_ext x inner_ext.  Never reads outside that extent.  vec: src and ld are multiples of 16 bytes.
template <typename T>
__device__ __forceinline__ void io_tile_load(T* __restrict__ tile, const T* __restrict__ src, long ld, bool vec, long outer0, long inner0, long outer_ext, long inner_ext) {
	using IT = IoTile<T>;
	const int t = threadIdx.x, lane = t & 63, w = t >> 6;
	if (vec) {
		const int sub = lane / IT::LPR, l = lane % IT::LPR;
		const int roff = sizeof(T) == 4 ? ((sub >> 1) | ((sub & 1) << 1)) : sub;      // (fp32: the two rows of one 32-lane group lie two apart, see above)
		constexpr int RPW = 64 / IT::LPR;                                              // rows per wave instruction
#pragma unroll
		for (int pass = 0; pass < 16 / RPW; ++pass) {
			const int ol = pass * 4 * RPW + w * RPW + roff;
			const long o = outer0 + ol, in = inner0 + (long)l * IT::VEC;
			typename IT::Vec x;
#pragma unroll
			for (int k = 0; k < IT::VEC; ++k) x.v[k] = T(0);
			if (o < outer_ext) {
				const T* p = src + o * ld + in;
				if (in + IT::VEC <= inner_ext) x = *reinterpret_cast<const typename IT::Vec*>(p);
				else {
#pragma unroll
					for (int k = 0; k < IT::VEC; ++k) if (in + k < inner_ext) x.v[k] = p[k];
				}
			}
#pragma unroll
			for (int k = 0; k < IT::VEC; ++k) tile[IT::at(ol, l * IT::VEC + k)] = x.v[k];
		}
	} else {
#pragma unroll 4
		for (int pass = 0; pass < 16; ++pass) {
			const int ol = pass * 4 + w;
			const long o = outer0 + ol, in = inner0 + lane;
			tile[IT::at(ol, lane)] = (o < outer_ext && in < inner_ext) ? src[o * ld + in] : T(0);
		}
	}
}

// Phase 2 as every kernel here runs it: thread t holds, for q = 0 .. 15, the element (il, jl) = (t & 63, (t >> 6) + 4 q) of the tile in the DESTINATION's
// coordinates (il along its contiguous index).  transposed: the source's inner index is the destination's outer one.
template <typename T>
__device__ __forceinline__ T io_tile_read(const T* __restrict__ tile, bool transposed, int il, int jl) {
	return tile[transposed ? IoTile<T>::at(il, jl) : IoTile<T>::at(jl, il)];
}

inline bool aligned16(const void* p, long ld, size_t elem) { return ((uintptr_t)p & 15) == 0 && ((size_t)ld * elem) % 16 == 0; }

} // namespace

} // namespace nmfamd
