// kernels_topk.hip -- the k best candidates of W H per query, product and selection in one launch (docs/TOPK.md).
//
// A query panel A and a candidate panel B of one layout (element (k, i) at [i * RP + k]); a query q names a row of A, the candidates are rows 0 ... count - 1 of B,
//     s(q, j) = sum_{k < r} A(queries[q], k) B(j, k)                                  (no eps)
// and per query the first k candidates in the total order (score descending, equal scores by ascending index) come back, candidates of the query's exclusion list
// left out.  No score goes to global memory: the product lands in MFMA accumulators and the selection reads them there.
//
// Work split.  A WAVE owns QW queries (32 in fp32: one 32 x 32 accumulator tile of v_mfma_f32_32x32x2_f32; 16 in fp64: v_mfma_f64_16x16x4_f64), a workgroup of nw <= 4
// waves a tile of nw * QW queries and one slab of candidates (blockIdx.y; slabs * slab_tiles tiles of QW candidates cover the count).  Every wave of the workgroup
// walks the whole slab against its own queries, so the waves share the candidate rows they load (the same addresses, close in time) and nothing else: the query rows,
// the lists and the exclusion bits of a query belong to one wave, and the only barriers are one per SEGMENT of TOPK_SEGMENT_TILES tiles, which keeps the waves near
// each other.  The wave gathers its query rows into LDS once, coordinates k >= r selected to zero; a lane loads 16 bytes of its candidate row per round, selected
// likewise (never multiplied by zero: the padding may hold anything), and the same 16 bytes of its query row from LDS.  Coordinate k sits in round c = k / 8, lane
// group g = (k % 8) / EL and element e = k % EL (EL = 4 floats, 2 doubles); MFMA step (c, e) multiplies the coordinates 8 c + EL g + e of all groups g.  Both operands
// use that map and it is the same for every pair, so a score is ONE chain over k whichever tile, wave, slab or call the pair lands in.  Rounds past r are skipped.
// A candidate slot at or past the count loads row count - 1 and is made ineligible by its index.
//
// Selection.  Per query a sorted list of its best k (score, index) so far in LDS, empty slots (-inf, TOPK_NONE).  Per accumulator register the lanes of a group hold
// the scores of one query against the tile's candidates; a lane tests eligibility (index below the count, query slot in use, exclusion bit clear) and compares with
// the query's k-th entry (kept in a register, read again after an insertion); a wave ballot tells whether anything gets in at all.  The lanes that pass are taken in lane order: the wave reads the list (lane p entry
// p), counts the entries that come before the newcomer, and shifts the tail by one.  A NaN compares false with everything and never enters a list.
// Exclusion.  Per segment the wave clears its queries' rows of a bitmap (QW queries x TOPK_SEGMENT_TILES * QW bits), walks their exclusion lists and sets the bits
// of the entries that fall into the segment with LDS atomics.
// k_topk_merge: one wave per query reduces the `slabs` partial lists to the final k in the same order, adds the base, fills with -1 / -inf.
// No index is checked here: k_topk_validate (or the host) comes first.  No float atomics; a repeated launch is bit-identical.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <limits>

#include "kernels.h"
#include "split3.h"

namespace nmfamd {

namespace {

constexpr int TOPK_NONE = 0x7fffffff;      // the index of an empty list slot: behind every candidate in the total order

typedef float tk_f32x16 __attribute__((ext_vector_type(16)));
typedef double tk_f64x4 __attribute__((ext_vector_type(4)));

template <typename T> struct TopkShape;
template <> struct TopkShape<float> {
	typedef float chunk_t __attribute__((ext_vector_type(4)));
	typedef tk_f32x16 acc_t;
	static constexpr int QW = 32, EL = 4, ACC = 16;
	__device__ static inline acc_t mfma(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
	// the query (row of the accumulator tile) that register v of a lane holds; its candidate is lane % QW
	__device__ static inline int row(int v, int lane) { return 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3); }
};
template <> struct TopkShape<double> {
	typedef double chunk_t __attribute__((ext_vector_type(2)));
	typedef tk_f64x4 acc_t;
	static constexpr int QW = 16, EL = 2, ACC = 4;
	__device__ static inline acc_t mfma(double a, double b, acc_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
	__device__ static inline int row(int v, int lane) { return (lane >> 4) + 4 * v; }
};

// a comes before b in the total order: score descending, equal scores (-0 = +0) by ascending index
template <typename T>
__device__ inline bool topk_before(T sa, int ia, T sb, int ib) { return sa > sb || (sa == sb && ia < ib); }

// the value of a lane whose number is uniform over the wave (it comes from a ballot): a read of that lane's register, no LDS round trip
__device__ inline int topk_lane(int x, int lane) { return __builtin_amdgcn_readlane(x, lane); }
__device__ inline float topk_lane(float x, int lane) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), lane)); }
__device__ inline double topk_lane(double x, int lane) {
	const unsigned long long b = __builtin_bit_cast(unsigned long long, x);
	const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, lane), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), lane);
	return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

__device__ inline int topk_shfl(int x, int lane) { return __shfl(x, lane); }
__device__ inline float topk_shfl(float x, int lane) { return __shfl(x, lane); }
__device__ inline double topk_shfl(double x, int lane) { return __shfl(x, lane); }

// LDS of a workgroup of nw waves, in bytes: query rows [nw * QW][RP + EL] of T, list scores [nw * QW][k] of T, list indices [nw * QW][k] of int, exclusion bits
// [nw * QW][TOPK_SEGMENT_TILES] of 32-bit words (QW <= 32 bits used per word)
template <typename T>
size_t topk_lds_bytes(int nw, int RP, int k) {
	const size_t qt = (size_t)nw * TopkShape<T>::QW;
	return qt * (size_t)(RP + TopkShape<T>::EL) * sizeof(T) + qt * (size_t)k * (sizeof(T) + sizeof(int)) + qt * TOPK_SEGMENT_TILES * sizeof(unsigned);
}

} // namespace

// part_s / part_i: [nq][gridDim.y][k], the slab's list of every query (indices 0-based, TOPK_NONE in empty slots).  slab_tiles: tiles of QW candidates per slab.
template <typename T>
__global__ __launch_bounds__(256) void k_topk_product(const int* __restrict__ queries, int nq, int k, int base, const T* __restrict__ A, const T* __restrict__ B,
                                                      int count, int RP, int r, const long* __restrict__ excl_ptr, const int* __restrict__ excl_idx, int slab_tiles,
                                                      T* __restrict__ part_s, int* __restrict__ part_i) {
	typedef TopkShape<T> S;
	typedef typename S::chunk_t chunk_t;
	typedef typename S::acc_t acc_t;
	constexpr int QW = S::QW, EL = S::EL, G = 64 / QW, ACC = S::ACC;
	extern __shared__ __attribute__((aligned(16))) unsigned char topk_smem[];
	const int nw = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int qt = nw * QW, LD = RP + EL;
	T* const a_all = reinterpret_cast<T*>(topk_smem);                                  // [qt][LD]
	T* const ls_all = a_all + (size_t)qt * LD;                                        // [qt][k]
	int* const li_all = reinterpret_cast<int*>(ls_all + (size_t)qt * k);               // [qt][k]
	unsigned* const bits_all = reinterpret_cast<unsigned*>(li_all + (size_t)qt * k);   // [qt][TOPK_SEGMENT_TILES]
	// this wave's share
	T* const a_w = a_all + (size_t)wave * QW * LD;
	T* const ls = ls_all + (size_t)wave * QW * k;
	int* const li = li_all + (size_t)wave * QW * k;
	unsigned* const bits = bits_all + (size_t)wave * QW * TOPK_SEGMENT_TILES;
	const long q0 = (long)blockIdx.x * qt + (long)wave * QW;      // first query slot of the wave
	const int qn = (int)max(0l, min((long)QW, (long)nq - q0));    // slots in use
	const int rounds = (r + 7) >> 3;                              // rounds of 8 coordinates that hold one below r
	const int sub = lane % QW, grp = lane / QW;

	// the query rows, by index, coordinates k >= r selected to zero (a slot not in use: zeros); the lists, empty
	for (int m = 0; m < QW; ++m) {
		const long row = m < qn ? (long)queries[q0 + m] - base : 0;
		const chunk_t* src = reinterpret_cast<const chunk_t*>(A + row * RP);
		for (int ch = lane; ch < rounds * G; ch += 64) {
			chunk_t x = src[ch];
#pragma unroll
			for (int e = 0; e < EL; ++e) x[e] = (m < qn && ch * EL + e < r) ? x[e] : T(0);
			*reinterpret_cast<chunk_t*>(a_w + (size_t)m * LD + ch * EL) = x;
		}
	}
	for (int p = lane; p < QW * k; p += 64) { ls[p] = -std::numeric_limits<T>::infinity(); li[p] = TOPK_NONE; }

	const int tile_lo = blockIdx.y * slab_tiles;
	const int tiles_all = (count + QW - 1) / QW;
	const int tile_hi = min(tile_lo + slab_tiles, tiles_all);
	// this lane's 16-byte chunks of its candidate row of a tile (a slot past the count: the last row, which exists; ineligible by its index below)
	auto cand_row = [&](int tile) { return reinterpret_cast<const chunk_t*>(B + (long)min(tile * QW + sub, count - 1) * RP) + grp; };
	chunk_t cur[4];
#pragma unroll
	for (int u = 0; u < 4; ++u) cur[u] = cand_row(tile_lo)[min(u, rounds - 1) * G];
	// the k-th entry of the list of the query that accumulator register v of this lane belongs to: read again from LDS only after an insertion under that register
	T thr_s[ACC]; int thr_i[ACC];
#pragma unroll
	for (int v = 0; v < ACC; ++v) { thr_s[v] = -std::numeric_limits<T>::infinity(); thr_i[v] = TOPK_NONE; }
	for (int seg_lo = tile_lo; seg_lo < tile_hi; seg_lo += TOPK_SEGMENT_TILES) {      // (uniform over the workgroup)
		const int seg_hi = min(seg_lo + TOPK_SEGMENT_TILES, tile_hi);
		__syncthreads();      // the waves stay within a segment of each other (and the first one: the LDS above is written)
		if (excl_ptr != nullptr) {
			for (int p = lane; p < QW * TOPK_SEGMENT_TILES; p += 64) bits[p] = 0u;
			__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
			__builtin_amdgcn_wave_barrier();
			const long c_lo = (long)seg_lo * QW, c_hi = (long)seg_hi * QW;
			for (int m = 0; m < qn; ++m) {
				const long e0 = excl_ptr[q0 + m], e1 = excl_ptr[q0 + m + 1];
				for (long e = e0 + lane; e < e1; e += 64) {
					const long c = (long)excl_idx[e] - base;
					if (c >= c_lo && c < c_hi) {
						const int o = (int)(c - c_lo);
						atomicOr(&bits[m * TOPK_SEGMENT_TILES + o / QW], 1u << (o % QW));
					}
				}
			}
			__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
			__builtin_amdgcn_wave_barrier();
		}
		for (int tile = seg_lo; tile < seg_hi; ++tile) {
			const int cand = tile * QW + sub;
			const chunk_t* bp = cand_row(tile);
			const chunk_t* bn = cand_row(min(tile + 1, tile_hi - 1));
			const T* ap = a_w + (size_t)sub * LD + grp * EL;
			acc_t acc;
#pragma unroll
			for (int v = 0; v < ACC; ++v) acc[v] = T(0);
			// four rounds of candidate chunks in flight while the four before them are multiplied; behind the last rounds of a tile, the first ones of the next
			// tile, which arrive during the selection (a round past the last one loads the last one again and is not used)
			chunk_t nxt[4];
			for (int c0 = 0; c0 < rounds; c0 += 4) {
				const bool last = c0 + 4 >= rounds;      // (uniform)
#pragma unroll
				for (int u = 0; u < 4; ++u) nxt[u] = last ? bn[min(u, rounds - 1) * G] : bp[min(c0 + 4 + u, rounds - 1) * G];
#pragma unroll
				for (int u = 0; u < 4; ++u) {
					const int c = c0 + u;
					if (c < rounds) {      // (uniform)
						const chunk_t xa = *reinterpret_cast<const chunk_t*>(ap + c * G * EL);
						const int k0 = (c * G + grp) * EL;
#pragma unroll
						for (int e = 0; e < EL; ++e) {
							const T be = k0 + e < r ? cur[u][e] : T(0);
							acc = S::mfma(xa[e], be, acc);
						}
					}
				}
#pragma unroll
				for (int u = 0; u < 4; ++u) cur[u] = nxt[u];
			}
			// selection on the accumulator tile: the exclusion words of the tile in one batch of LDS reads, the k-th entries from registers
			const int tl = tile - seg_lo;
			unsigned ex[ACC];
#pragma unroll
			for (int v = 0; v < ACC; ++v) ex[v] = excl_ptr != nullptr ? bits[S::row(v, lane) * TOPK_SEGMENT_TILES + tl] : 0u;
#pragma unroll
			for (int v = 0; v < ACC; ++v) {
				const int m = S::row(v, lane);
				const T sc = acc[v];
				const bool pass = cand < count && m < qn && ((ex[v] >> sub) & 1u) == 0u && topk_before<T>(sc, cand, thr_s[v], thr_i[v]);
				unsigned long long todo = __ballot(pass);
				const bool any = todo != 0ull;
				while (todo != 0ull) {      // (uniform) rare after the first tiles
					const int src = __ffsll((long long)todo) - 1;
					todo &= todo - 1ull;
					const T ns = topk_lane(sc, src);
					const int ni = tile * QW + src % QW, nm = S::row(v, src);
					T* const rs = ls + nm * k;
					int* const ri = li + nm * k;
					const bool held = lane < k;
					const T es = held ? rs[lane] : T(0);
					const int ei = held ? ri[lane] : 0;
					// the list is sorted: the entries before the newcomer are a prefix
					const int pos = __popcll(__ballot(held && topk_before<T>(es, ei, ns, ni)));
					__builtin_amdgcn_wave_barrier();
					if (pos < k) {      // (uniform; the k-th entry may have moved since the ballot)
						if (held && lane >= pos && lane + 1 < k) { rs[lane + 1] = es; ri[lane + 1] = ei; }
						if (lane == pos) { rs[pos] = ns; ri[pos] = ni; }
					}
					__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
					__builtin_amdgcn_wave_barrier();
				}
				if (any) {      // (uniform) the lists of this register's queries moved: their k-th entries again
					thr_s[v] = ls[m * k + k - 1];
					thr_i[v] = li[m * k + k - 1];
				}
			}
		}
	}
	// this slab's lists
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
	__builtin_amdgcn_wave_barrier();
	for (int m = 0; m < qn; ++m) {
		const long o = ((q0 + m) * (long)gridDim.y + blockIdx.y) * k;
		if (lane < k) { part_s[o + lane] = ls[m * k + lane]; part_i[o + lane] = li[m * k + lane]; }
	}
}

// One wave per query: the first k of the union of its `slabs` sorted lists (no candidate is in two of them).  A lane holds the heads of lists lane, lane + 64, ...
template <typename T>
__global__ __launch_bounds__(64) void k_topk_merge(const T* __restrict__ part_s, const int* __restrict__ part_i, int nq, int slabs, int k, int base,
                                                   int* __restrict__ out_idx, T* __restrict__ out_scores) {
	constexpr int OWN = TOPK_MAX_SLABS / 64;
	const int lane = threadIdx.x;
	const long q = blockIdx.x;
	const T* ps = part_s + q * slabs * (long)k;
	const int* pi = part_i + q * slabs * (long)k;
	const T ninf = -std::numeric_limits<T>::infinity();
	T hs[OWN]; int hi[OWN], pos[OWN];
#pragma unroll
	for (int u = 0; u < OWN; ++u) {
		const int l = lane + 64 * u;
		pos[u] = 0;
		hs[u] = l < slabs ? ps[(long)l * k] : ninf;
		hi[u] = l < slabs ? pi[(long)l * k] : TOPK_NONE;
	}
	for (int t = 0; t < k; ++t) {
		T bs = hs[0]; int bi = hi[0];
#pragma unroll
		for (int u = 1; u < OWN; ++u)
			if (topk_before<T>(hs[u], hi[u], bs, bi)) { bs = hs[u]; bi = hi[u]; }
#pragma unroll
		for (int w = 32; w > 0; w >>= 1) {
			const T os = topk_shfl(bs, lane ^ w);
			const int oi = topk_shfl(bi, lane ^ w);
			if (topk_before<T>(os, oi, bs, bi)) { bs = os; bi = oi; }
		}
		// (every lane holds the same winner; TOPK_NONE: every list is used up)
		const bool none = bi == TOPK_NONE;
		if (lane == 0) { out_idx[q * k + t] = none ? -1 : bi + base; out_scores[q * k + t] = none ? ninf : bs; }
		if (none) continue;
#pragma unroll
		for (int u = 0; u < OWN; ++u) {
			if (hi[u] == bi) {      // the one list that held it moves on
				const int l = lane + 64 * u;
				pos[u] += 1;
				hs[u] = pos[u] < k ? ps[(long)l * k + pos[u]] : ninf;
				hi[u] = pos[u] < k ? pi[(long)l * k + pos[u]] : TOPK_NONE;
			}
		}
	}
}

// first_bad[0] = the smallest q whose query lies outside [base, base + a_rows); first_bad[1] = the smallest q in 0 ... nq whose excl_ptr breaks the rule
// (excl_ptr[0] = 0, non-decreasing, excl_ptr[nq] = excl_nnz); first_bad[2] = the smallest e whose excluded index lies outside [base, base + count).  All start at
// 0xffffffff (the caller's fill) and are lowered by integer atomics.  Reads queries below nq, excl_ptr below nq + 1 and excl_idx below excl_nnz only: it does not
// trust excl_ptr for an extent.
__global__ __launch_bounds__(256) void k_topk_validate(const int* __restrict__ queries, long nq, int base, long a_rows, long count, const long* __restrict__ excl_ptr,
                                                       const int* __restrict__ excl_idx, long excl_nnz, unsigned* __restrict__ first_bad) {
	const long stride = (long)gridDim.x * blockDim.x, t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
	for (long q = t0; q < nq; q += stride) {
		const long i = (long)queries[q] - base;
		if (i < 0 || i >= a_rows) atomicMin(&first_bad[0], (unsigned)q);
	}
	if (excl_ptr == nullptr) return;
	for (long q = t0; q <= nq; q += stride) {
		const long p = excl_ptr[q];
		const bool ok = q == 0 ? p == 0 : p >= excl_ptr[q - 1];
		if (!ok || (q == nq && p != excl_nnz)) atomicMin(&first_bad[1], (unsigned)q);
	}
	for (long e = t0; e < excl_nnz; e += stride) {
		const long c = (long)excl_idx[e] - base;
		if (c < 0 || c >= count) atomicMin(&first_bad[2], (unsigned)min(e, 0xfffffffel));
	}
}

// Slabs of candidates per query tile: enough workgroups for 256 CUs when the queries are few, one slab when they are many; a function of (nq, count) only.
int topk_slabs(long nq, long count) {
	if (nq < 1 || count < 1) return 0;
	const long qtiles = (nq + 127) / 128, tiles = (count + 31) / 32;
	const long want = (TOPK_TARGET_WORKGROUPS + qtiles - 1) / qtiles;
	return (int)std::max(1l, std::min({want, tiles, (long)TOPK_MAX_SLABS}));
}

template <typename T>
int topk_waves(long nq, int RP, int k) {
	const int qw = TopkShape<T>::QW;
	int nw = (int)std::min(4l, (nq + qw - 1) / qw);
	while (nw > 1 && topk_lds_bytes<T>(nw, RP, k) > TOPK_LDS_LIMIT) --nw;
	return topk_lds_bytes<T>(nw, RP, k) <= TOPK_LDS_LIMIT ? nw : 0;
}
template int topk_waves<float>(long, int, int);
template int topk_waves<double>(long, int, int);

hipError_t launch_topk_validate(const int* queries, long nq, int base, long a_rows, long count, const long* excl_ptr, const int* excl_idx, long excl_nnz,
                                unsigned* first_bad, hipStream_t stream) {
	if (queries == nullptr || first_bad == nullptr || nq < 1 || nq > TOPK_MAX_QUERIES || a_rows < 1 || count < 1 || excl_nnz < 0 ||
	    (excl_ptr != nullptr && excl_nnz > 0 && excl_idx == nullptr))
		return hipErrorInvalidValue;
	const long most = std::max(nq + 1, excl_ptr != nullptr ? excl_nnz : 0l);
	const unsigned grid = (unsigned)std::min((most + 255) / 256, 2048l);
	hipLaunchKernelGGL(k_topk_validate, dim3(grid), dim3(256), 0, stream, queries, nq, base, a_rows, count, excl_ptr, excl_idx, excl_nnz, first_bad);
	return hipGetLastError();
}

template <typename T>
hipError_t launch_topk(const int* queries, long nq, int k, int base, const T* A, const T* B, long count, int RP, int r, const long* excl_ptr, const int* excl_idx,
                       int slabs, T* part_s, int* part_i, int* out_idx, T* out_scores, hipStream_t stream) {
	static std::atomic<unsigned long long> lds_done{0};
	constexpr int QW = TopkShape<T>::QW;
	if (queries == nullptr || A == nullptr || B == nullptr || part_s == nullptr || part_i == nullptr || out_idx == nullptr || out_scores == nullptr || nq < 1 ||
	    nq > TOPK_MAX_QUERIES || k < 1 || k > TOPK_MAX_K || (base != 0 && base != 1) || count < 1 || count > TOPK_MAX_CANDIDATES ||
	    !predict_rank_instantiated(RP, sizeof(T)) || r < 1 || r > RP || (excl_ptr != nullptr && excl_idx == nullptr))
		return hipErrorInvalidValue;
	const long tiles = (count + QW - 1) / QW;
	if (slabs == 0) slabs = topk_slabs(nq, count);
	if (slabs < 1 || slabs > TOPK_MAX_SLABS) return hipErrorInvalidValue;
	slabs = (int)std::min((long)slabs, tiles);
	const int slab_tiles = (int)((tiles + slabs - 1) / slabs);
	slabs = (int)((tiles + slab_tiles - 1) / slab_tiles);      // (no empty slab)
	const int nw = topk_waves<T>(nq, RP, k);
	if (nw < 1) return hipErrorInvalidValue;
	const size_t lds = topk_lds_bytes<T>(nw, RP, k);
	if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void*>(&k_topk_product<T>), TOPK_LDS_LIMIT, lds_done); e != hipSuccess) return e;
	const long qtiles = (nq + (long)nw * QW - 1) / ((long)nw * QW);
	hipLaunchKernelGGL((k_topk_product<T>), dim3((unsigned)qtiles, (unsigned)slabs), dim3(64 * nw), lds, stream, queries, (int)nq, k, base, A, B, (int)count, RP, r,
	                   excl_ptr, excl_idx, slab_tiles, part_s, part_i);
	if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
	hipLaunchKernelGGL((k_topk_merge<T>), dim3((unsigned)nq), dim3(64), 0, stream, part_s, part_i, (int)nq, slabs, k, base, out_idx, out_scores);
	return hipGetLastError();
}
template hipError_t launch_topk<float>(const int*, long, int, int, const float*, const float*, long, int, int, const long*, const int*, int, float*, int*, int*, float*,
                                       hipStream_t);
template hipError_t launch_topk<double>(const int*, long, int, int, const double*, const double*, long, int, int, const long*, const int*, int, double*, int*, int*,
                                        double*, hipStream_t);

} // namespace nmfamd
