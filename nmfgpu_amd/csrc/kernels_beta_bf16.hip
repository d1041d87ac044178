// kernels_beta_bf16.hip -- the mixed-precision form of the dense beta-divergence half-step (kernels_beta.hip; docs/DIVERGENCE.md, "Mixed precision"): the same
// launch, slab plan and partial panels as k_beta_fused_f32, with the operands of both products rounded to bf16 (round to nearest even) and the products on
// v_mfma_f32_32x32x16_bf16.  fp32: V, P + eps, the element-wise map, the error terms, every accumulation, the slabs' partial panels.  bf16: the panels A and B as they
// are staged into LDS, and Q and R in registers after the map.  k_beta_update runs on the fp32 master panels unchanged.
//
// This translation unit has its own text on purpose: a flag on the body of kernels_beta.hip reschedules the fp32 kernels (docs/DIVERGENCE.md, "Weighted").
//
// Operand maps (lane l: li = l & 31, h = l >> 5; wave (wo, wk) owns output columns 32 wo .. and reduction rows 32 wk .. of the tile):
//   first product   P(k, o) = sum_c B(k, c) A(o, c): K-step t covers c = 16 t .. 16 t + 15; the A operand is Bs[32 wk + li][16 t + 8 h + j], the B operand
//                   As[32 wo + li][16 t + 8 h + j], j = 0 .. 7 -- one 16-byte read each from the row images (rows padded by 16 bytes).
//                   The accumulator holds, in lane l, column o = li and rows k = (v & 3) + 8 (v >> 2) + 4 h, v = 0 .. 15.
//   second products num(o, c) = sum_k Q(k, o) B(k, c): the mapped accumulator IS the A operand -- registers 8 s .. 8 s + 7 converted pairwise are the fragment of
//                   K-step s (s = 0, 1), whose element j is row k(s, j, h) = 16 s + 8 (j >> 2) + 4 h + (j & 3).  The B operand's element j has to be B at that same
//                   row, column 32 ct + li: two 8-byte reads (j = 0 .. 3 at k = 16 s + 4 h, j = 4 .. 7 at k = 16 s + 4 h + 8) from a SECOND, k-major image of the
//                   B tile, Bt[c][k] (rows padded by 8 bytes: the 32 lanes of a half then cover the 64 banks once).
// The staging thread holds a 4 x 4 block of B (four rows, four columns): four 8-byte writes into the row image, four into the k-major image.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "kernels.h"
#include "split3.h"

namespace nmfamd {

typedef float mixed_f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t mixed_u32x2 __attribute__((ext_vector_type(2)));

constexpr int MIXED_GENERAL = 2;      // (the value of the BETA template parameter that takes beta at run time, as BETA_GENERAL of kernels_beta.hip)

__device__ inline float mixed_log2(float p) { return __builtin_amdgcn_logf(p); }
__device__ inline float mixed_exp2(float y) { return __builtin_amdgcn_exp2f(y); }

// two fp32 values to one dword of two bf16, round to nearest even (v_cvt_pk_bf16_f32): lo in bits 0 .. 15
__device__ inline uint32_t mixed_pack(float lo, float hi) {
	f32x2 pr; pr[0] = lo; pr[1] = hi;
	return __builtin_bit_cast(uint32_t, __builtin_convertvector(pr, bf16x2));
}

// the element-wise map and the error terms of one entry, fp32 (x = v, p = P + eps with P from the bf16 operands); padding entries give zeros and no terms
template <int BETA, bool TERMS>
__device__ inline void mixed_entry(float x, float p, bool valid, float be, float& q, float& rr, float& tf, float& td) {
	q = 0.f; rr = 0.f;
	if (!valid) return;
	if (BETA == 1) {
		q = x / p;
		if (TERMS) {
			const float d = x - p;
			tf += d * d;
			td += (x > 0.f ? x * log(q) : 0.f) - x + p;
		}
	} else if (BETA == MIXED_GENERAL) {
		const float t = mixed_exp2((be - 2.f) * mixed_log2(p));
		q = x * t;
		rr = t * p;
		if (TERMS) {
			const float d = x - p;
			tf += d * d;
			const float xb = x > 0.f ? mixed_exp2(be * mixed_log2(x)) : 0.f;
			td += xb + (be - 1.f) * (rr * p) - be * (x * rr);
		}
	} else {
		const float ip = 1.f / p;
		rr = ip;
		q = x * ip * ip;
		if (TERMS) {
			const float d = x - p, ratio = x * ip;
			tf += d * d;
			td += ratio - log(ratio) - 1.f;
		}
	}
}

// LDS, in bf16 elements: As [BO][RP + 8], Bs [KT][RP + 8], Bt [RP][KT + 4]
constexpr size_t mixed_lds_bytes(int RP, int BO, int KT) { return 2 * ((size_t)(BO + KT) * (RP + 8) + (size_t)RP * (KT + 4)); }

// WO x WK waves: WO tiles of 32 output columns, WK tiles of 32 reduction rows per step (WO * WK = 4)
template <int RP, int BETA, bool UPDATE, bool TERMS, int WO, int WK>
__global__ __launch_bounds__(256) void k_beta_fused_bf16(const float* __restrict__ X, long ldx, const float* __restrict__ A, const float* __restrict__ B, float eps, float bexp,
                                                         float* __restrict__ num_part, float* __restrict__ den_part, long part_stride,
                                                         float* __restrict__ tf_part, float* __restrict__ td_part, long t_stride,
                                                         int out_valid, int red_valid, int tiles_total, int tiles_per_slab) {
	constexpr int LD = RP + 8, LDT = 32 * WK + 4, BO = 32 * WO, KT = 32 * WK, NC = RP / 32;
	static_assert(WO * WK == 4, "four waves");
	static_assert((size_t)BO * RP * 4 <= 2 * ((size_t)KT * LD + (size_t)RP * LDT), "the combine region lies over the two B images");
	static_assert((BO * LD * 2) % 16 == 0 && (KT * LD * 2) % 16 == 0 && (LD * 2) % 16 == 0 && (LDT * 2) % 8 == 0, "16-byte row reads, 8-byte k-major reads");
	extern __shared__ __attribute__((aligned(16))) unsigned char mixed_smem[];
	uint16_t* As = reinterpret_cast<uint16_t*>(mixed_smem);      // [BO][LD]
	uint16_t* Bs = As + BO * LD;                                 // [KT][LD]
	uint16_t* Bt = Bs + KT * LD;                                 // [RP][LDT]
	const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
	const int wo = wave % WO, wk = wave / WO;
	const int li = lane & 31, h = lane >> 5;
	const int o0 = blockIdx.x * BO, slab = blockIdx.y;
	const int tile_begin = slab * tiles_per_slab, tile_end = min(tile_begin + tiles_per_slab, tiles_total);
	const int o = o0 + 32 * wo + li;
	const float e_v = in_vgpr(eps);
	const float b_v = BETA == MIXED_GENERAL ? in_vgpr(bexp) : 0.f;

	for (int idx = threadIdx.x * 4; idx < BO * RP; idx += 1024) {
		const int row = idx / RP, col = idx % RP;
		const float4 v = *reinterpret_cast<const float4*>(A + (long)(o0 + row) * RP + col);
		mixed_u32x2 w; w[0] = mixed_pack(v.x, v.y); w[1] = mixed_pack(v.z, v.w);
		*reinterpret_cast<mixed_u32x2*>(As + row * LD + col) = w;
	}

	mixed_f32x16 num[NC], den[NC];
#pragma unroll
	for (int ct = 0; ct < NC; ++ct)
#pragma unroll
		for (int v = 0; v < 16; ++v) { num[ct][v] = 0.f; den[ct][v] = 0.f; }
	float tf = 0.f, td = 0.f;

	for (int tile = tile_begin; tile < tile_end; ++tile) {
		const int kt = tile * KT;
		__syncthreads();      // (the previous tile's readers are done; the first pass: As is complete below)
		// a 4 x 4 block of the B tile per thread and pass: rows 4 rb .. 4 rb + 3, columns 4 cb .. 4 cb + 3
		for (int blk = threadIdx.x; blk < (KT / 4) * (RP / 4); blk += 256) {
			const int rb = blk / (RP / 4), cb = blk % (RP / 4);
			float4 v[4];
#pragma unroll
			for (int i = 0; i < 4; ++i) v[i] = *reinterpret_cast<const float4*>(B + (long)(kt + 4 * rb + i) * RP + 4 * cb);
			uint32_t lo[4], hi[4];      // row i: columns (0, 1) and (2, 3)
#pragma unroll
			for (int i = 0; i < 4; ++i) {
				lo[i] = mixed_pack(v[i].x, v[i].y); hi[i] = mixed_pack(v[i].z, v[i].w);
				mixed_u32x2 w; w[0] = lo[i]; w[1] = hi[i];
				*reinterpret_cast<mixed_u32x2*>(Bs + (4 * rb + i) * LD + 4 * cb) = w;
			}
			// the same sixteen bf16 values, k-major: column 4 cb + j holds rows 4 rb .. 4 rb + 3
#pragma unroll
			for (int j = 0; j < 4; ++j) {
				const uint32_t* src = j < 2 ? lo : hi;
				mixed_u32x2 w;
				if ((j & 1) == 0) {
					w[0] = (src[0] & 0xffffu) | (src[1] << 16);
					w[1] = (src[2] & 0xffffu) | (src[3] << 16);
				} else {
					w[0] = (src[0] >> 16) | (src[1] & 0xffff0000u);
					w[1] = (src[2] >> 16) | (src[3] & 0xffff0000u);
				}
				*reinterpret_cast<mixed_u32x2*>(Bt + (4 * cb + j) * LDT + 4 * rb) = w;
			}
		}
		// the V tile in the accumulator's layout: x[4 g + e] = X(o, kt + 32 wk + 8 g + 4 h + e), fp32 as it is
		float x[16];
		{
			const float* xr = X + (long)o * ldx + kt + 32 * wk + 4 * h;
#pragma unroll
			for (int g = 0; g < 4; ++g) {
				const float4 v = *reinterpret_cast<const float4*>(xr + 8 * g);
				x[4 * g] = v.x; x[4 * g + 1] = v.y; x[4 * g + 2] = v.z; x[4 * g + 3] = v.w;
			}
		}
		__syncthreads();
		// P(k, o) = sum_c B(k, c) A(o, c)
		mixed_f32x16 P;
#pragma unroll
		for (int v = 0; v < 16; ++v) P[v] = 0.f;
		{
			const uint16_t* bs = Bs + (32 * wk + li) * LD + 8 * h;
			const uint16_t* as = As + (32 * wo + li) * LD + 8 * h;
#pragma unroll
			for (int t = 0; t < RP / 16; ++t) {
				const bf16x8 fa = *reinterpret_cast<const bf16x8*>(bs + 16 * t);
				const bf16x8 fb = *reinterpret_cast<const bf16x8*>(as + 16 * t);
				P = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, P, 0, 0, 0);
			}
		}
		float q[16], rr[16];
#pragma unroll
		for (int v = 0; v < 16; ++v) {
			const int kk = kt + 32 * wk + (v & 3) + 8 * (v >> 2) + 4 * h;
			mixed_entry<BETA, TERMS>(x[v], P[v] + e_v, kk < red_valid && o < out_valid, b_v, q[v], rr[v], tf, td);
		}
		if (UPDATE) {
			const uint16_t* b2 = Bt + li * LDT + 32 * wk + 4 * h;
#pragma unroll
			for (int s = 0; s < 2; ++s) {
				// registers 8 s .. 8 s + 7 pairwise: the fragment of K-step s, element j = row 16 s + 8 (j >> 2) + 4 h + (j & 3)
				u32x4 qa, ra;
#pragma unroll
				for (int i = 0; i < 4; ++i) {
					qa[i] = mixed_pack(q[8 * s + 2 * i], q[8 * s + 2 * i + 1]);
					if (BETA != 1) ra[i] = mixed_pack(rr[8 * s + 2 * i], rr[8 * s + 2 * i + 1]);
				}
				const bf16x8 qf = __builtin_bit_cast(bf16x8, qa);
#pragma unroll
				for (int ct = 0; ct < NC; ++ct) {
					const uint16_t* bp = b2 + (32 * ct) * LDT + 16 * s;
					const mixed_u32x2 b_lo = *reinterpret_cast<const mixed_u32x2*>(bp);          // j = 0 .. 3: rows 16 s + 4 h + j
					const mixed_u32x2 b_hi = *reinterpret_cast<const mixed_u32x2*>(bp + 8);      // j = 4 .. 7: rows 16 s + 8 + 4 h + (j - 4)
					u32x4 bw; bw[0] = b_lo[0]; bw[1] = b_lo[1]; bw[2] = b_hi[0]; bw[3] = b_hi[1];
					const bf16x8 bop = __builtin_bit_cast(bf16x8, bw);
					num[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf, bop, num[ct], 0, 0, 0);
					if (BETA != 1) den[ct] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, ra), bop, den[ct], 0, 0, 0);
				}
			}
		}
	}
	__syncthreads();
	if (UPDATE) {
		// the WK waves of an output tile in wave order, through the region of the two B images; then the slab's partial panel rows, coalesced
		float* R = reinterpret_cast<float*>(Bs);
#pragma unroll
		for (int pass = 0; pass < (BETA != 1 ? 2 : 1); ++pass) {
			for (int w = 0; w < WK; ++w) {
				if (wk == w) {
#pragma unroll
					for (int ct = 0; ct < NC; ++ct)
#pragma unroll
						for (int v = 0; v < 16; ++v) {
							const int idx = (32 * wo + (v & 3) + 8 * (v >> 2) + 4 * h) * RP + 32 * ct + li;
							const float mine = pass == 0 ? num[ct][v] : den[ct][v];
							R[idx] = w == 0 ? mine : R[idx] + mine;
						}
				}
				__syncthreads();
			}
			float* dst = (pass == 0 ? num_part : den_part) + (long)slab * part_stride + (long)o0 * RP;
			for (int idx = threadIdx.x; idx < BO * RP; idx += 256) dst[idx] = R[idx];
			__syncthreads();
		}
	}
	if (TERMS) {
		if (BETA == MIXED_GENERAL) td *= 1.f / (b_v * (b_v - 1.f));
		// lane halves (h = 0 then 1), then the WK waves in order
		const float of = __shfl_xor(tf, 32), od = __shfl_xor(td, 32);
		const float sf = h == 0 ? tf + of : of + tf, sd = h == 0 ? td + od : od + td;
		static_assert(WK * BO * 2 * 4 <= BO * LD * 2, "the terms lie over the A image");
		float* Ts = reinterpret_cast<float*>(As);      // [WK][BO][2]
		if (h == 0) { Ts[(wk * BO + 32 * wo + li) * 2] = sf; Ts[(wk * BO + 32 * wo + li) * 2 + 1] = sd; }
		__syncthreads();
		if ((int)threadIdx.x < BO) {
			float a = 0.f, b = 0.f;
			for (int w = 0; w < WK; ++w) { a += Ts[(w * BO + threadIdx.x) * 2]; b += Ts[(w * BO + threadIdx.x) * 2 + 1]; }
			tf_part[(long)slab * t_stride + o0 + threadIdx.x] = a;
			td_part[(long)slab * t_stride + o0 + threadIdx.x] = b;
		}
	}
}

hipError_t launch_beta_fused_bf16(const float* X, long ldx, const float* A, const float* B, int RP, double beta_value, bool update, bool terms, float eps, const BetaPlan& plan,
                                  float* num_part, float* den_part, long part_stride, float* tf_part, float* td_part, long t_stride,
                                  int out_pad, int out_valid, int red_valid, hipStream_t stream) {
	// (the checks of launch_beta_fused<float>: the same plan, the same arguments)
	const float bexp = (float)beta_value;
	const int beta = bexp == 1.f ? 1 : bexp == 0.f ? 0 : MIXED_GENERAL;
	if (!beta_half_step_available(RP) || !std::isfinite((double)bexp) || (!update && !terms) || out_pad <= 0 || out_pad % 128 != 0 || plan.slabs < 1 ||
	    out_valid > out_pad || red_valid > (long)plan.tiles * plan.kt || ldx < (long)plan.tiles * plan.kt || ldx % 4 != 0)
		return hipErrorInvalidValue;
	if (update && (num_part == nullptr || (beta != 1 && den_part == nullptr))) return hipErrorInvalidValue;
	if (terms && (tf_part == nullptr || td_part == nullptr)) return hipErrorInvalidValue;
	if (plan.bo != (RP == 256 ? 64 : 32) || plan.kt != (RP == 256 ? 64 : 128)) return hipErrorInvalidValue;
	const dim3 grid((unsigned)(out_pad / plan.bo), (unsigned)plan.slabs), block(256);
	hipError_t e = hipSuccess;
#define NMFAMD_MIXED_GO(KERNEL, BYTES)                                                                                                                     \
	do {                                                                                                                                                   \
		static std::atomic<unsigned long long> done{0};                                                                                                    \
		e = allow_dynamic_lds(reinterpret_cast<const void*>(&KERNEL), (int)(BYTES), done);                                                                 \
		if (e != hipSuccess) return e;                                                                                                                     \
		hipLaunchKernelGGL(KERNEL, grid, block, (size_t)(BYTES), stream, X, ldx, A, B, eps, bexp, num_part, den_part, part_stride, tf_part, td_part, t_stride,   \
		                   out_valid, red_valid, plan.tiles, plan.tiles_per_slab);                                                                         \
	} while (0)
#define NMFAMD_MIXED_FORMS(RPV, BETAV, WO, WK)                                                                                                             \
	do {                                                                                                                                                   \
		constexpr size_t bytes = mixed_lds_bytes(RPV, 32 * WO, 32 * WK);                                                                                   \
		if (update && terms) NMFAMD_MIXED_GO((k_beta_fused_bf16<RPV, BETAV, true, true, WO, WK>), bytes);                                                  \
		else if (update) NMFAMD_MIXED_GO((k_beta_fused_bf16<RPV, BETAV, true, false, WO, WK>), bytes);                                                     \
		else NMFAMD_MIXED_GO((k_beta_fused_bf16<RPV, BETAV, false, true, WO, WK>), bytes);                                                                 \
	} while (0)
#define NMFAMD_MIXED_F32(RPV, WO, WK)                                                                                                                      \
	do {                                                                                                                                                   \
		if (beta == 1) NMFAMD_MIXED_FORMS(RPV, 1, WO, WK);                                                                                                 \
		else if (beta == MIXED_GENERAL) NMFAMD_MIXED_FORMS(RPV, MIXED_GENERAL, WO, WK);                                                                    \
		else NMFAMD_MIXED_FORMS(RPV, 0, WO, WK);                                                                                                           \
	} while (0)
	switch (RP) {
	case 64: NMFAMD_MIXED_F32(64, 1, 4); break;
	case 128: NMFAMD_MIXED_F32(128, 1, 4); break;
	default: NMFAMD_MIXED_F32(256, 2, 2); break;
	}
#undef NMFAMD_MIXED_F32
#undef NMFAMD_MIXED_FORMS
#undef NMFAMD_MIXED_GO
	return hipGetLastError();
}

} // namespace nmfamd
