// kernels.h -- launcher prototypes of the gfx950 kernels in kernels.hip (internal header).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <vector>

namespace nmfamd {

// How one factor product OUT(c, x) = sum_y F(c, y) A(x, y) is cut into workgroups.
struct FactorProductPlan {
	int th;           // x-tile height: 128 or 160 rows
	int xtiles;       // tiles of the output index x
	int steps_total;  // reduction length in MFMA K-steps (two y per step)
	int splits;       // workgroup slices of the reduction range = number of output slabs
	int nb;           // 32-wide N-blocks per wave tile: 2, or 1 when only the first 32 panel columns are needed (rank <= 32)
	int chunks;       // launches needed to cover RP = chunks * 64 factor rows
	int xhalves = 0;    // fp64 product: 64-row halves of x-tiles that hold valid rows
	int half_tiles = 0; // fp64 product: 1 = a workgroup takes one 64-row half of an x-tile and eight pieces of its K slice (kernels_f64.hip, RH = 1): small grids
	int col_split = 0; // split-operand product, RP = 64 only: 2 = a workgroup takes 32 of the 64 panel columns (twice the workgroups, half the MFMAs per K-step and
	                   // wave; the operand is split twice) -- for small reduction ranges, where the 128 x 64 form leaves most of the chip idle; same bits
};

FactorProductPlan plan_factor_product(int X, int Y, int RP, int num_cus);

// Optional passenger of a factor-product launch (rank-64 MU fast path, kernels_mu64.hip): reduce
// `parts` partial 64 x 64 Gram matrices into G, optionally turning its diagonal into column scales.
// Raises a kernel's dynamic LDS limit once per DEVICE (the attribute is per device; a process may switch
// devices through nmfgpu::chooseGpu).  `done` is the caller's static bit mask, one bit per device ordinal.
// (several threads may compute at once -- per-thread contexts, rank threads of a "numGpus" team: the mask is atomic; a lost
// race only repeats the idempotent hipFuncSetAttribute)
inline hipError_t allow_dynamic_lds(const void* kernel, int bytes, std::atomic<unsigned long long>& done) {
	int dev = 0;
	hipError_t e = hipGetDevice(&dev);
	if (e != hipSuccess) return e;
	if (dev >= 0 && dev < 64 && ((done.load(std::memory_order_acquire) >> dev) & 1ull)) return hipSuccess;
	e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
	if (e == hipSuccess && dev >= 0 && dev < 64) done.fetch_or(1ull << dev, std::memory_order_release);
	return e;
}

struct GramReduceArgs {
	const float* partials;  // [parts][4096]
	int parts;
	float* G;               // [4096]
	float* scale;           // [64] or nullptr
	int normalize;          // 1: scale = 1/sqrt(diag), G scaled on both sides; 0: scale = 1
	// the other kind of passenger (least-squares algorithms; fp32 kernel only, not together with the reduction):
	// inv_out <- (inv_a + regulariser)^-1, 64 x 64, one workgroup running k_inverse_gj64's body
	const float* inv_a = nullptr;
	float* inv_out = nullptr;
	float inv_offdiag = 0.f, inv_diag = 0.f;
	int inv_r = 0;
	// third kind (split-operand product only): G straight from the panel's split image instead of from partial matrices
	// (gram_image.h); image_ks = K-steps of 16 panel rows in the image (the all-zero step that closes it not counted)
	const void* image = nullptr;
	int image_ks = 0;
	// ... with normalize: the column scales from per-workgroup partial sums of squares the update kernel left ([colsq_parts][64], gram_image.h) instead of
	// from the diagonal of the product
	const float* colsq_part = nullptr;
	int colsq_parts = 0;
	// ... cut into ksplit slices of the K range (gram_image.h): 10 * ksplit passenger blocks, G then receives ksplit UNSCALED partial matrices ([ksplit][4096])
	// that the consumer adds and scales (launch_mu64_update32, qsplit); with normalize the scales must come from colsq_part
	int ksplit = 0;
	// ... or (spread > 0, the sixteen passengers of a whole problem): the ten tiles' K ranges dealt evenly to all GRAM_REDUCE_BLOCKS workgroups; G receives up to
	// GRAM_SPREAD_SLICES unscaled pieces per tile ([GRAM_SPREAD_SLICES][4096], absent pieces stay zero: the buffer is cleared once)
	int spread = 0;
	// ... and the LAST of the sixteen to finish adds the pieces in order and scales them as that consumer would -- (sum * scale[column]) * scale[row] -- into
	// spread_out (the finished 64 x 64 matrix); spread_counter: one word, zero between launches.  Its chain ends long before the product's, so the consumer gets one
	// finished matrix (the H update with three pieces to add took 6.8 us against 5.6)
	float* spread_out = nullptr;
	unsigned* spread_counter = nullptr;
	// fourth kind (bf16 factor product at padded rank 256 only, tri_gram_tile.h): the 256 x 256 Gram matrix of a panel from its bf16 fragments (tri_frags, tri_ks K-steps
	// of 16 panel rows) by TRI_PASSENGERS workgroups (K slices, the last one of a half reduces): G (fp32, both triangles), tri_diag (its diagonal, or nullptr), tri_x3 (its split image, or nullptr)
	const void* tri_frags = nullptr;
	int tri_ks = 0;
	void* tri_x3 = nullptr;
	float* tri_diag = nullptr;
	float* tri_partial = nullptr;       // [TRI_PASSENGERS / 2][36][1024] partial tiles
	unsigned* tri_counters = nullptr;   // two counters, zero between launches
	// fifth kind (split-operand product at padded ranks 128 ... 512, gram_wide.h): wide_parts K slices of every 128 x 128 super-block of the Gram matrix of the
	// fp32 panel wide_P (wide_len valid rows) as passenger workgroups -- what k_gram_wide_x3 does as a launch of its own; wide_partial: [wide_parts][RP][RP]
	// (blocks on and above the diagonal), reduced by launch_gram_reduce_x3 behind the product launch
	const float* wide_P = nullptr;
	int wide_len = 0, wide_parts = 0;
	float* wide_partial = nullptr;
};
constexpr int GRAM_REDUCE_BLOCKS = 16;
constexpr int TRI_PASSENGERS = 32;                 // tri_gram_tile.h: 16 K slices x 2 halves of the 36 upper-triangle tiles
constexpr int GRAM_IMAGE_TILES = 10;               // gram_image.h: upper triangle of the 4 x 4 grid of 16 x 16 tiles
constexpr int GRAM_SPREAD_SLICES = 3;              // ... pieces a tile arrives in when ten tiles are dealt to sixteen workgroups (gram_image.h, spread form)
constexpr int GRAM_KSPLIT_MAX = 8;                 // ... and the most K slices its K-split form is cut into
// What the Gram-from-image forms can serve (launch_gram_image_args, and the same request riding in launch_factor_product_x3).  A K-split or spread launch adds
// pieces of the K range, so no piece's diagonal is the column's sum of squares: with normalize the scales of these two forms must come from colsq_part.
// ... and the passenger workgroups such a request takes: what launch_gram_image_args launches and what launch_factor_product_x3 appends to the product's grid
inline int gram_image_workgroups(const GramReduceArgs& rg) { return rg.ksplit > 1 ? GRAM_IMAGE_TILES * rg.ksplit : GRAM_REDUCE_BLOCKS; }
inline bool gram_image_args_valid(const GramReduceArgs& rg) {
	const bool in_pieces = rg.ksplit > 1 || rg.spread > 0;
	return rg.image != nullptr && rg.ksplit <= GRAM_KSPLIT_MAX && !(in_pieces && rg.normalize != 0 && rg.colsq_part == nullptr);
}

// X: valid output length (the plan picks the tile height; panels must be allocated for xtiles * th rows).
// A is x-TILED: A(x, y) at A[(x/th) * tile_stride + y*th + x%th] (launch_tile / launch_tile_transposed).
// slabs: plan.splits partial results, slab s at slabs + s * slab_stride, panel layout [x][RP].
hipError_t launch_factor_product_f32(const FactorProductPlan& p, const float* A, long tile_stride, const float* F, int RP,
                                     float* slabs, long slab_stride, hipStream_t stream, const GramReduceArgs* rg = nullptr);

// Column-major (ld) -> x-tiled copy of an X x Y matrix into a ZERO-FILLED destination (untile: the reverse),
// and the x-tiled image of the TRANSPOSE of a column-major I x J matrix.
template <typename T>
hipError_t launch_tile(const T* src, long ld, int X, int Y, T* dst, long tile_stride, int th, bool untile, hipStream_t stream);
template <typename T>
hipError_t launch_tile_transposed(const T* src, long ld, int I, int J, T* dst, long tile_stride, int th, hipStream_t stream);

// Diagnostic build of the same kernel with in-kernel clock stamps (8 x uint64 per wave:
// shader clock at entry / first MFMA / loop end / kernel end, 100 MHz real time at entry / end, steps, XCC id).
hipError_t launch_factor_product_f32_stamped(const FactorProductPlan& p, const float* A, long lda, const float* F, int RP,
                                             float* slabs, long slab_stride, unsigned long long* stamps, hipStream_t stream);

// Rank-64 fp32 multiplicative-update fast path (kernels_mu64.hip).
// Partial Gram matrices of a panel, one per 64 panel columns ([len_pad/64][4096]), no reduction.
hipError_t launch_mu64_gram_partials(const float* P, int len_pad, float* partial, hipStream_t stream);
// Stand-alone form of the Gram reduction (used outside the iteration loop).
hipError_t launch_mu64_gram_reduce(const GramReduceArgs& rg, hipStream_t stream);
// Fused update (slab reduction, r x r product, element-wise update, error terms, partial Gram of the
// result).  is_w = 0: H panel, numerator scaled by `scale`; is_w = 1: Wt panel kept UNNORMALISED,
// old values scaled by `scale`; ps = tr(H^T W^T V) terms (H) / tr(H H^T W^T W) terms (W, needs Gprev).
hipError_t launch_mu64_update(int is_w, float* P, const float* slabs, int S, long slab_stride, const float* Q, const float* scale,
                              float eps, float* ps, int len_valid, int len_pad, float* gram_partial, const float* Gprev,
                              int compute_error, hipStream_t stream, void* x3_out = nullptr, int x3_ks = 0);
// The same update on 32-column tiles WITHOUT the partial Gram matrices (twice the workgroups, half the serial MFMA work per
// workgroup, no Gram in the critical path): for callers that take the Gram matrices from the split image (gram_image.h).
// x3_out is mandatory here.
// peers (optional): the summands are peers->count panels given by pointer (the exchange panels of a column-sharded run's ranks, in rank order; on this
// device or in a peer's memory) instead of S slabs slab_stride apart
constexpr int PEER_SLABS_MAX = 16;
struct PeerSlabs { const float* p[PEER_SLABS_MAX]; int count; };
// nsNMF's smoothing matrix S = (diag - off) I + off 1 1^T over the first r rank rows, applied AROUND the H update's r x r product (k_mu64_update32<.., NS>)
struct SmoothAround { float off, diag; int r; };
hipError_t launch_mu64_update32(int is_w, float* P, const float* slabs, int S, long slab_stride, const float* Q, const float* scale,
                                float eps, float* ps, int len_valid, int len_pad, const float* Gprev, int compute_error, hipStream_t stream,
                                void* x3_out, int x3_ks, const PeerSlabs* peers = nullptr, float* colsq_part = nullptr, int qsplit = 0, float* q_out = nullptr,
                                const SmoothAround* ns = nullptr);
// (ns, H update only: num = S D sum(slabs), den = S Q (S h), the split image written is that of S h_new -- the operand of nsNMF's V (S H)^T; the panel keeps h_new)
// (qsplit > 1, H update: Q holds qsplit unscaled partial matrices 4096 elements apart -- the K-split Gram passengers' output, GramReduceArgs::ksplit; every
//  workgroup adds them in order and scales the sum by `scale` on both sides, workgroup 0 also stores the finished matrix to q_out)
// (colsq_part, W update only: len_pad / 32 vectors of 64 partial sums of squares of the new rows, one per workgroup -- what the next Gram passengers turn into
//  the pending column scale, GramReduceArgs::colsq_part)
// out[i] = sum_k src.p[k][i] (rank order), count a multiple of 4: the r x r parts of the ranks' exchange buffers
hipError_t launch_sum_peers(const PeerSlabs& src, float* out, int count, hipStream_t stream);
// G (64 x 64) = P P^T from the split image of P (image_ks K-steps); normalize / scale as in GramReduceArgs.  Stand-alone form
// of the passenger workgroups of the split-operand product launch.
hipError_t launch_gram_from_image(const void* image, int image_ks, float* G, float* scale, int normalize, hipStream_t stream, const float* colsq_part = nullptr, int colsq_parts = 0);
hipError_t launch_gram_image_args(const GramReduceArgs& rg, hipStream_t stream);      // ... every field of rg as given, the K-split form included
// P(c, y) *= scale(c)
hipError_t launch_mu64_apply_scale(float* P, int len_pad, const float* scale, hipStream_t stream, void* x3_out = nullptr, int x3_ks = 0);
// G <- sum of `parts` partial 64 x 64 matrices; with scale != nullptr also scale(c) = 1 / sqrt(G(c, c)) (1 if 0) and
// G <- diag(scale) G diag(scale): the stand-alone (not passenger) form of the Gram reduction
hipError_t launch_gram64_from_partials(const float* partials, int parts, float* G, float* scale, hipStream_t stream);
hipError_t launch_gram64_normalize_all(const float* partials, int parts, float* Graw, float* G, float* scale, float* P, int len_pad, void* x3_out, int x3_ks, hipStream_t stream);
// the same in ONE launch: column scales from the update kernel's sums of squares (sq_parts vectors of 64) instead of the reduced diagonal; G = D (sum of the partial
// matrices) D; P <- P D and its split image
hipError_t launch_gram64_reduce_scale_all(const float* gram_part, int parts, const float* sumsq_part, int sq_parts, float* G, float* scale, float* P, int len_pad,
                                          void* x3_out, int x3_ks, hipStream_t stream);

// Generic (VALU) form, writes the finished panel (no slabs).  Xpad multiple of 64, RP multiple of 32.
template <typename T>
hipError_t launch_factor_product_valu(const T* A, long lda, int Xpad, int Y, const T* F, int RP, T* out, hipStream_t stream);

template <typename T>
hipError_t launch_reduce_slabs(const T* slabs, int S, long slab_stride, T* out, long count, hipStream_t stream);

// G = P P^T over len panel columns; partial holds parts * RP * RP elements of scratch.
template <typename T>
hipError_t launch_gram(const T* P, int RP, int len, int parts, T* partial, T* G, hipStream_t stream);

enum PanelMode { PANEL_MU = 0, PANEL_LS = 1, PANEL_SET = 2 };
// Extras of the multiplicative update at padded rank 256 with bf16 product operands (config 4, kernels_tri.hip).  W is carried unnormalised with a
// pending column scale D (as the rank-64 path does), and its bf16 fragments hold the unnormalised, unsmoothed values: scale and nsNMF smoothing move to
// the OUTPUT side of the product, (W D S)^T V = S D (W^T V) -- O(r n) work inside the H update instead of a pass over the panel.
struct PanelTriExtras {
	// A pending column scale is handed over as the staged sums of squares the update left behind (launch_colsq_stage: `parts` vectors of RP, added in
	// order): d(c) = sum > 0 ? 1 / sqrt(sum) : 1 -- kernel::normalizeColumns (KernelNormalizeColumns.cu:37-58) as a factor.  Every consumer forms d the
	// same way (tri_pending_scale() below), so they all see the same bits.  nullptr: ones.
	// numerator transform, per panel row y:  num'(y, c) = a * d(c) num(y, c) + b * sum_{c'} d(c') num(y, c'),  c < r  (zero beyond); d from num_colsq.
	bool num_transform = false;
	const float* num_colsq = nullptr;
	int num_colsq_parts = 0;
	float num_a = 1.0f, num_b = 0.0f;
	int r = 0;
	// denominator with the smoothing (and a pending scale) applied around the r x r product instead of inside its operand (32-row kernel):
	//   den(y, :) = S D G D S old(y, :),  S = den_a I + den_b 1 1^T on the first r columns, D = diag(d) from den_colsq (nullptr: ones), G = the split image given
	// -- the Gram matrix arrives as the reduction left it (unnormalised, unsmoothed) and no O(r^2) pass over it is launched
	bool den_transform = false;
	float den_a = 1.0f, den_b = 0.0f;
	const float* den_colsq = nullptr;
	int den_colsq_parts = 0;
	// the panel's own pending column scale: every old value is read as old(y, c) * d(c), d from old_colsq
	const float* old_colsq = nullptr;
	int old_colsq_parts = 0;
	// the old rows enter the r x r product rounded to bf16 (three MFMAs per tile instead of six, no operand split; Q keeps its three planes); the
	// element-wise step keeps the fp32 values.  Measured at rank 256 / nsNMF (tools/tri_accuracy.py): the bf16 mode's distance from the fp64 oracle does
	// not move (W 3.4e-4 vs 3.2e-4 after 10 iterations, 1.17e-3 vs 1.16e-3 after 40): it is set by the rounding of V and the factors in the big products
	bool old_as_bf16 = false;
	// bf16 fragments of the NEW rows (layout of k_finish_panel_bf16), K-steps >= frag_KS are not written; the 32-row kernel can smooth them on the way
	// (f(y, c) = frag_a x(y, c) + frag_b sum_c' x(y, c'), c < r; needs r), the 128-row kernel writes them as they are (frag_a = 1, frag_b = 0)
	void* frag_out = nullptr;
	long frag_KS = 0;
	float frag_a = 1.0f, frag_b = 0.0f;
};
int panel_update_rows(int RP, size_t elem);
// number of per-workgroup sum-of-squares partials launch_panel_update writes for a panel of len_pad columns
int panel_update_parts(int RP, size_t elem, int len_pad);

// fp32 / padded rank 64 specialisations (kernels_fast.hip); the generic launchers dispatch to them
hipError_t launch_gram64_f32(const float* P, int len, int parts, float* partial, float* G, hipStream_t stream);
hipError_t launch_panel_update64_f32(int mode, float* P, const float* slabs, int S, long slab_stride, const float* Q, int len_pad,
                                     float eps, float* ps, int len_valid, float* sumsq_part, float* num_out, hipStream_t stream);
// fp32 / padded rank 64, LDS-staged (kernels_wide.hip): 64 panel rows per workgroup
// gram_partial (optional): len_pad / 64 partial 64 x 64 Gram matrices of the new rows (layout of k_mu64_update)
hipError_t launch_panel_update64_lds_f32(int mode, float* P, const float* slabs, int S, long slab_stride, const float* Q, int len_pad,
                                         float eps, float* ps, int len_valid, float* sumsq_part, float* num_out, hipStream_t stream,
                                         float* gram_partial = nullptr, void* x3_out = nullptr, int x3_ks = 0);
// true when launch_panel_update<float> at padded rank 64 can deliver those partial Gram matrices
bool panel_update_delivers_gram(int RP, size_t elem);
// fp32 / padded rank 128 ... 512 (kernels_wide.hip)
bool panel_update_wide_available(int RP);
// long panels at padded rank 128 / 256 (kernels_wide.hip, k_panel_update_wide64_mu): multiplicative update with the r x r operand given as
// its split image; the result may go to another panel (P_out != P_in), e.g. to keep the unnormalised W readable while it is normalised
bool panel_update_long_available(int RP, int len_pad);
hipError_t launch_panel_update_long_mu(const float* P_in, float* P_out, const float* slabs, int S, long slab_stride, const void* q_split, int RP, int len_pad,
                                       float eps, float* ps, int len_valid, float* sumsq_part, hipStream_t stream, const PanelTriExtras* tri = nullptr);
bool gram_wide_available(int RP);
// the slice count launch_gram_wide_f32 settles on (at most `parts`)
int gram_wide_parts(int RP, int len, int parts);
// len: valid panel rows (the padding rows behind them are zero); partial: parts * RP * RP elements
hipError_t launch_gram_wide_f32(const float* P, int RP, int len, int parts, float* partial, float* G, hipStream_t stream);
// q_split (optional): 3 * 16 * (RP / 16 + 1) * (RP / 32) * 64 bytes of scratch; when given, the r x r product runs on the bf16
// matrix pipe with exactly split operands (fp32 accuracy, kernels_x3.hip) instead of the fp32 MFMA instructions
// Extras of the fused fp32 iteration at padded ranks 128 ... 512 (Engine::iterate_fused32w; the float counterpart of PanelFusedF64)
struct PanelFusedF32 {
	const float* old_scale = nullptr;   // W update: every old value is read as old(y, c) * old_scale[c]
	int h_side = 0;                     // H update with W = Wt D (S): Q is the RAW Gram matrix of the panel Wt, and
	const float* scale = nullptr;       //   d (nullptr: ones):  num <- S D num,  den = S D Q D S old
	int smooth = 0;                     //   0: S = I
	float off = 0.f, diag = 1.f;
	int r = 0;
	float* smooth_out = nullptr;        // H update with smoothing: a second panel that receives S new(y, :)
	void* x3_out = nullptr;             // the split image (k_pack_panel_x3's layout) of what the next product multiplies with: S new where there is smoothing, else new
	long x3_ks = 0;                     // ... K-steps >= x3_ks are not written
};
hipError_t launch_panel_update_wide_f32(int mode, float* P, const float* slabs, int S, long slab_stride, const float* Q, int RP, int len_pad,
                                        float eps, float* ps, int len_valid, float* sumsq_part, float* num_out, hipStream_t stream,
                                        void* q_split = nullptr, const PanelTriExtras* tri = nullptr, const PanelFusedF32* fused = nullptr);
// G = P P^T, its split image (the update kernel's operand: launch_panel_update_wide_f32 with Q == nullptr) and, W side, the pending column scale -- two launches
// the second half of launch_gram_wide_fused_f32 on its own: the slices came from passenger workgroups of a product launch (GramReduceArgs::wide_P)
hipError_t launch_gram_reduce_x3(const float* partial, int parts, int RP, float* G, void* qx3, const float* sumsq_part, int sq_parts, float* scale_out, hipStream_t stream);
// the slice count launch_gram_wide_fused_f32 settles on (at most `parts`)
int gram_wide_fused_parts(int RP, int len, int parts);
hipError_t launch_gram_wide_fused_f32(const float* P, int RP, int len, int parts, float* partial, float* G, void* qx3, const float* sumsq_part, int sq_parts,
                                      float* scale_out, hipStream_t stream);
template <typename T>
hipError_t launch_reduce_partials(const T* partial, int parts, long stride, T* out, long count, hipStream_t stream);
template <typename T>
hipError_t launch_normalize_panel_v2(T* P, int RP, int len_pad, T* sumsq_part, int parts, hipStream_t stream);

// See k_panel_update.  sumsq_part needs (len_pad / panel_update_rows) * RP elements.
template <typename T>
hipError_t launch_panel_update(int mode, T* P, const T* slabs, int S, long slab_stride, const T* Q, int RP, int len_pad,
                               T eps, T* ps, int len_valid, T* sumsq_part, T* num_out, hipStream_t stream, T* gram_partial = nullptr,
                               void* x3_out = nullptr, int x3_ks = 0,    // x3_out: split image of the new panel (kernels_x3.hip); only where panel_update_delivers_gram()
                               void* q_split = nullptr,                  // scratch for the split image of Q (wide fp32 panels, see launch_panel_update_wide_f32)
                               const PanelTriExtras* tri = nullptr);     // fp32, padded rank 256 only

// HALS (kernels_hals.hip): Gauss-Seidel sweep over the r coordinates of every panel column, P(:, y) <- the clamped coordinate-descent update
// against G (r x r Gram matrix) and the summed slabs; ps / sumsq_part (optional) as launch_panel_update's, with panel_sweep_hals_parts() partials.
// Padded ranks: fp32 64, 128, 256, 384, 512; fp64 multiples of 64 up to 512.
// l1, l2 >= 0: penalties on the swept factor (the step divides by G(k, k) + l2 and its gradient carries l2 p(k) + l1; ps keeps the raw slabs).  Both 0: the
// plain sweep, the same instantiation as before the penalties existed.
bool panel_sweep_hals_available(int RP, size_t elem);
int panel_sweep_hals_parts(int RP, size_t elem, int len_pad);
template <typename T>
hipError_t launch_panel_sweep_hals(T* P, const T* slabs, int S, long slab_stride, const T* G, int RP, int r, int len_pad, int len_valid, T* ps, T* sumsq_part,
                                   hipStream_t stream, T l1 = T(0), T l2 = T(0));
// Accelerated HALS (kernels_hals_multi.hip; docs/HALS.md, "Inner sweeps"): `sweeps` sweeps in a row against the same G and slabs, each from the result of the one
// before, in one launch; ps and sumsq_part from the final state.  sweeps outside HALS_SWEEPS_MIN ... HALS_SWEEPS_MAX: hipErrorInvalidValue; sweeps == 1 is
// launch_panel_sweep_hals, the same kernel as before the counts existed.
constexpr int HALS_SWEEPS_MIN = 1, HALS_SWEEPS_MAX = 64;
template <typename T>
hipError_t launch_panel_sweeps_hals(T* P, const T* slabs, int S, long slab_stride, const T* G, int RP, int r, int len_pad, int len_valid, T* ps, T* sumsq_part,
                                    hipStream_t stream, T l1, T l2, int sweeps);
// ... with per-column dynamic stopping (kernels_hals_dyn.hip; docs/HALS.md, "Dynamic stopping"): `sweeps` is the maximum; a column is frozen after sweep t when
// d_t <= tol^2 d_1, d_t the squared step of sweep t, and never stepped again.  counts (optional, len_pad ints): sweeps applied per column, 0 on padding.
// Always the dynamic kernel, one sweep included; tol outside (0, 1), NaN included: hipErrorInvalidValue, beside what launch_panel_sweeps_hals refuses.
template <typename T>
hipError_t launch_panel_sweeps_hals_dyn(T* P, const T* slabs, int S, long slab_stride, const T* G, int RP, int r, int len_pad, int len_valid, T* ps, T* sumsq_part,
                                        hipStream_t stream, T l1, T l2, int sweeps, double tol, int* counts);
// NeNMF (kernels_nenmf.hip; docs/NENMF.md): `steps` Nesterov-accelerated projected-gradient steps of the panel against G and the summed slabs in one launch, on the
// arrays of launch_panel_sweeps_hals and with its outputs (ps and sumsq_part from the final projected iterate, panel_steps_apg_parts() partials).  The step length
// is 1 / L, L = max row sum of G + l2, computed inside the launch; L <= 0 or not finite: the panel keeps its values.  Padded ranks 64 and 128 in both precisions;
// steps outside APG_STEPS_MIN ... APG_STEPS_MAX, another rank, a negative or non-finite penalty: hipErrorInvalidValue.
constexpr int APG_STEPS_MIN = 1, APG_STEPS_MAX = 256, APG_STEPS_DEFAULT = 8;
bool panel_steps_apg_available(int RP, size_t elem);
int panel_steps_apg_parts(int RP, size_t elem, int len_pad);
// c[t] = (alpha_t - 1) / alpha_{t+1}, alpha_0 = 1, alpha_{t+1} = (1 + sqrt(4 alpha_t^2 + 1)) / 2, t < steps: the extrapolation behind step t, in double
void apg_momentum(int steps, double* out);
template <typename T>
hipError_t launch_panel_steps_apg(T* P, const T* slabs, int S, long slab_stride, const T* G, int RP, int r, int len_pad, int len_valid, T* ps, T* sumsq_part,
                                  hipStream_t stream, T l1, T l2, int steps);
// ... with per-column dynamic stopping (kernels_nenmf_dyn.hip; docs/NENMF.md, "Dynamic stopping"): `steps` is the maximum; a column is frozen after step t when
// d_t <= tol^2 d_0, d_t = |P_{t+1} - Y_t|^2 of that column, keeps P_{t+1} and is never stepped again.  counts (optional, len_pad ints): steps applied per column,
// 0 on padding and where L admits no step.  Always the dynamic kernel, one step included; tol outside (0, 1), NaN included: hipErrorInvalidValue, beside what
// launch_panel_steps_apg refuses.
template <typename T>
hipError_t launch_panel_steps_apg_dyn(T* P, const T* slabs, int S, long slab_stride, const T* G, int RP, int r, int len_pad, int len_valid, T* ps, T* sumsq_part,
                                      hipStream_t stream, T l1, T l2, int steps, T tol, int* counts);
// W(:, c) <- W(:, c) / d(c), H(c, :) <- H(c, :) d(c) where d(c) = ||W(:, c)|| > 0, d from `parts` vectors of partial sums of squares (W H unchanged);
// sumsq_part needs RP elements of scratch behind the partials
template <typename T>
hipError_t launch_hals_normalize(T* Wt, int RP, int mpad, T* H, int npad, T* sumsq_part, int parts, hipStream_t stream);

// sumsq_part: parts * RP partial sums followed by 16 * RP elements of scratch
template <typename T>
hipError_t launch_normalize_panel(T* P, int RP, int len_pad, T* sumsq_part, int parts, hipStream_t stream);

template <typename T>
hipError_t launch_smooth_panel(const T* P, T* out, int RP, int r, long len_pad, T offdiag, T diag, hipStream_t stream);

template <typename T>
hipError_t launch_trace_small(const T* A, const T* B, int RP, int r, T* ps, hipStream_t stream, const T* b_colsq = nullptr, const T* b_scale = nullptr);

template <typename T>
hipError_t launch_row_dot(const T* A, const T* B, int RP, int r, long len, T* ps, hipStream_t stream, T* part = nullptr);      // part: ROW_DOT_GROUPS * RP scratch -> coalesced form
constexpr int ROW_DOT_GROUPS = 128;

template <typename T>
hipError_t launch_fill_small(T* A, int RP, int r, int reuse, T offdiag, T diag, hipStream_t stream);
// dst (device-visible host memory or device memory) <- src, count elements, by a small kernel on `stream`
template <typename T>
hipError_t launch_copy_small(T* dst, const T* src, long count, hipStream_t stream);
template <typename T>
hipError_t launch_copy_two(T* dst, const T* a, long na, const T* b, long nb, hipStream_t stream);      // dst = [a | b]

// Ainv = (A + regulariser)^-1, regulariser = offdiag everywhere, diag on the diagonal.  work: 2 * r * r doubles
// (r > 64 only; that route also adds the regulariser to A in place).
template <typename T>
hipError_t launch_inverse_small(T* A, int RP, int r, T* Ainv, double* work, T offdiag, T diag, hipStream_t stream);
// ... its r > 64 half (Householder QR through `work`) at any r: what the kernel tests run below 65 as well
template <typename T>
hipError_t launch_inverse_householder(T* A, int RP, int r, T* Ainv, double* work, T offdiag, T diag, hipStream_t stream);

template <typename T>
hipError_t launch_transpose(const T* src, long lds, int rows, int cols, T* dst, long ldd, hipStream_t stream);

// range_flag (optional, fp32): bit 0 is set when V holds a value outside what the split-operand product (kernels_x3.hip) is
// exact for -- not finite, |v| > 2^126 (the first bf16 cut would round to infinity) or 0 < |v| < 2^-100 (the third term would
// fall into the flushed bf16 subnormals)
template <typename T>
hipError_t launch_column_sumsq(const T* V, long ldv, int rows, int cols, T* ps, hipStream_t stream, int* range_flag = nullptr);

// ---- device-resident input and output (kernels_import.hip, docs/DEVICE_IO.md) ----
// layout: 0 column-major (ld >= rows), 1 row-major (ld >= cols); src is DEVICE memory, read only.  The bits OR-ed into *flags (an integer atomic: independent of order):
enum { IMPORT_BAD_VALUE = 1, IMPORT_BAD_WEIGHT = 2, IMPORT_SOME_WEIGHT = 4 };
// src (rows x cols) -> the column-major image dst (ld ldd >= rows_pad; rows_pad, cols_pad multiples of 64), written over the whole rows_pad x cols_pad: 0 beyond
// rows x cols.  rule: 0 none (flags may be null), 1 every entry finite and >= 0, 2 finite and > 0; a violation sets IMPORT_BAD_VALUE.
template <typename T>
hipError_t launch_import_dense(const T* src, long ld, int layout, int rows, int cols, T* dst, long ldd, long rows_pad, long cols_pad, int rule, int* flags, hipStream_t stream);
// The joint rule of the weighted upload: IMPORT_BAD_WEIGHT for a weight that is not finite or < 0, IMPORT_BAD_VALUE for an entry of V that is not finite, < 0 (or,
// with positive_rule, = 0) under a weight > 0, IMPORT_SOME_WEIGHT when a weight is > 0.  Vdst holds 0 wherever the weight is 0; Odst the weights.  wsum_part:
// import_weighted_parts(rows_pad, cols_pad) doubles, one partial sum of the weights per workgroup (the caller adds them in index order).
template <typename T>
hipError_t launch_import_weighted(const T* V, long ldv, int layoutV, const T* Omega, long ldo, int layoutO, int rows, int cols, T* Vdst, T* Odst, long ldd, long rows_pad,
                                  long cols_pad, int positive_rule, int* flags, double* wsum_part, hipStream_t stream);
long import_weighted_parts(long rows_pad, long cols_pad);
// A caller's factor, W (len x r; is_w) or H (r x len), to or from the panel [len_pad][RP].  Import writes the whole panel (exact zeros at coordinates >= r and entries
// >= len); export writes the len x r / r x len block only, never the gap of ld.
template <typename T>
hipError_t launch_import_panel(const T* src, long ld, int layout, bool is_w, int r, int len, T* panel, int RP, long len_pad, hipStream_t stream);
template <typename T>
hipError_t launch_export_panel(const T* panel, int RP, long len_pad, bool is_w, int r, int len, T* dst, long ld, int layout, hipStream_t stream);

// ---- device-resident input of the sparse engines (kernels_compact.hip, docs/DEVICE_IO.md) ----
// A dense src (rows x cols, layout and ld as above, DEVICE memory, read only) compacted into the CSR and CSC images of its stored entries -- masked: every entry that
// is not NaN (an infinite one sets IMPORT_BAD_VALUE in *flags), otherwise every entry != 0.  Count: rowcnt[i][tile column] (compact_row_counts ints) and
// colcnt[j][tile row] (compact_col_counts ints), tiles of 64 x 64, every count written once; *total (zeroed by the caller) += the number of stored entries.
long compact_row_counts(int rows, int cols);
long compact_col_counts(int rows, int cols);
template <typename T>
hipError_t launch_compact_count(const T* src, long ld, int layout, int rows, int cols, int masked, int* rowcnt, int* colcnt, int* flags, unsigned long long* total, hipStream_t stream);
// off_r / off_c: the exclusive scans of rowcnt / colcnt with the total behind the last element (launch_sp_scan).  csr_ptr[i] = off_r[i][0], csr_ptr[rows] = the total ...
hipError_t launch_compact_pointers(const int* off_r, const int* off_c, int rows, int cols, int* csr_ptr, int* csc_ptr, hipStream_t stream);
// ... and the entries: CSR rows ascending in their columns, CSC columns ascending in their rows; from_csr (or null): the CSR position of every CSC entry.  nnz: the
// total of the count; no position outside [0, nnz) is written.
template <typename T>
hipError_t launch_compact_scatter(const T* src, long ld, int layout, int rows, int cols, int masked, const int* off_r, const int* off_c, long nnz, int* csr_idx, T* csr_val,
                                  int* csc_idx, T* csc_val, int* from_csr, hipStream_t stream);
// The value rules of a sparse upload over values[0 .. nnz) in DEVICE memory: rule 1 every value finite and >= 0, rule 2 finite, rule 3 finite and > 0; a violation sets IMPORT_BAD_VALUE.
template <typename T>
hipError_t launch_sparse_value_rule(const T* values, long nnz, int rule, int* flags, hipStream_t stream);

// format: 1 CSR (ptr = rowPtr, idx = column indices), 2 CSC (ptr = columnPtr, idx = row indices),
// 3 COO (idx = row indices, idx2 = column indices); outer = rows (CSR) / columns (CSC).
template <typename T>
hipError_t launch_densify(int format, const T* values, const int* ptr, const int* idx, const int* idx2, long nnz, int outer, int base,
                          T* V, long ldv, int rows, int cols, hipStream_t stream);

// element (c, y) = draw number (y + y_first) * r + c of the counter-based stream (y_first: a column shard's first global column)
template <typename T>
hipError_t launch_fill_uniform(T* P, int RP, int r, long len, long len_pad, uint64_t seed, hipStream_t stream, long y_first = 0);

// ---- fp64 MFMA factor product (kernels_f64.hip): same x-tiled image of A (tile height 128), K-steps of four y ----
FactorProductPlan plan_factor_product_f64(int X, int Y, int RP, int num_cus);
// Passengers of the fp64 product launch (kernels_f64.hip, gram_ride_f64): the Gram matrix of a factor panel as it lies, K-sliced, reduced by the last arriver of every
// 64 x 64 super-block; and (W side) the pending column scale from the W update's sums of squares
struct GramRideF64 {
	const double* P;            // the panel (RP columns); nullptr: no passengers
	int len;                    // its valid rows (rows behind them up to the padded length are zero)
	int slices;                 // K slices per super-block
	double* partial;            // [slices][super-blocks][4096] scratch
	unsigned* counters;         // [super-blocks], zero between launches
	double* G;                  // the reduced matrix, both triangles
	const double* sumsq_part;   // the pending column scale's source: sumsq_parts vectors of RP partial sums of squares (nullptr: no scale passengers)
	int sumsq_parts;
	double* scale_out;          // [RP] d(c) = sum > 0 ? 1 / sqrt(sum) : 1
	const int* items;           // [super-blocks * slices] which (super-block, slice) passenger pid takes (gram_ride_f64_items; nullptr: pid order)
	int stop;                   // measurement builds (NMFAMD_RIDE64_STOP): 1 = passengers return at once, 2 = after their partial block, 3 = after counting in (results void)
	unsigned long long* stamps; // measurement builds: [4096][8] wall-clock stamps (product workgroups from 0, passengers from 2048), tools/stamp_f64.py
};
int gram_ride_f64_workgroups(int RP, int slices);
hipError_t launch_factor_product_f64(const FactorProductPlan& p, const double* A, long tile_stride, const double* F, int RP,
                                     double* slabs, long slab_stride, hipStream_t stream, const GramRideF64* ride = nullptr);
void gram_ride_f64_items(const FactorProductPlan& p, int RP, int slices, std::vector<int>& items);

// Extras of the fused double-precision iteration (Engine::iterate_fused64): W stays unnormalised in its panel with a pending column scale d (a vector the scale
// passengers of the W^T V launch leave), and nsNMF's smoothing S = (diag - off) I + off 1 1^T (first r entries) is applied where a row of the panel sits in LDS anyway
struct PanelFusedF64 {
	const double* old_scale;    // W update: every old value is read as old(y, c) * old_scale[c]
	int h_side;                 // H update with W = Wt D (S): Q is the RAW Gram matrix of the panel Wt, and
	const double* scale;        //   d (nullptr: ones):  num <- S D num  ((Wt D S)^T V = S D (Wt^T V)),  den = S D Q D S old  (D and S applied around the MFMA product)
	int smooth;                 //   0: S = I
	double off, diag;
	int r;
	double* smooth_out;         // H update: a second panel that receives S new(y, :) (the operand of V (S H)^T and of its Gram matrix)
	// W update on error iterations: ceil(trace_r / 4) extra workgroups behind the panel's compute the r terms of tr(H H^T W^T W) (k_trace_small's arithmetic:
	// trace_out[d] = sum_i A(i, d) B(d, i) f(d) f(i), f = trace_scale or ones) -- the launch of its own and the boundary around it are gone
	const double* trace_a;
	const double* trace_b;
	const double* trace_scale;
	double* trace_out;
	int trace_r;
	unsigned long long* stamps; // measurement builds: [workgroups][8] wall-clock stamps (wide kernel)
};
inline int panel_fused_f64_extra_workgroups(const PanelFusedF64* fx) { return (fx != nullptr && fx->trace_out != nullptr) ? (fx->trace_r + 3) / 4 : 0; }
// fp64 / padded rank 64 panel update on the fp64 MFMA pipe (32 panel rows per workgroup: len_pad / 32 norm partials)
hipError_t launch_panel_update64_f64(int mode, double* P, const double* slabs, int S, long slab_stride, const double* Q, int len_pad,
                                     double eps, double* ps, int len_valid, double* sumsq_part, double* num_out, hipStream_t stream, const PanelFusedF64* fused = nullptr);

// fp64 Gram matrix on the MFMA pipe (padded rank 64 or k * 128)
hipError_t launch_gram_f64(const double* P, int RP, int len, int parts, double* partial, double* G, hipStream_t stream);
// fp64 / padded rank 128 ... 512: 16 panel rows per workgroup
bool panel_update_wide_f64_available(int RP);
hipError_t launch_panel_update_wide_f64(int mode, double* P, const double* slabs, int S, long slab_stride, const double* Q, int RP, int len_pad,
                                        double eps, double* ps, int len_valid, double* sumsq_part, double* num_out, hipStream_t stream, const PanelFusedF64* fused = nullptr);

// ---- bf16-operand factor product (kernels_bf16.hip) ------------------------------------------
// Fragment-ordered bf16 images: streamed matrix (x-tiled by 128, KS = ceil(Y / 16) K-steps) and the factor
// panel [y][RP] (RP = 64 or a multiple of 128; 16 * KS * RP / 32 * 64 bytes).
hipError_t launch_pack_stream_bf16(const float* src, long ld, int X, int Y, bool transposed, void* dst, int xtiles, int KS, hipStream_t stream);
hipError_t launch_pack_panel_bf16(const float* P, int RP, int len, void* dst, int KS, hipStream_t stream);

// kernels_tri.hip -- factor-side passes at padded rank 256 with bf16 product operands (config 4)
bool tri_kernels_available(int RP);
// rows [row0, row0 + rows) of the panel P (multiples of 32): optional column normalisation in place (colsq = colsq_parts vectors of RP partial sums of squares
// over ALL rows, added in order; or nullptr), nsNMF smoothing with (offdiag, diag) in registers, bf16 fragments of the smoothed rows into the pack `dst`
// (K-steps >= KS are not written)
hipError_t launch_finish_panel_bf16(float* P, int RP, int r, long row0, long rows, const float* colsq, int colsq_parts, float offdiag, float diag, void* dst, long KS, hipStream_t stream);
// the update kernel's per-workgroup sums of squares (`parts` vectors of RP) -> colsq_stage_parts() staged vectors (and, final_sum != nullptr, their sum)
int colsq_stage_parts();
hipError_t launch_colsq_stage(const float* part, int RP, int parts, float* staged, float* final_sum, hipStream_t stream);
// G (RP x RP, both triangles, exactly symmetric) = P^T P over `len` panel rows; partial: gram_tri_partial_elems(max_parts) floats
hipError_t launch_gram_tri(const float* P, int RP, int len, int max_parts, float* partial, float* G, int num_cus, hipStream_t stream);
long gram_tri_partial_elems(int max_parts);
// the same matrix from the panel's bf16 fragments (KS K-steps of 16 rows, layout of k_finish_panel_bf16 without smoothing): ONE bf16 MFMA per tile and
// K-step, i.e. G = P~^T P~ of the ROUNDED panel P~ -- exactly the operand the product against V multiplies with, so numerator and denominator of the
// H update refer to the same matrix.  colsq != nullptr: G(r, c) *= d(r) d(c), the pending column scale of the panel (PanelTriExtras).
hipError_t launch_gram_tri_bf16(const void* frags, int RP, long KS, int max_parts, float* partial, float* G, const float* colsq, int colsq_parts, int num_cus, hipStream_t stream);
// the same product, reduced WITHOUT any scaling into G and, in the same launch, into the split image x3_out that the update kernels take as their r x r operand
// (launch_panel_update with Q = nullptr; A(c, k) = G(k, c)); diag_out[c] = G(c, c) = the sum of squares of column c of the rounded panel -- the pending
// column scale of that panel in the form PanelTriExtras takes it (one "staged" vector)
hipError_t launch_gram_tri_bf16_image(const void* frags, int RP, long KS, int max_parts, float* partial, float* G, void* x3_out, float* diag_out, int num_cus, hipStream_t stream);
// P(y, c) *= d(c) over `rows` panel rows (folds a pending column scale, given as staged sums of squares, into the panel); scale_out (optional): the RP factors
hipError_t launch_scale_panel_tri(float* P, int RP, long rows, const float* colsq, int colsq_parts, float* scale_out, hipStream_t stream);
// Gs = S G S, S = (diag - offdiag) I + offdiag 1 1^T on the first r rows / columns
// x3_out (optional): also the split image of Gs that the wide update kernels take as their r x r operand (launch_panel_update with Q = nullptr);
// its closing all-zero K-step is the caller's (written once)
hipError_t launch_smooth_gram(const float* G, float* Gs, int RP, int r, float offdiag, float diag, void* x3_out, hipStream_t stream);
// the finishing pass over ALL rows of a panel and its Gram matrix in one launch (+ the reduction); colsq != nullptr: P_out (!= P_in) <- the
// column-normalised panel, G = the Gram matrix of the normalised panel
hipError_t launch_finish_and_gram(const float* P_in, float* P_out, int RP, int r, long rows, int len, const float* colsq, int colsq_parts, float offdiag, float diag,
                                  void* dst, long KS, int max_parts, float* partial, float* G, int num_cus, hipStream_t stream);
hipError_t launch_factor_product_bf16(const FactorProductPlan& p, const void* A, int KS, const void* F, int RP,
                                      float* slabs, long slab_stride, hipStream_t stream, const GramReduceArgs* rg = nullptr);
// K-split of the bf16 product for `xtiles` x-tiles and KS K-steps at padded rank RP
int plan_splits_bf16(int xtiles, int KS, int RP, int num_cus);
// workgroups the bf16 product launches for a plan at padded rank 256 (what is left of the chip can carry TRI_PASSENGERS)
int bf16_product_workgroups(const FactorProductPlan& p);
#ifdef NMFAMD_DIAG_BUILD
void set_factor_product_bf16_stamps(unsigned long long* stamps);      // measurement build: the calling thread's next rank-256 product launch stamps its waves' lives (tools/stamp_bf16.py)
#endif

// ---- fp32 product by exact 3 x bf16 operand splitting (kernels_x3.hip), padded rank 64 ------------
// The streamed matrix is the x-tiled fp32 image (tile height 128); the factor panel is split into
// three bf16 planes in fragment order, KS K-steps plus one all-zero step: 3 * 16 bytes * (KS + 1) * (RP / 32) * 64.
hipError_t launch_pack_panel_x3(const float* P, int RP, int len, void* dst, int KS, hipStream_t stream);
// stamps (measurement build): X3_STAMP_WORDS words per wave, the kernel's end says which (tools/stamp_x3.py)
constexpr int X3_STAMP_WORDS = 12;
hipError_t launch_factor_product_x3(const FactorProductPlan& p, const float* A, long tile_stride, const void* F, int RP,
                                    float* slabs, long slab_stride, hipStream_t stream, const GramReduceArgs* rg = nullptr,
                                    unsigned long long* stamps = nullptr, bool y_tiled = false, int image_tile = 128,
                                    hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
// (ev_start / ev_stop: the launch's own start and stop times go to these events -- hipExtLaunchKernel -- instead of the caller recording two events around it:
//  a bracketed launch costs the stream ~12 us of barrier packets, rocprofv3 trace of bench.py's sampled iterations)
int plan_splits_x3(int xtiles, int KS, int num_cus, int reserve = 0);

// ---- one pass over V per multiplicative-update iteration at padded rank 64 (kernels_onepass.hip) -----------------------
// The H update is column-separable once W^T W is known (reference: RN2 = RR H, RN = W^T V, multiplyDivide per element,
// source/nmf/AlgorithmMultiplicativeFrobenius.h:176-191; KernelMultiplyDivide.cu:29-43): a 32-column panel of V is loaded
// ONCE, W^T V of the panel is reduced over its rows, the panel's columns of H are updated, and (V H^T) is accumulated
// (:240-241) while the panel is still on chip.  One persistent launch of 256 workgroups (see the kernel).
struct OnePassArgs {
	const float* V; long tile_stride;     // the 16-row tiled image: V(i, j) at V[(i / 16) * tile_stride + j * 16 + i % 16]
	const void* Wx3;                      // split image of the (unnormalised) W panel, NBT = 2 (kernels_x3.hip)
	const float* G;                       // 64 x 64: diag(scale) Wu^T Wu diag(scale)
	const float* scale;                   // 64: pending column scale of W
	const float* H;                       // panel [npad][64]: the old H
	float* H_out;                         // the new H (another panel: the four owner waves of a column read the whole old column at their own pace)
	float* ps; long ps_stride;            // error iterations: four partial vectors (one per owner wave) of the per-column terms of tr(H^T W^T V)
	float* slabs; long slab_stride;       // 8 partial (V H^T)^T panels [mpad][64], one per XCD
	float* hh_part;                       // [256][4096] partial H H^T, one per workgroup
	void* part_scratch;                   // [8][ONEPASS_SLOTS][32][256] x 64 B tagged partial sums
	void* hfrag_scratch;                  // [8][ONEPASS_SLOTS][64][4][8] x 8 B tagged split values of the new H columns
	unsigned* ticket;                     // [8] per-XCD arrival counters (never reset: 32 per launch)
	unsigned* abort_flag;                 // set when a workgroup gave up waiting (or found its XCD over-subscribed)
	int tile_rows;                        // mpad / 16
	int w_ks;                             // K-steps of 16 rows in the split image of W; step w_ks is the all-zero step that closes it
	int n;                                // valid columns
	int panels;                           // ceil(n / 32)
	unsigned seq;                         // launch number of this engine (tickets and tags derive from it)
	int compute_error;
	float eps;
	unsigned long long* stamps = nullptr; // diagnostic builds: 16 words per wave (see the kernel's end)
};
constexpr int ONEPASS_SLOTS = 4;
constexpr int ONEPASS_GROUP = 32;         // workgroups per XCD
constexpr int ONEPASS_XCDS = 8;
constexpr int ONEPASS_TILES_PER_WAVE = 5; // 16-row tiles per wave: 320 rows per workgroup, 10 240 per XCD
constexpr size_t onepass_part_bytes() { return (size_t)ONEPASS_XCDS * ONEPASS_SLOTS * ONEPASS_GROUP * 256 * 64; }
constexpr size_t onepass_hfrag_bytes() { return (size_t)ONEPASS_XCDS * ONEPASS_SLOTS * 64 * 32 * 8; }
// true when the shape fits the kernel's fixed cut (rows per XCD group) on this device
bool onepass_available(long mpad, int num_cus);
hipError_t launch_mu64_onepass(const OnePassArgs& a, hipStream_t stream);

// ---- sparse-V compute path (kernels_sparse.hip) ----------------------------------------------
// out(row, :) = sum_p val[p] P(idx[p], :) over the stored entries of `row`; rows in [rows, rows_pad) are zeroed.
template <typename T>
hipError_t launch_spmm_rows(const int* ptr, const int* idx, const T* val, const T* P, int RP, T* out, int rows, int rows_pad, hipStream_t stream);
// q[p] = val[p] / (A(row,:).B(idx[p],:) + eps) and the per-row sums of val*wh and val*log(val/wh)
template <typename T>
hipError_t launch_sddmm_quotient(const int* ptr, const int* idx, const T* val, const T* A, const T* B, int RP, T eps,
                                 T* q, T* t_vwh, T* t_kl, int rows, hipStream_t stream);
// KL half-step in one pass: out(row, :) = sum_p val[p] / (A(row,:).B(idx[p],:) + eps) * B(idx[p], :) (quotient and numerator
// together, one gather per stored entry); rows in [rows, rows_pad) are zeroed; optional per-row error terms as above
template <typename T>
// blocks > 1: ptr is the blocked pointer array [rows][blocks + 1] (a row's entries cut at the block boundaries of the gathered index);
// out then receives `blocks` partial panels out_stride apart (and t_vwh / t_kl `blocks` partial vectors of rows_pad), grid block-major
hipError_t launch_kl_fused(const int* ptr, const int* idx, const T* val, const T* A, const T* B, int RP, T eps,
                           T* out, T* t_vwh, T* t_kl, int rows, int rows_pad, hipStream_t stream, int blocks = 1, long out_stride = 0,
                           const T* a_scale = nullptr);      // a_scale (RP factors, optional): A(row, :) is read as A(row, c) * a_scale[c] -- W's pending column scale
template <typename T>
hipError_t launch_permute(const T* src, const int* perm, T* dst, long count, hipStream_t stream);
// sums(c) = sum_y P(c, y); partial: (len_pad / 128) * RP elements of scratch
template <typename T>
hipError_t launch_panel_rowsum(const T* P, int RP, int len_pad, T* partial, T* sums, hipStream_t stream);
// P(c, y) <- P(c, y) num(c, y) / (den(c) + eps); sumsq_part (optional): (len_pad / 128) * RP partial sums of squares
template <typename T>
// num: `parts` partial numerator panels part_stride apart, added in order
hipError_t launch_kl_update(T* P, const T* num, const T* den, int RP, int len_pad, T eps, T* sumsq_part, hipStream_t stream, int parts = 1, long part_stride = 0,
                            T* sum_part = nullptr,       // sum_part (optional): (len_pad / 128) * RP partial sums of the new values
                            const T* scale = nullptr);   // scale (RP factors, optional): P(c, y) <- (P(c, y) scale[c]) num(c, y) / (den(c) + eps)
// sums(c) = sum of the len_pad / 128 vectors of sum_part, divided by sqrt(sum of sumsq_part) where sumsq_part is given and that is > 0 (the column sums of a panel
// AFTER its column normalisation, from what its update left behind); RP in {64, 128, 256}
template <typename T>
hipError_t launch_kl_sums(const T* sum_part, const T* sumsq_part, int parts, int RP, T* sums, hipStream_t stream, T* scale_out = nullptr);      // scale_out (optional): 1 / sqrt(sum of squares), 1 where that is 0

// ---- missing-value NMF: the multiplicative update over the stored entries only (kernels_masked.hip, docs/MISSING.md) ----------------------------------------
// One fused half-step: for every row < rows of A (RP in {64, 128, 256}), over its stored entries p (ptr / idx / val: the CSC image with A = H, B = Wt, or the CSR
// image with A = Wt, B = H), wh_p = A(row, :) . B(idx[p], :), and in place
//     A(row, :) <- A(row, :) .* (sum_p val[p] B(idx[p], :)) ./ (sum_p wh_p B(idx[p], :) + eps)           (update; false: the residual-only form)
// t_res (optional): t_res[row] = sum_p (val[p] - wh_p)^2 with the old row.  sumsq_part (optional, update only): masked_norm_parts(rows) partial RP vectors of the
// sums of squares of the new rows, for launch_normalize_panel (which needs NORM_GROUPS = 16 further RP vectors of scratch behind them).
constexpr int MASKED_NORM_PARTS = 2048;
int masked_norm_parts(int rows);
template <typename T>
hipError_t launch_masked_half_step(const int* ptr, const int* idx, const T* val, T* A, const T* B, int RP, T eps, bool update,
                                   T* t_res, T* sumsq_part, int rows, hipStream_t stream);
// ... under the beta-divergence (kernels_masked_beta.hip, docs/MISSING.md "Beta-divergence"): the same launch shape and order of sums with p = wh_p + eps mapped per
// entry, in place
//     A(row, :) <- A(row, :) .* (sum_p val[p] p^(beta - 2) B(idx[p], :) ./ (sum_p p^(beta - 1) B(idx[p], :) + eps + l1 + l2 A(row, :)))^gamma
// beta is taken in the precision of T (0: the Itakura-Saito map, 1: the KL map, else the general one); gamma as launch_beta_update.  t_frob / t_div (both or
// neither): t_frob[row] = sum_p (val[p] - p)^2 and t_div[row] = sum_p d_beta(val[p] | p) with the old row.  update = false: the terms only, A untouched.  sumsq_part
// as above.  hipErrorInvalidValue for another RP, a beta or penalty that is not finite, a negative penalty, and a launch with nothing to write.
template <typename T>
hipError_t launch_masked_beta_half_step(const int* ptr, const int* idx, const T* val, T* A, const T* B, int RP, T eps, double beta, T l1, T l2, bool update,
                                        T* t_frob, T* t_div, T* sumsq_part, int rows, hipStream_t stream);
// ... by coordinate descent (kernels_masked_cd.hip, docs/MISSING.md "Coordinate descent"): per row its own normal equations G_i = sum_p b_p b_p^T, c_i = sum_p val[p] b_p
// (b_p = B(idx[p], :) with the coordinates >= r selected to 0, p in stored order, on the matrix pipe), then `sweeps` penalised HALS sweeps (docs/HALS.md) of the old row
// in place; a row without an entry becomes 0, coordinates >= r come out 0.  G_out [rows][RP][RP] and c_out [rows][RP] (both or neither): the normal equations as formed.
// hipErrorInvalidValue for a padded rank other than 64 / 128, r outside 1 ... RP, sweeps outside 1 ... MASKED_CD_MAX_SWEEPS, a negative or non-finite penalty.
constexpr int MASKED_CD_MAX_SWEEPS = 64;
constexpr int MASKED_CD_MAX_GRID = 2048;        // the workgroups stride over the rows
constexpr bool masked_cd_rank_instantiated(int RP) { return RP == 64 || RP == 128; }
template <typename T>
hipError_t launch_masked_cd_half_step(const int* ptr, const int* idx, const T* val, T* A, const T* B, int RP, int r, int rows, int sweeps, T l1, T l2, T* G_out, T* c_out,
                                      hipStream_t stream);

// ---- predict and score entries of W H (kernels_predict.hip, docs/PREDICT.md) ---------------------------------------------------------------------------------
// Over a coordinate list rows / cols (nnz entries, index base 0 or 1, unsorted, duplicates counted per copy; DEVICE memory) and the padded panels Wt ([.][RP]) and
// H ([.][RP]): out[p] = sum_{k < r} Wt(rows[p], k) H(cols[p], k), coordinates k >= r selected out.  vals (or null: predictions only, out needed): the values v_p;
// then part[3 w + {0, 1, 2}] = workgroup w's sums, in double, of (v_p - out[p])^2, of d_beta(v_p | out[p] + eps) and of the absolute values of the summands of
// d_beta -- predict_entry_parts(nnz) workgroups, which the caller adds in workgroup order; out may be null.  beta is taken in the precision of T (0: the
// Itakura-Saito map, 1: the KL map, NaN: no divergence -- the two last sums are 0 --, else the general form).  The kernel checks NO index: launch_predict_validate
// comes first.  hipErrorInvalidValue for a padded rank without an instantiation (predict_rank_instantiated), nnz outside 1 ... PREDICT_MAX_ENTRIES, r outside
// 1 ... RP, another base, an infinite beta and a launch with nothing to write.
constexpr int PREDICT_PASS_ENTRIES = 32;        // entries of one workgroup pass: sixteen groups, two entries in flight each
constexpr int PREDICT_MAX_PARTS = 2048;         // the grid: min(ceil(nnz / PREDICT_PASS_ENTRIES), PREDICT_MAX_PARTS) workgroups that stride over the passes
constexpr long PREDICT_MAX_ENTRIES = 0x7fffffffl;
int predict_entry_parts(long nnz);
bool predict_rank_instantiated(int RP, size_t elem_bytes);      // fp32: 64, 128, 256, 384, 512; fp64: 64 ... 512 in steps of 64
template <typename T>
hipError_t launch_predict_entries(const int* rows, const int* cols, const T* vals, long nnz, int base, const T* Wt, const T* H, int RP, int r, T eps, double beta,
                                  T* out, double* part, hipStream_t stream);
// first_bad[0] <- min(first_bad[0], the smallest p whose coordinate lies outside [base, base + m) x [base, base + n)); first_bad[1] likewise for the smallest p
// whose value breaks `rule` (0: vals not read; 1 finite and >= 0, 2 finite, 3 finite and > 0).  The caller fills both words with 0xffffffff first.  Reads the
// arrays below nnz only.
template <typename T>
hipError_t launch_predict_validate(const int* rows, const int* cols, const T* vals, long nnz, int base, int m, int n, int rule, unsigned* first_bad, hipStream_t stream);

// ---- the k best candidates of W H per query: fused product and selection (kernels_topk.hip, docs/TOPK.md) -----------------------------------------------------
// queries (nq indices of base 0 or 1 into the rows of the query panel A [.][RP]) against the candidates 0 ... count - 1 (rows of the candidate panel B [.][RP]):
// s(q, j) = sum_{k < r} A(queries[q], k) B(j, k), coordinates k >= r selected to zero in both operands.  Per query the first k candidates by (score descending,
// index ascending) that its exclusion list (excl_ptr [nq + 1], 64-bit, and excl_idx, candidate indices of the same base; both null: none) does not name:
// out_idx [nq][k] (in the caller's base; -1 where fewer than k are eligible) and out_scores [nq][k] (-inf there).  slabs: slices of the candidate range that one
// workgroup each walks (0: topk_slabs(nq, count)); the result does not depend on it.  part_s / part_i: room for nq * slabs * k partial entries (slabs as given, or
// the plan's).  Everything in DEVICE memory.  The kernels check NO index: launch_topk_validate, or the host, comes first.  hipErrorInvalidValue for a padded rank
// outside predict_rank_instantiated's list, k outside 1 ... TOPK_MAX_K, r outside 1 ... RP, another base, slabs outside 0 ... TOPK_MAX_SLABS.
constexpr int TOPK_MAX_K = 64;
constexpr int TOPK_MAX_SLABS = 256;
constexpr int TOPK_SEGMENT_TILES = 32;           // tiles of a slab that share one clearing of the exclusion bitmap
constexpr int TOPK_TARGET_WORKGROUPS = 1024;     // topk_slabs: four workgroups per CU when the queries alone give fewer
constexpr int TOPK_LDS_LIMIT = 160 * 1024;
constexpr long TOPK_MAX_QUERIES = 1l << 30, TOPK_MAX_CANDIDATES = 1l << 30;
int topk_slabs(long nq, long count);
template <typename T>
int topk_waves(long nq, int RP, int k);          // waves (of 32 fp32 / 16 fp64 queries) per workgroup: the most, up to 4, whose LDS fits; 0: none fits
template <typename T>
hipError_t launch_topk(const int* queries, long nq, int k, int base, const T* A, const T* B, long count, int RP, int r, const long* excl_ptr, const int* excl_idx,
                       int slabs, T* part_s, int* part_i, int* out_idx, T* out_scores, hipStream_t stream);
// first_bad[0] <- the smallest q whose query lies outside [base, base + a_rows); first_bad[1] <- the smallest q in 0 ... nq at which excl_ptr breaks its rule
// (excl_ptr[0] = 0, non-decreasing, excl_ptr[nq] = excl_nnz); first_bad[2] <- the smallest e whose excl_idx[e] lies outside [base, base + count).  The caller fills
// the three words with 0xffffffff first.  Reads queries below nq, excl_ptr below nq + 1, excl_idx below excl_nnz only.
hipError_t launch_topk_validate(const int* queries, long nq, int base, long a_rows, long count, const long* excl_ptr, const int* excl_idx, long excl_nnz,
                                unsigned* first_bad, hipStream_t stream);

// ---- dense beta-divergence NMF: generalised KL (beta = 1), Itakura-Saito (beta = 0) and the general form (any other finite beta), with optional L1 / L2 penalties, on
// ---- a dense resident V (kernels_beta.hip, docs/DIVERGENCE.md) ---------------------------------------------------------------------------------------------------
// How one half-step is cut: workgroups of `bo` output columns, reduction tiles of `kt` rows, `slabs` slices of the reduction range (tiles_per_slab tiles each, the last
// one maybe fewer) that write one partial panel each.  A function of the shape, the element size and the CU count only: it fixes the order of the sums.
constexpr int BETA_MAX_SLABS = 16;
struct BetaPlan { int bo = 0, kt = 0, slabs = 0, tiles = 0, tiles_per_slab = 0; };
bool beta_half_step_available(int RP);      // padded ranks 64, 128, 256
BetaPlan plan_beta_half_step(long out_pad, long red_pad, int RP, size_t elem_bytes, int num_cus, int force_slabs = 0);
// The fused launch: A [out_pad][RP] (read only), B [red_pad][RP], X [out_pad][ldx] with X(o, k) the entry of V at output index o and reduction index k (zero on the
// padding), red_pad = plan.tiles * plan.kt <= ldx.  beta: any finite value, taken in the precision of T; 1 and 0 run their own element-wise maps, every other value the
// general one (P^(beta - 2) as exp2((beta - 2) log2 P)).  update: the slabs' partial numerators num_part (and, beta != 1, denominators den_part) at part_stride elements;
// terms: the slabs' parts of the per-output-row error terms sum_k (x - p)^2 (tf_part) and of the divergence (td_part) at t_stride elements.  Entries with o >= out_valid
// or k >= red_valid add nothing to any sum.
template <typename T>
hipError_t launch_beta_fused(const T* X, long ldx, const T* A, const T* B, int RP, double beta, bool update, bool terms, T eps, const BetaPlan& plan,
                             T* num_part, T* den_part, long part_stride, T* tf_part, T* td_part, long t_stride,
                             int out_pad, int out_valid, int red_valid, hipStream_t stream);
// The slabs in order, then A(o, c) <- A(o, c) (num / (den + eps + l1 + l2 A(o, c)))^gamma for o < out_valid, c < r and 0 elsewhere (beta = 1: den = dsum(c); otherwise
// den from den_part; gamma = 1 / (2 - beta) below beta = 1, 1 up to beta = 2, 1 / (beta - 1) above; l1, l2 >= 0, both 0: the unpenalised quotient); sumsq_part / sum_part (optional): [out_pad / 128][RP] sums of squares / sums of the new values; t_frob / t_div (optional, both or none):
// the error terms of out_pad rows, slabs in order.  update = false: the terms only, A untouched.  weighted: the half-step of launch_beta_fused_weighted -- den
// from den_part at every beta (dsum is not read).
template <typename T>
hipError_t launch_beta_update(T* A, const T* num_part, const T* den_part, long part_stride, int slabs, const T* dsum, int RP, int r, int out_pad, int out_valid, T eps,
                              double beta, T l1, T l2, bool update, T* sumsq_part, T* sum_part, const T* tf_part, const T* td_part, long t_stride, T* t_frob,
                              T* t_div, hipStream_t stream, bool weighted = false);
// The weighted fused launch (kernels_beta_weighted.hip): launch_beta_fused with a second image OX of the layout, leading dimension and padding of X that holds the
// per-entry weights (>= 0; zero on the padding).  An entry with weight 0 is not there, whatever X holds at it (NaN included); every other entry's contribution to
// num, den and the two error terms is scaled by its weight.  den_part is written at every beta (beta = 1: den(o, c) = sum_k w(k, o) B(k, c)).
template <typename T>
hipError_t launch_beta_fused_weighted(const T* X, const T* OX, long ldx, const T* A, const T* B, int RP, double beta, bool update, bool terms, T eps, const BetaPlan& plan,
                                      T* num_part, T* den_part, long part_stride, T* tf_part, T* td_part, long t_stride,
                                      int out_pad, int out_valid, int red_valid, hipStream_t stream);
// The mixed-precision fused launch (kernels_beta_bf16.hip; fp32 engines only): launch_beta_fused<float> -- the same arguments, the same plan, the same partial panels --
// with the operands of both products (A, B, and Q, R after the element-wise map) rounded to bf16, round to nearest even, on v_mfma_f32_32x32x16_bf16.  X, P + eps, the
// map, the error terms and every accumulation stay fp32; launch_beta_update<float> follows it unchanged.
hipError_t launch_beta_fused_bf16(const float* X, long ldx, const float* A, const float* B, int RP, double beta, bool update, bool terms, float eps, const BetaPlan& plan,
                                  float* num_part, float* den_part, long part_stride, float* tf_part, float* td_part, long t_stride,
                                  int out_pad, int out_valid, int red_valid, hipStream_t stream);
// The update launch of the minibatch update (kernels_beta_online.hip), on a grid of one workgroup per BETA_ROWS_PER_WG panel rows: the slabs in order, den = (their
// den_part, or dsum(c) at beta = 1) + eps + l1 + l2 P(o, c), then for o < out_valid, c < r
//     online = false:  P(o, c) <- P(o, c) (num / den)^gamma                                        (launch_beta_update's update; Aacc, Bacc and rho are not looked at)
//     online = true:   Aacc <- rho Aacc + P^(1 / gamma) num,  Bacc <- rho Bacc + den,  P <- (Aacc / Bacc)^gamma        (0 <= rho <= 1; Aacc, Bacc: [out_pad][RP])
// flush: new values below eps become 0.  P is 0 on the padding afterwards; Aacc and Bacc are not touched there.  sum_part (optional): [out_pad / BETA_ROWS_PER_WG][RP]
// sums of the new values, what launch_kl_sums takes with parts = out_pad / BETA_ROWS_PER_WG.  part_stride >= out_pad * RP.
constexpr int BETA_ROWS_PER_WG = 16;
template <typename T>
hipError_t launch_beta_update_rows(T* P, T* Aacc, T* Bacc, const T* num_part, const T* den_part, long part_stride, int slabs, const T* dsum, int RP, int r, int out_pad,
                                   int out_valid, T eps, double beta, T l1, T l2, bool online, T rho, bool flush, T* sum_part, hipStream_t stream);
// Aacc <- P, Bacc <- 1 on `count` elements: the accumulators of a minibatch engine whenever its factors are set
template <typename T>
hipError_t launch_beta_online_reset(const T* P, T* Aacc, T* Bacc, long count, hipStream_t stream);

// ---- the CSR and CSC images of a sparse V built on the device (kernels_sparse_setup.hip) ----------------------------------------
// flags (one int, zeroed by the caller): bit 0 = an entry outside the matrix or outside every pointer range, bit 1 = pointer array not ascending, bit 2 = the
// entries are not in (row, column) order.  format: 1 CSR (a = rowPtr, outer = rows), 2 CSC (a = columnPtr, outer = columns), 3 COO (a = rows, b = columns)
hipError_t launch_sp_expand(int format, const int* a, const int* b, long nnz, int outer, int base, int m, int n, int* row, int* col, int* flags, hipStream_t stream);
// ptr[0 .. segments] = exclusive scan of the histogram of key[0 .. count) (counts: `segments` ints of scratch), maxlen[0] = the longest segment
hipError_t launch_sp_histogram_scan(const int* key, long count, int segments, int* counts, int* ptr, int* maxlen, hipStream_t stream);
// the scan alone, over counts somebody else wrote (kernels_compact.hip): ptr[0 .. count] = exclusive scan of counts[0 .. count), maxlen[0] = the largest count;
// ptr and counts are different arrays
hipError_t launch_sp_scan(const int* counts, int count, int* ptr, int* maxlen, hipStream_t stream);
long sp_segment_sort_capacity();
// items <- the positions 0 .. count - 1 grouped by key (segment s at [ptr[s], ptr[s + 1])), every segment ascending by (minor[item], item) -- by item alone
// when minor == nullptr.  fill: `segments` ints of scratch; maxlen: the longest segment (<= sp_segment_sort_capacity())
hipError_t launch_sp_scatter_sort(const int* key, long count, int segments, const int* ptr, int* fill, int* items, const int* minor, int maxlen, hipStream_t stream);
template <typename T>
hipError_t launch_sp_gather_csr(const int* order, const int* row, const int* col, const T* val, long nnz, int* csr_idx, T* csr_val, int* rowq, hipStream_t stream);
template <typename T>
hipError_t launch_sp_gather_csc(const int* cq, const int* rowq, const T* csr_val, long nnz, int* csc_idx, T* csc_val, hipStream_t stream);
template <typename T>
hipError_t launch_sp_col_sumsq(const int* csc_ptr, const T* csc_val, int n, T* vtv, double* colsum, hipStream_t stream);
hipError_t launch_sp_boundaries(const int* ptr, const int* idx, int rows, long range, int blocks, int* bp, hipStream_t stream);

} // namespace nmfamd
