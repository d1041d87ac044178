// engine.h -- device-resident state and per-iteration orchestration of one factorisation
// (internal header).  This is the MI355X-native replacement of the reference's L2/L1 layers:
// IAlgorithm + the five Algorithm*.h classes (source/nmf/Algorithm.h:38-77) and DeviceMatrix
// (source/common/Matrix.h:446-645).  Everything stays in HBM between upload and download;
// the host sees n + r partial sums on error iterations, exactly like the reference.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>
#include <string>
#include <vector>

#include "device_buffers.h"
#include "engine_state.h"
#include "kernels.h"

namespace nmfamd {

// What Engine::plan reads of the device -- and all it reads: the plan, and with it the kernel path and the order of every partial sum, is a function of the shape,
// the parameters, these three numbers and the environment switches.  device_facts() gathers them from the current HIP device; nmfamd_plan_geometry takes them from its caller.
struct DeviceFacts {
	int num_cus = 256;
	size_t memory_side_cache_bytes = 0;   // AMD Infinity Cache; 0 = unknown: no cache window
	size_t free_bytes = 0;                // free device memory before the engine allocates anything
};
hipError_t device_facts(DeviceFacts* out);

// What the runtime knows about a pointer, without an engine and without a kernel: kind 0 not known to the runtime (ordinary host memory), 1 device memory, 2 pinned
// host memory, 3 anything else (managed, array); device: where it lives (-1 for kind 0); bytes_from_p: bytes from p to the end of its allocation (0 unless kind = 1).
void device_pointer_info(const void* p, int* kind, int* device, unsigned long long* bytes_from_p);

// ALG_HALS: coordinate descent (kernels_hals.hip, docs/HALS.md) -- the generic launch sequence only, single-engine runs only (no three-phase / sharded form)
// ALG_NENMF: the HALS iteration with accelerated projected-gradient steps in place of the sweeps (kernels_nenmf.hip, docs/NENMF.md); HALS's limits
enum Algorithm { ALG_MU = 0, ALG_GDCLS = 1, ALG_ALS = 2, ALG_ACLS = 3, ALG_AHCLS = 4, ALG_NSNMF = 5, ALG_HALS = 6, ALG_NENMF = 7 };
// the two algorithms that share the HALS iteration (products, slabs, ps, trace, normalisation, penalties, constant W) and differ in the step of a factor
inline bool hals_family(int alg) { return alg == ALG_HALS || alg == ALG_NENMF; }

struct AlgorithmParams {
	double lambda = 0, lambdaW = 0, lambdaH = 0, alphaW = 0, alphaH = 0, theta = 0;
	// extensions without a reference counterpart (selected by new Parameter names, see abi.cpp):
	double divergence = 0;      // 0: Frobenius objective, 1: generalised KL divergence, 2: Itakura-Saito divergence, 3: the beta-divergence at beta_value (multiplicative
	                            // update only; 2 and 3 are always the dense path)
	double sparse_compute = 0;  // 1: keep V as CSR + CSC in HBM and multiply by SpMM instead of densifying
	double precision = 0;       // 1: bf16 MFMA operands (V, W, H rounded to bf16 inside the two big products), fp32 everywhere else
	double missing_values = 0;  // 1: fit the stored entries only (multiplicative update; implies sparse compute, kernels_masked.hip, docs/MISSING.md)
	// L1 / L2 penalties on W and on H; all 0: the unpenalised iteration.  HALS (docs/HALS.md: scikit-learn's coordinate descent) and the dense divergence updates
	// (docs/DIVERGENCE.md: scikit-learn's solver="mu") take them, no other engine.  Engine::set_hals_penalties changes them between iterations.
	double l1W = 0, l1H = 0, l2W = 0, l2H = 0;
	// HALS: sweeps per product in the H step and in the W step (accelerated HALS, docs/HALS.md "Inner sweeps"); integers in 1 ... 64, (1, 1): the plain iteration.
	// Engine::set_hals_sweeps changes them between iterations.
	double sweeps_h = 1, sweeps_w = 1;
	// HALS: the tolerance delta of the per-column dynamic stopping rule (docs/HALS.md, "Dynamic stopping"), in [0, 1); 0: static counts.  With delta > 0 the
	// counts above are maximum counts.  Engine::set_hals_sweep_tolerance changes it between iterations.
	double sweep_tolerance = 0;
	// NeNMF: projected-gradient steps per product in the H step and in the W step (docs/NENMF.md); integers in 1 ... 256.  Engine::set_nenmf_steps changes them
	// between iterations.
	double steps_h = APG_STEPS_DEFAULT, steps_w = APG_STEPS_DEFAULT;
	// NeNMF: the tolerance delta of the per-column dynamic stopping rule (docs/NENMF.md, "Dynamic stopping"), in [0, 1); 0: static counts.  With delta > 0 the
	// counts above are maximum counts.  Engine::set_nenmf_step_tolerance changes it between iterations.
	double steps_tolerance = 0;
	double dense_compute = 0;  // 1 with divergence = 1: the KL update on a dense resident V (kernels_beta.hip, docs/DIVERGENCE.md) instead of over the stored entries
	double beta_value = 0;      // divergence = 3: the beta of the divergence, any finite value (0 and 1 run the Itakura-Saito and dense KL engines as they are)
	double weighted = 0;        // 1 on a dense divergence engine: per-entry weights uploaded beside V (upload_dense_weighted; kernels_beta_weighted.hip, docs/DIVERGENCE.md)
	double mixed_precision = 0; // 1 on a dense divergence fp32 engine: the operands of the fused half-step's products rounded to bf16 (kernels_beta_bf16.hip, docs/DIVERGENCE.md)
	double batch_size = 0;      // > 0 on a dense divergence engine: the minibatch (online) update over blocks of batch_size columns of V (kernels_beta_online.hip, docs/DIVERGENCE.md)
	double forget_factor = 0;   // ... its forgetting factor in [0, 1]: rho = forget_factor^(min(batch_size, n) / n) scales the accumulated numerator and denominator of W
	// missing_values = 1: the divergence of the masked update -- 0 Frobenius (kernels_masked.hip), 1 generalised KL, 2 Itakura-Saito, 3 the beta-divergence at
	// missing_beta (kernels_masked_beta.hip, docs/MISSING.md "Beta-divergence"); fields of their own, as 'weighted' has: 'divergence' stays refused beside missing_values
	double missing_divergence = 0, missing_beta = 0;
	bool is_masked() const { return missing_values != 0; }
	bool is_masked_beta() const { return missing_values != 0 && missing_divergence != 0; }
	double masked_beta() const { return missing_divergence == 2 ? 0.0 : missing_divergence == 3 ? missing_beta : 1.0; }
	bool is_minibatch() const { return batch_size != 0; }
	// the dense beta-divergence update: Itakura-Saito (beta = 0) and the general form always, generalised KL (beta = 1) with dense_compute
	bool is_beta_dense() const { return divergence == 2 || divergence == 3 || (divergence == 1 && dense_compute != 0); }
	double beta() const { return divergence == 2 ? 0.0 : divergence == 3 ? beta_value : 1.0; }
	bool takes_penalties(bool is_hals) const { return is_hals || is_beta_dense() || is_masked_beta(); }
	bool hals_penalised() const { return l1W != 0 || l1H != 0 || l2W != 0 || l2H != 0; }
};

// What a set of penalties (l1W, l1H, l2W, l2H) must satisfy, stated once for Engine::set_hals_penalties and nmfgpu::compute: nullptr, or why not.
// fp32: the kernels of a float engine take the values as float, where a large double is not finite.  takes_penalties: a HALS engine or a dense divergence engine
// (AlgorithmParams::takes_penalties).
inline const char* hals_penalties_fault(double l1W, double l1H, double l2W, double l2H, bool fp32, bool takes_penalties) {
	const double v[4] = {l1W, l1H, l2W, l2H};
	bool any = false;
	for (double x : v) {
		if (!(x >= 0) || x > 1.7976931348623157e308) return "HALS penalties: l1W, l1H, l2W and l2H must be finite and >= 0";
		if (fp32 && x > 3.4028234663852886e38) return "HALS penalties: value out of the range of the engine's precision";
		any = any || x != 0;
	}
	if (any && !takes_penalties) return "HALS penalties: only the HALS algorithm takes l1W / l1H / l2W / l2H";
	return nullptr;
}

// What the sweep counts of accelerated HALS must satisfy, stated once for Engine::set_hals_sweeps and nmfgpu::compute (which reads them from Parameters, as
// doubles): nullptr, or why not.
inline const char* hals_sweeps_fault(double sweeps_h, double sweeps_w, bool is_hals) {
	for (double x : {sweeps_h, sweeps_w}) {
		if (!(x >= HALS_SWEEPS_MIN && x <= HALS_SWEEPS_MAX) || x != (double)(int)x) return "HALS sweeps: sweepsH and sweepsW must be integers in 1 ... 64";
	}
	if ((sweeps_h != 1 || sweeps_w != 1) && !is_hals) return "HALS sweeps: only the HALS algorithm takes sweepsH / sweepsW other than 1";
	return nullptr;
}

// What the step counts of NeNMF must satisfy, stated once for Engine::set_nenmf_steps and nmfgpu::compute (which reads them from Parameters, as doubles): nullptr,
// or why not.  given: the caller named a count (a Parameter, the setter), which only a NeNMF engine takes.
inline const char* nenmf_steps_fault(double steps_h, double steps_w, bool given, bool is_nenmf) {
	if (given && !is_nenmf) return "NeNMF steps: only the NeNMF algorithm takes stepsH / stepsW";
	for (double x : {steps_h, steps_w}) {
		if (!(x >= APG_STEPS_MIN && x <= APG_STEPS_MAX) || x != (double)(int)x) return "NeNMF steps: stepsH and stepsW must be integers in 1 ... 256";
	}
	return nullptr;
}

// What the tolerance of the dynamic stopping rule must satisfy, stated once for Engine::set_hals_sweep_tolerance and nmfgpu::compute: nullptr, or why not.
inline const char* hals_sweep_tolerance_fault(double delta, bool is_hals) {
	if (!(delta >= 0 && delta < 1)) return "HALS sweep tolerance: sweepsTolerance must be a finite value in [0, 1)";      // (NaN fails both comparisons)
	if (delta != 0 && !is_hals) return "HALS sweep tolerance: only the HALS algorithm takes a sweepsTolerance other than 0";
	return nullptr;
}

// ... and the tolerance of NeNMF's rule, for Engine::set_nenmf_step_tolerance and nmfgpu::compute.  given: the caller named a value that only a NeNMF engine takes
// (the setter: any value; a Parameter: a non-zero one).
inline const char* nenmf_step_tolerance_fault(double delta, bool given, bool is_nenmf) {
	if (!(delta >= 0 && delta < 1)) return "NeNMF step tolerance: stepsTolerance must be a finite value in [0, 1)";      // (NaN fails both comparisons)
	if (given && !is_nenmf) return "NeNMF step tolerance: only the NeNMF algorithm takes a stepsTolerance";
	return nullptr;
}

// What the parameters of the dense beta-divergence update (docs/DIVERGENCE.md) must satisfy, stated once for Engine::allocate and nmfgpu::compute: nullptr, or why not.
inline const char* beta_dense_fault(const AlgorithmParams& p, bool is_mu, int r, int row_blocks = 1) {
	if (!(p.dense_compute == 0 || p.dense_compute == 1)) return "dense divergence update: 'denseCompute' has to be 0 or 1";
	if (p.dense_compute != 0 && p.divergence == 0) return "dense divergence update: 'denseCompute' selects the dense form of a divergence ('divergence' = 1 or 2), not the Frobenius objective";
	if (!(p.beta_value - p.beta_value == 0)) return "dense divergence update: 'beta' has to be finite";
	if (p.beta_value != 0 && p.divergence != 3) return "dense divergence update: 'beta' needs 'divergence' = 3 (the general beta-divergence)";
	if (!p.is_beta_dense()) return nullptr;
	if (!is_mu) return "dense divergence update: the Multiplicative algorithm only";
	if (p.sparse_compute != 0 || p.missing_values != 0) return "dense divergence update: does not combine with 'sparseCompute' or 'missingValues' (V is kept dense; a divergence with beta <= 0 is undefined at 0)";
	if (p.precision > 0) return "dense divergence update: no bf16 operands";
	if (r > 256) return "dense divergence update: rank <= 256";
	if (row_blocks > 1) return "dense divergence update: single GPU only (no row blocks)";
	return nullptr;
}

// What 'missing_divergence' and 'missing_beta' (nmfamd_params_v7) must satisfy, after beta_dense_fault: nullptr, or why not.  (A 'missing_beta' outside the range of
// the engine's precision is Engine::check_parameters' to refuse.)
inline const char* masked_beta_fault(const AlgorithmParams& p, bool is_mu, int r, int row_blocks = 1) {
	const double d = p.missing_divergence;
	if (!(d == 0 || d == 1 || d == 2 || d == 3)) return "missing-value divergence: 'missingDivergence' has to be 0 (Frobenius), 1 (KL), 2 (Itakura-Saito) or 3 (beta)";
	if (!(p.missing_beta - p.missing_beta == 0)) return "missing-value divergence: 'missingBeta' has to be finite";
	if (p.missing_beta != 0 && d != 3) return "missing-value divergence: 'missingBeta' needs 'missingDivergence' = 3 (the general beta-divergence)";
	if (d == 0) return nullptr;
	if (p.missing_values != 1) return "missing-value divergence: 'missingDivergence' needs 'missingValues' = 1";
	if (p.divergence != 0) return "missing-value divergence: does not combine with 'divergence' (that one selects the unmasked updates)";
	if (!is_mu) return "missing-value divergence: the Multiplicative algorithm only";
	if (r > 256) return "missing-value divergence: rank <= 256";
	if (p.weighted != 0 || p.mixed_precision != 0 || p.batch_size != 0) return "missing-value divergence: does not combine with 'weighted', 'mixedPrecision' or 'batchSize' (those are the dense engines')";
	if (row_blocks > 1) return "missing-value divergence: single GPU only (no row blocks)";
	return nullptr;
}

// The solver of a Frobenius missing-value engine (docs/MISSING.md, "Coordinate descent"): 0 the multiplicative update, 1 coordinate descent over the observed entries
// with sweeps_h / sweeps_w sweeps per half-step and scikit-learn's penalties.  A setting of the engine (Engine::set_missing_solver), not a field of AlgorithmParams.
struct MissingSolver {
	int solver = 0, sweeps_h = 1, sweeps_w = 1;
	double l1W = 0, l1H = 0, l2W = 0, l2H = 0;
};
constexpr int MISSING_CD_MAX_RANK = 128;      // (the padded ranks kernels_masked_cd.hip instantiates: 64 and 128)
// What such a setting must satisfy, stated once for Engine::set_missing_solver and nmfgpu::compute (which reads it from Parameters, as doubles): nullptr, or why not.
// masked / frobenius: the engine fits the observed entries only / under the Frobenius objective; r: its rank.
inline const char* missing_solver_fault(double solver, double sweeps_h, double sweeps_w, double l1W, double l1H, double l2W, double l2H, bool fp32, bool masked, bool frobenius,
                                        int r) {
	if (!(solver == 0 || solver == 1)) return "missing-value solver: 'missingSolver' has to be 0 (multiplicative update) or 1 (coordinate descent)";
	if (!masked) return "missing-value solver: needs 'missingValues' = 1 (an engine that fits the observed entries only)";
	if (!frobenius) return "missing-value solver: the Frobenius objective only ('missingDivergence' = 0)";
	for (double x : {sweeps_h, sweeps_w})
		if (!(x >= 1 && x <= 64) || x != (double)(int)x) return "missing-value solver: sweepsH and sweepsW must be integers in 1 ... 64";
	bool any = sweeps_h != 1 || sweeps_w != 1;
	for (double x : {l1W, l1H, l2W, l2H}) {
		if (!(x >= 0) || x > 1.7976931348623157e308) return "missing-value solver: l1W, l1H, l2W and l2H must be finite and >= 0";
		if (fp32 && x > 3.4028234663852886e38) return "missing-value solver: penalty out of the range of the engine's precision";
		any = any || x != 0;
	}
	if (solver == 0 && any) return "missing-value solver: the multiplicative update takes sweeps 1 and penalties 0 only";
	if (solver == 1 && r > MISSING_CD_MAX_RANK) return "missing-value solver: coordinate descent supports 1 ... 128 features";
	return nullptr;
}

// What 'weighted' (nmfamd_params_v4) must satisfy, after beta_dense_fault: nullptr, or why not.
inline const char* weighted_fault(const AlgorithmParams& p) {
	if (!(p.weighted == 0 || p.weighted == 1)) return "weighted NMF: 'weighted' has to be 0 or 1";
	if (p.weighted != 0 && !p.is_beta_dense()) return "weighted NMF: only on a dense divergence engine ('divergence' = 2 or 3, or 1 with 'denseCompute')";
	return nullptr;
}

// What 'mixedPrecision' (nmfamd_params_v5) must satisfy, after beta_dense_fault and weighted_fault: nullptr, or why not.  ('precision' = 1 on a dense divergence
// engine stays refused by beta_dense_fault: there it would mean V itself stored in bf16.)
inline const char* mixed_precision_fault(const AlgorithmParams& p, bool fp32) {
	if (!(p.mixed_precision == 0 || p.mixed_precision == 1)) return "mixed precision: 'mixedPrecision' has to be 0 or 1";
	if (p.mixed_precision == 0) return nullptr;
	if (!p.is_beta_dense()) return "mixed precision: only on a dense divergence engine ('divergence' = 2 or 3, or 1 with 'denseCompute')";
	if (!fp32) return "mixed precision: single-precision engines only";
	if (p.weighted != 0) return "mixed precision: does not combine with 'weighted' (the weighted kernels have no bf16 form)";
	return nullptr;
}

// What 'batchSize' and 'forgetFactor' (nmfamd_params_v6) must satisfy, after the three above: nullptr, or why not.
inline const char* minibatch_fault(const AlgorithmParams& p) {
	if (!(p.forget_factor >= 0 && p.forget_factor <= 1)) return "minibatch update: 'forgetFactor' has to be a finite value in [0, 1]";
	if (p.batch_size == 0) return p.forget_factor != 0 ? "minibatch update: 'forgetFactor' needs a 'batchSize'" : nullptr;
	if (!(p.batch_size >= 128 && p.batch_size <= 2147483520.0) || p.batch_size != (double)(128 * (long)(p.batch_size / 128)))
		return "minibatch update: 'batchSize' has to be a positive multiple of 128 (the padding unit of the panels, which covers every kernel's reduction tile)";
	if (!p.is_beta_dense()) return "minibatch update: only on a dense divergence engine ('divergence' = 2 or 3, or 1 with 'denseCompute')";
	if (p.weighted != 0) return "minibatch update: does not combine with 'weighted' (the accumulating update has no weighted form)";
	return nullptr;
}

// Status codes shared with nmfgpu_amd.h (NMFAMD_*).
// ST_VALUE_RANGE: V holds values the split-operand product is not exact for (infinities, NaN, |v| > 2^126, 0 < |v| < 2^-100):
// the caller recreates the engine with precision = -1 (native fp32 MFMA instructions) -- nmfgpu::compute does that by itself
enum Status { ST_OK = 0, ST_INVALID = 1, ST_NO_DEVICE_MEMORY = 2, ST_NO_HOST_MEMORY = 3, ST_HIP_ERROR = 4, ST_NO_DEVICE = 5, ST_VALUE_RANGE = 6 };

// Padded rank of the factor panels: 64, or above that a multiple of 128 in fp32 (the 128-column forms of the split-operand product, the wide fp32 update and Gram
// kernels) and of 64 in fp64 (round 5: every fp64 kernel works in 64-column units -- the reference example's r = 158 ran as 256, now 192: 0.56 of the r x r work
// and 0.75 of the product's)
inline int padded_rank(int r, size_t elem_bytes = 4) { return r <= 64 ? 64 : (elem_bytes == 8 ? ((r + 63) / 64) * 64 : ((r + 127) / 128) * 128); }
inline long pad128(long v) { return ((v + 127) / 128) * 128; }

template <typename T>
class Engine {
public:
	Engine(int m, int n, int r, int algorithm, const AlgorithmParams& params);
	~Engine();

	// Creation in three steps: check_parameters() (the *_fault checks, prm_ rounded to T), plan() (every decision that fixes which kernels run and in which order
	// partial sums are added; no HIP call) and allocate_buffers() (memory, zero fills, streams and events for what plan() decided).  allocate() runs all three with
	// the facts of the current device; check_parameters() + plan() alone serve nmfamd_plan_geometry on a machine without one.
	Status allocate();
	Status check_parameters();
	Status plan(const DeviceFacts& device);
	// Row-block form of the sharded W step (sharded.cpp): the padded row count becomes a multiple of 128 * blocks, so that
	// the Wt panel splits into `blocks` equal row blocks.  Call before allocate().
	void set_row_blocks(int blocks) { row_blocks_ = blocks > 1 ? blocks : 1; }
	// the sharded three-phase API driven by a team of ONE rank: the exchange buffer goes from w_products() to w_finish() as it is
	void set_sole_rank(bool sole) { sole_rank_ = sole; }
	// The one-pass iteration (kernels_onepass.hip) claims every CU of the device for one persistent launch: engines that run
	// beside others on one device (rank threads of a team) opt out.  Call before allocate().
	void set_one_pass(bool allow) { one_pass_allowed_ = allow; }
	// 0: not in use, 1: in use, 2: was in use and gave up (a launch could not form its groups; the two-pass iteration took over)
	int one_pass_state() const { return one_pass_ ? 1 : (one_pass_gave_up_ ? 2 : 0); }
	void set_stream(hipStream_t s) { stream_ = s; }
	hipStream_t stream() const { return stream_; }

	// V: host, column-major / sparse.  Builds V, Vt and the sorted tr(V^T V) vector.
	Status upload_dense(const T* V, long ld);
	Status upload_sparse(int format, const T* values, const int* a, const int* b, long nnz, int base);
	// weighted engines: V and the weights Omega (m x n, column-major, host); the only upload they take.  Omega finite and >= 0 with one entry > 0; V obeys the rule
	// of the engine's beta where Omega > 0 and is not looked at (stored as 0) where Omega = 0.  A second call replaces both.
	Status upload_dense_weighted(const T* V, long ldv, const T* Omega, long ldo);
	bool is_weighted() const { return weighted_; }
	// The same two uploads from DEVICE memory of the engine's device (docs/DEVICE_IO.md): layout 0 column-major (ld >= m), 1 row-major (ld >= n).  The matrix is
	// imported into the column-major staging image by kernels_import.hip, which evaluates the value rules of the host upload in the same pass; everything behind the
	// staging image (finish_upload, the weights' transpose) is the host upload's code, so the resident images and the error terms are the host upload's bit for bit
	// -- only the sum of the weights is added in another order (one partial per workgroup, then in index order).  Statuses and last_error() texts are the host
	// upload's; with several kinds of violation: a bad weight, then a bad entry of V, then "at least one weight".  Ordering: the call runs hipDeviceSynchronize()
	// before its first read, so a matrix produced on any stream of the device is complete, and returns after the engine's stream is idle.  The source is never
	// written.  ST_INVALID with last_error() before any device work for a pointer that is null, not device memory of the engine's device (host and pinned host
	// memory included), not aligned to the element, or whose extent (outer - 1) * ld + inner does not lie inside its allocation; for ld below the inner extent and
	// for another layout; and on an engine with sparse_compute / missing_values (their dense input becomes triplets on the host).
	Status upload_dense_device(const T* V, long ld, int layout);
	Status upload_dense_weighted_device(const T* V, long ldv, int layout_v, const T* Omega, long ldo, int layout_o);
	// upload_sparse with values, a and b in DEVICE memory (nmfamd_engine_upload_sparse_device), branch by branch: the host entry's refusals with its statuses and
	// texts (the value rules evaluated by a kernel), the pointer checks and the ordering of upload_dense_device over nnz elements of T (values), nnz ints (b) and nnz
	// (COO) or outer + 1 ints (a).  Sparse engines: the arrays are copied device-to-device into the arrays the image builder owns (build_sparse_images: the same code
	// on the same bits as the host entry); an input the builder hands back, and NMFAMD_SPARSE_SETUP=host, cost a download and run the host path as it is.  Every
	// other engine densifies the caller's arrays where they lie, inside the same upload_image fill.  Nothing of the caller's memory is kept or written.
	Status upload_sparse_from_device(int format, const T* values, const int* a, const int* b, long nnz, int base);
	// Dense V in DEVICE memory on an engine with sparse_compute / missing_values (nmfamd_engine_upload_dense_device_stored; every other engine refuses it): the
	// stored entries of upload_dense -- missing values: not NaN, zeros included, an infinite entry refused; otherwise != 0 -- compacted into the CSR and CSC images by
	// kernels_compact.hip (count, scan, scatter: no sort, no limit on a row's or column's length), then finish_sparse_images.  The images, the terms and every later
	// result equal upload_dense's bit for bit (sum(V) of the KL divergence: added per column, then across columns).  Checks and ordering of upload_dense_device.
	Status upload_dense_device_stored(const T* V, long ld, int layout);

	// W: host m x r (ld), H: host r x n (ld).  Either pointer may be null (leave as is).  PanelState: factors_touched, then w_set / h_set for the factor given.
	Status set_factors(const T* W, long ldw, const T* H, long ldh);
	Status get_factors(T* W, long ldw, T* H, long ldh);   // nsNMF returns W S, like the reference
	// ... to and from DEVICE memory, in either layout (W: m x r, H: r x n; 0 column-major, 1 row-major), with the semantics of the host forms (a null pointer leaves
	// that factor; the transitions of set_factors; nsNMF returns W S) and the pointer checks and the ordering of upload_dense_device: hipDeviceSynchronize() before the
	// first access, return after the engine's stream is idle -- so any stream may have written the input and any stream may read the output.  get writes the m x r /
	// r x n block only: the bytes in the gap of ld stay as they are.
	Status set_factors_device(const T* W, long ldw, int layout_w, const T* H, long ldh, int layout_h);
	Status get_factors_device(T* W, long ldw, int layout_w, T* H, long ldh, int layout_h);
	// h_first_column: global index of this engine's first column (column shards draw their part of ONE stream)
	Status randomize_factors(unsigned seed, bool w, bool h, long h_first_column = 0);
	// Predict and score entries of W H (docs/PREDICT.md), W and H being what get_factors would return now: out[p] = sum_k W(rows[p], k) H(k, cols[p]) over nnz >= 1
	// coordinates of index base 0 or 1 (unsorted, duplicates counted per copy).  values (or null: out needed) are the entries' values in T; then sums[0 .. 3] =
	// sum (v_p - out[p])^2, sum d_beta(v_p | out[p] + eps), the sum of the absolute values of the summands of d_beta, and sqrt(sums[0] / nnz); beta = NaN: no
	// divergence (sums[1], sums[2] = NaN), any finite v; otherwise the value rule of the masked beta engines.  device: every array lies in DEVICE memory of the
	// engine's device (the pointer checks and the ordering of upload_dense_device; a validation launch over the index arrays -- and the values -- runs first, and the
	// gather is not launched unless every coordinate lies inside the matrix); else in host memory (checked on the host before any device work, staged into buffers
	// the engine owns).  One body for both.  ST_INVALID with last_error() for a coordinate outside the matrix (naming the first p), a value that breaks the rule, an
	// engine with row blocks or one driven through the three-phase (column-sharded) entries, and an engine whose factors were never set.  The effects on the engine
	// are get_factors' and no more: the error of the last error iteration stays as it was.  Sums: per-entry terms in T, added in double per 16-lane group in entry
	// order, groups in group order, workgroups in workgroup order on the host; bit-identical between calls and between the two forms.
	Status predict_entries(const int* rows, const int* cols, const T* values, long nnz, int base, double beta, T* out, double* sums, bool device);
	// The k best candidates of W H per query (docs/TOPK.md), W and H being what get_factors would return now.  axis 0: a query is a row of V and the candidates are
	// the n columns; axis 1: a query is a column and the candidates are the m rows.  queries: nq >= 1 indices of base 0 or 1 (unsorted, duplicates allowed);
	// 1 <= k <= TOPK_MAX_K.  out_idx [nq][k] (int32, in the caller's base) and out_scores [nq][k]: per query the first k eligible candidates by (score descending,
	// index ascending), -1 / -inf where fewer than k are eligible.  excl_ptr [nq + 1] (64-bit, starts at 0, non-decreasing) and excl_idx [excl_ptr[nq]] (candidate
	// indices of the same base, unsorted, duplicates allowed), or both null: the candidates that are not eligible for a query.  device: every array lies in DEVICE
	// memory (the pointer checks and the ordering of upload_dense_device, excl_idx over excl_nnz elements; a validation launch reads the index arrays first and the
	// product is not launched unless it found everything inside); else in host memory (checked on the host before any device work -- excl_nnz is not read --, staged
	// into buffers the engine owns).  One body for both.  Refusals and effects as predict_entries.  Bit-identical between calls and between the two forms.
	Status top_k(const int* queries, long nq, int k, int axis, int base, const long* excl_ptr, const int* excl_idx, long excl_nnz, int* out_idx, T* out_scores, bool device);

	// The W^T V launch (and its Gram passengers) of the NEXT iteration, enqueued ahead of it: it writes the split-K slabs, G and the column scale -- scratch the
	// next iterate() would overwrite anyway -- so a caller that is about to block on this iteration's error value (nmfgpu::compute: the threshold test decides
	// whether there is a next iteration) keeps the device busy meanwhile.  Rank-64 fused path only; a no-op elsewhere.  The next iterate() skips the launch;
	// a W or a V from outside in between makes it void (PanelState::w_set, v_replaced; a new H alone does not: the launch reads W and V).
	Status begin_next_iteration();
	// One iteration.  With compute_error the frobenius()/rmsd() values are refreshed (host sync).
	Status iterate(bool compute_error, bool constant_w);
	// HALS: the penalties of the iterations that follow (>= 0 and finite; all 0: the unpenalised iteration, normalisation included).  Valid any time
	// between iterations.  ST_INVALID with last_error() for a bad value, and for a non-zero one on an engine of another algorithm.
	Status set_hals_penalties(double l1W, double l1H, double l2W, double l2H);
	// HALS: sweeps per product of the iterations that follow, h in the H step and w in the W step (1 ... 64; (1, 1): the plain iteration).  Valid any time between
	// iterations.  ST_INVALID with last_error() for a count out of range, and for a count other than 1 on an engine of another algorithm.
	Status set_hals_sweeps(int h, int w);
	// Missing values, Frobenius: the solver of the iterations that follow (docs/MISSING.md, "Coordinate descent") -- 0 the multiplicative update (sweeps 1 and
	// penalties 0 only), 1 coordinate descent over the observed entries (kernels_masked_cd.hip; rank <= 128).  Valid any time between iterations; a setting, no
	// factor changes.  ST_INVALID with last_error() for whatever missing_solver_fault names, every other engine included.
	Status set_missing_solver(const MissingSolver& s);
	const MissingSolver& missing_solver() const { return cd_; }
	// HALS: the tolerance delta of the per-column dynamic stopping rule for the iterations that follow (docs/HALS.md, "Dynamic stopping"); 0: the static counts,
	// bit for bit.  Valid any time between iterations.  ST_INVALID with last_error() for a value outside [0, 1), NaN included, and for a non-zero one on an engine
	// of another algorithm.
	Status set_hals_sweep_tolerance(double delta);
	// NeNMF: projected-gradient steps per product of the iterations that follow, h in the H step and w in the W step (1 ... 256).  Valid any time between
	// iterations.  ST_INVALID with last_error() for a count out of range, and on an engine of another algorithm.
	Status set_nenmf_steps(int h, int w);
	// NeNMF: the tolerance delta of the per-column dynamic stopping rule for the iterations that follow (docs/NENMF.md, "Dynamic stopping"); 0: the static counts,
	// bit for bit.  Valid any time between iterations.  ST_INVALID with last_error() for a value outside [0, 1), NaN included, and on an engine of another
	// algorithm.
	Status set_nenmf_step_tolerance(double delta);
	// NeNMF: the steps applied per column of H (which = 0, n entries) or row of W (which = 1, m entries) in the most recent step launch of that factor, with the
	// contract of hals_sweep_counts.
	long nenmf_step_counts(int which, int* out, long capacity);
	// HALS: the sweeps applied per column of H (which = 0, n entries) or row of W (which = 1, m entries) in the most recent step of that factor.  Waits for the
	// stream.  The number of entries copied; negative on another engine, for another `which`, for a capacity too small and before any such step.
	long hals_sweep_counts(int which, int* out, long capacity);

	// Split form for column-sharded multi-GPU runs (exchange = device buffer of exchange_count()
	// elements: the local (V H^T)^T panel followed by the local H H^T):
	//   h_step -> w_products(exchange) -> [all-reduce exchange across ranks] -> w_finish(exchange)
	Status h_step(bool compute_error);
	Status w_products(T* exchange);
	Status w_finish(const T* exchange, bool compute_error);
	// ... and without a reduction in between: exchanges[p] = rank p's exchange buffer as its w_products() left it, readable from this device (count ranks, rank
	// order).  Available where direct_w_finish() says so (rank-64 multiplicative update on the split-operand path).
	Status w_finish_peers(const T* const* exchanges, int count, bool compute_error);
	bool direct_w_finish() const { return fused_capable() && gram_image_ && prm_.divergence == 0; }
	// KL update (sparse V): the exchange also carries the row sums of the local H and, on error iterations, the per-row error terms:
	//   [ numerator panel RP x mpad | H_g H_g^T RP x RP | rowsum(H_g) RP | tr terms mpad | KL terms mpad ]
	// (masked engines have no three-phase form: no exchange)
	long exchange_count() const { return prm_.is_masked() || beta_dense_ ? 0 : (long)RP_ * mpad_ + (long)RP_ * RP_ + (prm_.divergence != 0 ? (long)RP_ + 2 * mpad_ : 0); }
	bool is_kl() const { return prm_.divergence != 0; }
	bool is_masked() const { return prm_.is_masked(); }
	bool is_masked_beta() const { return masked_beta_; }
	double masked_beta() const { return mbeta_; }      // the beta of a masked divergence engine, in the precision of T
	bool is_beta_dense() const { return beta_dense_; }
	// sharded runs: the error terms refer to the whole matrix (sorted tr(V^T V) terms of ALL columns, sum of ALL entries, total column count)
	void set_error_globals(const std::vector<T>& vtv_sorted_all, double sum_v_all, long total_columns) { column_shard_ = true; h_vtv_ = vtv_sorted_all; sum_v_ = sum_v_all; err_total_columns_ = total_columns; }
	double sum_v() const { return sum_v_; }
	// Row-block form of w_finish (reduce-scatter by row blocks of W -> every GPU updates its rows -> all-reduce
	// of the r column-norm partials -> all-gather of the normalised rows).  num_rows: the reduced (V H^T)^T rows
	// [row0, row0 + rows) in panel layout; hht: the reduced H H^T.  w_update_rows leaves the r partial sums of squares of
	// the new rows in colsq (device, RP elements); after their all-reduce w_normalize_rows scales the block, and once the
	// blocks of every rank have been gathered into w_panel(), w_rows_replaced() drops what was derived from the old W.
	Status w_update_rows(const T* num_rows, const T* hht, long row0, long rows, bool compute_error, T* colsq);
	Status w_normalize_rows(long row0, long rows, T* colsq);
	void w_rows_replaced() { state_.w_rows_replaced(); }
	T* w_panel() { return Wt_; }
	double beta() const { return beta_; }      // the beta of a dense divergence engine, in the precision of T
	int kl_blocks(bool w_step) const { return prm_.divergence != 0 && !beta_dense_ ? (w_step ? kl_blocks_w_ : kl_blocks_h_) : 0; }
	int gram_k_slices() const { return gram_spread_ ? GRAM_REDUCE_BLOCKS : gram_ksplit_; }      // (16: the spread form)
	bool w_col_split() const { return w_col_split_; }
	int fused_launches() const {
		if ((fused_capable() && !one_pass_ && gram_image_) || (fused64_planned_ && fused64_capable())) return 4;
		return fused32w_planned_ && fused32w_capable() ? 8 - (f32w_ride_h_ > 0 ? 1 : 0) - (f32w_ride_w_ > 0 ? 1 : 0) : 0;
	}
	int gram_ride_slices(bool w_side) const { return fused64_planned_ ? (w_side ? f64_slices_w_ : f64_slices_h_) : (fused32w_planned_ ? (w_side ? f32w_ride_w_ : f32w_ride_h_) : 0); }
	// Row-block form at padded rank 256 with bf16 operands (config 4): between two W updates the OTHER ranks read only the bf16 fragments of a rank's rows (the next
	// W^T V's operand and the Gram matrix are made from them) -- so the all-gather carries the fragments w_normalize_rows() left for this rank's rows (RP / 2 four-byte
	// words per row: 25.6 MB at config 4 instead of 51.2 MB of fp32 rows) and the fp32 rows of the other ranks stay STALE in w_panel() until somebody needs them
	// (get_factors, a fresh set of fragments): then the hook -- the sharded run's all-gather of the fp32 row blocks, a COLLECTIVE -- runs first.
	bool w_fragment_exchange() const { return tri_; }
	void* w_fragments() { return Wtb_; }
	long w_fragment_words_per_row() const { return RP_ / 2; }
	// the fragments of every rank's rows have been gathered into w_fragments(); stale: the fp32 rows of the other ranks were not
	void w_fragments_gathered(bool stale) { state_.w_fragments_gathered(stale); }
	void set_w_gather_hook(std::function<Status()> hook) { w_gather_hook_ = std::move(hook); }
	void w_rows_gathered() { state_.w_rows_stale = false; }
	bool w_rows_stale() const { return state_.w_rows_stale; }
	Status materialize() { return materialize_w(); }
	// error terms of the last error iteration (host copies): n_local per-column terms and r terms
	const std::vector<T>& terms_htwtv() { finalize_error(false); return h_psN_; }
	const std::vector<T>& terms_hhtwtw() { finalize_error(false); return h_psR_; }
	const std::vector<T>& terms_vtv_sorted() const { return h_vtv_; }
	long error_terms_to_device(T* dst, long capacity);   // [psN (last count) | psR (r)], D2D on the stream
	// sharded runs: the terms are fetched with error_terms_to_device() only -- the engine's own copy to the host (and its event) is skipped
	void set_error_terms_stay_on_device(bool stay) { error_terms_stay_ = stay; }
	void resolve_error(const std::vector<T>& vtv_sorted, std::vector<T> htwtv, std::vector<T> hhtwtw, long total_elements);      // (sorts copies: terms_htwtv() keeps the column order)

	// Error of the most recent error iteration.  The n + r partial sums travel to the host
	// asynchronously; the first reader waits for them and does the sorted summation, so a caller
	// that does not look at the error every time (the benchmark loop) never stalls the stream.
	double kl_divergence() { finalize_error(true); return kl_; }
	double divergence_value() { finalize_error(true); return kl_; }      // the objective of whichever divergence the engine has (KL, Itakura-Saito or general beta; no penalty terms)
	bool sparse_mode() const { return sparse_; }
	bool sparse_setup_on_device() const { return sparse_setup_on_device_; }
	long nnz() const { return nnz_; }
	double frobenius() { finalize_error(true); return frob_; }
	double frobenius_squared() { finalize_error(true); return frob2_; }      // the resolved sum before the root
	double rmsd() { finalize_error(true); return rmsd_; }

	// Timing of the dominant kernel (the factor product): when enabled, every launch is bracketed
	// by HIP events on the engine's stream; dominant_stats reads them back (host sync).
	// stride: time the launches of every stride-th iteration only (1 = all)
	void enable_kernel_timing(bool on, int stride = 1) { timing_ = on; timing_stride_ = stride > 0 ? stride : 1; timing_iter_ = 0; }
	// kind_ms / kind_launches (optional, two entries each): the same split by product -- [0] the H-side product (W^T V, or the KL H half-step's gather), [1] the W side
	void dominant_stats(double* total_ms, long* launches, double* pair_overhead_ms = nullptr, double* kind_ms = nullptr, long* kind_launches = nullptr);

	int m() const { return m_; }
	int n() const { return n_; }
	int r() const { return r_; }
	int rp() const { return RP_; }
	// GDCLS and the ALS family evaluate tr(H^T W^T V) as r terms (one per factor row, from the reduced sums: identical on every rank of a
	// column-sharded run); the multiplicative algorithms as one term per column of V
	bool error_terms_per_factor_row() const { return alg_ != ALG_MU && alg_ != ALG_NSNMF && !hals_family(alg_); }
	int algorithm() const { return alg_; }
	long mpad() const { return mpad_; }
	long npad() const { return npad_; }
	int slabs_h() const { return planH_.splits; }
	int slabs_w() const { return planW_.splits; }
	// which kernel runs the two big products: 0 fp32 MFMA, 1 bf16-rounded operands, 2 fp32 by exact 3 x bf16 splitting,
	// 3 fp64 MFMA, 4 VALU fallback kernel (NMFAMD_FORCE_VALU), 5 sparse (SpMM), 6 the fused dense beta-divergence half-step (kernels_beta.hip)
	int resident_images() const { return sparse_ ? 0 : weighted_ ? 4 : (one_image_ ? 1 : 2); }      // (weighted: V, the weights and both transposes)
	int product_kernel() const { return beta_dense_ ? (mixed_ ? 7 : 6) : sparse_ ? 5 : bf16_ ? 1 : x3_ ? 2 : !tiled_ ? 4 : (sizeof(T) == 8 ? 3 : 0); }
	const char* last_error() const { return last_error_; }

	// test access to device intermediates (panel layout, host copies)
	Status debug_read(int which, T* out, long count);

private:
	Status hip_fail(hipError_t e, const char* what);
	Status allocate_buffers();                       // third step of allocate(): a buffer exists if plan() set its flag; no decision of its own
	DeviceBuffers buffers_;                          // every device and pinned allocation of the engine, creation and uploads alike: the typed members below are views
	// set by plan(), read by allocate_buffers(): the fused fp64 / wide fp32 iteration is in use (f64_* / f32w_scale_ exist), qx3_ exists, the stamp buffers of the
	// measurement builds exist; the passengers' work tables until they are uploaded
	bool fused64_planned_ = false, fused32w_planned_ = false, wide_q_image_ = false, f64_stamps_wanted_ = false, op_stamps_wanted_ = false;
	std::vector<int> f64_items_h_host_, f64_items_w_host_;
	Status h_step_impl(bool compute_error);
	// prepacked: the split (x3) image of F is already in Wx3_ / Hx3_ (emitted by the update kernel that wrote F)
	Status product_h(const T* F, const GramReduceArgs* rg = nullptr, bool prepacked = false);   // slabs_ <- partials of F V   (r x n)
	Status product_w(const T* F, const GramReduceArgs* rg = nullptr, T* single_slab_out = nullptr, bool prepacked = false);   // slabs_ (or the caller's panel when there is one K slice) <- partials of (V F^T)^T (r x m)
	bool fused_capable() const;                      // fp32, padded rank 64, MU (and nsNMF on the split-operand products)
	bool fused32w_capable() const;                   // fp32, split-operand products, MU / nsNMF, padded ranks 128 ... 512: the eight-launch iteration of iterate_fused32w
	Status iterate_fused32w(bool compute_error);     // (Gram slices + reduce) / product / update, twice; W carried unnormalised with a pending column scale, no pack / smooth / normalise launches
	bool fused64_capable() const;                    // fp64, MU / nsNMF, any padded rank up to 512: the four-launch iteration of iterate_fused64
	Status iterate_fused64(bool compute_error);      // product (+ Gram passengers) / update / product (+ Gram passengers) / update, W carried unnormalised with a pending column scale
	bool gram_from_update() const;                   // GDCLS / ALS family at fp32, padded rank 64: Gram matrices from the update kernel's partials
	Status iterate_mu64(bool compute_error);         // the four-launch iteration of kernels_mu64.hip
	Status iterate_onepass(bool compute_error);      // the one-pass iteration of kernels_onepass.hip
	Status onepass_check();                          // host sync: did a one-pass launch give up?
	Status materialize_w(bool whole_panel = true);
	Status ensure_w_rows();                          // fold the pending column scale into Wt_
	Status normalize_w(bool from_gram_partials, int norm_parts);   // column normalisation of W after its update
	Status normal_inverse(T* A, T offdiag, T diag);  // Qinv_ <- (A + regulariser)^-1, A destroyed
	Status normal_inverse_fork(T* A, T offdiag, T diag);   // the same on the side stream; normal_inverse_join() before Qinv_ is read
	Status normal_inverse_join();
	bool passengers_ride(const FactorProductPlan& plan) const; // split-operand product, rank 64: the Gram passengers find CUs beside the product blocks
	bool inverse_rides(const FactorProductPlan& plan) const;   // the inverse can be a passenger workgroup of the product launch
	Status finish_upload(T* Vcol);                   // (its first statement is PanelState::v_replaced)
	template <typename Fill> Status upload_image(bool zeroed, Fill fill);   // every dense upload behind its checks: staging image, fill(T* Vcol), finish_upload, release; a new input path is a fill
	Status refuse_weighted(int flags);               // the three refusals of a weighted upload by IMPORT_* flags, in their precedence; ST_OK if none
	Status finish_weighted_upload(double sum_w);     // ... and its tail: finish_upload(V_), Omt_, the synchronisation, sum_w_, beta_uploaded_
	Status export_panel_w(bool want_w, const T** src);   // get_factors / get_factors_device: one-pass check, materialize_w, nsNMF's W S; *src = the panel to read W from
	Status upload_triplets(std::vector<int>& rows, std::vector<int>& cols, std::vector<T>& vals);   // sparse mode: builds CSR + CSC on the host (the fall-back of upload_sparse_device)
	Status upload_sparse_device(int format, const T* values, const int* a, const int* b, long nnz, int base, bool* fallback);   // ... on the device (kernels_sparse_setup.hip), from HOST arrays: three copies, then ...
	template <typename Fill> Status build_sparse_images(int format, long nnz, int base, bool* fallback, Fill fill);   // ... the builder on device arrays it owns; fill copies the caller's arrays into them
	Status finish_sparse_images(long nnz);            // the tail of every device-side builder: tr(V^T V) terms, sum_v_, nnz_, sparse_setup_on_device_, setup_kl_blocks
	Status upload_sparse_on_host(int format, const T* values, const int* a, const int* b, long nnz, int base);   // host arrays -> triplets -> upload_triplets
	enum { SPARSE_NO_ENTRY = 8 };                     // (beside the IMPORT_* flags of kernels.h)
	Status refuse_sparse_input(int format, long nnz); // what both forms of the sparse upload refuse before they look at an array
	Status refuse_sparse_values(int found);           // ... and on a missing-values engine: SPARSE_NO_ENTRY, or IMPORT_BAD_VALUE for a value that is not finite
	bool sparse_setup_on_host() const;                // NMFAMD_SPARSE_SETUP=host
	Status setup_kl_blocks();
	bool sparse_setup_on_device_ = false;
	Status iterate_kl(bool compute_error);            // KL-divergence multiplicative update (sparse mode)
	Status iterate_masked(bool compute_error, bool constant_w);   // multiplicative update over the stored entries only (kernels_masked.hip)
	Status iterate_masked_beta(bool compute_error, bool constant_w);   // ... under the beta-divergence (kernels_masked_beta.hip)
	Status iterate_masked_cd(bool compute_error, bool constant_w);     // ... by coordinate descent (kernels_masked_cd.hip; cd_.solver == 1)
	Status masked_refuses(const char* what);          // ST_INVALID with last_error_ set: no three-phase / sharded form of the masked update
	const char* masked_value_fault() const;           // the text of a stored value that breaks the rule of a masked divergence engine's beta
	Status iterate_beta_minibatch(bool compute_error);            // ... its minibatch (online) form: one pass over the batches (kernels_beta_online.hip)
	Status iterate_beta(bool compute_error, bool constant_w);     // dense beta-divergence multiplicative update (kernels_beta.hip, docs/DIVERGENCE.md)
	Status beta_refuses(const char* what);            // ... nor of the dense beta-divergence update
	Status beta_check_values(const T* values, long count, long ld, long rows);   // upload: beta <= 0 needs finite values > 0, beta > 0 finite values >= 0
	const char* beta_value_fault() const;             // ... the text of a violation
	// the check of a caller's device matrix (rows x cols, layout, ld) before any device work: ST_OK, or ST_INVALID with last_error() naming `name` and what is wrong
	Status check_device_matrix(const char* name, const void* p, long ld, int layout, long rows, long cols);
	Status check_device_vector(const char* name, const void* p, size_t elem, long count);   // ... of a device array of `count` elements of `elem` bytes (null taken where count is 0)
	Status check_device_extent(const std::string& name, const void* p, size_t elem, unsigned long long elems, const std::string& extent);   // what the two share, over the element size
	Status refuse(std::string text) { error_text_ = std::move(text); last_error_ = error_text_.c_str(); return ST_INVALID; }
	std::string error_text_;                          // owns a composed last_error_ text
	int device_ = -1;                                 // the HIP device the buffers live on (allocate_buffers)
	// predict_entries: staging of host coordinate lists (pe_rows_, pe_cols_, pe_vals_) and of the predictions (pe_out_), pe_cap_ entries each, grown on demand; the
	// per-workgroup sums (pe_part_: 3 * PREDICT_MAX_PARTS doubles) and the two words of the validation launch (pe_flags_); pinned landing buffers of the sums and
	// flags (pe_pin_) and of the predictions (pe_pin_out_, pe_pin_cap_ entries)
	int *pe_rows_ = nullptr, *pe_cols_ = nullptr;
	T *pe_vals_ = nullptr, *pe_out_ = nullptr, *pe_pin_out_ = nullptr;
	double *pe_part_ = nullptr, *pe_pin_ = nullptr;
	unsigned* pe_flags_ = nullptr;
	long pe_cap_ = 0, pe_pin_cap_ = 0;
	// top_k: staging of host queries and exclusion lists (tk_q_, tk_eptr_: tk_q_cap_ queries; tk_eidx_: tk_e_cap_ entries), the slabs' partial lists (tk_part_s_,
	// tk_part_i_: tk_part_cap_ entries), the results of host calls (tk_out_i_, tk_out_s_ and their pinned landing buffers tk_pin_i_, tk_pin_s_: tk_out_cap_ entries),
	// the three words of the validation launch (tk_flags_) and their pinned landing buffer (tk_pin_flags_)
	int *tk_q_ = nullptr, *tk_eidx_ = nullptr, *tk_part_i_ = nullptr, *tk_out_i_ = nullptr, *tk_pin_i_ = nullptr;
	long* tk_eptr_ = nullptr;
	T *tk_part_s_ = nullptr, *tk_out_s_ = nullptr, *tk_pin_s_ = nullptr;
	unsigned *tk_flags_ = nullptr, *tk_pin_flags_ = nullptr;
	long tk_q_cap_ = 0, tk_e_cap_ = 0, tk_part_cap_ = 0, tk_out_cap_ = 0;
	bool have_w_ = false, have_h_ = false;            // a W / an H has been set or drawn (set_factors, set_factors_device, randomize_factors)
	bool column_shard_ = false;                       // the three-phase entries or a sharded run have driven this engine: it holds a column shard of a larger matrix
	Status fetch_error_terms(int count_n);            // enqueue the copies, do not wait
	void finalize_error(bool resolve);
	void record_begin(int kind = 0);
	void record_end();
	bool timed_launch_events(int kind, hipEvent_t* start, hipEvent_t* stop);      // a sampled launch that takes its own start / stop events (hipExtLaunchKernel); then timed_launch_done()
	void timed_launch_done() { ev_used_ += 2; }

	int m_, n_, r_, RP_, alg_;
	int row_blocks_ = 1;
	AlgorithmParams prm_;
	long mpad_, npad_;
	long strideV_ = 0, strideVt_ = 0, elemsV_ = 0, elemsVt_ = 0;   // x-tiled images of V / Vt
	int num_cus_ = 256;
	hipStream_t stream_ = nullptr;
	// side stream for the r x r inverse of the least-squares algorithms: one workgroup, independent of the product
	// against V that follows the Gram matrix, so the two run side by side (the product leaves CUs idle)
	hipStream_t aux_ = nullptr;
	hipEvent_t ev_fork_ = nullptr, ev_join_ = nullptr;
	bool overlap_inverse_ = false;
	bool tiled_ = false;                      // V_/Vt_ are x-tiled (fp32 MFMA path)
	const char* last_error_ = "";

	T *V_ = nullptr, *Vt_ = nullptr;
	T *Wt_ = nullptr, *H_ = nullptr;          // factor panels
	PanelState state_;                        // which derived buffers describe them and V, and the transitions of the entries that change one from outside (engine_state.h)
	T *Ws_ = nullptr, *Hs_ = nullptr;         // nsNMF: smoothed copies (W S)^T and S H
	T *slabs_ = nullptr;
	T *numW_ = nullptr;                       // reduced (V H^T)^T panel (LS family error terms, sharded runs)
	T *Wold_ = nullptr;                       // LS family: W before the update
	T *rowdot_part_ = nullptr;                // ... and the per-workgroup partial vectors of launch_row_dot's coalesced form
	T *G_ = nullptr, *G2_ = nullptr, *HHt_ = nullptr, *Qinv_ = nullptr, *gram_part_ = nullptr;
	T *sumsq_part_ = nullptr;
	// HALS: the sweeps applied per column of H (npad) and per row of W (mpad) in the most recent H and W step of the dynamic kernel (0 on padding); *_valid_: a
	// step of that factor has run.  A NeNMF engine keeps the counts of its steps in the same members.
	int *hals_counts_h_ = nullptr, *hals_counts_w_ = nullptr;
	bool hals_counts_h_valid_ = false, hals_counts_w_valid_ = false;
	int hals_static_h_ = 0, hals_static_w_ = 0;      // > 0: that step ran this fixed number of sweeps (tolerance 0, or a maximum of 1) and wrote no counts
	// one panel sweep launch of an HALS step, static or dynamic by prm_.sweep_tolerance, and the counts of the step
	Status hals_sweeps(bool w_step, T* P, const T* G, int S, int len_pad, int len_valid, T* ps, T* sumsq_part, T l1, T l2);
	// NeNMF: the launch of prm_.steps_h / steps_w projected-gradient steps in the same place, on the same arrays, static or dynamic by prm_.steps_tolerance
	Status apg_steps(bool w_step, T* P, const T* G, int S, int len_pad, int len_valid, T* ps, T* sumsq_part, T l1, T l2);
	// the step of a factor of whichever of the two algorithms the engine runs, and the number of partial sums of squares its W step leaves
	long family_counts(int which, int* out, long capacity);
	Status family_step(bool w_step, T* P, const T* G, int S, int len_pad, int len_valid, T* ps, T* sumsq_part, T l1, T l2) {
		return alg_ == ALG_NENMF ? apg_steps(w_step, P, G, S, len_pad, len_valid, ps, sumsq_part, l1, l2) : hals_sweeps(w_step, P, G, S, len_pad, len_valid, ps, sumsq_part, l1, l2);
	}
	int family_parts(int len_pad) const { return alg_ == ALG_NENMF ? panel_steps_apg_parts(RP_, sizeof(T), len_pad) : panel_sweep_hals_parts(RP_, sizeof(T), len_pad); }
	// bf16-operand products (kernels_bf16.hip): fragment-ordered bf16 images of V, Vt and of the two factor panels
	bool bf16_ = false;
	void *Vb_ = nullptr, *Vtb_ = nullptr, *Wtb_ = nullptr, *Hb_ = nullptr;
	int ksW_ = 0, ksH_ = 0;
	FactorProductPlan planHb_, planWb_;
	// fp32 products on the bf16 matrix pipe by exact 3-way operand splitting (kernels_x3.hip): the fp32 tiled
	// images of V stay as they are, the factor panel is split into Wx3_ / Hx3_ before each product
	bool x3_ = false;
	// one resident image of V instead of two: W^T V reads the image tiled along its reduction index (the y-tiled form of
	// k_factor_product_x3; ~20 % slower per launch, half the memory).  Chosen when two images would not fit, or by
	// NMFAMD_ONE_IMAGE.
	bool one_image_ = false;
	int img_th_ = 128;        // rows per tile of the V image: 16 with one resident image (both kernel forms read contiguously), else the plan's
	void *Wx3_ = nullptr, *Hx3_ = nullptr;
	void* qx3_ = nullptr;     // split image of the r x r operand of the wide fp32 panel update
	FactorProductPlan planHx_, planWx_;
	// sparse-V compute path (kernels_sparse.hip): CSR and CSC images of V, 0-based
	bool sparse_ = false;
	long nnz_ = 0;
	int *csr_ptr_ = nullptr, *csr_idx_ = nullptr, *csc_ptr_ = nullptr, *csc_idx_ = nullptr, *csc_from_csr_ = nullptr;
	T *csr_val_ = nullptr, *csc_val_ = nullptr, *q_ = nullptr, *q2_ = nullptr;
	T *t_vwh_ = nullptr, *t_kl_ = nullptr, *rowsum_part_ = nullptr, *sW_ = nullptr, *sH_ = nullptr;
	// KL half-steps with the gathered factor cut into blocks that fit an XCD's L2 (kernels_sparse.hip, k_kl_fused): blocked pointer arrays
	// [rows][blocks + 1] of the CSR image (W step: column blocks of H) and of the CSC image (H step: row blocks of W), partial panels
	int kl_blocks_w_ = 1, kl_blocks_h_ = 1;
	int *csr_bptr_ = nullptr, *csc_bptr_ = nullptr;
	T *kl_part_ = nullptr, *kl_tpart_ = nullptr;
	double sum_v_ = 0, kl_ = 0;
	// KL error terms travel like the Frobenius ones: pinned landing buffer [t_vwh (m) | t_kl (m) | sW (RP) | sH (RP) | psR (RP)],
	// copied stream-ordered, summed on the host only when somebody reads the error
	T* pin_kl_ = nullptr;
	bool kl_pending_ = false, kl_unresolved_ = false;
	std::vector<T> h_klrow_, h_sW_, h_sH_;
	// masked update: per-workgroup sums of squares of the new W rows ([MASKED_NORM_PARTS + 16][RP]); the per-row residual terms travel through pin_kl_ (first m)
	T* msq_part_ = nullptr;
	bool masked_pending_ = false, masked_unresolved_ = false;
	MissingSolver cd_;      // set_missing_solver: the penalties rounded to T
	// ... under the beta-divergence (prm_.is_masked_beta()): mbeta_ = prm_.masked_beta() rounded to T, what the launches take; the two per-row terms travel like the
	// dense divergence engines' (t_vwh_ / t_kl_ -> pin_kl_, beta_pending_), rmsd over the stored entries
	bool masked_beta_ = false;
	double mbeta_ = 1;
	// dense beta-divergence update: V_ is the column-major image (the H step's), Vt_ its transpose (the W step's); slabs_ holds the slabs' partial numerators,
	// beta_den_ their partial denominators (beta = 0), beta_tpart_ the slabs' parts of the two per-row error terms ([2][BETA_MAX_SLABS][mpad])
	bool beta_dense_ = false, beta_uploaded_ = false;
	double beta_ = 1;      // prm_.beta() rounded to T: what the launches take and what selects the engine (0: Itakura-Saito, 1: dense KL, else the general form)
	BetaPlan betaH_, betaW_;
	T *beta_den_ = nullptr, *beta_tpart_ = nullptr;
	bool beta_pending_ = false, beta_unresolved_ = false;
	// ... weighted (prm_.weighted): Om_ / Omt_ are the images of the weights in the layouts of V_ / Vt_, sum_w_ their sum (in double, on the host, at upload: rmsd's
	// divisor); beta_den_ is allocated at beta = 1 too (the weighted KL denominator is a product)
	bool weighted_ = false;
	// ... minibatch (prm_.batch_size > 0): batch_ columns per step, rho_ = forget_factor^(min(batch_, n) / n) in the precision of T; the plans of the two half-steps
	// of a full batch (betaHb_, betaWb_) and of the remainder batch (betaHr_, betaWr_); online_A_ / online_B_ the accumulated numerator and denominator panels of W
	// ([mpad][RP], set to W and 1 before the first step after the factors were set: PanelState::online_stale)
	bool minibatch_ = false;
	long batch_ = 0;
	double rho_ = 0;
	BetaPlan betaHb_, betaWb_, betaHr_, betaWr_;
	T *online_A_ = nullptr, *online_B_ = nullptr;
	// ... mixed precision (prm_.mixed_precision, fp32 only): iterate_beta launches launch_beta_fused_bf16 in place of launch_beta_fused, nothing else changes
	bool mixed_ = false;
	T *Om_ = nullptr, *Omt_ = nullptr;
	double sum_w_ = 0;
	// rank-64 MU fast path: W is kept unnormalised with a pending column scale (kernels_mu64.hip)
	float *gramW_part_ = nullptr, *gramH_part_ = nullptr, *scale_ = nullptr, *Graw64_ = nullptr;
	bool w_col_split_ = false;       // V H^T from 128 x 32 workgroups and one slab (narrow column shards, Engine::plan)
	bool gram_spread_ = false;       // ... or, one slice: the sixteen passengers share the ten tiles' K ranges (gram_image.h, spread form) and the last one finishes G_
	unsigned* gram_spread_counter_ = nullptr;
	int gram_ksplit_ = 1;            // K slices of the W^T W passengers (gram_image.h): > 1 for column shards narrower than config 2
	float* Gpart_ = nullptr;         // [GRAM_KSPLIT_MAX][4096] unscaled slices of W^T W (the H update adds and scales them, and stores G_)
	float* wsq_part_ = nullptr;      // [mpad / 32][64] partial sums of squares of the rows the last W update wrote (k_mu64_update32<true>): the pending column scale's source
	// split-operand path: Gram matrices from the split images (gram_image.h), 32-column update kernel -- no partial Gram matrices
	bool gram_image_ = false;
	GramReduceArgs gram_args(bool of_w, float* G, float* scale, int normalize) const;
	Status standalone_gram(const GramReduceArgs& rg);
	Status mu64_update(bool is_w, const T* slabs, int S, long slab_stride, const T* Q, bool compute_error, const PeerSlabs* peers = nullptr);
	// padded rank 256 with bf16 product operands (kernels_tri.hip): one pass per factor between its update and the product that streams
	// it (normalise + smooth + bf16 fragments), Gram matrices of the smoothed panels from the unsmoothed ones (S G S)
	bool tri_ = false;
	unsigned* tri_ride_counters_ = nullptr;          // arrival counters of the Gram passengers (tri_gram_tile.h): zero between launches
	bool tri_ride_w_ = false, tri_ride_h_ = false;   // the Gram matrix of W / of S H rides in the W^T V / V (S H)^T launch (Engine::plan leaves TRI_PASSENGERS CUs free)
	bool sole_rank_ = false;
	T* kl_scale_ = nullptr;          // KL iteration: W's pending column scale d (RP factors, from k_kl_sums; PanelState::kl_scale_pending)
	bool kl_err_iter_ = false;       // sharded KL: h_step's compute_error, for the W-side evaluation in w_products
	long err_total_columns_ = 0;     // sharded runs: columns of the whole matrix (0: this engine's own n)
	Status kl_h_step();
	Status kl_w_products(T* exchange, bool compute_error);
	Status kl_w_finish(const T* exchange, bool compute_error);
	bool tri_w_den_bf16_ = true;     // the W update's r x r product takes the old rows rounded to bf16 (NMFAMD_TRI_FP32_DEN=1: six-term fp32-accurate product)
	// Gw_raw_ holds W^T W without the pending scale: what the error term's trace multiplies it with
	const T* tri_trace_scale() const { return (tri_ && state_.tri_scale_pending) ? reinterpret_cast<const T*>(colsq_) : nullptr; }
	std::function<Status()> w_gather_hook_;
	int colsq_parts_ = 1;            // staged partial vectors in colsq_ (kernels_tri.hip: launch_colsq_stage)
	float *gram_tri_part_ = nullptr, *Gw_raw_ = nullptr, *Gh_raw_ = nullptr, *colsq_ = nullptr;
	struct Smoothing { T off, diag; };               // nsNMF's S = (1 - theta) I + theta / r 1 1^T as (off-diagonal, diagonal), in T: the one place that computes them; the identity (0, 1) on every other engine
	Smoothing smoothing_constants() const { const T off = (T)prm_.theta / (T)(unsigned)r_; return alg_ == ALG_NSNMF ? Smoothing{off, (T)((1.0 - (T)prm_.theta) + off)} : Smoothing{T(0), T(1)}; }
	hipError_t smooth_panel(const T* P, T* Ps, long len_pad) { const auto [off, diag] = smoothing_constants(); return launch_smooth_panel<T>(P, Ps, RP_, r_, len_pad, off, diag, stream_); }
	Status tri_prepare_w(GramReduceArgs* ride = nullptr);          // Wtb_, Gw_raw_, G_ for the H step (ride: the Gram matrix as passengers of the product launch that follows, tri_gram_tile.h)
	Status tri_prepare_h(T* hht, bool local_q, GramReduceArgs* ride = nullptr);    // Hb_, Gh_raw_, hht (= the Gram matrix of the smoothed H) for the W step
	Status tri_update_w(const T* num, int S, long stride, const T* hht);   // W update + normalisation + everything tri_prepare_w() would do
	// fused double-precision iteration (round 6, iterate_fused64; PanelState::f64_pending): the column scale is applied by the consumers (kernels_f64.hip: gram_ride_f64 -> f64_scale_, PanelFusedF64) -- materialize_w() folds it into the panel
	float* f32w_scale_ = nullptr;                    // fused fp32 iteration at padded ranks >= 128: the pending column scale (k_gram_reduce_x3)
	int f32w_ride_h_ = 0, f32w_ride_w_ = 0;         // ... K slices per super-block of W^T W / H H^T that ride the product launches as passenger workgroups (0: a launch of their own)
	Status fused64_product_h();
	double *f64_scale_ = nullptr, *f64_partial_ = nullptr;
	unsigned* f64_counters_ = nullptr;
	int *f64_items_h_ = nullptr, *f64_items_w_ = nullptr;   // XCD-aware work tables of the passengers (gram_ride_f64_items)
	int f64_slices_h_ = 0, f64_slices_w_ = 0;        // K slices of the Gram passengers riding in the W^T V / V H^T launch
	const GramRideF64* ride64_ = nullptr;            // set around a product_h / product_w call
	unsigned long long* f64_stamps_ = nullptr;       // measurement builds (NMFAMD_F64_STAMPS = file): [4 launches][4096][8] stamps of the LAST fused iteration, written out by the destructor
	bool h_partials_unneeded_ = false; // set by iterate() around its H step: GDCLS takes H H^T from the split image beside the product against V
	int normalize_next_ = 0;
	T *psN_ = nullptr, *psR_ = nullptr;
	long ps_stride_ = 0;
	double* inv_work_ = nullptr;
	T* stage_ = nullptr;                      // upload/download staging (max(m, n) x r)
	int* range_flag_ = nullptr;               // device word, see launch_column_sumsq
	long slab_stride_ = 0;
	int gram_parts_ = 128;
	FactorProductPlan planH_, planW_;
	// one pass over V per iteration (kernels_onepass.hip): scratch of the in-launch hand-offs, per-XCD partial results
	bool one_pass_allowed_ = true, one_pass_ = false, one_pass_gave_up_ = false;
	void *op_part_ = nullptr, *op_hfrag_ = nullptr;
	unsigned *op_ctl_ = nullptr;                      // [0..7] tickets, [8] abort flag
	float *op_slabs_ = nullptr, *op_hh_part_ = nullptr, *op_ps4_ = nullptr;
	T* op_H2_ = nullptr;                              // the panel the next one-pass launch writes the new H into (swapped with H_ after it)
	unsigned op_seq_ = 0;
	unsigned* pin_abort_ = nullptr;
	unsigned long long* op_stamps_ = nullptr;          // diagnostic builds (NMFAMD_ONEPASS_STAMPS = file the last launch's stamps go to)

	T *pin_psN_ = nullptr, *pin_psR_ = nullptr;
	bool error_terms_stay_ = false;
	bool ps_last_direct_ = false;   // ... and the most recent error iteration did (error_terms_to_device reads the pinned buffer then)
	bool ps_direct_ = false;        // this (error) iteration's update kernels write the pinned buffer directly (iterate_mu64)
	T* pin_psN_dev_ = nullptr;      // the device's address of pin_psN_ (hipHostGetDevicePointer): fetch_error_terms writes it from a kernel
	hipEvent_t err_event_ = nullptr;
	bool err_pending_ = false, err_unresolved_ = false;
	int err_count_ = 0;
	std::vector<T> h_vtv_, h_psN_, h_psR_;
	double frob_ = 0, frob2_ = 0, rmsd_ = 0;

	bool timing_ = false;
	int timing_stride_ = 1;
	long timing_iter_ = 0;
	bool timing_now_ = false;
	std::vector<hipEvent_t> ev_;
	std::vector<char> ev_kind_;              // per event pair: which product it brackets (record_begin)
	size_t ev_used_ = 0;
};

// Host-side part of the error evaluation: sorted, interleaved accumulation in double
// (source/nmf/FrobeniusResolver.cpp:29-51).  The two iteration-dependent vectors are sorted here.
template <typename T>
double resolve_frobenius(const std::vector<T>& vtv_sorted, std::vector<T>& htwtv, std::vector<T>& hhtwtw);
// ... before the root (negative for a term vector that is not an error at all: the ALS family's constant-W trace)
template <typename T>
double resolve_frobenius_squared(const std::vector<T>& vtv_sorted, std::vector<T>& htwtv, std::vector<T>& hhtwtw);

} // namespace nmfamd
