/* nmfgpu_amd.h -- C-ABI of the MI355X engine BELOW the nmfgpu.h boundary.
 *
 * nmfgpu.h (nmfgpu::compute and friends) is the drop-in boundary: host pointers in, host
 * pointers out, one blocking call per factorisation.  This header exposes the same engine
 * one level lower, for callers that want V to stay resident in HBM across calls (the benchmark
 * harness, the column-sharded multi-GPU driver, the per-kernel parity tests).  Plain C: opaque
 * handles, plain pointers and sizes, int status codes; no C++ or torch types.
 *
 * Each entry point names the reference code whose job it does (paths relative to the nmfgpu
 * v0.2.3 tree).  All matrices are column-major; "ld" is a leading dimension in elements.
 * The `_f32` / `_f64` suffix is the element type (the reference's NumericType = float / double).
 */
#ifndef NMFGPU_AMD_H
#define NMFGPU_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(NMFGPU_EXPORTING)
#  define NMFAMD_API __attribute__((visibility("default")))
#else
#  define NMFAMD_API
#endif

/* status codes */
enum {
	NMFAMD_OK = 0,
	NMFAMD_INVALID_ARGUMENT = 1,
	NMFAMD_NO_DEVICE_MEMORY = 2,
	NMFAMD_NO_HOST_MEMORY = 3,
	NMFAMD_HIP_ERROR = 4,
	NMFAMD_NO_DEVICE = 5,
	NMFAMD_VALUE_RANGE = 6   /* upload: V holds infinities, NaN, |v| > 2^126 or 0 < |v| < 2^-100, which the default fp32 product (operands split
	                            exactly into three bf16 terms) does not cover: create the engine with nmfamd_params.precision = -1 (native fp32
	                            MFMA instructions).  nmfgpu::compute and the Python Engine do that by themselves. */
};

/* algorithm ids = nmfgpu::NmfAlgorithm (include/nmfgpu.h:107-114; NMFAMD_HALS is an extension: coordinate descent, docs/HALS.md -- dense or
   sparse compute, L1 / L2 penalties through nmfamd_engine_set_hals_penalties, no three-phase / sharded form).  The dense divergence engines (NMFAMD_MU with
   divergence 2, 3, or 1 with dense_compute) take the same penalties on their multiplicative update (docs/DIVERGENCE.md).
   NMFAMD_NENMF is an extension too (docs/NENMF.md): the iteration of NMFAMD_HALS with Nesterov-accelerated projected-gradient steps in place of the sweeps
   (nmfamd_engine_set_nenmf_steps); ranks 1 ... 128 in either precision, otherwise the limits and the penalties of NMFAMD_HALS */
enum { NMFAMD_MU = 0, NMFAMD_GDCLS = 1, NMFAMD_ALS = 2, NMFAMD_ACLS = 3, NMFAMD_AHCLS = 4, NMFAMD_NSNMF = 5, NMFAMD_HALS = 6, NMFAMD_NENMF = 7 };

/* sparse formats = nmfgpu::StorageFormat (include/nmfgpu.h:177-186) */
enum { NMFAMD_DENSE = 0, NMFAMD_CSR = 1, NMFAMD_CSC = 2, NMFAMD_COO = 3 };

/* Algorithm parameters, the reference's name/value list (Interface.cpp:41-49, 249-326) as a struct.  Fields are only ever added at the END:
 * callers build the struct from this header (a struct declared by hand from an older copy is shorter than what the library reads). */
typedef struct nmfamd_params {
	double lambda;   /* GDCLS  "lambda"  */
	double lambdaW;  /* ACLS / AHCLS "lambdaW" */
	double lambdaH;  /* ACLS / AHCLS "lambdaH" */
	double alphaW;   /* AHCLS "alphaW" */
	double alphaH;   /* AHCLS "alphaH" */
	double theta;    /* nsNMF "theta" */
	/* extensions without a reference counterpart (nmfgpu::compute: Parameter names "divergence", "sparseCompute") */
	double divergence;      /* 0 = Frobenius objective; 1 = generalised KL divergence (Multiplicative only; over the stored entries of a sparse image of V -- implies
	                           sparse_compute -- unless nmfamd_params_v2.dense_compute = 1); 2 = Itakura-Saito divergence (Multiplicative only, always the dense path of
	                           docs/DIVERGENCE.md: every entry of V finite and > 0, dense input only); 3 = the beta-divergence at nmfamd_params_v3.beta (Multiplicative only,
	                           always the dense path; nmfamd_engine_create_v2) */
	double sparse_compute;  /* 1 = keep V as CSR + CSC in HBM and use SpMM / SDDMM kernels instead of densifying (Multiplicative, and HALS with
	                           divergence 0; rank <= 256) */
	double precision;       /* Parameter "precision", float engines only.  0 = fp32 accuracy: products on the bf16 matrix pipe with every
	                           operand split exactly into three bf16 terms (kernels_x3.hip); -1 = native fp32 MFMA instructions;
	                           1 = operands rounded to bf16 (reduced precision, half the bytes of V per pass) */
	double missing_values;  /* Parameter "missingValues".  1 = fit the observed entries only (docs/MISSING.md): the stored entries of a sparse V, the
	                           non-NaN entries of a dense V (zeros included); Multiplicative with divergence 0 only, implies sparse_compute.  Such an
	                           engine has no three-phase / sharded form: nmfamd_engine_h_step / _w_products / _w_finish and nmfamd_sharded_create return
	                           NMFAMD_INVALID_ARGUMENT; nmfamd_engine_frobenius / _rmsd report the error over the observed entries */
} nmfamd_params;

/* nmfamd_params with the fields added since nmfamd_engine_create's struct was frozen.  nmfamd_engine_create reads a nmfamd_params of the size it was compiled
 * with, so a field added there would be read past the struct of a caller built against an older header; the fields that follow therefore live in this
 * struct, which nmfamd_engine_create_v2 takes together with its size (it reads min(params_size, sizeof(nmfamd_params_v2)) bytes and takes the rest as 0, as
 * nmfamd_engine_geometry_sized does for its struct).  Fields are only ever added at the END. */
typedef struct nmfamd_params_v2 {
	nmfamd_params base;
	double dense_compute;   /* Parameter "denseCompute".  1 with base.divergence = 1: the KL update on a dense resident V (docs/DIVERGENCE.md: fused matrix-pipe half-steps,
	                           kernels_beta.hip) instead of over the stored entries; every entry finite and >= 0, sparse input is densified.  The same iteration as the
	                           sparse path.  Refused with divergence = 0; not needed with divergence = 2.  The dense divergence engines (this, and divergence = 2)
	                           are single-GPU: rank <= 256, no sparse_compute / missing_values / bf16 precision (bf16 product operands under fp32 data are
	                           nmfamd_params_v5.mixed_precision), no three-phase / sharded form
	                           (nmfamd_engine_h_step / _w_products / _w_finish and nmfamd_sharded_create return NMFAMD_INVALID_ARGUMENT); constant_w is available.
	                           An upload that breaks the value rule returns NMFAMD_INVALID_ARGUMENT with nmfamd_engine_last_error set */
} nmfamd_params_v2;

/* nmfamd_params_v2 followed by what has been added since (nmfamd_params_v2 keeps its size: callers pass sizeof of the struct they were built with).
 * nmfamd_engine_create_v2 reads min(params_size, sizeof(nmfamd_params_v3)) bytes and takes the rest as 0. */
typedef struct nmfamd_params_v3 {
	nmfamd_params_v2 v2;
	double beta;            /* Parameter "beta", with v2.base.divergence = 3: the beta of the beta-divergence, any finite value (0.5 and 1.5 are the usual choices for
	                           magnitude spectrograms; 2 is the Frobenius objective run as a multiplicative divergence update).  The multiplicative update of
	                           scikit-learn's solver="mu" on a dense resident V (docs/DIVERGENCE.md); beta is taken in the engine's precision.  beta = 0 and beta = 1 run the
	                           engines of divergence = 2 and of divergence = 1 with dense_compute, bit for bit.  beta <= 0: every entry of V finite and > 0, dense
	                           input only; beta > 0: finite and >= 0, sparse input is densified.  A non-zero beta with another divergence, and a non-finite beta, are
	                           refused.  The limits of the dense divergence engines (nmfamd_params_v2.dense_compute) apply */
} nmfamd_params_v3;

/* nmfamd_params_v3 followed by what has been added since (v2 and v3 keep their sizes).  nmfamd_engine_create_v2 takes it with its size (see
 * nmfamd_params_v5). */
typedef struct nmfamd_params_v4 {
	nmfamd_params_v3 v3;
	double weighted;        /* 0 or 1.  1: weighted NMF (docs/DIVERGENCE.md, "Weighted update") -- the objective is sum_ij w_ij d_beta(v_ij | (W H)_ij) with a matrix of
	                           weights w >= 0 uploaded beside V by nmfamd_engine_upload_dense_weighted (the only upload such an engine takes).  A weight of 0 means the
	                           entry is not there (missing-value NMF for every beta; V may hold anything at it, NaN included); real weights are weighted NMF (LS-NMF at
	                           beta = 2).  Only on a dense divergence engine: v3.v2.base.divergence = 2 or 3, or 1 with dense_compute; any other value, and weighted = 1
	                           on any other engine, is refused at creation.  The limits of the dense divergence engines apply */
} nmfamd_params_v4;

/* nmfamd_params_v4 followed by what has been added since (v2 to v4 keep their sizes).  nmfamd_engine_create_v2 reads min(params_size, sizeof(nmfamd_params_v5))
 * bytes and takes the rest as 0. */
typedef struct nmfamd_params_v5 {
	nmfamd_params_v4 v4;
	double mixed_precision; /* 0 or 1.  1: the mixed-precision form of the dense divergence update (docs/DIVERGENCE.md, "Mixed precision"; kernels_beta_bf16.hip) -- the
	                           operands of the fused half-step's two products (the panels W and H as they are staged, and Q = V .* P^(beta - 2), R = P^(beta - 1) after
	                           the element-wise map) are rounded to bf16, round to nearest even, and multiplied on the bf16 matrix instructions; V, P + eps, the map,
	                           the error terms, every accumulation and the master panels stay fp32.  Only on a single-precision dense divergence engine
	                           (divergence = 2 or 3, or 1 with dense_compute) without weights: any other value, a double-precision engine, weighted = 1 with it, and
	                           mixed_precision = 1 on any other engine are refused at creation.  base.precision = 1 stays refused on these engines (it would mean V
	                           itself stored in bf16).  The limits of the dense divergence engines apply */
} nmfamd_params_v5;

/* nmfamd_params_v5 followed by what has been added since (v2 to v5 keep their sizes).  nmfamd_engine_create_v2 reads min(params_size, sizeof(nmfamd_params_v6))
 * bytes and takes the rest as 0: a v5-sized struct gives the engine it always gave. */
typedef struct nmfamd_params_v6 {
	nmfamd_params_v5 v5;
	double batch_size;      /* 0, or a positive multiple of 128.  > 0: the minibatch (online) form of the dense divergence update (docs/DIVERGENCE.md, "Minibatch
	                           update"; scikit-learn's MiniBatchNMF).  One iteration is one pass over the column ranges [0, b), [b, 2 b), ... of V in order (the last one
	                           the remainder): the columns of H in the batch take the ordinary multiplicative step, W the online one from numerator and denominator
	                           panels accumulated over the batches.  No normalisation; the errors of an error iteration are those of (W, H) AFTER the pass.  Only on a
	                           dense divergence engine (divergence = 2 or 3, or 1 with dense_compute), single or double precision, with or without penalties and
	                           mixed_precision; not with weighted = 1; nmfamd_engine_iterate refuses constant_w on it.  Any other value is refused at creation */
	double forget_factor;   /* in [0, 1], taken literally: rho = forget_factor^(min(batch_size, n) / n) scales the accumulated panels before a step adds its own
	                           (scikit-learn's default is 0.7; 0: every step keeps only its own numerator and denominator).  A non-zero value without a batch_size is
	                           refused at creation */
} nmfamd_params_v6;

/* nmfamd_params_v6 followed by what has been added since (v2 to v6 keep their sizes).  nmfamd_engine_create_v2 and nmfamd_plan_geometry read
 * min(params_size, sizeof(nmfamd_params_v7)) bytes and take the rest as 0: a v6-sized struct gives the engine it always gave. */
typedef struct nmfamd_params_v7 {
	nmfamd_params_v6 v6;
	double missing_divergence; /* with base.missing_values = 1: the divergence of the masked update (docs/MISSING.md, "Beta-divergence").  0 = the Frobenius objective
	                              (kernels_masked.hip, as ever); 1 = generalised KL; 2 = Itakura-Saito; 3 = the beta-divergence at missing_beta.  The iteration is the
	                              weighted update of docs/DIVERGENCE.md at 0 / 1 weights with both sums over the stored entries only -- O(nnz r) at every beta
	                              (kernels_masked_beta.hip).  beta <= 0: every stored value finite and > 0 (a stored zero is refused); beta > 0: finite and >= 0 (a stored
	                              zero is an observation); an upload that breaks the rule returns NMFAMD_INVALID_ARGUMENT with nmfamd_engine_last_error set.
	                              nmfamd_engine_set_hals_penalties is accepted (none: normalisation as the weighted update; any: none); constant_w is available;
	                              nmfamd_engine_divergence reports sum_p d_beta(v_p | (W H)_p + eps) over the stored entries, frobenius / rmsd the residual over them.
	                              base.divergence stays refused beside missing_values.  Refused at creation with nmfamd_engine_last_error: a value outside
	                              {0, 1, 2, 3}; != 0 without missing_values = 1, with base.divergence != 0, with another algorithm than Multiplicative, r > 256,
	                              weighted, mixed_precision, batch_size or row blocks.  The three-phase and sharded calls are refused as on every masked engine */
	double missing_beta;       /* with missing_divergence = 3: the beta, any finite value, taken in the engine's precision; 0 and 1 run the kernels of
	                              missing_divergence = 2 and 1, bit for bit.  A non-zero value with another missing_divergence, and a value that is not finite or
	                              lies outside the range of the engine's precision, are refused at creation */
} nmfamd_params_v7;

typedef struct nmfamd_engine nmfamd_engine;  /* opaque; owns every device buffer of one factorisation */

/* Number of visible HIP devices (0 when there is none), and the library's build description. */
NMFAMD_API int nmfamd_device_count(void);
NMFAMD_API const char* nmfamd_build_info(void);
/* Text of the last failed HIP call on this thread's engine (diagnostics only).  e = NULL: why the last nmfamd_engine_create on this thread failed. */
NMFAMD_API const char* nmfamd_engine_last_error(const nmfamd_engine* e);

/* Creates the device state for V (m x n) ~ W (m x r) H (r x n) on the CURRENT HIP device.
 * Replaces IAlgorithm::allocateMemory (e.g. AlgorithmMultiplicativeFrobenius.h:85-128) minus the
 * upload.  elem_bytes: 4 (float) or 8 (double).  stream: a hipStream_t (0 = the null stream);
 * every kernel and copy of this engine is issued on it. */
NMFAMD_API int nmfamd_engine_create(int m, int n, int r, int algorithm, const nmfamd_params* params,
                                    int elem_bytes, void* stream, nmfamd_engine** out);
/* The same with the sized, extended parameter struct (nmfamd_params_v2 ... _v7; params_size = sizeof of the caller's struct, at least
 * sizeof(nmfamd_params) unless params is NULL) and the row blocks of nmfamd_engine_create_blocks (1: none). */
NMFAMD_API int nmfamd_engine_create_v2(int m, int n, int r, int algorithm, const void* params, unsigned long params_size,
                                       int elem_bytes, void* stream, int row_blocks, nmfamd_engine** out);
NMFAMD_API void nmfamd_engine_destroy(nmfamd_engine* e);

/* Upload V from host memory; builds V, its transpose and the sorted tr(V^T V) vector.
 * Replaces DeviceMatrix::copyFrom(inputMatrix) + the trace kernel + host sort
 * (AlgorithmMultiplicativeFrobenius.h:118-126; sparse -> dense with index base: Matrix.h:145-232). */
NMFAMD_API int nmfamd_engine_upload_dense(nmfamd_engine* e, const void* V, long ld);
/* Weighted engines (nmfamd_params_v4.weighted = 1): V and the weights Omega, both m x n column-major host matrices of the engine's precision.  Every weight
 * finite and >= 0, at least one > 0; where a weight is > 0, V obeys the value rule of the engine's beta (finite; > 0 for beta <= 0, >= 0 for beta > 0); where it
 * is 0, V is not looked at (and is stored as 0).  Keeps four dense images (V, Omega and their transposes: nmfamd_geometry.resident_images = 4); a second call
 * replaces both matrices.  rmsd = frobenius / sqrt(sum of the weights).  NMFAMD_INVALID_ARGUMENT with nmfamd_engine_last_error for a value that breaks a rule
 * and on an engine that is not weighted; a weighted engine refuses nmfamd_engine_upload_dense and nmfamd_engine_upload_sparse the same way. */
NMFAMD_API int nmfamd_engine_upload_dense_weighted(nmfamd_engine* e, const void* V, long ldv, const void* Omega, long ldo);
/* format CSR: a = rowPtr (m+1), b = column indices; CSC: a = columnPtr (n+1), b = row indices;
 * COO: a = row indices, b = column indices (nnz each).  base = 0 or 1. */
NMFAMD_API int nmfamd_engine_upload_sparse(nmfamd_engine* e, int format, const void* values, const int* a, const int* b, long nnz, int base);

/* W: m x r, H: r x n, host memory; a null pointer leaves that factor untouched.
 * Replaces CopyStrategy (source/init/CopyStrategy.h:41-46) and storeFactorization. */
NMFAMD_API int nmfamd_engine_set_factors(nmfamd_engine* e, const void* W, long ldw, const void* H, long ldh);
NMFAMD_API int nmfamd_engine_get_factors(nmfamd_engine* e, void* W, long ldw, void* H, long ldh);

/* ---- device-resident input and output (docs/DEVICE_IO.md) ------------------------------------
 * The four entries above with DEVICE pointers: a matrix that already lies in HBM (computed by another library on the same GPU) goes into the engine, and the
 * factors come out of it, without crossing to the host.  layout: NMFAMD_COLUMN_MAJOR (ld >= rows) or NMFAMD_ROW_MAJOR (ld >= columns); ld in elements.
 * Pointer check, before any device work: the memory has to be device memory of the engine's device (hipPointerGetAttributes), aligned to the element, and the
 * extent the call touches -- (outer - 1) * ld + inner elements -- has to lie inside its allocation (hipMemGetAddressRange).  A null pointer where one is needed,
 * host or pinned host memory, managed memory, another device's memory, ld below the inner extent and a layout other than 0 / 1 return
 * NMFAMD_INVALID_ARGUMENT with nmfamd_engine_last_error naming the argument and what is wrong; no kernel reads such a pointer.
 * Ordering: each entry calls hipDeviceSynchronize() before its first access -- a matrix produced on ANY stream of the device is complete, and nobody still reads
 * a destination -- and returns after the engine's stream is idle, so any stream may use the result.  Sources are never written. */
enum { NMFAMD_COLUMN_MAJOR = 0, NMFAMD_ROW_MAJOR = 1 };
/* Replaces nmfamd_engine_upload_dense for V (m x n) in device memory: a copy / transpose kernel writes the column-major staging image of the host upload and
 * evaluates the value rule of a dense divergence engine in the same pass; everything behind that image is the host upload's code, so the resident images, the
 * tr(V^T V) terms and every later result equal those of nmfamd_engine_upload_dense on the same values bit for bit.  Statuses and nmfamd_engine_last_error texts
 * are the host entry's: NMFAMD_INVALID_ARGUMENT for a value that breaks the rule (the engine is then without a valid V), NMFAMD_VALUE_RANGE as there.
 * Refused on an engine with sparse_compute or missing_values (nmfamd_engine_upload_dense_device_stored is the entry of those) and on a weighted engine. */
NMFAMD_API int nmfamd_engine_upload_dense_device(nmfamd_engine* e, const void* V, long ld, int layout);
/* Replaces nmfamd_engine_upload_dense_weighted: V and Omega (m x n each, layouts independent of each other) in device memory.  The joint value rule is evaluated
 * on the device; with more than one kind of violation the one reported is: a bad weight, then a bad entry of V, then "at least one weight has to be > 0".  The
 * resident images equal the host entry's bit for bit; the sum of the weights (rmsd's divisor) is added in double as one partial per 64 x 64 tile and then in tile
 * order -- a function of the input and the shape only, within m n 2^-53 (relative) of the host entry's sum.  Refused on an engine that is not weighted. */
NMFAMD_API int nmfamd_engine_upload_dense_weighted_device(nmfamd_engine* e, const void* V, long ldv, int layout_v, const void* Omega, long ldo, int layout_o);
/* Replaces nmfamd_engine_upload_sparse for arrays in device memory (format, a, b, base as there; a and b are 32-bit).  The pointer check covers nnz elements
 * (values), nnz ints (b) and nnz (COO) or outer + 1 ints (a); a null values / b is taken where nnz = 0.  Refusals, statuses and nmfamd_engine_last_error texts are
 * the host entry's word for word; its value rules (a dense divergence engine with beta > 0: finite and >= 0; missing_values: finite, at least one entry) are
 * evaluated by a kernel.  sparse_compute / missing_values engines copy the arrays device-to-device into arrays the image builder owns and build the CSR and CSC
 * images there (nmfamd_geometry.sparse_setup = 1); an input that builder hands back -- an entry outside the matrix, pointer arrays that do not ascend, a row or
 * column longer than 8192 entries, nnz = 0 -- and NMFAMD_SPARSE_SETUP=host cost a download of the arrays and take the host entry's path (sparse_setup = 0).  Every
 * other engine densifies the arrays where they lie.  The result equals the host entry's on the same values bit for bit (densifying engines: for unique
 * coordinates; three or more duplicates of one coordinate are added in no fixed order, there as here). */
NMFAMD_API int nmfamd_engine_upload_sparse_device(nmfamd_engine* e, int format, const void* values, const int* a, const int* b, long nnz, int base);
/* Dense V (m x n, layout and ld as for nmfamd_engine_upload_dense_device) in device memory on an engine with sparse_compute or missing_values -- the engines that
 * refuse nmfamd_engine_upload_dense_device; every other engine refuses this entry.  The stored entries are those of nmfamd_engine_upload_dense: with missing_values
 * every entry that is not NaN, zeros included (an infinite entry, and a V without an observed entry, are refused with the host entry's texts), otherwise every
 * entry != 0.  Both images are compacted on the device (count, scan, scatter: no limit on the length of a row or column; sparse_setup = 1) and equal the host
 * entry's bit for bit, as does everything computed from them. */
NMFAMD_API int nmfamd_engine_upload_dense_device_stored(nmfamd_engine* e, const void* V, long ld, int layout);
/* Replace nmfamd_engine_set_factors / _get_factors: W (m x r) and H (r x n) in device memory, each in its own layout; a null pointer leaves that factor (its ld and
 * layout are then not looked at).  set invalidates what nmfamd_engine_set_factors invalidates and writes exact zeros into the panels' padding; get returns what
 * nmfamd_engine_get_factors returns (nsNMF: W S) and writes the m x r / r x n block only -- bytes in the gap of ld stay as they are. */
NMFAMD_API int nmfamd_engine_set_factors_device(nmfamd_engine* e, const void* W, long ldw, int layout_w, const void* H, long ldh, int layout_h);
NMFAMD_API int nmfamd_engine_get_factors_device(nmfamd_engine* e, void* W, long ldw, int layout_w, void* H, long ldh, int layout_h);
/* No kernel, no engine: what the pointer check sees.  kind: 0 not known to the runtime (ordinary host memory, NULL), 1 device memory, 2 pinned host memory,
 * 3 anything else (managed, array); device: the HIP device it belongs to (-1 for kind 0); bytes_from_p: bytes from p to the end of its allocation (0 unless
 * kind = 1; an allocator that carves tensors out of larger blocks reports the block's end).  NMFAMD_NO_DEVICE without a HIP device. */
NMFAMD_API int nmfamd_device_pointer_info(const void* p, int* kind, int* device, unsigned long long* bytes_from_p);

/* ---- predict and score entries of W H (docs/PREDICT.md) ----------------------------------------
 * rows / cols: nnz >= 1 coordinates (i_p, j_p), 32-bit, index base 0 or 1, unsorted, duplicates counted once per copy.  W and H are what
 * nmfamd_engine_get_factors would return at this moment (nsNMF: W S; pending scales folded in), and the effects on the engine are exactly that call's: the factors
 * after iterate, predict, iterate equal those after iterate, get_factors, iterate bit for bit, and the error of the last error iteration stays as it was.
 *   predict: out[p] = sum_{k < r} W(i_p, k) H(k, j_p) in the engine's precision, no eps.
 *   score:   values v_p in the engine's precision; out may be NULL.  sums[0] = sum (v_p - out[p])^2, sums[1] = sum d_beta(v_p | out[p] + eps) (eps the machine
 *            epsilon of the precision; v^beta = 0 at v = 0; the KL form at beta = 1, Itakura-Saito at beta = 0, the general form elsewhere, beta = 2 included),
 *            sums[2] = the sum of the absolute values of the summands of d_beta (the scale of sums[1]'s rounding), sums[3] = sqrt(sums[0] / nnz).  beta <= 0 needs
 *            every value finite and > 0, beta > 0 finite and >= 0; beta = NaN: no divergence wanted -- any finite value, sums[1] = sums[2] = NaN.
 * Per-entry terms are formed in the engine's precision and added in double in a fixed order (16-lane group, workgroup, host): a repeated call is bit-identical,
 * and the host and the device form give the same bits.
 * NMFAMD_INVALID_ARGUMENT with nmfamd_engine_last_error, before any result is written: a coordinate outside [base, base + m) x [base, base + n) (the text names the
 * first such p; host arrays are checked on the host before any device work, device arrays by a validation launch that reads the index arrays only -- the gather is
 * not launched unless it found every coordinate inside), a value that breaks the rule, an engine created with row blocks > 1 or driven through the three-phase /
 * sharded entries (it holds a column shard), an engine whose factors were never set, nnz < 1, another base.
 * _device: every array in device memory, with the pointer check and the ordering of the entries above (sums stays a host array). */
NMFAMD_API int nmfamd_engine_predict(nmfamd_engine* e, const int* rows, const int* cols, long nnz, int base, void* out);
NMFAMD_API int nmfamd_engine_score(nmfamd_engine* e, const int* rows, const int* cols, const void* values, long nnz, int base, double beta, void* out_or_NULL,
                                   double sums[4]);
NMFAMD_API int nmfamd_engine_predict_device(nmfamd_engine* e, const int* rows, const int* cols, long nnz, int base, void* out);
NMFAMD_API int nmfamd_engine_score_device(nmfamd_engine* e, const int* rows, const int* cols, const void* values, long nnz, int base, double beta, void* out_or_NULL,
                                          double sums[4]);

/* ---- the k best candidates of W H per query (docs/TOPK.md) -------------------------------------
 * queries: nq >= 1 indices, 32-bit, index base 0 or 1, unsorted, duplicates allowed.  axis 0: a query is a row i of V and the candidates are the n columns,
 * s(i, j) = sum_{k < r} W(i, k) H(k, j); axis 1: a query is a column and the candidates are the m rows.  1 <= k <= nmfamd_top_k_max() (64).  W, H and the effects
 * on the engine as for nmfamd_engine_predict.  Scores in the engine's precision, no eps.
 * Per query the candidates are ordered by score descending, equal scores (numerically: -0 = +0) by ascending index; out_idx [nq][k] (int32, in the caller's base)
 * and out_scores [nq][k] hold the first k ELIGIBLE candidates in that order, and index -1 / score -inf in the remaining slots when fewer than k are eligible.
 * excl_ptr [nq + 1] (64-bit, excl_ptr[0] = 0, non-decreasing) and excl_idx [excl_ptr[nq]] (32-bit candidate indices in the caller's base; unsorted, duplicates
 * allowed), or both NULL: a candidate listed for query q is not eligible for q.
 * NMFAMD_INVALID_ARGUMENT with a last_error, before any device work, for the engines nmfamd_engine_predict refuses, nq < 1, k outside its range, another base or
 * axis, a malformed excl_ptr and a query or excluded index outside its range (the first bad one is named).
 * _device: every array in device memory, with the pointer check and the ordering of the entries above; excl_nnz is the extent of excl_idx and has to equal
 * excl_ptr[nq].  A validation launch reads the index arrays first; the product is not launched unless it found everything inside. */
NMFAMD_API int nmfamd_top_k_max(void);
NMFAMD_API int nmfamd_top_k_slabs(long nq, long count);   /* slices of the candidate range that one workgroup each walks: a function of the two numbers only */
NMFAMD_API int nmfamd_engine_top_k(nmfamd_engine* e, const int* queries, long nq, int k, int axis, int base, const long* excl_ptr, const int* excl_idx, int* out_idx,
                                   void* out_scores);
NMFAMD_API int nmfamd_engine_top_k_device(nmfamd_engine* e, const int* queries, long nq, int k, int axis, int base, const long* excl_ptr, const int* excl_idx,
                                          long excl_nnz, int* out_idx, void* out_scores);

/* Uniform (0,1] fill, the same seed for both factors (source/init/RandomValueStrategy.cpp:29-70). */
NMFAMD_API int nmfamd_engine_randomize(nmfamd_engine* e, unsigned seed, int w, int h);

/* `count` iterations of IAlgorithm::computeIteration (Algorithm.h:59).  Iterations are numbered
 * first_iteration, first_iteration+1, ...; the error is evaluated when the number is a multiple of
 * error_every (10 in the reference, SingleGpuDispatcher.h:37; 0 = never) or equals last_iteration
 * (0 = no such iteration).  Returns after the work has been ENQUEUED; the error terms of an error
 * iteration travel to the host asynchronously and nmfamd_engine_frobenius / _rmsd wait for them
 * (nmfgpu::compute reads them after every error iteration, like the reference's dispatcher). */
NMFAMD_API int nmfamd_engine_iterate(nmfamd_engine* e, int count, int first_iteration, int error_every, int last_iteration, int constant_w);
NMFAMD_API int nmfamd_engine_synchronize(nmfamd_engine* e);
/* HALS engines: the penalties of scikit-learn's coordinate descent, which then minimises
 *   1/2 ||V - W H||^2 + l1W ||W||_1 + l1H ||H||_1 + 1/2 l2W ||W||^2 + 1/2 l2H ||H||^2     (docs/HALS.md has the mapping from alpha_W, alpha_H, l1_ratio).
 * Dense divergence engines (divergence 2, 3, or 1 with dense_compute): the same four terms added to the divergence, by scikit-learn's solver="mu" -- each
 * half-step's denominator carries + l1 + l2 A before the power (docs/DIVERGENCE.md); nmfamd_engine_divergence keeps reporting the divergence alone.
 * Masked divergence engines (missing_values = 1 with nmfamd_params_v7.missing_divergence != 0; docs/MISSING.md): likewise, over the stored entries.
 * Valid any time between iterations (a regularisation path on one resident V); takes effect at the next nmfamd_engine_iterate.  While any of the four is
 * non-zero the column normalisation of W is skipped; all zeros restores the unpenalised iteration.  nmfamd_engine_frobenius / _rmsd keep reporting
 * ||V - W H||, not the penalised objective.  NMFAMD_INVALID_ARGUMENT (with nmfamd_engine_last_error) for a negative or non-finite value, and for a
 * non-zero value on any other engine. */
NMFAMD_API int nmfamd_engine_set_hals_penalties(nmfamd_engine* e, double l1W, double l1H, double l2W, double l2H);
/* HALS engines: accelerated HALS (Gillis & Glineur 2012; docs/HALS.md, "Inner sweeps").  The H step computes W^T W and W^T V once and applies its sweep sweeps_h
 * times in a row, the W step H H^T and V H^T once and its sweep sweeps_w times, each sweep from the result of the one before, in one launch; everything else
 * (penalties, normalisation, error reporting, constant W: the H step only) is as with one sweep.  1 ... 64 each; (1, 1), the default, is the plain iteration.
 * Valid any time between iterations; takes effect at the next nmfamd_engine_iterate.  NMFAMD_INVALID_ARGUMENT (with nmfamd_engine_last_error) for a count
 * outside 1 ... 64, and for a count other than 1 on any other engine. */
NMFAMD_API int nmfamd_engine_set_hals_sweeps(nmfamd_engine* e, int sweeps_h, int sweeps_w);
/* Missing-value engines under the Frobenius objective (missing_values = 1, missing_divergence = 0; docs/MISSING.md, "Coordinate descent"): the solver of the
 * iterations that follow.  solver 0, the default: the multiplicative update; it takes only the neutral extras (sweeps 1, penalties 0).  solver 1: coordinate
 * descent over the observed entries -- the H step solves every column of H against its own Gram matrix sum_{i in Omega_j} w_i w_i^T with sweeps_h HALS sweeps
 * (docs/HALS.md) and the penalties (l1_h, l2_h), the W step every row of W likewise with sweeps_w and (l1_w, l2_w), which minimises
 *   1/2 sum_Omega (v - W H)^2 + l1_w ||W||_1 + l1_h ||H||_1 + 1/2 l2_w ||W||^2 + 1/2 l2_h ||H||^2;
 * no normalisation; the reported error stays the direct residual sum over the observed entries for (W_{k-1}, H_k); constant W runs the H step only.  Rank <= 128.
 * Valid any time between iterations; takes effect at the next nmfamd_engine_iterate; no factor changes.  NMFAMD_INVALID_ARGUMENT (with nmfamd_engine_last_error)
 * on any other engine, for another solver, a count outside 1 ... 64, a negative or non-finite penalty, extras with solver 0, and solver 1 at a rank above 128.
 * nmfamd_engine_set_hals_penalties and nmfamd_engine_set_hals_sweeps keep refusing such an engine. */
/* The rule nmfamd_engine_set_missing_solver and nmfgpu::compute's "missingSolver" apply, without an engine or a device: NULL where an engine of elem_bytes (4 or 8)
 * and rank r with these missing_values / missing_divergence would take the setting, else the text of the refusal (a static string). */
NMFAMD_API const char* nmfamd_missing_solver_fault(double solver, double sweeps_h, double sweeps_w, double l1_w, double l1_h, double l2_w, double l2_h, int elem_bytes,
                                                   double missing_values, double missing_divergence, int r);
NMFAMD_API int nmfamd_engine_set_missing_solver(nmfamd_engine* e, int solver, int sweeps_h, int sweeps_w, double l1_w, double l1_h, double l2_w, double l2_h);
/* HALS engines: per-column dynamic stopping of the inner sweeps (docs/HALS.md, "Dynamic stopping").  With delta in (0, 1) the counts of
 * nmfamd_engine_set_hals_sweeps become maximum counts: within one step a column of the swept panel is frozen after its sweep t when the squared step of that
 * sweep is at most delta^2 times the squared step of its first sweep, and is not stepped again.  0, the default, runs the static counts, bit for bit.  Valid any
 * time between iterations; takes effect at the next nmfamd_engine_iterate.  NMFAMD_INVALID_ARGUMENT (with nmfamd_engine_last_error) for a negative or
 * non-finite value, for a value of 1 or more, and for a non-zero value on any other engine. */
NMFAMD_API int nmfamd_engine_set_hals_sweep_tolerance(nmfamd_engine* e, double delta);
/* HALS engines: the sweeps applied to each column of H (which = 0: n entries) or row of W (which = 1: m entries) by the most recent step of that factor, 1 ...
 * the maximum count (the maximum itself for every entry while the tolerance is 0).  Synchronises.  Returns the number of entries copied, or a negative value: on
 * an engine of another algorithm, for another `which`, for capacity below n (m), and before any step of that factor -- with constant W no W step runs, so
 * which = 1 keeps returning what it returned before. */
NMFAMD_API long nmfamd_engine_hals_sweep_counts(nmfamd_engine* e, int which, int* out, long capacity);
/* NeNMF engines (docs/NENMF.md): the H step computes W^T W and W^T V once and takes steps_h accelerated projected-gradient steps
 *   H <- max(0, Y - (W^T W Y + l2H Y - W^T V + l1H) / L),  L = ||W^T W||_inf + l2H,  followed by Nesterov's extrapolation of Y,
 * in one launch, the W step steps_w of them against H H^T and V H^T; everything else (penalties through nmfamd_engine_set_hals_penalties, normalisation, error
 * reporting, constant W: the H step only) is as on a HALS engine.  1 ... 256 each; a new engine has (8, 8).  Valid any time between iterations; takes effect at
 * the next nmfamd_engine_iterate.  NMFAMD_INVALID_ARGUMENT (with nmfamd_engine_last_error) for a count outside 1 ... 256, and on any other engine.  On a NeNMF
 * engine nmfamd_engine_set_hals_sweeps refuses a count other than 1 and nmfamd_engine_set_hals_sweep_tolerance a value other than 0. */
NMFAMD_API int nmfamd_engine_set_nenmf_steps(nmfamd_engine* e, int steps_h, int steps_w);
/* NeNMF engines: per-column dynamic stopping of the projected-gradient steps (docs/NENMF.md, "Dynamic stopping").  With delta in (0, 1) the counts of
 * nmfamd_engine_set_nenmf_steps become maximum counts: within one step launch a column of the panel is frozen after its step t when |P_{t+1} - Y_t|^2 of that
 * column is at most delta^2 times that of its first step, keeps P_{t+1} and is not stepped again.  0, the default, runs the static counts, bit for bit.  Valid any
 * time between iterations; takes effect at the next nmfamd_engine_iterate.  NMFAMD_INVALID_ARGUMENT (with nmfamd_engine_last_error) for a negative or
 * non-finite value, for a value of 1 or more, and for any value on an engine of another algorithm. */
NMFAMD_API int nmfamd_engine_set_nenmf_step_tolerance(nmfamd_engine* e, double delta);
/* NeNMF engines: the steps applied to each column of H (which = 0: n entries) or row of W (which = 1: m entries) by the most recent step launch of that factor,
 * 1 ... the maximum count (the maximum itself for every entry while the tolerance is 0; 0 for every entry where L admitted no step).  Synchronises.  Returns the
 * number of entries copied, or a negative value: on an engine of another algorithm, for another `which`, for capacity below n (m), and before any step of that
 * factor -- with constant W no W step runs, so which = 1 keeps returning what it returned before. */
NMFAMD_API long nmfamd_engine_nenmf_step_counts(nmfamd_engine* e, int which, int* out, long capacity);
/* Frobenius norm / RMSD of the most recent error iteration (IAlgorithm::frobeniusNorm / rmsd). */
NMFAMD_API double nmfamd_engine_frobenius(nmfamd_engine* e);
NMFAMD_API double nmfamd_engine_rmsd(nmfamd_engine* e);
/* Generalised KL divergence D(V || W H) of the most recent error iteration (divergence = 1 only). */
NMFAMD_API double nmfamd_engine_kl_divergence(nmfamd_engine* e);
/* The objective of whichever divergence the engine has, of the most recent error iteration: the generalised KL divergence (divergence = 1, sparse or dense: equal to
 * nmfamd_engine_kl_divergence), the Itakura-Saito divergence sum (v / p - log(v / p) - 1), p = (W H) + eps (divergence = 2), or the beta-divergence
 * sum (v^beta + (beta - 1) p^beta - beta v p^(beta - 1)) / (beta (beta - 1)) with v^beta = 0 at v = 0 (divergence = 3).  The divergence alone: no penalty terms. */
NMFAMD_API double nmfamd_engine_divergence(nmfamd_engine* e);

/* Dominant-kernel timing.  enable = k > 0: every launch of the factor-product kernel (the two
 * products against V, reference: gemm TN / NT at AlgorithmMultiplicativeFrobenius.h:187-188,240-241)
 * in every k-th iteration is bracketed by HIP events on the engine's stream (k = 1: all launches;
 * an event pair costs a few microseconds of stream time, so the harness samples).  enable = 0: off.
 * _read synchronises, returns the summed duration and the number of launches timed since the last
 * read, and resets the counters. */
NMFAMD_API int nmfamd_engine_kernel_timing(nmfamd_engine* e, int enable);
NMFAMD_API int nmfamd_engine_kernel_timing_read(nmfamd_engine* e, double* total_ms, long* launches);
/* The same, plus what an EMPTY event pair reports on the idle stream (ms): the share of each sample that is not kernel time. */
NMFAMD_API int nmfamd_engine_kernel_timing_read2(nmfamd_engine* e, double* total_ms, long* launches, double* pair_overhead_ms);
/* ... and split by product: kind_ms[2] / kind_launches[2] = {H-side product (W^T V; y-tiled form when one image of V is resident), W-side product (V H^T)} */
NMFAMD_API int nmfamd_engine_kernel_timing_read3(nmfamd_engine* e, double* total_ms, long* launches, double* pair_overhead_ms, double* kind_ms, long* kind_launches);

/* Geometry the harness needs for its roofline arithmetic. */
typedef struct nmfamd_geometry {
	int m, n, r;
	int padded_rank;       /* RP: factor rows as stored and multiplied */
	long padded_m, padded_n;
	int slabs_h, slabs_w;  /* split-K slices of the two factor products */
	long exchange_count;   /* elements of the multi-GPU exchange buffer */
	int product_kernel;    /* 0 fp32 MFMA, 1 bf16-rounded operands, 2 fp32 by exact 3 x bf16 operand splitting, 3 fp64 MFMA,
	                          4 VALU kernel (NMFAMD_FORCE_VALU), 5 sparse SpMM, 6 the fused dense beta-divergence half-step (kernels_beta.hip: slabs_h / slabs_w
	                          are then the reduction slabs of its two launches, which fix the summation order; resident_images = 2, or 4 on a weighted engine;
	                          kl_blocks_* = 0), 7 the same half-step with bf16 operands (nmfamd_params_v5.mixed_precision, kernels_beta_bf16.hip; resident_images = 2) */
	int resident_images;   /* dense images of V kept in HBM: 2 (V and V^T, each streamed along its output index), 1 (only V: W^T V
	                          reads it along the reduction index; chosen when two would not fit, or by NMFAMD_ONE_IMAGE), 0 sparse, 4 a weighted dense divergence
	                          engine (V, the weights and the transposes of both) */
	int one_pass;          /* rank-64 multiplicative update: 1 = V is streamed ONCE per iteration (W^T V, the H update and V H^T in one
	                          persistent launch, kernels_onepass.hip; the MEASUREMENT build only since round 6: NMFAMD_ONE_PASS=1 there); 0 = two passes; 2 = a one-pass launch
	                          gave up (it could not keep its workgroups resident) and the engine reported the error */
	/* round 5: the counts that fix the ORDER of partial sums (and so the bits of a result), so that a run can be reproduced: all of them functions of the
	 * shape and of the device's properties only (never of what else occupies the device) */
	int kl_blocks_w, kl_blocks_h;   /* KL update: L2-sized blocks the gathered factor is cut into (1 = unblocked; 0 = not the KL update) */
	int gram_k_slices;              /* rank-64 multiplicative update: K slices of the W^T W passengers (1, 2, 4, 8), or 16: the ten tiles' K ranges dealt evenly
	                                   to the sixteen passengers of a whole problem's W^T V launch (up to three pieces per tile, added in order) */
	int w_col_split;                /* 1: V H^T runs as 128 x 32 workgroups (narrow column shards) */
	/* round 6 */
	int fused_launches;             /* 4: an iteration is product (+ Gram passengers) / update / product (+ Gram passengers) / update -- fp32 at padded rank 64
	                                   (multiplicative update; nsNMF on the split-operand products) and, round 6, double precision (multiplicative update and nsNMF,
	                                   padded ranks up to 512); 8: fp32 at padded ranks 128 ... 512 (Gram slices, reduction + split image + scale, product, update --
	                                   twice; the generic sequence: 14), 7 or 6 where the Gram slices of a side ride its product launch; 0: the generic launch sequence */
	int sparse_setup;               /* sparse compute: where the CSR + CSC images of the last upload were built: 1 = on the device (kernels_sparse_setup.hip),
	                                   0 = on the host (NMFAMD_SPARSE_SETUP=host, or an input the device path hands back: entries outside the matrix, a row or
	                                   column of more than 8 192 entries, pointer arrays that do not ascend), -1 = not a sparse-compute engine */
	int gram_ride_slices_h, gram_ride_slices_w;   /* K slices per super-block of the Gram passengers riding in W^T V / V H^T -- double precision (64 x 64 super-blocks) and
	                                                 fp32 at padded ranks 128 ... 512 (128 x 128; 0: the slices are a launch of their own); they fix the order of the partial sums */
} nmfamd_geometry;
NMFAMD_API int nmfamd_engine_geometry(const nmfamd_engine* e, nmfamd_geometry* out);
/* The same for a caller compiled against an older (shorter) or newer (longer) nmfamd_geometry: writes min(struct_size, sizeof(nmfamd_geometry)) bytes, never
 * past the caller's struct (the struct only ever grows at its end; round 3 added `one_pass`, round 5 the four counts behind it, round 6 three more).  Returns NMFAMD_INVALID_ARGUMENT for struct_size < 8. */
NMFAMD_API int nmfamd_engine_geometry_sized(const nmfamd_engine* e, void* out, unsigned long struct_size);
/* The geometry an engine created with these arguments would report on a device with num_cus compute units, a memory-side cache (AMD Infinity Cache) of
 * memory_side_cache_bytes (0: none known) and free_bytes of free memory, WITHOUT a device: it runs the parameter checks and the planning step of engine creation --
 * the step that fixes the kernel path and the order of every partial sum, from the shape, the parameters, these three numbers and the environment switches -- and
 * allocates nothing (no HIP call; works in a process on a machine without a GPU).  params_sized / params_size, elem_bytes and row_blocks as for
 * nmfamd_engine_create_v2; geometry_out / struct_size as for nmfamd_engine_geometry_sized.  kl_blocks_* and sparse_setup depend on an upload: they are those of a
 * freshly created engine.  Where creation would refuse the arguments this returns the same status, with the reason in nmfamd_engine_last_error(NULL). */
NMFAMD_API int nmfamd_plan_geometry(int m, int n, int r, int algorithm, const void* params_sized, unsigned long params_size, int elem_bytes, int row_blocks,
                                    int num_cus, unsigned long long memory_side_cache_bytes, unsigned long long free_bytes, void* geometry_out, unsigned long struct_size);

/* ---- column-sharded multi-GPU form of the multiplicative update ------------------------------
 * Rank g holds V(:, J_g), H(:, J_g) and a full replica of W.  Per iteration:
 *     nmfamd_engine_h_step        local: H(:, J_g) update, no communication
 *     nmfamd_engine_w_products    local: exchange <- [ (V_g H_g^T)^T panel | H_g H_g^T ]
 *     <all-reduce(sum) of `exchange` across ranks -- RCCL, done by the caller>
 *     nmfamd_engine_w_finish      replicated: W update + column normalisation from the reduced sums
 * `exchange` is a DEVICE pointer to exchange_count elements owned by the caller (so that the
 * collective library can register it).  On error iterations h_step / w_finish leave the local
 * error terms on the host: n_local per-column terms of tr(H^T W^T V), r terms of
 * tr(H H^T W^T W) computed from the REDUCED H H^T, and the sorted local tr(V^T V) terms. */
NMFAMD_API int nmfamd_engine_h_step(nmfamd_engine* e, int compute_error);
NMFAMD_API int nmfamd_engine_w_products(nmfamd_engine* e, void* exchange);
NMFAMD_API int nmfamd_engine_w_finish(nmfamd_engine* e, const void* exchange, int compute_error);
/* A caller that drives the three phases for a team of ONE rank (no reduction between w_products and w_finish: `exchange` reaches w_finish as w_products
 * left it) may say so: the engine then skips work that only a reduced buffer needs (rank 256 / bf16: re-splitting H H^T).  sole != 0 is a promise. */
NMFAMD_API int nmfamd_engine_set_sole_rank(nmfamd_engine* e, int sole);
/* Row-block form of nmfamd_engine_w_finish for callers that reduce-scatter the panel themselves (the torch-facing wrapper
 * nmfgpu_amd/distributed.py; the native loop nmfamd_sharded_* does the same inside the library): num_rows = the reduced
 * (V H^T)^T rows [row0, row0 + rows) in panel layout (DEVICE), hht = the reduced H H^T (DEVICE, padded_rank^2), colsq =
 * padded_rank DEVICE elements that receive the sums of squares of the new rows.  After the all-reduce of colsq:
 * _w_normalize_rows; after the all-gather of every rank's rows into nmfamd_engine_w_panel(): _w_rows_replaced.
 * rows and row0 are multiples of 128 (engine created with nmfamd_engine_create_blocks). */
NMFAMD_API int nmfamd_engine_w_update_rows(nmfamd_engine* e, const void* num_rows, const void* hht, long row0, long rows, int compute_error, void* colsq);
NMFAMD_API int nmfamd_engine_w_normalize_rows(nmfamd_engine* e, long row0, long rows, void* colsq);
NMFAMD_API int nmfamd_engine_w_rows_replaced(nmfamd_engine* e);
NMFAMD_API void* nmfamd_engine_w_panel(nmfamd_engine* e);     /* DEVICE pointer: padded_m rows of padded_rank elements */
/* which: 0 = sorted tr(V^T V) terms (n), 1 = tr(H^T W^T V) terms (n), 2 = tr(H H^T W^T W) terms (r).
 * Returns the number of elements copied (<= capacity), negative on error. */
NMFAMD_API long nmfamd_engine_error_terms(nmfamd_engine* e, int which, void* out, long capacity);
/* Stream-ordered form for callers that must not stall the stream on error iterations: copies the n_local
 * tr(H^T W^T V) terms followed by the r tr(H H^T W^T W) terms of the last error iteration into the DEVICE buffer
 * `dst` (device-to-device, asynchronous on the engine's stream).  Returns n_local + r, negative on error. */
NMFAMD_API long nmfamd_engine_error_terms_to_device(nmfamd_engine* e, void* dst_device, long capacity);
/* The host half of the error evaluation (source/nmf/FrobeniusResolver.cpp:29-51) on caller-supplied
 * term vectors (the two latter ones are sorted in place). */
NMFAMD_API double nmfamd_resolve_frobenius_f32(const float* vtv_sorted, long n_vtv, float* htwtv, long n_htwtv, float* hhtwtw, long n_hhtwtw);
NMFAMD_API double nmfamd_resolve_frobenius_f64(const double* vtv_sorted, long n_vtv, double* htwtv, long n_htwtv, double* hhtwtw, long n_hhtwtw);

/* ---- the same sharded iteration driven natively (no torch in the loop) -------------------------------------------
 * A communicator is one rank of an RCCL clique, created through RCCL's C API (librccl.so is loaded on first use):
 * rank 0 obtains 128 bytes of unique id, hands them to the other ranks by whatever means the caller has (bench.py:
 * torch.distributed's store; nmfgpu::compute with Parameter "numGpus": threads of one process share it directly), and every
 * rank calls nmfamd_comm_create_rccl with ITS HIP device current -- the call blocks until all `world` ranks have arrived.
 * A sharded run binds one engine (created with nmfamd_engine_create_blocks(..., row_blocks = world)) to one communicator:
 *   mode 0  reduce-scatter of (V H^T)^T by row blocks of W + all-reduce of H H^T -> every rank updates its m / world rows
 *           -> all-reduce of the r column sums of squares -> normalise -> all-gather of the row blocks   
 *   mode 1  one all-reduce of the whole exchange buffer, identical W update on every rank
 * rows / total_columns: shape of the WHOLE matrix; this rank's engine holds the columns
 * [total_columns * rank / world, total_columns * (rank + 1) / world).  nmfamd_sharded_iterate numbers iterations like
 * nmfamd_engine_iterate and only ENQUEUES work; _frobenius / _rmsd wait for the gathered error terms of the most recent
 * error iteration and run the reference's sorted host summation on them (FrobeniusResolver.cpp:29-51). */
typedef struct nmfamd_comm nmfamd_comm;
typedef struct nmfamd_sharded nmfamd_sharded;
NMFAMD_API int nmfamd_comm_rccl_available(void);
NMFAMD_API int nmfamd_comm_unique_id(void* out_128_bytes);
NMFAMD_API int nmfamd_comm_create_rccl(const void* id_128_bytes, int world, int rank, nmfamd_comm** out);
NMFAMD_API void nmfamd_comm_destroy(nmfamd_comm* c);
/* The in-process transport (csrc/comm.h, LocalComm): the ranks are THREADS of one process, each with its own HIP device current (the same device, or
 * peer-mapped devices of one node); every rank's kernels read the peers' buffers where they lie -- over xGMI when the devices differ.  This is the
 * transport of nmfgpu::compute with Parameter "numGpus" when RCCL is not used, and the one whose multiplicative update needs no reduction kernel at
 * all (replicated mode at padded rank 64: the W update adds the ranks' exchange panels in its prologue, two buffers alternate, one rendezvous per
 * iteration).  One thread creates the group, every rank thread calls nmfamd_comm_create_local (blocks until all `world` ranks have joined; fails on
 * every rank when two devices cannot map each other's memory).  nmfamd_local_group_abort makes every rank waiting in a collective return an error. */
typedef struct nmfamd_local_group nmfamd_local_group;
NMFAMD_API int nmfamd_local_group_create(int world, nmfamd_local_group** out);
NMFAMD_API void nmfamd_local_group_destroy(nmfamd_local_group* g);
NMFAMD_API void nmfamd_local_group_abort(nmfamd_local_group* g);
NMFAMD_API int nmfamd_comm_create_local(nmfamd_local_group* g, int rank, nmfamd_comm** out);
/* why nmfamd_comm_create_local failed: names the pair of devices that cannot map each other's memory (valid until the calling thread's next call) */
NMFAMD_API const char* nmfamd_local_group_last_error(nmfamd_local_group* g);
/* Set-up self-test of the in-process transport (run by nmfamd_comm_create_local when world > 1; NMFAMD_SELFTEST=0 skips it): every rank publishes a pattern in
 * both exchange slots and in a collective's buffer, every rank reads every peer's through the kernels the iteration uses (the W update's prologue, the r x r
 * sum, the reduce / gather kernels) and checks every word; then a second pattern at the SAME addresses.  A mismatch fails nmfamd_comm_create_local on every
 * rank and names the (reader, owner) pair in nmfamd_local_group_last_error.  One line about the test (empty before it ran; valid until the thread's next call).
 * Lifetime rules of the transport: the exchange buffers belong to the GROUP and live until every rank has closed its communicator; closing a communicator
 * (nmfamd_comm_destroy) first drains the rank's device, so that no kernel of this rank still reads a peer's buffer. */
NMFAMD_API const char* nmfamd_local_group_selftest(nmfamd_local_group* g);
/* "rccl" / "in-process (peer reads)" */
NMFAMD_API const char* nmfamd_comm_transport(const nmfamd_comm* c);
/* nmfamd_engine_create with the padded row count rounded up to a multiple of 128 * row_blocks (equal row blocks of W) */
NMFAMD_API int nmfamd_engine_create_blocks(int m, int n, int r, int algorithm, const nmfamd_params* params, int elem_bytes, void* stream,
                                           int row_blocks, nmfamd_engine** out);
NMFAMD_API int nmfamd_sharded_create(nmfamd_engine* e, nmfamd_comm* c, int mode, long rows, long total_columns, nmfamd_sharded** out);
NMFAMD_API void nmfamd_sharded_destroy(nmfamd_sharded* s);
NMFAMD_API int nmfamd_sharded_iterate(nmfamd_sharded* s, int count, int first_iteration, int error_every, int last_iteration);
/* Row-block mode at padded rank 256 with bf16 operands (config 4): between two W updates the ranks exchange the bf16 fragments of their row blocks only, so
 * the fp32 rows of the OTHER ranks' blocks in nmfamd_engine_w_panel() are those of an earlier iteration until they are gathered.  They are gathered
 *   (a) by nmfamd_sharded_iterate itself when a batch ends on its last_iteration (> 0), and
 *   (b) by this call -- a COLLECTIVE: every rank of the communicator must make it, at the same point of its stream.
 * nmfamd_engine_get_factors on an engine whose rows are still stale gathers them through the live sharded run (then it, too, is a collective that every rank must
 * make); after nmfamd_sharded_destroy it fails with NMFAMD_INVALID_ARGUMENT rather than hand out stale rows.  A no-op in every other mode. */
NMFAMD_API int nmfamd_sharded_gather_w(nmfamd_sharded* s);
NMFAMD_API double nmfamd_sharded_frobenius(nmfamd_sharded* s);
NMFAMD_API double nmfamd_sharded_rmsd(nmfamd_sharded* s);
NMFAMD_API const char* nmfamd_sharded_last_error(const nmfamd_sharded* s);

/* The host-side initialisers (run once per run, before the iteration loop; host memory only, no device or
 * context needed).  k-means: Lloyd with a Forgy start (source/kmeans/kMeans.cu:126-278); data is m x n with
 * leading dimension ld, clusters m x k (ldc), membership n entries; *iterations receives the passes done.
 * host_init: method is the NmfInitializationMethod value (include/nmfgpu.h:87-96) for MeanColumns,
 * KMeans* and EInNMF (source/init/KMeansStrategy.cpp:31-65, EInNMF.cu:44-119); W is m x r (ld m), H r x n
 * (ld r) or NULL.  method 100 / 101 / 102: the SVD-based start NNDSVD / NNDSVDa / NNDSVDar (Boutsidis & Gallopoulos 2008; not in the reference -- BASELINE's
 * north star names it -- nmfgpu::compute selects it with Parameter{"nndsvd", 0 | 1 | 2}, which overrides initMethod): truncated SVD of V by block subspace
 * iteration on the host, in double.  Return 0, or 1 (invalid argument) for arguments the reference rejects. */
NMFAMD_API int nmfamd_host_kmeans_f32(const float* data, long ld, int m, int n, float* clusters, long ldc, int k,
                                      unsigned* membership, unsigned seed, unsigned maxiter, double threshold, unsigned* iterations);
NMFAMD_API int nmfamd_host_kmeans_f64(const double* data, long ld, int m, int n, double* clusters, long ldc, int k,
                                      unsigned* membership, unsigned seed, unsigned maxiter, double threshold, unsigned* iterations);
NMFAMD_API int nmfamd_host_init_f32(const float* V, long ldv, int m, int n, int r, int method, unsigned seed, float* W, float* H);
NMFAMD_API int nmfamd_host_init_f64(const double* V, long ldv, int m, int n, int r, int method, unsigned seed, double* W, double* H);

/* ---- single operations on host data (parity tests of the individual kernels) -----------------
 * OUT (r x X) = F (r x Y) * A^T, A is X x Y: the factor product both big GEMMs are instances of.
 * out_slabs (optional) receives the number of split-K slabs the MFMA kernel used.
 * use_valu != 0 selects the generic VALU kernel (the cross-check) instead of the fp32 / fp64 MFMA kernel. */
NMFAMD_API int nmfamd_op_factor_product_f32(const float* A, long lda, int X, int Y, const float* F, long ldf, int r,
                                            float* OUT, long ldo, int use_valu, int* out_slabs);
NMFAMD_API int nmfamd_op_factor_product_f64(const double* A, long lda, int X, int Y, const double* F, long ldf, int r,
                                            double* OUT, long ldo, int use_valu, int* out_slabs);
/* Tuning / diagnosis of the factor-product kernel (rank 64) on synthetic device data: average of
 * `reps` back-to-back launches; optionally (stamps_out != NULL) one launch of the diagnostic build that
 * records 8 uint64 per wave: shader clock at entry / first MFMA / loop end / kernel end, 100 MHz
 * real-time counter at entry / end, K-steps, XCC id. */
NMFAMD_API int nmfamd_tune_factor_product(int X, int Y, int reps, double* avg_us, unsigned long long* stamps_out, long stamps_capacity, long* stamps_count);
/* The same product with bf16-rounded operands (v_mfma_f32_32x32x16_bf16, fp32 accumulation), r <= 64. */
NMFAMD_API int nmfamd_op_factor_product_bf16(const float* A, long lda, int X, int Y, const float* F, long ldf, int r, float* OUT, long ldo);
/* The same product at fp32 accuracy on the bf16 matrix pipe: both operands split exactly into three bf16 terms, six
 * cross products, fp32 accumulation (kernels_x3.hip), any r.  reps > 0 additionally times `reps` launches of the
 * product kernel alone (HIP events) into *avg_us. */
NMFAMD_API int nmfamd_op_factor_product_x3(const float* A, long lda, int X, int Y, const float* F, long ldf, int r, float* OUT, long ldo,
                                           int reps, double* avg_us);
/* The same with A stored tiled along the REDUCTION index y (the image the other product of an iteration streams along its
 * output index): one resident image of V serves both products. */
NMFAMD_API int nmfamd_op_factor_product_x3_ytiled(const float* A, long lda, int X, int Y, const float* F, long ldf, int r, float* OUT, long ldo,
                                                  int reps, double* avg_us);
/* Diagnostic (NMFAMD_X3_VARIANT = 10..13 builds): per wave {shader cycles, 100 MHz ticks, K-steps of the main loop; 100 MHz
 * stamps at entry, loop start, loop end, tail end, exit; at the first operand split (the first K-step's rows are there), at the end of an odd piece's first K-step
 * (0: whole turns), at the first MFMA group of the loop's first turn; one unused word} = 12 words per wave of one more launch; stamps_capacity in 8-byte words;
 * *waves receives the number of waves stamped. */
NMFAMD_API int nmfamd_tune_factor_product_x3(int X, int Y, unsigned long long* stamps_out, long stamps_capacity, long* waves);
/* G (r x r) = P P^T for a host r x len matrix P. */
NMFAMD_API int nmfamd_op_gram_f32(const float* P, long ldp, int r, int len, float* G, long ldg);
NMFAMD_API int nmfamd_op_gram_f64(const double* P, long ldp, int r, int len, double* G, long ldg);
/* Ainv = (A + regulariser)^-1 for a host r x r matrix (offdiag / diag added as KernelFillMatrix.cu:29-45). */
NMFAMD_API int nmfamd_op_inverse_f32(const float* A, long lda, int r, float offdiag, float diag, float* Ainv, long ldi);
/* Test entry of the same inverse on every route that launches it (docs/INVERSE.md).  route 0: launch_inverse_small as the engines call it (Gauss-Jordan up to r = 64,
 * Householder QR above); 1: the Householder route at any r; 2 / 3 (float, r <= 64): the Gauss-Jordan body as the passenger workgroup of the product launch that
 * nmfamd_op_factor_product_f32 / nmfamd_op_factor_product_x3 make of A_prod (X x Y, column-major), F_prod (64 x Y) and OUT (64 x X) -- NULL / 0 on routes 0 and 1.
 * Ainv_full: RP x RP (RP = the padded rank, returned in *rp_out: 64 up to r = 64, then the next multiple of 128 in float and of 64 in double), copied to the device
 * before the launch and back whole after it.  A_after (RP x RP, or NULL): the device image of A starts as this array with the r x r block of A on top and is copied
 * back as the launch left it.  NMFAMD_INVALID_ARGUMENT, with no output touched, for routes 2 and 3 in double or at r > 64 and wherever a launcher refuses
 * (the fp32 MFMA product carries a passenger from 16 x-tiles on). */
NMFAMD_API int nmfamd_op_inverse_ex_f32(const float* A, long lda, int r, float offdiag, float diag, int route, float* Ainv_full, float* A_after, int* rp_out,
                                        const float* A_prod, long lda_prod, int X, int Y, const float* F_prod, long ldf_prod, float* OUT, long ldo);
NMFAMD_API int nmfamd_op_inverse_ex_f64(const double* A, long lda, int r, double offdiag, double diag, int route, double* Ainv_full, double* A_after, int* rp_out,
                                        const float* A_prod, long lda_prod, int X, int Y, const float* F_prod, long ldf_prod, float* OUT, long ldo);
/* Test entry of the rank-64 Gram matrix from the split image of a panel (docs/GRAM.md): one launch at a time, every input caller-built, every output buffer uploaded as
 * the caller filled it and copied back whole.  P: [len][64] panel rows (NULL: no image, which the launcher refuses); colsq_part: [colsq_parts][64] partial sums of squares
 * or NULL; normalize, ksplit, spread: GramReduceArgs' fields as given; finish: the spread form with spread_out and the counter word.  ride 0: launch_gram_image_args;
 * 1 / 2: as passenger workgroups of the x-tiled / y-tiled split-operand product of A_prod (X x Y, column-major) and F_prod (64 x Y) over the 16-row image, whose result
 * goes to OUT_ride (64 x X) and, from a launch without passengers, to OUT_plain.  3: of the x-tiled product over 128-row tiles with FactorProductPlan::col_split = 2
 * (128 x 32 workgroups, one slab: a narrow column shard's V H^T).  `launches` (1 ... 4) launches in a row share G, scale and the counter; launch i finishes
 * into spread_out + 4096 i.  G: g_elems floats (4096 per slice or piece).  counter[0]: the counter word before the first launch; counter[1 + i]: after launch i.
 * plan[6]: matrices the form writes into G, passenger workgroups, pairs of K-steps, K-steps of the image, x-tiles and K slices of the product.
 * NMFAMD_INVALID_ARGUMENT wherever a launcher refuses. */
NMFAMD_API int nmfamd_op_gram_image_f32(const float* P, int len, const float* colsq_part, int colsq_parts, int normalize, int ksplit, int spread, int finish, int ride,
                                        int launches, float* G, long g_elems, float* scale, float* spread_out, unsigned* counter, int* plan,
                                        const float* A_prod, long lda_prod, int X, int Y, const float* F_prod, long ldf_prod, float* OUT_plain, float* OUT_ride, long ldo);
/* Test entry of the rank-64 Gram matrix from partial 64 x 64 matrices (docs/GRAM.md).  route 0: launch_mu64_gram_partials (P [len_pad][64] -> partials, one matrix per
 * 64 panel rows, parts = len_pad / 64); 1: launch_mu64_gram_reduce; 2: the same reduction as the passenger workgroups of the split-operand product of A_prod and F_prod
 * (as nmfamd_op_gram_image_f32, ride 1), 6: the same on the col_split product launch (ride 3); 3: launch_gram64_from_partials (scale NULL: the sum alone); 4: launch_gram64_normalize_all; 5: launch_gram64_reduce_scale_all
 * (sumsq_part: [sq_parts][64]).  Routes 4 and 5 scale the panel P in place and write x3_ks K-steps of its split image into x3 (the image of len_pad / 16 + 1 K-steps).
 * Buffers a route does not use may be NULL. */
NMFAMD_API int nmfamd_op_gram64_partials_f32(int route, float* P, int len_pad, float* partials, int parts, int normalize, const float* sumsq_part, int sq_parts,
                                             float* Graw, float* G, float* scale, void* x3, int x3_ks,
                                             const float* A_prod, long lda_prod, int X, int Y, const float* F_prod, long ldf_prod, float* OUT_plain, float* OUT_ride, long ldo);
/* Test entry of the fp32 Gram matrix at padded ranks 128 ... 512 (docs/GRAM.md).  route 0: launch_gram_wide_f32; 1: launch_gram_wide_fused_f32; 2: launch_gram_reduce_x3
 * alone on the caller's slices; 3: the slices as passenger workgroups of the x-tiled split-operand product of A_prod (X x Y) and F_prod (r_prod x Y) over the 16-row image,
 * for the slice count of route 1.  P: [len][RP] panel rows; partial: part_elems floats ([slices][RP][RP]); G: [RP][RP]; qx3: the split image of G (RP / 16 + 1 K-steps);
 * sumsq_part: [sq_parts][RP] or NULL; scale_out: [RP].  plan[0]: the slice count the launcher settled on. */
NMFAMD_API int nmfamd_op_gram_wide_f32(int route, const float* P, int RP, int len, int parts, float* partial, long part_elems, float* G, void* qx3, const float* sumsq_part,
                                       int sq_parts, float* scale_out, int* plan,
                                       const float* A_prod, long lda_prod, int X, int Y, const float* F_prod, long ldf_prod, int r_prod, float* OUT_plain, float* OUT_ride, long ldo);
/* The passes between the update of a factor panel and the next product at padded rank 256 with bf16 product operands (129 <= r <= 256):
 * optional column normalisation (colsq: r sums of squares or NULL), nsNMF smoothing by theta, bf16 rounding; the Gram matrix of the panel and of
 * the smoothed panel.  P, P_out, pack_out: [len][ldp / r] rows of r values; G_raw, G_smooth: [r][r].  Outputs may be NULL. */
NMFAMD_API int nmfamd_op_factor_passes_f32(const float* P, long ldp, int r, int len, const float* colsq, float theta, float* P_out, float* pack_out,
                                           float* G_raw, float* G_smooth, int reps, double* avg_us_finish, double* avg_us_gram);
/* One multiplicative update of a panel (129 <= r <= 256) as the bf16 path at padded rank 256 runs it (csrc/kernels.h, PanelTriExtras).  A pending column
 * scale is given as the sums of squares it comes from: d(c) = s[c] > 0 ? 1 / sqrt(s[c]) : 1; S = (1 - theta) I + (theta / r) 1 1^T.
 *   old'(y, c) = P(y, c) * d_old(c)                                       (old_colsq NULL: ones)
 *   num'(y, :) = S (d_num .* num(y, :))                                    (transform_num != 0; num_colsq NULL: ones)
 *   den(y, :)  = old'(y, :) Q + eps,  or  S D_num Q D_num S old'(y, :) + eps when transform_den != 0
 *   P_out = old' .* num' ./ den                                            (unnormalised)
 *   pack_out = bf16 of P_out as written for the next product, smoothed by frag_theta first when that is not 0
 *   scale_out(c) = d of the columns of P_out, gram_out = diag(scale) pack^T pack diag(scale);
 *   gram_raw_out = pack^T pack, gram_image_out = the same matrix read back from the split image the reduction writes beside it, diag_out = its diagonal.
 * Row-major [len][r] and [r][r]; outputs may be NULL. */
NMFAMD_API int nmfamd_op_tri_update_f32(const float* P, const float* num, const float* Q, int r, int len, const float* old_colsq, int transform_num,
                                        const float* num_colsq, float theta, float frag_theta, int transform_den, float* P_out, float* pack_out,
                                        float* scale_out, float* gram_out, float* gram_raw_out, float* gram_image_out, float* diag_out);
/* One launch of the HALS sweep (kernels_hals.hip) on host arrays in panel layout, for tests: P [len_pad][RP] (updated in place), S slabs of
 * [len_pad][RP] at slab_stride >= len_pad * RP elements (the gaps between them are not read), G [RP][RP]; coordinates k >= r and columns
 * y >= len_valid are padding.  ps (len_pad values) and sumsq_part ((len_pad / 16) * RP values, enough for every rank) may be NULL; both are copied
 * to the device before the launch and back after it, so entries the kernel does not write keep what the caller put there.  *parts: the rows of
 * sumsq_part the sweep writes.  NMFAMD_INVALID_ARGUMENT wherever the launcher refuses (RP not instantiated, r outside 1 .. RP,
 * len_pad % 128 != 0, len_valid > len_pad). */
NMFAMD_API int nmfamd_op_hals_sweep_f32(float* P, const float* slabs, int S, long slab_stride, const float* G, int RP, int r, int len_pad, int len_valid,
                                        float* ps, float* sumsq_part, int* parts);
NMFAMD_API int nmfamd_op_hals_sweep_f64(double* P, const double* slabs, int S, long slab_stride, const double* G, int RP, int r, int len_pad, int len_valid,
                                        double* ps, double* sumsq_part, int* parts);
/* The same launch with penalties l1, l2 >= 0 on the swept factor: step k divides by G(k, k) + l2 (skipped where that is <= 0) and its gradient is
 * G(k, :) . p + l2 p(k) - a(k) + l1; ps is formed from the raw slabs.  l1 = l2 = 0 runs the unpenalised kernel.  NMFAMD_INVALID_ARGUMENT also for a negative
 * or non-finite penalty. */
NMFAMD_API int nmfamd_op_hals_sweep_pen_f32(float* P, const float* slabs, int S, long slab_stride, const float* G, int RP, int r, int len_pad, int len_valid,
                                            float* ps, float* sumsq_part, int* parts, float l1, float l2);
NMFAMD_API int nmfamd_op_hals_sweep_pen_f64(double* P, const double* slabs, int S, long slab_stride, const double* G, int RP, int r, int len_pad, int len_valid,
                                            double* ps, double* sumsq_part, int* parts, double l1, double l2);
/* `sweeps` penalised sweeps in a row against the same G and slabs, each from the result of the one before, in one launch (kernels_hals_multi.hip); ps and
 * sumsq_part from the final state, copied in and out as above.  sweeps = 1 is the launch of nmfamd_op_hals_sweep_pen_*.  NMFAMD_INVALID_ARGUMENT also for
 * sweeps outside 1 ... 64. */
NMFAMD_API int nmfamd_op_hals_sweeps_f32(float* P, const float* slabs, int S, long slab_stride, const float* G, int RP, int r, int len_pad, int len_valid,
                                         float* ps, float* sumsq_part, int* parts, float l1, float l2, int sweeps);
NMFAMD_API int nmfamd_op_hals_sweeps_f64(double* P, const double* slabs, int S, long slab_stride, const double* G, int RP, int r, int len_pad, int len_valid,
                                         double* ps, double* sumsq_part, int* parts, double l1, double l2, int sweeps);
/* At most `sweeps` sweeps with per-column dynamic stopping at the tolerance tol (kernels_hals_dyn.hip; docs/HALS.md, "Dynamic stopping"), always through
 * k_sweeps_hals_dyn, one sweep included.  counts (len_pad values, may be NULL): the sweeps applied to each column, 0 on padding.  NMFAMD_INVALID_ARGUMENT also
 * for tol outside (0, 1), NaN included. */
NMFAMD_API int nmfamd_op_hals_sweeps_dyn_f32(float* P, const float* slabs, int S, long slab_stride, const float* G, int RP, int r, int len_pad, int len_valid,
                                             float* ps, float* sumsq_part, int* parts, float l1, float l2, int sweeps, double tol, int* counts);
NMFAMD_API int nmfamd_op_hals_sweeps_dyn_f64(double* P, const double* slabs, int S, long slab_stride, const double* G, int RP, int r, int len_pad, int len_valid,
                                             double* ps, double* sumsq_part, int* parts, double l1, double l2, int sweeps, double tol, int* counts);
/* `steps` accelerated projected-gradient steps of NeNMF with the penalties (l1, l2) in one launch (kernels_nenmf.hip; docs/NENMF.md), on the arrays of
 * nmfamd_op_hals_sweeps_* and with its outputs: ps and sumsq_part from the final projected iterate, *parts = len_pad / the kernel's columns per workgroup (32 in
 * single, 16 in double precision).  Padded ranks 64 and 128.  NMFAMD_INVALID_ARGUMENT for steps outside 1 ... 256, another padded rank, a negative or
 * non-finite penalty and wherever nmfamd_op_hals_sweeps_* refuses. */
NMFAMD_API int nmfamd_op_apg_steps_f32(float* P, const float* slabs, int S, long slab_stride, const float* G, int RP, int r, int len_pad, int len_valid,
                                       float* ps, float* sumsq_part, int* parts, float l1, float l2, int steps);
NMFAMD_API int nmfamd_op_apg_steps_f64(double* P, const double* slabs, int S, long slab_stride, const double* G, int RP, int r, int len_pad, int len_valid,
                                       double* ps, double* sumsq_part, int* parts, double l1, double l2, int steps);
/* At most `steps` steps with per-column dynamic stopping at the tolerance tol (kernels_nenmf_dyn.hip; docs/NENMF.md, "Dynamic stopping"), always through
 * k_apg_steps_dyn, one step included.  counts (len_pad values, may be NULL): the steps applied to each column, 0 on padding.  NMFAMD_INVALID_ARGUMENT also for tol
 * outside (0, 1), NaN included. */
NMFAMD_API int nmfamd_op_apg_steps_dyn_f32(float* P, const float* slabs, int S, long slab_stride, const float* G, int RP, int r, int len_pad, int len_valid,
                                           float* ps, float* sumsq_part, int* parts, float l1, float l2, int steps, float tol, int* counts);
NMFAMD_API int nmfamd_op_apg_steps_dyn_f64(double* P, const double* slabs, int S, long slab_stride, const double* G, int RP, int r, int len_pad, int len_valid,
                                           double* ps, double* sumsq_part, int* parts, double l1, double l2, int steps, double tol, int* counts);
/* The HALS column normalisation on host panels Wt [mpad][RP] and H [npad][RP] (both updated in place) from parts x RP partial sums of squares:
 * d(c) = sqrt(sum of the parts); where d(c) > 0, Wt(:, c) / d(c) and H(:, c) * d(c). */
NMFAMD_API int nmfamd_op_hals_normalize_f32(float* Wt, int RP, int mpad, float* H, int npad, const float* sumsq_part, int parts);
NMFAMD_API int nmfamd_op_hals_normalize_f64(double* Wt, int RP, int mpad, double* H, int npad, const double* sumsq_part, int parts);
/* One half-step of the dense beta-divergence update (kernels_beta.hip, docs/DIVERGENCE.md) on host arrays, for tests: the fused launch and the update launch.
 * A [out_pad][RP] is the panel that is updated (in place), B [red_pad][RP] the other one, X [out_pad][ldx] the image of V with X(o, k) the entry at output index o and
 * reduction index k (zero on the padding; ldx >= red_pad, a multiple of 4); coordinates c >= r, rows o >= out_valid and reduction indices k >= red_valid are padding.
 * beta: 1 generalised KL (dsum: the RP denominators, the column sums of B) or 0 Itakura-Saito (dsum unused).  form: 0 update, 1 update + error terms, 2 error
 * terms only (A stays as it is).  force_slabs: 0 = the planned slab count, else that many (at most 16, at most the number of reduction tiles); *slabs: the count that ran.
 * t_frob / t_div (out_pad values each, forms 1 and 2): per output row the sums of (x - p)^2 and of the divergence, p = A(o, :) . B(k, :) + eps.  sumsq_part / sum_part
 * (optional, (out_pad / 128) * RP values): the per-workgroup sums of squares / sums of the new values.  NMFAMD_INVALID_ARGUMENT wherever the launchers refuse
 * (RP not 64 / 128 / 256, sizes that are not multiples of 128, ...). */
NMFAMD_API int nmfamd_op_beta_half_step_f32(float* A, const float* B, const float* X, long ldx, int RP, int r, int out_pad, int out_valid, int red_pad, int red_valid,
                                            int beta, int form, int force_slabs, const float* dsum, float* t_frob, float* t_div, float* sumsq_part, float* sum_part,
                                            int* slabs);
NMFAMD_API int nmfamd_op_beta_half_step_f64(double* A, const double* B, const double* X, long ldx, int RP, int r, int out_pad, int out_valid, int red_pad, int red_valid,
                                            int beta, int form, int force_slabs, const double* dsum, double* t_frob, double* t_div, double* sumsq_part, double* sum_part,
                                            int* slabs);
/* The same with any finite beta (0 and 1 run the launches above; every other value the general form, where t_div is the beta-divergence of
 * nmfamd_engine_divergence) and penalties l1, l2 >= 0 on the updated panel: A <- A (num / (den + eps + l1 + l2 A))^gamma.  dsum: beta = 1 only. */
NMFAMD_API int nmfamd_op_beta_half_step_general_f32(float* A, const float* B, const float* X, long ldx, int RP, int r, int out_pad, int out_valid, int red_pad,
                                                    int red_valid, double beta, double l1, double l2, int form, int force_slabs, const float* dsum, float* t_frob,
                                                    float* t_div, float* sumsq_part, float* sum_part, int* slabs);
NMFAMD_API int nmfamd_op_beta_half_step_general_f64(double* A, const double* B, const double* X, long ldx, int RP, int r, int out_pad, int out_valid, int red_pad,
                                                    int red_valid, double beta, double l1, double l2, int form, int force_slabs, const double* dsum, double* t_frob,
                                                    double* t_div, double* sumsq_part, double* sum_part, int* slabs);
/* The mixed-precision half-step (kernels_beta_bf16.hip; docs/DIVERGENCE.md, "Mixed precision"): nmfamd_op_beta_half_step_general_f32 with the fused launch whose
 * product operands are rounded to bf16; the update launch is the same.  Single precision only. */
NMFAMD_API int nmfamd_op_beta_half_step_mixed_f32(float* A, const float* B, const float* X, long ldx, int RP, int r, int out_pad, int out_valid, int red_pad,
                                                  int red_valid, double beta, double l1, double l2, int form, int force_slabs, const float* dsum, float* t_frob,
                                                  float* t_div, float* sumsq_part, float* sum_part, int* slabs);
/* The weighted half-step (kernels_beta_weighted.hip; docs/DIVERGENCE.md, "Weighted update"): nmfamd_op_beta_half_step_general_* with Omega, an array of the shape
 * and leading dimension of X that holds the weights (>= 0; 0 on the padding).  An entry with weight 0 is not there, whatever X holds at it.  The denominator is a
 * product at every beta: dsum is not used. */
NMFAMD_API int nmfamd_op_beta_half_step_weighted_f32(float* A, const float* B, const float* X, const float* Omega, long ldx, int RP, int r, int out_pad, int out_valid,
                                                     int red_pad, int red_valid, double beta, double l1, double l2, int form, int force_slabs, const float* dsum,
                                                     float* t_frob, float* t_div, float* sumsq_part, float* sum_part, int* slabs);
NMFAMD_API int nmfamd_op_beta_half_step_weighted_f64(double* A, const double* B, const double* X, const double* Omega, long ldx, int RP, int r, int out_pad, int out_valid,
                                                     int red_pad, int red_valid, double beta, double l1, double l2, int form, int force_slabs, const double* dsum,
                                                     double* t_frob, double* t_div, double* sumsq_part, double* sum_part, int* slabs);
/* The update launch of the minibatch update on caller-built arrays (kernels_beta_online.hip; docs/DIVERGENCE.md, "Minibatch update"): P [out_pad][RP] the panel,
 * num_part / den_part [slabs][out_pad][RP] the slabs' partial numerators / denominators (added in slab order; den_part unused at beta = 1, where dsum holds the RP
 * denominators), den = their sum + eps + l1 + l2 P.  online = 0: P <- P (num / den)^gamma.  online = 1: Aacc <- rho Aacc + P^(1 / gamma) num, Bacc <- rho Bacc + den,
 * P <- (Aacc / Bacc)^gamma (Aacc, Bacc: [out_pad][RP], replaced on the valid coordinates; 0 <= rho <= 1).  flush = 1: new values below eps become 0.  Rows
 * o >= out_valid and coordinates c >= r of P are 0 afterwards.  sum_part (optional, (out_pad / 16) * RP values): the sums of the new values over each 16 rows.
 * out_pad a multiple of 128, RP 64 / 128 / 256, at most 16 slabs. */
NMFAMD_API int nmfamd_op_beta_update_rows_f32(float* P, float* Aacc, float* Bacc, const float* num_part, const float* den_part, int slabs, const float* dsum, int RP,
                                              int r, int out_pad, int out_valid, double beta, double l1, double l2, int online, double rho, int flush, float* sum_part);
NMFAMD_API int nmfamd_op_beta_update_rows_f64(double* P, double* Aacc, double* Bacc, const double* num_part, const double* den_part, int slabs, const double* dsum, int RP,
                                              int r, int out_pad, int out_valid, double beta, double l1, double l2, int online, double rho, int flush, double* sum_part);
/* The two launches of a half-step one at a time, for the kernel-level tests (docs/DIVERGENCE.md, "Kernel-level tests").
 * op_beta_fused: the fused launch alone -- launch_beta_fused, launch_beta_fused_weighted with Omega (an array like X), launch_beta_fused_bf16 with mixed (f32
 * only, no Omega) -- under the plan nmfamd_op_beta_half_step_* uses.  A, B, X, ldx and the valid counts as there; update / terms: which of the launch's outputs are
 * asked for (at least one).  plan[5]: slabs, tiles, tiles_per_slab, bo, kt.  With all four output arrays NULL only the plan is returned and nothing is launched; the
 * caller sizes num_part / den_part [slabs][out_pad][RP] and tf_part / td_part [slabs][out_pad] (terms) from it.  The output arrays are uploaded as the caller
 * filled them and are not cleared before the launch: what the launch does not write (den_part at the unweighted beta = 1) comes back unchanged. */
NMFAMD_API int nmfamd_op_beta_fused_f32(const float* A, const float* B, const float* X, const float* Omega, long ldx, int RP, int out_pad, int out_valid, int red_pad,
                                        int red_valid, double beta, int update, int terms, int mixed, int force_slabs, float* num_part, float* den_part, float* tf_part,
                                        float* td_part, int* plan);
NMFAMD_API int nmfamd_op_beta_fused_f64(const double* A, const double* B, const double* X, const double* Omega, long ldx, int RP, int out_pad, int out_valid, int red_pad,
                                        int red_valid, double beta, int update, int terms, int mixed, int force_slabs, double* num_part, double* den_part, double* tf_part,
                                        double* td_part, int* plan);
/* op_beta_update: launch_beta_update alone on caller-built partial panels.  P [out_pad][RP] (in place); num_part / den_part [slabs][out_pad][RP], dsum [RP] (the
 * denominators of the unweighted beta = 1), tf_part / td_part [slabs][out_pad] with t_frob / t_div [out_pad] (all four or none); weighted: the launch the weighted
 * engines run (den_part at every beta).  update = 0: the terms only, P untouched.  sumsq_part / sum_part [(out_pad / 128)][RP] and t_frob / t_div are uploaded as the
 * caller filled them.  At most 16 slabs.  NMFAMD_INVALID_ARGUMENT wherever launch_beta_update refuses, nothing launched. */
NMFAMD_API int nmfamd_op_beta_update_f32(float* P, const float* num_part, const float* den_part, int slabs, const float* dsum, int RP, int r, int out_pad, int out_valid,
                                         double beta, double l1, double l2, int weighted, int update, const float* tf_part, const float* td_part, float* sumsq_part,
                                         float* sum_part, float* t_frob, float* t_div);
NMFAMD_API int nmfamd_op_beta_update_f64(double* P, const double* num_part, const double* den_part, int slabs, const double* dsum, int RP, int r, int out_pad, int out_valid,
                                         double beta, double l1, double l2, int weighted, int update, const double* tf_part, const double* td_part, double* sumsq_part,
                                         double* sum_part, double* t_frob, double* t_div);
/* The launches of the sparse path (kernels_sparse.hip), one each, on caller-built host arrays, for tests.  Panels are row-major [rows][RP]; a sparse image is
 * ptr / idx / val with 0-based int32 indices ascending within a row, nnz stored entries, the indices referring to rows of the gathered panel (b_rows / p_rows of
 * them).  eps is the epsilon of the type, as in the engine's KL iteration.  Output arrays are uploaded as the caller filled them and are not cleared before the
 * launch: what a launch does not write comes back unchanged.  NMFAMD_INVALID_ARGUMENT for sizes that do not fit, ranges of ptr outside [0, nnz], an index
 * outside the gathered panel, and wherever the launcher refuses (the gathers and the KL update run at RP 64, 128 and 256 only).
 *
 * kl_fused: out(row, :) = sum_p val[p] / (s .* A(row, :) . B(idx[p], :) + eps) * B(idx[p], :) over the row's entries (s = a_scale, NULL: ones); rows in
 * [rows, rows_pad) of out are zeroed.  t_vwh / t_kl (both or neither): per row sum val * wh and sum val * log(val / (wh + eps)) over the entries with val > 0.
 * blocks > 1: ptr is the [rows][blocks + 1] boundary array (entry b of a row: the first position whose index is >= b * ceil(b_rows / blocks)), out is
 * [blocks][rows_pad][RP] and t_vwh / t_kl are [blocks][rows_pad]: one partial result per block. */
NMFAMD_API int nmfamd_op_kl_fused_f32(const int* ptr, const int* idx, const float* val, long nnz, const float* A, const float* B, long b_rows, int RP, int rows,
                                      int rows_pad, int blocks, const float* a_scale, float* out, float* t_vwh, float* t_kl);
NMFAMD_API int nmfamd_op_kl_fused_f64(const int* ptr, const int* idx, const double* val, long nnz, const double* A, const double* B, long b_rows, int RP, int rows,
                                      int rows_pad, int blocks, const double* a_scale, double* out, double* t_vwh, double* t_kl);
/* masked_beta_half_step: one launch of the masked beta-divergence half-step (kernels_masked_beta.hip, docs/MISSING.md "Beta-divergence") of any instantiation.
 * A [a_rows][RP] (a_rows >= rows; in place: rows < `rows` are updated unless update = 0, the others come back as they were), B [b_rows][RP], RP 64, 128 or 256;
 * ptr / idx / val as above with rows + 1 offsets.  divergence / beta as nmfamd_params_v7.missing_divergence / missing_beta (1, 2, or 3 with beta); l1, l2 the
 * penalties of the half-step.  t_frob / t_div (both or neither, `rows` values) and sumsq_part (optional, update only; sumsq_parts = nmfamd_masked_norm_parts(rows)
 * vectors of RP values) are uploaded as the caller filled them, so what the launch does not write comes back unchanged. */
NMFAMD_API int nmfamd_masked_norm_parts(int rows);
NMFAMD_API int nmfamd_op_masked_beta_half_step_f32(const int* ptr, const int* idx, const float* val, long nnz, float* A, long a_rows, const float* B, long b_rows, int RP,
                                                   int rows, int divergence, double beta, double l1, double l2, int update, float* t_frob, float* t_div,
                                                   float* sumsq_part, int sumsq_parts);
NMFAMD_API int nmfamd_op_masked_beta_half_step_f64(const int* ptr, const int* idx, const double* val, long nnz, double* A, long a_rows, const double* B, long b_rows, int RP,
                                                   int rows, int divergence, double beta, double l1, double l2, int update, double* t_frob, double* t_div,
                                                   double* sumsq_part, int sumsq_parts);
/* masked_cd_half_step: one launch of the coordinate-descent half-step over the observed entries (kernels_masked_cd.hip, docs/MISSING.md "Coordinate descent").
 * A [a_rows][RP] (a_rows >= rows; rows < `rows` are updated in place, the others come back as they were), B [b_rows][RP], RP 64 or 128, r in 1 ... RP the
 * coordinates that count (the others may hold anything in A and B and come out 0 in the updated rows); ptr / idx / val as above with rows + 1 offsets, every index
 * inside B (checked here, on the host).  sweeps in 1 ... 64; l1, l2 the penalties of the half-step, finite and >= 0.  G_out [rows][RP][RP] and c_out [rows][RP]
 * (both or neither): the normal equations G_i = sum_p b_p b_p^T, c_i = sum_p val[p] b_p the launch formed for each row. */
NMFAMD_API int nmfamd_op_masked_cd_half_step_f32(const int* ptr, const int* idx, const float* val, long nnz, float* A, long a_rows, const float* B, long b_rows, int RP, int r,
                                                 int rows, int sweeps, double l1, double l2, float* G_out, float* c_out);
NMFAMD_API int nmfamd_op_masked_cd_half_step_f64(const int* ptr, const int* idx, const double* val, long nnz, double* A, long a_rows, const double* B, long b_rows, int RP, int r,
                                                 int rows, int sweeps, double l1, double l2, double* G_out, double* c_out);
/* predict_entries: one launch of the gather of kernels_predict.hip (docs/PREDICT.md) on caller-built padded panels Wt [w_rows][RP] and H [h_rows][RP] (fp32: RP 64,
 * 128, 256, 384, 512; fp64: 64 ... 512 in steps of 64), r in 1 ... RP the coordinates that count.  rows / cols: nnz >= 1 coordinates of index base 0 or 1, each
 * inside the panels (checked here, on the host: NMFAMD_INVALID_ARGUMENT).  vals (or NULL) and beta as nmfamd_engine_score, without its value rule.  out (or NULL
 * with vals; out_len >= nnz values) and part (with vals: parts = nmfamd_predict_entry_parts(nnz) triples of doubles -- a workgroup's sums of the squared errors, of
 * d_beta and of its absolute summands, to be added in index order) are uploaded as the caller filled them, so what the launch does not write comes back unchanged. */
NMFAMD_API int nmfamd_predict_entry_parts(long nnz);
NMFAMD_API int nmfamd_op_predict_entries_f32(const int* rows, const int* cols, const float* vals, long nnz, int base, const float* Wt, long w_rows, const float* H,
                                             long h_rows, int RP, int r, double beta, float* out, long out_len, double* part, int parts);
NMFAMD_API int nmfamd_op_predict_entries_f64(const int* rows, const int* cols, const double* vals, long nnz, int base, const double* Wt, long w_rows, const double* H,
                                             long h_rows, int RP, int r, double beta, double* out, long out_len, double* part, int parts);
/* top_k: the two launches of kernels_topk.hip (docs/TOPK.md) on caller-built padded panels: the query panel A [a_rows][RP] and the candidate panel B [b_rows][RP]
 * (RP as predict_entries), r in 1 ... RP the coordinates that count, candidates 0 ... count - 1 (count <= b_rows).  queries, k, base, excl_ptr / excl_idx (or both
 * NULL) and the outputs as nmfamd_engine_top_k; every index is checked here, on the host (NMFAMD_INVALID_ARGUMENT).  slabs: 0 for nmfamd_top_k_slabs(nq, count),
 * or 1 ... 256 to override it; the result does not depend on it. */
NMFAMD_API int nmfamd_op_top_k_f32(const int* queries, long nq, int k, int base, const float* A, long a_rows, const float* B, long b_rows, long count, int RP, int r,
                                   const long* excl_ptr, const int* excl_idx, int slabs, int* out_idx, float* out_scores);
NMFAMD_API int nmfamd_op_top_k_f64(const int* queries, long nq, int k, int base, const double* A, long a_rows, const double* B, long b_rows, long count, int RP, int r,
                                   const long* excl_ptr, const int* excl_idx, int slabs, int* out_idx, double* out_scores);
/* kl_update: P(y, c) <- (P(y, c) * scale(c)) * (sum over the parts of num) / (den(c) + eps) on P [len_pad][RP] (scale NULL: ones); num holds `parts` panels
 * part_stride values apart (a multiple of 4, >= len_pad * RP when parts > 1; what lies between two panels is not read).  sumsq_part / sum_part (each optional,
 * [len_pad / 128][RP]): per 128 rows the sums of squares / the sums of the new values.  len_pad a multiple of 128. */
NMFAMD_API int nmfamd_op_kl_update_f32(float* P, const float* num, int parts, long part_stride, const float* den, const float* scale, int RP, int len_pad,
                                       float* sumsq_part, float* sum_part);
NMFAMD_API int nmfamd_op_kl_update_f64(double* P, const double* num, int parts, long part_stride, const double* den, const double* scale, int RP, int len_pad,
                                       double* sumsq_part, double* sum_part);
/* kl_sums: sums(c) = sum over the parts of sum_part(., c), divided by sqrt(sum over the parts of sumsq_part(., c)) where sumsq_part is given and that sum is > 0;
 * scale (optional): 1 / sqrt of that sum, 1 where it is 0.  sum_part, sumsq_part: [parts][RP]. */
NMFAMD_API int nmfamd_op_kl_sums_f32(const float* sum_part, const float* sumsq_part, int parts, int RP, float* sums, float* scale);
NMFAMD_API int nmfamd_op_kl_sums_f64(const double* sum_part, const double* sumsq_part, int parts, int RP, double* sums, double* scale);
/* panel_rowsum: sums(c) = sum over y of P(y, c), P [len_pad][RP], len_pad a multiple of 128. */
NMFAMD_API int nmfamd_op_panel_rowsum_f32(const float* P, int RP, int len_pad, float* sums);
NMFAMD_API int nmfamd_op_panel_rowsum_f64(const double* P, int RP, int len_pad, double* sums);
/* spmm_rows: out(row, :) = sum_p val[p] * P(idx[p], :) over the row's entries; rows in [rows, rows_pad) of out are zeroed. */
NMFAMD_API int nmfamd_op_spmm_rows_f32(const int* ptr, const int* idx, const float* val, long nnz, const float* P, long p_rows, int RP, int rows, int rows_pad,
                                       float* out);
NMFAMD_API int nmfamd_op_spmm_rows_f64(const int* ptr, const int* idx, const double* val, long nnz, const double* P, long p_rows, int RP, int rows, int rows_pad,
                                       double* out);
/* sddmm_quotient: q[p] = val[p] / (A(row, :) . B(idx[p], :) + eps) for every stored entry (nnz values; A [rows][RP]); t_vwh / t_kl (both or neither, `rows`
 * values): the per-row terms of kl_fused, the logarithm taken in double. */
NMFAMD_API int nmfamd_op_sddmm_quotient_f32(const int* ptr, const int* idx, const float* val, long nnz, const float* A, const float* B, long b_rows, int RP, int rows,
                                            float* q, float* t_vwh, float* t_kl);
NMFAMD_API int nmfamd_op_sddmm_quotient_f64(const int* ptr, const int* idx, const double* val, long nnz, const double* A, const double* B, long b_rows, int RP, int rows,
                                            double* q, double* t_vwh, double* t_kl);
/* The extras of the fused iterations' launch for nmfamd_op_panel_update_* below (PanelFusedF32 / PanelFusedF64, csrc/kernels.h). */
typedef struct nmfamd_panel_fused {
	const void* old_scale;    /* RP values or NULL (W side): every old value is read as old(y, c) * old_scale[c] */
	int h_side;               /* H side: Q is the raw Gram matrix, num <- S D num, den = S D Q D S old */
	const void* scale;        /* RP values or NULL: the diagonal of D */
	int smooth;               /* 0: S = I; else S = (diag - off) I + off 1 1^T on the first r rank rows */
	double off, diag;
	int r;
	void* smooth_out;         /* [len_pad][RP] or NULL: S new (H side with smoothing), copied in and out like the other outputs */
	float* x3_out;            /* fp32 only, [len_pad][RP] floats or NULL: the decoded split image of S new (of new without smoothing) */
} nmfamd_panel_fused;
/* One launch of the Frobenius panel update (docs/PANEL_UPDATE.md) on host arrays in panel layout, for tests: through launch_panel_update<T> with the arguments the
 * engines pass, or -- `fused` given -- through the launchers the fused iterations call (fp32 at padded ranks 128 ... 512 with Q handed over as its split image; fp64 at
 * padded rank 64 and 128 ... 512).  mode: 0 multiplicative, 1 least squares, 2 plain slab sum.  P [len_pad][RP] (updated in place), S slabs of [len_pad][RP] at
 * slab_stride >= len_pad * RP elements (the gaps are not read), Q [RP][RP]; len_pad a multiple of 128.  Optional outputs (NULL: not requested, not allocated), each
 * copied to the device before the launch and back after it, so that what the launch leaves alone keeps the caller's values: ps (len_pad), sumsq_part (sumsq_rows rows
 * of RP, at least *parts of them), num_out [len_pad][RP], gram_partial (len_pad / 64 matrices of 64 x 64).  x3_out [len_pad][RP] floats: the split image of the new
 * rows decoded by adding its three bf16 planes (a slot the launch did not write decodes to NaN).  split_q: the scratch for the split image of Q is given; tri: an
 * all-default PanelTriExtras is given.  *parts = panel_update_parts().  NMFAMD_INVALID_ARGUMENT, with no output touched, wherever the launcher refuses. */
NMFAMD_API int nmfamd_op_panel_update_f32(int mode, float* P, const float* slabs, int S, long slab_stride, const float* Q, int RP, int len_pad, int len_valid, float eps,
                                          float* ps, float* sumsq_part, long sumsq_rows, float* num_out, float* gram_partial, float* x3_out, int split_q, int tri,
                                          const nmfamd_panel_fused* fused, int* parts);
NMFAMD_API int nmfamd_op_panel_update_f64(int mode, double* P, const double* slabs, int S, long slab_stride, const double* Q, int RP, int len_pad, int len_valid, double eps,
                                          double* ps, double* sumsq_part, long sumsq_rows, double* num_out, double* gram_partial, float* x3_out, int split_q, int tri,
                                          const nmfamd_panel_fused* fused, int* parts);
/* Which kernel the last nmfamd_op_panel_update_* of the calling thread was sent to, where forms that return the same values share a launcher (csrc/panel_form.h):
 * 0 a kernel outside kernels_wide.hip, 1 k_panel_update64_lds_f32, 2 k_panel_update_wide_f32 (32 rows per workgroup), 3 its fused instantiation,
 * 4 k_panel_update_rows_mu (128 rows), 5 k_panel_update_wide64_mu (64 rows). */
NMFAMD_API int nmfamd_op_panel_update_last_form(void);
/* One launch of the rank-64 fused multiplicative update (kernels_mu64.hip): tile = 64 through launch_mu64_update (gram_partial: len_pad / 64 matrices of 64 x 64, may be
 * NULL here, the kernel always writes them), tile = 32 through launch_mu64_update32 (colsq_part: len_pad / 32 vectors of 64, W side; qsplit in {2, 4, 8}: Q holds
 * qsplit unscaled 64 x 64 slices and q_out receives the finished matrix; ns != 0: SmoothAround {ns_off, ns_diag, ns_r}).  P [len_pad][64], scale 64 values, ps len_pad
 * values (H side: one term per valid column; W side: 64 terms, needs Gprev), x3_out [len_pad][64] floats: the decoded split image.  Outputs copied in and out as
 * above; no peer slabs.  NMFAMD_INVALID_ARGUMENT where the launcher refuses, and for a combination that would have a kernel go through a NULL pointer. */
NMFAMD_API int nmfamd_op_mu64_update_f32(int is_w, int tile, float* P, const float* slabs, int S, long slab_stride, const float* Q, const float* scale, float eps,
                                         int len_pad, int len_valid, float* ps, const float* Gprev, int compute_error, float* gram_partial, float* colsq_part,
                                         int qsplit, float* q_out, int ns, float ns_off, float ns_diag, int ns_r, float* x3_out);
/* Test access to an engine's device intermediates in panel layout: which = 0 Wt, 1 H, 2 W^T W,
 * 3 H H^T, 4 slabs, 5 inverse, 6 V, 7 Vt; rank-256 fp32 engines also 8 W^T W as last reduced, 9 staged column sums of squares,
 * 10 / 11 the bf16 fragments of W / H as 4-byte words; fp32 engines on the rank-64 fused path also 20 the pending column scale of W (64 values) and 21 the Wt panel
 * as it lies, unnormalised while that scale is pending (0 folds the scale in first), 22 the gram_k_slices unscaled K slices of W^T W (engines with more than one).
 * A negative count is refused. */
NMFAMD_API int nmfamd_engine_debug_read(nmfamd_engine* e, int which, void* out, long count);

#ifdef __cplusplus
}
#endif
#endif /* NMFGPU_AMD_H */
