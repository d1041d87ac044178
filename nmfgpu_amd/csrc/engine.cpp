// engine.cpp -- device-resident factorisation state and the per-iteration kernel sequences.
//
// Operation order per algorithm follows the reference's computeIteration bodies:
//   MU     source/nmf/AlgorithmMultiplicativeFrobenius.h:150-248
//   nsNMF  source/nmf/AlgorithmNonSmoothNMF.h:159-226
//   GDCLS  source/nmf/AlgorithmGradientDescentConstrainedLeastSquares.h:159-272
//   ACLS / AHCLS  source/nmf/AlgorithmAlternatingHoyerConstrainedLeastSquares.h:171-296
//   ALS    source/nmf/AlgorithmAlternatingLeastSquares.h:146-224
// but the eight vendor-BLAS calls + five custom kernels of one iteration collapse into the
// fused kernels of kernels.hip (see DESIGN.md section 4 for the mapping).
#include "engine.h"
#include "tuning.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <type_traits>

namespace nmfamd {

#define HIPX(call)                                        \
	do {                                                  \
		hipError_t e__ = (call);                          \
		if (e__ != hipSuccess) return hip_fail(e__, #call); \
	} while (0)

template <typename T>
double resolve_frobenius(const std::vector<T>& vtv_sorted, std::vector<T>& htwtv, std::vector<T>& hhtwtw) {
	return std::sqrt(resolve_frobenius_squared<T>(vtv_sorted, htwtv, hhtwtw));
}
template double resolve_frobenius<float>(const std::vector<float>&, std::vector<float>&, std::vector<float>&);
template double resolve_frobenius<double>(const std::vector<double>&, std::vector<double>&, std::vector<double>&);

// Ascending sort of the error-term vectors (std::sort in source/nmf/FrobeniusResolver.cpp:33-35).  A sorted sequence of values is the same whatever the
// algorithm, so long vectors go through a radix sort on the order-preserving integer image of the floating-point bits (three or four passes over n keys instead of
// n log n comparisons): at config 2's n = 5 000 the comparison sort cost the drop-in loop ~0.2 ms of host time per error iteration -- with the device idle, because
// whether the run goes on depends on the value (nmfgpu::compute, thresholdValue) -- 108 us per iteration end to end against 87 in the resident engine.
// NaNs (a diverged run) keep std::sort's company: they are sent to the comparison sort.
template <typename T>
static void sort_terms(std::vector<T>& v) {
	const size_t n = v.size();
	if (n < 256) { std::sort(v.begin(), v.end()); return; }
	for (size_t i = 0; i < n; ++i) if (v[i] != v[i]) { std::sort(v.begin(), v.end()); return; }
	using U = typename std::conditional<sizeof(T) == 4, std::uint32_t, std::uint64_t>::type;
	constexpr int BITS = 11, BUCKETS = 1 << BITS, PASSES = (int)((8 * sizeof(T) + BITS - 1) / BITS);
	constexpr U SIGN = (U)1 << (8 * sizeof(T) - 1);
	std::vector<U> a(n), b(n);
	for (size_t i = 0; i < n; ++i) {
		U u;
		std::memcpy(&u, &v[i], sizeof(T));
		a[i] = (u & SIGN) ? ~u : (u | SIGN);          // negative values: all bits flipped; others: sign bit set -- unsigned order = numeric order (-0 before +0)
	}
	std::vector<size_t> count(BUCKETS);
	for (int p = 0; p < PASSES; ++p) {
		const int shift = p * BITS;
		std::fill(count.begin(), count.end(), (size_t)0);
		for (size_t i = 0; i < n; ++i) ++count[(a[i] >> shift) & (BUCKETS - 1)];
		size_t run = 0;
		for (int k = 0; k < BUCKETS; ++k) { const size_t c = count[k]; count[k] = run; run += c; }
		for (size_t i = 0; i < n; ++i) b[count[(a[i] >> shift) & (BUCKETS - 1)]++] = a[i];
		a.swap(b);
	}
	for (size_t i = 0; i < n; ++i) {
		const U u = (a[i] & SIGN) ? (a[i] & ~SIGN) : ~a[i];
		std::memcpy(&v[i], &u, sizeof(T));
	}
}

template <typename T>
double resolve_frobenius_squared(const std::vector<T>& vtv_sorted, std::vector<T>& htwtv, std::vector<T>& hhtwtw) {
	sort_terms(htwtv);
	sort_terms(hhtwtw);
	double acc = 0.0;
	const size_t mx = std::max(vtv_sorted.size(), std::max(htwtv.size(), hhtwtw.size()));
	for (size_t j = 0; j < mx; ++j) {
		if (j < vtv_sorted.size()) acc += vtv_sorted[j];
		if (j < htwtv.size()) acc -= 2.f * htwtv[j];   // float literal: the product is formed in T, as in the reference
		if (j < hhtwtw.size()) acc += hhtwtw[j];
	}
	return acc;
}
template double resolve_frobenius_squared<float>(const std::vector<float>&, std::vector<float>&, std::vector<float>&);
template double resolve_frobenius_squared<double>(const std::vector<double>&, std::vector<double>&, std::vector<double>&);

// Size of the device's memory-side cache (AMD Infinity Cache): not in hipDeviceProp_t, so a table by architecture -- 256 MiB
// on gfx942 / gfx950 in SPX mode (/opt/skills/guides/MI355X_MICROARCH.md, "Infinity Cache (L3) 256 MiB") -- which
// NMFAMD_MALL_MB overrides (other parts, partitioned modes, several engines sharing the cache).  0 = unknown: no window.
// The free memory is asked for here, once, whatever the plan: plan() looks at it on the split-operand path only, where the question used to be put -- before the
// engine's first allocation there as well, so the answer is the same.  A device that does not answer counts as one with room.
hipError_t device_facts(DeviceFacts* out) {
	int dev = 0;
	hipDeviceProp_t prop;
	hipError_t e = hipGetDevice(&dev);
	if (e == hipSuccess) e = hipGetDeviceProperties(&prop, dev);
	if (e != hipSuccess) return e;
	out->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
	out->memory_side_cache_bytes = (std::strncmp(prop.gcnArchName, "gfx942", 6) == 0 || std::strncmp(prop.gcnArchName, "gfx950", 6) == 0) ? (size_t)256 << 20 : 0;
	if (const char* env = std::getenv("NMFAMD_MALL_MB")) { const long mb = std::atol(env); out->memory_side_cache_bytes = mb > 0 ? (size_t)mb << 20 : 0; }
	size_t total_b = 0;
	if (hipMemGetInfo(&out->free_bytes, &total_b) != hipSuccess) { (void)hipGetLastError(); out->free_bytes = std::numeric_limits<size_t>::max(); }
	return hipSuccess;
}

template <typename T>
Engine<T>::Engine(int m, int n, int r, int algorithm, const AlgorithmParams& params)
	: m_(m), n_(n), r_(r), RP_(padded_rank(r, (params.sparse_compute != 0 || params.divergence != 0 || params.is_masked()) ? 4 : sizeof(T))), alg_(algorithm), prm_(params), mpad_(pad128(m)), npad_(pad128(n)) {}

template <typename T>
Status Engine<T>::hip_fail(hipError_t e, const char* what) {
	last_error_ = what;
	(void)hipGetLastError();
	return e == hipErrorOutOfMemory ? ST_NO_DEVICE_MEMORY : ST_HIP_ERROR;
}

#ifdef NMFAMD_DIAG_BUILD
// measurement build, NMFAMD_BF_STAMPS=<file>: the waves' life stamps of the last W^T V (kind 0) and V H^T (kind 1) launch of the rank-256 bf16 product, written
// to the file when an engine is destroyed (tools/stamp_bf16.py): [kind][512 workgroups][4 waves][entry, loop start, loop end, exit] in 100 MHz ticks
static unsigned long long* g_bf_stamps = nullptr;
static unsigned long long* bf_stamps(int kind) {
	static const char* path = std::getenv("NMFAMD_BF_STAMPS");
	if (path == nullptr) return nullptr;
	if (g_bf_stamps == nullptr) {
		if (hipMalloc((void**)&g_bf_stamps, 2 * 512 * 16 * sizeof(unsigned long long)) != hipSuccess) { g_bf_stamps = nullptr; return nullptr; }
		(void)hipMemset(g_bf_stamps, 0, 2 * 512 * 16 * sizeof(unsigned long long));
	}
	return g_bf_stamps + (long)kind * 512 * 16;
}
static void bf_stamps_dump() {
	const char* path = std::getenv("NMFAMD_BF_STAMPS");
	if (g_bf_stamps == nullptr || path == nullptr) return;
	std::vector<unsigned long long> h(2 * 512 * 16);
	(void)hipDeviceSynchronize();
	if (hipMemcpy(h.data(), g_bf_stamps, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess) {
		if (FILE* f = std::fopen(path, "wb")) { std::fwrite(h.data(), sizeof(unsigned long long), h.size(), f); std::fclose(f); }
	}
}
#endif

template <typename T>
Engine<T>::~Engine() {
#ifdef NMFAMD_DIAG_BUILD
	if (bf16_) bf_stamps_dump();
#endif
	if (f64_stamps_ != nullptr) {
		std::vector<unsigned long long> h((size_t)4 * 4096 * 8);
		if (hipMemcpy(h.data(), f64_stamps_, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost) == hipSuccess) {
			if (FILE* f = std::fopen(tuning_env("NMFAMD_F64_STAMPS"), "wb")) { std::fwrite(h.data(), sizeof(unsigned long long), h.size(), f); std::fclose(f); }
		}
	}
	if (err_event_) (void)hipEventDestroy(err_event_);
	if (ev_fork_) (void)hipEventDestroy(ev_fork_);
	if (ev_join_) (void)hipEventDestroy(ev_join_);
	if (aux_) (void)hipStreamDestroy(aux_);
	for (hipEvent_t e : ev_) (void)hipEventDestroy(e);
}      // (buffers_ frees the memory)

template <typename T>
Status Engine<T>::allocate() {
	if (Status s = check_parameters()) return s;
	DeviceFacts device;
	HIPX(device_facts(&device));
	if (Status s = plan(device)) return s;
	return allocate_buffers();
}

template <typename T>
Status Engine<T>::check_parameters() {
	if (m_ <= 0|| n_ <= 0 || r_ <= 0 || alg_ < 0 || alg_ > ALG_NENMF) return ST_INVALID;
	if (alg_ == ALG_HALS && !panel_sweep_hals_available(RP_, sizeof(T))) { last_error_ = "HALS: no sweep kernel for this padded rank (fp32: 64 ... 512, fp64: multiples of 64 up to 512)"; return ST_INVALID; }
	if (alg_ == ALG_NENMF && !panel_steps_apg_available(RP_, sizeof(T))) { last_error_ = "NeNMF: no step kernel for this padded rank (supported ranks: 1 ... 128, in either precision)"; return ST_INVALID; }
	if (const char* why = nenmf_steps_fault(prm_.steps_h, prm_.steps_w, false, alg_ == ALG_NENMF)) { last_error_ = why; return ST_INVALID; }
	if (Status s = set_hals_penalties(prm_.l1W, prm_.l1H, prm_.l2W, prm_.l2H)) return s;      // (values that came with the parameters: the setter's checks, and its rounding of prm_ to T)
	if (const char* why = hals_sweeps_fault(prm_.sweeps_h, prm_.sweeps_w, alg_ == ALG_HALS)) { last_error_ = why; return ST_INVALID; }
	if (const char* why = hals_sweep_tolerance_fault(prm_.sweep_tolerance, alg_ == ALG_HALS)) { last_error_ = why; return ST_INVALID; }
	if (const char* why = nenmf_step_tolerance_fault(prm_.steps_tolerance, prm_.steps_tolerance != 0, alg_ == ALG_NENMF)) { last_error_ = why; return ST_INVALID; }
	if (const char* why = beta_dense_fault(prm_, alg_ == ALG_MU, r_, row_blocks_)) { last_error_ = why; return ST_INVALID; }
	if (const char* why = masked_beta_fault(prm_, alg_ == ALG_MU, r_, row_blocks_)) { last_error_ = why; return ST_INVALID; }
	if (const char* why = weighted_fault(prm_)) { last_error_ = why; return ST_INVALID; }
	beta_dense_ = prm_.is_beta_dense();
	masked_beta_ = prm_.is_masked_beta();
	if (masked_beta_) {
		// beta in the engine's precision, as the dense engines take theirs: a value that rounds to 0 or 1 there IS the Itakura-Saito or the KL map
		mbeta_ = (double)(T)prm_.masked_beta();
		if (!std::isfinite(mbeta_)) { last_error_ = "missing-value divergence: 'missingBeta' out of the range of the engine's precision"; return ST_INVALID; }
	}
	if (const char* why = mixed_precision_fault(prm_, sizeof(T) == 4)) { last_error_ = why; return ST_INVALID; }
	if (const char* why = minibatch_fault(prm_)) { last_error_ = why; return ST_INVALID; }
	weighted_ = prm_.weighted != 0;
	mixed_ = prm_.mixed_precision != 0;
	minibatch_ = prm_.is_minibatch();
	if (beta_dense_) {
		// beta in the engine's precision, as the penalties: a value that rounds to 0 or 1 there IS the Itakura-Saito or the dense KL engine
		beta_ = (double)(T)prm_.beta();
		if (!std::isfinite(beta_)) { last_error_ = "dense divergence update: 'beta' out of the range of the engine's precision"; return ST_INVALID; }
	}
	return ST_OK;
}

// Everything that decides which kernels run and in which order partial sums are added, from the shape, the parameters, the three device facts and the environment
// switches: no HIP call, so nmfamd_plan_geometry (and the CPU suite through it) sees exactly what an engine on such a device would run.
template <typename T>
Status Engine<T>::plan(const DeviceFacts& device) {
	num_cus_ = device.num_cus;

	// both products run on the MFMA pipe: fp32 (kernels.hip) or fp64 (kernels_f64.hip), each with its own cut
	const bool f64 = std::is_same<T, double>::value;
	planH_ = f64 ? plan_factor_product_f64(n_, m_, RP_, num_cus_) : plan_factor_product(n_, m_, RP_, num_cus_);
	planW_ = f64 ? plan_factor_product_f64(m_, n_, RP_, num_cus_) : plan_factor_product(m_, n_, RP_, num_cus_);
	const bool mfma = std::getenv("NMFAMD_FORCE_VALU") == nullptr;
	// ranks <= 32: the fp32 product computes 32 panel columns instead of 64 (half the MFMA work; the kernel turns HBM-bound)
	if (RP_ == 64 && r_ <= 32 && tuning_env("NMFAMD_FP_FULL_WIDTH") == nullptr) { planH_.nb = f64 ? 2 : 1; planW_.nb = planH_.nb; }      // (fp64 counts 16-column tiles)
	if (!mfma) { planH_.splits = 1; planW_.splits = 1; planH_.th = planW_.th = 128; planH_.xtiles = (int)(pad128(n_) / 128); planW_.xtiles = (int)(pad128(m_) / 128); }
	tiled_ = mfma;
	// (the SpMM / KL / masked kernels gather RP / 64 = 1, 2 or 4 values per lane: sparse runs keep the 128-column padding in either precision, see the constructor)
	sparse_ = !beta_dense_ && (prm_.sparse_compute != 0 || prm_.divergence != 0 || prm_.is_masked());
	if (prm_.is_masked() && (alg_ != ALG_MU || prm_.divergence != 0 || RP_ > 256)) { last_error_ = "missing values: multiplicative update with the Frobenius objective, rank <= 256"; return ST_INVALID; }
	if (sparse_) {
		// sparse compute: multiplicative update (either objective, masked or not) and HALS (Frobenius, not masked), padded rank 64 / 128 / 256
		const char* why = nullptr;
		if (hals_family(alg_) && (prm_.divergence != 0 || prm_.is_masked())) why = "HALS: sparse compute with the Frobenius objective only (no 'divergence', no missing values)";
		else if (alg_ != ALG_MU && !hals_family(alg_)) why = "sparse compute: multiplicative update and HALS only";
		else if (RP_ > 256) why = "sparse compute needs rank <= 256 (the SpMM kernels gather 1, 2 or 4 values per lane)";
		if (why != nullptr) { last_error_ = why; return ST_INVALID; }
		tiled_ = false;
		planH_.splits = planW_.splits = 1; planH_.th = planW_.th = 128;
		planH_.xtiles = (int)(pad128(n_) / 128); planW_.xtiles = (int)(pad128(m_) / 128);
	}
	if (beta_dense_) {
		// dense beta-divergence update (kernels_beta.hip): V_ is the plain column-major image, Vt_ its transpose; the slab counts of the two fused half-steps
		// (a function of the shape and the CU count) are what slabs_h() / slabs_w() report
		tiled_ = false;
		planH_.th = planW_.th = 128;
		planH_.xtiles = (int)(pad128(n_) / 128); planW_.xtiles = (int)(pad128(m_) / 128);
		betaH_ = plan_beta_half_step(pad128(n_), pad128(m_), RP_, sizeof(T), num_cus_);
		betaW_ = plan_beta_half_step(pad128(m_), pad128(n_), RP_, sizeof(T), num_cus_);
		planH_.splits = betaH_.slabs; planW_.splits = betaW_.slabs;
		if (minibatch_) {
			// the minibatch update: the same two launches on a block of columns -- a full batch and the remainder batch, each padded to 128 (the reported slab
			// counts stay those of the full shape, which the error iterations' terms-only launch uses)
			batch_ = (long)prm_.batch_size;
			rho_ = (double)(T)std::pow(prm_.forget_factor, (double)std::min<long>(batch_, n_) / (double)n_);
			const long rem = n_ % batch_;
			if (batch_ <= n_) {
				betaHb_ = plan_beta_half_step(batch_, pad128(m_), RP_, sizeof(T), num_cus_);
				betaWb_ = plan_beta_half_step(pad128(m_), batch_, RP_, sizeof(T), num_cus_);
			}
			if (rem > 0) {
				betaHr_ = plan_beta_half_step(pad128(rem), pad128(m_), RP_, sizeof(T), num_cus_);
				betaWr_ = plan_beta_half_step(pad128(m_), pad128(rem), RP_, sizeof(T), num_cus_);
			}
		}
	}
	if (prm_.precision > 0) {
		// bf16 operands for the two big products, dense (resident) V only; every algorithm, padded rank 64 or k * 128
		if (!std::is_same<T, float>::value || sparse_ || !mfma) return ST_INVALID;
		bf16_ = true;
		tiled_ = false;
		planH_.th = planW_.th = 128;
		planH_.xtiles = (int)(pad128(n_) / 128); planW_.xtiles = (int)(pad128(m_) / 128);
		ksW_ = (n_ + 15) / 16; ksH_ = (m_ + 15) / 16;
		planH_.splits = plan_splits_bf16(planH_.xtiles, ksH_, RP_, num_cus_);
		planW_.splits = plan_splits_bf16(planW_.xtiles, ksW_, RP_, num_cus_);
		// Padded rank 256 (the kernels_tri.hip iteration): the Gram matrix of the operand a product multiplies V with rides in that product's launch as TRI_PASSENGERS
		// workgroups (tri_gram_tile.h) -- its consumer is the update kernel behind the launch.  V (S H)^T leaves the CUs free as it is (config 4: 224 workgroups);
		// W^T V is planned with one K slice fewer (9 -> 8: 252 -> 224 workgroups).  NMFAMD_TRI_RIDE = 0 / h / w: none / only (S H)(S H)^T / only W^T W.
		if (RP_ == 256 && (alg_ == ALG_MU || alg_ == ALG_NSNMF) && tri_kernels_available(RP_)) {
			const char* e = tuning_env("NMFAMD_TRI_RIDE");
			const bool want_w = e == nullptr || (e[0] != '0' && e[0] != 'h'), want_h = e == nullptr || (e[0] != '0' && e[0] != 'w');
			if (want_w && num_cus_ > 2 * TRI_PASSENGERS) {
				FactorProductPlan t = planH_;
				t.splits = plan_splits_bf16(planH_.xtiles, ksH_, RP_, num_cus_ - TRI_PASSENGERS);
				if (bf16_product_workgroups(t) + TRI_PASSENGERS <= num_cus_) { planH_.splits = t.splits; tri_ride_w_ = true; }
			}
			tri_ride_h_ = want_h && bf16_product_workgroups(planW_) + TRI_PASSENGERS <= num_cus_;
		}
		planHb_ = planH_; planWb_ = planW_;
	}
	// fp32, dense, MFMA path: both products run on the bf16 matrix pipe with every operand split exactly into
	// three bf16 terms (fp32-level accuracy, six cross products; kernels_x3.hip) -- HBM-bound instead of bound by
	// the fp32 MFMA rate.  precision = -1 (or NMFAMD_FP32_NATIVE) keeps the native fp32 MFMA instructions.
	// (ranks <= 32 stay on the fp32 MFMA kernel: with half its MFMA work it is HBM-bound already and needs no split image)
	// ... except where one image in the memory-side cache pays more than the halved MFMA work (§3: 107 -> 100 us at config 2's shape)
	// One resident image pays when it fits the memory-side (Infinity) cache and two do not: a window around the cache size,
	// computed once from the device (DeviceFacts::memory_side_cache_bytes)
	const size_t image_bytes = sizeof(T) * (size_t)pad128(m_) * (size_t)pad128(n_);
	const size_t mall = device.memory_side_cache_bytes;
	const bool cache_window = mall > 0 && (double)image_bytes > 0.6 * (double)mall && (double)image_bytes < 1.12 * (double)mall && std::getenv("NMFAMD_ONE_IMAGE") == nullptr;
	// (the opt-in one-pass iteration runs on the split-operand products whatever the rank)
#ifdef NMFAMD_DIAG_BUILD
	const char* op_env = tuning_env("NMFAMD_ONE_PASS");
	const bool op_req = op_env != nullptr && std::atoi(op_env) != 0 && one_pass_allowed_ && row_blocks_ == 1 && fused_capable() && RP_ == 64 &&
	                    std::getenv("NMFAMD_GRAM_PARTIALS") == nullptr && tuning_env("NMFAMD_IMAGE_TILE128") == nullptr && onepass_available(pad128(m_), num_cus_);
#else
	const bool op_req = false;      // (kernels_onepass.hip is part of the measurement build only: round 6)
#endif
	if (std::is_same<T, float>::value && tiled_ && !bf16_ && !sparse_ && RP_ % 64 == 0 && prm_.precision == 0 && (planH_.nb == 2 || cache_window || op_req) &&
	    tuning_env("NMFAMD_FP32_NATIVE") == nullptr) {
		planH_.nb = planW_.nb = 2;
		x3_ = true;
		planH_.th = planW_.th = 128;
		planH_.xtiles = (int)(pad128(n_) / 128); planW_.xtiles = (int)(pad128(m_) / 128);
		ksW_ = (n_ + 15) / 16; ksH_ = (m_ + 15) / 16;
		// W^T W rides in the W^T V launch as passenger workgroups (gram_image.h).  Its chain -- the fragments of all m rows through ONE CU per tile, 24 us at
		// config 2's m -- must stay shorter than the product: for a column shard narrower than config 2 the K range is
		// cut into slices (10 passenger workgroups each, CUs the product plan leaves free); config 2 itself keeps one slice and its plan (measured hidden).
		gram_ksplit_ = 1;
		if (fused_capable() && RP_ == 64 && std::getenv("NMFAMD_GRAM_PARTIALS") == nullptr) {
			const double product_us = 6.0 + (double)sizeof(T) * (double)pad128(m_) * (double)pad128(n_) / 5.0e6;       // (bytes at ~5 TB/s + launch and fill)
			const double pairs = (ksH_ + 2) / 2;
			while (gram_ksplit_ < GRAM_KSPLIT_MAX && 24.0 * (pairs / 317.0) / gram_ksplit_ > 0.55 * product_us) gram_ksplit_ *= 2;      // (24 us for config 2's 317 pairs in one slice: one CU's L2 rate, gram_image.h)
			// (NMFAMD_GRAM_KSPLIT = 1 / 2 / 4 / 8 forces the slice count: the parity tests run every form at shapes the oracle covers)
			if (const char* e = tuning_env("NMFAMD_GRAM_KSPLIT")) { const int k = std::atoi(e); if (k == 1 || k == 2 || k == 4 || k == 8) gram_ksplit_ = k; }
		}
		planH_.splits = plan_splits_x3(planH_.xtiles, ksH_, num_cus_, gram_ksplit_ > 1 ? GRAM_IMAGE_TILES * gram_ksplit_ : 0);
		planW_.splits = plan_splits_x3(planW_.xtiles, ksW_, num_cus_);
		planHx_ = planH_; planWx_ = planW_;
		planHx_.steps_total = ksH_; planWx_.steps_total = ksW_;
		planHx_.nb = planWx_.nb = 2;
		// One resident image of V or two?  With two, each product streams its own image along its output index (the
		// faster kernel form); with one, W^T V reads the image of V along its reduction index (y-tiled form, ~20 % slower
		// per launch on its own).  One image wins when it fits the 256 MiB memory-side cache but two do not: both products
		// of an iteration then find most of V there (config 2: V H^T 49 -> 37 us, iteration 126 -> 108 us).  Measured
		// (10 000 x 5 000 scaled, r = 64): 148 MB two images 97 us / one 102; 185 MB 109 / 100; 207 MB 126 / 108; 246 MB
		// 145 / 129; 266 MB 152 / 143; 328 MB 173 / 174; 1.6 GB 792 / 988.  Also one image when two (plus the staging
		// image of the upload) do not fit in HBM.  NMFAMD_ONE_IMAGE = 1 / 0 forces the choice.
		const char* force = std::getenv("NMFAMD_ONE_IMAGE");
		// the one-pass iteration needs ONE image (16-row tiles) and nothing else
		// (measurement build, NMFAMD_ONE_PASS=1: measured slower than the two-pass iteration, docs/HISTORY.md)
		one_pass_ = op_req && (force == nullptr || std::atoi(force) != 0);
		if (one_pass_) one_image_ = true;
		else if (force != nullptr) one_image_ = std::atoi(force) != 0;
		else if (cache_window) one_image_ = true;
		else if (3 * image_bytes + (image_bytes >> 3) > device.free_bytes) one_image_ = true;
		// V H^T of a narrow column shard (short reduction range: at most 20 K-steps per wave without K slices): ONE slab from 128 x 32 workgroups, two per x-tile and two to a
		// CU (kernels_x3.hip, NBW = 1), instead of up to three K slices of 128 x 64 ones.  Per wave the 128 x 64 form is bound by its own MFMA issue (35 cycles each) while
		// a third of the chip's SIMDs work; the narrow form puts a second wave on every SIMD (the operand split is done twice, so it pays only while the range is short).
		// Same bits as the 128 x 64 form with one slice; and one slab is the exchange panel of the sharded loop as it stands (no k_reduce_slabs launch).
		// Measured at m = 10 000 (tools/shard_trace.py; fused loop / rank-of-N rehearsal, us per iteration): n = 625: 39.4 -> 36.6 / 40.4 -> 37.5; n = 1 250: 44.4 -> 44.3 /
		// 48.5 -> 45.3; n = 1 900: 50.8 -> 52.9 / 54.8 -> 54.0; n = 2 500: 58.5 -> 61.7 / 63.4 -> 62.5 -- hence the limit of 80 K-steps.  Both products in this form at
		// config 2: 92.7 -> 106.7 us (NMFAMD_X3_COLSPLIT = 2).  NMFAMD_X3_COLSPLIT = 0 / 1 forces the choice (parity test, measurements).
		w_col_split_ = false;
		if (RP_ == 64 && fused_capable() && !one_image_ && 2 * planW_.xtiles + GRAM_REDUCE_BLOCKS <= 2 * num_cus_) {
			w_col_split_ = ksW_ <= 80 && 4 * planW_.xtiles >= num_cus_;
			if (const char* e = tuning_env("NMFAMD_X3_COLSPLIT")) { const int v = std::atoi(e); if (v == 0) w_col_split_ = false; else if (v == 1) w_col_split_ = true; }
			if (w_col_split_) { planW_.splits = planWx_.splits = 1; planWx_.col_split = 2; }
		}
		// (measurement builds, NMFAMD_X3_COLSPLIT = 2: both products from 128 x 32 workgroups, two per CU, with the plan's K slices)
		if (const char* e = tuning_env("NMFAMD_X3_COLSPLIT")) { if (std::atoi(e) == 2 && RP_ == 64 && fused_capable()) { planHx_.col_split = planWx_.col_split = 2; w_col_split_ = true; } }
	}
	// panels (and the slabs the products write) cover whole x-tiles and whole 128-column update tiles
	mpad_ = pad128(std::max<long>(m_, (long)planW_.xtiles * planW_.th));
	if (row_blocks_ > 1) { const long g = 128l * row_blocks_; mpad_ = ((mpad_ + g - 1) / g) * g; }   // equal row blocks of whole 128-row tiles
	npad_ = pad128(std::max<long>(n_, (long)planH_.xtiles * planH_.th));
	img_th_ = (one_image_ && tuning_env("NMFAMD_IMAGE_TILE128") == nullptr) ? 16 : planW_.th;
	strideV_ = (long)img_th_ * npad_;
	strideVt_ = (long)planH_.th * mpad_;
	elemsV_ = mpad_ * npad_;     // tiled or not: every tile spans all columns
	elemsVt_ = tiled_ ? (long)planH_.xtiles * strideVt_ : mpad_ * npad_;
	slab_stride_ = (long)RP_ * std::max(mpad_, npad_);
	ps_stride_ = std::max<long>(npad_, RP_);
	// wide fp32 panels: the update kernel multiplies with the split image of an r x r matrix (kernels_wide.hip)
	wide_q_image_ = std::is_same<T, float>::value && panel_update_wide_available(RP_) && std::getenv("NMFAMD_FORCE_VALU") == nullptr && tuning_env("NMFAMD_WIDE_FP32_MFMA") == nullptr;
	tri_ = bf16_ && tri_kernels_available(RP_) && (alg_ == ALG_MU || alg_ == ALG_NSNMF);
	if (tri_) tri_w_den_bf16_ = tuning_env("NMFAMD_TRI_FP32_DEN") == nullptr;
	overlap_inverse_ = alg_ >= ALG_GDCLS && alg_ <= ALG_AHCLS && tuning_env("NMFAMD_NO_OVERLAP") == nullptr;      // (the r x r inverse on a side stream)
	gram_image_ = x3_ && fused_capable() && RP_ == 64 && std::getenv("NMFAMD_GRAM_PARTIALS") == nullptr;
	one_pass_ = one_pass_ && x3_ && gram_image_ && one_image_ && img_th_ == 16;
	op_stamps_wanted_ = one_pass_ && tuning_env("NMFAMD_ONEPASS_STAMPS") != nullptr;
	// W^T W of a whole problem (one K slice): the ten tiles' K ranges dealt to all sixteen passengers (gram_image.h) -- with a tile each, ten of them were the
	// last workgroups of config 2's W^T V launch (37 - 40 us against 33 - 36.5 for the product blocks, profiles/r05_update_tail.md).  NMFAMD_GRAM_SPREAD=0
	// (measurement builds) restores that form.
	if (fused_capable() || gram_from_update()) gram_spread_ = gram_ksplit_ == 1 && !(tuning_env("NMFAMD_GRAM_SPREAD") != nullptr && std::atoi(tuning_env("NMFAMD_GRAM_SPREAD")) == 0);
	fused32w_planned_ = fused32w_capable();
	if (fused32w_planned_) {
		// The Gram slices as passengers of the product launch (gram_wide.h) where the product's first round of workgroups leaves CUs free for them and their chain --
		// a slice's K-steps at ~0.75 us each under the product's memory stream (measured: 625 steps in one slice made a 330 us launch 460) -- stays inside the launch,
		// or is shorter than the launch of their own it replaces (~10 us); otherwise k_gram_wide_x3.  Measured (profiles/r06_f32w_ride_ab.txt), 10 000 x 5 000:
		// r = 128 184.4 -> 166.7 us per iteration, r = 158 336.3 -> 309.7; 4096 x 165, r = 158: 103.7 -> 83.6; forced at r = 500 (one slice per super-block): 709 -> 967.
		// NMFAMD_F32W_RIDE = 0 / 1 (measurement builds): never / wherever a CU is free.
		const int nbk = RP_ / 128, nsuper = nbk * (nbk + 1) / 2;
		const char* force = tuning_env("NMFAMD_F32W_RIDE");
		auto ride = [&](const FactorProductPlan& p, long len) {
			const int wgs = p.xtiles * p.splits;      // (per layer of 128 columns; the passengers sit in the first layer)
			if (wgs >= num_cus_ || (force != nullptr && std::atoi(force) == 0)) return 0;
			const int slices = std::min((num_cus_ - wgs) / nsuper, gram_wide_fused_parts(RP_, (int)len, gram_parts_));
			if (slices < 1) return 0;
			const long steps = ((len + 15) / 16 + slices - 1) / slices;
			const double chain_us = 5.0 + 0.75 * (double)steps;
			const double product_us = 6.0 + (double)nbk * sizeof(T) * (double)mpad_ * (double)npad_ / 3.2e6;      // (65 us per layer of 128 columns at config 2's shape)
			return (chain_us <= 0.8 * product_us || steps <= 8 || (force != nullptr && std::atoi(force) == 1)) ? slices : 0;
		};
		f32w_ride_h_ = ride(planHx_, m_);
		f32w_ride_w_ = ride(planWx_, n_);
	}
	fused64_planned_ = fused64_capable();
	if (fused64_planned_) {
		// Gram passengers of the two product launches (kernels_f64.hip, gram_ride_f64): as many K slices per 64 x 64 super-block as the product's grid leaves CUs for,
		// at most 16 (the level-1 finisher adds them one after the other), at least 4 (a grid that fills the chip: the passengers queue behind the product blocks)
		const int nbk = RP_ / 64, nsuper = nbk * (nbk + 1) / 2;
		auto slices = [&](const FactorProductPlan& p, long len) {
			const int room = (num_cus_ - (p.half_tiles ? 2 : 1) * p.xtiles * p.splits * p.chunks - nbk) / nsuper;
			const int by_len = (int)std::max<long>(1, (len + 3) / 4 / 16);       // (at least 8 K-steps of four rows per wave half)
			return std::max(1, std::min(std::min(16, by_len), std::max(4, room)));
		};
		f64_slices_h_ = slices(planH_, m_);      // W^T W beside W^T V
		f64_slices_w_ = slices(planW_, n_);      // H H^T beside V H^T
		if (tuning_env("NMFAMD_RIDE64_PID_ORDER") == nullptr) {      // (the passengers' XCD-aware work tables: built here, uploaded by allocate_buffers)
			gram_ride_f64_items(planH_, RP_, f64_slices_h_, f64_items_h_host_);
			gram_ride_f64_items(planW_, RP_, f64_slices_w_, f64_items_w_host_);
		}
		f64_stamps_wanted_ = tuning_env("NMFAMD_F64_STAMPS") != nullptr;
	}
	return ST_OK;
}

// Memory, zero fills (on stream_, in this order), the side stream and the events for what plan() decided.
template <typename T>
Status Engine<T>::allocate_buffers() {
	const long slab_elems = slab_stride_ * std::max(std::max(planH_.splits, planW_.splits), std::max(std::max(betaHb_.slabs, betaWb_.slabs), std::max(betaHr_.slabs, betaWr_.slabs)));
	const long panelW = (long)RP_ * mpad_, panelH = (long)RP_ * npad_, rr = (long)RP_ * RP_;
	auto dalloc = [&](T** p, long elems) { return buffers_.device(p, (size_t)elems * sizeof(T), true, stream_); };      // (zero-filled)
	auto bytes = [&](auto** p, size_t count, bool zero = false) { return buffers_.device(p, count, zero, stream_); };
	HIPX(hipGetDevice(&device_));      // (the device entries compare a caller's pointer against it)
	if (bf16_) {
		HIPX(bytes(&Vb_, 16 * (size_t)planW_.xtiles * ksW_ * 256));
		HIPX(bytes(&Vtb_, 16 * (size_t)planH_.xtiles * ksH_ * 256));
		{
			// (row-block sharded runs all-gather the fragments in place, world x blk_rows / 16 K-steps = mpad_ / 16 of them -- more than ksH_ whenever m is not a
			//  multiple of 128 x world (config 4's 50 000 rows on 8 ranks are padded to 50 176); the K-steps behind ksH_ are never read by a product and stay zero)
			const size_t ks_alloc = (size_t)std::max<long>(ksH_, mpad_ / 16);
			HIPX(bytes(&Wtb_, 16 * ks_alloc * (RP_ / 32) * 64));
			if (ks_alloc > (size_t)ksH_) HIPX(hipMemsetAsync((char*)Wtb_ + 16 * (size_t)ksH_ * (RP_ / 32) * 64, 0, 16 * (ks_alloc - (size_t)ksH_) * (RP_ / 32) * 64, stream_));
		}
		HIPX(bytes(&Hb_, 16 * (size_t)ksW_ * (RP_ / 32) * 64));
	} else if (!sparse_) {
		if (x3_) {
			// + 1: the all-zero K-step that closes the image (written here once; the update kernels never touch it)
			HIPX(bytes(&Wx3_, 3 * 16 * (size_t)(ksH_ + 1) * (RP_ / 32) * 64, true));
			HIPX(bytes(&Hx3_, 3 * 16 * (size_t)(ksW_ + 1) * (RP_ / 32) * 64, true));
		}
		HIPX(dalloc(&V_, elemsV_));
		if (!one_image_) HIPX(dalloc(&Vt_, elemsVt_));
	} else {
		HIPX(dalloc(&t_vwh_, mpad_));
		HIPX(dalloc(&t_kl_, mpad_));
		HIPX(dalloc(&rowsum_part_, (std::max(mpad_, npad_) / 128) * RP_));
		HIPX(dalloc(&sW_, RP_));
		HIPX(dalloc(&sH_, RP_));
		HIPX(dalloc(&kl_scale_, RP_));
		HIPX(buffers_.pinned(&pin_kl_, sizeof(T) * (2 * (size_t)m_ + 3 * (size_t)RP_)));
		if (prm_.is_masked()) HIPX(dalloc(&msq_part_, (long)(MASKED_NORM_PARTS + 16) * RP_));      // (+ 16: launch_normalize_panel's compaction scratch)
	}
	if (beta_dense_) {
		HIPX(dalloc(&t_vwh_, mpad_));
		HIPX(dalloc(&t_kl_, mpad_));
		// (minibatch: k_beta_update_rows leaves one vector of sums per BETA_ROWS_PER_WG rows, not per 128)
		HIPX(dalloc(&rowsum_part_, (std::max(mpad_, npad_) / (minibatch_ ? BETA_ROWS_PER_WG : 128)) * RP_));
		HIPX(dalloc(&sW_, RP_));
		HIPX(dalloc(&sH_, RP_));
		if (minibatch_) { HIPX(dalloc(&online_A_, (long)RP_ * mpad_)); HIPX(dalloc(&online_B_, (long)RP_ * mpad_)); }
		HIPX(dalloc(&beta_tpart_, 2l * BETA_MAX_SLABS * mpad_));
		if (beta_ != 1 || weighted_) HIPX(dalloc(&beta_den_, slab_elems));
		if (weighted_) { HIPX(dalloc(&Om_, elemsV_)); HIPX(dalloc(&Omt_, elemsVt_)); }
		HIPX(buffers_.pinned(&pin_kl_, sizeof(T) * (2 * (size_t)m_ + 3 * (size_t)RP_)));
	}
	HIPX(dalloc(&Wt_, panelW));
	HIPX(dalloc(&H_, panelH));
	// wide fp32 panels: scratch for the split image of the r x r matrix (zero: the closing all-zero K-step -- k_smooth_gram writes the others only)
	if (wide_q_image_) HIPX(bytes(&qx3_, 3 * 16 * (size_t)(RP_ / 16 + 1) * (RP_ / 32) * 64, true));
	HIPX(dalloc(&slabs_, slab_elems));
	HIPX(dalloc(&numW_, panelW));
	HIPX(dalloc(&G_, rr));
	HIPX(dalloc(&G2_, rr));
	HIPX(dalloc(&HHt_, rr));
	HIPX(dalloc(&Qinv_, rr));
	HIPX(dalloc(&gram_part_, rr * gram_parts_));
	HIPX(dalloc(&sumsq_part_, ((long)std::max({panel_update_parts(RP_, sizeof(T), (int)mpad_), (int)(mpad_ / panel_update_rows(RP_, sizeof(T))),
	                                           hals_family(alg_) ? family_parts((int)mpad_) : 0}) + 16) * RP_));
	if (hals_family(alg_)) {
		// the sweep (step) counts of the most recent H and W step (dynamic stopping, docs/HALS.md, docs/NENMF.md)
		HIPX(bytes(&hals_counts_h_, sizeof(int) * (size_t)npad_, true));
		HIPX(bytes(&hals_counts_w_, sizeof(int) * (size_t)mpad_, true));
	}
	// the two error-term vectors share one allocation (and one pinned landing buffer): ONE device-to-host copy per error iteration
	HIPX(dalloc(&psN_, ps_stride_ + RP_));
	psR_ = psN_ + ps_stride_;
	HIPX(dalloc(&stage_, std::max(mpad_, npad_) * RP_));
	HIPX(bytes(&range_flag_, sizeof(int)));
	if (tri_) {
		HIPX(bytes(&gram_tri_part_, sizeof(float) * (size_t)std::max<long>(gram_tri_partial_elems(num_cus_), (long)(TRI_PASSENGERS / 2) * 36 * 1024)));
		HIPX(bytes(&tri_ride_counters_, 64, true));
		HIPX(bytes(&Gw_raw_, sizeof(float) * (size_t)rr, true));
		HIPX(bytes(&Gh_raw_, sizeof(float) * (size_t)rr, true));
		HIPX(bytes(&colsq_, sizeof(float) * (size_t)RP_ * colsq_stage_parts(), true));
	}
	if (alg_ == ALG_NSNMF) {
		HIPX(dalloc(&Ws_, panelW));                       // (tri_: only get_factors() materialises W S)
		if (!tri_) HIPX(dalloc(&Hs_, panelH));
	}
	if (alg_ >= ALG_GDCLS && alg_ <= ALG_AHCLS) {
		HIPX(dalloc(&Wold_, panelW));
		HIPX(dalloc(&rowdot_part_, (long)ROW_DOT_GROUPS * RP_));
		HIPX(bytes(&inv_work_, sizeof(double) * 2 * (size_t)r_ * r_));
		if (overlap_inverse_) {
			HIPX(hipStreamCreateWithFlags(&aux_, hipStreamNonBlocking));
			HIPX(hipEventCreateWithFlags(&ev_fork_, hipEventDisableTiming));
			HIPX(hipEventCreateWithFlags(&ev_join_, hipEventDisableTiming));
		}
	}
#ifdef NMFAMD_DIAG_BUILD
	if (one_pass_) {
		HIPX(bytes(&op_part_, onepass_part_bytes()));
		HIPX(bytes(&op_hfrag_, onepass_hfrag_bytes()));
		HIPX(bytes(&op_ctl_, 64));
		HIPX(bytes(&op_slabs_, sizeof(float) * (size_t)ONEPASS_XCDS * RP_ * mpad_));
		HIPX(bytes(&op_hh_part_, sizeof(float) * 4096 * (size_t)(ONEPASS_XCDS * ONEPASS_GROUP)));
		HIPX(bytes(&op_ps4_, sizeof(float) * 4 * (size_t)npad_));
		HIPX(dalloc(&op_H2_, panelH));
		HIPX(hipMemsetAsync(op_ps4_, 0, sizeof(float) * 4 * (size_t)npad_, stream_));
		HIPX(hipMemsetAsync(op_part_, 0, onepass_part_bytes(), stream_));
		HIPX(hipMemsetAsync(op_hfrag_, 0, onepass_hfrag_bytes(), stream_));
		HIPX(hipMemsetAsync(op_ctl_, 0, 64, stream_));
		HIPX(hipMemsetAsync(op_slabs_, 0, sizeof(float) * (size_t)ONEPASS_XCDS * RP_ * mpad_, stream_));
		HIPX(buffers_.pinned(&pin_abort_, sizeof(unsigned)));
		*pin_abort_ = 0;
		op_seq_ = 0;
		if (op_stamps_wanted_) HIPX(bytes(&op_stamps_, sizeof(unsigned long long) * 16 * 8 * ONEPASS_XCDS * ONEPASS_GROUP, true));
	}
#endif
	if (fused_capable() || gram_from_update()) {
		HIPX(bytes(&gramW_part_, sizeof(float) * 4096 * (size_t)(mpad_ / 64)));
		HIPX(bytes(&Graw64_, sizeof(float) * 4096));      // the reduced, unscaled W^T W of normalize_w's one-launch form
		HIPX(bytes(&gramH_part_, sizeof(float) * 4096 * (size_t)(npad_ / 64)));
		HIPX(bytes(&scale_, sizeof(float) * 64));
		HIPX(bytes(&Gpart_, sizeof(float) * 4096 * GRAM_KSPLIT_MAX, true));      // (spread form: a tile's absent pieces are never written)
		HIPX(bytes(&gram_spread_counter_, 64, true));
		HIPX(bytes(&wsq_part_, sizeof(float) * 64 * (size_t)(mpad_ / 32), true));
	}
	if (fused32w_planned_) HIPX(bytes(&f32w_scale_, sizeof(float) * (size_t)RP_, true));
	if (fused64_planned_) {
		const int nbk = RP_ / 64, nsuper = nbk * (nbk + 1) / 2;
		HIPX(bytes(&f64_scale_, sizeof(double) * (size_t)RP_));
		HIPX(bytes(&f64_partial_, sizeof(double) * 4096 * (size_t)nsuper * (size_t)std::max(f64_slices_h_, f64_slices_w_)));
		HIPX(bytes(&f64_counters_, sizeof(unsigned) * (size_t)(nsuper + 1), true));
		auto table = [&](int** dev, std::vector<int>& host) {      // (empty: NMFAMD_RIDE64_PID_ORDER, no work tables)
			hipError_t e = host.empty() ? hipSuccess : bytes(dev, sizeof(int) * host.size());
			if (e == hipSuccess && !host.empty()) e = hipMemcpy(*dev, host.data(), sizeof(int) * host.size(), hipMemcpyHostToDevice);
			std::vector<int>().swap(host);
			return e;
		};
		HIPX(table(&f64_items_h_, f64_items_h_host_));
		HIPX(table(&f64_items_w_, f64_items_w_host_));
		if (f64_stamps_wanted_) HIPX(bytes(&f64_stamps_, sizeof(unsigned long long) * 4 * 4096 * 8, true));
	}
	HIPX(buffers_.pinned(&pin_psN_, sizeof(T) * (size_t)(ps_stride_ + RP_)));
	pin_psR_ = pin_psN_ + ps_stride_;
	{
		void* dp = nullptr;       // the device's view of the pinned buffer (fetch_error_terms writes it from a kernel)
		if (hipHostGetDevicePointer(&dp, pin_psN_, 0) == hipSuccess) pin_psN_dev_ = static_cast<T*>(dp); else { (void)hipGetLastError(); pin_psN_dev_ = nullptr; }
	}
	HIPX(hipEventCreateWithFlags(&err_event_, hipEventDisableTiming));
	HIPX(hipStreamSynchronize(stream_));
	return ST_OK;
}

// ---- upload / download --------------------------------------------------------------------

// Column-major staging image of V (ld = mpad_) -> the resident images and the tr(V^T V) terms.
// MFMA path (fp32): V_ and Vt_ are x-TILED (kernels.hip, k_factor_product_f32); the staging image
// is a temporary.  Generic path: V_ IS the column-major image and Vt_ its plain transpose.
template <typename T>
Status Engine<T>::finish_upload(T* Vcol) {
	int odd_values = 0;
	state_.v_replaced();
	HIPX(hipMemsetAsync(range_flag_, 0, sizeof(int), stream_));
	HIPX(launch_column_sumsq<T>(Vcol, mpad_, m_, n_, psN_, stream_, x3_ ? range_flag_ : nullptr));
	h_vtv_.resize(n_);
	HIPX(hipMemcpyAsync(h_vtv_.data(), psN_, sizeof(T) * n_, hipMemcpyDeviceToHost, stream_));
	HIPX(hipMemcpyAsync(&odd_values, range_flag_, sizeof(int), hipMemcpyDeviceToHost, stream_));
	if (bf16_) {
		if constexpr (std::is_same<T, float>::value) {
			HIPX(launch_pack_stream_bf16(Vcol, mpad_, m_, n_, false, Vb_, planW_.xtiles, ksW_, stream_));
			HIPX(launch_pack_stream_bf16(Vcol, mpad_, n_, m_, true, Vtb_, planH_.xtiles, ksH_, stream_));
		}
	} else if (tiled_) {
		HIPX(hipMemsetAsync(V_, 0, sizeof(T) * (size_t)elemsV_, stream_));
		HIPX(launch_tile<T>(Vcol, mpad_, m_, n_, V_, strideV_, img_th_, false, stream_));
		if (!one_image_) {
			HIPX(hipMemsetAsync(Vt_, 0, sizeof(T) * (size_t)elemsVt_, stream_));
			HIPX(launch_tile_transposed<T>(Vcol, mpad_, m_, n_, Vt_, strideVt_, planH_.th, stream_));
		}
	} else {
		HIPX(launch_transpose<T>(Vcol, mpad_, m_, n_, Vt_, npad_, stream_));
	}
	HIPX(hipStreamSynchronize(stream_));
	std::sort(h_vtv_.begin(), h_vtv_.end());
	if (x3_ && odd_values != 0) {
		last_error_ = "V holds values outside the exact range of the split-operand product (not finite, |v| > 2^126 or 0 < |v| < 2^-100): use precision = -1";
		return ST_VALUE_RANGE;
	}
	return ST_OK;
}

template <typename T>
Status Engine<T>::upload_dense(const T* V, long ld) {
	if (!V || ld < m_) return ST_INVALID;
	if (weighted_) { last_error_ = "weighted NMF: V is uploaded together with its weights (upload_dense_weighted)"; return ST_INVALID; }
	if (beta_dense_) {
		beta_uploaded_ = false;
		if (Status st = beta_check_values(V, n_, ld, m_)) return st;
	}
	if (sparse_ && prm_.is_masked()) {
		// missing values: every entry that is not NaN is observed -- zeros included -- and becomes a stored entry
		std::vector<int> rows, cols; std::vector<T> vals;
		for (int j = 0; j < n_; ++j)
			for (int i = 0; i < m_; ++i) {
				const T v = V[(size_t)j * ld + i];
				if (std::isnan(v)) continue;
				if (!std::isfinite(v)) { last_error_ = "missing values: V holds an infinite value (NaN marks a missing entry)"; return ST_INVALID; }
				if (masked_beta_ && (v < T(0) || (mbeta_ <= 0 && v == T(0)))) { last_error_ = masked_value_fault(); return ST_INVALID; }
				rows.push_back(i); cols.push_back(j); vals.push_back(v);
			}
		if (vals.empty()) { last_error_ = "missing values: V has no observed entry"; return ST_INVALID; }
		return upload_triplets(rows, cols, vals);
	}
	if (sparse_) {
		// dense input on the sparse path: the non-zero entries become the stored entries
		std::vector<int> rows, cols; std::vector<T> vals;
		for (int j = 0; j < n_; ++j)
			for (int i = 0; i < m_; ++i) {
				const T v = V[(size_t)j * ld + i];
				if (v != T(0)) { rows.push_back(i); cols.push_back(j); vals.push_back(v); }
			}
		return upload_triplets(rows, cols, vals);
	}
	return upload_image(true, [&](T* Vcol) {
		HIPX(hipMemcpy2DAsync(Vcol, mpad_ * sizeof(T), V, ld * sizeof(T), m_ * sizeof(T), n_, hipMemcpyHostToDevice, stream_));
		return ST_OK;
	});
}

// Every dense upload behind its checks: the column-major image (V_, or a staging buffer where the resident images are tiled or bf16; zeroed: the fill leaves gaps), its fill, finish_upload()
template <typename T> template <typename Fill>
Status Engine<T>::upload_image(bool zeroed, Fill fill) {
	DeviceBuffers staging;      // freed on every way out
	T* Vcol = V_;
	if (tiled_ || bf16_) HIPX(staging.device(&Vcol, sizeof(T) * (size_t)(mpad_ * npad_), zeroed, stream_));
	if (Status st = fill(Vcol)) return st;
	if (Status st = finish_upload(Vcol)) return st;
	if (beta_dense_) beta_uploaded_ = true;
	return ST_OK;
}

// Weighted engines: V and its weights.  The values are checked jointly on the host (the weights alone, then V where its weight is > 0), the sum of the weights is
// taken in double, and V goes to the device with 0 wherever its weight is 0, so that nothing that is not finite ever sits in a resident image (the kernels
// mask by the weight all the same).  Four images: V_ / Om_ column-major, Vt_ / Omt_ their transposes.
template <typename T>
Status Engine<T>::upload_dense_weighted(const T* V, long ldv, const T* Omega, long ldo) {
	if (!weighted_) { last_error_ = "weighted upload: the engine was not created with 'weighted' = 1"; return ST_INVALID; }
	if (!V || !Omega || ldv < m_ || ldo < m_) return ST_INVALID;
	beta_uploaded_ = false;
	double sum_w = 0;
	int seen = 0;      // (IMPORT_SOME_WEIGHT once a weight > 0 was met)
	std::vector<T> clean((size_t)m_ * (size_t)n_);
	for (long j = 0; j < n_; ++j)
		for (long i = 0; i < m_; ++i) {
			const T w = Omega[(size_t)j * ldo + i];
			if (!std::isfinite(w) || w < T(0)) return refuse_weighted(IMPORT_BAD_WEIGHT);
			T v = T(0);
			if (w > T(0)) {
				v = V[(size_t)j * ldv + i];
				if (!std::isfinite(v) || v < T(0) || (beta_ <= 0 && v == T(0))) return refuse_weighted(IMPORT_BAD_VALUE);
				seen = IMPORT_SOME_WEIGHT;
				sum_w += (double)w;
			}
			clean[(size_t)j * m_ + i] = v;
		}
	if (Status st = refuse_weighted(seen)) return st;
	HIPX(hipMemcpy2DAsync(V_, mpad_ * sizeof(T), clean.data(), m_ * sizeof(T), m_ * sizeof(T), n_, hipMemcpyHostToDevice, stream_));
	HIPX(hipMemcpy2DAsync(Om_, mpad_ * sizeof(T), Omega, ldo * sizeof(T), m_ * sizeof(T), n_, hipMemcpyHostToDevice, stream_));
	return finish_weighted_upload(sum_w);
}

// What both forms of the weighted upload refuse, by the flags of kernels_import.hip in their precedence (the host form stops at the first bad element: one flag)
template <typename T>
Status Engine<T>::refuse_weighted(int flags) {
	if (flags & IMPORT_BAD_WEIGHT) last_error_ = "weighted NMF: every weight has to be finite and >= 0";
	else if (flags & IMPORT_BAD_VALUE) last_error_ = beta_ <= 0 ? "weighted NMF with beta <= 0: every entry of V with a weight > 0 has to be finite and > 0"
	                                                            : "weighted NMF with beta > 0: every entry of V with a weight > 0 has to be finite and >= 0";
	else if (!(flags & IMPORT_SOME_WEIGHT)) last_error_ = "weighted NMF: at least one weight has to be > 0";
	else return ST_OK;
	return ST_INVALID;
}

// ... and what both forms end with, V_ and Om_ holding the column-major images: the resident images and the error terms of V, the transpose of the weights
template <typename T>
Status Engine<T>::finish_weighted_upload(double sum_w) {
	if (Status st = finish_upload(V_)) return st;      // (V_ is the column-major image; Vt_ its transpose; synchronises)
	HIPX(launch_transpose<T>(Om_, mpad_, m_, n_, Omt_, npad_, stream_));
	HIPX(hipStreamSynchronize(stream_));
	sum_w_ = sum_w; beta_uploaded_ = true;
	return ST_OK;
}

// The dense beta-divergence update's demand on V: every entry finite, and > 0 at beta <= 0 (such a divergence is undefined at 0) or >= 0 at beta > 0
template <typename T>
Status Engine<T>::beta_check_values(const T* values, long count, long ld, long rows) {
	const bool is = beta_ <= 0;
	for (long j = 0; j < count; ++j)
		for (long i = 0; i < rows; ++i) {
			const T v = values[(size_t)j * ld + i];
			if (!std::isfinite(v) || v < T(0) || (is && v == T(0))) { last_error_ = beta_value_fault(); return ST_INVALID; }
		}
	return ST_OK;
}

template <typename T>
const char* Engine<T>::beta_value_fault() const {
	return beta_ == 0   ? "Itakura-Saito divergence: every entry of V has to be finite and > 0"
	       : beta_ == 1 ? "dense KL divergence: every entry of V has to be finite and >= 0"
	       : beta_ <= 0 ? "beta-divergence with beta <= 0: every entry of V has to be finite and > 0"
	                    : "beta-divergence with beta > 0: every entry of V has to be finite and >= 0";
}

// ---- device-resident input and output (docs/DEVICE_IO.md) ---------------------------------------

void device_pointer_info(const void* p, int* kind, int* device, unsigned long long* bytes_from_p) {
	*kind = 0; *device = -1; *bytes_from_p = 0;
	if (p == nullptr) return;
	hipPointerAttribute_t attr;
	std::memset(&attr, 0, sizeof(attr));
	if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return; }      // (older runtimes answer an ordinary host pointer with an error)
	if (attr.type == hipMemoryTypeUnregistered) return;
	*device = attr.device;
	if (attr.type == hipMemoryTypeHost) { *kind = 2; return; }
	if (attr.type != hipMemoryTypeDevice || attr.isManaged) { *kind = 3; return; }
	*kind = 1;
	hipDeviceptr_t base = nullptr; size_t size = 0;
	if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess) { (void)hipGetLastError(); return; }
	const uintptr_t b = (uintptr_t)base, q = (uintptr_t)p;
	if (q >= b && q - b < size) *bytes_from_p = (unsigned long long)(size - (q - b));
}

template <typename T>
Status Engine<T>::check_device_matrix(const char* name, const void* p, long ld, int layout, long rows, long cols) {
	const std::string n(name);
	if (p == nullptr) return refuse(n + ": null pointer");
	if (layout != 0 && layout != 1) return refuse(n + ": layout has to be 0 (column-major) or 1 (row-major)");
	const long inner = layout == 0 ? rows : cols, outer = layout == 0 ? cols : rows;
	if (ld < inner) return refuse(n + ": leading dimension below the " + (layout == 0 ? "row count (column-major)" : "column count (row-major)"));
	const unsigned long long elems = outer > 0 ? (unsigned long long)(outer - 1) * (unsigned long long)ld + (unsigned long long)inner : 0;
	return check_device_extent(n, p, sizeof(T), elems, "the extent (outer - 1) * ld + inner");
}

// ... of a caller's device array of `count` elements (a null pointer is taken where count is 0)
template <typename T>
Status Engine<T>::check_device_vector(const char* name, const void* p, size_t elem, long count) {
	const std::string n(name);
	if (count <= 0) return ST_OK;
	if (p == nullptr) return refuse(n + ": null pointer");
	return check_device_extent(n, p, elem, (unsigned long long)count, "the array of " + std::to_string(count) + " elements");
}

// What both have in common, over the element size: p (not null) is aligned to `elem`, device memory of the engine's device, and `elems` elements from p lie inside
// its allocation
template <typename T>
Status Engine<T>::check_device_extent(const std::string& n, const void* p, size_t elem, unsigned long long elems, const std::string& extent) {
	if ((uintptr_t)p % elem != 0) return refuse(n + ": pointer not aligned to the element size");
	int kind = 0, dev = -1; unsigned long long avail = 0;
	device_pointer_info(p, &kind, &dev, &avail);
	if (kind == 0) return refuse(n + ": not device memory (a pointer the HIP runtime does not know: host memory goes through the host entry)");
	if (kind == 2) return refuse(n + ": not device memory (pinned host memory goes through the host entry)");
	if (kind != 1) return refuse(n + ": not device memory (managed or array memory is not taken)");
	if (dev != device_) return refuse(n + ": memory of another device than the engine's");
	if (elems > 0 && elems * elem > avail) return refuse(n + ": " + extent + " reaches past the end of the allocation");
	return ST_OK;
}

template <typename T>
Status Engine<T>::upload_dense_device(const T* V, long ld, int layout) {
	if (weighted_) { last_error_ = "weighted NMF: V is uploaded together with its weights (upload_dense_weighted)"; return ST_INVALID; }
	if (sparse_) { last_error_ = "device upload: an engine with 'sparseCompute' or 'missingValues' builds its triplets on the host and takes dense input from host memory only"; return ST_INVALID; }
	if (Status st = check_device_matrix("V", V, ld, layout, m_, n_)) return st;
	if (beta_dense_) beta_uploaded_ = false;
	HIPX(hipDeviceSynchronize());      // whatever stream produced V has finished
	return upload_image(false, [&](T* Vcol) {      // (not zeroed: the import writes every element of the image)
		const int rule = beta_dense_ ? (beta_ <= 0 ? 2 : 1) : 0;
		int flags = 0;
		if (rule != 0) HIPX(hipMemsetAsync(range_flag_, 0, sizeof(int), stream_));
		HIPX(launch_import_dense<T>(V, ld, layout, m_, n_, Vcol, mpad_, mpad_, npad_, rule, range_flag_, stream_));
		if (rule != 0) { HIPX(hipMemcpyAsync(&flags, range_flag_, sizeof(int), hipMemcpyDeviceToHost, stream_)); HIPX(hipStreamSynchronize(stream_)); }
		if (flags & IMPORT_BAD_VALUE) { last_error_ = beta_value_fault(); return ST_INVALID; }
		return ST_OK;
	});
}

template <typename T>
Status Engine<T>::upload_dense_weighted_device(const T* V, long ldv, int layout_v, const T* Omega, long ldo, int layout_o) {
	if (!weighted_) { last_error_ = "weighted upload: the engine was not created with 'weighted' = 1"; return ST_INVALID; }
	if (Status st = check_device_matrix("V", V, ldv, layout_v, m_, n_)) return st;
	if (Status st = check_device_matrix("Omega", Omega, ldo, layout_o, m_, n_)) return st;
	beta_uploaded_ = false;
	HIPX(hipDeviceSynchronize());
	const long parts = import_weighted_parts(mpad_, npad_);
	DeviceBuffers scratch;      // freed on every way out
	double* part = nullptr;
	HIPX(scratch.device(&part, sizeof(double) * (size_t)parts, false, stream_));
	std::vector<double> h_part((size_t)parts);
	int flags = 0;
	HIPX(hipMemsetAsync(range_flag_, 0, sizeof(int), stream_));
	HIPX(launch_import_weighted<T>(V, ldv, layout_v, Omega, ldo, layout_o, m_, n_, V_, Om_, mpad_, mpad_, npad_, beta_ <= 0 ? 1 : 0, range_flag_, part, stream_));
	HIPX(hipMemcpyAsync(&flags, range_flag_, sizeof(int), hipMemcpyDeviceToHost, stream_));
	HIPX(hipMemcpyAsync(h_part.data(), part, sizeof(double) * (size_t)parts, hipMemcpyDeviceToHost, stream_));
	HIPX(hipStreamSynchronize(stream_));
	if (Status st = refuse_weighted(flags)) return st;
	double sum_w = 0;
	for (long i = 0; i < parts; ++i) sum_w += h_part[(size_t)i];      // in index order: a function of the input and the shape only
	return finish_weighted_upload(sum_w);
}

template <typename T>
Status Engine<T>::set_factors_device(const T* W, long ldw, int layout_w, const T* H, long ldh, int layout_h) {
	if (W) { if (Status st = check_device_matrix("W", W, ldw, layout_w, m_, r_)) return st; }
	if (H) { if (Status st = check_device_matrix("H", H, ldh, layout_h, r_, n_)) return st; }
	state_.factors_touched();
	HIPX(hipDeviceSynchronize());
	if (W) { state_.w_set(); have_w_ = true; HIPX(launch_import_panel<T>(W, ldw, layout_w, true, r_, m_, Wt_, RP_, mpad_, stream_)); }
	if (H) { state_.h_set(); have_h_ = true; HIPX(launch_import_panel<T>(H, ldh, layout_h, false, r_, n_, H_, RP_, npad_, stream_)); }
	HIPX(hipStreamSynchronize(stream_));
	return ST_OK;
}

template <typename T>
Status Engine<T>::get_factors_device(T* W, long ldw, int layout_w, T* H, long ldh, int layout_h) {
	if (W) { if (Status st = check_device_matrix("W", W, ldw, layout_w, m_, r_)) return st; }
	if (H) { if (Status st = check_device_matrix("H", H, ldh, layout_h, r_, n_)) return st; }
	HIPX(hipDeviceSynchronize());      // (no stream still writes or reads the destination)
	const T* src = nullptr;
	if (Status s = export_panel_w(W != nullptr, &src)) return s;
	if (W) HIPX(launch_export_panel<T>(src, RP_, mpad_, true, r_, m_, W, ldw, layout_w, stream_));
	if (H) HIPX(launch_export_panel<T>(H_, RP_, npad_, false, r_, n_, H, ldh, layout_h, stream_));
	HIPX(hipStreamSynchronize(stream_));
	return ST_OK;
}

template <typename T>
Status Engine<T>::upload_sparse(int format, const T* values, const int* a, const int* b, long nnz, int base) {
	if (nnz > 0 && (!values || !a || !b)) return ST_INVALID;
	if (Status st = refuse_sparse_input(format, nnz)) return st;
	if (beta_dense_) {
		beta_uploaded_ = false;
		if (nnz > 0) { if (Status st = beta_check_values(values, 1, nnz, nnz)) return st; }
	}
	if (sparse_ && prm_.is_masked()) {
		// missing values: every stored entry is observed (stored zeros too, which both image builders keep); its value must be finite, and there must be one
		if (nnz == 0) return refuse_sparse_values(SPARSE_NO_ENTRY);
		for (long p = 0; p < nnz; ++p)
			if (!std::isfinite(values[p]) || (masked_beta_ && (values[p] < T(0) || (mbeta_ <= 0 && values[p] == T(0))))) return refuse_sparse_values(IMPORT_BAD_VALUE);
	}
	if (sparse_) {
		// the images are built on the device (kernels_sparse_setup.hip); what that path does not cover -- entries outside the matrix (dropped by the host path), pointer
		// arrays that do not ascend, a row or column longer than its LDS sort takes, no entries at all -- and NMFAMD_SPARSE_SETUP=host take the host path
		if (!sparse_setup_on_host() && nnz > 0) {
			bool fallback = false;
			const Status st = upload_sparse_device(format, values, a, b, nnz, base, &fallback);
			if (!fallback) return st;
		}
		return upload_sparse_on_host(format, values, a, b, nnz, base);
	}
	DeviceBuffers scratch;      // the caller's arrays on the device: freed on every way out
	T* d_val = nullptr; int *d_a = nullptr, *d_b = nullptr;
	const int outer = format == 1 ? m_ : n_;
	const long na = format == 3 ? nnz : (long)outer + 1;
	HIPX(scratch.device(&d_val, sizeof(T) * (size_t)std::max<long>(nnz, 1), false, stream_));
	HIPX(scratch.device(&d_a, sizeof(int) * (size_t)std::max<long>(na, 1), false, stream_));
	HIPX(scratch.device(&d_b, sizeof(int) * (size_t)std::max<long>(nnz, 1), false, stream_));
	if (nnz > 0) {
		HIPX(hipMemcpyAsync(d_val, values, sizeof(T) * nnz, hipMemcpyHostToDevice, stream_));
		HIPX(hipMemcpyAsync(d_b, b, sizeof(int) * nnz, hipMemcpyHostToDevice, stream_));
	}
	if (na > 0) HIPX(hipMemcpyAsync(d_a, a, sizeof(int) * na, hipMemcpyHostToDevice, stream_));
	return upload_image(false, [&](T* Vcol) {      // (not zeroed: cleared here, V_ included where it is the image)
		HIPX(hipMemsetAsync(Vcol, 0, sizeof(T) * (size_t)(mpad_ * npad_), stream_));
		// CSR: ptr = a (rowPtr), idx = b (columns); CSC: ptr = a (columnPtr), idx = b (rows); COO: idx = a (rows), idx2 = b (columns)
		if (format == 3) HIPX(launch_densify<T>(3, d_val, nullptr, d_a, d_b, nnz, 0, base, Vcol, mpad_, m_, n_, stream_));
		else HIPX(launch_densify<T>(format, d_val, d_a, d_b, nullptr, nnz, outer, base, Vcol, mpad_, m_, n_, stream_));
		return ST_OK;
	});
}

// The CSR and CSC images built on the device from the caller's arrays as they are (kernels_sparse_setup.hip; reference: the device-side conversions of
// source/common/Matrix.h:145-232).  *fallback: the input needs the host path (nothing of this engine's state has been touched then, except freed images).
template <typename T>
Status Engine<T>::upload_sparse_device(int format, const T* values, const int* a, const int* b, long nnz, int base, bool* fallback) {
	return build_sparse_images(format, nnz, base, fallback, [&](T* d_val, size_t nv, int* d_a, size_t na, int* d_b, size_t nb) {
		HIPX(hipMemcpyAsync(d_val, values, nv, hipMemcpyHostToDevice, stream_));
		HIPX(hipMemcpyAsync(d_a, a, na, hipMemcpyHostToDevice, stream_));
		HIPX(hipMemcpyAsync(d_b, b, nb, hipMemcpyHostToDevice, stream_));
		return ST_OK;
	});
}

// ... behind the copies: fill(d_val, bytes, d_a, bytes, d_b, bytes) brings the caller's arrays (host memory: upload_sparse; device memory: upload_sparse_from_device)
// into device arrays this body owns -- which is what lets it adopt them as the CSR image where the input already is one
template <typename T> template <typename Fill>
Status Engine<T>::build_sparse_images(int format, long nnz, int base, bool* fallback, Fill fill) {
	*fallback = false;
	if (nnz >= (1l << 31)) return ST_INVALID;
	const int outer = format == 1 ? m_ : n_;
	const long na = format == 3 ? nnz : (long)outer + 1;
	const int segs = std::max(m_, n_);
	// scratch: freed on every way out
	T* d_val = nullptr;
	int *d_a = nullptr, *d_b = nullptr, *row = nullptr, *col = nullptr, *items = nullptr, *rowq = nullptr, *counts = nullptr, *small = nullptr;
	DeviceBuffers scratch;
	auto alloc = [&](auto** p, size_t bytes) { return scratch.device(p, std::max<size_t>(bytes, 16), false, stream_); };
	auto image = [&](auto** p, size_t bytes) { return buffers_.device(p, bytes, false, stream_); };      // (a part of the engine's CSR / CSC images)
	auto need_host = [&]() { *fallback = true; return ST_OK; };

	buffers_.release(csr_ptr_, csr_idx_, csc_ptr_, csc_idx_, csc_from_csr_, csr_val_, csc_val_, q_, q2_);
	nnz_ = 0;

	const size_t ni = sizeof(int) * (size_t)nnz, nv = sizeof(T) * (size_t)nnz;
	HIPX(alloc(&d_val, nv)); HIPX(alloc(&d_a, sizeof(int) * (size_t)na)); HIPX(alloc(&d_b, ni));
	HIPX(alloc(&row, ni)); HIPX(alloc(&col, ni));
	HIPX(alloc(&counts, sizeof(int) * (size_t)segs)); HIPX(alloc(&small, sizeof(int) * 4));
	if (Status st = fill(d_val, nv, d_a, sizeof(int) * (size_t)na, d_b, ni)) return st;
	HIPX(hipMemsetAsync(small, 0, sizeof(int) * 4, stream_));
	int* flags = small;                       // [0] flags, [1] longest row, [2] longest column
	HIPX(launch_sp_expand(format, d_a, d_b, nnz, outer, base, m_, n_, row, col, flags, stream_));
	HIPX(image(&csr_ptr_, sizeof(int) * (size_t)(m_ + 1)));
	HIPX(image(&csc_ptr_, sizeof(int) * (size_t)(n_ + 1)));
	HIPX(launch_sp_histogram_scan(row, nnz, m_, counts, csr_ptr_, small + 1, stream_));
	int h_small[4] = {0, 0, 0, 0};
	HIPX(hipMemcpyAsync(h_small, small, sizeof(int) * 4, hipMemcpyDeviceToHost, stream_));
	HIPX(hipStreamSynchronize(stream_));
	if ((h_small[0] & 3) != 0) return need_host();
	scratch.release(d_a, d_b);

	HIPX(alloc(&items, ni));
	if ((h_small[0] & 4) != 0) {
		// not in (row, column) order (COO, CSC, an unsorted CSR): the entries' positions by row, every row by (column, position)
		if (h_small[1] > sp_segment_sort_capacity()) return need_host();
		HIPX(alloc(&rowq, ni));
		HIPX(image(&csr_idx_, ni)); HIPX(image(&csr_val_, nv));
		HIPX(launch_sp_scatter_sort(row, nnz, m_, csr_ptr_, counts, items, col, h_small[1], stream_));
		HIPX(launch_sp_gather_csr<T>(items, row, col, d_val, nnz, csr_idx_, csr_val_, rowq, stream_));
	} else {
		// the input IS the CSR image (0-based by now): its buffers are adopted as they are
		csr_idx_ = col; buffers_.adopt(scratch, col);
		csr_val_ = d_val; buffers_.adopt(scratch, d_val); d_val = nullptr;
		rowq = row;
	}
	HIPX(launch_sp_histogram_scan(csr_idx_, nnz, n_, counts, csc_ptr_, small + 2, stream_));
	HIPX(hipMemcpyAsync(h_small, small, sizeof(int) * 4, hipMemcpyDeviceToHost, stream_));
	HIPX(hipStreamSynchronize(stream_));
	if (h_small[2] > sp_segment_sort_capacity()) return need_host();
	// the CSR positions by column, every column's list ascending = ascending row, duplicates in CSR order
	HIPX(launch_sp_scatter_sort(csr_idx_, nnz, n_, csc_ptr_, counts, items, nullptr, h_small[2], stream_));
	HIPX(image(&csc_idx_, ni)); HIPX(image(&csc_val_, nv));
	HIPX(launch_sp_gather_csc<T>(items, rowq, csr_val_, nnz, csc_idx_, csc_val_, stream_));
	const bool two_pass = tuning_env("NMFAMD_KL_TWO_PASS") != nullptr;      // (round 1's two-pass KL step, a measurement switch: quotient buffers + the CSR -> CSC permutation)
	if (two_pass) { csc_from_csr_ = items; buffers_.adopt(scratch, items); HIPX(image(&q_, nv)); HIPX(image(&q2_, nv)); }
	return finish_sparse_images(nnz);
}

// What every device-side builder of the sparse images ends with (build_sparse_images, upload_dense_device_stored), the images in place:
// tr(V^T V) terms per column (accumulated in T like the trace kernel, in the image's order) and sum(V) for the KL divergence, nnz_, the blocked KL gather
template <typename T>
Status Engine<T>::finish_sparse_images(long nnz) {
	DeviceBuffers scratch;      // freed on every way out
	T* d_vtv = nullptr;
	double* d_colsum = nullptr;
	auto alloc = [&](auto** p, size_t bytes) { return scratch.device(p, std::max<size_t>(bytes, 16), false, stream_); };
	HIPX(alloc(&d_vtv, sizeof(T) * (size_t)n_)); HIPX(alloc(&d_colsum, sizeof(double) * (size_t)n_));
	HIPX(launch_sp_col_sumsq<T>(csc_ptr_, csc_val_, n_, d_vtv, d_colsum, stream_));
	h_vtv_.assign(n_, T(0));
	std::vector<double> colsum((size_t)n_);
	HIPX(hipMemcpyAsync(h_vtv_.data(), d_vtv, sizeof(T) * (size_t)n_, hipMemcpyDeviceToHost, stream_));
	HIPX(hipMemcpyAsync(colsum.data(), d_colsum, sizeof(double) * (size_t)n_, hipMemcpyDeviceToHost, stream_));
	HIPX(hipStreamSynchronize(stream_));
	std::sort(h_vtv_.begin(), h_vtv_.end());
	sum_v_ = 0;
	for (int j = 0; j < n_; ++j) sum_v_ += colsum[j];
	nnz_ = nnz;
	sparse_setup_on_device_ = true;
	if (Status st = setup_kl_blocks()) return st;
	HIPX(hipStreamSynchronize(stream_));
	return ST_OK;
}

// What both forms of the sparse upload refuse before they look at an array: a format other than 1 ... 3 or nnz < 0 (no text), a weighted engine, a dense divergence
// engine with beta <= 0 (which is then without a valid V, as after any refused upload of such an engine)
template <typename T>
Status Engine<T>::refuse_sparse_input(int format, long nnz) {
	if (format < 1 || format > 3 || nnz < 0) return ST_INVALID;
	if (weighted_) { last_error_ = "weighted NMF: sparse input is refused; upload V dense together with its weights (upload_dense_weighted)"; return ST_INVALID; }
	if (beta_dense_ && beta_ <= 0) {
		// the stored entries are densified (launch_densify); an unstored entry is a zero, which a divergence with beta <= 0 (Itakura-Saito) does not take
		beta_uploaded_ = false;
		last_error_ = beta_ == 0 ? "Itakura-Saito divergence: sparse input is refused (unstored entries are zeros); upload V dense"
		                         : "beta-divergence with beta <= 0: sparse input is refused (unstored entries are zeros); upload V dense";
		return ST_INVALID;
	}
	return ST_OK;
}

// ... and the value rules of a missing-values engine, by what was found (the host loop, or the flags of kernels_compact.hip)
template <typename T>
Status Engine<T>::refuse_sparse_values(int found) {
	last_error_ = (found & SPARSE_NO_ENTRY) ? "missing values: no stored entry" : masked_beta_ ? masked_value_fault() : "missing values: a stored value is not finite";
	return ST_INVALID;
}

// The demand of a masked divergence engine on the stored values: finite, and > 0 at beta <= 0 (such a divergence is undefined at 0: a stored zero is refused) or >= 0
// at beta > 0 (a stored zero is an observation)
template <typename T>
const char* Engine<T>::masked_value_fault() const {
	return mbeta_ <= 0 ? "missing values with beta <= 0: every stored value has to be finite and > 0"
	                   : "missing values with beta > 0: every stored value has to be finite and >= 0";
}

template <typename T>
bool Engine<T>::sparse_setup_on_host() const {
	const char* where = std::getenv("NMFAMD_SPARSE_SETUP");
	return where != nullptr && std::strcmp(where, "host") == 0;
}

// The host path of a sparse upload on a sparse engine, from host arrays: triplets, then the host's counting sorts
template <typename T>
Status Engine<T>::upload_sparse_on_host(int format, const T* values, const int* a, const int* b, long nnz, int base) {
	sparse_setup_on_device_ = false;
	// expand to 0-based (row, column, value) triplets with the caller's index base applied exactly
	// (reference: cusparseSetMatIndexBase, Matrix.h:158-160,184-186,215-217); out-of-range entries are dropped
	std::vector<int> rows, cols; std::vector<T> vals;
	rows.reserve(nnz); cols.reserve(nnz); vals.reserve(nnz);
	auto push = [&](long i, long j, T v) { if (i >= 0 && i < m_ && j >= 0 && j < n_) { rows.push_back((int)i); cols.push_back((int)j); vals.push_back(v); } };
	if (format == 1) { for (int i = 0; i < m_; ++i) for (long p = (long)a[i] - base; p < (long)a[i + 1] - base && p < nnz; ++p) if (p >= 0) push(i, (long)b[p] - base, values[p]); }
	else if (format == 2) { for (int j = 0; j < n_; ++j) for (long p = (long)a[j] - base; p < (long)a[j + 1] - base && p < nnz; ++p) if (p >= 0) push((long)b[p] - base, j, values[p]); }
	else { for (long p = 0; p < nnz; ++p) push((long)a[p] - base, (long)b[p] - base, values[p]); }
	if (prm_.is_masked() && vals.empty()) { last_error_ = "missing values: no stored entry inside the matrix"; return ST_INVALID; }
	return upload_triplets(rows, cols, vals);
}

// upload_sparse for arrays in DEVICE memory of the engine's device, branch by branch (docs/DEVICE_IO.md, "Sparse input")
template <typename T>
Status Engine<T>::upload_sparse_from_device(int format, const T* values, const int* a, const int* b, long nnz, int base) {
	if (Status st = refuse_sparse_input(format, nnz)) return st;
	const int outer = format == 1 ? m_ : n_;
	const long na = format == 3 ? nnz : (long)outer + 1;
	if (Status st = check_device_vector("values", values, sizeof(T), nnz)) return st;
	if (Status st = check_device_vector("a", a, sizeof(int), na)) return st;
	if (Status st = check_device_vector("b", b, sizeof(int), nnz)) return st;
	if (beta_dense_) beta_uploaded_ = false;
	HIPX(hipDeviceSynchronize());      // whatever stream produced the arrays has finished
	const bool masked = sparse_ && prm_.is_masked();
	if (masked && nnz == 0) return refuse_sparse_values(SPARSE_NO_ENTRY);
	if ((beta_dense_ || masked) && nnz > 0) {
		int flags = 0;
		HIPX(hipMemsetAsync(range_flag_, 0, sizeof(int), stream_));
		HIPX(launch_sparse_value_rule<T>(values, nnz, beta_dense_ ? 1 : !masked_beta_ ? 2 : mbeta_ <= 0 ? 3 : 1, range_flag_, stream_));
		HIPX(hipMemcpyAsync(&flags, range_flag_, sizeof(int), hipMemcpyDeviceToHost, stream_));
		HIPX(hipStreamSynchronize(stream_));
		if (flags & IMPORT_BAD_VALUE) {
			if (masked) return refuse_sparse_values(IMPORT_BAD_VALUE);
			last_error_ = beta_value_fault(); return ST_INVALID;
		}
	}
	if (sparse_) {
		if (!sparse_setup_on_host() && nnz > 0) {
			bool fallback = false;
			const Status st = build_sparse_images(format, nnz, base, &fallback, [&](T* d_val, size_t nv, int* d_a, size_t nab, int* d_b, size_t nb) {
				HIPX(hipMemcpyAsync(d_val, values, nv, hipMemcpyDeviceToDevice, stream_));
				HIPX(hipMemcpyAsync(d_a, a, nab, hipMemcpyDeviceToDevice, stream_));
				HIPX(hipMemcpyAsync(d_b, b, nb, hipMemcpyDeviceToDevice, stream_));
				return ST_OK;
			});
			if (!fallback) return st;
		}
		// an input the device builder hands back (or NMFAMD_SPARSE_SETUP=host): the arrays come down and the host path runs as it is
		std::vector<T> h_val((size_t)nnz);
		std::vector<int> h_a((size_t)na), h_b((size_t)nnz);
		if (nnz > 0) {
			HIPX(hipMemcpyAsync(h_val.data(), values, sizeof(T) * (size_t)nnz, hipMemcpyDeviceToHost, stream_));
			HIPX(hipMemcpyAsync(h_b.data(), b, sizeof(int) * (size_t)nnz, hipMemcpyDeviceToHost, stream_));
		}
		if (na > 0) HIPX(hipMemcpyAsync(h_a.data(), a, sizeof(int) * (size_t)na, hipMemcpyDeviceToHost, stream_));
		HIPX(hipStreamSynchronize(stream_));
		return upload_sparse_on_host(format, h_val.data(), h_a.data(), h_b.data(), nnz, base);
	}
	// a densifying engine: launch_densify reads the caller's arrays where they lie (k_densify indexes values and idx below nnz and ptr below outer + 1 only -- the
	// extents checked above -- and its stores are guarded by the matrix's bounds)
	return upload_image(false, [&](T* Vcol) {
		HIPX(hipMemsetAsync(Vcol, 0, sizeof(T) * (size_t)(mpad_ * npad_), stream_));
		if (format == 3) HIPX(launch_densify<T>(3, values, nullptr, a, b, nnz, 0, base, Vcol, mpad_, m_, n_, stream_));
		else HIPX(launch_densify<T>(format, values, a, b, nullptr, nnz, outer, base, Vcol, mpad_, m_, n_, stream_));
		return ST_OK;
	});
}

// Dense V in DEVICE memory on a sparse engine: the stored entries of upload_dense compacted into both images on the device (kernels_compact.hip: count, scan,
// scatter -- no sort, so no limit on a row's or a column's length), then the tail of the sparse builder
template <typename T>
Status Engine<T>::upload_dense_device_stored(const T* V, long ld, int layout) {
	if (weighted_) { last_error_ = "weighted NMF: V is uploaded together with its weights (upload_dense_weighted)"; return ST_INVALID; }
	if (!sparse_) { last_error_ = "device upload of the stored entries: only an engine with 'sparseCompute' or 'missingValues' takes it; use nmfamd_engine_upload_dense_device"; return ST_INVALID; }
	if (Status st = check_device_matrix("V", V, ld, layout, m_, n_)) return st;
	HIPX(hipDeviceSynchronize());      // whatever stream produced V has finished
	const int masked = prm_.is_masked() ? 1 : 0;
	const long nr = compact_row_counts(m_, n_), nc = compact_col_counts(m_, n_);
	if (nr >= (1l << 31) - 1 || nc >= (1l << 31) - 1) return ST_INVALID;
	DeviceBuffers scratch;      // freed on every way out
	int *rowcnt = nullptr, *colcnt = nullptr, *off_r = nullptr, *off_c = nullptr, *small = nullptr;
	unsigned long long* total = nullptr;
	auto alloc = [&](auto** p, size_t bytes) { return scratch.device(p, std::max<size_t>(bytes, 16), false, stream_); };
	auto image = [&](auto** p, size_t bytes) { return buffers_.device(p, bytes, false, stream_); };
	HIPX(alloc(&rowcnt, sizeof(int) * (size_t)nr)); HIPX(alloc(&colcnt, sizeof(int) * (size_t)nc));
	HIPX(scratch.device(&total, sizeof(unsigned long long), true, stream_));
	HIPX(hipMemsetAsync(range_flag_, 0, sizeof(int), stream_));
	HIPX(launch_compact_count<T>(V, ld, layout, m_, n_, masked, rowcnt, colcnt, range_flag_, total, stream_));
	int flags = 0;
	unsigned long long h_total = 0;
	HIPX(hipMemcpyAsync(&flags, range_flag_, sizeof(int), hipMemcpyDeviceToHost, stream_));
	HIPX(hipMemcpyAsync(&h_total, total, sizeof(h_total), hipMemcpyDeviceToHost, stream_));
	HIPX(hipStreamSynchronize(stream_));
	// (up to here nothing of the engine's state has changed; the texts are upload_dense's)
	if (flags & IMPORT_BAD_VALUE) { last_error_ = "missing values: V holds an infinite value (NaN marks a missing entry)"; return ST_INVALID; }
	if (masked && h_total == 0) { last_error_ = "missing values: V has no observed entry"; return ST_INVALID; }
	if (h_total >= (1ull << 31)) return ST_INVALID;
	const long nnz = (long)h_total;

	buffers_.release(csr_ptr_, csr_idx_, csc_ptr_, csc_idx_, csc_from_csr_, csr_val_, csc_val_, q_, q2_);
	nnz_ = 0;
	HIPX(alloc(&off_r, sizeof(int) * (size_t)(nr + 1))); HIPX(alloc(&off_c, sizeof(int) * (size_t)(nc + 1))); HIPX(alloc(&small, sizeof(int) * 4));
	HIPX(launch_sp_scan(rowcnt, (int)nr, off_r, small, stream_));
	HIPX(launch_sp_scan(colcnt, (int)nc, off_c, small + 1, stream_));
	const size_t ni = sizeof(int) * (size_t)std::max<long>(nnz, 1), nv = sizeof(T) * (size_t)std::max<long>(nnz, 1);
	HIPX(image(&csr_ptr_, sizeof(int) * (size_t)(m_ + 1)));
	HIPX(image(&csc_ptr_, sizeof(int) * (size_t)(n_ + 1)));
	HIPX(image(&csr_idx_, ni)); HIPX(image(&csc_idx_, ni));
	HIPX(image(&csr_val_, nv)); HIPX(image(&csc_val_, nv));
	// (the quotient buffers and the CSR -> CSC permutation only serve round 1's two-pass KL step, a measurement switch)
	const bool two_pass = tuning_env("NMFAMD_KL_TWO_PASS") != nullptr;
	if (two_pass) { HIPX(image(&csc_from_csr_, ni)); HIPX(image(&q_, nv)); HIPX(image(&q2_, nv)); }
	HIPX(launch_compact_pointers(off_r, off_c, m_, n_, csr_ptr_, csc_ptr_, stream_));
	HIPX(launch_compact_scatter<T>(V, ld, layout, m_, n_, masked, off_r, off_c, nnz, csr_idx_, csr_val_, csc_idx_, csc_val_, csc_from_csr_, stream_));
	if (masked_beta_) {
		// the value rule of the engine's beta over the compacted values (the count pass knows finite from not finite only); a violation leaves the engine without
		// an image (nnz_ = 0: iterate refuses)
		HIPX(hipMemsetAsync(range_flag_, 0, sizeof(int), stream_));
		HIPX(launch_sparse_value_rule<T>(csr_val_, nnz, mbeta_ <= 0 ? 3 : 1, range_flag_, stream_));
		HIPX(hipMemcpyAsync(&flags, range_flag_, sizeof(int), hipMemcpyDeviceToHost, stream_));
		HIPX(hipStreamSynchronize(stream_));
		if (flags & IMPORT_BAD_VALUE) return refuse_sparse_values(IMPORT_BAD_VALUE);
	}
	return finish_sparse_images(nnz);
}

template <typename T>
Status Engine<T>::set_factors(const T* W, long ldw, const T* H, long ldh) {
	state_.factors_touched();
	if (W) {
		if (ldw < m_) return ST_INVALID;
		state_.w_set(); have_w_ = true;
		// host m x r (column-major) -> staging m x r (ld mpad) -> Wt panel (element (c, i) at [i * RP + c])
		HIPX(hipMemcpy2DAsync(stage_, mpad_ * sizeof(T), W, ldw * sizeof(T), m_ * sizeof(T), r_, hipMemcpyHostToDevice, stream_));
		HIPX(hipMemsetAsync(Wt_, 0, sizeof(T) * (size_t)RP_ * mpad_, stream_));
		HIPX(launch_transpose<T>(stage_, mpad_, m_, r_, Wt_, RP_, stream_));
	}
	if (H) {
		if (ldh < r_) return ST_INVALID;
		state_.h_set(); have_h_ = true;
		HIPX(hipMemsetAsync(H_, 0, sizeof(T) * (size_t)RP_ * npad_, stream_));
		HIPX(hipMemcpy2DAsync(H_, RP_ * sizeof(T), H, ldh * sizeof(T), r_ * sizeof(T), n_, hipMemcpyHostToDevice, stream_));
	}
	HIPX(hipStreamSynchronize(stream_));
	return ST_OK;
}

// *src: the panel get_factors / get_factors_device read W from -- pending scales folded in; nsNMF: W S in Ws_ (storeFactorization, AlgorithmNonSmoothNMF.h:221-225)
template <typename T>
Status Engine<T>::export_panel_w(bool want_w, const T** src) {
	if (one_pass_) { if (Status s = onepass_check()) return s; }
	if (Status s = materialize_w()) return s;
	*src = Wt_;
	if (want_w && alg_ == ALG_NSNMF) { HIPX(smooth_panel(Wt_, Ws_, mpad_)); *src = Ws_; }
	return ST_OK;
}

template <typename T>
Status Engine<T>::get_factors(T* W, long ldw, T* H, long ldh) {
	const T* src = nullptr;
	if (Status s = export_panel_w(W != nullptr && ldw >= m_, &src)) return s;
	if (W) {
		if (ldw < m_) return ST_INVALID;      // (behind materialize_w, which folds pending scales and so changes the bits of later iterations)
		HIPX(launch_transpose<T>(src, RP_, r_, m_, stage_, mpad_, stream_));
		HIPX(hipMemcpy2DAsync(W, ldw * sizeof(T), stage_, mpad_ * sizeof(T), m_ * sizeof(T), r_, hipMemcpyDeviceToHost, stream_));
	}
	if (H) {
		if (ldh < r_) return ST_INVALID;
		HIPX(hipMemcpy2DAsync(H, ldh * sizeof(T), H_, RP_ * sizeof(T), r_ * sizeof(T), n_, hipMemcpyDeviceToHost, stream_));
	}
	HIPX(hipStreamSynchronize(stream_));
	return ST_OK;
}

// Predict and score entries of W H (docs/PREDICT.md; kernels_predict.hip).  One body for host and device arrays: the refusals that need no array, the pointer checks
// (device) or the host check of every coordinate and value (host: before any device work), the staging of host arrays, the validation launch (device: no gather
// runs unless it found every coordinate inside), export_panel_w -- get_factors' effects -- and the gather; the per-workgroup sums land in pinned memory and are
// added in workgroup order.
template <typename T>
Status Engine<T>::predict_entries(const int* rows, const int* cols, const T* values, long nnz, int base, double beta, T* out, double* sums, bool device) {
	if (row_blocks_ > 1) return refuse("predict: an engine with row blocks holds a column shard of a sharded run (its export is a collective); predict on a single engine");
	if (column_shard_ || w_gather_hook_) return refuse("predict: the engine is bound to a sharded run and holds a column shard; predict on a single engine");
	if (!have_w_ || !have_h_) return refuse("predict: the engine has no factors yet (set_factors or randomize first)");
	if (nnz < 1 || nnz > PREDICT_MAX_ENTRIES) return refuse("predict: nnz has to be 1 ... 2^31 - 1 entries");
	if (base != 0 && base != 1) return refuse("predict: the index base has to be 0 or 1");
	if (rows == nullptr || cols == nullptr) return refuse("predict: null coordinate array");
	if (values == nullptr && out == nullptr) return refuse("predict: nothing to compute (neither values nor an output array)");
	if (values != nullptr && sums == nullptr) return refuse("score: null sums");
	if (!predict_rank_instantiated(RP_, sizeof(T))) return refuse("predict: no kernel for padded rank " + std::to_string(RP_));
	// the value rule of the masked beta engines, in the precision of T: 0 none, 1 finite and >= 0, 2 finite, 3 finite and > 0
	const double b = (double)(T)beta;
	if (values != nullptr && std::isinf(b)) return refuse("score: beta has to be finite (NaN: no divergence), within the range of the engine's precision");
	const int rule = values == nullptr ? 0 : b != b ? 2 : b <= 0 ? 3 : 1;
	auto bad_coordinate = [&](unsigned long p) {
		return refuse("predict: entry " + std::to_string(p) + " has a coordinate outside the matrix ([base, base + m) x [base, base + n))" +
		              (device ? "; found by the validation launch, the gather was not launched" : "; found on the host, before any device work"));
	};
	auto bad_value = [&](unsigned long p) {
		return refuse("score: value " + std::to_string(p) + (rule == 2 ? " is not finite" : rule == 3 ? " breaks the rule of beta <= 0: every value finite and > 0" : " breaks the rule of beta > 0: every value finite and >= 0"));
	};
	const int* d_rows = rows; const int* d_cols = cols; const T* d_vals = values; T* d_out = out;
	if (device) {
		if (Status st = check_device_vector("rows", rows, sizeof(int), nnz)) return st;
		if (Status st = check_device_vector("cols", cols, sizeof(int), nnz)) return st;
		if (values) { if (Status st = check_device_vector("values", values, sizeof(T), nnz)) return st; }
		if (out) { if (Status st = check_device_vector("out", out, sizeof(T), nnz)) return st; }
		HIPX(hipDeviceSynchronize());      // whatever stream produced the arrays has finished
	} else {
		for (long p = 0; p < nnz; ++p) {
			const long i = (long)rows[p] - base, j = (long)cols[p] - base;
			if (i < 0 || i >= m_ || j < 0 || j >= n_) return bad_coordinate((unsigned long)p);
		}
		for (long p = 0; rule != 0 && p < nnz; ++p) {
			const T v = values[p];
			if (!std::isfinite(v) || (rule == 1 && v < T(0)) || (rule == 3 && !(v > T(0)))) return bad_value((unsigned long)p);
		}
	}
	// the engine's own buffers
	if (pe_part_ == nullptr) {
		HIPX(buffers_.device(&pe_part_, sizeof(double) * 3 * PREDICT_MAX_PARTS, false, stream_));
		HIPX(buffers_.device(&pe_flags_, sizeof(unsigned) * 2, false, stream_));
		HIPX(buffers_.pinned(&pe_pin_, sizeof(double) * (3 * PREDICT_MAX_PARTS + 1)));
	}
	if (!device) {
		if (nnz > pe_cap_) {
			buffers_.release(pe_rows_, pe_cols_, pe_vals_, pe_out_);
			pe_cap_ = 0;
			const long cap = std::max(nnz, 1024l);
			HIPX(buffers_.device(&pe_rows_, sizeof(int) * (size_t)cap, false, stream_));
			HIPX(buffers_.device(&pe_cols_, sizeof(int) * (size_t)cap, false, stream_));
			HIPX(buffers_.device(&pe_vals_, sizeof(T) * (size_t)cap, false, stream_));
			HIPX(buffers_.device(&pe_out_, sizeof(T) * (size_t)cap, false, stream_));
			pe_cap_ = cap;
		}
		if (out != nullptr && nnz > pe_pin_cap_) {
			buffers_.release(pe_pin_out_);
			pe_pin_cap_ = 0;
			const long cap = std::max(nnz, 1024l);
			HIPX(buffers_.pinned(&pe_pin_out_, sizeof(T) * (size_t)cap));
			pe_pin_cap_ = cap;
		}
		HIPX(hipMemcpyAsync(pe_rows_, rows, sizeof(int) * (size_t)nnz, hipMemcpyHostToDevice, stream_));
		HIPX(hipMemcpyAsync(pe_cols_, cols, sizeof(int) * (size_t)nnz, hipMemcpyHostToDevice, stream_));
		if (values) HIPX(hipMemcpyAsync(pe_vals_, values, sizeof(T) * (size_t)nnz, hipMemcpyHostToDevice, stream_));
		d_rows = pe_rows_; d_cols = pe_cols_; d_vals = values ? pe_vals_ : nullptr; d_out = out ? pe_out_ : nullptr;
	} else {
		// no index of a device array has been looked at yet: the validation launch reads the index arrays (and the values) only, inside the extents checked above
		unsigned* flags = reinterpret_cast<unsigned*>(pe_pin_ + 3 * PREDICT_MAX_PARTS);
		HIPX(hipMemsetAsync(pe_flags_, 0xff, sizeof(unsigned) * 2, stream_));
		HIPX(launch_predict_validate<T>(d_rows, d_cols, d_vals, nnz, base, m_, n_, rule, pe_flags_, stream_));
		HIPX(hipMemcpyAsync(flags, pe_flags_, sizeof(unsigned) * 2, hipMemcpyDeviceToHost, stream_));
		HIPX(hipStreamSynchronize(stream_));
		if (flags[0] != 0xffffffffu) return bad_coordinate(flags[0]);      // (no gather was launched)
		if (flags[1] != 0xffffffffu) return bad_value(flags[1]);
	}
	const T* src = nullptr;
	if (Status s = export_panel_w(true, &src)) return s;
	const int parts = predict_entry_parts(nnz);
	HIPX(launch_predict_entries<T>(d_rows, d_cols, d_vals, nnz, base, src, H_, RP_, r_, std::numeric_limits<T>::epsilon(), beta, d_out, pe_part_, stream_));
	if (d_vals) HIPX(hipMemcpyAsync(pe_pin_, pe_part_, sizeof(double) * 3 * (size_t)parts, hipMemcpyDeviceToHost, stream_));
	if (!device && out) HIPX(hipMemcpyAsync(pe_pin_out_, pe_out_, sizeof(T) * (size_t)nnz, hipMemcpyDeviceToHost, stream_));
	HIPX(hipStreamSynchronize(stream_));
	if (!device && out) std::memcpy(out, pe_pin_out_, sizeof(T) * (size_t)nnz);
	if (d_vals) {
		double s[3] = {0, 0, 0};
		for (int w = 0; w < parts; ++w)      // in workgroup order
			for (int k = 0; k < 3; ++k) s[k] += pe_pin_[3 * w + k];
		const double nan = std::numeric_limits<double>::quiet_NaN();
		sums[0] = s[0]; sums[1] = b != b ? nan : s[1]; sums[2] = b != b ? nan : s[2]; sums[3] = std::sqrt(s[0] / (double)nnz);
	}
	return ST_OK;
}

// The k best candidates of W H per query (docs/TOPK.md; kernels_topk.hip).  One body for host and device arrays, shaped like predict_entries: the refusals that need no
// array, the pointer checks (device) or the host check of every index (host: before any device work), the staging of host arrays, the validation launch (device: no
// product runs unless it found everything inside), export_panel_w -- get_factors' effects -- and the two launches; host results come down through pinned memory.
template <typename T>
Status Engine<T>::top_k(const int* queries, long nq, int k, int axis, int base, const long* excl_ptr, const int* excl_idx, long excl_nnz, int* out_idx, T* out_scores,
                        bool device) {
	if (row_blocks_ > 1) return refuse("top_k: an engine with row blocks holds a column shard of a sharded run (its export is a collective); top_k on a single engine");
	if (column_shard_ || w_gather_hook_) return refuse("top_k: the engine is bound to a sharded run and holds a column shard; top_k on a single engine");
	if (!have_w_ || !have_h_) return refuse("top_k: the engine has no factors yet (set_factors or randomize first)");
	if (nq < 1 || nq > TOPK_MAX_QUERIES) return refuse("top_k: nq has to be 1 ... 2^30 queries");
	if (k < 1 || k > TOPK_MAX_K) return refuse("top_k: k has to be 1 ... " + std::to_string(TOPK_MAX_K));
	if (base != 0 && base != 1) return refuse("top_k: the index base has to be 0 or 1");
	if (axis != 0 && axis != 1) return refuse("top_k: axis has to be 0 (queries are rows) or 1 (queries are columns)");
	if (queries == nullptr || out_idx == nullptr || out_scores == nullptr) return refuse("top_k: null query or output array");
	if (excl_ptr == nullptr && excl_idx != nullptr) return refuse("top_k: excl_idx without excl_ptr");
	if (!predict_rank_instantiated(RP_, sizeof(T))) return refuse("top_k: no kernel for padded rank " + std::to_string(RP_));
	const long a_rows = axis == 0 ? m_ : n_, count = axis == 0 ? n_ : m_;
	const std::string where = device ? "; found by the validation launch, the product was not launched" : "; found on the host, before any device work";
	auto bad_query = [&](unsigned long q) {
		return refuse("top_k: query " + std::to_string(q) + " is outside [base, base + " + std::to_string(a_rows) + ")" + where);
	};
	auto bad_ptr = [&](unsigned long q) {
		return refuse("top_k: excl_ptr is malformed at " + std::to_string(q) + " (it starts at 0, does not decrease" + (device ? ", and ends at excl_nnz)" : ")") + where);
	};
	auto bad_excluded = [&](unsigned long e) {
		return refuse("top_k: excluded index " + std::to_string(e) + " is outside [base, base + " + std::to_string(count) + ")" + where);
	};
	if (device) {
		if (excl_nnz < 0) return refuse("top_k: excl_nnz is negative");
		if (Status st = check_device_vector("queries", queries, sizeof(int), nq)) return st;
		if (excl_ptr) {
			if (Status st = check_device_vector("excl_ptr", excl_ptr, sizeof(long), nq + 1)) return st;
			if (Status st = check_device_vector("excl_idx", excl_idx, sizeof(int), excl_nnz)) return st;
		}
		if (Status st = check_device_vector("indices", out_idx, sizeof(int), nq * k)) return st;
		if (Status st = check_device_vector("scores", out_scores, sizeof(T), nq * k)) return st;
		HIPX(hipDeviceSynchronize());      // whatever stream produced the arrays has finished
	} else {
		for (long q = 0; q < nq; ++q) {
			const long i = (long)queries[q] - base;
			if (i < 0 || i >= a_rows) return bad_query((unsigned long)q);
		}
		excl_nnz = 0;
		if (excl_ptr) {
			if (excl_ptr[0] != 0) return bad_ptr(0);
			for (long q = 1; q <= nq; ++q)
				if (excl_ptr[q] < excl_ptr[q - 1]) return bad_ptr((unsigned long)q);
			excl_nnz = excl_ptr[nq];
			if (excl_nnz > 0 && excl_idx == nullptr) return refuse("top_k: excl_ptr names entries and excl_idx is null");
			for (long e = 0; e < excl_nnz; ++e) {
				const long c = (long)excl_idx[e] - base;
				if (c < 0 || c >= count) return bad_excluded((unsigned long)e);
			}
		}
	}
	// the engine's own buffers
	if (tk_flags_ == nullptr) {
		HIPX(buffers_.device(&tk_flags_, sizeof(unsigned) * 3, false, stream_));
		HIPX(buffers_.pinned(&tk_pin_flags_, sizeof(unsigned) * 3));
	}
	const int slabs = topk_slabs(nq, count);
	const long part = nq * slabs * k, outs = nq * k;
	if (part > tk_part_cap_) {
		buffers_.release(tk_part_s_, tk_part_i_);
		tk_part_cap_ = 0;
		const long cap = std::max(part, 4096l);
		HIPX(buffers_.device(&tk_part_s_, sizeof(T) * (size_t)cap, false, stream_));
		HIPX(buffers_.device(&tk_part_i_, sizeof(int) * (size_t)cap, false, stream_));
		tk_part_cap_ = cap;
	}
	const int* d_q = queries; const long* d_eptr = excl_ptr; const int* d_eidx = excl_idx; int* d_oi = out_idx; T* d_os = out_scores;
	if (!device) {
		if (nq > tk_q_cap_) {
			buffers_.release(tk_q_, tk_eptr_);
			tk_q_cap_ = 0;
			const long cap = std::max(nq, 1024l);
			HIPX(buffers_.device(&tk_q_, sizeof(int) * (size_t)cap, false, stream_));
			HIPX(buffers_.device(&tk_eptr_, sizeof(long) * (size_t)(cap + 1), false, stream_));
			tk_q_cap_ = cap;
		}
		if (excl_nnz > tk_e_cap_) {
			buffers_.release(tk_eidx_);
			tk_e_cap_ = 0;
			const long cap = std::max(excl_nnz, 1024l);
			HIPX(buffers_.device(&tk_eidx_, sizeof(int) * (size_t)cap, false, stream_));
			tk_e_cap_ = cap;
		}
		if (outs > tk_out_cap_) {
			buffers_.release(tk_out_i_, tk_out_s_, tk_pin_i_, tk_pin_s_);
			tk_out_cap_ = 0;
			const long cap = std::max(outs, 1024l);
			HIPX(buffers_.device(&tk_out_i_, sizeof(int) * (size_t)cap, false, stream_));
			HIPX(buffers_.device(&tk_out_s_, sizeof(T) * (size_t)cap, false, stream_));
			HIPX(buffers_.pinned(&tk_pin_i_, sizeof(int) * (size_t)cap));
			HIPX(buffers_.pinned(&tk_pin_s_, sizeof(T) * (size_t)cap));
			tk_out_cap_ = cap;
		}
		HIPX(hipMemcpyAsync(tk_q_, queries, sizeof(int) * (size_t)nq, hipMemcpyHostToDevice, stream_));
		d_q = tk_q_; d_oi = tk_out_i_; d_os = tk_out_s_;
		d_eptr = nullptr; d_eidx = nullptr;
		if (excl_nnz > 0) {      // (lists that are all empty exclude nothing)
			HIPX(hipMemcpyAsync(tk_eptr_, excl_ptr, sizeof(long) * (size_t)(nq + 1), hipMemcpyHostToDevice, stream_));
			HIPX(hipMemcpyAsync(tk_eidx_, excl_idx, sizeof(int) * (size_t)excl_nnz, hipMemcpyHostToDevice, stream_));
			d_eptr = tk_eptr_; d_eidx = tk_eidx_;
		}
	} else {
		// no index of a device array has been looked at yet: the validation launch reads the index arrays only, inside the extents checked above
		HIPX(hipMemsetAsync(tk_flags_, 0xff, sizeof(unsigned) * 3, stream_));
		HIPX(launch_topk_validate(d_q, nq, base, a_rows, count, d_eptr, d_eidx, excl_nnz, tk_flags_, stream_));
		HIPX(hipMemcpyAsync(tk_pin_flags_, tk_flags_, sizeof(unsigned) * 3, hipMemcpyDeviceToHost, stream_));
		HIPX(hipStreamSynchronize(stream_));
		if (tk_pin_flags_[0] != 0xffffffffu) return bad_query(tk_pin_flags_[0]);      // (no product was launched)
		if (tk_pin_flags_[1] != 0xffffffffu) return bad_ptr(tk_pin_flags_[1]);
		if (tk_pin_flags_[2] != 0xffffffffu) return bad_excluded(tk_pin_flags_[2]);
		if (excl_nnz == 0) { d_eptr = nullptr; d_eidx = nullptr; }      // (every list is empty)
	}
	const T* src = nullptr;
	if (Status s = export_panel_w(true, &src)) return s;
	HIPX(launch_topk<T>(d_q, nq, k, base, axis == 0 ? src : H_, axis == 0 ? H_ : src, count, RP_, r_, d_eptr, d_eidx, slabs, tk_part_s_, tk_part_i_, d_oi, d_os, stream_));
	if (!device) {
		HIPX(hipMemcpyAsync(tk_pin_i_, tk_out_i_, sizeof(int) * (size_t)outs, hipMemcpyDeviceToHost, stream_));
		HIPX(hipMemcpyAsync(tk_pin_s_, tk_out_s_, sizeof(T) * (size_t)outs, hipMemcpyDeviceToHost, stream_));
	}
	HIPX(hipStreamSynchronize(stream_));
	if (!device) {
		std::memcpy(out_idx, tk_pin_i_, sizeof(int) * (size_t)outs);
		std::memcpy(out_scores, tk_pin_s_, sizeof(T) * (size_t)outs);
	}
	return ST_OK;
}

template <typename T>
Status Engine<T>::randomize_factors(unsigned seed, bool w, bool h, long h_first_column) {
	// The reference seeds W's and H's generators identically (RandomValueStrategy.cpp:53-69).
	state_.factors_touched();
	if (w) { state_.w_set(); have_w_ = true; HIPX(launch_fill_uniform<T>(Wt_, RP_, r_, m_, mpad_, seed, stream_)); }
	if (h) { state_.h_set(); have_h_ = true; HIPX(launch_fill_uniform<T>(H_, RP_, r_, n_, npad_, seed, stream_, h_first_column)); }
	return ST_OK;
}

// ---- the two big products ------------------------------------------------------------------

template <typename T>
void Engine<T>::record_begin(int kind) {
	if (!timing_ || !timing_now_) return;
	if (ev_used_ + 2 > ev_.size()) {
		for (int i = 0; i < 64; ++i) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return; ev_.push_back(e); }
	}
	if (ev_kind_.size() < ev_.size() / 2) ev_kind_.resize(ev_.size() / 2, 0);
	ev_kind_[ev_used_ / 2] = (char)kind;
	(void)hipEventRecord(ev_[ev_used_], stream_);
}

template <typename T>
bool Engine<T>::timed_launch_events(int kind, hipEvent_t* start, hipEvent_t* stop) {
	*start = *stop = nullptr;
	if (!timing_ || !timing_now_) return false;
	if (ev_used_ + 2 > ev_.size()) {
		for (int i = 0; i < 64; ++i) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return false; ev_.push_back(e); }
	}
	if (ev_kind_.size() < ev_.size() / 2) ev_kind_.resize(ev_.size() / 2, 0);
	ev_kind_[ev_used_ / 2] = (char)kind;
	*start = ev_[ev_used_]; *stop = ev_[ev_used_ + 1];
	return true;
}

template <typename T>
void Engine<T>::record_end() {
	if (!timing_ || !timing_now_ || ev_used_ + 2 > ev_.size()) return;
	(void)hipEventRecord(ev_[ev_used_ + 1], stream_);
	ev_used_ += 2;
}

template <typename T>
void Engine<T>::dominant_stats(double* total_ms, long* launches, double* pair_overhead_ms, double* kind_ms, long* kind_launches) {
	double tot = 0; long cnt = 0;
	double km[2] = {0, 0}; long kc[2] = {0, 0};
	(void)hipStreamSynchronize(stream_);
	for (size_t i = 0; i + 1 < ev_used_; i += 2) {
		float ms = 0;
		if (hipEventElapsedTime(&ms, ev_[i], ev_[i + 1]) == hipSuccess) {
			tot += ms; ++cnt;
			const int k = (i / 2 < ev_kind_.size() && ev_kind_[i / 2] != 0) ? 1 : 0;
			km[k] += ms; ++kc[k];
		}
	}
	ev_used_ = 0;
	if (total_ms) *total_ms = tot;
	if (launches) *launches = cnt;
	if (kind_ms) { kind_ms[0] = km[0]; kind_ms[1] = km[1]; }
	if (kind_launches) { kind_launches[0] = kc[0]; kind_launches[1] = kc[1]; }
	if (pair_overhead_ms) {
		// what an event pair reports with NOTHING between the two records (idle stream, smallest of eight):
		// the part of every sample above that is not kernel time
		double best = -1;
		if (ev_.size() >= 2) {
			for (int i = 0; i < 8; ++i) {
				(void)hipEventRecord(ev_[0], stream_);
				(void)hipEventRecord(ev_[1], stream_);
				(void)hipEventSynchronize(ev_[1]);
				float ms = 0;
				if (hipEventElapsedTime(&ms, ev_[0], ev_[1]) == hipSuccess && (best < 0 || ms < best)) best = ms;
			}
		}
		*pair_overhead_ms = best < 0 ? 0.0 : best;
	}
}

// Passenger arguments for the Gram matrix of W (of_w) or H of the rank-64 fast path: from the split image of the panel
// (gram_image_) or from the partial matrices the 64-column update kernel left behind.
template <typename T>
GramReduceArgs Engine<T>::gram_args(bool of_w, float* G, float* scale, int normalize) const {
	GramReduceArgs rg = {of_w ? gramW_part_ : gramH_part_, (int)((of_w ? mpad_ : npad_) / 64), G, scale, normalize};
	if (gram_image_) {
		rg.partials = nullptr; rg.parts = 0; rg.image = of_w ? Wx3_ : Hx3_; rg.image_ks = of_w ? ksH_ : ksW_;
		// the pending column scale of W from the sums of squares its update left (one vector per 32 panel rows)
		if (of_w && normalize != 0 && wsq_part_ != nullptr) { rg.colsq_part = wsq_part_; rg.colsq_parts = (int)(mpad_ / 32); }
		// W^T W beside the W^T V launch of a column shard: K slices into Gpart_, added and scaled by the H update (mu64_update)
		if (of_w && (const void*)G == (const void*)G_ && gram_ksplit_ > 1 && Gpart_ != nullptr && (normalize == 0 || rg.colsq_part != nullptr)) { rg.ksplit = gram_ksplit_; rg.G = Gpart_; }
		// ... of a whole problem: the sixteen passengers share the ten tiles' K ranges evenly (gram_image.h, spread form), pieces into Gpart_ for the same consumer
		else if (of_w && (const void*)G == (const void*)G_ && gram_spread_ && Gpart_ != nullptr && (normalize == 0 || rg.colsq_part != nullptr)) { rg.spread = 1; rg.G = Gpart_; rg.spread_out = G; rg.spread_counter = gram_spread_counter_; }
	}
	return rg;
}

template <typename T>
Status Engine<T>::standalone_gram(const GramReduceArgs& rg) {
	if (rg.image != nullptr) HIPX(launch_gram_image_args(rg, stream_));
	else HIPX(launch_mu64_gram_reduce(rg, stream_));
	return ST_OK;
}

// U_H / U_W of the rank-64 fast path (kernels_mu64.hip)
template <typename T>
Status Engine<T>::mu64_update(bool is_w, const T* slabs, int S, long slab_stride, const T* Q, bool compute_error, const PeerSlabs* peers) {
	if constexpr (std::is_same<T, float>::value) {
		const float eps = std::numeric_limits<float>::epsilon();
		float* P = is_w ? Wt_ : H_;
		// (ps_direct_: the update kernels write their error terms straight into the pinned host buffer -- no copy launch behind them, iterate_mu64)
		float* ps = ps_direct_ ? (is_w ? pin_psN_dev_ + ps_stride_ : pin_psN_dev_) : (is_w ? psR_ : psN_);
		const int len = is_w ? m_ : n_, len_pad = (int)(is_w ? mpad_ : npad_);
		void* xo = x3_ ? (is_w ? Wx3_ : Hx3_) : nullptr;
		const int xks = is_w ? ksH_ : ksW_;
		if (peers != nullptr && !gram_image_) return ST_INVALID;
		// nsNMF: the smoothing matrix goes around the H update's r x r product (the launches on either side work on the unsmoothed W image and on the image of S H)
		SmoothAround ns;
		ns.off = smoothing_constants().off; ns.diag = smoothing_constants().diag; ns.r = r_;
		const bool smooth = alg_ == ALG_NSNMF && !is_w;
		if (alg_ == ALG_NSNMF && !gram_image_) return ST_INVALID;
		if (gram_image_) HIPX(launch_mu64_update32(is_w ? 1 : 0, P, slabs, S, slab_stride, Q, scale_, eps, ps, len, len_pad, is_w ? G_ : nullptr, compute_error ? 1 : 0, stream_, xo, xks, peers,
		                                           is_w ? wsq_part_ : nullptr, (!is_w && (const void*)Q == (const void*)Gpart_) ? gram_ksplit_ : 0, (!is_w && (const void*)Q == (const void*)Gpart_) ? G_ : nullptr,
		                                           smooth ? &ns : nullptr));
		else HIPX(launch_mu64_update(is_w ? 1 : 0, P, slabs, S, slab_stride, Q, scale_, eps, ps, len, len_pad, is_w ? gramW_part_ : gramH_part_, is_w ? G_ : nullptr,
		                             compute_error ? 1 : 0, stream_, xo, xks));
	}
	return ST_OK;
}

template <typename T>
Status Engine<T>::product_h(const T* F, const GramReduceArgs* rg, bool prepacked) {
	if (sparse_) {
		// W^T V as a row-gather SpMM over the CSC image: out(:, j) = sum_i V(i, j) F(:, i)
		if (rg) { if (Status st = standalone_gram(*rg)) return st; }
		record_begin();
		HIPX(launch_spmm_rows<T>(csc_ptr_, csc_idx_, csc_val_, F, RP_, slabs_, n_, (int)npad_, stream_));
		record_end();
		return ST_OK;
	}
	if constexpr (std::is_same<T, float>::value) {
		if (bf16_) {
			// bf16 operands: the factor panel is re-rounded and re-ordered for every product
			if (!prepacked) HIPX(launch_pack_panel_bf16(F, RP_, m_, Wtb_, ksH_, stream_));
			if (rg && rg->tri_frags == nullptr && planHb_.xtiles < GRAM_REDUCE_BLOCKS) { if (Status st = standalone_gram(*rg)) return st; rg = nullptr; }
			record_begin();
#ifdef NMFAMD_DIAG_BUILD
			if (unsigned long long* st = bf_stamps(0)) set_factor_product_bf16_stamps(st);
#endif
			HIPX(launch_factor_product_bf16(planHb_, Vtb_, ksH_, Wtb_, RP_, slabs_, slab_stride_, stream_, rg));
			record_end();
			return ST_OK;
		}
		if (x3_) {
			if (!prepacked) HIPX(launch_pack_panel_x3(F, RP_, m_, Wx3_, ksH_, stream_));
			if (rg && rg->wide_P == nullptr && !passengers_ride(planHx_)) { if (Status st = standalone_gram(*rg)) return st; rg = nullptr; }
			hipEvent_t e0, e1;
			const bool timed = timed_launch_events(0, &e0, &e1);
			if (one_image_) HIPX(launch_factor_product_x3(planHx_, V_, strideV_, Wx3_, RP_, slabs_, slab_stride_, stream_, rg, nullptr, true, img_th_, e0, e1));
			else HIPX(launch_factor_product_x3(planHx_, Vt_, strideVt_, Wx3_, RP_, slabs_, slab_stride_, stream_, rg, nullptr, false, 128, e0, e1));
			if (timed) timed_launch_done();
			return ST_OK;
		}
		if (tiled_) {
			if (rg && planH_.xtiles < GRAM_REDUCE_BLOCKS) { if (Status st = standalone_gram(*rg)) return st; rg = nullptr; }
			record_begin();
			HIPX(launch_factor_product_f32(planH_, Vt_, strideVt_, F, RP_, slabs_, slab_stride_, stream_, rg));
			record_end();
			return ST_OK;
		}
	}
	if constexpr (std::is_same<T, double>::value) {
		if (tiled_) {
			record_begin();
			HIPX(launch_factor_product_f64(planH_, Vt_, strideVt_, F, RP_, slabs_, slab_stride_, stream_, ride64_));
			record_end();
			return ST_OK;
		}
	}
	record_begin();
	HIPX(launch_factor_product_valu<T>(Vt_, npad_, (int)npad_, m_, F, RP_, slabs_, stream_));
	record_end();
	return ST_OK;
}

template <typename T>
Status Engine<T>::product_w(const T* F, const GramReduceArgs* rg, T* single_slab_out, bool prepacked) {
	T* dest = (single_slab_out != nullptr && planW_.splits == 1) ? single_slab_out : slabs_;
	if (sparse_) {
		// (V H^T)^T over the CSR image: out(:, i) = sum_j V(i, j) F(:, j)
		if (rg) { if (Status st = standalone_gram(*rg)) return st; }
		record_begin(1);
		HIPX(launch_spmm_rows<T>(csr_ptr_, csr_idx_, csr_val_, F, RP_, dest, m_, (int)mpad_, stream_));
		record_end();
		return ST_OK;
	}
	if constexpr (std::is_same<T, float>::value) {
		if (bf16_) {
			if (!prepacked) HIPX(launch_pack_panel_bf16(F, RP_, n_, Hb_, ksW_, stream_));
			if (rg && rg->tri_frags == nullptr && planWb_.xtiles < GRAM_REDUCE_BLOCKS) { if (Status st = standalone_gram(*rg)) return st; rg = nullptr; }
			record_begin(1);
#ifdef NMFAMD_DIAG_BUILD
			if (unsigned long long* st = bf_stamps(1)) set_factor_product_bf16_stamps(st);
#endif
			HIPX(launch_factor_product_bf16(planWb_, Vb_, ksW_, Hb_, RP_, dest, slab_stride_, stream_, rg));
			record_end();
			return ST_OK;
		}
		if (x3_) {
			if (!prepacked) HIPX(launch_pack_panel_x3(F, RP_, n_, Hx3_, ksW_, stream_));
			if (rg && rg->wide_P == nullptr && !passengers_ride(planWx_)) { if (Status st = standalone_gram(*rg)) return st; rg = nullptr; }
			hipEvent_t e0, e1;
			const bool timed = timed_launch_events(1, &e0, &e1);
			HIPX(launch_factor_product_x3(planWx_, V_, strideV_, Hx3_, RP_, dest, slab_stride_, stream_, rg, nullptr, false, img_th_, e0, e1));
			if (timed) timed_launch_done();
			return ST_OK;
		}
		if (tiled_) {
			if (rg && planW_.xtiles < GRAM_REDUCE_BLOCKS) { if (Status st = standalone_gram(*rg)) return st; rg = nullptr; }
			record_begin(1);
			HIPX(launch_factor_product_f32(planW_, V_, strideV_, F, RP_, dest, slab_stride_, stream_, rg));
			record_end();
			return ST_OK;
		}
	}
	if constexpr (std::is_same<T, double>::value) {
		if (tiled_) {
			record_begin(1);
			HIPX(launch_factor_product_f64(planW_, V_, strideV_, F, RP_, dest, slab_stride_, stream_, ride64_));
			record_end();
			return ST_OK;
		}
	}
	record_begin(1);
	HIPX(launch_factor_product_valu<T>(V_, mpad_, (int)mpad_, n_, F, RP_, dest, stream_));
	record_end();
	return ST_OK;
}

template <typename T>
Status Engine<T>::normal_inverse(T* A, T offdiag, T diag) {
	HIPX(launch_inverse_small<T>(A, RP_, r_, Qinv_, inv_work_, offdiag, diag, stream_));
	return ST_OK;
}

// Fork: everything enqueued on the main stream so far (the Gram matrix, its saved copy) precedes the inverse;
// join: the main stream waits for the inverse before the update kernel reads Qinv_.  Between the two the main
// stream must not touch A, Qinv_ or inv_work_.
template <typename T>
Status Engine<T>::normal_inverse_fork(T* A, T offdiag, T diag) {
	if (!overlap_inverse_) return normal_inverse(A, offdiag, diag);
	HIPX(hipEventRecord(ev_fork_, stream_));
	HIPX(hipStreamWaitEvent(aux_, ev_fork_, 0));
	HIPX(launch_inverse_small<T>(A, RP_, r_, Qinv_, inv_work_, offdiag, diag, aux_));
	HIPX(hipEventRecord(ev_join_, aux_));
	return ST_OK;
}

// Split-operand product at padded rank 64: the sixteen passenger workgroups (Gram matrix from the split image, or the one that inverts) sit BEHIND the
// product blocks in the grid.  They ride when the product has at least sixteen x-tiles (config 2's shapes: the grid is several waves of workgroups and the
// passengers start as CUs drain) or when the whole grid fits the chip at once (column shards: few x-tiles, e.g. 5 x 26 + 16 workgroups at n = 625) --
// round 3 sent the latter to a stand-alone 16-workgroup launch of 28 us.
template <typename T>
bool Engine<T>::passengers_ride(const FactorProductPlan& plan) const {
	const int passengers = (&plan == &planHx_ && gram_ksplit_ > 1) ? GRAM_IMAGE_TILES * gram_ksplit_ : GRAM_REDUCE_BLOCKS;
	const int per_cu = plan.col_split == 2 ? 2 : 1;       // (128 x 32 workgroups: two to a CU)
	return RP_ == 64 && ((plan.xtiles >= GRAM_REDUCE_BLOCKS && passengers == GRAM_REDUCE_BLOCKS) || per_cu * plan.xtiles * plan.splits + passengers <= per_cu * num_cus_);
}

// fp32 product (native MFMA or split-operand kernel) at padded rank 64 with passenger blocks in its grid
template <typename T>
bool Engine<T>::inverse_rides(const FactorProductPlan& plan) const {
	return std::is_same<T, float>::value && tiled_ && !bf16_ && !sparse_ && RP_ == 64 && r_ <= 64 && plan.xtiles >= GRAM_REDUCE_BLOCKS &&
	       tuning_env("NMFAMD_NO_OVERLAP") == nullptr && tuning_env("NMFAMD_INVERSE_SIDE_STREAM") == nullptr;
}

template <typename T>
Status Engine<T>::normal_inverse_join() {
	if (!overlap_inverse_) return ST_OK;
	HIPX(hipStreamWaitEvent(stream_, ev_join_, 0));
	return ST_OK;
}

// ---- error terms ----------------------------------------------------------------------------

template <typename T>
Status Engine<T>::fetch_error_terms(int count_n) {
	finalize_error(false);   // the pinned buffers are about to be reused; an older fetch is long complete
	ps_last_direct_ = ps_direct_;
	if (error_terms_stay_) {
		// a sharded run gathers the terms of all ranks on the device (error_terms_to_device) and resolves them itself: no host copy, no event here
		err_count_ = count_n;
		return ST_OK;
	}
	// (a kernel that writes the pinned buffer, not hipMemcpyAsync: the runtime's copy idles the stream for ~18 us around its blit; NMFAMD_ERROR_MEMCPY=1 restores it)
	static const bool use_memcpy = tuning_env("NMFAMD_ERROR_MEMCPY") != nullptr;
	if (ps_direct_) { /* the update kernels of this iteration wrote the pinned buffer themselves */ }
	else if (use_memcpy || pin_psN_dev_ == nullptr) HIPX(hipMemcpyAsync(pin_psN_, psN_, sizeof(T) * (size_t)(ps_stride_ + r_), hipMemcpyDeviceToHost, stream_));
	else HIPX(launch_copy_small<T>(pin_psN_dev_, psN_, ps_stride_ + r_, stream_));
	HIPX(hipEventRecord(err_event_, stream_));
	err_pending_ = true;
	err_count_ = count_n;
	return ST_OK;
}

template <typename T>
long Engine<T>::error_terms_to_device(T* dst, long capacity) {
	const long cnt = (long)err_count_ + r_;
	if (err_count_ <= 0 || capacity < cnt) return -1;
	// (the last error iteration's update kernels wrote the pinned host buffer themselves, iterate_mu64: psN_ / psR_ on the device are an older iteration's -- ADVICE r5)
	if (ps_last_direct_) return launch_copy_two<T>(dst, pin_psN_dev_, err_count_, pin_psN_dev_ + ps_stride_, r_, stream_) == hipSuccess ? cnt : -1;
	// ONE small launch for both pieces (two runtime copies were two blit kernels)
	if (launch_copy_two<T>(dst, psN_, err_count_, psR_, r_, stream_) != hipSuccess) return -1;
	return cnt;
}

template <typename T>
void Engine<T>::finalize_error(bool resolve) {
	if (masked_pending_) {
		(void)hipEventSynchronize(err_event_);
		h_psN_.assign(pin_kl_, pin_kl_ + m_);                       // per-row sums of squared residuals over the stored entries
		masked_pending_ = false;
		masked_unresolved_ = true;
	}
	if (resolve && masked_unresolved_) {
		// a direct sum of residuals (not the trace formula), in double, row order; rmsd over the stored entries
		double s = 0;
		for (int i = 0; i < m_; ++i) s += (double)h_psN_[i];
		frob2_ = s;
		frob_ = std::sqrt(s);
		rmsd_ = frob_ / std::sqrt((double)nnz_);
		masked_unresolved_ = false;
	}
	if (beta_pending_) {
		(void)hipEventSynchronize(err_event_);
		h_psN_.assign(pin_kl_, pin_kl_ + m_);                       // per-row sums of (v - p)^2
		h_klrow_.assign(pin_kl_ + m_, pin_kl_ + 2 * (size_t)m_);    // per-row sums of the divergence
		beta_pending_ = false;
		beta_unresolved_ = true;
	}
	if (resolve && beta_unresolved_) {
		// direct sums, in double, row order
		double s = 0, d = 0;
		for (int i = 0; i < m_; ++i) { s += (double)h_psN_[i]; d += (double)h_klrow_[i]; }
		frob2_ = s;
		frob_ = std::sqrt(s);
		// (weighted: sum of the weights -- the observed count at 0 / 1 weights; a masked divergence engine: the stored entries)
		rmsd_ = frob_ / std::sqrt(weighted_ ? sum_w_ : masked_beta_ ? (double)nnz_ : (double)m_ * (double)n_);
		kl_ = d;
		beta_unresolved_ = false;
	}
	if (kl_pending_) {
		(void)hipEventSynchronize(err_event_);
		h_psN_.assign(pin_kl_, pin_kl_ + m_);                       // per-row terms of tr(H^T W^T V)
		h_klrow_.assign(pin_kl_ + m_, pin_kl_ + 2 * (size_t)m_);
		h_sW_.assign(pin_kl_ + 2 * (size_t)m_, pin_kl_ + 2 * (size_t)m_ + RP_);
		h_sH_.assign(pin_kl_ + 2 * (size_t)m_ + RP_, pin_kl_ + 2 * (size_t)m_ + 2 * RP_);
		h_psR_.assign(pin_kl_ + 2 * (size_t)m_ + 2 * RP_, pin_kl_ + 2 * (size_t)m_ + 2 * RP_ + r_);
		kl_pending_ = false;
		kl_unresolved_ = true;
	}
	if (resolve && kl_unresolved_) {
		resolve_error(h_vtv_, h_psN_, h_psR_, (long)((unsigned)m_ * (unsigned)(err_total_columns_ > 0 ? err_total_columns_ : n_)));
		double d = -sum_v_;
		for (int i = 0; i < m_; ++i) d += (double)h_klrow_[i];
		for (int c = 0; c < r_; ++c) d += (double)h_sW_[c] * (double)h_sH_[c];
		kl_ = d;
		kl_unresolved_ = false;
	}
	if (err_pending_) {
		(void)hipEventSynchronize(err_event_);
		h_psN_.assign(pin_psN_, pin_psN_ + err_count_);
		h_psR_.assign(pin_psR_, pin_psR_ + r_);
		err_pending_ = false;
		err_unresolved_ = true;
	}
	if (resolve && err_unresolved_) {
		resolve_error(h_vtv_, h_psN_, h_psR_, (long)((unsigned)m_ * (unsigned)(err_total_columns_ > 0 ? err_total_columns_ : n_)));
		err_unresolved_ = false;
	}
}

template <typename T>
void Engine<T>::resolve_error(const std::vector<T>& vtv_sorted, std::vector<T> htwtv, std::vector<T> hhtwtw, long total_elements) {
	frob2_ = resolve_frobenius_squared<T>(vtv_sorted, htwtv, hhtwtw);
	frob_ = std::sqrt(frob2_);
	rmsd_ = frob_ / std::sqrt((double)total_elements);
}

// ---- iteration --------------------------------------------------------------------------------

template <typename T>
Status Engine<T>::h_step(bool compute_error) {
	column_shard_ = true;
	// first call of an iteration in the sharded form: decides whether this iteration's products are timed
	timing_now_ = timing_ && (timing_iter_++ % timing_stride_ == 0);
	if (prm_.is_masked()) return masked_refuses("h_step");
	if (beta_dense_) return beta_refuses("h_step");
	if (prm_.divergence != 0) { kl_err_iter_ = compute_error; return kl_h_step(); }
	if (hals_family(alg_)) { last_error_ = "HALS: no three-phase (column-sharded) form"; return ST_INVALID; }
	return h_step_impl(compute_error);
}

template <typename T>
Status Engine<T>::h_step_impl(bool compute_error) {
	const T eps = std::numeric_limits<T>::epsilon();
	state_.h_product_ahead = false; state_.f64_product_ahead = false;                           // (the three-phase API enqueues its own W^T V)
	if constexpr (std::is_same<T, float>::value) {
		if (fused_capable()) {
			// sharded form of the four-launch iteration (kernels_mu64.hip): K_H + U_H here
			if (!state_.fused_ready) {
				if (!gram_image_) HIPX(launch_mu64_gram_partials(Wt_, (int)mpad_, gramW_part_, stream_));
				normalize_next_ = 0;
				state_.fused_ready = true;
			}
			GramReduceArgs rgW = gram_args(true, G_, scale_, normalize_next_);
			if (Status s = product_h(Wt_, &rgW, x3_ && state_.wx3_valid)) return s;
			if (Status s = mu64_update(false, slabs_, planH_.splits, slab_stride_, rgW.ksplit > 1 ? reinterpret_cast<const T*>(Gpart_) : G_, compute_error)) return s;
			state_.hx3_valid = x3_;
			return ST_OK;
		}
	}
	state_.hx3_valid = false;
	if constexpr (std::is_same<T, float>::value) {
		if (tri_) {
			// The fragments hold bf16(W) as the panel stores it -- unsmoothed, without the pending column scale D; the product's output gets both:
			// (W D S)^T V = S D (W^T V), applied by the H update to the summed slabs (PanelTriExtras).
			GramReduceArgs ride = {nullptr, 0, nullptr, nullptr, 0};
			if (Status s = tri_prepare_w(&ride)) return s;
			if (Status s = product_h(Wt_, ride.tri_frags != nullptr ? &ride : nullptr, true)) return s;
			const auto [off, diag] = smoothing_constants();
			PanelTriExtras ex;
			ex.num_transform = true;
			if (state_.tri_scale_pending) { ex.num_colsq = colsq_; ex.num_colsq_parts = colsq_parts_; }
			ex.num_a = (float)(diag - off); ex.num_b = (float)off; ex.r = r_;
			// ... and the denominator S D G D S H from the Gram matrix as the reduction left it (its split image is in qx3_): D and S around the product
			ex.den_transform = true;
			ex.den_a = ex.num_a; ex.den_b = ex.num_b;
			ex.den_colsq = ex.num_colsq; ex.den_colsq_parts = ex.num_colsq_parts;
			// ... and leaves the operand of the next V (S H)^T behind: the bf16 fragments of the smoothed new columns (AlgorithmNonSmoothNMF.h:194)
			ex.frag_out = Hb_; ex.frag_KS = ksW_; ex.frag_a = (float)(diag - off); ex.frag_b = (float)off;
			// (old_as_bf16 stays off here: the H update is bound by what a CU can ingest, not by its MFMAs -- 28.3 -> 27.7 us -- and H's distance from the
			// fp64 oracle doubles, 5.7e-5 -> 1.5e-4 after 10 iterations; the W update gains 11 us at no measurable cost, tri_update_w)
			// (state_.qx3_holds_g: the Gram reduction left the split image of W^T W in qx3_ -- Q = nullptr tells the update kernel so; else it packs Gw_raw_)
			HIPX(launch_panel_update<T>(PANEL_MU, H_, slabs_, planH_.splits, slab_stride_, state_.qx3_holds_g ? nullptr : reinterpret_cast<const T*>(Gw_raw_), RP_, (int)npad_, eps,
			                            compute_error ? psN_ : nullptr, n_, nullptr, nullptr, stream_, nullptr, nullptr, 0, qx3_, &ex));
			state_.qx3_holds_g = false;
			state_.hb_valid = true;
			return ST_OK;
		}
	}
	if (Status s = materialize_w()) return s;
	const T* F = Wt_;
	if (alg_ == ALG_NSNMF) {
		HIPX(smooth_panel(Wt_, Ws_, mpad_));
		F = Ws_;
	}
	if (!(state_.gram_w_ready && F == Wt_)) HIPX(launch_gram<T>(F, RP_, m_, gram_parts_, gram_part_, G_, stream_));
	state_.gram_w_ready = false;      // consumed (the inverse passenger / update below read G_; W changes in the W step)
	const int S = planH_.splits;
	if (hals_family(alg_)) {
		// coordinate sweep over every column of H against G = W^T W and the summed slabs of W^T V; ps: the per-column terms of tr(H^T W^T V), as PANEL_MU
		// writes them.  No split image of the new H: the next product packs its operand itself.
		if (Status s = product_h(F, nullptr, x3_ && state_.wx3_valid && F == Wt_)) return s;
		// (penalties: G and the slabs stay raw -- ps and the trace of the error term read them)
		// (sweeps_h sweeps against this one G and these slabs, in one launch; one sweep is launch_panel_sweep_hals)
		// (a sweep tolerance: the counts are maximum counts and every column stops by itself, kernels_hals_dyn.hip)
		// (NeNMF: steps_h projected-gradient steps in the same place, kernels_nenmf.hip)
		if (Status s = family_step(false, H_, G_, S, (int)npad_, n_, compute_error ? psN_ : nullptr, nullptr, (T)prm_.l1H, (T)prm_.l2H)) return s;
		state_.hx3_valid = false;
		return ST_OK;
	}
	if (alg_ == ALG_MU || alg_ == ALG_NSNMF) {
		if (Status s = product_h(F, nullptr, x3_ && state_.wx3_valid && F == Wt_)) return s;
		const bool emit = x3_ && alg_ == ALG_MU && panel_update_delivers_gram(RP_, sizeof(T));   // nsNMF's W step consumes the smoothed panel
		HIPX(launch_panel_update<T>(PANEL_MU, H_, slabs_, S, slab_stride_, G_, RP_, (int)npad_, eps,
		                            compute_error ? psN_ : nullptr, n_, nullptr, nullptr, stream_, nullptr, emit ? Hx3_ : nullptr, ksW_, qx3_));
		state_.hx3_valid = emit;
	} else {
		T off = 0, diag = 0;
		if (alg_ == ALG_GDCLS) diag = (T)prm_.lambda;
		else if (alg_ == ALG_ACLS) diag = (T)prm_.lambdaH;
		else if (alg_ == ALG_AHCLS) {
			const T lam = (T)prm_.lambdaH, alpha = (T)prm_.alphaH;
			T beta = (T)((1 - alpha) * std::sqrt((double)(unsigned)r_) + alpha);
			beta *= beta;
			off = -lam; diag = lam * beta - lam;
		}
		if (compute_error) HIPX(hipMemcpyAsync(G2_, G_, sizeof(T) * (size_t)RP_ * RP_, hipMemcpyDeviceToDevice, stream_));
		// the inverse of the normal matrix (one workgroup) runs beside the product against V: as a passenger
		// workgroup of the product launch where that exists (fp32 MFMA product, r <= 64), else on the side stream
		if (inverse_rides(planH_)) {
			if constexpr (std::is_same<T, float>::value) {
				GramReduceArgs rg = {nullptr, 0, nullptr, nullptr, 0};
				rg.inv_a = G_; rg.inv_out = Qinv_; rg.inv_offdiag = off; rg.inv_diag = diag; rg.inv_r = r_;
				if (Status s = product_h(F, &rg, x3_ && state_.wx3_valid && F == Wt_)) return s;
			}
		} else {
			if (Status s = normal_inverse_fork(G_, off, diag)) return s;
			if (Status s = product_h(F, nullptr, x3_ && state_.wx3_valid && F == Wt_)) return s;
			if (Status s = normal_inverse_join()) return s;
		}
		const bool emit = x3_ && panel_update_delivers_gram(RP_, sizeof(T));
		T* hpart = nullptr;
		// (GDCLS on the split-operand path at padded rank 64: the fused iteration takes H H^T from the split image beside the product, Engine::iterate -- the
		//  sharded form, w_products(), makes its own Gram pass over H)
		if constexpr (std::is_same<T, float>::value) { if (gram_from_update() && !(alg_ == ALG_GDCLS && emit && RP_ == 64 && passengers_ride(planWx_) && h_partials_unneeded_)) hpart = gramH_part_; }
		HIPX(launch_panel_update<T>(PANEL_LS, H_, slabs_, S, slab_stride_, Qinv_, RP_, (int)npad_, eps,
		                            nullptr, n_, nullptr, nullptr, stream_, hpart, emit ? Hx3_ : nullptr, ksW_, qx3_));
		state_.hx3_valid = emit;
		state_.gram_h_partials = hpart != nullptr;
	}
	return ST_OK;
}

template <typename T>
Status Engine<T>::w_products(T* exchange) {
	column_shard_ = true;
	if (prm_.is_masked()) return masked_refuses("w_products");
	if (beta_dense_) return beta_refuses("w_products");
	if (prm_.divergence != 0) return kl_w_products(exchange, kl_err_iter_);      // (sparse Frobenius compute shards through the code below: its two products are SpMMs over the shard's images)
	if (hals_family(alg_)) { last_error_ = "HALS: no three-phase (column-sharded) form"; return ST_INVALID; }
	T* ex_hht = exchange + (long)RP_ * mpad_;
	if constexpr (std::is_same<T, float>::value) {
		if (fused_capable()) {
			// K_W with the local H H^T reduced straight into the exchange buffer by the passenger
			// workgroups, then the local split-K slabs summed into the exchange panel
			GramReduceArgs rgH = gram_args(false, ex_hht, nullptr, 0);
			// a team of one: w_finish() sums the split-K slabs itself, as iterate_mu64() does -- no pass over the panel in between
			// (nsNMF: the H update of h_step left the split image of S H; without it -- no H step since the factors were set -- the smoothed panel is packed here)
			const T* Fh = H_;
			if (alg_ == ALG_NSNMF && !(x3_ && state_.hx3_valid)) {
				HIPX(smooth_panel(H_, Hs_, npad_));
				Fh = Hs_;
			}
			if (sole_rank_ && gram_image_) return product_w(Fh, &rgH, nullptr, x3_ && state_.hx3_valid);
			// one K slice (short column shards) writes the exchange panel itself
			if (Status s = product_w(Fh, &rgH, exchange, x3_ && state_.hx3_valid)) return s;
			if (planW_.splits > 1) HIPX(launch_reduce_slabs<T>(slabs_, planW_.splits, slab_stride_, exchange, (long)RP_ * mpad_, stream_));
			return ST_OK;
		}
	}
	if constexpr (std::is_same<T, float>::value) {
		if (tri_) {
			GramReduceArgs ride = {nullptr, 0, nullptr, nullptr, 0};
			if (Status s = tri_prepare_h(ex_hht, sole_rank_, sole_rank_ ? &ride : nullptr)) return s;      // (a team of one: nothing is added to ex_hht before the W update reads it)
			if (Status s = product_w(H_, ride.tri_frags != nullptr ? &ride : nullptr, exchange, true)) return s;
			if (planW_.splits > 1) HIPX(launch_reduce_slabs<T>(slabs_, planW_.splits, slab_stride_, exchange, (long)RP_ * mpad_, stream_));
			return ST_OK;
		}
	}
	const T* Fh = H_;
	if (alg_ == ALG_NSNMF) {
		// the smoothed local columns S H_g enter both sums (AlgorithmNonSmoothNMF.h:194-197,213)
		HIPX(smooth_panel(H_, Hs_, npad_));
		Fh = Hs_;
	}
	HIPX(launch_gram<T>(Fh, RP_, n_, gram_parts_, gram_part_, ex_hht, stream_));
	// a single K slice writes the exchange panel itself; several are summed into it
	if (Status s = product_w(Fh, nullptr, exchange)) return s;
	if (planW_.splits > 1) HIPX(launch_reduce_slabs<T>(slabs_, planW_.splits, slab_stride_, exchange, (long)RP_ * mpad_, stream_));
	return ST_OK;
}

template <typename T>
Status Engine<T>::w_finish(const T* exchange, bool compute_error) {
	column_shard_ = true;
	if (prm_.is_masked()) return masked_refuses("w_finish");
	if (beta_dense_) return beta_refuses("w_finish");
	if (prm_.divergence != 0) return kl_w_finish(exchange, compute_error);
	if (hals_family(alg_)) { last_error_ = "HALS: no three-phase (column-sharded) form"; return ST_INVALID; }
	const T eps = std::numeric_limits<T>::epsilon();
	const T* ex_hht = exchange + (long)RP_ * mpad_;
	if (alg_ != ALG_MU && alg_ != ALG_NSNMF) {
		// GDCLS / ALS / ACLS / AHCLS on the all-reduced sums (their extra products are r x r sized or row / column
		// separable): exactly the W step of iterate() with the reduced (V H^T)^T panel as the one "slab" and the reduced H H^T
		// (AlgorithmGradientDescentConstrainedLeastSquares.h:236-264, AlgorithmAlternatingHoyerConstrainedLeastSquares.h:226-284)
		const int norm_parts = panel_update_parts(RP_, sizeof(T), (int)mpad_);
		const bool ls_family = alg_ != ALG_GDCLS;
		if (compute_error) HIPX(launch_trace_small<T>(ex_hht, G2_, RP_, r_, psR_, stream_));      // G2_: W^T W saved before the regulariser (h_step)
		T* wpart = nullptr;
		if constexpr (std::is_same<T, float>::value) { if (gram_from_update()) wpart = gramW_part_; }
		state_.wx3_valid = false;
		if (!ls_family) {
			HIPX(launch_panel_update<T>(PANEL_MU, Wt_, exchange, 1, 0, ex_hht, RP_, (int)mpad_, eps, nullptr, m_, sumsq_part_, compute_error ? numW_ : nullptr, stream_,
			                            wpart, nullptr, 0, qx3_));
			if (Status st = normalize_w(wpart != nullptr, norm_parts)) return st;
			// tr(H^T W^T V) as diag((V H^T)^T W) with the UPDATED W (GDCLS :259-264)
			if (compute_error) HIPX(launch_row_dot<T>(numW_, Wt_, RP_, r_, mpad_, psN_, stream_, rowdot_part_));
		} else {
			T offW = 0, diagW = 0;
			if (alg_ == ALG_ACLS) diagW = (T)prm_.lambdaW;
			else if (alg_ == ALG_AHCLS) {
				const T lam = (T)prm_.lambdaW, alpha = (T)prm_.alphaW;
				T beta = (T)((1 - alpha) * std::sqrt((double)(unsigned)r_) + alpha);
				beta *= beta;
				offW = -lam; diagW = lam * beta - lam;
			}
			// (the inverse destroys its input: a copy of the reduced H H^T, the exchange buffer stays the caller's)
			HIPX(hipMemcpyAsync(HHt_, ex_hht, sizeof(T) * (size_t)RP_ * RP_, hipMemcpyDeviceToDevice, stream_));
			if (Status st = normal_inverse(HHt_, offW, diagW)) return st;
			if (compute_error) HIPX(hipMemcpyAsync(Wold_, Wt_, sizeof(T) * (size_t)RP_ * mpad_, hipMemcpyDeviceToDevice, stream_));
			HIPX(launch_panel_update<T>(PANEL_LS, Wt_, exchange, 1, 0, Qinv_, RP_, (int)mpad_, eps, nullptr, m_, sumsq_part_, compute_error ? numW_ : nullptr, stream_,
			                            wpart, nullptr, 0, qx3_));
			// tr(W_old^T (V H^T)) over r diagonals (ALS :199-205)
			if (compute_error) HIPX(launch_row_dot<T>(Wold_, numW_, RP_, r_, mpad_, psN_, stream_, rowdot_part_));
			if (Status st = normalize_w(wpart != nullptr, norm_parts)) return st;
		}
		if (compute_error) { if (Status st = fetch_error_terms(r_)) return st; }
		return ST_OK;
	}
	if constexpr (std::is_same<T, float>::value) {
		if (fused_capable()) {
			// U_W on the all-reduced sums: one "slab" (the exchange panel), Q = the reduced H H^T  (a team of one: the split-K slabs as w_products left them)
			if (sole_rank_ && gram_image_) { if (Status s = mu64_update(true, slabs_, planW_.splits, slab_stride_, ex_hht, compute_error)) return s; }
			else if (Status s = mu64_update(true, exchange, 1, 0, ex_hht, compute_error)) return s;
			state_.wx3_valid = x3_;
			normalize_next_ = 1;
			state_.w_pending = true;
			if (compute_error) { if (Status s = fetch_error_terms(n_)) return s; }
			return ST_OK;
		}
	}
	if (compute_error) {
		const T* wtw = tri_ ? reinterpret_cast<const T*>(Gw_raw_) : G_;      // MU: W^T W of this iteration's H step (rank-256 bf16 path: the unscaled Gram matrix + tri_trace_scale())
		if (alg_ == ALG_NSNMF) {                            // unsmoothed W^T W (AlgorithmNonSmoothNMF.h:201-202)
			if (tri_) wtw = reinterpret_cast<const T*>(Gw_raw_);      // (by-product of this iteration's H step)
			else { HIPX(launch_gram<T>(Wt_, RP_, m_, gram_parts_, gram_part_, G2_, stream_)); wtw = G2_; }
		}
		HIPX(launch_trace_small<T>(ex_hht, wtw, RP_, r_, psR_, stream_, tri_trace_scale()));
		if (Status s = fetch_error_terms(n_)) return s;
	}
	state_.wx3_valid = false;
	if (tri_) return tri_update_w(exchange, 1, 0, (sole_rank_ && state_.qx3_holds_hht) ? nullptr : ex_hht);
	HIPX(launch_panel_update<T>(PANEL_MU, Wt_, exchange, 1, 0, ex_hht, RP_, (int)mpad_, eps, nullptr, m_, sumsq_part_, nullptr, stream_, nullptr, nullptr, 0, qx3_));
	HIPX(launch_normalize_panel<T>(Wt_, RP_, (int)mpad_, sumsq_part_, panel_update_parts(RP_, sizeof(T), (int)mpad_), stream_));
	return ST_OK;
}

// W step of a column-sharded run whose ranks read each other's exchange buffers (comm.h, direct_exchange): the W update sums the ranks' (V_g H_g^T)^T panels in
// its prologue, in rank order -- every rank adds the same values in the same order, so the replicas of W stay bit-identical; the r x r parts are summed first
// (one small launch; nothing to do for a team of one).  Rank-64 multiplicative update on the split-operand path only (direct_w_finish()).
template <typename T>
Status Engine<T>::w_finish_peers(const T* const* exchanges, int count, bool compute_error) {
	column_shard_ = true;
	if (prm_.is_masked()) return masked_refuses("w_finish_peers");
	if (beta_dense_) return beta_refuses("w_finish_peers");
	if (!direct_w_finish() || count < 1 || count > PEER_SLABS_MAX || exchanges == nullptr) return ST_INVALID;
	if constexpr (std::is_same<T, float>::value) {
		PeerSlabs panels = {}, hhts = {};
		panels.count = hhts.count = count;
		for (int p = 0; p < count; ++p) { panels.p[p] = exchanges[p]; hhts.p[p] = exchanges[p] + (long)RP_ * mpad_; }
		const float* Q = hhts.p[0];
		if (count > 1) { HIPX(launch_sum_peers(hhts, HHt_, RP_ * RP_, stream_)); Q = HHt_; }
		if (Status s = mu64_update(true, nullptr, count, 0, Q, compute_error, &panels)) return s;
		state_.wx3_valid = x3_;
		normalize_next_ = 1;
		state_.w_pending = true;
		if (compute_error) { if (Status s = fetch_error_terms(n_)) return s; }
	}
	return ST_OK;
}

// ---- row-block form of the W step (one block per rank, see engine.h) -----------------------------------------------
template <typename T>
Status Engine<T>::w_update_rows(const T* num_rows, const T* hht, long row0, long rows, bool compute_error, T* colsq) {
	column_shard_ = true;
	if (prm_.is_masked()) return masked_refuses("w_update_rows");
	if (beta_dense_) return beta_refuses("w_update_rows");
	if (alg_ != ALG_MU && alg_ != ALG_NSNMF) return ST_INVALID;
	if (rows <= 0 || rows % 128 != 0 || row0 < 0 || row0 % 128 != 0 || row0 + rows > mpad_) return ST_INVALID;
	const T eps = std::numeric_limits<T>::epsilon();
	// Gw_raw_ is the Gram matrix of the panel WITHOUT its pending column scale: the trace below needs that scale even when materialize_w() is about to
	// fold it into the panel (a caller that used w_finish() before: ADVICE r3) -- the staged sums stay where they are
	const T* trace_scale = tri_trace_scale();
	if (Status s = materialize_w(false)) return s;      // (a pending column scale belongs to the old W; fold it in first.  This rank's rows are current: no gather)
	if (compute_error) {
		const T* wtw = tri_ ? reinterpret_cast<const T*>(Gw_raw_) : G_;      // MU: W^T W of this iteration's H step (rank-256 bf16 path: the unscaled Gram matrix + its scale)
		if (alg_ == ALG_NSNMF) {                            // unsmoothed W^T W (AlgorithmNonSmoothNMF.h:201-202)
			if (tri_) wtw = reinterpret_cast<const T*>(Gw_raw_);
			else { HIPX(launch_gram<T>(Wt_, RP_, m_, gram_parts_, gram_part_, G2_, stream_)); wtw = G2_; }
		}
		HIPX(launch_trace_small<T>(hht, wtw, RP_, r_, psR_, stream_, trace_scale));
		if (Status s = fetch_error_terms(n_)) return s;
	}
	const long valid = std::max<long>(0, std::min<long>(rows, (long)m_ - row0));
	HIPX(launch_panel_update<T>(PANEL_MU, Wt_ + row0 * RP_, num_rows, 1, 0, hht, RP_, (int)rows, eps, nullptr, (int)valid, sumsq_part_, nullptr, stream_,
	                            nullptr, nullptr, 0, qx3_));
	if constexpr (std::is_same<T, float>::value) {
		if (tri_) {
			HIPX(launch_colsq_stage(sumsq_part_, RP_, panel_update_parts(RP_, sizeof(T), (int)rows), colsq_, colsq, stream_));
			return ST_OK;
		}
	}
	HIPX(launch_reduce_partials<T>(sumsq_part_, panel_update_parts(RP_, sizeof(T), (int)rows), RP_, colsq, RP_, stream_));
	return ST_OK;
}

template <typename T>
Status Engine<T>::w_normalize_rows(long row0, long rows, T* colsq) {
	if (prm_.is_masked()) return masked_refuses("w_normalize_rows");
	if (beta_dense_) return beta_refuses("w_normalize_rows");
	if (rows <= 0 || rows % 128 != 0 || row0 < 0 || row0 + rows > mpad_) return ST_INVALID;
	// colsq: the r sums of squares over ALL rows (one "partial"): kernel::normalizeColumns' sum > 0 ? x / sqrt(sum) : x
	if constexpr (std::is_same<T, float>::value) {
		if (tri_) {
			// the same pass leaves the bf16 fragments of the normalised rows for the next W^T V (unsmoothed: S is applied to the product's output)
			HIPX(launch_finish_panel_bf16(Wt_, RP_, r_, row0, rows, colsq, colsq == colsq_ ? colsq_parts_ : 1, 0.0f, 1.0f, Wtb_, ksH_, stream_));
			state_.tri_rows_cover = row0 == 0 && rows == mpad_;
			state_.wtb_valid = state_.tri_rows_cover;
			state_.tri_gw_ready = false;
			return ST_OK;
		}
	}
	HIPX(launch_normalize_panel_v2<T>(Wt_ + row0 * RP_, RP_, (int)rows, colsq, 1, stream_));
	return ST_OK;
}

// ---- padded rank 256, bf16 product operands (kernels_tri.hip) ---------------------------------------------------------------------
template <typename T>
Status Engine<T>::tri_prepare_w(GramReduceArgs* ride) {
	if constexpr (std::is_same<T, float>::value) {
		const bool wide = qx3_ != nullptr && panel_update_wide_available(RP_);
		if (!state_.wtb_valid) {
			if (Status s = ensure_w_rows()) return s;      // (the fp32 rows of the other ranks first: engine.h, w_fragment_exchange)
			// plain re-rounding of the panel as it lies (no smoothing, no normalisation: W is as the caller / the gather left it)
			HIPX(launch_finish_panel_bf16(Wt_, RP_, r_, 0, mpad_, nullptr, 0, 0.0f, 1.0f, Wtb_, ksH_, stream_));
			state_.wtb_valid = true;
		}
		if (!state_.tri_gw_ready) {
			// W^T W of the ROUNDED W (the matrix the product multiplies V with), as the reduction leaves it: Gw_raw_ and its split image are NOT normalised
			// and not smoothed -- the H update applies D and S around its r x r product (PanelTriExtras::den_transform), the error term's trace applies D
			// (AlgorithmNonSmoothNMF.h:201-202 wants the unsmoothed W^T W).  Round 3 first ran k_smooth_gram here (6.5 us) and a staging launch for D (4.7 us).
			// The diagonal of the matrix IS the new pending scale: sums of squares of the rounded columns (one "staged" vector).
			if (ride != nullptr && tri_ride_w_) {
				// as passengers of the W^T V launch the caller is about to make: every consumer (H update, error trace, the next W update's pending scale) runs behind it
				ride->tri_frags = Wtb_; ride->tri_ks = ksH_; ride->tri_partial = gram_tri_part_; ride->tri_counters = tri_ride_counters_; ride->G = Gw_raw_; ride->tri_x3 = wide ? qx3_ : nullptr; ride->tri_diag = state_.tri_scale_from_gram ? colsq_ : nullptr;
			} else HIPX(launch_gram_tri_bf16_image(Wtb_, RP_, ksH_, num_cus_, gram_tri_part_, Gw_raw_, wide ? qx3_ : nullptr, state_.tri_scale_from_gram ? colsq_ : nullptr, num_cus_, stream_));
			if (state_.tri_scale_from_gram) { colsq_parts_ = 1; state_.tri_scale_from_gram = false; }
			state_.tri_gw_ready = true;
			state_.qx3_holds_g = wide;
		}
	}
	return ST_OK;
}

// hht = (S H)(S H)^T for the W step, from the bf16 fragments of the smoothed columns the H update left in Hb_ -- the Gram matrix of exactly the operand
// V is multiplied with.  local_q: hht stays what the W update multiplies with (no reduction over ranks in between), so the reduction also leaves its split
// image in qx3_ and the update's launcher need not pack it (k_pack_panel_x3, 4.9 us).
template <typename T>
Status Engine<T>::tri_prepare_h(T* hht, bool local_q, GramReduceArgs* ride) {
	if constexpr (std::is_same<T, float>::value) {
		if (!state_.hb_valid) {
			// H did not come from this engine's H update (set_factors / randomize between the two half-steps): one finishing pass makes the fragments
			const auto [off, diag] = smoothing_constants();
			HIPX(launch_finish_panel_bf16(H_, RP_, r_, 0, npad_, nullptr, 0, off, diag, Hb_, ksW_, stream_));
			state_.hb_valid = true;
		}
		const bool image = local_q && qx3_ != nullptr && panel_update_wide_available(RP_);
		if (image && ride != nullptr && tri_ride_h_) { ride->tri_frags = Hb_; ride->tri_ks = ksW_; ride->tri_partial = gram_tri_part_; ride->tri_counters = tri_ride_counters_; ride->G = hht; ride->tri_x3 = qx3_; ride->tri_diag = nullptr; }      // (rides in the V (S H)^T launch)
		else if (image) HIPX(launch_gram_tri_bf16_image(Hb_, RP_, ksW_, num_cus_, gram_tri_part_, hht, qx3_, nullptr, num_cus_, stream_));
		else HIPX(launch_gram_tri_bf16(Hb_, RP_, ksW_, num_cus_, gram_tri_part_, hht, nullptr, 0, num_cus_, stream_));
		state_.qx3_holds_g = false;
		state_.qx3_holds_hht = image;
	}
	return ST_OK;
}

// The W update of the rank-256 bf16 path on the whole panel: num = the reduced (V (S H)^T)^T panel (S slabs), hht its r x r operand
// (nullptr: its split image is in qx3_).  ONE pass over the panel: the update kernel reads the old rows with their pending column scale, writes the new
// rows unnormalised, their bf16 fragments (what the next W^T V multiplies with) and the partial sums of squares; the column normalisation
// (kernel::normalizeColumns, KernelNormalizeColumns.cu:37-58) becomes the new pending scale.  Round 2 followed the update with k_finish_panel_bf16
// (read + write of the panel, 30 us at config 4) and took the Gram matrix from the fp32 panel by split operands (k_gram_tri_x3, 29 us).
template <typename T>
Status Engine<T>::tri_update_w(const T* num, int S, long stride, const T* hht) {
	if constexpr (std::is_same<T, float>::value) {
		const T eps = std::numeric_limits<T>::epsilon();
		const int parts = panel_update_parts(RP_, sizeof(T), (int)mpad_);
		state_.wx3_valid = false;
		PanelTriExtras ex;
		if (state_.tri_scale_pending) { ex.old_colsq = colsq_; ex.old_colsq_parts = colsq_parts_; }
		ex.frag_out = Wtb_; ex.frag_KS = ksH_;
		// the old rows enter W (SH)(SH)^T rounded to bf16: 63.7 -> 52.3 us, W's distance from the fp64 oracle unchanged (3.4e-4 vs 3.2e-4 after 10 iterations,
		// 1.17e-3 vs 1.16e-3 after 40, tools/tri_accuracy.py); NMFAMD_TRI_FP32_DEN=1 keeps the six-term product
		ex.old_as_bf16 = tri_w_den_bf16_;
		HIPX(launch_panel_update<T>(PANEL_MU, Wt_, num, S, stride, hht, RP_, (int)mpad_, eps, nullptr, m_, nullptr, nullptr, stream_, nullptr, nullptr, 0, qx3_, &ex));
		state_.qx3_holds_g = state_.qx3_holds_hht = false;
		// The new pending scale comes out of the next Gram reduction (tri_prepare_w): d(c) = 1 / sqrt(sum of squares of the ROUNDED column c) -- the column
		// norms of the matrix the product multiplies with; they differ from the fp32 norms by ~1e-5 relative (zero-mean rounding over m rows).  Every consumer
		// (H update, next W update, error trace, materialize_w) runs after that reduction.
		state_.tri_scale_pending = true;
		state_.tri_scale_from_gram = true;
		(void)parts;
		state_.wtb_valid = true;
		state_.tri_rows_cover = true;
		state_.tri_gw_ready = false;
		return ST_OK;
	}
	return ST_INVALID;
}

template <typename T>
bool Engine<T>::fused_capable() const {
	// (evaluated before allocate(): no tiled_ here.  nsNMF (round 6): only on the split-operand products with the Gram matrices taken from the images -- x3_ is false
	//  until the plan has chosen that path, so the one-pass request and the native-fp32 plan never see it)
	return std::is_same<T, float>::value && RP_ == 64 && !prm_.is_beta_dense() &&
	       (alg_ == ALG_MU || (alg_ == ALG_NSNMF && x3_ && !bf16_ && !sparse_ && std::getenv("NMFAMD_GRAM_PARTIALS") == nullptr)) &&
	       std::getenv("NMFAMD_FORCE_VALU") == nullptr && std::getenv("NMFAMD_NO_FUSED_MU") == nullptr;
}

// fp32 at padded ranks 128 ... 512 on the split-operand products (ranks 65 ... 512 in float: what rounds 1 - 5 ran as the generic sequence of 14 launches):
// multiplicative update and nsNMF.  The bf16 mode keeps its own path.
template <typename T>
bool Engine<T>::fused32w_capable() const {
	return std::is_same<T, float>::value && x3_ && tiled_ && !bf16_ && !sparse_ && (alg_ == ALG_MU || alg_ == ALG_NSNMF) && RP_ >= 128 && panel_update_wide_available(RP_) &&
	       gram_wide_available(RP_) && wide_q_image_ &&
	       std::getenv("NMFAMD_FORCE_VALU") == nullptr && std::getenv("NMFAMD_NO_FUSED_MU") == nullptr;
}

// One iteration in EIGHT launches, none of them a pack, a smoothing pass or a normalisation (the generic sequence: 14.2 at r = 128):
//   Gram slices of Wt (k_gram_wide_x3) -> k_gram_reduce_x3: Wt^T Wt, ITS split image (the update's operand) and the pending column scale d
//   Wt^T V from the split image the W update left
//   H update (FX): num <- S D (sum of the slabs), den = S D (Wt^T Wt) D S h around the MFMA product; writes H, S H and the split image of the next product's operand
//   the same for S H: Gram slices -> reduction + split image; V (S H)^T; W update (old rows read as Wt d, result unnormalised, its split image, sums of squares)
// The float counterpart of iterate_fused64 without passengers: the split-operand product kernel is the headline's and stays as it is.
template <typename T>
Status Engine<T>::iterate_fused32w(bool compute_error) {
	if constexpr (std::is_same<T, float>::value) {
		const float eps = std::numeric_limits<float>::epsilon();
		const bool ns = alg_ == ALG_NSNMF;
		const auto [off, diag] = smoothing_constants();      // (the identity unless nsNMF)
		const int norm_parts = panel_update_parts(RP_, sizeof(T), (int)mpad_);
		const float* dscale = state_.f32w_pending ? f32w_scale_ : nullptr;
		// H step
		if (f32w_ride_h_ > 0) {
			GramReduceArgs rg = {nullptr, 0, nullptr, nullptr, 0};
			rg.wide_P = Wt_; rg.wide_len = m_; rg.wide_parts = f32w_ride_h_; rg.wide_partial = gram_part_;
			if (Status s = product_h(Wt_, &rg, state_.wx3_valid)) return s;
			HIPX(launch_gram_reduce_x3(gram_part_, f32w_ride_h_, RP_, G_, qx3_, state_.f32w_pending ? sumsq_part_ : nullptr, norm_parts, f32w_scale_, stream_));
		} else {
			HIPX(launch_gram_wide_fused_f32(Wt_, RP_, m_, gram_parts_, gram_part_, G_, qx3_, state_.f32w_pending ? sumsq_part_ : nullptr, norm_parts, f32w_scale_, stream_));
			if (Status s = product_h(Wt_, nullptr, state_.wx3_valid)) return s;
		}
		state_.wx3_valid = true;
		PanelFusedF32 fh;
		fh.h_side = 1; fh.scale = dscale; fh.r = r_;
		if (ns) { fh.smooth = 1; fh.off = off; fh.diag = diag; fh.smooth_out = Hs_; }
		fh.x3_out = Hx3_; fh.x3_ks = ksW_;
		HIPX(launch_panel_update_wide_f32(PANEL_MU, H_, slabs_, planH_.splits, slab_stride_, nullptr, RP_, (int)npad_, eps, compute_error ? psN_ : nullptr, n_, nullptr, nullptr,
		                                  stream_, qx3_, nullptr, &fh));
		// W step
		const float* Fh = ns ? Hs_ : H_;
		if (f32w_ride_w_ > 0) {
			GramReduceArgs rg = {nullptr, 0, nullptr, nullptr, 0};
			rg.wide_P = Fh; rg.wide_len = n_; rg.wide_parts = f32w_ride_w_; rg.wide_partial = gram_part_;
			if (Status s = product_w(Fh, &rg, nullptr, true)) return s;
			HIPX(launch_gram_reduce_x3(gram_part_, f32w_ride_w_, RP_, HHt_, qx3_, nullptr, 0, nullptr, stream_));
		} else {
			HIPX(launch_gram_wide_fused_f32(Fh, RP_, n_, gram_parts_, gram_part_, HHt_, qx3_, nullptr, 0, nullptr, stream_));
			if (Status s = product_w(Fh, nullptr, nullptr, true)) return s;
		}
		state_.hx3_valid = !ns;
		// tr((S H)(S H)^T W^T W) with the W^T W of this iteration's H step (the pending scale applied on the way: D G D)
		if (compute_error) HIPX(launch_trace_small<T>(HHt_, G_, RP_, r_, psR_, stream_, nullptr, dscale));
		PanelFusedF32 fw;
		fw.old_scale = dscale;
		fw.x3_out = Wx3_; fw.x3_ks = ksH_;
		HIPX(launch_panel_update_wide_f32(PANEL_MU, Wt_, slabs_, planW_.splits, slab_stride_, nullptr, RP_, (int)mpad_, eps, nullptr, m_, sumsq_part_, nullptr,
		                                  stream_, qx3_, nullptr, &fw));
		state_.f32w_pending = true;
		state_.wx3_valid = true;          // (of the panel as it lies)
		state_.gram_w_ready = false;
		if (compute_error) { if (Status s = fetch_error_terms(n_)) return s; }
	}
	return ST_OK;
}

// Double precision, multiplicative update and nsNMF on the MFMA kernels of kernels_f64.hip at any padded rank they cover: what the reference's own callers run
// (example/main.cpp: NmfDescription<double>, nsNMF, r = 158; the R binding).  NMFAMD_NO_FUSED_MU=1 keeps the generic launch sequence (the cross-check path).
template <typename T>
bool Engine<T>::fused64_capable() const {
	return std::is_same<T, double>::value && tiled_ && !sparse_ && !bf16_ && !beta_dense_ && (alg_ == ALG_MU || alg_ == ALG_NSNMF) && RP_ % 64 == 0 && RP_ <= 512 &&
	       (RP_ == 64 || panel_update_wide_f64_available(RP_)) && std::getenv("NMFAMD_FORCE_VALU") == nullptr && std::getenv("NMFAMD_NO_FUSED_MU") == nullptr;
}

// One iteration in FOUR launches (the generic sequence: 10 at padded rank 64, 12 for nsNMF -- smoothing x 2, Gram + reduction x 2, product x 2, update x 2,
// normalise + compaction of its partial sums):
//   1. W^T V from the panel as it lies (Wt: unnormalised, unsmoothed) + passengers: Wt^T Wt, and the column scale d from the last W update's sums of squares
//   2. H update: numerator S D (sum of the slabs) -- (Wt D S)^T V = S D (Wt^T V) --, denominator S D (Wt^T Wt) D S h with D and S applied around the MFMA
//      product; writes H and, nsNMF, the smoothed panel S H
//   3. V (S H)^T + passengers: (S H)(S H)^T
//   4. W update: old rows read as W d, result left unnormalised + per-workgroup sums of squares (the first half of kernel::normalizeColumns)
// References: AlgorithmMultiplicativeFrobenius.h:165-248, AlgorithmNonSmoothNMF.h:174-218 (same operation order per element; the column scale is a factor
// 1 / sqrt(sum) where the reference divides by sqrt(sum): 1 ulp, inside the 1e-9 the fp64 tests ask).
// launch 1 of the fused double-precision iteration: W^T V from the panel as it lies + the Gram passengers (W^T W, the pending column scale)
template <typename T>
Status Engine<T>::fused64_product_h() {
	if constexpr (std::is_same<T, double>::value) {
		struct RideGuard { const GramRideF64*& p; ~RideGuard() { p = nullptr; } } guard{ride64_};
		GramRideF64 gw = {};
		gw.P = Wt_; gw.len = m_; gw.slices = f64_slices_h_; gw.partial = f64_partial_; gw.counters = f64_counters_; gw.G = G_;
		gw.sumsq_part = state_.f64_pending ? sumsq_part_ : nullptr; gw.sumsq_parts = panel_update_parts(RP_, sizeof(T), (int)mpad_); gw.scale_out = f64_scale_;
		if (const char* e = tuning_env("NMFAMD_RIDE64_STOP")) gw.stop = std::atoi(e);
		gw.stamps = f64_stamps_;
		gw.items = f64_items_h_;
		ride64_ = &gw;
		return product_h(Wt_);
	}
	return ST_OK;
}

template <typename T>
Status Engine<T>::iterate_fused64(bool compute_error) {
	if constexpr (std::is_same<T, double>::value) {
		const double eps = std::numeric_limits<double>::epsilon();
		const bool ns = alg_ == ALG_NSNMF;
		const auto [off, diag] = smoothing_constants();      // (the identity unless nsNMF)
		struct RideGuard { const GramRideF64*& p; ~RideGuard() { p = nullptr; } } guard{ride64_};
		// Error iterations of a single engine: the H update writes its n terms and the W update's trace workgroups their r terms straight into the pinned host
		// buffer (its device address): no k_trace_small launch, no copy launch (as iterate_mu64 does since round 5) -- 1.2 us per iteration on average at the
		// reference example's shape.  The previous error iteration's values leave the buffer first.
		ps_direct_ = compute_error && !error_terms_stay_ && pin_psN_dev_ != nullptr && tuning_env("NMFAMD_ERROR_COPY_KERNEL") == nullptr;
		if (ps_direct_) finalize_error(false);
		struct DirectGuard { bool& f; ~DirectGuard() { f = false; } } direct_guard{ps_direct_};
		T* const ps_n = ps_direct_ ? pin_psN_dev_ : psN_;
		T* const ps_r = ps_direct_ ? pin_psN_dev_ + ps_stride_ : psR_;
		// 1 (already enqueued by begin_next_iteration() behind the previous error iteration: nothing has touched W, V or the scratch since)
		if (state_.f64_product_ahead) state_.f64_product_ahead = false;
		else if (Status s = fused64_product_h()) return s;
		// 2
		PanelFusedF64 fh = {};
		const double* dscale = state_.f64_pending ? f64_scale_ : nullptr;
		fh.h_side = (dscale != nullptr || ns) ? 1 : 0;      // (a normalised W and no smoothing: G_ is W^T W as the update needs it)
		fh.scale = dscale; fh.r = r_;
		if (ns) { fh.smooth = 1; fh.off = off; fh.diag = diag; fh.smooth_out = Hs_; }
		fh.stamps = f64_stamps_ != nullptr ? f64_stamps_ + 1l * 4096 * 8 : nullptr;
		if (RP_ == 64) HIPX(launch_panel_update64_f64(PANEL_MU, H_, slabs_, planH_.splits, slab_stride_, G_, (int)npad_, eps, compute_error ? ps_n : nullptr, n_, nullptr, nullptr, stream_, &fh));
		else HIPX(launch_panel_update_wide_f64(PANEL_MU, H_, slabs_, planH_.splits, slab_stride_, G_, RP_, (int)npad_, eps, compute_error ? ps_n : nullptr, n_, nullptr, nullptr, stream_, &fh));
		// 3
		const double* Fh = ns ? Hs_ : H_;
		GramRideF64 gh = {};
		gh.P = Fh; gh.len = n_; gh.slices = f64_slices_w_; gh.partial = f64_partial_; gh.counters = f64_counters_; gh.G = HHt_;
		if (const char* e = tuning_env("NMFAMD_RIDE64_STOP")) gh.stop = std::atoi(e);
		gh.stamps = f64_stamps_ != nullptr ? f64_stamps_ + 2l * 4096 * 8 : nullptr;
		gh.items = f64_items_w_;
		ride64_ = &gh;
		if (Status s = product_w(Fh)) return s;
		ride64_ = nullptr;
		// 4 -- and, on error iterations, tr((S H)(S H)^T W^T W) with the W^T W of this iteration's H step, unsmoothed (AlgorithmNonSmoothNMF.h:201-202;
		// AlgorithmMultiplicativeFrobenius.h:212) by extra workgroups of the same launch (G_ is the Gram matrix of the panel as it lies: the pending scale is applied
		// on the way, D G D = W^T W of the normalised W)
		PanelFusedF64 fw = {};
		fw.old_scale = dscale;
		if (compute_error) { fw.trace_a = HHt_; fw.trace_b = G_; fw.trace_scale = dscale; fw.trace_out = ps_r; fw.trace_r = r_; }
		fw.stamps = f64_stamps_ != nullptr ? f64_stamps_ + 3l * 4096 * 8 : nullptr;
		if (RP_ == 64) HIPX(launch_panel_update64_f64(PANEL_MU, Wt_, slabs_, planW_.splits, slab_stride_, HHt_, (int)mpad_, eps, nullptr, m_, sumsq_part_, nullptr, stream_, &fw));
		else HIPX(launch_panel_update_wide_f64(PANEL_MU, Wt_, slabs_, planW_.splits, slab_stride_, HHt_, RP_, (int)mpad_, eps, nullptr, m_, sumsq_part_, nullptr, stream_, &fw));
		state_.f64_pending = true;
		state_.gram_w_ready = false;
		state_.hx3_valid = false; state_.wx3_valid = false;
		if (compute_error) { if (Status s = fetch_error_terms(n_)) return s; }
	}
	return ST_OK;
}

// GDCLS and the ALS family never smooth their factors, so the Gram matrix the next half-step needs is the Gram matrix of
// exactly what the update kernel has just written: at fp32 / padded rank 64 that kernel emits it as partial matrices
// (64 panel rows each) and the 16-block reduction of the fused MU path replaces a pass over the panel.
template <typename T>
bool Engine<T>::gram_from_update() const {
	return std::is_same<T, float>::value && alg_ >= ALG_GDCLS && alg_ <= ALG_AHCLS && panel_update_delivers_gram(RP_, sizeof(T)) &&
	       tuning_env("NMFAMD_NO_GRAM_FROM_UPDATE") == nullptr;
}

// Column normalisation of W after its update (kernel::normalizeColumns).  With partial Gram matrices of the unnormalised W
// at hand: their reduction yields the column scales 1 / ||W(:, c)|| and W^T W of the NORMALISED W in one 16-block launch,
// W is scaled in place, and the next H step finds its Gram matrix ready.  Otherwise: norms from the sum-of-squares partials.
template <typename T>
Status Engine<T>::normalize_w(bool from_gram_partials, int norm_parts) {
	if constexpr (std::is_same<T, float>::value) {
		if (from_gram_partials) {
			if (x3_ && Graw64_ != nullptr && tuning_env("NMFAMD_NORMALIZE_TWO_LAUNCHES") == nullptr) {
				// ONE launch (round 4): column scales from the update's sums of squares, G = D (sum of the partial Gram matrices) D, W <- W D and its split image
				HIPX(launch_gram64_reduce_scale_all(gramW_part_, (int)(mpad_ / 64), sumsq_part_, norm_parts, G_, scale_, Wt_, (int)mpad_, Wx3_, ksH_, stream_));
			} else if (x3_ && Graw64_ != nullptr) {
				// reduction, then ONE launch: scales from the raw diagonal, G = D Graw D, W <- W D and its split image for the next W^T V
				HIPX(launch_gram64_normalize_all(gramW_part_, (int)(mpad_ / 64), Graw64_, G_, scale_, Wt_, (int)mpad_, Wx3_, ksH_, stream_));
			} else {
			HIPX(launch_gram64_from_partials(gramW_part_, (int)(mpad_ / 64), G_, scale_, stream_));
			// the scaling pass also leaves the split image of the normalised W for the next W^T V
			HIPX(launch_mu64_apply_scale(Wt_, (int)mpad_, scale_, stream_, x3_ ? Wx3_ : nullptr, ksH_));
			}
			state_.wx3_valid = x3_;
			state_.gram_w_ready = true;
			return ST_OK;
		}
	}
	state_.gram_w_ready = false;
	HIPX(launch_normalize_panel<T>(Wt_, RP_, (int)mpad_, sumsq_part_, norm_parts, stream_));
	return ST_OK;
}

template <typename T>
Status Engine<T>::ensure_w_rows() {
	// (row-block sharded run with the fragment exchange: whoever wants the WHOLE fp32 panel gets the other ranks' rows first -- a collective, engine.h)
	if (state_.w_rows_stale) {
		if (!w_gather_hook_) { last_error_ = "the fp32 rows of the other ranks' blocks were not gathered (the sharded run that owns the exchange is closed)"; return ST_INVALID; }
		if (Status s = w_gather_hook_()) return s;
		state_.w_rows_stale = false;
	}
	return ST_OK;
}

template <typename T>
Status Engine<T>::materialize_w(bool whole_panel) {
	if (whole_panel) { if (Status s = ensure_w_rows()) return s; }
	if (state_.f32w_pending) {
		// the fused fp32 iteration at padded ranks >= 128 left W unnormalised (and the split image of THAT panel in Wx3_)
		HIPX(launch_normalize_panel<T>(Wt_, RP_, (int)mpad_, sumsq_part_, panel_update_parts(RP_, sizeof(T), (int)mpad_), stream_));
		state_.f32w_pending = false;
		state_.wx3_valid = false;
		state_.gram_w_ready = false;
	}
	if (state_.kl_scale_pending) {
		// the KL iteration left W unnormalised (iterate_kl): the pass it skipped
		HIPX(launch_normalize_panel<T>(Wt_, RP_, (int)mpad_, sumsq_part_, (int)(mpad_ / 128), stream_));
		state_.kl_scale_pending = false;
	}
	if (state_.f64_pending) {
		// the fused double-precision iteration left W unnormalised: the second half of kernel::normalizeColumns, as the generic iteration runs it after every W update
		HIPX(launch_normalize_panel<T>(Wt_, RP_, (int)mpad_, sumsq_part_, panel_update_parts(RP_, sizeof(T), (int)mpad_), stream_));
		state_.f64_pending = false;
		state_.f64_product_ahead = false;      // (an ahead launch multiplied with the unnormalised panel and its pending scale)
		state_.gram_w_ready = false;
	}
	if constexpr (std::is_same<T, float>::value) {
		if (state_.w_pending) {
			// column norms from the partial Grams of the unnormalised W, then W <- W diag(scale)
			GramReduceArgs rg = gram_args(true, G2_, scale_, 1);
			if (Status s = standalone_gram(rg)) return s;
			HIPX(launch_mu64_apply_scale(Wt_, (int)mpad_, scale_, stream_));
			state_.w_pending = false;
			state_.fused_ready = false;
			state_.h_product_ahead = false; state_.f64_product_ahead = false;
			state_.wx3_valid = false;
		}
		if (state_.tri_scale_pending) {
			if (state_.tri_scale_from_gram) { if (Status s = tri_prepare_w()) return s; }      // (the scale of the last W update comes out of the Gram reduction)
			// rank-256 bf16 path: W <- W diag(d), d from the staged sums of squares; the fragments (of the unscaled panel) are re-made on demand, the Gram matrices already
			// describe the normalised W
			HIPX(launch_scale_panel_tri(Wt_, RP_, mpad_, colsq_, colsq_parts_, nullptr, stream_));
			state_.tri_scale_pending = false;
			state_.wtb_valid = false;
			state_.tri_gw_ready = false;        // (Gw_raw_ and its image describe the unscaled panel)
			state_.qx3_holds_g = false;
		}
	}
	return ST_OK;
}

// One pass over V: G = W^T W (split image of W), then ONE persistent launch for W^T V, the H update and V H^T, then U_W.
template <typename T>
Status Engine<T>::iterate_onepass(bool compute_error) {
#ifdef NMFAMD_DIAG_BUILD
	if constexpr (std::is_same<T, float>::value) {
		if (!state_.fused_ready) { normalize_next_ = 0; state_.fused_ready = true; }
		if (!state_.wx3_valid) { HIPX(launch_pack_panel_x3(Wt_, RP_, m_, Wx3_, ksH_, stream_)); state_.wx3_valid = true; }
		GramReduceArgs rgW = gram_args(true, G_, scale_, normalize_next_);
		rgW.ksplit = 0; rgW.spread = 0; rgW.G = G_;       // (the persistent launch reads the finished matrix)
		if (Status s = standalone_gram(rgW)) return s;
		OnePassArgs a;
		a.V = V_; a.tile_stride = strideV_;
		a.Wx3 = Wx3_; a.G = G_; a.scale = scale_; a.ps = op_ps4_; a.ps_stride = npad_;
		if constexpr (std::is_same<T, float>::value) { a.H = H_; a.H_out = op_H2_; }
		a.slabs = op_slabs_; a.slab_stride = (long)RP_ * mpad_;
		a.hh_part = op_hh_part_; a.part_scratch = op_part_; a.hfrag_scratch = op_hfrag_;
		a.ticket = op_ctl_; a.abort_flag = op_ctl_ + 8;
		a.tile_rows = (int)(mpad_ / 16); a.w_ks = ksH_; a.n = n_; a.panels = (n_ + 31) / 32;
		a.seq = op_seq_++;
		a.compute_error = compute_error ? 1 : 0;
		a.eps = std::numeric_limits<float>::epsilon();
		a.stamps = op_stamps_;
		record_begin();
#ifdef NMFAMD_DIAG_BUILD
		HIPX(launch_mu64_onepass(a, stream_));
#else
		return ST_INVALID;      // (one_pass_ is never set in the shipped library)
#endif
		record_end();
		std::swap(H_, op_H2_);                             // the new H
		HIPX(launch_reduce_partials<float>(op_hh_part_, ONEPASS_XCDS * ONEPASS_GROUP, 4096, HHt_, 4096, stream_));
		if (compute_error) HIPX(launch_reduce_partials<float>(op_ps4_, 4, npad_, psN_, n_, stream_));   // the four owner waves' parts of the per-column terms
		if (Status s = mu64_update(true, op_slabs_, ONEPASS_XCDS, (long)RP_ * mpad_, HHt_, compute_error)) return s;
		state_.wx3_valid = x3_;
		state_.hx3_valid = false;
		normalize_next_ = 1;
		state_.w_pending = true;
		if (compute_error) {
			if (Status s = fetch_error_terms(n_)) return s;
			if (Status s = onepass_check()) return s;
		}
	}
#else
	(void)compute_error;
#endif
	return ST_OK;
}

// A launch that could not form its groups (an XCD with other than 32 of its workgroups: another kernel held CUs) gives
// up after bounded waits and leaves the abort word set; its outputs are void.
template <typename T>
Status Engine<T>::onepass_check() {
#ifdef NMFAMD_DIAG_BUILD

	HIPX(hipMemcpyAsync(pin_abort_, op_ctl_ + 8, sizeof(unsigned), hipMemcpyDeviceToHost, stream_));
	HIPX(hipStreamSynchronize(stream_));
	if (op_stamps_ != nullptr) {
		// diagnostic builds: the stamps of the last launch go to the file NMFAMD_ONEPASS_STAMPS names
		std::vector<unsigned long long> h(16 * 8 * ONEPASS_XCDS * ONEPASS_GROUP);
		if (hipMemcpy(h.data(), op_stamps_, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost) == hipSuccess) {
			if (FILE* f = std::fopen(tuning_env("NMFAMD_ONEPASS_STAMPS"), "wb")) { std::fwrite(h.data(), sizeof(unsigned long long), h.size(), f); std::fclose(f); }
		}
	}
	if (*pin_abort_ != 0) {
		one_pass_ = false; one_pass_gave_up_ = true;
		last_error_ = "the one-pass iteration could not keep its workgroups resident (another kernel on the device?): factors are void; unset NMFAMD_ONE_PASS";
		return ST_HIP_ERROR;
	}
#endif
	return ST_OK;
}

template <typename T>
Status Engine<T>::iterate_mu64(bool compute_error) {
	if constexpr (std::is_same<T, float>::value) {
		if (one_pass_) return iterate_onepass(compute_error);
		const float eps = std::numeric_limits<float>::epsilon();
		// Error iterations of a single engine: the two update kernels write their n + r terms into the pinned host buffer themselves (its device address): the
		// copy launch behind them (k_copy_small: 4.1 us, every tenth iteration) goes.  The previous error iteration's values leave the buffer first.
		static const bool no_direct = tuning_env("NMFAMD_ERROR_MEMCPY") != nullptr || tuning_env("NMFAMD_ERROR_COPY_KERNEL") != nullptr;
		ps_direct_ = compute_error && gram_image_ && !error_terms_stay_ && pin_psN_dev_ != nullptr && !no_direct;
		if (ps_direct_) finalize_error(false);
		struct DirectGuard { bool& f; ~DirectGuard() { f = false; } } direct_guard{ps_direct_};
		if (!state_.fused_ready) {
			if (!gram_image_) HIPX(launch_mu64_gram_partials(Wt_, (int)mpad_, gramW_part_, stream_));
			normalize_next_ = 0;
			state_.fused_ready = true;
		}
		GramReduceArgs rgW = gram_args(true, G_, scale_, normalize_next_);
		if (state_.h_product_ahead) state_.h_product_ahead = false;      // (begin_next_iteration() enqueued exactly this launch)
		else if (Status s = product_h(Wt_, &rgW, x3_ && state_.wx3_valid)) return s;
		if (Status s = mu64_update(false, slabs_, planH_.splits, slab_stride_, rgW.ksplit > 1 ? reinterpret_cast<const T*>(Gpart_) : G_, compute_error)) return s;
		GramReduceArgs rgH = gram_args(false, HHt_, nullptr, 0);
		if (Status s = product_w(H_, &rgH, nullptr, x3_)) return s;
		if (Status s = mu64_update(true, slabs_, planW_.splits, slab_stride_, HHt_, compute_error)) return s;
		state_.wx3_valid = x3_;
		state_.hx3_valid = false;
		normalize_next_ = 1;
		state_.w_pending = true;
		if (compute_error) {
			if (Status s = fetch_error_terms(n_)) return s;
		}
	}
	return ST_OK;
}

template <typename T>
Status Engine<T>::begin_next_iteration() {
	if constexpr (std::is_same<T, double>::value) {
		// the fused double-precision iteration: its first launch writes the split-K slabs, G_ and the scale vector -- scratch the next iterate() overwrites anyway
		if (!fused64_capable() || f64_partial_ == nullptr || !state_.f64_pending || state_.f64_product_ahead || prm_.divergence != 0) return ST_OK;
		const bool sampled = timing_now_;
		timing_now_ = false;
		const Status s = fused64_product_h();
		timing_now_ = sampled;
		if (s != ST_OK) return s;
		state_.f64_product_ahead = true;
		return ST_OK;
	}
	if constexpr (std::is_same<T, float>::value) {
		if (!fused_capable() || one_pass_ || !state_.fused_ready || state_.h_product_ahead || prm_.divergence != 0 || !x3_ || !state_.wx3_valid) return ST_OK;
		GramReduceArgs rgW = gram_args(true, G_, scale_, normalize_next_);
		// (not sampled: the launch belongs to the NEXT iteration -- or to none, when the threshold ends the run here)
		const bool sampled = timing_now_;
		timing_now_ = false;
		const Status s = product_h(Wt_, &rgW, true);
		timing_now_ = sampled;
		if (s != ST_OK) return s;
		state_.h_product_ahead = true;
	}
	return ST_OK;
}

template <typename T>
Status Engine<T>::set_hals_penalties(double l1W, double l1H, double l2W, double l2H) {
	// (prm_, not beta_dense_: check_parameters() calls this before it has looked at the divergence)
	if (const char* why = hals_penalties_fault(l1W, l1H, l2W, l2H, sizeof(T) == 4, prm_.takes_penalties(hals_family(alg_)))) { last_error_ = why; return ST_INVALID; }
	// kept rounded to T, as the sweeps take them: a value that rounds to 0 in the engine's precision is 0 for the normalisation switch too, and the
	// (T) casts where the sweeps are launched change nothing any more
	prm_.l1W = (double)(T)l1W; prm_.l1H = (double)(T)l1H; prm_.l2W = (double)(T)l2W; prm_.l2H = (double)(T)l2H;
	return ST_OK;
}

template <typename T>
Status Engine<T>::set_hals_sweeps(int h, int w) {
	if (const char* why = hals_sweeps_fault((double)h, (double)w, alg_ == ALG_HALS)) { last_error_ = why; return ST_INVALID; }
	prm_.sweeps_h = h; prm_.sweeps_w = w;
	return ST_OK;
}

template <typename T>
Status Engine<T>::set_missing_solver(const MissingSolver& s) {
	if (const char* why = missing_solver_fault(s.solver, s.sweeps_h, s.sweeps_w, s.l1W, s.l1H, s.l2W, s.l2H, sizeof(T) == 4, prm_.is_masked(), !prm_.is_masked_beta(), r_)) {
		last_error_ = why;
		return ST_INVALID;
	}
	// (nothing derived from a factor outlives a launch of either solver: PanelState has no flag to clear, and the factors stay as they are)
	cd_ = s;
	cd_.l1W = (double)(T)s.l1W; cd_.l1H = (double)(T)s.l1H; cd_.l2W = (double)(T)s.l2W; cd_.l2H = (double)(T)s.l2H;
	return ST_OK;
}

template <typename T>
Status Engine<T>::set_hals_sweep_tolerance(double delta) {
	if (const char* why = hals_sweep_tolerance_fault(delta, alg_ == ALG_HALS)) { last_error_ = why; return ST_INVALID; }
	prm_.sweep_tolerance = delta;
	return ST_OK;
}

template <typename T>
Status Engine<T>::set_nenmf_steps(int h, int w) {
	if (const char* why = nenmf_steps_fault((double)h, (double)w, true, alg_ == ALG_NENMF)) { last_error_ = why; return ST_INVALID; }
	prm_.steps_h = h; prm_.steps_w = w;
	return ST_OK;
}

template <typename T>
Status Engine<T>::set_nenmf_step_tolerance(double delta) {
	if (const char* why = nenmf_step_tolerance_fault(delta, true, alg_ == ALG_NENMF)) { last_error_ = why; return ST_INVALID; }
	prm_.steps_tolerance = delta;
	return ST_OK;
}

// The steps of one NeNMF step launch against slabs_ and G, routed as hals_sweeps routes the sweeps.  Tolerance 0: launch_panel_steps_apg, as before the tolerance
// existed; the counts are the static count and are written when somebody asks.  Tolerance > 0 and a maximum of one step: the same launch and counts of 1.
// Otherwise the dynamic kernel, which writes the counts itself.
template <typename T>
Status Engine<T>::apg_steps(bool w_step, T* P, const T* G, int S, int len_pad, int len_valid, T* ps, T* sumsq_part, T l1, T l2) {
	const int steps = (int)(w_step ? prm_.steps_w : prm_.steps_h);
	(w_step ? hals_counts_w_valid_ : hals_counts_h_valid_) = true;
	if (prm_.steps_tolerance > 0 && steps > 1) {
		// (a double in (0, 1) may round to 0 or to 1 in a float engine: kept inside the launcher's open interval)
		const T tol = std::min(std::max((T)prm_.steps_tolerance, std::numeric_limits<T>::min()), std::nextafter(T(1), T(0)));
		HIPX(launch_panel_steps_apg_dyn<T>(P, slabs_, S, slab_stride_, G, RP_, r_, len_pad, len_valid, ps, sumsq_part, stream_, l1, l2, steps, tol,
		                                   w_step ? hals_counts_w_ : hals_counts_h_));
		(w_step ? hals_static_w_ : hals_static_h_) = 0;
		return ST_OK;
	}
	HIPX(launch_panel_steps_apg<T>(P, slabs_, S, slab_stride_, G, RP_, r_, len_pad, len_valid, ps, sumsq_part, stream_, l1, l2, steps));
	(w_step ? hals_static_w_ : hals_static_h_) = steps;
	return ST_OK;
}

// The sweeps of one HALS step against slabs_ and G.  Tolerance 0: launch_panel_sweeps_hals, as before the tolerance existed -- the counts of the step are then
// the static count, which nobody has to launch anything for: they are written when somebody asks (hals_sweep_counts).  Tolerance > 0 and a maximum of one sweep:
// the same launch (there is nothing to decide) and counts of 1.  Otherwise the dynamic kernel, which writes the counts itself.
template <typename T>
Status Engine<T>::hals_sweeps(bool w_step, T* P, const T* G, int S, int len_pad, int len_valid, T* ps, T* sumsq_part, T l1, T l2) {
	const int sweeps = (int)(w_step ? prm_.sweeps_w : prm_.sweeps_h);
	int* counts = w_step ? hals_counts_w_ : hals_counts_h_;
	(w_step ? hals_counts_w_valid_ : hals_counts_h_valid_) = true;
	if (prm_.sweep_tolerance > 0 && sweeps > 1) {
		HIPX(launch_panel_sweeps_hals_dyn<T>(P, slabs_, S, slab_stride_, G, RP_, r_, len_pad, len_valid, ps, sumsq_part, stream_, l1, l2, sweeps, prm_.sweep_tolerance, counts));
		(w_step ? hals_static_w_ : hals_static_h_) = 0;
		return ST_OK;
	}
	HIPX(launch_panel_sweeps_hals<T>(P, slabs_, S, slab_stride_, G, RP_, r_, len_pad, len_valid, ps, sumsq_part, stream_, l1, l2, sweeps));
	(w_step ? hals_static_w_ : hals_static_h_) = sweeps;
	return ST_OK;
}

template <typename T>
long Engine<T>::hals_sweep_counts(int which, int* out, long capacity) {
	if (alg_ != ALG_HALS) { last_error_ = "HALS sweep counts: only a HALS engine has them"; return -1; }
	return family_counts(which, out, capacity);
}

template <typename T>
long Engine<T>::nenmf_step_counts(int which, int* out, long capacity) {
	if (alg_ != ALG_NENMF) { last_error_ = "NeNMF step counts: only a NeNMF engine has them"; return -1; }
	return family_counts(which, out, capacity);
}

// (the counts of either algorithm of the family; the messages name the engine's own)
template <typename T>
long Engine<T>::family_counts(int which, int* out, long capacity) {
	const bool ne = alg_ == ALG_NENMF;
	if (which != 0 && which != 1) { last_error_ = ne ? "NeNMF step counts: which has to be 0 (H) or 1 (W)" : "HALS sweep counts: which has to be 0 (H) or 1 (W)"; return -1; }
	const long len = which == 0 ? n_ : m_;
	if (!(which == 0 ? hals_counts_h_valid_ : hals_counts_w_valid_)) {
		last_error_ = ne ? "NeNMF step counts: no step of this factor has run yet" : "HALS sweep counts: no step of this factor has run yet";
		return -1;
	}
	if (out == nullptr || capacity < len) {
		last_error_ = ne ? "NeNMF step counts: the output holds fewer than n (m) entries" : "HALS sweep counts: the output holds fewer than n (m) entries";
		return -1;
	}
	const int fixed = which == 0 ? hals_static_h_ : hals_static_w_;
	if (fixed > 0) {      // (the step ran a fixed number of sweeps (steps): nothing was written on the device)
		if (hipStreamSynchronize(stream_) != hipSuccess) return -1;
		for (long i = 0; i < len; ++i) out[i] = fixed;
		return len;
	}
	if (hipMemcpyAsync(out, which == 0 ? hals_counts_h_ : hals_counts_w_, sizeof(int) * (size_t)len, hipMemcpyDeviceToHost, stream_) != hipSuccess ||
	    hipStreamSynchronize(stream_) != hipSuccess) { last_error_ = ne ? "NeNMF step counts: copy failed" : "HALS sweep counts: copy failed"; return -1; }
	return len;
}

template <typename T>
Status Engine<T>::iterate(bool compute_error, bool constant_w) {
	const T eps = std::numeric_limits<T>::epsilon();
	timing_now_ = timing_ && (timing_iter_++ % timing_stride_ == 0);
	if (prm_.is_masked()) return masked_beta_ ? iterate_masked_beta(compute_error, constant_w) : iterate_masked(compute_error, constant_w);      // (before the KL test: a masked engine never has divergence != 0, allocate())
	if (beta_dense_ && minibatch_) {
		if (constant_w) { last_error_ = "minibatch update: no constant-W form (with W fixed a batch step is the full H step: use the engine without 'batchSize')"; return ST_INVALID; }
		return iterate_beta_minibatch(compute_error);
	}
	if (beta_dense_) return iterate_beta(compute_error, constant_w);
	if (prm_.divergence != 0) return constant_w ? ST_INVALID : iterate_kl(compute_error);
	if (fused_capable() && !constant_w) return iterate_mu64(compute_error);
	if (fused64_capable() && !constant_w) return iterate_fused64(compute_error);
	if (f32w_scale_ != nullptr && fused32w_capable() && !constant_w) return iterate_fused32w(compute_error);
	const int norm_parts = panel_update_parts(RP_, sizeof(T), (int)mpad_);
	h_partials_unneeded_ = !constant_w;              // (the fused iteration: H H^T rides the product where it can)
	const Status hs = h_step_impl(compute_error);
	h_partials_unneeded_ = false;
	if (hs != ST_OK) return hs;

	const bool ls_family = alg_ == ALG_ALS || alg_ == ALG_ACLS || alg_ == ALG_AHCLS;
	int error_terms_n = n_;   // length of the tr(H^T W^T V) term vector

	if (!(constant_w && !compute_error)) {
		const T* Fh = H_;
		bool hht_done = false;
		GramReduceArgs tri_ride = {nullptr, 0, nullptr, nullptr, 0};
		if (tri_) {
			// (riding in the product launch below; on error iterations the trace that reads H H^T then runs behind that launch)
			if (Status s = tri_prepare_h(HHt_, true, !constant_w ? &tri_ride : nullptr)) return s;
			hht_done = true;
		} else if (alg_ == ALG_NSNMF) {
			HIPX(smooth_panel(H_, Hs_, npad_));
			Fh = Hs_;
		}
		// GDCLS at padded rank 64 on the split-operand path (round 4): H H^T only feeds the W update, which runs AFTER the product against V -- so it is taken from
		// the split image of H by the passenger workgroups of that launch, as the multiplicative update does (gram_image.h): no reduction launch, no partial Gram
		// matrices out of the H update.  (The ALS family inverts H H^T beside the product and needs it before.)
		bool hht_rides = false;
		if constexpr (std::is_same<T, float>::value) {
			hht_rides = !constant_w && alg_ == ALG_GDCLS && x3_ && state_.hx3_valid && Fh == H_ && RP_ == 64 && !state_.gram_h_partials && passengers_ride(planWx_);
			if (!hht_rides && state_.gram_h_partials && Fh == H_) {
				// H H^T from the partial Gram matrices the H update left behind
				HIPX(launch_gram64_from_partials(gramH_part_, (int)(npad_ / 64), HHt_, nullptr, stream_));
				hht_done = true;
			}
		}
		if (!hht_done && !hht_rides) HIPX(launch_gram<T>(Fh, RP_, n_, gram_parts_, gram_part_, HHt_, stream_));
		if (compute_error && !hht_rides && tri_ride.tri_frags == nullptr) {
			const T* wtw = tri_ ? reinterpret_cast<const T*>(Gw_raw_) : G_;      // MU: W^T W of this iteration's H step (rank-256 bf16 path: the unscaled Gram matrix + tri_trace_scale())
			if (alg_ == ALG_NSNMF) {                            // unsmoothed W^T W (AlgorithmNonSmoothNMF.h:201-202)
				if (tri_) wtw = reinterpret_cast<const T*>(Gw_raw_);
				else if (fused_capable()) wtw = G_;             // (rank 64: the H step's passengers took it from the unsmoothed image, pending scale applied)
				else { HIPX(launch_gram<T>(Wt_, RP_, m_, gram_parts_, gram_part_, G2_, stream_)); wtw = G2_; }
			} else if (alg_ != ALG_MU && !hals_family(alg_)) wtw = G2_;      // LS algorithms: copy saved before the regulariser (MU, HALS: W^T W of this H step)
			HIPX(launch_trace_small<T>(HHt_, wtw, RP_, r_, psR_, stream_, tri_trace_scale()));
		}
		if (!constant_w) {
			const int S = planW_.splits;
			T offW = 0, diagW = 0;
			if (ls_family) {
				if (alg_ == ALG_ACLS) diagW = (T)prm_.lambdaW;
				else if (alg_ == ALG_AHCLS) {
					const T lam = (T)prm_.lambdaW, alpha = (T)prm_.alphaW;
					T beta = (T)((1 - alpha) * std::sqrt((double)(unsigned)r_) + alpha);
					beta *= beta;
					offW = -lam; diagW = lam * beta - lam;
				}
				// (the trace kernel above has read H H^T; the inverse destroys it) -- beside the product against V
				if (!inverse_rides(planW_)) { if (Status s = normal_inverse_fork(HHt_, offW, diagW)) return s; }
			}
			if (ls_family && inverse_rides(planW_)) {
				if constexpr (std::is_same<T, float>::value) {
					GramReduceArgs rg = {nullptr, 0, nullptr, nullptr, 0};
					rg.inv_a = HHt_; rg.inv_out = Qinv_; rg.inv_offdiag = offW; rg.inv_diag = diagW; rg.inv_r = r_;
					if (Status s = product_w(Fh, &rg, nullptr, x3_ && state_.hx3_valid && Fh == H_)) return s;
				}
			} else if (hht_rides) {
				if constexpr (std::is_same<T, float>::value) {
					GramReduceArgs rg = {nullptr, 0, HHt_, nullptr, 0};
					rg.image = Hx3_; rg.image_ks = ksW_;
					if (Status s = product_w(Fh, &rg, nullptr, true)) return s;
					// (the error term's trace reads the finished H H^T: behind the launch that made it)
					if (compute_error) HIPX(launch_trace_small<T>(HHt_, G2_, RP_, r_, psR_, stream_, tri_trace_scale()));
				}
			} else {
				if (Status s = product_w(Fh, tri_ride.tri_frags != nullptr ? &tri_ride : nullptr, nullptr, tri_ || (x3_ && state_.hx3_valid && Fh == H_))) return s;
				// (rank 256, H H^T rode in that launch: the error term's trace of H H^T against the unsmoothed W^T W of this iteration's H step, AlgorithmNonSmoothNMF.h:201-202)
				if (compute_error && tri_ride.tri_frags != nullptr) HIPX(launch_trace_small<T>(HHt_, reinterpret_cast<const T*>(Gw_raw_), RP_, r_, psR_, stream_, tri_trace_scale()));
			}
			if (hals_family(alg_)) {
				// coordinate sweep over every row of W against H H^T and the summed slabs of V H^T, then the column normalisation that keeps W H:
				// W(:, c) / d(c), H(c, :) d(c) -- applied to H at once, no pending scale.  With a penalty there is no normalisation: it keeps W H but not the
				// penalty terms, and without it one iteration is one pass of scikit-learn's coordinate descent (docs/HALS.md).
				state_.wx3_valid = false;
				state_.gram_w_ready = false;
				if (prm_.hals_penalised()) {
					if (Status s = family_step(true, Wt_, HHt_, S, (int)mpad_, m_, nullptr, nullptr, (T)prm_.l1W, (T)prm_.l2W)) return s;
				} else {
					if (Status s = family_step(true, Wt_, HHt_, S, (int)mpad_, m_, nullptr, sumsq_part_, T(0), T(0))) return s;
					HIPX(launch_hals_normalize<T>(Wt_, RP_, (int)mpad_, H_, (int)npad_, sumsq_part_, family_parts((int)mpad_), stream_));
				}
			} else if (!ls_family) {
				const bool gd_err = alg_ == ALG_GDCLS && compute_error;
				T* wpart = nullptr;
				if constexpr (std::is_same<T, float>::value) { if (gram_from_update()) wpart = gramW_part_; }
				state_.wx3_valid = false;
				if (tri_) {
					if (Status s = tri_update_w(slabs_, S, slab_stride_, state_.qx3_holds_hht ? nullptr : HHt_)) return s;
				} else {
					HIPX(launch_panel_update<T>(PANEL_MU, Wt_, slabs_, S, slab_stride_, HHt_, RP_, (int)mpad_, eps,
					                            nullptr, m_, sumsq_part_, gd_err ? numW_ : nullptr, stream_, wpart, nullptr, 0, qx3_));
					if (Status s = normalize_w(wpart != nullptr, norm_parts)) return s;
				}
				if (gd_err) {
					// tr(H^T W^T V) as diag((V H^T)^T W) with the UPDATED W (GDCLS :259-264)
					HIPX(launch_row_dot<T>(numW_, Wt_, RP_, r_, mpad_, psN_, stream_, rowdot_part_));
					error_terms_n = r_;
				}
			} else {
				if (!inverse_rides(planW_)) { if (Status s = normal_inverse_join()) return s; }
				if (compute_error) HIPX(hipMemcpyAsync(Wold_, Wt_, sizeof(T) * (size_t)RP_ * mpad_, hipMemcpyDeviceToDevice, stream_));
				T* wpart = nullptr;
				if constexpr (std::is_same<T, float>::value) { if (gram_from_update()) wpart = gramW_part_; }
				state_.wx3_valid = false;
				HIPX(launch_panel_update<T>(PANEL_LS, Wt_, slabs_, S, slab_stride_, Qinv_, RP_, (int)mpad_, eps,
				                            nullptr, m_, sumsq_part_, compute_error ? numW_ : nullptr, stream_, wpart, nullptr, 0, qx3_));
				if (compute_error) {
					// tr(W_old^T (V H^T)) over r diagonals (ALS :199-205)
					HIPX(launch_row_dot<T>(Wold_, numW_, RP_, r_, mpad_, psN_, stream_, rowdot_part_));
					error_terms_n = r_;
				}
				if (Status s = normalize_w(wpart != nullptr, norm_parts)) return s;
			}
		} else if (compute_error && alg_ != ALG_MU && alg_ != ALG_NSNMF && !hals_family(alg_)) {
			// constant basis vectors, LS algorithms: the reference's trace reads W against itself
			// (ALS/ACLS/AHCLS :199-205 with W never overwritten) or a stale buffer (GDCLS); here:
			// ALS family as the reference, GDCLS the product the formula names.
			if (ls_family) {
				HIPX(launch_row_dot<T>(Wt_, Wt_, RP_, r_, mpad_, psN_, stream_, rowdot_part_));
			} else {
				if (Status s = product_w(Fh)) return s;
				HIPX(launch_panel_update<T>(PANEL_SET, numW_, slabs_, planW_.splits, slab_stride_, HHt_, RP_, (int)mpad_, eps,
				                            nullptr, m_, nullptr, nullptr, stream_));
				HIPX(launch_row_dot<T>(numW_, Wt_, RP_, r_, mpad_, psN_, stream_, rowdot_part_));
			}
			error_terms_n = r_;
		}
	}
	if (compute_error) {
		if (Status s = fetch_error_terms(error_terms_n)) return s;
	}
	return ST_OK;
}

// Sparse mode: 0-based triplets (any order) -> CSR and CSC images on the device, the permutation
// between the two value orders, the sorted tr(V^T V) terms and sum(V).  Built on the host with stable
// counting sorts, once per upload (outside the iteration loop).  Duplicate coordinates stay separate
// entries (their contributions add; the densifying path adds them too, k_densify).
template <typename T>
Status Engine<T>::upload_triplets(std::vector<int>& rows, std::vector<int>& cols, std::vector<T>& vals) {
	const long nnz = (long)vals.size();
	if (nnz >= (1l << 31)) return ST_INVALID;
	std::vector<int> csr_ptr(m_ + 1, 0), csc_ptr(n_ + 1, 0), csr_idx(nnz), csc_idx(nnz), from_csr(nnz), order(nnz);
	std::vector<T> csr_val(nnz), csc_val(nnz);
	for (long p = 0; p < nnz; ++p) ++csr_ptr[rows[p] + 1];
	for (int i = 0; i < m_; ++i) csr_ptr[i + 1] += csr_ptr[i];
	{
		std::vector<int> fill(csr_ptr.begin(), csr_ptr.end() - 1);
		for (long p = 0; p < nnz; ++p) order[fill[rows[p]]++] = (int)p;       // stable by row
	}
	// inside a row: ascending column (stable), so that CSR / CSC / COO inputs of one matrix agree bit for bit
	// (a row whose columns already ascend -- what a CSR input usually is -- needs no sort: the check is one pass, the sort allocates and merges per row:
	//  ~0.2 s of config 3's 0.58 s set-up)
	for (int i = 0; i < m_; ++i) {
		const auto lo = order.begin() + csr_ptr[i], hi = order.begin() + csr_ptr[i + 1];
		auto by_col = [&](int x, int y) { return cols[x] < cols[y]; };
		if (!std::is_sorted(lo, hi, by_col)) std::stable_sort(lo, hi, by_col);
	}
	for (long q = 0; q < nnz; ++q) { csr_idx[q] = cols[order[q]]; csr_val[q] = vals[order[q]]; }
	for (long q = 0; q < nnz; ++q) ++csc_ptr[csr_idx[q] + 1];
	for (int j = 0; j < n_; ++j) csc_ptr[j + 1] += csc_ptr[j];
	{
		std::vector<int> fill(csc_ptr.begin(), csc_ptr.end() - 1);
		int row = 0;
		for (long q = 0; q < nnz; ++q) {
			while (q >= csr_ptr[row + 1]) ++row;
			const int dst = fill[csr_idx[q]]++;
			csc_idx[dst] = row; csc_val[dst] = csr_val[q]; from_csr[dst] = (int)q;
		}
	}
	// tr(V^T V) terms per column, accumulated in T like the trace kernel, and sum(V) for the KL divergence
	h_vtv_.assign(n_, T(0));
	sum_v_ = 0;
	for (int j = 0; j < n_; ++j) {
		T s = 0;
		for (int p = csc_ptr[j]; p < csc_ptr[j + 1]; ++p) { s += csc_val[p] * csc_val[p]; sum_v_ += (double)csc_val[p]; }
		h_vtv_[j] = s;
	}
	std::sort(h_vtv_.begin(), h_vtv_.end());

	buffers_.release(csr_ptr_, csr_idx_, csc_ptr_, csc_idx_, csc_from_csr_, csr_val_, csc_val_, q_, q2_);
	auto image = [&](auto** p, size_t bytes) { return buffers_.device(p, bytes, false, stream_); };
	const size_t ni = sizeof(int) * (size_t)std::max<long>(nnz, 1), nv = sizeof(T) * (size_t)std::max<long>(nnz, 1);
	HIPX(image(&csr_ptr_, sizeof(int) * (m_ + 1)));
	HIPX(image(&csc_ptr_, sizeof(int) * (n_ + 1)));
	// (the quotient buffers and the CSR -> CSC permutation only serve round 1's two-pass KL step, a measurement switch)
	const bool two_pass = tuning_env("NMFAMD_KL_TWO_PASS") != nullptr;
	HIPX(image(&csr_idx_, ni)); HIPX(image(&csc_idx_, ni));
	HIPX(image(&csr_val_, nv)); HIPX(image(&csc_val_, nv));
	if (two_pass) { HIPX(image(&csc_from_csr_, ni)); HIPX(image(&q_, nv)); HIPX(image(&q2_, nv)); }
	HIPX(hipMemcpyAsync(csr_ptr_, csr_ptr.data(), sizeof(int) * (m_ + 1), hipMemcpyHostToDevice, stream_));
	HIPX(hipMemcpyAsync(csc_ptr_, csc_ptr.data(), sizeof(int) * (n_ + 1), hipMemcpyHostToDevice, stream_));
	if (nnz > 0) {
		HIPX(hipMemcpyAsync(csr_idx_, csr_idx.data(), sizeof(int) * nnz, hipMemcpyHostToDevice, stream_));
		HIPX(hipMemcpyAsync(csc_idx_, csc_idx.data(), sizeof(int) * nnz, hipMemcpyHostToDevice, stream_));
		if (two_pass) HIPX(hipMemcpyAsync(csc_from_csr_, from_csr.data(), sizeof(int) * nnz, hipMemcpyHostToDevice, stream_));
		HIPX(hipMemcpyAsync(csr_val_, csr_val.data(), sizeof(T) * nnz, hipMemcpyHostToDevice, stream_));
		HIPX(hipMemcpyAsync(csc_val_, csc_val.data(), sizeof(T) * nnz, hipMemcpyHostToDevice, stream_));
	}
	nnz_ = nnz;
	if (Status st = setup_kl_blocks()) return st;
	HIPX(hipStreamSynchronize(stream_));
	nnz_ = nnz;
	return ST_OK;
}

// Blocked KL gather (kernels_sparse.hip, k_kl_fused): block counts from the shape and the device, per-(row, block) boundary pointers from the images on the device
template <typename T>
Status Engine<T>::setup_kl_blocks() {
	// KL divergence: cut the gathered factor into blocks that stay in an XCD's L2 (4 MiB; NMFAMD_KL_BLOCK_KB sets the block's bytes,
	// 0 = no blocking) when the whole factor does not: W step gathers rows of H by column index (range n), H step rows of Wt by row index
	// (range m).  A row's entries are sorted by that index, so its entries of block b are one range: only boundaries are needed.
	{
		buffers_.release(csr_bptr_, csc_bptr_, kl_part_, kl_tpart_);
		kl_blocks_w_ = kl_blocks_h_ = 1;
		const char* be = std::getenv("NMFAMD_KL_BLOCK_KB");
		const long block_bytes = be ? std::atol(be) * 1024 : 3584 * 1024;     // (measured at config 3: 2 MiB 1.73 ms / iteration, 3 MiB 1.62, 3.5 MiB 1.58, 4 MiB 1.57, 8 MiB 1.64; unblocked 2.14)
		if (prm_.divergence != 0 && block_bytes > 0) {
			const long rows_per_block = std::max<long>(64, block_bytes / ((long)RP_ * (long)sizeof(T)));
			auto cut = [&](long range) { return (range * RP_ * (long)sizeof(T) > 3l * 1024 * 1024) ? (int)std::min<long>(64, (range + rows_per_block - 1) / rows_per_block) : 1; };
			kl_blocks_w_ = cut(n_); kl_blocks_h_ = cut(m_);
			// five blocks or more: a multiple of eight, so that every XCD gathers from its OWN blocks (k_kl_fused) and fetches 1 / 8 of the factor per launch
			auto by_xcd = [](int b) { return b >= 5 ? ((b + 7) / 8) * 8 : b; };
			kl_blocks_w_ = by_xcd(kl_blocks_w_); kl_blocks_h_ = by_xcd(kl_blocks_h_);
			// every block writes its own partial numerator panel (and k_kl_update reads them all): keep that scratch within an eighth of the DEVICE's memory
			// (64 blocks of a 1M-row factor were 32 GB), halving the block count until it fits.  A function of the shape and of the device only
			// (round 4 asked the FREE memory, so the block count -- and with it the order of the partial sums, i.e. the bits -- depended on what else
			// occupied the device); if the allocation then fails, the unblocked gather runs (below).  geometry() reports the counts that ran.
			size_t free_b = 0, total_b = 0;
			if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); total_b = (size_t)1 << 62; }
			auto fit = [&](int b, long panel_rows) { while (b > 1 && (double)b * RP_ * (double)panel_rows * sizeof(T) > 0.125 * (double)total_b) b = b > 8 ? ((b / 2 + 7) / 8) * 8 : b / 2; return b; };
			kl_blocks_w_ = fit(kl_blocks_w_, mpad_); kl_blocks_h_ = fit(kl_blocks_h_, npad_);
			auto boundaries = [&](const int* ptr, const int* idx, int rows, long range, int blocks, int** dev) -> hipError_t {
				if (blocks <= 1) return hipSuccess;
				hipError_t e = buffers_.device(dev, sizeof(int) * (size_t)rows * (blocks + 1), false, stream_);
				if (e != hipSuccess) return e;
				return launch_sp_boundaries(ptr, idx, rows, range, blocks, *dev, stream_);      // (a row's indices ascend: block b of the row is one range)
			};
			HIPX(boundaries(csr_ptr_, csr_idx_, m_, n_, kl_blocks_w_, &csr_bptr_));
			HIPX(boundaries(csc_ptr_, csc_idx_, n_, m_, kl_blocks_h_, &csc_bptr_));
			const long pe = std::max<long>(kl_blocks_w_ > 1 ? (long)kl_blocks_w_ * RP_ * mpad_ : 0, kl_blocks_h_ > 1 ? (long)kl_blocks_h_ * RP_ * npad_ : 0);
			// (no room for the partial panels after all: the unblocked gather needs none)
			bool ok = pe == 0 || buffers_.device(&kl_part_, sizeof(T) * (size_t)pe, false, stream_) == hipSuccess;
			if (ok && kl_blocks_w_ > 1) ok = buffers_.device(&kl_tpart_, sizeof(T) * 2 * (size_t)kl_blocks_w_ * mpad_, false, stream_) == hipSuccess;
			if (!ok) {
				(void)hipGetLastError();
				buffers_.release(csr_bptr_, csc_bptr_, kl_part_, kl_tpart_);
				kl_blocks_w_ = kl_blocks_h_ = 1;
			}
		}
	}
	return ST_OK;
}

// KL-divergence multiplicative update (Lee & Seung, "Algorithms for Non-negative Matrix
// Factorization", NIPS 2001 -- the paper the reference's README cites; the reference itself only has
// the Frobenius form), in the skeleton of the reference's MU iteration: H step, W step, column
// normalisation of W, error terms referring to (W_{k-1}, H_k):
//   Q = V ./ (W H + eps) on the stored entries (SDDMM);  H .*= (W^T Q) ./ (colsum(W) + eps)
//   Q = V ./ (W H + eps) again;                          W .*= (Q H^T) ./ (rowsum(H) + eps);  normalise
template <typename T>
Status Engine<T>::iterate_kl(bool compute_error) {
	if (!sparse_ || nnz_ < 0) return ST_INVALID;
	const T eps = std::numeric_limits<T>::epsilon();
	const int norm_parts = (int)(mpad_ / 128);
	const bool two_pass = tuning_env("NMFAMD_KL_TWO_PASS") != nullptr;      // A/B: round 1's SDDMM + permute + SpMM per half-step
	// Round 6: W is left UNNORMALISED by its update, with the column scale d = 1 / sqrt(sum of squares) as a pending factor (kl_scale_, from the update's partial
	// sums, by the k_kl_sums launch that turns them into the column sums anyway): the pass over the 51 MB panel that normalised it (k_compact_partials +
	// k_normalize_panel_v2: 25 us at config 3) is gone.  W = Wt D enters the two half-steps through the row each fused kernel loads ONCE per output row
	// (a_scale), the H update's numerator is D (Wt^T Q), the W update reads its old rows as Wt D.  materialize_w() folds the scale in for everybody else.
	const bool keep_pending = !two_pass && std::getenv("NMFAMD_NO_FUSED_MU") == nullptr;
	if (!keep_pending) { if (Status st = materialize_w()) return st; }
	const T* dsc = state_.kl_scale_pending ? kl_scale_ : nullptr;
	// H step (no error terms here: they refer to the pair (W_{k-1}, H_k) of the second evaluation).  One pass over the CSC
	// image: quotient and numerator W^T Q together, one gathered row of W per stored entry (kernels_sparse.hip, k_kl_fused).
	record_begin();
	if (two_pass) {
		HIPX(launch_sddmm_quotient<T>(csr_ptr_, csr_idx_, csr_val_, Wt_, H_, RP_, eps, q_, (T*)nullptr, (T*)nullptr, m_, stream_));
		HIPX(launch_permute<T>(q_, csc_from_csr_, q2_, nnz_, stream_));
		HIPX(launch_spmm_rows<T>(csc_ptr_, csc_idx_, q2_, Wt_, RP_, slabs_, n_, (int)npad_, stream_));
	} else {
		if (kl_blocks_h_ > 1) HIPX(launch_kl_fused<T>(csc_bptr_, csc_idx_, csc_val_, H_, Wt_, RP_, eps, kl_part_, (T*)nullptr, (T*)nullptr, n_, (int)npad_, stream_, kl_blocks_h_, (long)RP_ * npad_, dsc));
		else HIPX(launch_kl_fused<T>(csc_ptr_, csc_idx_, csc_val_, H_, Wt_, RP_, eps, slabs_, (T*)nullptr, (T*)nullptr, n_, (int)npad_, stream_, 1, 0, dsc));
	}
	record_end();
	// the column sums of W: from the partial sums its last update left (round 4), or by a pass over the panel when W was set from outside
	if (!state_.kl_sw_ready) HIPX(launch_panel_rowsum<T>(Wt_, RP_, (int)mpad_, rowsum_part_, sW_, stream_));
	// ... and the update of H leaves the partial row sums of the NEW H (the W step's denominators) in rowsum_part_: one small launch instead of a pass over H
	if (!two_pass && kl_blocks_h_ > 1) HIPX(launch_kl_update<T>(H_, kl_part_, sW_, RP_, (int)npad_, eps, nullptr, stream_, kl_blocks_h_, (long)RP_ * npad_, rowsum_part_, dsc));
	else HIPX(launch_kl_update<T>(H_, slabs_, sW_, RP_, (int)npad_, eps, nullptr, stream_, 1, 0, rowsum_part_, dsc));
	HIPX(launch_kl_sums<T>(rowsum_part_, nullptr, (int)(npad_ / 128), RP_, sH_, stream_));
	// W step (the quotient is re-evaluated with the new H), over the CSR image; per-row error terms on error iterations only
	record_begin(1);
	if (two_pass) {
		HIPX(launch_sddmm_quotient<T>(csr_ptr_, csr_idx_, csr_val_, Wt_, H_, RP_, eps, q_, compute_error ? t_vwh_ : (T*)nullptr, compute_error ? t_kl_ : (T*)nullptr, m_, stream_));
		HIPX(launch_spmm_rows<T>(csr_ptr_, csr_idx_, q_, H_, RP_, slabs_, m_, (int)mpad_, stream_));
	} else {
		if (kl_blocks_w_ > 1) {
			HIPX(launch_kl_fused<T>(csr_bptr_, csr_idx_, csr_val_, Wt_, H_, RP_, eps, kl_part_, compute_error ? kl_tpart_ : (T*)nullptr,
			                        compute_error ? kl_tpart_ + (long)kl_blocks_w_ * mpad_ : (T*)nullptr, m_, (int)mpad_, stream_, kl_blocks_w_, (long)RP_ * mpad_, dsc));
			if (compute_error) {
				// the blocks' parts of the per-row error terms, block order
				HIPX(launch_reduce_partials<T>(kl_tpart_, kl_blocks_w_, mpad_, t_vwh_, m_, stream_));
				HIPX(launch_reduce_partials<T>(kl_tpart_ + (long)kl_blocks_w_ * mpad_, kl_blocks_w_, mpad_, t_kl_, m_, stream_));
			}
		} else
		HIPX(launch_kl_fused<T>(csr_ptr_, csr_idx_, csr_val_, Wt_, H_, RP_, eps, slabs_, compute_error ? t_vwh_ : (T*)nullptr, compute_error ? t_kl_ : (T*)nullptr,
		                        m_, (int)mpad_, stream_, 1, 0, dsc));
	}
	record_end();
	if (compute_error) {
		// Frobenius error by the reference's trace formula with (W_{k-1}, H_k); KL divergence next to it
		HIPX(launch_gram<T>(Wt_, RP_, m_, gram_parts_, gram_part_, G_, stream_));
		HIPX(launch_gram<T>(H_, RP_, n_, gram_parts_, gram_part_, HHt_, stream_));
		HIPX(launch_trace_small<T>(HHt_, G_, RP_, r_, psR_, stream_, nullptr, dsc));      // (G_ is the Gram matrix of the panel as it lies: D G D = W^T W of the normalised W)
		// the terms travel stream-ordered into pinned memory; the sorted host summation (100 000 per-row terms at config 3:
		// milliseconds) runs when the error is read -- the iteration loop does not wait for the GPU here
		finalize_error(false);
		T* p = pin_kl_;
		HIPX(hipMemcpyAsync(p, t_vwh_, sizeof(T) * m_, hipMemcpyDeviceToHost, stream_));
		HIPX(hipMemcpyAsync(p + m_, t_kl_, sizeof(T) * m_, hipMemcpyDeviceToHost, stream_));
		HIPX(hipMemcpyAsync(p + 2 * (size_t)m_, sW_, sizeof(T) * RP_, hipMemcpyDeviceToHost, stream_));
		HIPX(hipMemcpyAsync(p + 2 * (size_t)m_ + RP_, sH_, sizeof(T) * RP_, hipMemcpyDeviceToHost, stream_));
		HIPX(hipMemcpyAsync(p + 2 * (size_t)m_ + 2 * RP_, psR_, sizeof(T) * r_, hipMemcpyDeviceToHost, stream_));
		HIPX(hipEventRecord(err_event_, stream_));
		kl_pending_ = true;
	}
	if (!two_pass && kl_blocks_w_ > 1) HIPX(launch_kl_update<T>(Wt_, kl_part_, sH_, RP_, (int)mpad_, eps, sumsq_part_, stream_, kl_blocks_w_, (long)RP_ * mpad_, rowsum_part_, dsc));
	else HIPX(launch_kl_update<T>(Wt_, slabs_, sH_, RP_, (int)mpad_, eps, sumsq_part_, stream_, 1, 0, rowsum_part_, dsc));
	// colsum of the NORMALISED W = (sum of the new column) / (its norm), both from the update's per-workgroup partials (norm_parts = mpad / 128 of each); and the
	// pending scale itself
	HIPX(launch_kl_sums<T>(rowsum_part_, sumsq_part_, norm_parts, RP_, sW_, stream_, keep_pending ? kl_scale_ : nullptr));
	state_.kl_sw_ready = true;
	if (keep_pending) state_.kl_scale_pending = true;
	else HIPX(launch_normalize_panel<T>(Wt_, RP_, (int)mpad_, sumsq_part_, norm_parts, stream_));
	return ST_OK;
}

// Missing-value NMF (docs/MISSING.md): the multiplicative update with W H restricted to the stored entries Omega in both denominators, in the skeleton of
// the reference's MU iteration -- H step, W step with the new H, column normalisation of W (H is not rescaled), error of the pair (W_{k-1}, H_k):
//   H .*= (W^T V_Omega) ./ (W^T (W H)_Omega + eps)     one fused launch over the CSC image (kernels_masked.hip), H written in place
//   W .*= (V_Omega H^T) ./ ((W H)_Omega H^T + eps)     one fused launch over the CSR image, W written in place, + per-row residual terms on error iterations
//   normalise W                                          from the W launch's per-workgroup sums of squares (launch_normalize_panel)
// The residual terms sum_p (v_p - W_{k-1}(i_p, :) . H_k(:, j_p))^2 per row come from the W launch's own dot products (it reads the old row of W) -- or, under
// constant W, from the residual-only form of that launch; they travel to pinned memory and are summed in double by finalize_error().
template <typename T>
Status Engine<T>::iterate_masked(bool compute_error, bool constant_w) {
	if (!sparse_ || nnz_ <= 0) { last_error_ = "missing values: no stored entry has been uploaded"; return ST_INVALID; }
	if (cd_.solver == 1) return iterate_masked_cd(compute_error, constant_w);
	const T eps = std::numeric_limits<T>::epsilon();
	record_begin();
	HIPX(launch_masked_half_step<T>(csc_ptr_, csc_idx_, csc_val_, H_, Wt_, RP_, eps, true, (T*)nullptr, (T*)nullptr, n_, stream_));
	record_end();
	if (!constant_w || compute_error) {
		record_begin(1);
		if (!constant_w) HIPX(launch_masked_half_step<T>(csr_ptr_, csr_idx_, csr_val_, Wt_, H_, RP_, eps, true, compute_error ? t_vwh_ : (T*)nullptr, msq_part_, m_, stream_));
		else HIPX(launch_masked_half_step<T>(csr_ptr_, csr_idx_, csr_val_, Wt_, H_, RP_, eps, false, t_vwh_, (T*)nullptr, m_, stream_));
		record_end();
	}
	if (compute_error) {
		finalize_error(false);      // (the pinned buffer is about to be reused; an older copy is long complete)
		HIPX(hipMemcpyAsync(pin_kl_, t_vwh_, sizeof(T) * m_, hipMemcpyDeviceToHost, stream_));
		HIPX(hipEventRecord(err_event_, stream_));
		masked_pending_ = true;
	}
	if (!constant_w) HIPX(launch_normalize_panel<T>(Wt_, RP_, (int)mpad_, msq_part_, masked_norm_parts(m_), stream_));
	return ST_OK;
}

// Missing-value NMF by coordinate descent (docs/MISSING.md, "Coordinate descent"; set_missing_solver): HALS on sum_Omega (v - W H)^2 with scikit-learn's penalties,
// every row of a factor against its own Gram matrix over its observed entries -- one launch per half-step (kernels_masked_cd.hip):
//   H step over the CSC image (sweeps_h, l1H, l2H), W step with the new H over the CSR image (sweeps_w, l1W, l2W); no normalisation
// The error is iterate_masked's: the residual terms of the pair (W_{k-1}, H_k), from the terms-only form of the multiplicative launch between the two half-steps.
// As there, nothing derived from a factor outlives a launch: PanelState has no flag of this iteration.
template <typename T>
Status Engine<T>::iterate_masked_cd(bool compute_error, bool constant_w) {
	record_begin();
	HIPX(launch_masked_cd_half_step<T>(csc_ptr_, csc_idx_, csc_val_, H_, Wt_, RP_, r_, n_, cd_.sweeps_h, (T)cd_.l1H, (T)cd_.l2H, (T*)nullptr, (T*)nullptr, stream_));
	record_end();
	if (compute_error) {
		HIPX(launch_masked_half_step<T>(csr_ptr_, csr_idx_, csr_val_, Wt_, H_, RP_, std::numeric_limits<T>::epsilon(), false, t_vwh_, (T*)nullptr, m_, stream_));
		finalize_error(false);      // (the pinned buffer is about to be reused; an older copy is long complete)
		HIPX(hipMemcpyAsync(pin_kl_, t_vwh_, sizeof(T) * m_, hipMemcpyDeviceToHost, stream_));
		HIPX(hipEventRecord(err_event_, stream_));
		masked_pending_ = true;
	}
	if (!constant_w) {
		record_begin(1);
		HIPX(launch_masked_cd_half_step<T>(csr_ptr_, csr_idx_, csr_val_, Wt_, H_, RP_, r_, m_, cd_.sweeps_w, (T)cd_.l1W, (T)cd_.l2W, (T*)nullptr, (T*)nullptr, stream_));
		record_end();
	}
	return ST_OK;
}

// Missing-value NMF under the beta-divergence (docs/MISSING.md, "Beta-divergence"): the weighted update of docs/DIVERGENCE.md at 0 / 1 weights with both sums over the
// stored entries, in iterate_masked's skeleton -- one fused launch per half-step (kernels_masked_beta.hip) that maps every stored entry's p = wh_p + eps, accumulates
// numerator and denominator and applies the quotient, the penalties and gamma to its own row in place:
//   H step over the CSC image (l1H, l2H), W step with the new H over the CSR image (l1W, l2W), + the two per-row error terms of (W_{k-1}, H_k) on error iterations
//   normalisation as the weighted update: none with a penalty; beta = 1 the columns of W only (launch_normalize_panel); any other beta the compensated form
//   (launch_hals_normalize: W D^-1, D H), both from the W launch's per-workgroup sums of squares
// Under constant W the H step runs alone and an error iteration takes its terms from the terms-only form of the W-side launch.  The terms travel to pinned memory
// like the dense divergence engines' and are summed in double by finalize_error().  Nothing derived from a factor outlives a launch, so PanelState has no flag of
// this iteration: an upload or a factor from outside goes through its transitions as on every engine and finds nothing of ours to clear.
template <typename T>
Status Engine<T>::iterate_masked_beta(bool compute_error, bool constant_w) {
	if (!sparse_ || nnz_ <= 0) { last_error_ = "missing values: no stored entry has been uploaded"; return ST_INVALID; }
	const T eps = std::numeric_limits<T>::epsilon();
	const bool penalised = prm_.hals_penalised();
	const T l1W = (T)prm_.l1W, l1H = (T)prm_.l1H, l2W = (T)prm_.l2W, l2H = (T)prm_.l2H;
	record_begin();
	HIPX(launch_masked_beta_half_step<T>(csc_ptr_, csc_idx_, csc_val_, H_, Wt_, RP_, eps, mbeta_, l1H, l2H, true, (T*)nullptr, (T*)nullptr, (T*)nullptr, n_, stream_));
	record_end();
	if (!constant_w || compute_error) {
		T* tf = compute_error ? t_vwh_ : (T*)nullptr;
		T* td = compute_error ? t_kl_ : (T*)nullptr;
		record_begin(1);
		HIPX(launch_masked_beta_half_step<T>(csr_ptr_, csr_idx_, csr_val_, Wt_, H_, RP_, eps, mbeta_, l1W, l2W, !constant_w, tf, td,
		                                     constant_w || penalised ? (T*)nullptr : msq_part_, m_, stream_));
		record_end();
	}
	if (compute_error) {
		finalize_error(false);      // (the pinned buffer is about to be reused; an older copy is long complete)
		HIPX(hipMemcpyAsync(pin_kl_, t_vwh_, sizeof(T) * m_, hipMemcpyDeviceToHost, stream_));
		HIPX(hipMemcpyAsync(pin_kl_ + m_, t_kl_, sizeof(T) * m_, hipMemcpyDeviceToHost, stream_));
		HIPX(hipEventRecord(err_event_, stream_));
		beta_pending_ = true;
	}
	if (constant_w || penalised) return ST_OK;
	if (mbeta_ == 1) HIPX(launch_normalize_panel<T>(Wt_, RP_, (int)mpad_, msq_part_, masked_norm_parts(m_), stream_));
	else HIPX(launch_hals_normalize<T>(Wt_, RP_, (int)mpad_, H_, (int)npad_, msq_part_, masked_norm_parts(m_), stream_));
	return ST_OK;
}

// Dense beta-divergence update (docs/DIVERGENCE.md): generalised KL (beta = 1), Itakura-Saito (beta = 0) or any other beta on the dense images, one fused launch and
// one update launch per half-step (kernels_beta.hip), in the skeleton of the other multiplicative iterations -- H step, W step with the new H, normalisation, error of
// the pair (W_{k-1}, H_k) from the W launch's own evaluation of P:
//   beta = 1:  H .*= (W^T (V ./ P)) ./ (colsum(W) + eps);  W .*= ((V ./ P) H^T) ./ (rowsum(H) + eps);  normalise the columns of W (H is not rescaled): iterate_kl's iteration
//   beta = 0:  H .*= sqrt((W^T (V ./ P^2)) ./ (W^T (1 ./ P) + eps));  W likewise;  W(:, k) /= d_k, H(k, :) *= d_k with d_k = ||W(:, k)|| (W H unchanged)
//   general:   H .*= ((W^T (V .* P^(beta - 2))) ./ (W^T P^(beta - 1) + eps))^gamma;  W likewise;  the compensated normalisation of beta = 0
// With a penalty (set_hals_penalties) the denominators carry + l1 + l2 A (l1H, l2H in the H step, l1W, l2W in the W step) and there is no normalisation, HALS's rule:
// W D^-1 . D H keeps W H but not the penalty terms.  The KL denominators sW_ / sH_ are then the column sums of the panels as they are.
// Under constant W the H step runs alone; an error iteration then takes its terms from the terms-only form of the W-side launch.
// Weighted (kernels_beta_weighted.hip): the same skeleton with the images of the weights beside those of V; every denominator is a product (at beta = 1 it is
// sum_k w(k, o) B(k, :), not colsum(B): no sW_ / sH_, no launch_kl_sums), the normalisation is that of the unweighted engine of the same beta.
// Mixed precision (kernels_beta_bf16.hip): the two fused launches take bf16 operands; the update launches, the sums and the normalisation are the fp32 engine's.
// (the mixed-precision launch exists in fp32 only; allocate() refuses the switch on a double engine, so the other overload is never reached)
static hipError_t beta_fused_mixed(const float* X, long ldx, const float* A, const float* B, int RP, double beta, bool update, bool terms, float eps, const BetaPlan& plan,
                                   float* num_part, float* den_part, long part_stride, float* tf_part, float* td_part, long t_stride, int out_pad, int out_valid,
                                   int red_valid, hipStream_t stream) {
	return launch_beta_fused_bf16(X, ldx, A, B, RP, beta, update, terms, eps, plan, num_part, den_part, part_stride, tf_part, td_part, t_stride, out_pad, out_valid, red_valid, stream);
}
static hipError_t beta_fused_mixed(const double*, long, const double*, const double*, int, double, bool, bool, double, const BetaPlan&, double*, double*, long, double*, double*,
                                   long, int, int, int, hipStream_t) {
	return hipErrorInvalidValue;
}

template <typename T>
Status Engine<T>::iterate_beta(bool compute_error, bool constant_w) {
	if (!beta_uploaded_) { last_error_ = weighted_ ? "weighted NMF: no V and weights have been uploaded" : "dense divergence update: no V has been uploaded"; return ST_INVALID; }
	const T eps = std::numeric_limits<T>::epsilon();
	const double beta = beta_;
	const bool kl = beta == 1 && !weighted_, penalised = prm_.hals_penalised();      // (kl: the vector denominators of the unweighted beta = 1)
	const T l1W = (T)prm_.l1W, l1H = (T)prm_.l1H, l2W = (T)prm_.l2W, l2H = (T)prm_.l2H;
	const int partsH = (int)(npad_ / 128), partsW = (int)(mpad_ / 128);
	// H step: X = the column-major image (row j of X = column j of V)
	if (kl && !state_.kl_sw_ready) { HIPX(launch_panel_rowsum<T>(Wt_, RP_, (int)mpad_, rowsum_part_, sW_, stream_)); state_.kl_sw_ready = true; }
	record_begin();
	if (weighted_)
		HIPX(launch_beta_fused_weighted<T>(V_, Om_, mpad_, H_, Wt_, RP_, beta, true, false, eps, betaH_, slabs_, beta_den_, slab_stride_, (T*)nullptr, (T*)nullptr, 0,
		                                   (int)npad_, n_, m_, stream_));
	else if (mixed_)
		HIPX(beta_fused_mixed(V_, mpad_, H_, Wt_, RP_, beta, true, false, eps, betaH_, slabs_, beta_den_, slab_stride_, (T*)nullptr, (T*)nullptr, 0, (int)npad_, n_, m_, stream_));
	else
		HIPX(launch_beta_fused<T>(V_, mpad_, H_, Wt_, RP_, beta, true, false, eps, betaH_, slabs_, beta_den_, slab_stride_, (T*)nullptr, (T*)nullptr, 0,
		                          (int)npad_, n_, m_, stream_));
	record_end();
	HIPX(launch_beta_update<T>(H_, slabs_, beta_den_, slab_stride_, betaH_.slabs, sW_, RP_, r_, (int)npad_, n_, eps, beta, l1H, l2H, true, (T*)nullptr,
	                           kl ? rowsum_part_ : (T*)nullptr, (const T*)nullptr, (const T*)nullptr, 0, (T*)nullptr, (T*)nullptr, stream_, weighted_));
	if (kl) HIPX(launch_kl_sums<T>(rowsum_part_, nullptr, partsH, RP_, sH_, stream_));
	if (constant_w && !compute_error) return ST_OK;
	// W step (or, under constant W, its terms-only form): X = the transposed image
	T* tf = compute_error ? beta_tpart_ : (T*)nullptr;
	T* td = compute_error ? beta_tpart_ + (long)BETA_MAX_SLABS * mpad_ : (T*)nullptr;
	record_begin(1);
	if (weighted_)
		HIPX(launch_beta_fused_weighted<T>(Vt_, Omt_, npad_, Wt_, H_, RP_, beta, !constant_w, compute_error, eps, betaW_, slabs_, beta_den_, slab_stride_, tf, td, mpad_,
		                                   (int)mpad_, m_, n_, stream_));
	else if (mixed_)
		HIPX(beta_fused_mixed(Vt_, npad_, Wt_, H_, RP_, beta, !constant_w, compute_error, eps, betaW_, slabs_, beta_den_, slab_stride_, tf, td, mpad_, (int)mpad_, m_, n_, stream_));
	else
		HIPX(launch_beta_fused<T>(Vt_, npad_, Wt_, H_, RP_, beta, !constant_w, compute_error, eps, betaW_, slabs_, beta_den_, slab_stride_, tf, td, mpad_,
		                          (int)mpad_, m_, n_, stream_));
	record_end();
	HIPX(launch_beta_update<T>(Wt_, slabs_, beta_den_, slab_stride_, betaW_.slabs, sH_, RP_, r_, (int)mpad_, m_, eps, beta, l1W, l2W, !constant_w, sumsq_part_,
	                           kl ? rowsum_part_ : (T*)nullptr, tf, td, mpad_, compute_error ? t_vwh_ : (T*)nullptr, compute_error ? t_kl_ : (T*)nullptr, stream_,
	                           weighted_));
	if (compute_error) {
		finalize_error(false);      // (the pinned buffer is about to be reused; an older copy is long complete)
		HIPX(hipMemcpyAsync(pin_kl_, t_vwh_, sizeof(T) * m_, hipMemcpyDeviceToHost, stream_));
		HIPX(hipMemcpyAsync(pin_kl_ + m_, t_kl_, sizeof(T) * m_, hipMemcpyDeviceToHost, stream_));
		HIPX(hipEventRecord(err_event_, stream_));
		beta_pending_ = true;
	}
	if (constant_w) return ST_OK;
	if (kl) {
		// as iterate_kl: the column sums of the NORMALISED W from the update's partials, then the normalisation itself; penalised: the sums of W as it is
		HIPX(launch_kl_sums<T>(rowsum_part_, penalised ? (const T*)nullptr : sumsq_part_, partsW, RP_, sW_, stream_));
		state_.kl_sw_ready = true;
		if (!penalised) HIPX(launch_normalize_panel<T>(Wt_, RP_, (int)mpad_, sumsq_part_, partsW, stream_));
	} else if (!penalised) {
		// (the weighted beta = 1: the columns of W normalised, H not rescaled, as above -- without the column sums nobody reads)
		if (beta == 1) HIPX(launch_normalize_panel<T>(Wt_, RP_, (int)mpad_, sumsq_part_, partsW, stream_));
		else HIPX(launch_hals_normalize<T>(Wt_, RP_, (int)mpad_, H_, (int)npad_, sumsq_part_, partsW, stream_));
	}
	return ST_OK;
}

// The minibatch (online) form (docs/DIVERGENCE.md, "Minibatch update"; scikit-learn's MiniBatchNMF): one iteration is one pass over the column ranges [0, b),
// [b, 2 b), ... in order.  A batch J at column offset c0 takes the two fused launches of iterate_beta on offset pointers -- the H side on V_ + c0 mpad and
// H_ + c0 RP with the batch as its output range, the W side on Vt_ + c0 (leading dimension npad) with the batch as its reduction range -- and after each the
// fine-grained update launch of kernels_beta_online.hip: the ordinary update on H_J, the online one (A <- rho A + W^(1/gamma) num, B <- rho B + den,
// W <- (A / B)^gamma) on W.  Values below eps become 0 in H_J at beta < 1 and in W at beta <= 1.  No normalisation (a rescale of W would have to rescale A, B and
// every column of H); at beta = 1 the denominators are the column sums of W as it is and the row sums of H over J.  There is no single P in a pass, so the errors
// of an error iteration are those of (W_k, H_k) AFTER the pass, from one terms-only launch over the whole of V.
template <typename T>
Status Engine<T>::iterate_beta_minibatch(bool compute_error) {
	if (!beta_uploaded_) { last_error_ = "dense divergence update: no V has been uploaded"; return ST_INVALID; }
	const T eps = std::numeric_limits<T>::epsilon();
	const double beta = beta_;
	const bool kl = beta == 1;
	const T l1W = (T)prm_.l1W, l1H = (T)prm_.l1H, l2W = (T)prm_.l2W, l2H = (T)prm_.l2H;
	const int partsW = (int)(mpad_ / BETA_ROWS_PER_WG);
	if (state_.online_stale) { HIPX(launch_beta_online_reset<T>(Wt_, online_A_, online_B_, (long)RP_ * mpad_, stream_)); state_.online_stale = false; }
	if (kl && !state_.kl_sw_ready) { HIPX(launch_panel_rowsum<T>(Wt_, RP_, (int)mpad_, rowsum_part_, sW_, stream_)); state_.kl_sw_ready = true; }
	for (long c0 = 0; c0 < n_; c0 += batch_) {
		const int blen = (int)std::min<long>(batch_, n_ - c0), bpad = (int)pad128(blen);
		const bool full = blen == batch_;
		const BetaPlan& pH = full ? betaHb_ : betaHr_;
		const BetaPlan& pW = full ? betaWb_ : betaWr_;
		T* HJ = H_ + c0 * RP_;
		// H step on the batch's columns: its rows of the column-major image are the output range
		record_begin();
		if (mixed_)
			HIPX(beta_fused_mixed(V_ + c0 * mpad_, mpad_, HJ, Wt_, RP_, beta, true, false, eps, pH, slabs_, beta_den_, slab_stride_, (T*)nullptr, (T*)nullptr, 0, bpad, blen, m_, stream_));
		else
			HIPX(launch_beta_fused<T>(V_ + c0 * mpad_, mpad_, HJ, Wt_, RP_, beta, true, false, eps, pH, slabs_, beta_den_, slab_stride_, (T*)nullptr, (T*)nullptr, 0, bpad, blen, m_, stream_));
		record_end();
		HIPX(launch_beta_update_rows<T>(HJ, (T*)nullptr, (T*)nullptr, slabs_, beta_den_, slab_stride_, pH.slabs, sW_, RP_, r_, bpad, blen, eps, beta, l1H, l2H, false, T(0),
		                                beta < 1, kl ? rowsum_part_ : (T*)nullptr, stream_));
		if (kl) HIPX(launch_kl_sums<T>(rowsum_part_, nullptr, bpad / BETA_ROWS_PER_WG, RP_, sH_, stream_));
		// W step with the new H_J: the batch's columns of the transposed image are the reduction range
		record_begin(1);
		if (mixed_)
			HIPX(beta_fused_mixed(Vt_ + c0, npad_, Wt_, HJ, RP_, beta, true, false, eps, pW, slabs_, beta_den_, slab_stride_, (T*)nullptr, (T*)nullptr, 0, (int)mpad_, m_, blen, stream_));
		else
			HIPX(launch_beta_fused<T>(Vt_ + c0, npad_, Wt_, HJ, RP_, beta, true, false, eps, pW, slabs_, beta_den_, slab_stride_, (T*)nullptr, (T*)nullptr, 0, (int)mpad_, m_, blen, stream_));
		record_end();
		HIPX(launch_beta_update_rows<T>(Wt_, online_A_, online_B_, slabs_, beta_den_, slab_stride_, pW.slabs, sH_, RP_, r_, (int)mpad_, m_, eps, beta, l1W, l2W, true, (T)rho_,
		                                beta <= 1, kl ? rowsum_part_ : (T*)nullptr, stream_));
		if (kl) HIPX(launch_kl_sums<T>(rowsum_part_, nullptr, partsW, RP_, sW_, stream_));
	}
	if (compute_error) {
		// the terms-only form of the W-side launch over the whole of V, with the full-shape plan
		T* tf = beta_tpart_;
		T* td = beta_tpart_ + (long)BETA_MAX_SLABS * mpad_;
		if (mixed_)
			HIPX(beta_fused_mixed(Vt_, npad_, Wt_, H_, RP_, beta, false, true, eps, betaW_, slabs_, beta_den_, slab_stride_, tf, td, mpad_, (int)mpad_, m_, n_, stream_));
		else
			HIPX(launch_beta_fused<T>(Vt_, npad_, Wt_, H_, RP_, beta, false, true, eps, betaW_, slabs_, beta_den_, slab_stride_, tf, td, mpad_, (int)mpad_, m_, n_, stream_));
		HIPX(launch_beta_update<T>(Wt_, slabs_, beta_den_, slab_stride_, betaW_.slabs, sH_, RP_, r_, (int)mpad_, m_, eps, beta, l1W, l2W, false, (T*)nullptr, (T*)nullptr, tf, td,
		                           mpad_, t_vwh_, t_kl_, stream_, false));
		finalize_error(false);      // (the pinned buffer is about to be reused; an older copy is long complete)
		HIPX(hipMemcpyAsync(pin_kl_, t_vwh_, sizeof(T) * m_, hipMemcpyDeviceToHost, stream_));
		HIPX(hipMemcpyAsync(pin_kl_ + m_, t_kl_, sizeof(T) * m_, hipMemcpyDeviceToHost, stream_));
		HIPX(hipEventRecord(err_event_, stream_));
		beta_pending_ = true;
	}
	return ST_OK;
}

template <typename T>
Status Engine<T>::beta_refuses(const char* what) {
	static thread_local char text[160];
	std::snprintf(text, sizeof(text), "dense divergence update: %s -- no three-phase / sharded form (single GPU)", what);
	last_error_ = text;
	return ST_INVALID;
}

template <typename T>
Status Engine<T>::masked_refuses(const char* what) {
	static thread_local char text[160];
	std::snprintf(text, sizeof(text), "missing values: %s -- the masked update has no three-phase / sharded form", what);
	last_error_ = text;
	return ST_INVALID;
}

// ---- the KL update in the three phases of the column-sharded form ---------------------------------------------------------------------
// Rank g holds the CSC / CSR images of V(:, J_g), H(:, J_g) and a replica of W.  The H half-step is local.  The W half-step's numerator
// sum_j Q(i, j) H(:, j) and the row sums of H are sums over ALL columns: every rank contributes its columns' part through the exchange buffer
// (layout: Engine::exchange_count), as do the per-row error terms; the W update and its normalisation then run replicated.
template <typename T>
Status Engine<T>::kl_h_step() {
	if (!sparse_ || nnz_ < 0) return ST_INVALID;
	if (Status st = materialize_w()) return st;      // (the sharded form works on the normalised panel)
	const T eps = std::numeric_limits<T>::epsilon();
	record_begin();
	if (kl_blocks_h_ > 1) HIPX(launch_kl_fused<T>(csc_bptr_, csc_idx_, csc_val_, H_, Wt_, RP_, eps, kl_part_, (T*)nullptr, (T*)nullptr, n_, (int)npad_, stream_, kl_blocks_h_, (long)RP_ * npad_));
	else HIPX(launch_kl_fused<T>(csc_ptr_, csc_idx_, csc_val_, H_, Wt_, RP_, eps, slabs_, (T*)nullptr, (T*)nullptr, n_, (int)npad_, stream_));
	record_end();
	HIPX(launch_panel_rowsum<T>(Wt_, RP_, (int)mpad_, rowsum_part_, sW_, stream_));
	if (kl_blocks_h_ > 1) HIPX(launch_kl_update<T>(H_, kl_part_, sW_, RP_, (int)npad_, eps, nullptr, stream_, kl_blocks_h_, (long)RP_ * npad_));
	else HIPX(launch_kl_update<T>(H_, slabs_, sW_, RP_, (int)npad_, eps, nullptr, stream_));
	return ST_OK;
}

template <typename T>
Status Engine<T>::kl_w_products(T* exchange, bool compute_error) {
	if (!sparse_ || nnz_ < 0) return ST_INVALID;
	const T eps = std::numeric_limits<T>::epsilon();
	T* num = exchange;
	T* hht = num + (long)RP_ * mpad_;
	T* sh = hht + (long)RP_ * RP_;
	T* tv = sh + RP_;
	T* tk = tv + mpad_;
	record_begin(1);
	if (kl_blocks_w_ > 1) {
		HIPX(launch_kl_fused<T>(csr_bptr_, csr_idx_, csr_val_, Wt_, H_, RP_, eps, kl_part_, compute_error ? kl_tpart_ : (T*)nullptr,
		                        compute_error ? kl_tpart_ + (long)kl_blocks_w_ * mpad_ : (T*)nullptr, m_, (int)mpad_, stream_, kl_blocks_w_, (long)RP_ * mpad_));
		// the blocks' partial numerator panels (and error terms), block order, before the sum over ranks
		HIPX(launch_reduce_partials<T>(kl_part_, kl_blocks_w_, (long)RP_ * mpad_, num, (long)RP_ * mpad_, stream_));
		if (compute_error) {
			HIPX(launch_reduce_partials<T>(kl_tpart_, kl_blocks_w_, mpad_, tv, m_, stream_));
			HIPX(launch_reduce_partials<T>(kl_tpart_ + (long)kl_blocks_w_ * mpad_, kl_blocks_w_, mpad_, tk, m_, stream_));
		}
	} else {
		HIPX(launch_kl_fused<T>(csr_ptr_, csr_idx_, csr_val_, Wt_, H_, RP_, eps, num, compute_error ? tv : (T*)nullptr, compute_error ? tk : (T*)nullptr,
		                        m_, (int)mpad_, stream_));
	}
	record_end();
	HIPX(launch_panel_rowsum<T>(H_, RP_, (int)npad_, rowsum_part_, sh, stream_));
	if (compute_error) HIPX(launch_gram<T>(H_, RP_, n_, gram_parts_, gram_part_, hht, stream_));
	else {
		// the regions nobody reads on this iteration still ride the all-reduce: keep them finite (left alone they grow by the rank count per iteration)
		HIPX(hipMemsetAsync(hht, 0, sizeof(T) * (size_t)RP_ * RP_, stream_));
		HIPX(hipMemsetAsync(tv, 0, sizeof(T) * 2 * (size_t)mpad_, stream_));
	}
	return ST_OK;
}

template <typename T>
Status Engine<T>::kl_w_finish(const T* exchange, bool compute_error) {
	if (!sparse_ || nnz_ < 0) return ST_INVALID;
	// the error terms in the exchange buffer were (or were not) produced by w_products() under the flag h_step() latched: a caller asking for the
	// other thing here would read terms that are not there
	if (compute_error != kl_err_iter_) { last_error_ = "kl: w_finish(compute_error) differs from the h_step(compute_error) of the same iteration"; return ST_INVALID; }
	state_.kl_sw_ready = false;
	const T eps = std::numeric_limits<T>::epsilon();
	const int norm_parts = (int)(mpad_ / 128);
	const T* num = exchange;
	const T* hht = num + (long)RP_ * mpad_;
	const T* sh = hht + (long)RP_ * RP_;
	const T* tv = sh + RP_;
	const T* tk = tv + mpad_;
	if (compute_error) {
		// as iterate_kl: Frobenius error by the trace formula with (W_{k-1}, H_k), KL divergence next to it -- from the reduced terms
		HIPX(launch_gram<T>(Wt_, RP_, m_, gram_parts_, gram_part_, G_, stream_));
		HIPX(launch_trace_small<T>(hht, G_, RP_, r_, psR_, stream_));
		finalize_error(false);
		T* p = pin_kl_;
		HIPX(hipMemcpyAsync(p, tv, sizeof(T) * m_, hipMemcpyDeviceToHost, stream_));
		HIPX(hipMemcpyAsync(p + m_, tk, sizeof(T) * m_, hipMemcpyDeviceToHost, stream_));
		HIPX(hipMemcpyAsync(p + 2 * (size_t)m_, sW_, sizeof(T) * RP_, hipMemcpyDeviceToHost, stream_));
		HIPX(hipMemcpyAsync(p + 2 * (size_t)m_ + RP_, sh, sizeof(T) * RP_, hipMemcpyDeviceToHost, stream_));
		HIPX(hipMemcpyAsync(p + 2 * (size_t)m_ + 2 * RP_, psR_, sizeof(T) * r_, hipMemcpyDeviceToHost, stream_));
		HIPX(hipEventRecord(err_event_, stream_));
		kl_pending_ = true;
	}
	HIPX(launch_kl_update<T>(Wt_, num, sh, RP_, (int)mpad_, eps, sumsq_part_, stream_));
	HIPX(launch_normalize_panel<T>(Wt_, RP_, (int)mpad_, sumsq_part_, norm_parts, stream_));
	return ST_OK;
}

template <typename T>
Status Engine<T>::debug_read(int which, T* out, long count) {
	const T* src = nullptr; long avail = 0;
	if (count < 0) return ST_INVALID;
	switch (which) {
	case 0: if (Status st = materialize_w()) return st; src = Wt_; avail = (long)RP_ * mpad_; break;
	case 1: src = H_; avail = (long)RP_ * npad_; break;
	case 2: src = G_; avail = (long)RP_ * RP_; break;
	case 3: src = HHt_; avail = (long)RP_ * RP_; break;
	case 4: src = slabs_; avail = slab_stride_ * std::max(planH_.splits, planW_.splits); break;
	case 5: src = Qinv_; avail = (long)RP_ * RP_; break;
	case 8: case 9: case 10: case 11: {
		// rank-256 intermediates, read as fp32 words (diagnosis of runs that share a device: tools/shared_device_diff.py):
		// 8 = W^T W as the last Gram reduction left it, 9 = the staged column sums of squares, 10 / 11 = the bf16 fragments of W / of H
		if (!tri_ || sizeof(T) != 4) return ST_INVALID;
		const void* p = which == 8 ? (const void*)Gw_raw_ : which == 9 ? (const void*)colsq_ : which == 10 ? (const void*)Wtb_ : (const void*)Hb_;
		avail = which == 8 ? (long)RP_ * RP_ : which == 9 ? (long)RP_ : which == 10 ? (long)RP_ * mpad_ / 2 : (long)RP_ * npad_ / 2;
		if (!p || count > avail) return ST_INVALID;
		HIPX(hipMemcpyAsync(out, p, sizeof(T) * count, hipMemcpyDeviceToHost, stream_));
		HIPX(hipStreamSynchronize(stream_));
		return ST_OK;
	}
	case 12: case 13: case 14: case 15: case 16: case 17: case 18: case 19: {
		// the sparse images (tests/test_gpu_sparse_setup.py compares the device-built ones with the host-built ones): 12 / 13 = CSR / CSC values; 14 .. 19 = CSR
		// pointers, CSR column indices, CSC pointers, CSC row indices, blocked CSR / CSC boundary pointers as raw 32-bit words (fp32 engines: count = number of ints)
		if (!sparse_) return ST_INVALID;
		if (which >= 14 && sizeof(T) != 4) return ST_INVALID;
		const long bw = kl_blocks_w_ > 1 ? (long)m_ * (kl_blocks_w_ + 1) : 0, bh = kl_blocks_h_ > 1 ? (long)n_ * (kl_blocks_h_ + 1) : 0;
		const void* ptrs[] = {csr_val_, csc_val_, csr_ptr_, csr_idx_, csc_ptr_, csc_idx_, csr_bptr_, csc_bptr_};
		const long lens[] = {nnz_, nnz_, (long)m_ + 1, nnz_, (long)n_ + 1, nnz_, bw, bh};
		const void* sp = ptrs[which - 12];
		if (sp == nullptr || count > lens[which - 12]) return ST_INVALID;
		HIPX(hipMemcpyAsync(out, sp, sizeof(T) * count, hipMemcpyDeviceToHost, stream_));
		HIPX(hipStreamSynchronize(stream_));
		return ST_OK;
	}
	case 20: case 21: case 22: {
		// the rank-64 fused iteration's operands (tests/test_gpu_mu64_update.py ties na.op_mu64_update to what the engine launches): 20 = the pending column scale
		// of W the last product's passengers left (64 values), 21 = the Wt panel as it lies -- unnormalised while that scale is pending (0 folds the scale in first),
		// 22 = the gram_k_slices unscaled K slices of W^T W the H update adds and scales (engines whose plan cuts the Gram passengers' K range)
		if (sizeof(T) != 4 || !fused_capable() || scale_ == nullptr || (which == 22 && (Gpart_ == nullptr || gram_ksplit_ < 2))) return ST_INVALID;
		const void* p = which == 20 ? (const void*)scale_ : which == 21 ? (const void*)Wt_ : (const void*)Gpart_;
		if (count > (which == 20 ? 64l : which == 21 ? (long)RP_ * mpad_ : 4096l * gram_ksplit_)) return ST_INVALID;
		HIPX(hipMemcpyAsync(out, p, sizeof(T) * count, hipMemcpyDeviceToHost, stream_));
		HIPX(hipStreamSynchronize(stream_));
		return ST_OK;
	}
	case 6: case 7: {
		if (sparse_ || bf16_ || (one_image_ && which == 7)) return ST_INVALID;   // no fp32 dense image in sparse / bf16 mode; no V^T image
		// V (ld mpad_) / Vt (ld npad_) as column-major images; the MFMA path keeps them x-tiled
		const bool vt = which == 7;
		const T* img = vt ? Vt_ : V_;
		avail = mpad_ * npad_;
		if (count > avail) return ST_INVALID;
		if (!tiled_) { src = img; break; }
		T* tmp = nullptr;
		hipError_t e = buffers_.device(&tmp, sizeof(T) * (size_t)avail, true, stream_);
		if (e == hipSuccess) e = vt ? launch_tile<T>(img, npad_, n_, m_, tmp, strideVt_, planH_.th, true, stream_) : launch_tile<T>(img, mpad_, m_, n_, tmp, strideV_, img_th_, true, stream_);
		if (e == hipSuccess) e = hipMemcpyAsync(out, tmp, sizeof(T) * count, hipMemcpyDeviceToHost, stream_);
		if (e == hipSuccess) e = hipStreamSynchronize(stream_);
		buffers_.release(tmp);
		return e == hipSuccess ? ST_OK : hip_fail(e, "debug_read(V)");
	}
	default: return ST_INVALID;
	}
	if (count > avail) return ST_INVALID;
	HIPX(hipMemcpyAsync(out, src, sizeof(T) * count, hipMemcpyDeviceToHost, stream_));
	HIPX(hipStreamSynchronize(stream_));
	return ST_OK;
}

template class Engine<float>;
template class Engine<double>;

} // namespace nmfamd
