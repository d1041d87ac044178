// amd_api.cpp -- the extern "C" entry points of include/nmfgpu_amd.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <memory>
#include <new>
#include <type_traits>
#include <vector>

#include "../../include/nmfgpu_amd.h"
#include "comm.h"
#include "engine.h"
#include "tuning.h"
#include "host_init.h"
#include "sharded.h"
#include "panel_form.h"

using namespace nmfamd;

struct nmfamd_engine {
	int elem_bytes;
	std::unique_ptr<Engine<float>> f;
	std::unique_ptr<Engine<double>> d;
};

struct nmfamd_comm {
	std::unique_ptr<Comm> c;
};

struct nmfamd_local_group {
	std::shared_ptr<LocalGroup> g;
};

struct nmfamd_sharded {
	int elem_bytes;
	std::unique_ptr<ShardedRank<float>> f;
	std::unique_ptr<ShardedRank<double>> d;
};

namespace {
// why the last nmfamd_engine_create on this thread failed (the engine that knew is gone): nmfamd_engine_last_error(NULL)
thread_local std::string g_create_error;

// nmfamd_params or one of its sized successors (NULL: the defaults) -> the engine's parameters; false for a struct shorter than nmfamd_params
bool sized_params(const void* params_sized, unsigned long params_size, AlgorithmParams* out) {
	if (params_sized == nullptr) return true;
	if (params_size < sizeof(nmfamd_params)) return false;
	nmfamd_params_v7 v7;
	std::memset(&v7, 0, sizeof(v7));
	std::memcpy(&v7, params_sized, params_size < sizeof(v7) ? (size_t)params_size : sizeof(v7));
	const nmfamd_params_v6& v6 = v7.v6;
	const nmfamd_params_v5& v5 = v6.v5;
	const nmfamd_params_v4& v4 = v5.v4;
	const nmfamd_params_v3& v3 = v4.v3;
	const nmfamd_params_v2& v2 = v3.v2;
	const nmfamd_params& b = v2.base;
	AlgorithmParams& p = *out;
	p.lambda = b.lambda; p.lambdaW = b.lambdaW; p.lambdaH = b.lambdaH; p.alphaW = b.alphaW; p.alphaH = b.alphaH; p.theta = b.theta; p.divergence = b.divergence; p.sparse_compute = b.sparse_compute; p.precision = b.precision; p.missing_values = b.missing_values; p.dense_compute = v2.dense_compute; p.beta_value = v3.beta; p.weighted = v4.weighted; p.mixed_precision = v5.mixed_precision; p.batch_size = v6.batch_size; p.forget_factor = v6.forget_factor;
	p.missing_divergence = v7.missing_divergence; p.missing_beta = v7.missing_beta;
	return true;
}

// what nmfamd_engine_geometry reports of an engine, created or only planned
template <typename T>
void fill_geometry(const Engine<T>& g, nmfamd_geometry* out) {
	out->m = g.m(); out->n = g.n(); out->r = g.r(); out->padded_rank = g.rp();
	out->padded_m = g.mpad(); out->padded_n = g.npad();
	out->slabs_h = g.slabs_h(); out->slabs_w = g.slabs_w(); out->exchange_count = g.exchange_count();
	out->product_kernel = g.product_kernel(); out->resident_images = g.resident_images(); out->one_pass = g.one_pass_state();
	out->kl_blocks_w = g.kl_blocks(true); out->kl_blocks_h = g.kl_blocks(false); out->gram_k_slices = g.gram_k_slices(); out->w_col_split = g.w_col_split() ? 1 : 0;
	out->sparse_setup = g.sparse_mode() ? (g.sparse_setup_on_device() ? 1 : 0) : -1;
	out->fused_launches = g.fused_launches(); out->gram_ride_slices_h = g.gram_ride_slices(false); out->gram_ride_slices_w = g.gram_ride_slices(true);
}

// check_parameters() + plan() of an engine that allocates nothing: no HIP call
template <typename T>
Status plan_geometry(int m, int n, int r, int algorithm, const AlgorithmParams& p, int row_blocks, const DeviceFacts& device, nmfamd_geometry* out) {
	Engine<T> e(m, n, r, algorithm, p);
	e.set_row_blocks(row_blocks);
	Status st = e.check_parameters();
	if (st == ST_OK) st = e.plan(device);
	if (st == ST_OK) fill_geometry(e, out); else g_create_error = e.last_error();
	return st;
}

template <typename Fn32, typename Fn64>
int dispatch(nmfamd_engine* e, Fn32 f32, Fn64 f64) {
	if (!e) return NMFAMD_INVALID_ARGUMENT;
	return e->elem_bytes == 4 ? (int)f32(*e->f) : (int)f64(*e->d);
}
}

namespace {
struct DevBuf {
	void* p = nullptr;
	~DevBuf() { if (p) (void)hipFree(p); }
	hipError_t alloc(size_t bytes) { hipError_t e = hipMalloc(&p, bytes ? bytes : 16); if (e == hipSuccess) e = hipMemset(p, 0, bytes ? bytes : 16); return e; }
};

// the r x r inverse as the passenger workgroup of a product launch (nmfamd_op_inverse_ex_f32, routes 2 and 3): device buffers, GramReduceArgs::inv_*
struct InversePassenger { const float* a; float* out; float offdiag, diag; int r; };

// (passenger: a launcher that refuses it returns NMFAMD_INVALID_ARGUMENT with OUT untouched)
template <typename T>
int op_factor_product(const T* A, long lda, int X, int Y, const T* F, long ldf, int r, T* OUT, long ldo, bool use_valu, int* out_slabs, const InversePassenger* passenger = nullptr) {
	if (!A || !F || !OUT || X <= 0 || Y <= 0 || r <= 0 || lda < X || ldf < r || ldo < r) return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	const int RP = padded_rank(r, sizeof(T));
	int dev = 0; hipDeviceProp_t prop;
	if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return NMFAMD_HIP_ERROR;
	FactorProductPlan plan = std::is_same<T, double>::value ? plan_factor_product_f64(X, Y, RP, prop.multiProcessorCount)
	                                                         : plan_factor_product(X, Y, RP, prop.multiProcessorCount);
	if (RP == 64 && r <= 32) plan.nb = std::is_same<T, float>::value ? 1 : 2;      // as the engine does: 32 panel columns for small ranks (fp64 counts 16-column tiles)
	const long Xp = pad128(std::max<long>(X, (long)plan.xtiles * plan.th)), Yp = pad128(Y);
	const bool mfma = !use_valu;
	const int S = mfma ? plan.splits : 1;
	DevBuf dA, dF, dS, dO;
	const long slab_stride = (long)RP * Xp;
	if (dA.alloc(sizeof(T) * Xp * Yp) != hipSuccess || dF.alloc(sizeof(T) * RP * Yp) != hipSuccess ||
	    dS.alloc(sizeof(T) * slab_stride * S) != hipSuccess || dO.alloc(sizeof(T) * slab_stride) != hipSuccess) return NMFAMD_NO_DEVICE_MEMORY;
	if (hipMemcpy2D(dA.p, Xp * sizeof(T), A, lda * sizeof(T), X * sizeof(T), Y, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (hipMemcpy2D(dF.p, RP * sizeof(T), F, ldf * sizeof(T), r * sizeof(T), Y, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	hipError_t e;
	if constexpr (std::is_same<T, float>::value) {
		if (mfma) {
			DevBuf dT;   // x-tiled image of A for the MFMA kernel
			if (dT.alloc(sizeof(T) * Xp * Yp) != hipSuccess) return NMFAMD_NO_DEVICE_MEMORY;
			GramReduceArgs rg = {nullptr, 0, nullptr, nullptr, 0};
			if (passenger) { rg.inv_a = passenger->a; rg.inv_out = passenger->out; rg.inv_offdiag = passenger->offdiag; rg.inv_diag = passenger->diag; rg.inv_r = passenger->r; }
			e = launch_tile<float>((const float*)dA.p, Xp, X, Y, (float*)dT.p, plan.th * Yp, plan.th, false, nullptr);
			if (e == hipSuccess) e = launch_factor_product_f32(plan, (const float*)dT.p, plan.th * Yp, (const float*)dF.p, RP, (float*)dS.p, slab_stride, nullptr, passenger ? &rg : nullptr);
			if (e == hipSuccess) e = hipDeviceSynchronize();
		}
		else e = launch_factor_product_valu<T>((const T*)dA.p, Xp, (int)Xp, Y, (const T*)dF.p, RP, (T*)dS.p, nullptr);
	} else {
		if (mfma) {
			DevBuf dT;   // x-tiled image of A for the fp64 MFMA kernel
			if (dT.alloc(sizeof(T) * Xp * Yp) != hipSuccess) return NMFAMD_NO_DEVICE_MEMORY;
			e = hipMemset(dT.p, 0, sizeof(T) * Xp * Yp);
			if (e == hipSuccess) e = launch_tile<double>((const double*)dA.p, Xp, X, Y, (double*)dT.p, plan.th * Yp, plan.th, false, nullptr);
			if (e == hipSuccess) e = launch_factor_product_f64(plan, (const double*)dT.p, plan.th * Yp, (const double*)dF.p, RP, (double*)dS.p, slab_stride, nullptr);
			if (e == hipSuccess) e = hipDeviceSynchronize();
		}
		else e = launch_factor_product_valu<T>((const T*)dA.p, Xp, (int)Xp, Y, (const T*)dF.p, RP, (T*)dS.p, nullptr);
	}
	if (passenger && (!mfma || !std::is_same<T, float>::value || e == hipErrorInvalidValue)) return NMFAMD_INVALID_ARGUMENT;
	if (e != hipSuccess) return NMFAMD_HIP_ERROR;
	if (launch_reduce_slabs<T>((const T*)dS.p, S, slab_stride, (T*)dO.p, slab_stride, nullptr) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (hipMemcpy2D(OUT, ldo * sizeof(T), dO.p, RP * sizeof(T), r * sizeof(T), X, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (hipDeviceSynchronize() != hipSuccess) return NMFAMD_HIP_ERROR;
	if (out_slabs) *out_slabs = S;
	return NMFAMD_OK;
}
}

namespace {
template <typename T>
int host_kmeans(const T* data, long ld, int m, int n, T* clusters, long ldc, int k, unsigned* membership, unsigned seed,
                unsigned maxiter, double threshold, unsigned* iterations) {
	if (!data || !clusters || m <= 0 || n <= 0 || k <= 0 || ld < m || ldc < m) return nmfamd::ST_INVALID;
	nmfgpu::KMeansDescription<T> d{};
	d.inputMatrix.rows = (unsigned)m; d.inputMatrix.columns = (unsigned)n; d.inputMatrix.format = nmfgpu::StorageFormat::Dense;
	d.inputMatrix.dense.values = const_cast<T*>(data); d.inputMatrix.dense.leadingDimension = (unsigned)ld;
	d.outputMatrixClusters.rows = (unsigned)m; d.outputMatrixClusters.columns = (unsigned)k; d.outputMatrixClusters.format = nmfgpu::StorageFormat::Dense;
	d.outputMatrixClusters.dense.values = clusters; d.outputMatrixClusters.dense.leadingDimension = (unsigned)ldc;
	d.outputMemberships = membership; d.numClusters = (unsigned)k; d.numIterations = maxiter; d.seed = seed; d.thresholdValue = threshold;
	nmfgpu::KMeansSummary s{};
	if (nmfgpu::hostinit::compute_kmeans<T>(d, &s) != nmfgpu::ResultType::Success) return nmfamd::ST_INVALID;
	if (iterations) *iterations = s.iterations;
	return nmfamd::ST_OK;
}

template <typename T>
int host_init(const T* V, long ldv, int m, int n, int r, int method, unsigned seed, T* W, T* H) {
	if (!V || !W || m <= 0 || n <= 0 || r <= 0 || ldv < m) return nmfamd::ST_INVALID;
	nmfgpu::NmfDescription<T> d{};
	d.inputMatrix.rows = (unsigned)m; d.inputMatrix.columns = (unsigned)n; d.inputMatrix.format = nmfgpu::StorageFormat::Dense;
	d.inputMatrix.dense.values = const_cast<T*>(V); d.inputMatrix.dense.leadingDimension = (unsigned)ldv;
	d.features = (unsigned)r; d.seed = seed;
	// method 100 + v: the SVD-based start (NNDSVD, v = 0 plain / 1 "a" / 2 "ar"), which nmfgpu::compute selects with Parameter{"nndsvd", v}
	nmfgpu::Parameter svd{"nndsvd", (double)(method - 100)};
	if (method >= 100 && method <= 102) {
		if (r > std::min(m, n)) return nmfamd::ST_INVALID;
		d.initMethod = nmfgpu::NmfInitializationMethod::AllRandomValues; d.parameters = &svd; d.numParameters = 1;
		return nmfgpu::hostinit::initialize<T>(d, W, H) ? nmfamd::ST_OK : nmfamd::ST_INVALID;
	}
	d.initMethod = (nmfgpu::NmfInitializationMethod)method;
	if ((d.initMethod != nmfgpu::NmfInitializationMethod::MeanColumns) && r >= n) return nmfamd::ST_INVALID;
	return nmfgpu::hostinit::initialize<T>(d, W, H) ? nmfamd::ST_OK : nmfamd::ST_INVALID;
}
} // namespace

extern "C" {

int nmfamd_device_count(void) {
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
	return n;
}

const char* nmfamd_build_info(void) {
	return "nmfgpu-amd 0.2.3 (gfx950 HIP kernels: fp32 MFMA factor product, fused panel updates; no vendor BLAS)";
}

const char* nmfamd_engine_last_error(const nmfamd_engine* e) {
	if (!e) return g_create_error.c_str();
	return e->elem_bytes == 4 ? e->f->last_error() : e->d->last_error();
}

int nmfamd_engine_create(int m, int n, int r, int algorithm, const nmfamd_params* params, int elem_bytes, void* stream, nmfamd_engine** out) {
	return nmfamd_engine_create_blocks(m, n, r, algorithm, params, elem_bytes, stream, 1, out);
}

int nmfamd_engine_create_blocks(int m, int n, int r, int algorithm, const nmfamd_params* params, int elem_bytes, void* stream, int row_blocks, nmfamd_engine** out) {
	return nmfamd_engine_create_v2(m, n, r, algorithm, params, params ? sizeof(nmfamd_params) : 0, elem_bytes, stream, row_blocks, out);
}

int nmfamd_engine_create_v2(int m, int n, int r, int algorithm, const void* params_sized, unsigned long params_size, int elem_bytes, void* stream, int row_blocks, nmfamd_engine** out) {
	AlgorithmParams p;
	if (!sized_params(params_sized, params_size, &p)) return NMFAMD_INVALID_ARGUMENT;
	if (!out || (elem_bytes != 4 && elem_bytes != 8) || row_blocks < 1 || row_blocks > 64) return NMFAMD_INVALID_ARGUMENT;
	*out = nullptr;
	g_create_error.clear();
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	nmfamd_engine* e = new (std::nothrow) nmfamd_engine();
	if (!e) return NMFAMD_NO_HOST_MEMORY;
	e->elem_bytes = elem_bytes;
	Status st;
	try {
		if (elem_bytes == 4) { e->f.reset(new Engine<float>(m, n, r, algorithm, p)); e->f->set_stream((hipStream_t)stream); e->f->set_row_blocks(row_blocks); st = e->f->allocate(); }
		else { e->d.reset(new Engine<double>(m, n, r, algorithm, p)); e->d->set_stream((hipStream_t)stream); e->d->set_row_blocks(row_blocks); st = e->d->allocate(); }
	} catch (const std::bad_alloc&) { delete e; return NMFAMD_NO_HOST_MEMORY; }
	if (st != ST_OK) { g_create_error = nmfamd_engine_last_error(e); delete e; return (int)st; }
	*out = e;
	return NMFAMD_OK;
}

void nmfamd_engine_destroy(nmfamd_engine* e) { delete e; }

int nmfamd_comm_rccl_available(void) { return rccl_available() ? 1 : 0; }

int nmfamd_comm_unique_id(void* out_128_bytes) { return (int)rccl_unique_id(out_128_bytes); }

int nmfamd_comm_create_rccl(const void* id_128_bytes, int world, int rank, nmfamd_comm** out) {
	if (!out) return NMFAMD_INVALID_ARGUMENT;
	*out = nullptr;
	nmfamd_comm* c = new (std::nothrow) nmfamd_comm();
	if (!c) return NMFAMD_NO_HOST_MEMORY;
	Status st = rccl_comm_create(id_128_bytes, world, rank, &c->c);
	if (st != ST_OK) { delete c; return (int)st; }
	*out = c;
	return NMFAMD_OK;
}

void nmfamd_comm_destroy(nmfamd_comm* c) { delete c; }

int nmfamd_local_group_create(int world, nmfamd_local_group** out) {
	if (!out) return NMFAMD_INVALID_ARGUMENT;
	*out = nullptr;
	std::shared_ptr<LocalGroup> g = local_group_create(world);
	if (!g) return NMFAMD_INVALID_ARGUMENT;
	nmfamd_local_group* h = new (std::nothrow) nmfamd_local_group();
	if (!h) return NMFAMD_NO_HOST_MEMORY;
	h->g = std::move(g);
	*out = h;
	return NMFAMD_OK;
}

void nmfamd_local_group_destroy(nmfamd_local_group* g) { delete g; }
void nmfamd_local_group_abort(nmfamd_local_group* g) { if (g && g->g) local_group_abort(*g->g); }

int nmfamd_comm_create_local(nmfamd_local_group* g, int rank, nmfamd_comm** out) {
	if (!g || !g->g || !out) return NMFAMD_INVALID_ARGUMENT;
	*out = nullptr;
	nmfamd_comm* c = new (std::nothrow) nmfamd_comm();
	if (!c) { local_group_abort(*g->g); return NMFAMD_NO_HOST_MEMORY; }
	Status st = local_comm_create(g->g, rank, &c->c);
	if (st != ST_OK) { delete c; return (int)st; }
	*out = c;
	return NMFAMD_OK;
}

const char* nmfamd_local_group_last_error(nmfamd_local_group* g) {
	static thread_local std::string text;
	text = (g && g->g) ? local_group_failure(*g->g) : std::string();
	return text.c_str();
}

const char* nmfamd_local_group_selftest(nmfamd_local_group* g) {
	static thread_local std::string text;
	text = (g && g->g) ? local_group_selftest(*g->g) : std::string();
	return text.c_str();
}

const char* nmfamd_comm_transport(const nmfamd_comm* c) { return (c && c->c) ? c->c->transport() : ""; }

int nmfamd_sharded_create(nmfamd_engine* e, nmfamd_comm* c, int mode, long rows, long total_columns, nmfamd_sharded** out) {
	if (!e || !c || !c->c || !out) return NMFAMD_INVALID_ARGUMENT;
	*out = nullptr;
	nmfamd_sharded* s = new (std::nothrow) nmfamd_sharded();
	if (!s) return NMFAMD_NO_HOST_MEMORY;
	s->elem_bytes = e->elem_bytes;
	Status st;
	if (e->elem_bytes == 4) { s->f.reset(new ShardedRank<float>(e->f.get(), c->c.get(), mode, rows, total_columns)); st = s->f->prepare(); }
	else { s->d.reset(new ShardedRank<double>(e->d.get(), c->c.get(), mode, rows, total_columns)); st = s->d->prepare(); }
	if (st != ST_OK) { delete s; return (int)st; }
	*out = s;
	return NMFAMD_OK;
}

void nmfamd_sharded_destroy(nmfamd_sharded* s) { delete s; }

int nmfamd_sharded_iterate(nmfamd_sharded* s, int count, int first_iteration, int error_every, int last_iteration) {
	if (!s) return NMFAMD_INVALID_ARGUMENT;
	return (int)(s->elem_bytes == 4 ? s->f->run(count, first_iteration, error_every, last_iteration) : s->d->run(count, first_iteration, error_every, last_iteration));
}

int nmfamd_sharded_gather_w(nmfamd_sharded* s) {
	if (!s) return NMFAMD_INVALID_ARGUMENT;
	return (int)(s->elem_bytes == 4 ? s->f->gather_w_rows() : s->d->gather_w_rows());
}

double nmfamd_sharded_frobenius(nmfamd_sharded* s) { return !s ? 0.0 : (s->elem_bytes == 4 ? s->f->frobenius() : s->d->frobenius()); }
double nmfamd_sharded_rmsd(nmfamd_sharded* s) { return !s ? 0.0 : (s->elem_bytes == 4 ? s->f->rmsd() : s->d->rmsd()); }
const char* nmfamd_sharded_last_error(const nmfamd_sharded* s) { return !s ? "" : (s->elem_bytes == 4 ? s->f->last_error() : s->d->last_error()); }

int nmfamd_engine_upload_dense(nmfamd_engine* e, const void* V, long ld) {
	return dispatch(e, [&](Engine<float>& g) { return g.upload_dense((const float*)V, ld); },
	                   [&](Engine<double>& g) { return g.upload_dense((const double*)V, ld); });
}

int nmfamd_engine_upload_dense_weighted(nmfamd_engine* e, const void* V, long ldv, const void* Omega, long ldo) {
	return dispatch(e, [&](Engine<float>& g) { return g.upload_dense_weighted((const float*)V, ldv, (const float*)Omega, ldo); },
	                   [&](Engine<double>& g) { return g.upload_dense_weighted((const double*)V, ldv, (const double*)Omega, ldo); });
}

int nmfamd_engine_upload_sparse(nmfamd_engine* e, int format, const void* values, const int* a, const int* b, long nnz, int base) {
	return dispatch(e, [&](Engine<float>& g) { return g.upload_sparse(format, (const float*)values, a, b, nnz, base); },
	                   [&](Engine<double>& g) { return g.upload_sparse(format, (const double*)values, a, b, nnz, base); });
}

int nmfamd_engine_set_factors(nmfamd_engine* e, const void* W, long ldw, const void* H, long ldh) {
	return dispatch(e, [&](Engine<float>& g) { return g.set_factors((const float*)W, ldw, (const float*)H, ldh); },
	                   [&](Engine<double>& g) { return g.set_factors((const double*)W, ldw, (const double*)H, ldh); });
}

int nmfamd_engine_get_factors(nmfamd_engine* e, void* W, long ldw, void* H, long ldh) {
	return dispatch(e, [&](Engine<float>& g) { return g.get_factors((float*)W, ldw, (float*)H, ldh); },
	                   [&](Engine<double>& g) { return g.get_factors((double*)W, ldw, (double*)H, ldh); });
}

int nmfamd_engine_upload_dense_device(nmfamd_engine* e, const void* V, long ld, int layout) {
	return dispatch(e, [&](Engine<float>& g) { return g.upload_dense_device((const float*)V, ld, layout); },
	                   [&](Engine<double>& g) { return g.upload_dense_device((const double*)V, ld, layout); });
}

int nmfamd_engine_upload_sparse_device(nmfamd_engine* e, int format, const void* values, const int* a, const int* b, long nnz, int base) {
	return dispatch(e, [&](Engine<float>& g) { return g.upload_sparse_from_device(format, (const float*)values, a, b, nnz, base); },
	                   [&](Engine<double>& g) { return g.upload_sparse_from_device(format, (const double*)values, a, b, nnz, base); });
}

int nmfamd_engine_upload_dense_device_stored(nmfamd_engine* e, const void* V, long ld, int layout) {
	return dispatch(e, [&](Engine<float>& g) { return g.upload_dense_device_stored((const float*)V, ld, layout); },
	                   [&](Engine<double>& g) { return g.upload_dense_device_stored((const double*)V, ld, layout); });
}

int nmfamd_engine_upload_dense_weighted_device(nmfamd_engine* e, const void* V, long ldv, int layout_v, const void* Omega, long ldo, int layout_o) {
	return dispatch(e, [&](Engine<float>& g) { return g.upload_dense_weighted_device((const float*)V, ldv, layout_v, (const float*)Omega, ldo, layout_o); },
	                   [&](Engine<double>& g) { return g.upload_dense_weighted_device((const double*)V, ldv, layout_v, (const double*)Omega, ldo, layout_o); });
}

int nmfamd_engine_set_factors_device(nmfamd_engine* e, const void* W, long ldw, int layout_w, const void* H, long ldh, int layout_h) {
	return dispatch(e, [&](Engine<float>& g) { return g.set_factors_device((const float*)W, ldw, layout_w, (const float*)H, ldh, layout_h); },
	                   [&](Engine<double>& g) { return g.set_factors_device((const double*)W, ldw, layout_w, (const double*)H, ldh, layout_h); });
}

int nmfamd_engine_get_factors_device(nmfamd_engine* e, void* W, long ldw, int layout_w, void* H, long ldh, int layout_h) {
	return dispatch(e, [&](Engine<float>& g) { return g.get_factors_device((float*)W, ldw, layout_w, (float*)H, ldh, layout_h); },
	                   [&](Engine<double>& g) { return g.get_factors_device((double*)W, ldw, layout_w, (double*)H, ldh, layout_h); });
}

int nmfamd_engine_predict(nmfamd_engine* e, const int* rows, const int* cols, long nnz, int base, void* out) {
	if (!out) return NMFAMD_INVALID_ARGUMENT;
	return dispatch(e, [&](Engine<float>& g) { return g.predict_entries(rows, cols, nullptr, nnz, base, 0.0, (float*)out, nullptr, false); },
	                   [&](Engine<double>& g) { return g.predict_entries(rows, cols, nullptr, nnz, base, 0.0, (double*)out, nullptr, false); });
}

int nmfamd_engine_score(nmfamd_engine* e, const int* rows, const int* cols, const void* values, long nnz, int base, double beta, void* out, double sums[4]) {
	if (!values || !sums) return NMFAMD_INVALID_ARGUMENT;
	return dispatch(e, [&](Engine<float>& g) { return g.predict_entries(rows, cols, (const float*)values, nnz, base, beta, (float*)out, sums, false); },
	                   [&](Engine<double>& g) { return g.predict_entries(rows, cols, (const double*)values, nnz, base, beta, (double*)out, sums, false); });
}

int nmfamd_engine_predict_device(nmfamd_engine* e, const int* rows, const int* cols, long nnz, int base, void* out) {
	if (!out) return NMFAMD_INVALID_ARGUMENT;
	return dispatch(e, [&](Engine<float>& g) { return g.predict_entries(rows, cols, nullptr, nnz, base, 0.0, (float*)out, nullptr, true); },
	                   [&](Engine<double>& g) { return g.predict_entries(rows, cols, nullptr, nnz, base, 0.0, (double*)out, nullptr, true); });
}

int nmfamd_engine_score_device(nmfamd_engine* e, const int* rows, const int* cols, const void* values, long nnz, int base, double beta, void* out, double sums[4]) {
	if (!values || !sums) return NMFAMD_INVALID_ARGUMENT;
	return dispatch(e, [&](Engine<float>& g) { return g.predict_entries(rows, cols, (const float*)values, nnz, base, beta, (float*)out, sums, true); },
	                   [&](Engine<double>& g) { return g.predict_entries(rows, cols, (const double*)values, nnz, base, beta, (double*)out, sums, true); });
}

int nmfamd_engine_top_k(nmfamd_engine* e, const int* queries, long nq, int k, int axis, int base, const long* excl_ptr, const int* excl_idx, int* out_idx, void* out_scores) {
	return dispatch(e, [&](Engine<float>& g) { return g.top_k(queries, nq, k, axis, base, excl_ptr, excl_idx, 0, out_idx, (float*)out_scores, false); },
	                   [&](Engine<double>& g) { return g.top_k(queries, nq, k, axis, base, excl_ptr, excl_idx, 0, out_idx, (double*)out_scores, false); });
}

int nmfamd_engine_top_k_device(nmfamd_engine* e, const int* queries, long nq, int k, int axis, int base, const long* excl_ptr, const int* excl_idx, long excl_nnz,
                               int* out_idx, void* out_scores) {
	return dispatch(e, [&](Engine<float>& g) { return g.top_k(queries, nq, k, axis, base, excl_ptr, excl_idx, excl_nnz, out_idx, (float*)out_scores, true); },
	                   [&](Engine<double>& g) { return g.top_k(queries, nq, k, axis, base, excl_ptr, excl_idx, excl_nnz, out_idx, (double*)out_scores, true); });
}

int nmfamd_device_pointer_info(const void* p, int* kind, int* device, unsigned long long* bytes_from_p) {
	if (!kind || !device || !bytes_from_p) return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) { *kind = 0; *device = -1; *bytes_from_p = 0; return NMFAMD_NO_DEVICE; }
	device_pointer_info(p, kind, device, bytes_from_p);
	return NMFAMD_OK;
}

int nmfamd_engine_randomize(nmfamd_engine* e, unsigned seed, int w, int h) {
	return dispatch(e, [&](Engine<float>& g) { return g.randomize_factors(seed, w != 0, h != 0); },
	                   [&](Engine<double>& g) { return g.randomize_factors(seed, w != 0, h != 0); });
}

int nmfamd_engine_iterate(nmfamd_engine* e, int count, int first_iteration, int error_every, int last_iteration, int constant_w) {
	auto run = [&](auto& g) -> Status {
		for (int k = 0; k < count; ++k) {
			const int it = first_iteration + k;
			const bool err = (error_every > 0 && it % error_every == 0) || (last_iteration > 0 && it == last_iteration);
			Status s = g.iterate(err, constant_w != 0);
			if (s != ST_OK) return s;
		}
		return ST_OK;
	};
	return dispatch(e, run, run);
}

int nmfamd_engine_set_hals_penalties(nmfamd_engine* e, double l1W, double l1H, double l2W, double l2H) {
	auto set = [&](auto& g) { return g.set_hals_penalties(l1W, l1H, l2W, l2H); };
	return dispatch(e, set, set);
}

int nmfamd_engine_set_hals_sweeps(nmfamd_engine* e, int sweeps_h, int sweeps_w) {
	auto set = [&](auto& g) { return g.set_hals_sweeps(sweeps_h, sweeps_w); };
	return dispatch(e, set, set);
}

const char* nmfamd_missing_solver_fault(double solver, double sweeps_h, double sweeps_w, double l1_w, double l1_h, double l2_w, double l2_h, int elem_bytes,
                                        double missing_values, double missing_divergence, int r) {
	return nmfamd::missing_solver_fault(solver, sweeps_h, sweeps_w, l1_w, l1_h, l2_w, l2_h, elem_bytes == 4, missing_values == 1, missing_divergence == 0, r);
}

int nmfamd_engine_set_missing_solver(nmfamd_engine* e, int solver, int sweeps_h, int sweeps_w, double l1_w, double l1_h, double l2_w, double l2_h) {
	nmfamd::MissingSolver s;
	s.solver = solver; s.sweeps_h = sweeps_h; s.sweeps_w = sweeps_w; s.l1W = l1_w; s.l1H = l1_h; s.l2W = l2_w; s.l2H = l2_h;
	auto set = [&](auto& g) { return g.set_missing_solver(s); };
	return dispatch(e, set, set);
}

int nmfamd_engine_set_hals_sweep_tolerance(nmfamd_engine* e, double delta) {
	auto set = [&](auto& g) { return g.set_hals_sweep_tolerance(delta); };
	return dispatch(e, set, set);
}

int nmfamd_engine_set_nenmf_steps(nmfamd_engine* e, int steps_h, int steps_w) {
	auto set = [&](auto& g) { return g.set_nenmf_steps(steps_h, steps_w); };
	return dispatch(e, set, set);
}

int nmfamd_engine_set_nenmf_step_tolerance(nmfamd_engine* e, double delta) {
	auto set = [&](auto& g) { return g.set_nenmf_step_tolerance(delta); };
	return dispatch(e, set, set);
}

long nmfamd_engine_nenmf_step_counts(nmfamd_engine* e, int which, int* out, long capacity) {
	if (!e || !out) return -1;
	return e->elem_bytes == 4 ? e->f->nenmf_step_counts(which, out, capacity) : e->d->nenmf_step_counts(which, out, capacity);
}

long nmfamd_engine_hals_sweep_counts(nmfamd_engine* e, int which, int* out, long capacity) {
	if (!e || !out) return -1;
	return e->elem_bytes == 4 ? e->f->hals_sweep_counts(which, out, capacity) : e->d->hals_sweep_counts(which, out, capacity);
}

int nmfamd_engine_synchronize(nmfamd_engine* e) {
	if (!e) return NMFAMD_INVALID_ARGUMENT;
	hipStream_t s = e->elem_bytes == 4 ? e->f->stream() : e->d->stream();
	return hipStreamSynchronize(s) == hipSuccess ? NMFAMD_OK : NMFAMD_HIP_ERROR;
}

double nmfamd_engine_frobenius(nmfamd_engine* e) { return !e ? 0.0 : (e->elem_bytes == 4 ? e->f->frobenius() : e->d->frobenius()); }
double nmfamd_engine_kl_divergence(nmfamd_engine* e) { return !e ? 0.0 : (e->elem_bytes == 4 ? e->f->kl_divergence() : e->d->kl_divergence()); }
double nmfamd_engine_divergence(nmfamd_engine* e) { return !e ? 0.0 : (e->elem_bytes == 4 ? e->f->divergence_value() : e->d->divergence_value()); }
double nmfamd_engine_rmsd(nmfamd_engine* e) { return !e ? 0.0 : (e->elem_bytes == 4 ? e->f->rmsd() : e->d->rmsd()); }

int nmfamd_engine_kernel_timing(nmfamd_engine* e, int enable) {
	// enable: 0 = off, k > 0 = bracket the launches of every k-th iteration
	return dispatch(e, [&](Engine<float>& g) { g.enable_kernel_timing(enable != 0, enable); return ST_OK; },
	                   [&](Engine<double>& g) { g.enable_kernel_timing(enable != 0, enable); return ST_OK; });
}

int nmfamd_engine_kernel_timing_read(nmfamd_engine* e, double* total_ms, long* launches) {
	return dispatch(e, [&](Engine<float>& g) { g.dominant_stats(total_ms, launches); return ST_OK; },
	                   [&](Engine<double>& g) { g.dominant_stats(total_ms, launches); return ST_OK; });
}

int nmfamd_engine_kernel_timing_read2(nmfamd_engine* e, double* total_ms, long* launches, double* pair_overhead_ms) {
	if (!e) return NMFAMD_INVALID_ARGUMENT;
	if (e->elem_bytes == 4) e->f->dominant_stats(total_ms, launches, pair_overhead_ms); else e->d->dominant_stats(total_ms, launches, pair_overhead_ms);
	return NMFAMD_OK;
}

int nmfamd_engine_kernel_timing_read3(nmfamd_engine* e, double* total_ms, long* launches, double* pair_overhead_ms, double* kind_ms, long* kind_launches) {
	if (!e) return NMFAMD_INVALID_ARGUMENT;
	if (e->elem_bytes == 4) e->f->dominant_stats(total_ms, launches, pair_overhead_ms, kind_ms, kind_launches);
	else e->d->dominant_stats(total_ms, launches, pair_overhead_ms, kind_ms, kind_launches);
	return NMFAMD_OK;
}

int nmfamd_engine_geometry(const nmfamd_engine* e, nmfamd_geometry* out) {
	if (!e || !out) return NMFAMD_INVALID_ARGUMENT;
	if (e->elem_bytes == 4) fill_geometry(*e->f, out); else fill_geometry(*e->d, out);
	return NMFAMD_OK;
}

int nmfamd_plan_geometry(int m, int n, int r, int algorithm, const void* params_sized, unsigned long params_size, int elem_bytes, int row_blocks,
                         int num_cus, unsigned long long memory_side_cache_bytes, unsigned long long free_bytes, void* geometry_out, unsigned long struct_size) {
	AlgorithmParams p;
	if (!sized_params(params_sized, params_size, &p)) return NMFAMD_INVALID_ARGUMENT;
	if (!geometry_out || struct_size < 8 || (elem_bytes != 4 && elem_bytes != 8) || row_blocks < 1 || row_blocks > 64 || num_cus < 1) return NMFAMD_INVALID_ARGUMENT;
	g_create_error.clear();
	DeviceFacts device;
	device.num_cus = num_cus; device.memory_side_cache_bytes = (size_t)memory_side_cache_bytes; device.free_bytes = (size_t)free_bytes;
	nmfamd_geometry g;
	std::memset(&g, 0, sizeof(g));
	Status st;
	try {
		st = elem_bytes == 4 ? plan_geometry<float>(m, n, r, algorithm, p, row_blocks, device, &g) : plan_geometry<double>(m, n, r, algorithm, p, row_blocks, device, &g);
	} catch (const std::bad_alloc&) { return NMFAMD_NO_HOST_MEMORY; }
	if (st == ST_OK) std::memcpy(geometry_out, &g, struct_size < sizeof(g) ? (size_t)struct_size : sizeof(g));
	return (int)st;
}

int nmfamd_engine_geometry_sized(const nmfamd_engine* e, void* out, unsigned long struct_size) {
	if (!out || struct_size < 8) return NMFAMD_INVALID_ARGUMENT;
	nmfamd_geometry g;
	std::memset(&g, 0, sizeof(g));
	const int st = nmfamd_engine_geometry(e, &g);
	if (st != NMFAMD_OK) return st;
	std::memcpy(out, &g, struct_size < sizeof(g) ? (size_t)struct_size : sizeof(g));
	return NMFAMD_OK;
}

int nmfamd_engine_h_step(nmfamd_engine* e, int compute_error) {
	return dispatch(e, [&](Engine<float>& g) { return g.h_step(compute_error != 0); },
	                   [&](Engine<double>& g) { return g.h_step(compute_error != 0); });
}

int nmfamd_engine_set_sole_rank(nmfamd_engine* e, int sole) {
	return dispatch(e, [&](Engine<float>& g) { g.set_sole_rank(sole != 0); return ST_OK; },
	                   [&](Engine<double>& g) { g.set_sole_rank(sole != 0); return ST_OK; });
}

int nmfamd_engine_w_products(nmfamd_engine* e, void* exchange) {
	if (!exchange) return NMFAMD_INVALID_ARGUMENT;
	return dispatch(e, [&](Engine<float>& g) { return g.w_products((float*)exchange); },
	                   [&](Engine<double>& g) { return g.w_products((double*)exchange); });
}

int nmfamd_engine_w_finish(nmfamd_engine* e, const void* exchange, int compute_error) {
	if (!exchange) return NMFAMD_INVALID_ARGUMENT;
	return dispatch(e, [&](Engine<float>& g) { return g.w_finish((const float*)exchange, compute_error != 0); },
	                   [&](Engine<double>& g) { return g.w_finish((const double*)exchange, compute_error != 0); });
}

int nmfamd_engine_w_update_rows(nmfamd_engine* e, const void* num_rows, const void* hht, long row0, long rows, int compute_error, void* colsq) {
	return dispatch(e, [&](Engine<float>& g) { return g.w_update_rows((const float*)num_rows, (const float*)hht, row0, rows, compute_error != 0, (float*)colsq); },
	                   [&](Engine<double>& g) { return g.w_update_rows((const double*)num_rows, (const double*)hht, row0, rows, compute_error != 0, (double*)colsq); });
}
int nmfamd_engine_w_normalize_rows(nmfamd_engine* e, long row0, long rows, void* colsq) {
	return dispatch(e, [&](Engine<float>& g) { return g.w_normalize_rows(row0, rows, (float*)colsq); },
	                   [&](Engine<double>& g) { return g.w_normalize_rows(row0, rows, (double*)colsq); });
}
int nmfamd_engine_w_rows_replaced(nmfamd_engine* e) {
	return dispatch(e, [&](Engine<float>& g) { g.w_rows_replaced(); return ST_OK; }, [&](Engine<double>& g) { g.w_rows_replaced(); return ST_OK; });
}
void* nmfamd_engine_w_panel(nmfamd_engine* e) {
	if (!e) return nullptr;
	return e->elem_bytes == 4 ? (void*)e->f->w_panel() : (void*)e->d->w_panel();
}

long nmfamd_engine_error_terms(nmfamd_engine* e, int which, void* out, long capacity) {
	if (!e || !out || which < 0 || which > 2) return -1;
	auto copy = [&](auto& g) -> long {
		const auto& v = which == 0 ? g.terms_vtv_sorted() : (which == 1 ? g.terms_htwtv() : g.terms_hhtwtw());
		long cnt = std::min<long>((long)v.size(), capacity);
		if (cnt > 0) std::memcpy(out, v.data(), sizeof(v[0]) * (size_t)cnt);
		return cnt;
	};
	return e->elem_bytes == 4 ? copy(*e->f) : copy(*e->d);
}

long nmfamd_engine_error_terms_to_device(nmfamd_engine* e, void* dst_device, long capacity) {
	if (!e || !dst_device) return -1;
	return e->elem_bytes == 4 ? e->f->error_terms_to_device((float*)dst_device, capacity) : e->d->error_terms_to_device((double*)dst_device, capacity);
}

int nmfamd_host_kmeans_f32(const float* data, long ld, int m, int n, float* clusters, long ldc, int k, unsigned* membership, unsigned seed,
                           unsigned maxiter, double threshold, unsigned* iterations) {
	return host_kmeans<float>(data, ld, m, n, clusters, ldc, k, membership, seed, maxiter, threshold, iterations);
}
int nmfamd_host_kmeans_f64(const double* data, long ld, int m, int n, double* clusters, long ldc, int k, unsigned* membership, unsigned seed,
                           unsigned maxiter, double threshold, unsigned* iterations) {
	return host_kmeans<double>(data, ld, m, n, clusters, ldc, k, membership, seed, maxiter, threshold, iterations);
}
int nmfamd_host_init_f32(const float* V, long ldv, int m, int n, int r, int method, unsigned seed, float* W, float* H) {
	return host_init<float>(V, ldv, m, n, r, method, seed, W, H);
}
int nmfamd_host_init_f64(const double* V, long ldv, int m, int n, int r, int method, unsigned seed, double* W, double* H) {
	return host_init<double>(V, ldv, m, n, r, method, seed, W, H);
}

double nmfamd_resolve_frobenius_f32(const float* vtv_sorted, long n_vtv, float* htwtv, long n_htwtv, float* hhtwtw, long n_hhtwtw) {
	std::vector<float> a(vtv_sorted, vtv_sorted + n_vtv), b(htwtv, htwtv + n_htwtv), c(hhtwtw, hhtwtw + n_hhtwtw);
	double f = resolve_frobenius<float>(a, b, c);
	std::copy(b.begin(), b.end(), htwtv); std::copy(c.begin(), c.end(), hhtwtw);
	return f;
}

double nmfamd_resolve_frobenius_f64(const double* vtv_sorted, long n_vtv, double* htwtv, long n_htwtv, double* hhtwtw, long n_hhtwtw) {
	std::vector<double> a(vtv_sorted, vtv_sorted + n_vtv), b(htwtv, htwtv + n_htwtv), c(hhtwtw, hhtwtw + n_hhtwtw);
	double f = resolve_frobenius<double>(a, b, c);
	std::copy(b.begin(), b.end(), htwtv); std::copy(c.begin(), c.end(), hhtwtw);
	return f;
}

int nmfamd_engine_debug_read(nmfamd_engine* e, int which, void* out, long count) {
	return dispatch(e, [&](Engine<float>& g) { return g.debug_read(which, (float*)out, count); },
	                   [&](Engine<double>& g) { return g.debug_read(which, (double*)out, count); });
}

// ---- single operations on host data -------------------------------------------------------


// Tuning / diagnosis of the dominant kernel on synthetic device data: `reps` back-to-back launches
// timed with one event pair; optionally one more launch of the stamped build.
int nmfamd_tune_factor_product(int X, int Y, int reps, double* avg_us, unsigned long long* stamps_out, long stamps_capacity, long* stamps_count) {
	if (X <= 0 || Y <= 0 || reps <= 0 || !avg_us) return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	const int RP = 64;
	int dev = 0; hipDeviceProp_t prop;
	if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return NMFAMD_HIP_ERROR;
	FactorProductPlan plan = plan_factor_product(X, Y, RP, prop.multiProcessorCount);
	const long Xp = pad128(std::max<long>(X, (long)plan.xtiles * plan.th)), Yp = pad128(Y);
	DevBuf dA, dF, dS, dT;
	const long slab_stride = (long)RP * Xp;
	const long nwaves = (long)plan.xtiles * plan.splits * 8;
	if (dA.alloc(sizeof(float) * Xp * Yp) != hipSuccess || dF.alloc(sizeof(float) * RP * Yp) != hipSuccess ||
	    dS.alloc(sizeof(float) * slab_stride * plan.splits) != hipSuccess || dT.alloc(sizeof(unsigned long long) * 8 * nwaves) != hipSuccess) return NMFAMD_NO_DEVICE_MEMORY;
	if (launch_fill_uniform<float>((float*)dA.p, (int)Xp, (int)Xp, Yp, Yp, 1, nullptr) != hipSuccess) return NMFAMD_HIP_ERROR;   // Xp x Yp uniform (0,1]
	if (launch_fill_uniform<float>((float*)dF.p, RP, RP, Yp, Yp, 2, nullptr) != hipSuccess) return NMFAMD_HIP_ERROR;
	hipEvent_t e0, e1;
	if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return NMFAMD_HIP_ERROR;
	for (int i = 0; i < 3; ++i) launch_factor_product_f32(plan, (const float*)dA.p, plan.th * Yp, (const float*)dF.p, RP, (float*)dS.p, slab_stride, nullptr);
	(void)hipEventRecord(e0, nullptr);
	for (int i = 0; i < reps; ++i) launch_factor_product_f32(plan, (const float*)dA.p, plan.th * Yp, (const float*)dF.p, RP, (float*)dS.p, slab_stride, nullptr);
	(void)hipEventRecord(e1, nullptr);
	if (hipEventSynchronize(e1) != hipSuccess) return NMFAMD_HIP_ERROR;
	float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1);
	*avg_us = ms * 1e3 / reps;
	(void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
	if (stamps_out && stamps_capacity >= 8 * nwaves) {
		if (launch_factor_product_f32_stamped(plan, (const float*)dA.p, plan.th * Yp, (const float*)dF.p, RP, (float*)dS.p, slab_stride, (unsigned long long*)dT.p, nullptr) != hipSuccess) return NMFAMD_HIP_ERROR;
		if (hipMemcpy(stamps_out, dT.p, sizeof(unsigned long long) * 8 * nwaves, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
		if (stamps_count) *stamps_count = nwaves;
	} else if (stamps_count) *stamps_count = 0;
	return NMFAMD_OK;
}

int nmfamd_op_factor_product_f32(const float* A, long lda, int X, int Y, const float* F, long ldf, int r, float* OUT, long ldo, int use_valu, int* out_slabs) {
	return op_factor_product<float>(A, lda, X, Y, F, ldf, r, OUT, ldo, use_valu != 0, out_slabs);
}

int nmfamd_op_factor_product_bf16(const float* A, long lda, int X, int Y, const float* F, long ldf, int r, float* OUT, long ldo) {
	if (!A || !F || !OUT || X <= 0 || Y <= 0 || r <= 0 || lda < X || ldf < r || ldo < r) return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	int dev = 0; hipDeviceProp_t prop;
	if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return NMFAMD_HIP_ERROR;
	const int RP = padded_rank(r);
	const long Xp = pad128(X), Yp = pad128(Y);
	const int KS = (Y + 15) / 16;
	FactorProductPlan plan; plan.th = 128; plan.xtiles = (int)(Xp / 128); plan.steps_total = KS; plan.nb = 2; plan.chunks = 1;
	plan.splits = plan_splits_bf16(plan.xtiles, KS, RP, prop.multiProcessorCount);
	DevBuf dA, dF, dAb, dFb, dS, dO;
	const long slab_stride = (long)RP * Xp;
	if (dA.alloc(sizeof(float) * Xp * Yp) != hipSuccess || dF.alloc(sizeof(float) * RP * Yp) != hipSuccess ||
	    dAb.alloc(16 * (size_t)plan.xtiles * KS * 256) != hipSuccess || dFb.alloc(16 * (size_t)KS * (RP / 32) * 64) != hipSuccess ||
	    dS.alloc(sizeof(float) * slab_stride * plan.splits) != hipSuccess || dO.alloc(sizeof(float) * slab_stride) != hipSuccess) return NMFAMD_NO_DEVICE_MEMORY;
	if (hipMemcpy2D(dA.p, Xp * sizeof(float), A, lda * sizeof(float), X * sizeof(float), Y, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (hipMemcpy2D(dF.p, RP * sizeof(float), F, ldf * sizeof(float), r * sizeof(float), Y, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (launch_pack_stream_bf16((const float*)dA.p, Xp, X, Y, false, dAb.p, plan.xtiles, KS, nullptr) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (launch_pack_panel_bf16((const float*)dF.p, RP, Y, dFb.p, KS, nullptr) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (launch_factor_product_bf16(plan, dAb.p, KS, dFb.p, RP, (float*)dS.p, slab_stride, nullptr) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (launch_reduce_slabs<float>((const float*)dS.p, plan.splits, slab_stride, (float*)dO.p, slab_stride, nullptr) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (hipMemcpy2D(OUT, ldo * sizeof(float), dO.p, RP * sizeof(float), r * sizeof(float), X, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	return hipDeviceSynchronize() == hipSuccess ? NMFAMD_OK : NMFAMD_HIP_ERROR;
}

// x16: the x-tiled image in 16-row tiles (the engine's ONE resident image, read along its output index)
static int op_factor_product_x3(const float* A, long lda, int X, int Y, const float* F, long ldf, int r, float* OUT, long ldo, int reps, double* avg_us, bool y_tiled, bool x16 = false,
                                const InversePassenger* passenger = nullptr, const GramReduceArgs* ride = nullptr, int* out_plan = nullptr, int col_split = 0) {
	// ride: passenger workgroups of any other kind, every field as given (the Gram test entries); out_plan: {x-tiles, K slices} of the product launch
	// col_split 2 (r <= 64, the x-tiled form on 128-row tiles): 128 x 32 workgroups and one slab, as Engine::plan sets a narrow column shard's V H^T up
	if (col_split != 0 && (col_split != 2 || y_tiled || x16 || r > 64)) return NMFAMD_INVALID_ARGUMENT;
	if (!A || !F || !OUT || X <= 0 || Y <= 0 || r <= 0 || lda < X || ldf < r || ldo < r) return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	int dev = 0; hipDeviceProp_t prop;
	if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return NMFAMD_HIP_ERROR;
	const int RP = padded_rank(r);
	const long Xp = pad128(X), Yp = pad128(Y);
	const int KS = (Y + 15) / 16;
	FactorProductPlan plan; plan.th = 128; plan.xtiles = (int)(Xp / 128); plan.steps_total = KS; plan.nb = 2; plan.chunks = 1;
	plan.splits = plan_splits_x3(plan.xtiles, KS, prop.multiProcessorCount);
	if (col_split == 2) { plan.splits = 1; plan.col_split = 2; }
	DevBuf dA, dT, dF, dFb, dS, dO;
	const long slab_stride = (long)RP * Xp;
	if (dA.alloc(sizeof(float) * Xp * Yp) != hipSuccess || dT.alloc(sizeof(float) * Xp * Yp) != hipSuccess || dF.alloc(sizeof(float) * RP * Yp) != hipSuccess ||
	    dFb.alloc(3 * 16 * (size_t)(KS + 1) * (RP / 32) * 64) != hipSuccess ||
	    dS.alloc(sizeof(float) * slab_stride * plan.splits) != hipSuccess || dO.alloc(sizeof(float) * slab_stride) != hipSuccess) return NMFAMD_NO_DEVICE_MEMORY;
	if (hipMemset(dA.p, 0, sizeof(float) * Xp * Yp) != hipSuccess || hipMemset(dT.p, 0, sizeof(float) * Xp * Yp) != hipSuccess ||
	    hipMemset(dF.p, 0, sizeof(float) * RP * Yp) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (hipMemcpy2D(dA.p, Xp * sizeof(float), A, lda * sizeof(float), X * sizeof(float), Y, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (hipMemcpy2D(dF.p, RP * sizeof(float), F, ldf * sizeof(float), r * sizeof(float), Y, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	// x-tiled image of A (128-row tiles), or (y_tiled) the image tiled along the reduction index in 16-row tiles = the x-tiled image of A^T with tile height 16:
	// the form W^T V runs in on the engine's ONE resident image of V
	const int ith = (y_tiled || x16) ? 16 : 128;
	const long tstride = y_tiled ? 16 * Xp : (x16 ? 16 * Yp : 128 * Yp);
	if (y_tiled) { if (launch_tile_transposed<float>((const float*)dA.p, Xp, X, Y, (float*)dT.p, tstride, 16, nullptr) != hipSuccess) return NMFAMD_HIP_ERROR; }
	else if (launch_tile<float>((const float*)dA.p, Xp, X, Y, (float*)dT.p, tstride, ith, false, nullptr) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (launch_pack_panel_x3((const float*)dF.p, RP, Y, dFb.p, KS, nullptr) != hipSuccess) return NMFAMD_HIP_ERROR;
	GramReduceArgs rg = {nullptr, 0, nullptr, nullptr, 0};
	if (passenger) { rg.inv_a = passenger->a; rg.inv_out = passenger->out; rg.inv_offdiag = passenger->offdiag; rg.inv_diag = passenger->diag; rg.inv_r = passenger->r; }
	if (ride) rg = *ride;
	if (out_plan) { out_plan[0] = plan.xtiles; out_plan[1] = plan.splits; }
	if (hipError_t e = launch_factor_product_x3(plan, (const float*)dT.p, tstride, dFb.p, RP, (float*)dS.p, slab_stride, nullptr, (passenger || ride) ? &rg : nullptr, nullptr, y_tiled, ith); e != hipSuccess)
		return (passenger || ride) && e == hipErrorInvalidValue ? NMFAMD_INVALID_ARGUMENT : NMFAMD_HIP_ERROR;
	if (launch_reduce_slabs<float>((const float*)dS.p, plan.splits, slab_stride, (float*)dO.p, slab_stride, nullptr) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (hipMemcpy2D(OUT, ldo * sizeof(float), dO.p, RP * sizeof(float), r * sizeof(float), X, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (reps > 0 && avg_us) {
		// alternate between two images of A so that no launch finds its operand in the 256 MB memory-side cache
		// (inside an iteration the two products stream V and V^T in turn)
		DevBuf dT2;
		if (dT2.alloc(sizeof(float) * Xp * Yp) != hipSuccess) return NMFAMD_NO_DEVICE_MEMORY;
		if (hipMemcpy(dT2.p, dT.p, sizeof(float) * Xp * Yp, hipMemcpyDeviceToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
		hipEvent_t e0, e1;
		if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return NMFAMD_HIP_ERROR;
		for (int i = 0; i < 4; ++i) (void)launch_factor_product_x3(plan, (const float*)((i & 1) ? dT2.p : dT.p), tstride, dFb.p, RP, (float*)dS.p, slab_stride, nullptr, nullptr, nullptr, y_tiled, ith);
		(void)hipEventRecord(e0, nullptr);
		for (int i = 0; i < reps; ++i) (void)launch_factor_product_x3(plan, (const float*)((i & 1) ? dT2.p : dT.p), tstride, dFb.p, RP, (float*)dS.p, slab_stride, nullptr, nullptr, nullptr, y_tiled, ith);
		(void)hipEventRecord(e1, nullptr);
		if (hipEventSynchronize(e1) != hipSuccess) return NMFAMD_HIP_ERROR;
		float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1);
		*avg_us = ms * 1e3 / reps;
		(void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
	}
	return hipDeviceSynchronize() == hipSuccess ? NMFAMD_OK : NMFAMD_HIP_ERROR;
}

int nmfamd_op_factor_product_x3(const float* A, long lda, int X, int Y, const float* F, long ldf, int r, float* OUT, long ldo, int reps, double* avg_us) {
	return op_factor_product_x3(A, lda, X, Y, F, ldf, r, OUT, ldo, reps, avg_us, false);
}

int nmfamd_op_factor_product_x3_ytiled(const float* A, long lda, int X, int Y, const float* F, long ldf, int r, float* OUT, long ldo, int reps, double* avg_us) {
	return op_factor_product_x3(A, lda, X, Y, F, ldf, r, OUT, ldo, reps, avg_us, true);
}


int nmfamd_tune_factor_product_x3(int X, int Y, unsigned long long* stamps_out, long stamps_capacity, long* waves) {
	// X x Y = rows x columns of V (config 2: 10 000 x 5 000).  ONE image in 16-row tiles, as the engine keeps it; the two production forms alternate on it as they do
	// in an iteration (W^T V y-tiled, V H^T x-tiled), so the stamped launch finds the memory-side cache in the state the iteration leaves it in.
	// NMFAMD_X3_VARIANT = 10..13: the x-tiled launch is stamped; 30..33: the y-tiled one (kernels_x3.hip).
	if (X <= 0 || Y <= 0 || !stamps_out || !waves) return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	int dev = 0; hipDeviceProp_t prop;
	if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return NMFAMD_HIP_ERROR;
	const int RP = 64;
	const long Mp = pad128(X), Np = pad128(Y);
	const int ksW = (Y + 15) / 16, ksH = (X + 15) / 16;
	FactorProductPlan planW, planH;                  // V H^T: x = rows of V; W^T V: x = columns of V
	planW.th = planH.th = 128; planW.nb = planH.nb = 2; planW.chunks = planH.chunks = 1;
	planW.xtiles = (int)(Mp / 128); planW.steps_total = ksW; planW.splits = plan_splits_x3(planW.xtiles, ksW, prop.multiProcessorCount);
	planH.xtiles = (int)(Np / 128); planH.steps_total = ksH; planH.splits = plan_splits_x3(planH.xtiles, ksH, prop.multiProcessorCount);
	const char* ve = tuning_env("NMFAMD_X3_VARIANT");
	const bool ytiled = ve != nullptr && std::atoi(ve) >= 30;
	const FactorProductPlan& sp = ytiled ? planH : planW;
	const long nwaves = (long)sp.xtiles * sp.splits * 4;
	if (stamps_capacity < X3_STAMP_WORDS * nwaves) return NMFAMD_INVALID_ARGUMENT;
	DevBuf dA, dW, dH, dWx, dHx, dS, dT;
	const long slab_stride = (long)RP * std::max(Mp, Np);
	if (dA.alloc(sizeof(float) * Mp * Np) != hipSuccess || dW.alloc(sizeof(float) * RP * Mp) != hipSuccess || dH.alloc(sizeof(float) * RP * Np) != hipSuccess ||
	    dWx.alloc(3 * 16 * (size_t)(ksH + 1) * (RP / 32) * 64) != hipSuccess || dHx.alloc(3 * 16 * (size_t)(ksW + 1) * (RP / 32) * 64) != hipSuccess ||
	    dS.alloc(sizeof(float) * slab_stride * std::max(planW.splits, planH.splits)) != hipSuccess ||
	    dT.alloc(sizeof(unsigned long long) * X3_STAMP_WORDS * nwaves) != hipSuccess) return NMFAMD_NO_DEVICE_MEMORY;
	// (any buffer of the right size is an image of random data)
	if (launch_fill_uniform<float>((float*)dA.p, (int)Mp, (int)Mp, Np, Np, 1, nullptr) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (launch_fill_uniform<float>((float*)dW.p, RP, RP, Mp, Mp, 2, nullptr) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (launch_fill_uniform<float>((float*)dH.p, RP, RP, Np, Np, 3, nullptr) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (launch_pack_panel_x3((const float*)dW.p, RP, X, dWx.p, ksH, nullptr) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (launch_pack_panel_x3((const float*)dH.p, RP, Y, dHx.p, ksW, nullptr) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (hipMemset(dT.p, 0, sizeof(unsigned long long) * X3_STAMP_WORDS * nwaves) != hipSuccess) return NMFAMD_HIP_ERROR;
	const long stride = 16 * Np;
	for (int i = 0; i < 40; ++i) {
		const bool last = i == 39;
		unsigned long long* sy = last && ytiled ? (unsigned long long*)dT.p : nullptr;
		unsigned long long* sx = last && !ytiled ? (unsigned long long*)dT.p : nullptr;
		if (launch_factor_product_x3(planH, (const float*)dA.p, stride, dWx.p, RP, (float*)dS.p, slab_stride, nullptr, nullptr, sy, true, 16) != hipSuccess) return NMFAMD_HIP_ERROR;
		if (launch_factor_product_x3(planW, (const float*)dA.p, stride, dHx.p, RP, (float*)dS.p, slab_stride, nullptr, nullptr, sx, false, 16) != hipSuccess) return NMFAMD_HIP_ERROR;
	}
	if (hipMemcpy(stamps_out, dT.p, sizeof(unsigned long long) * X3_STAMP_WORDS * nwaves, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	*waves = nwaves;
	return NMFAMD_OK;
}

int nmfamd_op_factor_product_f64(const double* A, long lda, int X, int Y, const double* F, long ldf, int r, double* OUT, long ldo, int use_valu, int* out_slabs) {
	return op_factor_product<double>(A, lda, X, Y, F, ldf, r, OUT, ldo, use_valu != 0, out_slabs);
}

int nmfamd_op_gram_f32(const float* P, long ldp, int r, int len, float* G, long ldg) {
	if (!P || !G || r <= 0 || len <= 0 || ldp < r || ldg < r) return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	const int RP = padded_rank(r), parts = 128;
	const long lp = pad128(len);
	DevBuf dP, dPart, dG;
	if (dP.alloc(sizeof(float) * RP * lp) != hipSuccess || dPart.alloc(sizeof(float) * (size_t)RP * RP * parts) != hipSuccess || dG.alloc(sizeof(float) * RP * RP) != hipSuccess) return NMFAMD_NO_DEVICE_MEMORY;
	if (hipMemset(dP.p, 0, sizeof(float) * RP * lp) != hipSuccess) return NMFAMD_HIP_ERROR;   // the panel invariant: padding rows and columns are zero
	if (hipMemcpy2D(dP.p, RP * sizeof(float), P, ldp * sizeof(float), r * sizeof(float), len, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (launch_gram<float>((const float*)dP.p, RP, len, parts, (float*)dPart.p, (float*)dG.p, nullptr) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (hipMemcpy2D(G, ldg * sizeof(float), dG.p, RP * sizeof(float), r * sizeof(float), r, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	return hipDeviceSynchronize() == hipSuccess ? NMFAMD_OK : NMFAMD_HIP_ERROR;
}

int nmfamd_op_gram_f64(const double* P, long ldp, int r, int len, double* G, long ldg) {
	if (!P || !G || r <= 0 || len <= 0 || ldp < r || ldg < r) return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	const int RP = padded_rank(r, sizeof(double)), parts = 128;
	const long lp = pad128(len);
	DevBuf dP, dPart, dG;
	if (dP.alloc(sizeof(double) * RP * lp) != hipSuccess || dPart.alloc(sizeof(double) * (size_t)RP * RP * parts) != hipSuccess || dG.alloc(sizeof(double) * RP * RP) != hipSuccess) return NMFAMD_NO_DEVICE_MEMORY;
	if (hipMemcpy2D(dP.p, RP * sizeof(double), P, ldp * sizeof(double), r * sizeof(double), len, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (launch_gram<double>((const double*)dP.p, RP, len, parts, (double*)dPart.p, (double*)dG.p, nullptr) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (hipMemcpy2D(G, ldg * sizeof(double), dG.p, RP * sizeof(double), r * sizeof(double), r, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	return hipDeviceSynchronize() == hipSuccess ? NMFAMD_OK : NMFAMD_HIP_ERROR;
}

int nmfamd_op_inverse_f32(const float* A, long lda, int r, float offdiag, float diag, float* Ainv, long ldi) {
	if (!A || !Ainv || r <= 0 || lda < r || ldi < r) return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	const int RP = padded_rank(r);
	DevBuf dA, dI, dW;
	if (dA.alloc(sizeof(float) * RP * RP) != hipSuccess || dI.alloc(sizeof(float) * RP * RP) != hipSuccess || dW.alloc(sizeof(double) * 2 * (size_t)r * r) != hipSuccess) return NMFAMD_NO_DEVICE_MEMORY;
	if (hipMemcpy2D(dA.p, RP * sizeof(float), A, lda * sizeof(float), r * sizeof(float), r, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (launch_inverse_small<float>((float*)dA.p, RP, r, (float*)dI.p, (double*)dW.p, offdiag, diag, nullptr) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (hipMemcpy2D(Ainv, ldi * sizeof(float), dI.p, RP * sizeof(float), r * sizeof(float), r, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	return hipDeviceSynchronize() == hipSuccess ? NMFAMD_OK : NMFAMD_HIP_ERROR;
}

// Test entry of the r x r inverses on every route they are launched by (docs/INVERSE.md).  The device image of A starts as the caller's A_after (zeros without one) with
// the r x r block of A on top, the output as the caller's Ainv_full: what a launch leaves alone keeps the caller's sentinels.
extern "C++" {
template <typename T>
static int op_inverse_ex(const T* A, long lda, int r, T offdiag, T diag, int route, T* Ainv_full, T* A_after, int* rp_out,
                         const float* A_prod, long lda_prod, int X, int Y, const float* F_prod, long ldf_prod, float* OUT, long ldo) {
	constexpr bool f32 = std::is_same<T, float>::value;
	if (!A || !Ainv_full || !rp_out || r <= 0 || lda < r || route < 0 || route > 3) return NMFAMD_INVALID_ARGUMENT;
	const bool rides = route >= 2;
	if (rides && (!f32 || r > 64 || !A_prod || !F_prod || !OUT || X <= 0 || Y <= 0 || lda_prod < X || ldf_prod < 64 || ldo < 64)) return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	const int RP = padded_rank(r, sizeof(T));
	const size_t bytes = sizeof(T) * (size_t)RP * RP;
	DevBuf dA, dI, dW;
	if (dA.alloc(bytes) != hipSuccess || dI.alloc(bytes) != hipSuccess || dW.alloc(sizeof(double) * 2 * (size_t)r * r) != hipSuccess) return NMFAMD_NO_DEVICE_MEMORY;
	if (A_after && hipMemcpy(dA.p, A_after, bytes, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (hipMemcpy2D(dA.p, RP * sizeof(T), A, lda * sizeof(T), r * sizeof(T), r, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (hipMemcpy(dI.p, Ainv_full, bytes, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (rides) {
		if constexpr (f32) {
			const InversePassenger passenger = {(const float*)dA.p, (float*)dI.p, offdiag, diag, r};
			const int st = route == 2 ? op_factor_product<float>(A_prod, lda_prod, X, Y, F_prod, ldf_prod, 64, OUT, ldo, false, nullptr, &passenger)
			                          : op_factor_product_x3(A_prod, lda_prod, X, Y, F_prod, ldf_prod, 64, OUT, ldo, 0, nullptr, false, false, &passenger);
			if (st != NMFAMD_OK) return st;
		}
	} else {
		const hipError_t e = route == 0 ? launch_inverse_small<T>((T*)dA.p, RP, r, (T*)dI.p, (double*)dW.p, offdiag, diag, nullptr)
		                                : launch_inverse_householder<T>((T*)dA.p, RP, r, (T*)dI.p, (double*)dW.p, offdiag, diag, nullptr);
		if (e == hipErrorInvalidValue) return NMFAMD_INVALID_ARGUMENT;
		if (e != hipSuccess) return NMFAMD_HIP_ERROR;
	}
	if (hipDeviceSynchronize() != hipSuccess) return NMFAMD_HIP_ERROR;
	if (hipMemcpy(Ainv_full, dI.p, bytes, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (A_after && hipMemcpy(A_after, dA.p, bytes, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	*rp_out = RP;
	return NMFAMD_OK;
}
}

int nmfamd_op_inverse_ex_f32(const float* A, long lda, int r, float offdiag, float diag, int route, float* Ainv_full, float* A_after, int* rp_out,
                             const float* A_prod, long lda_prod, int X, int Y, const float* F_prod, long ldf_prod, float* OUT, long ldo) {
	return op_inverse_ex<float>(A, lda, r, offdiag, diag, route, Ainv_full, A_after, rp_out, A_prod, lda_prod, X, Y, F_prod, ldf_prod, OUT, ldo);
}

int nmfamd_op_inverse_ex_f64(const double* A, long lda, int r, double offdiag, double diag, int route, double* Ainv_full, double* A_after, int* rp_out,
                             const float* A_prod, long lda_prod, int X, int Y, const float* F_prod, long ldf_prod, float* OUT, long ldo) {
	return op_inverse_ex<double>(A, lda, r, offdiag, diag, route, Ainv_full, A_after, rp_out, A_prod, lda_prod, X, Y, F_prod, ldf_prod, OUT, ldo);
}

// Test entry of the rank-64 Gram matrix from the split image (gram_image.h, docs/GRAM.md): one launch at a time (`launches` of them in a row into the same buffers), every
// input caller-built, every output buffer uploaded as the caller filled it.  ride 0: launch_gram_image_args; 1 / 2: the same request as passenger workgroups of the x-tiled /
// y-tiled split-operand product over the 16-row image of A_prod, F_prod (the engine's two forms), whose result goes to OUT_ride and, from a launch without passengers, to OUT_plain.
int nmfamd_op_gram_image_f32(const float* P, int len, const float* colsq_part, int colsq_parts, int normalize, int ksplit, int spread, int finish, int ride, int launches,
                             float* G, long g_elems, float* scale, float* spread_out, unsigned* counter, int* plan,
                             const float* A_prod, long lda_prod, int X, int Y, const float* F_prod, long ldf_prod, float* OUT_plain, float* OUT_ride, long ldo) {
	if (!G || !plan || !counter || len <= 0 || launches < 1 || launches > 4 || ride < 0 || ride > 3 || (colsq_part && colsq_parts < 1) || (finish && !spread_out)) return NMFAMD_INVALID_ARGUMENT;
	if (ride != 0 && (!A_prod || !F_prod || !OUT_plain || !OUT_ride || X <= 0 || Y <= 0 || lda_prod < X || ldf_prod < 64 || ldo < 64)) return NMFAMD_INVALID_ARGUMENT;
	// (a request the launcher must refuse still gets there: the buffer only has to hold what an accepted one writes)
	const int slices = spread > 0 ? GRAM_SPREAD_SLICES : (ksplit > 1 ? std::min(ksplit, GRAM_KSPLIT_MAX) : 1);
	if (g_elems < 4096L * slices) return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	const int KS = (len + 15) / 16;
	DevBuf dP, dX, dC, dG, dS, dO, dN;
	if (dP.alloc(sizeof(float) * 64 * (size_t)(16 * KS)) != hipSuccess || dX.alloc(3 * 16 * (size_t)(KS + 1) * 2 * 64) != hipSuccess ||
	    dC.alloc(sizeof(float) * 64 * (size_t)std::max(colsq_parts, 1)) != hipSuccess || dG.alloc(sizeof(float) * g_elems) != hipSuccess || dS.alloc(sizeof(float) * 64) != hipSuccess ||
	    dO.alloc(sizeof(float) * 4096 * (size_t)launches) != hipSuccess || dN.alloc(sizeof(unsigned)) != hipSuccess) return NMFAMD_NO_DEVICE_MEMORY;
	if (P) {
		if (hipMemcpy(dP.p, P, sizeof(float) * 64 * (size_t)len, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
		if (launch_pack_panel_x3((const float*)dP.p, 64, len, dX.p, KS, nullptr) != hipSuccess) return NMFAMD_HIP_ERROR;
	}
	if (colsq_part && hipMemcpy(dC.p, colsq_part, sizeof(float) * 64 * (size_t)colsq_parts, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (hipMemcpy(dG.p, G, sizeof(float) * g_elems, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (scale && hipMemcpy(dS.p, scale, sizeof(float) * 64, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (spread_out && hipMemcpy(dO.p, spread_out, sizeof(float) * 4096 * (size_t)launches, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (hipMemcpy(dN.p, counter, sizeof(unsigned), hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	GramReduceArgs rg = {nullptr, 0, (float*)dG.p, scale ? (float*)dS.p : nullptr, normalize};
	rg.image = P ? dX.p : nullptr; rg.image_ks = KS;
	rg.colsq_part = colsq_part ? (const float*)dC.p : nullptr; rg.colsq_parts = colsq_part ? colsq_parts : 0;
	rg.ksplit = ksplit; rg.spread = spread;
	if (finish) rg.spread_counter = (unsigned*)dN.p;
	int pplan[2] = {0, 0};
	if (ride != 0) {
		// the product alone first: what it writes must not depend on who rides
		if (int st = op_factor_product_x3(A_prod, lda_prod, X, Y, F_prod, ldf_prod, 64, OUT_plain, ldo, 0, nullptr, ride == 2, ride == 1, nullptr, nullptr, nullptr, ride == 3 ? 2 : 0); st != NMFAMD_OK) return st;
	}
	for (int i = 0; i < launches; ++i) {
		if (finish) rg.spread_out = (float*)dO.p + 4096L * i;
		if (ride != 0) {
			if (int st = op_factor_product_x3(A_prod, lda_prod, X, Y, F_prod, ldf_prod, 64, OUT_ride, ldo, 0, nullptr, ride == 2, ride == 1, nullptr, &rg, pplan, ride == 3 ? 2 : 0); st != NMFAMD_OK) return st;
		} else {
			const hipError_t e = launch_gram_image_args(rg, nullptr);
			if (e == hipErrorInvalidValue) return NMFAMD_INVALID_ARGUMENT;
			if (e != hipSuccess) return NMFAMD_HIP_ERROR;
		}
		if (hipDeviceSynchronize() != hipSuccess) return NMFAMD_HIP_ERROR;
		if (hipMemcpy(counter + 1 + i, dN.p, sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	}
	if (hipMemcpy(G, dG.p, sizeof(float) * g_elems, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (scale && hipMemcpy(scale, dS.p, sizeof(float) * 64, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (spread_out && hipMemcpy(spread_out, dO.p, sizeof(float) * 4096 * (size_t)launches, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	plan[0] = slices; plan[1] = gram_image_workgroups(rg); plan[2] = (KS + 2) / 2; plan[3] = KS;        // (the launchers' own count, kernels.h)
	plan[4] = pplan[0]; plan[5] = pplan[1];
	return NMFAMD_OK;
}

// Test entry of the rank-64 Gram matrix from partial matrices (kernels_mu64.hip, docs/GRAM.md), one launcher per route:
//   0 launch_mu64_gram_partials   1 launch_mu64_gram_reduce   2 gram_reduce_block_x3, the passengers of the split-operand product (x-tiled over the 16-row image)
//   6 the same passengers on the col_split product launch (x-tiled over 128-row tiles, 128 x 32 workgroups)
//   3 launch_gram64_from_partials (scale NULL: the sum alone)   4 launch_gram64_normalize_all   5 launch_gram64_reduce_scale_all
// Every buffer is uploaded as the caller filled it and copied back whole.
int nmfamd_op_gram64_partials_f32(int route, float* P, int len_pad, float* partials, int parts, int normalize, const float* sumsq_part, int sq_parts,
                                  float* Graw, float* G, float* scale, void* x3, int x3_ks,
                                  const float* A_prod, long lda_prod, int X, int Y, const float* F_prod, long ldf_prod, float* OUT_plain, float* OUT_ride, long ldo) {
	if (route < 0 || route > 6) return NMFAMD_INVALID_ARGUMENT;
	const bool cs_ride = route == 6;          // route 2 on the 128 x 32 workgroups of a col_split product launch
	if (cs_ride) route = 2;
	const bool panel = route == 0 || route == 4 || route == 5;
	if (panel && (!P || len_pad < 64 || len_pad % 64 != 0)) return NMFAMD_INVALID_ARGUMENT;
	if (route == 0 ? (!partials || parts != len_pad / 64) : (!partials || !G || parts < 0)) return NMFAMD_INVALID_ARGUMENT;
	if ((route == 4 || route == 5) && (!scale || !x3 || x3_ks < 0 || x3_ks > len_pad / 16)) return NMFAMD_INVALID_ARGUMENT;
	if (route == 4 && !Graw) return NMFAMD_INVALID_ARGUMENT;
	if (route >= 1 && route <= 4 && parts < 1) return NMFAMD_INVALID_ARGUMENT;
	if (route == 5 && (!sumsq_part || sq_parts < 0)) return NMFAMD_INVALID_ARGUMENT;
	if (route == 2 && (!A_prod || !F_prod || !OUT_plain || !OUT_ride || X <= 0 || Y <= 0 || lda_prod < X || ldf_prod < 64 || ldo < 64)) return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	const size_t pb = panel ? sizeof(float) * 64 * (size_t)len_pad : 0, qb = sizeof(float) * 4096 * (size_t)std::max(parts, 1), gb = sizeof(float) * 4096;
	const size_t xb = panel && x3 ? 3 * 16 * (size_t)(len_pad / 16 + 1) * 2 * 64 : 0, sb = sizeof(float) * 64 * (size_t)std::max(sq_parts, 1);
	DevBuf dP, dQ, dR, dG, dS, dX, dV;
	if (dP.alloc(pb) != hipSuccess || dQ.alloc(qb) != hipSuccess || dR.alloc(gb) != hipSuccess || dG.alloc(gb) != hipSuccess || dS.alloc(256) != hipSuccess ||
	    dX.alloc(xb) != hipSuccess || dV.alloc(sb) != hipSuccess) return NMFAMD_NO_DEVICE_MEMORY;
	if (pb && hipMemcpy(dP.p, P, pb, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (parts > 0 && hipMemcpy(dQ.p, partials, sizeof(float) * 4096 * (size_t)parts, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (Graw && hipMemcpy(dR.p, Graw, gb, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (G && hipMemcpy(dG.p, G, gb, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (scale && hipMemcpy(dS.p, scale, 256, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (xb && hipMemcpy(dX.p, x3, xb, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (sumsq_part && sq_parts > 0 && hipMemcpy(dV.p, sumsq_part, sizeof(float) * 64 * (size_t)sq_parts, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	GramReduceArgs rg = {(const float*)dQ.p, parts, (float*)dG.p, scale ? (float*)dS.p : nullptr, normalize};
	hipError_t e = hipSuccess;
	switch (route) {
		case 0: e = launch_mu64_gram_partials((const float*)dP.p, len_pad, (float*)dQ.p, nullptr); break;
		case 1: e = launch_mu64_gram_reduce(rg, nullptr); break;
		case 2: {
			if (int st = op_factor_product_x3(A_prod, lda_prod, X, Y, F_prod, ldf_prod, 64, OUT_plain, ldo, 0, nullptr, false, !cs_ride, nullptr, nullptr, nullptr, cs_ride ? 2 : 0); st != NMFAMD_OK) return st;
			if (int st = op_factor_product_x3(A_prod, lda_prod, X, Y, F_prod, ldf_prod, 64, OUT_ride, ldo, 0, nullptr, false, !cs_ride, nullptr, &rg, nullptr, cs_ride ? 2 : 0); st != NMFAMD_OK) return st;
			break;
		}
		case 3: e = launch_gram64_from_partials((const float*)dQ.p, parts, (float*)dG.p, scale ? (float*)dS.p : nullptr, nullptr); break;
		case 4: e = launch_gram64_normalize_all((const float*)dQ.p, parts, (float*)dR.p, (float*)dG.p, (float*)dS.p, (float*)dP.p, len_pad, dX.p, x3_ks, nullptr); break;
		default: e = launch_gram64_reduce_scale_all((const float*)dQ.p, parts, (const float*)dV.p, sq_parts, (float*)dG.p, (float*)dS.p, (float*)dP.p, len_pad, dX.p, x3_ks, nullptr); break;
	}
	if (e == hipErrorInvalidValue) return NMFAMD_INVALID_ARGUMENT;
	if (e != hipSuccess || hipDeviceSynchronize() != hipSuccess) return NMFAMD_HIP_ERROR;
	if (pb && hipMemcpy(P, dP.p, pb, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (route == 0 && hipMemcpy(partials, dQ.p, sizeof(float) * 4096 * (size_t)parts, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (Graw && hipMemcpy(Graw, dR.p, gb, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (G && hipMemcpy(G, dG.p, gb, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (scale && hipMemcpy(scale, dS.p, 256, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (xb && hipMemcpy(x3, dX.p, xb, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	return NMFAMD_OK;
}

// Test entry of the Gram matrix at padded ranks 128 ... 512 in fp32 (kernels_wide.hip, gram_wide.h, docs/GRAM.md):
//   0 launch_gram_wide_f32 (mirrored slices, launch_reduce_partials)   1 launch_gram_wide_fused_f32 (k_gram_wide_x3<2, false>, k_gram_reduce_x3)
//   2 launch_gram_reduce_x3 alone on the caller's slices   3 the slices as passenger workgroups (GramReduceArgs::wide_P) of the x-tiled split-operand product of
//   A_prod (X x Y) and F_prod (r_prod x Y) over the 16-row image, for the slice count of route 1
// P: [len][RP]; partial: part_elems floats; every output buffer is uploaded as the caller filled it and copied back whole.  plan[0]: the slice count the launcher settled on.
int nmfamd_op_gram_wide_f32(int route, const float* P, int RP, int len, int parts, float* partial, long part_elems, float* G, void* qx3, const float* sumsq_part, int sq_parts,
                            float* scale_out, int* plan,
                            const float* A_prod, long lda_prod, int X, int Y, const float* F_prod, long ldf_prod, int r_prod, float* OUT_plain, float* OUT_ride, long ldo) {
	if (route < 0 || route > 3 || !partial || !plan || RP < 64 || RP % 64 != 0 || RP > 512 || part_elems < 0) return NMFAMD_INVALID_ARGUMENT;
	if (route != 2 && (!P || len <= 0)) return NMFAMD_INVALID_ARGUMENT;
	if (route != 3 && !G) return NMFAMD_INVALID_ARGUMENT;
	if (sumsq_part && (!scale_out || sq_parts < 1)) return NMFAMD_INVALID_ARGUMENT;
	if (route == 3 && (!A_prod || !F_prod || !OUT_plain || !OUT_ride || X <= 0 || Y <= 0 || r_prod <= 0 || lda_prod < X || ldf_prod < r_prod || ldo < r_prod)) return NMFAMD_INVALID_ARGUMENT;
	// (the passengers read the panel with the PRODUCT's padded rank: the two must agree, or the product be the rank-64 form that refuses them)
	if (route == 3 && padded_rank(r_prod) != RP && padded_rank(r_prod) != 64) return NMFAMD_INVALID_ARGUMENT;
	const bool wide = RP % 128 == 0;
	// the slice count each launcher settles on, from the launchers' own functions (kernels_wide.hip); a request a launcher must refuse still gets there, and writes nothing
	int settled = parts;
	if (wide && route == 0) settled = gram_wide_parts(RP, len, parts);
	if (wide && (route == 1 || route == 3)) settled = gram_wide_fused_parts(RP, len, parts);
	const size_t mat = (size_t)RP * RP;
	if (wide && settled >= 1 && (size_t)part_elems < mat * (size_t)settled) return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	const long lp = pad128(std::max(len, 1));
	const size_t xb = 3 * 16 * (size_t)(RP / 16 + 1) * (RP / 32) * 64;
	DevBuf dP, dQ, dG, dX, dV, dS;
	if (dP.alloc(sizeof(float) * RP * (size_t)lp) != hipSuccess || dQ.alloc(sizeof(float) * (size_t)part_elems) != hipSuccess || dG.alloc(sizeof(float) * mat) != hipSuccess ||
	    dX.alloc(xb) != hipSuccess || dV.alloc(sizeof(float) * RP * (size_t)std::max(sq_parts, 1)) != hipSuccess || dS.alloc(sizeof(float) * RP) != hipSuccess) return NMFAMD_NO_DEVICE_MEMORY;
	if (P && hipMemcpy(dP.p, P, sizeof(float) * RP * (size_t)len, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (part_elems > 0 && hipMemcpy(dQ.p, partial, sizeof(float) * (size_t)part_elems, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (G && hipMemcpy(dG.p, G, sizeof(float) * mat, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (qx3 && hipMemcpy(dX.p, qx3, xb, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (sumsq_part && hipMemcpy(dV.p, sumsq_part, sizeof(float) * RP * (size_t)sq_parts, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (scale_out && hipMemcpy(dS.p, scale_out, sizeof(float) * RP, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	const float* sq = sumsq_part ? (const float*)dV.p : nullptr;
	hipError_t e = hipSuccess;
	if (route == 0) e = launch_gram_wide_f32((const float*)dP.p, RP, len, parts, (float*)dQ.p, (float*)dG.p, nullptr);
	else if (route == 1) e = launch_gram_wide_fused_f32((const float*)dP.p, RP, len, parts, (float*)dQ.p, (float*)dG.p, qx3 ? dX.p : nullptr, sq, sq_parts, (float*)dS.p, nullptr);
	else if (route == 2) e = (parts >= 1 && (size_t)part_elems < mat * (size_t)parts) ? hipErrorInvalidValue
	                       : launch_gram_reduce_x3((const float*)dQ.p, parts, RP, (float*)dG.p, qx3 ? dX.p : nullptr, sq, sq_parts, (float*)dS.p, nullptr);
	else {
		GramReduceArgs rg = {nullptr, 0, nullptr, nullptr, 0};
		rg.wide_P = (const float*)dP.p; rg.wide_len = len; rg.wide_parts = settled; rg.wide_partial = (float*)dQ.p;
		if (int st = op_factor_product_x3(A_prod, lda_prod, X, Y, F_prod, ldf_prod, r_prod, OUT_plain, ldo, 0, nullptr, false, true); st != NMFAMD_OK) return st;
		if (int st = op_factor_product_x3(A_prod, lda_prod, X, Y, F_prod, ldf_prod, r_prod, OUT_ride, ldo, 0, nullptr, false, true, nullptr, &rg); st != NMFAMD_OK) return st;
	}
	if (e == hipErrorInvalidValue) return NMFAMD_INVALID_ARGUMENT;
	if (e != hipSuccess || hipDeviceSynchronize() != hipSuccess) return NMFAMD_HIP_ERROR;
	if (part_elems > 0 && hipMemcpy(partial, dQ.p, sizeof(float) * (size_t)part_elems, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (G && hipMemcpy(G, dG.p, sizeof(float) * mat, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (qx3 && hipMemcpy(qx3, dX.p, xb, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (scale_out && hipMemcpy(scale_out, dS.p, sizeof(float) * RP, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	plan[0] = settled;
	return NMFAMD_OK;
}

// Test / measurement entry of kernels_tri.hip (padded rank 256): the passes between a factor update and the next product.
// P: [len][ldp] panel rows; colsq (r values) or NULL; theta: nsNMF smoothing.  Outputs (any may be NULL): P_out = the panel after the optional
// column normalisation; pack_out [len][r] = the bf16 fragments of the smoothed panel, widened back to fp32; G_raw / G_smooth [r][r].
// One multiplicative update of a panel at padded rank 256 in the form the bf16 path uses it (PanelTriExtras): old values with a pending column scale, optional
// scale + smoothing of the numerator rows, new rows written unnormalised together with their bf16 fragments; then the pending scale of the new panel and the
// Gram matrix of its rounded rows.  All matrices row-major [len][r] / [r][r].
int nmfamd_op_tri_update_f32(const float* P, const float* num, const float* Q, int r, int len, const float* old_colsq, int transform_num, const float* num_colsq,
                             float theta, float frag_theta, int transform_den, float* P_out, float* pack_out, float* scale_out, float* gram_out,
                             float* gram_raw_out, float* gram_image_out, float* diag_out) {
	if (!P || !num || !Q || r <= 0 || len <= 0) return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	const int RP = padded_rank(r);
	if (!tri_kernels_available(RP)) return NMFAMD_INVALID_ARGUMENT;
	const long lp = pad128(len), KS = (len + 15) / 16;
	const size_t pack_bytes = 16 * (size_t)KS * (RP / 32) * 64;
	int dev = 0, cus = 256;
	hipDeviceProp_t prop;
	if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
	const int parts = panel_update_parts(RP, sizeof(float), (int)lp);
	DevBuf dP, dN, dQ, dOs, dNs, dPack, dPart, dG, dSq, dStage, dScale, dQx, dDummy, dG2, dImg, dDiag;
	const size_t img_bytes = (size_t)3 * 16 * (RP / 16 + 1) * (RP / 32) * 64;
	if (dG2.alloc(sizeof(float) * RP * RP) != hipSuccess || dImg.alloc(img_bytes) != hipSuccess || dDiag.alloc(sizeof(float) * RP) != hipSuccess) return NMFAMD_NO_DEVICE_MEMORY;
	if (dP.alloc(sizeof(float) * RP * lp) != hipSuccess || dN.alloc(sizeof(float) * RP * lp) != hipSuccess || dQ.alloc(sizeof(float) * RP * RP) != hipSuccess ||
	    dOs.alloc(sizeof(float) * RP) != hipSuccess || dNs.alloc(sizeof(float) * RP) != hipSuccess || dPack.alloc(pack_bytes) != hipSuccess ||
	    dPart.alloc(sizeof(float) * (size_t)gram_tri_partial_elems(cus)) != hipSuccess || dG.alloc(sizeof(float) * RP * RP) != hipSuccess ||
	    dSq.alloc(sizeof(float) * ((size_t)parts + 16) * RP) != hipSuccess || dStage.alloc(sizeof(float) * RP * colsq_stage_parts()) != hipSuccess ||
	    dScale.alloc(sizeof(float) * RP) != hipSuccess || dDummy.alloc(sizeof(float) * RP * 4) != hipSuccess || dQx.alloc((size_t)3 * 16 * (RP / 16 + 1) * (RP / 32) * 64) != hipSuccess) return NMFAMD_NO_DEVICE_MEMORY;
	if (hipMemcpy2D(dP.p, RP * sizeof(float), P, r * sizeof(float), r * sizeof(float), len, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (hipMemcpy2D(dN.p, RP * sizeof(float), num, r * sizeof(float), r * sizeof(float), len, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (hipMemcpy2D(dQ.p, RP * sizeof(float), Q, r * sizeof(float), r * sizeof(float), r, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (old_colsq && hipMemcpy(dOs.p, old_colsq, sizeof(float) * r, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (num_colsq && hipMemcpy(dNs.p, num_colsq, sizeof(float) * r, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	PanelTriExtras ex;
	ex.num_transform = transform_num != 0;
	ex.num_colsq = num_colsq ? (const float*)dNs.p : nullptr; ex.num_colsq_parts = 1;
	const float off = theta / (float)(unsigned)r, diag = (float)((1.0 - theta) + off);
	ex.num_a = diag - off; ex.num_b = off; ex.r = r;
	ex.old_colsq = old_colsq ? (const float*)dOs.p : nullptr; ex.old_colsq_parts = 1;
	ex.frag_out = dPack.p; ex.frag_KS = KS;
	const float foff = frag_theta / (float)(unsigned)r, fdiag = (float)((1.0 - frag_theta) + foff);
	if (frag_theta != 0.0f) { ex.frag_a = fdiag - foff; ex.frag_b = foff; }
	if (transform_den) { ex.den_transform = true; ex.den_a = ex.num_a; ex.den_b = ex.num_b; ex.den_colsq = ex.num_colsq; ex.den_colsq_parts = 1; }
	if (launch_panel_update<float>(PANEL_MU, (float*)dP.p, (const float*)dN.p, 1, 0, (const float*)dQ.p, RP, (int)lp, std::numeric_limits<float>::epsilon(), nullptr, len,
	                               (float*)dSq.p, nullptr, nullptr, nullptr, nullptr, 0, dQx.p, &ex) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (launch_colsq_stage((const float*)dSq.p, RP, parts, (float*)dStage.p, nullptr, nullptr) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (launch_scale_panel_tri((float*)dDummy.p, RP, 4, (const float*)dStage.p, colsq_stage_parts(), (float*)dScale.p, nullptr) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (launch_gram_tri_bf16(dPack.p, RP, KS, cus, (float*)dPart.p, (float*)dG.p, (const float*)dStage.p, colsq_stage_parts(), cus, nullptr) != hipSuccess) return NMFAMD_HIP_ERROR;
	// the reduction that also leaves the split image and the diagonal (what the engine's H step consumes)
	if (launch_gram_tri_bf16_image(dPack.p, RP, KS, cus, (float*)dPart.p, (float*)dG2.p, dImg.p, (float*)dDiag.p, cus, nullptr) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (gram_raw_out && hipMemcpy2D(gram_raw_out, r * sizeof(float), dG2.p, RP * sizeof(float), r * sizeof(float), r, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (diag_out && hipMemcpy(diag_out, dDiag.p, sizeof(float) * r, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (gram_image_out) {
		// image element: plane p of A(c, k) at bf16 index ((((ks * NBT + nb) * 3 + p) * 2 + h) * 32 + (c & 31)) * 8 + (k & 7), ks = k / 16, nb = c / 32, h = (k / 8) & 1; A(c, k) = G(k, c)
		std::vector<uint16_t> h(img_bytes / 2);
		if (hipMemcpy(h.data(), dImg.p, img_bytes, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
		const int NBT = RP / 32;
		for (int k = 0; k < r; ++k)
			for (int c = 0; c < r; ++c) {
				float sum = 0.f;
				for (int pl = 2; pl >= 0; --pl) {
					const size_t idx = (((((size_t)(k / 16) * NBT + c / 32) * 3 + pl) * 2 + ((k / 8) & 1)) * 32 + (c & 31)) * 8 + (k & 7);
					const uint32_t bits = (uint32_t)h[idx] << 16;
					float f;
					std::memcpy(&f, &bits, 4);
					sum += f;
				}
				gram_image_out[(size_t)k * r + c] = sum;
			}
	}
	if (P_out && hipMemcpy2D(P_out, r * sizeof(float), dP.p, RP * sizeof(float), r * sizeof(float), len, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (scale_out && hipMemcpy(scale_out, dScale.p, sizeof(float) * r, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (gram_out && hipMemcpy2D(gram_out, r * sizeof(float), dG.p, RP * sizeof(float), r * sizeof(float), r, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (pack_out) {
		std::vector<uint16_t> h(pack_bytes / 2);
		if (hipMemcpy(h.data(), dPack.p, pack_bytes, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
		const int NBT = RP / 32;
		for (long y = 0; y < len; ++y)
			for (int c = 0; c < r; ++c) {
				const long frag = ((y / 16) * NBT + c / 32) * 64 + ((y / 8) & 1) * 32 + (c & 31);
				const uint32_t bits = (uint32_t)h[frag * 8 + (y & 7)] << 16;
				float f;
				std::memcpy(&f, &bits, 4);
				pack_out[y * r + c] = f;
			}
	}
	return hipDeviceSynchronize() == hipSuccess ? NMFAMD_OK : NMFAMD_HIP_ERROR;
}

int nmfamd_op_factor_passes_f32(const float* P, long ldp, int r, int len, const float* colsq, float theta, float* P_out, float* pack_out,
                                float* G_raw, float* G_smooth, int reps, double* avg_us_finish, double* avg_us_gram) {
	if (!P || r <= 0 || len <= 0 || ldp < r) return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	const int RP = padded_rank(r);
	if (!tri_kernels_available(RP)) return NMFAMD_INVALID_ARGUMENT;
	const long lp = pad128(len), KS = (len + 15) / 16;
	const size_t pack_bytes = 16 * (size_t)KS * (RP / 32) * 64;
	int dev = 0, cus = 256;
	hipDeviceProp_t prop;
	if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
	DevBuf dP, dP0, dSq, dPack, dPart, dG, dGs;
	if (dP.alloc(sizeof(float) * RP * lp) != hipSuccess || dP0.alloc(sizeof(float) * RP * lp) != hipSuccess || dSq.alloc(sizeof(float) * RP) != hipSuccess ||
	    dPack.alloc(pack_bytes) != hipSuccess || dPart.alloc(sizeof(float) * (size_t)gram_tri_partial_elems(cus)) != hipSuccess ||
	    dG.alloc(sizeof(float) * RP * RP) != hipSuccess || dGs.alloc(sizeof(float) * RP * RP) != hipSuccess) return NMFAMD_NO_DEVICE_MEMORY;
	if (hipMemset(dP0.p, 0, sizeof(float) * RP * lp) != hipSuccess || hipMemset(dSq.p, 0, sizeof(float) * RP) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (hipMemcpy2D(dP0.p, RP * sizeof(float), P, ldp * sizeof(float), r * sizeof(float), len, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (colsq && hipMemcpy(dSq.p, colsq, sizeof(float) * r, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	const float off = theta / (float)(unsigned)r, diag = (float)((1.0 - theta) + off);
	hipEvent_t e0, e1;
	if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return NMFAMD_HIP_ERROR;
	const int n_reps = reps > 0 ? reps : 1;
	float ms_finish = 0.f, ms_gram = 0.f;
	for (int it = 0; it < n_reps; ++it) {
		// (the normalisation is in place: every repetition starts from the caller's panel)
		if (hipMemcpyAsync(dP.p, dP0.p, sizeof(float) * RP * lp, hipMemcpyDeviceToDevice, nullptr) != hipSuccess) return NMFAMD_HIP_ERROR;
		float ms = 0.f;
		(void)hipEventRecord(e0, nullptr);
		if (launch_finish_panel_bf16((float*)dP.p, RP, r, 0, lp, colsq ? (const float*)dSq.p : nullptr, 1, off, diag, dPack.p, KS, nullptr) != hipSuccess) return NMFAMD_HIP_ERROR;
		(void)hipEventRecord(e1, nullptr);
		if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) return NMFAMD_HIP_ERROR;
		ms_finish += ms;
		(void)hipEventRecord(e0, nullptr);
		if (launch_gram_tri((const float*)dP.p, RP, len, cus, (float*)dPart.p, (float*)dG.p, cus, nullptr) != hipSuccess) return NMFAMD_HIP_ERROR;
		if (launch_smooth_gram((const float*)dG.p, (float*)dGs.p, RP, r, off, diag, nullptr, nullptr) != hipSuccess) return NMFAMD_HIP_ERROR;
		(void)hipEventRecord(e1, nullptr);
		if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) return NMFAMD_HIP_ERROR;
		ms_gram += ms;
	}
	(void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
	if (avg_us_finish) *avg_us_finish = 1e3 * ms_finish / n_reps;
	if (avg_us_gram) *avg_us_gram = 1e3 * ms_gram / n_reps;
	if (P_out && hipMemcpy2D(P_out, ldp * sizeof(float), dP.p, RP * sizeof(float), r * sizeof(float), len, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (G_raw && hipMemcpy2D(G_raw, r * sizeof(float), dG.p, RP * sizeof(float), r * sizeof(float), r, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (G_smooth && hipMemcpy2D(G_smooth, r * sizeof(float), dGs.p, RP * sizeof(float), r * sizeof(float), r, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (pack_out) {
		std::vector<uint16_t> h(pack_bytes / 2);
		if (hipMemcpy(h.data(), dPack.p, pack_bytes, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
		const int NBT = RP / 32;
		for (long y = 0; y < len; ++y)
			for (int c = 0; c < r; ++c) {
				const long frag = ((y / 16) * NBT + c / 32) * 64 + ((y / 8) & 1) * 32 + (c & 31);
				const uint32_t bits = (uint32_t)h[frag * 8 + (y & 7)] << 16;
				float f;
				std::memcpy(&f, &bits, 4);
				pack_out[y * r + c] = f;
			}
	}
	return hipDeviceSynchronize() == hipSuccess ? NMFAMD_OK : NMFAMD_HIP_ERROR;
}

} // extern "C"

// Test entries of kernels_hals.hip: one launch of the sweep or of the normalisation on caller-supplied padded arrays, so that tests can put what
// they like into the padding.  No argument checks beyond the buffer sizes: the launchers decide what they accept.
namespace {
template <typename T>
int op_hals_sweep(T* P, const T* slabs, int S, long slab_stride, const T* G, int RP, int r, int len_pad, int len_valid, T* ps, T* sumsq_part, int* parts, T l1 = T(0), T l2 = T(0),
                  int sweeps = 0, bool dyn = false, double tol = 0, int* counts = nullptr, bool apg = false) {
	// sweeps == 0: the single-sweep launcher itself (nmfamd_op_hals_sweep_*, _pen_*); otherwise launch_panel_sweeps_hals, which decides about the count;
	// dyn: launch_panel_sweeps_hals_dyn with tol and (optionally) counts; apg: launch_panel_steps_apg with `sweeps` as its step count (nmfamd_op_apg_steps_*);
	// apg and dyn: launch_panel_steps_apg_dyn with tol and (optionally) counts (nmfamd_op_apg_steps_dyn_*)
	if (!P || !slabs || !G || !parts || S < 1 || RP < 1 || RP > 4096 || len_pad < 1 || slab_stride < (long)len_pad * RP) return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	const int np = apg ? panel_steps_apg_parts(RP, sizeof(T), len_pad) : panel_sweep_hals_parts(RP, sizeof(T), len_pad);
	const size_t panel = sizeof(T) * (size_t)len_pad * RP, all_slabs = sizeof(T) * (size_t)(((long)S - 1) * slab_stride + (long)len_pad * RP);
	DevBuf dP, dS, dG, dPs, dSq, dCnt;
	if (dP.alloc(panel) != hipSuccess || dS.alloc(all_slabs) != hipSuccess || dG.alloc(sizeof(T) * (size_t)RP * RP) != hipSuccess ||
	    dPs.alloc(sizeof(T) * (size_t)len_pad) != hipSuccess || dSq.alloc(sizeof(T) * (size_t)(np > 0 ? np : 1) * RP) != hipSuccess) return NMFAMD_NO_DEVICE_MEMORY;
	if (counts && (dCnt.alloc(sizeof(int) * (size_t)len_pad) != hipSuccess)) return NMFAMD_NO_DEVICE_MEMORY;
	if (counts && hipMemcpy(dCnt.p, counts, sizeof(int) * (size_t)len_pad, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (hipMemcpy(dP.p, P, panel, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dS.p, slabs, all_slabs, hipMemcpyHostToDevice) != hipSuccess ||
	    hipMemcpy(dG.p, G, sizeof(T) * (size_t)RP * RP, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (ps && hipMemcpy(dPs.p, ps, sizeof(T) * (size_t)len_pad, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (sumsq_part && np > 0 && hipMemcpy(dSq.p, sumsq_part, sizeof(T) * (size_t)np * RP, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	const hipError_t err = apg && dyn  ? launch_panel_steps_apg_dyn<T>((T*)dP.p, (const T*)dS.p, S, slab_stride, (const T*)dG.p, RP, r, len_pad, len_valid,
	                                                                   ps ? (T*)dPs.p : nullptr, sumsq_part ? (T*)dSq.p : nullptr, nullptr, l1, l2, sweeps, (T)tol,
	                                                                   counts ? (int*)dCnt.p : nullptr)
	                       : apg       ? launch_panel_steps_apg<T>((T*)dP.p, (const T*)dS.p, S, slab_stride, (const T*)dG.p, RP, r, len_pad, len_valid,
	                                                               ps ? (T*)dPs.p : nullptr, sumsq_part ? (T*)dSq.p : nullptr, nullptr, l1, l2, sweeps)
	                       : dyn       ? launch_panel_sweeps_hals_dyn<T>((T*)dP.p, (const T*)dS.p, S, slab_stride, (const T*)dG.p, RP, r, len_pad, len_valid,
	                                                                     ps ? (T*)dPs.p : nullptr, sumsq_part ? (T*)dSq.p : nullptr, nullptr, l1, l2, sweeps, tol,
	                                                                     counts ? (int*)dCnt.p : nullptr)
	                       : sweeps == 0 ? launch_panel_sweep_hals<T>((T*)dP.p, (const T*)dS.p, S, slab_stride, (const T*)dG.p, RP, r, len_pad, len_valid,
	                                                                ps ? (T*)dPs.p : nullptr, sumsq_part ? (T*)dSq.p : nullptr, nullptr, l1, l2)
	                                   : launch_panel_sweeps_hals<T>((T*)dP.p, (const T*)dS.p, S, slab_stride, (const T*)dG.p, RP, r, len_pad, len_valid,
	                                                                 ps ? (T*)dPs.p : nullptr, sumsq_part ? (T*)dSq.p : nullptr, nullptr, l1, l2, sweeps);
	if (err == hipErrorInvalidValue) return NMFAMD_INVALID_ARGUMENT;
	if (err != hipSuccess || hipDeviceSynchronize() != hipSuccess) return NMFAMD_HIP_ERROR;
	if (hipMemcpy(P, dP.p, panel, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (ps && hipMemcpy(ps, dPs.p, sizeof(T) * (size_t)len_pad, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (sumsq_part && hipMemcpy(sumsq_part, dSq.p, sizeof(T) * (size_t)np * RP, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (counts && hipMemcpy(counts, dCnt.p, sizeof(int) * (size_t)len_pad, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	*parts = np;
	return NMFAMD_OK;
}

template <typename T>
int op_hals_normalize(T* Wt, int RP, int mpad, T* H, int npad, const T* sumsq_part, int parts) {
	if (!Wt || !H || !sumsq_part || RP < 4 || RP % 4 != 0 || mpad < 1 || npad < 1 || parts < 1) return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	const size_t w = sizeof(T) * (size_t)mpad * RP, h = sizeof(T) * (size_t)npad * RP;
	DevBuf dW, dH, dSq;
	// (parts + 16) * RP: the launcher reduces into the scratch behind the partials, as the engine sizes its buffer
	if (dW.alloc(w) != hipSuccess || dH.alloc(h) != hipSuccess || dSq.alloc(sizeof(T) * ((size_t)parts + 16) * RP) != hipSuccess) return NMFAMD_NO_DEVICE_MEMORY;
	if (hipMemcpy(dW.p, Wt, w, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dH.p, H, h, hipMemcpyHostToDevice) != hipSuccess ||
	    hipMemcpy(dSq.p, sumsq_part, sizeof(T) * (size_t)parts * RP, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (launch_hals_normalize<T>((T*)dW.p, RP, mpad, (T*)dH.p, npad, (T*)dSq.p, parts, nullptr) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return NMFAMD_HIP_ERROR;
	if (hipMemcpy(Wt, dW.p, w, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(H, dH.p, h, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	return NMFAMD_OK;
}

template <typename T>
int op_beta_half_step(T* A, const T* B, const T* X, long ldx, int RP, int r, int out_pad, int out_valid, int red_pad, int red_valid, double beta_value, double l1d,
                      double l2d, int form, int force_slabs, const T* dsum, T* t_frob, T* t_div, T* sumsq_part, T* sum_part, int* slabs, const T* Omega = nullptr,
                      bool weighted = false, bool mixed = false) {
	// weighted: the half-step of kernels_beta_weighted.hip with Omega, an array like X (dsum is not used); mixed (float only): the fused launch of kernels_beta_bf16.hip
	const bool update = form == 0 || form == 1, terms = form == 1 || form == 2;
	if (weighted && !Omega) return NMFAMD_INVALID_ARGUMENT;
	const double beta = (double)(T)beta_value;      // (in the precision of T, as the launchers take it)
	const T l1 = (T)l1d, l2 = (T)l2d;
	if (!A || !B || !X || !beta_half_step_available(RP) || r < 1 || r > RP || !std::isfinite(beta) || !(l1d >= 0) || !(l2d >= 0) || !std::isfinite((double)l1) ||
	    !std::isfinite((double)l2) || form < 0 || form > 2 || out_pad < 128 || out_pad % 128 != 0 ||
	    red_pad < 128 || red_pad % 128 != 0 || out_valid < 0 || out_valid > out_pad || red_valid < 0 || red_valid > red_pad || ldx < red_pad || ldx % 4 != 0 ||
	    force_slabs < 0 || (update && beta == 1 && !dsum && !weighted) || (terms && (!t_frob || !t_div)))
		return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	int dev = 0;
	hipDeviceProp_t prop;
	if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return NMFAMD_HIP_ERROR;
	const BetaPlan plan = plan_beta_half_step(out_pad, red_pad, RP, sizeof(T), prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256, force_slabs);
	if (slabs) *slabs = plan.slabs;
	const size_t panelA = sizeof(T) * (size_t)out_pad * RP, panelB = sizeof(T) * (size_t)red_pad * RP, image = sizeof(T) * (size_t)out_pad * (size_t)ldx;
	const size_t parts = (size_t)(out_pad / 128) * RP;
	const long part_stride = (long)out_pad * RP;
	DevBuf dA, dB, dX, dNum, dDen, dT, dOut, dSum, dD, dO;
	if (weighted && (dO.alloc(image) != hipSuccess)) return NMFAMD_NO_DEVICE_MEMORY;
	if (weighted && hipMemcpy(dO.p, Omega, image, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (dA.alloc(panelA) != hipSuccess || dB.alloc(panelB) != hipSuccess || dX.alloc(image) != hipSuccess || dNum.alloc(panelA * plan.slabs) != hipSuccess ||
	    dDen.alloc(panelA * plan.slabs) != hipSuccess || dT.alloc(sizeof(T) * 2 * (size_t)plan.slabs * out_pad) != hipSuccess ||
	    dOut.alloc(sizeof(T) * 2 * (size_t)out_pad) != hipSuccess || dSum.alloc(sizeof(T) * 2 * parts) != hipSuccess || dD.alloc(sizeof(T) * (size_t)RP) != hipSuccess)
		return NMFAMD_NO_DEVICE_MEMORY;
	if (hipMemcpy(dA.p, A, panelA, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dB.p, B, panelB, hipMemcpyHostToDevice) != hipSuccess ||
	    hipMemcpy(dX.p, X, image, hipMemcpyHostToDevice) != hipSuccess || hipMemset(dSum.p, 0, sizeof(T) * 2 * parts) != hipSuccess ||
	    hipMemset(dOut.p, 0, sizeof(T) * 2 * (size_t)out_pad) != hipSuccess || hipMemset(dD.p, 0, sizeof(T) * (size_t)RP) != hipSuccess)
		return NMFAMD_HIP_ERROR;
	if (dsum && hipMemcpy(dD.p, dsum, sizeof(T) * (size_t)RP, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	T* tf = terms ? (T*)dT.p : nullptr;
	T* td = terms ? (T*)dT.p + (size_t)plan.slabs * out_pad : nullptr;
	T* of = terms ? (T*)dOut.p : nullptr;
	T* od = terms ? (T*)dOut.p + out_pad : nullptr;
	const T eps = std::numeric_limits<T>::epsilon();
	if (mixed) {
		if constexpr (sizeof(T) == 4) {
			if (launch_beta_fused_bf16((const T*)dX.p, ldx, (const T*)dA.p, (const T*)dB.p, RP, beta, update, terms, eps, plan, (T*)dNum.p, (T*)dDen.p, part_stride, tf, td,
			                           out_pad, out_pad, out_valid, red_valid, nullptr) != hipSuccess)
				return NMFAMD_HIP_ERROR;
		} else return NMFAMD_INVALID_ARGUMENT;
	} else if ((weighted ? launch_beta_fused_weighted<T>((const T*)dX.p, (const T*)dO.p, ldx, (const T*)dA.p, (const T*)dB.p, RP, beta, update, terms, eps, plan, (T*)dNum.p,
	                                              (T*)dDen.p, part_stride, tf, td, out_pad, out_pad, out_valid, red_valid, nullptr)
	              : launch_beta_fused<T>((const T*)dX.p, ldx, (const T*)dA.p, (const T*)dB.p, RP, beta, update, terms, eps, plan, (T*)dNum.p, (T*)dDen.p, part_stride, tf, td,
	                                     out_pad, out_pad, out_valid, red_valid, nullptr)) != hipSuccess)
		return NMFAMD_HIP_ERROR;
	if (launch_beta_update<T>((T*)dA.p, (const T*)dNum.p, (const T*)dDen.p, part_stride, plan.slabs, (const T*)dD.p, RP, r, out_pad, out_valid, eps, beta, l1, l2, update,
	                          (T*)dSum.p, (T*)dSum.p + parts, tf, td, out_pad, of, od, nullptr, weighted) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
		return NMFAMD_HIP_ERROR;
	if (hipMemcpy(A, dA.p, panelA, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (terms && (hipMemcpy(t_frob, of, sizeof(T) * (size_t)out_pad, hipMemcpyDeviceToHost) != hipSuccess ||
	              hipMemcpy(t_div, od, sizeof(T) * (size_t)out_pad, hipMemcpyDeviceToHost) != hipSuccess)) return NMFAMD_HIP_ERROR;
	if (sumsq_part && hipMemcpy(sumsq_part, dSum.p, sizeof(T) * parts, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (sum_part && hipMemcpy(sum_part, (T*)dSum.p + parts, sizeof(T) * parts, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	return NMFAMD_OK;
}

// k_beta_update_rows on caller-built arrays: P [out_pad][RP], num_part / den_part [slabs][out_pad][RP], dsum [RP] (beta = 1), Aacc / Bacc [out_pad][RP] (online)
template <typename T>
int op_beta_update_rows(T* P, T* Aacc, T* Bacc, const T* num_part, const T* den_part, int slabs, const T* dsum, int RP, int r, int out_pad, int out_valid, double beta_value,
                        double l1d, double l2d, int online, double rho, int flush, T* sum_part) {
	const double beta = (double)(T)beta_value;
	const T l1 = (T)l1d, l2 = (T)l2d;
	if (!P || !num_part || !beta_half_step_available(RP) || r < 1 || r > RP || !std::isfinite(beta) || !(l1d >= 0) || !(l2d >= 0) || !std::isfinite((double)l1) ||
	    !std::isfinite((double)l2) || out_pad < 128 || out_pad % 128 != 0 || out_valid < 0 || out_valid > out_pad || slabs < 1 || slabs > BETA_MAX_SLABS ||
	    (beta == 1 ? !dsum : !den_part) || (online && (!Aacc || !Bacc || !(rho >= 0) || !(rho <= 1))))
		return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	const size_t panel = sizeof(T) * (size_t)out_pad * RP, sums = sizeof(T) * (size_t)(out_pad / BETA_ROWS_PER_WG) * RP;
	DevBuf dP, dA, dB, dNum, dDen, dD, dSum;
	if (dP.alloc(panel) != hipSuccess || dA.alloc(panel) != hipSuccess || dB.alloc(panel) != hipSuccess || dNum.alloc(panel * slabs) != hipSuccess ||
	    dDen.alloc(panel * slabs) != hipSuccess || dD.alloc(sizeof(T) * (size_t)RP) != hipSuccess || dSum.alloc(sums) != hipSuccess)
		return NMFAMD_NO_DEVICE_MEMORY;
	if (hipMemcpy(dP.p, P, panel, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dNum.p, num_part, panel * slabs, hipMemcpyHostToDevice) != hipSuccess ||
	    hipMemset(dSum.p, 0, sums) != hipSuccess)
		return NMFAMD_HIP_ERROR;
	if (den_part && hipMemcpy(dDen.p, den_part, panel * slabs, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (dsum && hipMemcpy(dD.p, dsum, sizeof(T) * (size_t)RP, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (online && (hipMemcpy(dA.p, Aacc, panel, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dB.p, Bacc, panel, hipMemcpyHostToDevice) != hipSuccess)) return NMFAMD_HIP_ERROR;
	if (launch_beta_update_rows<T>((T*)dP.p, (T*)dA.p, (T*)dB.p, (const T*)dNum.p, (const T*)dDen.p, (long)out_pad * RP, slabs, (const T*)dD.p, RP, r, out_pad, out_valid,
	                               std::numeric_limits<T>::epsilon(), beta, l1, l2, online != 0, (T)rho, flush != 0, (T*)dSum.p, nullptr) != hipSuccess ||
	    hipDeviceSynchronize() != hipSuccess)
		return NMFAMD_HIP_ERROR;
	if (hipMemcpy(P, dP.p, panel, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (online && (hipMemcpy(Aacc, dA.p, panel, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(Bacc, dB.p, panel, hipMemcpyDeviceToHost) != hipSuccess)) return NMFAMD_HIP_ERROR;
	if (sum_part && hipMemcpy(sum_part, dSum.p, sums, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	return NMFAMD_OK;
}

// The fused launch of a half-step alone (launch_beta_fused<T>, launch_beta_fused_weighted<T> with Omega, launch_beta_fused_bf16 with mixed), with op_beta_half_step's
// plan, on caller-built arrays.  plan_out: slabs, tiles, tiles_per_slab, bo, kt.  All four output arrays NULL: the plan only, nothing launched -- the caller sizes
// num_part / den_part [slabs][out_pad][RP] and tf_part / td_part [slabs][out_pad] from it.  The outputs are uploaded as the caller filled them and are not cleared,
// so a test sees what the launch wrote and what it left alone.
template <typename T>
int op_beta_fused(const T* A, const T* B, const T* X, const T* Omega, long ldx, int RP, int out_pad, int out_valid, int red_pad, int red_valid, double beta_value,
                  int update, int terms, int mixed, int force_slabs, T* num_part, T* den_part, T* tf_part, T* td_part, int* plan_out) {
	const double beta = (double)(T)beta_value;
	const bool plan_only = !num_part && !den_part && !tf_part && !td_part;
	if (!plan_out || !beta_half_step_available(RP) || !std::isfinite(beta) || out_pad < 128 || out_pad % 128 != 0 || red_pad < 128 || red_pad % 128 != 0 ||
	    out_valid < 0 || out_valid > out_pad || red_valid < 0 || red_valid > red_pad || ldx < red_pad || ldx % 4 != 0 || force_slabs < 0 || (mixed && (Omega || sizeof(T) != 4)))
		return NMFAMD_INVALID_ARGUMENT;
	if (!plan_only && (!A || !B || !X || !num_part || !den_part || (terms && (!tf_part || !td_part)))) return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	int dev = 0;
	hipDeviceProp_t prop;
	if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return NMFAMD_HIP_ERROR;
	const BetaPlan plan = plan_beta_half_step(out_pad, red_pad, RP, sizeof(T), prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256, force_slabs);
	plan_out[0] = plan.slabs; plan_out[1] = plan.tiles; plan_out[2] = plan.tiles_per_slab; plan_out[3] = plan.bo; plan_out[4] = plan.kt;
	if (plan_only) return NMFAMD_OK;
	const size_t panelA = sizeof(T) * (size_t)out_pad * RP, panelB = sizeof(T) * (size_t)red_pad * RP, image = sizeof(T) * (size_t)out_pad * (size_t)ldx;
	const size_t parts = panelA * plan.slabs, tparts = sizeof(T) * (size_t)plan.slabs * out_pad;
	const long part_stride = (long)out_pad * RP;
	DevBuf dA, dB, dX, dO, dNum, dDen, dTf, dTd;
	if (dA.alloc(panelA) != hipSuccess || dB.alloc(panelB) != hipSuccess || dX.alloc(image) != hipSuccess || (Omega && dO.alloc(image) != hipSuccess) ||
	    dNum.alloc(parts) != hipSuccess || dDen.alloc(parts) != hipSuccess || dTf.alloc(tparts) != hipSuccess || dTd.alloc(tparts) != hipSuccess)
		return NMFAMD_NO_DEVICE_MEMORY;
	if (hipMemcpy(dA.p, A, panelA, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dB.p, B, panelB, hipMemcpyHostToDevice) != hipSuccess ||
	    hipMemcpy(dX.p, X, image, hipMemcpyHostToDevice) != hipSuccess || (Omega && hipMemcpy(dO.p, Omega, image, hipMemcpyHostToDevice) != hipSuccess) ||
	    hipMemcpy(dNum.p, num_part, parts, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dDen.p, den_part, parts, hipMemcpyHostToDevice) != hipSuccess)
		return NMFAMD_HIP_ERROR;
	if (terms && (hipMemcpy(dTf.p, tf_part, tparts, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dTd.p, td_part, tparts, hipMemcpyHostToDevice) != hipSuccess))
		return NMFAMD_HIP_ERROR;
	T* tf = terms ? (T*)dTf.p : nullptr;
	T* td = terms ? (T*)dTd.p : nullptr;
	const T eps = std::numeric_limits<T>::epsilon();
	hipError_t err = hipErrorInvalidValue;
	if (mixed) {
		if constexpr (sizeof(T) == 4)
			err = launch_beta_fused_bf16((const T*)dX.p, ldx, (const T*)dA.p, (const T*)dB.p, RP, beta, update != 0, terms != 0, eps, plan, (T*)dNum.p, (T*)dDen.p,
			                             part_stride, tf, td, out_pad, out_pad, out_valid, red_valid, nullptr);
	} else if (Omega)
		err = launch_beta_fused_weighted<T>((const T*)dX.p, (const T*)dO.p, ldx, (const T*)dA.p, (const T*)dB.p, RP, beta, update != 0, terms != 0, eps, plan, (T*)dNum.p,
		                                    (T*)dDen.p, part_stride, tf, td, out_pad, out_pad, out_valid, red_valid, nullptr);
	else
		err = launch_beta_fused<T>((const T*)dX.p, ldx, (const T*)dA.p, (const T*)dB.p, RP, beta, update != 0, terms != 0, eps, plan, (T*)dNum.p, (T*)dDen.p, part_stride,
		                           tf, td, out_pad, out_pad, out_valid, red_valid, nullptr);
	if (err == hipErrorInvalidValue) return NMFAMD_INVALID_ARGUMENT;
	if (err != hipSuccess || hipDeviceSynchronize() != hipSuccess) return NMFAMD_HIP_ERROR;
	if (hipMemcpy(num_part, dNum.p, parts, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(den_part, dDen.p, parts, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (terms && (hipMemcpy(tf_part, dTf.p, tparts, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(td_part, dTd.p, tparts, hipMemcpyDeviceToHost) != hipSuccess))
		return NMFAMD_HIP_ERROR;
	return NMFAMD_OK;
}

// launch_beta_update<T> alone on caller-built partial panels: P [out_pad][RP], num_part / den_part [slabs][out_pad][RP] (either may be NULL where the launch does not
// take it), dsum [RP], tf_part / td_part [slabs][out_pad] (both or neither).  sumsq_part / sum_part [out_pad / 128][RP] and t_frob / t_div [out_pad] are uploaded as the
// caller filled them.  Which combinations run is the launcher's decision: its hipErrorInvalidValue comes back as NMFAMD_INVALID_ARGUMENT, nothing launched.
template <typename T>
int op_beta_update(T* P, const T* num_part, const T* den_part, int slabs, const T* dsum, int RP, int r, int out_pad, int out_valid, double beta_value, double l1d,
                   double l2d, int weighted, int update, const T* tf_part, const T* td_part, T* sumsq_part, T* sum_part, T* t_frob, T* t_div) {
	// (the sizes every buffer below is cut from; everything else is left to launch_beta_update)
	if (!P || RP < 1 || RP > 256 || out_pad < 128 || out_pad % 128 != 0 || out_valid < 0 || out_valid > out_pad || slabs < 1 || slabs > BETA_MAX_SLABS ||
	    !sumsq_part || !sum_part)
		return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	const size_t panel = sizeof(T) * (size_t)out_pad * RP, sums = sizeof(T) * (size_t)(out_pad / 128) * RP, rows = sizeof(T) * (size_t)out_pad;
	DevBuf dP, dNum, dDen, dD, dSq, dSm, dTf, dTd, dOf, dOd;
	if (dP.alloc(panel) != hipSuccess || dNum.alloc(panel * slabs) != hipSuccess || dDen.alloc(panel * slabs) != hipSuccess || dD.alloc(sizeof(T) * (size_t)RP) != hipSuccess ||
	    dSq.alloc(sums) != hipSuccess || dSm.alloc(sums) != hipSuccess || dTf.alloc(rows * slabs) != hipSuccess || dTd.alloc(rows * slabs) != hipSuccess ||
	    dOf.alloc(rows) != hipSuccess || dOd.alloc(rows) != hipSuccess)
		return NMFAMD_NO_DEVICE_MEMORY;
	if (hipMemcpy(dP.p, P, panel, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dSq.p, sumsq_part, sums, hipMemcpyHostToDevice) != hipSuccess ||
	    hipMemcpy(dSm.p, sum_part, sums, hipMemcpyHostToDevice) != hipSuccess)
		return NMFAMD_HIP_ERROR;
	if (num_part && hipMemcpy(dNum.p, num_part, panel * slabs, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (den_part && hipMemcpy(dDen.p, den_part, panel * slabs, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (dsum && hipMemcpy(dD.p, dsum, sizeof(T) * (size_t)RP, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (tf_part && hipMemcpy(dTf.p, tf_part, rows * slabs, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (td_part && hipMemcpy(dTd.p, td_part, rows * slabs, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (t_frob && hipMemcpy(dOf.p, t_frob, rows, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (t_div && hipMemcpy(dOd.p, t_div, rows, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	const hipError_t err = launch_beta_update<T>((T*)dP.p, num_part ? (const T*)dNum.p : nullptr, den_part ? (const T*)dDen.p : nullptr, (long)out_pad * RP, slabs,
	                                             dsum ? (const T*)dD.p : nullptr, RP, r, out_pad, out_valid, std::numeric_limits<T>::epsilon(), beta_value, (T)l1d, (T)l2d,
	                                             update != 0, (T*)dSq.p, (T*)dSm.p, tf_part ? (const T*)dTf.p : nullptr, td_part ? (const T*)dTd.p : nullptr, out_pad,
	                                             t_frob ? (T*)dOf.p : nullptr, t_div ? (T*)dOd.p : nullptr, nullptr, weighted != 0);
	if (err == hipErrorInvalidValue) return NMFAMD_INVALID_ARGUMENT;
	if (err != hipSuccess || hipDeviceSynchronize() != hipSuccess) return NMFAMD_HIP_ERROR;
	if (hipMemcpy(P, dP.p, panel, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(sumsq_part, dSq.p, sums, hipMemcpyDeviceToHost) != hipSuccess ||
	    hipMemcpy(sum_part, dSm.p, sums, hipMemcpyDeviceToHost) != hipSuccess)
		return NMFAMD_HIP_ERROR;
	if (t_frob && hipMemcpy(t_frob, dOf.p, rows, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (t_div && hipMemcpy(t_div, dOd.p, rows, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	return NMFAMD_OK;
}

// Test entries of kernels_sparse.hip: one launch each on caller-built arrays, eps = epsilon of T as in Engine::iterate_kl.  The arguments are checked as far as the
// buffer sizes and the indices go (a stored index outside the gathered panel would be read on the device); which padded ranks run is the launchers' decision.
// Output arrays are uploaded as the caller filled them and are not cleared, so a test sees what a launch wrote and what it left alone.
bool sparse_image_ok(const int* ptr, const int* idx, long nnz, int rows, int blocks, long range) {
	// blocks == 1: ptr[rows + 1]; otherwise the (rows, blocks + 1) boundary array of k_sp_boundaries.  Every range inside [0, nnz], every index inside [0, range)
	const int per_row = blocks > 1 ? blocks + 1 : 1;
	const long count = blocks > 1 ? (long)rows * per_row : (long)rows + 1;
	for (long i = 0; i < count; ++i)
		if (ptr[i] < 0 || ptr[i] > nnz) return false;
	for (int row = 0; row < rows; ++row)
		for (int b = 0; b < (blocks > 1 ? blocks : 1); ++b)
			if (ptr[(long)row * per_row + b] > ptr[(long)row * per_row + b + 1]) return false;
	for (long p = 0; p < nnz; ++p)
		if (idx[p] < 0 || idx[p] >= range) return false;
	return true;
}

template <typename T>
hipError_t upload(DevBuf& d, const T* src, size_t count) {
	if (hipError_t e = d.alloc(sizeof(T) * count); e != hipSuccess) return e;
	return count ? hipMemcpy(d.p, src, sizeof(T) * count, hipMemcpyHostToDevice) : hipSuccess;
}

inline int op_status(hipError_t launch) {
	if (launch == hipErrorInvalidValue) return NMFAMD_INVALID_ARGUMENT;
	return launch == hipSuccess && hipDeviceSynchronize() == hipSuccess ? NMFAMD_OK : NMFAMD_HIP_ERROR;
}

template <typename T>
int op_kl_fused(const int* ptr, const int* idx, const T* val, long nnz, const T* A, const T* B, long b_rows, int RP, int rows, int rows_pad, int blocks, const T* a_scale,
                T* out, T* t_vwh, T* t_kl) {
	if (!ptr || !idx || !val || !A || !B || !out || (t_vwh == nullptr) != (t_kl == nullptr) || nnz < 0 || nnz > 0x7fffffffl || b_rows < 1 || RP < 64 || RP > 4096 ||
	    RP % 64 != 0 || rows < 1 || rows > rows_pad || blocks < 1 || blocks > 64 || !sparse_image_ok(ptr, idx, nnz, rows, blocks, b_rows))
		return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	const size_t panel = (size_t)rows_pad * RP, np = blocks > 1 ? (size_t)rows * (blocks + 1) : (size_t)rows + 1, nt = (size_t)blocks * rows_pad;
	DevBuf dPtr, dIdx, dVal, dA, dB, dS, dOut, dTv, dTk;
	if (upload(dPtr, ptr, np) != hipSuccess || upload(dIdx, idx, (size_t)nnz) != hipSuccess || upload(dVal, val, (size_t)nnz) != hipSuccess || upload(dA, A, panel) != hipSuccess ||
	    upload(dB, B, (size_t)b_rows * RP) != hipSuccess || upload(dOut, out, panel * blocks) != hipSuccess || (a_scale && upload(dS, a_scale, (size_t)RP) != hipSuccess) ||
	    (t_vwh && (upload(dTv, t_vwh, nt) != hipSuccess || upload(dTk, t_kl, nt) != hipSuccess)))
		return NMFAMD_NO_DEVICE_MEMORY;
	const int st = op_status(launch_kl_fused<T>((const int*)dPtr.p, (const int*)dIdx.p, (const T*)dVal.p, (const T*)dA.p, (const T*)dB.p, RP, std::numeric_limits<T>::epsilon(),
	                                            (T*)dOut.p, (T*)dTv.p, (T*)dTk.p, rows, rows_pad, nullptr, blocks, blocks > 1 ? (long)panel : 0, (const T*)dS.p));
	if (st != NMFAMD_OK) return st;
	if (hipMemcpy(out, dOut.p, sizeof(T) * panel * blocks, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (t_vwh && (hipMemcpy(t_vwh, dTv.p, sizeof(T) * nt, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(t_kl, dTk.p, sizeof(T) * nt, hipMemcpyDeviceToHost) != hipSuccess))
		return NMFAMD_HIP_ERROR;
	return NMFAMD_OK;
}

// One launch of the masked beta-divergence half-step (kernels_masked_beta.hip) on a caller-built image and caller-built padded panels.  divergence / beta select the
// map as nmfamd_params_v7 does (1 KL, 2 Itakura-Saito, 3 beta -- where 0 and 1 run the maps of 2 and 1).  A [a_rows][RP] comes back as the launch left it; t_frob /
// t_div [rows] and sumsq_part [masked_norm_parts(rows)][RP] are uploaded as the caller filled them.
template <typename T>
int op_masked_beta_half_step(const int* ptr, const int* idx, const T* val, long nnz, T* A, long a_rows, const T* B, long b_rows, int RP, int rows, int divergence, double beta,
                             double l1, double l2, int update, T* t_frob, T* t_div, T* sumsq_part, int sumsq_parts) {
	if (!ptr || !idx || !val || !A || !B || nnz < 0 || nnz > 0x7fffffffl || b_rows < 1 || rows < 1 || a_rows < rows || (RP != 64 && RP != 128 && RP != 256) ||
	    divergence < 1 || divergence > 3 || (divergence != 3 && beta != 0) || (t_frob == nullptr) != (t_div == nullptr) ||
	    (sumsq_part != nullptr && sumsq_parts != masked_norm_parts(rows)) || !sparse_image_ok(ptr, idx, nnz, rows, 1, b_rows))
		return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	const double b = divergence == 2 ? 0.0 : divergence == 3 ? beta : 1.0;
	const size_t panel = (size_t)a_rows * RP, ns = (size_t)(sumsq_part ? sumsq_parts : 0) * RP;
	DevBuf dPtr, dIdx, dVal, dA, dB, dTf, dTd, dSq;
	if (upload(dPtr, ptr, (size_t)rows + 1) != hipSuccess || upload(dIdx, idx, (size_t)nnz) != hipSuccess || upload(dVal, val, (size_t)nnz) != hipSuccess ||
	    upload(dA, A, panel) != hipSuccess || upload(dB, B, (size_t)b_rows * RP) != hipSuccess ||
	    (t_frob && (upload(dTf, t_frob, (size_t)rows) != hipSuccess || upload(dTd, t_div, (size_t)rows) != hipSuccess)) || (sumsq_part && upload(dSq, sumsq_part, ns) != hipSuccess))
		return NMFAMD_NO_DEVICE_MEMORY;
	const int st = op_status(launch_masked_beta_half_step<T>((const int*)dPtr.p, (const int*)dIdx.p, (const T*)dVal.p, (T*)dA.p, (const T*)dB.p, RP, std::numeric_limits<T>::epsilon(),
	                                                         b, (T)l1, (T)l2, update != 0, (T*)dTf.p, (T*)dTd.p, (T*)dSq.p, rows, nullptr));
	if (st != NMFAMD_OK) return st;
	if (hipMemcpy(A, dA.p, sizeof(T) * panel, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (t_frob && (hipMemcpy(t_frob, dTf.p, sizeof(T) * rows, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(t_div, dTd.p, sizeof(T) * rows, hipMemcpyDeviceToHost) != hipSuccess))
		return NMFAMD_HIP_ERROR;
	if (sumsq_part && hipMemcpy(sumsq_part, dSq.p, sizeof(T) * ns, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	return NMFAMD_OK;
}

// One launch of the coordinate-descent half-step over the observed entries (kernels_masked_cd.hip) on a caller-built image and caller-built padded panels.  A
// [a_rows][RP] comes back as the launch left it; G_out / c_out (both or neither) receive the normal equations of every row.
template <typename T>
int op_masked_cd_half_step(const int* ptr, const int* idx, const T* val, long nnz, T* A, long a_rows, const T* B, long b_rows, int RP, int r, int rows, int sweeps, double l1,
                           double l2, T* G_out, T* c_out) {
	if (!ptr || !idx || !val || !A || !B || nnz < 0 || nnz > 0x7fffffffl || b_rows < 1 || rows < 1 || a_rows < rows || !masked_cd_rank_instantiated(RP) || r < 1 || r > RP ||
	    (G_out == nullptr) != (c_out == nullptr) || !sparse_image_ok(ptr, idx, nnz, rows, 1, b_rows))
		return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	const size_t panel = (size_t)a_rows * RP, ng = G_out ? (size_t)rows * RP * RP : 0, nc = G_out ? (size_t)rows * RP : 0;
	DevBuf dPtr, dIdx, dVal, dA, dB, dG, dC;
	if (upload(dPtr, ptr, (size_t)rows + 1) != hipSuccess || upload(dIdx, idx, (size_t)nnz) != hipSuccess || upload(dVal, val, (size_t)nnz) != hipSuccess ||
	    upload(dA, A, panel) != hipSuccess || upload(dB, B, (size_t)b_rows * RP) != hipSuccess || (G_out && (upload(dG, G_out, ng) != hipSuccess || upload(dC, c_out, nc) != hipSuccess)))
		return NMFAMD_NO_DEVICE_MEMORY;
	const int st = op_status(launch_masked_cd_half_step<T>((const int*)dPtr.p, (const int*)dIdx.p, (const T*)dVal.p, (T*)dA.p, (const T*)dB.p, RP, r, rows, sweeps, (T)l1, (T)l2,
	                                                       (T*)dG.p, (T*)dC.p, nullptr));
	if (st != NMFAMD_OK) return st;
	if (hipMemcpy(A, dA.p, sizeof(T) * panel, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (G_out && (hipMemcpy(G_out, dG.p, sizeof(T) * ng, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(c_out, dC.p, sizeof(T) * nc, hipMemcpyDeviceToHost) != hipSuccess))
		return NMFAMD_HIP_ERROR;
	return NMFAMD_OK;
}

// One launch of the gather of kernels_predict.hip on caller-built padded panels (docs/PREDICT.md).  Every coordinate is checked here, on the host: the kernel
// checks none.  out and part are uploaded as the caller filled them.
template <typename T>
int op_predict_entries(const int* rows, const int* cols, const T* vals, long nnz, int base, const T* Wt, long w_rows, const T* H, long h_rows, int RP, int r, double beta,
                       T* out, long out_len, double* part, int parts) {
	if (!rows || !cols || !Wt || !H || nnz < 1 || nnz > PREDICT_MAX_ENTRIES || (base != 0 && base != 1) || w_rows < 1 || h_rows < 1 ||
	    !predict_rank_instantiated(RP, sizeof(T)) || r < 1 || r > RP || (!vals && !out) || (out && out_len < nnz) || (vals != nullptr) != (part != nullptr) ||
	    (part && parts != predict_entry_parts(nnz)) || (vals && std::isinf((double)(T)beta)))
		return NMFAMD_INVALID_ARGUMENT;
	for (long p = 0; p < nnz; ++p) {
		const long i = (long)rows[p] - base, j = (long)cols[p] - base;
		if (i < 0 || i >= w_rows || j < 0 || j >= h_rows) return NMFAMD_INVALID_ARGUMENT;
	}
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	DevBuf dR, dC, dV, dW, dH, dO, dP;
	if (upload(dR, rows, (size_t)nnz) != hipSuccess || upload(dC, cols, (size_t)nnz) != hipSuccess || (vals && upload(dV, vals, (size_t)nnz) != hipSuccess) ||
	    upload(dW, Wt, (size_t)w_rows * RP) != hipSuccess || upload(dH, H, (size_t)h_rows * RP) != hipSuccess || (out && upload(dO, out, (size_t)out_len) != hipSuccess) ||
	    (part && upload(dP, part, (size_t)parts * 3) != hipSuccess))
		return NMFAMD_NO_DEVICE_MEMORY;
	const int st = op_status(launch_predict_entries<T>((const int*)dR.p, (const int*)dC.p, (const T*)dV.p, nnz, base, (const T*)dW.p, (const T*)dH.p, RP, r,
	                                                   std::numeric_limits<T>::epsilon(), beta, (T*)dO.p, (double*)dP.p, nullptr));
	if (st != NMFAMD_OK) return st;
	if (out && hipMemcpy(out, dO.p, sizeof(T) * (size_t)out_len, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (part && hipMemcpy(part, dP.p, sizeof(double) * (size_t)parts * 3, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	return NMFAMD_OK;
}

// The two launches of kernels_topk.hip on caller-built padded panels (docs/TOPK.md).  Every index is checked here, on the host: the kernels check none.
template <typename T>
int op_top_k(const int* queries, long nq, int k, int base, const T* A, long a_rows, const T* B, long b_rows, long count, int RP, int r, const long* excl_ptr,
             const int* excl_idx, int slabs, int* out_idx, T* out_scores) {
	if (!queries || !A || !B || !out_idx || !out_scores || nq < 1 || nq > TOPK_MAX_QUERIES || k < 1 || k > TOPK_MAX_K || (base != 0 && base != 1) || a_rows < 1 ||
	    b_rows < 1 || count < 1 || count > b_rows || count > TOPK_MAX_CANDIDATES || !predict_rank_instantiated(RP, sizeof(T)) || r < 1 || r > RP || slabs < 0 ||
	    slabs > TOPK_MAX_SLABS || (!excl_ptr && excl_idx))
		return NMFAMD_INVALID_ARGUMENT;
	for (long q = 0; q < nq; ++q) {
		const long i = (long)queries[q] - base;
		if (i < 0 || i >= a_rows) return NMFAMD_INVALID_ARGUMENT;
	}
	long excl_nnz = 0;
	if (excl_ptr) {
		if (excl_ptr[0] != 0) return NMFAMD_INVALID_ARGUMENT;
		for (long q = 1; q <= nq; ++q)
			if (excl_ptr[q] < excl_ptr[q - 1]) return NMFAMD_INVALID_ARGUMENT;
		excl_nnz = excl_ptr[nq];
		if (excl_nnz > 0 && !excl_idx) return NMFAMD_INVALID_ARGUMENT;
		for (long e = 0; e < excl_nnz; ++e) {
			const long c = (long)excl_idx[e] - base;
			if (c < 0 || c >= count) return NMFAMD_INVALID_ARGUMENT;
		}
	}
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	const size_t part = (size_t)nq * (size_t)(slabs > 0 ? slabs : topk_slabs(nq, count)) * k, outs = (size_t)nq * k;
	DevBuf dQ, dA, dB, dP, dE, dPs, dPi, dOi, dOs;
	if (upload(dQ, queries, (size_t)nq) != hipSuccess || upload(dA, A, (size_t)a_rows * RP) != hipSuccess || upload(dB, B, (size_t)b_rows * RP) != hipSuccess ||
	    (excl_nnz > 0 && (upload(dP, excl_ptr, (size_t)nq + 1) != hipSuccess || upload(dE, excl_idx, (size_t)excl_nnz) != hipSuccess)) ||
	    dPs.alloc(sizeof(T) * part) != hipSuccess || dPi.alloc(sizeof(int) * part) != hipSuccess || dOi.alloc(sizeof(int) * outs) != hipSuccess ||
	    dOs.alloc(sizeof(T) * outs) != hipSuccess)
		return NMFAMD_NO_DEVICE_MEMORY;
	const int st = op_status(launch_topk<T>((const int*)dQ.p, nq, k, base, (const T*)dA.p, (const T*)dB.p, count, RP, r, (const long*)dP.p, (const int*)dE.p, slabs,
	                                        (T*)dPs.p, (int*)dPi.p, (int*)dOi.p, (T*)dOs.p, nullptr));
	if (st != NMFAMD_OK) return st;
	if (hipMemcpy(out_idx, dOi.p, sizeof(int) * outs, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(out_scores, dOs.p, sizeof(T) * outs, hipMemcpyDeviceToHost) != hipSuccess)
		return NMFAMD_HIP_ERROR;
	return NMFAMD_OK;
}

template <typename T>
int op_kl_update(T* P, const T* num, int parts, long part_stride, const T* den, const T* scale, int RP, int len_pad, T* sumsq_part, T* sum_part) {
	// num: `parts` panels of len_pad * RP values, part_stride values apart (what lies between them is uploaded too, and must not be read)
	if (!P || !num || !den || RP < 4 || RP > 4096 || RP % 4 != 0 || len_pad < 128 || len_pad % 128 != 0 || parts < 1 || parts > 4096 || part_stride % 4 != 0 ||
	    (parts > 1 && part_stride < (long)len_pad * RP) || part_stride < 0)
		return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	const size_t panel = (size_t)len_pad * RP, all_num = (size_t)(parts - 1) * (size_t)part_stride + panel, ns = (size_t)(len_pad / 128) * RP;
	DevBuf dP, dNum, dDen, dSc, dSq, dSm;
	if (upload(dP, P, panel) != hipSuccess || upload(dNum, num, all_num) != hipSuccess || upload(dDen, den, (size_t)RP) != hipSuccess ||
	    (scale && upload(dSc, scale, (size_t)RP) != hipSuccess) || (sumsq_part && upload(dSq, sumsq_part, ns) != hipSuccess) || (sum_part && upload(dSm, sum_part, ns) != hipSuccess))
		return NMFAMD_NO_DEVICE_MEMORY;
	const int st = op_status(launch_kl_update<T>((T*)dP.p, (const T*)dNum.p, (const T*)dDen.p, RP, len_pad, std::numeric_limits<T>::epsilon(), (T*)dSq.p, nullptr, parts, part_stride,
	                                             (T*)dSm.p, (const T*)dSc.p));
	if (st != NMFAMD_OK) return st;
	if (hipMemcpy(P, dP.p, sizeof(T) * panel, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (sumsq_part && hipMemcpy(sumsq_part, dSq.p, sizeof(T) * ns, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (sum_part && hipMemcpy(sum_part, dSm.p, sizeof(T) * ns, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	return NMFAMD_OK;
}

template <typename T>
int op_kl_sums(const T* sum_part, const T* sumsq_part, int parts, int RP, T* sums, T* scale) {
	if (!sum_part || !sums || parts < 1 || RP < 16 || RP > 4096 || RP % 16 != 0) return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	const size_t np = (size_t)parts * RP;
	DevBuf dA, dB, dS, dSc;
	if (upload(dA, sum_part, np) != hipSuccess || (sumsq_part && upload(dB, sumsq_part, np) != hipSuccess) || upload(dS, sums, (size_t)RP) != hipSuccess ||
	    (scale && upload(dSc, scale, (size_t)RP) != hipSuccess))
		return NMFAMD_NO_DEVICE_MEMORY;
	const int st = op_status(launch_kl_sums<T>((const T*)dA.p, (const T*)dB.p, parts, RP, (T*)dS.p, nullptr, (T*)dSc.p));
	if (st != NMFAMD_OK) return st;
	if (hipMemcpy(sums, dS.p, sizeof(T) * RP, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (scale && hipMemcpy(scale, dSc.p, sizeof(T) * RP, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	return NMFAMD_OK;
}

template <typename T>
int op_panel_rowsum(const T* P, int RP, int len_pad, T* sums) {
	if (!P || !sums || RP < 1 || RP > 4096 || len_pad < 128 || len_pad % 128 != 0) return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	DevBuf dP, dPart, dS;
	if (upload(dP, P, (size_t)len_pad * RP) != hipSuccess || dPart.alloc(sizeof(T) * (size_t)(len_pad / 128) * RP) != hipSuccess || upload(dS, sums, (size_t)RP) != hipSuccess)
		return NMFAMD_NO_DEVICE_MEMORY;
	const int st = op_status(launch_panel_rowsum<T>((const T*)dP.p, RP, len_pad, (T*)dPart.p, (T*)dS.p, nullptr));
	if (st != NMFAMD_OK) return st;
	return hipMemcpy(sums, dS.p, sizeof(T) * RP, hipMemcpyDeviceToHost) == hipSuccess ? NMFAMD_OK : NMFAMD_HIP_ERROR;
}

template <typename T>
int op_spmm_rows(const int* ptr, const int* idx, const T* val, long nnz, const T* P, long p_rows, int RP, int rows, int rows_pad, T* out) {
	if (!ptr || !idx || !val || !P || !out || nnz < 0 || nnz > 0x7fffffffl || p_rows < 1 || RP < 64 || RP > 4096 || RP % 64 != 0 || rows < 1 || rows > rows_pad ||
	    !sparse_image_ok(ptr, idx, nnz, rows, 1, p_rows))
		return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	const size_t panel = (size_t)rows_pad * RP;
	DevBuf dPtr, dIdx, dVal, dP, dOut;
	if (upload(dPtr, ptr, (size_t)rows + 1) != hipSuccess || upload(dIdx, idx, (size_t)nnz) != hipSuccess || upload(dVal, val, (size_t)nnz) != hipSuccess ||
	    upload(dP, P, (size_t)p_rows * RP) != hipSuccess || upload(dOut, out, panel) != hipSuccess)
		return NMFAMD_NO_DEVICE_MEMORY;
	const int st = op_status(launch_spmm_rows<T>((const int*)dPtr.p, (const int*)dIdx.p, (const T*)dVal.p, (const T*)dP.p, RP, (T*)dOut.p, rows, rows_pad, nullptr));
	if (st != NMFAMD_OK) return st;
	return hipMemcpy(out, dOut.p, sizeof(T) * panel, hipMemcpyDeviceToHost) == hipSuccess ? NMFAMD_OK : NMFAMD_HIP_ERROR;
}

template <typename T>
int op_sddmm_quotient(const int* ptr, const int* idx, const T* val, long nnz, const T* A, const T* B, long b_rows, int RP, int rows, T* q, T* t_vwh, T* t_kl) {
	if (!ptr || !idx || !val || !A || !B || !q || (t_vwh == nullptr) != (t_kl == nullptr) || nnz < 0 || nnz > 0x7fffffffl || b_rows < 1 || RP < 64 || RP > 4096 ||
	    RP % 64 != 0 || rows < 1 || !sparse_image_ok(ptr, idx, nnz, rows, 1, b_rows))
		return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	DevBuf dPtr, dIdx, dVal, dA, dB, dQ, dTv, dTk;
	if (upload(dPtr, ptr, (size_t)rows + 1) != hipSuccess || upload(dIdx, idx, (size_t)nnz) != hipSuccess || upload(dVal, val, (size_t)nnz) != hipSuccess ||
	    upload(dA, A, (size_t)rows * RP) != hipSuccess || upload(dB, B, (size_t)b_rows * RP) != hipSuccess || upload(dQ, q, (size_t)nnz) != hipSuccess ||
	    (t_vwh && (upload(dTv, t_vwh, (size_t)rows) != hipSuccess || upload(dTk, t_kl, (size_t)rows) != hipSuccess)))
		return NMFAMD_NO_DEVICE_MEMORY;
	const int st = op_status(launch_sddmm_quotient<T>((const int*)dPtr.p, (const int*)dIdx.p, (const T*)dVal.p, (const T*)dA.p, (const T*)dB.p, RP, std::numeric_limits<T>::epsilon(),
	                                                  (T*)dQ.p, (T*)dTv.p, (T*)dTk.p, rows, nullptr));
	if (st != NMFAMD_OK) return st;
	if (nnz > 0 && hipMemcpy(q, dQ.p, sizeof(T) * (size_t)nnz, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
	if (t_vwh && (hipMemcpy(t_vwh, dTv.p, sizeof(T) * (size_t)rows, hipMemcpyDeviceToHost) != hipSuccess ||
	              hipMemcpy(t_kl, dTk.p, sizeof(T) * (size_t)rows, hipMemcpyDeviceToHost) != hipSuccess)) return NMFAMD_HIP_ERROR;
	return NMFAMD_OK;
}
}

extern "C" {

int nmfamd_op_beta_update_rows_f32(float* P, float* Aacc, float* Bacc, const float* num_part, const float* den_part, int slabs, const float* dsum, int RP, int r, int out_pad,
                                   int out_valid, double beta, double l1, double l2, int online, double rho, int flush, float* sum_part) {
	return op_beta_update_rows<float>(P, Aacc, Bacc, num_part, den_part, slabs, dsum, RP, r, out_pad, out_valid, beta, l1, l2, online, rho, flush, sum_part);
}

int nmfamd_op_beta_update_rows_f64(double* P, double* Aacc, double* Bacc, const double* num_part, const double* den_part, int slabs, const double* dsum, int RP, int r,
                                   int out_pad, int out_valid, double beta, double l1, double l2, int online, double rho, int flush, double* sum_part) {
	return op_beta_update_rows<double>(P, Aacc, Bacc, num_part, den_part, slabs, dsum, RP, r, out_pad, out_valid, beta, l1, l2, online, rho, flush, sum_part);
}

int nmfamd_op_beta_fused_f32(const float* A, const float* B, const float* X, const float* Omega, long ldx, int RP, int out_pad, int out_valid, int red_pad, int red_valid,
                             double beta, int update, int terms, int mixed, int force_slabs, float* num_part, float* den_part, float* tf_part, float* td_part, int* plan) {
	return op_beta_fused<float>(A, B, X, Omega, ldx, RP, out_pad, out_valid, red_pad, red_valid, beta, update, terms, mixed, force_slabs, num_part, den_part, tf_part, td_part, plan);
}

int nmfamd_op_beta_fused_f64(const double* A, const double* B, const double* X, const double* Omega, long ldx, int RP, int out_pad, int out_valid, int red_pad, int red_valid,
                             double beta, int update, int terms, int mixed, int force_slabs, double* num_part, double* den_part, double* tf_part, double* td_part, int* plan) {
	return op_beta_fused<double>(A, B, X, Omega, ldx, RP, out_pad, out_valid, red_pad, red_valid, beta, update, terms, mixed, force_slabs, num_part, den_part, tf_part, td_part, plan);
}

int nmfamd_op_beta_update_f32(float* P, const float* num_part, const float* den_part, int slabs, const float* dsum, int RP, int r, int out_pad, int out_valid, double beta,
                              double l1, double l2, int weighted, int update, const float* tf_part, const float* td_part, float* sumsq_part, float* sum_part, float* t_frob,
                              float* t_div) {
	return op_beta_update<float>(P, num_part, den_part, slabs, dsum, RP, r, out_pad, out_valid, beta, l1, l2, weighted, update, tf_part, td_part, sumsq_part, sum_part, t_frob, t_div);
}

int nmfamd_op_beta_update_f64(double* P, const double* num_part, const double* den_part, int slabs, const double* dsum, int RP, int r, int out_pad, int out_valid, double beta,
                              double l1, double l2, int weighted, int update, const double* tf_part, const double* td_part, double* sumsq_part, double* sum_part, double* t_frob,
                              double* t_div) {
	return op_beta_update<double>(P, num_part, den_part, slabs, dsum, RP, r, out_pad, out_valid, beta, l1, l2, weighted, update, tf_part, td_part, sumsq_part, sum_part, t_frob, t_div);
}

int nmfamd_op_beta_half_step_f32(float* A, const float* B, const float* X, long ldx, int RP, int r, int out_pad, int out_valid, int red_pad, int red_valid, int beta,
                                 int form, int force_slabs, const float* dsum, float* t_frob, float* t_div, float* sumsq_part, float* sum_part, int* slabs) {
	if (beta != 0 && beta != 1) return NMFAMD_INVALID_ARGUMENT;
	return op_beta_half_step<float>(A, B, X, ldx, RP, r, out_pad, out_valid, red_pad, red_valid, (double)beta, 0.0, 0.0, form, force_slabs, dsum, t_frob, t_div, sumsq_part, sum_part, slabs);
}

int nmfamd_op_beta_half_step_f64(double* A, const double* B, const double* X, long ldx, int RP, int r, int out_pad, int out_valid, int red_pad, int red_valid, int beta,
                                 int form, int force_slabs, const double* dsum, double* t_frob, double* t_div, double* sumsq_part, double* sum_part, int* slabs) {
	if (beta != 0 && beta != 1) return NMFAMD_INVALID_ARGUMENT;
	return op_beta_half_step<double>(A, B, X, ldx, RP, r, out_pad, out_valid, red_pad, red_valid, (double)beta, 0.0, 0.0, form, force_slabs, dsum, t_frob, t_div, sumsq_part, sum_part, slabs);
}

int nmfamd_op_beta_half_step_general_f32(float* A, const float* B, const float* X, long ldx, int RP, int r, int out_pad, int out_valid, int red_pad, int red_valid,
                                         double beta, double l1, double l2, int form, int force_slabs, const float* dsum, float* t_frob, float* t_div,
                                         float* sumsq_part, float* sum_part, int* slabs) {
	return op_beta_half_step<float>(A, B, X, ldx, RP, r, out_pad, out_valid, red_pad, red_valid, beta, l1, l2, form, force_slabs, dsum, t_frob, t_div, sumsq_part, sum_part, slabs);
}

int nmfamd_op_beta_half_step_general_f64(double* A, const double* B, const double* X, long ldx, int RP, int r, int out_pad, int out_valid, int red_pad, int red_valid,
                                         double beta, double l1, double l2, int form, int force_slabs, const double* dsum, double* t_frob, double* t_div,
                                         double* sumsq_part, double* sum_part, int* slabs) {
	return op_beta_half_step<double>(A, B, X, ldx, RP, r, out_pad, out_valid, red_pad, red_valid, beta, l1, l2, form, force_slabs, dsum, t_frob, t_div, sumsq_part, sum_part, slabs);
}

int nmfamd_op_beta_half_step_mixed_f32(float* A, const float* B, const float* X, long ldx, int RP, int r, int out_pad, int out_valid, int red_pad, int red_valid,
                                       double beta, double l1, double l2, int form, int force_slabs, const float* dsum, float* t_frob, float* t_div,
                                       float* sumsq_part, float* sum_part, int* slabs) {
	return op_beta_half_step<float>(A, B, X, ldx, RP, r, out_pad, out_valid, red_pad, red_valid, beta, l1, l2, form, force_slabs, dsum, t_frob, t_div, sumsq_part, sum_part, slabs,
	                                nullptr, false, true);
}

int nmfamd_op_beta_half_step_weighted_f32(float* A, const float* B, const float* X, const float* Omega, long ldx, int RP, int r, int out_pad, int out_valid, int red_pad,
                                          int red_valid, double beta, double l1, double l2, int form, int force_slabs, const float* dsum, float* t_frob, float* t_div,
                                          float* sumsq_part, float* sum_part, int* slabs) {
	return op_beta_half_step<float>(A, B, X, ldx, RP, r, out_pad, out_valid, red_pad, red_valid, beta, l1, l2, form, force_slabs, dsum, t_frob, t_div, sumsq_part, sum_part, slabs,
	                                Omega, true);
}

int nmfamd_op_beta_half_step_weighted_f64(double* A, const double* B, const double* X, const double* Omega, long ldx, int RP, int r, int out_pad, int out_valid, int red_pad,
                                          int red_valid, double beta, double l1, double l2, int form, int force_slabs, const double* dsum, double* t_frob, double* t_div,
                                          double* sumsq_part, double* sum_part, int* slabs) {
	return op_beta_half_step<double>(A, B, X, ldx, RP, r, out_pad, out_valid, red_pad, red_valid, beta, l1, l2, form, force_slabs, dsum, t_frob, t_div, sumsq_part, sum_part, slabs,
	                                 Omega, true);
}

int nmfamd_op_hals_sweep_f32(float* P, const float* slabs, int S, long slab_stride, const float* G, int RP, int r, int len_pad, int len_valid, float* ps,
                             float* sumsq_part, int* parts) {
	return op_hals_sweep<float>(P, slabs, S, slab_stride, G, RP, r, len_pad, len_valid, ps, sumsq_part, parts);
}

int nmfamd_op_hals_sweep_f64(double* P, const double* slabs, int S, long slab_stride, const double* G, int RP, int r, int len_pad, int len_valid, double* ps,
                             double* sumsq_part, int* parts) {
	return op_hals_sweep<double>(P, slabs, S, slab_stride, G, RP, r, len_pad, len_valid, ps, sumsq_part, parts);
}

int nmfamd_op_hals_sweep_pen_f32(float* P, const float* slabs, int S, long slab_stride, const float* G, int RP, int r, int len_pad, int len_valid, float* ps,
                                 float* sumsq_part, int* parts, float l1, float l2) {
	return op_hals_sweep<float>(P, slabs, S, slab_stride, G, RP, r, len_pad, len_valid, ps, sumsq_part, parts, l1, l2);
}

int nmfamd_op_hals_sweep_pen_f64(double* P, const double* slabs, int S, long slab_stride, const double* G, int RP, int r, int len_pad, int len_valid, double* ps,
                                 double* sumsq_part, int* parts, double l1, double l2) {
	return op_hals_sweep<double>(P, slabs, S, slab_stride, G, RP, r, len_pad, len_valid, ps, sumsq_part, parts, l1, l2);
}

int nmfamd_op_hals_sweeps_f32(float* P, const float* slabs, int S, long slab_stride, const float* G, int RP, int r, int len_pad, int len_valid, float* ps,
                              float* sumsq_part, int* parts, float l1, float l2, int sweeps) {
	if (sweeps == 0) return NMFAMD_INVALID_ARGUMENT;      // (0 is op_hals_sweep's own mark for the single-sweep launcher)
	return op_hals_sweep<float>(P, slabs, S, slab_stride, G, RP, r, len_pad, len_valid, ps, sumsq_part, parts, l1, l2, sweeps);
}

int nmfamd_op_hals_sweeps_f64(double* P, const double* slabs, int S, long slab_stride, const double* G, int RP, int r, int len_pad, int len_valid, double* ps,
                              double* sumsq_part, int* parts, double l1, double l2, int sweeps) {
	if (sweeps == 0) return NMFAMD_INVALID_ARGUMENT;
	return op_hals_sweep<double>(P, slabs, S, slab_stride, G, RP, r, len_pad, len_valid, ps, sumsq_part, parts, l1, l2, sweeps);
}

int nmfamd_op_hals_sweeps_dyn_f32(float* P, const float* slabs, int S, long slab_stride, const float* G, int RP, int r, int len_pad, int len_valid, float* ps,
                                  float* sumsq_part, int* parts, float l1, float l2, int sweeps, double tol, int* counts) {
	return op_hals_sweep<float>(P, slabs, S, slab_stride, G, RP, r, len_pad, len_valid, ps, sumsq_part, parts, l1, l2, sweeps, true, tol, counts);
}

int nmfamd_op_hals_sweeps_dyn_f64(double* P, const double* slabs, int S, long slab_stride, const double* G, int RP, int r, int len_pad, int len_valid, double* ps,
                                  double* sumsq_part, int* parts, double l1, double l2, int sweeps, double tol, int* counts) {
	return op_hals_sweep<double>(P, slabs, S, slab_stride, G, RP, r, len_pad, len_valid, ps, sumsq_part, parts, l1, l2, sweeps, true, tol, counts);
}

int nmfamd_op_apg_steps_f32(float* P, const float* slabs, int S, long slab_stride, const float* G, int RP, int r, int len_pad, int len_valid, float* ps,
                            float* sumsq_part, int* parts, float l1, float l2, int steps) {
	return op_hals_sweep<float>(P, slabs, S, slab_stride, G, RP, r, len_pad, len_valid, ps, sumsq_part, parts, l1, l2, steps, false, 0, nullptr, true);
}

int nmfamd_op_apg_steps_f64(double* P, const double* slabs, int S, long slab_stride, const double* G, int RP, int r, int len_pad, int len_valid, double* ps,
                            double* sumsq_part, int* parts, double l1, double l2, int steps) {
	return op_hals_sweep<double>(P, slabs, S, slab_stride, G, RP, r, len_pad, len_valid, ps, sumsq_part, parts, l1, l2, steps, false, 0, nullptr, true);
}

int nmfamd_op_apg_steps_dyn_f32(float* P, const float* slabs, int S, long slab_stride, const float* G, int RP, int r, int len_pad, int len_valid, float* ps,
                                float* sumsq_part, int* parts, float l1, float l2, int steps, float tol, int* counts) {
	return op_hals_sweep<float>(P, slabs, S, slab_stride, G, RP, r, len_pad, len_valid, ps, sumsq_part, parts, l1, l2, steps, true, tol, counts, true);
}

int nmfamd_op_apg_steps_dyn_f64(double* P, const double* slabs, int S, long slab_stride, const double* G, int RP, int r, int len_pad, int len_valid, double* ps,
                                double* sumsq_part, int* parts, double l1, double l2, int steps, double tol, int* counts) {
	return op_hals_sweep<double>(P, slabs, S, slab_stride, G, RP, r, len_pad, len_valid, ps, sumsq_part, parts, l1, l2, steps, true, tol, counts, true);
}

int nmfamd_op_hals_normalize_f32(float* Wt, int RP, int mpad, float* H, int npad, const float* sumsq_part, int parts) {
	return op_hals_normalize<float>(Wt, RP, mpad, H, npad, sumsq_part, parts);
}

int nmfamd_op_hals_normalize_f64(double* Wt, int RP, int mpad, double* H, int npad, const double* sumsq_part, int parts) {
	return op_hals_normalize<double>(Wt, RP, mpad, H, npad, sumsq_part, parts);
}

int nmfamd_masked_norm_parts(int rows) { return rows > 0 ? masked_norm_parts(rows) : 0; }

int nmfamd_predict_entry_parts(long nnz) { return nnz > 0 ? predict_entry_parts(nnz) : 0; }

int nmfamd_top_k_max(void) { return TOPK_MAX_K; }
int nmfamd_top_k_slabs(long nq, long count) { return topk_slabs(nq, count); }

int nmfamd_op_top_k_f32(const int* queries, long nq, int k, int base, const float* A, long a_rows, const float* B, long b_rows, long count, int RP, int r,
                        const long* excl_ptr, const int* excl_idx, int slabs, int* out_idx, float* out_scores) {
	return op_top_k<float>(queries, nq, k, base, A, a_rows, B, b_rows, count, RP, r, excl_ptr, excl_idx, slabs, out_idx, out_scores);
}

int nmfamd_op_top_k_f64(const int* queries, long nq, int k, int base, const double* A, long a_rows, const double* B, long b_rows, long count, int RP, int r,
                        const long* excl_ptr, const int* excl_idx, int slabs, int* out_idx, double* out_scores) {
	return op_top_k<double>(queries, nq, k, base, A, a_rows, B, b_rows, count, RP, r, excl_ptr, excl_idx, slabs, out_idx, out_scores);
}

int nmfamd_op_predict_entries_f32(const int* rows, const int* cols, const float* vals, long nnz, int base, const float* Wt, long w_rows, const float* H, long h_rows, int RP,
                                  int r, double beta, float* out, long out_len, double* part, int parts) {
	return op_predict_entries<float>(rows, cols, vals, nnz, base, Wt, w_rows, H, h_rows, RP, r, beta, out, out_len, part, parts);
}

int nmfamd_op_predict_entries_f64(const int* rows, const int* cols, const double* vals, long nnz, int base, const double* Wt, long w_rows, const double* H, long h_rows, int RP,
                                  int r, double beta, double* out, long out_len, double* part, int parts) {
	return op_predict_entries<double>(rows, cols, vals, nnz, base, Wt, w_rows, H, h_rows, RP, r, beta, out, out_len, part, parts);
}

int nmfamd_op_masked_cd_half_step_f32(const int* ptr, const int* idx, const float* val, long nnz, float* A, long a_rows, const float* B, long b_rows, int RP, int r, int rows,
                                      int sweeps, double l1, double l2, float* G_out, float* c_out) {
	return op_masked_cd_half_step<float>(ptr, idx, val, nnz, A, a_rows, B, b_rows, RP, r, rows, sweeps, l1, l2, G_out, c_out);
}

int nmfamd_op_masked_cd_half_step_f64(const int* ptr, const int* idx, const double* val, long nnz, double* A, long a_rows, const double* B, long b_rows, int RP, int r, int rows,
                                      int sweeps, double l1, double l2, double* G_out, double* c_out) {
	return op_masked_cd_half_step<double>(ptr, idx, val, nnz, A, a_rows, B, b_rows, RP, r, rows, sweeps, l1, l2, G_out, c_out);
}

int nmfamd_op_masked_beta_half_step_f32(const int* ptr, const int* idx, const float* val, long nnz, float* A, long a_rows, const float* B, long b_rows, int RP, int rows,
                                        int divergence, double beta, double l1, double l2, int update, float* t_frob, float* t_div, float* sumsq_part, int sumsq_parts) {
	return op_masked_beta_half_step<float>(ptr, idx, val, nnz, A, a_rows, B, b_rows, RP, rows, divergence, beta, l1, l2, update, t_frob, t_div, sumsq_part, sumsq_parts);
}

int nmfamd_op_masked_beta_half_step_f64(const int* ptr, const int* idx, const double* val, long nnz, double* A, long a_rows, const double* B, long b_rows, int RP, int rows,
                                        int divergence, double beta, double l1, double l2, int update, double* t_frob, double* t_div, double* sumsq_part, int sumsq_parts) {
	return op_masked_beta_half_step<double>(ptr, idx, val, nnz, A, a_rows, B, b_rows, RP, rows, divergence, beta, l1, l2, update, t_frob, t_div, sumsq_part, sumsq_parts);
}

int nmfamd_op_kl_fused_f32(const int* ptr, const int* idx, const float* val, long nnz, const float* A, const float* B, long b_rows, int RP, int rows, int rows_pad, int blocks,
                           const float* a_scale, float* out, float* t_vwh, float* t_kl) {
	return op_kl_fused<float>(ptr, idx, val, nnz, A, B, b_rows, RP, rows, rows_pad, blocks, a_scale, out, t_vwh, t_kl);
}

int nmfamd_op_kl_fused_f64(const int* ptr, const int* idx, const double* val, long nnz, const double* A, const double* B, long b_rows, int RP, int rows, int rows_pad, int blocks,
                           const double* a_scale, double* out, double* t_vwh, double* t_kl) {
	return op_kl_fused<double>(ptr, idx, val, nnz, A, B, b_rows, RP, rows, rows_pad, blocks, a_scale, out, t_vwh, t_kl);
}

int nmfamd_op_kl_update_f32(float* P, const float* num, int parts, long part_stride, const float* den, const float* scale, int RP, int len_pad, float* sumsq_part,
                            float* sum_part) {
	return op_kl_update<float>(P, num, parts, part_stride, den, scale, RP, len_pad, sumsq_part, sum_part);
}

int nmfamd_op_kl_update_f64(double* P, const double* num, int parts, long part_stride, const double* den, const double* scale, int RP, int len_pad, double* sumsq_part,
                            double* sum_part) {
	return op_kl_update<double>(P, num, parts, part_stride, den, scale, RP, len_pad, sumsq_part, sum_part);
}

int nmfamd_op_kl_sums_f32(const float* sum_part, const float* sumsq_part, int parts, int RP, float* sums, float* scale) {
	return op_kl_sums<float>(sum_part, sumsq_part, parts, RP, sums, scale);
}

int nmfamd_op_kl_sums_f64(const double* sum_part, const double* sumsq_part, int parts, int RP, double* sums, double* scale) {
	return op_kl_sums<double>(sum_part, sumsq_part, parts, RP, sums, scale);
}

int nmfamd_op_panel_rowsum_f32(const float* P, int RP, int len_pad, float* sums) { return op_panel_rowsum<float>(P, RP, len_pad, sums); }

int nmfamd_op_panel_rowsum_f64(const double* P, int RP, int len_pad, double* sums) { return op_panel_rowsum<double>(P, RP, len_pad, sums); }

int nmfamd_op_spmm_rows_f32(const int* ptr, const int* idx, const float* val, long nnz, const float* P, long p_rows, int RP, int rows, int rows_pad, float* out) {
	return op_spmm_rows<float>(ptr, idx, val, nnz, P, p_rows, RP, rows, rows_pad, out);
}

int nmfamd_op_spmm_rows_f64(const int* ptr, const int* idx, const double* val, long nnz, const double* P, long p_rows, int RP, int rows, int rows_pad, double* out) {
	return op_spmm_rows<double>(ptr, idx, val, nnz, P, p_rows, RP, rows, rows_pad, out);
}

int nmfamd_op_sddmm_quotient_f32(const int* ptr, const int* idx, const float* val, long nnz, const float* A, const float* B, long b_rows, int RP, int rows, float* q,
                                 float* t_vwh, float* t_kl) {
	return op_sddmm_quotient<float>(ptr, idx, val, nnz, A, B, b_rows, RP, rows, q, t_vwh, t_kl);
}

int nmfamd_op_sddmm_quotient_f64(const int* ptr, const int* idx, const double* val, long nnz, const double* A, const double* B, long b_rows, int RP, int rows, double* q,
                                 double* t_vwh, double* t_kl) {
	return op_sddmm_quotient<double>(ptr, idx, val, nnz, A, B, b_rows, RP, rows, q, t_vwh, t_kl);
}

} // extern "C"

// Test entries of the Frobenius panel-update kernels (docs/PANEL_UPDATE.md): one launch through launch_panel_update<T> (or, with `fused`, through the launchers the
// fused iterations call) and one through launch_mu64_update / launch_mu64_update32, on caller-supplied padded arrays.  The checks here only keep the kernels inside
// the buffers; which combination of outputs a form accepts is the launchers' decision and comes back as NMFAMD_INVALID_ARGUMENT.
namespace {
// fp32 (len_pad, RP) from a split image in store_split3's layout (split3.h): the three planes added from the smallest up
void decode_split_image(const std::vector<uint16_t>& img, int RP, long len_pad, float* out) {
	const int NBT = RP / 32;
	for (long y = 0; y < len_pad; ++y)
		for (int c = 0; c < RP; ++c) {
			float sum = 0.f;
			for (int pl = 2; pl >= 0; --pl) {
				const size_t idx = (((((size_t)(y / 16) * NBT + c / 32) * 3 + pl) * 2 + ((y / 8) & 1)) * 32 + (c & 31)) * 8 + (y & 7);
				const uint32_t bits = (uint32_t)img[idx] << 16;
				float f;
				std::memcpy(&f, &bits, 4);
				sum += f;
			}
			out[y * RP + c] = sum;
		}
}
size_t split_image_bytes(int RP, long len_pad) { return (size_t)(len_pad / 16) * (RP / 32) * 3 * 64 * 16; }

// an image buffer filled with bf16 NaNs, so that a slot the kernel leaves alone decodes to NaN
hipError_t alloc_nan_image(DevBuf& b, size_t bytes) {
	if (hipError_t e = b.alloc(bytes); e != hipSuccess) return e;
	return hipMemset(b.p, 0xff, bytes);
}

template <typename T>
int op_panel_update(int mode, T* P, const T* slabs, int S, long slab_stride, const T* Q, int RP, int len_pad, int len_valid, T eps, T* ps, T* sumsq_part, long sumsq_rows,
                    T* num_out, T* gram_partial, float* x3_out, int split_q, int tri, const nmfamd_panel_fused* fused, int* parts) {
	constexpr bool f32 = std::is_same<T, float>::value;
	if (!P || !slabs || !Q || !parts || S < 1 || RP < 32 || RP > 512 || RP % 32 != 0 || len_pad < 128 || len_pad % 128 != 0 || len_valid < 0 || len_valid > len_pad ||
	    slab_stride < (long)len_pad * RP || mode < PANEL_MU || mode > PANEL_SET || (sumsq_part && sumsq_rows < 1)) return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	// (MODE_SET always runs the generic kernel, whose workgroups panel_update_parts() does not describe at a rank with a fast form: the engines ask for no partials there)
	const int generic_parts = len_pad / panel_update_rows(RP, sizeof(T));
	const int np = mode == PANEL_SET ? generic_parts : panel_update_parts(RP, sizeof(T), len_pad);
	if (sumsq_part && sumsq_rows < std::max(np, generic_parts)) return NMFAMD_INVALID_ARGUMENT;
	if (fused) {
		// the launchers behind `fused` have no checks of their own for these
		if (mode != PANEL_MU || gram_partial || x3_out || tri || num_out || (fused->smooth && (fused->r < 1 || fused->r > RP))) return NMFAMD_INVALID_ARGUMENT;
		if (f32 ? !panel_update_wide_available(RP) : !(RP == 64 || panel_update_wide_f64_available(RP))) return NMFAMD_INVALID_ARGUMENT;
		if ((fused->x3_out && !f32) || ((fused->smooth_out || fused->scale) && !fused->h_side)) return NMFAMD_INVALID_ARGUMENT;
	}
	const size_t panel = sizeof(T) * (size_t)len_pad * RP, all_slabs = sizeof(T) * (size_t)(((long)S - 1) * slab_stride + (long)len_pad * RP);
	const size_t q_image = (size_t)3 * 16 * (RP / 16 + 1) * (RP / 32) * 64, image = split_image_bytes(RP, len_pad);
	DevBuf dP, dS, dQ, dPs, dSq, dNum, dGram, dX3, dQx, dOs, dSc, dSm;
	if (dP.alloc(panel) != hipSuccess || dS.alloc(all_slabs) != hipSuccess || dQ.alloc(sizeof(T) * (size_t)RP * RP) != hipSuccess) return NMFAMD_NO_DEVICE_MEMORY;
	if (hipMemcpy(dP.p, P, panel, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dS.p, slabs, all_slabs, hipMemcpyHostToDevice) != hipSuccess ||
	    hipMemcpy(dQ.p, Q, sizeof(T) * (size_t)RP * RP, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	// every optional output starts as the caller's array, so that what a launch leaves alone keeps the caller's sentinels
	auto in = [](DevBuf& b, const void* src, size_t bytes) {
		if (src == nullptr) return (int)NMFAMD_OK;
		if (b.alloc(bytes) != hipSuccess) return (int)NMFAMD_NO_DEVICE_MEMORY;
		return hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice) == hipSuccess ? (int)NMFAMD_OK : (int)NMFAMD_HIP_ERROR;
	};
	if (int st = in(dPs, ps, sizeof(T) * (size_t)len_pad)) return st;
	if (int st = in(dSq, sumsq_part, sizeof(T) * (size_t)sumsq_rows * RP)) return st;
	if (int st = in(dNum, num_out, panel)) return st;
	if (int st = in(dGram, gram_partial, sizeof(T) * (size_t)(len_pad / 64) * 4096)) return st;
	if (x3_out && alloc_nan_image(dX3, image) != hipSuccess) return NMFAMD_NO_DEVICE_MEMORY;
	if ((split_q || (fused && f32)) && dQx.alloc(q_image) != hipSuccess) return NMFAMD_NO_DEVICE_MEMORY;
	hipError_t err = hipSuccess;
	panel_update_reset_form();
	if (fused) {
		if (int st = in(dOs, fused->old_scale, sizeof(T) * (size_t)RP)) return st;
		if (int st = in(dSc, fused->scale, sizeof(T) * (size_t)RP)) return st;
		if (int st = in(dSm, fused->smooth_out, panel)) return st;
		if (fused->x3_out && alloc_nan_image(dX3, image) != hipSuccess) return NMFAMD_NO_DEVICE_MEMORY;
		if constexpr (f32) {
			PanelFusedF32 fx;
			fx.old_scale = (const float*)dOs.p; fx.h_side = fused->h_side; fx.scale = (const float*)dSc.p; fx.smooth = fused->smooth;
			fx.off = (float)fused->off; fx.diag = (float)fused->diag; fx.r = fused->r; fx.smooth_out = (float*)dSm.p;
			fx.x3_out = fused->x3_out ? dX3.p : nullptr; fx.x3_ks = len_pad / 16;
			// the r x r operand as the fused iteration hands it over: its split image (A(c, k) = Q(k, c)), no fp32 matrix
			err = launch_pack_panel_x3((const float*)dQ.p, RP, RP, dQx.p, RP / 16, nullptr);
			if (err == hipSuccess)
				err = launch_panel_update_wide_f32(mode, (float*)dP.p, (const float*)dS.p, S, slab_stride, nullptr, RP, len_pad, eps, (float*)dPs.p, len_valid, (float*)dSq.p,
				                                   nullptr, nullptr, dQx.p, nullptr, &fx);
		} else {
			PanelFusedF64 fx = {};
			fx.old_scale = (const double*)dOs.p; fx.h_side = fused->h_side; fx.scale = (const double*)dSc.p; fx.smooth = fused->smooth;
			fx.off = fused->off; fx.diag = fused->diag; fx.r = fused->r; fx.smooth_out = (double*)dSm.p;
			err = RP == 64 ? launch_panel_update64_f64(mode, (double*)dP.p, (const double*)dS.p, S, slab_stride, (const double*)dQ.p, len_pad, eps, (double*)dPs.p, len_valid,
			                                           (double*)dSq.p, nullptr, nullptr, &fx)
			               : launch_panel_update_wide_f64(mode, (double*)dP.p, (const double*)dS.p, S, slab_stride, (const double*)dQ.p, RP, len_pad, eps, (double*)dPs.p, len_valid,
			                                              (double*)dSq.p, nullptr, nullptr, &fx);
		}
	} else {
		const PanelTriExtras none = PanelTriExtras();
		err = launch_panel_update<T>(mode, (T*)dP.p, (const T*)dS.p, S, slab_stride, (const T*)dQ.p, RP, len_pad, eps, (T*)dPs.p, len_valid, (T*)dSq.p, (T*)dNum.p, nullptr,
		                             (T*)dGram.p, dX3.p, x3_out ? len_pad / 16 : 0, split_q ? dQx.p : nullptr, tri ? &none : nullptr);
	}
	if (err == hipErrorInvalidValue) return NMFAMD_INVALID_ARGUMENT;
	if (err != hipSuccess || hipDeviceSynchronize() != hipSuccess) return NMFAMD_HIP_ERROR;
	auto out = [](void* dst, const DevBuf& b, size_t bytes) { return dst == nullptr || hipMemcpy(dst, b.p, bytes, hipMemcpyDeviceToHost) == hipSuccess; };
	if (!out(P, dP, panel) || !out(ps, dPs, sizeof(T) * (size_t)len_pad) || !out(sumsq_part, dSq, sizeof(T) * (size_t)sumsq_rows * RP) || !out(num_out, dNum, panel) ||
	    !out(gram_partial, dGram, sizeof(T) * (size_t)(len_pad / 64) * 4096) || (fused && !out(fused->smooth_out, dSm, panel))) return NMFAMD_HIP_ERROR;
	float* image_out = fused ? fused->x3_out : x3_out;
	if (image_out) {
		std::vector<uint16_t> h(image / 2);
		if (hipMemcpy(h.data(), dX3.p, image, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
		decode_split_image(h, RP, len_pad, image_out);
	}
	*parts = np;
	return NMFAMD_OK;
}
} // namespace

extern "C" {

int nmfamd_op_panel_update_f32(int mode, float* P, const float* slabs, int S, long slab_stride, const float* Q, int RP, int len_pad, int len_valid, float eps, float* ps,
                               float* sumsq_part, long sumsq_rows, float* num_out, float* gram_partial, float* x3_out, int split_q, int tri,
                               const nmfamd_panel_fused* fused, int* parts) {
	return op_panel_update<float>(mode, P, slabs, S, slab_stride, Q, RP, len_pad, len_valid, eps, ps, sumsq_part, sumsq_rows, num_out, gram_partial, x3_out, split_q, tri, fused, parts);
}

int nmfamd_op_panel_update_f64(int mode, double* P, const double* slabs, int S, long slab_stride, const double* Q, int RP, int len_pad, int len_valid, double eps, double* ps,
                               double* sumsq_part, long sumsq_rows, double* num_out, double* gram_partial, float* x3_out, int split_q, int tri,
                               const nmfamd_panel_fused* fused, int* parts) {
	return op_panel_update<double>(mode, P, slabs, S, slab_stride, Q, RP, len_pad, len_valid, eps, ps, sumsq_part, sumsq_rows, num_out, gram_partial, x3_out, split_q, tri, fused, parts);
}

int nmfamd_op_panel_update_last_form(void) { return panel_update_last_form(); }

int nmfamd_op_mu64_update_f32(int is_w, int tile, float* P, const float* slabs, int S, long slab_stride, const float* Q, const float* scale, float eps, int len_pad,
                              int len_valid, float* ps, const float* Gprev, int compute_error, float* gram_partial, float* colsq_part, int qsplit, float* q_out,
                              int ns, float ns_off, float ns_diag, int ns_r, float* x3_out) {
	if (!P || !slabs || !Q || !scale || S < 1 || len_pad < 128 || len_pad % 128 != 0 || len_valid < 0 || len_valid > len_pad || slab_stride < (long)len_pad * 64 ||
	    (tile != 32 && tile != 64) || qsplit < 0 || qsplit > 8) return NMFAMD_INVALID_ARGUMENT;
	// what the kernels would read or write through a null pointer, and what the 64-column launcher has no argument for
	if ((compute_error && (!ps || (is_w && !Gprev))) || (tile == 64 && (qsplit > 1 || ns || colsq_part || q_out)) || (tile == 32 && gram_partial) ||
	    (colsq_part && !is_w) || (q_out && qsplit < 2)) return NMFAMD_INVALID_ARGUMENT;
	if (nmfamd_device_count() <= 0) return NMFAMD_NO_DEVICE;
	const size_t panel = sizeof(float) * (size_t)len_pad * 64, all_slabs = sizeof(float) * (size_t)(((long)S - 1) * slab_stride + (long)len_pad * 64);
	const size_t qbytes = sizeof(float) * 4096 * (size_t)(qsplit > 1 ? qsplit : 1), image = split_image_bytes(64, len_pad), grams = sizeof(float) * (size_t)(len_pad / 64) * 4096;
	DevBuf dP, dS, dQ, dScale, dPs, dGprev, dGram, dColsq, dQout, dX3;
	if (dP.alloc(panel) != hipSuccess || dS.alloc(all_slabs) != hipSuccess || dQ.alloc(qbytes) != hipSuccess || dScale.alloc(sizeof(float) * 64) != hipSuccess ||
	    alloc_nan_image(dX3, image) != hipSuccess) return NMFAMD_NO_DEVICE_MEMORY;
	if (hipMemcpy(dP.p, P, panel, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dS.p, slabs, all_slabs, hipMemcpyHostToDevice) != hipSuccess ||
	    hipMemcpy(dQ.p, Q, qbytes, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dScale.p, scale, sizeof(float) * 64, hipMemcpyHostToDevice) != hipSuccess) return NMFAMD_HIP_ERROR;
	auto in = [](DevBuf& b, const void* src, size_t bytes) {
		if (src == nullptr) return (int)NMFAMD_OK;
		if (b.alloc(bytes) != hipSuccess) return (int)NMFAMD_NO_DEVICE_MEMORY;
		return hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice) == hipSuccess ? (int)NMFAMD_OK : (int)NMFAMD_HIP_ERROR;
	};
	if (int st = in(dPs, ps, sizeof(float) * (size_t)len_pad)) return st;
	if (int st = in(dGprev, Gprev, sizeof(float) * 4096)) return st;
	if (int st = in(dColsq, colsq_part, sizeof(float) * (size_t)(len_pad / 32) * 64)) return st;
	if (int st = in(dQout, q_out, sizeof(float) * 4096)) return st;
	// (the 64-column kernel always writes its partial Gram matrices)
	if (tile == 64) {
		if (dGram.alloc(grams) != hipSuccess) return NMFAMD_NO_DEVICE_MEMORY;
		if (hipMemset(dGram.p, 0xff, grams) != hipSuccess) return NMFAMD_HIP_ERROR;
	}
	const SmoothAround sm = {ns_off, ns_diag, ns_r};
	const hipError_t err =
	    tile == 64 ? launch_mu64_update(is_w, (float*)dP.p, (const float*)dS.p, S, slab_stride, (const float*)dQ.p, (const float*)dScale.p, eps, (float*)dPs.p, len_valid, len_pad,
	                                    (float*)dGram.p, (const float*)dGprev.p, compute_error, nullptr, x3_out ? dX3.p : nullptr, len_pad / 16)
	               : launch_mu64_update32(is_w, (float*)dP.p, (const float*)dS.p, S, slab_stride, (const float*)dQ.p, (const float*)dScale.p, eps, (float*)dPs.p, len_valid, len_pad,
	                                      (const float*)dGprev.p, compute_error, nullptr, dX3.p, len_pad / 16, nullptr, (float*)dColsq.p, qsplit, (float*)dQout.p, ns ? &sm : nullptr);
	if (err == hipErrorInvalidValue) return NMFAMD_INVALID_ARGUMENT;
	if (err != hipSuccess || hipDeviceSynchronize() != hipSuccess) return NMFAMD_HIP_ERROR;
	auto out = [](void* dst, const DevBuf& b, size_t bytes) { return dst == nullptr || hipMemcpy(dst, b.p, bytes, hipMemcpyDeviceToHost) == hipSuccess; };
	if (!out(P, dP, panel) || !out(ps, dPs, sizeof(float) * (size_t)len_pad) || !out(colsq_part, dColsq, sizeof(float) * (size_t)(len_pad / 32) * 64) ||
	    !out(q_out, dQout, sizeof(float) * 4096) || (tile == 64 && !out(gram_partial, dGram, grams))) return NMFAMD_HIP_ERROR;
	if (x3_out) {
		std::vector<uint16_t> h(image / 2);
		if (hipMemcpy(h.data(), dX3.p, image, hipMemcpyDeviceToHost) != hipSuccess) return NMFAMD_HIP_ERROR;
		decode_split_image(h, 64, len_pad, x3_out);
	}
	return NMFAMD_OK;
}

} // extern "C"
