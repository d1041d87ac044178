"""HALS with sparse compute (V kept as CSR + CSC, the two products as SpMM launches) on the GPU against the fp64 restatement of
tests/hals_penalty_reference.py on the densified V, with and without penalties.

Tolerances are those of tests/test_gpu_hals.py (factors 2e-4 fp32 / 1e-9 fp64, reported error 1e-5 / 1e-9).  fp64 runs 20 iterations; fp32 is
compared over ONE iteration from a state downloaded after 20 (the pattern of test_one_step_from_a_drifted_state), so that no number depends on
how fast sparse fp32 trajectories drift.
"""
import numpy as np
import pytest

import nmfgpu_amd as na
from tests import hals_penalty_reference as pen

pytestmark = pytest.mark.gpu

PEN = (0.05, 0.05, 0.01, 0.01)   # (l1W, l1H, l2W, l2H): V has 5 % entries in (0, 1], so G and a are small
EMPTY_ROWS, EMPTY_COLS = (3, 150, 299), (0, 77)


def F(a):
    return np.asfortranarray(a)


def rel(a, b):
    return np.linalg.norm(a.astype(np.float64) - b.astype(np.float64)) / max(np.linalg.norm(b.astype(np.float64)), 1e-300)


def kw(p):
    return dict(l1_w=p[0], l1_h=p[1], l2_w=p[2], l2_h=p[3])


@pytest.fixture(scope="module", autouse=True)
def _library_is_native():
    assert na.device_count() >= 1, "GPU tests need a HIP device"
    assert na.initialize() in (na.ResultType.Success, na.ResultType.ErrorAlreadyInitialized)
    na.set_verbosity(na.Verbosity.Nothing)
    yield
    na.finalize()


def sparse_problem(m, n, r, dtype, seed=1, density=0.05):
    """COO triplets sorted by (row, column) with a stored zero and a few empty rows and columns, the densified V (the values rounded to dtype), a start."""
    rng = np.random.default_rng(seed)
    rows, cols, vals, _ = pen.sparse_pattern(m, n, density, rng, EMPTY_ROWS, EMPTY_COLS)
    vals = vals.astype(dtype)
    assert vals[0] == 0
    V = np.zeros((m, n))
    V[rows, cols] = vals
    W = F((1.0 - rng.random((m, r))).astype(dtype))
    H = F((1.0 - rng.random((r, n))).astype(dtype))
    return (rows, cols, vals), V, W, H


def as_format(coo, m, n, fmt, base):
    """(values, a, b) of nmfamd_engine_upload_sparse: fmt 1 CSR, 2 CSC, 3 COO (shuffled)."""
    rows, cols, vals = coo
    if fmt == 1:
        ptr = np.zeros(m + 1, np.int32)
        np.cumsum(np.bincount(rows, minlength=m), out=ptr[1:])
        return vals, ptr + base, cols + base
    if fmt == 2:
        order = np.lexsort((rows, cols))
        ptr = np.zeros(n + 1, np.int32)
        np.cumsum(np.bincount(cols, minlength=n), out=ptr[1:])
        return vals[order], ptr + base, rows[order] + base
    perm = np.random.default_rng(1).permutation(len(vals))
    return vals[perm], (rows + base)[perm], (cols + base)[perm]


def engine(coo, m, n, W, H, fmt=1, base=0, **k):
    eng = na.Engine(m, n, W.shape[1], "hals", dtype=W.dtype, sparse_compute=True, **k)
    vals, a, b = as_format(coo, m, n, fmt, base)
    eng.upload_sparse(fmt, vals, a.astype(np.int32), b.astype(np.int32), base)
    eng.set_factors(W, H)
    return eng


def check_padding(eng):
    g = eng.geometry()
    RP, mp, np_ = g["padded_rank"], g["padded_m"], g["padded_n"]
    Wt = eng.debug_read(0, RP * mp).reshape(mp, RP)
    Hp = eng.debug_read(1, RP * np_).reshape(np_, RP)
    assert (Wt[:, eng.r:] == 0).all() and (Wt[eng.m:, :] == 0).all()
    assert (Hp[:, eng.r:] == 0).all() and (Hp[eng.n:, :] == 0).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("p", [(0.0, 0.0, 0.0, 0.0), PEN])
def test_formats_and_index_bases_bit_identical(dtype, p):
    m, n, r = 300, 200, 12
    coo, V, W, H = sparse_problem(m, n, r, dtype, seed=3)
    results = []
    for fmt in (1, 2, 3):
        for base in (0, 1):
            eng = engine(coo, m, n, W, H, fmt, base, **kw(p))
            g = eng.geometry()
            assert g["product_kernel"] == 5 and g["resident_images"] == 0 and g["fused_launches"] == 0
            errs = []
            for it in range(1, 6):
                eng.iterate(1, first_iteration=it, error_every=1)
                errs.append(eng.frobenius)
            results.append(eng.get_factors() + (errs,))
            eng.close()
    for Wg, Hg, errs in results[1:]:
        assert np.array_equal(Wg, results[0][0]) and np.array_equal(Hg, results[0][1]) and errs == results[0][2]


# padded ranks 64, 128, 256 (m, n well above r: where m or n is below r the Gram matrices are singular and the result is set by rounding, in fp64
# too -- test_seeded_ragged_sweep of tests/test_gpu_hals.py)
SHAPES = [(300, 200, 12), (600, 500, 100), (900, 700, 200)]


@pytest.mark.parametrize("m,n,r", SHAPES)
@pytest.mark.parametrize("p", [(0.0, 0.0, 0.0, 0.0), PEN])
def test_fp64_parity_with_restatement(m, n, r, p):
    coo, V, W, H = sparse_problem(m, n, r, np.float64, seed=5 + r)
    eng = engine(coo, m, n, W, H, **kw(p))
    assert eng.geometry()["padded_rank"] == (64 if r <= 64 else 128 if r <= 128 else 256)
    W64, H64, done = W, H, 0
    for iters in (1, 20):
        W64, H64, errs = pen.run(V, W64, H64, iters - done, *p)
        eng.iterate(iters - done, first_iteration=done + 1, error_every=0, last_iteration=iters)
        done = iters
        Wg, Hg = eng.get_factors()
        print(r, p, iters, "rel W", rel(Wg, W64), "rel H", rel(Hg, H64), "error", eng.frobenius, errs[-1])
        assert rel(Wg, W64) < 1e-9 and rel(Hg, H64) < 1e-9, (iters, rel(Wg, W64), rel(Hg, H64))
        assert abs(eng.frobenius - errs[-1]) <= 1e-9 * errs[-1], (iters, eng.frobenius, errs[-1])
    # empty rows / columns of V: zero rows of W, zero columns of H, nothing undefined
    assert (Wg[list(EMPTY_ROWS)] == 0).all() and (Hg[:, list(EMPTY_COLS)] == 0).all()
    assert np.isfinite(Wg).all() and np.isfinite(Hg).all()
    check_padding(eng)
    eng.close()


@pytest.mark.parametrize("m,n,r", SHAPES)
@pytest.mark.parametrize("p", [(0.0, 0.0, 0.0, 0.0), PEN])
def test_fp32_one_step_from_a_drifted_state(m, n, r, p):
    coo, V, W, H = sparse_problem(m, n, r, np.float32, seed=7 + r)
    eng = engine(coo, m, n, W, H, **kw(p))
    eng.iterate(20, error_every=0, last_iteration=20)
    W0, H0 = eng.get_factors()
    assert (W0[list(EMPTY_ROWS)] == 0).all() and (H0[:, list(EMPTY_COLS)] == 0).all()
    assert np.isfinite(W0).all() and np.isfinite(H0).all() and np.isfinite(eng.frobenius)
    eng.iterate(1, first_iteration=21, error_every=0, last_iteration=21)
    Wg, Hg = eng.get_factors()
    reported = eng.frobenius
    check_padding(eng)
    eng.close()
    W64, H64, err = pen.iteration(V, W0, H0, *p)
    print(r, p, "rel W", rel(Wg, W64), "rel H", rel(Hg, H64), "error", reported, err)
    assert rel(Wg, W64) < 2e-4 and rel(Hg, H64) < 2e-4, (rel(Wg, W64), rel(Hg, H64))
    assert abs(reported - err) <= 1e-5 * err, (reported, err)


def test_constant_w_on_sparse_v():
    m, n, r = 300, 200, 12
    coo, V, W, H = sparse_problem(m, n, r, np.float64, seed=11)
    eng = engine(coo, m, n, W, H, **kw(PEN))
    eng.iterate(5, error_every=5, constant_w=True)
    Wg, Hg = eng.get_factors()
    _, H64, errs = pen.run(V, W, H, 5, *PEN, constant_w=True)
    assert np.array_equal(Wg, W) and rel(Hg, H64) < 1e-9 and abs(eng.frobenius - errs[-1]) <= 1e-9 * errs[-1]
    eng.close()


# ------------------------------------------------------------------ through nmfgpu::compute

def csr_description(coo, m, n, base=0):
    vals, ptr, idx = as_format(coo, m, n, 1, base)
    keep = (np.ascontiguousarray(vals), np.ascontiguousarray(ptr, dtype=np.int32), np.ascontiguousarray(idx, dtype=np.int32))
    return na.api.sparse_description(na.StorageFormat.CSR, m, n, *keep, base=na.IndexBase.One if base else na.IndexBase.Zero), keep


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("p", [(0.0, 0.0, 0.0, 0.0), PEN])
def test_compute_on_a_csr_description(dtype, p):
    """ErrorInvalidArgument before HALS took sparse compute.  fp64 runs 20 iterations; fp32 one, so that its numbers do not depend on how fast a
    sparse fp32 trajectory drifts (the threshold and two-run test below runs fp32 for many)."""
    m, n, r = 300, 200, 12
    coo, V, W, H = sparse_problem(m, n, r, dtype, seed=13)
    desc, keep = csr_description(coo, m, n, base=1)
    iters = 1 if dtype == np.float32 else 20
    tol_f, tol_e = (2e-4, 1e-5) if dtype == np.float32 else (1e-9, 1e-9)
    params = {"sparseCompute": 1, "l1W": p[0], "l1H": p[1], "l2W": p[2], "l2H": p[3]}
    W64, H64, errs = pen.run(V, W, H, iters, *p)
    s = na.Summary()
    res = na.compute(desc, W, H, algorithm=na.NmfAlgorithm.HALS, iterations=iters, parameters=params, summary=s)
    assert res == na.ResultType.Success, res
    rec = s.record(0)
    assert rec.numIterations == iters
    assert abs(rec.frobenius - errs[-1]) <= tol_e * errs[-1], (rec.frobenius, errs[-1])
    assert rel(W, W64) < tol_f and rel(H, H64) < tol_f, (rel(W, W64), rel(H, H64))


@pytest.mark.parametrize("p", [(0.0, 0.0, 0.0, 0.0), PEN])
def test_compute_threshold_and_two_runs(p):
    m, n, r = 300, 200, 12
    coo, V, W, H = sparse_problem(m, n, r, np.float32, seed=17)
    desc, keep = csr_description(coo, m, n)
    params = {"sparseCompute": 1, "l1W": p[0], "l1H": p[1], "l2W": p[2], "l2H": p[3]}
    s = na.Summary()
    res = na.compute(desc, W, H, algorithm=na.NmfAlgorithm.HALS, iterations=2000, threshold=1e-3, parameters=params, summary=s)
    assert res == na.ResultType.Success, res
    rec = s.record(0)
    assert rec.numIterations < 2000
    got = np.linalg.norm(V - W.astype(np.float64) @ H.astype(np.float64))
    assert rec.frobenius > 0 and abs(got - rec.frobenius) < 0.01 * rec.frobenius, (got, rec.frobenius)
    best = {}
    for runs in (1, 2):
        s = na.Summary()
        res = na.compute(desc, W, H, algorithm=na.NmfAlgorithm.HALS, init=na.NmfInitializationMethod.AllRandomValues, iterations=40, runs=runs, seed=5,
                         parameters=params, summary=s)
        assert res == na.ResultType.Success, res
        assert 1 <= s.record_count() <= runs
        best[runs] = s.record(s.best_run()).frobenius
        assert best[runs] == min(s.record(i).frobenius for i in range(s.record_count()))
    assert best[2] <= best[1]


def test_refusals():
    m, n = 300, 280
    rng = np.random.default_rng(0)
    # rank 257: padded rank 384, beyond what the SpMM kernels gather
    for dtype in (np.float32, np.float64):
        with pytest.raises(na.EngineError) as info:
            na.Engine(m, n, 257, "hals", dtype=dtype, sparse_compute=True)
        assert info.value.status == 1 and "rank <= 256" in str(info.value), str(info.value)
    eng = na.Engine(m, n, 256, "hals", sparse_compute=True)
    assert eng.geometry()["padded_rank"] == 256
    eng.close()
    for k in (dict(divergence="kl"), dict(missing_values=True), dict(divergence="kl", sparse_compute=True)):
        with pytest.raises(na.EngineError) as info:
            na.Engine(m, n, 8, "hals", **k)
        # (missing values: the refusal of the masked update itself comes first)
        assert info.value.status == 1 and ("missing values" if "missing_values" in k else "Frobenius objective only") in str(info.value), (k, str(info.value))
    coo, V, W, H = sparse_problem(m, n, 8, np.float32, seed=19)
    desc, keep = csr_description(coo, m, n)
    W0, H0 = W.copy(), H.copy()
    bad = na.ResultType.ErrorInvalidArgument
    hals = dict(algorithm=na.NmfAlgorithm.HALS, iterations=3)
    for extra in ({"divergence": 1}, {"numGpus": 2}, {"missingValues": 1}):
        assert na.compute(desc, W, H, parameters={"sparseCompute": 1, **extra}, **hals) == bad, extra
    assert np.array_equal(W, W0) and np.array_equal(H, H0)
    Ww, Hw = F(rng.random((m, 257)).astype(np.float32)), F(rng.random((257, n)).astype(np.float32))
    assert na.compute(desc, Ww, Hw, parameters={"sparseCompute": 1}, **hals) == bad
    # the three-phase API keeps refusing HALS, sparse or not
    eng = engine(coo, m, n, W, H)
    with pytest.raises(na.EngineError) as info:
        eng.h_step(False)
    assert info.value.status == 1
    eng.close()
