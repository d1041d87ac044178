"""Missing-value NMF under the beta-divergence on the GPU (docs/MISSING.md, "Beta-divergence"): the masked update of kernels_masked_beta.hip against the fp64
entry-list restatement (tests/masked_beta_reference.py) and against the dense weighted engine at 0 / 1 weights; penalties, constant W, every input form, edge rows
and columns, duplicates, the value rule of beta, nmfgpu::compute with "missingDivergence" / "missingBeta", the refusals, and what the feature is for.

Tolerances: TOL of tests/test_gpu_beta_general.py.  The divergence at density 0.02 is a cancelled sum (the fit is nearly exact), so in fp32 it is held to the absolute
bound etol * S there, S the fp64 sum over the stored entries of the absolute values of the three summands of d_beta; from density 0.3 up the bound is relative."""
import numpy as np
import pytest

import nmfgpu_amd as na
from nmfgpu_amd import api
from tests import masked_beta_reference as mbref
from tests import masked_reference as mref

pytestmark = pytest.mark.gpu

TOL = {np.float32: (2e-4, 1e-5), np.float64: (1e-9, 1e-9)}       # factors, errors (frobenius, rmsd, divergence)
PEN = (0.05, 0.05, 0.01, 0.01)                                   # (l1W, l1H, l2W, l2H), as tests/test_gpu_beta_general.py
DTYPES = [np.float32, np.float64]
BETAS = [-1.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0]


def F(a):
    return np.asfortranarray(a)


def rel(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b), 1e-300))


def eps_of(dtype):
    return float(np.finfo(dtype).eps)


def start(m, n, r, dtype, seed):
    rng = np.random.default_rng(seed)
    return F((1.0 - rng.random((m, r))).astype(dtype)), F((1.0 - rng.random((r, n))).astype(dtype))


def kw_of(beta):
    """The keywords of a beta: "is" and "kl" at 0 and 1, "beta" otherwise."""
    return dict(missing_divergence="is") if beta == 0 else dict(missing_divergence="kl") if beta == 1 else dict(missing_divergence="beta", missing_beta=beta)


def engine(m, n, r, dtype, beta, pen=mbref.NO_PENALTIES, **kw):
    return na.Engine(m, n, r, "mu", dtype=dtype, missing_values=True, l1_w=pen[0], l1_h=pen[1], l2_w=pen[2], l2_h=pen[3], **dict(kw_of(beta), **kw))


def upload_csr(eng, rows, cols, vals, m, base=0):
    ptr, idx, v = mref.csr_of(rows, cols, vals, m)
    eng.upload_sparse(1, v.astype(eng.dtype), ptr + base, idx + base, base)


def run_engine(eng, W0, H0, iters, constant_w=False, first=1):
    if W0 is not None:
        eng.set_factors(W0, H0)
    eng.iterate(iters, first_iteration=first, error_every=0, last_iteration=first + iters - 1, constant_w=constant_w)
    W, H = eng.get_factors()
    return W, H, eng.frobenius, eng.rmsd, eng.divergence_value


def check(got, want, dtype, absolute_divergence=False, what="", scale=1.0):
    """got: (W, H, frobenius, rmsd, divergence) of an engine; want: the restatement's run (with S sixth).  scale: a multiple of TOL (2 between two engines)."""
    ftol, etol = (scale * t for t in TOL[dtype])
    S = want[5]
    figures = (rel(got[0], want[0]), rel(got[1], want[1]), abs(got[2] / want[2] - 1), abs(got[3] / want[3] - 1), abs(got[4] - want[4]) / max(abs(want[4]), 1e-300),
               abs(got[4] - want[4]) / S)
    print(f"{what} {np.dtype(dtype).name}: W {figures[0]:.2e} H {figures[1]:.2e} frobenius {figures[2]:.2e} rmsd {figures[3]:.2e} divergence {figures[4]:.2e} (of S: {figures[5]:.2e})")
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1]))
    assert figures[0] < ftol and figures[1] < ftol, figures
    assert figures[2] < etol and figures[3] < etol, figures
    assert (figures[5] if absolute_divergence else figures[4]) < etol, figures


@pytest.fixture(scope="module")
def ctx():
    assert na.initialize() in (na.ResultType.Success, na.ResultType.ErrorAlreadyInitialized)
    na.set_verbosity(na.Verbosity.Nothing)
    yield
    na.finalize()


# 1. parity with the restatement: every map and every exponent, every padded rank, sparse to complete
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("density", [0.02, 0.3, 1.0])
@pytest.mark.parametrize("r,beta", [(r, b) for r in (8, 65, 129) for b in BETAS] + [(256, 0.5)])
def test_parity_with_restatement(r, beta, density, dtype):
    m, n, iters = 131 + r % 7, 97 + r % 5, 20
    rows, cols, vals = mref.planted_ratings(m, n, density, seed=r + int(100 * density))
    W0, H0 = start(m, n, r, dtype, seed=r)
    eng = engine(m, n, r, dtype, beta)
    rp = eng.geometry()["padded_rank"]
    assert rp == (64 if r <= 64 else 128 if r <= 128 else 256)
    upload_csr(eng, rows, cols, vals, m)
    got = run_engine(eng, W0, H0, iters)
    want = mbref.run(rows, cols, vals, W0, H0, iters, beta, eps_of(dtype))
    check(got, want, dtype, absolute_divergence=dtype == np.float32 and density == 0.02, what=f"beta {beta} r {r} density {density}")
    assert got[3] == pytest.approx(got[2] / np.sqrt(len(vals)), rel=1e-12)
    # padding coordinates stay exactly zero; rows and columns without an entry become exactly zero
    Hp = eng.debug_read(1, rp * n).reshape(n, rp)
    assert np.all(Hp[:, r:] == 0)
    seen_r, seen_c = np.zeros(m, bool), np.zeros(n, bool)
    seen_r[rows] = True; seen_c[cols] = True
    assert np.all(got[0][~seen_r] == 0) and np.all(got[1][:, ~seen_c] == 0)
    eng.close()


# 2. the dense weighted engine on the same Omega as 0 / 1 weights, from the same start
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("beta", [0.0, 0.5, 1.0])
def test_agrees_with_the_dense_weighted_engine(beta, dtype):
    m, n, r, iters = 137, 101, 9, 20
    rows, cols, vals = mref.planted_ratings(m, n, 0.3, seed=21)
    W0, H0 = start(m, n, r, dtype, seed=22)
    want = mbref.run(rows, cols, vals, W0, H0, iters, beta, eps_of(dtype))
    eng = engine(m, n, r, dtype, beta)
    upload_csr(eng, rows, cols, vals, m)
    masked = run_engine(eng, W0, H0, iters)
    eng.close()
    dense_kw = dict(divergence="is") if beta == 0 else dict(divergence="kl", dense_compute=True) if beta == 1 else dict(divergence="beta", beta=beta)
    weng = na.Engine(m, n, r, "mu", dtype=dtype, weighted=True, **dense_kw)
    V = np.zeros((m, n), dtype); V[rows, cols] = vals
    Om = np.zeros((m, n), dtype); Om[rows, cols] = 1
    weng.upload(F(V), weights=F(Om))
    dense = run_engine(weng, W0, H0, iters)
    weng.close()
    check(masked, want, dtype, what=f"masked beta {beta}")
    check(dense, want, dtype, what=f"weighted beta {beta}")
    check(masked, dense + (want[5],), dtype, what=f"masked against weighted beta {beta}", scale=2.0)


# 3. penalties, and set_penalties back to zero restores the unpenalised iteration, normalisation included
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("beta", [0.0, 0.5, 1.0])
def test_penalties(beta, dtype):
    m, n, r, iters = 137, 101, 9, 20
    rows, cols, vals = mref.planted_ratings(m, n, 0.3, seed=31 + int(10 * beta))
    W0, H0 = start(m, n, r, dtype, seed=32)
    eng = engine(m, n, r, dtype, beta, PEN)
    upload_csr(eng, rows, cols, vals, m)
    got = run_engine(eng, W0, H0, iters)
    pen = tuple(float(dtype(p)) for p in PEN)
    want = mbref.run(rows, cols, vals, W0, H0, iters, beta, eps_of(dtype), pen=pen)
    check(got, want, dtype, what=f"penalised beta {beta}")
    plain = mbref.run(rows, cols, vals, W0, H0, iters, beta, eps_of(dtype))
    assert rel(got[0], plain[0]) > 1e-3      # (the penalties did something; without normalisation W is not unit-norm either)
    assert not np.allclose(np.linalg.norm(got[0].astype(np.float64), axis=0), 1.0, atol=1e-3)
    eng.set_penalties(0.0, 0.0, 0.0, 0.0)
    more = run_engine(eng, None, None, 5, first=iters + 1)
    check(more, mbref.run(rows, cols, vals, got[0], got[1], 5, beta, eps_of(dtype)), dtype, what=f"penalties back to zero, beta {beta}")
    assert np.allclose(np.linalg.norm(more[0].astype(np.float64), axis=0), 1.0, atol=1e-4)
    eng.close()


# 4. constant W: the H step alone, W bit for bit, the errors from the terms-only launch
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("beta", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("r", [16, 200])
def test_constant_w(r, beta, dtype):
    m, n, iters = 140, 100, 10
    rows, cols, vals = mref.planted_ratings(m, n, 0.3, seed=41 + r)
    W0, H0 = start(m, n, r, dtype, seed=42)
    eng = engine(m, n, r, dtype, beta)
    upload_csr(eng, rows, cols, vals, m)
    got = run_engine(eng, W0, H0, iters, constant_w=True)
    assert np.array_equal(got[0], W0)
    check(got, mbref.run(rows, cols, vals, W0, H0, iters, beta, eps_of(dtype), const_w=True), dtype, what=f"constant W beta {beta} r {r}")
    eng.close()


# 5. the same Omega through every input form, the device-resident ones included: bit-identical; a repeated run too
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("beta", [0.5, 1.0])
def test_every_input_form_is_bit_identical(beta, dtype):
    import torch
    m, n, r, iters = 173, 141, 10, 12
    rows, cols, vals = mref.planted_ratings(m, n, 0.2, seed=51)
    vals = vals.astype(dtype)
    W0, H0 = start(m, n, r, dtype, seed=52)
    outs = []

    def go(upload):
        eng = engine(m, n, r, dtype, beta)
        upload(eng)
        outs.append(run_engine(eng, W0, H0, iters))
        eng.close()

    D = np.full((m, n), np.nan, dtype=dtype); D[rows, cols] = vals
    go(lambda e: e.upload(F(D)))
    for base in (0, 1):
        go(lambda e: upload_csr(e, rows, cols, vals, m, base))
        cp, ci, cv = mref.csc_of(rows, cols, vals, n)
        go(lambda e: e.upload_sparse(2, cv.astype(dtype), cp + base, ci + base, base))
        perm = np.random.default_rng(53 + base).permutation(len(vals))
        go(lambda e: e.upload_sparse(3, vals[perm], (rows[perm] + base).astype(np.int32), (cols[perm] + base).astype(np.int32), base))
    ptr, idx, v = mref.csr_of(rows, cols, vals, m)
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (v.astype(dtype), ptr, idx)]
    go(lambda e: e.upload_sparse_device(1, *dev, 0))
    Dd = torch.from_numpy(np.ascontiguousarray(D)).cuda()
    go(lambda e: e.upload_device_stored(Dd))
    go(lambda e: upload_csr(e, rows, cols, vals, m))
    for o in outs[1:]:
        assert np.array_equal(o[0], outs[0][0]) and np.array_equal(o[1], outs[0][1])
        assert o[2:] == outs[0][2:]


# 6. empty rows and columns, duplicated COO entries
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("beta", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("r", [5, 200])
def test_edge_rows_columns_and_duplicates(r, beta, dtype):
    m, n, iters = 150, 120, 20
    rows, cols, vals = mref.planted_ratings(m, n, 0.3, seed=61 + r)
    keep = (rows % 17 != 3) & (cols % 13 != 5)
    rows, cols, vals = rows[keep], cols[keep], vals[keep]
    rng = np.random.default_rng(62)
    d = rng.choice(len(vals), 60, replace=False)
    rows, cols, vals = np.append(rows, rows[d]), np.append(cols, cols[d]), np.append(vals, rng.integers(1, 6, 60).astype(np.float64))
    perm = rng.permutation(len(vals))
    W0, H0 = start(m, n, r, dtype, seed=63)
    eng = engine(m, n, r, dtype, beta)
    eng.upload_sparse(3, vals[perm].astype(dtype), rows[perm].astype(np.int32), cols[perm].astype(np.int32), 0)
    got = run_engine(eng, W0, H0, iters)
    check(got, mbref.run(rows, cols, vals, W0, H0, iters, beta, eps_of(dtype)), dtype, what=f"edges and duplicates beta {beta} r {r}")
    assert got[3] == pytest.approx(got[2] / np.sqrt(len(vals)), rel=1e-12)      # (a duplicate counts once per stored copy)
    assert np.all(got[0][np.arange(m) % 17 == 3] == 0) and np.all(got[1][:, np.arange(n) % 13 == 5] == 0)
    assert np.all(got[0] >= 0) and np.all(got[1] >= 0)
    eng.close()


# 7. a stored zero: an observation at beta > 0, refused at beta <= 0 -- on the host paths and on the device paths
def with_zeros(m, n, seed):
    rows, cols, vals = mref.planted_ratings(m, n, 0.25, seed=seed)
    rng = np.random.default_rng(seed + 1)
    taken = set(zip(rows.tolist(), cols.tolist()))
    pairs = sorted({(int(i), int(j)) for i, j in zip(rng.integers(0, m, 400), rng.integers(0, n, 400))} - taken)
    zr, zc = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    return (rows, cols, vals), (np.append(rows, zr), np.append(cols, zc), np.append(vals, np.zeros(len(zr))))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("beta", [0.5, 1.0, 2.0])
def test_stored_zeros_are_observed_above_beta_zero(beta, dtype):
    m, n, r, iters = 120, 90, 6, 20
    without, zeros = with_zeros(m, n, seed=71)
    W0, H0 = start(m, n, r, dtype, seed=73)
    results = []
    for R, Cc, Vv in (without, zeros):
        eng = engine(m, n, r, dtype, beta)
        upload_csr(eng, R, Cc, Vv, m)
        got = run_engine(eng, W0, H0, iters)
        check(got, mbref.run(R, Cc, Vv, W0, H0, iters, beta, eps_of(dtype)), dtype, what=f"stored zeros beta {beta}")
        results.append(got)
        eng.close()
    assert rel(results[0][1], results[1][1]) > 1e-2
    assert results[1][3] == pytest.approx(results[1][2] / np.sqrt(len(zeros[2])), rel=1e-12)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("beta", [-1.0, 0.0, 0.5])
def test_value_rule_on_host_and_device_paths(beta, dtype):
    import torch
    m, n, r = 120, 90, 6
    good, zeros = with_zeros(m, n, seed=81)
    # beta <= 0: a stored zero is refused; beta > 0: a negative value is
    rows, cols, vals = zeros
    vals = vals.astype(dtype)
    if beta > 0:
        vals = vals.copy(); vals[vals == 0] = -1.0
    text = "missing values with beta <= 0: every stored value has to be finite and > 0" if beta <= 0 else "missing values with beta > 0: every stored value has to be finite and >= 0"
    ptr, idx, v = mref.csr_of(rows, cols, vals, m)
    v = v.astype(dtype)
    D = np.full((m, n), np.nan, dtype=dtype); D[rows, cols] = vals
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (v, ptr, idx)]
    Dd = torch.from_numpy(np.ascontiguousarray(D)).cuda()
    uploads = {"dense": lambda e: e.upload(F(D)), "csr": lambda e: e.upload_sparse(1, v, ptr, idx, 0),
               "device csr": lambda e: e.upload_sparse_device(1, *dev, 0), "device dense": lambda e: e.upload_device_stored(Dd)}
    for name, upload in uploads.items():
        eng = engine(m, n, r, dtype, beta)
        with pytest.raises(na.EngineError) as err:
            upload(eng)
        assert err.value.status == 1 and text in str(err.value), (name, str(err.value))
        eng.randomize(3)
        with pytest.raises(na.EngineError) as err:      # the engine does not iterate
            eng.iterate(1, first_iteration=1, error_every=0, last_iteration=1)
        assert err.value.status == 1, name
        # ... and takes a good upload afterwards
        upload_csr(eng, *good, m)
        eng.iterate(2, first_iteration=1, error_every=0, last_iteration=2)
        assert np.isfinite(eng.divergence_value) and eng.divergence_value > 0
        eng.close()
    inf = v.copy(); inf[5] = np.inf
    eng = engine(m, n, r, dtype, beta)
    with pytest.raises(na.EngineError):
        eng.upload_sparse(1, inf, ptr, idx, 0)
    eng.close()


# 8. nmfgpu::compute with "missingDivergence" and "missingBeta"
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["dense", "csr"])
@pytest.mark.parametrize("beta", [1.0, 0.5])
def test_compute(ctx, beta, form, dtype):
    m, n, r, iters = 160, 120, 7, 20
    rows, cols, vals = mref.planted_ratings(m, n, 0.35, seed=91)
    W0, H0 = start(m, n, r, dtype, seed=92)
    params = {"missingValues": 1, "missingDivergence": 1} if beta == 1 else {"missingValues": 1, "missingDivergence": 3, "missingBeta": beta}
    keep = []
    if form == "dense":
        D = np.full((m, n), np.nan, dtype=dtype); D[rows, cols] = vals
        V = F(D)
    else:
        ptr, idx, v = mref.csr_of(rows, cols, vals, m)
        v = v.astype(dtype); keep = [ptr, idx, v]
        V = api.sparse_description(na.StorageFormat.CSR, m, n, v, ptr, idx)
    ftol, etol = TOL[dtype]

    def against(W, H, rec, want):
        assert rel(W, want[0]) < ftol and rel(H, want[1]) < ftol, (rel(W, want[0]), rel(H, want[1]))
        assert rec.frobenius == pytest.approx(want[2], rel=etol) and rec.rmsd == pytest.approx(want[3], rel=etol)
        assert rec.rmsd == pytest.approx(rec.frobenius / np.sqrt(len(vals)), rel=1e-12)

    W, H = W0.copy(order="F"), H0.copy(order="F")
    s = na.Summary()
    assert na.compute(V, W, H, iterations=iters, parameters=params, summary=s) == na.ResultType.Success
    against(W, H, s.record(0), mbref.run(rows, cols, vals, W0, H0, iters, beta, eps_of(dtype)))
    assert s.record(0).numIterations == iters
    # with penalties
    W, H = W0.copy(order="F"), H0.copy(order="F")
    pen = tuple(float(dtype(p)) for p in PEN)
    assert na.compute(V, W, H, iterations=iters, parameters=dict(params, l1W=PEN[0], l1H=PEN[1], l2W=PEN[2], l2H=PEN[3]), summary=s) == na.ResultType.Success
    against(W, H, s.record(0), mbref.run(rows, cols, vals, W0, H0, iters, beta, eps_of(dtype), pen=pen))
    # AllRandomValues: reproducible by seed
    outs = []
    for _ in range(2):
        W, H = W0.copy(order="F"), H0.copy(order="F")
        assert na.compute(V, W, H, iterations=15, init=na.NmfInitializationMethod.AllRandomValues, seed=5, parameters=params) == na.ResultType.Success
        assert not np.array_equal(W, W0)
        outs.append((W, H))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    # an RMSD threshold stop: the first test (iteration 20) ends a run of 200
    s2 = na.Summary()
    W, H = W0.copy(order="F"), H0.copy(order="F")
    assert na.compute(V, W, H, iterations=200, threshold_type=na.NmfThresholdType.RMSD, threshold=1e3, parameters=params, summary=s2) == na.ResultType.Success
    assert s2.record(0).numIterations == 20
    s.destroy(); s2.destroy()
    del keep


def test_compute_refusals(ctx):
    m, n, r = 60, 40, 4
    rows, cols, vals = mref.planted_ratings(m, n, 0.3, seed=101)
    D = np.full((m, n), np.nan, dtype=np.float32); D[rows, cols] = vals
    V = F(D)
    W0, H0 = start(m, n, r, np.float32, seed=102)
    bad = na.ResultType.ErrorInvalidArgument

    def go(Vd, params, **kw):
        W, H = W0.copy(order="F"), H0.copy(order="F")
        res = na.compute(Vd, W, H, iterations=5, parameters=params, **kw)
        if res != na.ResultType.Success:
            assert np.array_equal(W, W0) and np.array_equal(H, H0)
        return res

    on = {"missingValues": 1, "missingDivergence": 1}
    assert go(V, on) == na.ResultType.Success
    assert go(V, {"missingValues": 1, "missingDivergence": 3, "missingBeta": 0.5, "l1W": 0.1}) == na.ResultType.Success
    assert go(V, {"missingValues": 1, "l1W": 0.1}) == bad                 # (the Frobenius masked engine keeps refusing penalties)
    assert go(V, {"missingDivergence": 1}) == bad
    assert go(V, {"missingValues": 0, "missingDivergence": 1}) == bad
    for value in (4, -1, 0.5, float("nan")):
        assert go(V, {"missingValues": 1, "missingDivergence": value}) == bad
    assert go(V, {**on, "missingBeta": 0.5}) == bad
    assert go(V, {"missingValues": 1, "missingDivergence": 3, "missingBeta": float("inf")}) == bad
    assert go(V, {"missingValues": 1, "missingDivergence": 3, "missingBeta": 1e300}) == bad
    assert go(V, {**on, "divergence": 1}) == bad
    assert go(V, {**on, "divergence": 3, "beta": 0.5}) == bad
    assert go(V, on, algorithm=na.NmfAlgorithm.HALS) == bad
    assert go(V, {**on, "lambda": 0.1}, algorithm=na.NmfAlgorithm.GDCLS) == bad
    assert go(V, {**on, "numGpus": 2}) == bad
    for init in (na.NmfInitializationMethod.MeanColumns, na.NmfInitializationMethod.KMeansAndRandomValues, na.NmfInitializationMethod.EInNMF):
        assert go(V, on, init=init) == bad
    assert go(V, {**on, "nndsvd": 1}) == bad
    assert go(V, {**on, "l1W": -1.0}) == bad
    # the value rule: a stored zero at beta <= 0, a negative value at beta > 0
    Dz = D.copy(); Dz[rows[0], cols[0]] = 0.0
    assert go(F(Dz), {"missingValues": 1, "missingDivergence": 2}) == bad
    assert go(F(Dz), on) == na.ResultType.Success
    Dn = D.copy(); Dn[rows[0], cols[0]] = -1.0
    assert go(F(Dn), on) == bad
    Vw = F(np.random.default_rng(103).random((300, 280)).astype(np.float32))
    Ww = F(np.ones((300, 257), np.float32)); Hw = F(np.ones((257, 280), np.float32))
    assert na.compute(Vw, Ww, Hw, iterations=2, parameters=on) == bad


# 9. refusals at creation; the three-phase and sharded calls; the penalties' door
def test_engine_refusals():
    m, n, r = 90, 70, 6
    for kw, text in ((dict(missing_divergence="kl"), "missing-value divergence: 'missingDivergence' needs 'missingValues' = 1"),
                     (dict(missing_values=True, missing_divergence="kl", divergence="kl"), "missing-value divergence: does not combine with 'divergence'"),
                     (dict(missing_values=True, missing_divergence="kl", algorithm="hals"), "missing-value divergence: the Multiplicative algorithm only"),
                     (dict(missing_values=True, missing_divergence="beta", missing_beta=1e300), "missing-value divergence: 'missingBeta' out of the range of the engine's precision"),
                     (dict(missing_values=True, missing_divergence="kl", row_blocks=2), "missing-value divergence: single GPU only (no row blocks)")):
        with pytest.raises(na.EngineError) as err:
            na.Engine(m, n, r, **dict(dict(algorithm="mu"), **kw))
        assert err.value.status == 1 and text in str(err.value), str(err.value)
    with pytest.raises(na.EngineError) as err:
        na.Engine(m, n, 257, "mu", missing_values=True, missing_divergence="kl")
    assert "missing-value divergence: rank <= 256" in str(err.value)
    # the Frobenius masked engine keeps refusing penalties; a masked divergence engine takes them
    with pytest.raises(na.EngineError):
        na.Engine(m, n, r, "mu", missing_values=True, l1_w=0.1)
    rows, cols, vals = mref.planted_ratings(m, n, 0.3, seed=111)
    eng = engine(m, n, r, np.float32, 1.0)
    with pytest.raises(na.EngineError):      # nothing uploaded yet
        eng.iterate(1, first_iteration=1, error_every=0, last_iteration=1)
    upload_csr(eng, rows, cols, vals, m)
    W0, H0 = start(m, n, r, np.float32, seed=112)
    eng.set_factors(W0, H0)
    eng.set_penalties(0.1, 0.0, 0.0, 0.2)
    with pytest.raises(na.EngineError):
        eng.set_penalties(-0.1, 0.0, 0.0, 0.0)
    eng.set_penalties(0.0, 0.0, 0.0, 0.0)
    import torch
    ex = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")
    for call in (lambda: eng.h_step(True), lambda: eng.w_products(ex.data_ptr()), lambda: eng.w_finish(ex.data_ptr(), True)):
        with pytest.raises(na.EngineError) as e:
            call()
        assert e.value.status == 1
    group = na.LocalGroup(1)
    comm = na.LocalComm(group, 0)
    with pytest.raises(na.EngineError) as e:
        na.ShardedRun(eng, comm, m, n, na.SHARD_REPLICATED)
    assert e.value.status == 1
    comm.close()
    # the engine itself is unharmed
    eng.iterate(3, first_iteration=1, error_every=0, last_iteration=3)
    assert np.isfinite(eng.divergence_value) and eng.divergence_value > 0 and np.isfinite(eng.frobenius)
    eng.close()


# 10. the general selector at beta 0 and 1 is the Itakura-Saito and the KL engine, bit for bit; a repeated run is bit-identical
@pytest.mark.parametrize("dtype", DTYPES)
def test_routing_of_beta_0_and_1_and_reproducibility(dtype):
    m, n, r, iters = 150, 110, 70, 12
    rows, cols, vals = mref.planted_ratings(m, n, 0.3, seed=121)
    W0, H0 = start(m, n, r, dtype, seed=122)

    def go(**kw):
        eng = na.Engine(m, n, r, "mu", dtype=dtype, missing_values=True, **kw)
        upload_csr(eng, rows, cols, vals, m)
        out = run_engine(eng, W0, H0, iters)
        eng.close()
        return out

    for named, beta in (("is", 0.0), ("kl", 1.0)):
        a, b, c = go(missing_divergence=named), go(missing_divergence="beta", missing_beta=beta), go(missing_divergence=named)
        for x in (b, c):
            assert np.array_equal(a[0], x[0]) and np.array_equal(a[1], x[1]) and a[2:] == x[2:]
    # a beta that rounds to 1 in the engine's precision is the KL engine
    if dtype == np.float32:
        a, b = go(missing_divergence="kl"), go(missing_divergence="beta", missing_beta=1.0 + 1e-12)
        assert np.array_equal(a[0], b[0]) and a[2:] == b[2:]


# 11. what it is for: counts observed at 30 % of the entries, a Poisson model
def test_masked_kl_on_planted_poisson_counts():
    m, n, k, iters = 400, 300, 5, 300
    rng = np.random.default_rng(131)
    rate = 8.0 * rng.random((m, k)) @ rng.random((k, n))      # mean rate about 10
    counts = rng.poisson(rate).astype(np.float64)
    mask = rng.random((m, n)) < 0.3
    rows, cols = np.nonzero(mask)
    vals = counts[rows, cols]
    hr, hc = np.nonzero(~mask)
    eps = eps_of(np.float32)
    fits = {}
    for name, kw in (("masked kl", dict(missing_values=True, missing_divergence="kl")), ("masked frobenius", dict(missing_values=True)),
                     ("plain kl", dict(sparse_compute=True, divergence="kl"))):
        eng = na.Engine(m, n, k, "mu", dtype=np.float32, **kw)
        upload_csr(eng, rows, cols, vals, m)
        eng.randomize(7)
        eng.iterate(iters, first_iteration=1, error_every=0, last_iteration=iters)
        W, H = eng.get_factors()
        assert np.all(np.isfinite(W)) and np.all(np.isfinite(H))
        fits[name] = (mbref.divergence(rows, cols, vals, W, H, 1.0, eps), mbref.divergence(hr, hc, counts[hr, hc], W, H, 1.0, eps))
        if name == "masked kl":
            assert eng.divergence_value == pytest.approx(fits[name][0], rel=1e-4)
        eng.close()
    print({k: (f"{v[0]:.4e}", f"{v[1]:.4e}") for k, v in fits.items()})
    # over the observed entries the KL fit has the lower KL divergence than the least-squares fit of the same entries
    assert fits["masked kl"][0] < fits["masked frobenius"][0], fits
    # held out: below a quarter of what plain sparse KL (unstored = 0) reaches -- the ratio of test_gpu_masked.py's Frobenius pair
    assert fits["masked kl"][1] < 0.25 * fits["plain kl"][1], fits
