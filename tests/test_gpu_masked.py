"""Missing-value NMF on the GPU (docs/MISSING.md): the masked multiplicative update over the observed entries, against the fp64 restatement
(tests/masked_reference.py), the C oracle, and plain sparse MU; every input form, edge rows and columns, constant W, nmfgpu::compute with
Parameter "missingValues", and the refusals of the three-phase and sharded forms."""
import numpy as np
import pytest

import nmfgpu_amd as na
from nmfgpu_amd import api
from oracle import oracle
from tests import masked_reference as ref

pytestmark = pytest.mark.gpu

TOL = {np.float32: (2e-4, 1e-5), np.float64: (1e-9, 1e-9)}       # factors, error


def F(a):
    return np.asfortranarray(a)


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def eps_of(dtype):
    return float(np.finfo(dtype).eps)


def start(m, n, r, dtype, seed):
    rng = np.random.default_rng(seed)
    return F((1.0 - rng.random((m, r))).astype(dtype)), F((1.0 - rng.random((r, n))).astype(dtype))


def masked_engine(m, n, r, dtype):
    return na.Engine(m, n, r, "mu", dtype=dtype, missing_values=True)


def upload_csr(eng, rows, cols, vals, m, base=0):
    ptr, idx, v = ref.csr_of(rows, cols, vals, m)
    eng.upload_sparse(1, v.astype(eng.dtype), ptr + base, idx + base, base)


def run_engine(eng, W0, H0, iters, constant_w=False):
    eng.set_factors(W0, H0)
    eng.iterate(iters, first_iteration=1, error_every=0, last_iteration=iters, constant_w=constant_w)
    W, H = eng.get_factors()
    return W, H, eng.frobenius, eng.rmsd


def check_against_restatement(got, want, dtype):
    ftol, etol = TOL[dtype]
    Wg, Hg, fg, rg = got
    Wr, Hr, fr, rr = want
    assert np.all(np.isfinite(Wg)) and np.all(np.isfinite(Hg))
    assert rel(Wg, Wr) < ftol and rel(Hg, Hr) < ftol, (rel(Wg, Wr), rel(Hg, Hr))
    assert fg == pytest.approx(fr, rel=etol) and rg == pytest.approx(rr, rel=etol)


@pytest.fixture(scope="module")
def ctx():
    assert na.initialize() in (na.ResultType.Success, na.ResultType.ErrorAlreadyInitialized)
    na.set_verbosity(na.Verbosity.Nothing)
    yield
    na.finalize()


# 1. parity: every instantiation (padded rank 64 / 128 / 256 = VEC 1 / 2 / 4), ragged shapes, sparse to complete
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("r", [8, 64, 65, 128, 129, 256])
@pytest.mark.parametrize("density", [0.02, 0.3, 1.0])
def test_parity_with_restatement(dtype, r, density):
    m, n, iters = 131 + r % 7, 97 + r % 5, 20
    rows, cols, vals = ref.planted_ratings(m, n, density, seed=r + int(100 * density))
    W0, H0 = start(m, n, r, dtype, seed=r)
    eng = masked_engine(m, n, r, dtype)
    assert eng.geometry()["padded_rank"] == (64 if r <= 64 else 128 if r <= 128 else 256)
    upload_csr(eng, rows, cols, vals, m)
    got = run_engine(eng, W0, H0, iters)
    want = ref.run(rows, cols, vals, W0, H0, iters, eps_of(dtype))
    check_against_restatement(got, want, dtype)
    # padding coordinates stay exactly zero
    rp = eng.geometry()["padded_rank"]
    Hp = eng.debug_read(1, rp * n).reshape(n, rp)
    assert np.all(Hp[:, r:] == 0)
    eng.close()


# 2. every entry observed: the reference's multiplicative update
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_complete_omega_is_the_oracle_mu(dtype):
    m, n, r, iters = 150, 110, 12, 20
    rng = np.random.default_rng(2)
    V = F(rng.random((m, n)).astype(dtype))
    W0, H0 = start(m, n, r, dtype, seed=3)
    eng = masked_engine(m, n, r, dtype)
    eng.upload(V)
    got = run_engine(eng, W0, H0, iters)
    W64, H64 = F(W0.astype(np.float64)), F(H0.astype(np.float64))
    res = oracle.run("mu", F(V.astype(np.float64)), W64, H64, iters)
    ftol, etol = TOL[dtype]
    assert rel(got[0], W64) < ftol and rel(got[1], H64) < ftol
    # (the oracle's error comes from the trace formula: its own cancellation bounds the fp64 comparison)
    assert got[2] == pytest.approx(res["frobenius"], rel=max(etol, 1e-8)) and got[3] == pytest.approx(res["rmsd"], rel=max(etol, 1e-8))
    eng.close()


# 3. a stored zero is an observation
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_stored_zeros_are_observed(dtype):
    m, n, r, iters = 120, 90, 6, 20
    rows, cols, vals = ref.planted_ratings(m, n, 0.25, seed=31)
    rng = np.random.default_rng(32)
    zr, zc = rng.integers(0, m, 400), rng.integers(0, n, 400)
    taken = set(zip(rows.tolist(), cols.tolist()))
    keep = np.array([(i, j) not in taken for i, j in zip(zr.tolist(), zc.tolist())])
    pairs = sorted(set(zip(zr[keep].tolist(), zc[keep].tolist())))
    zr, zc = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    rows_z, cols_z, vals_z = np.append(rows, zr), np.append(cols, zc), np.append(vals, np.zeros(len(zr)))
    W0, H0 = start(m, n, r, dtype, seed=33)
    results = []
    for R, Cc, Vv in ((rows, cols, vals), (rows_z, cols_z, vals_z)):
        eng = masked_engine(m, n, r, dtype)
        upload_csr(eng, R, Cc, Vv, m)
        got = run_engine(eng, W0, H0, iters)
        check_against_restatement(got, ref.run(R, Cc, Vv, W0, H0, iters, eps_of(dtype)), dtype)
        results.append(got)
        eng.close()
    assert rel(results[0][1], results[1][1]) > 1e-2
    assert results[1][3] == pytest.approx(results[1][2] / np.sqrt(len(vals_z)), rel=1e-12)


# 4. the same Omega through every input form: bit-identical; a repeated run too
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_input_form_is_bit_identical(dtype):
    m, n, r, iters = 173, 141, 10, 12
    rows, cols, vals = ref.planted_ratings(m, n, 0.2, seed=41)
    vals = vals.astype(dtype)
    W0, H0 = start(m, n, r, dtype, seed=42)
    outs = []

    def go(upload):
        eng = masked_engine(m, n, r, dtype)
        upload(eng)
        out = run_engine(eng, W0, H0, iters)
        eng.close()
        outs.append(out)

    D = np.full((m, n), np.nan, dtype=dtype); D[rows, cols] = vals
    go(lambda e: e.upload(F(D)))
    for base in (0, 1):
        go(lambda e: upload_csr(e, rows, cols, vals, m, base))
        cp, ci, cv = ref.csc_of(rows, cols, vals, n)
        go(lambda e: e.upload_sparse(2, cv.astype(dtype), cp + base, ci + base, base))
        perm = np.random.default_rng(43 + base).permutation(len(vals))
        go(lambda e: e.upload_sparse(3, vals[perm], (rows[perm] + base).astype(np.int32), (cols[perm] + base).astype(np.int32), base))
    go(lambda e: upload_csr(e, rows, cols, vals, m))
    for o in outs[1:]:
        assert np.array_equal(o[0], outs[0][0]) and np.array_equal(o[1], outs[0][1])
        assert o[2] == outs[0][2] and o[3] == outs[0][3]


# 5. empty rows and columns, duplicated COO entries
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("r", [5, 100, 200])
def test_edge_rows_columns_and_duplicates(dtype, r):
    m, n, iters = 150, 120, 20
    rows, cols, vals = ref.planted_ratings(m, n, 0.3, seed=51 + r)
    keep = (rows % 17 != 3) & (cols % 13 != 5)
    rows, cols, vals = rows[keep], cols[keep], vals[keep]
    rng = np.random.default_rng(52)
    d = rng.choice(len(vals), 60, replace=False)
    rows, cols, vals = np.append(rows, rows[d]), np.append(cols, cols[d]), np.append(vals, rng.integers(1, 6, 60).astype(np.float64))
    perm = rng.permutation(len(vals))
    W0, H0 = start(m, n, r, dtype, seed=53)
    eng = masked_engine(m, n, r, dtype)
    eng.upload_sparse(3, vals[perm].astype(dtype), rows[perm].astype(np.int32), cols[perm].astype(np.int32), 0)
    got = run_engine(eng, W0, H0, iters)
    check_against_restatement(got, ref.run(rows, cols, vals, W0, H0, iters, eps_of(dtype)), dtype)
    Wg, Hg = got[0], got[1]
    assert np.all(Wg[np.arange(m) % 17 == 3] == 0) and np.all(Hg[:, np.arange(n) % 13 == 5] == 0)
    assert np.all(Wg >= 0) and np.all(Hg >= 0)
    eng.close()


# 6. capability: a planted low-rank matrix seen at 30 % of its entries
def test_held_out_error_beats_plain_sparse_mu():
    m, n, k, iters = 400, 300, 5, 300
    rng = np.random.default_rng(61)
    V0 = rng.random((m, k)) @ rng.random((k, n))
    mask = rng.random((m, n)) < 0.3
    rows, cols = np.nonzero(mask)
    vals = V0[rows, cols].astype(np.float32)
    held = ~mask
    rmse = {}
    for name, kw in (("masked", dict(missing_values=True)), ("plain", dict(sparse_compute=True))):
        eng = na.Engine(m, n, k, "mu", dtype=np.float32, **kw)
        upload_csr(eng, rows, cols, vals, m)
        eng.randomize(7)
        eng.iterate(iters, first_iteration=1, error_every=0, last_iteration=iters)
        W, H = eng.get_factors()
        assert np.all(np.isfinite(W)) and np.all(np.isfinite(H))
        rmse[name] = float(np.sqrt(np.mean(((W.astype(np.float64) @ H.astype(np.float64)) - V0)[held] ** 2)))
        eng.close()
    assert rmse["masked"] < 0.25 * rmse["plain"], rmse


# 7. constant W: the H step, and the error from the residual-only pass
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("r", [16, 128, 200])
def test_constant_w(dtype, r):
    m, n, iters = 140, 100, 10
    rows, cols, vals = ref.planted_ratings(m, n, 0.3, seed=71 + r)
    W0, H0 = start(m, n, r, dtype, seed=72)
    eng = masked_engine(m, n, r, dtype)
    upload_csr(eng, rows, cols, vals, m)
    got = run_engine(eng, W0, H0, iters, constant_w=True)
    assert np.array_equal(got[0], W0)
    want = ref.run(rows, cols, vals, W0, H0, iters, eps_of(dtype), const_w=True)
    check_against_restatement(got, want, dtype)
    eng.close()


# 8. nmfgpu::compute with Parameter "missingValues"
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("form", ["dense", "csr"])
def test_compute_with_missing_values(ctx, dtype, form):
    m, n, r, iters = 160, 120, 7, 20
    rows, cols, vals = ref.planted_ratings(m, n, 0.35, seed=81)
    W0, H0 = start(m, n, r, dtype, seed=82)
    keep = []
    if form == "dense":
        D = np.full((m, n), np.nan, dtype=dtype); D[rows, cols] = vals
        V = F(D)
    else:
        ptr, idx, v = ref.csr_of(rows, cols, vals, m)
        v = v.astype(dtype); keep = [ptr, idx, v]
        V = api.sparse_description(na.StorageFormat.CSR, m, n, v, ptr, idx)
    W, H = W0.copy(order="F"), H0.copy(order="F")
    s = na.Summary()
    assert na.compute(V, W, H, iterations=iters, parameters={"missingValues": 1}, summary=s) == na.ResultType.Success
    want = ref.run(rows, cols, vals, W0, H0, iters, eps_of(dtype))
    rec = s.record(0)
    check_against_restatement((W, H, rec.frobenius, rec.rmsd), want, dtype)
    assert rec.rmsd == pytest.approx(rec.frobenius / np.sqrt(len(vals)), rel=1e-12)
    assert rec.numIterations == iters
    # AllRandomValues: reproducible by seed
    outs = []
    for _ in range(2):
        W, H = W0.copy(order="F"), H0.copy(order="F")
        assert na.compute(V, W, H, iterations=15, init=na.NmfInitializationMethod.AllRandomValues, seed=5,
                          parameters={"missingValues": 1}) == na.ResultType.Success
        assert not np.array_equal(W, W0)
        outs.append((W, H))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    # an RMSD threshold stop: the first test (iteration 20) ends a run of 200
    s2 = na.Summary()
    W, H = W0.copy(order="F"), H0.copy(order="F")
    assert na.compute(V, W, H, iterations=200, threshold_type=na.NmfThresholdType.RMSD, threshold=1e3, parameters={"missingValues": 1},
                      summary=s2) == na.ResultType.Success
    assert s2.record(0).numIterations == 20
    s.destroy(); s2.destroy()
    del keep


def test_compute_refusals(ctx):
    m, n, r = 60, 40, 4
    rows, cols, vals = ref.planted_ratings(m, n, 0.3, seed=91)
    D = np.full((m, n), np.nan, dtype=np.float32); D[rows, cols] = vals
    V = F(D)
    W0, H0 = start(m, n, r, np.float32, seed=92)
    bad = na.ResultType.ErrorInvalidArgument

    def go(Vd, params, **kw):
        W, H = W0.copy(order="F"), H0.copy(order="F")
        res = na.compute(Vd, W, H, iterations=5, parameters=params, **kw)
        if res != na.ResultType.Success:
            assert np.array_equal(W, W0) and np.array_equal(H, H0)
        return res

    on = {"missingValues": 1}
    assert go(V, on) == na.ResultType.Success
    assert go(V, {"missingValues": 0}) != bad           # (today's behaviour: NaN then reaches the dense path)
    assert go(V, {**on, "lambda": 0.1}, algorithm=na.NmfAlgorithm.GDCLS) == bad
    assert go(V, on, algorithm=na.NmfAlgorithm.HALS) == bad
    assert go(V, {**on, "divergence": 1}) == bad
    assert go(V, {**on, "numGpus": 2}) == bad
    for init in (na.NmfInitializationMethod.MeanColumns, na.NmfInitializationMethod.KMeansAndRandomValues,
                 na.NmfInitializationMethod.KMeansAndAbsoluteWTV, na.NmfInitializationMethod.KMeansAndNonNegativeWTV, na.NmfInitializationMethod.EInNMF):
        assert go(V, on, init=init) == bad
    assert go(V, {**on, "nndsvd": 1}) == bad
    for value in (2, -1, 0.5):
        assert go(V, {"missingValues": value}) == bad
    assert go(F(np.full((m, n), np.nan, dtype=np.float32)), on) == bad
    ptr, idx, v = ref.csr_of(rows, cols, vals, m)
    v = v.astype(np.float32)
    empty = api.sparse_description(na.StorageFormat.CSR, m, n, v[:0], np.zeros(m + 1, np.int32), idx[:0])
    assert go(empty, on) == bad
    vinf = v.copy(); vinf[3] = np.inf
    assert go(api.sparse_description(na.StorageFormat.CSR, m, n, vinf, ptr, idx), on) == bad
    Dinf = D.copy(); Dinf[rows[0], cols[0]] = -np.inf
    assert go(F(Dinf), on) == bad
    Vw = F(np.random.default_rng(93).random((300, 280)).astype(np.float32))
    Ww = F(np.ones((300, 257), np.float32)); Hw = F(np.ones((257, 280), np.float32))
    assert na.compute(Vw, Ww, Hw, iterations=2, parameters=on) == bad


# 9. no three-phase or sharded form
def test_engine_refuses_three_phase_and_sharded_forms():
    m, n, r = 90, 70, 6
    rows, cols, vals = ref.planted_ratings(m, n, 0.3, seed=101)
    eng = masked_engine(m, n, r, np.float32)
    upload_csr(eng, rows, cols, vals, m)
    W0, H0 = start(m, n, r, np.float32, seed=102)
    eng.set_factors(W0, H0)
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
    assert np.isfinite(eng.frobenius) and eng.frobenius > 0
    eng.close()


# 10. medium size: config 3's shape scaled by 1 / 20
def test_medium_size():
    m, n, r = 20000, 5000, 128
    rng = np.random.default_rng(111)
    nnz = m * n // 100
    flat = np.unique(rng.integers(0, m * n, nnz))
    rows, cols = flat // n, flat % n
    vals = rng.integers(1, 6, len(flat)).astype(np.float64)
    W0, H0 = start(m, n, r, np.float64, seed=112)
    eng = masked_engine(m, n, r, np.float64)
    upload_csr(eng, rows, cols, vals, m)
    got = run_engine(eng, W0, H0, 5)
    eng.close()
    check_against_restatement(got, ref.run(rows, cols, vals, W0, H0, 5, eps_of(np.float64), chunk=1 << 15), np.float64)
    eng = masked_engine(m, n, r, np.float32)
    upload_csr(eng, rows, cols, vals, m)
    W, H, frob, _ = run_engine(eng, W0.astype(np.float32, order="F"), H0.astype(np.float32, order="F"), 50)
    eng.close()
    assert np.all(np.isfinite(W)) and np.all(np.isfinite(H)) and np.all(W >= 0) and np.all(H >= 0) and np.isfinite(frob)
    norms = np.linalg.norm(W.astype(np.float64), axis=0)
    assert np.allclose(norms, 1.0, atol=1e-4)
