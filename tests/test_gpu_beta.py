"""Dense beta-divergence NMF on the GPU (docs/DIVERGENCE.md): the Itakura-Saito (beta = 0) and dense generalised-KL (beta = 1) multiplicative updates against
the numpy restatement (tests/beta_reference.py), the C oracle's KL iteration and the sparse KL engine; several reduction slabs, reproducibility, monotonicity,
constant W, the kernel entry at every instantiation, nmfgpu::compute with Parameter "divergence" = 2, and the refusals.

Tolerances: fp64 1e-9 on factors, errors and the divergence value; fp32 the project's standing 2e-4 on factors and 1e-5 on the errors (tests/test_gpu_masked.py) --
the divergence value included: numpy's own fp32 run of the restatement differs from its fp64 run by 1.4e-6 on the factors and 8e-8 on the divergence on these
problems, two orders inside."""
import numpy as np
import pytest

import nmfgpu_amd as na
from oracle import oracle
from tests import beta_reference as ref

pytestmark = pytest.mark.gpu

TOL = {np.float32: (2e-4, 1e-5), np.float64: (1e-9, 1e-9)}       # factors, errors (frobenius, rmsd, divergence)
DIV = {0: "is", 1: "kl"}


def F(a):
    return np.asfortranarray(a)


def rel(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b), 1e-300))


def eps_of(dtype):
    return float(np.finfo(dtype).eps)


def problem(m, n, r, dtype, seed):
    V = F(ref.planted(m, n, seed=seed).astype(dtype))
    W0, H0 = ref.start(m, n, r, seed + 1, dtype)
    return V, W0, H0


def beta_engine(m, n, r, dtype, beta):
    return na.Engine(m, n, r, "mu", dtype=dtype, divergence=DIV[beta], dense_compute=(beta == 1))


def run_engine(eng, W0, H0, iters, constant_w=False):
    eng.set_factors(W0, H0)
    eng.iterate(iters, first_iteration=1, error_every=0, last_iteration=iters, constant_w=constant_w)
    W, H = eng.get_factors()
    return W, H, eng.frobenius, eng.rmsd, eng.divergence_value


def check(got, want, dtype, what=""):
    ftol, etol = TOL[dtype]
    figures = (rel(got[0], want[0]), rel(got[1], want[1]), abs(got[2] / want[2] - 1), abs(got[3] / want[3] - 1), abs(got[4] / want[4] - 1))
    print(f"{what} {np.dtype(dtype).name}: W {figures[0]:.2e} H {figures[1]:.2e} frobenius {figures[2]:.2e} rmsd {figures[3]:.2e} divergence {figures[4]:.2e}")
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1]))
    assert figures[0] < ftol and figures[1] < ftol, figures
    assert figures[2] < etol and figures[3] < etol and figures[4] < etol, figures


def reference(V, W0, H0, iters, beta, dtype, **kw):
    return ref.run(V.astype(np.float64), W0.astype(np.float64), H0.astype(np.float64), iters, beta, eps_of(dtype), **kw)


@pytest.fixture(scope="module")
def ctx():
    assert na.initialize() in (na.ResultType.Success, na.ResultType.ErrorAlreadyInitialized)
    na.set_verbosity(na.Verbosity.Nothing)
    yield
    na.finalize()


# 1. parity with the restatement: every padded rank (64 / 128 / 256), ragged shapes, padding exactly zero
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("r", [8, 64, 65, 128, 129, 256])
@pytest.mark.parametrize("beta", [0, 1])
def test_parity_with_restatement(beta, r, dtype):
    m, n, iters = 131 + r % 7, 97 + r % 5, 20
    V, W0, H0 = problem(m, n, r, dtype, seed=r + beta)
    eng = beta_engine(m, n, r, dtype, beta)
    g = eng.geometry()
    rp = g["padded_rank"]
    assert rp == (64 if r <= 64 else 128 if r <= 128 else 256)
    assert g["product_kernel"] == 6 and g["resident_images"] == 2 and g["kl_blocks_w"] == 0 and g["kl_blocks_h"] == 0 and g["exchange_count"] == 0
    assert g["slabs_h"] >= 1 and g["slabs_w"] >= 1
    eng.upload(V)
    got = run_engine(eng, W0, H0, iters)
    check(got, reference(V, W0, H0, iters, beta, dtype), dtype, f"beta {beta} r {r}")
    if beta == 1:
        assert eng.kl_divergence == got[4]
    Hp = eng.debug_read(1, rp * g["padded_n"]).reshape(g["padded_n"], rp)
    Wp = eng.debug_read(0, rp * g["padded_m"]).reshape(g["padded_m"], rp)
    assert np.all(Hp[:, r:] == 0) and np.all(Hp[n:] == 0) and np.all(Wp[:, r:] == 0) and np.all(Wp[m:] == 0)
    assert np.all(Hp[:n, :r] >= 0) and np.all(Wp[:m, :r] >= 0)
    eng.close()


# 2. dense KL: the oracle's iteration, the sparse KL engine's, and a V with zeros
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dense_kl_is_the_oracle_and_the_sparse_engine(dtype):
    m, n, r, iters = 150, 110, 12, 20
    V, W0, H0 = problem(m, n, r, dtype, seed=21)
    eng = beta_engine(m, n, r, dtype, 1)
    eng.upload(V)
    got = run_engine(eng, W0, H0, iters)
    eng.close()
    W64, H64 = F(W0.astype(np.float64)), F(H0.astype(np.float64))
    res = oracle.run_kl(F(V.astype(np.float64)), W64, H64, iters)
    ftol, etol = TOL[dtype]
    assert rel(got[0], W64) < ftol and rel(got[1], H64) < ftol
    print(f"dense KL against oracle.run_kl {np.dtype(dtype).name}: W {rel(got[0], W64):.2e} H {rel(got[1], H64):.2e} frobenius {abs(got[2] / res['frobenius'] - 1):.2e} "
          f"rmsd {abs(got[3] / res['rmsd'] - 1):.2e} kl {abs(got[4] / res['kl'] - 1):.2e}")
    assert got[2] == pytest.approx(res["frobenius"], rel=etol) and got[3] == pytest.approx(res["rmsd"], rel=etol)
    assert got[4] == pytest.approx(res["kl"], rel=etol)
    sp = na.Engine(m, n, r, "mu", dtype=dtype, divergence="kl")
    assert sp.geometry()["product_kernel"] == 5
    sp.upload(V)
    sp.set_factors(W0, H0)
    sp.iterate(iters, first_iteration=1, error_every=0, last_iteration=iters)
    Ws, Hs = sp.get_factors()
    print(f"dense against sparse KL {np.dtype(dtype).name}: W {rel(got[0], Ws.astype(np.float64)):.2e} H {rel(got[1], Hs.astype(np.float64)):.2e} "
          f"kl {abs(got[4] / sp.kl_divergence - 1):.2e} frobenius {abs(got[2] / sp.frobenius - 1):.2e} rmsd {abs(got[3] / sp.rmsd - 1):.2e}")
    assert rel(got[0], Ws.astype(np.float64)) < ftol and rel(got[1], Hs.astype(np.float64)) < ftol
    assert got[4] == pytest.approx(sp.kl_divergence, rel=etol) and sp.divergence_value == sp.kl_divergence
    # fp64: 1e-9 on everything.  fp32: the sparse engine resolves ||V||^2 - 2 tr + tr from fp32 terms, so the rounding of its terms (the 1e-5 the errors are held to)
    # reaches its squared error amplified by ||V||^2 / frobenius^2, and its root by half of that
    amp = 1.0 if dtype == np.float64 else max(1.0, 0.5 * float(np.linalg.norm(V.astype(np.float64)) / got[2]) ** 2)
    assert got[2] == pytest.approx(sp.frobenius, rel=etol * amp) and got[3] == pytest.approx(sp.rmsd, rel=etol * amp)
    sp.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("form", ["dense", "csr"])
def test_dense_kl_with_zeros(dtype, form):
    m, n, r, iters = 140, 120, 9, 20
    V, W0, H0 = problem(m, n, r, dtype, seed=31)
    V[np.random.default_rng(32).random((m, n)) < 0.4] = 0
    eng = beta_engine(m, n, r, dtype, 1)
    if form == "dense":
        eng.upload(V)
    else:
        # sparse input on a dense-KL engine is densified
        rows, cols = np.nonzero(V)
        order = np.lexsort((cols, rows))
        rows, cols = rows[order], cols[order]
        ptr = np.zeros(m + 1, np.int32); np.add.at(ptr, rows + 1, 1); ptr = np.cumsum(ptr).astype(np.int32)
        eng.upload_sparse(1, V[rows, cols], ptr, cols.astype(np.int32), 0)
    got = run_engine(eng, W0, H0, iters)
    check(got, reference(V, W0, H0, iters, 1, dtype), dtype, f"KL with zeros ({form})")
    eng.close()


# 3. more than one reduction slab in each half-step; a repeated run is bit-identical
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("beta", [0, 1])
@pytest.mark.parametrize("shape", [(3000, 70), (70, 3000)])
def test_reduction_slabs(shape, beta, dtype):
    (m, n), r, iters = shape, 8, 20
    V, W0, H0 = problem(m, n, r, dtype, seed=41 + beta)
    outs = []
    for _ in range(2):
        eng = beta_engine(m, n, r, dtype, beta)
        g = eng.geometry()
        assert (g["slabs_h"] if m > n else g["slabs_w"]) > 1, g
        eng.upload(V)
        outs.append(run_engine(eng, W0, H0, iters))
        eng.close()
    check(outs[0], reference(V, W0, H0, iters, beta, dtype), dtype, f"slabs {shape} beta {beta}")
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert outs[0][2:] == outs[1][2:]


# 4. the Itakura-Saito divergence never rises (the compensated normalisation leaves W H as it is)
@pytest.mark.parametrize("dtype,slack", [(np.float64, 1e-12), (np.float32, 1e-5)])
def test_itakura_saito_is_non_increasing(dtype, slack):
    m, n, r = 200, 150, 10
    V, W0, H0 = problem(m, n, r, dtype, seed=51)
    eng = beta_engine(m, n, r, dtype, 0)
    eng.upload(V)
    eng.set_factors(W0, H0)
    hist = []
    for it in range(1, 41):
        eng.iterate(1, first_iteration=it, error_every=1)
        hist.append(eng.divergence_value)
    eng.close()
    print(f"IS {np.dtype(dtype).name}: {hist[0]:.6e} -> {hist[-1]:.6e}, largest relative rise {max(b / a - 1 for a, b in zip(hist, hist[1:])):.2e}")
    assert np.all(np.isfinite(hist)) and hist[-1] < 0.9 * hist[0]
    for a, b in zip(hist, hist[1:]):
        assert b <= a * (1 + slack), (a, b)


# 5. constant W: the H step alone, W untouched, the error from the terms-only form of the W-side launch
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("beta", [0, 1])
@pytest.mark.parametrize("r", [16, 200])
def test_constant_w(r, beta, dtype):
    m, n, iters = 140, 100, 10
    V, W0, H0 = problem(m, n, r, dtype, seed=61 + r)
    eng = beta_engine(m, n, r, dtype, beta)
    eng.upload(V)
    got = run_engine(eng, W0, H0, iters, constant_w=True)
    assert np.array_equal(got[0], W0)
    check(got, reference(V, W0, H0, iters, beta, dtype, const_w=True), dtype, f"constant W beta {beta} r {r}")
    assert got[2] > 0 and got[4] > 0
    eng.close()


# 6. the kernel entry: every instantiation (padded rank x precision x beta x form) once, against the restatement's half-step
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("RP", [64, 128, 256])
@pytest.mark.parametrize("beta", [0, 1])
@pytest.mark.parametrize("form", [0, 1, 2])
def test_half_step_kernel(form, beta, RP, dtype):
    out_valid, out_pad, red_valid, red_pad, r = 100, 128, 300, 384, RP - 3
    rng = np.random.default_rng(71 + RP + beta)
    A = np.zeros((out_pad, RP), dtype); A[:out_valid, :r] = 1.0 - rng.random((out_valid, r))
    B = np.zeros((red_pad, RP), dtype); B[:red_valid, :r] = 1.0 - rng.random((red_valid, r))
    X = np.zeros((out_pad, red_pad), dtype); X[:out_valid, :red_valid] = ref.planted(out_valid, red_valid, seed=72).astype(dtype)
    dsum = B.astype(np.float64).sum(axis=0)
    res = na.op_beta_half_step(A, B, X, r, out_valid, red_valid, beta, form, dsum=dsum.astype(dtype), force_slabs=2)
    assert res["slabs"] == 2
    eps = eps_of(dtype)
    A64, B64, X64 = A.astype(np.float64)[:out_valid, :r], B.astype(np.float64)[:red_valid, :r], X.astype(np.float64)[:out_valid, :red_valid]
    tol = 1e-5 if dtype == np.float32 else 1e-12
    if form == 2:
        assert np.array_equal(res["A"], A)
    else:
        want = ref.half_step(X64, A64, B64, beta, eps, dsum=dsum[:r])
        got = res["A"]
        assert rel(got[:out_valid, :r], want) < tol, rel(got[:out_valid, :r], want)
        assert np.all(got[out_valid:] == 0) and np.all(got[:, r:] == 0)
        assert np.allclose(res["sumsq_part"][0, :r], (want ** 2).sum(axis=0), rtol=10 * tol) and np.all(res["sumsq_part"][:, r:] == 0)
        assert np.allclose(res["sum_part"][0, :r], want.sum(axis=0), rtol=10 * tol)
    if form == 0:
        assert res["t_frob"] is None
    else:
        tf, td = ref.terms(X64, A64, B64, beta, eps)
        assert np.allclose(res["t_frob"][:out_valid], tf, rtol=10 * tol) and np.allclose(res["t_div"][:out_valid], td, rtol=10 * tol)
        assert np.all(res["t_frob"][out_valid:] == 0) and np.all(res["t_div"][out_valid:] == 0)
    # the planned slab count gives the same values up to the order of the sums
    if form == 0:
        one = na.op_beta_half_step(A, B, X, r, out_valid, red_valid, beta, form, dsum=dsum.astype(dtype), force_slabs=1)
        assert one["slabs"] == 1 and rel(one["A"], res["A"].astype(np.float64)) < tol
    with pytest.raises(na.EngineError):
        na.op_beta_half_step(A[:, :32], B[:, :32], X, 8, out_valid, red_valid, beta, form, dsum=dsum[:32].astype(dtype))


# 6b. the kernel entry with a leading dimension above the reduction length and two update workgroups (per-workgroup partial sums at blockIdx.x > 0)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("RP", [64, 256])
@pytest.mark.parametrize("beta", [0, 1])
def test_half_step_kernel_leading_dimension_and_parts(beta, RP, dtype):
    out_valid, out_pad, red_valid, red_pad, ldx, r = 200, 256, 150, 256, 384, RP - 5
    rng = np.random.default_rng(75 + RP + beta)
    A = np.zeros((out_pad, RP), dtype); A[:out_valid, :r] = 1.0 - rng.random((out_valid, r))
    B = np.zeros((red_pad, RP), dtype); B[:red_valid, :r] = 1.0 - rng.random((red_valid, r))
    X = np.full((out_pad, ldx), 7.0, dtype)      # (what lies behind red_pad in a row must not be read)
    X[:, :red_pad] = 0
    X[:out_valid, :red_valid] = ref.planted(out_valid, red_valid, seed=76).astype(dtype)
    dsum = B.astype(np.float64).sum(axis=0)
    res = na.op_beta_half_step(A, B, X, r, out_valid, red_valid, beta, 1, dsum=dsum.astype(dtype))
    eps = eps_of(dtype)
    A64, B64, X64 = A.astype(np.float64)[:out_valid, :r], B.astype(np.float64)[:red_valid, :r], X.astype(np.float64)[:out_valid, :red_valid]
    tol = 1e-5 if dtype == np.float32 else 1e-12
    want = ref.half_step(X64, A64, B64, beta, eps, dsum=dsum[:r])
    got = res["A"]
    assert rel(got[:out_valid, :r], want) < tol, rel(got[:out_valid, :r], want)
    assert np.all(got[out_valid:] == 0) and np.all(got[:, r:] == 0)
    assert res["sumsq_part"].shape == (2, RP)
    for part, rows in ((0, slice(0, 128)), (1, slice(128, out_valid))):
        assert np.allclose(res["sumsq_part"][part, :r], (want[rows] ** 2).sum(axis=0), rtol=10 * tol)
        assert np.allclose(res["sum_part"][part, :r], want[rows].sum(axis=0), rtol=10 * tol)
    tf, td = ref.terms(X64, A64, B64, beta, eps)
    assert np.allclose(res["t_frob"][:out_valid], tf, rtol=10 * tol) and np.allclose(res["t_div"][:out_valid], td, rtol=10 * tol)
    assert np.all(res["t_frob"][out_valid:] == 0) and np.all(res["t_div"][out_valid:] == 0)


# 7. nmfgpu::compute with Parameter "divergence" = 2 (and the dense KL form), CopyExisting and a random start
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("params,beta", [({"divergence": 2}, 0), ({"divergence": 1, "denseCompute": 1}, 1)])
def test_compute(ctx, dtype, params, beta):
    m, n, r, iters = 160, 120, 7, 20
    V, W0, H0 = problem(m, n, r, dtype, seed=81)
    W, H = W0.copy(order="F"), H0.copy(order="F")
    s = na.Summary()
    assert na.compute(V, W, H, iterations=iters, parameters=params, summary=s) == na.ResultType.Success
    want = reference(V, W0, H0, iters, beta, dtype)
    rec = s.record(0)
    ftol, etol = TOL[dtype]
    assert rel(W, want[0]) < ftol and rel(H, want[1]) < ftol
    assert rec.frobenius == pytest.approx(want[2], rel=etol) and rec.rmsd == pytest.approx(want[3], rel=etol) and rec.numIterations == iters
    outs = []
    for _ in range(2):
        W, H = W0.copy(order="F"), H0.copy(order="F")
        assert na.compute(V, W, H, iterations=15, init=na.NmfInitializationMethod.AllRandomValues, seed=5, parameters=params) == na.ResultType.Success
        assert not np.array_equal(W, W0) and np.all(np.isfinite(W)) and np.all(np.isfinite(H))
        outs.append((W, H))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    # every initialisation is allowed (V is dense), and constant basis vectors
    W, H = W0.copy(order="F"), H0.copy(order="F")
    assert na.compute(V, W, H, iterations=5, init=na.NmfInitializationMethod.MeanColumns, parameters=params) == na.ResultType.Success
    W, H = W0.copy(order="F"), H0.copy(order="F")
    assert na.compute(V, W, H, iterations=5, constant_basis_vectors=True, parameters=params) == na.ResultType.Success
    assert np.array_equal(W, W0) and rel(H, reference(V, W0, H0, 5, beta, dtype, const_w=True)[1]) < ftol
    s.destroy()


# 8. what an upload refuses
def test_upload_refusals(ctx):
    m, n, r = 60, 40, 4
    V, W0, H0 = problem(m, n, r, np.float32, seed=91)
    bad = na.ResultType.ErrorInvalidArgument

    def upload(beta, Vd):
        eng = beta_engine(m, n, r, np.float32, beta)
        try:
            eng.upload(F(Vd))
            return 0
        except na.EngineError as e:
            assert "finite" in str(e)
            return e.status
        finally:
            eng.close()

    def spoiled(value):
        Vd = V.copy(); Vd[7, 5] = value
        return Vd

    assert upload(0, V) == 0 and upload(1, V) == 0 and upload(1, spoiled(0.0)) == 0
    for value in (0.0, -1.0, np.nan, np.inf):
        assert upload(0, spoiled(value)) == 1
    for value in (-1.0, np.nan, np.inf):
        assert upload(1, spoiled(value)) == 1
    for params, values in (({"divergence": 2}, (0.0, -1.0)), ({"divergence": 1, "denseCompute": 1}, (-1.0, np.nan))):
        for value in values:
            W, H = W0.copy(order="F"), H0.copy(order="F")
            assert na.compute(F(spoiled(value)), W, H, iterations=3, parameters=params) == bad
            assert np.array_equal(W, W0) and np.array_equal(H, H0)
    # sparse input: refused by Itakura-Saito (unstored entries are zeros), a negative stored value by dense KL
    ptr = np.arange(m + 1, dtype=np.int32); idx = np.zeros(m, np.int32); vals = np.ones(m, np.float32)
    eng = beta_engine(m, n, r, np.float32, 0)
    with pytest.raises(na.EngineError) as e:
        eng.upload_sparse(1, vals, ptr, idx, 0)
    assert e.value.status == 1
    # ... and an engine that was refused its V does not iterate
    with pytest.raises(na.EngineError):
        eng.iterate(1)
    eng.close()
    eng = beta_engine(m, n, r, np.float32, 1)
    neg = vals.copy(); neg[3] = -1
    with pytest.raises(na.EngineError) as e:
        eng.upload_sparse(1, neg, ptr, idx, 0)
    assert e.value.status == 1
    eng.upload_sparse(1, vals, ptr, idx, 0)
    eng.close()
    # what the constructor refuses
    for kw in (dict(divergence="is", sparse_compute=True), dict(divergence="is", missing_values=True), dict(divergence="kl", dense_compute=True, sparse_compute=True),
               dict(dense_compute=True), dict(divergence="is", precision="bf16")):
        with pytest.raises(na.EngineError) as e:
            na.Engine(m, n, r, "mu", dtype=np.float32, **kw)
        assert e.value.status == 1
    for alg in ("gdcls", "hals", "nsnmf"):
        with pytest.raises(na.EngineError):
            na.Engine(m, n, r, alg, dtype=np.float32, divergence="is")
    with pytest.raises(na.EngineError):
        na.Engine(300, 280, 257, "mu", dtype=np.float32, divergence="is")


# 9. no three-phase or sharded form
@pytest.mark.parametrize("beta", [0, 1])
def test_engine_refuses_three_phase_and_sharded_forms(beta):
    m, n, r = 90, 70, 6
    V, W0, H0 = problem(m, n, r, np.float32, seed=101)
    eng = beta_engine(m, n, r, np.float32, beta)
    eng.upload(V)
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
    assert np.isfinite(eng.frobenius) and eng.frobenius > 0 and np.isfinite(eng.divergence_value)
    eng.close()


# 10. medium size: several waves of workgroups, both precisions
@pytest.mark.parametrize("beta", [0, 1])
def test_medium_size(beta):
    m, n, r, iters = 2100, 1300, 40, 5
    V, W0, H0 = problem(m, n, r, np.float64, seed=111)
    want = reference(V, W0, H0, iters, beta, np.float64)
    for dtype in (np.float64, np.float32):
        eng = beta_engine(m, n, r, dtype, beta)
        eng.upload(F(V.astype(dtype)))
        got = run_engine(eng, F(W0.astype(dtype)), F(H0.astype(dtype)), iters)
        eng.close()
        w = want if dtype == np.float64 else reference(V.astype(np.float32), W0.astype(np.float32), H0.astype(np.float32), iters, beta, np.float32)
        check(got, w, dtype, f"medium beta {beta}")
