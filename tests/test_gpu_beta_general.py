"""General dense beta-divergence NMF with L1 / L2 penalties on the GPU (docs/DIVERGENCE.md): the engine at beta = -1, 0.5, 1.5, 3 against the numpy restatement
(tests/beta_general_reference.py), the penalties on beta = 0, 1 and 0.5, V with zeros, the routing of beta = 0 and beta = 1 to the Itakura-Saito and dense KL
engines, reproducibility, constant W, the kernel entry at every new instantiation, and nmfgpu::compute with Parameter "divergence" = 3.

Tolerances, the project's standing ones (tests/test_gpu_beta.py): fp64 1e-9 on factors, errors and the divergence value; fp32 2e-4 on the factors and 1e-5 on the
errors and the divergence value.  numpy's own fp32 run of the restatement, with the power taken as exp2(y log2 P) as the kernels take it, differs from its fp64 run by
at most 1.6e-6 on the factors, 9e-8 on the Frobenius error and 2.1e-7 on the divergence value on these problems: two orders inside.  Measured on an MI355X, the
fp32 engine (v_log_f32 / v_exp_f32) against the fp64 restatement: at most 1.3e-6 on the factors (penalised beta = 1), 1.9e-8 on the Frobenius error and 1.4e-6 on the
divergence value (beta = 0.5); the fp64 engine at most 2.8e-15, 4.4e-16 and 1.1e-15.  The kernel entry is held to
tests/test_gpu_beta.py's figures for one half-step: 1e-5 (fp32) and 1e-12 (fp64) on the panel, ten times that on the sums and the per-row terms."""
import numpy as np
import pytest

import nmfgpu_amd as na
from tests import beta_general_reference as gen

pytestmark = pytest.mark.gpu

TOL = {np.float32: (2e-4, 1e-5), np.float64: (1e-9, 1e-9)}       # factors, errors (frobenius, rmsd, divergence)
PEN = (0.05, 0.05, 0.01, 0.01)                                   # (l1W, l1H, l2W, l2H)
DTYPES = [np.float32, np.float64]


def F(a):
    return np.asfortranarray(a)


def rel(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b), 1e-300))


def eps_of(dtype):
    return float(np.finfo(dtype).eps)


def problem(m, n, r, dtype, seed, zeros=0.0):
    V = F(gen.planted(m, n, seed=seed).astype(dtype))
    if zeros:
        V[np.random.default_rng(seed + 1000).random((m, n)) < zeros] = 0
    W0, H0 = gen.start(m, n, r, seed + 1, dtype)
    return V, W0, H0


def engine(m, n, r, dtype, beta, pen=gen.NO_PENALTIES):
    """The engine of a beta: "is" and dense "kl" at 0 and 1 (the penalties are new there), "beta" otherwise."""
    kw = dict(l1_w=pen[0], l1_h=pen[1], l2_w=pen[2], l2_h=pen[3])
    if beta == 0:
        return na.Engine(m, n, r, "mu", dtype=dtype, divergence="is", **kw)
    if beta == 1:
        return na.Engine(m, n, r, "mu", dtype=dtype, divergence="kl", dense_compute=True, **kw)
    return na.Engine(m, n, r, "mu", dtype=dtype, divergence="beta", beta=beta, **kw)


def run_engine(eng, W0, H0, iters, constant_w=False, first=1):
    if W0 is not None:
        eng.set_factors(W0, H0)
    eng.iterate(iters, first_iteration=first, error_every=0, last_iteration=first + iters - 1, constant_w=constant_w)
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
    return gen.run(V.astype(np.float64), W0.astype(np.float64), H0.astype(np.float64), iters, beta, eps_of(dtype), **kw)


def csr_of(V):
    m = V.shape[0]
    rows, cols = np.nonzero(V)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    ptr = np.zeros(m + 1, np.int32); np.add.at(ptr, rows + 1, 1); ptr = np.cumsum(ptr).astype(np.int32)
    return V[rows, cols], ptr, cols.astype(np.int32)


@pytest.fixture(scope="module")
def ctx():
    assert na.initialize() in (na.ResultType.Success, na.ResultType.ErrorAlreadyInitialized)
    na.set_verbosity(na.Verbosity.Nothing)
    yield
    na.finalize()


# 1. parity with the restatement: every padded rank, ragged shapes, padding exactly zero
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("beta,r", [(b, r) for b in (-1.0, 0.5, 1.5, 3.0) for r in (8, 65, 129)] + [(0.5, 256)])
def test_parity_with_restatement(beta, r, dtype):
    m, n, iters = 131 + r % 7, 97 + r % 5, 20
    V, W0, H0 = problem(m, n, r, dtype, seed=r + 20 + int(10 * beta))
    eng = engine(m, n, r, dtype, beta)
    g = eng.geometry()
    rp = g["padded_rank"]
    assert rp == (64 if r <= 64 else 128 if r <= 128 else 256)
    assert g["product_kernel"] == 6 and g["resident_images"] == 2 and g["kl_blocks_w"] == 0 and g["kl_blocks_h"] == 0 and g["exchange_count"] == 0
    assert g["slabs_h"] >= 1 and g["slabs_w"] >= 1
    eng.upload(V)
    got = run_engine(eng, W0, H0, iters)
    check(got, reference(V, W0, H0, iters, beta, dtype), dtype, f"beta {beta} r {r}")
    Hp = eng.debug_read(1, rp * g["padded_n"]).reshape(g["padded_n"], rp)
    Wp = eng.debug_read(0, rp * g["padded_m"]).reshape(g["padded_m"], rp)
    assert np.all(np.isfinite(Hp)) and np.all(np.isfinite(Wp))
    assert np.all(Hp[:, r:] == 0) and np.all(Hp[n:] == 0) and np.all(Wp[:, r:] == 0) and np.all(Wp[m:] == 0)
    assert np.all(Hp[:n, :r] >= 0) and np.all(Wp[:m, :r] >= 0)
    eng.close()


# 2. the penalties: no normalisation; changed between iterations
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("beta", [0, 1, 0.5])
def test_penalties(beta, dtype):
    m, n, r, iters = 137, 101, 9, 20
    V, W0, H0 = problem(m, n, r, dtype, seed=200 + int(10 * beta))
    eng = engine(m, n, r, dtype, beta, PEN)
    eng.upload(V)
    got = run_engine(eng, W0, H0, iters)
    want = reference(V, W0, H0, iters, beta, dtype, pen=PEN)
    check(got, want, dtype, f"penalised beta {beta}")
    plain = reference(V, W0, H0, iters, beta, dtype)
    assert rel(got[1], plain[1]) > 1e-3      # (the penalties do something)
    # penalised, then unpenalised (normalisation included), on the same engine
    first = run_engine(eng, W0, H0, 10)
    eng.set_penalties(0.0, 0.0, 0.0, 0.0)
    second = run_engine(eng, None, None, 10, first=11)
    w1 = reference(V, W0, H0, 10, beta, dtype, pen=PEN)
    check(first, w1, dtype, f"penalised beta {beta}, 10 iterations")
    check(second, reference(V, w1[0], w1[1], 10, beta, dtype), dtype, f"then unpenalised beta {beta}")
    # ... and back, through the setter alone
    eng.set_penalties(*PEN)
    check(run_engine(eng, W0, H0, iters), want, dtype, f"penalised again beta {beta}")
    with pytest.raises(na.EngineError) as e:
        eng.set_penalties(-1.0, 0.0, 0.0, 0.0)
    assert e.value.status == 1
    eng.close()


# 3. V with zeros: allowed for beta > 0 (dense, or sparse input densified), refused for beta <= 0
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["dense", "csr"])
@pytest.mark.parametrize("beta", [0.5, 1.5])
def test_zeros_in_v(beta, form, dtype):
    m, n, r, iters = 140, 120, 9, 20
    V, W0, H0 = problem(m, n, r, dtype, seed=31, zeros=0.4)
    eng = engine(m, n, r, dtype, beta)
    if form == "dense":
        eng.upload(V)
    else:
        eng.upload_sparse(1, *csr_of(V), 0)
    got = run_engine(eng, W0, H0, iters)
    check(got, reference(V, W0, H0, iters, beta, dtype), dtype, f"beta {beta} with zeros ({form})")
    eng.close()


def test_zeros_are_refused_below_beta_zero():
    m, n, r = 140, 120, 9
    V, W0, H0 = problem(m, n, r, np.float32, seed=31, zeros=0.4)
    eng = engine(m, n, r, np.float32, -1.0)
    with pytest.raises(na.EngineError) as e:
        eng.upload(V)
    assert e.value.status == 1 and "finite and > 0" in str(e.value)
    with pytest.raises(na.EngineError) as e:
        eng.upload_sparse(1, *csr_of(V), 0)
    assert e.value.status == 1 and "sparse input is refused" in str(e.value)
    with pytest.raises(na.EngineError):
        eng.iterate(1)
    eng.upload(F(V + np.float32(0.25)))      # (a valid V afterwards is taken)
    eng.set_factors(W0, H0)
    eng.iterate(2, first_iteration=1, error_every=0, last_iteration=2)
    assert np.isfinite(eng.divergence_value) and eng.divergence_value > 0
    eng.close()


# 4. one beta means one iteration however it is selected
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_routing_of_beta_0_and_1(beta, dtype):
    m, n, r, iters = 150, 110, 70, 12
    V, W0, H0 = problem(m, n, r, dtype, seed=41)
    outs = []
    for kw in (dict(divergence="beta", beta=beta), dict(divergence="is") if beta == 0 else dict(divergence="kl", dense_compute=True)):
        eng = na.Engine(m, n, r, "mu", dtype=dtype, **kw)
        eng.upload(V)
        outs.append(run_engine(eng, W0, H0, iters))
        eng.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert outs[0][2:] == outs[1][2:]


# 5. a repeated run is bit-identical (several reduction slabs in the W step)
@pytest.mark.parametrize("dtype", DTYPES)
def test_reproducibility(dtype):
    m, n, r, iters = 70, 3000, 8, 10
    V, W0, H0 = problem(m, n, r, dtype, seed=51)
    outs = []
    for _ in range(2):
        eng = engine(m, n, r, dtype, 0.5, PEN)
        assert eng.geometry()["slabs_w"] > 1
        eng.upload(V)
        outs.append(run_engine(eng, W0, H0, iters))
        eng.close()
    check(outs[0], reference(V, W0, H0, iters, 0.5, dtype, pen=PEN), dtype, "slabs, penalised beta 0.5")
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert outs[0][2:] == outs[1][2:]


# 6. constant W: the H step alone, W untouched, the error from the terms-only form of the W-side launch
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("r", [16, 200])
def test_constant_w(r, dtype):
    m, n, iters = 140, 100, 10
    V, W0, H0 = problem(m, n, r, dtype, seed=61 + r)
    eng = engine(m, n, r, dtype, 0.5)
    eng.upload(V)
    got = run_engine(eng, W0, H0, iters, constant_w=True)
    assert np.array_equal(got[0], W0)
    check(got, reference(V, W0, H0, iters, 0.5, dtype, const_w=True), dtype, f"constant W beta 0.5 r {r}")
    assert got[2] > 0 and got[4] > 0
    eng.close()


# 7. the kernel entry: every new instantiation (padded rank x precision x form) once per slab count, against the restatement's half-step; two update workgroups
#    (out_pad = 256), two reduction tiles in fp32 at RP <= 128 and four at RP = 256 (red_pad = 256), ragged valid sizes, r = RP - 3
def half_step_case(RP, dtype, beta, seed):
    out_valid, out_pad, red_valid, red_pad, r = 200, 256, 190, 256, RP - 3
    rng = np.random.default_rng(seed)
    A = np.zeros((out_pad, RP), dtype); A[:out_valid, :r] = 1.0 - rng.random((out_valid, r))
    B = np.zeros((red_pad, RP), dtype); B[:red_valid, :r] = 1.0 - rng.random((red_valid, r))
    X = np.zeros((out_pad, red_pad), dtype); X[:out_valid, :red_valid] = gen.planted(out_valid, red_valid, seed=72).astype(dtype)
    return A, B, X, r, out_valid, red_valid


def check_half_step(res, A, B, X, r, out_valid, red_valid, beta, form, l1, l2, dtype):
    eps = eps_of(dtype)
    tol = 1e-5 if dtype == np.float32 else 1e-12
    A64, B64, X64 = A.astype(np.float64)[:out_valid, :r], B.astype(np.float64)[:red_valid, :r], X.astype(np.float64)[:out_valid, :red_valid]
    got = res["A"]
    if form == 2:
        assert np.array_equal(got, A)
    else:
        want = gen.half_step(X64, A64, B64, beta, eps, float(dtype(l1)), float(dtype(l2)))
        figure = rel(got[:out_valid, :r], want)
        print(f"half-step beta {beta} form {form} penalties ({l1}, {l2}) {np.dtype(dtype).name} RP {A.shape[1]} slabs {res['slabs']}: panel {figure:.2e}")
        assert figure < tol, figure
        assert np.all(got[out_valid:] == 0) and np.all(got[:, r:] == 0)
        assert res["sumsq_part"].shape == (2, A.shape[1])
        g64 = got.astype(np.float64)
        for part, rows in ((0, slice(0, 128)), (1, slice(128, 256))):
            assert np.allclose(res["sumsq_part"][part], (g64[rows] ** 2).sum(axis=0), rtol=10 * tol, atol=0)
            assert np.allclose(res["sum_part"][part], g64[rows].sum(axis=0), rtol=10 * tol, atol=0)
    if form == 0:
        assert res["t_frob"] is None
    else:
        tf, td = gen.terms(X64, A64, B64, beta, eps)
        print(f"    terms: frobenius {np.max(np.abs(res['t_frob'][:out_valid] / tf - 1)):.2e} divergence {np.max(np.abs(res['t_div'][:out_valid] / td - 1)):.2e}")
        assert np.allclose(res["t_frob"][:out_valid], tf, rtol=10 * tol) and np.allclose(res["t_div"][:out_valid], td, rtol=10 * tol)
        assert np.all(res["t_frob"][out_valid:] == 0) and np.all(res["t_div"][out_valid:] == 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("RP", [64, 128, 256])
@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("force_slabs", [1, 2])
def test_half_step_kernel(force_slabs, form, RP, dtype):
    beta = 0.5
    A, B, X, r, out_valid, red_valid = half_step_case(RP, dtype, beta, seed=71 + RP)
    for l1, l2 in ((0.0, 0.0), (0.05, 0.01)):
        res = na.op_beta_half_step_general(A, B, X, r, out_valid, red_valid, beta, form, l1=l1, l2=l2, force_slabs=force_slabs)
        assert res["slabs"] == force_slabs
        check_half_step(res, A, B, X, r, out_valid, red_valid, beta, form, l1, l2, dtype)
    with pytest.raises(na.EngineError):
        na.op_beta_half_step_general(A, B, X, r, out_valid, red_valid, float("nan"), form)
    with pytest.raises(na.EngineError):
        na.op_beta_half_step_general(A, B, X, r, out_valid, red_valid, beta, form, l1=-1.0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_half_step_kernel_penalised_at_beta_0_and_1(beta, dtype):
    RP = 64
    A, B, X, r, out_valid, red_valid = half_step_case(RP, dtype, beta, seed=75)
    dsum = B.astype(np.float64).sum(axis=0).astype(dtype)
    res = na.op_beta_half_step_general(A, B, X, r, out_valid, red_valid, beta, 1, l1=0.05, l2=0.01, dsum=dsum, force_slabs=2)
    check_half_step(res, A, B, X, r, out_valid, red_valid, beta, 1, 0.05, 0.01, dtype)
    # without penalties the general entry is the existing one, bit for bit
    a = na.op_beta_half_step_general(A, B, X, r, out_valid, red_valid, beta, 1, dsum=dsum, force_slabs=2)
    b = na.op_beta_half_step(A, B, X, r, out_valid, red_valid, int(beta), 1, dsum=dsum, force_slabs=2)
    assert np.array_equal(a["A"], b["A"]) and np.array_equal(a["t_div"], b["t_div"]) and np.array_equal(a["sum_part"], b["sum_part"])
    assert not np.array_equal(a["A"], res["A"])


# 8. nmfgpu::compute with Parameter "divergence" = 3 and "beta", with and without the penalties; the penalties on "divergence" = 2
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("penalised", [False, True])
def test_compute(ctx, dtype, penalised):
    m, n, r, iters = 160, 120, 7, 20
    V, W0, H0 = problem(m, n, r, dtype, seed=81)
    params = {"divergence": 3, "beta": 0.5}
    pen = gen.NO_PENALTIES
    if penalised:
        pen = PEN
        params.update({"l1W": PEN[0], "l1H": PEN[1], "l2W": PEN[2], "l2H": PEN[3]})
    W, H = W0.copy(order="F"), H0.copy(order="F")
    s = na.Summary()
    assert na.compute(V, W, H, iterations=iters, parameters=params, summary=s) == na.ResultType.Success
    want = reference(V, W0, H0, iters, 0.5, dtype, pen=pen)
    assert s.record_count() == 1
    rec = s.record(0)
    ftol, etol = TOL[dtype]
    print(f"compute beta 0.5 penalised {penalised} {np.dtype(dtype).name}: W {rel(W, want[0]):.2e} H {rel(H, want[1]):.2e} frobenius {abs(rec.frobenius / want[2] - 1):.2e} "
          f"rmsd {abs(rec.rmsd / want[3] - 1):.2e}")
    assert rel(W, want[0]) < ftol and rel(H, want[1]) < ftol
    assert rec.frobenius == pytest.approx(want[2], rel=etol) and rec.rmsd == pytest.approx(want[3], rel=etol) and rec.numIterations == iters
    s.destroy()


def test_compute_from_a_random_start_and_penalised_itakura_saito(ctx):
    m, n, r = 160, 120, 7
    V, W0, H0 = problem(m, n, r, np.float32, seed=81)
    errors = []
    for iters in (5, 40):
        W, H = W0.copy(order="F"), H0.copy(order="F")
        s = na.Summary()
        assert na.compute(V, W, H, iterations=iters, init=na.NmfInitializationMethod.AllRandomValues, seed=5, parameters={"divergence": 3, "beta": 1.5},
                          summary=s) == na.ResultType.Success
        assert not np.array_equal(W, W0) and np.all(np.isfinite(W)) and np.all(np.isfinite(H))
        errors.append(s.record(0).frobenius)
        s.destroy()
    assert np.all(np.isfinite(errors)) and 0 < errors[1] < errors[0]
    outs = []
    for params in ({"divergence": 2}, {"divergence": 2, "l1H": 0.05}):
        W, H = W0.copy(order="F"), H0.copy(order="F")
        assert na.compute(V, W, H, iterations=10, parameters=params) == na.ResultType.Success
        outs.append((W, H))
    want = reference(V, W0, H0, 10, 0, np.float32, pen=(0.0, 0.05, 0.0, 0.0))
    assert rel(outs[1][0], want[0]) < 2e-4 and rel(outs[1][1], want[1]) < 2e-4
    assert rel(outs[1][1], outs[0][1].astype(np.float64)) > 1e-3
