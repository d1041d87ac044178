"""Weighted dense beta-divergence NMF on the GPU (docs/DIVERGENCE.md, "Weighted update"): the weighted kernel entry at every instantiation, weights of 1 against
the unweighted kernel and engine bit for bit, the rule that a zero weight hides the value, the engine against the numpy restatement
(tests/weighted_reference.py) at beta = -1 ... 3, penalties, constant W, reproducibility, a second upload, and the refusals.

Tolerances are those of tests/test_gpu_beta_general.py, whose arithmetic this is plus one multiply per entry: the kernel entry 1e-5 (fp32) and 1e-12 (fp64) on
the panel, ten times that on the sums and the per-row terms; the engine (TOL) 2e-4 on the factors and 1e-5 on the errors in fp32, 1e-9 in fp64."""
import numpy as np
import pytest

import nmfgpu_amd as na
from tests import weighted_reference as wref
from tests.test_gpu_beta_general import PEN, TOL, eps_of, half_step_case, rel

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
ZERO_ROW, ZERO_COL = 5, 9      # the row and the column of V without a single observed entry


def F(a):
    return np.asfortranarray(a)


# ---- the kernel entry ------------------------------------------------------------------------------------------------------------------------------

ZERO_OUT, ZERO_RED = 7, 11      # the output row and the reduction row whose weights are all 0


def weighted_case(RP, dtype, seed):
    """half_step_case of tests/test_gpu_beta_general.py (out 200 / 256, red 190 / 256, r = RP - 3) with weights uniform in (0, 2], 30 % zeros, one all-zero output
    row and one all-zero reduction row; X is NaN wherever the weight is 0, the padding included."""
    A, B, X, r, out_valid, red_valid = half_step_case(RP, dtype, 0.5, seed)
    Om = np.zeros_like(X)
    Om[:out_valid, :red_valid] = wref.weights(out_valid, red_valid, seed + 1, zero_row=ZERO_OUT, zero_col=ZERO_RED).astype(dtype)
    X = X.copy()
    X[Om == 0] = np.nan
    return A, B, X, Om, r, out_valid, red_valid


def worst(got, want):
    """max |got / want - 1| over want != 0; got must be exactly 0 where want is."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.all(got[want == 0] == 0)
    nz = want != 0
    return float(np.max(np.abs(got[nz] / want[nz] - 1))) if nz.any() else 0.0


def check_weighted_half_step(res, A, B, X, Om, r, out_valid, red_valid, beta, form, l1, l2, dtype):
    eps = eps_of(dtype)
    tol = 1e-5 if dtype == np.float32 else 1e-12
    A64, B64 = A.astype(np.float64)[:out_valid, :r], B.astype(np.float64)[:red_valid, :r]
    X64, O64 = X.astype(np.float64)[:out_valid, :red_valid], Om.astype(np.float64)[:out_valid, :red_valid]
    got = res["A"]
    assert np.all(np.isfinite(got))
    if form == 2:
        assert np.array_equal(got, A)
    else:
        want = wref.half_step(X64, O64, A64, B64, beta, eps, float(dtype(l1)), float(dtype(l2)))
        figure = rel(got[:out_valid, :r], want)
        print(f"weighted half-step beta {beta} form {form} penalties ({l1}, {l2}) {np.dtype(dtype).name} RP {A.shape[1]} slabs {res['slabs']}: panel {figure:.2e}")
        assert figure < tol, figure
        assert np.all(got[out_valid:] == 0) and np.all(got[:, r:] == 0)
        assert np.all(got[ZERO_OUT] == 0) and np.all(want[ZERO_OUT] == 0)
        assert res["sumsq_part"].shape == (2, A.shape[1])
        assert np.all(np.isfinite(res["sumsq_part"])) and np.all(np.isfinite(res["sum_part"]))
        g64 = got.astype(np.float64)
        for part, rows in ((0, slice(0, 128)), (1, slice(128, 256))):
            assert np.allclose(res["sumsq_part"][part], (g64[rows] ** 2).sum(axis=0), rtol=10 * tol, atol=0)
            assert np.allclose(res["sum_part"][part], g64[rows].sum(axis=0), rtol=10 * tol, atol=0)
    if form == 0:
        assert res["t_frob"] is None
    else:
        tf, td = wref.terms(X64, O64, A64, B64, beta, eps)
        assert np.all(np.isfinite(res["t_frob"])) and np.all(np.isfinite(res["t_div"]))
        print(f"    terms: frobenius {worst(res['t_frob'][:out_valid], tf):.2e} divergence {worst(res['t_div'][:out_valid], td):.2e}")
        assert np.allclose(res["t_frob"][:out_valid], tf, rtol=10 * tol, atol=0) and np.allclose(res["t_div"][:out_valid], td, rtol=10 * tol, atol=0)
        assert res["t_frob"][ZERO_OUT] == 0 and res["t_div"][ZERO_OUT] == 0
        assert np.all(res["t_frob"][out_valid:] == 0) and np.all(res["t_div"][out_valid:] == 0)


# 1. every new instantiation (padded rank x precision x form) once per slab count
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("RP", [64, 128, 256])
@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("force_slabs", [1, 2])
def test_weighted_half_step_kernel(force_slabs, form, RP, dtype):
    beta = 0.5
    A, B, X, Om, r, out_valid, red_valid = weighted_case(RP, dtype, seed=71 + RP)
    for l1, l2 in ((0.0, 0.0), (0.05, 0.01)):
        res = na.op_beta_half_step_weighted(A, B, X, Om, r, out_valid, red_valid, beta, form, l1=l1, l2=l2, force_slabs=force_slabs)
        assert res["slabs"] == force_slabs
        check_weighted_half_step(res, A, B, X, Om, r, out_valid, red_valid, beta, form, l1, l2, dtype)
    with pytest.raises(na.EngineError):
        na.op_beta_half_step_weighted(A, B, X, Om, r, out_valid, red_valid, float("nan"), form)
    with pytest.raises(na.EngineError):
        na.op_beta_half_step_weighted(A, B, X, Om, r, out_valid, red_valid, beta, form, l1=-1.0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("force_slabs", [1, 2])
@pytest.mark.parametrize("beta", [0.0, 1.0, 2.0])
def test_weighted_half_step_kernel_other_betas(beta, force_slabs, dtype):
    RP, form = 64, 1
    A, B, X, Om, r, out_valid, red_valid = weighted_case(RP, dtype, seed=75)
    res = na.op_beta_half_step_weighted(A, B, X, Om, r, out_valid, red_valid, beta, form, force_slabs=force_slabs)
    assert res["slabs"] == force_slabs
    check_weighted_half_step(res, A, B, X, Om, r, out_valid, red_valid, beta, form, 0.0, 0.0, dtype)


# 2. weights of 1 are the unweighted kernel: bit for bit where the arithmetic is the same (a product with 1.0 is exact, the summation order is the same); at
#    beta = 1 within the tolerance of 1, because the denominator comes from the matrix pipe instead of dsum
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("RP", [64, 128])
@pytest.mark.parametrize("force_slabs", [1, 2])
@pytest.mark.parametrize("beta", [0.5, 0.0, 1.0])
def test_weights_of_one_are_the_unweighted_kernel(beta, force_slabs, RP, dtype):
    A, B, X, r, out_valid, red_valid = half_step_case(RP, dtype, beta, seed=71 + RP)
    Om = np.zeros_like(X)
    Om[:out_valid, :red_valid] = 1
    dsum = B.astype(np.float64).sum(axis=0).astype(dtype)
    tol = 1e-5 if dtype == np.float32 else 1e-12
    for form in (0, 1, 2):
        a = na.op_beta_half_step_weighted(A, B, X, Om, r, out_valid, red_valid, beta, form, force_slabs=force_slabs)
        b = na.op_beta_half_step_general(A, B, X, r, out_valid, red_valid, beta, form, dsum=dsum, force_slabs=force_slabs)
        assert a["slabs"] == b["slabs"] == force_slabs
        if form != 0:
            assert np.array_equal(a["t_frob"], b["t_frob"]) and np.array_equal(a["t_div"], b["t_div"])      # (the terms do not involve the denominator)
        if beta != 1:
            assert np.array_equal(a["A"], b["A"])
            assert np.array_equal(a["sumsq_part"], b["sumsq_part"]) and np.array_equal(a["sum_part"], b["sum_part"])
        else:
            figure = rel(a["A"], b["A"].astype(np.float64))
            print(f"beta 1, weights of 1 against the unweighted kernel, {np.dtype(dtype).name} RP {RP} form {form}: {figure:.2e}")
            assert figure < tol
            assert np.allclose(a["sumsq_part"], b["sumsq_part"], rtol=10 * tol, atol=0) and np.allclose(a["sum_part"], b["sum_part"], rtol=10 * tol, atol=0)


# 3. a zero weight hides the value
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("beta", [0.5, 0.0, 1.0])
def test_a_zero_weight_hides_the_value(beta, form, dtype):
    RP = 64
    A, B, X, Om, r, out_valid, red_valid = weighted_case(RP, dtype, seed=77)
    hidden = np.array([np.nan, np.inf, -5.0, 1e30], dtype)
    Xa, Xb = X.copy(), X.copy()
    where = np.argwhere(Om == 0)
    Xa[Om == 0] = hidden[np.arange(len(where)) % 4]
    Xb[Om == 0] = 0
    a = na.op_beta_half_step_weighted(A, B, Xa, Om, r, out_valid, red_valid, beta, form, l1=0.05, l2=0.01, force_slabs=2)
    b = na.op_beta_half_step_weighted(A, B, Xb, Om, r, out_valid, red_valid, beta, form, l1=0.05, l2=0.01, force_slabs=2)
    for key in ("A", "sumsq_part", "sum_part") + (("t_frob", "t_div") if form else ()):
        assert np.all(np.isfinite(a[key])), key
        assert np.array_equal(a[key], b[key]), key


# ---- the engine ------------------------------------------------------------------------------------------------------------------------------------

def problem(m, n, r, dtype, seed, zeros=0.3):
    """V (NaN wherever its weight is 0), the weights (30 % zeros, an all-zero row and an all-zero column) and a start."""
    Om = wref.weights(m, n, seed + 2, zero_row=ZERO_ROW, zero_col=ZERO_COL, zeros=zeros, dtype=dtype)
    V = F(wref.planted(m, n, seed=seed).astype(dtype))
    V[Om == 0] = np.nan
    W0, H0 = wref.start(m, n, r, seed + 1, dtype)
    return V, Om, W0, H0


def engine(m, n, r, dtype, beta, pen=wref.NO_PENALTIES, weighted=True):
    kw = dict(l1_w=pen[0], l1_h=pen[1], l2_w=pen[2], l2_h=pen[3], weighted=weighted)
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


def reference(V, Om, W0, H0, iters, beta, dtype, **kw):
    return wref.run(V.astype(np.float64), Om.astype(np.float64), W0.astype(np.float64), H0.astype(np.float64), iters, beta, eps_of(dtype), **kw)


def check(got, want, dtype, what=""):
    ftol, etol = TOL[dtype]
    figures = (rel(got[0], want[0]), rel(got[1], want[1]), abs(got[2] / want[2] - 1), abs(got[3] / want[3] - 1), abs(got[4] / want[4] - 1))
    print(f"weighted {what} {np.dtype(dtype).name}: W {figures[0]:.2e} H {figures[1]:.2e} frobenius {figures[2]:.2e} rmsd {figures[3]:.2e} divergence {figures[4]:.2e}")
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1])) and np.all(np.isfinite(got[2:]))
    assert figures[0] < ftol and figures[1] < ftol, figures
    assert figures[2] < etol and figures[3] < etol and figures[4] < etol, figures


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


# 4. parity with the restatement: every beta, every padded rank, ragged shapes, exact zeros where nothing is observed and in the padding
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("beta,r", [(b, r) for b in (-1.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0) for r in (8, 65, 129)] + [(0.5, 256)])
def test_parity_with_restatement(beta, r, dtype):
    m, n, iters = 131 + r % 7, 97 + r % 5, 20
    V, Om, W0, H0 = problem(m, n, r, dtype, seed=r + 20 + int(10 * beta))
    eng = engine(m, n, r, dtype, beta)
    g = eng.geometry()
    rp = g["padded_rank"]
    assert rp == (64 if r <= 64 else 128 if r <= 128 else 256)
    assert g["product_kernel"] == 6 and g["resident_images"] == 4 and g["exchange_count"] == 0
    eng.upload(V, weights=Om)
    got = run_engine(eng, W0, H0, iters)
    want = reference(V, Om, W0, H0, iters, beta, dtype)
    check(got, want, dtype, f"beta {beta} r {r}")
    assert want[3] == pytest.approx(want[2] / np.sqrt(Om.astype(np.float64).sum()), rel=1e-14)      # (rmsd over the sum of the weights)
    Hp = eng.debug_read(1, rp * g["padded_n"]).reshape(g["padded_n"], rp)
    Wp = eng.debug_read(0, rp * g["padded_m"]).reshape(g["padded_m"], rp)
    assert np.all(np.isfinite(Hp)) and np.all(np.isfinite(Wp))
    assert np.all(Hp[:, r:] == 0) and np.all(Hp[n:] == 0) and np.all(Wp[:, r:] == 0) and np.all(Wp[m:] == 0)
    assert np.all(Hp[:n, :r] >= 0) and np.all(Wp[:m, :r] >= 0)
    assert np.all(Wp[ZERO_ROW] == 0) and np.all(Hp[ZERO_COL] == 0)
    eng.close()


# 5. the penalties: no normalisation; changed between iterations
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("beta", [0, 1, 0.5])
def test_penalties(beta, dtype):
    m, n, r, iters = 137, 101, 9, 20
    V, Om, W0, H0 = problem(m, n, r, dtype, seed=200 + int(10 * beta))
    eng = engine(m, n, r, dtype, beta, PEN)
    eng.upload(V, weights=Om)
    got = run_engine(eng, W0, H0, iters)
    want = reference(V, Om, W0, H0, iters, beta, dtype, pen=PEN)
    check(got, want, dtype, f"penalised beta {beta}")
    plain = reference(V, Om, W0, H0, iters, beta, dtype)
    assert rel(got[1], plain[1]) > 1e-3      # (the penalties do something)
    first = run_engine(eng, W0, H0, 10)
    eng.set_penalties(0.0, 0.0, 0.0, 0.0)
    second = run_engine(eng, None, None, 10, first=11)
    w1 = reference(V, Om, W0, H0, 10, beta, dtype, pen=PEN)
    check(first, w1, dtype, f"penalised beta {beta}, 10 iterations")
    check(second, reference(V, Om, w1[0], w1[1], 10, beta, dtype), dtype, f"then unpenalised beta {beta}")
    eng.set_penalties(*PEN)
    check(run_engine(eng, W0, H0, iters), want, dtype, f"penalised again beta {beta}")
    eng.close()


# 6. constant W: the H step alone, W untouched, the errors from the terms-only form
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("r", [16, 200])
def test_constant_w(r, dtype):
    m, n, iters = 140, 100, 10
    V, Om, W0, H0 = problem(m, n, r, dtype, seed=61 + r)
    eng = engine(m, n, r, dtype, 0.5)
    eng.upload(V, weights=Om)
    got = run_engine(eng, W0, H0, iters, constant_w=True)
    assert np.array_equal(got[0], W0)
    check(got, reference(V, Om, W0, H0, iters, 0.5, dtype, const_w=True), dtype, f"constant W beta 0.5 r {r}")
    assert got[2] > 0 and got[4] > 0
    eng.close()


# 7. a repeated run is bit-identical (several reduction slabs in the W step); a second upload replaces V and the weights
@pytest.mark.parametrize("dtype", DTYPES)
def test_reproducibility_and_second_upload(dtype):
    m, n, r, iters = 70, 3000, 8, 10
    V, Om, W0, H0 = problem(m, n, r, dtype, seed=51)
    Om2 = wref.weights(m, n, 99, zero_row=3, zero_col=4, zeros=0.5, dtype=dtype)
    V2 = F(wref.planted(m, n, seed=52).astype(dtype))
    V2[Om2 == 0] = np.inf
    outs = []
    for _ in range(2):
        eng = engine(m, n, r, dtype, 0.5, PEN)
        assert eng.geometry()["slabs_w"] > 1
        eng.upload(V, weights=Om)
        outs.append(run_engine(eng, W0, H0, iters))
        if len(outs) == 1:
            eng.close()
    check(outs[0], reference(V, Om, W0, H0, iters, 0.5, dtype, pen=PEN), dtype, "slabs, penalised beta 0.5")
    assert same(outs[0], outs[1])
    eng.upload(V2, weights=Om2)      # (the engine of the second run)
    again = run_engine(eng, W0, H0, iters)
    eng.close()
    fresh = engine(m, n, r, dtype, 0.5, PEN)
    fresh.upload(V2, weights=Om2)
    want = run_engine(fresh, W0, H0, iters)
    fresh.close()
    assert same(again, want) and not same(again, outs[0])


# 8. weights of 1 on the engine: the unweighted engine, bit for bit at beta != 1
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("beta", [0.0, 0.5, 1.0])
def test_weights_of_one_are_the_unweighted_engine(beta, dtype):
    m, n, r, iters = 150, 110, 70, 10
    V = F(wref.planted(m, n, seed=41).astype(dtype))
    W0, H0 = wref.start(m, n, r, 42, dtype)
    outs = []
    for weighted in (True, False):
        eng = engine(m, n, r, dtype, beta, weighted=weighted)
        if weighted:
            eng.upload(V, weights=F(np.ones((m, n), dtype)))
        else:
            eng.upload(V)
        outs.append(run_engine(eng, W0, H0, iters))
        eng.close()
    if beta != 1:
        assert same(outs[0], outs[1])
    else:
        check(outs[0], tuple(np.asarray(x, np.float64) if isinstance(x, np.ndarray) else x for x in outs[1]), dtype, "weights of 1 against the unweighted engine, beta 1")


# 9. refusals: status 1 and a reason
def refused(call, *words):
    with pytest.raises(na.EngineError) as e:
        call()
    text = str(e.value)
    assert e.value.status == 1, text
    assert "(" in text and len(text.split("(", 1)[1]) > 8, text      # (a reason came with it)
    for word in words:
        assert word in text, text


def test_refusals_at_creation():
    m, n, r = 60, 50, 4
    refused(lambda: na.Engine(m, n, r, "mu", divergence="frobenius", weighted=True), "weighted")
    refused(lambda: na.Engine(m, n, r, "mu", divergence="kl", weighted=True), "weighted")
    refused(lambda: na.Engine(m, n, r, "hals", weighted=True), "weighted")
    refused(lambda: na.Engine(m, n, r, "hals", divergence="is", weighted=True))
    refused(lambda: na.Engine(m, n, r, "mu", precision="bf16", weighted=True), "weighted")
    refused(lambda: na.Engine(m, n, r, "mu", divergence="is", precision="bf16", weighted=True), "bf16")


@pytest.mark.parametrize("dtype", DTYPES)
def test_refusals_at_upload(dtype):
    m, n, r = 60, 50, 4
    V, Om, W0, H0 = problem(m, n, r, dtype, seed=91)
    Vc = F(np.where(Om > 0, V, dtype(1)))
    eng = engine(m, n, r, dtype, 0.0)
    refused(lambda: eng.upload(Vc), "weights")
    rows, cols = np.nonzero(Vc)
    refused(lambda: eng.upload_sparse(3, Vc[rows, cols], rows.astype(np.int32), cols.astype(np.int32), 0), "sparse")
    plain = engine(m, n, r, dtype, 0.0, weighted=False)
    refused(lambda: plain.upload(Vc, weights=Om), "weighted")
    plain.close()

    def with_weight(value, at=(1, 1)):
        O = Om.copy(order="F")
        O[at] = value
        return O

    refused(lambda: eng.upload(V, weights=with_weight(-0.5)), "weight")
    refused(lambda: eng.upload(V, weights=with_weight(np.nan)), "weight")
    refused(lambda: eng.upload(V, weights=with_weight(np.inf)), "weight")
    refused(lambda: eng.upload(V, weights=F(np.zeros((m, n), dtype))), "weight")
    # v = 0 under a weight > 0 is refused at beta = 0, under a weight of 0 it is not looked at; NaN under a weight > 0 is refused at every beta
    at = tuple(np.argwhere(Om > 0)[3])
    hidden = tuple(np.argwhere(Om == 0)[3])
    Vz = V.copy(order="F"); Vz[at] = 0
    refused(lambda: eng.upload(Vz, weights=Om), "> 0")
    Vn = V.copy(order="F"); Vn[at] = np.nan
    refused(lambda: eng.upload(Vn, weights=Om), "finite")
    with pytest.raises(na.EngineError):      # (an engine refused its upload does not iterate)
        eng.iterate(1)
    Vh = V.copy(order="F"); Vh[hidden] = 0
    eng.upload(Vh, weights=Om)
    got = run_engine(eng, W0, H0, 3)
    check(got, reference(V, Om, W0, H0, 3, 0.0, dtype), dtype, "after the refusals")
    pos = engine(m, n, r, dtype, 0.5)
    refused(lambda: pos.upload(Vn, weights=Om), "finite")
    pos.upload(Vz, weights=Om)      # (beta > 0 takes a zero)
    pos.close()
    eng.close()


def test_refusals_of_the_three_phase_and_sharded_calls():
    import torch
    m, n, r = 60, 50, 4
    V, Om, W0, H0 = problem(m, n, r, np.float32, seed=93)
    eng = engine(m, n, r, np.float32, 0.5)
    eng.upload(V, weights=Om)
    eng.set_factors(W0, H0)
    ex = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")
    for call in (lambda: eng.h_step(True), lambda: eng.w_products(ex.data_ptr()), lambda: eng.w_finish(ex.data_ptr(), True)):
        refused(call)
    group = na.LocalGroup(1)
    comm = na.LocalComm(group, 0)
    with pytest.raises(na.EngineError) as e:
        na.ShardedRun(eng, comm, m, n, na.SHARD_REPLICATED)
    assert e.value.status == 1
    comm.close()
    got = run_engine(eng, W0, H0, 3)      # (the engine itself is unharmed)
    check(got, reference(V, Om, W0, H0, 3, 0.5, np.float32), np.float32, "after the refused calls")
    eng.close()
