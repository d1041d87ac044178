"""The mixed-precision dense divergence update on the GPU (docs/DIVERGENCE.md, "Mixed precision"; kernels_beta_bf16.hip): the kernel entry on exact data (the
operand maps of both bf16 products), every instantiation against the exact and the bf16-emulating restatement (tests/beta_mixed_reference.py), the engine over
twenty iterations, the behaviour that carries over from the fp32 engine, refusals, geometry and nmfgpu::compute.

Tolerances (tests/beta_mixed_cases.py; tests/test_beta_mixed_cpu.py recomputes every figure on the CPU):
  exact data             4 fp32 ulp per element of the updated panel: every operand is a bf16 value and every sum an integer below 2^24, so only the update's
                         own division and product round.
  against the exact fp64 restatement, one half-step, componentwise: 1.05 gamma (2 |beta - 2| + 2 |beta - 1| + 4) 2^-9 + 1e-5 (0.8 - 1.2e-2 here; the
                         restatement itself is at most 1.2e-3 away).
  against the emulating restatement: 4 x its own two-run figure (fp32 against fp64 accumulation) -- one half-step 4 x 3.1e-6 on the panel by norm; twenty
                         iterations 4 x 8.2e-4 on the factors and 4 x 3.4e-5 on frobenius, rmsd and the divergence value; the divergence value against the EXACT
                         restatement 4 x 7.4e-5.  The per-row terms of one half-step: the standing fp32 figure 1e-4.
Observed on an MI355X (every test prints its figures: pytest -s): exact data at most 0.5 ulp at every padded rank and slab count; one half-step against the
emulating restatement by norm at most 4.8e-6, against the exact update componentwise at most 1.15e-3, per-row terms 2.0e-7 (Frobenius) and 5.8e-7 (divergence);
twenty iterations, factors at most 7.4e-4, errors and divergence value 2.9e-5, divergence value against the exact restatement 6.1e-5."""
import ctypes as C

import numpy as np
import pytest

import nmfgpu_amd as na
from nmfgpu_amd import engine as engine_module
from tests import beta_general_reference as gen
from tests import beta_mixed_cases as cases
from tests import beta_mixed_reference as mix

pytestmark = pytest.mark.gpu

PEN = (0.05, 0.05, 0.01, 0.01)      # (l1W, l1H, l2W, l2H): tests/test_gpu_beta_general.py's
rel, EPS = cases.rel, cases.EPS32
TOL_PANEL = cases.MARGIN * cases.FIGURE_HALF_STEP_PANEL
TOL_FACTORS = cases.MARGIN * cases.FIGURE_ENGINE_FACTORS
TOL_ERRORS = cases.MARGIN * cases.FIGURE_ENGINE_ERRORS
TOL_DIVERGENCE_VS_EXACT = cases.MARGIN * cases.FIGURE_ENGINE_DIVERGENCE_VS_EXACT


def engine(m, n, r, beta, pen=gen.NO_PENALTIES, route="own", **kw):
    """route "own": "is" / dense "kl" at beta 0 / 1; "beta": divergence="beta" at every beta."""
    kw = dict(dtype=np.float32, mixed_precision=True, l1_w=pen[0], l1_h=pen[1], l2_w=pen[2], l2_h=pen[3], **kw)
    if route == "own" and beta == 0:
        return na.Engine(m, n, r, "mu", divergence="is", **kw)
    if route == "own" and beta == 1:
        return na.Engine(m, n, r, "mu", divergence="kl", dense_compute=True, **kw)
    return na.Engine(m, n, r, "mu", divergence="beta", beta=beta, **kw)


def run_engine(eng, W0, H0, iters, constant_w=False):
    eng.set_factors(W0, H0)
    eng.iterate(iters, first_iteration=1, error_every=0, last_iteration=iters, constant_w=constant_w)
    W, H = eng.get_factors()
    return W, H, eng.frobenius, eng.rmsd, eng.divergence_value


def check(got, want, what):
    figures = (rel(got[0], want[0]), rel(got[1], want[1]), abs(got[2] / want[2] - 1), abs(got[3] / want[3] - 1), abs(got[4] / want[4] - 1))
    print(f"{what}: W {figures[0]:.2e} H {figures[1]:.2e} frobenius {figures[2]:.2e} rmsd {figures[3]:.2e} divergence {figures[4]:.2e}")
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1]))
    assert figures[0] < TOL_FACTORS and figures[1] < TOL_FACTORS, figures
    assert max(figures[2:]) < TOL_ERRORS, figures


def emulated(V, W0, H0, iters, beta, **kw):
    return mix.run(V.astype(np.float64), W0.astype(np.float64), H0.astype(np.float64), iters, beta, EPS, **kw)


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def check_sums(res, RP):
    g64 = res["A"].astype(np.float64)
    assert res["sumsq_part"].shape == (2, RP)
    for part, rows in ((0, slice(0, 128)), (1, slice(128, 256))):
        assert np.allclose(res["sumsq_part"][part], (g64[rows] ** 2).sum(axis=0), rtol=1e-4, atol=0)
        assert np.allclose(res["sum_part"][part], g64[rows].sum(axis=0), rtol=1e-4, atol=0)


# 1. the kernel entry on exact data: a wrong k permutation or operand map of either product changes integers
@pytest.mark.parametrize("RP", cases.RPS)
@pytest.mark.parametrize("force_slabs", [1, 2])
def test_half_step_exact_data(force_slabs, RP):
    A, B, X, r, out_valid, red_valid = case = cases.exact_case(RP, 500 + RP)
    res = na.op_beta_half_step_mixed(A, B, X, r, out_valid, red_valid, 2.0, 0, force_slabs=force_slabs)
    assert res["slabs"] == force_slabs
    A64, B64, X64 = cases.valid(*case, np.float64)
    want = mix.half_step(X64, A64, B64, 2.0, EPS)
    got = res["A"]
    ulps = np.abs(got[:out_valid, :r].astype(np.float64) - want) / np.spacing(np.maximum(want, np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)
    print(f"exact data RP {RP} slabs {force_slabs}: at most {ulps.max():.2f} ulp, {int((want > 0).sum())} non-zero entries")
    assert (want > 0).sum() > 1000
    assert ulps.max() <= 4, ulps.max()
    assert np.all(got[out_valid:] == 0) and np.all(got[:, r:] == 0)
    check_sums(res, RP)


# 2. the kernel entry at every instantiation: padded rank x beta x form, once per slab count, without and with penalties
@pytest.mark.parametrize("RP", cases.RPS)
@pytest.mark.parametrize("beta", cases.HALF_STEP_BETAS)
@pytest.mark.parametrize("form", [0, 1, 2])
@pytest.mark.parametrize("force_slabs", [1, 2])
def test_half_step_kernel(force_slabs, form, beta, RP):
    A, B, X, r, out_valid, red_valid = case = cases.half_step_case(RP, 71 + RP)
    A64, B64, X64 = cases.valid(*case, np.float64)
    dsum = B.astype(np.float64).sum(axis=0).astype(np.float32) if beta == 1 else None
    d64 = None if dsum is None else dsum.astype(np.float64)[:r]
    for l1, l2 in cases.HALF_STEP_PENALTIES:
        res = na.op_beta_half_step_mixed(A, B, X, r, out_valid, red_valid, beta, form, l1=l1, l2=l2, dsum=dsum, force_slabs=force_slabs)
        assert res["slabs"] == force_slabs
        got = res["A"]
        if form == 2:
            assert np.array_equal(got, A)
        else:
            p1, p2 = float(np.float32(l1)), float(np.float32(l2))
            exact = gen.half_step(X64, A64, B64, beta, EPS, p1, p2, dsum=d64)
            emul = mix.half_step(X64, A64, B64, beta, EPS, p1, p2, dsum=d64)
            worst = float(np.max(np.abs(got[:out_valid, :r] / exact - 1)))
            by_norm = rel(got[:out_valid, :r], emul)
            print(f"half-step beta {beta} form {form} penalties ({l1}, {l2}) RP {RP} slabs {force_slabs}: against the exact update componentwise {worst:.2e} "
                  f"(bound {cases.derived_bound(beta):.2e}), against the emulating restatement by norm {by_norm:.2e} (tolerance {TOL_PANEL:.2e})")
            assert worst < cases.derived_bound(beta), worst
            assert by_norm < TOL_PANEL, by_norm
            assert np.all(got[out_valid:] == 0) and np.all(got[:, r:] == 0)
            check_sums(res, RP)
        if form == 0:
            assert res["t_frob"] is None
        else:
            tf, td = mix.terms(X64, A64, B64, beta, EPS)
            print(f"    terms: frobenius {np.max(np.abs(res['t_frob'][:out_valid] / tf - 1)):.2e} divergence {np.max(np.abs(res['t_div'][:out_valid] / td - 1)):.2e}")
            assert np.allclose(res["t_frob"][:out_valid], tf, rtol=cases.TOL_HALF_STEP_TERMS, atol=0)
            assert np.allclose(res["t_div"][:out_valid], td, rtol=cases.TOL_HALF_STEP_TERMS, atol=0)
            assert np.all(res["t_frob"][out_valid:] == 0) and np.all(res["t_div"][out_valid:] == 0)


# 3. the engine over twenty iterations, every padded rank; beta = 0 and 1 through both routes
@pytest.mark.parametrize("r", cases.ENGINE_RANKS)
@pytest.mark.parametrize("beta", cases.ENGINE_BETAS)
def test_engine_against_the_restatements(beta, r):
    m, n = cases.ENGINE_SHAPE
    V, W0, H0 = cases.engine_problem(r, beta)
    outs = []
    for route in (("own", "beta") if beta in (0.0, 1.0) else ("beta",)):
        eng = engine(m, n, r, beta, route=route)
        g = eng.geometry()
        rp = g["padded_rank"]
        assert rp == (64 if r <= 64 else 128 if r <= 128 else 256)
        assert g["product_kernel"] == 7 and g["resident_images"] == 2 and g["slabs_h"] >= 1 and g["slabs_w"] >= 1
        eng.upload(V)
        outs.append(run_engine(eng, W0, H0, cases.ENGINE_ITERS))
        Hp = eng.debug_read(1, rp * g["padded_n"]).reshape(g["padded_n"], rp)
        Wp = eng.debug_read(0, rp * g["padded_m"]).reshape(g["padded_m"], rp)
        assert np.all(Hp[:, r:] == 0) and np.all(Hp[n:] == 0) and np.all(Wp[:, r:] == 0) and np.all(Wp[m:] == 0)
        eng.close()
    if len(outs) == 2:
        assert same(outs[0], outs[1])
    check(outs[0], cases.emulated_run(r, beta, np.float64), f"mixed engine beta {beta} r {r}")
    exact = gen.run(V.astype(np.float64), W0.astype(np.float64), H0.astype(np.float64), cases.ENGINE_ITERS, beta, EPS)
    figure = abs(outs[0][4] / exact[4] - 1)
    print(f"    divergence value against the exact fp64 restatement: {figure:.2e} (tolerance {TOL_DIVERGENCE_VS_EXACT:.2e}); factors {rel(outs[0][0], exact[0]):.2e} {rel(outs[0][1], exact[1]):.2e}")
    assert figure < TOL_DIVERGENCE_VS_EXACT, figure


# 4. what carries over from the fp32 engine
def test_repeated_run_is_bit_identical():
    m, n, r, iters = 70, 3000, 8, 10
    V = np.asfortranarray(gen.planted(m, n, seed=51).astype(np.float32))
    W0, H0 = gen.start(m, n, r, 52, np.float32)
    outs = []
    for _ in range(2):
        eng = engine(m, n, r, 0.5, PEN)
        assert eng.geometry()["slabs_w"] > 1
        eng.upload(V)
        outs.append(run_engine(eng, W0, H0, iters))
        eng.close()
    assert same(outs[0], outs[1])
    check(outs[0], emulated(V, W0, H0, iters, 0.5, pen=PEN), "slabs, penalised beta 0.5")


@pytest.mark.parametrize("r", [16, 200])
def test_constant_w(r):
    m, n, iters = 140, 100, 10
    V = np.asfortranarray(gen.planted(m, n, seed=61 + r).astype(np.float32))
    W0, H0 = gen.start(m, n, r, 62 + r, np.float32)
    eng = engine(m, n, r, 0.5)
    eng.upload(V)
    got = run_engine(eng, W0, H0, iters, constant_w=True)
    assert np.array_equal(got[0], W0)
    check(got, emulated(V, W0, H0, iters, 0.5, const_w=True), f"constant W beta 0.5 r {r}")
    assert got[2] > 0 and got[4] > 0
    eng.close()


@pytest.mark.parametrize("beta", [0.0, 1.0, 0.5])
def test_a_penalised_run_is_not_normalised(beta):
    m, n, r, iters = 137, 101, 9, 20
    V = np.asfortranarray(gen.planted(m, n, seed=200 + int(10 * beta)).astype(np.float32))
    W0, H0 = gen.start(m, n, r, 201 + int(10 * beta), np.float32)
    eng = engine(m, n, r, beta, PEN)
    eng.upload(V)
    got = run_engine(eng, W0, H0, iters)
    check(got, emulated(V, W0, H0, iters, beta, pen=PEN), f"penalised beta {beta}")
    assert np.max(np.abs(np.linalg.norm(got[0].astype(np.float64), axis=0) - 1)) > 1e-2
    eng.close()


def csr_of(V):
    m = V.shape[0]
    rows, cols = np.nonzero(V)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    ptr = np.zeros(m + 1, np.int32); np.add.at(ptr, rows + 1, 1); ptr = np.cumsum(ptr).astype(np.int32)
    return V[rows, cols], ptr, cols.astype(np.int32)


@pytest.mark.parametrize("beta", [1.0, 1.5])
def test_zeros_in_v_and_a_csr_upload(beta):
    m, n = cases.ENGINE_SHAPE
    r, iters = 9, cases.ENGINE_ITERS
    V, W0, H0 = cases.engine_problem(r, beta, zeros=0.3)
    assert 0.2 < np.mean(V == 0) < 0.4
    eng = engine(m, n, r, beta)
    eng.upload(V)
    dense = run_engine(eng, W0, H0, iters)
    check(dense, emulated(V, W0, H0, iters, beta), f"30 % zeros beta {beta}")
    eng.close()
    if beta == 1.0:
        eng = engine(m, n, r, beta)
        eng.upload_sparse(1, *csr_of(V), 0)
        assert same(run_engine(eng, W0, H0, iters), dense)
        eng.close()


def test_medium_case():
    m, n, r, iters, beta = 2100, 1300, 40, 5, 0.5      # several rounds of workgroups in both launches
    V = np.asfortranarray(gen.planted(m, n, seed=77).astype(np.float32))
    W0, H0 = gen.start(m, n, r, 78, np.float32)
    eng = engine(m, n, r, beta)
    eng.upload(V)
    got = run_engine(eng, W0, H0, iters)
    check(got, emulated(V, W0, H0, iters, beta), "2100 x 1300 r 40, 5 iterations, beta 0.5")
    eng.close()


# 5. refusals and geometry
def refused(call, *words):
    with pytest.raises(na.EngineError) as e:
        call()
    text = str(e.value)
    assert e.value.status == 1, text
    for word in words:
        assert word in text, text


def create_raw(params, size, m=60, n=50, r=4, elem_bytes=4):
    lib = engine_module.library()
    lib.nmfamd_engine_last_error.restype = C.c_char_p
    h = C.c_void_p()
    st = lib.nmfamd_engine_create_v2(m, n, r, engine_module.ALGORITHMS["mu"], C.byref(params), C.c_ulong(size), elem_bytes, C.c_void_p(0), 1, C.byref(h))
    return st, h, (lib.nmfamd_engine_last_error(None) or b"").decode()


def params_v5(divergence, beta, mixed):
    P = engine_module
    return P._ParamsV5(P._ParamsV4(P._ParamsV3(P._ParamsV2(P._Params(0, 0, 0, 0, 0, 0, divergence, 0, 0, 0), 0.0), beta), 0.0), mixed)


def test_refusals_at_creation():
    m, n, r = 60, 50, 4
    refused(lambda: na.Engine(m, n, r, "mu", dtype=np.float64, divergence="is", mixed_precision=True), "mixed precision", "single")
    refused(lambda: na.Engine(m, n, r, "mu", divergence="is", weighted=True, mixed_precision=True), "mixed precision", "weighted")
    refused(lambda: na.Engine(m, n, r, "hals", mixed_precision=True), "mixed precision")
    refused(lambda: na.Engine(m, n, r, "mu", mixed_precision=True), "mixed precision", "dense divergence")
    refused(lambda: na.Engine(m, n, r, "mu", divergence="kl", mixed_precision=True), "mixed precision")      # (the sparse KL engine)
    # 'precision' stays what it was on these engines, with its present message
    refused(lambda: na.Engine(m, n, r, "mu", divergence="is", precision="bf16"), "no bf16 operands")
    refused(lambda: na.Engine(m, n, r, "mu", divergence="is", precision="bf16", mixed_precision=True), "no bf16 operands")
    st, h, why = create_raw(params_v5(3.0, 0.5, 2.0), C.sizeof(engine_module._ParamsV5))
    assert st == 1 and not h and "mixedPrecision" in why, (st, why)
    st, h, why = create_raw(params_v5(3.0, 0.5, 0.5), C.sizeof(engine_module._ParamsV5))
    assert st == 1 and not h and "mixedPrecision" in why, (st, why)


def test_a_v4_sized_struct_is_the_fp32_engine():
    # the field behind the size given is not read: the same bytes with the v4 size create the engine of the parent
    p = params_v5(3.0, 0.5, 1.0)
    lib = engine_module.library()
    kernels = []
    for size in (C.sizeof(engine_module._ParamsV4), C.sizeof(engine_module._ParamsV5)):
        st, h, why = create_raw(p, size)
        assert st == 0 and h, why
        g = engine_module._Geometry()
        assert lib.nmfamd_engine_geometry_sized(h, C.byref(g), C.c_ulong(C.sizeof(g))) == 0
        kernels.append((g.product_kernel, g.resident_images))
        lib.nmfamd_engine_destroy(h)
    assert kernels == [(6, 2), (7, 2)]
    assert C.sizeof(engine_module._ParamsV4) == 13 * 8 and C.sizeof(engine_module._ParamsV5) == 14 * 8


def test_the_three_phase_calls_are_refused():
    m, n, r = 60, 50, 4
    V = np.asfortranarray(gen.planted(m, n, seed=93).astype(np.float32))
    W0, H0 = gen.start(m, n, r, 94, np.float32)
    eng = engine(m, n, r, 0.5)
    eng.upload(V)
    eng.set_factors(W0, H0)
    refused(lambda: eng.h_step(True), "dense divergence")
    got = run_engine(eng, W0, H0, 3)      # (the engine itself is unharmed)
    check(got, emulated(V, W0, H0, 3, 0.5), "after the refused call")
    eng.close()


def test_the_kernel_entry_is_float32_only():
    A, B, X, r, out_valid, red_valid = cases.half_step_case(64, 135)
    with pytest.raises(TypeError):
        na.op_beta_half_step_mixed(A.astype(np.float64), B.astype(np.float64), X.astype(np.float64), r, out_valid, red_valid, 0.5)
    with pytest.raises(na.EngineError):
        na.op_beta_half_step_mixed(A, B, X, r, out_valid, red_valid, float("nan"))


@pytest.fixture(scope="module")
def ctx():
    assert na.initialize() in (na.ResultType.Success, na.ResultType.ErrorAlreadyInitialized)
    na.set_verbosity(na.Verbosity.Nothing)
    yield
    na.finalize()


def test_compute(ctx):
    m, n, r, iters = 160, 120, 7, 20
    V = np.asfortranarray(gen.planted(m, n, seed=81).astype(np.float32))
    W0, H0 = gen.start(m, n, r, 82, np.float32)
    W, H = W0.copy(order="F"), H0.copy(order="F")
    s = na.Summary()
    assert na.compute(V, W, H, iterations=iters, parameters={"divergence": 3, "beta": 0.5, "mixedPrecision": 1}, summary=s) == na.ResultType.Success
    eng = engine(m, n, r, 0.5)
    eng.upload(V)
    want = run_engine(eng, W0, H0, iters)
    eng.close()
    rec = s.record(0)
    print(f"compute against the engine: W {rel(W, want[0]):.2e} H {rel(H, want[1]):.2e} frobenius {abs(rec.frobenius / want[2] - 1):.2e}")
    assert np.array_equal(W, want[0]) and np.array_equal(H, want[1])
    assert rec.frobenius == pytest.approx(want[2], rel=1e-6) and rec.rmsd == pytest.approx(want[3], rel=1e-6) and rec.numIterations == iters
    s.destroy()
    # the fp32 engine of the same call is another iteration: the switch reached the engine
    W2, H2 = W0.copy(order="F"), H0.copy(order="F")
    assert na.compute(V, W2, H2, iterations=iters, parameters={"divergence": 3, "beta": 0.5}) == na.ResultType.Success
    assert not np.array_equal(W2, W) and np.all(np.isfinite(W2))
    # refused before any device work: a value other than 0 / 1, double precision, another engine
    assert na.compute(V, W2, H2, iterations=2, parameters={"divergence": 3, "beta": 0.5, "mixedPrecision": 2}) == na.ResultType.ErrorInvalidArgument
    assert na.compute(V, W2, H2, iterations=2, parameters={"mixedPrecision": 1}) == na.ResultType.ErrorInvalidArgument
    V64, W64, H64 = V.astype(np.float64, order="F"), W0.astype(np.float64, order="F"), H0.astype(np.float64, order="F")
    assert na.compute(V64, W64, H64, iterations=2, parameters={"divergence": 3, "beta": 0.5, "mixedPrecision": 1}) == na.ResultType.ErrorInvalidArgument
