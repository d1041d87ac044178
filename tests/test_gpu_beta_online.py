"""Minibatch (online) dense beta-divergence NMF on the GPU (docs/DIVERGENCE.md, "Minibatch update"): the update launch k_beta_update_rows through
op_beta_update_rows, and the engine with batch_size against the numpy restatement (tests/beta_online_reference.py).  The cases, the tolerances and the reasoning
behind them are in tests/beta_online_cases.py; tests/test_beta_online_cpu.py recomputes the figures they rest on without a GPU."""
import ctypes as C

import numpy as np
import pytest

import nmfgpu_amd as na
from nmfgpu_amd import engine as engine_module
from tests import beta_general_reference as gen
from tests import beta_online_cases as cases

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


def eps_of(dtype):
    return float(np.finfo(dtype).eps)


def kwargs_of(beta, pen=gen.NO_PENALTIES):
    kw = dict(l1_w=pen[0], l1_h=pen[1], l2_w=pen[2], l2_h=pen[3])
    if beta == 0:
        return dict(divergence="is", **kw)
    if beta == 1:
        return dict(divergence="kl", dense_compute=True, **kw)
    return dict(divergence="beta", beta=beta, **kw)


def run_engine(eng, W0, H0, passes, first=1):
    if W0 is not None:
        eng.set_factors(W0, H0)
    eng.iterate(passes, first_iteration=first, error_every=0, last_iteration=first + passes - 1)
    W, H = eng.get_factors()
    return W, H, eng.frobenius, eng.rmsd, eng.divergence_value


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


# 1. the kernel entry: every padded rank, both forms, both precisions; inside, every beta (vector and panel denominators, the three powers), slab count, rho and
#    penalty setting, on 203 valid rows of 256 with the constructed flush entries and zeros of P
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("RP", [64, 128, 256])
@pytest.mark.parametrize("online", [False, True])
def test_update_rows_kernel(online, RP, dtype):
    tol = 10 * eps_of(dtype)
    r, v = cases.KERNEL_RANKS[RP], cases.KERNEL_OUT_VALID
    worst = 0.0
    for beta in cases.KERNEL_BETAS:
        for slabs in cases.KERNEL_SLABS:
            for rho in (cases.KERNEL_RHOS if online else (0.0,)):
                for pen in cases.KERNEL_PENALTIES:
                    P, num, den, A, B = cases.kernel_case(RP, dtype, beta, slabs, online, rho, pen)
                    want = cases.kernel_reference(P, num, den, A, B, RP, beta, online, rho, pen, dtype)
                    res = na.op_beta_update_rows(P, num, den, r, v, beta, l1=pen[0], l2=pen[1], acc=(A, B) if online else None, rho=rho, flush=True)
                    got = res["P"]
                    figs = [cases.rel(got[:v, :r], want[0])]
                    if online:
                        figs += [cases.rel(res["A"][:v, :r], want[1]), cases.rel(res["B"][:v, :r], want[2])]
                        # the accumulators are not touched on the padding
                        assert np.array_equal(res["A"][v:], A[v:]) and np.array_equal(res["A"][:, r:], A[:, r:])
                        assert np.array_equal(res["B"][v:], B[v:]) and np.array_equal(res["B"][:, r:], B[:, r:])
                    else:
                        assert res["A"] is None and res["B"] is None
                    worst = max(worst, *figs)
                    assert max(figs) < tol, (beta, slabs, rho, pen, figs)
                    assert np.all(np.isfinite(got)) and np.all(got[v:] == 0) and np.all(got[:, r:] == 0)
                    # the flush: eps / 4 goes to 0, 4 eps stays; a zero of P comes back exactly where rho A > 0
                    assert np.all(got[cases.FLUSH_LOW] == 0) and np.all(got[cases.FLUSH_HIGH] > 0)
                    assert np.all((got[cases.ZERO_ENTRIES] > 0) == (online and rho > 0))
                    assert np.array_equal(got[:v, :r] == 0, want[0] == 0)
                    sums = got.astype(np.float64).reshape(-1, 16, RP).sum(axis=1)
                    assert res["sum_part"].shape == (cases.KERNEL_OUT_PAD // 16, RP)
                    assert np.allclose(res["sum_part"], sums, rtol=10 * tol, atol=0)
    print(f"update rows {'online' if online else 'plain'} RP {RP} {np.dtype(dtype).name}: worst norm-relative figure {worst:.2e} (tolerance {tol:.2e})")


def test_update_rows_without_flush_and_refusals():
    RP, dtype, beta = 64, np.float32, 0.5
    r, v = cases.KERNEL_RANKS[RP], cases.KERNEL_OUT_VALID
    P, num, den, A, B = cases.kernel_case(RP, dtype, beta, 3, True, 0.4, (0.0, 0.0))
    kept = na.op_beta_update_rows(P, num, den, r, v, beta, acc=(A, B), rho=0.4, flush=False)["P"]
    assert np.all(kept[cases.FLUSH_LOW] > 0) and np.all(kept[cases.FLUSH_LOW] < eps_of(dtype))
    for bad in (dict(rho=1.5), dict(rho=float("nan")), dict(l1=-1.0)):
        with pytest.raises(na.EngineError):
            na.op_beta_update_rows(P, num, den, r, v, beta, **{"acc": (A, B), "rho": 0.4, **bad})
    with pytest.raises(na.EngineError):
        na.op_beta_update_rows(P, num, den, r, v, float("nan"))
    with pytest.raises(na.EngineError):
        na.op_beta_update_rows(P[:200], num[:, :200], den[:, :200], r, 100, beta)      # (out_pad is not a multiple of 128)


# 2. the engine against the restatement: 128 / 128 / 44 columns at RP = 64 in both precisions, RP = 256 with a remainder of 72, one batch that holds all of V
@pytest.mark.parametrize("shape,beta,pen,dtype", cases.engine_cases())
def test_engine_against_restatement(shape, beta, pen, dtype):
    m, n, r, batch = shape
    V, W0, H0 = cases.problem(shape, beta, dtype)
    want = cases.reference_run(shape, beta, eps_of(dtype), pen, data=dtype)
    assert want[5] == 0      # (the fp64 restatement flushes nothing on this data)
    eng = na.Engine(m, n, r, "mu", dtype=dtype, batch_size=batch, forget_factor=cases.FORGET, **kwargs_of(beta, pen))
    g = eng.geometry()
    rp = g["padded_rank"]
    assert g["product_kernel"] == 6 and g["resident_images"] == 2
    eng.upload(V)
    got = run_engine(eng, W0, H0, cases.PASSES)
    factors, errors = cases.figures(got, want)
    print(f"minibatch {shape} beta {beta} pen {pen} {np.dtype(dtype).name}: factors {factors:.2e} errors {errors:.2e}")
    ftol, etol = cases.TOL[dtype]
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1]))
    assert factors < ftol and errors < etol
    # coordinates >= r and the padding stay 0
    Hp = eng.debug_read(1, rp * g["padded_n"]).reshape(g["padded_n"], rp)
    Wp = eng.debug_read(0, rp * g["padded_m"]).reshape(g["padded_m"], rp)
    assert np.all(Hp[:, r:] == 0) and np.all(Hp[n:] == 0) and np.all(Wp[:, r:] == 0) and np.all(Wp[m:] == 0)
    # the full-batch engine of the same parameters is another iteration: the switch reached the engine
    full = na.Engine(m, n, r, "mu", dtype=dtype, **kwargs_of(beta, pen))
    full.upload(V)
    other = run_engine(full, W0, H0, cases.PASSES)
    assert cases.rel(other[0], got[0]) > 1e-3
    full.close()
    eng.close()


def test_mixed_engine_against_the_emulating_restatement():
    shape, beta = cases.MIXED_CASE
    m, n, r, batch = shape
    V, W0, H0 = cases.problem(shape, beta, np.float32)
    want = cases.reference_run(shape, beta, cases.EPS32, mixed=True)
    assert want[5] == 0
    eng = na.Engine(m, n, r, "mu", batch_size=batch, forget_factor=cases.FORGET, mixed_precision=True, **kwargs_of(beta))
    assert eng.geometry()["product_kernel"] == 7
    eng.upload(V)
    got = run_engine(eng, W0, H0, cases.PASSES)
    factors, errors = cases.figures(got, want)
    print(f"mixed minibatch {shape} beta {beta}: factors {factors:.2e} (tolerance {cases.MARGIN * cases.FIGURE_MIXED_FACTORS:.2e}) errors {errors:.2e} "
          f"(tolerance {cases.MARGIN * cases.FIGURE_MIXED_ERRORS:.2e})")
    assert factors < cases.MARGIN * cases.FIGURE_MIXED_FACTORS and errors < cases.MARGIN * cases.FIGURE_MIXED_ERRORS
    eng.close()


# 3. reproducibility; set_factors starts the accumulators again; passes can be split over calls
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("beta", [0.5, 1.0])
def test_repeated_runs_are_bit_identical(beta, dtype):
    shape = (140, 1500, 8, 256)      # six batches, the last one of 220 columns; several slabs in the H-side launches
    m, n, r, batch = shape
    V, W0, H0 = cases.problem(shape, beta, dtype)
    outs = []
    for _ in range(2):
        eng = na.Engine(m, n, r, "mu", dtype=dtype, batch_size=batch, **kwargs_of(beta, cases.PEN))
        eng.upload(V)
        outs.append(run_engine(eng, W0, H0, 4))
        again = run_engine(eng, W0, H0, 4)      # (the same engine from the same start: A and B were set again)
        assert same(outs[-1], again)
        # four passes in one call are two and two
        eng.set_factors(W0, H0)
        eng.iterate(2, first_iteration=1, error_every=0, last_iteration=4)
        split = run_engine(eng, None, None, 2, first=3)
        assert same(outs[-1], split)
        eng.close()
    assert same(outs[0], outs[1])


# 4. batch_size = 0 / None is today's engine, bit for bit; a v5-sized struct with v6 bytes behind it too
def create_raw(params, size, m=60, n=50, r=4, elem_bytes=4):
    lib = engine_module.library()
    lib.nmfamd_engine_last_error.restype = C.c_char_p
    h = C.c_void_p()
    st = lib.nmfamd_engine_create_v2(m, n, r, engine_module.ALGORITHMS["mu"], C.byref(params), C.c_ulong(size), elem_bytes, C.c_void_p(0), 1, C.byref(h))
    return st, h, (lib.nmfamd_engine_last_error(None) or b"").decode()


def params_v6(divergence, beta, batch, forget, weighted=0.0, mixed=0.0, dense=0.0):
    P = engine_module
    v5 = P._ParamsV5(P._ParamsV4(P._ParamsV3(P._ParamsV2(P._Params(0, 0, 0, 0, 0, 0, divergence, 0, 0, 0), dense), beta), weighted), mixed)
    return P._ParamsV6(v5, batch, forget)


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_batch_size_is_the_full_batch_engine(dtype):
    m, n, r, beta = 150, 300, 9, 0.5
    V, W0, H0 = cases.problem((m, n, r, 0), beta, dtype)
    outs = []
    for kw in (dict(), dict(batch_size=None), dict(batch_size=0), dict(batch_size=0, forget_factor=0.3)):
        eng = na.Engine(m, n, r, "mu", dtype=dtype, **kwargs_of(beta), **kw)
        eng.upload(V)
        outs.append(run_engine(eng, W0, H0, 6))
        eng.close()
    want = gen.run(V.astype(np.float64), W0.astype(np.float64), H0.astype(np.float64), 6, beta, eps_of(dtype))
    assert cases.rel(outs[0][0], want[0]) < cases.TOL[dtype][0]
    assert all(same(outs[0], o) for o in outs[1:])


def test_a_v5_sized_struct_is_the_full_batch_engine():
    assert C.sizeof(engine_module._ParamsV6) == 16 * 8 and C.sizeof(engine_module._ParamsV5) == 14 * 8
    m, n, r, beta = 150, 300, 9, 0.5
    V, W0, H0 = cases.problem((m, n, r, 0), beta, np.float32)
    wants = []
    for kw in (dict(), dict(batch_size=128, forget_factor=0.7)):
        eng = na.Engine(m, n, r, "mu", **kwargs_of(beta), **kw)
        eng.upload(V)
        wants.append(run_engine(eng, W0, H0, 5))
        eng.close()
    p = params_v6(3.0, beta, 128.0, 0.7)
    outs = []
    for size in (C.sizeof(engine_module._ParamsV5), C.sizeof(engine_module._ParamsV6)):
        st, h, why = create_raw(p, size, m, n, r)
        assert st == 0 and h, why
        eng = na.Engine.from_handle(h, m, n, r, np.float32)
        eng.upload(V)
        outs.append(run_engine(eng, W0, H0, 5))
        eng.close()
    assert same(outs[0], wants[0]) and same(outs[1], wants[1])
    assert not np.array_equal(outs[0][0], outs[1][0])


# 5. refusals, each by status and words, at creation
def refused(call, *words):
    with pytest.raises(na.EngineError) as e:
        call()
    text = str(e.value)
    assert e.value.status == 1, text
    for word in words:
        assert word in text, text


def test_refusals_at_creation():
    m, n, r = 60, 50, 4
    for b in (100, 64, -128, 192, 128.5, float("nan"), float("inf")):
        refused(lambda: na.Engine(m, n, r, "mu", divergence="is", batch_size=b), "batchSize", "multiple of 128")
    for f in (-0.1, 1.5, float("nan"), float("inf")):
        refused(lambda: na.Engine(m, n, r, "mu", divergence="is", batch_size=128, forget_factor=f), "forgetFactor", "[0, 1]")
    refused(lambda: na.Engine(m, n, r, "mu", batch_size=128), "minibatch", "dense divergence")
    refused(lambda: na.Engine(m, n, r, "hals", batch_size=128), "minibatch", "dense divergence")
    refused(lambda: na.Engine(m, n, r, "mu", divergence="kl", batch_size=128), "minibatch", "dense divergence")      # (the sparse KL engine)
    refused(lambda: na.Engine(m, n, r, "mu", divergence="is", weighted=True, batch_size=128), "minibatch", "weighted")
    # a forgetting factor without a batch size: the C struct takes the value literally
    st, h, why = create_raw(params_v6(2.0, 0.0, 0.0, 0.7), C.sizeof(engine_module._ParamsV6))
    assert st == 1 and not h and "forgetFactor" in why and "batchSize" in why, (st, why)
    st, h, why = create_raw(params_v6(2.0, 0.0, 0.0, 0.0), C.sizeof(engine_module._ParamsV6))
    assert st == 0 and h, why
    engine_module.library().nmfamd_engine_destroy(h)
    # forget_factor = 0 with a batch size is allowed: every step keeps only its own numerator and denominator
    eng = na.Engine(m, n, r, "mu", divergence="is", batch_size=128, forget_factor=0.0)
    eng.close()


def test_constant_w_and_the_three_phase_calls_are_refused():
    shape, beta = (60, 200, 4, 128), 0.5
    m, n, r, batch = shape
    V, W0, H0 = cases.problem(shape, beta, np.float32)
    eng = na.Engine(m, n, r, "mu", batch_size=batch, **kwargs_of(beta))
    eng.upload(V)
    eng.set_factors(W0, H0)
    refused(lambda: eng.iterate(1, constant_w=True), "minibatch", "constant")
    # every three-phase, row-block and sharded entry point, as on the full-batch engines
    import torch
    ex = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")
    refused(lambda: eng.h_step(True), "dense divergence", "h_step")
    refused(lambda: eng.w_products(ex.data_ptr()), "dense divergence", "w_products")
    refused(lambda: eng.w_finish(ex.data_ptr(), True), "dense divergence", "w_finish")
    refused(lambda: eng.w_update_rows(ex.data_ptr(), ex.data_ptr(), 0, m, False, ex.data_ptr()), "dense divergence", "w_update_rows")
    refused(lambda: eng.w_normalize_rows(0, m, ex.data_ptr()), "dense divergence", "w_normalize_rows")
    refused(lambda: na.Engine(m, n, r, "mu", batch_size=batch, row_blocks=2, **kwargs_of(beta)), "dense divergence", "row blocks")
    group = na.LocalGroup(1)
    comm = na.LocalComm(group, 0)
    with pytest.raises(na.EngineError) as e:
        na.ShardedRun(eng, comm, m, n, na.SHARD_REPLICATED)
    assert e.value.status == 1
    comm.close()
    got = run_engine(eng, W0, H0, 3)      # (the engine itself is unharmed)
    want = cases.onl.run(V.astype(np.float64), W0.astype(np.float64), H0.astype(np.float64), 3, beta, cases.EPS32, batch, 0.7)
    factors, errors = cases.figures(got, want)
    assert factors < cases.TOL[np.float32][0] and errors < cases.TOL[np.float32][1]
    eng.close()


# 6. forget_factor = 0 and one batch: the un-normalised full-batch update (the penalised full-batch engine does not normalise either)
def test_no_memory_and_one_batch_is_the_penalised_full_batch_iteration():
    m, n, r, beta = 203, 300, 9, 2.0
    V, W0, H0 = cases.problem((m, n, r, 0), beta, np.float64)
    mini = na.Engine(m, n, r, "mu", dtype=np.float64, batch_size=384, forget_factor=0.0, **kwargs_of(beta, cases.PEN))
    mini.upload(V)
    got = run_engine(mini, W0, H0, 1)
    mini.close()
    want = gen.run(V, W0, H0, 1, beta, eps_of(np.float64), pen=cases.PEN)
    assert cases.rel(got[0], want[0]) < 1e-12 and cases.rel(got[1], want[1]) < 1e-12


# 7. nmfgpu::compute with "batchSize"
@pytest.fixture(scope="module")
def ctx():
    assert na.initialize() in (na.ResultType.Success, na.ResultType.ErrorAlreadyInitialized)
    na.set_verbosity(na.Verbosity.Nothing)
    yield
    na.finalize()


def test_compute(ctx):
    shape, beta = cases.SHAPE_SMALL, 0.5
    m, n, r, batch = shape
    V, W0, H0 = cases.problem(shape, beta, np.float32)
    want = cases.reference_run(shape, beta, cases.EPS32)
    W, H = W0.copy(order="F"), H0.copy(order="F")
    s = na.Summary()
    assert na.compute(V, W, H, iterations=cases.PASSES, parameters={"divergence": 3, "beta": beta, "batchSize": batch}, summary=s) == na.ResultType.Success
    rec = s.record(0)
    ftol, etol = cases.TOL[np.float32]
    print(f"compute: W {cases.rel(W, want[0]):.2e} H {cases.rel(H, want[1]):.2e} frobenius {abs(rec.frobenius / want[2] - 1):.2e}")
    assert cases.rel(W, want[0]) < ftol and cases.rel(H, want[1]) < ftol      # (an absent "forgetFactor" is 0.7)
    assert rec.frobenius == pytest.approx(want[2], rel=etol) and rec.rmsd == pytest.approx(want[3], rel=etol) and rec.numIterations == cases.PASSES
    s.destroy()
    eng = na.Engine(m, n, r, "mu", batch_size=batch, forget_factor=0.7, **kwargs_of(beta))
    eng.upload(V)
    same_run = run_engine(eng, W0, H0, cases.PASSES)
    eng.close()
    assert np.array_equal(W, same_run[0]) and np.array_equal(H, same_run[1])
    W2, H2 = W0.copy(order="F"), H0.copy(order="F")
    assert na.compute(V, W2, H2, iterations=cases.PASSES, parameters={"divergence": 3, "beta": beta, "batchSize": batch, "forgetFactor": 0.2}) == na.ResultType.Success
    assert not np.array_equal(W2, W) and np.all(np.isfinite(W2))
    # refused before any device work
    for params in ({"divergence": 3, "beta": beta, "batchSize": 100}, {"divergence": 3, "beta": beta, "forgetFactor": 0.5}, {"batchSize": 128},
                   {"divergence": 3, "beta": beta, "batchSize": 128, "forgetFactor": 1.5}):
        assert na.compute(V, W2, H2, iterations=2, parameters=params) == na.ResultType.ErrorInvalidArgument
