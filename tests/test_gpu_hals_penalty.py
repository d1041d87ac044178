"""HALS with L1 / L2 penalties (scikit-learn's coordinate descent, docs/HALS.md) on the GPU against the fp64 restatement of
tests/hals_penalty_reference.py.

Tolerances are those of tests/test_gpu_hals.py: factors within 2e-4 relative (fp32) and 1e-9 (fp64), the reported error within 1e-5 / 1e-9.  As
there, fp32 multi-iteration factor parity uses planted problems (on uniformly random V fp32 HALS trajectories drift apart on their own), and the
reported error is checked on random V, where the residual is large enough for the fp32 trace formula (relative error ~ eps (||V|| / error)^2);
after 20 fp32 iterations on random V only up to r = 200, as in test_parity_with_restatement.
"""
import numpy as np
import pytest

import nmfgpu_amd as na
from tests import hals_penalty_reference as pen
from tests import hals_reference as ref

pytestmark = pytest.mark.gpu

PEN = (0.5, 0.5, 0.1, 0.1)       # (l1W, l1H, l2W, l2H)


def F(a):
    return np.asfortranarray(a)


def problem(m, n, r, dtype, seed=1):
    rng = np.random.default_rng(seed)
    V = F(rng.random((m, n)).astype(dtype))
    W = F((1.0 - rng.random((m, r))).astype(dtype))
    H = F((1.0 - rng.random((r, n))).astype(dtype))
    return V, W, H


def planted(m, n, r, dtype, seed=1):
    rng = np.random.default_rng(seed)
    V = F((rng.random((m, r)) @ rng.random((r, n)) + 0.01 * rng.random((m, n))).astype(dtype))
    W = F((1.0 - rng.random((m, r))).astype(dtype))
    H = F((1.0 - rng.random((r, n))).astype(dtype))
    return V, W, H


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


def engine(V, W, H, **k):
    m, n = V.shape
    eng = na.Engine(m, n, W.shape[1], "hals", dtype=V.dtype, **k)
    eng.upload(V)
    eng.set_factors(W, H)
    return eng


def check_padding(eng):
    g = eng.geometry()
    RP, mp, np_ = g["padded_rank"], g["padded_m"], g["padded_n"]
    Wt = eng.debug_read(0, RP * mp).reshape(mp, RP)
    Hp = eng.debug_read(1, RP * np_).reshape(np_, RP)
    assert (Wt[:, eng.r:] == 0).all() and (Wt[eng.m:, :] == 0).all()
    assert (Hp[:, eng.r:] == 0).all() and (Hp[eng.n:, :] == 0).all()


# padded ranks 64, 128, 256 and one above (fp32: 384, fp64: 320)
PARITY = [(500, 300, 12, np.float32), (1000, 777, 100, np.float32), (1000, 777, 200, np.float32), (1000, 777, 300, np.float32),
          (500, 300, 12, np.float64), (1000, 777, 100, np.float64), (600, 500, 200, np.float64), (600, 500, 300, np.float64)]


@pytest.mark.parametrize("m,n,r,dtype", PARITY)
def test_parity_with_restatement(m, n, r, dtype):
    tol_f, tol_e = (2e-4, 1e-5) if dtype == np.float32 else (1e-9, 1e-9)
    for kind in ("planted", "random"):
        V, W, H = (planted if kind == "planted" else problem)(m, n, r, dtype, seed=m + n + r)
        eng = engine(V, W, H, **kw(PEN))
        assert eng.geometry()["fused_launches"] == 0
        W64, H64 = W.astype(np.float64), H.astype(np.float64)
        done = 0
        for iters in (1, 20):
            W64, H64, errs = pen.run(V.astype(np.float64), W64, H64, iters - done, *PEN)
            eng.iterate(iters - done, first_iteration=done + 1, error_every=0, last_iteration=iters)
            done = iters
            Wg, Hg = eng.get_factors()
            reported = eng.frobenius
            print(kind, iters, "rel W", rel(Wg, W64), "rel H", rel(Hg, H64), "error", reported, errs[-1])
            if kind == "planted" or iters == 1:
                assert rel(Wg, W64) < tol_f and rel(Hg, H64) < tol_f, (kind, iters, rel(Wg, W64), rel(Hg, H64))
            if kind == "random" and (iters == 1 or dtype == np.float64 or r <= 200):
                # ||V - W_{k-1} H_k||, not the penalised objective
                assert abs(reported - errs[-1]) <= tol_e * errs[-1], (iters, reported, errs[-1])
        check_padding(eng)
        eng.close()


@pytest.mark.parametrize("dtype,slack", [(np.float32, 1e-6), (np.float64, 1e-12)])
@pytest.mark.parametrize("p", [PEN, (0.0, 2.0, 0.0, 0.0), (0.0, 0.0, 1.0, 1.0)])
def test_penalised_objective_is_monotone(dtype, slack, p):
    V, W, H = problem(600, 400, 16, dtype, seed=9)
    eng = engine(V, W, H, **kw(p))
    objs = [pen.objective(V, W, H, *p)]
    for it in range(1, 61):
        eng.iterate(1, first_iteration=it, error_every=0)
        objs.append(pen.objective(V, *eng.get_factors(), *p))
    eng.close()
    for a, b in zip(objs, objs[1:]):
        assert b <= a * (1 + slack), (a, b)
    assert objs[-1] < objs[0]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_normalisation_runs_only_without_penalties(dtype):
    V, W, H = problem(400, 300, 10, dtype, seed=3)
    tol = 1e-5 if dtype == np.float32 else 1e-12
    eng = engine(V, W, H, **kw(PEN))
    eng.iterate(1, error_every=0)
    norms = np.linalg.norm(eng.get_factors()[0].astype(np.float64), axis=0)
    want = np.linalg.norm(pen.iteration(V, W, H, *PEN)[0], axis=0)
    assert (np.abs(norms - 1.0) > 0.1).all() and np.allclose(norms, want, rtol=1e-3), norms
    W1, H1 = eng.get_factors()
    eng.set_penalties()
    eng.iterate(1, first_iteration=2, error_every=0)
    norms = np.linalg.norm(eng.get_factors()[0].astype(np.float64), axis=0)
    # (from this start the first sweeps clamp some components to zero for good: a zero column keeps its d = 0 guard, the others are unit)
    live = np.linalg.norm(ref.iteration(V, W1, H1)[0], axis=0) > 0
    assert live.sum() >= 3 and np.array_equal(norms > 0, live), (norms, live)
    assert (np.abs(norms[live] - 1.0) < tol).all(), norms
    eng.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_constant_w_sweeps_h_with_its_penalties(dtype):
    tol_f, tol_e = (2e-4, 1e-5) if dtype == np.float32 else (1e-9, 1e-9)
    V, W, H = problem(700, 500, 24, dtype, seed=13)
    p = (3.0, 20.0, 5.0, 50.0)                              # (the W penalties are not used)
    eng = engine(V, W, H, **kw(p))
    eng.iterate(10, error_every=5, constant_w=True)
    Wg, Hg = eng.get_factors()
    assert np.array_equal(Wg, W)
    _, H64, errs = pen.run(V.astype(np.float64), W, H, 10, *p, constant_w=True)
    _, H0, _ = ref.run(V.astype(np.float64), W, H, 10, constant_w=True)
    assert rel(Hg, H64) < tol_f, rel(Hg, H64)
    assert rel(H0, H64) > 100 * tol_f                       # (the penalties matter here)
    assert abs(eng.frobenius - errs[-1]) <= tol_e * errs[-1]
    check_padding(eng)
    eng.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_explicit_zeros_are_the_unpenalised_engine(dtype):
    V, W, H = problem(500, 300, 70, dtype, seed=5)
    out = []
    for k in ({}, kw((0.0, 0.0, 0.0, 0.0))):
        eng = engine(V, W, H, **k)
        eng.iterate(5, error_every=0, last_iteration=5)
        out.append(eng.get_factors() + (eng.frobenius,))
        eng.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_penalties_set_and_reset_between_iterations(dtype):
    """A regularisation path on one resident V: ten penalised iterations, then the penalties back to zero and ten more."""
    tol_f, tol_e = (2e-4, 1e-5) if dtype == np.float32 else (1e-9, 1e-9)
    V, W, H = planted(800, 600, 20, dtype, seed=17)
    eng = engine(V, W, H)
    eng.set_penalties(*PEN)
    eng.iterate(10, error_every=0, last_iteration=10)
    W64, H64, _ = pen.run(V.astype(np.float64), W, H, 10, *PEN)
    Wg, Hg = eng.get_factors()
    assert rel(Wg, W64) < tol_f and rel(Hg, H64) < tol_f, (rel(Wg, W64), rel(Hg, H64))
    eng.set_penalties(0.0, 0.0, 0.0, 0.0)
    eng.iterate(10, first_iteration=11, error_every=0, last_iteration=20)
    W64, H64, _ = pen.run(V.astype(np.float64), W64, H64, 10)
    Wg, Hg = eng.get_factors()
    assert rel(Wg, W64) < tol_f and rel(Hg, H64) < tol_f, (rel(Wg, W64), rel(Hg, H64))
    assert (np.abs(np.linalg.norm(Wg.astype(np.float64), axis=0) - 1.0) < 1e-5).all()
    check_padding(eng)
    eng.close()


def test_l1_makes_the_factors_sparse():
    """The problem of tests/test_hals_penalty_cpu.py: after 30 iterations at least four times as many exact zeros in H (and W) with
    l1W = l1H = 5 as without, on the GPU and against the restatement's unpenalised count.  The counts themselves are compared with the restatement's
    loosely, by what the fp32 factor tolerance implies and no more: with tau = 2e-4 ||X64|| (no element is further off than the norm allows), a GPU
    zero needs a restatement entry <= tau, and a restatement zero a GPU entry <= tau -- an fp32 clamp may differ on entries at rounding level."""
    rng = np.random.default_rng(7)
    m, n, r = 300, 200, 12
    V = F((rng.random((m, r)) @ rng.random((r, n)) + 0.01 * rng.random((m, n))).astype(np.float32))
    W = F((1.0 - rng.random((m, r))).astype(np.float32))
    H = F((1.0 - rng.random((r, n))).astype(np.float32))
    zeros, zeros64 = {}, {}
    for l1 in (0.0, 5.0):
        eng = engine(V, W, H, l1_w=l1, l1_h=l1)
        eng.iterate(30, error_every=0)
        Wg, Hg = eng.get_factors()
        eng.close()
        W64, H64, _ = pen.run(V.astype(np.float64), W, H, 30, l1, l1, 0.0, 0.0)
        zeros[l1] = (int((Wg == 0).sum()), int((Hg == 0).sum()))
        zeros64[l1] = (int((W64 == 0).sum()), int((H64 == 0).sum()))
        print("l1", l1, "zeros (W, H)", zeros[l1], "restatement", zeros64[l1], "rel W", rel(Wg, W64), "rel H", rel(Hg, H64))
        assert rel(Wg, W64) < 2e-4 and rel(Hg, H64) < 2e-4, (l1, rel(Wg, W64), rel(Hg, H64))
        for got, want, count, count64 in ((Wg, W64, zeros[l1][0], zeros64[l1][0]), (Hg, H64, zeros[l1][1], zeros64[l1][1])):
            tau = 2e-4 * np.linalg.norm(want)
            assert count <= int((want <= tau).sum()), (l1, count, int((want <= tau).sum()))
            assert count64 <= int((got <= tau).sum()), (l1, count64, int((got <= tau).sum()))
    assert zeros[5.0][1] >= 4 * zeros[0.0][1] and zeros[5.0][0] >= 4 * zeros[0.0][0], zeros
    assert zeros[5.0][1] >= 4 * zeros64[0.0][1] and zeros[5.0][0] >= 4 * zeros64[0.0][0], (zeros, zeros64)
    assert zeros[0.0][1] > 0


def test_setter_refusals():
    V, W, H = problem(200, 150, 6, np.float32)
    eng = engine(V, W, H)
    for p in ((-1.0, 0, 0, 0), (0, float("nan"), 0, 0), (0, 0, float("inf"), 0), (0, 0, 0, -1e-30), (1e300, 0, 0, 0)):
        with pytest.raises(na.EngineError) as info:
            eng.set_penalties(*p)
        assert info.value.status == 1 and "penalties" in str(info.value), (p, str(info.value))
    # a refused call changes nothing: the iteration is the unpenalised one
    eng.iterate(1, error_every=1)
    W64, H64, err = ref.iteration(V, W, H)
    assert rel(eng.get_factors()[0], W64) < 2e-4 and abs(eng.frobenius - err) <= 1e-5 * err
    eng.close()
    with pytest.raises(na.EngineError) as info:
        na.Engine(200, 150, 6, "hals", l1_h=-2.0)
    assert info.value.status == 1
    mu = na.Engine(200, 150, 6, "mu", l1_w=0.0, l2_h=0.0)          # zeros are accepted by every algorithm
    mu.set_penalties(0.0, 0.0, 0.0, 0.0)
    with pytest.raises(na.EngineError) as info:
        mu.set_penalties(0.0, 0.5, 0.0, 0.0)
    assert info.value.status == 1 and "HALS" in str(info.value)
    mu.close()
    with pytest.raises(na.EngineError):
        na.Engine(200, 150, 6, "mu", l2_w=1.0)


def test_penalties_survive_the_native_fp32_fallback():
    """An upload with a value outside the split-operand product's range makes the Python Engine recreate itself on the native fp32 products
    (r = 64: the engine starts on the split-operand products): the penalties go along -- those of the constructor, and those of a later set_penalties."""
    m, n, r = 640, 520, 64
    V, W, H = planted(m, n, r, np.float32, seed=19)
    V[5, 7] = 1e-40                                         # (a denormal: NMFAMD_VALUE_RANGE on the first upload)
    p2 = (0.25, 0.75, 0.05, 0.2)
    for ctor, later in ((PEN, None), ((0.0, 0.0, 0.0, 0.0), p2)):
        eng = na.Engine(m, n, r, "hals", **kw(ctor))
        if later is not None:
            eng.set_penalties(*later)
        assert eng.geometry()["product_kernel"] == 2
        eng.upload(V)
        assert eng.geometry()["product_kernel"] == 0        # (another engine behind the same object)
        eng.set_factors(W, H)
        eng.iterate(3, error_every=0, last_iteration=3)
        p = later if later is not None else ctor
        W64, H64, errs = pen.run(V.astype(np.float64), W, H, 3, *p)
        Wg, Hg = eng.get_factors()
        print(p, "rel W", rel(Wg, W64), "rel H", rel(Hg, H64), "unpenalised rel W", rel(ref.run(V.astype(np.float64), W, H, 3)[0], W64))
        assert rel(Wg, W64) < 2e-4 and rel(Hg, H64) < 2e-4, (p, rel(Wg, W64), rel(Hg, H64))
        # the unpenalised iteration (what a recreated engine without the penalties would run) is far from it: normalised W
        assert rel(ref.run(V.astype(np.float64), W, H, 3)[0], W64) > 0.1
        eng.close()


# ------------------------------------------------------------------ through nmfgpu::compute

PARAMS = {"l1W": PEN[0], "l1H": PEN[1], "l2W": PEN[2], "l2H": PEN[3]}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_compute_copy_existing(dtype):
    tol_f, tol_e = (2e-4, 1e-5) if dtype == np.float32 else (1e-9, 1e-9)
    V, W, H = problem(800, 600, 12, dtype, seed=23)
    W64, H64, errs = pen.run(V.astype(np.float64), W, H, 30, *PEN)
    s = na.Summary()
    res = na.compute(V, W, H, algorithm=na.NmfAlgorithm.HALS, iterations=30, parameters=PARAMS, summary=s)
    assert res == na.ResultType.Success, res
    assert rel(W, W64) < tol_f and rel(H, H64) < tol_f, (rel(W, W64), rel(H, H64))
    rec = s.record(0)
    assert abs(rec.frobenius - errs[-1]) <= tol_e * errs[-1], (rec.frobenius, errs[-1])
    assert rec.numIterations == 30
    # the unpenalised run is another one
    assert abs(ref.run(V.astype(np.float64), W, H, 30)[2][-1] - errs[-1]) > 100 * tol_e * errs[-1]


def test_compute_threshold_and_two_runs():
    V, W, H = problem(800, 600, 12, np.float32, seed=31)
    s = na.Summary()
    res = na.compute(V, W, H, algorithm=na.NmfAlgorithm.HALS, iterations=2000, threshold=1e-2, parameters=PARAMS, summary=s)
    assert res == na.ResultType.Success, res
    rec = s.record(0)
    assert rec.numIterations < 2000
    # the reported error is ||V - W H|| of the last H step, not the penalised objective (which is far larger here)
    got = np.linalg.norm(V.astype(np.float64) - W.astype(np.float64) @ H.astype(np.float64))
    assert rec.frobenius > 0 and abs(got - rec.frobenius) < 0.01 * rec.frobenius, (got, rec.frobenius)
    best = {}
    for runs in (1, 2):
        s = na.Summary()
        res = na.compute(V, W, H, algorithm=na.NmfAlgorithm.HALS, init=na.NmfInitializationMethod.AllRandomValues, iterations=40, runs=runs, seed=5,
                         parameters=PARAMS, summary=s)
        assert res == na.ResultType.Success, res
        assert 1 <= s.record_count() <= runs
        best[runs] = s.record(s.best_run()).frobenius
        assert best[runs] == min(s.record(i).frobenius for i in range(s.record_count()))
    assert best[2] <= best[1]


def test_compute_refusals_on_the_gpu_path():
    V, W, H = problem(300, 200, 8, np.float32)
    W0, H0 = W.copy(), H.copy()
    bad = na.ResultType.ErrorInvalidArgument
    for params in ({"l1W": -1.0}, {"l2H": float("nan")}, {"l1H": float("inf")}):
        assert na.compute(V, W, H, algorithm=na.NmfAlgorithm.HALS, iterations=5, parameters=params) == bad
    assert na.compute(V, W, H, iterations=5, parameters={"l1W": 0.5}) == bad
    assert np.array_equal(W, W0) and np.array_equal(H, H0)
    # zero-valued penalties with the multiplicative update: the same run as without them
    Wa, Ha, Wb, Hb = W.copy(order="F"), H.copy(order="F"), W.copy(order="F"), H.copy(order="F")
    assert na.compute(V, Wa, Ha, iterations=5, parameters={"l1W": 0.0, "l1H": 0.0, "l2W": 0.0, "l2H": 0.0}) == na.ResultType.Success
    assert na.compute(V, Wb, Hb, iterations=5) == na.ResultType.Success
    assert np.array_equal(Wa, Wb) and np.array_equal(Ha, Hb)
