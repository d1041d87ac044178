"""Per-column dynamic stopping of NeNMF's steps on the GPU, engine level (docs/NENMF.md, "Dynamic stopping"): Engine(..., "nenmf", step_tolerance=),
Engine.set_step_tolerance, Engine.step_counts and the "stepsTolerance" Parameter, against tests/nenmf_dyn_reference.py.

As at kernel level (tests/test_gpu_nenmf_dyn_steps.py) values and rule are checked separately: the restatement is fed the ENGINE's counts, read after every
iteration, and must give the engine's factors -- fp64 within 1e-9, fp32 within 4 x the distance of the fp32 numpy restatement from the fp64 one at the same counts
(tests/test_nenmf_dyn_cpu.py pins the figure) -- and, after the first iteration, the engine's counts must equal the restatement's own on at least 98 % of the
columns of H and of the rows of W.
"""
import numpy as np
import pytest

import nmfgpu_amd as na
from tests import hals_multi_cases as mc
from tests import nenmf_dyn_cases as dc
from tests import nenmf_dyn_reference as dyn

pytestmark = pytest.mark.gpu

SHAPES = [pytest.param(m, n, r, dtype, id=f"{m}x{n}-r{r}-{np.dtype(dtype).name}") for (m, n, r) in dc.ENGINE_SHAPES for dtype in (np.float32, np.float64)]
T_H, T_W = dc.ENGINE_STEPS


@pytest.fixture(scope="module", autouse=True)
def _library_is_native():
    assert na.device_count() >= 1, "GPU tests need a HIP device"
    assert na.initialize() in (na.ResultType.Success, na.ResultType.ErrorAlreadyInitialized)
    na.set_verbosity(na.Verbosity.Nothing)
    yield
    na.finalize()


def refused(call, *words):
    with pytest.raises(na.EngineError) as info:
        call()
    assert info.value.status == 1 and all(w in str(info.value) for w in words), str(info.value)


def make_engine(m, n, r, dtype, kind="plain", **kw):
    coo, V, W, H, p, constant_w = dc.engine_problem(m, n, r, dtype, kind)
    eng = na.Engine(m, n, r, "nenmf", dtype=dtype, sparse_compute=coo is not None, l1_w=p[0], l1_h=p[1], l2_w=p[2], l2_h=p[3], **kw)
    if coo is None:
        eng.upload(V)
    else:
        rows, cols, vals = coo
        ptr = np.zeros(m + 1, np.int32)
        np.cumsum(np.bincount(rows, minlength=m), out=ptr[1:])
        eng.upload_sparse(1, vals, ptr, cols.astype(np.int32), 0)
    eng.set_factors(W, H)
    return eng, V, W, H, p, constant_w


@pytest.mark.parametrize("kind", dc.ENGINE_KINDS)
@pytest.mark.parametrize("m,n,r,dtype", SHAPES)
def test_iterations_against_the_restatement_at_the_engines_counts(m, n, r, dtype, kind):
    """(12, 12) at delta = 0.1 after 1 and 5 iterations: plain, penalised, constant W and sparse compute."""
    tol = dc.engine_tolerance(dtype)
    eng, V, W, H, p, constant_w = make_engine(m, n, r, dtype, kind, steps_h=T_H, steps_w=T_W, step_tolerance=dc.ENGINE_TOL)
    forced, kept_w = [], None
    for it in range(1, max(dc.ENGINE_ITERS) + 1):
        eng.iterate(1, first_iteration=it, error_every=1, constant_w=constant_w)
        ch = eng.step_counts(0)
        assert ch.shape == (n,) and ch.dtype == np.int32 and ch.min() >= 1 and ch.max() <= T_H
        if constant_w:
            refused(lambda: eng.step_counts(1), "NeNMF", "counts")
            cw = None
        else:
            cw = eng.step_counts(1)
            assert cw.shape == (m,) and cw.min() >= 1 and cw.max() <= T_W
        forced.append((ch, cw))
        if it not in dc.ENGINE_ITERS:
            continue
        Wg, Hg = eng.get_factors()
        W64, H64, errs, _ = dyn.run(V, W, H, it, T_H, T_W, dc.ENGINE_TOL, p, constant_w, forced=forced)
        print(kind, it, "W", dc.rel(Wg, W64), "H", dc.rel(Hg, H64), "tolerance", tol, "error", eng.frobenius, errs[-1])
        if constant_w:
            assert np.array_equal(Wg, W)
        else:
            assert dc.rel(Wg, W64) < tol, (it, dc.rel(Wg, W64))
        assert dc.rel(Hg, H64) < tol, (it, dc.rel(Hg, H64))
        if dtype == np.float64:
            assert abs(eng.frobenius - errs[-1]) <= 1e-9 * errs[-1], (it, eng.frobenius, errs[-1])
        if it == 1:      # the rule: the restatement's own counts, on the first iteration (whose counts are diverse)
            _, _, _, own = dyn.run(V, W, H, 1, T_H, T_W, dc.ENGINE_TOL, p, constant_w)
            same_h = float((ch == own[0][0]).mean())
            same_w = 1.0 if constant_w else float((cw == own[0][1]).mean())
            print("    H counts", np.bincount(ch).tolist(), "equal on", same_h, "W counts", None if constant_w else np.bincount(cw).tolist(), "equal on", same_w)
            assert len(set(ch.tolist())) > 1, "every column took the same number of steps: the case shows nothing"
            assert same_h >= dc.FLIP_CAP and same_w >= dc.FLIP_CAP
    g = eng.geometry()
    RP, mp, np_ = g["padded_rank"], g["padded_m"], g["padded_n"]
    Wt, Hp = eng.debug_read(0, RP * mp).reshape(mp, RP), eng.debug_read(1, RP * np_).reshape(np_, RP)
    assert (Wt[:, r:] == 0).all() and (Wt[m:, :] == 0).all() and (Hp[:, r:] == 0).all() and (Hp[n:, :] == 0).all()
    eng.close()


@pytest.mark.parametrize("m,n,r,dtype", SHAPES)
def test_tolerance_zero_is_the_static_engine(m, n, r, dtype):
    """delta = 0 through every interface -- not given, the constructor argument, the setter (after a non-zero value) -- at steps (6, 4): the factors and errors of
    an engine that never heard of the tolerance, bit for bit, over 3 iterations; the counts are the static counts.  A maximum of 1 at delta > 0 is the static launch
    too, with counts of 1."""
    out = []
    for how in ("absent", "constructor", "setter"):
        eng, V, W, H, _, _ = make_engine(m, n, r, dtype, steps_h=6, steps_w=4, **(dict(step_tolerance=0.0) if how == "constructor" else {}))
        if how == "setter":
            eng.set_step_tolerance(0.25)
            eng.set_step_tolerance(0)
        errs = []
        for it in range(1, 4):
            eng.iterate(1, first_iteration=it, error_every=1)
            errs.append(eng.frobenius)
        out.append((*eng.get_factors(), errs))
        assert (eng.step_counts(0) == 6).all() and eng.step_counts(0).shape == (n,) and (eng.step_counts(1) == 4).all() and eng.step_counts(1).shape == (m,)
        eng.close()
    for other in out[1:]:
        assert np.array_equal(out[0][0], other[0]) and np.array_equal(out[0][1], other[1]) and out[0][2] == other[2]
    one = []
    for tol in (0.0, 0.5):
        eng, *_ = make_engine(m, n, r, dtype, steps_h=1, steps_w=1, step_tolerance=tol)
        eng.iterate(2, error_every=0, last_iteration=2)
        one.append((*eng.get_factors(), eng.frobenius))
        assert (eng.step_counts(0) == 1).all() and (eng.step_counts(1) == 1).all()
        eng.close()
    assert np.array_equal(one[0][0], one[1][0]) and np.array_equal(one[0][1], one[1][1]) and one[0][2] == one[1][2]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_setter_takes_effect_at_the_next_iteration(dtype):
    """Two static iterations, then set_step_tolerance(0.1) and one more: bit for bit a fresh engine created with the tolerance and started from the factors after
    the first two; the counts turn from the static count to the rule's."""
    m, n, r = dc.ENGINE_SHAPES[1]
    eng, V, W, H, _, _ = make_engine(m, n, r, dtype, steps_h=T_H, steps_w=T_W)
    eng.iterate(2, error_every=0)
    W2, H2 = eng.get_factors()
    assert (eng.step_counts(0) == T_H).all()
    eng.set_step_tolerance(dc.ENGINE_TOL)
    assert (eng.step_counts(0) == T_H).all(), "the counts of the step that ran stay until the next one"
    eng.iterate(1, first_iteration=3, error_every=1)
    Wa, Ha = eng.get_factors()
    ca, ea = (eng.step_counts(0), eng.step_counts(1)), eng.frobenius
    eng.close()
    fresh, *_ = make_engine(m, n, r, dtype, steps_h=T_H, steps_w=T_W, step_tolerance=dc.ENGINE_TOL)
    fresh.set_factors(W2, H2)
    fresh.iterate(1, first_iteration=3, error_every=1)
    Wb, Hb = fresh.get_factors()
    assert np.array_equal(Wa, Wb) and np.array_equal(Ha, Hb) and ea == fresh.frobenius
    assert np.array_equal(ca[0], fresh.step_counts(0)) and np.array_equal(ca[1], fresh.step_counts(1))
    fresh.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_step_counts_before_a_step_and_under_constant_w(dtype):
    m, n, r = dc.ENGINE_SHAPES[0]
    eng, V, W, H, _, _ = make_engine(m, n, r, dtype, steps_h=T_H, steps_w=T_W, step_tolerance=dc.ENGINE_TOL)
    refused(lambda: eng.step_counts(0), "NeNMF", "counts")              # (before any step)
    refused(lambda: eng.step_counts(1), "NeNMF", "counts")
    refused(lambda: eng.step_counts(2), "NeNMF", "which")
    eng.iterate(1, error_every=0)
    cw = eng.step_counts(1)
    assert len(set(cw.tolist())) > 1
    eng.iterate(2, first_iteration=2, error_every=0, constant_w=True)
    assert np.array_equal(eng.step_counts(1), cw), "constant W: the W counts are what the last W step left"
    assert eng.step_counts(0).shape == (n,)
    eng.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_compute_with_the_parameter_is_the_engine(dtype):
    m, n, r = dc.ENGINE_SHAPES[1]
    eng, V, W, H, _, _ = make_engine(m, n, r, dtype, steps_h=T_H, steps_w=T_W, step_tolerance=dc.ENGINE_TOL)
    eng.iterate(4, error_every=0, last_iteration=4)
    We, He = eng.get_factors()
    err = eng.frobenius
    eng.close()
    Wc, Hc = W.copy(order="F"), H.copy(order="F")
    s = na.Summary()
    res = na.compute(V, Wc, Hc, algorithm=na.NmfAlgorithm.NeNMF, iterations=4, parameters={"stepsH": T_H, "stepsW": T_W, "stepsTolerance": dc.ENGINE_TOL}, summary=s)
    assert res == na.ResultType.Success, res
    assert np.array_equal(Wc, We) and np.array_equal(Hc, He)
    assert abs(s.record(0).frobenius - err) <= 1e-12 * err
    Ws, Hs = W.copy(order="F"), H.copy(order="F")
    assert na.compute(V, Ws, Hs, algorithm=na.NmfAlgorithm.NeNMF, iterations=4, parameters={"stepsH": T_H, "stepsW": T_W}) == na.ResultType.Success
    assert not np.array_equal(Ws, Wc), "the tolerance changed nothing"


# ------------------------------------------------------------------ refusals

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bad_tolerances_are_refused(dtype):
    for bad in (-0.1, 1.0, 2.0, float("nan"), float("inf")):
        refused(lambda: na.Engine(60, 50, 8, "nenmf", dtype=dtype, step_tolerance=bad), "NeNMF", "tolerance")
    eng = na.Engine(60, 50, 8, "nenmf", dtype=dtype)
    for bad in (-0.1, -1e-300, 1.0, 2.0, float("nan"), float("inf")):
        refused(lambda: eng.set_step_tolerance(bad), "NeNMF", "tolerance", "[0, 1)")
    eng.set_step_tolerance(0.999)
    eng.set_step_tolerance(0.0)
    # HALS's own tolerance and counts stay refused on a NeNMF engine
    refused(lambda: eng.set_sweep_tolerance(0.1), "HALS")
    refused(lambda: eng.sweep_counts(0), "HALS")
    eng.close()


def test_other_engines_refuse_the_tolerance_and_have_no_step_counts():
    for k in (dict(algorithm="hals"), dict(algorithm="mu"), dict(algorithm="mu", divergence="is"), dict(algorithm="als")):
        eng = na.Engine(60, 50, 8, **k)
        refused(lambda: eng.set_step_tolerance(0.1), "NeNMF", "tolerance")
        refused(lambda: eng.set_step_tolerance(0.0), "NeNMF", "tolerance")
        refused(lambda: eng.step_counts(0), "NeNMF", "counts")
        eng.close()
        refused(lambda: na.Engine(60, 50, 8, step_tolerance=0.1, **k), "NeNMF")
    V, W, H = mc.planted(300, 257, 20, np.float64, seed=7)
    bad = na.ResultType.ErrorInvalidArgument
    for alg, prm in ((na.NmfAlgorithm.Multiplicative, {"stepsTolerance": 0.1}), (na.NmfAlgorithm.HALS, {"stepsTolerance": 0.1}),
                     (na.NmfAlgorithm.NeNMF, {"stepsTolerance": 1.0}), (na.NmfAlgorithm.NeNMF, {"stepsTolerance": -0.5}),
                     (na.NmfAlgorithm.NeNMF, {"stepsTolerance": float("nan")}), (na.NmfAlgorithm.NeNMF, {"stepsTolerance": float("inf")})):
        assert na.compute(V, W.copy(order="F"), H.copy(order="F"), algorithm=alg, iterations=3, parameters=prm) == bad, (alg, prm)
    assert na.compute(V, W.copy(order="F"), H.copy(order="F"), algorithm=na.NmfAlgorithm.Multiplicative, iterations=3,
                      parameters={"stepsTolerance": 0.0}) == na.ResultType.Success
