"""Per-column dynamic stopping of the HALS inner sweeps on the GPU, engine level (docs/HALS.md, "Dynamic stopping"): Engine(..., "hals", sweep_tolerance=),
Engine.set_sweep_tolerance, Engine.sweep_counts and the "sweepsTolerance" Parameter, against tests/hals_dyn_reference.py.

As at kernel level (tests/test_gpu_hals_dyn_sweep.py) values and rule are checked separately: the restatement is fed the ENGINE's counts and must give the
engine's factors and error -- fp64 within 1e-9, fp32 within 2e-4 for the factors and 1e-5 for the error, the standing figures of tests/test_gpu_hals.py -- and
the engine's counts must equal the restatement's own for at least 98 % of the columns of H and of the rows of W (tests/test_hals_dyn_cpu.py: numpy fp32 stays
within that cap on these inputs).
"""
import numpy as np
import pytest

import nmfgpu_amd as na
from tests import hals_dyn_cases as dc
from tests import hals_dyn_reference as dyn
from tests import hals_multi_cases as mc
from tests import hals_penalty_reference as pen

pytestmark = pytest.mark.gpu

SHAPES = [pytest.param(m, n, r, dtype, id=f"{m}x{n}-r{r}-{np.dtype(dtype).name}") for (m, n, r) in dc.ENGINE_SHAPES for dtype in (np.float32, np.float64)]
NONE = (0.0, 0.0, 0.0, 0.0)


@pytest.fixture(scope="module", autouse=True)
def _library_is_native():
    assert na.device_count() >= 1, "GPU tests need a HIP device"
    assert na.initialize() in (na.ResultType.Success, na.ResultType.ErrorAlreadyInitialized)
    na.set_verbosity(na.Verbosity.Nothing)
    yield
    na.finalize()


def kw(p):
    return dict(l1_w=p[0], l1_h=p[1], l2_w=p[2], l2_h=p[3])


def engine(V, W, H, **k):
    m, n = V.shape
    eng = na.Engine(m, n, W.shape[1], "hals", dtype=V.dtype, **k)
    eng.upload(V)
    eng.set_factors(W, H)
    return eng


@pytest.mark.parametrize("m,n,r,dtype", SHAPES)
def test_tolerance_zero_is_the_static_engine(m, n, r, dtype):
    """set_sweep_tolerance(0) at sweeps (4, 4): the factors and errors of an engine that never saw the setter, bit for bit, over 5 iterations; the counts are 4."""
    V, W, H = dc.engine_problem(m, n, r, dtype)
    out = []
    for give in (False, True):
        eng = engine(V, W, H, sweeps_h=4, sweeps_w=4)
        if give:
            eng.set_sweep_tolerance(0.25)
            eng.set_sweep_tolerance(0)
        errs = []
        for it in range(1, 6):
            eng.iterate(1, first_iteration=it, error_every=1)
            errs.append(eng.frobenius)
        out.append((*eng.get_factors(), errs))
        assert (eng.sweep_counts(0) == 4).all() and eng.sweep_counts(0).shape == (n,) and eng.sweep_counts(0).dtype == np.int32
        assert (eng.sweep_counts(1) == 4).all() and eng.sweep_counts(1).shape == (m,)
        eng.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]


@pytest.mark.parametrize("penalised", [False, True])
@pytest.mark.parametrize("m,n,r,dtype", SHAPES)
def test_one_iteration_against_the_restatement(m, n, r, dtype, penalised):
    p = dc.ENGINE_PENALTIES if penalised else NONE
    tol_f, tol_e = (2e-4, 1e-5) if dtype == np.float32 else (1e-9, 1e-9)
    V, W, H = dc.engine_problem(m, n, r, dtype)
    eng = engine(V, W, H, sweeps_h=dc.ENGINE_SWEEPS, sweeps_w=dc.ENGINE_SWEEPS, sweep_tolerance=dc.ENGINE_TOL, **kw(p))
    eng.iterate(1, error_every=1)
    Wg, Hg = eng.get_factors()
    ch, cw = eng.sweep_counts(0), eng.sweep_counts(1)
    reported = eng.frobenius
    eng.close()
    assert ch.shape == (n,) and cw.shape == (m,)
    assert ch.min() >= 1 and ch.max() <= dc.ENGINE_SWEEPS and cw.min() >= 1 and cw.max() <= dc.ENGINE_SWEEPS
    # values: the restatement at the engine's counts
    W64, H64, err, _, _ = dyn.iteration(V, W, H, dc.ENGINE_SWEEPS, dc.ENGINE_SWEEPS, dc.ENGINE_TOL, p, forced_h=ch, forced_w=cw)
    print("rel W", mc.rel(Wg, W64), "rel H", mc.rel(Hg, H64), "error", reported, err)
    assert mc.rel(Wg, W64) < tol_f and mc.rel(Hg, H64) < tol_f, (mc.rel(Wg, W64), mc.rel(Hg, H64))
    assert abs(reported - err) <= tol_e * err, (reported, err)
    # the rule: the restatement's own counts
    _, _, _, ch_own, cw_own = dyn.iteration(V, W, H, dc.ENGINE_SWEEPS, dc.ENGINE_SWEEPS, dc.ENGINE_TOL, p)
    same_h, same_w = float((ch == ch_own).mean()), float((cw == cw_own).mean())
    print("H counts", np.bincount(ch).tolist(), "equal on", same_h, "W counts", np.bincount(cw).tolist(), "equal on", same_w)
    assert len(set(cw.tolist())) > 1, "every row took the same number of sweeps: the case shows nothing"
    assert same_h >= dc.FLIP_CAP and same_w >= dc.FLIP_CAP


@pytest.mark.parametrize("penalised", [False, True])
@pytest.mark.parametrize("m,n,r,dtype", SHAPES)
def test_twenty_iterations_are_monotone_and_no_worse_than_plain(m, n, r, dtype, penalised):
    """delta = 0.1 at sweeps (16, 16) on uniformly random V (a residual large enough for the fp32 trace formula): the reported error -- with penalties the
    penalised objective of tests/test_gpu_hals_penalty.py, from the factors -- does not rise (the slack of tests/test_gpu_hals.py), and ends no higher than that
    of sweeps (1, 1) after as many iterations."""
    slack = 1e-6 if dtype == np.float32 else 1e-12
    p = dc.ENGINE_PENALTIES if penalised else NONE
    V, W, H = mc.problem(m, n, r, dtype, seed=m + n + r)

    def run(**k):
        eng = engine(V, W, H, **kw(p), **k)
        vals = []
        for it in range(1, 21):
            eng.iterate(1, first_iteration=it, error_every=1)
            vals.append(pen.objective(V, *eng.get_factors(), *p) if penalised else eng.frobenius)
        counts = eng.sweep_counts(0)
        eng.close()
        return vals, counts

    vals, counts = run(sweeps_h=16, sweeps_w=16, sweep_tolerance=0.1)
    plain, ones = run()
    print("dynamic", vals[0], vals[-1], "plain", plain[-1], "H counts of the last step", np.bincount(counts).tolist())
    assert (ones == 1).all() and counts.min() >= 1 and counts.max() <= 16
    for a, b in zip(vals, vals[1:]):
        assert b <= a * (1 + slack), (a, b)
    assert vals[-1] <= plain[-1] * (1 + slack), (vals[-1], plain[-1])


@pytest.mark.parametrize("m,n,r,dtype", SHAPES)
def test_constant_w(m, n, r, dtype):
    """constant_w: W stays bit for bit, the H counts are reported, and there are no W counts (no W step has run: sweep_counts(1) raises)."""
    V, W, H = dc.engine_problem(m, n, r, dtype)
    eng = engine(V, W, H, sweeps_h=dc.ENGINE_SWEEPS, sweeps_w=dc.ENGINE_SWEEPS, sweep_tolerance=dc.ENGINE_TOL)
    eng.iterate(2, error_every=0, last_iteration=2, constant_w=True)
    Wg, Hg = eng.get_factors()
    assert np.array_equal(Wg, W)
    ch = eng.sweep_counts(0)
    assert ch.shape == (n,) and ch.min() >= 1 and ch.max() <= dc.ENGINE_SWEEPS
    with pytest.raises(na.EngineError) as info:
        eng.sweep_counts(1)
    assert "counts" in str(info.value)
    assert not np.array_equal(Hg, H)
    eng.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_sparse_compute_formats_are_bit_identical(dtype):
    """Sparse compute uses the same sweep call sites: CSR and CSC uploads at delta = 0.1 give bit-identical factors and counts, with counts that differ."""
    m, n, r = 200, 150, 70
    rng = np.random.default_rng(11)
    rows, cols, vals, _ = pen.sparse_pattern(m, n, 0.1, rng, (3, 150), (0, 77))
    vals = vals.astype(dtype)
    W = mc.F((1.0 - rng.random((m, r))).astype(dtype))
    H = mc.F((1.0 - rng.random((r, n))).astype(dtype))
    out = []
    for fmt in (1, 2):
        eng = na.Engine(m, n, r, "hals", dtype=dtype, sparse_compute=True, sweeps_h=8, sweeps_w=8, sweep_tolerance=0.1)
        if fmt == 1:
            ptr = np.zeros(m + 1, np.int32)
            np.cumsum(np.bincount(rows, minlength=m), out=ptr[1:])
            eng.upload_sparse(1, vals, ptr, cols.astype(np.int32), 0)
        else:
            order = np.lexsort((rows, cols))
            ptr = np.zeros(n + 1, np.int32)
            np.cumsum(np.bincount(cols, minlength=n), out=ptr[1:])
            eng.upload_sparse(2, vals[order], ptr, rows[order].astype(np.int32), 0)
        eng.set_factors(W, H)
        eng.iterate(3, error_every=0, last_iteration=3)
        out.append((*eng.get_factors(), eng.sweep_counts(0), eng.sweep_counts(1), eng.frobenius))
        eng.close()
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)
    assert len(set(out[0][3].tolist())) > 1 and out[0][2].min() >= 1 and out[0][3].max() <= 8


# ------------------------------------------------------------------ refusals

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bad_tolerances_are_refused(dtype):
    for bad in (-0.1, 1.0, 2.0, float("nan"), float("inf")):
        with pytest.raises(na.EngineError) as info:
            na.Engine(60, 50, 8, "hals", dtype=dtype, sweep_tolerance=bad)
        assert info.value.status == 1, bad
    eng = na.Engine(60, 50, 8, "hals", dtype=dtype)
    for bad in (-0.1, -1e-300, 1.0, 2.0, float("nan"), float("inf")):
        with pytest.raises(na.EngineError) as info:
            eng.set_sweep_tolerance(bad)
        assert info.value.status == 1 and "tolerance" in str(info.value), (bad, str(info.value))
    with pytest.raises(na.EngineError):
        eng.sweep_counts(0)                          # (before any step)
    eng.set_sweep_tolerance(0.999)
    eng.set_sweep_tolerance(0.0)
    eng.close()


def test_other_engines_take_only_zero():
    for k in (dict(algorithm="mu"), dict(algorithm="mu", divergence="is"), dict(algorithm="als")):
        eng = na.Engine(60, 50, 8, **k)
        with pytest.raises(na.EngineError) as info:
            eng.set_sweep_tolerance(0.1)
        assert info.value.status == 1 and "tolerance" in str(info.value) and "HALS" in str(info.value), k
        eng.set_sweep_tolerance(0.0)
        with pytest.raises(na.EngineError):
            eng.sweep_counts(0)
        eng.close()
        with pytest.raises(na.EngineError):
            na.Engine(60, 50, 8, sweep_tolerance=0.1, **k)
        na.Engine(60, 50, 8, sweep_tolerance=0.0, **k).close()


def test_compute_takes_the_tolerance():
    V, W, H = mc.planted(300, 257, 20, np.float64, seed=7)
    bad = na.ResultType.ErrorInvalidArgument
    for alg, prm in ((na.NmfAlgorithm.Multiplicative, {"sweepsTolerance": 0.1}), (na.NmfAlgorithm.HALS, {"sweepsTolerance": 1.0}),
                     (na.NmfAlgorithm.HALS, {"sweepsTolerance": -0.5}), (na.NmfAlgorithm.HALS, {"sweepsTolerance": float("nan")})):
        assert na.compute(V, W.copy(order="F"), H.copy(order="F"), algorithm=alg, iterations=3, parameters=prm) == bad, (alg, prm)
    assert na.compute(V, W.copy(order="F"), H.copy(order="F"), algorithm=na.NmfAlgorithm.Multiplicative, iterations=3,
                      parameters={"sweepsTolerance": 0.0}) == na.ResultType.Success
    errs = []
    for prm in ({}, {"sweepsTolerance": 0.1, "sweepsH": 8}):
        s = na.Summary()
        Wc, Hc = W.copy(order="F"), H.copy(order="F")
        assert na.compute(V, Wc, Hc, algorithm=na.NmfAlgorithm.HALS, iterations=10, parameters=prm, summary=s) == na.ResultType.Success
        errs.append(s.record(0).frobenius)
    print("error after 10 iterations: (1, 1)", errs[0], "sweepsH = 8 at delta = 0.1", errs[1])
    assert errs[1] < errs[0]
    # ... and it is the restatement's run (sweepsW stays 1)
    W64, H64 = W.astype(np.float64), H.astype(np.float64)
    for _ in range(10):
        W64, H64, err, _, _ = dyn.iteration(V, W64, H64, 8, 1, 0.1)
    assert abs(errs[1] - err) <= 1e-9 * err, (errs[1], err)
