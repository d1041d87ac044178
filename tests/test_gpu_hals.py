"""HALS (coordinate descent, kernels_hals.hip) on the GPU against the fp64 restatement of tests/hals_reference.py.

Tolerances: factors after 1 and 20 iterations within 2e-4 relative (fp32: split-operand and native fp32 MFMA products) and 1e-9 (fp64); the reported
error within 1e-5 / 1e-9 relative.  The sweep kernel forms G(k, :) . h as lane partials summed by a butterfly, the restatement as one dot product:
the two differ in rounding only.
"""
import numpy as np
import pytest

import nmfgpu_amd as na
from tests import hals_reference as ref

pytestmark = pytest.mark.gpu


def F(a):
    return np.asfortranarray(a)


def problem(m, n, r, dtype, seed=1):
    rng = np.random.default_rng(seed)
    V = F(rng.random((m, n)).astype(dtype))
    W = F((1.0 - rng.random((m, r))).astype(dtype))
    H = F((1.0 - rng.random((r, n))).astype(dtype))
    return V, W, H


def planted(m, n, r, dtype, seed=1):
    """V = W0 H0 + 0.01 noise: a rank-r structure under small non-negative noise.  On uniformly random V (or under heavy noise) the fp32 trajectories of
    HALS leave the fp64 one at a rate set by the problem, not by the kernels: at 1 000 x 777, r = 450, 5e-8 after one iteration and 1.6e-2 after twenty,
    and two fp32 product forms differ by as much from each other.  Its small residual in turn limits the trace formula of the reported error in fp32
    (relative error ~ eps (||V|| / error)^2): the reported error is checked on uniformly random V, where the residual is large."""
    rng = np.random.default_rng(seed)
    V = F((rng.random((m, r)) @ rng.random((r, n)) + 0.01 * rng.random((m, n))).astype(dtype))
    W = F((1.0 - rng.random((m, r))).astype(dtype))
    H = F((1.0 - rng.random((r, n))).astype(dtype))
    return V, W, H


def rel(a, b):
    return np.linalg.norm(a.astype(np.float64) - b.astype(np.float64)) / max(np.linalg.norm(b.astype(np.float64)), 1e-300)


@pytest.fixture(scope="module", autouse=True)
def _library_is_native():
    assert na.device_count() >= 1, "GPU tests need a HIP device"
    assert na.initialize() in (na.ResultType.Success, na.ResultType.ErrorAlreadyInitialized)
    na.set_verbosity(na.Verbosity.Nothing)
    yield
    na.finalize()


def engine(V, W, H, **kw):
    m, n = V.shape
    eng = na.Engine(m, n, W.shape[1], "hals", dtype=V.dtype, **kw)
    eng.upload(V)
    eng.set_factors(W, H)
    return eng


def check_padding(eng):
    """The padded panels hold exact zeros outside the m x r / r x n blocks."""
    g = eng.geometry()
    RP, mp, np_ = g["padded_rank"], g["padded_m"], g["padded_n"]
    Wt = eng.debug_read(0, RP * mp).reshape(mp, RP)
    Hp = eng.debug_read(1, RP * np_).reshape(np_, RP)
    assert (Wt[:, eng.r:] == 0).all() and (Wt[eng.m:, :] == 0).all()
    assert (Hp[:, eng.r:] == 0).all() and (Hp[eng.n:, :] == 0).all()


PARITY = [
    # (m, n, r, dtype)
    (500, 300, 7, np.float32), (500, 300, 33, np.float32), (1000, 777, 64, np.float32), (1000, 777, 100, np.float32),
    (1000, 777, 200, np.float32), (1000, 777, 450, np.float32),
    (500, 300, 7, np.float64), (1000, 777, 64, np.float64), (1000, 777, 100, np.float64), (1000, 777, 150, np.float64),
    (1000, 777, 450, np.float64),
    (40000, 300, 64, np.float32),
    # the sweep instantiations no case above reaches: fp32 RP 384, fp64 RP 256, 320, 384, 512
    (1000, 777, 300, np.float32),
    (600, 500, 200, np.float64), (600, 500, 300, np.float64), (600, 500, 350, np.float64), (1000, 777, 500, np.float64),
]


def run_both(eng, V, W, H, check):
    """1 and 20 iterations on the engine and in the restatement; check(iterations, (Wg, Hg), (W64, H64), reported, restated error)"""
    V64, W64, H64 = V.astype(np.float64), W.astype(np.float64), H.astype(np.float64)
    done = 0
    for iters in (1, 20):
        W64, H64, errs = ref.run(V64, W64, H64, iters - done)
        eng.iterate(iters - done, first_iteration=done + 1, error_every=0, last_iteration=iters)
        done = iters
        check(iters, eng.get_factors(), (W64, H64), eng.frobenius, errs[-1])


@pytest.mark.parametrize("m,n,r,dtype", PARITY)
def test_parity_with_restatement(m, n, r, dtype):
    tol_f, tol_e = (2e-4, 1e-5) if dtype == np.float32 else (1e-9, 1e-9)

    def factors(iters, got, want, reported, restated):
        assert rel(got[0], want[0]) < tol_f, (iters, rel(got[0], want[0]))
        assert rel(got[1], want[1]) < tol_f, (iters, rel(got[1], want[1]))

    def error(iters, got, want, reported, restated):
        # (fp32 at r = 450 on random V: after 20 iterations the trajectory itself has moved -- factors 1.6e-2, error 2.7e-4 from the fp64 one)
        if iters == 1 or dtype == np.float64 or r <= 200:
            assert abs(reported - restated) <= tol_e * restated, (iters, reported, restated)
        if iters == 1:
            factors(iters, got, want, reported, restated)

    V, W, H = planted(m, n, r, dtype, seed=m + n + r)
    eng = engine(V, W, H)
    assert eng.geometry()["fused_launches"] == 0
    run_both(eng, V, W, H, factors)
    check_padding(eng)
    eng.close()
    V, W, H = problem(m, n, r, dtype, seed=m + n + r)
    eng = engine(V, W, H)
    run_both(eng, V, W, H, error)
    eng.close()


def test_parity_native_fp32_products():
    V, W, H = planted(1000, 777, 64, np.float32, seed=4)
    eng = engine(V, W, H, precision="fp32_mfma")
    W64, H64, errs = ref.run(V.astype(np.float64), W, H, 20)
    eng.iterate(20, error_every=0, last_iteration=20)
    Wg, Hg = eng.get_factors()
    assert rel(Wg, W64) < 2e-4 and rel(Hg, H64) < 2e-4, (rel(Wg, W64), rel(Hg, H64))
    assert abs(eng.frobenius - errs[-1]) <= 1e-5 * errs[-1]
    eng.close()


@pytest.mark.parametrize("dtype,slack", [(np.float32, 1e-6), (np.float64, 1e-12)])
def test_objective_is_monotone(dtype, slack):
    V, W, H = problem(600, 400, 16, dtype, seed=9)
    eng = engine(V, W, H)
    errs = []
    for it in range(1, 301):
        eng.iterate(1, first_iteration=it, error_every=1)
        errs.append(eng.frobenius)
    for a, b in zip(errs, errs[1:]):
        assert b <= a * (1 + slack), (a, b)
    assert errs[-1] < errs[0]
    eng.close()


def test_converges_faster_than_mu_on_a_planted_problem():
    rng = np.random.default_rng(21)
    m, n, r = 2000, 1500, 20
    V = F((rng.random((m, r)) @ rng.random((r, n)) + 0.01 * rng.random((m, n))).astype(np.float32))
    W, H = F(rng.random((m, r)).astype(np.float32)), F(rng.random((r, n)).astype(np.float32))
    out = {}
    for alg in ("hals", "mu"):
        eng = na.Engine(m, n, r, alg)
        eng.upload(V)
        eng.set_factors(W, H)
        eng.iterate(100, error_every=0, last_iteration=100)
        out[alg] = eng.frobenius
        eng.close()
    assert out["hals"] < out["mu"], out


def test_constant_w_projects_onto_the_basis():
    V, W, H = problem(700, 500, 24, np.float32, seed=13)
    eng = engine(V, W, H)
    eng.iterate(10, error_every=5, constant_w=True)
    Wg, Hg = eng.get_factors()
    assert np.array_equal(Wg, W)                            # neither updated nor normalised
    _, H64, errs = ref.run(V.astype(np.float64), W, H, 10, constant_w=True)
    assert rel(Hg, H64) < 2e-4, rel(Hg, H64)
    assert abs(eng.frobenius - errs[-1]) <= 1e-5 * errs[-1]
    eng.close()


def test_bf16_products_run_and_descend():
    V, W, H = problem(1000, 777, 64, np.float32, seed=17)
    eng = engine(V, W, H, precision="bf16")
    eng.iterate(1, error_every=1)
    e1 = eng.frobenius
    eng.iterate(20, first_iteration=2, error_every=0, last_iteration=21)
    assert eng.frobenius < e1
    check_padding(eng)
    eng.close()


def test_force_valu_agrees_with_mfma(monkeypatch):
    # (the VALU product sums in one fp32 chain per element, the split-operand one is fp32-accurate, and HALS carries every rounding difference forward:
    #  7.7e-5 apart after 20 iterations on this problem, where the split-operand form is within 1.5e-5 of the fp64 restatement)
    V, W, H = planted(1000, 777, 64, np.float32, seed=19)
    eng = engine(V, W, H)
    eng.iterate(20, error_every=0, last_iteration=20)
    Wm, Hm = eng.get_factors()
    eng.close()
    monkeypatch.setenv("NMFAMD_FORCE_VALU", "1")
    eng = engine(V, W, H)
    assert eng.geometry()["product_kernel"] == 4
    eng.iterate(20, error_every=0, last_iteration=20)
    Wv, Hv = eng.get_factors()
    eng.close()
    assert rel(Wv, Wm) < 2e-4 and rel(Hv, Hm) < 2e-4, (rel(Wv, Wm), rel(Hv, Hm))


def test_three_phase_api_refuses_hals():
    import torch
    V, W, H = problem(300, 200, 16, np.float32)
    eng = engine(V, W, H)
    assert eng.geometry()["fused_launches"] == 0
    ex = torch.zeros(eng.geometry()["exchange_count"], dtype=torch.float32, device="cuda")
    for call in (lambda: eng.h_step(False), lambda: eng.w_products(ex.data_ptr()), lambda: eng.w_finish(ex.data_ptr(), False)):
        with pytest.raises(na.EngineError) as info:
            call()
        assert info.value.status == 1
    eng.close()


# ------------------------------------------------------------------ through nmfgpu::compute

def test_compute_copy_existing():
    V, W, H = problem(800, 600, 12, np.float32, seed=23)
    W64, H64, errs = ref.run(V.astype(np.float64), W, H, 30)
    s = na.Summary()
    res = na.compute(V, W, H, algorithm=na.NmfAlgorithm.HALS, iterations=30, summary=s)
    assert res == na.ResultType.Success, res
    assert rel(W, W64) < 2e-4 and rel(H, H64) < 2e-4, (rel(W, W64), rel(H, H64))
    rec = s.record(0)
    assert abs(rec.frobenius - errs[-1]) <= 1e-5 * errs[-1], (rec.frobenius, errs[-1])
    assert rec.numIterations == 30


def test_compute_random_two_runs_keeps_the_best():
    V, W, H = problem(800, 600, 12, np.float32, seed=29)
    best = {}
    for runs in (1, 2):
        s = na.Summary()
        res = na.compute(V, W, H, algorithm=na.NmfAlgorithm.HALS, init=na.NmfInitializationMethod.AllRandomValues, iterations=40, runs=runs, seed=5, summary=s)
        assert res == na.ResultType.Success, res
        assert 1 <= s.record_count() <= runs                # (a run is recorded when it improves on the ones before it)
        best[runs] = s.record(s.best_run()).frobenius
        assert best[runs] == min(s.record(i).frobenius for i in range(s.record_count()))
        # the factors handed back are those of the best run: the W step after its last error evaluation can only lower the error
        got = np.linalg.norm(V.astype(np.float64) - W.astype(np.float64) @ H.astype(np.float64))
        assert got <= best[runs] * (1 + 1e-5)
    assert best[2] <= best[1]                               # run 1 of the two-run call is the one-run call


def test_compute_threshold_stops_early():
    V, W, H = problem(800, 600, 12, np.float32, seed=31)
    s = na.Summary()
    res = na.compute(V, W, H, algorithm=na.NmfAlgorithm.HALS, iterations=2000, threshold=1e-2, summary=s)
    assert res == na.ResultType.Success, res
    rec = s.record(0)
    assert rec.numIterations < 2000
    # the reported error is that of the last H step; the W step after it can only lower it
    got = np.linalg.norm(V.astype(np.float64) - W.astype(np.float64) @ H.astype(np.float64))
    assert rec.frobenius > 0 and got <= rec.frobenius * (1 + 1e-5) and got > 0.99 * rec.frobenius


def test_compute_progress_line_names_hals(capfd):
    V, W, H = problem(300, 200, 8, np.float32)
    na.set_verbosity(na.Verbosity.Summary)
    try:
        res = na.compute(V, W, H, algorithm=na.NmfAlgorithm.HALS, iterations=10)
    finally:
        na.set_verbosity(na.Verbosity.Nothing)
    assert res == na.ResultType.Success
    assert "'HALS'" in capfd.readouterr().out


@pytest.mark.parametrize("params", [{"numGpus": 2}, {"divergence": 1}])
def test_compute_refusals(params):
    V, W, H = problem(300, 200, 8, np.float32)
    res = na.compute(V, W, H, algorithm=na.NmfAlgorithm.HALS, iterations=10, parameters=params)
    assert res == na.ResultType.ErrorInvalidArgument


# ------------------------------------------------------------------ one step from a drifted state

def per_column(got, want, tol, what):
    """Every column within tol relative, with an absolute floor of 1 % of the RMS column norm (clamped columns near zero); a wrong tile or row block
    is off by O(1)."""
    got, want = got.astype(np.float64), want.astype(np.float64)
    floor = 1e-2 * np.linalg.norm(want) / np.sqrt(want.shape[1])
    err = np.linalg.norm(got - want, axis=0)
    lim = tol * np.maximum(np.linalg.norm(want, axis=0), floor)
    assert (err <= lim).all(), (what, int(np.argmax(err / lim)), float((err / lim).max()))


@pytest.mark.parametrize("m,n,r,dtype", [(1000, 777, 450, np.float32), (1000, 777, 300, np.float32), (1000, 777, 500, np.float64)])
def test_one_step_from_a_drifted_state(m, n, r, dtype):
    """After 20 iterations on random V (where fp32 trajectories drift apart), one engine iteration and one fp64 restatement iteration from the
    same downloaded state: per column of W and H 1e-3 (fp32; 5e-8 in the global norm was measured) or 1e-9 (fp64), the global norms at 2e-4 /
    1e-9, and the reported error at 1e-5 / 1e-9 -- the check the 20-iteration fp32 test at r = 450 has to skip."""
    tol_c, tol_f, tol_e = (1e-3, 2e-4, 1e-5) if dtype == np.float32 else (1e-9, 1e-9, 1e-9)
    V, W, H = problem(m, n, r, dtype, seed=m + n + r + 1)
    eng = engine(V, W, H)
    eng.iterate(20, error_every=0, last_iteration=20)
    W0, H0 = eng.get_factors()
    eng.iterate(1, first_iteration=21, error_every=0, last_iteration=21)
    Wg, Hg = eng.get_factors()
    reported = eng.frobenius
    W64, H64, err = ref.iteration(V, W0, H0)
    check_padding(eng)
    eng.close()
    per_column(Wg, W64, tol_c, "W")
    per_column(Hg, H64, tol_c, "H")
    assert rel(Wg, W64) < tol_f and rel(Hg, H64) < tol_f, (rel(Wg, W64), rel(Hg, H64))
    assert abs(reported - err) <= tol_e * err, (reported, err)


# ------------------------------------------------------------------ ragged shapes at every rank boundary

def _ragged_cases():
    out = []
    for dtype, rps in ((np.float32, [64, 128, 256, 384, 512]), (np.float64, [64, 128, 192, 256, 320, 384, 448, 512])):
        rs = [1] + [q for RP in rps[:-1] for q in (RP, RP + 1)] + [512]
        for seed in range(24):
            rng = np.random.default_rng(1000 * (dtype == np.float64) + seed)
            r = rs[seed % len(rs)] if seed < len(rs) else int(rng.choice(rs))
            pick = lambda: int(rng.choice([1, 2, 127, 128, 129, int(rng.integers(3, 300)), r + int(rng.integers(0, 40))]))
            m, n = pick(), pick()
            out.append(pytest.param(m, n, r, dtype, seed, id=f"{np.dtype(dtype).name}-{m}x{n}-r{r}-s{seed}"))
    return out


@pytest.mark.parametrize("m,n,r,dtype,seed", _ragged_cases())
def test_seeded_ragged_sweep(m, n, r, dtype, seed):
    """m, n in {1, 2, 127, 128, 129, ...}, often below r, with r on both sides of every padded-rank boundary: fp64 3 iterations at 1e-9; fp32 one
    iteration at 2e-4.  The padding stays exactly 0 throughout.
    Where m or n is below r, G (or H H^T) is singular: once a sweep has brought the residual to rounding level, later steps divide that noise by
    diagonal entries that can be tiny (n = 1: H H^T(k, k) = h_k^2), and the result is set by rounding, in fp64 too (2 x 127 at r = 193: a numpy
    restatement with the dot products over reversed coordinates lands 0.59 away from the forward one in W).  There each bound is the larger
    of the one above and 10 x the distance of such a restatement (ref.iteration_in, in the engine's dtype, reversed order) from the fp64 one:
    derived from the problem, never from GPU output."""
    V, W, H = problem(m, n, r, dtype, seed=seed)
    eng = engine(V, W, H)
    iters = 3 if dtype == np.float64 else 1
    eng.iterate(iters, error_every=0, last_iteration=iters)
    Wg, Hg = eng.get_factors()
    check_padding(eng)
    eng.close()
    W64, H64, _ = ref.run(V, W, H, iters)
    tol_w = tol_h = 1e-9 if dtype == np.float64 else 2e-4
    if min(m, n) < r:
        Wx, Hx = W, H
        for _ in range(iters):
            Wx, Hx = ref.iteration_in(V, Wx, Hx, dtype, reverse=True)
        tol_w, tol_h = max(tol_w, 10 * rel(Wx, W64)), max(tol_h, 10 * rel(Hx, H64))
    assert rel(Wg, W64) < tol_w and rel(Hg, H64) < tol_h, (rel(Wg, W64), tol_w, rel(Hg, H64), tol_h)


# ------------------------------------------------------------------ degenerate columns

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_zero_column_and_row_stay_zero(dtype):
    """W(:, k) = 0 with H(k, :) = 0: G(k, k) = 0 skips row k of H, H H^T(k, k) = 0 skips column k of W, and the d = 0 guard leaves it: exact zeros."""
    tol = 2e-4 if dtype == np.float32 else 1e-9
    V, W, H = problem(300, 200, 12, dtype, seed=41)
    W[:, 5] = 0.0
    H[5, :] = 0.0
    eng = engine(V, W, H)
    eng.iterate(3, error_every=0, last_iteration=3)
    Wg, Hg = eng.get_factors()
    check_padding(eng)
    eng.close()
    assert (Wg[:, 5] == 0).all() and (Hg[5, :] == 0).all()
    W64, H64, _ = ref.run(V, W, H, 3)
    assert rel(Wg, W64) < tol and rel(Hg, H64) < tol, (rel(Wg, W64), rel(Hg, H64))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_zero_column_alone(dtype):
    """W(:, k) = 0 alone: row k of H is skipped in the H step (it keeps its values), then column k of W is updated from them."""
    tol = 2e-4 if dtype == np.float32 else 1e-9
    V, W, H = problem(300, 200, 12, dtype, seed=43)
    W[:, 7] = 0.0
    eng = engine(V, W, H)
    eng.iterate(1, error_every=0, last_iteration=1)
    Wg, Hg = eng.get_factors()
    check_padding(eng)
    eng.close()
    W64, H64, _ = ref.run(V, W, H, 1)
    assert np.abs(W64[:, 7]).max() > 0                      # (the restatement updates it: the case is not vacuous)
    assert rel(Wg, W64) < tol and rel(Hg, H64) < tol, (rel(Wg, W64), rel(Hg, H64))


# ------------------------------------------------------------------ padding after every product mode

@pytest.mark.parametrize("dtype,precision,valu", [
    (np.float32, "native", False), (np.float32, "fp32_mfma", False), (np.float32, "bf16", False), (np.float32, "native", True),
    (np.float64, "native", False), (np.float64, "native", True)])
def test_padding_after_every_product_mode(dtype, precision, valu, monkeypatch):
    """Ragged m and n (mpad 384 != npad 256): every product mode leaves the padded panels exactly 0 after the sweep and the normalisation."""
    if valu:
        monkeypatch.setenv("NMFAMD_FORCE_VALU", "1")
    V, W, H = problem(301, 130, 20, dtype, seed=47)
    eng = engine(V, W, H, precision=precision)
    g = eng.geometry()
    assert g["padded_m"] != g["padded_n"]
    if valu:
        assert g["product_kernel"] == 4
    eng.iterate(3, error_every=1)
    check_padding(eng)
    Wg, Hg = eng.get_factors()
    eng.close()
    assert np.isfinite(Wg).all() and np.isfinite(Hg).all() and np.isfinite(eng.frobenius)


# ------------------------------------------------------------------ through nmfgpu::compute in double, and the rank limit

def test_compute_copy_existing_double():
    V, W, H = problem(800, 600, 12, np.float64, seed=23)
    W64, H64, errs = ref.run(V, W, H, 30)
    s = na.Summary()
    res = na.compute(V, W, H, algorithm=na.NmfAlgorithm.HALS, iterations=30, summary=s)
    assert res == na.ResultType.Success, res
    assert rel(W, W64) < 1e-9 and rel(H, H64) < 1e-9, (rel(W, W64), rel(H, H64))
    rec = s.record(0)
    assert abs(rec.frobenius - errs[-1]) <= 1e-9 * errs[-1], (rec.frobenius, errs[-1])
    assert rec.numIterations == 30


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_rank_513_is_refused(dtype):
    V, W, H = problem(600, 600, 513, dtype)
    with pytest.raises(na.EngineError) as info:
        na.Engine(600, 600, 513, "hals", dtype=dtype)
    assert info.value.status == 1
    res = na.compute(V, W, H, algorithm=na.NmfAlgorithm.HALS, iterations=2)
    assert res != na.ResultType.Success, res
