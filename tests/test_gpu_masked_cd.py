"""Missing-value coordinate descent on the GPU (docs/MISSING.md, "Coordinate descent"): an engine with missing_solver="cd" against the fp64 restatement
(tests/masked_cd_reference.py) -- factors, reported error, constant W, padding, every input form, the multiplicative update it replaces and returns to, predict /
score / top_k, nmfgpu::compute with Parameter "missingSolver", and the refusals of the setter.

Tolerances: fp64 hals_multi_cases.TOL_F64; fp32 hals_multi_cases.MARGIN times the distance between the float32 and the fp64 restatement on the same case and
iteration count, computed here on the CPU (never from the engine's output); the reported error as tests/test_gpu_hals_multi.py holds it."""
import numpy as np
import pytest

import nmfgpu_amd as na
from nmfgpu_amd import api
from tests import hals_multi_cases as hm
from tests import masked_cd_reference as cd
from tests import masked_reference as mref
from tests import topk_reference as tref

pytestmark = pytest.mark.gpu

SHAPES = [(90, 70, 6), (150, 120, 70)]
DTYPES = [np.float32, np.float64]
SWEEPS = [(1, 1), (3, 2)]
PENALTIES = [(0.0, 0.0, 0.0, 0.0), (0.05, 0.05, 0.01, 0.01)]      # (l1W, l1H, l2W, l2H)
SNAPSHOTS = (1, 2, 5)
ERR_TOL = {np.float32: 1e-5, np.float64: 1e-9}
MU_TOL = {np.float32: (2e-4, 1e-5), np.float64: (1e-9, 1e-9)}       # tests/test_gpu_masked.py's: factors, error
EMPTY_ROW, EMPTY_COL = 3, 5


def F(a):
    return np.asfortranarray(a)


_PROBLEMS, _REFS = {}, {}


def problem(shape, dtype):
    """(rows, cols, vals, W0, H0): planted ratings at 30 % of the entries without row EMPTY_ROW and column EMPTY_COL, a positive start rounded to dtype."""
    key = (shape, np.dtype(dtype).name)
    if key not in _PROBLEMS:
        m, n, r = shape
        rows, cols, vals = mref.planted_ratings(m, n, 0.3, seed=m + r)
        keep = (rows != EMPTY_ROW) & (cols != EMPTY_COL)
        W0, H0 = cd.start(m, n, r, m + n)
        out = (rows[keep], cols[keep], vals[keep], F(W0.astype(dtype)), F(H0.astype(dtype)))
        for a in out:
            a.setflags(write=False)
        _PROBLEMS[key] = out
    return _PROBLEMS[key]


def restated(shape, dtype, sweeps, penalties, iters=max(SNAPSHOTS), const_w=False):
    """{iteration: (W, H)} at SNAPSHOTS and [error per iteration] of the fp64 restatement from the dtype-rounded start (cached, never written)."""
    key = (shape, np.dtype(dtype).name, sweeps, penalties, iters, const_w)
    if key not in _REFS:
        rows, cols, vals, W0, H0 = problem(shape, dtype)
        imgs = cd.images(rows, cols, vals, shape[0], shape[1])
        W, H = W0.astype(np.float64), H0.astype(np.float64)
        snaps, errs = {}, []
        for it in range(1, iters + 1):
            W, H, f = cd.iteration(rows, cols, vals, W, H, sweeps[0], sweeps[1], penalties, const_w, imgs)
            errs.append(f)
            if it in SNAPSHOTS or it == iters:
                snaps[it] = (W.copy(), H.copy())
        _REFS[key] = (snaps, errs)
    return _REFS[key]


def fp32_figures(shape, sweeps, penalties):
    """{iteration: (distance of W, distance of H)} between the float32 and the fp64 restatement at SNAPSHOTS."""
    rows, cols, vals, W0, H0 = problem(shape, np.float32)
    snaps, _ = restated(shape, np.float32, sweeps, penalties)
    m, n, r = shape
    csr, csc = cd.images(rows, cols, vals, m, n)
    W, H = np.array(W0, dtype=np.float32), np.array(H0, dtype=np.float32)
    l1W, l1H, l2W, l2H = penalties
    out = {}
    for it in range(1, max(SNAPSHOTS) + 1):
        Ht = cd.half_step_in(*csc, H.T, W, r, n, sweeps[0], l1H, l2H)
        H = np.ascontiguousarray(Ht.T)
        W = cd.half_step_in(*csr, W, Ht, r, m, sweeps[1], l1W, l2W)
        if it in SNAPSHOTS:
            out[it] = (hm.rel(W, snaps[it][0]), hm.rel(H, snaps[it][1]))
    return out


def cd_engine(shape, dtype, sweeps=(1, 1), penalties=(0.0, 0.0, 0.0, 0.0)):
    m, n, r = shape
    l1W, l1H, l2W, l2H = penalties
    return na.Engine(m, n, r, "mu", dtype=dtype, missing_values=True, missing_solver="cd", missing_sweeps_h=sweeps[0], missing_sweeps_w=sweeps[1],
                     l1_w=l1W, l1_h=l1H, l2_w=l2W, l2_h=l2H)


def upload_csr(eng, rows, cols, vals, m):
    ptr, idx, v = mref.csr_of(rows, cols, vals, m)
    eng.upload_sparse(1, v.astype(eng.dtype), ptr, idx, 0)


def run(eng, W0, H0, iters, constant_w=False):
    eng.set_factors(W0, H0)
    eng.iterate(iters, first_iteration=1, error_every=0, last_iteration=iters, constant_w=constant_w)
    W, H = eng.get_factors()
    return W, H, eng.frobenius, eng.rmsd


@pytest.fixture(scope="module")
def ctx():
    assert na.initialize() in (na.ResultType.Success, na.ResultType.ErrorAlreadyInitialized)
    na.set_verbosity(na.Verbosity.Nothing)
    yield
    na.finalize()


def ident(v):
    if isinstance(v, type):
        return np.dtype(v).name
    return "x".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("penalties", PENALTIES, ids=["plain", "pen"])
@pytest.mark.parametrize("sweeps", SWEEPS, ids=ident)
@pytest.mark.parametrize("dtype", DTYPES, ids=ident)
@pytest.mark.parametrize("shape", SHAPES, ids=ident)
def test_parity_error_and_padding(shape, dtype, sweeps, penalties):
    """Factors after 1, 2 and 5 iterations, frobenius and rmsd of every iteration, non-negativity, the empty row and column, exact zeros in the padding."""
    m, n, r = shape
    rows, cols, vals, W0, H0 = problem(shape, dtype)
    snaps, errs = restated(shape, dtype, sweeps, penalties)
    figures = fp32_figures(shape, sweeps, penalties) if dtype == np.float32 else None
    eng = cd_engine(shape, dtype, sweeps, penalties)
    rp = eng.geometry()["padded_rank"]
    assert rp == (64 if r <= 64 else 128)
    upload_csr(eng, rows, cols, vals, m)
    eng.set_factors(W0, H0)
    for it in range(1, max(SNAPSHOTS) + 1):
        eng.iterate(1, first_iteration=it, error_every=1)
        f, q = eng.frobenius, eng.rmsd
        assert f == pytest.approx(errs[it - 1], rel=ERR_TOL[dtype]), (it, f, errs[it - 1])
        assert q == pytest.approx(errs[it - 1] / np.sqrt(len(vals)), rel=ERR_TOL[dtype])
        if it not in SNAPSHOTS:
            continue
        W, H = eng.get_factors()
        tw, th = (hm.TOL_F64, hm.TOL_F64) if dtype == np.float64 else (hm.MARGIN * figures[it][0], hm.MARGIN * figures[it][1])
        dw, dh = hm.rel(W, snaps[it][0]), hm.rel(H, snaps[it][1])
        print(f"{ident(shape)} {np.dtype(dtype).name} sweeps {sweeps} pen {penalties[0] != 0} it {it}: W {dw:.2e} (tol {tw:.2e}) H {dh:.2e} (tol {th:.2e})")
        assert np.all(np.isfinite(W)) and np.all(np.isfinite(H))
        assert dw <= tw and dh <= th, (it, dw, tw, dh, th)
        assert np.all(W >= 0) and np.all(H >= 0)
        assert np.all(W[EMPTY_ROW] == 0) and np.all(H[:, EMPTY_COL] == 0)
        Hp = eng.debug_read(1, rp * n).reshape(n, rp)
        Wp = eng.debug_read(0, rp * m).reshape(m, rp)
        assert np.all(Hp[:, r:] == 0) and np.all(Wp[:, r:] == 0)
        assert np.array_equal(Hp[:, :r].T, H) and np.array_equal(Wp[:, :r], W)
    eng.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=ident)
@pytest.mark.parametrize("shape", SHAPES, ids=ident)
def test_constant_w(shape, dtype):
    m, n, r = shape
    rows, cols, vals, W0, H0 = problem(shape, dtype)
    sweeps, penalties = (3, 2), PENALTIES[1]
    snaps, errs = restated(shape, dtype, sweeps, penalties, iters=3, const_w=True)
    eng = cd_engine(shape, dtype, sweeps, penalties)
    upload_csr(eng, rows, cols, vals, m)
    W, H, f, _ = run(eng, W0, H0, 3, constant_w=True)
    eng.close()
    assert np.array_equal(W, W0)
    # (with W fixed the H step is a function of H alone: the fp32 figure is the half-step's, bounded by the full iteration's of the parity test)
    tol = hm.TOL_F64 if dtype == np.float64 else hm.MARGIN * max(hm.rel(_const_w_in(shape, sweeps, penalties), snaps[3][1]), 0.0)
    assert hm.rel(H, snaps[3][1]) <= tol
    assert f == pytest.approx(errs[-1], rel=ERR_TOL[dtype])


def _const_w_in(shape, sweeps, penalties):
    rows, cols, vals, W0, H0 = problem(shape, np.float32)
    return cd.run_in(rows, cols, vals, W0, H0, 3, sweeps[0], sweeps[1], penalties, const_w=True)[1]


@pytest.mark.parametrize("dtype", DTYPES, ids=ident)
def test_every_input_form_and_a_repeat_are_bit_identical(dtype):
    import torch
    shape = SHAPES[1]
    m, n, r = shape
    rows, cols, vals, W0, H0 = problem(shape, dtype)
    vals = vals.astype(dtype)
    outs = []

    def go(upload):
        eng = cd_engine(shape, dtype, (2, 2), PENALTIES[1])
        upload(eng)
        outs.append(run(eng, W0, H0, 4))
        eng.close()

    D = np.full((m, n), np.nan, dtype=dtype); D[rows, cols] = vals
    go(lambda e: e.upload(F(D)))
    go(lambda e: upload_csr(e, rows, cols, vals, m))
    cp, ci, cv = mref.csc_of(rows, cols, vals, n)
    go(lambda e: e.upload_sparse(2, cv.astype(dtype), cp, ci, 0))
    perm = np.random.default_rng(43).permutation(len(vals))
    coo = (vals[perm], rows[perm].astype(np.int32), cols[perm].astype(np.int32))
    go(lambda e: e.upload_sparse(3, *coo, 0))
    go(lambda e: e.upload_device_stored(torch.from_numpy(np.ascontiguousarray(D)).cuda()))
    go(lambda e: e.upload_sparse_device(3, *[torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in coo], 0))
    go(lambda e: upload_csr(e, rows, cols, vals, m))      # a repeat
    for o in outs[1:]:
        assert np.array_equal(o[0], outs[0][0]) and np.array_equal(o[1], outs[0][1])
        assert o[2] == outs[0][2] and o[3] == outs[0][3]
    assert np.isfinite(outs[0][2]) and not np.array_equal(outs[0][0], W0)


@pytest.mark.parametrize("case", cd.TABLE[:2], ids=lambda c: f"{c[0]}x{c[1]}-r{c[2]}")
def test_ahead_of_the_multiplicative_update(case):
    """fp64 engines from one start: 30 iterations of coordinate descent report a lower error than 100 of the multiplicative update."""
    m, n, r, density, seed = case
    rows, cols, vals = mref.planted_ratings(m, n, density, seed)
    W0, H0 = (F(x) for x in cd.start(m, n, r, seed))
    errs = {}
    for solver, iters in (("cd", 30), ("mu", 100)):
        eng = na.Engine(m, n, r, "mu", dtype=np.float64, missing_values=True, missing_solver=solver)
        upload_csr(eng, rows, cols, vals, m)
        errs[solver] = run(eng, W0, H0, iters)[2]
        eng.close()
    print(case, errs)
    assert errs["cd"] < errs["mu"], errs
    assert errs["cd"] == pytest.approx(cd.run(rows, cols, vals, W0, H0, 30)[2][-1], rel=1e-9)


@pytest.mark.parametrize("dtype", DTYPES, ids=ident)
def test_switching_back_to_the_multiplicative_update(dtype):
    """After set_missing_solver("mu") the next iteration is the masked multiplicative update from the factors as they are; and back again."""
    shape = SHAPES[0]
    m, n, r = shape
    rows, cols, vals, W0, H0 = problem(shape, dtype)
    eng = cd_engine(shape, dtype, (2, 2))
    upload_csr(eng, rows, cols, vals, m)
    eng.set_factors(W0, H0)
    eng.iterate(3, error_every=0)
    eng.set_missing_solver("mu")
    W1, H1 = eng.get_factors()
    eng.iterate(1, first_iteration=1, error_every=1)
    W2, H2 = eng.get_factors()
    Wr, Hr, fr = mref.iteration(rows, cols, vals, W1, H1, float(np.finfo(dtype).eps), compute_error=True)
    ftol, etol = MU_TOL[dtype]
    assert hm.rel(W2, Wr) < ftol and hm.rel(H2, Hr) < ftol
    assert eng.frobenius == pytest.approx(fr, rel=etol)
    # a fresh multiplicative engine from the same factors gives the same bits: the switch left nothing behind
    fresh = na.Engine(m, n, r, "mu", dtype=dtype, missing_values=True)
    upload_csr(fresh, rows, cols, vals, m)
    fresh.set_factors(W1, H1)
    fresh.iterate(1, first_iteration=1, error_every=1)
    Wf, Hf = fresh.get_factors()
    assert np.array_equal(Wf, W2) and np.array_equal(Hf, H2) and fresh.frobenius == eng.frobenius
    fresh.close()
    # and forward again: the iteration of an engine that was never switched, from these factors
    eng.set_missing_solver("cd", 2, 2)
    eng.iterate(1, first_iteration=1, error_every=1)
    other = cd_engine(shape, dtype, (2, 2))
    upload_csr(other, rows, cols, vals, m)
    other.set_factors(W2, H2)
    other.iterate(1, first_iteration=1, error_every=1)
    for a, b in zip(eng.get_factors(), other.get_factors()):
        assert np.array_equal(a, b)
    assert eng.frobenius == other.frobenius
    eng.close(); other.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=ident)
def test_predict_score_and_top_k(dtype):
    shape = SHAPES[1]
    m, n, r = shape
    rows, cols, vals, W0, H0 = problem(shape, dtype)
    eng = cd_engine(shape, dtype, (2, 2), PENALTIES[1])
    upload_csr(eng, rows, cols, vals, m)
    W, H, f, _ = run(eng, W0, H0, 3)
    W64, H64 = W.astype(np.float64), H.astype(np.float64)
    u = hm.UNIT[dtype]
    exact = np.einsum("pk,pk->p", W64[rows], H64.T[cols])
    bound = tref.gamma(r, u) * np.einsum("pk,pk->p", np.abs(W64[rows]), np.abs(H64.T[cols]))
    pred = eng.predict(rows.astype(np.int32), cols.astype(np.int32))
    assert np.all(np.abs(pred - exact) <= bound)
    sc = eng.score(rows.astype(np.int32), cols.astype(np.int32), vals.astype(dtype))
    assert sc["count"] == len(vals)
    assert sc["sq"] == pytest.approx(float(np.sum((vals - exact) ** 2)), rel=ERR_TOL[dtype])
    queries = np.array([0, EMPTY_ROW, 17, m - 1], dtype=np.int32)
    for axis, A, B, q in ((0, W64, H64.T, queries), (1, H64.T, W64, np.array([0, EMPTY_COL, n - 1], dtype=np.int32))):
        idx, scores = eng.top_k(q, 7, axis=axis)
        tref.check_top_k(idx, scores, A, B, q, 7, None, 0, u)
    # the engine is as it was: the next iteration is that of an engine that was never asked
    eng.iterate(1, first_iteration=1, error_every=1)
    other = cd_engine(shape, dtype, (2, 2), PENALTIES[1])
    upload_csr(other, rows, cols, vals, m)
    other.set_factors(W, H)
    other.iterate(1, first_iteration=1, error_every=1)
    for a, b in zip(eng.get_factors(), other.get_factors()):
        assert np.array_equal(a, b)
    eng.close(); other.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=ident)
@pytest.mark.parametrize("form", ["dense", "csr"])
def test_compute_with_missing_solver(ctx, dtype, form):
    """nmfgpu::compute with "missingSolver" = 1 and the solver's sweeps and penalties equals the engine run bit for bit."""
    shape = SHAPES[0]
    m, n, r = shape
    rows, cols, vals, W0, H0 = problem(shape, dtype)
    iters = 12
    keep = []
    if form == "dense":
        D = np.full((m, n), np.nan, dtype=dtype); D[rows, cols] = vals
        V = F(D)
    else:
        ptr, idx, v = mref.csr_of(rows, cols, vals, m)
        v = v.astype(dtype); keep = [ptr, idx, v]
        V = api.sparse_description(na.StorageFormat.CSR, m, n, v, ptr, idx)
    params = {"missingValues": 1, "missingSolver": 1, "sweepsH": 3, "sweepsW": 2, "l1W": 0.05, "l1H": 0.05, "l2W": 0.01, "l2H": 0.01}
    W, H = W0.copy(order="F"), H0.copy(order="F")
    s = na.Summary()
    assert na.compute(V, W, H, iterations=iters, parameters=params, summary=s) == na.ResultType.Success
    rec = s.record(0)
    eng = cd_engine(shape, dtype, (3, 2), PENALTIES[1])
    upload_csr(eng, rows, cols, vals, m)
    eng.set_factors(W0, H0)
    eng.iterate(iters, first_iteration=1, error_every=10, last_iteration=iters)
    We, He = eng.get_factors()
    assert np.array_equal(W, We) and np.array_equal(H, He)
    assert rec.frobenius == eng.frobenius and rec.rmsd == eng.rmsd and rec.numIterations == iters
    eng.close()
    # "missingSolver" = 0 is the multiplicative update of "missingValues" alone
    outs = []
    for p in ({"missingValues": 1}, {"missingValues": 1, "missingSolver": 0}):
        W, H = W0.copy(order="F"), H0.copy(order="F")
        assert na.compute(V, W, H, iterations=5, parameters=p) == na.ResultType.Success
        outs.append((W, H))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    s.destroy()
    del keep


def test_threshold_stop_at_the_restatements_iteration(ctx):
    """A Frobenius threshold between the restatement's changes over iterations 20 -> 30 and 30 -> 40 ends a run of 60 at iteration 40 (fp64: the changes of an fp32
    trajectory are not separated from each other by more than its distance from the restatement)."""
    shape, dtype = SHAPES[0], np.float64
    m, n, r = shape
    rows, cols, vals, W0, H0 = problem(shape, dtype)
    errs = cd.run(rows, cols, vals, W0, H0, 40)[2]
    d20, d30, d40 = (abs(errs[t - 1] - errs[t - 11]) for t in (20, 30, 40))
    assert d20 > d30 > 2 * d40 > 0, (d20, d30, d40)
    threshold = float(np.sqrt(d30 * d40))
    D = np.full((m, n), np.nan, dtype=dtype); D[rows, cols] = vals
    W, H = W0.copy(order="F"), H0.copy(order="F")
    s = na.Summary()
    assert na.compute(F(D), W, H, iterations=60, threshold_type=na.NmfThresholdType.Frobenius, threshold=threshold,
                      parameters={"missingValues": 1, "missingSolver": 1}, summary=s) == na.ResultType.Success
    rec = s.record(0)
    assert rec.numIterations == 40
    assert rec.frobenius == pytest.approx(errs[39], rel=1e-9)
    s.destroy()


def test_refusals_of_the_setter():
    m, n, r = 90, 70, 6

    def refusal(call):
        with pytest.raises(na.EngineError) as info:
            call()
        assert info.value.status == 1
        return str(info.value)

    plain = na.Engine(m, n, r, "mu", dtype=np.float32)
    assert "needs 'missingValues' = 1" in refusal(lambda: plain.set_missing_solver("cd"))
    assert "needs 'missingValues' = 1" in refusal(lambda: plain.set_missing_solver("mu"))
    plain.close()
    assert "needs 'missingValues' = 1" in refusal(lambda: na.Engine(m, n, r, "hals", missing_solver="cd"))
    beta = na.Engine(m, n, r, "mu", dtype=np.float32, missing_values=True, missing_divergence="kl")
    assert "Frobenius objective only" in refusal(lambda: beta.set_missing_solver("cd"))
    beta.close()
    wide = na.Engine(140, 135, 129, "mu", dtype=np.float64, missing_values=True)
    assert "1 ... 128 features" in refusal(lambda: wide.set_missing_solver("cd"))
    wide.set_missing_solver("mu")
    wide.close()
    assert "1 ... 128 features" in refusal(lambda: na.Engine(140, 135, 129, "mu", missing_values=True, missing_solver="cd"))
    eng = na.Engine(m, n, r, "mu", dtype=np.float32, missing_values=True)
    for sweeps in ((0, 1), (1, 0), (65, 1), (1, 65)):
        assert "integers in 1 ... 64" in refusal(lambda: eng.set_missing_solver("cd", *sweeps))
    for bad in (-0.1, float("nan"), float("inf")):
        for slot in range(4):
            p = [0.0] * 4
            p[slot] = bad
            assert "finite and >= 0" in refusal(lambda: eng.set_missing_solver("cd", 1, 1, *p))
    assert "range of the engine's precision" in refusal(lambda: eng.set_missing_solver("cd", 1, 1, 1e39))
    assert "sweeps 1 and penalties 0 only" in refusal(lambda: eng.set_missing_solver("mu", 2, 1))
    assert "sweeps 1 and penalties 0 only" in refusal(lambda: eng.set_missing_solver("mu", 1, 1, 0.0, 0.1))
    # the HALS engines' setters keep refusing a masked engine, whatever its solver
    eng.set_missing_solver("cd", 2, 2, 0.1, 0.1, 0.1, 0.1)
    assert "only the HALS algorithm" in refusal(lambda: eng.set_penalties(0.1, 0.0, 0.0, 0.0))
    assert "only the HALS algorithm" in refusal(lambda: eng.set_sweeps(2, 2))
    # a refused call changes nothing: the engine still runs the setting it had
    rows, cols, vals = mref.planted_ratings(m, n, 0.3, seed=1)
    upload_csr(eng, rows, cols, vals, m)
    W0, H0 = (F(x.astype(np.float32)) for x in cd.start(m, n, r, 1))
    got = run(eng, W0, H0, 2)
    eng.close()
    other = cd_engine((m, n, r), np.float32, (2, 2), (0.1, 0.1, 0.1, 0.1))
    upload_csr(other, rows, cols, vals, m)
    want = run(other, W0, H0, 2)
    other.close()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
