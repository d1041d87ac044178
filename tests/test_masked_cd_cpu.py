"""Missing-value coordinate descent without a device (docs/MISSING.md, "Coordinate descent"): what tests/masked_cd_reference.py -- the yardstick of
tests/test_gpu_masked_cd_kernel.py and tests/test_gpu_masked_cd.py -- itself satisfies, and the refusals that need no device."""
import numpy as np
import pytest

from tests import hals_penalty_reference as pen
from tests import masked_cd_reference as cd
from tests import masked_reference as mref


def table_problem(case):
    m, n, r, density, seed = case
    rows, cols, vals = mref.planted_ratings(m, n, density, seed)
    W, H = cd.start(m, n, r, seed)
    return rows, cols, vals, W, H


_RUNS = {}


def cd_run(case, sweeps):
    if (case, sweeps) not in _RUNS:
        rows, cols, vals, W, H = table_problem(case)
        _RUNS[(case, sweeps)] = cd.run(rows, cols, vals, W, H, 30, sweeps, sweeps)
    return _RUNS[(case, sweeps)]


@pytest.mark.parametrize("sweeps", [1, 3])
@pytest.mark.parametrize("case", cd.TABLE, ids=lambda c: f"{c[0]}x{c[1]}-r{c[2]}")
def test_reported_error_is_monotone(case, sweeps):
    """The error of the pair (W_{k-1}, H_k) never increases over 30 iterations, within a factor 1 + 1e-12."""
    errs = cd_run(case, sweeps)[2]
    assert len(errs) == 30
    for a, b in zip(errs, errs[1:]):
        assert b <= a * (1 + 1e-12), errs


@pytest.mark.parametrize("case", cd.TABLE, ids=lambda c: f"{c[0]}x{c[1]}-r{c[2]}")
def test_ahead_of_the_multiplicative_update(case):
    """Thirty iterations of coordinate descent end below a hundred of the multiplicative update from the same start; three sweeps per half-step end lower still."""
    rows, cols, vals, W, H = table_problem(case)
    mu = mref.run(rows, cols, vals, W, H, 100, np.finfo(np.float64).eps)[2]
    one, three = cd_run(case, 1)[2][-1], cd_run(case, 3)[2][-1]
    print(f"{case}: cd(1) {one:.4f} cd(3) {three:.4f} mu100 {mu:.4f}")
    assert one < mu
    assert three < one


@pytest.mark.parametrize("penalties", [(0.05, 0.02, 0.01, 0.03), (0.0, 0.1, 0.2, 0.0)])
def test_fully_observed_is_penalised_hals(penalties):
    """Every entry observed: each row's Gram matrix is the factor's, and one iteration is hals_penalty_reference's (no normalisation with a penalty)."""
    rng = np.random.default_rng(7)
    m, n, r = 40, 30, 5
    V = rng.random((m, r)) @ rng.random((r, n)) + 0.01 * rng.random((m, n))
    W, H = cd.start(m, n, r, 7)
    rows, cols = np.nonzero(np.ones((m, n), dtype=bool))
    W1, H1, f1 = cd.iteration(rows, cols, V[rows, cols], W, H, penalties=penalties)
    l1W, l1H, l2W, l2H = penalties
    W2, H2, f2 = pen.iteration(V, W, H, l1W, l1H, l2W, l2H)
    assert np.linalg.norm(W1 - W2) <= 1e-12 * np.linalg.norm(W2)
    assert np.linalg.norm(H1 - H2) <= 1e-12 * np.linalg.norm(H2)
    assert abs(f1 - f2) <= 1e-12 * f2


def test_penalised_objective_decreases():
    """With penalties every half-step is an exact block-coordinate minimisation of the penalised objective: it never increases."""
    case = cd.TABLE[0]
    rows, cols, vals, W, H = table_problem(case)
    penalties = (0.05, 0.05, 0.01, 0.01)
    last = cd.objective(rows, cols, vals, W, H, penalties)
    for _ in range(5):
        W, H, _ = cd.iteration(rows, cols, vals, W, H, 2, 2, penalties)
        now = cd.objective(rows, cols, vals, W, H, penalties)
        assert now <= last * (1 + 1e-12)
        last = now


def test_empty_rows_and_padding_of_a_half_step():
    """A row without an entry becomes 0, rows beyond `rows` stay, coordinates >= r of an updated row become 0; the fp32 form agrees with the fp64 one."""
    rng = np.random.default_rng(3)
    ptr = np.array([0, 3, 3, 5], dtype=np.int32)
    idx = np.array([4, 1, 4, 0, 2], dtype=np.int32)
    val = rng.random(5)
    A = rng.random((4, 8)); B = rng.random((6, 8))
    out, G, c = cd.half_step(ptr, idx, val, A, B, 5, 3, sweeps=2, l1=0.01, l2=0.02)
    assert np.array_equal(out[1], np.zeros(8)) and np.array_equal(out[3], A[3])
    assert np.array_equal(out[:3, 5:], np.zeros((3, 3)))
    assert np.allclose(G[0], B[[4, 1, 4], :5].T @ B[[4, 1, 4], :5]) and np.array_equal(G[1], np.zeros((5, 5)))
    out32 = cd.half_step_in(ptr, idx, val, A, B, 5, 3, sweeps=2, l1=0.01, l2=0.02)
    assert out32.dtype == np.float32
    assert np.linalg.norm(out32[:3] - out[:3]) <= 1e-5 * np.linalg.norm(out[:3])


# ------------------------------------------------------------------ refusals that need no device

def test_the_rule_of_the_setter():
    import nmfgpu_amd as na
    ok = dict(dtype=np.float32, missing_values=True, missing_divergence=0, r=128)
    assert na.missing_solver_fault(1, 1, 1, **ok) is None
    assert na.missing_solver_fault(1, 64, 3, 0.1, 0.2, 0.3, 0.4, **ok) is None
    assert na.missing_solver_fault(0, **ok) is None
    assert "0 (multiplicative update) or 1" in na.missing_solver_fault(2, **ok)
    assert "0 (multiplicative update) or 1" in na.missing_solver_fault(0.5, **ok)
    assert "needs 'missingValues' = 1" in na.missing_solver_fault(1, **{**ok, "missing_values": False})
    assert "Frobenius objective only" in na.missing_solver_fault(1, **{**ok, "missing_divergence": 1})
    assert "1 ... 128 features" in na.missing_solver_fault(1, **{**ok, "r": 129})
    assert na.missing_solver_fault(0, **{**ok, "r": 129}) is None
    for sweeps in ((0, 1), (1, 65), (1.5, 1)):
        assert "integers in 1 ... 64" in na.missing_solver_fault(1, *sweeps, **ok)
    for bad in (-0.1, float("nan"), float("inf")):
        for slot in range(4):
            p = [0.0] * 4
            p[slot] = bad
            assert "finite and >= 0" in na.missing_solver_fault(1, 1, 1, *p, **ok)
    assert "range of the engine's precision" in na.missing_solver_fault(1, 1, 1, 1e39, **ok)
    assert na.missing_solver_fault(1, 1, 1, 1e39, **{**ok, "dtype": np.float64}) is None
    for extras in ((2, 1, 0, 0, 0, 0), (1, 1, 0, 0, 0.1, 0)):
        assert "sweeps 1 and penalties 0 only" in na.missing_solver_fault(0, *extras, **ok)


def test_python_refuses_before_the_library():
    import nmfgpu_amd as na
    e = na.Engine.from_handle(0, 10, 10, 2)
    with pytest.raises(ValueError):
        e.set_missing_solver("hals")
    with pytest.raises(ValueError):
        e.set_missing_solver("cd", 1.5, 1)
    with pytest.raises(na.EngineError):      # (no engine behind the wrapper: the library refuses the null handle)
        e.set_missing_solver("cd")
    with pytest.raises(ValueError):
        na.Engine(10, 10, 2, missing_values=True, missing_sweeps_h=2)


@pytest.fixture
def context():
    import nmfgpu_amd as na
    assert na.initialize() in (na.ResultType.Success, na.ResultType.ErrorAlreadyInitialized)
    na.set_verbosity(na.Verbosity.Nothing)
    yield na
    na.finalize()


def test_compute_refuses_before_the_device(context):
    na = context
    rng = np.random.default_rng(0)
    m, n, r = 20, 12, 3
    V = np.asfortranarray(rng.random((m, n)).astype(np.float32))
    V[0, 0] = np.nan
    W = np.asfortranarray(rng.random((m, r)).astype(np.float32)); H = np.asfortranarray(rng.random((r, n)).astype(np.float32))
    W0, H0 = W.copy(), H.copy()
    bad = na.ResultType.ErrorInvalidArgument

    def run(params, V=V, W=W, H=H, **kw):
        return na.compute(V, W, H, iterations=3, parameters=params, **kw)

    on = {"missingValues": 1, "missingSolver": 1}
    assert run({"missingSolver": 1}) == bad
    assert run({"missingSolver": 0}) == bad
    assert run({"missingValues": 0, "missingSolver": 1}) == bad
    for d in (1, 2, 3):
        assert run({**on, "missingDivergence": d, **({"missingBeta": 0.5} if d == 3 else {})}) == bad
    for value in (2, -1, 0.5, float("nan")):
        assert run({"missingValues": 1, "missingSolver": value}) == bad
    assert run({**on, "sweepsH": 0}) == bad
    assert run({**on, "sweepsW": 65}) == bad
    assert run({**on, "l1W": -1.0}) == bad
    assert run({**on, "l2H": float("inf")}) == bad
    assert run({"missingValues": 1, "missingSolver": 0, "sweepsH": 2}) == bad
    assert run({"missingValues": 1, "missingSolver": 0, "l1H": 0.1}) == bad
    assert run(on, algorithm=na.NmfAlgorithm.HALS) == bad
    # without the solver the extras stay the HALS engines': refused beside the multiplicative algorithm, as before
    assert run({"missingValues": 1, "sweepsH": 2}) == bad
    assert run({"missingValues": 1, "l1W": 0.1}) == bad
    Vw = np.asfortranarray(rng.random((140, 135)).astype(np.float32))
    Vw[0, 0] = np.nan
    Ww = np.asfortranarray(rng.random((140, 129)).astype(np.float32)); Hw = np.asfortranarray(rng.random((129, 135)).astype(np.float32))
    assert run(on, V=Vw, W=Ww, H=Hw) == bad
    assert np.array_equal(W, W0) and np.array_equal(H, H0)
    if na.device_count() == 0:
        # the valid forms get as far as the device
        assert run(on) == na.ResultType.ErrorExternalLibrary
        assert run({**on, "sweepsH": 3, "sweepsW": 2, "l1W": 0.1, "l2H": 0.2}) == na.ResultType.ErrorExternalLibrary
        assert run({"missingValues": 1, "missingSolver": 0}) == na.ResultType.ErrorExternalLibrary
        assert run({"missingValues": 1, "missingSolver": 0}, V=Vw, W=Ww, H=Hw) == na.ResultType.ErrorExternalLibrary
