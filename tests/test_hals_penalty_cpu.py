"""Penalised HALS without a GPU: the fp64 restatement the GPU tests compare with (tests/hals_penalty_reference.py) against the unpenalised one and
against the properties that define it (a non-increasing penalised objective, sparse factors under L1), and the refusals nmfgpu::compute makes for
the penalty parameters before it touches a device."""
import numpy as np
import pytest

from tests import hals_penalty_reference as pen
from tests import hals_reference as ref


def issue_problem():
    """The problem the sparsity floor below was derived on: default_rng(7), V = rand(m, r) rand(r, n) + 0.01 rand(m, n), start 1 - rand, in that order."""
    rng = np.random.default_rng(7)
    m, n, r = 300, 200, 12
    V = rng.random((m, r)) @ rng.random((r, n)) + 0.01 * rng.random((m, n))
    W = 1.0 - rng.random((m, r))
    H = 1.0 - rng.random((r, n))
    return V, W, H


def test_zero_penalties_are_the_unpenalised_restatement():
    V, W, H = issue_problem()
    Wa, Ha, Wb, Hb = W, H, W, H
    for _ in range(10):
        Wa, Ha, ea = pen.iteration(V, Wa, Ha)
        Wb, Hb, eb = ref.iteration(V, Wb, Hb)
        assert np.array_equal(Wa, Wb) and np.array_equal(Ha, Hb) and ea == eb
    # ... and with constant W
    Wa, Ha, ea = pen.iteration(V, W, H, constant_w=True)
    Wb, Hb, eb = ref.iteration(V, W, H, constant_w=True)
    assert np.array_equal(Wa, Wb) and np.array_equal(Ha, Hb) and ea == eb


def assert_monotone(V, W, H, p, iters=30, constant_w=False):
    objs = [pen.objective(V, W, H, *p)]
    for _ in range(iters):
        W, H, _e = pen.iteration(V, W, H, *p, constant_w=constant_w)
        objs.append(pen.objective(V, W, H, *p))
    for a, b in zip(objs, objs[1:]):
        assert b <= a * (1 + 1e-12), (p, a, b)
    assert objs[-1] < objs[0]
    return W, H


@pytest.mark.parametrize("p", [(0.5, 0.5, 0.1, 0.1), (0.0, 2.0, 0.0, 0.0), (1.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 1.0)])
def test_penalised_objective_never_increases(p):
    V, W, H = issue_problem()
    assert_monotone(V, W, H, p)


def test_penalised_objective_never_increases_with_constant_w():
    V, W, H = issue_problem()
    Wn, _ = assert_monotone(V, W, H, (0.0, 0.7, 0.0, 0.3), constant_w=True)
    assert np.array_equal(Wn, W)


def test_penalised_objective_never_increases_on_sparse_v():
    rng = np.random.default_rng(11)
    m, n, r = 300, 200, 12
    _rows, _cols, _vals, V = pen.sparse_pattern(m, n, 0.05, rng, empty_rows=(3, 150), empty_cols=(0, 77))
    W = 1.0 - rng.random((m, r))
    H = 1.0 - rng.random((r, n))
    Wn, Hn = assert_monotone(V, W, H, (0.05, 0.05, 0.01, 0.01))
    # empty rows / columns of V: zero rows of W and zero columns of H (the first sweep clamps them: a = 0, gradient > 0)
    assert (Wn[[3, 150]] == 0).all() and (Hn[:, [0, 77]] == 0).all()
    assert np.isfinite(Wn).all() and np.isfinite(Hn).all()


def test_l1_makes_the_factors_sparse():
    """After 30 iterations from one start, H (and W) have at least four times as many exact zeros with l1W = l1H = 5 as with no penalty; the factor
    four is a floor under 922 against 120 (of 2 400, H) and 1 526 against 197 (of 3 600, W) that a restatement gave on this problem."""
    V, W, H = issue_problem()
    W0, H0, _ = pen.run(V, W, H, 30)
    W5, H5, _ = pen.run(V, W, H, 30, 5.0, 5.0, 0.0, 0.0)
    print("zeros of H:", int((H5 == 0).sum()), "against", int((H0 == 0).sum()), "; of W:", int((W5 == 0).sum()), "against", int((W0 == 0).sum()))
    print("relative error:", np.linalg.norm(V - W5 @ H5) / np.linalg.norm(V), "against", np.linalg.norm(V - W0 @ H0) / np.linalg.norm(V))
    assert (H5 == 0).sum() >= 4 * (H0 == 0).sum() and (H0 == 0).sum() > 0
    assert (W5 == 0).sum() >= 4 * (W0 == 0).sum()


def test_l2_updates_a_coordinate_with_zero_diagonal():
    """G[k,k] = 0 is skipped without l2 and updated with it (d_k = l2 > 0)."""
    G = np.diag([2.0, 0.0, 4.0])
    A = np.array([[4.0], [3.0], [8.0]])
    P = np.array([[1.0], [5.0], [1.0]])
    assert np.array_equal(pen.sweep(P, A, G), [[2.0], [5.0], [2.0]])
    # d = (4, 2, 6); p1 <- 5 - (2 * 5 - 3 + 1) / 2 = 1
    assert np.array_equal(pen.sweep(P, A, G, 1.0, 2.0), [[1.0 - (2.0 + 2.0 - 4.0 + 1.0) / 4.0], [1.0], [1.0 - (4.0 + 2.0 - 8.0 + 1.0) / 6.0]])


# ------------------------------------------------------------------ nmfgpu::compute: refusals before any device work

@pytest.fixture
def context():
    import nmfgpu_amd as na
    assert na.initialize() in (na.ResultType.Success, na.ResultType.ErrorAlreadyInitialized)
    na.set_verbosity(na.Verbosity.Nothing)
    yield na
    na.finalize()


def _compute(V, W, H, params, **kw):
    import nmfgpu_amd as na
    return na.compute(V, W, H, iterations=3, parameters=params, **kw)


def test_refusals_before_the_device(context):
    na = context
    rng = np.random.default_rng(0)
    m, n, r = 20, 12, 3
    V = np.asfortranarray(rng.random((m, n)).astype(np.float32))
    W = np.asfortranarray(rng.random((m, r)).astype(np.float32)); H = np.asfortranarray(rng.random((r, n)).astype(np.float32))
    W0, H0 = W.copy(), H.copy()
    bad = na.ResultType.ErrorInvalidArgument
    hals = dict(algorithm=na.NmfAlgorithm.HALS)
    for name in ("l1W", "l1H", "l2W", "l2H"):
        for value in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
            assert _compute(V, W, H, {name: value}, **hals) == bad, (name, value)
        # a finite double that is not finite in the engine's precision
        assert _compute(V, W, H, {name: 1e300}, **hals) == bad, name
        # a non-zero value with another algorithm
        assert _compute(V, W, H, {name: 0.5}) == bad, name
        assert _compute(V, W, H, {name: 0.5, "lambda": 0.1}, algorithm=na.NmfAlgorithm.GDCLS) == bad, name
        assert _compute(V, W, H, {name: 0.5, "theta": 0.5}, algorithm=na.NmfAlgorithm.nsNMF) == bad, name
    # what stays refused for HALS, with or without penalties and sparse compute
    for extra in ({}, {"l1H": 0.5}, {"sparseCompute": 1}):
        assert _compute(V, W, H, {**extra, "divergence": 1}, **hals) == bad
        assert _compute(V, W, H, {**extra, "numGpus": 2}, **hals) == bad
        assert _compute(V, W, H, {**extra, "missingValues": 1}, **hals) == bad
    assert _compute(V, W, H, {"sparseCompute": 1}, algorithm=na.NmfAlgorithm.ALS) == bad
    # sparse compute with HALS: at most 256 features
    Vw = np.asfortranarray(rng.random((300, 280)).astype(np.float32))
    Ww = np.asfortranarray(rng.random((300, 257)).astype(np.float32)); Hw = np.asfortranarray(rng.random((257, 280)).astype(np.float32))
    assert _compute(Vw, Ww, Hw, {"sparseCompute": 1}, **hals) == bad
    assert np.array_equal(W, W0) and np.array_equal(H, H0)
    if na.device_count() == 0:
        # the valid forms get as far as the device: penalties and sparse compute with HALS, zero-valued penalties with any algorithm
        ok = na.ResultType.ErrorExternalLibrary
        assert _compute(V, W, H, {"l1W": 0.5, "l1H": 0.5, "l2W": 0.1, "l2H": 0.1}, **hals) == ok
        assert _compute(V, W, H, {"sparseCompute": 1}, **hals) == ok
        assert _compute(V, W, H, {"sparseCompute": 1, "l1H": 2.0}, **hals) == ok
        assert _compute(V, W, H, {"l1W": 0.0, "l1H": 0.0, "l2W": 0.0, "l2H": 0.0}) == ok
        assert _compute(V, W, H, {"l2W": 0.0, "lambda": 0.1}, algorithm=na.NmfAlgorithm.GDCLS) == ok
