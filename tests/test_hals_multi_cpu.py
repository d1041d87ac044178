"""Accelerated HALS without a GPU (docs/HALS.md, "Inner sweeps"): the fp64 restatement the GPU tests compare with (tests/hals_multi_reference.py) against the
restatements it is built on and against the properties that define it, the conditions the kernel-level GPU tests rely on (tests/hals_multi_cases.py), the fp32
yardstick of the engine tests, and what the loaded library exports."""
import numpy as np
import pytest

from tests import hals_multi_cases as mc
from tests import hals_multi_reference as multi
from tests import hals_penalty_reference as pen
from tests import hals_reference as ref

PEN = (0.05, 0.05, 0.01, 0.01)


def test_one_sweep_each_is_the_plain_restatement_bit_for_bit():
    V, W, H = mc.planted(120, 90, 9, np.float64, seed=3)
    Wa, Ha, ea = multi.run(V, W, H, 8, 1, 1)
    Wb, Hb, eb = ref.run(V, W, H, 8)
    assert np.array_equal(Wa, Wb) and np.array_equal(Ha, Hb) and ea == eb
    Wa, Ha, ea = multi.run(V, W, H, 8, 1, 1, PEN)
    Wb, Hb, eb = pen.run(V, W, H, 8, *PEN)
    assert np.array_equal(Wa, Wb) and np.array_equal(Ha, Hb) and ea == eb
    for p in ((0.0, 0.0, 0.0, 0.0), PEN):
        Wa, Ha, ea = multi.run(V, W, H, 3, 1, 1, p, constant_w=True)
        Wb, Hb, eb = pen.run(V, W, H, 3, *p, constant_w=True)
        assert np.array_equal(Wa, W) and np.array_equal(Ha, Hb) and ea == eb


@pytest.mark.parametrize("l1,l2", [(0.0, 0.0), (0.05, 0.01), (2.0, 0.0)])
def test_objective_does_not_rise_from_one_inner_sweep_to_the_next(l1, l2):
    """For fixed W, 1/2 ||V - W H||^2 + l1 ||H||_1 + 1/2 l2 ||H||^2 after t + 1 sweeps is at most that after t sweeps (1e-12 relative): every coordinate step
    minimises it exactly along its coordinate."""
    V, W, H = mc.planted(120, 90, 9, np.float64, seed=5)
    H0 = H      # (the sweeps return new arrays)
    A, G = W.T @ V, W.T @ W
    objs = [pen.objective(V, W, H, 0.0, l1, 0.0, l2)]
    for _ in range(8):
        H = multi.sweeps(H, A, G, None, 1, l1, l2)
        objs.append(pen.objective(V, W, H, 0.0, l1, 0.0, l2))
    for a, b in zip(objs, objs[1:]):
        assert b <= a * (1 + 1e-12), (a, b)
    assert objs[-1] < objs[0]
    assert np.array_equal(H, multi.sweeps(H0, A, G, None, 8, l1, l2))      # (s sweeps: s applications of one)


def test_more_sweeps_reach_a_lower_error_in_twenty_iterations():
    V, W, H = mc.planted(500, 300, 7, np.float64, seed=1)
    e11 = np.linalg.norm(V - np.matmul(*multi.run(V, W, H, 20, 1, 1)[:2]))
    e44 = np.linalg.norm(V - np.matmul(*multi.run(V, W, H, 20, 4, 4)[:2]))
    print("||V - W H|| after 20 iterations: (1, 1)", e11, "(4, 4)", e44)
    assert e44 < e11


# ------------------------------------------------------------------ conditions on the kernel cases of tests/test_gpu_hals_multi.py

CASE_IDS = [mc.case_id(c) for c in mc.SWEEP_CASES]


@pytest.mark.parametrize("case", mc.SWEEP_CASES, ids=CASE_IDS)
def test_order_case_stays_an_integer_problem(case):
    """At s = 2 and 3 every value of every sweep and every G . h of order_case is an integer below 2^24 (the largest found: 128), so fp32 and fp64 kernels in any
    summation order must reproduce the fp64 sweeps exactly.  Where r >= 3, every valid column still changes in the last sweep: a kernel that runs one sweep less
    differs in every column."""
    dtype, RP, r, lv, S = case
    P, slabs, G = ref.order_case(RP, r, mc.LEN_PAD, lv, S, mc.case_rng(case, 1), dtype)
    A = slabs.astype(np.float64).sum(axis=0)[:lv, :r].T
    assert all((np.abs(slabs.astype(np.float64)[:t + 1].sum(axis=0)) < 2 ** 24).all() for t in range(S))
    G64 = G.astype(np.float64)[:r, :r]
    h = P[:lv, :r].astype(np.float64).T
    largest = 0.0
    for s in range(1, max(mc.SWEEP_COUNTS) + 1):
        before = h.copy()
        for k in range(r):
            if G64[k, k] <= 0:
                continue
            terms = G64[k][:, None] * h
            dot = terms.sum(axis=0)
            h[k] = np.maximum(0.0, h[k] - (dot - A[k]) / G64[k, k])
            largest = max(largest, np.abs(terms).sum(axis=0).max(), np.abs(dot - A[k]).max(), np.abs(h[k]).max())
            assert (dot == np.round(dot)).all() and (h[k] == np.round(h[k])).all()
        assert np.array_equal(h.T, multi.panel_sweeps(P, slabs, G, r, lv, s))
        if r >= 3 and s in mc.SWEEP_COUNTS:
            assert (np.abs(h - before).max(axis=0) > 0).all(), f"sweep {s} leaves a column as it was"
    print(mc.case_id(case), "largest intermediate", largest)
    assert largest < 2 ** 24, largest


SEPARABLE = [c for c in mc.SWEEP_CASES if c[2] >= 3]      # (r = 1: the second sweep is a no-op, nothing to separate; r = 2 does not occur)


@pytest.mark.parametrize("case", SEPARABLE, ids=[mc.case_id(c) for c in SEPARABLE])
def test_dominant_case_separates_three_sweeps_from_two(case):
    """At s = 3 the last sweep of dominant_case moves every valid column, and some element by more than 100 x multi_sweep_bound in fp64 and at fp32 RP 64 (found:
    moves of 3.8e-3 at RP 64, 1.5e-3 at RP 256).  At the fp32 unit roundoff the bound grows with RP (gamma_{RP + S + 4}) while the move shrinks, so the ratio falls:
    24 ... 37 at RP 256, 5.6 ... 12 at RP 384, 3.2 ... 12 at RP 512.  What the GPU test needs is a ratio above 2: a kernel that runs s - 1 sweeps, or restarts from
    the old h, lands within the bound of the two-sweep result and cannot also be within the bound of the three-sweep one.  That is asserted for every case; the
    exact order_case test separates the sweep counts in every column besides.  (r = 1: the second sweep is a no-op, nothing to separate.)"""
    dtype, RP, r, lv, S = case
    for l1, l2 in mc.SWEEP_PENALTIES:
        P, slabs, G = ref.dominant_case(RP, r, mc.LEN_PAD, lv, S, mc.case_rng(case, 2), dtype)
        h1, h2, h3 = (multi.panel_sweeps(P, slabs, G, r, lv, s, l1, l2) for s in (1, 2, 3))
        b = multi.multi_sweep_bound(P[:lv].T, slabs[:, :lv].transpose(0, 2, 1), G, r, 3, mc.UNIT[dtype], l1, l2).T
        move = np.abs(h3 - h2)
        assert (move.max(axis=1) > 0).all()
        ratio = (move / np.maximum(b, 1e-300)).max()
        print(mc.case_id(case), (l1, l2), "largest move", move.max(), "move / bound", ratio)
        assert ratio > (100.0 if dtype == np.float64 or RP == 64 else 2.0), ratio
        assert (np.abs(h3 - h1) / np.maximum(b, 1e-300)).max() > 2.0      # (every sweep from the old h: the one-sweep result)


@pytest.mark.parametrize("case", [c for c in mc.SWEEP_CASES if c[0] == np.float32], ids=[mc.case_id(c) for c in mc.SWEEP_CASES if c[0] == np.float32])
@pytest.mark.parametrize("order", ["sequential", "reversed"])
def test_multi_sweep_bound_holds_for_float32_numpy_sweeps(case, order):
    """hals_reference.sweep_f32 repeated s times, in both summation orders, lies within multi_sweep_bound of the fp64 sweeps after every sweep; with s = 1 the
    bound is sweep_bound itself."""
    dtype, RP, r, lv, S = case
    P, slabs, G = ref.dominant_case(RP, r, mc.LEN_PAD, lv, S, mc.case_rng(case, 2), dtype)
    Pv, Sv = P[:lv].T, slabs[:, :lv].transpose(0, 2, 1)
    bounds = multi.multi_sweep_bound(Pv, Sv, G, r, 3, mc.UNIT[dtype], history=True)
    assert np.array_equal(bounds[0], ref.sweep_bound(Pv, Sv, G, r, mc.UNIT[dtype]))
    for s in (1, 2, 3):
        err = np.abs(multi.sweeps_f32(P, slabs, G, r, lv, s, order).astype(np.float64) - multi.panel_sweeps(P, slabs, G, r, lv, s))
        assert (err <= bounds[s - 1].T).all(), (s, (err / np.maximum(bounds[s - 1].T, 1e-300)).max())


def test_penalised_bound_is_the_bound_of_the_equivalent_problem():
    """G + l2 I against a - l1: the plain sweeps of that problem are the penalised sweeps (to rounding), which is what multi_sweep_bound relies on."""
    case = next(c for c in mc.SWEEP_CASES if c[1] == 128 and c[2] == 127)
    dtype, RP, r, lv, S = case
    P, slabs, G = ref.dominant_case(RP, r, mc.LEN_PAD, lv, S, mc.case_rng(case, 2), dtype)
    S_eq, G_eq = multi.equivalent_problem(slabs[:, :lv].transpose(0, 2, 1), G, r, 0.05, 0.01)
    plain = multi.sweeps(P[:lv, :r].T, S_eq.sum(axis=0)[:r], G_eq[:r, :r], r, 3)
    assert np.allclose(plain.T, multi.panel_sweeps(P, slabs, G, r, lv, 3, 0.05, 0.01), rtol=1e-12, atol=1e-13)


# ------------------------------------------------------------------ the fp32 yardstick of the engine tests

def test_engine_figure_is_what_the_restatements_give():
    """FIGURE_ENGINE_FACTORS is the largest norm-relative distance of W or H between the fp32 and the fp64 numpy restatement over the fp32 engine cases, held to
    [found, 1.5 x found]; the standing 2e-4 of tests/test_gpu_hals.py would already be missed by numpy itself at r = 129."""
    found = 0.0
    for case in mc.ENGINE_CASES:
        if case[4] != np.float32:
            continue
        for iters in mc.ENGINE_ITERS:
            w, h = mc.fp32_figure(case, iters)
            print(mc.engine_case_id(case), iters, "W", w, "H", h)
            found = max(found, w, h)
    print("found", found, "recorded", mc.FIGURE_ENGINE_FACTORS)
    assert found <= mc.FIGURE_ENGINE_FACTORS <= 1.5 * found, (found, mc.FIGURE_ENGINE_FACTORS)
    assert mc.MARGIN == 4.0 and mc.TOL_F64 == 1e-9


# ------------------------------------------------------------------ the library and nmfgpu::compute, no device needed

def test_library_exports_the_new_entries():
    from nmfgpu_amd import _lib
    lib = _lib.library()
    for name in ("nmfamd_engine_set_hals_sweeps", "nmfamd_op_hals_sweeps_f32", "nmfamd_op_hals_sweeps_f64"):
        assert hasattr(lib, name), name


def test_compute_refuses_bad_counts_before_the_device():
    import nmfgpu_amd as na
    assert na.initialize() in (na.ResultType.Success, na.ResultType.ErrorAlreadyInitialized)
    na.set_verbosity(na.Verbosity.Nothing)
    try:
        rng = np.random.default_rng(0)
        m, n, r = 20, 12, 3
        V = mc.F(rng.random((m, n)).astype(np.float32))
        W, H = mc.F(rng.random((m, r)).astype(np.float32)), mc.F(rng.random((r, n)).astype(np.float32))
        W0, H0 = W.copy(), H.copy()
        bad = na.ResultType.ErrorInvalidArgument
        hals = dict(algorithm=na.NmfAlgorithm.HALS, iterations=3)
        for name in ("sweepsH", "sweepsW"):
            for value in (2.5, 0, 65, -1, float("nan"), float("inf"), 1e300):
                assert na.compute(V, W, H, parameters={name: value}, **hals) == bad, (name, value)
            assert na.compute(V, W, H, iterations=3, parameters={name: 2}) == bad, name                      # Multiplicative
            assert na.compute(V, W, H, iterations=3, parameters={name: 2, "divergence": 2}) == bad, name     # a dense divergence engine
            assert na.compute(V, W, H, iterations=3, algorithm=na.NmfAlgorithm.ALS, parameters={name: 2}) == bad, name
        assert np.array_equal(W, W0) and np.array_equal(H, H0)
        if na.device_count() == 0:
            ok = na.ResultType.ErrorExternalLibrary      # the valid forms get as far as the device
            assert na.compute(V, W, H, parameters={"sweepsH": 3, "sweepsW": 2}, **hals) == ok
            assert na.compute(V, W, H, parameters={"sweepsH": 64, "sweepsW": 1, "l1H": 0.5}, **hals) == ok
            assert na.compute(V, W, H, iterations=3, parameters={"sweepsH": 1, "sweepsW": 1}) == ok
    finally:
        na.finalize()
