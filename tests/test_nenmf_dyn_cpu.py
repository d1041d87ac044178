"""Per-column dynamic stopping of NeNMF's steps without a GPU (docs/NENMF.md, "Dynamic stopping"): that the inputs of the GPU tests (tests/nenmf_dyn_cases.py)
still show what those tests rely on, the figures their fp32 tolerances come from, self-checks of the restatement (tests/nenmf_dyn_reference.py) -- among them
that it tells the rule from its likely mistakes -- and the interface as far as it goes without a device."""
import collections

import numpy as np
import pytest

from tests import hals_multi_cases as mc
from tests import nenmf_cases as nc
from tests import nenmf_dyn_cases as dc
from tests import nenmf_dyn_reference as dyn
from tests import nenmf_reference as nenmf

CASES = [pytest.param(c, id=dc.case_id(c)) for c in dc.STEP_CASES]


# ------------------------------------------------------------------ 1. the inputs

def test_the_cases_are_the_ones_the_kernel_can_go_wrong_at():
    assert (dc.LEN_PAD, dc.LEN_VALID, dc.TOL, dc.MAX_STEPS) == (128, 100, 0.1, 12) and dc.PENALTIES == ((0.0, 0.0), (0.05, 0.01)) and dc.FLIP_CAP == 0.98
    for dtype, rps in nc.INSTANTIATIONS.items():
        mine = [c for c in dc.STEP_CASES if c[0] == dtype]
        assert {(c[1], c[2]) for c in mine} == {(64, 5), (64, 61), (64, 64), (128, 125), (128, 128)}
        assert {c[3] for c in mine} == {1, 3}
        assert dc.EARLY_FROM % dc.TILE[dtype] == 0
    assert dc.ENGINE_SHAPES == ((131, 97, 9), (200, 150, 70)) and dc.ENGINE_TOL == 0.1 and dc.ENGINE_STEPS == (12, 12)


@pytest.mark.parametrize("case", CASES)
def test_inputs_are_diverse_and_fp32_stays_under_the_flip_cap(case):
    """G >= 0 entrywise; the fp64 counts of every case are diverse (at r >= RP - 3: 1, 2, 4, 8 or 9 and 12, twenty columns at the maximum and every workgroup from
    column 64 on below it); an fp32 numpy run of the rule agrees with them on at least FLIP_CAP of the columns; the loose and the tight tolerance give what the
    workgroup-exit and the static-bits check of the GPU test need."""
    dtype, RP, r, S = case
    for l1, l2 in dc.PENALTIES:
        P, slabs, G = dc.step_case(case, l1, l2)
        assert (G >= 0).all() and (G == G.T).all() and not G[r:].any() and not G[:, r:].any()
        assert not P[dc.LEN_VALID:].any() and not slabs[:, dc.LEN_VALID:].any() and not P[:, r:].any()
        _, counts = dc.restated(case, l1, l2)
        hist = dict(collections.Counter(counts.tolist()))
        print(dc.case_id(case), (l1, l2), sorted(hist.items()))
        assert dc.diversity_faults(case, counts) == []
        if r >= RP - 3:
            assert hist == {1: 23, 2: 19, 4: 34, (8 if l1 else 9): 4, 12: 20}, hist
        else:
            assert max(hist) < dc.MAX_STEPS
        _, c32 = dyn.panel_steps_dyn(P, slabs, G, r, dc.LEN_VALID, dc.MAX_STEPS, dc.TOL, l1, l2, dtype=np.float32)
        assert float((c32 == counts).mean()) >= dc.FLIP_CAP
        _, loose = dyn.panel_steps_dyn(P, slabs, G, r, dc.LEN_VALID, dc.LOOSE_MAX, dc.LOOSE_TOL, l1, l2, dtype=dtype)
        assert dict(collections.Counter(loose.tolist())) == {1: 23, 2: 77}
        _, tight = dyn.panel_steps_dyn(P, slabs, G, r, dc.LEN_VALID, dc.TIGHT_MAX, dc.TIGHT_TOL, l1, l2, dtype=dtype)
        assert int((tight == dc.TIGHT_MAX).sum()) == 77 and 2 * 77 >= dc.LEN_VALID


def test_the_valid_block_does_not_depend_on_len_pad():
    case = dc.STEP_CASES[1]
    a, b = dc.step_case(case), dc.step_case(case, len_pad=256)
    assert b[0].shape[0] == 256 and np.array_equal(a[0], b[0][:128]) and np.array_equal(a[1], b[1][:, :128]) and np.array_equal(a[2], b[2])
    P, slabs, G = dc.step_case(dc.ZERO_G_CASE, zero_g=True)
    assert not G.any() and P.any()
    got, counts = dyn.panel_steps_dyn(P, slabs, G, dc.ZERO_G_CASE[2], dc.LEN_VALID, 5, 0.1)
    assert np.array_equal(got, P[:dc.LEN_VALID, :dc.ZERO_G_CASE[2]]) and not counts.any(), "L <= 0: no step, counts 0"


# ------------------------------------------------------------------ 2. the figures

def test_step_figure_is_what_the_restatements_give():
    """FIGURE_STEPS: the largest norm-relative distance of the fp32 numpy restatement from the fp64 one, at the fp64 counts, over the fp32 step cases; held to
    [found, 1.5 x found]."""
    found = max(dc.step_fp32_figure(case, l1, l2) for case in dc.STEP_CASES if case[0] == np.float32 for l1, l2 in dc.PENALTIES)
    print("found", found, "recorded", dc.FIGURE_STEPS)
    assert found <= dc.FIGURE_STEPS <= 1.5 * found, (found, dc.FIGURE_STEPS)
    assert dc.MARGIN == 4.0 and dc.TOL_F64 == 1e-9


def test_engine_figure_is_what_the_restatements_give():
    """FIGURE_ENGINE_FACTORS: the same for W and H over the engine shapes and kinds after 1 and 5 iterations."""
    found = 0.0
    for shape in dc.ENGINE_SHAPES:
        for kind in dc.ENGINE_KINDS:
            for iters in dc.ENGINE_ITERS:
                w, h = dc.engine_fp32_figure(shape, kind, iters)
                print(shape, kind, iters, "W", w, "H", h)
                found = max(found, w, h)
    print("found", found, "recorded", dc.FIGURE_ENGINE_FACTORS)
    assert found <= dc.FIGURE_ENGINE_FACTORS <= 1.5 * found, (found, dc.FIGURE_ENGINE_FACTORS)
    assert dc.ENGINE_ITERS == (1, 5) and dc.ENGINE_KINDS == ("plain", "pen", "constw", "sparse")


# ------------------------------------------------------------------ 3. the restatement

@pytest.mark.parametrize("case", CASES)
def test_forced_maximum_is_the_static_restatement(case):
    """forced = T on every column: nenmf_reference.panel_steps at T, bit for bit, in both dtypes; so is a tolerance of 0."""
    r = case[2]
    for l1, l2 in dc.PENALTIES:
        P, slabs, G = dc.step_case(case, l1, l2)
        for dtype in (np.float64, np.float32):
            for T in (1, 5, dc.MAX_STEPS):
                want, _ = nenmf.panel_steps(P, slabs, G, r, dc.LEN_VALID, T, l1, l2, dtype=dtype)
                got, counts = dyn.panel_steps_dyn(P, slabs, G, r, dc.LEN_VALID, T, dc.TOL, l1, l2, dtype=dtype, forced=np.full(dc.LEN_VALID, T))
                assert np.array_equal(got, want) and (counts == T).all()
                got, counts = dyn.panel_steps_dyn(P, slabs, G, r, dc.LEN_VALID, T, 0.0, l1, l2, dtype=dtype)
                assert np.array_equal(got, want) and (counts == T).all()


@pytest.mark.parametrize("case", CASES)
def test_the_rule_is_per_column(case):
    """Permuting the columns permutes results and counts, and a column alone gives what it gives in the panel (values to the rounding of another product shape)."""
    r = case[2]
    P, slabs, G = dc.step_case(case, *dc.PENALTIES[1])
    want, counts = dc.restated(case, *dc.PENALTIES[1])
    perm = np.random.default_rng(5).permutation(dc.LEN_VALID)
    Pp, sp = P.copy(), slabs.copy()
    Pp[:dc.LEN_VALID] = P[perm]
    sp[:, :dc.LEN_VALID] = slabs[:, perm]
    got, cp = dyn.panel_steps_dyn(Pp, sp, G, r, dc.LEN_VALID, dc.MAX_STEPS, dc.TOL, *dc.PENALTIES[1])
    assert np.array_equal(cp, counts[perm]) and dc.rel(got, want[perm]) < 1e-14
    for y in (0, 1, 2, 3, 66):
        one, c1 = dyn.panel_steps_dyn(P[y:y + 1], slabs[:, y:y + 1], G, r, 1, dc.MAX_STEPS, dc.TOL, *dc.PENALTIES[1])
        assert c1[0] == counts[y] and dc.rel(one[0], want[y]) < 1e-14


@pytest.mark.parametrize("case", CASES)
def test_a_frozen_column_is_untouched_by_further_steps(case):
    """A larger maximum changes only the columns that were at the maximum: a column frozen after t steps has the value and the count it had, bit for bit; and its
    value is that of the static restatement at t steps."""
    r = case[2]
    P, slabs, G = dc.step_case(case)
    a, ca = dc.restated(case, 0.0, 0.0)
    b, cb = dyn.panel_steps_dyn(P, slabs, G, r, dc.LEN_VALID, 2 * dc.MAX_STEPS, dc.TOL)
    frozen = ca < dc.MAX_STEPS
    assert frozen.any() and np.array_equal(a[frozen], b[frozen]) and np.array_equal(ca[frozen], cb[frozen])
    assert (cb[~frozen] >= dc.MAX_STEPS).all()
    for t in sorted(set(ca.tolist())):
        static, _ = nenmf.panel_steps(P, slabs, G, r, dc.LEN_VALID, t)
        assert np.array_equal(a[ca == t], static[ca == t])


@pytest.mark.parametrize("case", CASES)
def test_the_bound_on_the_projected_gradient(case):
    """On every column the norm of the projected gradient of the penalised subproblem at the result is at most 2 L sqrt(d_last) (docs/NENMF.md)."""
    r = case[2]
    for l1, l2 in dc.PENALTIES:
        P, slabs, G = dc.step_case(case, l1, l2)
        A = dyn.panel_rhs(slabs, r, dc.LEN_VALID)
        out, counts, d_last, L = dyn.apg_dyn(P[:dc.LEN_VALID, :r].T, A.T, G[:r, :r], dc.MAX_STEPS, dc.TOL, l1, l2, give_d=True)
        pg = dyn.projected_gradient_norm(out, A.T, G[:r, :r], l1, l2)
        bound = 2.0 * L * np.sqrt(d_last)
        assert (pg <= bound * (1 + 1e-9) + 1e-13).all(), float((pg - bound).max())
        assert (pg[counts > 1] > 0).any()


MISTAKES = {
    "d measured against P_t": dict(d_against_p=True),
    "threshold from d_(t-1)": dict(threshold_from_previous=True),
    "frozen column still extrapolated": dict(extrapolate_frozen=True),
}


@pytest.mark.parametrize("case", CASES)
def test_the_restatement_tells_the_rule_from_its_mistakes(case):
    """Each mistake changes the counts of more columns than the rule check admits (1 - FLIP_CAP), or -- the extrapolated frozen column, whose counts are the
    rule's -- moves the values by more than 10 x the GPU tolerance of the case."""
    r = case[2]
    tol = dc.step_tolerance(case)
    for l1, l2 in dc.PENALTIES:
        P, slabs, G = dc.step_case(case, l1, l2)
        want, counts = dc.restated(case, l1, l2)
        for name, switch in MISTAKES.items():
            got, c = dyn.panel_steps_dyn(P, slabs, G, r, dc.LEN_VALID, dc.MAX_STEPS, dc.TOL, l1, l2, **switch)
            differ = float((c != counts).mean())
            print(dc.case_id(case), (l1, l2), name, "counts differ on", differ, "values", dc.rel(got, want))
            if name == "frozen column still extrapolated":
                assert np.array_equal(c, counts) and dc.rel(got, want) > 10 * tol, (name, dc.rel(got, want))
            else:
                assert differ > 1 - dc.FLIP_CAP, (name, differ)


def test_iteration_at_forced_maximum_is_the_static_iteration():
    for kind in ("plain", "pen", "constw"):
        _, V, W, H, p, constant_w = dc.engine_problem(131, 97, 9, np.float64, kind)
        W1, H1, errs = nenmf.run(V, W, H, 3, 4, 3, p, constant_w)
        forced = [(np.full(97, 4), np.full(131, 3))] * 3
        W2, H2, errs2, counts = dyn.run(V, W, H, 3, 4, 3, 0.1, p, constant_w, forced=forced)
        assert np.array_equal(W1, W2) and np.array_equal(H1, H2) and errs == errs2
        assert all((ch == 4).all() and (constant_w or (cw == 3).all()) for ch, cw in counts)
    _, V, W, H, p, _ = dc.engine_problem(131, 97, 9, np.float64)
    _, _, _, counts = dyn.run(V, W, H, 2, *dc.ENGINE_STEPS, dc.ENGINE_TOL)
    assert all(c.min() >= 1 and c.max() <= 12 for pair in counts for c in pair)
    assert all(len(set(c.tolist())) >= 5 for c in counts[0]), "the first iteration of the engine problems has diverse counts (later ones run to the maximum)"


# ------------------------------------------------------------------ 4. the interface, no device needed

def test_library_exports_the_new_entries():
    from nmfgpu_amd import _lib
    import nmfgpu_amd as na
    lib = _lib.library()
    for name in ("nmfamd_engine_set_nenmf_step_tolerance", "nmfamd_engine_nenmf_step_counts", "nmfamd_op_apg_steps_dyn_f32", "nmfamd_op_apg_steps_dyn_f64"):
        assert hasattr(lib, name), name
    assert callable(na.op_apg_steps_dyn) and callable(na.Engine.set_step_tolerance) and callable(na.Engine.step_counts)


def test_compute_refuses_bad_tolerances_before_the_device():
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
        nen = dict(algorithm=na.NmfAlgorithm.NeNMF, iterations=3)
        for value in (-0.1, -1e-300, 1.0, 1.5, float("nan"), float("inf"), -float("inf")):
            assert na.compute(V, W, H, parameters={"stepsTolerance": value}, **nen) == bad, value
        assert na.compute(V, W, H, iterations=3, parameters={"stepsTolerance": 0.1}) == bad                       # Multiplicative
        assert na.compute(V, W, H, iterations=3, algorithm=na.NmfAlgorithm.HALS, parameters={"stepsTolerance": 0.1}) == bad
        assert na.compute(V, W, H, iterations=3, algorithm=na.NmfAlgorithm.ALS, parameters={"stepsTolerance": 0.5}) == bad
        assert na.compute(V, W, H, parameters={"stepsTolerance": 0.1, "sweepsTolerance": 0.1}, **nen) == bad
        assert np.array_equal(W, W0) and np.array_equal(H, H0)
        if na.device_count() == 0:
            ok = na.ResultType.ErrorExternalLibrary      # the valid forms get as far as the device
            assert na.compute(V, W, H, parameters={"stepsTolerance": 0.1}, **nen) == ok
            assert na.compute(V, W, H, parameters={"stepsTolerance": 0.0}, **nen) == ok
            assert na.compute(V, W, H, parameters={"stepsTolerance": 0.999, "stepsH": 256, "stepsW": 1}, **nen) == ok
            assert na.compute(V, W, H, iterations=3, parameters={"stepsTolerance": 0.0}) == ok                    # absent means 0: another algorithm takes 0
    finally:
        na.finalize()
