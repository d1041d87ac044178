"""NeNMF without a GPU (docs/NENMF.md): the figures the GPU tests take their fp32 tolerances from, that those tolerances can tell the likely mistakes from the
algorithm, self-checks of the restatement (tests/nenmf_reference.py), and the interface as far as it goes without a device."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import hals_multi_cases as mc
from tests import hals_multi_reference as multi
from tests import nenmf_cases as nc
from tests import nenmf_reference as nenmf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ 1. the figures

def test_step_figure_is_what_the_restatements_give():
    """FIGURE_STEPS: the largest norm-relative distance of the fp32 numpy steps from the fp64 ones over the fp32 step cases, held to [found, 1.5 x found]."""
    found = 0.0
    for case in nc.STEP_CASES:
        if case[0] != np.float32:
            continue
        for T in nc.STEP_COUNTS:
            for l1, l2 in nc.STEP_PENALTIES:
                found = max(found, nc.step_fp32_figure(case, T, l1, l2))
    print("found", found, "recorded", nc.FIGURE_STEPS)
    assert found <= nc.FIGURE_STEPS <= 1.5 * found, (found, nc.FIGURE_STEPS)
    assert nc.MARGIN == 4.0 and nc.TOL_F64 == 1e-9


def test_engine_figure_is_what_the_restatements_give():
    """FIGURE_ENGINE_FACTORS: the same over the fp32 engine cases at (5, 3) after 1 and 10 iterations, W and H."""
    found = 0.0
    for case in nc.ENGINE_CASES:
        if case[4] != np.float32:
            continue
        for iters in nc.ENGINE_ITERS:
            w, h = nc.engine_fp32_figure(case, iters)
            print(nc.engine_case_id(case), iters, "W", w, "H", h)
            found = max(found, w, h)
    print("found", found, "recorded", nc.FIGURE_ENGINE_FACTORS)
    assert found <= nc.FIGURE_ENGINE_FACTORS <= 1.5 * found, (found, nc.FIGURE_ENGINE_FACTORS)
    assert (nc.STEPS_H, nc.STEPS_W) == (5, 3) and nc.ENGINE_ITERS == (1, 10)


def test_the_cases_are_the_ones_the_kernel_can_go_wrong_at():
    assert nc.LEN_PAD == 256 and nc.STEP_COUNTS == (1, 2, 5) and nc.STEP_PENALTIES == ((0.0, 0.0), (0.05, 0.01))
    for dtype, rps in nc.INSTANTIATIONS.items():
        tile = nc.TILE[dtype]
        mine = [c for c in nc.STEP_CASES if c[0] == dtype]
        prev = 0
        for RP in rps:
            assert {c[2] for c in mine if c[1] == RP} == {prev + 1, RP - 1, RP}
            prev = RP
        assert {c[3] for c in mine} == {1, tile - 1, tile + 1, 255}
        assert {c[4] for c in mine} == {1, 3}
    assert any(c[2] == 1 for c in nc.STEP_CASES)
    P, slabs, G = nc.step_problem(nc.ZERO_G_CASE, zero_g=True)
    assert not G.any() and P.any()
    got, _ = nenmf.panel_steps(P, slabs, G, nc.ZERO_G_CASE[2], nc.ZERO_G_CASE[3], 5)
    assert np.array_equal(got, P[:nc.ZERO_G_CASE[3], :nc.ZERO_G_CASE[2]]), "L <= 0 leaves the panel as it is"
    assert nenmf.momentum(3)[0] == 0.0 and 0.28 < nenmf.momentum(3)[1] < 0.29       # (alpha_0 - 1) / alpha_1 = 0;  (alpha_1 - 1) / alpha_2 = 0.2818...


# ------------------------------------------------------------------ 2. telling mistakes apart

MISTAKES = {
    "one step fewer": None,
    "no momentum": dict(with_momentum=False),
    "Y returned instead of P": dict(give_y=True),
    "L without l2": dict(l2_in_L=False),
    "l1 dropped": dict(l1_in_gradient=False),
}


def applies(name, case, T, l1, l2):
    """Where a mistake changes the result at all.  The penalty mistakes need penalties.  The coefficient of the first extrapolation is (alpha_0 - 1) / alpha_1 = 0, so
    at 2 steps there is no momentum to lose: that mistake is looked for at the counts with a non-zero coefficient (5).  At r = 1 the step is the exact solution of the
    one-dimensional problem (L = G_11 + l2 is the curvature itself), every later step finds nothing left to do, and only a mistake in the gradient shows."""
    if name in ("L without l2", "l1 dropped") and l1 == 0 and l2 == 0:
        return False
    if name == "no momentum" and T < 3:
        return False
    if case[2] == 1 and name != "l1 dropped":
        return False
    return True


@pytest.mark.parametrize("case", [pytest.param(c, id=nc.case_id(c)) for c in nc.STEP_CASES])
def test_every_mistake_lies_outside_ten_tolerances(case):
    """At every step-level case with 2 or more steps each mistake is farther from the restatement than 10 x the GPU tolerance of that case."""
    dtype, RP, r, lv, S = case
    P, slabs, G = nc.step_problem(case)
    tol = nc.step_tolerance(case)
    for T in (t for t in nc.STEP_COUNTS if t >= 2):
        for l1, l2 in nc.STEP_PENALTIES:
            want, _ = nc.restated_steps(case, T, l1, l2)
            for name, switch in MISTAKES.items():
                if not applies(name, case, T, l1, l2):
                    continue
                wrong, _ = nenmf.panel_steps(P, slabs, G, r, lv, T - 1 if switch is None else T, l1, l2, **(switch or {}))
                d = nc.rel(wrong, want)
                assert d > 10 * tol, (name, T, (l1, l2), d, tol)


def test_the_exemptions_are_not_mistakes():
    """What `applies` leaves out gives the restatement's own result (to rounding): no momentum at 2 steps, and at r = 1 a step more or less."""
    case = next(c for c in nc.STEP_CASES if c[2] == 63 and c[0] == np.float32)
    P, slabs, G = nc.step_problem(case)
    same, _ = nenmf.panel_steps(P, slabs, G, case[2], case[3], 2, with_momentum=False)
    assert np.array_equal(same, nc.restated_steps(case, 2, 0.0, 0.0)[0])
    for one in (c for c in nc.STEP_CASES if c[2] == 1):
        P, slabs, G = nc.step_problem(one)
        for T in (2, 5):
            a, _ = nenmf.panel_steps(P, slabs, G, 1, one[3], T - 1)
            assert nc.rel(a, nc.restated_steps(one, T, 0.0, 0.0)[0]) < 1e-15


# ------------------------------------------------------------------ 3. the solver

def test_three_thousand_steps_solve_the_nnls():
    rng = np.random.default_rng(11)
    m, n, r = 40, 30, 5
    V, W, H0 = rng.random((m, n)), rng.random((m, r)), rng.random((r, n))
    G, A = W.T @ W, W.T @ V
    H = nenmf.apg(H0, A, G, 3000)
    grad = G @ H - A
    assert (H >= 0).all()
    assert np.abs(np.minimum(grad, 0.0)).max() <= 1e-8, "a negative gradient coordinate: not dual feasible"
    assert np.abs(H * grad).max() <= 1e-8, "complementary slackness"
    assert nc.rel(H, multi.sweeps(H0, A, G, None, 3000)) <= 1e-6


# ------------------------------------------------------------------ 4. the objective

@pytest.mark.parametrize("penalties", [(0.0, 0.0, 0.0, 0.0), mc.ENGINE_PENALTIES])
def test_objective_does_not_rise(penalties):
    V, W, H = mc.planted(300, 257, 70, np.float64, seed=3)
    before = nenmf.objective(V, W, H, penalties)
    first = before
    for _ in range(30):
        W, H, _ = nenmf.iteration(V, W, H, nc.STEPS_H, nc.STEPS_W, penalties)
        now = nenmf.objective(V, W, H, penalties)
        assert now <= before * (1 + 1e-12), (before, now)
        before = now
    assert before < 0.6 * first and (W >= 0).all() and (H >= 0).all()


# ------------------------------------------------------------------ 5. the interface, no device needed

def _probe(source: str) -> str:
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "probe.cpp"), os.path.join(td, "probe")
        open(src, "w").write(source)
        subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        return subprocess.check_output([exe]).decode().strip()


def test_the_id_is_seven_everywhere():
    import nmfgpu_amd.api as api
    import nmfgpu_amd.engine as engine
    assert engine.ALGORITHMS["nenmf"] == 7 and api.NmfAlgorithm.NeNMF == 7
    assert engine.ALGORITHMS["hals"] == 6 and api.NmfAlgorithm.HALS == 6
    assert _probe(r'''
#include <nmfgpu.h>
#include <cstdio>
int main() { printf("%d %d\n", (int)nmfgpu::NmfAlgorithm::HALS, (int)nmfgpu::NmfAlgorithm::NeNMF); return 0; }
''') == "6 7"
    assert _probe(r'''
#include <nmfgpu_amd.h>
#include <cstdio>
int main() { printf("%d %d\n", (int)NMFAMD_HALS, (int)NMFAMD_NENMF); return 0; }
''') == "6 7"


def test_library_exports_the_new_entries():
    from nmfgpu_amd import _lib
    lib = _lib.library()
    for name in ("nmfamd_engine_set_nenmf_steps", "nmfamd_op_apg_steps_f32", "nmfamd_op_apg_steps_f64"):
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
        nen = dict(algorithm=na.NmfAlgorithm.NeNMF, iterations=3)
        for name in ("stepsH", "stepsW"):
            for value in (2.5, 0, 257, -1, float("nan"), float("inf"), 1e300):
                assert na.compute(V, W, H, parameters={name: value}, **nen) == bad, (name, value)
            assert na.compute(V, W, H, iterations=3, parameters={name: 8}) == bad, name                       # Multiplicative
            assert na.compute(V, W, H, iterations=3, algorithm=na.NmfAlgorithm.HALS, parameters={name: 8}) == bad, name
        assert na.compute(V, W, H, parameters={"sweepsH": 2}, **nen) == bad
        assert na.compute(V, W, H, parameters={"sweepsTolerance": 0.1}, **nen) == bad
        assert na.compute(V, W, H, parameters={"numGpus": 2}, **nen) == bad
        assert na.compute(V, W, H, parameters={"divergence": 1}, **nen) == bad
        Wb, Hb = mc.F(rng.random((200, 129)).astype(np.float32)), mc.F(rng.random((129, 150)).astype(np.float32))
        assert na.compute(mc.F(rng.random((200, 150)).astype(np.float32)), Wb, Hb, **nen) == bad      # no step kernel above rank 128
        assert np.array_equal(W, W0) and np.array_equal(H, H0)
        if na.device_count() == 0:
            ok = na.ResultType.ErrorExternalLibrary      # the valid forms get as far as the device
            assert na.compute(V, W, H, **nen) == ok
            assert na.compute(V, W, H, parameters={"stepsH": 256, "stepsW": 1, "l1H": 0.5, "sweepsH": 1}, **nen) == ok
    finally:
        na.finalize()
