"""The mixed-precision dense divergence update without a GPU (docs/DIVERGENCE.md, "Mixed precision"): the restatement's rounding helper on hand-picked patterns, the
derived componentwise bound of one bf16-operand update against the exact update, and the two-run figures (the emulating restatement with fp32 against fp64
accumulation) that tests/test_gpu_beta_mixed.py takes its tolerances from (tests/beta_mixed_cases.py holds them; here every one is recomputed).

Figures on this machine's numpy: one half-step, panel by norm at most 3.1e-6 (7.9e-5 componentwise), per-row terms 6.3e-8; twenty iterations, factors 8.2e-4, errors
3.3e-5; the emulating restatement's divergence value against the exact restatement's 7.4e-5; one bf16-operand update against the exact one componentwise at most
1.2e-3, where the derived bound is 0.8 - 2.1e-2."""
import numpy as np
import pytest

from tests import beta_general_reference as gen
from tests import beta_mixed_cases as C
from tests import beta_mixed_reference as mix


def f32(bits):
    return np.array([bits], np.uint32).view(np.float32)


def bits_of(x):
    return int(np.asarray(x, np.float32).reshape(1).view(np.uint32)[0])


@pytest.mark.parametrize("pattern,want", [
    (0x3F800000, 0x3F800000),      # 1.0: exact values unchanged
    (0x3F808000, 0x3F800000),      # a tie above an even mantissa: down
    (0x3F818000, 0x3F820000),      # a tie above an odd mantissa: up
    (0x3F808001, 0x3F810000),      # just above the tie: up
    (0x3F807FFF, 0x3F800000),      # just below the tie: down
    (0x3FFF8000, 0x40000000),      # a tie that carries into the exponent
    (0x00000000, 0x00000000),      # 0
    (0x34000000, 0x34000000),      # 2^-23, the engine's eps
    (0x43800000, 0x43800000),      # 256
    (0x43808000, 0x43800000),      # 257 is a tie between 256 and 258: to even
    (0xBF818000, 0xBF820000),      # the sign is kept
])
def test_rounding_patterns(pattern, want):
    assert bits_of(mix.round_bf16(f32(pattern))) == want
    assert bits_of(mix.round_bf16(f32(pattern).astype(np.float64))) == want      # (a float64 array holds the same values)


def test_rounding_properties():
    rng = np.random.default_rng(1)
    x = rng.standard_normal(20000).astype(np.float32) * np.float32(2.0) ** rng.integers(-20, 20, 20000).astype(np.float32)
    y = mix.round_bf16(x)
    assert y.dtype == x.dtype and np.all((y.view(np.uint32) & 0xFFFF) == 0)
    assert np.all(np.abs(y.astype(np.float64) - x) <= np.abs(x.astype(np.float64)) * 2.0 ** -8)      # (8 significant bits: half an ulp is at most 2^-8 of the value)
    assert np.array_equal(mix.round_bf16(y), y)
    ints = np.arange(0, 257, dtype=np.float32)
    assert np.array_equal(mix.round_bf16(ints), ints)      # what the exact-data GPU test relies on


# one update with bf16 operands against the exact update, componentwise, at the shapes of the GPU test
@pytest.mark.parametrize("RP", C.RPS)
def test_derived_bound(RP):
    A, B, X = C.valid(*C.half_step_case(RP, 71 + RP), np.float64)
    for beta in (-1.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0):
        exact = gen.half_step(X, A, B, beta, C.EPS32)
        got = mix.half_step(X, A, B, beta, C.EPS32)
        worst = float(np.max(np.abs(got / exact - 1)))
        print(f"RP {RP} beta {beta}: componentwise {worst:.2e} (norm {C.rel(got, exact):.2e}) bound {C.derived_bound(beta):.2e}")
        assert worst < C.derived_bound(beta)
        assert worst > 2.0 ** -14      # (the roundings are there: the update is not the exact one)


def two_runs_half_step():
    panel = terms = 0.0
    for RP in C.RPS:
        case = C.half_step_case(RP, 71 + RP)
        for beta in C.HALF_STEP_BETAS:
            for l1, l2 in C.HALF_STEP_PENALTIES:
                out = {}
                for dt in (np.float32, np.float64):
                    A, B, X = C.valid(*case, dt)
                    out[dt] = (mix.half_step(X, A, B, beta, dt(C.EPS32), float(np.float32(l1)), float(np.float32(l2))),) + mix.terms(X, A, B, beta, dt(C.EPS32))
                panel = max(panel, C.rel(out[np.float32][0], out[np.float64][0]))
                terms = max(terms, C.rel(out[np.float32][1], out[np.float64][1]), C.rel(out[np.float32][2], out[np.float64][2]))
    return panel, terms


def recorded(constant, found):
    """A recorded figure is the largest found, rounded up: never below it, and not inflated."""
    return found <= constant <= 1.5 * found


def test_figures_of_one_half_step():
    panel, terms = two_runs_half_step()
    print(f"one half-step, fp32 against fp64 accumulation: panel {panel:.2e} terms {terms:.2e}")
    assert recorded(C.FIGURE_HALF_STEP_PANEL, panel), panel
    assert terms < C.TOL_HALF_STEP_TERMS / 100      # (the standing figure the terms are held to is far above the accumulation's share)


def test_figures_of_twenty_iterations():
    factors = errors = vs_exact = 0.0
    for r in C.ENGINE_RANKS:
        for beta in C.ENGINE_BETAS:
            a, b = C.emulated_run(r, beta, np.float32), C.emulated_run(r, beta, np.float64)
            V, W0, H0 = C.engine_problem(r, beta)
            exact = gen.run(V.astype(np.float64), W0.astype(np.float64), H0.astype(np.float64), C.ENGINE_ITERS, beta, C.EPS32)
            factors = max(factors, C.rel(a[0], b[0]), C.rel(a[1], b[1]))
            errors = max(errors, *(abs(a[i] / b[i] - 1) for i in (2, 3, 4)))
            vs_exact = max(vs_exact, abs(b[4] / exact[4] - 1))
            assert C.rel(b[0], exact[0]) < 5e-3 and C.rel(b[1], exact[1]) < 5e-3      # (the mode stays near the exact iteration: a few 2^-9)
    print(f"20 iterations, fp32 against fp64 accumulation: factors {factors:.2e} errors {errors:.2e}; divergence value against the exact run {vs_exact:.2e}")
    assert recorded(C.FIGURE_ENGINE_FACTORS, factors), factors
    assert recorded(C.FIGURE_ENGINE_ERRORS, errors), errors
    assert recorded(C.FIGURE_ENGINE_DIVERGENCE_VS_EXACT, vs_exact), vs_exact


def test_exact_case_is_exact():
    """The data of the exact-data GPU test: every operand is a bf16 value and the restatement's update at beta = 2 does not depend on the accumulation dtype."""
    for RP in C.RPS:
        case = C.exact_case(RP, 500 + RP)
        A, B, X = C.valid(*case, np.float64)
        P = A @ B.T
        assert P.min() >= 1 and P.max() <= 256 and np.array_equal(mix.round_bf16(P), P) and np.array_equal(mix.round_bf16(X), X)
        assert (X @ B).max() < 2 ** 24 and (P @ B).max() < 2 ** 24
        want = mix.half_step(X, A, B, 2.0, C.EPS32)
        assert np.array_equal(mix.round_bf16(P + C.EPS32), P)
        A32, B32, X32 = C.valid(*case, np.float32)
        got = mix.half_step(X32, A32, B32, 2.0, np.float32(C.EPS32))
        assert np.max(np.abs(got[want > 0] / want[want > 0] - 1)) < 4 * 2.0 ** -23
