"""The cases and the figures that tests/test_gpu_nenmf_steps.py, tests/test_gpu_nenmf.py and tests/test_nenmf_cpu.py share (docs/NENMF.md), in the manner of
tests/hals_multi_cases.py, whose problems and helpers the engine level reuses.

Step level: every instantiated (dtype, RP) of k_apg_steps at r = previous RP + 1, RP - 1 and RP; len_valid rotates over 1, tile - 1, tile + 1 and LEN_PAD - 1 (tile:
the kernel's columns per workgroup), S over 1 and 3.  Every case runs at 1, 2 and 5 steps (none, one and several extrapolations), plain and penalised.

Engine level: (steps_h, steps_w) = (5, 3) against tests/nenmf_reference.py after 1 and 10 iterations, on the kinds and shapes of hals_multi_cases.ENGINE_CASES that
the instantiated ranks cover.

Tolerances: fp64 1e-9, the project's standing figure.  fp32: MARGIN x a figure, the largest norm-relative distance of the restatement run in fp32 numpy from its
fp64 run over the test's own fp32 cases -- one figure for the step level, one for the engine level; tests/test_nenmf_cpu.py recomputes both and fails if a constant
is smaller than what it finds or more than 1.5 times larger.
"""
import numpy as np

from tests import hals_multi_cases as mc
from tests import nenmf_reference as nenmf

LEN_PAD = 256
INSTANTIATIONS = {np.float32: [64, 128], np.float64: [64, 128]}
TILE = {np.float32: 32, np.float64: 16}            # panel columns per workgroup (ApgGeom::COLS)
STEP_COUNTS = (1, 2, 5)
STEP_PENALTIES = ((0.0, 0.0), (0.05, 0.01))         # (l1, l2)
MARGIN = 4.0
TOL_F64 = 1e-9
F, rel = mc.F, mc.rel


def _step_cases():
    """(dtype, RP, r, len_valid, S)"""
    out = []
    for dtype, rps in INSTANTIATIONS.items():
        prev = 0
        lvs = [1, TILE[dtype] - 1, TILE[dtype] + 1, LEN_PAD - 1]
        for RP in rps:
            for r in (prev + 1, RP - 1, RP):
                i = len(out)
                out.append((dtype, RP, r, lvs[i % 4], (1, 3)[(i + i // 4) % 2]))
            prev = RP
    return out


STEP_CASES = _step_cases()
ZERO_G_CASE = (np.float32, 64, 33, 40, 1)           # G = 0: L <= 0, the panel keeps its values


def case_id(case):
    dtype, RP, r, lv, S = case
    return f"{np.dtype(dtype).name}-RP{RP}-r{r}-len{lv}-S{S}"


def case_rng(case, salt=0):
    return np.random.default_rng(case[1] * 1000 + case[2] + 7000 + salt)


def step_problem(case, zero_g=False):
    """(P, slabs, G) in panel layout (P (LEN_PAD, RP), slabs (S, LEN_PAD, RP), G (RP, RP)), zero on the padding.  G = M^T M of a non-negative M, scaled so that its
    largest row sum is 1: then l2 = 0.01 is 1 % of L and l1 = 0.05 a tenth of a typical entry of a, and a mistake in either shows.  a = G x + noise for a half-empty
    x >= 0 (so that the clamp is active), split over the slabs at random; the old panel uniform in [0, 1)."""
    dtype, RP, r, len_valid, S = case
    rng = case_rng(case)
    M = rng.random((r + 16, r))
    Gr = M.T @ M
    Gr /= Gr.sum(axis=1).max()
    G = np.zeros((RP, RP))
    if not zero_g:
        G[:r, :r] = Gr
    x = rng.random((len_valid, r)) * (rng.random((len_valid, r)) < 0.5)
    A = np.zeros((LEN_PAD, RP))
    A[:len_valid, :r] = x @ Gr + 0.05 * rng.uniform(-1.0, 1.0, size=(len_valid, r))
    P = np.zeros((LEN_PAD, RP))
    P[:len_valid, :r] = rng.random((len_valid, r))
    slabs = np.zeros((S, LEN_PAD, RP))
    for s in range(S - 1):
        slabs[s + 1] = rng.uniform(-0.5, 0.5, size=(LEN_PAD, RP)) * (A != 0)
    slabs[0] = A - slabs[1:].sum(axis=0)
    return P.astype(dtype), slabs.astype(dtype), G.astype(dtype)


_STEPS = {}


def restated_steps(case, T, l1, l2):
    """((len_valid, r) block after T fp64 steps, the fp64 sums of the slabs of that block) -- cached: the tests share one result and nobody changes it."""
    key = (case_id(case), T, l1, l2)
    if key not in _STEPS:
        P, slabs, G = step_problem(case)
        _STEPS[key] = nenmf.panel_steps(P, slabs, G, case[2], case[3], T, l1, l2)
    return _STEPS[key]


def step_fp32_figure(case, T, l1, l2):
    P, slabs, G = step_problem(case)
    got, _ = nenmf.panel_steps(P, slabs, G, case[2], case[3], T, l1, l2, dtype=np.float32)
    return rel(got, restated_steps(case, T, l1, l2)[0])


# the largest norm-relative distance of the fp32 numpy steps from the fp64 ones over the fp32 STEP_CASES x STEP_COUNTS x STEP_PENALTIES
FIGURE_STEPS = 3.3e-7      # (found: 3.06e-7, RP 64, r = 63, 5 penalised steps; one step stays below 1.8e-7)


def step_tolerance(case):
    return TOL_F64 if case[0] == np.float64 else MARGIN * FIGURE_STEPS


# ------------------------------------------------------------------ engine level

STEPS_H, STEPS_W = 5, 3
ENGINE_ITERS = (1, 10)
# (kind, m, n, r, dtype) as hals_multi_cases.ENGINE_CASES, without the ranks above 128 (no step kernel: docs/NENMF.md)
ENGINE_CASES = [
    ("dense", 500, 300, 7, np.float32), ("dense", 500, 300, 33, np.float32), ("dense", 300, 257, 70, np.float32),
    ("dense", 500, 300, 7, np.float64), ("dense", 500, 300, 33, np.float64), ("dense", 300, 257, 70, np.float64),
    ("sparse", 300, 257, 70, np.float32), ("sparse", 300, 257, 70, np.float64),
    ("pen", 300, 257, 70, np.float32), ("pen", 300, 257, 70, np.float64),
    ("constw", 500, 300, 33, np.float32), ("constw", 500, 300, 33, np.float64),
]
FIGURE_ENGINE_FACTORS = 8.0e-6      # (found: 7.30e-6, H of the constant-W case after 10 iterations; the dense cases stay below 4.3e-6)
engine_case_id, engine_problem = mc.engine_case_id, mc.engine_problem

_RUNS = {}


def restated(case, iters):
    """(W, H, errors) of the fp64 restatement at (STEPS_H, STEPS_W) after `iters` iterations (cached)."""
    key = (engine_case_id(case), iters)
    if key not in _RUNS:
        _, V, W, H, penalties, constant_w = engine_problem(case)
        _RUNS[key] = nenmf.run(np.asarray(V, np.float64), W, H, iters, STEPS_H, STEPS_W, penalties, constant_w)
    return _RUNS[key]


def engine_fp32_figure(case, iters):
    """The norm-relative distances (W, H) of the fp32 numpy restatement from the fp64 one on an fp32 engine case."""
    _, V, W, H, penalties, constant_w = engine_problem(case)
    W32, H32 = nenmf.run_in(V, W, H, iters, STEPS_H, STEPS_W, np.float32, penalties, constant_w)
    W64, H64, _ = restated(case, iters)
    return rel(W32, W64), rel(H32, H64)


def engine_tolerance(case):
    return TOL_F64 if case[4] == np.float64 else MARGIN * FIGURE_ENGINE_FACTORS
