"""The inputs that tests/test_gpu_nenmf_dyn_steps.py, tests/test_gpu_nenmf_dyn.py and tests/test_nenmf_dyn_cpu.py share (docs/NENMF.md, "Dynamic stopping"), in
the manner of tests/hals_dyn_cases.py: the CPU test checks, without a device, every condition the GPU tests rely on.

Step level.  Every instantiated (dtype, RP) of k_apg_steps_dyn at len_pad = 128, len_valid = 100, r in {RP - 3, RP} (and r = 5 at RP 64), S in {1, 3}, plain and
penalised, delta = 0.1 with a maximum of 12 steps.  The input is built so that the fp64 restatement's counts are diverse (step_case):

  G is entrywise >= 0 (L is its largest row sum): a weak symmetric random coupling (largest row sum 0.01) and a diagonal set by up to four blocks of coordinates
  with the values DIAGONALS -- an error that lives in block b contracts under a plain step at about 1 - g_b / L.

  Columns come in the kinds of hals_dyn_cases.sweep_case.  "block b": the start is the interior solution x* > 0 of the column (a = (G + l2 I) x* + l1) plus a
  positive perturbation inside block b.  "far": every coordinate perturbed, each with a sign of its own.  "zero": start 0 and a < 0, a fixed point in every precision
  (every step clamps to exactly 0): count 1.  Columns below 64 mix all kinds; columns from 64 on (a tile boundary for 32 and for 16 columns per workgroup) hold
  only kinds that freeze early, so those workgroups take the early exit while the others run to the maximum.
"""
import numpy as np

from tests import hals_dyn_cases as hdc
from tests import hals_multi_cases as mc
from tests import hals_penalty_reference as pen
from tests import nenmf_cases as nc
from tests import nenmf_dyn_reference as dyn

LEN_PAD, LEN_VALID = 128, 100
TOL, MAX_STEPS = 0.1, 12
PENALTIES = ((0.0, 0.0), (0.05, 0.01))
DIAGONALS = {1: (1.0,), 2: (1.0, 0.1), 3: (1.0, 0.3, 0.05), 4: (1.0, 0.4, 0.12, 0.03)}
COUPLING = 0.01
FLIP_CAP = 0.98                                   # the rule check: counts equal for at least this share of the valid columns (hals_dyn_cases' figure)
EARLY_FROM = 64                                   # columns from here on hold only early-freezing kinds
EARLY_DIAGONAL = 0.3                              # ... blocks with at least this diagonal
MARGIN, TOL_F64 = nc.MARGIN, nc.TOL_F64
TILE = nc.TILE
rel = mc.rel

# (dtype, RP, r, S)
STEP_CASES = [(dtype, RP, r, (1, 3)[i % 2])
              for dtype, rps in nc.INSTANTIATIONS.items()
              for RP in rps
              for i, r in enumerate(([5] if RP == 64 else []) + [RP - 3, RP])]
ZERO_G_CASE = (np.float32, 64, 33, 1)


def case_id(case):
    dtype, RP, r, S = case
    return f"{np.dtype(dtype).name}-RP{RP}-r{r}-S{S}"


def blocks_of(r):
    """The coordinate ranges of the diagonal blocks of G and their diagonal values: min(4, r // 2) near-equal ranges."""
    nb = max(1, min(4, r // 2))
    edges = [round(i * r / nb) for i in range(nb + 1)]
    return [(edges[i], edges[i + 1]) for i in range(nb)], DIAGONALS[nb]


def step_case(case, l1=0.0, l2=0.0, len_pad=LEN_PAD, zero_g=False):
    """(P (len_pad, RP), slabs (S, len_pad, RP), G (RP, RP)) in the case's dtype, zero on all padding (the launch helper of the GPU test puts NaN there).  The
    valid block does not depend on len_pad."""
    dtype, RP, r, S = case
    rng = np.random.default_rng(RP * 1000 + r + 7 * S)
    blocks, diag = blocks_of(r)
    G = np.zeros((RP, RP))
    M = np.triu(rng.uniform(0.0, 1.0, size=(r, r)), 1)
    M = M + M.T
    G[:r, :r] = M * (COUPLING / max(M.sum(axis=1).max(), 1e-300))
    for (lo, hi), g in zip(blocks, diag):
        G[np.arange(lo, hi), np.arange(lo, hi)] = g
    slowest = len(blocks) - 1
    early = [b for b, g in enumerate(diag) if g >= EARLY_DIAGONAL]
    A = np.zeros((len_pad, RP))
    P = np.zeros((len_pad, RP))
    Gp = G[:r, :r] + l2 * np.eye(r)
    for y in range(LEN_VALID):
        if y < EARLY_FROM:
            kind = ("block", slowest) if y % 4 == 0 else ("far", 0) if y % 4 == 1 else ("block", (y // 4) % len(blocks)) if y % 4 == 2 else ("zero", 0)
        else:
            kind = ("zero", 0) if y % 5 == 0 else ("block", early[y % len(early)])
        if kind[0] == "zero":
            A[y, :r] = -rng.uniform(0.5, 1.5, size=r)
            continue
        x = rng.uniform(2.0, 3.0, size=r)
        A[y, :r] = Gp @ x + l1
        P[y, :r] = x
        if kind[0] == "far":
            P[y, :r] += rng.uniform(0.2, 0.6) * (1.0 + 0.3 * rng.uniform(-1.0, 1.0, size=r)) * rng.choice([-1.0, 1.0], size=r)
        else:
            lo, hi = blocks[kind[1]]
            P[y, lo:hi] += rng.uniform(0.2, 0.6) * (1.0 + 0.3 * rng.uniform(-1.0, 1.0, size=hi - lo))
    slabs = np.zeros((S, len_pad, RP))
    for s in range(S - 1):
        slabs[s + 1, :LEN_VALID, :r] = rng.uniform(-0.5, 0.5, size=(LEN_VALID, r))
    slabs[0] = A - slabs[1:].sum(axis=0)
    if zero_g:
        G[:] = 0.0
    return P.astype(dtype), slabs.astype(dtype), G.astype(dtype)


LOOSE_TOL, LOOSE_MAX = 0.999, 64                  # the workgroup-exit check: every column freezes after its second step at the latest
TIGHT_TOL, TIGHT_MAX = 1e-30, 4                   # the static-bits check: only a step that moves nothing freezes


def workgroups(case):
    """The valid-column ranges of the workgroups of a case (ApgGeom::COLS columns each)."""
    cols = TILE[case[0]]
    return [(lo, min(lo + cols, LEN_VALID)) for lo in range(0, LEN_VALID, cols)]


def diversity_faults(case, counts):
    """What the restatement's counts of a case must show before anything is compared with them; the list of conditions that fail.  r = 5 has two blocks and never
    reaches the maximum: it is held to three distinct counts and an early-exit workgroup only."""
    counts = np.asarray(counts)
    small = case[2] < case[1] - 3
    faults = []
    if counts.min() < 1 or counts.max() > MAX_STEPS:
        faults.append("a count outside 1 ... the maximum")
    if len(set(counts.tolist())) < 3:
        faults.append("fewer than three distinct counts")
    groups = [counts[lo:hi] for lo, hi in workgroups(case)]
    if not any((g < MAX_STEPS).all() for g in groups):
        faults.append("no workgroup whose valid columns all freeze before the maximum (the early exit)")
    if small:
        return faults
    if len(set(counts.tolist())) < 5:
        faults.append("fewer than five distinct counts")
    if not (counts == MAX_STEPS).any():
        faults.append("no column at the maximum")
    if not any((g == MAX_STEPS).any() for g in groups):
        faults.append("no workgroup that runs to the maximum")
    if any((g == MAX_STEPS).any() for lo, g in zip(range(0, LEN_VALID, TILE[case[0]]), groups) if lo >= EARLY_FROM):
        faults.append("a workgroup from column 64 on reaches the maximum")
    return faults


_RESTATED = {}


def restated(case, l1, l2, T=MAX_STEPS, tol=TOL):
    """((len_valid, r) values, counts) of the fp64 restatement on a step case (cached: the tests share one result and nobody changes it)."""
    key = (case_id(case), l1, l2, T, tol)
    if key not in _RESTATED:
        P, slabs, G = step_case(case, l1, l2)
        _RESTATED[key] = dyn.panel_steps_dyn(P, slabs, G, case[2], LEN_VALID, T, tol, l1, l2)
    return _RESTATED[key]


def column_distances(got, want):
    """Per column (row of the (len_valid, r) block) whose wanted value is not 0: |got - want| / |want|."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    norms = np.linalg.norm(want, axis=1)
    on = norms > 0
    return np.linalg.norm(got - want, axis=1)[on] / norms[on]


def step_fp32_figure(case, l1, l2):
    """The largest norm-relative distance of a column of the fp32 numpy restatement from the fp64 one, both at the fp64 counts."""
    P, slabs, G = step_case(case, l1, l2)
    want, counts = restated(case, l1, l2)
    got, _ = dyn.panel_steps_dyn(P, slabs, G, case[2], LEN_VALID, MAX_STEPS, TOL, l1, l2, dtype=np.float32, forced=counts)
    return float(column_distances(got, want).max())


# the largest such distance over the fp32 STEP_CASES x PENALTIES
FIGURE_STEPS = 2.7e-7      # (found: 2.55e-7, a column of RP 128, r = 125, plain; RP 64 stays below 2.2e-7)


def step_tolerance(case):
    return TOL_F64 if case[0] == np.float64 else MARGIN * FIGURE_STEPS


# ------------------------------------------------------------------ engine level

ENGINE_SHAPES = ((131, 97, 9), (200, 150, 70))      # (m, n, r): RP 64, and RP 128
ENGINE_TOL, ENGINE_STEPS = 0.1, (12, 12)
ENGINE_PENALTIES = hdc.ENGINE_PENALTIES
ENGINE_ITERS = (1, 5)
ENGINE_KINDS = ("plain", "pen", "constw", "sparse")


def engine_problem(m, n, r, dtype, kind="plain"):
    """(coo or None, V, W, H, penalties, constant_w)"""
    if kind == "sparse":      # (hals_multi_cases.sparse_problem with empty rows and columns that these shapes have)
        rng = np.random.default_rng(m + n + r)
        rows, cols, vals, _ = pen.sparse_pattern(m, n, 0.1, rng, (3, m - 31), (0, n // 2))
        vals = vals.astype(dtype)
        V = np.zeros((m, n))
        V[rows, cols] = vals
        W = mc.F((1.0 - rng.random((m, r))).astype(dtype))
        H = mc.F((1.0 - rng.random((r, n))).astype(dtype))
        return (rows, cols, vals), V, W, H, (0.0, 0.0, 0.0, 0.0), False
    V, W, H = mc.planted(m, n, r, dtype, seed=m + n + r)
    return None, V, W, H, ENGINE_PENALTIES if kind == "pen" else (0.0, 0.0, 0.0, 0.0), kind == "constw"


def engine_fp32_figure(shape, kind, iters):
    """The norm-relative distances (W, H) of the fp32 numpy restatement from the fp64 one on an fp32 engine problem, both at the fp64 counts."""
    _, V, W, H, penalties, constant_w = engine_problem(*shape, np.float32, kind)
    W64, H64, _, counts = dyn.run(V, W, H, iters, *ENGINE_STEPS, ENGINE_TOL, penalties, constant_w)
    W32, H32, _, _ = dyn.run(V, W, H, iters, *ENGINE_STEPS, ENGINE_TOL, penalties, constant_w, forced=counts, dtype=np.float32)
    return rel(W32, W64), rel(H32, H64)


# the largest such distance over ENGINE_SHAPES x ENGINE_KINDS x ENGINE_ITERS
FIGURE_ENGINE_FACTORS = 1.7e-5      # (found: 1.58e-5, H of the constant-W case of 200 x 150, r = 70 after 5 iterations; one iteration stays below 2.8e-6)


def engine_tolerance(dtype):
    return TOL_F64 if np.dtype(dtype) == np.float64 else MARGIN * FIGURE_ENGINE_FACTORS
