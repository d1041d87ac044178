"""The inputs that tests/test_gpu_hals_dyn_sweep.py, tests/test_gpu_hals_dyn.py and tests/test_hals_dyn_cpu.py share (docs/HALS.md, "Dynamic stopping"), in the
manner of tests/hals_multi_cases.py: the CPU test checks, without a device, every condition the GPU tests rely on.

Sweep level.  Every instantiated (dtype, RP) of k_sweeps_hals_dyn at len_pad = 128, len_valid = 100, r in {RP - 3, RP} (and r = 5 at RP 64), S in {1, 3}, plain and
penalised, delta = 0.1 with a maximum of 12 sweeps.  The input is built so that the fp64 restatement's counts are diverse (sweep_case):

  G is diagonally dominant (so hals_multi_reference.multi_sweep_bound stays tight) with unit diagonal and up to four diagonal blocks of coordinates whose
  off-diagonal row sums are RATES -- Gauss-Seidel contracts an error that lives in a block at about that block's rate -- plus a weak random coupling (row sum 0.01).

  Columns come in kinds.  "block b": the start is the interior solution x* > 0 of the column (a = (G + l2 I) x* + l1) plus a perturbation inside block b, so the
  column converges at the rate of that block: the slowest block (0.93) is still moving by a factor > delta at the maximum, the fast ones freeze after 2 ... 5
  sweeps.  "far": the same with every block perturbed, each with a sign of its own.  "zero": start 0 and a < 0, a fixed point in every precision (every step clamps to exactly 0): count 1.
  Columns below 64 mix all kinds; columns from 64 on (one workgroup of 64 columns, two of 32 or three of 16 -- HalsGeom::COLS -- with the padding behind them)
  hold only kinds that freeze early, so those workgroups take the early exit while the others run to the maximum.
"""
import numpy as np

from tests import hals_dyn_reference as dyn
from tests import hals_multi_cases as mc

LEN_PAD, LEN_VALID = 128, 100
TOL, MAX_SWEEPS = 0.1, 12
PENALTIES = ((0.0, 0.0), (0.05, 0.01))
RATES = {1: (0.93,), 2: (0.93, 0.3), 3: (0.93, 0.6, 0.3), 4: (0.93, 0.75, 0.5, 0.25)}
COUPLING = 0.01
FLIP_CAP = 0.98                                   # the rule check: counts equal for at least this share of the valid columns
EARLY_FROM = 64                                   # columns from here on hold only early-freezing kinds

# (dtype, RP, r, S)
SWEEP_CASES = [(dtype, RP, r, (1, 3)[i % 2])
               for dtype, rps in mc.INSTANTIATIONS.items()
               for RP in rps
               for i, r in enumerate(([5] if RP == 64 else []) + [RP - 3, RP])]


def case_id(case):
    dtype, RP, r, S = case
    return f"{np.dtype(dtype).name}-RP{RP}-r{r}-S{S}"


def blocks_of(r):
    """The coordinate ranges of the diagonal blocks of G and their rates: min(4, r // 2) near-equal ranges."""
    nb = max(1, min(4, r // 2))
    edges = [round(i * r / nb) for i in range(nb + 1)]
    return [(edges[i], edges[i + 1]) for i in range(nb)], RATES[nb]


def sweep_case(case, l1=0.0, l2=0.0):
    """(P (len_pad, RP), slabs (S, len_pad, RP), G (RP, RP)) in the case's dtype, zero on all padding (the launch helper of the GPU test puts NaN there)."""
    dtype, RP, r, S = case
    rng = np.random.default_rng(RP * 1000 + r + 7 * S)
    blocks, rates = blocks_of(r)
    G = np.zeros((RP, RP))
    M = rng.uniform(-1.0, 1.0, size=(r, r))
    M = np.triu(M, 1)
    M = M + M.T
    G[:r, :r] = M * (COUPLING / np.abs(M).sum(axis=1).max())
    for (lo, hi), rate in zip(blocks, rates):
        G[lo:hi, lo:hi] -= rate / max(hi - lo - 1, 1)
    G[np.arange(r), np.arange(r)] = 1.0
    fast = [b for b, rate in enumerate(rates) if rate <= 0.6]
    A = np.zeros((LEN_PAD, RP))
    P = np.zeros((LEN_PAD, RP))
    Gp = G[:r, :r] + l2 * np.eye(r)
    for y in range(LEN_VALID):
        if y < EARLY_FROM:
            kind = ("block", 0) if y % 4 == 0 else ("far", 0) if y % 4 == 1 else ("block", (y // 4) % len(blocks)) if y % 4 == 2 else ("zero", 0)
        else:
            kind = ("zero", 0) if y % 5 == 0 else ("block", fast[y % len(fast)])
        if kind[0] == "far":
            x = rng.uniform(2.0, 3.0, size=r)
            A[y, :r] = Gp @ x + l1
            P[y, :r] = x + rng.uniform(0.2, 0.6) * (1.0 + 0.3 * rng.uniform(-1.0, 1.0, size=r)) * rng.choice([-1.0, 1.0], size=len(blocks))[np.searchsorted(
                [hi for _, hi in blocks], np.arange(r), side="right")]
        elif kind[0] == "zero":
            A[y, :r] = -rng.uniform(0.5, 1.5, size=r)
        else:
            x = rng.uniform(2.0, 3.0, size=r)
            A[y, :r] = Gp @ x + l1
            lo, hi = blocks[kind[1]]
            P[y, :r] = x
            P[y, lo:hi] += rng.uniform(0.2, 0.6) * (1.0 + 0.3 * rng.uniform(-1.0, 1.0, size=hi - lo))
    slabs = np.zeros((S, LEN_PAD, RP))
    for s in range(S - 1):
        slabs[s + 1, :LEN_VALID, :r] = rng.uniform(-0.5, 0.5, size=(LEN_VALID, r))
    slabs[0] = A - slabs[1:].sum(axis=0)
    return P.astype(dtype), slabs.astype(dtype), G.astype(dtype)


LOOSE_TOL, LOOSE_MAX = 0.999, 64


def settled_case(case):
    """sweep_case with the panel three fp64 sweeps on: every moving column is past the first sweeps (where the step of a Gauss-Seidel pass may still grow) and its
    steps shrink from sweep to sweep, so that at delta = LOOSE_TOL every column freezes after its second sweep at the latest -- the input of the workgroup-exit check."""
    P, slabs, G = sweep_case(case)
    r = case[2]
    on, _ = dyn.panel_sweeps_dyn(P, slabs, G, r, LEN_VALID, 3, 0.0)
    P = P.copy()
    P[:LEN_VALID, :r] = on.astype(case[0])
    return P, slabs, G


def workgroups(case):
    """The valid-column ranges of the workgroups of a case (HalsGeom::COLS columns each)."""
    cols = mc.cols_and_chunk(case[0], case[1])[0]
    return [(lo, min(lo + cols, LEN_VALID)) for lo in range(0, LEN_VALID, cols)]


def diversity_faults(case, counts):
    """What the restatement's counts of a case must show before anything is compared with them; the list of conditions that fail."""
    counts = np.asarray(counts)
    faults = []
    if counts.min() < 1 or counts.max() > MAX_SWEEPS:
        faults.append("a count outside 1 ... the maximum")
    if len(set(counts.tolist())) < 3:
        faults.append("fewer than three distinct counts")
    if not (counts == MAX_SWEEPS).any():
        faults.append("no column at the maximum")
    groups = [counts[lo:hi] for lo, hi in workgroups(case)]
    if not any((g < MAX_SWEEPS).all() for g in groups):
        faults.append("no workgroup whose valid columns all freeze before the maximum (the early exit)")
    if not any((g == MAX_SWEEPS).any() for g in groups):
        faults.append("no workgroup that runs to the maximum")
    return faults


_RESTATED = {}


def restated(case, l1, l2):
    """((len_valid, r) values, counts) of the fp64 restatement on a sweep case (cached: the tests share one result and nobody changes it)."""
    key = (case_id(case), l1, l2)
    if key not in _RESTATED:
        P, slabs, G = sweep_case(case, l1, l2)
        _RESTATED[key] = dyn.panel_sweeps_dyn(P, slabs, G, case[2], LEN_VALID, MAX_SWEEPS, TOL, l1, l2)
    return _RESTATED[key]


# ------------------------------------------------------------------ engine level

ENGINE_SHAPES = ((131, 97, 9), (200, 150, 70))      # (m, n, r): RP 64, and RP 128
ENGINE_TOL, ENGINE_SWEEPS = 0.1, 8
ENGINE_PENALTIES = (0.05, 0.05, 0.01, 0.01)       # (l1W, l1H, l2W, l2H): the penalised case of tests/test_gpu_hals_penalty.py's planted runs


def engine_problem(m, n, r, dtype):
    return mc.planted(m, n, r, dtype, seed=m + n + r)
