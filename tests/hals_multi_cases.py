"""The cases and the figures that tests/test_gpu_hals_multi.py and tests/test_hals_multi_cpu.py share (docs/HALS.md, "Inner sweeps"), in the manner of
tests/beta_mixed_cases.py.

Sweep level: every instantiated (dtype, RP) of k_sweeps_hals with r, len_valid and S chosen as tests/test_gpu_hals_sweep.py chooses them (the selection is copied
here as plain tuples, so that the CPU test can check the conditions the GPU test relies on without a device).

Engine level: (s_H, s_W) = (3, 2) against tests/hals_multi_reference.py after 1 and 10 iterations.  fp64 is held to 1e-9, the project's standing figure.  The standing
fp32 figure of tests/test_gpu_hals.py (2e-4) does not carry over: with more sweeps per iteration an fp32 trajectory leaves the fp64 one sooner, whatever computes
it.  The yardstick is the restatement itself: its run in fp32 numpy against its run in fp64, on the GPU test's own fp32 cases, on the CPU.  FIGURE_ENGINE_FACTORS
is the largest norm-relative distance of W or H over those cases; the CPU test recomputes it and fails if the constant is smaller than what it finds or more than 1.5
times larger.  The GPU tolerance is MARGIN x the figure: the GPU sums in another order than numpy.
"""
import numpy as np

from tests import hals_multi_reference as multi
from tests import hals_penalty_reference as pen

LEN_PAD = 256
INSTANTIATIONS = {np.float32: [64, 128, 256, 384, 512], np.float64: [64, 128, 192, 256, 320, 384, 448, 512]}
UNIT = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
SWEEP_COUNTS = (2, 3)
SWEEP_PENALTIES = ((0.0, 0.0), (0.05, 0.01))


def cols_and_chunk(dtype, RP):
    """(columns per workgroup, rows of G per LDS chunk) of the sweep kernels (HalsGeom): only to choose r and len_valid at the edges."""
    L = 4 if RP <= 64 else 8 if RP <= 128 else 16 if RP <= 256 else 32
    C = 1 if RP <= 128 else 2
    KC = min(65536 // (RP * np.dtype(dtype).itemsize), RP)
    return (256 // L) * C, KC


def _sweep_cases():
    """(dtype, RP, r, len_valid, S): r = prev + 1, RP - 1, RP and both sides of an LDS chunk boundary; len_valid and S rotate over all the cases."""
    out = []
    for dtype, rps in INSTANTIATIONS.items():
        prev = 0
        for RP in rps:
            cols, kc = cols_and_chunk(dtype, RP)
            rs = [prev + 1, RP - 1, RP]
            m = next((q for q in range(kc, RP, kc) if q >= prev + 2 and q + 1 < RP - 1), None)
            if m is not None:
                rs += [m, m + 1]
            lvs = [1, cols - 1, cols + 1, LEN_PAD - 1]
            for r in sorted(set(rs)):
                i = len(out)
                out.append((dtype, RP, r, lvs[i % 4], (1, 3)[(i // 4) % 2]))
            prev = RP
    return out


SWEEP_CASES = _sweep_cases()


def case_id(case):
    dtype, RP, r, lv, S = case
    return f"{np.dtype(dtype).name}-RP{RP}-r{r}-len{lv}-S{S}"


def case_rng(case, salt):
    return np.random.default_rng(case[1] * 1000 + case[2] + 100 + salt)


def streams_g(case):
    """Whether the kernel streams G through LDS in more than one chunk at this r (every sweep restages from chunk 0 there)."""
    dtype, RP, r, _, _ = case
    return r > cols_and_chunk(dtype, RP)[1]


# ------------------------------------------------------------------ engine level

SWEEPS_H, SWEEPS_W = 3, 2
ENGINE_ITERS = (1, 10)
ENGINE_PENALTIES = (0.05, 0.05, 0.01, 0.01)       # (l1W, l1H, l2W, l2H): 0.05 and 0.01 on both factors
MARGIN = 4.0
TOL_F64 = 1e-9
# (kind, m, n, r, dtype); kind: "dense" planted V, "sparse" sparse compute on a random 5 % pattern, "pen" planted with ENGINE_PENALTIES, "constw" constant W
ENGINE_CASES = [
    ("dense", 500, 300, 7, np.float32), ("dense", 500, 300, 33, np.float32), ("dense", 300, 257, 70, np.float32), ("dense", 300, 257, 129, np.float32),
    ("dense", 500, 300, 7, np.float64), ("dense", 600, 500, 200, np.float64),
    ("sparse", 300, 257, 70, np.float32), ("sparse", 300, 257, 70, np.float64),
    ("pen", 300, 257, 70, np.float32), ("pen", 300, 257, 70, np.float64),
    ("constw", 500, 300, 33, np.float32), ("constw", 500, 300, 33, np.float64),
]
# the largest norm-relative distance of W or H between the fp32 and the fp64 numpy restatement over the fp32 ENGINE_CASES at ENGINE_ITERS; see the module docstring
FIGURE_ENGINE_FACTORS = 2.1e-4      # (found: 1.75e-4, W of the dense r = 129 case after 10 iterations; the r = 7 case stays at 8.8e-6)
EMPTY_ROWS, EMPTY_COLS = (3, 150, 299), (0, 77)


def engine_case_id(case):
    kind, m, n, r, dtype = case
    return f"{kind}-{m}x{n}-r{r}-{np.dtype(dtype).name}"


def F(a):
    return np.asfortranarray(a)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / max(np.linalg.norm(np.asarray(b, np.float64)), 1e-300))


def problem(m, n, r, dtype, seed=1):
    """tests/test_gpu_hals.py's problem(): uniformly random V, where the residual is large enough for the fp32 trace formula of the reported error."""
    rng = np.random.default_rng(seed)
    V = F(rng.random((m, n)).astype(dtype))
    W = F((1.0 - rng.random((m, r))).astype(dtype))
    H = F((1.0 - rng.random((r, n))).astype(dtype))
    return V, W, H


def planted(m, n, r, dtype, seed=1):
    """tests/test_gpu_hals.py's planted(): V = W0 H0 + 0.01 noise."""
    rng = np.random.default_rng(seed)
    V = F((rng.random((m, r)) @ rng.random((r, n)) + 0.01 * rng.random((m, n))).astype(dtype))
    W = F((1.0 - rng.random((m, r))).astype(dtype))
    H = F((1.0 - rng.random((r, n))).astype(dtype))
    return V, W, H


def sparse_problem(m, n, r, dtype, seed=1, density=0.05):
    """tests/test_gpu_hals_sparse.py's sparse_problem(): COO triplets sorted by (row, column) with a stored zero and a few empty rows and columns, the densified V
    (the values rounded to dtype), a start."""
    rng = np.random.default_rng(seed)
    rows, cols, vals, _ = pen.sparse_pattern(m, n, density, rng, EMPTY_ROWS, EMPTY_COLS)
    vals = vals.astype(dtype)
    V = np.zeros((m, n))
    V[rows, cols] = vals
    W = F((1.0 - rng.random((m, r))).astype(dtype))
    H = F((1.0 - rng.random((r, n))).astype(dtype))
    return (rows, cols, vals), V, W, H


def engine_problem(case):
    """(coo or None, V as the restatement takes it, W, H, penalties, constant_w) of an engine case."""
    kind, m, n, r, dtype = case
    seed = m + n + r
    if kind == "sparse":
        coo, V, W, H = sparse_problem(m, n, r, dtype, seed)
        return coo, V, W, H, (0.0, 0.0, 0.0, 0.0), False
    V, W, H = planted(m, n, r, dtype, seed)
    return None, V, W, H, ENGINE_PENALTIES if kind == "pen" else (0.0, 0.0, 0.0, 0.0), kind == "constw"


_RUNS = {}


def restated(case, iters):
    """(W, H, errors) of the fp64 restatement at (SWEEPS_H, SWEEPS_W) after `iters` iterations (cached: the tests share one result and nobody changes it)."""
    key = (engine_case_id(case), iters)
    if key not in _RUNS:
        _, V, W, H, penalties, constant_w = engine_problem(case)
        _RUNS[key] = multi.run(np.asarray(V, np.float64), W, H, iters, SWEEPS_H, SWEEPS_W, penalties, constant_w)
    return _RUNS[key]


def fp32_figure(case, iters):
    """The norm-relative distances (W, H) of the fp32 numpy restatement from the fp64 one on an fp32 engine case."""
    _, V, W, H, penalties, constant_w = engine_problem(case)
    W32, H32 = multi.run_in(V, W, H, iters, SWEEPS_H, SWEEPS_W, np.float32, penalties, constant_w)
    W64, H64, _ = restated(case, iters)
    return rel(W32, W64), rel(H32, H64)
