"""The cases and the tolerances that tests/test_gpu_beta_mixed.py and tests/test_beta_mixed_cpu.py share (docs/DIVERGENCE.md, "Mixed precision").

The GPU differs from the bf16-emulating restatement (tests/beta_mixed_reference.py) only where its fp32 accumulation flips a bf16 rounding of an operand.  The
yardstick for that is the restatement itself: its run with fp32 accumulation against its run with fp64 accumulation, on the GPU test's own cases, on the CPU.  The
constants below are the largest figures of those two-run comparisons; the CPU test recomputes every one and fails if a constant is smaller than what it finds or
more than 1.5 times larger, so they cannot drift.  A GPU tolerance is 4 x its figure: the MFMA sums in another order than numpy, so other entries flip."""
import numpy as np

from tests import beta_general_reference as gen
from tests import beta_mixed_reference as mix

EPS32 = float(np.finfo(np.float32).eps)
RPS = (64, 128, 256)
HALF_STEP_BETAS = (0.0, 1.0, 0.5)
HALF_STEP_PENALTIES = ((0.0, 0.0), (0.05, 0.01))
ENGINE_SHAPE = (131, 97)
ENGINE_RANKS = (9, 70, 129)
ENGINE_BETAS = (0.0, 0.5, 1.0, 1.5)
ENGINE_ITERS = 20
MARGIN = 4.0

# the two-run figures (fp32 against fp64 accumulation of the emulating restatement), largest over the cases; see the module docstring
FIGURE_HALF_STEP_PANEL = 3.1e-6       # one half-step, the updated panel, norm-relative (componentwise the same comparison reaches 7.9e-5: compare panels by norm)
FIGURE_ENGINE_FACTORS = 8.2e-4        # 20 iterations, W and H, norm-relative (the flips of twenty iterations add up: the exact restatement is only 1.0e-3 away)
FIGURE_ENGINE_ERRORS = 3.4e-5         # 20 iterations, frobenius, rmsd and the divergence value, relative
# the emulating restatement (fp64 accumulation) against the EXACT fp64 restatement, 20 iterations, the divergence value, relative: what bf16 operands cost
FIGURE_ENGINE_DIVERGENCE_VS_EXACT = 7.4e-5
# The per-row error terms of one half-step are formed in fp32 from the bf16-operand P by the map of the fp32 kernel (hardware log2 / exp2 at a general beta, which
# numpy's fp32 run does not model: its two-run figure is 6.3e-8).  They are held to the project's standing fp32 figure for these terms (tests/test_gpu_beta.py,
# tests/test_gpu_beta_general.py: ten times the panel's 1e-5, componentwise), against the EMULATING restatement.
TOL_HALF_STEP_TERMS = 1e-4


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / max(np.linalg.norm(np.asarray(b, np.float64)), 1e-300))


def half_step_case(RP, seed):
    """tests/test_gpu_beta_general.py's half_step_case in fp32: out 200 / 256, red 190 / 256, r = RP - 3."""
    out_valid, out_pad, red_valid, red_pad, r = 200, 256, 190, 256, RP - 3
    rng = np.random.default_rng(seed)
    A = np.zeros((out_pad, RP), np.float32); A[:out_valid, :r] = 1.0 - rng.random((out_valid, r))
    B = np.zeros((red_pad, RP), np.float32); B[:red_valid, :r] = 1.0 - rng.random((red_valid, r))
    X = np.zeros((out_pad, red_pad), np.float32); X[:out_valid, :red_valid] = gen.planted(out_valid, red_valid, seed=72).astype(np.float32)
    return A, B, X, r, out_valid, red_valid


def exact_case(RP, seed):
    """The same shape with data that bf16 and fp32 hold exactly: A, B in {0, 1} at RP = 256 and {0, 1, 2} below with at most 63 non-zero columns per row
    beside column 0, which is 1 everywhere (so 1 <= P <= 253, and P + eps rounds back to P), V small integers; at beta = 2 then Q = V, R = P, and every
    product and sum is an integer below 2^24."""
    out_valid, out_pad, red_valid, red_pad, r = 200, 256, 190, 256, RP - 3
    rng = np.random.default_rng(seed)
    top = 2 if RP == 256 else 3

    def panel(rows):
        P = rng.integers(0, top, (rows, r)).astype(np.float32)
        if RP < 256:
            for row in P:
                row[1 + rng.permutation(r - 1)[63:]] = 0
        P[:, 0] = 1
        return P
    A = np.zeros((out_pad, RP), np.float32); A[:out_valid, :r] = panel(out_valid)
    B = np.zeros((red_pad, RP), np.float32); B[:red_valid, :r] = panel(red_valid)
    X = np.zeros((out_pad, red_pad), np.float32); X[:out_valid, :red_valid] = rng.integers(0, 8, (out_valid, red_valid))
    return A, B, X, r, out_valid, red_valid


def valid(A, B, X, r, out_valid, red_valid, dtype):
    return A[:out_valid, :r].astype(dtype), B[:red_valid, :r].astype(dtype), X[:out_valid, :red_valid].astype(dtype)


def engine_problem(r, beta, zeros=0.0, shape=ENGINE_SHAPE):
    m, n = shape
    seed = 300 + r + int(10 * beta)
    V = np.asfortranarray(gen.planted(m, n, seed=seed).astype(np.float32))
    if zeros:
        V[np.random.default_rng(seed + 1000).random((m, n)) < zeros] = 0
    W0, H0 = gen.start(m, n, r, seed + 1, np.float32)
    return V, W0, H0


_RUNS = {}


def emulated_run(r, beta, dtype, **kw):
    """The emulating restatement's run of an engine case (cached: every test that needs it shares one result, and nobody changes it)."""
    key = (r, beta, np.dtype(dtype).name, tuple(sorted(kw.items())))
    if key not in _RUNS:
        V, W0, H0 = engine_problem(r, beta)
        _RUNS[key] = mix.run(V.astype(dtype), W0.astype(dtype), H0.astype(dtype), ENGINE_ITERS, beta, EPS32, dtype=dtype, **kw)
    return _RUNS[key]


def derived_bound(beta):
    """The first-order componentwise bound on one update against the exact update (docs/DIVERGENCE.md): gamma (2 |beta - 2| + 2 |beta - 1| + 4) 2^-9, allowed
    1.05 x plus 1e-5 for the second-order terms and the fp32 accumulation.  (bf16 keeps 8 significant bits, so a single rounding can be off by 2^-8 of the value
    and a worst-case bound is twice this; the test holds the smaller figure, which random roundings meet with room: tests/test_beta_mixed_cpu.py.)"""
    return 1.05 * gen.gamma_of(beta) * (2 * abs(beta - 2) + 2 * abs(beta - 1) + 4) * 2.0 ** -9 + 1e-5
