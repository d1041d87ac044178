"""The cases and the tolerances that tests/test_gpu_beta_online.py and tests/test_beta_online_cpu.py share (docs/DIVERGENCE.md, "Minibatch update").

Engine runs are held to the figures of tests/test_gpu_beta_general.py: fp32 2e-4 on the factors and 1e-5 on the errors and the divergence value, fp64 1e-9 on all.
That stands because numpy's own fp32 run of the restatement stays under a quarter of the fp32 figures on these cases, which the CPU test asserts (largest: 5.9e-7
on the factors, 1.3e-8 on the errors).  The data is a planted product times gamma noise with a positive start, on which the fp64 restatement never flushes an entry
(asserted where the runs are made): the flush is the kernel test's subject.

The mixed-precision engine is compared with the bf16-emulating restatement; its tolerance is MARGIN x the emulation's own fp32-against-fp64 figure, the rule of
tests/beta_mixed_cases.py: the constants below are those two-run figures, and the CPU test fails if one is smaller than what it finds or more than 1.5 times larger.

The kernel entry is held to 10 eps of T, norm-relative, on the new panel and the two accumulators, and ten times that on the sums, as check_half_step of
tests/test_gpu_beta_general.py holds the existing update.  numpy's own fp32 run of update_rows on the kernel test's cases differs from its fp64 run by at most
KERNEL_FP32_FIGURE (the CPU test recomputes it), and 4 x that is below 10 eps: the figure stays."""
import numpy as np

from tests import beta_general_reference as gen
from tests import beta_online_reference as onl

EPS32 = float(np.finfo(np.float32).eps)
PEN = (0.05, 0.05, 0.01, 0.01)      # (l1W, l1H, l2W, l2H)
PASSES = 5
FORGET = 0.7
BETAS = (0.0, 0.5, 1.0, 2.0)
TOL = {np.float32: (2e-4, 1e-5), np.float64: (1e-9, 1e-9)}      # factors, errors
MARGIN = 4.0

# (m, n, r, batch): batches of 128 / 128 / 44 at RP = 64; RP = 256 (reduction tiles of 64 in fp32) with a remainder of 72; one batch that holds all of V
SHAPE_SMALL = (203, 300, 9, 128)
SHAPE_WIDE = (150, 200, 129, 128)
SHAPE_ONE_BATCH = (203, 300, 9, 384)
MIXED_CASE = (SHAPE_SMALL, 0.5)

# the emulating restatement with fp32 accumulation against the same with fp64 accumulation on MIXED_CASE: factors (norm-relative), errors (relative)
FIGURE_MIXED_FACTORS = 5.0e-5
FIGURE_MIXED_ERRORS = 4.6e-6
# numpy's fp32 run of update_rows against its fp64 run on the kernel test's cases, norm-relative, the largest of panel, A and B
KERNEL_FP32_FIGURE = 8.3e-8


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / max(np.linalg.norm(np.asarray(b, np.float64)), 1e-300))


def problem(shape, beta, dtype):
    m, n, r, _ = shape
    seed = 500 + r + int(10 * beta)
    V = np.asfortranarray(gen.planted(m, n, seed=seed).astype(dtype))
    W0, H0 = gen.start(m, n, r, seed + 1, dtype)
    return V, W0, H0


_RUNS = {}


def reference_run(shape, beta, eps, pen=gen.NO_PENALTIES, dtype=np.float64, mixed=False, data=np.float32):
    """The restatement's run of an engine case on the data as `data` holds it, accumulated in `dtype` (cached: every test that needs it shares one result, and
    nobody changes it).  Returns (W, H, frobenius, rmsd, divergence, flushed) with flushed the number of entries the run set to 0."""
    key = (shape, beta, float(eps), pen, np.dtype(dtype).name, mixed, np.dtype(data).name)
    if key not in _RUNS:
        V, W0, H0 = problem(shape, beta, data)
        flushed = []
        out = onl.run(V.astype(dtype), W0.astype(dtype), H0.astype(dtype), PASSES, beta, eps, shape[3], FORGET, pen, dtype=dtype, mixed=mixed, flushed=flushed)
        _RUNS[key] = out + (int(sum(flushed)),)
    return _RUNS[key]


def figures(got, want):
    """(factors, errors): the larger of the two norm-relative factor differences, the largest of the three relative error differences."""
    return (max(rel(got[0], want[0]), rel(got[1], want[1])), max(abs(got[k] / want[k] - 1) for k in (2, 3, 4)))


def engine_cases():
    """(shape, beta, penalties, dtype) of every unmixed engine run of the GPU test."""
    cases = [(SHAPE_SMALL, b, gen.NO_PENALTIES, dt) for dt in (np.float32, np.float64) for b in BETAS]
    cases += [(SHAPE_SMALL, 0.5, PEN, dt) for dt in (np.float32, np.float64)]
    cases += [(SHAPE_WIDE, b, gen.NO_PENALTIES, np.float32) for b in BETAS]
    cases += [(SHAPE_ONE_BATCH, 1.0, gen.NO_PENALTIES, np.float32)]
    return cases


# ---- the kernel entry ---------------------------------------------------------------------------------------------------------------------------------------------
KERNEL_OUT_PAD, KERNEL_OUT_VALID = 256, 203      # not a multiple of the workgroup's 16 rows, and across a 128-row part
KERNEL_RANKS = {64: 61, 128: 125, 256: 253}
KERNEL_BETAS = (1.0, 2.0, 0.0, 0.5)              # vector denominators (gamma = 1); panel denominators with gamma = 1, 1/2 and 2/3
KERNEL_SLABS = (1, 3)
KERNEL_RHOS = (0.0, 0.4, 1.0)
KERNEL_PENALTIES = ((0.0, 0.0), (0.05, 0.01))
FLUSH_LOW, FLUSH_HIGH, ZERO_ENTRIES = (slice(0, 8), 1), (slice(8, 16), 2), (slice(20, 40), 3)      # (rows, column) of the constructed entries


def kernel_case(RP, dtype, beta, slabs, online, rho, pen, seed=7):
    """Arrays of the kernel test in `dtype`: P, num_part, den (a vector at beta = 1), A, B -- P with zeros at ZERO_ENTRIES (where A > 0), and numerators scaled so
    that the fp64 update gives eps / 4 at FLUSH_LOW and 4 eps at FLUSH_HIGH (their A is 0, so the new value is proportional to num^gamma in both forms)."""
    r, out_pad, out_valid = KERNEL_RANKS[RP], KERNEL_OUT_PAD, KERNEL_OUT_VALID
    eps = float(np.finfo(dtype).eps)
    rng = np.random.default_rng(seed + RP + slabs)
    P = np.zeros((out_pad, RP), dtype); P[:out_valid, :r] = 1.0 - rng.random((out_valid, r))
    P[ZERO_ENTRIES] = 0
    num = (0.5 + rng.random((slabs, out_pad, RP))).astype(dtype)
    den = (0.5 + rng.random(RP)).astype(dtype) if beta == 1 else (0.5 + rng.random((slabs, out_pad, RP))).astype(dtype)
    A = (0.5 + rng.random((out_pad, RP))).astype(dtype); B = (0.5 + rng.random((out_pad, RP))).astype(dtype)
    A[FLUSH_LOW] = 0; A[FLUSH_HIGH] = 0
    g = gen.gamma_of(beta)
    for where, target in ((FLUSH_LOW, eps / 4), (FLUSH_HIGH, 4 * eps)):
        now = kernel_reference(P, num, den, A, B, RP, beta, online, rho, pen, dtype, flush=False)[0][where]
        num[(slice(None),) + where] *= ((target / now) ** (1.0 / g)).astype(dtype)
    return P, num, den, A, B


def kernel_reference(P, num, den, A, B, RP, beta, online, rho, pen, dtype, flush=True, accumulate=np.float64):
    """update_rows on the valid part of kernel_case's arrays, accumulated in `accumulate` with the eps, penalties and rho of `dtype`: (panel, A, B)."""
    r, v = KERNEL_RANKS[RP], KERNEL_OUT_VALID
    cut = lambda a: a[..., :v, :r].astype(accumulate)
    n = cut(num).sum(axis=0) if num.shape[0] > 1 else cut(num)[0]
    d = den[:r].astype(accumulate) if den.ndim == 1 else (cut(den).sum(axis=0) if den.shape[0] > 1 else cut(den)[0])
    acc = (cut(A), cut(B)) if online else None
    return onl.update_rows(cut(P), n, d, beta, accumulate(np.finfo(dtype).eps), float(dtype(pen[0])), float(dtype(pen[1])), acc, float(dtype(rho)), flush)
