"""The numpy restatement of the minibatch (online) dense beta-divergence update (tests/beta_online_reference.py) against scikit-learn's MiniBatchNMF, and the
figures the GPU test's tolerances rest on (tests/beta_online_cases.py).  No GPU.

The restatement adds eps where scikit-learn replaces zeros by EPSILON (P = W H + eps against a clip of W H at EPSILON below beta = 2, den + eps against
den == 0 -> EPSILON); nothing else is known to differ.  Measured: one online half-step differs by at most 6.2e-16 norm-relative over the cases below, five passes at
203 x 300 by at most 1.1e-15, both under a quarter of the 1e-13 (a step) and 1e-12 (a run) that the existing comparisons with scikit-learn hold, so those figures
stand."""
import numpy as np
import pytest

from tests import beta_general_reference as gen
from tests import beta_online_cases as cases
from tests import beta_online_reference as onl

sk = pytest.importorskip("sklearn.decomposition._nmf")

EPS = float(np.finfo(np.float64).eps)
BETAS = (-1.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0)
STEP_TOL, RUN_TOL = 1e-13, 1e-12


# 1a. one online half-step against _multiplicative_update_h(..., A, B, rho)
@pytest.mark.parametrize("penalties", [(0.0, 0.0), (0.3, 0.2)])
@pytest.mark.parametrize("beta", BETAS)
def test_online_half_step_is_scikit_learns(beta, penalties):
    m, b, r, rho = 37, 29, 5, 0.4
    rng = np.random.default_rng(11)
    VJ = gen.planted(m, b, seed=12)
    W = 1.0 - rng.random((m, r)); HJ = 1.0 - rng.random((r, b))
    A = 0.5 + rng.random((m, r)); B = 0.5 + rng.random((m, r))
    l1, l2 = penalties
    got, gA, gB = onl.half_step(VJ, W, HJ.T.copy(), beta, EPS, l1, l2, acc=(A, B), rho=rho)
    sA, sB = A.T.copy(), B.T.copy()
    want = sk._multiplicative_update_h(np.array(VJ.T, order="C"), np.array(HJ.T, order="C"), np.array(W.T, order="C"), beta, l1, l2, gen.gamma_of(beta), A=sA, B=sB, rho=rho)
    figure = max(cases.rel(got, want.T), cases.rel(gA, sA.T), cases.rel(gB, sB.T))
    print(f"online half-step beta {beta} penalties {penalties}: {figure:.2e}")
    assert figure < STEP_TOL / 4      # (the measured difference stays under a quarter of the figure: the figure stands)
    assert figure < STEP_TOL


# 1b. five passes against MiniBatchNMF on V^T; penalised: alpha_W alone, which scikit-learn scales by the feature count (constant over the batches) and applies to
#     the codes -- this project's H (alpha_H is scaled by each batch's own length, which the engine's constant penalties do not restate)
@pytest.mark.parametrize("alpha", [0.0, 1e-3])
@pytest.mark.parametrize("beta", BETAS)
def test_five_passes_are_scikit_learns(beta, alpha):
    m, n, r = 203, 300, 9
    V = gen.planted(m, n, seed=21)
    W0, H0 = gen.start(m, n, r, 22)
    est = sk.MiniBatchNMF(n_components=r, init="custom", batch_size=128, beta_loss=beta, tol=0, max_no_improvement=None, fresh_restarts=False, forget_factor=0.7,
                          max_iter=5, alpha_W=alpha, alpha_H=0.0, l1_ratio=0.5)
    codes = est.fit_transform(np.array(V.T, order="C"), W=np.array(H0.T, order="C"), H=np.array(W0.T, order="C"))      # (copies: scikit-learn updates them in place)
    assert est.n_iter_ == 5 and est.n_steps_ == 15
    pen = (0.0, m * alpha * 0.5, 0.0, m * alpha * 0.5)
    W, H = onl.run(V, W0, H0, 5, beta, EPS, 128, 0.7, pen)[:2]
    figure = max(cases.rel(W, est.components_.T), cases.rel(H, codes.T))
    print(f"five passes beta {beta} alpha_W {alpha}: {figure:.2e}")
    assert figure < RUN_TOL / 4
    assert figure < RUN_TOL


# 2. forget_factor = 0 with a single batch: the un-normalised full-batch update
@pytest.mark.parametrize("penalties", [gen.NO_PENALTIES, cases.PEN])
@pytest.mark.parametrize("beta", BETAS)
def test_no_memory_and_one_batch_is_the_full_batch_update(beta, penalties):
    m, n, r = 61, 83, 6
    V = gen.planted(m, n, seed=31)
    W0, H0 = gen.start(m, n, r, 32)
    assert onl.batches(n, 128) == [(0, n)] and onl.rho_of(0.0, 128, n) == 0.0
    W, H, A, B = onl.run_pass(V, W0, H0, W0.copy(), np.ones_like(W0), 128, beta, EPS, 0.0, penalties)
    H1 = gen.half_step(V.T, H0.T, W0, beta, EPS, penalties[1], penalties[3]).T
    W1 = gen.half_step(V, W0, H1.T, beta, EPS, penalties[0], penalties[2])
    print(f"one batch, rho 0, beta {beta}: W {cases.rel(W, W1):.2e} H {cases.rel(H, H1):.2e}")
    assert cases.rel(H, H1) < 1e-14 and cases.rel(W, W1) < 1e-13


# 3. the objective falls over 30 passes (the online update is not monotone: only the two ends are compared)
@pytest.mark.parametrize("beta", [0.0, 0.5, 1.0, 2.0])
def test_objective_falls(beta):
    m, n, r = 203, 300, 9
    V = gen.planted(m, n, seed=41)
    W0, H0 = gen.start(m, n, r, 42)
    W, H = onl.run(V, W0, H0, 30, beta, EPS, 128, 0.7)[:2]
    before, after = onl.objective(V, W0, H0, beta, EPS), onl.objective(V, W, H, beta, EPS)
    print(f"beta {beta}: objective {before:.6g} -> {after:.6g}")
    assert np.all(np.isfinite(W)) and np.all(np.isfinite(H)) and after < before


# 4. what the GPU test's tolerances rest on: numpy's own fp32 run of the restatement on the engine cases, and no flush in the fp64 runs
@pytest.mark.parametrize("shape,beta,pen,dtype", [c for c in cases.engine_cases() if c[3] == np.float32])
def test_fp32_run_of_the_restatement_is_within_a_quarter_of_the_engine_tolerances(shape, beta, pen, dtype):
    want = cases.reference_run(shape, beta, cases.EPS32, pen)
    got = cases.reference_run(shape, beta, cases.EPS32, pen, dtype=np.float32)
    factors, errors = cases.figures(got, want)
    print(f"fp32 restatement {shape} beta {beta} pen {pen}: factors {factors:.2e} errors {errors:.2e} flushed {want[5]}")
    assert want[5] == 0
    assert factors < cases.TOL[np.float32][0] / 4 and errors < cases.TOL[np.float32][1] / 4


def test_fp64_cases_never_flush():
    for shape, beta, pen, dtype in cases.engine_cases():
        if dtype == np.float64:
            assert cases.reference_run(shape, beta, EPS, pen, data=np.float64)[5] == 0


def test_mixed_figures():
    shape, beta = cases.MIXED_CASE
    want = cases.reference_run(shape, beta, cases.EPS32, mixed=True)
    got = cases.reference_run(shape, beta, cases.EPS32, dtype=np.float32, mixed=True)
    factors, errors = cases.figures(got, want)
    print(f"emulating restatement, fp32 against fp64 accumulation: factors {factors:.2e} errors {errors:.2e} flushed {want[5]}")
    assert want[5] == 0
    assert factors <= cases.FIGURE_MIXED_FACTORS <= 1.5 * factors
    assert errors <= cases.FIGURE_MIXED_ERRORS <= 1.5 * errors


def test_kernel_figure():
    worst = 0.0
    for RP in cases.KERNEL_RANKS:
        for beta in cases.KERNEL_BETAS:
            for slabs in cases.KERNEL_SLABS:
                for online in (False, True):
                    for rho in (cases.KERNEL_RHOS if online else (0.0,)):
                        for pen in cases.KERNEL_PENALTIES:
                            arrays = cases.kernel_case(RP, np.float32, beta, slabs, online, rho, pen)
                            want = cases.kernel_reference(*arrays, RP, beta, online, rho, pen, np.float32)
                            got = cases.kernel_reference(*arrays, RP, beta, online, rho, pen, np.float32, accumulate=np.float32)
                            worst = max([worst] + [cases.rel(g, w) for g, w in zip(got, want) if w is not None])
                            # the constructed entries: flushed at eps / 4, kept at 4 eps, and a zero of P comes back where rho A > 0
                            assert np.all(want[0][cases.FLUSH_LOW] == 0) and np.all(want[0][cases.FLUSH_HIGH] > 0)
                            assert np.all((want[0][cases.ZERO_ENTRIES] > 0) == (online and rho > 0))
    print(f"numpy fp32 update_rows against fp64, norm-relative: {worst:.2e}")
    assert worst <= cases.KERNEL_FP32_FIGURE <= 1.5 * worst
    assert 4 * cases.KERNEL_FP32_FIGURE < 10 * cases.EPS32
