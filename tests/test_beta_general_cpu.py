"""General dense beta-divergence NMF with L1 / L2 penalties, without a GPU (docs/DIVERGENCE.md): the numpy restatement the GPU tests compare with
(tests/beta_general_reference.py) against the existing restatement at beta = 0 and 1, against scikit-learn's solver="mu" with and without penalties, its objective's
monotonicity, the nmfamd_params_v3 layout on both sides of the C boundary, and the refusals nmfgpu::compute makes before it touches a device."""
import ctypes as C
import os
import subprocess
import tempfile
import warnings

import numpy as np
import pytest

from tests import beta_general_reference as gen
from tests import beta_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS64 = float(np.finfo(np.float64).eps)
SHAPES = [(131, 97, 8), (200, 150, 65)]
PENALTIES = [(0.5, 0.5, 0.0, 0.0), (0.0, 0.0, 0.1, 0.1), (0.5, 0.5, 0.1, 0.1)]      # (l1W, l1H, l2W, l2H)


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@pytest.mark.parametrize("beta", [0, 1])
@pytest.mark.parametrize("m,n,r", SHAPES)
def test_restatement_is_the_existing_one_at_beta_0_and_1(beta, m, n, r):
    V = ref.planted(m, n, seed=r)
    W0, H0 = ref.start(m, n, r, seed=r + 1)
    for const_w in (False, True):
        want = ref.run(V, W0, H0, 12, beta, EPS64, const_w=const_w)
        got = gen.run(V, W0, H0, 12, float(beta), EPS64, const_w=const_w)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2:] == want[2:]
    # fp32 as well (the GPU tests' spread figures come from it)
    want = ref.run(V, W0, H0, 5, beta, float(np.finfo(np.float32).eps), dtype=np.float32)
    got = gen.run(V, W0, H0, 5, beta, float(np.finfo(np.float32).eps), dtype=np.float32)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2:] == want[2:]


def test_gamma_is_scikit_learns_rule():
    assert gen.gamma_of(-1.0) == 1.0 / 3.0 and gen.gamma_of(0.0) == 0.5 and gen.gamma_of(0.5) == 1.0 / 1.5
    assert gen.gamma_of(1.0) == 1.0 and gen.gamma_of(1.5) == 1.0 and gen.gamma_of(2.0) == 1.0 and gen.gamma_of(3.0) == 0.5


def test_divergence_limits():
    """The general divergence value tends to the KL and Itakura-Saito values of the existing restatement as beta tends to 1 and 0."""
    m, n, r = 40, 30, 4
    V = ref.planted(m, n, seed=3)
    W, H = ref.start(m, n, r, seed=4)
    for beta, h in ((1, 1e-6), (0, 1e-6)):
        want = float(ref.terms(V, W, H.T, beta, EPS64)[1].sum())
        for b in (beta + h, beta - h):
            assert gen.divergence(V, W, H, b, EPS64) == pytest.approx(want, rel=1e-4)


# scikit-learn's solver="mu" on the transposed problem (it updates its LEFT factor first: on V^T, with W = H0^T and H = W0^T, that is our H-then-W order).
# It scales its penalties by the matrix dimensions: l1_reg_W = n_features alpha_W l1_ratio, l2_reg_W = n_features alpha_W (1 - l1_ratio), l1_reg_H / l2_reg_H the
# same with n_samples and alpha_H.  On V^T (n_samples = n, n_features = m) its W is our H^T, so (l1H, l2H) = m alpha_W (l1_ratio, 1 - l1_ratio) and
# (l1W, l2W) = n alpha_H (l1_ratio, 1 - l1_ratio).
@pytest.mark.parametrize("penalised", [False, True])
@pytest.mark.parametrize("beta", [-1.0, 0.5, 1.5, 3.0])
@pytest.mark.parametrize("m,n,r", SHAPES)
def test_scikit_learn_cross_check(m, n, r, beta, penalised):
    sk = pytest.importorskip("sklearn.decomposition")
    from sklearn.decomposition._nmf import _beta_divergence
    iters = 30
    V = ref.planted(m, n, seed=r + 30)
    W0, H0 = ref.start(m, n, r, seed=r + 31)
    l1_ratio = 5.0 / 6.0
    alpha_W, alpha_H = (0.06 / m, 0.06 / n) if penalised else (0.0, 0.0)
    pen = (n * alpha_H * l1_ratio, m * alpha_W * l1_ratio, n * alpha_H * (1.0 - l1_ratio), m * alpha_W * (1.0 - l1_ratio))
    if penalised:
        assert np.allclose(pen, (0.05, 0.05, 0.01, 0.01), rtol=1e-12)
    W, H = gen.run(V, W0, H0, iters, beta, EPS64, pen=pen)[:2]
    model = sk.NMF(n_components=r, solver="mu", beta_loss=beta, init="custom", max_iter=iters, tol=0, alpha_W=alpha_W, alpha_H=alpha_H, l1_ratio=l1_ratio)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Ht = model.fit_transform(np.ascontiguousarray(V.T), W=np.ascontiguousarray(H0.T), H=np.ascontiguousarray(W0.T))
    assert model.n_iter_ == iters
    figure = rel(W @ H, (Ht @ model.components_).T)
    ours = gen.divergence(V, W, H, beta, EPS64)
    theirs = float(_beta_divergence(np.ascontiguousarray(V.T), np.ascontiguousarray(H.T), np.ascontiguousarray(W.T), beta))
    print(f"beta {beta} penalised {penalised} ({m} x {n}, r {r}): W H {figure:.2e} divergence {abs(ours / theirs - 1):.2e}")
    assert figure <= 1e-12
    assert ours == pytest.approx(theirs, rel=1e-12)


def test_one_half_step_is_scikit_learns():
    pytest.importorskip("sklearn.decomposition")
    from sklearn.decomposition._nmf import _multiplicative_update_h
    m, n, r = 60, 45, 7
    V = ref.planted(m, n, seed=40)
    W0, H0 = ref.start(m, n, r, seed=41)
    for beta in (-1.0, 0.0, 0.5, 1.0, 1.5, 3.0):
        H1 = gen.half_step(V.T, H0.T, W0, beta, EPS64, 0.05, 0.01).T
        want = _multiplicative_update_h(V, W0, H0.copy(), beta, 0.05, 0.01, gen.gamma_of(beta))
        assert rel(H1, want) <= 1e-13, (beta, rel(H1, want))


@pytest.mark.parametrize("beta", [-1.0, 0.5, 1.5, 3.0])
def test_divergence_is_non_increasing(beta):
    m, n, r = 131, 97, 8
    V = ref.planted(m, n, seed=r + 20)
    W0, H0 = ref.start(m, n, r, seed=r + 21)
    hist = gen.run(V, W0, H0, 40, beta, EPS64, history=True)[5]
    assert len(hist) == 40 and np.all(np.isfinite(hist)) and hist[-1] < hist[0]
    for a, b in zip(hist, hist[1:]):
        assert b <= a * (1 + 1e-12), (a, b)


@pytest.mark.parametrize("pen", PENALTIES)
@pytest.mark.parametrize("beta", [-1.0, 0.0, 0.5, 1.0, 1.5, 3.0])
def test_penalised_objective_is_non_increasing(beta, pen):
    m, n, r = 131, 97, 8
    V = ref.planted(m, n, seed=r + 20)
    W0, H0 = ref.start(m, n, r, seed=r + 21)
    out = gen.run(V, W0, H0, 40, beta, EPS64, pen=pen, history=True)
    hist = out[5]
    assert len(hist) == 40 and np.all(np.isfinite(hist)) and hist[-1] < hist[0]
    for a, b in zip(hist, hist[1:]):
        assert b <= a * (1 + 1e-12), (a, b)
    # the history is the objective function's value, and the reported divergence carries no penalty terms
    W, H = out[0], out[1]
    assert gen.objective(V, W, H, beta, EPS64, pen) == pytest.approx(gen.divergence(V, W, H, beta, EPS64) + gen.penalty_terms(W, H, pen), rel=1e-15)
    assert out[4] < hist[-1]
    # ... and a penalised run is not normalised, an unpenalised one is
    assert not np.allclose((W * W).sum(axis=0), 1.0)
    Wn = gen.run(V, W0, H0, 3, beta, EPS64)[0]
    assert np.allclose((Wn * Wn).sum(axis=0), 1.0)


def test_params_v3_layout_matches_the_header():
    from nmfgpu_amd.engine import _ParamsV2, _ParamsV3
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "probe.c"), os.path.join(td, "probe")
        open(src, "w").write(r'''
#include <nmfgpu_amd.h>
#include <stddef.h>
#include <stdio.h>
int main(void) { printf("%zu %zu %zu %zu\n", sizeof(nmfamd_params_v2), offsetof(nmfamd_params_v3, v2), offsetof(nmfamd_params_v3, beta), sizeof(nmfamd_params_v3)); return 0; }
''')
        subprocess.check_call(["g++", "-x", "c++", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        size2, off_v2, off_beta, size3 = map(int, subprocess.check_output([exe]).decode().split())
    assert size2 == C.sizeof(_ParamsV2)
    assert off_v2 == _ParamsV3.v2.offset == 0
    assert off_beta == _ParamsV3.beta.offset == size2
    assert size3 == C.sizeof(_ParamsV3) == size2 + 8 and _ParamsV3._fields_[-1][0] == "beta"


@pytest.fixture
def context():
    import nmfgpu_amd as na
    assert na.initialize() in (na.ResultType.Success, na.ResultType.ErrorAlreadyInitialized)
    na.set_verbosity(na.Verbosity.Nothing)
    yield na
    na.finalize()


def test_refusals_before_the_device(context):
    na = context
    m, n, r = 20, 12, 3
    V = np.asfortranarray(ref.planted(m, n, seed=50).astype(np.float32))
    W0, H0 = ref.start(m, n, r, seed=51, dtype=np.float32)
    W, H = W0.copy(order="F"), H0.copy(order="F")
    bad = na.ResultType.ErrorInvalidArgument

    def go(params, Vd=V, Wd=W, Hd=H, **kw):
        return na.compute(Vd, Wd, Hd, iterations=3, parameters=params, **kw)

    GEN = {"divergence": 3, "beta": 0.5}
    # "beta" without "divergence" = 3, whatever its value
    for params in ({"beta": 0.5}, {"beta": 0.0}, {"divergence": 2, "beta": 0.5}, {"divergence": 1, "denseCompute": 1, "beta": 1.0}, {"divergence": 0, "beta": 2.0}):
        assert go(params) == bad
    # a beta that is not finite
    for value in (float("nan"), float("inf"), -float("inf")):
        assert go({"divergence": 3, "beta": value}) == bad
    # another algorithm, sparse compute, missing values, several GPUs
    for alg in (na.NmfAlgorithm.GDCLS, na.NmfAlgorithm.ALS, na.NmfAlgorithm.nsNMF, na.NmfAlgorithm.HALS):
        assert go(GEN, algorithm=alg) == bad
    assert go({**GEN, "sparseCompute": 1}) == bad
    assert go({**GEN, "missingValues": 1}) == bad
    assert go({**GEN, "numGpus": 2}) == bad
    # rank above 256
    Vw = np.asfortranarray(ref.planted(300, 280, seed=52).astype(np.float32))
    Ww, Hw = ref.start(300, 280, 257, seed=53, dtype=np.float32)
    assert go(GEN, Vd=Vw, Wd=Ww, Hd=Hw) == bad
    # penalties that are negative or NaN, on every dense divergence
    for on in (GEN, {"divergence": 2}, {"divergence": 1, "denseCompute": 1}):
        for name in ("l1W", "l1H", "l2W", "l2H"):
            for value in (-0.5, float("nan")):
                assert go({**on, name: value}) == bad
    # the Frobenius multiplicative update and the sparse KL update still take no penalties
    assert go({"l1W": 0.5}) == bad
    assert go({"divergence": 1, "l1H": 0.5}) == bad
    assert np.array_equal(W, W0) and np.array_equal(H, H0)
    if na.device_count() == 0:
        # the valid forms get as far as the device
        gone = na.ResultType.ErrorExternalLibrary
        assert go(GEN) == gone
        assert go({"divergence": 3, "beta": -1.0}) == gone
        assert go({"divergence": 3}) == gone      # (beta = 0: Itakura-Saito)
        assert go({**GEN, "l1W": 0.05, "l1H": 0.05, "l2W": 0.01, "l2H": 0.01}) == gone
        assert go({"divergence": 2, "l1H": 0.05}) == gone
        assert go({"divergence": 1, "denseCompute": 1, "l2W": 0.01}) == gone
        assert go(GEN, constant_basis_vectors=True) == gone
