"""Dense beta-divergence NMF without a GPU (docs/DIVERGENCE.md): the numpy restatement the GPU tests compare with (tests/beta_reference.py) against the C oracle's
KL iteration, its Itakura-Saito objective's monotonicity, scikit-learn's multiplicative-update solver, the nmfamd_params layout on both sides of the C boundary,
and the refusals nmfgpu::compute makes before it touches a device."""
import ctypes as C
import os
import subprocess
import tempfile
import warnings

import numpy as np
import pytest

from oracle import oracle
from tests import beta_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS64 = float(np.finfo(np.float64).eps)
SHAPES = [(131, 97, 8), (200, 150, 65)]


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@pytest.mark.parametrize("m,n,r", SHAPES)
def test_kl_restatement_is_the_oracle(m, n, r):
    iters = 30
    V = ref.planted(m, n, seed=r)
    W0, H0 = ref.start(m, n, r, seed=r + 1)
    W, H, frob, rmsd, kl = ref.run(V, W0, H0, iters, 1, EPS64)
    Wo, Ho = W0.copy(order="F"), H0.copy(order="F")
    res = oracle.run_kl(V, Wo, Ho, iters)
    assert rel(W, Wo) <= 1e-12 and rel(H, Ho) <= 1e-12, (rel(W, Wo), rel(H, Ho))
    assert frob == pytest.approx(res["frobenius"], rel=1e-9) and rmsd == pytest.approx(res["rmsd"], rel=1e-9)
    assert kl == pytest.approx(res["kl"], rel=1e-9)


@pytest.mark.parametrize("m,n,r", SHAPES)
def test_kl_with_zeros_is_the_oracle(m, n, r):
    iters = 12
    V = ref.planted(m, n, seed=r + 10)
    V[np.random.default_rng(r).random((m, n)) < 0.3] = 0.0
    W0, H0 = ref.start(m, n, r, seed=r + 11)
    W, H, frob, rmsd, kl = ref.run(V, W0, H0, iters, 1, EPS64)
    Wo, Ho = W0.copy(order="F"), H0.copy(order="F")
    res = oracle.run_kl(V, Wo, Ho, iters)
    assert rel(W, Wo) <= 1e-12 and rel(H, Ho) <= 1e-12
    assert frob == pytest.approx(res["frobenius"], rel=1e-9) and kl == pytest.approx(res["kl"], rel=1e-9)


@pytest.mark.parametrize("beta", [0, 1])
@pytest.mark.parametrize("m,n,r", SHAPES)
def test_divergence_is_non_increasing(beta, m, n, r):
    V = ref.planted(m, n, seed=r + 20)
    W0, H0 = ref.start(m, n, r, seed=r + 21)
    # (the compensated normalisation leaves W H as it is: the objective of the majorise-minimise update then never rises; the KL engine's plain normalisation of W
    #  changes W H between iterations and carries no such guarantee, so beta = 1 is run compensated here)
    hist = ref.run(V, W0, H0, 50, beta, EPS64, compensated=True, history=True)[5]
    assert len(hist) == 50 and np.all(np.isfinite(hist))
    for a, b in zip(hist, hist[1:]):
        assert b <= a * (1 + 1e-12), (a, b)
    assert hist[-1] < 0.9 * hist[0]


@pytest.mark.parametrize("beta,loss", [(0, "itakura-saito"), (1, "kullback-leibler")])
@pytest.mark.parametrize("m,n,r", SHAPES)
def test_scikit_learn_cross_check(beta, loss, m, n, r):
    sk = pytest.importorskip("sklearn.decomposition")
    iters = 30
    V = ref.planted(m, n, seed=r + 30)
    W0, H0 = ref.start(m, n, r, seed=r + 31)
    W, H = ref.run(V, W0, H0, iters, beta, EPS64, compensated=True)[:2]
    # scikit-learn updates its LEFT factor first: on V^T, with W = H0^T and H = W0^T, that is our H-then-W order
    model = sk.NMF(n_components=r, solver="mu", beta_loss=loss, init="custom", max_iter=iters, tol=0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Ht = model.fit_transform(np.ascontiguousarray(V.T), W=np.ascontiguousarray(H0.T), H=np.ascontiguousarray(W0.T))
    assert model.n_iter_ == iters
    assert rel(W @ H, (Ht @ model.components_).T) <= 1e-12


def test_half_step_is_the_iteration():
    m, n, r = 60, 45, 7
    V = ref.planted(m, n, seed=40)
    W0, H0 = ref.start(m, n, r, seed=41)
    for beta in (0, 1):
        H1 = ref.half_step(V.T, H0.T, W0, beta, EPS64).T
        W1 = ref.half_step(V, W0, H1.T, beta, EPS64)
        W1, H1 = ref.normalize(W1, H1, beta == 0)
        W, H = ref.run(V, W0, H0, 1, beta, EPS64)[:2]
        assert np.array_equal(W, W1) and np.array_equal(H, H1)
        Wc, Hc = ref.run(V, W0, H0, 3, beta, EPS64, const_w=True)[:2]
        assert np.array_equal(Wc, W0) and not np.array_equal(Hc, H0)


def test_params_layout_matches_the_header():
    from nmfgpu_amd.engine import _Params, _ParamsV2
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "probe.c"), os.path.join(td, "probe")
        open(src, "w").write(r'''
#include <nmfgpu_amd.h>
#include <stddef.h>
#include <stdio.h>
int main(void) { printf("%zu %zu %zu %zu %zu\n", offsetof(nmfamd_params, missing_values), sizeof(nmfamd_params), offsetof(nmfamd_params_v2, base),
                        offsetof(nmfamd_params_v2, dense_compute), sizeof(nmfamd_params_v2)); return 0; }
''')
        subprocess.check_call(["g++", "-x", "c++", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        off_missing, size, off_base, off, size2 = map(int, subprocess.check_output([exe]).decode().split())
    # nmfamd_params is frozen (nmfamd_engine_create reads it unsized): as it was, on both sides
    assert off_missing == _Params.missing_values.offset and size == C.sizeof(_Params) and off_missing + 8 == size
    # nmfamd_params_v2: the frozen struct first, the new field at the end, on both sides
    assert off_base == _ParamsV2.base.offset == 0
    assert off == _ParamsV2.dense_compute.offset == size
    assert size2 == C.sizeof(_ParamsV2) == off + 8 and _ParamsV2._fields_[-1][0] == "dense_compute"


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

    IS, KL = {"divergence": 2}, {"divergence": 1, "denseCompute": 1}
    for on in (IS, KL):
        # another algorithm
        for alg in (na.NmfAlgorithm.GDCLS, na.NmfAlgorithm.ALS, na.NmfAlgorithm.nsNMF, na.NmfAlgorithm.HALS):
            assert go(on, algorithm=alg) == bad
        # sparse compute, missing values, several GPUs
        assert go({**on, "sparseCompute": 1}) == bad
        assert go({**on, "missingValues": 1}) == bad
        assert go({**on, "numGpus": 2}) == bad
    # denseCompute without a divergence, and values that are not 0 or 1
    assert go({"denseCompute": 1}) == bad
    assert go({"divergence": 0, "denseCompute": 1}) == bad
    assert go({"denseCompute": 1, "missingValues": 1}) == bad
    for value in (2, -1, 0.5, float("nan")):
        assert go({"divergence": 1, "denseCompute": value}) == bad
    # rank above 256
    Vw = np.asfortranarray(ref.planted(300, 280, seed=52).astype(np.float32))
    Ww, Hw = ref.start(300, 280, 257, seed=53, dtype=np.float32)
    for on in (IS, KL):
        assert go(on, Vd=Vw, Wd=Ww, Hd=Hw) == bad
    assert np.array_equal(W, W0) and np.array_equal(H, H0)
    if na.device_count() == 0:
        # the valid forms get as far as the device: every initialisation, constant basis vectors, denseCompute = 0 (the sparse KL path)
        gone = na.ResultType.ErrorExternalLibrary
        for on in (IS, KL):
            assert go(on) == gone
            assert go(on, constant_basis_vectors=True) == gone
            for init in (na.NmfInitializationMethod.AllRandomValues, na.NmfInitializationMethod.MeanColumns, na.NmfInitializationMethod.KMeansAndRandomValues):
                assert go(on, init=init) == gone
        assert go({"divergence": 1, "denseCompute": 0}) == gone
        assert go({"divergence": 1}, constant_basis_vectors=True) == bad      # (the sparse KL path keeps refusing constant W)
