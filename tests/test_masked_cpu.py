"""Missing-value NMF without a GPU: the fp64 restatement the GPU tests compare with (against the C oracle and an independent dense
weighted form), the nmfamd_params layout on both sides of the C boundary, and the refusals nmfgpu::compute makes before it touches a device."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from oracle import oracle
from tests import masked_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS64 = float(np.finfo(np.float64).eps)


def _start(m, n, r, seed):
    rng = np.random.default_rng(seed)
    return (np.asfortranarray(1.0 - rng.random((m, r))), np.asfortranarray(1.0 - rng.random((r, n))))


def _dense_weighted(M, V, W, H, eps):
    """The same iteration as a dense weighted update: M(i, j) = number of stored copies of (i, j), V(i, j) = the sum of their values."""
    H = H * (W.T @ V) / (W.T @ (M * (W @ H)) + eps)
    W = W * (V @ H.T) / ((M * (W @ H)) @ H.T + eps)
    return ref.normalize_columns(W), H


def test_complete_omega_is_the_oracle_mu():
    m, n, r, iters = 37, 23, 5, 20
    rng = np.random.default_rng(3)
    V = np.asfortranarray(rng.random((m, n)))
    W0, H0 = _start(m, n, r, 4)
    rows, cols, vals = ref.entries_of_dense(V)
    assert len(vals) == m * n
    W, H, frob, rmsd = ref.run(rows, cols, vals, W0, H0, iters, EPS64)
    Wo, Ho = W0.copy(order="F"), H0.copy(order="F")
    res = oracle.run("mu", V, Wo, Ho, iters)
    assert np.max(np.abs(W - Wo)) <= 1e-12 * np.max(np.abs(Wo))
    assert np.max(np.abs(H - Ho)) <= 1e-12 * np.max(np.abs(Ho))
    # (the oracle evaluates the same error by the trace formula)
    assert abs(frob - res["frobenius"]) <= 1e-9 * res["frobenius"]
    assert abs(rmsd - res["rmsd"]) <= 1e-9 * res["rmsd"]


def test_restatement_is_the_dense_weighted_update():
    # empty row 2, empty column 4, a duplicated entry and explicit zeros
    m, n, r = 9, 7, 3
    rng = np.random.default_rng(5)
    rows, cols = np.nonzero(rng.random((m, n)) < 0.6)
    keep = (rows != 2) & (cols != 4)
    rows, cols = rows[keep], cols[keep]
    vals = rng.integers(0, 4, size=len(rows)).astype(np.float64)
    assert np.any(vals == 0)
    rows, cols, vals = np.append(rows, rows[3]), np.append(cols, cols[3]), np.append(vals, 2.5)
    M = np.zeros((m, n)); V = np.zeros((m, n))
    np.add.at(M, (rows, cols), 1.0); np.add.at(V, (rows, cols), vals)
    W, H = _start(m, n, r, 6)
    Wd, Hd = W.copy(), H.copy()
    for _ in range(5):
        W, H, _f = ref.iteration(rows, cols, vals, W, H, EPS64, chunk=4)
        Wd, Hd = _dense_weighted(M, V, Wd, Hd, EPS64)
    assert np.allclose(W, Wd, rtol=1e-12, atol=1e-15) and np.allclose(H, Hd, rtol=1e-12, atol=1e-15)
    assert np.all(W[2] == 0) and np.all(H[:, 4] == 0)
    assert np.all(np.isfinite(W)) and np.all(np.isfinite(H))


def test_duplicate_counts_twice_and_stored_zero_counts():
    m, n, r = 6, 5, 2
    rows, cols, vals = ref.planted_ratings(m, n, 0.7, 11)
    W0, H0 = _start(m, n, r, 12)
    base = ref.run(rows, cols, vals, W0, H0, 3, EPS64)
    dup = ref.run(np.append(rows, rows[0]), np.append(cols, cols[0]), np.append(vals, vals[0]), W0, H0, 3, EPS64)
    assert not np.allclose(base[1], dup[1])
    # a stored zero at an entry that was not observed
    free = [(i, j) for i in range(m) for j in range(n) if not np.any((rows == i) & (cols == j))]
    assert free
    i, j = free[0]
    zero = ref.run(np.append(rows, i), np.append(cols, j), np.append(vals, 0.0), W0, H0, 3, EPS64)
    assert not np.allclose(base[1], zero[1])
    # the error counts |Omega| with every copy
    assert zero[3] == pytest.approx(zero[2] / np.sqrt(len(vals) + 1), rel=1e-15)


def test_chunked_form_matches_the_whole():
    rows, cols, vals = ref.planted_ratings(60, 40, 0.2, 21)
    W0, H0 = _start(60, 40, 6, 22)
    a = ref.run(rows, cols, vals, W0, H0, 4, EPS64)
    b = ref.run(rows, cols, vals, W0, H0, 4, EPS64, chunk=17)
    assert np.allclose(a[0], b[0], rtol=1e-13) and np.allclose(a[1], b[1], rtol=1e-13) and a[2] == pytest.approx(b[2], rel=1e-13)


def test_params_layout_matches_the_header():
    from nmfgpu_amd.engine import _Params
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "probe.c"), os.path.join(td, "probe")
        open(src, "w").write(r'''
#include <nmfgpu_amd.h>
#include <stddef.h>
#include <stdio.h>
int main(void) { printf("%zu %zu\n", offsetof(nmfamd_params, missing_values), sizeof(nmfamd_params)); return 0; }
''')
        subprocess.check_call(["g++", "-x", "c++", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        off, size = map(int, subprocess.check_output([exe]).decode().split())
    assert off == _Params.missing_values.offset
    assert size == C.sizeof(_Params)
    # the last field
    assert off + 8 == size and _Params._fields_[-1][0] == "missing_values"


def _compute(V, W, H, params, **kw):
    import nmfgpu_amd as na
    return na.compute(V, W, H, iterations=3, parameters=params, **kw)


@pytest.fixture
def context():
    import nmfgpu_amd as na
    assert na.initialize() in (na.ResultType.Success, na.ResultType.ErrorAlreadyInitialized)
    na.set_verbosity(na.Verbosity.Nothing)
    yield na
    na.finalize()


def test_refusals_before_the_device(context):
    na = context
    rng = np.random.default_rng(0)
    m, n, r = 20, 12, 3
    V = np.asfortranarray(rng.random((m, n)).astype(np.float32))
    V[0, 0] = np.nan
    W = np.asfortranarray(rng.random((m, r)).astype(np.float32)); H = np.asfortranarray(rng.random((r, n)).astype(np.float32))
    W0, H0 = W.copy(), H.copy()
    bad = na.ResultType.ErrorInvalidArgument
    on = {"missingValues": 1}
    assert _compute(V, W, H, on, algorithm=na.NmfAlgorithm.GDCLS) == bad
    assert _compute(V, W, H, {**on, "lambda": 0.1}, algorithm=na.NmfAlgorithm.GDCLS) == bad
    assert _compute(V, W, H, on, algorithm=na.NmfAlgorithm.HALS) == bad
    assert _compute(V, W, H, {**on, "divergence": 1}) == bad
    assert _compute(V, W, H, {**on, "numGpus": 2}) == bad
    for init in (na.NmfInitializationMethod.MeanColumns, na.NmfInitializationMethod.KMeansAndRandomValues, na.NmfInitializationMethod.EInNMF):
        assert _compute(V, W, H, on, init=init) == bad
    assert _compute(V, W, H, {**on, "nndsvd": 0}) == bad
    for value in (2, -1, 0.5, float("nan")):
        assert _compute(V, W, H, {"missingValues": value}) == bad
    Vnan = np.asfortranarray(np.full((m, n), np.nan, dtype=np.float32))
    assert _compute(Vnan, W, H, on) == bad
    from nmfgpu_amd import api
    empty = api.sparse_description(na.StorageFormat.CSR, m, n, np.zeros(0, np.float32), np.zeros(m + 1, np.int32), np.zeros(0, np.int32))
    assert _compute(empty, W, H, on) == bad
    Vw = np.asfortranarray(rng.random((300, 280)).astype(np.float32))
    Ww = np.asfortranarray(rng.random((300, 257)).astype(np.float32)); Hw = np.asfortranarray(rng.random((257, 280)).astype(np.float32))
    assert _compute(Vw, Ww, Hw, on) == bad
    assert np.array_equal(W, W0) and np.array_equal(H, H0)
    if na.device_count() == 0:
        # the valid forms get as far as the device
        assert _compute(V, W, H, on) == na.ResultType.ErrorExternalLibrary
        assert _compute(V, W, H, on, init=na.NmfInitializationMethod.AllRandomValues) == na.ResultType.ErrorExternalLibrary
        assert _compute(V, W, H, {"missingValues": 0}) == na.ResultType.ErrorExternalLibrary
