"""NeNMF on the GPU at engine level (docs/NENMF.md): the engine cases of tests/nenmf_cases.py at (steps_h, steps_w) = (5, 3) against tests/nenmf_reference.py (fp64
1e-9; fp32 4 x the distance of the fp32 numpy restatement from the fp64 one, pinned by tests/test_nenmf_cpu.py), the three sparse uploads, nmfgpu::compute, set_steps,
and every refusal of the interface with the word that names its cause."""
import numpy as np
import pytest

import nmfgpu_amd as na
from tests import hals_multi_cases as mc
from tests import nenmf_cases as nc
from tests import nenmf_reference as nenmf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _library_is_native():
    assert na.device_count() >= 1, "GPU tests need a HIP device"
    assert na.initialize() in (na.ResultType.Success, na.ResultType.ErrorAlreadyInitialized)
    na.set_verbosity(na.Verbosity.Nothing)
    yield
    na.finalize()


def as_csr(coo, m, n):
    rows, cols, vals = coo
    ptr = np.zeros(m + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=m), out=ptr[1:])
    return vals, ptr, cols.astype(np.int32)


def as_csc(coo, m, n):
    rows, cols, vals = coo
    order = np.lexsort((rows, cols))
    ptr = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(cols, minlength=n), out=ptr[1:])
    return vals[order], ptr, rows[order].astype(np.int32)


def make_engine(case, fmt=1, **kw):
    """The engine of an engine case with its V uploaded and its start set, and the case's (V, W, H, penalties, constant_w)."""
    kind, m, n, r, dtype = case
    coo, V, W, H, p, constant_w = nc.engine_problem(case)
    eng = na.Engine(m, n, r, "nenmf", dtype=dtype, sparse_compute=coo is not None, l1_w=p[0], l1_h=p[1], l2_w=p[2], l2_h=p[3], **kw)
    if coo is None:
        eng.upload(V)
    elif fmt == 1:
        eng.upload_sparse(1, *as_csr(coo, m, n), 0)
    elif fmt == 2:
        eng.upload_sparse(2, *as_csc(coo, m, n), 0)
    else:
        eng.upload_sparse(3, coo[2], coo[0], coo[1], 0)
    eng.set_factors(W, H)
    return eng, V, W, H, p, constant_w


def check_padding(eng):
    g = eng.geometry()
    RP, mp, np_ = g["padded_rank"], g["padded_m"], g["padded_n"]
    Wt = eng.debug_read(0, RP * mp).reshape(mp, RP)
    Hp = eng.debug_read(1, RP * np_).reshape(np_, RP)
    assert (Wt[:, eng.r:] == 0).all() and (Wt[eng.m:, :] == 0).all()
    assert (Hp[:, eng.r:] == 0).all() and (Hp[eng.n:, :] == 0).all()


@pytest.mark.parametrize("case", [pytest.param(c, id=nc.engine_case_id(c)) for c in nc.ENGINE_CASES])
def test_engine_parity_with_restatement(case):
    """(5, 3): W, H and the reported error after 1 and 10 iterations against the fp64 restatement -- dense and sparse compute, penalised, constant W.  The generic
    launch sequence (fused_launches == 0)."""
    dtype = case[4]
    tol = nc.engine_tolerance(case)
    eng, V, W, H, p, constant_w = make_engine(case, steps_h=nc.STEPS_H, steps_w=nc.STEPS_W)
    assert eng.geometry()["fused_launches"] == 0
    done = 0
    for iters in nc.ENGINE_ITERS:
        eng.iterate(iters - done, first_iteration=done + 1, error_every=0, last_iteration=iters, constant_w=constant_w)
        done = iters
        Wg, Hg = eng.get_factors()
        W64, H64, errs = nc.restated(case, iters)
        print(nc.engine_case_id(case), iters, "W", nc.rel(Wg, W64), "H", nc.rel(Hg, H64), "tolerance", tol, "error", eng.frobenius, errs[-1])
        if constant_w:
            assert np.array_equal(Wg, W)
        else:
            assert nc.rel(Wg, W64) < tol, (iters, nc.rel(Wg, W64))
        assert nc.rel(Hg, H64) < tol, (iters, nc.rel(Hg, H64))
        if dtype == np.float64:
            assert abs(eng.frobenius - errs[-1]) <= 1e-9 * errs[-1], (iters, eng.frobenius, errs[-1])
    check_padding(eng)
    eng.close()


@pytest.mark.parametrize("dtype,tol", [(np.float32, 1e-5), (np.float64, 1e-9)])
@pytest.mark.parametrize("constant_w", [False, True])
def test_reported_error_on_random_v(dtype, tol, constant_w):
    """Uniformly random V (a residual large enough for the fp32 trace formula, as in tests/test_gpu_hals_multi.py): the reported error after 1 and 10 iterations is
    ||V - W H|| with the W of the H step and the H after the last step."""
    V, W, H = mc.problem(500, 300, 33, dtype, seed=833)
    eng = na.Engine(500, 300, 33, "nenmf", dtype=dtype, steps_h=nc.STEPS_H, steps_w=nc.STEPS_W)
    eng.upload(V)
    eng.set_factors(W, H)
    _, _, errs = nenmf.run(V.astype(np.float64), W, H, 10, nc.STEPS_H, nc.STEPS_W, constant_w=constant_w)
    done = 0
    for iters in (1, 10):
        eng.iterate(iters - done, first_iteration=done + 1, error_every=0, last_iteration=iters, constant_w=constant_w)
        done = iters
        print(np.dtype(dtype).name, constant_w, iters, "reported", eng.frobenius, "restated", errs[iters - 1])
        assert abs(eng.frobenius - errs[iters - 1]) <= tol * errs[iters - 1], (iters, eng.frobenius, errs[iters - 1])
    eng.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_sparse_uploads_are_bit_identical(dtype):
    case = ("sparse", 300, 257, 70, dtype)
    out = []
    for fmt in (1, 2, 3):
        eng, *_ = make_engine(case, fmt=fmt, steps_h=nc.STEPS_H, steps_w=nc.STEPS_W)
        eng.iterate(3, error_every=0, last_iteration=3)
        out.append((*eng.get_factors(), eng.frobenius))
        eng.close()
    for other in out[1:]:
        assert np.array_equal(other[0], out[0][0]) and np.array_equal(other[1], out[0][1]) and other[2] == out[0][2]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_compute_with_parameters_is_the_engine_with_set_steps(dtype):
    V, W, H = mc.planted(300, 257, 20, dtype, seed=7)
    eng = na.Engine(300, 257, 20, "nenmf", dtype=dtype)
    eng.set_steps(6, 4)
    eng.upload(V)
    eng.set_factors(W, H)
    eng.iterate(5, error_every=0, last_iteration=5)
    We, He = eng.get_factors()
    err = eng.frobenius
    eng.close()
    Wc, Hc = W.copy(order="F"), H.copy(order="F")
    s = na.Summary()
    res = na.compute(V, Wc, Hc, algorithm=na.NmfAlgorithm.NeNMF, iterations=5, parameters={"stepsH": 6, "stepsW": 4}, summary=s)
    assert res == na.ResultType.Success, res
    assert np.array_equal(Wc, We) and np.array_equal(Hc, He)
    assert abs(s.record(0).frobenius - err) <= 1e-12 * err
    if dtype == np.float64:
        W64, H64, errs = nenmf.run(V, W, H, 5, 6, 4)
        assert nc.rel(Wc, W64) < 1e-9 and nc.rel(Hc, H64) < 1e-9 and abs(err - errs[-1]) <= 1e-9 * errs[-1]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_set_steps_between_iterations_is_a_fresh_engine_with_those_counts(dtype):
    """Two iterations at the default (8, 8), then set_steps(3, 2) and two more: bit for bit a fresh engine created with (3, 2) and started from the factors after
    the first two.  The default is 8: an engine given (8, 8) explicitly is the one given nothing."""
    V, W, H = mc.planted(300, 257, 70, dtype, seed=6)
    eng = na.Engine(300, 257, 70, "nenmf", dtype=dtype)
    eng.upload(V)
    eng.set_factors(W, H)
    eng.iterate(2, error_every=0)
    W2, H2 = eng.get_factors()
    eng.set_steps(3, 2)
    eng.iterate(2, first_iteration=3, error_every=0, last_iteration=4)
    Wa, Ha = eng.get_factors()
    ea = eng.frobenius
    eng.close()
    fresh = na.Engine(300, 257, 70, "nenmf", dtype=dtype, steps_h=3, steps_w=2)
    fresh.upload(V)
    fresh.set_factors(W2, H2)
    fresh.iterate(2, first_iteration=3, error_every=0, last_iteration=4)
    Wb, Hb = fresh.get_factors()
    assert np.array_equal(Wa, Wb) and np.array_equal(Ha, Hb) and ea == fresh.frobenius
    fresh.close()
    given = na.Engine(300, 257, 70, "nenmf", dtype=dtype, steps_h=8, steps_w=8)
    given.upload(V)
    given.set_factors(W, H)
    given.iterate(2, error_every=0)
    Wg, Hg = given.get_factors()
    given.close()
    assert np.array_equal(Wg, W2) and np.array_equal(Hg, H2)


# ------------------------------------------------------------------ refusals

def refused(call, word):
    with pytest.raises(na.EngineError) as info:
        call()
    assert info.value.status == 1 and word in str(info.value), str(info.value)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bad_counts_are_refused(dtype):
    for bad in (0, 257, -1):
        for h, w in ((bad, 8), (8, bad)):
            refused(lambda: na.Engine(60, 50, 8, "nenmf", dtype=dtype, steps_h=h, steps_w=w), "steps")
    eng = na.Engine(60, 50, 8, "nenmf", dtype=dtype)
    for bad in (0, 257, -1):
        for h, w in ((bad, 8), (8, bad)):
            refused(lambda: eng.set_steps(h, w), "steps")
    with pytest.raises(ValueError):
        eng.set_steps(2.5, 1)
    eng.set_steps(256, 1)
    eng.set_steps(1, 256)
    # the HALS setters: penalties are shared, sweep counts and the sweep tolerance are not
    eng.set_penalties(0.1, 0.0, 0.0, 0.2)
    eng.set_penalties()
    eng.set_sweeps(1, 1)
    refused(lambda: eng.set_sweeps(2, 1), "HALS")
    eng.set_sweep_tolerance(0.0)
    refused(lambda: eng.set_sweep_tolerance(0.1), "HALS")
    refused(lambda: eng.sweep_counts(0), "HALS")
    eng.close()


def test_ranks_without_a_step_kernel_are_refused_at_creation():
    refused(lambda: na.Engine(300, 200, 129, "nenmf", dtype=np.float32), "rank")
    refused(lambda: na.Engine(300, 200, 129, "nenmf", dtype=np.float64), "rank")
    na.Engine(300, 200, 128, "nenmf", dtype=np.float64).close()
    V, W, H = mc.problem(300, 200, 129, np.float32)
    assert na.compute(V, W, H, algorithm=na.NmfAlgorithm.NeNMF, iterations=2) == na.ResultType.ErrorInvalidArgument


def test_limits_are_those_of_hals():
    refused(lambda: na.Engine(60, 50, 8, "nenmf", divergence="kl"), "Frobenius")
    refused(lambda: na.Engine(60, 50, 8, "nenmf", missing_values=True), "missing")
    na.Engine(60, 50, 8, "nenmf", sparse_compute=True).close()
    import torch
    eng = na.Engine(60, 50, 8, "nenmf")
    ex = torch.zeros(eng.geometry()["exchange_count"], dtype=torch.float32, device="cuda")
    for call in (lambda: eng.h_step(False), lambda: eng.w_products(ex.data_ptr()), lambda: eng.w_finish(ex.data_ptr(), False)):
        refused(call, "three-phase")
    eng.close()


def test_other_engines_refuse_the_counts():
    for kw in (dict(algorithm="hals"), dict(algorithm="mu"), dict(algorithm="mu", divergence="is"), dict(algorithm="als")):
        eng = na.Engine(60, 50, 8, **kw)
        refused(lambda: eng.set_steps(8, 8), "NeNMF")
        eng.close()
        refused(lambda: na.Engine(60, 50, 8, steps_h=4, **kw), "NeNMF")


def test_compute_refusals():
    V, W, H = mc.problem(300, 200, 8, np.float32)
    bad = na.ResultType.ErrorInvalidArgument
    nen = dict(algorithm=na.NmfAlgorithm.NeNMF, iterations=3)
    assert na.compute(V, W, H, parameters={"stepsH": 2.5}, **nen) == bad
    assert na.compute(V, W, H, parameters={"stepsW": 0}, **nen) == bad
    assert na.compute(V, W, H, parameters={"stepsW": 257}, **nen) == bad
    assert na.compute(V, W, H, parameters={"sweepsH": 2}, **nen) == bad
    assert na.compute(V, W, H, parameters={"numGpus": 2}, **nen) == bad
    assert na.compute(V, W, H, algorithm=na.NmfAlgorithm.HALS, iterations=3, parameters={"stepsH": 8}) == bad
    assert na.compute(V, W, H, algorithm=na.NmfAlgorithm.Multiplicative, iterations=3, parameters={"stepsW": 8}) == bad
    assert na.compute(V, W, H, parameters={"stepsH": 1, "stepsW": 256, "l1H": 0.01}, **nen) == na.ResultType.Success
