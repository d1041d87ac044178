"""Accelerated HALS on the GPU (kernels_hals_multi.hip, docs/HALS.md "Inner sweeps"): several sweeps per product, in one launch.

Sweep level, through nmfamd_op_hals_sweeps_* at every instantiated (dtype, RP), against the fp64 sweeps of tests/hals_multi_reference.py.  As in
tests/test_gpu_hals_sweep.py no expectation assumes the kernel's lane mapping or summation order: exact results on the integer problem (s = 2 and 3), the
running-error bound carried over the sweeps on a diagonally dominant G (s = 3, plain and penalised), padding, and s = 1 against the single-sweep entry bit for bit.
tests/test_hals_multi_cpu.py checks on the CPU that these cases can tell s sweeps from s - 1 and from s restarts.

Engine level at (s_H, s_W) = (3, 2) against the restatement: tolerances from tests/hals_multi_cases.py (fp64 1e-9; fp32 4 x the distance of the fp32 numpy restatement
from the fp64 one on the same cases, pinned by the CPU test).
"""
import numpy as np
import pytest

import nmfgpu_amd as na
from tests import hals_multi_cases as mc
from tests import hals_multi_reference as multi
from tests import hals_reference as ref

pytestmark = pytest.mark.gpu

LEN_PAD = mc.LEN_PAD
CASES = [pytest.param(c, id=mc.case_id(c)) for c in mc.SWEEP_CASES]


@pytest.fixture(scope="module", autouse=True)
def _library_is_native():
    assert na.device_count() >= 1, "GPU tests need a HIP device"
    assert na.initialize() in (na.ResultType.Success, na.ResultType.ErrorAlreadyInitialized)
    na.set_verbosity(na.Verbosity.Nothing)
    yield
    na.finalize()


def launch(P, slabs, G, r, len_valid, sweeps, l1=0.0, l2=0.0, entry="sweeps"):
    """The kernel on a case: with more than one slab they lie 16 RP elements apart and the gaps hold NaN, which any read of them would carry into the result; ps
    and sumsq_part start as NaN sentinels.  entry = "sweep": the single-sweep entry of tests/test_gpu_hals_sweep.py (sweeps must be 1)."""
    S, len_pad, RP = slabs.shape
    stride = len_pad * RP + (16 * RP if S > 1 else 0)
    flat = np.full((S, stride), np.nan, dtype=P.dtype)
    flat[:, :len_pad * RP] = slabs.reshape(S, -1)
    sentinels = dict(ps=np.full(len_pad, np.nan, P.dtype), sumsq_part=np.full((len_pad // 16) * RP, np.nan, P.dtype))
    if entry == "sweep":
        assert sweeps == 1
        out = na.op_hals_sweep(P, flat, G, r, len_valid, penalties=None if l1 == 0 and l2 == 0 else (l1, l2), **sentinels)
    else:
        out = na.op_hals_sweeps(P, flat, G, r, len_valid, sweeps, l1=l1, l2=l2, **sentinels)
    assert out["parts"] == len_pad // mc.cols_and_chunk(P.dtype.type, RP)[0]
    return out


def assert_padding_is_zero(out, r, len_valid):
    P = out["P"]
    assert (P[:, r:] == 0).all() and (P[len_valid:, :] == 0).all()
    assert not np.isnan(out["ps"][:len_valid]).any() and np.isnan(out["ps"][len_valid:]).all()   # ps(y) written exactly where y < len_valid
    assert not np.isnan(out["sumsq_part"]).any()


@pytest.mark.parametrize("sweeps", mc.SWEEP_COUNTS)
@pytest.mark.parametrize("case", CASES)
def test_order_and_chunks_are_exact_over_the_sweeps(case, sweeps):
    """Tridiagonal 0 / 1 G with unit diagonal (a few zeros: skipped) and integer a, h: s fp64 sweeps are all-integer, and so must be the kernel's.  A sweep too few or
    too many, a restart from the old h, or a row of the chunk left in LDS by the end of the sweep before (where G is streamed) changes some h_k; ps and the sums of
    squares are integers too and must be those of the final state."""
    dtype, RP, r, len_valid, S = case
    P, slabs, G = ref.order_case(RP, r, LEN_PAD, len_valid, S, mc.case_rng(case, 1), dtype)
    out = launch(P, slabs, G, r, len_valid, sweeps)
    want = multi.panel_sweeps(P, slabs, G, r, len_valid, sweeps)
    got = out["P"][:len_valid, :r].astype(np.float64)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} elements differ, first (y, k) = {bad[:4].tolist()}"
    a = slabs.astype(np.float64).sum(axis=0)[:len_valid, :r]
    assert np.array_equal(out["ps"][:len_valid].astype(np.float64), (want * a).sum(axis=1)), "ps is not formed from the final h"
    colsq = np.zeros(RP)
    colsq[:r] = (want * want).sum(axis=0)
    assert np.array_equal(out["sumsq_part"].astype(np.float64).sum(axis=0), colsq), "the sums of squares are not those of the final h"
    assert_padding_is_zero(out, r, len_valid)


@pytest.mark.parametrize("l1,l2", mc.SWEEP_PENALTIES)
@pytest.mark.parametrize("case", CASES)
def test_three_sweeps_within_the_carried_error_bound(case, l1, l2):
    """Random diagonally dominant G, signed a, s = 3: every element within multi_sweep_bound of the fp64 sweeps; ps(y) = sum_k h_k a_k (the raw a) within
    gamma_{RP+S} sum_k |h_k a_k| + sum_k b_k |a_k| of the final state; the rows of sumsq_part add up to the column sums of squares of the kernel's own output."""
    dtype, RP, r, len_valid, S = case
    u = mc.UNIT[dtype]
    P, slabs, G = ref.dominant_case(RP, r, LEN_PAD, len_valid, S, mc.case_rng(case, 2), dtype)
    out = launch(P, slabs, G, r, len_valid, 3, l1, l2)
    want = multi.panel_sweeps(P, slabs, G, r, len_valid, 3, l1, l2)
    b = multi.multi_sweep_bound(P[:len_valid].T, slabs[:, :len_valid].transpose(0, 2, 1), G, r, 3, u, l1, l2).T
    got = out["P"][:len_valid, :r].astype(np.float64)
    err = np.abs(got - want)
    print(mc.case_id(case), (l1, l2), "worst error / bound", (err / np.maximum(b, 1e-300)).max())
    assert (err <= b).all(), f"worst error / bound {(err / np.maximum(b, 1e-300)).max():.3g} at {np.unravel_index(np.argmax(err - b), err.shape)}"
    a = slabs.astype(np.float64).sum(axis=0)[:len_valid, :r]
    ps_tol = ref.gamma(RP + S, u) * np.abs(want * a).sum(axis=1) + (b * np.abs(a)).sum(axis=1)
    assert (np.abs(out["ps"][:len_valid] - (want * a).sum(axis=1)) <= ps_tol).all()
    own = out["P"].astype(np.float64)
    colsq = (own * own).sum(axis=0)
    assert (np.abs(out["sumsq_part"].astype(np.float64).sum(axis=0) - colsq) <= ref.gamma(LEN_PAD, u) * colsq).all()
    assert_padding_is_zero(out, r, len_valid)


@pytest.mark.parametrize("case", CASES)
def test_padding_garbage_changes_nothing(case):
    """Finite garbage in the padding of G, P and the slabs (coordinates >= r, columns >= len_valid), three penalised sweeps: the valid block, ps and the partial
    sums of squares are those of the clean launch bit for bit, the padding of the panel comes out exactly 0 and ps(y >= len_valid) keeps its sentinel."""
    dtype, RP, r, len_valid, S = case
    rng = mc.case_rng(case, 3)
    P, slabs, G = ref.dominant_case(RP, r, LEN_PAD, len_valid, S, rng, dtype)
    clean = launch(P, slabs, G, r, len_valid, 3, 0.05, 0.01)
    dirty = launch(*ref.with_garbage(P, slabs, G, r, len_valid, rng), r, len_valid, 3, 0.05, 0.01)
    assert np.array_equal(dirty["P"][:len_valid, :r], clean["P"][:len_valid, :r])
    assert (dirty["P"][:, r:] == 0).all(), "coordinates >= r are not 0"
    assert (dirty["P"][len_valid:, :] == 0).all(), "columns >= len_valid are not 0"
    assert np.array_equal(dirty["ps"][:len_valid], clean["ps"][:len_valid]) and np.isnan(dirty["ps"][len_valid:]).all()
    assert np.array_equal(dirty["sumsq_part"], clean["sumsq_part"]), "padding columns reach the partial sums of squares"


@pytest.mark.parametrize("l1,l2", mc.SWEEP_PENALTIES)
@pytest.mark.parametrize("case", CASES)
def test_one_sweep_is_the_single_sweep_entry(case, l1, l2):
    """sweeps = 1 through the new entry is op_hals_sweep bit for bit, ps and sumsq_part included (the launcher forwards it to the single-sweep kernel)."""
    dtype, RP, r, len_valid, S = case
    rng = mc.case_rng(case, 4)
    P, slabs, G = ref.with_garbage(*ref.dominant_case(RP, r, LEN_PAD, len_valid, S, rng, dtype), r, len_valid, rng)
    old = launch(P, slabs, G, r, len_valid, 1, l1, l2, entry="sweep")
    new = launch(P, slabs, G, r, len_valid, 1, l1, l2)
    assert np.array_equal(new["P"], old["P"]) and np.array_equal(new["sumsq_part"], old["sumsq_part"])
    assert np.array_equal(new["ps"][:len_valid], old["ps"][:len_valid]) and np.isnan(new["ps"][len_valid:]).all()
    assert_padding_is_zero(new, r, len_valid)


# ------------------------------------------------------------------ engine level

def as_csr(coo, m, n):
    rows, cols, vals = coo
    ptr = np.zeros(m + 1, np.int32)
    np.cumsum(np.bincount(rows, minlength=m), out=ptr[1:])
    return vals, ptr, cols.astype(np.int32)


def make_engine(case, **kw):
    """The engine of an engine case with its V uploaded and its start set, and the case's (V, W, H, penalties, constant_w)."""
    kind, m, n, r, dtype = case
    coo, V, W, H, p, constant_w = mc.engine_problem(case)
    eng = na.Engine(m, n, r, "hals", dtype=dtype, sparse_compute=coo is not None, l1_w=p[0], l1_h=p[1], l2_w=p[2], l2_h=p[3], **kw)
    if coo is not None:
        eng.upload_sparse(1, *as_csr(coo, m, n), 0)
    else:
        eng.upload(V)
    eng.set_factors(W, H)
    return eng, V, W, H, p, constant_w


def check_padding(eng):
    g = eng.geometry()
    RP, mp, np_ = g["padded_rank"], g["padded_m"], g["padded_n"]
    Wt = eng.debug_read(0, RP * mp).reshape(mp, RP)
    Hp = eng.debug_read(1, RP * np_).reshape(np_, RP)
    assert (Wt[:, eng.r:] == 0).all() and (Wt[eng.m:, :] == 0).all()
    assert (Hp[:, eng.r:] == 0).all() and (Hp[eng.n:, :] == 0).all()


@pytest.mark.parametrize("case", [pytest.param(c, id=mc.engine_case_id(c)) for c in mc.ENGINE_CASES])
def test_engine_parity_with_restatement(case):
    """(s_H, s_W) = (3, 2): the factors after 1 and 10 iterations against the fp64 restatement, dense and sparse compute, penalised, constant W."""
    dtype = case[4]
    tol = mc.TOL_F64 if dtype == np.float64 else mc.MARGIN * mc.FIGURE_ENGINE_FACTORS
    eng, V, W, H, p, constant_w = make_engine(case, sweeps_h=mc.SWEEPS_H, sweeps_w=mc.SWEEPS_W)
    done = 0
    for iters in mc.ENGINE_ITERS:
        eng.iterate(iters - done, first_iteration=done + 1, error_every=0, last_iteration=iters, constant_w=constant_w)
        done = iters
        Wg, Hg = eng.get_factors()
        W64, H64, _ = mc.restated(case, iters)
        print(mc.engine_case_id(case), iters, "W", mc.rel(Wg, W64), "H", mc.rel(Hg, H64), "tolerance", tol)
        if constant_w:
            assert np.array_equal(Wg, W)
        else:
            assert mc.rel(Wg, W64) < tol, (iters, mc.rel(Wg, W64))
        assert mc.rel(Hg, H64) < tol, (iters, mc.rel(Hg, H64))
    check_padding(eng)
    eng.close()


@pytest.mark.parametrize("dtype,tol", [(np.float32, 1e-5), (np.float64, 1e-9)])
@pytest.mark.parametrize("constant_w", [False, True])
def test_reported_error_on_random_v(dtype, tol, constant_w):
    """Uniformly random V (a residual large enough for the fp32 trace formula): the reported error after 1 and 10 iterations at (3, 2) is the restatement's,
    ||V - W H|| with the W of the H step and the H after the LAST inner sweep (ps comes from the final h)."""
    V, W, H = mc.problem(500, 300, 33, dtype, seed=833)
    eng = na.Engine(500, 300, 33, "hals", dtype=dtype, sweeps_h=mc.SWEEPS_H, sweeps_w=mc.SWEEPS_W)
    eng.upload(V)
    eng.set_factors(W, H)
    _, _, errs = multi.run(V.astype(np.float64), W, H, 10, mc.SWEEPS_H, mc.SWEEPS_W, constant_w=constant_w)
    done = 0
    for iters in (1, 10):
        eng.iterate(iters - done, first_iteration=done + 1, error_every=0, last_iteration=iters, constant_w=constant_w)
        done = iters
        print(np.dtype(dtype).name, constant_w, iters, "reported", eng.frobenius, "restated", errs[iters - 1])
        assert abs(eng.frobenius - errs[iters - 1]) <= tol * errs[iters - 1], (iters, eng.frobenius, errs[iters - 1])
    eng.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("penalised", [False, True])
def test_counts_of_one_change_nothing(dtype, penalised):
    """An engine that was never given counts and one after set_sweeps(1, 1) (having run at other counts in between is not needed: the counts are plain state)
    produce bit-identical factors and errors over 5 iterations."""
    V, W, H = mc.planted(300, 257, 70, dtype, seed=5)
    p = dict(l1_w=0.05, l1_h=0.05, l2_w=0.01, l2_h=0.01) if penalised else {}
    out = []
    for give in (False, True):
        eng = na.Engine(300, 257, 70, "hals", dtype=dtype, **p)
        eng.upload(V)
        eng.set_factors(W, H)
        if give:
            eng.set_sweeps(4, 3)
            eng.set_sweeps(1, 1)
        errs = []
        for it in range(1, 6):
            eng.iterate(1, first_iteration=it, error_every=1)
            errs.append(eng.frobenius)
        out.append((*eng.get_factors(), errs))
        eng.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]


def test_set_sweeps_takes_effect_at_the_next_iteration():
    """One iteration at (1, 1), then set_sweeps(3, 2) and one more: the restatement with the same schedule, fp64 at 1e-9."""
    V, W, H = mc.planted(300, 257, 70, np.float64, seed=6)
    eng = na.Engine(300, 257, 70, "hals", dtype=np.float64)
    eng.upload(V)
    eng.set_factors(W, H)
    eng.iterate(1, error_every=0)
    eng.set_sweeps(3, 2)
    eng.iterate(1, first_iteration=2, error_every=0, last_iteration=2)
    Wg, Hg = eng.get_factors()
    W64, H64, _ = multi.run(V, W, H, 1)
    W64, H64, errs = multi.run(V, W64, H64, 1, 3, 2)
    assert mc.rel(Wg, W64) < 1e-9 and mc.rel(Hg, H64) < 1e-9 and abs(eng.frobenius - errs[0]) <= 1e-9 * errs[0]
    eng.close()


def test_compute_takes_the_counts():
    V, W, H = mc.planted(300, 257, 20, np.float64, seed=7)
    W64, H64, errs = multi.run(V, W, H, 5, 3, 2)
    s = na.Summary()
    res = na.compute(V, W, H, algorithm=na.NmfAlgorithm.HALS, iterations=5, parameters={"sweepsH": 3, "sweepsW": 2}, summary=s)
    assert res == na.ResultType.Success, res
    assert mc.rel(W, W64) < 1e-9 and mc.rel(H, H64) < 1e-9, (mc.rel(W, W64), mc.rel(H, H64))
    assert abs(s.record(0).frobenius - errs[-1]) <= 1e-9 * errs[-1]


# ------------------------------------------------------------------ refusals

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bad_counts_are_refused(dtype):
    for bad in (0, 65, -1):
        for h, w in ((bad, 1), (1, bad)):
            with pytest.raises(na.EngineError) as info:
                na.Engine(60, 50, 8, "hals", dtype=dtype, sweeps_h=h, sweeps_w=w)
            assert info.value.status == 1, (h, w)
    eng = na.Engine(60, 50, 8, "hals", dtype=dtype)
    for bad in (0, 65, -1):
        for h, w in ((bad, 1), (1, bad)):
            with pytest.raises(na.EngineError) as info:
                eng.set_sweeps(h, w)
            assert info.value.status == 1 and "sweeps" in str(info.value), (h, w, str(info.value))
    eng.set_sweeps(64, 64)
    eng.set_sweeps(1, 1)
    eng.close()
    P, G = np.zeros((128, 64), dtype), np.eye(64, dtype=dtype)
    for bad in (0, 65, -1):
        with pytest.raises(na.EngineError) as info:
            na.op_hals_sweeps(P, np.zeros((1, 128 * 64), dtype), G, 1, 128, bad)
        assert info.value.status == 1, bad
    na.op_hals_sweeps(P, np.zeros((1, 128 * 64), dtype), G, 1, 128, 64)


def test_other_engines_take_only_one():
    for kw in (dict(algorithm="mu"), dict(algorithm="mu", divergence="is"), dict(algorithm="als")):
        eng = na.Engine(60, 50, 8, **kw)
        with pytest.raises(na.EngineError) as info:
            eng.set_sweeps(2, 1)
        assert info.value.status == 1 and "HALS" in str(info.value), kw
        eng.set_sweeps(1, 1)
        eng.close()
        with pytest.raises(na.EngineError):
            na.Engine(60, 50, 8, sweeps_h=2, **kw)
        na.Engine(60, 50, 8, sweeps_h=1, sweeps_w=1, **kw).close()


def test_compute_refusals():
    V, W, H = mc.problem(300, 200, 8, np.float32)
    bad = na.ResultType.ErrorInvalidArgument
    assert na.compute(V, W, H, algorithm=na.NmfAlgorithm.HALS, iterations=3, parameters={"sweepsH": 2.5}) == bad
    assert na.compute(V, W, H, algorithm=na.NmfAlgorithm.HALS, iterations=3, parameters={"sweepsH": 0}) == bad
    assert na.compute(V, W, H, algorithm=na.NmfAlgorithm.Multiplicative, iterations=3, parameters={"sweepsH": 2}) == bad
    assert na.compute(V, W, H, algorithm=na.NmfAlgorithm.Multiplicative, iterations=3, parameters={"sweepsH": 1, "sweepsW": 1}) == na.ResultType.Success
