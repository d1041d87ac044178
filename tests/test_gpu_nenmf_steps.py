"""The NeNMF step kernel on the GPU (kernels_nenmf.hip, docs/NENMF.md) through nmfamd_op_apg_steps_* at every instantiated (dtype, RP), against the fp64 steps of
tests/nenmf_reference.py on the problems of tests/nenmf_cases.py.  No expectation assumes the kernel's tiling or summation order: the tolerances are those of
tests/nenmf_cases.py (fp64 1e-9; fp32 4 x the distance of the fp32 numpy steps from the fp64 ones, pinned by tests/test_nenmf_cpu.py, which also shows that they tell a
step too few, lost momentum, Y for P and a dropped penalty from the real thing)."""
import numpy as np
import pytest

import nmfgpu_amd as na
from tests import hals_reference as ref
from tests import nenmf_cases as nc

pytestmark = pytest.mark.gpu

CASES = [pytest.param(c, id=nc.case_id(c)) for c in nc.STEP_CASES]


@pytest.fixture(scope="module", autouse=True)
def _library_is_native():
    assert na.device_count() >= 1, "GPU tests need a HIP device"
    yield


def launch(P, slabs, G, r, len_valid, steps, l1=0.0, l2=0.0):
    """The kernel on a case: with more than one slab they lie 16 RP elements apart and the gaps hold NaN, which any read of them would carry into the result; ps
    and sumsq_part start as NaN sentinels, so that entries the kernel does not own show."""
    S, len_pad, RP = slabs.shape
    stride = len_pad * RP + (16 * RP if S > 1 else 0)
    flat = np.full((S, stride), np.nan, dtype=P.dtype)
    flat[:, :len_pad * RP] = slabs.reshape(S, -1)
    out = na.op_apg_steps(P, flat, G, r, len_valid, steps, l1=l1, l2=l2, ps=np.full(len_pad, np.nan, P.dtype),
                          sumsq_part=np.full((len_pad // 16) * RP, np.nan, P.dtype))
    assert out["parts"] == len_pad // nc.TILE[P.dtype.type]
    return out


def check_against_restatement(out, want, slabs, case, tol):
    dtype, RP, r, len_valid, S = case
    u = 2.0 ** -24 if dtype == np.float32 else 2.0 ** -53
    a = slabs.astype(np.float64).sum(axis=0)[:len_valid, :r]
    a_abs = np.abs(slabs.astype(np.float64)).sum(axis=0)[:len_valid, :r]      # (the slabs may cancel: their sum is rounded relative to this)
    got = out["P"][:len_valid, :r].astype(np.float64)
    d = nc.rel(got, want)
    print(nc.case_id(case), "distance", d, "tolerance", tol)
    assert d < tol, d
    # ps(y) = sum_k p(k, y) a(k, y) with the raw slabs, from the kernel's own final panel: any order of the sum over k and over the slabs
    ps_want = (got * a).sum(axis=1)
    ps_tol = ref.gamma(RP + S, u) * (np.abs(got) * a_abs).sum(axis=1) + 1e-300
    assert (np.abs(out["ps"][:len_valid] - ps_want) <= ps_tol).all(), "ps is not sum_k p_T(k) a(k)"
    own = out["P"].astype(np.float64)
    colsq = (own * own).sum(axis=0)
    assert (np.abs(out["sumsq_part"].astype(np.float64).sum(axis=0) - colsq) <= ref.gamma(nc.LEN_PAD, u) * colsq).all(), "the sums of squares are not those of P_T"
    # what the kernel owns and what it does not
    assert (out["P"][:, r:] == 0).all() and (out["P"][len_valid:, :] == 0).all(), "padding is not exactly 0"
    assert not np.isnan(out["ps"][:len_valid]).any() and np.isnan(out["ps"][len_valid:]).all(), "ps(y) is written exactly where y < len_valid"
    assert not np.isnan(out["sumsq_part"]).any() and (out["sumsq_part"][:, r:] == 0).all()


@pytest.mark.parametrize("l1,l2", nc.STEP_PENALTIES)
@pytest.mark.parametrize("steps", nc.STEP_COUNTS)
@pytest.mark.parametrize("case", CASES)
def test_steps_match_the_restatement(case, steps, l1, l2):
    """1 step (no extrapolation), 2 (one) and 5 (several), plain and penalised: the panel within the tolerance of the fp64 steps; ps, the partial sums of squares and
    the number of parts; exact zeros on the padding; sentinels where the kernel owns nothing."""
    P, slabs, G = nc.step_problem(case)
    out = launch(P, slabs, G, case[2], case[3], steps, l1, l2)
    want, _ = nc.restated_steps(case, steps, l1, l2)
    check_against_restatement(out, want, slabs, case, nc.step_tolerance(case))


@pytest.mark.parametrize("case", CASES)
def test_padding_garbage_changes_nothing(case):
    """Finite garbage in the padding of G, P and the slabs (coordinates >= r, columns >= len_valid), five penalised steps: the valid block, ps and the partial sums
    of squares are those of the clean launch bit for bit and the padding of the panel comes out exactly 0."""
    dtype, RP, r, len_valid, S = case
    P, slabs, G = nc.step_problem(case)
    clean = launch(P, slabs, G, r, len_valid, 5, 0.05, 0.01)
    dirty = launch(*ref.with_garbage(P, slabs, G, r, len_valid, nc.case_rng(case, 3)), r, len_valid, 5, 0.05, 0.01)
    assert np.array_equal(dirty["P"], clean["P"])
    assert (dirty["P"][:, r:] == 0).all() and (dirty["P"][len_valid:, :] == 0).all()
    assert np.array_equal(dirty["ps"][:len_valid], clean["ps"][:len_valid]) and np.isnan(dirty["ps"][len_valid:]).all()
    assert np.array_equal(dirty["sumsq_part"], clean["sumsq_part"]), "padding reaches the partial sums of squares"


@pytest.mark.parametrize("case", CASES)
def test_result_does_not_depend_on_len_pad(case):
    """The same columns in a panel of 256 and of 384: bit for bit the same on the shared columns (L is one value per launch, computed the same way by every workgroup,
    and nothing crosses workgroups)."""
    dtype, RP, r, len_valid, S = case
    P, slabs, G = nc.step_problem(case)
    small = launch(P, slabs, G, r, len_valid, 5, 0.05, 0.01)
    P2 = np.zeros((384, RP), dtype)
    P2[:256] = P
    slabs2 = np.zeros((S, 384, RP), dtype)
    slabs2[:, :256] = slabs
    large = launch(P2, slabs2, G, r, len_valid, 5, 0.05, 0.01)
    assert np.array_equal(large["P"][:256], small["P"]) and (large["P"][256:] == 0).all()
    assert np.array_equal(large["ps"][:len_valid], small["ps"][:len_valid])
    k = small["parts"]
    assert np.array_equal(large["sumsq_part"][:k], small["sumsq_part"]) and (large["sumsq_part"][k:] == 0).all()


@pytest.mark.parametrize("steps", (1, 5))
def test_zero_g_leaves_the_panel(steps):
    """G = 0: L <= 0 and no step is taken; the valid block keeps its values, the padding is 0, ps and the sums of squares describe that panel."""
    case = nc.ZERO_G_CASE
    dtype, RP, r, len_valid, S = case
    P, slabs, G = nc.step_problem(case, zero_g=True)
    out = launch(P, slabs, G, r, len_valid, steps)
    assert np.array_equal(out["P"], P)
    check_against_restatement(out, P[:len_valid, :r].astype(np.float64), slabs, case, 1e-300 + nc.step_tolerance(case))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_launcher_refusals(dtype):
    P, G, slab = np.zeros((128, 64), dtype), np.eye(64, dtype=dtype), np.zeros((1, 128 * 64), dtype)
    for bad in (0, 257, -1):
        with pytest.raises(na.EngineError) as info:
            na.op_apg_steps(P, slab, G, 1, 128, bad)
        assert info.value.status == 1, bad
    na.op_apg_steps(P, slab, G, 1, 128, 256)
    for RP in (32, 192, 256):      # no instantiation
        with pytest.raises(na.EngineError) as info:
            na.op_apg_steps(np.zeros((128, RP), dtype), np.zeros((1, 128 * RP), dtype), np.eye(RP, dtype=dtype), 1, 128, 2)
        assert info.value.status == 1, RP
    for l1, l2 in ((-0.1, 0.0), (0.0, -0.1), (float("nan"), 0.0), (0.0, float("nan")), (float("inf"), 0.0)):
        with pytest.raises(na.EngineError) as info:
            na.op_apg_steps(P, slab, G, 1, 128, 2, l1=l1, l2=l2)
        assert info.value.status == 1, (l1, l2)
    with pytest.raises(ValueError):
        na.op_apg_steps(P, slab, G, 1, 128, 2.5)
