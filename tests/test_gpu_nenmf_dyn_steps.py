"""Per-column dynamic stopping of NeNMF's projected-gradient steps on the GPU, kernel level (kernels_nenmf_dyn.hip, docs/NENMF.md "Dynamic stopping"):
k_apg_steps_dyn through nmfamd_op_apg_steps_dyn_* at every instantiated (dtype, RP), against tests/nenmf_dyn_reference.py on the inputs of
tests/nenmf_dyn_cases.py (tests/test_nenmf_dyn_cpu.py shows on the CPU that these inputs give diverse counts and keep an fp32 run within the cap on threshold flips).

Values and rule are checked separately.  Values: the restatement is run again with the KERNEL's counts forced per column, and every valid column must lie within
the tolerance of the case (fp64 1e-9; fp32 4 x the distance of the fp32 numpy restatement from the fp64 one, pinned by the CPU test), relative to the norm of the
column.  Rule: the kernel's counts equal the restatement's own for at least 98 % of the valid columns (a column on the threshold may freeze one step apart).
"""
import numpy as np
import pytest

import nmfgpu_amd as na
from tests import hals_multi_cases as mc
from tests import hals_reference as ref
from tests import nenmf_dyn_cases as dc
from tests import nenmf_dyn_reference as dyn

pytestmark = pytest.mark.gpu

LEN_VALID = dc.LEN_VALID
CASES = [pytest.param(c, id=dc.case_id(c)) for c in dc.STEP_CASES]


@pytest.fixture(scope="module", autouse=True)
def _library_is_native():
    assert na.device_count() >= 1, "GPU tests need a HIP device"
    assert na.initialize() in (na.ResultType.Success, na.ResultType.ErrorAlreadyInitialized)
    na.set_verbosity(na.Verbosity.Nothing)
    yield
    na.finalize()


def launch(P, slabs, G, r, steps, tol, l1=0.0, l2=0.0, static=False):
    """The kernel on a case: the slabs lie 16 RP elements apart where there are several, and the gaps, the slab rows of the padding columns and the padding columns
    of the panel hold NaN, which any use of them would carry into the result; ps and sumsq_part start as NaN sentinels.  static: op_apg_steps instead."""
    S, len_pad, RP = slabs.shape
    slabs = slabs.copy()
    slabs[:, LEN_VALID:, :] = np.nan
    P = P.copy()
    P[LEN_VALID:, :] = np.nan
    stride = len_pad * RP + (16 * RP if S > 1 else 0)
    flat = np.full((S, stride), np.nan, dtype=P.dtype)
    flat[:, :len_pad * RP] = slabs.reshape(S, -1)
    sentinels = dict(ps=np.full(len_pad, np.nan, P.dtype), sumsq_part=np.full((len_pad // 16) * RP, np.nan, P.dtype))
    if static:
        out = na.op_apg_steps(P, flat, G, r, LEN_VALID, steps, l1=l1, l2=l2, **sentinels)
    else:
        out = na.op_apg_steps_dyn(P, flat, G, r, LEN_VALID, steps, tol, l1=l1, l2=l2, **sentinels)
    assert out["parts"] == len_pad // dc.TILE[P.dtype.type]
    return out


def assert_padding_and_no_nan(out, r):
    P = out["P"]
    assert (P[:, r:] == 0).all(), "coordinates >= r are not 0"
    assert (P[LEN_VALID:, :] == 0).all(), "padding columns are not 0"
    assert not np.isnan(P).any() and not np.isnan(out["sumsq_part"]).any()
    assert not np.isnan(out["ps"][:LEN_VALID]).any() and np.isnan(out["ps"][LEN_VALID:]).all()      # (ps(y) is written exactly where y < len_valid)
    if "counts" in out:
        assert (out["counts"][LEN_VALID:] == 0).all(), "padding columns have a count"


def same_results(a, b):
    return (np.array_equal(a["P"], b["P"]) and np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["sumsq_part"], b["sumsq_part"])
            and np.array_equal(a["ps"][:LEN_VALID], b["ps"][:LEN_VALID]))


@pytest.mark.parametrize("l1,l2", dc.PENALTIES)
@pytest.mark.parametrize("case", CASES)
def test_values_rule_padding_and_repeat(case, l1, l2):
    dtype, RP, r, S = case
    tol = dc.step_tolerance(case)
    _, counts_own = dc.restated(case, l1, l2)
    assert dc.diversity_faults(case, counts_own) == []
    P, slabs, G = dc.step_case(case, l1, l2)
    out = launch(P, slabs, G, r, dc.MAX_STEPS, dc.TOL, l1, l2)
    counts = out["counts"][:LEN_VALID]
    same = float((counts == counts_own).mean())
    print(dc.case_id(case), (l1, l2), "kernel counts", np.bincount(counts, minlength=dc.MAX_STEPS + 1).tolist(), "equal to the restatement's on", same)
    assert counts.min() >= 1 and counts.max() <= dc.MAX_STEPS
    # 3. padding, NaN, repeatability
    assert_padding_and_no_nan(out, r)
    assert same_results(launch(P, slabs, G, r, dc.MAX_STEPS, dc.TOL, l1, l2), out)
    # 1. values, at the kernel's own counts: every valid column
    want, _ = dyn.panel_steps_dyn(P, slabs, G, r, LEN_VALID, dc.MAX_STEPS, dc.TOL, l1, l2, forced=counts)
    got = out["P"][:LEN_VALID, :r].astype(np.float64)
    err = dc.column_distances(got, want)
    print("    worst column distance", err.max(), "whole block", dc.rel(got, want), "tolerance", tol)
    assert not got[np.linalg.norm(want, axis=1) == 0].any(), "a column whose restated result is 0 is not 0"
    assert (err < tol).all(), (int(np.argmax(err)), float(err.max()), tol)
    # ps: the tolerance of the values carried through the dot product (Cauchy-Schwarz), and the rounding of a sum of r products of S-term sums
    u = mc.UNIT[dtype]
    a = slabs.astype(np.float64).sum(axis=0)[:LEN_VALID, :r]
    ps_tol = tol * np.linalg.norm(want, axis=1) * np.linalg.norm(a, axis=1) + ref.gamma(RP + S, u) * np.abs(want * a).sum(axis=1)
    assert (np.abs(out["ps"][:LEN_VALID] - (want * a).sum(axis=1)) <= ps_tol).all()
    # the sums of squares: of the panel the kernel wrote, to the rounding of its sums
    own = out["P"].astype(np.float64)
    colsq = (own * own).sum(axis=0)
    assert (np.abs(out["sumsq_part"].astype(np.float64).sum(axis=0) - colsq) <= ref.gamma(dc.LEN_PAD, u) * colsq).all()
    # 2. the rule
    assert same >= dc.FLIP_CAP, f"counts differ from the restatement's on {int((counts != counts_own).sum())} of {LEN_VALID} columns"


@pytest.mark.parametrize("l1,l2", dc.PENALTIES)
@pytest.mark.parametrize("case", CASES)
def test_workgroup_exit_and_static_bits(case, l1, l2):
    """delta = 0.999 with a maximum of 64: every valid count is at most 2 (the workgroups leave the loop; 62 more steps would also change the values), and the
    columns at 2 carry the bits of op_apg_steps at 2 steps.  delta = 1e-30 with a maximum of 4: nothing but an exact fixed point freezes, and every column whose
    count is the maximum carries the bits of op_apg_steps at that count, P and ps -- the dynamic kernel makes the step in the static kernel's order."""
    dtype, RP, r, S = case
    P, slabs, G = dc.step_case(case, l1, l2)
    loose = launch(P, slabs, G, r, dc.LOOSE_MAX, dc.LOOSE_TOL, l1, l2)
    counts = loose["counts"][:LEN_VALID]
    assert counts.min() >= 1 and counts.max() <= 2, np.bincount(counts).tolist()
    two = launch(P, slabs, G, r, 2, 0.0, l1, l2, static=True)
    at_two = counts == 2
    assert at_two.sum() >= LEN_VALID // 2 and np.array_equal(loose["P"][:LEN_VALID][at_two], two["P"][:LEN_VALID][at_two])
    assert np.array_equal(loose["ps"][:LEN_VALID][at_two], two["ps"][:LEN_VALID][at_two])
    assert_padding_and_no_nan(loose, r)
    tight = launch(P, slabs, G, r, dc.TIGHT_MAX, dc.TIGHT_TOL, l1, l2)
    static = launch(P, slabs, G, r, dc.TIGHT_MAX, 0.0, l1, l2, static=True)
    full = tight["counts"][:LEN_VALID] == dc.TIGHT_MAX
    print(dc.case_id(case), "columns at the maximum with delta = 1e-30:", int(full.sum()))
    assert full.sum() >= LEN_VALID // 2
    assert np.array_equal(tight["P"][:LEN_VALID][full], static["P"][:LEN_VALID][full]) and np.array_equal(tight["ps"][:LEN_VALID][full], static["ps"][:LEN_VALID][full])
    assert (tight["counts"][:LEN_VALID][~full] == 1).all(), "a column below the maximum that is not a fixed point"
    assert_padding_and_no_nan(tight, r)


@pytest.mark.parametrize("case", CASES)
def test_tiling_independence(case):
    """The same columns in a panel of len_pad 128 and of 256: the same bits and counts on the valid columns, zeros behind them."""
    dtype, RP, r, S = case
    l1, l2 = dc.PENALTIES[1]
    a = launch(*dc.step_case(case, l1, l2), r, dc.MAX_STEPS, dc.TOL, l1, l2)
    b = launch(*dc.step_case(case, l1, l2, len_pad=256), r, dc.MAX_STEPS, dc.TOL, l1, l2)
    assert b["P"].shape[0] == 256 and b["counts"].shape == (256,)
    assert np.array_equal(a["P"], b["P"][:128]) and np.array_equal(a["counts"], b["counts"][:128]) and np.array_equal(a["ps"][:LEN_VALID], b["ps"][:LEN_VALID])
    assert not b["P"][128:].any() and not b["counts"][128:].any()
    assert np.array_equal(a["sumsq_part"], b["sumsq_part"][:a["parts"]]) and not b["sumsq_part"][a["parts"]:].any()
    assert_padding_and_no_nan(b, r)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_zero_g_keeps_the_panel_and_counts_nothing(dtype):
    case = (dtype,) + dc.ZERO_G_CASE[1:]
    r = case[2]
    P, slabs, G = dc.step_case(case, zero_g=True)
    out = launch(P, slabs, G, r, 5, 0.1)
    assert np.array_equal(out["P"][:LEN_VALID, :r], P[:LEN_VALID, :r]) and P[:LEN_VALID, :r].any()
    assert (out["counts"] == 0).all()
    assert_padding_and_no_nan(out, r)
    pen = launch(P, slabs, G, r, 5, 0.1, 0.0, 0.25)          # (l2 alone makes L > 0: steps are taken)
    assert (pen["counts"][:LEN_VALID] >= 1).all() and not np.array_equal(pen["P"], out["P"])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_launcher_refusals(dtype):
    P, G, slab = np.zeros((128, 64), dtype), np.eye(64, dtype=dtype), np.zeros((1, 128 * 64), dtype)

    def refused(*args, **kw):
        with pytest.raises(na.EngineError) as info:
            na.op_apg_steps_dyn(*args, **kw)
        return info.value.status == 1

    for tol in (0.0, -0.1, 1.0, 1.5, float("nan"), float("inf")):
        assert refused(P, slab, G, 1, 128, 4, tol), tol
    for steps in (0, 257, -1):
        assert refused(P, slab, G, 1, 128, steps, 0.1), steps
    for RP in (32, 192, 256):      # no instantiation
        assert refused(np.zeros((128, RP), dtype), np.zeros((1, 128 * RP), dtype), np.eye(RP, dtype=dtype), 1, 128, 2, 0.1), RP
    for l1, l2 in ((-0.1, 0.0), (0.0, -0.1), (float("nan"), 0.0), (0.0, float("nan")), (float("inf"), 0.0)):
        assert refused(P, slab, G, 1, 128, 2, 0.1, l1=l1, l2=l2), (l1, l2)
    assert refused(P, slab, G, 0, 128, 4, 0.1) and refused(P, slab, G, 65, 128, 4, 0.1)                      # r outside 1 ... RP
    assert refused(P, slab, G, 1, 129, 4, 0.1)                                                             # len_valid > len_pad
    assert refused(np.zeros((64, 64), dtype), np.zeros((1, 64 * 64), dtype), G, 1, 64, 4, 0.1)              # len_pad % 128
    out = na.op_apg_steps_dyn(P, slab, G, 1, 128, 1, 0.5)             # one step runs the dynamic kernel too
    assert (out["counts"] == 1).all()
    out = na.op_apg_steps_dyn(P, slab, G, 1, 100, 256, 0.999999)
    assert (out["counts"][:100] == 1).all() and (out["counts"][100:] == 0).all()      # (all zeros with a = 0: a fixed point)
