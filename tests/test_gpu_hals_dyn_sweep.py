"""Per-column dynamic stopping of the HALS inner sweeps on the GPU, kernel level (kernels_hals_dyn.hip, docs/HALS.md "Dynamic stopping"): k_sweeps_hals_dyn
through nmfamd_op_hals_sweeps_dyn_* at every instantiated (dtype, RP), against tests/hals_dyn_reference.py on the inputs of tests/hals_dyn_cases.py
(tests/test_hals_dyn_cpu.py shows on the CPU that these inputs give diverse counts and keep an fp32 run within the cap on threshold flips).

Values and rule are checked separately.  Values: the restatement is run again with the KERNEL's counts forced per column, and every valid column must lie within
the running-error bound that tests/test_gpu_hals_multi.py holds three sweeps to, carried to each column's own count (hals_dyn_reference.dyn_bound).  Rule: the
kernel's counts equal the restatement's own for at least 98 % of the valid columns (a column on the threshold may freeze one sweep apart).
"""
import numpy as np
import pytest

import nmfgpu_amd as na
from tests import hals_dyn_cases as dc
from tests import hals_dyn_reference as dyn
from tests import hals_multi_cases as mc
from tests import hals_reference as ref

pytestmark = pytest.mark.gpu

LEN_PAD, LEN_VALID = dc.LEN_PAD, dc.LEN_VALID
CASES = [pytest.param(c, id=dc.case_id(c)) for c in dc.SWEEP_CASES]


@pytest.fixture(scope="module", autouse=True)
def _library_is_native():
    assert na.device_count() >= 1, "GPU tests need a HIP device"
    assert na.initialize() in (na.ResultType.Success, na.ResultType.ErrorAlreadyInitialized)
    na.set_verbosity(na.Verbosity.Nothing)
    yield
    na.finalize()


def launch(P, slabs, G, r, sweeps, tol, l1=0.0, l2=0.0, static=False):
    """The kernel on a case: the slabs lie 16 RP elements apart where there are several, and the gaps, the slab rows of the padding columns and the padding columns
    of the panel hold NaN, which any use of them would carry into the result; ps and sumsq_part start as NaN sentinels.  static: op_hals_sweeps instead."""
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
        out = na.op_hals_sweeps(P, flat, G, r, LEN_VALID, sweeps, l1=l1, l2=l2, **sentinels)
    else:
        out = na.op_hals_sweeps_dyn(P, flat, G, r, LEN_VALID, sweeps, tol, l1=l1, l2=l2, **sentinels)
    assert out["parts"] == len_pad // mc.cols_and_chunk(P.dtype.type, RP)[0]
    return out


def assert_padding_and_no_nan(out, r):
    P = out["P"]
    assert (P[:, r:] == 0).all(), "coordinates >= r are not 0"
    assert (P[LEN_VALID:, :] == 0).all(), "padding columns are not 0"
    assert not np.isnan(P).any() and not np.isnan(out["sumsq_part"]).any()
    assert not np.isnan(out["ps"][:LEN_VALID]).any() and np.isnan(out["ps"][LEN_VALID:]).all()      # (ps(y) is written exactly where y < len_valid)
    if "counts" in out:
        assert (out["counts"][LEN_VALID:] == 0).all(), "padding columns have a count"


@pytest.mark.parametrize("l1,l2", dc.PENALTIES)
@pytest.mark.parametrize("case", CASES)
def test_values_rule_padding_and_repeat(case, l1, l2):
    dtype, RP, r, S = case
    u = mc.UNIT[dtype]
    want_own, counts_own = dc.restated(case, l1, l2)
    assert dc.diversity_faults(case, counts_own) == []
    P, slabs, G = dc.sweep_case(case, l1, l2)
    out = launch(P, slabs, G, r, dc.MAX_SWEEPS, dc.TOL, l1, l2)
    counts = out["counts"][:LEN_VALID]
    same = float((counts == counts_own).mean())
    print(dc.case_id(case), (l1, l2), "kernel counts", np.bincount(counts, minlength=dc.MAX_SWEEPS + 1).tolist(), "equal to the restatement's on", same)
    assert counts.min() >= 1 and counts.max() <= dc.MAX_SWEEPS
    # 3. padding, NaN, repeatability
    assert_padding_and_no_nan(out, r)
    again = launch(P, slabs, G, r, dc.MAX_SWEEPS, dc.TOL, l1, l2)
    assert np.array_equal(again["P"], out["P"]) and np.array_equal(again["counts"], out["counts"]) and np.array_equal(again["sumsq_part"], out["sumsq_part"])
    assert np.array_equal(again["ps"][:LEN_VALID], out["ps"][:LEN_VALID])
    # 1. values, at the kernel's own counts: every valid column
    want, _ = dyn.panel_sweeps_dyn(P, slabs, G, r, LEN_VALID, dc.MAX_SWEEPS, dc.TOL, l1, l2, forced=counts)
    b = dyn.dyn_bound(P, slabs, G, r, LEN_VALID, counts, u, l1, l2)
    got = out["P"][:LEN_VALID, :r].astype(np.float64)
    err = np.abs(got - want)
    print("    worst error / bound", (err / np.maximum(b, 1e-300)).max(), "worst error", err.max())
    assert (err <= b).all(), f"worst error / bound {(err / np.maximum(b, 1e-300)).max():.3g} at {np.unravel_index(np.argmax(err - b), err.shape)}"
    a = slabs.astype(np.float64).sum(axis=0)[:LEN_VALID, :r]
    ps_tol = ref.gamma(RP + S, u) * np.abs(want * a).sum(axis=1) + (b * np.abs(a)).sum(axis=1)
    assert (np.abs(out["ps"][:LEN_VALID] - (want * a).sum(axis=1)) <= ps_tol).all()
    own = out["P"].astype(np.float64)
    colsq = (own * own).sum(axis=0)
    assert (np.abs(out["sumsq_part"].astype(np.float64).sum(axis=0) - colsq) <= ref.gamma(LEN_PAD, u) * colsq).all()
    # 2. the rule
    assert same >= dc.FLIP_CAP, f"counts differ from the restatement's on {int((counts != counts_own).sum())} of {LEN_VALID} columns"


@pytest.mark.parametrize("case", CASES)
def test_workgroup_exit_and_static_bits(case):
    """delta = 0.999 with a maximum of 64: every valid count is at most 2 (the workgroups leave the loop; 62 more sweeps would also change the values).  delta = 1e-30:
    nothing but an exact fixed point freezes, and every column whose count is the maximum carries the bits of op_hals_sweeps at that count."""
    dtype, RP, r, S = case
    P, slabs, G = dc.settled_case(case)
    loose = launch(P, slabs, G, r, dc.LOOSE_MAX, dc.LOOSE_TOL)
    assert loose["counts"][:LEN_VALID].min() >= 1 and loose["counts"][:LEN_VALID].max() <= 2, np.bincount(loose["counts"][:LEN_VALID]).tolist()
    two = launch(P, slabs, G, r, 2, 0.0, static=True)
    at_two = loose["counts"][:LEN_VALID] == 2
    assert at_two.any() and np.array_equal(loose["P"][:LEN_VALID][at_two], two["P"][:LEN_VALID][at_two])
    assert_padding_and_no_nan(loose, r)
    P, slabs, G = dc.sweep_case(case)
    tight = launch(P, slabs, G, r, 4, 1e-30)
    static = launch(P, slabs, G, r, 4, 0.0, static=True)
    full = tight["counts"][:LEN_VALID] == 4
    print(dc.case_id(case), "columns at the maximum with delta = 1e-30:", int(full.sum()))
    assert full.sum() >= LEN_VALID // 2
    assert np.array_equal(tight["P"][:LEN_VALID][full], static["P"][:LEN_VALID][full]) and np.array_equal(tight["ps"][:LEN_VALID][full], static["ps"][:LEN_VALID][full])
    assert_padding_and_no_nan(tight, r)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_launcher_refusals(dtype):
    P, G, slab = np.zeros((128, 64), dtype), np.eye(64, dtype=dtype), np.zeros((1, 128 * 64), dtype)

    def refused(*args, **kw):
        with pytest.raises(na.EngineError) as info:
            na.op_hals_sweeps_dyn(*args, **kw)
        return info.value.status == 1

    for tol in (0.0, -0.1, 1.0, 1.5, float("nan"), float("inf")):
        assert refused(P, slab, G, 1, 128, 4, tol), tol
    for sweeps in (0, 65, -1):
        assert refused(P, slab, G, 1, 128, sweeps, 0.1), sweeps
    assert refused(P, slab, G, 0, 128, 4, 0.1) and refused(P, slab, G, 65, 128, 4, 0.1)                      # r outside 1 ... RP
    assert refused(P, slab, G, 1, 129, 4, 0.1)                                                             # len_valid > len_pad
    assert refused(P, slab, G, 1, 128, 4, 0.1, l1=-1.0) and refused(P, slab, G, 1, 128, 4, 0.1, l2=float("nan"))
    assert refused(np.zeros((64, 64), dtype), np.zeros((1, 64 * 64), dtype), G, 1, 64, 4, 0.1)              # len_pad % 128
    if dtype is np.float32:
        assert refused(np.zeros((128, 192), dtype), np.zeros((1, 128 * 192), dtype), np.eye(192, dtype=dtype), 1, 128, 4, 0.1)      # fp32 has no RP 192
    out = na.op_hals_sweeps_dyn(P, slab, G, 1, 128, 1, 0.5)           # one sweep runs the dynamic kernel too
    assert (out["counts"] == 1).all()
    out = na.op_hals_sweeps_dyn(P, slab, G, 1, 100, 64, 0.999999)
    assert (out["counts"][:100] == 1).all() and (out["counts"][100:] == 0).all()      # (all zeros with a = 0: a fixed point)
