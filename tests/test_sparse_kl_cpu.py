"""CPU checks behind tests/test_gpu_sparse_kl_ops.py (no device): the restatements of tests/sparse_kl_reference.py against dense numpy formulas, `boundaries`
against a brute-force loop, the exactness proofs and the promised contents of the case builders (tests/sparse_kl_cases.py), every arithmetic bound against an
emulation of the operation in float32 and in float64 in two summation orders that are not the kernels', and the new symbols."""
import os
import re

import numpy as np
import pytest

import nmfgpu_amd as na
from tests import sparse_kl_cases as cases
from tests import sparse_kl_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ["float32", "float64"]
OPS = ("kl_fused", "kl_update", "kl_sums", "panel_rowsum", "spmm_rows", "sddmm_quotient")


def close(a, b):
    return np.allclose(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), rtol=1e-13, atol=0)


# ---------------------------------------------------------------------------------------------------------------- the restatements themselves

def test_restatements_match_dense_formulas():
    rng = np.random.default_rng(3)
    m, n, RP, r, eps = 9, 12, 8, 5, 1e-3
    V = rng.random((m, n)) * (rng.random((m, n)) < 0.4)
    V[2] = 0                                                              # an empty row
    stored = V != 0
    ptr = np.concatenate([[0], np.cumsum(stored.sum(axis=1))]).astype(np.int32)
    idx = np.concatenate([np.nonzero(row)[0] for row in stored]).astype(np.int32)
    val = V[stored]
    A = np.zeros((16, RP)); B = np.zeros((n, RP)); s = np.ones(RP)
    A[:m, :r] = rng.random((m, r)); B[:, :r] = rng.random((n, r)); s[:r] = 0.5 + rng.random(r)
    WH = (A[:m] * s) @ B.T
    Q = np.where(stored, V / (WH + eps), 0)
    want = ref.kl_fused(ptr, idx, val, A, B, m, 16, eps, s)
    assert close(want["out"][0, :m], Q @ B) and np.all(want["out"][0, m:] == 0)
    assert close(want["t_vwh"][0], (V * WH).sum(axis=1))
    with np.errstate(divide="ignore", invalid="ignore"):
        kl = np.where(stored, V * np.log(V / (WH + eps)), 0)
    assert close(want["t_kl"][0], kl.sum(axis=1)) and close(want["kl_abs"][0], np.abs(kl).sum(axis=1)) and close(want["kl_x"][0], V.sum(axis=1))
    assert np.array_equal(want["n"][0], stored.sum(axis=1))
    # the blocked form: per block the same formula on the block's columns, and the blocks add up to the whole
    for blocks in (2, 3, 5):
        bp = ref.boundaries(ptr, idx, n, blocks)
        part = ref.kl_fused(bp, idx, val, A, B, m, 16, eps, s, blocks)
        per = -(-n // blocks)
        for b in range(blocks):
            cols = slice(b * per, min(n, (b + 1) * per))
            assert close(part["out"][b, :m], Q[:, cols] @ B[cols])
            assert close(part["t_vwh"][b], (V * WH)[:, cols].sum(axis=1)) and close(part["t_kl"][b], kl[:, cols].sum(axis=1))
        assert close(part["out"].sum(axis=0), want["out"][0]) and close(part["t_kl"].sum(axis=0), want["t_kl"][0])
    sd = ref.sddmm_quotient(ptr, idx, val, A * s, B, m, eps)
    assert close(sd["q"], Q[stored]) and close(sd["t_vwh"], want["t_vwh"][0]) and close(sd["t_kl"], want["t_kl"][0])
    sp = ref.spmm_rows(ptr, idx, val - 0.5, B, m, 16)
    assert close(sp["out"][:m], np.where(stored, V - 0.5, 0) @ B) and close(sp["abs"][:m], np.where(stored, np.abs(V - 0.5), 0) @ B) and np.all(sp["out"][m:] == 0)
    # round_den: the denominator rounded to the launch's type
    one = ref.kl_fused(np.array([0, 1], np.int32), np.array([0], np.int32), np.array([3.0]), np.array([[4.0]]), np.array([[1.0]]), 1, 1, ref.eps_of(np.float32),
                       round_den=np.float32)
    assert one["out"][0, 0, 0] == 0.75 and ref.kl_fused(np.array([0, 1], np.int32), np.array([0], np.int32), np.array([3.0]), np.array([[4.0]]), np.array([[1.0]]),
                                                      1, 1, ref.eps_of(np.float32))["out"][0, 0, 0] < 0.75
    P = rng.random((256, RP)); nums = rng.random((3, 256, RP)); den = rng.random(RP)
    up = ref.kl_update(P, nums, den, eps, s)
    assert close(up["P"], P * s * nums.sum(axis=0) / (den + eps))
    assert close(up["sum_part"], np.stack([up["P"][:128].sum(axis=0), up["P"][128:].sum(axis=0)]).astype(np.float64))
    assert close(up["sumsq_part"][1], (np.asarray(up["P"][128:], dtype=np.float64) ** 2).sum(axis=0))
    sa = rng.random((7, RP)); sb = rng.random((7, RP)); sb[:, 3] = 0
    ks = ref.kl_sums(sa, sb)
    d = np.sqrt(sb.sum(axis=0)); d[3] = 1
    assert close(ks["sums"], sa.sum(axis=0) / d) and close(ks["scale"], 1 / d) and ks["scale"][3] == 1 and close(ref.kl_sums(sa)["sums"], sa.sum(axis=0))
    assert close(ref.panel_rowsum(P - 0.5)["sums"], (P - 0.5).sum(axis=0)) and close(ref.panel_rowsum(P - 0.5)["abs"], np.abs(P - 0.5).sum(axis=0))


def test_boundaries_against_a_brute_force_loop():
    rng = np.random.default_rng(5)
    for index_range, blocks in ((40, 2), (40, 3), (40, 8), (40, 16), (7, 16), (100, 7), (1, 2)):
        lengths = rng.integers(0, 30, 20)
        ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
        idx = np.concatenate([np.sort(rng.integers(0, index_range, L)) for L in lengths] + [np.zeros(0, np.int64)]).astype(np.int32)
        got = ref.boundaries(ptr, idx, index_range, blocks)
        per = (index_range + blocks - 1) // blocks
        for i in range(20):
            for b in range(blocks + 1):
                p = ptr[i]
                while p < ptr[i + 1] and (b == blocks or idx[p] < b * per):
                    p += 1
                assert got[i, b] == p, (index_range, blocks, i, b)
        # the blocks of a row partition its entries by index
        for i in range(20):
            for b in range(blocks):
                seg = idx[got[i, b]:got[i, b + 1]]
                assert np.all(seg // per == b)


# ---------------------------------------------------------------------------------------------------------------- the builders

def _check_contents(case):
    ptr, idx, val, rows = case["ptr"], case["idx"], case["val"], case["rows"]
    lengths = np.diff(ptr)
    assert tuple(lengths) == cases.row_lengths(rows)
    if rows >= len(cases.ROW_LENGTHS):
        assert set(cases.ROW_LENGTHS) <= set(lengths.tolist())
    for i in range(rows):
        assert np.all(np.diff(idx[ptr[i]:ptr[i + 1]]) >= 0)
    panel = case["B"] if "B" in case else case["P"]
    valid = case.get("range", cases.GATHER_VALID)
    assert 0 in idx and valid - 1 in idx and idx.max() == valid - 1                     # the first and the last valid row of the gathered panel
    assert any(np.any(np.diff(idx[ptr[i]:ptr[i + 1]]) == 0) for i in range(rows))       # a duplicated index
    assert np.any(val == 0)                                                              # a stored explicit zero
    used = np.zeros(len(panel), bool); used[idx] = True
    assert np.all(np.isfinite(panel[used])) and np.all(np.isnan(panel[~used])) and not used[valid:].any() and (~used[:valid]).any()
    assert np.all(panel[used][:, case["r"]:] == 0)
    if "A" in case:
        A = case["A"]
        assert np.all(np.isnan(A[rows:])) and np.all(A[:rows, case["r"]:] == 0)
        if rows > 1:
            z = case["zero_row"]
            assert np.all(A[z] == 0) and lengths[z] > 0 and np.all(A[:rows][np.arange(rows) != z, :case["r"]].max(axis=1) > 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_builders_prove_exactness_and_hold_the_promised_contents(dtype):
    """gather_case(kind="exact") asserts its own proof while it builds; here every case is built, its contents are checked, and the restatement's values turn out
    representable in float32 (what an exact computation in 24 bits returns)."""
    for RP, ranks in cases.RANKS.items():
        for r in ranks:
            for rows, rows_pad in cases.ROWS:
                for scaled in (False, True):
                    case = cases.gather_case(dtype, RP, r, rows, rows_pad, "exact", scaled)
                    _check_contents(case)
                    _check_contents(cases.gather_case(dtype, RP, r, rows, rows_pad, "random", scaled))
                    assert (case["a_scale"] is not None) == scaled
                _check_contents(cases.spmm_case(dtype, RP, r, rows, rows_pad, "exact")[0])
                _check_contents(cases.spmm_case(dtype, RP, r, rows, rows_pad, "random")[0])
    for RP, r in ((64, 63), (256, 255)):
        case, _, want = cases.gather_reference(dtype, RP, r, 130, 256, "exact", True)
        for k in ("out", "t_vwh"):
            assert np.array_equal(want[k].astype(np.float32).astype(ref.WORK), want[k])
        for blocks in cases.BLOCKS:
            bcase, bptr, bwant = cases.gather_reference(dtype, RP, r, 130, 256, "exact", False, blocks)
            _check_contents(bcase)
            n = bwant["n"]
            assert np.any(n.sum(axis=1) == 0) or blocks < 8              # blocks that are empty for every row ...
            assert np.any((n > 0).sum(axis=0)[n.sum(axis=0) > 0] == 1)   # ... and rows with all their entries in one block
            assert np.array_equal(bwant["out"].astype(np.float32).astype(ref.WORK), bwant["out"])
            whole = ref.kl_fused(bcase["ptr"], bcase["idx"], bcase["val"], bcase["A"], bcase["B"], 130, 256, ref.eps_of(np.dtype(dtype)), None, 1, round_den=np.dtype(dtype))
            assert np.array_equal(bwant["out"].sum(axis=0), whole["out"][0])      # exact inputs: the blocks add up to the whole without any rounding


@pytest.mark.parametrize("dtype", DTYPES)
def test_update_sums_and_rowsum_builders(dtype):
    for RP, ranks in cases.RANKS.items():
        r = ranks[0]
        for parts in cases.UPDATE_PARTS:
            for len_pad in (128, 384) if parts in cases.UPDATE_LONG_PARTS else (128,):
                for want_sumsq, with_scale in cases.update_settings(parts):
                    case, want = cases.update_case(dtype, RP, r, len_pad, parts, "exact", with_scale)
                    panel, stride = len_pad * RP, case["stride"]
                    assert stride == panel + 16 * RP and (case["scale"] is not None) == with_scale
                    gaps = np.ones(case["num"].size, bool)
                    for k in range(parts):
                        gaps[k * stride:k * stride + panel] = False
                        assert parts == 1 or np.any(case["num"][k * stride:k * stride + panel] != 0)      # every part carries something
                    assert np.all(np.isnan(case["num"][gaps])) and gaps.sum() == parts * 16 * RP and np.all(np.isfinite(case["num"][~gaps]))
                    assert np.all(case["den"][r:] == 0) and np.all(case["P"][:, r:] == 0) and np.all(want["P"][:, r:] == 0)
                    for k in ("P", "sum_part", "sumsq_part"):
                        assert np.array_equal(want[k].astype(np.float32).astype(ref.WORK), want[k])
        for parts in cases.SUMS_PARTS:
            sa, sb, zc, with_sq, without = cases.sums_case(dtype, RP, r, parts, "exact")
            assert np.all(sb[:, zc] == 0) and with_sq["scale"][zc] == 1 and with_sq["sums"][zc] == without["sums"][zc]
            for a in (with_sq["sums"], with_sq["scale"], without["sums"]):
                assert np.array_equal(a.astype(np.float32).astype(ref.WORK), a)
    # the settings cover the engine's two forms with and without the pending scale
    seen = {s for parts in cases.UPDATE_PARTS for s in cases.update_settings(parts)}
    assert seen == {(False, False), (False, True), (True, False), (True, True)}


# ---------------------------------------------------------------------------------------------------------------- the bounds, against code that is not the kernel

def ordered_sum(x, order):
    """Sum over axis 0 in the type of x: "forward" one term after the other; "pairwise": the terms reversed, then neighbours added level by level."""
    if len(x) == 0:
        return np.zeros(x.shape[1:], x.dtype)
    if order == "forward":
        acc = x[0].copy()
        for k in range(1, len(x)):
            acc = acc + x[k]
        return acc
    x = x[::-1]
    while len(x) > 1:
        even = x[0:len(x) - len(x) % 2:2] + x[1::2]
        x = np.concatenate([even, x[-1:]]) if len(x) % 2 else even
    return x[0]


def emulate_fused(case, ptr, blocks, order):
    dt = case["dtype"].type
    eps = dt(ref.eps_of(dt))
    rows, rows_pad, RP = case["rows"], case["rows_pad"], case["RP"]
    rg = ptr if blocks > 1 else np.stack([ptr[:-1], ptr[1:]], axis=1)
    out = np.zeros((blocks, rows_pad, RP), dt); tv = np.zeros((blocks, rows), dt); tk = np.zeros((blocks, rows), dt)
    q_all = np.zeros(len(case["val"]), dt)
    for row in range(rows):
        a = case["A"][row] if case["a_scale"] is None else case["A"][row] * case["a_scale"]
        for b in range(blocks):
            lo, hi = rg[row, b], rg[row, b + 1]
            x = case["val"][lo:hi]; Bj = case["B"][case["idx"][lo:hi]]
            wh = ordered_sum((Bj * a).T, order)
            den = wh + eps
            q = x / den
            q_all[lo:hi] = q
            out[b, row] = ordered_sum(q[:, None] * Bj, order)
            tv[b, row] = ordered_sum(x * wh, order)
            pos = x > 0
            tk[b, row] = ordered_sum(x[pos] * np.log(x[pos] / den[pos]), order)
    assert out.dtype == dt and tk.dtype == dt
    return out, tv, tk, q_all


@pytest.mark.parametrize("order", ["forward", "pairwise"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_bounds_hold_for_an_emulation_in_another_order(dtype, order):
    u = ref.unit_roundoff(dtype)
    for RP, r, blocks in ((64, 63, 1), (64, 1, 3), (128, 65, 8), (256, 255, 1)):
        case, bptr, want = cases.gather_reference(dtype, RP, r, 130, 256, "random", blocks == 1, blocks)
        rows = case["rows"]
        out, tv, tk, q = emulate_fused(case, bptr if blocks > 1 else case["ptr"], blocks, order)
        ratios = (cases.worst_ratio(out, want["out"], ref.fused_out_bound(RP, np.pad(want["n"], ((0, 0), (0, 256 - rows))), want["out"], u)),
                  cases.worst_ratio(tv, want["t_vwh"], ref.vwh_bound(RP, want["n"], want["t_vwh"], u)),
                  cases.worst_ratio(tk, want["t_kl"], ref.kl_term_bound(RP, want["n"], want["kl_x"], want["kl_abs"], u)))
        assert max(ratios) <= 1, (RP, r, blocks, ratios)
        assert min(ratios) > 0      # (an emulation in the launch's type does round: a bound of this size is not vacuous)
    case, sd = cases.sddmm_reference(dtype, 128, 65, 130, 256, "random")
    _, tv, tk, q = emulate_fused(case, case["ptr"], 1, order)
    assert cases.worst_ratio(q, sd["q"], ref.quotient_bound(128, sd["q"], u)) <= 1
    assert cases.worst_ratio(tv[0], sd["t_vwh"], ref.vwh_bound(128, sd["n"], sd["t_vwh"], u)) <= 1
    assert cases.worst_ratio(tk[0], sd["t_kl"], ref.kl_term_bound(128, sd["n"], sd["kl_x"], sd["kl_abs"], u)) <= 1
    for RP, r in ((64, 63), (256, 129)):
        sc, sw = cases.spmm_case(dtype, RP, r, 130, 256, "random")
        got = np.zeros((256, RP), sc["dtype"])
        for row in range(130):
            lo, hi = sc["ptr"][row], sc["ptr"][row + 1]
            got[row] = ordered_sum(sc["val"][lo:hi, None] * sc["P"][sc["idx"][lo:hi]], order)
        ratio = cases.worst_ratio(got, sw["out"], ref.spmm_bound(np.pad(sw["n"], (0, 126)), sw["abs"], u))
        assert 0 < ratio <= 1, ratio


@pytest.mark.parametrize("order", ["forward", "pairwise"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_update_sums_and_rowsum_bounds_hold_for_an_emulation_in_another_order(dtype, order):
    u = ref.unit_roundoff(dtype)
    dt = np.dtype(dtype).type
    for RP, r, parts, with_scale in ((64, 63, 1, False), (64, 1, 7, True), (128, 65, 17, True), (256, 255, 64, False)):
        case, want = cases.update_case(dtype, RP, r, 128, parts, "random", with_scale)
        panel, stride = 128 * RP, case["stride"]
        nums = np.stack([case["num"][k * stride:k * stride + panel].reshape(128, RP) for k in range(parts)])
        old = case["P"] if case["scale"] is None else case["P"] * case["scale"]
        new = old * ordered_sum(nums, order) / (case["den"] + dt(ref.eps_of(dt)))
        assert new.dtype == dt
        assert 0 < cases.worst_ratio(new, want["P"], ref.update_bound(parts, want["P"], u)) <= 1
        s, sbound, sq, sqbound = ref.update_sum_bounds(new, u)
        assert cases.worst_ratio(ordered_sum(new, order)[None], s, sbound) <= 1 and cases.worst_ratio(ordered_sum(new * new, order)[None], sq, sqbound) <= 1
    for parts in (2, 65, 513, 1600):
        sa, sb, zc, with_sq, without = cases.sums_case(dtype, 64, 63, parts, "random")
        a, b = ordered_sum(sa, order), ordered_sum(sb, order)
        root = np.sqrt(np.where(b > 0, b, dt(1)))
        assert cases.worst_ratio(a, without["sums"], ref.sums_bound(parts, without["sums"], u)) <= 1
        assert cases.worst_ratio(a / root, with_sq["sums"], ref.sums_bound(parts, with_sq["sums"], u)) <= 1
        assert cases.worst_ratio(dt(1) / root, with_sq["scale"], ref.sums_bound(parts, with_sq["scale"], u)) <= 1
    for len_pad in cases.ROWSUM_LEN_PADS:
        P, want = cases.rowsum_case(dtype, 128, 65, len_pad, "random")
        assert 0 < cases.worst_ratio(ordered_sum(P, order), want["sums"], ref.rowsum_bound(len_pad, want["abs"], u)) <= 1


# ---------------------------------------------------------------------------------------------------------------- the entries

def test_sparse_test_entries_are_declared_exported_and_wrapped():
    header = open(os.path.join(ROOT, "include", "nmfgpu_amd.h")).read()
    declared = set(re.findall(r"\b(nmfamd_[a-z_0-9]+)\s*\(", header))
    lib = na.library()
    for op in OPS:
        for suffix in ("f32", "f64"):
            name = f"nmfamd_op_{op}_{suffix}"
            assert name in declared and hasattr(lib, name), name
        assert callable(getattr(na, f"op_{op}"))


def test_wrappers_refuse_misshapen_arrays_before_the_library_sees_them():
    case = cases.gather_case("float32", 64, 63, 5, 128, "random")
    with pytest.raises(ValueError):
        na.op_kl_fused(case["ptr"][:-1], case["idx"], case["val"], case["A"], case["B"], 5, 128)
    with pytest.raises(ValueError):
        na.op_kl_fused(case["ptr"], case["idx"], case["val"], case["A"][:64], case["B"], 5, 128)
    with pytest.raises(ValueError):
        na.op_spmm_rows(case["ptr"], case["idx"][:-1], case["val"], case["B"], 5, 128)
    with pytest.raises(ValueError):
        na.op_kl_update(np.zeros((128, 64), np.float32), np.zeros((2, 128, 32), np.float32), np.zeros(64, np.float32))
    with pytest.raises(TypeError):
        na.op_panel_rowsum(np.zeros((128, 64), np.int32))
    # the library itself refuses an index outside the gathered panel and a range outside the image before it looks for a device
    bad = case["idx"].copy(); bad[3] = len(case["B"])
    with pytest.raises(na.EngineError) as e:
        na.op_kl_fused(case["ptr"], bad, case["val"], case["A"], case["B"], 5, 128)
    assert e.value.status == 1
    badp = case["ptr"].copy(); badp[-1] += 1
    with pytest.raises(na.EngineError) as e:
        na.op_spmm_rows(badp, case["idx"], case["val"], case["B"], 5, 128)
    assert e.value.status == 1
