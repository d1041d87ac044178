"""Predict and score without a device (docs/PREDICT.md): the fp64 restatement (tests/predict_reference.py) against a dense W @ H and the definitions of d_beta
written out here, the host helper split_entries, the new symbols of the built library, and the op entry's answer on a machine without a GPU."""
import os
import re

import numpy as np
import pytest

import nmfgpu_amd as na
from tests import predict_reference as pref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETAS = [-1.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0]
ENTRIES = ("nmfamd_engine_predict", "nmfamd_engine_score", "nmfamd_engine_predict_device", "nmfamd_engine_score_device", "nmfamd_predict_entry_parts",
           "nmfamd_op_predict_entries_f32", "nmfamd_op_predict_entries_f64")


def d_beta(v, p, beta):
    """The beta-divergence of one pair, from its definition (Fevotte & Idier 2011, eq. 2), v^beta = 0 at v = 0."""
    if beta == 1:
        return (v * np.log(v / p) if v > 0 else 0.0) - v + p
    if beta == 0:
        return v / p - np.log(v / p) - 1.0
    vb = v ** beta if v > 0 else 0.0
    return (vb + (beta - 1.0) * p ** beta - beta * v * p ** (beta - 1.0)) / (beta * (beta - 1.0))


def problem(seed=3, m=37, n=29, r=6, nnz=500):
    rng = np.random.default_rng(seed)
    W, H = rng.random((m, r)), rng.random((r, n))
    rows, cols = rng.integers(0, m, nnz), rng.integers(0, n, nnz)      # unsorted, with duplicates
    rows[:2], cols[:2] = (0, m - 1), (0, n - 1)
    vals = rng.integers(0, 6, nnz).astype(np.float64)
    return W, H, rows, cols, vals


@pytest.mark.parametrize("base", [0, 1])
def test_predict_is_the_gathered_dense_product(base):
    W, H, rows, cols, _ = problem()
    out, mag = pref.predict(rows + base, cols + base, W, H, base)
    dense = W @ H
    assert np.allclose(out, dense[rows, cols], rtol=1e-13, atol=0)
    assert np.allclose(mag, (np.abs(W) @ np.abs(H))[rows, cols], rtol=1e-13, atol=0)
    assert len(np.unique(rows * H.shape[1] + cols)) < len(rows), "the list has duplicates"


@pytest.mark.parametrize("beta", BETAS)
def test_score_is_the_sum_of_the_definitions(beta):
    W, H, rows, cols, vals = problem()
    if beta <= 0:
        vals = vals + 1.0      # (the value rule of beta <= 0)
    assert pref.value_rule_holds(vals, beta)
    eps = 2.0 ** -52
    got = pref.score(rows, cols, vals, W, H, beta, eps)
    p = (W @ H)[rows, cols]
    want_div = sum(d_beta(v, q + eps, beta) for v, q in zip(vals, p))
    assert got["count"] == len(vals)
    assert got["sq"] == pytest.approx(float(((vals - p) ** 2).sum()), rel=1e-12)
    assert got["rmsd"] == pytest.approx(float(np.sqrt(((vals - p) ** 2).mean())), rel=1e-12)
    assert got["abs_div"] >= abs(got["div"]) and got["abs_div"] > 0
    assert abs(got["div"] - want_div) <= 1e-12 * got["abs_div"]
    if beta == 2.0:
        assert got["div"] == pytest.approx(0.5 * float(((vals - (p + eps)) ** 2).sum()), rel=1e-10)


def test_score_without_a_beta_and_the_value_rule():
    W, H, rows, cols, vals = problem()
    got = pref.score(rows, cols, vals - 3.0, W, H, None, 2.0 ** -52)      # any finite value
    assert np.isnan(got["div"]) and np.isnan(got["abs_div"]) and np.isfinite(got["sq"])
    assert pref.value_rule_holds(vals - 3.0, None) and not pref.value_rule_holds(vals - 3.0, 1.0)
    assert pref.value_rule_holds(vals, 0.5) and not pref.value_rule_holds(vals, 0.0) and pref.value_rule_holds(vals + 1, -1.0)
    assert not pref.value_rule_holds(np.array([1.0, np.inf]), None) and not pref.value_rule_holds(np.array([1.0, np.nan]), 2.0)


def test_split_entries():
    _, _, rows, cols, vals = problem(nnz=1000)
    (tr, tc, tv), (hr, hc, hv) = na.split_entries(rows, cols, vals, 0.25, seed=11)
    assert len(hr) == 250 and len(tr) == 750
    again = na.split_entries(rows, cols, vals, 0.25, seed=11)
    for a, b in zip((tr, tc, tv, hr, hc, hv), again[0] + again[1]):
        assert np.array_equal(a, b)
    other = na.split_entries(rows, cols, vals, 0.25, seed=12)
    assert not np.array_equal(other[1][0], hr) or not np.array_equal(other[1][1], hc)
    # disjoint as positions of the list, and their union is the list: tag every position through the values
    tags = np.arange(1000, dtype=np.float64)
    (_, _, ta), (_, _, tb) = na.split_entries(rows, cols, tags, 0.25, seed=11)
    assert len(np.intersect1d(ta, tb)) == 0 and np.array_equal(np.sort(np.concatenate([ta, tb])), tags)
    assert np.all(np.diff(ta) > 0) and np.all(np.diff(tb) > 0), "both parts keep the order of the input"
    assert np.array_equal(rows[tb.astype(int)], hr) and np.array_equal(vals[ta.astype(int)], tv)
    assert len(na.split_entries(rows, cols, vals, 0.0, 1)[1][0]) == 0 and len(na.split_entries(rows, cols, vals, 1.0, 1)[0][0]) == 0
    with pytest.raises(ValueError):
        na.split_entries(rows, cols, vals[:-1], 0.25, 1)
    with pytest.raises(ValueError):
        na.split_entries(rows, cols, vals, 1.5, 1)


def test_entries_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "nmfgpu_amd.h")).read()
    lib = na.library()
    for name in ENTRIES:
        assert re.search(r"NMFAMD_API\s+int\s+" + name + r"\s*\(", header), f"{name} is not declared"
        assert hasattr(lib, name), f"{name} is not exported"
    for name in ("predict", "score"):
        assert callable(getattr(na.Engine, name))
    doc = open(os.path.join(ROOT, "docs", "PREDICT.md")).read()
    for name in ENTRIES:
        assert name in doc or name.rsplit("_f", 1)[0] in doc, f"docs/PREDICT.md does not name {name}"


def test_parts_are_a_function_of_nnz():
    assert [na.predict_entry_parts(k) for k in (1, 32, 33, 64, 65, 2048 * 32, 2048 * 32 + 1, 10 ** 9)] == [1, 1, 2, 2, 3, 2048, 2048, 2048]


def test_op_answers_without_a_device():
    rng = np.random.default_rng(5)
    Wt = np.zeros((128, 64), np.float32); H = np.zeros((128, 64), np.float32)
    Wt[:, :7] = rng.random((128, 7)); H[:, :7] = rng.random((128, 7))
    rows, cols = rng.integers(0, 128, 40), rng.integers(0, 128, 40)
    vals = rng.integers(1, 6, 40).astype(np.float32)
    # what the entry refuses it refuses anywhere: before it looks for a device
    for kw in (dict(r=0), dict(r=65), dict(base=2)):
        with pytest.raises(na.EngineError) as err:
            na.op_predict_entries(rows, cols, Wt, H, **{"r": 7, **kw})
        assert err.value.status == 1
    with pytest.raises(na.EngineError) as err:
        na.op_predict_entries(rows + 100, cols, Wt, H, 7)      # a coordinate outside the panel
    assert err.value.status == 1
    with pytest.raises(na.EngineError) as err:
        na.op_predict_entries(rows, cols, np.zeros((128, 192), np.float32), np.zeros((128, 192), np.float32), 7)      # fp32 has no padded rank 192
    assert err.value.status == 1
    if na.device_count() == 0:
        with pytest.raises(na.EngineError) as err:
            na.op_predict_entries(rows, cols, Wt, H, 7, vals=vals, beta=1.0)
        assert err.value.status == 5      # NMFAMD_NO_DEVICE
    else:
        res = na.op_predict_entries(rows, cols, Wt, H, 7, vals=vals, beta=1.0)
        want, _ = pref.predict(rows, cols, Wt[:, :7], H[:, :7].T)
        assert np.allclose(res["out"], want, rtol=1e-5)
