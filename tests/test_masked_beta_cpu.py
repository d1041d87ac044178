"""Missing-value NMF under the beta-divergence without a GPU (docs/MISSING.md, "Beta-divergence"): the entry-list restatement the GPU tests compare with
(tests/masked_beta_reference.py) against the weighted restatement at 0 / 1 weights, its objective's monotonicity with an empty row and an empty column, the
refusals of the planning step with their messages, and the nmfamd_params_v7 layout (a v6-sized struct plans as before)."""
import ctypes as C

import numpy as np
import pytest

from nmfgpu_amd import engine as eng
from tests import masked_beta_reference as mbref
from tests import masked_reference as mref
from tests import weighted_reference as wref

PEN = (0.05, 0.05, 0.01, 0.01)      # (l1W, l1H, l2W, l2H): PEN of tests/test_gpu_beta_general.py
EPS64 = float(np.finfo(np.float64).eps)
BETAS = [-1.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0]
PENS = [wref.NO_PENALTIES, PEN]
MI355X = dict(num_cus=256, memory_side_cache_bytes=256 << 20, free_bytes=200 << 30)


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def observed(m, n, share, seed, empty_row=None, empty_col=None):
    """A random Omega of about `share` of the entries with positive integer values, optionally without any entry in one row and in one column."""
    rng = np.random.default_rng(seed)
    mask = rng.random((m, n)) < share
    if empty_row is not None:
        mask[empty_row, :] = False
    if empty_col is not None:
        mask[:, empty_col] = False
    rows, cols = np.nonzero(mask)
    return rows, cols, rng.integers(1, 6, len(rows)).astype(np.float64), mask


@pytest.mark.parametrize("pen", PENS, ids=["plain", "penalised"])
@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("const_w", [False, True])
def test_restatement_is_the_weighted_update_at_01_weights(beta, pen, const_w):
    m, n, r, iters = 131, 97, 9, 20
    rows, cols, vals, mask = observed(m, n, 0.3, seed=7, empty_row=17, empty_col=40)
    V = np.full((m, n), np.nan); V[rows, cols] = vals      # (what lies under a zero weight is never looked at)
    W0, H0 = wref.start(m, n, r, seed=8)
    got = mbref.run(rows, cols, vals, W0, H0, iters, beta, EPS64, pen=pen, const_w=const_w)
    want = wref.run(V, mask.astype(np.float64), W0, H0, iters, beta, EPS64, pen=pen, const_w=const_w)
    assert rel(got[0], want[0]) < 1e-12 and rel(got[1], want[1]) < 1e-12
    for k in (2, 3, 4):
        assert got[k] == pytest.approx(want[k], rel=1e-12)
    assert got[5] >= abs(got[4])


@pytest.mark.parametrize("pen", PENS, ids=["plain", "penalised"])
@pytest.mark.parametrize("beta", BETAS)
def test_objective_is_non_increasing(beta, pen):
    m, n, r = 131, 97, 9
    rows, cols, vals, _ = observed(m, n, 0.3, seed=r + 20, empty_row=17, empty_col=40)
    W0, H0 = wref.start(m, n, r, seed=r + 21)
    out = mbref.run(rows, cols, vals, W0, H0, 40, beta, EPS64, pen=pen, history=True)
    hist = out[6]
    assert len(hist) == 40 and np.all(np.isfinite(hist)) and hist[-1] < hist[0]
    for a, b in zip(hist, hist[1:]):
        assert b <= a * (1 + 1e-12), (a, b)
    W, H = out[0], out[1]
    assert np.all(np.isfinite(W)) and np.all(np.isfinite(H))
    assert np.all(W[17] == 0) and np.all(H[:, 40] == 0)      # (nothing observed there)
    assert out[3] == pytest.approx(out[2] / np.sqrt(len(vals)), rel=1e-15)


def test_duplicates_count_once_per_copy():
    m, n, r = 40, 30, 4
    rows, cols, vals, _ = observed(m, n, 0.4, seed=31)
    W0, H0 = wref.start(m, n, r, seed=32)
    twice = mbref.run(np.tile(rows, 2), np.tile(cols, 2), np.tile(vals, 2), W0, H0, 1, 0.5, EPS64, pen=PEN)
    once = mbref.run(rows, cols, vals, W0, H0, 1, 0.5, EPS64, pen=PEN)
    # (both sums double, the penalties do not: the step differs, and the error terms of the unchanged W with the new H are sums over twice the entries)
    assert rel(twice[1], once[1]) > 1e-6
    plain2 = mbref.run(np.tile(rows, 2), np.tile(cols, 2), np.tile(vals, 2), W0, H0, 1, 0.5, 0.0, const_w=True)
    plain1 = mbref.run(rows, cols, vals, W0, H0, 1, 0.5, 0.0, const_w=True)
    assert rel(plain2[1], plain1[1]) < 1e-14 and plain2[4] == pytest.approx(2 * plain1[4], rel=1e-13)


REFUSALS = [
    (dict(missing_divergence="kl"), "missing-value divergence: 'missingDivergence' needs 'missingValues' = 1"),
    (dict(missing_values=True, missing_divergence="kl", divergence="kl"), "missing-value divergence: does not combine with 'divergence' (that one selects the unmasked updates)"),
    (dict(missing_values=True, missing_divergence="is", algorithm="nsnmf"), "missing-value divergence: the Multiplicative algorithm only"),
    (dict(missing_values=True, missing_divergence="is", algorithm="hals"), "missing-value divergence: the Multiplicative algorithm only"),
    (dict(missing_values=True, missing_divergence="kl", r=257), "missing-value divergence: rank <= 256"),
    (dict(missing_values=True, missing_divergence="kl", row_blocks=2), "missing-value divergence: single GPU only (no row blocks)"),
    (dict(missing_values=True, missing_divergence="beta", missing_beta=float("inf")), "missing-value divergence: 'missingBeta' has to be finite"),
    (dict(missing_values=True, missing_divergence="beta", missing_beta=float("nan")), "missing-value divergence: 'missingBeta' has to be finite"),
    (dict(missing_values=True, missing_divergence="beta", missing_beta=1e300), "missing-value divergence: 'missingBeta' out of the range of the engine's precision"),
    (dict(missing_values=True, missing_divergence="kl", weighted=True),
     "missing-value divergence: does not combine with 'weighted', 'mixedPrecision' or 'batchSize' (those are the dense engines')"),
    (dict(missing_values=True, missing_divergence="kl", mixed_precision=True),
     "missing-value divergence: does not combine with 'weighted', 'mixedPrecision' or 'batchSize' (those are the dense engines')"),
    (dict(missing_values=True, missing_divergence="kl", batch_size=128),
     "missing-value divergence: does not combine with 'weighted', 'mixedPrecision' or 'batchSize' (those are the dense engines')"),
    # the two refusals the existing tests pin stay, word for word
    (dict(missing_values=True, divergence="kl"), "missing values: multiplicative update with the Frobenius objective, rank <= 256"),
    (dict(missing_values=True, divergence="is"),
     "dense divergence update: does not combine with 'sparseCompute' or 'missingValues' (V is kept dense; a divergence with beta <= 0 is undefined at 0)"),
]


@pytest.mark.parametrize("change,message", REFUSALS, ids=[" ".join(f"{k}={getattr(v, '__name__', v)}" for k, v in c.items()) for c, _ in REFUSALS])
def test_refusals_carry_their_messages(change, message):
    args = dict(dict(m=300, n=200, r=8), **change)
    with pytest.raises(eng.EngineError) as err:
        eng.plan_geometry(args.pop("m"), args.pop("n"), args.pop("r"), **args, **MI355X)
    assert err.value.status == 1
    assert str(err.value) == f"nmfamd_plan_geometry: invalid argument ({message})"


def _plan(p, size, elem_bytes=4, r=8):
    g = eng._Geometry()
    lib = eng.library()
    lib.nmfamd_engine_last_error.restype = C.c_char_p
    st = lib.nmfamd_plan_geometry(300, 200, r, 0, C.byref(p), C.c_ulong(size), elem_bytes, 1, 256, C.c_ulonglong(0), C.c_ulonglong(0), C.byref(g), C.c_ulong(C.sizeof(g)))
    return st, (lib.nmfamd_engine_last_error(None) or b"").decode(), {k: getattr(g, k) for k, _ in eng._Geometry._fields_}


def test_refusals_reached_through_the_struct_only():
    """(the keyword arguments cannot say a value outside {0, 1, 2, 3} or a missing_beta without missing_divergence = 3)"""
    base = [0.0] * 16
    base[7] = base[9] = 1.0      # sparse_compute, missing_values
    for value in (4.0, -1.0, 0.5, float("nan")):
        st, why, _ = _plan(eng._params_struct(base + [value, 0.0]), C.sizeof(eng._ParamsV7))
        assert st == 1 and why == "missing-value divergence: 'missingDivergence' has to be 0 (Frobenius), 1 (KL), 2 (Itakura-Saito) or 3 (beta)"
    for div in (0.0, 1.0, 2.0):
        st, why, _ = _plan(eng._params_struct(base + [div, 0.5]), C.sizeof(eng._ParamsV7))
        assert st == 1 and why == "missing-value divergence: 'missingBeta' needs 'missingDivergence' = 3 (the general beta-divergence)"
    # missing_values = 2 is no switch for it
    two = list(base); two[9] = 2.0
    st, why, _ = _plan(eng._params_struct(two + [1.0, 0.0]), C.sizeof(eng._ParamsV7))
    assert st == 1 and why == "missing-value divergence: 'missingDivergence' needs 'missingValues' = 1"
    # 1e300 is a beta of a double engine
    assert _plan(eng._params_struct(base + [3.0, 1e300]), C.sizeof(eng._ParamsV7), elem_bytes=8)[0] == 0


def test_params_v7_layout_and_a_v6_sized_struct_plans_as_before():
    assert C.sizeof(eng._ParamsV6) == 16 * 8 and C.sizeof(eng._ParamsV7) == 18 * 8
    assert eng._ParamsV7.missing_divergence.offset == 16 * 8 and eng._ParamsV7.missing_beta.offset == 17 * 8
    # a list of sixteen values still makes a struct, with the new fields at 0
    p16 = eng._params_struct([0.0] * 16)
    assert p16.missing_divergence == 0.0 and p16.missing_beta == 0.0
    values = eng._param_values(missing_values=True, missing_divergence="beta", missing_beta=0.5)
    assert len(values) == 18 and values[16:] == [3.0, 0.5] and values[7] == 1.0 and values[9] == 1.0
    p = eng._params_struct(values)
    plain = eng._params_struct(eng._param_values(missing_values=True))
    full = _plan(p, C.sizeof(p))
    # the library reads as much as the caller's size covers: cut to v6 the same bytes plan the Frobenius masked engine
    cut = _plan(p, C.sizeof(eng._ParamsV6))
    ref = _plan(plain, C.sizeof(plain))
    assert full[0] == 0 and cut[0] == 0 and ref[0] == 0
    assert cut[2] == ref[2]
    assert full[2]["product_kernel"] == 5 and full[2]["resident_images"] == 0 and full[2]["exchange_count"] == 0 and full[2]["padded_rank"] == 64
    for r, rp in ((64, 64), (65, 128), (129, 256), (256, 256)):
        for dtype in (np.float32, np.float64):      # (the gather kernels keep the 128-column padding in either precision)
            g = eng.plan_geometry(300, 200, r, dtype=dtype, missing_values=True, missing_divergence="kl", **MI355X)
            assert g["padded_rank"] == rp
    with pytest.raises(ValueError):
        eng._param_values(missing_values=True, missing_beta=0.5)
    with pytest.raises(ValueError):
        eng._param_values(missing_values=True, missing_divergence="beta")
