"""Engine.predict and Engine.score on the GPU (docs/PREDICT.md), one engine of every family after three iterations at the suite's small shapes (300 x 257 and
500 x 300): the predictions against W @ H of get_factors, host arrays against device arrays bit for bit, the side effects against get_factors' (the trajectory
and the error of the last error iteration), score against a masked engine's own error and against the host evaluation of a held-out set, and the refusals.

Bounds, none of them measured (u = 2^-24 or 2^-53; gamma_k(u) = k u / (1 - k u)):
  predictions            |out[p] - (W @ H)[i_p, j_p]| <= gamma_r(u) sum_k |w_k h_k|: the standard bound of an r-term dot product, any order.
  score against an engine's own error (constant W, so that W_(k-1) = W_k): the engine adds the same per-entry terms in T in another order -- gamma_nnz(u) times the
                         sum of the absolute terms -- and each term carries the per-term bound of tests/test_gpu_masked_beta_kernel.py, ten times TOL of the absolute
                         summands; the engine squares v - (p + eps) where score squares v - p: 2 eps sum |v - p| + nnz eps^2 more on the squared error.
  held-out divergence against the host evaluation on get_factors' W, H: the per-term bound, plus gamma_(r+1)(u) of the absolute summands for the prediction the
                         term is formed from and the addition of eps (for the KL form |d d_beta / d p| |p| = |p - v| <= the absolute summands)."""
import ctypes as C

import numpy as np
import pytest

import nmfgpu_amd as na
from tests import masked_beta_reference as mbref
from tests import predict_reference as pref

pytestmark = pytest.mark.gpu

TOL = {np.float32: 1e-5, np.float64: 1e-12}
U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
A, B = (300, 257), (500, 300)
# name: (shape, r, dtype, algorithm, keywords, how V goes in)
FAMILIES = {
    "mu_r7_pending_scale": (A, 7, np.float32, "mu", {}, "dense"),
    "mu_r70": (A, 70, np.float32, "mu", {}, "dense"),
    "mu_r200": (B, 200, np.float32, "mu", {}, "dense"),
    "mu_f64_r70": (A, 70, np.float64, "mu", {}, "dense"),
    "nsnmf": (A, 5, np.float32, "nsnmf", dict(theta=0.3), "dense"),
    "hals": (B, 5, np.float32, "hals", {}, "dense"),
    "nenmf": (A, 5, np.float32, "nenmf", {}, "dense"),
    "dense_kl": (A, 9, np.float32, "mu", dict(divergence="kl", dense_compute=True), "dense"),
    "sparse_kl": (A, 9, np.float32, "mu", dict(divergence="kl", sparse_compute=True), "stored"),
    "masked_frobenius": (B, 9, np.float32, "mu", dict(missing_values=True), "observed"),
    "masked_beta_05": (A, 9, np.float32, "mu", dict(missing_values=True, missing_divergence="beta", missing_beta=0.5), "observed"),
    "weighted": (A, 9, np.float32, "mu", dict(weighted=True, divergence="beta", beta=0.5), "weighted"),
}
_cache = {}


def F(a):
    return np.asfortranarray(a)


def torch_():
    import torch
    assert torch.cuda.is_available()
    return torch


def eps_of(dtype):
    return float(np.finfo(dtype).eps)


def problem(name):
    """V in [0.1, 1.1) with 30 % of the entries stored / observed / weighted where the family wants that, W0, H0 in (0, 1], 2 000 coordinates (unsorted, duplicates,
    both corners) with values; built once per family and never written."""
    if name not in _cache:
        (m, n), r, dtype, _, _, how = FAMILIES[name]
        rng = np.random.default_rng(len(name) + r)
        V = (rng.random((m, n)) + 0.1).astype(dtype)
        mask = rng.random((m, n)) < 0.3
        weights = None
        if how == "stored":
            V = np.where(mask, V, 0).astype(dtype)
        elif how == "observed":
            V = np.where(mask, V, np.nan).astype(dtype)
        elif how == "weighted":
            weights = F(np.where(mask, rng.random((m, n)) + 0.5, 0).astype(dtype))
        W0, H0 = F((1.0 - rng.random((m, r))).astype(dtype)), F((1.0 - rng.random((r, n))).astype(dtype))
        rows, cols = rng.integers(0, m, 2000).astype(np.int32), rng.integers(0, n, 2000).astype(np.int32)
        rows[0], cols[0], rows[-1], cols[-1] = 0, 0, m - 1, n - 1
        rows[5], cols[5] = rows[4], cols[4]
        vals = (rng.random(2000) + 0.1).astype(dtype)
        _cache[name] = dict(V=F(V), weights=weights, W0=W0, H0=H0, rows=rows, cols=cols, vals=vals, mask=mask)
        for a in _cache[name].values():
            if a is not None:
                a.setflags(write=False)
    return _cache[name]


def engine(name, iterations=3):
    (m, n), r, dtype, alg, kw, _ = FAMILIES[name]
    p = problem(name)
    eng = na.Engine(m, n, r, alg, dtype=dtype, **kw)
    if p["weights"] is not None:
        eng.upload(p["V"], weights=p["weights"])
    else:
        eng.upload(p["V"])
    eng.set_factors(p["W0"], p["H0"])
    if iterations:
        eng.iterate(iterations, error_every=1)
    return eng


def errors_of(eng, name):
    kw = FAMILIES[name][4]
    return bits(np.array((eng.frobenius, eng.rmsd) + ((eng.divergence_value,) if ("divergence" in kw or "missing_divergence" in kw) else ())))


def bits(a):
    return np.asarray(a).tobytes()


def on_device(a):
    t = torch_().from_numpy(np.ascontiguousarray(a)).cuda()
    torch_().cuda.synchronize()
    return t


# 1. every family: the bound, the two forms, both bases, the effects on the engine
@pytest.mark.parametrize("name", list(FAMILIES))
def test_predict_and_score_of_every_family(name):
    (m, n), r, dtype, _, _, _ = FAMILIES[name]
    p = problem(name)
    rows, cols, vals = p["rows"], p["cols"], p["vals"]
    eng, twin = engine(name), engine(name)
    before = errors_of(eng, name)
    out = eng.predict(rows, cols)
    assert out.dtype == dtype and out.shape == (2000,)
    assert errors_of(eng, name) == before, "the error of the last error iteration moved"
    # against W @ H of get_factors -- the twin's, which ran the same three iterations: this engine goes on with nothing but predict behind it
    W, H = twin.get_factors()
    exact, mag = pref.predict(rows, cols, W, H)
    err, bound = np.abs(out.astype(np.float64) - exact), pref.gamma(r, U[dtype]) * mag
    print(f"{name}: predictions {float(np.max(err / np.maximum(bound, 1e-300))):.2f} of the bound")
    assert np.all(np.isfinite(out)) and np.all(err <= bound)
    # the effects are get_factors': the twin took get_factors where this engine took predict, and both go on
    eng.iterate(2, first_iteration=4, error_every=1)
    twin.iterate(2, first_iteration=4, error_every=1)
    (W2, H2), (Wt2, Ht2) = eng.get_factors(), twin.get_factors()
    assert bits(W2) == bits(Wt2) and bits(H2) == bits(Ht2), "predict disturbed the trajectory where get_factors does not"
    assert errors_of(eng, name) == errors_of(twin, name)
    # index base 1, a repeated call, and the device form: the same bits
    out = eng.predict(rows, cols)
    assert bits(eng.predict(rows + 1, cols + 1, base=1)) == bits(out) and bits(eng.predict(rows, cols)) == bits(out)
    torch = torch_()
    d_rows, d_cols, d_vals = on_device(rows), on_device(cols), on_device(vals)
    d_out = eng.predict(d_rows, d_cols)
    assert isinstance(d_out, torch.Tensor) and d_out.is_cuda and bits(d_out.cpu().numpy()) == bits(out)
    for beta in (None, 1.0, 0.0, 0.5, 2.0):
        host = eng.score(rows, cols, vals, beta=beta, return_predictions=True)
        dev = eng.score(d_rows, d_cols, d_vals, beta=beta, return_predictions=True)
        blind = eng.score(rows, cols, vals, beta=beta)
        assert bits(host["predictions"]) == bits(out) and bits(dev["predictions"].cpu().numpy()) == bits(out)
        for key in ("sq", "rmsd", "div", "abs_div", "count"):
            assert bits(np.float64(host[key])) == bits(np.float64(dev[key])) == bits(np.float64(blind[key])), (beta, key)
        want = pref.score_of_predictions(vals, out.astype(np.float64), beta, eps_of(dtype))
        assert host["count"] == 2000 and host["rmsd"] == np.sqrt(host["sq"] / 2000)
        assert abs(host["sq"] - want["sq"]) <= (pref.gamma(3, U[dtype]) + pref.gamma(2000, 2.0 ** -53)) * want["sq"]
        if beta is None:
            assert np.isnan(host["div"]) and np.isnan(host["abs_div"])
        else:
            assert abs(host["div"] - want["div"]) <= 10 * TOL[dtype] * want["abs_div"] and abs(host["abs_div"] - want["abs_div"]) <= 10 * TOL[dtype] * want["abs_div"]
    eng.close(); twin.close()


# 2. score over the training coordinates of a masked beta engine agrees with the engine's own error (constant W: the error refers to the current pair)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("beta", [0.5, 1.0, 0.0])
def test_score_agrees_with_the_engines_own_error(beta, dtype):
    m, n, r = A[0], A[1], 9
    rng = np.random.default_rng(17)
    mask = rng.random((m, n)) < 0.3
    rows, cols = (a.astype(np.int32) for a in np.nonzero(mask))
    vals = (rng.random(len(rows)) + 0.1).astype(dtype)
    kw = dict(missing_divergence="is") if beta == 0 else dict(missing_divergence="kl") if beta == 1 else dict(missing_divergence="beta", missing_beta=beta)
    eng = na.Engine(m, n, r, "mu", dtype=dtype, missing_values=True, **kw)
    eng.upload_sparse(3, vals, rows, cols)
    eng.set_factors(F((1.0 - rng.random((m, r))).astype(dtype)), F((1.0 - rng.random((r, n))).astype(dtype)))
    eng.iterate(3, error_every=0)
    eng.iterate(1, first_iteration=4, error_every=0, last_iteration=4, constant_w=True)
    frob, div = eng.frobenius, eng.divergence_value
    got = eng.score(rows, cols, vals, beta=beta, return_predictions=True)
    nnz, u, eps = len(rows), U[dtype], eps_of(dtype)
    resid = np.abs(vals.astype(np.float64) - got["predictions"].astype(np.float64))
    b_sq = (pref.gamma(nnz, u) + 10 * TOL[dtype]) * got["sq"] + 2 * eps * float(resid.sum()) + nnz * eps * eps
    b_div = (pref.gamma(nnz, u) + 10 * TOL[dtype]) * got["abs_div"]
    print(f"beta {beta} {np.dtype(dtype).name}: sq {abs(got['sq'] - frob * frob) / b_sq:.3f} div {abs(got['div'] - div) / b_div:.3f} of their bounds")
    assert abs(got["sq"] - frob * frob) <= b_sq and abs(got["div"] - div) <= b_div
    assert got["rmsd"] == pytest.approx(eng.rmsd, rel=1e-4 if dtype == np.float32 else 1e-10) and (eng.frobenius, eng.divergence_value) == (frob, div)
    eng.close()


# 3. what it is for: the held-out KL of counts observed at 30 % of the entries (the problem of docs/MISSING.md), on the device
def test_held_out_kl_on_planted_poisson_counts():
    m, n, k, iters = 400, 300, 5, 300
    rng = np.random.default_rng(131)
    rate = 8.0 * rng.random((m, k)) @ rng.random((k, n))
    counts = rng.poisson(rate).astype(np.float64)
    mask = rng.random((m, n)) < 0.3
    rows, cols = (a.astype(np.int32) for a in np.nonzero(mask))
    hr, hc = (a.astype(np.int32) for a in np.nonzero(~mask))
    vals, held = counts[rows, cols].astype(np.float32), counts[hr, hc].astype(np.float32)
    eps, u, tol = eps_of(np.float32), U[np.float32], TOL[np.float32]
    held_out = {}
    for name, kw in (("masked kl", dict(missing_values=True, missing_divergence="kl")), ("plain kl", dict(sparse_compute=True, divergence="kl"))):
        eng = na.Engine(m, n, k, "mu", dtype=np.float32, **kw)
        eng.upload_sparse(3, vals, rows, cols)
        eng.randomize(7)
        eng.iterate(iters, first_iteration=1, error_every=0, last_iteration=iters)
        got = eng.score(hr, hc, held, beta=1.0)
        W, H = eng.get_factors()
        want = mbref.divergence(hr, hc, held, W, H, 1.0, eps)
        bound = (10 * tol + pref.gamma(k + 1, u)) * got["abs_div"]      # (k + 1: the dot product and the addition of eps)
        print(f"{name}: held-out KL {got['div']:.4e} (host {want:.4e}, {abs(got['div'] - want) / bound:.3f} of the bound) over {got['count']} entries")
        assert got["count"] == len(hr) and abs(got["div"] - want) <= bound
        held_out[name] = got["div"]
        eng.close()
    assert held_out["masked kl"] < 0.25 * held_out["plain kl"], held_out


# 4. the refusals, each with the word that names its cause
def test_refusals():
    name = "masked_beta_05"
    (m, n), r, dtype, _, _, _ = FAMILIES[name]
    p = problem(name)
    rows, cols, vals = p["rows"], p["cols"], p["vals"]
    eng = engine(name)
    torch = torch_()

    def refused(call, *words):
        with pytest.raises(na.EngineError) as err:
            call()
        assert err.value.status == 1
        for w in words:
            assert w in str(err.value), (w, str(err.value))
        return str(err.value)

    # a coordinate outside the matrix: the first bad p is named; on the device path the validation launch stops the gather
    bad_r = rows.copy(); bad_r[[700, 1500]] = m
    refused(lambda: eng.predict(bad_r, cols), "outside", "entry 700", "on the host")
    refused(lambda: eng.predict(rows, cols, base=1), "outside", "entry 0 ")
    bad_c = cols.copy(); bad_c[1999] = -1
    refused(lambda: eng.score(rows, bad_c, vals, beta=1.0), "outside", "entry 1999")
    sentinel = torch.full((2000,), float("nan"), dtype=torch.float32, device="cuda")
    d_rows, d_cols, d_bad_r = on_device(rows), on_device(cols), on_device(bad_r)
    st = eng._lib.nmfamd_engine_predict_device(eng._h, C.c_void_p(d_bad_r.data_ptr()), C.c_void_p(d_cols.data_ptr()), C.c_long(2000), 0, C.c_void_p(sentinel.data_ptr()))
    text = eng._lib.nmfamd_engine_last_error(eng._h).decode()
    assert st == 1 and "outside" in text and "entry 700" in text and "the gather was not launched" in text
    torch.cuda.synchronize()
    assert bool(torch.isnan(sentinel).all()), "a gather wrote predictions behind a failed validation"
    refused(lambda: eng.predict(on_device(rows), on_device(bad_c)), "outside", "entry 1999", "not launched")
    # a value that breaks the rule of the beta asked for
    zero = vals.copy(); zero[3] = 0
    neg = vals.copy(); neg[40] = -1
    inf = vals.copy(); inf[7] = np.inf
    refused(lambda: eng.score(rows, cols, zero, beta=0.0), "value 3", "> 0")
    refused(lambda: eng.score(rows, cols, neg, beta=1.0), "value 40", ">= 0")
    refused(lambda: eng.score(rows, cols, inf, beta=None), "value 7", "finite")
    refused(lambda: eng.score(on_device(rows), on_device(cols), on_device(zero), beta=-1.0), "value 3", "> 0")
    refused(lambda: eng.score(on_device(rows), on_device(cols), on_device(neg), beta=2.0), "value 40", ">= 0")
    assert np.isfinite(eng.score(rows, cols, zero, beta=0.5)["div"]) and np.isfinite(eng.score(rows, cols, neg, beta=None)["sq"])
    refused(lambda: eng.score(rows, cols, vals, beta=float("inf")), "beta")
    # host memory handed to the device entry
    out = np.zeros(2000, dtype)
    st = eng._lib.nmfamd_engine_predict_device(eng._h, C.c_void_p(rows.ctypes.data), C.c_void_p(cols.ctypes.data), C.c_long(2000), 0, C.c_void_p(out.ctypes.data))
    assert st == 1 and "rows: not device memory" in eng._lib.nmfamd_engine_last_error(eng._h).decode()
    st = eng._lib.nmfamd_engine_predict_device(eng._h, C.c_void_p(d_rows.data_ptr()), C.c_void_p(d_cols.data_ptr()), C.c_long(2000), 0, C.c_void_p(out.ctypes.data))
    assert st == 1 and "out: not device memory" in eng._lib.nmfamd_engine_last_error(eng._h).decode()
    # mismatched lengths, host and device arrays mixed, no entry at all
    with pytest.raises(ValueError, match="length"):
        eng.predict(rows, cols[:-1])
    with pytest.raises(ValueError, match="length"):
        eng.score(rows, cols, vals[:-1], beta=1.0)
    with pytest.raises(ValueError, match="length"):
        eng.predict(on_device(rows), on_device(cols[:-1]))
    with pytest.raises(TypeError):
        eng.predict(on_device(rows), cols)
    refused(lambda: eng.predict(rows[:0], cols[:0]), "nnz")
    # after all that the engine still answers
    assert np.all(np.isfinite(eng.predict(rows, cols)))
    eng.close()
    # an engine with row blocks holds a column shard; an engine without factors has nothing to predict from
    blocks = na.Engine(A[0], A[1], 7, "mu", row_blocks=2)
    blocks.randomize(3)
    refused(lambda: blocks.predict(rows, cols), "row blocks")
    blocks.close()
    empty = na.Engine(A[0], A[1], 7, "mu")
    refused(lambda: empty.predict(rows, cols), "no factors")
    empty.randomize(3, w=True, h=False)
    refused(lambda: empty.predict(rows, cols), "no factors")
    empty.randomize(3, w=False, h=True)
    assert np.all(np.isfinite(empty.predict(rows, cols)))      # (no upload of V is needed)
    empty.close()
