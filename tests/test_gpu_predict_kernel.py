"""One launch of the gather of kernels_predict.hip (docs/PREDICT.md) through na.op_predict_entries, against the fp64 restatement (tests/predict_reference.py): every
instantiated (dtype, padded rank) at r = previous padded rank + 1, RP - 1 and RP, on panels of 128 + 128 rows, at every entry count at which the launch takes
another path: 1, around the sixteen groups of a workgroup (15, 16, 17), around one workgroup pass of 32 entries (31, 32, 33) and one full grid stride plus one
(2048 * 32 + 1: workgroup 0 takes a second pass).

Bounds, none of them measured:
  predictions   |out[p] - exact| <= gamma_r(u) sum_k |w_k h_k|, u = 2^-24 or 2^-53: the standard bound of a dot product of r terms in any order.
  sq            against the fp64 sum of (v - out)^2 over the kernel's own predictions: the subtraction, the square and the conversion are three roundings of T, the
                sum is nnz additions in double: (gamma_3(u) + gamma_nnz(2^-53)) sq.
  div, abs_div  against the fp64 definitions on the kernel's own predictions: the per-term bound tests/test_gpu_masked_beta_kernel.py holds for t_div, ten times
                TOL, taken on the absolute summands (abs_div) -- it is the same arithmetic."""
import numpy as np
import pytest

import nmfgpu_amd as na
from tests import predict_reference as pref

pytestmark = pytest.mark.gpu

TOL = {np.float32: 1e-5, np.float64: 1e-12}
U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
RANKS = {np.float32: [64, 128, 256, 384, 512], np.float64: [64, 128, 192, 256, 320, 384, 448, 512]}
PASS, GRID = 32, 2048
COUNTS = (1, 15, 16, 17, PASS - 1, PASS, PASS + 1, GRID * PASS + 1)
M, N, ROWS = 125, 120, 128      # the valid rows of W and columns of H inside panels of 128 + 128 rows
BETAS = [1.0, 0.0, 0.5, 2.0, None, -1.0, 1.5, 3.0]
CASES = [(dt, RP, r) for dt in (np.float32, np.float64) for i, RP in enumerate(RANKS[dt]) for r in ((RANKS[dt][i - 1] if i else 0) + 1, RP - 1, RP)]
_cache = {}


def eps_of(dtype):
    return float(np.finfo(dtype).eps)


def panels(dtype, RP, r, garbage=False):
    """Wt (ROWS, RP) and H (ROWS, RP) with values in (0, 1] at the M / N valid rows and the r valid coordinates; the padding zero or, with garbage, finite garbage."""
    rng = np.random.default_rng(RP + r)
    Wt = np.zeros((ROWS, RP), dtype); H = np.zeros((ROWS, RP), dtype)
    Wt[:M, :r] = 1.0 - rng.random((M, r)); H[:N, :r] = 1.0 - rng.random((N, r))
    if garbage:
        for P, valid in ((Wt, M), (H, N)):
            P[:, r:] = np.where(np.arange(RP - r) % 2 == 0, 1e30, -7.5)[None, :]
            P[valid:, :r] = -3e20
    return Wt, H


def entries(nnz, base, seed):
    """nnz coordinates, unsorted, with duplicates, the two corners among them; values 1 ... 5."""
    key = (nnz, base, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        rows, cols = rng.integers(0, M, nnz), rng.integers(0, N, nnz)
        rows[-1], cols[-1] = M - 1, N - 1
        if nnz > 1:
            rows[0], cols[0] = 0, 0
        if nnz > 3:
            rows[2], cols[2] = rows[1], cols[1]      # a duplicate next to its copy, whatever the draw
        _cache[key] = ((rows + base).astype(np.int32), (cols + base).astype(np.int32), rng.integers(1, 6, nnz))
    return _cache[key]


def launch(rows, cols, vals, Wt, H, r, beta, base, dtype, score=True):
    return na.op_predict_entries(rows, cols, Wt, H, r, vals=vals.astype(dtype) if score else None, beta=beta, base=base, out_len=len(rows) + 5)


def same(a, b):
    return (a is None and b is None) or np.asarray(a).tobytes() == np.asarray(b).tobytes()


def check(res, rows, cols, vals, Wt, H, r, beta, base, dtype, what):
    nnz, u, tol = len(rows), U[dtype], TOL[dtype]
    out = res["out"]
    assert out.shape == (nnz + 5,) and np.all(np.isnan(out[nnz:])), "the sentinels past nnz"
    exact, mag = pref.predict(rows, cols, Wt[:, :r], H[:, :r].T, base)
    err = np.abs(out[:nnz].astype(np.float64) - exact)
    bound = pref.gamma(r, u) * mag
    print(f"{what}: predictions {float(np.max(err / bound)):.2f} of the bound", end="")
    assert np.all(np.isfinite(out[:nnz])) and np.all(err <= bound)
    if res["part"] is None:
        print()
        return
    assert res["part"].shape == (na.predict_entry_parts(nnz), 3) and np.all(np.isfinite(res["part"]))
    want = pref.score_of_predictions(vals, out[:nnz].astype(np.float64), beta, eps_of(dtype))
    e_sq = abs(res["sq"] - want["sq"])
    b_sq = (pref.gamma(3, u) + pref.gamma(nnz, 2.0 ** -53)) * want["sq"]
    print(f", sq {e_sq / max(b_sq, 1e-300):.2f} of the bound", end="")
    assert e_sq <= b_sq
    if beta is None:
        assert np.isnan(res["div"]) and np.isnan(res["abs_div"]) and np.all(res["part"][:, 1:] == 0)
        print()
        return
    e_div, e_abs = abs(res["div"] - want["div"]) / want["abs_div"], abs(res["abs_div"] - want["abs_div"]) / want["abs_div"]
    print(f", div {e_div:.2e} abs_div {e_abs:.2e} (of the absolute summands)")
    assert e_div <= 10 * tol and e_abs <= 10 * tol


# 1. every instantiation at the three ranks, every entry count, both index bases; garbage in the padding; a repeated launch
@pytest.mark.parametrize("dtype,RP,r", CASES, ids=[f"{np.dtype(c[0]).name}-{c[1]}-{c[2]}" for c in CASES])
def test_every_instantiation(dtype, RP, r):
    Wt, H = panels(dtype, RP, r)
    Wg, Hg = panels(dtype, RP, r, garbage=True)
    for k, nnz in enumerate(COUNTS):
        beta = BETAS[(k + r) % len(BETAS)]
        for base in ((0, 1) if nnz < 1000 else (1,)):
            rows, cols, vals = entries(nnz, base, seed=nnz)
            what = f"{np.dtype(dtype).name} RP {RP} r {r} nnz {nnz} base {base} beta {beta}"
            res = launch(rows, cols, vals, Wt, H, r, beta, base, dtype)
            check(res, rows, cols, vals, Wt, H, r, beta, base, dtype, what)
            again = launch(rows, cols, vals, Wt, H, r, beta, base, dtype)
            dirty = launch(rows, cols, vals, Wg, Hg, r, beta, base, dtype)
            for key in ("out", "part"):
                assert same(res[key], again[key]), f"{what}: a repeated launch changed {key}"
                assert same(res[key], dirty[key]), f"{what}: the padding reached {key}"
            # predictions alone: the same bits, no sums
            plain = launch(rows, cols, vals, Wt, H, r, None, base, dtype, score=False)
            assert same(plain["out"], res["out"]) and plain["part"] is None


# 2. every beta at one shape of each precision, and the score without predictions
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("beta", [-1.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0, None])
def test_every_beta(beta, dtype):
    RP, r, nnz = 128, 70, 3 * PASS + 7
    Wt, H = panels(dtype, RP, r)
    rows, cols, vals = entries(nnz, 0, seed=9)
    if beta is None or beta > 0:
        vals = vals - 1      # zeros among the values: v^beta = 0 at v = 0, v log v = 0
    res = launch(rows, cols, vals, Wt, H, r, beta, 0, dtype)
    check(res, rows, cols, vals, Wt, H, r, beta, 0, dtype, f"{np.dtype(dtype).name} beta {beta}")
    blind = na.op_predict_entries(rows, cols, Wt, H, r, vals=vals.astype(dtype), beta=beta, want_out=False)
    assert blind["out"] is None and same(blind["part"], res["part"])
    if beta == 2.0:      # the general form there is half the squared error against out + eps
        assert res["div"] == pytest.approx(0.5 * res["sq"], rel=1e-3)


# 3. beta = 0 and beta = 1 are the Itakura-Saito and the KL forms, not the general one evaluated there (which divides by beta (beta - 1) = 0)
def test_special_forms_are_selected():
    Wt, H = panels(np.float32, 64, 8)
    rows, cols, vals = entries(100, 0, seed=4)
    a, b, c = (launch(rows, cols, vals, Wt, H, 8, beta, 0, np.float32) for beta in (0.0, 1.0, 0.5))
    assert np.isfinite(a["div"]) and np.isfinite(b["div"]) and len({a["div"], b["div"], c["div"]}) == 3
    # a beta that rounds to 1 in the precision of the panels is the KL form
    d = launch(rows, cols, vals, Wt, H, 8, 1.0 + 1e-12, 0, np.float32)
    assert same(b["part"], d["part"])


# 4. what the entry refuses
def test_refusals():
    Wt, H = panels(np.float32, 64, 8)
    rows, cols, vals = entries(17, 0, seed=1)
    none = np.zeros(0, np.int32)
    for args, kw in (((none, none, Wt, H, 8), {}),                                                      # nnz = 0
                     ((rows, cols, Wt, H, 0), {}), ((rows, cols, Wt, H, 65), {}),                       # r outside 1 ... RP
                     ((rows, cols, np.zeros((ROWS, 192), np.float32), np.zeros((ROWS, 192), np.float32), 8), {}),      # fp32 has no padded rank 192
                     ((rows, cols, np.zeros((ROWS, 576)), np.zeros((ROWS, 576)), 8), {}),               # nor fp64 one of 576
                     ((rows, cols, np.zeros((ROWS, 96)), np.zeros((ROWS, 96)), 8), {}),
                     ((rows + ROWS, cols, Wt, H, 8), {}), ((rows, cols - 1, Wt, H, 8), {}),             # a coordinate outside the panels
                     ((rows, cols, Wt, H, 8), dict(base=2)),
                     ((rows, cols, Wt, H, 8), dict(want_out=False)),                                    # nothing to write
                     ((rows, cols, Wt, H, 8), dict(vals=vals, beta=float("inf")))):
        with pytest.raises(na.EngineError) as err:
            na.op_predict_entries(*args, **kw)
        assert err.value.status == 1, (args[4:], kw)
