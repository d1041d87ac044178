"""One launch of the masked beta-divergence half-step (kernels_masked_beta.hip, docs/MISSING.md "Beta-divergence") through na.op_masked_beta_half_step, against the
entry-list restatement (tests/masked_beta_reference.py): every instantiation (fp32 / fp64 x padded rank 64 / 128 / 256 x KL / Itakura-Saito / general map x update /
update + terms / terms only), at the smallest shapes that reach each path.

Bounds (docs/DIVERGENCE.md, "Kernel-level tests"): the project's half-step bound on the panel -- norm-relative 1e-5 in fp32, 1e-12 in fp64 -- and ten times that on
the sums of squares and on the per-row terms.  The divergence term of a row is a sum with cancellation, so its bound is on the sum of the absolute values of its
summands, never relative to the result (same section)."""
import numpy as np
import pytest

import nmfgpu_amd as na
from tests import masked_beta_reference as mbref

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
TOL = {np.float32: 1e-5, np.float64: 1e-12}
MAPS = [("kl", None, 1.0), ("is", None, 0.0), ("beta", 0.5, 0.5)]      # (divergence, beta of the entry, beta of the restatement)
FORMS = ["update", "update+terms", "terms"]
LENGTHS = (0, 1, 7, 8, 9, 17)      # before, at and past the 8-entry step of a wave
B_ROWS = 40


def rel(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b), 1e-300))


def case(rows, r, dtype, seed, lengths=None):
    """A CSR image of `rows` rows with lengths drawn from LENGTHS (every length present when rows allow), ascending indices into a gathered panel of B_ROWS rows,
    integer values 1 .. 5; A with three further rows that no launch may touch; padding coordinates zero in A and B."""
    rng = np.random.default_rng(seed)
    RP = 64 if r <= 64 else 128 if r <= 128 else 256
    if lengths is None:
        lengths = rng.permutation(np.resize(LENGTHS, rows)) if rows >= len(LENGTHS) else rng.choice(LENGTHS[1:], rows)
    ptr = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
    idx = np.concatenate([np.sort(rng.choice(B_ROWS, int(k), replace=False)) for k in lengths] + [np.zeros(0, np.int64)]).astype(np.int32)
    val = rng.integers(1, 6, len(idx)).astype(dtype)
    A = np.zeros((rows + 3, RP), dtype); A[:, :r] = 1.0 - rng.random((rows + 3, r))
    B = np.zeros((B_ROWS, RP), dtype); B[:, :r] = 1.0 - rng.random((B_ROWS, r))
    keys = np.repeat(np.arange(rows), lengths)
    return dict(ptr=ptr, idx=idx, val=val, A=A, B=B, keys=keys, rows=rows, r=r, RP=RP, lengths=np.asarray(lengths))


def groups_of_part(part, parts, rows):
    """The rows workgroup `part` of a launch with sums of squares owns: row groups part, part + parts, ..."""
    out = []
    for rg in range(part, (rows + 3) // 4, parts):
        out.extend(range(4 * rg, min(4 * rg + 4, rows)))
    return out


def check(c, res, beta, form, l1, l2, dtype, what):
    tol, eps = TOL[dtype], float(np.finfo(dtype).eps)
    rows, r = c["rows"], c["r"]
    A64, B64, v64 = c["A"].astype(np.float64)[:rows, :r], c["B"].astype(np.float64)[:, :r], c["val"].astype(np.float64)
    got = res["A"]
    assert np.array_equal(got[rows:], c["A"][rows:]), "rows past the launch were touched"
    if form == "terms":
        assert np.array_equal(got, c["A"]), "the terms-only form wrote A"
        assert res["sumsq_part"] is None
    else:
        want = mbref.half_step(c["keys"], c["idx"], v64, A64, B64, beta, eps, float(dtype(l1)), float(dtype(l2)))
        figure = rel(got[:rows, :r], want)
        print(f"{what}: panel {figure:.2e}")
        assert np.all(np.isfinite(got)) and figure < tol, figure
        assert np.all(got[:rows, r:] == 0), "padding coordinates"
        assert np.all(got[:rows][c["lengths"] == 0] == 0), "a row without an entry becomes 0"
        parts = na.masked_norm_parts(rows)
        assert res["sumsq_part"].shape == (parts, c["RP"])
        g64 = got.astype(np.float64)
        for part in range(parts):
            own = groups_of_part(part, parts, rows)
            assert np.allclose(res["sumsq_part"][part], (g64[own] ** 2).sum(axis=0), rtol=10 * tol, atol=0), part
    if form == "update":
        assert res["t_frob"] is None and res["t_div"] is None
    else:
        tf, td, ta = mbref.terms(c["keys"], c["idx"], v64, A64, B64, beta, eps)
        ef = np.max(np.abs(res["t_frob"] - tf) / np.maximum(tf, 1e-300)) if len(v64) else 0.0
        ed = np.max(np.abs(res["t_div"] - td) / np.maximum(ta, 1e-300)) if len(v64) else 0.0
        print(f"{what}: terms frobenius {ef:.2e} divergence {ed:.2e} (of the absolute summands)")
        assert np.all(np.abs(res["t_frob"] - tf) <= 10 * tol * tf) and np.all(np.abs(res["t_div"] - td) <= 10 * tol * ta)
        assert np.all(res["t_frob"][c["lengths"] == 0] == 0) and np.all(res["t_div"][c["lengths"] == 0] == 0)


def launch(c, divergence, beta, form, l1=0.0, l2=0.0):
    return na.op_masked_beta_half_step(c["ptr"], c["idx"], c["val"], c["A"], c["B"], c["rows"], divergence, beta, l1=l1, l2=l2, update=form != "terms",
                                       terms=form != "update", sumsq=form != "terms")


# 1. every instantiation, rows not a multiple of the four waves, with and without penalties
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("r", [8, 64, 65, 128, 200, 256])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("which", MAPS, ids=[m[0] for m in MAPS])
def test_every_instantiation(which, form, r, dtype):
    divergence, beta_arg, beta = which
    for rows in (1, 5, 130):
        c = case(rows, r, dtype, seed=rows + r)
        for l1, l2 in ((0.0, 0.0), (0.05, 0.01)):
            res = launch(c, divergence, beta_arg, form, l1, l2)
            check(c, res, beta, form, l1, l2, dtype, f"{divergence} {form} r {r} rows {rows} {np.dtype(dtype).name} ({l1}, {l2})")
            again = launch(c, divergence, beta_arg, form, l1, l2)      # a repeated launch: bit-identical
            for k in ("A", "t_frob", "t_div", "sumsq_part"):
                assert (res[k] is None and again[k] is None) or np.array_equal(res[k], again[k]), k


# 2. the other exponents gamma of the general map: 1/3 (beta -1), 1 (1.5, 2), 1/2 (3)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("beta", [-1.0, 1.5, 2.0, 3.0])
def test_general_map_at_every_gamma(beta, dtype):
    c = case(130, 65, dtype, seed=int(10 * beta) + 50)
    for l1, l2 in ((0.0, 0.0), (0.05, 0.01)):
        res = launch(c, "beta", beta, "update+terms", l1, l2)
        check(c, res, beta, "update+terms", l1, l2, dtype, f"beta {beta} {np.dtype(dtype).name} ({l1}, {l2})")


# 3. beta = 0 and beta = 1 through the general selector run the Itakura-Saito and the KL forms, bit for bit
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("r", [8, 128, 256])
def test_general_selector_at_0_and_1(r, dtype):
    c = case(130, r, dtype, seed=60 + r)
    for named, beta in (("is", 0.0), ("kl", 1.0)):
        for form in FORMS:
            a, b = launch(c, named, None, form, 0.05, 0.01), launch(c, "beta", beta, form, 0.05, 0.01)
            for k in ("A", "t_frob", "t_div", "sumsq_part"):
                assert (a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]), (named, form, k)
    # ... and they are three different maps
    assert not np.array_equal(launch(c, "is", None, "update")["A"], launch(c, "kl", None, "update")["A"])
    assert not np.array_equal(launch(c, "beta", 0.5, "update")["A"], launch(c, "kl", None, "update")["A"])


# 4. more row groups than MASKED_NORM_PARTS: the workgroups stride, and the partial sums of squares follow them
@pytest.mark.parametrize("dtype", DTYPES)
def test_workgroups_stride_past_the_norm_parts(dtype):
    rows = 8200
    c = case(rows, 8, dtype, seed=70, lengths=np.full(rows, 3))
    assert na.masked_norm_parts(rows) == 2048 and (rows + 3) // 4 == 2050
    res = launch(c, "kl", None, "update+terms")
    check(c, res, 1.0, "update+terms", 0.0, 0.0, dtype, f"8200 rows {np.dtype(dtype).name}")
    # without sums of squares the grid is one workgroup per row group: the same rows, bit for bit
    plain = na.op_masked_beta_half_step(c["ptr"], c["idx"], c["val"], c["A"], c["B"], rows, "kl", None, update=True, terms=True, sumsq=False)
    assert np.array_equal(plain["A"], res["A"]) and np.array_equal(plain["t_div"], res["t_div"]) and plain["sumsq_part"] is None


# 5. what the entry refuses
def test_refusals():
    c = case(5, 8, np.float32, seed=80)
    for kw in (dict(beta=float("nan")), dict(beta=float("inf")), dict(beta=0.5, l1=-1.0), dict(beta=0.5, l2=float("inf"))):
        with pytest.raises(na.EngineError) as err:
            na.op_masked_beta_half_step(c["ptr"], c["idx"], c["val"], c["A"], c["B"], 5, "beta", **kw)
        assert err.value.status == 1
    with pytest.raises(na.EngineError):      # nothing to write
        na.op_masked_beta_half_step(c["ptr"], c["idx"], c["val"], c["A"], c["B"], 5, "kl", update=False, terms=False)
    with pytest.raises(na.EngineError):      # sums of squares belong to an update
        na.op_masked_beta_half_step(c["ptr"], c["idx"], c["val"], c["A"], c["B"], 5, "kl", update=False, terms=True, sumsq=True)
    bad = c["idx"].copy(); bad[0] = B_ROWS
    with pytest.raises(na.EngineError):      # an index outside the gathered panel
        na.op_masked_beta_half_step(c["ptr"], bad, c["val"], c["A"], c["B"], 5, "kl")
    with pytest.raises(na.EngineError):      # a padded rank without a kernel
        na.op_masked_beta_half_step(c["ptr"], c["idx"], c["val"], np.ones((8, 192), np.float32), np.ones((B_ROWS, 192), np.float32), 5, "kl")
