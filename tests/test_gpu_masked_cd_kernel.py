"""One launch of the coordinate-descent half-step over the observed entries (kernels_masked_cd.hip, docs/MISSING.md "Coordinate descent") through
na.op_masked_cd_half_step, against tests/masked_cd_reference.py: both precisions, padded rank 64 at r = 1, 63, 64 and 128 at r = 65, 127, 128, a gathered panel of
137 rows of which 120 are valid, 24 rows of 0 ... 200 entries with unsorted and duplicated indices.

No expectation assumes the kernel's lane mapping or summation order: the integer problems are exact in any order, and the real-valued ones are held to
hals_multi_cases.TOL_F64 in fp64 and, in fp32, to hals_multi_cases.MARGIN times the distance between the float32 and the fp64 restatement ON THE SAME CASE, computed
here on the CPU -- never to anything the kernel returned."""
import numpy as np
import pytest

import nmfgpu_amd as na
from tests import hals_multi_cases as hm
from tests import masked_cd_reference as cd

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
RANKS = [1, 63, 64, 65, 127, 128]
B_ROWS, B_VALID = 137, 120
LENGTHS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 200)      # around the 32-entry staging tile, and a long row
ROW_LENGTHS = LENGTHS * 2 + (0, 1, 33, 65)
EXTRA = 3                                             # rows of A past the launch
CASES = [(dt, r) for dt in DTYPES for r in RANKS]


def ident(case):
    return f"{np.dtype(case[0]).name}-r{case[1]}"


def padded(r):
    return 64 if r <= 64 else 128


def image(seed, lengths=ROW_LENGTHS):
    """ptr, idx: unsorted indices into the valid rows of the gathered panel; every third row with two entries or more repeats its first index."""
    rng = np.random.default_rng(seed)
    lengths = rng.permutation(np.asarray(lengths))
    ptr = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
    idx = rng.integers(0, B_VALID, int(ptr[-1])).astype(np.int32)
    for i in range(0, len(lengths), 3):
        if lengths[i] >= 2:
            idx[ptr[i] + 1] = idx[ptr[i]]
    return ptr, idx, lengths


def panels(dtype, r, rng, rows, integer=False):
    """A (rows + EXTRA, RP) and B (B_ROWS, RP) with zero padding: integers 0 ... 3 in B and 0 ... 7 in A, or reals in (0, 1]."""
    RP = padded(r)
    A = np.zeros((rows + EXTRA, RP), dtype); B = np.zeros((B_ROWS, RP), dtype)
    if integer:
        A[:, :r] = rng.integers(0, 8, (rows + EXTRA, r)); B[:B_VALID, :r] = rng.integers(0, 4, (B_VALID, r))
    else:
        A[:, :r] = 1.0 - rng.random((rows + EXTRA, r)); B[:B_VALID, :r] = 1.0 - rng.random((B_VALID, r))
    return A, B


def garbage(A, B, r, rng):
    """Finite garbage, large and of both signs, in the coordinates >= r of A and B and in the rows of B past the valid ones."""
    A, B = A.copy(), B.copy()
    A[:, r:] = rng.uniform(-1e6, 1e6, A[:, r:].shape)
    B[:, r:] = rng.uniform(-1e6, 1e6, B[:, r:].shape)
    B[B_VALID:] = rng.uniform(-1e6, 1e6, B[B_VALID:].shape)
    return A, B


@pytest.mark.parametrize("case", CASES, ids=ident)
def test_normal_equations_are_exact(case):
    """Integer B and val: G_i and c_i equal the integer sums bit for bit (every sum is below 2^24), zero at the coordinates >= r and for the empty rows."""
    dtype, r = case
    rng = np.random.default_rng(100 + r)
    ptr, idx, lengths = image(r)
    rows, RP = len(lengths), padded(r)
    A, B = panels(dtype, r, rng, rows, integer=True)
    val = rng.integers(0, 6, len(idx)).astype(dtype)
    Ag, Bg = garbage(A, B, r, rng)
    res = na.op_masked_cd_half_step(ptr, idx, val, Ag, Bg, rows, r, normal=True)
    assert res["G"].shape == (rows, RP, RP) and res["c"].shape == (rows, RP)
    assert res["G"].dtype == dtype and np.all(np.isfinite(res["G"])) and np.all(np.isfinite(res["c"]))
    want_G = np.zeros((rows, RP, RP)); want_c = np.zeros((rows, RP))
    for i in range(rows):
        Bi = B[idx[ptr[i]:ptr[i + 1]]].astype(np.int64)
        want_G[i] = Bi.T @ Bi
        want_c[i] = Bi.T @ val[ptr[i]:ptr[i + 1]].astype(np.int64)
    assert want_G.max() < 2 ** 24 and want_c.max() < 2 ** 24
    assert np.array_equal(res["G"], want_G.astype(dtype))
    assert np.array_equal(res["c"], want_c.astype(dtype))
    assert np.all(res["G"][:, r:, :] == 0) and np.all(res["G"][:, :, r:] == 0) and np.all(res["c"][:, r:] == 0)
    assert np.all(res["G"][lengths == 0] == 0)


def exact_case(dtype, r, ridge, seed):
    """Every gathered row has ONE non-zero coordinate (row j: coordinate j mod r), a power of two, and a row of the image hits a coordinate once or four times (the same
    index four times), so G_i is diagonal.  ridge = False: values 2^-2 ... 2^2, l2 = 0: G_kk is a power of two.  ridge = True: the rows hit once hold 1 and the rows hit
    four times 1/2, l2 = 1: G_kk + l2 = 2.  A and val small integers, l1 dyadic: every step of a sweep is exact in fp32."""
    rng = np.random.default_rng(seed)
    RP = padded(r)
    B = np.zeros((B_ROWS, RP), dtype)
    j = np.arange(B_VALID)
    once = j < 60
    B[j, j % r] = np.where(once, 1.0, 0.5) if ridge else 2.0 ** ((j % 5) - 2)
    rows = 12
    entries, lengths = [], []
    for i in range(rows):
        if i in (4, 9):
            lengths.append(0)
            continue
        ks = rng.choice(min(r, B_VALID), size=rng.integers(1, min(r, 40) + 1), replace=False)
        row = []
        for k in ks:
            cand = j[j % r == k]
            if ridge:
                pick = int(rng.choice(cand))
                row += [pick] * (1 if once[pick] else 4)
            else:
                row += [int(rng.choice(cand))] * int(rng.choice((1, 4)))
        row = list(rng.permutation(row))
        entries += row
        lengths.append(len(row))
    ptr = np.concatenate(([0], np.cumsum(lengths))).astype(np.int32)
    idx = np.asarray(entries, dtype=np.int32)
    val = rng.integers(0, 8, len(idx)).astype(dtype)
    A = np.zeros((rows + EXTRA, RP), dtype)
    A[:, :r] = rng.integers(0, 8, (rows + EXTRA, r))
    return ptr, idx, val, A, B, rows, ((0.25, 1.0) if ridge else (0.5, 0.0))


@pytest.mark.parametrize("ridge", [False, True], ids=["l2=0", "l2=1"])
@pytest.mark.parametrize("case", CASES, ids=ident)
def test_sweeps_are_exact(case, ridge):
    """Diagonal G_i with powers of two: the new panel equals the fp64 restatement cast to the kernel's type, bit for bit, after 1, 2 and 5 sweeps."""
    dtype, r = case
    ptr, idx, val, A, B, rows, (l1, l2) = exact_case(dtype, r, ridge, 200 + r)
    for sweeps in (1, 2, 5):
        want, G, _ = cd.half_step(ptr, idx, val, A, B, r, rows, sweeps, l1, l2)
        assert all(np.count_nonzero(G[i] - np.diag(np.diag(G[i]))) == 0 for i in range(rows))
        got = na.op_masked_cd_half_step(ptr, idx, val, A, B, rows, r, sweeps, l1, l2)["A"]
        assert np.array_equal(got, want.astype(dtype)), sweeps
        assert np.array_equal(got[rows:], A[rows:])
    assert np.any(want[:rows, :r] != A[:rows, :r])


@pytest.mark.parametrize("sweeps,l1,l2", [(1, 0.0, 0.0), (3, 0.05, 0.01)], ids=["s1", "s3-pen"])
@pytest.mark.parametrize("case", CASES, ids=ident)
def test_real_valued_panels(case, sweeps, l1, l2):
    dtype, r = case
    rng = np.random.default_rng(300 + r)
    ptr, idx, lengths = image(50 + r)
    rows = len(lengths)
    A, B = panels(dtype, r, rng, rows)
    val = rng.integers(1, 6, len(idx)).astype(dtype)
    l1, l2 = float(dtype(l1)), float(dtype(l2))
    want, G, c = cd.half_step(ptr, idx, val, A, B, r, rows, sweeps, l1, l2)
    if dtype == np.float64:
        tol = hm.TOL_F64
    else:
        figure = hm.rel(cd.half_step_in(ptr, idx, val, A, B, r, rows, sweeps, l1, l2)[:rows], want[:rows])
        tol = hm.MARGIN * figure
        print(f"{ident(case)} sweeps {sweeps}: float32 restatement {figure:.2e}")
    res = na.op_masked_cd_half_step(ptr, idx, val, A, B, rows, r, sweeps, l1, l2, normal=True)
    got = res["A"]
    dist = hm.rel(got[:rows], want[:rows])
    print(f"{ident(case)} sweeps {sweeps}: kernel {dist:.2e} (tolerance {tol:.2e})")
    assert np.all(np.isfinite(got)) and dist <= tol, (dist, tol)
    assert np.all(got[:rows] >= 0) and np.all(got[:rows, r:] == 0)
    assert np.all(got[:rows][lengths == 0] == 0), "a row without an entry becomes 0"
    assert np.array_equal(got[rows:], A[rows:]), "rows past the launch were touched"
    # the normal equations: a k-ordered chain of the type's own fused multiply-adds, within the type's rounding of a sum of `length` positive terms
    u = hm.UNIT[dtype]
    assert np.all(np.abs(res["G"][:, :r, :r] - G) <= 2 * (lengths.max() + 1) * u * np.abs(G) + 1e-300)
    assert np.all(np.abs(res["c"][:, :r] - c) <= 2 * (lengths.max() + 1) * u * np.abs(c) + 1e-300)
    assert np.array_equal(res["G"], np.swapaxes(res["G"], 1, 2)), "G_i is symmetric bit for bit"


@pytest.mark.parametrize("case", CASES, ids=ident)
def test_garbage_does_not_reach_the_result(case):
    """Garbage in the coordinates >= r of A and B and in the rows of B past the valid ones: the same bits as with clean padding, and coordinates >= r of A exactly 0."""
    dtype, r = case
    rng = np.random.default_rng(400 + r)
    ptr, idx, lengths = image(60 + r)
    rows = len(lengths)
    A, B = panels(dtype, r, rng, rows)
    val = (1.0 - rng.random(len(idx))).astype(dtype)
    Ag, Bg = garbage(A, B, r, rng)
    clean = na.op_masked_cd_half_step(ptr, idx, val, A, B, rows, r, 2, 0.05, 0.01, normal=True)
    dirty = na.op_masked_cd_half_step(ptr, idx, val, Ag, Bg, rows, r, 2, 0.05, 0.01, normal=True)
    for key in ("G", "c"):
        assert np.array_equal(clean[key], dirty[key]), key
    assert np.array_equal(clean["A"][:rows], dirty["A"][:rows])
    assert np.array_equal(dirty["A"][rows:], Ag[rows:])
    assert np.all(dirty["A"][:rows, r:] == 0)
    assert np.all(dirty["A"][:rows][lengths == 0] == 0), "an empty row becomes 0 whatever it held"


@pytest.mark.parametrize("case", CASES, ids=ident)
def test_skipped_steps_keep_the_old_value(case):
    """A coordinate no gathered row touches has d_k = 0 at l2 = 0: in a row with entries it keeps its old value, bit for bit; in a row without, it becomes 0."""
    dtype, r = case
    rng = np.random.default_rng(500 + r)
    ptr, idx, lengths = image(70 + r)
    rows = len(lengths)
    A, B = panels(dtype, r, rng, rows)
    dead = sorted({0, r // 2, r - 1})
    B[:, dead] = 0
    val = (1.0 - rng.random(len(idx))).astype(dtype)
    got = na.op_masked_cd_half_step(ptr, idx, val, A, B, rows, r, 3, 0.05, 0.0)["A"]
    live = lengths > 0
    assert np.array_equal(got[:rows][live][:, dead], A[:rows][live][:, dead])
    assert np.all(got[:rows][~live] == 0)
    if r > len(dead):
        assert np.any(got[:rows][live] != A[:rows][live])
    # with l2 > 0 the step is taken: max(0, p - (l2 p + l1) / l2) = 0
    ridge = na.op_masked_cd_half_step(ptr, idx, val, A, B, rows, r, 1, 0.05, 0.5)["A"]
    assert np.all(ridge[:rows][:, dead] == 0)


@pytest.mark.parametrize("case", CASES, ids=ident)
def test_determinism_and_independence_of_rows(case):
    """Two launches give the same bits, and the bits of a row do not depend on which other rows the launch holds."""
    dtype, r = case
    rng = np.random.default_rng(600 + r)
    ptr, idx, lengths = image(80 + r)
    rows = len(lengths)
    A, B = panels(dtype, r, rng, rows)
    val = (1.0 - rng.random(len(idx))).astype(dtype)
    one = na.op_masked_cd_half_step(ptr, idx, val, A, B, rows, r, 2, 0.05, 0.01, normal=True)
    two = na.op_masked_cd_half_step(ptr, idx, val, A, B, rows, r, 2, 0.05, 0.01, normal=True)
    for key in ("A", "G", "c"):
        assert np.array_equal(one[key], two[key]), key
    keep = [i for i in range(rows) if i % 3 != 1][::-1]      # a subset of the rows, in another order
    sub_ptr = np.concatenate(([0], np.cumsum(lengths[keep]))).astype(np.int32)
    sub_idx = np.concatenate([idx[ptr[i]:ptr[i + 1]] for i in keep]).astype(np.int32)
    sub_val = np.concatenate([val[ptr[i]:ptr[i + 1]] for i in keep]).astype(dtype)
    sub = na.op_masked_cd_half_step(sub_ptr, sub_idx, sub_val, A[keep], B, len(keep), r, 2, 0.05, 0.01, normal=True)
    assert np.array_equal(sub["A"], one["A"][keep])
    assert np.array_equal(sub["G"], one["G"][keep]) and np.array_equal(sub["c"], one["c"][keep])


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_refusals(dtype):
    rng = np.random.default_rng(9)
    ptr, idx, lengths = image(9)
    rows = len(lengths)
    A, B = panels(dtype, 64, rng, rows)
    val = np.ones(len(idx), dtype)
    ok = na.op_masked_cd_half_step(ptr, idx, val, A, B, rows, 64)["A"]
    assert np.all(np.isfinite(ok))

    def refused(*args, **kw):
        with pytest.raises(na.EngineError) as info:
            na.op_masked_cd_half_step(*args, **kw)
        assert info.value.status == 1

    for RP in (32, 192, 256):      # the padded ranks without an instantiation
        refused(ptr, idx, val, np.zeros((rows, RP), dtype), np.zeros((B_ROWS, RP), dtype), rows, min(RP, 64))
    refused(ptr, idx, val, A, B, rows, 0)
    refused(ptr, idx, val, A, B, rows, 65)
    refused(ptr, idx, val, A, B, rows, 64, 0)
    refused(ptr, idx, val, A, B, rows, 64, 65)
    for bad in (-0.5, float("nan"), float("inf")):
        refused(ptr, idx, val, A, B, rows, 64, 1, bad, 0.0)
        refused(ptr, idx, val, A, B, rows, 64, 1, 0.0, bad)
    outside = idx.copy()
    outside[5] = B_ROWS
    refused(ptr, outside, val, A, B, rows, 64)
    with pytest.raises(ValueError):
        na.op_masked_cd_half_step(ptr, idx, val, A[:rows - 1], B, rows, 64)
