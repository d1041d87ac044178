"""The two launches of kernels_topk.hip (docs/TOPK.md) through na.op_top_k, against the fp64 restatement (tests/topk_reference.py).

Exact cases: panels of integers 0 ... 3 at the r valid coordinates.  Every dot product is an integer <= 9 * 512 < 2^24, exact in both precisions in any order, so
indices and scores must EQUAL the reference's bit for bit, and ties are frequent, which exercises the index tie-break.  Real-valued panels go through
check_top_k, whose bound is the standard one of a dot product of r terms in any order, gamma_r(u) sum |a b|, u = 2^-24 or 2^-53: none of it measured."""
import numpy as np
import pytest

import nmfgpu_amd as na
from tests import topk_reference as tref

pytestmark = pytest.mark.gpu

U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}
RANKS = {np.float32: [64, 128, 256, 384, 512], np.float64: [64, 128, 192, 256, 320, 384, 448, 512]}
CASES = [(dt, RP, r) for dt in (np.float32, np.float64) for i, RP in enumerate(RANKS[dt]) for r in ((RANKS[dt][i - 1] if i else 0) + 1, RP - 1, RP)]
COUNTS = (1, 31, 32, 33, 127, 128, 129)
NQS = (1, 31, 32, 33, 65)
KS = (1, 2, 31, 32, 33, 64)
A_VALID, ROWS = 120, 137      # rows of the query panel that queries name, inside panels of 137 rows: 8 rows past the largest count
_cache = {}


def panels(dtype, RP, r, count, kind="int", garbage=False):
    """A (ROWS, RP) and B (ROWS, RP): integers 0 ... 3 (or reals in (0, 1]) at the A_VALID / count valid rows and the r valid coordinates; the rest zero or, with
    garbage, finite garbage at k >= r and -3e20 in the rows past the valid ones."""
    key = (dtype, RP, r, count, kind)
    if key not in _cache:
        rng = np.random.default_rng(RP * 1000 + r + count)
        A = np.zeros((ROWS, RP), dtype); B = np.zeros((ROWS, RP), dtype)
        if kind == "int":
            A[:A_VALID, :r] = rng.integers(0, 4, (A_VALID, r)); B[:count, :r] = rng.integers(0, 4, (count, r))
        else:
            A[:A_VALID, :r] = 1.0 - rng.random((A_VALID, r)); B[:count, :r] = 1.0 - rng.random((count, r))
        _cache[key] = (A, B)
    A, B = _cache[key]
    if garbage:
        A, B = A.copy(), B.copy()
        for P, valid in ((A, A_VALID), (B, count)):
            P[:, r:] = np.where(np.arange(RP - r) % 2 == 0, 1e30, -7.5)[None, :]
            P[valid:, :r] = -3e20
    return A, B


def query_list(nq, base, seed, unused=None):
    """nq queries, unsorted, with a duplicate and both ends of the range among them; `unused`: a row nobody asks for."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, A_VALID, nq)
    if unused is not None:
        q[q == unused] = 0
    q[-1] = A_VALID - 1
    if nq > 1:
        q[0] = 0
    if nq > 3:
        q[2] = q[1]
    return (q + base).astype(np.int32)


def reference(A, B, count, r, queries, k, exclude, base):
    return tref.top_k(A[:, :r], B[:count, :r], queries, k, exclude, base)


def same(got, want, dtype):
    return np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].astype(dtype).tobytes()


def bits(res):
    return res[0].tobytes() + res[1].tobytes()


# 1. + 2. every instantiation at the three ranks; counts, query counts, k and the base cycle across the cases; garbage in the padding gives the same bits
@pytest.mark.parametrize("dtype,RP,r", CASES, ids=[f"{np.dtype(c[0]).name}-{c[1]}-{c[2]}" for c in CASES])
def test_exact_cases(dtype, RP, r):
    n = CASES.index((dtype, RP, r))
    for step, count in enumerate(COUNTS):
        nq, k, base = NQS[(n + step) % len(NQS)], KS[(n + 2 * step) % len(KS)], (n + step) % 2
        A, B = panels(dtype, RP, r, count)
        queries = query_list(nq, base, seed=n + step, unused=5)
        what = f"{np.dtype(dtype).name} RP {RP} r {r} count {count} nq {nq} k {k} base {base}"
        got = na.op_top_k(queries, k, A, B, count, r, base=base)
        want = reference(A, B, count, r, queries, k, None, base)
        assert got[0].dtype == np.int32 and got[1].dtype == dtype and same(got, want, dtype), what
        Ag, Bg = panels(dtype, RP, r, count, garbage=True)
        Ag[5, :] = -3e20      # a row of the query panel nobody asks for
        dirty = na.op_top_k(queries, k, Ag, Bg, count, r, base=base)
        assert bits(dirty) == bits(got), f"{what}: the padding reached the result"


# every count, query count and k met at one instantiation per precision, whatever the cycle above leaves out
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_exact_every_count_query_count_and_k(dtype):
    RP, r = 64, 7
    for count in COUNTS:
        A, B = panels(dtype, RP, r, count)
        for i, nq in enumerate(NQS):
            k = KS[(i + count) % len(KS)]
            queries = query_list(nq, 1, seed=nq)
            assert same(na.op_top_k(queries, k, A, B, count, r, base=1), reference(A, B, count, r, queries, k, None, 1), dtype), (count, nq, k)
    A, B = panels(dtype, RP, r, 129)
    queries = query_list(33, 0, seed=3)
    for k in KS:
        assert same(na.op_top_k(queries, k, A, B, 129, r), reference(A, B, 129, r, queries, k, None, 0), dtype), k
    assert na.library().nmfamd_top_k_max() == na.TOPK_MAX_K == 64


# 3. slabs, a repeated launch, the order of the queries and their company
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_slabs_and_query_order_do_not_change_a_row(dtype):
    RP, r, count, k, nq = 128, 70, 131, 10, 37
    for kind in ("int", "real"):
        A, B = panels(dtype, RP, r, count, kind)
        queries = query_list(nq, 0, seed=8)
        first = na.op_top_k(queries, k, A, B, count, r)
        for slabs in (1, 2, 3, 0, na.top_k_slabs(nq, count)):
            assert bits(na.op_top_k(queries, k, A, B, count, r, slabs=slabs)) == bits(first), f"{kind}: slabs {slabs}"
        if kind == "int":
            assert same(first, reference(A, B, count, r, queries, k, None, 0), dtype)
        else:
            tref.check_top_k(first[0], first[1], A[:, :r], B[:count, :r], queries, k, None, 0, U[dtype])
        back = na.op_top_k(queries[::-1].copy(), k, A, B, count, r, slabs=2)
        assert bits((back[0][::-1].copy(), back[1][::-1].copy())) == bits(first), f"{kind}: the reversed list"
        for q in (0, 1, 17, nq - 1):
            alone = na.op_top_k(queries[q:q + 1], k, A, B, count, r)
            assert bits(alone) == bits((first[0][q:q + 1], first[1][q:q + 1])), f"{kind}: query {q} alone"
    # few queries against many candidates are cut into many slabs, many queries into few; never more slabs than tiles of 32 candidates
    assert na.top_k_slabs(1, 20000) == 256 and na.top_k_slabs(100000, 20000) == 2 and na.top_k_slabs(1 << 20, 20000) == 1 and na.top_k_slabs(5, 33) == 2


# 4. exclusion, exactly (integer panels)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_exclusion(dtype):
    RP, r, count, nq = 64, 9, 100, 35
    A, B = panels(dtype, RP, r, count)
    rng = np.random.default_rng(11)
    for base in (0, 1):
        queries = query_list(nq, base, seed=2)
        lists = [rng.integers(0, count, rng.integers(0, 30)) for _ in range(nq)]
        lists[0] = np.zeros(0, np.int64)                                   # an empty list
        lists[1] = np.array([3, 3, 3, 50, 3, 50, 99, 0])                   # duplicates, both ends
        lists[2] = rng.permutation(count)                                  # everything: the row is all -1 / -inf
        lists[3] = rng.permutation(count)[:count - 4]                      # fewer than k stay
        lists[4] = np.array([47, 48, 49, 50, 51, 52, 63, 64, 31, 32])      # around the slab boundaries of slabs = 2 in both precisions
        lists[34] = np.arange(count - 1, -1, -1)[:60]                      # the last query: a long descending list
        ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
        idx = (np.concatenate(lists) + base).astype(np.int32)
        for k, slabs in ((7, 0), (7, 2), (64, 2), (1, 3)):
            got = na.op_top_k(queries, k, A, B, count, r, exclude=(ptr, idx), base=base, slabs=slabs)
            want = reference(A, B, count, r, queries, k, (ptr, idx), base)
            assert same(got, want, dtype), (base, k, slabs)
            assert np.all(got[0][2] == -1) and np.all(np.isneginf(got[1][2])) and (k < 5 or np.sum(got[0][3] >= 0) == 4)
    # all lists empty: the result without lists
    queries = query_list(nq, 0, seed=2)
    empty = (np.zeros(nq + 1, np.int64), np.zeros(0, np.int32))
    assert bits(na.op_top_k(queries, 5, A, B, count, r, exclude=empty)) == bits(na.op_top_k(queries, 5, A, B, count, r))
    # more than one segment of the bitmap (32 tiles): entries on both sides of its boundary
    count = 32 * 32 + 40
    rngb = np.random.default_rng(3)
    Bb = np.zeros((count + 9, RP), dtype); Bb[:count, :r] = rngb.integers(0, 4, (count, r))
    lists = [rngb.integers(0, count, 400) for _ in range(nq)]
    lists[5] = np.arange(1000, count)
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    idx = np.concatenate(lists).astype(np.int32)
    for slabs in (1, 0):
        got = na.op_top_k(queries, 20, A, Bb, count, r, exclude=(ptr, idx), slabs=slabs)
        assert same(got, reference(A, Bb, count, r, queries, 20, (ptr, idx), 0), dtype), slabs


# 5. real-valued panels
@pytest.mark.parametrize("dtype,RP,r", [(np.float32, 128, 100), (np.float64, 192, 130), (np.float32, 512, 500), (np.float64, 512, 449)])
def test_real_valued_panels(dtype, RP, r):
    count, nq, k = 129, 65, 10
    A, B = panels(dtype, RP, r, count, "real")
    queries = query_list(nq, 1, seed=6)
    lists = [np.random.default_rng(q).integers(0, count, 12) for q in range(nq)]
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    idx = (np.concatenate(lists) + 1).astype(np.int32)
    for excl in (None, (ptr, idx)):
        got = na.op_top_k(queries, k, A, B, count, r, exclude=excl, base=1)
        tref.check_top_k(got[0], got[1], A[:, :r], B[:count, :r], queries, k, excl, 1, U[dtype])
        assert bits(na.op_top_k(queries, k, A, B, count, r, exclude=excl, base=1)) == bits(got), "a repeated launch"


# 6. what the entry refuses
def test_refusals():
    count, r = 100, 8
    A, B = panels(np.float32, 64, r, count)
    q = query_list(17, 0, seed=1)
    ptr = np.arange(18, dtype=np.int64); idx = np.arange(17, dtype=np.int32)
    ok = dict(queries=q, k=5, A=A, B=B, count=count, r=r)
    na.op_top_k(**ok, exclude=(ptr, idx))
    wide = np.zeros((ROWS, 192), np.float32)
    for change in (dict(queries=np.zeros(0, np.int32)),                                   # nq = 0
                   dict(k=0), dict(k=65),
                   dict(r=0), dict(r=65),
                   dict(A=wide, B=wide),                                                  # fp32 has no padded rank 192
                   dict(A=np.zeros((ROWS, 576)), B=np.zeros((ROWS, 576))),                # nor fp64 one of 576
                   dict(queries=q + ROWS), dict(queries=q - 1),                           # a query outside the panel
                   dict(exclude=(ptr, idx + count - 16)), dict(exclude=(ptr, idx - 1)),   # an excluded index outside the candidates
                   dict(exclude=(ptr + 1, np.arange(18, dtype=np.int32))),                # excl_ptr does not start at 0
                   dict(exclude=(np.concatenate([ptr[:9], ptr[7:8], ptr[10:]]), idx)),    # excl_ptr decreases
                   dict(base=2),
                   dict(count=ROWS + 1),                                                  # more candidates than rows of B
                   dict(count=0), dict(slabs=257)):
        with pytest.raises(na.EngineError) as err:
            na.op_top_k(**{**ok, **change})
        assert err.value.status == 1, change
