"""The host side of top_k (docs/TOPK.md) without a GPU: the fp64 reference on a hand-made case with ties, the tolerant checker -- which must raise on a row with a
clearly worse candidate swapped in, an excluded candidate, an unsorted row, a wrong fill count, a score off its bound and an index twice --, and
exclusion_lists."""
import numpy as np
import pytest

import nmfgpu_amd as na
from tests import topk_reference as tref

U32 = 2.0 ** -24


def hand_made():
    """3 queries x 5 candidates, r = 2; scores (query x candidate):
         q0: 2 4 4 0 2      q1: 1 1 1 1 1      q2: 2 3 3 1 2"""
    A = np.array([[2.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    B = np.array([[1.0, 1.0], [2.0, 1.0], [2.0, 1.0], [0.0, 1.0], [1.0, 1.0]])
    return A, B


def test_reference_on_a_hand_made_case_with_ties():
    A, B = hand_made()
    s = A @ B.T
    assert s.tolist() == [[2, 4, 4, 0, 2], [1, 1, 1, 1, 1], [2, 3, 3, 1, 2]]
    idx, sc = tref.top_k(A, B, [0, 1, 2], 3)
    assert idx.tolist() == [[1, 2, 0], [0, 1, 2], [1, 2, 0]]      # equal scores by ascending index
    assert sc.tolist() == [[4, 4, 2], [1, 1, 1], [3, 3, 2]]
    # base 1, a duplicate query, unsorted queries
    idx, sc = tref.top_k(A, B, [3, 1, 3], 2, base=1)
    assert idx.tolist() == [[2, 3], [2, 3], [2, 3]] and sc.tolist() == [[3, 3], [4, 4], [3, 3]]
    # k above the count: the shortfall is filled
    idx, sc = tref.top_k(A, B, [1], 7)
    assert idx.tolist() == [[0, 1, 2, 3, 4, -1, -1]] and np.all(np.isneginf(sc[0, 5:])) and sc[0, :5].tolist() == [1] * 5
    # exclusion: unsorted, with a duplicate; one query loses everything
    excl = (np.array([0, 3, 8, 8]), np.array([2, 1, 2, 4, 3, 2, 1, 0]))
    idx, sc = tref.top_k(A, B, [0, 1, 2], 3, exclude=excl)
    assert idx.tolist() == [[0, 4, 3], [-1, -1, -1], [1, 2, 0]]
    assert sc[0].tolist() == [2, 2, 0] and np.all(np.isneginf(sc[1]))
    # -0 and +0 are one score: the index decides
    idx, _ = tref.top_k(np.array([[1.0]]), np.array([[0.0], [-0.0], [0.0]]), [0], 3)
    assert idx.tolist() == [[0, 1, 2]]


def real_case():
    rng = np.random.default_rng(5)
    A = 1.0 - rng.random((6, 9)); B = 1.0 - rng.random((40, 9))
    queries = np.array([5, 0, 3, 3])
    ptr = np.array([0, 2, 2, 5, 45])
    idx = np.concatenate([[7, 7], [1, 39, 0], np.arange(40)])      # query 3 excludes everything
    return A, B, queries, (ptr, idx)


def test_checker_accepts_the_reference_and_a_result_within_rounding():
    A, B, queries, excl = real_case()
    for k in (1, 5, 40, 41):
        for e in (None, excl):
            idx, sc = tref.top_k(A, B, queries, k, exclude=e)
            tref.check_top_k(idx, sc, A, B, queries, k, e, 0, U32)
            tref.check_top_k(idx, sc.astype(np.float32), A, B, queries, k, e, 0, U32)
            idx1, sc1 = tref.top_k(A, B, queries + 1, k, exclude=None if e is None else (e[0], e[1] + 1), base=1)
            assert np.array_equal(np.where(idx >= 0, idx + 1, -1), idx1) and np.array_equal(sc, sc1)
            tref.check_top_k(idx1, sc1, A, B, queries + 1, k, None if e is None else (e[0], e[1] + 1), 1, U32)


def test_checker_is_not_vacuous():
    A, B, queries, excl = real_case()
    k = 5
    idx, sc = tref.top_k(A, B, queries, k, exclude=excl)
    full = A[queries] @ B.T

    def bad(i, s, match):
        with pytest.raises(AssertionError, match=match):
            tref.check_top_k(i, s, A, B, queries, k, excl, 0, U32)

    tref.check_top_k(idx, sc, A, B, queries, k, excl, 0, U32)
    # a clearly worse candidate swapped in for the last slot (its own score, so that everything else holds)
    worst = int(np.argmin(full[1]))
    i, s = idx.copy(), sc.copy(); i[1, -1] = worst; s[1, -1] = full[1, worst]
    bad(i, s, "clearly better")
    # an excluded candidate in the last slot of query 0 (candidate 7 is on its list)
    i, s = idx.copy(), sc.copy(); i[0, -1] = 7; s[0, -1] = min(full[0, 7], s[0, -2])
    bad(i, s, "excluded")
    # an unsorted row
    i, s = idx.copy(), sc.copy(); i[1, [0, 1]] = i[1, [1, 0]]; s[1, [0, 1]] = s[1, [1, 0]]
    bad(i, s, "out of order")
    # a wrong fill count: query 3 has nothing eligible, query 1 everything
    i, s = idx.copy(), sc.copy(); i[3, 0] = 2; s[3, 0] = full[3, 2]
    bad(i, s, "shortfall")
    i, s = idx.copy(), sc.copy(); i[1, -1] = -1; s[1, -1] = -np.inf
    bad(i, s, "out of range")
    # a score off by more than its bound; an index twice; an index past the count
    i, s = idx.copy(), sc.copy(); s[1, 0] *= 1.0 + 1e-4
    bad(i, s, "bound")
    i, s = idx.copy(), sc.copy(); i[1, 1] = i[1, 0]; s[1, 1] = s[1, 0]
    bad(i, s, "twice")
    i, s = idx.copy(), sc.copy(); i[1, 0] = 40
    bad(i, s, "out of range")


def test_exclusion_lists():
    rows = np.array([2, 0, 2, 1, 2, 0])
    cols = np.array([4, 1, 0, 3, 4, 2])
    ptr, idx = na.exclusion_lists([2, 1, 3, 2, 0], rows, cols)
    assert ptr.dtype == np.int64 and idx.dtype == np.int32
    assert ptr.tolist() == [0, 3, 4, 4, 7, 9]
    assert idx.tolist() == [4, 0, 4, 3, 4, 0, 4, 1, 2]      # the order of the coordinate list, duplicates kept, a query twice gets its list twice
    # axis 1: a query is a column, its list the rows
    ptr, idx = na.exclusion_lists([4, 9], rows, cols, axis=1)
    assert ptr.tolist() == [0, 2, 2] and idx.tolist() == [2, 2]
    # base 1 in, base 1 out
    ptr, idx = na.exclusion_lists([3], rows + 1, cols + 1, base=1)
    assert ptr.tolist() == [0, 3] and idx.tolist() == [5, 1, 5]
    # nothing to exclude
    ptr, idx = na.exclusion_lists([0, 1], np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert ptr.tolist() == [0, 0, 0] and idx.shape == (0,)
    with pytest.raises(ValueError):
        na.exclusion_lists([0], rows, cols[:-1])
    with pytest.raises(ValueError):
        na.exclusion_lists([0], rows, cols, axis=2)
    # the reference takes what it builds: no training entry comes back
    A, B = 1.0 - np.random.default_rng(1).random((3, 4)), 1.0 - np.random.default_rng(2).random((5, 4))
    q = np.array([0, 1, 2])
    excl = na.exclusion_lists(q, rows, cols)
    got, _ = tref.top_k(A, B, q, 5, exclude=excl)
    seen = set(zip(rows.tolist(), cols.tolist()))
    assert all((int(q[a]), int(j)) not in seen for a in range(3) for j in got[a] if j >= 0)
    assert (got >= 0).sum(axis=1).tolist() == [3, 4, 3]


def test_exported_names():
    assert na.TOPK_MAX_K == 64 and callable(na.op_top_k) and callable(na.top_k_slabs) and hasattr(na.Engine, "top_k")
