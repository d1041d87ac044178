"""fp64 numpy restatement of top_k (docs/TOPK.md), and the tolerant check of a computed result.

A (a_rows, r) is the query panel, B (count, r) the candidate panel, both cut to the coordinates and the candidates that count; a query names a row of A (index base
`base`), the score of candidate j is s = A[query] . B[j].  The total order: score descending, equal scores by ascending index.  exclude: None or (excl_ptr,
excl_idx), a CSR over the queries of candidates (in `base`) that are not eligible."""
from __future__ import annotations

import numpy as np

from tests.sparse_kl_reference import gamma  # noqa: F401  (gamma(k, u) = k u / (1 - k u), the standard bound's constant)


def eligible_mask(q, count, exclude, base):
    ok = np.ones(count, dtype=bool)
    if exclude is not None:
        ptr, idx = np.asarray(exclude[0], dtype=np.int64), np.asarray(exclude[1], dtype=np.int64)
        ok[idx[ptr[q]:ptr[q + 1]] - base] = False
    return ok


def top_k(A, B, queries, k, exclude=None, base=0):
    """(indices (nq, k) int32 in `base`, scores (nq, k) float64): per query the first k eligible candidates by a stable sort on (-score, index); -1 / -inf where
    fewer than k are eligible."""
    A = np.asarray(A, dtype=np.float64); B = np.asarray(B, dtype=np.float64)
    queries = np.asarray(queries, dtype=np.int64)
    count = B.shape[0]
    idx = np.full((len(queries), k), -1, dtype=np.int32)
    sc = np.full((len(queries), k), -np.inf)
    for q, row in enumerate(queries - base):
        s = B @ A[row] + 0.0      # (-0 -> +0: numeric equality)
        cand = np.nonzero(eligible_mask(q, count, exclude, base))[0]
        order = cand[np.argsort(-s[cand], kind="stable")][:k]      # cand ascends, so equal scores keep ascending index
        idx[q, :len(order)] = order + base
        sc[q, :len(order)] = s[order]
    return idx, sc


def check_top_k(indices, scores, A, B, queries, k, exclude, base, u):
    """Asserts that (indices, scores) is a correct top k up to the rounding of a dot product of r terms in unit roundoff u.  With s the fp64 score of a pair and
    b = gamma(r, u) sum |a b| its bound:
      1. returned indices are distinct, in range, not excluded; the -1 / -inf fill is exactly the shortfall and sits at the end;
      2. |returned score - s| <= b;
      3. the row is sorted by (returned score descending, index ascending);
      4. every eligible candidate that was not returned has s_j - b_j <= s_last + b_last (last: the last returned candidate of a full row)."""
    A = np.asarray(A, dtype=np.float64); B = np.asarray(B, dtype=np.float64)
    queries = np.asarray(queries, dtype=np.int64)
    indices = np.asarray(indices); scores = np.asarray(scores)
    count, r = B.shape
    assert indices.shape == (len(queries), k) and scores.shape == (len(queries), k), "shape of the result"
    g = gamma(r, u)
    for q, row in enumerate(queries - base):
        s = B @ A[row]
        b = g * (np.abs(B) @ np.abs(A[row]))
        ok = eligible_mask(q, count, exclude, base)
        want = min(k, int(ok.sum()))
        got = indices[q].astype(np.int64)
        assert np.all(got[want:] == -1) and np.all(np.isneginf(scores[q, want:])), f"query {q}: the fill is not exactly the shortfall ({k - want} slots)"
        j = got[:want] - base
        assert np.all(j >= 0) and np.all(j < count), f"query {q}: an index out of range (or a fill slot among the first {want})"
        assert len(set(j.tolist())) == want, f"query {q}: an index twice"
        assert np.all(ok[j]), f"query {q}: an excluded candidate came back"
        sq = scores[q, :want].astype(np.float64)
        assert np.all(np.abs(sq - s[j]) <= b[j]), f"query {q}: a score off by more than its bound"
        for t in range(1, want):
            assert sq[t - 1] > sq[t] or (sq[t - 1] == sq[t] and j[t - 1] < j[t]), f"query {q}: slots {t - 1}, {t} out of order"
        if 0 < want == k:
            rest = ok.copy()
            rest[j] = False
            last = j[-1]
            assert np.all(s[rest] - b[rest] <= s[last] + b[last]), f"query {q}: a candidate clearly better than the last returned one was left out"
