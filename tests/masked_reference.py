"""fp64 numpy restatement of the missing-value multiplicative update (docs/MISSING.md), over the stored entries p of V.

Omega is a list of stored entries (rows[p], cols[p], vals[p]): duplicates count once per copy, explicit zeros are observed, a row or
column without an entry is allowed.  One iteration:

    H step   H(:, j) .*= (sum_p v_p W(i_p, :)) ./ (sum_p (W(i_p, :) . H(:, j)) W(i_p, :) + eps)     p over the entries of column j
    W step   W(i, :) .*= (sum_p v_p H(:, j_p)) ./ (sum_p (W(i, :) . H(:, j_p)) H(:, j_p) + eps)    p over the entries of row i, new H
    normalise the columns of W (sum of squares > 0 only); H is not rescaled

and the error of an error iteration is that of the pair (W_{k-1}, H_k): sqrt(sum_p (v_p - W_{k-1}(i_p, :) . H_k(:, j_p))^2), rmsd = that / sqrt(|Omega|).
eps is the machine epsilon of the engine's element type.  Everything here is float64.

The dot products run over chunks of entries (``chunk``) and the accumulations are sparse x dense products, so medium problems (a million
entries at r = 128) fit in memory and take seconds.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp


def _dots(rows, cols, W, Ht, chunk):
    """wh_p = W(i_p, :) . H(:, j_p) for every stored entry (Ht = H^T, contiguous)."""
    out = np.empty(len(rows))
    for s in range(0, len(rows), chunk):
        out[s:s + chunk] = np.einsum("pk,pk->p", W[rows[s:s + chunk]], Ht[cols[s:s + chunk]])
    return out


def _accumulate(keys, gather_idx, F, a, b, length):
    """num(key, :) = sum_p a_p F(gather_idx_p, :), den(key, :) = sum_p b_p F(gather_idx_p, :)  (F: rows are factor rows).
    As sparse x dense products: the coordinate form adds the copies of a duplicated (key, gather) pair, which is the sum over p."""
    shape = (length, F.shape[0])
    num = sp.csr_matrix((a, (keys, gather_idx)), shape=shape) @ F
    den = sp.csr_matrix((b, (keys, gather_idx)), shape=shape) @ F
    return np.asarray(num), np.asarray(den)


def normalize_columns(W):
    s = np.sum(W * W, axis=0)
    nz = s > 0
    W[:, nz] = W[:, nz] / np.sqrt(s[nz])
    return W


def iteration(rows, cols, vals, W, H, eps, *, compute_error=False, const_w=False, chunk=1 << 16):
    """One iteration on float64 copies.  Returns (W, H, frobenius or None)."""
    rows = np.asarray(rows, dtype=np.int64); cols = np.asarray(cols, dtype=np.int64); vals = np.asarray(vals, dtype=np.float64)
    m, n = W.shape[0], H.shape[1]
    W = np.array(W, dtype=np.float64); H = np.array(H, dtype=np.float64)
    wh = _dots(rows, cols, W, np.ascontiguousarray(H.T), chunk)
    num, den = _accumulate(cols, rows, W, vals, wh, n)
    H = H * num.T / (den.T + eps)
    frob = None
    if compute_error or not const_w:
        Ht = np.ascontiguousarray(H.T)
        wh = _dots(rows, cols, W, Ht, chunk)         # old W, new H
        if compute_error:
            frob = float(np.sqrt(np.sum((vals - wh) ** 2)))
        if not const_w:
            num, den = _accumulate(rows, cols, Ht, vals, wh, m)
            W = normalize_columns(W * num / (den + eps))
    return W, H, frob


def run(rows, cols, vals, W, H, iterations, eps, *, const_w=False, chunk=1 << 16):
    """`iterations` iterations, the error on the last one.  Returns (W, H, frobenius, rmsd)."""
    frob = None
    for it in range(1, iterations + 1):
        W, H, f = iteration(rows, cols, vals, W, H, eps, compute_error=it == iterations, const_w=const_w, chunk=chunk)
        if f is not None:
            frob = f
    return W, H, frob, frob / np.sqrt(len(vals))


def entries_of_dense(V):
    """The observed entries of a dense V with NaN = missing, in column-major order."""
    Vf = np.asarray(V)
    cols, rows = np.nonzero(~np.isnan(Vf.T))
    return rows, cols, Vf[rows, cols]


def planted_ratings(m, n, density, seed, *, rating_max=5):
    """Integer ratings 1 .. rating_max at a random `density` share of the entries (every entry at density 1): (rows, cols, vals), row-major order."""
    rng = np.random.default_rng(seed)
    mask = np.ones((m, n), dtype=bool) if density >= 1.0 else rng.random((m, n)) < density
    rows, cols = np.nonzero(mask)
    vals = rng.integers(1, rating_max + 1, size=len(rows)).astype(np.float64)
    return rows, cols, vals


def csr_of(rows, cols, vals, m):
    """0-based CSR arrays of entries given in row-major order (stable: duplicates keep their order)."""
    order = np.lexsort((cols, rows))
    rows, cols, vals = np.asarray(rows)[order], np.asarray(cols)[order], np.asarray(vals)[order]
    ptr = np.zeros(m + 1, dtype=np.int32)
    np.add.at(ptr, rows + 1, 1)
    return np.cumsum(ptr).astype(np.int32), cols.astype(np.int32), vals


def csc_of(rows, cols, vals, n):
    """0-based CSC arrays (column pointer, row indices, values)."""
    order = np.lexsort((rows, cols))
    rows, cols, vals = np.asarray(rows)[order], np.asarray(cols)[order], np.asarray(vals)[order]
    ptr = np.zeros(n + 1, dtype=np.int32)
    np.add.at(ptr, cols + 1, 1)
    return np.cumsum(ptr).astype(np.int32), rows.astype(np.int32), vals
