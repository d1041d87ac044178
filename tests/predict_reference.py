"""fp64 numpy restatement of predict and score (docs/PREDICT.md): the value of W H at a coordinate list and the error over it.

The list is (rows[p], cols[p]) of index base `base`, unsorted, duplicates counted once per copy.  predict gathers one row of W and one column of H per entry;
score adds, over the entries, (v - p)^2, d_beta(v | p + eps) and the absolute values of the summands of d_beta -- the per-entry forms are those of the masked
engines (tests/masked_beta_reference.entry_terms: KL at beta = 1, Itakura-Saito at beta = 0, the general form elsewhere, v^beta = 0 at v = 0)."""
from __future__ import annotations

import numpy as np

from tests import masked_beta_reference as mbref
from tests.sparse_kl_reference import gamma  # noqa: F401  (gamma(k, u) = k u / (1 - k u), the standard bound's constant)


def predict(rows, cols, W, H, base=0, chunk=1 << 13):
    """out[p] = sum_k W[rows[p] - base, k] H[k, cols[p] - base], and beside it sum_k |W H| (the scale of a computed dot product's rounding), both in fp64."""
    W = np.asarray(W, dtype=np.float64); Ht = np.ascontiguousarray(np.asarray(H, dtype=np.float64).T)
    i = np.asarray(rows, dtype=np.int64) - base; j = np.asarray(cols, dtype=np.int64) - base
    assert i.min() >= 0 and i.max() < W.shape[0] and j.min() >= 0 and j.max() < Ht.shape[0]
    out = np.empty(len(i)); mag = np.empty(len(i))
    for s in range(0, len(i), chunk):
        prod = W[i[s:s + chunk]] * Ht[j[s:s + chunk]]
        out[s:s + chunk] = prod.sum(axis=1)
        mag[s:s + chunk] = np.abs(prod).sum(axis=1)
    return out, mag


def entry_terms(vals, pred, beta, eps):
    """Per entry: (v - pred)^2 and, with a beta, d_beta(v | pred + eps) and the sum of the absolute values of its summands (beta None: NaN)."""
    vals = np.asarray(vals, dtype=np.float64); pred = np.asarray(pred, dtype=np.float64)
    sq = (vals - pred) ** 2
    if beta is None:
        return sq, np.full(len(sq), np.nan), np.full(len(sq), np.nan)
    _, td, ta = mbref.entry_terms(vals, pred + eps, beta)
    return sq, td, ta


def score_of_predictions(vals, pred, beta, eps):
    """The five results of score from given predictions."""
    sq, td, ta = entry_terms(vals, pred, beta, eps)
    n = len(sq)
    return {"sq": float(sq.sum()), "rmsd": float(np.sqrt(sq.sum() / n)), "div": float(td.sum()), "abs_div": float(ta.sum()), "count": n}


def score(rows, cols, vals, W, H, beta, eps, base=0):
    return score_of_predictions(vals, predict(rows, cols, W, H, base)[0], beta, eps)


def value_rule_holds(vals, beta):
    """beta <= 0: every value finite and > 0; beta > 0: finite and >= 0; beta None: finite."""
    vals = np.asarray(vals, dtype=np.float64)
    if not np.all(np.isfinite(vals)):
        return False
    return True if beta is None else bool(np.all(vals > 0)) if beta <= 0 else bool(np.all(vals >= 0))
