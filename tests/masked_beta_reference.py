"""fp64 numpy restatement of missing-value NMF under the beta-divergence (docs/MISSING.md, "Beta-divergence"), over the stored entries p of V.

Omega is a list of stored entries (rows[p], cols[p], vals[p]) as in tests/masked_reference.py: duplicates count once per copy, a row or column without an entry
is allowed.  On an Omega without duplicates an iteration is the one of tests/weighted_reference.py (`run`) with 0 / 1 weights.  With
p = A(row, :) . B(idx_p, :) + eps a half-step is

    num = sum_p v_p p^(beta - 2) B(idx_p, :),   den = sum_p p^(beta - 1) B(idx_p, :),   A(row, :) <- A(row, :) .* (num ./ (den + eps + l1 + l2 A(row, :)))^gamma

(H step over the entries of a column with (l1H, l2H), W step over the entries of a row with the new H and (l1W, l2W)); gamma, the penalties and the normalisation
are the weighted update's: none with a penalty, beta = 1 the columns of W without rescaling H, any other beta the compensated form.  The errors of an iteration
refer to (W_{k-1}, H_k): frobenius = sqrt(sum_p (v_p - p)^2), rmsd = frobenius / sqrt(|Omega|), divergence = sum_p d_beta(v_p | p) without penalty terms.

The dot products run over chunks of entries and the accumulations are sparse x dense products (masked_reference's helpers)."""
from __future__ import annotations

import numpy as np

from tests import beta_reference as ref
from tests import masked_reference as mref
from tests import weighted_reference as wref

gamma_of, penalty_terms, NO_PENALTIES = wref.gamma_of, wref.penalty_terms, wref.NO_PENALTIES


def entry_map(v, p, beta):
    """(q, r) = (v p^(beta - 2), p^(beta - 1)) per stored entry, in the three forms of the kernels."""
    if beta == 1:
        return v / p, np.ones_like(p)
    if beta == 0:
        ip = 1.0 / p
        return v * ip * ip, ip
    t = p ** (beta - 2.0)
    return v * t, t * p


def half_step(keys, gather, vals, A, B, beta, eps, l1=0.0, l2=0.0, chunk=1 << 16):
    """The update of the panel A (out x r) against B (red x r): entry p belongs to row keys[p] of A and gathers row gather[p] of B."""
    p = mref._dots(keys, gather, A, B, chunk) + eps
    q, r = entry_map(vals, p, beta)
    num, den = mref._accumulate(keys, gather, B, q, r, A.shape[0])
    quo = num / (den + eps + l1 + l2 * A)
    g = gamma_of(beta)
    return A * (quo if g == 1.0 else np.sqrt(quo) if g == 0.5 else quo ** g)      # (a zero quotient stays 0)


def entry_terms(vals, p, beta):
    """Per stored entry: (v - p)^2, d_beta(v | p) with v^beta = 0 at v = 0, and the sum of the absolute values of the three summands of d_beta."""
    tf = (vals - p) ** 2
    pos = vals > 0
    vp = np.where(pos, vals, 1.0)
    if beta == 1:
        pieces = (np.where(pos, vals * np.log(vp / p), 0.0), -vals, p)
    elif beta == 0:
        ratio = vals / p
        pieces = (ratio, -np.log(ratio), -np.ones_like(p))
    else:
        c = beta * (beta - 1.0)
        pm1 = p ** (beta - 1.0)
        pieces = (np.where(pos, vp ** beta, 0.0) / c, (beta - 1.0) * pm1 * p / c, -beta * vals * pm1 / c)
    return tf, pieces[0] + pieces[1] + pieces[2], np.abs(pieces[0]) + np.abs(pieces[1]) + np.abs(pieces[2])


def terms(keys, gather, vals, A, B, beta, eps, chunk=1 << 16):
    """Per row of A: sum (v - p)^2, sum d_beta(v | p) and sum of the absolute summands, over the row's stored entries."""
    p = mref._dots(keys, gather, A, B, chunk) + eps
    tf, td, ta = entry_terms(vals, p, beta)
    n = A.shape[0]
    return np.bincount(keys, tf, n), np.bincount(keys, td, n), np.bincount(keys, ta, n)


def run(rows, cols, vals, W0, H0, iters, beta, eps, pen=NO_PENALTIES, const_w=False, history=False, chunk=1 << 16):
    """`iters` iterations from (W0, H0) with penalties pen = (l1W, l1H, l2W, l2H).  Returns (W, H, frobenius, rmsd, divergence, S) of the last iteration -- S the sum
    over the stored entries of the absolute values of the three summands of d_beta, the scale of the divergence's rounding -- and with history=True the objective
    (divergence + penalty terms, at (W_{k-1}, H_k)) of every iteration as a seventh entry."""
    l1W, l1H, l2W, l2H = pen
    penalised = any(p != 0 for p in pen)
    rows = np.asarray(rows, dtype=np.int64); cols = np.asarray(cols, dtype=np.int64); vals = np.asarray(vals, dtype=np.float64)
    W = np.array(W0, dtype=np.float64); H = np.array(H0, dtype=np.float64)
    frob = rmsd = div = scale = 0.0
    hist = []
    for it in range(1, iters + 1):
        Ht = half_step(cols, rows, vals, np.ascontiguousarray(H.T), W, beta, eps, l1H, l2H, chunk)
        H = Ht.T
        if history or it == iters:
            tf, td, ta = terms(rows, cols, vals, W, Ht, beta, eps, chunk)
            frob = float(np.sqrt(tf.sum())); rmsd = frob / np.sqrt(len(vals)); div = float(td.sum()); scale = float(ta.sum())
            hist.append(div + penalty_terms(W, H, pen))
        if not const_w:
            W = half_step(rows, cols, vals, W, Ht, beta, eps, l1W, l2W, chunk)
            if not penalised:
                W, H = ref.normalize(W, H, beta != 1)
    out = (np.asfortranarray(W), np.asfortranarray(H), frob, rmsd, div, scale)
    return out + (hist,) if history else out


def divergence(rows, cols, vals, W, H, beta, eps):
    """sum_p d_beta(v_p | (W H)_p + eps) over the stored entries."""
    W = np.asarray(W, dtype=np.float64)
    return float(terms(np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64), np.asarray(vals, dtype=np.float64), W,
                       np.ascontiguousarray(np.asarray(H, dtype=np.float64).T), beta, eps)[1].sum())
