"""The numpy restatement of the weighted dense beta-divergence multiplicative update (docs/DIVERGENCE.md, "Weighted update"), dtype-generic.  It extends
tests/beta_general_reference.py by a matrix of weights Om >= 0: the objective is sum_ij om_ij d_beta(v_ij | P_ij) plus the penalty terms, P = W H + eps, and each
half-step is
    A <- A .* (num ./ (den + eps + l1 + l2 A))^gamma,    num = (Om .* V .* P^(beta - 2)) B,  den = (Om .* P^(beta - 1)) B        (B the other panel)
with gamma, the penalties and the normalisation of the unweighted update of the same beta (none with a penalty; beta = 1 normalises the columns of W without
rescaling H; any other beta uses the compensated form).  At beta = 1 the denominator is Om^T-weighted, not colsum(B).

A weight of 0 means "not there", not "times zero": such an entry is SELECTED out of num, den and every error term, so V may hold anything at it (NaN, inf).
The errors of an iteration refer to (W_{k-1}, H_k): frobenius = sqrt(sum om (v - P)^2), rmsd = frobenius / sqrt(sum om), divergence = sum om d_beta (no
penalty terms)."""
import numpy as np

from tests import beta_general_reference as gen
from tests import beta_reference as ref

planted, start, gamma_of, penalty_terms, NO_PENALTIES = gen.planted, gen.start, gen.gamma_of, gen.penalty_terms, gen.NO_PENALTIES


def weights(rows, cols, seed, zero_row=None, zero_col=None, zeros=0.3, dtype=np.float64):
    """Uniform in (0, 2] with a share `zeros` of exact zeros, and optionally one all-zero row and one all-zero column."""
    rng = np.random.default_rng(seed)
    Om = 2.0 * (1.0 - rng.random((rows, cols)))
    Om[rng.random((rows, cols)) < zeros] = 0.0
    if zero_row is not None:
        Om[zero_row, :] = 0.0
    if zero_col is not None:
        Om[:, zero_col] = 0.0
    return np.asfortranarray(Om.astype(dtype))


def entries(X, Om, P, beta):
    """The mapped entries (Om .* X .* P^(beta - 2), Om .* P^(beta - 1)), zero -- by selection -- where Om = 0."""
    dt = P.dtype.type
    obs = Om > 0
    Xs = np.where(obs, X, dt(1))      # (what lies under a zero weight never enters the arithmetic)
    if beta == 1:
        q, r = Xs / P, np.ones_like(P)
    elif beta == 0:
        ip = 1.0 / P
        q, r = Xs * ip * ip, ip
    else:
        t = P ** dt(beta - 2.0)
        q, r = Xs * t, t * P
    return np.where(obs, Om * q, dt(0)), np.where(obs, Om * r, dt(0))


def num_den(X, Om, A, B, beta, eps):
    Q, R = entries(X, Om, A @ B.T + eps, beta)
    return Q @ B, R @ B


def half_step(X, Om, A, B, beta, eps, l1=0.0, l2=0.0):
    """The update of the panel A (out x r) against B (red x r) with X, Om (out x red) = V and its weights seen from A's side."""
    dt = A.dtype.type
    num, den = num_den(X, Om, A, B, beta, eps)
    quo = num / (den + eps + dt(l1) + dt(l2) * A)
    g = gamma_of(beta)
    return A * (quo if g == 1.0 else np.sqrt(quo) if g == 0.5 else quo ** dt(g))      # (a zero quotient stays 0)


def terms(X, Om, A, B, beta, eps):
    """Per row of A: sum om (x - p)^2 and sum om d_beta(x | p), with p = A B^T + eps, over the entries with om > 0."""
    dt = A.dtype.type
    P = A @ B.T + eps
    obs = Om > 0
    Xs = np.where(obs, X, dt(1))
    tf = np.where(obs, Om * (Xs - P) ** 2, dt(0)).sum(axis=1)
    pos = Xs > 0
    Xp = np.where(pos, Xs, dt(1))
    if beta == 1:
        d = np.where(pos, Xs * np.log(Xp / P), dt(0)) - Xs + P
    elif beta == 0:
        ratio = Xs / P
        d = ratio - np.log(ratio) - 1.0
    else:
        xb = np.where(pos, Xp ** dt(beta), dt(0))
        pm1 = P ** dt(beta - 1.0)
        d = (xb + dt(beta - 1.0) * pm1 * P - dt(beta) * Xs * pm1) / dt(beta * (beta - 1.0))
    return tf, np.where(obs, Om * d, dt(0)).sum(axis=1)


def divergence(V, Om, W, H, beta, eps):
    return float(terms(V, Om, W, H.T, beta, eps)[1].astype(np.float64).sum())


def run(V, Om, W0, H0, iters, beta, eps, pen=NO_PENALTIES, const_w=False, dtype=np.float64, history=False):
    """`iters` iterations from (W0, H0) with weights Om and penalties pen = (l1W, l1H, l2W, l2H).  Returns (W, H, frobenius, rmsd, divergence) of the last
    iteration, and with history=True the objective (weighted divergence + penalty terms, at (W_{k-1}, H_k)) of every iteration as a sixth entry."""
    l1W, l1H, l2W, l2H = pen
    penalised = any(p != 0 for p in pen)
    Om = np.asarray(Om, dtype=dtype)
    V = np.asarray(V, dtype=dtype)
    W = np.array(W0, dtype=dtype); H = np.array(H0, dtype=dtype)
    eps = dtype(eps)
    sum_w = float(Om.astype(np.float64).sum())
    frob = rmsd = div = 0.0
    hist = []
    for it in range(1, iters + 1):
        H = half_step(V.T, Om.T, H.T, W, beta, eps, l1H, l2H).T
        if history or it == iters:
            tf, td = terms(V, Om, W, H.T, beta, eps)
            frob = float(np.sqrt(tf.astype(np.float64).sum())); rmsd = frob / np.sqrt(sum_w); div = float(td.astype(np.float64).sum())
            hist.append(div + penalty_terms(W, H, pen))
        if not const_w:
            W = half_step(V, Om, W, H.T, beta, eps, l1W, l2W)
            if not penalised:
                W, H = ref.normalize(W, H, beta != 1)
    out = (np.asfortranarray(W), np.asfortranarray(H), frob, rmsd, div)
    return out + (hist,) if history else out
