"""fp64 numpy restatement of one penalised HALS iteration (docs/HALS.md, "Penalties"): scikit-learn's coordinate descent, which minimises

    1/2 ||V - W H||^2 + l1W ||W||_1 + l1H ||H||_1 + 1/2 l2W ||W||^2 + 1/2 l2H ||H||^2.

Step k of a sweep with the penalties (l1, l2) of the factor being swept, written out coordinate by coordinate:

    d_k = G[k,k] + l2                                    (skipped where d_k <= 0)
    p[k] <- max(0, p[k] - (G[k,:] . p + l2 p[k] - a[k] + l1) / d_k)

G and a stay unpenalised.  One iteration is the H sweep with (l1H, l2H), then the W sweep with (l1W, l2W); the column normalisation of
tests/hals_reference.py runs only when all four penalties are 0 (W D^-1 . D H keeps W H but not the penalty terms), and then the iteration is
hals_reference.iteration bit for bit.  The error of an iteration is ||V - W H|| with the W of the H step and the new H -- not the penalised
objective -- as the engine reports it.
"""
import numpy as np

from tests import hals_reference as ref


def sweep(P, A, G, l1=0.0, l2=0.0, r=None):
    """The penalised Gauss-Seidel sweep on the columns of P (R x ncols, R >= r) in fp64; rows >= r are returned unchanged."""
    P = np.array(P, dtype=np.float64)
    r = P.shape[0] if r is None else r
    G = np.asarray(G, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64)
    for k in range(r):
        d = G[k, k] + l2
        if d <= 0:
            continue
        P[k] = np.maximum(0.0, P[k] - (G[k, :r] @ P[:r] + l2 * P[k] - A[k] + l1) / d)
    return P


def h_step(V, W, H, l1H=0.0, l2H=0.0):
    return sweep(H, W.T @ V, W.T @ W, l1H, l2H)


def w_step(V, W, H, l1W=0.0, l2W=0.0):
    Q = H @ H.T
    return sweep(W.T, (V @ H.T).T, Q.T, l1W, l2W).T


def iteration(V, W, H, l1W=0.0, l1H=0.0, l2W=0.0, l2H=0.0, constant_w=False):
    """(W, H, error) after one iteration, in fp64.  V: a dense array (a sparse V is densified by the caller: the iteration is the same)."""
    V, W, H = (np.asarray(x, dtype=np.float64) for x in (V, W, H))
    H = h_step(V, W, H, l1H, l2H)
    err = float(np.linalg.norm(V - W @ H))
    if not constant_w:
        W = w_step(V, W, H, l1W, l2W)
        if l1W == 0 and l1H == 0 and l2W == 0 and l2H == 0:
            W, H = ref.normalize(W, H)
    return W, H, err


def run(V, W, H, iters, l1W=0.0, l1H=0.0, l2W=0.0, l2H=0.0, constant_w=False):
    """(W, H, [error per iteration])"""
    W, H = np.asarray(W, dtype=np.float64), np.asarray(H, dtype=np.float64)
    errs = []
    for _ in range(iters):
        W, H, e = iteration(V, W, H, l1W, l1H, l2W, l2H, constant_w)
        errs.append(e)
    return W, H, errs


def objective(V, W, H, l1W=0.0, l1H=0.0, l2W=0.0, l2H=0.0):
    """The penalised objective (W, H >= 0: the L1 norms are plain sums)."""
    V, W, H = (np.asarray(x, dtype=np.float64) for x in (V, W, H))
    R = V - W @ H
    return float(0.5 * (R * R).sum() + l1W * np.abs(W).sum() + l1H * np.abs(H).sum() + 0.5 * l2W * (W * W).sum() + 0.5 * l2H * (H * H).sum())


def panel_sweep(P, slabs, G, r, len_valid, l1, l2):
    """The fp64 penalised sweep of the valid block of a case in panel layout (hals_reference's sweep problems): (len_valid, r)."""
    A = np.asarray(slabs, dtype=np.float64).sum(axis=0)
    return sweep(P[:len_valid, :r].T, A[:len_valid, :r].T, G[:r, :r], l1, l2, r).T


def sparse_pattern(m, n, density, rng, empty_rows=(), empty_cols=()):
    """A random pattern as COO triplets sorted by (row, column): values in (0, 1], the given rows and columns empty, and one stored zero (the
    first entry).  Returns (rows, cols, vals, dense V in fp64)."""
    mask = rng.random((m, n)) < density
    mask[list(empty_rows), :] = False
    mask[:, list(empty_cols)] = False
    rows, cols = np.nonzero(mask)
    vals = 1.0 - rng.random(len(rows))
    vals[0] = 0.0
    V = np.zeros((m, n))
    V[rows, cols] = vals
    return rows.astype(np.int32), cols.astype(np.int32), vals, V
