"""fp64 numpy restatement of one HALS iteration (docs/HALS.md), the yardstick of tests/test_hals_cpu.py and tests/test_gpu_hals.py.

One iteration, H then W:
  H step: G = W^T W, A = W^T V; for k = 0 .. r-1 (skipping G[k,k] <= 0), every column at once:
          H[k,:] <- max(0, H[k,:] - (G[k,:] H - A[k,:]) / G[k,k])       (rows l < k already updated: Gauss-Seidel)
  W step: Q = H H^T, B = V H^T;  W[:,k] <- max(0, W[:,k] - (W Q[:,k] - B[:,k]) / Q[k,k])
  normalisation: d = ||W[:,k]||; where d > 0, W[:,k] /= d and H[k,:] *= d (W H unchanged)
The error of the iteration is ||V - W H|| with the W of the H step and the new H (before the normalisation), as the engine reports it.

Both steps are one sweep (`sweep`) over the columns of a panel: H's columns against W^T W, W^T's columns against H H^T.  `sweep_bound`
bounds, element by element, how far a floating-point sweep in any summation order may land from the exact one.
"""
import numpy as np


def sweep(P, A, G, r=None):
    """The Gauss-Seidel sweep of kernels_hals.hip on the columns of P (R x ncols, R >= r) in fp64: for k = 0 .. r-1, skipping G[k,k] <= 0,
    P[k,:] <- max(0, P[k,:] - (G[k,:r] P[:r] - A[k,:]) / G[k,k]), rows l < k already updated.  Rows >= r are returned unchanged."""
    P = np.array(P, dtype=np.float64)
    r = P.shape[0] if r is None else r
    G = np.asarray(G, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64)
    for k in range(r):
        if G[k, k] <= 0:
            continue
        P[k] = np.maximum(0.0, P[k] - (G[k, :r] @ P[:r] - A[k]) / G[k, k])
    return P


def gamma(n, u):
    return n * u / (1.0 - n * u)


def sweep_bound(P, A_slabs, G, r, u):
    """Per-element bound on |computed - exact| for a sweep of P (RP x ncols) against the S slabs A_slabs (S x RP x ncols, summed in any order)
    and G (RP x RP), every dot product and slab sum in any order with unit roundoff u.  Step k has the local error
        delta_k = 2 gamma_{RP+S+4} (sum_l |G_kl h_l| + sum_s |slab_s(k)|) / G_kk + 2 u |h_k|
    (h: the exact state at step k, h_k its new value; the factor 2 covers the first-order terms of the inexact state), and in exact arithmetic the
    new h_k depends on the h_l, l < k, with the weights G_kl / G_kk (not on its old value), so errors propagate as
        b_k = delta_k + sum_{l<k} |G_kl| / G_kk b_l.
    The clamp is 1-Lipschitz and adds nothing.  A skipped coordinate keeps its input: b_k = 0.  Useful only where G is diagonally dominant
    (sum_{l != k} |G_kl| <= G_kk / 2, where b stays near 2 max delta); on a Gram-like G it becomes vacuous.  Returns b, r x ncols."""
    S = np.asarray(A_slabs, dtype=np.float64)
    G = np.asarray(G, dtype=np.float64)
    RP = G.shape[0]
    g = gamma(RP + S.shape[0] + 4, u)
    h = np.array(P[:r], dtype=np.float64)
    A = S.sum(axis=0)[:r]
    slab_abs = np.abs(S).sum(axis=0)[:r]
    Gr = G[:r, :r]
    b = np.zeros_like(h)
    for k in range(r):
        d = Gr[k, k]
        if d <= 0:
            continue
        mag = np.abs(Gr[k]) @ np.abs(h)
        h[k] = np.maximum(0.0, h[k] - (Gr[k] @ h - A[k]) / d)
        b[k] = 2.0 * g * (mag + slab_abs[k]) / d + 2.0 * u * np.abs(h[k]) + (np.abs(Gr[k, :k]) / d) @ b[:k]
    return b


def h_step(V, W, H):
    return sweep(H, W.T @ V, W.T @ W)


def w_step(V, W, H):
    Q = H @ H.T
    return sweep(W.T, (V @ H.T).T, Q.T).T          # (row k of Q^T: the column W Q[:, k] is formed from)


def normalize(W, H):
    W, H = W.copy(), H.copy()
    d = np.sqrt((W * W).sum(axis=0))
    for k in range(W.shape[1]):
        if d[k] > 0:
            W[:, k] /= d[k]
            H[k, :] *= d[k]
    return W, H


def iteration(V, W, H, constant_w=False):
    """(W, H, error) after one iteration, in fp64."""
    V, W, H = (np.asarray(x, dtype=np.float64) for x in (V, W, H))
    H = h_step(V, W, H)
    err = float(np.linalg.norm(V - W @ H))
    if not constant_w:
        W = w_step(V, W, H)
        W, H = normalize(W, H)
    return W, H, err


def iteration_in(V, W, H, dtype, reverse=False):
    """(W, H) after one iteration with every product, sweep and norm in numpy `dtype`, the dot products of the sweeps over reversed
    coordinates when `reverse`.  Not a yardstick: a measure of how far plain rounding moves a step on a given problem (where the
    Gauss-Seidel steps cancel, e.g. when m or n is below r, later steps divide rounding noise by tiny diagonal entries)."""
    f = np.dtype(dtype).type
    V, W, H = (np.asarray(x, dtype=f) for x in (V, W, H))
    o = slice(None, None, -1) if reverse else slice(None)

    def sweep_in(P, A, G):
        P = P.copy()
        for k in range(P.shape[0]):
            if G[k, k] <= 0:
                continue
            P[k] = np.maximum(f(0), P[k] - (G[k, o] @ P[o] - A[k]) / G[k, k])
        return P

    H = sweep_in(H, W.T @ V, W.T @ W)
    Q = H @ H.T
    W = sweep_in(W.T.copy(), (V @ H.T).T, Q.T).T
    d = np.sqrt((W * W).sum(axis=0))
    live = d > 0
    W[:, live] /= d[live]
    H[live] *= d[live][:, None]
    return W, H


def run(V, W, H, iters, constant_w=False):
    """(W, H, [error per iteration])"""
    W, H = np.asarray(W, dtype=np.float64), np.asarray(H, dtype=np.float64)
    errs = []
    for _ in range(iters):
        W, H, e = iteration(V, W, H, constant_w)
        errs.append(e)
    return W, H, errs


# ------------------------------------------------------------------ sweep problems in panel layout (tests/test_gpu_hals_sweep.py)
# P (len_pad, RP): column y of the panel is P[y]; slabs (S, len_pad, RP); G (RP, RP).  Coordinates k >= r and columns y >= len_valid are zero
# (the engine's padding) unless `with_garbage` fills them.

def layout_case(RP, r, len_pad, len_valid, S, rng, dtype):
    """G diagonal, G_kk = 2^((k mod 7) - 3); a(k, y) distinct signed integers, |a| <= 2^16, split exactly over the S slabs; old h small
    integers.  Every operation of the sweep is exact in fp32: the result is max(0, a / G_kk) bit for bit."""
    G = np.zeros((RP, RP))
    k = np.arange(r)
    G[k, k] = 2.0 ** ((k % 7) - 3)
    A = np.zeros((len_pad, RP))
    A[:len_valid, :r] = rng.permutation(np.arange(-2 ** 16, 2 ** 16 + 1))[:len_valid * r].reshape(len_valid, r)
    P = np.zeros((len_pad, RP))
    P[:len_valid, :r] = rng.integers(0, 8, size=(len_valid, r))
    return P.astype(dtype), _split(A, S, rng, 2 ** 10).astype(dtype), G.astype(dtype)


def order_case(RP, r, len_pad, len_valid, S, rng, dtype):
    """G symmetric tridiagonal with unit diagonal, off-diagonals 0 / 1 at random and a few diagonal entries 0 (skipped coordinates); a and old h
    integers in [0, 64].  The sweep is all-integer and exact, and its Gauss-Seidel order shows: h_k depends on the new h_{k-1}."""
    G = np.zeros((RP, RP))
    k = np.arange(r)
    G[k, k] = 1.0
    off = rng.integers(0, 2, size=max(r - 1, 0)).astype(np.float64)
    G[k[:-1], k[:-1] + 1] = off
    G[k[:-1] + 1, k[:-1]] = off
    skip = rng.choice(r, size=min(r, r // 24 + 1), replace=False) if r > 1 else np.zeros(0, int)
    G[skip, skip] = 0.0
    A = np.zeros((len_pad, RP))
    A[:len_valid, :r] = rng.integers(0, 65, size=(len_valid, r))
    P = np.zeros((len_pad, RP))
    P[:len_valid, :r] = rng.integers(0, 65, size=(len_valid, r))
    return P.astype(dtype), _split(A, S, rng, 8).astype(dtype), G.astype(dtype)


def dominant_case(RP, r, len_pad, len_valid, S, rng, dtype):
    """A random symmetric G with diagonal in [1, 2] and sum_{l != k} |G_kl| <= 1/2 (diagonally dominant, where sweep_bound is tight), signed a in
    [-1, 2) split over the slabs at random, old h in [0, 2)."""
    M = rng.uniform(-1.0, 1.0, size=(r, r))
    M = np.triu(M, 1)
    M = M + M.T
    rows = np.abs(M).sum(axis=1).max()
    G = np.zeros((RP, RP))
    G[:r, :r] = M * (0.5 / rows if rows > 0 else 0.0)
    G[np.arange(r), np.arange(r)] = rng.uniform(1.0, 2.0, size=r)
    A = np.zeros((len_pad, RP))
    A[:len_valid, :r] = rng.uniform(-1.0, 2.0, size=(len_valid, r))
    P = np.zeros((len_pad, RP))
    P[:len_valid, :r] = rng.uniform(0.0, 2.0, size=(len_valid, r))
    slabs = np.zeros((S, len_pad, RP))
    for s in range(S - 1):
        slabs[s + 1] = rng.uniform(-0.5, 0.5, size=(len_pad, RP)) * (A != 0)
    slabs[0] = A - slabs[1:].sum(axis=0)
    return P.astype(dtype), slabs.astype(dtype), G.astype(dtype)


def _split(A, S, rng, spread):
    """S integer slabs that sum to the integer matrix A exactly (in any order: every partial sum is a small integer)."""
    slabs = np.zeros((S,) + A.shape)
    for s in range(1, S):
        slabs[s] = rng.integers(-spread, spread + 1, size=A.shape) * (A != 0)
    slabs[0] = A - slabs[1:].sum(axis=0)
    return slabs


def with_garbage(P, slabs, G, r, len_valid, rng):
    """Copies with finite garbage in every padding entry: G rows and columns >= r, P and the slabs at coordinates >= r and columns >= len_valid."""
    P, slabs, G = P.copy(), slabs.copy(), G.copy()
    junk = lambda shape: rng.uniform(-100.0, 100.0, size=shape).astype(P.dtype)
    G[r:, :] = junk(G[r:, :].shape)
    G[:, r:] = junk(G[:, r:].shape)
    for X in (P, *slabs):
        X[:, r:] = junk(X[:, r:].shape)
        X[len_valid:, :] = junk(X[len_valid:, :].shape)
    return P, slabs, G


def panel_sweep(P, slabs, G, r, len_valid):
    """The fp64 sweep of the valid block of a case, in panel layout (len_valid, r)."""
    A = np.asarray(slabs, dtype=np.float64).sum(axis=0)
    return sweep(P[:len_valid, :r].T, A[:len_valid, :r].T, G[:r, :r], r).T


def sweep_f32(P, slabs, G, r, len_valid, order="sequential", variant=None):
    """The sweep of a case in float32 numpy with a fixed summation order (`sequential`: l = 0 .. r-1 and slabs 0 .. S-1; `reversed`), or, with
    `variant`, a deliberately wrong sweep (fp64): "jacobi" (every step reads the old h), "drop_last_slab", "next_row" (row k+1 of G at step k).
    Returns (len_valid, r)."""
    if variant is not None:
        S = np.asarray(slabs, dtype=np.float64)[:, :len_valid, :r]
        if variant == "drop_last_slab":
            S = S[:-1]
        A = S.sum(axis=0).T
        G64 = np.asarray(G, dtype=np.float64)[:r, :r]
        h0 = np.asarray(P, dtype=np.float64)[:len_valid, :r].T.copy()
        h = h0.copy()
        for k in range(r):
            if G64[k, k] <= 0:
                continue
            row = G64[(k + 1) % r] if variant == "next_row" else G64[k]
            src = h0 if variant == "jacobi" else h
            h[k] = np.maximum(0.0, h[k] - (row @ src - A[k]) / G64[k, k])
        return h.T
    f = np.float32
    S = np.asarray(slabs, dtype=f)[:, :len_valid, :r]
    if order == "reversed":
        S = S[::-1]
    A = np.add.accumulate(S, axis=0)[-1].T
    Gf = np.asarray(G, dtype=f)[:r, :r]
    h = np.asarray(P, dtype=f)[:len_valid, :r].T.copy()
    for k in range(r):
        d = Gf[k, k]
        if d <= 0:
            continue
        terms = Gf[k][:, None] * h
        if order == "reversed":
            terms = terms[::-1]
        dot = np.add.accumulate(terms, axis=0)[-1]
        h[k] = np.maximum(f(0), h[k] - (dot - A[k]) * (f(1) / d))
    return h.T
