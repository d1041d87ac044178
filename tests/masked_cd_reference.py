"""fp64 numpy restatement of missing-value coordinate descent (docs/MISSING.md, "Coordinate descent"): HALS on sum_Omega (v - W H)^2 with
scikit-learn's penalties, every row of a factor against its OWN Gram matrix over its observed entries.

A half-step over an image (ptr / idx / val: CSR with A = W, B = H^T, or CSC with A = H^T, B = W), for every row i with stored entries p:

    G_i = sum_p b_p b_p^T,   c_i = sum_p v_p b_p,       b_p = B[idx[p], :r]            (formed explicitly)
    `sweeps` times, from the old row:  tests/hals_reference.py's sweep of a_i against (G_i, c_i) -- tests/hals_penalty_reference.py's with penalties:
        for k = 0 .. r-1:  d_k = G_i[k,k] + l2 (skipped where d_k <= 0);  a_i[k] <- max(0, a_i[k] - (G_i[k,:] . a_i + l2 a_i[k] - c_i[k] + l1) / d_k)

A row without a stored entry becomes 0; coordinates >= r of an updated row are 0.  One iteration is the H half-step with (l1H, l2H), then the W
half-step with the new H and (l1W, l2W); there is no normalisation.  The error of an iteration is tests/masked_reference.py's: the direct residual
sum over the stored entries for the pair (W of the H step, new H).

`half_step_in` / `run_in` are the same in numpy `dtype` with every sum in REVERSED order (the entries of a row, the coordinates of a dot product):
not a yardstick, a measure of how far plain rounding moves a result on a given case (the fp32 tolerance of the GPU tests is a multiple of it).
"""
import numpy as np

from tests import hals_penalty_reference as pen
from tests import hals_reference as ref
from tests import masked_reference as mref


def normal_equations(ptr, idx, val, B, r, row):
    """(G_i, c_i) of one row in fp64: (r, r) and (r,)."""
    sl = slice(int(ptr[row]), int(ptr[row + 1]))
    Bg = np.asarray(B, dtype=np.float64)[np.asarray(idx[sl], dtype=np.int64), :r]
    return Bg.T @ Bg, Bg.T @ np.asarray(val[sl], dtype=np.float64)


def sweep_row(a, c, G, sweeps, l1, l2):
    """`sweeps` sweeps of one row a (r,) against (G, c)."""
    P = np.array(a, dtype=np.float64)[:, None]
    for _ in range(sweeps):
        P = pen.sweep(P, c[:, None], G, l1, l2) if (l1 != 0 or l2 != 0) else ref.sweep(P, c[:, None], G)
    return P[:, 0]


def half_step(ptr, idx, val, A, B, r, rows=None, sweeps=1, l1=0.0, l2=0.0):
    """(A_new, G, c): A (>= rows, R) with rows < `rows` updated (their coordinates >= r set to 0) and the others as given; G (rows, r, r), c (rows, r)."""
    A = np.array(A, dtype=np.float64)
    rows = len(ptr) - 1 if rows is None else rows
    G = np.zeros((rows, r, r)); c = np.zeros((rows, r))
    for i in range(rows):
        A[i, r:] = 0.0
        if ptr[i + 1] == ptr[i]:
            A[i, :r] = 0.0
            continue
        G[i], c[i] = normal_equations(ptr, idx, val, B, r, i)
        A[i, :r] = sweep_row(A[i, :r], c[i], G[i], sweeps, l1, l2)
    return A, G, c


def frobenius(rows, cols, vals, W, H):
    wh = mref._dots(np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64), W, np.ascontiguousarray(H.T), 1 << 16)
    return float(np.sqrt(np.sum((np.asarray(vals, dtype=np.float64) - wh) ** 2)))


def images(rows, cols, vals, m, n):
    """(CSR, CSC) of the entries, each (ptr, idx, val)."""
    return mref.csr_of(rows, cols, vals, m), mref.csc_of(rows, cols, vals, n)


def iteration(rows, cols, vals, W, H, sweeps_h=1, sweeps_w=1, penalties=(0.0, 0.0, 0.0, 0.0), const_w=False, imgs=None):
    """(W, H, frobenius) after one iteration on float64 copies; penalties = (l1W, l1H, l2W, l2H)."""
    W = np.array(W, dtype=np.float64); H = np.array(H, dtype=np.float64)
    m, r = W.shape
    n = H.shape[1]
    l1W, l1H, l2W, l2H = penalties
    csr, csc = imgs if imgs is not None else images(rows, cols, vals, m, n)
    Ht, _, _ = half_step(*csc, H.T, W, r, n, sweeps_h, l1H, l2H)
    H = np.ascontiguousarray(Ht.T)
    frob = frobenius(rows, cols, vals, W, H)
    if not const_w:
        W, _, _ = half_step(*csr, W, Ht, r, m, sweeps_w, l1W, l2W)
    return W, H, frob


def run(rows, cols, vals, W, H, iterations, sweeps_h=1, sweeps_w=1, penalties=(0.0, 0.0, 0.0, 0.0), const_w=False):
    """(W, H, [frobenius per iteration])"""
    imgs = images(rows, cols, vals, W.shape[0], H.shape[1])
    errs = []
    for _ in range(iterations):
        W, H, f = iteration(rows, cols, vals, W, H, sweeps_h, sweeps_w, penalties, const_w, imgs)
        errs.append(f)
    return W, H, errs


def objective(rows, cols, vals, W, H, penalties=(0.0, 0.0, 0.0, 0.0)):
    """The penalised objective over the stored entries (W, H >= 0)."""
    l1W, l1H, l2W, l2H = penalties
    return 0.5 * frobenius(rows, cols, vals, W, H) ** 2 + l1W * W.sum() + l1H * H.sum() + 0.5 * l2W * (W * W).sum() + 0.5 * l2H * (H * H).sum()


# ------------------------------------------------------------------ the rounding measure

def half_step_in(ptr, idx, val, A, B, r, rows=None, sweeps=1, l1=0.0, l2=0.0, dtype=np.float32):
    """half_step's A_new with every operation in numpy `dtype` and every sum reversed: G_i and c_i add the row's entries last to first, one at a
    time, and the dot product of a step runs over the coordinates r-1 .. 0."""
    f = np.dtype(dtype).type
    A = np.array(A, dtype=f); B = np.asarray(B, dtype=f); val = np.asarray(val, dtype=f)
    l1, l2 = f(l1), f(l2)
    rows = len(ptr) - 1 if rows is None else rows
    for i in range(rows):
        A[i, r:] = 0
        if ptr[i + 1] == ptr[i]:
            A[i, :r] = 0
            continue
        G = np.zeros((r, r), dtype=f); c = np.zeros(r, dtype=f)
        for p in range(int(ptr[i + 1]) - 1, int(ptr[i]) - 1, -1):
            b = B[idx[p], :r]
            G += np.outer(b, b)
            c += val[p] * b
        a = A[i, :r].copy()
        for _ in range(sweeps):
            for k in range(r):
                d = G[k, k] + l2
                if d <= 0:
                    continue
                a[k] = max(f(0), a[k] - (G[k, ::-1] @ a[::-1] + l2 * a[k] - c[k] + l1) / d)
        A[i, :r] = a
    return A


def run_in(rows, cols, vals, W, H, iterations, sweeps_h=1, sweeps_w=1, penalties=(0.0, 0.0, 0.0, 0.0), const_w=False, dtype=np.float32):
    """(W, H) of `iterations` iterations through half_step_in."""
    f = np.dtype(dtype).type
    W = np.array(W, dtype=f); H = np.array(H, dtype=f)
    m, r = W.shape
    n = H.shape[1]
    l1W, l1H, l2W, l2H = penalties
    csr, csc = images(rows, cols, vals, m, n)
    for _ in range(iterations):
        Ht = half_step_in(*csc, H.T, W, r, n, sweeps_h, l1H, l2H, dtype)
        H = np.ascontiguousarray(Ht.T)
        if not const_w:
            W = half_step_in(*csr, W, Ht, r, m, sweeps_w, l1W, l2W, dtype)
    return W, H


# ------------------------------------------------------------------ problems

def start(m, n, r, seed):
    """A random positive start in fp64: entries in (0, 1]."""
    rng = np.random.default_rng(1000 + seed)
    return 1.0 - rng.random((m, r)), 1.0 - rng.random((r, n))


# (m, n, r, density, seed) of masked_reference.planted_ratings: the problems on which coordinate descent was compared with the multiplicative update
TABLE = ((90, 70, 6, 0.3, 1), (200, 150, 12, 0.1, 2), (120, 100, 5, 0.5, 3))
