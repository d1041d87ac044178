"""fp64 numpy restatement of accelerated HALS with per-column dynamic stopping (docs/HALS.md, "Dynamic stopping"), built on tests/hals_multi_reference.py.

One panel sweep step against a fixed Gram matrix G and right-hand side a, with a maximum of s sweeps and a tolerance delta in [0, 1), treats every column on its own:
  sweep t = 1, 2, ... is the (penalised) Gauss-Seidel pass of hals_reference / hals_penalty_reference over k = 0 ... r - 1;
  d_t = sum_{k < r} (p_k^(t) - p_k^(t-1))^2;
  after sweep t the column is frozen if d_t <= delta^2 d_1 (at t = 1 and delta < 1: only where the sweep moved nothing, a fixed point);
  a frozen column is never stepped again; a column is also done after sweep s;
  count = the number of sweeps applied, 1 ... s.
delta = 0 is hals_multi_reference.sweeps itself (the same calls: bit for bit), with every count s.

`forced` replaces the rule by given per-column counts: the GPU tests feed the kernel's own counts back, so that the values are compared exactly where the kernel
stopped and the rule is compared separately (a column on the threshold may freeze one sweep apart in another precision or summation order).  `dtype` runs
every product, step and d_t in a numpy dtype: not a yardstick for the kernels, but the measure of how many columns plain fp32 rounding moves across the threshold
(tests/test_hals_dyn_cpu.py holds the GPU tests' inputs to the cap with it).
"""
import numpy as np

from tests import hals_multi_reference as multi
from tests import hals_reference as ref


def sweeps_dyn(P, A, G, r=None, s=1, tol=0.0, l1=0.0, l2=0.0, forced=None, dtype=np.float64, history=None):
    """(P, counts) after at most s sweeps of the columns of P (R x ncols) against A and G.  history: a list that receives P[:r] after every sweep."""
    f = np.dtype(dtype).type
    R, ncols = np.shape(P)
    r = R if r is None else r
    if tol == 0 and forced is None and f is np.float64 and history is None:
        return multi.sweeps(P, A, G, r, s, l1, l2), np.full(ncols, s, dtype=np.int32)
    P = np.array(P, dtype=f)
    A = np.asarray(A, dtype=f)
    G = np.asarray(G, dtype=f)
    l1, l2 = f(l1), f(l2)
    penalised = l1 != 0 or l2 != 0
    tol2 = f(tol * tol)                              # delta^2, rounded once to the precision of the run
    counts = np.zeros(ncols, dtype=np.int32)
    live = np.ones(ncols, dtype=bool)
    thr = np.zeros(ncols, dtype=f)
    for t in range(s):
        idx = np.flatnonzero(live if forced is None else np.asarray(forced) > t)
        if idx.size == 0:
            break
        old = P[:r, idx]
        new = old.copy()
        a = A[:r, idx]
        for k in range(r):
            d = G[k, k] + l2 if penalised else G[k, k]
            if d <= 0:
                continue
            if penalised:
                new[k] = np.maximum(f(0), new[k] - (G[k, :r] @ new + l2 * new[k] - a[k] + l1) / d)
            else:
                new[k] = np.maximum(f(0), new[k] - (G[k, :r] @ new - a[k]) / d)
        P[:r, idx] = new
        counts[idx] = t + 1
        if history is not None:
            history.append(P[:r].copy())
        if forced is None and tol > 0:
            moved = new - old
            d_t = (moved * moved).sum(axis=0, dtype=f)
            if t == 0:
                thr[idx] = tol2 * d_t
            live[idx] = ~(d_t <= thr[idx])
    return P, counts


def column_objective(P, A, G, r, l1=0.0, l2=0.0):
    """The (penalised) objective of every column for fixed G and a, up to its constant: 1/2 p^T G p - a^T p + l1 sum p + 1/2 l2 p^T p (p >= 0)."""
    p = np.asarray(P, dtype=np.float64)[:r]
    G = np.asarray(G, dtype=np.float64)[:r, :r]
    a = np.asarray(A, dtype=np.float64)[:r]
    return 0.5 * (p * (G @ p)).sum(axis=0) - (a * p).sum(axis=0) + l1 * p.sum(axis=0) + 0.5 * l2 * (p * p).sum(axis=0)


def panel_sweeps_dyn(P, slabs, G, r, len_valid, s, tol, l1=0.0, l2=0.0, forced=None, dtype=np.float64):
    """The step on the valid block of a case in panel layout (P (len_pad, RP), slabs (S, len_pad, RP)): ((len_valid, r) values, len_valid counts).  The slabs are
    summed in fp64 and the sum rounded to dtype."""
    A = np.asarray(slabs, dtype=np.float64)[:, :len_valid, :r].sum(axis=0)
    out, counts = sweeps_dyn(np.asarray(P)[:len_valid, :r].T, A.T, np.asarray(G)[:r, :r], r, s, tol, l1, l2, forced, dtype)
    return out.T, counts


def dyn_bound(P, slabs, G, r, len_valid, counts, u, l1=0.0, l2=0.0):
    """hals_multi_reference.multi_sweep_bound for per-column counts: column j gets the bound after counts[j] sweeps.  (len_valid, r).  A frozen column is not
    stepped, so no error is added to it after its last sweep."""
    counts = np.asarray(counts)
    hist = multi.multi_sweep_bound(np.asarray(P, np.float64)[:len_valid].T, np.asarray(slabs, np.float64)[:, :len_valid].transpose(0, 2, 1), G, r, int(counts.max()), u,
                                   l1, l2, history=True)
    b = np.zeros((r, len_valid))
    for j in range(len_valid):
        b[:, j] = hist[counts[j] - 1][:, j]
    return b.T


# ------------------------------------------------------------------ iteration level

def h_step(V, W, H, s, tol, l1H=0.0, l2H=0.0, forced=None):
    return sweeps_dyn(H, W.T @ V, W.T @ W, None, s, tol, l1H, l2H, forced)


def w_step(V, W, H, s, tol, l1W=0.0, l2W=0.0, forced=None):
    Q = H @ H.T
    Wt, counts = sweeps_dyn(W.T, (V @ H.T).T, Q.T, None, s, tol, l1W, l2W, forced)
    return Wt.T, counts


def iteration(V, W, H, s_h, s_w, tol, penalties=(0.0, 0.0, 0.0, 0.0), constant_w=False, forced_h=None, forced_w=None):
    """(W, H, error, counts_h, counts_w) after one iteration in fp64: hals_multi_reference.iteration with the dynamic steps.  counts_w is None with constant W."""
    l1W, l1H, l2W, l2H = penalties
    V, W, H = (np.asarray(x, dtype=np.float64) for x in (V, W, H))
    H, ch = h_step(V, W, H, s_h, tol, l1H, l2H, forced_h)
    err = float(np.linalg.norm(V - W @ H))
    cw = None
    if not constant_w:
        W, cw = w_step(V, W, H, s_w, tol, l1W, l2W, forced_w)
        if l1W == 0 and l1H == 0 and l2W == 0 and l2H == 0:
            W, H = ref.normalize(W, H)
    return W, H, err, ch, cw
