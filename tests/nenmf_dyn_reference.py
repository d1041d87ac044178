"""fp64 numpy restatement of NeNMF with per-column dynamic stopping of the projected-gradient steps (docs/NENMF.md, "Dynamic stopping"), built on
tests/nenmf_reference.py, whose step arithmetic it repeats operation for operation and whose products, normalisation and error it calls.

One step launch against a fixed Gram matrix G, right-hand side A and penalties (l1, l2), with a maximum of T steps and a tolerance delta in [0, 1), treats every
column on its own, L and the momentum coefficients c_t being the launch's:
    Y_0 = P_0;  for t = 0 ... T - 1:
        P_{t+1} = max(0, Y_t - (G Y_t + l2 Y_t - a + l1) / L)
        d_t     = sum_{k < r} (P_{t+1}[k] - Y_t[k])^2
        count   = t + 1
        if d_t <= delta^2 d_0: the column is frozen, its result is P_{t+1}          (at t = 0 and delta < 1: only where the step moved nothing, a fixed point)
        else Y_{t+1} = P_{t+1} + c_t (P_{t+1} - P_t)
A frozen column is never stepped again.  L <= 0 or not finite: no step, counts 0.

`forced` replaces the rule by given per-column counts: the GPU tests feed the kernel's own counts back, so that the values are compared exactly where the kernel
stopped and the rule is compared separately (a column on the threshold may freeze one step apart in another precision or summation order).  `dtype` runs every
product, step and d_t in a numpy dtype.  The remaining switches are the mistakes that tests/test_nenmf_dyn_cpu.py must be able to tell from the rule.
"""
import numpy as np

from tests import hals_reference as ref
from tests import nenmf_reference as nenmf


def tol2_of(tol, dtype):
    """delta^2 as the launcher forms it: delta rounded to dtype, squared in double, rounded once to dtype."""
    f = np.dtype(dtype).type
    return f(float(f(tol)) * float(f(tol)))


def apg_dyn(P, A, G, T, tol, l1=0.0, l2=0.0, dtype=np.float64, forced=None, d_against_p=False, threshold_from_previous=False, extrapolate_frozen=False, give_d=False):
    """(P, counts) after at most T steps on the columns of P (r x ncols) against A and G; with give_d also the last d_t of every column and L.  Every column is
    stepped with the whole panel (the arithmetic of nenmf_reference.apg, a frozen column's result dropped), so that forced = T is that function bit for bit."""
    f = np.dtype(dtype).type
    P, A, G = (np.array(x, dtype=f) for x in (P, A, G))
    ncols = P.shape[1]
    l1, l2 = f(l1), f(l2)
    counts = np.zeros(ncols, dtype=np.int32)
    d_last = np.zeros(ncols, dtype=f)
    L = G.sum(axis=1, dtype=f).max() + l2
    if not (L > 0 and np.isfinite(L)):
        return (P, counts, d_last, L) if give_d else (P, counts)
    tol2 = tol2_of(tol, f)
    Y = P.copy()
    c = [f(x) for x in nenmf.momentum(T)]
    live = np.ones(ncols, dtype=bool)
    thr = np.zeros(ncols, dtype=f)
    for t in range(T):
        act = live if forced is None else np.asarray(forced) > t
        if not act.any():
            break
        grad = G @ Y + l2 * Y - A + l1
        Pn = np.maximum(f(0), Y - grad / L)
        moved = Pn - (P if d_against_p else Y)
        d = (moved * moved).sum(axis=0, dtype=f)
        Yn = Pn + c[t] * (Pn - P)
        P = np.where(act, Pn, P)
        Y = np.where(act, Yn, Y)
        counts[act] = t + 1
        d_last[act] = d[act]
        if forced is None and tol > 0:
            if t == 0:
                thr = tol2 * d
            frozen = act & (d <= thr)
            if extrapolate_frozen:
                P = np.where(frozen, Yn, P)
            live = act & ~frozen
            if threshold_from_previous:
                thr = tol2 * d
    return (P, counts, d_last, L) if give_d else (P, counts)


def panel_rhs(slabs, r, len_valid, dtype=np.float64):
    """The summed slabs of the valid block, as nenmf_reference.panel_steps sums them: (len_valid, r)."""
    return np.asarray(slabs, dtype=dtype).sum(axis=0, dtype=dtype)[:len_valid, :r]


def panel_steps_dyn(P, slabs, G, r, len_valid, T, tol, l1=0.0, l2=0.0, dtype=np.float64, forced=None, **mistakes):
    """The step launch on the valid block of a case in panel layout (P (len_pad, RP), slabs (S, len_pad, RP)): ((len_valid, r) block, len_valid counts)."""
    A = panel_rhs(slabs, r, len_valid, dtype)
    out, counts = apg_dyn(P[:len_valid, :r].T, A.T, G[:r, :r], T, tol, l1, l2, dtype, forced, **mistakes)
    return out.T, counts


def projected_gradient_norm(P, A, G, l1=0.0, l2=0.0):
    """Per column, the norm of the projected gradient of 1/2 p^T (G + l2 I) p - (a - l1)^T p over p >= 0 at P (r x ncols), in fp64: the gradient where p > 0,
    its negative part where p = 0."""
    P, A, G = (np.asarray(x, dtype=np.float64) for x in (P, A, G))
    g = G @ P + l2 * P - A + l1
    pg = np.where(P > 0, g, np.minimum(g, 0.0))
    return np.sqrt((pg * pg).sum(axis=0))


# ------------------------------------------------------------------ iteration level

def iteration(V, W, H, t_h, t_w, tol, penalties=(0.0, 0.0, 0.0, 0.0), constant_w=False, forced_h=None, forced_w=None, dtype=np.float64):
    """(W, H, error, counts_h, counts_w) after one iteration: nenmf_reference.iteration with the dynamic steps.  counts_w is None with constant W.  In another dtype
    than fp64: nenmf_reference.run_in's iteration, every product, step and norm in that dtype."""
    f = np.dtype(dtype).type
    l1W, l1H, l2W, l2H = penalties
    V, W, H = (np.array(x, dtype=f) for x in (V, W, H))
    H, ch = apg_dyn(H, W.T @ V, W.T @ W, t_h, tol, l1H, l2H, f, forced_h)
    err = float(np.linalg.norm(np.asarray(V, np.float64) - np.asarray(W, np.float64) @ np.asarray(H, np.float64)))
    cw = None
    if not constant_w:
        Q = H @ H.T
        Wt, cw = apg_dyn(W.T, (V @ H.T).T, Q.T, t_w, tol, l1W, l2W, f, forced_w)
        W = Wt.T if f is np.float64 else np.ascontiguousarray(Wt.T)      # (the layouts of nenmf_reference.iteration and run_in: the sums of the norms follow them)
        if not any(penalties):
            if f is np.float64:
                W, H = ref.normalize(W, H)
            else:
                d = np.sqrt((W * W).sum(axis=0))
                on = d > 0
                W[:, on] /= d[on]
                H[on] *= d[on][:, None]
    return W, H, err, ch, cw


def run(V, W, H, iters, t_h, t_w, tol, penalties=(0.0, 0.0, 0.0, 0.0), constant_w=False, forced=None, dtype=np.float64):
    """(W, H, [error per iteration], [(counts_h, counts_w) per iteration]).  forced: such a list of counts, applied in place of the rule."""
    errs, counts = [], []
    for i in range(iters):
        fh, fw = (None, None) if forced is None else forced[i]
        W, H, e, ch, cw = iteration(V, W, H, t_h, t_w, tol, penalties, constant_w, fh, fw, dtype)
        errs.append(e)
        counts.append((ch, cw))
    return W, H, errs, counts
