"""fp64 numpy restatement of accelerated HALS (docs/HALS.md, "Inner sweeps"; Gillis & Glineur 2012), built on tests/hals_reference.py and
tests/hals_penalty_reference.py.

With s_H and s_W sweeps per product, one iteration is
  H step: G = W^T W and A = W^T V once, then the sweep of hals_reference (hals_penalty_reference with (l1H, l2H)) s_H times, each from the result of the one before;
  W step: Q = H H^T and B = V H^T from the new H once, then s_W sweeps with (l1W, l2W);
  the normalisation of hals_reference, skipped while a penalty is non-zero.
The error of an iteration is ||V - W H|| with the W of the H step and the H after the last H sweep.  (1, 1) is hals_reference.iteration (hals_penalty_reference.iteration with
penalties) bit for bit: the same calls in the same order.

`multi_sweep_bound` carries hals_reference.sweep_bound over the sweeps; `run_in` is the same iteration in a numpy dtype -- not a yardstick for the kernels, but a
measure of how far plain rounding moves a trajectory (tests/hals_multi_cases.py takes the fp32 tolerance of the engine tests from it).
"""
import numpy as np

from tests import hals_penalty_reference as pen
from tests import hals_reference as ref


def sweeps(P, A, G, r=None, s=1, l1=0.0, l2=0.0):
    """s applications of the sweep to the columns of P (R x ncols) against one A and one G, in fp64: hals_reference.sweep where both penalties are 0 (the same
    arithmetic as without the counts), else hals_penalty_reference.sweep."""
    P = np.array(P, dtype=np.float64)
    for _ in range(s):
        P = ref.sweep(P, A, G, r) if l1 == 0 and l2 == 0 else pen.sweep(P, A, G, l1, l2, r)
    return P


def h_step(V, W, H, s=1, l1H=0.0, l2H=0.0):
    return sweeps(H, W.T @ V, W.T @ W, None, s, l1H, l2H)


def w_step(V, W, H, s=1, l1W=0.0, l2W=0.0):
    Q = H @ H.T
    return sweeps(W.T, (V @ H.T).T, Q.T, None, s, l1W, l2W).T


def iteration(V, W, H, s_h=1, s_w=1, penalties=(0.0, 0.0, 0.0, 0.0), constant_w=False):
    """(W, H, error) after one iteration, in fp64.  penalties = (l1W, l1H, l2W, l2H)."""
    l1W, l1H, l2W, l2H = penalties
    V, W, H = (np.asarray(x, dtype=np.float64) for x in (V, W, H))
    H = h_step(V, W, H, s_h, l1H, l2H)
    err = float(np.linalg.norm(V - W @ H))
    if not constant_w:
        W = w_step(V, W, H, s_w, l1W, l2W)
        if l1W == 0 and l1H == 0 and l2W == 0 and l2H == 0:
            W, H = ref.normalize(W, H)
    return W, H, err


def run(V, W, H, iters, s_h=1, s_w=1, penalties=(0.0, 0.0, 0.0, 0.0), constant_w=False):
    """(W, H, [error per iteration])"""
    W, H = np.asarray(W, dtype=np.float64), np.asarray(H, dtype=np.float64)
    errs = []
    for _ in range(iters):
        W, H, e = iteration(V, W, H, s_h, s_w, penalties, constant_w)
        errs.append(e)
    return W, H, errs


def run_in(V, W, H, iters, s_h, s_w, dtype, penalties=(0.0, 0.0, 0.0, 0.0), constant_w=False):
    """(W, H) after `iters` iterations with every product, sweep and norm in numpy `dtype` (hals_reference.iteration_in with the counts and the penalties)."""
    f = np.dtype(dtype).type
    l1W, l1H, l2W, l2H = (f(x) for x in penalties)
    V, W, H = (np.array(x, dtype=f) for x in (V, W, H))

    def sweeps_in(P, A, G, s, l1, l2):
        P = P.copy()
        for _ in range(s):
            for k in range(P.shape[0]):
                d = G[k, k] + l2
                if d <= 0:
                    continue
                P[k] = np.maximum(f(0), P[k] - (G[k] @ P + l2 * P[k] - A[k] + l1) / d)
        return P

    for _ in range(iters):
        H = sweeps_in(H, W.T @ V, W.T @ W, s_h, l1H, l2H)
        if constant_w:
            continue
        Q = H @ H.T
        W = sweeps_in(W.T.copy(), (V @ H.T).T, Q.T, s_w, l1W, l2W).T
        if not any(penalties):
            d = np.sqrt((W * W).sum(axis=0))
            live = d > 0
            W[:, live] /= d[live]
            H[live] *= d[live][:, None]
    return W, H


def equivalent_problem(A_slabs, G, r, l1, l2):
    """The penalised sweep is the plain sweep of G + l2 I against a - l1.  Returns (slabs, G) of that problem for slabs of shape (S, RP, valid columns): -l1 on the
    coordinates < r as one more slab, and three empty ones for the roundings the plain sweep does not have (l2 p(k): a product and a sum; G_kk + l2), so that the
    gamma index of sweep_bound grows by four, as in tests/test_gpu_hals_sweep_pen.py.  Without penalties: the problem itself."""
    S = np.asarray(A_slabs, dtype=np.float64)
    G = np.asarray(G, dtype=np.float64)
    if l1 == 0 and l2 == 0:
        return S, G
    extra = np.zeros((4,) + S.shape[1:])
    extra[0, :r] = -l1
    return np.concatenate([S, extra]), G + l2 * np.eye(G.shape[0])


def multi_sweep_bound(P, A_slabs, G, r, s, u, l1=0.0, l2=0.0, history=False):
    """hals_reference.sweep_bound carried over s sweeps: per-element bound on |computed - exact| after s floating-point sweeps of P (RP x ncols) against the slabs
    A_slabs (S x RP x ncols) and G, every dot product and slab sum in any order with unit roundoff u.  In sweep t, step k has the local error delta_k^(t) of
    sweep_bound, formed from the exact state of that step, and the new h_k depends (in exact arithmetic) on the h_l, l != k -- on the entries l < k of this sweep
    and l > k of the sweep before, not on its own old value -- with the weights G_kl / G_kk:
        b_k^(t) = delta_k^(t) + sum_{l<k} |G_kl| / G_kk b_l^(t) + sum_{l>k} |G_kl| / G_kk b_l^(t-1),     b^(0) = 0.
    A skipped coordinate keeps its exact input through every sweep: b_k = 0.  Penalised form: G_kk + l2 in place of G_kk, through equivalent_problem (every column
    passed in is then taken as valid).  s = 1 is sweep_bound.  Returns b (r x ncols) of the last sweep, or with `history` the list of all s."""
    S, G = equivalent_problem(A_slabs, G, r, l1, l2)
    RP = G.shape[0]
    g = ref.gamma(RP + S.shape[0] + 4, u)
    h = np.array(P[:r], dtype=np.float64)
    A = S.sum(axis=0)[:r]
    slab_abs = np.abs(S).sum(axis=0)[:r]
    Gr = G[:r, :r]
    b = np.zeros_like(h)
    out = []
    for _ in range(s):
        before = b
        b = np.zeros_like(h)
        for k in range(r):
            d = Gr[k, k]
            if d <= 0:
                continue
            mag = np.abs(Gr[k]) @ np.abs(h)
            h[k] = np.maximum(0.0, h[k] - (Gr[k] @ h - A[k]) / d)
            b[k] = (2.0 * g * (mag + slab_abs[k]) / d + 2.0 * u * np.abs(h[k]) + (np.abs(Gr[k, :k]) / d) @ b[:k]
                    + (np.abs(Gr[k, k + 1:]) / d) @ before[k + 1:])
        out.append(b)
    return out if history else b


def panel_sweeps(P, slabs, G, r, len_valid, s, l1=0.0, l2=0.0):
    """The s fp64 sweeps of the valid block of a case in panel layout (hals_reference's sweep problems): (len_valid, r)."""
    A = np.asarray(slabs, dtype=np.float64).sum(axis=0)
    return sweeps(P[:len_valid, :r].T, A[:len_valid, :r].T, G[:r, :r], r, s, l1, l2).T


def sweeps_f32(P, slabs, G, r, len_valid, s, order="sequential"):
    """hals_reference.sweep_f32 (float32 numpy, a fixed summation order) applied s times, each time to the result of the time before: (len_valid, r)."""
    P = np.array(P, dtype=np.float32)
    for _ in range(s):
        P[:len_valid, :r] = ref.sweep_f32(P, slabs, G, r, len_valid, order)
    return P[:len_valid, :r]
