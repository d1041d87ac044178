"""fp64 numpy restatement of NeNMF (docs/NENMF.md; Guan, Tao, Luo, Yuan 2012): Nesterov-accelerated projected-gradient steps on the NNLS problem of one factor, in
the iteration of HALS.  The products, the normalisation and the error are those of tests/hals_reference.py / tests/hals_penalty_reference.py, which this module
calls and does not restate.

For a panel P (r x ncols), the Gram matrix G, the right-hand side A and the penalties (l1, l2) of that factor:
    L = max_k sum_l G[k, l] + l2
    Y_0 = P_0, alpha_0 = 1
    P_{t+1} = max(0, Y_t - (G Y_t + l2 Y_t - A + l1) / L);  alpha_{t+1} = (1 + sqrt(4 alpha_t^2 + 1)) / 2;  Y_{t+1} = P_{t+1} + (alpha_t - 1) / alpha_{t+1} (P_{t+1} - P_t)
and the result is P_T.  L <= 0 or not finite: P_0.  The coefficient behind the first step is (alpha_0 - 1) / alpha_1 = 0: Y_1 = P_1.

`apg` takes the mistakes that tests/test_nenmf_cpu.py must be able to tell from the real thing as switches; `run_in` is the whole iteration in a numpy dtype -- not a
yardstick for the kernel but a measure of how far plain rounding moves a result (tests/nenmf_cases.py takes the fp32 tolerances from it).
"""
import numpy as np

from tests import hals_penalty_reference as pen
from tests import hals_reference as ref


def momentum(T):
    """[(alpha_t - 1) / alpha_{t+1} for t < T], in double."""
    out, alpha = [], 1.0
    for _ in range(T):
        nxt = (1.0 + np.sqrt(4.0 * alpha * alpha + 1.0)) / 2.0
        out.append((alpha - 1.0) / nxt)
        alpha = nxt
    return out


def lipschitz(G, l2=0.0):
    """The infinity norm of G (row sums as they are: G = W^T W >= 0 entrywise) + l2, an upper bound of lambda_max(G + l2 I)."""
    return np.asarray(G).sum(axis=1).max() + l2


def apg(P, A, G, T, l1=0.0, l2=0.0, dtype=np.float64, with_momentum=True, give_y=False, l2_in_L=True, l1_in_gradient=True):
    """T steps on the columns of P (r x ncols) against A and G, every operation in numpy `dtype`; the momentum coefficients in double, rounded to dtype.  The
    switches are the mistakes of tests/test_nenmf_cpu.py; all at their defaults: the algorithm."""
    f = np.dtype(dtype).type
    P, A, G = (np.array(x, dtype=f) for x in (P, A, G))
    l1, l2 = f(l1), f(l2)
    L = G.sum(axis=1, dtype=f).max() + (l2 if l2_in_L else f(0))
    if not (L > 0 and np.isfinite(L)):
        return P
    Y = P.copy()
    c = [f(x) for x in momentum(T)]
    for t in range(T):
        grad = G @ Y + l2 * Y - A + (l1 if l1_in_gradient else f(0))
        Pn = np.maximum(f(0), Y - grad / L)
        Y = Pn + (c[t] if with_momentum else f(0)) * (Pn - P)
        P = Pn
    return Y if give_y else P


def h_step(V, W, H, T, l1H=0.0, l2H=0.0):
    return apg(H, W.T @ V, W.T @ W, T, l1H, l2H)


def w_step(V, W, H, T, l1W=0.0, l2W=0.0):
    Q = H @ H.T
    return apg(W.T, (V @ H.T).T, Q.T, T, l1W, l2W).T


def iteration(V, W, H, t_h, t_w, penalties=(0.0, 0.0, 0.0, 0.0), constant_w=False):
    """(W, H, error) after one iteration, in fp64: hals_multi_reference.iteration with T steps in place of the sweeps.  penalties = (l1W, l1H, l2W, l2H)."""
    l1W, l1H, l2W, l2H = penalties
    V, W, H = (np.asarray(x, dtype=np.float64) for x in (V, W, H))
    H = h_step(V, W, H, t_h, l1H, l2H)
    err = float(np.linalg.norm(V - W @ H))
    if not constant_w:
        W = w_step(V, W, H, t_w, l1W, l2W)
        if not any(penalties):
            W, H = ref.normalize(W, H)
    return W, H, err


def run(V, W, H, iters, t_h, t_w, penalties=(0.0, 0.0, 0.0, 0.0), constant_w=False):
    """(W, H, [error per iteration])"""
    W, H = np.asarray(W, dtype=np.float64), np.asarray(H, dtype=np.float64)
    errs = []
    for _ in range(iters):
        W, H, e = iteration(V, W, H, t_h, t_w, penalties, constant_w)
        errs.append(e)
    return W, H, errs


def run_in(V, W, H, iters, t_h, t_w, dtype, penalties=(0.0, 0.0, 0.0, 0.0), constant_w=False):
    """(W, H) after `iters` iterations with every product, step and norm in numpy `dtype`."""
    f = np.dtype(dtype).type
    l1W, l1H, l2W, l2H = penalties
    V, W, H = (np.array(x, dtype=f) for x in (V, W, H))
    for _ in range(iters):
        H = apg(H, W.T @ V, W.T @ W, t_h, l1H, l2H, dtype=f)
        if constant_w:
            continue
        Q = H @ H.T
        W = np.ascontiguousarray(apg(W.T, (V @ H.T).T, Q.T, t_w, l1W, l2W, dtype=f).T)
        if not any(penalties):
            d = np.sqrt((W * W).sum(axis=0))
            live = d > 0
            W[:, live] /= d[live]
            H[live] *= d[live][:, None]
    return W, H


def objective(V, W, H, penalties=(0.0, 0.0, 0.0, 0.0)):
    """The penalised objective 1/2 ||V - W H||^2 + l1W ||W||_1 + l1H ||H||_1 + 1/2 l2W ||W||^2 + 1/2 l2H ||H||^2 (hals_penalty_reference.objective)."""
    l1W, l1H, l2W, l2H = penalties
    return pen.objective(V, W, H, l1W, l1H, l2W, l2H)


def panel_steps(P, slabs, G, r, len_valid, T, l1=0.0, l2=0.0, dtype=np.float64, **mistakes):
    """The T steps of the valid block of a case in panel layout (hals_reference's sweep problems): ((len_valid, r) new block, the summed slabs of that block)."""
    A = np.asarray(slabs, dtype=dtype).sum(axis=0, dtype=dtype)[:len_valid, :r]
    return apg(P[:len_valid, :r].T, A.T, G[:r, :r], T, l1, l2, dtype=dtype, **mistakes).T, A
