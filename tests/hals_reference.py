"""fp64 numpy restatement of one HALS iteration (docs/HALS.md), the yardstick of tests/test_hals_cpu.py and tests/test_gpu_hals.py.

One iteration, H then W:
  H step: G = W^T W, A = W^T V; for k = 0 .. r-1 (skipping G[k,k] <= 0), every column at once:
          H[k,:] <- max(0, H[k,:] - (G[k,:] H - A[k,:]) / G[k,k])       (rows l < k already updated: Gauss-Seidel)
  W step: Q = H H^T, B = V H^T;  W[:,k] <- max(0, W[:,k] - (W Q[:,k] - B[:,k]) / Q[k,k])
  normalisation: d = ||W[:,k]||; where d > 0, W[:,k] /= d and H[k,:] *= d (W H unchanged)
The error of the iteration is ||V - W H|| with the W of the H step and the new H (before the normalisation), as the engine reports it.
"""
import numpy as np


def h_step(V, W, H):
    G = W.T @ W
    A = W.T @ V
    H = H.copy()
    for k in range(H.shape[0]):
        if G[k, k] <= 0:
            continue
        H[k, :] = np.maximum(0.0, H[k, :] - (G[k, :] @ H - A[k, :]) / G[k, k])
    return H


def w_step(V, W, H):
    Q = H @ H.T
    B = V @ H.T
    W = W.copy()
    for k in range(W.shape[1]):
        if Q[k, k] <= 0:
            continue
        W[:, k] = np.maximum(0.0, W[:, k] - (W @ Q[:, k] - B[:, k]) / Q[k, k])
    return W


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


def run(V, W, H, iters, constant_w=False):
    """(W, H, [error per iteration])"""
    W, H = np.asarray(W, dtype=np.float64), np.asarray(H, dtype=np.float64)
    errs = []
    for _ in range(iters):
        W, H, e = iteration(V, W, H, constant_w)
        errs.append(e)
    return W, H, errs
