"""The numpy restatement of the dense beta-divergence multiplicative update (docs/DIVERGENCE.md) the tests compare the engine with: beta = 1 (generalised KL)
and beta = 0 (Itakura-Saito), dtype-generic (fp64 unless asked otherwise).

With P = W H + eps and gamma = 1 (beta = 1) or 1/2 (beta = 0) one iteration is
    H <- H .* (W^T (V .* P^(beta - 2)) ./ (W^T P^(beta - 1) + eps))^gamma
    W <- W .* ((V .* P^(beta - 2)) H^T ./ (P^(beta - 1) H^T + eps))^gamma        with the new H
    beta = 1: the columns of W are normalised, H is not rescaled (oracle_kl_run's iteration);  beta = 0: W(:, k) /= d_k, H(k, :) *= d_k, d_k = ||W(:, k)|| > 0
and the errors of an iteration refer to (W_{k-1}, H_k): frobenius^2 = sum (v - P)^2, rmsd = frobenius / sqrt(m n), divergence =
sum (v log(v / P) - v + P) over v > 0 plus sum P over v = 0 (beta = 1), sum (v / P - log(v / P) - 1) (beta = 0), all with the W step's own P."""
import numpy as np


def planted(m, n, k=5, seed=0, noise_shape=8.0):
    """A strictly positive matrix with rank structure: a planted rank-k product times gamma noise of mean 1, plus 1e-3."""
    rng = np.random.default_rng(seed)
    V0 = rng.random((m, k)) @ rng.random((k, n))
    return np.asfortranarray(V0 * rng.gamma(noise_shape, 1.0 / noise_shape, (m, n)) + 1e-3)


def start(m, n, r, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    return np.asfortranarray((1.0 - rng.random((m, r))).astype(dtype)), np.asfortranarray((1.0 - rng.random((r, n))).astype(dtype))


def half_step(X, A, B, beta, eps, dsum=None):
    """The update of the panel A (out x r) against B (red x r) with X (out x red) = V seen from A's side: H step X = V^T, A = H^T, B = W; W step X = V, A = W, B = H^T."""
    P = A @ B.T + eps
    if beta == 1:
        num = (X / P) @ B
        den = B.sum(axis=0) if dsum is None else dsum
        return A * (num / (den + eps))
    ip = 1.0 / P
    num = (X * ip * ip) @ B
    den = ip @ B
    return A * np.sqrt(num / (den + eps))


def terms(X, A, B, beta, eps):
    """Per row of A: sum (x - p)^2 and the divergence, with p = A B^T + eps."""
    P = A @ B.T + eps
    tf = ((X - P) ** 2).sum(axis=1)
    if beta == 1:
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(X > 0, X * np.log(np.where(X > 0, X, 1.0) / P), 0.0)
        return tf, (t - X + P).sum(axis=1)
    ratio = X / P
    return tf, (ratio - np.log(ratio) - 1.0).sum(axis=1)


def normalize(W, H, compensated):
    d = np.sqrt((W * W).sum(axis=0))
    d = np.where(d > 0, d, 1.0).astype(W.dtype)
    return W / d, (H * d[:, None] if compensated else H)


def run(V, W0, H0, iters, beta, eps, const_w=False, compensated=None, dtype=np.float64, history=False):
    """`iters` iterations from (W0, H0).  compensated: the normalisation (None: the engine's -- beta = 0 compensated, beta = 1 not).  Returns
    (W, H, frobenius, rmsd, divergence) of the last iteration, and with history=True the divergence of every iteration as a sixth entry."""
    if compensated is None:
        compensated = beta == 0
    V = np.asarray(V, dtype=dtype); W = np.array(W0, dtype=dtype); H = np.array(H0, dtype=dtype)
    eps = dtype(eps)
    m, n = V.shape
    frob = rmsd = div = 0.0
    hist = []
    for it in range(1, iters + 1):
        H = half_step(V.T, H.T, W, beta, eps).T
        if history or it == iters:
            tf, td = terms(V, W, H.T, beta, eps)
            frob = float(np.sqrt(tf.astype(np.float64).sum())); rmsd = frob / np.sqrt(float(m) * n); div = float(td.astype(np.float64).sum())
            hist.append(div)
        if not const_w:
            W = half_step(V, W, H.T, beta, eps)
            W, H = normalize(W, H, compensated)
    out = (np.asfortranarray(W), np.asfortranarray(H), frob, rmsd, div)
    return out + (hist,) if history else out
