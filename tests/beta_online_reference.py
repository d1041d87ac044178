"""The numpy restatement of the minibatch (online) dense beta-divergence update (docs/DIVERGENCE.md, "Minibatch update"), dtype-generic: scikit-learn's
MiniBatchNMF (Lefevre, Bach & Fevotte 2011) in this project's orientation -- V is m x n with the samples as COLUMNS, so V = X^T, W = components_^T, H = codes^T.

The batches are the column ranges [0, b), [b, 2b), ... in order, the last one the remainder; rho = forget_factor^(min(b, n) / n).  One step on the columns J, with
P = W H_J + eps and gamma, the penalties and eps those of tests/beta_general_reference.py:
    H_J <- H_J .* (num ./ (den + eps + l1H + l2H H_J))^gamma                                           the ordinary half-step on the batch's columns
    num = (V_J .* P^(beta - 2)) H_J^T,  den = P^(beta - 1) H_J^T + eps + l1W + l2W W                   with the new H_J, reduced over J only
    A <- rho A + W^(1/gamma) .* num,   B <- rho B + den,   W <- (A ./ B)^gamma                         the online half-step
and values below eps are set to 0 in H_J when beta < 1 and in W when beta <= 1.  A = W and B = 1 at the start.  One pass is every batch once; there is no
normalisation; the errors of a pass refer to (W_k, H_k) AFTER the pass.  mixed=True takes the products with the bf16 roundings of tests/beta_mixed_reference.py."""
import numpy as np

from tests import beta_general_reference as gen
from tests import beta_mixed_reference as mix

planted, start, gamma_of = gen.planted, gen.start, gen.gamma_of
NO_PENALTIES = gen.NO_PENALTIES


def batches(n, batch_size):
    b = min(int(batch_size), n)
    return [(c0, min(c0 + b, n)) for c0 in range(0, n, b)]


def rho_of(forget_factor, batch_size, n):
    return float(forget_factor) ** (min(int(batch_size), n) / n)


def num_den(X, A, B, beta, eps, mixed=False):
    """The two products of a half-step of the panel A (out x r) against B (red x r) with X (out x red); den is None at beta = 1 (the caller's column sums)."""
    dt = A.dtype.type
    if mixed:
        Q, R = mix._map(X, mix._product(A, B, eps), beta, dt)
        Bb = mix.round_bf16(B)
        return mix.round_bf16(Q) @ Bb, (None if beta == 1 else mix.round_bf16(R) @ Bb)
    Q, R = mix._map(X, A @ B.T + eps, beta, dt)
    return Q @ B, (None if beta == 1 else R @ B)


def power(a, g):
    """a^g by the three cases of the kernels: g = 1, g = 1/2 (a square root), any other g (0 stays 0)."""
    if g == 1.0:
        return a
    if g == 0.5:
        return np.sqrt(a)
    with np.errstate(divide="ignore"):
        return np.where(a > 0, np.exp2(a.dtype.type(g) * np.log2(np.where(a > 0, a, 1))), 0).astype(a.dtype)


def inverse_power(a, g):
    """a^(1/g): a itself, a square at g = 1/2, otherwise exp2(log2(a) / g) with 0 kept at 0."""
    if g == 1.0:
        return a
    if g == 0.5:
        return a * a
    with np.errstate(divide="ignore"):
        return np.where(a > 0, np.exp2(a.dtype.type(1.0 / g) * np.log2(np.where(a > 0, a, 1))), 0).astype(a.dtype)


def update_rows(P, num, den, beta, eps, l1=0.0, l2=0.0, acc=None, rho=0.0, flush=False):
    """What k_beta_update_rows does with the summed numerators num and denominators den (a panel, or a vector at beta = 1) of the panel P: the ordinary update
    (acc None) or the online one (acc = (A, B), which are replaced).  Returns (the new panel, A, B)."""
    dt = P.dtype.type
    g = gamma_of(beta)
    d = den + dt(eps) + dt(l1) + dt(l2) * P
    if acc is None:
        new, A, B = P * power(num / d, g), None, None
    else:
        A = dt(rho) * acc[0] + inverse_power(P, g) * num
        B = dt(rho) * acc[1] + d
        new = power(A / B, g)
    if flush:
        new = np.where(new < dt(eps), dt(0), new)
    return new.astype(P.dtype), A, B


def half_step(X, P, B, beta, eps, l1=0.0, l2=0.0, acc=None, rho=0.0, flush=False, mixed=False):
    """beta_general_reference.half_step's arguments, followed by update_rows'."""
    num, den = num_den(X, P, B, beta, eps, mixed)
    if den is None:
        den = B.sum(axis=0)
    return update_rows(P, num, den, beta, eps, l1, l2, acc, rho, flush)


def step(V, W, H, A, B, cols, beta, eps, rho, pen=NO_PENALTIES, mixed=False, flushed=None):
    """One step on the columns cols = (c0, c1): returns the new (W, H, A, B); H is changed in its columns c0 .. c1 only.  flushed (a list): gets the number of
    entries the two flushes set to 0 that were not 0 before them."""
    l1W, l1H, l2W, l2H = pen
    c0, c1 = cols
    VJ = V[:, c0:c1]
    HJ, _, _ = half_step(VJ.T, H[:, c0:c1].T, W, beta, eps, l1H, l2H, mixed=mixed)
    if beta < 1:
        if flushed is not None:
            flushed.append(int(np.count_nonzero((HJ < eps) & (HJ != 0))))
        HJ = np.where(HJ < eps, HJ.dtype.type(0), HJ)
    H = H.copy()
    H[:, c0:c1] = HJ.T
    Wn, A, B = half_step(VJ, W, HJ, beta, eps, l1W, l2W, acc=(A, B), rho=rho, mixed=mixed)
    if beta <= 1:
        if flushed is not None:
            flushed.append(int(np.count_nonzero((Wn < eps) & (Wn != 0))))
        Wn = np.where(Wn < eps, Wn.dtype.type(0), Wn)
    return Wn, H, A, B


def run_pass(V, W, H, A, B, batch_size, beta, eps, rho, pen=NO_PENALTIES, mixed=False, flushed=None):
    for cols in batches(V.shape[1], batch_size):
        W, H, A, B = step(V, W, H, A, B, cols, beta, eps, rho, pen, mixed, flushed)
    return W, H, A, B


def objective(V, W, H, beta, eps, pen=NO_PENALTIES):
    """The divergence over the whole of V plus the penalty terms (beta_general_reference.objective)."""
    return gen.objective(V, W, H, beta, eps, pen)


def run(V, W0, H0, passes, beta, eps, batch_size, forget_factor=0.7, pen=NO_PENALTIES, dtype=np.float64, mixed=False, flushed=None):
    """`passes` passes from (W0, H0) with A = W0, B = 1.  Returns (W, H, frobenius, rmsd, divergence), the errors of (W, H) after the last pass over the whole of V."""
    V = np.asarray(V, dtype=dtype); W = np.array(W0, dtype=dtype); H = np.array(H0, dtype=dtype)
    eps = dtype(eps)
    m, n = V.shape
    A, B = W.copy(), np.ones_like(W)
    rho = rho_of(forget_factor, batch_size, n)
    for _ in range(passes):
        W, H, A, B = run_pass(V, W, H, A, B, batch_size, beta, eps, rho, pen, mixed, flushed)
    tf, td = (mix.terms if mixed else gen.terms)(V, W, H.T, beta, eps)
    frob = float(np.sqrt(tf.astype(np.float64).sum()))
    return np.asfortranarray(W), np.asfortranarray(H), frob, frob / np.sqrt(float(m) * n), float(td.astype(np.float64).sum())
