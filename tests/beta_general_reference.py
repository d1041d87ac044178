"""The numpy restatement of the general dense beta-divergence multiplicative update with L1 / L2 penalties (docs/DIVERGENCE.md, "General beta and the
penalties"), dtype-generic.  It extends tests/beta_reference.py, whose pieces it calls at beta = 0 and beta = 1 without penalties.

With P = W H + eps one iteration is the H step, then the W step with the new H, each
    A <- A .* (num ./ (den + eps + l1 + l2 A))^gamma,    num = (V .* P^(beta - 2)) B,  den = P^(beta - 1) B        (B the other panel)
    gamma = 1 / (2 - beta) for beta < 1, 1 for 1 <= beta <= 2, 1 / (beta - 1) for beta > 2                       (scikit-learn's rule)
with (l1, l2) = (l1H, l2H) in the H step and (l1W, l2W) in the W step: scikit-learn's solver="mu" up to the project's eps.  Then the normalisation: none with a
non-zero penalty; otherwise beta = 1 normalises the columns of W without rescaling H, every other beta uses the compensated form (W H unchanged).
The errors of an iteration refer to (W_{k-1}, H_k): frobenius, rmsd, and the divergence alone (no penalty terms)
    sum (v^beta + (beta - 1) P^beta - beta v P^(beta - 1)) / (beta (beta - 1)),    v^beta = 0 at v = 0
with its limits at beta = 1 and beta = 0 (beta_reference.terms)."""
import numpy as np

from tests import beta_reference as ref

planted, start, normalize = ref.planted, ref.start, ref.normalize
NO_PENALTIES = (0.0, 0.0, 0.0, 0.0)      # (l1W, l1H, l2W, l2H)


def gamma_of(beta):
    return 1.0 / (2.0 - beta) if beta < 1 else (1.0 if beta <= 2 else 1.0 / (beta - 1.0))


def half_step(X, A, B, beta, eps, l1=0.0, l2=0.0, dsum=None):
    """The update of the panel A (out x r) against B (red x r) with X (out x red) = V seen from A's side (beta_reference.half_step's arguments)."""
    if beta in (0, 1) and l1 == 0 and l2 == 0:
        return ref.half_step(X, A, B, beta, eps, dsum=dsum)
    dt = A.dtype.type
    P = A @ B.T + eps
    if beta == 1:
        num = (X / P) @ B
        den = B.sum(axis=0) if dsum is None else dsum
    elif beta == 0:
        ip = 1.0 / P
        num = (X * ip * ip) @ B
        den = ip @ B
    else:
        t = P ** dt(beta - 2.0)
        num = (X * t) @ B
        den = (t * P) @ B
    quo = num / (den + eps + dt(l1) + dt(l2) * A)
    g = gamma_of(beta)
    return A * (quo if g == 1.0 else np.sqrt(quo) if g == 0.5 else quo ** dt(g))


def terms(X, A, B, beta, eps):
    """Per row of A: sum (x - p)^2 and the divergence, with p = A B^T + eps."""
    if beta in (0, 1):
        return ref.terms(X, A, B, beta, eps)
    dt = A.dtype.type
    P = A @ B.T + eps
    tf = ((X - P) ** 2).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        xb = np.where(X > 0, np.where(X > 0, X, 1.0) ** dt(beta), 0.0)
    pm1 = P ** dt(beta - 1.0)
    return tf, ((xb + dt(beta - 1.0) * pm1 * P - dt(beta) * X * pm1) / dt(beta * (beta - 1.0))).sum(axis=1)


def divergence(V, W, H, beta, eps):
    return float(terms(V, W, H.T, beta, eps)[1].astype(np.float64).sum())


def penalty_terms(W, H, pen):
    l1W, l1H, l2W, l2H = pen
    W = W.astype(np.float64); H = H.astype(np.float64)
    return float(l1W * W.sum() + l1H * H.sum() + 0.5 * l2W * (W * W).sum() + 0.5 * l2H * (H * H).sum())


def objective(V, W, H, beta, eps, pen=NO_PENALTIES):
    """What the penalised update minimises: the divergence plus l1W |W|_1 + l1H |H|_1 + 1/2 l2W |W|^2 + 1/2 l2H |H|^2 (scikit-learn's objective)."""
    return divergence(V, W, H, beta, eps) + penalty_terms(W, H, pen)


def run(V, W0, H0, iters, beta, eps, pen=NO_PENALTIES, const_w=False, dtype=np.float64, history=False):
    """`iters` iterations from (W0, H0) with penalties pen = (l1W, l1H, l2W, l2H).  Returns (W, H, frobenius, rmsd, divergence) of the last iteration, and with
    history=True the objective (divergence + penalty terms, at (W_{k-1}, H_k)) of every iteration as a sixth entry."""
    l1W, l1H, l2W, l2H = pen
    penalised = any(p != 0 for p in pen)
    V = np.asarray(V, dtype=dtype); W = np.array(W0, dtype=dtype); H = np.array(H0, dtype=dtype)
    eps = dtype(eps)
    m, n = V.shape
    frob = rmsd = div = 0.0
    hist = []
    for it in range(1, iters + 1):
        H = half_step(V.T, H.T, W, beta, eps, l1H, l2H).T
        if history or it == iters:
            tf, td = terms(V, W, H.T, beta, eps)
            frob = float(np.sqrt(tf.astype(np.float64).sum())); rmsd = frob / np.sqrt(float(m) * n); div = float(td.astype(np.float64).sum())
            hist.append(div + penalty_terms(W, H, pen))
        if not const_w:
            W = half_step(V, W, H.T, beta, eps, l1W, l2W)
            if not penalised:
                W, H = normalize(W, H, beta != 1)
    out = (np.asfortranarray(W), np.asfortranarray(H), frob, rmsd, div)
    return out + (hist,) if history else out
