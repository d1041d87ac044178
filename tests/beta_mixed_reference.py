"""The numpy restatement of the mixed-precision dense beta-divergence update (docs/DIVERGENCE.md, "Mixed precision"), built on tests/beta_general_reference.py.

The update is the general one with exactly these roundings to bf16 (round to nearest even, by bit arithmetic on the fp32 pattern) and no others:
    the two panels A and B as operands of P = A B^T;  Q = X .* P^(beta - 2) and R = P^(beta - 1) as operands of num = Q B and den = R B (B the rounded panel).
Everything else is in the accumulation dtype given (fp64 unless asked otherwise): X unrounded, P + eps, the element-wise map, the sums, the error terms (formed
from the bf16-operand P), the denominator of beta = 1 (the column sums of the UNROUNDED B) and the update itself, which multiplies the unrounded master panel A."""
import numpy as np

from tests import beta_general_reference as gen

planted, start, normalize, gamma_of = gen.planted, gen.start, gen.normalize, gen.gamma_of
NO_PENALTIES = gen.NO_PENALTIES


def round_bf16(a):
    """Every value to the nearest bf16 (ties to even), through its fp32 bit pattern; the result has the dtype of `a`.  Finite values only."""
    a = np.asarray(a)
    bits = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return bits.astype(np.uint32).view(np.float32).reshape(a.shape).astype(a.dtype)


def _product(A, B, eps):
    return round_bf16(A) @ round_bf16(B).T + eps


def _map(X, P, beta, dt):
    """Q and R (None at beta = 1) before their rounding."""
    if beta == 1:
        return X / P, None
    if beta == 0:
        ip = 1.0 / P
        return X * ip * ip, ip
    t = P ** dt(beta - 2.0)
    return X * t, t * P


def half_step(X, A, B, beta, eps, l1=0.0, l2=0.0, dsum=None):
    """beta_general_reference.half_step with the bf16 operands."""
    dt = A.dtype.type
    Bb = round_bf16(B)
    Q, R = _map(X, _product(A, B, eps), beta, dt)
    num = round_bf16(Q) @ Bb
    if beta == 1:
        den = B.sum(axis=0) if dsum is None else dsum
    else:
        den = round_bf16(R) @ Bb
    quo = num / (den + eps + dt(l1) + dt(l2) * A)
    g = gamma_of(beta)
    return A * (quo if g == 1.0 else np.sqrt(quo) if g == 0.5 else quo ** dt(g))


def terms(X, A, B, beta, eps):
    """Per row of A: sum (x - p)^2 and the divergence, with p = bf16(A) bf16(B)^T + eps."""
    dt = A.dtype.type
    P = _product(A, B, eps)
    tf = ((X - P) ** 2).sum(axis=1)
    if beta == 1:
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(X > 0, X * np.log(np.where(X > 0, X, 1.0) / P), 0.0)
        return tf, (t - X + P).sum(axis=1)
    if beta == 0:
        ratio = X / P
        return tf, (ratio - np.log(ratio) - 1.0).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        xb = np.where(X > 0, np.where(X > 0, X, 1.0) ** dt(beta), 0.0)
    pm1 = P ** dt(beta - 1.0)
    return tf, ((xb + dt(beta - 1.0) * pm1 * P - dt(beta) * X * pm1) / dt(beta * (beta - 1.0))).sum(axis=1)


def run(V, W0, H0, iters, beta, eps, pen=NO_PENALTIES, const_w=False, dtype=np.float64, history=False):
    """beta_general_reference.run with the mixed-precision half-steps and terms; the normalisation and everything else as there."""
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
            hist.append(div + gen.penalty_terms(W, H, pen))
        if not const_w:
            W = half_step(V, W, H.T, beta, eps, l1W, l2W)
            if not penalised:
                W, H = normalize(W, H, beta != 1)
    out = (np.asfortranarray(W), np.asfortranarray(H), frob, rmsd, div)
    return out + (hist,) if history else out
