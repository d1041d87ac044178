"""Inputs of the r x r inverse tests (tests/test_inverse_cpu.py, tests/test_gpu_inverse.py) and their references, computed once per case and shared.

Kinds (seeded default_rng, nothing above 300 x 300):
  spd    W^T W with W uniform in [0, 1), max(4 r, 64) x r: the normal matrix of the least-squares algorithms;
  perm   (D + 0.1 N) with its rows rotated by one, D diagonal in [1, 2], N uniform in +-1/r: every pivot lies off the diagonal;
  exact  diag(2^e), e in [-8, 8], with its rows rotated by three: its inverse is exact in both types.
A case is (kind, r, (offdiag, diag), k): the matrix in type T times 2^k and the regulariser rounded to T times 2^k -- exact scalings, so that the regularised matrix
of scale k is 2^k times that of scale 0 bit for bit and one reference serves all scales of a case (asserted in `case`)."""
import functools

import numpy as np

from tests import inverse_reference as ref

GJ_RANKS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 40, 63, 64)          # Gauss-Jordan: the column-per-wave borders 8 | 9 (eight waves) and 16 | 17 (four)
HH_RANKS = (65, 96, 100, 128, 129, 200, 256, 300)                          # Householder as the engines reach it (route 0)
HH_SMALL_RANKS = (1, 3, 8, 64)                                             # ... and below 65, where only route 1 reaches it
REGS = ((0.0, 0.0), (-0.01, 0.5), (0.0, 0.01))
SCALES = (0, 12, 24, -24)
COND_MAX = 1e4

# (kind, regulariser, scale) run at every Gauss-Jordan rank: every regulariser, every scale on both random kinds
GJ_SET = tuple([("spd", reg, 0) for reg in REGS] + [("spd", REGS[1], k) for k in SCALES[1:]] + [("perm", REGS[0], k) for k in SCALES] +
               [("perm", REGS[1], 0), ("perm", REGS[2], 0), ("exact", REGS[0], 0)])
# ... at every Householder rank.  The perm kind stays below 65: it exists for the pivot permutation, which only Gauss-Jordan has, and at cond2 = 2 bound (a) is 32
# unit roundoffs whatever r is, while every dense inversion in double accumulates with r -- LAPACK's own residual on it is 0.4 of the bound at r = 65 and 0.75 to 1.95
# at r = 300.  Every regulariser, the launch without the fill kernel (0, 0), every scale:
HH_SET = (("spd", REGS[1], 0), ("spd", REGS[0], 12), ("spd", REGS[2], -24), ("spd", REGS[1], 24), ("exact", REGS[0], 0))
# ... from 200 on two references per rank and type (the refinement of a 300 x 300 matrix in extended precision takes over a second on the host)
HH_SET_LARGE = (("spd", REGS[1], 24), ("spd", REGS[0], 12), ("exact", REGS[0], 0))
HH_LARGE_FROM = 200
# ... and below 65 through route 1
HH_SMALL_SET = HH_SET + (("perm", REGS[0], 0), ("perm", REGS[1], 24))


def householder_cases(dtype, ranks=HH_RANKS):
    for r in ranks:
        yield from all_cases(dtype, (r,), HH_SET_LARGE if r >= HH_LARGE_FROM else HH_SET)


def _rotate_rows(M, by):
    return np.roll(M, by, axis=0)


@functools.lru_cache(maxsize=None)
def _base(kind, r):
    """The unscaled matrix in double."""
    rng = np.random.default_rng(1000 * r + {"spd": 1, "perm": 2, "exact": 3}[kind])
    if kind == "spd":
        W = rng.random((max(4 * r, 64), r))
        return W.T @ W
    if kind == "perm":
        D = np.diag(1.0 + rng.random(r))
        N = (2 * rng.random((r, r)) - 1) / r
        return _rotate_rows(D + 0.1 * N, 1)
    assert kind == "exact"
    return _rotate_rows(np.diag(2.0 ** rng.integers(-8, 9, size=r)), 3)


@functools.lru_cache(maxsize=None)
def _unscaled(kind, r, reg, dtype):
    """(A, Areg, Xref, cond) at scale 0 in type `dtype`; Xref in the extended type."""
    dt = np.dtype(dtype)
    A = np.asfortranarray(_base(kind, r).astype(dt))
    off, diag = dt.type(reg[0]), dt.type(reg[1])
    Areg = ref.regularised(A, off, diag)
    if kind == "exact":
        nz = Areg != 0
        X = np.zeros((r, r))
        X.T[nz] = 1.0 / Areg[nz].astype(np.float64)            # (P D)^-1 = D^-1 P^T: the reciprocals, transposed
        Xref = ref.lift(X)
    else:
        Xref = ref.refined_inverse(Areg)
    for a in (A, Areg):
        a.setflags(write=False)
    return A, Areg, Xref, ref.cond2(Areg)


def case(kind, r, reg, k, dtype):
    """dict(A, offdiag, diag, Areg, Xref, cond, ...) of one case; A and the regulariser are what the launch is given."""
    dt = np.dtype(dtype)
    A0, Areg0, X0, cond = _unscaled(kind, r, tuple(reg), dt.name)
    s = dt.type(2.0) ** k
    A = np.asfortranarray(A0 * s)
    off, diag = dt.type(reg[0]) * s, dt.type(reg[1]) * s
    Areg = ref.regularised(A, off, diag)
    assert A.dtype == dt and np.array_equal(Areg, Areg0 * s) and np.all(np.isfinite(Areg)) and np.array_equal(A / s, A0), "the scaling is not exact"
    Xref = X0 * ref.lift(np.float64(2.0) ** -k)                 # exact: a power of two
    A.setflags(write=False)
    return dict(kind=kind, r=r, reg=tuple(reg), k=k, dtype=dt, A=A, offdiag=float(off), diag=float(diag), Areg=Areg, Xref=Xref, cond=cond,
                name=f"{kind} r={r} reg={tuple(reg)} 2^{k} {dt.name}")


def all_cases(dtype, ranks, selection):
    for r in ranks:
        for kind, reg, k in selection:
            yield case(kind, r, reg, k, dtype)


def product_operands():
    """The product a passenger rides on: X = 2560 (sixteen x-tiles even at tile height 160), Y = 64, padded rank 64 -- small integers, so every form returns the same bits."""
    rng = np.random.default_rng(77)
    A = np.asfortranarray(rng.integers(0, 8, size=(2560, 64)).astype(np.float32))
    F = np.asfortranarray(rng.integers(-4, 5, size=(64, 64)).astype(np.float32))
    return A, F
