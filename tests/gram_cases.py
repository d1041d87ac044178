"""The cases of the Gram-matrix kernel tests (docs/GRAM.md, "Cases"): shared by tests/test_gram_cpu.py, which applies the defects to them, and by the
tests/test_gpu_gram_*.py modules, which run them.  Every case is built from its own seed; nothing here touches a device.

Data kinds.  `random`: signed, held to the bounds.  The others are EXACT -- every partial sum is an fp32 value in any order -- and compared as bits:
  ints     integers in [-3, 3]: |sum| <= 9 * len < 2^24
  pow2     four values +-2^e(c) per column (one where the panel is shorter): the sum of squares is 4^(e + 1), the scale 2^-(e + 1), both scaling products exact
  planes   one pair of columns per panel row; the lower column holds (1 + 2^-9 + 2^-18) 2^e, the upper (1 + 2^-10 + 2^-20) 2^e': the planes are single bits and
           each of the six kept terms of their product is a bit of its own (2^0, 2^-9, 2^-10, 2^-18, 2^-19, 2^-20 times 2^(e + e')), the three dropped ones lie
           below the last bit (2^-28, 2^-29, 2^-38).  An element that at most PLANES_EXACT_ROWS panel rows contribute to is exact in any order of summation
           (multiples of 2^-20 below 2 * 8: 24 bits); exact_mask() says which."""
import zlib

import numpy as np

IMAGE_LENS = (1, 15, 16, 17, 31, 32, 33, 48, 100, 127, 128, 129, 225, 257, 1301)       # (225: pairs = 8, the spread form's exact deal of five pairs per workgroup)
WIDE_LENS = (1, 16, 17, 63, 64, 65, 127, 128, 129, 1000)
COLSQ_PARTS = (1, 7, 8, 9, 40, 41, 316, 320, 321, 400)
REDUCE_PARTS = (1, 2, 3, 8, 9, 16, 17)
WIDE_PARTS = (1, 3, 16, 128)
WIDE_SQ_PARTS = (1, 2, 3, 4, 5, 9, 33)
WIDE_RP = (128, 256, 384)
IMAGE_FORMS = ("one", "ksplit2", "ksplit4", "ksplit8", "spread", "spread_finish")
KINDS = ("random", "ints", "pow2", "planes")
PLANES_EXACT_ROWS = 8
A_PLANES = 1.0 + 2.0 ** -9 + 2.0 ** -18
B_PLANES = 1.0 + 2.0 ** -10 + 2.0 ** -20


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _pairs(r):
    return [(a, b) for a in range(r) for b in range(a + 1, r)]


def panel(kind, length, r, RP=64, zero_col=None, seed=0):
    """A [length][RP] fp32 panel with r valid columns (the others zero) and optionally one valid column zeroed."""
    rng = _rng("panel", kind, length, r, RP, seed)
    P = np.zeros((length, RP), np.float32)
    if kind == "random":
        P[:, :r] = rng.standard_normal((length, r)) * np.exp(rng.uniform(-2, 2, (1, r)))
    elif kind == "ints":
        P[:, :r] = rng.integers(-3, 4, (length, r))
    elif kind == "pow2":
        e = rng.integers(-6, 7, r)
        k = 4 if length >= 4 else 1
        for c in range(r):
            rows = rng.choice(length, k, replace=False)
            P[rows, c] = rng.choice([-1.0, 1.0], k) * 2.0 ** e[c]
    elif kind == "planes":
        e = rng.integers(-4, 5, r)
        pr = _pairs(r)
        for y in range(length):
            if r == 1:          # (one column: PLANES_EXACT_ROWS rows of it at the most)
                if y % -(-length // PLANES_EXACT_ROWS) == 0:
                    P[y, 0] = A_PLANES * 2.0 ** e[0]
                continue
            a, b = pr[(y + 31 * seed) % len(pr)]
            P[y, a] = A_PLANES * 2.0 ** e[a]
            P[y, b] = B_PLANES * 2.0 ** e[b]
    else:
        raise ValueError(kind)
    if zero_col is not None and zero_col < r:
        P[:, zero_col] = 0
    return P


def exact_mask(kind, P):
    """Which elements of P^T P (and of every slice of it) are exact in fp32 in any order of summation."""
    C = P.shape[1]
    if kind in ("ints", "pow2"):
        return np.ones((C, C), bool)
    if kind == "planes":
        nz = (P != 0).astype(np.int64)
        return (nz.T @ nz) <= PLANES_EXACT_ROWS
    return np.zeros((C, C), bool)


def colsq(kind, parts, r, RP=64, zero_col=None, seed=0):
    """A caller-built [parts][RP] array of partial sums of squares, independent of any panel.  random: positive; the exact kinds: every column sums to a power of
    four in any order (the value 4^e / 4 in four parts -- the first, the last and two between, so that every batch of the kernels' sums holds one -- or 4^e in the
    one part there is)."""
    rng = _rng("colsq", kind, parts, r, RP, seed)
    Q = np.zeros((parts, RP), np.float32)
    if kind == "random":
        Q[:, :r] = rng.uniform(0.1, 2.0, (parts, r)) * np.exp(rng.uniform(-2, 2, (1, r)))
    else:
        e = rng.integers(-5, 6, r)
        if parts >= 4:
            where = sorted({0, parts // 3, (2 * parts) // 3, parts - 1})
            assert len(where) == 4
            for c in range(r):
                Q[where, c] = 4.0 ** e[c] / 4
        else:
            Q[0, :r] = 4.0 ** e
    if zero_col is not None and zero_col < r:
        Q[:, zero_col] = 0
    return Q


def partial_matrices(kind, parts, seed=0, C=64, r=None):
    """Caller-built [parts][C][C] symmetric partial Gram matrices with a positive diagonal.  Exact kinds: small integers (any order of summation exact); with pow2
    the diagonal of the SUM is a power of four (the scales and both scaling products are exact)."""
    rng = _rng("partials", kind, parts, seed, C, r)
    r = C if r is None else r
    M = np.zeros((parts, C, C), np.float32)
    if kind == "random":
        for p in range(parts):
            X = rng.standard_normal((8, r))
            M[p, :r, :r] = X.T @ X
        return M
    A = rng.integers(-4, 5, (parts, r, r))
    A = np.triu(A, 1)
    M[:, :r, :r] = A + A.transpose(0, 2, 1)
    d = np.arange(r)
    if kind == "pow2":
        e = rng.integers(0, 5, r)
        M[:, d, d] = 0
        M[rng.integers(0, parts, r), d, d] = 4.0 ** e
    else:
        M[:, d, d] = rng.integers(1, 9, (parts, r))
    return M


def image_cases():
    """(id, dict) of the rank-64 image cases: len x (r, kind, zero column); every form runs each of them."""
    out = []
    for n in IMAGE_LENS:
        out.append((f"len{n}-r64-random", dict(length=n, r=64, kind="random", zero_col=None)))
        out.append((f"len{n}-r64-ints", dict(length=n, r=64, kind="ints", zero_col=None)))
    for n in (17, 33, 100, 257, 1301):
        out.append((f"len{n}-r64-planes", dict(length=n, r=64, kind="planes", zero_col=None)))
        out.append((f"len{n}-r61-pow2-zero5", dict(length=n, r=61, kind="pow2", zero_col=5)))
    out.append(("len48-r1-planes", dict(length=48, r=1, kind="planes", zero_col=None)))
    out.append(("len129-r1-random", dict(length=129, r=1, kind="random", zero_col=None)))
    out.append(("len100-r61-random-zero17", dict(length=100, r=61, kind="random", zero_col=17)))
    return out


def image_colsq_cases():
    """(id, dict): the part counts of the scale sums on one short panel; 400 parts also with exact data."""
    out = [(f"colsq{p}-random", dict(parts=p, kind="random", zero_col=None)) for p in COLSQ_PARTS]
    out += [(f"colsq{p}-pow2-zero9", dict(parts=p, kind="pow2", zero_col=9)) for p in (1, 9, 41, 321, 400)]
    return out


def wide_cases():
    """(id, dict) of the padded ranks' cases: every len at RP 128 with the slice counts, the other ranks on fewer."""
    out = []
    for n in WIDE_LENS:
        for parts in WIDE_PARTS:
            if parts in (3, 128) and n not in (64, 65, 129, 1000):
                continue
            out.append((f"rp128-len{n}-parts{parts}-random", dict(RP=128, length=n, r=128, parts=parts, kind="random", zero_col=None)))
        out.append((f"rp128-len{n}-parts16-ints", dict(RP=128, length=n, r=125, parts=16, kind="ints", zero_col=None)))
    for RP in (256, 384):
        for n, parts in ((17, 16), (129, 3), (1000, 128)):
            out.append((f"rp{RP}-len{n}-parts{parts}-random", dict(RP=RP, length=n, r=RP - 3, parts=parts, kind="random", zero_col=7)))
        out.append((f"rp{RP}-len257-parts16-planes", dict(RP=RP, length=257, r=RP, parts=16, kind="planes", zero_col=None)))
        out.append((f"rp{RP}-len65-parts16-ints-r1", dict(RP=RP, length=65, r=1, parts=16, kind="ints", zero_col=None)))
    out.append(("rp512-len129-parts16-random", dict(RP=512, length=129, r=509, parts=16, kind="random", zero_col=None)))
    return out
