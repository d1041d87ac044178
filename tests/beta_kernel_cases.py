"""The cases of the kernel-level tests of the dense beta-divergence half-step (tests/test_gpu_beta_fused.py, tests/test_gpu_beta_update.py; the device-free
tests/test_beta_kernel_cpu.py runs its defect checks on the same ones): the smallest shapes that still meet every mechanism of the kernels.

Shapes: out_pad 128 or 256 (one and two update workgroups; four and eight output blocks at bo = 32, 16 and 32 in fp64), red_pad 384 (three fp32 tiles at RP <= 128,
six at RP 256, twelve in fp64: with two or three slabs they come out uneven -- at RP <= 128 three slabs of one tile, two slabs of two and one).

Three kinds of data.
  random   the project's planted V and 1 - random panels (tests/beta_reference.py), weights with 30 % zeros.
  exact    bit for bit at beta in {0, 1}:
           a  A one-hot per row with value 2 or 4, B with entries in {1, 2, 4} that change along every row and column, X integers 1 .. 8.  P is a power of two
              >= 2, so P + eps rounds back to P (a tie to even at 2, below half an ulp above), Q and R are dyadic and every partial sum is a small multiple of
              2^-8: any order of summation gives the same bits.
           b  (beta = 1) A and B integers 2 .. 4 in every entry, X = Z o (A B^T) with Z in 1 .. 4: a dense first product, and Q = Z exactly.
           c  X one-hot per output row on the operands of a: num(o, :) is one scaled row of B -- the K index of the accumulator map, read off directly.
           Weights are 1/2, 1, 2 or 0.  Every operand fits bf16, so the mixed launch is held to the same bits.  quantum(), sums_are_exact() and fits() state these claims as numbers (tests/test_beta_kernel_cpu.py).
  tiny     (on random and a) the old values of output row 0 are 1e-30 / 2^-100 (float64: 1e-60 / 2^-200): P + eps = eps and Q = X / eps, the one place where a missing eps shows.
The update launch's cases are built the same way: random partial panels, or integers whose slab sums are powers of two (the quotient is 4^e, the square root
2^e), a denominator column of zeros (den + eps = eps), and penalties l1 = 32, l2 = 8 against denominators 2^j - 32 - 8 a.

X, Omega and the partial panels hold NaN on every position the launches must not read: rows >= out_valid, columns >= red_valid, rank columns >= r."""
import numpy as np

from tests import beta_reference as ref
from tests import weighted_reference as wref
from tests.panel_update_cases import same_bits, worst_ratio      # noqa: F401  (shared helpers)

RED_PAD = 384
OUT_VALID = [(128, 1), (128, 32), (128, 33), (128, 127), (128, 128), (256, 129)]       # (out_pad, out_valid)
RED_VALID = [1, 3, 4, 5, 31, 32, 33, 127, 128, 129, 384]
GENERAL_BETAS = [-1.0, 0.5, 1.5, 2.0, 3.0]      # the general map and the three gamma branches; -1 is the largest |beta - 2|
FORMS = [("plain", "float32"), ("plain", "float64"), ("weighted", "float32"), ("weighted", "float64"), ("mixed", "float32")]
RANKS = [64, 128, 256]
OUTPUTS = ["update", "update+terms", "terms"]


def ranks_of(RP):
    return [1, RP - 3, RP]


def shape_for(i):
    """The i-th combination of (out_pad, out_valid, red_valid, force_slabs, ldx): a walk through the three lists with coprime steps, so that a few dozen calls meet
    every value of each with several of the others; every ninth has ldx > red_pad."""
    out_pad, ov = OUT_VALID[i % len(OUT_VALID)]
    return out_pad, ov, RED_VALID[(5 * i + i // 6) % len(RED_VALID)], (i + i // 4) % 4, RED_PAD + 16 if i % 9 == 4 else RED_PAD


def _grids(rows, cols):
    return np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")


def fused_case(kind, form, dtype, RP, r, out_pad, out_valid, red_valid, *, ldx=RED_PAD, seed=0, tiny=False, nan_padding=True):
    """dict(A, B, X, Omega, ...) for op_beta_fused.  kind: random, a, b, c."""
    dt = np.dtype(dtype).type
    ov, rv = out_valid, red_valid
    o, k = _grids(out_pad, ldx)
    valid = (o < ov) & (k < rv)
    A = np.zeros((out_pad, RP)); B = np.zeros((RED_PAD, RP)); X = np.zeros((out_pad, ldx)); Om = None
    ko, kc = _grids(RED_PAD, RP)
    oo, oc = _grids(out_pad, RP)
    if kind == "random":
        rng = np.random.default_rng([seed, RP, r, ov, rv])
        X[:ov, :rv] = ref.planted(ov, rv, seed=seed + 1)
        A[:ov, :r] = 1.0 - rng.random((ov, r))
        B[:rv, :r] = 1.0 - rng.random((rv, r))
        if form == "weighted":
            Om = np.zeros((out_pad, ldx))
            Om[:ov, :rv] = wref.weights(ov, rv, seed + 2)
        if tiny:
            A[0, :r] = 1e-30 if dt == np.float32 else 1e-60
    else:
        Bv = 2.0 ** ((ko + 2 * kc + (ko >> 2)) % 3)
        if kind == "b":
            A = np.where((oo < ov) & (oc < r), 2.0 + (oo + oc) % 3, 0.0)
            B = np.where((ko < rv) & (kc < r), 2.0 + (ko + 2 * kc + (ko >> 2)) % 3, 0.0)
            Z = 1.0 + (o + 3 * k + (k >> 3)) % 4
            X = np.where(valid, Z[:, :ldx] * np.pad(A @ B.T, ((0, 0), (0, ldx - RED_PAD))), 0.0)
        else:
            hot = (7 * np.arange(out_pad) + 3) % r
            A[np.arange(ov), hot[:ov]] = np.where(np.arange(ov) % 2 == 1, 2.0, 4.0)
            B = np.where((ko < rv) & (kc < r), Bv, 0.0)
            if kind == "a":
                X = np.where(valid, 1.0 + (3 * o + 5 * k + (k >> 3)) % 8, 0.0)
            else:
                X[np.arange(ov), (5 * np.arange(ov) + 1) % rv] = 4.0
            if tiny:
                A[0, hot[0]] = 2.0 ** (-100 if dt == np.float32 else -200)
        if form == "weighted":
            Om = np.where(valid & ((o + 2 * k) % 5 != 0), 2.0 ** ((o + k) % 3 - 1), 0.0)
    if Om is not None:
        X = np.where(valid & (Om == 0), np.nan, X)      # a weight of 0 hides whatever X holds
    if nan_padding:
        X = np.where(valid, X, np.nan)
        if Om is not None:
            Om = np.where(valid, Om, np.nan)
    return {"kind": kind, "form": form, "exact": kind != "random", "A": A.astype(dt), "B": B.astype(dt), "X": X.astype(dt), "Omega": None if Om is None else Om.astype(dt),
            "RP": RP, "r": r, "out_pad": out_pad, "out_valid": ov, "red_valid": rv, "ldx": ldx, "dtype": dt, "tiny": tiny}


def quantum(a):
    """The largest power of two that divides every entry of a (1 for an all-zero array)."""
    a = np.abs(np.asarray(a, dtype=np.float64))
    a = a[(a != 0) & np.isfinite(a)]
    if a.size == 0:
        return 1.0
    m, e = np.frexp(a)
    mi = (m * 2.0 ** 53).astype(np.int64)
    low = mi & -mi
    return float(2.0 ** (np.log2(low.astype(np.float64)) + e - 53).min())


def sums_are_exact(terms, other, dtype):
    """Every partial sum of sum_k terms(o, k) other(k, c), in any order, is exact in dtype: row by row the products are multiples of one quantum and the sum of
    their magnitudes stays below 2^(mantissa bits) quanta."""
    bits = 24 if np.dtype(dtype) == np.float32 else 53
    qo = quantum(other)
    mag = np.abs(terms) @ np.abs(other)
    for row in range(terms.shape[0]):
        if mag[row].max(initial=0.0) / (quantum(terms[row]) * qo) >= 2.0 ** bits:
            return False
    return True


def fits(a, dtype):
    a = np.asarray(a, dtype=np.float64)
    return bool(np.array_equal(a.astype(dtype).astype(np.float64), a))


def update_case(kind, dtype, RP, r, out_pad, out_valid, S, beta, *, penalised=False, zero_den=False, vec=None, seed=0):
    """dict(P, num_part, den, terms, l1, l2) for op_beta_update.  vec: den as the RP values of dsum (default: at beta = 1).  zero_den: one denominator column of
    zeros.  P holds 7 on the padding, the partial panels NaN."""
    dt = np.dtype(dtype).type
    vec = (beta == 1) if vec is None else vec
    o, c = _grids(out_pad, RP)
    live = (o < out_valid) & (c < r)
    c0 = r // 2
    if kind == "random":
        rng = np.random.default_rng([seed, RP, r, out_valid, S])
        P = 0.1 + rng.random((out_pad, RP))
        num = rng.random((S, out_pad, RP))
        den = 0.5 + rng.random((S, out_pad, RP))
        dsum = 0.5 + S * rng.random(RP)
        tf, td = rng.random((S, out_pad)), rng.random((S, out_pad)) - 0.5
        l1, l2 = (0.05, 0.5) if penalised else (0.0, 0.0)
    else:
        s = np.arange(S)[:, None, None]
        P = 2.0 ** ((3 * o + 5 * c) % 4)
        l1, l2 = (32.0, 0.0 if vec else 8.0) if penalised else (0.0, 0.0)      # (a vector of denominators cannot follow l2 a)
        j = (7 if penalised else 5) + ((c if vec else o + c) % 3)
        e = (o + 2 * c) % 3
        num = 1.0 + (s + o[None] + c[None]) % 3
        den = 1.0 + (s + o[None]) % 2 + 0.0 * c[None]
        total_den = 2.0 ** j - l1 - (0.0 if vec else l2 * P)
        num[0] += 2.0 ** (j + 2 * e) - num.sum(axis=0)
        den[0] += total_den - den.sum(axis=0)
        dsum = 2.0 ** ((7 if penalised else 5) + np.arange(RP) % 3) - l1
        tf = 1.0 + (np.arange(S)[:, None] + 3 * np.arange(out_pad)[None, :]) % 7
        td = tf - 4.0
    if zero_den:
        den[:, :, c0] = 0.0
        dsum[c0] = 0.0
        if kind != "random":
            num[:, :, c0] = 1.0
            num[0, :, c0] = 16.0 - (S - 1)
    P = np.where(live, P, 7.0)
    num = np.where(live[None], num, np.nan)
    den = np.where(live[None], den, np.nan)
    dsum = np.where(np.arange(RP) < r, dsum, np.nan)
    return {"kind": kind, "exact": kind != "random", "P": P.astype(dt), "num_part": num.astype(dt), "den": (dsum if vec else den).astype(dt), "terms": (tf.astype(dt), td.astype(dt)),
            "l1": l1, "l2": l2, "RP": RP, "r": r, "out_pad": out_pad, "out_valid": out_valid, "S": S, "beta": beta, "dtype": dt, "zero_den_column": c0 if zero_den else None}


def beta_of(betakind, i):
    return {"kl": 1.0, "is": 0.0}.get(betakind, GENERAL_BETAS[i % len(GENERAL_BETAS)])


def fused_calls(form, dtype, RP, betakind, outputs):
    """What the GPU module runs for one instantiation of the fused launch, as keyword dicts for fused_case plus beta and force_slabs.  Every instantiation gets a
    random case on a walking shape, a random case with the whole reduction range (the last tile of every slab holds data) and, at beta in {0, 1}, exact case a;
    the update + terms instantiations add the tiny row, the update-only ones exact case c and, at beta = 1, b.  The general instantiations walk through
    GENERAL_BETAS, the tiny row and the full-range case run at -1 (the largest |beta - 2|)."""
    i = (FORMS.index((form, dtype)) * 27 + RANKS.index(RP) * 9 + ["kl", "is", "general"].index(betakind) * 3 + OUTPUTS.index(outputs))
    ranks = ranks_of(RP)
    out_pad, ov, rv, fs, ldx = shape_for(i)
    calls = [dict(kind="random", r=ranks[i % 3], out_pad=out_pad, out_valid=ov, red_valid=rv, ldx=ldx, force_slabs=fs, beta=beta_of(betakind, i), seed=i)]
    full = (256, 129) if i % 2 else (128, 127)
    calls.append(dict(kind="random", r=RP - 3, out_pad=full[0], out_valid=full[1], red_valid=RED_PAD, ldx=RED_PAD, force_slabs=1 + i % 3, beta=beta_of(betakind, 0), seed=i + 1))
    if betakind != "general":
        out_pad, ov, rv, fs, ldx = shape_for(i + 7)
        calls.append(dict(kind="a", r=ranks[(i + 1) % 3], out_pad=out_pad, out_valid=ov, red_valid=rv, ldx=ldx, force_slabs=fs, beta=beta_of(betakind, i)))
        calls.append(dict(kind="a", r=RP, out_pad=128, out_valid=128, red_valid=RED_PAD, ldx=RED_PAD, force_slabs=1 + (i + 1) % 3, beta=beta_of(betakind, i)))
    if outputs == "update+terms":
        calls.append(dict(kind="random", r=RP - 3, out_pad=128, out_valid=33, red_valid=129, ldx=RED_PAD, force_slabs=i % 3, beta=beta_of(betakind, 0), seed=i + 2, tiny=True))
        if betakind != "general":
            calls.append(dict(kind="a", r=RP - 3, out_pad=128, out_valid=33, red_valid=129, ldx=RED_PAD, force_slabs=i % 3, beta=beta_of(betakind, i), tiny=True))
    if outputs == "update" and betakind != "general":
        calls.append(dict(kind="c", r=RP, out_pad=128, out_valid=127, red_valid=RED_PAD, ldx=RED_PAD, force_slabs=2, beta=beta_of(betakind, i)))
        if betakind == "kl":
            calls.append(dict(kind="b", r=RP - 3, out_pad=128, out_valid=127, red_valid=RED_PAD - 1, ldx=RED_PAD, force_slabs=3, beta=1.0))
    return calls


UPDATE_BETAS = [1.0, 0.0] + GENERAL_BETAS
UPDATE_SLABS = [1, 2, 3, 16]


def update_calls(dtype, RP, beta, outputs):
    """What the GPU module runs for one combination of the update launch, as keyword dicts for update_case plus `weighted`: a random and an exact case on walking
    shapes and slab counts, a penalised pair (the EXT launch; exact only where the quotient is exact: gamma 1 or 1/2), and a zero denominator column."""
    i = (["float32", "float64"].index(dtype) * 63 + RANKS.index(RP) * 21 + UPDATE_BETAS.index(beta) * 3 + OUTPUTS.index(outputs))
    ranks = ranks_of(RP)
    exact_ok = beta in (0.0, 1.0, 1.5, 2.0, 3.0)        # gamma = 1 or 1/2: the quotient 4^e and its root are exact (-1 and 0.5 have gamma 1/3 and 2/3)
    calls = []
    for j, kind in enumerate(["random", "exact"] if exact_ok else ["random"]):
        out_pad, ov = OUT_VALID[(i + 3 * j) % len(OUT_VALID)]
        calls.append(dict(kind=kind, r=ranks[(i + j) % 3], out_pad=out_pad, out_valid=ov, S=UPDATE_SLABS[(i + j) % 4], weighted=(i + j) % 5 == 0 and beta != 1))
        calls.append(dict(kind=kind, r=RP - 3, out_pad=256, out_valid=129, S=UPDATE_SLABS[(i + j + 1) % 4], penalised=True, weighted=(i + j) % 2 == 1, vec=False if (i + j) % 2 == 1 else None))
    calls.append(dict(kind="exact" if beta in (1.0, 1.5, 2.0) else "random", r=ranks[(i + 1) % 3], out_pad=128, out_valid=127, S=UPDATE_SLABS[(i + 2) % 4], zero_den=True))
    return calls
