"""Inputs of the panel-update tests (tests/test_panel_update_cpu.py, tests/test_gpu_panel_update.py, tests/test_gpu_mu64_update.py) and the comparisons they share.

Two kinds of case:
  exact   small integers and powers of two on which every product and every partial sum of the kernels is an integer below 2^24 (exact in float32 whatever the
          order of summation) and every operand of an r x r product fits one bf16 plane (exact on the split-operand forms too).  Q has entries 1 .. 31 that change
          with every step along a row and along a column and is not symmetric (Q[k, c] = Q[c, k] only where 31 divides c - k); the 32-column rank-64 kernel, which
          reads its operand by rows, gets the symmetric counterpart.  MODE_LS gets signs (so that the clamp works) and a numerator with eight entries per row whose
          positions walk through every K index with the row index; MODE_MU gets dense numerators and old values that are powers of two.
  random  non-negative uniform data at the engines' eps.
Rank rows from r on are zero in every operand, panel rows from len_valid on are zero, and the gaps between the slabs hold NaN."""
import numpy as np

GAP = 96          # elements between two slabs that no kernel may read
# What the GPU modules run the panel update at, (len_pad, len_valid, S): one and three workgroups of every form; len_valid 1, mid-tile, len_pad - 1, len_pad; S 1, 2,
# 8, 9 and 18 -- past the second batch of every form (batches of 3 in k_panel_update_wide_f32, 5 in k_panel_update64_lds_f32, up to 8 in the fp64 kernels)
SHAPES = [(128, 128, 1), (128, 1, 2), (128, 77, 8), (384, 383, 9), (384, 200, 18)]
RANKS = {64: 33, 128: 128, 192: 150, 256: 200, 320: 320, 384: 257, 448: 400, 512: 512}       # padded rank -> the rank the cases fill


def worst_ratio(got, want, bound):
    """max |got - want| / bound; an element with a zero bound must be met exactly."""
    err = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64))
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    if err.size == 0:
        return 0.0
    if not np.all(np.isfinite(err)):
        return np.inf
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    return float(ratio.max())


def same_bits(got, want, dtype):
    """The launch returned the restatement's values rounded to dtype (which on the exact cases is no rounding), no NaN among them."""
    want = np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and not np.any(np.isnan(got)) and np.array_equal(np.asarray(got, dtype=np.float64), want.astype(dtype).astype(np.float64))


def to_bf16(x):
    """Round-to-nearest-even to bf16, returned as float32."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def exact_q(RP, r, *, signed=False, symmetric=False):
    k, c = np.meshgrid(np.arange(RP), np.arange(RP), indexing="ij")
    Q = 1.0 + ((k + c + 11 * (((k ^ c) >> 1) & 1)) % 31 if symmetric else (k + 5 * c) % 31)
    if signed:
        Q = np.where(((k + c) if symmetric else (3 * k + c)) % 7 < 2, -Q, Q)
    Q[r:, :] = 0
    Q[:, r:] = 0
    return Q


def pack_slabs(parts, dtype):
    """(S, len_pad, RP) -> the (S, stride) array the launches take, NaN in the gaps."""
    S = parts.shape[0]
    flat = parts.reshape(S, -1)
    out = np.full((S, flat.shape[1] + GAP), np.nan, dtype=dtype)
    out[:, :flat.shape[1]] = flat
    return out


def exact_case(mode, RP, r, len_pad, len_valid, S, dtype, *, symmetric=False):
    """dict(P, slabs, Q): see the module docstring."""
    y, c = np.meshgrid(np.arange(len_pad), np.arange(RP), indexing="ij")
    live = (y < len_valid) & (c < r)
    parts = np.zeros((S, len_pad, RP))
    if mode == "mu":
        P = np.where(live, 2.0 ** ((3 * y + 5 * c) % 4), 0.0)
        for s in range(S):
            parts[s] = np.where(live, (y + 2 * c + s) % 3, 0)
    else:
        P = np.where(live, 7.0, 0.0)          # (MODE_LS and MODE_SET do not read the old values)
        # eight entries per row at columns 8 y + 5 j (mod r): 5 j runs through every residue of 8, so the rows between them reach every K index once 8 len_valid
        # exceeds r + 35 (every shape of the GPU modules with more than one valid row); two of the eight count twice, each unit goes to a slab of its own turn
        for yy in range(len_valid):
            for j in range(8):
                col = (8 * yy + 5 * j) % r
                for i in range(2 if (yy + j) % 4 == 0 else 1):
                    parts[(yy + j + i) % S, yy, col] += 1
    return {"P": P.astype(dtype), "slabs": pack_slabs(parts, dtype), "Q": exact_q(RP, r, signed=(mode == "ls"), symmetric=symmetric).astype(dtype), "exact": True,
            "RP": RP, "r": r, "len_pad": len_pad, "len_valid": len_valid, "S": S}


def random_case(mode, RP, r, len_pad, len_valid, S, dtype, seed, *, symmetric=False):
    rng = np.random.default_rng([seed, RP, r, len_pad, len_valid, S])
    y, c = np.meshgrid(np.arange(len_pad), np.arange(RP), indexing="ij")
    live = (y < len_valid) & (c < r)
    P = np.where(live, 0.1 + rng.random((len_pad, RP)), 0.0)
    parts = np.where(live[None], rng.random((S, len_pad, RP)), 0.0)
    Q = rng.random((RP, RP))
    if symmetric:
        Q = (Q + Q.T) / 2
    if mode == "ls":
        Q = Q - 0.5
    Q[r:, :] = 0
    Q[:, r:] = 0
    return {"P": P.astype(dtype), "slabs": pack_slabs(parts, dtype), "Q": Q.astype(dtype), "exact": False, "RP": RP, "r": r, "len_pad": len_pad,
            "len_valid": len_valid, "S": S}


def make_case(kind, mode, RP, r, len_pad, len_valid, S, dtype, *, symmetric=False, seed=0):
    if kind == "exact":
        return exact_case(mode, RP, r, len_pad, len_valid, S, dtype, symmetric=symmetric)
    return random_case(mode, RP, r, len_pad, len_valid, S, dtype, seed, symmetric=symmetric)


def tiny_row(case):
    """The case with the old values of row 0 all but zero (2^-100 on the exact cases, 1e-30 otherwise): the denominator of that row vanishes against eps, so the
    row is old * num / eps -- the one place where a multiplicative update without its eps gives other finite values."""
    out = dict(case)
    P = case["P"].copy()
    P[0, :case["r"]] = 2.0 ** -100 if case["exact"] else 1e-30
    out["P"] = P
    return out


def scale_vector(kind, r, dtype, seed=0):
    """The pending column scale of the rank-64 and fused forms: powers of two on the exact cases, (0.5, 1.5) otherwise; ones from r on."""
    s = np.ones(64 if r <= 64 else r)
    if kind == "exact":
        s[:r] = 2.0 ** ((np.arange(r) % 3) - 1)
    else:
        s[:r] = 0.5 + np.random.default_rng([seed, r]).random(r)
    return s.astype(dtype)


def slices_of(Q, qsplit, kind):
    """qsplit symmetric slices that add up to Q: integers on the exact cases (floor((Q + i) / qsplit) sums to Q over i), random shares otherwise."""
    if qsplit <= 1:
        return Q
    if kind == "exact":
        return np.stack([np.floor((Q + i) / qsplit) for i in range(qsplit)]).astype(np.float32)
    w = np.random.default_rng(qsplit).random((qsplit, 64, 64))
    w = w + w.transpose(0, 2, 1)
    return (Q[None] * w / w.sum(axis=0)).astype(np.float32)


def gprev_of(kind, r):
    """The W side's second trace operand: integers on the exact cases."""
    return exact_q(64, r).astype(np.float32) if kind == "exact" else np.random.default_rng(r).random((64, 64)).astype(np.float32)


def scaled_exactness_report(case, scale, Q_slices, Gprev):
    """The same promise for what the rank-64 and fused exact cases add to the plain ones: a power-of-two scale on the old values (W side) or on the numerator
    (H side), integer slices of Q added and scaled on both sides, the integer trace operand.  With scales 1/2, 1, 2 every value is a multiple of 1/4: `quarters`
    says that four times every product and partial sum is an integer, `largest` is four times the largest magnitude (below 2^24: exact in any order)."""
    RP, len_pad = case["RP"], case["len_pad"]
    P = case["P"].astype(np.float64)
    s = np.asarray(scale, dtype=np.float64)[:RP]
    slabs = case["slabs"][:, :len_pad * RP].astype(np.float64).reshape(-1, len_pad, RP)
    num = slabs.sum(axis=0)
    Qs = np.asarray(Q_slices, dtype=np.float64).reshape(-1, RP, RP)
    partial = np.cumsum(np.abs(Qs), axis=0)
    Qsum = Qs.sum(axis=0)
    Qf = (Qsum * s[None, :]) * s[:, None]
    values = [s, partial, Qsum * s[None, :], Qf, P * s, num * s, (P * s) @ np.abs(Qsum), P @ np.abs(Qf), (P * s) * num, P * (num * s)]
    if Gprev is not None:
        values.append((np.abs(Qsum) * np.abs(np.asarray(Gprev, dtype=np.float64)).T).sum(axis=0))
    operands = [s, Qsum, Qf, P * s, P]
    return {"largest": 4 * max(float(np.abs(v).max()) for v in values), "quarters": all(np.array_equal(4 * v, np.round(4 * v)) for v in values),
            "powers_of_two": bool(np.all(np.log2(s) == np.round(np.log2(s)))), "symmetric_slices": all(np.array_equal(q, q.T) for q in Qs),
            "one_plane": all(np.array_equal(to_bf16(o), o.astype(np.float32)) for o in operands)}


def exactness_report(case, mode, part_rows=128):
    """What the exact cases promise, as numbers a test can assert on: the largest magnitude any product or partial sum of the update can reach (every operand
    taken by absolute value, so every partial sum in any order is below it), whether all of them are integers, and whether the operands of the r x r product fit
    one bf16 plane."""
    RP, len_pad = case["RP"], case["len_pad"]
    P, Q = case["P"].astype(np.float64), case["Q"].astype(np.float64)
    slabs = case["slabs"][:, :len_pad * RP].astype(np.float64).reshape(-1, len_pad, RP)
    num = np.abs(slabs).sum(axis=0)
    values = [P, Q, slabs, num]
    if mode == "mu":
        den = np.abs(P) @ np.abs(Q)
        values += [den, np.abs(P) * num]
        operands = [P, Q]
    else:
        new = num @ np.abs(Q) if mode == "ls" else num
        values += [new, (new * num).sum(axis=1), (new ** 2).reshape(len_pad // part_rows, part_rows, RP).sum(axis=1)]
        if RP == 64:
            b = new.reshape(-1, 64, 64)
            values.append(np.einsum("bya,byc->bac", b, b))
        operands = [num, Q]
    return {"largest": max(float(np.abs(v).max()) for v in values), "integers": all(np.array_equal(v, np.round(v)) for v in values),
            "one_plane": all(np.array_equal(to_bf16(o), o.astype(np.float32)) for o in operands)}
