"""Case builders of the sparse KL kernel tests, shared by tests/test_sparse_kl_cpu.py (no device) and tests/test_gpu_sparse_kl_ops.py.

Two kinds of case.  "exact": inputs that make every operation of a launch exact in float32 (hence in float64), so the launch must return the bits of the
restatement whatever its order -- the builder PROVES that on the spot (the assertions in _prove_gather_exact / update_case) instead of trusting the recipe.
"random": nonnegative random data (signed values for the SpMM) for the arithmetic bounds of tests/sparse_kl_reference.py.

Every image holds rows of the lengths ROW_LENGTHS -- the edges of k_kl_fused's trip of 8 entries and of k_spmm_rows' chunk of 64 with its 4-way unrolled body --
as far as it has rows for them (an image of 1 row has one of 65 entries, one of 5 rows has 0, 9, 65, 130, 1), and: the first and the last valid row of the
gathered panel as indices, a row with a duplicated index, a stored explicit zero and (images of more than one row) an output row whose row of A is all zero, where
the quotient is x / eps.  Rows of the gathered panel that no index refers to, the rows beyond its last valid row among them, and the rows of A beyond `rows` hold
NaN.  Padding columns (c >= r) are zero in A, B and P: the kernels' contract.  Built once per parameter set and shared: the arrays are read-only."""
import functools

import numpy as np

from tests import sparse_kl_reference as ref

ROW_LENGTHS = (0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 130)
RANKS = {64: (1, 63, 64), 128: (65, 128), 256: (129, 255)}          # valid ranks per padded rank
ROWS = ((1, 128), (5, 128), (127, 128), (128, 128), (130, 256))      # (rows, rows_pad)
GATHER_VALID, GATHER_PAD = 300, 384                                  # rows of the gathered panel: valid, allocated
BLOCKED_RANGE, BLOCKED_PAD = 40, 128                                 # the blocked form gathers from a short range, so that blocks stay empty
BLOCKS = (2, 3, 8, 16)                                               # 2, 3: block-major mapping; 8, 16: the per-XCD mapping (blocks % 8 == 0)
# referenced rows of the short range: 25 ... 38 are never referenced (blocks 5, 6 of 8 and 9 ... 12 of 16 are empty for every row, as are 14 and 15 of 16, which
# lie beyond the range), 39 is (the last valid row); 5 and 17 are holes inside otherwise used blocks
BLOCKED_REFERENCED = tuple(i for i in range(25) if i not in (5, 17)) + (39,)

UPDATE_PARTS = tuple(range(1, 18)) + (24, 25, 64)
UPDATE_LONG_PARTS = (1, 2, 9, 13, 25)                                # also run at len_pad 384
SUMS_PARTS = (1, 2, 63, 64, 65, 511, 512, 513, 1025, 1600)
ROWSUM_LEN_PADS = (128, 640)
EXACT_LIMIT = 2.0 ** 24


def frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.flags.writeable = False


def row_lengths(rows: int):
    if rows == 1:
        return (65,)
    if rows == 5:
        return (0, 9, 65, 130, 1)
    return tuple(ROW_LENGTHS[i % len(ROW_LENGTHS)] for i in range(rows))


def build_image(rows: int, referenced, rng, values):
    """ptr / idx / val of `rows` rows with row_lengths(rows), indices drawn from `referenced` (ascending within a row; with repeats only where a row is longer than
    the set), values from values(count).  Returns (ptr, idx, val, zero_a_row): zero_a_row is the row whose row of A the case sets to zero (None for one row)."""
    referenced = np.asarray(referenced, dtype=np.int32)
    lengths = row_lengths(rows)
    ptr = np.zeros(rows + 1, np.int32)
    ptr[1:] = np.cumsum(lengths)
    idx = np.zeros(ptr[-1], np.int32)
    val = np.asarray(values(int(ptr[-1])))
    longest = int(np.argmax(lengths))
    dup_row = lengths.index(65)
    for i, L in enumerate(lengths):
        chosen = rng.choice(referenced, L, replace=L > len(referenced))
        if i == longest:
            chosen[0], chosen[-1] = referenced[0], referenced[-1]          # the first and the last valid row of the gathered panel
        chosen.sort()
        if i == dup_row:
            chosen[31] = chosen[30]                                         # a duplicated index (stays ascending)
        idx[ptr[i]:ptr[i + 1]] = chosen
    val[ptr[dup_row] + 2] = 0                                               # a stored explicit zero
    assert idx[ptr[longest]] == referenced[0] and idx[ptr[longest + 1] - 1] == referenced[-1]
    return ptr, idx, val, (lengths.index(9) if rows > 1 else None)


def _prove_gather_exact(ptr, idx, val, A, B, a_scale, rows, dtype):
    """Every operation of the gather on these inputs is exact in a type with 24 significant bits: per row, with den_p the (power-of-two) denominators,
      * the dot products: all products a_c B(j, c) are multiples of the smallest nonzero |a_c| (a power of two) and their absolute sum in that unit is < 2^24,
        so every partial sum in any order is exact; the sum is 0 or a power of two >= 4, which the add of eps leaves as it is (0 + eps = eps);
      * the quotients x_p / den_p: a small integer over a power of two;
      * out(row, c) = sum_p x_p B(j_p, c) / den_p and t_vwh(row) = sum_p x_p wh_p: all terms are multiples of 1 / max_p den_p (of min_p wh_p) and their absolute
        sum in that unit is < 2^24."""
    eps = ref.eps_of(dtype)
    s = np.ones(A.shape[1]) if a_scale is None else a_scale.astype(np.float64)
    for row in range(rows):
        lo, hi = ptr[row], ptr[row + 1]
        if hi == lo:
            continue
        a = A[row].astype(np.float64) * s
        Bj = B[idx[lo:hi]].astype(np.float64)
        x = val[lo:hi].astype(np.float64)
        assert np.all(np.isfinite(Bj)) and np.all(np.isfinite(a))
        prods = Bj * a
        unit = np.min(np.abs(a[a != 0])) if np.any(a != 0) else 1.0
        assert np.log2(unit) == np.round(np.log2(unit))
        assert np.all(prods / unit == np.round(prods / unit)) and np.all(np.abs(prods).sum(axis=1) / unit < EXACT_LIMIT)
        wh = prods.sum(axis=1)
        nz = wh != 0
        assert np.all(wh[nz] >= 4) and np.all(np.log2(wh[nz]) == np.round(np.log2(wh[nz])))
        den = np.asarray(wh + eps, dtype=dtype).astype(np.float64)
        assert np.array_equal(den[nz], wh[nz]) and np.all(den[~nz] == eps)
        top = den.max()
        terms = (x / den)[:, None] * Bj * top
        assert np.all(terms == np.round(terms)) and np.all(np.abs(terms).sum(axis=0) < EXACT_LIMIT)
        if np.any(nz):
            low = wh[nz].min()
            assert np.all(x * wh / low == np.round(x * wh / low)) and np.abs(x * wh).sum() / low < EXACT_LIMIT


@functools.lru_cache(maxsize=None)
def gather_case(dtype_name: str, RP: int, r: int, rows: int, rows_pad: int, kind: str, scaled: bool = False, blocked: bool = False):
    """A case of op_kl_fused / op_sddmm_quotient: dict with ptr, idx, val, A (rows_pad, RP), B (gathered panel), a_scale (or None), rows, rows_pad, r, RP, range
    (the valid rows of the gathered panel).  kind "exact" or "random" (module docstring)."""
    dtype = np.dtype(dtype_name)
    seed = [RP, r, rows, rows_pad, int(kind == "exact"), int(scaled), int(blocked), dtype.itemsize]
    rng = np.random.default_rng(seed)
    valid, pad = (BLOCKED_RANGE, BLOCKED_PAD) if blocked else (GATHER_VALID, GATHER_PAD)
    if blocked:
        referenced = np.array(BLOCKED_REFERENCED)
    else:
        inner = np.sort(rng.choice(np.arange(1, valid - 1), (2 * valid) // 3, replace=False))
        referenced = np.concatenate([[0], inner, [valid - 1]])
    exact = kind == "exact"
    values = (lambda k: rng.integers(1, 4, k).astype(dtype)) if exact else (lambda k: (0.02 + 0.08 * rng.random(k)).astype(dtype))
    ptr, idx, val, zero_row = build_image(rows, referenced, rng, values)
    referenced = np.unique(idx)                                          # (a short image does not reach every candidate: what no index refers to holds NaN)
    A = np.full((rows_pad, RP), np.nan, dtype)
    B = np.full((pad, RP), np.nan, dtype)
    a_scale = None
    if exact:
        a0 = 2.0 ** rng.integers(0, 3, r); a0[r - 1] = 1
        s = np.ones(RP)
        if scaled:
            s[:r] = 2.0 ** rng.integers(0, 2, r); s[r - 1] = 1
            a_scale = s.astype(dtype)
        w = a0 * s[:r]                                                   # what the dot product sees of a row of A, up to the row's power of two
        body = rng.integers(0, 3, (len(referenced), r)).astype(np.float64)
        partial = body[:, :r - 1] @ w[:r - 1]
        top = 2.0 ** np.ceil(np.log2(max(4.0, partial.max())))
        target = top * (1 + (np.arange(len(referenced)) % 2))           # w . B(j, :): a power of two >= 4
        body[:, r - 1] = target - partial
        assert np.all(body >= 0)
        B[referenced] = 0
        B[referenced, :r] = body
        A[:rows] = 0
        A[:rows, :r] = (2.0 ** (np.arange(rows) % 6))[:, None] * a0[None, :]
    else:
        if scaled:
            a_scale = np.ones(RP, dtype); a_scale[:r] = (0.5 + 1.5 * rng.random(r)).astype(dtype)
        B[referenced] = 0
        B[referenced, :r] = (0.5 + rng.random((len(referenced), r))).astype(dtype)
        A[:rows] = 0
        A[:rows, :r] = (0.5 + rng.random((rows, r))).astype(dtype)
    if zero_row is not None:
        A[zero_row] = 0
    if exact:
        _prove_gather_exact(ptr, idx, val, A, B, a_scale, rows, dtype)
    case = {"ptr": ptr, "idx": idx, "val": val, "A": A, "B": B, "a_scale": a_scale, "rows": rows, "rows_pad": rows_pad, "r": r, "RP": RP, "range": valid,
            "zero_row": zero_row, "dtype": dtype, "exact": exact}
    frozen(ptr, idx, val, A, B, a_scale)
    return case


@functools.lru_cache(maxsize=None)
def gather_reference(dtype_name: str, RP: int, r: int, rows: int, rows_pad: int, kind: str, scaled: bool = False, blocks: int = 1):
    """(case, boundary array or None, restatement) of op_kl_fused on gather_case(...); blocks > 1: the blocked case and its boundaries.  In a random case the
    builder also checks that no row's divergence terms cancel (sum |term| <= 8 |sum term|): the t_kl bound is relative to sum |term|."""
    case = gather_case(dtype_name, RP, r, rows, rows_pad, kind, scaled, blocks > 1)
    dtype = case["dtype"]
    bptr = ref.boundaries(case["ptr"], case["idx"], case["range"], blocks) if blocks > 1 else None
    want = ref.kl_fused(bptr if blocks > 1 else case["ptr"], case["idx"], case["val"], case["A"], case["B"], rows, rows_pad, ref.eps_of(dtype), case["a_scale"], blocks,
                        round_den=dtype if case["exact"] else None)
    if not case["exact"]:
        assert np.all(want["kl_abs"] <= 8 * np.abs(want["t_kl"]))
    frozen(bptr, *[v for v in want.values()])
    return case, bptr, want


@functools.lru_cache(maxsize=None)
def sddmm_reference(dtype_name: str, RP: int, r: int, rows: int, rows_pad: int, kind: str):
    case = gather_case(dtype_name, RP, r, rows, rows_pad, kind)
    dtype = case["dtype"]
    want = ref.sddmm_quotient(case["ptr"], case["idx"], case["val"], case["A"], case["B"], rows, ref.eps_of(dtype), round_den=dtype if case["exact"] else None)
    frozen(*want.values())
    return case, want


@functools.lru_cache(maxsize=None)
def spmm_case(dtype_name: str, RP: int, r: int, rows: int, rows_pad: int, kind: str):
    """A case of op_spmm_rows (signed values) and its restatement: (dict with ptr, idx, val, P, rows, rows_pad, r, RP; restatement).  Exact: small integers, every
    term an integer and every absolute sum < 2^24 (asserted)."""
    dtype = np.dtype(dtype_name)
    rng = np.random.default_rng([7, RP, r, rows, rows_pad, int(kind == "exact"), dtype.itemsize])
    inner = np.sort(rng.choice(np.arange(1, GATHER_VALID - 1), (2 * GATHER_VALID) // 3, replace=False))
    referenced = np.concatenate([[0], inner, [GATHER_VALID - 1]])
    exact = kind == "exact"
    values = (lambda k: rng.integers(-3, 4, k).astype(dtype)) if exact else (lambda k: (2 * rng.random(k) - 1).astype(dtype))
    ptr, idx, val, _ = build_image(rows, referenced, rng, values)
    referenced = np.unique(idx)
    P = np.full((GATHER_PAD, RP), np.nan, dtype)
    P[referenced] = 0
    P[referenced, :r] = rng.integers(0, 8, (len(referenced), r)).astype(dtype) if exact else rng.random((len(referenced), r)).astype(dtype)
    want = ref.spmm_rows(ptr, idx, val, P, rows, rows_pad)
    if exact:
        assert np.all(want["abs"] < EXACT_LIMIT)        # integers throughout
    case = {"ptr": ptr, "idx": idx, "val": val, "P": P, "rows": rows, "rows_pad": rows_pad, "r": r, "RP": RP, "dtype": dtype, "exact": exact}
    frozen(ptr, idx, val, P, *want.values())
    return case, want


def update_settings(parts: int):
    """(want_sumsq, with_scale) of the launches at a part count: the H step's form (sums only) and the W step's (sums of squares and sums), each with or without
    the pending scale; all four at 1, 9 and 17 parts, otherwise the two forms with the scale on alternating sides."""
    if parts in (1, 9, 17):
        return ((False, False), (False, True), (True, False), (True, True))
    return ((False, parts % 2 == 0), (True, parts % 2 == 1))


@functools.lru_cache(maxsize=None)
def update_case(dtype_name: str, RP: int, r: int, len_pad: int, parts: int, kind: str, with_scale: bool):
    """A case of op_kl_update and its restatement: (dict with P, num (flat, the part panels `stride` values apart with NaN between them), stride, parts, den, scale,
    r, RP, len_pad; restatement).  The stride is 16 RP values wider than a panel.  Exact: den in {4, 8, 16} on the valid columns and 0 on the padding (0 * 0 / eps
    = 0), P in {0 ... 3}, scale in {1, 2}, the parts' numerators small integers that add up to at most 8 -- every new value is a multiple of 1 / 16 and the sums of
    128 of them and of their squares stay below 2^24 units (asserted)."""
    dtype = np.dtype(dtype_name)
    rng = np.random.default_rng([11, RP, r, len_pad, parts, int(kind == "exact"), int(with_scale), dtype.itemsize])
    exact = kind == "exact"
    panel = len_pad * RP
    stride = panel + 16 * RP
    P = np.zeros((len_pad, RP), dtype); den = np.zeros(RP, dtype)
    nums = np.zeros((parts, len_pad, RP), dtype)
    scale = None
    if exact:
        P[:, :r] = rng.integers(0, 4, (len_pad, r))
        den[:r] = 2.0 ** rng.integers(2, 5, r)
        total = rng.integers(0, 9, (len_pad, r))
        owner = rng.integers(0, parts, (8, len_pad, r))                  # every unit of the total goes to a part of its own choice
        for k in range(8):
            np.add.at(nums, (owner[k], *np.indices((len_pad, r))), (total > k).astype(dtype))
        if with_scale:
            scale = np.ones(RP, dtype); scale[:r] = 2.0 ** rng.integers(0, 2, r)
    else:
        P[:, :r] = rng.random((len_pad, r)); den[:r] = 0.5 + rng.random(r)
        nums[:, :, :r] = rng.random((parts, len_pad, r))
        if with_scale:
            scale = np.ones(RP, dtype); scale[:r] = 0.5 + 1.5 * rng.random(r)
    num = np.full((parts - 1) * stride + panel + 16 * RP, np.nan, dtype)
    for k in range(parts):
        num[k * stride:k * stride + panel] = nums[k].ravel()
    want = ref.kl_update(P, nums, den, ref.eps_of(dtype), scale, round_den=dtype if exact else None)
    if exact:
        assert np.all(nums.sum(axis=0) <= 8) and np.all(nums[:, :, r:] == 0)
        d = np.asarray(den[:r].astype(np.float64) + ref.eps_of(dtype), dtype=dtype)
        assert np.array_equal(d, den[:r])                                # the add of eps changes nothing
        v = want["P"].astype(np.float64)
        assert np.all(v * 16 == np.round(v * 16))
        g = v.reshape(-1, 128, RP)
        assert np.all(g.sum(axis=1) * 16 < EXACT_LIMIT) and np.all((g * g).sum(axis=1) * 256 < EXACT_LIMIT)
    case = {"P": P, "num": num, "stride": stride, "parts": parts, "den": den, "scale": scale, "r": r, "RP": RP, "len_pad": len_pad, "dtype": dtype, "exact": exact}
    frozen(P, num, den, scale, *want.values())
    return case, want


@functools.lru_cache(maxsize=None)
def sums_case(dtype_name: str, RP: int, r: int, parts: int, kind: str):
    """A case of op_kl_sums and its restatements with and without sumsq_part: (sum_part, sumsq_part, zero column, restatement with, restatement without).  One
    valid column's sums of squares are all zero (the guard: sums = the plain sum, scale = 1).  Exact: small integers; every other column's sums of squares add up
    to a power of four (the last part makes up the difference), so the square root, the reciprocal and the division are exact too."""
    dtype = np.dtype(dtype_name)
    rng = np.random.default_rng([13, RP, r, parts, int(kind == "exact"), dtype.itemsize])
    sa = np.zeros((parts, RP), dtype); sb = np.zeros((parts, RP), dtype)
    zero_col = r // 2
    if kind == "exact":
        sa[:, :r] = rng.integers(0, 8, (parts, r))
        sb[:, :r] = rng.integers(0, 4, (parts, r))
        rest = sb[:-1, :r].astype(np.float64).sum(axis=0)
        total = 4.0 ** np.ceil(np.log2(np.maximum(rest, 1)) / 2 + 1)
        sb[-1, :r] = total - rest
        assert np.all(sb >= 0) and np.all(total < EXACT_LIMIT) and np.all(sa.astype(np.float64).sum(axis=0) < EXACT_LIMIT)
    else:
        sa[:, :r] = rng.random((parts, r)); sb[:, :r] = rng.random((parts, r))
    sb[:, zero_col] = 0
    with_sq, without = ref.kl_sums(sa, sb), ref.kl_sums(sa)
    frozen(sa, sb, with_sq["sums"], with_sq["scale"], without["sums"])
    return sa, sb, zero_col, with_sq, without


@functools.lru_cache(maxsize=None)
def rowsum_case(dtype_name: str, RP: int, r: int, len_pad: int, kind: str):
    dtype = np.dtype(dtype_name)
    rng = np.random.default_rng([17, RP, r, len_pad, int(kind == "exact"), dtype.itemsize])
    P = np.zeros((len_pad, RP), dtype)
    P[:len_pad - 3, :r] = rng.integers(0, 8, (len_pad - 3, r)) if kind == "exact" else rng.random((len_pad - 3, r))
    want = ref.panel_rowsum(P)
    frozen(P, *want.values())
    return P, want


# ---------------------------------------------------------------------------------------------------------------- comparisons

def worst_ratio(got, want, bound):
    """max over the elements of |got - want| / bound (0 / 0 counts as 0, anything / 0 as infinity): <= 1 means every element is inside its bound."""
    err = np.abs(np.asarray(got).astype(ref.WORK) - want)
    bound = np.asarray(bound).astype(ref.WORK)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0, np.where(bound > 0, err / bound, np.inf))
    if np.any(np.isnan(err)):
        return float("inf")
    return float(ratio.max()) if ratio.size else 0.0


def same_bits(got, want, dtype) -> bool:
    """The launch's array against the restatement rounded to the launch's type (exact cases: the restatement's values are representable), NaN equal to NaN."""
    return np.array_equal(np.asarray(got), np.asarray(want).astype(dtype), equal_nan=True)
