"""High-precision restatements of the six launches of nmfgpu_amd/csrc/kernels_sparse.hip that have an operation entry (op_kl_fused, op_kl_update, op_kl_sums,
op_panel_rowsum, op_spmm_rows, op_sddmm_quotient), written from the formulas in that file's comments with plain loops over the rows and numpy over a row's stored
entries.  Nothing here knows about lanes, groups, trips, batches or the order of a sum.  Also the error bounds the tests hold the launches to, and `boundaries`,
the rule of k_sp_boundaries.

The arithmetic is done in WORK: numpy's extended type where the platform has one (x86: 64 significant bits), float64 otherwise, so that a float64 launch is judged
against something more precise than itself.

u is the unit roundoff of the launch's type T and gamma(k) = k u / (1 - k u).  Every bound below holds for any summation order and with or without contraction of
a multiply and an add; they are derived from the operations, not measured:
  a sum of k nonnegative terms computed in T has a relative error of at most gamma(k - 1); a dot product over the RP coordinates of a panel row at most gamma(RP);
  each further rounded operation (the pending scale, the add of eps, the division, a product, the rounding of an input) adds one u -- the `+ 8` and `+ 4` are
  slack for those."""
import numpy as np

WORK = np.longdouble
LOG_ULPS = 4      # cap on the device logarithm's error, in units of u |log|: keeps the test independent of the math library's version


def unit_roundoff(dtype) -> float:
    return float(np.finfo(dtype).eps) / 2


def eps_of(dtype) -> float:
    """The eps the engine's KL iteration passes to its launches: the epsilon of the type."""
    return float(np.finfo(dtype).eps)


def gamma(k, u):
    ku = np.asarray(k, dtype=np.float64) * u
    assert np.all(ku < 0.5)
    return ku / (1 - ku)


def boundaries(ptr, idx, index_range: int, blocks: int) -> np.ndarray:
    """k_sp_boundaries' rule: per = ceil(range / blocks); entry b < blocks of a row is the first position of the row whose index is >= b per, entry `blocks` is
    the row's end (a row's indices ascend).  (rows, blocks + 1) int32."""
    per = -(-int(index_range) // int(blocks))
    rows = len(ptr) - 1
    out = np.empty((rows, blocks + 1), np.int32)
    for i in range(rows):
        seg = np.asarray(idx[ptr[i]:ptr[i + 1]])
        out[i, :blocks] = ptr[i] + np.searchsorted(seg, np.arange(blocks, dtype=np.int64) * per, side="left")
        out[i, blocks] = ptr[i + 1]
    return out


def _denominator(wh, eps, round_den):
    """wh + eps.  round_den (a dtype): rounded to that type -- what a launch in that type computes when every OTHER operation is exact (the constructed cases:
    there wh + eps rounds back to wh, which no arithmetic in WORK would do)."""
    d = wh + WORK(eps)
    return d if round_den is None else d.astype(round_den).astype(WORK)


def _ranges(ptr, rows, blocks):
    ptr = np.asarray(ptr)
    if blocks > 1:
        assert ptr.shape == (rows, blocks + 1)
        return ptr
    assert ptr.shape == (rows + 1,)
    return np.stack([ptr[:-1], ptr[1:]], axis=1)


def _entry_terms(x, wh, den):
    """Per stored entry: the quotient, val * wh and val * log(val / (wh + eps)) (0 where val is not > 0)."""
    q = x / den
    pos = x > 0
    kl = np.zeros(len(x), WORK)
    kl[pos] = x[pos] * np.log(x[pos] / den[pos])
    return q, x * wh, kl


def kl_fused(ptr, idx, val, A, B, rows, rows_pad, eps, a_scale=None, blocks=1, round_den=None):
    """out(row, :) = sum_p val[p] / ((s .* A(row, :)) . B(idx[p], :) + eps) * B(idx[p], :), per block of the boundary array; t_vwh(row) = sum_p val wh,
    t_kl(row) = sum_p val log(val / (wh + eps)).  Returns a dict: `out` (blocks, rows_pad, RP) with zeros in the rows >= rows, `t_vwh`, `t_kl` (blocks, rows), and
    what the bounds need: `n` (blocks, rows) the entries per row and block, `kl_abs` the sums of |val log(.)| and `kl_x` the sums of val over the entries > 0."""
    RP = A.shape[1]
    rng_ = _ranges(ptr, rows, blocks)
    out = np.zeros((blocks, rows_pad, RP), WORK)
    t_vwh = np.zeros((blocks, rows), WORK); t_kl = np.zeros((blocks, rows), WORK)
    n = np.zeros((blocks, rows), np.int64); kl_abs = np.zeros((blocks, rows), WORK); kl_x = np.zeros((blocks, rows), WORK)
    s = None if a_scale is None else np.asarray(a_scale).astype(WORK)
    for row in range(rows):
        a = np.asarray(A[row]).astype(WORK)
        if s is not None:
            a = a * s
        for b in range(blocks):
            lo, hi = int(rng_[row, b]), int(rng_[row, b + 1])
            if hi <= lo:
                continue
            x = np.asarray(val[lo:hi]).astype(WORK)
            Bj = np.asarray(B[idx[lo:hi]]).astype(WORK)
            wh = Bj @ a
            q, vwh, kl = _entry_terms(x, wh, _denominator(wh, eps, round_den))
            out[b, row] = q @ Bj
            t_vwh[b, row] = vwh.sum(); t_kl[b, row] = kl.sum()
            n[b, row] = hi - lo; kl_abs[b, row] = np.abs(kl).sum(); kl_x[b, row] = x[x > 0].sum()
    return {"out": out, "t_vwh": t_vwh, "t_kl": t_kl, "n": n, "kl_abs": kl_abs, "kl_x": kl_x}


def sddmm_quotient(ptr, idx, val, A, B, rows, eps, round_den=None):
    """q[p] = val[p] / (A(row, :) . B(idx[p], :) + eps) for every stored entry, and the per-row terms of kl_fused.  The same dict with `q` (nnz) for `out`; `n`,
    `kl_abs`, `kl_x`, `t_vwh`, `t_kl` have the shape (rows,)."""
    q = np.zeros(len(val), WORK)
    t_vwh = np.zeros(rows, WORK); t_kl = np.zeros(rows, WORK); kl_abs = np.zeros(rows, WORK); kl_x = np.zeros(rows, WORK)
    n = np.zeros(rows, np.int64)
    for row in range(rows):
        lo, hi = int(ptr[row]), int(ptr[row + 1])
        if hi <= lo:
            continue
        x = np.asarray(val[lo:hi]).astype(WORK)
        wh = np.asarray(B[idx[lo:hi]]).astype(WORK) @ np.asarray(A[row]).astype(WORK)
        q[lo:hi], vwh, kl = _entry_terms(x, wh, _denominator(wh, eps, round_den))
        t_vwh[row] = vwh.sum(); t_kl[row] = kl.sum()
        n[row] = hi - lo; kl_abs[row] = np.abs(kl).sum(); kl_x[row] = x[x > 0].sum()
    return {"q": q, "t_vwh": t_vwh, "t_kl": t_kl, "n": n, "kl_abs": kl_abs, "kl_x": kl_x}


def spmm_rows(ptr, idx, val, P, rows, rows_pad):
    """out(row, :) = sum_p val[p] P(idx[p], :); rows >= rows are zero.  Returns a dict: `out`, `abs` (the same sums over |val[p] P(idx[p], :)|), `n` (rows)."""
    RP = P.shape[1]
    out = np.zeros((rows_pad, RP), WORK); ab = np.zeros((rows_pad, RP), WORK)
    n = np.zeros(rows, np.int64)
    for row in range(rows):
        lo, hi = int(ptr[row]), int(ptr[row + 1])
        if hi <= lo:
            continue
        x = np.asarray(val[lo:hi]).astype(WORK)
        Pj = np.asarray(P[idx[lo:hi]]).astype(WORK)
        out[row] = x @ Pj; ab[row] = np.abs(x) @ np.abs(Pj)
        n[row] = hi - lo
    return {"out": out, "abs": ab, "n": n}


def kl_update(P, nums, den, eps, scale=None, round_den=None):
    """P(y, c) <- (P(y, c) scale(c)) (sum over the parts of num(y, c)) / (den(c) + eps); nums: (parts, len_pad, RP).  Returns a dict: `P`, and the sums of the new
    values and of their squares over each 128 rows, `sum_part`, `sumsq_part` ((len_pad / 128, RP))."""
    P = np.asarray(P).astype(WORK)
    num = np.zeros_like(P)
    for part in nums:
        num = num + np.asarray(part).astype(WORK)
    d = _denominator(np.asarray(den).astype(WORK), eps, round_den)
    old = P if scale is None else P * np.asarray(scale).astype(WORK)
    new = old * num / d
    groups = new.reshape(-1, 128, new.shape[1])
    return {"P": new, "sum_part": groups.sum(axis=1), "sumsq_part": (groups * groups).sum(axis=1)}


def kl_sums(sum_part, sumsq_part=None):
    """sums(c) = sum over the parts of sum_part(., c), divided by the square root of the sum over the parts of sumsq_part(., c) where that is given and > 0;
    scale(c) = 1 / that square root, 1 where the sum of squares is 0 (None without sumsq_part)."""
    sa = np.asarray(sum_part).astype(WORK).sum(axis=0)
    if sumsq_part is None:
        return {"sums": sa, "scale": None}
    sb = np.asarray(sumsq_part).astype(WORK).sum(axis=0)
    root = np.sqrt(np.where(sb > 0, sb, WORK(1)))
    return {"sums": sa / root, "scale": WORK(1) / root}


def panel_rowsum(P):
    """sums(c) = sum over the rows y of P(y, c).  Returns a dict: `sums`, `abs` (the sums of |P|)."""
    P = np.asarray(P).astype(WORK)
    return {"sums": P.sum(axis=0), "abs": np.abs(P).sum(axis=0)}


# ---------------------------------------------------------------------------------------------------------------- bounds (absolute, per element)

def fused_out_bound(RP, n, want, u):
    """out(row, c) of one block panel: gamma(RP + n + 8) want, n the row's entries in the block (n: (blocks, rows); want: (blocks, rows, RP))."""
    return gamma(RP + n + 8, u)[..., None] * np.abs(want)


def vwh_bound(RP, n, want, u):
    return gamma(RP + n + 4, u) * np.abs(want)


def kl_term_bound(RP, n, kl_x, kl_abs, u):
    """sum_p x_p (gamma(RP + 4) + L u |log(x_p / (wh_p + eps))|) + gamma(n) sum_p |term_p|, with sum_p x_p |log(.)| = sum_p |term_p|."""
    return gamma(RP + 4, u) * kl_x + (LOG_ULPS * u + gamma(n, u)) * kl_abs


def quotient_bound(RP, want, u):
    return gamma(RP + 4, u) * np.abs(want)


def spmm_bound(n, abs_sums, u):
    """gamma(n + 2) sum_p |val_p P(idx_p, c)| (n: (rows,); abs_sums: (rows, RP))."""
    return gamma(n + 2, u)[:, None] * abs_sums


def update_bound(parts, want, u):
    return gamma(parts + 4, u) * np.abs(want)


def update_sum_bounds(own, u):
    """The per-workgroup sums against the launch's OWN output rows `own` (len_pad, RP): gamma(128) sum |v| for sum_part, gamma(129) sum v^2 for sumsq_part.
    Returns (sums, bound, sums of squares, bound)."""
    g = np.asarray(own).astype(WORK).reshape(-1, 128, own.shape[1])
    s, sq = g.sum(axis=1), (g * g).sum(axis=1)
    return s, gamma(128, u) * np.abs(g).sum(axis=1), sq, gamma(129, u) * sq


def sums_bound(parts, want, u):
    """gamma(parts + 4) relative, on sums and on scale."""
    return gamma(parts + 4, u) * np.abs(want)


def rowsum_bound(len_pad, abs_sums, u):
    return gamma(len_pad, u) * abs_sums
