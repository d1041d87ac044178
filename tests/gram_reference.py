"""float64 restatements of the Gram-matrix kernels, one launch at a time, with element-wise bounds (docs/GRAM.md): the rank-64 matrix from the split image
(gram_image.h: one slice, K-split, spread), the rank-64 reductions of partial matrices (kernels_mu64.hip) and the slices and reductions of the padded ranks
128 ... 512 (gram_wide.h, kernels_wide.hip).  tests/test_gram_cpu.py shows what the bounds catch (MUTATIONS); the tests/test_gpu_gram_*.py modules hold the kernels
to them.

Every quantity is a pair (value, absolute bound).
  split routes   The value is the sum of the SIX KEPT bf16 x bf16 terms of every product (tests/test_split3.py), not P^T P: each term is exact in fp32, so the only
                 error is that of adding them.  The matrix pipe's internal adder is not documented, so the count is the loosest one: one rounding per kept term,
                 6 * (padded rows of the range), plus the additions of the waves' partial tiles; bound = gamma(n) * sum |kept terms|, any order.
                 (The float64 sums below are themselves exact on the exact cases and carry a relative 2^-53 per addition elsewhere, five orders below u.)
  sums           n values added in any order: gamma(n) * sum |values| (n counts the additions of a zero the kernels make, too).
  scales         q > 0 ? 1 / sqrt(q) : 1, restated literally; the root and the reciprocal are correctly rounded (the library is built without fast-math,
                 docs/DIVERGENCE.md, "Documented and measured constants"): two roundings on top of half the relative bound of q.
  scaled element (v * s[c]) * s[r]: two products.
Nothing here is measured on the device."""
import numpy as np

from tests.panel_update_reference import gamma
from tests.test_split3 import split3

U = 2.0 ** -24
SPREAD_SLICES, KSPLIT_MAX, REDUCE_BLOCKS, IMAGE_TILES = 3, 8, 16, 10         # csrc/kernels.h
# kept terms in the order the kernels issue them: (plane of the row operand, plane of the column operand), 0 = hi, 1 = mid, 2 = lo
KEPT = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))
DROPPED = ((1, 2), (2, 1), (2, 2))

# the defects tests/test_gram_cpu.py applies, numbered as in docs/GRAM.md
# (a seventeenth, the mirror taken from the lower triangle of a diagonal block, has no restatement: both triangles sum the same six products, see the CPU module)
MUTATIONS = ("drop_term_0", "drop_term_1", "drop_term_2", "drop_term_3", "drop_term_4", "drop_term_5", "skip_boundary_step", "double_boundary_step",
             "drop_last_pair", "no_mirror", "scale_wrong_source", "scale_once", "drop_colsq_batch", "drop_spread_piece", "drop_quarter_slice", "qx3_unmirrored")


def planes(P):
    """The three bf16 planes of an fp32 array, as float64."""
    hi, mid, lo, _ = split3(np.asarray(P, dtype=np.float32))
    return [x.astype(np.float64) for x in (hi, mid, lo)]


def six_term(pl, y0, y1, mutate=None):
    """(value, sum of magnitudes) of the kept terms of P^T P over the panel rows [y0, y1) (clipped to the panel), pl = planes(P)."""
    n = pl[0].shape[0]
    y0, y1 = max(0, min(y0, n)), max(0, min(y1, n))
    C = pl[0].shape[1]
    val, mag = np.zeros((C, C)), np.zeros((C, C))
    if y1 <= y0:
        return val, mag
    for t, (i, j) in enumerate(KEPT):
        if mutate == f"drop_term_{t}":
            continue
        a, b = pl[i][y0:y1], pl[j][y0:y1]
        val += a.T @ b
        mag += np.abs(a).T @ np.abs(b)
    return upper_mirrored(val), upper_mirrored(mag)


def upper_mirrored(v):
    """Both triangles carry the UPPER element's value, as every kernel here writes them (the six-term sums of (r, c) and (c, r) add the same products in another order)."""
    v = np.array(v)
    iu = np.triu_indices(v.shape[-1], 1)
    v[..., iu[1], iu[0]] = v[..., iu[0], iu[1]]
    return v


def dropped_terms_ratio(P, Q=None):
    """max over the products P(y, r) Q(y, c) of |three dropped terms| / (|a| |b|), computed exactly."""
    a = planes(P)
    b = a if Q is None else planes(Q)
    worst = 0.0
    fa = np.abs(np.asarray(P, dtype=np.float64))
    fb = fa if Q is None else np.abs(np.asarray(Q, dtype=np.float64))
    for y in range(a[0].shape[0]):
        d = sum(np.outer(a[i][y], b[j][y]) for i, j in DROPPED)
        full = np.outer(fa[y], fb[y])
        nz = full > 0
        if nz.any():
            worst = max(worst, float((np.abs(d[nz]) / full[nz]).max()))
    return worst


def sum_bound(n, mag):
    return gamma(max(n, 1), U) * mag


# ---- scales ---------------------------------------------------------------------------------------------------------------------------------------------

def rsqrt_scale(q, qb):
    """(s, bound) of s = q > 0 ? 1 / sqrt(q) : 1 for q known to the absolute bound qb."""
    q = np.asarray(q, dtype=np.float64); qb = np.broadcast_to(np.asarray(qb, dtype=np.float64), q.shape)
    pos = q > 0
    assert np.all(qb[pos] < 0.01 * q[pos]), "a sum of squares whose bound reaches zero: the guarded branch is not decided"
    assert np.all(qb[~pos] == 0) and np.all(q[~pos] == 0), "sums of squares are not negative"
    qq = np.where(pos, q, 1.0)
    d = np.where(pos, qb / qq, 0.0)
    s = np.where(pos, 1.0 / np.sqrt(qq), 1.0)
    e_root = (1 + 0.5 * d / (1 - d)) * (1 + U) - 1
    rel = e_root / (1 - e_root) + U * (1 + e_root / (1 - e_root))
    return s, np.where(pos, s * rel, 0.0)


def scale_both_sides(v, vb, s, sb, mutate=None):
    """(value, bound) of (v * s[c]) * s[r] for the matrix v[r, c]."""
    sc, sr = s[None, :], s[:, None]
    rc, rr = (sb / s)[None, :], (sb / s)[:, None]
    if mutate == "scale_once":
        sr, rr = np.ones_like(sr), np.zeros_like(rr)
    grow = (1 + rc) * (1 + rr) * (1 + U) ** 2
    val = v * sc * sr
    return val, np.abs(sc * sr) * vb * grow + np.abs(val) * (grow - 1)


def colsq_sum(colsq_part, mutate=None):
    """(q, bound) of the column sums of a [parts][C] array of partial sums of squares: gram_image_segment adds them in batches of 40 per group of threads,
    stride 320, the eight groups in order; k_gram_reduce_x3 and k_mu64_reduce_scale_all_x3 in four groups.  Any order: gamma(parts + groups)."""
    cp = np.asarray(colsq_part, dtype=np.float64)
    if mutate == "drop_colsq_batch":
        cp = cp[:320]              # (the second batch of every thread group: parts 320 ...)
    return cp.sum(axis=0), sum_bound(cp.shape[0] + 8, np.abs(cp).sum(axis=0))


# ---- rank 64 from the split image -----------------------------------------------------------------------------------------------------------------------

def image_geometry(length):
    ks = (length + 15) // 16
    return ks, (ks + 2) // 2


def tile_of(t):
    ti = 0 if t < 4 else 1 if t < 7 else 2 if t < 9 else 3
    tj = t if t < 4 else t - 3 if t < 7 else t - 5 if t < 9 else 3
    return ti, tj


def spread_deal(pairs):
    """The spread form's deal (gram_image_block): a list of (workgroup, tile, piece, first pair, end pair), pairs counted inside the tile."""
    total = IMAGE_TILES * pairs
    out = []
    for blk in range(REDUCE_BLOCKS if pairs > 0 else 0):
        w0, w1 = total * blk // REDUCE_BLOCKS, total * (blk + 1) // REDUCE_BLOCKS
        t = w0 // pairs
        while t < IMAGE_TILES and t * pairs < w1:
            a, b = max(w0, t * pairs), min(w1, (t + 1) * pairs)
            if b > a:
                first = blk
                while first > 0 and total * first // REDUCE_BLOCKS > t * pairs:
                    first -= 1
                out.append((blk, t, blk - first, a - t * pairs, b - t * pairs))
            t += 1
    return out


def _rows_of_pairs(p0, p1, ks, mutate, inner):
    """Panel rows of the pairs of K-steps [p0, p1) of an image of ks K-steps.  inner: the range starts at a boundary between two pieces."""
    y0, y1 = 32 * p0, min(32 * p1, 16 * ks)
    if inner and mutate == "skip_boundary_step":
        y0 += 16
    if inner and mutate == "double_boundary_step":
        y0 -= 16
    return y0, y1


def _count(p0, p1):
    return 6 * 32 * max(p1 - p0, 0) + 3          # one rounding per kept term of the padded rows, the four waves' tiles added


def image_scales(pl, length, colsq_part, normalize, mutate=None):
    """(s, bound, q source) of the column scales of the one-slice form and of the slices' publisher."""
    if not normalize:
        return np.ones(64), np.zeros(64)
    from_parts = colsq_part is not None
    if mutate == "scale_wrong_source":
        from_parts = not from_parts
        if from_parts:
            colsq_part = np.ones((1, 64))        # (what a stale buffer might hold)
    if from_parts:
        q, qb = colsq_sum(colsq_part, mutate)
    else:
        ks, pairs = image_geometry(length)
        v, m = six_term(pl, 0, length, mutate)
        q, qb = np.diag(v).copy(), np.diag(sum_bound(_count(0, pairs), m)).copy()
    return rsqrt_scale(q, qb)


def gram_image(P, colsq_part=None, normalize=0, ksplit=0, spread=0, mutate=None):
    """Restates one launch of k_gram_image / the image passengers.  Returns a dict of (value, bound) pairs: `G` (the one-slice form: [64][64]; else the unscaled
    slices / pieces [slices][64][64], absent pieces 0 with bound 0), `scale`, and in the spread form `spread_out` (what the last workgroup finishes)."""
    P = np.asarray(P, dtype=np.float32)
    length = P.shape[0]
    pl = planes(P)
    ks, pairs = image_geometry(length)
    if mutate == "drop_last_pair":
        pairs = max(ks // 2, 0)
    res = {}
    in_pieces = ksplit > 1 or spread > 0
    # the slices and pieces publish scales from colsq_part, or ones: never from a diagonal (the launcher refuses that request)
    assert not (in_pieces and normalize and colsq_part is None)
    s, sb = image_scales(pl, length, colsq_part, normalize, mutate)
    if in_pieces and normalize and mutate == "scale_wrong_source":
        # what the refusal keeps out: the publisher (slice 0, or piece 0 of a diagonal tile) taking the scale from the diagonal of ITS part of the K range
        q = np.zeros(64)
        for ti in range(4):
            if spread > 0:
                t = (0, 4, 7, 9)[ti]
                a, b = next((a, b) for _, tt, piece, a, b in spread_deal(pairs) if tt == t and piece == 0)
            else:
                a, b = 0, pairs // ksplit
            y0, y1 = _rows_of_pairs(a, b, ks, None, False)
            q[16 * ti:16 * ti + 16] = np.diag(six_term(pl, y0, y1)[0])[16 * ti:16 * ti + 16]
        s, sb = rsqrt_scale(q, 0.0)
    res["scale"] = (s, sb)
    if not in_pieces:
        y0, y1 = _rows_of_pairs(0, pairs, ks, mutate, False)
        v, m = six_term(pl, y0, y1, mutate)
        res["G"] = scale_both_sides(v, sum_bound(_count(0, pairs), m), s, sb, mutate)
        if mutate == "no_mirror":
            res["G"][0][np.tril_indices(64, -16)] = np.nan
        return res
    if spread > 0:
        val, bnd = np.zeros((SPREAD_SLICES, 64, 64)), np.zeros((SPREAD_SLICES, 64, 64))
        for blk, t, piece, a, b in spread_deal(pairs):
            assert piece < SPREAD_SLICES
            if mutate == "drop_spread_piece" and piece == 1:
                continue
            ti, tj = tile_of(t)
            y0, y1 = _rows_of_pairs(a, b, ks, mutate, a > 0)
            v, m = six_term(pl, y0, y1, mutate)
            e = sum_bound(_count(a, b), m)
            R, Cc = slice(16 * ti, 16 * ti + 16), slice(16 * tj, 16 * tj + 16)
            val[piece, R, Cc], bnd[piece, R, Cc] = v[R, Cc], e[R, Cc]
            if ti != tj and mutate != "no_mirror":
                val[piece, Cc, R], bnd[piece, Cc, R] = v[R, Cc].T, e[R, Cc].T
        res["G"] = (val, bnd)
        tot = val.sum(axis=0)
        tb = bnd.sum(axis=0) + gamma(SPREAD_SLICES - 1, U) * (np.abs(val).sum(axis=0) + bnd.sum(axis=0))
        res["spread_out"] = scale_both_sides(tot, tb, s, sb, mutate)
        return res
    val, bnd = np.zeros((ksplit, 64, 64)), np.zeros((ksplit, 64, 64))
    for sl in range(ksplit):
        p0, p1 = pairs * sl // ksplit, pairs * (sl + 1) // ksplit
        y0, y1 = _rows_of_pairs(p0, p1, ks, mutate, sl > 0 and p1 > p0)
        v, m = six_term(pl, y0, y1, mutate)
        val[sl], bnd[sl] = v, sum_bound(_count(p0, p1), m)
        if mutate == "no_mirror":
            val[sl][np.tril_indices(64, -16)] = np.nan
    res["G"] = (val, bnd)
    return res


# ---- rank 64 from partial matrices ----------------------------------------------------------------------------------------------------------------------

def gram_partials(P):
    """launch_mu64_gram_partials: one matrix per 64 panel rows, fp32 products on the matrix pipe (64 products and 64 additions per element)."""
    P = np.asarray(P, dtype=np.float64).reshape(-1, 64, 64)
    val = np.einsum("pyr,pyc->prc", P, P)
    return val, gamma(128, U) * np.einsum("pyr,pyc->prc", np.abs(P), np.abs(P))


def partial_sum(partials, mutate=None):
    """The sum of [parts][...] partial matrices, any grouping (two halves, four quarters, in order): gamma(parts + 4)."""
    p = np.asarray(partials, dtype=np.float64)
    if mutate == "drop_quarter_slice" and p.shape[0] > 1:
        n = p.shape[0]
        g = next(g for g in range(4) if n * (g + 1) // 4 > n * g // 4)
        p = np.delete(p, n * (g + 1) // 4 - 1, axis=0)          # the last slice of the first quarter that has any
    return p.sum(axis=0), sum_bound(p.shape[0] + 4, np.abs(p).sum(axis=0))


def gram_reduce(partials, normalize, mutate=None):
    """launch_mu64_gram_reduce, gram_reduce_block_x3, launch_gram64_from_partials with a scale: G = D (sum) D, D from the diagonal of the sum."""
    v, vb = partial_sum(partials, mutate)
    if not normalize:
        return {"G": (v, vb), "scale": (np.ones(64), np.zeros(64))}
    s, sb = rsqrt_scale(np.diag(v).copy(), np.diag(vb).copy())
    return {"G": scale_both_sides(v, vb, s, sb, mutate), "scale": (s, sb)}


def gram_reduce_scale_all(partials, sumsq_part, mutate=None):
    """launch_gram64_reduce_scale_all: the scales from the sums of squares, G = D (sum) D."""
    v, vb = partial_sum(partials, mutate)
    if mutate == "scale_wrong_source":
        q, qb = np.diag(v).copy(), np.diag(vb).copy()
    else:
        q, qb = colsq_sum(sumsq_part)
    s, sb = rsqrt_scale(q, qb)
    return {"G": scale_both_sides(v, vb, s, sb, mutate), "scale": (s, sb)}


def scale_from_value(q_dev):
    """The scale of a sum of squares the DEVICE holds (an fp32 array): two correctly rounded operations on an exact input."""
    return rsqrt_scale(np.asarray(q_dev, dtype=np.float64), 0.0)


def scaled_panel(P, scale_dev):
    """P(y, c) * scale(c) in fp32: one product, an exact function of the scales the launch published."""
    return (np.asarray(P, dtype=np.float32) * np.asarray(scale_dev, dtype=np.float32)[None, :]).astype(np.float32)


def scaled_matrix_fp32(G_dev, scale_dev):
    """(G(r, c) * s(c)) * s(r) in fp32, the two products in the kernels' order: an exact function of its fp32 inputs."""
    s = np.asarray(scale_dev, dtype=np.float32)
    return ((np.asarray(G_dev, dtype=np.float32) * s[None, :]).astype(np.float32) * s[:, None]).astype(np.float32)


# ---- the split image ------------------------------------------------------------------------------------------------------------------------------------

def pack_panel_x3(P, ks):
    """The split image of the panel P ([len][RP] fp32) in k_pack_panel_x3's layout, ks K-steps (the closing step not included), as bf16 bit patterns:
    Fx[(((ks * NBT + nb) * 3 + plane) * 2 + h) * 32 + r][j] = plane of P(16 ks + 8 h + j, 32 nb + r)."""
    P = np.asarray(P, dtype=np.float32)
    length, RP = P.shape
    nbt = RP // 32
    full = np.zeros((16 * ks, RP), np.float32)
    full[:min(length, 16 * ks)] = P[:16 * ks]
    hi, mid, lo, _ = split3(full)
    out = np.empty((ks, nbt, 3, 2, 32, 8), np.uint16)
    for k, x in enumerate((hi, mid, lo)):
        bits = (np.ascontiguousarray(x).view(np.uint32) >> 16).astype(np.uint16)             # (each plane is a bf16 value: the low half is zero)
        out[:, :, k] = bits.reshape(ks, 2, 8, nbt, 32).transpose(0, 3, 1, 4, 2)               # [ks][h][j][nb][r] -> [ks][nb][h][r][j]
    return out.reshape(-1)


# ---- padded ranks 128 ... 512 ---------------------------------------------------------------------------------------------------------------------------

def wide_parts(RP, length, parts):
    nb = RP // 128
    nsuper = nb * (nb + 1) // 2
    return max(1, min(parts, max(16, 512 // nsuper), max(1, length // 64)))


def wide_written(RP, mirror):
    """Which elements of a slice k_gram_wide_x3<.., MIRROR> writes: the upper triangle, its mirror image (MIRROR), or only inside the 32 x 32 diagonal blocks."""
    r, c = np.indices((RP, RP))
    return (r <= c) | mirror | (r // 32 == c // 32)


def gram_wide_slices(P, RP, parts, mirror, mutate=None):
    """The slices of k_gram_wide_x3 for the SETTLED slice count `parts`: (value, bound, written), [parts][RP][RP].  Slice s holds the K-steps
    [steps * s / parts, steps * (s + 1) / parts) of 16 panel rows."""
    P = np.asarray(P, dtype=np.float32)
    pl = planes(P)
    steps = (P.shape[0] + 15) // 16
    val, bnd = np.zeros((parts, RP, RP)), np.zeros((parts, RP, RP))
    for s in range(parts):
        s0, s1 = steps * s // parts, steps * (s + 1) // parts
        y0, y1 = 16 * s0, 16 * s1
        if s > 0 and s1 > s0 and mutate == "skip_boundary_step":
            y0 += 16
        if s > 0 and s1 > s0 and mutate == "double_boundary_step":
            y0 -= 16
        v, m = six_term(pl, y0, y1, mutate)
        val[s], bnd[s] = v, sum_bound(6 * 16 * max(s1 - s0, 0), m)
    wr = wide_written(RP, mirror and mutate != "no_mirror")
    return val, bnd, wr


def gram_reduce_x3(partial, parts, RP, sumsq_part=None, mutate=None):
    """k_gram_reduce_x3 on the caller's slices (only the blocks on and above the diagonal are read): `G` (value, bound) and `scale`."""
    p = np.asarray(partial, dtype=np.float64)[:parts]
    up = np.triu(np.ones((RP // 32, RP // 32), bool)).repeat(32, 0).repeat(32, 1)          # 32 x 32 blocks on and above the diagonal
    v, vb = partial_sum(np.where(up, p, 0.0), mutate)
    lowb = ~up
    v[lowb], vb[lowb] = v.T[lowb], vb.T[lowb]
    if mutate == "no_mirror":
        v[lowb] = np.nan
    res = {"G": (v, vb)}
    if sumsq_part is not None:
        q, qb = colsq_sum(sumsq_part)
        res["scale"] = rsqrt_scale(q, qb)
    return res


def qx3_of(G_dev, mutate=None):
    """The split image k_gram_reduce_x3 writes beside G: that of G as a panel (row k, column c), RP / 16 K-steps."""
    G = np.asarray(G_dev, dtype=np.float32)
    RP = G.shape[0]
    if mutate == "qx3_unmirrored":
        up = np.triu(np.ones((RP // 32, RP // 32), bool), 1).repeat(32, 0).repeat(32, 1)
        G = G.copy()
        for bi in range(RP // 32):
            for bj in range(bi + 1, RP // 32):
                G[32 * bj:32 * bj + 32, 32 * bi:32 * bi + 32] = G[32 * bi:32 * bi + 32, 32 * bj:32 * bj + 32]      # the tile as it lies, not transposed
        del up
    return pack_panel_x3(G, RP // 16)


# ---- holding a launch's output to a (value, bound) pair -------------------------------------------------------------------------------------------------

def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def held(name, got, ref, exact=None, worst=None, key=None):
    """Asserts the fp32 output `got` against ref = (value, bound): equal as VALUES to fl32(value) where `exact` says so or the bound is zero, within the bound
    elsewhere.  Returns (and records under worst[key]) the largest error / bound."""
    val, bnd = np.asarray(ref[0], dtype=np.float64), np.asarray(ref[1], dtype=np.float64)
    got = np.asarray(got)
    assert got.shape == val.shape, (name, got.shape, val.shape)
    assert np.isfinite(got).all(), f"{name}: not finite at {np.argwhere(~np.isfinite(got))[:4].tolist()}"
    ex = np.broadcast_to(np.zeros((), bool) if exact is None else exact, val.shape) | (bnd == 0)
    want = val.astype(np.float32)
    bad = ex & (got != want)
    assert not bad.any(), f"{name}: exact elements differ at {np.argwhere(bad)[:4].tolist()}: {got[bad][:4]} != {want[bad][:4]}"
    err = np.abs(got.astype(np.float64) - val)
    over = ~ex & (err > bnd)
    assert not over.any(), f"{name}: beyond the bound at {np.argwhere(over)[:4].tolist()}: error / bound {(err[over] / bnd[over]).max():.3g}"
    ratio = float((err[~ex] / bnd[~ex]).max()) if (~ex).any() else 0.0
    if worst is not None:
        worst[key] = max(worst.get(key, 0.0), ratio)
    return ratio
