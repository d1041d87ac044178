"""Float64 restatements of the Frobenius panel update (docs/PANEL_UPDATE.md), written from the documented semantics: the comment block above k_panel_update
(nmfgpu_amd/csrc/kernels.hip), the header of kernels_mu64.hip and the struct comments of kernels.h (PanelFusedF32 / PanelFusedF64 / SmoothAround) -- plain
numpy, no fast path restated.  Panels are (len_pad, RP) arrays, row y = panel column y of the kernels' comments, Q is (RP, RP) and enters as

    den(y, c) = sum_k Q[k, c] old(y, k)        (MODE_MU)          new(y, c) = max(0, sum_k Q[k, c] num(y, k))        (MODE_LS)

Every function returns float64 values together with what the error bounds need: the same expressions evaluated on absolute values (`*_abs`) and the number of
roundings on the longest path to each result (`depth_*`).  The bounds hold for ANY order of summation:

    a quantity computed from non-negative operands by +, *, / with at most N roundings on a path has a relative error of at most gamma(N) = N u / (1 - N u)
    (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1 and 3.3); with signed operands the same gamma(N) applies to the expression evaluated on
    absolute values.

`mutate` names one deliberate defect (tests/test_panel_update_cpu.py holds the bounds against each of them)."""
import numpy as np

MUTATIONS = ("drop_slab", "drop_k_term", "transpose_q", "no_eps", "scale_wrong_side", "len_valid_off_by_one")
# |dropped terms| of the six-term product of exactly split operands, relative to |a b| (nmfgpu_amd/csrc/kernels_x3.hip, header: "<= ~2^-23 |a b|")
SPLIT_DROP = 2.0 ** -23


def unit_roundoff(dtype):
    return float(np.finfo(np.dtype(dtype)).eps) / 2


def eps_of(dtype):
    """The eps of the multiplicative update: machine epsilon of the type (the engines pass std::numeric_limits<T>::epsilon())."""
    return float(np.finfo(np.dtype(dtype)).eps)


def gamma(n, u):
    assert n * u < 0.01
    return n * u / (1 - n * u)


def numerator(slabs, len_pad, RP, mutate=None):
    """num = sum of the slabs; slab s is the first len_pad * RP values of row s of `slabs` (the rest of the row is a gap)."""
    s = np.asarray(slabs, dtype=np.float64)[:, :len_pad * RP].reshape(slabs.shape[0], len_pad, RP)
    if mutate == "drop_slab":
        s = s[:-1] if s.shape[0] > 1 else 0 * s
    return s.sum(axis=0), np.abs(s).sum(axis=0)


def _q(Q, mutate):
    Q = np.asarray(Q, dtype=np.float64)
    if mutate == "transpose_q":
        Q = Q.T
    if mutate == "drop_k_term":
        Q = Q.copy()
        Q[Q.shape[0] // 3, :] = 0       # one K-term of every r x r product
    return Q


def side_outputs(new, num, len_valid, part_rows, *, image_zero_past_valid=True, mutate=None):
    """What the update leaves for the next launch, from the new rows and the numerator the kernel multiplied with:
    ps(y) = sum_c new num (y < len_valid), sumsq_part (one vector per `part_rows` rows), gram_partial (one 64 x 64 matrix per 64 rows),
    colsq_part (one vector per 32 rows), image (the new rows; rows >= len_valid zero where the kernel masks them)."""
    len_pad, RP = new.shape
    lv = len_valid - 1 if mutate == "len_valid_off_by_one" else len_valid
    out = {"ps": (new * num).sum(axis=1)[:lv], "sumsq_part": (new ** 2).reshape(len_pad // part_rows, part_rows, RP).sum(axis=1),
           "colsq_part": (new ** 2).reshape(len_pad // 32, 32, RP).sum(axis=1) if len_pad % 32 == 0 else None}
    image = new.copy()
    if image_zero_past_valid:
        image[lv:] = 0
    out["image"] = image
    if RP == 64 and len_pad % 64 == 0:
        blocks = new.reshape(len_pad // 64, 64, 64)
        out["gram_partial"] = np.einsum("bya,byc->bac", blocks, blocks)
    return out


def side_bounds(new_abs, b_new, num_abs, b_num, len_valid, part_rows, u):
    """Absolute bounds of the side outputs for any summation order, from element-wise bounds b_new, b_num on the new rows and on the numerator:
    every product carries the factors' errors, the sum of n products adds gamma(n) of the sum of their magnitudes."""
    len_pad, RP = new_abs.shape
    hn, hm = new_abs + b_new, num_abs + b_num          # the largest magnitudes the kernel can hold
    out = {"ps": ((b_new * hm + new_abs * b_num) + gamma(RP, u) * hn * hm).sum(axis=1)[:len_valid]}
    sq = lambda rows: ((2 * new_abs * b_new + b_new ** 2) + gamma(rows, u) * hn ** 2).reshape(len_pad // rows, rows, RP).sum(axis=1)
    out["sumsq_part"], out["colsq_part"] = sq(part_rows), (sq(32) if len_pad % 32 == 0 else None)
    if RP == 64 and len_pad % 64 == 0:
        a, b, h = new_abs.reshape(-1, 64, 64), b_new.reshape(-1, 64, 64), hn.reshape(-1, 64, 64)
        out["gram_partial"] = np.einsum("bya,byc->bac", a, b) + np.einsum("bya,byc->bac", b, a) + np.einsum("bya,byc->bac", b, b) + gamma(64, u) * np.einsum("bya,byc->bac", h, h)
    return out


def panel_update(mode, P, slabs, Q, len_valid, eps, part_rows, u, *, split_q=False, mutate=None):
    """launch_panel_update's semantics.  Returns dict: new, num, b_new, b_num (element-wise bounds for unit roundoff u), the side outputs and their bounds.
    Roundings counted (S slabs, RP the padded rank):
      num                      S - 1 additions
      MODE_MU  old * num       + 1;   den: RP products and RP - 1 additions, + eps: RP + 1;   the division: + 1         => gamma(S + RP + 2) * new
      MODE_LS  the dot product of num with a column of Q: RP products, RP - 1 additions on top of num's            => gamma(S + RP - 1) * (|Q|^T |num|)
      split_q  every product of the r x r operand additionally drops terms of at most SPLIT_DROP |a b|: two more units of roundoff per product"""
    P = np.asarray(P, dtype=np.float64)
    len_pad, RP = P.shape
    S = slabs.shape[0]
    num, num_abs = numerator(slabs, len_pad, RP, mutate)
    Qm = _q(Q, mutate)
    b_num = gamma(max(S - 1, 1), u) * num_abs if S > 1 else 0 * num_abs
    extra = int(round(SPLIT_DROP / u)) if split_q else 0
    if mode == "mu":
        den = P @ Qm
        new = P * num / (den + (0 if mutate == "no_eps" else eps))
        new_abs = new
        b_new = gamma(S + RP + 2 + extra, u) * new_abs
    elif mode == "ls":
        dot = num @ Qm
        new = np.maximum(dot, 0)
        new_abs = np.abs(new)
        b_new = gamma(S + RP - 1 + extra, u) * (num_abs @ np.abs(Qm))
    else:
        new, new_abs, b_new = num, num_abs, b_num
    out = {"new": new, "num": num, "b_new": b_new, "b_num": b_num, "new_abs": new_abs, "num_abs": num_abs}
    out.update(side_outputs(new, num, len_valid, part_rows, mutate=mutate))
    out["bounds"] = side_bounds(new_abs, b_new, num_abs, b_num, len_valid, part_rows, u)
    return out


def smoothing(x, off, diag, r):
    """S x over the first r entries of every row, S = (diag - off) I + off 1 1^T; entries from r on come out zero."""
    y = np.zeros_like(x)
    y[:, :r] = (diag - off) * x[:, :r] + off * x[:, :r].sum(axis=1, keepdims=True)
    return y


def combine_q(Q, scale, qsplit):
    """The r x r operand of the K-split Gram passengers: the slices added in order, then scaled on both sides, (sum * scale[column]) * scale[row]."""
    Q = np.asarray(Q, dtype=np.float64).reshape(max(qsplit, 1), 64, 64)
    if qsplit <= 1:
        return Q[0]
    s = np.asarray(scale, dtype=np.float64)
    return (Q.sum(axis=0) * s[None, :]) * s[:, None]


def mu64_update(is_w, P, slabs, Q, scale, len_valid, eps, u, *, tile=32, Gprev=None, qsplit=0, ns=None, mutate=None):
    """The rank-64 fused multiplicative update (kernels_mu64.hip, header; kernels.h at launch_mu64_update / launch_mu64_update32).
      H side: num = scale (.) sum(slabs);  new = old num / (Q old + eps);  ps(y) = sum_c new num
      W side: old' = old (.) scale;        new = old' num / (Q old' + eps) (kept unnormalised);  ps(d) = sum_i Q[i, d] Gprev[d, i]
      qsplit: Q = combine_q(slices);   ns = (off, diag, r): num = S D sum(slabs), den = S Q (S old), image of S new, the panel keeps new.
    The 32-column kernel reads its r x r operand by rows, den(c) = sum_k Q[c, k] old(k) (its comment: "Q is symmetric: a row is a column"), the 64-column kernel
    and every launch_panel_update form by columns, den(c) = sum_k Q[k, c] old(k): with the symmetric matrices the engine passes the two are the same, and the
    tests give the 32-column kernel symmetric matrices (docs/PANEL_UPDATE.md, "Orientation of Q").
    Roundings: num S (the scale included), old' 1; den 64 products and 63 additions on top of its operands, + eps; with qsplit the operand carries qsplit + 1;
    with ns every smoothed vector carries 65 more (63 additions, two products, one addition)."""
    P = np.asarray(P, dtype=np.float64)
    len_pad = P.shape[0]
    S = slabs.shape[0]
    scale = np.asarray(scale, dtype=np.float64)
    num, _ = numerator(slabs, len_pad, 64, mutate)
    wrong = mutate == "scale_wrong_side"
    on_old = bool(is_w) != wrong
    old = P * scale[None, :] if on_old else P
    num = num if on_old else num * scale[None, :]
    Qf = _q(combine_q(Q, scale, qsplit), mutate)
    d_q = qsplit + 1 if qsplit > 1 else 0
    d_num, d_old = S - 1 + (0 if on_old else 1), (1 if on_old else 0)
    vec = old
    if ns is not None:
        off, diag, r = ns
        num = smoothing(num, off, diag, r)
        vec = smoothing(old, off, diag, r)
        d_num += 65
    t = vec @ Qf
    d_den = d_q + d_old + (65 if ns is not None else 0) + 1 + 63
    den = t
    if ns is not None:
        den = smoothing(t, off, diag, r)
        den[:, r:] = t[:, r:]            # (rows past r: old value 0, the quotient is never used)
        d_den += 65
    new = old * num / (den + (0 if mutate == "no_eps" else eps))
    depth = (d_old + d_num + 1) + (d_den + 1) + 1
    b_new = gamma(depth, u) * new
    b_num = gamma(max(d_num, 1), u) * num
    image_src, b_img = new, b_new
    if ns is not None:
        image_src = smoothing(new, off, diag, r)
        b_img = gamma(depth + 65, u) * image_src
    out = {"new": new, "num": num, "b_new": b_new, "b_num": b_num, "q_out": Qf if qsplit > 1 else None, "b_q_out": gamma(max(d_q, 1), u) * np.abs(Qf), "depth": depth}
    side = side_outputs(new, num, len_valid, 32, mutate=mutate)
    bounds = side_bounds(new, b_new, num, b_num, len_valid, 32, u)
    lv = len(side["ps"])
    image = image_src.copy(); image[lv:] = 0
    out["image"], out["b_image"] = image, b_img
    if is_w:
        side["ps"] = None if Gprev is None else (np.asarray(Q, dtype=np.float64).reshape(64, 64) * np.asarray(Gprev, dtype=np.float64).T).sum(axis=0)
        bounds["ps"] = None if Gprev is None else gamma(64, u) * (np.abs(np.asarray(Q, dtype=np.float64).reshape(64, 64)) * np.abs(np.asarray(Gprev, dtype=np.float64).T)).sum(axis=0)
    for k in ("ps", "sumsq_part", "colsq_part", "gram_partial"):
        out[k] = side[k]
    out["bounds"] = bounds
    return out


def fused_update(P, slabs, Q, len_valid, eps, part_rows, u, *, old_scale=None, h_side=False, scale=None, smooth=False, off=0.0, diag=1.0, r=0, split_q=False,
                 mutate=None):
    """The multiplicative update of the fused iterations (PanelFusedF32 / PanelFusedF64, kernels.h):
      W side: old' = old (.) old_scale;  new = old' num / (Q^T-product of old' + eps), kept unnormalised
      H side: Q is the raw Gram matrix of the unnormalised panel, D = diag(scale) (ones when absent; zero from r on with smoothing), S the smoothing matrix:
              num' = S D num,  u = D S old,  den = S D (Q u),  new = old num' / (den + eps);  smooth_out = S new;  the image is that of S new (of new without smoothing)
    Every S and D adds its roundings to the path; the bound is gamma(depth) on the expression evaluated with absolute values, which here (all operands
    non-negative) is the expression itself."""
    P = np.asarray(P, dtype=np.float64)
    len_pad, RP = P.shape
    S = slabs.shape[0]
    num, _ = numerator(slabs, len_pad, RP, mutate)
    Qm = _q(Q, mutate)
    extra = int(round(SPLIT_DROP / u)) if split_q else 0
    wrong = mutate == "scale_wrong_side"
    if not h_side:
        os_ = np.ones(RP) if old_scale is None else np.asarray(old_scale, dtype=np.float64)
        old = P if wrong else P * os_[None, :]
        if wrong:
            num = num * os_[None, :]
        den = old @ Qm
        new = old * num / (den + (0 if mutate == "no_eps" else eps))
        depth = (1 + S - 1 + 1) + (1 + RP + extra + 1) + 1
        smooth_out, image_src, b_extra = None, new, 0
    else:
        d = np.ones(RP) if scale is None else np.asarray(scale, dtype=np.float64).copy()
        sm = (lambda x: smoothing(x, off, diag, r)) if smooth else (lambda x: x)
        if smooth:
            d[r:] = 0
        ds = RP + 2 if smooth else 0                # roundings of one application of S
        if wrong:
            num_p, uvec = sm(num), sm(P * d[None, :])
        else:
            num_p, uvec = sm(num * d[None, :]), sm(P) * d[None, :]
        den = sm((uvec @ Qm) * d[None, :])
        new = P * num_p / (den + (0 if mutate == "no_eps" else eps))
        depth = (S + ds + 1) + (ds + 1 + RP + extra + 1 + ds + 1) + 1
        num = num_p
        smooth_out = sm(new) if smooth else None
        image_src, b_extra = (smooth_out, ds) if smooth else (new, 0)
    b_new = gamma(depth, u) * new
    b_num = gamma(S + (RP + 3 if h_side and smooth else 1), u) * num
    out = {"new": new, "num": num, "b_new": b_new, "b_num": b_num, "smooth_out": smooth_out, "image": image_src, "b_image": gamma(depth + b_extra, u) * image_src,
           "depth": depth}
    side = side_outputs(new, num, len_valid, part_rows, image_zero_past_valid=False, mutate=mutate)
    for k in ("ps", "sumsq_part"):
        out[k] = side[k]
    out["bounds"] = side_bounds(new, b_new, num, b_num, len_valid, part_rows, u)
    return out
