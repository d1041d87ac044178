"""The restatement of the Gram-matrix kernels (tests/gram_reference.py) and its cases (tests/gram_cases.py) checked without a device (docs/GRAM.md): the exact
constructions do what they say, the ranges of slices and pieces tile the K range, and every defect of MUTATIONS leaves the bounds -- or moves a bit of an exact
case -- on at least one case of every form that can exhibit it.  The GPU modules rely on all of this."""
import numpy as np
import pytest

from tests import gram_cases as gc
from tests import gram_reference as gr
from tests.test_split3 import round_bf16, split3

F32 = np.float32


def _representable(v):
    v = np.asarray(v, dtype=np.float64)
    return v.astype(F32).astype(np.float64) == v


# ---- the constructions ----------------------------------------------------------------------------------------------------------------------------------

def test_plane_values_have_single_bit_planes_and_six_distinct_kept_bits():
    a, b = F32(gc.A_PLANES), F32(gc.B_PLANES)
    assert float(a) == gc.A_PLANES and float(b) == gc.B_PLANES                       # fp32 values
    pa = [float(x) for x in split3(a)[:3]]
    pb = [float(x) for x in split3(b)[:3]]
    assert pa == [1.0, 2.0 ** -9, 2.0 ** -18] and pb == [1.0, 2.0 ** -10, 2.0 ** -20]
    kept = sorted(pa[i] * pb[j] for i, j in gr.KEPT)
    assert kept == sorted([1.0, 2.0 ** -9, 2.0 ** -10, 2.0 ** -18, 2.0 ** -19, 2.0 ** -20])            # each term a bit of its own
    total = sum(kept)
    assert _representable(total)
    dropped = [pa[i] * pb[j] for i, j in gr.DROPPED]
    assert max(dropped) < np.spacing(F32(total)) / 2 and sum(dropped) < np.spacing(F32(total)) / 2      # below the last bit of the result
    for t in range(6):        # dropping any one kept term moves the fp32 result
        rest = sum(pa[i] * pb[j] for k, (i, j) in enumerate(gr.KEPT) if k != t)
        assert _representable(rest) and F32(rest) != F32(total)
    # ... and the square of either value (the diagonal) is exact as well
    for p in (pa, pb):
        assert _representable(sum(p[i] * p[j] for i, j in gr.KEPT))


@pytest.mark.parametrize("length,r,RP", [(17, 64, 64), (257, 64, 64), (1301, 64, 64), (48, 1, 64), (257, 256, 256)])
def test_planes_panels_are_exact_where_the_mask_says(length, r, RP):
    P = gc.panel("planes", length, r, RP)
    mask = gc.exact_mask("planes", P)
    pl = gr.planes(P)
    v, m = gr.six_term(pl, 0, length)
    assert _representable(v[mask]).all() and mask[:r, :r][np.triu_indices(r, 1)].all()       # every off-diagonal element is exact
    # every prefix of the panel rows is exact too: any slice, piece or wave range
    for y1 in (1, 16, 32, length // 2):
        assert _representable(gr.six_term(pl, 0, y1)[0][mask]).all()
    hit = (v != 0) & mask
    assert hit.any()
    for t in range(6):
        vt = gr.six_term(pl, 0, length, mutate=f"drop_term_{t}")[0]
        assert (vt[hit].astype(F32) != v[hit].astype(F32)).all(), t             # one dropped kept term moves EVERY touched exact element
    assert gr.dropped_terms_ratio(P[:64]) < 2.0 ** -26


@pytest.mark.parametrize("kind", ["ints", "pow2"])
def test_exact_kinds_are_exact(kind):
    P = gc.panel(kind, 1301, 61, zero_col=5)
    pl = gr.planes(P)
    assert np.array_equal(pl[1], np.zeros_like(pl[1])) and np.array_equal(pl[2], np.zeros_like(pl[2]))      # bf16 values: one plane
    v, m = gr.six_term(pl, 0, 1301)
    assert np.array_equal(v, P.astype(np.float64).T @ P.astype(np.float64)) and m.max() < 2 ** 24 and _representable(v).all()
    if kind == "pow2":
        d = np.diag(v)[:61]
        assert d[5] == 0 and np.array_equal(np.delete(d, 5), 4.0 ** np.round(np.log2(np.delete(d, 5)) / 2))
        s, sb = gr.rsqrt_scale(np.diag(v).copy(), 0.0)
        assert s[5] == 1.0 and _representable(s).all() and _representable(v * s[None, :] * s[:, None]).all()
    Q = gc.colsq("pow2", 400, 61, zero_col=9)
    q = Q.astype(np.float64).sum(axis=0)
    assert q[9] == 0 and (np.log2(np.delete(q[:61], 9)) % 2 == 0).all()
    for lo, hi in ((0, 40), (0, 320), (320, 400)):          # one non-zero part in every batch the kernels form
        assert (Q[lo:hi, 0] != 0).any()


def test_dropped_terms_stay_below_2_to_minus_22_and_the_kept_sum_is_the_product():
    for n, r in ((100, 64), (129, 1), (257, 64)):
        P = gc.panel("random", n, r)
        assert gr.dropped_terms_ratio(P) <= 2.0 ** -22
        v, m = gr.six_term(gr.planes(P), 0, n)
        exact = P.astype(np.float64).T @ P.astype(np.float64)
        assert (np.abs(v - exact) <= 2.0 ** -22 * (np.abs(P).astype(np.float64).T @ np.abs(P).astype(np.float64)) + 1e-300).all()
        assert (m >= np.abs(v)).all() and np.array_equal(v, v.T)


def test_pack_panel_layout_round_trips():
    P = gc.panel("random", 37, 64)
    bits = gr.pack_panel_x3(P, 3).reshape(3, 2, 3, 2, 32, 8)
    vals = (bits.astype(np.uint32) << 16).view(F32)
    for ks, nb, h, r, j in ((0, 0, 0, 0, 0), (2, 1, 0, 31, 4), (1, 1, 1, 7, 7), (2, 0, 1, 3, 0)):
        y, c = 16 * ks + 8 * h + j, 32 * nb + r
        want = P[y, c] if y < 37 else F32(0)
        assert F32(vals[ks, nb, 0, h, r, j] + vals[ks, nb, 1, h, r, j] + vals[ks, nb, 2, h, r, j]) == want
        assert vals[ks, nb, 0, h, r, j] == round_bf16(want)
    full = vals.astype(np.float64).sum(axis=2)                     # [ks][nb][h][r][j]
    back = full.transpose(0, 2, 4, 1, 3).reshape(48, 64)
    assert np.array_equal(back[:37], P.astype(np.float64)) and not back[37:].any()


# ---- ranges ---------------------------------------------------------------------------------------------------------------------------------------------

def test_spread_deal_tiles_every_tile_in_at_most_three_pieces():
    lens = set(gc.IMAGE_LENS) | set(range(1, 700, 13))
    for n in sorted(lens):
        ks, pairs = gr.image_geometry(n)
        assert 32 * pairs >= 16 * ks + 16 or ks % 2 == 1                      # an even KS ends in a pair of zero steps, an odd one in one zero step
        deal = gr.spread_deal(pairs)
        for t in range(gr.IMAGE_TILES):
            mine = sorted((p, a, b) for _, tt, p, a, b in deal if tt == t)
            assert [p for p, _, _ in mine] == list(range(len(mine))) and len(mine) <= gr.SPREAD_SLICES, (n, t, mine)
            assert mine[0][1] == 0 and mine[-1][2] == pairs and all(x[2] == y[1] for x, y in zip(mine, mine[1:])), (n, t, mine)
        busy = {blk for blk, *_ in deal}
        if 10 * pairs < 16:
            assert len(busy) < 16                                           # empty workgroups: the cases with len <= 32
    assert any(len([1 for _, tt, *_ in gr.spread_deal(gr.image_geometry(n)[1]) if tt == 0]) == 1 for n in gc.IMAGE_LENS)      # a tile in one piece
    # pairs = 8 (len 225, a case of the GPU modules): sixteen workgroups of exactly five pairs
    assert 225 in gc.IMAGE_LENS and gr.image_geometry(225)[1] == 8
    assert [sum(b - a for blk, *_, a, b in gr.spread_deal(8) if blk == w) for w in range(16)] == [5] * 16


@pytest.mark.parametrize("cid,c", gc.image_cases(), ids=[i for i, _ in gc.image_cases()])
def test_slices_and_pieces_add_up_to_the_one_slice_matrix(cid, c):
    P = gc.panel(c["kind"], c["length"], c["r"], zero_col=c["zero_col"])
    one = gr.gram_image(P)["G"][0]
    exact = c["kind"] != "random"
    for form in ("ksplit2", "ksplit4", "ksplit8", "spread"):
        k = int(form[6:]) if form.startswith("ksplit") else 0
        pieces = gr.gram_image(P, ksplit=k, spread=int(form == "spread"))["G"][0]
        tot = pieces.sum(axis=0)
        assert np.array_equal(tot, one) if exact else np.allclose(tot, one, rtol=1e-12, atol=1e-12), form
        assert np.array_equal(pieces, pieces.transpose(0, 2, 1))


def test_wide_slice_counts_step_where_the_cases_say():
    assert [gr.wide_parts(128, n, 16) for n in (63, 64, 127, 128, 129, 1000)] == [1, 1, 1, 2, 2, 15]
    assert gr.wide_parts(128, 1000, 128) == 15 and gr.wide_parts(128, 100000, 128) == 128 and gr.wide_parts(384, 100000, 128) == 85
    for cid, c in gc.wide_cases():
        P = gc.panel(c["kind"], c["length"], c["r"], RP=c["RP"], zero_col=c["zero_col"])
        parts = gr.wide_parts(c["RP"], c["length"], c["parts"])
        v, b, wr = gr.gram_wide_slices(P, c["RP"], parts, True)
        whole = gr.six_term(gr.planes(P), 0, c["length"])[0]
        assert np.allclose(v.sum(axis=0), whole, rtol=1e-12, atol=1e-12), cid
        if c["RP"] != 128:          # (every case of RP 128, the first of the ranks above)
            break


# ---- defects --------------------------------------------------------------------------------------------------------------------------------------------

def _moved(ref, mut, exact_mask):
    """(beyond twice the bound anywhere, any bit of the exact elements) for a pair of (value, bound) results."""
    (v, b), (w, _) = ref, mut
    v, w, b = np.asarray(v), np.asarray(w), np.asarray(b)
    diff = np.where(np.isnan(w) | np.isnan(v), np.inf, np.abs(w - v))
    by_bound = bool((diff > 2 * b).any() and (diff > 0).any())
    m = np.broadcast_to(exact_mask, v.shape)
    by_bits = bool((diff[m] > 0).any()) if m.any() else False
    return by_bound, by_bits


def _image_outputs(form, c, colsq_part, normalize, mutate):
    P = gc.panel(c["kind"], c["length"], c["r"], zero_col=c["zero_col"])
    k = int(form[6:]) if form.startswith("ksplit") else 0
    res = gr.gram_image(P, colsq_part=colsq_part, normalize=normalize, ksplit=k, spread=int(form.startswith("spread")), mutate=mutate)
    if form != "spread_finish":
        res.pop("spread_out", None)
    return res, gc.exact_mask(c["kind"], P)


IMAGE_DEFECTS = {
    "one": ["drop_term_%d" % t for t in range(6)] + ["drop_last_pair", "no_mirror", "scale_wrong_source", "scale_once", "drop_colsq_batch"],
    "ksplit": ["drop_term_%d" % t for t in range(6)] + ["skip_boundary_step", "double_boundary_step", "drop_last_pair", "no_mirror", "scale_wrong_source",
               "drop_colsq_batch"],
    "spread": ["drop_term_%d" % t for t in range(6)] + ["skip_boundary_step", "double_boundary_step", "drop_last_pair", "no_mirror", "scale_wrong_source",
               "drop_colsq_batch"],
    "spread_finish": ["scale_wrong_source", "scale_once", "drop_spread_piece", "drop_colsq_batch"],
}
# what only the exact cases are sure to show: the bound of a random case is wider than the defect (docs/GRAM.md, "The limits of the defect checks")
ONLY_EXACT = {("one", "drop_term_0"), ("one", "drop_term_1"), ("one", "drop_term_2"), ("ksplit", "drop_term_0"), ("ksplit", "drop_term_1"), ("ksplit", "drop_term_2"),
              ("spread", "drop_term_0"), ("spread", "drop_term_1"), ("spread", "drop_term_2")}


def _image_defect(form_class, mutate):
    forms = {"one": ["one"], "ksplit": ["ksplit2", "ksplit4", "ksplit8"], "spread": ["spread"], "spread_finish": ["spread_finish"]}[form_class]
    by_bound = by_bits = False
    for form in forms:
        for cid, c in gc.image_cases():
            variants = [(None, 0)]
            if mutate in ("scale_wrong_source", "scale_once", "drop_colsq_batch"):
                exact = c["kind"] != "random"
                cs = gc.colsq("pow2" if exact else "random", 400, c["r"], zero_col=c["zero_col"])
                variants = [(cs, 1)] + ([(None, 1)] if form == "one" and mutate != "drop_colsq_batch" else [])
            for cs, nz in variants:
                ref, mask = _image_outputs(form, c, cs, nz, None)
                mut, _ = _image_outputs(form, c, cs, nz, mutate)
                for name in ref:
                    em = (mask.any(axis=0) if name == "scale" else mask) if c["kind"] != "random" else np.zeros((), bool)
                    if name == "scale" and c["kind"] != "random":
                        em = np.ones(64, bool)
                    bb, bx = _moved(ref[name], mut[name], em)
                    by_bound |= bb and c["kind"] == "random"
                    by_bits |= bx
    return by_bound, by_bits


@pytest.mark.parametrize("form_class,mutate", [(f, m) for f, ms in IMAGE_DEFECTS.items() for m in ms])
def test_image_defects_are_caught(form_class, mutate):
    by_bound, by_bits = _image_defect(form_class, mutate)
    assert by_bound or by_bits, "no case of this form shows the defect"
    assert by_bits, "the exact cases show every defect"
    assert (not by_bound) == ((form_class, mutate) in ONLY_EXACT), (by_bound, by_bits)


def test_mirror_from_the_lower_triangle_cannot_show_in_the_values():
    """Defect `mirror_lower`: the kept terms of (r, c) and of (c, r) are the same six products, so both triangles hold the same exact sum; which triangle a kernel
    mirrors moves the ORDER of the additions only.  No restatement can tell, and the bound holds either way; the kernels' outputs are asserted exactly symmetric."""
    P = gc.panel("random", 100, 64)
    pl = gr.planes(P)
    val = np.zeros((64, 64))
    for i, j in gr.KEPT:
        val += pl[i].T @ pl[j]
    assert np.allclose(val, val.T, rtol=1e-13, atol=0)
    Pp = gc.panel("planes", 100, 64)
    pp = gr.planes(Pp)
    raw = sum(pp[i].T @ pp[j] for i, j in gr.KEPT)
    assert np.array_equal(raw, raw.T)


@pytest.mark.parametrize("mutate", ["drop_quarter_slice", "scale_once", "scale_wrong_source"])
def test_reduction_defects_are_caught(mutate):
    seen_bound = seen_bits = False
    for parts in gc.REDUCE_PARTS:
        for kind in ("random", "pow2"):
            M = gc.partial_matrices(kind, parts)
            sq = gc.colsq("random" if kind == "random" else "pow2", 9, 64)
            for ref, mut in ((gr.gram_reduce(M, 1), gr.gram_reduce(M, 1, mutate)), (gr.gram_reduce_scale_all(M, sq), gr.gram_reduce_scale_all(M, sq, mutate))):
                bb, bx = _moved(ref["G"], mut["G"], np.array(kind != "random"))
                seen_bound |= bb and kind == "random"
                seen_bits |= bx
                bb, bx = _moved(ref["scale"], mut["scale"], np.array(kind != "random"))
                seen_bound |= bb and kind == "random"
                seen_bits |= bx
    assert seen_bound and seen_bits


WIDE_DEFECTS = ["drop_term_%d" % t for t in range(6)] + ["skip_boundary_step", "double_boundary_step", "no_mirror"]
WIDE_ONLY_EXACT = {"drop_term_0", "drop_term_1", "drop_term_2"}


@pytest.mark.parametrize("mutate", WIDE_DEFECTS)
def test_wide_slice_defects_are_caught(mutate):
    by_bound = by_bits = False
    for cid, c in gc.wide_cases():
        if c["RP"] > 256:
            continue
        P = gc.panel(c["kind"], c["length"], c["r"], RP=c["RP"], zero_col=c["zero_col"])
        parts = gr.wide_parts(c["RP"], c["length"], c["parts"])
        v, b, wr = gr.gram_wide_slices(P, c["RP"], parts, True)
        w, _, wm = gr.gram_wide_slices(P, c["RP"], parts, True, mutate)
        if mutate == "no_mirror":
            by_bits |= bool((wr != wm).any()); by_bound |= bool((wr != wm).any())
            continue
        bb, bx = _moved((v, b), (w, b), gc.exact_mask(c["kind"], P))
        by_bound |= bb and c["kind"] == "random"
        by_bits |= bx
    assert by_bits
    assert (not by_bound) == (mutate in WIDE_ONLY_EXACT)


@pytest.mark.parametrize("mutate", ["drop_quarter_slice", "no_mirror"])
def test_reduce_x3_defects_are_caught(mutate):
    by_bound = by_bits = False
    for parts in (1, 3, 9, 16):
        for kind in ("random", "ints"):
            S = gc.partial_matrices(kind, parts, C=128)
            ref, mut = gr.gram_reduce_x3(S, parts, 128), gr.gram_reduce_x3(S, parts, 128, mutate=mutate)
            bb, bx = _moved(ref["G"], mut["G"], np.array(kind != "random"))
            by_bound |= bb and kind == "random"
            by_bits |= bx
    assert by_bound and by_bits


def test_qx3_from_the_unmirrored_tile_moves_the_image():
    G = gr.gram_reduce_x3(gc.partial_matrices("random", 3, C=128), 3, 128)["G"][0].astype(F32)
    assert np.array_equal(G, G.T)
    assert not np.array_equal(gr.qx3_of(G), gr.qx3_of(G, mutate="qx3_unmirrored"))
    assert np.array_equal(gr.qx3_of(G), gr.pack_panel_x3(G, 8))
