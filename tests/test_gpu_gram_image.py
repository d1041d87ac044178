"""The rank-64 Gram matrix from the split image (gram_image.h), one launch at a time through na.op_gram_image, element by element against the restatement of
tests/gram_reference.py on the cases of tests/gram_cases.py (docs/GRAM.md; tests/test_gram_cpu.py checks restatement, cases and bounds without a device).

Forms: one (sixteen workgroups, the finished matrix), ksplit2 / 4 / 8 (unscaled slices), spread (up to three unscaled pieces per tile), spread_finish (the last
workgroup adds and scales them into spread_out, the counter word returns to zero).  Every form stand-alone (k_gram_image) and riding as the passenger workgroups
of the split-operand product: x-tiled and y-tiled over the 16-row image (the whole problem's two forms), and x-tiled over 128-row tiles with col_split = 2 (128 x 32
workgroups, two to a CU, one slab: a narrow column shard's V H^T, the production instantiation with its own register cap, passenger offset and LDS size).

What every launch is held to:
  values     every slice, piece, scale and finished element within its derived bound; the exact kinds (ints, pow2, planes) as bits -- one dropped kept term moves a
             bit of a planes case
  symmetry   every unscaled output -- G, every slice and piece, spread_out -- is exactly symmetric; a SCALED element is (v s[c]) s[r], rounded twice, so (r, c) and
             (c, r) may differ in the last bit wherever they are scaled one by one: inside the diagonal tiles of the one-slice form, everywhere in spread_out,
             which is instead held as bits to that function of the pieces and scales the launch left (docs/GRAM.md, "Findings")
  untouched  outputs start as NaN (the pieces of the spread form as the zeros of their one clear): absent pieces are still zero, the matrix behind the last slice
             is still NaN, a missing scale is not written
and across launches: riding returns the stand-alone bits, the product's bits do not depend on its passengers, a second spread launch into the same buffers
returns the same bits, and the launcher refuses what the kernel cannot serve."""
import functools

import numpy as np
import pytest

import nmfgpu_amd as na
from tests import gram_cases as gc
from tests import gram_reference as gr

pytestmark = pytest.mark.gpu

WORST = {}      # (form, output) -> worst error / bound of the random cases, printed when the module is done
INVALID_ARGUMENT = 1
CASES = gc.image_cases()
CASE = dict(CASES)


@pytest.fixture(scope="module", autouse=True)
def _report():
    assert na.device_count() >= 1, "GPU tests need a HIP device"
    yield
    for (form, output), ratio in sorted(WORST.items()):
        print(f"\nworst error / bound  image {form:<14} {output:<10}: {ratio:.3g}", end="")
    print()


def form_args(form):
    return dict(ksplit=int(form[6:]) if form.startswith("ksplit") else 0, spread=int(form.startswith("spread")), finish=form == "spread_finish")


@functools.lru_cache(maxsize=None)
def panel_of(cid):
    c = CASE[cid]
    P = gc.panel(c["kind"], c["length"], c["r"], zero_col=c["zero_col"])
    P.setflags(write=False)
    return P


@functools.lru_cache(maxsize=None)
def product():
    rng = np.random.default_rng(5)
    A = np.asfortranarray(rng.uniform(0, 1, (200, 300)).astype(np.float32))
    F = np.asfortranarray(rng.uniform(0, 1, (64, 300)).astype(np.float32))
    return A, F


def variants(form, c):
    """(label, colsq_part, normalize) a form is run with: unscaled, the scales from the sums of squares, and (one slice only) from the product's own diagonal."""
    exact = c["kind"] != "random"
    cs = gc.colsq("pow2" if exact else "random", 9, c["r"], zero_col=c["zero_col"])
    out = [("raw", None, 0), ("colsq", cs, 1)]
    if form == "one":
        out.append(("diag", None, 1))
    return out


def check(form, cid, got, P, cs, normalize, tag=""):
    c = CASE[cid]
    fa = form_args(form)
    ref = gr.gram_image(P, colsq_part=cs, normalize=normalize, ksplit=fa["ksplit"], spread=fa["spread"])
    mask = gc.exact_mask(c["kind"], P)
    exact = c["kind"] != "random"
    # the scales are exact where the sum of squares is a power of four: the caller-built sums of the exact kinds, and the diagonal of a pow2 panel
    scale_exact = exact and (not normalize or cs is not None or c["kind"] == "pow2")
    scaled_exact = scale_exact
    slices = got["slices"]
    G = got["G"]
    assert np.isnan(G[slices:]).all(), f"{form} {tag}: the matrix behind the last slice was written"
    if form == "one":
        assert slices == 1 and got["workgroups"] == 16
        gr.held(f"{form} {tag} G", G[0], ref["G"], mask if scaled_exact else None, WORST, (form, "G " + tag))
        # the mirrored tile is written from the same values; INSIDE a diagonal tile (r, c) and (c, r) are scaled one by one, (v s[c]) s[r] against (v s[r]) s[c]
        off = np.ones((64, 64), bool) if not normalize else (np.arange(64)[:, None] // 16 != np.arange(64)[None, :] // 16)
        assert np.array_equal(gr.bits(np.where(off, G[0], 0)), gr.bits(np.where(off, G[0], 0).T.copy())), f"{form} {tag} G: not symmetric"
    else:
        assert slices == (3 if fa["spread"] else fa["ksplit"]) and got["workgroups"] == (16 if fa["spread"] else 10 * fa["ksplit"])
        for s in range(slices):
            gr.held(f"{form} {tag} slice {s}", G[s], (ref["G"][0][s], ref["G"][1][s]), mask if exact else None, WORST, (form, "pieces"))
            assert np.array_equal(gr.bits(G[s]), gr.bits(G[s].T.copy())), f"{form} {tag} slice {s}: not symmetric"
    pairs = got["pairs"]
    assert (got["image_ks"], pairs) == gr.image_geometry(c["length"])
    gr.held(f"{form} {tag} scale", got["scale"], ref["scale"], np.array(scale_exact), WORST, (form, "scale " + tag))
    if fa["finish"]:
        for i, out in enumerate(got["spread_out"]):
            gr.held(f"{form} {tag} spread_out {i}", out, ref["spread_out"], mask if scaled_exact else None, WORST, (form, "spread_out"))
            # an exact function of the pieces and scales the launch left: ((p0 + p1) + p2), then the two products, element by element
            tot = ((G[0] + G[1]).astype(np.float32) + G[2]).astype(np.float32)
            assert np.array_equal(gr.bits(out), gr.bits(gr.scaled_matrix_fp32(tot, got["scale"]))), f"{form} {tag} spread_out: not ((p0 + p1) + p2) s[c] s[r]"
            if not normalize:
                assert np.array_equal(gr.bits(out), gr.bits(out.T.copy())), f"{form} {tag} spread_out: not symmetric"
            assert np.array_equal(gr.bits(out), gr.bits(got["spread_out"][0])), f"{form} {tag} spread_out: launch {i} differs from launch 0"
        assert got["counter"] == [0] * len(got["counter"]), f"{form} {tag} counter after the launches: {got['counter']}"
    else:
        assert np.isnan(got["spread_out"]).all(), f"{form} {tag}: spread_out written without a request"


@pytest.mark.parametrize("cid", [i for i, _ in CASES])
@pytest.mark.parametrize("form", gc.IMAGE_FORMS)
def test_image_standalone_f32(form, cid):
    P = panel_of(cid)
    for tag, cs, nz in variants(form, CASE[cid]):
        got = na.op_gram_image(P, colsq_part=cs, normalize=nz, launches=2 if form == "spread_finish" else 1, **form_args(form))
        check(form, cid, got, P, cs, nz, tag)


@pytest.mark.parametrize("cc", [i for i, _ in gc.image_colsq_cases()])
@pytest.mark.parametrize("form", ["one", "ksplit2", "spread_finish"])
def test_image_scale_sums_f32(form, cc):
    """The batches of the scale sums: 40 parts per thread group and round trip, stride 320 -- config 2 stops at 316."""
    q = dict(gc.image_colsq_cases())[cc]
    cid = "len100-r64-random" if q["kind"] == "random" else "len100-r61-pow2-zero5"
    P = panel_of(cid)
    cs = gc.colsq(q["kind"], q["parts"], CASE[cid]["r"], zero_col=q["zero_col"])
    got = na.op_gram_image(P, colsq_part=cs, normalize=1, **form_args(form))
    check(form, cid, got, P, cs, 1, "colsq")


@pytest.mark.parametrize("cid", ["len17-r64-random", "len100-r64-random", "len257-r64-planes", "len1301-r64-random", "len33-r61-pow2-zero5"])
@pytest.mark.parametrize("ride", [1, 2, 3], ids=["xtiled", "ytiled", "colsplit"])
@pytest.mark.parametrize("form", gc.IMAGE_FORMS)
def test_image_riding_returns_the_standalone_bits_f32(form, ride, cid):
    P = panel_of(cid)
    plain = None
    for tag, cs, nz in variants(form, CASE[cid]):
        kw = dict(colsq_part=cs, normalize=nz, **form_args(form))
        alone = na.op_gram_image(P, **kw)
        rode = na.op_gram_image(P, ride=ride, product=product(), **kw)
        check(form, cid, rode, P, cs, nz, tag)
        for name in ("G", "scale", "spread_out"):
            assert np.array_equal(gr.bits(rode[name]), gr.bits(alone[name])), f"{form} {tag} riding {ride}: {name} differs from the stand-alone launch"
        assert rode["counter"] == alone["counter"] and rode["workgroups"] == alone["workgroups"]
        if ride == 3:
            assert rode["splits"] == 1 and rode["xtiles"] == 2
        assert np.isfinite(rode["out_ride"]).all()
        assert np.array_equal(gr.bits(rode["out_ride"]), gr.bits(rode["out_plain"])), f"{form} {tag}: the product's bits change with passengers aboard"
        plain = rode["out_plain"] if plain is None else plain
        assert np.array_equal(gr.bits(plain), gr.bits(rode["out_plain"]))
    A, F = product()
    exact = F.astype(np.float64) @ A.astype(np.float64).T
    assert np.abs(plain - exact).max() <= 1e-5 * np.abs(exact).max()          # (the product itself: tests/test_gpu_parity.py holds it element-wise)


@pytest.mark.parametrize("cid", ["len1-r64-random", "len32-r64-ints", "len100-r64-random", "len257-r64-planes"])
def test_spread_finish_without_scale_and_launched_three_times_f32(cid):
    """No scale buffer: spread_out is the plain sum of the pieces.  Three launches into the same pieces and counter, nothing cleared between them."""
    P = panel_of(cid)
    got = na.op_gram_image(P, spread=1, finish=True, with_scale=False, launches=3)
    assert got["scale"] is None and got["counter"] == [0, 0, 0]
    ref = gr.gram_image(P, spread=1)
    mask = gc.exact_mask(CASE[cid]["kind"], P)
    for out in got["spread_out"]:
        gr.held("spread_out", out, ref["spread_out"], mask if CASE[cid]["kind"] != "random" else None, WORST, ("spread_finish", "spread_out"))
        assert np.array_equal(gr.bits(out), gr.bits(got["spread_out"][0]))
    for s in range(3):
        gr.held(f"piece {s}", got["G"][s], (ref["G"][0][s], ref["G"][1][s]), mask if CASE[cid]["kind"] != "random" else None)


def test_refusals_run_no_kernel():
    P = panel_of("len100-r64-random")
    cs = gc.colsq("random", 9, 64)

    def refused(**kw):
        with pytest.raises(na.EngineError) as e:
            na.op_gram_image(kw.pop("P", P), **kw)
        assert e.value.status == INVALID_ARGUMENT, e.value

    refused(ksplit=gr.KSPLIT_MAX + 1)
    refused(ksplit=16, colsq_part=cs, normalize=1)
    refused(ksplit=2, normalize=1)                            # the scales of a slice's diagonal
    refused(spread=1, normalize=1)                            # ... and of a piece's: refused since this test exists
    refused(spread=1, finish=True, normalize=1)
    refused(P=None, length=100)                               # no image
    for ride in (1, 2, 3):
        refused(spread=1, normalize=1, ride=ride, product=product())
        refused(ksplit=2, normalize=1, ride=ride, product=product())
        refused(ksplit=9, ride=ride, product=product())
    # ... and the same requests with the sums of squares are served
    na.op_gram_image(P, spread=1, finish=True, normalize=1, colsq_part=cs)
    na.op_gram_image(P, ksplit=8, normalize=1, colsq_part=cs)
