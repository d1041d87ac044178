"""The fp32 Gram matrix at padded ranks 128 ... 512 (gram_wide.h, kernels_wide.hip), one launcher at a time through na.op_gram_wide, against the restatement of
tests/gram_reference.py on the cases of tests/gram_cases.py (docs/GRAM.md; tests/test_gram_cpu.py checks it without a device).

Routes:  0  launch_gram_wide_f32          k_gram_wide_x3<2> (slices mirrored), launch_reduce_partials
         1  launch_gram_wide_fused_f32    k_gram_wide_x3<2, false> (upper blocks only), k_gram_reduce_x3: G, its split image qx3, the pending scale
         2  launch_gram_reduce_x3         alone, on caller-built slices: NaN below the diagonal blocks and behind `parts`
         3  GramReduceArgs::wide_P        the slices as passenger workgroups of the NBW = 4 split-operand product (ring of four K-steps)

Held to: every slice against the restatement of its OWN K range, element by element (a row that lands in the neighbouring slice shows in both); which elements
of a slice a form writes (the rest is still NaN); G within the bound of its sum and exactly symmetric; qx3 as bits of split3(G) in k_pack_panel_x3's layout with
the closing K-step untouched; the scale; the exact kinds as bits; riding slices equal to the stand-alone slice kernel's; refusals."""
import functools

import numpy as np
import pytest

import nmfgpu_amd as na
from tests import gram_cases as gc
from tests import gram_reference as gr

pytestmark = pytest.mark.gpu

WORST = {}
INVALID_ARGUMENT = 1
CASES = gc.wide_cases()
CASE = dict(CASES)
NAN16 = 0x7FC0


@pytest.fixture(scope="module", autouse=True)
def _report():
    assert na.device_count() >= 1, "GPU tests need a HIP device"
    yield
    for (route, output), ratio in sorted(WORST.items()):
        print(f"\nworst error / bound  wide {route:<12} {output:<8}: {ratio:.3g}", end="")
    print()


@functools.lru_cache(maxsize=None)
def panel_of(cid):
    c = CASE[cid]
    P = gc.panel(c["kind"], c["length"], c["r"], RP=c["RP"], zero_col=c["zero_col"])
    P.setflags(write=False)
    return P


@functools.lru_cache(maxsize=None)
def slices_of(cid, mirror):
    """The restated slices of a case, computed once: (value, bound, written) for the settled slice count."""
    c = CASE[cid]
    return gr.gram_wide_slices(panel_of(cid), c["RP"], gr.wide_parts(c["RP"], c["length"], c["parts"]), mirror)


@functools.lru_cache(maxsize=None)
def product(r_prod):
    rng = np.random.default_rng(7)
    return (np.asfortranarray(rng.uniform(0, 1, (200, 300)).astype(np.float32)), np.asfortranarray(rng.uniform(0, 1, (r_prod, 300)).astype(np.float32)))


def settled(cid):
    c = CASE[cid]
    return gr.wide_parts(c["RP"], c["length"], c["parts"])


def symmetric(a):
    return np.array_equal(gr.bits(a), gr.bits(np.ascontiguousarray(a.T)))


def check_slices(route, cid, got, mirror):
    c = CASE[cid]
    RP, parts = c["RP"], gr.wide_parts(c["RP"], c["length"], c["parts"])
    assert got["parts"] == parts, (got["parts"], parts)
    val, bnd, wr = slices_of(cid, mirror)
    S = got["partial"]
    assert np.isnan(S[parts:]).all(), f"{route}: a slice behind the last one was written"
    mask = gc.exact_mask(c["kind"], panel_of(cid))
    for s in range(parts):
        assert np.isnan(S[s][~wr]).all(), f"{route} slice {s}: written outside what the form writes"
        assert np.isfinite(S[s][wr]).all(), f"{route} slice {s}: an element of the form's range is not written"
        got_s = np.where(wr, S[s], 0.0).astype(np.float32)
        gr.held(f"{route} slice {s}", got_s, (np.where(wr, val[s], 0.0), np.where(wr, bnd[s], 0.0)), mask if c["kind"] != "random" else None, WORST, (route, "slices"))
        both = wr & wr.T
        assert np.array_equal(gr.bits(np.where(both, S[s], 0)), gr.bits(np.ascontiguousarray(np.where(both, S[s], 0).T))), f"{route} slice {s}: mirror image differs"
    return val, bnd


def check_sum(route, cid, got, val, bnd):
    c = CASE[cid]
    tot = val.sum(axis=0)
    tb = bnd.sum(axis=0) + gr.sum_bound(val.shape[0] + 4, np.abs(val).sum(axis=0) + bnd.sum(axis=0))
    mask = gc.exact_mask(c["kind"], panel_of(cid))
    gr.held(f"{route} G", got["G"], (tot, tb), mask if c["kind"] != "random" else None, WORST, (route, "G"))
    assert symmetric(got["G"]), f"{route}: G is not symmetric"


@pytest.mark.parametrize("cid", [i for i, _ in CASES])
def test_gram_wide_f32(cid):
    got = na.op_gram_wide(0, CASE[cid]["RP"], P=panel_of(cid), parts=CASE[cid]["parts"], slices_alloc=settled(cid) + 1)
    val, bnd = check_slices("mirrored", cid, got, True)
    check_sum("mirrored", cid, got, val, bnd)


# (the part counts of the scale sums dealt over the cases in order; test_gram_reduce_x3_alone_f32 runs every count)
@pytest.mark.parametrize("cid,sq_parts", [(cid, gc.WIDE_SQ_PARTS[k % len(gc.WIDE_SQ_PARTS)]) for k, (cid, _) in enumerate(CASES)])
def test_gram_wide_fused_f32(cid, sq_parts):
    c = CASE[cid]
    RP = c["RP"]
    exact = c["kind"] != "random"
    sq = gc.colsq("pow2" if exact else "random", sq_parts, c["r"], RP=RP, zero_col=c["zero_col"])
    got = na.op_gram_wide(1, RP, P=panel_of(cid), parts=c["parts"], sumsq_part=sq, slices_alloc=settled(cid) + 1)
    val, bnd = check_slices("fused", cid, got, False)
    check_sum("fused", cid, got, val, bnd)
    check_image_and_scale("fused", got, RP, sq, exact)


def check_image_and_scale(route, got, RP, sq, exact):
    img = gr.qx3_of(got["G"])
    assert np.array_equal(got["qx3"][:img.size], img), f"{route}: qx3 is not the split image of the G the launch wrote"
    assert (got["qx3"][img.size:] == NAN16).all(), f"{route}: the closing K-step of qx3 was written"
    if sq is not None:
        q, qb = gr.colsq_sum(sq)
        gr.held(f"{route} scale", got["scale"], gr.rsqrt_scale(q, qb), np.array(exact), WORST, (route, "scale"))


# (the scale sums do not depend on the rank: every part count at RP 128, three of them above)
REDUCE_ALONE = [(128, parts, sq) for parts in (1, 3, 16) for sq in gc.WIDE_SQ_PARTS] + [(RP, parts, sq) for RP, parts in ((256, 9), (384, 33), (512, 5)) for sq in (1, 5, 33)]


@pytest.mark.parametrize("kind", ["random", "ints"])
@pytest.mark.parametrize("RP,parts,sq_parts", REDUCE_ALONE)
def test_gram_reduce_x3_alone_f32(RP, parts, sq_parts, kind):
    S = np.full((parts + 2, RP, RP), np.nan, np.float32)                 # NaN behind `parts` ...
    S[:parts] = gc.partial_matrices(kind, parts, C=RP, r=RP - 3)
    low = ~np.triu(np.ones((RP // 32, RP // 32), bool)).repeat(32, 0).repeat(32, 1)
    S[:, low] = np.nan                                                   # ... and on the blocks below the diagonal, which the slices never hold
    sq = gc.colsq("pow2" if kind == "ints" else "random", sq_parts, RP - 3, RP=RP, zero_col=2)
    got = na.op_gram_wide(2, RP, parts=parts, partial=S, sumsq_part=sq)
    ref = gr.gram_reduce_x3(np.nan_to_num(S), parts, RP)
    gr.held("reduce_x3 G", got["G"], ref["G"], np.array(kind != "random"), WORST, ("reduce_x3", "G"))
    assert symmetric(got["G"])
    assert np.array_equal(gr.bits(got["partial"]), gr.bits(S)), "the reduction wrote into its input"
    check_image_and_scale("reduce_x3", got, RP, sq, kind != "random")
    assert got["scale"][2] == 1.0


@pytest.mark.parametrize("cid", ["rp128-len17-parts16-random", "rp128-len129-parts16-random", "rp128-len1000-parts128-random", "rp128-len65-parts16-ints",
                                 "rp256-len257-parts16-planes", "rp384-len1000-parts128-random"])
def test_riding_slices_return_the_standalone_bits_f32(cid):
    """gram_wide_slice<4, false> as passengers against gram_wide_slice<2, false> as a launch of its own: the same device function with another ring depth, the
    K-steps of a slice added in the same order."""
    c = CASE[cid]
    RP = c["RP"]
    alone = na.op_gram_wide(1, RP, P=panel_of(cid), parts=c["parts"], slices_alloc=settled(cid) + 1)
    rode = na.op_gram_wide(3, RP, P=panel_of(cid), parts=c["parts"], product=product(RP), slices_alloc=settled(cid) + 1)
    check_slices("riding", cid, rode, False)
    assert rode["parts"] == alone["parts"]
    assert np.array_equal(gr.bits(rode["partial"]), gr.bits(alone["partial"])), "the riding slices differ from the stand-alone slice kernel's"
    assert np.isfinite(rode["out_ride"]).all()
    assert np.array_equal(gr.bits(rode["out_ride"]), gr.bits(rode["out_plain"])), "the product's bits change with passengers aboard"


def test_refusals_run_no_kernel():
    S = np.zeros((2, 128, 128), np.float32)
    P = gc.panel("random", 100, 128, RP=128)

    def refused(route, RP, **kw):
        with pytest.raises(na.EngineError) as e:
            na.op_gram_wide(route, RP, **kw)
        assert e.value.status == INVALID_ARGUMENT

    refused(2, 128, parts=2, partial=S, with_qx3=False)                            # qx3 == nullptr
    refused(2, 128, parts=0, partial=S)                                            # parts < 1
    refused(2, 64, parts=2, partial=np.zeros((2, 64, 64), np.float32))             # padded rank 64
    refused(1, 128, P=P, parts=4, with_qx3=False)
    refused(0, 64, P=gc.panel("random", 100, 64), parts=4)
    refused(3, 128, P=P, parts=4, product=product(64))                             # wide passengers on the rank-64 product forms (NBW = 2)
