"""The rank-64 Gram matrix from partial 64 x 64 matrices (kernels_mu64.hip and the passenger reduction of kernels_x3.hip), one launch at a time through
na.op_gram64_partials, against the restatement of tests/gram_reference.py (docs/GRAM.md; tests/test_gram_cpu.py checks it without a device).

Routes:  0  launch_mu64_gram_partials            one matrix per 64 panel rows, fp32 products on the matrix pipe
         1  launch_mu64_gram_reduce              sixteen workgroups, two groups of parts; normalize 0 / 1
         2  gram_reduce_block_x3                 the same reduction as sixteen passenger workgroups of the split-operand product, FOUR groups of parts
         6  ... of the col_split product launch  (128 x 32 workgroups over 128-row tiles, one slab)
         3  launch_gram64_from_partials          launch_reduce_partials, then (with a scale) k_scale_gram64
         4  launch_gram64_normalize_all          Graw, then G = D Graw D, the scaled panel and its split image
         5  launch_gram64_reduce_scale_all       the same in one launch, the scales from sums of squares

Held to: every element within its derived bound, the exact kinds as bits; sums of symmetric matrices exactly symmetric; what is an exact function of other OUTPUTS
as bits -- G = (Graw s[c]) s[r] of route 4, the scaled panel P s[c], its split image -- and refusals.  Routes 1 and 2 return the same bits wherever the grouping of
the parts cannot matter (exact data, and up to two parts); elsewhere they differ, see test_riding_reduction_against_the_standalone_kernel."""
import functools

import numpy as np
import pytest

import nmfgpu_amd as na
from tests import gram_cases as gc
from tests import gram_reference as gr

pytestmark = pytest.mark.gpu

WORST = {}
INVALID_ARGUMENT = 1
ROUTE_NAME = {0: "partials", 1: "reduce", 2: "reduce_ride", 6: "reduce_ride_cs", 3: "from_partials", 4: "normalize_all", 5: "reduce_scale_all"}


@pytest.fixture(scope="module", autouse=True)
def _report():
    assert na.device_count() >= 1, "GPU tests need a HIP device"
    yield
    for (route, output), ratio in sorted(WORST.items()):
        print(f"\nworst error / bound  rank64 {route:<17} {output:<8}: {ratio:.3g}", end="")
    print()


@functools.lru_cache(maxsize=None)
def product():
    rng = np.random.default_rng(6)
    return (np.asfortranarray(rng.uniform(0, 1, (200, 300)).astype(np.float32)), np.asfortranarray(rng.uniform(0, 1, (64, 300)).astype(np.float32)))


def symmetric(a):
    return np.array_equal(gr.bits(a), gr.bits(np.ascontiguousarray(a.T)))


@pytest.mark.parametrize("kind", ["random", "ints"])
@pytest.mark.parametrize("len_pad", [64, 128, 320])
def test_partials_f32(len_pad, kind):
    P = gc.panel(kind, len_pad, 61, zero_col=3)
    got = na.op_gram64_partials(0, P=P)["partials"]
    assert got.shape == (len_pad // 64, 64, 64)
    gr.held("partials", got, gr.gram_partials(P), np.array(kind != "random"), WORST, ("partials", "partial"))
    for p in got:
        assert symmetric(p), "a partial matrix is not symmetric"


def check_reduction(route, got, M, normalize, kind, with_scale=True):
    ref = gr.gram_reduce(M, normalize)
    name = ROUTE_NAME[route]
    exact = np.array(kind != "random")
    gr.held(f"{name} G", got["G"], ref["G"], exact, WORST, (name, "G n%d" % normalize))
    if with_scale:
        gr.held(f"{name} scale", got["scale"], ref["scale"], exact, WORST, (name, "scale"))
    else:
        assert got["scale"] is None
    if not normalize:
        assert symmetric(got["G"]), f"{name}: the sum of symmetric matrices is not symmetric"


@pytest.mark.parametrize("kind", ["random", "pow2"])
@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("parts", gc.REDUCE_PARTS)
@pytest.mark.parametrize("route", [1, 2, 6], ids=["standalone", "riding", "riding_colsplit"])
def test_reduce_f32(route, parts, normalize, kind):
    M = gc.partial_matrices(kind, parts, r=61 if kind == "random" else 64)
    got = na.op_gram64_partials(route, partials=M, normalize=normalize, product=product() if route != 1 else None)
    check_reduction(route, got, M, normalize, kind)
    if route != 1:
        assert np.isfinite(got["out_ride"]).all()
        assert np.array_equal(gr.bits(got["out_ride"]), gr.bits(got["out_plain"])), "the product's bits change with passengers aboard"


@pytest.mark.parametrize("normalize", [0, 1])
@pytest.mark.parametrize("parts", gc.REDUCE_PARTS)
def test_riding_reduction_against_the_standalone_kernel(parts, normalize):
    """The comment above k_mu64_gram_reduce claims the passengers' arithmetic and order.  That holds for the passengers of the fp32 product (kernels.hip, 512
    threads, two groups of parts); the passengers of the split-operand product have 256 threads and add FOUR groups, (((g0 + g1) + g2) + g3) against (h0 + h1).
    So: the same bits on exact data at every part count, and on random data where both groupings are the same sum (one or two parts); from three parts on the two
    kernels may differ in the last bit, each inside its own bound (test_reduce_f32)."""
    for kind in ("pow2", "random"):
        M = gc.partial_matrices(kind, parts)
        alone = na.op_gram64_partials(1, partials=M, normalize=normalize)
        rode = na.op_gram64_partials(2, partials=M, normalize=normalize, product=product())
        cs = na.op_gram64_partials(6, partials=M, normalize=normalize, product=product())
        for name in ("G", "scale"):          # the same passengers on either product launch
            assert np.array_equal(gr.bits(cs[name]), gr.bits(rode[name])), f"{kind} parts {parts}: {name} differs between the two product launches it rides in"
        if kind == "pow2" or parts <= 2:
            for name in ("G", "scale"):
                assert np.array_equal(gr.bits(rode[name]), gr.bits(alone[name])), f"{kind} parts {parts}: {name} differs between the riding and the stand-alone reduction"
        else:
            ref = gr.gram_reduce(M, normalize)
            assert (np.abs(rode["G"].astype(np.float64) - alone["G"]) <= 2 * ref["G"][1]).all()


@pytest.mark.parametrize("kind", ["random", "pow2"])
@pytest.mark.parametrize("with_scale", [False, True], ids=["sum", "scaled"])
@pytest.mark.parametrize("parts", gc.REDUCE_PARTS)
def test_from_partials_f32(parts, with_scale, kind):
    M = gc.partial_matrices(kind, parts)
    got = na.op_gram64_partials(3, partials=M, with_scale=with_scale)
    check_reduction(3, got, M, int(with_scale), kind, with_scale)


def check_panel_outputs(name, got, P_in, x3_ks):
    """The scaled panel and its split image are exact functions of the scales the launch published."""
    want = gr.scaled_panel(P_in, got["scale"])
    assert np.array_equal(gr.bits(got["P"]), gr.bits(want)), f"{name}: the scaled panel is not P(y, c) * scale(c)"
    len_pad = P_in.shape[0]
    img = gr.pack_panel_x3(got["P"], x3_ks)
    assert np.array_equal(got["x3"][:img.size], img), f"{name}: the split image is not that of the scaled panel"
    assert (got["x3"][img.size:] == 0x7FC0).all(), f"{name}: the image was written beyond x3_ks = {x3_ks} of {len_pad // 16} K-steps"


@pytest.mark.parametrize("kind", ["random", "pow2"])
@pytest.mark.parametrize("parts,len_pad,x3_ks", [(1, 64, 4), (3, 128, 8), (9, 128, 5), (17, 320, 20)])
def test_normalize_all_f32(parts, len_pad, x3_ks, kind):
    M = gc.partial_matrices(kind, parts, r=61)
    P = gc.panel("pow2" if kind == "pow2" else "random", len_pad, 61)
    got = na.op_gram64_partials(4, P=P, partials=M, x3_ks=x3_ks)
    exact = np.array(kind != "random")
    gr.held("normalize_all Graw", got["Graw"], gr.partial_sum(M), exact, WORST, ("normalize_all", "Graw"))
    assert symmetric(got["Graw"])
    ref = gr.gram_reduce(M, 1)
    gr.held("normalize_all G", got["G"], ref["G"], exact, WORST, ("normalize_all", "G"))
    gr.held("normalize_all scale", got["scale"], ref["scale"], exact, WORST, ("normalize_all", "scale"))
    # the scales from the diagonal the DEVICE holds: two correctly rounded operations; G an exact function of Graw and the scales
    gr.held("normalize_all scale of Graw", got["scale"], gr.scale_from_value(np.diag(got["Graw"])), None, WORST, ("normalize_all", "rsqrt"))
    assert np.array_equal(gr.bits(got["G"]), gr.bits(gr.scaled_matrix_fp32(got["Graw"], got["scale"]))), "G is not (Graw s[c]) s[r]"
    check_panel_outputs("normalize_all", got, P, x3_ks)


@pytest.mark.parametrize("kind", ["random", "pow2"])
@pytest.mark.parametrize("parts,sq_parts,len_pad,x3_ks", [(1, 1, 64, 4), (2, 3, 64, 3), (3, 4, 128, 8), (9, 5, 128, 8), (16, 158, 320, 20), (17, 193, 128, 8), (8, 400, 64, 4)])
def test_reduce_scale_all_f32(parts, sq_parts, len_pad, x3_ks, kind):
    M = gc.partial_matrices("ints" if kind == "pow2" else "random", parts, r=61)
    sq = gc.colsq(kind, sq_parts, 61, zero_col=11)
    P = gc.panel("pow2" if kind == "pow2" else "random", len_pad, 61)
    got = na.op_gram64_partials(5, P=P, partials=M, sumsq_part=sq, x3_ks=x3_ks)
    ref = gr.gram_reduce_scale_all(M, sq)
    exact = np.array(kind != "random")
    gr.held("reduce_scale_all G", got["G"], ref["G"], exact, WORST, ("reduce_scale_all", "G"))
    gr.held("reduce_scale_all scale", got["scale"], ref["scale"], exact, WORST, ("reduce_scale_all", "scale"))
    assert got["scale"][11] == 1.0          # the guarded branch: a zero column
    check_panel_outputs("reduce_scale_all", got, P, x3_ks)


def test_refusals_run_no_kernel():
    """Route 5 is refused by launch_gram64_reduce_scale_all.  launch_mu64_gram_reduce and launch_gram64_from_partials have no refusal of their own: with no
    parts it is the test entry that declines, so the last two lines only pin the entry's contract."""
    M = gc.partial_matrices("random", 3)
    P = gc.panel("random", 64, 64)
    sq = gc.colsq("random", 3, 64)
    for kw in (dict(route=5, P=P, partials=M[:0], sumsq_part=sq), dict(route=5, P=P, partials=M, sumsq_part=sq[:0]), dict(route=1, partials=M[:0]),
               dict(route=3, partials=M[:0])):
        with pytest.raises(na.EngineError) as e:
            na.op_gram64_partials(kw.pop("route"), **kw)
        assert e.value.status == INVALID_ARGUMENT
