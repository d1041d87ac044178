"""The rank-64 fused multiplicative update (nmfgpu_amd/csrc/kernels_mu64.hip), one launch at a time through na.op_mu64_update, against the restatement
tests/panel_update_reference.mu64_update (docs/PANEL_UPDATE.md; tests/test_panel_update_cpu.py checks restatement, cases and bounds without a device).

k_mu64_update<IS_W> (tile 64): both sides, with its partial Gram matrices.  k_mu64_update32<IS_W, U, QS, NS> (tile 32): the launcher picks U = 13 for more than eight
slabs and 7 otherwise, QS from qsplit, NS from ns.  Its 18 instantiations and the case of this module that launches each:

  IS_W  U   QS  NS     launched by
  1     7   1   -      test_both_tiles_both_sides[32-w]          S = 1, 8
  1     13  1   -      test_both_tiles_both_sides[32-w]          S = 9, 14, 15, 16, 28
  0     7   1   -      test_both_tiles_both_sides[32-h]          S = 1, 8
  0     13  1   -      test_both_tiles_both_sides[32-h]          S = 9, 14, 15, 16, 28
  0     7   2   -      test_k_split_operand[2]                   S = 2
  0     7   4   -      test_k_split_operand[4]                   S = 2
  0     7   8   -      test_k_split_operand[8]                   S = 2
  0     13  2   -      test_k_split_operand[2]                   S = 9
  0     13  4   -      test_k_split_operand[4]                   S = 9
  0     13  8   -      test_k_split_operand[8]                   S = 9
  0     7   1   NS     test_smoothing_around_the_product[0]      S = 2
  0     7   2   NS     test_smoothing_around_the_product[2]      S = 2
  0     7   4   NS     test_smoothing_around_the_product[4]      S = 2
  0     7   8   NS     test_smoothing_around_the_product[8]      S = 2
  0     13  1   NS     test_smoothing_around_the_product[0]      S = 9
  0     13  2   NS     test_smoothing_around_the_product[2]      S = 9
  0     13  4   NS     test_smoothing_around_the_product[4]      S = 9
  0     13  8   NS     test_smoothing_around_the_product[8]      S = 9

Orientation of Q: k_mu64_update reads the r x r operand by columns like every launch_panel_update form, den(c) = sum_k Q[k, c] old(k); k_mu64_update32 reads it by
rows, den(c) = sum_k Q[c, k] old(k) (its comment: "Q is symmetric: a row is a column").  The engine only ever passes Gram matrices, so the two agree there; the
cases of this module are symmetric with entries that change with every step along a row, and test_tile32_reads_its_operand_by_rows pins the difference down.

Expectations as in tests/test_gpu_panel_update.py: exact (the denominator is exact, the result within the two roundings of den + eps and the division; q_out and the
W side's trace terms to the bit), arithmetic (bounds for any order of summation), written (NaN sentinels; padding rows and rank rows past r exact zeros)."""
import numpy as np
import pytest

import nmfgpu_amd as na
from tests import panel_update_cases as cases
from tests import panel_update_reference as ref

pytestmark = pytest.mark.gpu

F32 = np.float32
U = ref.unit_roundoff(F32)
EPS = ref.eps_of(F32)
WORST = {}
# (len_pad, len_valid) dealt to the slab counts in turn: one and three workgroups of the 64-column kernel (two and six... twelve of the 32-column one)
LENGTHS = [(128, 128), (128, 1), (384, 383), (384, 200), (128, 77), (384, 33)]
# 1, 8 | 9, 14, 15: both U; 16 and 28: past the second batch of the 64-column kernel (1 + 7 + 7) and of U = 13 (1 + 13 + 13)
SLABS = [1, 8, 9, 14, 15, 16, 28]


@pytest.fixture(scope="module", autouse=True)
def _library_is_native():
    assert na.device_count() >= 1, "GPU tests need a HIP device"
    yield
    for (form, output), ratio in sorted(WORST.items()):
        print(f"\nworst error / bound  {form:<16} {output:<12} float32: {ratio:.3f}", end="")
    print()


def within(form, output, got, want, bound, what):
    ratio = cases.worst_ratio(got, want, bound)
    WORST[(form, output)] = max(WORST.get((form, output), 0.0), ratio)
    assert ratio <= 1, f"{form} {output} {what}: worst error / bound {ratio:.3g}"


slices_of = cases.slices_of


def run(kind, is_w, tile, r, len_pad, lv, S, *, compute_error=True, qsplit=0, ns=None, form=None, symmetric=True, transpose_for_ref=False):
    case = cases.make_case(kind, "mu", 64, r, len_pad, lv, S, F32, symmetric=symmetric)
    scale = cases.scale_vector(kind, r, F32)
    Q = slices_of(case["Q"], qsplit, kind)
    Gprev = cases.gprev_of(kind, r)
    ps = np.full(len_pad, np.nan, F32)
    got = na.op_mu64_update(is_w, case["P"], case["slabs"], Q, scale, lv, tile=tile, Gprev=Gprev if is_w else None, compute_error=compute_error, qsplit=qsplit, ns=ns,
                            colsq_part=bool(is_w) and tile == 32, ps=ps)
    want = ref.mu64_update(is_w, case["P"], case["slabs"], Q.T if transpose_for_ref else Q, scale, lv, EPS, U, Gprev=Gprev if is_w else None, qsplit=qsplit, ns=ns)
    form = form or f"update{tile}_{'w' if is_w else 'h'}"
    what = f"{kind} tile={tile} is_w={is_w} r={r} len_pad={len_pad} len_valid={lv} S={S} qsplit={qsplit} ns={ns}"
    P = got["P"]
    assert np.all(np.isfinite(P)), f"{what}: NaN reached the panel"
    assert np.all(P[lv:] == 0) and np.all(P[:, r:] == 0), f"{what}: padding rows / rank rows past r are not exact zeros"
    exact = kind == "exact" and ns is None
    b_new = ref.gamma(2, U) * want["new"] if exact else want["b_new"]
    b_num = 0 * want["num"] if exact else want["b_num"]
    bounds = ref.side_bounds(want["new"], b_new, want["num"], b_num, lv, 32, U)

    def hold(name, g, w, b):
        """Exact cases: inside gamma(2) (not recorded among the worst ratios of the arithmetic cases); otherwise `within`."""
        if not exact:
            return within(form, name, g, w, b, what)
        ratio = cases.worst_ratio(g, w, b)
        assert ratio <= 1, f"{form} {name} {what}: worst error / bound {ratio:.3g} (exact case)"

    hold("P", P, want["new"], b_new)
    # error terms
    if not compute_error:
        assert np.all(np.isnan(got["ps"])), f"{what}: ps touched without compute_error"
    elif is_w:
        assert np.all(np.isfinite(got["ps"][:64])) and np.all(np.isnan(got["ps"][64:])), what
        if kind == "exact":
            assert cases.same_bits(got["ps"][:64], want["ps"], F32), what
        else:
            within(form, "ps", got["ps"][:64], want["ps"], want["bounds"]["ps"], what)
    else:
        assert np.all(np.isfinite(got["ps"][:lv])) and np.all(np.isnan(got["ps"][lv:])), what
        hold("ps", got["ps"][:lv], want["ps"], bounds["ps"])
    if tile == 64:
        assert np.all(np.isfinite(got["gram_partial"])), what
        hold("gram_partial", got["gram_partial"], want["gram_partial"], bounds["gram_partial"])
    if got["colsq_part"] is not None:
        assert np.all(np.isfinite(got["colsq_part"])) and np.all(got["colsq_part"][:, r:] == 0), what
        hold("colsq_part", got["colsq_part"], want["colsq_part"], bounds["colsq_part"])
    if qsplit > 1:
        if kind == "exact":
            assert cases.same_bits(got["q_out"], want["q_out"], F32), f"{what}: q_out is not the ordered sum scaled on both sides"
        else:
            within(form, "q_out", got["q_out"], want["q_out"], want["b_q_out"], what)
    # the split image: the new rows bit for bit (rows from len_valid on zero); with smoothing that of S new
    image = got["x3"]
    assert np.all(np.isfinite(image)) and np.all(image[lv:] == 0) and np.all(image[:, r:] == 0), what
    if ns is None:
        masked = P.copy(); masked[lv:] = 0
        assert np.array_equal(image, masked), f"{what}: the split image does not add up to the new panel"
    else:
        within(form, "image", image, want["image"], want["b_image"], what)
    return got


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("side", ["h", "w"])
@pytest.mark.parametrize("tile", [32, 64])
def test_both_tiles_both_sides(tile, side, kind):
    is_w = side == "w"
    for i, S in enumerate(SLABS):
        len_pad, lv = LENGTHS[i % len(LENGTHS)]
        for r in (33, 64):
            on = run(kind, is_w, tile, r, len_pad, lv, S)
            off = run(kind, is_w, tile, r, len_pad, lv, S, compute_error=False)
            assert np.array_equal(on["P"], off["P"]) and np.array_equal(on["x3"], off["x3"])


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("side", ["h", "w"])
def test_tile32_against_tile64(side, kind):
    """Form against form on identical input: within the sum of the bounds."""
    is_w = side == "w"
    for (len_pad, lv), S in zip(LENGTHS, SLABS):
        a = run(kind, is_w, 32, 33, len_pad, lv, S)
        b = run(kind, is_w, 64, 33, len_pad, lv, S)
        case = cases.make_case(kind, "mu", 64, 33, len_pad, lv, S, F32, symmetric=True)
        want = ref.mu64_update(is_w, case["P"], case["slabs"], case["Q"], cases.scale_vector(kind, 33, F32), lv, EPS, U)
        assert cases.worst_ratio(a["P"], b["P"], 2 * (ref.gamma(2, U) * want["new"] if kind == "exact" else want["b_new"])) <= 1
        if is_w and kind == "exact":
            assert np.array_equal(a["ps"], b["ps"], equal_nan=True)       # (the trace terms: integers)


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("qsplit", [2, 4, 8])
def test_k_split_operand(qsplit, kind):
    for S, (len_pad, lv) in ((2, (128, 77)), (9, (384, 383))):
        for r in (33, 64):
            run(kind, False, 32, r, len_pad, lv, S, qsplit=qsplit, form="update32_h_qs")


@pytest.mark.parametrize("qsplit", [0, 2, 4, 8])
def test_smoothing_around_the_product(qsplit):
    for S, (len_pad, lv) in ((2, (128, 77)), (9, (384, 383))):
        for r in (1, 33, 64):
            for kind in ("exact", "random"):
                # theta = 0: S = I, a = 1 and b = 0 -- the bits of the launch without smoothing
                plain = run(kind, False, 32, r, len_pad, lv, S, qsplit=qsplit, form="update32_h_qs" if qsplit else None)
                zero = run(kind, False, 32, r, len_pad, lv, S, qsplit=qsplit, ns=(0.0, 1.0, r), form="update32_h_ns")
                assert np.array_equal(plain["P"], zero["P"]) and np.array_equal(plain["x3"], zero["x3"]) and np.array_equal(plain["ps"], zero["ps"], equal_nan=True)
                run(kind, False, 32, r, len_pad, lv, S, qsplit=qsplit, ns=(0.5 / r, 0.5 + 0.5 / r, r), form="update32_h_ns")


def test_tile32_reads_its_operand_by_rows():
    """The finding of docs/PANEL_UPDATE.md, "Orientation of Q": with a Q that is not symmetric the 64-column kernel matches the restatement as it stands, the
    32-column kernel matches it with Q transposed -- and not the other way round."""
    for kind in ("exact", "random"):
        run(kind, False, 64, 33, 128, 77, 2, symmetric=False)
        run(kind, False, 32, 33, 128, 77, 2, symmetric=False, transpose_for_ref=True)
        case = cases.make_case(kind, "mu", 64, 33, 128, 77, 2, F32)
        scale = cases.scale_vector(kind, 33, F32)
        got = na.op_mu64_update(False, case["P"], case["slabs"], case["Q"], scale, 77, tile=32)
        want = ref.mu64_update(False, case["P"], case["slabs"], case["Q"], scale, 77, EPS, U)
        assert cases.worst_ratio(got["P"], want["new"], want["b_new"]) > 1


@pytest.mark.parametrize("kind", ["exact", "random"])
def test_eps_on_a_vanishing_denominator(kind):
    """cases.tiny_row on both tiles and both sides: row 0 is old * num / eps (see tests/test_gpu_panel_update.py, test_eps_decides_where_the_denominator_vanishes)."""
    for tile in (32, 64):
        for is_w in (False, True):
            case = cases.tiny_row(cases.make_case(kind, "mu", 64, 33, 128, 77, 8, F32, symmetric=True))
            scale = cases.scale_vector(kind, 33, F32)
            got = na.op_mu64_update(is_w, case["P"], case["slabs"], case["Q"], scale, 77, tile=tile)
            want = ref.mu64_update(is_w, case["P"], case["slabs"], case["Q"], scale, 77, EPS, U)
            bound = ref.gamma(2, U) * want["new"] if kind == "exact" else want["b_new"]
            assert np.all(np.isfinite(got["P"])) and np.any(got["P"][0] > 0)
            assert cases.worst_ratio(got["P"], want["new"], bound) <= 1, (tile, is_w, cases.worst_ratio(got["P"], want["new"], bound))
            if kind == "exact":
                assert cases.same_bits(got["P"][0], want["new"][0], F32), (tile, is_w)


def test_w_update_of_the_default_fused_iteration_is_this_launch():
    """Operations against the engine: the default iteration at padded rank 64 (four launches, kernels_mu64.hip) keeps W unnormalised with a pending column scale.
    Two iterations on a 600 x 500 problem at rank 50; around the second one the test reads what its W update was launched with -- the W panel as it lay (debug
    read 21), the pending scale the product's passengers left (20), the W step's slabs (4), H H^T (3), the Gram matrix of the error terms (2) -- and launches
    launch_mu64_update32 through op_mu64_update with the engine's argument order: the engine's unnormalised W, bit for bit, so the entry's scale side, slab
    order and operands cannot drift from the engine's.  The factors the engine hands out are that panel times 1 / sqrt of the summed colsq_part: restated in
    float32 and held to gamma(parts + 3) (the sum of the partials in any order, square root, reciprocal, product).
    (The H update of the same iteration: test_h_update_of_the_default_fused_iteration_is_this_launch.)"""
    m, n, r = 600, 500, 50
    rng = np.random.default_rng(17)
    V = np.asfortranarray(rng.random((m, n)).astype(F32))
    W0 = np.asfortranarray((0.1 + rng.random((m, r))).astype(F32))
    H0 = np.asfortranarray((0.1 + rng.random((r, n))).astype(F32))
    eng = na.Engine(m, n, r, "mu", dtype=F32)
    try:
        eng.upload(V)
        eng.set_factors(W0, H0)
        geo = eng.geometry()
        assert geo["padded_rank"] == 64 and geo["fused_launches"] == 4 and geo["product_kernel"] == 2, geo
        mpad, npad, S = geo["padded_m"], geo["padded_n"], geo["slabs_w"]
        stride = 64 * max(mpad, npad)
        eng.iterate(1, first_iteration=1, error_every=1000)
        Wt1 = eng.debug_read(21, 64 * mpad).reshape(mpad, 64)
        eng.iterate(1, first_iteration=2, error_every=1000)
        scale = eng.debug_read(20, 64)
        slabs = eng.debug_read(4, stride * S).reshape(S, stride)
        HHt = eng.debug_read(3, 4096).reshape(64, 64)
        G = eng.debug_read(2, 4096).reshape(64, 64)
        Wt2 = eng.debug_read(21, 64 * mpad).reshape(mpad, 64)
        W2, _ = eng.get_factors()
    finally:
        eng.close()
    assert not np.array_equal(scale, np.ones(64, F32)), "the second iteration's pending scale is trivial: the tie would not see which side it goes on"
    got = na.op_mu64_update(True, Wt1, slabs, HHt, scale, m, tile=32, Gprev=G, colsq_part=True)
    assert np.array_equal(got["P"], Wt2), "the engine's unnormalised W differs from the same launch through op_mu64_update"
    parts = mpad // 32
    sumsq = got["colsq_part"].sum(axis=0, dtype=F32)
    d = np.ones(64, F32)       # (columns from r on: no sum of squares, scale 1)
    d[sumsq > 0] = F32(1) / np.sqrt(sumsq[sumsq > 0])
    want = (got["P"] * d[None, :])[:m, :r]
    ratio = cases.worst_ratio(W2, want, ref.gamma(parts + 3, U) * np.abs(want))
    assert ratio <= 1, f"W of the engine is {ratio:.3g} of gamma(parts + 3) from the chain of operations"


@pytest.mark.parametrize("m,n,slices", [(600, 500, 16), (4000, 100, 4)])
def test_h_update_of_the_default_fused_iteration_is_this_launch(m, n, slices):
    """Operations against the engine, H side.  The fused iteration (Engine::iterate_mu64) opens with product_h(Wt, passengers) and
    mu64_update(false, slabs, planH.splits, stride, ksplit > 1 ? Gpart : G, ...); Engine::h_step_impl -- the three-phase entry -- issues the same two calls, and
    stops there, with the H update's slabs still in place (inside iterate_mu64 the W product overwrites them).  So: one default iteration (W is now unnormalised
    with a pending scale), then
      engine A: a second default iteration;
      engine B: h_step, and reads of what its H update was launched with -- the H panel before (debug read 1), the slabs (4), the pending scale (20), the r x r
                operand: the finished W^T W (2) or, where the plan cuts the Gram passengers' K range, its unscaled K slices (22) with q_out left in (2).
    B's H equals A's bit for bit (h_step is the iteration's first half), and op_mu64_update with the engine's argument order -- the scale on the numerator, the
    32-column kernel, qsplit = gram_k_slices -- returns that H bit for bit, and q_out the engine's finished matrix bit for bit.
    600 x 500: gram_k_slices reports 16, the spread form: sixteen passengers share the K range and the last of them hands over one finished matrix, no qsplit.
    4000 x 100: tall and narrow, the plan takes four K slices: the qsplit form."""
    r = 50
    rng = np.random.default_rng(19)
    V = np.asfortranarray(rng.random((m, n)).astype(F32))
    W0 = np.asfortranarray((0.1 + rng.random((m, r))).astype(F32))
    H0 = np.asfortranarray((0.1 + rng.random((r, n))).astype(F32))

    def start():
        eng = na.Engine(m, n, r, "mu", dtype=F32)
        eng.upload(V)
        eng.set_factors(W0, H0)
        eng.iterate(1, first_iteration=1, error_every=1000)
        return eng

    a = start()
    try:
        a.iterate(1, first_iteration=2, error_every=1000)
        _, Ha = a.get_factors()
    finally:
        a.close()
    b = start()
    try:
        geo = b.geometry()
        assert geo["padded_rank"] == 64 and geo["fused_launches"] == 4 and geo["product_kernel"] == 2 and geo["gram_k_slices"] == slices, geo
        mpad, npad, S = geo["padded_m"], geo["padded_n"], geo["slabs_h"]
        stride = 64 * max(mpad, npad)
        H1 = b.debug_read(1, 64 * npad).reshape(npad, 64)
        b.h_step(False)
        scale = b.debug_read(20, 64)
        slabs = b.debug_read(4, stride * S).reshape(S, stride)
        G = b.debug_read(2, 4096).reshape(64, 64)
        qsplit = slices if slices in (2, 4, 8) else 0
        Q = b.debug_read(22, 4096 * qsplit).reshape(qsplit, 64, 64) if qsplit else G
        H2 = b.debug_read(1, 64 * npad).reshape(npad, 64)
    finally:
        b.close()
    assert np.array_equal(H2[:n, :r].T, Ha), "h_step's H update is not the fused iteration's"
    assert not np.array_equal(scale, np.ones(64, F32)), "the pending scale is trivial: the tie would not see which side it goes on"
    got = na.op_mu64_update(False, H1, slabs, Q, scale, n, tile=32, qsplit=qsplit)
    assert np.array_equal(got["P"], H2), "the engine's H differs from the same launch through op_mu64_update"
    if qsplit:
        assert np.array_equal(got["q_out"], G), "q_out differs from the matrix the engine's H update left"


def test_refusals_leave_every_output_alone():
    case = cases.make_case("random", "mu", 64, 33, 128, 100, 2, F32, symmetric=True)
    scale = cases.scale_vector("random", 33, F32)
    Q8 = slices_of(case["Q"], 8, "random")

    def refused(is_w, Q, **kw):
        ps = np.full(128, np.nan, F32)
        P0 = case["P"].copy()
        with pytest.raises(na.EngineError) as e:
            na.op_mu64_update(is_w, case["P"], case["slabs"], Q, scale, 100, ps=ps, **kw)
        assert e.value.status == 1, kw
        assert np.all(np.isnan(ps)) and np.array_equal(case["P"], P0)

    refused(True, Q8[:2], tile=32, qsplit=2)                        # the K-split operand belongs to the H side
    refused(False, Q8[:3], tile=32, qsplit=3)                       # 2, 4 or 8 slices
    refused(True, case["Q"], tile=32, ns=(0.1, 0.9, 33))            # so does the smoothing
    refused(False, case["Q"], tile=32, ns=(0.1, 0.9, 0))            # its rank: 1 ... 64
    refused(False, case["Q"], tile=32, ns=(0.1, 0.9, 65))
    refused(False, Q8[:2], tile=64, qsplit=2)                       # the 64-column launcher has neither
    refused(False, case["Q"], tile=64, ns=(0.1, 0.9, 33))
    refused(True, case["Q"], tile=32, compute_error=True)           # the W side's trace terms need Gprev
