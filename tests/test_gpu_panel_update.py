"""Every dispatch target of launch_panel_update<T> (nmfgpu_amd/csrc/kernels.hip) and the fused launches behind it, one launch at a time through
na.op_panel_update, against the restatement of tests/panel_update_reference.py (docs/PANEL_UPDATE.md has the map of kernels and the derivation of the bounds;
tests/test_panel_update_cpu.py checks restatement, cases and bounds without a device).

Kernel forms reached, by the name the tests and the table of worst ratios use:
  generic         k_panel_update<T, MU / LS / SET>: under NMFAMD_FORCE_VALU (float32 RP 64 keeps its LDS form there), at float32 RP 192 (no fast form), and
                  MODE_SET everywhere
  lds64           k_panel_update64_lds_f32 (float32 RP 64; gram_partial and the split image)
  old64           k_panel_update64_f32 (measurement build, NMFAMD_UPDATE64_OLD)
  wide_f32        k_panel_update_wide_f32<MODE, NCB> at RP 128 / 256 / 384 / 512 with the fp32 Q
  wide_f32_splitq ... with the split bf16 image of Q
  wide_f32_fused  k_panel_update_wide_f32<MU, NCB, FX>: W side (old_scale) and H side (scale, smoothing), Q as its split image only
  long            k_panel_update_rows_mu (RP 128; RP 256 without ps) and k_panel_update_wide64_mu (RP 256 with ps) at len_pad = 33 024
  f64_64          k_panel_update64_f64<MODE, HS> plain and fused
  wide_f64        k_panel_update_wide_f64 at RP 128 ... 512 in steps of 64, plain and fused

Three kinds of expectation:
  exact       integer inputs (tests/panel_update_cases.py): MODE_LS, MODE_SET, num_out, ps, sumsq_part and gram_partial return the restatement's bits; in MODE_MU the
              denominator is exact and the result is within the two roundings every form performs on it (den + eps, the division): gamma(2) relative;
  arithmetic  random non-negative data at the engines' eps, every element within a bound that holds for any order of summation;
  written     every output starts as NaN, the slab gaps and the sumsq_part rows past `parts` are NaN: what a launch must write is finite, ps[len_valid:] and the
              spare rows are still NaN, padding rows and rank rows past r are exact zeros, and the split image equals the new panel bit for bit."""
import numpy as np
import pytest

import nmfgpu_amd as na
from tests import panel_update_cases as cases
from tests import panel_update_reference as ref

pytestmark = pytest.mark.gpu

WORST = {}      # (kernel form, output, dtype) -> worst observed error / bound over the arithmetic cases, printed when the module is done
SHAPES, RANKS = cases.SHAPES, cases.RANKS       # (shared with the device-free mutation check)


@pytest.fixture(scope="module", autouse=True)
def _library_is_native():
    assert na.device_count() >= 1, "GPU tests need a HIP device"
    yield
    for (form, output, dtype), ratio in sorted(WORST.items()):
        print(f"\nworst error / bound  {form:<16} {output:<12} {dtype}: {ratio:.3f}", end="")
    print()


def within(form, output, dtype, got, want, bound, what):
    ratio = cases.worst_ratio(got, want, bound)
    key = (form, output, np.dtype(dtype).name)
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    assert ratio <= 1, f"{form} {output} {what}: worst error / bound {ratio:.3g}"


def form_of(dtype, RP, mode, split_q=False, forced=False):
    f32 = np.dtype(dtype) == np.float32
    if forced or mode == "set" or RP == 192 and f32:
        return "generic"
    if f32:
        return "lds64" if RP == 64 else ("wide_f32_splitq" if split_q else "wide_f32")
    return "f64_64" if RP == 64 else "wide_f64"


def launch(case, mode, **kw):
    """op_panel_update with every optional output as NaN sentinels: ps, more sumsq_part rows than any form writes, num_out."""
    dt = case["P"].dtype
    ps = np.full(case["len_pad"], np.nan, dt)
    sumsq = np.full((case["len_pad"] // 4 + 2, case["RP"]), np.nan, dt)
    return na.op_panel_update(mode, case["P"], case["slabs"], case["Q"], case["len_valid"], ps=ps, sumsq_part=sumsq, **kw)


def check(form, case, mode, got, what, *, split_q=False, want=None, image_key="x3", masked_image=True):
    """One launch against its restatement: what was and was not written, then bits or bounds."""
    dt = case["P"].dtype
    RP, r, len_pad, lv = case["RP"], case["r"], case["len_pad"], case["len_valid"]
    u = ref.unit_roundoff(dt)
    parts = got["parts"]
    assert parts > 0 and len_pad % parts == 0, what
    if want is None:
        want = ref.panel_update(mode, case["P"], case["slabs"], case["Q"], lv, ref.eps_of(dt), len_pad // parts, u, split_q=split_q)
    P, ps, sq = got["P"], got["ps"], got["sumsq_part"]
    # written
    assert np.all(np.isfinite(P)), f"{what}: NaN reached the panel"
    assert np.all(P[lv:] == 0) and np.all(P[:, r:] == 0), f"{what}: padding rows / rank rows past r are not exact zeros"
    assert np.all(np.isfinite(ps[:lv])) and np.all(np.isnan(ps[lv:])), f"{what}: ps must be written below len_valid and nowhere else"
    assert np.all(np.isfinite(sq[:parts])) and np.all(np.isnan(sq[parts:])), f"{what}: sumsq_part must be written in its {parts} rows and nowhere else"
    outputs = [("P", P, want["new"], None), ("ps", ps[:lv], want["ps"], want["bounds"]["ps"]), ("sumsq_part", sq[:parts], want["sumsq_part"], want["bounds"]["sumsq_part"])]
    if got.get("num_out") is not None:
        assert np.all(np.isfinite(got["num_out"])), what
        outputs.append(("num_out", got["num_out"], want["num"], want["b_num"]))
    if got.get("gram_partial") is not None:
        assert np.all(np.isfinite(got["gram_partial"])), what
        outputs.append(("gram_partial", got["gram_partial"], want["gram_partial"], want["bounds"]["gram_partial"]))
    if got.get(image_key) is not None:
        image = P.astype(np.float32).copy()
        if masked_image:
            image[lv:] = 0
        assert np.array_equal(got[image_key], image), f"{what}: the split image does not add up to the new panel"
    if got.get("smooth_out") is not None:
        assert np.all(np.isfinite(got["smooth_out"])) and np.all(got["smooth_out"][lv:] == 0) and np.all(got["smooth_out"][:, r:] == 0), what
    exact_bits = case["exact"] and mode != "mu"
    if case["exact"] and mode == "mu":
        # the denominator and old * num are exact; den + eps and the division round once each, in every form
        b_new = ref.gamma(2, u) * want["new"]
        bounds = ref.side_bounds(want["new"], b_new, want["num"], 0 * want["num"], lv, len_pad // parts, u)
        assert cases.same_bits(got["num_out"], want["num"], dt) if got.get("num_out") is not None else True, what
    else:
        b_new, bounds = want["b_new"], want["bounds"]
    for name, g, w, b in outputs:
        if exact_bits:
            assert cases.same_bits(g, w, dt), f"{form} {name} {what}: differs at {np.argwhere(np.asarray(g, dtype=np.float64) != np.asarray(w))[:4].tolist()}"
        else:
            bound = b_new if name == "P" else (bounds[name] if name in bounds else b)
            if case["exact"]:
                assert cases.worst_ratio(g, w, bound) <= 1, f"{form} {name} {what}: {cases.worst_ratio(g, w, bound):.3g} of the exact case's bound"
            else:
                within(form, name, dt, g, w, bound, what)
    return want


def run_shapes(dtype, RP, mode, kind, *, split_q=False, forced=False, shapes=SHAPES, **kw):
    form = form_of(dtype, RP, mode, split_q, forced)
    results = []
    for len_pad, lv, S in shapes:
        case = cases.make_case(kind, mode, RP, RANKS[RP], len_pad, lv, S, dtype)
        what = f"{kind} {mode} RP={RP} len_pad={len_pad} len_valid={lv} S={S}"
        got = launch(case, mode, num_out=True, split_q=split_q, **kw)
        assert got["form"] == {"lds64": "lds64", "wide_f32": "wide32", "wide_f32_splitq": "wide32"}.get(form, "other"), (what, got["form"])
        check(form, case, mode, got, what, split_q=split_q)
        if (len_pad, lv, S) in (shapes[0], shapes[-1]):
            # the launch without num_out (what the engines run outside GDCLS error iterations): the same panel and side outputs, bit for bit
            bare = launch(case, mode, split_q=split_q, **kw)
            assert bare["num_out"] is None and bare["form"] == got["form"], what
            for key in ("P", "ps", "sumsq_part", "gram_partial", "x3"):
                assert (bare[key] is None and got[key] is None) or np.array_equal(bare[key], got[key], equal_nan=True), f"{what}: {key} changes with num_out"
        results.append((case, got))
    return results


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("mode", ["mu", "ls"])
def test_lds64_with_gram_partial_and_split_image(mode, kind):
    for case, got in run_shapes(np.float32, 64, mode, kind, gram_partial=True, x3=True):
        assert got["parts"] == case["len_pad"] // 64
        # without the extras: the same panel, nothing else touched
        plain = launch(case, mode)
        assert np.array_equal(plain["P"], got["P"]) and np.array_equal(plain["ps"], got["ps"], equal_nan=True) and plain["x3"] is None and plain["gram_partial"] is None


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("mode", ["mu", "ls"])
@pytest.mark.parametrize("RP", [128, 256, 384, 512])
def test_wide_f32_with_fp32_q_and_with_split_q(RP, mode, kind):
    plain = run_shapes(np.float32, RP, mode, kind)
    split = run_shapes(np.float32, RP, mode, kind, split_q=True)
    u = ref.unit_roundoff(np.float32)
    for (case, a), (_, b) in zip(plain, split):
        assert a["parts"] == b["parts"] == case["len_pad"] // 32
        if case["exact"]:
            # one-plane operands: the six-term product is exact, the two forms agree to the bit
            assert np.array_equal(a["P"], b["P"]) and np.array_equal(a["ps"], b["ps"], equal_nan=True) and np.array_equal(a["sumsq_part"], b["sumsq_part"], equal_nan=True)
        else:
            wa = ref.panel_update(mode, case["P"], case["slabs"], case["Q"], case["len_valid"], ref.eps_of(np.float32), 32, u)
            wb = ref.panel_update(mode, case["P"], case["slabs"], case["Q"], case["len_valid"], ref.eps_of(np.float32), 32, u, split_q=True)
            assert cases.worst_ratio(a["P"], b["P"], wa["b_new"] + wb["b_new"]) <= 1


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("mode", ["mu", "ls"])
@pytest.mark.parametrize("RP", [64, 128, 192, 256, 320, 384, 448, 512])
def test_f64_every_rank(RP, mode, kind):
    for case, got in run_shapes(np.float64, RP, mode, kind):
        assert got["parts"] == case["len_pad"] // (32 if RP == 64 else 16)


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_generic_kernel_set_mode_and_the_rank_no_fast_form_takes(dtype, kind):
    dt = np.dtype(dtype).type
    for RP in (64, 192, 512):
        run_shapes(dt, RP, "set", kind, shapes=SHAPES[2:4])
    if dt == np.float32:
        for mode in ("mu", "ls"):
            run_shapes(dt, 192, mode, kind)


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_generic_kernel_under_force_valu_against_the_fast_forms(dtype, kind, monkeypatch):
    """NMFAMD_FORCE_VALU routes every rank to k_panel_update; form against form on identical input: within the sum of the bounds, bit-equal on the exact cases in
    MODE_LS (in MODE_MU the forms may round den + eps and the quotient alike or not: both are inside gamma(2))."""
    dt = np.dtype(dtype).type
    u = ref.unit_roundoff(dt)
    # (float32 at RP 64 keeps its LDS-staged form under the switch: the launcher does not ask there)
    for RP in ((128, 256) if dt == np.float32 else (64, 128, 256)):
        for mode in ("mu", "ls"):
            fast = run_shapes(dt, RP, mode, kind, shapes=SHAPES[1:4])
            monkeypatch.setenv("NMFAMD_FORCE_VALU", "1")
            slow = run_shapes(dt, RP, mode, kind, forced=True, shapes=SHAPES[1:4])
            monkeypatch.delenv("NMFAMD_FORCE_VALU")
            for (case, a), (_, b) in zip(fast, slow):
                rows = 32       # (panel_update_rows: 32 rows per workgroup, fewer when two [rows][RP] images would not fit 64 KiB)
                while 2 * rows * RP * np.dtype(dt).itemsize > 65536:
                    rows //= 2
                assert b["parts"] == case["len_pad"] // rows
                if case["exact"] and mode == "ls":
                    assert np.array_equal(a["P"], b["P"]) and np.array_equal(a["ps"], b["ps"], equal_nan=True)
                else:
                    w = ref.panel_update(mode, case["P"], case["slabs"], case["Q"], case["len_valid"], ref.eps_of(dt), 32, u)
                    bound = 2 * (ref.gamma(2, u) * w["new"] if case["exact"] else w["b_new"])
                    assert cases.worst_ratio(a["P"], b["P"], bound) <= 1, (RP, mode)


def test_old_rank64_kernel_against_the_lds_form(diag_build, monkeypatch):
    for kind in ("exact", "random"):
        for mode in ("mu", "ls"):
            new = run_shapes(np.float32, 64, mode, kind, shapes=SHAPES[1:4])
            monkeypatch.setenv("NMFAMD_UPDATE64_OLD", "1")
            old = []
            for len_pad, lv, S in SHAPES[1:4]:
                case = cases.make_case(kind, mode, 64, RANKS[64], len_pad, lv, S, np.float32)
                got = launch(case, mode, num_out=True)
                check("old64", case, mode, got, f"{kind} {mode} len_pad={len_pad} len_valid={lv} S={S}")
                assert got["parts"] == len_pad // 128
                old.append(got)
            monkeypatch.delenv("NMFAMD_UPDATE64_OLD")
            u = ref.unit_roundoff(np.float32)
            for (case, a), b in zip(new, old):
                if kind == "exact" and mode == "ls":
                    assert np.array_equal(a["P"], b["P"]) and np.array_equal(a["ps"], b["ps"], equal_nan=True)
                else:
                    w = ref.panel_update(mode, case["P"], case["slabs"], case["Q"], case["len_valid"], ref.eps_of(np.float32), 64, u)
                    assert cases.worst_ratio(a["P"], b["P"], 2 * (ref.gamma(2, u) * w["new"] if kind == "exact" else w["b_new"])) <= 1


@pytest.mark.parametrize("with_ps", [False, True])
@pytest.mark.parametrize("RP", [128, 256])
def test_long_forms_against_the_32_row_kernel(RP, with_ps):
    """len_pad = 33 024 >= 32 768 with the split image of Q: k_panel_update_rows_mu, and at RP 256 with ps k_panel_update_wide64_mu (the rows kernel's
    instantiation with error terms spills at that rank: the launcher keeps it out).  The forms return the same values and the same partials, so the kernel taken
    is read from the launcher itself (`form`, nmfamd_op_panel_update_last_form) and asserted.  Against the restatement, and against the 32-row kernel (the fp32-Q form never
    takes the long path) on the same input within both bounds."""
    len_pad, lv, S = 33024, 33001, 2
    u = ref.unit_roundoff(np.float32)
    for kind in ("exact", "random"):
        case = cases.make_case(kind, "mu", RP, RANKS[RP], len_pad, lv, S, np.float32)
        ps = np.full(len_pad, np.nan, np.float32) if with_ps else None
        sumsq = np.full((len_pad // 32 + 2, RP), np.nan, np.float32)
        long = na.op_panel_update("mu", case["P"], case["slabs"], case["Q"], lv, ps=ps, sumsq_part=sumsq, split_q=True)
        short = na.op_panel_update("mu", case["P"], case["slabs"], case["Q"], lv, ps=ps, sumsq_part=sumsq)
        assert long["parts"] == short["parts"] == len_pad // 32
        # the launcher's choice, as it reports it: the 128-row kernel, but at RP 256 with error terms (that instantiation spills) the 64-row one; the fp32-Q form
        # stays with the 32-row kernel
        assert long["form"] == ("wide64" if RP == 256 and with_ps else "rows128"), long["form"]
        assert short["form"] == "wide32", short["form"]
        want = ref.panel_update("mu", case["P"], case["slabs"], case["Q"], lv, ref.eps_of(np.float32), 32, u, split_q=True)
        b_new = ref.gamma(2, u) * want["new"] if kind == "exact" else want["b_new"]
        bounds = ref.side_bounds(want["new"], b_new, want["num"], 0 * want["num"] if kind == "exact" else want["b_num"], lv, 32, u)
        for name, got in (("long", long), ("wide_f32", short)):
            assert np.all(np.isfinite(got["P"])) and np.all(got["P"][lv:] == 0) and np.all(got["P"][:, RANKS[RP]:] == 0), (name, kind)
            assert np.all(np.isfinite(got["sumsq_part"][:len_pad // 32])) and np.all(np.isnan(got["sumsq_part"][len_pad // 32:])), (name, kind)
            if with_ps:
                assert np.all(np.isfinite(got["ps"][:lv])) and np.all(np.isnan(got["ps"][lv:])), (name, kind)
            if kind == "exact":
                assert cases.worst_ratio(got["P"], want["new"], b_new) <= 1, name
            else:
                within(name, "P", np.float32, got["P"], want["new"], b_new, f"RP={RP} ps={with_ps}")
                within(name, "sumsq_part", np.float32, got["sumsq_part"][:len_pad // 32], want["sumsq_part"], bounds["sumsq_part"], f"RP={RP} ps={with_ps}")
                if with_ps:
                    within(name, "ps", np.float32, got["ps"][:lv], want["ps"], bounds["ps"], f"RP={RP}")
        assert cases.worst_ratio(long["P"], short["P"], 2 * b_new) <= 1


def fused_args(kind, side, RP, r, dtype):
    sc = cases.scale_vector(kind, RP, dtype)
    if side == "w":
        return {"old_scale": sc}, {"old_scale": sc}
    smooth = side == "h_smooth"
    # (exact cases: theta / r and 1 - theta + theta / r are not dyadic, so the smoothed form is held to its bound there too)
    kw = {"h_side": True, "scale": sc, "smooth": smooth, "off": 0.5 / r, "diag": 0.5 + 0.5 / r, "r": r}
    return dict(kw, smooth_out=smooth), kw


@pytest.mark.parametrize("side", ["w", "h", "h_smooth"])
@pytest.mark.parametrize("dtype,RP", [("float32", 128), ("float32", 256), ("float32", 384), ("float32", 512), ("float64", 64), ("float64", 128), ("float64", 192),
                                      ("float64", 256), ("float64", 320), ("float64", 384), ("float64", 448), ("float64", 512)])
def test_fused_forms(dtype, RP, side):
    """The launches the default engines run: launch_panel_update_wide_f32(..., fused) with Q as its split image, launch_panel_update64_f64 /
    launch_panel_update_wide_f64(..., fused).  W side: the panel's pending scale on the old values; H side: D and S around the r x r product."""
    dt = np.dtype(dtype).type
    f32 = dt == np.float32
    u = ref.unit_roundoff(dt)
    form = "wide_f32_fused" if f32 else ("f64_64_fused" if RP == 64 else "wide_f64_fused")
    r = RANKS[RP]
    for kind in ("exact", "random"):
        for len_pad, lv, S in SHAPES[1:]:
            case = cases.make_case(kind, "mu", RP, r, len_pad, lv, S, dt)
            fused, kw = fused_args(kind, side, RP, r, dt)
            if f32:
                fused["x3"] = True
            got = launch(case, "mu", fused=fused)
            assert got["form"] == ("wide32_fused" if f32 else "other")
            parts = got["parts"]
            want = ref.fused_update(case["P"], case["slabs"], case["Q"], lv, ref.eps_of(dt), len_pad // parts, u, split_q=f32, **kw)
            what = f"{kind} {side} RP={RP} len_pad={len_pad} len_valid={lv} S={S}"
            P, ps, sq = got["P"], got["ps"], got["sumsq_part"]
            assert np.all(np.isfinite(P)) and np.all(P[lv:] == 0) and np.all(P[:, r:] == 0), what
            assert np.all(np.isfinite(ps[:lv])) and np.all(np.isnan(ps[lv:])) and np.all(np.isfinite(sq[:parts])) and np.all(np.isnan(sq[parts:])), what
            if kind == "exact" and side != "h_smooth":
                # powers of two as scales: numerator and denominator stay exact, two roundings as in the plain forms
                b_new = ref.gamma(2, u) * want["new"]
                assert cases.worst_ratio(P, want["new"], b_new) <= 1, what
                bounds = ref.side_bounds(want["new"], b_new, want["num"], 0 * want["num"], lv, len_pad // parts, u)
                assert cases.worst_ratio(ps[:lv], want["ps"], bounds["ps"]) <= 1 and cases.worst_ratio(sq[:parts], want["sumsq_part"], bounds["sumsq_part"]) <= 1, what
            else:
                within(form, "P", dt, P, want["new"], want["b_new"], what)
                within(form, "ps", dt, ps[:lv], want["ps"], want["bounds"]["ps"], what)
                within(form, "sumsq_part", dt, sq[:parts], want["sumsq_part"], want["bounds"]["sumsq_part"], what)
            if side == "h_smooth":
                sm = got["smooth_out"]
                assert np.all(np.isfinite(sm)) and np.all(sm[lv:] == 0) and np.all(sm[:, r:] == 0), what
                within(form, "smooth_out", dt, sm, want["smooth_out"], want["b_image"], what)
            if f32:
                # the image is that of what the next product multiplies with, bit for bit
                assert np.array_equal(got["x3"], got["smooth_out"] if side == "h_smooth" else P), what


def test_refusals_leave_every_output_alone():
    """What the launchers reject comes back as NMFAMD_INVALID_ARGUMENT (status 1), nothing launched: the arrays handed in keep their NaN."""
    def refused(case, mode, **kw):
        ps = np.full(case["len_pad"], np.nan, case["P"].dtype)
        sumsq = np.full((case["len_pad"] // 4, case["RP"]), np.nan, case["P"].dtype)
        P0 = case["P"].copy()
        with pytest.raises(na.EngineError) as e:
            na.op_panel_update(mode, case["P"], case["slabs"], case["Q"], case["len_valid"], ps=ps, sumsq_part=sumsq, **kw)
        assert e.value.status == 1, (mode, kw)
        assert np.all(np.isnan(ps)) and np.all(np.isnan(sumsq)) and np.array_equal(case["P"], P0)

    c64, c128, c256 = (cases.make_case("random", "mu", RP, RANKS[RP], 128, 100, 2, np.float32) for RP in (64, 128, 256))
    d64 = cases.make_case("random", "mu", 64, 33, 128, 100, 2, np.float64)
    refused(c128, "mu", gram_partial=True)            # gram_partial away from RP 64
    refused(c128, "mu", x3=True)
    refused(d64, "mu", gram_partial=True)             # ... and away from float32
    refused(d64, "mu", x3=True)
    refused(c64, "set", gram_partial=True)            # MODE_SET with gram_partial
    refused(c64, "mu", tri=True)                      # tri away from RP 256
    refused(c128, "mu", tri=True)
    refused(d64, "mu", tri=True)
    refused(c256, "ls", tri=True)                     # tri with anything but MODE_MU
    refused(c128, "ls", fused={"old_scale": np.ones(128)})      # the fused launch is multiplicative only
    refused(c64, "mu", fused={"old_scale": np.ones(64)})        # ... and float32 has it at the wide ranks only
    # tri at RP 256 / MODE_MU is accepted: all-default extras are the plain update
    got = launch(c256, "mu", tri=True, split_q=True)
    assert np.array_equal(got["P"], launch(c256, "mu", split_q=True)["P"])


@pytest.mark.parametrize("kind", ["exact", "random"])
def test_eps_decides_where_the_denominator_vanishes(kind, monkeypatch):
    """cases.tiny_row: the old values of row 0 are all but zero, its denominator vanishes against eps and the row is old * num / eps -- what a kernel without its
    eps, or with another one, gets wrong by orders of magnitude (tests/test_panel_update_cpu.py shows that defect leaving the bound on exactly these inputs).
    Every form once, float32 and float64."""
    for dtype, RP, split_q, fused, forced in (("float32", 64, False, False, False), ("float32", 192, False, False, False), ("float32", 256, False, False, False),
                                              ("float32", 256, True, False, False), ("float32", 128, False, True, False), ("float32", 128, False, False, True),
                                              ("float64", 64, False, False, False), ("float64", 320, False, False, False), ("float64", 64, False, True, False),
                                              ("float64", 256, False, True, False), ("float64", 128, False, False, True)):
        dt = np.dtype(dtype).type
        u = ref.unit_roundoff(dt)
        len_pad, lv, S = SHAPES[2]
        case = cases.tiny_row(cases.make_case(kind, "mu", RP, RANKS[RP], len_pad, lv, S, dt))
        what = f"{kind} {dtype} RP={RP} split_q={split_q} fused={fused} forced={forced}"
        if forced:
            monkeypatch.setenv("NMFAMD_FORCE_VALU", "1")
        if fused:
            sc = cases.scale_vector(kind, RP, dt)
            got = launch(case, "mu", fused={"old_scale": sc})
            want = ref.fused_update(case["P"], case["slabs"], case["Q"], lv, ref.eps_of(dt), len_pad // got["parts"], u, split_q=dt == np.float32, old_scale=sc)
        else:
            got = launch(case, "mu", split_q=split_q)
            want = ref.panel_update("mu", case["P"], case["slabs"], case["Q"], lv, ref.eps_of(dt), len_pad // got["parts"], u, split_q=split_q)
        if forced:
            monkeypatch.delenv("NMFAMD_FORCE_VALU")
        assert np.all(np.isfinite(got["P"])) and np.any(got["P"][0] > 0), what
        # (exact case: the denominator of row 0 is far below half an ulp of eps, den + eps = eps exactly, and the quotient by a power of two is exact)
        bound = ref.gamma(2, u) * want["new"] if kind == "exact" else want["b_new"]
        assert cases.worst_ratio(got["P"], want["new"], bound) <= 1, f"{what}: {cases.worst_ratio(got['P'], want['new'], bound):.3g} of the bound"
        if kind == "exact":
            assert cases.same_bits(got["P"][0], want["new"][0], dt), what


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_one_iteration_of_the_generic_sequence_is_the_chain_of_these_launches(dtype, monkeypatch):
    """Operations against the engine, so that the entry cannot drift from what the engine launches: iterations under NMFAMD_NO_FUSED_MU (the generic sequence:
    product, Gram matrix, launch_panel_update, normalisation) on a 150 x 130 problem at rank 20.
      H: one iteration with W held constant, then the same launch through op_panel_update on the slabs and the Gram matrix W^T W the engine left behind: the
         engine's H, bit for bit.
      W: one whole iteration, then op_panel_update on the W step's slabs and H H^T, from the W handed in: the engine's W is that panel divided by the square root
         of the summed partial sums of squares (launch_normalize_panel) -- restated in the engine's type and held to gamma(parts + 2): the sum of `parts`
         partials in any order, the square root (which halves the sum's error and rounds once), the division."""
    monkeypatch.setenv("NMFAMD_NO_FUSED_MU", "1")
    dt = np.dtype(dtype).type
    u = ref.unit_roundoff(dt)
    m, n, r = 150, 130, 20
    rng = np.random.default_rng(11)
    V = np.asfortranarray(rng.random((m, n)).astype(dt))
    W0 = np.asfortranarray((0.1 + rng.random((m, r))).astype(dt))
    H0 = np.asfortranarray((0.1 + rng.random((r, n))).astype(dt))

    def engine_run(constant_w):
        eng = na.Engine(m, n, r, "mu", dtype=dt)
        try:
            eng.upload(V)
            eng.set_factors(W0, H0)
            eng.iterate(1, first_iteration=1, error_every=1000, constant_w=constant_w)
            W1, H1 = eng.get_factors()
            geo = eng.geometry()
            RP, npad, mpad = geo["padded_rank"], geo["padded_n"], geo["padded_m"]
            S = geo["slabs_h"] if constant_w else geo["slabs_w"]
            stride = RP * max(mpad, npad)
            slabs = eng.debug_read(4, stride * S).reshape(S, stride)
            Q = eng.debug_read(2 if constant_w else 3, RP * RP).reshape(RP, RP)
        finally:
            eng.close()
        assert RP == 64 and S >= 1
        return W1, H1, slabs, Q, mpad, npad

    _, H1, slabs, G, mpad, npad = engine_run(True)
    Hp = np.zeros((npad, 64), dt); Hp[:n, :r] = H0.T
    got = na.op_panel_update("mu", Hp, slabs, G, n)
    assert np.array_equal(got["P"][:n, :r].T, H1), "H of the engine differs from the same launch through op_panel_update"
    assert np.all(got["P"][n:] == 0) and np.all(got["P"][:, r:] == 0)

    W1, H1b, slabs, HHt, mpad, npad = engine_run(False)
    assert np.array_equal(H1b, H1)
    Wt = np.zeros((mpad, 64), dt); Wt[:m, :r] = W0
    w = na.op_panel_update("mu", Wt, slabs, HHt, m, sumsq_part=np.full((mpad // 4, 64), np.nan, dt))
    parts = w["parts"]
    sumsq = w["sumsq_part"][:parts].sum(axis=0, dtype=dt)
    norm = np.sqrt(sumsq)
    want = (w["P"] / np.where(norm > 0, norm, dt(1)))[:m, :r]
    assert want.dtype == dt
    ratio = cases.worst_ratio(W1, want, ref.gamma(parts + 2, u) * np.abs(want))
    assert ratio <= 1, f"W of the engine is {ratio:.3g} of gamma(parts + 2) from the chain of operations"
