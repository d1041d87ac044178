"""The fused launch of the dense beta-divergence half-step, one launch at a time through na.op_beta_fused, per slab and element-wise against the restatement of
tests/beta_kernel_reference.py (docs/DIVERGENCE.md, "Kernel-level tests": the layouts, the rounding counts behind the bounds, the measured constants and the table
of worst ratios; tests/test_beta_kernel_cpu.py checks restatement, cases and bounds without a device).

Every instantiation runs at least once and is named in its test id: {plain float32 (MFMA), plain float64 (VALU), weighted float32, weighted float64, mixed} x RP
{64, 128, 256} x {beta = 1, beta = 0, general} x {update, update + terms, terms only}.

Three kinds of expectation:
  exact       cases a, b, c of tests/beta_kernel_cases.py: num_part, den_part and (case a) tf_part are the restatement's bits; td_part goes through a logarithm and
              is held to its bound, as are the terms of the vanishing row;
  arithmetic  random data: every element of every slab within a bound that holds for any order of summation;
  written     every output starts as NaN, and X and Omega hold NaN on every position outside the valid block: all out_pad x RP values of every slab's num_part
              are written (exact zeros on rows >= out_valid), den_part at beta != 1 or with weights -- and is still NaN at the unweighted beta = 1 --, the terms
              for all out_pad rows; without `update` the partial panels are still NaN."""
import numpy as np
import pytest

import nmfgpu_amd as na
from tests import beta_kernel_cases as cases
from tests import beta_kernel_reference as kref

pytestmark = pytest.mark.gpu

WORST = {}      # (form, dtype, output) -> worst observed error / bound over the random cases, printed when the module is done


@pytest.fixture(scope="module", autouse=True)
def _library_is_native():
    assert na.device_count() >= 1, "GPU tests need a HIP device"
    yield
    for (form, dtype, output), ratio in sorted(WORST.items()):
        print(f"\nworst error / bound  fused {form:<9} {dtype:<8} {output:<9}: {ratio:.3f}", end="")
    print()


def within(form, dtype, output, got, want, what):
    ratio = cases.worst_ratio(got, want.v, want.b)
    key = (form, np.dtype(dtype).name, output)
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    assert ratio <= 1, f"{form} {output} {what}: worst error / bound {ratio:.3g}"


def launch(case, beta, *, update=True, terms=False, force_slabs=0):
    return na.op_beta_fused(case["A"], case["B"], case["X"], case["out_valid"], case["red_valid"], beta, update=update, terms=terms, Omega=case["Omega"],
                            mixed=case["form"] == "mixed", force_slabs=force_slabs)


def restate(case, beta, got, *, update=True, terms=False):
    return kref.fused(case["A"], case["B"], case["X"], case["out_valid"], case["red_valid"], beta, got, case["dtype"], Omega=case["Omega"],
                      mixed=case["form"] == "mixed", update=update, terms=terms, exact=case["exact"])


def check(case, beta, got, what, *, update=True, terms=False, general_key=""):
    """One launch against its restatement: the plan, what was and was not written, then bits or bounds."""
    dt, form = case["dtype"], case["form"]
    out_pad, RP, ov = case["out_pad"], case["RP"], case["out_valid"]
    f32 = dt == np.float32
    assert (got["bo"], got["kt"]) == (((64, 64) if RP == 256 else (32, 128)) if f32 else (8, 32)), what
    assert got["tiles"] == cases.RED_PAD // got["kt"] and got["slabs"] == -(-got["tiles"] // got["tiles_per_slab"]) and 1 <= got["slabs"] <= 16, what
    S = got["slabs"]
    num, den, tf, td = got["num_part"], got["den_part"], got["tf_part"], got["td_part"]
    assert num.shape == den.shape == (S, out_pad, RP)
    has_den = update and (beta != 1 or form == "weighted")
    # written
    if update:
        assert np.all(np.isfinite(num)), f"{what}: num_part is not written everywhere"
        assert np.all(num[:, ov:] == 0), f"{what}: num_part rows past out_valid are not exact zeros"
    else:
        assert np.all(np.isnan(num)), f"{what}: the terms-only launch wrote num_part"
    if has_den:
        assert np.all(np.isfinite(den)) and np.all(den[:, ov:] == 0), f"{what}: den_part is not written everywhere"
    else:
        assert np.all(np.isnan(den)), f"{what}: den_part must be left alone"
    if terms:
        assert tf.shape == td.shape == (S, out_pad) and np.all(np.isfinite(tf)) and np.all(np.isfinite(td)), f"{what}: the terms are not written for every row"
        assert np.all(tf[:, ov:] == 0) and np.all(td[:, ov:] == 0), what
    else:
        assert tf is None and td is None
    want = restate(case, beta, got, update=update, terms=terms)
    key = form + general_key
    outputs = []
    if update:
        outputs.append(("num_part", num, want["num"], True))
    if has_den:
        outputs.append(("den_part", den, want["den"], True))
    if terms:
        outputs.append(("tf_part", tf, want["tf"], case["kind"] == "a"))
        outputs.append(("td_part", td, want["td"], False))
    for name, g, w, bits in outputs:
        if case["exact"] and bits:
            if name == "tf_part" and case["tiny"]:
                # (x - eps on the vanishing row is not representable)
                assert cases.worst_ratio(g[:, :1], w.v[:, :1], w.b[:, :1]) <= 1, what
                g, w = g[:, 1:], kref.E(w.v[:, 1:], w.b[:, 1:], w.u)
            assert cases.same_bits(g, w.v, dt), f"{key} {name} {what}: differs at {np.argwhere(np.asarray(g, dtype=np.float64) != w.v)[:4].tolist()}"
        elif case["exact"]:
            assert cases.worst_ratio(g, w.v, w.b) <= 1, f"{key} {name} {what}: {cases.worst_ratio(g, w.v, w.b):.3g} of the exact case's bound"
        else:
            within(key, dt, name, g, w, what)
    return want


INSTANTIATIONS = [(form, dtype, RP, betakind, outputs) for form, dtype in cases.FORMS for RP in cases.RANKS for betakind in ("kl", "is", "general")
                  for outputs in cases.OUTPUTS]


@pytest.mark.parametrize("form,dtype,RP,betakind,outputs", INSTANTIATIONS, ids=["-".join(map(str, t)) for t in INSTANTIATIONS])
def test_every_instantiation_per_slab_against_the_restatement(form, dtype, RP, betakind, outputs):
    update, terms = outputs != "terms", outputs != "update"
    for call in cases.fused_calls(form, dtype, RP, betakind, outputs):
        beta, fs = call["beta"], call["force_slabs"]
        case = cases.fused_case(form=form, dtype=dtype, RP=RP, **{k: v for k, v in call.items() if k not in ("beta", "force_slabs")})
        what = f"{call}"
        got = launch(case, beta, update=update, terms=terms, force_slabs=fs)
        if fs:
            assert got["slabs"] == kref.host_plan(cases.RED_PAD, RP, dtype, fs)["slabs"] and got["tiles_per_slab"] == kref.host_plan(cases.RED_PAD, RP, dtype, fs)["tiles_per_slab"], what
        check(case, beta, got, what, update=update, terms=terms, general_key=" general" if betakind == "general" else "")


FORM_IDS = [f"{f}-{d}" for f, d in cases.FORMS]


@pytest.mark.parametrize("form,dtype", cases.FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("beta", [1.0, 0.0, 0.5])
def test_invalid_positions_of_x_and_omega_are_not_read(beta, form, dtype):
    """NaN against zeros on every position outside the valid block (rows >= out_valid, columns >= red_valid, the columns between red_pad and ldx), and NaN against
    1 under every zero weight: the same bits.  beta_entry, betaw_entry and mixed_entry select those entries out before they touch x."""
    for RP, kind in ((64, "random"), (256, "a" if beta != 0.5 else "random")):
        kw = dict(kind=kind, form=form, dtype=dtype, RP=RP, r=RP - 3, out_pad=128, out_valid=33, red_valid=129, ldx=cases.RED_PAD + 16)
        a, b = cases.fused_case(**kw), cases.fused_case(nan_padding=False, **kw)
        assert np.isnan(a["X"]).sum() > np.isnan(b["X"]).sum()
        if form == "weighted":
            assert np.all(np.isnan(b["X"]) == (b["Omega"] == 0) & (np.arange(128)[:, None] < 33) & (np.arange(kw["ldx"])[None, :] < 129)) and np.any(np.isnan(b["X"]))
            b["X"] = np.where(np.isnan(b["X"]), 1, b["X"]).astype(b["X"].dtype)
        else:
            assert not np.any(np.isnan(b["X"]))
        ga, gb = launch(a, beta, terms=True, force_slabs=2), launch(b, beta, terms=True, force_slabs=2)
        for key in ("num_part", "den_part", "tf_part", "td_part"):
            assert np.array_equal(ga[key], gb[key], equal_nan=True), f"{key} RP={RP}: what lies outside the valid block reaches the result"


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("RP", cases.RANKS)
@pytest.mark.parametrize("beta", [0.0, 0.5, -1.0])
def test_all_weights_one_is_the_unweighted_launch_bit_for_bit(beta, RP, dtype):
    """The claim of kernels_beta_weighted.hip's header, on the partial panels themselves (beta != 1: at beta = 1 the unweighted launch writes no denominator)."""
    for kind in ("random", "a") if beta == 0 else ("random",):
        plain = cases.fused_case(kind, "plain", dtype, RP, RP - 3, 128, 127, 383, seed=5)
        weighted = dict(plain, form="weighted", Omega=np.where(np.isnan(plain["X"]), np.nan, 1).astype(plain["X"].dtype))
        gp, gw = launch(plain, beta, force_slabs=3), launch(weighted, beta, force_slabs=3)
        assert gp["slabs"] == gw["slabs"] == 3
        assert np.array_equal(gp["num_part"], gw["num_part"]) and np.array_equal(gp["den_part"], gw["den_part"]), (kind, beta, RP)


@pytest.mark.parametrize("form,dtype", cases.FORMS, ids=FORM_IDS)
def test_two_runs_give_the_same_bits_and_the_slab_count_stays_within_the_bounds(form, dtype):
    for RP, beta in ((64, 1.0), (128, 0.0), (256, -1.0)):
        case = cases.fused_case("random", form, dtype, RP, RP - 3, 256, 129, 384, seed=9)
        runs = {s: launch(case, beta, terms=True, force_slabs=s) for s in (1, 2, 3)}
        again = launch(case, beta, terms=True, force_slabs=3)
        for key in ("num_part", "den_part", "tf_part", "td_part"):
            assert np.array_equal(runs[3][key], again[key], equal_nan=True), f"{key}: a repeated run differs"
        one = restate(case, beta, runs[1], terms=True)
        for s in (2, 3):
            assert runs[s]["slabs"] == s
            many = restate(case, beta, runs[s], terms=True)
            for key, name in (("num_part", "num"), ("den_part", "den"), ("tf_part", "tf"), ("td_part", "td")):
                if many[name] is None:
                    continue
                # the slabs added on the host in float64 (no further rounding): within the sum of the slabs' bounds and the one-slab bound
                total = runs[s][key].astype(np.float64).sum(axis=0)
                bound = many[name].b.sum(axis=0) + one[name].b[0]
                assert np.allclose(many[name].v.sum(axis=0), one[name].v[0], rtol=1e-12, atol=1e-300)
                ratio = cases.worst_ratio(total, runs[1][key][0], bound)
                assert ratio <= 1, f"{key} RP={RP}: {s} slabs against one: {ratio:.3g} of the bounds"


def test_refusals_of_the_entry():
    case = cases.fused_case("random", "plain", "float32", 64, 61, 128, 100, 300)
    for kw in (dict(update=False, terms=False), dict(mixed=True, Omega=np.ones_like(case["X"]))):
        with pytest.raises(na.EngineError) as e:
            na.op_beta_fused(case["A"], case["B"], case["X"], 100, 300, 1.0, **kw)
        assert e.value.status == 1, kw
    for ov, rv in ((129, 300), (100, 385), (-1, 300)):
        with pytest.raises(na.EngineError) as e:
            na.op_beta_fused(case["A"], case["B"], case["X"], ov, rv, 1.0)
        assert e.value.status == 1
    with pytest.raises(na.EngineError) as e:
        na.op_beta_fused(case["A"][:, :48], case["B"][:, :48], case["X"], 100, 300, 1.0)       # no launch at RP 48
    assert e.value.status == 1
    with pytest.raises(na.EngineError) as e:
        na.op_beta_fused(case["A"].astype(np.float64), case["B"], case["X"], 100, 300, 1.0, mixed=True)      # the mixed launch is float32 only
    assert e.value.status == 1
