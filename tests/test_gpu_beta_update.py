"""The update launch of the dense beta-divergence half-step (launch_beta_update, k_beta_update<T, EXT>) alone through na.op_beta_update on caller-built partial panels,
element-wise against the restatement of tests/beta_kernel_reference.py -- and the ties that keep the two test entries from drifting from what the project runs:
op_beta_update(op_beta_fused(...)) is op_beta_half_step* bit for bit, one H step of an engine is this pair of launches, and k_beta_update_rows without accumulators
returns launch_beta_update's panel (docs/DIVERGENCE.md, "Kernel-level tests").

Every combination is named in its id: {float32, float64} x RP {64, 128, 256} x beta {1, 0, -1, 0.5, 1.5, 2, 3} (the vector denominator, the square root, the
general power below 1 and above 2, gamma = 1 on a panel denominator) x {update, update + terms, terms only}; the slab counts 1, 2, 3, 16, the penalties and the
weighted engines' launch walk through them (tests/beta_kernel_cases.py, update_calls).

Expectations: bits on the exact cases (integer partial panels whose slab sums are powers of two), bounds on the random ones; the partial panels hold NaN on padding
rows and on columns >= r and the panel holds 7 there: the new panel is exactly 0 on them and both sums are finite; what the launch does not write is still NaN."""
import numpy as np
import pytest

import nmfgpu_amd as na
from tests import beta_kernel_cases as cases
from tests import beta_kernel_reference as kref

pytestmark = pytest.mark.gpu

WORST = {}
PINNED = {}     # what the ties found, printed when the module is done


@pytest.fixture(scope="module", autouse=True)
def _library_is_native():
    assert na.device_count() >= 1, "GPU tests need a HIP device"
    yield
    for (form, dtype, output), ratio in sorted(WORST.items()):
        print(f"\nworst error / bound  update {form:<14} {dtype:<8} {output:<10}: {ratio:.3f}", end="")
    for key, value in sorted(PINNED.items()):
        print(f"\n{key}: {value}", end="")
    print()


def within(form, dtype, output, got, want, what):
    ratio = cases.worst_ratio(got, want.v, want.b)
    key = (form, np.dtype(dtype).name, output)
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    assert ratio <= 1, f"{form} {output} {what}: worst error / bound {ratio:.3g}"


def power_of(beta):
    g = kref.gamma_of(beta)
    return "gamma 1" if g == 1.0 else "square root" if g == 0.5 else "general power"


def launch(case, *, weighted=False, update=True, terms=False):
    return na.op_beta_update(case["P"], case["num_part"], case["den"], case["r"], case["out_valid"], case["beta"], l1=case["l1"], l2=case["l2"], weighted=weighted,
                             update=update, terms=case["terms"] if terms else None)


def check(case, got, what, *, weighted=False, update=True, terms=False):
    dt, RP, r, ov, out_pad = case["dtype"], case["RP"], case["r"], case["out_valid"], case["out_pad"]
    want = kref.update(case["P"], case["num_part"], case["den"], r, ov, case["beta"], dt, l1=case["l1"], l2=case["l2"], weighted=weighted,
                       terms=case["terms"] if terms else None, exact=case["exact"])
    P, sq, sm = got["P"], got["sumsq_part"], got["sum_part"]
    outputs = []
    if update:
        assert np.all(np.isfinite(P)), f"{what}: NaN reached the panel"
        assert np.all(P[ov:] == 0) and np.all(P[:, r:] == 0), f"{what}: padding rows / rank columns past r are not exact zeros"
        assert np.all(np.isfinite(sq)) and np.all(np.isfinite(sm)), f"{what}: the sums are not finite"
        assert np.all(sq[:, r:] == 0) and np.all(sm[:, r:] == 0), what
        outputs += [("P", P, want["new"]), ("sumsq_part", sq, want["sumsq_part"]), ("sum_part", sm, want["sum_part"])]
    else:
        assert np.array_equal(P, case["P"]), f"{what}: the terms-only launch touched the panel"
        assert np.all(np.isnan(sq)) and np.all(np.isnan(sm)), f"{what}: the terms-only launch wrote the sums"
    if terms:
        assert np.all(np.isfinite(got["t_frob"])) and np.all(np.isfinite(got["t_div"])), what
        outputs += [("t_frob", got["t_frob"], want["t_frob"]), ("t_div", got["t_div"], want["t_div"])]
    else:
        assert got["t_frob"] is None and got["t_div"] is None
    form = power_of(case["beta"]) + (", penalised" if case["l1"] or case["l2"] else "")
    for name, g, w in outputs:
        if case["exact"]:
            assert cases.same_bits(g, w.v, dt), f"{form} {name} {what}: differs at {np.argwhere(np.asarray(g, dtype=np.float64) != w.v)[:4].tolist()}"
        else:
            within(form, dt, name, g, w, what)
    return want


COMBINATIONS = [(dtype, RP, beta, outputs) for dtype in ("float32", "float64") for RP in cases.RANKS for beta in cases.UPDATE_BETAS for outputs in cases.OUTPUTS]


@pytest.mark.parametrize("dtype,RP,beta,outputs", COMBINATIONS, ids=["-".join(map(str, t)) for t in COMBINATIONS])
def test_every_combination_against_the_restatement(dtype, RP, beta, outputs):
    update, terms = outputs != "terms", outputs != "update"
    for call in cases.update_calls(dtype, RP, beta, outputs):
        weighted = call.get("weighted", False)
        case = cases.update_case(dtype=dtype, RP=RP, beta=beta, **{k: v for k, v in call.items() if k != "weighted"})
        got = launch(case, weighted=weighted, update=update, terms=terms)
        check(case, got, f"{call}", weighted=weighted, update=update, terms=terms)
        c0 = case["zero_den_column"]
        if c0 is not None and update:
            # den + eps = eps: old * num / eps, which a launch without its eps turns into a division by zero
            assert np.all(np.isfinite(got["P"][:, c0])) and np.all(got["P"][:case["out_valid"], c0] > 0), call
            if case["exact"]:
                num = np.nansum(case["num_part"][:, :case["out_valid"], c0].astype(np.float64), axis=0)
                a = case["P"][:case["out_valid"], c0].astype(np.float64)
                assert np.array_equal(got["P"][:case["out_valid"], c0].astype(np.float64), a * num / kref.eps_of(dtype)), call


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("beta", [1.0, 0.0, 1.5, 2.0, 3.0])
def test_ext_and_plain_launches_return_the_same_bits(beta, dtype):
    """No penalty, gamma in {1, 1/2}: k_beta_update<T, false> (the launch beta = 0 and beta = 1 always had) and k_beta_update<T, true> (reached here through
    `weighted`, which takes the denominator as a panel at every beta) run the same arithmetic."""
    for RP, S in ((64, 3), (256, 16)):
        for kind in ("random", "exact"):
            case = cases.update_case(kind, dtype, RP, RP - 3, 256, 129, S, beta, vec=False)
            plain = dict(case)
            if beta == 1:
                # the plain launch takes the vector: a panel whose slabs add up to it, exactly (one slab holds it, the others zero)
                vec = cases.update_case(kind, dtype, RP, RP - 3, 256, 129, S, beta)
                plain["den"] = vec["den"]
                den = np.zeros_like(case["den"]); den[0] = vec["den"][None, :]
                case["den"] = den
            a = launch(plain, terms=True)
            b = launch(case, weighted=True, terms=True)
            for key in ("P", "sumsq_part", "sum_part", "t_frob", "t_div"):
                assert np.array_equal(a[key], b[key]), f"{key} RP={RP} {kind}: the EXT launch differs from the plain one"


def test_refusals_of_launch_beta_update():
    """What launch_beta_update rejects comes back as NMFAMD_INVALID_ARGUMENT (status 1), nothing launched."""
    c = cases.update_case("random", "float32", 64, 61, 128, 100, 2, 0.0)
    v = cases.update_case("random", "float32", 64, 61, 128, 100, 2, 1.0)

    def refused(P, num, den, r, ov, beta, **kw):
        with pytest.raises(na.EngineError) as e:
            na.op_beta_update(P, num, den, r, ov, beta, **kw)
        assert e.value.status == 1, (beta, kw)

    refused(c["P"], c["num_part"], c["den"], 0, 100, 0.0)                         # r < 1
    refused(c["P"], c["num_part"], c["den"], 65, 100, 0.0)                        # r > RP
    refused(c["P"], c["num_part"], c["den"], 61, 100, np.inf)                     # a non-finite beta
    refused(c["P"], c["num_part"], c["den"], 61, 100, 0.0, l1=-1.0)               # negative penalties
    refused(c["P"], c["num_part"], c["den"], 61, 100, 0.0, l2=np.inf)
    refused(c["P"], c["num_part"], None, 61, 100, 0.0, slabs=2)                   # beta != 1 needs den_part
    refused(c["P"], c["num_part"], c["den"], 61, 100, 1.0)                        # the unweighted beta = 1 needs dsum ...
    refused(v["P"], v["num_part"], v["den"], 61, 100, 1.0, weighted=True)         # ... and the weighted one den_part
    refused(c["P"], None, c["den"], 61, 100, 0.0, slabs=2)                        # an update needs num_part
    refused(c["P"], c["num_part"], c["den"], 61, 100, 0.0, update=False)          # neither update nor terms
    refused(c["P"][:, :48], c["num_part"][:, :, :48], c["den"][:, :, :48], 40, 100, 0.0)      # no launch at RP 48
    refused(c["P"], c["num_part"], c["den"], 61, 129, 0.0)                        # the entry's own: out_valid past out_pad
    # accepted: the terms alone need no partial panels
    got = na.op_beta_update(c["P"], None, None, 61, 100, 0.0, update=False, terms=c["terms"])
    assert np.array_equal(got["P"], c["P"]) and np.all(np.isfinite(got["t_frob"]))


HALF_STEPS = [("plain", "float32"), ("plain", "float64"), ("general", "float32"), ("general", "float64"), ("weighted", "float32"), ("weighted", "float64"),
              ("mixed", "float32")]


@pytest.mark.parametrize("entry,dtype", HALF_STEPS, ids=[f"{e}-{d}" for e, d in HALF_STEPS])
def test_the_two_entries_chained_are_the_half_step_entry_bit_for_bit(entry, dtype):
    """op_beta_update(op_beta_fused(...)) against op_beta_half_step / _general / _weighted / _mixed: the same plan, the same launches, the same bits -- panel,
    sums and terms, at every form (0 update, 1 update + terms, 2 terms only)."""
    form = {"plain": "plain", "general": "plain"}.get(entry, entry)
    betas = [1.0, 0.0] if entry == "plain" else [1.0, 0.0, 0.5, 3.0]
    pen = (0.0, 0.0) if entry == "plain" else (0.05, 0.5)
    for RP, beta in [(RP, betas[i % len(betas)]) for i, RP in enumerate((64, 128, 256, 64))]:
        for kind_form in (0, 1, 2):
            r, out_pad, ov, rv, fs = RP - 3, 256, 129, 383, kind_form
            case = cases.fused_case("random", form, dtype, RP, r, out_pad, ov, rv, seed=kind_form, nan_padding=False)
            A, B, X = case["A"], case["B"], np.nan_to_num(case["X"], nan=1.0)
            Om = case["Omega"]
            dsum = B.sum(axis=0, dtype=B.dtype) if beta == 1 and form != "weighted" else None
            update, terms = kind_form != 2, kind_form != 0
            if entry == "plain":
                whole = na.op_beta_half_step(A, B, X, r, ov, rv, int(beta), kind_form, dsum=dsum, force_slabs=fs)
            elif entry == "general":
                whole = na.op_beta_half_step_general(A, B, X, r, ov, rv, beta, kind_form, l1=pen[0], l2=pen[1], dsum=dsum, force_slabs=fs)
            elif entry == "weighted":
                whole = na.op_beta_half_step_weighted(A, B, X, Om, r, ov, rv, beta, kind_form, l1=pen[0], l2=pen[1], force_slabs=fs)
            else:
                whole = na.op_beta_half_step_mixed(A, B, X, r, ov, rv, beta, kind_form, l1=pen[0], l2=pen[1], dsum=dsum, force_slabs=fs)
            fused = na.op_beta_fused(A, B, X, ov, rv, beta, update=update, terms=terms, Omega=Om, mixed=form == "mixed", force_slabs=fs)
            assert fused["slabs"] == whole["slabs"]
            den = dsum if dsum is not None else fused["den_part"]
            got = na.op_beta_update(A, fused["num_part"] if update else None, den if update else None, r, ov, beta, l1=pen[0], l2=pen[1], weighted=form == "weighted",
                                    update=update, terms=(fused["tf_part"], fused["td_part"]) if terms else None, slabs=fused["slabs"])
            what = f"{entry} {dtype} RP={RP} beta={beta} form={kind_form}"
            assert np.array_equal(got["P"], whole["A"]), what
            if update:
                assert np.array_equal(got["sumsq_part"], whole["sumsq_part"]) and np.array_equal(got["sum_part"], whole["sum_part"]), what
            if terms:
                assert np.array_equal(got["t_frob"], whole["t_frob"]) and np.array_equal(got["t_div"], whole["t_div"]), what


ENGINES = [("float32", 1.0, ""), ("float32", 0.0, ""), ("float32", 0.5, ""), ("float64", 1.0, ""), ("float64", 0.0, ""), ("float64", 0.5, ""),
           ("float32", 0.5, "weighted"), ("float32", 0.0, "mixed")]


@pytest.mark.parametrize("dtype,beta,kind", ENGINES, ids=[f"{d}-beta{b}{'-' + k if k else ''}" for d, b, k in ENGINES])
def test_one_h_step_of_an_engine_is_this_pair_of_launches(dtype, beta, kind):
    """iterate(1, constant_w=True) from set factors against op_beta_fused + op_beta_update on the panels and the V image the engine holds (debug_read 0, 1, 6) with the
    engine's slab count: the engine's H, bit for bit.  The engine plans with plan_beta_half_step as the entry does, so force_slabs = slabs_h reproduces its plan."""
    dt = np.dtype(dtype).type
    m, n, r = 200, 190, 20
    rng = np.random.default_rng(17)
    from tests import beta_reference as ref
    V = np.asfortranarray(ref.planted(m, n, seed=4).astype(dt))
    W0, H0 = ref.start(m, n, r, 5, dt)
    Om = None
    kw = {}
    if kind == "weighted":
        Om = np.asfortranarray(np.where(rng.random((m, n)) < 0.3, 0.0, 0.5 + rng.random((m, n))).astype(dt))
        kw["weighted"] = True
    if kind == "mixed":
        kw["mixed_precision"] = True
    if beta == 1:
        eng = na.Engine(m, n, r, "mu", dtype=dt, divergence="kl", dense_compute=True, **kw)
    elif beta == 0:
        eng = na.Engine(m, n, r, "mu", dtype=dt, divergence="is", **kw)
    else:
        eng = na.Engine(m, n, r, "mu", dtype=dt, divergence="beta", beta=beta, **kw)
    try:
        eng.upload(V, Om) if Om is not None else eng.upload(V)
        eng.set_factors(W0, H0)
        geo = eng.geometry()
        RP, npad, mpad = geo["padded_rank"], geo["padded_n"], geo["padded_m"]
        Wp = eng.debug_read(0, RP * mpad).reshape(mpad, RP)
        Hp = eng.debug_read(1, RP * npad).reshape(npad, RP)
        X = eng.debug_read(6, mpad * npad).reshape(npad, mpad)
        eng.iterate(1, first_iteration=1, error_every=1000, constant_w=True)
        H1 = eng.debug_read(1, RP * npad).reshape(npad, RP)
    finally:
        eng.close()
    assert np.array_equal(Wp[:m, :r], W0) and np.array_equal(Hp[:n, :r], H0.T) and (Om is not None or np.array_equal(X[:n, :m], V.T))
    red_pad = -(-m // 128) * 128
    assert npad % 128 == 0 and mpad >= red_pad
    OmX = None
    if Om is not None:
        OmX = np.zeros((npad, mpad), dt); OmX[:n, :m] = Om.T
    fused = na.op_beta_fused(Hp, Wp[:red_pad], X, n, m, beta, Omega=OmX, mixed=kind == "mixed", force_slabs=geo["slabs_h"])
    assert fused["slabs"] == geo["slabs_h"]
    vec = beta == 1 and kind != "weighted"
    den = na.op_panel_rowsum(Wp) if vec else fused["den_part"]
    got = na.op_beta_update(Hp, fused["num_part"], den, r, n, beta, weighted=kind == "weighted")
    assert np.array_equal(got["P"], H1), "H of the engine differs from the same pair of launches through the entries"
    assert np.any(H1[:n, :r] != Hp[:n, :r])


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("beta", cases.UPDATE_BETAS)
def test_update_rows_without_accumulators_against_the_update_launch(beta, dtype):
    """k_beta_update_rows (the minibatch engines' update launch, 16 rows per workgroup) and k_beta_update on the same partial panels: both within the update's
    bounds of the restatement.  Whether their panels are bit-identical is recorded -- docs/NEXT.md 7 needs that fact before the full-batch engines move onto
    k_beta_update_rows -- and pinned: they are, with and without penalties, at every gamma (docs/DIVERGENCE.md)."""
    same = True
    for RP, S, pen in ((64, 1, False), (128, 3, True), (256, 16, False), (256, 2, True)):
        case = cases.update_case("random", dtype, RP, RP - 3, 256, 129, S, beta, penalised=pen, seed=S)
        full = launch(case)
        want = check(case, full, f"RP={RP} S={S} pen={pen}")
        # (the rows kernel reads its partial panels on the valid coordinates only, like the update launch: the NaN stay)
        rows = na.op_beta_update_rows(case["P"], case["num_part"], case["den"], case["r"], case["out_valid"], beta, l1=case["l1"], l2=case["l2"])
        assert np.all(np.isfinite(rows["P"])) and np.all(rows["P"][129:] == 0) and np.all(rows["P"][:, RP - 3:] == 0)
        within("rows kernel", case["dtype"], "P", rows["P"], want["new"], f"RP={RP} S={S} pen={pen}")
        same = same and np.array_equal(rows["P"], full["P"])
        # the 16-row sums add up to the 128-row sums within the sums' bound
        sums = rows["sum_part"].astype(np.float64).reshape(2, 8, RP).sum(axis=1)
        assert cases.worst_ratio(sums, want["sum_part"].v, want["sum_part"].b) <= 1
    PINNED[f"k_beta_update_rows == k_beta_update, bit for bit ({dtype}, beta {beta})"] = same
    assert same, "the panels of k_beta_update_rows and k_beta_update differ in bits"
