"""Device-free checks of the kernel-level tests of the dense beta-divergence half-step (docs/DIVERGENCE.md, "Kernel-level tests"):
  1. the per-launch restatement of tests/beta_kernel_reference.py, summed over its slabs and pushed through its own update, is the half-step of the references the
     project already has (beta_reference, beta_general_reference, weighted_reference, beta_mixed_reference) to float64 rounding;
  2. the exact cases of tests/beta_kernel_cases.py are exact in float32 and in float64 (and in bf16 where the mixed launch runs them);
  3. every defect of beta_kernel_reference.MUTATIONS, applied to the restatement, leaves the bound on the cases the GPU modules run, at the loosest bound of each
     form: float32, RP 256, one slab, and beta = -1 for the general map.  A kernel with the defect returns the defective value within its own rounding error, so a
     defect counts as caught where it moves an element by more than TWICE the bound (on an exact case: by anything)."""
import numpy as np
import pytest

from tests import beta_general_reference as gen
from tests import beta_kernel_cases as cases
from tests import beta_kernel_reference as kref
from tests import beta_mixed_reference as mixed_ref
from tests import beta_reference as ref
from tests import weighted_reference as wref

FUSED_MUTATIONS = ("drop_tile", "drop_rank_term", "swap_row_groups", "no_eps_p", "red_valid_off_by_one", "out_valid_off_by_one", "den_from_q", "weight_twice")
UPDATE_MUTATIONS = ("no_eps_den", "out_valid_off_by_one", "drop_slab", "l2_new_value", "wrong_gamma")
# the defects only special data can show (docs/DIVERGENCE.md, "The limits of the defect checks"): eps is far below the rounding of every quotient elsewhere
ONLY_TINY = {"no_eps_p"}
ONLY_ZERO_DEN = {"no_eps_den"}


def build(call, form, dtype, RP):
    kw = {k: v for k, v in call.items() if k not in ("beta", "force_slabs")}
    return cases.fused_case(form=form, dtype=dtype, RP=RP, **kw)


def restate(case, beta, plan, *, update=True, terms=True, mutate=None):
    return kref.fused(case["A"], case["B"], case["X"], case["out_valid"], case["red_valid"], beta, plan, case["dtype"], Omega=case["Omega"],
                      mixed=case["form"] == "mixed", update=update, terms=terms, exact=case["exact"], mutate=mutate)


@pytest.mark.parametrize("form,dtype", cases.FORMS, ids=[f"{f}-{d}" for f, d in cases.FORMS])
@pytest.mark.parametrize("beta", [1.0, 0.0] + cases.GENERAL_BETAS)
def test_restatement_is_the_half_step_of_the_existing_references(beta, form, dtype):
    RP, r, out_pad, ov, rv = 64, 61, 128, 101, 300
    case = cases.fused_case("random", form, dtype, RP, r, out_pad, ov, rv, ldx=400, seed=3)
    eps = kref.eps_of(dtype)
    for pen in ((0.0, 0.0), (0.05, 0.5)):
        plan = kref.host_plan(cases.RED_PAD, RP, dtype, 3)
        assert plan["slabs"] == 3
        got = restate(case, beta, plan)
        A, B, X = (case[k].astype(np.float64) for k in ("A", "B", "X"))
        Av, Bv, Xv = A[:ov, :r], B[:rv, :r], X[:ov, :rv]
        vec = beta == 1 and form != "weighted"
        den = B.sum(axis=0) if vec else got["den"].v
        new = kref.update(A, got["num"].v, den, r, ov, beta, dtype, l1=pen[0], l2=pen[1], weighted=form == "weighted", terms=(got["tf"].v, got["td"].v))
        l1, l2 = (float(case["dtype"](p)) for p in pen)
        if form == "weighted":
            Om = case["Omega"].astype(np.float64)[:ov, :rv]
            want = wref.half_step(Xv, Om, Av, Bv, beta, eps, l1, l2)
            tf, td = wref.terms(Xv, Om, Av, Bv, beta, eps)
        elif form == "mixed":
            want = mixed_ref.half_step(Xv, Av, Bv, beta, eps, l1, l2)
            tf, td = mixed_ref.terms(Xv, Av, Bv, beta, eps)
        else:
            want = gen.half_step(Xv, Av, Bv, beta, eps, l1, l2) if pen != (0.0, 0.0) or beta not in (0, 1) else ref.half_step(Xv, Av, Bv, beta, eps)
            tf, td = gen.terms(Xv, Av, Bv, beta, eps)
        # (the launch takes gamma in the engine's type: 1/3 and 2/3 rounded to float32 move the power by up to 2^-24 |ln quo|, which the float64 references do not do)
        rtol = 1e-12 if dtype == "float64" or gen.gamma_of(beta) in (1.0, 0.5) else 2.0 ** -24 * 8
        assert np.allclose(new["new"].v[:ov, :r], want, rtol=rtol, atol=0), (beta, form, pen)
        assert np.all(new["new"].v[ov:] == 0) and np.all(new["new"].v[:, r:] == 0)
        assert np.allclose(new["t_frob"].v[:ov], tf, rtol=1e-12) and np.allclose(new["t_div"].v[:ov], td, rtol=1e-10, atol=1e-12 * np.abs(td).max())
        assert np.all(new["t_frob"].v[ov:] == 0) and np.all(new["t_div"].v[ov:] == 0)
        # the sums the update leaves: per 128 rows
        assert np.allclose(new["sumsq_part"].v.sum(axis=0), (new["new"].v ** 2).sum(axis=0), rtol=1e-13)
        assert np.allclose(new["sum_part"].v.sum(axis=0), new["new"].v.sum(axis=0), rtol=1e-13)


def test_host_plan_is_the_launchers_plan_for_a_forced_count():
    # kernels_beta.hip, plan_beta_half_step with force_slabs: tiles_per_slab = ceil(tiles / min(force, tiles, 16)), slabs = ceil(tiles / tiles_per_slab)
    assert kref.host_plan(384, 64, "float32", 2) == {"bo": 32, "kt": 128, "tiles": 3, "tiles_per_slab": 2, "slabs": 2}
    assert kref.host_plan(384, 256, "float32", 3) == {"bo": 64, "kt": 64, "tiles": 6, "tiles_per_slab": 2, "slabs": 3}
    assert kref.host_plan(384, 128, "float64", 16) == {"bo": 8, "kt": 32, "tiles": 12, "tiles_per_slab": 1, "slabs": 12}
    assert kref.host_plan(384, 128, "float64", 5)["slabs"] == 4        # (five collapses to four slabs of three tiles)
    assert [kref.slab_rows(kref.host_plan(384, 64, "float32", 2), s) for s in (0, 1)] == [(0, 256), (256, 384)]


@pytest.mark.parametrize("form,dtype", cases.FORMS, ids=[f"{f}-{d}" for f, d in cases.FORMS])
@pytest.mark.parametrize("kind,beta,tiny", [("a", 1.0, False), ("a", 0.0, False), ("a", 1.0, True), ("a", 0.0, True), ("b", 1.0, False), ("c", 1.0, False), ("c", 0.0, False)])
def test_exact_fused_cases_are_exact(kind, beta, tiny, form, dtype):
    """The claims of the exact cases, without a device: P + eps rounds to P (to eps on the tiny row) in the type, Q and R are representable (in bf16 too: the mixed
    launch rounds nothing), and every partial sum of P, num, den and -- case a -- of the squared differences is exact in any order."""
    dt = np.dtype(dtype).type
    eps = dt(np.finfo(dt).eps)
    for RP, r in ((64, 1), (128, 125), (256, 256)):
        case = cases.fused_case(kind, form, dtype, RP, r, 128, 127, 383, tiny=tiny)
        ov, rv = case["out_valid"], case["red_valid"]
        A, B = case["A"].astype(np.float64)[:ov], case["B"].astype(np.float64)[:rv]
        assert cases.sums_are_exact(A, B.T, dtype)
        P = A @ B.T
        Pt = P.astype(dt)
        assert np.array_equal(Pt.astype(np.float64), P)
        want = Pt.copy()
        if tiny:
            want[0] = eps
        assert np.array_equal(Pt + eps, want), "P + eps does not round back to P"
        W = None if case["Omega"] is None else case["Omega"].astype(np.float64)[:ov, :rv]
        Xv = case["X"].astype(np.float64)[:ov, :rv]
        u = kref.unit_roundoff(dtype)
        Q, R, tf, _ = kref.entry_map(Xv, W, kref.E(want.astype(np.float64), 0.0, u), beta, terms=kind == "a")
        for M in (Q, R):
            if M is None:
                continue
            assert np.all(np.isfinite(M.v)) and cases.fits(M.v, dtype) and cases.sums_are_exact(M.v, B, dtype)
            if dtype == "float32":
                assert np.array_equal(mixed_ref.round_bf16(M.v), M.v) and np.array_equal(mixed_ref.round_bf16(A), A) and np.array_equal(mixed_ref.round_bf16(B), B)
        if kind == "a":
            # (x - eps on the tiny row is not representable: that row's terms are held to their bounds)
            f = tf.v[1:] if tiny else tf.v
            assert cases.fits(f, dtype) and cases.sums_are_exact(f, np.ones((rv, 1)), dtype)
        if kind == "c":
            # one entry of X per output row: num(o, :) is Q(k(o), o) times row k(o) of B
            hot = (5 * np.arange(ov) + 1) % rv
            live = ~np.isnan(Xv[np.arange(ov), hot])
            assert np.array_equal((Q.v @ B)[live], (Q.v[np.arange(ov), hot][:, None] * B[hot])[live])


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("beta", [1.0, 0.0, 1.5, 2.0, 3.0])
def test_exact_update_cases_are_exact(beta, dtype):
    dt = np.dtype(dtype).type
    for RP, r, S, pen, zero in ((64, 1, 1, False, False), (128, 125, 3, True, False), (256, 256, 16, False, beta in (1.0, 1.5, 2.0)), (64, 64, 2, True, False)):
        for vec in ((None, False) if beta == 1 else (None,)):
            case = cases.update_case("exact", dtype, RP, r, 256, 129, S, beta, penalised=pen, zero_den=zero, vec=vec)
            live = (np.arange(256)[:, None] < 129) & (np.arange(RP)[None, :] < r)
            num = np.where(live[None], case["num_part"].astype(np.float64), 0.0)
            assert np.all(num == np.round(num)) and np.abs(num).sum(axis=0).max() < 2 ** 24
            den = case["den"].astype(np.float64)
            total = np.where(live, np.broadcast_to(den, (256, RP)) if den.ndim == 1 else np.where(live[None], den, 0.0).sum(axis=0), 1.0)
            d = (total.astype(dt) + dt(np.finfo(dt).eps)).astype(np.float64) + case["l1"] + case["l2"] * np.where(live, case["P"].astype(np.float64), 0.0)
            m, _ = np.frexp(d[live])
            assert np.all(m == 0.5), "a denominator is not a power of two"
            want = kref.update(case["P"], case["num_part"], case["den"], r, 129, beta, dtype, l1=case["l1"], l2=case["l2"], weighted=vec is False, terms=case["terms"], exact=True)
            for key in ("new", "sumsq_part", "sum_part", "t_frob", "t_div"):
                assert np.all(np.isfinite(want[key].v)) and cases.fits(want[key].v, dtype), (key, RP, S)
            assert cases.sums_are_exact((want["new"].v ** 2).T, np.ones((256, 1)), dtype) and np.any(want["new"].v > 0)


def moved(mut, want, exact):
    """Whether a defect shows: any other bits on an exact case, more than twice the bound otherwise."""
    for key in want:
        if want[key] is None:
            continue
        if exact:
            if not np.array_equal(mut[key].v, want[key].v):
                return True
        elif cases.worst_ratio(mut[key].v, want[key].v, 2 * want[key].b) > 1:
            return True
    return False


@pytest.mark.parametrize("form", ["plain", "weighted", "mixed"])
@pytest.mark.parametrize("betakind", ["kl", "is", "general"])
def test_every_fused_defect_leaves_the_bound(betakind, form):
    RP, dtype = 256, "float32"
    caught = {m: set() for m in FUSED_MUTATIONS}
    for outputs in ("update+terms", "update"):
        for call in cases.fused_calls(form, dtype, RP, betakind, outputs):
            case = build(call, form, dtype, RP)
            beta = -1.0 if betakind == "general" else call["beta"]
            plan = kref.host_plan(cases.RED_PAD, RP, dtype, 1)
            want = restate(case, beta, plan, terms=outputs != "update")
            for m in FUSED_MUTATIONS:
                if (m == "weight_twice" and form != "weighted") or (m == "den_from_q" and want["den"] is None):
                    continue
                if moved(restate(case, beta, plan, terms=outputs != "update", mutate=m), want, case["exact"]):
                    caught[m].add(("tiny " if case["tiny"] else "") + ("exact" if case["exact"] else "random"))
    for m, where in caught.items():
        if (m == "weight_twice" and form != "weighted") or (m == "den_from_q" and betakind == "kl" and form != "weighted"):
            continue
        assert where, f"{m} is not caught at {form} {betakind}"
        if m in ONLY_TINY:
            assert any(w.startswith("tiny") for w in where), (m, where)      # the vanishing row is where eps is sure to show
        else:
            assert "random" in where or "tiny random" in where, f"{m}: caught on {where} only"


@pytest.mark.parametrize("beta", cases.UPDATE_BETAS)
def test_every_update_defect_leaves_the_bound(beta):
    RP, dtype = 256, "float32"
    caught = {m: set() for m in UPDATE_MUTATIONS}
    for outputs in cases.OUTPUTS:
        for call in cases.update_calls(dtype, RP, beta, outputs):
            weighted = call.get("weighted", False)
            case = cases.update_case(dtype=dtype, RP=RP, beta=beta, **{k: v for k, v in call.items() if k != "weighted"})
            run = lambda mutate=None: kref.update(case["P"], case["num_part"], case["den"], case["r"], case["out_valid"], beta, dtype, l1=case["l1"], l2=case["l2"],
                                                  weighted=weighted, exact=case["exact"], mutate=mutate)
            want = run()
            for m in UPDATE_MUTATIONS:
                if (m == "drop_slab" and case["S"] == 1) or (m == "l2_new_value" and case["l2"] == 0):
                    continue
                if moved(run(m), want, case["exact"]):
                    caught[m].add(("zero_den " if case["zero_den_column"] is not None else "") + ("exact" if case["exact"] else "random"))
    for m, where in caught.items():
        assert where, f"{m} is not caught at beta {beta}"
        if m in ONLY_ZERO_DEN:
            assert any(w.startswith("zero_den") for w in where), (m, where)
        else:
            assert "random" in where, f"{m}: caught on {where} only"
