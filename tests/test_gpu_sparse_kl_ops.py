"""The launches of the sparse KL path (nmfgpu_amd/csrc/kernels_sparse.hip) one at a time, through op_kl_fused, op_kl_update, op_kl_sums, op_panel_rowsum,
op_spmm_rows and op_sddmm_quotient, against the restatements of tests/sparse_kl_reference.py at (float32, float64) x padded rank (64, 128, 256).

Three kinds of expectation (the cases and their reasons: tests/sparse_kl_cases.py; the bounds: tests/sparse_kl_reference.py; tests/test_sparse_kl_cpu.py checks
both without a device):
  exact       inputs on which every operation is exact: the launch returns the bits of the restatement, so a swapped lane, group, block, part or column, a
              dropped or doubled tail entry or part shows as a different value;
  arithmetic  random data at the engine's eps: every element within a bound that holds for any summation order;
  written     every output starts as NaN: what a launch must write is finite (rows beyond `rows` and padding columns exact zeros), what it must leave alone is
              still NaN, and the NaN rows of the gathered panel, of A beyond `rows` and between the part panels reach no output.
Then the cross-checks: blocked against unblocked, SDDMM + SpMM against the fused gather, and one iteration of the engine against the chain of operations."""
import numpy as np
import pytest

import nmfgpu_amd as na
from tests import sparse_kl_cases as cases
from tests import sparse_kl_reference as ref

pytestmark = pytest.mark.gpu

DTYPES = ["float32", "float64"]
RPS = [64, 128, 256]
WORST = {}      # (operation, dtype) -> worst observed error / bound over the arithmetic cases: a record of headroom, printed when the module is done


@pytest.fixture(scope="module", autouse=True)
def _library_is_native():
    assert na.device_count() >= 1, "GPU tests need a HIP device"
    yield
    for (op, dtype), ratio in sorted(WORST.items()):
        print(f"\nworst error / bound  {op:<22} {dtype}: {ratio:.3f}", end="")
    print()


def within(op, dtype, got, want, bound, what):
    ratio = cases.worst_ratio(got, want, bound)
    WORST[(op, dtype)] = max(WORST.get((op, dtype), 0.0), ratio)
    assert ratio <= 1, f"{op} {what}: worst error / bound {ratio:.3g}"


def run_fused(case, ptr=None, blocks=1, terms=True):
    return na.op_kl_fused(case["ptr"] if ptr is None else ptr, case["idx"], case["val"], case["A"], case["B"], case["rows"], case["rows_pad"], blocks, case["a_scale"], terms)


def check_fused(dtype, what, case, want, got, blocks):
    """One launch of the gather against its restatement, per block panel: bits or bounds, and what was and was not written."""
    rows, rows_pad, RP, r = case["rows"], case["rows_pad"], case["RP"], case["r"]
    u = ref.unit_roundoff(dtype)
    out, tv, tk = got["out"], got["t_vwh"], got["t_kl"]
    assert out.shape == (blocks, rows_pad, RP) and tv.shape == tk.shape == (blocks, rows_pad)
    assert np.all(np.isfinite(out)), f"{what}: NaN reached the output, or part of it was not written"
    assert np.all(out[:, rows:] == 0) and np.all(out[:, :, r:] == 0), what
    assert np.all(np.isfinite(tv[:, :rows])) and np.all(np.isfinite(tk[:, :rows])) and np.all(np.isnan(tv[:, rows:])) and np.all(np.isnan(tk[:, rows:])), what
    if case["exact"]:
        assert cases.same_bits(out, want["out"], dtype), f"{what}: out differs in {np.argwhere(out != want['out'].astype(dtype))[:4].tolist()}"
        assert cases.same_bits(tv[:, :rows], want["t_vwh"], dtype), what
    else:
        n_pad = np.pad(want["n"], ((0, 0), (0, rows_pad - rows)))
        within("kl_fused out", dtype, out, want["out"], ref.fused_out_bound(RP, n_pad, want["out"], u), what)
        within("kl_fused t_vwh", dtype, tv[:, :rows], want["t_vwh"], ref.vwh_bound(RP, want["n"], want["t_vwh"], u), what)
    # (the logarithm is never exact: the divergence terms are held to their bound in both kinds of case)
    within("kl_fused t_kl", dtype, tk[:, :rows], want["t_kl"], ref.kl_term_bound(RP, want["n"], want["kl_x"], want["kl_abs"], u), what)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("RP", RPS)
@pytest.mark.parametrize("kind", ["exact", "random"])
def test_kl_fused_every_rank_and_row_count(kind, RP, dtype):
    for r in cases.RANKS[RP]:
        for rows, rows_pad in cases.ROWS:
            for scaled in (False, True):
                case, _, want = cases.gather_reference(dtype, RP, r, rows, rows_pad, kind, scaled)
                what = f"{kind} r={r} rows={rows} scaled={scaled}"
                got = run_fused(case)
                check_fused(dtype, what, case, want, got, 1)
                # the form without error terms: the same numerators, nothing else touched
                plain = run_fused(case, terms=False)
                assert plain["t_vwh"] is None and plain["t_kl"] is None and np.array_equal(plain["out"], got["out"]), what


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("RP", RPS)
@pytest.mark.parametrize("blocks", cases.BLOCKS)
def test_kl_fused_blocked_matches_per_block_and_adds_up_to_the_unblocked_form(blocks, RP, dtype):
    """2 and 3 blocks run the block-major mapping, 8 and 16 the per-XCD one.  The gathered range is 40 rows: some blocks are empty for every row (their panels are
    written all the same: zeros), some rows have all their entries in one block."""
    ranks = cases.RANKS[RP]
    for kind in ("exact", "random"):
        for r, (rows, rows_pad), scaled in ((ranks[0], (130, 256), False), (ranks[-1], (5, 128), True), (ranks[-1], (127, 128), False)):
            case, bptr, want = cases.gather_reference(dtype, RP, r, rows, rows_pad, kind, scaled, blocks)
            what = f"{kind} blocks={blocks} r={r} rows={rows}"
            check_fused(dtype, what, case, want, run_fused(case, bptr, blocks), blocks)
            whole = ref.kl_fused(case["ptr"], case["idx"], case["val"], case["A"], case["B"], rows, rows_pad, ref.eps_of(np.dtype(dtype)), case["a_scale"], 1,
                                 round_den=np.dtype(dtype) if case["exact"] else None)
            for k in ("out", "t_vwh", "t_kl"):
                assert np.allclose(want[k].sum(axis=0).astype(np.float64), whole[k][0].astype(np.float64), rtol=1e-13, atol=0), (what, k)
            if case["exact"]:
                # ... and the unblocked launch on the same image returns that sum's bits
                assert cases.same_bits(run_fused(case)["out"][0], want["out"].sum(axis=0), dtype), what


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("RP", RPS)
def test_spmm_rows(RP, dtype):
    u = ref.unit_roundoff(dtype)
    for kind in ("exact", "random"):
        for r in cases.RANKS[RP]:
            for rows, rows_pad in cases.ROWS:
                case, want = cases.spmm_case(dtype, RP, r, rows, rows_pad, kind)
                what = f"{kind} r={r} rows={rows}"
                out = na.op_spmm_rows(case["ptr"], case["idx"], case["val"], case["P"], rows, rows_pad)
                assert out.shape == (rows_pad, RP) and np.all(np.isfinite(out)) and np.all(out[rows:] == 0) and np.all(out[:, r:] == 0), what
                if case["exact"]:
                    assert cases.same_bits(out, want["out"], dtype), what
                else:
                    within("spmm_rows", dtype, out, want["out"], ref.spmm_bound(np.pad(want["n"], (0, rows_pad - rows)), want["abs"], u), what)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("RP", RPS)
def test_sddmm_quotient_and_its_two_pass_sequence_against_the_fused_gather(RP, dtype):
    u = ref.unit_roundoff(dtype)
    for kind in ("exact", "random"):
        for r in cases.RANKS[RP]:
            for rows, rows_pad in cases.ROWS:
                case, want = cases.sddmm_reference(dtype, RP, r, rows, rows_pad, kind)
                what = f"{kind} r={r} rows={rows}"
                got = na.op_sddmm_quotient(case["ptr"], case["idx"], case["val"], case["A"], case["B"], rows, terms=True)
                q, tv, tk = got["q"], got["t_vwh"], got["t_kl"]
                assert q.shape == case["val"].shape and np.all(np.isfinite(q)), f"{what}: a quotient was not written"
                assert tv.shape == tk.shape == (rows,) and np.all(np.isfinite(tv)) and np.all(np.isfinite(tk)), what
                if case["exact"]:
                    assert cases.same_bits(q, want["q"], dtype) and cases.same_bits(tv, want["t_vwh"], dtype), what
                else:
                    within("sddmm q", dtype, q, want["q"], ref.quotient_bound(RP, want["q"], u), what)
                    within("sddmm t_vwh", dtype, tv, want["t_vwh"], ref.vwh_bound(RP, want["n"], want["t_vwh"], u), what)
                within("sddmm t_kl", dtype, tk, want["t_kl"], ref.kl_term_bound(RP, want["n"], want["kl_x"], want["kl_abs"], u), what)
                plain = na.op_sddmm_quotient(case["ptr"], case["idx"], case["val"], case["A"], case["B"], rows)
                assert plain["t_vwh"] is None and np.array_equal(plain["q"], q), what
                # the two-pass sequence (quotients, then the SpMM over them) against the fused gather: both within their bounds of the same restatement.
                # Two passes: the quotients' gamma(RP + 4), carried through a sum of nonnegative terms, plus the SpMM's gamma(n + 2) on the rounded quotients
                _, _, fused_want = cases.gather_reference(dtype, RP, r, rows, rows_pad, kind)
                two = na.op_spmm_rows(case["ptr"], case["idx"], q, case["B"], rows, rows_pad)
                fused = run_fused(case, terms=False)["out"][0]
                n_pad = np.pad(want["n"], (0, rows_pad - rows))
                g_q = ref.gamma(RP + 4, u)
                two_bound = (g_q + ref.gamma(n_pad + 2, u) * (1 + g_q))[:, None] * fused_want["out"][0]
                fused_bound = ref.fused_out_bound(RP, n_pad[None], fused_want["out"], u)[0]
                assert cases.worst_ratio(two, fused.astype(ref.WORK), two_bound + fused_bound) <= 1, what
                if case["exact"]:
                    assert np.array_equal(two, fused), what


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("RP", RPS)
@pytest.mark.parametrize("kind", ["exact", "random"])
def test_kl_update_every_part_count(kind, RP, dtype):
    """1 ... 17, 24, 25 and 64 part panels: every size of the tail after the batches of eight, none, one and several whole batches.  The panels lie 16 RP values
    further apart than they are long, with NaN in between."""
    u = ref.unit_roundoff(dtype)
    ranks = cases.RANKS[RP]
    for i, parts in enumerate(cases.UPDATE_PARTS):
        r = ranks[i % len(ranks)]
        for len_pad in (128, 384) if parts in cases.UPDATE_LONG_PARTS else (128,):
            for want_sumsq, with_scale in cases.update_settings(parts):
                case, want = cases.update_case(dtype, RP, r, len_pad, parts, kind, with_scale)
                what = f"{kind} parts={parts} len_pad={len_pad} r={r} sumsq={want_sumsq} scale={with_scale}"
                got = na.op_kl_update(case["P"], case["num"], case["den"], case["scale"], want_sumsq, True, case["stride"], parts=parts)
                P, sm, sq = got["P"], got["sum_part"], got["sumsq_part"]
                assert (sq is not None) == want_sumsq and sm.shape == (len_pad // 128, RP) and (sq is None or sq.shape == sm.shape)
                assert np.all(np.isfinite(P)) and np.all(np.isfinite(sm)) and (sq is None or np.all(np.isfinite(sq))), f"{what}: NaN from between the panels"
                assert np.all(P[:, r:] == 0) and np.all(sm[:, r:] == 0), what
                if case["exact"]:
                    assert cases.same_bits(P, want["P"], dtype), f"{what}: P differs in {np.argwhere(P != want['P'].astype(dtype))[:4].tolist()}"
                    assert cases.same_bits(sm, want["sum_part"], dtype) and (sq is None or cases.same_bits(sq, want["sumsq_part"], dtype)), what
                else:
                    within("kl_update P", dtype, P, want["P"], ref.update_bound(parts, want["P"], u), what)
                    s, s_bound, ss, ss_bound = ref.update_sum_bounds(P, u)      # (against the launch's OWN output rows)
                    within("kl_update sum_part", dtype, sm, s, s_bound, what)
                    if sq is not None:
                        within("kl_update sumsq_part", dtype, sq, ss, ss_bound, what)
    # sums of squares alone (no caller of the engine asks for that, the kernel allows it)
    case, want = cases.update_case(dtype, RP, ranks[0], 128, 3, kind, False)
    got = na.op_kl_update(case["P"], case["num"], case["den"], None, True, False, case["stride"], parts=3)
    assert got["sum_part"] is None and np.all(np.isfinite(got["sumsq_part"]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("RP", RPS)
def test_kl_sums_up_to_1600_parts(RP, dtype):
    """Parts on both sides of 64 (one per thread group) and of 512 (the second trip of the groups' loop, which the engine takes from 65 537 rows on)."""
    u = ref.unit_roundoff(dtype)
    ranks = cases.RANKS[RP]
    for kind in ("exact", "random"):
        for i, parts in enumerate(cases.SUMS_PARTS):
            r = ranks[i % len(ranks)]
            sa, sb, zero_col, with_sq, without = cases.sums_case(dtype, RP, r, parts, kind)
            what = f"{kind} parts={parts} r={r}"
            plain = na.op_kl_sums(sa)
            both = na.op_kl_sums(sa, sb, want_scale=True)
            only_sums = na.op_kl_sums(sa, sb)
            assert plain["scale"] is None and only_sums["scale"] is None and np.array_equal(only_sums["sums"], both["sums"]), what
            for a in (plain["sums"], both["sums"], both["scale"]):
                assert a.shape == (RP,) and np.all(np.isfinite(a)), what
            assert np.all(plain["sums"][r:] == 0) and np.all(both["sums"][r:] == 0) and np.all(both["scale"][r:] == 1), what
            # the guard: a column whose sums of squares are all zero keeps its plain sum, and its scale is 1 exactly
            assert both["sums"][zero_col] == plain["sums"][zero_col] and both["scale"][zero_col] == 1, what
            if kind == "exact":
                assert cases.same_bits(plain["sums"], without["sums"], dtype), what
                assert cases.same_bits(both["sums"], with_sq["sums"], dtype) and cases.same_bits(both["scale"], with_sq["scale"], dtype), what
            else:
                within("kl_sums sums", dtype, plain["sums"], without["sums"], ref.sums_bound(parts, without["sums"], u), what)
                within("kl_sums sums", dtype, both["sums"], with_sq["sums"], ref.sums_bound(parts, with_sq["sums"], u), what)
                within("kl_sums scale", dtype, both["scale"], with_sq["scale"], ref.sums_bound(parts, with_sq["scale"], u), what)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("RP", RPS)
def test_panel_rowsum(RP, dtype):
    u = ref.unit_roundoff(dtype)
    for kind in ("exact", "random"):
        for r in cases.RANKS[RP]:
            for len_pad in cases.ROWSUM_LEN_PADS:
                P, want = cases.rowsum_case(dtype, RP, r, len_pad, kind)
                sums = na.op_panel_rowsum(P)
                assert sums.shape == (RP,) and np.all(np.isfinite(sums)) and np.all(sums[r:] == 0)
                if kind == "exact":
                    assert cases.same_bits(sums, want["sums"], dtype), (kind, r, len_pad)
                else:
                    within("panel_rowsum", dtype, sums, want["sums"], ref.rowsum_bound(len_pad, want["abs"], u), f"r={r} len_pad={len_pad}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_padded_rank_192_is_refused(dtype):
    """k_kl_update's thread mapping needs RP / 4 to divide 256, and the gathers are instantiated for 64, 128 and 256: the launchers refuse 192 instead of running
    something else.  (The engine never asks: its padded ranks are 64, 128, 256, 384.)"""
    dt = np.dtype(dtype)
    ptr, idx, val = np.array([0, 2], np.int32), np.array([0, 1], np.int32), np.ones(2, dt)
    for RP, refused in ((192, True), (64, False), (128, False), (256, False)):
        A, B, P = np.ones((128, RP), dt), np.ones((4, RP), dt), np.ones((128, RP), dt)
        calls = (lambda: na.op_kl_update(P, np.ones((1, 128, RP), dt), np.ones(RP, dt), None, True, True),
                 lambda: na.op_kl_fused(ptr, idx, val, A, B, 1, 128),
                 lambda: na.op_spmm_rows(ptr, idx, val, B, 1, 128),
                 lambda: na.op_sddmm_quotient(ptr, idx, val, A, B, 1))
        for call in calls:
            if refused:
                with pytest.raises(na.EngineError) as e:
                    call()
                assert e.value.status == 1
            else:
                call()


# ---------------------------------------------------------------------------------------------------------------- the engine launches what the entries launch

def _tie_problem():
    m, n, r = 150, 130, 20
    rng = np.random.default_rng(29)
    V = (rng.integers(1, 6, (m, n)) * (rng.random((m, n)) < 0.15)).astype(np.float32)
    W0 = np.asfortranarray((1.0 - rng.random((m, r))).astype(np.float32))
    H0 = np.asfortranarray((1.0 - rng.random((r, n))).astype(np.float32))
    return m, n, r, V, W0, H0


def _image(V):
    """(ptr, idx, val) of the rows of the dense V: its nonzeros in ascending column order."""
    stored = V != 0
    ptr = np.concatenate([[0], np.cumsum(stored.sum(axis=1))]).astype(np.int32)
    return ptr, np.nonzero(stored)[1].astype(np.int32), V[stored].astype(np.float32)


def _engine_iteration(V, W0, H0, error):
    m, r = W0.shape
    n = H0.shape[1]
    eng = na.Engine(m, n, r, "mu", divergence="kl")
    try:
        ptr, idx, val = _image(V)
        eng.upload_sparse(1, val, ptr, idx, 0)
        eng.set_factors(W0, H0)
        eng.iterate(1, first_iteration=1, error_every=1 if error else 0, last_iteration=1)
        W, H = eng.get_factors()
        return W, H, (eng.kl_divergence if error else None), eng.geometry()
    finally:
        eng.close()


def test_one_engine_iteration_is_the_chain_of_operations():
    """One KL iteration from set_factors on a 150 x 130 problem at rank 20 (float32) against the same launches through the operation entries, so that the entries
    cannot drift from what the engine launches:
      H: op_panel_rowsum(Wt) -> op_kl_fused over the CSC image (A = H, B = Wt) -> op_kl_update: the engine's H, bit for bit;
      W: op_kl_sums of that update's partial sums (the denominators) -> op_kl_fused over the CSR image (A = Wt, B = the new H) -> op_kl_update -> the column
         normalisation.  Engine::materialize_w is not one multiply per element: launch_normalize_panel adds the partial sums of squares up again, takes the square
         root in T and DIVIDES by it.  So the expectation restates that (v / sqrt(sum) in float32) and holds the engine to 2u relative of it; the sum of the two
         partials here has one order only, so a device square root and division that round correctly make it bit for bit -- the test prints which it was."""
    m, n, r, V, W0, H0 = _tie_problem()
    W, H, _, geo = _engine_iteration(V, W0, H0, False)
    RP, mpad, npad = geo["padded_rank"], geo["padded_m"], geo["padded_n"]
    assert (RP, mpad, npad) == (64, 256, 256) and geo["kl_blocks_w"] == geo["kl_blocks_h"] == 1
    Wt = np.zeros((mpad, RP), np.float32); Wt[:m, :r] = W0
    Hp = np.zeros((npad, RP), np.float32); Hp[:n, :r] = H0.T
    sW = na.op_panel_rowsum(Wt)
    num = na.op_kl_fused(*_image(np.ascontiguousarray(V.T)), Hp, Wt, n, npad)["out"]
    h = na.op_kl_update(Hp, num, sW, None, False, True)
    assert np.array_equal(H, h["P"][:n, :r].T), "H of the engine differs from the chain of operations"
    sH = na.op_kl_sums(h["sum_part"])["sums"]
    num = na.op_kl_fused(*_image(V), Wt, h["P"], m, mpad)["out"]
    w = na.op_kl_update(Wt, num, sH, None, True, True)
    sumsq = w["sumsq_part"].sum(axis=0, dtype=np.float32)                  # (two partials: one order)
    norm = np.sqrt(sumsq)
    want = (w["P"] / np.where(norm > 0, norm, np.float32(1)))[:m, :r]
    assert want.dtype == np.float32
    u = ref.unit_roundoff(np.float32)
    assert np.all(np.abs(W.astype(np.float64) - want) <= 2 * u * np.abs(want)), "W of the engine is further than 2u from the chain of operations"
    print(f"\nengine tie: W {'bit for bit' if np.array_equal(W, want) else 'within 2u, not bit for bit'}; H bit for bit")
    # the pending scale the engine keeps for its next iteration is what op_kl_sums makes of the same partials: 1 / norm within 2u
    scale = na.op_kl_sums(w["sum_part"], w["sumsq_part"], want_scale=True)["scale"]
    assert np.all(np.abs(scale[:r].astype(np.float64) * norm[:r] - 1) <= 2 * u)


def test_two_pass_sequence_agrees_with_the_fused_one(monkeypatch, diag_build):
    """NMFAMD_KL_TWO_PASS (measurement build): SDDMM, the permutation of the quotients into the CSC order (k_permute) and an SpMM per half-step instead of the
    fused gather -- the same arithmetic in another grouping of a row's entries, so the factors of one iteration agree to float32 rounding (the 1e-6 of
    test_kl_blocked_gather_equals_unblocked is 2e-6 there; one iteration here)."""
    m, n, r, V, W0, H0 = _tie_problem()
    monkeypatch.delenv("NMFAMD_KL_TWO_PASS", raising=False)
    Wf, Hf, klf, _ = _engine_iteration(V, W0, H0, True)
    monkeypatch.setenv("NMFAMD_KL_TWO_PASS", "1")
    Wt, Ht, klt, _ = _engine_iteration(V, W0, H0, True)
    rel = lambda a, b: np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b.astype(np.float64))
    assert rel(Wt, Wf) < 1e-6 and rel(Ht, Hf) < 1e-6, (rel(Wt, Wf), rel(Ht, Hf))
    # (another grouping of 2 900 entries' terms does not return the fused sequence's bits: if it does, the switch was not read and k_permute did not run)
    assert not (np.array_equal(Wt, Wf) and np.array_equal(Ht, Hf)), "NMFAMD_KL_TWO_PASS changed nothing"
    assert klt == pytest.approx(klf, rel=1e-5)
