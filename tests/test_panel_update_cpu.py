"""Device-free checks of what the panel-update GPU tests rely on (tests/panel_update_reference.py, tests/panel_update_cases.py):
  1. the restatement, chained into one multiplicative-update and one nsNMF iteration, reproduces the project's independent oracle;
  2. the "exact" cases are exact in float32 and in the three-plane bf16 split;
  3. every deliberate defect of panel_update_reference.MUTATIONS, applied to the restatement, leaves the test's bound in at least one element of the inputs the GPU
     tests use -- the condition that keeps the bounds from being loose enough to hide such a defect."""
import numpy as np
import pytest

from oracle import oracle
from tests import panel_update_cases as cases
from tests import panel_update_reference as ref

U32, U64 = ref.unit_roundoff("float32"), ref.unit_roundoff("float64")


def _two_slabs(A, B):
    """A^T B (one panel row per column of A) cut into two K slices, as a split-K product leaves it."""
    h = A.shape[0] // 2
    return np.stack([(A[:h].T @ B[:h]).reshape(-1), (A[h:].T @ B[h:]).reshape(-1)])


def _normalise(W, sumsq_part):
    s = sumsq_part.sum(axis=0)
    return W / np.where(s > 0, np.sqrt(s), 1.0)[None, :]


@pytest.mark.parametrize("algorithm,theta", [("mu", 0.0), ("nsnmf", 0.4)])
def test_restatement_chained_into_one_iteration_matches_the_oracle(algorithm, theta):
    rng = np.random.default_rng(5)
    m, n, r = 48, 64, 6
    V = np.asfortranarray(rng.random((m, n)))
    W = np.asfortranarray(0.1 + rng.random((m, r)))
    H = np.asfortranarray(0.1 + rng.random((r, n)))
    Wo, Ho = W.copy(order="F"), H.copy(order="F")
    oracle.run(algorithm, V, Wo, Ho, 1, theta=theta)
    eps = ref.eps_of("float64")
    S = (1 - theta) * np.eye(r) + theta / r * np.ones((r, r))
    Ws = W @ S
    # H step: the panel is H^T (one row per column of H), the numerator W^T V in two K slices, Q = W^T W
    h = ref.panel_update("mu", H.T, _two_slabs(V, Ws), Ws.T @ Ws, n, eps, n, U64)
    Hn = h["new"].T
    Hs = S @ Hn
    # W step: the panel is W, the numerator V (S H)^T, Q = (S H)(S H)^T; then the column normalisation from the partial sums of squares
    w = ref.panel_update("mu", W, _two_slabs(V.T, Hs.T), Hs @ Hs.T, m, eps, m // 2, U64)
    Wn = _normalise(w["new"], w["sumsq_part"])
    got_w = Wn @ S       # (the oracle hands back W S for nsNMF; S = I otherwise)
    assert np.max(np.abs(Hn - Ho) / np.abs(Ho)) <= 1e-12
    assert np.max(np.abs(got_w - Wo) / np.abs(Wo)) <= 1e-12
    # ps(y) = sum_c new num is the per-column term of tr(H^T W^T V)
    assert np.allclose(h["ps"], np.einsum("cy,cy->y", Hn, Ws.T @ V), rtol=1e-12, atol=0)


def test_rank64_restatement_with_pending_scale_and_smoothing_matches_the_oracle():
    """The same H step through mu64_update: W kept unnormalised with its pending scale, the smoothing applied around the r x r product, the K-split operand."""
    rng = np.random.default_rng(6)
    m, n, r, theta = 48, 64, 6, 0.4
    V = np.asfortranarray(rng.random((m, n)))
    Wu = 0.1 + rng.random((m, r))
    d = 1 / np.sqrt((Wu ** 2).sum(axis=0))
    W = np.asfortranarray(Wu * d)
    H = np.asfortranarray(0.1 + rng.random((r, n)))
    Wo, Ho = W.copy(order="F"), H.copy(order="F")
    oracle.run("nsnmf", V, Wo, Ho, 1, theta=theta, const_w=True)
    pad = lambda a: np.pad(a, ((0, 0), (0, 64 - r)))
    scale = np.ones(64); scale[:r] = d
    G = np.zeros((2, 64, 64))
    G[0, :r, :r] = Wu[:20].T @ Wu[:20]; G[1, :r, :r] = Wu[20:].T @ Wu[20:]
    slabs = np.stack([pad((Wu[:20].T @ V[:20]).T).reshape(-1), pad((Wu[20:].T @ V[20:]).T).reshape(-1)])
    got = ref.mu64_update(0, pad(H.T), slabs, G, scale, n, ref.eps_of("float64"), U64, qsplit=2, ns=(theta / r, (1 - theta) + theta / r, r))
    assert np.max(np.abs(got["new"][:, :r].T - Ho) / np.abs(Ho)) <= 1e-12
    assert np.all(got["new"][:, r:] == 0)
    S = (1 - theta) * np.eye(r) + theta / r * np.ones((r, r))
    assert np.allclose(got["image"][:, :r].T, S @ Ho, rtol=1e-12, atol=0)
    assert np.allclose(got["q_out"][:r, :r], W.T @ W, rtol=1e-12, atol=0)


EXACT_SHAPES = [(64, 64, 128, 128, 9), (64, 33, 384, 383, 15), (128, 128, 128, 77, 9), (192, 192, 128, 127, 2), (256, 200, 384, 383, 12), (384, 384, 128, 1, 8),
                (512, 512, 128, 128, 15)]


@pytest.mark.parametrize("mode", ["mu", "ls", "set"])
@pytest.mark.parametrize("RP,r,len_pad,len_valid,S", EXACT_SHAPES)
def test_exact_cases_are_exact_in_float32_and_in_one_bf16_plane(RP, r, len_pad, len_valid, S, mode):
    for symmetric in (False, True):
        case = cases.exact_case(mode, RP, r, len_pad, len_valid, S, np.float32, symmetric=symmetric)
        rep = cases.exactness_report(case, mode)
        assert rep["integers"] and rep["largest"] < 2 ** 24 and rep["one_plane"], rep
        Q = case["Q"]
        assert np.array_equal(Q, Q.T) == symmetric
        # the entries change with every step along a row and a column
        assert np.all(Q[:r, 1:r] != Q[:r, :r - 1]) and np.all(Q[1:r, :r] != Q[:r - 1, :r])
        assert np.all(np.isnan(case["slabs"][:, len_pad * RP:])) and case["slabs"].shape == (S, len_pad * RP + cases.GAP)
        assert np.all(case["P"][len_valid:] == 0) and np.all(case["P"][:, r:] == 0)


def test_split_of_an_exact_case_decodes_to_itself():
    """hi + mid + lo, each a bf16 rounding of the residual: the three planes the kernels write add up to the float32 value (nmfgpu_amd/csrc/split3.h)."""
    rng = np.random.default_rng(2)
    x = np.concatenate([rng.random(1000).astype(np.float32) * 300, np.arange(280, dtype=np.float32)])
    hi = cases.to_bf16(x); mid = cases.to_bf16(x - hi); lo = cases.to_bf16(x - hi - mid)
    assert np.array_equal((lo + mid) + hi, x)
    assert np.array_equal(cases.to_bf16(np.arange(32, dtype=np.float32)), np.arange(32, dtype=np.float32))


def _violates(got, want, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        return cases.worst_ratio(got, want, bound) > 1


PANEL_MUTATIONS = ["drop_slab", "drop_k_term", "transpose_q", "no_eps", "len_valid_off_by_one"]


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("mode", ["mu", "ls"])
@pytest.mark.parametrize("mutation", PANEL_MUTATIONS)
def test_every_defect_of_the_panel_update_leaves_the_bounds(mutation, mode, kind):
    """On the shapes and ranks the GPU module runs (cases.SHAPES at the smallest and the largest padded rank), in each mode by itself, against the loosest bound of
    the module there (float32, split operands).  What each defect is shown on:
      dropped slab, dropped K-term, Q transposed   the new rows, on every shape with more than one valid row;
      off-by-one len_valid                         the split image of the rank-64 form, whose rows from len_valid on are zero (ps is shorter by construction of
                                                   the defect: that is no test of a bound and is not counted);
      eps left out                                 MODE_MU only, and only on cases.tiny_row() of the shape: wherever the denominator is of the size of the data,
                                                   eps is below the rounding of the quotient and no bound can see it.  The GPU modules launch that row
                                                   (test_eps_decides_where_the_denominator_vanishes, test_eps_on_a_vanishing_denominator)."""
    if mutation == "no_eps" and mode == "ls":
        return      # (MODE_LS has no eps)
    eps = ref.eps_of("float32")
    for RP in (64, 512):
        r = cases.RANKS[RP]
        for len_pad, len_valid, S in cases.SHAPES[1:]:
            if len_valid == 1 and mutation in ("drop_k_term", "transpose_q", "len_valid_off_by_one"):
                continue      # (one valid row: it need not meet the dropped K-term; nothing is left of it with one row less)
            case = cases.make_case(kind, mode, RP, r, len_pad, len_valid, S, np.float32)
            if mutation == "no_eps":
                case = cases.tiny_row(case)
            args = (mode, case["P"], case["slabs"], case["Q"], len_valid, eps, 32, U32)
            want = ref.panel_update(*args, split_q=True)
            with np.errstate(invalid="ignore", divide="ignore"):
                bad = ref.panel_update(*args, split_q=True, mutate=mutation)
            # (MODE_MU on exact inputs: two roundings, den + eps and the division; everything else must match to the bit)
            b_new = (ref.gamma(2, U32) * want["new"] if mode == "mu" else 0 * want["new"]) if kind == "exact" else want["b_new"]
            got, ok = (bad["image"], want["image"]) if mutation == "len_valid_off_by_one" else (bad["new"], want["new"])
            assert _violates(got, ok, b_new), (mutation, mode, kind, RP, len_pad, len_valid, S)


@pytest.mark.parametrize("qsplit", [0, 2, 4, 8])
@pytest.mark.parametrize("r", [1, 33, 64])
def test_scaled_exact_cases_are_exact(r, qsplit):
    """What the rank-64 and fused exact cases add to the plain ones -- power-of-two scales, integer slices of Q, the integer trace operand -- keeps every product
    and partial sum exact in float32 and every operand of the r x r product in one bf16 plane, so that gamma(2) on the new rows and bit equality of q_out and of
    the W side's trace terms are fair to ask.  (In MODE_MU ps, sumsq_part, gram_partial and colsq_part are sums of rounded quotients: they are held to their
    bounds, never to bits.)"""
    for len_pad, len_valid, S in ((128, 77, 2), (384, 383, 28)):
        case = cases.exact_case("mu", 64, r, len_pad, len_valid, S, np.float32, symmetric=True)
        rep = cases.scaled_exactness_report(case, cases.scale_vector("exact", r, np.float32), cases.slices_of(case["Q"], qsplit, "exact"), cases.gprev_of("exact", r))
        assert rep["quarters"] and rep["largest"] < 2 ** 24 and rep["powers_of_two"] and rep["symmetric_slices"] and rep["one_plane"], rep
    for RP in (128, 512):
        case = cases.exact_case("mu", RP, cases.RANKS[RP], 384, 200, 18, np.float32)
        rep = cases.scaled_exactness_report(case, cases.scale_vector("exact", RP, np.float32), case["Q"], None)
        assert rep["quarters"] and rep["largest"] < 2 ** 24 and rep["powers_of_two"] and rep["one_plane"], rep


@pytest.mark.parametrize("mutation", ["drop_slab", "drop_k_term", "no_eps", "scale_wrong_side", "len_valid_off_by_one"])
@pytest.mark.parametrize("form", ["h", "w", "h_qsplit8", "h_ns"])
def test_every_defect_of_the_rank64_update_leaves_the_bounds(form, mutation):
    """The loosest rank-64 bound: 15 slabs, eight K slices, smoothing around the product."""
    is_w = form == "w"
    r, len_pad, len_valid, S = 33, 128, 77, 15
    qsplit = 8 if form in ("h_qsplit8", "h_ns") else 0
    ns = (0.5 / r, 0.5 + 0.5 / r, r) if form == "h_ns" else None
    case = cases.random_case("mu", 64, r, len_pad, len_valid, S, np.float32, 3, symmetric=True)
    Q = case["Q"] if not qsplit else np.stack([case["Q"] / qsplit] * qsplit).astype(np.float32)
    scale = cases.scale_vector("random", r, np.float32)
    P = case["P"].copy()
    if mutation == "no_eps":
        P[0, :r] = 1e-30
    eps = ref.eps_of("float32")
    want = ref.mu64_update(is_w, P, case["slabs"], Q, scale, len_valid, eps, U32, qsplit=qsplit, ns=ns)
    with np.errstate(invalid="ignore", divide="ignore"):
        bad = ref.mu64_update(is_w, P, case["slabs"], Q, scale, len_valid, eps, U32, qsplit=qsplit, ns=ns, mutate=mutation)
    if mutation == "len_valid_off_by_one":
        assert _violates(bad["image"], want["image"], want["b_image"]) and (is_w or len(bad["ps"]) != len(want["ps"]))
    else:
        assert _violates(bad["new"], want["new"], want["b_new"]), (form, mutation, want["depth"])


# (Q read transposed: on the W side only -- the H side's operand is the Gram matrix of the panel, symmetric by construction)
FUSED_DEFECTS = [(side, mutation) for side in ("w", "h", "h_smooth") for mutation in ("drop_slab", "drop_k_term", "transpose_q", "no_eps", "scale_wrong_side")
                 if not (mutation == "transpose_q" and side != "w")]


@pytest.mark.parametrize("side,mutation", FUSED_DEFECTS)
def test_every_defect_of_the_fused_update_leaves_the_bounds(side, mutation):
    RP, r, len_pad, len_valid, S = 512, 300, 128, 77, 15
    case = cases.random_case("mu", RP, r, len_pad, len_valid, S, np.float32, 4)
    sc = cases.scale_vector("random", RP, np.float32)
    P = case["P"].copy()
    if mutation == "no_eps":
        P[0, :r] = 1e-30
    kw = {"old_scale": sc} if side == "w" else {"h_side": True, "scale": sc, "smooth": side == "h_smooth", "off": 0.5 / r, "diag": 0.5 + 0.5 / r, "r": r}
    eps = ref.eps_of("float32")
    want = ref.fused_update(P, case["slabs"], case["Q"], len_valid, eps, 32, U32, split_q=True, **kw)
    with np.errstate(invalid="ignore", divide="ignore"):
        bad = ref.fused_update(P, case["slabs"], case["Q"], len_valid, eps, 32, U32, split_q=True, mutate=mutation, **kw)
    assert _violates(bad["new"], want["new"], want["b_new"]), (side, mutation, want["depth"])
