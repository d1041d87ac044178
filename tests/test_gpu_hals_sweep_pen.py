"""The penalised HALS sweep (kernels_hals.hip, k_sweep_hals<T, RP, true>) as an operation, at every instantiated (dtype, RP), through
nmfamd_op_hals_sweep_pen_* against the fp64 sweep of tests/hals_penalty_reference.py.

As tests/test_gpu_hals_sweep.py, no expectation assumes the kernel's lane mapping or summation order:
  exact: integer problems with integer l1, l2 where every G[k,k] + l2 is a power of two and every intermediate fits 24 bits, so the new panel, ps
         and the partial sums of squares must match the fp64 sweep bit for bit;
  arithmetic: a diagonally dominant G with fractional penalties inside hals_reference.sweep_bound of the equivalent unpenalised problem;
  padding / equivalence: garbage in the padding changes nothing, and l1 = l2 = 0 through the new entry is the old entry bit for bit.
"""
import numpy as np
import pytest

import nmfgpu_amd as na
from tests import hals_penalty_reference as pen
from tests import hals_reference as ref
from tests.test_gpu_hals_sweep import CASES, LEN_PAD, UNIT, cols_and_chunk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _library_is_native():
    assert na.device_count() >= 1, "GPU tests need a HIP device"


def launch(P, slabs, G, r, len_valid, penalties, gap=True):
    """The kernel on a case (penalties = None: the unpenalised entry); the gaps between the slabs hold NaN, ps and sumsq_part start as NaN."""
    S, len_pad, RP = slabs.shape
    stride = len_pad * RP + (16 * RP if gap and S > 1 else 0)
    flat = np.full((S, stride), np.nan, dtype=P.dtype)
    flat[:, :len_pad * RP] = slabs.reshape(S, -1)
    out = na.op_hals_sweep(P, flat, G, r, len_valid, ps=np.full(len_pad, np.nan, P.dtype),
                           sumsq_part=np.full((len_pad // 16) * RP, np.nan, P.dtype), penalties=penalties)
    assert out["parts"] == len_pad // cols_and_chunk(P.dtype.type, RP)[0]
    return out


def assert_padding_is_zero(out, r, len_valid):
    P = out["P"]
    assert (P[:, r:] == 0).all() and (P[len_valid:, :] == 0).all()
    assert not np.isnan(out["ps"][:len_valid]).any() and np.isnan(out["ps"][len_valid:]).all()
    assert not np.isnan(out["sumsq_part"]).any()


def assert_exact(out, P, slabs, G, r, len_valid, l1, l2):
    """Panel, ps (from the raw a) and the column sums of squares equal the fp64 sweep's exactly."""
    want = pen.panel_sweep(P, slabs, G, r, len_valid, l1, l2)
    got = out["P"][:len_valid, :r].astype(np.float64)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} elements differ, first (y, k) = {bad[:4].tolist()}"
    a = slabs.astype(np.float64).sum(axis=0)[:len_valid, :r]
    assert np.array_equal(out["ps"][:len_valid].astype(np.float64), (want * a).sum(axis=1)), "ps is not sum_k p_new(k) a(k) with the raw a"
    colsq = np.zeros(P.shape[1])
    colsq[:r] = (want * want).sum(axis=0)
    assert np.array_equal(out["sumsq_part"].astype(np.float64).sum(axis=0), colsq)
    assert_padding_is_zero(out, r, len_valid)
    return want


def diagonal_case(RP, r, len_pad, len_valid, S, rng, dtype, diag_values):
    """G diagonal with entries from diag_values, a integers in [-32, 32] split exactly over the slabs, old p integers in [0, 8).  With d = G_kk + l2
    a power of two <= 8 the new entry is max(0, (a - l1) / d): at most 3 fraction bits, |p a| <= 2^10 (ps < 2^19), p^2 <= 2^10 with 6 fraction bits
    (a column's sum over 256 rows < 2^18): everything exact in fp32."""
    G = np.zeros((RP, RP))
    k = np.arange(r)
    G[k, k] = np.asarray(diag_values, dtype=np.float64)[(k * 5 + k // 7) % len(diag_values)]
    A = np.zeros((len_pad, RP))
    A[:len_valid, :r] = rng.integers(-32, 33, size=(len_valid, r))
    P = np.zeros((len_pad, RP))
    P[:len_valid, :r] = rng.integers(0, 8, size=(len_valid, r))
    return P.astype(dtype), ref._split(A, S, rng, 8).astype(dtype), G.astype(dtype)


def pairs_case(RP, r, len_pad, len_valid, S, rng, dtype):
    """G with diagonal 0 / 1 and coordinates 2j, 2j + 1 coupled by G = 1 at random; a, old p integers in [0, 16].  With l2 = 1 (d = 1 or 2):
    p(2j) <- max(0, (a - l1 - p_old(2j+1)) / d), p(2j+1) <- max(0, (a - l1 - p_new(2j)) / d): the Gauss-Seidel order shows, at most 2 fraction bits,
    p <= 16: ps < 2^17 and the sums of squares < 2^16 with 4 fraction bits, exact in fp32."""
    G = np.zeros((RP, RP))
    k = np.arange(r)
    G[k, k] = rng.integers(0, 2, size=r)
    j = np.arange(0, r - 1, 2)
    off = rng.integers(0, 2, size=len(j)).astype(np.float64)
    G[j, j + 1] = off
    G[j + 1, j] = off
    A = np.zeros((len_pad, RP))
    A[:len_valid, :r] = rng.integers(0, 17, size=(len_valid, r))
    P = np.zeros((len_pad, RP))
    P[:len_valid, :r] = rng.integers(0, 17, size=(len_valid, r))
    return P.astype(dtype), ref._split(A, S, rng, 8).astype(dtype), G.astype(dtype)


@pytest.mark.parametrize("dtype,RP,r,len_valid,S", CASES)
def test_diagonal_is_exact_and_zero_diagonal_is_updated(dtype, RP, r, len_valid, S):
    """l1 = 3, l2 = 1 and G_kk in {0, 1, 3, 7}: d = 1, 2, 4, 8.  A coordinate with G_kk = 0 is updated (d = l2 > 0)."""
    rng = np.random.default_rng(RP * 1000 + r + 10)
    P, slabs, G = diagonal_case(RP, r, LEN_PAD, len_valid, S, rng, dtype, (0, 1, 3, 7))
    out = launch(P, slabs, G, r, len_valid, (3.0, 1.0))
    want = assert_exact(out, P, slabs, G, r, len_valid, 3.0, 1.0)
    k = np.arange(r)
    a = slabs.astype(np.float64).sum(axis=0)[:len_valid, :r]
    assert np.array_equal(want, np.maximum(0.0, (a - 3.0) / (G[k, k].astype(np.float64) + 1.0)))      # (the restatement itself: closed form)
    zero = G[k, k] == 0
    assert zero[0] and (out["P"][:len_valid, :r][:, zero] == np.maximum(0.0, a[:, zero] - 3.0)).all()


@pytest.mark.parametrize("dtype,RP,r,len_valid,S", CASES)
def test_zero_diagonal_without_l2_is_skipped(dtype, RP, r, len_valid, S):
    """l1 = 2, l2 = 0 and G_kk in {0, 1, 2, 4, 8}: a coordinate with G_kk = 0 keeps its old value, the others move by the L1 term."""
    rng = np.random.default_rng(RP * 1000 + r + 11)
    P, slabs, G = diagonal_case(RP, r, LEN_PAD, len_valid, S, rng, dtype, (0, 1, 2, 4, 8))
    out = launch(P, slabs, G, r, len_valid, (2.0, 0.0))
    assert_exact(out, P, slabs, G, r, len_valid, 2.0, 0.0)
    zero = G[np.arange(r), np.arange(r)] == 0
    assert zero[0] and np.array_equal(out["P"][:len_valid, :r][:, zero], P[:len_valid, :r][:, zero])


@pytest.mark.parametrize("dtype,RP,r,len_valid,S", CASES)
def test_order_is_exact(dtype, RP, r, len_valid, S):
    rng = np.random.default_rng(RP * 1000 + r + 12)
    P, slabs, G = pairs_case(RP, r, LEN_PAD, len_valid, S, rng, dtype)
    out = launch(P, slabs, G, r, len_valid, (2.0, 1.0))
    assert_exact(out, P, slabs, G, r, len_valid, 2.0, 1.0)


@pytest.mark.parametrize("dtype,RP,r,len_valid,S", CASES)
def test_arithmetic_within_running_error_bound(dtype, RP, r, len_valid, S):
    """Diagonally dominant G, l1 = 0.375, l2 = 0.625.  The penalised sweep is the plain sweep of G + l2 I against a - l1, so sweep_bound of that
    problem applies, with -l1 as one more slab and three empty ones for the roundings the plain sweep does not have (l2 p(k): a product and a sum;
    G_kk + l2): its gamma index grows by four.  Padding garbage changes nothing and comes out as zeros."""
    u = UNIT[dtype]
    l1, l2 = 0.375, 0.625
    rng = np.random.default_rng(RP * 1000 + r + 13)
    P, slabs, G = ref.dominant_case(RP, r, LEN_PAD, len_valid, S, rng, dtype)
    out = launch(P, slabs, G, r, len_valid, (l1, l2))
    want = pen.panel_sweep(P, slabs, G, r, len_valid, l1, l2)
    extra = np.zeros((4,) + slabs.shape[1:])
    extra[0, :len_valid, :r] = -l1
    slabs_eq = np.concatenate([slabs.astype(np.float64), extra])
    G_eq = G.astype(np.float64) + l2 * np.eye(RP)
    assert np.allclose(ref.panel_sweep(P, slabs_eq, G_eq, r, len_valid), want, rtol=1e-12, atol=1e-13)
    b = ref.sweep_bound(P[:len_valid].T, slabs_eq[:, :len_valid].transpose(0, 2, 1), G_eq, r, u).T
    got = out["P"][:len_valid, :r].astype(np.float64)
    err = np.abs(got - want)
    assert (err <= b).all(), f"worst error / bound {(err / np.maximum(b, 1e-300)).max():.3g} at {np.unravel_index(np.argmax(err - b), err.shape)}"
    a = slabs.astype(np.float64).sum(axis=0)[:len_valid, :r]
    ps_tol = ref.gamma(RP + S, u) * np.abs(want * a).sum(axis=1) + (b * np.abs(a)).sum(axis=1)
    assert (np.abs(out["ps"][:len_valid] - (want * a).sum(axis=1)) <= ps_tol).all()
    assert_padding_is_zero(out, r, len_valid)
    dirty = launch(*ref.with_garbage(P, slabs, G, r, len_valid, rng), r, len_valid, (l1, l2))
    assert np.array_equal(dirty["P"], out["P"]) and (dirty["P"][:, r:] == 0).all() and (dirty["P"][len_valid:, :] == 0).all()
    assert np.array_equal(dirty["ps"][:len_valid], out["ps"][:len_valid]) and np.isnan(dirty["ps"][len_valid:]).all()
    assert np.array_equal(dirty["sumsq_part"], out["sumsq_part"])


@pytest.mark.parametrize("dtype,RP,r,len_valid,S", CASES)
def test_zero_penalties_are_the_old_entry(dtype, RP, r, len_valid, S):
    rng = np.random.default_rng(RP * 1000 + r + 14)
    P, slabs, G = ref.with_garbage(*ref.dominant_case(RP, r, LEN_PAD, len_valid, S, rng, dtype), r, len_valid, rng)
    old = launch(P, slabs, G, r, len_valid, None)
    new = launch(P, slabs, G, r, len_valid, (0.0, 0.0))
    assert np.array_equal(new["P"], old["P"]) and np.array_equal(new["sumsq_part"], old["sumsq_part"])
    assert np.array_equal(new["ps"][:len_valid], old["ps"][:len_valid]) and np.isnan(new["ps"][len_valid:]).all()
    assert_padding_is_zero(new, r, len_valid)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_bad_penalties_are_refused(dtype):
    P = np.zeros((128, 64), dtype)
    G = np.eye(64, dtype=dtype)
    for p in ((-1.0, 0.0), (0.0, -0.5), (float("nan"), 0.0), (0.0, float("inf"))):
        with pytest.raises(na.EngineError) as info:
            na.op_hals_sweep(P, np.zeros((1, 128 * 64), dtype), G, 1, 128, penalties=p)
        assert info.value.status == 1, p
