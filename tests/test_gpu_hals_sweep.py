"""The HALS sweep (kernels_hals.hip) as an operation, at every instantiated (dtype, RP), against the fp64 sweep of tests/hals_reference.py.

One launch per check through nmfamd_op_hals_sweep_* on caller-built padded arrays.  Three kinds of expectation, none of which assumes the
kernel's lane mapping or summation order:
  layout / order: problems where every operation is exact (integers, powers of two), so the kernel must match the fp64 sweep bit for bit;
  arithmetic: a diagonally dominant G, where every element must lie within sweep_bound, a running-error bound valid for any order;
  padding: garbage in every padding entry changes nothing, and the padding comes out as exact zeros.
"""
import numpy as np
import pytest

import nmfgpu_amd as na
from tests import hals_reference as ref

pytestmark = pytest.mark.gpu

LEN_PAD = 256
INSTANTIATIONS = {np.float32: [64, 128, 256, 384, 512], np.float64: [64, 128, 192, 256, 320, 384, 448, 512]}
UNIT = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}


def cols_and_chunk(dtype, RP):
    """(columns per workgroup, rows of G per LDS chunk) of k_sweep_hals<T, RP> (HalsGeom): only to choose r and len_valid at the edges."""
    L = 4 if RP <= 64 else 8 if RP <= 128 else 16 if RP <= 256 else 32
    C = 1 if RP <= 128 else 2
    KC = min(65536 // (RP * np.dtype(dtype).itemsize), RP)
    return (256 // L) * C, KC


def _cases():
    out = []
    for dtype, rps in INSTANTIATIONS.items():
        prev = 0
        for RP in rps:
            cols, kc = cols_and_chunk(dtype, RP)
            rs = [prev + 1, RP - 1, RP]
            m = next((q for q in range(kc, RP, kc) if q >= prev + 2 and q + 1 < RP - 1), None)
            if m is not None:
                rs += [m, m + 1]
            lvs = [1, cols - 1, cols + 1, LEN_PAD - 1]
            for r in sorted(set(rs)):
                i = len(out)                         # (len_valid and S rotate over all the cases, not per instantiation)
                lv, S = lvs[i % 4], (1, 3)[(i // 4) % 2]
                out.append(pytest.param(dtype, RP, r, lv, S, id=f"{np.dtype(dtype).name}-RP{RP}-r{r}-len{lv}-S{S}"))
            prev = RP
    return out


CASES = _cases()


@pytest.fixture(scope="module", autouse=True)
def _library_is_native():
    assert na.device_count() >= 1, "GPU tests need a HIP device"


def launch(P, slabs, G, r, len_valid, gap=True):
    """The kernel on a case; with gap the slabs lie 16 RP elements apart and the gaps hold NaN, which any read of them would carry into the result.
    ps and sumsq_part start as NaN sentinels."""
    S, len_pad, RP = slabs.shape
    stride = len_pad * RP + (16 * RP if gap and S > 1 else 0)
    flat = np.full((S, stride), np.nan, dtype=P.dtype)
    flat[:, :len_pad * RP] = slabs.reshape(S, -1)
    out = na.op_hals_sweep(P, flat, G, r, len_valid, ps=np.full(len_pad, np.nan, P.dtype),
                           sumsq_part=np.full((len_pad // 16) * RP, np.nan, P.dtype))
    assert out["parts"] == len_pad // cols_and_chunk(P.dtype.type, RP)[0]
    return out


def assert_padding_is_zero(out, r, len_valid):
    P = out["P"]
    assert (P[:, r:] == 0).all() and (P[len_valid:, :] == 0).all()
    assert not np.isnan(out["ps"][:len_valid]).any() and np.isnan(out["ps"][len_valid:]).all()   # ps(y) written exactly where y < len_valid
    assert not np.isnan(out["sumsq_part"]).any()


@pytest.mark.parametrize("dtype,RP,r,len_valid,S", CASES)
def test_layout_is_exact(dtype, RP, r, len_valid, S):
    """Diagonal G with power-of-two entries and distinct integer a: h_new = max(0, a / G_kk) bit for bit.  A swapped lane, register, column or
    slab moves a distinct value to the wrong place."""
    rng = np.random.default_rng(RP * 1000 + r)
    P, slabs, G = ref.layout_case(RP, r, LEN_PAD, len_valid, S, rng, dtype)
    out = launch(P, slabs, G, r, len_valid)
    k = np.arange(r)
    want = np.maximum(0.0, slabs.astype(np.float64).sum(axis=0)[:len_valid, :r] / G[k, k].astype(np.float64))
    got = out["P"][:len_valid, :r].astype(np.float64)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} elements differ, first (y, k) = {bad[:4].tolist()}"
    assert_padding_is_zero(out, r, len_valid)


@pytest.mark.parametrize("dtype,RP,r,len_valid,S", CASES)
def test_order_and_chunks_are_exact(dtype, RP, r, len_valid, S):
    """Tridiagonal 0 / 1 G with unit diagonal (a few zeros: skipped) and integer a, h: the fp64 sweep is all-integer, and so must be the kernel's.
    Jacobi order, a stale or shifted row of G at an LDS chunk boundary or a wrong owner lane changes some h_k."""
    rng = np.random.default_rng(RP * 1000 + r + 1)
    P, slabs, G = ref.order_case(RP, r, LEN_PAD, len_valid, S, rng, dtype)
    out = launch(P, slabs, G, r, len_valid)
    want = ref.panel_sweep(P, slabs, G, r, len_valid)
    got = out["P"][:len_valid, :r].astype(np.float64)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} elements differ, first (y, k) = {bad[:4].tolist()}"
    assert_padding_is_zero(out, r, len_valid)


@pytest.mark.parametrize("dtype,RP,r,len_valid,S", CASES)
def test_arithmetic_within_running_error_bound(dtype, RP, r, len_valid, S):
    """Random diagonally dominant G, signed a: every element within sweep_bound of the fp64 sweep; ps(y) = sum_k h_k a_k within
    gamma_{RP+S} sum_k |h_k a_k| + sum_k b_k |a_k|; the rows of sumsq_part add up to the column sums of squares of the kernel's own output."""
    u = UNIT[dtype]
    rng = np.random.default_rng(RP * 1000 + r + 2)
    P, slabs, G = ref.dominant_case(RP, r, LEN_PAD, len_valid, S, rng, dtype)
    out = launch(P, slabs, G, r, len_valid)
    want = ref.panel_sweep(P, slabs, G, r, len_valid)
    b = ref.sweep_bound(P[:len_valid].T, slabs[:, :len_valid].transpose(0, 2, 1), G, r, u).T
    got = out["P"][:len_valid, :r].astype(np.float64)
    err = np.abs(got - want)
    assert (err <= b).all(), f"worst error / bound {(err / np.maximum(b, 1e-300)).max():.3g} at {np.unravel_index(np.argmax(err - b), err.shape)}"
    a = slabs.astype(np.float64).sum(axis=0)[:len_valid, :r]
    ps_want = (want * a).sum(axis=1)
    ps_tol = ref.gamma(RP + S, u) * np.abs(want * a).sum(axis=1) + (b * np.abs(a)).sum(axis=1)
    assert (np.abs(out["ps"][:len_valid] - ps_want) <= ps_tol).all()
    own = out["P"].astype(np.float64)
    colsq = (own * own).sum(axis=0)
    assert (np.abs(out["sumsq_part"].astype(np.float64).sum(axis=0) - colsq) <= ref.gamma(LEN_PAD, u) * colsq).all()
    assert_padding_is_zero(out, r, len_valid)


@pytest.mark.parametrize("dtype,RP,r,len_valid,S", CASES)
def test_padding_garbage_changes_nothing(dtype, RP, r, len_valid, S):
    """Finite garbage in the padding of G, P and the slabs (coordinates >= r, columns >= len_valid): the valid block, ps and the partial sums of
    squares are those of the clean launch bit for bit, the padding of the panel comes out exactly 0 and ps(y >= len_valid) keeps its sentinel."""
    rng = np.random.default_rng(RP * 1000 + r + 3)
    P, slabs, G = ref.dominant_case(RP, r, LEN_PAD, len_valid, S, rng, dtype)
    clean = launch(P, slabs, G, r, len_valid)
    dirty = launch(*ref.with_garbage(P, slabs, G, r, len_valid, rng), r, len_valid)
    assert np.array_equal(dirty["P"][:len_valid, :r], clean["P"][:len_valid, :r])
    assert (dirty["P"][:, r:] == 0).all(), "coordinates >= r are not 0"
    assert (dirty["P"][len_valid:, :] == 0).all(), "columns >= len_valid are not 0"
    assert np.array_equal(dirty["ps"][:len_valid], clean["ps"][:len_valid]) and np.isnan(dirty["ps"][len_valid:]).all()
    assert np.array_equal(dirty["sumsq_part"], clean["sumsq_part"]), "padding columns reach the partial sums of squares"


def test_availability_table():
    """The accepted padded ranks are exactly the instantiations; r = 0, r > RP, len_pad % 128 != 0 and len_valid > len_pad are refused."""
    for dtype, rps in INSTANTIATIONS.items():
        accepted = []
        for RP in range(64, 641, 64):
            P = np.zeros((128, RP), dtype)
            G = np.eye(RP, dtype=dtype)
            try:
                na.op_hals_sweep(P, np.zeros((1, 128 * RP), dtype), G, 1, 128)
                accepted.append(RP)
            except na.EngineError as e:
                assert e.status == 1, (RP, e)
        assert accepted == rps, (np.dtype(dtype).name, accepted)
        RP = rps[-1]
        G = np.eye(RP, dtype=dtype)
        for len_pad, r, len_valid in ((128, 0, 128), (128, RP + 1, 128), (192, 1, 192), (128, 1, 129)):
            with pytest.raises(na.EngineError) as info:
                na.op_hals_sweep(np.zeros((len_pad, RP), dtype), np.zeros((1, len_pad * RP), dtype), G, r, len_valid)
            assert info.value.status == 1, (len_pad, r, len_valid)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_normalisation(dtype):
    """W / d and H d with d = sqrt(sum of the parts) in fp64, within (gamma_parts / 2 + 4u) per element; a column whose sum is 0 (a zero column
    of W, and the padding coordinates) comes back bit-identical."""
    u = UNIT[dtype]
    rng = np.random.default_rng(31)
    RP, r, m, n, mpad, npad, parts = 128, 100, 250, 97, 256, 128, 7
    Wt = np.zeros((mpad, RP)); Wt[:m, :r] = rng.random((m, r))
    H = np.zeros((npad, RP)); H[:n, :r] = rng.random((n, r)) * 3
    Wt[:, 37] = 0.0
    Wt, H = Wt.astype(dtype), H.astype(dtype)
    bounds = np.linspace(0, mpad, parts + 1).astype(int)
    sq = np.stack([(Wt[a:b].astype(np.float64) ** 2).sum(axis=0) for a, b in zip(bounds, bounds[1:])]).astype(dtype)
    out = na.op_hals_normalize(Wt, H, sq)
    d = np.sqrt(sq.astype(np.float64).sum(axis=0))
    live = d > 0
    tol = 0.5 * ref.gamma(parts, u) + 4 * u
    W64, H64 = Wt.astype(np.float64), H.astype(np.float64)
    assert (np.abs(out["Wt"][:, live] - W64[:, live] / d[live]) <= tol * np.abs(W64[:, live] / d[live])).all()
    assert (np.abs(out["H"][:, live] - H64[:, live] * d[live]) <= tol * np.abs(H64[:, live] * d[live])).all()
    assert not live[37] and live[:r].sum() == r - 1 and not live[r:].any()
    assert np.array_equal(out["Wt"][:, ~live], Wt[:, ~live]) and np.array_equal(out["H"][:, ~live], H[:, ~live])
