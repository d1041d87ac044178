"""The start of an odd wave piece of the split-operand product (kernels_x3.hip, ODD): both ring slots are requested ahead of the
piece's first K-step, that step runs out of slot 1 with the slot's refill in its last phase, and the loop of whole turns runs at
least once.  The shapes are the smallest at which that start can go wrong (pieces as x3_odd_pieces and plan_splits_x3 deal them
on 256 CUs, four wave pieces per K slice):

    (X, Y)       K-steps   pieces                      pins
    (128, 192)   12        3, 3, 3, 3                  the loop runs exactly once
    (300, 540)   34        7, 9, 9, 9                  mixed lengths, ragged last step (540 = 33 * 16 + 12)
    (300, 560)   35        9, 9, 9, 9                  one step past the range: the clamped step against the all-zero K-step
    (300, 790)   50        5, 7, 5, 7 | 7, 5, 7, 7     two K slices

Bounds: integer operands in [0, 128) keep every partial sum exact in fp32 (Y * 127^2 <= 790 * 16129 < 2^24), so the result is
the int64 product whatever the order of addition; random operands keep the product's own bound of tests/test_gpu_parity.py,
|gpu - fp64| <= 4e-7 * sum|a b| per element; the engine's factors the suite's 2e-4 against the fp64 oracle."""
import ctypes as C

import numpy as np
import pytest

import nmfgpu_amd as na
from nmfgpu_amd._lib import library
from oracle import oracle

pytestmark = pytest.mark.gpu

SHAPES = [(128, 192), (300, 540), (300, 560), (300, 790)]
RANKS = [64, 33]


def F(a):
    return np.asfortranarray(a)


def rel(a, b):
    return np.linalg.norm(a.astype(np.float64) - b.astype(np.float64)) / max(np.linalg.norm(b.astype(np.float64)), 1e-300)


@pytest.fixture(scope="module", autouse=True)
def _library_is_native():
    assert na.device_count() >= 1, "GPU tests need a HIP device"
    assert na.initialize() in (na.ResultType.Success, na.ResultType.ErrorAlreadyInitialized)
    na.set_verbosity(na.Verbosity.Nothing)
    yield
    na.finalize()


def x_tiled(A, Fm):
    return na.op_factor_product_x3(A, Fm)


def y_tiled(A, Fm):
    X, Y = A.shape
    r = Fm.shape[0]
    out = np.zeros((r, X), dtype=np.float32, order="F")
    st = library().nmfamd_op_factor_product_x3_ytiled(C.c_void_p(A.ctypes.data), C.c_long(X), X, Y, C.c_void_p(Fm.ctypes.data), C.c_long(r), r,
                                                      C.c_void_p(out.ctypes.data), C.c_long(r), 0, None)
    assert st == 0, st
    return out


@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("X,Y", SHAPES)
def test_integer_operands_give_the_exact_product(X, Y, r):
    """A K-step run twice, skipped, or paired with another step's fragments changes an exact integer sum."""
    assert Y * 127 * 127 < 2 ** 24
    rng = np.random.default_rng(1000 * X + Y + r)
    A = F(rng.integers(0, 128, (X, Y)).astype(np.float32)); Fm = F(rng.integers(0, 128, (r, Y)).astype(np.float32))
    want = (Fm.astype(np.int64) @ A.astype(np.int64).T).astype(np.float32)
    for name, form in (("x-tiled", x_tiled), ("y-tiled", y_tiled)):
        out = form(A, Fm)
        wrong = int((out != want).sum())
        print(f"{name} ({X}, {Y}, r = {r}): {wrong} of {want.size} elements differ from the int64 product")
        assert np.array_equal(out, want), name


@pytest.mark.parametrize("r", RANKS)
@pytest.mark.parametrize("X,Y", SHAPES)
def test_random_operands_keep_the_bound_and_the_forms_agree(X, Y, r):
    rng = np.random.default_rng(7 * X + 3 * Y + r)
    A = F((rng.random((X, Y)) - 0.25).astype(np.float32)); Fm = F((rng.random((r, Y)) - 0.3).astype(np.float32))
    want = Fm.astype(np.float64) @ A.astype(np.float64).T
    bound = 4e-7 * (np.abs(Fm).astype(np.float64) @ np.abs(A).astype(np.float64).T)
    ox, oy = x_tiled(A, Fm), y_tiled(A, Fm)
    print(f"({X}, {Y}, r = {r}): largest |gpu - fp64| / sum|a b| = {(np.abs(ox - want) / bound).max() * 4e-7:.3g} (bound 4e-7)")
    assert (np.abs(ox - want) <= bound).all()
    assert np.array_equal(oy, ox)


def test_engine_on_the_16_row_tile_forms(monkeypatch):
    """m = 300, n = 540, r = 64, MU: the split-operand product on one resident image of V runs the shipped 16-row-tile forms, x-tiled for V H^T (34 K-steps:
    pieces 7, 9, 9, 9) and y-tiled for W^T V (19 K-steps: 5, 5, 5, 5, one step past the range); on two images the 128-row-tile forms."""
    m, n, r, iters = 300, 540, 64, 10
    rng = np.random.default_rng(61)
    V = F(rng.random((m, n)).astype(np.float32))
    W = F((1.0 - rng.random((m, r))).astype(np.float32))
    H = F((1.0 - rng.random((r, n))).astype(np.float32))
    V64, W64, H64 = (F(x.astype(np.float64)) for x in (V, W, H))
    oracle.run("mu", V64, W64, H64, iters)
    out = {}
    for one in (True, False):
        monkeypatch.setenv("NMFAMD_ONE_IMAGE", "1" if one else "0")
        eng = na.Engine(m, n, r, "mu")
        g = eng.geometry()
        assert g["product_kernel"] == 2
        assert g["resident_images"] == (1 if one else 2)
        eng.upload(V); eng.set_factors(W, H)
        eng.iterate(iters, last_iteration=iters)
        out[one] = eng.get_factors()
        print(f"one image = {one}: rel W {rel(out[one][0], W64):.3g}, rel H {rel(out[one][1], H64):.3g} (bound 2e-4)")
        assert rel(out[one][0], W64) < 2e-4 and rel(out[one][1], H64) < 2e-4
    assert np.array_equal(out[True][0], out[False][0]) and np.array_equal(out[True][1], out[False][1])
