"""The r x r inverse of the least-squares algorithms on every route that launches it, one launch of one workgroup at a time through na.op_inverse, against the
extended-precision reference of tests/inverse_reference.py on the cases of tests/inverse_cases.py (docs/INVERSE.md maps kernels, routes and tests;
tests/test_inverse_cpu.py checks reference, cases and bounds without a device).

Routes:  0  launch_inverse_small as the engines call it: k_inverse_gj64<T> (eight waves) up to r = 64, k_fill_small + k_inverse_small<T> (Householder) above
         1  the Householder launch at any r
         2  the Gauss-Jordan body as the passenger workgroup of k_factor_product_f32 (eight waves)              float32, r <= 64
         3  ... of k_factor_product_x3 (four waves, sixteen columns each: what the fp32 engines run)            float32, r <= 64

What every launch is held to (`check`), the letters as in docs/INVERSE.md:
  a  residual      max(|X Areg - I|, |Areg X - I|) <= 8 eps(T) cond2(Areg)
  b  float32       |X - fl32(Xref)| <= ulp32(Xref) + 8 2^-52 cond2 max|Xref| element-wise: the regulariser is added in T, the arithmetic is double
  c  exact         the `exact` kind returns the exact inverse bit for bit (a transposed or mis-permuted write-back shows as whole entries)
  d  padding       the RP x RP output starts as NaN: zero outside the r x r block, finite inside
  e  input         Gauss-Jordan leaves the input buffer as it was; Householder leaves A + regulariser (one addition in T) in the r x r block and the padding alone
and across launches:
  f  scale         Gauss-Jordan: op(2^k A, 2^k reg) 2^k has the bits of op(A, reg), k = 12, 24, -24 (Householder: a at every scale)
  g  routes        float32: routes 2 and 3 return the bits of route 0, and the product they ride on the bits of the same product without a passenger
  h  determinism and refusals."""
import functools

import numpy as np
import pytest

import nmfgpu_amd as na
from tests import inverse_cases as cases
from tests import inverse_reference as ref

pytestmark = pytest.mark.gpu

WORST = {}      # (route, kernel, dtype, bound) -> worst observed figure / bound, printed when the module is done
DTYPES = ("float32", "float64")
INVALID_ARGUMENT = 1


@pytest.fixture(scope="module", autouse=True)
def _library_is_native():
    assert na.device_count() >= 1, "GPU tests need a HIP device"
    yield
    for (route, kernel, dtype, bound), ratio in sorted(WORST.items()):
        print(f"\nworst figure / bound  route {route} {kernel:<12} {dtype} ({bound}): {ratio:.3g}", end="")
    print()


@functools.lru_cache(maxsize=None)
def product():
    A, F = cases.product_operands()
    return A, F, na.op_factor_product(A, F)[0], na.op_factor_product_x3(A, F)


def launch(c, route):
    if route >= 2:
        A, F = product()[:2]
        return na.op_inverse(c["A"], c["offdiag"], c["diag"], route=route, full=True, product=(A, F))
    return na.op_inverse(c["A"], c["offdiag"], c["diag"], route=route, full=True)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def check(c, got, route, failures):
    """a ... e on one launch; what fails is appended to `failures` with its figure, so that one run names every case."""
    r, dt, name = c["r"], c["dtype"], f"route {route} {c['name']}"
    gauss_jordan = route >= 2 or (route == 0 and r <= 64)
    kernel = "gauss_jordan" if gauss_jordan else "householder"
    RP, inv, after = got["rp"], got["inv"], got["a_after"]
    assert RP == na.inverse_padded_rank(r, dt) and inv.shape == (RP, RP) and after.shape == (RP, RP)
    X = inv[:r, :r]

    def fail(letter, what):
        failures.append(f"({letter}) {name}: {what}")

    def within(letter, figure_over_bound, what):
        key = (route, kernel, dt.name, letter)
        WORST[key] = max(WORST.get(key, 0.0), figure_over_bound)
        if not figure_over_bound <= 1:
            fail(letter, f"{what} is {figure_over_bound:.3g} of its bound (cond2 {c['cond']:.3g})")
    # d
    if not np.all(np.isfinite(X)):
        fail("d", "a value of the r x r block is not finite")
    if not (np.all(inv[r:, :] == 0) and np.all(inv[:, r:] == 0)):
        fail("d", "the output is not zero outside the r x r block")
    # e
    want_block = c["A"] if gauss_jordan else c["Areg"]
    if not np.array_equal(bits(after[:r, :r]), bits(want_block)):
        fail("e", "the input buffer does not hold " + ("its input" if gauss_jordan else "A + regulariser added in T"))
    if not (np.all(np.isnan(after[r:, :])) and np.all(np.isnan(after[:, r:]))):
        fail("e", "the padding of the input buffer was written")
    # a, b, c
    within("a", ref.residual(X, c["Areg"]) / ref.bound_a(dt, c["cond"]), "the residual")
    if dt == np.float32:
        within("b", ref.excess_b(X, c["Xref"], c["cond"]), "the distance to the rounded truth")
    if c["kind"] == "exact" and not np.array_equal(X, ref.lower(c["Xref"], dt)):
        fail("c", f"not the exact inverse at {np.argwhere(X != ref.lower(c['Xref'], dt))[:4].tolist()}")
    if route >= 2:
        # g
        if not np.array_equal(bits(X), bits(launch(c, 0)["inv"][:r, :r])):
            fail("g", "not the bits of the stand-alone launch")
        if not np.array_equal(bits(got["out"]), bits(product()[route])):
            fail("g", "the product that carried the passenger differs from the same product without one")
    return X


def run(dtype, ranks, selection, route):
    failures = []
    for r in ranks:
        plain = {}
        for kind, reg, k in selection:
            c = cases.case(kind, r, reg, k, dtype)
            X = check(c, launch(c, route), route, failures)
            gauss_jordan = route >= 2 or (route == 0 and r <= 64)
            if gauss_jordan and kind != "exact":
                # f (every selection lists a case's scale 2^0 ahead of its other scales)
                if k == 0:
                    plain[kind, reg] = X
                elif (kind, reg) in plain and not np.array_equal(X * c["dtype"].type(2.0) ** k, plain[kind, reg]):
                    rel = np.abs(X.astype(np.float64) * 2.0 ** k / plain[kind, reg].astype(np.float64) - 1).max()
                    failures.append(f"(f) route {route} {c['name']}: times 2^{k} not the bits of scale 2^0, relative difference up to {rel:.3g}")
    assert not failures, f"{len(failures)} failures, the first of them:\n" + "\n".join(failures[:12])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("r", cases.GJ_RANKS)
def test_gauss_jordan_stand_alone(dtype, r):
    run(dtype, (r,), cases.GJ_SET, 0)


@pytest.mark.parametrize("route", [2, 3])
@pytest.mark.parametrize("r", cases.GJ_RANKS)
def test_gauss_jordan_as_a_passenger_of_the_product(route, r):
    run("float32", (r,), cases.GJ_SET, route)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("r", cases.HH_RANKS)
def test_householder_as_the_engines_reach_it(dtype, r):
    run(dtype, (r,), cases.HH_SET_LARGE if r >= cases.HH_LARGE_FROM else cases.HH_SET, 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("r", cases.HH_SMALL_RANKS + cases.HH_RANKS[:2])
def test_householder_launched_directly(dtype, r):
    run(dtype, (r,), cases.HH_SMALL_SET if r <= 64 else cases.HH_SET, 1)


@pytest.mark.parametrize("dtype,route,r", [("float32", 0, 40), ("float64", 0, 40), ("float32", 2, 17), ("float32", 3, 17), ("float32", 0, 100), ("float64", 1, 33)])
def test_the_same_call_twice_returns_the_same_bits(dtype, route, r):
    c = cases.case("spd", r, cases.REGS[1], 0, dtype)
    one, two = launch(c, route), launch(c, route)
    for key in ("inv", "a_after") + (("out",) if route >= 2 else ()):
        assert np.array_equal(bits(one[key]), bits(two[key])), key


@pytest.mark.parametrize("dtype,route,r,X", [("float64", 2, 8, 2560), ("float64", 3, 8, 2560), ("float32", 2, 65, 2560), ("float32", 3, 65, 2560), ("float32", 2, 8, 1280)],
                         ids=["f64_route2", "f64_route3", "r65_route2", "r65_route3", "ten_x_tiles_route2"])
def test_refusals_leave_every_output_alone(dtype, route, r, X):
    """Routes 2 and 3 exist in float32 up to r = 64, and the fp32 MFMA product carries a passenger from sixteen x-tiles on (launch_fp_d)."""
    c = cases.case("spd", r, cases.REGS[1], 0, dtype)
    RP = na.inverse_padded_rank(r, dtype)
    A, F = product()[:2]
    A = np.asfortranarray(A[:X])
    outs = dict(inv=np.full((RP, RP), np.nan, dtype=dtype, order="F"), a_after=np.full((RP, RP), np.nan, dtype=dtype, order="F"))
    OUT = np.full((64, X), np.nan, dtype=np.float32, order="F")
    with pytest.raises(na.EngineError) as err:
        na.op_inverse(c["A"], c["offdiag"], c["diag"], route=route, full=outs, product=(A, F, OUT))
    assert err.value.status == INVALID_ARGUMENT
    assert np.all(np.isnan(outs["inv"])) and np.all(np.isnan(outs["a_after"])) and np.all(np.isnan(OUT))


def test_plain_call_still_returns_the_r_x_r_inverse():
    c = cases.case("spd", 40, cases.REGS[1], 0, "float32")
    X = na.op_inverse(c["A"], c["offdiag"], c["diag"])
    assert X.shape == (40, 40) and X.dtype == np.float32 and np.array_equal(bits(X), bits(launch(c, 0)["inv"][:40, :40]))
