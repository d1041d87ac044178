"""Device-free checks of what tests/test_gpu_inverse.py relies on (tests/inverse_reference.py, tests/inverse_cases.py; docs/INVERSE.md):
  1. every case is conditioned as the bounds assume (cond2 <= 1e4), its refined inverse is converged, and LAPACK's double-precision inverse, rounded to the
     type under test, keeps bounds (a) and (b): the bounds ask nothing a backward-stable inversion in double cannot deliver;
  2. the numpy restatement of the Gauss-Jordan body, which divides a pivot row by its pivot once, at the write-back, keeps every bound and equality of the GPU tests;
  3. every deliberate defect of inverse_reference.MUTATIONS leaves at least one of them -- among them the pivot row formed as row_p - (1 - 1 / piv) row_p, which
     loses bound (a) in double from scale 2^12 on and the scale equivariance at every scale."""
import numpy as np
import pytest

from tests import inverse_cases as cases
from tests import inverse_reference as ref

DTYPES = ("float32", "float64")


def test_extended_precision_is_available():
    assert ref.EPS_X < 2e-19


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ["gauss_jordan", "householder_small", "householder"])
def test_cases_are_conditioned_and_a_double_inverse_keeps_the_bounds(dtype, which):
    worst_a = worst_b = 0.0
    every = {"gauss_jordan": lambda: cases.all_cases(dtype, cases.GJ_RANKS, cases.GJ_SET),
             "householder_small": lambda: cases.all_cases(dtype, cases.HH_SMALL_RANKS, cases.HH_SMALL_SET),
             "householder": lambda: cases.householder_cases(dtype)}[which]
    for c in every():
        r, cond, Areg = c["r"], c["cond"], c["Areg"]
        # (the exact kind spans 2^-8 ... 2^8 by construction: it is held to equality, zero residual included, not to a bound that depends on cond)
        assert cond <= cases.COND_MAX or c["kind"] == "exact", (c["name"], cond)
        # converged: what is left is the evaluation of the residual itself, r products of magnitude <= |X|_2 |A|_2 = cond per element
        assert ref.residual(c["Xref"], Areg) <= 4 * max(r, 2) * ref.EPS_X * cond, c["name"]
        lapack = np.linalg.inv(Areg.astype(np.float64)).astype(dtype)
        ra = ref.residual(lapack, Areg) / ref.bound_a(dtype, cond)
        worst_a = max(worst_a, ra)
        assert ra <= 1, (c["name"], ra)
        if dtype == "float32":
            rb = ref.excess_b(lapack, c["Xref"], cond)
            worst_b = max(worst_b, rb)
            assert rb <= 1, (c["name"], rb)
        if c["kind"] == "exact":
            assert np.array_equal(lapack, ref.lower(c["Xref"], dtype)) and ref.residual(ref.lower(c["Xref"], dtype), Areg) == 0, c["name"]
    print(f"\nLAPACK in double, rounded to {dtype}: worst residual / bound (a) {worst_a:.3g}, worst error / bound (b) {worst_b:.3g}")


def _gj(c, mutation=None):
    return ref.gauss_jordan(c["A"], c["offdiag"], c["diag"], mutation)


@pytest.mark.parametrize("dtype", DTYPES)
def test_restated_gauss_jordan_keeps_every_bound(dtype):
    for r in cases.GJ_RANKS:
        plain = {}
        for kind, reg, k in cases.GJ_SET:
            c = cases.case(kind, r, reg, k, dtype)
            X = _gj(c)
            assert ref.residual(X, c["Areg"]) <= ref.bound_a(dtype, c["cond"]), c["name"]
            if dtype == "float32":
                assert ref.excess_b(X, c["Xref"], c["cond"]) <= 1, c["name"]
            if kind == "exact":
                assert np.array_equal(X, ref.lower(c["Xref"], dtype)), c["name"]
            if k == 0:
                plain[kind, reg] = X
            else:
                assert np.array_equal(X * np.dtype(dtype).type(2.0) ** k, plain[kind, reg]), f"{c['name']}: not the bits of scale 2^0"


def test_difference_pivot_row_loses_the_residual_bound_in_double_and_the_equivariance():
    """The formula the kernels carried before the division of the pivot row was deferred to the write-back."""
    for r in (2, 9, 40, 64):
        c0 = cases.case("spd", r, cases.REGS[1], 0, "float64")
        X0 = _gj(c0, "difference_pivot_row")
        for k in (12, 24):
            c = cases.case("spd", r, cases.REGS[1], k, "float64")
            X = _gj(c, "difference_pivot_row")
            assert ref.residual(X, c["Areg"]) > ref.bound_a("float64", c["cond"]), c["name"]
            assert not np.array_equal(X * 2.0 ** k, X0), c["name"]
    # (float32 output: the loss stays under the output rounding, and so does the difference between two scales)
    c0, c = cases.case("spd", 40, cases.REGS[1], 0, "float64"), cases.case("spd", 40, cases.REGS[1], -24, "float64")
    assert not np.array_equal(_gj(c, "difference_pivot_row") * 2.0 ** -24, _gj(c0, "difference_pivot_row"))


def test_regulariser_added_in_double_leaves_bound_b():
    hit = [r for r in cases.GJ_RANKS if r > 1 and
           ref.excess_b(_gj(cases.case("spd", r, cases.REGS[1], 0, "float32"), "regulariser_in_double"), cases.case("spd", r, cases.REGS[1], 0, "float32")["Xref"],
                        cases.case("spd", r, cases.REGS[1], 0, "float32")["cond"]) > 1]
    assert len(hit) >= len(cases.GJ_RANKS) // 2, hit


@pytest.mark.parametrize("mutation", ["transposed_write_back", "unpermuted_write_back"])
def test_wrong_write_back_shows_on_the_exact_and_permuted_cases(mutation):
    for r in cases.GJ_RANKS:
        if r < 4:
            continue      # (below four rows a rotation by three is the identity or its own transpose)
        for kind in ("exact", "perm"):
            c = cases.case(kind, r, cases.REGS[0], 0, "float32")
            X = _gj(c, mutation)
            if kind == "exact":
                assert not np.array_equal(X, ref.lower(c["Xref"], "float32")), c["name"]
            else:
                assert ref.residual(X, c["Areg"]) > ref.bound_a("float32", c["cond"]), c["name"]
