"""The restatement of the per-column dynamic stopping rule (tests/hals_dyn_reference.py; docs/HALS.md, "Dynamic stopping") on the CPU, and the soundness of the
inputs that tests/test_gpu_hals_dyn_sweep.py and tests/test_gpu_hals_dyn.py put on a device (tests/hals_dyn_cases.py): no GPU needed."""
import numpy as np
import pytest

from tests import hals_dyn_cases as dc
from tests import hals_dyn_reference as dyn
from tests import hals_multi_cases as mc
from tests import hals_multi_reference as multi
from tests import hals_reference as ref

CASES = [pytest.param(c, id=dc.case_id(c)) for c in dc.SWEEP_CASES]
SMALL = [c for c in dc.SWEEP_CASES if c[0] is np.float64 and c[1] in (64, 128)]


def small_problem(seed=3, r=11, ncols=40):
    """A dominant G, signed a and a start as tests/hals_reference.py's dominant_case builds them, as (P, A, G) with the columns along axis 1."""
    P, slabs, G = ref.dominant_case(64, r, 128, ncols, 1, np.random.default_rng(seed), np.float64)
    return P[:ncols, :r].T.copy(), slabs[0][:ncols, :r].T.copy(), G[:r, :r].copy()


def diverse_problem(l1=0.0, l2=0.0):
    """The valid block of a sweep case of the GPU test (slow and fast columns under one G), as (P, A, G) with the columns along axis 1."""
    case = (np.float64, 64, 61, 1)
    P, slabs, G = dc.sweep_case(case, l1, l2)
    return P[:dc.LEN_VALID, :61].T.copy(), slabs[0][:dc.LEN_VALID, :61].T.copy(), G[:61, :61].copy()


@pytest.mark.parametrize("l1,l2", dc.PENALTIES)
def test_tolerance_zero_is_the_static_restatement(l1, l2):
    P, A, G = small_problem()
    got, counts = dyn.sweeps_dyn(P, A, G, None, 5, 0.0, l1, l2)
    assert np.array_equal(got, multi.sweeps(P, A, G, None, 5, l1, l2)) and (counts == 5).all()
    # ... and the iteration is hals_multi_reference's
    V, W, H = mc.planted(60, 50, 7, np.float64, seed=2)
    p = (l1, l1, l2, l2)
    W1, H1, e1, ch, cw = dyn.iteration(V, W, H, 3, 2, 0.0, p)
    W0, H0, e0 = multi.iteration(V, W, H, 3, 2, p)
    assert np.array_equal(W1, W0) and np.array_equal(H1, H0) and e1 == e0 and (ch == 3).all() and (cw == 2).all()


@pytest.mark.parametrize("l1,l2", dc.PENALTIES)
@pytest.mark.parametrize("case", [pytest.param(c, id=dc.case_id(c)) for c in SMALL])
def test_counts_in_range_and_objective_non_increasing(case, l1, l2):
    """Counts lie in 1 ... s; the (penalised) objective of every column does not rise from one sweep to the next, frozen columns included (they keep theirs)."""
    P, slabs, G = dc.sweep_case(case, l1, l2)
    r = case[2]
    A = slabs.astype(np.float64).sum(axis=0)[:dc.LEN_VALID, :r].T
    hist = []
    out, counts = dyn.sweeps_dyn(P[:dc.LEN_VALID, :r].T, A, G[:r, :r], r, dc.MAX_SWEEPS, dc.TOL, l1, l2, history=hist)
    assert counts.min() >= 1 and counts.max() <= dc.MAX_SWEEPS and len(hist) == counts.max()
    obj = [dyn.column_objective(P[:dc.LEN_VALID, :r].T, A, G, r, l1, l2)] + [dyn.column_objective(h, A, G, r, l1, l2) for h in hist]
    for before, after in zip(obj, obj[1:]):
        assert (after <= before + 1e-12 * (1.0 + np.abs(before))).all()
    # a frozen column keeps its value: the state after its last sweep is the final one
    for j in range(dc.LEN_VALID):
        assert np.array_equal(hist[counts[j] - 1][:, j], out[:r, j])


def test_fixed_point_gets_count_one_and_keeps_its_value():
    # an all-integer problem, so that the fixed point is exact: G = 4 I - tridiagonal ones, integer solutions x > 0, a = G x
    rng = np.random.default_rng(4)
    r, ncols = 11, 40
    G = 4.0 * np.eye(r) - np.eye(r, k=1) - np.eye(r, k=-1)
    solved = rng.integers(1, 6, size=(r, ncols)).astype(np.float64)
    A = G @ solved
    assert np.array_equal(multi.sweeps(solved, A, G, None, 1), solved), "not a fixed point of the sweep"
    start = solved + 1.0
    start[:, ::2] = solved[:, ::2]
    got, counts = dyn.sweeps_dyn(start, A, G, None, 9, 0.1)
    assert (counts[::2] == 1).all() and np.array_equal(got[:, ::2], solved[:, ::2])
    assert (counts[1::2] > 1).all()


@pytest.mark.parametrize("l1,l2", dc.PENALTIES)
def test_permuting_the_columns_permutes_results_and_counts(l1, l2):
    P, A, G = diverse_problem(l1, l2)
    perm = np.random.default_rng(1).permutation(P.shape[1])
    got, counts = dyn.sweeps_dyn(P, A, G, None, 9, 0.1, l1, l2)
    got_p, counts_p = dyn.sweeps_dyn(P[:, perm], A[:, perm], G, None, 9, 0.1, l1, l2)
    assert np.array_equal(counts_p, counts[perm]) and len(set(counts.tolist())) > 1
    assert np.allclose(got_p, got[:, perm], rtol=0, atol=1e-14)      # (the row-times-block products may round differently for another column order)


def test_forced_counts_reproduce_the_rule():
    P, A, G = diverse_problem()
    got, counts = dyn.sweeps_dyn(P, A, G, None, 9, 0.1)
    assert len(set(counts.tolist())) > 2
    again, counts2 = dyn.sweeps_dyn(P, A, G, None, 9, 0.5, forced=counts)      # (the tolerance is not looked at)
    assert np.array_equal(counts2, counts) and np.array_equal(again, got)


@pytest.mark.parametrize("l1,l2", dc.PENALTIES)
@pytest.mark.parametrize("case", CASES)
def test_gpu_sweep_inputs_are_sound(case, l1, l2):
    """Each input of the kernel-level GPU test: the fp64 restatement's counts pass the diversity conditions, and the restatement in numpy fp32 stays within the cap
    on threshold flips that the GPU test holds the kernel to."""
    _, counts = dc.restated(case, l1, l2)
    assert dc.diversity_faults(case, counts) == []
    P, slabs, G = dc.sweep_case(case, l1, l2)
    _, c32 = dyn.panel_sweeps_dyn(P, slabs, G, case[2], dc.LEN_VALID, dc.MAX_SWEEPS, dc.TOL, l1, l2, dtype=np.float32)
    same = float((c32 == counts).mean())
    print(dc.case_id(case), (l1, l2), "counts", np.bincount(counts, minlength=dc.MAX_SWEEPS + 1)[1:].tolist(), "fp32 numpy agrees on", same)
    assert same >= dc.FLIP_CAP


@pytest.mark.parametrize("case", CASES)
def test_gpu_exit_inputs_are_sound(case):
    """The input of the GPU test's workgroup-exit check: at delta = 0.999 every count is at most 2, in fp64 and in numpy fp32, and some columns do take two."""
    P, slabs, G = dc.settled_case(case)
    for dtype in (np.float64, np.float32):
        _, counts = dyn.panel_sweeps_dyn(P, slabs, G, case[2], dc.LEN_VALID, dc.LOOSE_MAX, dc.LOOSE_TOL, dtype=dtype)
        assert counts.min() >= 1 and counts.max() == 2


@pytest.mark.parametrize("penalised", [False, True])
@pytest.mark.parametrize("m,n,r", dc.ENGINE_SHAPES)
def test_gpu_engine_inputs_are_sound(m, n, r, penalised):
    """The engine-level GPU test's one iteration at delta = 0.1, sweeps (8, 8): the counts of both steps are not all equal, and numpy fp32 agrees with fp64 within
    the cap."""
    p = dc.ENGINE_PENALTIES if penalised else (0.0, 0.0, 0.0, 0.0)
    V, W, H = dc.engine_problem(m, n, r, np.float32)
    _, _, _, ch, cw = dyn.iteration(V, W, H, dc.ENGINE_SWEEPS, dc.ENGINE_SWEEPS, dc.ENGINE_TOL, p)
    assert 1 <= ch.min() and ch.max() <= dc.ENGINE_SWEEPS and 1 <= cw.min() and cw.max() <= dc.ENGINE_SWEEPS
    V64, W64, H64 = (np.asarray(x, np.float64) for x in (V, W, H))
    H32, ch32 = dyn.sweeps_dyn(H, (W64.T @ V64), (W64.T @ W64), None, dc.ENGINE_SWEEPS, dc.ENGINE_TOL, p[1], p[3], dtype=np.float32)
    same_h = float((ch32 == ch).mean())
    print((m, n, r), penalised, "H counts", np.bincount(ch, minlength=dc.ENGINE_SWEEPS + 1)[1:].tolist(), "W counts",
          np.bincount(cw, minlength=dc.ENGINE_SWEEPS + 1)[1:].tolist(), "fp32 numpy agrees on", same_h)
    assert same_h >= dc.FLIP_CAP
