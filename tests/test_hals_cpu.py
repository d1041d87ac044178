"""HALS without a GPU: the algorithm id on both C boundaries and in Python, and a self-check of the fp64 restatement the GPU tests compare with."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import hals_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _probe(source: str) -> str:
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "probe.cpp"), os.path.join(td, "probe")
        open(src, "w").write(source)
        subprocess.check_call(["g++", "-std=c++11", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        return subprocess.check_output([exe]).decode().strip()


def test_cxx_header_has_hals_after_nsnmf():
    out = _probe(r'''
#include <nmfgpu.h>
#include <cstdio>
int main() { printf("%d %d\n", (int)nmfgpu::NmfAlgorithm::nsNMF, (int)nmfgpu::NmfAlgorithm::HALS); return 0; }
''')
    assert out == "5 6"


def test_c_header_has_nmfamd_hals():
    out = _probe(r'''
#include <nmfgpu_amd.h>
#include <cstdio>
int main() { printf("%d %d\n", (int)NMFAMD_NSNMF, (int)NMFAMD_HALS); return 0; }
''')
    assert out == "5 6"


def test_python_ids():
    import nmfgpu_amd.api as api
    import nmfgpu_amd.engine as engine
    assert api.NmfAlgorithm.HALS == 6
    assert engine.ALGORITHMS["hals"] == 6
    # the existing ids stay where they are
    assert [int(a) for a in api.NmfAlgorithm][:6] == [0, 1, 2, 3, 4, 5]


def test_restatement_objective_is_non_increasing():
    rng = np.random.default_rng(7)
    m, n, r = 60, 45, 6
    V = rng.random((m, n))
    W, H = 1.0 - rng.random((m, r)), 1.0 - rng.random((r, n))
    W, H, errs = ref.run(V, W, H, 50)
    for a, b in zip(errs, errs[1:]):
        assert b <= a * (1 + 1e-12), (a, b)
    assert errs[-1] < errs[0]
    assert (W >= 0).all() and (H >= 0).all()
    # the normalisation leaves unit columns and does not change the model
    assert np.allclose(np.linalg.norm(W, axis=0), 1.0)


def test_restatement_normalisation_keeps_the_product():
    rng = np.random.default_rng(3)
    W, H = rng.random((20, 4)), rng.random((4, 15))
    W[:, 2] = 0.0                                           # a zero column is left alone (the sum > 0 guard)
    W2, H2 = ref.normalize(W, H)
    assert np.allclose(W2 @ H2, W @ H)
    assert (W2[:, 2] == 0).all() and np.array_equal(H2[2], H[2])


def test_restatement_fixed_point():
    """An exact factorisation with unit columns of W: every coordinate is at its clamped optimum (gradient 0, zeros stay 0), so one iteration is the identity."""
    rng = np.random.default_rng(11)
    m, n, r = 40, 30, 5
    W = rng.random((m, r))
    W /= np.linalg.norm(W, axis=0)
    H = rng.random((r, n))
    H[rng.random((r, n)) < 0.3] = 0.0
    V = W @ H
    W1, H1, err = ref.iteration(V, W, H)
    assert err < 1e-12 * np.linalg.norm(V)
    assert np.allclose(W1, W, rtol=0, atol=1e-12)
    assert np.allclose(H1, H, rtol=0, atol=1e-12)          # (the zeros of H too: their gradient is 0 up to rounding, the clamp keeps them at 0)


def test_restatement_is_gauss_seidel():
    """The H step uses the rows it has already updated: on a problem where W's columns are correlated it differs from the Jacobi form."""
    rng = np.random.default_rng(5)
    V = rng.random((30, 20))
    W = rng.random((30, 3)) + 1.0
    H = rng.random((3, 20))
    G, A = W.T @ W, W.T @ V
    jacobi = H.copy()
    for k in range(3):
        jacobi[k] = np.maximum(0.0, H[k] - (G[k] @ H - A[k]) / G[k, k])
    gs = ref.h_step(V, W, H)
    assert np.allclose(gs[0], jacobi[0])                    # row 0 sees no updated rows
    assert not np.allclose(gs[1:], jacobi[1:])


# ------------------------------------------------------------------ the sweep yardstick of tests/test_gpu_hals_sweep.py

def _bound(P, slabs, G, r, len_valid, u):
    return ref.sweep_bound(P[:len_valid].T, slabs[:, :len_valid].transpose(0, 2, 1), G, r, u).T


def test_sweep_is_the_restatement_step():
    """h_step and w_step are one sweep each; the sweep leaves rows >= r alone."""
    rng = np.random.default_rng(2)
    V, W, H = rng.random((25, 18)), rng.random((25, 4)), rng.random((4, 18))
    H1 = ref.h_step(V, W, H)
    G, A = W.T @ W, W.T @ V
    assert np.array_equal(H1, ref.sweep(H, A, G))
    P = np.vstack([H, rng.random((2, 18))])
    out = ref.sweep(P, np.vstack([A, np.zeros((2, 18))]), np.pad(G, ((0, 2), (0, 2))), r=4)
    assert np.array_equal(out[:4], H1) and np.array_equal(out[4:], P[4:])


@pytest.mark.parametrize("RP", [64, 128, 256, 384, 512])
def test_float32_sweeps_stay_inside_the_bound(RP):
    u = 2.0 ** -24
    rng = np.random.default_rng(RP)
    for r, S in ((RP, 1), (RP - 1, 3), (RP // 2 + 1, 2)):
        P, slabs, G = ref.dominant_case(RP, r, 128, 12, S, rng, np.float32)
        want = ref.panel_sweep(P, slabs, G, r, 12)
        b = _bound(P, slabs, G, r, 12, u)
        for order in ("sequential", "reversed"):
            got = ref.sweep_f32(P, slabs, G, r, 12, order)
            assert (np.abs(got - want) <= b).all(), (order, r, (np.abs(got - want) / b).max())
        # (not vacuous: on a diagonally dominant G the bound stays a small multiple of the local error)
        assert b.max() < 1e-3, b.max()


@pytest.mark.parametrize("variant", ["jacobi", "drop_last_slab", "next_row"])
def test_wrong_sweeps_fall_outside_the_bound(variant):
    u = 2.0 ** -24
    rng = np.random.default_rng(17)
    for RP, r in ((64, 64), (256, 200), (512, 511)):
        P, slabs, G = ref.dominant_case(RP, r, 128, 12, 3, rng, np.float32)
        want = ref.panel_sweep(P, slabs, G, r, 12)
        b = _bound(P, slabs, G, r, 12, u)
        got = ref.sweep_f32(P, slabs, G, r, 12, variant=variant)
        assert (np.abs(got - want) > b).any(), (variant, RP, r)


@pytest.mark.parametrize("case", ["layout_case", "order_case"])
def test_exact_constructions_are_exact_in_float32(case):
    rng = np.random.default_rng(23)
    make = getattr(ref, case)
    for RP, r, lv, S in ((64, 1, 1, 1), (64, 64, 63, 3), (384, 295, 255, 3), (320, 276, 17, 1), (512, 512, 255, 3)):
        P, slabs, G = make(RP, r, 256, lv, S, rng, np.float32)
        want = ref.panel_sweep(P, slabs, G, r, lv)
        for order in ("sequential", "reversed"):
            assert np.array_equal(ref.sweep_f32(P, slabs, G, r, lv, order), want), (case, RP, r, order)
        if case == "layout_case":
            k = np.arange(r)
            a = slabs.astype(np.float64).sum(axis=0)[:lv, :r]
            assert np.array_equal(want, np.maximum(0.0, a / G[k, k].astype(np.float64)))
            assert len(np.unique(a)) == a.size and np.abs(a).max() <= 2 ** 16
        else:
            # the Gauss-Seidel order is visible: the Jacobi form of the same step differs somewhere (r > 1)
            if r > 1:
                assert not np.array_equal(ref.sweep_f32(P, slabs, G, r, lv, variant="jacobi"), want)
