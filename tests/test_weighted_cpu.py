"""Weighted dense beta-divergence NMF without a GPU (docs/DIVERGENCE.md, "Weighted update"): the numpy restatement the GPU tests compare with
(tests/weighted_reference.py) against an independent triple-loop evaluation, against the unweighted restatement at weights of 1, its objective's monotonicity
with zero weights (an all-zero row and column included), the rule that a zero weight hides the value, and the nmfamd_params_v4 layout on both sides of the C
boundary."""
import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from tests import beta_general_reference as gen
from tests import weighted_reference as wref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS64 = float(np.finfo(np.float64).eps)
BETAS = [-1.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0]
PENALTIES = [(0.5, 0.5, 0.0, 0.0), (0.0, 0.0, 0.1, 0.1), (0.5, 0.5, 0.1, 0.1)]      # (l1W, l1H, l2W, l2H): tests/test_beta_general_cpu.py's


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@pytest.mark.parametrize("beta", BETAS)
def test_restatement_against_a_triple_loop(beta):
    out, red, r = 7, 5, 2
    rng = np.random.default_rng(3)
    X = gen.planted(out, red, k=2, seed=4)
    Om = wref.weights(out, red, seed=5, zero_row=2, zero_col=1)
    X[Om == 0] = np.nan
    A, B = 1.0 - rng.random((out, r)), 1.0 - rng.random((red, r))
    num, den = np.zeros((out, r)), np.zeros((out, r))
    tf, td = np.zeros(out), np.zeros(out)
    for o in range(out):
        for k in range(red):
            w = Om[o, k]
            if w == 0:
                continue
            x = X[o, k]
            p = sum(A[o, c] * B[k, c] for c in range(r)) + EPS64
            if beta == 1:
                d = x * math.log(x / p) - x + p
            elif beta == 0:
                d = x / p - math.log(x / p) - 1.0
            else:
                d = (x ** beta + (beta - 1.0) * p ** beta - beta * x * p ** (beta - 1.0)) / (beta * (beta - 1.0))
            tf[o] += w * (x - p) ** 2
            td[o] += w * d
            for c in range(r):
                num[o, c] += w * x * p ** (beta - 2.0) * B[k, c]
                den[o, c] += w * p ** (beta - 1.0) * B[k, c]
    got_num, got_den = wref.num_den(X, Om, A, B, beta, EPS64)
    assert np.all(np.isfinite(got_num)) and np.all(np.isfinite(got_den))
    assert np.allclose(got_num, num, rtol=1e-13, atol=0) and np.allclose(got_den, den, rtol=1e-13, atol=0)
    assert np.all(got_num[2] == 0) and np.all(got_den[2] == 0)
    got_tf, got_td = wref.terms(X, Om, A, B, beta, EPS64)
    assert np.allclose(got_tf, tf, rtol=1e-13, atol=0) and np.allclose(got_td, td, rtol=1e-12, atol=1e-15)
    want = A * (num / (den + EPS64 + 0.05 + 0.01 * A)) ** gen.gamma_of(beta)
    assert np.allclose(wref.half_step(X, Om, A, B, beta, EPS64, 0.05, 0.01), want, rtol=1e-13, atol=0)


@pytest.mark.parametrize("pen", [gen.NO_PENALTIES, (0.05, 0.05, 0.01, 0.01)])
@pytest.mark.parametrize("beta", [0.0, 0.5, 1.0, 2.0])
def test_weights_of_one_are_the_unweighted_restatement(beta, pen):
    m, n, r, iters = 131, 97, 9, 12
    V = gen.planted(m, n, seed=11)
    W0, H0 = gen.start(m, n, r, seed=12)
    for const_w in (False, True):
        want = gen.run(V, W0, H0, iters, beta, EPS64, pen=pen, const_w=const_w)
        got = wref.run(V, np.ones((m, n)), W0, H0, iters, beta, EPS64, pen=pen, const_w=const_w)
        figures = (rel(got[0], want[0]), rel(got[1], want[1]), abs(got[2] / want[2] - 1), abs(got[3] / want[3] - 1), abs(got[4] / want[4] - 1))
        print(f"beta {beta} pen {pen} const_w {const_w}: {figures}")
        assert max(figures) <= 1e-12, figures


@pytest.mark.parametrize("pen", [gen.NO_PENALTIES] + PENALTIES)
@pytest.mark.parametrize("beta", BETAS)
def test_weighted_objective_is_non_increasing(beta, pen):
    m, n, r = 131, 97, 9
    V = gen.planted(m, n, seed=r + 20)
    Om = wref.weights(m, n, seed=r + 22, zero_row=17, zero_col=40)
    W0, H0 = gen.start(m, n, r, seed=r + 21)
    out = wref.run(V, Om, W0, H0, 40, beta, EPS64, pen=pen, history=True)
    hist = out[5]
    assert len(hist) == 40 and np.all(np.isfinite(hist)) and hist[-1] < hist[0]
    for a, b in zip(hist, hist[1:]):
        assert b <= a * (1 + 1e-12), (a, b)
    W, H = out[0], out[1]
    assert np.all(np.isfinite(W)) and np.all(np.isfinite(H))
    assert np.all(W[17] == 0) and np.all(H[:, 40] == 0)      # (nothing observed there: a zero row of W, a zero column of H, no NaN)
    assert out[3] == pytest.approx(out[2] / np.sqrt(Om.sum()), rel=1e-15)


@pytest.mark.parametrize("beta", [0.0, 0.5, 1.0, 2.0])
def test_a_zero_weight_hides_the_value(beta):
    m, n, r = 60, 45, 7
    V = gen.planted(m, n, seed=31)
    Om = wref.weights(m, n, seed=32, zero_row=3, zero_col=5)
    W0, H0 = gen.start(m, n, r, seed=33)
    outs = []
    for hidden in (0.0, np.nan, np.inf, -5.0, 1e30):
        Vh = V.copy()
        Vh[Om == 0] = hidden
        outs.append(wref.run(Vh, Om, W0, H0, 8, beta, EPS64, pen=(0.05, 0.05, 0.01, 0.01)))
    for o in outs[1:]:
        assert np.array_equal(o[0], outs[0][0]) and np.array_equal(o[1], outs[0][1]) and o[2:] == outs[0][2:]
    assert np.all(np.isfinite(outs[0][0])) and np.all(np.isfinite(outs[0][1])) and np.all(np.isfinite(outs[0][2:]))


def test_params_v4_layout_matches_the_header():
    from nmfgpu_amd.engine import _ParamsV3, _ParamsV4
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "probe.c"), os.path.join(td, "probe")
        open(src, "w").write(r'''
#include <nmfgpu_amd.h>
#include <stddef.h>
#include <stdio.h>
int main(void) { printf("%zu %zu %zu %zu %zu\n", sizeof(nmfamd_params_v2), sizeof(nmfamd_params_v3), offsetof(nmfamd_params_v4, v3), offsetof(nmfamd_params_v4, weighted), sizeof(nmfamd_params_v4)); return 0; }
''')
        subprocess.check_call(["g++", "-x", "c++", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        size2, size3, off_v3, off_weighted, size4 = map(int, subprocess.check_output([exe]).decode().split())
    assert size3 == C.sizeof(_ParamsV3) == size2 + 8      # (v2 and v3 keep their sizes)
    assert off_v3 == _ParamsV4.v3.offset == 0
    assert off_weighted == _ParamsV4.weighted.offset == size3
    assert size4 == C.sizeof(_ParamsV4) == size3 + 8 and _ParamsV4._fields_[-1][0] == "weighted"


def test_the_new_entries_are_declared_and_wrapped():
    import nmfgpu_amd as na
    header = open(os.path.join(ROOT, "include", "nmfgpu_amd.h")).read()
    for name in ("nmfamd_engine_upload_dense_weighted", "nmfamd_op_beta_half_step_weighted_f32", "nmfamd_op_beta_half_step_weighted_f64"):
        assert name in header
    assert callable(na.op_beta_half_step_weighted)
