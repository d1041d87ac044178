"""A coordinate-descent missing-value engine that is re-entered equals a fresh one, in the manner of tests/test_gpu_engine_reentry.py: after the engine has
iterated on one problem, a new V and new factors from outside must leave nothing of the old state behind -- W, H and the error of three iterations are compared bit
for bit with an engine that never held the old state.  The solver is a setting of the engine, not a factor change: it survives every re-entry action, and a switch
of the solver between the two problems leaves nothing behind either."""
import numpy as np
import pytest

import nmfgpu_amd as na
from tests.test_gpu_device_io import F, assert_same_run, on_device, same_bits

pytestmark = pytest.mark.gpu

M, N = 130, 257
SEED = 12345
CD = dict(missing_values=True, missing_solver="cd", missing_sweeps_h=2, missing_sweeps_w=3, l1_w=0.02, l2_h=0.01)
FAMILIES = {"masked_cd_f32_r5": (np.float32, 5), "masked_cd_f64_r70": (np.float64, 70)}
# (a) V, then both factors in one call; (b) W and H in two calls, W first; (c) H first; (d) the factors through the device entries; (e) V, then randomize;
# (f) V, then randomize W alone and set H; (g) as (a) on an engine that ran the multiplicative update on the first problem and was switched in between
ACTIONS = ("a", "b", "c", "d", "e", "f", "g")
_problems, _references = {}, {}


def problem(family):
    if family not in _problems:
        dtype, r = FAMILIES[family]
        both = []
        for seed in (7, 8):
            rng = np.random.default_rng(seed)
            V = (rng.random((M, N)) + 0.1).astype(dtype)
            V[rng.random((M, N)) < 0.6] = np.nan
            V = F(V)
            W = F((1.0 - rng.random((M, r))).astype(dtype))
            H = F((1.0 - rng.random((r, N))).astype(dtype))
            for a in (V, W, H):
                a.setflags(write=False)
            both.append((V, W, H))
        _problems[family] = both
    return _problems[family]


def make(family, **kw):
    dtype, r = FAMILIES[family]
    return na.Engine(M, N, r, "mu", dtype=dtype, **{**CD, **kw})


def enter(eng, action, V, W0, H0):
    eng.upload(V)
    if action in ("a", "g"):
        eng.set_factors(W0, H0)
    elif action == "b":
        eng.set_factors(W0, None)
        eng.set_factors(None, H0)
    elif action == "c":
        eng.set_factors(None, H0)
        eng.set_factors(W0, None)
    elif action == "d":
        eng.set_factors_device(on_device(np.asarray(W0), "cm_gap")[0], on_device(np.asarray(H0), "rm_gap")[0])
    elif action == "e":
        eng.randomize(SEED)
    elif action == "f":
        eng.randomize(SEED, w=True, h=False)
        eng.set_factors(None, H0)
    else:
        raise ValueError(action)


def three_iterations(eng):
    eng.iterate(3, error_every=1)
    W, H = eng.get_factors()
    return W, H, eng.frobenius


def reference(family, action):
    key = (family, action if action in ("e", "f") else "a")
    if key not in _references:
        V, W0, H0 = problem(family)[0]
        eng = make(family)
        enter(eng, key[1], V, W0, H0)
        assert eng.geometry()["padded_rank"] == (64 if FAMILIES[family][1] <= 64 else 128)
        _references[key] = three_iterations(eng)
        eng.close()
    return _references[key]


@pytest.mark.parametrize("action", ACTIONS)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_reentered_engine_equals_fresh(family, action):
    (V, W0, H0), (V2, W1, H1) = problem(family)
    want = reference(family, action)
    if action == "g":
        eng = make(family, missing_solver="mu", missing_sweeps_h=1, missing_sweeps_w=1, l1_w=0.0, l2_h=0.0)
    else:
        eng = make(family)
    eng.upload(V2)
    eng.set_factors(W1, H1)
    eng.iterate(2, error_every=1)
    if action == "g":
        eng.set_missing_solver("cd", CD["missing_sweeps_h"], CD["missing_sweeps_w"], l1_w=CD["l1_w"], l2_h=CD["l2_h"])
    enter(eng, action, V, W0, H0)
    got = three_iterations(eng)
    eng.close()
    assert not same_bits(got[0], W1)
    assert_same_run(got, want, f"{family} ({action})")
