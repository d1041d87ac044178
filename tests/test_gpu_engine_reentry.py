"""An engine that is re-entered equals a fresh one: after an engine has iterated on one problem -- so that it holds pending column scales, valid split and bf16
images, Gram matrices marked ready, products enqueued ahead and online accumulators -- a new V and new factors from outside must leave nothing of the old state
behind.  Every family of iteration is run on a used engine after one re-entry action and compared bit for bit (W, H and the error of three iterations) with an
engine that never held the old state.  A flag of Engine's PanelState (csrc/engine_state.h) that a transition forgets shows here as a stale image.

m = 130, n = 257 (padded to 256 x 384) as in test_gpu_device_io.py: every tile loop has a partial tile.  geometry() is asserted so that each case is the family it
claims to be."""
import numpy as np
import pytest

import nmfgpu_amd as na
from tests.test_gpu_device_io import F, assert_same_run, on_device, same_bits

pytestmark = pytest.mark.gpu

M, N = 130, 257
SEED = 12345
KL = dict(divergence="kl", dense_compute=True)
IS = dict(divergence="is")
B05 = dict(divergence="beta", beta=0.5)

# name: (algorithm, dtype, r, keyword arguments of Engine, kind of V, product_kernel, fused_launches, (m, n))
FAMILIES = {
    "mu64_native": ("mu", np.float32, 5, {}, "dense", 0, 0),
    "mu64_split_gram": ("mu", np.float32, 40, {}, "dense", 2, 4),
    "wide_fp32_fused": ("mu", np.float32, 70, {}, "dense", 2, 6),
    "fp64_fused_r5": ("mu", np.float64, 5, {}, "dense", 3, 4),
    "fp64_fused_r70": ("mu", np.float64, 70, {}, "dense", 3, 4),
    "nsnmf_f32_r40": ("nsnmf", np.float32, 40, dict(theta=0.3), "dense", 2, 4),
    "nsnmf_f64_r5": ("nsnmf", np.float64, 5, dict(theta=0.3), "dense", 3, 4),
    "gdcls": ("gdcls", np.float32, 5, {}, "dense", 0, 0),
    "als": ("als", np.float32, 5, {}, "dense", 0, 0),
    "bf16": ("mu", np.float32, 5, dict(precision="bf16"), "dense", 1, 0),
    "bf16_rank256": ("mu", np.float32, 130, dict(precision="bf16"), "dense", 1, 0, (260, 257)),
    "hals": ("hals", np.float32, 5, {}, "dense", 0, 0),
    "nenmf": ("nenmf", np.float32, 5, {}, "dense", 0, 0),
    "hals_tolerance": ("hals", np.float32, 5, dict(sweeps_h=3, sweeps_w=3, sweep_tolerance=0.1), "dense", 0, 0),
    "nenmf_tolerance": ("nenmf", np.float32, 5, dict(steps_h=4, steps_w=4, step_tolerance=0.1), "dense", 0, 0),
    "sparse_kl": ("mu", np.float32, 5, dict(divergence="kl"), "zeros", 5, 0),
    "masked": ("mu", np.float32, 5, dict(missing_values=True), "nan", 5, 0),
    "sparse_compute": ("mu", np.float32, 5, dict(sparse_compute=True), "zeros", 5, 0),
    "dense_kl": ("mu", np.float32, 5, KL, "dense", 6, 0),
    "dense_is": ("mu", np.float32, 5, IS, "dense", 6, 0),
    "dense_beta05": ("mu", np.float32, 5, B05, "dense", 6, 0),
    "dense_beta05_minibatch": ("mu", np.float32, 5, dict(batch_size=128, **B05), "dense", 6, 0),
    "dense_beta05_mixed": ("mu", np.float32, 5, dict(mixed_precision=True, **B05), "dense", 7, 0),
    "dense_beta05_weighted": ("mu", np.float32, 5, dict(weighted=True, **B05), "weighted", 6, 0),
}
# (a) V, then both factors in one call; (b) W and H in two calls, W first; (c) H first; (d) as (a) through the device entries; (e) V, then randomize;
# (f) V, then randomize W alone and set H
ACTIONS = ("a", "b", "c", "d", "e", "f")
_problems, _references = {}, {}


def problem(family):
    """(V, weights or None, W0, H0) and the same with other values for the run that uses the engine first; built once per family and never written.
    "zeros": a third of the entries are 0 (not stored), at other places in the second problem, so that the sparse images change their size;
    "nan": a tenth of the entries are missing."""
    if family not in _problems:
        _, dtype, r, _, kind, _, _, *shape = FAMILIES[family]
        m, n = shape[0] if shape else (M, N)
        both = []
        for seed in (7, 8):
            rng = np.random.default_rng(seed)
            V = (rng.random((m, n)) + 0.1).astype(dtype)
            W = F((1.0 - rng.random((m, r))).astype(dtype))
            H = F((1.0 - rng.random((r, n))).astype(dtype))
            Om = None
            if kind == "zeros":
                V[rng.random((m, n)) < 1 / 3] = 0
            elif kind == "nan":
                V[rng.random((m, n)) < 0.1] = np.nan
            elif kind == "weighted":
                Om = (rng.random((m, n)) * 2).astype(dtype)
                Om[rng.random((m, n)) < 1 / 3] = 0
                Om = F(Om)
            V = F(V)
            for a in (V, Om, W, H):
                if a is not None:
                    a.setflags(write=False)
            both.append((V, Om, W, H))
        assert not same_bits(both[0][0], both[1][0])
        _problems[family] = both
    return _problems[family]


def make(family):
    algorithm, dtype, r, kw, _, _, _, *shape = FAMILIES[family]
    m, n = shape[0] if shape else (M, N)
    return na.Engine(m, n, r, algorithm, dtype=dtype, **kw)


def upload(eng, V, Om):
    eng.upload(V) if Om is None else eng.upload(V, weights=Om)


def check_family(eng, family):
    _, _, _, kw, kind, kernel, launches, *_ = FAMILIES[family]
    g = eng.geometry()
    sparse = kind in ("zeros", "nan")
    assert (g["product_kernel"], g["fused_launches"], g["sparse_setup"]) == (kernel, launches, 0 if sparse else -1), (family, g)
    assert (g["padded_m"], g["padded_n"]) == (256 if g["m"] == 130 else 384, 384)
    assert g["padded_rank"] == (256 if family == "bf16_rank256" else 128 if FAMILIES[family][2] == 70 else 64)


def enter(eng, action, V, Om, W0, H0):
    """the re-entry action (on a fresh engine: its plain counterpart)"""
    if action == "d":
        g = eng.geometry()
        if g["sparse_setup"] != -1 or g["product_kernel"] == 5:      # (sparse engines refuse the device upload: only their factors go through the device form)
            upload(eng, V, Om)
        elif Om is None:
            eng.upload_device(on_device(np.asarray(V), "rm_gap")[0])
        else:
            eng.upload_device(on_device(np.asarray(V), "rm_gap")[0], weights=on_device(np.asarray(Om), "cm_gap")[0])
        eng.set_factors_device(on_device(np.asarray(W0), "cm_gap")[0], on_device(np.asarray(H0), "rm_gap")[0])
        return
    upload(eng, V, Om)
    if action == "a":
        eng.set_factors(W0, H0)
    elif action == "b":
        eng.set_factors(W0, None)
        eng.set_factors(None, H0)
    elif action == "c":
        eng.set_factors(None, H0)
        eng.set_factors(W0, None)
    elif action == "e":
        eng.randomize(SEED)
    elif action == "f":
        eng.randomize(SEED, w=True, h=False)
        eng.set_factors(None, H0)
    else:
        raise ValueError(action)


def three_iterations(eng, family):
    eng.iterate(3, error_every=1)
    W, H = eng.get_factors()
    divergence = FAMILIES[family][3].get("divergence") is not None
    return W, H, (eng.divergence_value if divergence else eng.frobenius)


def reference(family, action):
    """the run of an engine that never held another state: (a) ... (d) start from the same factors, so they share one reference"""
    key = (family, action if action in ("e", "f") else "a")
    if key not in _references:
        V, Om, W0, H0 = problem(family)[0]
        eng = make(family)
        enter(eng, key[1], V, Om, W0, H0)
        check_family(eng, family)
        _references[key] = three_iterations(eng, family)
        eng.close()
        for a in _references[key][:2]:
            a.setflags(write=False)
    return _references[key]


@pytest.mark.parametrize("action", ACTIONS)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_reentered_engine_equals_fresh(family, action):
    (V, Om, W0, H0), (V2, Om2, W1, H1) = problem(family)
    want = reference(family, action)
    eng = make(family)
    upload(eng, V2, Om2)
    eng.set_factors(W1, H1)
    eng.iterate(2, error_every=1)
    enter(eng, action, V, Om, W0, H0)
    check_family(eng, family)
    got = three_iterations(eng, family)
    eng.close()
    assert not same_bits(got[0], W1)
    assert_same_run(got, want, f"{family} ({action})")
