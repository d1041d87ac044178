"""The planning step of engine creation (Engine::plan, csrc/engine.cpp) without a device: nmfamd_plan_geometry / engine.plan_geometry take the three device
facts a plan depends on -- CU count, memory-side cache size, free bytes -- as arguments.

tests/golden/engine_plans.json holds Engine.geometry() of engines CREATED on an MI355X before creation was split into its three steps, with the device facts read
just before each creation: the headline configurations at their per-device shapes, narrow column shards, row-block engines, HALS / NeNMF, the dense divergence
engines and a masked engine.  A planning mistake changes the kernel path or the order of partial sums of such a configuration; here it changes a field."""
import json
import os
import subprocess

import numpy as np
import pytest

from nmfgpu_amd import engine as eng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "engine_plans.json")) as _f:
    RECORDED = json.load(_f)

MI355X = dict(num_cus=256, memory_side_cache_bytes=256 << 20, free_bytes=280 << 30)


def _facts(case):
    return {k: case["facts"][k] for k in ("num_cus", "memory_side_cache_bytes", "free_bytes")}


@pytest.mark.parametrize("case", RECORDED, ids=[c["name"] for c in RECORDED])
def test_plan_matches_the_engine_created_on_the_device(case):
    g = eng.plan_geometry(case["m"], case["n"], case["r"], dtype=np.dtype(case["dtype"]), **case["kwargs"], **_facts(case))
    assert g == case["geometry"]


def test_the_recording_covers_the_paths_it_is_there_for():
    """(what the recorded engines ran, so that a re-recording that lost a path is seen)"""
    by = {c["name"]: c["geometry"] for c in RECORDED}
    assert (by["c2_mu"]["product_kernel"], by["c2_mu"]["resident_images"], by["c2_mu"]["gram_k_slices"], by["c2_mu"]["fused_launches"]) == (2, 1, 16, 4)
    assert by["c4_nsnmf_bf16"]["product_kernel"] == 1 and by["c3_sparse_kl"]["product_kernel"] == 5 and by["example_nsnmf_f64"]["product_kernel"] == 3
    assert by["shard_625"]["w_col_split"] == 1 and by["shard_625"]["gram_k_slices"] in (2, 4, 8)
    assert by["row_blocks_8_c2_shard"]["padded_m"] % (128 * 8) == 0
    assert by["beta_is_plain"]["product_kernel"] == 6 and by["beta_is_mixed"]["product_kernel"] == 7 and by["beta_kl_weighted"]["resident_images"] == 4


# ---- expectations that follow from the rules in Engine::plan, not from a recording ----

def test_free_memory_below_three_and_an_eighth_images_keeps_one_image():
    m, n, r = 2000, 1000, 64
    image = 4 * 2048 * 1024                      # fp32, both sides padded to 128: far below the cache window
    bound = 3 * image + image // 8               # two images plus the staging image of the upload, and an eighth
    facts = dict(MI355X)
    assert eng.plan_geometry(m, n, r, **dict(facts, free_bytes=bound))["resident_images"] == 2
    assert eng.plan_geometry(m, n, r, **dict(facts, free_bytes=bound - 1))["resident_images"] == 1
    assert eng.plan_geometry(m, n, r, **dict(facts, free_bytes=0))["resident_images"] == 1


def test_a_cache_size_of_zero_closes_the_cache_window():
    """Config 2's image (207 MB) lies in the window around 256 MiB: one image; without a cache (size 0: unknown) two, and so at a cache of 1 GiB (both fit)."""
    assert eng.plan_geometry(10000, 5000, 64, **MI355X)["resident_images"] == 1
    assert eng.plan_geometry(10000, 5000, 64, **dict(MI355X, memory_side_cache_bytes=0))["resident_images"] == 2
    assert eng.plan_geometry(10000, 5000, 64, **dict(MI355X, memory_side_cache_bytes=1 << 30))["resident_images"] == 2
    # ranks <= 32 take the split-operand product only inside the window
    assert eng.plan_geometry(10000, 5000, 20, **MI355X)["product_kernel"] == 2
    assert eng.plan_geometry(10000, 5000, 20, **dict(MI355X, memory_side_cache_bytes=0))["product_kernel"] == 0


@pytest.mark.parametrize("value,images", [("0", 2), ("1", 1)])
def test_one_image_switch_forces_the_choice(monkeypatch, value, images):
    monkeypatch.setenv("NMFAMD_ONE_IMAGE", value)
    assert eng.plan_geometry(10000, 5000, 64, **MI355X)["resident_images"] == images      # (inside the window)
    assert eng.plan_geometry(2000, 1000, 64, **MI355X)["resident_images"] == images       # (outside it)
    assert eng.plan_geometry(2000, 1000, 64, **dict(MI355X, free_bytes=0))["resident_images"] == images


def test_force_valu_selects_the_valu_product(monkeypatch):
    monkeypatch.setenv("NMFAMD_FORCE_VALU", "1")
    for dtype in (np.float32, np.float64):
        g = eng.plan_geometry(300, 200, 20, dtype=dtype, **MI355X)
        assert g["product_kernel"] == 4 and g["slabs_h"] == 1 and g["slabs_w"] == 1 and g["fused_launches"] == 0


def test_no_fused_mu_selects_the_generic_launch_sequence(monkeypatch):
    shapes = [(300, 200, 64, np.float32), (300, 200, 130, np.float32), (300, 200, 20, np.float64)]
    assert [eng.plan_geometry(m, n, r, dtype=dt, **MI355X)["fused_launches"] > 0 for m, n, r, dt in shapes] == [True] * 3
    monkeypatch.setenv("NMFAMD_NO_FUSED_MU", "1")
    assert [eng.plan_geometry(m, n, r, dtype=dt, **MI355X)["fused_launches"] for m, n, r, dt in shapes] == [0] * 3


def test_upload_dependent_fields_are_those_of_a_fresh_engine():
    g = eng.plan_geometry(1000, 800, 8, divergence="kl", sparse_compute=True, **MI355X)
    assert (g["product_kernel"], g["resident_images"], g["kl_blocks_w"], g["kl_blocks_h"], g["sparse_setup"]) == (5, 0, 1, 1, 0)
    assert eng.plan_geometry(1000, 800, 8, **MI355X)["sparse_setup"] == -1


REFUSALS = [
    # (every refusal of Engine::check_parameters and Engine::plan that the parameters of nmfamd_engine_create_v2 can reach, with its message)
    (dict(m=0), ""),
    (dict(algorithm="hals", r=600), "HALS: no sweep kernel for this padded rank (fp32: 64 ... 512, fp64: multiples of 64 up to 512)"),
    (dict(algorithm="nenmf", r=129), "NeNMF: no step kernel for this padded rank (supported ranks: 1 ... 128, in either precision)"),
    (dict(dense_compute=True), "dense divergence update: 'denseCompute' selects the dense form of a divergence ('divergence' = 1 or 2), not the Frobenius objective"),
    (dict(divergence="is", algorithm="nsnmf"), "dense divergence update: the Multiplicative algorithm only"),
    (dict(divergence="is", sparse_compute=True), "dense divergence update: does not combine with 'sparseCompute' or 'missingValues' (V is kept dense; a divergence with beta <= 0 is undefined at 0)"),
    (dict(divergence="is", precision="bf16"), "dense divergence update: no bf16 operands"),
    (dict(divergence="is", r=257), "dense divergence update: rank <= 256"),
    (dict(divergence="is", row_blocks=2), "dense divergence update: single GPU only (no row blocks)"),
    (dict(divergence="beta", beta=float("inf")), "dense divergence update: 'beta' has to be finite"),
    (dict(divergence="beta", beta=1e300), "dense divergence update: 'beta' out of the range of the engine's precision"),
    (dict(weighted=True), "weighted NMF: only on a dense divergence engine ('divergence' = 2 or 3, or 1 with 'denseCompute')"),
    (dict(mixed_precision=True), "mixed precision: only on a dense divergence engine ('divergence' = 2 or 3, or 1 with 'denseCompute')"),
    (dict(divergence="is", mixed_precision=True, dtype=np.float64), "mixed precision: single-precision engines only"),
    (dict(divergence="is", mixed_precision=True, weighted=True), "mixed precision: does not combine with 'weighted' (the weighted kernels have no bf16 form)"),
    (dict(batch_size=128, forget_factor=2.0), "minibatch update: 'forgetFactor' has to be a finite value in [0, 1]"),
    (dict(divergence="is", batch_size=100), "minibatch update: 'batchSize' has to be a positive multiple of 128 (the padding unit of the panels, which covers every kernel's reduction tile)"),
    (dict(batch_size=128), "minibatch update: only on a dense divergence engine ('divergence' = 2 or 3, or 1 with 'denseCompute')"),
    (dict(divergence="is", batch_size=128, weighted=True), "minibatch update: does not combine with 'weighted' (the accumulating update has no weighted form)"),
    (dict(missing_values=True, divergence="kl"), "missing values: multiplicative update with the Frobenius objective, rank <= 256"),
    (dict(missing_values=True, algorithm="nsnmf"), "missing values: multiplicative update with the Frobenius objective, rank <= 256"),
    (dict(missing_values=True, r=300), "missing values: multiplicative update with the Frobenius objective, rank <= 256"),
    (dict(algorithm="hals", sparse_compute=True, divergence="kl"), "HALS: sparse compute with the Frobenius objective only (no 'divergence', no missing values)"),
    (dict(algorithm="gdcls", sparse_compute=True), "sparse compute: multiplicative update and HALS only"),
    (dict(sparse_compute=True, r=300), "sparse compute needs rank <= 256 (the SpMM kernels gather 1, 2 or 4 values per lane)"),
    (dict(precision="bf16", dtype=np.float64), ""),
    (dict(precision="bf16", sparse_compute=True), ""),
]


@pytest.mark.parametrize("change,message", REFUSALS, ids=[" ".join(f"{k}={getattr(v, '__name__', v)}" for k, v in c.items()) for c, _ in REFUSALS])
def test_refusals_keep_their_messages(change, message):
    args = dict(dict(m=300, n=200, r=8), **change)
    with pytest.raises(eng.EngineError) as err:
        eng.plan_geometry(args.pop("m"), args.pop("n"), args.pop("r"), **args, **MI355X)
    assert err.value.status == 1
    assert str(err.value) == "nmfamd_plan_geometry: invalid argument" + (f" ({message})" if message else "")


def test_forget_factor_without_a_batch_size_is_refused_at_the_c_interface():
    """(Engine.__init__ and plan_geometry drop forget_factor when there is no batch_size: this refusal is reached through the struct only)"""
    import ctypes as C
    p = eng._params_struct([0.0] * 15 + [0.5])
    g = eng._Geometry()
    lib = eng.library()
    st = lib.nmfamd_plan_geometry(300, 200, 8, 0, C.byref(p), C.c_ulong(C.sizeof(p)), 4, 1, 256, C.c_ulonglong(0), C.c_ulonglong(0), C.byref(g), C.c_ulong(C.sizeof(g)))
    lib.nmfamd_engine_last_error.restype = C.c_char_p
    assert st == 1 and lib.nmfamd_engine_last_error(None) == b"minibatch update: 'forgetFactor' needs a 'batchSize'"
    # ... and the arguments of the entry itself
    assert lib.nmfamd_plan_geometry(300, 200, 8, 0, None, C.c_ulong(0), 2, 1, 256, C.c_ulonglong(0), C.c_ulonglong(0), C.byref(g), C.c_ulong(C.sizeof(g))) == 1
    assert lib.nmfamd_plan_geometry(300, 200, 8, 0, None, C.c_ulong(0), 4, 1, 256, C.c_ulonglong(0), C.c_ulonglong(0), None, C.c_ulong(C.sizeof(g))) == 1
    assert lib.nmfamd_plan_geometry(300, 200, 8, 0, None, C.c_ulong(0), 4, 1, 256, C.c_ulonglong(0), C.c_ulonglong(0), C.byref(g), C.c_ulong(C.sizeof(g))) == 0
    assert (g.m, g.n, g.r, g.padded_rank, g.padded_m, g.padded_n) == (300, 200, 8, 64, 384, 256)


# ---- the owner of the engine's memory under AddressSanitizer + UBSan, on the host ----

def test_buffer_owner_under_sanitizers(tmp_path):
    """csrc/device_buffers.h with the HIP allocation functions defined by the driver on malloc / free (tests/cpp/device_buffers_sanitize.cpp): allocate, release,
    re-allocate, adoption and destruction with live buffers, with no leak and no double free."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = tmp_path / "owner_san"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include",
           os.path.join(ROOT, "tests", "cpp", "device_buffers_sanitize.cpp"), "-o", str(exe)]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr
    assert run.stdout.strip().endswith("ok")


# ---- on the device: the engine agrees with its planner ----

def _device_facts():
    import torch
    p = torch.cuda.get_device_properties(0)
    mall = (256 << 20) if p.gcnArchName[:6] in ("gfx942", "gfx950") else 0
    if os.environ.get("NMFAMD_MALL_MB"):
        mall = max(int(os.environ["NMFAMD_MALL_MB"]), 0) << 20
    return dict(num_cus=int(p.multi_processor_count), memory_side_cache_bytes=mall, free_bytes=int(torch.cuda.mem_get_info()[0]))


ON_DEVICE = [
    dict(r=5), dict(r=64), dict(r=130), dict(r=20, dtype=np.float64), dict(r=256, algorithm="nsnmf", precision="bf16", theta=0.5),
    dict(r=8, divergence="kl", sparse_compute=True), dict(r=8, algorithm="hals"), dict(r=8, algorithm="nenmf"), dict(r=8, divergence="is"),
    dict(r=8, divergence="is", batch_size=128),
]


@pytest.mark.gpu
@pytest.mark.parametrize("kw", ON_DEVICE, ids=[" ".join(f"{k}={getattr(v, '__name__', v)}" for k, v in kw.items()) for kw in ON_DEVICE])
def test_engine_agrees_with_its_planner(kw):
    """Creation only, at the smallest shapes that reach each branch of Engine::plan."""
    facts = _device_facts()
    e = eng.Engine(300, 200, **kw)
    try:
        assert e.geometry() == eng.plan_geometry(300, 200, **kw, **facts)
    finally:
        e.close()
