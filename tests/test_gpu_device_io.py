"""Device-resident input and output on the GPU (docs/DEVICE_IO.md): an engine fed by upload_device / set_factors_device from torch tensors against one fed by
upload / set_factors from the same numpy values, bit for bit (np.array_equal) -- the images, the tr(V^T V) terms, the factors and the error after three
iterations -- in every input form (column-major and row-major, with and without a leading-dimension gap, and a pointer no 16-byte load is aligned for), the value
rules with the host upload's statuses and texts, the weighted upload, the factor panels in both directions, and the refusals that run no kernel.

m = 130 = 2 * 64 + 2 and n = 257 = 4 * 64 + 1 leave a ragged tile on both sides (padded to 256 and 384); r = 5 has padded rank 64 and r = 70 padded rank 128.
The one quantity that is not bit-identical is the sum of the weights behind rmsd() of a weighted engine: both paths add the same m n non-negative doubles, in
another order, and two orders of k non-negative terms differ by at most k 2^-53 relative to the sum (each of the k - 1 additions rounds by at most 2^-53 of a
partial sum that never exceeds the total); rmsd divides by its root, which halves the bound, so m n 2^-53 holds with room."""
import ctypes as C

import numpy as np
import pytest

import nmfgpu_amd as na

pytestmark = pytest.mark.gpu

M, N = 130, 257
FORMS = ("cm", "cm_gap", "rm", "rm_gap", "rm_off1")
DIVERGENCES = {1.0: dict(divergence="kl", dense_compute=True), 0.0: dict(divergence="is"), 0.5: dict(divergence="beta", beta=0.5)}
_cache = {}


def torch_():
    import torch
    assert torch.cuda.is_available()
    return torch


def F(a):
    return np.asfortranarray(a)


def problem(dtype, r, seed=7):
    """V in [0.1, 1.1) (every value rule holds), W0, H0 in (0, 1]; built once per (dtype, r) and never written."""
    key = (np.dtype(dtype).name, r, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        V = F((rng.random((M, N)) + 0.1).astype(dtype))
        W0 = F((1.0 - rng.random((M, r))).astype(dtype))
        H0 = F((1.0 - rng.random((r, N))).astype(dtype))
        for a in (V, W0, H0):
            a.setflags(write=False)
        _cache[key] = (V, W0, H0)
    return _cache[key]


def on_device(A, form):
    """(view, base): A (numpy, rows x cols) as a device tensor view of that shape in the given form, and the buffer it is a view of.  Gaps hold NaN."""
    torch = torch_()
    rows, cols = A.shape
    t = torch.from_numpy(np.ascontiguousarray(A))
    if form == "cm":
        base = t.T.contiguous().cuda()                       # (cols, rows) contiguous: its .T is column-major with ld = rows
        view = base.T
    elif form == "cm_gap":
        base = torch.full((cols, rows + 3), float("nan"), dtype=t.dtype, device="cuda")
        base[:, :rows] = t.T.cuda()
        view = base[:, :rows].T                              # ld = rows + 3
    elif form == "rm":
        base = t.cuda()
        view = base
    elif form == "rm_gap":
        base = torch.full((rows, cols + 5), float("nan"), dtype=t.dtype, device="cuda")
        base[:, :cols] = t.cuda()
        view = base[:, :cols]                                # ld = cols + 5
    elif form == "rm_off1":
        base = torch.full((rows * cols + 1,), float("nan"), dtype=t.dtype, device="cuda")
        base[1:] = t.cuda().reshape(-1)
        view = base[1:].view(rows, cols)                     # starts one element into its buffer
        assert view.data_ptr() % 16 != 0
    else:
        raise ValueError(form)
    assert tuple(view.shape) == (rows, cols)
    torch.cuda.synchronize()
    return view, base


def same_bits(a, b):
    """np.array_equal on the bit patterns (so that NaN equals NaN and -0 differs from 0)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def feed_device(eng, V, form, weights=None, wform=None):
    """upload_device from a tensor in the given form; the source must compare equal to a clone taken before the call."""
    torch = torch_()
    view, base = on_device(V, form)
    before = base.clone()
    if weights is None:
        eng.upload_device(view)
    else:
        wview, wbase = on_device(weights, wform or form)
        wbefore = wbase.clone()
        eng.upload_device(view, weights=wview)
        assert same_bits(wbase.cpu().numpy(), wbefore.cpu().numpy())
    torch.cuda.synchronize()
    assert same_bits(base.cpu().numpy(), before.cpu().numpy())


def after_iterations(eng, W0, H0, count=3, divergence=False):
    eng.set_factors(W0, H0)
    eng.iterate(count, error_every=1)
    W, H = eng.get_factors()
    return W, H, (eng.divergence_value if divergence else eng.frobenius)


def assert_same_run(a, b, what):
    assert same_bits(a[0], b[0]), f"{what}: W differs"
    assert same_bits(a[1], b[1]), f"{what}: H differs"
    assert a[2] == b[2] and np.isfinite(a[2]), f"{what}: error {a[2]!r} against {b[2]!r}"


# ---- images and terms ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype, precision, r", [(np.float32, "native", 70), (np.float32, "native", 5), (np.float32, "fp32_mfma", 5), (np.float32, "bf16", 5),
                                                 (np.float64, "native", 5), (np.float64, "fp32_mfma", 5)])
def test_images_and_terms(dtype, precision, r, form):
    """precision "native" is the default: the split-operand product where the plan chooses it (here at r = 70: product_kernel 2), else the native instructions;
    "fp32_mfma" is nmfamd_params.precision = -1."""
    V, W0, H0 = problem(dtype, r)
    host = na.Engine(M, N, r, "mu", dtype=dtype, precision=precision)
    dev = na.Engine(M, N, r, "mu", dtype=dtype, precision=precision)
    host.upload(V)
    feed_device(dev, V, form)
    assert host.geometry() == dev.geometry()
    assert host.geometry()["product_kernel"] == {("float32", "native", 70): 2, ("float32", "bf16", 5): 1, ("float64", "native", 5): 3, ("float64", "fp32_mfma", 5): 3}.get(
        (np.dtype(dtype).name, precision, r), 0)
    assert same_bits(host.error_terms(0), dev.error_terms(0))
    if precision != "bf16":
        g = host.geometry()
        count = g["padded_m"] * g["padded_n"]
        for which in (6, 7):
            assert same_bits(host.debug_read(which, count), dev.debug_read(which, count)), f"image {which}"
    assert_same_run(after_iterations(dev, W0, H0), after_iterations(host, W0, H0), f"{np.dtype(dtype).name} {precision} {form}")
    host.close()
    dev.close()


@pytest.mark.parametrize("algorithm, r", [("hals", 5), ("nenmf", 5), ("nsnmf", 5), ("mu", 70)])
def test_one_algorithm_of_each_family(algorithm, r):
    V, W0, H0 = problem(np.float32, r)
    kw = dict(theta=0.3) if algorithm == "nsnmf" else {}
    runs = []
    for device in (False, True):
        eng = na.Engine(M, N, r, algorithm, **kw)
        feed_device(eng, V, "rm_gap") if device else eng.upload(V)
        runs.append(after_iterations(eng, W0, H0))
        eng.close()
    assert_same_run(runs[1], runs[0], f"{algorithm} r = {r}")


@pytest.mark.parametrize("batch", [None, 128])
@pytest.mark.parametrize("beta", [1.0, 0.0, 0.5])
def test_dense_divergence_engines(beta, batch):
    r = 5
    V, W0, H0 = problem(np.float32, r)
    runs = []
    for device in (False, True):
        eng = na.Engine(M, N, r, "mu", batch_size=batch, **DIVERGENCES[beta])
        feed_device(eng, V, "rm_gap") if device else eng.upload(V)
        runs.append(after_iterations(eng, W0, H0, divergence=True))
        eng.close()
    assert_same_run(runs[1], runs[0], f"beta {beta} batch {batch}")


# ---- value rules ------------------------------------------------------------------------------------------------------------------------------------

def refusal(call):
    """(status, the message without the name of the entry in front: the status text and last_error)"""
    with pytest.raises(na.EngineError) as e:
        call()
    return e.value.status, str(e.value).split(": ", 1)[1]


@pytest.mark.parametrize("beta, bad", [(1.0, np.nan), (1.0, np.inf), (1.0, -1.0), (0.0, 0.0)])
@pytest.mark.parametrize("form", ["cm_gap", "rm_off1"])
def test_value_rules(beta, bad, form):
    r = 5
    V, W0, H0 = problem(np.float32, r)
    Vb = V.copy(order="F")
    Vb[M - 1, N - 1] = bad      # the ragged corner
    host = na.Engine(M, N, r, "mu", **DIVERGENCES[beta])
    dev = na.Engine(M, N, r, "mu", **DIVERGENCES[beta])
    want = refusal(lambda: host.upload(Vb))
    got = refusal(lambda: feed_device(dev, Vb, form))
    assert want[0] == 1 and want == got and "(" in got[1], (want, got)
    for eng in (host, dev):
        eng.set_factors(W0, H0)
    assert refusal(lambda: host.iterate(1)) == refusal(lambda: dev.iterate(1))
    host.upload(V)
    feed_device(dev, V, form)
    assert_same_run(after_iterations(dev, W0, H0, divergence=True), after_iterations(host, W0, H0, divergence=True), "after the refusal")
    host.close()
    dev.close()


def test_value_range():
    r = 70      # (at this shape the default precision runs the split-operand product from padded rank 64 on; r = 5 stays on the native instructions)
    V, W0, H0 = problem(np.float32, r)
    Vs = V.copy(order="F")
    Vs[M - 1, N - 1] = 1e-41      # below 2^-100: outside the exact range of the split-operand product
    lib = na.library()
    h = C.c_void_p()
    assert lib.nmfamd_engine_create(M, N, r, 0, None, 4, None, C.byref(h)) == 0
    raw = na.Engine.from_handle(h, M, N, r, np.float32)
    assert raw.geometry()["product_kernel"] == 2
    view, _ = on_device(Vs, "rm_gap")
    vp, ld, layout = na.device_matrix(view, (M, N), np.float32)
    assert lib.nmfamd_engine_upload_dense_device(h, C.c_void_p(vp), C.c_long(ld), layout) == 6
    assert refusal(lambda: raw.upload_device(view))[0] == 6      # (an engine from a handle is never recreated)
    raw.close()
    host = na.Engine(M, N, r, "mu")
    dev = na.Engine(M, N, r, "mu")
    host.upload(Vs)
    feed_device(dev, Vs, "rm_gap")
    assert host.geometry()["product_kernel"] == dev.geometry()["product_kernel"] == 0      # both recreated on the native fp32 instructions
    assert_same_run(after_iterations(dev, W0, H0), after_iterations(host, W0, H0), "value range")
    host.close()
    dev.close()


# ---- weighted ---------------------------------------------------------------------------------------------------------------------------------------

def weights_of(dtype, seed=11):
    rng = np.random.default_rng(seed)
    Om = (rng.random((M, N)) * 2).astype(dtype)
    Om[rng.random((M, N)) < 1 / 3] = 0
    Om[M - 1, N - 1] = 0.5
    return F(Om)


@pytest.mark.parametrize("form, wform", [("cm", "cm"), ("rm_gap", "cm_gap"), ("cm_gap", "rm_off1"), ("rm_off1", "rm")])
def test_weighted(form, wform):
    r = 5
    V, W0, H0 = problem(np.float32, r)
    Om = weights_of(np.float32)
    Vn = V.copy()
    zeros = np.argwhere(Om == 0)
    Vn[tuple(zeros[::3].T)] = np.nan      # NaN under some of the zero weights
    assert np.isnan(Vn).sum() > 1000 and abs((Om == 0).mean() - 1 / 3) < 0.03
    host = na.Engine(M, N, r, "mu", weighted=True, **DIVERGENCES[0.5])
    host.upload(F(Vn), weights=Om)
    want = after_iterations(host, W0, H0, divergence=True)
    want_rmsd = host.rmsd
    rmsds = []
    for _ in range(2):
        dev = na.Engine(M, N, r, "mu", weighted=True, **DIVERGENCES[0.5])
        feed_device(dev, Vn, form, Om, wform)
        assert_same_run(after_iterations(dev, W0, H0, divergence=True), want, f"weighted {form} / {wform}")
        rmsds.append(dev.rmsd)
        dev.close()
    print(f"rmsd host {want_rmsd!r} device {rmsds[0]!r} relative difference {abs(rmsds[0] / want_rmsd - 1):.3e} bound {M * N * 2.0 ** -53:.3e}")
    assert rmsds[0] == rmsds[1]
    assert want_rmsd > 0 and abs(rmsds[0] / want_rmsd - 1) <= M * N * 2.0 ** -53
    host.close()


def test_weighted_refusals():
    r = 5
    V, W0, H0 = problem(np.float32, r)
    Om = weights_of(np.float32)
    neg, nan, none = Om.copy(), Om.copy(), np.zeros_like(Om)
    neg[M - 1, N - 1] = -1.0
    nan[M - 1, N - 1] = np.nan
    Vz = V.copy()
    Vz[M - 1, N - 1] = 0.0      # under the weight 0.5
    for beta, Vx, Ox in ((0.5, V, neg), (0.5, V, nan), (0.5, V, none), (0.0, Vz, Om)):
        host = na.Engine(M, N, r, "mu", weighted=True, **DIVERGENCES[beta])
        dev = na.Engine(M, N, r, "mu", weighted=True, **DIVERGENCES[beta])
        want = refusal(lambda: host.upload(F(Vx), weights=F(Ox)))
        got = refusal(lambda: feed_device(dev, Vx, "rm_gap", Ox, "cm_gap"))
        assert want[0] == 1 and want == got and "(" in got[1], (want, got)
        host.close()
        dev.close()
    weighted = na.Engine(M, N, r, "mu", weighted=True, **DIVERGENCES[0.5])
    plain = na.Engine(M, N, r, "mu", **DIVERGENCES[0.5])
    host_w, host_p = refusal(lambda: weighted.upload(V)), refusal(lambda: plain.upload(V, weights=Om))
    got_w, got_p = refusal(lambda: feed_device(weighted, V, "rm")), refusal(lambda: feed_device(plain, V, "rm", Om, "rm"))
    assert got_w == host_w and got_w[0] == 1 and "(" in got_w[1]
    assert got_p == host_p and got_p[0] == 1 and "(" in got_p[1]
    weighted.close()
    plain.close()


# ---- factors ----------------------------------------------------------------------------------------------------------------------------------------

LAYOUTS = [("cm_gap", "cm_gap"), ("cm_gap", "rm_gap"), ("rm_gap", "cm_gap"), ("rm_gap", "rm_gap")]


@pytest.mark.parametrize("r", [5, 70])
@pytest.mark.parametrize("wform, hform", LAYOUTS)
def test_set_factors_device(r, wform, hform):
    V, W0, H0 = problem(np.float32, r)
    host = na.Engine(M, N, r, "mu")
    dev = na.Engine(M, N, r, "mu")
    host.set_factors(W0, H0)
    (wv, wb), (hv, hb) = on_device(W0, wform), on_device(H0, hform)
    before = wb.clone(), hb.clone()
    dev.set_factors_device(wv, hv)
    assert same_bits(wb.cpu().numpy(), before[0].cpu().numpy()) and same_bits(hb.cpu().numpy(), before[1].cpu().numpy())
    W, H = dev.get_factors()
    assert same_bits(W, W0) and same_bits(H, H0)
    g = dev.geometry()
    for which, count in ((0, g["padded_rank"] * g["padded_m"]), (1, g["padded_rank"] * g["padded_n"])):
        panel = dev.debug_read(which, count)
        assert same_bits(panel, host.debug_read(which, count)), f"panel {which}"
        P = panel.reshape(-1, g["padded_rank"])
        length = M if which == 0 else N
        assert np.all(P[:, r:] == 0) and np.all(P[length:] == 0) and np.all(P[:length, :r] > 0)
    host.close()
    dev.close()


@pytest.mark.parametrize("r", [5, 70])
@pytest.mark.parametrize("wform, hform", LAYOUTS)
def test_get_factors_device(r, wform, hform):
    torch = torch_()
    V, W0, H0 = problem(np.float32, r)
    eng = na.Engine(M, N, r, "mu")
    eng.set_factors(W0, H0)
    W, H = eng.get_factors()
    (wv, wb), (hv, hb) = on_device(np.full((M, r), np.nan, np.float32), wform), on_device(np.full((r, N), np.nan, np.float32), hform)
    eng.get_factors_device(wv, hv)
    torch.cuda.synchronize()
    assert same_bits(wv.cpu().numpy(), W) and same_bits(hv.cpu().numpy(), H)
    # every element outside the block is still NaN: the count of numbers in the buffer is the block's
    assert int((~torch.isnan(wb)).sum()) == M * r and int((~torch.isnan(hb)).sum()) == r * N
    eng.close()


def test_none_for_either_factor():
    torch = torch_()
    r = 5
    V, W0, H0 = problem(np.float32, r)
    W1, H1 = F(W0 * 0.5), F(H0 * 0.25)
    eng = na.Engine(M, N, r, "mu")
    eng.set_factors(W0, H0)
    eng.set_factors_device(on_device(W1, "rm")[0], None)
    W, H = eng.get_factors()
    assert same_bits(W, W1) and same_bits(H, H0)
    eng.set_factors_device(None, on_device(H1, "cm")[0])
    W, H = eng.get_factors()
    assert same_bits(W, W1) and same_bits(H, H1)
    wv, wb = on_device(np.full((M, r), np.nan, np.float32), "rm")
    hv, hb = on_device(np.full((r, N), np.nan, np.float32), "rm")
    eng.get_factors_device(wv, None)
    eng.get_factors_device(None, None)
    torch.cuda.synchronize()
    assert same_bits(wv.cpu().numpy(), W1) and bool(torch.isnan(hb).all())
    eng.get_factors_device(None, hv)
    assert same_bits(hv.cpu().numpy(), H1)
    eng.close()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_nsnmf_returns_w_s(dtype):
    r = 5
    V, W0, H0 = problem(dtype, r)
    eng = na.Engine(M, N, r, "nsnmf", dtype=dtype, theta=0.3)
    eng.upload(V)
    eng.set_factors(W0, H0)
    eng.iterate(2, error_every=0)
    W, H = eng.get_factors()
    assert not same_bits(W, W0)
    wv, _ = on_device(np.full((M, r), np.nan, dtype), "cm_gap")
    hv, _ = on_device(np.full((r, N), np.nan, dtype), "rm_gap")
    eng.get_factors_device(wv, hv)
    assert same_bits(wv.cpu().numpy(), W) and same_bits(hv.cpu().numpy(), H)
    eng.close()


# ---- refusals that run no kernel ----------------------------------------------------------------------------------------------------------------------

def test_device_pointer_info():
    torch = torch_()
    a = np.zeros(64, np.float32)
    assert na.device_pointer_info(a.ctypes.data) == {"kind": "unknown", "device": -1, "bytes_from_p": 0}
    assert na.device_pointer_info(0)["kind"] == "unknown"
    t = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")
    info = na.device_pointer_info(t.data_ptr())
    assert info["kind"] == "device" and info["device"] == torch.cuda.current_device()
    assert info["bytes_from_p"] >= t.numel() * 4      # (torch carves tensors out of larger blocks: the block's end)
    assert na.device_pointer_info(t.data_ptr() + 4096)["bytes_from_p"] == info["bytes_from_p"] - 4096
    p = torch.zeros(1024, dtype=torch.float32).pin_memory()
    assert na.device_pointer_info(p.data_ptr())["kind"] == "pinned" and na.device_pointer_info(p.data_ptr())["bytes_from_p"] == 0


def test_refusals_that_run_no_kernel():
    torch = torch_()
    r = 5
    V, W0, H0 = problem(np.float32, r)
    eng = na.Engine(M, N, r, "mu")
    eng.upload(V)
    want = after_iterations(eng, W0, H0)
    good = torch.from_numpy(np.ascontiguousarray(V)).cuda()
    pinned = torch.from_numpy(np.ascontiguousarray(V)).pin_memory()
    host = np.ascontiguousarray(V)
    out_w = torch.zeros((M, r), dtype=torch.float32, device="cuda")
    p = good.data_ptr()
    # (every triple is wrong for V and for H alike -- H is r x n, row-major here, so its inner extent is V's)
    bad = {"a null pointer": (0, N, 1), "pinned host memory": (pinned.data_ptr(), N, 1), "host memory": (host.ctypes.data, N, 1), "ld below the columns": (p, N - 1, 1),
           "layout 2": (p, N, 2), "an extent past the allocation": (p, 1 << 40, 1), "a pointer off the element": (p + 2, N, 1)}
    for what, triple in bad.items():
        calls = {"upload_device": lambda: eng.upload_device(triple), "set_factors_device": lambda: eng.set_factors_device(None, triple),
                 "get_factors_device": lambda: eng.get_factors_device(None, triple)}
        for name, call in calls.items():
            if what == "a null pointer" and name != "upload_device":
                continue      # (a null factor means: leave it)
            try:
                call()
            except na.EngineError as e:
                status, text = e.status, str(e)
            else:
                pytest.fail(f"{what} / {name}: not refused")
            assert status == 1 and "(" in text and len(text.split("(", 1)[1]) > 8, f"{what} / {name}: {status} {text}"
    assert "leading dimension" in refusal(lambda: eng.upload_device((p, M - 1, 0)))[1]      # column-major: ld below the rows
    for what, text in (("a null pointer", "null"), ("pinned host memory", "pinned"), ("host memory", "not device memory"), ("layout 2", "layout"),
                       ("ld below the columns", "leading dimension"), ("an extent past the allocation", "allocation"), ("a pointer off the element", "aligned")):
        assert text in refusal(lambda: eng.upload_device(bad[what]))[1], what
    weighted = na.Engine(M, N, r, "mu", weighted=True, **DIVERGENCES[0.5])
    for triple in bad.values():
        assert refusal(lambda: weighted.upload_device((p, N, 1), weights=triple))[0] == 1
        assert refusal(lambda: weighted.upload_device(triple, weights=(p, N, 1)))[0] == 1
    weighted.close()
    for kw in (dict(sparse_compute=True), dict(missing_values=True)):
        other = na.Engine(M, N, r, "mu", **kw)
        status, text = refusal(lambda: other.upload_device(good))
        assert status == 1 and "sparseCompute" in text and "missingValues" in text, text
        other.upload(V)      # (the host entry still serves it)
        other.set_factors(W0, H0)
        other.iterate(1, error_every=1)
        assert np.isfinite(other.frobenius)
        other.close()
    # the engine is as usable as before: the resident V and the factors' state were not touched
    assert_same_run(after_iterations(eng, W0, H0), want, "after the refusals")
    eng.upload_device(good)
    eng.get_factors_device(out_w, None)
    assert_same_run(after_iterations(eng, W0, H0), want, "after a good device upload")
    eng.close()
