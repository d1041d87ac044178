"""Device-resident sparse input on the GPU (docs/DEVICE_IO.md, "Sparse input" and "Dense input on the sparse engines"): an engine fed by upload_sparse_device /
upload_device_stored from torch tensors against a second engine fed through the HOST entry (upload_sparse / upload) with the same values.  Every comparison is
bit for bit (np.array_equal / ==): the CSR and CSC images (debug_read 12 ... 17; the index images are readable on float32 engines only), the dense images of the
densifying engines (6, 7), the tr(V^T V) terms, and the factors and the error after a few iterations; refusals carry the host entry's status and text.

The dense inputs of upload_device_stored hold multiples of 2^-6 below 8: the host adds sum(V) of the KL divergence in one chain of doubles, the device per column
and then across the columns, and with at most 130 * 257 such values (each a multiple of 2^-6, the sum below 2^19) every partial sum is exact in a double either way,
so kl_divergence can be compared with ==, like everything else."""
import numpy as np
import pytest

import nmfgpu_amd as na

pytestmark = pytest.mark.gpu

M, N = 130, 257
FORMS = ("cm", "cm_gap", "rm", "rm_gap", "rm_off1")
_cache = {}


def torch_():
    import torch
    assert torch.cuda.is_available()
    return torch


def F(a):
    return np.asfortranarray(a)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def refusal(call):
    """(status, the message without the name of the entry in front: the status text and last_error)"""
    with pytest.raises(na.EngineError) as e:
        call()
    return e.value.status, str(e.value).split(": ", 1)[1]


def factors(m, n, r, dtype=np.float32, seed=3):
    key = (m, n, r, np.dtype(dtype).name, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        W, H = F((1.0 - rng.random((m, r))).astype(dtype)), F((1.0 - rng.random((r, n))).astype(dtype))
        W.setflags(write=False); H.setflags(write=False)
        _cache[key] = (W, H)
    return _cache[key]


def triplets(m, n, density, seed, duplicates=0, dtype=np.float32):
    rng = np.random.default_rng(seed)
    nnz = max(1, int(m * n * density))
    lin = rng.choice(m * n, size=nnz, replace=False)
    rows, cols = (lin // n).astype(np.int32), (lin % n).astype(np.int32)
    if duplicates:
        d = rng.integers(0, nnz, size=duplicates)
        rows, cols = np.concatenate([rows, rows[d]]), np.concatenate([cols, cols[d]])
    vals = (rng.integers(1, 6, size=len(rows)).astype(np.float32) + rng.random(len(rows)).astype(np.float32)).astype(dtype)
    return rows, cols, vals


def as_format(fmt, rows, cols, vals, m, n, base, order):
    """fmt 1 CSR / 2 CSC / 3 COO arrays (values, a, b) of the same entries; order "sorted" or "unsorted" inside an outer index (COO: row-major order or random)."""
    rng = np.random.default_rng(7)
    if fmt == 3:
        perm = np.lexsort((cols, rows)) if order == "sorted" else rng.permutation(len(vals))
        return vals[perm], (rows[perm] + base).astype(np.int32), (cols[perm] + base).astype(np.int32)
    outer, inner, count = (rows, cols, m) if fmt == 1 else (cols, rows, n)
    tie = inner if order == "sorted" else rng.random(len(vals))
    perm = np.lexsort((tie, outer))
    ptr = np.zeros(count + 1, dtype=np.int64)
    np.add.at(ptr, outer + 1, 1)
    ptr = np.cumsum(ptr)
    return vals[perm], (ptr + base).astype(np.int32), (inner[perm] + base).astype(np.int32)


def feed_sparse_device(eng, fmt, arrays, base):
    """upload_sparse_device from three tensors; every source must compare equal to a clone taken before the call."""
    torch = torch_()
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in arrays]
    before = [t.clone() for t in dev]
    torch.cuda.synchronize()
    eng.upload_sparse_device(fmt, *dev, base)
    torch.cuda.synchronize()
    for t, b in zip(dev, before):
        assert same_bits(t.cpu().numpy(), b.cpu().numpy())


def sparse_images(eng, nnz, m, n):
    out = {12: eng.debug_read(12, nnz), 13: eng.debug_read(13, nnz)}
    if eng.dtype == np.float32:      # (the index images are read as 32-bit words: float32 engines)
        for which, count in ((14, m + 1), (15, nnz), (16, n + 1), (17, nnz)):
            out[which] = eng.debug_read(which, count).view(np.int32)
    return out


def assert_same_images(a, b):
    assert set(a) == set(b)
    for which in b:
        assert same_bits(a[which], b[which]), f"image {which}"


def run(eng, W, H, count, value):
    eng.set_factors(W, H)
    eng.iterate(count, first_iteration=1, error_every=1, last_iteration=count)
    Wg, Hg = eng.get_factors()
    return Wg, Hg, getattr(eng, value)


def assert_same_run(a, b, what=""):
    assert same_bits(a[0], b[0]), f"{what}: W differs"
    assert same_bits(a[1], b[1]), f"{what}: H differs"
    assert a[2] == b[2] and np.isfinite(a[2]), f"{what}: error {a[2]!r} against {b[2]!r}"


# ---- case 1: sparse arrays on the engines that keep V sparse ------------------------------------------------------------------------------------------

def sparse_pair(fmt, base, order, m, n, r, kw, value, dtype=np.float32, algorithm="mu", iters=6, monkeypatch=None):
    monkeypatch.delenv("NMFAMD_SPARSE_SETUP", raising=False)
    rows, cols, vals = triplets(m, n, 0.07, seed=10 * fmt + base, duplicates=40, dtype=dtype)
    arrays = as_format(fmt, rows, cols, vals, m, n, base, order)
    W, H = factors(m, n, r, dtype)
    host = na.Engine(m, n, r, algorithm, dtype=dtype, **kw)
    dev = na.Engine(m, n, r, algorithm, dtype=dtype, **kw)
    host.upload_sparse(fmt, *arrays, base)
    feed_sparse_device(dev, fmt, arrays, base)
    assert host.geometry()["sparse_setup"] == 1 and dev.geometry()["sparse_setup"] == 1
    assert_same_images(sparse_images(dev, len(vals), m, n), sparse_images(host, len(vals), m, n))
    assert same_bits(dev.error_terms(0), host.error_terms(0))
    assert_same_run(run(dev, W, H, iters, value), run(host, W, H, iters, value), f"format {fmt} base {base} {order}")
    host.close()
    dev.close()


@pytest.mark.parametrize("fmt", [1, 2, 3])
@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("order", ["sorted", "unsorted"])
def test_sparse_arrays_on_a_sparse_compute_engine(fmt, base, order, monkeypatch):
    sparse_pair(fmt, base, order, 517, 389, 12, dict(sparse_compute=True), "frobenius", monkeypatch=monkeypatch)


@pytest.mark.parametrize("what, fmt, base, order, kw, value, dtype, algorithm", [
    ("sparse KL", 1, 0, "sorted", dict(sparse_compute=True, divergence="kl"), "kl_divergence", np.float32, "mu"),
    ("missing values", 3, 1, "unsorted", dict(missing_values=True), "rmsd", np.float32, "mu"),
    ("sparse HALS", 2, 0, "sorted", dict(sparse_compute=True), "frobenius", np.float32, "hals"),
    ("float64", 1, 1, "unsorted", dict(sparse_compute=True), "frobenius", np.float64, "mu"),
])
def test_sparse_arrays_on_the_other_sparse_engines(what, fmt, base, order, kw, value, dtype, algorithm, monkeypatch):
    sparse_pair(fmt, base, order, 517, 389, 12, kw, value, dtype, algorithm, monkeypatch=monkeypatch)


# ---- case 2: the densifying engines ---------------------------------------------------------------------------------------------------------------

def dense_image(eng, which):
    g = eng.geometry()
    try:
        return eng.debug_read(which, g["padded_m"] * g["padded_n"])
    except na.EngineError:
        return None      # (an engine that keeps no such image: then neither twin does)


@pytest.mark.parametrize("kw, value", [(dict(), "frobenius"), (dict(divergence="kl", dense_compute=True), "divergence_value")])
@pytest.mark.parametrize("fmt, base, order", [(1, 0, "sorted"), (2, 1, "unsorted"), (3, 1, "unsorted")])
def test_densifying_engines(kw, value, fmt, base, order):
    """Unique coordinates: k_densify adds duplicates atomically, and three or more of them round in an order no two runs share."""
    r = 5
    rows, cols, vals = triplets(M, N, 0.2, seed=21)
    arrays = as_format(fmt, rows, cols, vals, M, N, base, order)
    W, H = factors(M, N, r)
    host = na.Engine(M, N, r, "mu", **kw)
    dev = na.Engine(M, N, r, "mu", **kw)
    host.upload_sparse(fmt, *arrays, base)
    feed_sparse_device(dev, fmt, arrays, base)
    assert host.geometry() == dev.geometry()
    assert same_bits(dev.error_terms(0), host.error_terms(0))
    for which in (6, 7):
        a, b = dense_image(dev, which), dense_image(host, which)
        assert (a is None) == (b is None) and (a is None or same_bits(a, b)), f"image {which}"
    assert dense_image(host, 6) is not None
    assert_same_run(run(dev, W, H, 3, value), run(host, W, H, 3, value), f"densify {kw} format {fmt}")
    host.close()
    dev.close()


# ---- case 3: inputs the device builder hands back -----------------------------------------------------------------------------------------------------

def test_hand_back(monkeypatch):
    monkeypatch.delenv("NMFAMD_SPARSE_SETUP", raising=False)
    m, n, r = 300, 200, 6
    rows, cols, vals = triplets(m, n, 0.1, seed=2)
    W, H = factors(m, n, r, seed=9)
    outside = (np.concatenate([vals, [9.0]]).astype(np.float32), np.concatenate([rows, [m + 5]]).astype(np.int32), np.concatenate([cols, [1]]).astype(np.int32))
    m2 = 9000
    rng = np.random.default_rng(9)
    long_column = ((1.0 + rng.random(m2 + 500)).astype(np.float32), np.concatenate([np.arange(m2), rng.integers(0, m2, 500)]).astype(np.int32),
                   np.concatenate([np.full(m2, 3), rng.integers(0, n, 500)]).astype(np.int32))
    for (mm, arrays) in ((m, outside), (m2, long_column)):
        Wm, _ = factors(mm, n, r, seed=9)
        host = na.Engine(mm, n, r, "mu", sparse_compute=True)
        dev = na.Engine(mm, n, r, "mu", sparse_compute=True)
        host.upload_sparse(3, *arrays, 0)
        feed_sparse_device(dev, 3, arrays, 0)
        assert host.geometry()["sparse_setup"] == 0 and dev.geometry()["sparse_setup"] == 0
        assert_same_run(run(dev, Wm, H, 3, "frobenius"), run(host, Wm, H, 3, "frobenius"), f"hand-back m = {mm}")
        host.close()
        dev.close()
    # the switch takes the same way
    monkeypatch.setenv("NMFAMD_SPARSE_SETUP", "host")
    good = (vals, rows, cols)
    host = na.Engine(m, n, r, "mu", sparse_compute=True)
    dev = na.Engine(m, n, r, "mu", sparse_compute=True)
    host.upload_sparse(3, *good, 0)
    feed_sparse_device(dev, 3, good, 0)
    assert dev.geometry()["sparse_setup"] == 0
    assert_same_run(run(dev, W, H, 3, "frobenius"), run(host, W, H, 3, "frobenius"), "NMFAMD_SPARSE_SETUP=host")
    host.close()
    dev.close()


# ---- case 4: refusals with the host entry's status and text ---------------------------------------------------------------------------------------------

def test_refusals_of_sparse_arrays():
    torch = torch_()
    r = 5
    rows, cols, vals = triplets(M, N, 0.1, seed=4)
    neg, nan = vals.copy(), vals.copy()
    neg[-1] = -1.0
    nan[-1] = np.nan
    empty = (np.zeros(0, np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32))
    weights = dict(weighted=True, divergence="beta", beta=0.5)
    cases = [("a negative value, beta = 1", dict(divergence="kl", dense_compute=True), (neg, rows, cols)),
             ("NaN, missing values", dict(missing_values=True), (nan, rows, cols)),
             ("no entry, missing values", dict(missing_values=True), empty),
             ("Itakura-Saito", dict(divergence="is"), (vals, rows, cols)),
             ("weighted", weights, (vals, rows, cols))]
    for what, kw, arrays in cases:
        host = na.Engine(M, N, r, "mu", **kw)
        dev = na.Engine(M, N, r, "mu", **kw)
        want = refusal(lambda: host.upload_sparse(3, *arrays, 0))
        got = refusal(lambda: dev.upload_sparse_device(3, *[torch.from_numpy(x).cuda() for x in arrays], 0))
        assert want[0] == 1 and got == want and "(" in got[1], (what, want, got)
        host.close()
        dev.close()
    # a format outside 1 ... 3: the host entry's status (it gives no text)
    eng = na.Engine(M, N, r, "mu", sparse_compute=True)
    dev_arrays = [torch.from_numpy(x).cuda() for x in (vals, rows, cols)]
    assert refusal(lambda: eng.upload_sparse(4, vals, rows, cols, 0)) == refusal(lambda: eng.upload_sparse_device(4, *dev_arrays, 0))
    eng.close()


# ---- case 5: refusals that run no kernel ----------------------------------------------------------------------------------------------------------------

def test_refusals_that_run_no_kernel(monkeypatch):
    monkeypatch.delenv("NMFAMD_SPARSE_SETUP", raising=False)
    torch = torch_()
    r = 5
    rows, cols, vals = triplets(M, N, 0.1, seed=4)
    fmt, base = 1, 0
    arrays = as_format(fmt, rows, cols, vals, M, N, base, "sorted")
    nnz = len(vals)
    W, H = factors(M, N, r)
    eng = na.Engine(M, N, r, "mu", sparse_compute=True)
    eng.upload_sparse(fmt, *arrays, base)
    want = run(eng, W, H, 3, "frobenius")
    images = sparse_images(eng, nnz, M, N)
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in arrays]
    pinned = [torch.from_numpy(np.ascontiguousarray(x)).pin_memory() for x in arrays]
    counts = (nnz, M + 1, nnz)
    good = [(t.data_ptr(), c) for t, c in zip(dev, counts)]
    names = ("values", "a", "b")

    def call(k, pair):
        args = list(good)
        args[k] = pair
        return refusal(lambda: eng.upload_sparse_device(fmt, *args, base))

    for k, name in enumerate(names):
        for what, ptr, text in (("host memory", np.ascontiguousarray(arrays[k]).ctypes.data, "not device memory"), ("pinned memory", pinned[k].data_ptr(), "pinned")):
            status, msg = call(k, (ptr, counts[k]))
            assert status == 1 and "(" in msg and name + ":" in msg and text in msg, (name, what, msg)
    status, msg = call(0, (0, nnz))
    assert status == 1 and "values: null" in msg, msg
    # `a` one element short of what the call reads: its m + 1 ints start m ints before the end of their allocation
    end = dev[1].data_ptr() + na.device_pointer_info(dev[1].data_ptr())["bytes_from_p"]
    status, msg = call(1, (end - 4 * M, M + 1))
    assert status == 1 and "a:" in msg and "allocation" in msg, msg
    assert na.device_pointer_info(end - 4 * (M + 1))["bytes_from_p"] == 4 * (M + 1)      # (... and one element earlier they would fit)
    status, msg = call(2, (dev[2].data_ptr() + 2, nnz))
    assert status == 1 and "b:" in msg and "aligned" in msg, msg
    # the engine is as it was: the images were not touched and it runs as before
    assert_same_images(sparse_images(eng, nnz, M, N), images)
    assert_same_run(run(eng, W, H, 3, "frobenius"), want, "after the refusals")
    eng.upload_sparse_device(fmt, *good, base)      # (raw pairs are taken)
    assert_same_run(run(eng, W, H, 3, "frobenius"), want, "after a good device upload")
    eng.close()


# ---- case 6: dense V on the sparse engines ----------------------------------------------------------------------------------------------------------------

def on_device(A, form):
    """(view, base): A (numpy, rows x cols) as a device tensor view of that shape in the given form, and the buffer it is a view of.  Gaps hold 7.0 (a value that
    would be stored if it were read)."""
    torch = torch_()
    rows, cols = A.shape
    t = torch.from_numpy(np.ascontiguousarray(A))
    if form == "cm":
        base = t.T.contiguous().cuda()
        view = base.T
    elif form == "cm_gap":
        base = torch.full((cols, rows + 3), 7.0, dtype=t.dtype, device="cuda")
        base[:, :rows] = t.T.cuda()
        view = base[:, :rows].T
    elif form == "rm":
        base = t.cuda()
        view = base
    elif form == "rm_gap":
        base = torch.full((rows, cols + 5), 7.0, dtype=t.dtype, device="cuda")
        base[:, :cols] = t.cuda()
        view = base[:, :cols]
    elif form == "rm_off1":
        base = torch.full((rows * cols + 1,), 7.0, dtype=t.dtype, device="cuda")
        base[1:] = t.cuda().reshape(-1)
        view = base[1:].view(rows, cols)
        assert view.data_ptr() % 16 != 0
    else:
        raise ValueError(form)
    torch.cuda.synchronize()
    return view, base


def feed_stored(eng, V, form):
    torch = torch_()
    view, base = on_device(V, form)
    before = base.clone()
    eng.upload_device_stored(view)
    torch.cuda.synchronize()
    assert same_bits(base.cpu().numpy(), before.cpu().numpy())


def stored_problem(dtype, missing, m=M, n=N):
    """Multiples of 2^-6 in (0, 8) (see the module's docstring); about 30 % holes (zeros, or NaN on a missing-values engine, where some stored entries are zeros);
    row 70 and column 200 empty, the tile rows 64 .. 127 x columns 64 .. 127 empty, the tile rows 0 .. 63 x columns 128 .. 191 full."""
    key = ("stored", np.dtype(dtype).name, missing, m, n)
    if key not in _cache:
        rng = np.random.default_rng(31)
        hole = np.nan if missing else 0.0
        V = (rng.integers(1, 512, size=(m, n)) / 64.0).astype(dtype)
        if missing:
            V[rng.random((m, n)) < 0.05] = 0.0      # stored zeros
        V[rng.random((m, n)) < 0.3] = hole
        V[70, :] = hole
        V[:, 200] = hole
        V[64:128, 64:128] = hole
        V[0:64, 128:192] = (rng.integers(1, 512, size=(64, 64)) / 64.0).astype(dtype)
        V = F(V)
        V.setflags(write=False)
        _cache[key] = V
    return _cache[key]


def stored_pair(V, form, kw, value, dtype=np.float32, r=5):
    m, n = V.shape
    W, H = factors(m, n, r, dtype)
    host = na.Engine(m, n, r, "mu", dtype=dtype, **kw)
    dev = na.Engine(m, n, r, "mu", dtype=dtype, **kw)
    host.upload(V)
    feed_stored(dev, V, form)
    assert dev.geometry()["sparse_setup"] == 1
    missing = bool(kw.get("missing_values"))
    nnz = int((~np.isnan(V)).sum()) if missing else int((V != 0).sum())
    a, b = sparse_images(dev, nnz, m, n), sparse_images(host, nnz, m, n)
    assert_same_images(a, b)
    if dtype == np.float32:
        assert a[14][-1] == nnz and a[16][-1] == nnz
    assert same_bits(dev.error_terms(0), host.error_terms(0))
    assert_same_run(run(dev, W, H, 3, value), run(host, W, H, 3, value), f"stored {form} {kw}")
    host.close()
    dev.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("missing", [False, True])
def test_upload_device_stored(form, missing):
    V = stored_problem(np.float32, missing)
    assert 0.25 < (np.isnan(V) if missing else V == 0).mean() < 0.45 and (not missing or (V == 0).sum() > 500)
    stored_pair(V, form, dict(missing_values=True) if missing else dict(sparse_compute=True), "rmsd" if missing else "frobenius")


def test_upload_device_stored_float64():
    stored_pair(stored_problem(np.float64, True), "rm_gap", dict(missing_values=True), "rmsd", np.float64)


def test_upload_device_stored_sparse_kl():
    stored_pair(stored_problem(np.float32, False), "cm_gap", dict(sparse_compute=True, divergence="kl"), "kl_divergence")


def test_upload_device_stored_builds_the_permutation_of_the_two_pass_kl_step(monkeypatch, diag_build):
    """NMFAMD_KL_TWO_PASS (measurement build) permutes the quotients from the CSR order into the CSC order through csc_from_csr_, which the scatter kernel computes
    from the tile's row masks: with a wrong permutation the two-pass iteration would not return the bits it returns from the host-built images."""
    monkeypatch.setenv("NMFAMD_KL_TWO_PASS", "1")
    stored_pair(stored_problem(np.float32, False), "rm_gap", dict(sparse_compute=True, divergence="kl"), "kl_divergence")


# ---- case 7: no capacity limit on the stored route ----------------------------------------------------------------------------------------------------------

def test_no_capacity_limit_on_the_stored_route():
    """Fully observed columns of 9 000 entries: longer than the segment sort of the sparse builder takes (8 192), which the compaction does not use."""
    m, n = 9000, 130
    rng = np.random.default_rng(5)
    V = F((rng.integers(1, 512, size=(m, n)) / 64.0).astype(np.float32))
    stored_pair(V, "rm", dict(missing_values=True), "rmsd")


# ---- case 8: refusals of upload_device_stored ---------------------------------------------------------------------------------------------------------------

def test_refusals_of_upload_device_stored():
    r = 5
    V = stored_problem(np.float32, True)
    W, H = factors(M, N, r)
    inf = V.copy(order="F")
    inf[M - 1, N - 1] = np.inf      # the ragged corner
    nothing = F(np.full((M, N), np.nan, np.float32))
    for bad, text in ((inf, "infinite"), (nothing, "no observed entry")):
        host = na.Engine(M, N, r, "mu", missing_values=True)
        dev = na.Engine(M, N, r, "mu", missing_values=True)
        dev.upload(V)
        before = run(dev, W, H, 2, "rmsd")
        want = refusal(lambda: host.upload(bad))
        got = refusal(lambda: feed_stored(dev, bad, "rm_gap"))
        assert want[0] == 1 and got == want and text in got[1], (want, got)
        assert_same_run(run(dev, W, H, 2, "rmsd"), before, "after the refusal")      # (refused before anything of the engine changed)
        host.close()
        dev.close()
    dense = stored_problem(np.float32, False)
    plain = na.Engine(M, N, r, "mu")
    status, text = refusal(lambda: feed_stored(plain, dense, "rm"))
    assert status == 1 and "upload_dense_device" in text, text
    plain.close()
    weighted = na.Engine(M, N, r, "mu", weighted=True, divergence="beta", beta=0.5)
    got = refusal(lambda: feed_stored(weighted, dense, "rm"))
    assert got == refusal(lambda: weighted.upload(dense)) and got[0] == 1 and "weights" in got[1], got
    weighted.close()
    # a pointer the check refuses, on the engine that takes the entry
    eng = na.Engine(M, N, r, "mu", sparse_compute=True)
    status, text = refusal(lambda: eng.upload_device_stored((np.ascontiguousarray(dense).ctypes.data, N, 1)))
    assert status == 1 and "V:" in text and "not device memory" in text, text
    eng.close()
