"""usage: python tools/time_upload.py [--sparse] [--other PATH/libnmfgpu64.so] [--reps 10] [--warmup 2] [--no-trace]      (on the GPU box)
Wall time of getting V into an engine and the factors out of it at 10 000 x 5 000, r = 64, fp32 (docs/DEVICE_IO.md): Engine.upload from pageable numpy memory
with another build of the library (--other: the commit before; without it the column is left out) and with this build, Engine.upload_device from a torch tensor on
the same GPU, column-major and row-major, and get_factors against get_factors_device -- the median of --reps calls after --warmup, all in one process, for a
default "mu" engine, a beta = 0 dense divergence engine (the host upload walks V with its value loop) and a weighted beta = 0.5 engine (the loop plus a cleaned
copy).  The device uploads include the hipDeviceSynchronize the entry starts with; the tensors exist before the clock starts (that V is already in HBM is the
premise).  Unless --no-trace, a child under `rocprofv3 --kernel-trace` then repeats the device uploads and the kernel time of the import launch is printed beside
the wall time: what remains is finish_upload, the part both paths share.

--sparse: the two sparse rows of docs/DEVICE_IO.md instead -- Engine.upload_sparse (host arrays; --other's build and this one) against Engine.upload_sparse_device
(torch tensors) on the benchmark's sparse configuration (bench.py, make_sparse_problem: CSR 100 000 x 20 000 at 1 %, r = 128, KL), and Engine.upload (numpy) against
Engine.upload_device_stored (torch tensor, row-major and column-major) at 10 000 x 5 000 on a missing_values engine with 10 % NaN; then, unless --no-trace, the
kernel times of the compaction's launches (count, the two scans, scatter) from a traced child."""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M, N, R = 10000, 5000, 64
ENGINES = (("mu (default)", dict(), False), ("beta = 0 dense", dict(divergence="is"), False), ("weighted beta = 0.5", dict(divergence="beta", beta=0.5, weighted=True), True))


def median_ms(call, reps, warmup):
    import torch
    out = []
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), min(out), max(out)


def data():
    import torch
    assert torch.cuda.is_available()
    rng = np.random.default_rng(1)
    V = np.asfortranarray((rng.random((M, N)) + 0.1).astype(np.float32))
    Om = np.asfortranarray((rng.random((M, N)) * (rng.random((M, N)) > 0.3)).astype(np.float32))
    dev = {}
    for name, a in (("V", V), ("Om", Om)):
        t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        dev[name, "rm"] = t
        dev[name, "cm"] = t.T.contiguous().T
    torch.cuda.synchronize()
    return V, Om, dev


def fmt(label, t):
    return f"{label:58s} median {t[0]:9.2f} ms   (min {t[1]:.2f}, max {t[2]:.2f})"


def wall(a):
    import torch
    import nmfgpu_amd as na
    from nmfgpu_amd import _lib
    V, Om, dev = data()
    for name, kw, weighted in ENGINES:
        print(f"--- {name}", flush=True)
        w = dict(weights=Om) if weighted else {}
        if a.other:
            with _lib.use_library(a.other):      # (an engine keeps the library it was created with)
                e = na.Engine(M, N, R, "mu", **kw)
            print(fmt("upload, pageable numpy, other build", median_ms(lambda: e.upload(V, **w), a.reps, a.warmup)), flush=True)
            e.close()
        e = na.Engine(M, N, R, "mu", **kw)
        print(fmt("upload, pageable numpy, this build", median_ms(lambda: e.upload(V, **w), a.reps, a.warmup)), flush=True)
        for form in ("cm", "rm"):
            wd = dict(weights=dev["Om", form]) if weighted else {}
            print(fmt(f"upload_device, torch tensor, {'column' if form == 'cm' else 'row'}-major", median_ms(lambda: e.upload_device(dev["V", form], **wd), a.reps, a.warmup)), flush=True)
        e.randomize(1)
        print(fmt("get_factors (numpy)", median_ms(lambda: e.get_factors(), a.reps, a.warmup)), flush=True)
        Wd = torch.empty((M, R), dtype=torch.float32, device="cuda")
        Hd = torch.empty((R, N), dtype=torch.float32, device="cuda")
        print(fmt("get_factors_device (torch, row-major)", median_ms(lambda: e.get_factors_device(Wd, Hd), a.reps, a.warmup)), flush=True)
        print(fmt("set_factors_device (torch, row-major)", median_ms(lambda: e.set_factors_device(Wd, Hd), a.reps, a.warmup)), flush=True)
        W, H = e.get_factors()
        print(fmt("set_factors (numpy)", median_ms(lambda: e.set_factors(W, H), a.reps, a.warmup)), flush=True)
        e.close()


def child(a):
    import nmfgpu_amd as na
    V, Om, dev = data()
    for name, kw, weighted in ENGINES:
        e = na.Engine(M, N, R, "mu", **kw)
        for form in ("cm", "rm"):
            for _ in range(a.reps):
                e.upload_device(dev["V", form], **(dict(weights=dev["Om", form]) if weighted else {}))
        e.close()


def traced(a):
    d = tempfile.mkdtemp(prefix="upload_", dir="/tmp")
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps)]
    out = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise SystemExit(out.stderr[-2000:])
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))]
    rows.sort()
    # an upload is everything from one import launch up to the next one
    starts = [i for i, r in enumerate(rows) if "k_import_dense" in r[2] or "k_import_weighted" in r[2]]
    if len(starts) != len(ENGINES) * 2 * a.reps:
        raise SystemExit(f"{len(starts)} import launches in the trace, expected {len(ENGINES) * 2 * a.reps}")
    print("--- kernel time inside upload_device (rocprofv3 --kernel-trace; medians over the calls): the import launch, and every other kernel up to the next import")
    at = 0
    for name, _, _ in ENGINES:
        for form in ("column-major", "row-major"):
            imp, rest = [], []
            for k in range(a.reps):
                i = starts[at + k]
                j = starts[at + k + 1] if at + k + 1 < len(starts) else len(rows)
                imp.append(rows[i][1] / 1e6)
                rest.append(sum(r[1] for r in rows[i + 1:j] if "fill" not in r[2].lower()) / 1e6)
            at += a.reps
            print(f"{name:22s} {form:13s} import kernel {np.median(imp):8.3f} ms, other kernels of the upload {np.median(rest):8.3f} ms", flush=True)


def sparse_data():
    import torch
    import bench
    assert torch.cuda.is_available()
    val, ptr, idx, _, _ = bench.make_sparse_problem()
    rng = np.random.default_rng(1)
    V = (rng.random((M, N)) + 0.1).astype(np.float32)
    V[rng.random((M, N)) < 0.1] = np.nan
    V = np.asfortranarray(V)
    t = torch.from_numpy(np.ascontiguousarray(V)).cuda()
    dev = {"csr": [torch.from_numpy(x).cuda() for x in (val, ptr, idx)], "rm": t, "cm": t.T.contiguous().T}
    torch.cuda.synchronize()
    return (val, ptr, idx), V, dev


def sparse_wall(a):
    import bench
    import nmfgpu_amd as na
    from nmfgpu_amd import _lib
    csr, V, dev = sparse_data()
    c3 = bench.C3
    m, n, r = c3["rows"], c3["columns"], c3["features"]
    print(f"--- sparse CSR {m} x {n}, {len(csr[0])} stored entries, r = {r}, KL (the benchmark's sparse configuration)", flush=True)
    if a.other:
        with _lib.use_library(a.other):
            e = na.Engine(m, n, r, "mu", divergence="kl")
        print(fmt("upload_sparse, numpy arrays, other build", median_ms(lambda: e.upload_sparse(1, *csr, 0), a.reps, a.warmup)), flush=True)
        e.close()
    e = na.Engine(m, n, r, "mu", divergence="kl")
    print(fmt("upload_sparse, numpy arrays, this build", median_ms(lambda: e.upload_sparse(1, *csr, 0), a.reps, a.warmup)), flush=True)
    print(fmt("upload_sparse_device, torch tensors", median_ms(lambda: e.upload_sparse_device(1, *dev["csr"], 0), a.reps, a.warmup)), flush=True)
    assert e.geometry()["sparse_setup"] == 1
    e.close()
    print(f"--- dense {M} x {N} with 10 % NaN on a missing_values engine, r = {R}", flush=True)
    if a.other:
        with _lib.use_library(a.other):
            e = na.Engine(M, N, R, "mu", missing_values=True)
        print(fmt("upload, pageable numpy, other build", median_ms(lambda: e.upload(V), a.reps, a.warmup)), flush=True)
        e.close()
    e = na.Engine(M, N, R, "mu", missing_values=True)
    print(fmt("upload, pageable numpy, this build", median_ms(lambda: e.upload(V), a.reps, a.warmup)), flush=True)
    for form in ("cm", "rm"):
        print(fmt(f"upload_device_stored, torch tensor, {'column' if form == 'cm' else 'row'}-major", median_ms(lambda: e.upload_device_stored(dev[form]), a.reps, a.warmup)), flush=True)
    assert e.geometry()["sparse_setup"] == 1
    e.close()


def sparse_child(a):
    import nmfgpu_amd as na
    _, V, dev = sparse_data()
    e = na.Engine(M, N, R, "mu", missing_values=True)
    for form in ("cm", "rm"):
        for _ in range(a.reps):
            e.upload_device_stored(dev[form])
    e.close()


def sparse_traced(a):
    d = tempfile.mkdtemp(prefix="upload_", dir="/tmp")
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--sparse", "--child", "--reps", str(a.reps)]
    out = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise SystemExit(out.stderr[-2000:])
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))]
    rows.sort()
    # an upload is everything from one count launch up to the next one
    starts = [i for i, r in enumerate(rows) if "k_compact_count" in r[2]]
    if len(starts) != 2 * a.reps:
        raise SystemExit(f"{len(starts)} count launches in the trace, expected {2 * a.reps}")
    print("--- kernel time inside upload_device_stored (rocprofv3 --kernel-trace; medians over the calls)")
    for f, form in enumerate(("column-major", "row-major")):
        parts = {"k_compact_count": [], "k_sp_scan": [], "k_compact_pointers": [], "k_compact_scatter": [], "k_sp_col_sumsq": [], "other": []}
        for k in range(a.reps):
            i = starts[f * a.reps + k]
            j = starts[f * a.reps + k + 1] if f * a.reps + k + 1 < len(starts) else len(rows)
            acc = dict.fromkeys(parts, 0.0)
            for r in rows[i:j]:
                if "fill" in r[2].lower():
                    continue
                acc[next((name for name in parts if name in r[2]), "other")] += r[1] / 1e6
            for name in parts:
                parts[name].append(acc[name])
        print(f"{form:13s} " + ", ".join(f"{name} {np.median(v):8.3f} ms" for name, v in parts.items()), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sparse", action="store_true")
    ap.add_argument("--other", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.other:
        a.other = os.path.abspath(a.other)
    if a.child:
        return sparse_child(a) if a.sparse else child(a)
    if a.sparse:
        sparse_wall(a)
        if not a.no_trace:
            sparse_traced(a)
        return
    wall(a)
    if not a.no_trace:
        traced(a)


if __name__ == "__main__":
    main()
