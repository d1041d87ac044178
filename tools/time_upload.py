"""usage: python tools/time_upload.py [--other PATH/libnmfgpu64.so] [--reps 10] [--warmup 2] [--no-trace]      (on the GPU box)
Wall time of getting V into an engine and the factors out of it at 10 000 x 5 000, r = 64, fp32 (docs/DEVICE_IO.md): Engine.upload from pageable numpy memory
with another build of the library (--other: the commit before; without it the column is left out) and with this build, Engine.upload_device from a torch tensor on
the same GPU, column-major and row-major, and get_factors against get_factors_device -- the median of --reps calls after --warmup, all in one process, for a
default "mu" engine, a beta = 0 dense divergence engine (the host upload walks V with its value loop) and a weighted beta = 0.5 engine (the loop plus a cleaned
copy).  The device uploads include the hipDeviceSynchronize the entry starts with; the tensors exist before the clock starts (that V is already in HBM is the
premise).  Unless --no-trace, a child under `rocprofv3 --kernel-trace` then repeats the device uploads and the kernel time of the import launch is printed beside
the wall time: what remains is finish_upload, the part both paths share."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.other:
        a.other = os.path.abspath(a.other)
    if a.child:
        return child(a)
    wall(a)
    if not a.no_trace:
        traced(a)


if __name__ == "__main__":
    main()
