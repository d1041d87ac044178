"""Sparse HALS (docs/HALS.md, "Sparse compute") beside the sparse-Frobenius multiplicative update on one CSR at BASELINE config 3's shape
(100 000 x 20 000, 1 % stored, r = 128, fp32), in one process, from the same start.

Prints, per algorithm: the wall time per iteration of plain iterations and of error iterations (stream synchronised around each timed block), the
event-timed H-side / W-side product launches (nmfamd_engine_kernel_timing_read3), and the relative error ||V - W H|| / ||V|| after 10 and 100
iterations.  "hals-pen" is HALS with l1W = l1H = 0.05, l2W = l2H = 0.01.  --sweeps-h / --sweeps-w (default 1 / 1) other than 1 add a row "sparse hals h,w":
accelerated HALS with that many sweeps per product (docs/HALS.md, "Inner sweeps").

    python tools/time_hals_sparse.py [--iters 50] [--warmup 10] [--rows 100000] [--cols 20000] [--sweeps-h 4 --sweeps-w 4]
    python tools/time_hals_sparse.py --kernels      a child run of 40 plain sparse HALS iterations under `rocprofv3 --kernel-trace`: launches and
                                                    median duration per kernel and grid size (set-up launches included: they show once or twice)
"""
import argparse
import collections
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench
import nmfgpu_amd as na


def time_block(eng, iters, error_every):
    eng.synchronize()
    t0 = time.perf_counter()
    eng.iterate(iters, first_iteration=1, error_every=error_every, last_iteration=0)
    eng.synchronize()
    if error_every:
        eng.frobenius      # (waits for the last error terms and sums them)
    return (time.perf_counter() - t0) / iters * 1e3


def trace_child(rows, cols):
    val, ptr, idx, W, H = bench.make_sparse_problem(m=rows, n=cols)
    eng = na.Engine(W.shape[0], H.shape[1], W.shape[1], "hals", sparse_compute=True)
    eng.upload_sparse(1, val, ptr, idx, 0)
    eng.set_factors(W, H)
    eng.iterate(40, first_iteration=1, error_every=0, last_iteration=0)
    eng.synchronize()
    eng.close()


def kernels(rows, cols):
    d = tempfile.mkdtemp(prefix="ths_", dir="/tmp")
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", "python3", os.path.abspath(__file__), "--trace-child", "--rows", str(rows),
           "--cols", str(cols)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise SystemExit(out.stderr[-2000:])
    per = collections.defaultdict(list)
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if "nmfamd" in row["Kernel_Name"]:
                per[(row["Kernel_Name"].split("(")[0][:80], row.get("Grid_Size_X", row.get("Grid_Size", "?")))].append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    for (k, g), v in sorted(per.items(), key=lambda kv: -sum(kv[1])):
        v = sorted(v)
        print(f"{k:82s} grid {g:>10s} x{len(v):4d} median {v[len(v) // 2] / 1e3:9.2f} us total {sum(v) / 1e3:10.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rows", type=int, default=bench.C3["rows"])
    ap.add_argument("--cols", type=int, default=bench.C3["columns"])
    ap.add_argument("--sweeps-h", type=int, default=1)
    ap.add_argument("--sweeps-w", type=int, default=1)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--trace-child", action="store_true")
    a = ap.parse_args()
    if a.trace_child:
        return trace_child(a.rows, a.cols)
    if a.kernels:
        return kernels(a.rows, a.cols)
    val, ptr, idx, W, H = bench.make_sparse_problem(m=a.rows, n=a.cols)
    m, n, r = W.shape[0], H.shape[1], W.shape[1]
    norm_v = float(np.sqrt((val.astype(np.float64) ** 2).sum()))
    print(f"CSR {m} x {n}, nnz {len(val)} ({100.0 * len(val) / m / n:.2f} %), r = {r}, fp32, ||V|| = {norm_v:.4f}")
    runs = [("sparse-frobenius mu", "mu", {}), ("sparse hals", "hals", {}), ("sparse hals-pen", "hals", dict(l1_w=0.05, l1_h=0.05, l2_w=0.01, l2_h=0.01))]
    if (a.sweeps_h, a.sweeps_w) != (1, 1):
        runs.append((f"sparse hals {a.sweeps_h},{a.sweeps_w}", "hals", dict(sweeps_h=a.sweeps_h, sweeps_w=a.sweeps_w)))
    for name, alg, kw in runs:
        eng = na.Engine(m, n, r, alg, sparse_compute=True, **kw)
        eng.upload_sparse(1, val, ptr, idx, 0)
        eng.set_factors(W, H)
        errs = {}
        for upto in (10, 100):
            first = 1 if upto == 10 else 11
            eng.iterate(upto - first + 1, first_iteration=first, error_every=0, last_iteration=upto)
            errs[upto] = eng.frobenius / norm_v
        eng.iterate(a.warmup, first_iteration=1, error_every=0, last_iteration=0)
        plain = time_block(eng, a.iters, 0)
        err = time_block(eng, a.iters, 1)
        eng.kernel_timing(1)
        eng.iterate(a.iters, first_iteration=1, error_every=0, last_iteration=0)
        _, _, idle, (ms_h, ms_w), (c_h, c_w) = eng.kernel_timing_read3()
        eng.kernel_timing(0)
        print(f"{name:>20}: {plain:.3f} ms / iteration, {err:.3f} ms / error iteration; H side {ms_h / max(c_h, 1):.3f} ms, W side {ms_w / max(c_w, 1):.3f} ms "
              f"per product launch (idle event pair {idle:.4f} ms); relative error after 10 / 100 iterations {errs[10]:.5f} / {errs[100]:.5f}", flush=True)
        eng.close()


if __name__ == "__main__":
    main()
