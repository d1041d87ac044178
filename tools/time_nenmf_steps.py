"""usage: python tools/time_nenmf_steps.py [--other PATH/libnmfgpu64.so] [--ranks 64,128] [--steps 1,8,16] [--sweeps 1,3] [--iterations 60]
                                          [--tolerance 1e-30] [--other-nenmf] [--constant-w]      (on the GPU box)
Kernel time of the NeNMF step launch (k_apg_steps, docs/NENMF.md) at 10 000 x 5 000, fp32, beside the HALS sweep launch (k_sweep_hals / k_sweeps_hals) of another
build of the library (--other: the commit before, say; without it this build's), all in ONE process under one `rocprofv3 --kernel-trace`: per rank the child runs
the HALS engines at the given sweep counts and the NeNMF engines at the given step counts one after the other, the same number of iterations each, from the same
start.  An iteration launches its factor kernel twice, for H and then for W, so the launches of a kernel family in start order fall into the configurations by
position; the first ten iterations of each are dropped.  Prints the mean kernel time of the H launch and of the W launch per configuration, and the cost of one
more step, (T_b - T_a) / (b - a) for the two largest step counts.
--tolerance DELTA: every step count runs once more as a MAXIMUM count with per-column dynamic stopping at DELTA (k_apg_steps_dyn, docs/NENMF.md "Dynamic
stopping"; 1e-30 freezes nothing, so the difference to the static row is what the rule itself costs); --other-nenmf: the static step counts also run on the
--other build (k_apg_steps of the commit before).  --constant-w: W is kept, so an iteration launches the H kernel only -- the NNLS solve of new data against a
fixed basis, every time from the same start -- and the dynamic rows print the histogram of the counts of their last step (not with --wall).
--wall: no profiler; wall time per iteration instead, every configuration in turn within a round, five rounds of 200 iterations (tools/time_hals_sweeps.py's way)."""
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
M, N = 10000, 5000
SKIP = 10


def configurations(a):
    """(label, kernel family in the trace, algorithm, count, on the other build, tolerance)"""
    out = [(f"{'other ' if a.other else ''}hals ({s},{s})", "hals", "hals", int(s), bool(a.other), 0.0) for s in a.sweeps.split(",") if s]
    steps = [int(t) for t in a.steps.split(",") if t]
    if a.other and a.other_nenmf:
        out += [(f"other nenmf ({t},{t})", "nenmf", "nenmf", t, True, 0.0) for t in steps]
    out += [(f"nenmf ({t},{t})", "nenmf", "nenmf", t, False, 0.0) for t in steps]
    if a.tolerance > 0:
        out += [(f"nenmf (<={t},<={t}) delta {a.tolerance:g}", "nenmf_dyn", "nenmf", t, False, a.tolerance) for t in steps if t > 1]
    return out


def engines_for(a, r, V):
    import contextlib
    import nmfgpu_amd as na
    from nmfgpu_amd import _lib
    out = []
    for label, _, alg, count, other, tol in configurations(a):
        kw = dict(sweeps_h=count, sweeps_w=count) if alg == "hals" else dict(steps_h=count, steps_w=count)
        if tol > 0:
            kw["step_tolerance"] = tol
        with (_lib.use_library(a.other) if other else contextlib.nullcontext()):      # (an engine keeps the library it was created with)
            e = na.Engine(M, N, r, alg, **kw)
        e.upload(V)
        out.append((label, e))
    return out


def problem(r, rng):
    W = np.asfortranarray((1.0 - rng.random((M, r))).astype(np.float32))
    H = np.asfortranarray((1.0 - rng.random((r, N))).astype(np.float32))
    return W, H


def child(a):
    rng = np.random.default_rng(1)
    V = np.asfortranarray(rng.random((M, N)).astype(np.float32))
    for r in (int(x) for x in a.ranks.split(",")):
        W, H = problem(r, rng)
        for name, e in engines_for(a, r, V):
            e.set_factors(W, H)
            if a.constant_w:      # (every launch solves from the same start: a second H step against the same W would begin at the solution)
                for _ in range(a.iterations):
                    e.set_factors(None, H)
                    e.iterate(1, error_every=0, constant_w=True)
            else:
                e.iterate(a.iterations, error_every=0)
            e.synchronize()
            if "delta" in name:
                print(f"r = {r:3d} {name}: counts of the last H step {np.bincount(e.step_counts(0)).tolist()}", flush=True)
            e.close()


def wall(a):
    rng = np.random.default_rng(1)
    V = np.asfortranarray(rng.random((M, N)).astype(np.float32))
    for r in (int(x) for x in a.ranks.split(",")):
        W, H = problem(r, rng)
        engines = engines_for(a, r, V)
        times = {k: [] for k, _ in engines}
        for _ in range(5):
            for k, e in engines:
                e.set_factors(W, H)
                e.iterate(20, error_every=0)
                e.synchronize()
                t0 = time.perf_counter()
                e.iterate(200, first_iteration=21, error_every=0)
                e.synchronize()
                times[k].append((time.perf_counter() - t0) / 200 * 1e6)
        for k, v in times.items():
            print(f"r = {r:3d} {k:36s} median {np.median(v):7.1f} us / iteration, range {min(v):7.1f} ... {max(v):7.1f}; runs {' '.join(f'{x:.1f}' for x in v)}", flush=True)
        for _, e in engines:
            e.close()


def traced(a, passthrough):
    d = tempfile.mkdtemp(prefix="nenmf_", dir="/tmp")
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--child", *passthrough]
    out = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise SystemExit(out.stderr[-2000:])
    print("".join(line + "\n" for line in out.stdout.splitlines() if line.startswith("r = ")), end="")
    launches = {"hals": [], "nenmf": [], "nenmf_dyn": []}
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            name = row["Kernel_Name"]
            family = ("nenmf_dyn" if "k_apg_steps_dyn" in name else "nenmf" if "k_apg_steps" in name
                      else "hals" if ("k_sweep_hals" in name or "k_sweeps_hals" in name) else None)
            if family:
                launches[family].append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    for v in launches.values():
        v.sort()
    at = {k: 0 for k in launches}
    each = 1 if a.constant_w else 2                # launches of the factor kernel per iteration
    per = each * a.iterations
    for r in (int(x) for x in a.ranks.split(",")):
        found = {}
        for label, family, alg, count, other, tol in configurations(a):
            mine = launches[family][at[family]:at[family] + per]
            at[family] += per
            if len(mine) != per:
                raise SystemExit(f"{label}: {len(mine)} launches in the trace, expected {per}")
            kept = mine[each * SKIP:]
            h = np.array([ns for _, ns in kept[0::each]]) / 1e3
            w = h if a.constant_w else np.array([ns for _, ns in kept[1::2]]) / 1e3
            if not other and tol == 0:
                found[(alg, count)] = (h.mean(), w.mean())
            tail = "" if a.constant_w else f", W launch {w.mean():8.2f} us (min {w.min():.2f}), mean of the two {(h.mean() + w.mean()) / 2:8.2f} us"
            print(f"r = {r:3d} {label}: H launch {h.mean():8.2f} us (min {h.min():.2f}){tail}", flush=True)
        ts = sorted(c for alg, c in found if alg == "nenmf")
        if len(ts) >= 2:
            lo, hi = ts[-2], ts[-1]
            dh = (found[("nenmf", hi)][0] - found[("nenmf", lo)][0]) / (hi - lo)
            dw = (found[("nenmf", hi)][1] - found[("nenmf", lo)][1]) / (hi - lo)
            print(f"r = {r:3d} one more step, (T = {hi} minus T = {lo}) / {hi - lo}: H {dh:.2f} us, W {dw:.2f} us")
        ss = sorted(c for alg, c in found if alg == "hals")
        if len(ss) >= 2:
            lo, hi = ss[0], ss[-1]
            dh = (found[("hals", hi)][0] - found[("hals", lo)][0]) / (hi - lo)
            dw = (found[("hals", hi)][1] - found[("hals", lo)][1]) / (hi - lo)
            print(f"r = {r:3d} one more sweep, (s = {hi} minus s = {lo}) / {hi - lo}: H {dh:.2f} us, W {dw:.2f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", default=None)
    ap.add_argument("--ranks", default="64,128")
    ap.add_argument("--steps", default="1,8,16")
    ap.add_argument("--sweeps", default="1,3")
    ap.add_argument("--iterations", type=int, default=60)
    ap.add_argument("--tolerance", type=float, default=0.0)
    ap.add_argument("--other-nenmf", action="store_true")
    ap.add_argument("--constant-w", action="store_true")
    ap.add_argument("--wall", action="store_true")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.other:
        a.other = os.path.abspath(a.other)
    if a.child:
        return child(a)
    if a.wall:
        return wall(a)
    passthrough = ["--ranks", a.ranks, "--steps", a.steps, "--sweeps", a.sweeps, "--iterations", str(a.iterations), "--tolerance", repr(a.tolerance)]
    passthrough += (["--other", a.other] if a.other else []) + (["--other-nenmf"] if a.other_nenmf else []) + (["--constant-w"] if a.constant_w else [])
    traced(a, passthrough)


if __name__ == "__main__":
    main()
