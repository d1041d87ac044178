"""Times of missing-value coordinate descent (docs/MISSING.md, "Coordinate descent") against the masked multiplicative update on one CSR at BASELINE
config 3's shape (100 000 x 20 000, 1 % stored, fp32), in one process, after a warm-up.

Part 1, per rank in --ranks and sweep count in --sweeps: the wall time per plain iteration and per error iteration (stream synchronised around each timed block),
and the event-timed H-side / W-side half-steps (nmfamd_engine_kernel_timing_read3); the masked multiplicative update beside them.

Part 2, per rank: the error the masked multiplicative update reports after --mu-iters iterations from the start of bench.make_sparse_problem, the wall time it
took, and the wall time coordinate descent takes from the same start to report that error or less (it is asked for its error every --check iterations, the
multiplicative update only at the end; both times include those error iterations).  --other PATH runs the multiplicative update of part 2 on another build of the
library (the parent commit's): the comparison docs/HALS.md makes.

    python tools/time_masked_cd.py [--ranks 64,128] [--sweeps 1,4] [--iters 20] [--warmup 3] [--mu-iters 1000] [--check 5] [--max-cd-iters 400]
                                   [--rows 100000] [--cols 20000] [--other PATH/libnmfgpu64.so] [--skip-target]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench
import nmfgpu_amd as na
from nmfgpu_amd import _lib


def time_block(eng, iters, error_every):
    eng.synchronize()
    t0 = time.perf_counter()
    eng.iterate(iters, first_iteration=1, error_every=error_every, last_iteration=0)
    eng.synchronize()
    if error_every:
        eng.frobenius      # (waits for the last error terms and sums them)
    return (time.perf_counter() - t0) / iters * 1e3


def report(name, eng, a):
    eng.iterate(a.warmup, first_iteration=1, error_every=0, last_iteration=0)
    plain = time_block(eng, a.iters, 0)
    err = time_block(eng, a.iters, 1)
    eng.kernel_timing(1)
    eng.iterate(a.iters, first_iteration=1, error_every=0, last_iteration=0)
    _, _, idle, (ms_h, ms_w), (c_h, c_w) = eng.kernel_timing_read3()
    eng.kernel_timing(0)
    print(f"{name:>22}: {plain:.3f} ms / iteration, {err:.3f} ms / error iteration; H side {ms_h / max(c_h, 1):.3f} ms, W side {ms_w / max(c_w, 1):.3f} ms "
          f"per launch bracket (idle event pair {idle:.4f} ms)", flush=True)
    return ms_h / max(c_h, 1), ms_w / max(c_w, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", default="64,128")
    ap.add_argument("--sweeps", default="1,4")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mu-iters", type=int, default=1000)
    ap.add_argument("--check", type=int, default=5)
    ap.add_argument("--max-cd-iters", type=int, default=400)
    ap.add_argument("--rows", type=int, default=bench.C3["rows"])
    ap.add_argument("--cols", type=int, default=bench.C3["columns"])
    ap.add_argument("--other", default=None)
    ap.add_argument("--skip-target", action="store_true")
    a = ap.parse_args()
    ranks = [int(x) for x in a.ranks.split(",")]
    sweeps = [int(x) for x in a.sweeps.split(",")]
    for r in ranks:
        val, ptr, idx, W, H = bench.make_sparse_problem(m=a.rows, n=a.cols, r=r)
        m, n = W.shape[0], H.shape[1]
        nnz = len(val)
        print(f"CSR {m} x {n}, nnz {nnz} ({100.0 * nnz / m / n:.2f} %), r = {r}, fp32", flush=True)

        def engine(**kw):
            eng = na.Engine(m, n, r, "mu", missing_values=True, **kw)
            eng.upload_sparse(1, val, ptr, idx, 0)
            eng.set_factors(W, H)
            return eng

        eng = engine()
        report("masked mu", eng, a)
        eng.close()
        rp = 64 if r <= 64 else 128
        # the Gram work of a half-step before the symmetry saving: 2 RP^2 per stored entry
        flop = 2.0 * rp * rp * nnz
        for s in sweeps:
            eng = engine(missing_solver="cd", missing_sweeps_h=s, missing_sweeps_w=s)
            ms_h, ms_w = report(f"masked cd, sweeps {s}", eng, a)
            print(f"{'':>22}  Gram work {flop / 1e12:.3f} TFLOP per half-step: H side {flop / (ms_h * 1e-3) / 1e12:.1f}, W side {flop / (ms_w * 1e-3) / 1e12:.1f} TFLOP/s "
                  f"if the sweeps were free", flush=True)
            eng.close()
        if a.skip_target:
            continue
        # part 2: the error of the multiplicative update after --mu-iters iterations, and the time coordinate descent needs to report it
        if a.other:
            with _lib.use_library(a.other):
                eng = engine()
        else:
            eng = engine()
        eng.synchronize()
        t0 = time.perf_counter()
        eng.iterate(a.mu_iters, first_iteration=1, error_every=0, last_iteration=a.mu_iters)
        target = eng.frobenius
        t_mu = time.perf_counter() - t0
        eng.close()
        print(f"{'masked mu':>22}: error {target:.4f} after {a.mu_iters} iterations, {t_mu * 1e3:.1f} ms" + (f" (library {a.other})" if a.other else ""), flush=True)
        for s in sweeps:
            eng = engine(missing_solver="cd", missing_sweeps_h=s, missing_sweeps_w=s)
            eng.synchronize()
            t0 = time.perf_counter()
            done, err = 0, float("inf")
            while done < a.max_cd_iters and not err <= target:
                eng.iterate(a.check, first_iteration=done + 1, error_every=0, last_iteration=done + a.check)
                done += a.check
                err = eng.frobenius
            t_cd = time.perf_counter() - t0
            eng.close()
            verdict = f"reached after {done} iterations" if err <= target else f"NOT reached within {done} iterations"
            print(f"{'masked cd, sweeps ' + str(s):>22}: error {err:.4f}, {verdict}, {t_cd * 1e3:.1f} ms ({t_mu / t_cd:.2f} x the multiplicative update's time)", flush=True)


if __name__ == "__main__":
    main()
