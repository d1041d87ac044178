"""Iteration times of the missing-value update under the beta-divergence (docs/MISSING.md, "Beta-divergence") against the Frobenius masked update -- the
yardstick, measured in the same run -- on one CSR at BASELINE config 3's shape (100 000 x 20 000, 1 % stored, r = 128, fp32), in one process, after a warm-up.
beta = 1 (the KL map: a division per entry), 0 (Itakura-Saito: a reciprocal) and 0.5 (the general map: a log2 / exp2 pair per entry, and the general power
gamma = 2 / 3 on the r values of every row).

Prints, per update: the wall time per iteration of plain iterations and of error iterations (stream synchronised around each timed block), and the event-timed
H-side / W-side half-steps (nmfamd_engine_kernel_timing_read3) of the plain iterations with the rate at which they gather factor rows.

    python tools/time_masked_beta.py [--iters 50] [--warmup 10] [--rows 100000] [--cols 20000]
"""
import argparse
import os
import sys
import time

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rows", type=int, default=bench.C3["rows"])
    ap.add_argument("--cols", type=int, default=bench.C3["columns"])
    a = ap.parse_args()
    val, ptr, idx, W, H = bench.make_sparse_problem(m=a.rows, n=a.cols)
    m, n, r = W.shape[0], H.shape[1], W.shape[1]
    print(f"CSR {m} x {n}, nnz {len(val)} ({100.0 * len(val) / m / n:.2f} %), r = {r}, fp32")
    forms = (("frobenius (yardstick)", dict()), ("beta 1 (kl)", dict(missing_divergence="kl")), ("beta 0 (is)", dict(missing_divergence="is")),
             ("beta 0.5 (general)", dict(missing_divergence="beta", missing_beta=0.5)))
    for name, kw in forms:
        eng = na.Engine(m, n, r, "mu", missing_values=True, **kw)
        eng.upload_sparse(1, val, ptr, idx, 0)
        eng.set_factors(W, H)
        eng.iterate(a.warmup, first_iteration=1, error_every=0, last_iteration=0)
        plain = time_block(eng, a.iters, 0)
        err = time_block(eng, a.iters, 1)
        eng.kernel_timing(1)
        eng.iterate(a.iters, first_iteration=1, error_every=0, last_iteration=0)
        _, _, idle, (ms_h, ms_w), (c_h, c_w) = eng.kernel_timing_read3()
        eng.kernel_timing(0)
        rp = eng.geometry()["padded_rank"]
        h, w = ms_h / max(c_h, 1), ms_w / max(c_w, 1)
        # one gathered factor row of RP fp32 values per stored entry and half-step
        tb = [len(val) * rp * 4 / (ms * 1e-3) / 1e12 for ms in (h, w)]
        print(f"{name:>22}: {plain:.3f} ms / iteration, {err:.3f} ms / error iteration; H side {h:.3f} ms ({tb[0]:.2f} TB/s of factor rows), "
              f"W side {w:.3f} ms ({tb[1]:.2f} TB/s) per launch bracket (idle event pair {idle:.4f} ms)")
        eng.close()


if __name__ == "__main__":
    main()
