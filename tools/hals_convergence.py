"""usage: python tools/hals_convergence.py [ITERS]      (on the GPU box)
HALS against the multiplicative update from the same start: the relative error ||V - W H|| / ||V|| every 10th iteration up to ITERS (default 1000), the
iterations each algorithm needs to reach the error MU has after ITERS, and the unprofiled wall time per iteration (200 iterations without error terms) -- so
the time to that error.  Two problems: planted (V = W0 H0 + 0.01 noise, 2 000 x 1 500, r = 20) and config 2's random shape (10 000 x 5 000, r = 64).
docs/HALS.md records the output."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nmfgpu_amd as na  # noqa: E402


def curve(alg, V, W, H, iters):
    m, n = V.shape
    eng = na.Engine(m, n, W.shape[1], alg)
    eng.upload(V)
    eng.set_factors(W, H)
    nv = float(np.linalg.norm(V.astype(np.float64)))
    out = []
    for it in range(10, iters + 1, 10):
        eng.iterate(10, first_iteration=it - 9, error_every=10)
        out.append((it, eng.frobenius / nv))
    eng.set_factors(W, H)
    eng.iterate(20, error_every=0)
    eng.synchronize()
    t0 = time.perf_counter()
    eng.iterate(200, first_iteration=21, error_every=0)
    eng.synchronize()
    us = (time.perf_counter() - t0) / 200 * 1e6
    eng.close()
    return out, us


def first_below(c, target):
    return next((it for it, e in c if e <= target), None)


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    na.initialize()
    na.set_verbosity(na.Verbosity.Nothing)
    rng = np.random.default_rng(21)
    problems = []
    m, n, r = 2000, 1500, 20
    V = np.asfortranarray((rng.random((m, r)) @ rng.random((r, n)) + 0.01 * rng.random((m, n))).astype(np.float32))
    problems.append(("planted 2000 x 1500, r = 20", V, r))
    m, n, r = 10000, 5000, 64
    problems.append(("random 10000 x 5000, r = 64 (config 2)", np.asfortranarray(rng.random((m, n)).astype(np.float32)), r))
    for name, V, r in problems:
        m, n = V.shape
        W = np.asfortranarray(rng.random((m, r)).astype(np.float32))
        H = np.asfortranarray(rng.random((r, n)).astype(np.float32))
        cm, us_mu = curve("mu", V, W, H, iters)
        ch, us_h = curve("hals", V, W, H, iters)
        target = cm[-1][1]
        print(f"== {name}: relative error of MU after {iters} iterations {target:.6e}")
        for alg, c, us in (("MU", cm, us_mu), ("HALS", ch, us_h)):
            it = first_below(c, target)
            at = {k: e for k, e in c}
            pts = " ".join(f"{k}:{at[k]:.5e}" for k in (10, 20, 50, 100, 200, 500, 1000) if k in at)
            print(f"  {alg:5s} {us:8.1f} us/iteration; reaches it after {it} iterations = {it * us / 1e3 if it else float('nan'):.1f} ms; {pts}")
    na.finalize()


if __name__ == "__main__":
    main()
