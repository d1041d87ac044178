"""usage: python tools/hals_convergence.py [ITERS] [--sweeps-h 1,2,4 --sweeps-w 1,2,4]      (on the GPU box)
HALS against the multiplicative update from the same start: the relative error ||V - W H|| / ||V|| every 10th iteration up to ITERS (default 1000), the
iterations each algorithm needs to reach the error MU has after ITERS, and the unprofiled wall time per iteration (200 iterations without error terms) -- so
the time to that error.  Two problems: planted (V = W0 H0 + 0.01 noise, 2 000 x 1 500, r = 20) and config 2's random shape (10 000 x 5 000, r = 64).
--sweeps-h / --sweeps-w: comma lists of equal length, one HALS row per pair of sweep counts (accelerated HALS, docs/HALS.md "Inner sweeps"; default 1 / 1).
Per problem the tool also times an iteration at (1, 1), (2, 1), (1, 2), (5, 1) and (1, 5): the differences are what one more H sweep and one more W sweep cost
inside the launch, the figures Gillis & Glineur's rule s = 1 + alpha rho (--alpha, default 0.5) takes its rho from; one more HALS row runs at the counts the
rule gives, rounded to the nearest integer, unless they are among the given pairs.  docs/HALS.md records the output."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nmfgpu_amd as na  # noqa: E402


def per_iteration_us(eng, W, H, count=200):
    eng.set_factors(W, H)
    eng.iterate(20, error_every=0)
    eng.synchronize()
    t0 = time.perf_counter()
    eng.iterate(count, first_iteration=21, error_every=0)
    eng.synchronize()
    return (time.perf_counter() - t0) / count * 1e6


def sweep_costs(V, W, H):
    """(iteration at (1, 1), one more H sweep, one more W sweep) in microseconds of wall time, medians of five: what an extra in-launch sweep costs."""
    m, n = V.shape
    eng = na.Engine(m, n, W.shape[1], "hals")
    eng.upload(V)
    out = []
    for counts in ((1, 1), (2, 1), (1, 2), (5, 1), (1, 5)):
        eng.set_sweeps(*counts)
        out.append(float(np.median([per_iteration_us(eng, W, H) for _ in range(5)])))
    eng.close()
    base = out[0]
    return base, out[1] - base, out[2] - base, (out[3] - base) / 4, (out[4] - base) / 4


def curve(alg, V, W, H, iters, sweeps=(1, 1)):
    m, n = V.shape
    eng = na.Engine(m, n, W.shape[1], alg, sweeps_h=sweeps[0], sweeps_w=sweeps[1])
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
    ap = argparse.ArgumentParser()
    ap.add_argument("iters", nargs="?", type=int, default=1000)
    ap.add_argument("--sweeps-h", default="1")
    ap.add_argument("--sweeps-w", default="1")
    ap.add_argument("--alpha", type=float, default=0.5, help="the alpha of Gillis & Glineur's rule s = 1 + alpha rho; one more HALS row runs at the counts it gives")
    a = ap.parse_args()
    iters = a.iters
    pairs = list(zip((int(x) for x in a.sweeps_h.split(",")), (int(x) for x in a.sweeps_w.split(","))))
    if len(a.sweeps_h.split(",")) != len(a.sweeps_w.split(",")):
        raise SystemExit("--sweeps-h and --sweeps-w need lists of equal length")
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
        rows = [("MU", cm, us_mu)]
        for sw in pairs:
            ch, us_h = curve("hals", V, W, H, iters, sw)
            rows.append(("HALS" if sw == (1, 1) else f"HALS {sw[0]},{sw[1]}", ch, us_h))
        target = cm[-1][1]
        print(f"== {name}: relative error of MU after {iters} iterations {target:.6e}")
        base, dh, dw, dh4, dw4 = sweep_costs(V, W, H)
        print(f"  HALS iteration at (1, 1) {base:.1f} us; one more H sweep {dh:+.1f} us (mean of four more {dh4:+.1f}), one more W sweep {dw:+.1f} us (mean of four more {dw4:+.1f})")
        # Gillis & Glineur's static rule s = 1 + alpha rho, rho = cost of a factor's products / cost of its sweep: the products (and whatever else is not a sweep)
        # taken as half of the iteration without its two sweeps each, a sweep as the mean cost of one more in the launch
        rest = max(base - dh4 - dw4, 0.0) / 2
        rule = tuple(int(min(64, max(1, round(1 + a.alpha * rest / max(d, 1e-3))))) for d in (dh4, dw4))
        print(f"  rule (alpha = {a.alpha}): rho_H = {rest / max(dh4, 1e-3):.2f}, rho_W = {rest / max(dw4, 1e-3):.2f} -> sweeps ({rule[0]}, {rule[1]})")
        if rule not in pairs:
            ch, us_h = curve("hals", V, W, H, iters, rule)
            rows.append((f"HALS {rule[0]},{rule[1]}", ch, us_h))
        for alg, c, us in rows:
            it = first_below(c, target)
            at = {k: e for k, e in c}
            pts = " ".join(f"{k}:{at[k]:.5e}" for k in (10, 20, 50, 100, 200, 500, 1000) if k in at)
            print(f"  {alg:10s} {us:8.1f} us/iteration; reaches it after {it} iterations = {it * us / 1e3 if it else float('nan'):.1f} ms; {pts}")
    na.finalize()


if __name__ == "__main__":
    main()
