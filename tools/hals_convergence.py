"""usage: python tools/hals_convergence.py [ITERS] [--sweeps-h 1,2,4 --sweeps-w 1,2,4] [--sweep-tolerance 0.3,0.1] [--nenmf-steps 8,16,32] [--nenmf-step-tolerance 0.3,0.1]      (on the GPU box)
HALS against the multiplicative update from the same start: the relative error ||V - W H|| / ||V|| every 10th iteration up to ITERS (default 1000), the
iterations each algorithm needs to reach the error MU has after ITERS, and the unprofiled wall time per iteration (200 iterations without error terms) -- so
the time to that error.  Two problems: planted (V = W0 H0 + 0.01 noise, 2 000 x 1 500, r = 20) and config 2's random shape (10 000 x 5 000, r = 64).
--sweeps-h / --sweeps-w: comma lists of equal length, one HALS row per pair of sweep counts (accelerated HALS, docs/HALS.md "Inner sweeps"; default 1 / 1).
Per problem the tool also times an iteration at (1, 1), (2, 1), (1, 2), (5, 1) and (1, 5): the differences are what one more H sweep and one more W sweep cost
inside the launch, the figures Gillis & Glineur's rule s = 1 + alpha rho (--alpha, default 0.5) takes its rho from; one more HALS row runs at the counts the
rule gives, rounded to the nearest integer, unless they are among the given pairs.
--sweep-tolerance: a comma list of tolerances delta of the per-column dynamic stopping rule (docs/HALS.md, "Dynamic stopping"); every given pair of counts is run
once more per delta as MAXIMUM counts, and the row shows the mean number of sweeps a column of H and a row of W took per step (sampled at every 10th iteration,
up to the iteration that reaches the target) next to the timings.  docs/HALS.md records the output.
--nenmf-steps: a comma list of step counts T; one NeNMF row (docs/NENMF.md) per value at (T, T), from the same start and to the same target, timed like the HALS
rows.  --nenmf-step-tolerance: a comma list of tolerances delta of NeNMF's per-column stopping rule (docs/NENMF.md, "Dynamic stopping"); every T runs once more
per delta as a MAXIMUM count, with the mean number of steps per column as for --sweep-tolerance.  docs/NENMF.md records that output."""
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


def curve(alg, V, W, H, iters, sweeps=(1, 1), tol=0.0, target=None, steps=None, step_tol=0.0):
    """([(iteration, relative error)], microseconds per iteration, [(mean H count, mean W count)] per error point or None without a tolerance, and with a target
    the wall time in ms of a run from the start to the first error point at or below it, without error terms: median of three -- with a tolerance the
    iterations of a run do not cost the same, so iterations x time per iteration is only an estimate there)"""
    m, n = V.shape
    kw = dict(steps_h=steps[0], steps_w=steps[1]) if steps is not None else {}      # (steps: the counts of a "nenmf" engine; step_tol: its tolerance)
    if step_tol > 0:
        kw["step_tolerance"] = step_tol
    eng = na.Engine(m, n, W.shape[1], alg, sweeps_h=sweeps[0], sweeps_w=sweeps[1], sweep_tolerance=tol, **kw)
    eng.upload(V)
    eng.set_factors(W, H)
    nv = float(np.linalg.norm(V.astype(np.float64)))
    out, counts = [], [] if tol > 0 or step_tol > 0 else None
    for it in range(10, iters + 1, 10):
        eng.iterate(10, first_iteration=it - 9, error_every=10)
        out.append((it, eng.frobenius / nv))
        if tol > 0:
            counts.append((float(eng.sweep_counts(0).mean()), float(eng.sweep_counts(1).mean())))
        elif step_tol > 0:
            counts.append((float(eng.step_counts(0).mean()), float(eng.step_counts(1).mean())))
    eng.set_factors(W, H)
    eng.iterate(20, error_every=0)
    eng.synchronize()
    t0 = time.perf_counter()
    eng.iterate(200, first_iteration=21, error_every=0)
    eng.synchronize()
    us = (time.perf_counter() - t0) / 200 * 1e6
    direct = None
    it = first_below(out, target) if target is not None else None
    if it:
        runs = []
        for _ in range(3):
            eng.set_factors(W, H)
            eng.synchronize()
            t0 = time.perf_counter()
            eng.iterate(it, first_iteration=1, error_every=0)
            eng.synchronize()
            runs.append((time.perf_counter() - t0) * 1e3)
        direct = float(np.median(runs))
    eng.close()
    return out, us, counts, direct


def first_below(c, target):
    return next((it for it, e in c if e <= target), None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("iters", nargs="?", type=int, default=1000)
    ap.add_argument("--sweeps-h", default="1")
    ap.add_argument("--sweeps-w", default="1")
    ap.add_argument("--sweep-tolerance", default="", help="comma list of tolerances of the dynamic stopping rule; each pair of counts runs once more per value, as maximum counts")
    ap.add_argument("--alpha", type=float, default=0.5, help="the alpha of Gillis & Glineur's rule s = 1 + alpha rho; one more HALS row runs at the counts it gives")
    ap.add_argument("--nenmf-steps", default="", help="comma list of step counts T: one NeNMF row per value at (T, T)")
    ap.add_argument("--nenmf-step-tolerance", default="", help="comma list of tolerances of NeNMF's stopping rule; each T runs once more per value, as a maximum count")
    a = ap.parse_args()
    iters = a.iters
    pairs = list(zip((int(x) for x in a.sweeps_h.split(",")), (int(x) for x in a.sweeps_w.split(","))))
    if len(a.sweeps_h.split(",")) != len(a.sweeps_w.split(",")):
        raise SystemExit("--sweeps-h and --sweeps-w need lists of equal length")
    tols = [float(x) for x in a.sweep_tolerance.split(",") if x]
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
        cm, us_mu, _, _ = curve("mu", V, W, H, iters)
        target = cm[-1][1]
        rows = [("MU", cm, us_mu, None, None)]
        for sw in pairs:
            ch, us_h, _, direct = curve("hals", V, W, H, iters, sw, target=target)
            rows.append(("HALS" if sw == (1, 1) else f"HALS {sw[0]},{sw[1]}", ch, us_h, None, direct))
            for tol in tols if sw != (1, 1) else []:
                ch, us_h, counts, direct = curve("hals", V, W, H, iters, sw, tol, target)
                rows.append((f"HALS <={sw[0]},<={sw[1]} delta {tol:g}", ch, us_h, counts, direct))
        print(f"== {name}: relative error of MU after {iters} iterations {target:.6e}")
        base, dh, dw, dh4, dw4 = sweep_costs(V, W, H)
        print(f"  HALS iteration at (1, 1) {base:.1f} us; one more H sweep {dh:+.1f} us (mean of four more {dh4:+.1f}), one more W sweep {dw:+.1f} us (mean of four more {dw4:+.1f})")
        # Gillis & Glineur's static rule s = 1 + alpha rho, rho = cost of a factor's products / cost of its sweep: the products (and whatever else is not a sweep)
        # taken as half of the iteration without its two sweeps each, a sweep as the mean cost of one more in the launch
        rest = max(base - dh4 - dw4, 0.0) / 2
        rule = tuple(int(min(64, max(1, round(1 + a.alpha * rest / max(d, 1e-3))))) for d in (dh4, dw4))
        print(f"  rule (alpha = {a.alpha}): rho_H = {rest / max(dh4, 1e-3):.2f}, rho_W = {rest / max(dw4, 1e-3):.2f} -> sweeps ({rule[0]}, {rule[1]})")
        if rule not in pairs:
            ch, us_h, _, direct = curve("hals", V, W, H, iters, rule, target=target)
            rows.append((f"HALS {rule[0]},{rule[1]}", ch, us_h, None, direct))
        for T in (int(x) for x in a.nenmf_steps.split(",") if x):
            cn, us_n, _, direct = curve("nenmf", V, W, H, iters, target=target, steps=(T, T))
            rows.append((f"NeNMF {T},{T}", cn, us_n, None, direct))
            for delta in (float(x) for x in a.nenmf_step_tolerance.split(",") if x):
                cn, us_n, counts, direct = curve("nenmf", V, W, H, iters, target=target, steps=(T, T), step_tol=delta)
                rows.append((f"NeNMF <={T},<={T} delta {delta:g}", cn, us_n, counts, direct))
        for alg, c, us, counts, direct in rows:
            it = first_below(c, target)
            at = {k: e for k, e in c}
            pts = " ".join(f"{k}:{at[k]:.5e}" for k in (10, 20, 50, 100, 200, 500, 1000) if k in at)
            mean = ""
            if counts:
                upto = counts[:it // 10] if it else counts
                mean = f" mean sweeps per step H {np.mean([h for h, _ in upto]):.2f} W {np.mean([w for _, w in upto]):.2f} (last sample {counts[-1][0]:.2f} / {counts[-1][1]:.2f});"
            timed = f" (timed from the start: {direct:.1f} ms)" if direct is not None else ""
            print(f"  {alg:28s} {us:8.1f} us/iteration;{mean} reaches it after {it} iterations = {it * us / 1e3 if it else float('nan'):.1f} ms{timed}; {pts}")
    na.finalize()


if __name__ == "__main__":
    main()
