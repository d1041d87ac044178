"""Iteration times of the dense beta-divergence update (docs/DIVERGENCE.md) on one strictly positive dense V: the dense KL iteration (--mode dense-kl), the
Itakura-Saito iteration (--mode is), the general beta-divergence iteration (--mode beta --beta 0.5), and the KL iteration that takes the sparse route for dense
input (--mode kl: what a build without the dense path runs).  --penalties l1W l1H l2W l2H times the penalised iteration of a dense mode.  --weighted F times
the weighted iteration of a dense mode (docs/DIVERGENCE.md, "Weighted update") with 0 / 1 weights, a share F of them 0 (drawn independently per entry).
--mode masked --weighted F times the gather-path missing-value engine (docs/MISSING.md: Frobenius, missing_values=True) on the same V and the same 0 / 1 weights.
--mixed times the mixed-precision iteration of a dense mode (docs/DIVERGENCE.md, "Mixed precision": bf16 operands).  --objective K [K2 ...] also reports the divergence value
reached K iterations after the start (from the same start, after the timing): the figure to compare a mixed run with an fp32 run by.
--batch-size B [--forget-factor F] times the minibatch form of a dense mode (docs/DIVERGENCE.md, "Minibatch update"): an iteration is then one pass over the
batches, and --objective K reports the divergence value after K passes (of (W, H) after the pass; the full-batch figure is that of (W_{k-1}, H_k)).

One process per run: without --child this script starts --runs fresh child processes one after the other and prints their figures with the median and the
spread.  A child warms up, then times plain iterations and error iterations (wall time per iteration, stream synchronised around each block) and reads the
event-timed H-side / W-side launches (nmfamd_engine_kernel_timing_read3).  NMFAMD_LIBRARY selects the library, so the same script times another build.

    python tools/time_beta.py --mode dense-kl [--beta 0.5] [--penalties 0 0 0 0] [--weighted 0.5] [--mixed] [--batch-size 1024] [--forget-factor 0.7] [--objective 200] [--rows 10000] [--cols 5000] [--rank 64] [--iters 50] [--warmup 10] [--runs 5]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def problem(m, n, r, seed=7):
    import numpy as np
    rng = np.random.default_rng(seed)
    V = (rng.random((m, 5), dtype=np.float32) @ rng.random((5, n), dtype=np.float32)) * rng.gamma(8.0, 1.0 / 8.0, (m, n)).astype(np.float32) + np.float32(1e-3)
    W = (1.0 - rng.random((m, r))).astype(np.float32)
    H = (1.0 - rng.random((r, n))).astype(np.float32)
    return np.asfortranarray(V), np.asfortranarray(W), np.asfortranarray(H)


def time_block(eng, iters, error_every):
    eng.synchronize()
    t0 = time.perf_counter()
    eng.iterate(iters, first_iteration=1, error_every=error_every, last_iteration=0)
    eng.synchronize()
    if error_every:
        eng.frobenius      # (waits for the last error terms and sums them)
    return (time.perf_counter() - t0) / iters * 1e3


def child(a):
    import nmfgpu_amd as na
    V, W, H = problem(a.rows, a.cols, a.rank)
    kw = {"dense-kl": dict(divergence="kl", dense_compute=True), "is": dict(divergence="is"), "kl": dict(divergence="kl"),
          "beta": dict(divergence="beta", beta=a.beta), "masked": {}}[a.mode]
    if any(a.penalties):
        kw.update(l1_w=a.penalties[0], l1_h=a.penalties[1], l2_w=a.penalties[2], l2_h=a.penalties[3])
    if a.mode == "masked":
        import numpy as np
        Om = np.random.default_rng(11).random((a.rows, a.cols), dtype=np.float32) >= np.float32(a.weighted if a.weighted is not None else 0.0)
        V[~Om] = np.nan
        eng = na.Engine(a.rows, a.cols, a.rank, "mu", missing_values=True)
        eng.upload(V)
    elif a.weighted is not None:
        import numpy as np
        Om = np.asfortranarray((np.random.default_rng(11).random((a.rows, a.cols), dtype=np.float32) >= np.float32(a.weighted)).astype(np.float32))
        eng = na.Engine(a.rows, a.cols, a.rank, "mu", weighted=True, **kw)
        eng.upload(V, weights=Om)
    else:
        if a.mixed:
            kw.update(mixed_precision=True)
        if a.batch_size:
            kw.update(batch_size=a.batch_size, forget_factor=a.forget_factor)
        eng = na.Engine(a.rows, a.cols, a.rank, "mu", **kw)
        eng.upload(V)
    eng.set_factors(W, H)
    eng.iterate(a.warmup, first_iteration=1, error_every=0, last_iteration=0)
    plain = time_block(eng, a.iters, 0)
    err = time_block(eng, a.iters, 1)
    eng.kernel_timing(1)
    eng.iterate(a.iters, first_iteration=1, error_every=0, last_iteration=0)
    _, _, idle, (ms_h, ms_w), (c_h, c_w) = eng.kernel_timing_read3()
    eng.kernel_timing(0)
    g = eng.geometry()
    out = {"mode": a.mode, "beta": a.beta if a.mode == "beta" else None, "penalties": a.penalties, "weighted": a.weighted, "mixed": bool(a.mixed), "batch_size": a.batch_size, "forget_factor": a.forget_factor if a.batch_size else None, "rows": a.rows, "cols": a.cols, "rank": a.rank, "ms_iteration": plain, "ms_error_iteration": err, "ms_h_launch": ms_h / max(c_h, 1),
           "ms_w_launch": ms_w / max(c_w, 1), "ms_idle_event_pair": idle, "product_kernel": g["product_kernel"], "slabs_h": g["slabs_h"], "slabs_w": g["slabs_w"],
           "frobenius": eng.frobenius}
    if a.objective:
        # (an error iteration changes nothing an iteration reads, so the later counts continue the run of the earlier ones)
        eng.set_factors(W, H)
        done, values = 0, {}
        for k in sorted(a.objective):
            eng.iterate(k - done, first_iteration=done + 1, error_every=0, last_iteration=k)
            done, values[k] = k, eng.divergence_value
        out["objective_iterations"], out["objective"] = done, values[done]
        if len(values) > 1:
            out["objectives"] = {str(k): v for k, v in values.items()}
    eng.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["dense-kl", "is", "kl", "beta", "masked"], default="dense-kl")
    ap.add_argument("--beta", type=float, default=0.5)
    ap.add_argument("--penalties", type=float, nargs=4, default=[0.0, 0.0, 0.0, 0.0])
    ap.add_argument("--weighted", type=float, default=None, help="share of zero weights of the weighted iteration (0 / 1 weights)")
    ap.add_argument("--mixed", action="store_true", help="the mixed-precision iteration of a dense mode (bf16 operands)")
    ap.add_argument("--batch-size", type=int, default=0, help="the minibatch form of a dense mode: columns per batch (a multiple of 128); an iteration is one pass")
    ap.add_argument("--forget-factor", type=float, default=0.7)
    ap.add_argument("--objective", type=int, nargs="+", default=[], help="also report the divergence value this many iterations after the start (several counts: each of them)")
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--cols", type=int, default=5000)
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    results = []
    for _ in range(a.runs):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--mode", a.mode, "--rows", str(a.rows), "--cols", str(a.cols), "--rank", str(a.rank),
               "--iters", str(a.iters), "--warmup", str(a.warmup), "--beta", str(a.beta), "--penalties", *map(str, a.penalties)]
        if a.weighted is not None:
            cmd += ["--weighted", str(a.weighted)]
        if a.mixed:
            cmd += ["--mixed"]
        if a.batch_size:
            cmd += ["--batch-size", str(a.batch_size), "--forget-factor", str(a.forget_factor)]
        if a.objective:
            cmd += ["--objective", *map(str, a.objective)]
        line = subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True, timeout=600).stdout.strip().splitlines()[-1]
        print(line, flush=True)
        results.append(json.loads(line))
    for key in ("ms_iteration", "ms_error_iteration", "ms_h_launch", "ms_w_launch"):
        vals = [r[key] for r in results]
        print(f"{a.mode}{' ' + str(a.beta) if a.mode == 'beta' else ''}{' weighted ' + str(a.weighted) if a.weighted is not None else ''}{' mixed' if a.mixed else ''}{' batch ' + str(a.batch_size) if a.batch_size else ''} {a.rows} x {a.cols} r {a.rank} {key}: median {statistics.median(vals):.4f} min {min(vals):.4f} max {max(vals):.4f} ({len(vals)} runs)")


if __name__ == "__main__":
    main()
