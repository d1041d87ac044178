"""Times of Engine.score (docs/PREDICT.md) on the coordinates of BASELINE config 3 (100 000 x 20 000, 1 % stored, r = 128, fp32) against what a caller had before
it: get_factors plus a numpy loop over the entries.  One process, one masked KL engine after a few iterations; every step runs under a time limit of its own
(--step-limit seconds: the process ends there, nothing is retried).

Prints, for the coordinates in CSR order and in shuffled order:
  the wall time of score() on device arrays (a host clock around calls that end in a stream synchronise; it holds the validation launch, the gather launch and
  the two synchronisations between them) and on host arrays (staging of 12 bytes per entry included);
  with --events, the time between two device events around the same call (what the device was busy or waited on);
and once: get_factors() plus the numpy evaluation of the same five results, checked against score()'s.
The kernel time proper is the k_predict_entries row of a `rocprofv3 --kernel-trace --stats` run of this script (--profile-run: device arrays only, few repeats).

    python tools/time_predict.py [--reps 20] [--rows 100000] [--cols 20000] [--step-limit 300] [--profile-run]
"""
import argparse
import os
import signal
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench
import nmfgpu_amd as na


class step:
    """with step("name", limit): the body under an alarm of `limit` seconds; a step that runs out ends the process."""

    def __init__(self, name, limit):
        self.name, self.limit = name, int(limit)

    def __enter__(self):
        def out(signum, frame):
            print(f"step '{self.name}' ran past its limit of {self.limit} s", flush=True)
            os._exit(124)
        signal.signal(signal.SIGALRM, out)
        signal.alarm(self.limit)
        self.t0 = time.perf_counter()
        return self

    def __exit__(self, *exc):
        signal.alarm(0)
        print(f"[{self.name}: {time.perf_counter() - self.t0:.1f} s]", flush=True)
        return False


def host_evaluation(eng, rows, cols, vals, beta, chunk=1 << 16):
    """What a caller has without score(): both factors come down, numpy gathers and adds."""
    W, H = eng.get_factors()
    Ht = np.ascontiguousarray(H.T)
    eps = np.float32(np.finfo(np.float32).eps)
    sq = div = 0.0
    for s in range(0, len(rows), chunk):
        p = np.einsum("ij,ij->i", W[rows[s:s + chunk]], Ht[cols[s:s + chunk]])
        v = vals[s:s + chunk]
        sq += float(((v - p).astype(np.float64) ** 2).sum())
        q = (p + eps).astype(np.float64)
        v = v.astype(np.float64)
        div += float((np.where(v > 0, v * np.log(np.where(v > 0, v, 1.0) / q), 0.0) - v + q).sum())
    assert beta == 1.0
    return sq, div


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", type=int, default=bench.C3["rows"])
    ap.add_argument("--cols", type=int, default=bench.C3["columns"])
    ap.add_argument("--step-limit", type=int, default=300)
    ap.add_argument("--profile-run", action="store_true", help="device arrays only, three calls per order: the run to put under rocprofv3 --kernel-trace --stats")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available() or na.device_count() < 1:
        raise SystemExit("time_predict.py needs a HIP device: nothing here falls back to the CPU")

    with step("problem", a.step_limit):
        val, ptr, idx, W, H = bench.make_sparse_problem(m=a.rows, n=a.cols)
        m, n, r = W.shape[0], H.shape[1], W.shape[1]
        nnz = len(val)
        rows = np.repeat(np.arange(m, dtype=np.int32), np.diff(ptr))
        perm = np.random.default_rng(2).permutation(nnz)
        orders = {"CSR order": (rows, idx, val), "shuffled": (rows[perm], idx[perm], val[perm])}
        print(f"{m} x {n}, nnz {nnz} ({100.0 * nnz / m / n:.2f} %), r = {r}, fp32; per call {nnz * 2 * 128 * 4 / 1e9:.2f} GB of gathered factor rows "
              f"+ {nnz * 12 / 1e9:.2f} GB of coordinates and values", flush=True)
    with step("engine", a.step_limit):
        eng = na.Engine(m, n, r, "mu", missing_values=True, missing_divergence="kl")
        eng.upload_sparse(1, val, ptr, idx, 0)
        eng.set_factors(W, H)
        eng.iterate(5, first_iteration=1, error_every=0, last_iteration=5)
        print(f"engine: padded rank {eng.geometry()['padded_rank']}, its own KL over the stored entries {eng.divergence_value:.6e}", flush=True)

    results = {}
    for name, (rr, cc, vv) in orders.items():
        with step(f"score, {name}", a.step_limit):
            d = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (rr, cc, vv)]
            torch.cuda.synchronize()
            first = eng.score(*d, beta=1.0)      # (warm-up: code objects, the engine's buffers)
            reps = 3 if a.profile_run else a.reps
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
            t0 = time.perf_counter()
            for s, e in ev:
                s.record()
                got = eng.score(*d, beta=1.0)
                e.record()
            torch.cuda.synchronize()
            wall_dev = (time.perf_counter() - t0) / reps * 1e3
            ev_ms = sorted(s.elapsed_time(e) for s, e in ev)
            assert got == first, "score is not bit-identical between calls"
            line = f"{name:>10}: score on device arrays {wall_dev:.3f} ms / call (wall), {ev_ms[len(ev_ms) // 2]:.3f} ms median between device events"
            if not a.profile_run:
                eng.score(rr, cc, vv, beta=1.0)
                t0 = time.perf_counter()
                for _ in range(max(a.reps // 4, 2)):
                    host = eng.score(rr, cc, vv, beta=1.0)
                wall_host = (time.perf_counter() - t0) / max(a.reps // 4, 2) * 1e3
                assert host == got, "host and device arrays give different bits"
                line += f"; on host arrays {wall_host:.3f} ms / call"
            print(line + f"; div {got['div']:.6e} sq {got['sq']:.6e} rmsd {got['rmsd']:.6f}", flush=True)
            results[name] = got
            del d
    if not a.profile_run:
        with step("get_factors + numpy", a.step_limit):
            rr, cc, vv = orders["CSR order"]
            t0 = time.perf_counter()
            sq, div = host_evaluation(eng, rr, cc, vv, 1.0)
            wall = (time.perf_counter() - t0) * 1e3
            got = results["CSR order"]
            print(f"get_factors + numpy over the same entries: {wall:.0f} ms; div {div:.6e} (score: {got['div']:.6e}, {abs(div - got['div']) / got['abs_div']:.1e} of the "
                  f"absolute summands apart), sq {sq:.6e} ({abs(sq - got['sq']) / got['sq']:.1e} apart)", flush=True)
    eng.close()


if __name__ == "__main__":
    main()
