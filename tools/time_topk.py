"""Times of Engine.top_k (docs/TOPK.md) at the factors of BASELINE config 3 (100 000 x 20 000, 1 % stored, r = 128, fp32) against what a caller had before it:
(a) get_factors plus a blocked numpy product with argpartition, (b) get_factors, the factors uploaded again and torch.topk(Wq @ H, k) over row blocks on the
device.  One process, one masked KL engine after a few iterations; every step runs under a time limit of its own (--step-limit seconds: the process ends there,
nothing is retried).

Prints, for k = 10 and k = 64, all rows as queries, with and without the training entries excluded:
  the wall time of top_k() on device arrays (a host clock around calls that end in a stream synchronise; it holds the validation launch, the product launch, the
  merge launch and the synchronisations) and the median time between two device events around the same call;
and once per k: the two yardsticks, (a) on the first --host-rows rows (scaled to all rows in the printed line, and said so), (b) on all rows; the result of (b) and
of top_k go through the tolerant check of tests/topk_reference.py on --check-rows queries each, not through equality.
The kernel times proper are the k_topk_product and k_topk_merge rows of a `rocprofv3 --kernel-trace --stats` run of this script (--profile-run: device arrays
only, three calls per case, no yardsticks).

    python tools/time_topk.py [--reps 20] [--rows 100000] [--cols 20000] [--step-limit 300] [--profile-run]
"""
import argparse
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench
import nmfgpu_amd as na
from tests import topk_reference as tref


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


def host_top_k(W, H, rows, k, block=2048):
    """Yardstick (a): a blocked numpy product and argpartition per block, the k sorted afterwards."""
    idx = np.empty((rows, k), np.int32); sc = np.empty((rows, k), W.dtype)
    for s in range(0, rows, block):
        S = W[s:s + block] @ H
        part = np.argpartition(-S, k - 1, axis=1)[:, :k]
        ps = np.take_along_axis(S, part, axis=1)
        order = np.argsort(-ps, axis=1, kind="stable")
        idx[s:s + block] = np.take_along_axis(part, order, axis=1); sc[s:s + block] = np.take_along_axis(ps, order, axis=1)
    return idx, sc


def torch_top_k(torch, Wd, Hd, k, block=8192):
    """Yardstick (b): torch.topk of a row block of the product, on the device."""
    idx, sc = [], []
    for s in range(0, Wd.shape[0], block):
        v, i = torch.topk(Wd[s:s + block] @ Hd, k, dim=1)
        idx.append(i.to(torch.int32)); sc.append(v)
    return torch.cat(idx), torch.cat(sc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", type=int, default=bench.C3["rows"])
    ap.add_argument("--cols", type=int, default=bench.C3["columns"])
    ap.add_argument("--host-rows", type=int, default=8192, help="rows of yardstick (a); its time is scaled to all rows")
    ap.add_argument("--check-rows", type=int, default=200)
    ap.add_argument("--step-limit", type=int, default=300)
    ap.add_argument("--profile-run", action="store_true", help="device arrays only, three calls per case: the run to put under rocprofv3 --kernel-trace --stats")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available() or na.device_count() < 1:
        raise SystemExit("time_topk.py needs a HIP device: nothing here falls back to the CPU")

    with step("problem", a.step_limit):
        val, ptr, idx, W, H = bench.make_sparse_problem(m=a.rows, n=a.cols)
        m, n, r = W.shape[0], H.shape[1], W.shape[1]
        nnz = len(val)
        queries = np.arange(m, dtype=np.int32)
        excl = (ptr.astype(np.int64), idx.astype(np.int32))      # the CSR of the training entries is the exclusion list of "all rows, in order"
        print(f"{m} x {n}, nnz {nnz} ({100.0 * nnz / m / n:.2f} %), r = {r}, fp32; {m} queries x {n} candidates = {2.0 * m * n * r / 1e12:.3f} TFLOP, "
              f"a score block of {4.0 * m * n / 1e9:.1f} GB that is never written; slabs {na.top_k_slabs(m, n)}", flush=True)
    with step("engine", a.step_limit):
        eng = na.Engine(m, n, r, "mu", missing_values=True, missing_divergence="kl")
        eng.upload_sparse(1, val, ptr, idx, 0)
        eng.set_factors(W, H)
        eng.iterate(5, first_iteration=1, error_every=0, last_iteration=5)
        print(f"engine: padded rank {eng.geometry()['padded_rank']}", flush=True)
        d_q = torch.from_numpy(queries).cuda()
        d_excl = (torch.from_numpy(excl[0]).cuda(), torch.from_numpy(excl[1]).cuda())
        torch.cuda.synchronize()

    reps = 3 if a.profile_run else a.reps
    results = {}
    for k in (10, 64):
        for name, ex in (("all candidates", None), ("training entries excluded", d_excl)):
            with step(f"top_k, k = {k}, {name}", a.step_limit):
                first = eng.top_k(d_q, k, exclude=ex)      # (warm-up: code objects, the engine's buffers)
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
                t0 = time.perf_counter()
                for s, e in ev:
                    s.record()
                    got = eng.top_k(d_q, k, exclude=ex)
                    e.record()
                torch.cuda.synchronize()
                wall = (time.perf_counter() - t0) / reps * 1e3
                ev_ms = sorted(s.elapsed_time(e) for s, e in ev)
                assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1]), "top_k is not bit-identical between calls"
                print(f"k = {k:2d}, {name:>26}: top_k on device arrays {wall:.3f} ms / call (wall), {ev_ms[len(ev_ms) // 2]:.3f} ms median between device events; "
                      f"{2.0 * m * n * r / (ev_ms[len(ev_ms) // 2] * 1e-3) / 1e12:.1f} TFLOP/s of the product", flush=True)
                results[(k, ex is not None)] = (got[0].cpu().numpy(), got[1].cpu().numpy())
    if a.profile_run:
        eng.close()
        return

    with step("get_factors", a.step_limit):
        t0 = time.perf_counter()
        Wf, Hf = eng.get_factors()
        t_get = (time.perf_counter() - t0) * 1e3
        Wc, Hc = np.ascontiguousarray(Wf), np.ascontiguousarray(Hf)
        W64, Ht64 = Wc.astype(np.float64), np.ascontiguousarray(Hc.T.astype(np.float64))
        sample = np.random.default_rng(4).choice(m, min(a.check_rows, m), replace=False).astype(np.int32)
        print(f"get_factors: {t_get:.0f} ms", flush=True)
    u = 2.0 ** -24
    for k in (10, 64):
        with step(f"check of top_k, k = {k}", a.step_limit):
            for with_excl in (False, True):
                gi, gs = results[(k, with_excl)]
                e = None
                if with_excl:
                    e = (np.concatenate([[0], np.cumsum(np.diff(excl[0])[sample])]).astype(np.int64),
                         np.concatenate([excl[1][excl[0][q]:excl[0][q + 1]] for q in sample]).astype(np.int32))
                tref.check_top_k(gi[sample], gs[sample], W64, Ht64, sample, k, e, 0, u)
            print(f"k = {k}: top_k passes check_top_k on {len(sample)} queries, with and without exclusion", flush=True)
        with step(f"(a) numpy, k = {k}", a.step_limit):
            rows = min(a.host_rows, m)
            t0 = time.perf_counter()
            host_top_k(Wc, Hc, rows, k)
            t_a = (time.perf_counter() - t0) * 1e3
            print(f"k = {k}: (a) get_factors + blocked numpy product + argpartition: {t_a:.0f} ms for {rows} rows, i.e. {t_get + t_a * m / rows:.0f} ms for all {m} "
                  f"(scaled by {m / rows:.2f}, get_factors added)", flush=True)
        with step(f"(b) torch.topk, k = {k}", a.step_limit):
            t0 = time.perf_counter()
            Wd, Hd = torch.from_numpy(Wc).cuda(), torch.from_numpy(Hc).cuda()
            torch.cuda.synchronize()
            t_up = (time.perf_counter() - t0) * 1e3
            torch_top_k(torch, Wd, Hd, k)      # (warm-up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                bi, bs = torch_top_k(torch, Wd, Hd, k)
            torch.cuda.synchronize()
            t_b = (time.perf_counter() - t0) / 3 * 1e3
            tref.check_top_k(bi.cpu().numpy()[sample], bs.cpu().numpy()[sample], W64, Ht64, sample, k, None, 0, u)
            print(f"k = {k}: (b) torch.topk(Wq @ H) over row blocks of 8192 on the device: {t_b:.3f} ms / pass over all rows (factors already uploaded: "
                  f"{t_get:.0f} ms down + {t_up:.0f} ms up once); passes check_top_k on {len(sample)} queries", flush=True)
            del Wd, Hd
    eng.close()


if __name__ == "__main__":
    main()
