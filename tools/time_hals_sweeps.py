"""usage: python tools/time_hals_sweeps.py [--other PATH/libnmfgpu64.so] [--ranks 64,128] [--sweeps 1,2,4]      (on the GPU box)
Wall time per HALS iteration at 10 000 x 5 000, fp32, with s sweeps per product in both steps (docs/HALS.md, "Inner sweeps"): five runs of 200 iterations each
(after 20 warm-up iterations), every configuration in turn within a round, all in one process; prints the runs, the median and the range.  --other: another build
of the library (the commit before a change, say) runs at (1, 1) in the same rounds, so that the two are compared under the same conditions."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nmfgpu_amd as na  # noqa: E402
from nmfgpu_amd import _lib  # noqa: E402


def run(eng, W, H, count=200):
    eng.set_factors(W, H)
    eng.iterate(20, error_every=0)
    eng.synchronize()
    t0 = time.perf_counter()
    eng.iterate(count, first_iteration=21, error_every=0)
    eng.synchronize()
    return (time.perf_counter() - t0) / count * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", default=None)
    ap.add_argument("--other-last", action="store_true", help="create and time the other build's engine after this build's, not before (an engine's place in the order can show)")
    ap.add_argument("--ranks", default="64,128")
    ap.add_argument("--sweeps", default="1,2,4")
    a = ap.parse_args()
    m, n = 10000, 5000
    rng = np.random.default_rng(1)
    V = np.asfortranarray(rng.random((m, n)).astype(np.float32))
    for r in (int(x) for x in a.ranks.split(",")):
        W = np.asfortranarray((1.0 - rng.random((m, r))).astype(np.float32))
        H = np.asfortranarray((1.0 - rng.random((r, n))).astype(np.float32))
        engines = {}

        def other():
            if a.other:
                with _lib.use_library(a.other):      # (an engine keeps the library it was created with)
                    engines["other (1,1)"] = na.Engine(m, n, r, "hals")

        if not a.other_last:
            other()
        for s in (int(x) for x in a.sweeps.split(",")):
            engines[f"this ({s},{s})"] = na.Engine(m, n, r, "hals", sweeps_h=s, sweeps_w=s)
        if a.other_last:
            other()
        for e in engines.values():
            e.upload(V)
        times = {k: [] for k in engines}
        for _ in range(5):
            for k, e in engines.items():
                times[k].append(run(e, W, H))
        for k, v in times.items():
            print(f"r = {r:3d} {k:13s} median {np.median(v):7.1f} us / iteration, range {min(v):7.1f} ... {max(v):7.1f}; runs {' '.join(f'{x:.1f}' for x in v)}", flush=True)
        for e in engines.values():
            e.close()


if __name__ == "__main__":
    main()
