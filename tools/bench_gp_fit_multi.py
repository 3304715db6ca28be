#!/usr/bin/env python3
"""One mrbo_gp_fit_multi call against the S plain mrbo_gp_fit_theta calls it replaces, at the size
of one line search of the BO loops' refit.

Shapes: (d, N) = (2, 20), (6, 64), (4, 128); P = 12 candidates per data set (mle._STEPS), S = 4,
16, 60 data sets (Matérn-5/2, σn2 = 1e-6, data sets and lengthscales differ per data set).

Per shape and S it times, with host pointers as the L-BFGS driver calls them,
  multi   one gp_fit_multi over the S surrogates, and
  plain   S gp_fit_batch calls one after another (what the loop over the trials does),
as wall time of a window of `--inner` repetitions divided by `--inner` -- staging, launch, copy
back and the synchronisation every call ends with included, since that is what the loop pays.
The two alternate `--reps` times after `--warmup` untimed rounds; medians and min/max are
reported, one JSON line per (shape, S).  ratio = multi / plain (below 1: the batched call is
faster).  multi_kernel_ms / plain_kernel_ms are mrbo_last_gp_fit_ms of the one launch and the
sum over the S launches (HIP events around the kernels).  Both sides compute the same bits
(checked once per case before timing).

    python tools/bench_gp_fit_multi.py [--S 4,16,60] [--reps 5] [--inner 10] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rollout-bayesian-optimization_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = ((2, 20), (6, 64), (4, 128))
P = 12


def surrogates(S, d, N):
    from mrbo.kernels import Matern52
    from mrbo.surrogates import Surrogate
    out = []
    for q in range(S):
        rng = np.random.default_rng(1000 * d + q)
        X = rng.random((d, N))
        y = np.sin(3 * X.sum(0)) + 0.1 * rng.standard_normal(N)
        out.append(Surrogate(Matern52((1.0,)), X, y, capacity=N, σn2=1e-6))
    th = np.stack([np.sqrt(d) * (0.3 + 0.05 * q % 1.0) * (1.0 + 0.5 ** np.arange(P)) for q in range(S)])
    return out, th


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--S", default="4,16,60")
    ap.add_argument("--reps", type=int, default=5, help="timed windows per side (at least 3)")
    ap.add_argument("--inner", type=int, default=10, help="repetitions inside one timed window")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    if a.reps < 3:
        sys.exit("--reps: at least 3")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_gp_fit_multi.py needs a GPU: a timing taken without one says nothing")
    from mrbo import _lib
    from mrbo.mle import gp_fit_batch, gp_fit_multi
    last_ms = _lib.load().mrbo_last_gp_fit_ms
    for d, N in SHAPES:
        for S in [int(s) for s in a.S.split(",")]:
            surs, th = surrogates(S, d, N)

            def run_multi():
                r = gp_fit_multi(surs, th)
                return r, last_ms()

            def run_plain():
                rs, ms = [], 0.0
                for q, s in enumerate(surs):
                    rs.append(gp_fit_batch(s, th[q]))
                    ms += last_ms()
                return rs, ms

            rm, rp = run_multi()[0], run_plain()[0]
            same = all(rm[k][q].tobytes() == rp[q][k].tobytes() for q in range(S) for k in ("ll", "grad", "status"))

            def window(fn):
                t0 = time.perf_counter()
                ms = 0.0
                for _ in range(a.inner):
                    ms += fn()[1]
                return (time.perf_counter() - t0) / a.inner * 1e3, ms / a.inner

            for _ in range(a.warmup):
                window(run_multi)
                window(run_plain)
            tm, tp, km, kp = [], [], [], []
            for _ in range(a.reps):          # alternate: both sides see the same machine
                t, k = window(run_multi)
                tm.append(t)
                km.append(k)
                t, k = window(run_plain)
                tp.append(t)
                kp.append(k)
            line = dict(bench="gp_fit_multi", d=d, N=N, P=P, S=S, reps=a.reps, inner=a.inner,
                        multi_ms=statistics.median(tm), plain_ms=statistics.median(tp),
                        ratio=statistics.median(tm) / statistics.median(tp),
                        multi_ms_min_max=[min(tm), max(tm)], plain_ms_min_max=[min(tp), max(tp)],
                        multi_kernel_ms=statistics.median(km), plain_kernel_ms=statistics.median(kp),
                        same_bits=bool(same), ok=bool((rm["status"] == 0).all()),
                        timing="wall clock of host-pointer calls (staging, launch, copy back, synchronise), median of "
                        "reps windows of inner repetitions each, multi and plain alternating; kernel_ms from HIP events")
            s = json.dumps(line)
            print(s, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(s + "\n")


if __name__ == "__main__":
    main()
