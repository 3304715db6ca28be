#!/usr/bin/env python3
"""The device-resident MLE refit (mrbo_gp_optimize_multi) against the host-driven loop it replaces,
and the BO loops with the refit on either path.

Rows (default): (d, N) = (2, 20), (6, 64), (4, 128) × S = 1, 4, 16, 60 data sets, Matérn-5/2,
σn2 = 1e-6, ℓ₀ = 1, box [0.1, 5].  Per row it times, on the same data sets from the same starts,
  device    one mle.gp_optimize_multi call (host pointers: staging, every round's launches, the
            final copy back and synchronisation), and
  baseline  mle.projected_lbfgs_multi over mle.gp_fit_multi (optimize_multi's minimisation without
            its set_kernel, which both paths run afterwards and which is left out on both sides),
as wall time of a window of `--inner` repetitions divided by `--inner`.  The two alternate `--reps`
times after `--warmup` untimed rounds; medians and min/max are reported, one JSON line per row.
`below_spread` says whether the device median lies below the baseline median minus the baseline's
own min-to-max spread.  rounds / stopped_at are the device call's result; baseline_kernel_ms is the
sum of mrbo_last_gp_fit_ms over the baseline's launches (HIP events around each kernel);
device_kernel_ms_est is an ESTIMATE of the same sum for the device call, which does not time its
launches: the kernel time of one (1, S) launch plus (rounds − 1) × that of one (12, S) launch, both
measured on plain gp_fit_multi calls at the starts.  θ, −ll, gradient and iteration counts of the
two sides are compared once per row before timing (same_bits).

--loops runs the end-to-end pairs instead: run_myopic (budget 10, 16 lockstep trials) and
bayesopt.run (budget 5, 16 lockstep trials, h = 1) on Branin with device_mle off and on, the second
of two runs in one process each; total wall time, the sum of mle_times and its share of the wall.

    python tools/bench_gp_optimize.py [--S 1,4,16,60] [--reps 5] [--inner 10] [--out FILE]
    python tools/bench_gp_optimize.py --loops [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "rollout-bayesian-optimization_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = ((2, 20), (6, 64), (4, 128))
LO, HI = [0.1], [5.0]


def surrogates(S, d, N):
    from mrbo.kernels import Matern52
    from mrbo.surrogates import Surrogate
    out = []
    for q in range(S):
        rng = np.random.default_rng(1000 * d + q)
        X = rng.random((d, N))
        y = np.sin(3 * X.sum(0)) + 0.1 * rng.standard_normal(N)
        out.append(Surrogate(Matern52((1.0,)), X, y, capacity=N, σn2=1e-6))
    return out


def emit(line, out):
    s = json.dumps(line)
    print(s, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(s + "\n")


def rows(a):
    from mrbo import _lib
    from mrbo.mle import _STEPS, gp_fit_multi, gp_optimize_multi, projected_lbfgs_multi
    last_ms = _lib.load().mrbo_last_gp_fit_ms
    for d, N in SHAPES:
        for S in [int(s) for s in a.S.split(",")]:
            surs = surrogates(S, d, N)
            th0 = np.ones((S, 1))

            def run_device():
                return gp_optimize_multi(surs, th0, LO, HI), 0.0

            def run_baseline():
                ms = [0.0]

                def fg_multi(idx, T):
                    r = gp_fit_multi([surs[i] for i in idx], T)
                    ms[0] += last_ms()
                    return np.where(r["status"] == 0, -r["ll"], np.nan), -r["grad"]
                return projected_lbfgs_multi(fg_multi, list(th0), LO, HI), ms[0]

            rd, rb = run_device()[0], run_baseline()[0]
            same = all(rd["theta"][q].tobytes() == rb[q][0].tobytes() and rd["neg_log_likelihood"][q] == rb[q][1]
                       and rd["gradient"][q].tobytes() == rb[q][2].tobytes() and rd["iterations"][q] == rb[q][3]
                       for q in range(S))
            gp_fit_multi(surs, th0[:, :, None])
            k1 = last_ms()
            gp_fit_multi(surs, np.clip(1.0 - 0.5 * _STEPS[None, :, None] * np.ones((S, 1, 1)), LO[0], HI[0]))
            k12 = last_ms()

            def window(fn):
                t0 = time.perf_counter()
                ms = 0.0
                for _ in range(a.inner):
                    ms += fn()[1]
                return (time.perf_counter() - t0) / a.inner * 1e3, ms / a.inner

            for _ in range(a.warmup):
                window(run_device)
                window(run_baseline)
            td, tb, kb = [], [], []
            for _ in range(a.reps):          # alternate: both sides see the same machine
                td.append(window(run_device)[0])
                t, k = window(run_baseline)
                tb.append(t)
                kb.append(k)
            md, mb, spread = statistics.median(td), statistics.median(tb), max(tb) - min(tb)
            emit(dict(bench="gp_optimize", d=d, N=N, S=S, reps=a.reps, inner=a.inner, device_ms=md, baseline_ms=mb,
                      ratio=md / mb, device_ms_min_max=[min(td), max(td)], baseline_ms_min_max=[min(tb), max(tb)],
                      baseline_spread_ms=spread, below_spread=bool(md < mb - spread), rounds=rd["rounds"],
                      stopped_at=rd["stopped_at"], iterations=[int(v) for v in rd["iterations"]],
                      baseline_kernel_ms=statistics.median(kb), device_kernel_ms_est=k1 + (rd["rounds"] - 1) * k12,
                      fit_kernel_ms_1xS=k1, fit_kernel_ms_12xS=k12, same_bits=bool(same),
                      timing="wall clock of host-pointer calls, median of reps windows of inner repetitions each, "
                      "device and baseline alternating; baseline_kernel_ms from HIP events, device_kernel_ms_est an "
                      "estimate (rounds × per-launch kernel time)"), a.out)


def loops(a):
    from mrbo import bayesopt
    quiet = lambda *_: None
    cases = [
        ("run_myopic", lambda dm, out: bayesopt.run_myopic("braninhoo", out, budget=10, trials=16, parallel_trials=16,
                                                           optimize=True, reuse_surrogate=False, device_mle=dm, log=quiet)),
        ("run_h1", lambda dm, out: bayesopt.run("braninhoo", out, budget=5, trials=16, parallel_trials=16, optimize=True,
                                                horizon=1, reuse_surrogate=False, device_mle=dm, log=quiet)),
    ]
    for name, fn in cases:
        ells = {}
        for dm in (False, True):
            for rep in range(2):
                with tempfile.TemporaryDirectory() as tmp:
                    t0 = time.perf_counter()
                    res = fn(dm, tmp)
                    wall = time.perf_counter() - t0
                # one mle_times array per chunk and rule: every trial of the chunk carries a copy
                mle = sum(float(r["mle_times"].sum()) for (acq, trial), r in res.items() if trial == 0)
                ells[dm] = [res[k]["ell_end"] for k in sorted(res)]
                emit(dict(bench="gp_optimize_loops", loop=name, device_mle=dm, run=rep + 1, wall_s=wall, mle_s=mle,
                          mle_share=mle / wall, trials=len(res)), a.out)
        emit(dict(bench="gp_optimize_loops", loop=name, same_final_lengthscales=ells[False] == ells[True]), a.out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--S", default="1,4,16,60")
    ap.add_argument("--reps", type=int, default=5, help="timed windows per side (at least 5)")
    ap.add_argument("--inner", type=int, default=10, help="repetitions inside one timed window (at least 10)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loops", action="store_true", help="the end-to-end BO loops instead of the rows")
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    if a.reps < 5 or a.inner < 10:
        sys.exit("--reps: at least 5, --inner: at least 10")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_gp_optimize.py needs a GPU: a timing taken without one says nothing")
    (loops if a.loops else rows)(a)


if __name__ == "__main__":
    main()
