#!/usr/bin/env python3
"""The acquisition solve of a BO step as one device-resident call (mrbo_rollout_solve) against the
host-driven loop it replaces, and bayesopt.run with the solve on either path.

Rows (default): one acquisition solve of 50 iterations at the BO loop's size -- Branin, d = 2,
N = 20, 200 samples × 9 restarts (the 8 points of generate_batch(6) and the incumbent's), 16 inner
starts -- for h = 1, 2, S = 1, 4, 16 surrogates and both solvers ("sga": StandardSGA η = 0.01,
"adam": BoxAdam η = 0.01 box widths).  Per row it times, on the same surrogates,
  device    bayesopt.rollout_solve_multi(..., device_solve=True): one mrbo_rollout_solve call, and
  host      the same with device_solve=False: the loop of mrbo/utils.py stochastic_solve_multi, the
            final evaluation and pick_restart,
as wall time of one solve.  The two alternate `--reps` times after `--warmup` untimed rounds; medians
and min/max are reported, one JSON line per row.  `below_spread` says whether the device median lies
below the host median minus the host's own min-to-max spread.  Per side the row also carries the
iteration after which no restart was active (the host's history length, the call's result[1]), the
launches made, and the summed rollout-kernel time of one solve's launches (mrbo_kernel_times: HIP
events around each kernel) -- host wall − host kernel time is the overhead the call removes, host
kernel − device kernel time what skipping the stopped restarts saves.  xnext and the means of the
two sides are compared once per row before timing (same_bits).

--loops runs the end-to-end pair instead: bayesopt.run on Branin, 16 lockstep trials, budget 5,
h = 1, three rules, device_solve off and on (--loops-off: off only, for a run on another library),
the second of two runs in one process each.

    python tools/bench_rollout_solve.py [--S 1,4,16] [--h 1,2] [--reps 5] [--out FILE]
    python tools/bench_rollout_solve.py --loops [--out FILE]
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

D, N, M, BATCH, STARTS, ITERS = 2, 20, 200, 6, 14, 50     # R = 6 + 2 + the incumbent = 9; 14 + 2 inner starts
ETA = {"sga": 0.01, "adam": 0.01}


def surrogates(S):
    from mrbo import testfns
    from mrbo.decision_rules import EI
    from mrbo.kernels import Matern52
    from mrbo.surrogates import Surrogate
    tf = testfns.TestBraninHoo()
    lbs, ubs = tf.get_bounds()
    out = []
    for q in range(S):
        rng = np.random.default_rng(1906 + q)
        X = lbs[:, None] + (ubs - lbs)[:, None] * rng.random((D, N))
        out.append(Surrogate(Matern52((1.0,)), X, tf(X), capacity=N, decision_rule=EI(), σn2=1e-6))
    return out, lbs, ubs


def emit(line, out):
    s = json.dumps(line)
    print(s, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(s + "\n")


def rows(a):
    from mrbo import bayesopt
    from mrbo.rollout import _plan_for_multi
    for h in [int(v) for v in a.h.split(",")]:
        for S in [int(v) for v in a.S.split(",")]:
            surs, lbs, ubs = surrogates(S)
            plan = _plan_for_multi(surs, h, M, BATCH + 3, STARTS + 2, lbs, ubs, 0.0, 0, {})   # the solves' plan
            for solver in ("sga", "adam"):

                def solve(device_solve):
                    trace = []
                    t0 = time.perf_counter()
                    picks = bayesopt.rollout_solve_multi(surs, lbs, ubs, h, M, BATCH, STARTS, ITERS, 0.0,
                                                         eta=ETA[solver], solver=solver, trace=trace,
                                                         device_solve=device_solve)
                    wall = (time.perf_counter() - t0) * 1e3
                    t = trace[0]
                    if device_solve:
                        launched, stopped_at = t["result"][0], t["result"][1]
                    else:
                        launched = stopped_at = len(t["history"])
                    kernel = sum(plan.kernel_times(launched + 1))      # + the final evaluation
                    return wall, kernel, launched, stopped_at, picks, t

                dev, host = solve(True), solve(False)
                same = (all(a_[0].tobytes() == b_[0].tobytes() and a_[1] == b_[1] for a_, b_ in zip(dev[4], host[4]))
                        and dev[5]["x"].tobytes() == host[5]["x"].tobytes()
                        and np.asarray(dev[5]["means"]).tobytes() == np.asarray(host[5]["means"]).tobytes())
                for _ in range(a.warmup):
                    solve(True)
                    solve(False)
                td, th, kd, kh = [], [], [], []
                for _ in range(a.reps):          # alternate: both sides see the same machine
                    r = solve(True)
                    td.append(r[0])
                    kd.append(r[1])
                    r = solve(False)
                    th.append(r[0])
                    kh.append(r[1])
                md, mh, spread = statistics.median(td), statistics.median(th), max(th) - min(th)
                emit(dict(bench="rollout_solve", d=D, N=N, M=M, R=BATCH + 3, h=h, S=S, solver=solver, eta=ETA[solver],
                          iterations=ITERS, reps=a.reps, device_ms=md, host_ms=mh, ratio=md / mh,
                          device_ms_min_max=[min(td), max(td)], host_ms_min_max=[min(th), max(th)],
                          host_spread_ms=spread, below_spread=bool(md < mh - spread),
                          device_launched=dev[2], device_stopped_at=dev[3], host_launched=host[2],
                          host_stopped_at=host[3], device_kernel_ms=statistics.median(kd),
                          host_kernel_ms=statistics.median(kh), status_bits=list(dev[5]["result"][2:]),
                          same_bits=bool(same),
                          timing="wall clock of one rollout_solve_multi call, median of reps, device and host "
                          "alternating; kernel_ms: sum of the HIP-event times of the solve's rollout kernels"),
                     a.out)


def loops(a):
    from mrbo import bayesopt
    quiet = lambda *_: None
    Xs = {}
    for ds in ((False,) if a.loops_off else (False, True)):
        for rep in range(2):
            with tempfile.TemporaryDirectory() as tmp:
                kw = dict(device_solve=True) if ds else {}     # off: also what an older library's package takes
                t0 = time.perf_counter()
                res = bayesopt.run("braninhoo", tmp, budget=5, trials=16, parallel_trials=16, horizon=1,
                                   reuse_surrogate=False, log=quiet, **kw)
                wall = time.perf_counter() - t0
            solves = sum(float(r["times"].sum()) for (acq, trial), r in res.items() if trial == 0)
            Xs[ds] = b"".join(res[k]["X"].tobytes() + res[k]["y"].tobytes() for k in sorted(res))
            emit(dict(bench="rollout_solve_loops", loop="run_h1", device_solve=ds, run=rep + 1, wall_s=wall,
                      solve_s=solves, solve_share=solves / wall, trials=len(res), label=a.label), a.out)
    if len(Xs) == 2:
        emit(dict(bench="rollout_solve_loops", loop="run_h1", same_observations=Xs[False] == Xs[True]), a.out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--S", default="1,4,16")
    ap.add_argument("--h", default="1,2")
    ap.add_argument("--reps", type=int, default=5, help="timed solves per side (at least 5)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--loops", action="store_true", help="the end-to-end BO loop instead of the rows")
    ap.add_argument("--loops-off", action="store_true", help="with --loops: the host-driven path only")
    ap.add_argument("--label", default="", help="with --loops: a tag for the JSON lines (which library ran)")
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    if a.reps < 5:
        sys.exit("--reps: at least 5")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_rollout_solve.py needs a GPU: a timing taken without one says nothing")
    (loops if (a.loops or a.loops_off) else rows)(a)


if __name__ == "__main__":
    main()
