#!/usr/bin/env python3
"""The EI control variate measured at the BO loop's size: Branin, d = 2, M = 200
samples × 9 restarts (the 8 points of generate_batch(6) and the incumbent's), 16 inner starts.

  --ratios   (a) the variance ratio std_cv²/std_plain² of the value and of each gradient component,
             per restart, on the surrogates of a recorded 5-step BO run (20 initial observations, so
             N = 20 … 24, fmini over the observed points; the run itself uses the plain estimator),
             for h = 1 and 2.  A series whose control is constant (β = 0: EI0 underflows there) keeps
             the plain row; they are counted and reported apart from the series with β ≠ 0.
  --solve    (b) one rollout_solve_multi call (device_solve=True, S = 4 surrogates, N = 20, 25
             iterations so that all its launches fit the timing ring) with the switch on against off,
             the two alternating, median of --reps after --warmup, the off path's max − min as
             spread; the control launches' share of the call's kernel time from mrbo_kernel_times
             (with the switch on the ring holds rollout, control, rollout, control, …).
  --loop     (c) bayesopt.run on Branin, 16 lockstep trials, budget 5, h = 1, EI, device_solve=True:
             final gaps and wall time, on and off (the second of two runs each).

One JSON line per row, appended to --out as well.

    python tools/bench_control_variate.py --ratios --solve --loop --out profiles/control_variate/bench.jsonl
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

D, N, M, BATCH, STARTS = 2, 20, 200, 6, 14      # R = 6 + 2 + the incumbent = 9; 14 + 2 inner starts
DEV = "cuda:0"


def emit(line, out):
    s = json.dumps(line)
    print(s, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(s + "\n")


def branin_surrogates(S, n=N, spare=0):
    from mrbo import testfns
    from mrbo.decision_rules import EI
    from mrbo.kernels import Matern52
    from mrbo.surrogates import Surrogate
    tf = testfns.TestBraninHoo()
    lbs, ubs = tf.get_bounds()
    out = []
    for q in range(S):
        rng = np.random.default_rng(1906 + q)
        X = lbs[:, None] + (ubs - lbs)[:, None] * rng.random((D, n))
        out.append(Surrogate(Matern52((1.0,)), X, tf(X), capacity=n + spare, decision_rule=EI(), σn2=1e-6))
    return out, lbs, ubs, tf


def ratios(a):
    import torch
    from mrbo import bayesopt
    from mrbo.engine import initial_guesses, rnstream, to_device
    from mrbo.rollout import _plan_for
    from mrbo.utils import generate_batch
    for h in (1, 2):
        (sur,), lbs, ubs, tf = branin_surrogates(1, spare=5)
        sur.fmini_over_capacity = False     # fmini over the observed points: over the zero-padded buffer (Q3) it
        # is 0 < min Branin, EI0 underflows on the whole box and no series has a control
        rn, xs = rnstream(M, D, h + 1), initial_guesses(STARTS, lbs, ubs)
        per_step = []
        for step in range(5):
            batch = np.hstack([generate_batch(BATCH, lbs, ubs), bayesopt.incumbent_start(sur, lbs, ubs)[:, None]])
            R = batch.shape[1]
            plan = _plan_for(sur, h, M, R, xs.shape[1], lbs, ubs, 0.0, 0, {})
            dx0, drn, dxs = to_device(batch, DEV), to_device(rn, DEV), to_device(xs, DEV)
            out = plan.alloc_outputs(with_gradient=True)
            plan.simulate(dx0, drn, dxs, out)
            ctl = plan.simulate_control(dx0, drn, dxs)
            eto, beta = plan.eto_cv(dx0, out, ctl)
            plain = plan.eto(out)
            torch.cuda.synchronize()
            W = 2 + 2 * D + 2
            eto, plain = (t.cpu().numpy().reshape((W, R), order="F").T for t in (eto, plain))
            beta = beta.cpu().numpy().reshape((1 + D, R), order="F").T               # R×(1+d)
            cols = [1] + list(range(2 + D, 2 + 2 * D))
            with np.errstate(all="ignore"):
                ratio = (eto[:, cols] / plain[:, cols]) ** 2
            per_step.append(dict(step=step, N=int(sur.observed), ratio=ratio, use=beta != 0.0))
            xnext, _ = bayesopt.rollout_solve(sur, lbs, ubs, h, M, BATCH, STARTS, 50, 0.0, eta=0.01, solver="adam",
                                              device_solve=True)
            sur.condition(xnext, float(tf.f(xnext)))
        ratio = np.concatenate([s["ratio"] for s in per_step])                      # (5·R)×(1+d)
        use = np.concatenate([s["use"] for s in per_step])
        names = ["value"] + [f"grad_{k}" for k in range(D)]
        line = dict(bench="control_variate_ratios", fn="braninhoo", d=D, N=[s["N"] for s in per_step], M=M,
                    R=int(ratio.shape[0] // 5), h=h, steps=5)
        for k, name in enumerate(names):
            r_use = ratio[use[:, k], k]
            r_all = np.where(use[:, k], ratio[:, k], 1.0)
            line[name] = dict(series=int(use.shape[0]), with_control=int(use[:, k].sum()),
                              median_with_control=float(np.median(r_use)) if r_use.size else None,
                              mean_with_control=float(r_use.mean()) if r_use.size else None,
                              min=float(r_use.min()) if r_use.size else None,
                              max=float(r_use.max()) if r_use.size else None,
                              mean_all=float(r_all.mean()), median_all=float(np.median(r_all)))
        emit(line, a.out)


def solve(a):
    from mrbo import bayesopt
    from mrbo.rollout import _plan_for_multi
    S, iters = 4, 25
    for h in (1, 2):
        surs, lbs, ubs, _ = branin_surrogates(S)
        plan = _plan_for_multi(surs, h, M, BATCH + 3, STARTS + 2, lbs, ubs, 0.0, 0, {})
        for solver, eta in (("sga", 0.01), ("adam", 0.01)):

            def one(on):
                trace = []
                t0 = time.perf_counter()
                bayesopt.rollout_solve_multi(surs, lbs, ubs, h, M, BATCH, STARTS, iters, 0.0, eta=eta, solver=solver,
                                             trace=trace, device_solve=True, variance_reduction=on)
                wall = (time.perf_counter() - t0) * 1e3
                launched = trace[0]["result"][0] + 1                   # + the final evaluation
                kt = plan.kernel_times((2 if on else 1) * launched)
                rollout = sum(kt[0::2]) if on else sum(kt)
                control = sum(kt[1::2]) if on else 0.0
                return wall, rollout, control, trace[0]["result"]

            for _ in range(a.warmup):
                one(True)
                one(False)
            on, off = [], []
            for _ in range(a.reps):
                on.append(one(True))
                off.append(one(False))
            med = lambda rows, k: statistics.median(r[k] for r in rows)
            w_on, w_off = med(on, 0), med(off, 0)
            spread = max(r[0] for r in off) - min(r[0] for r in off)
            emit(dict(bench="control_variate_solve", fn="braninhoo", d=D, N=N, M=M, R=BATCH + 3, S=S, h=h, solver=solver,
                      eta=eta, iterations=iters, reps=a.reps, on_ms=w_on, off_ms=w_off, time_ratio=w_on / w_off,
                      off_spread_ms=spread, on_ms_min_max=[min(r[0] for r in on), max(r[0] for r in on)],
                      off_ms_min_max=[min(r[0] for r in off), max(r[0] for r in off)],
                      on_rollout_kernel_ms=med(on, 1), on_control_kernel_ms=med(on, 2),
                      control_share_of_rollout=med(on, 2) / med(on, 1), off_rollout_kernel_ms=med(off, 1),
                      on_result=list(on[-1][3]), off_result=list(off[-1][3]),
                      timing="wall clock of one rollout_solve_multi call (device_solve=True), median of reps, on and "
                      "off alternating; kernel ms: HIP events around each launch (mrbo_kernel_times)"), a.out)


def loop(a):
    from mrbo import bayesopt
    quiet = lambda *_: None
    for on in (False, True):
        for rep in range(2):
            with tempfile.TemporaryDirectory() as tmp:
                t0 = time.perf_counter()
                res = bayesopt.run("braninhoo", tmp, budget=5, trials=16, parallel_trials=16, horizon=1, rules=("ei",),
                                   reuse_surrogate=False, log=quiet, device_solve=True, variance_reduction=on)
                wall = time.perf_counter() - t0
            gaps = np.array([res[k]["gaps"][-1] for k in sorted(res)])
            emit(dict(bench="control_variate_loop", fn="braninhoo", trials=16, budget=5, h=1, rule="ei",
                      variance_reduction=on, run=rep + 1, wall_s=wall, final_gap_mean=float(gaps.mean()),
                      final_gap_median=float(np.median(gaps)), final_gaps=[float(g) for g in gaps]), a.out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ratios", action="store_true")
    ap.add_argument("--solve", action="store_true")
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--reps", type=int, default=5, help="timed solves per side (at least 5)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    if a.reps < 5:
        sys.exit("--reps: at least 5")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_control_variate.py needs a GPU: a timing taken without one says nothing")
    if not (a.ratios or a.solve or a.loop):
        a.ratios = a.solve = a.loop = True
    if a.ratios:
        ratios(a)
    if a.solve:
        solve(a)
    if a.loop:
        loop(a)


if __name__ == "__main__":
    main()
