#!/usr/bin/env python3
"""The fitted output scale measured: the fit launch in plain and in profile mode,
and the BO loops with standardisation off and on.

--fits: one fit call with P = 12 candidates on each of S = 16 data sets at (d, N) = (2, 20), (6, 64)
and (4, 128), Matérn-5/2, σn2 = 1e-6, through the C entry points with host pointers:
  plain         mrbo_gp_fit_multi of this library,
  profile       mrbo_gp_fit_profile_multi of this library,
  parent_plain  mrbo_gp_fit_multi of --parent-lib, a libmrbo.so built from the commit before the
                profile mode (left out without the option).
A sample is the median kernel time (mrbo_last_gp_fit_ms: HIP events around the launch) and the mean
wall time of a window of --inner calls; the sides alternate --reps times after --warmup untimed
rounds.  Per shape one JSON line: medians, min and max per side, whether this library's plain
median lies within the parent's own min-to-max spread, and profile over plain.

--bo: bayesopt.run (EI, 8 lockstep trials, budget 10, optimize, device_mle and device_solve) on
braninhoo, rosenbrock and goldsteinprice at h = 0 and 1, standardize off and on.  Per run one JSON
line: the final gaps (median and quartiles over the trials), the share of (solve, trial) pairs
whose Sobol-batch restarts all start with an exactly zero ETO gradient, and wall time.  The share
comes from one extra rollout launch at the start points before each solve (the rows of the
ascent's first iteration), whose time is taken out of wall_s.

    python tools/bench_standardize.py --fits [--parent-lib PATH] [--out FILE]
    python tools/bench_standardize.py --bo [--out FILE]
"""
import argparse
import ctypes
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
S, P = 16, 12


def emit(line, out):
    s = json.dumps(line)
    print(s, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(s + "\n")


def fits(a):
    from mrbo import _lib
    L = _lib.load()
    parent = None
    if a.parent_lib:
        parent = ctypes.CDLL(a.parent_lib)
        parent.mrbo_gp_fit_multi.argtypes = L.mrbo_gp_fit_multi.argtypes
        parent.mrbo_last_gp_fit_ms.restype = ctypes.c_double
    dp = ctypes.POINTER(ctypes.c_double)
    vp = lambda x: ctypes.c_void_p(x.ctypes.data)
    for d, N in SHAPES:
        keep = []
        for q in range(S):
            rng = np.random.default_rng(1000 * d + q)
            X = np.asfortranarray(rng.random((d, N)))
            y = 300.0 * (np.sin(3 * X.sum(0)) + 0.1 * rng.standard_normal(N))
            keep.append((X, np.ascontiguousarray(y - y.mean())))
        sds = (_lib.SurrogateDesc * S)(*[_lib.SurrogateDesc(d, N, 0, 1.0, 1e-6, 0.0, X.ctypes.data_as(dp), None, N, None,
                                                            y.ctypes.data_as(dp), 1.0) for X, y in keep])
        th = np.ascontiguousarray(np.tile(np.linspace(0.3, 2.0, P) * np.sqrt(d), (S, 1)))
        ll, grad, s2 = np.zeros((S, P)), np.zeros((S, P)), np.zeros((S, P))
        st = np.zeros((S, P), dtype=np.int32)
        H = _lib.MRBO_FLAG_HOST_POINTERS

        def plain(lib):
            def call():
                rc = lib.mrbo_gp_fit_multi(sds, S, P, 1, vp(th), vp(ll), vp(grad), vp(st), None, None, H, None)
                assert rc == 0 and (st == 0).all(), (rc, st)
                return lib.mrbo_last_gp_fit_ms()
            return call

        def profile():
            rc = L.mrbo_gp_fit_profile_multi(sds, S, P, 1, vp(th), vp(ll), vp(grad), vp(s2), vp(st), None, None, H, None)
            assert rc == 0 and (st == 0).all(), (rc, st)
            return L.mrbo_last_gp_fit_ms()

        sides = {"plain": plain(L), "profile": profile}
        if parent is not None:
            sides["parent_plain"] = plain(parent)
            sides["parent_plain"]()
            ref = ll.copy(), grad.copy()
            sides["plain"]()
            same = bool(ref[0].tobytes() == ll.tobytes() and ref[1].tobytes() == grad.tobytes())
        else:
            same = None

        def window(fn):
            t0 = time.perf_counter()
            ks = [fn() for _ in range(a.inner)]
            return statistics.median(ks), (time.perf_counter() - t0) / a.inner * 1e3

        for _ in range(a.warmup):
            for fn in sides.values():
                window(fn)
        ker = {k: [] for k in sides}
        wall = {k: [] for k in sides}
        for _ in range(a.reps):              # alternate: every side sees the same machine
            for k, fn in sides.items():
                km, wm = window(fn)
                ker[k].append(km)
                wall[k].append(wm)
        line = dict(bench="standardize_fit", d=d, N=N, S=S, P=P, reps=a.reps, inner=a.inner)
        for k in sides:
            line[f"{k}_kernel_ms"] = statistics.median(ker[k])
            line[f"{k}_kernel_ms_min_max"] = [min(ker[k]), max(ker[k])]
            line[f"{k}_wall_ms"] = statistics.median(wall[k])
            line[f"{k}_wall_ms_min_max"] = [min(wall[k]), max(wall[k])]
        line["profile_over_plain_kernel"] = line["profile_kernel_ms"] / line["plain_kernel_ms"]
        line["profile_over_plain_wall"] = line["profile_wall_ms"] / line["plain_wall_ms"]
        if parent is not None:
            for m in ("kernel", "wall"):
                lo, hi = line[f"parent_plain_{m}_ms_min_max"]
                line[f"plain_within_parent_spread_{m}"] = bool(lo <= line[f"plain_{m}_ms"] <= hi)
            line["plain_same_bits_as_parent"] = same
        line["timing"] = ("kernel: HIP events around the launch, median of reps windows, each the median of inner calls; "
                          "wall: host-pointer call, median of reps windows, each the mean of inner calls; sides alternate")
        emit(line, a.out)


def bo(a):
    from mrbo import bayesopt
    from mrbo.optimizers import StandardSGA
    from mrbo.trajectory import TrajectoryParameters
    from mrbo.utils import ExperimentSetup, generate_batch, stochastic_solve_multi
    real = bayesopt.rollout_solve_multi
    diag = dict(t=0.0, zero=0, n=0)

    def counting(surs, lbs, ubs, horizon, mc_samples, batch_size, starts, sgd_iterations, theta, **kw):
        t0 = time.perf_counter()
        lbs_, ubs_ = np.asarray(lbs, float), np.asarray(ubs, float)
        batch = generate_batch(batch_size, lbs_, ubs_)
        x0 = np.stack([batch] * len(surs), axis=2)
        tp = TrajectoryParameters(start=batch[:, 0], hypers=[theta], horizon=horizon, mc_iterations=mc_samples,
                                  use_low_discrepancy_sequence=True, spatial_lowerbounds=lbs_, spatial_upperbounds=ubs_)
        es = ExperimentSetup(tp, number_of_starts=starts)
        opts = [[StandardSGA(η=0.0) for _ in range(x0.shape[1])] for _ in surs]
        _, hist = stochastic_solve_multi(opts, list(surs), tp, es, x0.copy(), iterations=1)
        for etos in hist[0]:
            diag["zero"] += all((e.gradient() == 0.0).all() for e in etos)
            diag["n"] += 1
        diag["t"] += time.perf_counter() - t0
        return real(surs, lbs, ubs, horizon, mc_samples, batch_size, starts, sgd_iterations, theta, **kw)

    bayesopt.rollout_solve_multi = counting
    try:
        for fn in ("braninhoo", "rosenbrock", "goldsteinprice"):
            for h in (0, 1):
                for std in (False, True):
                    diag.update(t=0.0, zero=0, n=0)
                    with tempfile.TemporaryDirectory() as tmp:
                        t0 = time.perf_counter()
                        res = bayesopt.run(fn, tmp, budget=10, trials=8, parallel_trials=8, reuse_surrogate=False,
                                           horizon=h, optimize=True, device_mle=True, device_solve=True, rules=("ei",),
                                           standardize=std, log=lambda *_: None)
                        wall = time.perf_counter() - t0 - diag["t"]
                    gaps = np.array([r["gaps"][-1] for r in res.values()])
                    q1, med, q3 = (float(v) for v in np.percentile(gaps, [25, 50, 75]))
                    emit(dict(bench="standardize_bo", function=fn, horizon=h, standardize=std, trials=len(res), budget=10,
                              gap_median=med, gap_q1=q1, gap_q3=q3, gaps=[float(g) for g in gaps],
                              zero_gradient_solves=diag["zero"], solves=diag["n"],
                              zero_gradient_share=diag["zero"] / max(diag["n"], 1), wall_s=wall,
                              ell_end_median=float(np.median([r["ell_end"] for r in res.values()]))), a.out)
    finally:
        bayesopt.rollout_solve_multi = real


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--fits", action="store_true")
    ap.add_argument("--bo", action="store_true")
    ap.add_argument("--parent-lib", default="", help="libmrbo.so of the commit before the profile mode")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not (a.fits or a.bo):
        sys.exit("one of --fits, --bo")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_standardize.py needs a GPU: a timing taken without one says nothing")
    if a.fits:
        fits(a)
    if a.bo:
        bo(a)


if __name__ == "__main__":
    main()
