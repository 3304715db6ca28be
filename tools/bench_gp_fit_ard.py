#!/usr/bin/env python3
"""ARD lengthscales measured, by tools/bench_standardize.py's protocol: the sides
alternate, a sample is a window of --inner calls (median HIP-event kernel time, mean wall time), the
figure the median of --reps windows after --warmup untimed rounds.

--fits: one fit call with P = 12 candidates on each of S = 16 data sets at (d, N) = (2, 20), (6, 64) and
(4, 128), Matérn-5/2, σn2 = 1e-6, profiled likelihood, host pointers: mrbo_gp_fit_ard_multi (`ard`) against
mrbo_gp_fit_profile_multi (`iso`) at the same shape.
--refit: one mrbo_gp_optimize_ard_multi call (`device`) against the host-driven optimize_ard_multi
(`host`) at S = 1, 4, 16 on (d, N) = (6, 64): wall time of the whole refit from ℓ_u = 1 in [0.1, 5]^d, and
whether both end at the same lengthscales bit for bit.
--bo: bayesopt.run (EI, h = 0 and 1) and run_myopic with standardize=True, ard off and on, on braninhoo,
rosenbrock and hartmann6d: 8 lockstep trials, budget 10, device_mle (and device_solve in run).  Per run
one JSON line: the final gaps (median and quartiles), the final lengthscales and wall time.

    python tools/bench_gp_fit_ard.py --fits --refit --bo [--out FILE]
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


def _datasets(d, N, n):
    keep = []
    for q in range(n):
        rng = np.random.default_rng(1000 * d + q)
        X = np.asfortranarray(rng.random((d, N)))
        y = np.sin(6 * X[0]) + 0.3 * X[-1] + 0.05 * rng.standard_normal(N)   # anisotropic: x₁, weakly the last
        keep.append((X, np.ascontiguousarray(y - y.mean())))
    return keep


def _windows(sides, a):
    def window(fn):
        t0 = time.perf_counter()
        ks = [fn() for _ in range(a.inner)]
        return statistics.median(ks), (time.perf_counter() - t0) / a.inner * 1e3
    for _ in range(a.warmup):
        for fn in sides.values():
            window(fn)
    ker, wall = {k: [] for k in sides}, {k: [] for k in sides}
    for _ in range(a.reps):              # alternate: every side sees the same machine
        for k, fn in sides.items():
            km, wm = window(fn)
            ker[k].append(km)
            wall[k].append(wm)
    return ker, wall


def fits(a):
    from mrbo import _lib
    L = _lib.load()
    dp = ctypes.POINTER(ctypes.c_double)
    vp = lambda x: ctypes.c_void_p(x.ctypes.data)
    H = _lib.MRBO_FLAG_HOST_POINTERS
    for d, N in SHAPES:
        keep = _datasets(d, N, S)
        sds = (_lib.SurrogateDesc * S)(*[_lib.SurrogateDesc(d, N, 0, 1.0, 1e-6, 0.0, X.ctypes.data_as(dp), None, N, None,
                                                            y.ctypes.data_as(dp), 1.0) for X, y in keep])
        ell = np.linspace(0.3, 2.0, P) * np.sqrt(d)
        th = np.ascontiguousarray(np.tile(ell, (S, 1)))
        ells = np.ascontiguousarray(np.tile((ell[:, None] * np.array([0.5, 1.0, 2.0])[np.arange(d) % 3][None, :]), (S, 1, 1)))
        ll, s2 = np.zeros((S, P)), np.zeros((S, P))
        g1, gd = np.zeros((S, P)), np.zeros((S, P, d))
        st = np.zeros((S, P), dtype=np.int32)

        def iso():
            rc = L.mrbo_gp_fit_profile_multi(sds, S, P, 1, vp(th), vp(ll), vp(g1), vp(s2), vp(st), None, None, H, None)
            assert rc == 0 and (st == 0).all(), (rc, st)
            return L.mrbo_last_gp_fit_ms()

        def ard():
            rc = L.mrbo_gp_fit_ard_multi(sds, S, P, vp(ells), vp(ll), vp(gd), vp(s2), vp(st), None, None, H, None)
            assert rc == 0 and (st == 0).all(), (rc, st)
            return L.mrbo_last_gp_fit_ms()

        ker, wall = _windows({"iso": iso, "ard": ard}, a)
        line = dict(bench="ard_fit", d=d, N=N, S=S, P=P, reps=a.reps, inner=a.inner)
        for k in ker:
            line[f"{k}_kernel_ms"] = statistics.median(ker[k])
            line[f"{k}_kernel_ms_min_max"] = [min(ker[k]), max(ker[k])]
            line[f"{k}_wall_ms"] = statistics.median(wall[k])
            line[f"{k}_wall_ms_min_max"] = [min(wall[k]), max(wall[k])]
        line["ard_over_iso_kernel"] = line["ard_kernel_ms"] / line["iso_kernel_ms"]
        line["ard_over_iso_wall"] = line["ard_wall_ms"] / line["iso_wall_ms"]
        emit(line, a.out)


def refit(a):
    from mrbo.ard import ARDSurrogate, gp_optimize_ard_multi, optimize_ard_multi
    from mrbo.kernels import Matern52
    d, N = 6, 64
    for n in (1, 4, 16):
        make = lambda: [ARDSurrogate(Matern52(), X, y, capacity=N, standardize=True) for X, y in _datasets(d, N, n)]
        surs = make()
        ends = {}

        def device():
            r = gp_optimize_ard_multi(surs, np.ones((n, d)), 0.1, 5.0, profile_amplitude=True)
            ends["device"] = r["ells"].copy(), int(r["iterations"].max()), r["rounds"]
            return 0.0

        def host():
            hs = make()                                   # optimize_ard_multi moves its surrogates: fresh ones
            t0 = time.perf_counter()
            r = optimize_ard_multi(hs, 0.1, 5.0)
            ends["host"] = np.stack([x["ells"] for x in r]), max(x["iterations"] for x in r)
            return (time.perf_counter() - t0) * 1e3

        wall = {"device": [], "host": []}
        for rep in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            device()
            dt = (time.perf_counter() - t0) * 1e3
            ht = host()                                   # the refit alone, without building the surrogates
            if rep >= a.warmup:
                wall["device"].append(dt)
                wall["host"].append(ht)
        emit(dict(bench="ard_refit", d=d, N=N, S=n, reps=a.reps, line_searches_max=ends["device"][1],
                  rounds=ends["device"][2], device_wall_ms=statistics.median(wall["device"]),
                  device_wall_ms_min_max=[min(wall["device"]), max(wall["device"])],
                  host_wall_ms=statistics.median(wall["host"]),
                  host_wall_ms_min_max=[min(wall["host"]), max(wall["host"])],
                  host_over_device=statistics.median(wall["host"]) / statistics.median(wall["device"]),
                  same_bits=bool(ends["device"][0].tobytes() == ends["host"][0].tobytes())), a.out)


def bo(a):
    from mrbo import bayesopt
    for fn in ("braninhoo", "rosenbrock", "hartmann6d"):
        for loop, h in (("run", 0), ("run", 1), ("run_myopic", None)):
            for ard in (False, True):
                with tempfile.TemporaryDirectory() as tmp:
                    t0 = time.perf_counter()
                    if loop == "run":
                        res = bayesopt.run(fn, tmp, budget=10, trials=8, parallel_trials=8, reuse_surrogate=False, horizon=h,
                                           optimize=True, device_mle=True, device_solve=True, rules=("ei",),
                                           standardize=True, ard=ard, log=lambda *_: None)
                    else:
                        res = bayesopt.run_myopic(fn, tmp, budget=10, trials=8, parallel_trials=8, reuse_surrogate=False,
                                                  optimize=True, device_mle=True, rules=("ei",), standardize=True,
                                                  ard=ard, log=lambda *_: None)
                    wall = time.perf_counter() - t0
                gaps = np.array([r["gaps"][-1] for r in res.values()])
                q1, med, q3 = (float(v) for v in np.percentile(gaps, [25, 50, 75]))
                ells = (np.stack([r["ells"] for r in res.values()]) if ard
                        else np.array([[r["ell_end"]] for r in res.values()]))
                emit(dict(bench="ard_bo", loop=loop, function=fn, horizon=h, ard=ard, trials=len(res), budget=10,
                          gap_median=med, gap_q1=q1, gap_q3=q3, gaps=[float(g) for g in gaps],
                          ells_median=[float(v) for v in np.median(ells, axis=0)],
                          ells_on_upper_bound=[int(v) for v in (ells == 5.0).sum(axis=0)], wall_s=wall), a.out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--fits", action="store_true")
    ap.add_argument("--refit", action="store_true")
    ap.add_argument("--bo", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="", help="also append the JSON lines to this file")
    a = ap.parse_args()
    if not (a.fits or a.refit or a.bo):
        sys.exit("one of --fits, --refit, --bo")
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_gp_fit_ard.py needs a GPU: a timing taken without one says nothing")
    if a.fits:
        fits(a)
    if a.refit:
        refit(a)
    if a.bo:
        bo(a)


if __name__ == "__main__":
    main()
