#!/usr/bin/env python3
"""ms per launch of C3's arrays at h = 5, M = 1024, R = 64: the FMAX = 6 unit's rollout_kernel<6,1,1,1>,
which no bench.py configuration runs.  Ten launches after three, by HIP events; one JSON line.
usage (on the GPU): [MRBO_LIB=/path/to/libmrbo.so] python tools/bench_c3_h5.py"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "rollout-bayesian-optimization_amd"), ROOT]
import torch
from parity import _plan, _problem_arrays
from mrbo.engine import rnstream, to_device
M, R, h = 1024, 64, 5
g = _problem_arrays("C3", M, R)
g["h"] = h
g["rnstream"] = rnstream(M, 6, h + 1)
p = _plan(g)
dev = "cuda:0"
out = p.alloc_outputs(with_gradient=True, want_policy=False, want_obs=False)
x0, rn, xs = to_device(g["x0s"], dev), to_device(g["rnstream"], dev), to_device(g["xstarts"], dev)
for _ in range(3):
    p.simulate(x0, rn, xs, out)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
n = 10
e0.record()
for _ in range(n):
    p.simulate(x0, rn, xs, out)
e1.record()
torch.cuda.synchronize()
info = p.info()
print(json.dumps(dict(row="C3 arrays at h = 5, M = 1024, R = 64", ms_per_launch=e0.elapsed_time(e1) / n, launches=n,
                      info={k: info[k] for k in ("spec", "rpl", "fmax", "lds_bytes", "waves_per_group")},
                      status_errors=int((out["status"] != 0).sum().item()))))
