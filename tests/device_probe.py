"""Loader of the device-primitive probe (tests/device_probe.hip): test infrastructure only.

The probe wraps the inlined building blocks of csrc/mrbo_device.h (fexp, the roots, ei_phi_Phi,
rule_partials, rad_eval, the cost model, the wave reductions, dual_uniform) in one small kernel per
group, so that tests/test_gpu_primitives.py can hold each of them to an mpmath reference on its own.
It is compiled with the product's flags (__graft_entry__.HIPCC_FLAGS, -I csrc) into
tests/_probe/libmrbo_probe.so and is never linked into libmrbo.so.

Known limit: the probe compiles the inlined functions standalone.  FMA contraction around a call
site inside the rollout kernel can differ from the probe's, so the error bounds of the tests hold
under either contraction, while the bit-equality claims (fexp == exp, the six- and seven-argument
rule_partials, rad_eval2 == two rad_eval) are checked for the probe's compilation only.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SRC = os.path.join(ROOT, "tests", "device_probe.hip")
CSRC = os.path.join(ROOT, "rollout-bayesian-optimization_amd", "csrc")
HEADER = os.path.join(CSRC, "mrbo_device.h")
OUT = os.path.join(ROOT, "tests", "_probe", "libmrbo_probe.so")

_dp = ctypes.POINTER(ctypes.c_double)
_lib = None


def _hipcc():
    h = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return h if os.path.exists(h) else None


def stale(out=OUT):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(p) > t for p in (SRC, HEADER))


def compile_probe(out=OUT, header_dir=CSRC):
    """Compile the probe (one hipcc call, a few seconds).  header_dir: where mrbo_device.h is taken
    from (another directory builds the probe against another version of the header)."""
    from __graft_entry__ import HIPCC_FLAGS
    hipcc = _hipcc()
    if hipcc is None:
        raise RuntimeError("device probe: hipcc not found")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    tmp = out + ".tmp"
    subprocess.check_call([hipcc] + HIPCC_FLAGS + ["-shared", "-I", header_dir, "-o", tmp, SRC])
    os.replace(tmp, out)
    return out


def ensure_built():
    """Compile when the library is missing or older than its source or the header, and hipcc is there."""
    if stale() and _hipcc() is not None:
        compile_probe()
    return OUT


def load(path=None):
    """The probe library through ctypes.  A missing library (no hipcc to build it) raises: on a GPU
    test that is a failure, not a skip."""
    global _lib
    if path is None:
        if _lib is not None:
            return _lib
        path = ensure_built()
    if not os.path.exists(path):
        raise RuntimeError(f"device probe: {path} is missing and cannot be built here")
    L = ctypes.CDLL(path)
    i, d = ctypes.c_int, ctypes.c_double
    L.probe_exp.argtypes = [_dp, _dp, _dp, i]
    L.probe_roots.argtypes = [_dp, _dp, i]
    L.probe_phi.argtypes = [_dp, _dp, i]
    L.probe_rule.argtypes = [i, _dp, _dp, _dp, d, d, d, _dp, i]
    L.probe_rad.argtypes = [i, d, d, _dp, _dp, i]
    L.probe_cost.argtypes = [i, i, d, _dp, _dp, _dp, _dp, _dp, i]
    L.probe_reduce.argtypes = [i, i, _dp, _dp]
    L.probe_allreduce.argtypes = [_dp, _dp]
    L.probe_dual.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _dp, _dp, i]
    for f in ("exp", "roots", "phi", "rule", "rad", "cost", "reduce", "allreduce", "dual"):
        getattr(L, "probe_" + f).restype = i
    if path == OUT:
        _lib = L
    return L


def _in(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return a.ctypes.data_as(_dp)


def _ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"device probe: {what} returned HIP error {rc}")


class Probe:
    """NumPy front of the launchers (every call is one kernel launch on device 0)."""

    def __init__(self, lib=None):
        self.L = lib or load()

    def exp(self, x):
        """(fexp(x), exp(x)) evaluated in the same kernel."""
        x = _in(x)
        f, e = np.empty_like(x), np.empty_like(x)
        _ok(self.L.probe_exp(_p(x), _p(f), _p(e), x.size), "probe_exp")
        return f, e

    def roots(self, s):
        """dict r, ir (sqrt_rsqrt), sqrt0 (fast_sqrt0), sig, isig (sig_isig)."""
        s = _in(s)
        out = np.empty((5, s.size))
        _ok(self.L.probe_roots(_p(s), _p(out), s.size), "probe_roots")
        return dict(zip(("r", "ir", "sqrt0", "sig", "isig"), out))

    def phi(self, z):
        z = _in(z)
        out = np.empty((2, z.size))
        _ok(self.L.probe_phi(_p(z), _p(out), z.size), "probe_phi")
        return out[0], out[1]

    def rule(self, rule, mu, sig, isig, theta, fmin, sigma_tol):
        """(seven-argument overload, six-argument overload), each [7][n] in the order of EIp."""
        mu, sig, isig = _in(mu), _in(sig), _in(isig)
        out = np.empty((2, 7, mu.size))
        _ok(self.L.probe_rule(rule, _p(mu), _p(sig), _p(isig), theta, fmin, sigma_tol, _p(out), mu.size), "probe_rule")
        return out[0], out[1]

    def rad(self, kind, cK, cP, rho2):
        """(rad_eval [3][n], rad_eval2 a-results [3][n], rad_eval2 b-results [3][n] at rho2[::-1])."""
        rho2 = _in(rho2)
        out = np.empty((3, 3, rho2.size))
        _ok(self.L.probe_rad(kind, cK, cP, _p(rho2), _p(out), rho2.size), "probe_rad")
        return out[0], out[1], out[2]

    def cost(self, D, cost, c0, lb, delta, w, x):
        """x [n][D] -> c [n], ∇c [n][D], Hc [n][D][D]."""
        tab = _in(np.concatenate([lb, delta, w]))
        x = _in(x)
        n = x.shape[0]
        c, g, H = np.empty(n), np.empty((n, D)), np.empty((n, D, D))
        _ok(self.L.probe_cost(D, cost, c0, _p(tab), _p(x), _p(c), _p(g), _p(H), n), "probe_cost")
        return c, g, H

    def reduce(self, v, half=False):
        """v [64][K] -> red [K] (wave_reduce<K>) or [2][K] (half_reduce<K> in both halves)."""
        v = _in(v)
        K = v.shape[1]
        red = np.empty((2, K) if half else (K,))
        _ok(self.L.probe_reduce(K, int(half), _p(v), _p(red)), "probe_reduce")
        return red

    def allreduce(self, v):
        """v [64] -> (wave_allreduce1, lanes_min<64>, lanes_min<32>), each as held by the 64 lanes."""
        v = _in(v)
        out = np.empty((3, 64))
        _ok(self.L.probe_allreduce(_p(v), _p(out)), "probe_allreduce")
        return out[0], out[1], out[2]

    def dual(self, seed, traj, j, k):
        """(device, host) values of dual_uniform."""
        seed = np.ascontiguousarray(seed, dtype=np.uint64)
        traj = np.ascontiguousarray(traj, dtype=np.int64)
        j = np.ascontiguousarray(j, dtype=np.int32)
        k = np.ascontiguousarray(k, dtype=np.int32)
        dev, host = np.empty(seed.size), np.empty(seed.size)
        _ok(self.L.probe_dual(seed.ctypes.data, traj.ctypes.data, j.ctypes.data, k.ctypes.data, _p(dev), _p(host),
                              seed.size), "probe_dual")
        return dev, host
