"""ctypes wrapper of the CPU oracle (oracle/build/librbo_oracle.so).

TEST INFRASTRUCTURE ONLY -- the parity checker and the cpu_baseline "port".
Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this.
The product (rollout-bayesian-optimization_amd/mrbo) never imports it.
"""
import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "build", "librbo_oracle.so")
_lib = None

COSTS = {"none": 0, "quadratic": 1, "loglinear": 2}
KERNELS = {"matern52": 0, "matern32": 1, "matern12": 2, "se": 3, "periodic": 4}
TESTFNS = {"gramacylee": 0, "braninhoo": 1, "hartmann6d": 2, "ackley": 3, "rosenbrock": 4, "rastrigin": 5}

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)
_lp = ctypes.POINTER(ctypes.c_int64)


class Surrogate(ctypes.Structure):
    _fields_ = [("d", ctypes.c_int32), ("N", ctypes.c_int32), ("kernel", ctypes.c_int32),
                ("ell", ctypes.c_double), ("sigma_n2", ctypes.c_double), ("fmini", ctypes.c_double),
                ("X", _dp), ("L", _dp), ("c", _dp), ("y", _dp), ("period", ctypes.c_double)]


class Params(ctypes.Structure):
    _fields_ = [("h", ctypes.c_int32), ("M", ctypes.c_int32), ("R", ctypes.c_int32), ("nstarts", ctypes.c_int32),
                ("theta", ctypes.c_double), ("lbs", _dp), ("ubs", _dp),
                ("max_iters", ctypes.c_int32), ("max_ls", ctypes.c_int32),
                ("x_tol", ctypes.c_double), ("f_tol", ctypes.c_double), ("g_tol", ctypes.c_double),
                ("htol", ctypes.c_double), ("sigma_tol", ctypes.c_double), ("seed", ctypes.c_uint64),
                ("sample_offset", ctypes.c_int32), ("samples_total", ctypes.c_int32),
                ("with_gradient", ctypes.c_int32), ("nthreads", ctypes.c_int32), ("rule", ctypes.c_int32),
                ("cost", ctypes.c_int32), ("cost_c0", ctypes.c_double), ("cost_w", _dp), ("kappa", _dp),
                ("vbound", _dp), ("ylip", _dp)]


def build():
    subprocess.check_call(["make", "-s", "-C", _HERE])


_override = None


def use_library(path):
    """Load the oracle from `path` (e.g. the -O3 -march=native timing build of bench.py's
    cpu_baseline leg) for later calls; None restores the checker build."""
    global _lib, _override
    _override = path
    _lib = None


def lib():
    global _lib
    if _lib is None:
        path = _override or _LIB_PATH
        if path == _LIB_PATH and not os.path.exists(_LIB_PATH):
            build()
        L = ctypes.CDLL(path)
        L.rbo_gen_uniform.argtypes = [ctypes.c_int32, ctypes.c_int32, _dp]
        L.rbo_gen_low_discrepancy_sequence.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _dp]
        L.rbo_generate_initial_guesses.argtypes = [ctypes.c_int32, ctypes.c_int32, _dp, _dp, _dp]
        L.rbo_kronecker_quasirand.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _dp]
        L.rbo_dual_uniform.argtypes = [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
        L.rbo_dual_uniform.restype = ctypes.c_double
        L.rbo_testfn.argtypes = [ctypes.c_int32, ctypes.c_int32, _dp]
        L.rbo_testfn.restype = ctypes.c_double
        L.rbo_eval_base.argtypes = [ctypes.POINTER(Surrogate), ctypes.c_int32, ctypes.c_double, ctypes.c_double,
                                    ctypes.c_int32, _dp, _dp]
        L.rbo_eval_base_p.argtypes = [ctypes.POINTER(Surrogate), ctypes.POINTER(Params), ctypes.c_int32, _dp, _dp]
        L.rbo_simulate_mc.argtypes = [ctypes.POINTER(Surrogate), ctypes.POINTER(Params), _dp, _dp, _dp, _dp, _dp,
                                      _dp, _dp, _dp, _ip, _dp, _dp, _dp, _lp]
        L.rbo_log_likelihood.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_double,
                                         ctypes.c_double, _dp, _dp, _dp, _dp, _dp, _dp]
        L.rbo_log_likelihood_theta.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _dp,
                                               ctypes.c_double, ctypes.c_double, _dp, _dp, _dp, _dp, _dp, _dp]
        L.rbo_simulate_ghq.argtypes = [ctypes.POINTER(Surrogate), ctypes.POINTER(Params), _dp, _dp, _dp, _dp, _dp,
                                       _dp, _dp, _dp, _dp, _ip, _dp, _dp, _dp, _lp]
        L.rbo_base_solve.argtypes = [ctypes.POINTER(Surrogate), ctypes.POINTER(Params), ctypes.c_int32, _dp, _dp,
                                     _dp, _ip, _lp]
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _f64(a):
    return np.require(np.asarray(a, dtype=np.float64), requirements=["F", "A"])


def gen_uniform(samples, dim):
    out = np.zeros((dim, samples), order="F")
    assert lib().rbo_gen_uniform(samples, dim, _p(out)) == 0
    return out


def gen_low_discrepancy_sequence(M, d, H):
    out = np.zeros((M, d + 1, H), order="F")
    assert lib().rbo_gen_low_discrepancy_sequence(M, d, H, _p(out)) == 0
    return out


def generate_initial_guesses(n, lbs, ubs):
    lbs, ubs = _f64(lbs), _f64(ubs)
    d = lbs.size
    out = np.zeros((d, n + 2), order="F")
    assert lib().rbo_generate_initial_guesses(n, d, _p(lbs), _p(ubs), _p(out)) == 0
    return out


def kronecker_quasirand(d, N, start=0):
    out = np.zeros((d, N), order="F")
    lib().rbo_kronecker_quasirand(d, N, start, _p(out))
    return out


def dual_uniform(seed, traj, j, k):
    return lib().rbo_dual_uniform(seed, traj, j, k)


def testfn(name, x):
    x = _f64(x)
    return lib().rbo_testfn(TESTFNS[name], x.size, _p(x))


class OracleSurrogate:
    """Holds the base-surrogate arrays alive for the C struct."""

    def __init__(self, X, L, c, y, kernel="matern52", ell=1.0, sigma_n2=1e-6, fmini=None, period=1.0):
        self.X, self.L, self.c, self.y = _f64(X), _f64(L), _f64(c), _f64(y)
        d, N = self.X.shape
        fm = float(np.min(self.y)) if fmini is None else float(fmini)
        self.s = Surrogate(d, N, KERNELS[kernel], ell, sigma_n2, fm, _p(self.X), _p(self.L), _p(self.c), _p(self.y),
                           float(period))


RULES = {"EI": 0, "POI": 1, "LCB": 2}


def log_likelihood(X, y, kernel="matern52", ell=1.0, sigma_n2=1e-6, want_fit=False):
    """(ll, dll[, L, c]) of the GP refit at lengthscale ell; NaNs on PosDefException."""
    X, y = _f64(X), _f64(y).ravel()
    d, N = X.shape
    ll, dll = ctypes.c_double(), ctypes.c_double()
    L = np.zeros((N, N), order="F")
    c = np.zeros(N)
    rc = lib().rbo_log_likelihood(d, N, KERNELS[kernel], float(ell), float(sigma_n2), _p(X), _p(y), ctypes.byref(ll),
                                  ctypes.byref(dll), _p(L), _p(c))
    if rc < 0:
        raise ValueError(f"log_likelihood: kernel {kernel} not supported")
    return (ll.value, dll.value, L, c) if want_fit else (ll.value, dll.value)


def log_likelihood_theta(X, y, kernel, theta, sigma_n2=1e-6, period=1.0, want_fit=False):
    """(ll, grad[, L, c]): ∇log_likelihood over θ = (ℓ) or, for the Periodic kernel, (ℓ, p)
    (a one-element θ keeps `period`).  NaNs on PosDefException."""
    X, y = _f64(X), _f64(y).ravel()
    th = _f64(theta).ravel()
    d, N = X.shape
    ll = ctypes.c_double()
    grad = np.zeros(th.size)
    L = np.zeros((N, N), order="F")
    c = np.zeros(N)
    rc = lib().rbo_log_likelihood_theta(d, N, KERNELS[kernel], th.size, _p(th), float(period), float(sigma_n2), _p(X),
                                        _p(y), ctypes.byref(ll), _p(grad), _p(L), _p(c))
    if rc < 0:
        raise ValueError(f"log_likelihood_theta: kernel {kernel} with {th.size} hyperparameters")
    return (ll.value, grad, L, c) if want_fit else (ll.value, grad)


def eval_base(osur, xs, theta=0.0, sigma_tol=1e-8, rule="EI", cost=None, lbs=None, ubs=None):
    """Base-surrogate evaluation, columns [μ, σ, α, ∇μ, ∇σ, ∇α, Hα, ∂∇α/∂θ] per point; with
    cost=(kind, c0, w) (and the box lbs, ubs) the NonUniformCost-weighted α/c(x) and its derivatives."""
    xs = _f64(xs)
    d, P = xs.shape
    stride = 3 + 4 * d + d * d
    out = np.zeros((stride, P), order="F")
    if cost is None:
        assert lib().rbo_eval_base(ctypes.byref(osur.s), RULES[rule], theta, sigma_tol, P, _p(xs), _p(out)) == 0
        return out
    lbs, ubs, cw = _f64(lbs).ravel(), _f64(ubs).ravel(), _f64(cost[2]).ravel()
    ck = COSTS[cost[0]] if isinstance(cost[0], str) else int(cost[0])
    prm = Params(0, 1, 1, 1, theta, _p(lbs), _p(ubs), 0, 0, 0.0, 0.0, 0.0, 0.0, sigma_tol, 0, 0, 0, 0, 1,
                 RULES[rule], ck, float(cost[1]), _p(cw))
    assert lib().rbo_eval_base_p(ctypes.byref(osur.s), ctypes.byref(prm), P, _p(xs), _p(out)) == 0
    return out


def simulate_mc(osur, x0s, rnstream, xstarts, lbs, ubs, h, theta=0.0, dual_y_dx=None, replay_x=None,
                max_iters=50, max_ls=20, x_tol=1e-3, f_tol=1e-3, g_tol=1e-8, htol=1e-4, sigma_tol=1e-8,
                seed=1906, with_gradient=True, nthreads=0, want_policy=True, sample_offset=0,
                samples_total=0, rule="EI", ghq=None, cost=None, want_kappa=False, policy_fill=0.0):
    """Run the oracle's simulate_trajectory_mc for every restart column of x0s (d×R).
    ghq=(nodes, weights), each M×(h+1): the Gauss–Hermite estimator (rbo_simulate_ghq) instead
    of the rnstream draws (rnstream is then only used for its M).
    cost=(kind, c0, w): NonUniformCost weighting of the inner-solve rule (rbo_oracle.h RBO_COST_*).
    want_kappa: also return "kappa" (M×R), each trajectory's largest cond₁ of the acquisition
    Hessians its adjoint solved with (rbo_params.kappa; 1 when none), "vbound" (M×R) the first-order
    bound on the rounding difference of its value and "ylip" (M×R) max_k ‖∂y_k/∂x_k‖₁
    (rbo_params.vbound / ylip).
    policy_fill: what "policy_x" holds before the run -- a failed trajectory (status != 0) writes the
    columns up to its last step only and leaves the later ones as they were."""
    x0s, xstarts = _f64(x0s), _f64(xstarts)
    lbs, ubs = _f64(lbs), _f64(ubs)
    d, R = x0s.shape
    if ghq is not None:
        nodes, weights = _f64(ghq[0]), _f64(ghq[1])
        M = nodes.shape[0]
        assert nodes.shape == (M, h + 1) and weights.shape == (M, h + 1), (nodes.shape, weights.shape)
    else:
        rnstream = _f64(rnstream)
        M = rnstream.shape[0]
        assert rnstream.shape == (M, d + 1, h + 1), rnstream.shape
    cw = None
    ck, c0 = 0, 1.0
    if cost is not None:
        ck = COSTS[cost[0]] if isinstance(cost[0], str) else int(cost[0])
        c0 = float(cost[1])
        cw = _f64(cost[2]).ravel()
        assert cw.size == d, (cw.size, d)
    prm = Params(h, M, R, xstarts.shape[1], theta, _p(lbs), _p(ubs), max_iters, max_ls, x_tol, f_tol, g_tol,
                 htol, sigma_tol, seed, sample_offset, samples_total, 1 if with_gradient else 0, nthreads,
                 RULES[rule], ck, c0, _p(cw))
    kappa = np.zeros((M, R), order="F") if want_kappa else None
    vbound = np.zeros((M, R), order="F") if want_kappa else None
    ylip = np.zeros((M, R), order="F") if want_kappa else None
    prm.kappa, prm.vbound, prm.ylip = _p(kappa), _p(vbound), _p(ylip)
    values = np.zeros((M, R), order="F")
    grad_x = np.zeros((d, M, R), order="F")
    grad_t = np.zeros((1, M, R), order="F")
    status = np.zeros((M, R), dtype=np.int32, order="F")
    policy = np.full((d, h + 1, M, R), float(policy_fill), order="F") if want_policy else None
    obs = np.zeros((h + 1, M, R), order="F")
    eto = np.zeros((2 + 2 * d + 2, R), order="F")
    evals = np.zeros((3, M, R), dtype=np.int64, order="F")   # [grad, value, hess] per trajectory
    dy = None if dual_y_dx is None else _f64(dual_y_dx)
    rp = None if replay_x is None else _f64(replay_x)
    if ghq is not None:
        rc = lib().rbo_simulate_ghq(ctypes.byref(osur.s), ctypes.byref(prm), _p(x0s), _p(nodes), _p(weights),
                                    _p(xstarts), _p(dy), _p(rp), _p(values), _p(grad_x), _p(grad_t),
                                    status.ctypes.data_as(_ip), _p(policy), _p(obs), _p(eto),
                                    evals.ctypes.data_as(_lp))
    else:
        rc = lib().rbo_simulate_mc(ctypes.byref(osur.s), ctypes.byref(prm), _p(x0s), _p(rnstream), _p(xstarts),
                                   _p(dy), _p(rp), _p(values), _p(grad_x), _p(grad_t),
                                   status.ctypes.data_as(_ip), _p(policy), _p(obs), _p(eto),
                                   evals.ctypes.data_as(_lp))
    assert rc == 0, rc
    return dict(values=values, grad_x=grad_x, grad_theta=grad_t, status=status, policy_x=policy, obs=obs,
                eto=eto, evals=evals, kappa=kappa, vbound=vbound, ylip=ylip)


def base_solve(osur, xstarts, lbs, ubs, theta=0.0, rule="EI", max_iters=50, max_ls=20, x_tol=1e-3, f_tol=1e-3,
               g_tol=1e-8, sigma_tol=1e-8):
    """base_solve(s; xstart) from every column of xstarts (d×n) on the base surrogate (rbo_base_solve):
    (xmin d×n, fmin n, status n, evals 3×n)."""
    xstarts, lbs, ubs = _f64(xstarts), _f64(lbs).ravel(), _f64(ubs).ravel()
    d, n = xstarts.shape
    prm = Params(0, 1, 1, n, theta, _p(lbs), _p(ubs), max_iters, max_ls, x_tol, f_tol, g_tol, 1e-4, sigma_tol, 0, 0,
                 0, 0, 1, RULES[rule], 0, 1.0, None)
    xmin = np.zeros((d, n), order="F")
    fmin = np.zeros(n)
    status = np.zeros(n, dtype=np.int32)
    evals = np.zeros((3, n), dtype=np.int64, order="F")
    rc = lib().rbo_base_solve(ctypes.byref(osur.s), ctypes.byref(prm), n, _p(xstarts), _p(xmin), _p(fmin),
                              status.ctypes.data_as(_ip), evals.ctypes.data_as(_lp))
    assert rc == 0, rc
    return xmin, fmin, status, evals
