"""Device-resident MLE refits on the device (mrbo_gp_optimize_multi, include/mrbo.h): ONE call
minimises −log_likelihood for S data sets, and every output carries the bits of the specification
-- mle.lbfgs_scalar driven by the plain gp_fit_batch on each data set alone -- on each fit-kernel
path, for every kernel family, with a short history, a failing start, a short budget, host and
device pointers; mle.optimize_multi and the BO loops end where the host-driven loop ends.  The host
side is tests/test_mle_device.py."""
import copy
import ctypes

import numpy as np
import pytest

import conftest  # noqa: F401  (sys.path)
from test_gpu_gp_fit_multi import _data, _kernel, _periodic_surrogates, same_bits

pytestmark = pytest.mark.gpu

LO, HI = [0.1], [5.0]


def _surrogates(kernel, d, N, seeds, sn2=1e-6):
    from mrbo.surrogates import Surrogate
    out = []
    for seed in seeds:
        X, y = _data(d, N, seed=seed)
        out.append(Surrogate(_kernel(kernel, [1.0]), X, y, capacity=N, σn2=sn2))
    return out


def _spec(s, theta0, lo, hi, **kw):
    """The specification on one data set alone: lbfgs_scalar over the plain fit call."""
    from mrbo.mle import gp_fit_batch, lbfgs_scalar

    def fg(T):
        r = gp_fit_batch(s, T)
        return np.where(r["status"] == 0, -r["ll"], np.nan), -r["grad"]
    return lbfgs_scalar(fg, theta0, lo, hi, **kw)


def _assert_equals_spec(surs, theta0, lo, hi, iterations=30, history=10):
    """gp_optimize_multi's slot q against the specification on surs[q], bit for bit (a NaN equals
    a NaN); returns (the call's dict, the specification's iteration counts)."""
    from mrbo.mle import gp_optimize_multi
    theta0 = np.asarray(theta0, dtype=np.float64).reshape(len(surs), -1)
    r = gp_optimize_multi(surs, theta0, lo, hi, iterations=iterations, history=history)
    nt = theta0.shape[1]
    assert r["theta"].shape == (len(surs), nt) and r["gradient"].shape == (len(surs), nt)
    assert r["neg_log_likelihood"].shape == (len(surs),) and r["iterations"].shape == (len(surs),)
    its = []
    for q, s in enumerate(surs):
        x, f, g, it = _spec(s, theta0[q], lo, hi, iterations=iterations, m=history)
        got = (r["theta"][q], r["neg_log_likelihood"][q], r["gradient"][q], r["iterations"][q])
        print(q, "spec", x, f, g, it, "device", *got)
        assert same_bits(got[0], x), (q, got, x)
        if np.isnan(f) or np.isnan(g).any():
            assert np.array_equal(got[1], f, equal_nan=True) and np.array_equal(got[2], g, equal_nan=True), (q, got)
        else:
            assert same_bits(got[1], np.float64(f)) and same_bits(got[2], g), (q, got, f, g)
        assert got[3] == it, (q, got, it)
        its.append(it)
    # every problem stops in the step kernel of round 1 + its iteration count (round 1 is the
    # start): the last stop is the true one, and the host reads it at most two rounds late
    assert r["stopped_at"] == 1 + max(its), (r["stopped_at"], its)
    assert r["stopped_at"] <= r["rounds"] <= min(r["stopped_at"] + 2, iterations + 1), (r["rounds"], r["stopped_at"])
    return r, its


# one case per fit-kernel path, at the smallest shape of the issue that takes it
PATHS = [
    pytest.param(2, 20, (8, 0, 3), id="tile-one-tile"),
    pytest.param(3, 48, (300, 301, 302), id="register"),
    pytest.param(6, 72, (600, 601, 602), id="lds"),
    pytest.param(4, 96, (400, 401, 402), id="tile-three-rows"),
]


@pytest.mark.parametrize("d,N,seeds", PATHS)
def test_device_equals_specification_matern52(gpu, d, N, seeds):
    surs = _surrogates("matern52", d, N, seeds)
    r, its = _assert_equals_spec(surs, np.ones((3, 1)), LO, HI)
    assert not same_bits(r["theta"][0], r["theta"][1])      # three different problems
    if N == 20:
        # the data sets of test_optimize_multi_equals_optimize: they stop after different iteration
        # counts, so the early stoppers sit frozen while the launches go on for the others
        assert len(set(its)) == 3 and min(its) > 3, its


def test_history_wraps(gpu):
    """history = 2 on problems of more than 3 iterations: the ring of (s, y) pairs overwrites its
    oldest entry."""
    surs = _surrogates("matern52", 2, 20, (8, 0, 3))
    r, its = _assert_equals_spec(surs, np.ones((3, 1)), LO, HI, history=2)
    assert min(its) > 3, its
    r1, _ = _assert_equals_spec(surs, np.ones((3, 1)), LO, HI, history=1)


@pytest.mark.parametrize("kernel,sn2", [("matern32", 1e-6), ("matern12", 1e-6), ("se", 1e-3)])
def test_other_kernels(gpu, kernel, sn2):
    surs = _surrogates(kernel, 2, 20, (8, 0, 3), sn2=sn2)
    r, its = _assert_equals_spec(surs, np.ones((3, 1)), LO, HI)
    assert np.isfinite(r["neg_log_likelihood"]).all() and max(its) > 1, (r, its)


def test_periodic_two_hyperparameters(gpu):
    """θ = (ℓ, p): nt = 2, a different start per data set (the nt·P·S strides of the launches)."""
    periods = [1.3, 0.8, 2.5]
    surs = _periodic_surrogates(20, periods)
    th0 = np.array([[1.0, per] for per in periods])
    r, its = _assert_equals_spec(surs, th0, [0.1, 0.5], [5.0, 3.0])
    assert np.isfinite(r["neg_log_likelihood"]).all() and max(its) > 1, (r, its)
    r, its = _assert_equals_spec(surs, th0, [0.1, 0.5], [5.0, 3.0], history=2)


def test_periodic_lengthscale_alone(gpu):
    """θ = (ℓ) with each data set's own period (nt = 1)."""
    periods = [2.1, 2.0, 2.7]    # the oracle-driven specification ends at ℓ = 1.87 (5 iterations), on the
    surs = _periodic_surrogates(20, periods)   # lower bound (1) and at 0.44 (8) on these
    r, its = _assert_equals_spec(surs, np.ones((3, 1)), LO, HI)
    assert np.isfinite(r["neg_log_likelihood"]).all() and len(set(its)) == 3, (r, its)
    # the period really is the data set's: data sets 0 and 2 with each other's period end elsewhere
    other = _periodic_surrogates(20, [periods[2], periods[1], periods[0]])
    from mrbo.mle import gp_optimize_multi
    r2 = gp_optimize_multi(other, np.ones((3, 1)), LO, HI)
    assert not same_bits(r2["theta"][0], r["theta"][0]) and not same_bits(r2["theta"][2], r["theta"][2])
    assert same_bits(r2["theta"][1], r["theta"][1]) and same_bits(r2["gradient"][1], r["gradient"][1])


def test_a_start_on_an_active_bound_inside_a_batch(gpu):
    """Slot 1 starts on the lower bound with the gradient pointing outward (where that data set's
    minimisation ends, test_periodic_lengthscale_alone): it stops in round 1 with no line search
    made, and never proposes a trial point -- its slots of the later (12, S) launches hold its
    start.  Slot 2 starts above the box and is clipped onto the upper bound, where it is free."""
    periods = [2.1, 2.0, 2.7]
    surs = _periodic_surrogates(20, periods)
    th0 = np.array([[1.0], [0.1], [7.0]])
    r, its = _assert_equals_spec(surs, th0, LO, HI)
    assert its[1] == 0 and r["theta"][1, 0] == 0.1 and r["gradient"][1, 0] > 0, (r, its)
    assert np.isfinite(r["neg_log_likelihood"]).all() and min(its[0], its[2]) > 1, (r, its)
    # every slot stops at once: one round, the start's
    r, its = _assert_equals_spec(surs[1:2] * 3, np.full((3, 1), 0.1), LO, HI)
    assert its == [0, 0, 0] and r["stopped_at"] == 1 and r["rounds"] <= 3, (r, its)


def _call(surs, th0, device, iterations=30):
    """mrbo_gp_optimize_multi through ctypes with host or device pointers: (theta, nll, grad, iters, result)."""
    import torch
    from mrbo import _lib
    L = _lib.load()
    n, d, Sn = surs[0].observed, surs[0].X.shape[0], len(surs)
    dp = ctypes.POINTER(ctypes.c_double)
    keep = [(np.asfortranarray(s.X[:, :n]), np.ascontiguousarray(s.y[:n])) for s in surs]
    sds = (_lib.SurrogateDesc * Sn)(*[
        _lib.SurrogateDesc(d, n, int(s.ψ.kind), 1.0, float(s.σn2), 0.0, X.ctypes.data_as(dp), None, n, None,
                           y.ctypes.data_as(dp), float(s.ψ.period)) for s, (X, y) in zip(surs, keep)])
    th0 = np.ascontiguousarray(th0, dtype=np.float64).reshape(Sn, -1)
    nt = th0.shape[1]
    lo, hi = np.full(nt, 0.1), np.full(nt, 5.0)
    arrays = [th0, np.zeros((Sn, nt)), np.zeros(Sn), np.zeros((Sn, nt)), np.zeros(Sn, dtype=np.int32)]
    if device:
        bufs = [torch.from_numpy(a).to("cuda:0") for a in arrays]
        torch.cuda.synchronize()
        p = lambda a: ctypes.c_void_p(a.data_ptr())
        flags = 0
    else:
        bufs = arrays
        p = lambda a: ctypes.c_void_p(a.ctypes.data)
        flags = _lib.MRBO_FLAG_HOST_POINTERS
    res = (ctypes.c_int32 * 2)()
    opts = _lib.MleOpts(iterations, 0, 0.0, 0.0)
    h = lambda a: ctypes.c_void_p(a.ctypes.data)
    _lib.check(L.mrbo_gp_optimize_multi(sds, Sn, nt, p(bufs[0]), h(lo), h(hi), ctypes.byref(opts), p(bufs[1]),
                                        p(bufs[2]), p(bufs[3]), p(bufs[4]), res, flags, None))
    out = [b.cpu().numpy() if device else b for b in bufs[1:]]
    if device:
        assert same_bits(bufs[0].cpu().numpy(), th0)      # the starts are an input
    return out + [list(res)]


@pytest.mark.parametrize("n", [1, 3])
def test_one_data_set_and_device_pointers(gpu, n):
    """Device-pointer mode gives the bits of host-pointer mode, and for one hyperparameter the call
    ends where mle.optimize (projected_lbfgs over numpy) ends: a dot product is one multiplication."""
    from mrbo.mle import optimize
    surs = _surrogates("matern52", 3, 48, (300, 301, 302)[:n])
    host = _call(surs, np.ones((n, 1)), device=False)
    dev = _call(surs, np.ones((n, 1)), device=True)
    for a, b in zip(host[:4], dev[:4]):
        assert same_bits(a, b)
    assert host[4][1] == dev[4][1]                  # the same true stop round (the rounds launched may differ)
    for q, s in enumerate(copy.deepcopy(surs)):
        one = optimize(s, LO, HI)
        assert same_bits(host[0][q], one["theta"]) and same_bits(host[2][q], one["gradient"])
        assert host[1][q] == one["neg_log_likelihood"] and host[3][q] == one["iterations"]


def test_a_failing_start_is_isolated(gpu, oracle):
    """SE kernel, σn2 = 0: at ℓ = 1e10 K is all ones and its factorisation fails (the oracle confirms
    it first), so slot 1, started there, has f = NaN: one line search, nothing accepted, its start
    returned.  The other slots are what they are alone."""
    from mrbo.mle import gp_optimize_multi
    from mrbo.surrogates import Surrogate
    from mrbo.utils import kronecker_quasirand
    surs = []
    for q in range(3):
        X = kronecker_quasirand(2, 12, 11 * q + 1)
        y = np.sin(3 * X.sum(0))
        assert np.isnan(oracle.log_likelihood(X, y, "se", 1e10, 0.0)[0])
        assert np.isfinite(oracle.log_likelihood(X, y, "se", 0.2, 0.0)[0])
        surs.append(Surrogate(_kernel("se", [0.2]), X, y, capacity=12, σn2=0.0))
    th0 = np.array([[0.2], [1e10], [0.2]])
    r, its = _assert_equals_spec(surs, th0, [0.1], [1e10])
    assert np.isnan(r["neg_log_likelihood"][1]) and r["theta"][1, 0] == 1e10 and its[1] == 1
    assert np.isfinite(r["neg_log_likelihood"][[0, 2]]).all()
    for q in (0, 2):
        solo = gp_optimize_multi([surs[q]], th0[q:q + 1], [0.1], [1e10])
        for k in ("theta", "neg_log_likelihood", "gradient", "iterations"):
            assert same_bits(solo[k][0], r[k][q]), (q, k)


def test_a_short_budget(gpu):
    """iterations = 3: every problem still running stops on the budget, in round 4."""
    surs = _surrogates("matern52", 2, 20, (8, 0, 3))
    r, its = _assert_equals_spec(surs, np.ones((3, 1)), LO, HI, iterations=3)
    assert its == [3, 3, 3] and r["stopped_at"] == 4 and r["rounds"] == 4
    r, its = _assert_equals_spec(surs, np.ones((3, 1)), LO, HI, iterations=1)
    assert its == [1, 1, 1] and r["rounds"] == 2


def test_optimize_multi_on_the_device_equals_the_host_loop(gpu):
    from mrbo.mle import optimize, optimize_multi
    surs = _surrogates("matern52", 2, 20, (8, 0, 3))
    a, b = copy.deepcopy(surs), copy.deepcopy(surs)
    ra = optimize_multi(a, LO, HI, device=False)
    rb = optimize_multi(b, LO, HI, device=True)
    for s0, sa, sb, x, y in zip(surs, a, b, ra, rb):
        assert same_bits(sa.ψ.θ, sb.ψ.θ) and not same_bits(sa.ψ.θ, s0.ψ.θ)
        assert same_bits(sa.L, sb.L) and same_bits(sa.c, sb.c)
        assert same_bits(x["theta"], y["theta"]) and same_bits(x["gradient"], y["gradient"])
        assert x["neg_log_likelihood"] == y["neg_log_likelihood"] and x["iterations"] == y["iterations"]
    one = optimize(copy.deepcopy(surs[1]), LO, HI, device=True)
    assert same_bits(one["theta"], rb[1]["theta"]) and one["iterations"] == rb[1]["iterations"]


def _assert_runs_equal(on, off):
    assert set(on) == set(off) and len(on) > 0
    for key in on:
        for k in ("gaps", "y", "X"):
            assert same_bits(on[key][k], off[key][k]), (key, k)
        assert on[key]["ell_end"] == off[key]["ell_end"] and on[key]["ell_end"] != on[key]["ell_start"]
        if "mle_times" in off[key]:      # the lockstep path times its batched refit, as before
            assert on[key]["mle_times"].shape == off[key]["mle_times"].shape and (on[key]["mle_times"] > 0).all()


@pytest.mark.parametrize("parallel_trials", [2, 1])
def test_bo_loop_with_the_device_refit(gpu, tmp_path, parallel_trials):
    from mrbo import bayesopt
    kw = dict(budget=2, trials=2, horizon=0, mc_samples=8, sgd_iterations=2, optimize=True, rules=("ei",),
              reuse_surrogate=False, parallel_trials=parallel_trials, log=lambda *_: None)
    on = bayesopt.run("braninhoo", str(tmp_path / "on"), device_mle=True, **kw)
    off = bayesopt.run("braninhoo", str(tmp_path / "off"), device_mle=False, **kw)
    _assert_runs_equal(on, off)


@pytest.mark.parametrize("parallel_trials", [2, 1])
def test_myopic_loop_with_the_device_refit(gpu, tmp_path, parallel_trials):
    from mrbo import bayesopt
    kw = dict(budget=3, trials=2, rules=("ei",), optimize=True, reuse_surrogate=False,
              parallel_trials=parallel_trials, log=lambda *_: None)
    on = bayesopt.run_myopic("braninhoo", str(tmp_path / "on"), device_mle=True, **kw)
    off = bayesopt.run_myopic("braninhoo", str(tmp_path / "off"), device_mle=False, **kw)
    _assert_runs_equal(on, off)
