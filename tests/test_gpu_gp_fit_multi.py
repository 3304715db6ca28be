"""Batched GP refits on the device (mrbo_gp_fit_multi, include/mrbo.h): ONE launch of grid (P, S)
fits S data sets at P hyperparameter vectors each, and block q of every output carries the bits of
the plain mrbo_gp_fit_theta call on data set q -- on each of the three fit kernels, with and
without the factor outputs, also when one slot of the launch fails; mle.optimize_multi and the BO
loop's batched refit end where the per-surrogate optimize ends.  The host side is
tests/test_gp_fit_multi.py."""
import copy
import ctypes

import numpy as np
import pytest

import conftest  # noqa: F401  (sys.path)

pytestmark = pytest.mark.gpu

S, P = 3, 5   # P ≠ S, neither a power of two: a transposed (p, q) index shows


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _data(d, N, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.random((d, N))
    return X, np.sin(3 * X.sum(0)) + 0.1 * rng.standard_normal(N)


def _kernel(name, theta):
    from mrbo import kernels
    return {"matern52": kernels.Matern52, "matern32": kernels.Matern32, "matern12": kernels.Matern12,
            "se": kernels.SquaredExponential, "periodic": kernels.Periodic}[name](list(theta))


def _surrogates(kernel, d, N, sn2=1e-6, n=S):
    from mrbo.surrogates import Surrogate
    out = []
    for q in range(n):
        X, y = _data(d, N, seed=100 * d + q)
        out.append(Surrogate(_kernel(kernel, [1.0]), X, y, capacity=N, σn2=sn2))
    return out


def _ells(kernel, d, n=S):
    """(S, P) lengthscales, different for every data set; SE's stay where K is positive definite."""
    base = np.array([0.2, 0.5, 1.0, 2.0, 4.0]) * np.sqrt(d) * (0.15 if kernel == "se" else 1.0)
    return np.stack([base * (1.0 + 0.07 * q) for q in range(n)])


def _assert_blocks_equal(surs, th, want_fit, expect_ok=True):
    """gp_fit_multi's block q against the plain gp_fit_batch(surs[q], th[q]), bit for bit."""
    from mrbo.mle import gp_fit_batch, gp_fit_multi
    r = gp_fit_multi(surs, th, want_fit=want_fit)
    nt = th.shape[2] if th.ndim == 3 else 1
    N = surs[0].observed
    assert r["ll"].shape == (len(surs), P) and r["grad"].shape == (len(surs), P, nt)
    assert r["status"].shape == (len(surs), P) and r["dll"].shape == (len(surs), P)
    plain = [gp_fit_batch(s, th[q], want_fit=want_fit) for q, s in enumerate(surs)]
    for q, one in enumerate(plain):
        for k in ("ll", "grad", "dll", "status"):
            assert same_bits(r[k][q], one[k]), (q, k)
        if want_fit:   # a failed candidate writes neither L nor c: its slot of both is undefined
            ok = one["status"] == 0
            assert same_bits(r["L"][q][:, :, ok], one["L"][:, :, ok]), (q, "L")
            assert same_bits(r["c"][q][:, ok], one["c"][:, ok]), (q, "c")
    if want_fit:
        assert r["L"].shape == (len(surs), N, N, P) and r["c"].shape == (len(surs), N, P)
    if expect_ok:
        assert (r["status"] == 0).all(), r["status"]
    # the blocks are different fits: equal blocks would hide a launch that reads one data set S times
    assert not same_bits(r["ll"][0], r["ll"][1])
    return r, plain


# one case per kernel path, at the smallest shape of the issue that takes it
PATHS = [
    pytest.param(2, 20, False, id="tile-one-tile"),
    pytest.param(3, 48, False, id="register"),
    pytest.param(3, 48, True, id="lds-with-outputs"),
    pytest.param(6, 72, False, id="lds"),
    pytest.param(4, 96, False, id="tile-three-rows"),
    pytest.param(4, 96, True, id="tile-three-rows-with-outputs"),
]


@pytest.mark.parametrize("d,N,want_fit", PATHS)
def test_blocks_equal_plain_calls_matern52(gpu, d, N, want_fit):
    _assert_blocks_equal(_surrogates("matern52", d, N), _ells("matern52", d), want_fit)


@pytest.mark.parametrize("want_fit", [False, True])
@pytest.mark.parametrize("kernel", ["matern32", "matern12", "se"])
def test_blocks_equal_plain_calls_other_kernels(gpu, kernel, want_fit):
    _assert_blocks_equal(_surrogates(kernel, 3, 48), _ells(kernel, 3), want_fit)


def _periodic_surrogates(N, periods):
    from mrbo.surrogates import Surrogate
    out = []
    for q, per in enumerate(periods):
        rng = np.random.default_rng(40 + q)   # 1-D data: the kernel of a distance is PD in one dimension
        X = rng.random((1, N)) * 3.0
        y = np.sin(3 * X[0]) + 0.1 * rng.standard_normal(N)
        out.append(Surrogate(_kernel("periodic", [1.0, per]), X, y, capacity=N, σn2=1e-3))
    return out


@pytest.mark.parametrize("want_fit", [False, True])
@pytest.mark.parametrize("N", [20, 48])
def test_blocks_equal_plain_calls_periodic(gpu, N, want_fit):
    """θ = (ℓ, p) per candidate (nt = 2), and θ = (ℓ) with each data set's own period (nt = 1)."""
    periods = [1.3, 0.8, 2.5]
    surs = _periodic_surrogates(N, periods)
    th = np.array([[0.7, 1.3], [1.5, 0.8], [2.0, 2.5], [0.5, 1.9], [1.1, 1.1]])
    th2 = np.stack([th * (1.0 + 0.05 * q) for q in range(S)])
    _assert_blocks_equal(surs, th2, want_fit)
    r1, _ = _assert_blocks_equal(surs, th2[:, :, 0], want_fit)
    # the period really is the data set's: the same surrogate at another period gives other bits
    from mrbo.mle import gp_fit_batch
    other = _periodic_surrogates(N, [periods[1], periods[0], periods[2]])
    assert not same_bits(gp_fit_batch(other[0], th2[0, :, 0])["ll"], r1["ll"][0])


def _call_multi(surs, th, device):
    """mrbo_gp_fit_multi through ctypes with host or device pointers; returns (ll, grad, status, c)."""
    import torch
    from mrbo import _lib
    L = _lib.load()
    n, d, Sn = surs[0].observed, surs[0].X.shape[0], len(surs)
    dp = ctypes.POINTER(ctypes.c_double)
    keep = [(np.asfortranarray(s.X[:, :n]), np.ascontiguousarray(s.y[:n])) for s in surs]
    sds = (_lib.SurrogateDesc * Sn)(*[
        _lib.SurrogateDesc(d, n, int(s.ψ.kind), 1.0, float(s.σn2), 0.0, X.ctypes.data_as(dp), None, n, None,
                           y.ctypes.data_as(dp), float(s.ψ.period)) for s, (X, y) in zip(surs, keep)])
    th = np.ascontiguousarray(th, dtype=np.float64)
    Pn = th.shape[1]
    if device:
        t = lambda a: torch.from_numpy(a).to("cuda:0")
        bufs = [t(th), t(np.zeros((Sn, Pn))), t(np.zeros((Sn, Pn))), t(np.zeros((Sn, Pn), dtype=np.int32)),
                t(np.zeros((Sn, Pn, n)))]
        torch.cuda.synchronize()
        p = lambda a: ctypes.c_void_p(a.data_ptr())
        flags = 0
    else:
        bufs = [th, np.zeros((Sn, Pn)), np.zeros((Sn, Pn)), np.zeros((Sn, Pn), dtype=np.int32), np.zeros((Sn, Pn, n))]
        p = lambda a: ctypes.c_void_p(a.ctypes.data)
        flags = _lib.MRBO_FLAG_HOST_POINTERS
    _lib.check(L.mrbo_gp_fit_multi(sds, Sn, Pn, 1, p(bufs[0]), p(bufs[1]), p(bufs[2]), p(bufs[3]), None, p(bufs[4]),
                                   flags, None))
    assert L.mrbo_last_gp_fit_ms() > 0.0      # the multi launch is timed as the plain one is
    return [b.cpu().numpy() if device else b for b in bufs[1:]]


@pytest.mark.parametrize("n", [1, S])
def test_one_data_set_and_device_pointers(gpu, n):
    """S = 1 is mrbo_gp_fit_theta; device-pointer mode gives the bits of host-pointer mode (c_out
    alone requested: the outputs are optional one by one)."""
    from mrbo.mle import gp_fit_batch
    surs = _surrogates("matern52", 3, 48, n=n)
    th = _ells("matern52", 3, n=n)
    host = _call_multi(surs, th, device=False)
    dev = _call_multi(surs, th, device=True)
    for h, g in zip(host, dev):
        assert same_bits(h, g)
    for q, s in enumerate(surs):
        one = gp_fit_batch(s, th[q], want_fit=True)
        assert same_bits(host[0][q], one["ll"]) and same_bits(host[1][q], one["dll"])
        assert same_bits(host[2][q], one["status"]) and same_bits(host[3][q].T, one["c"])


# ---- one failing slot leaves the launch's other slots alone ------------------------------------
ISOLATION = [
    pytest.param(2, 12, False, id="tile-one-tile"),
    pytest.param(2, 33, False, id="register"),
    pytest.param(2, 33, True, id="lds"),
    pytest.param(4, 81, False, id="tile-three-rows"),
]


@pytest.mark.parametrize("d,N,want_fit", ISOLATION)
def test_a_failing_slot_is_isolated(gpu, oracle, d, N, want_fit):
    """SE kernel, σn2 = 0: at ℓ = 1e10 ψ rounds to exactly 1 for every pair, K is all ones and the
    second pivot is exactly 0 (PosDefException), while ℓ = 0.2 factors (the oracle's fit confirms
    both first).  N = 12 in the unit square, and the smallest N of every other kernel path (in
    [0, 1]⁴ at N = 81, where 81 points of the unit square would leave K near singular at ℓ = 0.2)."""
    from mrbo.surrogates import Surrogate
    from mrbo.utils import kronecker_quasirand
    bad_p, bad_q = 3, 1
    surs = []
    for q in range(S):
        X = kronecker_quasirand(d, N, 11 * q + 1)
        y = np.sin(3 * X.sum(0))
        assert np.isnan(oracle.log_likelihood(X, y, "se", 1e10, 0.0)[0])
        assert np.isfinite(oracle.log_likelihood(X, y, "se", 0.2, 0.0)[0])
        surs.append(Surrogate(_kernel("se", [0.2]), X, y, capacity=N, σn2=0.0))
    th = np.full((S, P), 0.2)
    th[bad_q, bad_p] = 1e10
    r, plain = _assert_blocks_equal(surs, th, want_fit, expect_ok=False)   # status and bits equal the plain calls'
    expect = np.zeros((S, P), dtype=np.int32)
    expect[bad_q, bad_p] = 1
    assert np.array_equal(r["status"], expect)
    assert np.array_equal(np.isnan(r["ll"]), expect == 1)
    assert np.isnan(r["grad"][bad_q, bad_p]).all() and np.isfinite(np.delete(r["grad"].ravel(), bad_q * P + bad_p)).all()
    # the good slots of the data set with the failure: all at ℓ = 0.2, so all the same fit
    good = [p for p in range(P) if p != bad_p]
    assert all(same_bits(r["ll"][bad_q, p], r["ll"][bad_q, good[0]]) for p in good)


# ---- the lockstep optimiser ---------------------------------------------------------------------
def test_optimize_multi_equals_optimize(gpu):
    """Three d = 2, N = 20 data sets on which the oracle-driven minimiser (tests/test_mle.py's
    _oracle_fg, Matérn-5/2, σn2 = 1e-6, ℓ₀ = 1, box [0.1, 5]) stops after 7, 9 and 12 iterations."""
    from mrbo.mle import optimize, optimize_multi
    from mrbo.surrogates import Surrogate
    surs = []
    for seed in (8, 0, 3):
        X, y = _data(2, 20, seed=seed)
        surs.append(Surrogate(_kernel("matern52", [1.0]), X, y, capacity=20, σn2=1e-6))
    alone = [optimize(s, [0.1], [5.0]) for s in copy.deepcopy(surs)]
    together = optimize_multi(surs, [0.1], [5.0])
    its = [r["iterations"] for r in together]
    assert len(set(its)) > 1, its
    for s, a, b in zip(surs, alone, together):
        assert same_bits(a["theta"], b["theta"]) and same_bits(a["gradient"], b["gradient"])
        assert a["neg_log_likelihood"] == b["neg_log_likelihood"] and a["iterations"] == b["iterations"]
        assert s.ψ.lengthscale == b["theta"][0]          # set_kernel at the optimum


def test_bo_loop_refits_in_one_call(gpu, tmp_path):
    from mrbo import bayesopt
    kw = dict(budget=2, trials=2, horizon=0, mc_samples=8, sgd_iterations=2, optimize=True, rules=("ei",),
              reuse_surrogate=False, log=lambda *_: None)
    par = bayesopt.run("braninhoo", str(tmp_path / "par"), parallel_trials=2, **kw)
    seq = bayesopt.run("braninhoo", str(tmp_path / "seq"), parallel_trials=1, **kw)
    assert set(par) == set(seq) and len(par) == 2
    for key in par:
        for k in ("gaps", "y", "X"):
            assert same_bits(par[key][k], seq[key][k]), (key, k)
        assert par[key]["ell_end"] == seq[key]["ell_end"] and par[key]["ell_end"] != par[key]["ell_start"]
        assert par[key]["mle_times"].shape == (2,) and (par[key]["mle_times"] > 0).all()
