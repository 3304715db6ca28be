"""The fitted output scale, host side: the numpy specification of the
profiled-amplitude likelihood (mle.profile_log_likelihood_host) against a brute-force maximum over
the amplitude and finite differences, Surrogate(standardize=True) against a plain numpy GP with
kernel s²ψ and mean m, the share of the box on which the base EI underflows with and without
standardisation (on the CPU oracle), and the argument checks of the two new C entry points, which
return before any HIP call.  The device side is tests/test_gpu_standardize.py."""
import ctypes
import inspect

import numpy as np
import pytest
from scipy.optimize import minimize_scalar

import conftest  # noqa: F401  (sys.path)

MRBO_ERR_ARG = -1
SN2 = 1e-6


def _design(name, N, offset=3):
    """lbs + w·kronecker_quasirand(d, N, offset) on the objective's box, and its observations."""
    from mrbo import bayesopt
    from mrbo.utils import kronecker_quasirand
    fn = bayesopt.TESTFNS[name]()
    lbs, ubs = fn.get_bounds()
    X = lbs[:, None] + (ubs - lbs)[:, None] * kronecker_quasirand(fn.dim, N, offset)
    return X, fn(X), lbs, ubs


def _K(ψ, X, sn2):
    from mrbo.kernels import eval_KXX
    return eval_KXX(ψ, X, σn2=sn2)


def _full_ll(ψ, X, r, sn2, s2):
    """log N(r; 0, s²·(Ψ + σn2·I)): the full Gaussian likelihood the profile maximises over s²."""
    K = s2 * _K(ψ, X, sn2)
    L = np.linalg.cholesky(K)
    z = np.linalg.solve(L, r)
    return -0.5 * z @ z - np.log(np.diag(L)).sum() - 0.5 * len(r) * np.log(2 * np.pi)


def _spec_cases():
    from mrbo.kernels import Matern52, Periodic
    X, y, _, _ = _design("braninhoo", 20)
    cases = [(f"matern52-{ell}", Matern52([ell]), X, y - y.mean(), SN2) for ell in (0.5, 1.0, 3.0)]
    rng = np.random.default_rng(40)   # 1-D data: the kernel of a distance is PD in one dimension
    X1 = rng.random((1, 20)) * 3.0
    y1 = 40.0 * np.sin(3 * X1[0]) + 4.0 * rng.standard_normal(20) + 100.0
    cases.append(("periodic-nt2", Periodic([0.7, 1.3]), X1, y1 - y1.mean(), 1e-3))
    return cases


@pytest.mark.parametrize("case", range(4))
def test_spec_is_the_maximum_over_the_amplitude(case):
    """ll_p(θ) = max over s² of the full Gaussian log likelihood, attained at ŝ² = q/N."""
    from mrbo.mle import profile_log_likelihood_host
    name, ψ, X, r, sn2 = _spec_cases()[case]
    p = profile_log_likelihood_host(X, r, ψ, sn2)
    res = minimize_scalar(lambda t: -_full_ll(ψ, X, r, sn2, np.exp(t)), bounds=(np.log(p["s2"]) - 8, np.log(p["s2"]) + 8),
                          method="bounded", options=dict(xatol=1e-10))
    assert p["ll"] == pytest.approx(-res.fun, rel=1e-9, abs=1e-9), name
    assert np.exp(res.x) == pytest.approx(p["s2"], rel=1e-4), name      # a flat maximum: ll is quadratic around it
    assert p["ll"] == pytest.approx(_full_ll(ψ, X, r, sn2, p["s2"]), rel=1e-11, abs=1e-10)
    for f in (0.9, 1.1):
        assert _full_ll(ψ, X, r, sn2, f * p["s2"]) < p["ll"]


@pytest.mark.parametrize("case", range(4))
def test_spec_gradient_matches_central_differences(case):
    from mrbo.kernels import set_hyperparameters
    from mrbo.mle import profile_log_likelihood_host
    import copy
    name, ψ, X, r, sn2 = _spec_cases()[case]
    g = profile_log_likelihood_host(X, r, ψ, sn2)["grad"]
    assert g.shape == (len(ψ.θ),)
    for t in range(len(ψ.θ)):
        h = 1e-6 * ψ.θ[t]
        lls = []
        for sgn in (1.0, -1.0):
            θ = ψ.θ.copy()
            θ[t] += sgn * h
            lls.append(profile_log_likelihood_host(X, r, set_hyperparameters(copy.deepcopy(ψ), θ), sn2)["ll"])
        fd = (lls[0] - lls[1]) / (2 * h)
        assert g[t] == pytest.approx(fd, rel=1e-5, abs=1e-5), (name, t)


def test_spec_is_invariant_to_the_data_scale_and_rejects_constant_data():
    """ll_p(a·r) = ll_p(r) − N·log a, the gradient does not move and ŝ² scales by a²; r = 0 has no
    amplitude."""
    from mrbo.kernels import Matern52
    from mrbo.mle import profile_log_likelihood_host
    X, y, _, _ = _design("braninhoo", 20)
    r = y - y.mean()
    p1 = profile_log_likelihood_host(X, r, Matern52([1.0]), SN2)
    p2 = profile_log_likelihood_host(X, 8.0 * r, Matern52([1.0]), SN2)
    assert p2["ll"] == pytest.approx(p1["ll"] - 20 * np.log(8.0), rel=1e-12)
    assert p2["grad"][0] == pytest.approx(p1["grad"][0], rel=1e-12)
    assert p2["s2"] == pytest.approx(64.0 * p1["s2"], rel=1e-12)
    with pytest.raises(ValueError, match="constant"):
        profile_log_likelihood_host(X, np.zeros(20), Matern52([1.0]), SN2)


# ---- Surrogate(standardize=True) ---------------------------------------------------------------
def _numpy_gp(ψ, X, y, sn2, xs):
    """Posterior mean and standard deviation of a GP with constant mean m = mean(y), kernel s²ψ and
    noise s²σn2, s² = rᵀ(Ψ + σn2·I)⁻¹r/N: restated without the surrogate's buffers."""
    m = y.mean()
    r = y - m
    Kn = _K(ψ, X, sn2)
    s2 = r @ np.linalg.solve(Kn, r) / len(y)
    K = s2 * Kn
    D = xs[:, None, :] - X[:, :, None]
    k = s2 * ψ(np.sqrt((D * D).sum(0)))
    μ = m + k.T @ np.linalg.solve(K, r)
    v = s2 * float(ψ(0.0)) - (k * np.linalg.solve(K, k)).sum(0)
    return μ, np.sqrt(np.maximum(v, 0.0)), m, np.sqrt(s2)


def test_standardised_surrogate_is_a_numpy_gp_with_fitted_scale():
    from mrbo.kernels import Matern52
    from mrbo.surrogates import Surrogate
    from mrbo.utils import kronecker_quasirand
    X, y, lbs, ubs = _design("braninhoo", 20)
    s = Surrogate(Matern52([2.0]), X, y, capacity=25, σn2=SN2, standardize=True)
    xs = lbs[:, None] + (ubs - lbs)[:, None] * kronecker_quasirand(2, 64, 1000)
    μ, σ, m, amp = _numpy_gp(Matern52([2.0]), X, y, SN2, xs)
    assert s.m == pytest.approx(m, rel=1e-14) and s.s == pytest.approx(amp, rel=1e-9)
    pm, ps = s.posterior(xs)
    np.testing.assert_allclose(pm, μ, rtol=1e-7, atol=1e-7 * np.abs(y).max())
    np.testing.assert_allclose(ps, σ, rtol=1e-5, atol=1e-6 * amp)
    one = s.posterior(xs[:, 3])
    assert one == pytest.approx((pm[3], ps[3]), rel=1e-12)      # a matrix-vector product against a column of a product
    # what the plans and fits read: the standardised values; what the user reads: the raw ones
    np.testing.assert_array_equal(s.get_active_observations(), y)
    np.testing.assert_allclose(s.y[:20], (y - m) / amp, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(s.c[:20], np.linalg.solve(_K(s.ψ, X, SN2), s.y[:20]), rtol=1e-6, atol=1e-6 * np.abs(s.c).max())
    assert s.y[:20] @ s.c[:20] == pytest.approx(20.0, rel=1e-10)          # ỹᵀK⁻¹ỹ = N: unit amplitude
    assert s.fmini() == s.y[:20].min() and s.fmini() < 0.0 == s.y[20:].min()   # observed points only
    # the default is the reference's surrogate
    p = Surrogate(Matern52([2.0]), X, y, capacity=25, σn2=SN2)
    assert not p.standardize and (p.m, p.s) == (0.0, 1.0) and p.y_raw is None
    np.testing.assert_array_equal(p.y[:20], y)
    assert p.fmini() == 0.0


def test_standardised_pick_is_invariant_to_an_affine_map_of_the_objective(oracle):
    """y → a·y + b leaves ỹ, and with it the base-EI argmax over a fixed grid, where it was."""
    from mrbo.kernels import Matern52
    from mrbo.surrogates import Surrogate
    from mrbo.utils import kronecker_quasirand
    X, y, lbs, ubs = _design("braninhoo", 20)
    xs = lbs[:, None] + (ubs - lbs)[:, None] * kronecker_quasirand(2, 256, 1000)
    picks, eis = [], []
    for a, b in ((1.0, 0.0), (250.0, -17.0), (1e-3, 4.0)):
        s = Surrogate(Matern52([1.0]), X, a * y + b, capacity=20, σn2=SN2, standardize=True)
        o = oracle.OracleSurrogate(X, s.L[:20, :20], s.c[:20], s.y[:20], fmini=s.fmini())
        ei = oracle.eval_base(o, xs)[2]
        picks.append(int(np.argmax(ei)))
        eis.append(ei)
        assert s.s == pytest.approx(a * Surrogate(Matern52([1.0]), X, y, capacity=20, standardize=True).s, rel=1e-9)
    assert picks[0] == picks[1] == picks[2]
    np.testing.assert_allclose(eis[1], eis[0], rtol=1e-6, atol=1e-9 * eis[0].max())
    np.testing.assert_allclose(eis[2], eis[0], rtol=1e-6, atol=1e-9 * eis[0].max())


def test_condition_set_kernel_and_reset_restandardise():
    from mrbo.kernels import Matern52
    from mrbo.surrogates import Surrogate
    X, y, _, _ = _design("goldsteinprice", 12)
    s = Surrogate(Matern52([1.0]), X[:, :9], y[:9], capacity=12, σn2=SN2, standardize=True)
    v = s.version
    for j in range(9, 12):
        assert s.condition(X[:, j], y[j]) is s
    assert s.version == v + 3
    fresh = Surrogate(Matern52([1.0]), X, y, capacity=12, σn2=SN2, standardize=True)

    def same(a, b):
        assert a.m == pytest.approx(b.m, rel=1e-13) and a.s == pytest.approx(b.s, rel=1e-9)
        np.testing.assert_allclose(a.y[:12], b.y[:12], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(a.c[:12], b.c[:12], rtol=1e-6, atol=1e-7 * np.abs(b.c).max())
        np.testing.assert_array_equal(a.get_active_observations(), y)
    same(s, fresh)
    v = s.version
    s.set_kernel(Matern52([0.4]))
    assert s.version == v + 1 and s.s != fresh.s
    same(s, Surrogate(Matern52([0.4]), X, y, capacity=12, σn2=SN2, standardize=True))
    s.reset(X[:, :5], y[:5])
    five = Surrogate(Matern52([0.4]), X[:, :5], y[:5], capacity=12, σn2=SN2, standardize=True)
    assert s.observed == 5 and s.m == pytest.approx(five.m) and s.s == pytest.approx(five.s, rel=1e-9)
    # a single point, or constant data, has no amplitude: s = 1
    assert Surrogate(Matern52(), X[:, :1], y[:1], capacity=4, standardize=True).s == 1.0
    const = Surrogate(Matern52(), X[:, :4], np.full(4, 7.0), capacity=4, standardize=True)
    assert const.s == 1.0 and const.m == 7.0 and (const.y == 0.0).all()
    # past capacity the surrogate doubles and stays standardised on the raw values
    big = fresh.condition(np.array([0.5, 0.5]), 3.0)
    assert big is not fresh and big.standardize and big.capacity == 24 and big.get_active_observations()[-1] == 3.0


# ---- the underflow table of DESIGN.md §17 -----------------------------------------------------
@pytest.mark.parametrize("name", ["braninhoo", "rosenbrock", "goldsteinprice"])
def test_base_ei_underflows_on_raw_observations_and_not_on_standardised(oracle, name):
    """ℓ = 1, σn2 = 1e-6, N = 20: the share of 256 quasi-random points of the box at which the base
    EI is exactly 0 (and with it its gradient).  Measured 26 % / 88 % / 85 % on the raw observations
    and 0 % on the standardised ones."""
    from mrbo.kernels import Matern52
    from mrbo.surrogates import Surrogate
    from mrbo.utils import kronecker_quasirand
    X, y, lbs, ubs = _design(name, 20, 3)
    xs = lbs[:, None] + (ubs - lbs)[:, None] * kronecker_quasirand(len(lbs), 256, 1000)
    share = {}
    for std in (False, True):
        s = Surrogate(Matern52([1.0]), X, y, capacity=20, σn2=SN2, standardize=std)
        o = oracle.OracleSurrogate(X, s.L[:20, :20], s.c[:20], s.y[:20], fmini=s.fmini())
        out = oracle.eval_base(o, xs)
        d = len(lbs)
        ei, gei = out[2], out[3 + 2 * d:3 + 3 * d]
        share[std] = float(np.mean(ei == 0.0))
        assert ((gei == 0.0).all(axis=0) >= (ei == 0.0)).all()       # a zero EI comes with a zero gradient
    print(f"{name}: EI == 0 at {100 * share[False]:.0f} % raw, {100 * share[True]:.0f} % standardised")
    assert share[False] > 0.20, share
    assert share[True] < 0.05, share


# ---- argument checks of the new entry points (before any HIP call) ----------------------------
def _desc(d=2, N=4, kernel=0):
    from mrbo import _lib
    dp = ctypes.POINTER(ctypes.c_double)
    X = np.asfortranarray(np.arange(d * N, dtype=np.float64).reshape(d, N) / (d * N))
    y = np.linspace(-1.0, 1.0, N)
    return _lib.SurrogateDesc(d, N, kernel, 1.0, SN2, 0.0, X.ctypes.data_as(dp), None, N, None, y.ctypes.data_as(dp), 1.0), (X, y)


def _fit_profile(S=2, P=2, nt=1, null_s2=False):
    from mrbo import _lib
    L = _lib.load()
    descs = [_desc(), _desc()]
    arr = (_lib.SurrogateDesc * 2)(*[sd for sd, _ in descs])
    n = 4
    th, ll, grad, s2 = np.ones(2 * n), np.zeros(n), np.zeros(2 * n), np.zeros(n)
    st = np.zeros(n, dtype=np.int32)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    rc = L.mrbo_gp_fit_profile_multi(arr, S, P, nt, vp(th), vp(ll), vp(grad), None if null_s2 else vp(s2), vp(st), None,
                                     None, _lib.MRBO_FLAG_HOST_POINTERS, None)
    return rc, L.mrbo_last_error()


def _optimize_profile(S=2, nt=1, null_s2=False, flags=None):
    from mrbo import _lib
    L = _lib.load()
    descs = [_desc(), _desc()]
    arr = (_lib.SurrogateDesc * 2)(*[sd for sd, _ in descs])
    a = {k: np.ones(4) for k in ("theta0", "theta", "nll", "grad", "s2")}
    lo, hi = np.full(2, 0.1), np.full(2, 5.0)
    its = np.zeros(2, dtype=np.int32)
    res = (ctypes.c_int32 * 2)()
    vp = lambda a_: ctypes.c_void_p(a_.ctypes.data)
    rc = L.mrbo_gp_optimize_profile_multi(arr, S, nt, vp(a["theta0"]), vp(lo), vp(hi), None, vp(a["theta"]), vp(a["nll"]),
                                          vp(a["grad"]), None if null_s2 else vp(a["s2"]), vp(its), res,
                                          _lib.MRBO_FLAG_HOST_POINTERS if flags is None else flags, None)
    return rc, L.mrbo_last_error()


def test_profile_entry_points_check_their_arguments_before_any_device_call():
    assert _fit_profile(null_s2=True)[0] == MRBO_ERR_ARG
    rc, msg = _fit_profile(S=0)
    assert rc == MRBO_ERR_ARG and b"S=0" in msg
    assert _fit_profile(P=0)[0] == MRBO_ERR_ARG
    rc, msg = _fit_profile(nt=2)                     # Matérn-5/2 has one hyperparameter
    assert rc == MRBO_ERR_ARG and b"nt=2" in msg
    assert _fit_profile(nt=0)[0] == MRBO_ERR_ARG
    assert _optimize_profile(null_s2=True)[0] == MRBO_ERR_ARG
    rc, msg = _optimize_profile(S=0)
    assert rc == MRBO_ERR_ARG and b"S=0" in msg
    rc, msg = _optimize_profile(nt=2)
    assert rc == MRBO_ERR_ARG and b"nt=2" in msg
    assert _optimize_profile(flags=4)[0] == MRBO_ERR_ARG


def test_every_new_keyword_defaults_to_off():
    from mrbo import bayesopt, mle
    from mrbo.surrogates import Surrogate
    off = lambda f, k: inspect.signature(f).parameters[k].default is False
    assert off(mle.gp_fit_multi, "profile") and off(mle.gp_fit_batch, "profile")
    for f in (mle.optimize, mle.optimize_multi, mle.gp_optimize_multi):
        assert off(f, "profile_amplitude")
    assert off(Surrogate.__init__, "standardize")
    assert off(bayesopt.run, "standardize") and off(bayesopt.run_myopic, "standardize")
    assert bayesopt.parse(["--output-dir", "o", "--function-name", "braninhoo"]).standardize is False
    assert bayesopt.parse(["--output-dir", "o", "--function-name", "braninhoo", "--standardize"]).standardize is True


def test_optimize_multi_refuses_a_mixed_batch():
    from mrbo.kernels import Matern52
    from mrbo.mle import optimize_multi
    from mrbo.surrogates import Surrogate
    X, y, _, _ = _design("braninhoo", 6)
    surs = [Surrogate(Matern52(), X, y, capacity=6, standardize=std) for std in (True, False)]
    with pytest.raises(ValueError, match="standardised and plain"):
        optimize_multi(surs, [0.1], [5.0])
