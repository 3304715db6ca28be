"""ARD lengthscales on the host: the float64 specification of the ARD likelihood
against centred differences and, at equal lengthscales, against the oracle's isotropic likelihood; the
ARD refit on an anisotropic design; ARDSurrogate against plain numpy; and the argument checks of the two
entry points, which return before any HIP call."""
import ctypes
import math

import numpy as np
import pytest

from test_mle import _data, _ll_tol

KERNELS = ["matern52", "matern32", "matern12", "se"]
KIND = {"matern52": 0, "matern32": 1, "matern12": 2, "se": 3}
SN2 = 1e-6
MRBO_ERR_ARG, MRBO_ERR_UNSUPPORTED = -1, -2      # include/mrbo.h


def aniso_design():
    """d = 3, N = 24: only x₁ matters much, x₂ a little, x₃ not at all."""
    X = np.random.default_rng(3).random((3, 24))
    y = np.sin(6.0 * X[0]) + 0.3 * X[1]
    return X, y - y.mean()


def _psi1(kernel, rho):
    if kernel == "matern52":
        s = np.sqrt(5.0) * rho
        return (1 + s + s * s / 3) * np.exp(-s)
    if kernel == "matern32":
        s = np.sqrt(3.0) * rho
        return (1 + s) * np.exp(-s)
    if kernel == "matern12":
        return np.exp(-rho)
    return np.exp(-rho * rho / 2)


def ard_K(X, kernel, ells, sn2=SN2):
    """K from the formula, independently of mrbo.ard."""
    Z = X / np.asarray(ells, float)[:, None]
    rho = np.sqrt(((Z[:, :, None] - Z[:, None, :]) ** 2).sum(0))
    return _psi1(kernel, rho) + sn2 * np.eye(X.shape[1])


@pytest.mark.parametrize("profile", [False, True])
@pytest.mark.parametrize("kernel", KERNELS)
def test_specification_gradient_against_centred_differences(kernel, profile):
    from mrbo.ard import ard_log_likelihood_host
    X, y = aniso_design()
    ells = np.array([0.4, 1.1, 2.3])
    r = ard_log_likelihood_host(X, y, KIND[kernel], ells, SN2, profile=profile)
    h = 1e-6
    fd = np.zeros(3)
    for u in range(3):
        e = np.zeros(3)
        e[u] = h
        fd[u] = (ard_log_likelihood_host(X, y, KIND[kernel], ells + e, SN2, profile=profile)["ll"]
                 - ard_log_likelihood_host(X, y, KIND[kernel], ells - e, SN2, profile=profile)["ll"]) / (2 * h)
    err = np.abs(r["grad"] - fd).max() / np.abs(r["grad"]).max()
    print(f"{kernel} profile={profile}: grad {r['grad']}, relative error against differences {err:.2e}")
    assert err <= 1e-5
    np.testing.assert_allclose(r["L"] @ r["L"].T, ard_K(X, kernel, ells), rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("d,N", [(3, 20), (6, 64)])
def test_specification_at_equal_lengthscales_against_the_oracle(oracle, kernel, d, N):
    from mrbo.ard import ard_log_likelihood_host
    X, y = _data(d, N)
    ell = 0.8 * np.sqrt(d) * (0.15 if kernel == "se" else 1.0)
    ll, dll, L, c = oracle.log_likelihood(X, y, kernel, ell, SN2, want_fit=True)
    r = ard_log_likelihood_host(X, y, KIND[kernel], np.full(d, ell), SN2)
    assert abs(r["ll"] - ll) <= _ll_tol(ll, L, c), (r["ll"], ll)
    assert r["grad"].sum() == pytest.approx(dll, rel=1e-8, abs=1e-8 * (1 + abs(ll)))


def test_profiled_specification_at_equal_lengthscales_is_the_isotropic_one():
    from mrbo.ard import ard_log_likelihood_host
    from mrbo.kernels import Matern52
    from mrbo.mle import profile_log_likelihood_host
    X, y = aniso_design()
    iso = profile_log_likelihood_host(X, y, Matern52([0.7]), SN2)
    r = ard_log_likelihood_host(X, y, 0, np.full(3, 0.7), SN2, profile=True)
    assert r["ll"] == pytest.approx(iso["ll"], rel=1e-9)
    assert r["grad"].sum() == pytest.approx(iso["grad"][0], rel=1e-8)
    assert r["s2"] == pytest.approx(iso["s2"], rel=1e-9)


def test_ard_refit_on_the_specification_finds_the_irrelevant_inputs():
    """The check that ARD is exercised and not an isotropic shortcut: ℓ₂ = ℓ₃ = 5 (the bound), ℓ₁ < 1, and
    a profiled likelihood more than 10 above the isotropic optimum's."""
    from mrbo.ard import ard_log_likelihood_host
    from mrbo.kernels import Matern52
    from mrbo.mle import lbfgs_scalar, profile_log_likelihood_host
    X, y = aniso_design()

    def fg_ard(T):
        r = [ard_log_likelihood_host(X, y, 0, t, SN2, profile=True) for t in T]
        return np.array([-a["ll"] for a in r]), np.array([-a["grad"] for a in r])

    def fg_iso(T):
        r = [profile_log_likelihood_host(X, y, Matern52([float(t[0])]), SN2) for t in T]
        return np.array([-a["ll"] for a in r]), np.array([-a["grad"] for a in r])

    ells, f, g, it = lbfgs_scalar(fg_ard, np.ones(3), [0.1] * 3, [5.0] * 3, iterations=30)
    ell, f_iso, _, _ = lbfgs_scalar(fg_iso, np.ones(1), [0.1], [5.0], iterations=30)
    print(f"ARD optimum {ells} ll_p {-f:.2f} after {it} line searches; isotropic optimum {ell} ll_p {-f_iso:.2f}")
    assert ells[0] < 1.0 and ells[1] == 5.0 and ells[2] == 5.0
    assert -f > -f_iso + 10.0


# ---- ARDSurrogate ---------------------------------------------------------------------------------
def _numpy_gp(X, y, kernel, ells, xs, standardize):
    """Posterior mean and standard deviation of a plain numpy GP with the ARD kernel, raw units."""
    K = ard_K(X, kernel, ells)
    m = y.mean() if standardize else 0.0
    r = y - m
    c = np.linalg.solve(K, r)
    s = math.sqrt(r @ c / len(y)) if standardize else 1.0
    Z, zs = X / ells[:, None], xs / ells[:, None]
    k = _psi1(kernel, np.sqrt(((Z[:, :, None] - zs[:, None, :]) ** 2).sum(0)))
    μ = m + k.T @ c
    σ = s * np.sqrt(np.maximum(1.0 - (k * np.linalg.solve(K, k)).sum(0), 0.0))
    return μ, σ


def _branin_design(N=12):
    from mrbo import testfns
    f = testfns.TestBraninHoo()
    lbs, ubs = f.get_bounds()
    X = lbs[:, None] + (ubs - lbs)[:, None] * np.random.default_rng(7).random((2, N))
    return X, f(X), lbs, ubs


@pytest.mark.parametrize("standardize", [False, True])
def test_ard_surrogate_against_numpy(standardize):
    from mrbo.ard import ARDSurrogate
    from mrbo.kernels import Matern52
    X, y, lbs, ubs = _branin_design()
    ells = np.array([3.0, 4.5])
    s = ARDSurrogate(Matern52(), X, y, ells=ells, capacity=20, standardize=standardize)
    n = s.observed
    np.testing.assert_allclose(s.inner.K[:n, :n], ard_K(X, "matern52", ells), rtol=1e-13, atol=0)
    xs = lbs[:, None] + (ubs - lbs)[:, None] * np.random.default_rng(8).random((2, 9))
    μ, σ = s.posterior(xs)
    μr, σr = _numpy_gp(X, y, "matern52", ells, xs, standardize)
    np.testing.assert_allclose(μ, μr, rtol=1e-7, atol=1e-7 * np.abs(y).max())
    np.testing.assert_allclose(σ, σr, rtol=1e-5, atol=1e-6 * (σr.max() + 1.0))
    μ1, σ1 = s.posterior(xs[:, 0])
    assert (μ1, σ1) == pytest.approx((μ[0], σ[0]), rel=1e-12)     # one point: floats (BLAS may sum in another order)
    np.testing.assert_allclose(s.unwhiten(s.whiten(xs)), xs, rtol=1e-15, atol=0)
    np.testing.assert_allclose(s.unwhiten(s.whiten(xs[:, 0])), xs[:, 0], rtol=1e-15, atol=0)
    zl, zu = s.whitened_box(lbs, ubs)
    np.testing.assert_array_equal(zl, lbs / ells)
    np.testing.assert_array_equal(zu, ubs / ells)
    assert s.get_active_covariates().shape == (2, n) and (s.get_active_observations() == y).all()


def _same_fit(a, b):
    n = a.observed
    assert b.observed == n
    np.testing.assert_array_equal(a.X[:, :n], b.X[:, :n])
    np.testing.assert_array_equal(a.ells, b.ells)
    for name in ("K", "L"):
        np.testing.assert_allclose(getattr(a.inner, name)[:n, :n], getattr(b.inner, name)[:n, :n], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(a.inner.c[:n], b.inner.c[:n], rtol=1e-6, atol=1e-9 * np.abs(b.inner.c[:n]).max())
    np.testing.assert_allclose(a.inner.y[:n], b.inner.y[:n], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("standardize", [False, True])
def test_ard_surrogate_maintenance_equals_fresh_fits(standardize):
    from mrbo.ard import ARDSurrogate
    from mrbo.kernels import Matern52
    X, y, lbs, ubs = _branin_design()
    ells = np.array([3.0, 4.5])
    fresh = lambda Xf, yf, e: ARDSurrogate(Matern52(), Xf, yf, ells=e, capacity=20, standardize=standardize)
    s = fresh(X[:, :10], y[:10], ells)
    v0 = s.version
    assert s.condition(X[:, 10], y[10]) is s
    s.condition(X[:, 11], y[11])
    assert s.version > v0
    _same_fit(s, fresh(X, y, ells))
    s.set_lengthscales([1.5, 6.0])
    _same_fit(s, fresh(X, y, np.array([1.5, 6.0])))
    s.reset(X[:, :7], y[:7])
    _same_fit(s, fresh(X[:, :7], y[:7], np.array([1.5, 6.0])))
    with pytest.raises(ValueError, match="positive finite"):
        s.set_lengthscales([1.0, 0.0])


def test_ard_surrogate_at_equal_lengthscales_is_the_isotropic_surrogate():
    from mrbo.ard import ARDSurrogate
    from mrbo.kernels import Matern52
    from mrbo.surrogates import Surrogate
    X, y, _, _ = _branin_design()
    a = ARDSurrogate(Matern52(), X, y, ells=(2.0, 2.0), capacity=12)
    b = Surrogate(Matern52([2.0]), X, y, capacity=12)
    np.testing.assert_allclose(a.inner.K, b.K, rtol=1e-13, atol=0)
    d = ARDSurrogate(Matern52([2.0]), X, y, capacity=12)          # the default: ψ's ℓ in every dimension
    np.testing.assert_array_equal(d.ells, [2.0, 2.0])
    np.testing.assert_array_equal(d.inner.K, a.inner.K)
    assert d.inner.ψ.lengthscale == 1.0


def test_periodic_has_no_ard_form():
    from mrbo.ard import ARDSurrogate, ard_log_likelihood_host
    from mrbo.kernels import Periodic
    X, y, _, _ = _branin_design()
    with pytest.raises(ValueError, match="Periodic"):
        ARDSurrogate(Periodic(), X, y)
    with pytest.raises(ValueError, match="Periodic"):
        ard_log_likelihood_host(X, y, 4, [1.0, 1.0], SN2)


# ---- argument checks of the entry points (before any HIP call) ---------------------------------------
def _call(which, d=2, N=4, kernel=0, S=2, P=2, null=None, lo=0.1, hi=5.0, profile=True):
    from mrbo import _lib
    L = _lib.load()
    dp = ctypes.POINTER(ctypes.c_double)
    X = np.asfortranarray(np.arange(d * N, dtype=np.float64).reshape(d, N) / (d * N))
    y = np.linspace(-1.0, 1.0, N)
    sd = _lib.SurrogateDesc(d, N, kernel, 1.0, SN2, 0.0, X.ctypes.data_as(dp), None, N, None, y.ctypes.data_as(dp), 1.0)
    arr = (_lib.SurrogateDesc * 2)(sd, sd)
    n = 2 * max(P, 1)
    a = dict(ells=np.ones(n * d), ll=np.zeros(n), grad=np.zeros(n * d), s2=np.zeros(n), st=np.zeros(n, dtype=np.int32),
             lo=np.full(d, lo), hi=np.full(d, hi), its=np.zeros(2, dtype=np.int32))
    if not profile:
        null = "s2" if null is None else null
    vp = lambda k: None if k == null else ctypes.c_void_p(a[k].ctypes.data)
    H = _lib.MRBO_FLAG_HOST_POINTERS
    if which == "fit":
        rc = L.mrbo_gp_fit_ard_multi(arr, S, P, vp("ells"), vp("ll"), vp("grad"), vp("s2"), vp("st"), None, None, H, None)
    else:
        res = (ctypes.c_int32 * 2)()
        rc = L.mrbo_gp_optimize_ard_multi(arr, S, vp("ells"), vp("lo"), vp("hi"), None, vp("ells"), vp("ll"), vp("grad"),
                                          vp("s2"), vp("its"), res, H, None)
    return rc, L.mrbo_last_error()


@pytest.mark.parametrize("which", ["fit", "optimize"])
def test_ard_entry_points_check_their_arguments_before_any_device_call(which):
    rc, msg = _call(which, kernel=4)
    assert rc == MRBO_ERR_ARG and b"Periodic" in msg
    rc, msg = _call(which, N=129)
    assert rc == MRBO_ERR_UNSUPPORTED and b"128" in msg
    rc, msg = _call(which, d=17)
    assert rc == MRBO_ERR_UNSUPPORTED and b"16" in msg
    rc, msg = _call(which, S=0)
    assert rc == MRBO_ERR_ARG and b"S=0" in msg
    for k in ("ells", "ll", "grad") + (("st",) if which == "fit" else ("lo", "hi", "its")):
        assert _call(which, null=k)[0] == MRBO_ERR_ARG, k
    if which == "fit":
        assert _call(which, P=0)[0] == MRBO_ERR_ARG
    else:
        rc, msg = _call(which, lo=2.0, hi=1.0)
        assert rc == MRBO_ERR_ARG and b"bounds" in msg
        assert _call(which, hi=np.inf)[0] == MRBO_ERR_ARG
        assert _call(which, lo=np.nan)[0] == MRBO_ERR_ARG


def test_ard_needs_optimize_and_defaults_to_off(tmp_path):
    import inspect
    from mrbo import bayesopt
    with pytest.raises(ValueError, match="optimize"):
        bayesopt.run("braninhoo", str(tmp_path), budget=1, trials=1, ard=True, optimize=False, log=lambda *_: None)
    with pytest.raises(ValueError, match="optimize"):
        bayesopt.run_myopic("braninhoo", str(tmp_path), budget=1, trials=1, ard=True, optimize=False, log=lambda *_: None)
    for f in (bayesopt.run, bayesopt.run_myopic):
        assert inspect.signature(f).parameters["ard"].default is False
    assert bayesopt.parse(["--output-dir", "o", "--function-name", "braninhoo"]).ard is False
    assert bayesopt.parse(["--output-dir", "o", "--function-name", "braninhoo", "--ard", "--optimize"]).ard is True
