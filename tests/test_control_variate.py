"""The EI control variate, the host side: the NumPy specification mrbo/variance.py
against mpmath, against central differences, on synthetic arrays and on the CPU oracle's
trajectories; the argument checks of the three new entry points (they return before the plan is read
and before any HIP call, so a stand-in plan pointer serves, as in tests/test_rollout_solve.py); the
CLI flag.  The device side is tests/test_gpu_control_variate.py."""
import ctypes
import functools

import numpy as np
import pytest

import conftest  # noqa: F401  (sys.path)

import mpmath as mp  # noqa: E402  (as tests/test_gpu_primitives.py)

mp.mp.dps = 40

MRBO_ERR_ARG = -1
_BUF = np.zeros(64)                                   # every array argument: never read or written
_PLAN = ctypes.create_string_buffer(64)               # the stand-in plan

# ei0 forms φ + uΦ from libm's exp and erfc: DESIGN.md §14's 4 × rule gives that closed form
# 7335·(1 + u²) ulp (tests/test_gpu_primitives.py C_EI_TAIL, host maximum 1833.6); the product with σ
# adds half an ulp
C_EI0 = 7336


def test_ei0_against_mpmath():
    from mrbo import variance as V
    rng = np.random.default_rng(7)
    u = np.concatenate([np.linspace(-30.0, 8.0, 400), rng.uniform(-30.0, 8.0, 600), [0.0, -0.0, 1e-300, -1e-300]])
    sigma = np.concatenate([np.geomspace(1e-8, 10.0, 400), 10.0 ** rng.uniform(-8.0, 1.0, 600), [1.0, 1e-8, 10.0, 0.5]])
    # inputs that reproduce u exactly: μ = 0 and fmini = u·σ would round; hand ei0 (μ, σ) with
    # fmini − μ = u·σ and take u back from what ei0 itself divides
    fmini = 0.25
    mu = fmini - u * sigma
    uu = (fmini - mu) / sigma
    ei, _ = V.ei0(mu, sigma, np.zeros((1, u.size)), np.zeros((1, u.size)), fmini)
    ref = [mp.mpf(float(s_)) * (mp.mpf(float(x)) * mp.ncdf(mp.mpf(float(x))) + mp.npdf(mp.mpf(float(x))))
           for x, s_ in zip(uu, sigma)]
    worst = 0.0
    for v, r, x in zip(ei, ref, uu):
        ulp = float(np.spacing(abs(float(r)))) if float(r) != 0.0 else 2.0 ** -1074
        err = float(abs(mp.mpf(float(v)) - r) / mp.mpf(ulp)) / (1.0 + x * x)
        worst = max(worst, err)
    print(f"ei0 vs mpmath: {worst:.1f} (1 + u²)-ulp, limit {C_EI0}")
    assert worst <= C_EI0, worst


def test_ei0_gradient_against_central_differences():
    """∇EI0 = φ(u)·∇σ − Φ(u)·∇μ along the line (μ, σ) = (μ0 + t·gμ, σ0 + t·gσ).  With step 1e-5, σ0 in
    [0.5, 2], |u| ≤ 3 and |gμ|, |gσ| ≤ 1 the central difference is off by h²/6·|f'''| ≤ 1e-10·few and by
    the rounding of two EI0 values over 2h, ≤ 1e-15·10/1e-5 = 1e-9: the bar is 1e-8."""
    from mrbo import variance as V
    rng = np.random.default_rng(11)
    n, h, fmini = 200, 1e-5, -0.3
    sigma = rng.uniform(0.5, 2.0, n)
    u = rng.uniform(-3.0, 3.0, n)
    mu = fmini - u * sigma
    gmu, gsig = rng.uniform(-1.0, 1.0, (1, n)), rng.uniform(-1.0, 1.0, (1, n))
    _, g = V.ei0(mu, sigma, gmu, gsig, fmini)
    zero = np.zeros((1, n))
    fp, _ = V.ei0(mu + h * gmu[0], sigma + h * gsig[0], zero, zero, fmini)
    fm, _ = V.ei0(mu - h * gmu[0], sigma - h * gsig[0], zero, zero, fmini)
    err = np.abs(g[0] - (fp - fm) / (2.0 * h)).max()
    print(f"∇EI0 vs central differences: {err:.2e}")
    assert err <= 1e-8, err


# ---- cv_rows on synthetic arrays ---------------------------------------------------------------------
def _synthetic(M=48, K=5, d=3, seed=3):
    rng = np.random.default_rng(seed)
    b = rng.normal(size=(M, K))
    gb = rng.normal(size=(d, M, K))
    a = 0.7 * b + 0.3 * rng.normal(size=(M, K)) + 1.5
    ga = -0.4 * gb + 0.5 * rng.normal(size=(d, M, K))
    gt = rng.normal(size=(M, K))
    return a, ga, gt, b, gb, rng.normal(size=K), rng.normal(size=(d, K))


def test_cv_rows_target_equal_to_control():
    from mrbo import variance as V
    a, ga, gt, _, _, e, ge = _synthetic()
    eto, beta = V.cv_rows(a, ga, gt, a.copy(), ga.copy(), e, ge)
    d = ga.shape[0]
    assert np.array_equal(beta, np.ones_like(beta))
    assert np.array_equal(eto[:, 1], np.zeros(a.shape[1])) and np.array_equal(eto[:, 2 + d:2 + 2 * d], np.zeros((a.shape[1], d)))
    for got, abar, ee in [(eto[:, 0], a.mean(axis=0), e)] + [(eto[:, 2 + k], ga[k].mean(axis=0), ge[k]) for k in range(d)]:
        bound = 2.0 * np.spacing(np.maximum(np.abs(abar), np.abs(ee)))
        assert (np.abs(got - ee) <= bound).all(), (got, ee, bound)
    # ∇θ: the plain columns
    plain = V.plain_rows(a, ga, gt, d)
    assert np.array_equal(eto[:, 2 + 2 * d:], plain[:, 2 + 2 * d:])


@pytest.mark.parametrize("case", ["constant", "nan", "M=1"])
def test_cv_rows_fall_back_to_the_plain_row(case):
    from mrbo import variance as V
    M = 1 if case == "M=1" else 48
    a, ga, gt, b, gb, e, ge = _synthetic(M=M)
    d = ga.shape[0]
    if case == "constant":
        b, gb = np.full_like(b, 0.25), np.full_like(gb, -3.0)
    elif case == "nan":
        b, gb = b.copy(), gb.copy()
        b[3], gb[:, 5] = np.nan, np.nan
    e, ge = np.full_like(e, np.nan), np.full_like(ge, np.nan)      # never read by a plain row
    with np.errstate(all="ignore"):
        eto, beta = V.cv_rows(a, ga, gt, b, gb, e, ge)
        plain = V.plain_rows(a, ga, gt, d)
    assert np.array_equal(beta, np.zeros_like(beta))
    assert np.array_equal(eto, plain, equal_nan=True)
    if M > 1:
        assert np.isfinite(eto).all()
        np.testing.assert_allclose(eto[:, 0], a.mean(axis=0), rtol=1e-14)
        np.testing.assert_allclose(eto[:, 1], a.std(axis=0, ddof=1), rtol=1e-13)
    else:
        assert np.array_equal(eto[:, 0], a[0]) and np.isnan(eto[:, 1]).all()


def test_cv_rows_never_raise_the_std():
    """Σ(da − β·db)² = Saa − Sab²/Sbb ≤ Saa: an identity, so the bar is rounding only."""
    from mrbo import variance as V
    for seed in range(5):
        a, ga, gt, b, gb, e, ge = _synthetic(seed=seed)
        d = ga.shape[0]
        eto, beta = V.cv_rows(a, ga, gt, b, gb, e, ge)
        plain = V.plain_rows(a, ga, gt, d)
        cols = [1] + list(range(2 + d, 2 + 2 * d))
        assert (beta != 0.0).all()
        assert (eto[:, cols] <= plain[:, cols] * (1.0 + 1e-12)).all()
        assert (eto[:, cols] < 0.99 * plain[:, cols]).any()      # and the correlated series do gain


def test_cv_rows_without_gradients():
    from mrbo import variance as V
    a, ga, gt, b, gb, e, ge = _synthetic()
    d = ga.shape[0]
    full, bf = V.cv_rows(a, ga, gt, b, gb, e, ge)
    eto, beta = V.cv_rows(a, None, None, b, None, e, ge)
    assert np.array_equal(eto[:, :2], full[:, :2]) and np.array_equal(beta[0], bf[0])
    assert np.array_equal(eto[:, 2:], np.zeros((a.shape[1], 2 * d + 2))) and np.array_equal(beta[1:], np.zeros((d, a.shape[1])))


# ---- on the oracle's trajectories --------------------------------------------------------------------
D, N, H, M, R = 2, 12, 1, 64, 3
LBS, UBS = -np.ones(D), 2.0 * np.ones(D)


def _objective(X):
    """Smooth, of scale 0.45 under the unit-variance prior: EI is of order 1e-1 near the incumbent."""
    U = (X - LBS[:, None]) / (UBS - LBS)[:, None]
    return 0.3 * (np.sin(3.0 * U.sum(axis=0)) + 0.5 * np.cos(5.0 * U[0]))


@functools.lru_cache(maxsize=None)
def _oracle_runs():
    """The oracle at h = 1 and at h = 0 on the step-0 slab, once.  Kronecker design from offset 0:
    with it the oracle alone meets the 6·std/√M cap (largest row: 0.12 of it) and restart 1 has
    trajectories of both kinds."""
    from oracle import oracle as O
    from mrbo.decision_rules import EI
    from mrbo.kernels import Matern52
    from mrbo.surrogates import Surrogate
    from mrbo.utils import kronecker_quasirand
    X = LBS[:, None] + (UBS - LBS)[:, None] * kronecker_quasirand(D, N, 0)
    s = Surrogate(Matern52((1.0,)), X, _objective(X), capacity=N, decision_rule=EI(), σn2=1e-6)
    osur = O.OracleSurrogate(s.X[:, :N], s.L[:N, :N], s.c[:N], s.y[:N], fmini=s.fmini())
    rn = O.gen_low_discrepancy_sequence(M, D, H + 1)
    xs = O.generate_initial_guesses(4, LBS, UBS)
    x0 = LBS[:, None] + (UBS - LBS)[:, None] * np.array([[0.2, 0.55, 0.8], [0.3, 0.6, 0.15]])
    full = O.simulate_mc(osur, x0, rn, xs, LBS, UBS, H)
    ctl = O.simulate_mc(osur, x0, np.asfortranarray(rn[:, :, :1]), xs, LBS, UBS, 0)
    base = O.eval_base(osur, x0)
    assert not full["status"].any() and not ctl["status"].any()
    return full, ctl, base, s.fmini()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_oracle_trajectories_whose_best_step_is_zero_equal_their_control(oracle):
    full, ctl, _, _ = _oracle_runs()
    best0 = np.argmin(full["obs"], axis=0) == 0                   # M×R (argmin: the first minimum, as resolve)
    assert best0.any() and (~best0).any()
    assert np.array_equal(_bits(full["values"][best0]), _bits(ctl["values"][best0]))
    assert np.array_equal(_bits(full["grad_x"][:, best0]), _bits(ctl["grad_x"][:, best0]))
    assert not np.array_equal(_bits(full["values"][~best0]), _bits(ctl["values"][~best0]))


def test_oracle_rows_with_the_control(oracle):
    from mrbo import variance as V
    full, ctl, base, fmini = _oracle_runs()
    ei, gei = V.ei0(base[0], base[1], base[3:3 + D], base[3 + D:3 + 2 * D], fmini)
    eto, beta = V.cv_rows(full["values"], full["grad_x"], full["grad_theta"][0], ctl["values"], ctl["grad_x"], ei, gei)
    plain = V.plain_rows(full["values"], full["grad_x"], full["grad_theta"][0], D)
    np.testing.assert_allclose(plain, full["eto"].T, rtol=1e-12, atol=1e-15)   # the oracle's own plain rows
    cap = 6.0 * plain[:, 1] / np.sqrt(M)
    print("|mean_cv − mean_plain| / cap:", np.abs(eto[:, 0] - plain[:, 0]) / cap, "β:", beta[0])
    assert (beta[0] != 0.0).any()
    assert (np.abs(eto[:, 0] - plain[:, 0]) <= cap).all()
    cols = [1] + list(range(2 + D, 2 + 2 * D))
    use = np.vstack([beta[0][None], beta[1:]]).T != 0.0            # R×(1+d)
    assert (eto[:, cols][use] <= plain[:, cols][use] * (1.0 + 1e-12)).all()


def test_oracle_horizon_zero_rows_are_the_base_acquisition(oracle):
    """At h = 0 the target IS the control: β = 1, std = 0 and the row is EI0, ∇EI0 -- the oracle's α
    and ∇α (EI, θ = 0) wherever the control varies."""
    from mrbo import variance as V
    _, ctl, base, fmini = _oracle_runs()
    ei, gei = V.ei0(base[0], base[1], base[3:3 + D], base[3 + D:3 + 2 * D], fmini)
    eto, beta = V.cv_rows(ctl["values"], ctl["grad_x"], None, ctl["values"], ctl["grad_x"], ei, gei)
    use = beta[0] != 0.0
    assert use.any()
    assert np.array_equal(beta[:, use], np.ones((1 + D, int(use.sum())))) and np.array_equal(eto[use, 1], np.zeros(int(use.sum())))
    alpha, galpha = base[2], base[3 + 2 * D:3 + 3 * D]
    # the oracle's α is imp·Φ + σ·φ, EI0 is σ·(u·Φ + φ): the same sum, associated differently, each
    # within (1 + u²) ulp-thousands of the exact value (C_EI0); |u| ≤ 3 here
    np.testing.assert_allclose(eto[use, 0], alpha[use], rtol=1e-10)
    np.testing.assert_allclose(eto[use, 2:2 + D], galpha[:, use].T, rtol=1e-10, atol=1e-12)


# ---- argument errors, without a device ---------------------------------------------------------------
def _p(null=False):
    return None if null else ctypes.c_void_p(_BUF.ctypes.data)


def _plan(null=False):
    return None if null else ctypes.cast(_PLAN, ctypes.c_void_p)


def _control(null=(), flags=0):
    from mrbo import _lib
    L = _lib.load()
    a = {k: _p(k in null) for k in ("x0s", "rnstream", "xstarts", "values0", "grad_x0", "status0")}
    rc = L.mrbo_simulate_control(_plan("plan" in null), a["x0s"], a["rnstream"], a["xstarts"], a["values0"],
                                 a["grad_x0"], a["status0"], flags, None)
    return rc, L.mrbo_last_error()


@pytest.mark.parametrize("name", ["plan", "x0s", "rnstream", "xstarts", "values0", "grad_x0", "status0"])
def test_simulate_control_rejects_null_arguments(name):
    rc, msg = _control(null=(name,))
    assert rc == MRBO_ERR_ARG and b"null" in msg, msg


@pytest.mark.parametrize("flags", [4, 8, 1 | 4, 2 | 16])
def test_simulate_control_rejects_unknown_flags(flags):
    rc, msg = _control(flags=flags)
    assert rc == MRBO_ERR_ARG and b"flags" in msg, msg


def _reduce(null=(), flags=0):
    from mrbo import _lib
    L = _lib.load()
    names = ("x0s", "values", "grad_x", "grad_theta", "values0", "grad_x0", "eto", "beta")
    a = {k: _p(k in null) for k in names}
    rc = L.mrbo_eto_reduce_cv(_plan("plan" in null), *[a[k] for k in names], flags, None)
    return rc, L.mrbo_last_error()


@pytest.mark.parametrize("name", ["plan", "x0s", "values", "values0", "grad_x0", "eto"])
def test_eto_reduce_cv_rejects_null_arguments(name):
    rc, msg = _reduce(null=(name,))
    assert rc == MRBO_ERR_ARG and b"null" in msg, msg


@pytest.mark.parametrize("flags", [1, 2, 4])
def test_eto_reduce_cv_rejects_flags(flags):
    rc, msg = _reduce(flags=flags)
    assert rc == MRBO_ERR_ARG and b"flags" in msg, msg


def test_set_control_variate_rejects_a_null_plan():
    from mrbo import _lib
    L = _lib.load()
    assert L.mrbo_plan_set_control_variate(None, 1) == MRBO_ERR_ARG and b"null" in L.mrbo_last_error()


# ---- the CLI and the defaults ------------------------------------------------------------------------
def test_cli_accepts_variance_reduction():
    from mrbo import bayesopt
    base = ["--output-dir", "o", "--function-name", "gramacylee"]
    assert bayesopt.parse(base).variance_reduction is False
    assert bayesopt.parse(base + ["--variance-reduction"]).variance_reduction is True


@pytest.mark.parametrize("name", ["rollout_solve", "rollout_solve_multi", "run"])
def test_variance_reduction_is_off_by_default(name):
    import inspect
    from mrbo import bayesopt, utils
    assert inspect.signature(getattr(bayesopt, name)).parameters["variance_reduction"].default is False
    for f in (utils.stochastic_solve_batch, utils.stochastic_solve_multi):
        assert inspect.signature(f).parameters["variance_reduction"].default is False
