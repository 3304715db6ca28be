"""The fitted output scale on the device: mrbo_gp_fit_profile_multi against the
numpy specification (mle.profile_log_likelihood_host) on each of the three fit kernels, with a
failing and a constant slot in the launch; its blocks against the S = 1 call and its factors against
the plain call's, bit for bit; mrbo_gp_optimize_profile_multi against mle.lbfgs_scalar driven by the
profile fit call, bit for bit; one acquisition solve on a Goldstein–Price design, where the raw
surrogate leaves the restarts without a gradient and the standardised one does not; and the BO
loops with standardize=True across their four paths.  The host side is tests/test_standardize.py."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import conftest  # noqa: F401  (sys.path)

pytestmark = pytest.mark.gpu

S, P = 3, 4
BAD_Q, BAD_P, CONST_Q = 0, 2, 1     # the slot whose θ fails Cholesky, the constant data set


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _kernel(name, theta):
    from mrbo import kernels
    return {"matern52": kernels.Matern52, "periodic": kernels.Periodic}[name](list(theta))


def _centred_data(d, N, seed):
    """Observations of a scale far from 1 (the reason for the profile), centred as the caller of
    the profile entry points centres them."""
    rng = np.random.default_rng(seed)
    X = rng.random((d, N)) * (3.0 if d == 1 else 1.0)
    y = 300.0 * (np.sin(3 * X.sum(0)) + 0.1 * rng.standard_normal(N)) + 1000.0
    return X, y - y.mean()


def _fit_case(kernel, d, N, constant=True):
    """S surrogates and (S, P[, nt]) hyperparameters.  Data set CONST_Q is constant (zeros after
    centring).  Matérn-5/2: slot (BAD_Q, BAD_P) has ℓ = −1, which puts off-diagonal entries far above
    the diagonal, so no Cholesky exists.  Periodic: ℓ and p enter ψ through squares and no finite θ
    breaks K on these data; that case carries the constant data set alone."""
    from mrbo.surrogates import Surrogate
    sn2 = 1e-6 if kernel == "matern52" else 1e-3
    surs = []
    for q in range(S):
        X, r = _centred_data(d, N, seed=1000 * d + 10 * N + q)
        if constant and q == CONST_Q:
            r = np.zeros(N)
        surs.append(Surrogate(_kernel(kernel, [1.0] if kernel == "matern52" else [1.0, 1.0]), X, r, capacity=N, σn2=sn2))
    if kernel == "matern52":
        th = np.stack([np.array([0.3, 0.7, 0.9, 1.5]) * (1.0 + 0.07 * q) for q in range(S)])
        th[BAD_Q, BAD_P] = -1.0
    else:
        base = np.array([[0.7, 1.3], [1.5, 0.8], [2.0, 2.5], [0.5, 1.9]])
        th = np.stack([base * (1.0 + 0.05 * q) for q in range(S)])
    return surs, th, sn2


def _spec(s, theta, sn2):
    """profile_log_likelihood_host at one slot: its dict, or the status the device must report."""
    from mrbo.mle import profile_log_likelihood_host
    n = s.observed
    θ = np.atleast_1d(theta)
    ψ = _kernel("matern52" if len(s.ψ.θ) == 1 else "periodic", θ)
    try:
        return profile_log_likelihood_host(s.X[:, :n], s.y[:n], ψ, sn2)
    except np.linalg.LinAlgError:
        return 1
    except ValueError:
        return 2


FIT_SHAPES = [
    pytest.param("matern52", 2, 20, id="tile-one-tile"),
    pytest.param("matern52", 2, 48, id="register"),
    pytest.param("matern52", 2, 72, id="lds"),
    pytest.param("matern52", 2, 96, id="tile-three-rows"),
    pytest.param("periodic", 1, 20, id="periodic-nt2"),
]


@pytest.mark.parametrize("kernel,d,N", FIT_SHAPES)
def test_fit_profile_multi_against_the_numpy_specification(gpu, kernel, d, N):
    """ll_p, ∂ll_p and ŝ² of every good slot within the bars tests/test_mle.py holds the plain ll and
    gradient to (rtol 1e-8, atol 1e-8·(1 + |ll|); ŝ² rtol 1e-8); status 1 where the specification's
    Cholesky fails, status 2 in every slot of the constant data set, NaN outputs there, and the
    other slots carry the bits of a launch without either."""
    from mrbo.mle import gp_fit_multi
    surs, th, sn2 = _fit_case(kernel, d, N)
    r = gp_fit_multi(surs, th, profile=True)
    nt = th.shape[2] if th.ndim == 3 else 1
    assert r["ll"].shape == (S, P) and r["s2"].shape == (S, P) and r["grad"].shape == (S, P, nt)
    expect = np.zeros((S, P), dtype=np.int32)
    for q in range(S):
        for p in range(P):
            sp = _spec(surs[q], th[q, p], sn2)
            if not isinstance(sp, dict):
                expect[q, p] = sp
                continue
            ll, g, s2 = r["ll"][q, p], r["grad"][q, p], r["s2"][q, p]
            tol = 1e-8 * (1 + abs(sp["ll"]))
            print(f"N={N} q={q} p={p}: ll {ll:.15g} (spec {sp['ll']:.15g}, Δ {abs(ll - sp['ll']):.2e}, bar {tol + 1e-8 * abs(sp['ll']):.2e}) "
                  f"grad Δ {np.abs(g - sp['grad']).max():.2e} s2 rel Δ {abs(s2 / sp['s2'] - 1):.2e} "
                  f"cond {np.linalg.cond(sp['L'] @ sp['L'].T):.1e}")
            assert r["status"][q, p] == 0
            assert ll == pytest.approx(sp["ll"], rel=1e-8, abs=tol)
            assert g == pytest.approx(sp["grad"], rel=1e-8, abs=tol)
            assert s2 == pytest.approx(sp["s2"], rel=1e-8)
    assert (expect[CONST_Q] == 2).all() and (np.delete(expect, CONST_Q, axis=0) != 2).all()
    if kernel == "matern52":
        assert expect[BAD_Q, BAD_P] == 1 and expect.sum() == 1 + 2 * P
    assert np.array_equal(r["status"], expect), r["status"]
    bad = expect != 0
    assert np.isnan(r["ll"][bad]).all() and np.isnan(r["s2"][bad]).all() and np.isnan(r["grad"][bad]).all()
    assert np.isfinite(r["ll"][~bad]).all() and np.isfinite(r["grad"][~bad]).all() and (r["s2"][~bad] > 0).all()
    # the same launch without the failing θ and without the constant data set: the other slots' bits
    surs2, th2, _ = _fit_case(kernel, d, N, constant=False)
    if kernel == "matern52":
        th2[BAD_Q, BAD_P] = 0.9
    r2 = gp_fit_multi(surs2, th2, profile=True)
    assert (r2["status"] == 0).all()
    for k in ("ll", "grad", "s2"):
        assert same_bits(r[k][~bad], r2[k][~bad]), k
    # the amplitude was worth fitting: the data are not of unit scale
    assert r["s2"][~bad].min() > 100.0


@pytest.mark.parametrize("kernel,d,N", FIT_SHAPES)
def test_profile_blocks_equal_single_calls_and_factors_equal_the_plain_calls(gpu, kernel, d, N):
    """Block q of the batch is the S = 1 call's, bit for bit (NaNs included), with and without the
    factor outputs; L and c do not depend on the amplitude and are the plain call's."""
    from mrbo.mle import gp_fit_batch, gp_fit_multi
    surs, th, _ = _fit_case(kernel, d, N)
    for want_fit in (False, True):
        r = gp_fit_multi(surs, th, want_fit=want_fit, profile=True)
        for q, s in enumerate(surs):
            one = gp_fit_batch(s, th[q], want_fit=want_fit, profile=True)
            for k in ("ll", "grad", "dll", "s2", "status"):
                assert same_bits(r[k][q], one[k]), (want_fit, q, k)
            if want_fit:
                plain = gp_fit_batch(s, th[q], want_fit=True)
                ok = plain["status"] == 0          # a failed Cholesky writes neither
                assert same_bits(r["L"][q][:, :, ok], plain["L"][:, :, ok]), q
                assert same_bits(r["c"][q][:, ok], plain["c"][:, ok]), q
                assert same_bits(one["L"][:, :, ok], plain["L"][:, :, ok]) and same_bits(one["c"][:, ok], plain["c"][:, ok])
                assert np.array_equal(plain["status"] == 1, r["status"][q] == 1)
        assert not same_bits(r["ll"][0], r["ll"][2])


def test_profile_fit_device_pointers(gpu):
    """Device-pointer mode gives the bits of host-pointer mode (s2 included)."""
    import torch
    from mrbo import _lib
    from mrbo.mle import gp_fit_multi
    surs, th, _ = _fit_case("matern52", 2, 48)
    host = gp_fit_multi(surs, th, profile=True)
    L = _lib.load()
    n = 48
    dp = ctypes.POINTER(ctypes.c_double)
    keep = [(np.asfortranarray(s.X[:, :n]), np.ascontiguousarray(s.y[:n])) for s in surs]
    sds = (_lib.SurrogateDesc * S)(*[
        _lib.SurrogateDesc(2, n, int(s.ψ.kind), 1.0, float(s.σn2), 0.0, X.ctypes.data_as(dp), None, n, None,
                           y.ctypes.data_as(dp), 1.0) for s, (X, y) in zip(surs, keep)])
    t = lambda a: torch.from_numpy(a).to("cuda:0")
    bufs = [t(np.ascontiguousarray(th)), t(np.zeros((S, P))), t(np.zeros((S, P))), t(np.zeros((S, P))),
            t(np.zeros((S, P), dtype=np.int32))]
    torch.cuda.synchronize()
    p = lambda a: ctypes.c_void_p(a.data_ptr())
    _lib.check(L.mrbo_gp_fit_profile_multi(sds, S, P, 1, p(bufs[0]), p(bufs[1]), p(bufs[2]), p(bufs[3]), p(bufs[4]),
                                           None, None, 0, None))
    ll, grad, s2, st = [b.cpu().numpy() for b in bufs[1:]]
    assert same_bits(ll, host["ll"]) and same_bits(grad, host["dll"]) and same_bits(s2, host["s2"])
    assert np.array_equal(st, host["status"])


# ---- the device refit ----------------------------------------------------------------------------
def _mle_surrogates(d, N, seeds):
    from mrbo.surrogates import Surrogate
    out = []
    for seed in seeds:
        rng = np.random.default_rng(seed)
        X = rng.random((d, N))
        y = np.sin(3 * X.sum(0)) + 0.1 * rng.standard_normal(N)
        out.append(Surrogate(_kernel("matern52", [1.0]), X, 50.0 * (y - y.mean()), capacity=N, σn2=1e-6))
    return out


def _lbfgs_spec(s, theta0, lo, hi, c1=1e-4):
    """mle.lbfgs_scalar driven by the profile fit call on one data set alone; beside its result the
    line searches made, the trial steps it rejected (the accepted step was not the first) and ŝ² at
    the accepted points, read off the evaluations with the minimiser's own Armijo test."""
    from mrbo.mle import gp_fit_batch, lbfgs_scalar
    st = dict(ls=0, rejected=0, s2=np.nan)

    def fg(T):
        r = gp_fit_batch(s, T, profile=True)
        f, g = np.where(r["status"] == 0, -r["ll"], np.nan), -r["grad"]
        if len(T) == 1:
            st.update(x=T[0].copy(), f=float(f[0]), g=g[0].copy(), s2=float(r["s2"][0]))
        else:
            st["ls"] += 1
            for k in range(len(T)):
                dx = [float(T[k][i] - st["x"][i]) for i in range(T.shape[1])]
                dot = dx[0] * float(st["g"][0])
                for i in range(1, len(dx)):
                    dot = dot + dx[i] * float(st["g"][i])
                if np.isfinite(f[k]) and float(f[k]) <= st["f"] + c1 * dot:
                    st["rejected"] += k
                    st.update(x=T[k].copy(), f=float(f[k]), g=g[k].copy(), s2=float(r["s2"][k]))
                    break
        return f, g
    return lbfgs_scalar(fg, theta0, lo, hi), st


@pytest.mark.parametrize("d,N,seeds,starts", [
    pytest.param(2, 20, (8, 0, 3), (1.0, 4.0, 1.0), id="tile-one-tile"),
    pytest.param(6, 48, (3, 4, 8), (1.0, 4.0, 1.0), id="register"),
])
def test_device_refit_equals_lbfgs_scalar_on_the_profile_fit(gpu, d, N, seeds, starts):
    from mrbo.mle import gp_optimize_multi
    surs = _mle_surrogates(d, N, seeds)
    th0 = np.array(starts).reshape(S, 1)
    specs = [_lbfgs_spec(s, th0[q], [0.1], [5.0]) for q, s in enumerate(surs)]
    print([(sp[3], st["ls"], st["rejected"]) for sp, st in specs])
    # the case exercises the minimiser: line searches in a row and trial steps that Armijo rejects
    assert any(st["ls"] >= 2 for _, st in specs) and any(st["rejected"] >= 1 for _, st in specs)
    r = gp_optimize_multi(surs, th0, [0.1], [5.0], profile_amplitude=True)
    assert r["s2"].shape == (S,)
    for q, ((x, f, g, it), st) in enumerate(specs):
        assert same_bits(r["theta"][q], x), (q, r["theta"][q], x)
        assert same_bits(r["neg_log_likelihood"][q], np.float64(f)) and same_bits(r["gradient"][q], g), q
        assert r["iterations"][q] == it == st["ls"], q
        assert same_bits(r["s2"][q], np.float64(st["s2"])), (q, r["s2"][q], st["s2"])   # the accepted point's
    assert r["stopped_at"] == 1 + max(sp[3] for sp, _ in specs)
    # another objective than the plain likelihood: on data 50× the unit scale the plain refit ends elsewhere
    plain = gp_optimize_multi(surs, th0, [0.1], [5.0])
    assert "s2" not in plain and not same_bits(plain["theta"], r["theta"])


def test_device_refit_device_pointers(gpu):
    """mrbo_gp_optimize_profile_multi with device pointers gives the bits of host-pointer mode, s2 included."""
    import torch
    from mrbo import _lib
    from mrbo.mle import gp_optimize_multi
    surs = _mle_surrogates(2, 20, (8, 0, 3))
    th0 = np.array([[1.0], [4.0], [1.0]])
    host = gp_optimize_multi(surs, th0, [0.1], [5.0], profile_amplitude=True)
    L = _lib.load()
    dp = ctypes.POINTER(ctypes.c_double)
    keep = [(np.asfortranarray(s.X[:, :20]), np.ascontiguousarray(s.y[:20])) for s in surs]
    sds = (_lib.SurrogateDesc * S)(*[
        _lib.SurrogateDesc(2, 20, int(s.ψ.kind), 1.0, float(s.σn2), 0.0, X.ctypes.data_as(dp), None, 20, None,
                           y.ctypes.data_as(dp), 1.0) for s, (X, y) in zip(surs, keep)])
    bufs = [torch.from_numpy(a).to("cuda:0") for a in (th0, np.zeros((S, 1)), np.zeros(S), np.zeros((S, 1)), np.zeros(S),
                                                       np.zeros(S, dtype=np.int32))]
    torch.cuda.synchronize()
    p = lambda a: ctypes.c_void_p(a.data_ptr())
    lo, hi = np.array([0.1]), np.array([5.0])
    h = lambda a: ctypes.c_void_p(a.ctypes.data)
    res = (ctypes.c_int32 * 2)()
    opts = _lib.MleOpts(30, 10, 0.0, 0.0)
    _lib.check(L.mrbo_gp_optimize_profile_multi(sds, S, 1, p(bufs[0]), h(lo), h(hi), ctypes.byref(opts), p(bufs[1]),
                                                p(bufs[2]), p(bufs[3]), p(bufs[4]), p(bufs[5]), res, 0, None))
    theta, nll, grad, s2, its = [b.cpu().numpy() for b in bufs[1:]]
    assert same_bits(theta, host["theta"]) and same_bits(nll, host["neg_log_likelihood"])
    assert same_bits(grad, host["gradient"]) and same_bits(s2, host["s2"]) and np.array_equal(its, host["iterations"])
    assert res[1] == host["stopped_at"] and (s2 > 0).all()


def test_optimize_profiles_a_standardised_surrogate_on_both_paths(gpu):
    """mle.optimize / optimize_multi on Surrogate(standardize=True): the profiled likelihood by
    default, host loop and device call ending at the same θ, and the surrogate restandardised there."""
    import copy
    from mrbo.mle import gp_optimize_multi, optimize, optimize_multi
    from mrbo.surrogates import Surrogate
    raw = _mle_surrogates(2, 20, (8, 0, 3))
    surs = [Surrogate(_kernel("matern52", [1.0]), s.X, 7.0 * s.y + 90.0, capacity=20, σn2=1e-6, standardize=True)
            for s in raw]
    want = gp_optimize_multi(surs, None, [0.1], [5.0], profile_amplitude=True)
    a, b, c = copy.deepcopy(surs), copy.deepcopy(surs), copy.deepcopy(surs)
    host = optimize_multi(a, [0.1], [5.0])
    dev = optimize_multi(b, [0.1], [5.0], device=True)
    alone = [optimize(s, [0.1], [5.0]) for s in c]
    for q in range(S):
        # the device minimiser is lbfgs_scalar's arithmetic, which for one variable is projected_lbfgs's
        for r in (host[q], dev[q], alone[q]):
            assert same_bits(r["theta"], want["theta"][q]) and r["neg_log_likelihood"] == want["neg_log_likelihood"][q]
        fresh = Surrogate(_kernel("matern52", want["theta"][q]), surs[q].X, surs[q].get_active_observations(),
                          capacity=20, σn2=1e-6, standardize=True)
        for s in (a[q], b[q], c[q]):
            assert s.ψ.lengthscale == want["theta"][q, 0] and s.s == fresh.s and same_bits(s.y, fresh.y)
        # ŝ² of the refit on ỹ rescales the amplitude the surrogate ends with
        assert fresh.s == pytest.approx(surs[q].s * np.sqrt(want["s2"][q]), rel=1e-9)


# ---- one acquisition solve -----------------------------------------------------------------------
GP_N, GP_OFFSET = 20, 10    # on the CPU oracle every restart of this design has a zero raw ETO gradient


@functools.lru_cache(maxsize=None)
def _solve(standardize, device_solve):
    from mrbo import bayesopt
    from mrbo.kernels import Matern52
    from mrbo.surrogates import Surrogate
    from mrbo.utils import kronecker_quasirand
    fn = bayesopt.TESTFNS["goldsteinprice"]()
    lbs, ubs = fn.get_bounds()
    X = lbs[:, None] + (ubs - lbs)[:, None] * kronecker_quasirand(2, GP_N, GP_OFFSET)
    sur = Surrogate(Matern52([1.0]), X, fn(X), capacity=GP_N, σn2=1e-6, standardize=standardize)
    trace = []
    xnext, mean = bayesopt.rollout_solve(sur, lbs, ubs, 1, 16, 4, 2, 2, 0.0, eta=0.02, solver="adam", trace=trace,
                                         device_solve=device_solve)
    return xnext, mean, trace[0]


def test_raw_surrogate_has_no_gradient_and_the_standardised_one_has(gpu):
    for standardize, check in ((False, lambda z: z.mean() >= 0.5), (True, lambda z: not z.any())):
        _, _, t = _solve(standardize, False)
        R = t["batch"].shape[1] - 1                       # the Sobol batch; the last restart is the incumbent's
        g = np.stack([e.gradient() for e in t["history"][0][:R]])
        zero = (g == 0.0).all(axis=1)
        print("standardize", standardize, "zero ETO gradients in iteration 1:", zero.tolist())
        assert check(zero), (standardize, g)
    # without a gradient the ascent leaves a restart where it started (BoxAdam maps it to the unit box and
    # back: a rounding of the last bits); with one it moves
    _, _, tr = _solve(False, False)
    g = np.stack([e.gradient() for e in tr["history"][0]])
    still = (g == 0.0).all(axis=1)
    np.testing.assert_allclose(tr["x"][:, still], tr["batch"][:, still], rtol=1e-14, atol=1e-14)
    _, _, ts = _solve(True, False)
    assert (np.abs(ts["x"] - ts["batch"]).max(axis=0) > 0).any()


@pytest.mark.parametrize("standardize", [False, True])
def test_device_solve_equals_the_host_loop(gpu, standardize):
    hx, hm, ht = _solve(standardize, False)
    dx, dm, dt = _solve(standardize, True)
    assert same_bits(hx, dx) and hm == dm
    assert same_bits(ht["x"], np.asarray(dt["x"]).reshape(ht["x"].shape)) and ht["pick"] == dt["pick"]
    assert same_bits(np.asarray(ht["means"], dtype=np.float64), np.asarray(dt["means"], dtype=np.float64).ravel())


# ---- the BO loops --------------------------------------------------------------------------------
BO_KW = dict(horizon=1, budget=2, trials=3, mc_samples=16, batch_size=2, starts=4, sgd_iterations=3, optimize=True)


@functools.lru_cache(maxsize=None)
def _bo(tmp, standardize, lockstep, device):
    from mrbo import bayesopt
    out = os.path.join(tmp, f"s{int(standardize)}l{int(lockstep)}d{int(device)}")
    res = bayesopt.run("rosenbrock", out, standardize=standardize, parallel_trials=3 if lockstep else 1,
                       reuse_surrogate=False, device_mle=device, device_solve=device, log=lambda *_: None, **BO_KW)
    csvs = {}
    for f in sorted(os.listdir(os.path.join(out, "rosenbrock"))):
        if f.endswith(".csv") and "_times" not in f:
            csvs[f] = open(os.path.join(out, "rosenbrock", f)).read()
    return res, csvs


@pytest.fixture(scope="module")
def bo_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("bo"))


def test_standardised_bo_loops_agree_across_their_paths(gpu, bo_dir):
    ref, ref_csv = _bo(bo_dir, True, True, False)
    assert len(ref) == 9                                           # three rules × three trials
    for lockstep, device in ((True, True), (False, False), (False, True)):
        res, csv = _bo(bo_dir, True, lockstep, device)
        assert set(res) == set(ref)
        for key in ref:
            for k in ("X", "y", "gaps", "simple_regret", "minimum_observations"):
                assert same_bits(res[key][k], ref[key][k]), (lockstep, device, key, k)
            assert res[key]["ell_end"] == ref[key]["ell_end"]
        assert csv == ref_csv and len(csv) == 12
    # raw units: y is the objective at X, and the refit moved the lengthscale
    from mrbo import bayesopt
    fn = bayesopt.TESTFNS["rosenbrock"]()
    for key, r in ref.items():
        assert same_bits(r["y"], fn(r["X"])) and r["y"].shape == (7,)
    assert any(r["ell_end"] != r["ell_start"] for r in ref.values())


def test_standardize_off_reproduces_the_recorded_loop(gpu, bo_dir):
    """standardize=False is the loop as it was: X and y of every trial equal those recorded from the
    commit before the option existed (tests/golden/standardize_off_bo.json, float64 as hex), on
    every path; and they are not the standardised loop's."""
    with open(os.path.join(conftest.GOLDEN, "standardize_off_bo.json")) as f:
        gold = json.load(f)
    for lockstep, device in ((True, False), (True, True), (False, False), (False, True)):
        res, _ = _bo(bo_dir, False, lockstep, device)
        assert len(res) == len(gold) == 9
        for (acq, trial), r in res.items():
            g = gold[f"{acq}/{trial}"]
            assert [float(v).hex() for v in r["X"].ravel()] == g["X"], (lockstep, device, acq, trial)
            assert [float(v).hex() for v in r["y"].ravel()] == g["y"], (lockstep, device, acq, trial)
            assert float(r["ell_end"]).hex() == g["ell_end"]
    on, _ = _bo(bo_dir, True, True, False)
    off, _ = _bo(bo_dir, False, True, False)
    assert any(not same_bits(on[k]["X"], off[k]["X"]) for k in on)
