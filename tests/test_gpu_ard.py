"""ARD lengthscales on the device: mrbo_gp_fit_ard_multi against the numpy specification
(mrbo.ard.ard_log_likelihood_host) within the bars tests/test_mle.py holds the isotropic kernels to, its
d = 1 case against the isotropic fit, the independence of its slots bit for bit, its failure statuses;
mrbo_gp_optimize_ard_multi against mle.lbfgs_scalar driven by the fit call, bit for bit; the whitened
evaluation against the isotropic surrogate; and the BO loops with ard=True across their paths.  The host
side is tests/test_ard.py."""
import functools

import numpy as np
import pytest

import conftest  # noqa: F401  (sys.path)
from test_ard import KERNELS, KIND, SN2
from test_gpu_gp_fit_multi import _data, _kernel, same_bits
from test_mle import _ll_tol

pytestmark = pytest.mark.gpu

S, P = 3, 4
SHAPES = [(1, 8), (2, 20), (3, 33), (6, 64), (6, 65), (16, 40), (4, 128)]


def _surrogates(kernel, d, N, centre=False, sn2=SN2, n=S):
    from mrbo.surrogates import Surrogate
    out = []
    for q in range(n):
        X, y = _data(d, N, seed=100 * d + q)
        out.append(Surrogate(_kernel(kernel, [1.0]), X, y - y.mean() if centre else y, capacity=N, σn2=sn2))
    return out


def _candidates(kernel, d):
    """test_gp_fit_vs_oracle's pattern (0.2, 0.5, 1, 2)·√d (× 0.15 for SE) times per-dimension factors
    cycling through (0.5, 1, 2), the cycle shifted by the data set: (S, P, d)."""
    base = np.array([0.2, 0.5, 1.0, 2.0]) * np.sqrt(d) * (0.15 if kernel == "se" else 1.0)
    f = np.array([0.5, 1.0, 2.0])
    return np.stack([base[:, None] * f[(np.arange(d) + q) % 3][None, :] for q in range(S)])


# the largest differences seen per quantity, printed by the last case for DESIGN.md §18
WORST = {}


def _worst(name, v):
    WORST[name] = max(WORST.get(name, 0.0), float(v))


@pytest.mark.parametrize("profile", [False, True], ids=["plain", "profile"])
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("d,N", SHAPES)
def test_fit_against_the_specification(gpu, kernel, d, N, profile):
    from mrbo.ard import ard_log_likelihood_host, gp_fit_ard_multi
    surs = _surrogates(kernel, d, N, centre=profile)
    ells = _candidates(kernel, d)
    r = gp_fit_ard_multi(surs, ells, want_fit=True, profile=profile)
    rr = gp_fit_ard_multi(surs, ells, profile=profile)
    assert r["ll"].shape == (S, P) and r["grad"].shape == (S, P, d) and r["L"].shape == (S, N, N, P)
    for k in ("ll", "grad", "status") + (("s2",) if profile else ()):
        assert same_bits(r[k], rr[k]), k                       # the factor outputs change nothing else
    for q, s in enumerate(surs):
        for p in range(P):
            try:
                ref = ard_log_likelihood_host(s.X[:, :N], s.y[:N], KIND[kernel], ells[q, p], SN2, profile=profile)
            except np.linalg.LinAlgError:
                assert r["status"][q, p] == 1 and np.isnan(r["ll"][q, p])
                continue
            assert r["status"][q, p] == 0, (q, p, r["status"])
            ll, L, c = ref["ll"], ref["L"], ref["c"]
            tol = _ll_tol(ll, L, c)
            gtol = 1e-8 * (1 + abs(ll))
            _worst("ll/tol", abs(r["ll"][q, p] - ll) / tol)
            _worst("grad/(1e-8|g| + atol)", (np.abs(r["grad"][q, p] - ref["grad"]) / (1e-8 * np.abs(ref["grad"]) + gtol)).max())
            assert abs(r["ll"][q, p] - ll) <= tol, (r["ll"][q, p], ll, tol)
            np.testing.assert_allclose(r["grad"][q, p], ref["grad"], rtol=1e-8, atol=gtol)
            if profile:
                _worst("s2 rel", abs(r["s2"][q, p] / ref["s2"] - 1.0))
                assert r["s2"][q, p] == pytest.approx(ref["s2"], rel=1e-8)
            kap = np.linalg.cond(L @ L.T)
            atol = max(1e-12, 10.0 * np.sqrt(kap) * 2.0 ** -53) * np.abs(L).max()
            _worst("L/atol", np.abs(r["L"][q, :, :, p] - L).max() / atol)
            _worst("c rel max", np.abs(r["c"][q, :, p] - c).max() / np.abs(c).max())
            np.testing.assert_allclose(r["L"][q, :, :, p], L, rtol=1e-10, atol=atol)
            assert (np.triu(r["L"][q, :, :, p], 1) == 0.0).all()
            np.testing.assert_allclose(r["c"][q, :, p], c, rtol=1e-8, atol=1e-8 * np.abs(c).max())
    print("largest differences so far:", {k: f"{v:.3g}" for k, v in WORST.items()})


@pytest.mark.parametrize("profile", [False, True], ids=["plain", "profile"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_one_dimension_is_the_isotropic_fit(gpu, kernel, profile):
    from mrbo.ard import gp_fit_ard_batch
    from mrbo.mle import gp_fit_batch
    (s,) = _surrogates(kernel, 1, 8, centre=profile, n=1)
    ells = np.array([0.2, 0.5, 1.0, 2.0]) * (0.15 if kernel == "se" else 1.0)
    a = gp_fit_ard_batch(s, ells[:, None], want_fit=True, profile=profile)
    b = gp_fit_batch(s, ells, want_fit=True, profile=profile)
    assert (a["status"] == 0).all() and (b["status"] == 0).all()
    for p in range(len(ells)):
        ll = b["ll"][p]
        assert abs(a["ll"][p] - ll) <= _ll_tol(ll, b["L"][:, :, p], b["c"][:, p])
        assert a["grad"][p, 0] == pytest.approx(b["dll"][p], rel=1e-8, abs=1e-8 * (1 + abs(ll)))
        if profile:
            assert a["s2"][p] == pytest.approx(b["s2"][p], rel=1e-8)
        np.testing.assert_allclose(a["c"][:, p], b["c"][:, p], rtol=1e-8, atol=1e-8 * np.abs(b["c"][:, p]).max())


@pytest.mark.parametrize("profile", [False, True], ids=["plain", "profile"])
@pytest.mark.parametrize("d,N", [(3, 33), (6, 65)])
def test_slots_are_independent(gpu, d, N, profile):
    """Bad lengthscales (status 3) and, in profile mode, a constant data set (status 2) leave their
    neighbours with the bits of a launch without them; block q is the S = 1 call's, candidate p the
    P = 1 call's."""
    from mrbo.ard import gp_fit_ard_batch, gp_fit_ard_multi
    from mrbo.surrogates import Surrogate
    keys = ("ll", "grad", "status", "L", "c") + (("s2",) if profile else ())
    surs = _surrogates("matern52", d, N, centre=profile)
    ells = _candidates("matern52", d)
    good = gp_fit_ard_multi(surs, ells, want_fit=True, profile=profile)
    assert (good["status"] == 0).all()
    bad = ells.copy()
    bad[0, 1, d - 1] = 0.0
    bad[2, 3, 0] = -1.0
    mixed = list(surs)
    if profile:
        mixed[1] = Surrogate(_kernel("matern52", [1.0]), surs[1].X[:, :N], np.zeros(N), capacity=N, σn2=SN2)
    r = gp_fit_ard_multi(mixed, bad, want_fit=True, profile=profile)
    expect = np.zeros((S, P), dtype=np.int32)
    expect[0, 1] = expect[2, 3] = 3
    if profile:
        expect[1, :] = 2
    assert (r["status"] == expect).all(), r["status"]
    fails = expect != 0
    assert np.isnan(r["ll"][fails]).all() and np.isnan(r["grad"][fails]).all()
    if profile:
        assert np.isnan(r["s2"][fails]).all()
    for q in range(S):
        for p in range(P):
            if not fails[q, p]:
                for k in keys[:3] + keys[5:]:
                    assert same_bits(r[k][q, p], good[k][q, p]), (q, p, k)
                assert same_bits(r["L"][q, :, :, p], good["L"][q, :, :, p]) and same_bits(r["c"][q, :, p], good["c"][q, :, p])
    for q in range(S):
        one = gp_fit_ard_batch(mixed[q], bad[q], want_fit=True, profile=profile)
        ok = ~fails[q]
        for k in keys[:3] + keys[5:]:
            assert np.array_equal(one[k], r[k][q], equal_nan=True), (q, k)
        assert same_bits(one["L"][:, :, ok], r["L"][q][:, :, ok]) and same_bits(one["c"][:, ok], r["c"][q][:, ok])
    for p in range(P):
        one = gp_fit_ard_batch(surs[0], ells[0, p:p + 1], want_fit=True, profile=profile)
        for k in keys[:3] + keys[5:]:
            assert same_bits(one[k][0], good[k][0, p]), (p, k)
        assert same_bits(one["L"][:, :, 0], good["L"][0, :, :, p]) and same_bits(one["c"][:, 0], good["c"][0, :, p])


@pytest.mark.parametrize("profile", [False, True], ids=["plain", "profile"])
def test_negative_noise_fails_every_slot(gpu, profile):
    """σn2 = −1 zeroes the diagonal (ψ(0) = 1): the first pivot is 0, status 1 and NaN everywhere."""
    from mrbo.ard import gp_fit_ard_multi
    surs = _surrogates("se", 2, 10, centre=profile)
    for s in surs:
        s.σn2 = -1.0
    r = gp_fit_ard_multi(surs, np.full((S, 2, 2), 0.5), profile=profile)
    assert (r["status"] == 1).all() and np.isnan(r["ll"]).all() and np.isnan(r["grad"]).all()
    if profile:
        assert np.isnan(r["s2"]).all()


# ---- the device refit ---------------------------------------------------------------------------------
def _refit_surrogates(d, N, centre):
    """Three problems of one shape: data set 0 depends on x₁ and weakly on x₂ only (its other
    lengthscales run to the bound), the others are tests/test_mle.py's isotropic data."""
    from mrbo.surrogates import Surrogate
    out = []
    for q in range(S):
        X, y = _data(d, N, seed=100 * d + q)
        if q == 0:
            y = np.sin(6.0 * X[0]) + 0.3 * X[1]
        out.append(Surrogate(_kernel("matern52", [1.0]), X, y - y.mean() if centre else y, capacity=N, σn2=SN2))
    return out


@pytest.mark.parametrize("profile", [False, True], ids=["plain", "profile"])
@pytest.mark.parametrize("d,N", [(2, 20), (6, 64)])
def test_device_refit_equals_lbfgs_scalar_on_the_fit_call(gpu, d, N, profile):
    from mrbo.ard import gp_fit_ard_batch, gp_optimize_ard_multi
    from mrbo.mle import lbfgs_scalar
    surs = _refit_surrogates(d, N, profile)
    lo, hi = [0.1] * d, [5.0] * d
    r = gp_optimize_ard_multi(surs, np.ones((S, d)), 0.1, 5.0, profile_amplitude=profile)
    assert r["ells"].shape == (S, d) and r["gradient"].shape == (S, d)
    its, on_bound = [], False
    for q, s in enumerate(surs):
        def fg(T):
            f = gp_fit_ard_batch(s, T, profile=profile)
            return np.where(f["status"] == 0, -f["ll"], np.nan), -f["grad"]
        x, f, g, it = lbfgs_scalar(fg, np.ones(d), lo, hi)
        print(q, "spec", x, f, g, it, "device", r["ells"][q], r["neg_log_likelihood"][q], r["gradient"][q],
              r["iterations"][q])
        assert same_bits(r["ells"][q], x) and same_bits(r["neg_log_likelihood"][q], np.float64(f)), q
        assert same_bits(r["gradient"][q], g) and r["iterations"][q] == it, q
        if profile:
            s2 = gp_fit_ard_batch(s, x[None], profile=True)["s2"][0]
            assert same_bits(r["s2"][q], s2), (q, r["s2"][q], s2)
        its.append(it)
        on_bound = on_bound or bool(((x == 0.1) | (x == 5.0)).any())
    assert r["stopped_at"] == 1 + max(its)
    # not vacuous: real line searches, problems frozen while others run, an active bound
    assert max(its) >= 3 and len(set(its)) > 1 and on_bound, (its, on_bound)


def test_optimize_ard_host_and_device_end_at_the_same_lengthscales(gpu):
    from mrbo.ard import ARDSurrogate, optimize_ard, optimize_ard_multi
    from mrbo.kernels import Matern52
    make = lambda std: [ARDSurrogate(Matern52(), s.X[:, :20], s.y[:20], capacity=20, standardize=std)
                        for s in _refit_surrogates(2, 20, False)]
    for std in (False, True):
        host, dev, alone = make(std), make(std), make(std)
        rh = optimize_ard_multi(host, 0.1, 5.0)
        rd = optimize_ard_multi(dev, 0.1, 5.0, device=True)
        for q in range(S):
            ra = optimize_ard(alone[q], 0.1, 5.0)
            assert same_bits(rh[q]["ells"], rd[q]["ells"]) and same_bits(rh[q]["ells"], ra["ells"]), (std, q)
            assert same_bits(host[q].ells, rh[q]["ells"]) and same_bits(dev[q].ells, host[q].ells)
            assert same_bits(host[q].inner.K, dev[q].inner.K)
            assert rh[q]["iterations"] == rd[q]["iterations"] >= 1
        assert any(len(set(h.ells)) > 1 for h in host)


# ---- evaluation in whitened coordinates ---------------------------------------------------------------
def test_whitened_evaluation_equals_the_isotropic_surrogate(gpu):
    """evaluate_base on ARDSurrogate(ells = (ℓ, ℓ)).inner at z = x/ℓ against the isotropic surrogate at ℓ and
    x: μ, σ and α equal and ∇_z α = ℓ·∇_x α, at the rtol of 1e-9 tests/test_gpu_parity.py holds evaluate to."""
    from mrbo import testfns
    from mrbo.ard import ARDSurrogate
    from mrbo.kernels import Matern52
    from mrbo.rollout import evaluate_base
    from mrbo.surrogates import Surrogate
    ell = 0.7
    fn = testfns.TestBraninHoo()
    lbs, ubs = fn.get_bounds()
    X = lbs[:, None] + (ubs - lbs)[:, None] * np.random.default_rng(20).random((2, 20))
    y = fn(X)
    iso = Surrogate(Matern52([ell]), X, y, capacity=20)
    ard = ARDSurrogate(Matern52(), X, y, ells=(ell, ell), capacity=20)
    xs = np.hstack([lbs[:, None] + (ubs - lbs)[:, None] * np.random.default_rng(21).random((2, 12)),
                    X[:, :4] + 0.05])                      # near observed points too: σ and α are not flat there
    a = evaluate_base(ard.inner, ard.whiten(xs), [0.0])
    b = evaluate_base(iso, xs, [0.0])
    moved = 0
    for ea, eb in zip(a, b):
        assert ea.μ == pytest.approx(eb.μ, rel=1e-9, abs=1e-9 * np.abs(y).max())
        assert ea.σ == pytest.approx(eb.σ, rel=1e-9, abs=1e-12)
        assert ea.αxθ == pytest.approx(eb.αxθ, rel=1e-9, abs=1e-12)
        scale = np.abs(eb.grad_αx).max()
        np.testing.assert_allclose(ea.grad_αx, ell * eb.grad_αx, rtol=1e-9, atol=1e-9 * ell * scale + 1e-300)
        moved += scale > 0.0
    assert moved >= 4                                      # the gradient identity is tested on non-zero gradients


# ---- the BO loops -----------------------------------------------------------------------------------------
RUN_KW = dict(horizon=1, budget=3, trials=2, mc_samples=16, batch_size=4, sgd_iterations=5, starts=4, rules=("ei",),
              optimize=True, ard=True, reuse_surrogate=False, log=lambda *_: None)
MYOPIC_KW = dict(budget=4, trials=2, starts=8, rules=("ei",), optimize=True, ard=True, reuse_surrogate=False,
                 log=lambda *_: None)


@pytest.fixture(scope="module")
def bo_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("ard_bo"))


@functools.lru_cache(maxsize=None)
def _run(tmp, lockstep, device_mle, device_solve):
    from mrbo import bayesopt
    return bayesopt.run("braninhoo", f"{tmp}/r{int(lockstep)}{int(device_mle)}{int(device_solve)}",
                        parallel_trials=2 if lockstep else 1, device_mle=device_mle, device_solve=device_solve, **RUN_KW)


@functools.lru_cache(maxsize=None)
def _myopic(tmp, lockstep, device_mle):
    from mrbo import bayesopt
    return bayesopt.run_myopic("braninhoo", f"{tmp}/m{int(lockstep)}{int(device_mle)}",
                               parallel_trials=2 if lockstep else 1, device_mle=device_mle, **MYOPIC_KW)


def _check_loop(ref, others, n_obs):
    from mrbo import bayesopt
    fn = bayesopt.TESTFNS["braninhoo"]()
    lbs, ubs = fn.get_bounds()
    assert len(ref) == 2
    for name, res in others.items():
        assert set(res) == set(ref)
        for key in ref:
            for k in ("X", "y", "ells"):
                assert same_bits(res[key][k], ref[key][k]), (name, key, k, res[key][k], ref[key][k])
    for r in ref.values():
        assert r["X"].shape == (2, n_obs) and same_bits(r["y"], fn(r["X"]))
        assert (r["X"] >= lbs[:, None]).all() and (r["X"] <= ubs[:, None]).all()
        assert ((r["ells"] >= 0.1) & (r["ells"] <= 5.0)).all()
    assert any(r["ells"][0] != r["ells"][1] for r in ref.values()), [r["ells"] for r in ref.values()]


def test_run_with_ard_agrees_across_its_paths(gpu, bo_dir):
    ref = _run(bo_dir, False, False, False)
    _check_loop(ref, {"lockstep": _run(bo_dir, True, False, False), "device_mle": _run(bo_dir, False, True, False),
                      "device_solve": _run(bo_dir, False, False, True)}, 5 + 3)


def test_run_myopic_with_ard_agrees_across_its_paths(gpu, bo_dir):
    ref = _myopic(bo_dir, False, False)
    _check_loop(ref, {"lockstep": _myopic(bo_dir, True, False), "device_mle": _myopic(bo_dir, False, True)}, 5 + 4)
