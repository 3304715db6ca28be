"""ARD lengthscales: one lengthscale per input dimension (build-defined, no reference counterpart;
DESIGN.md §18).

The four radial kernels (Matérn-5/2, -3/2, -1/2, SE) depend on x only through ρ = ‖(x − x′)/ℓ‖, so a GP
with θ = (ℓ_1 … ℓ_d) is the unit-lengthscale isotropic GP on the whitened coordinates z = x/ℓ
(componentwise):

    K_ik        = ψ(ρ_ik; ℓ = 1) + σn2·δ_ik,      ρ_ik = ‖z_i − z_k‖
    ∂K_ik/∂ℓ_u  = g(ρ_ik)·(x_iu − x_ku)²/ℓ_u³,   g(ρ) = −ψ′(ρ; 1)/ρ   (0 on the diagonal and where ρ_ik = 0)

What this module adds around that observation:
  ard_log_likelihood_host   the float64 numpy specification of the ARD likelihood (plain and profiled)
  gp_fit_ard_multi/_batch   the device fit (mrbo_gp_fit_ard_multi: S data sets × P candidates, one launch)
  gp_optimize_ard_multi     the device refit (mrbo_gp_optimize_ard_multi: mle.lbfgs_scalar on d variables)
  optimize_ard(_multi)      the refit of ARDSurrogates, host-driven or as the one device call
  ARDSurrogate              raw X, y and `ells` around `inner`, an ordinary Surrogate on Z = X/ells with
                            ψ at ℓ = 1: plans, evaluate_base, base_solve and the rollout run on `inner`
                            unchanged, in whitened coordinates.
Periodic has no such form and is refused.
"""
import ctypes
import math

import numpy as np

from . import _lib
from .kernels import MATERN12, MATERN32, MATERN52, PERIODIC, SE, RadialBasisFunction
from .mle import lbfgs_scalar_multi
from .surrogates import DEFAULT_CAPACITY, Surrogate

ARD_N_MAX, ARD_D_MAX = 128, 16       # the device fit's range (one workgroup's LDS)
_NAMES = {MATERN52: "Matern52", MATERN32: "Matern32", MATERN12: "Matern12", SE: "SquaredExponential"}


def _kind(kind):
    """A kernel id from an id or a RadialBasisFunction; Periodic and unknown ids are refused."""
    k = int(getattr(kind, "kind", kind))
    if k == PERIODIC:
        raise ValueError("ARD lengthscales: the Periodic kernel has no ARD form")
    if k not in _NAMES:
        raise ValueError(f"ARD lengthscales: kernel id {k}")
    return k


def unit_kernel(kind):
    """ψ of the family `kind` at ℓ = 1: the kernel of the whitened GP."""
    k = _kind(kind)
    return RadialBasisFunction(_NAMES[k], k, (1.0,))


def _g(kind, ρ):
    """g(ρ) = −ψ′(ρ; ℓ = 1)/ρ in closed form; 0 where ρ = 0 (δK vanishes there)."""
    ρ = np.asarray(ρ, dtype=np.float64)
    pos = ρ > 0.0
    r = np.where(pos, ρ, 1.0)
    if kind == MATERN52:
        s = np.sqrt(5.0) * r
        g = 5.0 / 3.0 * (1.0 + s) * np.exp(-s)
    elif kind == MATERN32:
        g = 3.0 * np.exp(-np.sqrt(3.0) * r)
    elif kind == MATERN12:
        g = np.exp(-r) / r
    else:
        g = np.exp(-0.5 * r * r)
    return np.where(pos, g, 0.0)


def ard_kernel_matrix(X, kind, ells, σn2):
    """K = ψ(‖(x_i − x_k)/ℓ‖; ℓ = 1) + σn2·I for the d×N points X."""
    Z = np.asarray(X, dtype=np.float64) / np.asarray(ells, dtype=np.float64).ravel()[:, None]
    D = Z[:, :, None] - Z[:, None, :]
    ρ = np.sqrt((D * D).sum(0))
    np.fill_diagonal(ρ, 0.0)
    return unit_kernel(kind)(ρ) + σn2 * np.eye(Z.shape[1])


def ard_log_likelihood_host(X, y, kind, ells, σn2, profile=False):
    """The ARD marginal likelihood in float64 numpy, the specification of the device fit.

    X d×N, y (N,) (the caller centres it for the profiled form), `kind` a kernel id or a
    RadialBasisFunction of the family, ells (d,).  profile=False: ll = −yᵀc/2 − Σ log L_ii − (N/2) log 2π and
    ∂ll/∂ℓ_u = (cᵀδK_u c − tr(K⁻¹δK_u))/2; profile=True: mle.profile_log_likelihood_host's ll_p and
    ∂ll_p/∂ℓ_u = (N/(2q))·cᵀδK_u c − tr(K⁻¹δK_u)/2 with q = yᵀc, ŝ² = q/N.  Returns dict(ll, grad (d,), s2
    (None in the plain form), L, c).  Raises LinAlgError when K is not positive definite and ValueError
    when some ℓ_u is not positive and finite or, in the profiled form, q is not positive and finite."""
    k = _kind(kind)
    X = np.asarray(X, dtype=np.float64)
    r = np.asarray(y, dtype=np.float64).ravel()
    ells = np.asarray(ells, dtype=np.float64).ravel()
    d, N = X.shape
    if ells.shape != (d,) or not (np.isfinite(ells) & (ells > 0.0)).all():
        raise ValueError(f"ARD lengthscales {ells}: {d} positive finite values")
    Z = X / ells[:, None]
    D = Z[:, :, None] - Z[:, None, :]
    D2 = D * D
    ρ = np.sqrt(D2.sum(0))
    np.fill_diagonal(ρ, 0.0)
    K = unit_kernel(k)(ρ) + σn2 * np.eye(N)
    L = np.linalg.cholesky(K)
    c = np.linalg.solve(L.T, np.linalg.solve(L, r))
    q = float(r @ c)
    Kinv = np.linalg.solve(L.T, np.linalg.solve(L, np.eye(N)))
    g = _g(k, ρ)
    np.fill_diagonal(g, 0.0)
    dK = g[None] * D2 / ells[:, None, None]                     # Δ_u²/ℓ_u³ = Δz_u²/ℓ_u
    cdc = np.array([c @ dK[u] @ c for u in range(d)])
    tr = np.array([np.sum(Kinv * dK[u]) for u in range(d)])
    logdet = float(np.log(np.diag(L)).sum())
    if profile:
        if not (q > 0.0 and math.isfinite(q)):
            raise ValueError("profiled likelihood: yᵀK⁻¹y is not positive and finite (constant data)")
        ll = -0.5 * N * math.log(q / N) - logdet - 0.5 * N * (1.0 + math.log(2.0 * math.pi))
        return dict(ll=ll, grad=N / (2.0 * q) * cdc - 0.5 * tr, s2=q / N, L=L, c=c)
    ll = -0.5 * q - logdet - 0.5 * N * math.log(2.0 * math.pi)
    return dict(ll=ll, grad=0.5 * (cdc - tr), s2=None, L=L, c=c)


# ---- the device fit ------------------------------------------------------------------------------
def _fit_data(s):
    """(raw X d×n, the targets of the fit (n,), kernel id, σn2, fmini) of an ARDSurrogate or a Surrogate.
    The targets are what the surrogate models: the standardised values where it standardises."""
    n = s.observed
    if isinstance(s, ARDSurrogate):
        return s.X[:, :n], s.inner.y[:n], s.kind, s.σn2, s.inner.fmini()
    return s.X[:, :n], s.y[:n], _kind(s.ψ), s.σn2, s.fmini()


def _descs(surs):
    """The SurrogateDesc array of one ARD call (and the arrays it points into): the surrogates share
    d, N, the kernel family and σn2; Periodic, N > 128 and d > 16 are left to the library's checks."""
    data = [_fit_data(s) for s in surs]
    d, n = data[0][0].shape
    for q, (X, _, k, sn2, _) in enumerate(data[1:], start=1):
        if X.shape != (d, n):
            raise ValueError(f"surrogate {q} has d = {X.shape[0]}, N = {X.shape[1]}; surrogate 0 has d = {d}, N = {n}")
        if k != data[0][2] or sn2 != data[0][3]:
            raise ValueError(f"surrogate {q} differs from surrogate 0 in its kernel family or σn2")
    dp = ctypes.POINTER(ctypes.c_double)
    keep = [(np.asfortranarray(X), np.ascontiguousarray(y)) for X, y, *_ in data]
    sds = (_lib.SurrogateDesc * len(surs))(*[
        _lib.SurrogateDesc(d, n, int(k), 1.0, float(sn2), float(fm), X.ctypes.data_as(dp), None, n, None,
                           y.ctypes.data_as(dp), 1.0)
        for (X, y), (_, _, k, sn2, fm) in zip(keep, data)])
    return sds, keep, d, n


def _vp(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def gp_fit_ard_multi(surs, ells, want_fit=False, profile=False):
    """The ARD fit of S surrogates at P lengthscale vectors each, in one launch (mrbo_gp_fit_ard_multi).

    `ells` is (S, P, d).  Returns dict(ll (S, P), grad (S, P, d), status (S, P)[, s2 (S, P) with
    profile=True][, L (S, N, N, P), c (S, N, P) with want_fit]); status 1 = a pivot is not positive,
    2 = profile mode and constant data, 3 = some ℓ_u is not positive and finite.  Block q carries the
    bits of the S = 1 call on surrogate q, candidate p those of a P = 1 call."""
    surs = list(surs)
    if len(surs) < 1:
        raise ValueError("a batched fit needs at least one surrogate")
    sds, keep, d, n = _descs(surs)
    S = len(surs)
    th = np.asarray(ells, dtype=np.float64)
    if th.ndim != 3 or th.shape[0] != S or th.shape[2] != d:
        raise ValueError(f"ells has shape {th.shape}: (S, P, d) = ({S}, P, {d})")
    th = np.ascontiguousarray(th)
    P = th.shape[1]
    L = _lib.load()
    ll, grad = np.zeros((S, P)), np.zeros((S, P, d))
    st = np.zeros((S, P), dtype=np.int32)
    s2 = np.zeros((S, P)) if profile else None
    Lo = np.zeros((S, P, n, n)) if want_fit else None      # N×N×P×S column-major
    co = np.zeros((S, P, n)) if want_fit else None
    _lib.check(L.mrbo_gp_fit_ard_multi(sds, S, P, _vp(th), _vp(ll), _vp(grad), _vp(s2), _vp(st), _vp(Lo), _vp(co),
                                       _lib.MRBO_FLAG_HOST_POINTERS, None))
    out = dict(ll=ll, grad=grad, status=st)
    if profile:
        out["s2"] = s2
    if want_fit:
        out["L"], out["c"] = Lo.transpose(0, 3, 2, 1), co.transpose(0, 2, 1)
    return out


def gp_fit_ard_batch(s, ells, want_fit=False, profile=False):
    """gp_fit_ard_multi's S = 1 form: `ells` (P, d); every entry of the dict loses its leading axis."""
    th = np.asarray(ells, dtype=np.float64)
    r = gp_fit_ard_multi([s], th.reshape((1,) + th.shape) if th.ndim == 2 else th, want_fit, profile)
    return {k: v[0] for k, v in r.items()}


def gp_optimize_ard_multi(surs, ell0=None, lowerbounds=None, upperbounds=None, iterations=30, history=10,
                          profile_amplitude=False):
    """The S ARD refits as ONE device-resident call (mrbo_gp_optimize_ard_multi): problem q starts at
    ell0[q] (default: the ARDSurrogates' current ells) and ends, bit for bit, where mle.lbfgs_scalar
    driven by gp_fit_ard_batch(surs[q], ·) ends.  The bounds are scalars or (d,).  The surrogates are left
    untouched.  Returns dict(ells (S, d), neg_log_likelihood (S,), gradient (S, d), iterations (S,),
    rounds, stopped_at[, s2 (S,) with profile_amplitude=True])."""
    surs = list(surs)
    if len(surs) < 1:
        raise ValueError("a batched refit needs at least one surrogate")
    if lowerbounds is None or upperbounds is None:
        raise ValueError("gp_optimize_ard_multi needs lowerbounds and upperbounds")
    if int(iterations) < 1 or not 1 <= int(history) <= 16:
        raise ValueError(f"iterations = {iterations}, history = {history}: at least 1, and 1..16")
    sds, keep, d, n = _descs(surs)
    S = len(surs)
    th0 = np.stack([s.ells for s in surs]) if ell0 is None else np.asarray(ell0, dtype=np.float64)
    if th0.shape != (S, d):
        raise ValueError(f"ell0 has shape {th0.shape}: (S, d) = ({S}, {d})")
    th0 = np.ascontiguousarray(th0, dtype=np.float64)
    lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lowerbounds, dtype=np.float64).ravel(), (d,)))
    hi = np.ascontiguousarray(np.broadcast_to(np.asarray(upperbounds, dtype=np.float64).ravel(), (d,)))
    L = _lib.load()
    opts = _lib.MleOpts(int(iterations), int(history), 0.0, 0.0)
    th, f, g = np.zeros((S, d)), np.zeros(S), np.zeros((S, d))
    its = np.zeros(S, dtype=np.int32)
    s2 = np.zeros(S) if profile_amplitude else None
    res = (ctypes.c_int32 * 2)()
    _lib.check(L.mrbo_gp_optimize_ard_multi(sds, S, _vp(th0), _vp(lo), _vp(hi), ctypes.byref(opts), _vp(th), _vp(f),
                                            _vp(g), _vp(s2), _vp(its), res, _lib.MRBO_FLAG_HOST_POINTERS, None))
    out = dict(ells=th, neg_log_likelihood=f, gradient=g, iterations=its, rounds=int(res[0]), stopped_at=int(res[1]))
    if profile_amplitude:
        out["s2"] = s2
    return out


def _bounds(d, lower, upper):
    lo = np.broadcast_to(np.asarray(lower, dtype=np.float64).ravel(), (d,)).copy()
    hi = np.broadcast_to(np.asarray(upper, dtype=np.float64).ravel(), (d,)).copy()
    return lo, hi


def optimize_ard(s, lower, upper, iterations=30, device=False):
    """Maximise the ARD likelihood of ARDSurrogate `s` over its d lengthscales within the box (scalars
    or (d,)), from s.ells, then s.set_lengthscales at the optimum.  The host-driven projected L-BFGS
    (mle.lbfgs_scalar's arithmetic) on the fit call, or with device=True the one device call, which ends
    at the same ells bit for bit.  A standardised surrogate fits the
    profiled-amplitude likelihood.  Returns dict(ells, neg_log_likelihood, gradient, iterations)."""
    return optimize_ard_multi([s], lower, upper, iterations, device)[0]


def optimize_ard_multi(surs, lower, upper, iterations=30, device=False):
    """optimize_ard for the surrogates of k lockstep trials: every round's evaluations are ONE
    gp_fit_ard_multi launch (mle.lbfgs_scalar_multi), or with device=True the whole minimisation is
    one gp_optimize_ard_multi call.  Every surrogate ends where optimize_ard alone leaves it."""
    surs = list(surs)
    std = [bool(s.standardize) for s in surs]
    if any(std) and not all(std):
        raise ValueError("optimize_ard_multi: standardised and plain surrogates in one batch")
    profile = std[0]
    d = surs[0].X.shape[0]
    lo, hi = _bounds(d, lower, upper)
    out = []
    if device:
        r = gp_optimize_ard_multi(surs, None, lo, hi, iterations, profile_amplitude=profile)
        for q, s in enumerate(surs):
            ells = r["ells"][q].copy()
            s.set_lengthscales(ells)
            out.append(dict(ells=ells, neg_log_likelihood=float(r["neg_log_likelihood"][q]),
                            gradient=r["gradient"][q].copy(), iterations=int(r["iterations"][q])))
        return out

    def fg_multi(idx, T):
        r = gp_fit_ard_multi([surs[i] for i in idx], T, profile=profile)
        return np.where(r["status"] == 0, -r["ll"], np.nan), -r["grad"]

    # the projected L-BFGS in lbfgs_scalar's arithmetic, the device minimiser's: with d > 1 variables
    # numpy's dot products (projected_lbfgs_multi) round differently and the two paths would part
    res = lbfgs_scalar_multi(fg_multi, [s.ells.copy() for s in surs], lo, hi, iterations)
    for s, (ells, f, g, it) in zip(surs, res):
        s.set_lengthscales(ells)
        out.append(dict(ells=np.array(ells), neg_log_likelihood=f, gradient=g, iterations=it))
    return out


# ---- the surrogate -------------------------------------------------------------------------------
class ARDSurrogate:
    """A GP surrogate with one lengthscale per input dimension.

    Keeps the raw covariates `X` (d×capacity, zero padded), the vector `ells` (default: ψ's ℓ in every
    dimension) and `inner`, an ordinary Surrogate on Z = X/ells with ψ's family at ℓ = 1 that holds the
    observations (standardised with standardize=True), K, L and c.  Everything that evaluates the model
    on the device -- plans, evaluate_base, base_solve, the rollout -- takes `inner` and works in whitened
    coordinates: whiten(x) = x/ells, unwhiten(z) = z·ells, whitened_box(lbs, ubs) the image of a box.
    posterior(x) takes raw x and returns raw units.  A standardised ARD surrogate always refits the
    profiled likelihood (optimize_ard), like Surrogate(standardize=True)."""

    def __init__(self, ψ, X, y, ells=None, capacity=DEFAULT_CAPACITY, decision_rule=None, σn2=1e-6, standardize=False):
        X = np.asarray(X, dtype=np.float64)
        d, N = X.shape
        self.kind = _kind(ψ)
        self.ells = (np.full(d, float(ψ.lengthscale)) if ells is None
                     else np.array(ells, dtype=np.float64).ravel())
        self._check_ells(self.ells, d)
        self.capacity = int(capacity)
        self.X = np.zeros((d, self.capacity))
        self.X[:, :N] = X
        self.inner = Surrogate(unit_kernel(self.kind), X / self.ells[:, None], y, capacity=capacity,
                               decision_rule=decision_rule, σn2=σn2, standardize=standardize)

    @staticmethod
    def _check_ells(ells, d):
        if ells.shape != (d,) or not (np.isfinite(ells) & (ells > 0.0)).all():
            raise ValueError(f"ARD lengthscales {ells}: {d} positive finite values")

    # what the loops read off a surrogate
    observed = property(lambda self: self.inner.observed)
    version = property(lambda self: self.inner.version)
    σn2 = property(lambda self: self.inner.σn2)
    standardize = property(lambda self: self.inner.standardize)
    ψ = property(lambda self: self.inner.ψ)

    @property
    def fmini_over_capacity(self):
        return self.inner.fmini_over_capacity

    @fmini_over_capacity.setter
    def fmini_over_capacity(self, v):
        self.inner.fmini_over_capacity = v

    def get_active_covariates(self):
        """The raw covariates (d×observed)."""
        return self.X[:, : self.observed]

    def get_active_observations(self):
        """The observations as given (raw units)."""
        return self.inner.get_active_observations()

    def get_decision_rule(self):
        return self.inner.get_decision_rule()

    def set_decision_rule(self, g):
        self.inner.set_decision_rule(g)

    # coordinates
    def whiten(self, x):
        x = np.asarray(x, dtype=np.float64)
        return x / (self.ells if x.ndim == 1 else self.ells.reshape((-1,) + (1,) * (x.ndim - 1)))

    def unwhiten(self, z):
        z = np.asarray(z, dtype=np.float64)
        return z * (self.ells if z.ndim == 1 else self.ells.reshape((-1,) + (1,) * (z.ndim - 1)))

    def whitened_box(self, lbs, ubs):
        return self.whiten(np.asarray(lbs, dtype=np.float64)), self.whiten(np.asarray(ubs, dtype=np.float64))

    # maintenance
    def reset(self, X, y):
        """Refit on (X, y) with the current ells (Surrogate.reset on the whitened points)."""
        X = np.asarray(X, dtype=np.float64)
        self.X[:, : X.shape[1]] = X
        self.inner.reset(X / self.ells[:, None], y)

    def set_lengthscales(self, ells):
        """New lengthscales: `inner` is refit on Z = X/ells with the observations it holds."""
        ells = np.array(ells, dtype=np.float64).ravel()
        self._check_ells(ells, self.X.shape[0])
        self.ells = ells
        n = self.observed
        self.inner.reset(self.X[:, :n] / ells[:, None], self.inner.get_active_observations().copy())

    def condition(self, xnew, ynew):
        """condition! at the raw point xnew.  Past capacity it follows Surrogate.condition: the
        observation reaches only the returned, resized copy."""
        x = np.asarray(xnew, dtype=np.float64).ravel()
        n = self.observed
        if n == self.capacity:
            big = ARDSurrogate(self.ψ, self.X, self.get_active_observations().copy(), ells=self.ells,
                               capacity=2 * self.capacity, decision_rule=self.get_decision_rule(), σn2=self.σn2,
                               standardize=self.standardize)
            return big.condition(x, ynew)
        self.X[:, n] = x
        self.inner.condition(x / self.ells, ynew)
        return self

    def posterior(self, x):
        """Posterior mean and standard deviation of the objective at raw x (d,) or (d, n), raw units."""
        return self.inner.posterior(self.whiten(x))
