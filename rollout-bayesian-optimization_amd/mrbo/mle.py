"""Between-step surrogate maintenance: marginal likelihood and its maximisation.

Mirrors radial_basis_surrogates.jl:
  log_likelihood(s)       :770-776
  ∇log_likelihood(s)      :787-799 (δlog_likelihood :778-785, eval_Dθ_KXX radial_basis_functions.jl:264-284)
  optimize!(s; lowerbounds, upperbounds, optim_options=Optim.Options(iterations=30))  :805-829
The likelihood and its lengthscale derivative are evaluated on the GPU (mrbo_gp_fit: one
workgroup per candidate lengthscale, refit K → L → c on device).  The outer minimiser of
−log_likelihood is build-defined: the reference's Fminbox(LBFGS()) lives in Optim.jl, absent
and unpinned here, so `optimize` runs a deterministic projected L-BFGS with a batched
backtracking line search (all trial step lengths evaluated in one launch); both reach the
box-constrained stationary point of the same objective from the same start.
The refits of k lockstep BO trials run together (no reference counterpart): gp_fit_multi is one
launch for S surrogates × P candidates (mrbo_gp_fit_multi), projected_lbfgs_multi advances the S
minimisations in lockstep through the same per-problem code, optimize_multi is optimize for a list.
gp_optimize_multi runs those S minimisations as one device-resident call (mrbo_gp_optimize_multi:
no host round trip per line search); lbfgs_scalar is the specification its step kernel is held to.
The profiled-amplitude likelihood (build-defined, opt-in: profile=True / profile_amplitude=True)
models the data as s·g, g ~ GP(0, ψ_θ) + σn2, with s² at its closed-form maximiser; the same
kernels evaluate it (mrbo_gp_fit_profile_multi), profile_log_likelihood_host is its specification.
"""
import ctypes
import math

import numpy as np

from . import _lib

# the trial step lengths of one line search, evaluated together
_STEPS = 0.5 ** np.arange(12)


def _nt(s):
    """Hyperparameters of the kernel: (ℓ), or (ℓ, p) for Periodic (radial_basis_functions.jl:98-103)."""
    return len(s.ψ.θ)


def _dpsi_dtheta(ψ, ρ):
    """∂ψ/∂θ_t(ρ) in closed form (eval_Dθ_KXX's entries, radial_basis_functions.jl:264-284 by
    ForwardDiff there): (nt, ...) -- ∂/∂ℓ, and ∂/∂p for Periodic."""
    from .kernels import MATERN12, MATERN32, MATERN52, PERIODIC
    l = ψ.lengthscale
    if ψ.kind == PERIODIC:
        p = ψ.period
        u = np.pi * ρ / p
        su = np.sin(u)
        v = ψ(ρ)
        return np.stack([v * 4.0 * su * su / l ** 3, v * 2.0 * u * np.sin(2.0 * u) / (l * l * p)])
    if ψ.kind == MATERN52:
        s = np.sqrt(5.0) * ρ / l
        return (s * s / 3.0 * (1.0 + s) * np.exp(-s) / l)[None]
    if ψ.kind == MATERN32:
        s = np.sqrt(3.0) * ρ / l
        return (s * s * np.exp(-s) / l)[None]
    if ψ.kind == MATERN12:
        s = ρ / l
        return (s * np.exp(-s) / l)[None]
    return (ψ(ρ) * ρ * ρ / l ** 3)[None]


def profile_log_likelihood_host(X, y, ψ, σn2):
    """The profiled-amplitude likelihood in float64 numpy, the specification of the device's profile
    mode: the data r = y (d×N X, the caller centres y) are r = s·g with g ~ GP(0, ψ) + σn2 noise and
    the amplitude at its closed-form maximiser ŝ² = q/N, q = rᵀK⁻¹r, K = Ψ + σn2·I:
        ll_p       = −(N/2)·log(q/N) − Σ log L_ii − (N/2)(1 + log 2π)
        ∂ll_p/∂θ_t = (N/(2q))·(cᵀ δK_t c) − tr(K⁻¹ δK_t)/2,   c = K⁻¹r.
    Returns dict(ll, grad (nt,), s2, L, c).  Raises LinAlgError when K is not positive definite and
    ValueError when q is not positive and finite (constant data)."""
    X = np.asarray(X, dtype=np.float64)
    r = np.asarray(y, dtype=np.float64).ravel()
    N = r.size
    D = X[:, :, None] - X[:, None, :]
    ρ = np.sqrt((D * D).sum(0))
    np.fill_diagonal(ρ, 0.0)
    K = ψ(ρ) + σn2 * np.eye(N)
    L = np.linalg.cholesky(K)
    c = np.linalg.solve(L.T, np.linalg.solve(L, r))
    q = float(r @ c)
    if not (q > 0.0 and math.isfinite(q)):
        raise ValueError("profiled likelihood: rᵀK⁻¹r is not positive and finite (constant data)")
    Kinv = np.linalg.solve(L.T, np.linalg.solve(L, np.eye(N)))
    dK = _dpsi_dtheta(ψ, ρ)
    for t in range(dK.shape[0]):
        np.fill_diagonal(dK[t], 0.0)
    grad = np.array([N / (2.0 * q) * (c @ dK[t] @ c) - 0.5 * np.sum(Kinv * dK[t]) for t in range(dK.shape[0])])
    ll = -0.5 * N * math.log(q / N) - float(np.log(np.diag(L)).sum()) - 0.5 * N * (1.0 + math.log(2.0 * math.pi))
    return dict(ll=ll, grad=grad, s2=q / N, L=L, c=c)


def gp_fit_batch(s, thetas, want_fit=False, profile=False):
    """Refit the base GP of `s` at each hyperparameter vector on the device (mrbo_gp_fit_theta).

    `thetas` is (P,) -- lengthscales -- or (P, nt) with nt = len(s.ψ.θ).  Returns dict(ll, grad
    (P, nt), dll (= grad[:, 0]), status[, L (N×N×P), c (N×P)]); status 1 = PosDefException.
    profile=True: the profiled-amplitude likelihood (gp_fit_multi's, S = 1), with s2 (P,) added."""
    if profile:
        r = gp_fit_multi([s], np.asarray(thetas, dtype=np.float64)[None], want_fit, profile=True)
        out = {k: v[0] for k, v in r.items()}
        out["dll"] = out["dll"].copy()
        return out
    L = _lib.load()
    th = np.asarray(thetas, dtype=np.float64)
    th = np.ascontiguousarray(th.reshape(th.shape[0], -1) if th.ndim > 1 else th.reshape(-1, 1))
    P, nt = th.shape
    n = s.observed
    X = np.asfortranarray(s.X[:, :n])
    y = np.ascontiguousarray(s.y[:n])
    dp = ctypes.POINTER(ctypes.c_double)
    sd = _lib.SurrogateDesc(X.shape[0], n, int(s.ψ.kind), float(s.ψ.lengthscale), float(s.σn2), float(s.fmini()),
                            X.ctypes.data_as(dp), None, n, None, y.ctypes.data_as(dp), float(s.ψ.period))
    ll, grad = np.zeros(P), np.zeros((P, nt))
    st = np.zeros(P, dtype=np.int32)
    Lo = np.zeros((n, n, P), order="F") if want_fit else None
    co = np.zeros((n, P), order="F") if want_fit else None
    vp = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None
    _lib.check(L.mrbo_gp_fit_theta(ctypes.byref(sd), P, nt, vp(th), vp(ll), vp(grad), vp(st), vp(Lo), vp(co),
                                   _lib.MRBO_FLAG_HOST_POINTERS, None))
    out = dict(ll=ll, grad=grad, dll=grad[:, 0].copy(), status=st)
    if want_fit:
        out["L"], out["c"] = Lo, co
    return out


def check_fit_batch(surs):
    """The surrogates of one mrbo_gp_fit_multi call share d, N, the kernel family and σn2.  Raises a
    ValueError naming the first that differs from surrogate 0; returns (d, N, nt)."""
    if len(surs) < 1:
        raise ValueError("a batched refit needs at least one surrogate")
    s0 = surs[0]
    d, N = s0.X.shape[0], s0.observed
    for q, s in enumerate(surs[1:], start=1):
        if s.X.shape[0] != d or s.observed != N:
            raise ValueError(f"surrogate {q} has d = {s.X.shape[0]}, N = {s.observed}; surrogate 0 has d = {d}, N = {N}")
        if s.ψ.kind != s0.ψ.kind or s.σn2 != s0.σn2:
            raise ValueError(f"surrogate {q} differs from surrogate 0 in its kernel family or σn2")
    return d, N, _nt(s0)


def gp_fit_multi(surs, thetas, want_fit=False, profile=False):
    """gp_fit_batch for S surrogates with P hyperparameter vectors each, in one launch
    (mrbo_gp_fit_multi): block q is bit-identical to gp_fit_batch(surs[q], thetas[q]).
    profile=True evaluates the profiled-amplitude likelihood instead (mrbo_gp_fit_profile_multi:
    ll and grad are ll_p and ∂ll_p of profile_log_likelihood_host, s2 (S, P) is added to the dict,
    status 2 marks constant data; L and c are the plain call's).

    `thetas` is (S, P) -- lengthscales -- or (S, P, nt).  The surrogates share d, N, the kernel
    family and σn2 (ValueError otherwise).  Returns dict(ll (S, P), grad (S, P, nt), dll
    (= grad[:, :, 0]), status (S, P)[, L (S, N, N, P), c (S, N, P)])."""
    surs = list(surs)
    d, n, _ = check_fit_batch(surs)
    S = len(surs)
    th = np.asarray(thetas, dtype=np.float64)
    if th.ndim < 2 or th.shape[0] != S:
        raise ValueError(f"thetas has shape {th.shape}: (S, P) or (S, P, nt) with S = {S}")
    th = np.ascontiguousarray(th.reshape(S, th.shape[1], -1))
    P, nt = th.shape[1:]
    L = _lib.load()
    dp = ctypes.POINTER(ctypes.c_double)
    keep = [(np.asfortranarray(s.X[:, :n]), np.ascontiguousarray(s.y[:n])) for s in surs]
    sds = (_lib.SurrogateDesc * S)(*[
        _lib.SurrogateDesc(d, n, int(s.ψ.kind), float(s.ψ.lengthscale), float(s.σn2), float(s.fmini()),
                           X.ctypes.data_as(dp), None, n, None, y.ctypes.data_as(dp), float(s.ψ.period))
        for s, (X, y) in zip(surs, keep)])
    ll, grad = np.zeros((S, P)), np.zeros((S, P, nt))
    st = np.zeros((S, P), dtype=np.int32)
    Lo = np.zeros((S, P, n, n)) if want_fit else None      # N×N×P×S column-major
    co = np.zeros((S, P, n)) if want_fit else None
    vp = lambda a: ctypes.c_void_p(a.ctypes.data) if a is not None else None
    if profile:
        s2 = np.zeros((S, P))
        _lib.check(L.mrbo_gp_fit_profile_multi(sds, S, P, nt, vp(th), vp(ll), vp(grad), vp(s2), vp(st), vp(Lo), vp(co),
                                               _lib.MRBO_FLAG_HOST_POINTERS, None))
    else:
        _lib.check(L.mrbo_gp_fit_multi(sds, S, P, nt, vp(th), vp(ll), vp(grad), vp(st), vp(Lo), vp(co),
                                       _lib.MRBO_FLAG_HOST_POINTERS, None))
    out = dict(ll=ll, grad=grad, dll=grad[:, :, 0].copy(), status=st)
    if profile:
        out["s2"] = s2
    if want_fit:
        out["L"], out["c"] = Lo.transpose(0, 3, 2, 1), co.transpose(0, 2, 1)
    return out


def log_likelihood(s):
    """log_likelihood(s) at the surrogate's current hyperparameters (radial_basis_surrogates.jl:770-776)."""
    r = gp_fit_batch(s, s.ψ.θ[None, :])
    if r["status"][0]:
        raise np.linalg.LinAlgError("PosDefException (cholesky of K)")
    return float(r["ll"][0])


def grad_log_likelihood(s):
    """∇log_likelihood(s) (radial_basis_surrogates.jl:787-799): ∂/∂θ_t for every kernel hyperparameter."""
    r = gp_fit_batch(s, s.ψ.θ[None, :])
    if r["status"][0]:
        raise np.linalg.LinAlgError("PosDefException (cholesky of K)")
    return r["grad"][0].copy()


def _lbfgs_problem(x0, lo, hi, iterations, g_tol, m, c1):
    """One box-constrained minimisation as a coroutine: it yields the (P, n) points it needs
    evaluated, is sent (f (P,), g (P, n)) for them, and returns (x, f, g, iterations).  The first
    request is the start (P = 1), every later one a line search (P = len(_STEPS)).  Both
    projected_lbfgs and projected_lbfgs_multi drive this one implementation."""
    x = np.clip(np.asarray(x0, float), lo, hi)
    f, g = yield x[None]
    f, g = float(f[0]), g[0]
    S, Y = [], []
    it = 0
    for it in range(1, iterations + 1):
        free = ~(((x <= lo) & (g > 0)) | ((x >= hi) & (g < 0)))
        if not free.any() or np.max(np.abs(g[free])) <= g_tol:
            it -= 1
            break
        # two-loop recursion on the free variables
        q = np.where(free, g, 0.0)
        al = []
        for s_, y_ in reversed(list(zip(S, Y))):
            a = (s_ @ q) / (y_ @ s_)
            al.append(a)
            q = q - a * y_
        if S:
            q = q * ((S[-1] @ Y[-1]) / (Y[-1] @ Y[-1]))
        else:
            q = q / max(np.max(np.abs(q)), 1.0)     # first step: at most unit length
        for (s_, y_), a in zip(zip(S, Y), reversed(al)):
            b = (y_ @ q) / (y_ @ s_)
            q = q + (a - b) * s_
        p = -np.where(free, q, 0.0)
        if g @ p >= 0:                                # not a descent direction: steepest descent
            p = -np.where(free, g, 0.0)
        trial = np.clip(x[None] + _STEPS[:, None] * p[None], lo, hi)
        ft, gt = yield trial
        ok = np.isfinite(ft) & (ft <= f + c1 * ((trial - x[None]) @ g))
        if not ok.any():
            break
        k = int(np.argmax(ok))
        xn, fn, gn = trial[k], float(ft[k]), gt[k]
        sk, yk = xn - x, gn - g
        if sk @ yk > 1e-12 * max(np.linalg.norm(sk) * np.linalg.norm(yk), 1e-300):
            S.append(sk)
            Y.append(yk)
            if len(S) > m:
                S.pop(0)
                Y.pop(0)
        moved = np.max(np.abs(sk))
        x, f, g = xn, fn, gn
        if moved == 0.0:
            break
    return x, f, g, it


def projected_lbfgs(fg_batch, x0, lower, upper, iterations=30, g_tol=1e-8, m=10, c1=1e-4):
    """Minimise f over the box [lower, upper] from x0.

    fg_batch(X) takes a (P, n) array of points and returns (f (P,), g (P, n)); a point where f
    cannot be evaluated returns f = NaN.  Each iteration: L-BFGS direction on the free
    variables (bounds active with an outward gradient are fixed), then the first step length
    of 1, 1/2, ..., 1/2048 along the projected path meeting the Armijo condition -- all
    lengths evaluated in one batch.  Returns (x, f, g, iterations)."""
    lo, hi = np.asarray(lower, float), np.asarray(upper, float)
    prob = _lbfgs_problem(x0, lo, hi, iterations, g_tol, m, c1)
    pts = next(prob)
    try:
        while True:
            pts = prob.send(fg_batch(pts))
    except StopIteration as done:
        return done.value


def projected_lbfgs_multi(fg_multi, x0s, lower, upper, iterations=30, g_tol=1e-8, m=10, c1=1e-4):
    """projected_lbfgs for one independent minimisation per row of x0s, in lockstep: every round
    evaluates the pending points of all problems still running in ONE call.

    fg_multi(idx, X) takes the indices of the running problems and their points X (len(idx), P, n)
    -- the same P for all of them: 1 for the starts, then one line search each -- and returns
    (f (len(idx), P), g (len(idx), P, n)).  A problem that stops (converged, no Armijo step, zero
    move, budget spent) drops out of idx; the loop ends when idx is empty.  Each problem goes
    through projected_lbfgs's own arithmetic (_lbfgs_problem), so its result is the one
    projected_lbfgs gives it alone.  Returns a list of (x, f, g, iterations)."""
    lo, hi = np.asarray(lower, float), np.asarray(upper, float)
    probs = [_lbfgs_problem(x0, lo, hi, iterations, g_tol, m, c1) for x0 in x0s]
    out = [None] * len(probs)
    pending = {i: next(prob) for i, prob in enumerate(probs)}
    while pending:
        idx = sorted(pending)
        f, g = fg_multi(np.asarray(idx, dtype=np.intp), np.stack([pending[i] for i in idx]))
        for k, i in enumerate(idx):
            try:
                pending[i] = probs[i].send((f[k], g[k]))
            except StopIteration as done:
                out[i] = done.value
                del pending[i]
    return out


def _lbfgs_scalar_problem(x0, lower, upper, iterations, g_tol, m, c1):
    """lbfgs_scalar as a coroutine with _lbfgs_problem's protocol: it yields the (P, n) points it needs
    evaluated, is sent (f (P,), g (P, n)) for them, and returns (x, f, g, iterations).  lbfgs_scalar and
    lbfgs_scalar_multi drive this one implementation."""
    lo = [float(v) for v in np.asarray(lower, float).ravel()]
    hi = [float(v) for v in np.asarray(upper, float).ravel()]
    n = len(lo)
    R = range(n)

    def clip(v, i):
        if v < lo[i]:
            v = lo[i]
        if v > hi[i]:
            v = hi[i]
        return v

    def dot(a, b):
        r = a[0] * b[0]
        for i in range(1, n):
            r = r + a[i] * b[i]
        return r

    def absmax(a):          # np.max(np.abs(a)): a NaN stays
        r = abs(a[0])
        for i in range(1, n):
            v = abs(a[i])
            if v > r or v != v:
                r = v
        return r

    def points(pts):
        return np.array(pts, dtype=np.float64).reshape(len(pts), n)

    def values(fg, npts):
        f, g = fg
        return [float(v) for v in f], [[float(v) for v in row] for row in np.asarray(g).reshape(npts, n)]

    x = [clip(float(v), i) for i, v in enumerate(np.asarray(x0, float).ravel())]
    ft, gt = values((yield points([x])), 1)
    f, g = ft[0], gt[0]
    S, Y = [], []
    it = 0
    while it < iterations:
        it += 1
        free = [not ((x[i] <= lo[i] and g[i] > 0) or (x[i] >= hi[i] and g[i] < 0)) for i in R]
        if not any(free) or all(abs(g[i]) <= g_tol for i in R if free[i]):
            it -= 1
            break
        # two-loop recursion on the free variables
        q = [g[i] if free[i] else 0.0 for i in R]
        al = [0.0] * len(S)
        for j in reversed(range(len(S))):
            a = dot(S[j], q) / dot(Y[j], S[j])
            al[j] = a
            q = [q[i] - a * Y[j][i] for i in R]
        if S:
            sc = dot(S[-1], Y[-1]) / dot(Y[-1], Y[-1])
            q = [q[i] * sc for i in R]
        else:
            mx = absmax(q)                        # first step: at most unit length
            if 1.0 > mx:
                mx = 1.0
            q = [q[i] / mx for i in R]
        for j in range(len(S)):
            b = dot(Y[j], q) / dot(Y[j], S[j])
            q = [q[i] + (al[j] - b) * S[j][i] for i in R]
        p = [-(q[i] if free[i] else 0.0) for i in R]
        if dot(g, p) >= 0:                        # not a descent direction: steepest descent
            p = [-(g[i] if free[i] else 0.0) for i in R]
        trial = [[clip(x[i] + float(st) * p[i], i) for i in R] for st in _STEPS]
        ft, gt = values((yield points(trial)), len(trial))
        k = -1
        for kk in range(len(trial)):
            d = [trial[kk][i] - x[i] for i in R]
            if math.isfinite(ft[kk]) and ft[kk] <= f + c1 * dot(d, g):
                k = kk
                break
        if k < 0:
            break
        xn, fn, gn = trial[k], ft[k], gt[k]
        sk = [xn[i] - x[i] for i in R]
        yk = [gn[i] - g[i] for i in R]
        thr = math.sqrt(dot(sk, sk)) * math.sqrt(dot(yk, yk))
        if 1e-300 > thr:
            thr = 1e-300
        if dot(sk, yk) > 1e-12 * thr:
            S.append(sk)
            Y.append(yk)
            if len(S) > m:
                S.pop(0)
                Y.pop(0)
        moved = absmax(sk)
        x, f, g = xn, fn, gn
        if moved == 0.0:
            break
    return np.array(x), f, np.array(g), it


def lbfgs_scalar(fg_batch, x0, lower, upper, iterations=30, g_tol=1e-8, m=10, c1=1e-4):
    """projected_lbfgs restated on Python floats: every operation of _lbfgs_problem written out
    one rounding at a time -- a dot product is a0*b0 + a1*b1 + ... left to right, a norm the square
    root of that, nothing fused.  This is the specification of the device minimiser
    (mrbo_gp_optimize_multi's step kernel, csrc/mrbo_mle.hip, performs these operations in this
    order in fp64), so the two agree bit for bit on the same evaluations.  For one variable it
    equals projected_lbfgs exactly (a dot product is one multiplication); for more, numpy's `@` may
    fuse its multiply-adds and the two can differ in the last bits.  Returns (x, f, g, iterations)
    with x and g as arrays."""
    prob = _lbfgs_scalar_problem(x0, lower, upper, iterations, g_tol, m, c1)
    pts = next(prob)
    try:
        while True:
            pts = prob.send(fg_batch(pts))
    except StopIteration as done:
        return done.value


def lbfgs_scalar_multi(fg_multi, x0s, lower, upper, iterations=30, g_tol=1e-8, m=10, c1=1e-4):
    """lbfgs_scalar for one independent minimisation per row of x0s, in lockstep, with
    projected_lbfgs_multi's protocol: fg_multi(idx, X) evaluates the pending points X (len(idx), P, n) of
    the problems still running in ONE call.  Each problem goes through lbfgs_scalar's own arithmetic, so
    its result is the one lbfgs_scalar -- and the device minimiser -- gives it alone.  Returns a list of
    (x, f, g, iterations)."""
    probs = [_lbfgs_scalar_problem(x0, lower, upper, iterations, g_tol, m, c1) for x0 in x0s]
    out = [None] * len(probs)
    pending = {i: next(prob) for i, prob in enumerate(probs)}
    while pending:
        idx = sorted(pending)
        f, g = fg_multi(np.asarray(idx, dtype=np.intp), np.stack([pending[i] for i in idx]))
        for k_, i in enumerate(idx):
            try:
                pending[i] = probs[i].send((f[k_], g[k_]))
            except StopIteration as done:
                out[i] = done.value
                del pending[i]
    return out


def gp_optimize_multi(surs, theta0=None, lowerbounds=None, upperbounds=None, iterations=30, history=10,
                      profile_amplitude=False):
    """The S minimisations of optimize_multi as ONE device-resident call (mrbo_gp_optimize_multi):
    the data sets are staged once, and every line-search round -- one fit launch of grid (12, S) and
    one step kernel -- follows the last on the stream without a host round trip.  Problem q starts
    at theta0[q] (default: the surrogates' current θ) and ends, bit for bit, where lbfgs_scalar
    driven by gp_fit_batch(surs[q], ·) ends.  The surrogates are left untouched.  A Periodic
    kernel with theta0 of shape (S, 1) is minimised over ℓ alone, every data set at its own period.

    Returns dict(theta (S, nt), neg_log_likelihood (S,), gradient (S, nt), iterations (S,), rounds
    -- fit launches made, the start's included --, stopped_at -- the round after which no problem
    ran, 1 + max(iterations)).  profile_amplitude=True minimises −ll_p, the profiled-amplitude
    likelihood (mrbo_gp_optimize_profile_multi; its specification is lbfgs_scalar driven by
    gp_fit_batch(·, profile=True)), and adds s2 (S,): the amplitude ŝ² at theta."""
    surs = list(surs)
    d, n, nt = check_fit_batch(surs)
    if lowerbounds is None or upperbounds is None:
        raise ValueError("gp_optimize_multi needs lowerbounds and upperbounds")
    if int(iterations) < 1 or not 1 <= int(history) <= 16:
        raise ValueError(f"iterations = {iterations}, history = {history}: at least 1, and 1..16")
    S = len(surs)
    th0 = np.stack([s.ψ.θ for s in surs]) if theta0 is None else np.asarray(theta0, dtype=np.float64)
    if th0.shape[:1] == (S,) and th0.ndim <= 2 and th0.size == S and nt == 2:
        nt = 1          # Periodic over ℓ alone: every data set keeps its own period
    if th0.shape not in ((S, nt), (S,) if nt == 1 else None):
        raise ValueError(f"theta0 has shape {th0.shape}: (S, nt) = ({S}, {nt})")
    th0 = np.ascontiguousarray(th0.reshape(S, nt), dtype=np.float64)
    lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lowerbounds, dtype=np.float64).ravel(), (nt,)))
    hi = np.ascontiguousarray(np.broadcast_to(np.asarray(upperbounds, dtype=np.float64).ravel(), (nt,)))
    L = _lib.load()
    dp = ctypes.POINTER(ctypes.c_double)
    keep = [(np.asfortranarray(s.X[:, :n]), np.ascontiguousarray(s.y[:n])) for s in surs]
    sds = (_lib.SurrogateDesc * S)(*[
        _lib.SurrogateDesc(d, n, int(s.ψ.kind), float(s.ψ.lengthscale), float(s.σn2), float(s.fmini()),
                           X.ctypes.data_as(dp), None, n, None, y.ctypes.data_as(dp), float(s.ψ.period))
        for s, (X, y) in zip(surs, keep)])
    opts = _lib.MleOpts(int(iterations), int(history), 0.0, 0.0)
    th, f, g = np.zeros((S, nt)), np.zeros(S), np.zeros((S, nt))
    its = np.zeros(S, dtype=np.int32)
    res = (ctypes.c_int32 * 2)()
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    if profile_amplitude:
        s2 = np.zeros(S)
        _lib.check(L.mrbo_gp_optimize_profile_multi(sds, S, nt, vp(th0), vp(lo), vp(hi), ctypes.byref(opts), vp(th),
                                                    vp(f), vp(g), vp(s2), vp(its), res,
                                                    _lib.MRBO_FLAG_HOST_POINTERS, None))
    else:
        _lib.check(L.mrbo_gp_optimize_multi(sds, S, nt, vp(th0), vp(lo), vp(hi), ctypes.byref(opts), vp(th), vp(f),
                                            vp(g), vp(its), res, _lib.MRBO_FLAG_HOST_POINTERS, None))
    out = dict(theta=th, neg_log_likelihood=f, gradient=g, iterations=its, rounds=int(res[0]),
               stopped_at=int(res[1]))
    if profile_amplitude:
        out["s2"] = s2
    return out


def optimize(s, lowerbounds, upperbounds, iterations=30, device=False, profile_amplitude=False):
    """optimize!(s; lowerbounds, upperbounds) (radial_basis_surrogates.jl:805-829): maximise the
    log likelihood over the kernel hyperparameters (ℓ; Periodic ℓ and p) within the box, then
    set_kernel! at the optimum.  device=True runs the minimisation as one device-resident call
    (gp_optimize_multi with S = 1).  profile_amplitude=True maximises the profiled-amplitude
    likelihood instead (on either path); a standardised surrogate (Surrogate(standardize=True))
    always does, its amplitude being part of the fit."""
    profile_amplitude = bool(profile_amplitude) or bool(getattr(s, "standardize", False))
    if device:
        return optimize_multi([s], lowerbounds, upperbounds, iterations, device=True,
                              profile_amplitude=profile_amplitude)[0]

    def fg(T):
        r = gp_fit_batch(s, T, profile=profile_amplitude)
        f = np.where(r["status"] == 0, -r["ll"], np.nan)
        return f, -r["grad"]

    θ, f, g, it = projected_lbfgs(fg, s.ψ.θ.copy(), lowerbounds, upperbounds, iterations)
    from .kernels import set_hyperparameters
    s.set_kernel(set_hyperparameters(s.ψ, θ))
    return dict(theta=θ, neg_log_likelihood=f, gradient=g, iterations=it)


def optimize_multi(surs, lowerbounds, upperbounds, iterations=30, device=False, profile_amplitude=False):
    """optimize for the surrogates of k lockstep trials: the minimisations advance together, and
    each round's evaluations -- one line search per surrogate still running -- are ONE
    gp_fit_multi launch instead of one launch per surrogate.  Every surrogate ends with the θ,
    objective, gradient and iteration count optimize alone gives it.  Returns optimize's dict per
    surrogate.  device=True runs the whole minimisation in one device-resident call
    (gp_optimize_multi: no host round trip per round) and then set_kernel on the host as before.
    profile_amplitude=True maximises the profiled-amplitude likelihood instead (on either path)."""
    surs = list(surs)
    check_fit_batch(surs)
    std = [bool(getattr(s, "standardize", False)) for s in surs]
    if any(std) and not all(std):
        raise ValueError("optimize_multi: standardised and plain surrogates in one batch")
    profile_amplitude = bool(profile_amplitude) or std[0]   # a standardised surrogate fits its amplitude
    from .kernels import set_hyperparameters
    if device:
        r = gp_optimize_multi(surs, None, lowerbounds, upperbounds, iterations, profile_amplitude=profile_amplitude)
        out = []
        for q, s in enumerate(surs):
            θ = r["theta"][q].copy()
            s.set_kernel(set_hyperparameters(s.ψ, θ))
            out.append(dict(theta=θ, neg_log_likelihood=float(r["neg_log_likelihood"][q]),
                            gradient=r["gradient"][q].copy(), iterations=int(r["iterations"][q])))
        return out

    def fg_multi(idx, T):
        r = gp_fit_multi([surs[i] for i in idx], T, profile=profile_amplitude)
        f = np.where(r["status"] == 0, -r["ll"], np.nan)
        return f, -r["grad"]

    res = projected_lbfgs_multi(fg_multi, [s.ψ.θ.copy() for s in surs], lowerbounds, upperbounds, iterations)
    out = []
    for s, (θ, f, g, it) in zip(surs, res):
        s.set_kernel(set_hyperparameters(s.ψ, θ))
        out.append(dict(theta=θ, neg_log_likelihood=f, gradient=g, iterations=it))
    return out
