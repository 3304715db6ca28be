"""simulate_trajectory_mc -- mirror of rollout.jl:279-340, running on libmrbo.so.

``simulate_trajectory_mc(T, tp; inner_solve_xstarts, resolutions, spatial_gradients_container,
hyperparameter_gradients_container)`` keeps the reference signature (one start point, M
samples, caller-owned containers overwritten in place, ExpectedTrajectoryOutput returned).
``simulate_trajectory_mc_batch`` is the MI355X-shaped entry: R restarts × M samples in one
launch, outputs left on the device.
"""
import hashlib

import numpy as np

from . import _lib
from .engine import RolloutPlan, from_device, to_device
from .trajectory import ExpectedTrajectoryOutput

_PLANS = {}


def _state_key(s):
    """What a plan is built from, by content: id(s) and s.version alone do not identify a surrogate --
    CPython reuses the id of a freed one, and a fresh surrogate starts at the same version -- so a
    plan cached for a surrogate that is gone was handed to its successor at the same address (as
    shim._key, which hashes the arrays for the same reason)."""
    n = s.observed
    h = hashlib.blake2b(digest_size=16)
    for a in (s.X[:, :n], s.L[:n, :n], s.c[:n], s.y[:n]):
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return (id(s), s.version, n, h.hexdigest(), s.ψ.kind, float(s.ψ.lengthscale), float(s.ψ.period), float(s.σn2),
            float(s.fmini()))


def _plan_for(s, h, M, R, nstarts, lbs, ubs, theta, device, opts):
    """The cached plan of one surrogate: the S = 1 surrogate batch."""
    return _plan_for_multi([s], h, M, R, nstarts, lbs, ubs, theta, device, opts)


def surrogate_dict(s):
    """The fields of a Surrogate that RolloutPlan.from_surrogates reads (its observed part)."""
    n = s.observed
    return dict(X=s.X[:, :n], L=s.L[:n, :n], c=s.c[:n], y=s.y[:n], kernel=s.ψ.kind, lengthscale=s.ψ.lengthscale,
                sigma_n2=s.σn2, fmini=s.fmini(), period=s.ψ.period)


def check_surrogate_batch(surrogates):
    """Host-side shape check of a surrogate batch: the surrogates share the input dimension, the
    number of observed points, the kernel family, σn2 and the decision rule (the plan carries one
    rule).  Raises ValueError; returns (d, N)."""
    if len(surrogates) < 1:
        raise ValueError("a surrogate batch needs at least one surrogate")
    s0 = surrogates[0]
    d, N = s0.X.shape[0], s0.observed
    g0 = s0.get_decision_rule()
    for q, s in enumerate(surrogates[1:], start=1):
        if s.X.shape[0] != d or s.observed != N:
            raise ValueError(f"surrogate {q} has d = {s.X.shape[0]}, N = {s.observed}; surrogate 0 has d = {d}, N = {N}")
        if s.ψ.kind != s0.ψ.kind or s.σn2 != s0.σn2:
            raise ValueError(f"surrogate {q} differs from surrogate 0 in its kernel family or σn2")
        g = s.get_decision_rule()
        if g.rule_id != g0.rule_id or g.σtol != g0.σtol:
            raise ValueError(f"surrogate {q} differs from surrogate 0 in its decision rule")
    return d, N


def _plan_key(ss, h, M, R, nstarts, lbs, ubs, theta, device, opts):
    """The plan cache's key.  The bounds enter with their shape: a (d,) box is shared, the same
    numbers as (d, S) are per-surrogate boxes -- another plan, whose calls take other xstarts."""
    lbs, ubs = np.asarray(lbs), np.asarray(ubs)
    return (tuple(_state_key(s) for s in ss), h, M, R, nstarts, lbs.shape, tuple(lbs.ravel(order="F")),
            ubs.shape, tuple(ubs.ravel(order="F")), float(theta), device, tuple(sorted(opts.items())))


def _plan_for_multi(ss, h, M, R, nstarts, lbs, ubs, theta, device, opts):
    """The plan cache: one RolloutPlan.from_surrogates plan for the surrogates `ss`, cached on their
    identities, versions and contents (_state_key).  lbs, ubs: (d,), or (d, S) for a boxed plan."""
    check_surrogate_batch(ss)
    g = ss[0].get_decision_rule()
    opts = dict(opts)
    opts.setdefault("rule", g.rule_id)       # the surrogates' base decision rule (Q12: T.θ)
    opts.setdefault("sigma_tol", g.σtol)
    key = _plan_key(ss, h, M, R, nstarts, lbs, ubs, theta, device, opts)
    p = _PLANS.get(key)
    if p is None:
        p = RolloutPlan.from_surrogates([surrogate_dict(s) for s in ss], h, M, R, nstarts, lbs, ubs, theta,
                                        device=device, **opts)
        if len(_PLANS) > 16:
            _PLANS.clear()
        _PLANS[key] = p
    return p


def raise_on_status(status):
    st = np.asarray(status)
    bad = st[st != 0]
    if bad.size:
        bits = int(np.bitwise_or.reduce(bad))
        msgs = [m for b, m in _lib.STATUS_BITS.items() if bits & b]
        raise FloatingPointError(f"{bad.size} trajectories failed: " + "; ".join(msgs))


class BatchResult:
    """Device-resident outputs of one batched launch (flat, column-major)."""

    def __init__(self, plan, out, eto):
        self.plan = plan
        self.out = out
        self.eto_dev = eto

    def numpy(self):
        p = self.plan
        d, M, R, h = p.d, p.M, p.R, p.h
        o = self.out
        res = dict(values=from_device(o["values"], (M, R)), status=from_device(o["status"], (M, R)))
        if "grad_x" in o:
            res["grad_x"] = from_device(o["grad_x"], (d, M, R))
            res["grad_theta"] = from_device(o["grad_theta"], (1, M, R))
        if "policy_x" in o:
            res["policy_x"] = from_device(o["policy_x"], (d, h + 1, M, R))
        if "obs" in o:
            res["obs"] = from_device(o["obs"], (h + 1, M, R))
        if "evals" in o:
            res["evals"] = from_device(o["evals"], (_lib.NCOUNTERS, M, R))
        if self.eto_dev is not None:
            res["eto"] = from_device(self.eto_dev, (2 + 2 * d + 2, R))
        return res

    def etos(self, with_gradient=True):
        e = from_device(self.eto_dev, (2 + 2 * self.plan.d + 2, self.plan.R))
        return [ExpectedTrajectoryOutput.from_row(e[:, r], self.plan.d, with_gradient) for r in range(self.plan.R)]


def simulate_trajectory_mc_batch(T, tp, x0s, inner_solve_xstarts, with_gradient=True, dual_y_dx=None, replay_x=None,
                                 want_policy=False, want_obs=False, device=0, rnstream=None,
                                 variance_reduction=False, **opts):
    """R restarts (columns of x0s) × tp.mc_iters samples in one kernel launch.  variance_reduction=True:
    a second launch at horizon 0 follows and the ETO rows are the control-variate ones
    (RolloutPlan.simulate_control / eto_cv); the per-trajectory outputs are unchanged."""
    x0s = np.asarray(x0s, dtype=np.float64)
    if x0s.ndim == 1:
        x0s = x0s.reshape(-1, 1)
    last = lambda a: None if a is None else np.asarray(a)[..., None]   # the S axis of the one surrogate
    return simulate_trajectory_mc_multi([T], tp, last(x0s), inner_solve_xstarts, with_gradient=with_gradient,
                                        dual_y_dx=last(dual_y_dx), replay_x=last(replay_x), want_policy=want_policy,
                                        want_obs=want_obs, device=device, rnstream=rnstream,
                                        variance_reduction=variance_reduction, **opts)[0]


def _eto(plan, dx0, drn, dxs, out, with_gradient, variance_reduction):
    """The ETO rows of a launch: mrbo_eto_reduce, or with variance_reduction the control launch at
    the same x0 and mrbo_eto_reduce_cv."""
    if not variance_reduction:
        return plan.eto(out)
    ctl = plan.simulate_control(dx0, drn, dxs, with_gradient=with_gradient)
    return plan.eto_cv(dx0, out, ctl, want_beta=False)[0]


def check_multi_x0s(x0s, S, d=None):
    """x0s of a surrogate batch: d×R×S (d×S: one restart each).  Raises ValueError; returns the
    float64 d×R×S array."""
    x0s = np.asarray(x0s, dtype=np.float64)
    if x0s.ndim == 2:
        x0s = x0s[:, None, :]
    if x0s.ndim != 3 or x0s.shape[2] != S or (d is not None and x0s.shape[0] != d):
        raise ValueError(f"x0s must be d×R×S with S = {S}" + (f", d = {d}" if d is not None else "") +
                         f"; got {x0s.shape}")
    return x0s


def per_surrogate_parameters(tp, S):
    """`tp` of a multi call: one TrajectoryParameters shared by the S surrogates -- returns (tp, None)
    -- or a list of S, one per surrogate, each with its own box -- returns (tp[0], (lbs, ubs)) with
    the bounds d×S.  The S share horizon, sample count and, bit for bit, the MC stream (the launch
    has one); a difference is a ValueError."""
    if not isinstance(tp, (list, tuple)):
        return tp, None
    if len(tp) != S:
        raise ValueError(f"{len(tp)} TrajectoryParameters for {S} surrogates")
    t0 = tp[0]
    for q, t in enumerate(tp[1:], start=1):
        if t.horizon != t0.horizon or t.mc_iters != t0.mc_iters:
            raise ValueError(f"TrajectoryParameters {q} differs from 0 in horizon or mc_iters")
        a, b = np.asarray(t.rnstream_sequence), np.asarray(t0.rnstream_sequence)
        if a.shape != b.shape or a.tobytes() != b.tobytes():
            raise ValueError(f"TrajectoryParameters {q} has another rnstream_sequence than 0: the surrogates of a "
                             "launch share the MC stream")
    bounds = [t.get_spatial_bounds() for t in tp]
    return t0, (np.stack([np.asarray(b[0], dtype=np.float64) for b in bounds], axis=1),
                np.stack([np.asarray(b[1], dtype=np.float64) for b in bounds], axis=1))


def check_multi_xstarts(xstarts, d, S, boxed, name="inner_solve_xstarts"):
    """The inner starts (or base-solve guesses) of a multi call: d×n shared, or with per-surrogate
    boxes d×n×S.  Raises ValueError; returns the float64 array."""
    xs = np.asarray(xstarts, dtype=np.float64)
    if boxed and (xs.ndim != 3 or xs.shape[0] != d or xs.shape[2] != S):
        raise ValueError(f"{name} must be d×n×S with d = {d}, S = {S} when every surrogate has its own box; "
                         f"got {xs.shape}")
    if not boxed and (xs.ndim != 2 or xs.shape[0] != d):
        raise ValueError(f"{name} must be d×n with d = {d}; got {xs.shape}")
    return xs


def simulate_trajectory_mc_multi(Ts, tp, x0s, inner_solve_xstarts, with_gradient=True, dual_y_dx=None,
                                 replay_x=None, want_policy=False, want_obs=False, device=0, rnstream=None,
                                 variance_reduction=False, **opts):
    """simulate_trajectory_mc_batch for S trajectories on S DIFFERENT base surrogates (Ts) in ONE
    kernel launch (RolloutPlan.from_surrogates): x0s is d×R×S -- R restarts per surrogate --, tp,
    the MC stream and the inner starts are shared, dual_y_dx / replay_x are d×h×M×R×S.  Returns one
    BatchResult per surrogate (views of the launch's device outputs), each bit-identical to
    simulate_trajectory_mc_batch(Ts[q], tp, x0s[:, :, q], ...).

    Per-surrogate boxes: tp a list of S TrajectoryParameters (their bounds the boxes, their MC
    streams equal bit for bit) and inner_solve_xstarts d×nstarts×S.  Still one launch (a boxed
    plan); result q is simulate_trajectory_mc_batch(Ts[q], tp[q], x0s[:, :, q],
    inner_solve_xstarts[:, :, q], ...)."""
    import torch
    Ts = list(Ts)
    S = len(Ts)
    if S < 1:
        raise ValueError("simulate_trajectory_mc_multi needs at least one trajectory")
    d0, _ = check_surrogate_batch([T.s for T in Ts])
    x0s = check_multi_x0s(x0s, S, d0)
    if any(float(T.θ[0]) != float(Ts[0].θ[0]) for T in Ts):
        raise ValueError("the trajectories of a surrogate batch share the decision-rule hyperparameter θ")
    d, R, _ = x0s.shape
    tp, boxes = per_surrogate_parameters(tp, S)
    lbs, ubs = tp.get_spatial_bounds() if boxes is None else boxes
    if boxes is not None or np.ndim(inner_solve_xstarts) != 2:   # (d, n) starts on a shared box: as ever
        inner_solve_xstarts = check_multi_xstarts(inner_solve_xstarts, d, S, boxes is not None)
    rn = tp.rnstream_sequence if rnstream is None else rnstream
    M = rn.shape[0]
    h = tp.horizon
    for name, a in (("dual_y_dx", dual_y_dx), ("replay_x", replay_x)):
        if a is not None and np.shape(a) != (d, max(h, 1), M, R, S):
            raise ValueError(f"{name} must be d×h×M×R×S = {(d, max(h, 1), M, R, S)}; got {np.shape(a)}")
    plan = _plan_for_multi([T.s for T in Ts], h, M, R, inner_solve_xstarts.shape[1], lbs, ubs, Ts[0].θ[0], device,
                           opts)
    dev = f"cuda:{device}"
    drn = rn if isinstance(rn, torch.Tensor) else to_device(rn, dev)
    out = plan.alloc_outputs(with_gradient=with_gradient, want_policy=want_policy, want_obs=want_obs)
    dx0, dxs = to_device(x0s, dev), to_device(inner_solve_xstarts, dev)
    plan.simulate(dx0, drn, dxs, out,
                  dual_y_dx=None if dual_y_dx is None else to_device(dual_y_dx, dev),
                  replay_x=None if replay_x is None else to_device(replay_x, dev))
    eto = _eto(plan, dx0, drn, dxs, out, with_gradient, variance_reduction)   # variance_reduction: as the batch call
    W = 2 + 2 * d + 2
    res = []
    for q in range(S):   # block q of every flat output: the surrogate index is the slowest
        oq = {k: v[q * (v.numel() // S):(q + 1) * (v.numel() // S)] for k, v in out.items()}
        res.append(BatchResult(plan, oq, eto[q * W * R:(q + 1) * W * R]))   # plan.R: restarts per surrogate
    return res


def simulate_trajectory_mc(T, tp, inner_solve_xstarts, resolutions, spatial_gradients_container=None,
                           hyperparameter_gradients_container=None, device=0, **opts):
    """rollout.jl:279-340 (the reference signature; one start point tp.x0)."""
    T.set_start(tp.get_starting_point())  # set_start!(T, get_starting_point(tp)) :287  (T.θ kept, Q12)
    with_gradient = spatial_gradients_container is not None and hyperparameter_gradients_container is not None
    br = simulate_trajectory_mc_batch(T, tp, T.x0.reshape(-1, 1), np.asarray(inner_solve_xstarts),
                                      with_gradient=with_gradient, device=device, **opts)
    res = br.numpy()
    raise_on_status(res["status"])
    resolutions[:] = res["values"][:, 0]
    if with_gradient:
        spatial_gradients_container[:, :] = res["grad_x"][:, :, 0]
        hyperparameter_gradients_container[:, :] = res["grad_theta"][:, :, 0]
    return ExpectedTrajectoryOutput.from_row(res["eto"][:, 0], T.x0.size, with_gradient)


def ghq_node_arrays(nodes, weights, indices):
    """nodes[indices[m]], weights[indices[m]] as M×depth column-major arrays (the sampler state
    set_nodes!/set_weights! receives per sample, rollout.jl:431-432)."""
    idx = np.asarray([np.asarray(ix, dtype=np.int64) for ix in indices])
    nodes = np.asarray(nodes, dtype=np.float64)
    weights = np.asarray(weights, dtype=np.float64)
    return np.asfortranarray(nodes[idx]), np.asfortranarray(weights[idx])


def simulate_trajectory_ghq_batch(T, tp, x0s, inner_solve_xstarts, nodes, weights, indices, with_gradient=True,
                                  dual_y_dx=None, replay_x=None, want_policy=False, want_obs=False, device=0, **opts):
    """Gauss–Hermite estimator for R restarts (columns of x0s) × len(indices) node vectors."""
    x0s = np.asarray(x0s, dtype=np.float64)
    if x0s.ndim == 1:
        x0s = x0s.reshape(-1, 1)
    d, R = x0s.shape
    tn, tw = ghq_node_arrays(nodes, weights, indices)
    M, depth = tn.shape
    if depth != tp.horizon + 1:   # GaussHermiteObservable max_invocations (observables.jl:59 assertion)
        raise ValueError(f"node vectors of depth {depth}; the rollout observes horizon+1 = {tp.horizon + 1} times")
    lbs, ubs = tp.get_spatial_bounds()
    plan = _plan_for(T.s, tp.horizon, M, R, inner_solve_xstarts.shape[1], lbs, ubs, T.θ[0], device, opts)
    dev = f"cuda:{device}"
    out = plan.alloc_outputs(with_gradient=with_gradient, want_policy=want_policy, want_obs=want_obs)
    plan.simulate_ghq(to_device(x0s, dev), to_device(tn, dev), to_device(tw, dev), to_device(inner_solve_xstarts, dev),
                      out, dual_y_dx=None if dual_y_dx is None else to_device(dual_y_dx, dev),
                      replay_x=None if replay_x is None else to_device(replay_x, dev))
    return BatchResult(plan, out, plan.eto(out))


def simulate_trajectory_ghq(T, tp, inner_solve_xstarts, resolutions, nodes, weights, indices,
                            spatial_gradients_container=None, hyperparameter_gradients_container=None, device=0,
                            **opts):
    """rollout.jl:409-467 (the reference signature): ETO of the Gauss–Hermite resolutions, mean and
    n−1 std exactly as the Monte-Carlo version (:452-466)."""
    T.set_start(tp.get_starting_point())
    with_gradient = spatial_gradients_container is not None and hyperparameter_gradients_container is not None
    br = simulate_trajectory_ghq_batch(T, tp, T.x0.reshape(-1, 1), np.asarray(inner_solve_xstarts), nodes, weights,
                                       indices, with_gradient=with_gradient, device=device, **opts)
    res = br.numpy()
    raise_on_status(res["status"])
    resolutions[:] = res["values"][:, 0]
    if with_gradient:
        spatial_gradients_container[:, :] = res["grad_x"][:, :, 0]
        hyperparameter_gradients_container[:, :] = res["grad_theta"][:, :, 0]
    return ExpectedTrajectoryOutput.from_row(res["eto"][:, 0], T.x0.size, with_gradient)


class SurrogateEval:
    """The lazily-forced quantities of eval(s, x, θ) (radial_basis_surrogates.jl:224-310)."""

    def __init__(self, col, d):
        self.μ = float(col[0])
        self.σ = float(col[1])
        self.αxθ = float(col[2])
        self.grad_μ = col[3:3 + d].copy()
        self.grad_σ = col[3 + d:3 + 2 * d].copy()
        self.grad_αx = col[3 + 2 * d:3 + 3 * d].copy()
        self.Hαx = col[3 + 3 * d:3 + 3 * d + d * d].reshape((d, d), order="F").copy()
        self.d2α_dxdθ = col[3 + 3 * d + d * d:3 + 4 * d + d * d].copy()


def evaluate_base(s, xs, θ, device=0):
    xs = np.asarray(xs, dtype=np.float64)
    d = xs.shape[0]
    lb = np.zeros(d)
    plan = _plan_for(s, 0, 1, 1, 1, lb, lb + 1.0, float(np.asarray(θ).ravel()[0]), device, {})
    out = plan.eval_base(xs)
    return [SurrogateEval(out[:, j], d) for j in range(out.shape[1])]
