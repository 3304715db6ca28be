"""Non-myopic Bayesian-optimisation loop on the rollout acquisition.

Mirrors experiments/nonmyopic_bayesopt.jl -- its CLI, its experiment layout and its CSV outputs
(create_csv / write_to_csv, utils.jl:155-172) -- with the acquisition step routed through the
rollout path as the survey prescribes: the reference's main loop calls the myopic
multistart_base_solve! (:245-253) and its adaptive driver names a rollout_solver that is
defined nowhere (experiments/adaptive_bayesopt.jl:490), so the solver here is build-defined:

  batch = generate_batch(batch_size)             utils.jl:97-106 (Sobol + two near-bound points)
          + one restart next to the incumbent     (build-defined, rollout_solve)
  x_r  ← stochastic_solve from every batch point  utils.jl:235-265 (StandardSGA, eswavs stop),
         all restarts in one rollout launch per SGA iteration (stochastic_solve_batch)
  xnext = the restart with the largest final ETO mean, clamped to the box, that is not an
          already observed point

Per budget step the metrics are recorded as in the reference (:268-289): time of the solve,
gap and simple regret of the observations BEFORE conditioning on xnext, then condition!,
optionally optimize! (lengthscale MLE on the device, bounds [0.1, 5]), then the minimum
observation.  `allocations` is the reference's @timed byte count; the build records the
device workspace is preallocated and writes 0.

Parity with the reference's BO trajectories is unpinned: Julia's MersenneTwister initial
designs, Optim.jl's inner solves and the undefined rollout solver cannot be reproduced.
"""
import argparse
import os
import time

import numpy as np

from . import testfns as T
from .decision_rules import EI, LCB, POI
from .kernels import Matern52
from .optimizers import Adam, StandardSGA
from .rollout import _plan_for_multi, simulate_trajectory_mc_multi
from .surrogates import FantasySurrogate, Surrogate
from .trajectory import Trajectory, TrajectoryParameters
from .utils import ExperimentSetup, gap, generate_batch, simple_regret, stochastic_solve_multi

INITIAL_OBSERVATIONS = 5            # nonmyopic_bayesopt.jl:131
METRICS = ["times", "gaps", "allocations", "simple_regret", "minimum_observations"]   # :191
KERNEL_LBS, KERNEL_UBS = [0.1], [5.0]   # :230

TESTFNS = {
    "gramacylee": T.TestGramacyLee,
    "braninhoo": T.TestBraninHoo,
    "hartmann6d": T.TestHartmann6D,
    "rosenbrock": T.TestRosenbrock,
    **{f"ackley{d}d": (lambda d=d: T.TestAckley(d)) for d in (1, 2, 3, 4, 5, 8)},
    **{f"rastrigin{d}d": (lambda d=d: T.TestRastrigin(d)) for d in (1, 4)},
    "hartmann3d": T.TestHartmann3D,
    "sixhump": T.TestSixHump,
    "goldsteinprice": T.TestGoldsteinPrice,
    "griewank3d": lambda: T.TestGriewank(3),
    "levy10d": lambda: T.TestLevy(10),
}


# ---- CSV outputs (utils.jl:155-172) --------------------------------------------------------
def _fmt(v):
    v = float(v)
    return repr(v) if np.isfinite(v) else ("NaN" if np.isnan(v) else ("Inf" if v > 0 else "-Inf"))


def create_csv(filename, budget):
    """create_csv: header [trial; 1..budget] and one placeholder row of −1.0."""
    with open(filename + ".csv", "w") as f:
        f.write(",".join(["trial"] + [str(b) for b in range(1, budget + 1)]) + "\n")
        f.write(",".join(["-1.0"] * (budget + 1)) + "\n")


def write_to_csv(filename, data):
    """write_to_csv: append `data` as one row (CSV.write(Tables.table(data'), append=true) writes
    the budget values only, without a trial column)."""
    with open(filename + ".csv", "a") as f:
        f.write(",".join(_fmt(v) for v in np.asarray(data, dtype=np.float64).ravel()) + "\n")


def write_metadata(directory, budget, trials, starts):
    """write_metadata_to_file (:102-118)."""
    with open(os.path.join(directory, "metadata.txt"), "w") as f:
        f.write(f"Budget: {budget}\nNumber of Trials: {trials}\nNumber of Starts: {starts}\n")


# ---- one acquisition solve -------------------------------------------------------------------
class BoxAdam:
    """Adam (optimizers.jl:25-74) on the box-normalised coordinates u = (x − lb)/(ub − lb), projected
    onto the box after every step: a step of ≈ η box widths per coordinate whatever the scale of
    the objective (StandardSGA's fixed η either stalls or throws restarts out of the box when the
    acquisition's gradient is large, e.g. Branin's).  Build-defined: the reference's rollout solver
    is undefined (experiments/adaptive_bayesopt.jl:490)."""

    def __init__(self, lbs, ubs, η=0.02):
        self.lbs, self.ubs = np.asarray(lbs, float), np.asarray(ubs, float)
        self.w = self.ubs - self.lbs
        self.adam = Adam(η=η)

    def update(self, x, grad_f):
        u = (x - self.lbs) / self.w
        self.adam.update(u, np.asarray(grad_f, float) * self.w)
        x[:] = np.clip(self.lbs + self.w * u, self.lbs, self.ubs)
        return x


INCUMBENT_NUDGE = 1e-2     # box widths: the incumbent restart starts this far off the observed point


def incumbent_start(sur, lbs, ubs):
    """The incumbent restart: the best observed point moved INCUMBENT_NUDGE box widths towards the
    box centre in every coordinate (at an observed point σ and its gradient vanish, so a restart
    placed exactly there cannot move)."""
    X, y = sur.get_active_covariates(), sur.get_active_observations()
    xb = np.asarray(X[:, int(np.argmin(y))], float)
    w = ubs - lbs
    step = np.where(xb <= 0.5 * (lbs + ubs), 1.0, -1.0) * INCUMBENT_NUDGE * w
    return np.clip(xb + step, lbs, ubs)


def _device_solve(plan, x0, tp, es, sgd_iterations, eta, solver, incumbent, variance_reduction=False):
    """The acquisition solve as ONE library call (mrbo_rollout_solve) on the plan the host loop would
    use: the ascent from x0 (StandardSGA, or BoxAdam with Adam's default β1, β2, ε), the projection
    onto the box, the final evaluation and pick_restart.  Every output equals the host loop's.
    variance_reduction sets the plan's control-variate switch for the call and clears it afterwards
    (the plan is cached and shared with the calls that leave it off)."""
    if variance_reduction:
        plan.set_control_variate(True)
    try:
        # per-surrogate boxes: tp, es lists of S (equal MC streams), the starts d×nstarts×S
        xstarts = np.stack([e.get_starts() for e in es], axis=2) if isinstance(es, (list, tuple)) else es.get_starts()
        tp = tp[0] if isinstance(tp, (list, tuple)) else tp
        return plan.rollout_solve_host(x0, tp.rnstream_sequence, xstarts,
                                       optimizer="sga" if solver == "sga" else "box_adam", iterations=sgd_iterations,
                                       eta=eta, sample_size=tp.mc_iters, incumbent=incumbent)
    finally:
        if variance_reduction:
            plan.set_control_variate(False)


def rollout_solve(sur, lbs, ubs, horizon, mc_samples, batch_size, starts, sgd_iterations, theta, eta=0.01,
                  device=0, solver="sga", incumbent=True, trace=None, device_solve=False, variance_reduction=False):
    """xnext from the rollout acquisition: restarts from a Sobol batch (StandardSGA with step `eta`,
    or BoxAdam with `eta` box widths per step), best final ETO mean.

    incumbent=True adds one restart next to the best observed point (incumbent_start) and never
    returns an already observed point while another restart ends elsewhere.  Both are the build's
    answer to an acquisition that underflows to exactly 0 on the whole Sobol batch -- an objective
    of large scale under the reference's unit-variance, zero-mean surrogate (Rosenbrock,
    Goldstein–Price): every batch restart then has a zero gradient, the argmax ties at the first
    restart and the loop re-observes it for the rest of the budget.
    `trace`, a list, receives one dict per call (batch, final points, final ETO means, pick).
    device_solve=True runs the ascent, the final evaluation and the pick as one device-resident call
    (mrbo_rollout_solve) with the same results; the default keeps the host-driven loop.
    variance_reduction=True (the reference's --variance-reduction): every ETO row of the ascent and
    the final means use EI0 at the restart's point as a control variate (mrbo/variance.py, DESIGN.md
    §16), on either path with the same results.
    rollout_solve_multi on the one surrogate; the trace entry drops the surrogate axis."""
    multi = None if trace is None else []
    (out,) = rollout_solve_multi([sur], lbs, ubs, horizon, mc_samples, batch_size, starts, sgd_iterations, theta,
                                 eta=eta, device=device, solver=solver, incumbent=incumbent, trace=multi,
                                 device_solve=device_solve, variance_reduction=variance_reduction)
    if trace is not None:
        t = multi[0]
        entry = dict(batch=t["batch"][:, :, 0], x=t["x"][:, :, 0], means=t["means"][:, 0], pick=t["pick"][0])
        if device_solve:
            entry["result"] = t["result"]
        else:
            entry["history"] = [etos[0] for etos in t["history"]]
        trace.append(entry)
    return out


def pick_restart(sur, x, etos, lbs, ubs, incumbent):
    """rollout_solve's choice among the restarts' final points x (d×R): the largest final ETO mean,
    with incumbent=True never an already observed point while another restart ends elsewhere.
    Returns (index, the means with non-finite ones at −inf)."""
    means = np.array([e.mean() for e in etos])
    means = np.where(np.isfinite(means), means, -np.inf)
    rank = means.copy()
    if incumbent:
        Xa = sur.get_active_covariates()
        w = ubs - lbs
        d = np.abs((x[:, :, None] - Xa[:, None, :]) / w[:, None, None]).max(axis=0).min(axis=1)
        rank = np.where(d > 1e-9, rank, -np.inf) if (d > 1e-9).any() else rank
    return int(np.argmax(rank)), means


def rollout_solve_multi(surs, lbs, ubs, horizon, mc_samples, batch_size, starts, sgd_iterations, theta, eta=0.01,
                        device=0, solver="sga", incumbent=True, trace=None, device_solve=False,
                        variance_reduction=False):
    """rollout_solve for S surrogates of equal size at once (the lockstep trials of run(...,
    parallel_trials=k)): the same Sobol batch on each, its own incumbent restart, the outer ascent of
    all S·R restarts with one rollout launch per SGA iteration (stochastic_solve_multi) and one for
    the final ETO means.  Returns [(xnext, mean)] per surrogate, each what rollout_solve returns on
    that surrogate alone.  `trace`, a list, receives one dict per call (x0 d×R×S, the final points,
    the final ETO means R×S, the picks; the host loop adds its `history`).  device_solve=True: one
    mrbo_rollout_solve call on the surrogate batch instead of the host-driven loop, same results.
    variance_reduction=True: the control-variate ETO rows, as rollout_solve.

    lbs, ubs of shape (d, S): surrogate q solves over its own box [lbs[:, q], ubs[:, q]] -- its own
    Sobol batch, incumbent start, inner starts, BoxAdam box, projection and pick -- on ONE boxed plan
    (RolloutPlan.from_surrogates), one launch per iteration or one mrbo_rollout_solve call; result q is
    rollout_solve(surs[q], lbs[:, q], ubs[:, q], ...)."""
    lbs, ubs = np.asarray(lbs, float), np.asarray(ubs, float)
    if lbs.ndim == 2 or ubs.ndim == 2:
        return _rollout_solve_boxes(list(surs), lbs, ubs, horizon, mc_samples, batch_size, starts, sgd_iterations,
                                    theta, eta, device, solver, incumbent, trace, device_solve, variance_reduction)
    batch = generate_batch(batch_size, lbs, ubs)
    batches = [np.hstack([batch, incumbent_start(s, lbs, ubs)[:, None]]) if incumbent else batch for s in surs]
    x0 = np.stack(batches, axis=2)                                     # d×R×S
    tp = TrajectoryParameters(start=batch[:, 0], hypers=[theta], horizon=horizon, mc_iterations=mc_samples,
                              use_low_discrepancy_sequence=True, spatial_lowerbounds=lbs, spatial_upperbounds=ubs)
    es = ExperimentSetup(tp, number_of_starts=starts)
    trajs = [Trajectory(s, FantasySurrogate(s, horizon), start=batch[:, 0], hypers=[theta], horizon=horizon)
             for s in surs]
    if device_solve:
        plan = _plan_for_multi(list(surs), horizon, tp.rnstream_sequence.shape[0], x0.shape[1],
                               es.get_starts().shape[1], lbs, ubs, trajs[0].θ[0], device, {})
        r = _device_solve(plan, x0, tp, es, sgd_iterations, eta, solver, incumbent, variance_reduction)
        if trace is not None:
            trace.append(dict(batch=x0, x=r["x"], means=r["means"], pick=[int(k) for k in r["pick"]],
                              result=r["result"]))
        return [(r["xnext"][:, q].copy(), float(r["mean"][q])) for q in range(len(trajs))]
    opts = [[StandardSGA(η=eta) if solver == "sga" else BoxAdam(lbs, ubs, η=eta) for _ in range(x0.shape[1])]
            for _ in surs]
    x, history = stochastic_solve_multi(opts, surs, tp, es, x0, Ts=trajs, iterations=sgd_iterations, device=device,
                                        variance_reduction=variance_reduction)
    x = np.clip(x, lbs[:, None, None], ubs[:, None, None])
    brs = simulate_trajectory_mc_multi(trajs, tp, x, es.get_starts(), with_gradient=False, device=device,
                                       variance_reduction=variance_reduction)
    out, picks, all_means = [], [], []
    for q, s in enumerate(surs):
        xq = x[:, :, q]
        k, means = pick_restart(s, xq, brs[q].etos(with_gradient=False), lbs, ubs, incumbent)
        out.append((xq[:, k].copy(), float(means[k])))
        picks.append(k)
        all_means.append(means)
    if trace is not None:
        trace.append(dict(batch=x0, x=x.copy(), means=np.stack(all_means, axis=1), pick=picks, history=history))
    return out


def _rollout_solve_boxes(surs, lbs, ubs, horizon, mc_samples, batch_size, starts, sgd_iterations, theta, eta, device,
                         solver, incumbent, trace, device_solve, variance_reduction):
    """rollout_solve_multi with per-surrogate boxes lbs, ubs (d×S): everything rollout_solve derives
    from the box once per surrogate, the launches on one boxed plan."""
    from .engine import check_bounds
    S = len(surs)
    check_bounds(lbs, ubs, surs[0].X.shape[0], S)
    batches, tps, ess = [], [], []
    for q, s in enumerate(surs):
        lq, uq = np.ascontiguousarray(lbs[:, q]), np.ascontiguousarray(ubs[:, q])
        batch = generate_batch(batch_size, lq, uq)
        batches.append(np.hstack([batch, incumbent_start(s, lq, uq)[:, None]]) if incumbent else batch)
        tps.append(TrajectoryParameters(start=batch[:, 0], hypers=[theta], horizon=horizon, mc_iterations=mc_samples,
                                        use_low_discrepancy_sequence=True, spatial_lowerbounds=lq,
                                        spatial_upperbounds=uq))
        ess.append(ExperimentSetup(tps[q], number_of_starts=starts))
    x0 = np.stack(batches, axis=2)                                     # d×R×S
    trajs = [Trajectory(s, FantasySurrogate(s, horizon), start=batches[q][:, 0], hypers=[theta], horizon=horizon)
             for q, s in enumerate(surs)]
    if device_solve:
        from .rollout import per_surrogate_parameters
        per_surrogate_parameters(tps, S)   # the launch has one MC stream
        plan = _plan_for_multi(surs, horizon, tps[0].rnstream_sequence.shape[0], x0.shape[1],
                               ess[0].get_starts().shape[1], lbs, ubs, trajs[0].θ[0], device, {})
        r = _device_solve(plan, x0, tps, ess, sgd_iterations, eta, solver, incumbent, variance_reduction)
        if trace is not None:
            trace.append(dict(batch=x0, x=r["x"], means=r["means"], pick=[int(k) for k in r["pick"]],
                              result=r["result"]))
        return [(r["xnext"][:, q].copy(), float(r["mean"][q])) for q in range(S)]
    opts = [[StandardSGA(η=eta) if solver == "sga" else BoxAdam(lbs[:, q], ubs[:, q], η=eta)
             for _ in range(x0.shape[1])] for q in range(S)]
    x, history = stochastic_solve_multi(opts, surs, tps, ess, x0, Ts=trajs, iterations=sgd_iterations, device=device,
                                        variance_reduction=variance_reduction)
    x = np.clip(x, lbs[:, None, :], ubs[:, None, :])
    xstarts = np.stack([e.get_starts() for e in ess], axis=2)
    brs = simulate_trajectory_mc_multi(trajs, tps, x, xstarts, with_gradient=False, device=device,
                                       variance_reduction=variance_reduction)
    out, picks, all_means = [], [], []
    for q, s in enumerate(surs):
        xq = x[:, :, q]
        k, means = pick_restart(s, xq, brs[q].etos(with_gradient=False), lbs[:, q], ubs[:, q], incumbent)
        out.append((xq[:, k].copy(), float(means[k])))
        picks.append(k)
        all_means.append(means)
    if trace is not None:
        trace.append(dict(batch=x0, x=x.copy(), means=np.stack(all_means, axis=1), pick=picks, history=history))
    return out


def _check_parallel_trials(parallel_trials, reuse_surrogate):
    k = int(parallel_trials)
    if k < 1:
        raise ValueError(f"parallel_trials = {parallel_trials}: at least 1")
    if k > 1 and reuse_surrogate:
        raise ValueError("parallel_trials > 1 needs reuse_surrogate=False: with the reused surrogate trial t inherits "
                         "trial t-1's kernel and stale capacity buffer (Q3), a sequential dependence")
    return k


# ---- ARD surrogates in the loops (build-defined) ------------------------------
ARD_LB, ARD_UB = 0.1, 5.0            # the refit's box in every dimension: [0.1, 5]^d, as KERNEL_LBS / KERNEL_UBS


def _new_surrogate(ard, X, y, capacity, rule, standardize):
    """The loops' surrogate: Matérn-5/2, σn2 = 1e-6; with `ard` an ARDSurrogate starting at ℓ_u = 1."""
    if ard:
        from .ard import ARDSurrogate
        return ARDSurrogate(Matern52(), X, y, capacity=capacity, decision_rule=rule, σn2=1e-6, standardize=standardize)
    return Surrogate(Matern52(), X, y, capacity=capacity, decision_rule=rule, σn2=1e-6, standardize=standardize)


def _ard_rollout_pick(s, lbs, ubs, *args, **kw):
    """rollout_solve on ARDSurrogate s: the solve runs on s.inner over the whitened box, xnext is mapped
    back and clipped to the raw box.  The solver's step `eta` therefore acts in whitened coordinates
    (units of the fitted lengthscale; BoxAdam: widths of the whitened box)."""
    zl, zu = s.whitened_box(lbs, ubs)
    znext, mean = rollout_solve(s.inner, zl, zu, *args, **kw)
    return np.clip(s.unwhiten(znext), lbs, ubs), mean


def _ard_myopic_pick(s, lbs, ubs, guesses, theta, device):
    """multistart_base_solve on ARDSurrogate s: guesses and box whitened, the solve on s.inner (its
    x_tol acts in whitened coordinates), the minimiser mapped back and clipped to the raw box."""
    from .rbf_optim import base_solve_batch, findmin_candidates
    zl, zu = s.whitened_box(lbs, ubs)
    zs, fs, _ = base_solve_batch(s.inner, zl, zu, s.whiten(guesses), [theta], device=device)
    return np.clip(s.unwhiten(zs[:, findmin_candidates(zs, fs)]), lbs, ubs)


def _ard_rollout_picks(surs, lbs, ubs, *args, **kw):
    """_ard_rollout_pick for the lockstep trials `surs` as ONE rollout_solve_multi on their `inner`
    surrogates over their whitened boxes (a boxed plan); each xnext mapped back and clipped per trial."""
    boxes = [s.whitened_box(lbs, ubs) for s in surs]
    zl, zu = np.stack([b[0] for b in boxes], axis=1), np.stack([b[1] for b in boxes], axis=1)
    picks = rollout_solve_multi([s.inner for s in surs], zl, zu, *args, **kw)
    return [(np.clip(s.unwhiten(znext), lbs, ubs), mean) for s, (znext, mean) in zip(surs, picks)]


def _ard_myopic_picks(surs, lbs, ubs, guesses, theta, device):
    """_ard_myopic_pick for the lockstep trials `surs` as ONE base_solve_multi on their `inner`
    surrogates: boxes and guesses whitened per trial, minimisers mapped back and clipped per trial."""
    from .rbf_optim import base_solve_multi, findmin_candidates
    boxes = [s.whitened_box(lbs, ubs) for s in surs]
    zl, zu = np.stack([b[0] for b in boxes], axis=1), np.stack([b[1] for b in boxes], axis=1)
    zg = np.stack([s.whiten(guesses) for s in surs], axis=2)
    zs, fs, _ = base_solve_multi([s.inner for s in surs], zl, zu, zg, [theta], device=device)
    return [np.clip(s.unwhiten(zs[:, findmin_candidates(zs[:, :, q], fs[:, q]), q]), lbs, ubs)
            for q, s in enumerate(surs)]


def _check_ard(ard, optimize):
    if ard and not optimize:
        raise ValueError("ard=True needs optimize=True: the ARD lengthscales are what the refit fits "
                         "(without it every ℓ_u stays 1, the isotropic default)")


# ---- the experiment loop (nonmyopic_bayesopt.jl:120-300) -------------------------------------
def run(function_name, output_dir, budget=15, trials=60, starts=16, horizon=0, mc_samples=200, batch_size=8,
        sgd_iterations=50, optimize=False, seed=1906, device=0, log=print, rules=("ei", "poi", "lcb"), eta=0.01,
        initial_observations=INITIAL_OBSERVATIONS, solver="sga", fmini_over_capacity=True, incumbent=True,
        reuse_surrogate=True, parallel_trials=1, device_mle=False, device_solve=False, variance_reduction=False,
        standardize=False, ard=False):
    """The experiment loop; `rules` selects a subset of the reference's three acquisitions (all by
    default, as nonmyopic_bayesopt.jl), `eta` the StandardSGA step of the build-defined solver
    (default 0.01, StandardSGA's own default, optimizers.jl:9),
    `initial_observations` the initial design size (5 in the current script, :131), `solver` "sga"
    (StandardSGA, η = eta) or "adam" (BoxAdam, eta box widths per step); fmini_over_capacity=False
    turns the reference's Q3 off (fmini over the observed points, not the zero-padded buffer),
    incumbent=False drops rollout_solve's incumbent restart and no-repeat pick (the round-2 solver).
    reuse_surrogate=True (the reference, :233-235): one surrogate of capacity budget + initial for
    every rule and trial, reset! per trial -- the kernel carries over between trials, and fmini over
    the capacity buffer (Q3) sees the stale observations of the previous trial past the initial
    design; False: a fresh surrogate per trial (the round-3 loop).
    parallel_trials=k > 1 (needs reuse_surrogate=False, else ValueError): up to k trials advance in
    lockstep -- every budget step is ONE batched acquisition solve for their k surrogates (a
    surrogate batch, rollout_solve_multi), then each trial conditions (and optionally runs MLE) on
    its own surrogate.  The trials observe exactly what they observe one after another; `times`
    records the batched solve's wall time for each of its trials.
    device_mle=True (with optimize): the MLE refit's minimisation runs as one device-resident call
    (mle.optimize(..., device=True)); the default keeps the host-driven loop.
    device_solve=True: every acquisition solve is one device-resident call (mrbo_rollout_solve: the
    ascent, the final evaluation and the pick) with the host loop's results; the default keeps the
    host-driven loop.
    variance_reduction=True (the reference's --variance-reduction, nonmyopic_bayesopt.jl:64-66): every
    acquisition solve uses EI0 as a control variate (rollout_solve), on either solve path.
    standardize=True (build-defined): the surrogates fit their output scale
    (Surrogate(standardize=True): y = m + s·g), the acquisition runs on the standardised
    observations and `optimize` maximises the profiled-amplitude likelihood.  Gaps, regrets, minimum
    observations and the returned y stay in the objective's raw units.
    ard=True (build-defined; needs optimize=True, else ValueError): ARDSurrogates, one
    lengthscale per input dimension.  Each step refits the ells in the box [0.1, 5]^d (on the host, or with
    device_mle as one device call; with parallel_trials > 1 one batched refit per chunk), runs the
    acquisition solve on the surrogate's `inner` over the whitened box z = x/ells, maps xnext back and clips
    it to the raw box.  The inner solve's x_tol and the outer ascent's `eta` therefore act in whitened
    coordinates, i.e. in units of the fitted lengthscales.  Lockstep trials solve together: their whitened
    boxes differ, so the chunk's solve runs on a boxed plan (per-surrogate boxes, rollout_solve_multi with
    (d, S) bounds).  Every result carries `ells`, the trial's final lengthscales."""
    parallel_trials = _check_parallel_trials(parallel_trials, reuse_surrogate)
    _check_ard(ard, optimize)
    testfn = TESTFNS[function_name]()
    lbs, ubs = testfn.get_bounds()
    directory = os.path.join(output_dir, function_name)
    os.makedirs(directory, exist_ok=True)
    table = {"ei": (EI(), 0.0), "poi": (POI(), 0.0), "lcb": (LCB(), 2.0)}
    acquisitions = [f"rollout_{horizon}_{r}" for r in rules]
    dr_hypers = [table[r][1] for r in rules]
    rules = [table[r][0] for r in rules]
    for metric in METRICS:
        for acq in acquisitions:
            create_csv(os.path.join(directory, f"{acq}_{metric}"), budget)
    write_metadata(directory, budget, trials, starts)
    rng = np.random.default_rng(seed)
    initial_samples = [lbs[:, None] + (ubs - lbs)[:, None] * rng.random((testfn.dim, initial_observations))
                       for _ in range(trials)]
    true_minimum = float(testfn.f(np.asarray(testfn.xopt[0], dtype=np.float64)))
    results = {}
    sur = None
    if reuse_surrogate:    # :233 "Preallocate entire surrogate object and reuse"
        sur = _new_surrogate(ard, np.zeros((testfn.dim, 1)), np.zeros(1), budget + initial_observations, None,
                             standardize)
    for acq, rule, theta in zip(acquisitions, rules, dr_hypers):
        if reuse_surrogate:
            sur.set_decision_rule(rule)                                   # :241
        log(f"Conducting experiments with acquisition = {acq}")
        for t0_ in range(0, trials if parallel_trials > 1 else 0, parallel_trials):
            chunk = list(range(t0_, min(t0_ + parallel_trials, trials)))
            surs = [_new_surrogate(ard, initial_samples[t], testfn(initial_samples[t]), budget + initial_observations,
                                   rule, standardize) for t in chunk]
            for s in surs:
                s.fmini_over_capacity = fmini_over_capacity
            ell_starts = [float(s.ψ.lengthscale) for s in surs]
            initial_bests = [float(np.min(testfn(initial_samples[t]))) for t in chunk]
            rec = [{m: np.zeros(budget) for m in METRICS} for _ in chunk]
            mle_times = np.zeros(budget)   # wall time of the chunk's batched refit per budget step
            for b in range(budget):
                t0 = time.perf_counter()
                if ard:   # the trials' whitened boxes differ: one solve on a boxed plan
                    picks = _ard_rollout_picks(surs, lbs, ubs, horizon, mc_samples, batch_size, starts, sgd_iterations,
                                               theta, eta=eta, device=device, solver=solver, incumbent=incumbent,
                                               device_solve=device_solve, variance_reduction=variance_reduction)
                else:
                    picks = rollout_solve_multi(surs, lbs, ubs, horizon, mc_samples, batch_size, starts,
                                                sgd_iterations, theta, eta=eta, device=device, solver=solver,
                                                incumbent=incumbent, device_solve=device_solve,
                                                variance_reduction=variance_reduction)
                dt = time.perf_counter() - t0
                for s, r, (xnext, _), initial_best in zip(surs, rec, picks, initial_bests):
                    r["times"][b] = dt
                    observed_best = float(np.min(s.get_active_observations()))
                    r["simple_regret"][b] = simple_regret(true_minimum, observed_best)
                    r["gaps"][b] = gap(initial_best, observed_best, true_minimum)
                    s.condition(xnext, float(testfn.f(xnext)))
                    r["minimum_observations"][b] = float(np.min(s.get_active_observations()))
                if optimize:   # every trial has conditioned: one batched refit for the chunk
                    from .mle import optimize_multi
                    t0 = time.perf_counter()
                    if ard:
                        from .ard import optimize_ard_multi
                        optimize_ard_multi(surs, ARD_LB, ARD_UB, device=device_mle)
                    else:
                        optimize_multi(surs, KERNEL_LBS, KERNEL_UBS, device=device_mle)
                    mle_times[b] = time.perf_counter() - t0
            for trial, s, r, ell_start in zip(chunk, surs, rec, ell_starts):
                log(f"{acq} trial {trial + 1}/{trials}: gap {r['gaps'][-1]:.4f}, {r['times'].sum():.2f} s of solves")
                for metric in METRICS:
                    write_to_csv(os.path.join(directory, f"{acq}_{metric}"), r[metric])
                results[(acq, trial)] = dict(times=r["times"], gaps=r["gaps"], simple_regret=r["simple_regret"],
                                             minimum_observations=r["minimum_observations"], mle_times=mle_times.copy(),
                                             X=s.get_active_covariates().copy(), y=s.get_active_observations().copy(),
                                             ell_start=ell_start, ell_end=float(s.ψ.lengthscale),
                                             repeats=np.zeros(budget, dtype=bool))
                if ard:
                    results[(acq, trial)]["ells"] = s.ells.copy()
        for trial in range(trials if parallel_trials == 1 else 0):
            Xinit = initial_samples[trial]
            yinit = testfn(Xinit)
            if reuse_surrogate:
                sur.reset(Xinit, yinit)                                   # :253
            else:
                sur = _new_surrogate(ard, Xinit, yinit, budget + initial_observations, rule, standardize)
            sur.fmini_over_capacity = fmini_over_capacity
            ell_start = float(sur.ψ.lengthscale)
            initial_best = float(np.min(yinit))
            times, gaps, allocs, regrets, minobs = (np.zeros(budget) for _ in range(5))
            repeats = np.zeros(budget, dtype=bool)
            for b in range(budget):
                t0 = time.perf_counter()
                xnext, _ = (_ard_rollout_pick if ard else rollout_solve)(
                    sur, lbs, ubs, horizon, mc_samples, batch_size, starts, sgd_iterations, theta, eta=eta,
                    device=device, solver=solver, incumbent=incumbent, device_solve=device_solve,
                    variance_reduction=variance_reduction)
                times[b] = time.perf_counter() - t0
                observed_best = float(np.min(sur.get_active_observations()))
                regrets[b] = simple_regret(true_minimum, observed_best)
                gaps[b] = gap(initial_best, observed_best, true_minimum)
                sur.condition(xnext, float(testfn.f(xnext)))
                if optimize and ard:
                    from .ard import optimize_ard
                    optimize_ard(sur, ARD_LB, ARD_UB, device=device_mle)
                elif optimize:
                    from .mle import optimize as mle_optimize
                    mle_optimize(sur, KERNEL_LBS, KERNEL_UBS, device=device_mle)
                minobs[b] = float(np.min(sur.get_active_observations()))
            log(f"{acq} trial {trial + 1}/{trials}: gap {gaps[-1]:.4f}, {times.sum():.2f} s of solves")
            for metric, data in zip(METRICS, (times, gaps, allocs, regrets, minobs)):
                write_to_csv(os.path.join(directory, f"{acq}_{metric}"), data)
            results[(acq, trial)] = dict(times=times, gaps=gaps, simple_regret=regrets, minimum_observations=minobs,
                                         X=sur.get_active_covariates().copy(), y=sur.get_active_observations().copy(),
                                         ell_start=ell_start, ell_end=float(sur.ψ.lengthscale), repeats=repeats)
            if ard:
                results[(acq, trial)]["ells"] = sur.ells.copy()
    return results


# ---- the myopic experiment loop (experiments/myopic_bayesopt.jl:93-270) -----------------------
MYOPIC_RULES = {"ei": (EI, 0.0), "poi": (POI, 0.0), "lcb": (LCB, 2.0)}   # :151-153 (random: no solve)


def run_myopic(function_name, output_dir, budget=100, trials=60, starts=64, seed=1906, device=0, log=print,
               rules=("ei", "poi", "lcb"), optimize=True, initial_observations=INITIAL_OBSERVATIONS,
               reuse_surrogate=True, capacity=None, solve_margin=0.0, no_repeat=False, parallel_trials=1,
               device_mle=False, standardize=False, ard=False):
    """myopic_bayesopt.jl's loop: per budget step xnext = multistart_base_solve!(sur, …; guesses =
    generate_initial_guesses(starts, lbs, ubs), θfixed) -- the deterministic multistart local solve of
    the analytic acquisition on the base surrogate (:224-233), here mrbo_base_solve on the device --
    then the metrics before conditioning (:234-245), condition!, optimize! (lengthscale MLE, bounds
    [0.1, 5], :248-249) and the minimum observation.  CSVs `<acq>_<metric>.csv` as the reference.

    reuse_surrogate=True (the reference): ONE surrogate, built once with capacity = budget (:205),
    serves every rule (set_decision_rule!, :208) and every trial (reset!(sur, Xinit, yinit), :217).
    reset! keeps the kernel, so each trial starts from the lengthscale the previous trial's last
    optimize! left (only the very first trial starts at Matern52()'s ℓ = 1), and past `capacity`
    observations condition! conditions a discarded resized copy (Surrogate.condition).  False: a
    fresh surrogate with ℓ = 1 and capacity budget + initial per trial (the round-3 loop).

    solve_margin (diagnostic, build-defined; 0 = the reference's box): the acquisition is solved on
    the box shrunk by solve_margin·(ub − lb) per side -- a proxy for IPNewton's interior iterates
    (rbf_optim.jl:24-30: a log barrier keeps them off the faces), used to test whether the
    projected Newton's stops on the faces explain a difference.
    no_repeat (diagnostic, build-defined; False = the reference's findmin): the best start whose
    minimiser is not an observed point (within 1e-6 of a box width) is taken, to test whether
    re-observing a point explains a difference; every trial records its repeated observations.
    parallel_trials=k > 1 (needs reuse_surrogate=False, else ValueError): up to k trials advance in
    lockstep, every budget step one mrbo_base_solve launch on their k surrogates (base_solve_multi).
    device_mle=True: optimize!'s minimisation runs as one device-resident call
    (mle.optimize(..., device=True)); the default keeps the host-driven loop.
    standardize=True: surrogates that fit their output scale, as in run.
    ard=True (needs optimize=True, else ValueError; not with the no_repeat diagnostic): ARDSurrogates as in
    run -- the ells refit in [0.1, 5]^d after every observation, the multistart solve on `inner` with the
    guesses and the box whitened (its x_tol in whitened coordinates, units of the fitted lengthscales),
    the minimiser mapped back and clipped to the raw box; lockstep trials solve in one launch on a boxed
    plan (base_solve_multi with (d, S) bounds and whitened guesses d×n×S)."""
    from .rbf_optim import base_solve_batch, base_solve_multi, findmin_candidates, multistart_base_solve
    parallel_trials = _check_parallel_trials(parallel_trials, reuse_surrogate)
    _check_ard(ard, optimize)
    if ard and no_repeat:
        raise ValueError("ard=True: the no_repeat diagnostic is not available on ARD surrogates")
    from .utils import generate_initial_guesses
    testfn = TESTFNS[function_name]()
    lbs, ubs = testfn.get_bounds()
    directory = os.path.join(output_dir, "myopic", function_name)
    os.makedirs(directory, exist_ok=True)
    for metric in METRICS:
        for acq in rules:
            create_csv(os.path.join(directory, f"{acq}_{metric}"), budget)
    write_metadata(directory, budget, trials, starts)
    guesses = generate_initial_guesses(starts, lbs, ubs)                     # :186
    rng = np.random.default_rng(seed)
    initial_samples = [lbs[:, None] + (ubs - lbs)[:, None] * rng.random((testfn.dim, initial_observations))
                       for _ in range(trials)]                              # :187
    true_minimum = float(testfn.f(np.asarray(testfn.xopt[0], dtype=np.float64)))
    results = {}
    sur = None
    if reuse_surrogate:    # :205 "Preallocate entire surrogate object and reuse"
        # capacity = BUDGET as the reference; it must hold the initial design (a reset! past
        # capacity is a BoundsError in Julia), so a budget below it gets the design's size
        sur = _new_surrogate(ard, np.zeros((testfn.dim, 1)), np.zeros(1),
                             capacity or max(budget, initial_observations), None, standardize)
    for acq in rules:
        make_rule, theta = MYOPIC_RULES[acq]
        if reuse_surrogate:
            sur.set_decision_rule(make_rule())                            # :208
        log(f"Conducting experiments with acquisition = {acq}")
        for t0_ in range(0, trials if parallel_trials > 1 else 0, parallel_trials):
            chunk = list(range(t0_, min(t0_ + parallel_trials, trials)))
            surs = [_new_surrogate(ard, initial_samples[t], testfn(initial_samples[t]),
                                   capacity or budget + initial_observations, make_rule(), standardize)
                    for t in chunk]
            ell_starts = [float(s.ψ.lengthscale) for s in surs]
            initial_bests = [float(np.min(testfn(initial_samples[t]))) for t in chunk]
            rec = [{m: np.zeros(budget) for m in METRICS} for _ in chunk]
            reps = [np.zeros(budget, dtype=bool) for _ in chunk]
            mle_times = np.zeros(budget)   # wall time of the chunk's batched refit per budget step
            tol = 1e-6 * (ubs - lbs)[:, None]
            for b in range(budget):
                t0 = time.perf_counter()
                w = (ubs - lbs) * solve_margin
                if ard:   # the trials' whitened boxes differ: one solve on a boxed plan
                    ard_next = _ard_myopic_picks(surs, lbs + w, ubs - w, guesses, theta, device)
                else:
                    xs_, fs_, _ = base_solve_multi(surs, lbs + w, ubs - w, guesses, [theta], device=device)
                dt = time.perf_counter() - t0
                for q, (s, r, initial_best) in enumerate(zip(surs, rec, initial_bests)):
                    Xo = s.X[:, :s.observed]
                    if ard:
                        xnext = ard_next[q]
                    else:
                        xq, fq = xs_[:, :, q], fs_[:, q]
                        fresh = [i for i in range(xq.shape[1])
                                 if not (np.abs(Xo - xq[:, i:i + 1]) <= tol).all(axis=0).any()] if no_repeat else []
                        xnext = (xq[:, fresh[findmin_candidates(xq[:, fresh], fq[fresh])]] if fresh
                                 else xq[:, findmin_candidates(xq, fq)]).copy()
                    r["times"][b] = dt
                    reps[q][b] = bool((np.abs(Xo - xnext[:, None]) <= tol).all(axis=0).any())
                    observed_best = float(np.min(s.get_active_observations()))
                    r["simple_regret"][b] = simple_regret(true_minimum, observed_best)
                    r["gaps"][b] = gap(initial_best, observed_best, true_minimum)
                    s.condition(xnext, float(testfn.f(xnext)))
                    r["minimum_observations"][b] = float(np.min(s.get_active_observations()))
                if optimize:   # every trial has conditioned: one batched refit for the chunk
                    from .mle import optimize_multi
                    t0 = time.perf_counter()
                    if ard:
                        from .ard import optimize_ard_multi
                        optimize_ard_multi(surs, ARD_LB, ARD_UB, device=device_mle)
                    else:
                        optimize_multi(surs, KERNEL_LBS, KERNEL_UBS, device=device_mle)
                    mle_times[b] = time.perf_counter() - t0
            for trial, s, r, ell_start, rp in zip(chunk, surs, rec, ell_starts, reps):
                log(f"myopic {acq} trial {trial + 1}/{trials}: gap {r['gaps'][-1]:.4f}, "
                    f"{r['times'].sum():.2f} s of solves")
                for metric in METRICS:
                    write_to_csv(os.path.join(directory, f"{acq}_{metric}"), r[metric])
                results[(acq, trial)] = dict(times=r["times"], gaps=r["gaps"], simple_regret=r["simple_regret"],
                                             minimum_observations=r["minimum_observations"], mle_times=mle_times.copy(),
                                             X=s.get_active_covariates().copy(), y=s.get_active_observations().copy(),
                                             ell_start=ell_start, ell_end=float(s.ψ.lengthscale), repeats=rp)
                if ard:
                    results[(acq, trial)]["ells"] = s.ells.copy()
        for trial in range(trials if parallel_trials == 1 else 0):
            Xinit = initial_samples[trial]
            yinit = testfn(Xinit)
            if reuse_surrogate:
                sur.reset(Xinit, yinit)                                   # :217
            else:
                sur = _new_surrogate(ard, Xinit, yinit, capacity or budget + initial_observations, make_rule(),
                                     standardize)
            ell_start = float(sur.ψ.lengthscale)
            initial_best = float(np.min(yinit))
            times, gaps, allocs, regrets, minobs = (np.zeros(budget) for _ in range(5))
            repeats = np.zeros(budget, dtype=bool)
            xnext = np.zeros(testfn.dim)
            for b in range(budget):
                t0 = time.perf_counter()
                w = (ubs - lbs) * solve_margin
                if ard:
                    xnext[:] = _ard_myopic_pick(sur, lbs + w, ubs - w, guesses, theta, device)
                elif no_repeat:
                    xs_, fs_, _ = base_solve_batch(sur, lbs + w, ubs - w, guesses, [theta], device=device)
                    Xo = sur.X[:, :sur.observed]
                    tol = 1e-6 * (ubs - lbs)[:, None]
                    fresh = [i for i in range(xs_.shape[1])
                             if not (np.abs(Xo - xs_[:, i:i + 1]) <= tol).all(axis=0).any()]
                    pick = findmin_candidates(xs_[:, fresh], fs_[fresh]) if fresh else None
                    xnext[:] = xs_[:, fresh[pick]] if fresh else xs_[:, findmin_candidates(xs_, fs_)]
                elif solve_margin > 0.0:
                    multistart_base_solve(sur, xnext, lbs + w, ubs - w, guesses, [theta], device=device)
                else:
                    multistart_base_solve(sur, xnext, lbs, ubs, guesses, [theta], device=device)
                times[b] = time.perf_counter() - t0
                Xo = sur.X[:, :sur.observed]
                repeats[b] = bool((np.abs(Xo - xnext[:, None]) <= 1e-6 * (ubs - lbs)[:, None]).all(axis=0).any())
                observed_best = float(np.min(sur.get_active_observations()))
                regrets[b] = simple_regret(true_minimum, observed_best)
                gaps[b] = gap(initial_best, observed_best, true_minimum)
                sur.condition(xnext, float(testfn.f(xnext)))
                if optimize and ard:
                    from .ard import optimize_ard
                    optimize_ard(sur, ARD_LB, ARD_UB, device=device_mle)
                elif optimize:
                    from .mle import optimize as mle_optimize
                    mle_optimize(sur, KERNEL_LBS, KERNEL_UBS, device=device_mle)
                minobs[b] = float(np.min(sur.get_active_observations()))
            log(f"myopic {acq} trial {trial + 1}/{trials}: gap {gaps[-1]:.4f}, {times.sum():.2f} s of solves")
            for metric, data in zip(METRICS, (times, gaps, allocs, regrets, minobs)):
                write_to_csv(os.path.join(directory, f"{acq}_{metric}"), data)
            results[(acq, trial)] = dict(times=times, gaps=gaps, simple_regret=regrets, minimum_observations=minobs,
                                         X=sur.get_active_covariates().copy(), y=sur.get_active_observations().copy(),
                                         ell_start=ell_start, ell_end=float(sur.ψ.lengthscale), repeats=repeats)
            if ard:
                results[(acq, trial)]["ells"] = sur.ells.copy()
    return results


def parse(argv=None):
    """parse_command_line (nonmyopic_bayesopt.jl:4-75)."""
    ap = argparse.ArgumentParser("Non-myopic Bayesian optimisation on the MI355X rollout acquisition")
    ap.add_argument("--seed", type=int, default=1906)
    ap.add_argument("--optimize", action="store_true", help="optimize the surrogate's lengthscale (MLE)")
    ap.add_argument("--starts", type=int, default=16)
    ap.add_argument("--trials", type=int, default=60)
    ap.add_argument("--budget", type=int, default=15)
    ap.add_argument("--output-dir", required=True)
    ap.add_argument("--mc-samples", type=int, default=200)
    ap.add_argument("--horizon", type=int, default=0)
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--function-name", required=True, choices=sorted(TESTFNS))
    ap.add_argument("--sgd-iterations", type=int, default=50)
    ap.add_argument("--parallel-trials", type=int, default=1,
                    help="trials advanced in lockstep, one batched acquisition solve per budget step "
                         "(> 1 runs a fresh surrogate per trial)")
    ap.add_argument("--device-mle", action="store_true",
                    help="with --optimize: run the MLE refit's minimisation as one device-resident call")
    ap.add_argument("--device-solve", action="store_true",
                    help="run every acquisition solve as one device-resident call (same results)")
    ap.add_argument("--variance-reduction", action="store_true",
                    help="Use EI as a control variate for variance reduction")
    ap.add_argument("--standardize", action="store_true",
                    help="fit the surrogate's output scale (mean and amplitude) and run the acquisition on the "
                         "standardised observations; with --optimize the profiled-amplitude likelihood")
    ap.add_argument("--ard", action="store_true",
                    help="with --optimize: one lengthscale per input dimension (ARD), refit in [0.1, 5]^d; the "
                         "acquisition solve runs in the whitened coordinates x/ell")
    return ap.parse_args(argv)


def main(argv=None):
    a = parse(argv)
    run(a.function_name, a.output_dir, budget=a.budget, trials=a.trials, starts=a.starts, horizon=a.horizon,
        mc_samples=a.mc_samples, batch_size=a.batch_size, sgd_iterations=a.sgd_iterations, optimize=a.optimize,
        seed=a.seed, parallel_trials=a.parallel_trials, reuse_surrogate=a.parallel_trials == 1,
        device_mle=a.device_mle, device_solve=a.device_solve, variance_reduction=a.variance_reduction,
        standardize=a.standardize, ard=a.ard)


if __name__ == "__main__":
    main()
