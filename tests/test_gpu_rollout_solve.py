"""The acquisition solve of a BO step as one device-resident call (mrbo_box_adam_step,
mrbo_pick_restart, mrbo_rollout_solve, include/mrbo.h).  The specification is the host-driven path
as it stands -- bayesopt.rollout_solve / rollout_solve_multi with device_solve=False, and below it
BoxAdam, StandardSGA, eswavs and pick_restart -- whose ETO rows already come from mrbo_eto_reduce.
So every output of the device path must equal the host path's BIT FOR BIT: float64 compared on
their raw bits (NaNs compare), indices and flags as integers.  No tolerance anywhere.

Surrogates are built as tests/test_gpu_surrogate_batch.py builds its own (Kronecker designs from a
different offset per surrogate, lengthscales 1.0, 0.7, 1.3 in turn), on Branin for the half-wave
shape and on a smooth objective of unit scale (`wave`) for the other two; data, offsets and steps
were chosen so that the HOST loop's history alone shows restarts stopping at different iterations
inside the budget and others running to its end (asserted before anything is compared).  Every solve
is run once per module and shared by the tests that read it.  d ≤ 6 throughout: eswavs on the device sums its d
ratios in index order, numpy switches to pairwise summation at d ≥ 8."""
import functools

import numpy as np
import pytest

import conftest  # noqa: F401  (sys.path)

pytestmark = pytest.mark.gpu

ELLS = (1.0, 0.7, 1.3)
ITERS = 12
DEV = "cuda:0"


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def wave(d, q):
    """A smooth objective of unit scale on the box [−1, 2]^d (under the unit-variance surrogate the
    acquisition then has a gradient, and Monte-Carlo noise on it, over the whole box -- Branin's
    values of 0..300 leave EI at exactly 0 on most of its box)."""
    lbs, ubs = -np.ones(d), 2.0 * np.ones(d)

    def f(X):
        U = (X - lbs[:, None]) / (ubs - lbs)[:, None]
        return np.sin(3.0 * U.sum(axis=0) + q) + 0.5 * np.cos(5.0 * U[0] + 2.0 * q)
    return f, lbs, ubs


def make_surrogates(fn, d, N, S, rule="ei", off=0):
    from mrbo import configs
    from mrbo.decision_rules import EI, POI
    from mrbo.kernels import Matern52
    from mrbo.surrogates import Surrogate
    from mrbo.utils import kronecker_quasirand
    surs = []
    for q in range(S):
        if fn == "wave":
            f, lbs, ubs = wave(d, q)
        else:
            f = configs.make_testfn(fn, d)
            lbs, ubs = f.get_bounds()
        X = lbs[:, None] + (ubs - lbs)[:, None] * kronecker_quasirand(d, N, 37 * q + off)
        surs.append(Surrogate(Matern52((ELLS[q % 3],)), X, f(X), capacity=N,
                              decision_rule=POI() if rule == "poi" else EI(), σn2=1e-6))
    return surs, lbs, ubs


def plain_plan(s, h, M, R, ns, lbs, ubs, theta=0.0):
    from mrbo.engine import RolloutPlan
    g = s.get_decision_rule()
    n = s.observed
    return RolloutPlan(s.X[:, :n], s.L[:n, :n], s.c[:n], s.y[:n], s.ψ.kind, s.ψ.lengthscale, s.σn2, s.fmini(), h, M,
                       R, ns, lbs, ubs, theta, period=s.ψ.period, rule=g.rule_id, sigma_tol=g.σtol)


def batch_plan(surs, h, M, R, ns, lbs, ubs, theta=0.0):
    from mrbo.engine import RolloutPlan
    from mrbo.rollout import surrogate_dict
    g = surs[0].get_decision_rule()
    return RolloutPlan.from_surrogates([surrogate_dict(s) for s in surs], h, M, R, ns, lbs, ubs, theta,
                                       rule=g.rule_id, sigma_tol=g.σtol)


# ---- the BoxAdam step ----------------------------------------------------------------------------
def test_box_adam_step_equals_box_adam_update(gpu):
    """d = 2, R = 6, hand-made ETO rows, three consecutive steps t = 1..3; no rollout is launched.
    Restart 0: an ordinary gradient; 1: a zero gradient with zero std (a NaN ratio: keeps iterating);
    2: iterates at t = 1, stopped by eswavs at t = 2, and offered a large gradient at t = 3 that it
    must ignore; 3 and 4: gradients that throw it over the lower / the upper face (clipped); 5: a NaN
    gradient component (a NaN ratio keeps iterating, x, m and v turn NaN there and stay)."""
    torch = gpu
    from mrbo.bayesopt import BoxAdam
    from mrbo.engine import to_device
    from mrbo.trajectory import ExpectedTrajectoryOutput
    from mrbo.utils import eswavs
    d, R, M, eta = 2, 6, 16, 0.02
    surs, lbs, ubs = make_surrogates("braninhoo", d, 8, 1)
    plan = plain_plan(surs[0], 0, M, R, 4, lbs, ubs)
    W = 2 + 2 * d + 2
    x = np.array([[1.0, 4.0], [2.5, 7.5], [-1.0, 11.0], [-4.9, 0.1], [9.9, 14.9], [3.0, 3.0]]).T.copy()   # d×R
    nan = np.nan
    #        restart:   0             1           2               3               4              5
    grads = [[(0.3, -0.2), (0.0, 0.0), (1.0, 1.0), (-50.0, -60.0), (50.0, 70.0), (nan, 0.1)],
             [(0.1, 0.25), (0.0, 0.0), (1e-3, 1e-3), (-40.0, 1.0), (45.0, -2.0), (0.2, 0.1)],
             [(-0.2, 0.15), (0.0, 0.0), (30.0, 30.0), (2.0, -1.0), (-1.0, 3.0), (0.2, nan)]]
    stds = [(0.05, 0.04), (0.0, 0.0), (1.0, 1.0), (1.0, 2.0), (2.0, 1.0), (0.01, 0.01)]
    etos = np.zeros((3, R, W))
    for t in range(3):
        for r in range(R):
            etos[t, r, 0:2] = (0.1 * r, 0.01)
            etos[t, r, 2:2 + d] = grads[t][r]
            etos[t, r, 2 + d:2 + 2 * d] = stds[r]
    # the host loop's step (stochastic_solve_batch): eswavs, else BoxAdam.update, per restart
    hx = x.copy()
    opts = [BoxAdam(lbs, ubs, η=eta) for _ in range(R)]
    hact = np.ones(R, dtype=np.int32)
    dx = to_device(x, DEV)
    dact = torch.ones(R, dtype=torch.int32, device=DEV)
    dm = torch.zeros(d * R, dtype=torch.float64, device=DEV)
    dv = torch.zeros(d * R, dtype=torch.float64, device=DEV)
    for t in range(3):
        with np.errstate(all="ignore"):
            for r in range(R):
                if not hact[r]:
                    continue
                e = ExpectedTrajectoryOutput.from_row(etos[t, r], d)
                if eswavs(e.gradient(), e.std_gradient() ** 2, M):
                    hact[r] = 0
                    continue
                opts[r].update(hx[:, r], e.gradient())
        plan.box_adam_step(torch.from_numpy(etos[t].ravel()).to(DEV), dx, dact, dm, dv, t + 1, M, eta=eta)
        gx = dx.cpu().numpy().reshape((d, R), order="F")
        gm = dm.cpu().numpy().reshape((d, R), order="F")
        gv = dv.cpu().numpy().reshape((d, R), order="F")
        hm = np.stack([o.adam.m[-1] if o.adam.m else np.zeros(d) for o in opts], axis=1)
        hv = np.stack([o.adam.v[-1] if o.adam.v else np.zeros(d) for o in opts], axis=1)
        assert np.array_equal(dact.cpu().numpy(), hact), (t, dact.cpu().numpy(), hact)
        assert same_bits(gx, hx), (t, gx, hx)
        assert same_bits(gm, hm), (t, gm, hm)
        assert same_bits(gv, hv), (t, gv, hv)
    # the cases are what they claim to be
    assert hact.tolist() == [1, 1, 0, 1, 1, 1]
    assert opts[2].adam.t == 1 and opts[0].adam.t == 3
    assert hx[0, 3] == lbs[0] and hx[1, 3] == lbs[1] and hx[0, 4] == ubs[0] and hx[1, 4] == ubs[1]
    assert np.isnan(hx[0, 5]) and np.isnan(hx[1, 5]) and np.isfinite(hx[:, :5]).all()
    assert len(plan.kernel_times(64)) == 0          # no rollout launch


# ---- the pick ------------------------------------------------------------------------------------
class _Mean:
    def __init__(self, v):
        self.v = v

    def mean(self):
        return self.v


def test_pick_restart_equals_the_host_rule(gpu):
    """d = 2, N = 5, R = 5, S = 2, crafted points and means, with and without the incumbent rule."""
    torch = gpu
    from mrbo.bayesopt import pick_restart
    from mrbo.engine import to_device
    d, N, R, S = 2, 5, 5, 2
    surs, lbs, ubs = make_surrogates("braninhoo", d, N, S)
    plan = batch_plan(surs, 0, 4, R, 4, lbs, ubs)
    W = 2 + 2 * d + 2
    X = [s.get_active_covariates() for s in surs]
    mid = 0.5 * (lbs + ubs)
    novel = lambda k: mid + 0.01 * (k + 1) * (ubs - lbs)        # nowhere near a Kronecker design point
    nan, inf = np.nan, np.inf
    scenarios = {
        # surrogate 0: a NaN and a +inf mean rank −inf; restarts 3 and 4 tie at the top and 3 sits exactly
        # on an observed point: with the rule 4 wins, without it the first of the tie.
        # surrogate 1: every restart on an observed point -- the plain argmax, ties to the first index
        "observed-and-ties": ([np.stack([novel(0), novel(1), novel(2), X[0][:, 1], novel(4)], axis=1),
                               X[1][:, [0, 1, 2, 3, 4]]],
                              [[nan, inf, 1.0, 2.0, 2.0], [0.5, 3.0, 3.0, -1.0, nan]],
                              {True: [4, 1], False: [3, 1]}),
        # surrogate 0: no finite mean at all: restart 0.  surrogate 1: the best mean belongs to a restart
        # with a NaN coordinate (not novel), restart 0 sits on an observed point, restart 1 is novel
        "all-minus-inf-and-nan-point": ([np.stack([novel(k) for k in range(5)], axis=1),
                                         np.stack([X[1][:, 2], novel(1), np.array([nan, mid[1]]), X[1][:, 0],
                                                   X[1][:, 4]], axis=1)],
                                        [[nan, inf, -inf, nan, inf], [4.0, 1.0, 9.0, 5.0, -inf]],
                                        {True: [0, 1], False: [0, 2]}),
    }
    for name, (xs, means, expect) in scenarios.items():
        x = np.stack(xs, axis=2)                                  # d×R×S
        eto = np.zeros((S, R, W))
        eto[:, :, 0] = np.array(means)
        dx, deto = to_device(x, DEV), torch.from_numpy(eto.ravel()).to(DEV)
        for incumbent in (True, False):
            dmeans = torch.zeros(R * S, dtype=torch.float64, device=DEV)
            xnext, mean, pick = plan.pick_restart(dx, deto, incumbent=incumbent, means=dmeans)
            xn2, mean2, pick2 = plan.pick_restart(dx, deto, incumbent=incumbent)          # means = NULL
            torch.cuda.synchronize()
            gx = xnext.cpu().numpy().reshape((d, S), order="F")
            for q in range(S):
                with np.errstate(all="ignore"):
                    k, hmeans = pick_restart(surs[q], x[:, :, q], [_Mean(v) for v in means[q]], lbs, ubs, incumbent)
                assert k == expect[incumbent][q], (name, incumbent, q, k)
                assert int(pick[q]) == k, (name, incumbent, q, int(pick[q]), k)
                assert same_bits(dmeans.cpu().numpy()[q * R:(q + 1) * R], hmeans), (name, incumbent, q)
                assert same_bits(gx[:, q], x[:, k, q]), (name, incumbent, q)
                assert same_bits(mean.cpu().numpy()[q:q + 1], np.array([float(hmeans[k])])), (name, incumbent, q)
            assert torch.equal(pick, pick2) and same_bits(xn2.cpu().numpy(), xnext.cpu().numpy())
            assert same_bits(mean2.cpu().numpy(), mean.cpu().numpy())


# ---- one call against the host loop ---------------------------------------------------------------
SHAPES = {
    # (a) the half-wave kernel
    "half": dict(fn="braninhoo", d=2, N=20, h=1, M=16, batch=1, starts=2, S=3, spec=2),
    # (b) the full-wave square layout
    "square": dict(fn="wave", d=2, N=40, h=2, M=16, batch=1, starts=2, S=2, spec=1),
    # (c) the generic kernel on a plain plan, through rollout_solve: 8 batch restarts + the incumbent's.
    # POI's gradient on the unit-scale objective is of order 1e-2 over a box 3 wide: StandardSGA gets
    # a step that lets restarts reach a stationary point (and eswavs stop them) within the budget
    "generic": dict(fn="wave", off=4, d=1, N=8, h=0, M=16, batch=6, starts=2, S=1, spec=0, rule="poi", plain=True,
                    eta=dict(sga=1.0, adam=0.02)),
}
ETA = {"sga": 0.01, "adam": 0.02}


def eta_of(shape, solver):
    return SHAPES[shape.partition(":")[0]].get("eta", ETA)[solver]


@functools.lru_cache(maxsize=None)
def surrogates(shape):
    sh = SHAPES[shape]
    return make_surrogates(sh["fn"], sh["d"], sh["N"], sh["S"], sh.get("rule", "ei"), sh.get("off", 0))


@functools.lru_cache(maxsize=None)
def solved(shape, solver, device_solve, iterations=ITERS):
    """(picks, trace entry) of one acquisition solve on a shape; one surrogate of (a) alone: shape
    "half:q"."""
    from mrbo import bayesopt
    name, _, q = shape.partition(":")
    sh = SHAPES[name]
    surs, lbs, ubs = surrogates(name)
    trace = []
    kw = dict(eta=eta_of(shape, solver), solver=solver, incumbent=True, trace=trace, device_solve=device_solve)
    args = (lbs, ubs, sh["h"], sh["M"], sh["batch"], sh["starts"], iterations, 0.0)
    if sh.get("plain") or q:
        picks = [bayesopt.rollout_solve(surs[int(q or 0)], *args, **kw)]
        t = dict(trace[0])
        t["means"] = np.asarray(t["means"])[:, None]
        t["x"] = t["x"][:, :, None]
        t["pick"] = [t["pick"]]
        if "history" in t:
            t["history"] = [[etos] for etos in t["history"]]
        return picks, t
    return bayesopt.rollout_solve_multi(surs, *args, **kw), trace[0]


def stop_iterations(shape, solver, iterations=ITERS):
    """From the host loop's history alone: the iteration at which eswavs stops every restart (0: it
    runs to the budget), R×S."""
    from mrbo.utils import eswavs
    _, t = solved(shape, solver, False, iterations)
    M = SHAPES[shape.partition(":")[0]]["M"]
    R, S = t["means"].shape
    stops = np.zeros((R, S), dtype=int)
    for i, per_sur in enumerate(t["history"]):
        for q in range(S):
            for r in range(R):
                e = per_sur[q][r]
                if stops[r, q] == 0 and eswavs(e.gradient(), e.std_gradient() ** 2, M):
                    stops[r, q] = i + 1
    return stops, len(t["history"])


def spread_of_stops(stops, iterations=ITERS):
    """At least two restarts stop at different iterations, one of them strictly inside the budget,
    and at least one restart runs to the budget."""
    stopped = stops[stops > 0]
    return len(set(stopped.tolist())) >= 2 and (stopped < iterations).any() and (stops == 0).any()


def assert_same_solve(a, b, label):
    (pa, ta), (pb, tb) = a, b
    assert len(pa) == len(pb)
    for q, ((xa, ma), (xb, mb)) in enumerate(zip(pa, pb)):
        assert same_bits(xa, xb), f"{label}: xnext of surrogate {q} differs: {xa} {xb}"
        assert same_bits(np.array([ma]), np.array([mb])), f"{label}: mean of surrogate {q} differs: {ma} {mb}"
    assert same_bits(ta["x"], tb["x"]), f"{label}: end points differ\n{ta['x']}\n{tb['x']}"
    assert same_bits(ta["means"], tb["means"]), f"{label}: means differ\n{ta['means']}\n{tb['means']}"
    assert [int(k) for k in ta["pick"]] == [int(k) for k in tb["pick"]], f"{label}: picks differ"


@pytest.mark.parametrize("solver", ["sga", "adam"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_one_call_equals_the_host_loop(gpu, shape, solver):
    host, dev = solved(shape, solver, False), solved(shape, solver, True)
    stops, launched = stop_iterations(shape, solver)
    print(f"{shape} {solver}: host stop iterations (restart × surrogate)\n{stops}\nhost launches {launched}, "
          f"device result {dev[1]['result']}")
    # the comparison is not vacuous: restarts stop at different iterations, one strictly inside the
    # budget, and one runs to the budget
    assert spread_of_stops(stops), stops
    assert_same_solve(host, dev, f"{shape} {solver}")
    res = dev[1]["result"]
    assert res[2] == 0 and res[3] == 0, res                       # no trajectory failed in any launch
    assert res[1] == launched, (res, launched)
    assert res[0] <= min(ITERS, res[1] + 2), res


@pytest.mark.parametrize("shape", list(SHAPES))
def test_shapes_reach_their_kernels(gpu, shape):
    """The plan of each shape runs the kernel it is there for: half-wave, full-wave square, generic."""
    sh = SHAPES[shape]
    surs, lbs, ubs = surrogates(shape)
    R, ns = sh["batch"] + 2 + 1, sh["starts"] + 2           # generate_batch + the incumbent; initial guesses
    plan = (plain_plan(surs[0], sh["h"], sh["M"], R, ns, lbs, ubs) if sh.get("plain") else
            batch_plan(surs, sh["h"], sh["M"], R, ns, lbs, ubs))
    info = plan.info()
    assert info["spec"] == sh["spec"] and info["S"] == sh["S"], info
    assert info["rpl"] == 1, info


@pytest.mark.parametrize("solver", ["sga", "adam"])
def test_batch_block_equals_a_plain_plan(gpu, solver):
    """Shape (a): block q of every output of the S = 3 call equals the call on surrogate q's plain plan."""
    picks, t = solved("half", solver, True)
    for q in range(SHAPES["half"]["S"]):
        p1, t1 = solved(f"half:{q}", solver, True)
        assert same_bits(picks[q][0], p1[0][0]) and same_bits(np.array([picks[q][1]]), np.array([p1[0][1]])), q
        assert same_bits(t["x"][:, :, q], t1["x"][:, :, 0]), (q, t["x"][:, :, q], t1["x"][:, :, 0])
        assert same_bits(t["means"][:, q], t1["means"][:, 0]), q
        assert int(t["pick"][q]) == int(t1["pick"][0]), q


def _half_inputs():
    """Shape (a)'s plan inputs as rollout_solve_multi forms them."""
    from mrbo.bayesopt import incumbent_start
    from mrbo.engine import initial_guesses, rnstream
    from mrbo.utils import generate_batch
    sh = SHAPES["half"]
    surs, lbs, ubs = surrogates("half")
    batch = generate_batch(sh["batch"], lbs, ubs)
    x0 = np.stack([np.hstack([batch, incumbent_start(s, lbs, ubs)[:, None]]) for s in surs], axis=2)
    return surs, lbs, ubs, x0, rnstream(sh["M"], sh["d"], sh["h"] + 1), initial_guesses(sh["starts"], lbs, ubs)


@pytest.mark.parametrize("solver", ["sga", "adam"])
def test_device_pointers_equal_host_pointers(gpu, solver):
    torch = gpu
    from mrbo.engine import to_device
    sh = SHAPES["half"]
    surs, lbs, ubs, x0, rn, xs = _half_inputs()
    d, R, S = x0.shape
    plan = batch_plan(surs, sh["h"], sh["M"], R, xs.shape[1], lbs, ubs)
    kw = dict(optimizer="sga" if solver == "sga" else "box_adam", iterations=ITERS, eta=ETA[solver],
              sample_size=sh["M"], incumbent=True)
    h = plan.rollout_solve_host(x0, rn, xs, **kw)
    dx = to_device(x0, DEV)
    means = torch.zeros(R * S, dtype=torch.float64, device=DEV)
    active = torch.full((R * S,), -1, dtype=torch.int32, device=DEV)
    xnext, mean, pick, res = plan.rollout_solve(dx, to_device(rn, DEV), to_device(xs, DEV), means=means, active=active,
                                                **kw)
    assert res == h["result"]
    assert same_bits(dx.cpu().numpy(), h["x"].ravel(order="F"))
    assert same_bits(xnext.cpu().numpy(), h["xnext"].ravel(order="F"))
    assert same_bits(mean.cpu().numpy(), h["mean"]) and np.array_equal(pick.cpu().numpy(), h["pick"])
    assert same_bits(means.cpu().numpy(), h["means"].ravel(order="F"))
    assert np.array_equal(active.cpu().numpy(), h["active"].ravel(order="F"))
    # and both are the module's shared solve through bayesopt
    _, t = solved("half", solver, True)
    assert same_bits(h["x"], t["x"]) and same_bits(h["means"], t["means"]) and res == t["result"]
    # the stop flags: 1 exactly where the host history never stops the restart
    stops, _ = stop_iterations("half", solver)
    assert np.array_equal(h["active"] != 0, stops == 0), (h["active"], stops)


@pytest.mark.parametrize("solver", ["sga", "adam"])
def test_budget_of_one_iteration(gpu, solver):
    host, dev = solved("half", solver, False, 1), solved("half", solver, True, 1)
    assert_same_solve(host, dev, f"one iteration, {solver}")
    assert dev[1]["result"][:2] == (1, 1) and len(host[1]["history"]) == 1


def test_lagged_stop_when_every_restart_stops(gpu):
    """Shape (c)'s restarts that eswavs stops, alone on a plan (restart r of a launch equals an
    R = 1 launch at its x0, so they stop where they stop in the full batch): the host loop ends at
    the last of their stop iterations, inside the budget, and the call launches at most the LAG = 2
    iterations more that it takes the host to see it."""
    from mrbo.optimizers import StandardSGA
    from mrbo.surrogates import FantasySurrogate
    from mrbo.trajectory import Trajectory, TrajectoryParameters
    from mrbo.utils import ExperimentSetup, stochastic_solve_batch
    sh = SHAPES["generic"]
    (sur,), lbs, ubs = surrogates("generic")
    stops, _ = stop_iterations("generic", "sga")
    cols = np.flatnonzero(stops[:, 0] > 0)
    assert cols.size >= 2, stops
    x0 = solved("generic", "sga", False)[1]["batch"][:, cols]
    eta = eta_of("generic", "sga")
    tp = TrajectoryParameters(start=x0[:, 0], hypers=[0.0], horizon=sh["h"], mc_iterations=sh["M"],
                              use_low_discrepancy_sequence=True, spatial_lowerbounds=lbs, spatial_upperbounds=ubs)
    es = ExperimentSetup(tp, number_of_starts=sh["starts"])
    traj = Trajectory(sur, FantasySurrogate(sur, sh["h"]), start=x0[:, 0], hypers=[0.0], horizon=sh["h"])
    x, history = stochastic_solve_batch([StandardSGA(η=eta) for _ in cols], sur, tp, es, x0, T=traj, iterations=ITERS)
    assert len(history) == stops[cols, 0].max() < ITERS, (len(history), stops)
    plan = plain_plan(sur, sh["h"], sh["M"], cols.size, es.get_starts().shape[1], lbs, ubs)
    r = plan.rollout_solve_host(x0, tp.rnstream_sequence, es.get_starts(), optimizer="sga", iterations=ITERS, eta=eta,
                                sample_size=sh["M"], incumbent=False)
    res = r["result"]
    print(f"host launches {len(history)}, device result {res}")
    assert res[1] == len(history) and res[0] <= min(ITERS, res[1] + 2) and res[0] < ITERS, res
    assert res[2] == 0 and res[3] == 0 and (r["active"] == 0).all(), (res, r["active"])
    assert same_bits(r["x"], np.clip(x, lbs[:, None], ubs[:, None])), (r["x"], x)


@pytest.mark.parametrize("solver", ["sga", "adam"])
def test_the_plan_is_reused(gpu, solver):
    """A second call on the same plan, from other starts, equals a fresh plan's; a plain simulate
    after it runs every trajectory (nothing is skipped any more) and equals a fresh plan's."""
    torch = gpu
    from mrbo.engine import to_device
    sh = SHAPES["half"]
    surs, lbs, ubs, x0, rn, xs = _half_inputs()
    d, R, S = x0.shape
    kw = dict(optimizer="sga" if solver == "sga" else "box_adam", iterations=ITERS, eta=ETA[solver],
              sample_size=sh["M"], incumbent=True)
    x1 = lbs[:, None, None] + (ubs - lbs)[:, None, None] * (0.15 + 0.7 * ((x0 - lbs[:, None, None]) /
                                                                          (ubs - lbs)[:, None, None]))[:, ::-1, ::-1]
    used, fresh = (batch_plan(surs, sh["h"], sh["M"], R, xs.shape[1], lbs, ubs) for _ in range(2))
    first = used.rollout_solve_host(x0, rn, xs, **kw)
    assert (first["active"] == 0).any()                      # the first call did skip restarts
    a, b = used.rollout_solve_host(x1, rn, xs, **kw), fresh.rollout_solve_host(x1, rn, xs, **kw)
    assert set(a) == set(b)
    for k in a:
        assert a[k] == b[k] if k == "result" else same_bits(a[k], b[k]), k
    assert not same_bits(a["x"], first["x"])
    outs = []
    for plan in (used, fresh):
        out = plan.alloc_outputs(with_gradient=True, want_policy=True, want_obs=True, want_evals=True)
        for v in out.values():
            v.fill_(-7)                                       # a skipped trajectory would leave this
        plan.simulate(to_device(x0, DEV), to_device(rn, DEV), to_device(xs, DEV), out)
        torch.cuda.synchronize()
        outs.append({k: v.cpu().numpy() for k, v in out.items()})
    for k in outs[0]:
        assert same_bits(outs[0][k], outs[1][k]), k
    assert (outs[0]["status"] == 0).all()


# ---- the BO loop ---------------------------------------------------------------------------------
def _same_trials(a, b):
    assert set(a) == set(b)
    for key in a:
        for k in ("X", "y", "gaps", "minimum_observations"):
            assert same_bits(np.ascontiguousarray(a[key][k]), np.ascontiguousarray(b[key][k])), (key, k)


@pytest.mark.parametrize("parallel_trials,solver", [(3, "sga"), (1, "sga"), (3, "adam")])
def test_bo_loop_with_the_device_solve(gpu, tmp_path, parallel_trials, solver):
    from mrbo import bayesopt
    kw = dict(horizon=1, budget=2, trials=3, mc_samples=16, batch_size=2, starts=4, sgd_iterations=3, rules=("ei",),
              reuse_surrogate=False, log=lambda *_: None, parallel_trials=parallel_trials, solver=solver)
    off = bayesopt.run("gramacylee", str(tmp_path / "off"), device_solve=False, **kw)
    on = bayesopt.run("gramacylee", str(tmp_path / "on"), device_solve=True, **kw)
    assert len(on) == 3
    _same_trials(on, off)
    for m in bayesopt.METRICS:
        if m != "times":
            assert (open(tmp_path / "on" / "gramacylee" / f"rollout_1_ei_{m}.csv").read() ==
                    open(tmp_path / "off" / "gramacylee" / f"rollout_1_ei_{m}.csv").read())
