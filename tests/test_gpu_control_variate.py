"""The EI control variate on the device (mrbo_simulate_control, mrbo_eto_reduce_cv,
mrbo_plan_set_control_variate, include/mrbo.h).  The specification is
mrbo/variance.py: the device's rows are held to cv_rows fed the device's own arrays and the read-back
mrbo_eval_base columns, at the project's ETO bars (tests/test_gpu.py: rtol 1e-12 on means, 1e-10 on
stds and gradient means), each taken relative to the sum of the magnitudes of the terms the output is
formed from; everything that the design makes exact is compared on raw bits.

Shapes (one per kernel path): half-wave d = 2, N = 20, h = 1, M = 32, R = 3; full-wave with the restart
table N = 40, h = 2; generic POI, d = 1, N = 8, h = 1; packed layout N = 100, h = 1, M = 8, R = 2; a
surrogate batch S = 2 of the half-wave shape.  The objective is smooth and of scale 0.45 under the
unit-variance prior, and every restart starts a few hundredths of a box width off the best observed
point, so that EI0 there is not negligible and each shape has trajectories whose best observation is
step 0 and others (asserted; checked beforehand on the CPU oracle -- the packed shape needs ℓ = 0.1:
with ℓ = 1 its 100 points pin the surrogate down and step 0 is always the best).  Every launch runs
once per module and is shared."""
import ctypes
import functools

import numpy as np
import pytest

import conftest  # noqa: F401  (sys.path)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MRBO_ERR_UNSUPPORTED = -2
ELLS = (1.0, 0.7, 1.3)

SHAPES = {
    "half": dict(d=2, N=20, h=1, M=32, R=3, S=1, rule="ei", spec=2, rpl=1),
    "square": dict(d=2, N=40, h=2, M=32, R=3, S=1, rule="ei", spec=1, rpl=1, restart_tables=1),
    "generic": dict(d=1, N=8, h=1, M=32, R=3, S=1, rule="poi", spec=0, rpl=1),
    "packed": dict(d=2, N=100, h=1, M=8, R=2, S=1, rule="ei", rpl=2, ell=0.1),
    "batch": dict(d=2, N=20, h=1, M=32, R=3, S=2, rule="ei", spec=2, rpl=1),
}
NSTARTS = 4


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def objective(d, q):
    lbs, ubs = -np.ones(d), 2.0 * np.ones(d)

    def f(X):
        U = (X - lbs[:, None]) / (ubs - lbs)[:, None]
        return 0.3 * (np.sin(3.0 * U.sum(axis=0) + q) + 0.5 * np.cos(5.0 * U[0] + 2.0 * q))
    return f, lbs, ubs


@functools.lru_cache(maxsize=None)
def problem(shape):
    """Surrogates, box, starts d×R×S, MC stream and inner starts of a shape."""
    from mrbo.decision_rules import EI, POI
    from mrbo.kernels import Matern52
    from mrbo.surrogates import Surrogate
    from mrbo.engine import rnstream
    from mrbo.utils import generate_initial_guesses, kronecker_quasirand
    sh = SHAPES[shape]
    d, N, R, S = sh["d"], sh["N"], sh["R"], sh["S"]
    surs, x0 = [], np.zeros((d, R, S))
    for q in range(S):
        f, lbs, ubs = objective(d, q)
        X = lbs[:, None] + (ubs - lbs)[:, None] * kronecker_quasirand(d, N, 37 * q)
        y = f(X)
        surs.append(Surrogate(Matern52((sh.get("ell", ELLS[q % 3]),)), X, y, capacity=N,
                              decision_rule=POI() if sh["rule"] == "poi" else EI(), σn2=1e-6))
        xb = X[:, int(np.argmin(y))]
        mid = 0.5 * (lbs + ubs)
        for r in range(R):   # off the best observed point: towards the centre along one axis, further per restart
            step = np.zeros(d)
            step[r % d] = sh.get("nudge", 0.02) * (1 + r // d)
            x0[:, r, q] = xb + np.where(xb <= mid, 1.0, -1.0) * step * (ubs - lbs)
    rn = rnstream(sh["M"], d, sh["h"] + 1)
    xs = generate_initial_guesses(NSTARTS - 2, lbs, ubs)
    assert xs.shape == (d, NSTARTS)
    return surs, lbs, ubs, x0, rn, xs


def make_plan(shape, h=None):
    from mrbo.engine import RolloutPlan
    from mrbo.rollout import surrogate_dict
    sh = SHAPES[shape]
    surs, lbs, ubs, _, _, xs = problem(shape)
    g = surs[0].get_decision_rule()
    h = sh["h"] if h is None else h
    if sh["S"] == 1:
        s = surs[0]
        n = s.observed
        return RolloutPlan(s.X[:, :n], s.L[:n, :n], s.c[:n], s.y[:n], s.ψ.kind, s.ψ.lengthscale, s.σn2, s.fmini(), h,
                           sh["M"], sh["R"], xs.shape[1], lbs, ubs, 0.0, period=s.ψ.period, rule=g.rule_id,
                           sigma_tol=g.σtol)
    return RolloutPlan.from_surrogates([surrogate_dict(s) for s in surs], h, sh["M"], sh["R"], xs.shape[1], lbs, ubs,
                                       0.0, rule=g.rule_id, sigma_tol=g.σtol)


@functools.lru_cache(maxsize=None)
def launched(shape):
    """Every launch of a shape, once: the rollout launch (with obs), the control launch on the same
    plan, simulate on a plan created with h = 0, both reductions, the base evaluation; numpy arrays
    with the restart index K = R·S flattened (surrogate slowest)."""
    import torch
    from mrbo.engine import to_device
    sh = SHAPES[shape]
    d, M, R, S, h = sh["d"], sh["M"], sh["R"], sh["S"], sh["h"]
    K = R * S
    surs, lbs, ubs, x0, rn, xs = problem(shape)
    plan, plan0 = make_plan(shape), make_plan(shape, h=0)
    dx0, drn, dxs = to_device(x0, DEV), to_device(rn, DEV), to_device(xs, DEV)
    out = plan.alloc_outputs(with_gradient=True, want_obs=True)
    plan.simulate(dx0, drn, dxs, out)
    n_before = len(plan.kernel_times(64))
    ctl = plan.simulate_control(dx0, drn, dxs)
    n_after = len(plan.kernel_times(64))
    out0 = plan0.alloc_outputs(with_gradient=True)
    plan0.simulate(dx0, to_device(rn[:, :, :1], DEV), dxs, out0)
    eto, beta = plan.eto_cv(dx0, out, ctl)
    plain = plan.eto(out)
    # test 5's rows: the h = 0 plan's own launch as target AND control
    ctl0 = plan0.simulate_control(dx0, to_device(rn[:, :, :1], DEV), dxs)
    eto0, beta0 = plan0.eto_cv(dx0, out0, ctl0)
    base = plan.eval_base(x0.reshape(d, K, order="F"))
    torch.cuda.synchronize()
    if S > 1:   # restart r of surrogate q: point q·R + r of block q
        base = np.stack([base[:, q * R + r, q] for q in range(S) for r in range(R)], axis=1)
    W = 2 + 2 * d + 2
    g = lambda t, shp: t.cpu().numpy().reshape(shp, order="F")
    return dict(
        plan=plan, plan0=plan0, dev=dict(x0=dx0, rn=drn, xs=dxs, out=out, ctl=ctl),
        values=g(out["values"], (M, K)), grad_x=g(out["grad_x"], (d, M, K)), grad_theta=g(out["grad_theta"], (M, K)),
        status=g(out["status"], (M, K)), obs=g(out["obs"], (h + 1, M, K)),
        values0=g(ctl["values0"], (M, K)), grad_x0=g(ctl["grad_x0"], (d, M, K)), status0=g(ctl["status0"], (M, K)),
        h0_values=g(out0["values"], (M, K)), h0_grad_x=g(out0["grad_x"], (d, M, K)), h0_status=g(out0["status"], (M, K)),
        h0c_values=g(ctl0["values0"], (M, K)), h0c_grad_x=g(ctl0["grad_x0"], (d, M, K)),
        eto=g(eto, (W, K)).T, beta=g(beta, (1 + d, K)), plain=g(plain, (W, K)).T,
        eto0=g(eto0, (W, K)).T, beta0=g(beta0, (1 + d, K)),
        base=base, fmini=np.repeat([s.fmini() for s in surs], R), ring=(n_before, n_after))


def spec_rows(L, d):
    """cv_rows on the device's own arrays and the read-back base columns."""
    from mrbo import variance as V
    b = L["base"]
    ei, gei = V.ei0(b[0], b[1], b[3:3 + d], b[3 + d:3 + 2 * d], L["fmini"])
    return V.cv_rows(L["values"], L["grad_x"], L["grad_theta"], L["values0"], L["grad_x0"], ei, gei) + (ei, gei)


# ---- 0. the shapes run the kernels they are there for ------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_shapes_reach_their_kernels(gpu, shape):
    sh = SHAPES[shape]
    info = launched(shape)["plan"].info()
    assert info["rpl"] == sh["rpl"] and info["S"] == sh["S"], info
    if "spec" in sh:
        assert info["spec"] == sh["spec"], info
    if "restart_tables" in sh:
        assert info["restart_tables"] == sh["restart_tables"], info
    L = launched(shape)
    assert not L["status"].any() and not L["status0"].any() and not L["h0_status"].any()


# ---- 1. the control launch is simulate on an h = 0 plan ----------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_control_launch_equals_a_horizon_zero_plan(gpu, shape):
    L = launched(shape)
    assert same_bits(L["values0"], L["h0_values"])
    assert same_bits(L["grad_x0"], L["h0_grad_x"])
    assert np.array_equal(L["status0"], L["h0_status"])
    # and on the h = 0 plan itself
    assert same_bits(L["h0c_values"], L["h0_values"]) and same_bits(L["h0c_grad_x"], L["h0_grad_x"])
    assert L["ring"][1] == L["ring"][0] + 1          # one entry of the timing ring


# ---- 2. trajectories whose best step is 0 ARE their control ------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_best_step_zero_trajectories_equal_their_control(gpu, shape):
    L = launched(shape)
    best0 = np.argmin(L["obs"], axis=0) == 0            # the first minimum, as resolve takes it
    print(f"{shape}: {int(best0.sum())} of {best0.size} trajectories have their best observation at step 0")
    assert best0.any() and (~best0).any()
    assert same_bits(L["values"][best0], L["values0"][best0])
    assert same_bits(L["grad_x"][:, best0], L["grad_x0"][:, best0])
    assert not same_bits(L["values"][~best0], L["values0"][~best0])


# ---- 3. the reduction against the specification ------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_eto_cv_against_the_specification(gpu, shape):
    d, M = SHAPES[shape]["d"], SHAPES[shape]["M"]
    L = launched(shape)
    eto, beta, ei, gei = spec_rows(L, d)
    assert (beta[0] != 0.0).any(), beta
    assert np.array_equal(beta == 0.0, L["beta"] == 0.0), (beta, L["beta"])
    series = [(L["values"], L["values0"], ei, 0, 1, 1e-12)] + [
        (L["grad_x"][a], L["grad_x0"][a], gei[a], 2 + a, 2 + d + a, 1e-10) for a in range(d)]
    worst = dict(mean=0.0, std=0.0, beta=0.0)
    for k, (a, b, e, cm, cs, rtol_mean) in enumerate(series):
        bt = beta[k]
        da, db = a - a.mean(axis=0), b - b.mean(axis=0)
        use = bt != 0.0
        e_ = np.where(use, e, 0.0)
        mag_mean = np.abs(a).sum(axis=0) / M + np.abs(bt) * (np.abs(b).sum(axis=0) / M + np.abs(e_))
        mag_std = np.sqrt(((np.abs(da) + np.abs(bt) * np.abs(db)) ** 2).sum(axis=0) / (M - 1))
        Saa, Sbb = (da * da).sum(axis=0), (db * db).sum(axis=0)
        with np.errstate(all="ignore"):
            mag_beta = np.where(use, np.sqrt(Saa / np.where(Sbb > 0, Sbb, 1.0)), 0.0)
        em, es, eb = np.abs(L["eto"][:, cm] - eto[:, cm]), np.abs(L["eto"][:, cs] - eto[:, cs]), np.abs(L["beta"][k] - bt)
        with np.errstate(all="ignore"):
            worst["mean"] = max(worst["mean"], np.nanmax(np.where(mag_mean > 0, em / (rtol_mean * mag_mean), 0.0)))
            worst["std"] = max(worst["std"], np.nanmax(np.where(mag_std > 0, es / (1e-10 * mag_std), 0.0)))
            worst["beta"] = max(worst["beta"], np.nanmax(np.where(mag_beta > 0, eb / (1e-10 * mag_beta), 0.0)))
        assert (em <= rtol_mean * mag_mean).all(), (k, em, rtol_mean * mag_mean)
        assert (es <= 1e-10 * mag_std).all(), (k, es, 1e-10 * mag_std)
        assert (eb <= 1e-10 * mag_beta).all(), (k, eb, 1e-10 * mag_beta)
    print(f"{shape}: worst fraction of the bar -- {worst}")
    # ∇θ: mrbo_eto_reduce's columns, bit for bit
    assert same_bits(L["eto"][:, 2 + 2 * d:], L["plain"][:, 2 + 2 * d:])


# ---- 4. a constant control: the plain row, bit for bit ------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_constant_control_gives_mrbo_eto_reduce_bits(gpu, shape):
    import torch
    L = launched(shape)
    plan, dv = L["plan"], L["dev"]
    ctl = {k: v.clone() for k, v in dv["ctl"].items()}
    ctl["values0"].fill_(0.125)
    ctl["grad_x0"].fill_(-3.0)
    eto, beta = plan.eto_cv(dv["x0"], dv["out"], ctl)
    torch.cuda.synchronize()
    assert same_bits(eto.cpu().numpy(), plan.eto(dv["out"]).cpu().numpy())
    assert not beta.cpu().numpy().any()
    # and a NaN control
    ctl["values0"].fill_(float("nan"))
    ctl["grad_x0"][::7] = float("nan")
    eto, beta = plan.eto_cv(dv["x0"], dv["out"], ctl)
    torch.cuda.synchronize()
    assert same_bits(eto.cpu().numpy(), plan.eto(dv["out"]).cpu().numpy())
    assert not beta.cpu().numpy()[0::1 + SHAPES[shape]["d"]].any()


# ---- 5. an h = 0 plan: the row is the base acquisition ------------------------------------------------
@pytest.mark.parametrize("shape", ["half", "square", "packed", "batch"])        # the EI, θ = 0 shapes
def test_horizon_zero_rows_are_eval_base(gpu, shape):
    d = SHAPES[shape]["d"]
    L = launched(shape)
    eto0, beta0, b = L["eto0"], L["beta0"], L["base"]
    assert np.array_equal(beta0, np.ones_like(beta0)), beta0
    stds = np.concatenate([eto0[:, 1:2], eto0[:, 2 + d:2 + 2 * d], eto0[:, 3 + 2 * d:]], axis=1)
    assert np.array_equal(stds, np.zeros_like(stds)), stds
    alpha, galpha = b[2], b[3 + 2 * d:3 + 3 * d]
    # scale: the terms α and ∇α are formed from, imp·Φ + σ·φ and φ·∇σ − Φ·∇μ with φ, Φ ≤ 1
    s_alpha = np.abs(L["fmini"] - b[0]) + np.abs(b[1])
    s_grad = np.abs(b[3:3 + d]) + np.abs(b[3 + d:3 + 2 * d])
    print(f"{shape}: |mean − α|/scale {np.abs(eto0[:, 0] - alpha) / s_alpha}, "
          f"|∇ − ∇α|/scale {np.abs(eto0[:, 2:2 + d].T - galpha) / s_grad}")
    assert (np.abs(eto0[:, 0] - alpha) <= 1e-10 * s_alpha).all()
    assert (np.abs(eto0[:, 2:2 + d].T - galpha) <= 1e-10 * s_grad).all()


# ---- 6. the control never raises a std ----------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_std_never_above_the_plain_one(gpu, shape):
    d = SHAPES[shape]["d"]
    L = launched(shape)
    cols = [1] + list(range(2 + d, 2 + 2 * d))
    use = L["beta"].T != 0.0                            # K×(1+d)
    assert use.any()
    assert (L["eto"][:, cols][use] <= L["plain"][:, cols][use] * (1.0 + 1e-12)).all()
    assert same_bits(L["eto"][:, cols][~use], L["plain"][:, cols][~use])


# ---- 10. a call without gradients ---------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["half", "batch"])
def test_no_gradient_call(gpu, shape):
    import torch
    d = SHAPES[shape]["d"]
    L = launched(shape)
    plan, dv = L["plan"], L["dev"]
    out = plan.alloc_outputs(with_gradient=False)
    plan.simulate(dv["x0"], dv["rn"], dv["xs"], out)
    ctl = plan.simulate_control(dv["x0"], dv["rn"], dv["xs"], with_gradient=False)
    assert "grad_x0" not in ctl
    eto, beta = plan.eto_cv(dv["x0"], out, ctl)
    torch.cuda.synchronize()
    K = SHAPES[shape]["R"] * SHAPES[shape]["S"]
    eto = eto.cpu().numpy().reshape((2 + 2 * d + 2, K), order="F").T
    beta = beta.cpu().numpy().reshape((1 + d, K), order="F")
    assert same_bits(ctl["values0"].cpu().numpy().reshape(L["values0"].shape, order="F"), L["values0"])
    assert same_bits(eto[:, :2], L["eto"][:, :2]) and same_bits(beta[0], L["beta"][0])
    assert same_bits(eto[:, 2:], np.zeros((K, 2 * d + 2))) and same_bits(beta[1:], np.zeros((d, K)))


# ---- 7. the solve: one call against the host loop, with the control variate ---------------------------
ITERS = 12
# Steps chosen on the CPU oracle (the host loop replayed with oracle.simulate_mc at h and at 0 and
# variance.cv_rows): with them restarts stop at iterations {1, 2, 7, 9} / {1, 2, 4} (half: sga / adam)
# and {1, 3} / {1, 9, 10} (generic) while others run to the budget; the test asserts it on the GPU's history
SOLVES = {
    # the half-wave kernel on a surrogate batch, through rollout_solve_multi
    "half": dict(d=2, N=20, h=1, M=16, batch=1, starts=2, S=3, rule="ei", eta=dict(sga=0.3, adam=0.02)),
    # the generic kernel on a plain plan, through rollout_solve
    "generic": dict(d=1, N=8, h=1, M=16, batch=6, starts=2, S=1, rule="poi", eta=dict(sga=1.0, adam=0.02)),
}


@functools.lru_cache(maxsize=None)
def solve_surrogates(name):
    from mrbo.decision_rules import EI, POI
    from mrbo.kernels import Matern52
    from mrbo.surrogates import Surrogate
    from mrbo.utils import kronecker_quasirand
    sh = SOLVES[name]
    surs = []
    for q in range(sh["S"]):
        f, lbs, ubs = objective(sh["d"], q)
        X = lbs[:, None] + (ubs - lbs)[:, None] * kronecker_quasirand(sh["d"], sh["N"], 37 * q + 4)
        surs.append(Surrogate(Matern52((ELLS[q % 3],)), X, f(X), capacity=sh["N"],
                              decision_rule=POI() if sh["rule"] == "poi" else EI(), σn2=1e-6))
    return surs, lbs, ubs


@functools.lru_cache(maxsize=None)
def solved(name, solver, device_solve, variance_reduction=True):
    from mrbo import bayesopt
    sh = SOLVES[name]
    surs, lbs, ubs = solve_surrogates(name)
    trace = []
    kw = dict(eta=sh["eta"][solver], solver=solver, incumbent=True, trace=trace, device_solve=device_solve,
              variance_reduction=variance_reduction)
    args = (lbs, ubs, sh["h"], sh["M"], sh["batch"], sh["starts"], ITERS, 0.0)
    if sh["S"] == 1:
        picks = [bayesopt.rollout_solve(surs[0], *args, **kw)]
        t = dict(trace[0])
        t["means"], t["x"], t["pick"] = np.asarray(t["means"])[:, None], t["x"][:, :, None], [t["pick"]]
        if "history" in t:
            t["history"] = [[etos] for etos in t["history"]]
        return picks, t
    return bayesopt.rollout_solve_multi(surs, *args, **kw), trace[0]


def stop_iterations(name, solver):
    from mrbo.utils import eswavs
    _, t = solved(name, solver, False)
    R, S = t["means"].shape
    stops = np.zeros((R, S), dtype=int)
    for i, per_sur in enumerate(t["history"]):
        for q in range(S):
            for r in range(R):
                e = per_sur[q][r]
                with np.errstate(all="ignore"):
                    if stops[r, q] == 0 and eswavs(e.gradient(), e.std_gradient() ** 2, SOLVES[name]["M"]):
                        stops[r, q] = i + 1
    return stops, len(t["history"])


@pytest.mark.parametrize("solver", ["sga", "adam"])
@pytest.mark.parametrize("name", list(SOLVES))
def test_one_call_equals_the_host_loop_with_the_control_variate(gpu, name, solver):
    (ph, th), (pd, td) = solved(name, solver, False), solved(name, solver, True)
    stops, launched_ = stop_iterations(name, solver)
    print(f"{name} {solver}: host stop iterations (restart × surrogate)\n{stops}\nhost launches {launched_}, "
          f"device result {td['result']}")
    stopped = stops[stops > 0]
    # restarts stop at different iterations, one strictly inside the budget, and one runs to its end
    assert len(set(stopped.tolist())) >= 2 and (stopped < ITERS).any() and (stops == 0).any(), stops
    for q, ((xa, ma), (xb, mb)) in enumerate(zip(ph, pd)):
        assert same_bits(xa, xb) and same_bits(np.array([ma]), np.array([mb])), (q, xa, xb, ma, mb)
    assert same_bits(th["x"], td["x"]), (th["x"], td["x"])
    assert same_bits(th["means"], td["means"]), (th["means"], td["means"])
    assert [int(k) for k in th["pick"]] == [int(k) for k in td["pick"]]
    res = td["result"]
    assert res[2] == 0 and res[3] == 0 and res[1] == launched_, (res, launched_)
    # and the option does something: the plain solve ends elsewhere
    _, tp = solved(name, solver, True, False)
    assert not same_bits(tp["means"], td["means"])


# ---- 8. the switch -------------------------------------------------------------------------------------
def test_switch_on_and_off_again_changes_nothing(gpu):
    from mrbo.bayesopt import incumbent_start
    from mrbo.engine import initial_guesses, rnstream
    from mrbo.utils import generate_batch
    sh = SOLVES["half"]
    surs, lbs, ubs = solve_surrogates("half")
    batch = generate_batch(sh["batch"], lbs, ubs)
    x0 = np.stack([np.hstack([batch, incumbent_start(s, lbs, ubs)[:, None]]) for s in surs], axis=2)
    rn, xs = rnstream(sh["M"], sh["d"], sh["h"] + 1), initial_guesses(sh["starts"], lbs, ubs)
    from mrbo.engine import RolloutPlan
    from mrbo.rollout import surrogate_dict
    mk = lambda: RolloutPlan.from_surrogates([surrogate_dict(s) for s in surs], sh["h"], sh["M"], x0.shape[1],
                                             xs.shape[1], lbs, ubs, 0.0, rule=0, sigma_tol=1e-8)
    kw = dict(optimizer="box_adam", iterations=ITERS, eta=0.02, sample_size=sh["M"], incumbent=True)
    never, switched = mk(), mk()
    a = never.rollout_solve_host(x0, rn, xs, **kw)
    switched.set_control_variate(True)
    on = switched.rollout_solve_host(x0, rn, xs, **kw)
    # mrbo_stochastic_solve refuses the switch, before any device work
    L = switched.lib
    from mrbo import _lib
    o = _lib.SolveOpts(_lib.MRBO_OPT_SGA, 3, 0.01, 0.9, 0.999, 1e-8, 0.0)
    res = (ctypes.c_int32 * 3)()
    xbuf = np.array(x0, dtype=np.float64).ravel(order="F").copy()
    p = lambda v: ctypes.c_void_p(v.ctypes.data)
    rc = L.mrbo_stochastic_solve(switched.handle, p(xbuf), p(np.ascontiguousarray(rn.ravel(order="F"))),
                                 p(np.ascontiguousarray(xs.ravel(order="F"))), None, ctypes.byref(o), None, None, res,
                                 _lib.MRBO_FLAG_HOST_POINTERS, None)
    assert rc == MRBO_ERR_UNSUPPORTED and b"control variate" in L.mrbo_last_error()
    assert same_bits(xbuf, x0.ravel(order="F"))
    switched.set_control_variate(False)
    b = switched.rollout_solve_host(x0, rn, xs, **kw)
    for k in a:
        assert a[k] == b[k] if k == "result" else same_bits(a[k], b[k]), k
    assert not same_bits(on["means"], a["means"])
    # and with the switch off again mrbo_stochastic_solve runs
    rc = L.mrbo_stochastic_solve(switched.handle, p(xbuf), p(np.ascontiguousarray(rn.ravel(order="F"))),
                                 p(np.ascontiguousarray(xs.ravel(order="F"))), None, ctypes.byref(o), None, None, res,
                                 _lib.MRBO_FLAG_HOST_POINTERS, None)
    assert rc == 0, L.mrbo_last_error()


# ---- 9. the BO loop ------------------------------------------------------------------------------------
def test_bo_loop_with_variance_reduction_on_both_paths(gpu, tmp_path):
    from mrbo import bayesopt
    kw = dict(horizon=1, budget=3, trials=2, mc_samples=16, batch_size=2, starts=4, sgd_iterations=3, rules=("ei",),
              reuse_surrogate=False, log=lambda *_: None, parallel_trials=2, variance_reduction=True)
    off = bayesopt.run("gramacylee", str(tmp_path / "off"), device_solve=False, **kw)
    on = bayesopt.run("gramacylee", str(tmp_path / "on"), device_solve=True, **kw)
    assert set(on) == set(off) and len(on) == 2
    for key in on:
        for k in ("X", "y", "gaps", "minimum_observations"):
            assert same_bits(np.ascontiguousarray(on[key][k]), np.ascontiguousarray(off[key][k])), (key, k)
    for m in bayesopt.METRICS:
        if m != "times":
            assert (open(tmp_path / "on" / "gramacylee" / f"rollout_1_ei_{m}.csv").read() ==
                    open(tmp_path / "off" / "gramacylee" / f"rollout_1_ei_{m}.csv").read()), m
