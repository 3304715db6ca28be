"""Surrogate batches on the device (mrbo_plan_create_batch, include/mrbo.h): ONE plan and one launch
for S independent base surrogates.  The yardstick is inside the project: restart r of a launch
equals an R = 1 launch at its x0 and outputs do not depend on the trajectory schedule, so block q of
every output of a surrogate batch must equal, BIT FOR BIT, what a plain mrbo_plan_create plan on
surrogate q computes from the same inputs -- float64 compared on their raw bits (NaNs compare),
status and counters as integers.  No tolerance anywhere.

Surrogates are built as configs.Problem builds its own: Kronecker designs (from a different start
offset per surrogate) scaled to the test function's box, y = f(X), and lengthscales 1.0, 0.7, 1.3
in turn, so neither the data nor the lengthscale coincide.  The shapes are the smallest that reach
each kernel layout; every launch is run once per module and shared by the tests that read it."""
import ctypes
import functools
import time

import numpy as np
import pytest

import conftest  # noqa: F401  (sys.path)

pytestmark = pytest.mark.gpu

ELLS = (1.0, 0.7, 1.3)
NSOBOL = 16     # inner starts: 16 Sobol points + 2 near-bound points, as the configurations

SHAPES = {
    # 1: half-wave kernel, 15 trajectories per surrogate: one half of the last wave idles
    "half_odd": dict(fn="gramacylee", d=1, N=8, h=1, M=5, R=3, S=3, spec=2),
    # 2: half-wave kernel at C2's layout
    "half_c2": dict(fn="braninhoo", d=2, N=32, h=2, M=8, R=2, S=2, spec=2),
    # 3: square full-wave layout, start tables in LDS
    "square": dict(fn="hartmann6d", d=6, N=64, h=3, M=8, R=2, S=3, spec=1, batch=1),
    # 4: packed layout, 2 rows per lane: global start tables, per-slot work scratch
    "packed": dict(fn="hartmann6d", d=6, N=80, h=3, M=4, R=2, S=2, rpl=2),
    # 5: generic kernel (shape 2 with the SE kernel and POI)
    "generic": dict(fn="braninhoo", d=2, N=32, h=2, M=8, R=2, S=2, kernel="se", rule="poi", spec=0),
    # 6: shape 3 with the quadratic cost model
    "cost": dict(fn="hartmann6d", d=6, N=64, h=3, M=8, R=2, S=2, cost=True),
    # S larger than the plain plan's workgroups per surrogate would be
    "half_odd_60": dict(fn="gramacylee", d=1, N=8, h=1, M=5, R=3, S=60, spec=2, compare=(0, 29, 59)),
}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def make_surrogates(sh):
    from mrbo import configs
    from mrbo.decision_rules import EI, POI
    from mrbo.kernels import Matern52, SquaredExponential
    from mrbo.surrogates import Surrogate
    from mrbo.utils import kronecker_quasirand
    tf = configs.make_testfn(sh["fn"], sh["d"])
    lbs, ubs = tf.get_bounds()
    w = (ubs - lbs)[:, None]
    kern = SquaredExponential if sh.get("kernel") == "se" else Matern52
    rule = POI if sh.get("rule") == "poi" else EI
    surs, x0s = [], []
    for q in range(sh["S"]):
        X = lbs[:, None] + w * kronecker_quasirand(sh["d"], sh["N"], 37 * q)
        surs.append(Surrogate(kern((ELLS[q % 3],)), X, tf(X), capacity=sh["N"], decision_rule=rule(), σn2=1e-6))
        x0s.append(lbs[:, None] + w * kronecker_quasirand(sh["d"], sh["R"], 37 * q + sh["N"]))
    return surs, np.stack(x0s, axis=2), lbs, ubs            # x0s: d×R×S


def plan_opts(sh, surs):
    g = surs[0].get_decision_rule()
    o = dict(rule=g.rule_id, sigma_tol=g.σtol)
    if sh.get("cost"):
        o.update(cost="quadratic", cost_c0=1.0, cost_w=tuple([1.0] * sh["d"]))
    return o


class Case:
    """One shape: its surrogates and inputs, the surrogate-batch plan and one plain plan per compared
    surrogate, and the outputs of one rollout launch on each (host copies)."""

    def __init__(self, name, ghq=False):
        import torch
        from mrbo.engine import RolloutPlan, initial_guesses, rnstream, to_device
        from mrbo.rollout import surrogate_dict
        sh = self.sh = SHAPES[name]
        self.surs, self.x0s, lbs, ubs = make_surrogates(sh)
        self.lbs, self.ubs = lbs, ubs
        S, d, h, M, R = sh["S"], sh["d"], sh["h"], sh["M"], sh["R"]
        self.compare = sh.get("compare", tuple(range(S)))
        self.xstarts = initial_guesses(NSOBOL, lbs, ubs)
        ns = self.xstarts.shape[1]
        opts = plan_opts(sh, self.surs)
        th = 0.0
        dicts = [surrogate_dict(s) for s in self.surs]
        if ghq:      # 3 Gauss–Hermite nodes: every node vector of depth h + 1
            from mrbo.rollout import ghq_node_arrays
            from mrbo.utils import gauss_hermite, generate_indices
            nodes, weights = gauss_hermite(3)
            self.tn, self.tw = ghq_node_arrays(nodes, weights, generate_indices(3, h + 1))
            M = self.tn.shape[0]
        self.M = M
        self.batched = RolloutPlan.from_surrogates(dicts, h, M, R, ns, lbs, ubs, th, **opts)
        self.plain = {q: RolloutPlan(s.X[:, :s.observed], s.L[:s.observed, :s.observed], s.c[:s.observed],
                                     s.y[:s.observed], s.ψ.kind, s.ψ.lengthscale, s.σn2, s.fmini(), h, M, R, ns, lbs,
                                     ubs, th, period=s.ψ.period, **opts)
                      for q, s in ((q, self.surs[q]) for q in self.compare)}
        dev = "cuda:0"
        self.dev_xs = to_device(self.xstarts, dev)
        if ghq:
            self.dev_in = (to_device(self.tn, dev), to_device(self.tw, dev))
        else:
            self.dev_in = (to_device(rnstream(M, d, h + 1), dev),)
        self.dev_x0 = to_device(self.x0s, dev)
        self.dev_x0_q = {q: to_device(self.x0s[:, :, q], dev) for q in self.compare}
        self.ghq = ghq
        self.launches_before = len(self.batched.kernel_times(64))
        self.out = self.launch(self.batched, self.dev_x0)
        self.launches_after = len(self.batched.kernel_times(64))
        self.ref = {q: self.launch(self.plain[q], self.dev_x0_q[q]) for q in self.compare}
        torch.cuda.synchronize()

    def launch(self, plan, dx0):
        import torch
        out = plan.alloc_outputs(with_gradient=True, want_policy=True, want_obs=True, want_evals=True)
        if self.ghq:
            plan.simulate_ghq(dx0, self.dev_in[0], self.dev_in[1], self.dev_xs, out)
        else:
            plan.simulate(dx0, self.dev_in[0], self.dev_xs, out)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    def block(self, out, k, q):
        n = out[k].size // self.sh["S"]
        return out[k][q * n:(q + 1) * n]

    def assert_blocks_equal(self, out=None, label=""):
        out = self.out if out is None else out
        for q in self.compare:
            for k, v in self.ref[q].items():
                assert same_bits(self.block(out, k, q), v), f"{label} surrogate {q}: output {k} differs"


@functools.lru_cache(maxsize=None)
def case(name, ghq=False):
    return Case(name, ghq)


OUTPUTS = {"values", "grad_x", "grad_theta", "status", "policy_x", "obs", "evals"}


@pytest.mark.parametrize("name", ["half_odd", "half_c2", "square", "packed", "generic", "cost"])
def test_batch_equals_plain_plans(gpu, name):
    c = case(name)
    sh = c.sh
    info = c.batched.info()
    assert info["S"] == sh["S"]
    for q in c.compare:
        pi = c.plain[q].info()
        assert pi["S"] == 1
        assert {k: v for k, v in pi.items() if k != "S"} == {k: v for k, v in info.items() if k != "S"}
    if "spec" in sh:
        assert info["spec"] == sh["spec"]
    if "batch" in sh:
        assert info["batch"] == sh["batch"]
    if "rpl" in sh:
        assert info["rpl"] == sh["rpl"] and info["batch"] == 1     # global start tables
    if sh.get("cost"):
        assert info["spec"] in (0, 3)      # 3 where the kernel unit carries the cost specialisation
    assert set(c.out) == OUTPUTS
    T = sh["M"] * sh["R"] * sh["S"]
    assert c.out["values"].size == T and c.out["grad_x"].size == sh["d"] * T
    assert (c.out["status"] == 0).all()
    # not a vacuous comparison (the 1-D Gramacy–Lee trajectories at h = 1 have a ±0 spatial gradient
    # on the plain plans too: their bits, signs included, are compared below like any others)
    assert (c.out["values"] != 0).any() and ((c.out["grad_x"] != 0).any() or sh["d"] == 1)
    # the surrogates do differ: no two blocks of values coincide
    v = c.out["values"].reshape(sh["S"], -1)
    assert all(not same_bits(v[0], v[q]) for q in range(1, sh["S"]))
    c.assert_blocks_equal(label=name)


def test_more_surrogates_than_workgroups_per_surrogate(gpu):
    """S = 60: every surrogate still gets a workgroup (grid (max(1, ⌈blocks/S⌉), S)); surrogates 0, 29
    and 59 are compared with their plain plans, the rest checked for status."""
    c = case("half_odd_60")
    assert c.batched.info()["S"] == 60
    assert c.out["status"].size == 60 * 15 and (c.out["status"] == 0).all()
    c.assert_blocks_equal(label="S=60")


def test_from_surrogates_with_one_surrogate_is_the_plain_plan(gpu):
    import torch
    from mrbo.engine import RolloutPlan
    from mrbo.rollout import surrogate_dict
    c = case("square")
    sh = c.sh
    one = RolloutPlan.from_surrogates([surrogate_dict(c.surs[1])], sh["h"], sh["M"], sh["R"], c.xstarts.shape[1], c.lbs,
                                      c.ubs, 0.0, **plan_opts(sh, c.surs))
    assert one.S == 1 and one.info() == c.plain[1].info()
    out = c.launch(one, c.dev_x0_q[1])
    torch.cuda.synchronize()
    for k, v in c.ref[1].items():
        assert same_bits(out[k], v), k


def test_any_grid(gpu, monkeypatch):
    """MRBO_MAX_WPG=1 (one wave per workgroup, another grid): the same bits."""
    from mrbo.engine import RolloutPlan
    from mrbo.rollout import surrogate_dict
    c = case("half_c2")
    sh = c.sh
    monkeypatch.setenv("MRBO_MAX_WPG", "1")
    p1 = RolloutPlan.from_surrogates([surrogate_dict(s) for s in c.surs], sh["h"], sh["M"], sh["R"],
                                     c.xstarts.shape[1], c.lbs, c.ubs, 0.0, **plan_opts(sh, c.surs))
    assert p1.info()["waves_per_group"] == 1 and p1.info()["S"] == sh["S"]
    c.assert_blocks_equal(c.launch(p1, c.dev_x0), "MRBO_MAX_WPG=1")


def test_ghq(gpu):
    """Gauss–Hermite estimator on shape 2 with 3 nodes, S = 2: the rollout observes h + 1 = 3 times, so
    the tensor product of 3 nodes is 27 node vectors (9 would be the product at h = 1)."""
    c = case("half_c2", True)
    assert c.M == 3 ** (c.sh["h"] + 1)
    assert (c.out["values"] != 0).any()
    c.assert_blocks_equal(label="ghq")


def test_one_launch_per_simulate(gpu):
    """mrbo_kernel_times grows by exactly one per simulate on an S = 3 plan."""
    c = case("square")
    assert c.sh["S"] == 3 and c.launches_before == 0 and c.launches_after == 1
    n0 = len(c.batched.kernel_times(64))
    c.launch(c.batched, c.dev_x0)
    assert len(c.batched.kernel_times(64)) == n0 + 1
    assert all(t > 0 for t in c.batched.kernel_times(64))


def test_base_solve(gpu):
    """mrbo_base_solve: n = 5 starts on each of S = 3 base surrogates, xmin d×n×S, fmin/status n×S."""
    import torch
    from mrbo import _lib
    c = case("square")
    d, S, n = c.sh["d"], c.sh["S"], 5
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)

    def solve(plan, S_):
        xmin = torch.full((d * n * S_,), 7.0, dtype=torch.float64, device="cuda:0")
        fmin = torch.full((n * S_,), 7.0, dtype=torch.float64, device="cuda:0")
        status = torch.full((n * S_,), -1, dtype=torch.int32, device="cuda:0")
        evals = torch.full((_lib.NCOUNTERS * n * S_,), -1, dtype=torch.int64, device="cuda:0")
        _lib.check(plan.lib.mrbo_base_solve(plan.handle, n, p(c.dev_xs), p(xmin), p(fmin), p(status), p(evals), 0, st))
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (xmin, fmin, status, evals)]

    got = solve(c.batched, S)
    for q in c.compare:
        for name, g, r in zip(("xmin", "fmin", "status", "evals"), got, solve(c.plain[q], 1)):
            k = r.size
            assert same_bits(g[q * k:(q + 1) * k], r), f"surrogate {q}: {name} differs"
    assert not same_bits(got[1][:n], got[1][n:2 * n])

    # the Python mirror returns the same blocks
    from mrbo.rbf_optim import base_solve_batch, base_solve_multi
    xs, fs, ev = base_solve_multi(c.surs, c.lbs, c.ubs, c.xstarts[:, :n], [0.0])
    assert xs.shape == (d, n, S) and fs.shape == (n, S)
    for q in range(S):
        x1, f1, e1 = base_solve_batch(c.surs[q], c.lbs, c.ubs, c.xstarts[:, :n], [0.0])
        assert same_bits(xs[:, :, q], x1) and same_bits(fs[:, q], f1) and same_bits(ev[:, :, q], e1)


def test_eval_base(gpu):
    c = case("square")
    d, S, P = c.sh["d"], c.sh["S"], 7
    xs = c.xstarts[:, 3:3 + P]
    got = c.batched.eval_base(xs)
    assert got.shape == (3 + 4 * d + d * d, P, S)
    for q in c.compare:
        assert same_bits(np.ascontiguousarray(got[:, :, q]), np.ascontiguousarray(c.plain[q].eval_base(xs))), q
    assert not same_bits(np.ascontiguousarray(got[:, :, 0]), np.ascontiguousarray(got[:, :, 1]))


# ---- the outer ascent on the device --------------------------------------------------------------
SOLVE_ITERS = 12


def solve_starts(c):
    """Starts of the device ascent on shape 2: per surrogate one restart next to the incumbent (a
    large, well-resolved gradient: keeps iterating) and one Kronecker point of the box interior."""
    from mrbo.bayesopt import incumbent_start
    x0 = c.x0s.copy()
    for q, s in enumerate(c.surs):
        x0[:, 0, q] = incumbent_start(s, c.lbs, c.ubs)
    return x0


def stop_iterations(c, q, x0, optimizer, eta):
    """The baseline's stop iteration of every restart of surrogate q (0: never within the budget): the
    ascent of mrbo_stochastic_solve stepped from the host on the plain plan, one launch at a time."""
    import torch
    from mrbo.engine import to_device
    plan = c.plain[q]
    R, d = c.sh["R"], c.sh["d"]
    dx = to_device(x0[:, :, q], "cuda:0")
    act = torch.ones(R, dtype=torch.int32, device="cuda:0")
    m, v = torch.zeros(d * R, dtype=torch.float64, device="cuda:0"), torch.zeros(d * R, dtype=torch.float64,
                                                                                  device="cuda:0")
    stops = np.zeros(R, dtype=int)
    for it in range(1, SOLVE_ITERS + 1):
        out = plan.alloc_outputs()
        plan.simulate(dx, c.dev_in[0], c.dev_xs, out)
        e = plan.eto(out)
        if optimizer == "sga":
            plan.sga_step(e, dx, act, c.M, eta)
        else:
            plan.adam_step(e, dx, act, m, v, it, c.M, eta=eta)
        a = act.cpu().numpy()
        stops[(a == 0) & (stops == 0)] = it
    return stops, dx.cpu().numpy(), act.cpu().numpy()


@pytest.mark.parametrize("optimizer,eta", [("sga", 0.01), ("adam", 0.001)])
def test_device_stochastic_solve(gpu, optimizer, eta):
    """mrbo_stochastic_solve on shape 2, S = 2, 12 iterations: final x0s, ETO rows, active flags and
    the OR of the status bits equal the two plain plans' results.  The baseline's restarts stop at
    different iterations (asserted), so trajectories are skipped in the middle of the batch's
    launches -- in half-wave workgroups, whose two halves then hold one running and one skipped
    trajectory."""
    import torch
    from mrbo.engine import to_device
    c = case("half_c2")
    sh = c.sh
    d, R, S = sh["d"], sh["R"], sh["S"]
    W = 2 + 2 * d + 2
    x0 = solve_starts(c)

    def solve(plan, x0_, n):
        dx = to_device(x0_, "cuda:0")
        eto = torch.zeros(W * n, dtype=torch.float64, device="cuda:0")
        act = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
        res = plan.stochastic_solve(dx, c.dev_in[0], c.dev_xs, optimizer=optimizer, iterations=SOLVE_ITERS, eta=eta,
                                    eto=eto, active=act)
        return res, dx.cpu().numpy(), eto.cpu().numpy(), act.cpu().numpy()

    base = [solve(c.plain[q], x0[:, :, q], R) for q in range(S)]
    stops = np.concatenate([stop_iterations(c, q, x0, optimizer, eta)[0] for q in range(S)])
    print(f"{optimizer}: baseline stop iterations per (surrogate, restart): {stops.tolist()}")
    # restarts stop at different iterations, one of them strictly inside the budget
    assert len(set(stops.tolist())) > 1 and ((stops > 0) & (stops < SOLVE_ITERS)).any(), stops
    for q in range(S):     # the stepped baseline is the one-call baseline
        assert np.array_equal(base[q][3] != 0, stops[q * R:(q + 1) * R] == 0)
    res, gx, geto, gact = solve(c.batched, x0, R * S)
    for q in range(S):
        _, bx, beto, bact = base[q]
        assert same_bits(gx[q * d * R:(q + 1) * d * R], bx), f"surrogate {q}: final x0s differ"
        assert same_bits(geto[q * W * R:(q + 1) * W * R], beto), f"surrogate {q}: ETO rows differ"
        assert np.array_equal(gact[q * R:(q + 1) * R], bact), f"surrogate {q}: active differs"
    assert res[2] == functools.reduce(lambda a, b: a | b, (b_[0][2] for b_ in base))


def test_work_orders_are_unsupported(gpu):
    import torch
    from mrbo._lib import MrboError
    c = case("half_c2")
    T = c.sh["M"] * c.sh["R"]
    order = torch.arange(T, dtype=torch.int32, device="cuda:0")
    with pytest.raises(MrboError, match="mrbo error -2"):
        c.batched.set_order(order)
    out = c.batched.alloc_outputs()
    with pytest.raises(MrboError, match="mrbo error -2"):
        c.batched.order_longest_first(out)
    assert c.batched.lib.mrbo_plan_set_order(c.batched.handle, ctypes.c_void_p(order.data_ptr()), T) == -2
    c.assert_blocks_equal(c.launch(c.batched, c.dev_x0), "after the refused orders")


def test_multi_helper_returns_per_surrogate_results(gpu):
    """simulate_trajectory_mc_multi: per-surrogate BatchResults of one launch, each equal to
    simulate_trajectory_mc_batch on that surrogate."""
    from mrbo.rollout import simulate_trajectory_mc_batch, simulate_trajectory_mc_multi
    from mrbo.surrogates import FantasySurrogate
    from mrbo.trajectory import Trajectory, TrajectoryParameters
    c = case("half_c2")
    sh = c.sh
    tp = TrajectoryParameters(start=c.x0s[:, 0, 0], hypers=[0.0], horizon=sh["h"], mc_iterations=sh["M"],
                              use_low_discrepancy_sequence=True, spatial_lowerbounds=c.lbs, spatial_upperbounds=c.ubs)
    Ts = [Trajectory(s, FantasySurrogate(s, sh["h"]), start=c.x0s[:, 0, 0], hypers=[0.0], horizon=sh["h"])
          for s in c.surs]
    brs = simulate_trajectory_mc_multi(Ts, tp, c.x0s, c.xstarts, want_policy=True, want_obs=True)
    assert len(brs) == sh["S"]
    for q, br in enumerate(brs):
        one = simulate_trajectory_mc_batch(Ts[q], tp, c.x0s[:, :, q], c.xstarts, want_policy=True,
                                           want_obs=True).numpy()
        got = br.numpy()
        assert set(got) == set(one)
        for k, v in one.items():
            assert same_bits(np.ascontiguousarray(got[k]), np.ascontiguousarray(v)), (q, k)


# ---- the BO loops in lockstep --------------------------------------------------------------------
def _same_trials(a, b):
    assert set(a) == set(b)
    for key in a:
        for k in ("X", "y", "gaps", "minimum_observations"):
            assert same_bits(np.ascontiguousarray(a[key][k]), np.ascontiguousarray(b[key][k])), (key, k)


def test_bo_loop_in_lockstep(gpu, tmp_path):
    from mrbo import bayesopt
    kw = dict(horizon=1, budget=2, trials=3, mc_samples=16, batch_size=2, starts=4, sgd_iterations=3, rules=("ei",),
              reuse_surrogate=False, log=lambda *_: None)
    t0 = time.perf_counter()
    par = bayesopt.run("gramacylee", str(tmp_path / "par"), parallel_trials=3, **kw)
    t1 = time.perf_counter()
    seq = bayesopt.run("gramacylee", str(tmp_path / "seq"), parallel_trials=1, **kw)
    t2 = time.perf_counter()
    print(f"bayesopt.run wall time: parallel_trials=3 {t1 - t0:.3f} s, parallel_trials=1 {t2 - t1:.3f} s")
    assert len(par) == 3
    _same_trials(par, seq)
    for m in bayesopt.METRICS:
        if m != "times":
            assert (open(tmp_path / "par" / "gramacylee" / f"rollout_1_ei_{m}.csv").read() ==
                    open(tmp_path / "seq" / "gramacylee" / f"rollout_1_ei_{m}.csv").read())


def test_myopic_loop_in_lockstep(gpu, tmp_path):
    from mrbo import bayesopt
    kw = dict(budget=3, trials=3, starts=4, rules=("ei",), reuse_surrogate=False, log=lambda *_: None)
    t0 = time.perf_counter()
    par = bayesopt.run_myopic("gramacylee", str(tmp_path / "par"), parallel_trials=3, **kw)
    t1 = time.perf_counter()
    seq = bayesopt.run_myopic("gramacylee", str(tmp_path / "seq"), parallel_trials=1, **kw)
    t2 = time.perf_counter()
    print(f"bayesopt.run_myopic wall time: parallel_trials=3 {t1 - t0:.3f} s, parallel_trials=1 {t2 - t1:.3f} s")
    _same_trials(par, seq)
