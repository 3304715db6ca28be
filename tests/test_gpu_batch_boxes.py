"""Per-surrogate boxes in a surrogate batch on the device (mrbo_plan_create_batch_boxes, include/mrbo.h;
DESIGN.md §19).  The yardstick is inside the project, as in tests/test_gpu_surrogate_batch.py: block q
of every output of every call on a boxed plan must equal, BIT FOR BIT, the same call on a plain
mrbo_plan_create plan on surrogate q over box q with starts q -- float64 compared on their raw bits,
status and counters as integers.  No tolerance anywhere.

Inputs: box 0 is the test function's box, box q ≥ 1 a sub-box of it with its own offset and width
(SUB); surrogate q's observed points, its restarts and its inner starts initial_guesses(16, lbs_q,
ubs_q) are drawn in box q.  The shapes are those of tests/test_gpu_surrogate_batch.py (the smallest
that reach each kernel layout); every launch runs once per module and is shared."""
import ctypes
import functools

import numpy as np
import pytest

import conftest  # noqa: F401  (sys.path)
from test_gpu_surrogate_batch import ELLS, NSOBOL, SHAPES, make_surrogates, plan_opts, same_bits

pytestmark = pytest.mark.gpu

# box q in units of the test function's box: (offset, width) in every dimension; q = 0: all of it
SUB = ((0.0, 1.0), (0.30, 0.40), (0.05, 0.50))


def sub_boxes(lbs, ubs, S, sub=SUB):
    """d×S bounds: column 0 the box itself (its own bits), column q ≥ 1 the sub-box sub[q % len(sub)]."""
    w = ubs - lbs
    L = np.stack([lbs + sub[q % len(sub)][0] * w for q in range(S)], axis=1)
    U = np.stack([lbs + (sub[q % len(sub)][0] + sub[q % len(sub)][1]) * w for q in range(S)], axis=1)
    L[:, 0], U[:, 0] = lbs, ubs
    return L, U


def boxed_inputs(sh):
    """make_surrogates' construction with every surrogate's design, restarts and inner starts drawn in
    its own box: (surrogates, x0s d×R×S, L d×S, U d×S, xstarts d×ns×S)."""
    from mrbo import configs
    from mrbo.engine import initial_guesses
    from mrbo.kernels import Matern52, SquaredExponential
    from mrbo.surrogates import Surrogate
    from mrbo.utils import kronecker_quasirand
    surs0, _, lbs, ubs = make_surrogates(sh)     # rule, lengthscales and the function's box as that module has them
    kern = SquaredExponential if sh.get("kernel") == "se" else Matern52
    tf = configs.make_testfn(sh["fn"], sh["d"])
    L, U = sub_boxes(lbs, ubs, sh["S"])
    surs, x0s, xs = [], [], []
    for q, s0 in enumerate(surs0):
        lq, wq = L[:, q:q + 1], (U[:, q] - L[:, q])[:, None]
        X = lq + wq * kronecker_quasirand(sh["d"], sh["N"], 37 * q)
        surs.append(Surrogate(kern((ELLS[q % 3],)), X, tf(X), capacity=sh["N"],
                              decision_rule=s0.get_decision_rule(), σn2=1e-6))
        x0s.append(lq + wq * kronecker_quasirand(sh["d"], sh["R"], 37 * q + sh["N"]))
        xs.append(initial_guesses(NSOBOL, L[:, q].copy(), U[:, q].copy()))
    return surs, np.stack(x0s, axis=2), L, U, np.stack(xs, axis=2)


def plain_plan(s, h, M, R, ns, lbs, ubs, opts):
    from mrbo.engine import RolloutPlan
    n = s.observed
    return RolloutPlan(s.X[:, :n], s.L[:n, :n], s.c[:n], s.y[:n], s.ψ.kind, s.ψ.lengthscale, s.σn2, s.fmini(), h, M, R,
                       ns, np.ascontiguousarray(lbs), np.ascontiguousarray(ubs), 0.0, period=s.ψ.period, **opts)


class Case:
    """One shape: the boxed plan, one plain plan per surrogate on its own box, the shared-box batch on
    box 0, and the outputs of one launch on each (host copies).  mode: "mc", "ghq" or "control"."""

    def __init__(self, name, mode="mc"):
        import torch
        from mrbo.engine import RolloutPlan, rnstream, to_device
        from mrbo.rollout import surrogate_dict
        sh = self.sh = SHAPES[name]
        self.mode = mode
        self.surs, self.x0s, self.L, self.U, self.xstarts = boxed_inputs(sh)
        S, d, h, M, R = sh["S"], sh["d"], sh["h"], sh["M"], sh["R"]
        if mode == "control":
            # The control sample is max(fmini − y0, 0) with y0 drawn at x0: it is 0 in every sample at the
            # design's restarts, and still 1e-2 box widths from the best observed point (incumbent_start:
            # u = (fmini − μ)/σ between −3 and −10 on these surrogates, by the CPU oracle).  Restart 0 goes
            # 1e-5 widths from it, where σ is at its noise floor and u ≈ −0.1: about half the samples improve
            for q, s in enumerate(self.surs):
                xb = s.get_active_covariates()[:, int(np.argmin(s.get_active_observations()))]
                lq, uq = self.L[:, q], self.U[:, q]
                self.x0s[:, 0, q] = np.clip(xb + np.where(xb <= 0.5 * (lq + uq), 1.0, -1.0) * 1e-5 * (uq - lq), lq, uq)
        ns = self.ns = self.xstarts.shape[1]
        self.opts = plan_opts(sh, self.surs)
        self.dicts = [surrogate_dict(s) for s in self.surs]
        if mode == "ghq":
            from mrbo.rollout import ghq_node_arrays
            from mrbo.utils import gauss_hermite, generate_indices
            nodes, weights = gauss_hermite(3)
            tn, tw = ghq_node_arrays(nodes, weights, generate_indices(3, h + 1))
            M = tn.shape[0]
        self.M = M
        make = lambda lb, ub: RolloutPlan.from_surrogates(self.dicts, h, M, R, ns, lb, ub, 0.0, **self.opts)
        self.boxed = make(self.L, self.U)
        self.shared0 = make(self.L[:, 0].copy(), self.U[:, 0].copy())
        self.plain = [plain_plan(s, h, M, R, ns, self.L[:, q], self.U[:, q], self.opts)
                      for q, s in enumerate(self.surs)]
        dev = "cuda:0"
        self.dev_in = (to_device(tn, dev), to_device(tw, dev)) if mode == "ghq" else (to_device(rnstream(M, d, h + 1), dev),)
        self.dev_x0 = to_device(self.x0s, dev)
        self.dev_xs = to_device(self.xstarts, dev)
        self.dev_xs_q = [to_device(self.xstarts[:, :, q], dev) for q in range(S)]
        self.out = self.launch(self.boxed, self.dev_x0, self.dev_xs)
        self.ref = [self.launch(self.plain[q], to_device(self.x0s[:, :, q], dev), self.dev_xs_q[q]) for q in range(S)]
        # every surrogate on box 0 with starts 0: what the batch computed before it had boxes
        self.out0 = self.launch(self.shared0, self.dev_x0, self.dev_xs_q[0])
        torch.cuda.synchronize()

    def launch(self, plan, dx0, dxs):
        import torch
        if self.mode == "control":
            out = plan.simulate_control(dx0, self.dev_in[0], dxs)
        else:
            out = plan.alloc_outputs(with_gradient=True, want_policy=True, want_obs=True, want_evals=True)
            if self.mode == "ghq":
                plan.simulate_ghq(dx0, self.dev_in[0], self.dev_in[1], dxs, out)
            else:
                plan.simulate(dx0, self.dev_in[0], dxs, out)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    def block(self, out, k, q):
        n = out[k].size // self.sh["S"]
        return out[k][q * n:(q + 1) * n]

    def assert_blocks_equal(self, out=None, label=""):
        out = self.out if out is None else out
        for q, ref in enumerate(self.ref):
            assert set(ref) == set(out)
            for k, v in ref.items():
                assert same_bits(self.block(out, k, q), v), f"{label} surrogate {q}: output {k} differs"

    def box_acts(self):
        """The surrogates q ≥ 1 whose block differs in bits from the one computed on box 0 with starts 0,
        and those with a policy point on a face of their own box."""
        sh = self.sh
        differ, on_face = [], []
        for q in range(1, sh["S"]):
            if not same_bits(self.block(self.out, "policy_x", q), self.block(self.out0, "policy_x", q)):
                differ.append(q)
            pol = self.block(self.out, "policy_x", q).reshape((sh["d"], sh["h"] + 1, -1), order="F")[:, 1:, :]
            if ((pol == self.L[:, q][:, None, None]) | (pol == self.U[:, q][:, None, None])).any():
                on_face.append(q)
        return differ, on_face


@functools.lru_cache(maxsize=None)
def case(name, mode="mc"):
    return Case(name, mode)


OUTPUTS = {"values", "grad_x", "grad_theta", "status", "policy_x", "obs", "evals"}


# ---- 1: blocks equal plain plans --------------------------------------------------------------------
@pytest.mark.parametrize("name", ["half_odd", "half_c2", "square", "packed", "generic", "cost"])
def test_blocks_equal_plain_plans_on_their_boxes(gpu, name):
    c = case(name)
    sh = c.sh
    info = c.boxed.info()
    assert info["S"] == sh["S"] and c.boxed.boxed
    for p in c.plain:
        pi = p.info()
        assert {k: v for k, v in pi.items() if k != "S"} == {k: v for k, v in info.items() if k != "S"}
    assert info == c.shared0.info()           # mrbo_plan_info does not tell a boxed plan from a shared box
    for key in ("spec", "batch", "rpl"):
        if key in sh:
            assert info[key] == sh[key]
    assert set(c.out) == OUTPUTS
    assert (c.out["status"] == 0).all(), c.out["status"]
    assert all((r["status"] == 0).all() for r in c.ref)
    c.assert_blocks_equal(label=name)
    # surrogate 0 has box 0 and starts 0 on both plans: its block is the shared-box batch's
    for k in OUTPUTS:
        assert same_bits(c.block(c.out, k, 0), c.block(c.out0, k, 0)), k
    # not vacuous: the box acts -- some block q ≥ 1 differs from the one computed on box 0 with starts 0,
    # and policy points of some q ≥ 1 sit on a face of box q
    differ, on_face = c.box_acts()
    print(f"{name}: blocks that differ from the box-0 launch {differ}, with policy points on a face {on_face}")
    assert differ and on_face, (differ, on_face)
    bl, bu = c.boxed.boxes
    assert same_bits(bl, np.asfortranarray(c.L)) and same_bits(bu, np.asfortranarray(c.U))


# ---- 2: the other estimators ------------------------------------------------------------------------
def test_ghq(gpu):
    c = case("half_c2", "ghq")
    assert c.M == 3 ** (c.sh["h"] + 1) and (c.out["status"] == 0).all()
    c.assert_blocks_equal(label="ghq")
    differ, _ = c.box_acts()
    assert differ


def test_control(gpu):
    """simulate_control: the launch at horizon 0.  It has no inner solve, so no box acts on it: the
    comparison shows that the boxed plan's control launch addresses its blocks as the plain plans do."""
    c = case("square", "control")
    assert set(c.out) == {"values0", "status0", "grad_x0"} and (c.out["status0"] == 0).all()
    v0 = c.out["values0"].reshape(c.sh["S"], -1)
    assert all((v0[q] != 0).any() for q in range(c.sh["S"])) and not same_bits(v0[0], v0[1])
    c.assert_blocks_equal(label="control")


# ---- 3: base solve -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["half_c2", "square"])
def test_base_solve(gpu, name):
    """mrbo_base_solve with d×n×S starts: n = 5 starts of its own, in its own box, per surrogate."""
    import torch
    from mrbo import _lib
    from mrbo.engine import to_device
    c = case(name)
    d, S, n = c.sh["d"], c.sh["S"], 5
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)
    guesses = np.ascontiguousarray(c.xstarts[:, -n:, :])      # the last Sobol points and the two near-bound points

    def solve(plan, xs, S_):
        c_xs = to_device(xs, "cuda:0")
        xmin = torch.full((d * n * S_,), 7.0, dtype=torch.float64, device="cuda:0")
        fmin = torch.full((n * S_,), 7.0, dtype=torch.float64, device="cuda:0")
        status = torch.full((n * S_,), -1, dtype=torch.int32, device="cuda:0")
        evals = torch.full((_lib.NCOUNTERS * n * S_,), -1, dtype=torch.int64, device="cuda:0")
        _lib.check(plan.lib.mrbo_base_solve(plan.handle, n, p(c_xs), p(xmin), p(fmin), p(status), p(evals), 0, st))
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in (xmin, fmin, status, evals)]

    got = solve(c.boxed, guesses, S)
    assert (got[2] == 0).all()
    for q in range(S):
        for label, g, r in zip(("xmin", "fmin", "status", "evals"), got, solve(c.plain[q], guesses[:, :, q], 1)):
            k = r.size
            assert same_bits(g[q * k:(q + 1) * k], r), f"surrogate {q}: {label} differs"
    # the box acts: surrogate 1 from its own starts on box 0 ends elsewhere (in bits)
    on0 = solve(plain_plan(c.surs[1], c.sh["h"], c.M, c.sh["R"], c.ns, c.L[:, 0], c.U[:, 0], c.opts),
                guesses[:, :, 1], 1)
    assert not same_bits(on0[0], got[0][d * n:2 * d * n])
    # the Python mirror returns the same blocks
    from mrbo.rbf_optim import base_solve_batch, base_solve_multi
    xs, fs, ev = base_solve_multi(c.surs, c.L, c.U, guesses, [0.0])
    assert xs.shape == (d, n, S) and fs.shape == (n, S)
    assert same_bits(xs.ravel(order="F"), got[0]) and same_bits(fs.ravel(order="F"), got[1])
    for q in range(S):
        x1, f1, e1 = base_solve_batch(c.surs[q], c.L[:, q].copy(), c.U[:, q].copy(), guesses[:, :, q], [0.0])
        assert same_bits(xs[:, :, q], x1) and same_bits(fs[:, q], f1) and same_bits(ev[:, :, q], e1)


# ---- 4: equal boxes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["square", "packed"])
def test_equal_boxes_are_the_shared_box_batch(gpu, name):
    from mrbo.engine import RolloutPlan, to_device
    c = case(name)
    sh = c.sh
    S = sh["S"]
    rep = lambda a: np.tile(a[:, None], (1, S))
    eq = RolloutPlan.from_surrogates(c.dicts, sh["h"], c.M, sh["R"], c.ns, rep(c.L[:, 0]), rep(c.U[:, 0]), 0.0, **c.opts)
    assert eq.boxed
    xs = np.repeat(c.xstarts[:, :, 0:1], S, axis=2)
    out = c.launch(eq, c.dev_x0, to_device(xs, "cuda:0"))
    assert set(out) == OUTPUTS
    for k, v in c.out0.items():
        assert same_bits(out[k], v), k


def test_one_surrogate_on_its_own_box_is_the_plain_plan(gpu):
    from mrbo.engine import RolloutPlan, to_device
    c = case("square")
    sh = c.sh
    one = RolloutPlan.from_surrogates([c.dicts[1]], sh["h"], c.M, sh["R"], c.ns, c.L[:, 1:2], c.U[:, 1:2], 0.0, **c.opts)
    assert one.S == 1 and not one.boxed and one.info() == c.plain[1].info()
    out = c.launch(one, to_device(c.x0s[:, :, 1], "cuda:0"), c.dev_xs_q[1])
    for k, v in c.ref[1].items():
        assert same_bits(out[k], v), k


# ---- 5: the step, the projection, the pick ----------------------------------------------------------------
class _Mean:
    def __init__(self, v):
        self.v = v

    def mean(self):
        return self.v


@functools.lru_cache(maxsize=None)
def narrow():
    """d = 2, N = 5, S = 2 on Branin: box 0 the function's, box 1 a tenth of its width around its centre."""
    from mrbo import configs
    from mrbo.kernels import Matern52
    from mrbo.surrogates import Surrogate
    from mrbo.utils import kronecker_quasirand
    tf = configs.make_testfn("braninhoo", 2)
    lbs, ubs = tf.get_bounds()
    L, U = sub_boxes(lbs, ubs, 2, sub=((0.0, 1.0), (0.45, 0.10)))
    surs = []
    for q in range(2):
        X = L[:, q:q + 1] + (U[:, q] - L[:, q])[:, None] * kronecker_quasirand(2, 5, 37 * q)
        surs.append(Surrogate(Matern52((ELLS[q],)), X, tf(X), capacity=5, σn2=1e-6))
    return surs, L, U


def narrow_plan(h, M, R, ns):
    from mrbo.engine import RolloutPlan
    from mrbo.rollout import surrogate_dict
    surs, L, U = narrow()
    g = surs[0].get_decision_rule()
    return RolloutPlan.from_surrogates([surrogate_dict(s) for s in surs], h, M, R, ns, L, U, 0.0, rule=g.rule_id,
                                       sigma_tol=g.σtol)


def test_box_adam_step_uses_the_surrogates_box(gpu):
    """tests/test_gpu_rollout_solve.py's step test on R = 6 restarts per surrogate, S = 2: restart r of
    surrogate q against BoxAdam(lbs_q, ubs_q).update, three steps, no rollout launch.  Restart 5 gets a
    NaN gradient component; 3 and 4 are thrown over a face of their own box."""
    torch = gpu
    from mrbo.bayesopt import BoxAdam
    from mrbo.engine import to_device
    from mrbo.trajectory import ExpectedTrajectoryOutput
    from mrbo.utils import eswavs
    d, R, S, M, eta = 2, 6, 2, 16, 0.02
    surs, L, U = narrow()
    plan = narrow_plan(0, M, R, 4)
    W = 2 + 2 * d + 2
    u = np.array([[0.4, 0.27], [0.5, 0.5], [0.27, 0.73], [0.007, 0.007], [0.993, 0.993], [0.53, 0.2]]).T    # d×R in the unit box
    x = np.stack([L[:, q:q + 1] + (U[:, q] - L[:, q])[:, None] * u for q in range(S)], axis=2)               # d×R×S
    nan = np.nan
    grads = [[(0.3, -0.2), (0.0, 0.0), (1.0, 1.0), (-50.0, -60.0), (50.0, 70.0), (nan, 0.1)],
             [(0.1, 0.25), (0.0, 0.0), (1e-3, 1e-3), (-40.0, 1.0), (45.0, -2.0), (0.2, 0.1)],
             [(-0.2, 0.15), (0.0, 0.0), (30.0, 30.0), (2.0, -1.0), (-1.0, 3.0), (0.2, nan)]]
    stds = [(0.05, 0.04), (0.0, 0.0), (1.0, 1.0), (1.0, 2.0), (2.0, 1.0), (0.01, 0.01)]
    etos = np.zeros((3, S, R, W))
    for t in range(3):
        for q in range(S):
            for r in range(R):
                etos[t, q, r, 0:2] = (0.1 * r, 0.01)
                etos[t, q, r, 2:2 + d] = np.array(grads[t][r]) * (1.0 + 0.5 * q)
                etos[t, q, r, 2 + d:2 + 2 * d] = stds[r]
    hx, hx0 = x.copy(), x.copy()
    opts = [[BoxAdam(L[:, q], U[:, q], η=eta) for _ in range(R)] for q in range(S)]
    opts0 = [[BoxAdam(L[:, 0], U[:, 0], η=eta) for _ in range(R)] for q in range(S)]      # every restart on box 0
    hact = np.ones((R, S), dtype=np.int32)
    dx = to_device(x, "cuda:0")
    dact = torch.ones(R * S, dtype=torch.int32, device="cuda:0")
    dm = torch.zeros(d * R * S, dtype=torch.float64, device="cuda:0")
    dv = torch.zeros(d * R * S, dtype=torch.float64, device="cuda:0")
    for t in range(3):
        with np.errstate(all="ignore"):
            for q in range(S):
                for r in range(R):
                    if not hact[r, q]:
                        continue
                    e = ExpectedTrajectoryOutput.from_row(etos[t, q, r], d)
                    if eswavs(e.gradient(), e.std_gradient() ** 2, M):
                        hact[r, q] = 0
                        continue
                    opts[q][r].update(hx[:, r, q], e.gradient())
                    opts0[q][r].update(hx0[:, r, q], e.gradient())
        plan.box_adam_step(torch.from_numpy(etos[t].ravel()).to("cuda:0"), dx, dact, dm, dv, t + 1, M, eta=eta)
        gx = dx.cpu().numpy().reshape((d, R, S), order="F")
        gm = dm.cpu().numpy().reshape((d, R, S), order="F")
        gv = dv.cpu().numpy().reshape((d, R, S), order="F")
        hm = np.stack([np.stack([o.adam.m[-1] if o.adam.m else np.zeros(d) for o in oq], axis=1) for oq in opts], axis=2)
        hv = np.stack([np.stack([o.adam.v[-1] if o.adam.v else np.zeros(d) for o in oq], axis=1) for oq in opts], axis=2)
        assert np.array_equal(dact.cpu().numpy().reshape((R, S), order="F"), hact), t
        assert same_bits(gx, hx), (t, gx, hx)
        assert same_bits(gm, hm) and same_bits(gv, hv), t
    assert hact[:, 0].tolist() == [1, 1, 0, 1, 1, 1] and hact[:, 1].tolist() == [1, 1, 0, 1, 1, 1]
    for q in range(S):
        assert (hx[:, 3, q] == L[:, q]).all() and (hx[:, 4, q] == U[:, q]).all()
        assert np.isnan(hx[:, 5, q]).all() and np.isfinite(hx[:, :5, q]).all()
    # the box acts: surrogate 1's restarts stepped over box 0 end elsewhere, surrogate 0's do not
    assert same_bits(hx0[:, :, 0], hx[:, :, 0]) and not same_bits(hx0[:, :5, 1], hx[:, :5, 1])
    assert len(plan.kernel_times(64)) == 0          # no rollout launch


def test_pick_restart_uses_the_surrogates_box(gpu):
    """R = 3, S = 2, crafted points and means.  Surrogate 0: restart 0 has a NaN coordinate and the best
    mean (never novel), restart 2 sits 5e-9 of box 0's width from an observed point (novel), restart 1
    is far from all.  Surrogate 1 (box 1: a tenth of box 0's width): restart 1 has the best mean and
    sits 5e-10 of box 0's width from an observed point -- 5e-9 of its own box's, so the novelty
    threshold 1e-9 falls on opposite sides under the two widths (the distance is a tenth of the 5e-9
    one might first write down: at 5e-9 of box 0's width both widths call the restart novel)."""
    torch = gpu
    from mrbo.bayesopt import pick_restart
    from mrbo.engine import to_device
    d, R, S = 2, 3, 2
    surs, L, U = narrow()
    plan = narrow_plan(0, 4, R, 4)
    W = 2 + 2 * d + 2
    X = [s.get_active_covariates() for s in surs]
    w0 = U[:, 0] - L[:, 0]
    mid = lambda q, k: L[:, q] + (0.31 + 0.07 * k) * (U[:, q] - L[:, q])
    x = np.stack([np.stack([np.array([np.nan, mid(0, 0)[1]]), mid(0, 1), X[0][:, 2] + 5e-9 * w0], axis=1),
                  np.stack([X[1][:, 0], X[1][:, 3] + 5e-10 * w0, mid(1, 2)], axis=1)], axis=2)          # d×R×S
    means = [[9.0, 1.0, 3.0], [1.0, 5.0, 2.0]]
    eto = np.zeros((S, R, W))
    eto[:, :, 0] = np.array(means)
    dx, deto = to_device(x, "cuda:0"), torch.from_numpy(eto.ravel()).to("cuda:0")
    dmeans = torch.zeros(R * S, dtype=torch.float64, device="cuda:0")
    xnext, mean, pick = plan.pick_restart(dx, deto, incumbent=True, means=dmeans)
    torch.cuda.synchronize()
    gx = xnext.cpu().numpy().reshape((d, S), order="F")
    own, on_box0 = [], []
    for q in range(S):
        with np.errstate(all="ignore"):
            k, hmeans = pick_restart(surs[q], x[:, :, q], [_Mean(v) for v in means[q]], L[:, q], U[:, q], True)
            k0, _ = pick_restart(surs[q], x[:, :, q], [_Mean(v) for v in means[q]], L[:, 0], U[:, 0], True)
        own.append(k)
        on_box0.append(k0)
        assert int(pick[q]) == k, (q, int(pick[q]), k)
        assert same_bits(dmeans.cpu().numpy()[q * R:(q + 1) * R], hmeans), q
        assert same_bits(gx[:, q], x[:, k, q]), q
        assert same_bits(mean.cpu().numpy()[q:q + 1], np.array([float(hmeans[k])])), q
    assert own == [2, 1] and on_box0 == [2, 2], (own, on_box0)      # the picks differ from those computed with box 0
    xn, _, pk = plan.pick_restart(dx, deto, incumbent=False)
    torch.cuda.synchronize()
    assert pk.cpu().numpy().tolist() == [0, 1]


def test_projection_uses_the_surrogates_box(gpu):
    """The projection inside mrbo_rollout_solve against np.clip per surrogate: one StandardSGA iteration
    with η = 0 leaves x0 where it is (x + 0·∇ = x), so the returned end points are the projected starts.
    The starts lie outside box 1 on every side and inside box 0 (x0 takes no part in a launch's
    addressing: a point outside the box is evaluated like any other).  NaN coordinates go through the
    same clip in test_box_adam_step_uses_the_surrogates_box; none is fed to a rollout launch here."""
    from mrbo.engine import initial_guesses, rnstream
    d, R, S, M, h = 2, 4, 2, 4, 0
    surs, L, U = narrow()
    xs = np.stack([initial_guesses(2, L[:, q].copy(), U[:, q].copy()) for q in range(S)], axis=2)
    plan = narrow_plan(h, M, R, xs.shape[1])
    u = np.array([[0.2, 0.5], [0.5, 0.9], [0.8, 0.1], [0.5, 0.52]]).T                 # d×R in box 0's unit box
    x0 = np.repeat((L[:, 0:1] + (U[:, 0] - L[:, 0])[:, None] * u)[:, :, None], S, axis=2)
    r = plan.rollout_solve_host(x0, rnstream(M, d, h + 1), xs, optimizer="sga", iterations=1, eta=0.0)
    want = np.clip(x0, L[:, None, :], U[:, None, :])
    assert same_bits(np.ascontiguousarray(r["x"]), np.ascontiguousarray(want)), (r["x"], want)
    assert same_bits(want[:, :, 0], x0[:, :, 0]) and not same_bits(want[:, :3, 1], x0[:, :3, 1])
    assert same_bits(want[:, 3, 1], x0[:, 3, 1])           # the start inside box 1 stays
    assert not same_bits(np.clip(x0, L[:, None, 0:1], U[:, None, 0:1]), want)


# ---- 6: the acquisition solve -------------------------------------------------------------------------------
ITERS = 12
SOLVE = dict(fn="braninhoo", d=2, N=20, h=1, M=16, R=5, S=3)
ETA = {"sga": 0.1, "adam": 0.02}      # sga: 0.01 leaves every stop at iteration 1 or never (CPU oracle)


@functools.lru_cache(maxsize=None)
def solve_surrogates():
    surs, _, L, U, _ = boxed_inputs(dict(SOLVE))
    return surs, L, U


@functools.lru_cache(maxsize=None)
def solved(solver, vr, device_solve, q=None):
    """(picks, trace entry) of the acquisition solve: all S surrogates on a boxed plan, or surrogate q
    alone through rollout_solve on its own box."""
    from mrbo import bayesopt
    surs, L, U = solve_surrogates()
    trace = []
    kw = dict(eta=ETA[solver], solver=solver, incumbent=True, trace=trace, device_solve=device_solve,
              variance_reduction=vr)
    args = (SOLVE["h"], SOLVE["M"], SOLVE["R"] - 3, 2, ITERS, 0.0)     # generate_batch: R − 3 + 2 points, + the incumbent's
    if q is None:
        return bayesopt.rollout_solve_multi(surs, L, U, *args, **kw), trace[0]
    return [bayesopt.rollout_solve(surs[q], L[:, q].copy(), U[:, q].copy(), *args, **kw)], trace[0]


def stop_iterations(history, M):
    """From a host loop's history: the iteration at which eswavs stops every restart (0: never), R×S."""
    from mrbo.utils import eswavs
    S, R = len(history[0]), len(history[0][0])
    stops = np.zeros((R, S), dtype=int)
    for i, per_sur in enumerate(history):
        for q in range(S):
            for r in range(R):
                e = per_sur[q][r]
                if stops[r, q] == 0 and eswavs(e.gradient(), e.std_gradient() ** 2, M):
                    stops[r, q] = i + 1
    return stops


@pytest.mark.parametrize("solver,vr", [("sga", False), ("adam", False), ("adam", True)],
                         ids=["sga", "box_adam", "box_adam-variance_reduction"])
def test_rollout_solve_on_a_boxed_plan(gpu, solver, vr):
    """mrbo_rollout_solve on the boxed plan (device_solve=True) equals the host-driven
    rollout_solve_multi with (d, S) bounds and, per surrogate, rollout_solve on its own box."""
    S, R = SOLVE["S"], SOLVE["R"]
    (pd, td), (ph, th) = solved(solver, vr, True), solved(solver, vr, False)
    assert td["batch"].shape == (SOLVE["d"], R, S)
    stops = stop_iterations(th["history"], SOLVE["M"])
    print(f"{solver} vr={vr}: stop iterations (restart × surrogate)\n{stops}\ndevice result {td['result']}")
    # restarts stop at different iterations, one of them strictly inside the budget
    assert len(set(stops.ravel().tolist())) > 1 and ((stops > 0) & (stops < ITERS)).any(), stops
    assert td["result"][2] == 0 and td["result"][3] == 0, td["result"]
    for (xa, ma), (xb, mb) in zip(pd, ph):
        assert same_bits(xa, xb) and same_bits(np.array([ma]), np.array([mb]))
    assert same_bits(np.ascontiguousarray(td["x"]), np.ascontiguousarray(th["x"]))
    assert same_bits(np.ascontiguousarray(td["means"]), np.ascontiguousarray(th["means"]))
    assert [int(k) for k in td["pick"]] == [int(k) for k in th["pick"]]
    surs, L, U = solve_surrogates()
    for q in range(S):
        (p1,), t1 = solved(solver, vr, True, q)
        assert same_bits(pd[q][0], p1[0]) and same_bits(np.array([pd[q][1]]), np.array([p1[1]])), q
        assert same_bits(np.ascontiguousarray(td["batch"][:, :, q]), np.ascontiguousarray(t1["batch"])), q
        assert same_bits(np.ascontiguousarray(td["x"][:, :, q]), np.ascontiguousarray(t1["x"])), q
        assert same_bits(np.ascontiguousarray(td["means"][:, q]), np.ascontiguousarray(t1["means"])), q
        assert int(td["pick"][q]) == int(t1["pick"]), q
        assert (td["x"][:, :, q] >= L[:, q:q + 1]).all() and (td["x"][:, :, q] <= U[:, q:q + 1]).all()
    # the boxes differ, and so do the batches drawn in them
    assert not same_bits(np.ascontiguousarray(td["batch"][:, :, 0]), np.ascontiguousarray(td["batch"][:, :, 1]))


# ---- 7: the BO loops --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bo_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("batch_boxes_bo"))


def _spied(fn):
    """fn() with RolloutPlan.from_surrogates watched: (result, the S of every plan it created)."""
    from mrbo import rollout
    from mrbo.engine import RolloutPlan
    created = []
    orig = RolloutPlan.from_surrogates.__func__

    def spy(cls, surrogates, *a, **kw):
        surrogates = list(surrogates)
        created.append((len(surrogates), np.shape(a[4])))
        return orig(cls, surrogates, *a, **kw)

    rollout._PLANS.clear()            # no plan of an earlier run is handed out: every plan is created here
    RolloutPlan.from_surrogates = classmethod(spy)
    try:
        return fn(), created
    finally:
        RolloutPlan.from_surrogates = classmethod(orig)


def _same(a, b, label):
    assert set(a) == set(b)
    for key in a:
        for k in ("X", "y", "ells"):
            assert same_bits(a[key][k], b[key][k]), (label, key, k, a[key][k], b[key][k])


def test_run_with_ard_in_lockstep_is_one_solve_per_chunk(gpu, bo_dir):
    from mrbo import bayesopt
    from test_gpu_ard import RUN_KW
    run = lambda tag, **kw: bayesopt.run("braninhoo", f"{bo_dir}/{tag}", **{**RUN_KW, **kw})
    seq = run("seq", parallel_trials=1)
    lock, created = _spied(lambda: run("lock", parallel_trials=2))
    # every plan of the lockstep loop serves both trials, each on its own whitened box
    assert created and all(S == 2 and shape == (2, 2) for S, shape in created), created
    _same(lock, seq, "lockstep")
    assert any(r["ells"][0] != r["ells"][1] for r in seq.values())
    dev, created = _spied(lambda: run("lockdev", parallel_trials=2, device_solve=True))
    assert created and all(S == 2 for S, _ in created), created
    _same(dev, seq, "lockstep + device_solve")
    seq_vr = run("seqvr", parallel_trials=1, variance_reduction=True)
    lock_vr, created = _spied(lambda: run("lockvr", parallel_trials=2, variance_reduction=True))
    assert created and all(S == 2 for S, _ in created), created
    _same(lock_vr, seq_vr, "lockstep + variance_reduction")
    _same(run("lockdevvr", parallel_trials=2, device_solve=True, variance_reduction=True), seq_vr,
          "lockstep + device_solve + variance_reduction")


def test_run_myopic_with_ard_in_lockstep_is_one_solve_per_chunk(gpu, bo_dir):
    from mrbo import bayesopt
    from test_gpu_ard import MYOPIC_KW
    run = lambda tag, **kw: bayesopt.run_myopic("braninhoo", f"{bo_dir}/{tag}", **{**MYOPIC_KW, **kw})
    seq = run("mseq", parallel_trials=1)
    lock, created = _spied(lambda: run("mlock", parallel_trials=2))
    assert created and all(S == 2 and shape == (2, 2) for S, shape in created), created
    _same(lock, seq, "myopic lockstep")
