"""The rollout's per-trajectory failure statuses (include/mrbo.h MRBO_ST_*) on the GPU against the
oracle, on every kernel layout, and the entry points above the kernel on failing launches.

Inputs: tests/failure_inputs.py (five recipes, one per status bit; the layouts of CASES, each
asserted through plan.info()); tests/test_failure_paths.py holds, on the oracle alone, the
conditions that make these comparisons meaningful.  Per layout × recipe, one GPU launch with policy
points, observations and counters, its policy buffer filled with NaN beforehand, and:

 a. Status.  T2: the oracle replays the GPU's policy points -- as many as the GPU wrote: a trajectory
    that wrote w of its h + 1 policy columns is replayed to horizon w − 1 -- on its two builds;
    where the builds agree (they may disagree on max(1, 1 %) trajectories), the GPU's status is the
    replay's.  A replay cannot fail inside the inner solve (it has none): a trajectory that wrote
    w ≤ h columns and whose replay to w − 1 finishes failed in the solve of step w (bit 8, or
    bit 1 at a Newton iterate), and its status is held to T3 -- the oracle's own Newton solves --
    wherever the paths agree to 1e-6; at most max(1, 1 %) trajectories may be out of both checks.
    T3, on identical paths (every written policy column within 1e-12 relative): the same number of
    written columns, the same status, the same Newton counters -- the only record of the step at
    which a trajectory stopped (equal where the recipe leaves the acquisition surface alone; under
    parity.py's rule for rounding-sensitive surfaces where it puts a σ² = 0 boundary in the box:
    see the comment at the assertion).
 b. Non-vacuity on the GPU's own status array: the conditions of failure_inputs.conditions, no
    status value outside the recipe's list, and a last-step failure on the h = 3 twins.
 c. Failed trajectories: NaN value, ∇x, ∇θ; NaN observations and zero adjoint counters for a
    failure in the step loop (bits 1, 2, 4, 8); bit 16 comes from the adjoint itself, after the
    observations were written, so they stay and the adjoint counters hold ≥ 1 rich evaluation
    (mrbo.h, "Failed trajectories"); policy columns after the last step keep the caller's bytes
    (a second launch over a finite filler leaves exactly the filler there, and every other output
    bit for bit); the restart's ETO row is NaN exactly where the oracle's is.
 d. Finished trajectories of the same launch: the unchanged T2 bounds (parity._replay_t2), and
    bit for bit -- every output -- the same trajectories of a launch of the same plan in which no
    trajectory of their restart fails: the failing samples' Sobol rows (node rows) replaced by a
    finishing sample's; and, since the waves take trajectories of any restart from shared queues,
    of one more launch in which nothing fails in any restart (every sample that fails somewhere
    replaced by one that finishes everywhere, where the launch has such a sample).  No tolerance:
    this is what catches a half-wave partner or a workgroup neighbour disturbed by an early exit.
 e. Surrogate batch (S = 3, the middle surrogate with the scaled factor): every block bit for bit
    its own plain plan's.

Then the entry points above the kernel (d = 2, N = 12, ≤ 6 iterations): mrbo_stochastic_solve's
stop on a status bit, mrbo_rollout_solve's collected bits on both drivers with and without the
control variate, mrbo_simulate_control / mrbo_eto_reduce_cv on a failing control, mrbo_base_solve.

Left out: the eight-row layout (N = 512), for time.  Dropped recipe × layout pairs
(failure_inputs.DROPPED, each with its reason): the singular adjoint on four_rows_d3_n150 (both
h) and cost_kernel_d3_n70_h4 -- fewer than 10 % of the trajectories reach the adjoint's solve;
negative noise on poi_d2_n12_h3 and cost_generic_d2_n12 -- no sigma_n2 in the range where the
oracle's builds agree leaves ≥ 10 % of both kinds; the scaled factor on two_rows_d4_n96_h2 --
between "9 % fail" and "every trajectory fails at step 0" there is no scale (its h = 3 twin holds
it).  The quadratic cost at d = 2, N = 12 runs the generic kernel with the cost weighting; the
compile-time cost kernel needs N = 65..256 and h ≥ 4, so cost_kernel_d3_n70_h4 stands for it.  At
four_rows_d3_n150 negative noise surfaces as bit 2.
"""
import os

import numpy as np
import pytest

import failure_inputs as F
from conftest import ROOT, load_golden
from parity import MAX_LS, WORK_STEPS, _replay_t2

pytestmark = pytest.mark.gpu

ORACLE_FAST = os.path.join(ROOT, "oracle", "build", "librbo_oracle_fast.so")
OUTPUTS = ("values", "grad_x", "grad_theta", "obs", "policy_x", "evals", "status")


@pytest.fixture(scope="module")
def golden_c2():
    return load_golden("c2")


def make_plan(case, g, opts, R=None, **extra):
    from mrbo.engine import RolloutPlan
    o = {k: opts[k] for k in ("htol", "sigma_tol") if k in opts}
    if case.cost:
        kind, c0, w = case.cost_model()
        o.update(cost=kind, cost_c0=c0, cost_w=tuple(w))
    o.update(extra)
    M = g["ghq"][0].shape[0] if case.ghq else g["rnstream"].shape[0]
    return RolloutPlan(g["X"], g["L"], g["c"], g["y"], F.KERNEL_IDS[case.kernel], float(g["ell"]),
                       opts.get("sigma_n2", 1e-6), float(g["fmini"]), case.h, M, R or g["x0s"].shape[1],
                       g["xstarts"].shape[1], g["lbs"], g["ubs"], 0.0, rule=F.RULE_IDS[case.rule], **o)


SENTINEL = -12345.6789      # a finite filler no policy point of these boxes can equal


def launch(plan, g, ghq=None, rn=None, x0s=None, with_gradient=True, fill=float("nan")):
    """one launch; the policy buffer holds `fill` (NaN: failure_inputs.written_columns) beforehand"""
    import torch
    from mrbo.engine import from_device, to_device
    dev = "cuda:0"
    out = plan.alloc_outputs(with_gradient=with_gradient, want_policy=True, want_obs=True)
    out["policy_x"].fill_(fill)
    x0d = to_device(g["x0s"] if x0s is None else x0s, dev)
    xs = to_device(g["xstarts"], dev)
    if ghq is not None:
        plan.simulate_ghq(x0d, to_device(ghq[0], dev), to_device(ghq[1], dev), xs, out)
    else:
        plan.simulate(x0d, to_device(g["rnstream"] if rn is None else rn, dev), xs, out)
    eto = plan.eto(out)
    torch.cuda.synchronize()
    d, M, R, h = plan.d, plan.M, plan.R * plan.S, plan.h
    res = dict(values=from_device(out["values"], (M, R)), status=from_device(out["status"], (M, R)),
               obs=from_device(out["obs"], (h + 1, M, R)), eto=from_device(eto, (2 + 2 * d + 2, R)),
               evals=from_device(out["evals"], (5, M, R)), policy_x=from_device(out["policy_x"], (d, h + 1, M, R)))
    if with_gradient:
        res["grad_x"] = from_device(out["grad_x"], (d, M, R))
        res["grad_theta"] = from_device(out["grad_theta"], (1, M, R))
    return res


def on_build(oracle, fast, fn):
    if not fast:
        return fn()
    assert os.path.exists(ORACLE_FAST), "the oracle's timing build (make -C oracle) is needed"
    try:
        oracle.use_library(ORACLE_FAST)
        return fn()
    finally:
        oracle.use_library(None)


def replay_status(oracle, g, opts, kw, r, w, fast):
    """T2 status per trajectory: the oracle's replay of the GPU's policy points to horizon w − 1.
    Also returns the full-horizon replay (with the conditioning and the value bounds)."""
    h = int(g["h"])
    st = np.zeros(w.shape, dtype=np.int32)
    full = None
    for j in range(h + 1):
        rp = np.asfortranarray(r["policy_x"][:, 1:j + 1]) if j else None
        o = on_build(oracle, fast, lambda: F.oracle_run(oracle, g, opts, replay_x=rp, h=j, want_kappa=j == h, **kw))
        st = np.where(w == j + 1, o["status"], st)
        if j == h:
            full = o
    return st, full


def same_bits(a, b, msg):
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=msg)
    np.testing.assert_array_equal(a[~np.isnan(a)], b[~np.isnan(b)], err_msg=msg)


def check_failed_outputs(r, w):
    """c: what a failed trajectory leaves (mrbo.h "Failed trajectories")"""
    st = r["status"]
    failed = st != 0
    in_loop = failed & ((st & 16) == 0)
    adj = (st & 16) != 0
    hp1 = r["obs"].shape[0]
    assert np.isnan(r["values"][failed]).all() and np.isfinite(r["values"][~failed]).all()
    assert np.isnan(r["grad_x"][:, failed]).all() and np.isfinite(r["grad_x"][:, ~failed]).all()
    assert np.isnan(r["grad_theta"][:, failed]).all() and np.isfinite(r["grad_theta"][:, ~failed]).all()
    assert np.isnan(r["obs"][:, in_loop]).all() and np.isfinite(r["obs"][:, ~in_loop]).all()
    assert (r["evals"][3:, in_loop] == 0).all()
    assert (r["evals"][3, adj] >= 1).all()          # the rich evaluation whose Hessian was singular
    assert (w[~in_loop] == hp1).all() and (w[in_loop] >= 1).all()
    np.testing.assert_array_equal(np.isnan(r["eto"]).all(axis=0), failed.any(axis=0))
    assert np.isfinite(r["eto"][:, ~failed.any(axis=0)][0]).all()


@pytest.mark.parametrize("cid,recipe", F.PAIRS)
def test_failure_statuses_vs_oracle(gpu, oracle, golden_c2, monkeypatch, cid, recipe):
    case = F.CASE_BY_ID[cid]
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    g0 = case.problem(oracle, golden_c2)
    g, opts = case.apply(recipe, g0)
    kw = case.oracle_kw(g)
    ghq = g.get("ghq")
    plan = make_plan(case, g, opts)
    info = plan.info()
    assert {k: info[k] for k in case.info} == case.info, info
    r = launch(plan, g, ghq=ghq)
    st = r["status"]
    T = st.size
    allow = max(1, T // 100)
    w = F.written_columns(r["policy_x"])
    bit, mixed, allowed = case.expect(recipe)
    ok, counts = F.conditions(st, bit, mixed)
    failed = st != 0
    print(f"\n{cid} {recipe}: GPU status counts {counts}, failures per restart {failed.sum(axis=0).tolist()}, "
          f"by policy columns written {np.bincount(w[failed], minlength=case.h + 2).tolist()}")

    # ---- a. status: T2 (replay to the last written column) on both builds, T3 on the agreeing paths
    s2, full = replay_status(oracle, g, opts, kw, r, w, fast=False)
    s2f, _ = replay_status(oracle, g, opts, kw, r, w, fast=True)
    agree = s2 == s2f
    assert (~agree).sum() <= allow, ("the oracle's builds disagree", int((~agree).sum()))
    o = F.oracle_run(oracle, g, opts, **kw)
    wo = F.written_columns(o["policy_x"])
    wmin = np.minimum(w, wo)
    dx = np.abs(r["policy_x"] - o["policy_x"]) / (1 + np.abs(o["policy_x"]))
    dx = np.where(np.arange(case.h + 1)[None, :, None, None] < wmin[None, None], dx, 0.0)
    assert not np.isnan(dx).any()
    dxt = dx.max(axis=(0, 1))
    ident, near = dxt <= 1e-12, dxt <= 1e-6
    in_solve = failed & (w <= case.h) & (s2 == 0)     # failed in the inner solve of step w: T3 decides
    t2 = agree & ~in_solve
    print(f"  T2 decides {int(t2.sum())}, T3 {int((in_solve & near).sum())} of {T}; identical paths "
          f"{int(ident.sum())}, flips {int((~near).sum())}; builds disagree on {int((~agree).sum())}")
    bad = t2 & (st != s2)
    assert not bad.any(), ("T2 status", np.argwhere(bad)[:8].tolist(), st[bad][:8], s2[bad][:8], w[bad][:8])
    bad = in_solve & near & ((st != o["status"]) | (w != wo))
    assert not bad.any(), ("T3 status", np.argwhere(bad)[:8].tolist(), st[bad][:8], o["status"][bad][:8])
    assert (~(t2 | (in_solve & near))).sum() <= allow
    bad = ident & ((st != o["status"]) | (w != wo))
    assert not bad.any(), ("identical paths", np.argwhere(bad)[:8].tolist(), st[bad][:8], o["status"][bad][:8])
    # Newton counters on identical paths.  nan_starts and singular leave the acquisition surface as it
    # is: equal per trajectory.  The scaled factor and the negative noise put a σ² = 0 boundary inside
    # the box (α has a square-root singularity there and is NaN beyond it), a rounding-sensitive
    # surface in parity.py's sense: the oracle's own two builds differ on the work of 3 of 128
    # identical paths at d = 2, N = 12 with negative noise, by up to (2, 17, 2) -- one line search
    # exhausted on one side, accepted on the other, in a start that does not decide the solve.  So
    # those recipes take parity.py's "steps" rule: per trajectory within WORK_STEPS Newton steps, or
    # twice the builds' own largest difference on the same inputs, and unequal on at most 10 % of the
    # identical paths (an isolated event per affected solve).  A trajectory that stopped at another
    # step is off by a whole multistart (≥ 18 value evaluations and, here, ≥ 70 gradients).
    ev_r, ev_o = r["evals"][:3], np.asarray(o["evals"])
    dw = np.abs(ev_r - ev_o)[:, ident]
    unequal = (dw > 0).any(axis=0)
    if recipe in ("nan_starts", "singular"):
        lim = np.zeros(3, dtype=np.int64)
    else:
        of = on_build(oracle, True, lambda: F.oracle_run(oracle, g, opts, **kw))
        same = np.nan_to_num(np.abs(of["policy_x"] - o["policy_x"]) / (1 + np.abs(o["policy_x"]))).max(axis=(0, 1)) <= 1e-12
        dwo = np.abs(np.asarray(of["evals"]) - ev_o)[:, same]
        lim = np.maximum(np.array([WORK_STEPS, WORK_STEPS * (MAX_LS + 1), WORK_STEPS]), 2 * dwo.max(axis=1))
        assert unequal.mean() <= 0.10, float(unequal.mean())
    print(f"  Newton counters on {dw.shape[1]} identical paths: unequal on {int(unequal.sum())}, largest difference "
          f"{dw.max(axis=1).tolist()}, limit {lim.tolist()}")
    assert (dw <= lim[:, None]).all(), ("Newton counters", np.argwhere(ident)[unequal][:8].tolist(), dw[:, unequal][:, :8])
    # the T3 checks are not vacuous: most paths are identical, failed ones among them
    assert ident.mean() >= 0.5 and (ident & failed).any(), (float(ident.mean()), int((ident & failed).sum()))

    # ---- b. non-vacuity on the GPU's own output
    assert ok, counts
    assert set(counts) <= allowed, (counts, allowed)
    if (cid, recipe) in F.LAST_STEP:
        assert (w[failed] >= case.h).any()

    # ---- c. failed trajectories
    check_failed_outputs(r, w)
    # the columns after the last step are not written at all (not even with a NaN): the same launch
    # over a finite filler leaves exactly the filler there and the same bits everywhere else
    r2 = launch(plan, g, ghq=ghq, fill=SENTINEL)
    unwritten = np.arange(case.h + 1)[None, :, None, None] >= w[None, None]
    assert (r2["policy_x"][np.broadcast_to(unwritten, r2["policy_x"].shape)] == SENTINEL).all()
    assert not (r2["policy_x"][np.broadcast_to(~unwritten, r2["policy_x"].shape)] == SENTINEL).any()
    for k in OUTPUTS:
        a2 = np.where(unwritten, np.nan, r2[k]) if k == "policy_x" else r2[k]
        same_bits(r[k], a2, f"second launch {k}")
    if ((full["status"] != 0).any(axis=0) == failed.any(axis=0)).all():
        np.testing.assert_array_equal(np.isnan(r["eto"]), np.isnan(full["eto"]))

    # ---- d. finished trajectories: T2 bounds, then bit for bit against launches without failing neighbours
    fin = ~failed
    if not fin.any():
        return
    gg = dict(g, h=case.h)
    rr = dict(r)
    for k in ("values", "grad_x"):       # the replay's NaN rows are masked out; keep the norms finite
        rr[k] = np.where(failed if k == "values" else failed[None], 0.0, r[k])
    ff = dict(full)
    for k in ("values", "grad_x", "kappa", "vbound"):
        m = failed if full[k].ndim == 2 else failed[None]
        ff[k] = np.where(m, 1.0 if k in ("kappa", "vbound") else 0.0, full[k])
    _replay_t2(gg, rr, ff, fin & (full["status"] == 0))     # (a build disagreement is not a T2 value error)
    M = st.shape[0]
    for q in range(st.shape[1]):
        if not (fin[:, q].any() and failed[:, q].any()):
            continue
        src = int(np.flatnonzero(fin[:, q])[0])
        rows = np.where(failed[:, q], src, np.arange(M))
        if ghq is not None:
            clean = launch(plan, g, ghq=(np.asfortranarray(ghq[0][rows]), np.asfortranarray(ghq[1][rows])))
        else:
            clean = launch(plan, g, rn=np.asfortranarray(g["rnstream"][rows]))
        assert (clean["status"][:, q] == 0).all(), (q, clean["status"][:, q])
        keep = fin[:, q]
        for k in OUTPUTS:
            same_bits(r[k][..., keep, q], clean[k][..., keep, q], f"restart {q} {k}")
    # and a launch in which nothing fails anywhere (the waves take trajectories of any restart from
    # shared queues, so a half-wave partner may belong to another restart): every sample that fails
    # in some restart replaced by one that finishes in all of them, where such a sample exists
    common = np.flatnonzero(fin.all(axis=1))
    print(f"  samples finishing in every restart: {common.size} of {M}")
    if common.size:
        rows = np.where(failed.any(axis=1), common[0], np.arange(M))
        if ghq is not None:
            clean = launch(plan, g, ghq=(np.asfortranarray(ghq[0][rows]), np.asfortranarray(ghq[1][rows])))
        else:
            clean = launch(plan, g, rn=np.asfortranarray(g["rnstream"][rows]))
        assert (clean["status"] == 0).all(), clean["status"]
        for k in OUTPUTS:
            same_bits(r[k][..., common, :], clean[k][..., common, :], f"no failure anywhere: {k}")


def test_surrogate_batch_blocks_keep_their_own_bits(gpu, oracle, golden_c2):
    """e: S = 3 at d = 2, N = 12, the middle surrogate with the scaled factor: block q of every
    output is its own plain plan's, bit for bit -- the failing block's NaNs and bits included, and
    no bit of it in its neighbours."""
    from mrbo.engine import RolloutPlan
    case = F.CASE_BY_ID["half_d2_n12"]
    g0 = case.problem(oracle, golden_c2)
    gf, _ = case.apply("factor", g0)
    gs = [g0, gf, g0]
    sur = [dict(X=g["X"], L=g["L"], c=g["c"], y=g["y"], kernel=0, lengthscale=1.0, fmini=float(g["fmini"]))
           for g in gs]
    R, M = g0["x0s"].shape[1], g0["rnstream"].shape[0]
    batch = RolloutPlan.from_surrogates(sur, case.h, M, R, g0["xstarts"].shape[1], g0["lbs"], g0["ubs"], 0.0)
    assert batch.info()["S"] == 3 and batch.info()["spec"] == 2
    x0 = np.concatenate([g0["x0s"]] * 3, axis=1)
    rb = launch(batch, g0, x0s=x0)
    plain = [launch(make_plan(case, g, {}), g) for g in gs]
    for q in range(3):
        for k in OUTPUTS + ("eto",):
            same_bits(rb[k][..., q * R:(q + 1) * R], plain[q][k], f"block {q} {k}")
    assert (plain[0]["status"] == 0).all() and (plain[2]["status"] == 0).all()
    ok, counts = F.conditions(plain[1]["status"], 1, True)
    assert ok and set(counts) == {0, 1}, counts


# ---- the entry points above the kernel (d = 2, N = 12, ≤ 6 iterations) ---------------------------
ITERS, ETA, LAG = 6, 0.05, 2      # LAG: the host reads an iteration's check two iterations behind the launches


def _dev(a, dtype=None):
    import torch
    from mrbo.engine import to_device
    if dtype is None:
        return to_device(a, "cuda:0")
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


def _or(t):
    return int(np.bitwise_or.reduce(t.cpu().numpy().ravel()))


def host_ascent(plan, g, x0, iterations, eta, cv=False):
    """The ascent as plain calls -- per iteration mrbo_simulate_mc at the current x0, (the control
    launch and) the ETO rows, mrbo_sga_step -- on device tensors.  Returns the OR of the status
    words per iteration, x0 after every iteration and the number of restarts active after it."""
    import torch
    from mrbo.engine import from_device
    rn, xs = _dev(g["rnstream"]), _dev(g["xstarts"])
    R = plan.R * plan.S
    x, act = _dev(x0), torch.ones(R, dtype=torch.int32, device="cuda:0")
    bits, xk, nact = [], [], []
    for _ in range(iterations):
        out = plan.alloc_outputs(with_gradient=True)
        plan.simulate(x, rn, xs, out)
        b = _or(out["status"])
        if cv:
            ctl = plan.simulate_control(x, rn, xs)
            b |= _or(ctl["status0"])
            e, _ = plan.eto_cv(x, out, ctl)
        else:
            e = plan.eto(out)
        plan.sga_step(e, x, act, plan.M, eta)
        torch.cuda.synchronize()
        bits.append(b)
        xk.append(from_device(x, (plan.d, R)).copy())
        nact.append(int(act.sum().item()))
    return bits, xk, nact


MS = 8     # samples of the per-restart launches


def per_restart_problem(oracle, golden_c2, recipe):
    """A launch whose failures are per restart: the recipe's input at d = 2, N = 12 restricted to MS
    samples that finish from every random x0 (picked from a plain launch of the full input), with
    restarts 0 and 1 moved next to a data point, where step 0 itself fails (σ² < 0 under the scaled
    factor, the Schur complement of the update under negative noise).  Restarts 2 and 3 start
    clean.  Returns (case, problem, opts, the status of the launch at the starts)."""
    case = F.CASE_BY_ID["half_d2_n12"]
    g, opts = case.apply(recipe, case.problem(oracle, golden_c2))
    first = launch(make_plan(case, g, opts), g)
    rows = np.flatnonzero((first["status"] == 0).all(axis=1))
    assert rows.size >= MS, rows
    g = dict(g, rnstream=np.asfortranarray(g["rnstream"][rows[:MS]]))
    x0 = np.array(g["x0s"], order="F")
    x0[:, :2] = g["X"][:, :2] + (0.05 if recipe == "factor" else 0.01)
    g["x0s"] = x0
    st = launch(make_plan(case, g, opts), g)["status"]
    assert (st[:, :2] != 0).all() and (st[:, 2:] == 0).all(), st
    return case, g, opts, st


def test_stochastic_solve_ends_on_a_status_bit(gpu, oracle, golden_c2):
    """mrbo_stochastic_solve on the negative-noise input, restarts 0 and 1 failing from the first
    launch on (bit 4): no iteration is launched once the host has read a non-zero status, LAG = 2
    iterations behind the launches, so the call ends after 1 + LAG of its 6 iterations; result[2]
    is the OR of the status arrays of the launches it made, and x0 is what the same plain calls
    leave after those iterations, bit for bit -- recomputed here with mrbo_simulate_mc,
    mrbo_eto_reduce and mrbo_sga_step at the moving x0.  A restart with a failed trajectory has a
    NaN ETO row and the step moves it to NaN (Julia's x += η·NaN; the reference has thrown by
    then); the clean restarts keep ascending through the LAG iterations."""
    from mrbo.engine import from_device
    case, g, opts, st0 = per_restart_problem(oracle, golden_c2, "noise")
    bits0 = int(np.bitwise_or.reduce(st0.ravel()))
    assert bits0 == 4
    plan = make_plan(case, g, opts)
    x = _dev(g["x0s"])
    res = plan.stochastic_solve(x, _dev(g["rnstream"]), _dev(g["xstarts"]), optimizer="sga", iterations=ITERS, eta=ETA)
    xg = from_device(x, g["x0s"].shape)
    bits, xk, nact = host_ascent(make_plan(case, g, opts), g, g["x0s"], res[0], ETA)
    print(f"\nstochastic_solve result {res}; status OR per replayed iteration {bits}; active {nact}\nx0 {xg.tolist()}")
    assert bits[0] == bits0
    assert res[0] == 1 + LAG and res[0] < ITERS, res
    assert res[2] == int(np.bitwise_or.reduce(bits)) and res[2] & bits0, (res, bits)
    same_bits(xg, xk[-1], "x0 after the solve")
    assert np.isnan(xg[:, :2]).all() and np.isfinite(xg[:, 2:]).all()
    assert all(b != 0 for b in bits)    # a launch at a NaN x0 fails too: no phantom success


def test_shim_raises_on_a_status_bit(gpu, golden_c2):
    """the Julia binding's mirror (mrbo/shim.py stochastic_solve_batch) turns result[2] into an error"""
    from mrbo import shim
    from mrbo.kernels import Matern52
    from mrbo.surrogates import FantasySurrogate, Surrogate
    from mrbo.trajectory import Trajectory, TrajectoryParameters
    from mrbo.utils import ExperimentSetup
    X, y, lbs, ubs = golden_c2["X"], golden_c2["y"], golden_c2["lbs"], golden_c2["ubs"]
    s = Surrogate(Matern52([1.0]), X, y, capacity=12)
    s.σn2 = -0.02                        # the noise recipe: the fit stays, the fantasy updates take it
    rng = np.random.default_rng(0)
    x0 = lbs[:, None] + (ubs - lbs)[:, None] * rng.random((2, 4))
    tp = TrajectoryParameters(start=x0[:, 0], hypers=[0.0], horizon=2, mc_iterations=32,
                              use_low_discrepancy_sequence=True, spatial_lowerbounds=lbs, spatial_upperbounds=ubs)
    es = ExperimentSetup(tp=tp, number_of_starts=16)
    T = Trajectory(s, FantasySurrogate(s, 2), start=x0[:, 0], hypers=[0.0], horizon=2)
    with pytest.raises(RuntimeError, match="status bits"):
        shim.stochastic_solve_batch(T, tp, es.get_starts(), x0, iterations=ITERS, eta=ETA)


@pytest.mark.parametrize("cv", [False, True], ids=["plain", "control_variate"])
def test_rollout_solve_collects_the_bits(gpu, oracle, golden_c2, cv):
    """mrbo_rollout_solve on the scaled-factor input, with and without the control variate: status
    bits do not end the ascent; result[2] / result[3] are the ORs of the status words of the
    ascent's launches / the final launch (the control launches' included), recomputed from plain
    launches; the end points, means and pick are those of the same plain calls bit for bit; a
    restart with a failed trajectory ranks −∞ and never wins while a finite one exists."""
    import torch
    from mrbo.engine import from_device
    case, g, opts, _ = per_restart_problem(oracle, golden_c2, "factor")
    R, M, d = g["x0s"].shape[1], g["rnstream"].shape[0], 2
    plan = make_plan(case, g, opts)
    plan.set_control_variate(cv)
    r = plan.rollout_solve_host(g["x0s"], g["rnstream"], g["xstarts"], optimizer="sga", iterations=ITERS, eta=ETA,
                                incumbent=False)
    plan.set_control_variate(False)
    res = r["result"]
    # the same solve as plain calls
    ref = make_plan(case, g, opts)
    bits, xk, nact = host_ascent(ref, g, g["x0s"], res[0], ETA, cv=cv)
    xe = np.clip(xk[-1], g["lbs"][:, None], g["ubs"][:, None])
    xd, rn, xs = _dev(xe), _dev(g["rnstream"]), _dev(g["xstarts"])
    out = ref.alloc_outputs(with_gradient=False)
    ref.simulate(xd, rn, xs, out)
    fbits = _or(out["status"])
    if cv:
        ctl = ref.simulate_control(xd, rn, xs, with_gradient=False)
        fbits |= _or(ctl["status0"])
        e, _ = ref.eto_cv(xd, out, ctl)
    else:
        e = ref.eto(out)
    means = torch.empty(R, dtype=torch.float64, device="cuda:0")
    xn, mean, pick = ref.pick_restart(xd, e, incumbent=False, means=means)
    torch.cuda.synchronize()
    st_final = from_device(out["status"], (M, R))
    print(f"\nrollout_solve (cv={cv}) result {res}; ascent bits per iteration {bits}, active {nact}; final bits {fbits}; "
          f"failed trajectories per restart {(st_final != 0).sum(axis=0).tolist()}; means {r['means'].ravel()}")
    assert bits[0] != 0 and res[0] > 1                       # a bit in the first launch did not end the ascent
    assert res[2] == int(np.bitwise_or.reduce(bits)), (res, bits)
    assert res[3] == fbits, (res, fbits)
    same_bits(r["x"], xe, "end points")
    same_bits(r["means"].ravel(), from_device(means, (R,)), "means")
    same_bits(r["xnext"].ravel(), from_device(xn, (d,)), "xnext")
    assert int(r["pick"][0]) == int(pick.item())
    bad = (st_final != 0).any(axis=0)
    assert bad[:2].all() and (r["means"].ravel()[bad] == -np.inf).all()
    assert (~bad).any()                                      # a finite restart exists, and it wins
    assert not bad[int(r["pick"][0])] and np.isfinite(r["mean"][0])


@pytest.mark.parametrize("cv", [False, True], ids=["plain", "control_variate"])
def test_rollout_solve_drivers_agree_on_a_failing_surrogate(gpu, golden_c2, cv):
    """bayesopt.rollout_solve on a surrogate with the factor scaled by 0.95, 8 samples: the incumbent
    restart, 0.15 from the best data point, fails at step 0 (σ² < 0 there) and the five batch
    restarts start clean (the oracle: failures per restart [0, 0, 0, 0, 0, 8]).  The host-driven
    loop (stochastic_solve_multi and the Python pick_restart) and the device-resident call return
    the same end points, means, pick and next point, bit for bit; on both, finite and −∞ means are
    present, the failed restart's end point is NaN and its mean −∞, the finished restarts' end points
    are finite, and the pick is a finished restart."""
    from mrbo import bayesopt
    from mrbo.kernels import Matern52
    from mrbo.surrogates import Surrogate
    X, y, lbs, ubs = golden_c2["X"], golden_c2["y"], golden_c2["lbs"], golden_c2["ubs"]
    got = []
    for device_solve in (False, True):
        s = Surrogate(Matern52([1.0]), X, y, capacity=12)
        s.L[:12, :12] *= 0.95
        s.c[:12] /= 0.95 ** 2
        s.version += 1
        trace = []
        out = bayesopt.rollout_solve(s, lbs, ubs, 2, 8, 3, 16, ITERS, 0.0, eta=0.01, solver="sga", incumbent=True,
                                     trace=trace, device_solve=device_solve, variance_reduction=cv)
        got.append((out, trace[0]))
    (oh, th), (od, td) = got
    print(f"\ndevice result {td['result']}; means host {np.asarray(th['means']).ravel()} device "
          f"{np.asarray(td['means']).ravel()}; picks {int(th['pick'])} {int(td['pick'])}")
    assert td["result"][2] != 0 and td["result"][3] != 0
    for out, t in got:
        means = np.asarray(t["means"], dtype=np.float64).ravel()
        x = np.asarray(t["x"], dtype=np.float64).reshape(2, -1)
        fin = np.isfinite(means)
        assert fin.any() and (means[~fin] == -np.inf).all() and (~fin).any(), means
        assert not fin[-1]                                    # the incumbent restart
        assert np.isfinite(x[:, fin]).all() and np.isnan(x[:, -1]).all(), x
        assert fin[int(t["pick"])] and np.isfinite(out[1]) and out[1] == means[int(t["pick"])]
        assert int(t["pick"]) == int(np.argmax(means))        # the first one of the largest mean
    same_bits(np.asarray(th["x"]), np.asarray(td["x"]), "end points")
    same_bits(np.asarray(th["means"], dtype=np.float64).ravel(), np.asarray(td["means"], dtype=np.float64).ravel(), "means")
    assert int(th["pick"]) == int(td["pick"])
    same_bits(np.asarray(oh[0]), np.asarray(od[0]), "xnext")
    same_bits(np.array([oh[1]]), np.array([od[1]]), "mean")


def test_control_launch_status_and_plain_rows(gpu, oracle, golden_c2):
    """mrbo_simulate_control on the scaled-factor input with x0 near the data (where step 0 itself
    fails for some restarts): status0 is the oracle's status at horizon 0, per trajectory; and
    mrbo_eto_reduce_cv gives a restart whose target or control holds a NaN the rows of
    mrbo_eto_reduce, bit for bit, with β = 0 (no NaN reaches a plain row through a
    product with zero)."""
    import torch
    from mrbo.engine import from_device
    case = F.CASE_BY_ID["half_d2_n12"]
    g0 = case.problem(oracle, golden_c2)
    g, opts = case.apply("factor", g0)
    x0 = np.array(g["x0s"], order="F")
    x0[:, :2] = g["X"][:, :2] + 0.05          # two restarts inside the σ² < 0 neighbourhood of a data point
    g["x0s"] = x0
    R, M, d = x0.shape[1], g["rnstream"].shape[0], 2
    plan = make_plan(case, g, opts)
    xd, rn, xs = _dev(x0), _dev(g["rnstream"]), _dev(g["xstarts"])
    out = plan.alloc_outputs(with_gradient=True)
    plan.simulate(xd, rn, xs, out)
    ctl = plan.simulate_control(xd, rn, xs)
    e_cv, beta = plan.eto_cv(xd, out, ctl)
    e_pl = plan.eto(out)
    torch.cuda.synchronize()
    st0 = from_device(ctl["status0"], (M, R))
    st = from_device(out["status"], (M, R))
    o0 = F.oracle_run(oracle, g, opts, h=0)
    # At a Monte-Carlo observation point with σ² < 0 the kernel tests σ² ahead of the draw and reports
    # bit 1; the oracle, as the reference (gp_draw with gradient never takes σ), fails there in the
    # draw's factor, whose first pivot σ² is: bit 2 (mrbo.h "Failed trajectories").  Both stop at the
    # same step with the same outputs; the expected word carries the kernel's bit where the oracle's
    # own σ at x0 is NaN.
    sig0 = oracle.eval_base(F.oracle_surrogate(oracle, g, opts), x0)[1]
    expect = np.where(np.isnan(sig0)[None, :] & (o0["status"] == 2), 1, o0["status"])
    assert np.isnan(sig0[:2]).all() and np.isfinite(sig0[2:]).all(), sig0
    np.testing.assert_array_equal(st0, expect)
    print(f"\ncontrol status counts per restart {[(int((st0[:, q] != 0).sum())) for q in range(R)]}, "
          f"rollout failures per restart {(st != 0).sum(axis=0).tolist()}")
    assert (st0 != 0).any() and (st0 == 0).any()
    assert ((st != 0) | (st0 == 0)).all()                   # a failed control is a failed trajectory
    v0 = from_device(ctl["values0"], (M, R))
    assert np.isnan(v0[st0 != 0]).all() and np.isfinite(v0[st0 == 0]).all()
    W = 2 + 2 * d + 2
    e_cv, e_pl = from_device(e_cv, (W, R)), from_device(e_pl, (W, R))
    beta = from_device(beta, (1 + d, R))
    nan_row = (st != 0).any(axis=0)
    assert nan_row.any()
    same_bits(e_cv[:, nan_row], e_pl[:, nan_row], "plain rows")
    assert (beta[:, nan_row] == 0).all()
    print(f"beta (value series) per restart {beta[0].tolist()}")


@pytest.mark.parametrize("recipe", ["nan_starts", "factor"])
def test_base_solve_status_vs_oracle(gpu, oracle, golden_c2, recipe):
    """mrbo_base_solve on failing inputs, per start against oracle.base_solve: the status (bit 8
    masked: a start whose coordinates hold a NaN returns NaN and status 0, the host's findmin
    filters it), the minimizer and the minimum; mrbo/rbf_optim.py raises on a status."""
    import ctypes
    import torch
    from mrbo import _lib
    from mrbo.engine import from_device
    case = F.CASE_BY_ID["half_d2_n12"]
    g0 = case.problem(oracle, golden_c2)
    if recipe == "nan_starts":
        g, opts = F.nan_starts(g0, every=2)
    else:
        g, opts = case.apply("factor", g0)
    xs = np.array(g["xstarts"], order="F")
    if recipe == "factor":      # four more starts inside the σ² < 0 neighbourhood of a data point
        xs = np.asfortranarray(np.hstack([xs, g["X"][:, :4] + 0.05]))
    d, n = xs.shape
    p = make_plan(case, g, opts)
    dev = "cuda:0"
    xmin = torch.empty(d * n, dtype=torch.float64, device=dev)
    fmin = torch.empty(n, dtype=torch.float64, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    pp = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(p.lib.mrbo_base_solve(p.handle, n, pp(_dev(xs)), pp(xmin), pp(fmin), pp(st), None, 0,
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    xg, fg, sg = from_device(xmin, (d, n)), from_device(fmin, (n,)), from_device(st, (n,))
    xo, fo, so, _ = oracle.base_solve(F.oracle_surrogate(oracle, g, opts), xs, g["lbs"], g["ubs"])
    print(f"\nbase_solve {recipe}: GPU status {sg.tolist()}, oracle {so.tolist()}")
    np.testing.assert_array_equal(sg, so & ~8)
    assert not (sg & 8).any()
    np.testing.assert_array_equal(np.isnan(xg), np.isnan(xo))
    np.testing.assert_array_equal(np.isnan(fg), np.isnan(fo))
    ok = ~np.isnan(fo) & ~np.isnan(xo).any(axis=0) & (so == 0)
    dx = (np.abs(xg - xo) / (1 + np.abs(xo)))[:, ok].max(axis=0)
    assert (dx <= 2e-3).all() and (dx <= 1e-9).mean() >= 0.9, dx       # tests/test_base_solve.py's bars
    np.testing.assert_allclose(fg[ok][dx <= 1e-9], fo[ok][dx <= 1e-9], rtol=1e-9, atol=1e-300)
    if recipe == "nan_starts":
        nan_in = np.isnan(xs).any(axis=0)
        assert nan_in.any() and (sg == 0).all() and np.isnan(fg[nan_in]).all() and np.isfinite(fg[~nan_in]).all()
    else:
        assert (sg & 1).any() and (sg == 0).any()
        from mrbo.kernels import Matern52
        from mrbo.rbf_optim import base_solve_batch
        from mrbo.surrogates import Surrogate
        s = Surrogate(Matern52([1.0]), g0["X"], g0["y"], capacity=12)
        s.L[:12, :12] *= case.scale
        s.c[:12] /= case.scale ** 2
        s.version += 1
        with pytest.raises(FloatingPointError, match="trajectories failed"):
            base_solve_batch(s, g["lbs"], g["ubs"], xs, [0.0])
