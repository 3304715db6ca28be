"""The restart table (KParams::rtab): step 0 of a trajectory -- the EV_DRAW evaluation of the base
surrogate at the restart's x0 and the factor of its draw -- is the same for all M samples of a
restart, so the square full-wave layout computes it once per restart, in further workgroups of the
launch's prologue kernel, and every trajectory reads it.  The writer runs the trajectory's own
inlined code, so the yardstick is equality, bit for bit (NaN positions included), with the in-place
path that MRBO_RESTART_TABLES=0 keeps: values, both gradients, status, work counters, policy points
and observations.  plan.info()["restart_tables"] must be 1 on the one side and 0 on the other, so no
test passes by comparing a path with itself.  No tolerance anywhere.

The C3 problem arrays are built once per module and shared; every launch takes well under a second.
The half-wave kernel (C1 / C2 by default) and the N > 64 layouts (C4, C5) keep the in-place path and
report restart_tables = 0; their kernels' full-wave forms (MRBO_HALF=0) take the table."""
import functools

import numpy as np
import pytest

import conftest  # noqa: F401  (sys.path)
from parity import _plan, _problem_arrays, _run

OUTPUTS = ("values", "grad_x", "grad_theta", "status", "evals", "policy_x", "obs", "eto")


def same(a, b):
    """array_equal with NaNs equal where both have one (floats), exact for the integer outputs"""
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def assert_same_outputs(on, off, label=""):
    for k in OUTPUTS:
        if k in on or k in off:
            assert same(on[k], off[k]), f"{label}: output {k} differs between the table and the in-place path"


def both_paths(monkeypatch, g, run=_run, **plan_opts):
    """The same launch with the restart table and on the in-place path: (table, in place)."""
    monkeypatch.delenv("MRBO_RESTART_TABLES", raising=False)
    p_on = _plan(g, **plan_opts)
    assert p_on.info()["restart_tables"] == 1
    r_on = run(p_on, g)
    monkeypatch.setenv("MRBO_RESTART_TABLES", "0")
    p_off = _plan(g, **plan_opts)
    assert p_off.info()["restart_tables"] == 0
    r_off = run(p_off, g)
    monkeypatch.delenv("MRBO_RESTART_TABLES")
    return r_on, r_off


@functools.lru_cache(maxsize=None)
def c3_arrays():
    return _problem_arrays("C3", 32, 4)


def c3():
    """a fresh shallow copy: a test that changes an entry leaves the shared arrays alone"""
    return dict(c3_arrays())


@pytest.mark.gpu
def test_c3_equals_in_place(gpu, monkeypatch):
    """C3 at M = 32, R = 4: the benchmarked kernel, rollout_kernel<6, 1, 1> of the FMAX = 4 unit."""
    g = c3()
    on, off = both_paths(monkeypatch, g)
    assert (off["status"] == 0).all()
    assert (off["values"] != 0).any() and (off["grad_x"] != 0).any() and off["evals"][4].sum() > 0
    assert_same_outputs(on, off, "C3")


@pytest.mark.gpu
def test_generic_kernel_equals_in_place(gpu, monkeypatch):
    """The generic instantiation rollout_kernel<6, 1, 0> on the same launch."""
    monkeypatch.setenv("MRBO_GENERIC_KERNEL", "1")
    g = c3()
    p = _plan(g)
    assert p.info()["spec"] == 0
    on, off = both_paths(monkeypatch, g)
    assert (off["status"] == 0).all()
    assert_same_outputs(on, off, "C3 generic")


@pytest.mark.gpu
def test_c2_full_wave_equals_in_place(gpu, monkeypatch):
    """C2 at M = 64, R = 4 on its full-wave kernel (MRBO_HALF=0; d = 2, N = 32: the unfolded
    triangular products)."""
    monkeypatch.setenv("MRBO_HALF", "0")
    g = _problem_arrays("C2", 64, 4)
    on, off = both_paths(monkeypatch, g)
    assert (off["status"] == 0).all()
    assert_same_outputs(on, off, "C2 full wave")


@pytest.mark.gpu
@pytest.mark.parametrize("d,N,h", [(1, 7, 1), (3, 24, 4), (9, 20, 2)])
def test_ragged_shapes_equal_in_place(gpu, monkeypatch, d, N, h):
    """d = 1, N = 7, h = 1, the smallest ragged shape of the suite (full-wave kernel: MRBO_HALF=0);
    h = 4: the FMAX = 6 unit; d = 9: the one-wave-per-SIMD kernels, whose table header (5 + 2d +
    (d+1)(d+2)/2 = 78 doubles) is longer than a wave."""
    monkeypatch.setenv("MRBO_HALF", "0")
    ell = 0.6 * 65.536 * N ** (-1.0 / d)
    g = _problem_arrays(None, 32 if d == 1 else 8, 2, testfn="ackley", d=d, N=N, h=h, ell=ell)
    p = _plan(g)
    assert p.info()["fmax"] == (4 if h <= 3 and d <= 8 else 6) and p.info()["rpl"] == 1
    on, off = both_paths(monkeypatch, g)
    assert (off["status"] == 0).all()
    assert_same_outputs(on, off, f"ackley d={d} N={N} h={h}")


@pytest.mark.gpu
def test_layouts_without_the_table_report_it(gpu):
    """The half-wave kernel (C2) and the N > 64 layouts (C4) keep step 0 in place and say so."""
    p2 = _plan(_problem_arrays("C2", 8, 2))
    assert p2.info()["spec"] == 2 and p2.info()["restart_tables"] == 0
    p4 = _plan(_problem_arrays("C4", 4, 2))
    assert p4.info()["rpl"] == 2 and p4.info()["restart_tables"] == 0


@pytest.mark.gpu
def test_horizon_zero_equals_in_place(gpu, monkeypatch):
    """h = 0: the tabled step is the whole trajectory -- the observation y₀ of every sample comes from
    the restored μ and factor (at C3's x0 no y₀ improves on fmini: the values are 0 on both paths)."""
    g = c3()
    g["rnstream"] = np.asfortranarray(g["rnstream"][:, :, :1])
    on, off = both_paths(monkeypatch, g, h=0)
    assert (off["status"] == 0).all() and np.isfinite(off["obs"]).all()
    assert len(np.unique(off["obs"])) > 2 * off["obs"].shape[2]    # the samples' draws differ within a restart
    assert_same_outputs(on, off, "h = 0")


@pytest.mark.gpu
def test_single_sample_equals_in_place(gpu, monkeypatch):
    """M = 1: as many table rows as trajectories."""
    g = c3()
    g["rnstream"] = np.asfortranarray(g["rnstream"][:1])
    on, off = both_paths(monkeypatch, g)
    assert (off["status"] == 0).all()
    assert_same_outputs(on, off, "M = 1")


@pytest.mark.gpu
def test_ghq_equals_in_place(gpu, monkeypatch):
    """Gauss–Hermite observable, 3 nodes, 81 node vectors: step 0 reads σ and ∇σ from the table."""
    from mrbo.rollout import ghq_node_arrays
    from mrbo.utils import gauss_hermite, generate_indices
    g = c3()
    t, w = gauss_hermite(3)
    nodes, weights = ghq_node_arrays(t, w, generate_indices(3, int(g["h"]) + 1))
    ghq = (np.asfortranarray(nodes), np.asfortranarray(weights))
    on, off = both_paths(monkeypatch, g, run=lambda p, g_: _run(p, g_, ghq=ghq), M=nodes.shape[0])
    assert (off["status"] == 0).all() and (off["values"] != 0).any()
    assert_same_outputs(on, off, "GHQ")


@pytest.mark.gpu
def test_sharded_plans_equal_in_place(gpu, monkeypatch):
    """A sharded plan pair (samples 0..7 and 8..31 of 32): each shard equals its in-place launch, and
    the pair equals the single plan's launch."""
    g = c3()
    parts = []
    for lo, hi in [(0, 8), (8, 32)]:
        gg = dict(g)
        gg["rnstream"] = np.asfortranarray(g["rnstream"][lo:hi])
        on, off = both_paths(monkeypatch, gg, M=hi - lo, sample_offset=lo, samples_total=32)
        assert_same_outputs(on, off, f"shard {lo}:{hi}")
        parts.append(on)
    full = _run(_plan(g), g)
    assert same(np.concatenate([q["values"] for q in parts], 0), full["values"])
    assert same(np.concatenate([q["grad_x"] for q in parts], 1), full["grad_x"])


@pytest.mark.gpu
def test_surrogate_batch_equals_in_place(gpu, monkeypatch):
    """A surrogate batch with S = 2 on the square layout: row r + s·R of the table, one launch."""
    import test_gpu_surrogate_batch as sb
    monkeypatch.setitem(sb.SHAPES, "square_s2", dict(sb.SHAPES["square"], S=2))
    monkeypatch.delenv("MRBO_RESTART_TABLES", raising=False)
    c_on = sb.Case("square_s2")
    assert c_on.batched.info()["restart_tables"] == 1 and c_on.batched.info()["S"] == 2
    monkeypatch.setenv("MRBO_RESTART_TABLES", "0")
    c_off = sb.Case("square_s2")
    assert c_off.batched.info()["restart_tables"] == 0
    assert (c_off.out["status"] == 0).all()
    assert set(c_on.out) == sb.OUTPUTS
    for k in sb.OUTPUTS:
        assert same(c_on.out[k], c_off.out[k]), f"surrogate batch: output {k} differs"
    c_on.assert_blocks_equal(label="table, S = 2")    # and each block equals its (tabled) plain plan


@pytest.mark.gpu
@pytest.mark.parametrize("point,bit", [(4, 1), (5, 2)])
def test_x0_on_a_data_point_equals_in_place(gpu, monkeypatch, point, bit):
    """Restart 1 starts exactly on a base data point, the others do not: the in-place path fails that
    restart's trajectories at step 0 (non-zero status) and no others, and the table reproduces the
    failure.  The surrogate is C3's data without observation noise: with the configurations'
    σn² = 1e-6 the variance at a data point stays ≈ σn² > 0 and step 0 succeeds (status 0 on both
    paths), without it σ² = ψ(0) − |L⁻¹kx|² is zero up to rounding.  At data point 4 it comes out
    negative (status 1), at data point 5 non-negative and the factor of the draw fails (status 2) --
    the two step-0 failure branches the table carries."""
    from mrbo.decision_rules import EI
    from mrbo.engine import RolloutPlan
    from mrbo.kernels import Matern52
    from mrbo.surrogates import Surrogate
    g = c3()
    s = Surrogate(Matern52((1.0,)), g["X"].copy(), g["y"].copy(), capacity=g["X"].shape[1], decision_rule=EI(), σn2=0.0)
    n = s.observed
    x0 = np.array(g["x0s"], order="F", copy=True)
    x0[:, 1] = g["X"][:, point]
    g.update(x0s=x0, L=s.L[:n, :n], c=s.c[:n])
    M, R = g["rnstream"].shape[0], x0.shape[1]

    def plan():
        return RolloutPlan(g["X"], g["L"], g["c"], g["y"], 0, 1.0, 0.0, float(s.fmini()), int(g["h"]), M, R,
                           g["xstarts"].shape[1], g["lbs"], g["ubs"], 0.0)

    monkeypatch.delenv("MRBO_RESTART_TABLES", raising=False)
    p_on = plan()
    assert p_on.info()["restart_tables"] == 1
    on = _run(p_on, g)
    monkeypatch.setenv("MRBO_RESTART_TABLES", "0")
    p_off = plan()
    assert p_off.info()["restart_tables"] == 0
    off = _run(p_off, g)
    print("in-place status per restart:", [sorted(set(off["status"][:, r].tolist())) for r in range(R)])
    assert (off["status"][:, 1] != 0).all() and (off["status"][:, 1] == bit).all()
    assert (off["status"][:, [0, 2, 3]] == 0).all()
    assert np.isnan(off["values"][:, 1]).all() and np.isfinite(off["values"][:, [0, 2, 3]]).all()
    assert_same_outputs(on, off, f"x0 on data point {point}")


SOLVE_ITERS = 6


@pytest.mark.gpu
def test_skip_active_equals_in_place(gpu, monkeypatch):
    """mrbo_stochastic_solve's launches skip the restarts that eswavs has stopped (kp.skip_active),
    and the table's writer skips their rows.  A stepwise loop on the in-place plan finds when each
    restart stops: one stops while another still runs (asserted), so launches with a stopped restart
    are compared.  Final x0, ETO rows and stop flags are equal bit for bit."""
    import torch
    from mrbo.engine import from_device, to_device
    g = _problem_arrays("C3", 8, 4)      # M = 8: eswavs stops restart 0 after the first launch
    d, R = g["x0s"].shape
    M = g["rnstream"].shape[0]
    W = 2 + 2 * d + 2
    dev = "cuda:0"
    drn, dxs = to_device(g["rnstream"], dev), to_device(g["xstarts"], dev)

    def solve(plan):
        dx = to_device(g["x0s"], dev)
        eto = torch.full((W * R,), np.nan, dtype=torch.float64, device=dev)
        act = torch.full((R,), 7, dtype=torch.int32, device=dev)
        res = plan.stochastic_solve(dx, drn, dxs, optimizer="sga", iterations=SOLVE_ITERS, eta=0.01, eto=eto, active=act)
        return res, from_device(dx, (d, R)), eto.cpu().numpy(), act.cpu().numpy()

    monkeypatch.setenv("MRBO_RESTART_TABLES", "0")
    p_off = _plan(g)
    assert p_off.info()["restart_tables"] == 0
    dx = to_device(g["x0s"], dev)
    act = torch.ones(R, dtype=torch.int32, device=dev)
    out = p_off.alloc_outputs(with_gradient=True, want_evals=False)
    stops = np.zeros(R, dtype=int)       # iteration whose step stopped the restart (0: still running)
    for it in range(1, SOLVE_ITERS + 1):
        p_off.simulate(dx, drn, dxs, out)
        p_off.sga_step(p_off.eto(out), dx, act, M, 0.01)
        a = act.cpu().numpy()
        stops[(a == 0) & (stops == 0)] = it
    print("stop iteration per restart:", stops.tolist())
    first = stops[stops > 0].min() if (stops > 0).any() else 0
    assert 0 < first < SOLVE_ITERS and ((stops == 0) | (stops > first)).any(), stops
    off = solve(p_off)
    monkeypatch.delenv("MRBO_RESTART_TABLES")
    p_on = _plan(g)
    assert p_on.info()["restart_tables"] == 1
    on = solve(p_on)
    assert on[0] == off[0] and on[0][2] == 0
    for a, b, what in zip(on[1:], off[1:], ("final x0", "ETO rows", "stop flags")):
        assert same(a, b), f"skip_active: {what} differ"
    assert np.array_equal(off[3] != 0, stops == 0)      # the stepwise loop is the one-call loop


@pytest.mark.gpu
def test_second_launch_rewrites_the_table(gpu, monkeypatch):
    """x0 changes on the device between two launches of one plan (as the outer ascent moves it): the
    second launch equals a fresh plan's launch at the new x0 -- the table is rewritten, not reused."""
    import torch
    from mrbo.engine import from_device, to_device
    monkeypatch.delenv("MRBO_RESTART_TABLES", raising=False)
    g = c3()
    dev = "cuda:0"
    d, R = g["x0s"].shape
    M, h = g["rnstream"].shape[0], int(g["h"])
    x_new = np.asfortranarray(0.5 * (g["x0s"] + g["x0s"][:, ::-1]) * 0.9 + 0.03)
    drn, dxs = to_device(g["rnstream"], dev), to_device(g["xstarts"], dev)

    def launch(plan, dx0):
        out = plan.alloc_outputs(with_gradient=True, want_policy=True, want_obs=True)
        plan.simulate(dx0, drn, dxs, out)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    plan = _plan(g)
    assert plan.info()["restart_tables"] == 1
    dx = to_device(g["x0s"], dev)
    first = launch(plan, dx)
    dx.copy_(to_device(x_new, dev))          # the same device buffer, new contents
    second = launch(plan, dx)
    fresh = launch(_plan(g), to_device(x_new, dev))
    assert (fresh["status"] == 0).all()
    assert not same(first["values"], second["values"])
    for k in fresh:
        assert same(second[k], fresh[k]), f"second launch: output {k} differs from a fresh plan's"
    monkeypatch.setenv("MRBO_RESTART_TABLES", "0")
    p_off = _plan(g)
    assert p_off.info()["restart_tables"] == 0
    in_place = launch(p_off, to_device(x_new, dev))
    for k in fresh:
        assert same(second[k], in_place[k]), f"second launch: output {k} differs from the in-place path"


def test_flop_model_counts_the_step0_draw_once_per_restart():
    """mrbo.flops.launch_flops with and without the info key differs by exactly
    (ntraj − R·S)·f_draw(N, 0, d): one step-0 draw per restart instead of one per trajectory."""
    from mrbo import flops
    N, d, h, M, R, ns = 64, 6, 3, 32, 4, 18
    rng = np.random.default_rng(3)
    ev = rng.integers(0, 40, size=(flops.NCOUNTERS, M, R)).astype(np.float64)
    ev[1] += h * ns
    for base in (dict(rpl=1, blocks=256, batch=1), dict(rpl=1, blocks=256, batch=0), dict(rpl=1, blocks=8, batch=1, S=2)):
        off = flops.launch_flops(ev, N, d, h, info=dict(base, restart_tables=0), nstarts=ns)
        assert off == flops.launch_flops(ev, N, d, h, info=base, nstarts=ns)
        on = flops.launch_flops(ev, N, d, h, info=dict(base, restart_tables=1), nstarts=ns)
        assert off - on == (M * R - R) * flops.f_draw(N, 0, d)      # integers below 2^53: exact
    assert flops.launch_flops(ev, N, d, h) - flops.launch_flops(ev, N, d, h, info=dict(restart_tables=1)) \
        == (M * R - R) * flops.f_draw(N, 0, d)
    with pytest.raises(ValueError):      # the restarts are the last axis of evals: a flat array cannot say
        flops.launch_flops(ev.reshape(flops.NCOUNTERS, -1), N, d, h, info=dict(restart_tables=1))
