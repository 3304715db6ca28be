"""mrbo_stochastic_solve and mrbo_rollout_solve run ONE outer ascent (csrc/mrbo_api.hip, Ascent::run)
on one set of plan slots, and the plain Python entries are the S = 1 case of the batched ones.  What
the shared code can newly get wrong: one call leaving state behind for the other on the same plan
(slots, the skip list, the launch order), on a normal and on an error return; and the adapters
handing back the batched shapes.  Everything is compared on raw bits, at the shapes of
tests/test_gpu_rollout_solve.py (its "half" shape: Branin, d = 2, N = 20, h = 1, M = 16, 2 inner starts
+ 2, R = 4, 12 iterations; its "generic" shape for the adapters)."""
import numpy as np
import pytest

import conftest  # noqa: F401  (sys.path)
from test_gpu_rollout_solve import DEV, ETA, ITERS, SHAPES, eta_of, plain_plan, same_bits, surrogates

pytestmark = pytest.mark.gpu

Q = 0   # the surrogate of the "half" shape the plain plans are built on


def _inputs():
    """The half shape's x0 (d×R) on surrogate Q as rollout_solve forms it, other starts x1, the MC
    stream and the inner starts."""
    from mrbo.bayesopt import incumbent_start
    from mrbo.engine import initial_guesses, rnstream
    from mrbo.utils import generate_batch
    sh = SHAPES["half"]
    surs, lbs, ubs = surrogates("half")
    w = (ubs - lbs)[:, None]
    x0 = np.hstack([generate_batch(sh["batch"], lbs, ubs), incumbent_start(surs[Q], lbs, ubs)[:, None]])
    x1 = lbs[:, None] + w * (0.15 + 0.7 * ((x0 - lbs[:, None]) / w))[:, ::-1]
    return surs[Q], lbs, ubs, x0, x1, rnstream(sh["M"], sh["d"], sh["h"] + 1), initial_guesses(sh["starts"], lbs, ubs)


def _plan():
    sh = SHAPES["half"]
    s, lbs, ubs, x0, _, _, xs = _inputs()
    return plain_plan(s, sh["h"], sh["M"], x0.shape[1], xs.shape[1], lbs, ubs)


def _stochastic(torch, plan, x, rn, xs):
    """plan.stochastic_solve (StandardSGA) from x on device tensors: every output, as numpy."""
    from mrbo.engine import to_device
    d, R = x.shape
    dx = to_device(x, DEV)
    eto = torch.full(((2 + 2 * d + 2) * R,), np.nan, dtype=torch.float64, device=DEV)
    active = torch.full((R,), -1, dtype=torch.int32, device=DEV)
    res = plan.stochastic_solve(dx, to_device(rn, DEV), to_device(xs, DEV), optimizer="sga", iterations=ITERS,
                                eta=ETA["sga"], sample_size=SHAPES["half"]["M"], eto=eto, active=active)
    return dict(x=dx.cpu().numpy(), eto=eto.cpu().numpy(), active=active.cpu().numpy(), result=res)


def _rollout(plan, x, rn, xs):
    return plan.rollout_solve_host(x, rn, xs, optimizer="box_adam", iterations=ITERS, eta=ETA["adam"],
                                   sample_size=SHAPES["half"]["M"], incumbent=True)


def _assert_same(a, b, label):
    assert set(a) == set(b), label
    for k in a:
        assert a[k] == b[k] if k == "result" else same_bits(a[k], b[k]), (label, k, a[k], b[k])


def _assert_simulates_as_fresh(torch, used, x, rn, xs):
    """A plain simulate on `used` into buffers pre-filled with −7 runs every trajectory and equals a
    fresh plan's: nothing is left skipped."""
    from mrbo.engine import to_device
    outs = []
    for plan in (used, _plan()):
        out = plan.alloc_outputs(with_gradient=True, want_policy=True, want_obs=True, want_evals=True)
        for v in out.values():
            v.fill_(-7)
        plan.simulate(to_device(x, DEV), to_device(rn, DEV), to_device(xs, DEV), out)
        torch.cuda.synchronize()
        outs.append({k: v.cpu().numpy() for k, v in out.items()})
    for k in outs[0]:
        assert same_bits(outs[0][k], outs[1][k]), k
        assert not (outs[0][k] == -7).any(), k
    assert (outs[0]["status"] == 0).all()


def test_both_calls_on_one_plan(gpu):
    """stochastic_solve, rollout_solve_host, stochastic_solve from other starts, all on ONE plain plan:
    every output of each call equals the same call on a fresh plan, and a plain simulate afterwards
    runs every trajectory.  The first call did skip restarts (its returned stop flags)."""
    torch = gpu
    _, _, _, x0, x1, rn, xs = _inputs()
    used = _plan()
    s1 = _stochastic(torch, used, x0, rn, xs)
    r = _rollout(used, x0, rn, xs)
    s2 = _stochastic(torch, used, x1, rn, xs)
    print(f"stop flags {s1['active']} {r['active'].ravel()} {s2['active']}, results {s1['result']} {r['result']} "
          f"{s2['result']}")
    assert (s1["active"] == 0).any() and s1["result"][2] == 0, s1      # a restart stopped inside the budget
    _assert_same(s1, _stochastic(torch, _plan(), x0, rn, xs), "first stochastic_solve")
    _assert_same(r, _rollout(_plan(), x0, rn, xs), "rollout_solve_host after stochastic_solve")
    _assert_same(s2, _stochastic(torch, _plan(), x1, rn, xs), "stochastic_solve after rollout_solve_host")
    assert not same_bits(s1["x"], s2["x"])
    _assert_simulates_as_fresh(torch, used, x0, rn, xs)


def test_refused_calls_leave_the_plan_as_it_was(gpu):
    """rollout_solve with a negative step and stochastic_solve on a plan with the control variate on
    are refused with their error codes; a plain simulate on the same plan then equals a fresh plan's."""
    torch = gpu
    from mrbo._lib import MrboError
    from mrbo.engine import to_device
    _, _, _, x0, _, rn, xs = _inputs()
    plan = _plan()
    dev = [to_device(a, DEV) for a in (x0, rn, xs)]
    with pytest.raises(MrboError, match=r"mrbo error -1: eta=-1"):                  # MRBO_ERR_ARG
        plan.rollout_solve(*dev, optimizer="box_adam", iterations=ITERS, eta=-1.0)
    plan.set_control_variate(True)
    with pytest.raises(MrboError, match=r"mrbo error -2: .*control variate"):       # MRBO_ERR_UNSUPPORTED
        plan.stochastic_solve(*dev, optimizer="sga", iterations=ITERS)
    plan.set_control_variate(False)
    assert same_bits(dev[0].cpu().numpy(), x0.ravel(order="F"))                      # x0 untouched
    _assert_simulates_as_fresh(torch, plan, x0, rn, xs)


@pytest.mark.parametrize("device_solve", [False, True])
def test_rollout_solve_trace_keeps_its_plain_shape(gpu, device_solve):
    """bayesopt.rollout_solve at the generic shape (d = 1, N = 8, h = 0): the trace entry has the plain
    keys and shapes -- batch and x d×R, means 1-D, pick an int, the host path's history per iteration
    the R ETOs, the device path's result."""
    from mrbo import bayesopt
    from mrbo.trajectory import ExpectedTrajectoryOutput
    sh = SHAPES["generic"]
    (sur,), lbs, ubs = surrogates("generic")
    d, R = sh["d"], sh["batch"] + 2 + 1
    trace = []
    xnext, mean = bayesopt.rollout_solve(sur, lbs, ubs, sh["h"], sh["M"], sh["batch"], sh["starts"], ITERS, 0.0,
                                         eta=eta_of("generic", "sga"), solver="sga", incumbent=True, trace=trace,
                                         device_solve=device_solve)
    (t,) = trace
    assert set(t) == {"batch", "x", "means", "pick", "result" if device_solve else "history"}, set(t)
    assert np.shape(t["batch"]) == (d, R) and np.shape(t["x"]) == (d, R) and np.shape(t["means"]) == (R,)
    assert isinstance(t["pick"], int) and 0 <= t["pick"] < R
    assert np.shape(xnext) == (d,) and isinstance(mean, float)
    assert same_bits(xnext, np.asarray(t["x"])[:, t["pick"]]) and mean == float(t["means"][t["pick"]])
    if device_solve:
        assert len(t["result"]) == 4 and all(isinstance(v, int) for v in t["result"])
    else:
        assert 1 <= len(t["history"]) <= ITERS
        for etos in t["history"]:
            assert isinstance(etos, list) and len(etos) == R
            assert all(isinstance(e, ExpectedTrajectoryOutput) for e in etos)


def test_stochastic_solve_batch_keeps_its_plain_shape(gpu):
    """utils.stochastic_solve_batch at the generic shape: x is d×R, history per iteration a list of
    the R ETOs."""
    from mrbo.optimizers import StandardSGA
    from mrbo.trajectory import ExpectedTrajectoryOutput, TrajectoryParameters
    from mrbo.utils import ExperimentSetup, generate_batch, stochastic_solve_batch
    sh = SHAPES["generic"]
    (sur,), lbs, ubs = surrogates("generic")
    x0 = generate_batch(sh["batch"], lbs, ubs)
    d, R = x0.shape
    tp = TrajectoryParameters(start=x0[:, 0], hypers=[0.0], horizon=sh["h"], mc_iterations=sh["M"],
                              use_low_discrepancy_sequence=True, spatial_lowerbounds=lbs, spatial_upperbounds=ubs)
    es = ExperimentSetup(tp, number_of_starts=sh["starts"])
    x, history = stochastic_solve_batch([StandardSGA(η=eta_of("generic", "sga")) for _ in range(R)], sur, tp, es, x0,
                                        iterations=3)
    assert x.shape == (d, R) and x.dtype == np.float64 and not same_bits(x, x0)
    assert len(history) == 3
    for etos in history:
        assert isinstance(etos, list) and len(etos) == R
        assert all(isinstance(e, ExpectedTrajectoryOutput) for e in etos)
