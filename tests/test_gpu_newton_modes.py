"""The Newton iteration's evaluation sites with the mode fixed at compile time (evaluate<…, MODE>): on
the square full-wave layout (N ≤ 64, generic and Matérn-5/2 + EI kernels, FMAX 4 and 6, every d) the
head of a run (GSTART + projected-gradient test + BACK for a batched start, VALUE at the start point
otherwise), the line-search trial (VALUE, chained into GRADC + BACK by the fused iteration) and the
two-call loop's GRADC call are instantiations of their own, and the iteration around them is
straight-line.  The arithmetic and its order did not change, so the yardstick is the one of
tests/test_gpu_newton_fused.py: equality, bit for bit (NaN positions included), between the fused
iteration and the two-call loop that MRBO_NEWTON_FUSED=0 keeps -- values, both gradients, status, the
five work counters, policy points, observations and ETO rows (a base solve: minimisers, minima,
status, counters).  plan.info()["newton_fused"] is asserted 1 on the one side and 0 on the other in
every case, so no case compares a path with itself.  No tolerance anywhere.

That file holds C3 (M = 32, R = 4), max_iters = 2, max_ls = 1, the generic kernel, C2 on the
full-wave kernel, three ragged Ackley shapes and a stochastic solve.  This one adds what the new call
sites reach and that file does not: a run that begins with a VALUE evaluation (a base solve: no
batched start values), a cost-weighted plan, a surrogate batch, the FMAX = 6 unit at d = 6, and a
backtrack on the first direction of a run (the trial loop right after the head-of-run site).

The first-direction backtrack was searched on the CPU oracle before this file was written: with
max_iters = 1 every run has one direction at most, so every backtrack is one of a first direction.
C3 at ℓ = 1 has none (M ≤ 32, R ≤ 64, also at ℓ = 0.5 and 2); C3's arrays at ℓ = 0.3, M = 8, R = 4
have them on the oracle (17 of 32 trajectories), whose work counters the kernel's equal.

Not covered, as in that file: the exit "the tight certificate's row pass certifies after an accepted
trial".  No instrumented search was run for this file either (shapes tried: none), so none is claimed."""
import ctypes
import functools

import numpy as np
import pytest

import conftest  # noqa: F401  (sys.path)
from parity import _plan, _problem_arrays, _run

OUTPUTS = ("values", "grad_x", "grad_theta", "status", "evals", "policy_x", "obs", "eto")
GRAD, VALUE, HESS = 0, 1, 2      # rows of the work counters


def same(a, b):
    """array_equal with NaNs equal where both have one (floats), exact for the integer outputs"""
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def assert_same_outputs(on, off, label="", outputs=OUTPUTS):
    for k in outputs:
        assert k in on and k in off, f"{label}: output {k} missing"
        assert same(on[k], off[k]), f"{label}: output {k} differs between the fused and the two-call loop"


def both_paths(monkeypatch, make_plan, run):
    """run(plan) on a plan made with the fused iteration and on one made with the two-call loop:
    (fused, two calls)."""
    monkeypatch.delenv("MRBO_NEWTON_FUSED", raising=False)
    p_on = make_plan()
    assert p_on.info()["newton_fused"] == 1
    r_on = run(p_on)
    monkeypatch.setenv("MRBO_NEWTON_FUSED", "0")
    p_off = make_plan()
    assert p_off.info()["newton_fused"] == 0
    r_off = run(p_off)
    monkeypatch.delenv("MRBO_NEWTON_FUSED")
    return r_on, r_off


@functools.lru_cache(maxsize=None)
def c3_arrays(R=2, ell=None):
    return _problem_arrays("C3", 8, R, ell=ell)


def c3(R=2, ell=None):
    """a fresh shallow copy: a test that changes an entry leaves the shared arrays alone"""
    return dict(c3_arrays(R, ell))


def backtracks(r, g):
    """line-search trials beyond the first of a direction, per trajectory: every value evaluation is a
    batched start value (h · nstarts of them) or a trial, and every direction (one per Hessian) has
    exactly one first trial"""
    return r["evals"][VALUE] - int(g["h"]) * g["xstarts"].shape[1] - r["evals"][HESS]


@pytest.mark.gpu
def test_run_that_begins_with_a_value_evaluation(gpu, monkeypatch):
    """mrbo_base_solve at d = 2, N = 20 (Branin) on the full-wave kernel, 6 starts: a base solve has
    no batched start values (kp.batch off, have_f0 false), so every run begins with the VALUE
    evaluation at its start point -- the head-of-run VALUE site, chained into GRADC + BACK by the
    fused iteration and followed by a GRADC call of its own in the two-call loop."""
    import torch
    from mrbo import _lib
    from mrbo.engine import from_device, to_device
    from mrbo.utils import generate_initial_guesses
    monkeypatch.setenv("MRBO_HALF", "0")
    g = _problem_arrays(None, 4, 1, testfn="braninhoo", d=2, N=20, h=2)
    d = g["X"].shape[0]
    xs = generate_initial_guesses(4, g["lbs"], g["ubs"])
    n = xs.shape[1]
    assert n == 6
    dev = "cuda:0"
    dxs = to_device(xs, dev)
    pp = lambda t: ctypes.c_void_p(t.data_ptr())

    def solve(p):
        assert p.info()["spec"] == 1 and p.info()["rpl"] == 1
        xmin = torch.empty(d * n, dtype=torch.float64, device=dev)
        fmin = torch.empty(n, dtype=torch.float64, device=dev)
        st = torch.empty(n, dtype=torch.int32, device=dev)
        ev = torch.empty(_lib.NCOUNTERS * n, dtype=torch.int64, device=dev)
        _lib.check(p.lib.mrbo_base_solve(p.handle, n, pp(dxs), pp(xmin), pp(fmin), pp(st), pp(ev), 0,
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        return dict(xmin=from_device(xmin, (d, n)), fmin=from_device(fmin, (n,)), status=from_device(st, (n,)),
                    evals=from_device(ev, (_lib.NCOUNTERS, n)))

    on, off = both_paths(monkeypatch, lambda: _plan(g, h=0, M=1, R=1, nstarts=1), solve)
    ev = off["evals"]
    assert (off["status"] == 0).all() and np.isfinite(off["fmin"]).all()
    # one VALUE evaluation at every start point, then one first trial per direction (+ backtracks)
    assert (ev[VALUE] >= 1 + ev[HESS]).all()
    assert ev[GRAD].sum() > 0 and ev[HESS].sum() > 0 and (ev[HESS] >= 2).any()
    assert not same(off["xmin"], np.clip(xs, g["lbs"][:, None], g["ubs"][:, None]))   # the solves moved
    assert_same_outputs(on, off, "base solve d=2 N=20", ("xmin", "fmin", "status", "evals"))


@pytest.mark.gpu
def test_cost_weighted_plan_equals_two_calls(gpu, monkeypatch):
    """C3's arrays at M = 8, R = 2 with NonUniformCost (configs.problem(..., cost=True)): at N ≤ 64
    the generic kernel with kp.cost -- the cost terms of the value, the gradient, the Hessian and
    both certificates at every fixed-mode site."""
    from mrbo import configs
    g = c3()
    opts = configs.problem("C3", M=8, R=2, cost=True).plan_opts()
    assert opts["cost"]
    make = lambda: _plan(g, **opts)
    assert make().info()["spec"] == 0 and make().info()["rpl"] == 1
    on, off = both_paths(monkeypatch, make, lambda p: _run(p, g))
    assert (off["status"] == 0).all() and off["evals"][HESS].sum() > 0
    assert_same_outputs(on, off, "C3 + cost")
    # Some start ran two Newton iterations at least.  The counters are per trajectory, so the same
    # plan with that start alone (the near-bound start 16; the oracle's Hessians on these inputs are
    # almost all its): a trajectory then has h runs, and more than h Hessians put two in one run.
    g1 = dict(g, xstarts=np.ascontiguousarray(g["xstarts"][:, 16:17]))
    on1, off1 = both_paths(monkeypatch, lambda: _plan(g1, **opts), lambda p: _run(p, g1))
    assert (off1["status"] == 0).all()
    assert (off1["evals"][HESS] > int(g["h"])).any()
    assert_same_outputs(on1, off1, "C3 + cost, one start")
    plain = _run(_plan(g), g)
    assert not same(plain["values"], on["values"])       # the cost model did weigh the rule


@pytest.mark.gpu
def test_surrogate_batch_equals_two_calls(gpu, monkeypatch):
    """A surrogate batch S = 2 at d = 2, N = 20, h = 2 (Branin, surrogates built as
    tests/test_gpu_surrogate_batch.py builds its own) on the full-wave kernel: one launch, blockIdx.y
    selects the surrogate; fused against the two-call loop on all S blocks of every output."""
    import torch
    from mrbo import configs
    from mrbo.decision_rules import EI
    from mrbo.engine import RolloutPlan, initial_guesses, rnstream, to_device
    from mrbo.kernels import Matern52
    from mrbo.rollout import surrogate_dict
    from mrbo.surrogates import Surrogate
    from mrbo.utils import kronecker_quasirand
    monkeypatch.setenv("MRBO_HALF", "0")
    d, N, h, M, R, S = 2, 20, 2, 8, 2, 2
    tf = configs.make_testfn("braninhoo", d)
    lbs, ubs = tf.get_bounds()
    w = (ubs - lbs)[:, None]
    surs, x0s = [], []
    for q, ell in enumerate((1.0, 0.7)):
        X = lbs[:, None] + w * kronecker_quasirand(d, N, 37 * q)
        surs.append(Surrogate(Matern52((ell,)), X, tf(X), capacity=N, decision_rule=EI(), σn2=1e-6))
        x0s.append(lbs[:, None] + w * kronecker_quasirand(d, R, 37 * q + N))
    x0s = np.stack(x0s, axis=2)                            # d×R×S
    xstarts = initial_guesses(16, lbs, ubs)
    rule = surs[0].get_decision_rule()
    dicts = [surrogate_dict(s) for s in surs]
    dev = "cuda:0"
    dx0, drn, dxs = to_device(x0s, dev), to_device(rnstream(M, d, h + 1), dev), to_device(xstarts, dev)

    def make():
        return RolloutPlan.from_surrogates(dicts, h, M, R, xstarts.shape[1], lbs, ubs, 0.0, rule=rule.rule_id,
                                           sigma_tol=rule.σtol)

    def run(p):
        assert p.info()["S"] == S and p.info()["spec"] == 1 and p.info()["fmax"] == 4
        out = p.alloc_outputs(with_gradient=True, want_policy=True, want_obs=True, want_evals=True)
        p.simulate(dx0, drn, dxs, out)
        out["eto"] = p.eto(out)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    on, off = both_paths(monkeypatch, make, run)
    assert (off["status"] == 0).all()
    T = M * R
    evals = off["evals"].reshape(S, -1)                    # the surrogate index runs slowest
    assert all(e.any() for e in evals)
    assert (off["values"][:T] != 0).any() and (off["values"][T:] != 0).any()
    assert not same(off["values"][:T], off["values"][T:])  # two different surrogates
    assert_same_outputs(on, off, "surrogate batch S = 2")


@pytest.mark.gpu
def test_fmax6_unit_at_d6_equals_two_calls(gpu, monkeypatch):
    """C3's arrays with h = 4 at M = 8, R = 2: rollout_kernel<6, 1, 1> of the FMAX = 6 unit (four
    fantasy rows; the other file reaches FMAX = 6 at d = 3 and d = 9 only)."""
    from mrbo.engine import rnstream
    g = c3()
    g["h"] = 4
    rn = rnstream(8, 6, 5)
    make = lambda: _plan(g)
    info = make().info()
    assert info["fmax"] == 6 and info["rpl"] == 1 and info["spec"] == 1
    on, off = both_paths(monkeypatch, make, lambda p: _run(p, g, rn=rn))
    assert (off["status"] == 0).all()
    assert (off["values"] != 0).any() and off["evals"][HESS].sum() > 0
    assert_same_outputs(on, off, "C3 arrays, h = 4")


@pytest.mark.gpu
def test_backtrack_on_the_first_direction_of_a_run(gpu, monkeypatch):
    """C3's arrays at ℓ = 0.3, M = 8, R = 4 with max_iters = 1: a run ends with its first accepted
    trial, so every direction is the first of its run -- the one that follows the head-of-run GSTART
    site -- and every backtrack (counted as the other file counts them) is a second trial of such a
    direction.  The oracle has them on these inputs (module docstring)."""
    g = c3(4, 0.3)
    on, off = both_paths(monkeypatch, lambda: _plan(g, max_iters=1), lambda p: _run(p, g))
    assert (off["status"] == 0).all()
    runs = int(g["h"]) * g["xstarts"].shape[1]
    assert (off["evals"][HESS] <= runs).all()              # one direction per run at most
    assert (backtracks(off, g) > 0).any()
    assert_same_outputs(on, off, "C3 arrays at ℓ = 0.3, max_iters = 1")
