"""The fused Newton iteration of the inner solve: on the square full-wave layout (N ≤ 64, generic and
Matérn-5/2 + EI kernels, FMAX 4 and 6, every d) a line-search trial's VALUE evaluation runs the
iteration's decision code (projected Armijo test, accept, x_tol / f_tol, iteration limit, NaN, the two
gradient certificates) inside the evaluation call and, when the iteration continues, goes on to the
gradient columns, the projected-gradient test and the BACK part in the same call.  The fused call runs
the two-call loop's own code in the same order, so the yardstick is equality, bit for bit (NaN
positions included), with the two-call loop that MRBO_NEWTON_FUSED=0 keeps: values, both gradients,
status, the five work counters, policy points, observations and ETO rows.
plan.info()["newton_fused"] must be 1 on the one side and 0 on the other, so no test passes by
comparing a path with itself.  No tolerance anywhere.

The C3 problem arrays are built once per module and shared; every launch takes well under a second.
The half-wave kernel (C1 / C2 by default) and the N > 64 layouts (C4, C5) keep the two-call loop and
report newton_fused = 0.

Not covered: the exit "the tight certificate's row pass certifies after an accepted trial".  None of
the shapes below is known to reach it (on the CPU the row pass after an accepted trial runs at the
(1, 7, 1) and (3, 24, 4) Ackley shapes and fails every time), and no further shapes were searched
with an instrumented oracle for this file, so none is claimed here."""
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


def assert_same_outputs(on, off, label=""):
    for k in OUTPUTS:
        assert k in on and k in off, f"{label}: output {k} missing"
        assert same(on[k], off[k]), f"{label}: output {k} differs between the fused and the two-call loop"


def both_paths(monkeypatch, g, **plan_opts):
    """The same launch with the fused iteration and with the two-call loop: (fused, two calls)."""
    monkeypatch.delenv("MRBO_NEWTON_FUSED", raising=False)
    p_on = _plan(g, **plan_opts)
    assert p_on.info()["newton_fused"] == 1
    r_on = _run(p_on, g)
    monkeypatch.setenv("MRBO_NEWTON_FUSED", "0")
    p_off = _plan(g, **plan_opts)
    assert p_off.info()["newton_fused"] == 0
    r_off = _run(p_off, g)
    monkeypatch.delenv("MRBO_NEWTON_FUSED")
    return r_on, r_off


@functools.lru_cache(maxsize=None)
def c3_arrays():
    return _problem_arrays("C3", 32, 4)


def c3():
    """a fresh shallow copy: a test that changes an entry leaves the shared arrays alone"""
    return dict(c3_arrays())


def backtracks(r, g):
    """line-search trials beyond the first of a direction, per trajectory: every value evaluation is a
    batched start value (h · nstarts of them) or a trial, and every direction (one per Hessian) has
    exactly one first trial"""
    return r["evals"][VALUE] - int(g["h"]) * g["xstarts"].shape[1] - r["evals"][HESS]


@pytest.mark.gpu
def test_c3_equals_two_calls(gpu, monkeypatch):
    """C3 at M = 32, R = 4: the benchmarked kernel, rollout_kernel<6, 1, 1> of the FMAX = 4 unit.
    Accepted-and-continued trials, convergences after acceptance, backtracks (asserted from the
    counters), projected-gradient stops, kept and retried factorisations."""
    g = c3()
    on, off = both_paths(monkeypatch, g)
    assert (off["status"] == 0).all() and (on["status"] == 0).all()
    assert (off["values"] != 0).any() and (off["grad_x"] != 0).any() and off["evals"][GRAD].sum() > 0
    assert (backtracks(off, g) > 0).any()
    assert_same_outputs(on, off, "C3")


@pytest.mark.gpu
def test_max_iters_equals_two_calls(gpu, monkeypatch):
    """max_iters = 2: the iteration-limit exit inside the fused call."""
    g = c3()
    on, off = both_paths(monkeypatch, g, max_iters=2)
    assert (off["status"] == 0).all()
    assert off["evals"][HESS].sum() > 0
    assert_same_outputs(on, off, "C3 max_iters = 2")
    full = _run(_plan(g), g)
    assert not same(full["evals"], on["evals"])      # the limit did cut iterations short


@pytest.mark.gpu
def test_max_ls_equals_two_calls(gpu, monkeypatch):
    """max_ls = 1: the first failed Armijo test ends the iteration (no acceptable step)."""
    g = c3()
    on, off = both_paths(monkeypatch, g, max_ls=1)
    assert (off["status"] == 0).all()
    assert (backtracks(off, g) == 0).all()            # no second trial of any direction
    assert_same_outputs(on, off, "C3 max_ls = 1")
    full = _run(_plan(g), g)
    assert not same(full["evals"], on["evals"])


@pytest.mark.gpu
def test_generic_kernel_equals_two_calls(gpu, monkeypatch):
    """The generic instantiation rollout_kernel<6, 1, 0> on the same launch."""
    monkeypatch.setenv("MRBO_GENERIC_KERNEL", "1")
    g = c3()
    assert _plan(g).info()["spec"] == 0
    on, off = both_paths(monkeypatch, g)
    assert (off["status"] == 0).all()
    assert_same_outputs(on, off, "C3 generic")


@pytest.mark.gpu
def test_c2_full_wave_equals_two_calls(gpu, monkeypatch):
    """C2 at M = 64, R = 4 on its full-wave kernel (MRBO_HALF=0; d = 2, N = 32: the unfolded
    triangular products)."""
    monkeypatch.setenv("MRBO_HALF", "0")
    g = _problem_arrays("C2", 64, 4)
    assert _plan(g).info()["spec"] == 1
    on, off = both_paths(monkeypatch, g)
    assert (off["status"] == 0).all()
    assert_same_outputs(on, off, "C2 full wave")


@pytest.mark.gpu
@pytest.mark.parametrize("d,N,h", [(1, 7, 1), (3, 24, 4), (9, 20, 2)])
def test_ragged_shapes_equal_two_calls(gpu, monkeypatch, d, N, h):
    """The Ackley shapes of the restart-table test (full-wave kernel: MRBO_HALF=0): d = 1, N = 7, h = 1
    and d = 3, N = 24, h = 4 (the FMAX = 6 unit) run the tight certificate's row pass after accepted
    trials; d = 9: the column-chunked products of the one-wave-per-SIMD kernels."""
    monkeypatch.setenv("MRBO_HALF", "0")
    ell = 0.6 * 65.536 * N ** (-1.0 / d)
    g = _problem_arrays(None, 32 if d == 1 else 8, 2, testfn="ackley", d=d, N=N, h=h, ell=ell)
    p = _plan(g)
    assert p.info()["fmax"] == (4 if h <= 3 and d <= 8 else 6) and p.info()["rpl"] == 1
    on, off = both_paths(monkeypatch, g)
    assert (off["status"] == 0).all()
    assert off["evals"][HESS].sum() > 0
    assert_same_outputs(on, off, f"ackley d={d} N={N} h={h}")


@pytest.mark.gpu
def test_layouts_without_the_fused_loop_report_it(gpu):
    """The half-wave kernel (C2) and the N > 64 layouts (C4) keep the two-call loop and say so."""
    p2 = _plan(_problem_arrays("C2", 8, 2))
    assert p2.info()["spec"] == 2 and p2.info()["newton_fused"] == 0
    p4 = _plan(_problem_arrays("C4", 4, 2))
    assert p4.info()["rpl"] == 2 and p4.info()["newton_fused"] == 0


SOLVE_ITERS = 6


@pytest.mark.gpu
def test_stochastic_solve_equals_two_calls(gpu, monkeypatch):
    """One mrbo_stochastic_solve of 6 iterations at C3, M = 8, R = 4 on both paths: its launches skip
    the restarts that have stopped (kp.skip_active).  Final x0, ETO rows and stop flags are equal bit
    for bit."""
    import torch
    from mrbo.engine import from_device, to_device
    g = _problem_arrays("C3", 8, 4)
    d, R = g["x0s"].shape
    W = 2 + 2 * d + 2
    dev = "cuda:0"
    drn, dxs = to_device(g["rnstream"], dev), to_device(g["xstarts"], dev)

    def solve(plan):
        dx = to_device(g["x0s"], dev)
        eto = torch.full((W * R,), np.nan, dtype=torch.float64, device=dev)
        act = torch.full((R,), 7, dtype=torch.int32, device=dev)
        res = plan.stochastic_solve(dx, drn, dxs, optimizer="sga", iterations=SOLVE_ITERS, eta=0.01, eto=eto, active=act)
        return res, from_device(dx, (d, R)), eto.cpu().numpy(), act.cpu().numpy()

    monkeypatch.delenv("MRBO_NEWTON_FUSED", raising=False)
    p_on = _plan(g)
    assert p_on.info()["newton_fused"] == 1
    on = solve(p_on)
    monkeypatch.setenv("MRBO_NEWTON_FUSED", "0")
    p_off = _plan(g)
    assert p_off.info()["newton_fused"] == 0
    off = solve(p_off)
    assert on[0] == off[0] and on[0][2] == 0
    assert not same(off[1], g["x0s"])                 # the solve moved x0
    for a, b, what in zip(on[1:], off[1:], ("final x0", "ETO rows", "stop flags")):
        assert same(a, b), f"stochastic solve: {what} differ"
