"""The draw sites of a trajectory -- the EV_DRAW evaluation of every step, draw and condition -- stop
computing what nobody reads: a draw evaluation no longer forms the acquisition rule, its gradients or
the stashes a Hessian would take; the last step (k = h) ends its evaluation before the backward
product, draws y alone (∇y too at h = 0, where step 0 may be the best) and conditions no surface;
the batched start values sum nf rows, not FMAX.  Every value that is still produced keeps its
operands, their order and its contraction, so nothing a launch returns may move by a bit.

The change has no switch, so the yardstick is the library of the commit before it: every case's
outputs -- values, both gradients, status, the five work counters, policy points, observations and ETO
rows -- were recorded once from a build of that commit into tests/golden/draw_sites/<case>.npz and
are compared here bit for bit, NaN positions included, with no tolerance.

Re-recording: build the library of the commit whose bits are to be kept (a worktree of it, or a variant
library), then on the GPU
    MRBO_LIB=/path/to/that/libmrbo.so python tools/record_draw_sites.py
which runs run_case() below for every case and rewrites the .npz files.  A later change that moves a
rounding on purpose has to do that, and say so.

tests/test_gpu_small_phases.py, test_gpu_newton_modes.py, test_gpu_restart_tables.py and
test_gpu_failure_paths.py hold the main shapes; these cases (M = 8, R = 2 unless said) reach the arms
those do not:
  h0, h1          C3's arrays at h = 0 (the first step is the last) and h = 1; h0 runs with the restart
                  table and with MRBO_RESTART_TABLES=0, both held to the one recording
  nograd          C3's arrays without gradients
  replay          C3's arrays with replay_x taken from a first launch: no multistart, the draw sites alone
  ghq_full,       C2's arrays with the Gauss–Hermite observable, 5 nodes (M = 125 node vectors), with
  ghq_half        MRBO_HALF=0 and on the half-wave kernel
  cost_h1         the small-phases cost problem (Ackley d = 3, N = 70, quadratic cost) at h = 1
  starts40        C3's arrays with 40 + 2 inner starts: the batched start values' arm for more than 32
  last_fails_1_factor, last_fails_1_noise
                  failure_inputs' recipes factor (scale 0.998) and noise (σn² = −0.01) at d = 2, N = 32,
                  h = 2, M = 32, R = 4: bits 1 and 2 raised in the last step
  last_fails_4    recipe noise_near at h = 0: bit 4 at step 0, which is the last step

Non-vacuity of last_fails_1_* is established on the CPU by the oracle alone
(test_last_step_failures_exist_on_the_oracle): the same input at h and at h − 1 shares the stream's
leading steps, so a trajectory with status 0 at h − 1 and a non-zero status at h failed in its last
step.  On the oracle: factor {0: 75, 1: 30, 2: 23}, 50 of the 53 failures in the last step; noise
{0: 36, 1: 68, 2: 24}, 92 in the last step.  The GPU test asserts both kinds from the recorded status
and that the GPU's status equals the oracle's.
"""
import functools
import os

import numpy as np
import pytest

import conftest  # noqa: F401  (sys.path)
import failure_inputs as F
from parity import _plan, _problem_arrays, _run
from test_gpu_small_phases import _with_env, same

GOLDEN_DIR = os.path.join(conftest.GOLDEN, "draw_sites")
OUTPUTS = ("values", "grad_x", "grad_theta", "status", "evals", "policy_x", "obs", "eto")
M, R = 8, 2
FAIL_SHAPE = dict(d=2, N=32, h=2, M=32, R=4)
FAIL_RECIPES = {"last_fails_1_factor": ("factor", 0.998), "last_fails_1_noise": ("noise", -0.01)}
_SQ = dict(spec=1, rpl=1, fmax=4)


def _c3(h=None):
    from mrbo.engine import rnstream
    g = _problem_arrays("C3", M, R)
    if h is not None:
        g["h"] = h
        g["rnstream"] = rnstream(M, 6, h + 1)
    return g


def _launch(g, opts=None, **run_kw):
    p = _plan(g, **(opts or {}))
    return p.info(), _run(p, g, **run_kw), g


def _replay():
    g = _c3()
    p = _plan(g)
    first = _run(p, g)
    rp = np.asfortranarray(first["policy_x"][:, 1:])
    return p.info(), _run(p, g, replay=rp), g


def _ghq():
    from mrbo.rollout import ghq_node_arrays
    from mrbo.utils import gauss_hermite, generate_indices
    g = _problem_arrays("C2", M, R)
    t, w = gauss_hermite(F.GHQ_NODES)
    nodes, weights = ghq_node_arrays(t, w, generate_indices(F.GHQ_NODES, int(g["h"]) + 1))
    ghq = (np.asfortranarray(nodes), np.asfortranarray(weights))
    return _launch(g, dict(M=nodes.shape[0]), ghq=ghq)


def _cost_h1():
    from mrbo.engine import rnstream
    from test_gpu_small_phases import _ackley
    g = _ackley(3, 70, 4)
    g["h"] = 1
    g["rnstream"] = rnstream(M, 3, 2)
    return _launch(g, dict(cost="quadratic", cost_c0=1.0, cost_w=tuple(float(v) for v in np.linspace(0.5, 1.5, 3))))


def _starts40():
    from mrbo.utils import generate_initial_guesses
    g = _c3()
    g["xstarts"] = generate_initial_guesses(40, g["lbs"], g["ubs"])
    assert g["xstarts"].shape[1] > 32
    return _launch(g)


def fail_problem(oracle, name):
    """(problem, opts, h) of a last_fails_* case, from the oracle's stream and starts (no libmrbo.so)"""
    s = FAIL_SHAPE
    if name == "last_fails_4":
        g0 = F.plain_problem(oracle, s["d"], s["N"], 0, M=s["M"], R=s["R"])
        g, opts = F.noise_near(g0)
    else:
        recipe, v = FAIL_RECIPES[name]
        g0 = F.plain_problem(oracle, s["d"], s["N"], s["h"], M=s["M"], R=s["R"])
        g, opts = F.factor(g0, v) if recipe == "factor" else F.noise(g0, v)
    return g, opts, int(g["h"])


def _fails(name):
    from mrbo.engine import RolloutPlan
    from oracle import oracle as O
    g, opts, h = fail_problem(O, name)
    p = RolloutPlan(g["X"], g["L"], g["c"], g["y"], 0, float(g["ell"]), opts.get("sigma_n2", 1e-6), float(g["fmini"]), h,
                    g["rnstream"].shape[0], g["x0s"].shape[1], g["xstarts"].shape[1], g["lbs"], g["ubs"], 0.0)
    return p.info(), _run(p, g), g


# name -> (launch, the environments it runs in (the first is the recorded one), plan.info() entries per environment)
CASES = {
    "h0": (lambda: _launch(_c3(0)), ({}, {"MRBO_RESTART_TABLES": "0"}),
           (dict(_SQ, restart_tables=1), dict(_SQ, restart_tables=0))),
    "h1": (lambda: _launch(_c3(1)), ({},), (dict(_SQ, restart_tables=1),)),
    "nograd": (lambda: _launch(_c3(), with_gradient=False), ({},), (_SQ,)),
    "replay": (_replay, ({},), (_SQ,)),
    "ghq_full": (_ghq, ({"MRBO_HALF": "0"},), (_SQ,)),
    "ghq_half": (_ghq, ({},), (dict(spec=2, rpl=1, fmax=4),)),
    "cost_h1": (_cost_h1, ({},), (dict(rpl=2),)),
    "starts40": (_starts40, ({},), (dict(_SQ, batch=1),)),
    "last_fails_1_factor": (lambda: _fails("last_fails_1_factor"), ({},), (dict(spec=2, rpl=1, fmax=4),)),
    "last_fails_1_noise": (lambda: _fails("last_fails_1_noise"), ({},), (dict(spec=2, rpl=1, fmax=4),)),
    "last_fails_4": (lambda: _fails("last_fails_4"), ({},), (dict(spec=2, rpl=1, fmax=4),)),
}
ALL_CASES = tuple(CASES)


def run_case(name, env_index=0):
    """(plan.info(), the outputs, the input arrays) of one launch of the case on cuda:0"""
    launch, envs, _ = CASES[name]
    return _with_env(envs[env_index], launch)


def expected_info(name, env_index=0):
    return CASES[name][2][env_index]


def outputs_of(name):
    return tuple(k for k in OUTPUTS if not (name == "nograd" and k.startswith("grad_")))


def check_real_work(name, out, g):
    """what makes a case worth its recording, on the outputs of run_case(name)"""
    st = out["status"]
    if name.startswith("last_fails_1"):
        assert (st == 0).any() and (st != 0).any(), st
    elif name == "last_fails_4":
        assert (st == 4).all(), st
    else:
        assert (st == 0).all(), st
        assert np.isfinite(out["obs"]).all()
    if name == "starts40":
        assert g["xstarts"].shape[1] > 32
        assert (out["evals"][1] >= g["xstarts"].shape[1] * int(g["h"])).all()   # every start's value, every step
    if name in ("replay", "h0", "ghq_full", "ghq_half"):
        pass   # no multistart (replay, h = 0) or whatever the surface gives: the draw sites alone
    elif not name.startswith("last_fails"):
        assert (out["evals"][0] >= 1).any(), "no Newton iteration on any trajectory"


@functools.lru_cache(maxsize=None)
def golden(name):
    z = np.load(os.path.join(GOLDEN_DIR, f"{name}.npz"))
    return {k: z[k] for k in z.files}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL_CASES)
def test_outputs_equal_the_recorded_bits(gpu, name):
    ref = golden(name)
    for e in range(len(CASES[name][1])):
        info, out, g = run_case(name, e)
        for k, v in expected_info(name, e).items():
            assert info[k] == v, (name, e, k, info)
        check_real_work(name, out, g)
        for k in outputs_of(name):
            assert k in out and k in ref, f"{name}: output {k} missing"
            assert same(out[k], ref[k]), f"{name} (environment {e}): output {k} differs from the recorded bits"


@pytest.mark.gpu
@pytest.mark.parametrize("name", tuple(FAIL_RECIPES) + ("last_fails_4",))
def test_last_step_statuses_equal_the_oracle(gpu, oracle, name):
    g, opts, h = fail_problem(oracle, name)
    o = F.oracle_run(oracle, g, opts)
    ref = golden(name)["status"]
    if name != "last_fails_4":
        assert (ref == 0).any() and (ref != 0).any(), ref
    _, out, _ = run_case(name)
    print(f"\n{name}: GPU status counts { {int(v): int((out['status'] == v).sum()) for v in np.unique(out['status'])} }, "
          f"differing from the oracle on {int((out['status'] != o['status']).sum())}")
    np.testing.assert_array_equal(out["status"], o["status"])


@pytest.mark.parametrize("name", tuple(FAIL_RECIPES))
def test_last_step_failures_exist_on_the_oracle(oracle, name):
    g, opts, h = fail_problem(oracle, name)
    a = F.oracle_run(oracle, g, opts)
    b = F.oracle_run(oracle, g, opts, h=h - 1)
    last = (b["status"] == 0) & (a["status"] != 0)
    print(f"\n{name}: status counts { {int(v): int((a['status'] == v).sum()) for v in np.unique(a['status'])} }, "
          f"failed in the last step {int(last.sum())}")
    assert last.any() and (a["status"] == 0).any()


def test_last_step_status_4_on_the_oracle(oracle):
    g, opts, h = fail_problem(oracle, "last_fails_4")
    assert h == 0
    assert (F.oracle_run(oracle, g, opts)["status"] == 4).all()
