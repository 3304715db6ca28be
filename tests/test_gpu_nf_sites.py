"""In the Matérn-5/2 + EI kernel of the square full-wave layout at d = 6 and d = 2 (csrc/mrbo_rollout.hip:
step_nf_dim) the number of fantasy rows nf = S + 1 is found once per rollout step (trajectory()'s
nf_switch around the multistart) and is a template argument from there down: the multistart with
its batched start values, every Newton evaluation and the decision code between them run the copy
of that nf, with no dispatch of their own.  A copy sums the terms of rows r < nf in the order the
run-time form does, so nothing a launch returns may move by a bit.  The draw and rich evaluations
keep the run-time form.

The change has no switch of its own, so the yardstick is the library of the commit before it: every
case's outputs -- values, both gradients, status, the five work counters, policy points, observations
and ETO rows -- were recorded once from a build of that commit into tests/golden/nf_sites/<case>.npz
and are compared here bit for bit, NaN positions included, with no tolerance.  Every case also goes
through tests/parity.py's comparison with the CPU oracle, its bounds as they are.

Re-recording: build the library of the commit whose bits are to be kept, then on the GPU
    MRBO_LIB=/path/to/that/libmrbo.so python tools/record_nf_sites.py

tests/test_gpu_nf_copies.py, test_gpu_small_phases.py, test_gpu_draw_sites.py, test_gpu_newton_modes.py
and test_gpu_restart_tables.py put every arm nf = 0..5 last on this layout through the fused Newton
path with restart tables.  The cases here (C3's arrays at M = 8, R = 2 unless said otherwise) reach the
sites those do not:
  h3_two_call   MRBO_NEWTON_FUSED=0 at h = 3: the stand-alone GRADC site's arms nf = 1..3 (FMAX = 4)
  h5_two_call   the same at h = 5: the FMAX = 6 unit, arms up to nf = 5
  h3_no_rtab    MRBO_RESTART_TABLES=0 at h = 3: the step-0 draw evaluation in the kernel (nf = 0), then
                three dispatched steps
  h3_replay     a replay launch of the policy points of the h = 3 golden (tests/golden/small_phases/c3):
                no multistart, so no step takes the dispatch, and the draw and rich sites run beside
                the code of its arms; the Newton counters are zero
  c2_full_h3    C2's arrays (d = 2, N = 32) with MRBO_HALF=0 at h = 3: a second d through arms nf = 1..3

Every case asserts its plan.info() entries and test_gpu_small_phases.check_real_work: status 0 on every
trajectory, a Hessian on some trajectory, and on some trajectory a deepest inner solve whose policy
point is none of the clamped start points.  h3_two_call and h5_two_call have the inputs of the c3 and
c3_h5 cases there.  On the CPU oracle alone c2_full_h3's inputs give status 0 on 16 of 16 trajectories,
a Hessian on every one and a deepest solve that moved off the starts on 16 of 16.  h3_replay runs no solve: it
asserts status 0, zero Newton counters and that rich evaluations and adjoint pairs ran; its oracle
comparison is parity._replay_t2, the comparison of a replay launch (parity._compare's non-vacuity guard
asks for gradient evaluations of the inner solve, which a replay launch has none of by construction).
"""
import functools
import os

import numpy as np
import pytest

import conftest  # noqa: F401  (sys.path)
import test_gpu_small_phases as SP
from parity import _compare, _osur, _plan, _problem_arrays, _replay_t2, _run, _threads
from test_gpu_small_phases import GRAD, HESS, M, OUTPUTS, R, VALUE, _c3_at, _with_env, check_real_work, same

GOLDEN_DIR = os.path.join(conftest.GOLDEN, "nf_sites")
# spec = 1 is the Matérn-5/2 + EI kernel on the full wave, rollout_kernel<d, 1, 1, 1>; a plan on the
# half-wave kernel reports spec = 2 (test_gpu_small_phases: c2_half against c2_full), so c2_full_h3
# fails here if MRBO_HALF=0 stops taking effect
_F4 = dict(spec=1, rpl=1, fmax=4)
_F6 = dict(spec=1, rpl=1, fmax=6)
RICH, PAIRS = 3, 4      # rows of the work counters after GRAD, VALUE, HESS


def _c2_at(h):
    from mrbo.engine import rnstream
    g = _problem_arrays("C2", M, R)
    g["h"] = h
    g["rnstream"] = rnstream(M, g["X"].shape[0], h + 1)
    return g


def _replay_points():
    return np.asfortranarray(SP.golden("c3")["policy_x"][:, 1:])


# name -> (arrays, environment, plan.info() entries, replay points or None)
CASES = {
    "h3_two_call": (lambda: _c3_at(3), {"MRBO_NEWTON_FUSED": "0"}, dict(_F4, newton_fused=0), None),
    "h5_two_call": (lambda: _c3_at(5), {"MRBO_NEWTON_FUSED": "0"}, dict(_F6, newton_fused=0), None),
    "h3_no_rtab": (lambda: _c3_at(3), {"MRBO_RESTART_TABLES": "0"}, dict(_F4, restart_tables=0), None),
    "h3_replay": (lambda: _c3_at(3), {}, _F4, _replay_points),
    "c2_full_h3": (lambda: _c2_at(3), {"MRBO_HALF": "0"}, _F4, None),
}
ALL_CASES = tuple(CASES)


@functools.lru_cache(maxsize=None)
def run_case(name):
    """(plan.info(), the outputs, the input arrays) of one launch of the case on cuda:0; shared by the
    two tests below, which leave them unchanged"""
    arrays, env, _, replay = CASES[name]

    def launch():
        g = arrays()
        p = _plan(g)
        return p.info(), _run(p, g, replay=None if replay is None else replay()), g
    return _with_env(env, launch)


def expected_info(name):
    return CASES[name][2]


def check_work(name, out, g):
    """the non-vacuity assertions of the module docstring, on the outputs of run_case(name)"""
    if name != "h3_replay":
        check_real_work(name, out, g)
        return
    assert (out["status"] == 0).all(), out["status"]
    ev = out["evals"]
    assert (ev[GRAD] == 0).all() and (ev[VALUE] == 0).all() and (ev[HESS] == 0).all(), ev[:3]
    assert (ev[RICH] >= 1).any() and (ev[PAIRS] >= 1).any(), ev[3:]
    assert same(out["policy_x"][:, 1:], _replay_points())


@functools.lru_cache(maxsize=None)
def golden(name):
    z = np.load(os.path.join(GOLDEN_DIR, f"{name}.npz"))
    return {k: z[k] for k in z.files}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL_CASES)
def test_outputs_equal_the_recorded_bits(gpu, name):
    info, out, g = run_case(name)
    for k, v in expected_info(name).items():
        assert info[k] == v, (name, k, info)
    check_work(name, out, g)
    ref = golden(name)
    for k in OUTPUTS:
        assert k in out and k in ref, f"{name}: output {k} missing"
        assert same(out[k], ref[k]), f"{name}: output {k} differs from the recorded bits"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL_CASES)
def test_outputs_against_the_oracle(gpu, oracle, name):
    _, r, g = run_case(name)
    h = int(g["h"])
    kw = dict(nthreads=_threads(), rule="EI")
    args = (g["x0s"], g["rnstream"], g["xstarts"], g["lbs"], g["ubs"], h)
    o2 = oracle.simulate_mc(_osur(oracle, g), *args, replay_x=np.asfortranarray(r["policy_x"][:, 1:]),
                            want_policy=False, want_kappa=True, **kw)
    if name == "h3_replay":
        assert (o2["status"] == 0).all(), o2["status"]
        _replay_t2(g, r, o2)
        return
    o = oracle.simulate_mc(_osur(oracle, g), *args, **kw)
    _compare(f"nf_sites {name} ({M} x {R})", g, r, o, o2, M)
