"""On the square full-wave layout the evaluation's fantasy-row phases -- the E rows of the prologue, the
value and gradient reductions of phase 3, column 0 and the gradient columns of the fantasy rows (4a,
4b), the Gram and ∇μ entries, the backward product's fantasy part with w_f / P_f, and the Hessian's
fantasy points -- run one copy per number of fantasy rows nf = 0..FMAX, chosen by a switch on the
wave-uniform nf (csrc/mrbo_rollout.hip: nf_switch).  A copy has exactly nf rows' loads and FMAs and no
select on r < nf; every sum keeps its terms and their order, so nothing a launch returns may move by
a bit.

The change has no switch of its own, so the yardstick is the library of the commit before it: every
case's outputs -- values, both gradients, status, the five work counters, policy points, observations
and ETO rows -- were recorded once from a build of that commit into tests/golden/nf_copies/<case>.npz
and are compared here bit for bit, NaN positions included, with no tolerance.  The parent's bits are
not the only reference: every case also goes through tests/parity.py's comparison with the CPU oracle
(T2 replay and T3 end to end, its bounds as they are).

Re-recording: build the library of the commit whose bits are to be kept, then on the GPU
    MRBO_LIB=/path/to/that/libmrbo.so python tools/record_nf_copies.py

tests/test_gpu_small_phases.py holds nf up to 3 (FMAX = 4) and up to 5 (FMAX = 6) at the end of longer
rollouts; each case here (C3's arrays, M = 8, R = 2) puts one arm of the switch last, where an
off-by-one cannot hide behind a later step:
  h1, h2        the FMAX = 4 unit's specialised kernel, nf = 1 / nf = 2 as the deepest copy
  h4            the FMAX = 6 unit, nf = 4 as the deepest copy: the first arm the FMAX = 4 unit lacks
  poi_h5        the generic kernel (POI rule) in the FMAX = 6 unit, nf up to 5
  h1_no_rtab    MRBO_RESTART_TABLES=0: the step-0 draw evaluation runs in the kernel with nf = 0
  h2_two_call   MRBO_NEWTON_FUSED=0: the GRADC copies reached by a call of their own

Every case asserts its layout through plan.info(), status 0 on every trajectory, a Hessian on some
trajectory and that on some trajectory the deepest inner solve's policy point is none of the clamped
start points (test_gpu_small_phases.check_real_work).  On the CPU oracle alone these inputs give status
0 everywhere and a deepest solve that moved off the starts on 16 of 16 trajectories at h = 1 and h = 2,
3 of 16 at h = 4 and 8 of 16 at h = 5 with POI.
"""
import functools
import os

import numpy as np
import pytest

import conftest  # noqa: F401  (sys.path)
from parity import _compare, _osur, _plan, _run, _threads
from test_gpu_small_phases import M, OUTPUTS, R, _c3_at, _with_env, check_real_work, same

GOLDEN_DIR = os.path.join(conftest.GOLDEN, "nf_copies")
_F4 = dict(spec=1, rpl=1, fmax=4)

# name -> (horizon, plan options, environment, plan.info() entries, the oracle's rule)
CASES = {
    "h1": (1, {}, {}, _F4, "EI"),
    "h2": (2, {}, {}, _F4, "EI"),
    "h4": (4, {}, {}, dict(spec=1, rpl=1, fmax=6), "EI"),
    "poi_h5": (5, dict(rule=1), {}, dict(spec=0, rpl=1, fmax=6), "POI"),
    "h1_no_rtab": (1, {}, {"MRBO_RESTART_TABLES": "0"}, dict(_F4, restart_tables=0), "EI"),
    "h2_two_call": (2, {}, {"MRBO_NEWTON_FUSED": "0"}, dict(_F4, newton_fused=0), "EI"),
}
ALL_CASES = tuple(CASES)


@functools.lru_cache(maxsize=None)
def run_case(name):
    """(plan.info(), the outputs, the input arrays) of one launch of the case on cuda:0; shared by the
    two tests below, which leave them unchanged"""
    h, opts, env, _, _ = CASES[name]

    def launch():
        g = _c3_at(h)
        p = _plan(g, **opts)
        return p.info(), _run(p, g), g
    return _with_env(env, launch)


def expected_info(name):
    return CASES[name][3]


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
    check_real_work(name, out, g)
    ref = golden(name)
    for k in OUTPUTS:
        assert k in out and k in ref, f"{name}: output {k} missing"
        assert same(out[k], ref[k]), f"{name}: output {k} differs from the recorded bits"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL_CASES)
def test_outputs_against_the_oracle(gpu, oracle, name):
    _, r, g = run_case(name)
    h, rule = int(g["h"]), CASES[name][4]
    kw = dict(nthreads=_threads(), rule=rule)
    args = (g["x0s"], g["rnstream"], g["xstarts"], g["lbs"], g["ubs"], h)
    o = oracle.simulate_mc(_osur(oracle, g), *args, **kw)
    o2 = oracle.simulate_mc(_osur(oracle, g), *args, replay_x=np.asfortranarray(r["policy_x"][:, 1:]),
                            want_policy=False, want_kappa=True, **kw)
    _compare(f"nf_copies {name} ({M} x {R})", g, r, o, o2, M)
