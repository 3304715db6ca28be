"""The evaluation's small phases -- the fantasy rows' gradient columns (phase 4b), the Gram entries and
the Hessian assembly -- take the entry an index owns ((r, c) of the fantasy block, (a, b) of the packed
Gram and Hessian triangles) from the wave's lane index table (csrc/mrbo_lane_tables.h, written once by
wave_setup) instead of unranking it in every evaluation -- on the square layout (one row per lane: the
full-wave and half-wave kernels); the layouts with two or more rows per lane (two_rows, cost, l2_fed
below) keep the unranking and are held to the same bits.  Only integer indices changed hands: every
sum keeps its terms and their order, so nothing a launch returns may move by a bit.  (The fixed-trip,
select-masked form of the fantasy-row loops was measured with these cases too, equal to the bit and
not faster, and is not in the code: DESIGN.md §8.)

The change has no switch, so the yardstick is the library of the commit before it: every case's
outputs -- values, both gradients, status, the five work counters, policy points, observations and ETO
rows (the base solve: minimisers, minima, status, counters) -- were recorded once from a build of that
commit into tests/golden/small_phases/<case>.npz and are compared here bit for bit, NaN positions
included, with no tolerance.

Re-recording: build the library of the commit whose bits are to be kept (a worktree of it, or a variant
library), then on the GPU
    MRBO_LIB=/path/to/that/libmrbo.so python tools/record_small_phases.py
which runs run_case() below for every case and rewrites the .npz files.  A later change that moves a
rounding on purpose (another order of a sum, another contraction) has to do that, and say so.

Every case asserts its layout through plan.info() (spec, rpl, fmax), that it does real work (a Hessian
on some trajectory at least) and that the deepest multistart ran with nf = h fantasy rows: every
trajectory finishes with status 0, so each ran its h-th inner solve, which is the one on the surface
with h fantasy rows, and on some trajectory that solve's policy point is none of the start points, so
a Newton iteration moved it.

Cases (M = 8, R = 2), the smallest that reach each arm of the code:
  c3            C3's arrays (d = 6, N = 64, h = 3): the FMAX = 4 unit's square full-wave kernel
  c3_h5         the same at h = 5: the FMAX = 6 unit, nf up to 5 of 6 rows
  c3_poi        C3's arrays with the POI rule: the generic kernel at C3's shape
  d1            C1's arrays (d = 1: NG = 3, NH = 1, the shortest index ranges)
  d8            Ackley d = 8, N = 40, h = 3 (NG = 45, ∇μ on lanes 49..56: the placement boundary)
  d12_h5        Ackley d = 12, N = 40, h = 5 (NG and FMAX·d above 64: the lane-strided arms)
  c2_half       C2's arrays on the half-wave kernel
  c2_full       the same with MRBO_HALF=0
  two_rows      Ackley d = 2, N = 100, h = 2: two rows per lane (Branin at ℓ = 1 and this size moves no
                start point in its last inner solve, on the oracle as on the GPU)
  l2_fed        Ackley d = 3, N = 150, h = 2: four rows per lane, L0⁻¹ from L2
  cost          Ackley d = 3, N = 70, h = 4 with the quadratic cost: the cost-weighted kernel
  base_solve    mrbo_base_solve at d = 2, N = 20: runs that begin with a VALUE evaluation
"""
import ctypes
import functools
import os

import numpy as np
import pytest

import conftest  # noqa: F401  (sys.path)
from parity import _plan, _problem_arrays, _run

GOLDEN_DIR = os.path.join(conftest.GOLDEN, "small_phases")
OUTPUTS = ("values", "grad_x", "grad_theta", "status", "evals", "policy_x", "obs", "eto")
SOLVE_OUTPUTS = ("xmin", "fmin", "status", "evals")
GRAD, VALUE, HESS = 0, 1, 2      # rows of the work counters
M, R = 8, 2


def design_ell(d, N, width=65.536):
    """the lengthscale at the design spacing of N Ackley points (tests/failure_inputs.py)"""
    return 0.6 * width * N ** (-1.0 / d)


def _ackley(d, N, h):
    return _problem_arrays(None, M, R, testfn="ackley", d=d, N=N, h=h, ell=design_ell(d, N))


def _c3_at(h):
    from mrbo.engine import rnstream
    g = _problem_arrays("C3", M, R)
    g["h"] = h
    g["rnstream"] = rnstream(M, 6, h + 1)
    return g


# name -> (arrays, plan options, environment, plan.info() entries)
CASES = {
    "c3": (lambda: _problem_arrays("C3", M, R), {}, {}, dict(spec=1, rpl=1, fmax=4)),
    "c3_h5": (lambda: _c3_at(5), {}, {}, dict(spec=1, rpl=1, fmax=6)),
    "c3_poi": (lambda: _problem_arrays("C3", M, R), dict(rule=1), {}, dict(spec=0, rpl=1, fmax=4)),
    "d1": (lambda: _problem_arrays("C1", M, R), {}, {}, dict(spec=2, rpl=1, fmax=4)),
    "d8": (lambda: _ackley(8, 40, 3), {}, {}, dict(spec=1, rpl=1, fmax=4)),
    "d12_h5": (lambda: _ackley(12, 40, 5), {}, {}, dict(spec=0, rpl=1, fmax=6)),
    "c2_half": (lambda: _problem_arrays("C2", M, R), {}, {}, dict(spec=2, rpl=1, fmax=4)),
    "c2_full": (lambda: _problem_arrays("C2", M, R), {}, {"MRBO_HALF": "0"}, dict(spec=1, rpl=1, fmax=4)),
    "two_rows": (lambda: _ackley(2, 100, 2), {}, {}, dict(spec=1, rpl=2, fmax=4)),
    "l2_fed": (lambda: _ackley(3, 150, 2), {}, {}, dict(spec=1, rpl=4, fmax=4)),
    "cost": (lambda: _ackley(3, 70, 4),
             dict(cost="quadratic", cost_c0=1.0, cost_w=tuple(float(v) for v in np.linspace(0.5, 1.5, 3))), {},
             dict(spec=3, rpl=2, fmax=6)),
}
ALL_CASES = tuple(CASES) + ("base_solve",)


def _with_env(env, fn):
    """fn() with the environment entries set (a plan reads them when it is made)"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _base_solve():
    """mrbo_base_solve at d = 2, N = 20 (Branin) on the full-wave kernel, 6 starts
    (tests/test_gpu_newton_modes.py): no batched start values, every run begins with VALUE"""
    import torch
    from mrbo import _lib
    from mrbo.engine import from_device, to_device
    from mrbo.utils import generate_initial_guesses
    g = _problem_arrays(None, 4, 1, testfn="braninhoo", d=2, N=20, h=2)
    d = g["X"].shape[0]
    xs = generate_initial_guesses(4, g["lbs"], g["ubs"])
    n = xs.shape[1]
    dev = "cuda:0"
    dxs = to_device(xs, dev)
    pp = lambda t: ctypes.c_void_p(t.data_ptr())
    p = _plan(g, h=0, M=1, R=1, nstarts=1)
    xmin = torch.empty(d * n, dtype=torch.float64, device=dev)
    fmin = torch.empty(n, dtype=torch.float64, device=dev)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    ev = torch.empty(_lib.NCOUNTERS * n, dtype=torch.int64, device=dev)
    _lib.check(p.lib.mrbo_base_solve(p.handle, n, pp(dxs), pp(xmin), pp(fmin), pp(st), pp(ev), 0,
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    out = dict(xmin=from_device(xmin, (d, n)), fmin=from_device(fmin, (n,)), status=from_device(st, (n,)),
               evals=from_device(ev, (_lib.NCOUNTERS, n)))
    return p.info(), out, dict(g, xstarts=xs)


def run_case(name):
    """(plan.info(), the outputs, the input arrays) of one launch of the case on cuda:0"""
    if name == "base_solve":
        return _with_env({"MRBO_HALF": "0"}, _base_solve)
    arrays, opts, env, _ = CASES[name]

    def launch():
        g = arrays()
        p = _plan(g, **opts)
        return p.info(), _run(p, g), g
    return _with_env(env, launch)


def expected_info(name):
    return dict(spec=1, rpl=1, fmax=4) if name == "base_solve" else CASES[name][3]


def check_real_work(name, out, g):
    """the non-vacuity assertions of the module docstring, on the outputs of run_case(name)"""
    assert (out["status"] == 0).all(), out["status"]
    assert (out["evals"][HESS] >= 1).any(), "no Hessian on any trajectory"
    if name == "base_solve":
        assert np.isfinite(out["fmin"]).all()
        assert (out["evals"][VALUE] >= 1 + out["evals"][HESS]).all()   # VALUE at every start point first
        return
    h = int(g["h"])
    last = out["policy_x"][:, h].reshape(g["X"].shape[0], -1)           # d × (M·R): x_h of every trajectory
    assert np.isfinite(last).all() and np.isfinite(out["obs"][h]).all()
    starts = np.clip(g["xstarts"], g["lbs"][:, None], g["ubs"][:, None])
    moved = [not (last[:, t:t + 1] == starts).all(axis=0).any() for t in range(last.shape[1])]
    assert any(moved), "the inner solve on the surface with h fantasy rows moved no start point"


def same(a, b):
    """array_equal with NaNs equal where both have one (floats), exact for the integer outputs"""
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


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
    for k in (SOLVE_OUTPUTS if name == "base_solve" else OUTPUTS):
        assert k in out and k in ref, f"{name}: output {k} missing"
        assert same(out[k], ref[k]), f"{name}: output {k} differs from the recorded bits"
