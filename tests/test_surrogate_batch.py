"""Surrogate batches (mrbo_plan_create_batch, include/mrbo.h), the host side: the argument checks of
the C entry point -- they return before any HIP call, so they run without a GPU --, the
`parallel_trials` guard of the BO loops and the shape checks of the multi-surrogate helpers.  The
device side is tests/test_gpu_surrogate_batch.py."""
import ctypes

import numpy as np
import pytest

import conftest  # noqa: F401  (sys.path)

MRBO_ERR_ARG = -1


def _desc(d=2, N=4, kernel=0, sn2=1e-6, null=False):
    """One mrbo_surrogate_t over host arrays (kept alive by the caller through the returned tuple)."""
    from mrbo import _lib
    dp = ctypes.POINTER(ctypes.c_double)
    X = np.asfortranarray(np.arange(d * N, dtype=np.float64).reshape(d, N) / (d * N))
    L = np.eye(N, order="F")
    c = np.zeros(N)
    y = np.linspace(0.0, 1.0, N)
    sd = _lib.SurrogateDesc(d, N, kernel, 1.0, sn2, 0.0, None if null else X.ctypes.data_as(dp), L.ctypes.data_as(dp),
                            N, c.ctypes.data_as(dp), y.ctypes.data_as(dp), 1.0)
    return sd, (X, L, c, y)


def _create_batch(descs, S=None, d=2):
    from mrbo import _lib
    L = _lib.load()
    dp = ctypes.POINTER(ctypes.c_double)
    arr = (_lib.SurrogateDesc * max(len(descs), 1))(*[sd for sd, _ in descs])
    lb, ub = np.zeros(d), np.ones(d)
    pd = _lib.ParamsDesc(1, 4, 2, 3, 0, 0.0, lb.ctypes.data_as(dp), ub.ctypes.data_as(dp), 50, 20, 1e-3, 1e-3, 1e-8,
                         1e-4, 1e-8, 1906, 0, 0)
    h = ctypes.c_void_p()
    rc = L.mrbo_plan_create_batch(arr, len(descs) if S is None else S, ctypes.byref(pd), 0, ctypes.byref(h))
    return rc, L.mrbo_last_error(), h


def test_create_batch_rejects_S_below_one():
    rc, msg, h = _create_batch([_desc()], S=0)
    assert rc == MRBO_ERR_ARG and b"S=0" in msg and not h.value
    rc, msg, h = _create_batch([_desc()], S=-3)
    assert rc == MRBO_ERR_ARG and not h.value


def test_create_batch_rejects_a_null_entry():
    rc, msg, h = _create_batch([_desc(), _desc(null=True), _desc()])
    assert rc == MRBO_ERR_ARG and b"bad surrogate 1" in msg and not h.value


@pytest.mark.parametrize("other,what", [(dict(d=3), "d"), (dict(N=5), "N"), (dict(kernel=3), "kernel"),
                                        (dict(sn2=1e-4), "sigma_n2")])
def test_create_batch_rejects_mismatched_surrogates(other, what):
    """Surrogates of one batch share d, N, kernel and σn2: a mismatch is MRBO_ERR_ARG, reported
    before any device call (this test runs on a machine without a GPU)."""
    rc, msg, h = _create_batch([_desc(), _desc(), _desc(**other)])
    assert rc == MRBO_ERR_ARG and b"surrogate 2 differs" in msg and not h.value, (what, msg)


def test_create_batch_null_arguments():
    from mrbo import _lib
    L = _lib.load()
    h = ctypes.c_void_p()
    assert L.mrbo_plan_create_batch(None, 1, None, 0, ctypes.byref(h)) == MRBO_ERR_ARG


def test_parallel_trials_needs_fresh_surrogates(tmp_path):
    """With the reused surrogate trial t inherits trial t−1's kernel and capacity buffer (Q3): a
    sequential dependence, so lockstep trials refuse it -- before any solve."""
    from mrbo import bayesopt
    with pytest.raises(ValueError, match="reuse_surrogate=False"):
        bayesopt.run("gramacylee", str(tmp_path), budget=1, trials=2, parallel_trials=2, reuse_surrogate=True)
    with pytest.raises(ValueError, match="reuse_surrogate=False"):
        bayesopt.run_myopic("gramacylee", str(tmp_path), budget=1, trials=2, parallel_trials=2, reuse_surrogate=True)
    with pytest.raises(ValueError, match="at least 1"):
        bayesopt.run("gramacylee", str(tmp_path), budget=1, trials=2, parallel_trials=0, reuse_surrogate=False)
    assert bayesopt.parse(["--output-dir", "o", "--function-name", "gramacylee"]).parallel_trials == 1
    assert bayesopt.parse(["--output-dir", "o", "--function-name", "gramacylee", "--parallel-trials",
                           "4"]).parallel_trials == 4


def _surrogates(S, d=2, N=6, kernel=None, rule=None, sn2=1e-6):
    from mrbo.decision_rules import EI
    from mrbo.kernels import Matern52
    from mrbo.surrogates import Surrogate
    from mrbo.utils import kronecker_quasirand
    out = []
    for q in range(S):
        X = kronecker_quasirand(d, N, 11 * q)
        out.append(Surrogate((kernel or Matern52)((1.0 + 0.1 * q,)), X, np.sin(X.sum(axis=0)), capacity=N,
                             decision_rule=rule or EI(), σn2=sn2))
    return out


def test_multi_helpers_check_shapes():
    from mrbo.decision_rules import POI
    from mrbo.kernels import SquaredExponential
    from mrbo.rollout import check_multi_x0s, check_surrogate_batch, simulate_trajectory_mc_multi
    ss = _surrogates(3)
    assert check_surrogate_batch(ss) == (2, 6)
    with pytest.raises(ValueError, match="at least one"):
        check_surrogate_batch([])
    with pytest.raises(ValueError, match="N = 5"):
        check_surrogate_batch(ss[:2] + _surrogates(1, N=5))
    with pytest.raises(ValueError, match="d = 3"):
        check_surrogate_batch(ss[:2] + _surrogates(1, d=3))
    with pytest.raises(ValueError, match="kernel family"):
        check_surrogate_batch(ss[:2] + _surrogates(1, kernel=SquaredExponential))
    with pytest.raises(ValueError, match="kernel family or σn2"):
        check_surrogate_batch(ss[:2] + _surrogates(1, sn2=1e-4))
    with pytest.raises(ValueError, match="decision rule"):
        check_surrogate_batch(ss[:2] + _surrogates(1, rule=POI()))
    assert check_multi_x0s(np.zeros((2, 4, 3)), 3, 2).shape == (2, 4, 3)
    assert check_multi_x0s(np.zeros((2, 3)), 3).shape == (2, 1, 3)      # one restart per surrogate
    for bad in (np.zeros((2, 4, 2)), np.zeros((3, 4, 3)), np.zeros(6)):
        with pytest.raises(ValueError, match="d×R×S"):
            check_multi_x0s(bad, 3, 2)
    with pytest.raises(ValueError, match="at least one"):
        simulate_trajectory_mc_multi([], None, np.zeros((2, 1, 1)), np.zeros((2, 3)))


def test_stochastic_solve_multi_checks_optimizers():
    from mrbo.optimizers import StandardSGA
    from mrbo.trajectory import TrajectoryParameters
    from mrbo.utils import ExperimentSetup, stochastic_solve_multi
    ss = _surrogates(2)
    lbs, ubs = np.zeros(2), np.ones(2)
    tp = TrajectoryParameters(start=np.full(2, 0.5), hypers=[0.0], horizon=1, mc_iterations=4,
                              use_low_discrepancy_sequence=True, spatial_lowerbounds=lbs, spatial_upperbounds=ubs)
    es = ExperimentSetup(tp, number_of_starts=2)
    starts = np.full((2, 3, 2), 0.5)
    with pytest.raises(ValueError, match="2 lists of 3 optimizers"):
        stochastic_solve_multi([[StandardSGA()] * 3], ss, tp, es, starts)
    with pytest.raises(ValueError, match="2 lists of 3 optimizers"):
        stochastic_solve_multi([[StandardSGA()] * 3, [StandardSGA()] * 2], ss, tp, es, starts)
    with pytest.raises(ValueError, match="d×R×S"):
        stochastic_solve_multi([[StandardSGA()] * 3] * 2, ss, tp, es, np.full((2, 3, 3), 0.5))


def test_from_surrogates_checks_its_entries():
    from mrbo.engine import RolloutPlan
    lb, ub = np.zeros(2), np.ones(2)
    with pytest.raises(ValueError, match="at least one"):
        RolloutPlan.from_surrogates([], 1, 4, 2, 3, lb, ub, 0.0)
    good = dict(X=np.zeros((2, 4)), L=np.eye(4), c=np.zeros(4), y=np.zeros(4), kernel=0, lengthscale=1.0, fmini=0.0)
    with pytest.raises(ValueError, match="lacks"):
        RolloutPlan.from_surrogates([good, {k: v for k, v in good.items() if k != "fmini"}], 1, 4, 2, 3, lb, ub, 0.0)
    with pytest.raises(ValueError, match="surrogate 1"):
        RolloutPlan.from_surrogates([good, dict(good, L=np.eye(3))], 1, 4, 2, 3, lb, ub, 0.0)
