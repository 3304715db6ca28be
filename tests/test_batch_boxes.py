"""Per-surrogate boxes in a surrogate batch (mrbo_plan_create_batch_boxes, include/mrbo.h; DESIGN.md
§19), the host side: the argument checks of the C entry point -- they return before any HIP call, so
they run without a GPU --, the shape checks of the Python layers and the plan cache's key.  The
device side is tests/test_gpu_batch_boxes.py."""
import ctypes

import numpy as np
import pytest

import conftest  # noqa: F401  (sys.path)
from test_surrogate_batch import _desc, _surrogates

MRBO_ERR_ARG = -1


def _create_boxes(descs, lbs, ubs, d=2, cost=0, cost_w=None, params_box=False):
    """mrbo_plan_create_batch_boxes on the descriptors; lbs / ubs d×S arrays or None (a null pointer).
    The shared box of the parameters is null unless params_box: the call must not read it."""
    from mrbo import _lib
    L = _lib.load()
    dp = ctypes.POINTER(ctypes.c_double)
    arr = (_lib.SurrogateDesc * len(descs))(*[sd for sd, _ in descs])
    keep = [None if a is None else np.asfortranarray(np.asarray(a, dtype=np.float64)) for a in (lbs, ubs)]
    ptr = [None if a is None else a.ctypes.data_as(dp) for a in keep]
    lb, ub = np.zeros(d), np.ones(d)
    w = None if cost_w is None else np.asarray(cost_w, dtype=np.float64)
    pd = _lib.ParamsDesc(1, 4, 2, 3, 0, 0.0, lb.ctypes.data_as(dp) if params_box else None,
                         ub.ctypes.data_as(dp) if params_box else None, 50, 20, 1e-3, 1e-3, 1e-8, 1e-4, 1e-8, 1906, 0, 0,
                         cost, 1.0, None if w is None else w.ctypes.data_as(dp))
    h = ctypes.c_void_p()
    rc = L.mrbo_plan_create_batch_boxes(arr, len(descs), ctypes.byref(pd), ptr[0], ptr[1], 0, ctypes.byref(h))
    return rc, L.mrbo_last_error(), h


def _boxes(S, d=2):
    lbs = np.tile(np.zeros(d)[:, None], (1, S)) + 0.1 * np.arange(S)
    return lbs, lbs + 1.0


def test_the_entry_point_is_exported():
    from mrbo import _lib
    assert "mrbo_plan_create_batch_boxes" in _lib.EXPORTS
    assert _lib.load().mrbo_plan_create_batch_boxes is not None


def test_null_bounds():
    lbs, ubs = _boxes(2)
    for a, b in ((None, ubs), (lbs, None), (None, None)):
        rc, msg, h = _create_boxes([_desc(), _desc()], a, b)
        assert rc == MRBO_ERR_ARG and b"null" in msg and not h.value


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("which", ["lbs", "ubs"])
def test_non_finite_bound_names_the_surrogate(bad, which):
    lbs, ubs = _boxes(3)
    (lbs if which == "lbs" else ubs)[1, 2] = bad
    rc, msg, h = _create_boxes([_desc(), _desc(), _desc()], lbs, ubs)
    assert rc == MRBO_ERR_ARG and b"surrogate 2" in msg and b"dimension 1" in msg and not h.value, msg


def test_lb_above_ub_names_the_surrogate():
    lbs, ubs = _boxes(3)
    lbs[0, 1], ubs[0, 1] = 2.0, 1.0
    rc, msg, h = _create_boxes([_desc(), _desc(), _desc()], lbs, ubs)
    assert rc == MRBO_ERR_ARG and b"surrogate 1" in msg and b"dimension 0" in msg and not h.value, msg


def test_the_checks_of_the_shared_box_batch_apply():
    lbs, ubs = _boxes(3)
    rc, msg, h = _create_boxes([_desc(), _desc(), _desc(N=5)], lbs, ubs)
    assert rc == MRBO_ERR_ARG and b"surrogate 2 differs" in msg and not h.value
    rc, msg, h = _create_boxes([_desc(), _desc(null=True), _desc()], lbs, ubs)
    assert rc == MRBO_ERR_ARG and b"bad surrogate 1" in msg and not h.value
    from mrbo import _lib
    h = ctypes.c_void_p()
    assert _lib.load().mrbo_plan_create_batch_boxes(None, 1, None, None, None, 0, ctypes.byref(h)) == MRBO_ERR_ARG


def test_cost_model_is_checked_on_every_surrogates_box():
    """Today's rule (ub > lb in every dimension, so that u = (x − lb)/(ub − lb) and c(x) > 0 are
    defined on the box) per surrogate: a degenerate box on surrogate 1 alone is refused, and the
    shared box of the parameters (valid here) is not what is checked."""
    lbs, ubs = _boxes(2)
    ubs[1, 1] = lbs[1, 1]        # lb == ub passes the box check, not the cost model's
    rc, msg, h = _create_boxes([_desc(), _desc()], lbs, ubs, cost=1, cost_w=[1.0, 1.0], params_box=True)
    assert rc == MRBO_ERR_ARG and b"cost model" in msg and b"surrogate 1" in msg and not h.value, msg
    rc, msg, h = _create_boxes([_desc(), _desc()], *_boxes(2), cost=1, cost_w=[1.0, -1.0])
    assert rc == MRBO_ERR_ARG and b"quadratic cost weight 1" in msg and not h.value, msg


GOOD = dict(X=np.zeros((2, 4)), L=np.eye(4), c=np.zeros(4), y=np.zeros(4), kernel=0, lengthscale=1.0, fmini=0.0)


@pytest.mark.parametrize("lshape,ushape", [((2, 2), (2, 2)), ((2, 4), (2, 4)), ((2,), (2, 3)), ((2, 3), (2,)),
                                           ((3, 2), (3, 2)), ((2, 3, 1), (2, 3, 1)), ((6,), (6,))])
def test_from_surrogates_checks_the_bounds(lshape, ushape):
    """S = 3, d = 2: bounds are both (2,) or both (2, 3)."""
    from mrbo.engine import RolloutPlan
    with pytest.raises(ValueError, match=r"\(d, S\)"):
        RolloutPlan.from_surrogates([GOOD] * 3, 1, 4, 2, 3, np.zeros(lshape), np.ones(ushape), 0.0)


def test_check_bounds():
    from mrbo.engine import check_bounds
    assert check_bounds(np.zeros(2), np.ones(2), 2, 3) is False
    assert check_bounds([0.0, 0.0], [1.0, 1.0], 2, 3) is False
    assert check_bounds(np.zeros((2, 3)), np.ones((2, 3)), 2, 3) is True
    assert check_bounds(np.zeros((2, 1)), np.ones((2, 1)), 2, 1) is True


def _plan_stub(boxed, d=2, ns=5, S=3):
    """A RolloutPlan without a device plan: the fields check_xstarts reads."""
    from mrbo.engine import RolloutPlan
    p = RolloutPlan.__new__(RolloutPlan)
    p.d, p.nstarts, p.S, p.boxed = d, ns, S, boxed
    return p


def test_a_boxed_plan_checks_its_xstarts():
    p = _plan_stub(True)
    p.check_xstarts(np.zeros((2, 5, 3)))
    p.check_xstarts(np.zeros(30))                   # flat column-major: the device tensors' form
    p.check_xstarts(np.zeros((2, 7, 3)), n=7)       # a base solve's own count
    for bad in (np.zeros((2, 5)), np.zeros(10), np.zeros((2, 5, 2)), np.zeros((2, 3, 5)), np.zeros((5, 2, 3))):
        with pytest.raises(ValueError, match="d×n×S"):
            p.check_xstarts(bad)
    with pytest.raises(ValueError, match="d×n×S"):
        p.check_xstarts(np.zeros((2, 5, 3)), n=7)
    # every call that takes xstarts checks them before it touches the library
    for call in (lambda: p.simulate(None, None, np.zeros((2, 5)), {}),
                 lambda: p.simulate_ghq(None, None, None, np.zeros((2, 5)), {}),
                 lambda: p.simulate_control(None, None, np.zeros((2, 5))),
                 lambda: p.stochastic_solve(None, None, np.zeros((2, 5))),
                 lambda: p.rollout_solve(None, None, np.zeros((2, 5))),
                 lambda: p.rollout_solve_host(np.zeros((2, 4, 3)), np.zeros(8), np.zeros((2, 5)))):
        with pytest.raises(ValueError, match="d×n×S"):
            call()
    _plan_stub(False).check_xstarts(np.zeros((2, 5)))   # a shared box takes what it took


def _tp(lbs, ubs, M=4, h=1):
    from mrbo.trajectory import TrajectoryParameters
    return TrajectoryParameters(start=0.5 * (np.asarray(lbs) + np.asarray(ubs)), hypers=[0.0], horizon=h,
                                mc_iterations=M, use_low_discrepancy_sequence=True, spatial_lowerbounds=lbs,
                                spatial_upperbounds=ubs)


def test_multi_helpers_check_per_surrogate_arguments():
    from mrbo.rbf_optim import base_solve_multi
    from mrbo.rollout import per_surrogate_parameters, simulate_trajectory_mc_multi
    from mrbo.surrogates import FantasySurrogate
    from mrbo.trajectory import Trajectory
    ss = _surrogates(3)
    lbs, ubs = _boxes(3)
    tps = [_tp(lbs[:, q], ubs[:, q]) for q in range(3)]
    t0, (bl, bu) = per_surrogate_parameters(tps, 3)
    assert t0 is tps[0] and np.array_equal(bl, lbs) and np.array_equal(bu, ubs)
    assert per_surrogate_parameters(tps[0], 3) == (tps[0], None)
    with pytest.raises(ValueError, match="2 TrajectoryParameters for 3"):
        per_surrogate_parameters(tps[:2], 3)
    with pytest.raises(ValueError, match="horizon or mc_iters"):
        per_surrogate_parameters(tps[:2] + [_tp(lbs[:, 2], ubs[:, 2], M=8)], 3)
    other = _tp(lbs[:, 2], ubs[:, 2])
    other.rnstream_sequence = np.nextafter(np.asarray(other.rnstream_sequence), np.inf)   # one ulp off: not the same bits
    with pytest.raises(ValueError, match="rnstream_sequence"):
        per_surrogate_parameters(tps[:2] + [other], 3)
    Ts = [Trajectory(s, FantasySurrogate(s, 1), start=np.full(2, 0.5), hypers=[0.0], horizon=1) for s in ss]
    x0s = np.full((2, 2, 3), 0.5)
    # xstarts of shape (d, ns) with per-surrogate boxes, and of the wrong S
    for bad in (np.zeros((2, 5)), np.zeros((2, 5, 2))):
        with pytest.raises(ValueError, match="d×n×S"):
            simulate_trajectory_mc_multi(Ts, tps, x0s, bad)
    # guesses of the wrong rank, and mixed (d,) / (d, S) bounds, in base_solve_multi
    with pytest.raises(ValueError, match="d×n×S"):
        base_solve_multi(ss, lbs, ubs, np.zeros((2, 5)), [0.0])
    with pytest.raises(ValueError, match="d×n×S"):
        base_solve_multi(ss, lbs, ubs, np.zeros((2, 5, 2)), [0.0])
    with pytest.raises(ValueError, match="d×n "):
        base_solve_multi(ss, lbs[:, 0], ubs[:, 0], np.zeros((2, 5, 3)), [0.0])
    for a, b in ((lbs[:, 0], ubs), (lbs, ubs[:, 0]), (lbs[:, :2], ubs[:, :2])):
        with pytest.raises(ValueError, match=r"\(d, S\)"):
            base_solve_multi(ss, a, b, np.zeros((2, 5, 3)), [0.0])


def test_rollout_solve_multi_checks_the_bounds():
    from mrbo import bayesopt
    ss = _surrogates(3)
    lbs, ubs = _boxes(3)
    for a, b in ((lbs[:, 0], ubs), (lbs, ubs[:, 0]), (lbs[:, :2], ubs[:, :2])):
        with pytest.raises(ValueError, match=r"\(d, S\)"):
            bayesopt.rollout_solve_multi(ss, a, b, 1, 4, 2, 3, 2, 0.0)


def test_stochastic_solve_multi_takes_tp_and_es_together():
    from mrbo.optimizers import StandardSGA
    from mrbo.utils import ExperimentSetup, stochastic_solve_multi
    ss = _surrogates(2)
    lbs, ubs = _boxes(2)
    tps = [_tp(lbs[:, q], ubs[:, q]) for q in range(2)]
    ess = [ExperimentSetup(t, number_of_starts=2) for t in tps]
    opts = [[StandardSGA()] * 3] * 2
    with pytest.raises(ValueError, match="both shared or both lists"):
        stochastic_solve_multi(opts, ss, tps, ess[0], np.full((2, 3, 2), 0.5))
    with pytest.raises(ValueError, match="both shared or both lists"):
        stochastic_solve_multi(opts, ss, tps[0], ess, np.full((2, 3, 2), 0.5))


def test_plan_cache_key_separates_a_shared_box_from_boxes():
    """The same numbers as (d,) and as (d, 1) -- and S equal (d,) boxes as (d, S) -- are other plans:
    the calls of one take d×nstarts starts, those of the other d×nstarts×S."""
    from mrbo.rollout import _plan_key
    s1, s3 = _surrogates(1), _surrogates(3)
    lb, ub = np.array([0.0, 0.5]), np.array([1.0, 2.0])
    k = lambda ss, a, b: _plan_key(ss, 1, 4, 2, 3, a, b, 0.0, 0, {})
    assert k(s1, lb, ub) == k(s1, lb.copy(), list(ub))
    assert k(s1, lb, ub) != k(s1, lb[:, None], ub[:, None])
    rep = lambda a: np.tile(a[:, None], (1, 3))
    assert k(s3, lb, ub) != k(s3, rep(lb), rep(ub))
    # column-major, as the plan reads them: (d, S) bounds and their transpose's numbers differ
    b2 = np.array([[0.0, 0.1], [0.2, 0.3]])
    assert k(s3[:2], b2, b2 + 1) != k(s3[:2], b2.T, b2.T + 1)
    assert hash(k(s3, rep(lb), rep(ub))) == hash(k(s3, rep(lb), rep(ub)))
