"""Device-resident MLE refits (mrbo_gp_optimize_multi, include/mrbo.h), the host side: the argument
checks of the C entry point -- they return before any HIP call, so they run without a GPU -- and
mle.lbfgs_scalar, the Python-float restatement of projected_lbfgs that the device minimiser is held
to, against projected_lbfgs itself on pure-numpy objectives.  The device side is
tests/test_gpu_mle_device.py."""
import ctypes

import numpy as np
import pytest

import conftest  # noqa: F401  (sys.path)

MRBO_ERR_ARG = -1


def _desc(d=2, N=4, kernel=0, sn2=1e-6, null=False, period=1.0):
    """One mrbo_surrogate_t over host arrays (kept alive by the caller through the returned tuple)."""
    from mrbo import _lib
    dp = ctypes.POINTER(ctypes.c_double)
    X = np.asfortranarray(np.arange(d * N, dtype=np.float64).reshape(d, N) / (d * N))
    y = np.linspace(0.0, 1.0, N)
    sd = _lib.SurrogateDesc(d, N, kernel, 1.0, sn2, 0.0, None if null else X.ctypes.data_as(dp), None, N, None,
                            y.ctypes.data_as(dp), period)
    return sd, (X, y)


def _optimize(descs, S=None, nt=1, lower=(0.1, 0.1), upper=(5.0, 5.0), opts=None, null=()):
    """mrbo_gp_optimize_multi with host pointers; `null` names the arguments passed as NULL."""
    from mrbo import _lib
    L = _lib.load()
    arr = (_lib.SurrogateDesc * max(len(descs), 1))(*[sd for sd, _ in descs])
    S_ = len(descs) if S is None else S
    n = max(S_, 1) * max(nt, 1)
    a = dict(theta0=np.ones(n), lower=np.array(lower, dtype=np.float64), upper=np.array(upper, dtype=np.float64),
             theta=np.zeros(n), nll=np.zeros(n), grad=np.zeros(n), iters=np.zeros(n, dtype=np.int32))
    res = (ctypes.c_int32 * 2)()
    vp = lambda k: None if k in null else ctypes.c_void_p(a[k].ctypes.data)
    o = None if opts is None else ctypes.byref(_lib.MleOpts(*opts))
    rc = L.mrbo_gp_optimize_multi(arr, S_, nt, vp("theta0"), vp("lower"), vp("upper"), o, vp("theta"), vp("nll"),
                                  vp("grad"), vp("iters"), None if "result" in null else res,
                                  _lib.MRBO_FLAG_HOST_POINTERS, None)
    return rc, L.mrbo_last_error()


def test_optimize_multi_rejects_S_below_one():
    rc, msg = _optimize([_desc()], S=0)
    assert rc == MRBO_ERR_ARG and b"S=0" in msg
    assert _optimize([_desc()], S=-2)[0] == MRBO_ERR_ARG


def test_optimize_multi_rejects_a_null_entry():
    rc, msg = _optimize([_desc(), _desc(null=True), _desc()])
    assert rc == MRBO_ERR_ARG and b"bad surrogate 1" in msg


@pytest.mark.parametrize("other,what", [(dict(d=3), "d"), (dict(N=5), "N"), (dict(kernel=3), "kernel"),
                                        (dict(sn2=1e-4), "sigma_n2")])
def test_optimize_multi_rejects_mismatched_data_sets(other, what):
    rc, msg = _optimize([_desc(), _desc(), _desc(**other)])
    assert rc == MRBO_ERR_ARG and b"surrogate 2 differs" in msg, (what, msg)


def test_optimize_multi_rejects_nt_outside_the_kernels_range():
    rc, msg = _optimize([_desc(), _desc()], nt=2)          # Matérn-5/2 has one hyperparameter
    assert rc == MRBO_ERR_ARG and b"nt=2" in msg
    assert _optimize([_desc(), _desc()], nt=0)[0] == MRBO_ERR_ARG
    assert _optimize([_desc(kernel=4), _desc(kernel=4)], nt=3)[0] == MRBO_ERR_ARG
    rc, msg = _optimize([_desc(kernel=4), _desc(kernel=4, period=0.0)], nt=1)
    assert rc == MRBO_ERR_ARG and b"period" in msg


@pytest.mark.parametrize("lower,upper", [((5.0,), (0.1,)), ((np.nan,), (5.0,)), ((0.1,), (np.inf,)),
                                         ((-np.inf,), (5.0,)), ((0.1,), (np.nan,))])
def test_optimize_multi_rejects_bad_bounds(lower, upper):
    rc, msg = _optimize([_desc(), _desc()], lower=lower, upper=upper)
    assert rc == MRBO_ERR_ARG and b"bounds" in msg, msg
    # the second hyperparameter's bounds are checked too (Periodic, nt = 2)
    rc, msg = _optimize([_desc(kernel=4)], nt=2, lower=(0.1,) + lower, upper=(5.0,) + upper)
    assert rc == MRBO_ERR_ARG and b"hyperparameter 1" in msg, msg


@pytest.mark.parametrize("opts,what", [((30, 17, 0.0, 0.0), b"history"), ((30, -1, 0.0, 0.0), b"history"),
                                       ((-1, 10, 0.0, 0.0), b"iterations"), ((30, 10, -1.0, 0.0), b"g_tol"),
                                       ((30, 10, 0.0, np.nan), b"c1")])
def test_optimize_multi_rejects_options_out_of_range(opts, what):
    rc, msg = _optimize([_desc(), _desc()], opts=opts)
    assert rc == MRBO_ERR_ARG and what in msg, msg


@pytest.mark.parametrize("name", ["theta0", "lower", "upper", "theta", "nll", "grad", "iters", "result"])
def test_optimize_multi_rejects_null_arrays(name):
    rc, msg = _optimize([_desc(), _desc()], null=(name,))
    assert rc == MRBO_ERR_ARG and b"null" in msg, msg


def test_optimize_multi_null_surrogates_and_flags():
    from mrbo import _lib
    L = _lib.load()
    a = np.ones(2)
    p = ctypes.c_void_p(a.ctypes.data)
    res = (ctypes.c_int32 * 2)()
    assert L.mrbo_gp_optimize_multi(None, 1, 1, p, p, p, None, p, p, p, p, res, 0, None) == MRBO_ERR_ARG
    sd, _keep = _desc()
    arr = (_lib.SurrogateDesc * 1)(sd)
    lo, hi = np.array([0.1]), np.array([5.0])
    q = lambda v: ctypes.c_void_p(v.ctypes.data)
    assert L.mrbo_gp_optimize_multi(arr, 1, 1, p, q(lo), q(hi), None, p, p, p, p, res, 4, None) == MRBO_ERR_ARG
    assert b"flags" in L.mrbo_last_error()


def test_gp_optimize_multi_checks_its_arguments():
    """The Python entry point's own checks (no device call is reached)."""
    from test_gp_fit_multi import _surrogates
    from mrbo.mle import gp_optimize_multi
    ss = _surrogates(2)
    with pytest.raises(ValueError, match="at least one"):
        gp_optimize_multi([], None, [0.1], [5.0])
    with pytest.raises(ValueError, match="surrogate 2 has d = 2, N = 5"):
        gp_optimize_multi(ss + _surrogates(1, N=5), None, [0.1], [5.0])
    with pytest.raises(ValueError, match="lowerbounds and upperbounds"):
        gp_optimize_multi(ss)
    with pytest.raises(ValueError, match=r"theta0 has shape \(3, 1\)"):
        gp_optimize_multi(ss, np.ones((3, 1)), [0.1], [5.0])
    with pytest.raises(ValueError, match="history = 17"):
        gp_optimize_multi(ss, None, [0.1], [5.0], history=17)
    with pytest.raises(ValueError, match="iterations = 0"):
        gp_optimize_multi(ss, None, [0.1], [5.0], iterations=0)


# ---- lbfgs_scalar against projected_lbfgs -------------------------------------------------------
def _same(a, b):
    """(x, f, g, iterations) equal with ==, element for element."""
    return (np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2]) and a[3] == b[3]
            and np.shape(a[0]) == np.shape(b[0]))


def _quartic(X):
    x = X[:, 0]
    return (x - 0.3) ** 4 + 0.5 * (x - 0.3) ** 2, (4 * (x - 0.3) ** 3 + (x - 0.3))[:, None]


def _barrier(X):          # the shape of −ll in ℓ: linear growth against a logarithm; minimiser 0.5
    x = X[:, 0]
    return x - 3.0 * np.log(x + 2.5), (1.0 - 3.0 / (x + 2.5))[:, None]


def _wiggly(X):
    x = X[:, 0]
    return np.cosh(3 * (x + 0.5)) + np.sin(5 * x), (3 * np.sinh(3 * (x + 0.5)) + 5 * np.cos(5 * x))[:, None]


def _nan_trials(X):       # evaluates at the start only: no trial step is finite, so none meets Armijo
    f, g = _quartic(X)
    return (f, g) if len(X) == 1 else (np.full(len(X), np.nan), g)


# objective, start, box, options of the minimiser
ONE_D = [
    pytest.param(_quartic, 1.7, (-2.0, 2.0), {}, id="quartic"),
    pytest.param(_wiggly, 1.9, (-2.0, 2.0), {}, id="wiggly"),
    pytest.param(_quartic, -2.0, (-2.0, 2.0), {}, id="from-the-lower-bound"),
    pytest.param(_barrier, 0.2, (-2.0, 0.2), {}, id="starts-on-an-active-bound"),
    pytest.param(_barrier, 3.0, (-2.0, 0.2), {}, id="start-clipped-to-an-active-bound"),
    pytest.param(_nan_trials, 1.7, (-2.0, 2.0), {}, id="no-armijo-step"),
    pytest.param(_wiggly, 1.9, (-2.0, 2.0), dict(iterations=3), id="budget-spent"),
    pytest.param(_wiggly, 1.9, (-2.0, 2.0), dict(m=2), id="history-of-two"),
    pytest.param(_barrier, -1.9, (-2.0, 2.0), dict(m=1, g_tol=1e-12, c1=0.3), id="other-options"),
]


@pytest.mark.parametrize("fg,x0,box,kw", ONE_D)
def test_lbfgs_scalar_equals_projected_lbfgs_one_variable(fg, x0, box, kw):
    """One variable: every dot product is a single multiplication, so == holds by construction."""
    from mrbo.mle import lbfgs_scalar, projected_lbfgs
    a = projected_lbfgs(fg, np.array([x0]), [box[0]], [box[1]], **kw)
    b = lbfgs_scalar(fg, np.array([x0]), [box[0]], [box[1]], **kw)
    assert _same(a, b), (a, b)


def test_one_variable_problems_stop_in_different_ways():
    """What the cases above are there for: different iteration counts, a start on an active bound
    (no line search at all), a line search without an Armijo step (one counted iteration, the start
    kept) and a spent budget."""
    from mrbo.mle import lbfgs_scalar
    run = lambda fg, x0, box, **kw: lbfgs_scalar(fg, np.array([x0]), [box[0]], [box[1]], **kw)
    its = [run(_quartic, 1.7, (-2.0, 2.0))[3], run(_wiggly, 1.9, (-2.0, 2.0))[3], run(_quartic, -2.0, (-2.0, 2.0))[3]]
    assert len(set(its)) == 3 and min(its) > 3, its
    x, f, g, it = run(_barrier, 0.2, (-2.0, 0.2))
    assert it == 0 and x[0] == 0.2 and g[0] < 0
    x, f, g, it = run(_nan_trials, 1.7, (-2.0, 2.0))
    assert it == 1 and x[0] == 1.7 and np.isfinite(f)
    assert run(_wiggly, 1.9, (-2.0, 2.0), iterations=3)[3] == 3
    # a NaN objective at the start: one line search, nothing accepted (what a failing fit gives)
    x, f, g, it = run(lambda X: (np.full(len(X), np.nan), np.full((len(X), 1), np.nan)), 1.0, (0.1, 5.0))
    assert it == 1 and x[0] == 1.0 and np.isnan(f)


def test_lbfgs_scalar_history_pops():
    """m = 2 on problems of more than 3 iterations: the oldest pair leaves.  One variable: == by
    construction.  Two variables: == holds as well (see the next test), and the run differs from
    the m = 10 run, so the pop really acts."""
    from test_gp_fit_multi import HI, LO, PROBLEMS
    from mrbo.mle import lbfgs_scalar, projected_lbfgs
    a = projected_lbfgs(_wiggly, np.array([1.9]), [-2.0], [2.0], m=2)
    b = lbfgs_scalar(_wiggly, np.array([1.9]), [-2.0], [2.0], m=2)
    assert a[3] > 3 and _same(a, b), (a, b)
    fg, x0 = PROBLEMS[0]
    a = projected_lbfgs(fg, x0, LO, HI, m=2)
    b = lbfgs_scalar(fg, x0, LO, HI, m=2)
    assert a[3] > 3 and _same(a, b), (a, b)
    assert lbfgs_scalar(fg, x0, LO, HI, m=10)[3] != b[3]


@pytest.mark.parametrize("m", [10, 2])
def test_lbfgs_scalar_equals_projected_lbfgs_two_variables(m):
    """Two variables: a BLAS kernel behind numpy's 2-element `@` may fuse its multiply-add, which
    the specification never does, so == is not guaranteed in general.  On these three problems it
    holds for m = 10 and m = 2 (numpy 2.2.6 over OpenBLAS 0.3.29: x, f, g and the iteration count all
    equal), so == is what is asserted."""
    from test_gp_fit_multi import HI, LO, PROBLEMS
    from mrbo.mle import lbfgs_scalar, projected_lbfgs
    its = []
    for fg, x0 in PROBLEMS:
        a = projected_lbfgs(fg, x0, LO, HI, m=m)
        b = lbfgs_scalar(fg, x0, LO, HI, m=m)
        assert _same(a, b), (a, b)
        its.append(a[3])
    assert len(set(its)) == 3, its
    # the second problem ends on the bound it started on, gradient outward
    b = lbfgs_scalar(PROBLEMS[1][0], PROBLEMS[1][1], LO, HI, m=m)
    assert b[0][0] == 2.0 and b[2][0] < 0


def test_lbfgs_scalar_against_projected_lbfgs_two_variables_one_pair():
    """m = 1: the first two problems are equal with ==.  The third (condition 3000) spends all 30
    iterations and does differ: numpy's `@` rounds some 2-element dot products otherwise than
    a0*b0 + a1*b1 (with numpy 2.2.6 over OpenBLAS 0.3.29 about a quarter of random ones differ in the
    last bit), and 30 ill-conditioned iterations carry that along.  Measured there: equal iteration
    counts, θ relative difference 1.0187e-10, |Δf| 2.2334e-16 (f = 7.2e-12), max |Δg| 2.3257e-10
    (|g| = 6.7e-5).  Each bound is 16× its measured difference."""
    from test_gp_fit_multi import HI, LO, PROBLEMS
    from mrbo.mle import lbfgs_scalar, projected_lbfgs
    for fg, x0 in PROBLEMS[:2]:
        a, b = projected_lbfgs(fg, x0, LO, HI, m=1), lbfgs_scalar(fg, x0, LO, HI, m=1)
        assert _same(a, b), (a, b)
    fg, x0 = PROBLEMS[2]
    a, b = projected_lbfgs(fg, x0, LO, HI, m=1), lbfgs_scalar(fg, x0, LO, HI, m=1)
    dx, df, dg = np.max(np.abs(a[0] - b[0]) / np.abs(a[0])), abs(a[1] - b[1]), np.max(np.abs(a[2] - b[2]))
    print(a[3], b[3], dx, df, dg)
    assert a[3] == b[3] == 30, (a, b)
    assert dx <= 16 * 1.0187e-10 and df <= 16 * 2.2334e-16 and dg <= 16 * 2.3257e-10, (dx, df, dg)


def test_lbfgs_scalar_two_variables_isolated_failure_and_budget():
    """A line search without an Armijo step and a budget of two iterations, two variables: == holds."""
    from test_gp_fit_multi import HI, LO, PROBLEMS
    from mrbo.mle import lbfgs_scalar, projected_lbfgs

    def nan_trials(X):
        f, g = PROBLEMS[0][0](X)
        return (f, g) if len(X) == 1 else (np.full(len(X), np.nan), g)

    x0 = np.array([1.5, 1.0])
    a, b = projected_lbfgs(nan_trials, x0, LO, HI), lbfgs_scalar(nan_trials, x0, LO, HI)
    assert _same(a, b) and a[3] == 1 and np.array_equal(b[0], x0), (a, b)
    for fg, x0 in PROBLEMS:
        a, b = projected_lbfgs(fg, x0, LO, HI, iterations=2), lbfgs_scalar(fg, x0, LO, HI, iterations=2)
        assert _same(a, b), (a, b)
