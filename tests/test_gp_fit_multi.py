"""Batched GP refits (mrbo_gp_fit_multi, include/mrbo.h), the host side: the argument checks of the
C entry point -- they return before any HIP call, so they run without a GPU --, the shape check of
mle.gp_fit_multi and the lockstep minimiser projected_lbfgs_multi on pure-numpy objectives.  The
device side is tests/test_gpu_gp_fit_multi.py."""
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


def _fit_multi(descs, S=None, P=2, nt=1):
    from mrbo import _lib
    L = _lib.load()
    arr = (_lib.SurrogateDesc * max(len(descs), 1))(*[sd for sd, _ in descs])
    S_ = len(descs) if S is None else S
    n = max(S_, 1) * max(P, 1)
    th, ll, grad = np.ones(n * nt), np.zeros(n), np.zeros(n * nt)
    st = np.zeros(n, dtype=np.int32)
    vp = lambda a: ctypes.c_void_p(a.ctypes.data)
    rc = L.mrbo_gp_fit_multi(arr, S_, P, nt, vp(th), vp(ll), vp(grad), vp(st), None, None,
                             _lib.MRBO_FLAG_HOST_POINTERS, None)
    return rc, L.mrbo_last_error()


def test_fit_multi_rejects_S_and_P_below_one():
    rc, msg = _fit_multi([_desc()], S=0)
    assert rc == MRBO_ERR_ARG and b"S=0" in msg
    assert _fit_multi([_desc()], S=-2)[0] == MRBO_ERR_ARG
    assert _fit_multi([_desc()], P=0)[0] == MRBO_ERR_ARG


def test_fit_multi_rejects_a_null_entry():
    rc, msg = _fit_multi([_desc(), _desc(null=True), _desc()])
    assert rc == MRBO_ERR_ARG and b"bad surrogate 1" in msg


@pytest.mark.parametrize("other,what", [(dict(d=3), "d"), (dict(N=5), "N"), (dict(kernel=3), "kernel"),
                                        (dict(sn2=1e-4), "sigma_n2")])
def test_fit_multi_rejects_mismatched_data_sets(other, what):
    """The data sets of one call share d, N, kernel and σn2: a mismatch is MRBO_ERR_ARG, reported
    before any device call (this test runs on a machine without a GPU)."""
    rc, msg = _fit_multi([_desc(), _desc(), _desc(**other)])
    assert rc == MRBO_ERR_ARG and b"surrogate 2 differs" in msg, (what, msg)


def test_fit_multi_rejects_nt_outside_the_kernels_range():
    rc, msg = _fit_multi([_desc(), _desc()], nt=2)          # Matérn-5/2 has one hyperparameter
    assert rc == MRBO_ERR_ARG and b"nt=2" in msg
    assert _fit_multi([_desc(), _desc()], nt=0)[0] == MRBO_ERR_ARG
    # Periodic with nt = 1 keeps each entry's period, which must be positive in every entry
    rc, msg = _fit_multi([_desc(kernel=4), _desc(kernel=4, period=0.0)], nt=1)
    assert rc == MRBO_ERR_ARG and b"period" in msg


def test_fit_multi_null_arguments():
    from mrbo import _lib
    L = _lib.load()
    assert L.mrbo_gp_fit_multi(None, 1, 1, 1, None, None, None, None, None, None, 0, None) == MRBO_ERR_ARG


def _surrogates(S, d=2, N=6, kernel=None, sn2=1e-6):
    from mrbo.kernels import Matern52
    from mrbo.surrogates import Surrogate
    from mrbo.utils import kronecker_quasirand
    out = []
    for q in range(S):
        X = kronecker_quasirand(d, N, 11 * q)
        out.append(Surrogate((kernel or Matern52)((1.0 + 0.1 * q,)), X, np.sin(X.sum(axis=0)), capacity=N, σn2=sn2))
    return out


def test_gp_fit_multi_checks_its_list():
    from mrbo.kernels import SquaredExponential
    from mrbo.mle import gp_fit_multi, optimize_multi
    ss = _surrogates(2)
    th = np.ones((3, 4))
    with pytest.raises(ValueError, match="at least one"):
        gp_fit_multi([], th)
    with pytest.raises(ValueError, match="surrogate 2 has d = 2, N = 5"):
        gp_fit_multi(ss + _surrogates(1, N=5), th)
    with pytest.raises(ValueError, match="surrogate 1 has d = 3"):
        gp_fit_multi(ss[:1] + _surrogates(1, d=3) + ss[1:], th)
    with pytest.raises(ValueError, match="surrogate 2 differs .* kernel family"):
        gp_fit_multi(ss + _surrogates(1, kernel=SquaredExponential), th)
    with pytest.raises(ValueError, match="surrogate 2 differs .* σn2"):
        gp_fit_multi(ss + _surrogates(1, sn2=1e-4), th)
    with pytest.raises(ValueError, match=r"\(S, P\)"):
        gp_fit_multi(ss, np.ones((3, 4)))            # three θ blocks for two surrogates
    with pytest.raises(ValueError, match="surrogate 2 has d = 2, N = 5"):
        optimize_multi(ss + _surrogates(1, N=5), [0.1], [5.0])


# ---- projected_lbfgs_multi on numpy objectives ------------------------------------------------
def _quadratic(A, c):
    """f(x) = (x − c)ᵀA(x − c)/2 and its gradient for the rows of a (P, 2) array."""
    A, c = np.asarray(A, float), np.asarray(c, float)

    def fg(X):
        R = X - c
        G = R @ A
        return 0.5 * (R * G).sum(axis=1), G
    return fg


# conditioning 5, 30 and 3000 (the last rotated): they stop after different iteration counts.  The
# second starts ON the upper bound of x₀ with its minimiser beyond it, so that bound is active from
# the first iteration on (and the problem left is one-dimensional: it stops first).
_ROT = np.array([[np.cos(0.6), -np.sin(0.6)], [np.sin(0.6), np.cos(0.6)]])
PROBLEMS = [
    (_quadratic(np.diag([1.0, 5.0]), [0.3, -0.2]), np.array([1.5, 1.0])),
    (_quadratic(np.diag([1.0, 30.0]), [3.0, 0.4]), np.array([2.0, -1.5])),
    (_quadratic(_ROT @ np.diag([1.0, 3000.0]) @ _ROT.T, [-0.5, 0.7]), np.array([1.0, -1.0])),
]
LO, HI = [-2.0, -2.0], [2.0, 2.0]


def _recording(fgs, log):
    def fg_multi(idx, X):
        log.append((list(idx), X.shape))
        r = [fgs[i](X[k]) for k, i in enumerate(idx)]
        return np.stack([f for f, _ in r]), np.stack([g for _, g in r])
    return fg_multi


def _same(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2]) and a[3] == b[3]


def test_projected_lbfgs_multi_equals_the_single_runs():
    from mrbo.mle import _STEPS, projected_lbfgs, projected_lbfgs_multi
    fgs = [fg for fg, _ in PROBLEMS]
    x0s = [x0 for _, x0 in PROBLEMS]
    log = []
    res = projected_lbfgs_multi(_recording(fgs, log), x0s, LO, HI, iterations=30)
    alone = [projected_lbfgs(fg, x0, LO, HI, iterations=30) for fg, x0 in PROBLEMS]
    its = [r[3] for r in res]
    assert len(set(its)) == 3, its                    # they really stop at different rounds
    for r, a in zip(res, alone):
        assert _same(r, a), (r, a)
    assert res[1][0][0] == 2.0 and res[1][2][0] < 0   # ends on the bound it started on, gradient outward
    # every call: one P for all active problems -- the starts, then line searches -- and only
    # problems that have not stopped: problem i is in exactly its[i] line-search rounds (every
    # counted iteration makes one line search, and a stopped problem asks for nothing more)
    assert log[0] == ([0, 1, 2], (3, 1, 2))
    for idx, shape in log[1:]:
        assert shape == (len(idx), len(_STEPS), 2)
    rounds = [sum(i in idx for idx, _ in log[1:]) for i in range(3)]
    assert rounds == its, (its, rounds)
    for (a, _), (b, _) in zip(log[1:], log[2:]):
        assert set(b) <= set(a)                        # a stopped problem never comes back
    assert len(log) == 1 + max(rounds)                 # the loop ends with the last active problem


def test_projected_lbfgs_multi_isolates_a_problem_without_a_step():
    """A problem whose objective is NaN at every trial point finds no Armijo step and stops alone,
    at its start; the others run on as they do without it."""
    from mrbo.mle import projected_lbfgs, projected_lbfgs_multi

    def nan_trials(X):
        f, g = PROBLEMS[0][0](X)
        return (f, g) if len(X) == 1 else (np.full(len(X), np.nan), g)

    fgs = [PROBLEMS[1][0], nan_trials, PROBLEMS[2][0]]
    x0s = [PROBLEMS[1][1], np.array([1.5, 1.0]), PROBLEMS[2][1]]
    log = []
    res = projected_lbfgs_multi(_recording(fgs, log), x0s, LO, HI, iterations=30)
    alone = [projected_lbfgs(fg, x0, LO, HI, iterations=30) for fg, x0 in zip(fgs, x0s)]
    for r, a in zip(res, alone):
        assert _same(r, a), (r, a)
    assert np.array_equal(res[1][0], x0s[1]) and np.isfinite(res[1][1])
    assert [idx for idx, _ in log[:3]] == [[0, 1, 2], [0, 1, 2], [0, 2]]


def test_projected_lbfgs_multi_budget_and_empty():
    from mrbo.mle import projected_lbfgs, projected_lbfgs_multi
    fgs = [fg for fg, _ in PROBLEMS]
    x0s = [x0 for _, x0 in PROBLEMS]
    log = []
    res = projected_lbfgs_multi(_recording(fgs, log), x0s, LO, HI, iterations=2)
    assert [r[3] for r in res] == [min(2, projected_lbfgs(fg, x0, LO, HI)[3]) for fg, x0 in PROBLEMS]
    assert len(log) <= 3
    assert projected_lbfgs_multi(_recording(fgs, log), [], LO, HI) == []
