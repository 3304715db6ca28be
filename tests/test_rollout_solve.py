"""The device-resident acquisition solve (mrbo_box_adam_step, mrbo_pick_restart, mrbo_rollout_solve,
include/mrbo.h), the host side: the argument checks of the three entry points.  Every one of them
returns before the plan is read and before any HIP call, so the tests run without a GPU and hand the
library a stand-in plan pointer (a few zero bytes that nothing dereferences).  The device side is
tests/test_gpu_rollout_solve.py."""
import ctypes
import inspect

import numpy as np
import pytest

import conftest  # noqa: F401  (sys.path)

MRBO_ERR_ARG = -1
_BUF = np.zeros(64)                                   # every array argument: never read or written
_PLAN = ctypes.create_string_buffer(64)               # the stand-in plan


def _p(null=False):
    return None if null else ctypes.c_void_p(_BUF.ctypes.data)


def _plan(null=False):
    return None if null else ctypes.cast(_PLAN, ctypes.c_void_p)


# ---- mrbo_box_adam_step --------------------------------------------------------------------------
def _step(null=(), t=1, sample_size=16.0, eta=0.02, beta1=0.9, beta2=0.999, eps=1e-8, flags=0):
    from mrbo import _lib
    L = _lib.load()
    a = {k: _p(k in null) for k in ("eto", "x0s", "active", "m", "v")}
    rc = L.mrbo_box_adam_step(_plan("plan" in null), a["eto"], a["x0s"], a["active"], a["m"], a["v"], t, sample_size,
                              eta, beta1, beta2, eps, flags, None)
    return rc, L.mrbo_last_error()


@pytest.mark.parametrize("name", ["plan", "eto", "x0s", "active", "m", "v"])
def test_box_adam_step_rejects_null_arguments(name):
    rc, msg = _step(null=(name,))
    assert rc == MRBO_ERR_ARG and b"null" in msg, msg


@pytest.mark.parametrize("kw,what", [
    (dict(t=0), b"t=0"), (dict(t=-3), b"t=-3"),
    (dict(eta=-0.1), b"eta"), (dict(eta=np.nan), b"eta"), (dict(eta=np.inf), b"eta"),
    (dict(eps=-1e-8), b"eps"), (dict(eps=np.nan), b"eps"), (dict(eps=np.inf), b"eps"),
    (dict(sample_size=-1.0), b"sample_size"), (dict(sample_size=np.nan), b"sample_size"),
    (dict(sample_size=np.inf), b"sample_size"),
    (dict(beta1=1.0), b"beta1"), (dict(beta1=-0.1), b"beta1"), (dict(beta1=np.nan), b"beta1"),
    (dict(beta2=1.0), b"beta2"), (dict(beta2=-0.1), b"beta2"), (dict(beta2=np.nan), b"beta2"),
    (dict(flags=1), b"flags"), (dict(flags=2), b"flags"),
])
def test_box_adam_step_rejects_values_out_of_range(kw, what):
    rc, msg = _step(**kw)
    assert rc == MRBO_ERR_ARG and what in msg, msg


# ---- mrbo_pick_restart ---------------------------------------------------------------------------
def _pick(null=(), flags=0):
    from mrbo import _lib
    L = _lib.load()
    a = {k: _p(k in null) for k in ("x", "eto", "xnext", "mean", "pick", "means")}
    rc = L.mrbo_pick_restart(_plan("plan" in null), a["x"], a["eto"], 1, a["xnext"], a["mean"], a["pick"], a["means"],
                             flags, None)
    return rc, L.mrbo_last_error()


@pytest.mark.parametrize("name", ["plan", "x", "eto", "xnext", "mean", "pick"])
def test_pick_restart_rejects_null_arguments(name):
    rc, msg = _pick(null=(name,))
    assert rc == MRBO_ERR_ARG and b"null" in msg, msg


@pytest.mark.parametrize("flags", [1, 2, 4])
def test_pick_restart_rejects_flags(flags):
    rc, msg = _pick(flags=flags)
    assert rc == MRBO_ERR_ARG and b"flags" in msg, msg


# ---- mrbo_rollout_solve --------------------------------------------------------------------------
def _solve(null=(), flags=1, optimizer=2, iterations=12, eta=0.02, beta1=0.9, beta2=0.999, eps=1e-8, sample_size=0.0,
           incumbent=1):
    from mrbo import _lib
    L = _lib.load()
    a = {k: _p(k in null) for k in ("x0s", "rnstream", "xstarts", "xnext", "mean", "pick", "means", "active")}
    o = _lib.RolloutOpts(optimizer, iterations, eta, beta1, beta2, eps, sample_size, incumbent)
    res = (ctypes.c_int32 * 4)()
    rc = L.mrbo_rollout_solve(_plan("plan" in null), a["x0s"], a["rnstream"], a["xstarts"],
                              None if "opts" in null else ctypes.byref(o), a["xnext"], a["mean"], a["pick"],
                              a["means"], a["active"], None if "result" in null else res, flags, None)
    return rc, L.mrbo_last_error()


@pytest.mark.parametrize("name", ["plan", "x0s", "rnstream", "xstarts", "opts", "xnext", "mean", "pick", "result"])
def test_rollout_solve_rejects_null_arguments(name):
    rc, msg = _solve(null=(name,))
    assert rc == MRBO_ERR_ARG and b"null" in msg, msg


@pytest.mark.parametrize("kw,what", [
    (dict(iterations=0), b"iterations=0"), (dict(iterations=-1), b"iterations=-1"),
    (dict(optimizer=3), b"optimizer=3"), (dict(optimizer=-1), b"optimizer=-1"),
    (dict(eta=-0.1), b"eta"), (dict(eta=np.nan), b"eta"), (dict(eta=np.inf), b"eta"),
    (dict(eps=-1e-8), b"eps"), (dict(eps=np.nan), b"eps"), (dict(eps=np.inf), b"eps"),
    (dict(sample_size=-1.0), b"sample_size"), (dict(sample_size=np.nan), b"sample_size"),
    (dict(sample_size=np.inf), b"sample_size"),
    (dict(beta1=1.0), b"beta1"), (dict(beta1=-0.1), b"beta1"), (dict(beta1=np.nan), b"beta1"),
    (dict(beta2=1.0), b"beta2"), (dict(beta2=-0.1), b"beta2"), (dict(beta2=np.nan), b"beta2"),
    (dict(flags=2), b"flags"), (dict(flags=3), b"flags"), (dict(flags=4), b"flags"),
])
def test_rollout_solve_rejects_values_out_of_range(kw, what):
    rc, msg = _solve(**kw)
    assert rc == MRBO_ERR_ARG and what in msg, msg


@pytest.mark.parametrize("optimizer", [0, 1, 2])
def test_rollout_solve_checks_every_optimizer_alike(optimizer):
    """The option checks do not depend on the optimizer (StandardSGA ignores β and ε, but a value
    outside the range is refused all the same)."""
    assert _solve(optimizer=optimizer, beta1=1.5)[0] == MRBO_ERR_ARG
    assert _solve(optimizer=optimizer, iterations=0)[0] == MRBO_ERR_ARG


# ---- what stays as it was ------------------------------------------------------------------------
def test_stochastic_solve_still_refuses_box_adam():
    from mrbo import _lib
    L = _lib.load()
    assert _lib.MRBO_OPT_BOX_ADAM == 2
    o = _lib.SolveOpts(_lib.MRBO_OPT_BOX_ADAM, 12, 0.02, 0.9, 0.999, 1e-8, 0.0)
    res = (ctypes.c_int32 * 3)()
    rc = L.mrbo_stochastic_solve(_plan(), _p(), _p(), _p(), None, ctypes.byref(o), None, None, res,
                                 _lib.MRBO_FLAG_HOST_POINTERS, None)
    assert rc == MRBO_ERR_ARG and b"optimizer=2 unknown" in L.mrbo_last_error()


def test_cli_accepts_device_solve():
    from mrbo import bayesopt
    base = ["--output-dir", "out", "--function-name", "gramacylee"]
    assert bayesopt.parse(base).device_solve is False
    assert bayesopt.parse(base + ["--device-solve"]).device_solve is True


@pytest.mark.parametrize("name", ["rollout_solve", "rollout_solve_multi", "run"])
def test_device_solve_is_off_by_default(name):
    from mrbo import bayesopt
    assert inspect.signature(getattr(bayesopt, name)).parameters["device_solve"].default is False


def test_rollout_opts_mirror_the_c_struct():
    """mrbo_rollout_opts_t: two int32, five doubles, one int32 (padded to the doubles' alignment)."""
    from mrbo import _lib
    f = _lib.RolloutOpts
    assert [n for n, _ in f._fields_] == ["optimizer", "iterations", "eta", "beta1", "beta2", "eps", "sample_size",
                                          "incumbent"]
    assert (f.eta.offset, f.sample_size.offset, f.incumbent.offset, ctypes.sizeof(f)) == (8, 40, 48, 56)
