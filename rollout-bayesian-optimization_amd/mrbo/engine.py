"""RolloutPlan -- owns one libmrbo plan (device copy of the base surrogate + workspace) and
launches the rollout kernel on device-resident torch tensors.

torch is plumbing here (device memory, streams, torch.distributed); every arithmetic step of
the rollout path runs in libmrbo.so.
"""
import ctypes

import numpy as np

from . import _lib

DEFAULTS = dict(max_iters=50, max_ls=20, x_tol=1e-3, f_tol=1e-3, g_tol=1e-8, htol=1e-4, sigma_tol=1e-8, seed=1906,
                sample_offset=0, samples_total=0, cost="none", cost_c0=1.0, cost_w=())


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise _lib.MrboError("libmrbo requires a ROCm GPU (torch.cuda.is_available() is False); there is no CPU path")
    return torch


def _f64(a):
    return np.asfortranarray(np.asarray(a, dtype=np.float64))


def to_device(a, device):
    """numpy (any order) -> flat column-major float64 device tensor"""
    torch = _torch()
    flat = np.asarray(a, dtype=np.float64).ravel(order="F").copy()
    return torch.from_numpy(flat).to(device)


def from_device(t, shape):
    return t.detach().cpu().numpy().reshape(shape, order="F")


def check_bounds(lbs, ubs, d, S):
    """The bounds of a plan for S surrogates of dimension d: both (d,) -- one shared box, returns
    False -- or both (d, S) -- per-surrogate boxes, returns True.  Anything else, a mix of the two
    included, is a ValueError."""
    sl, su = np.shape(lbs), np.shape(ubs)
    if sl == (d,) and su == (d,):
        return False
    if sl == (d, S) and su == (d, S):
        return True
    raise ValueError(f"bounds must both be (d,) = {(d,)} (a shared box) or both (d, S) = {(d, S)} (one box per "
                     f"surrogate); got lbs {sl}, ubs {su}")


SURROGATE_KEYS = ("X", "L", "c", "y", "kernel", "lengthscale", "fmini")   # + sigma_n2, period (optional)


class RolloutPlan:
    """Device state for (surrogate, trajectory parameters)."""

    def __init__(self, X, L, c, y, kernel, lengthscale, sigma_n2, fmini, h, M, R, nstarts, lbs, ubs, theta,
                 device=0, period=1.0, **opts):
        self._create([dict(X=X, L=L, c=c, y=y, kernel=kernel, lengthscale=lengthscale, sigma_n2=sigma_n2,
                           fmini=fmini, period=period)], h, M, R, nstarts, lbs, ubs, theta, device, opts)

    @classmethod
    def from_surrogates(cls, surrogates, h, M, R, nstarts, lbs, ubs, theta, device=0, **opts):
        """A surrogate batch (mrbo_plan_create_batch): ONE plan and one launch per call for the S base
        surrogates of `surrogates`, each a mapping with X (d×N), L, c, y, kernel, lengthscale, fmini
        and optionally sigma_n2 (default 1e-6) and period (default 1).  They share d, N, kernel and
        sigma_n2; R is the number of restarts PER surrogate, and everything else is shared.  Inputs
        and outputs carry the surrogate index slowest (x0s d×R×S, values M×R×S, ...); block q of every
        output is bit-identical to a plain plan on surrogate q.

        lbs, ubs of shape (d,): one box shared by all.  Shape (d, S): a boxed plan
        (mrbo_plan_create_batch_boxes), surrogate q on its own box [lbs[:, q], ubs[:, q]]; every
        xstarts argument of its calls is then d×nstarts×S (base solves: d×n×S), block q the inner
        starts of surrogate q, and block q of every output is bit-identical to a plain plan on
        surrogate q over box q with starts q."""
        surrogates = list(surrogates)
        if not surrogates:
            raise ValueError("from_surrogates needs at least one surrogate")
        for q, s in enumerate(surrogates):
            missing = [k for k in SURROGATE_KEYS if k not in s]
            if missing:
                raise ValueError(f"surrogate {q} lacks {missing}")
        self = cls.__new__(cls)
        self._create(surrogates, h, M, R, nstarts, lbs, ubs, theta, device, opts)
        return self

    def _create(self, surrogates, h, M, R, nstarts, lbs, ubs, theta, device, opts):
        """The plan of the surrogate mappings `surrogates` (a plain plan: one), mrbo_plan_create_batch."""
        self.lib = _lib.load()
        self.S = len(surrogates)
        dp = ctypes.POINTER(ctypes.c_double)
        self._keep = []     # the host arrays the descriptors point into, alive until the create returns
        sds = (_lib.SurrogateDesc * self.S)()
        for q, s in enumerate(surrogates):
            X, L, c, y = _f64(s["X"]), _f64(s["L"]), _f64(s["c"]).ravel(), _f64(s["y"]).ravel()
            if X.ndim != 2 or L.shape != (X.shape[1], X.shape[1]) or c.size != X.shape[1] or y.size != X.shape[1]:
                raise ValueError(f"surrogate {q}: X is {X.shape}, L {L.shape}, c {c.size}, y {y.size}")
            self._keep.append((X, L, c, y))
            sds[q] = _lib.SurrogateDesc(X.shape[0], X.shape[1], int(s["kernel"]), float(s["lengthscale"]),
                                        float(s.get("sigma_n2", 1e-6)), float(s["fmini"]), X.ctypes.data_as(dp),
                                        L.ctypes.data_as(dp), X.shape[1], c.ctypes.data_as(dp), y.ctypes.data_as(dp),
                                        float(s.get("period", 1.0)))
        self._X, self._L, self._c, self._y = self._keep[0]
        self.d, self.N = self._X.shape
        per_surrogate = check_bounds(lbs, ubs, self.d, self.S)
        pd = self._params(h, M, R, nstarts, lbs, ubs, theta, device, opts)
        h_ = ctypes.c_void_p()
        if per_surrogate:
            _lib.check(self.lib.mrbo_plan_create_batch_boxes(sds, self.S, ctypes.byref(pd), self._lbs.ctypes.data_as(dp),
                                                             self._ubs.ctypes.data_as(dp), int(device),
                                                             ctypes.byref(h_)))
        else:
            _lib.check(self.lib.mrbo_plan_create_batch(sds, self.S, ctypes.byref(pd), int(device), ctypes.byref(h_)))
        self.handle = h_

    def _params(self, h, M, R, nstarts, lbs, ubs, theta, device, opts):
        """mrbo_params_t of the plan (and the plan's own copies of the sizes)."""
        o = dict(DEFAULTS)
        o.update(opts)
        self.opts = o
        self.h, self.M, self.R, self.nstarts = int(h), int(M), int(R), int(nstarts)
        # flat column-major: d on a shared box, d×S (surrogate slowest) with per-surrogate boxes
        self._lbs, self._ubs = _f64(lbs).ravel(order="F"), _f64(ubs).ravel(order="F")
        # a boxed plan: S > 1 surrogates on their own boxes (one surrogate on "its own" box is the plain plan)
        self.boxed = np.ndim(lbs) == 2 and self.S > 1
        self.theta = float(theta)
        self.device = device
        dp = ctypes.POINTER(ctypes.c_double)
        ck = _lib.COSTS[o["cost"]] if isinstance(o["cost"], str) else int(o["cost"])
        self._cost_w = _f64(o["cost_w"]).ravel() if ck else None
        if ck and self._cost_w.size != self.d:
            raise ValueError(f"cost_w has {self._cost_w.size} weights for d = {self.d}")
        pd = _lib.ParamsDesc(self.h, self.M, self.R, self.nstarts, int(o.get("rule", 0)), self.theta,
                             self._lbs.ctypes.data_as(dp),
                             self._ubs.ctypes.data_as(dp), int(o["max_iters"]), int(o["max_ls"]), float(o["x_tol"]),
                             float(o["f_tol"]), float(o["g_tol"]), float(o["htol"]), float(o["sigma_tol"]),
                             int(o["seed"]), int(o.get("sample_offset", 0)), int(o.get("samples_total", 0)),
                             ck, float(o["cost_c0"]), self._cost_w.ctypes.data_as(dp) if ck else None)
        return pd

    @property
    def boxes(self):
        """The plan's bounds as given: ((d,), (d,)) on a shared box, ((d, S), (d, S)) on a boxed plan."""
        if not self.boxed:
            return self._lbs[:self.d].copy(), self._ubs[:self.d].copy()
        shape = (self.d, self.S)
        return self._lbs.reshape(shape, order="F").copy(), self._ubs.reshape(shape, order="F").copy()

    def check_xstarts(self, xstarts, n=None):
        """On a boxed plan the inner starts are d×n×S (n: the plan's nstarts; a base solve's own
        count), as an array of that shape or flat column-major.  Raises ValueError otherwise; a
        plan with a shared box takes what it always took."""
        if not getattr(self, "boxed", False) or xstarts is None:
            return
        n = self.nstarts if n is None else int(n)
        want = (self.d, n, self.S)
        shape = tuple(xstarts.shape)
        if shape != want and shape != (self.d * n * self.S,):
            raise ValueError(f"a boxed plan takes inner starts d×n×S = {want}, one block per surrogate; "
                             f"got {shape}")

    def close(self):
        if getattr(self, "handle", None):
            self.lib.mrbo_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---------------------------------------------------------------------------------
    def alloc_outputs(self, with_gradient=True, want_policy=False, want_obs=False, want_evals=True):
        torch = _torch()
        dev = f"cuda:{self.device}"
        T = self.M * self.R * self.S
        out = dict(values=torch.empty(T, dtype=torch.float64, device=dev),
                   status=torch.empty(T, dtype=torch.int32, device=dev))
        if with_gradient:
            out["grad_x"] = torch.empty(self.d * T, dtype=torch.float64, device=dev)
            out["grad_theta"] = torch.empty(T, dtype=torch.float64, device=dev)
        if want_policy:
            out["policy_x"] = torch.empty(self.d * (self.h + 1) * T, dtype=torch.float64, device=dev)
        if want_obs:
            out["obs"] = torch.empty((self.h + 1) * T, dtype=torch.float64, device=dev)
        if want_evals:
            out["evals"] = torch.empty(_lib.NCOUNTERS * T, dtype=torch.int64, device=dev)
        return out

    def simulate(self, x0s, rnstream, xstarts, out, dual_y_dx=None, replay_x=None, stream=None):
        """Launch mrbo_simulate_mc on device tensors (flat, column-major)."""
        self.check_xstarts(xstarts)
        torch = _torch()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        flags = 0 if "grad_x" in out else _lib.MRBO_FLAG_NO_GRADIENT
        _lib.check(self.lib.mrbo_simulate_mc(
            self.handle, p(x0s), p(rnstream), p(xstarts), p(dual_y_dx), p(replay_x), p(out["values"]),
            p(out.get("grad_x")), p(out.get("grad_theta")), p(out["status"]), p(out.get("policy_x")),
            p(out.get("obs")), p(out.get("evals")), flags, ctypes.c_void_p(st.cuda_stream)))
        return out

    def simulate_ghq(self, x0s, nodes, weights, xstarts, out, dual_y_dx=None, replay_x=None, stream=None):
        """Launch mrbo_simulate_ghq: nodes / weights are M×(h+1) device tensors (flat, column-major)."""
        self.check_xstarts(xstarts)
        torch = _torch()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        flags = 0 if "grad_x" in out else _lib.MRBO_FLAG_NO_GRADIENT
        _lib.check(self.lib.mrbo_simulate_ghq(
            self.handle, p(x0s), p(nodes), p(weights), p(xstarts), p(dual_y_dx), p(replay_x), p(out["values"]),
            p(out.get("grad_x")), p(out.get("grad_theta")), p(out["status"]), p(out.get("policy_x")),
            p(out.get("obs")), p(out.get("evals")), flags, ctypes.c_void_p(st.cuda_stream)))
        return out

    def eto(self, out, stream=None):
        torch = _torch()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        W = 2 + 2 * self.d + 2
        e = torch.empty(W * self.R * self.S, dtype=torch.float64, device=f"cuda:{self.device}")
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        _lib.check(self.lib.mrbo_eto_reduce(self.handle, p(out["values"]), p(out.get("grad_x")),
                                            p(out.get("grad_theta")), p(e), 0, ctypes.c_void_p(st.cuda_stream)))
        return e

    # ---- the EI control variate (the specification is mrbo/variance.py) ----------
    def alloc_control(self, with_gradient=True):
        """Device outputs of simulate_control: values0, status0 and, with_gradient, grad_x0."""
        torch = _torch()
        dev = f"cuda:{self.device}"
        T = self.M * self.R * self.S
        out = dict(values0=torch.empty(T, dtype=torch.float64, device=dev),
                   status0=torch.empty(T, dtype=torch.int32, device=dev))
        if with_gradient:
            out["grad_x0"] = torch.empty(self.d * T, dtype=torch.float64, device=dev)
        return out

    def simulate_control(self, x0s, rnstream, xstarts, ctl=None, with_gradient=True, stream=None):
        """mrbo_simulate_control on device tensors: the plan's rollout launch run to horizon 0 -- the
        control samples of the trajectories `simulate` runs from the same x0s and rnstream (the
        plan's full stream: its step-0 slab is read).  ctl: the dict of alloc_control (allocated
        when None; without "grad_x0" the launch takes MRBO_FLAG_NO_GRADIENT)."""
        self.check_xstarts(xstarts)
        torch = _torch()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        if ctl is None:
            ctl = self.alloc_control(with_gradient)
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        flags = 0 if "grad_x0" in ctl else _lib.MRBO_FLAG_NO_GRADIENT
        _lib.check(self.lib.mrbo_simulate_control(self.handle, p(x0s), p(rnstream), p(xstarts), p(ctl["values0"]),
                                                  p(ctl.get("grad_x0")), p(ctl["status0"]), flags,
                                                  ctypes.c_void_p(st.cuda_stream)))
        return ctl

    def eto_cv(self, x0s, out, ctl, want_beta=True, stream=None):
        """mrbo_eto_reduce_cv: the ETO rows of `out` (simulate) with `ctl` (simulate_control at the
        same x0s) as the control.  Returns (eto W·R·S, beta (1+d)·R·S or None), device tensors."""
        torch = _torch()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        dev = f"cuda:{self.device}"
        W = 2 + 2 * self.d + 2
        e = torch.empty(W * self.R * self.S, dtype=torch.float64, device=dev)
        b = torch.empty((1 + self.d) * self.R * self.S, dtype=torch.float64, device=dev) if want_beta else None
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        _lib.check(self.lib.mrbo_eto_reduce_cv(self.handle, p(x0s), p(out["values"]), p(out.get("grad_x")),
                                               p(out.get("grad_theta")), p(ctl["values0"]), p(ctl.get("grad_x0")),
                                               p(e), p(b), 0, ctypes.c_void_p(st.cuda_stream)))
        return e, b

    def set_control_variate(self, on):
        """mrbo_plan_set_control_variate: rollout_solve's rows become eto_cv's (default off)."""
        _lib.check(self.lib.mrbo_plan_set_control_variate(self.handle, int(bool(on))))

    def partial_moments(self, out, M_local, stream=None):
        """mrbo_partial_moments: this shard's (W·R) [Σ, M2] rows, device tensor (parallel.py)."""
        torch = _torch()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        W = 2 + 2 * self.d + 2
        e = torch.empty(W * self.R * self.S, dtype=torch.float64, device=f"cuda:{self.device}")
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        _lib.check(self.lib.mrbo_partial_moments(self.handle, p(out["values"]), p(out.get("grad_x")),
                                              p(out.get("grad_theta")), int(M_local), p(e), 0,
                                              ctypes.c_void_p(st.cuda_stream)))
        return e

    def merge_moments(self, gathered, counts, stream=None):
        """mrbo_merge_moments: gathered = the ranks' partial_moments blocks concatenated in rank
        order (one flat device tensor of len(counts)·W·R), counts = their sample counts; returns
        the merged ETO rows (device tensor, eto()'s layout)."""
        torch = _torch()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        W = 2 + 2 * self.d + 2
        n = len(counts)
        if gathered.numel() != n * W * self.R * self.S or not gathered.is_cuda:
            raise ValueError(f"gathered must be a device tensor of {n}·{W}·{self.R * self.S} moments")
        e = torch.empty(W * self.R * self.S, dtype=torch.float64, device=f"cuda:{self.device}")
        c = (ctypes.c_int64 * n)(*[int(k) for k in counts])
        _lib.check(self.lib.mrbo_merge_moments(self.handle, n, ctypes.c_void_p(gathered.data_ptr()), c,
                                               ctypes.c_void_p(e.data_ptr()), 0, ctypes.c_void_p(st.cuda_stream)))
        return e

    def sga_step(self, eto, x0s, active, sample_size, eta, stream=None):
        """mrbo_sga_step: eswavs + StandardSGA for every active restart, in place on the device
        tensors x0s (d·R, column-major) and active (R, int32); eto from `eto()`."""
        torch = _torch()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        _lib.check(self.lib.mrbo_sga_step(self.handle, p(eto), p(x0s), p(active), float(sample_size), float(eta), 0,
                                          ctypes.c_void_p(st.cuda_stream)))

    def adam_step(self, eto, x0s, active, m, v, t, sample_size, eta=0.001, beta1=0.9, beta2=0.999, eps=1e-8,
                  stream=None):
        """mrbo_adam_step: eswavs + Adam update! (optimizers.jl:49-74) for every active restart, in
        place on the device tensors x0s, m, v (d·R, column-major, m = v = 0 before update 1) and
        active (R, int32); t is this update's count (1, 2, ...)."""
        torch = _torch()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        p = lambda t_: ctypes.c_void_p(t_.data_ptr())
        _lib.check(self.lib.mrbo_adam_step(self.handle, p(eto), p(x0s), p(active), p(m), p(v), int(t),
                                           float(sample_size), float(eta), float(beta1), float(beta2), float(eps), 0,
                                           ctypes.c_void_p(st.cuda_stream)))

    def stochastic_solve(self, x0s, rnstream, xstarts, optimizer="sga", iterations=50, eta=None, beta1=0.9,
                         beta2=0.999, eps=1e-8, sample_size=0, eto=None, active=None, dual_y_dx=None, stream=None):
        """mrbo_stochastic_solve on device tensors: the whole outer ascent (utils.jl:235-265) for the
        plan's R restarts in one call; x0s (d·R, column-major) is updated in place, eto (W·R) and
        active (R, int32) receive the final rows and stop flags when given.  Returns (iterations
        launched, iteration after which no restart was active, OR of the status bits)."""
        self.check_xstarts(xstarts)
        torch = _torch()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        p = lambda t_: None if t_ is None else ctypes.c_void_p(t_.data_ptr())
        opt = _lib.MRBO_OPT_SGA if optimizer == "sga" else _lib.MRBO_OPT_ADAM
        eta = (0.01 if opt == _lib.MRBO_OPT_SGA else 0.001) if eta is None else eta
        o = _lib.SolveOpts(opt, int(iterations), float(eta), float(beta1), float(beta2), float(eps), float(sample_size))
        res = (ctypes.c_int32 * 3)()
        _lib.check(self.lib.mrbo_stochastic_solve(self.handle, p(x0s), p(rnstream), p(xstarts), p(dual_y_dx),
                                                  ctypes.byref(o), p(eto), p(active), res, 0,
                                                  ctypes.c_void_p(st.cuda_stream)))
        return int(res[0]), int(res[1]), int(res[2])

    def box_adam_step(self, eto, x0s, active, m, v, t, sample_size, eta=0.02, beta1=0.9, beta2=0.999, eps=1e-8,
                      stream=None):
        """mrbo_box_adam_step: eswavs + BoxAdam.update (mrbo/bayesopt.py) over the plan's box -- on a
        boxed plan the box of the restart's surrogate -- for every active restart, in place on the
        device tensors of adam_step."""
        torch = _torch()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        p = lambda t_: ctypes.c_void_p(t_.data_ptr())
        _lib.check(self.lib.mrbo_box_adam_step(self.handle, p(eto), p(x0s), p(active), p(m), p(v), int(t),
                                               float(sample_size), float(eta), float(beta1), float(beta2),
                                               float(eps), 0, ctypes.c_void_p(st.cuda_stream)))

    def pick_restart(self, x, eto, incumbent=True, means=None, stream=None):
        """mrbo_pick_restart on device tensors: x (d·R·S, column-major), eto from `eto()`; means (R·S)
        receives the restarts' means when given.  Returns the device tensors (xnext d·S, mean S,
        pick int32 S); asynchronous."""
        torch = _torch()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        dev = f"cuda:{self.device}"
        xnext = torch.empty(self.d * self.S, dtype=torch.float64, device=dev)
        mean = torch.empty(self.S, dtype=torch.float64, device=dev)
        pick = torch.empty(self.S, dtype=torch.int32, device=dev)
        p = lambda t_: None if t_ is None else ctypes.c_void_p(t_.data_ptr())
        _lib.check(self.lib.mrbo_pick_restart(self.handle, p(x), p(eto), int(bool(incumbent)), p(xnext), p(mean),
                                              p(pick), p(means), 0, ctypes.c_void_p(st.cuda_stream)))
        return xnext, mean, pick

    OPTIMIZERS = {"sga": _lib.MRBO_OPT_SGA, "adam": _lib.MRBO_OPT_ADAM, "box_adam": _lib.MRBO_OPT_BOX_ADAM}

    def _rollout_opts(self, optimizer, iterations, eta, beta1, beta2, eps, sample_size, incumbent):
        opt = self.OPTIMIZERS[optimizer]
        eta = {"sga": 0.01, "adam": 0.001, "box_adam": 0.02}[optimizer] if eta is None else eta
        return _lib.RolloutOpts(opt, int(iterations), float(eta), float(beta1), float(beta2), float(eps),
                                float(sample_size), int(bool(incumbent)))

    def rollout_solve(self, x0s, rnstream, xstarts, optimizer="sga", iterations=50, eta=None, beta1=0.9, beta2=0.999,
                      eps=1e-8, sample_size=0, incumbent=True, means=None, active=None, stream=None):
        """mrbo_rollout_solve on device tensors: the whole acquisition solve of a BO step -- the ascent
        of the plan's R·S restarts ("sga", "adam" or "box_adam"), the projection of x0s (d·R·S,
        column-major, updated in place) onto the box, the final evaluation and the pick -- in one
        call.  means (R·S) and active (R·S, int32) receive the final means and stop flags when given.
        Returns (xnext d·S, mean S, pick int32 S) as device tensors and the call's result (iterations
        launched, iteration after which no restart was active, status bits of the ascent, of the final
        launch); the stream is synchronised."""
        self.check_xstarts(xstarts)
        torch = _torch()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        dev = f"cuda:{self.device}"
        xnext = torch.empty(self.d * self.S, dtype=torch.float64, device=dev)
        mean = torch.empty(self.S, dtype=torch.float64, device=dev)
        pick = torch.empty(self.S, dtype=torch.int32, device=dev)
        p = lambda t_: None if t_ is None else ctypes.c_void_p(t_.data_ptr())
        o = self._rollout_opts(optimizer, iterations, eta, beta1, beta2, eps, sample_size, incumbent)
        res = (ctypes.c_int32 * 4)()
        _lib.check(self.lib.mrbo_rollout_solve(self.handle, p(x0s), p(rnstream), p(xstarts), ctypes.byref(o), p(xnext),
                                               p(mean), p(pick), p(means), p(active), res, 0,
                                               ctypes.c_void_p(st.cuda_stream)))
        return xnext, mean, pick, tuple(int(r) for r in res)

    def rollout_solve_host(self, x0s, rnstream, xstarts, optimizer="sga", iterations=50, eta=None, beta1=0.9,
                           beta2=0.999, eps=1e-8, sample_size=0, incumbent=True, stream=None):
        """rollout_solve on numpy arrays (MRBO_FLAG_HOST_POINTERS: the library stages them once): x0s
        d×R×S (d×R on a plain plan), rnstream M×(d+1)×(h+1), xstarts d×nstarts (d×nstarts×S on a
        boxed plan).  Returns a dict of
        numpy arrays -- x (the projected end points, x0s's shape), xnext d×S, mean S, pick S, means
        R×S, active R×S -- and `result` as rollout_solve."""
        self.check_xstarts(xstarts)
        torch = _torch()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        d, R, S = self.d, self.R, self.S
        shape = np.shape(x0s)
        if shape not in ((d, R, S), (d, R * S)):
            raise ValueError(f"x0s must be d×R×S = {(d, R, S)}; got {shape}")
        x = np.asarray(x0s, dtype=np.float64).ravel(order="F").copy()
        rn = np.asarray(rnstream, dtype=np.float64).ravel(order="F")
        xs = np.asarray(xstarts, dtype=np.float64).ravel(order="F")
        if rn.size != self.M * (d + 1) * (self.h + 1) or xs.size != d * self.nstarts * (S if self.boxed else 1):
            raise ValueError(f"rnstream has {rn.size} entries, xstarts {xs.size}; the plan has M = {self.M}, "
                             f"h = {self.h}, {self.nstarts} inner starts")
        xnext, mean, means = np.empty(d * S), np.empty(S), np.empty(R * S)
        pick, active = np.empty(S, dtype=np.int32), np.empty(R * S, dtype=np.int32)
        p = lambda a: ctypes.c_void_p(a.ctypes.data)
        o = self._rollout_opts(optimizer, iterations, eta, beta1, beta2, eps, sample_size, incumbent)
        res = (ctypes.c_int32 * 4)()
        _lib.check(self.lib.mrbo_rollout_solve(self.handle, p(x), p(rn), p(xs), ctypes.byref(o), p(xnext), p(mean),
                                               p(pick), p(means), p(active), res, _lib.MRBO_FLAG_HOST_POINTERS,
                                               ctypes.c_void_p(st.cuda_stream)))
        return dict(x=x.reshape(shape, order="F"), xnext=xnext.reshape((d, S), order="F"), mean=mean, pick=pick,
                    means=means.reshape((R, S), order="F"), active=active.reshape((R, S), order="F"),
                    result=tuple(int(r) for r in res))

    def eval_base(self, xs):
        """eval(s, x, θ) at the columns of xs (d×P); returns (3+4d+d²)×P numpy -- on a surrogate
        batch (S > 1) the S blocks, (3+4d+d²)×P×S."""
        torch = _torch()
        xs = _f64(xs)
        d, P = xs.shape
        stride = 3 + 4 * d + d * d
        dx = to_device(xs, f"cuda:{self.device}")
        do = torch.empty(stride * P * self.S, dtype=torch.float64, device=f"cuda:{self.device}")
        st = torch.cuda.current_stream(self.device)
        _lib.check(self.lib.mrbo_eval_base(self.handle, P, ctypes.c_void_p(dx.data_ptr()),
                                           ctypes.c_void_p(do.data_ptr()), 0, ctypes.c_void_p(st.cuda_stream)))
        torch.cuda.synchronize(self.device)
        return from_device(do, (stride, P) if self.S == 1 else (stride, P, self.S))

    def last_kernel_ms(self):
        return self.lib.mrbo_last_kernel_ms(self.handle)

    def kernel_times(self, n):
        """mrbo_kernel_times: HIP-event durations (ms) of the rollout kernel alone in the plan's
        last min(n, launches, 64) mrbo_simulate_mc / _ghq launches, oldest first (waits for them)."""
        buf = (ctypes.c_double * max(int(n), 1))()
        k = self.lib.mrbo_kernel_times(self.handle, int(n), buf)
        _lib.check(min(k, 0))
        return [buf[i] for i in range(k)]

    # relative cost of one unit of each work counter (grad, value, hess, rich, pairs), in value
    # evaluations -- only the ORDER of the work depends on these, never a result
    ORDER_WEIGHTS = (2.5, 1.0, 3.0, 5.0, 3.0)

    def set_order(self, order, check=True):
        """mrbo_plan_set_order: an int32 device tensor holding a permutation of the M×R trajectory
        indices (m + M·r), or None for the identity.  The plan keeps a reference.  check=True
        refuses anything but a permutation (a duplicated index would run one trajectory on two waves
        at once and leave another unrun, its outputs undefined); check=False passes any order of the
        right length to the library (tests: the all-out-of-range guard)."""
        if self.S > 1:   # a surrogate batch has no work order: the library's MRBO_ERR_UNSUPPORTED
            _lib.check(self.lib.mrbo_plan_set_order(
                self.handle, None if order is None else ctypes.c_void_p(order.data_ptr()),
                0 if order is None else order.numel()))
        if order is None:
            _lib.check(self.lib.mrbo_plan_set_order(self.handle, None, 0))
            self._order = None
            return
        torch = _torch()
        if order.dtype != torch.int32 or not order.is_cuda or order.numel() != self.M * self.R:
            raise ValueError("order must be an int32 device tensor of M*R trajectory indices")
        if check and not torch.equal(torch.sort(order.to(torch.int64)).values,
                                     torch.arange(order.numel(), dtype=torch.int64, device=order.device)):
            raise ValueError("order is not a permutation of 0..M*R-1")
        self._order = order.contiguous()
        _lib.check(self.lib.mrbo_plan_set_order(self.handle, ctypes.c_void_p(self._order.data_ptr()),
                                                self._order.numel()))

    def order_longest_first(self, out, stream=None, order_out=None):
        """Schedule the next launches longest-first by the per-trajectory work counters of the
        launch that filled `out`: mrbo_plan_order_longest_first, on the device (no host round trip).
        Consecutive SGA steps move x0 a little and reuse the MC streams, so a trajectory's work
        repeats closely and the longest ones no longer start last (the launch's tail).

        The kernel's waves drain one queue per XCD over a contiguous eighth of the queue positions
        first (mrbo_rollout.hip rollout_kernel); the library re-orders each chunk's own trajectories
        longest first, so every XCD still writes the output rows of one contiguous index range
        (whole cache lines in one L2), and an XCD that drains its chunk early takes the short ends
        of the others.  The plan owns the order; order_out (int32 device tensor of M·R) receives a
        copy.  longest_first_order() is the torch mirror."""
        torch = _torch()
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        _lib.check(self.lib.mrbo_plan_order_longest_first(self.handle, p(out["evals"]), p(order_out),
                                                          ctypes.c_void_p(st.cuda_stream)))
        self._order = None

    @classmethod
    def longest_first_order(cls, evals):
        """Torch mirror of mrbo_plan_order_longest_first (longest_first_within_chunks of the
        integer work keys 2 × Σ ORDER_WEIGHTS · counters)."""
        import torch
        ev = evals.view(-1, _lib.NCOUNTERS).clamp(min=0)
        w2 = torch.tensor([int(round(2 * w)) for w in cls.ORDER_WEIGHTS], dtype=torch.int64, device=ev.device)
        return longest_first_within_chunks((ev.to(torch.int64) * w2).sum(1))

    def info(self):
        """Launch geometry: rows per lane, workgroups, waves per workgroup, batched start values,
        specialised kernel, LDS bytes per workgroup, fantasy capacity of the kernel unit (FMAX), base
        surrogates S (1: a plain plan), restart table (1: step 0 of a trajectory runs once per restart,
        0: in every trajectory -- MRBO_RESTART_TABLES=0, the half-wave kernel, N > 64), fused Newton
        iteration (1: an accepted line-search trial goes on to its gradient and Hessian in the same
        evaluation call, 0: the two-call loop -- MRBO_NEWTON_FUSED=0, the half-wave kernel, N > 64)."""
        v = (ctypes.c_int32 * 10)()
        _lib.check(self.lib.mrbo_plan_info(self.handle, v, 10))
        keys = ("rpl", "blocks", "waves_per_group", "batch", "spec", "lds_bytes", "fmax", "S", "restart_tables",
                "newton_fused")
        return dict(zip(keys, (int(x) for x in v)))


XCD_QUEUES = 8   # work-queue heads of the rollout kernel (MRBO_QUEUE_INTS / 16)
ORDER_WBITS = 29  # work-key bits of mrbo_plan_order_longest_first (csrc/mrbo_order.hip) below the chunk


def xcd_chunks(T, device=None):
    """Per-XCD queue chunk of every queue position 0..T-1: chunk x = [x·T/8, (x+1)·T/8) (integer
    division, as rollout_kernel computes them).  Pure index arithmetic (CPU-testable)."""
    import torch
    p = torch.arange(T, dtype=torch.int64, device=device)
    lo = torch.tensor([x * T // XCD_QUEUES for x in range(1, XCD_QUEUES)], dtype=torch.int64, device=device)
    return torch.bucketize(p, lo, right=True)


def longest_first_within_chunks(work, device=None):
    """The order of mrbo_plan_order_longest_first from integer work keys (2 × the weighted counters):
    every chunk's own trajectories, longest first, stable in index order on ties -- queue position r
    takes trajectory order[r] and stays in the chunk it had in index order."""
    import torch
    work = torch.as_tensor(work, dtype=torch.int64, device=device).clamp(0, (1 << ORDER_WBITS) - 1)
    chunk = xcd_chunks(work.numel(), work.device)
    key = ((XCD_QUEUES - 1 - chunk) << ORDER_WBITS) | work
    return torch.sort(key, descending=True, stable=True).indices.to(torch.int32)


def rnstream(M, d, H):
    """gen_low_discrepancy_sequence (utils.jl:65-74) via the library's host Sobol."""
    lib = _lib.load()
    out = np.zeros((M, d + 1, H), order="F")
    _lib.check(lib.mrbo_rnstream(int(M), int(d), int(H), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    return out


def initial_guesses(n, lbs, ubs):
    lib = _lib.load()
    lbs, ubs = _f64(lbs).ravel(), _f64(ubs).ravel()
    d = lbs.size
    out = np.zeros((d, n + 2), order="F")
    dp = ctypes.POINTER(ctypes.c_double)
    _lib.check(lib.mrbo_initial_guesses(int(n), d, lbs.ctypes.data_as(dp), ubs.ctypes.data_as(dp),
                                        out.ctypes.data_as(dp)))
    return out


def dual_uniform(seed, traj, j, k):
    return _lib.load().mrbo_dual_uniform(int(seed), int(traj), int(j), int(k))
