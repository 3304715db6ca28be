"""Inputs that reach each per-trajectory status bit of the rollout (include/mrbo.h MRBO_ST_*) far
above rounding, for tests/test_failure_paths.py (the oracle alone) and
tests/test_gpu_failure_paths.py (the GPU against the oracle).

Every input is a legitimate API input -- a base surrogate, a box, starts, a Sobol stream, solver
options -- and every failure is one of the numerical failures the API documents (the reference's
Julia exceptions); nothing here provokes a device fault.

A problem is a dict with the keys of tests/parity.py `_problem_arrays` (X, L, c, y, fmini, lbs,
ubs, x0s, rnstream, xstarts, h, ell, period) plus `kernel` (the oracle's name).  `plain_problem`
builds one without libmrbo.so: the design and the fit come from the package's CPU surrogate, the
Sobol stream and the inner starts from the oracle.  A recipe takes a plain problem and returns
(problem, opts): the altered problem and the options both sides take (sigma_n2, htol, sigma_tol).

  recipe        change to the plain input                                    bit   launch
  factor        L scaled by s < 1: σ² = ψ(0) − ‖L⁻¹k‖² turns negative where   1     mixed
                ‖L0⁻¹k‖² > s²·ψ(0), near the data and the fantasy points
  noise         sigma_n2 < 0, random x0: σ² is negative close to an earlier   1     mixed
                fantasy point, so the failures are at steps ≥ 1
  noise_near    sigma_n2 < 0, x0 = a data point + 0.01 ℓ: the Schur            4     all
                complement of update_cholesky! at step 0 is negative
  nan_starts    one coordinate of every inner start NaN: every Newton         8     all
                candidate is NaN
  singular      sigma_tol = 10 (the rule's σ < σtol branch returns exact      16    mixed
                zeros, Hα ≡ 0) with htol = 0, so det(Hα) = 0 passes the
                det test and the LU meets a zero pivot

The scale s and the noise are per case (CASES): what puts a shape's launch between "nothing fails"
and "everything fails" depends on how dense its K is.  They were tuned on the oracle alone
(tests/test_failure_paths.py holds the conditions and records the counts).
"""
import numpy as np

KERNEL_IDS = {"matern52": 0, "matern32": 1, "matern12": 2, "se": 3, "periodic": 4}
RULE_IDS = {"EI": 0, "POI": 1, "LCB": 2}

# recipe -> (the bit, whether finished and failed trajectories must share the launch and a restart)
EXPECT = {"factor": (1, True), "noise": (1, True), "noise_near": (4, False), "nan_starts": (8, False),
          "singular": (16, True)}
RECIPES = tuple(EXPECT)

M, R, NSTARTS = 32, 4, 16
GHQ_NODES = 5


def design_ell(d, N, width=65.536):
    """the lengthscale at the design spacing of N points in a box of this width (tests/test_gpu.py
    test_dimensions_and_sizes_replay_vs_oracle)"""
    return 0.6 * width * N ** (-1.0 / d)


def plain_problem(oracle, d, N, h, kernel="matern52", golden=None, M=M, R=R):
    """Centred Ackley(d) (y − mean y: the zero-mean GP then has structure to resolve, so the
    policy points differ from sample to sample) on a Kronecker design of N points at the
    design-spacing lengthscale -- or, with `golden` (the arrays of tests/golden/golden_c2.npz), that
    file's Branin data, box and inner starts at ℓ = 1 -- with M Sobol samples, R restarts uniform
    in the box (default_rng(0)) and 16 + 2 inner starts."""
    from mrbo import testfns
    from mrbo.kernels import Matern52, SquaredExponential
    from mrbo.surrogates import Surrogate
    from mrbo.utils import kronecker_quasirand
    psi = {"matern52": Matern52, "se": SquaredExponential}[kernel]
    if golden is not None:
        assert golden["X"].shape == (d, N)
        X, y, ell = np.array(golden["X"]), np.array(golden["y"]), 1.0
        lbs, ubs, xstarts = np.array(golden["lbs"]), np.array(golden["ubs"]), np.array(golden["xstarts"], order="F")
    else:
        tf = testfns.TestAckley(d)
        lbs, ubs = tf.get_bounds()
        X = lbs[:, None] + (ubs - lbs)[:, None] * kronecker_quasirand(d, N)
        y = tf(X)
        y = y - y.mean()
        ell = design_ell(d, N)
        xstarts = oracle.generate_initial_guesses(NSTARTS, lbs, ubs)
    s = Surrogate(psi([ell]), X, y, capacity=N, σn2=1e-6)
    g = dict(X=s.X[:, :N].copy(), L=s.L[:N, :N].copy(), c=s.c[:N].copy(), y=s.y[:N].copy(), fmini=s.fmini(),
             lbs=lbs, ubs=ubs, ell=ell, xstarts=xstarts)
    if golden is not None and kernel == "matern52":   # the file's own factor and coefficients
        g.update(L=np.array(golden["L"]), c=np.array(golden["c"]), fmini=float(golden["fmini"]))
    rng = np.random.default_rng(0)
    g["x0s"] = np.asfortranarray(lbs[:, None] + (ubs - lbs)[:, None] * rng.random((d, R)))
    g["rnstream"] = oracle.gen_low_discrepancy_sequence(M, d, h + 1)
    g.update(h=h, period=1.0, kernel=kernel)
    return g


def factor(g, scale=0.9):
    """L scaled, and c with it so that c stays L'\\(L\\y) as mrbo.h defines it (the two sides may use
    either form, and only agree on a surrogate whose L and c belong together): the factor of
    scale²·K, inconsistent with the kernel function alone"""
    q = dict(g)
    q["L"] = g["L"] * scale
    q["c"] = g["c"] / scale ** 2
    return q, {}


def noise(g, sigma_n2=-0.02):
    return dict(g), dict(sigma_n2=sigma_n2)


def noise_near(g, sigma_n2=-0.02, offset=0.01):
    q = dict(g)
    nr = g["x0s"].shape[1]
    q["x0s"] = np.asfortranarray(g["X"][:, :nr] + offset * float(g["ell"]))
    return q, dict(sigma_n2=sigma_n2)


def nan_starts(g, every=1):
    """every = 2: NaN in every other start only -- the NaN filter, nothing fails"""
    q = dict(g)
    xs = np.array(g["xstarts"], order="F")
    xs[0, ::every] = np.nan
    q["xstarts"] = xs
    return q, {}


def singular(g, htol=0.0):
    return dict(g), dict(sigma_tol=10.0, htol=htol)


class Case:
    """One kernel layout: the shape and environment that select it, what
    plan.info() must report, the per-shape recipe constants and the recipes it cannot hold."""

    def __init__(self, id, d, N, h, info, scale, noise, golden=False, kernel="matern52", rule="EI", cost=False,
                 ghq=False, env=None, noise_bit=1, bits=None, drop=None):
        self.id, self.d, self.N, self.h, self.info = id, d, N, h, info
        self.scale, self.noise, self.noise_bit = scale, noise, noise_bit
        self.golden, self.kernel, self.rule, self.cost, self.ghq = golden, kernel, rule, cost, ghq
        self.env = env or {}
        self.bits = bits or {}          # recipe -> the status values its launch may hold beside 0 and its bit
        self.drop = drop or {}          # recipe -> why this layout cannot hold it

    def recipes(self):
        return [r for r in RECIPES if r not in self.drop]

    def problem(self, oracle, golden_c2):
        g = plain_problem(oracle, self.d, self.N, self.h, kernel=self.kernel,
                          golden=golden_c2 if self.golden else None)
        if self.ghq:
            from mrbo.rollout import ghq_node_arrays
            from mrbo.utils import gauss_hermite, generate_indices
            t, w = gauss_hermite(GHQ_NODES)
            nodes, weights = ghq_node_arrays(t, w, generate_indices(GHQ_NODES, self.h + 1))
            g["ghq"] = (np.asfortranarray(nodes), np.asfortranarray(weights))
        return g

    def cost_model(self):
        return ("quadratic", 1.0, np.linspace(0.5, 1.5, self.d)) if self.cost else None

    def apply(self, recipe, g):
        if recipe == "factor":
            return factor(g, self.scale)
        if recipe == "noise":
            return noise(g, self.noise)
        if recipe == "noise_near":
            return noise_near(g, min(self.noise, -0.02))
        return {"nan_starts": nan_starts, "singular": singular}[recipe](g)

    def expect(self, recipe):
        """(the bit, mixed, the status values the launch may hold)"""
        bit, mixed = EXPECT[recipe]
        if recipe == "noise":
            bit = self.noise_bit
        return bit, mixed, {0, bit} | set(self.bits.get(recipe, ()))

    def oracle_kw(self, g):
        kw = dict(rule=self.rule, cost=self.cost_model())
        if self.ghq:
            kw["ghq"] = g["ghq"]
        return kw


_HALF = dict(spec=2, rpl=1, fmax=4, restart_tables=0)
_FULL = dict(spec=1, rpl=1, fmax=4, restart_tables=1)
_GEN = dict(spec=0, rpl=1, fmax=4, restart_tables=1)
_FEW_ADJ = ("fewer than 10 % of the trajectories reach the adjoint's solve (the best observation at a fantasy "
            "step and an improvement), so bit 16 stays below the 10 % condition")
_NOISE_D2 = ("between sigma_n2 = −0.001 and −0.1 fewer than 10 % of the trajectories {}, and beyond −0.1 the "
             "oracle's two builds begin to disagree on some statuses")

# The kernel layouts.  h = 3 twins (a failure at the last step) for every layout but the
# half-wave kernel, the cost kernel and the Gauss–Hermite estimator.
CASES = [
    Case("half_d2_n12", 2, 12, 2, _HALF, 0.9, -0.02, golden=True),
    Case("half_d3_n24", 3, 24, 2, _HALF, 0.99, -0.05),
    Case("half_off_d2_n12", 2, 12, 2, _FULL, 0.9, -0.02, golden=True, env={"MRBO_HALF": "0"}),
    Case("half_off_d3_n24", 3, 24, 2, _FULL, 0.99, -0.05, env={"MRBO_HALF": "0"}),
    Case("full_d6_n40_h2", 6, 40, 2, _FULL, 0.9, -0.1, bits={"factor": (2,)}),
    Case("full_d6_n40_h3", 6, 40, 3, _FULL, 0.9, -0.1, bits={"factor": (2,)}),
    Case("full_tables_off_d6_n40_h2", 6, 40, 2, dict(_FULL, restart_tables=0), 0.9, -0.1, bits={"factor": (2,)},
         env={"MRBO_RESTART_TABLES": "0"}),
    Case("full_tables_off_d6_n40_h3", 6, 40, 3, dict(_FULL, restart_tables=0), 0.9, -0.1, bits={"factor": (2,)},
         env={"MRBO_RESTART_TABLES": "0"}),
    Case("two_rows_d4_n96_h2", 4, 96, 2, dict(spec=1, rpl=2, fmax=4, restart_tables=0), 0.965, -0.05,
         drop={"factor": "bit 1 reaches 12 of 128 trajectories at scale 0.965 and every trajectory fails at step 0 "
                         "from 0.964 down: no scale leaves 10 % of both kinds at h = 2 (the h = 3 twin holds it)"}),
    Case("two_rows_d4_n96_h3", 4, 96, 3, dict(spec=1, rpl=2, fmax=4, restart_tables=0), 0.97, -0.05,
         bits={"noise": (2,)}),
    # negative noise shows here as bit 2 (the draw's covariance at the policy point), on 66 % of the
    # trajectories, and as bit 1 on 5 %: the recipe's bit at this shape is 2
    Case("four_rows_d3_n150_h2", 3, 150, 2, dict(spec=1, rpl=4, fmax=4, restart_tables=0), 0.995, -0.02, noise_bit=2,
         bits={"factor": (2,), "noise": (1,)}, drop={"singular": _FEW_ADJ}),
    Case("four_rows_d3_n150_h3", 3, 150, 3, dict(spec=1, rpl=4, fmax=4, restart_tables=0), 0.995, -0.02, noise_bit=2,
         bits={"factor": (2,), "noise": (1,)}, drop={"singular": _FEW_ADJ}),
    Case("wide_d9_n20_h2", 9, 20, 2, dict(spec=0, rpl=1, fmax=6, restart_tables=1), 0.8, -0.1, bits={"noise": (2,)}),
    Case("wide_d9_n20_h3", 9, 20, 3, dict(spec=0, rpl=1, fmax=6, restart_tables=1), 0.8, -0.1, bits={"noise": (2,)}),
    Case("generic_d2_n12_h2", 2, 12, 2, _GEN, 0.9, -0.02, golden=True, env={"MRBO_GENERIC_KERNEL": "1"}),
    Case("generic_d2_n12_h3", 2, 12, 3, _GEN, 0.9, -0.02, golden=True, env={"MRBO_GENERIC_KERNEL": "1"}),
    Case("se_d2_n12_h2", 2, 12, 2, _GEN, 0.9, -0.05, golden=True, kernel="se", bits={"factor": (2,)}),
    Case("se_d2_n12_h3", 2, 12, 3, _GEN, 0.9, -0.05, golden=True, kernel="se", bits={"factor": (2,)}),
    Case("poi_d2_n12_h2", 2, 12, 2, _GEN, 0.9, -0.02, golden=True, rule="POI", bits={"noise": (2,)}),
    Case("poi_d2_n12_h3", 2, 12, 3, _GEN, 0.9, -0.02, golden=True, rule="POI",
         drop={"noise": _NOISE_D2.format("finish")}),
    # the quadratic cost at d = 2, N = 12 runs the generic kernel (the compile-time cost kernel
    # exists at N = 65..256 in the FMAX = 6 units only); the cost kernel proper follows
    Case("cost_generic_d2_n12", 2, 12, 2, _GEN, 0.9, -0.02, golden=True, cost=True,
         drop={"noise": _NOISE_D2.format("fail")}),
    Case("cost_kernel_d3_n70_h4", 3, 70, 4, dict(spec=3, rpl=2, fmax=6, restart_tables=0), 0.99, -0.05, cost=True,
         bits={"factor": (2,), "noise": (2,)}, drop={"singular": _FEW_ADJ}),
    # no draw, so no bit 2; M = 5³ node vectors
    Case("ghq_d2_n12", 2, 12, 2, _HALF, 0.9, -0.02, golden=True, ghq=True),
]
CASE_BY_ID = {c.id: c for c in CASES}
PAIRS = [(c.id, r) for c in CASES for r in c.recipes()]
DROPPED = [(c.id, r, why) for c in CASES for r, why in c.drop.items()]
# the h = 3 twins must fail at the last step somewhere: these recipes can (bit 1 or 2 at any step)
LAST_STEP = [(c.id, r) for c in CASES for r in ("factor", "noise") if c.h == 3 and r not in c.drop]


def oracle_surrogate(oracle, g, opts):
    return oracle.OracleSurrogate(g["X"], g["L"], g["c"], g["y"], kernel=g.get("kernel", "matern52"),
                                  ell=float(g["ell"]), sigma_n2=opts.get("sigma_n2", 1e-6), fmini=float(g["fmini"]),
                                  period=float(g.get("period", 1.0)))


def oracle_run(oracle, g, opts, replay_x=None, h=None, rule="EI", cost=None, ghq=None, want_kappa=False, x0s=None,
               nthreads=8):
    """the oracle on (problem, opts); h below the problem's: the first h + 1 slabs of its stream (or
    node columns).  Its policy buffer starts as NaN (written_columns)."""
    h = int(g["h"]) if h is None else h
    kw = {k: opts[k] for k in ("htol", "sigma_tol") if k in opts}
    rn = None
    if ghq is None:
        rn = np.asfortranarray(g["rnstream"][:, :, :h + 1])
    else:
        kw["ghq"] = (np.asfortranarray(ghq[0][:, :h + 1]), np.asfortranarray(ghq[1][:, :h + 1]))
    return oracle.simulate_mc(oracle_surrogate(oracle, g, opts), g["x0s"] if x0s is None else x0s, rn, g["xstarts"],
                              g["lbs"], g["ubs"], h, replay_x=replay_x, rule=rule, cost=cost, want_kappa=want_kappa,
                              nthreads=nthreads, policy_fill=np.nan, want_policy=replay_x is None, **kw)


def written_columns(policy_x):
    """per trajectory (M×R), the number of leading policy columns x_0.. written into a buffer that
    was filled with NaN before the run: a failed trajectory leaves the columns after its last step
    as they were"""
    wr = ~np.isnan(policy_x).all(axis=0)
    hp1 = wr.shape[0]
    w = np.where(wr.all(axis=0), hp1, np.argmin(wr, axis=0))
    assert (wr == (np.arange(hp1)[:, None, None] < w[None])).all(), "written policy columns are not a prefix"
    return w


def conditions(status, bit, mixed):
    """the non-vacuity conditions of a recipe on one status array (M×R): the bit on ≥ 10 % of the
    trajectories and, for a mixed recipe, ≥ 10 % finished and a restart that holds both kinds.
    Returns (ok, counts)."""
    st = np.asarray(status)
    counts = {int(v): int((st == v).sum()) for v in np.unique(st)}
    has = (st & bit) != 0
    ok = has.mean() >= 0.10
    if mixed:
        fin = st == 0
        both = (fin.any(axis=0) & has.any(axis=0)).any()
        ok = ok and fin.mean() >= 0.10 and bool(both)
    return bool(ok), counts
