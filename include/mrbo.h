/*
 * mrbo.h -- C ABI of the MI355X rollout-acquisition evaluator (libmrbo.so).
 *
 * Drop-in boundary for the reference's Monte-Carlo rollout path.  The reference is pure
 * Julia and has no FFI; each entry point below replaces one Julia function (file:line in
 * /root/reference) and is what a `ccall` shim binds (INTEGRATION.md shows the shim):
 *
 *   mrbo_simulate_mc       simulate_trajectory_mc(T, tp; inner_solve_xstarts, resolutions,
 *                          spatial_gradients_container, hyperparameter_gradients_container)
 *                          rollout.jl:279-340 -- batched over R restarts (the x0 batch of the
 *                          outer ascent, utils.jl:97-106 / stochastic_solve utils.jl:235-265)
 *   mrbo_eto_reduce        the mean / std(n-1) tail of simulate_trajectory_mc, rollout.jl:328-339
 *   mrbo_stochastic_solve  stochastic_solve utils.jl:235-265 (eswavs + StandardSGA / Adam update!)
 *                          over a restart batch, the whole ascent in one call
 *   mrbo_rollout_solve     the build's acquisition solve of a BO step (the reference's rollout solver
 *                          is undefined): the ascent, the final evaluation and the pick in one call
 *   mrbo_simulate_control, mrbo_eto_reduce_cv   the build's EI control variate (the reference's
 *                          --variance-reduction names an undefined solver): variance-reduced ETO rows
 *   mrbo_eval_base         eval(s::Surrogate, x, θ) radial_basis_surrogates.jl:224-310 (μ, σ, ∇, Hα)
 *   mrbo_rnstream          gen_low_discrepancy_sequence utils.jl:65-74 (Sobol→Box–Muller(log10))
 *   mrbo_initial_guesses   generate_initial_guesses utils.jl:145-153
 *   mrbo_gp_fit            Surrogate(ψ, X, y) radial_basis_surrogates.jl:77-118 and its
 *                          log_likelihood / ∇log_likelihood (:770-799) for a batch of
 *                          lengthscales -- the evaluations behind optimize! (:805-829)
 *
 * Conventions
 *   - Plain pointers and sizes; matrices are column-major with the reference's (Julia) shapes.
 *   - Arrays passed to mrbo_simulate_mc / mrbo_eto_reduce / mrbo_eval_base are DEVICE pointers
 *     (hipMalloc'd or from a framework allocator) unless MRBO_FLAG_HOST_POINTERS is set, in
 *     which case the library stages them through device memory (PCIe-inclusive).
 *   - The plan owns the device copy of the base surrogate and all workspace; a call never
 *     allocates (graph-capturable) and is re-entrant per (plan, stream) pair.
 *   - Return value: 0 on success, negative mrbo_err_t on argument/launch errors (message via
 *     mrbo_last_error()).  Per-trajectory numerical failures -- the reference's Julia
 *     exceptions -- are reported in status[] (MRBO_ST_*), never as a return code.
 */
#ifndef MRBO_H
#define MRBO_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MRBO_ABI_VERSION 2

typedef enum {
  MRBO_OK = 0,
  MRBO_ERR_ARG = -1,      /* invalid argument (dimension, size, null pointer)            */
  MRBO_ERR_UNSUPPORTED = -2, /* shape outside the compiled kernels: d > 16, N > 512,
                                d > 8 with N > 128, h > 5 (gp_fit: N > 512) */
  MRBO_ERR_HIP = -3,      /* HIP runtime error                                          */
  MRBO_ERR_NOMEM = -4
} mrbo_err_t;

typedef enum {
  MRBO_KERNEL_MATERN52 = 0, /* radial_basis_functions.jl:60-68  */
  MRBO_KERNEL_MATERN32 = 1, /* :70-78 */
  MRBO_KERNEL_MATERN12 = 2, /* :80-88 */
  MRBO_KERNEL_SE = 3,       /* :90-96 */
  MRBO_KERNEL_PERIODIC = 4  /* :98-103  exp(−2 sin²(πρ/p)/ℓ²), p = mrbo_surrogate_t.period */
} mrbo_kernel_t;

typedef enum {
  MRBO_RULE_EI = 0,   /* decision_rules.jl:84-99   expected improvement                 */
  MRBO_RULE_POI = 1,  /* decision_rules.jl:101-115 probability of improvement           */
  MRBO_RULE_LCB = 2   /* decision_rules.jl:117-127 θσ − μ (negated lower confidence bound) */
} mrbo_rule_t;

/* NonUniformCost (cost_functions.jl:5-20: NonUniformCost(f) with ∇f, Hf) as closed-form families.
 * The reference's cost is an arbitrary closure referenced by no rule, surrogate or trajectory;
 * the build defines the cost-weighted acquisition f(x) = α(x)/c(x) of the inner policy solve
 * (α, ∇f, Hf, ∂∇f/∂θ and the adjoint perturbations all weighted; parity unpinned, the oracle
 * implements the same definition).  u_a = (x_a − lb_a)/(ub_a − lb_a) over the plan's box:
 *   MRBO_COST_QUADRATIC  c(x) = c0 + Σ_a w_a u_a²        MRBO_COST_LOGLINEAR  c(x) = c0·exp(Σ_a w_a u_a)
 * mrbo_plan_create refuses (MRBO_ERR_ARG) any model that is not positive on the box: c0 ≤ 0 or
 * non-finite, a non-finite weight, a negative QUADRATIC weight, or ub ≤ lb in some dimension. */
typedef enum { MRBO_COST_NONE = 0, MRBO_COST_QUADRATIC = 1, MRBO_COST_LOGLINEAR = 2 } mrbo_cost_t;

/* per-trajectory status bits: the reference's exceptions (SURVEY.md §8b "Errors") */
enum {
  MRBO_ST_OK = 0,
  MRBO_ST_SIGMA_NEG = 1,   /* DomainError sqrt(negative variance)   r_b_s.jl:528 */
  MRBO_ST_DRAW_NOT_PD = 2, /* PosDefException, gp_draw covariance    r_b_s.jl:537 */
  MRBO_ST_COND_NOT_PD = 4, /* PosDefException, update_cholesky!      r_b_s.jl:412 */
  MRBO_ST_ALL_NAN = 8,     /* findmin on an empty candidate list     rbf_optim.jl:96 */
  MRBO_ST_SINGULAR = 16    /* singular Hessian in solve_dual_x       rollout.jl:188 */
};

enum {
  MRBO_FLAG_HOST_POINTERS = 1, /* arrays are host memory; stage through the device  */
  MRBO_FLAG_NO_GRADIENT = 2    /* skip gradient(T): containers == nothing branch    */
};

/* Base GP surrogate (Surrogate struct, radial_basis_surrogates.jl:30-41), HOST memory. */
typedef struct {
  int32_t d;            /* input dimension                                        */
  int32_t N;            /* observed points (get_observed)                         */
  int32_t kernel;       /* mrbo_kernel_t                                          */
  double lengthscale;   /* ψ.θ[1]                                                 */
  double sigma_n2;      /* σn2                                                    */
  double fmini;         /* minimum(s.y) over the whole capacity buffer (Q3)       */
  const double* X;      /* d×N, column-major, leading dim d                       */
  const double* L;      /* N×N lower Cholesky factor of K, column-major, ld = ldL */
  int32_t ldL;
  const double* c;      /* N coefficients L'\(L\y)                                */
  const double* y;      /* N observations                                        */
  double period;        /* ψ.θ[2] of the Periodic kernel (unused otherwise)      */
} mrbo_surrogate_t;

/* TrajectoryParameters (trajectory.jl:43-94) + inner-solve options (rbf_optim.jl:24-30). */
typedef struct {
  int32_t h;            /* horizon (≤ 5)                                         */
  int32_t M;            /* MC samples per restart (tp.mc_iters)                  */
  int32_t R;            /* restarts (x0 batch)                                   */
  int32_t nstarts;      /* inner starts = columns of inner_solve_xstarts         */
  int32_t rule;         /* mrbo_rule_t                                           */
  double theta;         /* T.θ[1]: decision-rule hyperparameter (Q12: T.θ, not tp.θ) */
  const double* lbs;    /* d, HOST */
  const double* ubs;    /* d, HOST */
  int32_t max_iters;    /* inner Newton iterations per start      */
  int32_t max_ls;       /* backtracking steps                                    */
  double x_tol;         /* Optim x_tol (rbf_optim.jl:27) = 1e-3                  */
  double f_tol;         /* Optim f_tol = 1e-3                                    */
  double g_tol;         /* Optim default g_tol = 1e-8                            */
  double htol;          /* solve_dual_x det threshold (rollout.jl:156) = 1e-4    */
  double sigma_tol;     /* EI / POI σtol (decision_rules.jl:84, :102) = 1e-8     */
  uint64_t seed;        /* δx for solve_dual_y (rollout.jl:133) when dual_y_dx == NULL */
  int32_t sample_offset;/* global index of this plan's first MC sample (multi-GPU shard), 0 */
  int32_t samples_total;/* DEPRECATED, ignored (kept for the struct layout).  The δx counter */
                        /* RNG is keyed by the global sample index sample_offset + m alone */
                        /* (round 5), so all R restarts of a launch share the δx of sample */
                        /* m, and restart r equals an R = 1 launch at its x0.  The         */
                        /* reference draws a fresh rand(dim) per solve_dual_y call         */
                        /* (rollout.jl:133): restarts are NOT decorrelated. */
  int32_t cost;         /* mrbo_cost_t: NonUniformCost weighting of the inner-solve rule      */
  double cost_c0;       /* cost family parameter c0                                          */
  const double* cost_w; /* d weights, HOST (NULL with MRBO_COST_NONE)                        */
} mrbo_params_t;

typedef struct mrbo_plan mrbo_plan_t;

const char* mrbo_version(void);
const char* mrbo_last_error(void);
int mrbo_device_count(void);

/* Build the device state for (surrogate, params): copies X, L⁻¹ (packed), c; sizes the
 * persistent-wave grid and workspace.  `device` is a HIP ordinal.                         */
int mrbo_plan_create(const mrbo_surrogate_t* s, const mrbo_params_t* p, int32_t device, mrbo_plan_t** out);
int mrbo_plan_destroy(mrbo_plan_t* plan);

/* Surrogate batch: ONE plan, and one kernel launch per call, for S independent base surrogates
 * s[0..S-1] (no reference counterpart: the reference runs the trials of an experiment, or the
 * lengthscale hypotheses on one data set, one after another).  The surrogates share d, N, kernel
 * and sigma_n2 -- a mismatch, S < 1 or an entry without X / L / c / y is MRBO_ERR_ARG, checked
 * before any HIP call -- and differ in X, L, c, y, lengthscale, period and fmini; the plan holds,
 * per surrogate, everything mrbo_plan_create derives from them.  p is shared: the box (one box per
 * surrogate: mrbo_plan_create_batch_boxes below), rule, θ,
 * solver options, cost model, and p->R = the restarts PER SURROGATE; so are the rnstream / nodes
 * and the xstarts of the calls.  Every workgroup of a launch serves one surrogate (grid
 * (⌈workgroups/S⌉, S), one set of per-XCD work queues per surrogate) and runs the code of a plain
 * plan on it: surrogate q's block of every output is bit-identical to what mrbo_plan_create(&s[q],
 * p) computes from the same inputs (tests/test_gpu_surrogate_batch.py).
 *   Layout: the surrogate index is the slowest one everywhere -- x0s d×R×S; values, status,
 *   grad_theta M×R×S; grad_x d×M×R×S; policy_x d×(h+1)×M×R×S; obs (h+1)×M×R×S; evals
 *   MRBO_NCOUNTERS×M×R×S; dual_y_dx, replay_x d×h×M×R×S.
 *   mrbo_simulate_mc / mrbo_simulate_ghq: one rollout launch for all S surrogates, one entry of
 *   the timing ring (mrbo_kernel_times) per call.
 *   mrbo_eto_reduce, mrbo_partial_moments, mrbo_merge_moments, mrbo_sga_step, mrbo_adam_step,
 *   mrbo_stochastic_solve: the plan simply has R·S restarts -- ETO rows in (surrogate, restart)
 *   order, active int32[R·S], x0s / m / v d×(R·S).
 *   mrbo_base_solve: the n starts on each of the S base surrogates -- xmin d×n×S, fmin and status
 *   n×S, evals MRBO_NCOUNTERS×n×S.   mrbo_eval_base: the P points on each surrogate -- out
 *   (3+4d+d²)×P×S.
 *   Work orders are per plain plan: on S > 1 mrbo_plan_set_order and
 *   mrbo_plan_order_longest_first return MRBO_ERR_UNSUPPORTED, and mrbo_stochastic_solve keeps
 *   the index order instead of its automatic longest-first one.
 * mrbo_plan_create(s, p, ...) is mrbo_plan_create_batch(s, 1, p, ...).                          */
int mrbo_plan_create_batch(const mrbo_surrogate_t* s, int32_t S, const mrbo_params_t* p, int32_t device,
                           mrbo_plan_t** out);

/* Boxed plan: a surrogate batch whose surrogates each have their OWN box (the ARD trials of a BO
 * loop, each on its whitened box).  lbs / ubs are HOST arrays d×S, the surrogate index slowest;
 * p->lbs / p->ubs are ignored and may be NULL.  Every check of mrbo_plan_create_batch applies;
 * further MRBO_ERR_ARG, before any HIP call: null lbs or ubs, a non-finite bound or lb > ub in
 * any (dimension, surrogate) -- the message names the surrogate -- and a cost model on a box with
 * ub <= lb in some dimension (the weights cost_w stay shared; u is normalised over the
 * surrogate's own box).
 *   On a boxed plan every call that takes xstarts reads S blocks, the surrogate index slowest:
 *   mrbo_simulate_mc, mrbo_simulate_ghq, mrbo_simulate_control, mrbo_stochastic_solve and
 *   mrbo_rollout_solve d×nstarts×S, mrbo_base_solve d×n×S (host-pointer staging follows).  There
 *   is no flag: the plan decides, and a caller with equal starts replicates them.
 *   mrbo_box_adam_step, the projection inside mrbo_rollout_solve and mrbo_pick_restart use the box
 *   of the restart's surrogate (restart r of the R·S belongs to surrogate r / R).
 * Block q of every output of every call is bit-identical to the same call on
 * mrbo_plan_create(&s[q], p with box q) with starts q; S equal boxes and start blocks give the
 * bits of mrbo_plan_create_batch; S = 1 is the plain plan on box 0 (xstarts then d×nstarts).
 * Work orders stay MRBO_ERR_UNSUPPORTED at S > 1 (tests/test_gpu_batch_boxes.py).               */
int mrbo_plan_create_batch_boxes(const mrbo_surrogate_t* s, int32_t S, const mrbo_params_t* p, const double* lbs,
                                 const double* ubs, int32_t device, mrbo_plan_t** out);

/* simulate_trajectory_mc for the R×M trajectories of the plan.
 *   x0s        d×R          start of each restart (tp.x0 / set_start!, rollout.jl:287)
 *   rnstream   M×(d+1)×(h+1) tp.rnstream_sequence (trajectory.jl:52-68), shared by restarts
 *   xstarts    d×nstarts    inner_solve_xstarts (a boxed plan: d×nstarts×S, block q surrogate q's)
 *   dual_y_dx  d×h×M×R or NULL: δx of solve_dual_y call j (column j-1); NULL → counter RNG(seed)
 *   replay_x   d×h×M×R or NULL: inject policy points x_1..x_h instead of the inner solve
 *   values     M×R          resolutions
 *   grad_x     d×M×R        spatial_gradients_container          (may be NULL with NO_GRADIENT)
 *   grad_theta 1×M×R        hyperparameter_gradients_container   (may be NULL with NO_GRADIENT)
 *   status     M×R          MRBO_ST_* bits
 *   policy_x   d×(h+1)×M×R or NULL: x_0..x_h of every trajectory (fs.X[:, N+1:N+h+1])
 *   obs        (h+1)×M×R or NULL:   sampled observations y_0..y_h
 *   evals      MRBO_NCOUNTERS×M×R or NULL: per trajectory [gradient evals, value-only evals,
 *              Hessian completions, adjoint rich evals, adjoint perturbation pairs] -- the work
 *              counters of the FLOP roofline model (inner-solve counts are identical to the
 *              oracle's: same lazy Newton iteration)
 * Failed trajectories (status != 0; tests/test_gpu_failure_paths.py).  The step loop ends at the
 * first failure -- σ² < 0 at a Newton iterate of the inner solve (bit 1; the solve itself runs to
 * its end, and its work past that iterate is not the reference's, which has thrown) or at an
 * observation point (bit 1: the kernel tests σ² ahead of the draw with either observable.  The
 * reference's Monte-Carlo observable draws with gradient and never takes σ, so it -- and the oracle
 * -- fail there in the draw's factor, whose first pivot σ² is: PosDefException, bit 2.  Same step,
 * same outputs, another bit), a draw whose covariance is not positive definite with σ² ≥ 0 (bit 2),
 * update_cholesky! (bit 4), a multistart whose candidates are all NaN (bit 8) -- and the adjoint
 * does not run: values, grad_x, grad_theta and every obs entry
 * are NaN, counters 3 and 4 are 0, counters 0..2 hold the Newton work done so far, and policy_x
 * holds x_0..x_k, k the last step whose policy point was found (a failure inside the inner solve of
 * step k + 1, or at step k itself); the columns after x_k are NOT written and keep the caller's
 * bytes.  Bit 16 is raised by the adjoint itself, after the step loop and the observations:
 * values, grad_x and grad_theta are NaN, obs and policy_x are complete, and counters 3 and 4 hold
 * the adjoint work done (≥ 1 rich evaluation).  No failure touches another trajectory's outputs.
 * Launches on `stream` (hipStream_t, may be NULL) and returns without synchronising.       */
int mrbo_simulate_mc(mrbo_plan_t* plan, const double* x0s, const double* rnstream, const double* xstarts,
                     const double* dual_y_dx, const double* replay_x, double* values, double* grad_x,
                     double* grad_theta, int32_t* status, double* policy_x, double* obs, int64_t* evals,
                     uint32_t flags, void* stream);

#define MRBO_NCOUNTERS 5

/* simulate_trajectory_ghq(T, tp; inner_solve_xstarts, resolutions, nodes, weights, indices, …)
 * rollout.jl:409-467 — the Gauss–Hermite estimator.  Sample m (of M = length(indices)) uses the
 * node vector nodes[m, 0..h] = nodes[indices[m]] and weights[m, 0..h] = weights[indices[m]]
 * (M×(h+1), column-major; generate_indices utils.jl:217-221 builds the tensor product): step k
 * observes y = μ + √2·σ·t_k with recorded gradient weights[k]·(∇μ + √2·∇σ·t_k)
 * (GaussHermiteObservable observables.jl:32-81, get_gradient :157) and the resolution is
 * weights[best]·max(fmini − y_best, 0)/√π.  All other arguments and outputs as mrbo_simulate_mc
 * (the plan's M is the number of node vectors).                                              */
int mrbo_simulate_ghq(mrbo_plan_t* plan, const double* x0s, const double* nodes, const double* weights,
                      const double* xstarts, const double* dual_y_dx, const double* replay_x, double* values,
                      double* grad_x, double* grad_theta, int32_t* status, double* policy_x, double* obs,
                      int64_t* evals, uint32_t flags, void* stream);

/* ExpectedTrajectoryOutput per restart: eto R×W (row-major per restart, W = 2+2d+2):
 * [μxθ, σ_μxθ, ∇μx(d), σ_∇μx(d), ∇μθ, σ_∇μθ]; std uses n-1 (Q14).                     */
int mrbo_eto_reduce(mrbo_plan_t* plan, const double* values, const double* grad_x, const double* grad_theta,
                    double* eto, uint32_t flags, void* stream);

/* One step of the outer stochastic gradient ascent for the plan's R restarts, on the device
 * (stochastic_solve utils.jl:235-265): for every restart r with active[r] ≠ 0, eswavs
 * (utils.jl:114-123) on the ETO row r of eto (mrbo_eto_reduce's layout) with sample_size = the
 * global MC samples -- 1 − (sample_size/d)·Σ_a ∇μx_a²/σ_∇μx_a² > 0 sets active[r] = 0 -- else
 * StandardSGA update! (optimizers.jl:16-22) x0s[:, r] += η·∇μx.  Device pointers only (eto R×W,
 * x0s d×R, active R int32); asynchronous on `stream`, so consecutive launches of the ascent need
 * no host round trip.                                                                           */
int mrbo_sga_step(mrbo_plan_t* plan, const double* eto, double* x0s, int32_t* active, double sample_size, double eta,
                  uint32_t flags, void* stream);

/* The same step with Adam update! (optimizers.jl:49-74) in place of StandardSGA: m, v (device,
 * d×R, zero before the first update) are the restarts' moment estimates, t ≥ 1 the update count
 * of the active restarts (a restart that eswavs stops never updates again, so the active ones
 * share it); x0s[:, r] += η·m̂/(√v̂ + ε) with m̂ = m/(1 − β1^t), v̂ = v/(1 − β2^t).  The reference's
 * defaults: η = 0.001, β1 = 0.9, β2 = 0.999, ε = 1e-8 (optimizers.jl:35-40).                 */
int mrbo_adam_step(mrbo_plan_t* plan, const double* eto, double* x0s, int32_t* active, double* m, double* v, int32_t t,
                   double sample_size, double eta, double beta1, double beta2, double eps, uint32_t flags,
                   void* stream);

/* The reference's outer loop in ONE call: stochastic_solve(; optimizer, surrogate, tp, es, start)
 * (utils.jl:235-265) for the plan's R restarts at once -- the columns of x0s, e.g. the
 * generate_batch points (utils.jl:97-106) -- on the plan's surrogate, TrajectoryParameters and
 * inner starts.  Each iteration is [mrbo_simulate_mc at the current x0s, mrbo_eto_reduce,
 * mrbo_sga_step (StandardSGA update!, optimizers.jl:16-22) or mrbo_adam_step (Adam update!,
 * optimizers.jl:49-74)], at most opts->iterations (the reference: 50) times.  A restart stops
 * for good when its eswavs test (utils.jl:114-123) fires, as the reference's `break`; the call
 * returns once no restart is active (read back a few iterations behind the launches: the
 * iterations queued after the last stop find x0 unchanged and reproduce the same outputs) or the
 * budget is spent.  No host round trip per iteration, one plan, no plan rebuild.
 *   x0s      d×R in: the starts, out: get_starting_point(tpc) of every restart
 *   rnstream, xstarts, dual_y_dx   as mrbo_simulate_mc (dual_y_dx may be NULL)
 *   eto      R×W or NULL: the ETO rows (mrbo_eto_reduce's layout) of the last launch -- for a
 *            stopped restart, those at its final point
 *   active   R or NULL: 1 where eswavs never stopped the restart within the budget
 *   result   int32[3]: iterations launched, the iteration after which no restart was active (or
 *            the iterations launched), the OR of every launch's trajectory status bits (non-zero:
 *            the reference would have thrown -- the Julia method throws)
 * A status bit ends the ascent: like the stop flags, the bits of iteration j are read two iterations
 * behind the launches, so at most two more iterations follow the first one that carried a bit, and
 * result[2] holds theirs too.  x0s, eto and active are then those of the plain calls
 * [mrbo_simulate_mc, mrbo_eto_reduce, the step] repeated result[0] times: a restart with a failed
 * trajectory has a NaN ETO row, and the step moves its x0 to NaN (x += η·NaN).
 * Arrays are device pointers unless MRBO_FLAG_HOST_POINTERS (then staged once for the whole
 * ascent); synchronises `stream` before returning.                                            */
typedef enum {
  MRBO_OPT_SGA = 0,
  MRBO_OPT_ADAM = 1,
  MRBO_OPT_BOX_ADAM = 2   /* mrbo_rollout_solve only; mrbo_stochastic_solve refuses it */
} mrbo_optimizer_t;
typedef struct {
  int32_t optimizer;    /* mrbo_optimizer_t                                                  */
  int32_t iterations;   /* ≥ 1; the reference's loop: 50                                      */
  double eta;           /* StandardSGA η (default 0.01) / Adam η (default 0.001)              */
  double beta1;         /* Adam β1 (0.9); ignored by StandardSGA                              */
  double beta2;         /* Adam β2 (0.999)                                                    */
  double eps;           /* Adam ε (1e-8)                                                      */
  double sample_size;   /* eswavs sample size: global MC samples per restart (0 → the plan's M) */
} mrbo_solve_opts_t;
int mrbo_stochastic_solve(mrbo_plan_t* plan, double* x0s, const double* rnstream, const double* xstarts,
                          const double* dual_y_dx, const mrbo_solve_opts_t* opts, double* eto, int32_t* active,
                          int32_t* result, uint32_t flags, void* stream);

/* ---- the acquisition solve of a BO step (no reference counterpart: the reference's rollout solver
 * is undefined, experiments/adaptive_bayesopt.jl:490; the specification is the build's host-driven
 * loop, mrbo/bayesopt.py rollout_solve / rollout_solve_multi, and every output below is that loop's
 * bit for bit -- tests/test_gpu_rollout_solve.py).  All three work on plain plans and surrogate
 * batches; R is the plan's restarts per surrogate, the surrogate index is slowest.
 *
 * mrbo_box_adam_step: mrbo_adam_step with BoxAdam.update (mrbo/bayesopt.py) in place of Adam's: for
 * every restart with active[r] ≠ 0 the eswavs test, then, over the plan's box [lb, ub], w = ub − lb,
 *   u = (x − lb)/w,  g = ∇μx·w,  m ← β1·m + (1−β1)·g,  v ← β2·v + (1−β2)·g²,
 *   u ← u + η·(m/(1−β1^t))/(√(v/(1−β2^t)) + ε),  x ← clip(lb + w·u, lb, ub)
 * each operation rounded on its own; the clip by comparisons, so a NaN stays a NaN (numpy's clip).
 * Device pointers only (eto R·S×W, x0s / m / v d×R·S, active int32 R·S); asynchronous on `stream`.
 * MRBO_ERR_ARG, before any device call: a null argument, t < 1, a non-finite or negative eta, eps
 * or sample_size, β outside [0, 1), any flag.                                                   */
int mrbo_box_adam_step(mrbo_plan_t* plan, const double* eto, double* x0s, int32_t* active, double* m, double* v,
                       int32_t t, double sample_size, double eta, double beta1, double beta2, double eps,
                       uint32_t flags, void* stream);

/* bayesopt.pick_restart per surrogate: among the R final points x[:, :, q] (x d×R×S) with ETO rows
 * eto (R·S×W, only the means are read), the first one of the largest mean; means[r] is the mean, or
 * −∞ where it is not finite.  With incumbent ≠ 0 a restart is novel when
 *   min over the surrogate's N observed points X (the plan's device copy) of max_a |x_a − X_a|/w_a > 1e-9
 * (a non-finite coordinate: not novel), and while any restart of the surrogate is novel the others
 * rank −∞.  All ranks −∞: restart 0.  One workgroup per surrogate.
 *   xnext d×S: the picked points;  mean S: their means;  pick int32 S: their indices in 0..R−1
 *   means R×S or NULL
 * Device pointers only; asynchronous on `stream`.  MRBO_ERR_ARG, before any device call: a null plan,
 * x, eto, xnext, mean or pick, any flag.                                                       */
int mrbo_pick_restart(mrbo_plan_t* plan, const double* x, const double* eto, int32_t incumbent, double* xnext,
                      double* mean, int32_t* pick, double* means, uint32_t flags, void* stream);

/* rollout_solve_multi in ONE call.  The inputs are staged once (MRBO_FLAG_HOST_POINTERS; else they
 * are device pointers); then at most opts->iterations times [mrbo_simulate_mc with gradients at the
 * current x0s, mrbo_eto_reduce, mrbo_sga_step / mrbo_adam_step / mrbo_box_adam_step, the check
 * kernel] follow each other on the stream.  A restart that eswavs stops is skipped by the later
 * launches; the host reads the number of active restarts two iterations behind the launches and
 * ends the ascent once it is zero (the iterations queued meanwhile change nothing).  Unlike
 * mrbo_stochastic_solve, status bits do NOT end the ascent -- the host loop goes on, and the NaN
 * ETO rows of failed trajectories become −∞ means -- and the trajectory order is the plan's own.
 * Then x0s is projected onto the plan's box in place (NaN kept), ONE launch with
 * MRBO_FLAG_NO_GRADIENT evaluates every restart there (nothing skipped), mrbo_eto_reduce and
 * mrbo_pick_restart(opts->incumbent) follow, and the stream is synchronised, once.
 *   x0s      d×R×S in: the starts; out: the projected end points
 *   rnstream, xstarts   as mrbo_simulate_mc
 *   xnext, mean, pick, means   as mrbo_pick_restart (means may be NULL)
 *   active   int32 R×S or NULL: 1 where eswavs never stopped the restart within the budget
 *   result   HOST int32[4]: iterations launched; the iteration after which no restart was active
 *            (or the iterations launched); the OR of the status bits of the ascent's launches; the
 *            OR of the status bits of the final launch
 * MRBO_ERR_ARG, before any device call: a null plan, x0s, rnstream, xstarts, opts, xnext, mean, pick
 * or result; iterations < 1; an unknown optimizer; a non-finite or negative eta, eps or sample_size;
 * β outside [0, 1); a flag other than MRBO_FLAG_HOST_POINTERS.  The plan's mrbo_kernel_times ring
 * records every launch of the call.                                                            */
typedef struct {
  int32_t optimizer;    /* mrbo_optimizer_t: SGA, ADAM or BOX_ADAM                               */
  int32_t iterations;   /* ≥ 1                                                                   */
  double eta;           /* StandardSGA / Adam η; BOX_ADAM: box widths per step                   */
  double beta1;         /* Adam, BoxAdam β1 (0.9); ignored by StandardSGA                        */
  double beta2;         /* β2 (0.999)                                                            */
  double eps;           /* ε (1e-8)                                                              */
  double sample_size;   /* eswavs sample size (0 → the plan's M)                                 */
  int32_t incumbent;    /* ≠ 0: never pick an observed point while another restart ends elsewhere */
} mrbo_rollout_opts_t;
int mrbo_rollout_solve(mrbo_plan_t* plan, double* x0s, const double* rnstream, const double* xstarts,
                       const mrbo_rollout_opts_t* opts, double* xnext, double* mean, int32_t* pick, double* means,
                       int32_t* active, int32_t* result, uint32_t flags, void* stream);

/* ---- the EI control variate: variance-reduced ETO rows (the reference's --variance-reduction, "Use EI
 * as a control variate for variance reduction", experiments/nonmyopic_bayesopt.jl:64-66, ends in an
 * undefined solver; the definition is the build's, DESIGN.md §16, its specification mrbo/variance.py).
 * A trajectory's value is v = max(fmini − min_k y_k, 0); its step-0 part c = max(fmini − y_0, 0) is the
 * value of the same trajectory cut at horizon 0, with E[c] = EI0(x0) = σ·(u·Φ(u) + φ(u)) and
 * E[∇c] = φ(u)·∇σ − Φ(u)·∇μ, u = (fmini − μ)/σ, whatever the plan's rule, θ and cost model are.
 *
 * mrbo_simulate_control: the plan's own rollout launch run to horizon 0 on a plan of any h -- the
 * control samples of the trajectories mrbo_simulate_mc runs from the same x0s and rnstream (only the
 * stream's step-0 slab, its first M×(d+1) block, is read; a host stream is staged to that length).
 *   values0 M×R, grad_x0 d×M×R (may be NULL with MRBO_FLAG_NO_GRADIENT), status0 M×R
 * Bit-identical to mrbo_simulate_mc on a plan created with h = 0.  It honours the plan's order and a
 * solve's skipping of stopped restarts, and takes one entry of the timing ring.  Flags:
 * MRBO_FLAG_HOST_POINTERS, MRBO_FLAG_NO_GRADIENT; any other flag, a null plan or array: MRBO_ERR_ARG
 * before any device call.  Launches on `stream` without synchronising (device pointers).           */
int mrbo_simulate_control(mrbo_plan_t* plan, const double* x0s, const double* rnstream, const double* xstarts,
                          double* values0, double* grad_x0, int32_t* status0, uint32_t flags, void* stream);

/* mrbo_eto_reduce with the control variate.  Per restart and per series a -- the value and each
 * component of ∇x -- with target a_m (values / grad_x), control b_m (values0 / grad_x0) and the
 * control's expectation e:  ā = Σa/M, b̄ = Σb/M, da = a − ā, db = b − b̄, Sbb = Σdb², Sab = Σda·db,
 *   β = Sab/Sbb if Sbb > 0 and both sums are finite, else 0
 *   β ≠ 0:  mean = ā − β·(b̄ − e),  std = sqrt(Σ(da − β·db)²/(M − 1))
 *   β = 0:  the entries of mrbo_eto_reduce, bit for bit; e is not read (it may be NaN)
 * The ∇θ columns are always mrbo_eto_reduce's (the control does not depend on θ).  e comes from the
 * plan's base evaluation (the kernel of mrbo_eval_base) at x0s, launched by this call into a
 * plan-owned buffer (grown on first use), and the plan's fmini per surrogate.
 *   x0s d×R·S; values, grad_x, grad_theta as mrbo_eto_reduce (grad_x == NULL: value columns only, the
 *   gradient columns as mrbo_eto_reduce writes them and β_a = 0); values0, grad_x0 from
 *   mrbo_simulate_control at the same x0s; eto R·S×W in mrbo_eto_reduce's layout; beta (1+d)×R·S
 *   column-major [value, ∇x (d)] per restart, or NULL
 * Device pointers only; asynchronous on `stream`.  MRBO_ERR_ARG, before any device call: a null plan,
 * x0s, values, values0 or eto, grad_x without grad_x0, any flag.                                  */
int mrbo_eto_reduce_cv(mrbo_plan_t* plan, const double* x0s, const double* values, const double* grad_x,
                       const double* grad_theta, const double* values0, const double* grad_x0, double* eto,
                       double* beta, uint32_t flags, void* stream);

/* The switch (default off).  On: mrbo_rollout_solve runs, per iteration, [mrbo_simulate_mc,
 * mrbo_simulate_control, mrbo_eto_reduce_cv, the step, the check], and its tail the same two launches
 * without gradients before mrbo_pick_restart; stopped restarts are skipped in both launches; result[2]
 * and result[3] OR the status bits of both; the timing ring records both.  mrbo_stochastic_solve --
 * the reference's stochastic_solve, which has no control variate -- returns MRBO_ERR_UNSUPPORTED
 * before any device call.  mrbo_eto_reduce, the moments calls and mrbo_simulate_* ignore the switch,
 * and with it off every output of every call keeps its bits.  A null plan: MRBO_ERR_ARG.          */
int mrbo_plan_set_control_variate(mrbo_plan_t* plan, int32_t on);

/* Shard moments for the multi-GPU exchange: moments R×(2+2d+2) = [Σα, M2α, Σ∇x(d), M2∇x(d), Σ∇θ, M2∇θ]
 * over the first M_local samples of each restart (the outputs keep the plan's M as the restart
 * stride; 1 ≤ M_local ≤ M), M2 = Σ(x − x̄_local)² by two passes.  Ranks all-gather
 * (n, Σ, M2) and merge them with Chan's formula (mrbo/parallel.py merge_moments), which gives the
 * two-pass mean / std(n-1) of rollout.jl:328-339 without one-pass cancellation.            */
int mrbo_partial_moments(mrbo_plan_t* plan, const double* values, const double* grad_x, const double* grad_theta,
                         int32_t M_local, double* moments, uint32_t flags, void* stream);

/* The exchange's merge on the device (no host round trip per SGA step): moments = the nshards
 * ranks' mrbo_partial_moments blocks concatenated in rank order (nshards × R×W, what one
 * all-gather of the flat blocks produces), counts = their sample counts (HOST int64[nshards],
 * the shard sizes every rank knows; 1 ≤ nshards ≤ 64, a zero-count shard is skipped).  Chan's
 * pairwise merge left to right, then the ETO rows (mrbo_eto_reduce's layout, std n−1, Q14) into
 * eto (device, R×W) -- the same operations in the same order as mrbo/parallel.py merge_moments +
 * eto_from_moments.  Device pointers only; asynchronous on `stream`.                       */
int mrbo_merge_moments(mrbo_plan_t* plan, int32_t nshards, const double* moments, const int64_t* counts, double* eto,
                       uint32_t flags, void* stream);

/* eval(s, x, θ) of the base surrogate at P points xs (d×P); out stride 3+4d+d²:
 * [μ, σ, α, ∇μ(d), ∇σ(d), ∇α(d), Hα(d×d col-major), d2α/dxdθ(d)].                       */
int mrbo_eval_base(mrbo_plan_t* plan, int32_t P, const double* xs, double* out, uint32_t flags, void* stream);

/* base_solve(s::Surrogate; spatial_lbs, spatial_ubs, xstart, θfixed) rbf_optim.jl:35-66 for each
 * of n starts (columns of xstarts, d×n; any n ≥ 1; a boxed plan: d×n×S, block q the starts of
 * surrogate q) on the plan's BASE surrogate, with the plan's
 * rule, θ, box and solver options (the build's projected Newton, DESIGN.md §3, as the rollout's
 * inner solve): xmin d×n = the minimizers, fmin n = the minima of −α, status n (MRBO_ST_* bits
 * except ALL_NAN), evals MRBO_NCOUNTERS×n or NULL.  One wavefront per start.  The caller takes
 * multistart_base_solve!'s findmin over the candidates (rbf_optim.jl:103-135: drop minimizers
 * with a NaN, a NaN minimum wins, else the first minimum) -- mrbo/rbf_optim.py does.  Arrays are
 * device pointers unless MRBO_FLAG_HOST_POINTERS; launches on `stream` without synchronising. */
int mrbo_base_solve(mrbo_plan_t* plan, int32_t n, const double* xstarts, double* xmin, double* fmin, int32_t* status,
                    int64_t* evals, uint32_t flags, void* stream);

/* Base-GP fit at P hyperparameter vectors θ_p = thetas[p·nt .. p·nt+nt−1] (kernel, σn2, X d×N,
 * y N from s; s->L, s->c unused) -- the evaluations behind optimize!'s fg! (r_b_s.jl:810-814):
 * K = Ψ(‖Xi−Xj‖; θ_p)+σn2·I, L = chol(K), c = L'\(L\y), and
 *   ll[p]         = log_likelihood  (r_b_s.jl:770-776) = −yᵀc/2 − Σ log L_ii − N·log(2π)/2
 *   grad[p·nt+t]  = ∇log_likelihood (r_b_s.jl:787-799) = (cᵀ δK_t c − tr(L'\(L\δK_t)))/2,
 *                   δK_t = eval_Dθ_KXX(ψ, X, e_t) (radial_basis_functions.jl:264-284)
 * θ = (ℓ) for Matérn-5/2, -3/2, -1/2 and SE (nt = 1); Periodic (radial_basis_functions.jl:98-103)
 * takes θ = (ℓ, p) (nt = 2) or (ℓ) with p = s->period (nt = 1: ∂/∂ℓ only).
 * status[p] = 0, or 1 when cholesky throws PosDefException (ll, grad = NaN).  L_out (N×N×P,
 * lower, zeros above) and c_out (N×P) are optional (NULL).  thetas / ll / grad / status / L_out
 * / c_out are device pointers unless MRBO_FLAG_HOST_POINTERS; N ≤ 512 (every N the rollout
 * accepts).  Kernel by size: N ≤ 32 (and any N > 80) runs the 32 × 32-tile kernel on the fp64
 * matrix cores with ((2 + nt)·T(T+1)/2 + T)·1024·P doubles of workspace, T = ⌈N/32⌉, from the
 * per-device pool; 32 < N ≤ 64 with d ≤ 16 and without L_out / c_out runs the register kernel
 * (one candidate per workgroup, no workspace); otherwise 32 < N ≤ 80 with d ≤ 16 runs the LDS
 * kernel (the candidate in LDS, no workspace); d > 16 runs the tile kernel.  A configuration whose LDS (dynamic + the kernel's static arrays) exceeds
 * the device limit fails with MRBO_ERR_UNSUPPORTED.  Synchronises the stream before returning.
 * This is the S = 1 case of mrbo_gp_fit_multi (one code path, one launch of grid (P, 1)). */
int mrbo_gp_fit_theta(const mrbo_surrogate_t* s, int32_t P, int32_t nt, const double* thetas, double* ll,
                      double* grad, int32_t* status, double* L_out, double* c_out, uint32_t flags, void* stream);
/* mrbo_gp_fit_theta with nt = 1: ells[p] = ℓ_p, dll[p] = ∂ll/∂ℓ (Periodic: p = s->period). */
int mrbo_gp_fit(const mrbo_surrogate_t* s, int32_t P, const double* ells, double* ll, double* dll, int32_t* status,
                double* L_out, double* c_out, uint32_t flags, void* stream);

/* mrbo_gp_fit_theta for S data sets s[0..S-1] with P hyperparameter vectors each, in ONE launch of
 * grid (P, S) -- the refits of k lockstep BO trials (no reference counterpart: optimize! runs per
 * surrogate, r_b_s.jl:805-829).  The data sets share d, N, kernel and σn2 and differ in X, y and,
 * for Periodic with nt = 1, in period; lengthscale, L, c and fmini are unused.  The data set index
 * is slowest everywhere, as in mrbo_plan_create_batch: thetas nt×P×S, ll and status P×S, grad
 * nt×P×S, L_out N×N×P×S and c_out N×P×S (both optional).  Workgroup (p, q) fits data set q at
 * θ_{p,q} with the code of a plain call: block q of every output is bit-identical to
 * mrbo_gp_fit_theta(&s[q], P, nt, thetas + q·nt·P, ...), and a PosDefException in one slot
 * (status 1, NaN ll and grad) leaves every other slot of the launch as it is.  Kernel selection,
 * the LDS limit, pointer and flag conventions are those of mrbo_gp_fit_theta; the tile kernel's
 * workspace is its per-candidate size × P·S from the per-device pool (MRBO_ERR_NOMEM when that
 * fails).  All S data sets (and θ of a host call) go to the device in one copy, the small
 * outputs of a host call come back in one.  MRBO_ERR_ARG, before any device call: S < 1, P < 1,
 * an entry without X or y, an entry whose d, N, kernel or σn2 differs from s[0]'s, nt outside the
 * kernel's range, Periodic with nt = 1 and a non-positive period in any entry.  N > 512 (or
 * S > 65535) is MRBO_ERR_UNSUPPORTED.  Synchronises the stream before returning;
 * mrbo_last_gp_fit_ms reports the launch. */
int mrbo_gp_fit_multi(const mrbo_surrogate_t* s, int32_t S, int32_t P, int32_t nt, const double* thetas, double* ll,
                      double* grad, int32_t* status, double* L_out, double* c_out, uint32_t flags, void* stream);

/* optimize!(s; lowerbounds, upperbounds, optim_options) r_b_s.jl:805-829 for S data sets in ONE
 * call: S independent minimisations of −log_likelihood over the box [lower, upper], problem q from
 * theta0[q·nt ..] on data set s[q], by the build's projected L-BFGS with a batched backtracking line
 * search (mrbo/mle.py lbfgs_scalar is its specification, operation for operation).  The data sets
 * are staged once; one fit launch of grid (1, S) evaluates the clipped starts, then every round is
 * one fit launch of grid (12, S) -- the trial steps 1, 1/2, ..., 2⁻¹¹ of every problem -- and one
 * step kernel that accepts the line search, updates x, f, g and the (s, y) history and proposes the
 * next 12 trial θ, all on the device and without a host round trip: at most iterations + 1 rounds,
 * the start's included.  A stopped problem (converged, no Armijo step, zero move, budget spent)
 * keeps its state and its trial θ (its clipped start, if it stopped before any line search); the host reads the number of running problems two rounds
 * behind the launches, and the rounds launched after the last stop change no output.  A fit with
 * status ≠ 0 counts as f = NaN (never accepted; a failing start stops its problem after one line
 * search, with f = NaN at its clipped start).
 *   theta0   nt×S starts;  lower, upper  nt box bounds (HOST memory, finite, lower ≤ upper)
 *   opts     NULL: the defaults (a zero field takes its default)
 *   theta    nt×S minimisers;  nll  S: −log_likelihood there;  grad  nt×S: its gradient
 *   iters    S: line searches made (projected_lbfgs's iteration count)
 *   result   HOST int32[2]: rounds launched, the round after which no problem ran (1 + max iters)
 * theta0 / theta / nll / grad / iters are device pointers unless MRBO_FLAG_HOST_POINTERS.  The
 * checks on s, S and nt are mrbo_gp_fit_multi's; MRBO_ERR_ARG, before any device call, also for
 * lower > upper, a non-finite bound, history outside 1..16 (0: default), iterations < 0, a
 * negative or non-finite g_tol or c1, a null array, a flag other than MRBO_FLAG_HOST_POINTERS.  Kernel selection, workspace and the LDS limit
 * are those of a mrbo_gp_fit_multi call with P = 12.  Synchronises the stream once, at the end;
 * mrbo_last_gp_fit_ms is left as it was. */
typedef struct {
  int32_t iterations;  /* line searches at most (Optim.Options(iterations=30)); 0 → 30 */
  int32_t history;     /* L-BFGS pairs kept, 1..16; 0 → 10 */
  double  g_tol;       /* 0 → 1e-8 */
  double  c1;          /* Armijo constant; 0 → 1e-4 */
} mrbo_mle_opts_t;
int mrbo_gp_optimize_multi(const mrbo_surrogate_t* s, int32_t S, int32_t nt, const double* theta0,
                           const double* lower, const double* upper, const mrbo_mle_opts_t* opts, double* theta,
                           double* nll, double* grad, int32_t* iters, int32_t* result, uint32_t flags, void* stream);

/* The profiled-amplitude likelihood (build-defined, no reference counterpart): the data r = s->y are
 * modelled as r = s·g with g ~ GP(0, ψ_θ) + σn2 noise, and the amplitude sits at its closed-form
 * maximiser ŝ²(θ) = q/N, q = rᵀc, c = K⁻¹r, K = Ψ(θ) + σn2·I (the caller centres r).  What is left is
 *   ll[p]        = −(N/2)·log(q/N) − Σ log L_ii − (N/2)(1 + log 2π)
 *   grad[p·nt+t] = (N/(2q))·(cᵀ δK_t c) − tr(K⁻¹ δK_t)/2
 *   s2[p]        = q/N
 * from the sums the plain fit's kernels already hold (same kernels, same launch, another epilogue).
 * mrbo_gp_fit_profile_multi is mrbo_gp_fit_multi in every other respect -- layouts, checks, kernel
 * selection, workspace, synchronisation, L_out and c_out (bit-identical to the plain call's: they
 * do not depend on the amplitude) -- with s2 (P×S, as ll; not NULL: MRBO_ERR_ARG) as one more
 * output.  status[p] = 2 marks a slot whose q is not positive and finite (constant data: r = 0
 * after centring): ll, grad and s2 are NaN there, and every other slot of the launch is as it
 * would be without it, as for status 1. */
int mrbo_gp_fit_profile_multi(const mrbo_surrogate_t* s, int32_t S, int32_t P, int32_t nt, const double* thetas,
                              double* ll, double* grad, double* s2, int32_t* status, double* L_out, double* c_out,
                              uint32_t flags, void* stream);
/* mrbo_gp_optimize_multi minimising −ll_p: the fit launches run in profile mode, the step kernel
 * and every rule of the minimisation are the same.  s2 (S; device pointer unless
 * MRBO_FLAG_HOST_POINTERS; not NULL: MRBO_ERR_ARG) receives ŝ² at the returned theta, the accepted
 * point's (NaN where the start's fit failed). */
int mrbo_gp_optimize_profile_multi(const mrbo_surrogate_t* s, int32_t S, int32_t nt, const double* theta0,
                                   const double* lower, const double* upper, const mrbo_mle_opts_t* opts,
                                   double* theta, double* nll, double* grad, double* s2, int32_t* iters,
                                   int32_t* result, uint32_t flags, void* stream);

/* ARD lengthscales (build-defined, no reference counterpart): θ = (ℓ_1 … ℓ_d), one lengthscale per
 * input dimension, for Matérn-5/2, -3/2, -1/2 and SE.  These kernels see x only through
 * ρ = ‖(x − x′)/ℓ‖, so the model is the unit-lengthscale GP on z = x/ℓ (componentwise):
 *   K_ik = ψ(ρ_ik; ℓ = 1) + σn2·δ_ik,  ρ_ik = ‖z_i − z_k‖,
 *   ∂K_ik/∂ℓ_u = g(ρ_ik)·(x_iu − x_ku)²/ℓ_u³,  g(ρ) = −ψ′(ρ; 1)/ρ  (0 on the diagonal and where ρ_ik = 0).
 * s[q].lengthscale and s[q].period are ignored.
 *
 * mrbo_gp_fit_ard_multi: mrbo_gp_fit_multi's layouts with nt = d -- ells d×P×S (candidate p of data
 * set q at ells[(p + q·P)·d ..]), ll P×S, grad d×P×S, status P×S, L_out N×N×P×S (zeros above the
 * diagonal) and c_out N×P×S optional.  s2 = NULL: the plain likelihood, ll = −yᵀc/2 − Σ log L_ii −
 * (N/2) log 2π and grad_u = (cᵀδK_u c − tr(K⁻¹δK_u))/2.  s2 (P×S) given: the profiled-amplitude
 * likelihood of mrbo_gp_fit_profile_multi with the same δK_u, and s2 = yᵀc/N.
 * status: 0 ok; 1 a pivot is not positive; 2 profile mode and yᵀc is not positive and finite;
 * 3 some ℓ_u is not positive and finite (checked before K is built).  ll, grad and s2 are NaN on any
 * non-zero status, and every other slot of the launch is as it would be without the failing one:
 * block q carries the bits of the S = 1 call on data set q, candidate p those of a P = 1 call.
 * Before any device call: mrbo_gp_fit_multi's checks on s, S and P; Periodic → MRBO_ERR_ARG;
 * N > 128 or d > 16 → MRBO_ERR_UNSUPPORTED (one workgroup holds a candidate's z, factor, inverse and
 * coefficients in LDS). */
int mrbo_gp_fit_ard_multi(const mrbo_surrogate_t* s, int32_t S, int32_t P, const double* ells, double* ll,
                          double* grad, double* s2, int32_t* status, double* L_out, double* c_out, uint32_t flags,
                          void* stream);
/* mrbo_gp_optimize_multi over the d lengthscales: ell0 d×S starts, lower and upper d each (HOST
 * memory; non-finite or lower > upper → MRBO_ERR_ARG), ells and grad d×S, nll, iters S.  s2 = NULL
 * minimises −ll, s2 (S) given −ll_p with ŝ² at the returned ells.  The step kernel performs
 * mle.lbfgs_scalar's operations on d variables in its order (a dot product is a0·b0 + a1·b1 + …
 * left to right, nothing fused), so the result is the specification's bit for bit. */
int mrbo_gp_optimize_ard_multi(const mrbo_surrogate_t* s, int32_t S, const double* ell0, const double* lower,
                               const double* upper, const mrbo_mle_opts_t* opts, double* ells, double* nll,
                               double* grad, double* s2, int32_t* iters, int32_t* result, uint32_t flags,
                               void* stream);

/* Host helpers (HOST memory). */
int mrbo_rnstream(int32_t M, int32_t d, int32_t H, double* out);                 /* M×(d+1)×H */
int mrbo_initial_guesses(int32_t n, int32_t d, const double* lbs, const double* ubs, double* out); /* d×(n+2) */
double mrbo_dual_uniform(uint64_t seed, int64_t traj, int32_t j, int32_t k);

/* Timing of the last mrbo_simulate_mc / _ghq rollout kernel on its stream (HIP events around the
 * kernel launch alone), milliseconds; -1 before the first launch.  Waits for that launch.
 * mrbo_simulate_control is such a launch too: it takes one entry of the ring.                  */
double mrbo_last_kernel_ms(mrbo_plan_t* plan);

/* The same for the plan's last min(n, launches, 64) launches, oldest first, into ms[]; returns the
 * number written (≥ 0) or a negative mrbo_err_t.  Waits for those launches.                    */
int mrbo_kernel_times(mrbo_plan_t* plan, int32_t n, double* ms);

/* Kernel time of the last mrbo_gp_fit / _theta / _multi launch (HIP events around it), milliseconds; -1 before
 * the first call.  Process-wide (the last call on any stream). */
double mrbo_last_gp_fit_ms(void);

/* Launch geometry of a plan (no reference counterpart; measurement and FLOP accounting):
 * info[0..6] = rows per lane (1/2/4), workgroups, waves per workgroup, batched start values
 * (0/1), compile-time specialised kernel (0 generic, 1 Matérn-5/2 + EI, 2 its half-wave form: N ≤ 32, d ≤ 4, h ≤ 3, 3 Matérn-5/2 + EI + quadratic cost), LDS bytes per workgroup,
 * fantasy capacity of the kernel unit (4: the FMAX = 4 units of h ≤ 3, d ≤ 8; else 6);
 * info[7] = S, the plan's base surrogates (1: a plain plan; info[1] stays the workgroups of a plain
 * launch, a surrogate batch launches ⌈info[1]/S⌉ × S);
 * info[8] = restart table (1: the step-0 evaluation at x0 and the factor of its draw run once per
 * restart and every sample reads them; 0: every trajectory runs them -- MRBO_RESTART_TABLES=0 in the
 * environment at plan creation, the half-wave kernel, N > 64);
 * info[9] = fused Newton iteration of the inner solve (1: an accepted line-search trial that does not
 * end the iteration goes on to its gradient and Hessian in the same evaluation call; 0: the two-call
 * loop -- MRBO_NEWTON_FUSED=0 in the environment at plan creation, the half-wave kernel, N > 64);
 * results are bit-identical either way.  Writes min(n, 10). */
int mrbo_plan_info(const mrbo_plan_t* plan, int32_t* info, int32_t n);

/* Work order of the plan's later mrbo_simulate_mc / mrbo_simulate_ghq launches (no reference
 * counterpart; scheduling only, results do not depend on it): `order` is a DEVICE array of n =
 * M×R int32 trajectory indices (m + M·r), a permutation, handed to the persistent waves in that
 * order -- e.g. longest first by the previous launch's work counters, which shortens the launch's
 * tail.  Caller-owned; it must stay valid while launches use it.  NULL restores the identity.
 * n != M×R: MRBO_ERR_ARG; a surrogate batch (S > 1): MRBO_ERR_UNSUPPORTED.  An entry outside [0, M×R) runs the trajectory of its own queue index
 * (no write outside the outputs); tests/test_gpu_schedule.py holds every output bit-identical
 * under permuted, out-of-range and longest-first orders.  The library does not check that the
 * order is a permutation: with a duplicated index (or a mix of out-of-range entries and valid
 * ones that name the same trajectory) one trajectory runs on two waves at once and another never
 * runs -- its outputs are left undefined.  The Python mirror (RolloutPlan.set_order) checks. */
int mrbo_plan_set_order(mrbo_plan_t* plan, const int32_t* order, int64_t n);

/* The same, with the order computed on the device by the library (no reference counterpart;
 * scheduling only): `evals` is a DEVICE array of M×R×5 work counters as a previous
 * mrbo_simulate_mc on this plan wrote them.  The rollout kernel's waves drain one queue per XCD
 * over a contiguous eighth of the queue positions, chunk x = [x·T/8, (x+1)·T/8), before the
 * others; the order keeps every trajectory in its own chunk and puts each chunk's trajectories
 * longest first by their weighted work (grad 2.5, value 1, Hessian 3, adjoint rich evaluation 5,
 * adjoint pair 3, in value-evaluation units; one stable descending radix sort, ties in index
 * order), so the launch no longer ends on its longest trajectories and each XCD still writes one
 * contiguous range of output rows.  The plan owns the order (grown on demand, freed with the
 * plan); the plan's later launches use it until mrbo_plan_set_order replaces it (NULL:
 * identity).  Stream-ordered: no host round trip.  `order_out` (DEVICE, M×R int32, or NULL)
 * receives a copy of the order.  mrbo_stochastic_solve does this after its first launch when the
 * caller has set no order.  M×R ≥ 2^31: MRBO_ERR_ARG.                                          */
int mrbo_plan_order_longest_first(mrbo_plan_t* plan, const int64_t* evals, int32_t* order_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
