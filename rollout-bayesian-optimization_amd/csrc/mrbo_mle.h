// mrbo_mle.h -- interface between the host API (mrbo_api.hip) and the step kernel of
// mrbo_gp_optimize_multi (mrbo_mle.hip): the projected L-BFGS between two fit launches, S
// independent problems over nt ≤ 16 hyperparameters, one thread each.  The fit launches
// (mrbo_gpfit.hip) read `trial` (the start launch: `x`) and write ll, gll, status; the rest is the
// minimiser's own state.
#pragma once
#include <hip/hip_runtime.h>

namespace mrbo {

constexpr int MLE_STEPS = 12;      // trial steps of one line search: 1, 1/2, ..., 2⁻¹¹ (mle.py _STEPS)
constexpr int MLE_HIST_MAX = 16;   // L-BFGS pairs kept, at most
constexpr int MLE_NT_MAX = 16;     // 1 (ℓ), 2 (ℓ, p: Periodic), or d ≤ 16 lengthscales (the ARD refit)

struct MleParams {
  int S, nt, m, iterations;        // m: pairs kept
  double g_tol, c1;
  double lo[MLE_NT_MAX], hi[MLE_NT_MAX];
  const double* theta0;            // nt×S starts (mle_init_kernel reads them)
  double* trial;                   // nt×MLE_STEPS×S: the points of the line search
  const double* ll;                // P×S: P = 1 after the start launch, MLE_STEPS after a line search
  const double* gll;               // nt×P×S: ∇ll
  const int* status;               // P×S
  double* x;                       // nt×S: the iterate -- the call's theta output
  double* f;                       // S: −ll there (nll)
  double* g;                       // nt×S: its gradient (grad)
  int* it;                         // S: line searches made (iters)
  double* hs;                      // nt×m×S: the s vectors, a ring of m per problem
  double* hy;                      // nt×m×S: the y vectors
  double* al;                      // m×S: the two-loop recursion's α
  int* ring;                       // 3×S: pairs held, position of the oldest, 1 while the problem runs
  int* check;                      // the check ring, one int per slot: problems still running
  // profile-mode fits (mrbo_gp_optimize_profile_multi): the fit launches also write the profiled
  // amplitude of every slot, and the iterate's is kept beside f.  Both null otherwise.
  const double* s2_fit;            // P×S, as ll
  double* s2;                      // S: ŝ² at the iterate
};

// x = clip(theta0) and every trial point = x; no pairs, no line search made, every problem running
void launch_mle_init(hipStream_t st, const MleParams& p);
// first: take f, g from the start launch (P = 1); else accept the line search (P = MLE_STEPS).
// Then propose the next line search into `trial`, or stop; check[slot] = problems still running.
void launch_mle_step(bool first, int slot, hipStream_t st, const MleParams& p);

}  // namespace mrbo
