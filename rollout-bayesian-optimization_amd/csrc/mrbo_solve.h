// mrbo_solve.h -- interface between the host API (mrbo_api.hip) and the kernels of
// mrbo_rollout_solve that the outer ascent did not have yet (mrbo_solve.hip): BoxAdam's step, the
// projection of the end points onto the box and the choice among the restarts.  The rollout
// launches, the ETO reduction, the StandardSGA / Adam steps and the check kernel are mrbo_api.hip's.
#pragma once
#include <hip/hip_runtime.h>

namespace mrbo {

// eswavs (utils.jl:114-123) on the ETO row e of one restart: stop when 1 − (M/d)·Σ_a ∇_a²/σ_a² > 0 (a
// NaN ratio keeps iterating, as in Julia).  The d ratios are summed in index order.
__device__ __forceinline__ bool eswavs_stops(const double* e, int d, double sample_size) {
#pragma clang fp contract(off)   // the host mirror's (numpy) roundings: no fused multiply-adds
  double ratio = 0.0;
  for (int a = 0; a < d; ++a) {
    const double g = e[2 + a], s = e[2 + d + a];
    ratio += (g * g) / (s * s);
  }
  return 1.0 - (sample_size / d) * ratio > 0.0;
}

// eswavs + BoxAdam.update for every active restart (R: all restarts of the plan, R·S on a
// surrogate batch); c1 = 1 − β1^t, c2 = 1 − β2^t formed on the host.  Restart r uses the box of
// surrogate r / Rs, box_stride doubles per surrogate into lbs / ubs (0: one box shared by all)
void launch_box_adam_step(hipStream_t st, const double* eto, double* x0s, int* active, double* m, double* v, int R,
                          int d, const double* lbs, const double* ubs, int Rs, long long box_stride,
                          double sample_size, double eta, double b1, double b2, double eps, double c1, double c2);

// x ← clip(x, lb, ub) for the n = d·Rs·S coordinates of x, a NaN kept; boxes as in the step
void launch_box_project(hipStream_t st, double* x, long long n, int d, const double* lbs, const double* ubs, int Rs,
                        long long box_stride);

struct PickParams {
  int d, N, R, S;
  int ldX;                 // X0 is [S][d][ldX], the first N entries of a row observed
  int incumbent;
  const double* X0;        // the plan's device copy of the observed points
  const double* lbs;       // surrogate q's box at lbs + q·box_stride (0: one box shared by all)
  const double* ubs;
  long long box_stride;
  const double* x;         // d×R×S
  const double* eto;       // R·S rows of W = 2 + 2d + 2, the mean first
  double* means;           // R×S: the means, −∞ where not finite (never null here)
  int* novel;              // R×S scratch
  double* xnext;           // d×S
  double* mean;            // S
  int* pick;               // S
};
// pick_restart, one workgroup per surrogate
void launch_pick_restart(hipStream_t st, const PickParams& p);

}  // namespace mrbo
