// mrbo_cv.h -- interface between the host API (mrbo_api.hip) and the reduction of the EI control
// variate (mrbo_cv.hip): the ETO rows of a rollout launch with the horizon-0 launch of
// the same trajectories as the control and EI0(x0), ∇EI0(x0) as its known expectation.
#pragma once
#include <hip/hip_runtime.h>

namespace mrbo {

struct SurTab;

struct CvParams {
  int d, M, R, S;            // R: restarts per surrogate; the rows are R·S, the surrogate index slowest
  const double* values;      // M×R·S        the rollout launch (mrbo_simulate_mc)
  const double* grad_x;      // d×M×R·S      or null: value columns only
  const double* grad_theta;  // M×R·S        or null
  const double* values0;     // M×R·S        the control launch (mrbo_simulate_control)
  const double* grad_x0;     // d×M×R·S      (unread when grad_x is null)
  const double* base;        // mrbo_eval_base at the R·S points x0 on every surrogate:
                             // (3+4d+d²)×(R·S)×S; restart r of surrogate q reads point q·R + r of block q
  const SurTab* stab;        // the plan's per-surrogate table (fmini), null on a plain plan
  double fmini;              // a plain plan's fmini
  double* eto;               // R·S×W, mrbo_eto_reduce's layout
  double* beta;              // (1+d)×R·S or null
};

// grid (R·S, 1 + d + 1): one workgroup per restart and series (value, ∇x components, ∇θ)
void launch_cv_reduce(hipStream_t st, const CvParams& p);

}  // namespace mrbo
