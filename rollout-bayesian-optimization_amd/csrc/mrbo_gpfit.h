// mrbo_gpfit.h -- the mode of a fit launch (mrbo_gpfit.hip), beside GpFitParams (mrbo_dispatch.h,
// which the rollout units include too and which therefore stays as it is).
#pragma once
#include "mrbo_dispatch.h"

namespace mrbo {

// profile = 0: the plain likelihood of the data as given (log_likelihood, ∇log_likelihood); s2 unused.
// profile = 1: y = s·g, g ~ GP(0, ψ_θ) + σn2, with the amplitude at its closed-form maximiser
// ŝ² = yᵀc/N (c = K⁻¹y): ll and grad of GpFitParams receive the profiled likelihood
//   ll_p = −(N/2)·log(ŝ²) − Σ log L_ii − (N/2)(1 + log 2π),
//   ∂ll_p/∂θ_t = (cᵀδK_t c)/(2ŝ²) − tr(K⁻¹δK_t)/2
// and s2 (P×S) receives ŝ².  A candidate whose yᵀc is not positive and finite (constant data after
// centring) gets status 2 and NaN outputs.  L_out and c_out are the plain mode's.
struct GpFitMode {
  int profile;
  double* s2;
};

// launch_gpfit (mrbo_dispatch.h) in the given mode
void launch_gpfit(int P, int S, hipStream_t st, const GpFitParams& q, const GpFitMode& pm);

}  // namespace mrbo
