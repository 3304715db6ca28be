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
// ard = 1: one lengthscale per input dimension (mrbo_gpfit_ard.hip): GpFitParams carries nt = d and
// thetas d×P×S, θ_p = (ℓ_1 … ℓ_d); grad is d×P×S.  Either likelihood.  Status 3 marks a candidate
// with an ℓ_u that is not positive and finite.  N ≤ GPFIT_ARD_NMAX, d ≤ GPFIT_ARD_DMAX, no Periodic.
struct GpFitMode {
  int profile;
  double* s2;
  int ard;
};

// launch_gpfit (mrbo_dispatch.h) in the given mode (ard = 0)
void launch_gpfit(int P, int S, hipStream_t st, const GpFitParams& q, const GpFitMode& pm);

// the ARD fit (pm.ard = 1): one launch, grid (P, S), and its LDS bytes per workgroup
constexpr int GPFIT_ARD_NMAX = 128, GPFIT_ARD_DMAX = 16;
void launch_gpfit_ard(int P, int S, hipStream_t st, const GpFitParams& q, const GpFitMode& pm);
size_t gpfit_ard_lds();

}  // namespace mrbo
