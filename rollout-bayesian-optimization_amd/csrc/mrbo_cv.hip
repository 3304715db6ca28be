// mrbo_cv.hip -- the reduction of the EI control variate (mrbo_eto_reduce_cv).
//
// Per restart and series a (the value, or one component of ∇x) the target samples a_m come from the
// rollout launch and the control samples b_m from the horizon-0 launch of the same trajectories,
// whose expectation e is known: EI0(x0) and ∇EI0(x0) from the base evaluation at x0.  With
//   ā = Σa/M, b̄ = Σb/M, da = a − ā, db = b − b̄, Sbb = Σdb², Sab = Σda·db,
//   β = Sab/Sbb if Sbb > 0 and both sums are finite, else 0
// the row entries are  mean = ā − β·(b̄ − e),  std = √(Σ(da − β·db)²/(M − 1))  when β ≠ 0, and the
// plain ones of mrbo_eto_reduce, bit for bit, when β = 0.  The ∇θ series is always the plain one.
//
// The specification is mrbo/variance.py cv_rows.  Scalar fp64, centred sums (the mean first, then
// the squares about it), no fused multiply-add (contraction is off for this unit) -- with ONE
// exception: the plain centred square sum is accumulated by an explicit fma, because that is how
// reduce_kernel (mrbo_api.hip, compiled with the default contraction) forms it, and a β = 0 row must
// have its bits.  The thread-strided partial sums and the 256-wide tree are reduce_kernel's too.
// The work is a few hundred scalar operations per workgroup beside a rollout launch of milliseconds.
#include <hip/hip_runtime.h>

#include "mrbo_device.h"
#include "mrbo_cv.h"

#pragma clang fp contract(off)

namespace mrbo {

namespace {

constexpr int CV_THREADS = 256;

__global__ void __launch_bounds__(CV_THREADS) cv_reduce_kernel(CvParams p) {
  __shared__ double sh[CV_THREADS];
  const int r = blockIdx.x, comp = blockIdx.y, tid = threadIdx.x;
  const int d = p.d, M = p.M;
  const int W = 2 + 2 * d + 2;
  auto elem = [&](int m) -> double {   // reduce_kernel's
    const long long idx = (long long)m + (long long)M * r;
    if (comp == 0) return p.values[idx];
    if (comp <= d) return p.grad_x ? p.grad_x[idx * d + (comp - 1)] : 0.0;
    return p.grad_theta ? p.grad_theta[idx] : 0.0;
  };
  auto ctrl = [&](int m) -> double {   // read only for a series with a control
    const long long idx = (long long)m + (long long)M * r;
    return comp == 0 ? p.values0[idx] : p.grad_x0[idx * d + (comp - 1)];
  };
  auto block_sum = [&](double v) -> double {
    sh[tid] = v;
    __syncthreads();
    for (int s = CV_THREADS / 2; s > 0; s >>= 1) {
      if (tid < s) sh[tid] += sh[tid + s];
      __syncthreads();
    }
    const double t = sh[0];
    __syncthreads();
    return t;
  };
  // workgroup-uniform: the value always has a control, a ∇x component when the caller has gradients
  const bool has_ctrl = comp == 0 || (comp <= d && p.grad_x != nullptr);

  double s = 0.0;
  for (int m = tid; m < M; m += CV_THREADS) s += elem(m);
  const double tot = block_sum(s);
  const double abar = tot / M;
  double s2 = 0.0;
  for (int m = tid; m < M; m += CV_THREADS) {
    const double dv = elem(m) - abar;
    s2 = __builtin_fma(dv, dv, s2);   // reduce_kernel's contraction (see the header)
  }
  const double tot2 = block_sum(s2);

  double bbar = 0.0, beta = 0.0, resid = 0.0;
  bool use = false;
  if (has_ctrl) {
    double sb = 0.0;
    for (int m = tid; m < M; m += CV_THREADS) sb += ctrl(m);
    bbar = block_sum(sb) / M;
    double sbb = 0.0, sab = 0.0;
    for (int m = tid; m < M; m += CV_THREADS) {
      const double da = elem(m) - abar, db = ctrl(m) - bbar;
      sbb += db * db;
      sab += da * db;
    }
    const double Sbb = block_sum(sbb);
    const double Sab = block_sum(sab);
    if (Sbb > 0.0 && __builtin_isfinite(Sbb) && __builtin_isfinite(Sab)) beta = Sab / Sbb;
    use = beta != 0.0;   // β = 0 (or no β): the plain row; a NaN β cannot arise from finite sums
    if (use) {
      double sr = 0.0;
      for (int m = tid; m < M; m += CV_THREADS) {
        const double t = (elem(m) - abar) - beta * (ctrl(m) - bbar);
        sr += t * t;
      }
      resid = block_sum(sr);
    }
  }
  if (tid != 0) return;

  int c0, c1;
  if (comp == 0) { c0 = 0; c1 = 1; }
  else if (comp <= d) { c0 = 2 + (comp - 1); c1 = 2 + d + (comp - 1); }
  else { c0 = 2 + 2 * d; c1 = 3 + 2 * d; }
  double mean = tot / M;
  double sd = sqrt(tot2 / (M - 1));
  if (use) {   // a select: the expectation is not formed, let alone read, for a plain row
    const int RS = p.R * p.S, q = r / p.R;
    const double* o = p.base + (size_t)(3 + 4 * d + d * d) * ((size_t)r + (size_t)RS * q);
    const double fmini = p.stab ? p.stab[q].fmini : p.fmini;
    const double mu = o[0], sig = o[1];
    const double u = (fmini - mu) / sig;
    const PhiPair pp = ei_phi_Phi(u);
    double e;
    if (comp == 0) e = sig * (u * pp.Phi + pp.phi);                        // EI0 = σ·(u·Φ(u) + φ(u))
    else e = pp.phi * o[3 + d + (comp - 1)] - pp.Phi * o[3 + (comp - 1)];  // ∇EI0 = φ·∇σ − Φ·∇μ
    mean = abar - beta * (bbar - e);
    sd = sqrt(resid / (M - 1));
  }
  p.eto[(long long)W * r + c0] = mean;
  p.eto[(long long)W * r + c1] = sd;
  if (p.beta && comp <= d) p.beta[(long long)(1 + d) * r + comp] = use ? beta : 0.0;
}

}  // namespace

void launch_cv_reduce(hipStream_t st, const CvParams& p) {
  hipLaunchKernelGGL(cv_reduce_kernel, dim3(p.R * p.S, p.d + 2), dim3(CV_THREADS), 0, st, p);
}

}  // namespace mrbo
