// mrbo_solve.hip -- the kernels mrbo_rollout_solve adds to the outer ascent: BoxAdam's step, the
// projection of the end points onto the box, and the choice among the restarts' final ETO means.
//
// The specification is the host loop in mrbo/bayesopt.py (BoxAdam.update, rollout_solve's np.clip,
// pick_restart): every operation below is the one there, in its order, in fp64, each rounded on its
// own -- no fused multiply-add (contraction is off for this unit), IEEE division and square root.
// A clip is two comparisons, so a NaN passes through as it does through np.clip.  The work is a few
// scalar operations per restart; the rollout launches between two steps are the time.
#include <hip/hip_runtime.h>

#include <climits>

#include "mrbo_solve.h"

#pragma clang fp contract(off)

namespace mrbo {

namespace {

__device__ __forceinline__ double clip(double v, double lo, double hi) {
  if (v < lo) v = lo;
  if (v > hi) v = hi;
  return v;
}

// One thread per restart, as mrbo_adam_step: Adam's update on u = (x − lb)/w with the gradient g·w.
// Restart r of the R = Rs·S restarts belongs to surrogate r / Rs, whose box starts box_stride doubles
// after its predecessor's (a boxed plan: d; a shared box: 0).
__global__ void __launch_bounds__(64) box_adam_kernel(const double* eto, double* x0s, int* active, double* m, double* v,
                                                      int R, int d, const double* lbs, const double* ubs, int Rs,
                                                      long long box_stride, double sample_size, double eta, double b1,
                                                      double b2, double eps, double c1, double c2) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R || !active[r]) return;
  lbs += (r / Rs) * box_stride;
  ubs += (r / Rs) * box_stride;
  const double* e = eto + (size_t)(2 + 2 * d + 2) * r;
  if (eswavs_stops(e, d, sample_size)) {
    active[r] = 0;
    return;
  }
  for (int a = 0; a < d; ++a) {
    const size_t k = (size_t)d * r + a;
    const double lb = lbs[a], ub = ubs[a];
    const double w = ub - lb;
    double u = (x0s[k] - lb) / w;
    const double g = e[2 + a] * w;
    const double mk = b1 * m[k] + (1.0 - b1) * g;
    const double vk = b2 * v[k] + (1.0 - b2) * (g * g);
    m[k] = mk;
    v[k] = vk;
    u = u + (eta * (mk / c1)) / (__builtin_sqrt(vk / c2) + eps);
    x0s[k] = clip(lb + w * u, lb, ub);
  }
}

// coordinate k of the d·Rs·S: dimension k % d of restart k / d, surrogate k / (d·Rs)
__global__ void __launch_bounds__(64) box_project_kernel(double* x, long long n, int d, const double* lbs,
                                                         const double* ubs, int Rs, long long box_stride) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const long long a = k % d + (k / d / Rs) * box_stride;
  x[k] = clip(x[k], lbs[a], ubs[a]);
}

constexpr int PICK_THREADS = 256;

// Workgroup q serves surrogate q.  Pass 1, one thread per restart: its mean (−∞ where not finite)
// and, with the incumbent rule, whether it is novel -- the scan over the N observed points, the
// kernel's only loop of any size.  Pass 2: the first argmax of the ranks by a tree reduction whose
// ties go to the lower index.
__global__ void __launch_bounds__(PICK_THREADS) pick_kernel(PickParams p) {
  __shared__ double sv[PICK_THREADS];
  __shared__ int si[PICK_THREADS];
  __shared__ int any_novel;
  const int q = blockIdx.x, tid = threadIdx.x;
  const int d = p.d, R = p.R, W = 2 + 2 * d + 2;
  const double ninf = -__builtin_inf();
  const double* X = p.X0 + (size_t)q * d * p.ldX;
  const double* lbs = p.lbs + q * p.box_stride;   // workgroup q uses box q (a shared box: stride 0)
  const double* ubs = p.ubs + q * p.box_stride;
  if (tid == 0) any_novel = 0;
  __syncthreads();
  for (int r = tid; r < R; r += PICK_THREADS) {
    const size_t rg = (size_t)q * R + r;
    const double mu = p.eto[rg * W];
    p.means[rg] = __builtin_isfinite(mu) ? mu : ninf;
    int novel = 0;
    if (p.incumbent) {
      // min over the observed points of max_a |x_a − X_a|/w_a; a NaN anywhere makes both numpy
      // reductions NaN and the comparison false
      const double* xr = p.x + rg * d;
      bool nan = false;
      double mn = __builtin_inf();
      for (int j = 0; j < p.N; ++j) {
        double mx = 0.0;
        for (int a = 0; a < d; ++a) {
          const double t = fabs((xr[a] - X[(size_t)a * p.ldX + j]) / (ubs[a] - lbs[a]));
          if (t != t) nan = true;
          else if (t > mx) mx = t;
        }
        if (mx < mn) mn = mx;
      }
      novel = !nan && mn > 1e-9;
      if (novel) any_novel = 1;   // every writer stores the same value
    }
    p.novel[rg] = novel;
  }
  __syncthreads();   // this workgroup's means / novel flags, and any_novel
  const bool mask = p.incumbent && any_novel;
  double best = ninf;
  int bi = INT_MAX;
  for (int r = tid; r < R; r += PICK_THREADS) {
    const size_t rg = (size_t)q * R + r;
    const double rank = (mask && !p.novel[rg]) ? ninf : p.means[rg];
    if (bi == INT_MAX || rank > best) { best = rank; bi = r; }
  }
  sv[tid] = best;
  si[tid] = bi;
  __syncthreads();
  for (int s = PICK_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      const double ov = sv[tid + s];
      const int oi = si[tid + s];
      if (ov > sv[tid] || (ov == sv[tid] && oi < si[tid])) { sv[tid] = ov; si[tid] = oi; }
    }
    __syncthreads();
  }
  const int k = si[0];   // R ≥ 1: thread 0 holds restart 0 at least
  const size_t kg = (size_t)q * R + k;
  if (tid == 0) {
    p.pick[q] = k;
    p.mean[q] = p.means[kg];
  }
  for (int a = tid; a < d; a += PICK_THREADS) p.xnext[(size_t)q * d + a] = p.x[kg * d + a];
}

}  // namespace

void launch_box_adam_step(hipStream_t st, const double* eto, double* x0s, int* active, double* m, double* v, int R,
                          int d, const double* lbs, const double* ubs, int Rs, long long box_stride,
                          double sample_size, double eta, double b1, double b2, double eps, double c1, double c2) {
  hipLaunchKernelGGL(box_adam_kernel, dim3((R + 63) / 64), dim3(64), 0, st, eto, x0s, active, m, v, R, d, lbs, ubs,
                     Rs, box_stride, sample_size, eta, b1, b2, eps, c1, c2);
}

void launch_box_project(hipStream_t st, double* x, long long n, int d, const double* lbs, const double* ubs, int Rs,
                        long long box_stride) {
  hipLaunchKernelGGL(box_project_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, x, n, d, lbs, ubs, Rs,
                     box_stride);
}

void launch_pick_restart(hipStream_t st, const PickParams& p) {
  hipLaunchKernelGGL(pick_kernel, dim3(p.S), dim3(PICK_THREADS), 0, st, p);
}

}  // namespace mrbo
