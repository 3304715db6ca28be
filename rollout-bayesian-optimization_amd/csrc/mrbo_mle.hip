// mrbo_mle.hip -- the minimiser of mrbo_gp_optimize_multi on the device: what mle.py's
// projected L-BFGS does between two evaluations, so that the S minimisations of −log_likelihood
// advance from fit launch to fit launch without a host round trip.
//
// One thread per problem (the work is a few hundred scalar operations on nt ≤ 16 variables; the
// fit launches between two steps are the time).  The specification is mle.py lbfgs_scalar: every
// operation below is the one there, in its order, in fp64, each rounded on its own -- no fused
// multiply-add (contraction is off for this unit), plain division and square root, a dot product
// as a0*b0 + a1*b1 + ... left to right.  The results are therefore the specification's bit for bit
// (tests/test_gpu_mle_device.py).  The iterate, its objective, gradient and iteration count live
// in the call's output arrays; the (s, y) pairs and the recursion's α in global memory, so no
// array is indexed at run time in registers and the kernel needs no scratch.
//
// A problem that has stopped is never touched again: its outputs and its trial points stay, the
// fit launches recompute the same values for it and nobody reads them.
#include <hip/hip_runtime.h>

#include "mrbo_mle.h"

#pragma clang fp contract(off)

namespace mrbo {

namespace {

template <int NT>
__host__ __device__ __forceinline__ double dot(const double (&a)[NT], const double (&b)[NT]) {
  double r = a[0] * b[0];
#pragma unroll
  for (int i = 1; i < NT; ++i) r = r + a[i] * b[i];
  return r;
}

// max |a_i|; a NaN stays (numpy's max)
template <int NT>
__host__ __device__ __forceinline__ double absmax(const double (&a)[NT]) {
  double r = fabs(a[0]);
#pragma unroll
  for (int i = 1; i < NT; ++i) {
    const double v = fabs(a[i]);
    if (v > r || v != v) r = v;
  }
  return r;
}

__host__ __device__ __forceinline__ double clip(double v, double lo, double hi) {
  if (v < lo) v = lo;
  if (v > hi) v = hi;
  return v;
}

template <int NT>
__host__ __device__ __forceinline__ void load(const double* src, size_t k, double (&a)[NT]) {
#pragma unroll
  for (int i = 0; i < NT; ++i) a[i] = src[k * NT + i];
}

template <int NT>
__host__ __device__ __forceinline__ void store(double* dst, size_t k, const double (&a)[NT]) {
#pragma unroll
  for (int i = 0; i < NT; ++i) dst[k * NT + i] = a[i];
}

// One step of problem q; returns 1 while it runs.
template <int NT>
__host__ __device__ int step_problem(const MleParams& p, int q, bool first) {
  int* const npairs = p.ring + 3 * (size_t)q;
  int* const oldest = npairs + 1;
  int* const running = npairs + 2;
  if (!*running) return 0;
  const int m = p.m;
  double* const hs = p.hs + (size_t)q * m * NT;
  double* const hy = p.hy + (size_t)q * m * NT;
  double* const al = p.al + (size_t)q * m;
  double x[NT], g[NT], f;
  load<NT>(p.x, q, x);
  if (first) {   // the start's evaluation, P = 1
    f = p.status[q] == 0 ? -p.ll[q] : __builtin_nan("");
    load<NT>(p.gll, q, g);
#pragma unroll
    for (int i = 0; i < NT; ++i) g[i] = -g[i];
    p.f[q] = f;
    store<NT>(p.g, q, g);
    if (p.s2) p.s2[q] = p.s2_fit[q];
  } else {       // the line search: the first trial step that is finite and meets Armijo
    f = p.f[q];
    load<NT>(p.g, q, g);
    const size_t k0 = (size_t)q * MLE_STEPS;
    int k = -1;
    double xn[NT], fn = 0.0;
    for (int kk = 0; kk < MLE_STEPS; ++kk) {
      const double ft = p.status[k0 + kk] == 0 ? -p.ll[k0 + kk] : __builtin_nan("");
      load<NT>(p.trial, k0 + kk, xn);
      double dx[NT];
#pragma unroll
      for (int i = 0; i < NT; ++i) dx[i] = xn[i] - x[i];
      if (__builtin_isfinite(ft) && ft <= f + p.c1 * dot<NT>(dx, g)) {
        k = kk;
        fn = ft;
        break;
      }
    }
    if (k < 0) {
      *running = 0;
      return 0;
    }
    double gn[NT], sk[NT], yk[NT];
    load<NT>(p.gll, k0 + k, gn);
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      gn[i] = -gn[i];
      sk[i] = xn[i] - x[i];
      yk[i] = gn[i] - g[i];
    }
    double thr = sqrt(dot<NT>(sk, sk)) * sqrt(dot<NT>(yk, yk));
    if (1e-300 > thr) thr = 1e-300;
    if (dot<NT>(sk, yk) > 1e-12 * thr) {   // keep the pair; the oldest leaves a full ring
      int at;
      if (*npairs < m) {
        at = (*oldest + *npairs) % m;
        *npairs += 1;
      } else {
        at = *oldest;
        *oldest = (at + 1) % m;
      }
      store<NT>(hs, at, sk);
      store<NT>(hy, at, yk);
    }
    const double moved = absmax<NT>(sk);
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      x[i] = xn[i];
      g[i] = gn[i];
    }
    f = fn;
    store<NT>(p.x, q, x);
    p.f[q] = f;
    store<NT>(p.g, q, g);
    if (p.s2) p.s2[q] = p.s2_fit[k0 + k];
    if (moved == 0.0) {
      *running = 0;
      return 0;
    }
  }
  // the next iteration: stop on the budget or at a projected stationary point, else a direction
  const int it = p.it[q];
  if (it >= p.iterations) {
    *running = 0;
    return 0;
  }
  bool free_[NT], any = false, small = true;
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    free_[i] = !((x[i] <= p.lo[i] && g[i] > 0.0) || (x[i] >= p.hi[i] && g[i] < 0.0));
    if (free_[i]) {
      any = true;
      if (!(fabs(g[i]) <= p.g_tol)) small = false;
    }
  }
  if (!any || small) {
    *running = 0;
    return 0;
  }
  p.it[q] = it + 1;
  // two-loop recursion on the free variables
  const int n = *npairs, o = *oldest;
  double r[NT], s_[NT], y_[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) r[i] = free_[i] ? g[i] : 0.0;
  for (int j = n - 1; j >= 0; --j) {
    const int at = (o + j) % m;
    load<NT>(hs, at, s_);
    load<NT>(hy, at, y_);
    const double a = dot<NT>(s_, r) / dot<NT>(y_, s_);
    al[at] = a;
#pragma unroll
    for (int i = 0; i < NT; ++i) r[i] = r[i] - a * y_[i];
  }
  if (n > 0) {
    const int at = (o + n - 1) % m;
    load<NT>(hs, at, s_);
    load<NT>(hy, at, y_);
    const double sc = dot<NT>(s_, y_) / dot<NT>(y_, y_);
#pragma unroll
    for (int i = 0; i < NT; ++i) r[i] = r[i] * sc;
  } else {   // first step: at most unit length
    double mx = absmax<NT>(r);
    if (1.0 > mx) mx = 1.0;
#pragma unroll
    for (int i = 0; i < NT; ++i) r[i] = r[i] / mx;
  }
  for (int j = 0; j < n; ++j) {
    const int at = (o + j) % m;
    load<NT>(hs, at, s_);
    load<NT>(hy, at, y_);
    const double b = dot<NT>(y_, r) / dot<NT>(y_, s_);
    const double ab = al[at] - b;
#pragma unroll
    for (int i = 0; i < NT; ++i) r[i] = r[i] + ab * s_[i];
  }
  double dir[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) dir[i] = -(free_[i] ? r[i] : 0.0);
  if (dot<NT>(g, dir) >= 0.0) {   // not a descent direction: steepest descent
#pragma unroll
    for (int i = 0; i < NT; ++i) dir[i] = -(free_[i] ? g[i] : 0.0);
  }
  double step = 1.0;
  for (int kk = 0; kk < MLE_STEPS; ++kk) {
    double t[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) t[i] = clip(x[i] + step * dir[i], p.lo[i], p.hi[i]);
    store<NT>(p.trial, (size_t)q * MLE_STEPS + kk, t);
    step = step * 0.5;
  }
  return 1;
}

__global__ void mle_init_kernel(MleParams p) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= p.S) return;
  for (int i = 0; i < p.nt; ++i) {
    const double x = clip(p.theta0[(size_t)q * p.nt + i], p.lo[i], p.hi[i]);
    p.x[(size_t)q * p.nt + i] = x;
    // a problem that stops before its first line search never proposes: its trial points are its
    // start, so the later fit launches find defined values in its slots
    for (int kk = 0; kk < MLE_STEPS; ++kk) p.trial[((size_t)q * MLE_STEPS + kk) * p.nt + i] = x;
  }
  p.it[q] = 0;
  p.ring[3 * (size_t)q] = 0;
  p.ring[3 * (size_t)q + 1] = 0;
  p.ring[3 * (size_t)q + 2] = 1;
}

// one workgroup: its threads take the problems in turn and count those still running
template <int NT>
__global__ void mle_step_kernel(MleParams p, int first, int slot) {
  __shared__ int nrun;
  if (threadIdx.x == 0) nrun = 0;
  __syncthreads();
  int mine = 0;
  for (int q = threadIdx.x; q < p.S; q += blockDim.x) mine += step_problem<NT>(p, q, first != 0);
  if (mine) atomicAdd(&nrun, mine);
  __syncthreads();
  if (threadIdx.x == 0) p.check[slot] = nrun;
}

}  // namespace

void launch_mle_init(hipStream_t st, const MleParams& p) {
  hipLaunchKernelGGL(mle_init_kernel, dim3((p.S + 63) / 64), dim3(64), 0, st, p);
}

void launch_mle_step(bool first, int slot, hipStream_t st, const MleParams& p) {
  const dim3 block(p.S <= 64 ? 64 : 256);
  // nt = 1, 2: ℓ and (ℓ, p); 3..16: the ARD refit's d lengthscales (mrbo_gp_optimize_ard_multi)
#define MRBO_MLE_STEP(NT) \
  case NT: hipLaunchKernelGGL(mle_step_kernel<NT>, dim3(1), block, 0, st, p, first ? 1 : 0, slot); break;
  switch (p.nt) {
    MRBO_MLE_STEP(1) MRBO_MLE_STEP(2) MRBO_MLE_STEP(3) MRBO_MLE_STEP(4) MRBO_MLE_STEP(5) MRBO_MLE_STEP(6)
    MRBO_MLE_STEP(7) MRBO_MLE_STEP(8) MRBO_MLE_STEP(9) MRBO_MLE_STEP(10) MRBO_MLE_STEP(11) MRBO_MLE_STEP(12)
    MRBO_MLE_STEP(13) MRBO_MLE_STEP(14) MRBO_MLE_STEP(15) MRBO_MLE_STEP(16)
    default: break;   // the host API admits nt ≤ MLE_NT_MAX only
  }
#undef MRBO_MLE_STEP
}

}  // namespace mrbo
