// device_probe.hip -- test-only launchers around the numeric building blocks of csrc/mrbo_device.h.
//
// One small kernel per primitive group, one extern "C" launcher per kernel.  Every launcher takes
// HOST pointers, copies in, launches, synchronises, copies out and returns the HIP error code
// (0 = success).  Element-wise kernels run one thread per input element and check their index
// against n; the reduction kernels run exactly one full wave, so no permlane / DPP source lane is
// inactive.  Built by tests/device_probe.py into tests/_probe/libmrbo_probe.so; never linked into
// libmrbo.so.
#include "mrbo_device.h"

#include <vector>

using namespace mrbo;

namespace {

// device buffers of one launcher call, freed on every exit path
struct Bufs {
  std::vector<void*> p;
  hipError_t err = hipSuccess;
  ~Bufs() {
    for (void* q : p) (void)hipFree(q);
  }
  template <class T>
  T* in(const T* host, size_t n) {
    T* d = out<T>(n);
    if (err == hipSuccess && n) err = hipMemcpy(d, host, n * sizeof(T), hipMemcpyHostToDevice);
    return d;
  }
  template <class T>
  T* out(size_t n) {
    void* d = nullptr;
    if (err == hipSuccess) {
      err = hipMalloc(&d, (n ? n : 1) * sizeof(T));
      if (err == hipSuccess) p.push_back(d);
    }
    return (T*)d;
  }
  template <class T>
  void back(T* host, const T* dev, size_t n) {
    if (err == hipSuccess && n) err = hipMemcpy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost);
  }
  void ran() {
    if (err == hipSuccess) err = hipGetLastError();
    if (err == hipSuccess) err = hipDeviceSynchronize();
  }
};

constexpr int TPB = 256;
inline int blocks(int n) { return (n + TPB - 1) / TPB; }

// ---- fexp against the device library's exp() ------------------------------------------------
__global__ void k_exp(const double* x, double* f, double* e, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  f[i] = fexp(x[i]);
  e[i] = exp(x[i]);
}

// ---- sqrt_rsqrt, fast_sqrt0, sig_isig: out[5n] = r, ir, fast_sqrt0, sig, isig ----------------
__global__ void k_roots(const double* s, double* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double r, ir, sg, isg;
  sqrt_rsqrt(s[i], r, ir);
  sig_isig(s[i], sg, isg);
  out[i] = r;
  out[n + i] = ir;
  out[2 * n + i] = fast_sqrt0(s[i]);
  out[3 * n + i] = sg;
  out[4 * n + i] = isg;
}

// ---- ei_phi_Phi: out[2n] = φ, Φ -------------------------------------------------------------
__global__ void k_phi(const double* z, double* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const PhiPair p = ei_phi_Phi(z[i]);
  out[i] = p.phi;
  out[n + i] = p.Phi;
}

// ---- rule_partials: out[14n], outputs 0..6 the seven-argument overload (isig passed in),
//      7..13 the six-argument one ------------------------------------------------------------
__device__ void put(const EIp& e, double* out, int n, int i) {
  out[i] = e.g;
  out[n + i] = e.gmu;
  out[2 * n + i] = e.gsig;
  out[3 * n + i] = e.gmumu;
  out[4 * n + i] = e.gsigsig;
  out[5 * n + i] = e.gmuth;
  out[6 * n + i] = e.gsigth;
}
__global__ void k_rule(int rule, const double* mu, const double* sig, const double* isig, double theta, double fmin,
                       double sigma_tol, double* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  put(rule_partials(rule, mu[i], sig[i], theta, fmin, sigma_tol, isig[i]), out, n, i);
  put(rule_partials(rule, mu[i], sig[i], theta, fmin, sigma_tol), out + 7 * (size_t)n, n, i);
}

// ---- rad_eval / rad_eval2: out[9n] = ψ, g1, g2 of rad_eval(ρ²_i); then the a and the b results of
//      rad_eval2(ρ²_i, ρ²_{n−1−i}) ------------------------------------------------------------
__global__ void k_rad(int kind, double cK, double cP, const double* rho2, double* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Radial k;
  k.kind = kind;
  k.cK = cK;
  k.cP = cP;
  double psi, g1, g2, pa, g1a, g2a, pb, g1b, g2b;
  rad_eval(k, rho2[i], psi, g1, g2);
  rad_eval2(k, rho2[i], rho2[n - 1 - i], pa, g1a, g2a, pb, g1b, g2b);
  const size_t N = n;
  out[i] = psi;
  out[N + i] = g1;
  out[2 * N + i] = g2;
  out[3 * N + i] = pa;
  out[4 * N + i] = g1a;
  out[5 * N + i] = g2a;
  out[6 * N + i] = pb;
  out[7 * N + i] = g1b;
  out[8 * N + i] = g2b;
}

// ---- cost_eval<D>, cost_hess<D>: x [n][D], c [n], gc [n][D], H [n][D][D] ---------------------
template <int D>
__global__ void k_cost(int cost, double c0, const double* tab, const double* x, double* c, double* gc, double* H,
                       int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  KParams kp = {};
  kp.cost = cost;
  kp.cost_c0 = c0;
  kp.cost_tab = tab;
  double xi[D], g[D];
  for (int a = 0; a < D; ++a) xi[a] = x[(size_t)i * D + a];
  const double ci = cost_eval<D>(kp, xi, g);
  c[i] = ci;
  for (int a = 0; a < D; ++a) gc[(size_t)i * D + a] = g[a];
  for (int a = 0; a < D; ++a)
    for (int b = 0; b < D; ++b) H[((size_t)i * D + a) * D + b] = cost_hess<D>(kp, ci, a, b);
}

// ---- reductions: ONE wave.  in [64][K] (lane-major), red [K] (wave_reduce) or [2][K]
//      (half_reduce, one block of K sums per 32-lane half) -----------------------------------
template <int K, bool HALF>
__global__ void __launch_bounds__(64) k_reduce(const double* in, double* red) {
  const int lane = threadIdx.x;
  double v[K];
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = in[lane * K + k];
  if constexpr (HALF) half_reduce<K>(v, red + (lane >> 5) * K, lane);
  else wave_reduce<K>(v, red, lane);
}

// out [3][64]: wave_allreduce1, lanes_min<64> and lanes_min<32> as each of the 64 lanes holds them
__global__ void __launch_bounds__(64) k_allreduce(const double* in, double* out) {
  const int lane = threadIdx.x;
  const double v = in[lane];
  out[lane] = wave_allreduce1(v);
  out[64 + lane] = lanes_min<64>(v);
  out[128 + lane] = lanes_min<32>(v);
}

// ---- dual_uniform on the device ---------------------------------------------------------------
__global__ void k_dual(const unsigned long long* seed, const long long* traj, const int* j, const int* k, double* out,
                       int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = dual_uniform(seed[i], traj[i], j[i], k[i]);
}

template <int K, bool HALF>
int run_reduce(const double* in, double* red) {
  Bufs b;
  const double* din = b.in(in, 64 * (size_t)K);
  constexpr size_t NO = HALF ? 2 * K : K;
  double* dred = b.out<double>(NO);
  if (b.err == hipSuccess) b.err = hipMemset(dred, 0xff, NO * sizeof(double));   // NaN: unwritten slots show
  if (b.err == hipSuccess) hipLaunchKernelGGL((k_reduce<K, HALF>), dim3(1), dim3(64), 0, 0, din, dred);
  b.ran();
  b.back(red, dred, NO);
  return (int)b.err;
}

}  // namespace

extern "C" {

int probe_exp(const double* x, double* f, double* e, int n) {
  Bufs b;
  const double* dx = b.in(x, n);
  double* df = b.out<double>(n);
  double* de = b.out<double>(n);
  if (b.err == hipSuccess && n > 0) hipLaunchKernelGGL(k_exp, dim3(blocks(n)), dim3(TPB), 0, 0, dx, df, de, n);
  b.ran();
  b.back(f, df, n);
  b.back(e, de, n);
  return (int)b.err;
}

int probe_roots(const double* s, double* out, int n) {
  Bufs b;
  const double* ds = b.in(s, n);
  double* dout = b.out<double>(5 * (size_t)n);
  if (b.err == hipSuccess && n > 0) hipLaunchKernelGGL(k_roots, dim3(blocks(n)), dim3(TPB), 0, 0, ds, dout, n);
  b.ran();
  b.back(out, dout, 5 * (size_t)n);
  return (int)b.err;
}

int probe_phi(const double* z, double* out, int n) {
  Bufs b;
  const double* dz = b.in(z, n);
  double* dout = b.out<double>(2 * (size_t)n);
  if (b.err == hipSuccess && n > 0) hipLaunchKernelGGL(k_phi, dim3(blocks(n)), dim3(TPB), 0, 0, dz, dout, n);
  b.ran();
  b.back(out, dout, 2 * (size_t)n);
  return (int)b.err;
}

int probe_rule(int rule, const double* mu, const double* sig, const double* isig, double theta, double fmin,
               double sigma_tol, double* out, int n) {
  Bufs b;
  const double* dmu = b.in(mu, n);
  const double* dsig = b.in(sig, n);
  const double* disig = b.in(isig, n);
  double* dout = b.out<double>(14 * (size_t)n);
  if (b.err == hipSuccess && n > 0)
    hipLaunchKernelGGL(k_rule, dim3(blocks(n)), dim3(TPB), 0, 0, rule, dmu, dsig, disig, theta, fmin, sigma_tol, dout,
                       n);
  b.ran();
  b.back(out, dout, 14 * (size_t)n);
  return (int)b.err;
}

int probe_rad(int kind, double cK, double cP, const double* rho2, double* out, int n) {
  Bufs b;
  const double* dr = b.in(rho2, n);
  double* dout = b.out<double>(9 * (size_t)n);
  if (b.err == hipSuccess && n > 0)
    hipLaunchKernelGGL(k_rad, dim3(blocks(n)), dim3(TPB), 0, 0, kind, cK, cP, dr, dout, n);
  b.ran();
  b.back(out, dout, 9 * (size_t)n);
  return (int)b.err;
}

// D = 2 or 8 (else -1); tab = [lb (D), del (D), w (D)]
int probe_cost(int D, int cost, double c0, const double* tab, const double* x, double* c, double* gc, double* H,
               int n) {
  if (D != 2 && D != 8) return -1;
  Bufs b;
  const double* dtab = b.in(tab, 3 * (size_t)D);
  const double* dx = b.in(x, (size_t)n * D);
  double* dc = b.out<double>(n);
  double* dg = b.out<double>((size_t)n * D);
  double* dH = b.out<double>((size_t)n * D * D);
  if (b.err == hipSuccess && n > 0) {
    if (D == 2) hipLaunchKernelGGL(k_cost<2>, dim3(blocks(n)), dim3(TPB), 0, 0, cost, c0, dtab, dx, dc, dg, dH, n);
    else hipLaunchKernelGGL(k_cost<8>, dim3(blocks(n)), dim3(TPB), 0, 0, cost, c0, dtab, dx, dc, dg, dH, n);
  }
  b.ran();
  b.back(c, dc, n);
  b.back(gc, dg, (size_t)n * D);
  b.back(H, dH, (size_t)n * D * D);
  return (int)b.err;
}

// in [64][K]; red [K] (half = 0: wave_reduce<K>, K ≤ 32) or [2][K] (half = 1: half_reduce<K>, K ≤ 16)
int probe_reduce(int K, int half, const double* in, double* red) {
  if (!half) {
    switch (K) {
      case 1: return run_reduce<1, false>(in, red);
      case 2: return run_reduce<2, false>(in, red);
      case 4: return run_reduce<4, false>(in, red);
      case 8: return run_reduce<8, false>(in, red);
      case 16: return run_reduce<16, false>(in, red);
      case 32: return run_reduce<32, false>(in, red);
    }
  } else {
    switch (K) {
      case 1: return run_reduce<1, true>(in, red);
      case 2: return run_reduce<2, true>(in, red);
      case 4: return run_reduce<4, true>(in, red);
      case 8: return run_reduce<8, true>(in, red);
      case 16: return run_reduce<16, true>(in, red);
    }
  }
  return -1;
}

// in [64]; out [3][64] = wave_allreduce1, lanes_min<64>, lanes_min<32> as every lane holds them
int probe_allreduce(const double* in, double* out) {
  Bufs b;
  const double* din = b.in(in, 64);
  double* dout = b.out<double>(3 * 64);
  if (b.err == hipSuccess) hipLaunchKernelGGL(k_allreduce, dim3(1), dim3(64), 0, 0, din, dout);
  b.ran();
  b.back(out, dout, 3 * 64);
  return (int)b.err;
}

// dev = dual_uniform on the device, host = the same header function compiled for the host
int probe_dual(const unsigned long long* seed, const long long* traj, const int* j, const int* k, double* dev,
               double* host, int n) {
  for (int i = 0; i < n; ++i) host[i] = dual_uniform(seed[i], traj[i], j[i], k[i]);
  Bufs b;
  const unsigned long long* ds = b.in(seed, n);
  const long long* dt = b.in(traj, n);
  const int* dj = b.in(j, n);
  const int* dk = b.in(k, n);
  double* dout = b.out<double>(n);
  if (b.err == hipSuccess && n > 0) hipLaunchKernelGGL(k_dual, dim3(blocks(n)), dim3(TPB), 0, 0, ds, dt, dj, dk, dout, n);
  b.ran();
  b.back(dev, dout, n);
  return (int)b.err;
}

}  // extern "C"
