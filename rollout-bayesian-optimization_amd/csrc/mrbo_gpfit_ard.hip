// mrbo_gpfit_ard.hip -- the base-GP fit with one lengthscale per input dimension (ARD) and its
// marginal likelihood with the d-component gradient, for a batch of candidates (no reference
// counterpart).
//
// θ = (ℓ_1 … ℓ_d).  All four radial kernels see x only through ρ = ‖(x − x′)/ℓ‖, so the ARD GP is the
// unit-lengthscale isotropic GP on z = x/ℓ (componentwise):
//   K_ik = ψ(ρ_ik; ℓ = 1) + σn2·δ_ik,   ρ_ik = ‖z_i − z_k‖
//   ∂K_ik/∂ℓ_u = g(ρ_ik)·(z_iu − z_ku)²/ℓ_u,   g(ρ) = −ψ′(ρ; 1)/ρ      (0 on the diagonal and where ρ = 0)
//   g: Matérn-5/2 (5/3)(1+s)e⁻ˢ, s = √5ρ;  Matérn-3/2 3e⁻ˢ, s = √3ρ;  Matérn-1/2 e⁻ᵖ/ρ;  SE e^(−ρ²/2)
// The likelihoods are mrbo_gpfit.hip's: plain (log_likelihood, δlog_likelihood with δK_u above) and
// profiled (GpFitMode, mrbo_gpfit.h).  Periodic has no such form and is refused by the host API.
//
// One workgroup per (candidate p, data set q) of a (P, S) grid, addressed as gpfit_candidate()
// addresses them (mrbo_gpfit.hip): GpFitParams with nt = d and thetas d×P×S.  The layout is
// gpfit_lds_kernel's: z, K → L, V = L⁻¹ and c in LDS (N ≤ 128, d ≤ 16: 151 KB of the CU's 160 KiB),
// the same Cholesky, inverse and substitutions; the epilogue runs over the pairs j < i with
// K⁻¹_ij = Σ_{m≥i} V_mi V_mj and g(ρ_ij) formed once per pair and d accumulators per thread for
// tr(K⁻¹δK_u) and for cᵀδK_u c, reduced in a fixed order (wave butterflies, then the four waves'
// partial sums added by one thread): no floating-point atomics, so a slot's outputs depend on
// nothing but its own inputs.
//
// status per slot (NaN ll / grad / s2 on any non-zero one): 0 ok, 1 a pivot is not positive,
// 2 profile mode and yᵀc is not positive and finite, 3 some ℓ_u is not positive and finite (checked
// before K is built).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "mrbo_gpfit.h"

namespace mrbo {

namespace {

constexpr int GA_N = 128, GA_LD = 129, GA_THREADS = 256, GA_D = 16, GA_WAVES = GA_THREADS / 64;

__device__ __forceinline__ double ga_sum(double v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ψ(ρ; ℓ = 1) and g(ρ) = −ψ′(ρ; 1)/ρ from r2 = ρ² (r2 > 0 where g is used)
template <int KIND>
__device__ __forceinline__ double ga_psi(double r2) {
  constexpr double third = 1.0 / 3.0;
  if constexpr (KIND == 3) {
    return exp(-0.5 * r2);
  } else {
    const double c = (KIND == 0) ? sqrt(5.0) : (KIND == 1) ? sqrt(3.0) : 1.0;
    const double s = c * sqrt(r2), e = exp(-s);
    if constexpr (KIND == 0) return (1.0 + s * (1.0 + s * third)) * e;
    else if constexpr (KIND == 1) return (1.0 + s) * e;
    else return e;
  }
}
template <int KIND>
__device__ __forceinline__ double ga_g(double r2) {
  if constexpr (KIND == 3) {
    return exp(-0.5 * r2);
  } else {
    const double rho = sqrt(r2);
    if constexpr (KIND == 0) {
      const double s = sqrt(5.0) * rho;
      return (5.0 / 3.0) * (1.0 + s) * exp(-s);
    } else if constexpr (KIND == 1) {
      return 3.0 * exp(-sqrt(3.0) * rho);
    } else {
      return exp(-rho) / rho;
    }
  }
}

__device__ __forceinline__ void ga_fail(const GpFitParams& q, double* s2_out, int p, int status) {
  q.ll[p] = NAN;
  for (int u = 0; u < q.d; ++u) q.grad[(size_t)p * q.d + u] = NAN;
  if (s2_out) s2_out[p] = NAN;
  q.status[p] = status;
}

template <bool PROFILE>
__device__ __forceinline__ void gpfit_ard_body(const GpFitParams& q, int P, double* s2_out) {
  extern __shared__ __attribute__((aligned(16))) double gsm[];
  double* S = gsm;                      // GA_N × GA_LD: K → L below, Vᵀ above the diagonal
  double* ZS = S + GA_N * GA_LD;        // z[u][i] at u·GA_N + i (u < d ≤ 16)
  double* ld_ = ZS + GA_D * GA_N;       // L_ii
  double* dv = ld_ + GA_N;              // 1/L_ii
  double* cv = dv + GA_N;               // y, then c
  __shared__ double part[GA_WAVES][2 * GA_D + 2];
  __shared__ double il[GA_D];           // 1/ℓ_u
  __shared__ int fail;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if ((int)blockIdx.x >= P) return;   // whole workgroups
  const int p = blockIdx.x + blockIdx.y * P;   // gpfit_candidate (mrbo_gpfit.hip)
  const int N = q.N, d = q.d;
  const size_t xo = (size_t)blockIdx.y * d * N, yo = (size_t)blockIdx.y * N;   // this data set's X and y
  const double* ells = q.thetas + (size_t)p * d;
  {
    bool bad = false;   // every thread reads the same d values: a uniform exit
    for (int u = 0; u < d; ++u) {
      const double l = ells[u];
      bad = bad || !(l > 0.0) || !(l <= 1.79769313486231570815e308);
    }
    if (bad) {
      if (tid == 0) ga_fail(q, PROFILE ? s2_out : nullptr, p, 3);
      return;
    }
  }
  if (tid == 0) fail = 0;
  if (tid < d) il[tid] = 1.0 / ells[tid];
  for (int idx = tid; idx < d * N; idx += GA_THREADS) {
    const int u = idx % d, i = idx / d;
    ZS[u * GA_N + i] = q.X[xo + idx] / ells[u];
  }
  for (int i = tid; i < N; i += GA_THREADS) cv[i] = q.y[yo + i];
  __syncthreads();
  // K over the pairs j ≤ i, lower triangle (ψ(0) = 1 on the diagonal, + σn2)
  const int npair = N * (N + 1) / 2;
  auto kpairs = [&](auto kind_c) {
    constexpr int KIND = decltype(kind_c)::value;
    for (int qq = tid; qq < npair; qq += GA_THREADS) {
      int i = (int)((sqrt(8.0 * qq + 1.0) - 1.0) * 0.5);
      i += ((i + 1) * (i + 2) / 2 <= qq) ? 1 : 0;   // exact row of the triangle index
      i -= (i * (i + 1) / 2 > qq) ? 1 : 0;
      const int j = qq - i * (i + 1) / 2;
      double r2 = 0.0;
      for (int u = 0; u < d; ++u) { const double r = ZS[u * GA_N + i] - ZS[u * GA_N + j]; r2 = fma(r, r, r2); }
      S[i + GA_LD * j] = (i == j) ? 1.0 + q.sn2 : ga_psi<KIND>(r2);
    }
  };
  switch (q.kernel) {
    case 0: kpairs(std::integral_constant<int, 0>{}); break;
    case 1: kpairs(std::integral_constant<int, 1>{}); break;
    case 2: kpairs(std::integral_constant<int, 2>{}); break;
    default: kpairs(std::integral_constant<int, 3>{}); break;
  }
  __syncthreads();
  // right-looking Cholesky, one barrier per column (gpfit_lds_body's: thread (row i, parity)
  // updates S[i][j] for j ≡ parity; column k is scaled by the readers, stored one step later)
  {
    const int i = tid & (GA_N - 1), par = tid >> 7;
    double lprev = 0.0;
    for (int k = 0; k < N; ++k) {
      const double piv = S[k + GA_LD * k];
      if (!(piv > 0.0)) {   // every thread reads the same pivot: a uniform exit
        if (tid == 0) fail = 1;
        break;
      }
      double lkk, rl;
      sqrt_rsqrt(piv, lkk, rl);
      if (tid == 0) { ld_[k] = lkk; dv[k] = rl; }
      if (k > 0 && par == 0 && i > k - 1 && i < N) S[i + GA_LD * (k - 1)] = lprev;   // scaled L_i,k-1
      if (i > k && i < N) {
        const double lik = S[i + GA_LD * k] * rl;
        lprev = lik;
        for (int jb = k + 1 + par; jb <= i; jb += 16) {
          double lv[8], av[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int j = min(jb + 2 * u, i);
            lv[u] = S[j + GA_LD * k];
            av[u] = S[i + GA_LD * j];
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) av[u] = fma(-lik, lv[u] * rl, av[u]);
#pragma unroll
          for (int u = 0; u < 8; ++u)
            if (jb + 2 * u <= i) S[i + GA_LD * (jb + 2 * u)] = av[u];
        }
      }
      __syncthreads();
    }
  }
  __syncthreads();
  if (fail) {
    if (tid == 0) ga_fail(q, PROFILE ? s2_out : nullptr, p, 1);
    return;
  }
  if (w < 2) {
    // V = L⁻¹, column j = tid: V_jj = 1/L_jj, V_ij = −(Σ_{k=j}^{i−1} L_ik V_kj)/L_ii, rows ascending
    const int j = tid;
    const double djj = dv[j];
    for (int i = 64 * w + 1; i < N; ++i) {
      if (i <= j) continue;
      double sc[4] = {S[i + GA_LD * j] * djj, 0.0, 0.0, 0.0};
      int k = j + 1;
      for (; k + 8 <= i; k += 8) {
        double lv[8], vv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          lv[u] = S[i + GA_LD * (k + u)];
          vv[u] = S[j + GA_LD * (k + u)];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) sc[u & 3] = fma(lv[u], vv[u], sc[u & 3]);
      }
      for (; k < i; ++k) sc[0] = fma(S[i + GA_LD * k], S[j + GA_LD * k], sc[0]);
      S[j + GA_LD * i] = -((sc[0] + sc[1]) + (sc[2] + sc[3])) * dv[i];
    }
  } else if (w == 2) {
    // c = L'\(L\y): column-oriented substitutions, rows lane and lane + 64 in registers, the
    // solved entry broadcast by readlane
    double r[2];
    r[0] = (lane < N) ? cv[lane] : 0.0;
    r[1] = (lane + 64 < N) ? cv[lane + 64] : 0.0;
    for (int k = 0; k < N; ++k) {
      const double zk = readlane_d(r[k >> 6], k & 63) * dv[k];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int i = lane + 64 * h;
        if (i == k) r[h] = zk;
        else if (i > k && i < N) r[h] = fma(-S[i + GA_LD * k], zk, r[h]);
      }
    }
    for (int k = N - 1; k >= 0; --k) {
      const double ck = readlane_d(r[k >> 6], k & 63) * dv[k];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int i = lane + 64 * h;
        if (i == k) r[h] = ck;
        else if (i < k) r[h] = fma(-S[k + GA_LD * i], ck, r[h]);
      }
    }
    double yc = 0.0, lg = 0.0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int i = lane + 64 * h;
      if (i < N) {
        yc = fma(q.y[yo + i], r[h], yc);
        lg += log(ld_[i]);
      }
    }
    if (lane < N) cv[lane] = r[0];
    if (lane + 64 < N) cv[lane + 64] = r[1];
    yc = ga_sum(yc);
    lg = ga_sum(lg);
    if (lane == 0) { part[0][2 * GA_D] = yc; part[0][2 * GA_D + 1] = lg; }
  }
  __syncthreads();
  // the pairs j < i: wave w takes rows i ≡ w (mod 4), lanes over j in chunks of 64.  Per pair
  // K⁻¹_ij and g(ρ_ij) once, then tr_u += K⁻¹_ij·g·Δz_u², cgc_u += c_i c_j·g·Δz_u² (δK_u without its
  // 1/ℓ_u, applied to the sums)
  double tr[GA_D], cgc[GA_D];
#pragma unroll
  for (int u = 0; u < GA_D; ++u) tr[u] = cgc[u] = 0.0;
  auto traces = [&](auto kind_c) {
    constexpr int KIND = decltype(kind_c)::value;
    for (int i = 1 + w; i < N; i += GA_WAVES) {
      const double ci = cv[i];
      for (int jb = 0; jb < i; jb += 64) {
        const int j = jb + lane;
        if (j >= i) break;
        // K⁻¹_ij = V_ii V_ij + Σ_{m > i} V_mi V_mj
        double kc[4] = {dv[i] * S[j + GA_LD * i], 0.0, 0.0, 0.0};
        for (int mb = i + 1; mb < N; mb += 8) {
          double av[8], bv[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int m = min(mb + u, N - 1);
            const double x = S[i + GA_LD * m];
            bv[u] = S[j + GA_LD * m];
            av[u] = (mb + u < N) ? x : 0.0;
          }
#pragma unroll
          for (int u = 0; u < 8; ++u) kc[u & 3] = fma(av[u], bv[u], kc[u & 3]);
        }
        const double kij = (kc[0] + kc[1]) + (kc[2] + kc[3]);
        double dz2[GA_D], r2 = 0.0;
#pragma unroll
        for (int u = 0; u < GA_D; ++u) {
          dz2[u] = 0.0;
          if (u < d) {
            const double r = ZS[u * GA_N + i] - ZS[u * GA_N + j];
            dz2[u] = r * r;
            r2 += dz2[u];
          }
        }
        const double g = (r2 > 0.0) ? ga_g<KIND>(r2) : 0.0;   // coincident points: δK = 0
        const double kg = kij * g, cg = ci * cv[j] * g;
#pragma unroll
        for (int u = 0; u < GA_D; ++u)
          if (u < d) {
            tr[u] = fma(kg, dz2[u], tr[u]);
            cgc[u] = fma(cg, dz2[u], cgc[u]);
          }
      }
    }
  };
  switch (q.kernel) {
    case 0: traces(std::integral_constant<int, 0>{}); break;
    case 1: traces(std::integral_constant<int, 1>{}); break;
    case 2: traces(std::integral_constant<int, 2>{}); break;
    default: traces(std::integral_constant<int, 3>{}); break;
  }
#pragma unroll
  for (int u = 0; u < GA_D; ++u)
    if (u < d) {
      const double trs = ga_sum(tr[u]), cgs = ga_sum(cgc[u]);
      if (lane == 0) { part[w][u] = trs; part[w][GA_D + u] = cgs; }
    }
  __syncthreads();
  // Σ_{j<i} is half of the full sums: tr(K⁻¹δK_u)/2 and cᵀδK_u c/2 once scaled by 1/ℓ_u
  const double yc = part[0][2 * GA_D], lg = part[0][2 * GA_D + 1];
  bool ok = true;
  if (PROFILE) ok = (yc > 0.0) && (yc <= 1.79769313486231570815e308);   // uniform: every thread reads part
  if (tid == 0) {
    if (!ok) {
      ga_fail(q, s2_out, p, 2);
    } else {
      const double s2 = yc / N;
      for (int u = 0; u < d; ++u) {
        const double trs = ((part[0][u] + part[1][u]) + (part[2][u] + part[3][u])) * il[u];
        const double cgs = ((part[0][GA_D + u] + part[1][GA_D + u]) + (part[2][GA_D + u] + part[3][GA_D + u])) * il[u];
        q.grad[(size_t)p * d + u] = PROFILE ? cgs / s2 - trs : cgs - trs;
      }
      if (PROFILE) {
        q.ll[p] = -0.5 * N * log(s2) - lg - 0.5 * N * (1.0 + log(2.0 * 3.141592653589793));
        s2_out[p] = s2;
      } else {
        q.ll[p] = -0.5 * yc - lg - 0.5 * N * log(2.0 * 3.141592653589793);
      }
      q.status[p] = 0;
    }
  }
  if (q.L_out) {
    double* Lo = q.L_out + (size_t)N * N * p;
    for (int idx = tid; idx < N * N; idx += GA_THREADS) {
      const int i = idx % N, j = idx / N;
      Lo[idx] = (i > j) ? S[i + GA_LD * j] : ((i == j) ? ld_[i] : 0.0);
    }
  }
  if (q.c_out)
    for (int i = tid; i < N; i += GA_THREADS) q.c_out[(size_t)N * p + i] = cv[i];
}

__global__ void __launch_bounds__(GA_THREADS) gpfit_ard_kernel(GpFitParams q, int P) {
  gpfit_ard_body<false>(q, P, nullptr);
}
__global__ void __launch_bounds__(GA_THREADS) gpfit_ard_profile_kernel(GpFitParams q, int P, double* s2) {
  gpfit_ard_body<true>(q, P, s2);
}

size_t gpfit_ard_dyn_lds() { return sizeof(double) * ((size_t)GA_N * GA_LD + GA_D * GA_N + 3 * GA_N); }

}  // namespace

size_t gpfit_ard_lds() {
  size_t dyn = gpfit_ard_dyn_lds();
  hipFuncAttributes fa{};
  if (hipFuncGetAttributes(&fa, (const void*)gpfit_ard_profile_kernel) == hipSuccess) dyn += fa.sharedSizeBytes;
  else dyn += 4096;   // attributes unavailable: keep a margin for the static arrays
  return dyn;
}

void launch_gpfit_ard(int P, int S, hipStream_t st, const GpFitParams& q, const GpFitMode& pm) {
  if (pm.profile)
    hipLaunchKernelGGL(gpfit_ard_profile_kernel, dim3(P, S), dim3(GA_THREADS), gpfit_ard_dyn_lds(), st, q, P, pm.s2);
  else
    hipLaunchKernelGGL(gpfit_ard_kernel, dim3(P, S), dim3(GA_THREADS), gpfit_ard_dyn_lds(), st, q, P);
}

}  // namespace mrbo
