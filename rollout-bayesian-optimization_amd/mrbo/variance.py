"""The EI control variate of the rollout estimate -- the NumPy specification.

The reference's drivers advertise --variance-reduction, "Use EI as a control variate for variance
reduction" (experiments/nonmyopic_bayesopt.jl:64-66), and hand it to a solver that is defined
nowhere, so the estimator is build-defined.  A trajectory's value is v = max(fmini − min_k y_k, 0).
Its step-0 part c = max(fmini − y_0, 0), y_0 = μ(x0) + σ(x0)·z_0, is the value of the SAME trajectory
cut at horizon 0, and its expectation is known in closed form: with u = (fmini − μ)/σ

    E[c]  = EI0(x0)  = σ·(u·Φ(u) + φ(u))
    E[∇c] = ∇EI0(x0) = φ(u)·∇σ − Φ(u)·∇μ

(the pathwise gradient of c is −∇y_0·1[y_0 < fmini]; column 0 of the draw's Cholesky factor below the
diagonal is ∇σ and the other columns carry zero-mean noise, so the second line is exact).  Per restart
and per series a -- the value, or one component of ∇x -- with target samples a_m, control samples b_m
and the control's expectation e:

    ā = Σa/M,  b̄ = Σb/M,  da = a − ā,  db = b − b̄,  Sbb = Σdb²,  Sab = Σda·db
    β = Sab/Sbb  if Sbb > 0 and both sums are finite, else 0
    β ≠ 0:  mean = ā − β·(b̄ − e),   std = sqrt(Σ(da − β·db)²/(M − 1))
    β = 0:  mean = ā,               std = sqrt(Σda²/(M − 1))       (the plain row; e is not read)

The ∇θ columns are always the plain ones: the control does not depend on T.θ.  The device's
mrbo_eto_reduce_cv (csrc/mrbo_cv.hip) is held to cv_rows on its own inputs (tests/
test_gpu_control_variate.py); everything here is plain fp64 NumPy and runs without a GPU.
"""
import math

import numpy as np

_erfc = np.vectorize(math.erfc, otypes=[np.float64])
SQRT2 = math.sqrt(2.0)
INV_SQRT_2PI = 0.3989422804014327


def phi_Phi(u):
    """φ(u) = exp(−u²/2)/√(2π) and Φ(u) = ½·erfc(−u/√2) (libm)."""
    u = np.asarray(u, dtype=np.float64)
    return np.exp(-0.5 * (u * u)) * INV_SQRT_2PI, 0.5 * _erfc(-u / SQRT2)


def ei0(mu, sigma, gmu, gsig, fmini):
    """EI0 and ∇EI0 at P points: mu, sigma (P), gmu, gsig (d×P), fmini a scalar or (P).  Returns
    (EI0 (P), ∇EI0 (d×P)).  No σtol branch: the control's expectation is the closed form itself."""
    mu, sigma = np.asarray(mu, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    gmu, gsig = np.asarray(gmu, dtype=np.float64), np.asarray(gsig, dtype=np.float64)
    with np.errstate(all="ignore"):
        u = (fmini - mu) / sigma
        phi, Phi = phi_Phi(u)
        return sigma * (u * Phi + phi), phi * gsig - Phi * gmu


def _series(a, b, e):
    """One series: a, b are M×K (K restarts), e (K).  Returns (mean, std, beta), each (K)."""
    M = a.shape[0]
    with np.errstate(all="ignore"):
        abar, bbar = a.sum(axis=0) / M, b.sum(axis=0) / M
        da, db = a - abar, b - bbar
        Saa, Sbb, Sab = (da * da).sum(axis=0), (db * db).sum(axis=0), (da * db).sum(axis=0)
        ok = (Sbb > 0.0) & np.isfinite(Sbb) & np.isfinite(Sab)
        beta = np.where(ok, Sab / np.where(ok, Sbb, 1.0), 0.0)
        use = beta != 0.0
        bsel = np.where(use, beta, 0.0)
        res = np.where(use, da - bsel * np.where(use, db, 0.0), da)
        # selects, not multiplications by zero: a NaN control or expectation never reaches a plain row
        mean = np.where(use, abar - bsel * np.where(use, bbar - e, 0.0), abar)
        std = np.sqrt(np.where(use, (res * res).sum(axis=0), Saa) / (M - 1))
    return mean, std, np.where(use, beta, 0.0)


def cv_rows(values, grad_x, grad_theta, values0, grad_x0, ei, gei):
    """The ETO rows of K restarts with the control variate.

    values, values0   M×K      target and control values
    grad_x, grad_x0   d×M×K    target and control gradients (grad_x None: value columns only, the
                               gradient columns zero as mrbo_eto_reduce writes them and β_a = 0)
    grad_theta        M×K or None (always the plain columns)
    ei (K), gei (d×K)          EI0 and ∇EI0 at the K start points (ei0())

    Returns (eto, beta): eto K×W in mrbo_eto_reduce's layout [μ, σ_μ, ∇μx (d), σ_∇μx (d), ∇μθ, σ_∇μθ],
    beta (1+d)×K."""
    values, values0 = np.asarray(values, dtype=np.float64), np.asarray(values0, dtype=np.float64)
    M, K = values.shape
    gei = np.asarray(gei, dtype=np.float64)
    d = gei.shape[0]
    eto = np.zeros((K, 2 + 2 * d + 2))
    beta = np.zeros((1 + d, K))
    eto[:, 0], eto[:, 1], beta[0] = _series(values, values0, np.asarray(ei, dtype=np.float64))
    if grad_x is not None:
        grad_x, grad_x0 = np.asarray(grad_x, dtype=np.float64), np.asarray(grad_x0, dtype=np.float64)
        for a in range(d):
            eto[:, 2 + a], eto[:, 2 + d + a], beta[1 + a] = _series(grad_x[a], grad_x0[a], gei[a])
    if grad_theta is not None:
        gt = np.asarray(grad_theta, dtype=np.float64).reshape(M, K)
        nan = np.full((M, K), np.nan)
        eto[:, 2 + 2 * d], eto[:, 3 + 2 * d], _ = _series(gt, nan, np.full(K, np.nan))
    return eto, beta


def plain_rows(values, grad_x, grad_theta, d):
    """The rows without a control (β = 0 everywhere): the centred two-pass mean / std(n−1) that
    mrbo_eto_reduce computes (its summation order aside) -- cv_rows with a NaN control."""
    values = np.asarray(values, dtype=np.float64)
    M, K = values.shape
    return cv_rows(values, grad_x, grad_theta, np.full((M, K), np.nan), np.full((d, M, K), np.nan),
                   np.full(K, np.nan), np.full((d, K), np.nan))[0]
