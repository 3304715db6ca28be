"""The numeric building blocks of csrc/mrbo_device.h, each on its own, against mpmath.

The GPU tests run the primitives through the probe library (tests/device_probe.py) and compare
with mpmath at 40 digits, evaluated at exactly the fp64 inputs the device receives.  An ulp is an
ulp of the (fp64-rounded) reference value.

How the limits are fixed.  The project's own claims are asserted as the header states them: fexp
bit-equal to exp(), the roots within 2 ulp, exact branch values.  Every other limit is a constant
C_* below = 4 × the maximum normalised error that the SAME closed form has in plain host fp64
(NumPy / libm exp and erfc: the oracle's arithmetic, not the code under test) on the SAME inputs,
rounded up to an integer.  The factor 4 covers what the device does in addition: a fitted erfcx,
reciprocals by v_rcp + Newton steps, Estrin instead of Horner order, FMA contraction.  The CPU test
test_host_maxima_within_a_quarter_of_the_limits re-measures the host maxima, so a libm that differs
shows up there and not on the GPU.

Error models (err = |device − reference| in ulps of the reference):
  φ(z), Φ(z ≤ 0)        err ≤ C + z²/2         the exponent −z²/2 carries the relative rounding of z²
  Φ(z > 0)              |Φ − ref| ≤ 2⁻⁵²       one ulp of 1
  φ + zΦ, z ≤ 0         err ≤ C·(1 + z²)       the two terms cancel to a 1/z² fraction of either
  rule_partials         err ≤ C·(1 + z²) for outputs that hold Φ or the EI sum, C·(1 + z²/2) for the
                        pure-φ ones; POI's ∂²/∂σ² and ∂²/∂σ∂θ carry the polynomial factors 2 − z² and
                        1 − z², whose zeros make a relative error unbounded: their limit is multiplied
                        by the factor's condition number (2 + z²)/|2 − z²| resp. (1 + z²)/|1 − z²|.
                        The inputs have fmin = 0, so that I = fmin − μ − θ is ONE rounded operation:
                        with fmin ≠ 0 and μ near fmin the difference cancels, z = I/σ inherits an
                        absolute error ulp(μ)/σ that no ulp model of the OUTPUT covers, and the host
                        forms lose exactly as much.
  rad_eval, Matérn/SE   err ≤ C·(1 + s), s the exponent (c·ρ, resp. c·ρ²/2); where exp(−s) is
                        subnormal its absolute error 2⁻¹⁰⁷⁴ times the factor in front of it is allowed
  rad_eval, Periodic    absolute errors over the scales ψ, ψ·A·B (g1) and ψ·B²·A·(A + B) (g2), in units
                        of 2⁻⁵³·(1 + s + c·t): s = 2c·sin²(t/2) is the exponent, and t = B·ρ carries a
                        relative rounding that the exponent's derivative c·sin t turns into c·t·2⁻⁵³
  cost model            err ≤ C·(1 + |t|), t the log-linear exponent (0 for the quadratic model)
"""
import functools
import math

import numpy as np
import pytest

import conftest  # noqa: F401  (sys.path)
import device_probe

import mpmath as mp  # noqa: E402

mp.mp.dps = 40
mpf = mp.mpf

gpu_test = pytest.mark.gpu

# ---- the limits: 4 × the host maximum (beside each), rounded up ------------------------------------
C_PHI = 6                # φ, ulp beyond z²/2:                     host 1.335
C_PHI_CDF = 12           # Φ on z ≤ 0, (1 + z²/2)-ulp:             host 2.976
C_EI_TAIL = 7335         # φ + zΦ on [−36, 0], (1 + z²)-ulp:       host 1833.6 (ill-conditioned, see below)
C_RULE_CDF = 4492        # rule outputs with Φ or the EI sum:      host 1122.8 (ill-conditioned, see below)
C_RULE_PDF = 14          # pure-φ rule outputs:                    host 3.445
C_RAD = (10, 8, 10)      # Matérn and SE ψ, g1, g2:                host 2.418, 1.885, 2.291
C_PER = (7, 14, 355)     # Periodic ψ, g1, g2:                     host 1.509, 3.479, 88.56 (see below)
C_COST = 9               # c, ∇c, Hc:                              host 2.0015
# Two host forms are ill-conditioned, and their limits are as wide as the rule makes them:
#  * φ + zΦ with Φ = ½·erfc(−z/√2): the rounding of the argument −z/√2 reaches Φ multiplied by z², that
#    of z² reaches φ multiplied by z²/2, and the sum keeps a 1/z² fraction of either term -- z² ulp in
#    the (1 + z²) unit, 1.8e3 at z = −36.  The device forms both terms from ONE exponential, so that
#    the rounding of z² is a common factor.  That property gets limits of its own, by the same rule
#    from a host pair of the device's structure (_host_mills: one libm exponential, scipy's erfcx):
C_MILLS = 26             # Φ/φ on z ≤ 0, ulp:                      host 6.486
C_EI_TAIL_SHARED = 35    # φ + zΦ on [−36, 0], (1 + z²)-ulp:       host 8.570
C_RULE_EI_SHARED = 25    # EI's g and ∂g/∂μ, (1 + z²)-ulp:         host 6.043
#  * Periodic g2 holds (sin t − t cos t)/t³, whose closed form keeps a t²/3 fraction of its terms just
#    above the series switch at t = 0.1 (the device uses the same closed form there).

TINY = 2.0 ** -1074
DBL_MIN = 2.2250738585072014e-308
SQRT2 = math.sqrt(2.0)


def _f(xs):
    return np.array([float(v) for v in xs], dtype=np.float64)


def _ulp(ref):
    """spacing of the fp64-rounded reference (2⁻¹⁰⁷⁴ at zero and for subnormals)"""
    with np.errstate(all="ignore"):
        return np.maximum(np.spacing(np.abs(_f(ref))), TINY)


def _abs_err(val, ref):
    """|val − ref| with the difference taken in mpmath"""
    return np.array([float(abs(mpf(float(v)) - r)) for v, r in zip(val, ref)], dtype=np.float64)


def _err_ulps(val, ref):
    """|val − ref| / ulp(ref), the quotient taken in mpmath too (an error of a fraction of 2⁻¹⁰⁷⁴
    would round to a whole number of subnormal steps as an fp64 difference)"""
    return np.array([float(abs(mpf(float(v)) - r) / mpf(float(u))) for v, r, u in zip(val, ref, _ulp(ref))],
                    dtype=np.float64)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    """bit-equal, any NaN matching any NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def _report(name, worst, limit=None):
    print(f"[primitives] {name}: max {worst:.3g}" + (f" (limit {limit})" if limit is not None else ""))


@pytest.fixture(scope="module")
def probe(gpu):
    return device_probe.Probe()


# =====================================================================================================
# exponential
# =====================================================================================================
@functools.lru_cache(None)
def _exp_inputs():
    rng = np.random.default_rng(11)
    nx = np.nextafter
    special = [0.0, -0.0, 1e-300, -1e-300, 5e-324, -5e-324, 1e-310, -1e-310,
               709.78, nx(709.78, np.inf), nx(709.78, -np.inf), -745.13, nx(-745.13, np.inf), nx(-745.13, -np.inf),
               709.782712893384, nx(709.782712893384, np.inf), -708.3964185322641, -745.1332191019412,
               1024.0, -1024.0, 1075.0, -1075.0, nx(1024.0, np.inf), nx(-1075.0, -np.inf), np.inf, -np.inf, np.nan]
    return np.concatenate([np.linspace(-750.0, 710.0, 1461), rng.uniform(-750.0, 710.0, 700),
                           np.linspace(-40.0, 0.0, 801), rng.uniform(-40.0, 0.0, 700), rng.uniform(-1.0, 1.0, 200),
                           special])


@gpu_test
def test_fexp_bit_equal_to_exp_and_within_one_ulp(probe):
    x = _exp_inputs()
    f, e = probe.exp(x)
    bad = ~((_bits(f) == _bits(e)) | (np.isnan(f) & np.isnan(e)))
    assert not bad.any(), f"fexp != exp at x = {x[bad][:8]}: {f[bad][:8]} vs {e[bad][:8]}"
    fin = np.isfinite(x)
    ref = [mp.exp(mpf(float(v))) for v in x[fin]]
    normal = np.array([DBL_MIN <= r < mpf(1.7976931348623157e308) for r in ref])
    err = _err_ulps(f[fin][normal], [r for r, m in zip(ref, normal) if m])
    _report("fexp vs mpmath (ulp)", err.max(), 1)
    assert err.max() <= 1.0
    assert np.isnan(f[np.isnan(x)]).all()
    assert (f[x == np.inf] == np.inf).all() and (f[x == -np.inf] == 0.0).all()
    assert (f[x >= 709.79] == np.inf).all() and (f[x <= -745.14] == 0.0).all()


# =====================================================================================================
# roots
# =====================================================================================================
LO_T, HI_T = 1e-290, 1e290


def _neighbours(t):
    a = [t]
    for d in (-np.inf, np.inf):
        v = t
        for _ in range(2):
            v = np.nextafter(v, d)
            a.append(v)
    return a


@functools.lru_cache(None)
def _root_inputs():
    rng = np.random.default_rng(12)
    grid = 10.0 ** np.concatenate([np.linspace(-289.99, 289.99, 2500), rng.uniform(-289.99, 289.99, 1000)])
    edges = np.array(_neighbours(LO_T) + _neighbours(HI_T) + _neighbours(0.0) + [-0.0, 1e-300, 1e-310, 1e-320, 1e300,
                     -1.0, -1e-300, -1e300, np.inf, np.nan, 1.0, 4.0, 2.0])
    return np.concatenate([grid, edges])


@gpu_test
def test_roots_two_ulp_and_branch_values(probe):
    s = _root_inputs()
    o = probe.roots(s)
    inside = (s > LO_T) & (s < HI_T)
    closed = (s >= LO_T) & (s <= HI_T)
    sq = [mp.sqrt(mpf(float(v))) for v in s[closed]]
    # sqrt_rsqrt on [1e-290, 1e290]: the header's 2 ulp
    e_r, e_ir = _err_ulps(o["r"][closed], sq), _err_ulps(o["ir"][closed], [1 / v for v in sq])
    _report("sqrt_rsqrt r (ulp)", e_r.max(), 2)
    _report("sqrt_rsqrt ir (ulp)", e_ir.max(), 2)
    assert e_r.max() <= 2.0 and e_ir.max() <= 2.0
    # fast_sqrt0: the same root above 1e-290, zero at and below it, NaN for NaN
    sq_in = [mp.sqrt(mpf(float(v))) for v in s[inside]]
    e0 = _err_ulps(o["sqrt0"][inside], sq_in)
    _report("fast_sqrt0 (ulp)", e0.max(), 2)
    assert e0.max() <= 2.0
    below = (s <= LO_T) & np.isfinite(s)
    assert below.sum() >= 12 and (o["sqrt0"][below] == 0.0).all()
    assert np.isnan(o["sqrt0"][np.isnan(s)]).all()
    # sig_isig: sqrt_rsqrt inside (1e-290, 1e290), the IEEE root and quotient outside
    e_s, e_is = _err_ulps(o["sig"][inside], sq_in), _err_ulps(o["isig"][inside], [1 / v for v in sq_in])
    _report("sig_isig inside (ulp)", max(e_s.max(), e_is.max()), 2)
    assert e_s.max() <= 2.0 and e_is.max() <= 2.0
    assert _same_bits(o["sig"][inside], o["r"][inside]) and _same_bits(o["isig"][inside], o["ir"][inside])
    out = ~inside
    with np.errstate(all="ignore"):
        ieee_s = np.sqrt(s[out])
        ieee_i = 1.0 / ieee_s
    assert _same_bits(o["sig"][out], ieee_s), (s[out], o["sig"][out], ieee_s)
    assert _same_bits(o["isig"][out], ieee_i), (s[out], o["isig"][out], ieee_i)
    z = _bits(s) == 0   # +0
    assert (o["sig"][z] == 0.0).all() and (o["isig"][z] == np.inf).all()
    neg = s < 0
    assert neg.sum() >= 5 and np.isnan(o["sig"][neg]).all() and np.isnan(o["isig"][neg]).all()
    assert (o["sig"][s == np.inf] == np.inf).all() and (o["isig"][s == np.inf] == 0.0).all()
    assert np.isnan(o["sig"][np.isnan(s)]).all() and np.isnan(o["isig"][np.isnan(s)]).all()


# =====================================================================================================
# normal pair
# =====================================================================================================
@functools.lru_cache(None)
def _phi_inputs():
    rng = np.random.default_rng(13)
    return np.concatenate([np.linspace(-36.0, 36.0, 2401), rng.uniform(-36.0, 36.0, 1000), rng.uniform(-3.0, 3.0, 400),
                           [0.0, -0.0]])


@functools.lru_cache(None)
def _phi_ref():
    z = _phi_inputs()
    zz = [mpf(float(v)) for v in z]
    phi = [mp.npdf(v) for v in zz]
    Phi = [mp.erfc(-v / mp.sqrt(2)) / 2 for v in zz]
    ei = [p + v * P for p, v, P in zip(phi, zz, Phi)]
    return phi, Phi, ei


def _phi_errors(z, phi, Phi):
    """normalised errors of a (φ, Φ) pair: φ beyond z²/2 (ulp), Φ for z ≤ 0 beyond z²/2, Φ for z > 0
    (absolute), the EI tail φ + zΦ on z ≤ 0 in (1 + z²) ulp"""
    rphi, rPhi, rei = _phi_ref()
    neg = z <= 0
    e_phi = _err_ulps(phi, rphi) - 0.5 * z * z
    e_Phi = _err_ulps(Phi, rPhi)
    ei = phi + z * Phi
    e_ei = _err_ulps(ei, rei) / (1.0 + z * z)
    return dict(phi=e_phi.max(), Phi_neg=(e_Phi - 0.5 * z * z)[neg].max(), mills=_mills_error(z, phi, Phi),
                Phi_neg_rel=(e_Phi / (1.0 + 0.5 * z * z))[neg].max(),
                Phi_pos=_abs_err(Phi[~neg], [r for r, m in zip(rPhi, ~neg) if m]).max(), ei=e_ei[neg].max())


def _mills_error(z, phi, Phi):
    """error of the ratio Φ/φ on z ≤ 0 in ulps, the quotient of the two values taken exactly.  The
    ratio is √(π/2)·erfcx(−z/√2): it is free of the exponential and well conditioned in z, so this is
    the accuracy of the device's fitted erfcx, and the reason why φ + zΦ keeps its relative accuracy
    where the two terms cancel (an error of the shared exponential drops out of the ratio)."""
    rphi, rPhi, _ = _phi_ref()
    neg = np.flatnonzero(z <= 0)
    got = [mpf(float(Phi[i])) / mpf(float(phi[i])) for i in neg]
    want = [rPhi[i] / rphi[i] for i in neg]
    return float(max(abs(g - w) / mpf(float(np.spacing(float(w)))) for g, w in zip(got, want)))


def _host_mills(z):
    """(φ, Φ) of a host pair with the device's structure: one exponential, scipy's erfcx"""
    from scipy.special import erfcx
    E = np.exp(-0.5 * (z * z))
    q = 0.5 * E * erfcx(np.abs(z) / SQRT2)
    return E * 0.3989422804014327, np.where(z > 0, 1.0 - q, q)


def _host_phi_Phi(z):
    phi = np.exp(-0.5 * (z * z)) * 0.3989422804014327
    Phi = np.array([0.5 * math.erfc(-v / SQRT2) for v in z])
    return phi, Phi


@gpu_test
def test_ei_phi_Phi_against_mpmath(probe):
    z = _phi_inputs()
    phi, Phi = probe.phi(z)
    e = _phi_errors(z, phi, Phi)
    _report("phi: ulp beyond z^2/2", e["phi"], C_PHI)
    _report("Phi z<=0: ulp beyond z^2/2", e["Phi_neg"], C_PHI_CDF)
    _report("Phi z<=0: (1+z^2/2)-ulp", e["Phi_neg_rel"])
    _report("Phi z>0: abs", e["Phi_pos"], 2.0 ** -52)
    _report("EI tail: (1+z^2)-ulp", e["ei"], C_EI_TAIL)
    _report("Phi/phi z<=0 (ulp)", e["mills"], C_MILLS)
    assert e["ei"] <= C_EI_TAIL_SHARED
    assert e["phi"] <= C_PHI
    assert e["Phi_neg"] <= C_PHI_CDF
    assert e["Phi_pos"] <= 2.0 ** -52
    assert e["ei"] <= C_EI_TAIL
    assert e["mills"] <= C_MILLS
    # beyond the u = 40 clamp: φ = 0 and Φ ∈ {0, 1} exactly; NaN stays NaN
    far = np.array([56.6, 100.0, 1e300, -56.6, -100.0, -1e300, np.nan])
    fphi, fPhi = probe.phi(far)
    assert (fphi[:6] == 0.0).all()
    assert (fPhi[:3] == 1.0).all() and (fPhi[3:6] == 0.0).all()
    assert np.isnan(fphi[6]) and np.isnan(fPhi[6])


# =====================================================================================================
# decision rules
# =====================================================================================================
RULE_EI, RULE_POI, RULE_LCB = 0, 1, 2
SIGMA_TOL = 1e-8
RULE_CASES = [(RULE_EI, 0.0), (RULE_POI, 0.0), (RULE_POI, 0.05)]
RULE_OUT = ("g", "gmu", "gsig", "gmumu", "gsigsig", "gmuth", "gsigth")
# which outputs hold Φ or the EI sum (conditioning 1 + z²); the others are pure-φ (1 + z²/2)
RULE_CDF_OUT = {RULE_EI: (0, 1), RULE_POI: (0,)}


def _mp_pair(z):
    return mp.npdf(z), mp.erfc(-z / mp.sqrt(2)) / 2


def _rule_closed_forms(rule, mu, sig, theta, fmin, pair):
    """the seven partials listed in the header (any arithmetic: mpmath or host floats);
    pair(z) = (φ(z), Φ(z))"""
    imp = fmin - mu - theta
    z = imp / sig
    phi, Phi = pair(z)
    if rule == RULE_EI:
        return (imp * Phi + sig * phi, -Phi, phi, phi / sig, z * z * phi / sig, phi / sig, z * phi / sig)
    p2 = phi / (sig * sig)
    return (Phi, -phi / sig, -z * phi / sig, -z * p2, z * (2 - z * z) * p2, -z * p2, (1 - z * z) * p2)


def _rule_g(rule, mu, sig, theta, fmin):
    z = (fmin - mu - theta) / sig
    Phi = mp.erfc(-z / mp.sqrt(2)) / 2
    if rule == RULE_EI:
        return (fmin - mu - theta) * Phi + sig * mp.npdf(z)
    if rule == RULE_POI:
        return Phi
    return theta * sig - mu


def test_rule_closed_forms_match_mp_diff():
    """The reference partials of the GPU test are the derivatives of g(μ, σ, θ): mp.diff agrees."""
    orders = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (2, 0, 0), (0, 2, 0), (1, 0, 1), (0, 1, 1)]
    fmin = mpf("0.3")
    for rule, theta in RULE_CASES:
        for mu, sig in [(-0.4, 0.7), (0.9, 0.25), (0.3, 1.5), (2.0, 0.5), (-3.0, 0.8)]:
            mu, sig, th = mpf(mu), mpf(sig), mpf(theta)
            cf = _rule_closed_forms(rule, mu, sig, th, fmin, _mp_pair)
            for want, od in zip(cf, orders):
                got = mp.diff(lambda a, b, c: _rule_g(rule, a, b, c, fmin), (mu, sig, th), od)
                assert abs(got - want) <= mpf(10) ** -25 * (1 + abs(want)), (rule, theta, mu, sig, od, got, want)


@functools.lru_cache(None)
def _rule_inputs(theta):
    """(μ, σ) with fmin = 0 that put z = (−μ − θ)/σ in [−30, 30] and σ in [1e-8, 10]"""
    rng = np.random.default_rng(14)
    n = 1300
    z = np.concatenate([rng.uniform(-30.0, 30.0, n - 300), rng.uniform(-4.0, 4.0, 300)])
    sig = 10.0 ** rng.uniform(-8.0, 1.0, n)
    sig[:40] = SIGMA_TOL
    sig[40:80] = 10.0
    mu = -(z * sig) - theta
    return mu, sig


@functools.lru_cache(None)
def _rule_ref(rule, theta):
    mu, sig = _rule_inputs(theta)
    th = mpf(theta)
    rows = [_rule_closed_forms(rule, mpf(float(m)), mpf(float(s)), th, mpf(0), _mp_pair) for m, s in zip(mu, sig)]
    zs = np.array([float((-mpf(float(m)) - th) / mpf(float(s))) for m, s in zip(mu, sig)])
    return [[r[k] for r in rows] for k in range(7)], zs


def _rule_errors(rule, theta, out):
    """max normalised error over the CDF-type and over the PDF-type outputs"""
    ref, z = _rule_ref(rule, theta)
    worst = {"cdf": 0.0, "pdf": 0.0}
    for k in range(7):
        e = _err_ulps(out[k], ref[k])
        if k in RULE_CDF_OUT[rule]:
            worst["cdf"] = max(worst["cdf"], (e / (1.0 + z * z)).max())
            continue
        cond = 1.0 + 0.5 * z * z
        if rule == RULE_POI and k == 4:
            cond = cond * (2.0 + z * z) / np.abs(2.0 - z * z)
        if rule == RULE_POI and k == 6:
            cond = cond * (1.0 + z * z) / np.abs(1.0 - z * z)
        worst["pdf"] = max(worst["pdf"], (e / cond).max())
    return worst


def _host_rule(rule, theta, pair=None):
    """host fp64 partials from libm exp and erfc, or from another host pair (_host_mills)"""
    mu, sig = _rule_inputs(theta)
    return np.array(_rule_closed_forms(rule, mu, sig, theta, 0.0, pair or _host_phi_Phi))


@gpu_test
@pytest.mark.parametrize("rule,theta", RULE_CASES)
def test_rule_partials_against_mpmath(probe, rule, theta):
    mu, sig = _rule_inputs(theta)
    o7, o6 = probe.rule(rule, mu, sig, 1.0 / sig, theta, 0.0, SIGMA_TOL)
    assert _same_bits(o7, o6), "the six- and seven-argument overloads differ with isig = 1/sigma"
    w = _rule_errors(rule, theta, o7)
    _report(f"rule {rule} theta {theta}: CDF outputs, (1+z^2)-ulp", w["cdf"], C_RULE_CDF)
    _report(f"rule {rule} theta {theta}: PDF outputs, (1+z^2/2)-ulp", w["pdf"], C_RULE_PDF)
    assert w["cdf"] <= C_RULE_CDF
    if rule == RULE_EI:
        assert w["cdf"] <= C_RULE_EI_SHARED
    assert w["pdf"] <= C_RULE_PDF


@gpu_test
@pytest.mark.parametrize("rule,theta", RULE_CASES)
def test_rule_partials_sigma_branches(probe, rule, theta):
    below = np.nextafter(SIGMA_TOL, 0.0)
    sig = np.array([below, below, 0.0, 1e-300, SIGMA_TOL, np.nan, np.inf])
    mu = np.array([-0.3, 0.4, -0.3, 0.2, -theta - 1e-8, -0.3, -0.3])   # z = 1 at σ = σtol
    with np.errstate(all="ignore"):
        isig = 1.0 / sig
    o7, o6 = probe.rule(rule, mu, sig, isig, theta, 0.0, SIGMA_TOL)
    assert _same_bits(o7, o6)
    assert (o7[:, :4] == 0.0).all(), o7[:, :4]              # σ < σtol: exact zeros
    assert (o7[0, 4] != 0.0) and np.isfinite(o7[:, 4]).all()   # σ = σtol takes the rule
    assert np.isnan(o7[:, 5]).all(), o7[:, 5]               # σ = NaN falls through to NaN
    inf = o7[:, 6]                                          # σ = +inf: z = 0 exactly
    phi0 = 0.3989422804014327
    if rule == RULE_EI:
        assert inf[0] == np.inf and abs(inf[1] + 0.5) <= 2.0 ** -52 and inf[2] == phi0 and (inf[3:] == 0.0).all(), inf
    else:
        assert abs(inf[0] - 0.5) <= 2.0 ** -52 and (inf[1:] == 0.0).all(), inf


@gpu_test
def test_rule_partials_lcb(probe):
    theta = 2.0
    mu, sig = _rule_inputs(0.0)
    sig = np.concatenate([sig, [np.inf, 0.0, np.nextafter(SIGMA_TOL, 0.0)]])
    mu = np.concatenate([mu, [0.5, 0.5, 0.5]])
    with np.errstate(all="ignore"):
        o7, o6 = probe.rule(RULE_LCB, mu, sig, 1.0 / sig, theta, 0.0, SIGMA_TOL)
    assert _same_bits(o7, o6)
    fin = np.isfinite(sig)
    ref = [mpf(theta) * mpf(float(s)) - mpf(float(m)) for m, s in zip(mu[fin], sig[fin])]
    # θσ − μ may cancel (μ = −zσ with z near −θ): one rounding of each term, absolute
    scale = np.spacing(theta * sig[fin] + np.abs(mu[fin]))
    assert (_abs_err(o7[0][fin], ref) <= scale).all()
    assert o7[0][~fin][0] == np.inf
    for k, v in ((1, -1.0), (2, theta), (3, 0.0), (4, 0.0), (5, 0.0), (6, 1.0)):
        assert (o7[k] == v).all(), RULE_OUT[k]


# =====================================================================================================
# radial kernels
# =====================================================================================================
KINDS = {"matern52": 0, "matern32": 1, "matern12": 2, "se": 3, "periodic": 4}
ELLS = (0.05, 1.0, 20.0)
PERIODS = (0.8, 2.5)


def _cK(kind, ell):
    return {0: math.sqrt(5.0) / ell, 1: math.sqrt(3.0) / ell, 2: 1.0 / ell, 3: 1.0 / (ell * ell),
            4: 1.0 / (ell * ell)}[kind]


@functools.lru_cache(None)
def _rho2_grid():
    rng = np.random.default_rng(15)
    return np.concatenate([[0.0, 5e-324, 1e-300, 1e-200], 10.0 ** np.linspace(-40.0, 4.0, 331),
                           10.0 ** rng.uniform(-6.0, 4.0, 200)])


def _periodic_rho2(cP):
    """the common grid plus t = cP·ρ fine across the series switch at 0.1, and near π and 2π"""
    t = np.concatenate([np.linspace(0.05, 0.15, 241), np.nextafter(0.1, [0.0, 1.0]), [0.1],
                        math.pi + np.linspace(-1e-3, 1e-3, 21), 2 * math.pi + np.linspace(-1e-3, 1e-3, 21),
                        math.pi * (1 + np.array([-1e-9, 1e-9, -1e-13, 1e-13]))])
    return np.concatenate([_rho2_grid(), (t / cP) ** 2])


def _rad_cases(kind):
    if kind != 4:
        return [(ell, _cK(kind, ell), 0.0, _rho2_grid()) for ell in ELLS]
    return [(ell, _cK(kind, ell), 2.0 * math.pi / p, _periodic_rho2(2.0 * math.pi / p)) for ell in ELLS for p in PERIODS]


def _rad_forms(kind, c, B, rho2, exp, sqrt, sin, cos, small_f):
    """ψ, g1 = ψ'/ρ, g2 = (ψ'' − ψ'/ρ)/ρ² and the exponent s at one ρ² > 0 (any arithmetic);
    small_f(t): (sin t − t cos t)/t³ where the closed form cancels"""
    rho = sqrt(rho2)
    if kind == 4:
        A, t = B * c, B * rho
        h = sin(t / 2)
        s = 2 * c * h * h
        psi = exp(-s)
        sinc = sin(t) / t
        f = small_f(t) if t < 0.1 else (sin(t) - t * cos(t)) / (t * t * t)
        return psi, -psi * A * B * sinc, psi * B * B * A * (A * sinc * sinc + B * f), s
    if kind == 3:
        s = c * rho2 / 2
        e = exp(-s)
        return e, -c * e, c * c * e, s
    s = c * rho
    e = exp(-s)
    if kind == 0:
        return (1 + s + s * s / 3) * e, -(c * c / 3) * (1 + s) * e, (c * c * c * c / 3) * e, s
    if kind == 1:
        return (1 + s) * e, -c * c * e, c * c * c * e / rho, s
    return e, -c * e / rho, (c * c * e + c * e / rho) / rho2, s


def _rad_at_zero(kind, c, B):
    """ρ = 0: ψ(0) = 1, g1 = ψ''(0); g2 = 0 where the device branches (Matérn-3/2, -1/2), else the
    limit of the closed form, which the branch-free kinds return (it multiplies r rᵀ = 0)"""
    if kind == 4:
        A = B * c
        return mpf(1), -A * B, B * B * A * (A + B / 3)
    if kind == 3:
        return mpf(1), -c, c * c
    if kind == 0:
        return mpf(1), -c * c / 3, c * c * c * c / 3
    if kind == 1:
        return mpf(1), -c * c, mpf(0)
    return mpf(1), c * c, mpf(0)


def _f_series(t):
    """(sin t − t cos t)/t³ = Σ (−1)^k t^(2k)·(2k + 2)/(2k + 3)!  (t < 0.1: seven terms are exact to 1e-30)"""
    t2, acc, term = t * t, 0, None
    for k in range(7):
        term = (2 * k + 2) / mp.factorial(2 * k + 3) * (-1) ** k * t2 ** k
        acc = acc + term
    return acc


def _f_series_host(t):
    t2 = t * t
    return 1.0 / 3.0 + t2 * (-1.0 / 30.0 + t2 * (1.0 / 840.0 + t2 * (-1.0 / 45360.0 + t2 * (1.0 / 3991680.0))))


@functools.lru_cache(None)
def _rad_ref(kind):
    """per case: reference (ψ, g1, g2) in mpmath, the conditioning and the subnormal allowance"""
    out = []
    for ell, cK, cP, rho2 in _rad_cases(kind):
        c, B = mpf(cK), mpf(cP)
        refs, cond, sub = ([], [], []), [], ([], [], [])
        for r2 in rho2:
            if r2 == 0.0:
                q = _rad_at_zero(kind, c, B)
                s, t = mpf(0), mpf(0)
            else:
                x = mpf(float(r2))
                *q, s = _rad_forms(kind, c, B, x, mp.exp, mp.sqrt, mp.sin, mp.cos, _f_series)
                t = B * mp.sqrt(x)
            e = mp.exp(-s)
            for k in range(3):
                refs[k].append(q[k])
                sub[k].append(float(abs(q[k]) / e) * TINY)
            cond.append(float(1 + s + (c * t if kind == 4 else 0)))
        if kind == 4:
            A = B * c
            psi = _f(refs[0])
            mult = (1.0, float(A * B), float(B * B * A * (A + B)))
            scales = tuple(psi * m for m in mult)
            sub = [np.full(len(cond), m * TINY) for m in mult]
        else:
            scales = None
        out.append((refs, np.array(cond), [np.array(v) for v in sub], scales))
    return out


def _rad_errors(kind, results):
    """results: per case [3][n] values.  Max normalised error of ψ, g1, g2 over all cases; the points
    where the reference overflows fp64 (Matérn-1/2 g2 below ρ ≈ 1e-103) are left to the caller."""
    worst = np.zeros(3)
    for (refs, cond, sub, scales), val in zip(_rad_ref(kind), results):
        for k in range(3):
            rf = _f(refs[k])
            ok = np.isfinite(rf)
            err = _abs_err(val[k][ok], [r for r, m in zip(refs[k], ok) if m])
            # the allowance for a subnormal exponential (a few of its ulps, 2⁻¹⁰⁷⁴, times the factor in
            # front of it) is taken out before normalising; it is below 1e-300 of any normal result
            e = np.maximum(err - 4.0 * sub[k][ok], 0.0)
            if kind == 4:
                unit = np.maximum(2.0 ** -53 * scales[k][ok], TINY) * cond[ok]
            else:
                unit = _ulp([r for r, m in zip(refs[k], ok) if m]) * cond[ok]
            worst[k] = max(worst[k], (e / unit).max())
    return worst


def _host_rad(kind):
    res = []
    for ell, cK, cP, rho2 in _rad_cases(kind):
        val = np.empty((3, rho2.size))
        for i, r2 in enumerate(rho2):
            if r2 == 0.0:
                val[:, i] = [float(v) for v in _rad_at_zero(kind, cK, cP)]
                continue
            with np.errstate(all="ignore"):
                val[:, i] = _rad_forms(kind, cK, cP, np.float64(r2), np.exp, np.sqrt, np.sin, np.cos, _f_series_host)[:3]
        res.append(val)
    return res


@gpu_test
@pytest.mark.parametrize("name", list(KINDS))
def test_rad_eval_against_mpmath(probe, name):
    """ψ, g1, g2 of every kind against the closed forms, rad_eval2 against two rad_eval calls.

    Matérn-1/2 below ρ ≈ 1e-103 (ρ² < 1e-206): g2 ≈ c/ρ³ exceeds fp64 and the device returns +inf
    (1/ρ² itself overflows below ρ = 7.5e-155); at ρ = 0 the branch gives g2 = 0.  g2 multiplies
    r rᵀ, of magnitude ρ², so ∇²k of such a row is inf·0 on a data point that coincides with the
    evaluation point to 1e-103 -- not reachable from fp64 coordinates of ordinary size, whose differences
    are either 0 or above 1e-300·|x|.  Matérn-3/2 g2 = c³e/ρ stays finite for every ρ² > 0 (ρ ≥ 2.2e-162).
    From ρ² = 1e-200 upwards every output of every kind must be finite."""
    kind = KINDS[name]
    results = []
    for ell, cK, cP, rho2 in _rad_cases(kind):
        one, two_a, two_b = probe.rad(kind, cK, cP, rho2)
        for two, ref in ((two_a, one), (two_b, one[:, ::-1])):
            if kind == 0:
                # Matérn-5/2 g1 = −c²/3·(1 + cρ)·e: the compiler may fuse 1 + cρ in one function and not in
                # the other (the header says why the source is left alone).  The fused and the two-step
                # sum differ by at most one ulp (the product's rounding is below one ulp of the sum, the
                # sum's and the FMA's are half an ulp each), a relative 2u with u = 2⁻⁵³; each of the two
                # multiplications after it adds the two paths' roundings, 2u: below 6u in all, so at most
                # 5 ulp.  ψ and g2 hold no such sum and keep the bits.
                assert _same_bits(two[0], ref[0]) and _same_bits(two[2], ref[2]), "rad_eval2 != two rad_eval calls"
                with np.errstate(invalid="ignore"):
                    d = np.abs(two[1] - ref[1]) / np.spacing(np.abs(ref[1]))
                _report("rad_eval2 vs rad_eval, matern52 g1 (ulp)", d.max(), 5)
                assert d.max() <= 5.0
            else:
                assert _same_bits(two, ref), "rad_eval2 != two rad_eval calls"
        assert np.isfinite(one[:, rho2 >= 1e-200]).all()
        zero = rho2 == 0.0
        assert (one[0][zero] == 1.0).all()
        if kind in (1, 2):
            assert (one[2][zero] == 0.0).all()
        if kind == 2:
            assert (one[2][(rho2 > 0) & (rho2 < 1e-250)] == np.inf).all()
        results.append(one)
    worst = _rad_errors(kind, results)
    limits = C_PER if kind == 4 else C_RAD
    for k, q in enumerate(("psi", "g1", "g2")):
        _report(f"rad_eval {name} {q}", worst[k], limits[k])
    for k in range(3):
        assert worst[k] <= limits[k], (name, ("psi", "g1", "g2")[k], worst[k])


# =====================================================================================================
# cost model
# =====================================================================================================
COST_QUADRATIC, COST_LOGLINEAR = 1, 2
COST_C0 = 0.7


@functools.lru_cache(None)
def _cost_inputs(D):
    rng = np.random.default_rng(16 + D)
    lb = rng.uniform(-3.0, 1.0, D)
    delta = rng.uniform(0.5, 4.0, D)
    w = rng.uniform(0.1, 3.0, D)
    n = 120
    u = rng.uniform(0.0, 1.0, (n, D))
    u[:10] = rng.integers(0, 2, (10, D))      # corners of the box
    u[10] = 0.0
    u[11] = 1.0
    x = lb + u * delta
    x[:12] = np.where(u[:12] == 0.0, lb, lb + delta)
    return lb, delta, w, x


def _cost_forms(cost, c0, lb, delta, w, x, exp):
    """c, ∇c, Hc and the exponent t at one point (any arithmetic)"""
    D = len(lb)
    u = [(x[a] - lb[a]) / delta[a] for a in range(D)]
    if cost == COST_QUADRATIC:
        c = c0 + sum(w[a] * u[a] * u[a] for a in range(D))
        g = [2 * w[a] * u[a] / delta[a] for a in range(D)]
        H = [[(2 * w[a] / (delta[a] * delta[a]) if a == b else 0 * c0) for b in range(D)] for a in range(D)]
        return c, g, H, 0 * c0
    t = sum(w[a] * u[a] for a in range(D))
    c = c0 * exp(t)
    g = [c * w[a] / delta[a] for a in range(D)]
    H = [[c * (w[a] / delta[a]) * (w[b] / delta[b]) for b in range(D)] for a in range(D)]
    return c, g, H, t


@functools.lru_cache(None)
def _cost_ref(D, cost):
    lb, delta, w, x = _cost_inputs(D)
    m = lambda v: [mpf(float(q)) for q in v]   # noqa: E731
    rows = [_cost_forms(cost, mpf(COST_C0), m(lb), m(delta), m(w), m(xi), mp.exp) for xi in x]
    flat = [[r[0]] + list(r[1]) + [h for row in r[2] for h in row] for r in rows]
    return flat, np.array([float(abs(r[3])) for r in rows])


def _cost_error(D, cost, c, g, H):
    flat, t = _cost_ref(D, cost)
    worst = 0.0
    for i, ref in enumerate(flat):
        val = np.concatenate([[c[i]], g[i], H[i].ravel()])
        worst = max(worst, (_err_ulps(val, ref) / (1.0 + t[i])).max())
    return worst


def _host_cost(D, cost):
    lb, delta, w, x = _cost_inputs(D)
    rows = [_cost_forms(cost, COST_C0, lb, delta, w, xi, np.exp) for xi in x]
    return (np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), np.array([r[2] for r in rows]))


@gpu_test
@pytest.mark.parametrize("D", [2, 8])
@pytest.mark.parametrize("cost", [COST_QUADRATIC, COST_LOGLINEAR])
def test_cost_model_against_mpmath(probe, D, cost):
    lb, delta, w, x = _cost_inputs(D)
    c, g, H = probe.cost(D, cost, COST_C0, lb, delta, w, x)
    worst = _cost_error(D, cost, c, g, H)
    _report(f"cost model {cost} D={D}: (1+|t|)-ulp", worst, C_COST)
    assert worst <= C_COST
    # Hc symmetric: the quadratic model is diagonal; a log-linear entry is c·v_a·v_b rounded twice from
    # left to right, so (a, b) and (b, a) are two roundings of one product (the kernel evaluates each
    # pair once and stores it twice)
    Ht = np.swapaxes(H, 1, 2)
    if cost == COST_QUADRATIC:
        assert _same_bits(H, Ht)
    else:
        assert (np.abs(H - Ht) <= 2.0 * np.spacing(np.minimum(np.abs(H), np.abs(Ht)))).all()


# =====================================================================================================
# reductions (one wave)
# =====================================================================================================
# partner of lane l at each step, as the exchange instructions pair the lanes: v_permlane32_swap and
# v_permlane16_swap pair l with l^32 and l^16; DPP row_mirror pairs l with l^15 (15 − l within its row
# of 16), row_half_mirror l with l^7, quad_perm [2,3,0,1] and [1,0,3,2] l with l^2 and l^1
PARTNER = {32: 32, 16: 16, 8: 15, 4: 7, 2: 2, 1: 1}


def _emulate_reduce(v, top):
    """wave_reduce<K> (top = 32) / half_reduce<K> (top = 16) of v [64][K]: per lane the final value
    and the slot index, by the fixed butterfly of the header (fp64 adds in the device's order; the
    add of a pair is commutative, so both partners hold the same bits)"""
    v = np.array(v, dtype=np.float64)
    K = v.shape[1]
    lanes = np.arange(64)
    idx = np.zeros(64, dtype=int)
    M, H = top, K // 2
    while H >= 1:                       # transpose steps
        up = (lanes & M) != 0
        partner = lanes ^ PARTNER[M]
        new = v.copy()
        for q in range(H):
            lo = v[:, q] + v[partner, q]              # lanes with bit M clear: a(l) + a(partner)
            hi = v[partner, q + H] + v[:, q + H]      # lanes with it set: b(partner) + b(l)
            new[:, q] = np.where(up, hi, lo)
        v = new
        idx += np.where(up, H, 0)
        M //= 2
        H //= 2
    while M >= 1:                       # all-reduce steps
        v[:, 0] = v[:, 0] + v[lanes ^ PARTNER[M], 0]
        M //= 2
    return v[:, 0], idx


def _emulated_red(v, half):
    val, idx = _emulate_reduce(v, 16 if half else 32)
    K = v.shape[1]
    red = np.full((2, K) if half else (1, K), np.nan)
    for l in range(64):
        h = l >> 5 if half else 0
        if not np.isnan(red[h, idx[l]]):
            assert _bits(red[h, idx[l]:idx[l] + 1])[0] == _bits(val[l:l + 1])[0]
        red[h, idx[l]] = val[l]
    return red if half else red[0]


REDUCE_CASES = [(K, False) for K in (1, 2, 4, 8, 16, 32)] + [(K, True) for K in (1, 2, 4, 8, 16)]


@gpu_test
@pytest.mark.parametrize("K,half", REDUCE_CASES)
def test_wave_and_half_reduce(probe, K, half):
    lanes = np.arange(64)
    # (a) exact integer sums, distinct per lane and per component; the halves carry different data
    v = np.array([[(l + 1) * 2.0 ** k + (1000.0 * (k + 1) if l >= 32 else 0.0) for k in range(K)] for l in lanes])
    red = probe.reduce(v, half)
    if half:
        assert np.array_equal(red[0], v[:32].sum(axis=0)) and np.array_equal(red[1], v[32:].sum(axis=0)), red
    else:
        assert np.array_equal(red, v.sum(axis=0)), red
    # (b) random doubles: the bits of the fixed butterfly
    rng = np.random.default_rng(17 + K)
    for spread in (0.0, 20.0):          # of one magnitude, and over seventeen orders of magnitude
        r = rng.standard_normal((64, K)) * np.exp(rng.uniform(-spread, spread, (64, K)))
        assert _same_bits(probe.reduce(r, half), _emulated_red(r, half)), (K, half)


@gpu_test
def test_allreduce_and_lanes_min(probe):
    lanes = np.arange(64)
    v = (lanes + 1.0) * 3.0
    s, m64, m32 = probe.allreduce(v)
    assert (s == v.sum()).all() and (m64 == 3.0).all()
    assert (m32[:32] == 3.0).all() and (m32[32:] == 99.0).all()
    rng = np.random.default_rng(18)
    r = rng.standard_normal(64) * np.exp(rng.uniform(-20.0, 20.0, 64))
    s, m64, m32 = probe.allreduce(r)
    want, _ = _emulate_reduce(r[:, None], 32)
    assert _same_bits(s, want) and len(set(_bits(s))) == 1
    assert _same_bits(m64, np.full(64, r.min()))
    assert _same_bits(m32, np.repeat([r[:32].min(), r[32:].min()], 32))
    # (c) NaN in some lanes (fmin skips it), ±0, ±inf
    n = r.copy()
    n[[0, 5, 31, 32, 63]] = np.nan
    _, m64, m32 = probe.allreduce(n)
    assert _same_bits(m64, np.full(64, np.nanmin(n)))
    assert _same_bits(m32, np.repeat([np.nanmin(n[:32]), np.nanmin(n[32:])], 32))
    n = np.full(64, np.nan)
    n[40] = 2.5
    _, m64, m32 = probe.allreduce(n)
    assert (m64 == 2.5).all() and np.isnan(m32[:32]).all() and (m32[32:] == 2.5).all()
    zs = np.abs(r) + 1.0
    zs[[3, 40]] = 0.0
    zs[[17, 50]] = -0.0
    _, m64, m32 = probe.allreduce(zs)
    assert (m64 == 0.0).all() and len(set(_bits(m64))) == 1
    assert (m32 == 0.0).all() and len(set(_bits(m32[:32]))) == 1 and len(set(_bits(m32[32:]))) == 1
    inf = r.copy()
    inf[7] = np.inf
    inf[44] = -np.inf
    s, m64, m32 = probe.allreduce(inf)
    assert (m64 == -np.inf).all() and (m32[32:] == -np.inf).all()
    assert _same_bits(m32[:32], np.full(32, np.delete(r[:32], 7).min()))
    assert np.isnan(s).all()    # +inf + −inf
    inf[44] = 1.0
    s, m64, _ = probe.allreduce(inf)
    assert (s == np.inf).all()


# =====================================================================================================
# dual-draw stream
# =====================================================================================================
def _splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return z ^ (z >> 31)


def _dual_uniform(seed, traj, j, k):
    key = _splitmix64(_splitmix64(seed ^ 0x5851F42D4C957F2D) ^ (traj & 0xFFFFFFFFFFFFFFFF))
    key = _splitmix64(key ^ ((j & 0xFFFFFFFF) << 32 | (k & 0xFFFFFFFF)))
    return (key >> 11) / 9007199254740992.0


@gpu_test
def test_dual_uniform_device_equals_host(probe):
    rng = np.random.default_rng(19)
    n = 4096
    seed = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    seed[:4] = [0, 1, 1906, 2 ** 64 - 1]
    traj = rng.integers(0, 2 ** 20, n, dtype=np.int64)
    traj[1024:2048] = rng.integers(2 ** 32, 2 ** 62, 1024, dtype=np.int64)
    traj[:3] = [0, 2 ** 32, 2 ** 32 + 1]
    j = rng.integers(0, 64, n, dtype=np.int32)
    k = rng.integers(0, 16, n, dtype=np.int32)
    dev, host = probe.dual(seed, traj, j, k)
    assert _same_bits(dev, host)
    assert ((dev >= 0.0) & (dev < 1.0)).all()
    # and both are the stream the header writes down
    py = np.array([_dual_uniform(int(s), int(t), int(a), int(b)) for s, t, a, b in zip(seed[:256], traj[:256], j[:256], k[:256])])
    py2 = np.array([_dual_uniform(int(s), int(t), int(a), int(b))
                    for s, t, a, b in zip(seed[1024:1100], traj[1024:1100], j[1024:1100], k[1024:1100])])
    assert _same_bits(host[:256], py) and _same_bits(host[1024:1100], py2)


# =====================================================================================================
# CPU: the host maxima behind the constants
# =====================================================================================================
def _host_maxima():
    out = {}
    z = _phi_inputs()
    e = _phi_errors(z, *_host_phi_Phi(z))
    out["C_PHI"] = (e["phi"], C_PHI)
    out["C_PHI_CDF"] = (e["Phi_neg_rel"], C_PHI_CDF)
    out["C_EI_TAIL"] = (e["ei"], C_EI_TAIL)
    shared = _phi_errors(z, *_host_mills(z))
    out["C_MILLS"] = (shared["mills"], C_MILLS)
    out["C_EI_TAIL_SHARED"] = (shared["ei"], C_EI_TAIL_SHARED)
    out["C_RULE_EI_SHARED"] = (_rule_errors(RULE_EI, 0.0, _host_rule(RULE_EI, 0.0, _host_mills))["cdf"], C_RULE_EI_SHARED)
    cdf = pdf = 0.0
    for rule, theta in RULE_CASES:
        w = _rule_errors(rule, theta, _host_rule(rule, theta))
        cdf, pdf = max(cdf, w["cdf"]), max(pdf, w["pdf"])
    out["C_RULE_CDF"] = (cdf, C_RULE_CDF)
    out["C_RULE_PDF"] = (pdf, C_RULE_PDF)
    rad = np.zeros(3)
    for kind in (0, 1, 2, 3):
        rad = np.maximum(rad, _rad_errors(kind, _host_rad(kind)))
    per = _rad_errors(4, _host_rad(4))
    for k, q in enumerate(("PSI", "G1", "G2")):
        out[f"C_RAD_{q}"] = (rad[k], C_RAD[k])
        out[f"C_PER_{q}"] = (per[k], C_PER[k])
    cost = 0.0
    for D in (2, 8):
        for model in (COST_QUADRATIC, COST_LOGLINEAR):
            cost = max(cost, _cost_error(D, model, *_host_cost(D, model)))
    out["C_COST"] = (cost, C_COST)
    return out


def test_host_maxima_within_a_quarter_of_the_limits():
    """Each limit is 4 × the error of the same closed form in host fp64 (libm exp / erfc) on the same
    inputs, rounded up: the host maxima, measured again here, stay within a quarter of the constants."""
    for name, (host, limit) in _host_maxima().items():
        _report(f"host {name}", host, limit)
        assert host <= limit / 4.0, (name, host, limit)


def test_old_sinc_series_misses_the_periodic_limit():
    """The three-term series 1 − t²/6 + t⁴/120 that rad_eval used for sinc t below t = 0.1 misses the
    Periodic g1 limit by six orders of magnitude (first dropped term t⁶/5040: 2e-10 at t = 0.0999)."""
    t = mpf(float(np.float64(0.0999)))
    series = 1 - t * t / 6 + t ** 4 / 120
    rel = float(abs(series - mp.sin(t) / t) / (mp.sin(t) / t))
    cond = 1 + 2 * _cK(4, 1.0) * math.sin(0.04995) ** 2 + _cK(4, 1.0) * 0.0999
    assert rel > 1.9e-10
    assert rel / (2.0 ** -53 * cond) > 1e4 * C_PER[1]
