"""The McDougall-Wright-Jackett-Feistel equation of state (state_mod.F90:418-498, state_range_opt 'enforce') in 40-digit arithmetic
(mpmath), and its derivatives by mpmath.diff OF THAT DENSITY -- not a restatement of the reference's derivative code (:500-560), which
would carry the same reading of it.  Nothing here is imported from the library under test or from the oracle.

The coefficients are the decimal strings of tests/ice_ref.py: rho (typed in from the reference); the level pressures are ice_ref.pressz.
Range rule: -2 <= T <= 999, 0 <= S <= 0.999 [g/g]; the derivative with respect to a clipped argument is the derivative AT the clip value,
as the reference evaluates it (it differentiates the rational function, not the clip).

The density is a rational function of T, SQ = 1000 S and sqrt(SQ).  At S = 0 it has no Taylor series in S (the SQ^(3/2) terms), so a
difference quotient in S converges like sqrt(step) there; in q = sqrt(SQ) it is a ratio of polynomials, rho = a0 + a2 q^2 + a3 q^3 + ...,
and d rho / d SQ at 0 is a2 = rho''(q = 0) / 2: that second derivative is what is taken at S = 0."""
import functools

import mpmath as mp
import numpy as np

import ice_ref

DPS = 40
TMIN, TMAX, SMIN, SMAX = "-2", "999", "0", "0.999"
_C = {name: mp.mpf(text) for name, text in dict(
    n0_0="9.99843699e+2", n0_1="1.04004591e-2", n0_2="-3.24041825e-8", n1="7.35212840e+0",
    n2_0="-5.45928211e-2", n2_1="1.03970529e-7", n2_2="-1.23869360e-11", n3="3.98476704e-4",
    ns1_0="2.96938239e+0", ns1_1="5.18761880e-6", ns1t1="-7.23268813e-3", ns2="2.12382341e-3",
    d0_1="5.30848875e-6", d1_0="7.28606739e-3", d1_3="-1.27934137e-17", d2="-4.60835542e-5",
    d3_0="3.68390573e-7", d3_2="-3.03175128e-16", d4="1.80809186e-10",
    ds1="2.14691708e-3", ds1t1="-9.27062484e-6", ds1t3="-1.78343643e-10", dsqr="4.76534122e-6", dsqrt2="1.63410736e-9").items()}


def _density(t, sq, sqr, pbar):
    """rho [g/cm^3] of the (already clipped) temperature t, sq = 1000 S and sqr = sqrt(sq) at pbar [bars]; mpmath numbers"""
    c, p = _C, 10 * pbar
    n0 = c["n0_0"] + p * (c["n0_1"] + p * c["n0_2"])
    n2 = c["n2_0"] + p * (c["n2_1"] + p * c["n2_2"])
    ns1 = c["ns1_0"] + p * c["ns1_1"]
    d0 = 1 + p * c["d0_1"]
    d1 = c["d1_0"] + p ** 3 * c["d1_3"]
    d3 = c["d3_0"] + p ** 2 * c["d3_2"]
    w1 = n0 + t * (c["n1"] + t * (n2 + c["n3"] * t)) + sq * (ns1 + c["ns1t1"] * t + c["ns2"] * sq)
    w2 = d0 + t * (d1 + t * (c["d2"] + t * (d3 + c["d4"] * t))) + \
        sq * (c["ds1"] + t * (c["ds1t1"] + t * t * c["ds1t3"]) + sqr * (c["dsqr"] + t * t * c["dsqrt2"]))
    return w1 / w2 / 1000


def _clip(T, S):
    t = min(max(mp.mpf(T), mp.mpf(TMIN)), mp.mpf(TMAX))
    s = min(max(mp.mpf(S), mp.mpf(SMIN)), mp.mpf(SMAX))
    return t, s


@functools.lru_cache(maxsize=None)
def _point(T, S, pbar, derivs):
    with mp.workdps(DPS):
        t, s = _clip(T, S)
        p = mp.mpf(pbar)
        sq = 1000 * s
        r = _density(t, sq, mp.sqrt(sq), p)
        if not derivs:
            return float(r), None, None
        dt = mp.diff(lambda x: _density(x, sq, mp.sqrt(sq), p), t)
        if s > 0:
            ds = mp.diff(lambda x: _density(t, 1000 * x, mp.sqrt(1000 * x), p), s)
        else:
            ds = 1000 * mp.diff(lambda q: _density(t, q * q, q, p), mp.mpf(0), 2) / 2
        return float(r), float(dt), float(ds)


def _over(T, S, pbar, derivs):
    T, S, P = np.broadcast_arrays(np.asarray(T, dtype=np.float64), np.asarray(S, dtype=np.float64), np.asarray(pbar, dtype=np.float64))
    out = np.array([_point(float(t), float(s), float(p), derivs) for t, s, p in zip(T.ravel(), S.ravel(), P.ravel())], dtype=object)
    return [out[:, n].astype(np.float64).reshape(T.shape) if (derivs or n == 0) else None for n in range(3)]


def rho(T, S, pbar):
    """density [g/cm^3] at pbar [bars], rounded to float64 at the end; T [deg C], S [g/g] of any (broadcastable) shapes"""
    return _over(T, S, pbar, False)[0]


def rho_derivs(T, S, pbar):
    """(rho, d rho / d T, d rho / d S) with S in g/g, as the model holds them"""
    return tuple(_over(T, S, pbar, True))


@functools.lru_cache(maxsize=None)
def _one_minus_ratio(Ta, Sa, Tb, Sb, pbar):
    with mp.workdps(DPS):
        (ta, sa), (tb, sb), p = _clip(Ta, Sa), _clip(Tb, Sb), mp.mpf(pbar)
        ra = _density(ta, 1000 * sa, mp.sqrt(1000 * sa), p)
        rb = _density(tb, 1000 * sb, mp.sqrt(1000 * sb), p)
        return float(1 - ra / rb)


def one_minus_ratio(Ta, Sa, Tb, Sb, pbar):
    """1 - rho(Ta, Sa, pbar) / rho(Tb, Sb, pbar), the difference formed in 40 digits and rounded once (in float64 the subtraction loses
    the leading digits the two densities share)"""
    a = np.broadcast_arrays(*[np.asarray(x, dtype=np.float64) for x in (Ta, Sa, Tb, Sb, pbar)])
    out = [_one_minus_ratio(*[float(v) for v in row]) for row in zip(*[x.ravel() for x in a])]
    return np.array(out, dtype=np.float64).reshape(a[0].shape)


def pressz(km):
    """pressure [bars] of the levels, index 0 unused (ice_ref.pressz: state_mod.F90:1041, 1765-1766)"""
    return ice_ref.pressz(km)
