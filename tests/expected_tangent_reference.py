"""References of the definition in include/cpm_expected_tangent.h, computed from the f64 tables (not a conftest: imported by
tests/test_expected_tangent.py and tests/test_expected_tangent_gpu.py):

  exact_direction   forward mode over fractions.Fraction: by linearity a direction (d pi_0, d p_drive, c) is
                    expected_grad_reference.exact_tangent + c * expected_grad_dest_reference.exact_tangent_dest.
  magnitude         the header's magnitude recurrence -- |d pi_0|, |dq|, |c|, |dP|, every difference an addition -- over Fractions.
  numpy_tangent     the recurrence in numpy f64 (numpy's own order of sums); magnitude=True: the magnitude recurrence in f64, for the
                    sizes the exact form is too slow for.
  bounds            the header's coefficients: h * (Z + 10) * 2^-52 for d parking after h operators, two roundings more for d driving.
  lm_problem        the planted zero-residual problem of refine_expected_lm's tests, and a numpy evaluator for it.

Tables are the host arrays of the ABI: p_drive and d_p_drive (Z, T), p_dest and dP (Z origin, Z dest, T), d_pi0 (Z,)."""
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

import expected_reference as R
import expected_grad_reference as G
import expected_grad_dest_reference as D

EPS = R.EPS
IVP = R.IVP
C2 = 10          # the header's c2 (c1 = 1)


def exact_direction(p_drive, p_dest, pi0, flags, d_pi0=None, d_p_drive=None, c=0.0, dP=None, tables=None):
    """(d parking, d driving: (Z, T) object arrays of Fraction, d pi_next: list of Fraction) of one direction, no rounding"""
    Z, T = p_drive.shape
    d_pi0 = np.zeros(Z) if d_pi0 is None else d_pi0
    d_p_drive = np.zeros((Z, T)) if d_p_drive is None else np.where(G.inside(p_drive), d_p_drive, 0.0)
    park, drv, nxt = G.exact_tangent(p_drive, p_dest, pi0, flags, d_pi0, d_p_drive, tables)
    if c != 0.0:
        cf = Fraction(float(c))
        pk2, dr2, nx2 = D.exact_tangent_dest(p_drive, p_dest, dP, pi0, flags, tables)
        park, drv, nxt = park + cf * pk2, drv + cf * dr2, [a + cf * b for a, b in zip(nxt, nx2)]
    return park, drv, nxt


def _frac(a):
    return np.array([Fraction(float(v)) for v in np.asarray(a, dtype=np.float64).ravel()], dtype=object).reshape(np.shape(a))


def _propagate(p_drive, p_dest, pi0, flags, d_pi0, d_p_drive, c, dP, tables, magnitude, exact):
    """The definition's recurrence with numpy arrays of f64 (exact=False: numpy's order of sums) or of Fractions (exact=True);
    magnitude: absolute values and additions.  Returns (d parking, d driving (Z, T), d pi_next (Z,), parking, driving)."""
    Z, T = p_drive.shape
    conv = _frac if exact else (lambda a: np.asarray(a, dtype=np.float64))
    dtype = object if exact else np.float64
    mag = np.abs if magnitude else (lambda a: a)
    sign = 1 if magnitude else -1
    last, ell, r = tables if tables is not None else R.row_tables(p_dest)
    pre, hours = R.schedule(T, flags)
    on = G.inside(p_drive)
    pi = conv(np.full(Z, 1.0 / Z) if pi0 is None else pi0)
    dpi = conv(mag(np.zeros(Z) if d_pi0 is None else np.asarray(d_pi0, dtype=np.float64)))
    c = abs(float(c)) if magnitude else float(c)
    cc = Fraction(c) if exact else c
    dpark, ddrv = np.empty((Z, T), dtype=dtype), np.empty((Z, T), dtype=dtype)
    park, drv = np.empty((Z, T), dtype=dtype), np.empty((Z, T), dtype=dtype)
    cache = {}
    for s, t in enumerate(hours):
        if t not in cache:
            q = conv(R.clip_q(p_drive[:, t]))
            dq = conv(mag(np.zeros(Z) if d_p_drive is None else np.where(on[:, t], d_p_drive[:, t], 0.0)))
            cache[t] = (q, dq, conv(p_dest[:, :, t]), conv(r[t]), conv(mag(dP[:, :, t])) if c != 0.0 else None)
        q, dq, P, rr, DP = cache[t]
        zero = last[t] == 0.0
        nz = ~zero & (ell[t] >= 0)
        x, dx = pi * q, dpi * q + pi * dq
        if s >= pre:
            park[:, s - pre], drv[:, s - pre], dpark[:, s - pre], ddrv[:, s - pre] = pi, x, dpi, dx
        stay, dstay = pi * (1 - q), dpi * (1 - q) + sign * (pi * dq)
        nxt, dnxt = [], []
        for vec, st in ((x, stay), (dx, dstay)):
            res = np.zeros(Z, dtype=dtype) if not exact else np.array([Fraction(0)] * Z, dtype=object)
            for o in np.flatnonzero(nz):
                res[ell[t][o]] = res[ell[t][o]] + vec[o] * rr[o]
            v = (st + vec @ P) + res
            nxt.append(np.where(zero, v + vec, v))
        pi, dpi = nxt
        if c != 0.0:
            xm = np.where(zero, 0 * x, x)
            dpi = dpi + cc * (xm @ DP)
    return dpark, ddrv, dpi, park, drv


def magnitude(p_drive, p_dest, pi0, flags, d_pi0=None, d_p_drive=None, c=0.0, dP=None, tables=None):
    """(d parking~, d driving~ (Z, T), d pi_next~ (Z,)): object arrays of Fraction, the magnitude recurrence evaluated exactly"""
    return _propagate(p_drive, p_dest, pi0, flags, d_pi0, d_p_drive, c, dP, tables, True, True)[:3]


def numpy_tangent(p_drive, p_dest, pi0, flags, d_pi0=None, d_p_drive=None, c=0.0, dP=None, tables=None, magnitude=False):
    """(d parking, d driving (Z, T), d pi_next (Z,)) in f64; magnitude: the magnitude recurrence in f64 instead"""
    return _propagate(p_drive, p_dest, pi0, flags, d_pi0, d_p_drive, c, dP, tables, magnitude, False)[:3]


def bounds(Z, T, flags):
    """(coefficient of a d parking word per hour of the day (T,), of a d driving word (T,), of a d pi_next word): times the word's
    magnitude, the header's bound"""
    h = np.array(R.operators_behind(T, flags), dtype=np.float64)
    return h * (Z + C2) * EPS, (h * (Z + C2) + 2) * EPS, (h[-1] + 1) * (Z + C2) * EPS


def exact_bounds(Z, T, flags, mags):
    """the three bounds as object arrays / a list of Fraction from magnitude()'s result"""
    bp, bd, bn = bounds(Z, T, flags)
    fp, fd = [Fraction(float(v)) for v in bp], [Fraction(float(v)) for v in bd]
    park, drv = mags[0].copy(), mags[1].copy()
    for t in range(T):
        park[:, t], drv[:, t] = park[:, t] * fp[t], drv[:, t] * fd[t]
    return park, drv, [Fraction(float(bn)) * v for v in mags[2]]


def worst_ratio(got, exact, bound):
    """max over the words of |got - exact| / bound, and whether every word whose bound is 0 -- its magnitude is 0, or nothing has
    been rounded on the way to it -- is the exact value.  got: f64 array; exact, bound: same shape, Fractions (or f64)"""
    worst, exact_ok = Fraction(0), True
    for g, e, b in zip(np.asarray(got).ravel(), np.asarray(exact, dtype=object).ravel(), np.asarray(bound, dtype=object).ravel()):
        if not np.isfinite(g):
            return float("inf"), exact_ok
        e, b = Fraction(e), Fraction(b)
        if b == 0:
            exact_ok = exact_ok and Fraction(float(g)) == e
            continue
        worst = max(worst, abs(Fraction(float(g)) - e) / b)
    return float(worst), exact_ok


def directions(Z, T, K, seed, p_drive=None):
    """K distinct signed directions: (d_pi0 (Z, K), d_p_drive (Z, T, K), both F-order).  Direction 0 moves p_drive only, 1 pi_0 only
    (where K allows), the others both; NaN is planted in the p_drive directions where p_drive is not strictly inside (0, 1)."""
    rng = np.random.default_rng(seed)
    d_pi0 = np.asfortranarray(rng.uniform(-1.0, 1.0, (Z, K)))
    d_pd = np.asfortranarray(rng.uniform(-1.0, 1.0, (Z, T, K)))
    d_pi0[:, 0] = 0.0
    if K > 1:
        d_pd[:, :, 1] = 0.0
    if p_drive is not None:
        d_pd[~G.inside(p_drive)] = np.nan
    return d_pi0, d_pd


# ------------------------------------------------------------------ the planted problem of refine_expected_lm
LM_Z, LM_T, LM_SEED = 12, 6, 11
LM_TRUE = (0.8, 0.15, 0.75)       # (e_drive, p_min, p_max) the measured data are taken from
LM_START = (1.3, 0.05, 0.9)
LM_E_DEST = 2
LM_STEPS = 4
LM_WEIGHTS = {"activity_error": 1.0, "parking_error": 1.0}


def _minmax(v, axis):
    lo, hi = v.min(axis=axis, keepdims=True), v.max(axis=axis, keepdims=True)
    return (v - lo) / (hi - lo)


def lm_problem(O):
    """dict(dm, dist, s (Z, T): createpdrive(0, 1, 1), p_dest, measured_activity (T,), measured_parking (Z, T)): the oracle's synthetic
    datamatrix at Z = 12, T = 6 and the noise-free data of LM_TRUE with the IVP -- F is 0 there"""
    Z, T = LM_Z, LM_T
    dm, dist = O.synth_datamatrix(Z, T, LM_SEED, density=0.5)
    dm, dist = np.asfortranarray(dm), np.asfortranarray(dist)
    s = O.createpdrive(dm, dist, Z, T, 0.0, 1.0, 1.0)
    p_dest = O.createpdestin(dm, Z, T, LM_E_DEST)
    e, lo, hi = LM_TRUE
    parking, driving, _ = R.numpy_expected(lo + (hi - lo) * s ** e, p_dest, None, IVP)
    return dict(dm=dm, dist=dist, s=s, p_dest=p_dest, measured_activity=_minmax(driving.sum(axis=0), 0), measured_parking=_minmax(parking, 1))


def numpy_evaluator(prob):
    """(evaluator, jacobian): what refine_expected_lm needs, in numpy -- numpy_expected plus numpy_tangent on the problem's tables"""
    s, p_dest = prob["s"], prob["p_dest"]
    tables = R.row_tables(p_dest)
    ev = SimpleNamespace(measured_activity=prob["measured_activity"], measured_parking=prob["measured_parking"])

    def jacobian(pt):
        with np.errstate(divide="ignore", invalid="ignore"):
            se = s ** pt.e_drive
            dirs = [(pt.p_max - pt.p_min) * np.where(s > 0, se * np.log(np.where(s > 0, s, 1.0)), 0.0), 1.0 - se, se]
        p_drive = pt.p_min + (pt.p_max - pt.p_min) * se
        parking, driving, _ = R.numpy_expected(p_drive, p_dest, None, IVP, tables)
        dp, dd = zip(*[numpy_tangent(p_drive, p_dest, None, IVP, None, d, tables=tables)[:2] for d in dirs])
        return dict(parking=parking, driving=driving, d_parking=np.array(dp), d_driving=np.array(dd))

    return ev, jacobian
