"""References of the definitions in include/cpm_expected_grad_dest.h, computed from the f64 tables (not a conftest: imported by
tests/test_expected_grad_dest.py and tests/test_expected_grad_dest_gpu.py):

  exact_adjoint_dest   the backward pass of expected_grad_reference with the w terms, over fractions.Fraction (dyadic ints): grad_dest,
                       and with it grad_p_drive and grad_pi0; `magnitude`: the recurrence of the error bound with |G| and |dP|.
  bounds_dest          the header's bound on grad_dest from the magnitudes.
  numpy_adjoint_dest   the backward pass in numpy f64 with the sums a and w in the documented order (segments, four chains).
  exact_tangent_dest   forward mode over Fractions: (pi, d pi) propagated under p -> p + eps * dP with r and l fixed.
  e_dest_x, tangent_mp the f64 x createpdestin forms, and the tangent's definition in mpmath (60 digits) from x and the installed p.
  exact_trip_tangent   the tangent of the trip weights over Fractions, and its bound.

Tables are the host arrays of the ABI: p_drive (Z, T), p_dest and dP (Z origin, Z dest, T); cotangents (Z, T), g_next (Z,)."""
from fractions import Fraction

import mpmath
import numpy as np

import expected_reference as R
import expected_grad_reference as G
import expected_travel_reference as TR

EPS = R.EPS
mpmath.mp.dps = 60


def _backward(p_drive, p_dest, dP, g_park, g_drv, pi0, flags, g_next, tables, magnitude, fwd=None):
    """(dq[s][o], lambda after s = 0, gdest[s][o]), Fractions: expected_grad_reference._backward with
    gdest_s[o] = (pi_s[o] q[o]) * sum_d dP[o, d, t] mu[d], 0 for a zero row, no residual term"""
    Z, T = p_drive.shape
    last, ell, _ = tables
    states, cache = fwd if fwd is not None else G._forward(p_drive, p_dest, pi0, flags, tables)
    pre, hours = R.schedule(T, flags)
    g_park, g_drv = np.asarray(g_park, dtype=np.float64), np.asarray(g_drv, dtype=np.float64)
    gn = np.zeros(Z) if g_next is None else np.asarray(g_next, dtype=np.float64)
    gi, kg = R._dyadic(list(g_park.T.ravel()) + list(g_drv.T.ravel()) + list(gn))
    if magnitude:
        gi = [abs(v) for v in gi]
    sign = 1 if magnitude else -1
    mu, km = gi[2 * Z * T:], kg
    dq, gdest, tan = [None] * len(hours), [None] * len(hours), {}
    for s in reversed(range(len(hours))):
        t, j = hours[s], s - pre
        P, ri, kp, qi, kq = cache[t]
        if t not in tan:
            di, kd = R._dyadic(np.ascontiguousarray(dP[:, :, t]).ravel())
            if magnitude:
                di = [abs(v) for v in di]
            tan[t] = (np.array(di, dtype=object).reshape(Z, Z), kd)
        D, kd = tan[t]
        muv = np.array(mu, dtype=object)
        y, w = P @ muv, D @ muv                                      # scales km + kp, km + kd
        pis, kpi = states[s]
        gdest[s] = [Fraction(0) if last[t][o] == 0.0 else Fraction(pis[o] * qi[o] * int(w[o]), 1 << (kpi + kq + kd + km)) for o in range(Z)]
        a = []
        for o in range(Z):
            if last[t][o] == 0.0:
                a.append(mu[o] << kp)
            else:
                a.append(int(y[o]) + (ri[o] * mu[int(ell[t][o])] if ell[t][o] >= 0 else 0))
        S = max(kg, km + kp)
        gp = [gi[j * Z + o] << (S - kg) for o in range(Z)] if j >= 0 else [0] * Z
        gd = [gi[Z * T + j * Z + o] << (S - kg) for o in range(Z)] if j >= 0 else [0] * Z
        mus = [m << (S - km) for m in mu]
        c = [gd[o] + sign * mus[o] + (a[o] << (S - km - kp)) for o in range(Z)]
        dq[s] = [Fraction(pis[o] * c[o], 1 << (kpi + S)) for o in range(Z)]
        mu, km = G._trim([((gp[o] + mus[o]) << kq) + qi[o] * c[o] for o in range(Z)], S + kq)
    return dq, [Fraction(v, 1 << km) for v in mu], gdest


def _per_hour(terms, Z, T, flags, weight=None):
    _, hours = R.schedule(T, flags)
    out = np.empty((Z, T), dtype=object)
    for o in range(Z):
        for t in range(T):
            out[o, t] = sum(((weight(s) if weight else 1) * terms[s][o] for s in range(len(hours)) if hours[s] == t), Fraction(0))
    return out


def bound_weight(Z, N, s):
    """the factor of 2^-52 * W~_s in the header's bound: n K + s (Z + 8) + 4 with n = N - s"""
    return (N - s) * G.K(Z) + s * (Z + 8) + 4


def exact_adjoint_dest(p_drive, p_dest, dP, g_park, g_drv, pi0=None, flags=0, g_next=None, tables=None):
    """(grad_dest exact, its bound, grad_p_drive exact, grad_pi0 exact): (Z, T) object arrays of Fraction (grad_pi0 a list), over ONE
    exact forward pass"""
    Z, T = p_drive.shape
    tables = tables if tables is not None else R.row_tables(p_dest)
    fwd = G._forward(p_drive, p_dest, pi0, flags, tables)
    dq, lam, gdest = _backward(p_drive, p_dest, dP, g_park, g_drv, pi0, flags, g_next, tables, False, fwd)
    _, _, wbar = _backward(p_drive, p_dest, dP, g_park, g_drv, pi0, flags, g_next, tables, True, fwd)
    N = len(R.schedule(T, flags)[1])
    on = G.inside(p_drive)
    grad = _per_hour(dq, Z, T, flags)
    for o in range(Z):
        for t in range(T):
            if not on[o, t]:
                grad[o, t] = Fraction(0)
    bound = _per_hour(wbar, Z, T, flags, lambda s: bound_weight(Z, N, s) * Fraction(EPS))
    return _per_hour(gdest, Z, T, flags), bound, grad, lam


def _ordered_product(M, mu, Z):
    """sum over d of M[:, d] * mu[d] in the order of include/cpm_expected_grad.h: segments, chain (d - begin) mod 4 ascending from 0,
    ((c0 + c1) + c2) + c3, the segments in ascending order"""
    nseg, seg_len = G.segments(Z)
    total = None
    for sg in range(nseg):
        begin, end = sg * seg_len, min((sg + 1) * seg_len, Z)
        chains = []
        for c in range(4):
            acc = np.zeros(Z)
            for d in range(begin + c, end, 4):
                acc = acc + M[:, d] * mu[d]
            chains.append(acc)
        seg = ((chains[0] + chains[1]) + chains[2]) + chains[3]
        total = seg if total is None else total + seg
    return total


def numpy_adjoint_dest(p_drive, p_dest, dP, g_park, g_drv, pi0=None, flags=0, g_next=None, tables=None, bound_factor=None):
    """(grad_dest, grad_p_drive (Z, T), grad_pi0 (Z,)) in f64, one operation per step, a and w in the documented order (pi_s from
    numpy's own forward pass).  bound_factor: instead of grad_dest, bound_factor times the header's bound of it, from the magnitude
    recurrence evaluated in f64 (its own rounding, parts in 10^13 of a bound, is covered by the factor)."""
    Z, T = p_drive.shape
    mag = bound_factor is not None
    if mag:
        g_park, g_drv, dP = np.abs(g_park), np.abs(g_drv), np.abs(dP)
        g_next = None if g_next is None else np.abs(g_next)
    sign = 1.0 if mag else -1.0
    last, ell, r = tables if tables is not None else R.row_tables(p_dest)
    pre, hours = R.schedule(T, flags)
    N = len(hours)
    pi = np.full(Z, 1.0 / Z) if pi0 is None else np.asarray(pi0, dtype=np.float64).copy()
    states = []
    for s, t in enumerate(hours):
        states.append(pi)
        q = R.clip_q(p_drive[:, t])
        x = pi * q
        res = np.zeros(Z)
        nz = (last[t] != 0.0) & (ell[t] >= 0)
        np.add.at(res, ell[t][nz], (x * r[t])[nz])
        pi = (pi * (1.0 - q) + x @ p_dest[:, :, t]) + res + np.where(last[t] == 0.0, x, 0.0)
    with_mu = g_next is not None
    mu = np.zeros(Z) if g_next is None else np.asarray(g_next, dtype=np.float64).copy()
    on = G.inside(p_drive)
    grad, gdest = np.zeros((Z, T), order="F"), np.zeros((Z, T), order="F")
    for s in reversed(range(N)):
        t, j = hours[s], s - pre
        gp = g_park[:, j] if j >= 0 else np.zeros(Z)
        gd = g_drv[:, j] if j >= 0 else np.zeros(Z)
        q = R.clip_q(p_drive[:, t])
        if with_mu:
            nz = (last[t] != 0.0) & (ell[t] >= 0)
            a = _ordered_product(p_dest[:, :, t], mu, Z)
            a = np.where(nz, a + r[t] * mu[np.where(nz, ell[t], 0)], a)
            a = np.where(last[t] == 0.0, mu, a)
            w = np.where(last[t] == 0.0, 0.0, _ordered_product(dP[:, :, t], mu, Z))
        else:                                                       # mu is zero by construction: the products are skipped
            a, w = np.zeros(Z), np.zeros(Z)
        c = (gd + sign * mu) + a
        dq = states[s] * c
        term = (states[s] * q) * w
        if mag:
            term = bound_weight(Z, N, s) * EPS * bound_factor * term
        first = s >= pre                                            # the day's term is stored, the IVP's added to it
        grad[:, t] = np.where(on[:, t], dq if first else grad[:, t] + dq, 0.0)
        gdest[:, t] = term if first else gdest[:, t] + term
        mu = (gp + mu) + q * c
        with_mu = True
    return gdest, grad, mu


def exact_tangent_dest(p_drive, p_dest, dP, pi0, flags, tables=None):
    """(d parking, d driving: (Z, T) object arrays of Fraction, d pi_next: list): the derivative of expected()'s outputs under
    p_destin -> p_destin + eps * dP at eps = 0, with r and l held fixed (a zero row stays a zero row), over Fractions.  For small Z."""
    F = Fraction
    Z, T = p_drive.shape
    last, ell, r = tables if tables is not None else R.row_tables(p_dest)
    pre, hours = R.schedule(T, flags)
    pi = [F(float(v)) for v in (np.full(Z, 1.0 / Z) if pi0 is None else pi0)]
    dpi = [F(0)] * Z
    dpark, ddrv = np.empty((Z, T), dtype=object), np.empty((Z, T), dtype=object)
    for s, t in enumerate(hours):
        q = [F(float(v)) for v in R.clip_q(p_drive[:, t])]
        x, dx = [pi[o] * q[o] for o in range(Z)], [dpi[o] * q[o] for o in range(Z)]
        if s >= pre:
            for o in range(Z):
                dpark[o, s - pre], ddrv[o, s - pre] = dpi[o], dx[o]
        nxt, dnxt = [pi[o] * (1 - q[o]) for o in range(Z)], [dpi[o] * (1 - q[o]) for o in range(Z)]
        for o in range(Z):
            if last[t][o] == 0.0:
                nxt[o] += x[o]
                dnxt[o] += dx[o]
                continue
            for d in range(Z):
                pv = F(float(p_dest[o, d, t]))
                nxt[d] += x[o] * pv
                dnxt[d] += dx[o] * pv + x[o] * F(float(dP[o, d, t]))
            if ell[t][o] >= 0:
                rv = F(float(r[t][o]))
                nxt[int(ell[t][o])] += x[o] * rv
                dnxt[int(ell[t][o])] += dx[o] * rv
        pi, dpi = nxt, dnxt
    return dpark, ddrv, dpi


def signed_tangent(p_dest, seed):
    """a signed random dP in [-1, 1), rows NOT summing to 0, non-zero on a zero row as well (the library must ignore it there)"""
    return np.asfortranarray(np.random.default_rng(seed).uniform(-1.0, 1.0, p_dest.shape))


# ------------------------------------------------------------------ d p_destin / d e_dest
def e_dest_x(dm):
    """(Z, Z, T) f64: x = (mean - min_t) / (max_t - min_t) for pairs with max_t > 0, else 0 -- one IEEE operation per step, the value
    createpdestin forms (src/createpdestin.jl:10-28)"""
    mean = np.asarray(dm[:, :, :, 0], dtype=np.float64)
    mx, mn = mean.max(axis=2, keepdims=True), mean.min(axis=2, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        x = (mean - mn) / (mx - mn)
    return np.where(mx > 0, x, 0.0)


def tangent_mp(x_row, p_row):
    """(dP, bound) of one (origin, hour) row from its f64 x and installed f64 p, lists over the destinations: mpmath values of
    p * (ln x - sum p ln x) over the cells with p > 0 (0 elsewhere), and (n + 8) 2^-52 p (|l| + m~)"""
    idx = [d for d in range(len(p_row)) if p_row[d] > 0.0]
    l = {d: mpmath.log(mpmath.mpf(float(x_row[d]))) for d in idx}
    m = mpmath.fsum(mpmath.mpf(float(p_row[d])) * l[d] for d in idx)
    mbar = mpmath.fsum(mpmath.mpf(float(p_row[d])) * abs(l[d]) for d in idx)
    dP, bound = [mpmath.mpf(0)] * len(p_row), [mpmath.mpf(0)] * len(p_row)
    for d in idx:
        p = mpmath.mpf(float(p_row[d]))
        dP[d] = p * (l[d] - m)
        bound[d] = (len(idx) + 8) * mpmath.mpf(EPS) * p * (abs(l[d]) + mbar)
    return dP, bound


def p_of_e_mp(x_row, e):
    """x^e / sum x^e of one row in mpmath (x == 0 cells are 0; e > 0)"""
    w = [mpmath.power(mpmath.mpf(float(v)), e) if v > 0.0 else mpmath.mpf(0) for v in x_row]
    tot = mpmath.fsum(w)
    return [v / tot for v in w] if tot > 0 else w


# ------------------------------------------------------------------ the tangent of the trip weights
def exact_trip_tangent(dP, dm, dist, tables):
    """(dw_sec, dw_km, bound_sec, bound_km): (Z, T) object arrays of Fraction -- sum over d of dP * value, 0 for a zero row, no residual
    term; the bound is (Z / 4 + 16) 2^-52 sum |dP| |value|"""
    Z, _, T = dP.shape
    last = tables[0]
    sec, km = TR.trip_values(dm, dist)
    F = lambda v: Fraction(float(v))
    out = [np.empty((Z, T), dtype=object) for _ in range(4)]
    coef = (Fraction(Z, 4) + 16) * Fraction(EPS)
    for t in range(T):
        for which, val in ((0, sec[:, :, t]), (1, km)):
            for o in range(Z):
                zero = last[t][o] == 0.0
                terms = [F(dP[o, d, t]) * F(val[o, d]) for d in range(Z)]
                out[which][o, t] = Fraction(0) if zero else sum(terms, Fraction(0))
                out[2 + which][o, t] = Fraction(0) if zero else coef * sum((abs(v) for v in terms), Fraction(0))
    return tuple(out)
