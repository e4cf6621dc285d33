"""References of the definition in include/cpm_expected_grad.h, computed from the f64 tables (not a conftest: imported by
tests/test_expected_grad.py and tests/test_expected_grad_gpu.py):

  exact_adjoint    the backward pass over fractions.Fraction, built like expected_reference.exact_expected: f64 values are dyadic, so
                   the vectors of a step are put over one power-of-two denominator and the sums run over Python integers -- exact,
                   and fast enough for Z = 67 x 47 operators.  pi_s is the exact forward state, not the device's.
  magnitudes       the same recurrence with |G| in place of G and every difference an addition: lambda~ and D~_s exactly.
  bounds           the header's error bound from the magnitudes.
  numpy_adjoint    the backward pass in numpy f64 (numpy's own order of sums).
  exact_tangent    forward mode over Fractions: the derivative of (parking, driving, pi_next) in a direction (d pi_0, d p_drive).

Tables are the host arrays of the ABI: p_drive (Z, T), p_dest (Z origin, Z dest, T); cotangents g_park, g_drv (Z, T), g_next (Z,)."""
from fractions import Fraction

import numpy as np

import expected_reference as R

EPS = R.EPS
IVP = R.IVP


def segments(Z):
    """(number of destination segments, their length): grad_segments / grad_segment_len of csrc/cpm_expected_grad.h"""
    strips = -(-Z // 128)
    n = max(1, min(-(-1024 // strips), Z // 32, 64))
    return n, -(-Z // n)


def K(Z):
    """twice the roundings behind a term of lambda (include/cpm_expected_grad.h): a chain, the segments and 8 fixed ones"""
    n, seg_len = segments(Z)
    return 2 * (-(-seg_len // 4) + n + 8)


def inside(p_drive):
    """(Z, T) bool: p_drive strictly inside (0, 1) -- elsewhere (NaN included) q is flat and grad_p_drive is exactly 0"""
    with np.errstate(invalid="ignore"):
        return (p_drive > 0.0) & (p_drive < 1.0)


def _trim(v, k):
    g = min(((x & -x).bit_length() - 1) for x in v if x) if any(v) else 0   # (drop common trailing zeros: the ints stay short)
    g = min(g, k)
    return [x >> g for x in v], k - g


def _forward(p_drive, p_dest, pi0, flags, tables):
    """([(ints, k)] pi_s of every operator s, {hour: (P [o, d] ints, r ints, kp, q ints, kq)}), exact"""
    Z, T = p_drive.shape
    last, ell, r = tables
    start = np.full(Z, 1.0 / Z) if pi0 is None else pi0
    pi, kpi = R._dyadic(list(start))
    pre, hours = R.schedule(T, flags)
    states, cache = [], {}
    for s, t in enumerate(hours):
        if t not in cache:
            ints, kp = R._dyadic(np.concatenate([np.ascontiguousarray(p_dest[:, :, t]).ravel(), r[t]]))
            qi, kq = R._dyadic(R.clip_q(p_drive[:, t]))
            cache[t] = (np.array(ints[:Z * Z], dtype=object).reshape(Z, Z), ints[Z * Z:], kp, qi, kq)
        states.append((pi, kpi))
        if s + 1 == len(hours):
            break                                                   # (nothing reads pi_N)
        P, ri, kp, qi, kq = cache[t]
        x = [pi[o] * qi[o] for o in range(Z)]
        nxt = [(pi[o] * ((1 << kq) - qi[o])) << kp for o in range(Z)]
        y = np.array(x, dtype=object) @ P
        for d in range(Z):
            nxt[d] += int(y[d])
        for o in range(Z):
            if last[t][o] == 0.0:
                nxt[o] += x[o] << kp
            elif ell[t][o] >= 0:
                nxt[int(ell[t][o])] += x[o] * ri[o]
        pi, kpi = _trim(nxt, kpi + kq + kp)
    return states, cache


def _backward(p_drive, p_dest, g_park, g_drv, pi0, flags, g_next, tables, magnitude, fwd=None):
    """(dq[s][o] of every operator, lambda after s = 0), Fractions; magnitude: the recurrence of the error bound"""
    Z, T = p_drive.shape
    tables = tables if tables is not None else R.row_tables(p_dest)
    last, ell, _ = tables
    states, cache = fwd if fwd is not None else _forward(p_drive, p_dest, pi0, flags, tables)
    pre, hours = R.schedule(T, flags)
    g_park, g_drv = np.asarray(g_park, dtype=np.float64), np.asarray(g_drv, dtype=np.float64)
    gn = np.zeros(Z) if g_next is None else np.asarray(g_next, dtype=np.float64)
    gi, kg = R._dyadic(list(g_park.T.ravel()) + list(g_drv.T.ravel()) + list(gn))     # [T][Z], [T][Z], [Z]
    if magnitude:
        gi = [abs(v) for v in gi]
    sign = 1 if magnitude else -1
    mu, km = gi[2 * Z * T:], kg
    dq = [None] * len(hours)
    for s in reversed(range(len(hours))):
        t, j = hours[s], s - pre
        P, ri, kp, qi, kq = cache[t]
        y = P @ np.array(mu, dtype=object)                          # scale km + kp
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
        pis, kpi = states[s]
        dq[s] = [Fraction(pis[o] * c[o], 1 << (kpi + S)) for o in range(Z)]
        mu, km = _trim([((gp[o] + mus[o]) << kq) + qi[o] * c[o] for o in range(Z)], S + kq)
    return dq, [Fraction(v, 1 << km) for v in mu]


def exact_adjoint(p_drive, p_dest, g_park, g_drv, pi0=None, flags=0, g_next=None, tables=None, fwd=None):
    """(grad_p_drive: (Z, T) object array of Fraction, grad_pi0: list of Fraction), no rounding"""
    Z, T = p_drive.shape
    dq, lam = _backward(p_drive, p_dest, g_park, g_drv, pi0, flags, g_next, tables, False, fwd)
    _, hours = R.schedule(T, flags)
    on = inside(p_drive)
    grad = np.empty((Z, T), dtype=object)
    for o in range(Z):
        for t in range(T):
            grad[o, t] = sum((dq[s][o] for s in range(len(hours)) if hours[s] == t), Fraction(0)) if on[o, t] else Fraction(0)
    return grad, lam


def magnitudes(p_drive, p_dest, g_park, g_drv, pi0=None, flags=0, g_next=None, tables=None, fwd=None):
    """(D~[s][o] of every operator, lambda~ after s = 0), Fractions: the magnitude recurrence of include/cpm_expected_grad.h"""
    return _backward(p_drive, p_dest, g_park, g_drv, pi0, flags, g_next, tables, True, fwd)


def exact_with_bounds(p_drive, p_dest, g_park, g_drv, pi0=None, flags=0, g_next=None, tables=None):
    """(exact grad_p_drive, exact grad_pi0, their bounds): exact_adjoint, magnitudes and bounds over ONE exact forward pass"""
    tables = tables if tables is not None else R.row_tables(p_dest)
    fwd = _forward(p_drive, p_dest, pi0, flags, tables)
    grad, gpi0 = exact_adjoint(p_drive, p_dest, g_park, g_drv, pi0, flags, g_next, tables, fwd)
    bg, bp = bounds(p_drive, flags, *magnitudes(p_drive, p_dest, g_park, g_drv, pi0, flags, g_next, tables, fwd))
    return grad, gpi0, bg, bp


def bounds(p_drive, flags, Dbar, lam_bar, factor=1):
    """(bound of grad_p_drive (Z, T), bound of grad_pi0 (Z,)), Fractions, absolute: after n backward operators a word of lambda lies
    within n K 2^-52 lambda~, dq_s within ((N - s) K + s (Z + 8) + 4) 2^-52 D~_s; an entry of grad_p_drive within the sum over its
    operators, and 0 where p_drive is not strictly inside (0, 1)"""
    Z, T = p_drive.shape
    _, hours = R.schedule(T, flags)
    N, k, eps = len(hours), K(Z), Fraction(EPS) * factor
    on = inside(p_drive)
    bg = np.empty((Z, T), dtype=object)
    for o in range(Z):
        for t in range(T):
            bg[o, t] = sum((((N - s) * k + s * (Z + 8) + 4) * eps * Dbar[s][o] for s in range(N) if hours[s] == t), Fraction(0)) if on[o, t] else Fraction(0)
    return bg, [N * k * eps * v for v in lam_bar]


def worst_ratio(got, exact, bound):
    """max over the words of |got - exact| / bound, and whether every word whose bound is 0 is 0 (its exact value is).  got: f64
    array; exact, bound: same shape, Fractions (or f64)"""
    got = np.asarray(got)
    exact, bound = np.asarray(exact, dtype=object), np.asarray(bound, dtype=object)
    worst, zeros_ok = Fraction(0), True
    for g, e, b in zip(got.ravel(), exact.ravel(), bound.ravel()):
        e, b = Fraction(e), Fraction(b)
        if b == 0:
            zeros_ok = zeros_ok and g == 0.0 and e == 0
            continue
        if not np.isfinite(g):
            return float("inf"), zeros_ok
        worst = max(worst, abs(Fraction(float(g)) - e) / b)
    return float(worst), zeros_ok


def numpy_adjoint(p_drive, p_dest, g_park, g_drv, pi0=None, flags=0, g_next=None, tables=None, bound_factor=None):
    """(grad_p_drive (Z, T), grad_pi0 (Z,)) in f64.  bound_factor: instead, bound_factor times the header's bounds of the two, from the
    magnitude recurrence evaluated in f64 (for the sizes the exact form is too slow for: its own rounding, parts in 10^13 of a
    bound, is covered by the factor)"""
    Z, T = p_drive.shape
    if bound_factor is not None:
        g_park, g_drv = np.abs(g_park), np.abs(g_drv)
        g_next = None if g_next is None else np.abs(g_next)
    sign = -1.0 if bound_factor is None else 1.0
    last, ell, r = tables if tables is not None else R.row_tables(p_dest)
    pre, hours = R.schedule(T, flags)
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
    mu = np.zeros(Z) if g_next is None else np.asarray(g_next, dtype=np.float64).copy()
    on = inside(p_drive)
    grad = np.zeros((Z, T), order="F")
    for s in reversed(range(len(hours))):
        t, j = hours[s], s - pre
        gp = g_park[:, j] if j >= 0 else np.zeros(Z)
        gd = g_drv[:, j] if j >= 0 else np.zeros(Z)
        nz = (last[t] != 0.0) & (ell[t] >= 0)
        a = p_dest[:, :, t] @ mu + np.where(nz, r[t] * mu[np.where(nz, ell[t], 0)], 0.0)
        a = np.where(last[t] == 0.0, mu, a)
        c = (gd + sign * mu) + a
        coef = 1.0 if bound_factor is None else ((len(hours) - s) * K(Z) + s * (Z + 8) + 4) * EPS * bound_factor
        grad[:, t] = np.where(on[:, t], grad[:, t] + coef * (states[s] * c), 0.0)
        mu = (gp + mu) + R.clip_q(p_drive[:, t]) * c
    return grad, (mu if bound_factor is None else len(hours) * K(Z) * EPS * bound_factor * mu)


def exact_tangent(p_drive, p_dest, pi0, flags, d_pi0, d_p_drive, tables=None):
    """(d parking, d driving: (Z, T) object arrays of Fraction, d pi_next: list of Fraction): the derivative of expected()'s outputs
    in the direction (d_pi0 (Z,), d_p_drive (Z, T)), over Fractions.  q follows p_drive only strictly inside (0, 1).  For small Z."""
    F = Fraction
    Z, T = p_drive.shape
    last, ell, r = tables if tables is not None else R.row_tables(p_dest)
    pre, hours = R.schedule(T, flags)
    on = inside(p_drive)
    pi = [F(float(v)) for v in (np.full(Z, 1.0 / Z) if pi0 is None else pi0)]
    dpi = [F(v) for v in d_pi0]
    dpark, ddrv = np.empty((Z, T), dtype=object), np.empty((Z, T), dtype=object)

    def apply(t, stay, x):
        nxt = list(stay)
        for o in range(Z):
            if last[t][o] == 0.0:
                nxt[o] += x[o]
                continue
            for d in range(Z):
                nxt[d] += x[o] * F(float(p_dest[o, d, t]))
            if ell[t][o] >= 0:
                nxt[int(ell[t][o])] += x[o] * F(float(r[t][o]))
        return nxt

    for s, t in enumerate(hours):
        q = [F(float(v)) for v in R.clip_q(p_drive[:, t])]
        dq = [F(d_p_drive[o][t]) if on[o, t] else F(0) for o in range(Z)]
        x = [pi[o] * q[o] for o in range(Z)]
        dx = [dpi[o] * q[o] + pi[o] * dq[o] for o in range(Z)]
        if s >= pre:
            for o in range(Z):
                dpark[o, s - pre], ddrv[o, s - pre] = dpi[o], dx[o]
        stay = [pi[o] * (1 - q[o]) for o in range(Z)]
        dstay = [dpi[o] * (1 - q[o]) - pi[o] * dq[o] for o in range(Z)]
        pi, dpi = apply(t, stay, x), apply(t, dstay, dx)
    return dpark, ddrv, dpi


def signed_cotangents(Z, T, seed, kind="random"):
    """(g_park, g_drv (Z, T) F-order, g_next (Z,)): signed and random; "single": one non-zero word; "zero": all zero"""
    rng = np.random.default_rng(seed)
    gp, gd, gn = (np.asfortranarray(rng.uniform(-1.0, 1.0, (Z, T))), np.asfortranarray(rng.uniform(-1.0, 1.0, (Z, T))), rng.uniform(-1.0, 1.0, Z))
    if kind == "single":
        keep = gd[Z // 2, T - 1]
        gp[:], gd[:], gn[:] = 0.0, 0.0, 0.0
        gd[Z // 2, T - 1] = keep
    elif kind == "zero":
        gp[:], gd[:], gn[:] = 0.0, 0.0, 0.0
    return gp, gd, gn
