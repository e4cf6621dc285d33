"""Two references of the definition in include/cpm_expected.h, computed from the f64 tables (not a conftest: imported by
tests/test_expected.py and tests/test_expected_gpu.py):

  numpy_expected   the recurrence in numpy f64 (numpy's own order of sums);
  exact_expected   every table entry converted to fractions.Fraction and the recurrence evaluated without rounding.  f64 values are
                   dyadic, so the Fractions of an hour are put over one power-of-two denominator and the sums run over Python
                   integers: exact, and fast enough for Z = 67 x 47 operators.  `last` and `r` are the only f64 operations, as the
                   definition says, and pi_0 = None is the f64 quotient 1.0 / Z that the library starts from.

Tables are the host arrays of the ABI: p_drive (Z, T), p_dest (Z origin, Z dest, T)."""
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -52
IVP = 1  # CPM_EXPECT_IVP


class TableError(ValueError):
    """a non-zero row total exceeds 1 by more than Z * 2^-52: (hour, origin), 1-based"""

    def __init__(self, hour, origin):
        super().__init__(f"row total of hour {hour}, origin {origin} exceeds 1")
        self.hour, self.origin = hour, origin


def clip_q(col):
    """p_drive as the sampler's Bernoulli maps it: NaN and < 0 -> 0, >= 1 -> 1"""
    col = np.asarray(col, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        q = np.where(col > 0.0, col, 0.0)
    return np.minimum(q, 1.0)


def row_tables(p_dest):
    """(last, ell, r), each (T, Z): the f64 left-to-right row total, the last destination with p > 0 (-1: none), max(0, 1 - last)"""
    Z, _, T = p_dest.shape
    last = np.zeros((T, Z))
    ell = np.full((T, Z), -1, dtype=np.int64)
    for t in range(T):
        acc = np.zeros(Z)
        for d in range(Z):
            acc = acc + p_dest[:, d, t]
        last[t] = acc
        pos = p_dest[:, :, t] > 0.0
        has = pos.any(axis=1)
        ell[t, has] = Z - 1 - np.argmax(pos[has, ::-1], axis=1)
    bad = np.argwhere((last != 0.0) & (last > 1.0 + Z * EPS))
    if bad.size:
        raise TableError(int(bad[0][0]) + 1, int(bad[0][1]) + 1)
    return last, ell, np.maximum(0.0, 1.0 - last)


def schedule(T, flags):
    """[(hour of the operator, hour of the day its result is, or None)] -- with IVP the operators of hours 0 .. T-2 come first"""
    pre = T - 1 if (flags & IVP) else 0
    return pre, [(s if s < pre else s - pre) for s in range(pre + T)]


def operators_behind(T, flags):
    """h[t]: operators applied to pi_0 before it became parking[:, t]"""
    pre = T - 1 if (flags & IVP) else 0
    return [pre + t for t in range(T)]


def bound(Z, h):
    """relative bound of a parking word after h operators (include/cpm_expected.h): twice the derived h * (Z + 7) roundings"""
    return h * (Z + 8) * EPS


def bound_driving(Z, h):
    """driving = parking * q is one more rounding: covered by bound() from h = 1 on ((h (Z + 7) + 1) 2^-52 <= h (Z + 8) 2^-52); at
    h = 0 twice that one rounding"""
    return max(h * (Z + 8), 1) * EPS


def numpy_expected(p_drive, p_dest, pi0=None, flags=0, tables=None):
    """(parking (Z, T), driving (Z, T), pi_next (Z,)) in f64"""
    Z, T = p_drive.shape
    last, ell, r = tables if tables is not None else row_tables(p_dest)
    pi = np.full(Z, 1.0 / Z) if pi0 is None else np.asarray(pi0, dtype=np.float64).copy()
    pre, hours = schedule(T, flags)
    parking, driving = np.zeros((Z, T), order="F"), np.zeros((Z, T), order="F")
    for s, t in enumerate(hours):
        q = clip_q(p_drive[:, t])
        x = pi * q
        if s >= pre:
            parking[:, s - pre], driving[:, s - pre] = pi, x
        stay = pi * (1.0 - q)
        y = x @ p_dest[:, :, t]
        res = np.zeros(Z)
        nz = (last[t] != 0.0) & (ell[t] >= 0)
        np.add.at(res, ell[t][nz], (x * r[t])[nz])
        pi = (stay + y) + res + np.where(last[t] == 0.0, x, 0.0)
    return parking, driving, pi


def _dyadic(values):
    """f64 values (or dyadic Fractions) -> (Python ints, k) with value == int / 2**k exactly, through fractions.Fraction"""
    fr = [v if isinstance(v, Fraction) else Fraction(float(v)) for v in values]
    k = max(f.denominator.bit_length() - 1 for f in fr)
    return [f.numerator << (k - (f.denominator.bit_length() - 1)) for f in fr], k


def exact_expected(p_drive, p_dest, pi0=None, flags=0, tables=None):
    """(parking, driving: (Z, T) object arrays of Fraction, pi_next: list of Fraction), no rounding"""
    Z, T = p_drive.shape
    last, ell, r = tables if tables is not None else row_tables(p_dest)
    start = np.full(Z, 1.0 / Z) if pi0 is None else pi0          # (f64, or the Fractions of an earlier day's pi_next)
    pi, kpi = _dyadic(list(start))
    pre, hours = schedule(T, flags)
    parking, driving = np.empty((Z, T), dtype=object), np.empty((Z, T), dtype=object)
    cache = {}
    for s, t in enumerate(hours):
        if t not in cache:
            ints, kp = _dyadic(np.concatenate([np.ascontiguousarray(p_dest[:, :, t]).ravel(), r[t]]))
            qi, kq = _dyadic(clip_q(p_drive[:, t]))
            cache[t] = (np.array(ints[:Z * Z], dtype=object).reshape(Z, Z), ints[Z * Z:], kp, qi, kq)
        P, ri, kp, qi, kq = cache[t]
        x = [pi[o] * qi[o] for o in range(Z)]                     # scale kpi + kq
        if s >= pre:
            for z in range(Z):
                parking[z, s - pre] = Fraction(pi[z], 1 << kpi)
                driving[z, s - pre] = Fraction(x[z], 1 << (kpi + kq))
        nxt = [(pi[o] * ((1 << kq) - qi[o])) << kp for o in range(Z)]  # scale kpi + kq + kp
        y = np.array(x, dtype=object) @ P
        for d in range(Z):
            nxt[d] += int(y[d])
        for o in range(Z):
            if last[t][o] == 0.0:
                nxt[o] += x[o] << kp
            elif ell[t][o] >= 0:
                nxt[int(ell[t][o])] += x[o] * ri[o]
        pi, kpi = nxt, kpi + kq + kp
        g = min(((v & -v).bit_length() - 1) for v in pi if v) if any(pi) else 0  # (drop common trailing zeros: the ints stay short)
        g = min(g, kpi)
        pi, kpi = [v >> g for v in pi], kpi - g
    return parking, driving, [Fraction(v, 1 << kpi) for v in pi]


def worst_ratio(got, exact, tol):
    """max over the words of |got - exact| / (tol * exact), and whether every word whose exact value is 0 is 0.  got: f64 array,
    exact: same shape, Fractions (or f64: compared in Fractions all the same), tol: scalar or array"""
    got, exact = np.asarray(got), np.asarray(exact, dtype=object)
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), got.shape)
    worst, zeros_ok = Fraction(0), True
    for g, e, b in zip(got.ravel(), exact.ravel(), tol.ravel()):
        e = Fraction(e)
        if e == 0:
            zeros_ok = zeros_ok and g == 0.0
            continue
        err = abs(Fraction(float(g)) - e) / e
        if b == 0.0:
            if err != 0:
                return float("inf"), zeros_ok
            continue
        worst = max(worst, err / Fraction(float(b)))
    return float(worst), zeros_ok


def modified_tables(O, Z, T, table_seed=11):
    """the oracle's tables with a zero row, a row scaled by 0.7 in every hour (D1) and a row whose last three entries are 0"""
    p_drive, p_dest = O.synth_p_drive(Z, T, table_seed), O.synth_p_dest_dense(Z, T, table_seed)
    if Z > 7 and T > 5:
        p_dest[3, :, 5] = 0.0
    if Z > 7:
        p_dest[5, :, :] *= 0.7
        p_dest[7, Z - 3:, :] = 0.0
    return p_drive, p_dest
