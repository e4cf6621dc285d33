"""References of the definition in include/cpm_expected_travel_var.h, computed from the f64 tables (not a conftest: imported by
tests/test_expected_travel_var.py and tests/test_expected_travel_var_gpu.py), on top of expected_linear_var_reference and
expected_travel_reference:

  var_sec_mp / v_mp   var_sec and v(a) in mpmath (50 digits) from the f64 words, with the definition's exits;
  v_f64 / var_sec_f64 the documented f64 form of v(a) and var_sec, statement by statement, on the oracle's kit (orc_erf, orc_exp_neg);
  vsec_exact / vsec_numpy   the trip variance weight from a (Z, Z, T) var_sec array: over Fractions, and in f64 in the documented order;
  fraction_tv   the backward recurrence over fractions.Fraction, given v_sec as input; for small Z;
  int_tv        the same over Python integers with explicit binary scales; with bits=53 it asserts that every intermediate, and
                every sum in ANY order of its terms, is exact in f64: the reference of the bit-exact test;
  numpy_tv      the definition in numpy f64 in the documented order of the sums;
  magnitude=True  the magnitude recurrence of the error bound; bounds() the header's bound from it;
  brute_force   mean and variance of L by enumerating every path of one car with the trip reward and the variance of its draws;
  plain_tv      the recurrence with dense numpy sums (no documented order) and the two mutants of the statistical test;
  stat_*        the statistical test of the sampler's spread, shared by the CPU and the GPU test.

Tables are the host arrays of the ABI: p_drive (Z, T), p_dest (Z origin, Z dest, T), sec (Z origin, Z dest, T) and km (Z, Z) as
expected_travel_reference.trip_values returns them (the diagonal selected), v_sec (Z, T).  A functional is (A, B, S, D), each (Z, T).
Results: dict(mean, var, zone_mean, zone_var), zone_* per start zone."""
import math
from fractions import Fraction

import numpy as np

import expected_grad_reference as G
import expected_reference as R
import expected_travel_reference as TR
import expected_var_reference as V
import expected_linear_var_reference as LV

EPS = R.EPS
IVP = R.IVP
NotExact = LV.NotExact
SQRT_HALF = 7.0710678118654752440e-1
SQRT_2_OVER_PI = 7.9788456080286535588e-1
V_BOUND = 2.0 ** -46                       # the header's relative bound of v(a)
SERIES_MAX = 1.0
_FACT = [float(math.factorial(m)) for m in range(18)]


# ------------------------------------------------------------------------------------------------ var_sec
def _sigma(mu, sd_word):
    return 0.1 * mu if sd_word == 0 else sd_word


def v_mp(a):
    """v(a) = 1 - 2 a phi(a) / erf(a / sqrt 2) of the f64 word a > 0, as an mpmath number"""
    import mpmath as mp
    with mp.workdps(60):
        a = mp.mpf(a)
        return +(1 - 2 * a * mp.exp(-a * a / 2) / mp.sqrt(2 * mp.pi) / mp.erf(a / mp.sqrt(2)))


def var_sec_mp(mu, sd_word):
    """sd^2 v(a) in mpmath with the definition's exits (the f64 words sd and a are part of the definition); 0 is the int 0"""
    import mpmath as mp
    mu, sd_word = float(mu), float(sd_word)
    sd = _sigma(mu, sd_word)
    if not sd > 0.0:
        return 0
    a = (0.1 * mu) / sd
    if not a > 0.0:                          # erf of a <= 0 is not > 0: the mass exit
        return 0
    with mp.workdps(60):
        return +(mp.mpf(sd) ** 2 * v_mp(a))


def v_f64(O, a, E):
    """the documented f64 form, statement by statement (csrc/cpm_expected_travel_var.h, etv_v): Python floats are IEEE doubles and
    every line is one operation per step"""
    y = (a * a) * 0.5
    if a <= SERIES_MAX:
        x = -y
        n = 1.0 / (37.0 * _FACT[17])
        m = 1.0 / (35.0 * _FACT[17])
        for k in range(16, -1, -1):
            n = n * x + 1.0 / ((2.0 * k + 3.0) * _FACT[k])
            m = m * x + 1.0 / ((2.0 * k + 1.0) * _FACT[k])
        return ((2.0 * y) * n) / m
    g = ((a * SQRT_2_OVER_PI) * O.lib().orc_exp_neg(y)) / E
    return 1.0 - g


def var_sec_f64(O, mu, sd_word):
    mu, sd_word = float(mu), float(sd_word)
    sd = _sigma(mu, sd_word)
    if not sd > 0.0:
        return 0.0
    a = (0.1 * mu) / sd
    E = O.lib().orc_erf(a * SQRT_HALF)
    if not E > 0.0:
        return 0.0
    return (sd * v_f64(O, a, E)) * sd


def var_sec_array(O, dm, f=None):
    """(Z, Z, T) f64 [origin, destination, hour]: var_sec of every cell, 0 on the diagonal"""
    Z, _, T, _ = dm.shape
    f = f or (lambda mu, sd: var_sec_f64(O, mu, sd))
    out = np.zeros((Z, Z, T), order="F")
    for t in range(T):
        for o in range(Z):
            for d in range(Z):
                if d != o:
                    out[o, d, t] = f(dm[o, d, t, 0], dm[o, d, t, 1])
    return out


def vsec_exact(p_dest, var_sec, tables=None, conv=lambda x: Fraction(float(x))):
    """v_sec as a (Z, T) object array: the sum without rounding; var_sec entries through conv (Fractions, or mpmath numbers)"""
    Z, _, T = p_dest.shape
    last, ell, r = tables if tables is not None else R.row_tables(p_dest)
    out = np.empty((Z, T), dtype=object)
    for t in range(T):
        for o in range(Z):
            if last[t][o] == 0.0:
                out[o, t] = conv(0.0)
                continue
            tot = conv(0.0)
            for d in range(Z):
                if p_dest[o, d, t] != 0.0 and d != o:
                    tot = tot + conv(p_dest[o, d, t]) * var_sec[o][d][t]
            l = int(ell[t][o])
            if l >= 0 and l != o:
                tot = tot + conv(r[t][o]) * var_sec[o][l][t]
            out[o, t] = tot
    return out


def vsec_numpy(p_dest, var_sec, tables=None):
    """v_sec (Z, T) f64 in the documented order: expected_travel_reference.numpy_trip's, with var_sec in place of the seconds"""
    Z, _, T = p_dest.shape
    last, ell, r = tables if tables is not None else R.row_tables(p_dest)
    nseg, seg_len = TR.segments(Z, T)
    o = np.arange(Z)
    out = np.zeros((Z, T), order="F")
    for t in range(T):
        val = var_sec[:, :, t]
        total = None
        for s in range(nseg):
            begin, end = s * seg_len, min((s + 1) * seg_len, Z)
            chains = []
            for v in range(4):
                acc = np.zeros(Z)
                for d in range(begin + v, end, 4):
                    acc = acc + p_dest[:, d, t] * val[:, d]
                chains.append(acc)
            part = ((chains[0] + chains[1]) + chains[2]) + chains[3]
            total = part if total is None else total + part
        has = (last[t] != 0.0) & (ell[t] >= 0)
        l = np.where(has, ell[t], 0)
        total = np.where(has, total + r[t] * val[o, l], total)
        out[:, t] = np.where(last[t] == 0.0, 0.0, total)
    return out


def bound_vsec(Z):
    """the header's relative bound of a word of v_sec"""
    return (Z / 4.0 + 16.0) * EPS + 2.0 ** -45


# ------------------------------------------------------------------------------------------------ the bound
def operators(T, flags):
    return R.schedule(T, flags)


def K2(Z):
    """K' of the header: twice the roundings behind a term of V: those of the linear call and 3 for e and zeta"""
    n, seg_len = G.segments(Z)
    return 2 * (-(-seg_len // 4) + n + 15)


def bounds(Z, T, flags, mag, w=None):
    """the header's absolute bounds from the magnitude recurrence's result mag: dict(mean, var, zone_mean, zone_var)"""
    N = len(operators(T, flags)[1])
    k = K2(Z)
    bv = bound_vsec(Z) + 3 * 2.0 ** -53
    return {"zone_mean": [N * k * EPS * v for v in mag["zone_mean"]], "zone_var": [(2 * N * k * EPS + bv) * v for v in mag["zone_var"]],
            "mean": (N * k + Z + 2) * EPS * mag["mean"], "var": ((2 * N * k + Z + 2) * EPS + bv) * mag["var"]}


worst = LV.worst


def _moves(p_dest, last, ell, r, t, o, Z):
    """[(probability as a Fraction, destination)] of a driver of a non-zero row"""
    m = [(Fraction(float(p_dest[o, d, t])), d) for d in range(Z) if p_dest[o, d, t] != 0.0]
    if ell[t][o] >= 0 and r[t][o] != 0.0:
        m.append((Fraction(float(r[t][o])), int(ell[t][o])))
    return m


# ------------------------------------------------------------------------------------------------ over Fractions
def fraction_tv(p_drive, p_dest, A, B, S, D, sec, km, vsec, w=None, flags=0, tables=None, magnitude=False):
    """vsec: (Z, T) of f64 or Fractions"""
    F = Fraction
    Z, T = p_drive.shape
    last, ell, r = tables if tables is not None else R.row_tables(p_dest)
    pre, hours = operators(T, flags)
    fa = (lambda v: abs(F(float(v)))) if magnitude else (lambda v: F(float(v)))
    fv = lambda v: v if isinstance(v, Fraction) else F(float(v))
    mu, nu = [F(0)] * Z, [F(0)] * Z
    for s in range(len(hours) - 1, -1, -1):
        t, j = hours[s], s - pre
        q = [F(float(v)) for v in R.clip_q(p_drive[:, t])]
        V_, W_ = [], []
        for o in range(Z):
            gp, gd, cs, cd = (fa(A[o, j]), fa(B[o, j]), fa(S[o, j]), fa(D[o, j])) if j >= 0 else (F(0),) * 4
            e = lambda d: cs * fa(sec[o, d, t]) + cd * fa(km[o, d])
            if last[t][o] == 0.0:
                z = cs * F(TR.INTRA_SEC) + cd * F(TR.INTRA_KM)
                s1, s2, b = z, z * z, nu[o]
            else:
                terms = _moves(p_dest, last, ell, r, t, o, Z)
                zeta = (lambda d: (mu[d] + mu[o]) + e(d)) if magnitude else (lambda d: (mu[d] - mu[o]) + e(d))
                s1 = sum((p * zeta(d) for p, d in terms), F(0))
                s2 = sum((p * zeta(d) ** 2 for p, d in terms), F(0))
                b = sum((p * nu[d] for p, d in terms), F(0))
            db = gd + s1
            cv = s2 + s1 * s1 if magnitude else max(F(0), s2 - s1 * s1)
            J = q[o] * ((1 - q[o]) * db * db + cv + cs * cs * fv(vsec[o, t]))
            V_.append(gp + mu[o] + q[o] * db)
            W_.append((1 - q[o]) * nu[o] + q[o] * b + J)
        mu, nu = V_, W_
    ww = [F(1)] * Z if w is None else [F(float(v)) for v in w]
    return {"mean": sum(a * b for a, b in zip(ww, mu)), "var": sum(a * b for a, b in zip(ww, nu)), "zone_mean": mu, "zone_var": nu}


# ------------------------------------------------------------------------------------------------ over integers with binary scales
_trim, _fits = LV._trim, LV._fits


def int_tv(p_drive, p_dest, A, B, S, D, sec, km, vsec, w=None, flags=0, tables=None, magnitude=False, bits=None):
    """fraction_tv's result, exactly, over Python integers.  bits: assert that every intermediate of the recurrence and of the
    totals -- and every partial sum in any order of its terms -- is an integer of at most `bits` bits times a power of two."""
    Z, T = p_drive.shape
    last, ell, r = tables if tables is not None else R.row_tables(p_dest)
    pre, hours = operators(T, flags)
    flat = lambda x: list(np.asarray(x, dtype=np.float64).T.ravel())
    co, kg = R._dyadic(flat(A) + flat(B) + flat(S) + flat(D))
    if magnitude:
        co = [abs(x) for x in co]
    g = lambda which, j, o: co[(which * T + j) * Z + o]
    vs, kvs = R._dyadic([vsec[o, t] for t in range(T) for o in range(Z)])       # (f64 words or dyadic Fractions)
    cache = {}

    def hour(t):
        if t not in cache:
            vals, kp = R._dyadic(list(p_dest[:, :, t].ravel()) + list(r[t]))
            P = [vals[o * Z:(o + 1) * Z] for o in range(Z)]
            qi, kq = R._dyadic(list(R.clip_q(p_drive[:, t])))
            sv, ks = R._dyadic(list(np.ascontiguousarray(sec[:, :, t]).ravel()) + list(np.ascontiguousarray(km).ravel()) + [TR.INTRA_SEC, TR.INTRA_KM])
            if magnitude:
                sv = [abs(x) for x in sv]
            cache[t] = (P, vals[Z * Z:], kp, qi, kq, sv, ks)
        return cache[t]

    mu, km_, nu, kn = [0] * Z, 0, [0] * Z, 0
    for s in range(len(hours) - 1, -1, -1):
        t, j = hours[s], s - pre
        P, ri, kp, q, kq, sv, ks = hour(t)
        ke = kg + ks                              # e
        kz = max(km_, ke)                         # zeta
        kd = max(kg, kp + kz)                     # db
        kv = kq + kd                              # V
        ki1 = kq + 2 * kd                         # (1 - q) db^2 + cv
        ki = max(ki1, 2 * kg + kvs)               # ... + S^2 v_sec
        kw = max(kq + kp + kn, kq + ki)           # W
        Vn, Wn = [], []
        for o in range(Z):
            gp, gd, cs, cd = (g(0, j, o), g(1, j, o), g(2, j, o), g(3, j, o)) if j >= 0 else (0, 0, 0, 0)
            if last[t][o] == 0.0:
                ea, eb = cs * sv[2 * Z * Z], cd * sv[2 * Z * Z + 1]
                _fits([ea, eb], bits, "e")
                z = ea + eb                       # scale ke
                _fits([z * z], bits, "s2")
                s1, s2, b = z << (kp + kz - ke), (z * z) << (kp + 2 * kz - 2 * ke), nu[o] << kp
            else:
                terms = [(P[o][d], d) for d in range(Z) if P[o][d]]
                if ell[t][o] >= 0 and ri[o]:
                    terms.append((ri[o], int(ell[t][o])))
                zeta = []
                for _, d in terms:
                    ea, eb = cs * sv[o * Z + d], cd * sv[Z * Z + o * Z + d]
                    _fits([ea, eb], bits, "e")
                    eta = (mu[d] + mu[o]) if magnitude else (mu[d] - mu[o])
                    za, zb = eta << (kz - km_), (ea + eb) << (kz - ke)
                    _fits([eta], bits, "eta")
                    _fits([za, zb], bits, "zeta")
                    zeta.append(za + zb)
                t1 = [p * e for (p, _), e in zip(terms, zeta)]
                t2 = [x * e for x, e in zip(t1, zeta)]
                tb = [p * nu[d] for p, d in terms]
                for name, tt in (("s1", t1), ("s2", t2), ("b", tb)):
                    for x in tt:
                        _fits([x], bits, name)
                    _fits(tt, bits, name)
                s1, s2, b = sum(t1), sum(t2), sum(tb)     # scales kp + kz, kp + 2 kz, kp + kn
            db = (gd << (kd - kg)) + (s1 << (kd - kp - kz))
            sq = s1 * s1                                  # scale 2 (kp + kz)
            cv = (s2 << kp) + sq if magnitude else max(0, (s2 << kp) - sq)
            dd = db * db
            omq = (1 << kq) - q[o]
            in1, in2 = omq * dd, cv << (ki1 - 2 * (kp + kz))
            ss = cs * cs
            in3 = ss * vs[t * Z + o]                      # scale 2 kg + kvs
            ia, ib = (in1 + in2) << (ki - ki1), in3 << (ki - 2 * kg - kvs)
            J = q[o] * (ia + ib)                          # scale kq + ki
            va, vb, vc = gp << (kv - kg), mu[o] << (kv - km_), q[o] * db
            wa, wb, wc = (omq * nu[o]) << (kw - kq - kn), (q[o] * b) << (kw - kq - kp - kn), J << (kw - kq - ki)
            for name, tt in (("db", [gd << (kd - kg), s1 << (kd - kp - kz)]), ("s1^2", [sq]), ("cv", [s2 << kp, sq]), ("db^2", [dd]),
                             ("J", [in1, in2]), ("S^2", [ss]), ("S^2 v", [in3]), ("J", [ia, ib]), ("J", [J]), ("V", [va, vb, vc]),
                             ("W", [wa, wb, wc])):
                _fits(tt, bits, name)
            Vn.append(va + vb + vc)
            Wn.append(wa + wb + wc)
        both, kk = _trim(Vn + [1 << kv], kv)      # (the trailing 1 keeps the scale an exponent >= 0)
        mu, km_ = both[:Z], kk
        both, kk = _trim(Wn + [1 << kw], kw)
        nu, kn = both[:Z], kk
    wi, kwt = ([1] * Z, 0) if w is None else R._dyadic(list(w))
    tm, tv = [a * b for a, b in zip(wi, mu)], [a * b for a, b in zip(wi, nu)]
    _fits(tm, bits, "mean")
    _fits(tv, bits, "var")
    return {"mean": Fraction(sum(tm), 1 << (km_ + kwt)), "var": Fraction(sum(tv), 1 << (kn + kwt)),
            "zone_mean": [Fraction(x, 1 << km_) for x in mu], "zone_var": [Fraction(x, 1 << kn) for x in nu]}


# ------------------------------------------------------------------------------------------------ numpy, in the documented order
def numpy_tv(p_drive, p_dest, A, B, S, D, sec, km, vsec, w=None, flags=0, tables=None, magnitude=False):
    """f64, every step one IEEE operation, the sums in the order of include/cpm_expected_travel_var.h"""
    Z, T = p_drive.shape
    last, ell, r = tables if tables is not None else R.row_tables(p_dest)
    pre, hours = operators(T, flags)
    nseg, seg_len = G.segments(Z)
    A, B, S, D = (np.asarray(x, dtype=np.float64) for x in (A, B, S, D))
    vsec = np.asarray(vsec, dtype=np.float64)
    if magnitude:
        A, B, S, D, sec, km = (np.abs(x) for x in (A, B, S, D, sec, km))
    oz = np.arange(Z)
    mu, nu = np.zeros(Z), np.zeros(Z)
    for s in range(len(hours) - 1, -1, -1):
        t, j = hours[s], s - pre
        gp, gd, cs, cd = (A[:, j], B[:, j], S[:, j], D[:, j]) if j >= 0 else (np.zeros(Z),) * 4
        q = R.clip_q(p_drive[:, t])
        p = p_dest[:, :, t]
        sec_t = sec[:, :, t]
        zeta_of = lambda d: ((mu[d] + mu) if magnitude else (mu[d] - mu)) + (cs * sec_t[oz, d] + cd * km[oz, d])
        s1, s2, b = np.zeros(Z), np.zeros(Z), np.zeros(Z)
        for sg in range(nseg):
            begin, end = sg * seg_len, min(Z, (sg + 1) * seg_len)
            c1, c2, cb = np.zeros((4, Z)), np.zeros((4, Z)), np.zeros((4, Z))
            for d in range(begin, end):
                c = (d - begin) % 4
                e = zeta_of(d)
                tt = p[:, d] * e
                c1[c] = c1[c] + tt
                c2[c] = c2[c] + tt * e
                cb[c] = cb[c] + p[:, d] * nu[d]
            f = lambda x: ((x[0] + x[1]) + x[2]) + x[3]
            s1, s2, b = (f(c1), f(c2), f(cb)) if sg == 0 else (s1 + f(c1), s2 + f(c2), b + f(cb))
        has = (last[t] != 0.0) & (ell[t] >= 0)
        l = np.where(has, ell[t], 0)
        el = zeta_of(l)
        tl = r[t] * el
        s1 = np.where(has, s1 + tl, s1)
        s2 = np.where(has, s2 + tl * el, s2)
        b = np.where(has, b + r[t] * nu[l], b)
        zero = last[t] == 0.0
        z0 = cs * TR.INTRA_SEC + cd * TR.INTRA_KM
        s1, s2, b = np.where(zero, z0, s1), np.where(zero, z0 * z0, s2), np.where(zero, nu, b)
        omq = 1.0 - q
        db = gd + s1
        cv = s2 + s1 * s1 if magnitude else np.maximum(s2 - s1 * s1, 0.0)
        J = q * ((omq * (db * db) + cv) + (cs * cs) * vsec[:, t])
        mu, nu = (gp + mu) + q * db, (omq * nu + q * b) + J
    return {"mean": LV._total(w, mu), "var": LV._total(w, nu), "zone_mean": mu, "zone_var": nu}


# ------------------------------------------------------------------------------------------------ dense sums, and the mutants
def plain_tv(p_drive, p_dest, A, B, S, D, sec, km, vsec, w=None, flags=0, tables=None, mutant=None):
    """The recurrence with numpy's own sums (the statistical test asks for no bits).  mutant "no_draw" drops S^2 v_sec; "no_cov" forms
    s2 from eta alone and adds the spread of e separately: var(eta) + var(e) in place of var(eta + e), which drops the covariance
    between where the trip ends and how long it takes."""
    Z, T = p_drive.shape
    last, ell, r = tables if tables is not None else R.row_tables(p_dest)
    pre, hours = operators(T, flags)
    mu, nu = np.zeros(Z), np.zeros(Z)
    oz = np.arange(Z)
    for s in range(len(hours) - 1, -1, -1):
        t, j = hours[s], s - pre
        gp, gd, cs, cd = (A[:, j], B[:, j], S[:, j], D[:, j]) if j >= 0 else (np.zeros(Z),) * 4
        q = R.clip_q(p_drive[:, t])
        P = np.array(p_dest[:, :, t], dtype=np.float64)
        has = (last[t] != 0.0) & (ell[t] >= 0)
        P[oz[has], ell[t][has]] += r[t][has]
        zero = last[t] == 0.0
        P[zero, :] = 0.0
        P[oz[zero], oz[zero]] = 1.0
        e = cs[:, None] * sec[:, :, t] + cd[:, None] * km
        eta = mu[None, :] - mu[:, None]
        zeta = eta + e
        s1 = (P * zeta).sum(axis=1)
        if mutant == "no_cov":
            m_eta, m_e = (P * eta).sum(axis=1), (P * e).sum(axis=1)
            cv = (P * (eta - m_eta[:, None]) ** 2).sum(axis=1) + (P * (e - m_e[:, None]) ** 2).sum(axis=1)
        else:
            cv = (P * (zeta - s1[:, None]) ** 2).sum(axis=1)
        b = P @ nu
        db = gd + s1
        draw = 0.0 if mutant == "no_draw" else (cs * cs) * vsec[:, t]
        J = q * (((1.0 - q) * (db * db) + cv) + draw)
        mu, nu = (gp + mu) + q * db, ((1.0 - q) * nu + q * b) + J
    ww = np.ones(Z) if w is None else np.asarray(w, dtype=np.float64)
    return {"mean": float(ww @ mu), "var": float(ww @ nu), "zone_mean": mu, "zone_var": nu}


# ------------------------------------------------------------------------------------------------ every path of one car
def brute_force(p_drive, p_dest, A, B, S, D, sec, km, var_sec, w=None, flags=0, tables=None):
    """(mean, var) of L as Fractions by enumerating every path of one car from each start zone.  A path's reward holds the mean seconds
    of its trips; the draws are independent given the path, with mean sec and variance var_sec[o, d, t] (a (Z, Z, T) array of f64
    or Fractions), so var = var over the paths of the reward + the mean over the paths of sum S^2 var_sec (the law of total
    variance).  The last operator's destination is sampled and its trip counted, though its state is never applied."""
    F = Fraction
    Z, T = p_drive.shape
    last, ell, r = tables if tables is not None else R.row_tables(p_dest)
    pre, hours = operators(T, flags)
    N = len(hours)
    fv = lambda v: v if isinstance(v, Fraction) else F(float(v))

    def moves(t, o):
        if last[t][o] == 0.0:
            return [(F(1), o)]
        m = _moves(p_dest, last, ell, r, t, o, Z)
        assert sum(p for p, _ in m) == 1, "the row's law does not sum to 1: no probability space to enumerate"
        return m

    def walk(s, o, prob, reward, noise, acc):
        if s == N:
            acc[0] += prob * reward
            acc[1] += prob * reward * reward
            acc[2] += prob * noise
            return
        t, j = hours[s], s - pre
        gp, gd, cs, cd = (F(float(x[o, j])) for x in (A, B, S, D)) if j >= 0 else (F(0),) * 4
        q = F(float(R.clip_q(p_drive[:, t])[o]))
        if q != 1:
            walk(s + 1, o, prob * (1 - q), reward + gp, noise, acc)
        if q != 0:
            for p, d in moves(t, o):
                same = d == o
                e = cs * (F(TR.INTRA_SEC) if same else F(float(sec[o, d, t]))) + cd * (F(TR.INTRA_KM) if same else F(float(km[o, d])))
                vn = F(0) if same else cs * cs * fv(var_sec[o][d][t])
                walk(s + 1, d, prob * q * p, reward + gp + gd + e, noise + vn, acc)

    mean, var = F(0), F(0)
    for z in range(Z):
        wz = F(1) if w is None else F(float(w[z]))
        acc = [F(0), F(0), F(0)]
        walk(0, z, F(1), F(0), F(0), acc)
        mean += wz * acc[0]
        var += wz * (acc[1] - acc[0] ** 2 + acc[2])
    return mean, var


# ------------------------------------------------------------------------------------------------ functionals and tables
def signed_functionals(Z, T, K, seed):
    """K functionals: four (Z, T, K) F-order arrays A, B in -1 .. 1, S in -1e-3 .. 1e-3 (per second) and D in -0.1 .. 0.1 (per km)"""
    rng = np.random.default_rng(seed)
    u = lambda s: np.asfortranarray(rng.uniform(-s, s, (Z, T, K)))
    return u(1.0), u(1.0), u(1e-3), u(0.1)


def small_functionals(Z, T, K, seed):
    """integer coefficients: A, B in -2 .. 2, S and D in -1 .. 1"""
    rng = np.random.default_rng(seed)
    i = lambda lo, hi: np.asfortranarray(rng.integers(lo, hi + 1, (Z, T, K)).astype(np.float64))
    return i(-2, 2), i(-2, 2), i(-1, 1), i(-1, 1)


def dyadic_datamatrix(Z, T, seed=3):
    """(dm (Z, Z, T, 2), dist (Z, Z)): means in 1 .. 8 and distances in 0.5 .. 4 in steps of 1/2, every standard deviation negative
    (var_sec is exactly 0), and a diagonal that is NOT 300 s / 1 km: the select shows wherever p[o, o] > 0"""
    rng = np.random.default_rng(seed + Z)
    dm = np.zeros((Z, Z, T, 2), order="F")
    dm[..., 0] = rng.integers(2, 17, (Z, Z, T)) / 2.0
    dm[..., 1] = -1.0
    dist = np.asfortranarray(rng.integers(1, 9, (Z, Z)) / 2.0)
    return dm, dist


def stack4(funcs):
    """[(name, A, B, S, D)] -> the four (Z, T, K) arrays of Sampler.expected_travel_var"""
    return tuple(np.asfortranarray(np.stack([f[i] for f in funcs], axis=2)) for i in (1, 2, 3, 4))


# ------------------------------------------------------------------------------------------------ the statistical test
STAT_Z, STAT_T, STAT_CPZ, RUNS = V.STAT_Z, V.STAT_T, V.STAT_CPZ, V.RUNS


def stat_setup(O):
    """The tables of expected_linear_var_reference.stat_setup (p_drive in 0.2 .. 0.5) with the datamatrix they were built from, its
    standard deviations at 0.25 .. 0.4 of the mean where the generator gives them (a window of +-0.25 .. 0.4 sigma)."""
    p_drive, p_dest, zone0, w = LV.stat_setup(O)
    dm, dist = O.synth_datamatrix(STAT_Z, STAT_T, 11, 0.6)
    return p_drive, p_dest, zone0, w, np.asfortranarray(dm), np.asfortranarray(dist)


def draw_only_setup(O):
    """Tables on which ALL noise of the travel seconds is draw noise: p_drive = 1, every row sends its driver to ONE other zone, every
    mean is 1,000 s and every standard deviation 100 s (a = 1): var = C * T * sd^2 * v(1), and the mutant without S^2 v_sec gives 0."""
    Z, T = STAT_Z, STAT_T
    p_drive = np.ones((Z, T), order="F")
    p_dest = np.zeros((Z, Z, T), order="F")
    for t in range(T):
        for o in range(Z):
            p_dest[o, (o + 1 + t) % Z if (o + 1 + t) % Z != o else (o + 2 + t) % Z, t] = 1.0
    dm = np.zeros((Z, Z, T, 2), order="F")
    dm[..., 0], dm[..., 1] = 1000.0, 100.0
    dist = np.asfortranarray(np.full((Z, Z), 5.0))
    zone0 = np.repeat(np.arange(1, Z + 1), STAT_CPZ).astype(np.int64)
    return p_drive, p_dest, zone0, np.full(Z, float(STAT_CPZ)), dm, dist


def cov_setup(O):
    """Tables on which the covariance between where a trip ends and how long it takes is half of the variance: p_drive = 1 (no
    Bernoulli noise), every other zone equally likely, no draw noise (negative standard deviations), and seconds(o, d) =
    600 * (1 + h[o] + h[d]).  The value of being in d is then 600 * h[d] + a constant, eta[d] = 600 * (h[d] - h[o]) moves with
    e[d] = 600 * (1 + h[o] + h[d]), var(eta + e) = 4 * 600^2 var(h), and var(eta) + var(e) is half of it."""
    Z, T = STAT_Z, STAT_T
    p_drive = np.ones((Z, T), order="F")
    p_dest = np.zeros((Z, Z, T), order="F")
    p_dest[:, :, :] = 1.0 / (Z - 1)
    z = np.arange(Z)
    p_dest[z, z, :] = 0.0
    h = np.linspace(0.0, 1.0, Z)
    dm = np.zeros((Z, Z, T, 2), order="F")
    dm[..., 0] = (600.0 * (1.0 + h[:, None] + h[None, :]))[:, :, None]
    dm[..., 1] = -1.0
    dist = np.asfortranarray(np.full((Z, Z), 5.0))
    zone0 = np.repeat(np.arange(1, Z + 1), STAT_CPZ).astype(np.int64)
    return p_drive, p_dest, zone0, np.full(Z, float(STAT_CPZ)), dm, dist


def stat_functionals(Z, T, seed=3):
    """[(name, A, B, S, D)]: the total seconds, and the total seconds plus a random signed count functional whose spread is of the
    same order (its coefficients are scaled by the mean seconds of a trip)"""
    zero, one = np.zeros((Z, T), order="F"), np.ones((Z, T), order="F")
    A, B = LV.signed_functionals(Z, T, 1, seed)
    return [("seconds", zero, zero, one, zero), ("seconds_and_counts", np.asfortranarray(1000.0 * A[:, :, 0]), np.asfortranarray(1000.0 * B[:, :, 0]), one, zero)]


def stat_values(runs, funcs):
    """(runs, K): L of every run (parking, driving, seconds); the functionals here weigh the run's total seconds by S = 1"""
    return np.array([[float((A * park).sum() + (B * drv).sum()) + sec for _, A, B, _, _ in funcs] for park, drv, sec in runs])


def check_stat(L, mean, var, label, mutants=()):
    """the cap of expected_linear_var_reference.stat_within_cap, functional by functional; mutants: [(name, k, variances)] must lie
    outside the cap of functional k -- asserted from the numbers before the sample is looked at -- and fail"""
    K = L.shape[1]
    halves = []
    for k in range(K):
        ok, m, half = LV.stat_within_cap(L, mean, var, [k])
        halves.append(half)
        print(f"{label}: functional {k}: exact {m:.4f} +- {half:.4f}")
        assert ok, f"the exact variance misses the cap for functional {k}"
    for name, k, mv in mutants:
        ratio = float(var[k] / mv[k]) if mv[k] > 0 else math.inf       # what the mutant's statistic tends to
        assert abs(ratio - 1.0) > 2.0 * halves[k], f"the tables put the mutant {name} ({ratio:.3f}) inside the cap: choose others"
        if mv[k] > 0:
            okm, mm, halfm = LV.stat_within_cap(L, mean, mv, [k])
            print(f"{label}: functional {k}: mutant {name} {mm:.4f} +- {halfm:.4f} (tends to {ratio:.3f})")
            assert not okm, f"the mutant {name} passes the cap for functional {k}"
        else:
            print(f"{label}: functional {k}: mutant {name} has variance 0")
            assert L[:, k].std() > 0
