"""References of the definition in include/cpm_expected_linear_var.h, computed from the f64 tables (not a conftest: imported by
tests/test_expected_linear_var.py and tests/test_expected_linear_var_gpu.py):

  fraction_lv   the backward recurrence over fractions.Fraction with the sampler's exact law (r and the row total are the f64 words
                of the installed table, as the definition says), no rounding; for small Z;
  int_lv        the same over Python integers with explicit binary scales (every f64 is dyadic): the exact form for the larger
                sizes, and, with bits=53, the reference of the bit-exact test -- it asserts that every intermediate, and every sum in
                ANY order of its terms, is exact in f64;
  numpy_lv      the definition in numpy f64 in the documented order of the sums;
  magnitude=True  the magnitude recurrence of the error bound; bounds() the header's bound from it;
  brute_force   mean and variance of L by enumerating every path of one car, for tiny chains whose rows (with r) sum to 1 exactly;
  raw_moment_lv the mutant with raw moments sum p mu^2 - (sum p mu)^2 in place of the centred sums;
  stat_*        the statistical test of the sampler's spread, shared by the CPU and the GPU test.

Tables are the host arrays of the ABI: p_drive (Z, T), p_dest (Z origin, Z dest, T).  A functional is (A, B), each (Z, T).  Results:
dict(mean, var, zone_mean, zone_var), zone_* per start zone."""
from fractions import Fraction

import numpy as np

import expected_grad_reference as G
import expected_reference as R
import expected_var_reference as V

EPS = R.EPS
IVP = R.IVP


def operators(T, flags):
    """(pre, [hour of operator s]) for s = 0 .. N-1"""
    return R.schedule(T, flags)


def K2(Z):
    """K of the header: twice the roundings behind a term of V: a chain, the segments and 12 fixed ones"""
    n, seg_len = G.segments(Z)
    return 2 * (-(-seg_len // 4) + n + 12)


def bounds(Z, T, flags, mag, w=None):
    """the header's absolute bounds from the magnitude recurrence's result mag: dict(mean, var, zone_mean, zone_var)"""
    N = len(operators(T, flags)[1])
    k = K2(Z)
    return {"zone_mean": [N * k * EPS * v for v in mag["zone_mean"]], "zone_var": [2 * N * k * EPS * v for v in mag["zone_var"]],
            "mean": (N * k + Z + 2) * EPS * mag["mean"], "var": (2 * N * k + Z + 2) * EPS * mag["var"]}


# ------------------------------------------------------------------------------------------------ over Fractions
def fraction_lv(p_drive, p_dest, A, B, w=None, flags=0, tables=None, magnitude=False):
    F = Fraction
    Z, T = p_drive.shape
    last, ell, r = tables if tables is not None else R.row_tables(p_dest)
    pre, hours = operators(T, flags)
    fa = (lambda v: abs(F(float(v)))) if magnitude else (lambda v: F(float(v)))
    mu, nu = [F(0)] * Z, [F(0)] * Z
    for s in range(len(hours) - 1, -1, -1):
        t, j = hours[s], s - pre
        q = [F(float(v)) for v in R.clip_q(p_drive[:, t])]
        V_, W_ = [], []
        for o in range(Z):
            gp, gd = (fa(A[o, j]), fa(B[o, j])) if j >= 0 else (F(0), F(0))
            if last[t][o] == 0.0:
                s1, s2, b = F(0), F(0), nu[o]
            else:
                terms = [(F(float(p_dest[o, d, t])), d) for d in range(Z) if p_dest[o, d, t] != 0.0]
                if ell[t][o] >= 0:
                    terms.append((F(float(r[t][o])), int(ell[t][o])))
                eta = (lambda d: mu[d] + mu[o]) if magnitude else (lambda d: mu[d] - mu[o])
                s1 = sum((p * eta(d) for p, d in terms), F(0))
                s2 = sum((p * eta(d) ** 2 for p, d in terms), F(0))
                b = sum((p * nu[d] for p, d in terms), F(0))
            db = gd + s1
            cv = s2 + s1 * s1 if magnitude else max(F(0), s2 - s1 * s1)
            J = q[o] * ((1 - q[o]) * db * db + cv)
            V_.append(gp + mu[o] + q[o] * db)
            W_.append((1 - q[o]) * nu[o] + q[o] * b + J)
        mu, nu = V_, W_
    ww = [F(1)] * Z if w is None else [F(float(v)) for v in w]
    return {"mean": sum(a * b for a, b in zip(ww, mu)), "var": sum(a * b for a, b in zip(ww, nu)), "zone_mean": mu, "zone_var": nu}


# ------------------------------------------------------------------------------------------------ over integers with binary scales
def _trim(v, k):
    return G._trim(v, k)


class NotExact(AssertionError):
    pass


def _fits(terms, bits, what):
    """every partial sum of the integer terms, in any order, has an odd part below 2^bits"""
    if bits is None or not any(terms):
        return
    g = min(((x & -x).bit_length() - 1) for x in terms if x)
    if sum(abs(x) for x in terms) >> g >= 1 << bits:
        raise NotExact(f"{what} leaves {bits} bits")


def int_lv(p_drive, p_dest, A, B, w=None, flags=0, tables=None, magnitude=False, bits=None):
    """fraction_lv's result, exactly, over Python integers.  bits: assert that every intermediate of the recurrence and of the
    totals -- and every partial sum in any order of its terms -- is an integer of at most `bits` bits times a power of two."""
    Z, T = p_drive.shape
    last, ell, r = tables if tables is not None else R.row_tables(p_dest)
    pre, hours = operators(T, flags)
    co, kg = R._dyadic(list(np.asarray(A, dtype=np.float64).T.ravel()) + list(np.asarray(B, dtype=np.float64).T.ravel()))
    if magnitude:
        co = [abs(x) for x in co]
    gA = lambda j, o: co[j * Z + o]
    gB = lambda j, o: co[T * Z + j * Z + o]
    cache = {}

    def hour(t):
        if t not in cache:
            vals, kp = R._dyadic(list(p_dest[:, :, t].ravel()) + list(r[t]))
            P = [vals[o * Z:(o + 1) * Z] for o in range(Z)]
            qi, kq = R._dyadic(list(R.clip_q(p_drive[:, t])))
            cache[t] = (P, vals[Z * Z:], kp, qi, kq)
        return cache[t]

    mu, km, nu, kn = [0] * Z, 0, [0] * Z, 0
    for s in range(len(hours) - 1, -1, -1):
        t, j = hours[s], s - pre
        P, ri, kp, q, kq = hour(t)
        kd = max(kg, kp + km)                 # db
        kv = kq + kd                          # V
        kw = max(kq + kp + kn, 2 * kq + 2 * kd)   # W
        Vn, Wn = [], []
        for o in range(Z):
            gp, gd = (gA(j, o), gB(j, o)) if j >= 0 else (0, 0)
            if last[t][o] == 0.0:
                s1, s2, b = 0, 0, nu[o] << kp
            else:
                terms = [(P[o][d], d) for d in range(Z) if P[o][d]]
                if ell[t][o] >= 0 and ri[o]:
                    terms.append((ri[o], int(ell[t][o])))
                eta = [(mu[d] + mu[o]) if magnitude else (mu[d] - mu[o]) for _, d in terms]
                t1 = [p * e for (p, _), e in zip(terms, eta)]
                t2 = [x * e for x, e in zip(t1, eta)]
                tb = [p * nu[d] for p, d in terms]
                for name, tt in (("eta", eta), ("s1", t1), ("s2", t2), ("b", tb)):
                    for x in tt:
                        _fits([x], bits, name)
                    if name != "eta":
                        _fits(tt, bits, name)
                s1, s2, b = sum(t1), sum(t2), sum(tb)     # scales kp + km, kp + 2 km, kp + kn
            db = (gd << (kd - kg)) + (s1 << (kd - kp - km))
            sq = s1 * s1                                  # scale 2 (kp + km)
            cv = (s2 << kp) + sq if magnitude else max(0, (s2 << kp) - sq)
            dd = db * db
            omq = (1 << kq) - q[o]
            ki = kq + 2 * kd
            in1, in2 = omq * dd, cv << (ki - 2 * (kp + km))
            J = q[o] * (in1 + in2)                        # scale kq + ki = 2 kq + 2 kd
            va, vb, vc = gp << (kv - kg), mu[o] << (kv - km), q[o] * db
            wa, wb, wc = (omq * nu[o]) << (kw - kq - kn), (q[o] * b) << (kw - kq - kp - kn), J << (kw - 2 * kq - 2 * kd)
            for name, tt in (("db", [gd << (kd - kg), s1 << (kd - kp - km)]), ("s1^2", [sq]), ("cv", [s2 << kp, sq]), ("db^2", [dd]),
                             ("J", [in1, in2]), ("J", [J]), ("V", [va, vb, vc]), ("W", [wa, wb, wc])):
                _fits(tt, bits, name)
            Vn.append(va + vb + vc)
            Wn.append(wa + wb + wc)
        both, kk = _trim(Vn + [1 << kv], kv)      # (the trailing 1 keeps the scale an exponent >= 0)
        mu, km = both[:Z], kk
        both, kk = _trim(Wn + [1 << kw], kw)
        nu, kn = both[:Z], kk
    wi, kwt = ([1] * Z, 0) if w is None else R._dyadic(list(w))
    tm, tv = [a * b for a, b in zip(wi, mu)], [a * b for a, b in zip(wi, nu)]
    _fits(tm, bits, "mean")
    _fits(tv, bits, "var")
    return {"mean": Fraction(sum(tm), 1 << (km + kwt)), "var": Fraction(sum(tv), 1 << (kn + kwt)),
            "zone_mean": [Fraction(x, 1 << km) for x in mu], "zone_var": [Fraction(x, 1 << kn) for x in nu]}


# ------------------------------------------------------------------------------------------------ numpy, in the documented order
def _total(w, x):
    """chain i of 256 adds w[z] * x[z] for z = i, i + 256, ... from 0; the chains are added pairwise, i + h to i, h = 128 .. 1"""
    Z = len(x)
    acc = np.zeros(256)
    for z0 in range(0, Z, 256):
        n = min(256, Z - z0)
        acc[:n] = acc[:n] + (x[z0:z0 + n] if w is None else w[z0:z0 + n] * x[z0:z0 + n])
    h = 128
    while h:
        acc[:h] = acc[:h] + acc[h:2 * h]
        h //= 2
    return float(acc[0])


def numpy_lv(p_drive, p_dest, A, B, w=None, flags=0, tables=None, magnitude=False, raw=False):
    """f64, every step one IEEE operation, the sums in the order of include/cpm_expected_linear_var.h.  raw: the mutant (below)."""
    Z, T = p_drive.shape
    last, ell, r = tables if tables is not None else R.row_tables(p_dest)
    pre, hours = operators(T, flags)
    nseg, seg_len = G.segments(Z)
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    if magnitude:
        A, B = np.abs(A), np.abs(B)
    mu, nu = np.zeros(Z), np.zeros(Z)
    for s in range(len(hours) - 1, -1, -1):
        t, j = hours[s], s - pre
        gp, gd = (A[:, j], B[:, j]) if j >= 0 else (np.zeros(Z), np.zeros(Z))
        q = R.clip_q(p_drive[:, t])
        s1, s2, b = np.zeros(Z), np.zeros(Z), np.zeros(Z)
        if s != len(hours) - 1:
            p = p_dest[:, :, t]
            ctr = np.zeros(Z) if raw else mu
            for sg in range(nseg):
                begin, end = sg * seg_len, min(Z, (sg + 1) * seg_len)
                c1, c2, cb = np.zeros((4, Z)), np.zeros((4, Z)), np.zeros((4, Z))
                for d in range(begin, end):
                    c = (d - begin) % 4
                    e = mu[d] + ctr if magnitude else mu[d] - ctr
                    tt = p[:, d] * e
                    c1[c] = c1[c] + tt
                    c2[c] = c2[c] + tt * e
                    cb[c] = cb[c] + p[:, d] * nu[d]
                f = lambda x: ((x[0] + x[1]) + x[2]) + x[3]
                s1, s2, b = (f(c1), f(c2), f(cb)) if sg == 0 else (s1 + f(c1), s2 + f(c2), b + f(cb))
            has = (last[t] != 0.0) & (ell[t] >= 0)
            l = np.where(has, ell[t], 0)
            el = mu[l] + ctr if magnitude else mu[l] - ctr
            tl = r[t] * el
            s1 = np.where(has, s1 + tl, s1)
            s2 = np.where(has, s2 + tl * el, s2)
            b = np.where(has, b + r[t] * nu[l], b)
            zero = last[t] == 0.0
            s1, s2, b = np.where(zero, 0.0, s1), np.where(zero, 0.0, s2), np.where(zero, nu, b)
            if raw:          # the raw moments about 0: s1 = sum p mu, s2 = sum p mu^2; the mean shift is put back by hand
                tot = np.minimum(last[t], 1.0) + r[t]
                s1c = s1 - tot * mu
                s1, s2 = np.where(zero, 0.0, s1c), np.where(zero, 0.0, (s2 - s1 * s1) + s1c * s1c)
        omq = 1.0 - q
        db = gd + s1
        cv = s2 + s1 * s1 if magnitude else np.maximum(s2 - s1 * s1, 0.0)
        J = q * (omq * (db * db) + cv)
        mu, nu = (gp + mu) + q * db, (omq * nu + q * b) + J
    return {"mean": _total(w, mu), "var": _total(w, nu), "zone_mean": mu, "zone_var": nu}


def raw_moment_lv(p_drive, p_dest, A, B, w=None, flags=0, tables=None):
    """The mutant the centring rules out: the variance of the destination's value from the raw moments, sum p mu^2 - (sum p mu)^2
    (for rows that sum to 1), which is the same number in exact arithmetic and c^2 Z 2^-52 of noise in f64."""
    return numpy_lv(p_drive, p_dest, A, B, w, flags, tables, raw=True)


def worst(got, exact, bound):
    """{key: max |got - exact| / bound}, and whether every word whose bound is 0 is equal to the exact one (0 where that is 0)"""
    res, zeros_ok = {}, True
    for key in ("mean", "var", "zone_mean", "zone_var"):
        g, e, b = (np.atleast_1d(np.asarray(x, dtype=object)) for x in (got[key], exact[key], bound[key]))
        wmax = Fraction(0)
        for gi, ei, bi in zip(g, e, b):
            gi, ei, bi = Fraction(float(gi)), Fraction(ei), Fraction(bi)
            if bi == 0:
                zeros_ok = zeros_ok and gi == ei == 0
                continue
            wmax = max(wmax, abs(gi - ei) / bi)
        res[key] = float(wmax)
    return res, zeros_ok


# ------------------------------------------------------------------------------------------------ every path of one car
def brute_force(p_drive, p_dest, A, B, w=None, flags=0, tables=None):
    """(mean, var) of L as Fractions by enumerating every path of one car from each start zone: per operator the Bernoulli of q, and
    for a driver of a non-zero row the destination d with p[o, d] (the residual r at l).  Asserts that each row's law sums to 1."""
    F = Fraction
    Z, T = p_drive.shape
    last, ell, r = tables if tables is not None else R.row_tables(p_dest)
    pre, hours = operators(T, flags)
    N = len(hours)

    def moves(t, o):
        if last[t][o] == 0.0:
            return [(F(1), o)]
        m = [(F(float(p_dest[o, d, t])), d) for d in range(Z) if p_dest[o, d, t] != 0.0]
        if ell[t][o] >= 0 and r[t][o] != 0.0:
            m.append((F(float(r[t][o])), int(ell[t][o])))
        assert sum(p for p, _ in m) == 1, "the row's law does not sum to 1: no probability space to enumerate"
        return m

    def walk(s, o, prob, reward, acc):
        if s == N:
            acc[0] += prob * reward
            acc[1] += prob * reward * reward
            return
        t, j = hours[s], s - pre
        gp, gd = (F(float(A[o, j])), F(float(B[o, j]))) if j >= 0 else (F(0), F(0))
        q = F(float(R.clip_q(p_drive[:, t])[o]))
        if q != 1:
            walk(s + 1, o, prob * (1 - q), reward + gp, acc)
        if q != 0:
            if s == N - 1:                          # (sampled and never applied)
                walk(s + 1, o, prob * q, reward + gp + gd, acc)
            else:
                for p, d in moves(t, o):
                    walk(s + 1, d, prob * q * p, reward + gp + gd, acc)

    mean, var = F(0), F(0)
    for z in range(Z):
        wz = F(1) if w is None else F(float(w[z]))
        acc = [F(0), F(0)]
        walk(0, z, F(1), F(0), acc)
        mean += wz * acc[0]
        var += wz * (acc[1] - acc[0] ** 2)
    return mean, var


# ------------------------------------------------------------------------------------------------ functionals
def small_functionals(Z, T, K, seed, lo=-2, hi=2):
    """K functionals (A, B): (Z, T, K) F-order arrays of integers in lo .. hi"""
    rng = np.random.default_rng(seed)
    return (np.asfortranarray(rng.integers(lo, hi + 1, (Z, T, K)).astype(np.float64)),
            np.asfortranarray(rng.integers(lo, hi + 1, (Z, T, K)).astype(np.float64)))


def signed_functionals(Z, T, K, seed):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(rng.uniform(-1.0, 1.0, (Z, T, K))), np.asfortranarray(rng.uniform(-1.0, 1.0, (Z, T, K)))


def indicator(Z, T, kind, z, t):
    A, B = np.zeros((Z, T), order="F"), np.zeros((Z, T), order="F")
    (A if kind == "parking" else B)[z, t] = 1.0
    return A, B


# ------------------------------------------------------------------------------------------------ the statistical test
def stat_functionals(Z, T, seed=3):
    """[(group, A, B)]: driving_sum[t] for t = 1 .. 6, the car-hours parked in each zone over the day, 8 random signed functionals"""
    out = []
    for t in range(1, 7):
        B = np.zeros((Z, T), order="F")
        B[:, t] = 1.0
        out.append(("driving_sum", np.zeros((Z, T), order="F"), B))
    for z in range(Z):
        A = np.zeros((Z, T), order="F")
        A[z, :] = 1.0
        out.append(("car_hours", A, np.zeros((Z, T), order="F")))
    A, B = signed_functionals(Z, T, 8, seed)
    for k in range(8):
        out.append(("random", np.asfortranarray(A[:, :, k]), np.asfortranarray(B[:, :, k])))
    return out


STAT_P_MIN, STAT_P_MAX = 0.2, 0.5


def stat_setup(O):
    """expected_var_reference.stat_setup with tables that drive more (slow_tables with p_drive in 0.2 .. 0.5, not 0.03 .. 0.12).
    The mutant without covariances overstates the variance of driving_sum[t] by about the probability that a car drives (the
    zones' driving counts are negatively correlated by that much): 4 % on the slow tables, inside the cap of 400 seeds, which is
    5.5 * sqrt(2 / (6 * 400)) = 0.16 for six functionals; a third here.  The car-hours keep a ratio of 3.5 (11 on the slow tables):
    a car still stays put with probability 0.5 .. 0.8 per hour.  check_stat asserts both ratios before it looks at a sample."""
    p_drive, p_dest = V.slow_tables(O, V.STAT_Z, V.STAT_T, p_max=STAT_P_MAX, p_min=STAT_P_MIN)
    state, _ = O.initializestates(V.STAT_Z * V.STAT_CPZ, V.STAT_CPZ, V.STAT_T, with_trans=False)
    zone0 = np.ascontiguousarray(state[:, 0])
    w = np.bincount(zone0 - 1, minlength=V.STAT_Z).astype(np.float64)
    assert np.array_equal(w, np.full(V.STAT_Z, float(V.STAT_CPZ)))
    return p_drive, p_dest, zone0, w


def stat_stack(funcs):
    """the functionals as the (Z, T, K) arrays of Sampler.expected_linear_var"""
    return np.asfortranarray(np.stack([a for _, a, _ in funcs], axis=2)), np.asfortranarray(np.stack([b for _, _, b in funcs], axis=2))


def stat_values(runs, funcs):
    """(runs, K): L of every run's (parking, driving) count arrays"""
    return np.array([[float((A * park).sum() + (B * drv).sum()) for _, A, B in funcs] for park, drv in runs])


def mutant_var(funcs, ev):
    """the mutant that drops the covariances: sum A^2 var_parking + B^2 var_driving of the exact per-cell variances"""
    return np.array([float((A * A * ev["var_parking"]).sum() + (B * B * ev["var_driving"]).sum()) for _, A, B in funcs])


def stat_within_cap(L, mean, var, pick):
    """|mean(v) - 1| <= 5.5 std(v) / sqrt(R), v = the run's mean over the picked functionals of (L - mean)^2 / var, the standard error
    formed as expected_var_reference.within_cap forms it; returns (passes, mean, half width)"""
    pick = np.asarray(pick)
    assert (var[pick] > 0).all()
    v = ((L[:, pick] - mean[pick]) ** 2 / var[pick]).mean(axis=1)
    half = V.CAP * v.std(ddof=1) / np.sqrt(len(v))
    return abs(v.mean() - 1.0) <= half, v.mean(), half


def check_stat(L, funcs, mean, var, mut, label, with_mutant=True):
    """the cap over all functionals and per group with the exact variance; the mutant must fail for driving_sum and for car_hours"""
    groups = [g for g, _, _ in funcs]
    ok, m, half = stat_within_cap(L, mean, var, list(range(len(funcs))))
    print(f"{label}: all {len(funcs)} functionals: exact {m:.4f} +- {half:.4f}")
    assert ok, "the exact variance misses the cap over all functionals"
    for g in ("driving_sum", "car_hours", "random"):
        pick = [k for k, name in enumerate(groups) if name == g]
        ok, m, half = stat_within_cap(L, mean, var, pick)
        okm, mm, halfm = stat_within_cap(L, mean, mut, pick)
        print(f"{label}: {g}: exact {m:.4f} +- {half:.4f}, without covariances {mm:.4f} +- {halfm:.4f}")
        assert ok, f"the exact variance misses the cap for {g}"
        if with_mutant and g != "random":
            ratio = float((var[pick] / mut[pick]).mean())           # what the mutant's statistic tends to
            assert abs(ratio - 1.0) > 2.0 * half, f"the tables put the mutant's statistic for {g} ({ratio:.3f}) inside the cap: choose others"
            assert not okm, f"the variance without covariances passes the cap for {g}"
