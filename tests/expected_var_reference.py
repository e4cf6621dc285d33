"""References of the definition in include/cpm_expected_var.h, computed from the f64 tables (not a conftest: imported by
tests/test_expected_var.py and tests/test_expected_var_gpu.py):

  exact_var     every table entry as a fractions.Fraction, M_t and the chain P_{t+1} = P_t * M_t without rounding (r and the row
                total are the f64 words of the installed table, as the definition says; 1 - q is exact).  f64 values are dyadic, so
                an hour's Fractions are put over one power-of-two denominator and the products run over Python integers;
  int_var       the same chain for tables whose entries are multiples of 2^-8, over Python integers from the start (no Fraction is
                formed on the way in): M_t in units of 2^-16;
  numpy_var     the definition in numpy f64 (numpy's own order of sums in the product);
  bound / worst    the header's bound: the means relative, the variances absolute in units of the exact mean of the same cell;
  check_statistic  the statistical test of the sampler's spread, shared by the CPU and the GPU test.

Tables are the host arrays of the ABI: p_drive (Z, T), p_dest (Z origin, Z dest, T).  Outputs: dicts of four (Z, T) arrays."""
from fractions import Fraction

import numpy as np

import expected_reference as R

EPS = R.EPS
IVP = R.IVP
KEYS = ("mean_parking", "mean_driving", "var_parking", "var_driving")
RUNS, STAT_Z, STAT_CPZ, CAP = 400, 12, 40, 5.5       # the statistical test: seeds, zones, cars per zone, the cap in standard errors
STAT_T = 24


def schedule(T, flags):
    """[(hour of the operator, hour of the day whose matrix it produces or None)]; pre: operators in front of the day"""
    pre = T - 1 if (flags & IVP) else 0
    return pre, [((s if s < pre else s - pre), (s + 1 - pre if s + 1 - pre >= 0 else None)) for s in range(pre + T - 1)]


def operators_behind(T, flags):
    pre = T - 1 if (flags & IVP) else 0
    return [pre + t for t in range(T)]


def bound(Z, h):
    """E of the header: the relative bound of a mean word after h operators, and the bound of a variance word in units of the mean"""
    return (h + 1) * (Z + 8) * EPS


# ------------------------------------------------------------------------------------------------ M_t
def numpy_M(p_drive, p_dest, t, tables):
    """M_t[o][d] in f64, in the library's order: ((p * q) + q * r) + (1 - q), a term that does not apply left out"""
    last, ell, r = tables
    Z = p_drive.shape[0]
    q = R.clip_q(p_drive[:, t])
    M = p_dest[:, :, t] * q[:, None]
    o = np.arange(Z)
    has = (last[t] != 0.0) & (ell[t] >= 0)
    M[o[has], ell[t][has]] = M[o[has], ell[t][has]] + (q * r[t])[has]
    M[o, o] = M[o, o] + (1.0 - q)
    zero = last[t] == 0.0
    M[zero, :] = 0.0
    M[o[zero], o[zero]] = 1.0
    return M


def exact_M(p_drive, p_dest, t, tables):
    """M_t as a (Z, Z) object array of Fractions"""
    last, ell, r = tables
    Z = p_drive.shape[0]
    q = [Fraction(float(v)) for v in R.clip_q(p_drive[:, t])]
    M = np.empty((Z, Z), dtype=object)
    for o in range(Z):
        if last[t][o] == 0.0:
            for d in range(Z):
                M[o, d] = Fraction(int(d == o))
            continue
        for d in range(Z):
            M[o, d] = q[o] * Fraction(float(p_dest[o, d, t]))
        if ell[t][o] >= 0:
            M[o, int(ell[t][o])] += q[o] * Fraction(float(r[t][o]))
        M[o, o] += 1 - q[o]
    return M


def _ints(fracs):
    """dyadic Fractions (any shape) -> (object array of ints, k): value == int / 2**k"""
    a = np.asarray(fracs, dtype=object)
    k = max(f.denominator.bit_length() - 1 for f in a.ravel())
    out = np.empty(a.shape, dtype=object)
    for i, f in enumerate(a.ravel()):
        out.ravel()[i] = f.numerator << (k - (f.denominator.bit_length() - 1))
    return out, k


# ------------------------------------------------------------------------------------------------ the chain over integers
def _chain(Z, T, flags, hour_M, hour_q, w, kw):
    """hour_M(t) -> (int matrix, bits), hour_q(t) -> (int vector, bits), w: ints over 2**kw.  Four (Z, T) object arrays of Fractions."""
    out = {k: np.empty((Z, T), dtype=object) for k in KEYS}
    cache = {}

    def sums(P, kP, t):
        q, kq = hour_q(t)
        one_p, one_a = 1 << kP, 1 << (kP + kq)
        for z in range(Z):
            mp = md = vp = vd = 0
            for s in range(Z):
                if not w[s]:
                    continue
                pv = P[s, z]
                a = pv * q[z]
                mp += w[s] * pv
                md += w[s] * a
                vp += w[s] * pv * (one_p - pv)
                vd += w[s] * a * (one_a - a)
            out["mean_parking"][z, t] = Fraction(mp, 1 << (kP + kw))
            out["mean_driving"][z, t] = Fraction(md, 1 << (kP + kq + kw))
            out["var_parking"][z, t] = Fraction(vp, 1 << (2 * kP + kw))
            out["var_driving"][z, t] = Fraction(vd, 1 << (2 * (kP + kq) + kw))

    P = np.array([[int(s == o) for o in range(Z)] for s in range(Z)], dtype=object).reshape(Z, Z)
    kP = 0
    pre, steps = schedule(T, flags)
    if pre == 0:
        sums(P, kP, 0)
    for t, day in steps:
        if t not in cache:
            cache[t] = hour_M(t)
        M, km = cache[t]
        P, kP = P.dot(M), kP + km
        nz = [int(v) for v in P.ravel() if v]
        g = min(min((v & -v).bit_length() - 1 for v in nz), kP)     # (drop common trailing zeros: the ints stay short)
        if g:
            P, kP = np.array([v >> g for v in P.ravel()], dtype=object).reshape(Z, Z), kP - g
        if day is not None:
            sums(P, kP, day)
    return out


def _weights(w, Z):
    if w is None:
        return [1] * Z, 0
    wi, kw = _ints([Fraction(float(v)) for v in w])
    return [int(v) for v in wi], kw


def exact_var(p_drive, p_dest, w=None, flags=0, tables=None):
    """the four outputs as (Z, T) object arrays of Fractions, no rounding"""
    Z, T = p_drive.shape
    tables = tables if tables is not None else R.row_tables(p_dest)
    wi, kw = _weights(w, Z)
    return _chain(Z, T, flags, lambda t: _ints(exact_M(p_drive, p_dest, t, tables)),
                  lambda t: _ints([Fraction(float(v)) for v in R.clip_q(p_drive[:, t])]), wi, kw)


def int_var(p_drive, p_dest, w=None, flags=0):
    """The same for tables whose entries are multiples of 2^-8 (p_drive may lie outside [0, 1]: clipped) and integer w, over Python
    integers: q and p in units of 2^-8, M_t in units of 2^-16.  Every row total is at most 1 (asserted)."""
    Z, T = p_drive.shape
    q8 = np.rint(R.clip_q(p_drive) * 256).astype(np.int64)
    p8 = np.rint(p_dest * 256).astype(np.int64)
    assert np.array_equal(q8 / 256.0, R.clip_q(p_drive)) and np.array_equal(p8 / 256.0, p_dest), "not multiples of 2^-8"
    assert (p8 >= 0).all() and (p8.sum(axis=1) <= 256).all()
    wi = [1] * Z if w is None else [int(v) for v in w]
    assert w is None or np.array_equal(np.asarray(wi, dtype=np.float64), np.asarray(w, dtype=np.float64))

    def hour_M(t):
        M = np.empty((Z, Z), dtype=object)
        for o in range(Z):
            row = [int(v) for v in p8[o, :, t]]
            tot, q = sum(row), int(q8[o, t])
            if tot == 0:
                for d in range(Z):
                    M[o, d] = (1 << 16) if d == o else 0
                continue
            for d in range(Z):
                M[o, d] = q * row[d]
            M[o, max(d for d in range(Z) if row[d] > 0)] += q * (256 - tot)
            M[o, o] += (256 - q) * 256
        return M, 16

    return _chain(Z, T, flags, hour_M, lambda t: ([int(v) for v in q8[:, t]], 8), wi, 0)


def to_f64(fr):
    """a (Z, T) object array of Fractions -> f64, and whether every conversion was exact"""
    out = np.array([[float(v) for v in row] for row in fr], dtype=np.float64)
    exact = all(Fraction(float(v)) == v for v in np.asarray(fr, dtype=object).ravel())
    return out, exact


# ------------------------------------------------------------------------------------------------ numpy
def numpy_P(p_drive, p_dest, flags=0, tables=None):
    """[P_0 .. P_{T-1}] in f64"""
    Z, T = p_drive.shape
    tables = tables if tables is not None else R.row_tables(p_dest)
    P = np.eye(Z)
    pre, steps = schedule(T, flags)
    Ps = [P] if pre == 0 else []
    Ms = {}
    for t, day in steps:
        if t not in Ms:
            Ms[t] = numpy_M(p_drive, p_dest, t, tables)
        P = P @ Ms[t]
        if day is not None:
            Ps.append(P)
    return Ps


def numpy_var(p_drive, p_dest, w=None, flags=0, tables=None):
    """the four outputs as (Z, T) f64 arrays"""
    Z, T = p_drive.shape
    w = np.ones(Z) if w is None else np.asarray(w, dtype=np.float64)
    out = {k: np.zeros((Z, T), order="F") for k in KEYS}
    for t, P in enumerate(numpy_P(p_drive, p_dest, flags, tables)):
        a = P * R.clip_q(p_drive[:, t])[None, :]
        out["mean_parking"][:, t] = w @ P
        out["mean_driving"][:, t] = w @ a
        out["var_parking"][:, t] = w @ (P * np.maximum(1.0 - P, 0.0))
        out["var_driving"][:, t] = w @ (a * np.maximum(1.0 - a, 0.0))
    return out


def binomial_var(mean, C):
    """the width every earlier comparison used: C * pi * (1 - pi) with pi = mean / C -- an upper bound of the exact variance"""
    pi = np.asarray(mean, dtype=np.float64) / C
    return C * pi * (1.0 - pi)


# ------------------------------------------------------------------------------------------------ the bound
def worst(got, exact, Z, T, flags):
    """{key: max over the words of |got - exact| / bound}, and whether every word whose exact value is 0 is 0.  got: dict of f64
    (Z, T); exact: dict of Fractions (or f64: compared in Fractions all the same).  The bound of a mean word is E * its exact value,
    that of a variance word E * the exact MEAN of the same cell."""
    h = operators_behind(T, flags)
    res, zeros_ok = {}, True
    for key in KEYS:
        scale = exact["mean_" + key.split("_")[1]]
        w = Fraction(0)
        for t in range(T):
            E = Fraction(bound(Z, h[t]))
            for z in range(Z):
                e, g, m = Fraction(exact[key][z, t]), Fraction(float(got[key][z, t])), Fraction(scale[z, t])
                if e == 0:
                    zeros_ok = zeros_ok and g == 0
                    continue
                w = max(w, abs(g - e) / (E * m))
        res[key] = float(w)
    return res, zeros_ok


def worst_f64(got, want, Z, T, flags, factor=1.0):
    """the same against an f64 reference, vectorised (the sizes the exact form is too slow for)"""
    E = np.array([bound(Z, h) for h in operators_behind(T, flags)])[None, :] * factor
    res, zeros_ok = {}, True
    for key in KEYS:
        m = want["mean_" + key.split("_")[1]]
        zero = want[key] == 0.0
        zeros_ok = zeros_ok and bool(np.all(got[key][zero] == 0.0))
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(zero, 0.0, np.abs(got[key] - want[key]) / (E * m))
        res[key] = float(np.nan_to_num(ratio, nan=np.inf).max())
    return res, zeros_ok


# ------------------------------------------------------------------------------------------------ tables
def dyadic_tables(Z, T, seed=7):
    """p_drive, p_dest (multiples of 2^-3 and 2^-2, hence of 2^-8) and integer w, small enough that every product and sum of a T = 3 day is exact in f64:
    M_t is in units of 2^-5, P_2 of 2^-10, a of 2^-12 and a * (1 - a) of 2^-24, times w < 2^4 over at most 2^8 rows.  They hold a zero
    row, a row below 1 whose residual lands on l, p_drive clipped at both ends, a zero in w and non-zero diagonals p[o, o]."""
    assert T <= 3
    rng = np.random.default_rng(seed + Z)
    p_dest = np.zeros((Z, Z, T), order="F")
    for t in range(T):
        for o in range(Z):
            left = 8
            for d in rng.choice(Z, size=min(Z, 3), replace=False):
                k = int(rng.integers(0, left + 1))
                p_dest[o, d, t] += k / 8.0
                left -= k
            if (o + t) % 3 == 0:
                p_dest[o, o, t] += left / 8.0               # a diagonal entry, and the row is complete
    p_drive = rng.integers(0, 5, size=(Z, T)).astype(np.float64) / 4.0
    p_drive = np.asfortranarray(p_drive)
    p_drive[0, :] = [-0.25, 1.5, 0.0][:T]                   # clipped to 0, to 1, and 0 itself
    p_drive[Z - 1, 0] = 1.0
    p_dest[Z - 1, :, 0] = 0.0                               # a zero row that drives
    p_dest[0, :, 1] = 0.0
    p_dest[0, 0, 1] = 0.25                                  # row total 1/4: the residual 3/4 lands on l = 0, the diagonal
    if Z > 2:
        p_dest[1, :, 0] = 0.0
        p_dest[1, [0, Z - 2], 0] = [0.25, 0.5]              # the residual 1/4 lands on l = Z - 2
        p_drive[1, 0] = 0.75
    w = rng.integers(1, 12, size=Z).astype(np.float64)
    w[Z // 2] = 0.0
    return p_drive, p_dest, w


def dyadic8_tables(Z, T, seed=5):
    """tables of any T whose entries are multiples of 2^-8 (row totals, r and 1 - q are then exact: every row of M_t sums to 1 in
    rationals), with a zero row and rows below 1"""
    rng = np.random.default_rng(seed + Z)
    p8 = np.zeros((Z, Z, T), dtype=np.int64)
    for t in range(T):
        for o in range(Z):
            cuts = np.sort(rng.integers(0, 257, size=Z - 1))
            row = np.diff(np.concatenate([[0], cuts, [256]]))
            row[rng.integers(0, Z)] = 0                       # (the total drops below 1, or the entry was 0)
            p8[o, :, t] = row
    p8[Z // 2, :, T // 2] = 0
    q8 = rng.integers(0, 257, size=(Z, T))
    return np.asfortranarray(q8 / 256.0), np.asfortranarray(p8 / 256.0)


def slow_tables(O, Z, T, p_max=0.12, p_min=0.03, seed=11):
    """tables of a chain that mixes slowly: p_drive between p_min and p_max from the oracle's builders on a synthetic dataset"""
    dm, dist = O.synth_datamatrix(Z, T, seed, 0.6)
    return O.createpdrive(dm, dist, Z, T, p_min, p_max, 0.5), O.createpdestin(dm, Z, T, 2)


# ------------------------------------------------------------------------------------------------ the statistical test
def stat_setup(O):
    p_drive, p_dest = slow_tables(O, STAT_Z, STAT_T)
    state, _ = O.initializestates(STAT_Z * STAT_CPZ, STAT_CPZ, STAT_T, with_trans=False)
    zone0 = np.ascontiguousarray(state[:, 0])
    w = np.bincount(zone0 - 1, minlength=STAT_Z).astype(np.float64)
    assert np.array_equal(w, np.full(STAT_Z, float(STAT_CPZ)))
    return p_drive, p_dest, zone0, w


def g_with(runs, mean, var, used):
    kept, fixed, between = var >= 0.5, var == 0.0, (var > 0.0) & (var < 0.5)
    assert between.sum() <= var.size / 4, f"{between.sum()} of {var.size} cells have a variance in (0, 0.5)"
    g = np.zeros((len(runs), mean.shape[2]))
    for i, (park, drv) in enumerate(runs):
        n = np.stack([park, drv]).astype(np.float64)
        assert np.array_equal(n[fixed], mean[fixed]), "a count of variance 0 is not its mean"
        with np.errstate(divide="ignore", invalid="ignore"):
            g[i] = np.where(kept, (n - mean) ** 2 / used, 0.0).sum(axis=(0, 1))
    return g, kept.sum(axis=(0, 1))


def within_cap(g, kept, hours):
    """|mean(g) - 1| <= 5.5 std(g) / sqrt(R) for the mean over the kept cells of the given hours; returns (passes, mean, half width)"""
    v = g[:, hours].sum(axis=1) / kept[hours].sum()
    half = CAP * v.std(ddof=1) / np.sqrt(len(v))
    return abs(v.mean() - 1.0) <= half, v.mean(), half


def check_statistic(runs, ev, C, label):
    """the caps with the exact variance, and the mutant that puts the binomial variance into the same statistic"""
    mean = np.stack([ev["mean_parking"], ev["mean_driving"]])
    var = np.stack([ev["var_parking"], ev["var_driving"]])
    g, kept = g_with(runs, mean, var, var)
    gm, _ = g_with(runs, mean, var, binomial_var(mean, C))
    Tn = mean.shape[2]
    ok, m, half = within_cap(g, kept, list(range(Tn)))
    okm, mm, halfm = within_cap(gm, kept, list(range(Tn)))
    print(f"{label}: all hours: exact {m:.4f} +- {half:.4f}, binomial {mm:.4f} +- {halfm:.4f}")
    assert ok, "the exact variance misses the cap over all hours"
    assert not okm, "the binomial variance passes the cap over all hours"
    differ = 0
    for t in range(1, 7):
        ok, m, half = within_cap(g, kept, [t])
        okm, mm, halfm = within_cap(gm, kept, [t])
        k = var[:, :, t] >= 0.5
        ratio = (var[:, :, t][k] / binomial_var(mean, C)[:, :, t][k]).mean()          # what the mutant's statistic tends to
        print(f"{label}: hour {t}: exact {m:.4f} +- {half:.4f}, binomial {mm:.4f} +- {halfm:.4f}, variance ratio {ratio:.3f}")
        assert ok, f"the exact variance misses the cap at hour {t}"
        if abs(ratio - 1.0) > 0.1:
            differ += 1
            assert not okm, f"the binomial variance passes the cap at hour {t}"
    assert differ >= 3
    return differ
