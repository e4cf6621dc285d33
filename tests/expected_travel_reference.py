"""References of the definition in include/cpm_expected_travel.h, computed from the f64 tables (not a conftest: imported by
tests/test_expected_travel.py and tests/test_expected_travel_gpu.py), on top of expected_reference:

  exact_trip / exact_travel   every entry converted to fractions.Fraction (through the dyadic integers of expected_reference) and
                              the sums evaluated without rounding; `last`, `r` and the densities' q are the only f64 operations, as
                              the definitions say;
  numpy_trip / numpy_travel   the same in f64 in the order the header documents for the device: segments of destinations, four
                              interleaved chains per segment, chains then segments in order, the residual term last; the totals as
                              chunks of 1,024 words (256 chains, a wave's shuffle tree, four waves in order), then the chunks;
  bound_trip / bound_travel / bound_total   the header's relative bounds;
  trip_moments                the mean and the variance of one trip's seconds and kilometres (for the statistical tests).

Tables are the host arrays of the ABI: p_dest (Z origin, Z dest, T), datamatrix (Z origin, Z dest, T, 2: mean, std), dist (Z, Z)."""
import math
from fractions import Fraction

import numpy as np

import expected_reference as R

EPS = R.EPS
INTRA_SEC, INTRA_KM = 300.0, 1.0          # a trip inside a zone (src/resampling.jl:58-60)


def trip_values(dm, dist):
    """(sec (Z, Z, T), km (Z, Z)) indexed [origin, destination]: the mean word and the distance with the diagonal selected"""
    Z = dist.shape[0]
    sec = np.array(dm[:, :, :, 0], dtype=np.float64, order="F")
    km = np.array(dist, dtype=np.float64, order="F")
    z = np.arange(Z)
    sec[z, z, :] = INTRA_SEC
    km[z, z] = INTRA_KM
    return sec, km


def segments(Z, T):
    """(number of destination segments, their length): trip_segments / trip_segment_len of csrc/cpm_expected_travel.h"""
    base = -(-Z // 128) * T
    n = max(1, min(8, -(-Z // 64), -(-1024 // base)))
    return n, -(-Z // n)


def bound_trip(Z):
    """relative bound of a trip weight: twice the Z / 4 + 14 roundings a term passes (include/cpm_expected_travel.h)"""
    return (Z / 4.0 + 16.0) * EPS


def bound_travel(Z, h):
    """relative bound of a fleet's seconds / km word whose driving density lies h operators behind pi_0"""
    return R.bound_driving(Z, h) + (Z / 4.0 + 17.0) * EPS


def bound_total(Z, T, h_max):
    return bound_travel(Z, h_max) + (Z * T / 65536.0 + 20.0) * EPS


def planted_tables(O, Z, T, table_seed=11):
    """expected_reference.modified_tables (a zero row, a D1 row, a row that ends in zeros) with one row edited: the synthetic tables
    keep the diagonal empty, so the last origin's last two entries change places and the row is scaled by 0.8 -- an intra-zone cell
    with p > 0, and a residual that lands on the origin itself (ell == o, r > 0)."""
    p_drive, p_dest = R.modified_tables(O, Z, T, table_seed)
    o = Z - 1
    p_dest[o, [o - 1, o], :] = p_dest[o, [o, o - 1], :]
    p_dest[o, :, :] *= 0.8
    return p_drive, p_dest


def planted_datamatrix(O, Z, T, table_seed=11, density=0.5):
    """The oracle's synthetic datamatrix and distances with what the definition must not trip over: at density 0.5 half of the cells
    hold no mean (a mean of 0 under p > 0 on dense tables), and the diagonals, which the generator leaves empty, get values that are
    NOT 300 s and 1 km -- the select of the diagonal is visible wherever p[o, o] > 0 or a residual lands on the origin itself."""
    dm, dist = O.synth_datamatrix(Z, T, table_seed, density=density)
    z = np.arange(Z)
    dm[z, z, :, 0] = 777.25 + z[:, None]
    dm[z, z, :, 1] = 5.0
    dist[z, z] = 3.5
    dm[0, Z - 1, 0, :] = 0.0                 # (whatever the generator drew: one mean of 0 off the diagonal)
    return np.asfortranarray(dm), np.asfortranarray(dist)


# ------------------------------------------------------------------------------------------------ exact
def exact_trip(p_dest, dm, dist, tables=None):
    """(w_sec, w_km): (Z, T) object arrays of Fraction, no rounding"""
    Z, _, T = p_dest.shape
    last, ell, r = tables if tables is not None else R.row_tables(p_dest)
    sec, km = trip_values(dm, dist)
    out = [np.empty((Z, T), dtype=object), np.empty((Z, T), dtype=object)]
    for t in range(T):
        pi, kp = R._dyadic(np.concatenate([np.ascontiguousarray(p_dest[:, :, t]).ravel(), r[t]]))
        P = np.array(pi[:Z * Z], dtype=object).reshape(Z, Z)
        for which, val, intra in ((0, sec[:, :, t], INTRA_SEC), (1, km, INTRA_KM)):
            vi, kv = R._dyadic(np.ascontiguousarray(val).ravel())
            s = (P * np.array(vi, dtype=object).reshape(Z, Z)).sum(axis=1)
            for o in range(Z):
                if last[t][o] == 0.0:
                    out[which][o, t] = Fraction(intra)
                    continue
                tot = int(s[o])
                if ell[t][o] >= 0:
                    tot += pi[Z * Z + o] * vi[o * Z + int(ell[t][o])]
                out[which][o, t] = Fraction(tot, 1 << (kp + kv))
    return out[0], out[1]


def exact_travel(edrv, ew_sec, ew_km):
    """(seconds, km: (Z, T) Fractions, total_seconds, total_km) from the exact driving density and the exact weights"""
    seconds, km = edrv * ew_sec, edrv * ew_km
    return seconds, km, sum(seconds.ravel(), Fraction(0)), sum(km.ravel(), Fraction(0))


# ------------------------------------------------------------------------------------------------ f64, the device's order
def numpy_trip(p_dest, dm, dist, tables=None):
    """(w_sec, w_km), each (Z, T) f64 F-order, every step one f64 operation in the documented order"""
    Z, _, T = p_dest.shape
    last, ell, r = tables if tables is not None else R.row_tables(p_dest)
    sec, km = trip_values(dm, dist)
    nseg, seg_len = segments(Z, T)
    o = np.arange(Z)
    out = [np.zeros((Z, T), order="F"), np.zeros((Z, T), order="F")]
    for t in range(T):
        for which, val, intra in ((0, sec[:, :, t], INTRA_SEC), (1, km, INTRA_KM)):
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
            with np.errstate(invalid="ignore"):
                total = np.where(has, total + r[t] * val[o, l], total)
            out[which][:, t] = np.where(last[t] == 0.0, intra, total)
    return out[0], out[1]


def _wave_tree(v):
    """lane 0 of obj_wave_sum over 64 values: v[i] + v[i + 32], then 16, 8, 4, 2, 1"""
    v = np.array(v, dtype=np.float64)
    k = 32
    while k:
        v[:k] = v[:k] + v[k:2 * k]
        k >>= 1
    return v[0]


def _device_total(a):
    """the sum of a (Z, T) array in the order of k_exp_travel / k_exp_travel_total: chunks of 1,024 words of [T][Z], 256 chains of
    four words per chunk, the shuffle tree of a wave and four waves in order; then 64 chains over the chunks and the same tree"""
    flat = np.asarray(a, dtype=np.float64).ravel(order="F")
    pad = (-flat.size) % 1024
    chunks = np.concatenate([flat, np.zeros(pad)]).reshape(-1, 4, 256)   # (+0 behind the end: no bit of a non-negative sum changes)
    parts = []
    for c in chunks:
        acc = np.zeros(256)
        for row in c:
            acc = acc + row
        waves = [_wave_tree(acc[64 * w:64 * (w + 1)]) for w in range(4)]
        parts.append(((waves[0] + waves[1]) + waves[2]) + waves[3])
    parts = np.concatenate([parts, np.zeros((-len(parts)) % 64)]).reshape(-1, 64)
    acc = np.zeros(64)
    for row in parts:
        acc = acc + row
    return float(_wave_tree(acc))


def numpy_travel(driving, w_sec, w_km):
    """(seconds, km, total_seconds, total_km) from a (Z, T) driving density and the weights, in the device's order"""
    seconds, km = driving * w_sec, driving * w_km
    return seconds, km, _device_total(seconds), _device_total(km)


# ------------------------------------------------------------------------------------------------ moments of one trip
def _var_cell(mean, sigma):
    """the variance of the draw in [0.9 mu, 1.1 mu]: sigma^2 (1 - 2 a phi(a) / erf(a / sqrt 2)), a = 0.1 mu / sigma; 0 where sigma or
    the mass is not positive (the draw is the mean)"""
    mean, sigma = np.asarray(mean, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    out = np.zeros(mean.shape)
    for i in np.ndindex(mean.shape):
        s = float(sigma[i])
        if not s > 0.0:
            continue
        a = 0.1 * float(mean[i]) / s
        mass = math.erf(a / math.sqrt(2.0)) if a > 0.0 else 0.0
        if not mass > 0.0:
            continue
        phi = math.exp(-0.5 * a * a) / math.sqrt(2.0 * math.pi)
        out[i] = s * s * (1.0 - 2.0 * a * phi / mass)
    return out


def trip_moments(p_dest, dm, dist, tables=None):
    """(w_sec, w_km, v_sec, v_km), each (Z, T): the mean and the variance of the seconds and kilometres of one trip that leaves o in
    hour t.  With p~ the row with its residual on ell (the unit row on o for a zero row):
      w = sum p~[d] value[d],  v = sum p~[d] (var_cell[d] + value[d]^2) - w^2 = sum p~[d] var_cell[d] + sum p~[d] (value[d] - w)^2
    for sum p~ = 1; the second form is evaluated (no cancellation: a trip that always takes the same value has v == 0 exactly)."""
    Z, _, T = p_dest.shape
    last, ell, r = tables if tables is not None else R.row_tables(p_dest)
    sec, km = trip_values(dm, dist)
    z = np.arange(Z)
    var_km = _var_cell(dist, 0.1 * np.asarray(dist))
    var_km[z, z] = 0.0
    w = [np.zeros((Z, T)), np.zeros((Z, T))]
    v = [np.zeros((Z, T)), np.zeros((Z, T))]
    for t in range(T):
        pt = np.array(p_dest[:, :, t], dtype=np.float64)
        for o in range(Z):
            if last[t][o] == 0.0:
                pt[o, :] = 0.0
                pt[o, o] = 1.0
            elif ell[t][o] >= 0:
                pt[o, ell[t][o]] += r[t][o]
        mean, sd = dm[:, :, t, 0], dm[:, :, t, 1]
        var_sec = _var_cell(mean, np.where(sd == 0, 0.1 * mean, sd))
        var_sec[z, z] = 0.0
        for which, val, var in ((0, sec[:, :, t], var_sec), (1, km, var_km)):
            m = (pt * val).sum(axis=1)
            w[which][:, t] = m
            v[which][:, t] = (pt * var).sum(axis=1) + (pt * (val - m[:, None]) ** 2).sum(axis=1)
    return w[0], w[1], v[0], v[1]


# ------------------------------------------------------------------------------------------------ the statistical tests' inputs
_STAT = {}


def statistical_inputs(O, density):
    """Z = 67, T = 24, synth_datamatrix(table_seed 11, density), createpdrive(0.1, 0.9, 0.5), createpdestin(e_dest = 2), 2,000 cars per
    zone, with the row tables and the trips' moments: computed once per density and shared; nobody writes to them"""
    if density not in _STAT:
        Z, T, cpz = 67, 24, 2000
        dm, dist = O.synth_datamatrix(Z, T, 11, density=density)
        p_drive = O.createpdrive(dm, dist, Z, T, 0.1, 0.9, 0.5)
        p_dest = O.createpdestin(dm, Z, T, e_dest=2)
        tables = R.row_tables(p_dest)
        _STAT[density] = dict(Z=Z, C=Z * cpz, cpz=cpz, dm=dm, dist=dist, p_drive=p_drive, p_dest=p_dest, tables=tables,
                              moments=trip_moments(p_dest, dm, dist, tables))
    return _STAT[density]


def sums_per_cell(state, trans, Z):
    """(N, S, D), each (Z, T): the drivers that leave o in hour t and their summed trans[:, t, 2] (seconds) and trans[:, t, 3] (km)"""
    state, trans = np.asarray(state), np.asarray(trans)
    T = state.shape[1]
    N, S, D = np.zeros((Z, T)), np.zeros((Z, T)), np.zeros((Z, T))
    for t in range(T):
        drivers = trans[:, t, 0] == 1
        o = state[drivers, t].astype(np.int64) - 1
        N[:, t] = np.bincount(o, minlength=Z)
        S[:, t] = np.bincount(o, weights=trans[drivers, t, 2], minlength=Z)
        D[:, t] = np.bincount(o, weights=trans[drivers, t, 3], minlength=Z)
    return N, S, D


def check_cells(N, S, D, w_sec, w_km, v_sec, v_km, cap, what):
    """|S - N w| <= cap * sqrt(N v) in every cell with a driver (1e-9 relative where v == 0); returns the worst z-scores"""
    worst = []
    for name, got, w, v in (("seconds", S, w_sec, v_sec), ("km", D, w_km, v_km)):
        has = N > 0
        zero = has & (v <= 1e-18 * w * w)                   # (rounding of a variance that is 0: every trip of the cell takes one value)
        assert np.all(np.abs(got[zero] - N[zero] * w[zero]) <= 1e-9 * N[zero] * np.abs(w[zero])), (what, name)
        rnd = has & ~zero
        z = np.abs(got[rnd] - N[rnd] * w[rnd]) / np.sqrt(N[rnd] * v[rnd])
        print(f"{what}: {name}: {int(has.sum())} cells with a driver, {int(zero.sum())} without variance, worst z {z.max():.2f}")
        assert z.max() <= cap, (what, name)
        worst.append(float(z.max()))
    return worst
