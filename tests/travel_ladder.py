"""Datamatrices and probes that take the travel-time sampler through every branch of its f64 kit (csrc/cpm_rng.h; the CPU
restatement: orc_erf, orc_ppnd, orc_truncnormal_* under oracle/).  Not a conftest: imported by tests/test_travel_kit.py; numpy and
the oracle only, no GPU.

The datamatrices of the other tests hold standard deviations of 10 .. 40 % of the mean, or none (which becomes 10 %): the window
[0.9 mu, 1.1 mu] is then +-0.25 .. 1 sigma wide, which reaches two of det_erf's four branches and only the central rational of ppnd.
`ladder_datamatrix` keeps the means of O.synth_datamatrix and replaces every standard deviation by mean x rung, the rung drawn per cell
from RUNGS.  With a = 0.1 mu / sigma = 0.1 / rung the window's half width in sigmas, and x = a / sqrt 2 the argument of erf:

  rung      a        x       erf branch          the draw
  4         0.025    0.018   1 (x <= 0.46875)    central
  1         0.1      0.071   1                   central
  0.4       0.25     0.18    1                   central
  0.1       1        0.71    2 (x <= 4)          central
  0.0695    1.439    1.017   2                   central: |q| <= mass / 2 = 0.42494, just inside 0.425
  0.06      1.667    1.18    2                   tail from |u - 1/2| > 0.47 on (mass 0.904)
  0.03      3.33     2.36    2                   tail
  0.02      5        3.54    2                   tail
  0.015     6.67     4.71    3 (4 < x < 6)       tail; mass 1 - 2.6e-11
  0.0118    8.47     5.99    3                   tail; just below the x >= 6 short cut
  0.011     9.09     6.43    4 (x >= 6: 1.0)     tail; mass exactly 1
  0.001     100      70.7    4                   tail
  1e-6      1e5      7e4     4                   tail
  0         --       --      2                   no standard deviation: a tenth of the mean (src/resampling.jl:65-67), a = 1
  -0.2      -0.5     --      (erf of x < 0: 0)   sigma <= 0: the draw is the mean
  +inf      0        0       1 (erf(0) = 0)      mass 0: the draw is the mean

NaN means are out of scope and kept out of every fixture here: llrint(NaN) on the host and the device's conversion of NaN to an
integer differ, and the reference would have failed on such a cell long before (a NaN mean makes createpdrive's extrema NaN).  For
the same reason a mean of 0 takes +inf, not 0 x inf = NaN, as its "infinite" standard deviation in `probe_cells`.  orc_ppnd and the
device's ppnd also differ on a NaN argument (9 against NaN: the device tests |q| > 0.425, the oracle |q| <= 0.425); no draw can pass
one, since erf of NaN is 0 and a uniform is never NaN, so ppnd's probes hold no NaN either.

`census` counts trips per branch from the reference's per-car record, `draw_census` does the same for given (k53, mean, sd) and also
tells the two rationals of the tail, the val = 9 exit and the two clamps apart, which no resample reaches."""
import ctypes as C
import math

import numpy as np

RUNGS = (4.0, 1.0, 0.4, 0.1, 0.0695, 0.06, 0.03, 0.02, 0.015, 0.0118, 0.011, 0.001, 1e-6, 0.0, -0.2, math.inf)
LADDER_SEED = 0x1ADDE2
CLASSES = ("same_zone", "sigma_le_0", "mass_0", "erf_1", "erf_2", "erf_3", "erf_4", "central", "tail")
SQRT_HALF = 7.0710678118654752440e-1            # the constant of truncnormal_mass
E25 = math.exp(-25.0)                           # ppnd_tail switches rationals at sqrt(-ln r) = 5


def ladder_sd(dm, seed, keep_sd0=False):
    """Replaces dm[..., 1] in place by mean x rung on every cell that holds a mean, the rung drawn per cell; returns the (Z, Z, T)
    array of rung indices, -1 where the cell holds no mean (those cells keep their standard deviation).  keep_sd0: cells with a mean
    and no standard deviation stay as they are and count as rung 0."""
    mean = dm[..., 0]
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, len(RUNGS), size=mean.shape)
    if keep_sd0:
        idx[(mean != 0) & (dm[..., 1] == 0)] = RUNGS.index(0.0)
    rung = np.asarray(RUNGS)[idx]
    with np.errstate(invalid="ignore"):
        sd = np.where(np.isinf(rung), np.inf, mean * rung)
    held = mean != 0
    dm[..., 1][held] = sd[held]
    assert not np.isnan(dm).any()
    return np.where(held, idx, -1)


def ladder_datamatrix(O, Z, T, seed, density):
    """(datamatrix (Z, Z, T, 2), dist (Z, Z), rung index (Z, Z, T)): O.synth_datamatrix(Z, T, seed, density) with its standard
    deviations replaced by the ladder (see the module's docstring).  The generator leaves the diagonal empty; here every pair (z, z)
    gets a mean in every hour, so that createpdestin gives the diagonal weight and some trips end where they began (300 s and no
    draw, src/resampling.jl:58-60): the class `same_zone` of the census."""
    dm, dist = O.synth_datamatrix(Z, T, seed, density=density)
    rng = np.random.default_rng(LADDER_SEED ^ seed ^ 0xD1A6)
    z = np.arange(Z)
    dm[z, z, :, 0] = 300.0 + 2100.0 * rng.random((Z, T))         # (the generator's range of means)
    idx = ladder_sd(dm, LADDER_SEED ^ seed)
    return np.asfortranarray(dm), dist, idx


# ------------------------------------------------------------------------------------------------ the oracle's kit, vectorised
def _vec(fn, *cols):
    cols = [np.ascontiguousarray(c, dtype=np.float64).reshape(-1) for c in cols]
    return np.fromiter((fn(*(float(c[i]) for c in cols)) for i in range(cols[0].shape[0])), dtype=np.float64, count=cols[0].shape[0])


def orc(O, name, *cols):
    """orc_<name> of oracle/cpm_oracle.c element by element (float64 array)"""
    return _vec(getattr(O.lib(), "orc_" + name), *cols)


def orc_exp_neg(O, y):
    return _vec(O.lib().orc_exp_neg, y)


def sigma_of(mean, sd):
    """the sigma the kernels draw with: the standard deviation, or a tenth of the mean where the data hold none (src/resampling.jl:65-67)"""
    mean, sd = np.asarray(mean, dtype=np.float64), np.asarray(sd, dtype=np.float64)
    return np.where(sd == 0, 0.1 * mean, sd)


def orc_draw(O, k53, mean, sd):
    """(draw, mass, q16) of the oracle for cells (mean, sd) and u = k53 * 2^-53: what cpm_debug_travel_draw must return bit for bit.
    q16 = llrint(draw * 65536): np.rint rounds to nearest even like llrint in the default rounding mode, and every product here is
    far below 2^63."""
    s1 = sigma_of(mean, sd)
    mass = orc(O, "truncnormal_mass", mean, s1)
    u = np.asarray(k53, dtype=np.uint64).astype(np.float64) * 2.0 ** -53           # exact: k < 2^53
    draw = orc(O, "truncnormal_draw", u, mean, s1, mass)
    return draw, mass, np.rint(draw * 65536.0).astype(np.int64)


# ------------------------------------------------------------------------------------------------ census
def draw_census(O, k53, mean, sd):
    """Which statements of truncnormal_mass / truncnormal_draw / ppnd the draws (k53, mean, sd) execute, restated from the oracle's
    text; a dict of boolean arrays.  sigma_le_0 and mass_0 return the mean; the others are drawn: erf_1 .. erf_4 by the branch of
    det_erf that gave the cell's mass, central / tail_r_le_5 / tail_r_gt_5 / val_9 by the branch of ppnd, clamp_lo / clamp_hi where
    mu + sigma z fell outside the window."""
    mean = np.asarray(mean, dtype=np.float64)
    s1 = sigma_of(mean, sd)
    with np.errstate(all="ignore"):
        x = ((0.1 * mean) / s1) * SQRT_HALF
    mass = orc(O, "truncnormal_mass", mean, s1)
    u = np.asarray(k53, dtype=np.uint64).astype(np.float64) * 2.0 ** -53
    nosig = ~(s1 > 0.0)
    nomass = ~nosig & ~(mass > 0.0)
    drawn = ~nosig & ~nomass
    q = (u - 0.5) * mass
    aq = np.abs(q)
    r = 0.5 - aq
    tail = drawn & (aq > 0.425)
    val9 = tail & ~(r > 0.0)
    with np.errstate(all="ignore"):
        s = orc(O, "sqrt", -orc(O, "log", np.where(tail & ~val9, r, 0.5)))
        z = orc(O, "ppnd", np.where(drawn, q, 0.0))
        raw = mean + s1 * z
    return dict(sigma_le_0=nosig, mass_0=nomass,
                erf_1=drawn & (x <= 0.46875), erf_2=drawn & (x > 0.46875) & (x <= 4.0), erf_3=drawn & (x > 4.0) & (x < 6.0), erf_4=drawn & (x >= 6.0),
                central=drawn & ~tail, tail=tail, tail_r_le_5=tail & ~val9 & (s <= 5.0), tail_r_gt_5=tail & ~val9 & (s > 5.0), val_9=val9,
                clamp_lo=drawn & (raw < 0.9 * mean), clamp_hi=drawn & (raw > 1.1 * mean))


def trips_of_state(state):
    """(car, hour, origin, destination), 0-based, of the trips between DIFFERENT zones that a state matrix (C x T, 1-based zones, as
    fast_run(..., want_state=True) returns it) shows: hours 0 .. T - 2, since the destinations of hour T - 1 are in no column.  Every
    one of them took a travel-time draw; trips inside a zone (300 s, no draw) and the last hour's do not appear."""
    st = np.asarray(state)
    car, hour = np.nonzero(st[:, 1:] != st[:, :-1])
    return car, hour, st[car, hour] - 1, st[car, hour + 1] - 1


def trips_of_trans(state, trans):
    """the same from the reference's matrices (O.resampling): every trip of every hour, those inside a zone included"""
    car, hour = np.nonzero(np.asarray(trans)[:, :, 0] == 1)
    return car, hour, np.asarray(state)[car, hour] - 1, np.asarray(trans)[car, hour, 1].astype(np.int64) - 1


def trip_uniforms(O, seed, car, hour, T, car_offset=0):
    """the uniform of each trip's travel-time draw: the first of Philox stream 1 at step T - 1 + hour (include/cpm.h, RNG contract)"""
    L = O.lib()
    a, b = C.c_double(), C.c_double()
    out = np.empty(len(car))
    for i, (c, h) in enumerate(zip(car.tolist(), hour.tolist())):
        L.orc_uniforms(seed, car_offset + c, T - 1 + h, 1, C.byref(a), C.byref(b))
        out[i] = a.value
    return out


def census(O, dm, trips, seed=None, T=None):
    """Trips per class of CLASSES (a dict of counts) from (car, hour, origin, destination).  same_zone: 300 s, no draw; the other
    classes as in draw_census.  central / tail need the trips' uniforms: counted when `seed` is given, else absent."""
    car, hour, o, d = trips
    same = o == d
    mean, sd = dm[o, d, hour, 0], dm[o, d, hour, 1]
    k = np.zeros(len(car), dtype=np.uint64)
    if seed is not None:
        k = np.rint(trip_uniforms(O, seed, car, hour, T if T is not None else dm.shape[2]) * 2.0 ** 53).astype(np.uint64)
    dc = draw_census(O, k, mean, sd)
    out = dict(same_zone=int(same.sum()))
    for name in CLASSES[1:]:
        if name in ("central", "tail") and seed is None:
            continue
        out[name] = int((dc[name] & ~same).sum())
    return out


def rung_trips(rung_idx, trips):
    """trips per rung of RUNGS (trips between different zones on cells that hold a mean)"""
    car, hour, o, d = trips
    idx = rung_idx[o, d, hour]
    return np.bincount(idx[(o != d) & (idx >= 0)], minlength=len(RUNGS))


# ------------------------------------------------------------------------------------------------ probes
def with_neighbours(x, n=2):
    """x and its n neighbours on either side (nextafter), ascending"""
    out = [float(x)]
    lo = hi = float(x)
    for _ in range(n):
        lo, hi = math.nextafter(lo, -math.inf), math.nextafter(hi, math.inf)
        out = [lo] + out + [hi]
    return out


TINY, HUGE = 2.2250738585072014e-308, 1.7976931348623157e308       # the smallest and the largest normal


def kit_probes():
    """The arguments of every function of the kit, as float64 arrays: dict(erf, log, sqrt, ppnd, exp_neg).  ppnd's are q = +-(1/2 - r)."""
    erf = sum((with_neighbours(v) for v in (0.46875, 4.0, 6.0)), []) + [5e-324, 1e-200, 7.0, 1e300, -1.0, math.nan]
    erf = np.concatenate([erf, np.linspace(0.01, 6.5, 2000)])
    pos = sum((with_neighbours(v) for v in (0.5, 1.0, 1.4142135623730951, 2.0)), []) + [2.0 ** -53, 2.0 ** -54, TINY, HUGE]
    pos = np.concatenate([pos, 10.0 ** np.linspace(-307, 308, 1500)])
    r = np.concatenate([[2.0 ** -53, 2.0 ** -54, 0.0], with_neighbours(E25), 10.0 ** np.linspace(-16, math.log10(0.075), 1500)])
    q = np.concatenate([with_neighbours(0.425), 0.5 - r, np.linspace(-0.425, 0.425, 2001)])
    q = np.concatenate([q, -q])
    exp_neg = np.concatenate([np.linspace(0, 2, 201), np.linspace(2, 60, 59), [100.0, 700.0, 744.0, 800.0]])
    return dict(erf=np.asarray(erf), log=pos, sqrt=pos, ppnd=q, exp_neg=exp_neg)


PROBE_MEANS = (0.0, 62.72, 961.0, 2380.13, 1e-3, 1e7)


def mass_one_edge(O, mean):
    """(sd_below, sd_at): adjacent doubles with orc_truncnormal_mass(mean, sd_at) == 1.0 and < 1.0 at sd_below's other side, i.e. the
    largest standard deviation (found by bisection between mean x 0.011 and mean x 0.015) at which the mass rounds to exactly 1.0, and
    its upper neighbour, at which it does not."""
    L = O.lib()
    lo, hi = mean * 0.011, mean * 0.015
    assert L.orc_truncnormal_mass(mean, lo) == 1.0 and L.orc_truncnormal_mass(mean, hi) < 1.0
    while math.nextafter(lo, math.inf) < hi:
        mid = lo + (hi - lo) / 2
        if L.orc_truncnormal_mass(mean, mid) == 1.0:
            lo = mid
        else:
            hi = mid
    return hi, lo


def probe_cells(O):
    """[(mean, sd)]: PROBE_MEANS x (every rung of RUNGS and the two standard deviations of mass_one_edge)"""
    cells = []
    for mean in PROBE_MEANS:
        for rung in RUNGS:
            cells.append((mean, math.inf if math.isinf(rung) else mean * rung))
        if mean > 0:
            cells.extend((mean, sd) for sd in mass_one_edge(O, mean))
    return cells


# The upper clamp `x = hi` is not in the census: nothing reaches it.  It needs sigma > 0 and mass > 0, hence mu > 0 (a negative mean
# gives a < 0 and mass 0).  Then hi = fl(1.1 mu) lies ABOVE 1.1 mu (the double 1.1 is 1.1 + 8.9e-17), u <= 1 - 2^-53 keeps z below a
# -- there is no u = 1 to mirror the val = 9 exit of u = 0 --, and mu + sigma z would have to overshoot by 9 ulps of z.  A search over
# 400,000 random (mean, sd) at k = 2^53 - 1 found x == hi often and x > hi never.  The lower clamp is easy: lo = fl(0.9 mu) lies
# above 0.9 mu as well, so u = 0 lands on or below it.


def probe_k53(mass, rng):
    """The 53-bit draws for a cell of the given mass: the ends and the middle of the range with neighbours, the k on either side of
    |u - 1/2| mass = 0.425 (where ppnd goes out of line) and of 1/2 - |u - 1/2| mass = e^-25 (where ppnd_tail changes rationals),
    both signs, and 300 random k.  Sorted and distinct."""
    top = 2 ** 53
    ks = [0, 1, 2, 2 ** 52 - 1, 2 ** 52, 2 ** 52 + 1, top - 2, top - 1]
    if mass > 0.0:
        for edge in (0.425, 0.5 - E25):
            h = edge / mass                                  # |u - 1/2| at the edge
            if h < 0.5:
                c = int(math.floor(h * top))
                for d in (-2, -1, 0, 1, 2, 3):
                    ks += [2 ** 52 + c + d, 2 ** 52 - c - d]
    ks += rng.integers(0, top, size=300).tolist()
    return np.unique(np.clip(np.asarray(ks, dtype=np.int64), 0, top - 1)).astype(np.uint64)


def draw_probes(O, seed=0xD2A3):
    """(k53, mean, sd) of the whole probe product, cell by cell (each cell's k ascending), and the index ranges of the cells"""
    rng = np.random.default_rng(seed)
    L = O.lib()
    ks, ms, ss, spans, at = [], [], [], [], 0
    for mean, sd in probe_cells(O):
        s1 = 0.1 * mean if sd == 0 else sd
        k = probe_k53(L.orc_truncnormal_mass(mean, s1), rng)
        ks.append(k)
        ms.append(np.full(len(k), mean))
        ss.append(np.full(len(k), sd))
        spans.append((at, at + len(k)))
        at += len(k)
    return np.concatenate(ks), np.concatenate(ms), np.concatenate(ss), spans
