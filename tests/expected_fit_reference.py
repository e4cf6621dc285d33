"""include/cpm_expected_fit.h restated in numpy, ONE IEEE f64 operation per step and in the documented order (test infrastructure).

Hours are accumulated in explicit loops (acc = acc + d*d), never with .sum(axis=...): numpy's order of a reduction depends on the
array's shape.  The sums over zones go through zone_sum, the header's ZONE SUM written out; the chain rule's reductions through
chunk_sum.  chain_rule_mp is the chain rule in mpmath with the magnitude sums of the header's bound.

Layout: parking / driving / measured / w_sec are (T, Z) arrays here, hour-major like the device tensors.
"""
import mpmath
import numpy as np

mpmath.mp.dps = 50

FIT_WORDS = 16
EPS = 2.0 ** -53


def _tree64(v):
    """the wave tree: v[l] = v[l] + v[l + o] for o = 32 .. 1 over groups of 64 (last axis 64)"""
    for o in (32, 16, 8, 4, 2, 1):
        v = v[..., :o] + v[..., o:2 * o]
    return v[..., 0]


def _block_sum(v, block=256):
    """(nblocks,) sums of consecutive blocks of 256 along the last axis (absent words 0.0): four trees, then ((g0 + g1) + g2) + g3"""
    n = v.shape[-1]
    nb = (n + block - 1) // block
    pad = np.zeros(v.shape[:-1] + (nb * block,))
    pad[..., :n] = v
    g = _tree64(pad.reshape(v.shape[:-1] + (nb, 4, 64)))
    return ((g[..., 0] + g[..., 1]) + g[..., 2]) + g[..., 3]


def _lane_sum(parts):
    """a fleet's partial sums: lane l adds parts l, l + 64, ... in ascending order from 0.0, then the tree"""
    n = parts.shape[-1]
    rounds = (n + 63) // 64
    pad = np.zeros(parts.shape[:-1] + (rounds * 64,))
    pad[..., :n] = parts
    pad = pad.reshape(parts.shape[:-1] + (rounds, 64))
    acc = np.zeros(parts.shape[:-1] + (64,))
    for r in range(rounds):
        acc = acc + pad[..., r, :]
    return _tree64(acc)


def zone_sum(v):
    """ZONE SUM of the header along the last axis (Z)"""
    return _lane_sum(_block_sum(np.asarray(v, dtype=np.float64)))


def chunk_sum(v):
    """the chain rule's two-stage sum of a flat [T * Z] array of terms (0.0 where a term is not formed): chunks of 1,024 words, thread
    i adds words i, i + 256, i + 512, i + 768 from 0.0, the block tree, then the chunks as the blocks of ZONE SUM"""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    n = v.shape[0]
    nc = (n + 1023) // 1024
    pad = np.zeros(nc * 1024)
    pad[:n] = v
    pad = pad.reshape(nc, 4, 256)
    acc = np.zeros((nc, 256))
    for j in range(4):
        acc = acc + pad[:, j, :]
    return float(_lane_sum(_block_sum(acc)[:, 0]))


def _first_extremes(v):
    """(lo, hi, imin, imax) along axis 0, the first index that attains each (strict comparisons, ascending)"""
    lo, hi = v[0].copy(), v[0].copy()
    imin, imax = np.zeros(v.shape[1:], dtype=np.int64), np.zeros(v.shape[1:], dtype=np.int64)
    for t in range(1, v.shape[0]):
        less, more = v[t] < lo, v[t] > hi
        lo, imin = np.where(less, v[t], lo), np.where(less, t, imin)
        hi, imax = np.where(more, v[t], hi), np.where(more, t, imax)
    return lo, hi, imin, imax


def fit_reference(parking, driving, weights, measured_activity=None, measured_parking=None, w_sec=None, total_seconds=None):
    """One fleet.  parking, driving: (T, Z).  weights: (w_act, w_park, w_adrive).  total_seconds: cpm_expected_travel_dev's total on
    these densities (the device's own bits), needed where A_drive is wanted.  Returns dict(F, activity_error, parking_error, A_drive,
    n_valid, traffic_activity (T,), g_parking, g_driving (T, Z), e_z (Z,), valid (Z,), a (T,) the hour sums, ga (T,))."""
    p, x = np.asarray(parking, dtype=np.float64), np.asarray(driving, dtype=np.float64)
    T, Z = p.shape
    n = float(T)
    w_act, w_park, w_adr = (float(w) for w in weights)
    nan = float("nan")
    out = {}
    with np.errstate(all="ignore"):
        # traffic activity
        a = np.array([zone_sum(x[t]) for t in range(T)])
        lo, hi, imin, imax = (v.item() for v in _first_extremes(a.reshape(T, 1)))
        rng = hi - lo
        ga = np.zeros(T)
        act = np.full(T, nan)
        act_err = nan
        if rng != 0.0:
            act = np.array([(a[t] - lo) / rng for t in range(T)])
            if measured_activity is not None:
                m = np.asarray(measured_activity, dtype=np.float64)
                acc = s1 = s2 = 0.0
                for t in range(T):
                    d = act[t] - m[t]
                    acc = acc + d * d
                    e = (2.0 * d) / n
                    s1 = s1 + e * (1.0 - act[t])
                    s2 = s2 + e * act[t]
                    ga[t] = e / rng
                act_err = acc / n
                ga[imin] = ga[imin] - s1 / rng
                ga[imax] = ga[imax] - s2 / rng
                ga = w_act * ga
        out.update(a=a, traffic_activity=act, activity_error=act_err, ga=ga)

        # parking error
        zlo, zhi, zmin, zmax = _first_extremes(p)
        valid = np.zeros(Z, dtype=bool)
        e_z, g_park = np.zeros(Z), np.zeros((T, Z))
        if measured_parking is not None:
            mp_ = np.asarray(measured_parking, dtype=np.float64)
            msum = np.zeros(Z)
            for t in range(T):
                msum = msum + mp_[t]
            valid = (msum != 0) & (zlo != zhi)
            zr = zhi - zlo
            acc, s1, s2 = np.zeros(Z), np.zeros(Z), np.zeros(Z)
            es = np.zeros((T, Z))
            for t in range(T):
                v = (p[t] - zlo) / zr
                d = v - mp_[t]
                acc = acc + d * d
                es[t] = (2.0 * d) / n
                s1 = s1 + es[t] * (1.0 - v)
                s2 = s2 + es[t] * v
            e_z = np.where(valid, acc / n, 0.0)
        n_valid = int(valid.sum())
        park_err = nan if n_valid == 0 else float(zone_sum(e_z)) / float(n_valid)
        if n_valid and w_park != 0.0:
            for t in range(T):
                g = es[t] / zr
                g = np.where(zmin == t, g - s1 / zr, g)
                g = np.where(zmax == t, g - s2 / zr, g)
                g = g / float(n_valid)
                g_park[t] = np.where(valid, w_park * g, 0.0)
        out.update(parking_error=park_err, n_valid=n_valid, e_z=e_z, valid=valid, g_parking=g_park)

        a_drive = nan if total_seconds is None else float(total_seconds) / (n * 3600.0)
        out["A_drive"] = a_drive
        f = 0.0
        if w_act != 0.0:
            f = f + w_act * act_err
        if w_park != 0.0:
            f = f + w_park * park_err
        if w_adr != 0.0:
            f = f + w_adr * a_drive
        out["F"] = f

        g_drv = np.zeros((T, Z))
        if w_act != 0.0:
            g_drv = np.broadcast_to(ga[:, None], (T, Z)).copy()   # (assigned, not added to 0.0: a -0.0 stays -0.0)
        if w_adr != 0.0:
            g_drv = g_drv + w_adr * (np.asarray(w_sec, dtype=np.float64) / (n * 3600.0))
        out["g_driving"] = g_drv
    return out


def s_table(mean_sum):
    """(s (T, Z), on (Z,)) from the context's mean_sum (T, Z): (mean_sum - mn) / (mx - mn) with Julia's max / min (NaN if any), as
    k_pdrive_final forms it; on: mx > 0."""
    m = np.asarray(mean_sum, dtype=np.float64)
    with np.errstate(all="ignore"):
        bad = np.isnan(m).any(axis=0)
        mx, mn = np.where(bad, np.nan, m.max(axis=0)), np.where(bad, np.nan, m.min(axis=0))
        s = (m - mn) / (mx - mn)
    return s, mx > 0


def chain_rule_mp(grad_p_drive, s, on, p_min, p_max, e_drive, grad_dest=None, driving=None, dw_sec=None, w_adrive=0.0):
    """The chain rule of the header in mpmath on f64 inputs: (values, magnitudes), each (d_p_min, d_p_max, d_e_drive, d_e_dest);
    d_e_dest None without grad_dest.  grad_p_drive, s, grad_dest, driving, dw_sec: (T, Z); on: (Z,).  The magnitudes are the M of the
    header's bound: sum |g| for words 5 and 6, the sum of the terms' absolute values for words 7 and 8."""
    g = np.asarray(grad_p_drive, dtype=np.float64)
    T, Z = g.shape
    mpf = mpmath.mpf
    v = [mpf(0)] * 3
    mag = [mpf(0)] * 3
    e, span = mpf(float(e_drive)), mpf(float(p_max)) - mpf(float(p_min))
    for t, z in zip(*np.nonzero(g)):
        if not on[z]:
            continue
        gg, ss = mpf(float(g[t, z])), mpf(float(s[t, z]))
        se = mpmath.sqrt(ss) if e_drive == 0.5 else ss if e_drive == 1.0 else ss * ss if e_drive == 2.0 else (mpmath.power(ss, e) if ss > 0 else
                                                                                                               (mpf(0) if e > 0 else mpf(1)))
        v[0] += gg * (1 - se)
        v[1] += gg * se
        mag[0] += abs(gg)
        mag[1] += abs(gg)
        if ss > 0:
            term = gg * span * se * mpmath.log(ss)
            v[2] += term
            mag[2] += abs(term)
    d = m = None
    if grad_dest is not None:
        gd = np.asarray(grad_dest, dtype=np.float64)
        d, m = mpf(0), mpf(0)
        for val in gd.reshape(-1):
            d += mpf(float(val))
            m += abs(mpf(float(val)))
        if w_adrive != 0.0:
            xs, dw = np.asarray(driving, dtype=np.float64).reshape(-1), np.asarray(dw_sec, dtype=np.float64).reshape(-1)
            acc, am = mpf(0), mpf(0)
            for a_, b_ in zip(xs, dw):
                acc += mpf(float(a_)) * mpf(float(b_))
                am += abs(mpf(float(a_)) * mpf(float(b_)))
            scale = mpf(float(w_adrive)) / (mpf(T) * 3600)
            d += scale * acc
            m += abs(scale) * am
    return (v[0], v[1], v[2], d), (mag[0], mag[1], mag[2], m)


def chain_bound(T, Z):
    """the header's constant of words 5 .. 8: (96 + ceil(T * Z / 65536)) * 2^-53"""
    return (96 + -(-T * Z // 65536)) * EPS


def zone_sum_bound(Z):
    """the header's bound of a ZONE SUM of non-negative terms, relative"""
    return (16 + -(-Z // 16384)) * EPS
