"""Model selection on top of the sampler path (BASELINE.json configs[4]).

The reference tunes its four hyper-parameters with three sequential 1-D searches that live only
in the notebook (README.md:947-2435 of the reference): e_drive against the measured circadian
traffic activity (README.md:1134-1314), (p_min, p_max) against the share of life spent driving
A_set = 0.07 (README.md:1436-1676, clamp = src/correctparameters.jl:3-22) and e_dest against the
measured parking densities (README.md:2062-2276).  Every iteration = rebuild one table -> reset
state_matrix[:,1] = initial_state (the IVP is NOT re-run: README.md:1180,1549,2119) -> 24-hour
resample -> histogram -> scalar error.  Here one iteration is one `evaluate()` on the device:
cpm_build_p_drive / cpm_build_p_dest + cpm_resample from the cached post-IVP state.

`grid_sweep` is the build's generalisation named by BASELINE.json: a grid of
(e_drive, p_min, p_max, e_dest) points, dealt round-robin over the ranks of a torch.distributed
job (one process per GPU).  Points are independent, so there is NO collective on the data path;
the per-point scalars are gathered at the end.  Points sharing e_dest share the CDF (the
3 GB table is rebuilt only when e_dest changes), so each rank sorts its points by e_dest.

The reference's measured validation data (traffic_activity_measured.jld2, parking_density_measured.jld2)
are not in the repository; callers pass their own vectors (tests use synthetic ones).
"""
import zlib
from dataclasses import dataclass, field

import numpy as np

from .reference_api import correctparameters


# ------------------------------------------------------------------ objectives (host scalars)
def traffic_activity(driving):
    """min-max normalised column sums of the driving counts (src/saveresults.jl:23-28)."""
    a = np.asarray(driving, dtype=np.float64).sum(axis=0)
    with np.errstate(all="ignore"):
        return (a - a.min()) / (a.max() - a.min())


def traffic_activity_error(activity, measured):
    """mean squared error over the 24 hours (README.md:1279-1283)."""
    d = np.asarray(measured, dtype=np.float64) - np.asarray(activity, dtype=np.float64)
    return float(np.sum(d * d) / d.size)


def a_drive(sum_tt_q16, C, T=24):
    """share of life spent driving (src/averagedrivingtime.jl:10) from the fixed-point time sum."""
    return (sum_tt_q16 / 65536.0) / (C * T * 60 * 60)


def parking_density_error(parking, C, measured):
    """README.md:2219-2244: per-zone min-max normalisation over the day (zones with max == min are
    left as they are), MSE over 24 h for zones that are measured (row sum != 0) and not flat, averaged
    over the validated zones.  (Evaluated hour-major -- the count tensor's own layout, Z contiguous -- so that a point of
    the sweep costs the host tens of microseconds, not half a millisecond: with two contexts in flight the host is what
    a point waits for.)"""
    p = np.asarray(parking).T / float(C)                     # (T, Z); a view of a Julia-ordered (Z, T) array is contiguous this way
    m = np.asarray(measured, dtype=np.float64).T
    lo, hi = p.min(axis=0), p.max(axis=0)
    flat = hi == lo
    valid = (m.sum(axis=0) != 0) & ~flat
    if not valid.any():
        return float("nan")
    if not valid.all():
        p, m, lo, hi = p[:, valid], m[:, valid], lo[valid], hi[valid]
    pn = (p - lo) / (hi - lo)
    d = pn - m
    err = (d * d).sum(axis=0) / p.shape[0]
    return float(err.sum() / err.size)


def expected_objectives(parking_density, driving_density, measured_activity=None, measured_parking=None, seconds=None):
    """The sweep's noise-free objectives from Sampler.expected()'s (Z, T) densities: the functions above with the densities in
    place of counts / C.  Returns dict(traffic_activity (T,), and activity_error / parking_error where the measured data is given).
    seconds: Sampler.expected_travel()'s (Z, T) "seconds" (summed here) or its "total_seconds" (a scalar, used as it is) -- the result
    then also holds A_drive = total / (T * 3600), the share of the day a car drives (src/averagedrivingtime.jl:10) without the
    sampling noise; without it the result is what it was before that argument existed."""
    out = {"traffic_activity": traffic_activity(driving_density)}
    if measured_activity is not None:
        out["activity_error"] = traffic_activity_error(out["traffic_activity"], measured_activity)
    if measured_parking is not None:
        out["parking_error"] = parking_density_error(parking_density, 1, measured_parking)
    if seconds is not None:
        total = float(seconds) if np.ndim(seconds) == 0 else float(np.asarray(seconds, dtype=np.float64).sum())
        out["A_drive"] = total / (np.asarray(driving_density).shape[1] * 3600.0)
    return out


def count_zscores(parking, driving, ev):
    """Per-cell z-scores (N - mean) / sqrt(var) of resample()'s (Z, T) count arrays against Sampler.expected_var()'s dict ev (with
    start = the cars per zone the resample started from: cars_per_zone of init_states, or np.bincount(get_state() - 1,
    minlength=Z)).  Returns dict(parking, driving: (Z, T) float64, NaN where the variance is 0; parking_fixed, driving_fixed: (Z, T)
    bool, the cells of variance 0, reported apart; parking_fixed_ok, driving_fixed_ok: bool, every such count equals its mean, as
    it must)."""
    out = {}
    for name, n in (("parking", parking), ("driving", driving)):
        n = np.asarray(n, dtype=np.float64)
        mean = np.asarray(ev["mean_" + name], dtype=np.float64)
        var = np.asarray(ev["var_" + name], dtype=np.float64)
        if n.shape != mean.shape or var.shape != mean.shape:
            raise ValueError(f"count_zscores: {name} counts {n.shape}, mean {mean.shape}, variance {var.shape}")
        if (var < 0).any() or np.isnan(var).any():
            raise ValueError(f"count_zscores: a {name} variance is negative or NaN")
        fixed = var == 0
        z = np.full(mean.shape, np.nan)
        np.divide(n - mean, np.sqrt(var), out=z, where=~fixed)
        out[name] = z
        out[name + "_fixed"] = fixed
        out[name + "_fixed_ok"] = bool((n[fixed] == mean[fixed]).all())
    return out


# ------------------------------------------------------------------ the seed noise of the objectives (Sampler.expected_linear_var)
def activity_noise(sampler, start, ivp=False, sparse=False):
    """Exact mean and variance over the seed of driving_sum[t] = sum over z of resample()'s driving[z, t], for every hour: T
    functionals with B_k = 1 on hour k (Sampler.expected_linear_var).  start: (Z,) cars per start zone, or None (1 per zone).  Returns
    dict(mean (T,), var (T,)).  T is at most CPM_MAX_BATCH.  sparse: Sampler.expected_linear_var(sparse=True), the same bits from the
    compact rows of sparse tables."""
    Z, T = sampler.Z, sampler.T
    b = np.zeros((Z, T, T), order="F")
    for k in range(T):
        b[:, k, k] = 1.0
    return sampler.expected_linear_var(np.zeros((Z, T, T), order="F"), b, start=start, ivp=ivp, sparse=sparse)


def objective_noise_functionals(densities, C, measured_activity=None, measured_parking=None):
    """The coefficient arrays objective_noise() passes to Sampler.expected_linear_var: (names, a_parking (Z, T, K), b_driving
    (Z, T, K)), the objectives' gradients at the expected densities over C."""
    parking, driving = (np.asarray(d, dtype=np.float64) for d in densities)
    names, a, b = [], [], []
    zero = np.zeros(parking.shape, order="F")
    if measured_activity is not None:
        names.append("activity_error")
        a.append(zero)
        b.append(traffic_activity_error_grad(driving, measured_activity) / float(C))
    if measured_parking is not None:
        names.append("parking_error")
        a.append(parking_density_error_grad(parking, measured_parking) / float(C))
        b.append(zero)
    if not names:
        raise ValueError("objective_noise: neither measured_activity nor measured_parking is given")
    return names, np.asfortranarray(np.stack(a, axis=2)), np.asfortranarray(np.stack(b, axis=2))


def objective_noise(sampler, densities, C, start, measured_activity=None, measured_parking=None, ivp=False, sparse=False):
    """The FIRST-ORDER (delta-method) standard deviation over the seed of activity_error and parking_error of ONE resample of C cars:
    the objective is linearised at the expected densities (parking, driving) = densities (Sampler.expected() with pi_0 = start / C),
    its gradient (traffic_activity_error_grad / parking_density_error_grad, per density) over C is a linear functional of the counts,
    and Sampler.expected_linear_var gives that functional's exact variance.  Exact only for an objective that is linear in the
    counts; the errors are quadratic and min-max normalised, so this is the leading term for large C, and it is 0 where the gradient
    vanishes (a perfect fit), where the true spread is of second order.  start: (Z,) cars per start zone (sum C), or None.  Returns
    dict(activity_error_std, parking_error_std) for the objectives whose measured data is given.  sparse: as in activity_noise()."""
    names, a, b = objective_noise_functionals(densities, C, measured_activity, measured_parking)
    r = sampler.expected_linear_var(a, b, start=start, ivp=ivp, sparse=sparse)
    return {name + "_std": float(np.sqrt(r["var"][k])) for k, name in enumerate(names)}


def travel_noise(sampler, start, ivp=False, sparse=False):
    """Exact mean and standard deviation over the seed of the travel of ONE resample(travel=True): the total seconds, the total
    kilometres and A_drive = total seconds / (C * T * 3600), the formula of a_drive(), with C = sum(start)
    (Sampler.expected_travel_var with S = 1, and with D = 1).  start: (Z,) cars per start zone.  Returns dict(seconds_mean,
    seconds_std, km_mean, km_std, A_drive_mean, A_drive_std).  sparse: Sampler.expected_travel_var(sparse=True), the same bits from the
    compact rows of sparse tables under its condition on the cells that are not stored."""
    Z, T = sampler.Z, sampler.T
    zero = np.zeros((Z, T, 2), order="F")
    s, d = np.zeros((Z, T, 2), order="F"), np.zeros((Z, T, 2), order="F")
    s[:, :, 0] = 1.0
    d[:, :, 1] = 1.0
    r = sampler.expected_travel_var(zero, zero, s, d, start=start, ivp=ivp, sparse=sparse)
    C = float(np.asarray(start, dtype=np.float64).sum())
    std = np.sqrt(r["var"])
    return {"seconds_mean": float(r["mean"][0]), "seconds_std": float(std[0]), "km_mean": float(r["mean"][1]), "km_std": float(std[1]),
            "A_drive_mean": float(r["mean"][0]) / (C * T * 60 * 60), "A_drive_std": float(std[0]) / (C * T * 60 * 60)}


# ------------------------------------------------------------------ host cotangents of the noise-free objectives (for Sampler.expected_grad)
def _minmax_mse_grad(v, m, axis):
    """d/dv of mean over `axis` of ((v - lo) / (hi - lo) - m)^2, lo / hi the minimum / maximum of v along `axis` (the first one where
    several tie): the direct term, and the terms through lo and hi at the argmin and the argmax.  Slices with hi == lo give 0."""
    v, m = np.asarray(v, dtype=np.float64), np.asarray(m, dtype=np.float64)
    n = v.shape[axis]
    imin, imax = np.expand_dims(v.argmin(axis=axis), axis), np.expand_dims(v.argmax(axis=axis), axis)
    lo, hi = np.take_along_axis(v, imin, axis), np.take_along_axis(v, imax, axis)
    rng = hi - lo
    ok = rng != 0
    safe = np.where(ok, rng, 1.0)
    vn = (v - lo) / safe
    e = 2.0 * (vn - m) / n                                    # d / d(vn)
    g = e / safe
    np.put_along_axis(g, imin, np.take_along_axis(g, imin, axis) - (e * (1.0 - vn)).sum(axis=axis, keepdims=True) / safe, axis)
    np.put_along_axis(g, imax, np.take_along_axis(g, imax, axis) - (e * vn).sum(axis=axis, keepdims=True) / safe, axis)
    return np.where(ok, g, 0.0)


def traffic_activity_error_grad(driving, measured):
    """(Z, T): the derivative of traffic_activity_error(traffic_activity(driving), measured) with respect to driving[z, t] -- the same
    for every zone of an hour, since the activity reads the hours' sums -- with the min-max normalisation's terms at the argmin and the
    argmax hour.  The cotangent g_driving of Sampler.expected_grad for the objective "activity_error"."""
    d = np.asarray(driving, dtype=np.float64)
    g = _minmax_mse_grad(d.sum(axis=0), measured, 0)
    return np.asfortranarray(np.broadcast_to(g[None, :], d.shape))


def parking_density_error_grad(parking, measured):
    """(Z, T): the derivative of parking_density_error(parking, 1, measured) with respect to the density parking[z, t]: per valid zone
    the min-max normalised error's derivative, with its argmin and argmax terms, over the number of valid zones; 0 for a zone that is
    not valid (unmeasured or flat).  The cotangent g_parking of Sampler.expected_grad for the objective "parking_error"."""
    p = np.asarray(parking, dtype=np.float64)
    m = np.asarray(measured, dtype=np.float64)
    valid = (m.sum(axis=1) != 0) & (p.max(axis=1) != p.min(axis=1))
    if not valid.any():
        return np.zeros(p.shape, order="F")
    g = _minmax_mse_grad(p, m, 1) / float(valid.sum())
    return np.asfortranarray(np.where(valid[:, None], g, 0.0))


def a_drive_grad(w_sec):
    """(Z, T): the derivative of the noise-free A_drive = sum(driving * w_sec) / (T * 3600) with respect to driving[z, t], from
    Sampler.expected_trip()'s w_sec.  The cotangent g_driving of Sampler.expected_grad for the objective "A_drive"."""
    w = np.asarray(w_sec, dtype=np.float64)
    return np.asfortranarray(w / (w.shape[1] * 3600.0))


def p_drive_param_grads(grad_p_drive, s, p_min, p_max, e_drive):
    """(d_p_min, d_p_max, d_e_drive): the chain rule through p_drive = p_min + (p_max - p_min) * s^e_drive (createpdrive.jl:22-33), s the
    table build_p_drive(0, 1, 1) returns.  The sums run over the entries with grad_p_drive != 0 only: an entry whose p_drive is not
    strictly inside (0, 1) has gradient 0 (include/cpm_expected_grad.h), whatever s holds there (NaN included).  d(s^e)/de is
    s^e * ln s, and 0 at s = 0."""
    g = np.asarray(grad_p_drive, dtype=np.float64)
    s = np.asarray(s, dtype=np.float64)
    on = g != 0
    g, s = g[on], s[on]
    with np.errstate(all="ignore"):
        se = np.power(s, float(e_drive))
        sel = np.where(s > 0, se * np.log(np.where(s > 0, s, 1.0)), 0.0)
    return (float(np.sum(g * (1.0 - se))), float(np.sum(g * se)), float(np.sum(g * (float(p_max) - float(p_min)) * sel)))


def e_dest_param_grad(grad_dest, driving=None, dw_sec=None):
    """d objective / d e_dest from Sampler.expected_grad_dest's grad_dest under the tangent d p_destin / d e_dest: its sum, the term
    through the densities.  For "A_drive" = sum(driving * w_sec) / (T * 3600) the weights depend on p_destin too: with driving and
    Sampler.expected_trip_tangent()'s dw_sec the direct term sum(driving * dw_sec) / (T * 3600) is added, scaled as a_drive_grad scales
    its cotangent."""
    d = float(np.asarray(grad_dest, dtype=np.float64).sum())
    if dw_sec is not None:
        w = np.asarray(dw_sec, dtype=np.float64)
        d += float((np.asarray(driving, dtype=np.float64) * w).sum() / (w.shape[1] * 3600.0))
    return d


# ------------------------------------------------------------------ host residuals and their forward derivatives (for Sampler.expected_tangent)
def _minmax_residual_jvp(v, dv, m, axis):
    """(r, dr): r = ((v - lo) / (hi - lo) - m) / sqrt(n) along `axis` (n its length), so that sum(r * r) over the axis is the mean
    squared error of the min-max normalised v, and dr[p] its derivative along dv[p] (dv has one leading axis more than v).  lo / hi are
    attained at the FIRST minimum / maximum (include/cpm_expected_fit.h) and move with dv there.  A flat slice (hi == lo) has r = NaN,
    like its error, and dr = 0."""
    v, m, dv = np.asarray(v, dtype=np.float64), np.asarray(m, dtype=np.float64), np.asarray(dv, dtype=np.float64)
    n = v.shape[axis]
    imin, imax = np.expand_dims(v.argmin(axis=axis), axis), np.expand_dims(v.argmax(axis=axis), axis)
    lo, hi = np.take_along_axis(v, imin, axis), np.take_along_axis(v, imax, axis)
    rng = hi - lo
    ok = rng != 0
    safe = np.where(ok, rng, 1.0)
    vn = (v - lo) / safe
    dlo, dhi = np.take_along_axis(dv, imin[None], axis + 1), np.take_along_axis(dv, imax[None], axis + 1)
    dvn = (dv - dlo) / safe - vn * ((dhi - dlo) / safe)
    scale = 1.0 / np.sqrt(float(n))
    return np.where(ok, (vn - m) * scale, np.nan), np.where(ok, dvn * scale, 0.0)


def activity_residual_jvp(driving, d_driving, measured):
    """(r (T,), Jr (P, T)) of the traffic-activity term: sum(r * r) = traffic_activity_error(traffic_activity(driving), measured), and
    Jr[p] the derivative of r along d_driving[p] -- (Z, T) densities, (P, Z, T) tangents (Evaluator.expected_jacobian) -- carried
    through the hours' zone sums and the min-max normalisation."""
    a = np.asarray(driving, dtype=np.float64).sum(axis=0)
    da = np.asarray(d_driving, dtype=np.float64).sum(axis=1)
    return _minmax_residual_jvp(a, da, measured, 0)


def parking_residual_jvp(parking, d_parking, measured):
    """(r (Z, T), Jr (P, Z, T)) of the parking term: sum(r * r) = parking_density_error(parking, 1, measured), Jr[p] the derivative of
    r along d_parking[p].  A zone that is not valid (unmeasured or flat) has r = 0 and Jr = 0; with no valid zone r is NaN."""
    p = np.asarray(parking, dtype=np.float64)
    m = np.asarray(measured, dtype=np.float64)
    valid = (m.sum(axis=1) != 0) & (p.max(axis=1) != p.min(axis=1))
    if not valid.any():
        return np.full(p.shape, np.nan), np.zeros(np.shape(d_parking))
    r, dr = _minmax_residual_jvp(p, d_parking, m, 1)
    scale = 1.0 / np.sqrt(float(valid.sum()))
    return np.where(valid[:, None], r * scale, 0.0), np.where(valid[None, :, None], dr * scale, 0.0)


def a_drive_jvp(w_sec, d_driving, driving=None, dw_sec=None):
    """(P,): the derivative of the noise-free A_drive = sum(driving * w_sec) / (T * 3600) along d_driving[p], <a_drive_grad(w_sec),
    d_driving[p]>.  With driving and Sampler.expected_trip_tangent()'s dw_sec the direct term through the trip weights,
    sum(driving * dw_sec) / (T * 3600), is added to the LAST parameter: e_dest, in Evaluator.expected_jacobian's order."""
    w = np.asarray(w_sec, dtype=np.float64)
    n = w.shape[1] * 3600.0
    out = (np.asarray(d_driving, dtype=np.float64) * (w / n)[None]).sum(axis=(1, 2))
    if dw_sec is not None:
        out[-1] += float((np.asarray(driving, dtype=np.float64) * np.asarray(dw_sec, dtype=np.float64)).sum() / n)
    return out


def parking_density_zone_errors(parking, C, measured):
    """The definition of include/cpm_objectives.h on the host, one IEEE f64 operation per step and in its order: (err (Z,) float64
    with -1.0 for a zone that is not valid, valid (Z,) bool).  A zone is valid when its measured row, added in hour order, is != 0 and
    its counts are not flat; measured None: no zone is.  The hours are accumulated row by row (acc = acc + d*d), not with
    .sum(axis=...): numpy's order of a reduction depends on the array's shape, and the device's zone errors are compared bit for bit."""
    c = np.asarray(parking, dtype=np.int64)
    Z, T = c.shape
    n = float(C)
    cmin, cmax = c.min(axis=1), c.max(axis=1)
    if measured is None:
        return np.full(Z, -1.0), np.zeros(Z, dtype=bool)
    m = np.asarray(measured, dtype=np.float64)
    msum = np.zeros(Z)
    for t in range(T):
        msum = msum + m[:, t]
    valid = (msum != 0) & (cmin != cmax)
    with np.errstate(all="ignore"):
        lo, hi = cmin.astype(np.float64) / n, cmax.astype(np.float64) / n
        rng = hi - lo
        acc = np.zeros(Z)
        for t in range(T):
            p = c[:, t].astype(np.float64) / n
            d = (p - lo) / rng - m[:, t]
            acc = acc + d * d
        err = acc / float(T)
    return np.where(valid, err, -1.0), valid


def objectives_from_record(rec, pt, C, T, measured_activity=None, with_parking_error=True):
    """The result dict of Evaluator._objectives from one device record (include/cpm_objectives.h: int64[4 + 2*T]), without the count
    arrays: the traffic activity from the driving sums through traffic_activity (a (1, T) array has the same column sums, so it is
    bit-equal to the host path), A_drive from word 1, parking_error from the bits in word 3, and the two figures grid_sweep
    otherwise takes from the arrays: driving_total and hours_hold_all_cars (every hour's parking sum == C)."""
    rec = np.ascontiguousarray(rec, dtype=np.int64)
    driving_sum, parking_sum = rec[4:4 + T], rec[4 + T:4 + 2 * T]
    act = traffic_activity(driving_sum.reshape(1, T))
    out = {"e_drive": pt.e_drive, "p_min": pt.p_min, "p_max": pt.p_max, "e_dest": float(pt.e_dest),
           "A_drive": a_drive(int(rec[1]), C, T), "traffic_activity": act,
           "driving_total": int(driving_sum.sum()), "hours_hold_all_cars": bool((parking_sum == C).all())}
    if measured_activity is not None:
        out["activity_error"] = traffic_activity_error(act, measured_activity)
    if with_parking_error:
        out["parking_error"] = float(rec[3:4].view(np.float64)[0])
    return out


# ------------------------------------------------------------------ one evaluation
@dataclass
class Point:
    e_drive: float = 0.5
    p_min: float = 0.1
    p_max: float = 0.9
    e_dest: object = 2


@dataclass
class Evaluator:
    """Holds a Sampler whose datamatrix is uploaded and whose car state is the post-IVP state.

    expected_sparse=True runs the noise-free calls from the compact rows of sparse tables, with the bits of the default Evaluator and
    without ever building the dense p_destin array: evaluate_expected[_batch] (propagation and travel product), and
    expected_gradient[_batch], expected_fit and refine_expected with dest=False.  With dest=True, and in expected_jacobian and
    refine_expected_lm, the adjoint, the trip weights and the fit are the dense calls as before: the tangent of p_destin is a dense
    array.  The bits are the default Evaluator's on one condition (include/cpm_expected_sparse_grad.h): every mean of the datamatrix
    and every distance at a cell p_destin does NOT store is finite.  The dense trip weights form 0 * value there, so a NaN mean at
    a cell of zero count makes the default Evaluator's travel product, A_drive and their gradients NaN where the sparse ones are not.
    expected_noise runs from the compact rows too (include/cpm_expected_sparse_var.h), with travel=True on the further condition that
    var_sec of every cell that is not stored is finite (that header says which mean and std words are not).

    expected_sparse_dest=True (with expected_sparse=True) keeps the tangent of p_destin on the stored cells as well
    (include/cpm_expected_sparse_dest.h): expected_gradient[_batch], expected_fit and refine_expected with dest=True then run from the
    compact rows end to end, with the same bits, and neither the dense p_destin array nor the dense tangent is ever built.
    expected_jacobian and refine_expected_lm with dest=True keep the dense tangent unless expected_sparse_tangent=True.

    expected_sparse_tangent=True (with expected_sparse=True) runs the forward tangent from the compact rows as well
    (include/cpm_expected_sparse_tangent.h): expected_jacobian, and so refine_expected_lm, with the same bits and without the dense
    p_destin array; with dest=True (which needs expected_sparse_dest=True too) without the dense tangent either."""
    sampler: object
    C: int
    seed: int
    measured_activity: object = None
    measured_parking: object = None
    travel: bool = True
    fallbacks: int = 0      # pipelined points whose asynchronous step overflowed a bucket region and were evaluated again, blocking
    device_objectives: bool = False   # reduce the counts on the device (include/cpm_objectives.h): the host reads 4 + 2*T words per point
    # expected_sparse: evaluate_expected[_batch] (propagation and travel product), and expected_gradient[_batch], expected_fit and so
    # refine_expected with dest=False, run from the compact rows of sparse tables (include/cpm_expected_sparse.h,
    # include/cpm_expected_sparse_grad.h): same bits where the means and distances at cells that are not stored are finite (the class
    # docstring), and the dense p_destin array is never built.  With dest=True, and in
    # expected_jacobian / refine_expected_lm, the adjoint, the trip weights and the fit are the dense calls as before: the tangent of
    # p_destin is a dense array.
    expected_sparse: bool = False
    # expected_sparse_dest: behind expected_sparse, the calls above with dest=True read a compact tangent on the stored cells
    # (include/cpm_expected_sparse_dest.h) and stay sparse; expected_jacobian / refine_expected_lm keep the dense tangent.
    expected_sparse_dest: bool = False
    # expected_sparse_tangent: behind expected_sparse, expected_jacobian / refine_expected_lm call the forward tangent of the compact
    # rows (include/cpm_expected_sparse_tangent.h); with dest=True they read the compact tangent, which expected_sparse_dest keeps.
    expected_sparse_tangent: bool = False
    _e_dest: object = field(default=None, repr=False)
    _pipe: object = field(default=None, repr=False)
    _s_table: object = field(default=None, repr=False)   # build_p_drive(0, 1, 1): the datamatrix's own table, for expected_gradient
    _tangent: object = field(default=None, repr=False)   # the e_dest key whose d p_destin / d e_dest is installed (expected_gradient, dest=True)
    _tangent_compact: object = field(default=None, repr=False)   # ... and the key whose compact tangent is (expected_sparse_dest)
    _fit_measured: object = field(default=None, repr=False)   # expected_fit has installed the measured arrays in the context

    def __post_init__(self):
        if self.expected_sparse_dest and not self.expected_sparse:
            raise ValueError("Evaluator: expected_sparse_dest=True needs expected_sparse=True: the compact tangent serves the sparse calls alone")
        if self.expected_sparse_tangent and not self.expected_sparse:
            raise ValueError("Evaluator: expected_sparse_tangent=True needs expected_sparse=True: the sparse forward tangent reads the compact rows")
        if self.measured_parking is not None:   # Julia order, like the count tensors: the error is evaluated hour-major on contiguous rows
            self.measured_parking = np.asfortranarray(np.asarray(self.measured_parking, dtype=np.float64))
        if self.device_objectives:
            self.sampler.set_measured(self.measured_parking)    # once: resident in the context (None: forgets what it held)

    def _install(self, pt):
        self.sampler.build_p_drive(pt.p_min, pt.p_max, pt.e_drive, want=False)   # (Z x T work: the Z x Z x T mean is cached by the library)
        self._install_dest(pt.e_dest)

    def _install_dest(self, e_dest):
        key = e_dest_key(e_dest)
        if key != self._e_dest:              # the CDF and the row packs are rebuilt only when e_dest changes
            self.sampler.build_p_dest(e_dest, want=False)
            self._e_dest = key
            self._tangent = None             # (the library drops the tangent with the tables it belonged to)
            self._tangent_compact = None

    def _install_dest_tangent(self, dense=False):
        """d p_destin / d e_dest of the installed tables: the compact one under expected_sparse_dest, unless the caller reads the dense
        array (dense=True: the forward tangent)."""
        if self.expected_sparse_dest and not dense:
            if self._tangent_compact != self._e_dest:
                self.sampler.build_p_dest_tangent(want=False, sparse=True)
                self._tangent_compact = self._e_dest
        elif self._tangent != self._e_dest:  # rebuilt only when e_dest changes, like the tables
            self.sampler.build_p_dest_tangent(want=False)
            self._tangent = self._e_dest

    def _sparse(self, dest):
        """Whether a call runs from the compact rows: with dest only where the tangent is compact too."""
        return self.expected_sparse and (not dest or self.expected_sparse_dest)

    def _objectives(self, pt, parking, driving, sum_tt_q16):
        act = traffic_activity(driving)
        out = {"e_drive": pt.e_drive, "p_min": pt.p_min, "p_max": pt.p_max, "e_dest": float(pt.e_dest),
               "A_drive": a_drive(sum_tt_q16, self.C, self.sampler.T), "traffic_activity": act,
               "parking": parking, "driving": driving}
        if self.measured_activity is not None:
            out["activity_error"] = traffic_activity_error(act, self.measured_activity)
        if self.measured_parking is not None:
            out["parking_error"] = parking_density_error(parking, self.C, self.measured_parking)
        return out

    def evaluate(self, pt):
        """One point, blocking."""
        self._install(pt)
        r = self.sampler.resample(self.seed, travel=self.travel)
        if self.device_objectives:
            return self._from_record(pt, self._record_of_host_counts(r["parking"], r["driving"], r["sum_tt_q16"]))
        return self._objectives(pt, r["parking"], r["driving"], r["sum_tt_q16"])

    # -- noise-free form: the chain's mean (include/cpm_expected.h) and the expected travel (include/cpm_expected_travel.h); no cars --
    def _expected_from_device(self, pts, ivp, batch):
        """The installed tables' expected tensors and travel totals through the device entries: one propagation per fleet, 2 + 2*T*Z
        words per fleet to the host.  pts: the points whose tables are installed; batch: as the batch tables."""
        import torch
        s = self.sampler
        B, words = len(pts), s.expected_words()
        dev = f"cuda:{s.device}"
        out = torch.empty(B * words, dtype=torch.float64, device=dev)
        tot = torch.empty(2 * B, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(s.device)
        if batch:
            s.expected_batch_dev(out.data_ptr(), 0, ivp, sparse=self.expected_sparse)
        else:
            s.expected_dev(out.data_ptr(), 0, ivp, sparse=self.expected_sparse)
        s.expected_travel_dev(out.data_ptr(), B, 0, tot.data_ptr(), sparse=self.expected_sparse)
        s.sync()
        both = out.cpu().numpy().reshape(B, 2, s.T, s.Z)
        totals = tot.cpu().numpy().reshape(B, 2)
        outs = []
        for b, pt in enumerate(pts):
            parking, driving = both[b, 0].T, both[b, 1].T          # Julia order (Z, T): views
            r = {"e_drive": pt.e_drive, "p_min": pt.p_min, "p_max": pt.p_max, "e_dest": float(pt.e_dest)}
            r.update(expected_objectives(parking, driving, self.measured_activity, self.measured_parking, seconds=float(totals[b, 0])))
            r.update(total_seconds=float(totals[b, 0]), total_km=float(totals[b, 1]), parking=parking, driving=driving)
            outs.append(r)
        return outs

    def evaluate_expected(self, pt, ivp=True):
        """One point without sampling noise: installs its tables and returns the objectives of the chain's mean -- traffic_activity,
        activity_error / parking_error where the measured data is given, and A_drive from the expected travel-time sum.  ivp: the day
        starts from the uniform placement carried through hours 0 .. T-2, the expected form of the post-IVP state evaluate() samples
        from.  `parking` / `driving` are densities (counts / C in the mean).  Needs no cars."""
        self._install(pt)
        return self._expected_from_device([pt], ivp, False)[0]

    def expected_noise(self, pt, ivp=True, travel=False):
        """The seed noise of one point's resample of C cars: installs pt's tables and returns dict(activity: activity_noise()'s mean
        and var of driving_sum[t], and objective_noise()'s first-order activity_error_std / parking_error_std where the measured data
        is given).  The cars start C / Z per zone (init_states' uniform placement; ivp: in front of the IVP), the start of
        evaluate_expected().  travel: also A_drive: travel_noise()'s dict (exact, no linearisation).  Under expected_sparse every call
        here reads the compact rows (include/cpm_expected_sparse_var.h): the same bits, and the dense p_destin array is not built."""
        self._install(pt)
        s = self.sampler
        sparse = self.expected_sparse
        start = np.full(s.Z, self.C / s.Z)
        out = {"activity": activity_noise(s, start, ivp=ivp, sparse=sparse)}
        if self.measured_activity is not None or self.measured_parking is not None:
            out.update(objective_noise(s, s.expected(None, ivp=ivp, sparse=sparse), self.C, start, self.measured_activity, self.measured_parking,
                                       ivp=ivp, sparse=sparse))
        if travel:
            out["A_drive"] = travel_noise(s, start, ivp=ivp, sparse=sparse)
        return out

    def evaluate_expected_batch(self, pts, ivp=True):
        """The same for points that share e_dest, as the fleets of ONE batched propagation (build_p_drive_batch, expected_batch_dev,
        expected_travel_dev): a list of evaluate_expected()'s dicts, point for point and bit for bit."""
        pts = list(pts)
        if len({e_dest_key(pt.e_dest) for pt in pts}) != 1:
            raise ValueError("evaluate_expected_batch: the points of a batch share e_dest")
        self._install_dest(pts[0].e_dest)
        self.sampler.build_p_drive_batch([pt.p_min for pt in pts], [pt.p_max for pt in pts], [pt.e_drive for pt in pts])
        return self._expected_from_device(pts, ivp, True)

    def expected_gradient(self, pt, objective, ivp=True, dest=False):
        """The gradient of one noise-free objective of evaluate_expected(pt, ivp) -- "activity_error", "parking_error" or "A_drive" -- by
        one backward pass (Sampler.expected_grad): dict(objective, value, grad_p_drive (Z, T), grad_pi0 (Z,), d_p_min, d_p_max,
        d_e_drive).  The parameter derivatives are the chain rule through p_drive = p_min + (p_max - p_min) * s^e_drive with
        s = build_p_drive(0, 1, 1), cached here (it depends on the datamatrix alone); pt's own tables are installed when this returns.
        dest: the result also holds grad_dest (Z, T) and d_e_dest, from the same backward pass along d p_destin / d e_dest
        (Sampler.build_p_dest_tangent, rebuilt only when e_dest changes; pt.e_dest > 0).  For "A_drive" d_e_dest includes the direct
        term through the trip weights.  Without it nothing is built and the result is what it is without the argument."""
        if objective not in ("activity_error", "parking_error", "A_drive"):
            raise ValueError(f"expected_gradient: unknown objective {objective!r}")
        s = self.sampler
        if self._s_table is None:
            self._s_table = s.build_p_drive(0.0, 1.0, 1.0)
        r = self.evaluate_expected(pt, ivp)                       # (installs pt's tables: the table above is replaced)
        zero = np.zeros((s.Z, s.T), order="F")
        if objective == "activity_error":
            if self.measured_activity is None:
                raise ValueError("expected_gradient: activity_error needs measured_activity")
            gp, gd = zero, traffic_activity_error_grad(r["driving"], self.measured_activity)
        elif objective == "parking_error":
            if self.measured_parking is None:
                raise ValueError("expected_gradient: parking_error needs measured_parking")
            gp, gd = parking_density_error_grad(r["parking"], self.measured_parking), zero
        else:
            gp, gd = zero, a_drive_grad(s.expected_trip(sparse=self._sparse(dest))[0])
        if dest:
            self._install_dest_tangent()
            g = s.expected_grad_dest(gp, gd, ivp=ivp, sparse=self._sparse(dest))
        else:
            g = s.expected_grad(gp, gd, ivp=ivp, sparse=self.expected_sparse)
        d_min, d_max, d_e = p_drive_param_grads(g["grad_p_drive"], self._s_table, pt.p_min, pt.p_max, pt.e_drive)
        out = dict(objective=objective, value=r[objective], grad_p_drive=g["grad_p_drive"], grad_pi0=g["grad_pi0"],
                   d_p_min=d_min, d_p_max=d_max, d_e_drive=d_e)
        if dest:
            direct = objective == "A_drive"
            out["grad_dest"] = g["grad_dest"]
            out["d_e_dest"] = e_dest_param_grad(g["grad_dest"], r["driving"] if direct else None,
                                                s.expected_trip_tangent(sparse=self._sparse(dest))[0] if direct else None)
        return out

    def expected_gradient_batch(self, pts, objective, ivp=True, dest=False):
        """expected_gradient() for points that share e_dest, as the fleets of ONE batched forward propagation and ONE batched backward
        pass (evaluate_expected_batch, Sampler.expected_grad_batch): a list of expected_gradient()'s dicts, point for point and bit for
        bit.  The batch tables hold the points' p_drive when this returns; the context's own p_drive is the table s of the chain rule
        only if this call had to build it."""
        if objective not in ("activity_error", "parking_error", "A_drive"):
            raise ValueError(f"expected_gradient_batch: unknown objective {objective!r}")
        pts = list(pts)
        if len({e_dest_key(pt.e_dest) for pt in pts}) != 1:
            raise ValueError("expected_gradient_batch: the points of a batch share e_dest")
        if objective == "activity_error" and self.measured_activity is None:
            raise ValueError("expected_gradient_batch: activity_error needs measured_activity")
        if objective == "parking_error" and self.measured_parking is None:
            raise ValueError("expected_gradient_batch: parking_error needs measured_parking")
        s = self.sampler
        if self._s_table is None:
            self._s_table = s.build_p_drive(0.0, 1.0, 1.0)
        rs = self.evaluate_expected_batch(pts, ivp)
        B = len(pts)
        gp = np.zeros((s.Z, s.T, B), order="F")
        gd = np.zeros((s.Z, s.T, B), order="F")
        sparse = self._sparse(dest)
        w_sec = s.expected_trip(sparse=sparse)[0] if objective == "A_drive" else None
        for b, r in enumerate(rs):
            if objective == "activity_error":
                gd[:, :, b] = traffic_activity_error_grad(r["driving"], self.measured_activity)
            elif objective == "parking_error":
                gp[:, :, b] = parking_density_error_grad(r["parking"], self.measured_parking)
            else:
                gd[:, :, b] = a_drive_grad(w_sec)
        if dest:
            self._install_dest_tangent()
        g = s.expected_grad_batch(gp, gd, ivp=ivp, dest=dest, sparse=sparse, compact_tangent=sparse and dest)
        direct = dest and objective == "A_drive"
        dw_sec = s.expected_trip_tangent(sparse=sparse)[0] if direct else None
        outs = []
        for b, (pt, r) in enumerate(zip(pts, rs)):
            grad = np.asfortranarray(g["grad_p_drive"][:, :, b])
            d_min, d_max, d_e = p_drive_param_grads(grad, self._s_table, pt.p_min, pt.p_max, pt.e_drive)
            out = dict(objective=objective, value=r[objective], grad_p_drive=grad, grad_pi0=np.ascontiguousarray(g["grad_pi0"][:, b]),
                       d_p_min=d_min, d_p_max=d_max, d_e_drive=d_e)
            if dest:
                out["grad_dest"] = np.asfortranarray(g["grad_dest"][:, :, b])
                out["d_e_dest"] = e_dest_param_grad(out["grad_dest"], r["driving"] if direct else None, dw_sec)
            outs.append(out)
        return outs

    def expected_fit(self, pts, weights=None, ivp=True, dest=False):
        """Value and gradient of F = sum of weight * objective at points that share e_dest, in ONE device call with one forward
        propagation (Sampler.expected_fit_dev, include/cpm_expected_fit.h): the host reads B * (16 + T) words and reduces nothing.
        weights: a dict over "activity_error", "parking_error", "A_drive" (missing keys: 0), or a list of such dicts, one per point;
        None: 1 for activity_error alone.  A weighed objective needs its measured data.  Returns per point a dict with the scalar
        keys of expected_gradient() -- objective (the one weighed objective's name, else "F"), value (= F), d_p_min, d_p_max, d_e_drive,
    and d_e_dest when dest -- plus F, activity_error,
        parking_error, A_drive, n_valid, total_seconds, total_km and traffic_activity (T,).  The batch tables hold the points'
        p_drive when this returns."""
        pts, w = _fit_inputs("expected_fit", self, pts, weights)
        import torch
        s = self.sampler
        self._install_dest(pts[0].e_dest)
        if dest:
            self._install_dest_tangent()
        if self._fit_measured is None:   # once: resident in the context
            s.set_measured_activity(self.measured_activity)
            s.set_measured(self.measured_parking)
            self._fit_measured = True
        B, words = len(pts), s.fit_words()
        rec = torch.empty(B * words, dtype=torch.float64, device=f"cuda:{s.device}")
        torch.cuda.synchronize(s.device)
        s.expected_fit_dev([pt.p_min for pt in pts], [pt.p_max for pt in pts], [pt.e_drive for pt in pts], w, rec.data_ptr(), 0, ivp, dest,
                           sparse=self._sparse(dest), compact_tangent=self._sparse(dest) and dest)
        s.sync()
        r = s.fit_record(rec.cpu().numpy(), s.T)
        outs = []
        for b, pt in enumerate(pts):
            weighed = [k for k, v in zip(FIT_WEIGHT_KEYS, w[b]) if v != 0]
            out = {"e_drive": pt.e_drive, "p_min": pt.p_min, "p_max": pt.p_max, "e_dest": float(pt.e_dest),
                   "objective": weighed[0] if len(weighed) == 1 else "F", "value": float(r["F"][b])}
            for k in ("F", "activity_error", "parking_error", "A_drive", "d_p_min", "d_p_max", "d_e_drive", "total_seconds", "total_km"):
                out[k] = float(r[k][b])
            out["n_valid"] = int(r["n_valid"][b])
            if dest:
                out["d_e_dest"] = float(r["d_e_dest"][b])
            out["traffic_activity"] = r["traffic_activity"][b]
            outs.append(out)
        return outs

    def expected_jacobian(self, pt, ivp=True, dest=False):
        """The densities of evaluate_expected(pt, ivp) and their derivatives for the model's parameters, in forward mode: pt's tables
        are installed as expected_gradient() installs them, the direction tables d p_drive / d (p_min, p_max, e_drive) are built on the
        device (Sampler.build_p_drive_tangent_dev) and ONE tangent call (Sampler.expected_tangent_dev, include/cpm_expected_tangent.h)
        carries K = 3 directions -- 4 with dest: the last one along d p_destin / d e_dest (pt.e_dest > 0).  Returns dict(parking,
        driving (Z, T), d_parking, d_driving (P, Z, T)) in the parameter order (e_drive, p_min, p_max[, e_dest]).  The forward
        tangent reads the DENSE tangent of p_destin, under expected_sparse_dest alone as well.  Under expected_sparse_tangent=True the
        call is the one of include/cpm_expected_sparse_tangent.h instead: the same bits from the compact rows, and with dest (which
        then needs expected_sparse_dest=True) from the compact tangent, carried into destination columns once per tangent."""
        import torch
        s = self.sampler
        sparse = self.expected_sparse_tangent
        if sparse and dest and not self.expected_sparse_dest:
            raise ValueError("expected_jacobian: dest=True under expected_sparse_tangent=True needs expected_sparse_dest=True (the compact tangent)")
        self._install(pt)
        if dest:
            self._install_dest_tangent(dense=not sparse)
        K, zt = (4 if dest else 3), s.Z * s.T
        dev = f"cuda:{s.device}"
        built = torch.empty(3 * zt, dtype=torch.float64, device=dev)      # (p_min, p_max, e_drive), as the builder lays them out
        dpd = torch.zeros(K * zt, dtype=torch.float64, device=dev)
        out = torch.empty(K * 2 * zt, dtype=torch.float64, device=dev)
        primal = torch.empty(2 * zt, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(s.device)
        s.build_p_drive_tangent_dev(pt.p_min, pt.p_max, pt.e_drive, built.data_ptr())
        s.sync()
        dpd[:zt], dpd[zt:2 * zt], dpd[2 * zt:3 * zt] = built[2 * zt:], built[:zt], built[zt:2 * zt]
        torch.cuda.synchronize(s.device)
        s.expected_tangent_dev(K, out.data_ptr(), dpd.data_ptr(), c_dest=[0.0, 0.0, 0.0, 1.0][:K], ivp=ivp, d_expected_ptr=primal.data_ptr(),
                               sparse=sparse)
        s.sync()
        both = out.cpu().numpy().reshape(K, 2, s.T, s.Z)
        prim = primal.cpu().numpy().reshape(2, s.T, s.Z)
        return dict(parking=prim[0].T, driving=prim[1].T, d_parking=both[:, 0].transpose(0, 2, 1), d_driving=both[:, 1].transpose(0, 2, 1))

    # -- device objectives: the record of include/cpm_objectives.h in the place of the count tensor --
    def _from_record(self, pt, rec):
        return objectives_from_record(rec, pt, self.C, self.sampler.T, self.measured_activity, self.measured_parking is not None)

    def _record_of_host_counts(self, parking, driving, sum_tt_q16):
        """The counts of a blocking resample, uploaded and reduced by objectives_dev like every other point's: one definition of
        parking_error for the whole sweep.  Blocking; tensors of its own (the pipeline's slots may be in flight)."""
        import torch
        s = self.sampler
        zt = s.Z * s.T
        flat = np.zeros(s.counts_words(), dtype=np.int64)
        flat[:zt] = np.asarray(parking).ravel(order="F")          # Julia order (Z, T) read column by column IS [T][Z]
        flat[zt:2 * zt] = np.asarray(driving).ravel(order="F")
        flat[2 * zt] = int(sum_tt_q16)
        stream = self._pipe_stream()
        with torch.cuda.stream(stream):
            dev = torch.from_numpy(flat).to(f"cuda:{s.device}")
            obj = torch.zeros(s.objective_words(), dtype=torch.int64, device=f"cuda:{s.device}")
            s.objectives_dev(dev.data_ptr(), 1, self.C, obj.data_ptr())
            rec = obj.cpu().numpy()
        return rec

    def _obj_slot(self, slot, fleets):
        """Slot `slot`'s records of at least `fleets` fleets, device and pinned host (grown like the count tensors in _slot)."""
        import torch
        p, n = self._pipe, self.sampler.objective_words() * fleets
        if "obj_dev" not in p:
            p["obj_dev"], p["obj_host"] = [None, None], [None, None]
        if p["obj_dev"][slot] is None or p["obj_dev"][slot].numel() < n:
            p["done"][slot].synchronize()
            p["obj_dev"][slot] = torch.zeros(n, dtype=torch.int64, device=f"cuda:{self.sampler.device}")
            p["obj_host"][slot] = torch.zeros(n, dtype=torch.int64).pin_memory()
        return n

    # -- pipelined form: point k+1 runs on the GPU while the host reduces point k (two count tensors, pinned host twins) --
    def _slot(self, slot, n):
        """The pipeline's stream, and slot `slot`'s count tensors of at least n words.  A slot grows alone: when it is begun again its
        last step has been reduced (finish runs behind the begin of the next step), while the other slot's step may still be in flight
        -- its tensors and its event stay as they are."""
        import torch
        s = self.sampler
        self._pipe_stream()
        p = self._pipe
        if p["dev"][slot] is None or p["dev"][slot].numel() < n:
            p["done"][slot].synchronize()  # (a slot's event has recorded nothing yet, or a step that has been reduced)
            p["dev"][slot] = torch.zeros(n, dtype=torch.int64, device=f"cuda:{s.device}")
            p["host"][slot] = torch.zeros(n, dtype=torch.int64).pin_memory()
        return p

    def _pipe_stream(self):
        """The pipeline's stream (the context's own as a torch stream); the pipeline's bookkeeping is created with it."""
        import torch
        s = self.sampler
        if self._pipe is None:
            if s._stream is None:     # (a Sampler that was given its stream at construction keeps it; see Sampler.__init__)
                s.set_stream(torch.cuda.Stream(device=s.device))
            stream = s._stream_obj if hasattr(s._stream_obj, "cuda_stream") else torch.cuda.ExternalStream(s._stream, device=s.device)
            self._pipe = dict(stream=stream, dev=[None, None], host=[None, None], done=[torch.cuda.Event() for _ in range(2)])
        return self._pipe["stream"]

    def begin(self, pt, slot):
        """Enqueue the table update, the resample and the copy of its counts to the host for `pt`; returns at once."""
        import torch
        s = self.sampler
        n = s.counts_words()
        p = self._slot(slot, n)
        w = self._obj_slot(slot, 1) if self.device_objectives else 0
        self._install(pt)
        with torch.cuda.stream(p["stream"]):
            s.resample_dev(self.seed, p["dev"][slot].data_ptr(), travel=self.travel)
            if self.device_objectives:    # behind the resample on the same stream; only the record crosses to the host
                s.objectives_dev(p["dev"][slot].data_ptr(), 1, self.C, p["obj_dev"][slot].data_ptr())
                p["obj_host"][slot][:w].copy_(p["obj_dev"][slot][:w], non_blocking=True)
            else:
                p["host"][slot][:n].copy_(p["dev"][slot][:n], non_blocking=True)
            p["done"][slot].record(p["stream"])

    def finish(self, pt, slot):
        """Wait for `begin(pt, slot)` and reduce its counts.  A step whose status word is set (a bucket region overflowed: the
        asynchronous form cannot repeat itself) is evaluated again through the blocking call, which grows the regions."""
        p = self._pipe
        p["done"][slot].synchronize()
        if self.device_objectives:
            rec = p["obj_host"][slot].numpy()[:self.sampler.objective_words()].copy()   # (the pinned twin is reused two points later)
            if rec[0] != 0:               # (as below: the blocking call, whose counts go through objectives_dev as well)
                self.fallbacks += 1
                out = self.evaluate(pt)
                out["fallback"] = True
                return out
            return self._from_record(pt, rec)
        flat = p["host"][slot].numpy()
        Z, T = self.sampler.Z, self.sampler.T
        zt = Z * T
        if flat[2 * zt + 1] != 0:
            # (evaluate() installs pt's tables again -- the next point's are in place by now -- and the blocking resample grows the
            #  regions; the point already in flight behind this one was enqueued on the old regions and comes back here too)
            self.fallbacks += 1
            out = self.evaluate(pt)
            out["fallback"] = True
            return out
        both = flat[:2 * zt].copy()                           # (the pinned twin is reused two points later)
        parking = both[:zt].reshape((T, Z)).T                 # Julia order (Z, T): views, no second copy
        driving = both[zt:].reshape((T, Z)).T
        return self._objectives(pt, parking, driving, int(flat[2 * zt]))


    # -- batched form: the points of one batch share e_dest and run as the fleets of ONE batched resample (include/cpm_batch.h) --
    def begin_batch(self, pts, slot):
        """Enqueue the batch tables of `pts` (one e_dest), their batched resample and the copy of their counts to the host."""
        import torch
        s = self.sampler
        n = s.counts_words() * len(pts)
        p = self._slot(slot, n)        # (sized per slot: a lane's batches need not grow monotonically, nor be of one size)
        w = self._obj_slot(slot, len(pts)) if self.device_objectives else 0
        self._install_dest(pts[0].e_dest)
        s.build_p_drive_batch([pt.p_min for pt in pts], [pt.p_max for pt in pts], [pt.e_drive for pt in pts])
        with torch.cuda.stream(p["stream"]):
            s.resample_batch_dev(self.seed, p["dev"][slot].data_ptr(), travel=self.travel)
            if self.device_objectives:
                s.objectives_dev(p["dev"][slot].data_ptr(), len(pts), self.C, p["obj_dev"][slot].data_ptr())
                p["obj_host"][slot][:w].copy_(p["obj_dev"][slot][:w], non_blocking=True)
            else:
                p["host"][slot][:n].copy_(p["dev"][slot][:n], non_blocking=True)
            p["done"][slot].record(p["stream"])

    def finish_batch(self, pts, slot):
        """Wait for `begin_batch(pts, slot)` and reduce every fleet's counts; a fleet whose status word is set is evaluated again
        through the blocking call (and counted in `fallbacks`), as in finish()."""
        p = self._pipe
        p["done"][slot].synchronize()
        if self.device_objectives:
            ow = self.sampler.objective_words()
            recs = p["obj_host"][slot].numpy()[:ow * len(pts)].reshape(len(pts), ow).copy()   # (the pinned twin is reused two batches later)
            outs = []
            for b, pt in enumerate(pts):
                if recs[b, 0] != 0:
                    self.fallbacks += 1
                    out = self.evaluate(pt)
                    out["fallback"] = True
                else:
                    out = self._from_record(pt, recs[b])
                outs.append(out)
            return outs
        Z, T = self.sampler.Z, self.sampler.T
        zt, nw = Z * T, self.sampler.counts_words()
        flat = p["host"][slot].numpy()[:nw * len(pts)].reshape(len(pts), nw)
        bad = flat[:, 2 * zt + 1] != 0
        counts = flat[:, :2 * zt].copy()                      # (the pinned twin is reused two batches later)
        outs = []
        for b, pt in enumerate(pts):
            if bad[b]:
                self.fallbacks += 1
                out = self.evaluate(pt)
                out["fallback"] = True
            else:
                parking = counts[b, :zt].reshape((T, Z)).T
                driving = counts[b, zt:].reshape((T, Z)).T
                out = self._objectives(pt, parking, driving, int(flat[b, 2 * zt]))
            outs.append(out)
        return outs


FIT_WEIGHT_KEYS = ("activity_error", "parking_error", "A_drive")


def _fit_inputs(what, evaluator, pts, weights):
    """(points, (B, 3) weights) of Evaluator.expected_fit / refine_expected, checked before the sampler is touched: the points share
    e_dest, every weight key is known and finite, and a weighed objective has its measured data."""
    pts = list(pts)
    if not pts:
        raise ValueError(f"{what}: no points")
    if len({e_dest_key(pt.e_dest) for pt in pts}) != 1:
        raise ValueError(f"{what}: the points of a batch share e_dest")
    if weights is None:
        weights = {"activity_error": 1.0}
    per_point = [weights] * len(pts) if isinstance(weights, dict) else list(weights)
    if len(per_point) != len(pts):
        raise ValueError(f"{what}: {len(per_point)} weight dicts for {len(pts)} points")
    w = np.zeros((len(pts), 3))
    for b, d in enumerate(per_point):
        unknown = set(d) - set(FIT_WEIGHT_KEYS)
        if unknown:
            raise ValueError(f"{what}: unknown weight keys {sorted(unknown)}")
        for k, key in enumerate(FIT_WEIGHT_KEYS):
            w[b, k] = float(d.get(key, 0.0))
    if not np.isfinite(w).all():
        raise ValueError(f"{what}: a weight is not finite")
    if (w[:, 0] != 0).any() and evaluator.measured_activity is None:
        raise ValueError(f"{what}: a weight on activity_error needs measured_activity")
    if (w[:, 1] != 0).any() and evaluator.measured_parking is None:
        raise ValueError(f"{what}: a weight on parking_error needs measured_parking")
    return pts, w


DEFAULT_FIT_BOUNDS = {"e_drive": (1e-3, 16.0), "p_min": (0.0, 1.0), "p_max": (0.0, 1.0)}


def _project(x, lo, hi, gap):
    """(e_drive, p_min, p_max) onto the box, then onto p_min + gap <= p_max (the nearest point of that half-plane, kept in the box)."""
    x = np.minimum(np.maximum(x, lo), hi)
    if x[1] + gap > x[2]:
        mid = 0.5 * (x[1] + x[2])
        x[1], x[2] = mid - 0.5 * gap, mid + 0.5 * gap
        if x[1] < lo[1]:
            x[1], x[2] = lo[1], max(x[2], lo[1] + gap)
        if x[2] > hi[2]:
            x[1], x[2] = min(x[1], hi[2] - gap), hi[2]
    return x


def refine_expected(evaluator, pts, weights=None, steps=10, bounds=None, ivp=True, step0=1.0, shrink=0.5, armijo=1e-4, max_backtracks=12,
                    min_gap=1e-3, dest=False):
    """Projected gradient descent with Armijo backtracking on (e_drive, p_min, p_max) for the noise-free F of Evaluator.expected_fit:
    B starting points that share e_dest, ALL advanced by one expected_fit call per trial step (a point whose trial is refused halves
    its own step and waits for the next call; an accepted point doubles it).  bounds: dict over "e_drive", "p_min", "p_max" of
    (low, high); default e_drive in [1e-3, 16], 0 <= p_min < p_max <= 1 (min_gap apart).  A trial x+ = P(x - a * g) is accepted when
    F(x+) <= F(x) - armijo * <g, x - x+>.  Returns per point dict(path: [(Point, F), ...] of the accepted points, the start first;
    gradient: (d_e_drive, d_p_min, d_p_max) at the last one; result: expected_fit's dict there; calls: expected_fit calls made).
    dest: every expected_fit call also forms dF/de_dest (the points share e_dest, which stays where it is: the batch reads one p_destin
    table), and gradient gains it as a fourth entry -- the four-parameter gradient at every accepted point, for a caller that steps
    e_dest between refinements.  Plain host Python over the device call: nothing here is a kernel."""
    b = dict(DEFAULT_FIT_BOUNDS)
    for k, v in (bounds or {}).items():
        if k not in b:
            raise ValueError(f"refine_expected: unknown bound {k!r}")
        b[k] = (float(v[0]), float(v[1]))
    lo = np.array([b["e_drive"][0], b["p_min"][0], b["p_max"][0]])
    hi = np.array([b["e_drive"][1], b["p_min"][1], b["p_max"][1]])
    if not (lo <= hi).all():
        raise ValueError("refine_expected: bounds that cross")
    if not lo[0] > 0:
        raise ValueError("refine_expected: e_drive must stay above 0")
    if lo[1] + min_gap > hi[2]:
        raise ValueError("refine_expected: bounds that cross: no room for p_min < p_max")
    pts, _ = _fit_inputs("refine_expected", evaluator, pts, weights)
    e_dest = pts[0].e_dest
    B = len(pts)
    vec = lambda r: np.array([r["d_e_drive"], r["d_p_min"], r["d_p_max"]])
    point = lambda x: Point(e_drive=float(x[0]), p_min=float(x[1]), p_max=float(x[2]), e_dest=e_dest)
    x = [_project(np.array([pt.e_drive, pt.p_min, pt.p_max], dtype=np.float64), lo, hi, min_gap) for pt in pts]
    fit = (lambda q: evaluator.expected_fit(q, weights, ivp=ivp, dest=True)) if dest else (lambda q: evaluator.expected_fit(q, weights, ivp=ivp))
    cur = fit([point(v) for v in x])
    calls = 1
    paths = [[(point(x[k]), cur[k]["F"])] for k in range(B)]
    alpha = [float(step0)] * B
    accepted, refused = [0] * B, [0] * B
    for _ in range(int(steps) * (int(max_backtracks) + 1)):
        live = [k for k in range(B) if accepted[k] < steps and alpha[k] > 0 and np.isfinite(cur[k]["F"])]
        if not live:
            break
        trial = list(x)
        for k in live:
            trial[k] = _project(x[k] - alpha[k] * vec(cur[k]), lo, hi, min_gap)
        new = fit([point(v) for v in trial])
        calls += 1
        for k in live:
            moved = x[k] - trial[k]
            if not moved.any():                      # the projection holds the point where it is: nothing left to gain
                alpha[k] = 0.0
                continue
            if np.isfinite(new[k]["F"]) and new[k]["F"] <= cur[k]["F"] - armijo * float(vec(cur[k]) @ moved):
                x[k], cur[k] = trial[k], new[k]
                paths[k].append((point(x[k]), cur[k]["F"]))
                accepted[k] += 1
                refused[k] = 0
                alpha[k] *= 2.0
            else:
                refused[k] += 1
                alpha[k] = alpha[k] * shrink if refused[k] <= max_backtracks else 0.0
    grad = lambda r: tuple(vec(r)) + ((r["d_e_dest"],) if dest else ())
    return [dict(path=paths[k], gradient=grad(cur[k]), result=cur[k], calls=calls) for k in range(B)]


def _lm_terms(evaluator, jac, w, w_sec):
    """(F, result dict, J^T r, J^T J, gradient of F) over (e_drive, p_min, p_max) from one expected_jacobian() dict: the weighed
    least-squares residuals stacked, A_drive through its gradient only"""
    rows, jrows, res = [], [], {}
    F, lin = 0.0, np.zeros(3)
    if w[0] != 0:
        r, Jr = activity_residual_jvp(jac["driving"], jac["d_driving"][:3], evaluator.measured_activity)
        res["activity_error"] = float((r * r).sum())
        F += w[0] * res["activity_error"]
        rows.append(np.sqrt(w[0]) * r.ravel())
        jrows.append(np.sqrt(w[0]) * Jr.reshape(3, -1))
    if w[1] != 0:
        r, Jr = parking_residual_jvp(jac["parking"], jac["d_parking"][:3], evaluator.measured_parking)
        res["parking_error"] = float((r * r).sum())
        F += w[1] * res["parking_error"]
        rows.append(np.sqrt(w[1]) * r.ravel())
        jrows.append(np.sqrt(w[1]) * Jr.reshape(3, -1))
    if w[2] != 0:
        res["A_drive"] = float((np.asarray(jac["driving"]) * w_sec).sum() / (w_sec.shape[1] * 3600.0))
        F += w[2] * res["A_drive"]
        lin = w[2] * a_drive_jvp(w_sec, jac["d_driving"][:3])
    r = np.concatenate(rows) if rows else np.zeros(0)
    J = np.concatenate(jrows, axis=1) if jrows else np.zeros((3, 0))
    Jtr = J @ r
    res["F"] = F
    return F, res, Jtr, J @ J.T, 2.0 * Jtr + lin


def refine_expected_lm(evaluator, pts, weights=None, steps=10, bounds=None, ivp=True, lam0=1e-3, min_gap=1e-3, jacobian=None):
    """Levenberg-Marquardt on (e_drive, p_min, p_max) for the noise-free F of Evaluator.expected_fit, from the densities' Jacobian in
    forward mode: activity_error and parking_error are sums of squared residuals r (activity_residual_jvp, parking_residual_jvp) with
    Jacobian J; a weighed A_drive enters through its gradient only.  Per step
        delta = -(J^T J + lam * diag(J^T J))^-1 (J^T r + w_adrive / 2 * grad A_drive),
    the trial P(x + delta) (the projection of refine_expected) is accepted when F decreases, and lam is then divided by 3; a refused
    trial multiplies lam by 4.  steps: trial steps per point, ONE Jacobian call each (refine_expected takes up to 13 expected_fit calls
    per accepted step).  jacobian: a callable pt -> dict(parking, driving (Z, T), d_parking, d_driving (P >= 3, Z, T)[, w_sec (Z, T)]) in
    the parameter order (e_drive, p_min, p_max); default evaluator.expected_jacobian(pt, ivp=ivp), with Sampler.expected_trip()'s w_sec
    where A_drive is weighed -- any evaluator with measured_activity / measured_parking can drive it, a numpy one included.  Weights
    of the least-squares terms must not be negative.  bounds, min_gap: as in refine_expected.  Returns per point refine_expected's dict
    -- path: [(Point, F), ...] of the accepted points, the start first; gradient: dF/d(e_drive, p_min, p_max) at the last one; result:
    dict(F and the weighed terms) there; calls: Jacobian calls made -- plus lam, the damping it ended with.  The default Jacobian is
    the forward tangent, which reads the dense arrays: Evaluator.expected_sparse_dest changes nothing here (a Jacobian with dest=True
    keeps the dense tangent of p_destin) unless Evaluator.expected_sparse_tangent=True, under which the same path, point for point and
    bit for bit, comes from the compact rows (include/cpm_expected_sparse_tangent.h) and neither dense array is built."""
    b = dict(DEFAULT_FIT_BOUNDS)
    for k, v in (bounds or {}).items():
        if k not in b:
            raise ValueError(f"refine_expected_lm: unknown bound {k!r}")
        b[k] = (float(v[0]), float(v[1]))
    lo = np.array([b["e_drive"][0], b["p_min"][0], b["p_max"][0]])
    hi = np.array([b["e_drive"][1], b["p_min"][1], b["p_max"][1]])
    if not (lo <= hi).all():
        raise ValueError("refine_expected_lm: bounds that cross")
    if not lo[0] > 0:
        raise ValueError("refine_expected_lm: e_drive must stay above 0")
    if lo[1] + min_gap > hi[2]:
        raise ValueError("refine_expected_lm: bounds that cross: no room for p_min < p_max")
    if not (np.isfinite(lam0) and lam0 > 0):
        raise ValueError("refine_expected_lm: lam0 must be positive")
    pts, w = _fit_inputs("refine_expected_lm", evaluator, pts, weights)
    if (w[:, :2] < 0).any():
        raise ValueError("refine_expected_lm: a negative weight on a least-squares term")
    e_dest = pts[0].e_dest
    point = lambda x: Point(e_drive=float(x[0]), p_min=float(x[1]), p_max=float(x[2]), e_dest=e_dest)
    if jacobian is None:
        jacobian = lambda pt: evaluator.expected_jacobian(pt, ivp=ivp)
    outs = []
    for k, pt in enumerate(pts):
        calls = 0

        def terms(x):
            jac = jacobian(point(x))
            w_sec = None
            if w[k, 2] != 0:   # (after the call: the weights belong to the tables it installed)
                sparse = bool(getattr(evaluator, "expected_sparse_tangent", False))   # (the compact rows' weights: the dense array stays unbuilt)
                w_sec = np.asarray(jac["w_sec"] if "w_sec" in jac else evaluator.sampler.expected_trip(sparse=sparse)[0], dtype=np.float64)
            return _lm_terms(evaluator, jac, w[k], w_sec)

        x = _project(np.array([pt.e_drive, pt.p_min, pt.p_max], dtype=np.float64), lo, hi, min_gap)
        cur = terms(x)
        calls += 1
        path, lam = [(point(x), cur[0])], float(lam0)
        for _ in range(int(steps)):
            F, _, Jtr, JtJ, grad = cur
            if not np.isfinite(F):
                break
            diag = np.where(np.diag(JtJ) > 0, np.diag(JtJ), 1.0)     # (a parameter no residual moves with: damped on its own scale)
            try:
                delta = -np.linalg.solve(JtJ + lam * np.diag(diag), 0.5 * grad)
            except np.linalg.LinAlgError:
                break
            trial = _project(x + delta, lo, hi, min_gap)
            if not (x - trial).any():                # the projection holds the point where it is: nothing left to gain
                break
            new = terms(trial)
            calls += 1
            if np.isfinite(new[0]) and new[0] < F:
                x, cur, lam = trial, new, lam / 3.0
                path.append((point(x), cur[0]))
            else:
                lam *= 4.0
        outs.append(dict(path=path, gradient=tuple(cur[4]), result=cur[1], calls=calls, lam=lam))
    return outs


def e_dest_key(e_dest):
    """What tells two e_dest values apart for the tables: Julia's Float64^Int and Float64^Float64 differ (main.jl:38)."""
    return (type(e_dest).__name__, float(e_dest))


def batch_cuts(grid, order, batch):
    """`order` (indices into `grid`, already ordered by e_dest) cut into runs of at most `batch` CONSECUTIVE points that share one
    e_dest: the fleets of one batched resample each."""
    cuts, key = [], None
    for i in order:
        k = e_dest_key(grid[i].e_dest)
        if not cuts or k != key or len(cuts[-1]) >= batch:
            cuts.append([])
        cuts[-1].append(i)
        key = k
    return cuts


# ------------------------------------------------------------------ the reference's three searches
def search_exponent(evaluate_error, initial_values, step_size=10.0, max_iter=3, epsilon=0.001, good=0.02):
    """README.md:1100-1314 (e_drive) and 2040-2276 (e_dest): pick the best of a few initial values,
    take one step, then secant-like updates e <- e - step * d(error)/d(e), resetting to the best
    value whenever the error got worse.  Returns (best_value, best_error, history)."""
    hist = [(v, evaluate_error(v)) for v in initial_values]
    best, best_err = min(hist, key=lambda x: x[1])
    e = best + step_size * best_err                                        # Step 3.1
    for _ in range(max_iter):
        err = evaluate_error(e)
        hist.append((e, err))
        error_gradient = err - best_err
        param_gradient = e - best
        if error_gradient < 0:
            best_err, best = err, e
        else:
            e = best
        if param_gradient == 0:
            break
        e = e - step_size * error_gradient / param_gradient                # Step 3.2.6
        if best_err < good or abs(error_gradient) < epsilon:
            break
    return best, best_err, hist


def tune_p_min_max(evaluate_a_drive, A_set=0.07, p_min=0.1, p_max=0.9, max_iter=5):
    """README.md:1436-1676: move p_max (or p_min at the bounds) until A_drive matches A_set to the
    percent; clamp with correctparameters; reset when |dA| grows."""
    pm, px = [p_min], [p_max]
    A = [evaluate_a_drive(p_min, p_max)]
    dA = [A_set - A[0]]
    for n in range(2, max_iter + 1):
        a, b, d, ad = pm[-1], px[-1], dA[-1], A[-1]
        step = (b + a) * d / (n * ad)
        if b == 1:
            if a == b:
                break
            na, nb = a + step, b
        elif a == 0:
            if a == b:
                break
            na, nb = a, b + step
        elif a == b:
            na, nb = a + step, b
        else:
            na, nb = a, b + step
        na, nb = correctparameters(na, nb, a, b)
        an = evaluate_a_drive(na, nb)
        dn = A_set - an
        if int(A_set * 100) == int(an * 100):
            pm.append(na); px.append(nb); A.append(an); dA.append(dn)
            break
        if n > 2 and abs(dn) > abs(d):                                      # worse: reset
            na, nb, an, dn = a, b, ad, A_set - ad
        pm.append(na); px.append(nb); A.append(an); dA.append(dn)
    return pm[-1], px[-1], A[-1], list(zip(pm, px, A))


# ------------------------------------------------------------------ the grid of config 5
def make_grid(e_drive=(0.25, 0.5, 1.0, 2.0), p_min=(0.0, 0.05, 0.1, 0.2), p_max=(0.5, 0.7, 0.9, 1.0),
              e_dest=(0.5, 1, 2, 4)):
    """4 x 4 x 4 x 4 = 256 points by default."""
    return [Point(a, b, c, d) for d in e_dest for a in e_drive for b in p_min for c in p_max]


def points_of_rank(n_points, rank, world_size, order=None):
    """Block deal: rank r takes the r-th of world_size contiguous slices of `order` (default 0 .. n_points-1).  Independent
    points, no data-path collective.  With the points ordered by e_dest a rank's slice spans as few e_dest values as
    possible, so it rebuilds the CDF and the row packs (Z x Z x T work) as rarely as possible."""
    order = list(range(n_points)) if order is None else list(order)
    base, rem = divmod(len(order), int(world_size))
    begin = rank * base + min(rank, rem)
    return order[begin:begin + base + (1 if rank < rem else 0)]


def grid_sweep(evaluator, grid, rank=0, world_size=1, gather=True, checksums=False, batch=None):
    """Evaluate this rank's share of `grid`; returns a list (on every rank when gather) of dicts with the
    per-point scalars, ordered like `grid` (checksums: also CRC-32 of both count tensors, for the tests).

    `evaluator` may be a list of Evaluators on the same GPU (each with its own Sampler context, hence its own stream): the
    rank's slice is cut into as many contiguous pieces and the pieces advance in turn, so that a point of every context is on
    the GPU at any time.  A resample is a serial chain of an issue-bound sampler launch and a latency-bound placing launch
    per hour; two independent chains interleave on the chip (measured at S4k: 1.41 ms for two resamples side by side
    against 2 x 0.92 one after the other, profiles/round2_notes.md) -- the hours of ONE resample cannot.

    batch=B: each lane's slice is cut into batches of at most B consecutive points that share e_dest (batch_cuts); a batch is ONE
    batched resample of B fleets (Evaluator.begin_batch / finish_batch, pipelined like begin / finish).  Same results, point for point.

    An Evaluator with device_objectives=True returns dicts without count arrays: driving_total and hours_hold_all_cars then come from
    its records, and checksums=True (which needs the tensors) raises ValueError."""
    lanes = list(evaluator) if isinstance(evaluator, (list, tuple)) else [evaluator]
    C = lanes[0].C
    if checksums and any(getattr(ev, "device_objectives", False) for ev in lanes):
        raise ValueError("checksums=True needs the count tensors on the host: not together with Evaluator(device_objectives=True)")
    by_e_dest = sorted(range(len(grid)), key=lambda i: (float(grid[i].e_dest), type(grid[i].e_dest).__name__, i))
    mine = points_of_rank(len(grid), rank, world_size, by_e_dest)
    local = {}

    def lane_results(ev, pts):  # point k+1 is enqueued before point k is reduced on the host
        prev = None
        for k, i in enumerate(pts):
            ev.begin(grid[i], k & 1)
            yield (prev[0], ev.finish(grid[prev[0]], prev[1])) if prev is not None else None   # (None: the lane's first point is on its way)
            prev = (i, k & 1)
        if prev is not None:
            yield prev[0], ev.finish(grid[prev[0]], prev[1])

    def results():  # the lanes in turn: each next() enqueues that lane's next point and reduces its previous one
        gens = [lane_results(ev, points_of_rank(len(mine), l, len(lanes), mine)) for l, ev in enumerate(lanes)]
        while gens:
            for g in list(gens):
                try:
                    r = next(g)
                    if r is not None:
                        yield r
                except StopIteration:
                    gens.remove(g)

    def lane_batches(ev, pts):  # batch k+1 is enqueued before batch k is reduced; every step yields the list of results it reduced
        prev = None
        for k, cut in enumerate(batch_cuts(grid, pts, int(batch))):
            ev.begin_batch([grid[i] for i in cut], k & 1)
            yield list(zip(prev[0], ev.finish_batch([grid[i] for i in prev[0]], prev[1]))) if prev is not None else []
            prev = (cut, k & 1)
        if prev is not None:
            yield list(zip(prev[0], ev.finish_batch([grid[i] for i in prev[0]], prev[1])))

    def results_batched():
        gens = [lane_batches(ev, points_of_rank(len(mine), l, len(lanes), mine)) for l, ev in enumerate(lanes)]
        while gens:
            for g in list(gens):
                try:
                    yield from next(g)
                except StopIteration:
                    gens.remove(g)

    for i, r in (results() if batch is None else results_batched()):
        local[i] = {k: v for k, v in r.items() if np.isscalar(v)}
        local[i]["fallback"] = bool(r.get("fallback", False))   # evaluated twice: its asynchronous step had overflowed
        if "driving" in r:
            local[i]["driving_total"] = int(r["driving"].sum())
            local[i]["hours_hold_all_cars"] = bool((r["parking"].sum(axis=0) == C).all())
        else:  # (device objectives: the record's sums, no arrays)
            local[i]["driving_total"] = int(r["driving_total"])
            local[i]["hours_hold_all_cars"] = bool(r["hours_hold_all_cars"])
        if checksums:
            local[i]["parking_crc32"] = zlib.crc32(np.ascontiguousarray(r["parking"].ravel(order="F")).tobytes())
            local[i]["driving_crc32"] = zlib.crc32(np.ascontiguousarray(r["driving"].ravel(order="F")).tobytes())
    if world_size > 1 and gather:
        import torch.distributed as dist
        parts = [None] * world_size
        dist.all_gather_object(parts, local)
        local = {}
        for p in parts:
            local.update(p)
    return [local.get(i) for i in range(len(grid))]
