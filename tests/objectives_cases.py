"""Shared inputs of tests/test_objectives.py (host) and tests/test_objectives_gpu.py (device): the ladder of made-up count tensors,
the bound on the scalar, and a plain scalar-loop statement of the definition in include/cpm_objectives.h."""
import numpy as np

LADDER_Z = (1, 2, 63, 64, 65, 255, 256, 257, 513)      # the wave (64) and workgroup (256) edges of k_obj_zones
LADDER_T = (1, 2, 24)                                  # T = 1: every zone is flat


def bound(Z, T):
    """Relative difference allowed between two orders of the sums behind parking_error: every e_z is a sum of T non-negative terms and
    the scalar a sum of at most Z of them, each rounded operation within 2^-53 relative, plus the divisions -- (T + Z + 2) * 2^-53 on
    either side."""
    return 2 * (T + Z + 2) * 2.0 ** -53


def make_case(Z, T, seed=0):
    """Counts random in [0, 3000), about 10 % of the zones flat, about 30 % of the measured rows all zero, n_cars = 1000 * Z."""
    rng = np.random.default_rng(1000 * Z + T + seed)
    parking = rng.integers(0, 3000, size=(Z, T)).astype(np.int64)
    driving = rng.integers(0, 3000, size=(Z, T)).astype(np.int64)
    flat = rng.random(Z) < 0.1
    parking[flat] = parking[flat, :1]
    measured = rng.uniform(0, 1, (Z, T))
    measured[rng.random(Z) < 0.3] = 0.0
    return dict(Z=Z, T=T, parking=parking, driving=driving, measured=measured, n_cars=1000 * Z,
                sum_tt_q16=int(rng.integers(1, 2 ** 40)))


def tensor(parking, driving, sum_tt_q16=0, status=0):
    """The count tensor of cpm_resample_dev from (Z, T) arrays: parking[T][Z] | driving[T][Z] | sum_tt_q16 | status."""
    Z, T = parking.shape
    flat = np.zeros(2 * Z * T + 2, dtype=np.int64)
    flat[:Z * T] = np.asarray(parking).T.ravel()
    flat[Z * T:2 * Z * T] = np.asarray(driving).T.ravel()
    flat[2 * Z * T], flat[2 * Z * T + 1] = sum_tt_q16, status
    return flat


def loop_zone_errors(parking, C, measured):
    """The definition with Python floats, one zone and one hour at a time."""
    Z, T = parking.shape
    err, valid = [-1.0] * Z, [False] * Z
    n = float(C)
    for z in range(Z):
        s = 0.0
        for t in range(T):
            s = s + float(measured[z, t])
        c = [int(v) for v in parking[z]]
        cmin, cmax = min(c), max(c)
        if s == 0 or cmin == cmax:
            continue
        lo, hi = float(cmin) / n, float(cmax) / n
        acc = 0.0
        for t in range(T):
            p = float(c[t]) / n
            d = (p - lo) / (hi - lo) - float(measured[z, t])
            acc = acc + d * d
        err[z], valid[z] = acc / float(T), True
    return np.array(err, dtype=np.float64), np.array(valid, dtype=bool)


def scalar_of(err, valid):
    """parking_error from the zones' errors as the host restatement orders the sum (numpy's); NaN without a valid zone."""
    return float(err[valid].sum() / valid.sum()) if valid.any() else float("nan")
