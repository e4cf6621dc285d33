"""Hand-made datamatrices for the compact-row dataset route (csrc/cpm_dataset.h) and an exact reference for createpdestin's rows
(not a conftest: imported by tests/test_dataset_route.py; plain numpy, no GPU).

`edge_datamatrix` starts from O.synth_datamatrix(Z, T, TABLE_SEED, density=0.06), clears origins 0 .. 15 (0-based) and plants what that
generator never produces -- rows at the lengths where the kernels change behaviour, pairs with data in all 24 hours (kept cells of
weight 0, a row whose cells total 0), cells with a mean and no standard deviation, a standard deviation without a mean:

  o = 0         nothing: empty rows all day, p_drive = 0
  o = 1         row (1, 3) holds ONE cell, destination Z - 1
  o = 2 .. 7    rows (o, 5) and (o, 17) hold 63, 64, 65, 127, 128 and 129 cells, destinations 0, 31, 32, 63, 64 and Z - 1 among them;
                every pair is populated in exactly these two hours, so its weights are (m / max)^e in (0, 1]
  o = 8         40 pairs populated in all 24 hours, (8, 9) among them (it feeds zone 9 the cars row (9, 9) is drawn from); the pairs
                to the smallest and to the largest destination have their minimum at hour 7: row (8, 7) begins and ends with a kept
                cell of weight 0
  o = 9         12 pairs populated all day, every one with its minimum at hour 9: row (9, 9) holds 12 cells and totals 0
  o = 10        row (10, 6): 30 cells with standard deviation 0 (sigma = a tenth of the mean, src/resampling.jl:65-67); the same on
                5 % of the background cells
  o = 11        row (11, 5): 10 ordinary cells and the cell (11, 13, 5) with a standard deviation and no mean
  o = 14        22 pairs populated all day; those to zones 0 and Z - 1 hold their minimum from hour 0 to hour 11, so twelve rows begin and
                end with a kept cell of weight 0.  Where such a row totals less than 1, a draw above the total must come out at the last
                destination that HOLDS weight (D1), which is not the row's last cell: its high word equals the last cell's, so the
                walk over the row's cells decides
  o = 12, 13, 15  nothing (wide_variant plants on 12)

Origins 1 .. 7, 10 and 11 get five ordinary cells in each of their other hours, to destinations none of their planted pairs uses:
without them the hours without data make mean_sum NaN, createpdrive's extrema NaN and p_drive 0 all day (Appendix A-3), and no driver
would ever be drawn from the planted rows.  The planted rows keep their lengths: the fillers live in other hours.

Z = 358 is no multiple of 4, 32 or 64; the dense pack is 484 words, and the 256-word floor of pack_row_words decides the 60 % rule: a
longest row of 129 cells qualifies (10 x 276 <= 6 x 484), one of 160 (324 words) or 200 (420 words) does not.

`cap_datamatrix` (Z = 1,158, density 0.02) plants one row of 511 cells and one of `longest` cells, 512 = kDsCap or 513, each on a
cleared origin: Z = 1,158 is just above 1,154, the smallest Z at which a 512-cell sparse pack (884 words) passes the 60 % rule against
the dense one (1,476 words), and no multiple of 4 or 64.

`pdest_row_exact` computes a row of createpdestin in rational arithmetic, `pdest_row_bound` the relative error a correctly rounded
left-to-right evaluation may have against it."""
import fractions

import numpy as np

from conftest import TABLE_SEED

EDGE_SEED = 0xD5ED6E
CAP_SEED = 0xD5CA9
ROW_HOUR, ROW_HOUR_2 = 5, 17
ROW_LENGTHS = {2: 63, 3: 64, 4: 65, 5: 127, 6: 128, 7: 129}
MUST = (0, 31, 32, 63, 64)                     # ... and Z - 1
WIDE_ORIGIN, WIDE_HOUR, WIDE_CELLS = 12, 11, 200
NAN_ORIGIN = 14
CAP_FEEDERS = 300
CAP_ROWS = ((3, 4), (-2, 20))                  # (origin, hour) of the 511-cell row and of the `longest` row (origin counted from Z)


# ------------------------------------------------------------------------------------------------ shared probes of a CDF row
def _ref_categorical(cdf_row, k53):
    """first j with u <= cdf[j] after the D1 clamp (oracle semantics), 1-based; 0 for an all-zero row"""
    last = cdf_row[-1]
    if last == 0.0:
        return np.zeros(len(k53), dtype=np.int64)
    u = k53.astype(np.float64) * 2.0 ** -53  # exact: k < 2^53
    ue = np.where(u == 0.0, np.float64(5e-324), u)
    ue = np.minimum(ue, last)
    return np.searchsorted(cdf_row, ue, side="left").astype(np.int64) + 1


def _probe_k53(cdf, rng):
    """one below and one above every breakpoint, +- 2^21 around it, k = 0, 1, 2^53 - 1 and 3,000 random k"""
    t53 = np.floor(np.minimum(cdf, 1.0 - 2.0 ** -53) * 2.0 ** 53).astype(np.int64)
    return np.concatenate([np.array([0, 1, 2 ** 53 - 1, 2 ** 21, 2 ** 21 - 1])] +
                          [np.clip(t53 + d, 0, 2 ** 53 - 1) for d in (-2 ** 21, -1, 0, 1, 2 ** 21)] +
                          [rng.integers(0, 2 ** 53, size=3000)]).astype(np.uint64)


# ------------------------------------------------------------------------------------------------ planting
def _dests(rng, Z, n, exclude, must=()):
    """n distinct destinations, ascending: `must` and a draw from what is left of 0 .. Z - 1 without `exclude`"""
    must = np.asarray(must, dtype=np.int64)
    pool = np.setdiff1d(np.arange(Z), np.concatenate([np.asarray(exclude, dtype=np.int64), must]))
    pick = rng.choice(pool, size=n - len(must), replace=False)
    return np.sort(np.concatenate([must, pick])).astype(np.int64)


def _plant(dm, rng, o, t, dests, sd0=False):
    """means in [300, 2400) s and standard deviations of 10 .. 40 % of them (the ranges of O.synth_datamatrix)"""
    m = 300.0 + 2100.0 * rng.random(len(dests))
    sd = m * (0.1 + 0.3 * rng.random(len(dests)))
    dm[o, dests, t, 0] = m
    dm[o, dests, t, 1] = 0.0 if sd0 else sd


def _fill(dm, rng, o, hours, exclude, per_hour=5):
    Z = dm.shape[0]
    for t in hours:
        _plant(dm, rng, o, t, _dests(rng, Z, per_hour, exclude))


def edge_datamatrix(O, Z=358, T=24):
    """(datamatrix (Z, Z, T, 2), dist (Z, Z)), F-ordered: see the module's docstring"""
    assert Z >= 200 and T == 24
    dm, dist = O.synth_datamatrix(Z, T, TABLE_SEED, density=0.06)
    rng = np.random.default_rng(EDGE_SEED)
    sd0 = (dm[..., 0] != 0) & (rng.random((Z, Z, T)) < 0.05)    # 5 % of the background cells: a mean and no standard deviation
    dm[..., 1][sd0] = 0.0
    dm[0:16] = 0.0
    hours = set(range(T))
    # o = 1: one cell
    _plant(dm, rng, 1, 3, np.array([Z - 1]))
    _fill(dm, rng, 1, sorted(hours - {3}), [1, Z - 1])
    # o = 2 .. 7: the lengths around 64 and 128
    for o, n in ROW_LENGTHS.items():
        d = _dests(rng, Z, n, [o], MUST + (Z - 1,))
        _plant(dm, rng, o, ROW_HOUR, d)
        _plant(dm, rng, o, ROW_HOUR_2, d)
        _fill(dm, rng, o, sorted(hours - {ROW_HOUR, ROW_HOUR_2}), np.concatenate([[o], d]))
    # o = 8: pairs with data all day; the first and the last destination at their minimum in hour 7
    d = _dests(rng, Z, 40, [8], (9,))                           # (zone 9 among them: cars for the row below)
    for t in range(T):
        _plant(dm, rng, 8, t, d)
    dm[8, [d[0], d[-1]], 7, 0] = [250.0, 275.0]                 # (below every other mean of the pair)
    # o = 9: every pair at its minimum in hour 9
    d = _dests(rng, Z, 12, [9])
    for t in range(T):
        _plant(dm, rng, 9, t, d)
    dm[9, d, 9, 0] = 200.0 + 50.0 * rng.random(len(d))
    # o = 10: no standard deviation
    d = _dests(rng, Z, 30, [10])
    _plant(dm, rng, 10, 6, d, sd0=True)
    _fill(dm, rng, 10, sorted(hours - {6}), np.concatenate([[10], d]))
    # o = 11: a standard deviation without a mean (the plant of tests/test_gpu_parity.py::test_sparse_dataset_tables_equal_the_dense_ones)
    d = _dests(rng, Z, 10, [11, 13])
    _plant(dm, rng, 11, 5, d)
    _fill(dm, rng, 11, sorted(hours - {5}), np.concatenate([[11, 13], d]))
    dm[11, 13, 5, 0], dm[11, 13, 5, 1] = 0.0, 5.0
    # o = 14: rows that begin and end with a kept cell of weight 0 in twelve hours
    d = _dests(rng, Z, 22, [14], (0, Z - 1))
    for t in range(T):
        _plant(dm, rng, 14, t, d)
    dm[14, [0, Z - 1], 0:12, 0] = np.array([[250.0], [260.0]])  # (below every other mean of the two pairs)
    return np.asfortranarray(dm), dist


def wide_variant(dm):
    """the same matrix with 200 cells in row (12, 11) (and its twin seven hours later): the sparse pack of the longest row is more than
    60 % of the dense one.  Origin 12 gets the fillers of the other planted origins, so that it drives: the day on this matrix must
    differ from the day on the edge matrix, or a travel table left over from the other datamatrix would go unnoticed"""
    dm = dm.copy(order="F")
    Z, T = dm.shape[0], dm.shape[2]
    rng = np.random.default_rng(EDGE_SEED + 1)
    d = _dests(rng, Z, WIDE_CELLS, [WIDE_ORIGIN], (0, Z - 1))
    twin = (WIDE_HOUR + 7) % T
    _plant(dm, rng, WIDE_ORIGIN, WIDE_HOUR, d)
    _plant(dm, rng, WIDE_ORIGIN, twin, d)
    _fill(dm, rng, WIDE_ORIGIN, sorted(set(range(T)) - {WIDE_HOUR, twin}), np.concatenate([[WIDE_ORIGIN], d]))
    return dm


def nan_pair(dm):
    """(origin, destination) of nan_variant's constant pair: origin 14 and the first zone (not 0, not itself) it holds no data for.  An
    origin that drives, and a destination in the middle of its rows: the cell moves every later cell of origin 14's compact rows, so
    tables left over from this variant would show in the edge matrix's p_drive and travel times"""
    free = np.flatnonzero(dm[NAN_ORIGIN, :, :, 0].max(axis=1) == 0)
    return NAN_ORIGIN, int(free[(free > 0) & (free != NAN_ORIGIN)][0])


def nan_variant(dm):
    """the same matrix with one pair constant and non-zero over the day: (m - min) / (max - min) = 0 / 0 (Appendix A-5)"""
    o, j = nan_pair(dm)
    dm = dm.copy(order="F")
    dm[o, j, :, 0] = 700.0
    dm[o, j, :, 1] = 70.0
    return dm


def cap_rows(Z):
    """[(origin, hour)] of the 511-cell row and of the `longest` row of cap_datamatrix, 0-based"""
    return [(o % Z, t) for (o, t) in CAP_ROWS]


def cap_datamatrix(O, Z=1158, T=24, longest=512):
    """(datamatrix, dist): density 0.02, a row of 511 cells and one of `longest` cells (and their twins twelve hours later, so that the
    weights vary), each on an origin cleared beforehand: the planted pairs hold nothing but the two planted hours.  CAP_FEEDERS other
    origins get a cell towards each of the two origins in the three hours before its long row: at 8 cars per zone the row would see a
    driver or two, with the cars they send it sees a few dozen, and the travel rows written for it are sampled"""
    assert Z > 600 and T == 24
    dm, dist = O.synth_datamatrix(Z, T, TABLE_SEED, density=0.02)
    rng = np.random.default_rng(CAP_SEED)
    for (o, t), n in zip(cap_rows(Z), (511, longest)):
        dm[o] = 0.0
        d = _dests(rng, Z, n, [o], (0, Z - 1))
        _plant(dm, rng, o, t, d)
        _plant(dm, rng, o, (t + 12) % T, d)
        _fill(dm, rng, o, sorted(set(range(T)) - {t, (t + 12) % T}), np.concatenate([[o], d]))
    ours = [o for (o, _) in cap_rows(Z)]
    for (o, t) in cap_rows(Z):
        f = rng.choice(np.setdiff1d(np.arange(Z), ours), size=CAP_FEEDERS, replace=False)
        for h in (t - 3, t - 2, t - 1):
            m = 300.0 + 2100.0 * rng.random(len(f))
            dm[f, o, h, 0] = m
            dm[f, o, h, 1] = m * (0.1 + 0.3 * rng.random(len(f)))
    return np.asfortranarray(dm), dist


# ------------------------------------------------------------------------------------------------ what a fixture holds
def kept_cells(dm):
    """(Z, Z, T) bool: the cells the dataset route keeps in the compact row of (hour, origin) -- a mean, or a weight: x = (m - min) /
    (max - min) != 0 where max > 0 (NaN, of a pair constant over the day, is != 0) -- restated from src/createpdestin.jl:10-28"""
    m = dm[..., 0]
    mx, mn = m.max(axis=2), m.min(axis=2)
    return (m != 0) | ((mx > 0)[:, :, None] & (m != mn[:, :, None]))


def row_lengths(dm):
    """(Z, T) cells per compact row"""
    return kept_cells(dm).sum(axis=1)


# ------------------------------------------------------------------------------------------------ the exact reference
U = fractions.Fraction(1, 2 ** 53)             # unit roundoff of binary64


def pdest_row_exact(dm, i, t, e_dest=2):
    """Row (i, t) (0-based) of createpdestin (src/createpdestin.jl:10-46) in rational arithmetic: the extrema of every pair over the
    day, x = (mean - min) / (max - min) where max > 0, x^e_dest, the row sum and the division where the sum is positive.  Exact: no
    rounding and no summation order.  Returns a list of Z Fractions; None where a pair with max > 0 is constant over the day (the
    reference's 0 / 0)."""
    assert isinstance(e_dest, (int, np.integer)) and e_dest >= 1
    Z = dm.shape[0]
    w = [fractions.Fraction(0)] * Z
    day = np.ascontiguousarray(dm[i, :, :, 0])
    assert not np.isnan(day).any()
    for j in np.flatnonzero(day.max(axis=1) > 0):
        # (the extrema of 24 floats are two of them: comparisons do not round)
        mx, mn, m = (fractions.Fraction(float(v)) for v in (day[j].max(), day[j].min(), day[j, t]))
        if mx == mn:
            return None
        w[j] = ((m - mn) / (mx - mn)) ** int(e_dest)
    nf = sum(w)
    return [v / nf for v in w] if nf > 0 else w


def pdest_row_bound(n, e_dest=2):
    """Relative error of a correctly rounded evaluation of a row with n non-zero weights against pdest_row_exact, by the standard model
    fl(a op b) = (a op b)(1 + d), |d| <= u = 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, 2.2 and 3.1):

      x  = fl(fl(mean - min) / fl(max - min))         three roundings                         x (1 + d)^3
      w  = x^e by e - 1 multiplications               e * 3 + (e - 1) roundings               w (1 + d)^(4e - 1)
      nf = w_1 + .. + w_n, any order, terms >= 0      each term passes at most n - 1 additions  nf (1 + d)^(4e - 1 + n - 1)
           (adding the zeros in between is exact, so n counts the non-zero weights only)
      p  = fl(w / nf)                                 one more                                 p (1 + d)^(8e + n - 2)

    K = 8e + n - 2 factors in all, 4e of them above the fraction bar and 4e + n - 2 below it: (n + 14) u to first order for e = 2.
    With 1 + u <= 1 / (1 - u) the product of the factors lies in [(1 - u)^K, (1 - u)^-K], which is within 1 +- gamma_K,
    gamma_K = K u / (1 - K u): the bound returned.  All terms are non-negative, so no cancellation enters, and the weights of these
    fixtures (x >= 2^-52 * 300 / 2400 where it is not 0) are far above the underflow threshold.  The bound holds for the sequential
    sum of the oracle and the device and equally for a pairwise one."""
    K = 8 * int(e_dest) + n - 2
    return K * U / (1 - K * U)


def check_row_exact(got, exact, where=None):
    """`got` (Z floats) against pdest_row_exact's row: zero entries exactly zero, the others within pdest_row_bound.  Returns the largest
    relative error in units of the bound."""
    n = sum(1 for v in exact if v != 0)
    bound = pdest_row_bound(n)
    worst = fractions.Fraction(0)
    for j, (g, e) in enumerate(zip(got, exact)):
        if e == 0:
            assert g == 0.0, (where, j, g)
        else:
            assert np.isfinite(g), (where, j, g)
            err = abs(fractions.Fraction(float(g)) - e) / e
            assert err <= bound, (where, j, float(err), float(bound))
            worst = max(worst, err / bound)
    return float(worst)
