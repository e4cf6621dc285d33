"""One backward product of the expected densities, and one hour of the trip weights, restated twice, one IEEE f64 operation per step
(include/cpm_expected_sparse_grad.h):

  dense_u / dense_trip    -- in the order of k_exp_grad_u / k_exp_trip (csrc/cpm_expected_grad.h, csrc/cpm_expected_travel.h): EVERY
                             destination of origin o's row, zeros included, goes to chain (d - begin) & 3 of its segment; a chain starts
                             at +0 and adds acc = acc + p * value in ascending d; ((w0 + w1) + w2) + w3.
  sparse_u / sparse_trip  -- in the order of k_exps_grad_u / k_exps_trip (csrc/cpm_expected_sparse_grad.h): only the STORED cells of the
                             row, in ascending d.

The contract of the sparse calls is that the two agree in every bit, the sign of a zero included.  Layouts: p_t[o, d] one hour of
p_dest[o, d, t] as the library takes it; mean_t[o, d], dist[o, d] likewise; part[s, o] the segments' sums."""
import numpy as np

STRIP, SEG_MIN, MAX_SEG = 128, 32, 64          # kGradStrip, kGradSegMin, kGradMaxSeg
TRIP_MAX_SEG = 8                               # kTripMaxSeg
INTRA_SEC, INTRA_KM = 300.0, 1.0               # kTripIntraSec, kTripIntraKm


def grad_segments(Z):
    strips = (Z + STRIP - 1) // STRIP
    n = (1024 + strips - 1) // strips
    n = min(n, Z // SEG_MIN, MAX_SEG)
    return max(n, 1)


def trip_segments(Z, T):
    base = ((Z + STRIP - 1) // STRIP) * T
    n = (1024 + base - 1) // base
    n = min(n, (Z + 63) // 64, TRIP_MAX_SEG)
    return max(n, 1)


def segment_len(Z, nseg):
    return (Z + nseg - 1) // nseg


def combine(w):
    return ((w[0] + w[1]) + w[2]) + w[3]


def dense_parts(p_t, values, nseg):
    """part[s, o] with the term p_t[o, d] * values[o, d] (values may be (Z,): one word per destination); all origins in one numpy step"""
    Z = p_t.shape[0]
    seg_len = segment_len(Z, nseg)
    values = np.broadcast_to(values, (Z, Z))
    part = np.zeros((nseg, Z))
    for s in range(nseg):
        begin, end = s * seg_len, min(s * seg_len + seg_len, Z)
        w = [np.zeros(Z) for _ in range(4)]
        for d in range(begin, end):                      # (an empty trailing segment: no step, +0)
            v = (d - begin) & 3
            w[v] = w[v] + p_t[:, d] * values[:, d]
        part[s] = combine(w)
    return part


def rows_of(p_t, keep_zero=()):
    """the stored cells of every origin's row, sorted by destination: the cells with p != 0, and those named in keep_zero = {(o, d)}
    (cells of weight 0 that the dataset route keeps)"""
    Z = p_t.shape[0]
    rows = [[] for _ in range(Z)]
    for o, d in zip(*np.nonzero(p_t)):
        rows[o].append((int(d), float(p_t[o, d])))
    for o, d in keep_zero:
        if p_t[o, d] == 0.0:
            rows[o].append((int(d), 0.0))
    return [sorted(r) for r in rows]


def sparse_parts(rows, value, Z, nseg, chain=None):
    """part[s, o] over the stored cells only; value(o, d) the second factor; chain(d, begin): the chain a cell goes to"""
    seg_len = segment_len(Z, nseg)
    chain = chain or (lambda d, begin: (d - begin) & 3)
    part = np.zeros((nseg, Z))
    for o, row in enumerate(rows):
        w = [[0.0] * 4 for _ in range(nseg)]
        for d, p in row:
            if d >= Z:
                continue
            s = d // seg_len
            v = chain(d, s * seg_len)
            prod = float(np.float64(p) * np.float64(value(o, d)))
            w[s][v] = float(np.float64(w[s][v]) + np.float64(prod))
        for s in range(nseg):
            part[s, o] = combine([np.float64(x) for x in w[s]])
    return part


def finish(part):
    """the finishing kernels' sum of the segments: ascending, starting from segment 0's word"""
    a = part[0].copy()
    for s in range(1, part.shape[0]):
        a = a + part[s]
    return a


def running_sum(rows, value, Z):
    """mutant: one running sum per row, without segments or chains"""
    u = np.zeros(Z)
    for o, row in enumerate(rows):
        a = 0.0
        for d, p in row:
            if d < Z:
                a = float(np.float64(a) + np.float64(p) * np.float64(value(o, d)))
        u[o] = a
    return u


def dense_u(p_t, mu):
    return dense_parts(p_t, mu, grad_segments(p_t.shape[0]))


def sparse_u(rows, mu, Z, chain=None):
    return sparse_parts(rows, lambda o, d: mu[d], Z, grad_segments(Z), chain)


def trip_values(mean_t, dist):
    """sec(o, d) and km(o, d) with the diagonal selected"""
    Z = mean_t.shape[0]
    eye = np.eye(Z, dtype=bool)
    return np.where(eye, INTRA_SEC, mean_t), np.where(eye, INTRA_KM, dist)


def dense_trip(p_t, mean_t, dist, T):
    sec, km = trip_values(mean_t, dist)
    nseg = trip_segments(p_t.shape[0], T)
    return dense_parts(p_t, sec, nseg), dense_parts(p_t, km, nseg)


def sparse_trip(rows, mean_t, dist, Z, T):
    nseg = trip_segments(Z, T)
    sec = lambda o, d: INTRA_SEC if d == o else mean_t[o, d]
    km = lambda o, d: INTRA_KM if d == o else dist[o, d]
    return sparse_parts(rows, sec, Z, nseg), sparse_parts(rows, km, Z, nseg)


def kept_zero_cells(p_t):
    """for every fourth row with a positive cell: a kept cell of weight 0 before and one behind the row's last positive cell"""
    Z = p_t.shape[0]
    keep = []
    for o in range(0, Z, 4):
        pos = np.nonzero(p_t[o] > 0.0)[0]
        if len(pos) == 0:
            continue
        last = int(pos[-1])
        before = [d for d in range(last) if p_t[o, d] == 0.0]
        behind = [d for d in range(last + 1, Z) if p_t[o, d] == 0.0]
        if before:
            keep.append((o, before[len(before) // 2]))
        if behind:
            keep.append((o, behind[0]))
    return keep


def cotangent(Z, T, seed=5):
    """mu (T, Z): negative entries, exact zeros, and the last hour all zeros"""
    rng = np.random.default_rng(seed * 7919 + Z)
    mu = rng.normal(0.0, 1.0, (T, Z))
    mu[rng.random((T, Z)) < 0.2] = 0.0
    mu[T - 1] = 0.0
    return mu
