"""One hour of the expected densities restated twice, one IEEE f64 operation per step (include/cpm_expected_sparse.h):

  dense_hour   -- in the order of k_exp_hour (csrc/cpm_expected.h): every origin of the dense row, zeros included, goes to its lane;
                  the 64-lane shfl_down tree; the four waves in order; the residual lists the same way; (stay + y) + res (+ x).
  sparse_hour  -- in the order of k_exps_hour (csrc/cpm_expected_sparse.h): only the STORED cells of a destination column, sorted by
                  the key (lane, place in the lane), then the same tree and the same tail.

The contract of the sparse calls is that the two agree in every bit.  brute_walk() replays the loop indices of exp_stream -- which thread
touches which origin, in what order -- and is what the key rule is checked against.  Layouts: p_dest[o, d, t] as the library takes it."""
import functools

import numpy as np

LANES, WAVES, ROUND = 256, 4, 512          # kExpBlock, kExpWaves, kExpBlock * kExpUnroll


def head(Z, t, d):
    """the dense row of (t, d) starts 8 bytes behind a 16-byte line of the aligned [T][Z][Z] array"""
    return (Z & 1) == 1 and ((t * Z * Z + d * Z) & 1) == 1


def lane_key(o, Z, hd):
    """(lane, place in the lane) of origin o -- the lane rule of the header"""
    if not hd:
        if o >= (Z & ~1):
            return (0, Z)                  # odd Z: the last origin, behind lane 0's pairs
        return ((o >> 1) & 255, o)
    if o == 0:
        return (0, Z)                      # the first origin, behind lane 0's pairs
    return (((o - 1) >> 1) & 255, o)


def mutant_key(o, Z, hd):
    """a column sorted by origin alone: the lanes do not wrap at o >= 512 (what lies past lane 255 stays there)"""
    lane, place = lane_key(o, Z, hd)
    unwrapped = (o >> 1) if not hd else ((o - 1) >> 1 if o else 0)
    return (min(unwrapped, 255) if place != Z else 0, place)


def brute_walk(Z, hd):
    """exp_stream's loops, index for index: the origins thread tid multiplies, in order"""
    npairs = Z >> 1
    h = 1 if hd else 0
    out = []
    for tid in range(LANES):
        seq = []
        for k0 in range(tid, npairs, ROUND):
            for u in range(2):
                k = k0 + u * LANES
                if k < npairs:
                    seq += [h + 2 * k, h + 2 * k + 1]
        if (Z & 1) and tid == 0:
            seq.append(0 if hd else Z - 1)
        out.append(seq)
    return out


def wave_tree(v):
    """obj_wave_sum over the lanes (last axis, 64 long): v = v + shfl_down(v, o) for o = 32 .. 1 (a lane past the end reads itself)"""
    v = np.array(v, dtype=np.float64)
    o = 32
    while o > 0:
        shifted = np.concatenate([v[..., o:], v[..., 64 - o:]], axis=-1)
        v = v + shifted
        o >>= 1
    return v[..., 0]


def block_sum(acc):
    """exp_block_sum: acc[..., 256] -> the wave tree, then ((w0 + w1) + w2) + w3"""
    acc = np.asarray(acc, dtype=np.float64)
    w = wave_tree(acc.reshape(acc.shape[:-1] + (WAVES, 64)))
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def exp_q(v):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(~(v > 0.0), 0.0, np.where(v >= 1.0, 1.0, v))


def row_last(p_t):
    """the f64 left-to-right total of every origin's row (p_t[o, d])"""
    tot = np.zeros(p_t.shape[0])
    for d in range(p_t.shape[1]):
        tot = tot + p_t[:, d]
    return tot


def aux(p_t, last):
    """ell (last destination with p > 0, Z for a zero row), r = max(0, 1 - last)"""
    Z = p_t.shape[0]
    res = 1.0 - last
    r = np.where(res > 0.0, res, 0.0)
    ell = np.full(Z, Z, dtype=np.int64)
    for o in range(Z):
        if last[o] != 0.0:
            pos = np.nonzero(p_t[o] > 0.0)[0]
            if len(pos):
                ell[o] = pos[-1]
    return ell, r


def _residuals(x, ell, r, Z):
    """res[d]: x[o] * r[o] over the origins whose ell is d, ascending, thread tid taking every 256th of them; then block_sum"""
    res = np.zeros(Z)
    for d in range(Z):
        lst = np.nonzero(ell == d)[0]
        if len(lst) == 0:
            continue
        acc = np.zeros(LANES)
        for k, o in enumerate(lst):
            acc[k % LANES] = acc[k % LANES] + x[o] * r[o]
        res[d] = block_sum(acc)
    return res


def _tail(y, pi, q, x, last, ell, r):
    Z = len(pi)
    stay = pi * (1.0 - q)
    v = stay + y
    v = v + _residuals(x, ell, r, Z)
    return np.where(last == 0.0, v + x, v)


def dense_y(p_t, x, t):
    """y[d] in k_exp_hour's order; the destinations of one alignment at a time, every lane's next origin in one numpy step"""
    Z = p_t.shape[0]
    y = np.zeros(Z)
    for hd in (False, True):
        ds = np.array([d for d in range(Z) if head(Z, t, d) == hd], dtype=np.int64)
        if len(ds) == 0:
            continue
        walk = brute_walk(Z, hd)
        acc = np.zeros((len(ds), LANES))
        for j in range(max(len(s) for s in walk)):
            lanes = np.array([l for l in range(LANES) if j < len(walk[l])], dtype=np.int64)
            os_ = np.array([walk[l][j] for l in lanes], dtype=np.int64)
            prod = x[os_][None, :] * p_t[os_][:, ds].T          # (zeros included: x * 0 = +0)
            acc[:, lanes] = acc[:, lanes] + prod
        y[ds] = block_sum(acc)
    return y


def sparse_y(cols, x, Z, t, key=lane_key):
    """y[d] in k_exps_hour's order: cols[d] = [(o, p), ...] the stored cells of the column in any order"""
    y = np.zeros(Z)
    for d in range(Z):
        hd = head(Z, t, d)
        acc = [0.0] * LANES
        for o, p in sorted(cols[d], key=lambda c: key(c[0], Z, hd)):
            lane = key(o, Z, hd)[0]
            prod = float(np.float64(x[o]) * np.float64(p))
            acc[lane] = float(np.float64(acc[lane]) + np.float64(prod))
        y[d] = block_sum(np.array(acc))
    return y


def columns_of(p_t, keep_zero=()):
    """the stored cells of every destination column: the cells with p != 0, and those named in keep_zero = {(o, d)} (cells of weight 0
    that the dataset route keeps)"""
    Z = p_t.shape[0]
    cols = [[] for _ in range(Z)]
    for o, d in zip(*np.nonzero(p_t)):
        cols[d].append((int(o), float(p_t[o, d])))
    for o, d in keep_zero:
        if p_t[o, d] == 0.0:
            cols[d].append((int(o), 0.0))
    return cols


def dense_hour(p_t, pi, q_raw, t):
    q = exp_q(q_raw)
    x = pi * q
    last = row_last(p_t)
    ell, r = aux(p_t, last)
    return _tail(dense_y(p_t, x, t), pi, q, x, last, ell, r)


def sparse_hour(p_t, pi, q_raw, t, keep_zero=(), key=lane_key):
    q = exp_q(q_raw)
    x = pi * q
    last = row_last(p_t)
    ell, r = aux(p_t, last)
    return _tail(sparse_y(columns_of(p_t, keep_zero), x, p_t.shape[0], t, key), pi, q, x, last, ell, r)


# ------------------------------------------------------------------ the hand-made tables of the CPU and GPU cases
@functools.lru_cache(maxsize=None)
def sparse_tables(Z, T, seed=7, density=None):
    """(p_drive (Z, T), p_dest (Z, Z, T) F-order, info): random sparse rows with
      * a destination that EVERY origin of the last hour leads to (a column holding every origin), and most origins of the others;
      * destinations nobody leads to (empty columns);
      * all-zero rows in every hour but the last (the driver stays), rows that total 0.5 (residual rows) and single-cell rows;
    computed once and shared; nobody writes to them."""
    rng = np.random.default_rng(seed * 100003 + Z * 31 + T)
    if density is None:
        density = min(0.5, max(0.04, 12.0 / Z))
    w = rng.random((Z, Z, T))
    w[rng.random((Z, Z, T)) >= density] = 0.0
    full = (2 * Z) // 3
    empty = sorted({Z // 5, Z - 1 if Z > 4 else Z // 2} - {full})
    w[:, full, :] = rng.random((Z, T)) + 0.01
    w[:, empty, :] = 0.0
    tot = w.sum(axis=1, keepdims=True)
    p = np.divide(w, tot, out=np.zeros_like(w), where=tot > 0)
    p *= 1.0 - 2.0 ** -40                                        # (no row total above 1 by rounding)
    half = [o for o in {1 % Z, Z // 2, Z - 2 if Z > 2 else 0}]
    p[half, :, :] *= 0.5                                         # rows that total 0.5: residuals
    zero = [o for o in {0, Z // 3} if Z > 2]
    p[zero, :, :T - 1] = 0.0                                     # zero rows, not in the last hour
    p = np.asfortranarray(p)
    p_drive = np.asfortranarray(rng.uniform(0.05, 0.95, (Z, T)))
    p_drive[rng.random((Z, T)) < 0.05] = 0.0
    p_drive[rng.random((Z, T)) < 0.05] = 1.0
    for a in (p, p_drive):
        a.setflags(write=False)
    return p_drive, p, {"full": full, "empty": empty, "half": half, "zero": zero}


def pi0_with_zeros(Z, seed=3):
    pi = np.random.default_rng(seed + Z).uniform(0.0, 2.0, Z)
    pi[:: 3] = 0.0
    return pi
