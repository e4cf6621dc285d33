"""The backward product along a tangent of p_destin, restated for the compact tangent (include/cpm_expected_sparse_dest.h), one IEEE
f64 operation per step, on top of expected_sparse_grad_reference:

  dense_w / dense_trip_tan    -- in the order of k_exp_grad_dest_u / k_exp_trip on the dense tangent: EVERY destination of the row,
                                 zeros included, in its segment and chain.
  sparse_w / sparse_trip_tan  -- in the order of k_exps_grad_dest_u / k_exps_trip on the rows of sdp: the STORED cells only.

and the builder of d p_destin / d e_dest on the stored cells (k_exps_tan_cells), and the hand-made tables whose rows have the lengths
at which the kernels' row walk takes another path.  Layouts as in expected_sparse_grad_reference: dP_t[o, d] one hour of dP[o, d, t]."""
import functools

import numpy as np

import expected_sparse_grad_reference as G
import expected_sparse_reference as S

# rows of the walk tables, by origin: cells in the row.  One chunk of 64, a chunk boundary, the four chunks requested ahead, beyond them.
WALK_ROWS = {0: 0, 1: 1, 2: 63, 3: 64, 4: 65, 5: 255, 6: 256, 7: 257, 8: 309}
WALK_ONE_SEGMENT, WALK_EVERY_SEGMENT = 9, 10     # a row whose cells all lie in one segment; a row with one cell in every segment


def signed_tangent_on_cells(p_t, keep, seed):
    """dP_t (Z, Z): signed values on the stored cells (p != 0, and the kept cells of weight 0, which carry a non-zero tangent), every
    row summing to 0 up to rounding, exactly +0 off the stored cells"""
    Z = p_t.shape[0]
    stored = p_t != 0.0
    for o, d in keep:
        stored[o, d] = True
    rng = np.random.default_rng(seed)
    dP = np.where(stored, rng.uniform(-1.0, 1.0, (Z, Z)), 0.0)
    n = stored.sum(axis=1, keepdims=True)
    mean = np.divide(dP.sum(axis=1, keepdims=True), n, out=np.zeros((Z, 1)), where=n > 0)
    dP = np.where(stored, dP - mean, 0.0)
    dP[stored & (dP == 0.0)] = 0.25                       # (a stored cell is never an accidental zero; single-cell rows get a value)
    return dP, stored


def tangent_rows(rows, dP_t):
    """the rows of sdp: entry for entry with the rows of sp"""
    return [[(d, float(dP_t[o, d])) for d, _ in row] for o, row in enumerate(rows)]


def dense_w(dP_t, mu):
    return G.dense_parts(dP_t, mu, G.grad_segments(dP_t.shape[0]))


def sparse_w(trows, mu, Z, chain=None):
    return G.sparse_parts(trows, lambda o, d: mu[d], Z, G.grad_segments(Z), chain)


def dense_trip_tan(dP_t, mean_t, dist, T):
    return G.dense_trip(dP_t, mean_t, dist, T)


def sparse_trip_tan(trows, mean_t, dist, Z, T):
    return G.sparse_trip(trows, mean_t, dist, Z, T)


def build_row(x_row, p_row, log=np.log):
    """k_exps_tan_cells on one row's cells (ascending destination): m = m + p * log(x) over p > 0, then p * (log(x) - m); +0 at p == 0"""
    m = np.float64(0.0)
    for x, p in zip(x_row, p_row):
        if p > 0.0:
            m = m + np.float64(p) * log(np.float64(x))
    return [float(np.float64(p) * (log(np.float64(x)) - m)) if p > 0.0 else 0.0 for x, p in zip(x_row, p_row)]


@functools.lru_cache(maxsize=None)
def walk_tables(Z, T, seed=19):
    """(p_drive, p_dest (Z, Z, T) F-order): S.sparse_tables with the first rows of every hour replaced by rows of WALK_ROWS' lengths
    (cells spread over the whole row), a row inside one segment and a row with a cell in every segment.  Needs Z >= 320; an uploaded table takes sparse row packs only while its longest row is short beside Z."""
    p_drive, p, _ = S.sparse_tables(Z, T)
    p = np.array(p, order="F")
    rng = np.random.default_rng(seed + Z)
    nseg = G.grad_segments(Z)
    seg_len = G.segment_len(Z, nseg)
    for t in range(T):
        for o, n in WALK_ROWS.items():
            p[o, :, t] = 0.0
            cells = np.sort(rng.choice(Z, size=n, replace=False))
            if n:
                w = rng.uniform(0.1, 1.0, n)
                p[o, cells, t] = w / w.sum() * (1.0 - 2.0 ** -40)
        p[WALK_ONE_SEGMENT, :, t] = 0.0
        cells = np.arange(seg_len, min(2 * seg_len, Z))                  # all of segment 1
        p[WALK_ONE_SEGMENT, cells, t] = (1.0 - 2.0 ** -40) / len(cells)
        p[WALK_EVERY_SEGMENT, :, t] = 0.0
        cells = np.array([s * seg_len + s % (min(s * seg_len + seg_len, Z) - s * seg_len) for s in range(nseg) if s * seg_len < Z])
        p[WALK_EVERY_SEGMENT, cells, t] = 0.5 / len(cells)               # (a residual row as well)
    for a in (p,):
        a.setflags(write=False)
    return p_drive, p
