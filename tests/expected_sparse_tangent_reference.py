"""One operator of the forward tangent restated twice, one IEEE f64 operation per step (include/cpm_expected_sparse_tangent.h), on top
of expected_sparse_reference (the lane rule, the block sum, the residual lists) and expected_sparse_dest_reference (signed tangents on
the stored cells, the walk tables):

  order="dense"   -- k_tan_hour (csrc/cpm_expected_tangent.h): EVERY origin of the dense row of p under the primal x and the SIGNED dx,
                     and every origin of the dense row of dP under the masked primal xm, zeros included, each to its lane;
  order="sparse"  -- k_exps_tan_hour (csrc/cpm_expected_sparse_tangent.h): only the STORED cells of a destination column, sorted by
                     (lane, place in the lane), with cell_dp entry for entry beside cell_p;

then the same tree and the tangent's epilogue: dstay, (dstay + y) + res, the zero row, + c * u, dx_next.  The contract of the sparse
calls is that the two agree in every bit, the signs of zeros included.  Layouts: p_t[o, d] and dP_t[o, d] one hour of the library's
[o, d, t] arrays."""
import functools

import numpy as np

import expected_sparse_dest_reference as SD
import expected_sparse_grad_reference as G
import expected_sparse_reference as S


def inside(q_raw):
    """where p_drive is strictly inside (0, 1): a direction of p_drive counts only there (a select: NaN does not pass)"""
    q_raw = np.asarray(q_raw, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (q_raw > 0.0) & (q_raw < 1.0)


def tan_dq(q_raw, dq_raw):
    return np.where(inside(q_raw), dq_raw, 0.0)


def tangent_columns(cols, dP_t):
    """cell_dp: the tangent at the cells of every column, entry for entry with cols (k_exps_cells_dp)"""
    return [[(o, float(dP_t[o, d])) for o, _ in col] for d, col in enumerate(cols)]


def column_sums(order, vec, p_t, cols, t, key=S.lane_key):
    """y[d] = sum over o of vec[o] * p[o, d] in the order of `order`; vec may be signed (dx) and p_t may be the tangent (u)"""
    if order == "dense":
        return S.dense_y(p_t, vec, t)
    return S.sparse_y(cols, vec, p_t.shape[0], t, key)


def operator(order, p_t, dP_t, cols, dcols, pi, dpi, q_raw, dq_raw, c, t, qn_raw=None, dqn_raw=None, key=S.lane_key, u_on="xm"):
    """One operator of hour t for the primal and one direction.  Returns dict(pi_next, x_next, dpi_next, dx_next, y, dy, u): the words
    k_tan_hour / k_exps_tan_hour store, and the column sums behind them.  c: c_dest of the direction (u is formed when c != 0).
    u_on="x" is the mutant that forgets the mask of the zero rows."""
    Z = p_t.shape[0]
    q = S.exp_q(q_raw)
    dq = tan_dq(q_raw, np.zeros(Z) if dq_raw is None else dq_raw)
    x = pi * q
    a, b = dpi * q, pi * dq
    dx = a + b
    last = S.row_last(p_t)
    ell, r = S.aux(p_t, last)
    zero = last == 0.0
    y = column_sums(order, x, p_t, cols, t, key)
    dy = column_sums(order, dx, p_t, cols, t, key)
    pi_next = S._tail(y, pi, q, x, last, ell, r)                   # the primal: k_exp_hour's epilogue
    s1, s2 = dpi * (1.0 - q), pi * dq
    dstay = s1 - s2
    v = dstay + dy
    v = v + S._residuals(dx, ell, r, Z)
    v = np.where(zero, v + dx, v)
    u = None
    if c != 0.0:
        xm = x if u_on == "x" else np.where(zero, 0.0, x)
        u = column_sums(order, xm, dP_t, dcols, t, key)
        v = v + c * u
    out = dict(pi_next=pi_next, dpi_next=v, y=y, dy=dy, u=u)
    if qn_raw is not None:
        qn = S.exp_q(qn_raw)
        dqn = tan_dq(qn_raw, np.zeros(Z) if dqn_raw is None else dqn_raw)
        t1, t2 = v * qn, pi_next * dqn
        out.update(x_next=pi_next * qn, dx_next=t1 + t2)
    return out


# ------------------------------------------------------------------ the hand-made case of the CPU order tests
@functools.lru_cache(maxsize=None)
def order_case(Z, T=2):
    """S.sparse_tables(Z, T) with, per hour: G.kept_zero_cells (kept cells of weight 0), a kept cell on every ZERO row, a column whose
    only two cells hold the same weight (for terms that cancel exactly), a signed tangent on all stored cells; p_drive with the two
    origins of that column sharing one q, the zero rows' q inside (0, 1) and no q = 0 in the last hour; pi > 0 on the zero rows, zeros elsewhere.  Computed once,
    shared; nobody writes to it.  Returns dict(p_drive, hours=[dict(p_t, dP_t, keep, cols, dcols, stored)], info, cancel=(d, o1, o2) or None,
    empty=d or None, pi)."""
    p_drive, p_dest, info = S.sparse_tables(Z, T)
    p_drive = np.array(p_drive)
    rng = np.random.default_rng(4000 + Z)
    empty = list(info["empty"])
    cancel = None
    if len(empty) > 1:                                              # one empty column becomes the cancelling one, the other stays empty
        o1, o2 = sorted(info["half"])[:2]                           # rows that total 0.5: room for one more cell
        cancel = (empty[0], o1, o2)
        p_drive[o2, :] = p_drive[o1, :] = 0.375
    still_empty = empty[-1] if empty else None
    for o in info["zero"]:
        p_drive[o, :] = 0.625
    p_drive[p_drive[:, T - 1] == 0.0, T - 1] = 0.5                  # the last hour: q > 0 everywhere (dx of one sign has no zeros there)
    pi = rng.uniform(0.25, 2.0, Z)
    pi[rng.random(Z) < 0.3] = 0.0
    for o in info["zero"]:
        pi[o] = 1.5
    hours = []
    for t in range(T):
        p_t = np.array(p_dest[:, :, t])
        if cancel:
            p_t[cancel[1], cancel[0]] = p_t[cancel[2], cancel[0]] = 2.0 ** -6
        keep = [(o, d) for o, d in G.kept_zero_cells(p_t) if d not in empty]      # (the two columns above keep their cells as planned)
        for o in info["zero"]:
            if not p_t[o].any():                                    # a zero row (not in the last hour) keeps a cell that carries a tangent
                keep.append((o, next(d % Z for d in range(o + 7, o + 7 + Z) if d % Z not in empty)))
        dP_t, stored = SD.signed_tangent_on_cells(p_t, keep, 5000 + 7 * Z + t)
        cols = S.columns_of(p_t, keep)
        hours.append(dict(p_t=p_t, dP_t=dP_t, keep=keep, cols=cols, dcols=tangent_columns(cols, dP_t), stored=stored))
    p_drive.setflags(write=False)
    pi.setflags(write=False)
    return dict(p_drive=p_drive, hours=hours, info=info, cancel=cancel, empty=still_empty, pi=pi)


def order_directions(case, Z, T=2):
    """[(name, dpi (Z,), dq (Z, T) or None, c)]: signed; one that cancels exactly in the cancel column; one whose every dx is negative"""
    rng = np.random.default_rng(6000 + Z)
    signed = (rng.uniform(-1.0, 1.0, Z), rng.uniform(-1.0, 1.0, (Z, T)), -0.75)
    dpi = rng.uniform(-1.0, 1.0, Z)
    if case["cancel"]:
        _, o1, o2 = case["cancel"]
        dpi[o1], dpi[o2] = 0.8125, -0.8125                          # with one q and one weight: dx * p cancels exactly
    negative = (-rng.uniform(0.5, 1.0, Z), None, 0.0)               # dq = 0: dx = dpi * q <= 0, < 0 where q > 0
    return [("signed",) + signed, ("cancel", dpi, None, 1.0), ("negative",) + negative]
