"""One backward operator's three sums of the seed variances (include/cpm_expected_sparse_var.h), restated twice, one IEEE f64 operation
per step:

  dense_sums    -- in the order of k_elv_u / k_etv_u (csrc/cpm_expected_linear_var.h, csrc/cpm_expected_travel_var.h): EVERY destination
                   of origin o's row, zeros included, goes to chain (d - begin) & 3 of its segment; a chain starts at +0 and adds
                   acc = acc + term in ascending d; ((c0 + c1) + c2) + c3.
  sparse_sums   -- in the order of k_exps_elv_u / k_exps_etv_u (csrc/cpm_expected_sparse_var.h): only the STORED cells of the row, in
                   ascending d.

The term of a cell, for the count form: e = mu[d] - mu[o]; t = p * e; the three products t, t * e, p * nu[d].  For the travel form:
z = (mu[d] - mu[o]) + (S[o] * sec + D[o] * km); t = p * z; t, t * z, p * nu[d].  The contract of the sparse calls is that the two
orders agree in every bit, the sign of a zero included.  Layouts: p_t[o, d] one hour of p_dest[o, d, t]; sec[o, d], km[o, d] with
the diagonal selected (expected_sparse_grad_reference.trip_values); part[s, kind, o] the segments' sums, kind = s1, s2, b.

dense_vsec / sparse_vsec are the two orders of the trip variance weight: the walkers of expected_sparse_grad_reference over
trip_segments with the term p * var_sec (0 on the diagonal)."""
import numpy as np

import expected_sparse_grad_reference as G


def edge(S, D, sec, km):
    """e[o, d] = S[o] * sec[o, d] + D[o] * km[o, d]: two products and a sum"""
    return S[:, None] * sec + D[:, None] * km


def dense_sums(p_t, mu, nu, e=None):
    """part[s, kind, o]; e: None (the count form) or the (Z, Z) edge reward of the travel form; all origins in one numpy step"""
    Z = p_t.shape[0]
    nseg = G.grad_segments(Z)
    seg_len = G.segment_len(Z, nseg)
    part = np.zeros((nseg, 3, Z))
    for s in range(nseg):
        begin, end = s * seg_len, min(s * seg_len + seg_len, Z)
        w = [[np.zeros(Z) for _ in range(4)] for _ in range(3)]
        for d in range(begin, end):                      # (an empty trailing segment: no step, +0)
            v = (d - begin) & 3
            z = mu[d] - mu                               # centred at the origin's own mu[o], inside the term
            if e is not None:
                z = z + e[:, d]
            t = p_t[:, d] * z
            w[0][v] = w[0][v] + t
            w[1][v] = w[1][v] + t * z
            w[2][v] = w[2][v] + p_t[:, d] * nu[d]
        for k in range(3):
            part[s, k] = G.combine(w[k])
    return part


def sparse_sums(rows, mu, nu, Z, e=None, chain=None):
    """part[s, kind, o] over the stored cells only; e(o, d): the edge reward or None; chain(d, begin): the chain a cell goes to"""
    nseg = G.grad_segments(Z)
    seg_len = G.segment_len(Z, nseg)
    chain = chain or (lambda d, begin: (d - begin) & 3)
    part = np.zeros((nseg, 3, Z))
    for o, row in enumerate(rows):
        w = [[[0.0] * 4 for _ in range(3)] for _ in range(nseg)]
        mo = float(mu[o])
        for d, p in row:
            if d >= Z:
                continue
            s = d // seg_len
            v = chain(d, s * seg_len)
            z = float(mu[d]) - mo
            if e is not None:
                z = z + e(o, d)
            t = p * z
            tz = t * z
            pn = p * float(nu[d])
            w[s][0][v] = w[s][0][v] + t
            w[s][1][v] = w[s][1][v] + tz
            w[s][2][v] = w[s][2][v] + pn
        for s in range(nseg):
            for k in range(3):
                part[s, k, o] = G.combine([np.float64(x) for x in w[s][k]])
    return part


def edge_of(S, D, sec, km):
    """the same edge reward per stored cell, in Python floats: (S[o] * sec) + (D[o] * km)"""
    return lambda o, d: float(S[o]) * float(sec[o, d]) + float(D[o]) * float(km[o, d])


def finish(part):
    """the finishing kernels' sum of the segments per kind: (3, Z)"""
    return np.stack([G.finish(part[:, k]) for k in range(3)])


def uncentred_sums(rows, mu, nu, Z):
    """mutant: the shortcut on compact rows -- the raw moments sum p, sum p * mu, sum (p * mu) * mu in the sparse order, centred
    afterwards: s1 = m1 - mu[o] * m0, s2 = (m2 - (2 mu[o]) * m1) + (mu[o] * mu[o]) * m0.  -> (3, Z) like finish()"""
    nseg = G.grad_segments(Z)
    seg_len = G.segment_len(Z, nseg)
    raw = np.zeros((3, Z))
    m0 = G.finish(G.sparse_parts(rows, lambda o, d: 1.0, Z, nseg))
    m1 = G.finish(G.sparse_parts(rows, lambda o, d: mu[d], Z, nseg))
    m2 = np.zeros(Z)
    for o, row in enumerate(rows):
        w = [[0.0] * 4 for _ in range(nseg)]
        for d, p in row:
            if d < Z:
                s = d // seg_len
                v = (d - s * seg_len) & 3
                w[s][v] = w[s][v] + (p * float(mu[d])) * float(mu[d])
        tot = None
        for s in range(nseg):
            c = G.combine([np.float64(x) for x in w[s]])
            tot = c if tot is None else tot + c
        m2[o] = tot
    raw[0] = m1 - mu * m0
    raw[1] = (m2 - (2.0 * mu) * m1) + (mu * mu) * m0
    raw[2] = G.finish(G.sparse_parts(rows, lambda o, d: nu[d], Z, nseg))
    return raw


def state(Z, seed, zeros=False):
    """(mu, nu): signed mu with exact zeros and pairs of equal words (eta = 0 exactly), nu >= 0; zeros: the hour of all zeros"""
    if zeros:
        return np.zeros(Z), np.zeros(Z)
    rng = np.random.default_rng(seed * 6007 + Z)
    mu = rng.normal(0.0, 3.0, Z)
    mu[rng.random(Z) < 0.15] = 0.0
    mu[1::7] = mu[0]                                     # destinations whose mu is the origin's: terms of exactly 0
    nu = rng.uniform(0.0, 5.0, Z)
    nu[rng.random(Z) < 0.15] = 0.0
    return mu, nu


def plant_cancellation(p_t, mu, o=2):
    """in place: origin o's row becomes two cells of weight 0.25 at destinations 1 and 5, the same chain of segment 0, and mu is set so
    that mu[1] - mu[o] = 1.5 = -(mu[5] - mu[o]): the chain's s1 is 0.375 - 0.375, +0 exactly, where s2 is not.  Needs seg_len >= 6."""
    p_t[o, :] = 0.0
    p_t[o, 1] = p_t[o, 5] = 0.25
    mu[o], mu[1], mu[5] = 0.5, 2.0, -1.0


def dense_vsec(p_t, var_sec, T):
    """part[s, o] of the trip variance weight in k_exp_trip_var's order; var_sec[o, d] with 0 on the diagonal"""
    return G.dense_parts(p_t, var_sec, G.trip_segments(p_t.shape[0], T))


def sparse_vsec(rows, var_sec, Z, T):
    return G.sparse_parts(rows, lambda o, d: 0.0 if d == o else var_sec[o, d], Z, G.trip_segments(Z, T))
