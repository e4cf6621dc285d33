/*
 * cpm_expected_linear_var.h -- the exact mean and seed variance of any linear functional of a resample's counts of libcpm_hip.so,
 * from one backward pass over the installed p_destin tables, without a car or a random number.
 *
 * cpm_expected_var.h gives the variance of every single count parking[t][z] and driving[t][z].  The sweep reads sums over cells --
 * driving_sum[t], the errors of whole rows and columns -- and the cells are strongly correlated (a car that is in one zone is in no
 * other), so the per-cell variances say nothing about them.  Cars move independently given their start zones, so the variance of a
 * linear functional is a sum over the cars of the variance of one car's reward along its path, and that follows from a backward
 * recurrence over the chain: the traffic of cpm_expected_grad's backward pass, with no forward pass.  Covariances across hours are
 * included: the car-hours parked in a zone over the day are one functional.
 *
 * Definition.  Terms are those of cpm_expected.h and cpm_expected_grad.h: q (p_drive as the Bernoulli maps it), p[t][d][o] =
 * p_destin[o, d, t], last, l, r, zero rows, the row-total refusal (CPM_ERR_TABLE), CPM_EXPECT_IVP; the operators s = 0 .. N-1,
 * N = pre + T, pre = T - 1 under CPM_EXPECT_IVP and 0 otherwise, t(s) = s for s < pre and s - pre otherwise, j = s - pre.
 * Functional k of K has two coefficient arrays A_k[T][Z] and B_k[T][Z]:
 *   L_k = the sum over t, z of A_k[t][z] * parking[t][z] + B_k[t][z] * driving[t][z]     (cpm_resample's integer counts).
 * With w[s] cars starting in zone s (w = the cars per zone of cpm_init_states, or the histogram of cpm_get_state; under
 * CPM_EXPECT_IVP the placement in front of cpm_solve_ivp):
 *   mean_k = the sum over s of w[s] * V_0[s],     var_k = the sum over s of w[s] * W_0[s],
 * where V is the expected remaining reward of one car given its zone and W the variance of that reward.
 *
 * Backward pass.  Every step is ONE IEEE f64 operation (the library is built with -ffp-contract=off).  mu = nu = 0; for s = N-1
 * down to 0, with t = t(s), gp = A_k[j] and gd = B_k[j] (both 0 for j < 0, an operator in front of the day), for origin o:
 *   a zero row (last == 0): the drive leaves the car at o, still counted as driving: s1 = 0, s2 = 0, b = nu[o];
 *   otherwise, with eta[d] = mu[d] - mu[o], the deviation from the value of staying,
 *     s1 = (the sum over d of p[o, d] * eta[d])            + r[o] * eta[l[o]]
 *     s2 = (the sum over d of (p[o, d] * eta[d]) * eta[d]) + (r[o] * eta[l[o]]) * eta[l[o]]
 *     b  = (the sum over d of p[o, d] * nu[d])             + r[o] * nu[l[o]]          (the second terms only where l[o] exists);
 *   db = gd[o] + s1;
 *   J  = q * ((1 - q) * (db * db) + max(0, s2 - s1 * s1));
 *   V[o] = (gp[o] + mu[o]) + q * db;
 *   W[o] = ((1 - q) * nu[o] + q * b) + J;
 *   mu <- V, nu <- W.
 * (The probability that the centred sums leave with the origin is 1 - q * (sum p + r): where the f64 row total is not exact, its
 * rounding, at most Z * 2^-52, stays at o.)
 * The last operator (hour T-1, sampled and never applied) has mu = nu = 0: no product is formed, s1 = s2 = b = 0 and
 * J = q * ((1 - q) * (gd * gd)).
 *
 * The sums are centred at mu[o], and that is part of the contract: a functional that is constant over the zones of every hour (the
 * total count is C in every run) has every eta exactly 0 and gives a variance of exactly 0, where the raw moments
 * sum p * mu^2 - (sum p * mu)^2 would leave c^2 * Z * 2^-52 of noise.  The exact value of s2 - s1^2 is not negative for a row whose
 * total is at most 1 (Cauchy-Schwarz); it is clamped at 0.
 *
 * Order of the sums (no floating-point atomics; csrc/cpm_expected_linear_var.h): that of cpm_expected_grad.h.  The destinations are
 * cut into S consecutive segments of ceil(Z / S), S = max(1, min(64, floor(Z / 32), ceil(1024 / ceil(Z / 128)))); within a segment
 * destination d belongs to chain (d - begin) mod 4, a chain adds its terms in ascending d starting from 0, the four chains are added
 * in order, ((c0 + c1) + c2) + c3, then the segments in ascending order, then the residual term.  mean and var: chain i of 256 adds
 * w[z] * V_0[z] for z = i, i + 256, ... in ascending z starting from 0 (w NULL: the factor 1), then the 256 chains are added
 * pairwise, chain i + h to chain i for h = 128, 64, ... 1.  The order is a function of Z, T and the installed tables alone -- not of
 * K or a functional's place in the call: the same inputs give the same bits every time, and functional k of a call with K
 * functionals carries the bits of a K = 1 call on it.
 *
 * Error bound.  The terms are signed, so the bound is relative to the magnitude recurrence of non-negative terms: the same
 * recurrence with |gp|, |gd| in place of gp, gd, eta~[d] = mu~[d] + mu~[o] in place of eta, and s2~ + s1~ * s1~ in place of the
 * difference,
 *   s1~ = sum p * eta~ + r * eta~[l];  s2~ = sum p * eta~^2 + r * eta~[l]^2;  b~ = sum p * nu~[d] + r * nu~[l]
 *   (a zero row: s1~ = s2~ = 0, b~ = nu~[o]);
 *   db~ = |gd| + s1~;  J~ = q * ((1 - q) * db~^2 + (s2~ + s1~^2));  V~ = |gp| + mu~[o] + q * db~;  W~ = (1 - q) * nu~[o] + q * b~ + J~.
 * A product p * eta that ends up in a word of V passes the subtraction that forms eta, one multiplication, at most
 * ceil(ceil(Z / S) / 4) additions of its chain, 3 of the chains, S - 1 of the segments, 1 of the residual term, 1 into db, the
 * multiplication by q and 1 into V; every other term passes fewer.  That is at most R = ceil(ceil(Z / S) / 4) + S + 12 roundings of
 * 2^-53 each (the count of the operations that form J and W from the sums is rounded up into the 12), and K = 2 * R.  After n
 * backward operators a word of V lies within
 *   n * K * 2^-52 * V~
 * of its exact value, as a word of lambda in cpm_expected_grad.h.  W is of second degree in mu: an error of e * mu~ in mu moves
 * eta^2, s1^2 and db^2 by 2 * e of their magnitudes (up to second order), the roundings of an operator add at most (K + 4) * 2^-53
 * of J~ (s1 * s1 carries the roundings of s1 twice) and R * 2^-53 of the other terms, and nu carries its error through
 * the same non-negative recurrence: after n operators a word of W lies within
 *   2 * n * K * 2^-52 * W~
 * of its exact value.  W's terms are non-negative apart from s2 - s1^2, so the variance bound is relative to the magnitude word W~,
 * NOT to W itself: a functional whose variance nearly cancels (one that is nearly constant over the zones) has no relative bound,
 * as 1 - P has none in cpm_expected_var.h.  The totals add at most ceil(Z / 256) + 9 roundings of non-negative magnitudes:
 *   |mean_k - exact| <= (N * K + Z + 2) * 2^-52 * the sum of w * V~_0,   |var_k - exact| <= (2 * N * K + Z + 2) * 2^-52 * the sum of w * W~_0.
 * A word whose magnitude is 0 is 0.
 *
 * The calls need no cars, run no forward propagation, keep no Z x Z workspace and change no state of the context that a later call
 * reads.  They keep the state vectors of the passes and the segments' partial sums in a workspace of the context.  The first call
 * after the p_destin tables changed builds l and r and reads the row-total check back: it synchronises the stream once
 * (cpm_expected.h).  Tables with sparse row packs are expanded to the dense array first, as cpm_expected_var does; the same words
 * straight from the compact rows, without that array: cpm_expected_sparse_var.h.
 *
 * Status codes are those of cpm_expected_var: CPM_ERR_STATE without p_drive or p_destin tables, CPM_ERR_TABLE for a row total above
 * 1 (cpm_last_error() names the hour and the origin), CPM_ERR_HIP without a usable device, CPM_ERR_NOMEM for a failed allocation;
 * and CPM_ERR_ARG for a NULL coefficient or output array, unknown flag bits, K outside 1 .. CPM_MAX_BATCH and, in the blocking form,
 * a coefficient that is not finite or a start entry that is NaN, infinite or negative.  Conventions are those of cpm.h: int32
 * status, cpm_last_error(), no abort across the boundary, borrowed column-major host arrays.
 */
#ifndef CPM_EXPECTED_LINEAR_VAR_H
#define CPM_EXPECTED_LINEAR_VAR_H

#include "cpm_expected.h"

#ifdef __cplusplus
extern "C" {
#endif

/* enqueued on the context's stream.
 * d_start_or_null: DEVICE f64[Z] holding w; NULL: 1 per zone.  Read only.  flags: CPM_EXPECT_IVP or 0.
 * K: the number of functionals, 1 .. CPM_MAX_BATCH.
 * d_coeff: DEVICE f64[K][2][T][Z], A_k then B_k: the layout of cpm_expected_grad_dev's cotangent, K of them.  Read only.
 * d_out: DEVICE f64[K][2], mean then variance; every word written.
 * d_zone_or_null: DEVICE f64[K][2][Z], V_0 and W_0 per start zone; every word written.  The outputs are linear in w: a caller can
 * re-weigh them.  NULL: not wanted.
 * Nothing outside the two outputs is written. */
int32_t cpm_expected_linear_var_dev(cpm_ctx *ctx, const void *d_start_or_null, uint32_t flags, int32_t K, const void *d_coeff, void *d_out,
                                    void *d_zone_or_null);

/* blocking.  start_or_null: borrowed host f64[Z] or NULL.
 * a_parking / b_driving: Z x T x K Float64 column-major, the layout of cpm_resample_batch's count arrays.
 * mean / var: host f64[K].  zone_mean_or_null / zone_var_or_null: Z x K Float64 column-major, V_0 and W_0. */
int32_t cpm_expected_linear_var(cpm_ctx *ctx, const double *start_or_null, uint32_t flags, int32_t K, const double *a_parking,
                                const double *b_driving, double *mean, double *var, double *zone_mean_or_null, double *zone_var_or_null);

#ifdef __cplusplus
}
#endif
#endif
