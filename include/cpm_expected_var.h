/*
 * cpm_expected_var.h -- exact variances of a resample's counts of libcpm_hip.so, from the day's transition matrix, computed on the
 * device without a car or a random number.
 *
 * cpm_expected.h gives the mean of the sampler's Markov chain.  A comparison of a sampled count with that mean needs a width; the
 * binomial sqrt(C * pi * (1 - pi)) is only an upper bound.  Cars start in known zones and move independently, so a count is a
 * Poisson-binomial sum, and its exact variance follows from the t-step transition matrix.
 *
 * Definition.  q, r, l, the zero-row rule, the law and the row-total refusal (CPM_ERR_TABLE) are exactly those of cpm_expected.h.
 * M_t[o][d] is the probability that a car in o at hour t is in d at hour t + 1 under that law:
 *   q[o] * p[o, d] for every d,
 *   plus q[o] * r[o] at d = l[o],
 *   plus 1 - q[o] at d = o;
 *   for a zero row (last == 0) all of q[o] goes to d = o: M_t[o][o] = 1 and the rest of the row is 0.
 * As computed: ((p * q) + q * r) + (1 - q), every step one IEEE f64 operation, a term that does not apply left out.
 * P_0 = I; with CPM_EXPECT_IVP, P_0 = M_0 ... M_{T-2}.  In both cases P_{t+1} = P_t * M_t.
 * With w[s] the number of cars that start in zone s, for t = 0 .. T-1 and zone z:
 *   mean_parking[t][z] = sum over s of w[s] * P_t[s, z]
 *   mean_driving[t][z] = sum over s of w[s] * a,             a = P_t[s, z] * q_t[z]
 *   var_parking[t][z]  = sum over s of w[s] * (P * (1 - P))
 *   var_driving[t][z]  = sum over s of w[s] * (a * (1 - a))
 * (1 - P and 1 - a, whose exact values are not negative, are clamped at 0.)
 *
 * What the numbers are.  var_parking and var_driving are the variances of cpm_resample's counts parking[t][z] and driving[t][z]
 * over the seed, GIVEN the start zones of the cars (w = the cars per zone of cpm_init_states, or the histogram of cpm_get_state).
 * With CPM_EXPECT_IVP they are the variances over the seed of cpm_solve_ivp followed by cpm_resample, given the placement in front
 * of the IVP.  Covariances between zones are not given; the total over zones is C in every run: its variance is 0.  The outputs
 * are linear in w.
 *
 * Numerics.  No floating-point atomics.  The order of every sum is a function of Z and the installed tables alone: the same inputs
 * give the same bits every time.  The product runs on the f64 matrix instruction, which fuses its multiply-add: the contract with
 * the exact value is a bound, not bits.  All terms are non-negative, so, with u = 2^-52:
 *   a word of M_t is a sum of terms that are each rounded once (p * q, q * r, 1 - q) and pass at most two rounded sums: within 4u (relative);
 *   a word of P * M_t is a chain of Z fused multiply-adds of non-negative terms: within Z * u of the exact product of its operands;
 *   so after h operators a word of P lies within h * (Z + 8) * u (relative) of the exact value, as the words of cpm_expected.h do.
 *   A mean word adds Z + 2 roundings of non-negative terms to that: within E = (h + 1) * (Z + 8) * u (relative), where h = t, or
 *   T - 1 + t with CPM_EXPECT_IVP.
 *   A variance word has NO relative bound: 1 - P cancels when P is close to 1 (a car that stays put with probability 1 - 1e-17 has
 *   an exact variance of 1e-17 and a computed one of 0).  Its bound is absolute, in units of the MEAN word of the same cell: an error
 *   delta <= e * P of P moves P * (1 - P) by at most delta * |1 - 2P| + delta^2 <= e * P * (1 + e), the three roundings of
 *   w * (P * (1 - P)) and the sum's add at most (Z + 3) * u * P * w more, and the sum over s of w * P is the mean: a variance word
 *   lies within E * mean_parking[t][z] (var_driving: E * mean_driving[t][z]) of its exact value.
 *   A word whose exact value is 0 is 0.
 *
 * Workspace: two Z x Z f64 matrices (all start rows at once: p is read once per hour) and ceil(Z / 64) x 4 x Z partial sums, owned
 * by the context and allocated on first use; a failed allocation returns CPM_ERR_NOMEM with the bytes asked for in
 * cpm_last_error().  Tables with sparse row packs are expanded to the dense array first, as cpm_expected does.  The calls need no
 * cars and change no state of the context that a later call reads.  The first call after the p_destin tables changed synchronises
 * the stream once (cpm_expected.h).
 *
 * Conventions are those of cpm.h: int32 status, cpm_last_error(), no abort across the boundary, borrowed column-major host arrays.
 * Without a usable device every entry returns CPM_ERR_HIP.
 */
#ifndef CPM_EXPECTED_VAR_H
#define CPM_EXPECTED_VAR_H

#include "cpm_expected.h"

#ifdef __cplusplus
extern "C" {
#endif

/* enqueued on the context's stream.
 * d_start_or_null: DEVICE f64[Z] holding w; NULL: 1 per zone.  Read only.
 * flags: CPM_EXPECT_IVP or 0.
 * d_out: DEVICE f64[4][T][Z]: mean_parking, mean_driving, var_parking, var_driving; every word written.
 * CPM_ERR_STATE without p_drive or p_destin tables; CPM_ERR_ARG: NULL d_out, unknown flag bits. */
int32_t cpm_expected_var_dev(cpm_ctx *ctx, const void *d_start_or_null, uint32_t flags, void *d_out);

/* blocking.  start_or_null: borrowed host f64[Z] (CPM_ERR_ARG for a NaN, infinite or negative entry) or NULL.
 * mean_parking / mean_driving / var_parking / var_driving: Z x T Float64 column-major, the layout of cpm_resample's count arrays;
 * any of them may be NULL. */
int32_t cpm_expected_var(cpm_ctx *ctx, const double *start_or_null, uint32_t flags, double *mean_parking, double *mean_driving,
                         double *var_parking, double *var_driving);

#ifdef __cplusplus
}
#endif
#endif
