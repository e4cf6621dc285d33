/*
 * cpm_expected_travel_var.h -- the exact mean and seed variance of travel seconds, driven kilometres, A_drive and any linear
 * functional of a resample's counts together with them, of libcpm_hip.so: one backward pass over the installed p_destin tables, the
 * mean plane of the datamatrix and the distance matrix, without a car or a random number.
 *
 * cpm_expected_linear_var.h covers the functionals that are linear in the counts.  The travel sum of cpm_resample with
 * CPM_FLAG_TRAVEL is not one of them: it is a reward on the trips (origin -> destination, hour), with two sources of noise the counts
 * do not have -- which destination the car picks, and the truncated-normal draw of the trip's seconds -- and it is correlated with
 * where the car is afterwards.  All three fit the backward recurrence of cpm_expected_linear_var.h with an edge reward in the
 * centred sums and one more weight that is a property of the tables alone.
 *
 * Definition.  Terms are those of cpm_expected_linear_var.h and cpm_expected_travel.h: q, p[t][d][o] = p_destin[o, d, t], last, l, r,
 * zero rows, the row-total refusal; the operators s = 0 .. N-1, pre, t(s), j = s - pre, CPM_EXPECT_IVP; sec(o, d, t) and km(o, d) with
 * the diagonal select 300 s / 1 km.
 *
 * Variance of one trip's seconds, var_sec(o, d, t).  0 for d == o.  Otherwise, with mu = the mean word and sd = the std word of the
 * cell, sd = 0.1 * mu where the std word is == 0 (travel_time_q16 in csrc/cpm_kernels.h): 0 where !(sd > 0), and 0 where the mass
 * E = truncnormal_mass(mu, sd) = det_erf(a * sqrt(1/2)), a = (0.1 * mu) / sd, is not > 0 (the draw returns mu in both cases);
 * otherwise
 *   var_sec = (sd * v(a)) * sd,     v(a) = 1 - 2 a phi(a) / erf(a / sqrt 2),  phi(a) = exp(-a^2 / 2) / sqrt(2 pi),
 * the variance of a standard normal truncated to +-a, times sd^2.  v is evaluated from the f64 word a with the f64 kit of
 * csrc/cpm_rng.h (det_erf, exp_neg: +, -, *, / only, no libm), so the word is the same on every device and in the tests' restatement:
 *   a > 1:   v = 1 - ((a * 0.79788456080286535588) * exp_neg(y)) / E,      y = (a * a) * 0.5;
 *   a <= 1:  the closed form cancels (v -> a^2 / 3); with N(y) = sum (-y)^m / ((2 m + 3) m!) and M(y) = sum (-y)^m / ((2 m + 1) m!),
 *            exp(-y) = M - 2 y N and erf(a / sqrt 2) = a sqrt(2 / pi) M, so v = ((2 y) * N) / M: both sums for m = 0 .. 17 by
 *            Horner from m = 17 down, x = -y, the coefficient of m the f64 quotient 1.0 / ((2 m + 3) * m!) (the product and the
 *            quotient rounded once each).
 * Bound of v.  a <= 1, y <= 1/2: the terms alternate and fall, N >= 1/3 - y/5 >= 0.23 and the sum of the terms' magnitudes is at most
 * 0.45 (M: 0.85 and 1.18), so a Horner evaluation of 18 terms with rounded coefficients is within 2 * 18 * 2 * 2^-53 of N and within
 * 2 * 18 * 1.4 * 2^-53 of M; the truncation (m = 18: below 2^-74) does not show; y, 2 y N and the quotient add 4 roundings:
 * (72 + 51 + 4) * 2^-53 < 2^-46.  a > 1: g = 2 a phi / E <= 0.709 carries the error of exp_neg (within 2^-50 on y <= 745, tests/
 * test_travel_kit.py), of det_erf (Cody's rational forms: within 2^-50) and 5 roundings, and 1 - g >= 0.29 enlarges them by
 * g / (1 - g) <= 2.44: 2.44 * (8 + 8 + 5) * 2^-53 + 2^-53 < 2^-47.  So
 *   |v - exact v(a)| <= 2^-46 * v(a)      (a the f64 word), and var_sec within 2^-46 + 2^-52 of sd^2 v(a), relative.
 * Not part of the definition: the q16 rounding of each trip's seconds (2^-32 / 12 s^2 per trip), the 2^-53-probability clamp cases
 * of ppnd_tail (u = 0 with a mass of exactly 1.0), and the 2^-54 offset of the u = k * 2^-53 grid from symmetry.
 *
 * Trip variance weight, a property of the tables alone:
 *   v_sec[t][o] = (the sum over d of p[o, d] * var_sec(o, d, t)) + r[o] * var_sec(o, l[o], t);       0 for a zero row.
 * Order of the sums: that of the trip weights (cpm_expected_travel.h): trip_segments, the four chains (d - begin) mod 4 in ascending
 * d from 0, the chains in order, the segments ascending, the residual term last.  Every term is non-negative: a word lies within
 * (Z / 4 + 16) * 2^-52 + 2^-45 (relative) of the exact sum of p * sd^2 v(a); a word whose exact value is 0 is 0.  The weights are
 * cached in the context: built on first use and again on first use after anything that rebuilds the trip weights (cpm_expected_travel.h
 * lists the calls); cpm_expected_trip_var_builds counts the builds.  Building them builds the trip weights where those are stale.
 *
 * Functional k of K has four coefficient arrays A_k, B_k, S_k, D_k, each [T][Z]:
 *   L_k = the sum over t, z of A_k[t][z] * parking[t][z] + B_k[t][z] * driving[t][z]
 *       + the sum over the trips that leave o in hour t of (S_k[t][o] * the seconds of the trip + D_k[t][o] * km(o, d)).
 * All T hours' trips count, hour T included, as in cpm_expected_travel.h.  S = 1, A = B = D = 0 is the travel-time sum of
 * cpm_resample (sum_travel_time_q16 / 65536); divided by C * T * 3600 it is A_drive.
 *   mean_k = the sum over s of w[s] * V_0[s],     var_k = the sum over s of w[s] * W_0[s],      w as in cpm_expected_linear_var.h.
 *
 * Backward pass.  Every step is ONE IEEE f64 operation (the library is built with -ffp-contract=off).  mu = nu = 0; for s = N-1 down
 * to 0, with t = t(s), gp = A_k[j], gd = B_k[j], S = S_k[j], D = D_k[j] (all 0 for j < 0, an operator in front of the day), for
 * origin o:
 *   e[d]    = S[o] * sec(o, d, t) + D[o] * km(o, d)
 *   zeta[d] = (mu[d] - mu[o]) + e[d]
 *   s1 = (the sum over d of p[o, d] * zeta[d])             + r[o] * zeta[l[o]]
 *   s2 = (the sum over d of (p[o, d] * zeta[d]) * zeta[d]) + (r[o] * zeta[l[o]]) * zeta[l[o]]
 *   b  = (the sum over d of p[o, d] * nu[d])               + r[o] * nu[l[o]]          (the second terms only where l[o] exists);
 *   a zero row is a trip inside the zone: zeta = S[o] * 300 + D[o] * 1, s1 = zeta, s2 = zeta * zeta, b = nu[o];
 *   db = gd[o] + s1;
 *   J  = q * (((1 - q) * (db * db) + max(0, s2 - s1 * s1)) + (S[o] * S[o]) * v_sec[t][o]);
 *   V[o] = (gp[o] + mu[o]) + q * db;
 *   W[o] = ((1 - q) * nu[o] + q * b) + J;
 *   mu <- V, nu <- W.
 * The last operator (hour T-1) has mu = nu = 0 and forms its product like every other: zeta = e there.
 *
 * Order of the sums: that of cpm_expected_linear_var.h (grad_segments, chains (d - begin) mod 4, the segments ascending, the
 * residual term; the 256-chain totals).  Contract:
 *   - functional k of a call with K functionals carries the bits of a K = 1 call on it;
 *   - the same inputs give the same bits every time;
 *   - with finite means and distances and S = D = 0, every output word is bit for bit that of cpm_expected_linear_var[_dev]
 *     (e = 0 * sec + 0 * km = 0, zeta = eta + 0, and (0 * 0) * v_sec = 0 is added to a sum it does not change);
 *   - a functional that is constant over the zones of every hour with S = D = 0 still gives a variance of exactly 0.
 *
 * Error bound, relative to the magnitude recurrence of non-negative terms: that of cpm_expected_linear_var.h with |gp|, |gd|, |S|,
 * |D|, |sec|, |km| in place of the signed words, e~ = |S| |sec| + |D| |km|,
 *   eta~[d] = (mu~[d] + mu~[o]) + e~[d];   s1~ = sum p * eta~ + r * eta~[l];  s2~ = sum p * eta~^2 + r * eta~[l]^2;  b~ as before
 *   (a zero row: s1~ = e~, s2~ = e~^2, b~ = nu~[o]);
 *   db~ = |gd| + s1~;  J~ = q * (((1 - q) * db~^2 + (s2~ + s1~^2)) + S^2 * v_sec);  V~ = |gp| + mu~[o] + q * db~;
 *   W~ = (1 - q) * nu~[o] + q * b~ + J~.
 * A product p * zeta passes what p * eta passes in cpm_expected_linear_var.h and, in front of it, the two products and the sum
 * that form e (two roundings relative to e~) and the addition that forms zeta (one): R' = R + 3 =
 * ceil(ceil(Z / S) / 4) + S + 15 roundings of 2^-53, K' = 2 * R'.  After n backward operators
 *   a word of V lies within n * K' * 2^-52 * V~ of its exact value,
 *   a word of W lies within (2 * n * K' * 2^-52 + B_v) * W~,   B_v = (Z / 4 + 16) * 2^-52 + 2^-45 + 3 * 2^-53,
 * the second term for S^2 * v_sec, which enters J with v_sec's own bound (above), two roundings of its products and one of its sum,
 * and is carried through the non-negative recurrence of nu unamplified.  The totals:
 *   |mean_k - exact| <= (N * K' + Z + 2) * 2^-52 * the sum of w * V~_0,
 *   |var_k - exact|  <= ((2 * N * K' + Z + 2) * 2^-52 + B_v) * the sum of w * W~_0.
 * The exact value is that of the recurrence with the exact v(a) of every cell's f64 word a.  A word whose magnitude is 0 is 0.
 *
 * The calls need no cars, run no forward propagation, keep no Z x Z workspace and change no state of the context that a later call
 * reads.  Tables with sparse row packs are expanded to the dense array first, as cpm_expected_linear_var does; the sparse twins,
 * which read the compact rows instead, are in cpm_expected_sparse_var.h.  The first call after the tables changed synchronises the stream once (cpm_expected.h).
 *
 * Status codes are those of cpm_expected_linear_var (CPM_ERR_STATE without p_drive or p_destin tables, CPM_ERR_TABLE, CPM_ERR_HIP,
 * CPM_ERR_NOMEM, CPM_ERR_ARG for a NULL coefficient or output array, unknown flag bits, K outside 1 .. CPM_MAX_BATCH and, in the
 * blocking form, a coefficient that is not finite or a start entry that is NaN, infinite or negative), and CPM_ERR_STATE without a
 * datamatrix or a distance matrix, as in cpm_expected_travel (cpm_last_error() names which).  Conventions are those of cpm.h.
 */
#ifndef CPM_EXPECTED_TRAVEL_VAR_H
#define CPM_EXPECTED_TRAVEL_VAR_H

#include "cpm_expected.h"

#ifdef __cplusplus
extern "C" {
#endif

/* enqueued on the context's stream.  d_v: DEVICE f64[T][Z], v_sec; every word written.  CPM_ERR_ARG: NULL d_v. */
int32_t cpm_expected_trip_var_dev(cpm_ctx *ctx, void *d_v);

/* blocking.  v_sec: Z x T Float64 column-major host array. */
int32_t cpm_expected_trip_var(cpm_ctx *ctx, double *v_sec);

/* how often this context has built the trip variance weights; negative: a status code */
int64_t cpm_expected_trip_var_builds(const cpm_ctx *ctx);

/* enqueued on the context's stream.
 * d_start_or_null: DEVICE f64[Z] holding w; NULL: 1 per zone.  Read only.  flags: CPM_EXPECT_IVP or 0.
 * K: the number of functionals, 1 .. CPM_MAX_BATCH.
 * d_coeff: DEVICE f64[K][4][T][Z]: A_k, B_k, S_k, D_k.  Read only.
 * d_out: DEVICE f64[K][2], mean then variance; every word written.
 * d_zone_or_null: DEVICE f64[K][2][Z], V_0 and W_0 per start zone; every word written.  NULL: not wanted.
 * Nothing outside the two outputs is written. */
int32_t cpm_expected_travel_var_dev(cpm_ctx *ctx, const void *d_start_or_null, uint32_t flags, int32_t K, const void *d_coeff, void *d_out,
                                    void *d_zone_or_null);

/* blocking.  start_or_null: borrowed host f64[Z] or NULL.
 * a_parking / b_driving / s_seconds_or_null / d_km_or_null: Z x T x K Float64 column-major; a NULL trip array means zeros.
 * mean / var: host f64[K].  zone_mean_or_null / zone_var_or_null: Z x K Float64 column-major, V_0 and W_0. */
int32_t cpm_expected_travel_var(cpm_ctx *ctx, const double *start_or_null, uint32_t flags, int32_t K, const double *a_parking,
                                const double *b_driving, const double *s_seconds_or_null, const double *d_km_or_null, double *mean, double *var,
                                double *zone_mean_or_null, double *zone_var_or_null);

#ifdef __cplusplus
}
#endif
#endif
