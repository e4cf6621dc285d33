/*
 * cpm_expected.h -- expected parking and driving densities of libcpm_hip.so: the mean of the sampler's Markov chain, propagated on
 * the device without a car or a random number.
 *
 * Every other output of the library is a Monte-Carlo sample of C cars.  The model they sample is a time-inhomogeneous Markov chain;
 * its mean, the limit C -> infinity, is pi_{t+1} = pi_t * M_t (the reference's "joint origin-destination probability",
 * README.md:452-468).  The calls below evaluate that recurrence for THIS sampler's law -- rows are not renormalised, and a draw above
 * a row total below 1 goes to the row's last zone with p > 0 -- from the installed tables.
 *
 * Definition.  For hour t with the installed pdrive[t][.], p[t][.][.] (p[t][d][o] = p_destin[o, d, t]) and last[t][o], the f64
 * left-to-right total of row o that the device keeps.  Every step is ONE IEEE f64 operation (the library is built with
 * -ffp-contract=off):
 *   q[o]   = p_drive[o, t] as the sampler's Bernoulli maps it: NaN and values < 0 become 0, values >= 1 become 1;
 *   x[o]   = pi[o] * q[o],  s[o] = pi[o] * (1 - q[o]);
 *   a zero row (last == 0): x[o] goes to o itself (it is still "driving", src/resampling.jl:35-36);
 *   otherwise x[o] * p[o, d] goes to every d, and the residual x[o] * r[o] to l[o], where r[o] = max(0, 1 - last) and l[o] is the
 *   last destination with p > 0;
 *   a non-zero row whose total exceeds 1 by more than Z * 2^-52 is not the sampler's law under this rule: CPM_ERR_TABLE, and
 *   cpm_last_error() names the hour and the origin (1-based);
 *   pi_{t+1}[d] = ((s[d] + y[d]) + res[d]) (+ x[d] for a zero row), y[d] = the sum over o of x[o] * p[o, d], res[d] = the sum of
 *   the residuals that arrive at d.
 * Outputs: parking[t][z] = pi_t[z] and driving[t][z] = pi_t[z] * q[z], t = 0 .. T-1.  With C cars, C * parking and C * driving are
 * the expected counts of cpm_resample.
 *
 * The sums take no floating-point atomics.  Their order is a function of Z and the installed table alone -- not of B, a fleet's
 * place in the batch or the run: the same inputs give the same bits every time, and fleet b of a batch gives the bits of a B = 1
 * call with its p_drive installed.  All terms are non-negative: after h operators a word lies within h * (Z + 8) * 2^-52
 * (relative) of the exact value, and a word whose exact value is 0 is 0.
 *
 * CPM_EXPECT_IVP: the operators of hours 0 .. T-2 are applied to pi_0 first and the day starts from the result -- the expected
 * form of cpm_solve_ivp (src/solveinitialvalueproblem.jl:8-57).
 *
 * The calls need no cars and change no state of the context that a later resample reads.  The first call after the p_destin tables
 * changed builds l, r and the residual lists and reads the row-total check back: that call synchronises the stream once.
 * Tables with sparse row packs are expanded to the dense array first (as cpm_get_cdf_row does).
 *
 * Conventions are those of cpm.h: int32 status, cpm_last_error(), no abort across the boundary, borrowed column-major host arrays.
 * Without a usable device every entry returns CPM_ERR_HIP.
 */
#ifndef CPM_EXPECTED_H
#define CPM_EXPECTED_H

#include "cpm_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CPM_EXPECT_IVP 1u /* flags: start the day from pi_0 carried through hours 0 .. T-2 */

/* enqueued on the context's stream.
 * d_pi0_or_null: DEVICE f64[Z]; NULL: uniform 1 / Z, the reference's initial placement.  Read only.
 * d_out: DEVICE f64[2][T][Z], parking then driving; every word written.
 * d_pi_next_or_null: DEVICE f64[Z], pi after the day's last operator (the next day's pi_0).
 * CPM_ERR_STATE without p_drive or p_destin tables; CPM_ERR_ARG: NULL d_out, unknown flag bits. */
int32_t cpm_expected_dev(cpm_ctx *ctx, const void *d_pi0_or_null, uint32_t flags, void *d_out, void *d_pi_next_or_null);

/* the same for the B fleets of the installed batch tables (cpm_set_p_drive_batch / cpm_build_p_drive_batch), in one pass over p
 * per hour and eight fleets; all fleets start from the same pi_0.  d_out: DEVICE f64[B][2][T][Z].
 * CPM_ERR_STATE also without batch tables. */
int32_t cpm_expected_batch_dev(cpm_ctx *ctx, const void *d_pi0_or_null, uint32_t flags, void *d_out);

/* blocking.  pi0_or_null: borrowed host f64[Z] (CPM_ERR_ARG for a NaN, infinite or negative entry) or NULL.
 * parking_density / driving_density: Z x T Float64 column-major, the layout of cpm_resample's count arrays.
 * pi_next_or_null: host f64[Z]. */
int32_t cpm_expected(cpm_ctx *ctx, const double *pi0_or_null, uint32_t flags, double *parking_density, double *driving_density,
                     double *pi_next_or_null);
/* parking_density / driving_density: Z x T x B Float64 column-major, the layout of cpm_resample_batch's count arrays */
int32_t cpm_expected_batch(cpm_ctx *ctx, const double *pi0_or_null, uint32_t flags, double *parking_density, double *driving_density);

#ifdef __cplusplus
}
#endif
#endif
