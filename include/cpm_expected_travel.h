/*
 * cpm_expected_travel.h -- expected travel time and driven distance per zone and hour of libcpm_hip.so, and with them the noise-free
 * A_drive: the mean of what cpm_resample with CPM_FLAG_TRAVEL samples, without a car or a random number.
 *
 * The travel-time draw of one trip (csrc/cpm_rng.h, truncnormal_draw) is one inversion that is symmetric about the cell's mean,
 * x = mu + sigma * ppnd((u - 1/2) * E) inside the symmetric window [0.9 mu, 1.1 mu], and it is mu itself where sigma or E is not
 * positive: its expectation is the mean word of the cell, whatever the standard deviation.  (The 2^-54 offset of the u = k * 2^-53
 * grid from symmetry is not part of the definition.)  The expected seconds and kilometres of ONE trip that starts in zone o in hour t
 * are therefore a property of the installed tables alone -- p_destin, the datamatrix and the distance matrix, not p_drive, pi or the
 * fleet.
 *
 * Definition.  Terms are those of cpm_expected.h: p[t][d][o] = p_destin[o, d, t], last[t][o], l[t][o], r[t][o] = max(0, 1 - last).
 * Every step is ONE IEEE f64 operation (the library is built with -ffp-contract=off):
 *   sec(o, d, t) = 300.0 if d == o, else datamatrix[o, d, t, 1] (the mean word, as it is)
 *   km(o, d)     = 1.0   if d == o, else distance_matrix_km[o, d]
 *   a zero row (last == 0): w_sec[t][o] = 300.0, w_km[t][o] = 1.0 (the driver stays in o, src/resampling.jl:35-36, :58-60)
 *   otherwise:              w_sec[t][o] = (the sum over d of p[o, d] * sec(o, d, t)) + r[o] * sec(o, l[o], t), w_km likewise with km
 * The trip weights w[2][T][Z] hold w_sec, then w_km.  Per fleet, with the driving density x_t[o] (the second half of cpm_expected*'s
 * tensor):
 *   seconds[t][o] = x_t[o] * w_sec[t][o],  km[t][o] = x_t[o] * w_km[t][o],  totals = (the sum of seconds, the sum of km) over all t, o.
 * With C cars, C * seconds[t][o] is the expected sum of transition_matrix[i, t, 3] over the cars that leave o in hour t, and
 *   A_drive = totals[0] / (T * 3600)
 * is src/averagedrivingtime.jl:10 with sum / C taken to its mean.  All T hours count, hour T included: it is sampled and its trips are
 * summed, though its state is never applied.
 *
 * The result is the sampler's expectation for finite means; negative or non-finite means are passed through as they are (the draw
 * returns mu for mu < 0 too).
 *
 * Order of the sums (no floating-point atomics; csrc/cpm_expected_travel.h): the destinations are cut into S consecutive segments of
 * ceil(Z / S), S = max(1, min(8, ceil(Z / 64), ceil(1024 / (ceil(Z / 128) * T)))); within a segment destination d belongs to chain
 * (d - begin) mod 4, a chain adds its products in ascending d starting from 0, the four chains are added in order, then the segments
 * in order, then the residual term.  The totals: [T][Z] is cut into chunks of 1,024 consecutive words; chain i of a chunk's 256 adds
 * its words i, i + 256, i + 512, i + 768 in that order, the chains of a wave go through the fixed shuffle tree, the four waves are
 * added in order; then chain l of 64 adds the chunks l, l + 64, ... in ascending order and the 64 chains go through the same tree.
 * The order is a function of Z, T and the installed tables -- not of B, a fleet's place in the batch or the run: the same inputs
 * give the same bits every time, and fleet b of a batch gives the bits of a B = 1 call.
 *
 * Error bound, for tables whose means and distances are non-negative (all terms are then non-negative).  A term of a weight passes
 * one multiplication, at most ceil(Z / 4) additions of its chain, 3 of the chains, S - 1 <= 7 of the segments and 1 of the residual
 * term: at most Z / 4 + 14 roundings of 2^-53 each.  A weight lies within
 *   (Z / 4 + 16) * 2^-52                                      (relative, twice the derived count)
 * of its exact value; seconds and km of a fleet within the bound of the driving density (cpm_expected.h: max(h * (Z + 8), 1) * 2^-52
 * after h operators) plus (Z / 4 + 17) * 2^-52; a total (at most 3 + 9 + ceil(T * Z / 65,536) + 6 additions behind a word) within
 * the largest bound of its words plus (T * Z / 65,536 + 20) * 2^-52.  A word whose exact value is 0 is 0.
 *
 * The weights are cached in the context: built on first use and again on first use after the p_destin tables, the datamatrix or the
 * distance matrix changed (cpm_set_p_dest, cpm_build_p_dest, cpm_synth_tables*, cpm_refresh_tables; cpm_set_datamatrix,
 * cpm_createdatamatrix_*, cpm_synth_datamatrix; cpm_set_distance*).  p_drive does not enter.  Tables with sparse row packs are expanded
 * to the dense array first, as for the densities.
 *
 * The calls need no cars and change no state of the context that a later resample reads.  Status codes: CPM_ERR_STATE without
 * p_destin tables, a datamatrix or a distance matrix (cpm_last_error() names which); CPM_ERR_TABLE for a row total above 1, exactly as
 * for the densities.  Conventions are those of cpm.h: int32 status, cpm_last_error(), no abort across the boundary, borrowed
 * column-major host arrays.  Without a usable device every entry returns CPM_ERR_HIP.
 */
#ifndef CPM_EXPECTED_TRAVEL_H
#define CPM_EXPECTED_TRAVEL_H

#include "cpm_expected.h"

#ifdef __cplusplus
extern "C" {
#endif

/* enqueued on the context's stream (the first call after a table change synchronises once, as cpm_expected_dev does).
 * d_w: DEVICE f64[2][T][Z], w_sec then w_km; every word written.  CPM_ERR_ARG: NULL d_w. */
int32_t cpm_expected_trip_dev(cpm_ctx *ctx, void *d_w);

/* blocking.  w_sec / w_km: Z x T Float64 column-major host arrays. */
int32_t cpm_expected_trip(cpm_ctx *ctx, double *w_sec, double *w_km);

/* enqueued on the context's stream.
 * d_expected: DEVICE f64[B][2][T][Z] as cpm_expected_dev / cpm_expected_batch_dev wrote it; only the driving halves are read (any
 *   driving density will do, e.g. sampled counts / C).
 * d_travel: DEVICE f64[B][2][T][Z], seconds then km; every word written.  May be NULL.
 * d_totals: DEVICE f64[B][2], (sum of seconds, sum of km).  May be NULL.
 * CPM_ERR_ARG: NULL d_expected, B < 1, both outputs NULL. */
int32_t cpm_expected_travel_dev(cpm_ctx *ctx, const void *d_expected, int32_t B, void *d_travel, void *d_totals);

/* blocking: the propagation of cpm_expected (its densities bit for bit) and the product in one call.
 * pi0_or_null, flags: as for cpm_expected (CPM_EXPECT_IVP).  seconds / km: Z x T Float64 column-major.  totals: host f64[2]. */
int32_t cpm_expected_travel(cpm_ctx *ctx, const double *pi0_or_null, uint32_t flags, double *seconds, double *km, double *totals);
/* the same for the B fleets of the installed batch tables.  seconds / km: Z x T x B column-major; totals: host f64[B][2]. */
int32_t cpm_expected_travel_batch(cpm_ctx *ctx, const double *pi0_or_null, uint32_t flags, double *seconds, double *km, double *totals);

/* how often this context has built the trip weights (tests and tools see the cache through it); negative: a status code */
int64_t cpm_expected_trip_builds(const cpm_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif
