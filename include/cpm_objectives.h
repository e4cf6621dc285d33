/*
 * cpm_objectives.h -- the model-selection sweep's objectives of libcpm_hip.so, reduced on the device from a count tensor.
 *
 * The sweep (the reference notebook's three searches, README.md:947-2435) wants three scalars and a T-vector from every resample: the
 * column sums of the driving counts (traffic activity, src/saveresults.jl:23-28), the travel-time sum (src/averagedrivingtime.jl:10)
 * and the parking-density error against measured densities (README.md:2219-2244).  The counts are on the device already
 * (cpm_resample_dev, cpm_resample_batch_dev, a tensor behind an all-reduce); the calls below leave 4 + 2*T words per fleet there
 * instead of 2*T*Z + 2 for the host to reduce.
 *
 * Definition of a zone's error e_z.  Every step is ONE IEEE f64 operation, in the order written (the library is built with
 * -ffp-contract=off).  c[t] = parking[t][z], cmin / cmax its integer extremes over t, m[t] the measured density, n = n_cars:
 *   a zone is measured when the sum of its measured row, added in hour order t = 0 .. T-1, is != 0 (README.md:2236);
 *   a zone is flat when cmin == cmax; a zone is valid when it is measured and not flat;
 *   lo = (double)cmin / (double)n, hi = (double)cmax / (double)n;
 *   for t = 0 .. T-1: p = (double)c[t] / (double)n, d = (p - lo) / (hi - lo) - m[t], acc = acc + d*d;
 *   e_z = acc / (double)T.
 * parking_error = (sum of e_z over the valid zones) / (double)n_valid.  The zone sum takes no floating-point atomics; its order is
 * fixed by Z alone (not by B, the fleet's place in the batch or the run): the same tensor gives the same bits every time, and fleet b
 * of a batch gives the bits of a B = 1 call on its tensor.  Every e_z is bit for bit what the definition gives; the scalar is
 * within 2*(T + Z + 2) * 2^-53 (relative) of any other order of the same sums of non-negative terms.
 * Counts are taken to be below 2^53 (cpm_init_states admits fewer than 2^32 cars per context).
 *
 * Conventions are those of cpm.h: int32 status, cpm_last_error(), no abort across the boundary, borrowed column-major host arrays.
 */
#ifndef CPM_OBJECTIVES_H
#define CPM_OBJECTIVES_H

#include "cpm_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

/* parking_density_measured: Z x T Float64 column-major (Julia parking_density_measured[z, t]), uploaded and resident until it is
 * replaced or the context is destroyed; NULL: forget it.  A NaN or infinite entry gives CPM_ERR_ARG and leaves what was installed.
 * Needs a context only: no tables, no cars.  Blocking (the array is borrowed for the call). */
int32_t cpm_set_measured(cpm_ctx *ctx, const double *parking_density_measured);

/* enqueued on the context's stream: no synchronisation, no host read.
 * d_counts: DEVICE int64[B][2*T*Z + 2], the layout of cpm_resample_dev (B = 1) and cpm_resample_batch_dev; read only.
 * d_obj: DEVICE int64[B][4 + 2*T], one record per fleet, every word written:
 *   0            the fleet's status word, copied
 *   1            sum_tt_q16, copied
 *   2            n_valid: zones that are measured and not flat (0 when no measured data is installed)
 *   3            the bits of the f64 parking_error (NaN when n_valid == 0 or status != 0)
 *   4 .. 4+T-1   driving_sum[t] = sum over z of driving[t][z], exact
 *   4+T .. 4+2T-1  parking_sum[t] = sum over z of parking[t][z], exact
 * A fleet whose status word is set still gets words 0, 1 and 4.. from whatever its tensor holds.
 * d_zone_err_or_null: DEVICE f64[B][Z], e_z or -1.0 for a zone that is not valid; every word written.
 * n_cars: the divisor of the definition, the number of cars whose counts the tensor holds (a shard's before an all-reduce, the
 * fleet's after it).
 * CPM_ERR_ARG: NULL d_counts or d_obj, B < 1, B > CPM_MAX_BATCH, n_cars < 1. */
int32_t cpm_objectives_dev(cpm_ctx *ctx, const void *d_counts, int32_t B, int64_t n_cars, void *d_obj, void *d_zone_err_or_null);

#ifdef __cplusplus
}
#endif
#endif
