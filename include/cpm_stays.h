/*
 * cpm_stays.h -- parking-stay durations per zone and hour from the fused resample of libcpm_hip.so.
 *
 * cpm_resample returns where cars are, cpm_flows.h where they go; the calls below return how long a car stays parked before it drives
 * again: the quantity a parking map is drawn for (charging windows, turnover, long-stay demand per zone), and the first thing a user
 * derives from state_matrix / transition_matrix after the OD table -- without the one-thread-per-car kernels, the C x T x 5 words on
 * the host and the loop over the hours that cpm_resample(..., state_out, trans_out) costs.
 *
 * Definition.  Hours are 0-based here: t = 0 .. T-1 is the reference's hour t+1.
 *   Arrival hour.  For car i and hour t, a(i,t) = 0 if the car drove in no hour s < t.  Otherwise it is (the last s < t with
 *     transition_matrix[i,s,1] == 1) + 1.
 *     A trip inside a zone (an all-zero p_dest row keeps the origin, src/resampling.jl:35-36) ends a stay and starts a new one in the
 *     same zone.
 *     Hour T is sampled and not applied (:81-83).  A car that drives in it has ended its stay all the same, as in cpm_flows.h.
 *   stays is int32[T][Z][T].  stays[(t*Z + z)*T + L] is the number of this context's cars with state_matrix[i,t] == z+1,
 *     transition_matrix[i,t,1] == 1 and t - a(i,t) == L.  These are the cars that drove out of (or within) zone z+1 in hour t after
 *     L whole parked hours there.
 *     Cells with L > t are zero and are written.
 *     L == t if and only if the stay began with the day, so it is left-censored.
 *   parked is int32[Z][T].  parked[z*T + a] is the number of cars with state_matrix[i,T-1] == z+1 that did not drive in hour T-1 and
 *     have a(i,T-1) == a.  These stays are still open when the day ends, so they are right-censored.
 *   Identities.  sum_L stays[t][z][L] == driving[z][t].  sum_a parked[z][a] == parking[z][T-1] - driving[z][T-1].
 *   Sharding.  Shards of a fleet add exactly.
 *   Caller's arrays.  The call writes every word, so the caller need not zero the arrays.
 *
 * Conventions are those of cpm.h: int32 status, cpm_last_error(), no abort across the boundary, no CPU fallback.
 * The library keeps one 32-bit word per car between the hours (the hour in 8 bits): T > 255 gives CPM_ERR_ARG.
 */
#ifndef CPM_STAYS_H
#define CPM_STAYS_H

#include "cpm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* resampling (src/resampling.jl:3-89) as cpm_resample returns it, plus the stays defined above.  Blocking.
 * flags as for cpm_resample (CPM_FLAG_TRAVEL may be combined); parking, driving and the travel-time sum are bit for bit those of
 * cpm_resample with the same seed and flags; the context's state is left unchanged; an overflowed step is repaired by the call
 * itself as cpm_resample does, and the stays are those of the attempt whose counts are returned.
 * stays_out: int32[T*Z*T], parked_out: int32[Z*T] (row-major as written above, NOT the column-major layout of the counts).
 * sum_travel_time_q16 may be NULL; stays_out and parked_out may not (CPM_ERR_ARG). */
int32_t cpm_resample_stays(cpm_ctx *ctx, uint64_t seed, uint32_t flags, int64_t *parking_counts, int64_t *driving_counts,
                           int64_t *sum_travel_time_q16, int32_t *stays_out, int32_t *parked_out);
/* device-resident form, enqueued on the context's stream: d_counts as for cpm_resample_dev, d_stays a DEVICE pointer to
 * int32[T*Z*T], d_parked one to int32[Z*T].  status != 0 in d_counts invalidates both arrays; the caller repeats the step. */
int32_t cpm_resample_stays_dev(cpm_ctx *ctx, uint64_t seed, uint32_t flags, void *d_counts, void *d_stays, void *d_parked);

#ifdef __cplusplus
}
#endif
#endif
