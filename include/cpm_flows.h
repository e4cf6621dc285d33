/*
 * cpm_flows.h -- hourly origin-destination (OD) trip counts from the fused resample of libcpm_hip.so.
 *
 * The reference's resampling keeps, per car and hour, whether the car drove (transition_matrix[i,t,1], src/resampling.jl:19-21),
 * where it was (state_matrix[i,t], :11) and where it went (transition_matrix[i,t,2], :47; an all-zero p_dest row keeps the origin,
 * :35-36).  cpm_resample returns what saveresults sums of that over the cars of a zone (src/saveresults.jl:8-17); the calls below
 * return in addition the same cars counted by origin AND destination: the table a user derives first from transition_matrix
 * (trip-length distributions, charging demand on arrival, the zone pairs that carry the traffic), without the one-thread-per-car
 * kernels and the C x T x 5 words on the host that cpm_resample(..., state_out, trans_out) costs.
 *
 * Conventions are those of cpm.h: int32 status, cpm_last_error(), no abort across the boundary, no CPU fallback.
 */
#ifndef CPM_FLOWS_H
#define CPM_FLOWS_H

#include "cpm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cpm_set_option: how the grouped family computes the flows.  0 (default): one launch of the OD kernel behind every hour's launches;
 * 1: the runs of all T hours are kept (as for travel times, when they fit their 24 GiB budget; otherwise as 0) and ONE launch at the
 * end of the resample reads them all.  The flows do not depend on it.  (A travel resample keeps the runs anyway, and so does a
 * context under CPM_OPT_FUSED 6 .. 8, whose one launch for all hours has no hourly boundary: both take the one-launch form.) */
#define CPM_OPT_FLOWS_KEPT 16

/* resampling (src/resampling.jl:3-89) as cpm_resample returns it, plus the OD trip counts of every hour.
 * flows: int32[T][Z][Z], hour-major, then origin, destination fastest -- flows[(t*Z + o)*Z + d] = cars of this
 * context that drove (transition_matrix[i,t,1] == 1) from zone o+1 (state_matrix[i,t]) to zone d+1
 * (transition_matrix[i,t,2]) in hour t+1.  In Julia terms an Array{Int32,3}(undef, Z, Z, T) indexed
 * [destination, origin, hour].  Trips inside a zone (an all-zero p_dest row keeps the origin, :35-36) count on the diagonal.
 * All T hours are reported: hour T is sampled and not applied (:81-83), its trips are trips all the same.
 * The call writes every word; the caller need not zero the array.
 * flags as for cpm_resample (CPM_FLAG_TRAVEL may be combined); parking, driving and the travel-time sum are bit for bit those of
 * cpm_resample with the same seed and flags; the context's state is left unchanged; an overflowed step is repaired by the call
 * itself as cpm_resample does, and the flows are those of the attempt whose counts are returned.  A cell is an int32 (a context
 * holds fewer than 2^30 cars).  Shards of a fleet add exactly.  sum_travel_time_q16 may be NULL; flows_out may not (CPM_ERR_ARG). */
int32_t cpm_resample_flows(cpm_ctx *ctx, uint64_t seed, uint32_t flags, int64_t *parking_counts, int64_t *driving_counts,
                           int64_t *sum_travel_time_q16, int32_t *flows_out);
/* device-resident form: d_counts as for cpm_resample_dev, d_flows a DEVICE pointer to int32[T*Z*Z].
 * status != 0 in d_counts invalidates d_flows as well; the caller repeats the step. */
int32_t cpm_resample_flows_dev(cpm_ctx *ctx, uint64_t seed, uint32_t flags, void *d_counts, void *d_flows);

#ifdef __cplusplus
}
#endif
#endif
