/*
 * cpm_paths.h -- per-car day records from the fused resample of libcpm_hip.so, resident on the device.
 *
 * The reference's resampling (src/resampling.jl:3-89) returns state_matrix (where every car is at every hour) and
 * transition_matrix[:, :, 1:2] (whether it drove, and where to); everything downstream is a function of the two.  cpm_resample returns
 * them through the one-thread-per-car kernels, a synchronisation per hour and 40 bytes per car-hour on the host.  The calls below
 * return the same information as ONE 32-bit word per car-hour, from whatever kernel family produces the counts, and can leave it on
 * the device: flows, stays, trips per car, tours or the reference's own matrices are derived from it there.
 *
 * Definition.  Hours are 0-based here: t = 0 .. T-1 is the reference's hour t+1.  n is the context's car count; local car i is global
 * car first + i*stride, as everywhere else.
 *   paths is uint32[T][n], hour-major, the car index fastest:
 *     paths[t*n + i] = (transition_matrix[i,t,2] - 1) | (transition_matrix[i,t,1] == 1 ? 0x80000000 : 0)
 *   A car that did not drive carries its own zone, without the bit (:19).
 *   An all-zero p_dest row gives the origin with the bit set (:35-36).
 *   Hour T-1 holds what was sampled although it is never applied (:81-83), as cpm_flows.h and cpm_stays.h treat it.
 *   state_matrix[i,0] is the context's current state, and state_matrix[i,t+1] - 1 == paths[t*n + i] & 0x7fffffff.
 *   Sharding.  Shards of a fleet are disjoint row sets of the whole fleet's record.
 *   Caller's array.  The call writes every word, so the caller need not zero the array.
 *
 * Conventions are those of cpm.h: int32 status, cpm_last_error(), no abort across the boundary, no CPU fallback.
 */
#ifndef CPM_PATHS_H
#define CPM_PATHS_H

#include "cpm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* resampling as cpm_resample returns it, plus the record defined above.  Blocking.
 * flags as for cpm_resample (CPM_FLAG_TRAVEL may be combined); parking, driving and the travel-time sum are bit for bit those of
 * cpm_resample with the same seed and flags; the context's state is left unchanged; an overflowed step is repaired by the call
 * itself as cpm_resample does, and the record is that of the attempt whose counts are returned.
 * paths_out: host uint32[T*n].  sum_travel_time_q16 may be NULL; paths_out may not (CPM_ERR_ARG). */
int32_t cpm_resample_paths(cpm_ctx *ctx, uint64_t seed, uint32_t flags, int64_t *parking_counts, int64_t *driving_counts,
                           int64_t *sum_travel_time_q16, uint32_t *paths_out);
/* device-resident form, enqueued on the context's stream: d_counts as for cpm_resample_dev, d_paths a DEVICE pointer to uint32[T*n].
 * status != 0 in d_counts invalidates the record; the caller repeats the step.  Even then nothing is stored outside
 * [d_paths, d_paths + T*n).  A NULL pointer gives CPM_ERR_ARG.  d_paths must be 4-byte aligned (any device allocation is); the
 * kernels index a row with 32 bits, as everything per car does: n < 2^32 (cpm_init_states admits no more cars in one context). */
int32_t cpm_resample_paths_dev(cpm_ctx *ctx, uint64_t seed, uint32_t flags, void *d_counts, void *d_paths);
/* the reference's matrices ON THE DEVICE from a record, enqueued on the context's stream without a synchronisation:
 * d_state: DEVICE int64[T][n] (= state_matrix, C x T column-major, 1-based zones), or NULL;
 * d_trans: DEVICE f64[4][T][n] (= transition_matrix, C x T x 4 column-major), or NULL.
 * Both are bit-equal to what cpm_resample(..., state_out, trans_out) returns for the same seed, flags and context state.  Columns 3
 * and 4 (travel time, distance) are zero without CPM_FLAG_TRAVEL and otherwise re-derived from Philox streams 1 and 2.
 * The context's state and the seed MUST be those of the step that produced the record: hour 0's origins are read from the
 * context's state, and the travel columns are drawn from the seed.  d_paths may not be NULL (CPM_ERR_ARG). */
int32_t cpm_paths_expand_dev(cpm_ctx *ctx, uint64_t seed, uint32_t flags, const void *d_paths, void *d_state, void *d_trans);

#ifdef __cplusplus
}
#endif
#endif
