/*
 * cpm_batch.h -- batched resample of libcpm_hip.so: B fleets in one pass over the row packs.
 *
 * A batch is B fleets.  Each fleet has its own p_drive table and seed; all fleets share the context's installed p_destin
 * tables, its current car state (normally the post-IVP state) and, with CPM_FLAG_TRAVEL, its travel tables.  The model-selection
 * sweep's points that share e_dest differ only in p_drive: one batch runs several of them while every row pack is staged into
 * LDS once per hour and origin zone for all of them.
 *
 * Contract: fleet b's parking counts, driving counts and travel-time sum are bit for bit what cpm_resample(ctx, seeds[b], flags,
 * ...) returns from the same state with fleet b's p_drive installed, for every B, table kind, flag and fallback.  The RNG contract
 * of cpm.h is unchanged (Philox keyed by the fleet's seed, counter = (global car, step, stream)): fleets that share a seed draw
 * common random numbers.
 *
 * Conventions are those of cpm.h: int32 status, cpm_last_error(), no abort across the boundary, borrowed column-major host arrays.
 */
#ifndef CPM_BATCH_H
#define CPM_BATCH_H

#include "cpm.h"

#ifdef __cplusplus
extern "C" {
#endif

#define CPM_MAX_BATCH 64
/* cpm_get_info keys.  (Not 10 and 11: the key behind CPM_INFO_STEPS_REPEATED is pinned as unknown by the ABI harness of cpm.h.) */
#define CPM_INFO_BATCH 16              /* fleets of the installed batch tables (0: none) */
#define CPM_INFO_LAST_BATCH_FLEETS 17  /* fleets of the most recent batch step whose counts the batched kernels produced; 0 after any
                                        * other step, and after a batch step whose fleets all ran through the single-fleet step */
#define CPM_FORM_BATCH 10              /* CPM_INFO_LAST_FORM of a batch step that ran the batched kernels (CPM_INFO_LAST_KERNEL is then
                                        * CPM_KERNEL_ZONE_GROUPED) */

/* p_drives: Z x T x B Float64 (Julia p_drives[:,:,b]); replaces the batch tables.  The context's own p_drive is untouched. */
int32_t cpm_set_p_drive_batch(cpm_ctx *ctx, int32_t B, const double *p_drives);
/* createpdrive once per fleet from the cached Z x Z x T mean (as cpm_build_p_drive): fleet b = (p_min[b], p_max[b], e_drive[b]) */
int32_t cpm_build_p_drive_batch(cpm_ctx *ctx, int32_t B, const double *p_min, const double *p_max, const double *e_drive);
/* p_drives_out: Z x T x B of the installed batch tables */
int32_t cpm_get_p_drive_batch(cpm_ctx *ctx, double *p_drives_out);
/* blocking: parking / driving Z x T x B Int64, sum_tt_q16[B] (may be NULL); seeds[B].  Overflowed fleets are repeated by the
 * call itself (regions grown, or the single-fleet step). */
int32_t cpm_resample_batch(cpm_ctx *ctx, const uint64_t *seeds, uint32_t flags, int64_t *parking, int64_t *driving,
                           int64_t *sum_tt_q16_or_null);
/* asynchronous: d_counts = DEVICE int64[B][2*T*Z + 2], each fleet laid out like cpm_resample_dev's tensor with its own status
 * word.  A fleet whose status word is non-zero has invalid counts: the caller repeats it (as with cpm_resample_dev); the batch steps
 * that follow run on grown regions. */
int32_t cpm_resample_batch_dev(cpm_ctx *ctx, const uint64_t *seeds, uint32_t flags, void *d_counts);

#ifdef __cplusplus
}
#endif
#endif
