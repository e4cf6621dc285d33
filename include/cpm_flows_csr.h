/*
 * cpm_flows_csr.h -- the hourly origin-destination (OD) trip counts of cpm_flows.h as compressed sparse rows.
 *
 * The dense tensor of cpm_resample_flows, int32[T][Z][Z], is mostly zeros: a row holds the drivers of one zone and one hour, a few
 * hundred cars for thousands of destinations, and at Z = 8,192 the tensor is 6.4 GB.  The calls below return the same counts with
 * the zeros left out, in canonical CSR over the rows r = t*Z + o of that tensor:
 *
 *   row_ptr  int64[T*Z + 1]   row_ptr[0] = 0, non-decreasing, row_ptr[T*Z] = nnz = the number of non-zero cells of the dense tensor
 *                             (64-bit: the bound T * min(cars, Z*Z) passes 2^31 for large contexts)
 *   dest     int32[nnz]       dest[k], row_ptr[r] <= k < row_ptr[r+1]: the index d of flows[(t*Z + o)*Z + d], 0-based like the tensor's
 *                             own index, strictly ascending within a row
 *   count    int32[nnz]       count[k] = that cell, every entry > 0
 *
 * The layout is a function of the counts alone: bit-identical from run to run and across kernel families, hour forms and flows
 * forms (no arrival order of anything decides where a row lands).  In Julia terms
 *     SparseMatrixCSC(Z, Z*T, row_ptr .+ 1, dest .+ 1, count)
 * indexed [destination, (hour-1)*Z + origin]: column (hour-1)*Z + origin of it is the dense Array{Int32,3}'s [:, origin, hour].
 *
 * Conventions are those of cpm.h: int32 status, cpm_last_error(), no abort across the boundary, no CPU fallback.
 * CPM_OPT_FLOWS_KEPT (cpm_flows.h) applies unchanged: one set of launches behind every hour, or one over the kept runs of all hours;
 * a travel resample and a context under CPM_OPT_FUSED 6 .. 8 take the kept form, as for the dense tensor.  A row of Z zones must fit
 * twice in LDS (Z <= 20,400).
 */
#ifndef CPM_FLOWS_CSR_H
#define CPM_FLOWS_CSR_H

#include "cpm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* device-resident form, enqueued on the context's stream like cpm_resample_flows_dev.  d_counts as for cpm_resample_dev; d_row_ptr a
 * DEVICE pointer to int64[T*Z + 1]; d_dest, d_count DEVICE pointers to int32[cap].  d_row_ptr is always written completely and
 * exactly: d_row_ptr[T*Z] is the size the step needs even where it exceeds cap.  Entries with index < cap are written and valid;
 * nothing is stored at or behind cap.  cap = 0 (d_dest, d_count may then be NULL) sizes only.  status != 0 in d_counts invalidates
 * all three arrays; the caller repeats the step.  d_counts, d_row_ptr NULL, cap < 0, or cap > 0 with a NULL entry array: CPM_ERR_ARG. */
int32_t cpm_resample_flows_csr_dev(cpm_ctx *ctx, uint64_t seed, uint32_t flags, void *d_counts, void *d_row_ptr, void *d_dest, void *d_count,
                                   int64_t cap);

/* blocking form: parking, driving and the travel-time sum bit for bit those of cpm_resample with the same seed and flags; the
 * context's state is left unchanged; an overflowed step is repaired by the call itself.  Fills the HOST row_ptr_out[T*Z + 1] and
 * *nnz_out (= row_ptr_out[T*Z]); the entries stay on the device, in arrays the context owns (allocated by the first call, freed with
 * the context), until cpm_get_flows_csr fetches them.  The call never truncates and never asks for a retry: where its arrays were too
 * small it has run the step again on larger ones.  sum_travel_time_q16 may be NULL; the other pointers may not (CPM_ERR_ARG). */
int32_t cpm_resample_flows_csr(cpm_ctx *ctx, uint64_t seed, uint32_t flags, int64_t *parking_counts, int64_t *driving_counts,
                               int64_t *sum_travel_time_q16, int64_t *row_ptr_out, int64_t *nnz_out);

/* the entries of the last cpm_resample_flows_csr of this context: dest_out, count_out HOST int32[nnz].  CPM_ERR_ARG when there was no
 * such call or nnz is not the value it reported (size, allocate exactly, fetch).  nnz = 0 copies nothing. */
int32_t cpm_get_flows_csr(cpm_ctx *ctx, int32_t *dest_out, int32_t *count_out, int64_t nnz);

#ifdef __cplusplus
}
#endif
#endif
