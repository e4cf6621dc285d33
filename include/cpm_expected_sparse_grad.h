/*
 * cpm_expected_sparse_grad.h -- the adjoint of the expected densities (single and batched), the trip weights, the travel product and
 * cpm_expected_fit straight from the compact rows of sparse p_destin tables: what cpm_expected_sparse.h left to the dense array.
 *
 * Contract: every output word of every call below carries the bits of its dense namesake (cpm_expected_grad.h,
 * cpm_expected_grad_batch.h, cpm_expected_travel.h, cpm_expected_fit.h) on the same context.  The calls never read or build the
 * dense [T][Z][Z] p_destin array (CPM_INFO_P_DENSE does not change), and they change no state a later call reads: a resample, a
 * cpm_expected* call or a call of any other family gives what it would have given without them.  After these calls a fit on a sparse
 * dataset never holds the dense array.
 *
 * Why the backward operator needs no transpose.  It forms u[o] = sum over d of p[t][d][o] * mu[d]: a sum along origin o's OWN row of
 * the table, and the compact rows store exactly that row, sorted by destination.  (The forward operator sums along a destination's
 * column, which is why cpm_expected_sparse.h builds the rows' transpose.)  Beside the rows the calls need l and r of the
 * per-table arrays of cpm_expected_sparse.h, which are word for word the dense builder's.
 *
 * Why the bits are those of the dense call.  The dense product kernel fixes the order of the sum:
 *   nseg = grad_segments(Z), a function of Z alone, at most 64; seg_len = ceil(Z / nseg);
 *   destination d of origin o's row belongs to segment s = d / seg_len and to chain v = (d - s * seg_len) & 3;
 *   a chain starts at +0.0 and adds acc = acc + p * mu[d] in ascending d -- one rounding for the product, one for the sum;
 *   the four chains of a segment are added as ((w0 + w1) + w2) + w3 and stored as part[s][o] (part[s][f][o] for fleet f of a pass);
 *   the finishing kernel adds the segments in ascending order and then the residual term r * mu[l].
 * Which lane of the dense kernel owns an origin changes no sum.  Zero cells change no bit: a cell with p = 0 contributes +-0 for
 * finite mu, and a chain that starts at +0.0 and is +0.0 or non-zero after every step never becomes -0.0, because +0 + -0 = +0 and
 * exact cancellation rounds to +0; adding +-0 to it changes nothing.  So it suffices to give each STORED cell with d < Z to chain
 * (s, v) in ascending d (cells with d >= Z are skipped by every builder; cells of weight 0, which the dataset route keeps, are
 * harmless) and to write +0.0 for chains and segments without cells.  Empty trailing segments exist -- at Z = 1,089, nseg = 34 and
 * seg_len = 33, so segment 33 begins at 1,089 -- and the dense kernel stores +0.0 there: every word part[s][o] with s < nseg, o < Z is
 * written.  The finishing kernels are the dense call's own, fed the same layouts.  For the batch, each fleet's chains are those of
 * the single call operation for operation, so fleet b carries the bits of the B = 1 call.
 *
 * Precondition (adjoint): mu stays finite.  The blocking calls refuse non-finite cotangents, as their namesakes do; the _dev calls
 * do not check, and there 0 * inf = NaN of a cell that is not stored would differ from the dense call.
 *
 * The trip weights w_sec[t][o] = sum over d of p[t][d][o] * sec(o, d, t), w_km likewise, follow the same scheme with
 * trip_segments(Z, T) (at most 8) segments, the term p * (d == o ? 300.0 : mean[t][d][o]) and p * (d == o ? 1.0 : dist[d][o]), and
 * the dense call's finishing kernel.  The mean plane and the distances are read at the stored cells only.
 *
 * Precondition (trip weights, travel, fit): every mean word and every distance at a cell that is NOT stored must be finite.  The
 * dense kernel forms 0 * value there, and cpm_expected_travel.h passes non-finite means through (a NaN mean makes the dense weight
 * NaN even where p = 0); the sparse calls never see that word.  Negative means are fine.  The sparse weights live in a cache of
 * their own, so where the precondition fails a sparse call still changes nothing a later dense call returns.
 * cpm_expected_trip_builds counts dense builds only.
 *
 * cpm_expected_sparse_fit*: cpm_expected_fit with the propagation, the trip weights and the adjoint from the compact rows.
 * CPM_FIT_DEST is refused with CPM_ERR_ARG: the e_dest direction needs the tangent of p_destin, which is a dense [T][Z][Z] array;
 * use cpm_expected_fit for it.  The sparse form of cpm_expected_grad_dest*, on a compact tangent that lifts this refusal, is
 * cpm_expected_sparse_dest.h; the sparse form of cpm_expected_tangent is cpm_expected_sparse_tangent.h.
 *
 * Argument lists, layouts, flags and errors are those of the namesakes, with the two additions of cpm_expected_sparse.h:
 *   CPM_ERR_STATE when the installed p_destin tables have no compact rows; cpm_last_error() names the two routes that produce them;
 *   CPM_ERR_TABLE for a non-zero row whose total exceeds 1 + Z * 2^-52, with the text, the hour and the origin of the dense call.
 * Without a usable device every entry returns CPM_ERR_HIP.
 */
#ifndef CPM_EXPECTED_SPARSE_GRAD_H
#define CPM_EXPECTED_SPARSE_GRAD_H

#include "cpm_expected_travel.h"
#include "cpm_expected_fit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cpm_expected_grad_dev / cpm_expected_grad from the compact rows */
int32_t cpm_expected_sparse_grad_dev(cpm_ctx *ctx, const void *d_pi0_or_null, uint32_t flags, const void *d_cotangent, const void *d_gnext_or_null,
                                     void *d_grad_p_drive, void *d_grad_pi0_or_null);
int32_t cpm_expected_sparse_grad(cpm_ctx *ctx, const double *pi0_or_null, uint32_t flags, const double *g_parking, const double *g_driving,
                                 const double *g_next_or_null, double *grad_p_drive, double *grad_pi0_or_null);

/* cpm_expected_grad_batch_dev / cpm_expected_grad_batch from the compact rows (no grad_dest form: the tangent is a dense array) */
int32_t cpm_expected_sparse_grad_batch_dev(cpm_ctx *ctx, const void *d_pi0_or_null, uint32_t flags, const void *d_cotangent,
                                           const void *d_gnext_or_null, void *d_grad_p_drive, void *d_grad_pi0_or_null);
int32_t cpm_expected_sparse_grad_batch(cpm_ctx *ctx, const double *pi0_or_null, uint32_t flags, const double *g_parking, const double *g_driving,
                                       const double *g_next_or_null, double *grad_p_drive, double *grad_pi0_or_null);

/* cpm_expected_trip_dev / cpm_expected_trip from the compact rows: d_w DEVICE f64[2][T][Z], w_sec | w_km */
int32_t cpm_expected_sparse_trip_dev(cpm_ctx *ctx, void *d_w);
int32_t cpm_expected_sparse_trip(cpm_ctx *ctx, double *w_sec, double *w_km);

/* cpm_expected_travel_dev with the sparse weights; cpm_expected_travel / cpm_expected_travel_batch with the propagation of
 * cpm_expected_sparse.h and the sparse weights */
int32_t cpm_expected_sparse_travel_dev(cpm_ctx *ctx, const void *d_expected, int32_t B, void *d_travel_or_null, void *d_totals_or_null);
int32_t cpm_expected_sparse_travel(cpm_ctx *ctx, const double *pi0_or_null, uint32_t flags, double *seconds, double *km, double *totals_or_null);
int32_t cpm_expected_sparse_travel_batch(cpm_ctx *ctx, const double *pi0_or_null, uint32_t flags, double *seconds, double *km, double *totals_or_null);

/* cpm_expected_fit_dev / cpm_expected_fit from the compact rows; CPM_FIT_DEST and a non-NULL grad_dest are refused (CPM_ERR_ARG) */
int32_t cpm_expected_sparse_fit_dev(cpm_ctx *ctx, int32_t B, const double *p_min, const double *p_max, const double *e_drive, const void *d_pi0_or_null,
                                    uint32_t flags, const double *weights, void *d_record, void *d_expected_or_null, void *d_cotangent_or_null,
                                    void *d_grad_p_drive_or_null, void *d_grad_dest_must_be_null);
int32_t cpm_expected_sparse_fit(cpm_ctx *ctx, int32_t B, const double *p_min, const double *p_max, const double *e_drive, const double *pi0_or_null,
                                uint32_t flags, const double *weights, double *record, double *expected_or_null, double *cotangent_or_null,
                                double *grad_p_drive_or_null, double *grad_dest_must_be_null);

#ifdef __cplusplus
}
#endif
#endif
