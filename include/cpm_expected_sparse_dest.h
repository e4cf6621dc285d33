/*
 * cpm_expected_sparse_dest.h -- the e_dest direction straight from the compact rows of sparse p_destin tables: a compact tangent of
 * p_destin on the stored cells, the adjoint along it (single and batched), the tangent of the trip weights, and cpm_expected_sparse_fit
 * with CPM_FIT_DEST.  What the header of cpm_expected_sparse_grad left to the dense tangent array.
 *
 * Compact tangent.  One per context: sdp, f64 [T * Z][cap], cap the cells a compact row can hold.  Word e of row (t, o) is the tangent
 * dP[t][d][o] at the cell d = sj[row * cap + e] that word e of the row of p stores: entry for entry with the compact rows.  It is
 * allocated by the first call that installs one (8 * T * Z * cap bytes, the size of the rows' values; the dense tangent of
 * cpm_expected_grad_dest.h takes 8 * Z * Z * T).  Every call that drops the dense tangent drops it: any call that installs p_destin
 * tables and any new datamatrix.  The two tangents are independent: installing one neither installs nor drops the other, and the dense
 * calls of cpm_expected_grad_dest.h keep answering CPM_ERR_STATE while only the compact one exists.
 *   CPM_INFO_DEST_TANGENT_DENSE    1 when the dense tangent array is allocated and belongs to the installed tables, else 0;
 *   CPM_INFO_DEST_TANGENT_COMPACT  1 when a compact tangent is installed, else 0.
 *
 * Contract: every output word of every call below carries the bits of its dense namesake (cpm_expected_grad_dest.h,
 * cpm_expected_grad_batch.h, cpm_expected_fit.h) on a context that holds the same tables and the same tangent: grad_dest,
 * grad_p_drive, grad_pi0, dw_sec, dw_km and every word of a fit record, dF / d e_dest included.  The calls never read, build or
 * allocate the dense p_destin array or the dense tangent array (CPM_INFO_P_DENSE and CPM_INFO_DEST_TANGENT_DENSE stay 0), and they
 * change no state a later call reads.  After them a four-parameter gradient fit on a sparse dataset holds neither dense array.
 *
 * Why the bits agree.  The argument is the one the header of cpm_expected_sparse_grad makes for u.  w[o] = sum over d of dP[t][d][o] * mu[d] is a sum along
 * origin o's own row, the layout the compact rows store, and the dense kernel fixes its order as it fixes that of u:
 *   destination d belongs to segment s = d / seg_len (nseg = grad_segments(Z), seg_len = ceil(Z / nseg)) and to chain
 *   (d - s * seg_len) & 3; a chain starts at +0.0 and adds acc = acc + dP * mu[d] in ascending d, one rounding for the product and one
 *   for the sum; the four chains are added as ((w0 + w1) + w2) + w3 and stored as part_dp[s][o] (part_dp[s][f][o] for fleet f of a pass);
 *   the unchanged finishing kernels add the segments in ascending order; there is no residual term and w = 0 for a zero row.
 * A cell that is not stored has dP == 0 in the dense array (precondition below), so it contributes +-0 for finite mu, and a chain that
 * starts at +0.0 and is +0.0 or non-zero after every step never becomes -0.0: +0 + -0 = +0 and exact cancellation rounds to +0, for
 * terms of either sign.  Skipping the cell changes no bit.  So each STORED cell with d < Z goes to chain (s, v) in ascending d, mu[d] is
 * gathered once for the products with p and with dP, and +0.0 is written for chains and segments without cells, the empty trailing
 * segments of sizes like Z = 1,089 included.  The chains of u are those of cpm_expected_sparse_grad operation for operation, so
 * grad_p_drive and grad_pi0 carry the bits of that call as well.  For the batch each fleet's chains are those of the single call.
 * The tangent of the trip weights, dw = sum over d of dP * sec(o, d, t), is the walk of cpm_expected_sparse_trip with dP in place of p.
 *
 * Preconditions.  A finite mu (adjoint): the blocking calls refuse non-finite cotangents, the _dev calls do not check.  Finite means
 * and distances at cells that are not stored (trip tangent, fit), as for cpm_expected_sparse_trip.  And the dense twin's tangent is 0
 * off the stored cells: true of both installers below by construction.
 *
 * cpm_build_p_dest_tangent_sparse: d p_destin / d e_dest with the preconditions, the definition and the error bound of
 * cpm_build_p_dest_tangent, and the same operations per cell as that call's compact-row route: m = m + p * log(x) over the cells with
 * p > 0 in ascending destination, then p * (log(x) - m).  Cells with p == 0 or a destination >= Z get exactly +0.0.  Enqueued on the
 * context's stream.  CPM_ERR_STATE where the dense builder returns it, and where the tables have no compact rows or were uploaded.
 *
 * cpm_set_p_dest_tangent_sparse: the argument of cpm_set_p_dest_tangent, compacted onto the stored cells.  The array goes up hour by
 * hour through a staging buffer of one Z x Z block, which is released before the call returns; the dense device array is never
 * allocated.  CPM_ERR_ARG for an entry that is not finite; CPM_ERR_TABLE for a non-zero entry at a cell the rows do not store
 * (cpm_last_error() names hour, origin and destination).  Either way nothing is installed and an earlier tangent stays.  The route for
 * uploaded tables (CPM_OPT_SPARSE_UPLOAD) and for hand-made tangents.
 *
 * cpm_expected_sparse_fit[_dev] accepts CPM_FIT_DEST, and then a non-NULL grad_dest, while a compact tangent is installed; without
 * one it refuses the flag with CPM_ERR_ARG as before.
 *
 * Argument lists, layouts, flags and errors are those of the namesakes, with CPM_ERR_STATE when the tables have no compact rows
 * (cpm_last_error() names the two routes that produce them) or no compact tangent is installed, in front of anything that is read,
 * copied or enqueued.  Without a usable device every entry returns CPM_ERR_HIP.
 */
#ifndef CPM_EXPECTED_SPARSE_DEST_H
#define CPM_EXPECTED_SPARSE_DEST_H

#include "cpm_expected_grad_dest.h"
#include "cpm_expected_grad_batch.h"
#include "cpm_expected_fit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cpm_get_info keys */
#define CPM_INFO_DEST_TANGENT_DENSE 25
#define CPM_INFO_DEST_TANGENT_COMPACT 26

/* d p_destin / d e_dest of the installed tables onto the stored cells; enqueued on the context's stream */
int32_t cpm_build_p_dest_tangent_sparse(cpm_ctx *ctx);

/* dp: borrowed host Z x Z x T Float64 column-major, [origin, destination, hour].  Blocking. */
int32_t cpm_set_p_dest_tangent_sparse(cpm_ctx *ctx, const double *dp);

/* out: host Z x Z x T Float64 column-major; the cells' words, +0.0 elsewhere.  Blocking. */
int32_t cpm_get_p_dest_tangent_sparse(cpm_ctx *ctx, double *out);

/* cpm_expected_grad_dest_dev / cpm_expected_grad_dest from the compact rows and the compact tangent */
int32_t cpm_expected_sparse_grad_dest_dev(cpm_ctx *ctx, const void *d_pi0_or_null, uint32_t flags, const void *d_cotangent, const void *d_gnext_or_null,
                                          void *d_grad_p_drive, void *d_grad_pi0_or_null, void *d_grad_dest);
int32_t cpm_expected_sparse_grad_dest(cpm_ctx *ctx, const double *pi0_or_null, uint32_t flags, const double *g_parking, const double *g_driving,
                                      const double *g_next_or_null, double *grad_p_drive, double *grad_pi0_or_null, double *grad_dest);

/* cpm_expected_grad_dest_batch_dev / cpm_expected_grad_dest_batch likewise */
int32_t cpm_expected_sparse_grad_dest_batch_dev(cpm_ctx *ctx, const void *d_pi0_or_null, uint32_t flags, const void *d_cotangent,
                                                const void *d_gnext_or_null, void *d_grad_p_drive, void *d_grad_pi0_or_null, void *d_grad_dest);
int32_t cpm_expected_sparse_grad_dest_batch(cpm_ctx *ctx, const double *pi0_or_null, uint32_t flags, const double *g_parking, const double *g_driving,
                                            const double *g_next_or_null, double *grad_p_drive, double *grad_pi0_or_null, double *grad_dest);

/* cpm_expected_trip_tangent_dev / cpm_expected_trip_tangent from the compact tangent: d_dw DEVICE f64[2][T][Z], dw_sec | dw_km */
int32_t cpm_expected_sparse_trip_tangent_dev(cpm_ctx *ctx, void *d_dw);
int32_t cpm_expected_sparse_trip_tangent(cpm_ctx *ctx, double *dw_sec, double *dw_km);

#ifdef __cplusplus
}
#endif
#endif
