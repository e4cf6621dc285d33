/*
 * cpm_expected_sparse_tangent.h -- the forward tangent of the expected densities straight from the compact rows of sparse p_destin
 * tables and the compact tangent of cpm_expected_sparse_dest.h: K columns of the Jacobian of the densities, what a Gauss-Newton /
 * Levenberg-Marquardt step needs, without the dense p_destin array and without the dense tangent array.  The last member of the
 * noise-free family that read them: after it every cpm_expected* call of the library runs on a sparse dataset from the stored cells.
 *
 * Argument lists, layouts, the flag (CPM_EXPECT_IVP), K = 1 .. CPM_TANGENT_MAX_DIRECTIONS, the definition, the error bound and the
 * refusals are those of cpm_expected_tangent[_dev] (cpm_expected_tangent.h).  On top of them, in front of anything that is read,
 * copied or enqueued:
 *   CPM_ERR_STATE when the installed tables have no compact rows (CPM_INFO_SPARSE_TABLES == 0; cpm_last_error() names the two routes
 *     that produce them);
 *   CPM_ERR_STATE when some c_dest[k] != 0 and no COMPACT tangent is installed (CPM_INFO_DEST_TANGENT_COMPACT == 0).  A resident dense
 *     tangent does not count: the two tangents are independent (cpm_expected_sparse_dest.h).
 * CPM_ERR_TABLE for a row total above 1 carries the dense call's text.
 *
 * Contract: every output word carries the bits of cpm_expected_tangent[_dev] on a context that holds the same tables and the same
 * tangent: d_out (d_parking, d_driving), d_dpi_next and the primal, which therefore also carries the bits of cpm_expected_sparse_dev
 * and cpm_expected_dev.  The calls never read, build or allocate the dense p_destin array or the dense tangent array
 * (CPM_INFO_P_DENSE and CPM_INFO_DEST_TANGENT_DENSE stay 0), and they change nothing a later call of any family reads.  Direction k
 * alone gives the bits it gives among 16; the same inputs give the same bits every time.  No floating-point atomics.
 *
 * Why the bits agree.  Of one operator of hour t the dense kernel forms, per destination d and vector (the primal x and each
 * direction's dx),
 *   y[d] = the sum over origins o of dx[o] * p[o, d],      u[d] = the sum over origins o of xm[o] * dP[t][d][o],
 * xm the primal x with the origins of zero rows set to 0.  Both are sums down a destination's column in the order of the dense
 * kernel's stream and block sum, which cpm_expected_sparse.h restates as the lane rule: origin o belongs to one of 256 lanes (by
 * (o >> 1) & 255, or ((o - 1) >> 1) & 255 where an odd Z puts the row 8 bytes behind a 16-byte line, the odd end behind lane 0's
 * pairs); a lane starts at +0.0 and adds a = a + term in ascending origin, one rounding for the product and one for the sum; the
 * lanes go through the fixed wave tree and the four waves are added in order.  The sparse kernel keeps exactly that order over the
 * STORED cells of the column and skips the others.
 *   The primal: the argument of cpm_expected_sparse.h.  Terms are non-negative and a cell that is not stored adds +0.
 *   The signed vectors: the argument of cpm_expected_sparse_dest.h carries over.  A cell that is not stored has p == 0, so for a finite
 *   dx it contributes +0 or -0.  A lane's accumulator starts at +0.0 and is +0.0 or non-zero after every step, never -0.0: +0 + -0 =
 *   +0, exact cancellation rounds to +0 (round to nearest), and a product that underflows to -0 is absorbed the same way.  Adding +-0
 *   to +0 gives +0 and to a non-zero value gives that value.  So skipping the cell changes no bit, for terms of either sign.
 *   u: xm >= 0, and the dense twin's tangent is 0 off the stored cells (precondition, below), so an unstored cell contributes +-0 as
 *   well.  A kept cell of weight 0 that carries a tangent IS a stored cell: it takes part in both orders.  u is formed on xm, not x:
 *   the origin of a zero row contributes nothing whatever its cells carry, as in the dense call.
 * Everything behind the column sums -- the residual lists, dstay, (dstay + y) + res, the zero-row term, + c_dest[k] * u[d], dx_next
 * and the primal's own epilogue -- is the dense kernel's epilogue, operation for operation, on the same workspace.
 *
 * Preconditions.  Every dx the call forms is finite: the blocking form refuses non-finite dpi0 / dp_drive, the _dev form does not
 * check.  (dq is exactly 0 where p_drive is clipped, NaN included: the rule of cpm_expected_tangent.h, unchanged.)  The dense twin's
 * tangent is 0 off the stored cells: true of both compact installers by construction.
 *
 * How it runs.  One launch per operator and pass, as in the dense call; the stored cells of a column are walked 256 at a time in the
 * transposed, lane-sorted order cpm_expected_sparse_dev keeps.  The compact tangent is carried into that order once per tangent and
 * table build (8 bytes per stored cell, allocated and built only by a call with a non-zero c_dest); u rides on the first pass's walk
 * as one more product per cell, where the dense call streams a second Z x Z block.
 *
 * Not here: tangents of the batch tables' fleets, the objectives' JVP on the device, the sharded layer.
 */
#ifndef CPM_EXPECTED_SPARSE_TANGENT_H
#define CPM_EXPECTED_SPARSE_TANGENT_H

#include "cpm_expected_tangent.h"
#include "cpm_expected_sparse_dest.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cpm_expected_tangent_dev from the compact rows and the compact tangent; enqueued on the context's stream */
int32_t cpm_expected_sparse_tangent_dev(cpm_ctx *ctx, int32_t K, const void *d_pi0_or_null, uint32_t flags, const void *d_dpi0_or_null,
                                        const void *d_dp_drive_or_null, const double *c_dest, void *d_out, void *d_dpi_next_or_null,
                                        void *d_expected_or_null);

/* cpm_expected_tangent likewise; blocking */
int32_t cpm_expected_sparse_tangent(cpm_ctx *ctx, int32_t K, const double *pi0_or_null, uint32_t flags, const double *dpi0_or_null,
                                    const double *dp_drive_or_null, const double *c_dest, double *d_parking, double *d_driving, double *dpi_next_or_null,
                                    double *parking_or_null, double *driving_or_null);

#ifdef __cplusplus
}
#endif
#endif
