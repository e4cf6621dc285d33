/*
 * cpm_expected_sparse.h -- the expected densities of cpm_expected.h straight from the compact rows of sparse p_destin tables.
 *
 * Contract: every output word, and pi_next, carries the bits of the corresponding cpm_expected* call on the same context.
 *
 * The calls of cpm_expected.h read p_destin as the dense [T][Z][Z] array; for tables with sparse row packs (CPM_INFO_SPARSE_TABLES > 0:
 * cpm_build_p_dest on a sparse datamatrix, or cpm_set_p_dest under CPM_OPT_SPARSE_UPLOAD) they expand the compact rows to that array
 * first.  The calls below evaluate the same recurrence -- the definition in cpm_expected.h holds word for word -- from the stored cells
 * alone.  They never read or build the dense p_destin array (CPM_INFO_P_DENSE does not change), and they change no state a later
 * call reads: a resample, a cpm_expected* call or a call of any other family gives what it would have given without them.
 *
 * Why the bits are those of the dense call.  The dense kernel fixes the order of every sum: per destination d of hour t, a workgroup
 * of 256 lanes walks the dense row over the origins, a lane adds its own origins in ascending order (each term a = a + x[o] * p, one
 * rounding for the product and one for the sum), the 64 lanes of a wave pass through a fixed shuffle tree and the four waves are
 * added in order.  A cell with p = 0 contributes x * 0 = +0; adding +0 to a sum that starts at +0 and receives only non-negative
 * terms changes no bit.  So it suffices to give every STORED cell to the lane the dense kernel gives it to, in the same order.
 * That lane is a function of (o, Z, the alignment of the dense row) alone -- the lane rule:
 *   npairs = Z >> 1;  head(t, d) = Z odd && (t * Z * Z + d * Z) odd: the dense row of (t, d) then starts 8 bytes behind a 16-byte line;
 *   Z even:            head = 0 everywhere: origin o belongs to lane (o >> 1) & 255;
 *   Z odd, head = 0:   origin o < Z - 1 belongs to lane (o >> 1) & 255; the last origin Z - 1 to lane 0, AFTER all of lane 0's pairs;
 *   Z odd, head = 1:   origin o >= 1 belongs to lane ((o - 1) >> 1) & 255; origin 0 to lane 0, AFTER all of lane 0's pairs;
 *   within a lane: ascending origin.
 * (For odd Z head(t, d) = (t + d) odd: it alternates along the destinations and, at a fixed destination, from hour to hour.)
 * The sparse kernel keeps each destination column's cells sorted by (lane, place in the lane), lets lane L add its cells in that
 * order and then runs the dense kernel's own code: the wave tree, the four waves, the residual lists, the stay and the zero-row term,
 * ((s + y) + res) (+ x).  l, r and the residual lists come from the compact rows and are word for word those of the dense builder.
 *
 * The first call after the p_destin tables changed builds these per-table arrays (l, r, the residual lists, the transposed cells:
 * 12 bytes per stored cell, sized by their actual number) and synchronises the stream once, for the row-total check and the number
 * of cells; the builder's temporary is freed behind its last kernel, which waits for that kernel.
 *
 * Flags (CPM_EXPECT_IVP), argument lists, output layouts and errors are those of the cpm_expected* namesakes, with two additions:
 *   CPM_ERR_STATE when the installed p_destin tables have no compact rows (CPM_INFO_SPARSE_TABLES == 0); cpm_last_error() names the
 *   two routes that produce them;
 *   CPM_ERR_TABLE for a non-zero row whose total exceeds 1 + Z * 2^-52, with the text, the hour and the origin of the dense call.
 * Without a usable device every entry returns CPM_ERR_HIP.
 *
 * Not here (they read the dense array as before): the adjoints, the tangent, the trip weights, cpm_expected_fit and the refiners.
 */
#ifndef CPM_EXPECTED_SPARSE_H
#define CPM_EXPECTED_SPARSE_H

#include "cpm_expected.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cpm_expected_dev from the compact rows: d_out DEVICE f64[2][T][Z], d_pi_next_or_null DEVICE f64[Z]; enqueued on the context's stream */
int32_t cpm_expected_sparse_dev(cpm_ctx *ctx, const void *d_pi0_or_null, uint32_t flags, void *d_out, void *d_pi_next_or_null);

/* cpm_expected_batch_dev from the compact rows: d_out DEVICE f64[B][2][T][Z]; fleet b carries the bits of a B = 1 call with its
 * p_drive installed */
int32_t cpm_expected_sparse_batch_dev(cpm_ctx *ctx, const void *d_pi0_or_null, uint32_t flags, void *d_out);

/* blocking: cpm_expected and cpm_expected_batch from the compact rows */
int32_t cpm_expected_sparse(cpm_ctx *ctx, const double *pi0_or_null, uint32_t flags, double *parking_density, double *driving_density,
                            double *pi_next_or_null);
int32_t cpm_expected_sparse_batch(cpm_ctx *ctx, const double *pi0_or_null, uint32_t flags, double *parking_density, double *driving_density);

/* Test aid, blocking: the per-table arrays of the installed tables as the sparse builder (sparse != 0) or the dense builder (0: it
 * expands the dense array) left them, built first where they are stale.  ell: int32[T][Z] (0-based last destination with p > 0, Z
 * for a zero row), r: f64[T][Z], start: int32[T][Z + 1], list: int32[T][Z].  The two builders must agree in every word. */
int32_t cpm_expected_sparse_aux(cpm_ctx *ctx, int32_t sparse, int32_t *ell, double *r, int32_t *start, int32_t *list);

#ifdef __cplusplus
}
#endif
#endif
