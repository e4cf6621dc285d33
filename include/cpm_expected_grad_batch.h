/*
 * cpm_expected_grad_batch.h -- the adjoint of the expected densities of libcpm_hip.so for the B fleets of the installed batch tables:
 * the gradients of cpm_expected_grad.h and cpm_expected_grad_dest.h for B fleets in one pass over the p_destin tables.
 *
 * The points of a sweep come in runs that share e_dest, hence one p_destin, and the hour's Z x Z block of p dominates the bytes of
 * a backward operator.  cpm_expected_batch reads that block once for the fleets of a pass; these calls do the same backward: the
 * block of p -- and of the tangent dP -- is streamed once per operator and pass of at most 8 fleets.
 *
 * Contract.  Fleet b's slices of every output carry the bits of the B = 1 call (cpm_expected_grad_dev, cpm_expected_grad_dest_dev)
 * with fleet b's p_drive installed and fleet b's cotangents -- whatever B is, whatever b is and however the fleets were dealt to
 * passes.
 *
 * Everything else is inherited.  The definition of the backward pass, the order of every sum (the segments, the four chains, the
 * residual term), exact 0 at p_drive entries outside (0, 1) and the error bounds are those of cpm_expected_grad.h; grad_dest, the
 * tangent table and their bounds are those of cpm_expected_grad_dest.h.
 *
 * B is the installed batch of cpm_set_p_drive_batch / cpm_build_p_drive_batch (cpm_batch.h), 1 .. CPM_MAX_BATCH.  All fleets start
 * from the same pi_0, as in cpm_expected_batch.  Every fleet has its own cotangents, laid out like cpm_expected_batch_dev's d_out
 * (f64[B][2][T][Z]: a cotangent tensor can be formed in place from that call's output), and its own G_next (f64[B][Z]); NULL means
 * zeros for all fleets, and the last operator's product is then skipped for all of them.  The tangent dP is the context's one
 * table, shared by the fleets.
 *
 * No floating-point atomics; the same inputs give the same bits every time; every word of the outputs is written and nothing else;
 * no state that a later cpm_expected*, gradient or resample call reads is changed -- the context's own p_drive and the batch tables
 * included.
 *
 * Workspace of the context, in f64 words with Zs = Z rounded up to even, B8 = B rounded up to a multiple of 8 and S the segments
 * of cpm_expected_grad.h:
 *   ((2T - 1) * B + 2 * B + 2 * B8 + 16 * S) * Zs
 * -- pi_s of all operators and fleets, x and mu twice over, the segments' sums of one pass for p and for dP.  At Z = 4,096, T = 24,
 * B = 64 that is 124 MB, 99 MB of it pi_s.  It is shared with the B = 1 calls and only grows.
 *
 * Status codes are those of the B = 1 calls, and: CPM_ERR_STATE without batch tables; in the blocking forms CPM_ERR_ARG for a
 * cotangent word that is not finite, cpm_last_error() naming the fleet, the zone and the hour (all 1-based).  Every check that can
 * refuse comes before anything is enqueued.  Conventions are those of cpm.h.
 */
#ifndef CPM_EXPECTED_GRAD_BATCH_H
#define CPM_EXPECTED_GRAD_BATCH_H

#include "cpm_expected_grad_dest.h"

#ifdef __cplusplus
extern "C" {
#endif

/* enqueued on the context's stream.
 * d_pi0_or_null: DEVICE f64[Z]; NULL: uniform 1 / Z.  Read only.  flags: CPM_EXPECT_IVP or 0.
 * d_cotangent: DEVICE f64[B][2][T][Z], per fleet G_park then G_drv.  Read only.
 * d_gnext_or_null: DEVICE f64[B][Z]; NULL: zeros.  Read only.
 * d_grad_p_drive: DEVICE f64[B][T][Z]; every word written.
 * d_grad_pi0_or_null: DEVICE f64[B][Z]; every word written.  NULL: not wanted. */
int32_t cpm_expected_grad_batch_dev(cpm_ctx *ctx, const void *d_pi0_or_null, uint32_t flags, const void *d_cotangent, const void *d_gnext_or_null,
                                    void *d_grad_p_drive, void *d_grad_pi0_or_null);

/* blocking.  pi0_or_null: borrowed host f64[Z] or NULL.  g_parking / g_driving: Z x T x B Float64 column-major.
 * g_next_or_null: Z x B.  grad_p_drive: Z x T x B.  grad_pi0_or_null: Z x B. */
int32_t cpm_expected_grad_batch(cpm_ctx *ctx, const double *pi0_or_null, uint32_t flags, const double *g_parking, const double *g_driving,
                                const double *g_next_or_null, double *grad_p_drive, double *grad_pi0_or_null);

/* enqueued on the context's stream.  Arguments as cpm_expected_grad_batch_dev, and
 * d_grad_dest: DEVICE f64[B][T][Z]; every word written.  Needs a tangent (CPM_ERR_STATE). */
int32_t cpm_expected_grad_dest_batch_dev(cpm_ctx *ctx, const void *d_pi0_or_null, uint32_t flags, const void *d_cotangent, const void *d_gnext_or_null,
                                         void *d_grad_p_drive, void *d_grad_pi0_or_null, void *d_grad_dest);

/* blocking.  Arguments as cpm_expected_grad_batch, and grad_dest: Z x T x B Float64 column-major. */
int32_t cpm_expected_grad_dest_batch(cpm_ctx *ctx, const double *pi0_or_null, uint32_t flags, const double *g_parking, const double *g_driving,
                                     const double *g_next_or_null, double *grad_p_drive, double *grad_pi0_or_null, double *grad_dest);

#ifdef __cplusplus
}
#endif
#endif
