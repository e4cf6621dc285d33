/*
 * cpm_expected_grad.h -- the adjoint of the expected densities of libcpm_hip.so: the gradient of any differentiable objective of
 * cpm_expected's parking and driving densities with respect to every entry of p_drive and to the start distribution pi_0, in one
 * backward pass over the installed p_destin tables.
 *
 * The expected densities (cpm_expected.h) are a deterministic f64 function of the installed tables, so the sweep's noise-free
 * objectives can be differentiated.  A finite difference costs one propagation per parameter; the adjoint costs about one more
 * propagation for all Z * T entries of p_drive at once.
 *
 * Definition.  Terms are those of cpm_expected.h: q (p_drive as the Bernoulli maps it), p[t][d][o] = p_destin[o, d, t], last, l, r,
 * zero rows, CPM_EXPECT_IVP.  Number the operators s = 0 .. N-1, N = pre + T, pre = T - 1 under CPM_EXPECT_IVP and 0 otherwise; the
 * hour of operator s is t(s) = s for s < pre and s - pre otherwise.  pi_{s+1} = pi_s * M_{t(s)}, parking[j] = pi_{pre+j},
 * driving[j] = pi_{pre+j} * q_j, pi_next = pi_N.
 *
 * Inputs: the cotangents G_park[T][Z] and G_drv[T][Z] (one array [2][T][Z], laid out like cpm_expected_dev's d_out) and an optional
 * G_next[Z] (NULL: zeros).  They define the linear functional
 *   L = <G_park, parking> + <G_drv, driving> + <G_next, pi_next>;
 * with G = dF/d(parking, driving, pi_next) the outputs are, by the chain rule, the gradient of F at the installed tables.
 *
 * Backward pass.  Every step is ONE IEEE f64 operation (the library is built with -ffp-contract=off).  mu = G_next; for
 * s = N-1 down to 0, with t = t(s) and j = s - pre:
 *   gp = G_park[j] if j >= 0, else 0;  gd = G_drv[j] likewise;
 *   a zero row (last == 0): a[o] = mu[o];
 *   otherwise a[o] = (the sum over d of p[o, d] * mu[d]) + r[o] * mu[l[o]]   (the second term only where l[o] exists);
 *   c[o]      = (gd[o] - mu[o]) + a[o];
 *   dq_s[o]   = pi_s[o] * c[o];
 *   lambda[o] = (gp[o] + mu[o]) + q[o] * c[o];
 *   mu <- lambda.
 * Where mu is zero by construction -- the last operator without G_next: hour T-1, which is sampled and never applied -- the product
 * is skipped and a = 0.
 *
 * Outputs.  grad_pi0[Z] = mu after s = 0.  grad_p_drive[T][Z] = the sum of dq_s[o] over the operators with t(s) = t; under
 * CPM_EXPECT_IVP hours 0 .. T-2 have two operators each, and the day's term is taken first and the IVP's added to it (the order in
 * which the backward pass meets them).  An entry of grad_p_drive is exactly 0 wherever the installed p_drive[o, t] is not strictly
 * inside (0, 1) -- NaN, <= 0, >= 1: q is flat there.
 *
 * pi_s of every operator comes from the forward propagation, which the call runs itself with the kernels of cpm_expected_dev: its
 * bits for pi are those of that call.  (Operator N-1 is not applied: nothing reads pi_N.)
 *
 * Order of the sums (no floating-point atomics; csrc/cpm_expected_grad.h): the destinations are cut into S consecutive segments of
 * ceil(Z / S), S = max(1, min(64, floor(Z / 32), ceil(1024 / ceil(Z / 128)))); within a segment destination d belongs to chain
 * (d - begin) mod 4, a chain adds its products p * mu[d] in ascending d starting from 0, the four chains are added in order,
 * ((c0 + c1) + c2) + c3, then the segments in ascending order, then the residual term.  The order is a function of Z, T and the
 * installed tables alone: the same inputs give the same bits every time.
 *
 * Error bound.  The terms are signed, so the bound is relative to the magnitude recurrence: the same recurrence with |G| in place
 * of G and every difference an addition,
 *   mu~ = |G_next|;  a~ as a with mu~;  c~ = |gd| + mu~ + a~;  lambda~ = |gp| + mu~ + q * c~;  D~_s = pi_s * c~.
 * A product p * mu[d] that ends up in a word of lambda passes one multiplication, at most ceil(ceil(Z / S) / 4) additions of its
 * chain, 3 of the chains, S - 1 of the segments, 1 of the residual term, 1 into c, the multiplication by q and 1 into lambda; every
 * other term passes fewer.  That is at most R = ceil(ceil(Z / S) / 4) + S + 8 roundings of 2^-53 each (the count of the four
 * operations that form c and lambda is rounded up), and
 *   K = 2 * R   (<= Z + 32 for every Z: the chains are at most a quarter of the row)
 * is twice that count.  After n backward operators a word of lambda lies within
 *   n * K * 2^-52 * lambda~
 * of its exact value (each operator adds at most R * 2^-53 * lambda~ of its own, up to second order, and carries the error of mu
 * through the same non-negative recurrence), and dq_s, formed by operator n = N - s, within
 *   (n * K + s * (Z + 8) + 4) * 2^-52 * D~_s
 * where s * (Z + 8) * 2^-52 is cpm_expected.h's bound on pi_s.  An entry of grad_p_drive lies within the sum of the bounds of its
 * one or two dq terms (the + 4 of each covers the product and the addition of the two).  A word whose magnitude is 0 is 0.
 *
 * These calls read the installed p_drive (cpm_set_p_drive / cpm_build_p_drive); the fleets of the batch tables have
 * cpm_expected_grad_batch.h, whose outputs carry these calls' bits fleet by fleet.  The calls need no cars and change
 * no state of the context that a later resample or cpm_expected* call reads.  They keep pi_s of all N operators in a workspace of
 * the context (N * Z words, Z rounded up to even).  The first call after the p_destin tables changed builds l, r and the residual
 * lists and synchronises the stream once, as cpm_expected_dev does.  Tables with sparse row packs are expanded to the dense array
 * first, as for the densities.
 *
 * Status codes are those of cpm_expected: CPM_ERR_STATE without p_drive or p_destin tables, CPM_ERR_TABLE for a row total above 1
 * (cpm_last_error() names the hour and the origin), CPM_ERR_HIP without a usable device; and CPM_ERR_ARG for a NULL cotangent or
 * output, for unknown flag bits and, in the blocking form, for a cotangent word that is not finite.  Conventions are those of
 * cpm.h: int32 status, cpm_last_error(), no abort across the boundary, borrowed column-major host arrays.
 */
#ifndef CPM_EXPECTED_GRAD_H
#define CPM_EXPECTED_GRAD_H

#include "cpm_expected.h"

#ifdef __cplusplus
extern "C" {
#endif

/* enqueued on the context's stream.
 * d_pi0_or_null: DEVICE f64[Z]; NULL: uniform 1 / Z.  Read only.  flags: CPM_EXPECT_IVP or 0.
 * d_cotangent: DEVICE f64[2][T][Z], G_park then G_drv.  Read only.
 * d_gnext_or_null: DEVICE f64[Z], the cotangent of pi_next; NULL: zeros.  Read only.
 * d_grad_p_drive: DEVICE f64[T][Z]; every word written.
 * d_grad_pi0_or_null: DEVICE f64[Z]; every word written.  NULL: not wanted.
 * Nothing outside the two outputs is written. */
int32_t cpm_expected_grad_dev(cpm_ctx *ctx, const void *d_pi0_or_null, uint32_t flags, const void *d_cotangent, const void *d_gnext_or_null,
                              void *d_grad_p_drive, void *d_grad_pi0_or_null);

/* blocking.  pi0_or_null: borrowed host f64[Z] (CPM_ERR_ARG for a NaN, infinite or negative entry) or NULL.
 * g_parking / g_driving: Z x T Float64 column-major, the layout of the densities of the blocking density call.
 * g_next_or_null: host f64[Z].  grad_p_drive: Z x T Float64 column-major.  grad_pi0_or_null: host f64[Z]. */
int32_t cpm_expected_grad(cpm_ctx *ctx, const double *pi0_or_null, uint32_t flags, const double *g_parking, const double *g_driving,
                          const double *g_next_or_null, double *grad_p_drive, double *grad_pi0_or_null);

#ifdef __cplusplus
}
#endif
#endif
