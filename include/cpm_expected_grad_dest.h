/*
 * cpm_expected_grad_dest.h -- the adjoint of the expected densities of libcpm_hip.so along a tangent of the p_destin tables: the
 * derivative of any differentiable objective of cpm_expected's densities in a direction dP of p_destin, per (origin, hour) row,
 * from the same backward pass as cpm_expected_grad.h; and the one tangent the model needs, d p_destin / d e_dest, built on the
 * device.  With it the noise-free objectives have a derivative for all four parameters of the model (e_drive, p_min, p_max, e_dest).
 *
 * Terms are those of cpm_expected.h and cpm_expected_grad.h: q, p[t][d][o] = p_destin[o, d, t], last, l, r, zero rows, the operators
 * s = 0 .. N-1 with their hours t(s), pi_s, the cotangents G and the adjoint mu that enters operator s of the backward pass.
 *
 * Tangent table.  One per context: dP, f64[T][Z dest][Z origin], the layout of the dense p_destin array.  It is allocated by the
 * first call that installs one (8 * Z * Z * T bytes: 3.2 GB at Z = 4,096, T = 24); a context that never asks pays nothing.
 * EVERY call that installs p_destin tables drops the tangent -- cpm_set_p_dest, cpm_build_p_dest, cpm_synth_tables* -- and so does a
 * new datamatrix (cpm_set_datamatrix, cpm_createdatamatrix_*, cpm_synth_datamatrix).
 *
 * cpm_build_p_dest_tangent builds dP = d p_destin / d e_dest at the e_dest of the last successful cpm_build_p_dest, from the resident
 * datamatrix and the installed tables.  Per (origin o, hour t), every step ONE IEEE f64 operation:
 *   x  = (mean - min_t) / (max_t - min_t) for pairs with max_t > 0, the value createpdestin forms (src/createpdestin.jl:10-28);
 *   l  = log(x), the device's f64 log;
 *   m  = the sum over the cells with installed p > 0 of p * l, in ascending destination, starting from 0;
 *   dP = p * (l - m), p the INSTALLED f64 entry.
 * A cell with p == 0 is exactly 0; so are a zero row and a pair with max_t <= 0.  Both routes of cpm_build_p_dest are covered: on the
 * dense route x is recomputed from the datamatrix, on the compact-row route (CPM_INFO_SPARSE_TABLES != 0) it is the x the compact
 * rows keep per cell, the same f64 value.  This is the derivative of x^e / sum x^e in e, evaluated at the installed p; its rows sum
 * to 0 up to rounding.
 * Error bound of the builder: with n the number of cells of the row with p > 0 and m~ the sum of p * |l| over them, an entry lies
 * within
 *   (n + 8) * 2^-52 * p * (|l| + m~)
 * of the value the definition gives in exact arithmetic from the f64 x and the installed f64 p (n roundings of 2^-53 twice over for
 * m; the 8 covers the device log, 3 ulp by OpenCL's f64 limit that the device library is built to, and the two final operations).
 * CPM_ERR_STATE unless the installed p_destin came from cpm_build_p_dest on the datamatrix still resident, with e_dest > 0;
 * cpm_last_error() names what is missing.
 *
 * The adjoint along the tangent.  The arguments are those of cpm_expected_grad[_dev] plus one output, grad_dest[T][Z].  For operator s
 * of hour t, with the mu that enters it:
 *   w[o]           = the sum over d of dP[t][d][o] * mu[d]    (0 for a zero row; NO residual term);
 *   grad_dest_s[o] = (pi_s[o] * q[o]) * w[o];
 *   grad_dest[t][o] = the sum of grad_dest_s[o] over the operators with t(s) = t: the day's term, then the IVP's added to it, as for
 *   grad_p_drive.  Where mu is zero by construction (the last operator without G_next) the product is skipped and the term is 0.
 * Segments, chains and order of the sum w are exactly those documented for a in cpm_expected_grad.h, without the residual term.
 *
 * Meaning.  dL/dp_destin[o, d, t] = x_s[o] * mu[d] summed over the operators of hour t, x_s = pi_s * q: rank one.  grad_dest[t][o] is
 * the derivative of L along dP restricted to row (o, t), at FIXED r and l: the residual r = max(0, 1 - last) that the sampler gives
 * to the last destination is held where it is.  For a tangent whose rows sum to 0 -- every normalised family, d / d e_dest among them
 * -- that is the derivative of the exact law.  The sum of grad_dest over all rows is the derivative of L along dP.
 *
 * grad_p_drive and grad_pi0 of these calls carry the bits of cpm_expected_grad_dev on the same inputs.  No floating-point atomics;
 * the same inputs give the same bits every time; every word of the outputs is written and nothing else; no state that a later
 * cpm_expected* call or resample reads is changed.  The workspace of cpm_expected_grad grows by the segments' sums of w.  These calls read the
 * installed p_drive; the fleets of the batch tables have cpm_expected_grad_batch.h.
 *
 * Error bound, relative to the magnitude recurrence of cpm_expected_grad.h with |dP| in place of dP: w~[o] = the sum over d of
 * |dP[t][d][o]| * mu~[d], W~_s[o] = x_s[o] * w~[o].  mu enters operator s after n - 1 = N - s - 1 backward operators: within
 * (n - 1) * K * 2^-52 * mu~ (K of cpm_expected_grad.h).  A product dP * mu[d] passes one multiplication and at most
 * ceil(ceil(Z / S) / 4) + 3 + S - 1 additions, fewer than the R = K / 2 roundings of 2^-53 behind a term of lambda, so w lies within
 * ((n - 1) * K + K / 4) * 2^-52 * w~.  pi_s lies within s * (Z + 8) * 2^-52 (cpm_expected.h); the two products add one 2^-52.
 * grad_dest_s therefore lies within
 *   (n * K + s * (Z + 8) + 4) * 2^-52 * W~_s,    n = N - s,
 * the form of dq_s in cpm_expected_grad.h, and an entry of grad_dest within the sum of the bounds of its one or two terms (the + 4 of
 * each covers the addition of the two).  A word whose magnitude is 0 is 0.
 *
 * Tangent of the trip weights (cpm_expected_travel.h).  A_drive depends on p_destin through w_sec as well:
 *   dw_sec[t][o] = the sum over d of dP[t][d][o] * sec(o, d, t),   dw_km likewise with km(o, d),
 * with the values of cpm_expected_trip (diagonal 300 s and 1 km, the mean word, the distance) in that call's documented order of sums;
 * no residual term, 0 for a zero row.  Bound: (Z / 4 + 16) * 2^-52 times the sum of |dP| * |value|.  Needs a datamatrix and a
 * distance matrix (CPM_ERR_STATE).
 *
 * Status codes.  CPM_ERR_STATE without a tangent (cpm_set_p_dest_tangent or cpm_build_p_dest_tangent since the tables were last
 * installed); every other status as in cpm_expected_grad: CPM_ERR_STATE without p_drive or p_destin tables, CPM_ERR_TABLE for a row
 * total above 1, CPM_ERR_HIP without a usable device, CPM_ERR_ARG for NULL cotangents or outputs, unknown flag bits (refused before
 * anything is enqueued), a cotangent word that is not finite in the blocking form, and a tangent entry that is not finite in
 * cpm_set_p_dest_tangent.  Conventions are those of cpm.h: int32 status, cpm_last_error(), no abort across the boundary, borrowed
 * column-major host arrays.
 */
#ifndef CPM_EXPECTED_GRAD_DEST_H
#define CPM_EXPECTED_GRAD_DEST_H

#include "cpm_expected_grad.h"

#ifdef __cplusplus
extern "C" {
#endif

/* dp: borrowed host Z x Z x T Float64 column-major, [origin, destination, hour]: the layout of cpm_set_p_dest.  Blocking.
 * Needs installed p_destin tables (CPM_ERR_STATE). */
int32_t cpm_set_p_dest_tangent(cpm_ctx *ctx, const double *dp);

/* d p_destin / d e_dest of the installed tables, on the device.  out_or_null: host Z x Z x T Float64 column-major, or NULL (the
 * call then returns as soon as the kernels are enqueued on the context's stream). */
int32_t cpm_build_p_dest_tangent(cpm_ctx *ctx, double *out_or_null);

/* out: host Z x Z x T Float64 column-major.  Blocking. */
int32_t cpm_get_p_dest_tangent(cpm_ctx *ctx, double *out);

/* enqueued on the context's stream.  Arguments as cpm_expected_grad_dev, and
 * d_grad_dest: DEVICE f64[T][Z]; every word written. */
int32_t cpm_expected_grad_dest_dev(cpm_ctx *ctx, const void *d_pi0_or_null, uint32_t flags, const void *d_cotangent, const void *d_gnext_or_null,
                                   void *d_grad_p_drive, void *d_grad_pi0_or_null, void *d_grad_dest);

/* blocking.  Arguments as cpm_expected_grad, and grad_dest: Z x T Float64 column-major. */
int32_t cpm_expected_grad_dest(cpm_ctx *ctx, const double *pi0_or_null, uint32_t flags, const double *g_parking, const double *g_driving,
                               const double *g_next_or_null, double *grad_p_drive, double *grad_pi0_or_null, double *grad_dest);

/* enqueued on the context's stream.  d_dw: DEVICE f64[2][T][Z], dw_sec then dw_km; every word written. */
int32_t cpm_expected_trip_tangent_dev(cpm_ctx *ctx, void *d_dw);

/* blocking.  dw_sec, dw_km: Z x T Float64 column-major. */
int32_t cpm_expected_trip_tangent(cpm_ctx *ctx, double *dw_sec, double *dw_km);

#ifdef __cplusplus
}
#endif
#endif
