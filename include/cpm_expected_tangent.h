/*
 * cpm_expected_tangent.h -- the forward tangent of the expected densities of libcpm_hip.so: how cpm_expected's parking and driving
 * densities move, per zone and hour, in K directions of (pi_0, p_drive, p_destin) at once -- K columns of the Jacobian of the
 * densities, where cpm_expected_grad.h gives the gradient of one scalar.  With the three direction tables d p_drive / d (p_min, p_max,
 * e_drive), built on the device, and the tangent d p_destin / d e_dest of cpm_expected_grad_dest.h, the columns are those of the
 * model's four parameters: what a Gauss-Newton step on the noise-free objectives needs.
 *
 * Terms are those of cpm_expected.h, cpm_expected_grad.h and cpm_expected_grad_dest.h: q, p[t][d][o] = p_destin[o, d, t], last, l, r,
 * zero rows, the operators s = 0 .. N-1 with their hours t(s), pi_s, x = pi * q (the PRIMAL), the tangent table dP of the context.
 *
 * Direction k = (d pi_0 = dpi0[k][.] or 0, dp_drive = dp_drive[k][.][.] or 0, c_dest[k]): the densities' derivative at eps = 0 under
 *   pi_0 + eps * d pi_0,   p_drive + eps * dp_drive,   p_destin + eps * c_dest[k] * dP.
 *
 * Definition, for operator s of hour t and direction k.  Every step is ONE IEEE f64 operation, in the order written (the library is
 * built with -ffp-contract=off):
 *   dq[o]   = dp_drive[k][t][o] where the installed p_drive[o, t] is strictly inside (0, 1); elsewhere exactly 0, whatever the
 *             direction holds there (NaN included) -- the rule of cpm_expected_grad.h: q is flat there;
 *   dx[o]   = dpi[o] * q[o] + pi[o] * dq[o]              (two products, then their sum);
 *   dstay[o] = dpi[o] * (1 - q[o]) - pi[o] * dq[o]       (1 - q, two products, then their difference);
 *   outputs of the day's operators: d parking = dpi, d driving = dx;
 *   dpi_next[d] = ((dstay[d] + y[d]) + res[d])  + dx[d] for a zero row  + c_dest[k] * u[d] when c_dest[k] != 0   (in that order),
 *   y[d] and res[d] being the sums of cpm_expected.h with dx in place of x: over o of dx[o] * p[o, d], and of the residuals
 *   dx[o] * r[o] that arrive at d;
 *   u[d]    = the sum over o of x[o] * dP[t][d][o], x the PRIMAL pi * q; NO residual term, and the origins of zero rows contribute 0
 *             whatever the table holds there.  r and l are held fixed: the convention of cpm_expected_grad_dest.h, whose paragraph
 *             "Meaning" carries over -- for a tangent whose rows sum to 0 (d / d e_dest among them) this is the derivative of the exact
 *             law.
 * u is computed ONCE per operator and shared by all directions; it is not computed, and dP not read, when every c_dest is 0 or c_dest
 * is NULL.  Under CPM_EXPECT_IVP the operators in front of the day propagate the tangent like the primal.
 *
 * Order of the sums.  y, res and u have the order documented in cpm_expected.h (u that of y, over the row of dP).  No floating-point
 * atomics.  Nothing depends on K, on k or on how directions were dealt to passes: direction k gives the same bits alone as among 16;
 * the same inputs give the same bits every time; expected (the primal, when asked for) carries the BITS of cpm_expected_dev on the same
 * inputs.  Every word of the outputs is written and nothing else; nothing that a later cpm_expected*, gradient, fit or resample call
 * reads is changed.
 *
 * How it runs.  One launch per operator and pass; the primal rides as vector 0 of a pass and up to 7 directions as vectors 1 .. 7, so
 * the hour's Z x Z block of p is read once for the primal and seven tangents.  K > 7 takes further passes, which recompute the primal
 * with the same bits.  u is one more one-vector pass over the rows of dP in the workgroups of an operator's first pass.
 *
 * Error bound, derived (not measured).  Terms are signed, so the bound is relative to a MAGNITUDE: the recurrence above evaluated
 * exactly with |dpi_0|, |dq|, |c_dest|, |dP| in place of the signed values, the exact pi and q, and every difference an addition
 * (dstay~ = dpi~ * (1 - q) + pi * dq~).  It bounds the absolute value of every partial sum the device forms.
 *   Count, in roundings of 2^-53 relative to the magnitude, along the longest way of a term through ONE operator:
 *     dx: a product and the sum                                        2
 *     the product dx * p                                                1
 *     the sum y: Z terms, whatever the order                            Z - 1
 *     (dstay + y), + res, + dx of a zero row, + c * u                   4
 *   -- Z + 6.  The other ways are shorter: through dstay 1 - q, a product, the difference and the 4 additions (7); through res as
 *   through y with the list's sum (at most Z + 6); through u the primal product pi * q, the product with dP, Z - 1 additions, the product
 *   with c and the last addition (Z + 2).  A term that enters from the primal (pi * dq, x * dP) carries the primal's error: after s
 *   operators pi lies within s * (Z + 8) * 2^-52 (cpm_expected.h): Z + 8 units of 2^-52 per operator behind it, where the tangent's own
 *   operators cost (Z + 6) / 2.  So every way of h operators from pi_0 and d pi_0 to a word of dpi collects at most h * (Z + 8) units
 *   of 2^-52 to first order; the products of these errors are below h * 2^-52 while h * (Z + 8) < 2^25, and one unit per operator
 *   more covers them:
 *     a word of d parking after h operators lies within   (c1 * h * (Z + c2)) * 2^-52 * magnitude,   c1 = 1, c2 = 10,
 *     a word of d driving (dx: two more roundings) within (h * (Z + 10) + 2) * 2^-52 * magnitude,
 *   and dpi_next is a d parking word after h = N operators.  A word whose magnitude is 0 is exactly 0.
 *
 * The direction tables of p_drive.  cpm_build_p_drive_tangent[_dev] builds d p_drive / d (p_min, p_max, e_drive) at the given point
 * from the resident mean_sum of cpm_build_p_drive, with the s = (mean_sum - mn) / (mx - mn), the power s^e (sqrt, identity and the
 * square at e_drive = 0.5, 1, 2) and the log of the chain rule in cpm_expected_fit.h.  Each entry ONE f64 operation per step:
 *   d / d p_min = 1 - s^e;   d / d p_max = s^e;   d / d e_drive = (p_max - p_min) * (s^e * ln s), 0 where s <= 0;
 *   all three 0 where mx[z] <= 0 (the zone's p_drive is 0 whatever the parameters).
 * The constants of cpm_expected_fit.h hold: 16 ulp for the power, 4 for ln.
 *
 * Workspace of the context, in f64 words with Zs = Z rounded up to even and P = ceil(K / 7): 32 * P * Zs + 3 * Zs; the blocking forms
 * keep their device arrays besides (3 * K * T * Z + 2 * T * Z + (2 * K + 1) * Z).  It only grows.
 *
 * Status codes, every refusal before anything is enqueued: CPM_ERR_HIP without a usable device; CPM_ERR_ARG: a null context, K outside
 * 1 .. CPM_TANGENT_MAX_DIRECTIONS, NULL tangent outputs, unknown flag bits (CPM_EXPECT_IVP is the only flag), a c_dest that is not
 * finite, and in the blocking form a word of pi0 (as in cpm_expected), dpi0 or dp_drive that is not finite, or only one of parking /
 * driving; CPM_ERR_STATE: no p_drive or p_destin tables, a non-zero c_dest without a tangent (cpm_set_p_dest_tangent or
 * cpm_build_p_dest_tangent since the tables were last installed), cpm_build_p_drive_tangent* without a datamatrix and distance matrix;
 * CPM_ERR_TABLE for a row total above 1.  The calls read the INSTALLED p_drive and p_destin; the fleets of the batch tables are out of
 * scope.  Conventions are those of cpm.h: int32 status, cpm_last_error(), no abort across the boundary, borrowed column-major host
 * arrays.
 */
#ifndef CPM_EXPECTED_TANGENT_H
#define CPM_EXPECTED_TANGENT_H

#include "cpm_expected_grad_dest.h"

#define CPM_TANGENT_MAX_DIRECTIONS 16 /* K of one call */

#ifdef __cplusplus
extern "C" {
#endif

/* enqueued on the context's stream.  K = 1 .. CPM_TANGENT_MAX_DIRECTIONS.  flags: CPM_EXPECT_IVP.
 * d_pi0_or_null: DEVICE f64[Z]; NULL: uniform 1 / Z.  d_dpi0_or_null: DEVICE f64[K][Z]; d_dp_drive_or_null: DEVICE f64[K][T][Z]; NULL: zero.
 * c_dest: host f64[K], copied at the call, or NULL (zero).  All read only.
 * d_out: DEVICE f64[K][2][T][Z], per direction d parking then d driving; every word written.
 * d_dpi_next_or_null: DEVICE f64[K][Z], the tangent of pi after the day's last operator.
 * d_expected_or_null: DEVICE f64[2][T][Z], the primal: the bits of cpm_expected_dev. */
int32_t cpm_expected_tangent_dev(cpm_ctx *ctx, int32_t K, const void *d_pi0_or_null, uint32_t flags, const void *d_dpi0_or_null,
                                 const void *d_dp_drive_or_null, const double *c_dest, void *d_out, void *d_dpi_next_or_null, void *d_expected_or_null);

/* blocking.  pi0_or_null: borrowed host f64[Z] or NULL.  dpi0_or_null: Z x K, dp_drive_or_null: Z x T x K Float64 column-major.
 * d_parking, d_driving: Z x T x K Float64 column-major, the layout of cpm_expected_batch with K where that call has B.
 * dpi_next_or_null: Z x K.  parking_or_null, driving_or_null: Z x T, the primal (both or neither). */
int32_t cpm_expected_tangent(cpm_ctx *ctx, int32_t K, const double *pi0_or_null, uint32_t flags, const double *dpi0_or_null,
                             const double *dp_drive_or_null, const double *c_dest, double *d_parking, double *d_driving, double *dpi_next_or_null,
                             double *parking_or_null, double *driving_or_null);

/* enqueued on the context's stream.  d_out: DEVICE f64[3][T][Z], d / d p_min, d / d p_max, d / d e_drive; every word written.
 * The context's own p_drive and the batch tables are not touched. */
int32_t cpm_build_p_drive_tangent_dev(cpm_ctx *ctx, double p_min, double p_max, double e_drive, void *d_out);

/* blocking.  out: three Z x T Float64 column-major arrays, one behind the other. */
int32_t cpm_build_p_drive_tangent(cpm_ctx *ctx, double p_min, double p_max, double e_drive, double *out);

#ifdef __cplusplus
}
#endif
#endif
