/*
 * cpm_expected_fit.h -- value and four-parameter gradient of the noise-free objectives of libcpm_hip.so: from B parameter points
 * (p_min, p_max, e_drive; e_dest is the installed p_destin's) to a record of CPM_FIT_WORDS + T words per point in ONE enqueued call,
 * with ONE forward propagation and nothing reduced on the host.
 *
 * What the call does, all on the context's stream:
 *   (a) installs the B p_drive tables exactly as cpm_build_p_drive_batch does (the same kernel, the same bits).  THE BATCH TABLES HOLD
 *       THESE POINTS AFTERWARDS; the context's own p_drive is not touched;
 *   (b) runs the forward propagation of cpm_expected_grad_batch_dev once, pi_s of every operator kept, and forms the densities of the
 *       day: parking[j] = pi_{pre+j}, driving[j] = pi_{pre+j} * q_j (ONE multiplication) -- the bits of cpm_expected_batch_dev;
 *   (c) forms the objectives and the cotangent of F (below);
 *   (d) runs the backward pass of cpm_expected_grad_batch_dev (under CPM_FIT_DEST: of cpm_expected_grad_dest_batch_dev) on that
 *       cotangent, with G_next zero and grad_pi0 not wanted;
 *   (e) reduces grad_p_drive (and grad_dest) to dF/dp_min, dF/dp_max, dF/de_drive (and dF/de_dest) by the chain rule.
 *
 * Definitions.  Every step is ONE IEEE f64 operation, in the order written (the library is built with -ffp-contract=off).  n = (double)T.
 * Per fleet, with weights (w_act, w_park, w_adrive), p[t][z] = parking, x[t][z] = driving:
 *
 * Traffic activity.  a[t] = sum over z of x[t][z] (ZONE SUM, below).  lo / hi = the minimum / maximum of a over t, imin / imax the
 * FIRST hour that attains it (t ascending, strict comparisons).  range = hi - lo.  range != 0:
 *   traffic_activity[t] = v[t] = (a[t] - lo) / range;
 *   with measured activity m: for t = 0 .. T-1: d = v[t] - m[t], acc = acc + d*d, e[t] = (2*d) / n, s1 = s1 + e[t]*(1 - v[t]),
 *   s2 = s2 + e[t]*v[t], g[t] = e[t] / range; activity_error = acc / n; then g[imin] = g[imin] - s1/range, g[imax] = g[imax] - s2/range
 *   (in that order; imin != imax since range != 0); then ga[t] = w_act * g[t].
 * range == 0 (a flat activity): traffic_activity[t] = NaN, activity_error = NaN, ga[t] = 0.  Without measured activity:
 * activity_error = NaN, ga = 0.
 *
 * Parking error.  Per zone lo / hi / imin / imax of p[.][z] over t as above.  A zone is measured as cpm_objectives.h defines it, flat
 * when lo == hi, valid when measured and not flat (no measured parking installed: no zone is valid).  For a valid zone, range = hi - lo,
 * for t = 0 .. T-1: v = (p[t][z] - lo) / range, d = v - m[t][z], acc = acc + d*d, e = (2*d) / n, s1 = s1 + e*(1 - v), s2 = s2 + e*v;
 * e_z = acc / n -- the definition of cpm_objectives.h with densities in place of count / n.  n_valid = the number of valid zones;
 * parking_error = (ZONE SUM of e_z, 0.0 for a zone that is not valid) / (double)n_valid, NaN when n_valid == 0.
 * Cotangent of a valid zone: g = e / range; if t == imin: g = g - s1/range; if t == imax: g = g - s2/range; g = g / (double)n_valid;
 * G_park[t][z] = w_park * g.  A zone that is not valid, w_park == 0 or n_valid == 0: G_park = 0.
 *
 * A_drive = total_seconds / (n * 3600), total_seconds and total_km being the totals of cpm_expected_travel_dev on the densities just
 * formed, bit for bit.
 *
 * F = the sum of w * value over the terms whose weight is != 0, in the order act, park, adrive, starting from 0.  A term with weight 0
 * is not formed: a NaN parking_error does not reach F unless it is weighed.
 *
 * Cotangent, DEVICE f64[B][2][T][Z] (G_park then G_drv, the layout of cpm_expected_grad_batch_dev): G_park as above;
 *   G_drv[t][z] = 0; if w_act != 0: G_drv = ga[t]; if w_adrive != 0: G_drv = G_drv + w_adrive * (w_sec[t][z] / (n * 3600))
 * with w_sec the trip weights of cpm_expected_trip.  Every word is a fixed sequence of operations on the densities, except that a[t],
 * hence ga, and the ZONE SUM of e_z inside n_valid's scalar enter through a ZONE SUM.
 *
 * ZONE SUM.  The only sums whose order is not written above.  No floating-point atomics; the order is fixed by Z alone -- not by B,
 * the fleet's place or the run: blocks of 256 consecutive zones; inside a block four groups of 64, each reduced by the tree
 * v[l] = v[l] + v[l + o] for o = 32, 16, 8, 4, 2, 1 (absent zones are 0.0), the four groups then added in order ((g0 + g1) + g2) + g3;
 * the blocks' sums: lane l of 64 adds blocks l, l + 64, ... in ascending order from 0.0, then the same tree.  A sum of Z non-negative
 * terms formed this way is within (16 + ceil(Z / 16384)) * 2^-53 (relative) of the exact sum.
 *
 * Chain rule.  s[t][z] = (mean_sum - mn) / (mx - mn) recomputed from the context's mean_sum as cpm_build_p_drive forms it, s^e by the
 * same power function (sqrt, identity and the square at e_drive = 0.5, 1, 2).  Over the words i = t * Z + z of [T][Z] with
 * grad_p_drive[i] != 0 and mx[z] > 0:
 *   dF/dp_min = sum g * (1 - s^e);  dF/dp_max = sum g * s^e;  dF/de_drive = sum (g * (p_max - p_min)) * (s^e * ln s), 0 at s <= 0.
 * Under CPM_FIT_DEST: dF/de_dest = sum grad_dest; where w_adrive != 0 the direct term through the trip weights is added:
 * + w_adrive * (sum(x * dw_sec) / (n * 3600)), dw_sec being the tangent of cpm_expected_trip_tangent (kept by the context while the
 * tangent table and the trip weights stay).  Without CPM_FIT_DEST word 8 is NaN.
 * These reductions are two-stage and fixed by Z and T alone: chunks of 1,024 consecutive words; thread i of 256 adds the chunk's words
 * i, i + 256, i + 512, i + 768 in that order from 0.0; the 256 partial sums go through the block tree of ZONE SUM; the chunks' sums as
 * the blocks' sums there.  Bound: each of words 5 .. 8 is within (96 + ceil(T * Z / 65536)) * 2^-53 * M of the exact value of its
 * definition on the same g, where M is the sum of the absolute values of its terms -- with s^e and 1 - s^e both counted as 1 for
 * words 5 and 6 (the term 1 - s^e cancels where s^e is near 1).  The constant holds 16 ulp for the power function and 4 for ln.
 *
 * Record per fleet, f64[CPM_FIT_WORDS + T], every word written:
 *   0 F   1 activity_error   2 parking_error   3 A_drive   4 n_valid (as f64)   5 dF/dp_min   6 dF/dp_max   7 dF/de_drive
 *   8 dF/de_dest (NaN without CPM_FIT_DEST)   9 total_seconds   10 total_km   11 .. CPM_FIT_WORDS-1 reserved, 0
 *   CPM_FIT_WORDS .. CPM_FIT_WORDS+T-1  traffic_activity[T]
 *
 * Contract of the optional outputs.  d_expected carries the bits of cpm_expected_batch_dev on the same tables; d_grad_p_drive (and
 * d_grad_dest) carry the bits of cpm_expected_grad[_dest]_batch_dev called with d_cotangent as its cotangent.  Fleet b's record and
 * slices do not depend on B, on b, or on how fleets were dealt to passes; the same inputs give the same bits every time.  Nothing
 * that a later cpm_expected*, gradient or resample call reads is changed, except the batch tables (a).
 *
 * Workspace of the context beyond that of cpm_expected_grad_batch.h, in f64 words with nz = ceil(Z / 256), nc = ceil(T * Z / 1024):
 *   B * 6 * T * Z  (densities [B][2][T][Z], cotangents [B][2][T][Z], grad_p_drive and grad_dest [B][T][Z] each -- also where the caller
 *   passes its own) + 5 * B * Z + 2 * Z + B * (T * nz + nz + 5 * nc + T + 9), and B * (Z + nz) 32-bit words; 2 * T * Z for the trip
 *   weights' tangent once a call needs it.  It only grows.
 *
 * Bounds of the shapes: T <= 2,048; B = 1 .. CPM_MAX_BATCH (B = 1 is the single-point form).
 *
 * Status codes, every refusal before anything is enqueued: those of the batch gradient calls (CPM_ERR_HIP without a device, ...);
 * CPM_ERR_ARG: NULL parameter arrays, NULL weights, NULL record, a weight that is not finite, unknown flag bits, B outside its range,
 * a grad_dest array without CPM_FIT_DEST, T above 2,048; CPM_ERR_STATE: no datamatrix or distance matrix, no p_destin tables, CPM_FIT_DEST without a
 * tangent, a non-zero w_act without measured activity, a non-zero w_park without measured parking.  Conventions are those of cpm.h.
 */
#ifndef CPM_EXPECTED_FIT_H
#define CPM_EXPECTED_FIT_H

#include "cpm_expected_grad_batch.h"

#define CPM_FIT_DEST 0x100u /* flags: also dF/de_dest, along the installed tangent of p_destin */
#define CPM_FIT_WORDS 16    /* words of a record in front of the traffic activity */

#ifdef __cplusplus
extern "C" {
#endif

/* activity_or_null: host f64[T], the measured traffic activity; uploaded and resident until it is replaced or the context is
 * destroyed; NULL: forget it.  A NaN or infinite word gives CPM_ERR_ARG and leaves what was installed.  Needs a context only.
 * Blocking (the array is borrowed for the call).  Measured parking densities are cpm_set_measured's (cpm_objectives.h). */
int32_t cpm_set_measured_activity(cpm_ctx *ctx, const double *activity_or_null);

/* enqueued on the context's stream; no synchronisation beyond what cpm_expected_grad_batch_dev does after the tables changed and what
 * cpm_build_p_drive_batch does when the batch tables grow.
 * p_min, p_max, e_drive: host f64[B], copied at the call.  weights: host f64[B][3], (w_act, w_park, w_adrive) per fleet, copied.
 * d_pi0_or_null: DEVICE f64[Z]; NULL: uniform 1 / Z.  Read only.  flags: CPM_EXPECT_IVP, CPM_FIT_DEST.
 * d_record: DEVICE f64[B][CPM_FIT_WORDS + T]; every word written.
 * d_expected_or_null, d_cotangent_or_null: DEVICE f64[B][2][T][Z]; d_grad_p_drive_or_null, d_grad_dest_or_null: DEVICE f64[B][T][Z];
 * every word written; NULL: kept in the workspace. */
int32_t cpm_expected_fit_dev(cpm_ctx *ctx, int32_t B, const double *p_min, const double *p_max, const double *e_drive, const void *d_pi0_or_null,
                             uint32_t flags, const double *weights, void *d_record, void *d_expected_or_null, void *d_cotangent_or_null,
                             void *d_grad_p_drive_or_null, void *d_grad_dest_or_null);

/* blocking.  pi0_or_null: borrowed host f64[Z] or NULL.  record: f64[B][CPM_FIT_WORDS + T].  expected_or_null, cotangent_or_null:
 * per fleet two Z x T Float64 column-major arrays (f64[B][2][T][Z]); grad_p_drive_or_null, grad_dest_or_null: Z x T x B column-major. */
int32_t cpm_expected_fit(cpm_ctx *ctx, int32_t B, const double *p_min, const double *p_max, const double *e_drive, const double *pi0_or_null, uint32_t flags,
                         const double *weights, double *record, double *expected_or_null, double *cotangent_or_null, double *grad_p_drive_or_null,
                         double *grad_dest_or_null);

#ifdef __cplusplus
}
#endif
#endif
