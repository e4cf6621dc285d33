/*
 * cpm_expected_sparse_var.h -- the exact seed variances of count and travel functionals (cpm_expected_linear_var.h,
 * cpm_expected_travel_var.h) straight from the compact rows of sparse p_destin tables: the part of the noise-free family that
 * the earlier sparse headers (the densities, the adjoint, the e_dest direction, the forward tangent) left to the dense
 * array.  (cpm_expected_var carries the dense Z x Z matrix P_t whatever the tables are, and has no sparse form.)
 *
 * Contract: every output word of every call below carries the bits of its dense namesake on the same tables.  The calls never read,
 * build or keep the dense [T][Z][Z] p_destin array or any other Z x Z array (CPM_INFO_P_DENSE stays 0), and they change no state a
 * later call reads: a resample, a dense variance call or a call of any other family gives what it would have given without them.
 *
 * Why the bits are those of the dense call.  One backward operator of either recurrence needs, for origin o, three sums along o's OWN
 * row of the table, which is what the compact rows store, sorted by destination:
 *   s1 = sum p * zeta,   s2 = sum (p * zeta) * zeta,   b = sum p * nu[d],
 * zeta[d] = mu[d] - mu[o] for the count functionals and (mu[d] - mu[o]) + (S[o] * sec(o, d, t) + D[o] * km(o, d)) with travel.  The
 * dense kernels fix the order of each sum as the adjoint's product does (the header of cpm_expected_sparse_grad has the same argument):
 *   nseg = grad_segments(Z), seg_len = ceil(Z / nseg); destination d belongs to segment s = d / seg_len and to chain
 *   v = (d - s * seg_len) & 3, i.e. (d - begin) mod 4; a chain starts at +0.0 and adds acc = acc + term in ascending d; the four
 *   chains of a segment are added as ((c0 + c1) + c2) + c3; the finishing kernel adds the segments in ascending order and then the
 *   residual terms.
 * A cell with p = 0 contributes p * zeta = +-0, (p * zeta) * zeta = +-0 and p * nu = +-0 as long as zeta and nu are finite; a chain
 * that starts at +0.0 and is +0.0 or non-zero after every step never becomes -0.0 (+0 + -0 = +0, exact cancellation rounds to +0), so
 * adding +-0 to it changes nothing.  So giving only the STORED cells with d < Z to their chains, in ascending d, changes no bit, and
 * chains and segments without cells are +0.0 -- the empty trailing segment of sizes like Z = 1,089 (nseg = 34, seg_len = 33) included.
 * The term of a stored cell is formed by the dense kernel's own operations, one IEEE operation each: e = mu[d] - mu[o]; t = p * e;
 * t, t * e, p * nu[d].  The centring at mu[o] stays inside the term: sum p * mu - mu[o] * sum p is a different rounding and loses the
 * exact 0 of a functional that is constant over the zones.  The finishing kernels and the totals are the dense calls' own, fed l and
 * r of cpm_expected_sparse.h, which are word for word the dense builder's.  The order does not depend on K, on a functional's place
 * in the call or on how many functionals share a pass over the rows: functional k of K carries the bits of a K = 1 call.
 *
 * The trip variance weight v_sec[t][o] follows the same scheme over trip_segments(Z, T) segments with the term
 * p * (d == o ? 0.0 : var_sec(o, d, t)), as the sparse trip weights follow theirs, and the dense call's finishing kernel.
 *
 * Preconditions.
 *   (all calls) The state stays finite: mu and nu of every operator.  The blocking calls refuse non-finite coefficients, as their
 *   namesakes do; the _dev calls do not check, and there 0 * inf = NaN of a cell that is not stored would differ from the dense call.
 *   (travel and trip_var calls) At every cell that is NOT stored, the mean word, the distance and var_sec(mean word, std word) must
 *   be finite.  The dense kernel forms 0 * that word there; the sparse calls never see it.  Negative and zero means are fine.
 *   var_sec (etv_var_sec in csrc/cpm_expected_travel_var.h), with sd = 0.1 * mean where the std word is == 0 and the std word
 *   otherwise, is 0 -- finite -- wherever !(sd > 0), which covers a NaN mean or std word, a mean <= 0 with a std word of 0 and a
 *   negative std word, and wherever the mass E = det_erf(a / sqrt 2), a = (0.1 * mean) / sd, is not > 0, which covers a <= 0 and a
 *   NaN (a mean of +inf with a std word of 0 or +inf: inf / inf) and a = 0 (a std word of +inf with a finite mean).  It is NOT finite
 *   in exactly two cases, both with sd > 0:
 *     a == +inf -- a mean word of +inf with a finite std word > 0, or a finite quotient that overflows (mean 1e300, std 1e-300):
 *       v forms (inf * c) * exp_neg(inf) = inf * 0 = NaN;
 *     (sd * v(a)) * sd overflows -- v(a) <= 1, so only for sd >= 2^511 (about 6.7e153): +inf.
 *   Every other pair of words gives a finite var_sec -- among them every pair with |mean| < 2^511 and a std word that is 0, negative
 *   or between 0.1 * |mean| * 2^-1022 and 2^511.
 *   Where a precondition fails, the sparse call returns the value without that cell's NaN; it still changes nothing a later dense
 *   call returns.
 *
 * Caches.  The sparse v_sec lives in a cache of its own behind the sparse trip weights, as the dense one lives behind the dense
 * trip weights: built on first use and again on first use after anything that rebuilds the sparse trip weights (a new datamatrix,
 * new distances, new p_destin tables).  cpm_expected_sparse_trip_var_builds counts its builds; cpm_expected_trip_var_builds counts
 * dense builds only.  A sparse call changes nothing that a later dense call returns, and a dense call nothing that a later sparse
 * call returns.
 *
 * Argument lists, layouts, flags and status codes are those of the namesakes, with the two additions of cpm_expected_sparse.h:
 *   CPM_ERR_STATE when the installed p_destin tables have no compact rows; cpm_last_error() names the two routes that produce them;
 *   CPM_ERR_TABLE for a non-zero row whose total exceeds 1 + Z * 2^-52, with the text, the hour and the origin of the dense call.
 * Without a usable device every entry returns CPM_ERR_HIP.
 */
#ifndef CPM_EXPECTED_SPARSE_VAR_H
#define CPM_EXPECTED_SPARSE_VAR_H

#include "cpm_expected_linear_var.h"
#include "cpm_expected_travel_var.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cpm_expected_linear_var_dev / cpm_expected_linear_var from the compact rows */
int32_t cpm_expected_sparse_linear_var_dev(cpm_ctx *ctx, const void *d_start_or_null, uint32_t flags, int32_t K, const void *d_coeff, void *d_out,
                                           void *d_zone_or_null);
int32_t cpm_expected_sparse_linear_var(cpm_ctx *ctx, const double *start_or_null, uint32_t flags, int32_t K, const double *a_parking,
                                       const double *b_driving, double *mean, double *var, double *zone_mean_or_null, double *zone_var_or_null);

/* cpm_expected_trip_var_dev / cpm_expected_trip_var from the compact rows, and the builds of that cache (negative: a status code) */
int32_t cpm_expected_sparse_trip_var_dev(cpm_ctx *ctx, void *d_v);
int32_t cpm_expected_sparse_trip_var(cpm_ctx *ctx, double *v_sec);
int64_t cpm_expected_sparse_trip_var_builds(const cpm_ctx *ctx);

/* cpm_expected_travel_var_dev / cpm_expected_travel_var from the compact rows and the sparse v_sec */
int32_t cpm_expected_sparse_travel_var_dev(cpm_ctx *ctx, const void *d_start_or_null, uint32_t flags, int32_t K, const void *d_coeff, void *d_out,
                                           void *d_zone_or_null);
int32_t cpm_expected_sparse_travel_var(cpm_ctx *ctx, const double *start_or_null, uint32_t flags, int32_t K, const double *a_parking,
                                       const double *b_driving, const double *s_seconds_or_null, const double *d_km_or_null, double *mean, double *var,
                                       double *zone_mean_or_null, double *zone_var_or_null);

#ifdef __cplusplus
}
#endif
#endif
