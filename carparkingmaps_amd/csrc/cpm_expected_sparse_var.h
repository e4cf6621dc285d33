// cpm_expected_sparse_var.h -- the backward products of the seed variances and the trip variance weights from the compact rows of
// sparse p_destin tables (include/cpm_expected_sparse_var.h): k_exps_elv_u<NB>, k_exps_etv_u<NB>, k_exps_trip_var.
//
// The three sums of one backward operator of cpm_expected_linear_var.h / cpm_expected_travel_var.h,
//   s1 = sum p * zeta,   s2 = sum (p * zeta) * zeta,   b = sum p * nu[d],
// run along origin o's OWN row of the table, which is what d_sp / d_sj / d_scnt store, sorted by destination.  k_elv_u and k_etv_u fix
// the order: destination d belongs to segment s = d / seg_len (grad_segments) and to chain (d - s * seg_len) & 3, the wave of the dense
// kernel that is dealt d; a chain starts at +0 and adds in ascending d; the chains are added as ((c0 + c1) + c2) + c3.  A cell with
// p = 0 adds +-0 to each of the three sums for finite zeta and nu, and a chain that starts at +0 never becomes -0: giving only the
// STORED cells to their chains changes no bit (cpm_expected_sparse_grad.h has the argument; exps_row_walk is its walk, used unchanged).
//
// One wave per origin row on exps_row_walk<3 * NB>: per stored cell and functional the three rounded products
//   e = mu[d] - mu[o];  t = p * e;  { t, t * e, p * nu[d] }                                        (k_elv_u's operations, one IEEE each)
//   z = (mu[d] - mu[o]) + (S[o] * sec + D[o] * km);  t = p * z;  { t, t * z, p * nu[d] }             (k_etv_u's)
// The centring stays inside the term: sum p * mu - mu[o] * sum p would break the bits and the exact 0 of a constant functional.
// mu[o], S[o] and D[o] are uniform over the wave and loaded once; the state line [2][NB] of destination d is gathered per cell (64
// bytes at NB = 4: one line).  sec and km are gathered from the dense mean plane and the distance matrix at the stored cells only,
// the diagonal a select per cell, as in k_exps_trip.  The kernels write every word part[s][kind][f][o], s < nseg, kind < 3, f < nf,
// o < Z, in the dense finishing kernels' layouts ([nseg][3][kElvNB][Zs] and [nseg][3][kEtvNB][Zs]): chains and segments without
// cells get +0, the empty trailing segment of sizes like Z = 1,089 included.  k_elv_finish, k_etv_finish and k_elv_total are the
// dense calls' own.
//
// k_exps_trip_var is exps_row_walk<1> over trip_segments with the term p * (d == o ? 0 : etv_var_sec(mean, std)), the mean and std
// words gathered at the stored cells only, all hours in one launch; k_exp_trip_var_finish follows unchanged.
//
// Pass sizes: those of the dense passes, NB = 4 (2, 1 for partial passes) for the counts and NB = 2 (1) for travel.  The walk keeps
// 4 * NV f64 accumulators per lane and NV * 64 doubles in LDS, NV = 3 * NB.  As compiled for gfx950 (the kernel-resource-usage
// remarks of `make asm`; VGPRs / scratch bytes per lane / LDS bytes per one-wave block / waves per SIMD):
//   k_exps_elv_u<1>   61 / 0 / 2,048 / 8     k_exps_elv_u<2>   97 / 0 / 3,584 / 4     k_exps_elv_u<4>  169 / 0 / 6,656 / 2
//   k_exps_etv_u<1>   63 / 0 / 2,048 / 8     k_exps_etv_u<2>   99 / 0 / 3,584 / 4     k_exps_trip_var   56 / 0 / 1,024 / 7
// No instantiation spills.  NB = 4 halves the rows in flight per SIMD against NB = 2 and reads the rows half as often; which wins is a
// measurement (profiles/expected_sparse_var_notes.md).  A functional's chains do not depend on NB or its slot: functional k of K carries the bits of a K = 1 call.
//
// Separate kernels in a header of their own: no existing kernel moves.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cpm_expected_sparse_grad.h"
#include "cpm_expected_travel_var.h"

namespace cpm {

#ifndef CPM_EXPS_ELV_NB
#define CPM_EXPS_ELV_NB 4  // (a measurement twin is built with -DCPM_EXPS_ELV_NB=2: tools/expected_sparse_var_bench.py)
#endif
constexpr int kExpsElvNB = CPM_EXPS_ELV_NB;  // functionals of a sparse count pass
static_assert((kExpsElvNB == 1 || kExpsElvNB == 2 || kExpsElvNB == 4) && kExpsElvNB <= kElvNB, "the instantiations, and the layout of part");

// grid = Z, one wave per origin.  sp_t / sj_t / scnt_t: the hour's rows.  st: the pass's [Zs][2][NB].  part: [nseg][3][kElvNB][Zs]
// (s1, s2, b); every word s < nseg, f < nf, o < Z is written.
template <int NB>
__global__ __launch_bounds__(kExpsGradBlock) void k_exps_elv_u(const double *__restrict__ sp_t, const uint32_t *__restrict__ sj_t,
                                                               const uint32_t *__restrict__ scnt_t, uint32_t cap, const double *__restrict__ st, int Z,
                                                               int Zs, int seg_len, int nseg, int nf, double *__restrict__ part)
{
    const size_t o = blockIdx.x;
    const uint32_t n = min(scnt_t[o], cap);
    double mo[NB];  // the row's own mu[o]: the sums are centred at it
#pragma unroll
    for (int f = 0; f < NB; ++f) mo[f] = st[o * 2 * NB + f];
    double sum[3 * NB];
    exps_row_walk<3 * NB>(sp_t + o * cap, sj_t + o * cap, n, static_cast<uint32_t>(Z), static_cast<uint32_t>(seg_len),
                          [st, &mo](uint32_t d, double pv, double (&prod)[3 * NB]) {
                              const double *__restrict__ srow = st + static_cast<size_t>(d) * 2 * NB;
#pragma unroll
                              for (int f = 0; f < NB; ++f) {
                                  const double m = srow[f], nu = srow[NB + f];
                                  const double e = m - mo[f];
                                  const double t = pv * e;
                                  prod[3 * f] = t;
                                  prod[3 * f + 1] = t * e;
                                  prod[3 * f + 2] = pv * nu;
                              }
                          },
                          sum);
    const int s = static_cast<int>(threadIdx.x);
    if (s < nseg) {
#pragma unroll
        for (int f = 0; f < NB; ++f)
            if (f < nf) {
#pragma unroll
                for (int k = 0; k < 3; ++k) part[((static_cast<size_t>(s) * 3 + k) * kElvNB + f) * Zs + o] = sum[3 * f + k];
            }
    }
}

// grid = Z, one wave per origin.  m_t: the hour's block of the mean plane, dist: [Z dest][Z origin], read at the stored cells only.
// cs / cd: the pass's first functional's S_k[j] / D_k[j] (cot_stride words apart), or nullptr in front of the day.
// part: [nseg][3][kEtvNB][Zs]; every word s < nseg, f < nf, o < Z is written.
template <int NB>
__global__ __launch_bounds__(kExpsGradBlock) void k_exps_etv_u(const double *__restrict__ sp_t, const uint32_t *__restrict__ sj_t,
                                                               const uint32_t *__restrict__ scnt_t, uint32_t cap, const double *__restrict__ m_t,
                                                               const double *__restrict__ dist, const double *__restrict__ st,
                                                               const double *__restrict__ cs, const double *__restrict__ cd, size_t cot_stride, int Z, int Zs,
                                                               int seg_len, int nseg, int nf, double *__restrict__ part)
{
    const uint32_t o = blockIdx.x;
    const uint32_t n = min(scnt_t[o], cap);
    double mo[NB], So[NB], Do[NB];  // the row's own mu[o], S[o], D[o]
#pragma unroll
    for (int f = 0; f < NB; ++f) {
        const int g = f < nf ? f : nf - 1;  // (slots nf .. NB - 1 repeat functional nf - 1; their sums are not written)
        mo[f] = st[static_cast<size_t>(o) * 2 * NB + f];
        So[f] = cs ? cs[static_cast<size_t>(g) * cot_stride + o] : 0.0;
        Do[f] = cd ? cd[static_cast<size_t>(g) * cot_stride + o] : 0.0;
    }
    double sum[3 * NB];
    exps_row_walk<3 * NB>(sp_t + static_cast<size_t>(o) * cap, sj_t + static_cast<size_t>(o) * cap, n, static_cast<uint32_t>(Z),
                          static_cast<uint32_t>(seg_len),
                          [st, m_t, dist, o, Z, &mo, &So, &Do](uint32_t d, double pv, double (&prod)[3 * NB]) {
                              const size_t cell = static_cast<size_t>(d) * Z + o;
                              const double mw = m_t[cell], kw = dist[cell];
                              const double sec = d == o ? kTripIntraSec : mw, km = d == o ? kTripIntraKm : kw;
                              const double *__restrict__ srow = st + static_cast<size_t>(d) * 2 * NB;
#pragma unroll
                              for (int f = 0; f < NB; ++f) {
                                  const double m = srow[f], nu = srow[NB + f];
                                  const double z = (m - mo[f]) + (So[f] * sec + Do[f] * km);
                                  const double t = pv * z;
                                  prod[3 * f] = t;
                                  prod[3 * f + 1] = t * z;
                                  prod[3 * f + 2] = pv * nu;
                              }
                          },
                          sum);
    const int s = static_cast<int>(threadIdx.x);
    if (s < nseg) {
#pragma unroll
        for (int f = 0; f < NB; ++f)
            if (f < nf) {
#pragma unroll
                for (int k = 0; k < 3; ++k) part[((static_cast<size_t>(s) * 3 + k) * kEtvNB + f) * Zs + o] = sum[3 * f + k];
            }
    }
}

// grid = (Z, T), one wave per row.  sp / sj / scnt: all rows [T][Z].  mean / sdev: [T][Z dest][Z origin], read at the stored cells
// only.  part: [nseg][T][Z]; every word written.
__global__ __launch_bounds__(kExpsGradBlock) void k_exps_trip_var(const double *__restrict__ sp, const uint32_t *__restrict__ sj,
                                                                  const uint32_t *__restrict__ scnt, uint32_t cap, const double *__restrict__ mean,
                                                                  const double *__restrict__ sdev, int Z, int T, int seg_len, int nseg,
                                                                  double *__restrict__ part)
{
    const uint32_t o = blockIdx.x;
    const size_t t = blockIdx.y, row = t * Z + o;
    const uint32_t n = min(scnt[row], cap);
    const double *__restrict__ m_t = mean + t * Z * Z;
    const double *__restrict__ s_t = sdev + t * Z * Z;
    double sum[1];
    exps_row_walk<1>(sp + row * cap, sj + row * cap, n, static_cast<uint32_t>(Z), static_cast<uint32_t>(seg_len),
                     [m_t, s_t, o, Z](uint32_t d, double pv, double (&prod)[1]) {
                         const size_t cell = static_cast<size_t>(d) * Z + o;
                         const double m = m_t[cell], sd = s_t[cell];
                         prod[0] = pv * (d == o ? 0.0 : etv_var_sec(m, sd));
                     },
                     sum);
    const int s = static_cast<int>(threadIdx.x);
    if (s < nseg) part[(static_cast<size_t>(s) * T + t) * Z + o] = sum[0];
}

}  // namespace cpm
