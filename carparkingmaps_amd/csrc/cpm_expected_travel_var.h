// cpm_expected_travel_var.h -- the exact seed variance of travel seconds, kilometres and count functionals of a resample
// (include/cpm_expected_travel_var.h): etv_var_sec, k_exp_trip_var<ODD>, k_exp_trip_var_finish, k_etv_u<NB, ODD>, k_etv_finish.
//
// The trip variance weight v_sec[t][o] = sum over d of p[t][d][o] * var_sec(o, d, t) depends on the tables alone: ONE launch of
// k_exp_trip_var covers all hours, in k_exp_trip's shape (strips of kTripStrip origins, trip_segments, the deal of a segment over
// the four waves, kTripUnroll destinations in flight).  It reads p, the mean plane and the std plane of the datamatrix once
// (non-temporal loads) and evaluates var_sec per cell from the f64 kit of cpm_rng.h (det_erf, exp_neg; no libm).
//
// One backward operator is two launches, as in cpm_expected_linear_var.h.  k_etv_u streams the hour's Z x Z block of p TOGETHER with
// the hour's mean plane once per pass of nf <= NB functionals, and reads the distance matrix with plain loads (it is read again by
// every hour and every pass and stays in the last-level cache, as in k_exp_trip).  The strips of kGradStrip origins, the destination
// segments of grad_segments, the deal of a segment over the four waves and the non-temporal 16-byte loads (two 8-byte loads for odd
// Z) are those of k_elv_u; the diagonal is a select per element.  Per functional a lane keeps, for each of its two origins, its own
// S[o], D[o] and mu[o] and the three sums of the recurrence,
//   s1 = sum p * zeta,   s2 = sum (p * zeta) * zeta,   b = sum p * nu[d],      zeta = (mu[d] - mu[o]) + (S[o] * sec + D[o] * km),
// per word of p and functional: three multiplications and two additions for zeta, three multiplications and three additions for the
// sums, each ONE IEEE operation, acc = acc + term in ascending d of the wave's deal, from 0.  The chain of a sum is the wave
// (d - begin) mod 4 whatever the unroll: with S = D = 0 and finite means and distances zeta is eta + 0 and every word is k_elv_u's.
//
// NB = kEtvNB = 2, kEtvUnroll = 4.  A lane holds 6 * NB accumulators (12 * NB VGPRs), its own S, D and mu (6 * NB doubles:
// 12 * NB VGPRs) and the unrolled loads of three arrays (kEtvUnroll x 6 doubles: 48 VGPRs): 96 VGPRs before addresses and temporaries,
// 120 as compiled for gfx950 (the kernel-resource-usage remark of `make asm`; 90 at NB = 1), no scratch -- four waves per SIMD, the four
// workgroups per CU that grad_segments sizes the grid for.  NB = 4 with the same unroll needs 144 VGPRs before temporaries and
// leaves three workgroups per CU at best; kGradUnroll = 8 destinations of three arrays in flight need 96 VGPRs for the loads alone.
// The instantiation NB = 1 serves a pass of one.  A functional's chain does not depend on NB or its slot: functional k of K carries
// the bits of a K = 1 call.
//
// The four waves are added through LDS in rounds of kGradRound accumulators, ((w0 + w1) + w2) + w3, as in k_elv_u.
//
// k_etv_finish has a lane per (origin, functional): the segments in ascending order starting from segment 0's sum, then the residual
// terms with zeta[l], the zero rows (a trip inside the zone), and db, J with (S * S) * v_sec, V and W.  The totals are k_elv_total's.
//
// Separate kernels in a header of their own: no existing kernel moves.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cpm_rng.h"
#include "cpm_expected_travel.h"
#include "cpm_expected_linear_var.h"

namespace cpm {

constexpr int kEtvNB = 2;      // functionals of a pass
constexpr int kEtvUnroll = 4;  // destinations of a wave in flight (three arrays each)
constexpr double kEtvSeriesMax = 1.0;  // v(a) by its series for a <= 1 (include/cpm_expected_travel_var.h)

// v(a), the variance of a standard normal truncated to +-a, given a > 0 and E = det_erf(a / sqrt 2) > 0.
// a <= 1, with y = a * a / 2: v = 2 y * N(y) / M(y), N = sum (-y)^m / ((2 m + 3) m!), M = sum (-y)^m / ((2 m + 1) m!), m = 0 .. 17,
// by Horner from m = 17 down (no cancellation: v -> a^2 / 3).  a > 1: v = 1 - (a * 0.79788456080286535588 * exp_neg(y)) / E.
__device__ __forceinline__ double etv_v(double a, double E)
{
    const double y = (a * a) * 0.5;
    if (a <= kEtvSeriesMax) {
        const double x = -y;
        double n = 1.0 / (37.0 * 355687428096000.0), m = 1.0 / (35.0 * 355687428096000.0);  // m = 17
        n = n * x + 1.0 / (35.0 * 20922789888000.0), m = m * x + 1.0 / (33.0 * 20922789888000.0);
        n = n * x + 1.0 / (33.0 * 1307674368000.0), m = m * x + 1.0 / (31.0 * 1307674368000.0);
        n = n * x + 1.0 / (31.0 * 87178291200.0), m = m * x + 1.0 / (29.0 * 87178291200.0);
        n = n * x + 1.0 / (29.0 * 6227020800.0), m = m * x + 1.0 / (27.0 * 6227020800.0);
        n = n * x + 1.0 / (27.0 * 479001600.0), m = m * x + 1.0 / (25.0 * 479001600.0);
        n = n * x + 1.0 / (25.0 * 39916800.0), m = m * x + 1.0 / (23.0 * 39916800.0);
        n = n * x + 1.0 / (23.0 * 3628800.0), m = m * x + 1.0 / (21.0 * 3628800.0);
        n = n * x + 1.0 / (21.0 * 362880.0), m = m * x + 1.0 / (19.0 * 362880.0);
        n = n * x + 1.0 / (19.0 * 40320.0), m = m * x + 1.0 / (17.0 * 40320.0);
        n = n * x + 1.0 / (17.0 * 5040.0), m = m * x + 1.0 / (15.0 * 5040.0);
        n = n * x + 1.0 / (15.0 * 720.0), m = m * x + 1.0 / (13.0 * 720.0);
        n = n * x + 1.0 / (13.0 * 120.0), m = m * x + 1.0 / (11.0 * 120.0);
        n = n * x + 1.0 / (11.0 * 24.0), m = m * x + 1.0 / (9.0 * 24.0);
        n = n * x + 1.0 / (9.0 * 6.0), m = m * x + 1.0 / (7.0 * 6.0);
        n = n * x + 1.0 / (7.0 * 2.0), m = m * x + 1.0 / (5.0 * 2.0);
        n = n * x + 1.0 / 5.0, m = m * x + 1.0 / 3.0;
        n = n * x + 1.0 / 3.0, m = m * x + 1.0;
        return ((2.0 * y) * n) / m;
    }
    const double g = ((a * 7.9788456080286535588e-1) * exp_neg(y)) / E;  // 2 a phi(a) / E, sqrt(2 / pi)
    return 1.0 - g;
}

// var_sec of a cell between different zones from its mean and std words (travel_time_q16's sigma; truncnormal_draw's exits)
__device__ __forceinline__ double etv_var_sec(double mu, double sd_word)
{
    const double sd = sd_word == 0 ? 0.1 * mu : sd_word;
    if (!(sd > 0.0)) return 0.0;
    const double a = (0.1 * mu) / sd;  // (truncnormal_mass's a)
    const double E = det_erf(a * 7.0710678118654752440e-1);
    if (!(E > 0.0)) return 0.0;
    return (sd * etv_v(a, E)) * sd;
}

// grid = (ceil(Z / kTripStrip), T, nseg).  part: [nseg][T][Z] the segments' sums; every word written.
template <bool ODD>
__global__ __launch_bounds__(kExpBlock) void k_exp_trip_var(const double *__restrict__ p, const double *__restrict__ mean, const double *__restrict__ sdev,
                                                            int Z, int T, int seg_len, double *__restrict__ part)
{
    __shared__ double s_acc[kExpWaves][2][64];
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int t = static_cast<int>(blockIdx.y), seg = static_cast<int>(blockIdx.z);
    const int o0 = static_cast<int>(blockIdx.x) * kTripStrip;
    const int oa = ODD ? o0 + lane : o0 + 2 * lane, ob = ODD ? oa + 64 : oa + 1;
    const bool in_a = oa < Z, in_b = ob < Z;  // (Z even: both or neither)
    const int d_begin = seg * seg_len, d_end = d_begin + seg_len < Z ? d_begin + seg_len : Z;
    const size_t plane = static_cast<size_t>(t) * Z * Z;
    const double *__restrict__ p_t = p + plane;
    const double *__restrict__ m_t = mean + plane;
    const double *__restrict__ s_t = sdev + plane;

    double va = 0.0, vb = 0.0;
    for (int d0 = d_begin + wave; d0 < d_end; d0 += kExpWaves * kTripUnroll) {
        double pa[kTripUnroll], pb[kTripUnroll], ma[kTripUnroll], mb[kTripUnroll], sa[kTripUnroll], sb[kTripUnroll];
#pragma unroll
        for (int u = 0; u < kTripUnroll; ++u) {
            const int d = d0 + u * kExpWaves;  // (uniform over the wave)
            pa[u] = pb[u] = ma[u] = mb[u] = 0.0;
            sa[u] = sb[u] = -1.0;  // (no cell: var_sec = 0)
            if (d < d_end) {
                const size_t row = static_cast<size_t>(d) * Z;
                if (ODD) {
                    if (in_a) {
                        pa[u] = __builtin_nontemporal_load(p_t + row + oa);
                        ma[u] = __builtin_nontemporal_load(m_t + row + oa);
                        sa[u] = __builtin_nontemporal_load(s_t + row + oa);
                    }
                    if (in_b) {
                        pb[u] = __builtin_nontemporal_load(p_t + row + ob);
                        mb[u] = __builtin_nontemporal_load(m_t + row + ob);
                        sb[u] = __builtin_nontemporal_load(s_t + row + ob);
                    }
                } else if (in_a) {
                    const exp_f64x2 pv = __builtin_nontemporal_load(reinterpret_cast<const exp_f64x2 *>(p_t + row + oa));
                    const exp_f64x2 mv = __builtin_nontemporal_load(reinterpret_cast<const exp_f64x2 *>(m_t + row + oa));
                    const exp_f64x2 sv = __builtin_nontemporal_load(reinterpret_cast<const exp_f64x2 *>(s_t + row + oa));
                    pa[u] = pv.x, pb[u] = pv.y, ma[u] = mv.x, mb[u] = mv.y, sa[u] = sv.x, sb[u] = sv.y;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kTripUnroll; ++u) {
            const int d = d0 + u * kExpWaves;
            if (d < d_end) {
                va = va + pa[u] * (d == oa ? 0.0 : etv_var_sec(ma[u], sa[u]));
                vb = vb + pb[u] * (d == ob ? 0.0 : etv_var_sec(mb[u], sb[u]));
            }
        }
    }
    s_acc[wave][0][lane] = va;
    s_acc[wave][1][lane] = vb;
    __syncthreads();
    // thread (i, l), i < 2: accumulator i of lane l over the four waves, in order
    const int i = tid >> 6, l = tid & 63;
    if (i < 2) {
        const double sum = ((s_acc[0][i][l] + s_acc[1][i][l]) + s_acc[2][i][l]) + s_acc[3][i][l];
        const int o = ODD ? o0 + l + 64 * i : o0 + 2 * l + i;
        if (o < Z) part[(static_cast<size_t>(seg) * T + t) * Z + o] = sum;
    }
}

// The segments in order, the residual term and the zero rows.  grid = (ceil(Z / 256), T).  v: [T][Z].
__global__ __launch_bounds__(kExpBlock) void k_exp_trip_var_finish(const double *__restrict__ part, int nseg, const double *__restrict__ mean,
                                                                   const double *__restrict__ sdev, const double *__restrict__ last,
                                                                   const int *__restrict__ ell, const double *__restrict__ r, int Z, int T,
                                                                   double *__restrict__ v)
{
    const int o = static_cast<int>(blockIdx.x) * kExpBlock + static_cast<int>(threadIdx.x), t = static_cast<int>(blockIdx.y);
    if (o >= Z) return;
    const size_t zt = static_cast<size_t>(Z) * T, row = static_cast<size_t>(t) * Z + o;
    double acc = part[row];
    for (int s = 1; s < nseg; ++s) acc = acc + part[static_cast<size_t>(s) * zt + row];
    if (last[row] == 0.0) {  // a zero row: a trip inside the zone, 300 s and no draw
        acc = 0.0;
    } else {
        const int l = ell[row];
        if (l < Z) {  // the residual of a row total below 1 goes to the last destination with p > 0 (D1)
            const size_t cell = static_cast<size_t>(t) * Z * Z + static_cast<size_t>(l) * Z + o;
            acc = acc + r[row] * (l == o ? 0.0 : etv_var_sec(mean[cell], sdev[cell]));
        }
    }
    v[row] = acc;
}

// grid = (ceil(Z / kGradStrip), nseg).  p_t, m_t: the hour's block of p and of the mean plane; dist: [Z][Z].  st: the pass's
// [Zs][2][NB].  cs / cd: the pass's first functional's S_k[j] / D_k[j] (cot_stride words apart), or nullptr in front of the day.
// part: [nseg][3][kEtvNB][Zs] (s1, s2, b); words o < Z of functionals f < nf are all written.
template <int NB, bool ODD>
__global__ __launch_bounds__(kExpBlock) void k_etv_u(const double *__restrict__ p_t, const double *__restrict__ m_t, const double *__restrict__ dist,
                                                     const double *__restrict__ st, const double *__restrict__ cs, const double *__restrict__ cd,
                                                     size_t cot_stride, int Z, int Zs, int seg_len, int nf, double *__restrict__ part)
{
    constexpr int NA = kElvAcc * NB, ROUNDS = (NA + kGradRound - 1) / kGradRound;
    __shared__ double s_acc[kExpWaves][kGradRound][64];
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int seg = static_cast<int>(blockIdx.y);
    const int o0 = static_cast<int>(blockIdx.x) * kGradStrip;
    const int oa = ODD ? o0 + lane : o0 + 2 * lane, ob = ODD ? oa + 64 : oa + 1;
    const bool in_a = oa < Z, in_b = ob < Z;  // (Z even: both or neither)
    const int d_begin = seg * seg_len, d_end = d_begin + seg_len < Z ? d_begin + seg_len : Z;

    double ma[NB], mb[NB], Sa[NB], Sb[NB], Da[NB], Db[NB];  // the lane's own mu[o], S[o], D[o]
#pragma unroll
    for (int f = 0; f < NB; ++f) {
        const int g = f < nf ? f : nf - 1;  // (slots nf .. NB - 1 repeat functional nf - 1; their sums are not written)
        ma[f] = in_a ? st[static_cast<size_t>(oa) * 2 * NB + f] : 0.0;
        mb[f] = in_b ? st[static_cast<size_t>(ob) * 2 * NB + f] : 0.0;
        Sa[f] = cs && in_a ? cs[static_cast<size_t>(g) * cot_stride + oa] : 0.0;
        Sb[f] = cs && in_b ? cs[static_cast<size_t>(g) * cot_stride + ob] : 0.0;
        Da[f] = cd && in_a ? cd[static_cast<size_t>(g) * cot_stride + oa] : 0.0;
        Db[f] = cd && in_b ? cd[static_cast<size_t>(g) * cot_stride + ob] : 0.0;
    }
    double acc[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) acc[j] = 0.0;
    for (int d0 = d_begin + wave; d0 < d_end; d0 += kExpWaves * kEtvUnroll) {
        double pa[kEtvUnroll], pb[kEtvUnroll], sa[kEtvUnroll], sb[kEtvUnroll], ka[kEtvUnroll], kb[kEtvUnroll];
#pragma unroll
        for (int u = 0; u < kEtvUnroll; ++u) {
            const int d = d0 + u * kExpWaves;  // (uniform over the wave)
            pa[u] = pb[u] = sa[u] = sb[u] = ka[u] = kb[u] = 0.0;
            if (d < d_end) {
                const size_t row = static_cast<size_t>(d) * Z;
                if (ODD) {
                    if (in_a) {
                        pa[u] = __builtin_nontemporal_load(p_t + row + oa);
                        sa[u] = __builtin_nontemporal_load(m_t + row + oa);
                        ka[u] = dist[row + oa];
                    }
                    if (in_b) {
                        pb[u] = __builtin_nontemporal_load(p_t + row + ob);
                        sb[u] = __builtin_nontemporal_load(m_t + row + ob);
                        kb[u] = dist[row + ob];
                    }
                } else if (in_a) {
                    const exp_f64x2 pv = __builtin_nontemporal_load(reinterpret_cast<const exp_f64x2 *>(p_t + row + oa));
                    const exp_f64x2 mv = __builtin_nontemporal_load(reinterpret_cast<const exp_f64x2 *>(m_t + row + oa));
                    const exp_f64x2 dv = *reinterpret_cast<const exp_f64x2 *>(dist + row + oa);
                    pa[u] = pv.x, pb[u] = pv.y, sa[u] = mv.x, sb[u] = mv.y, ka[u] = dv.x, kb[u] = dv.y;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kEtvUnroll; ++u) {
            const int d = d0 + u * kExpWaves;
            if (d < d_end) {
                const double *__restrict__ srow = st + static_cast<size_t>(d) * 2 * NB;
                const double seca = d == oa ? kTripIntraSec : sa[u], secb = d == ob ? kTripIntraSec : sb[u];
                const double kma = d == oa ? kTripIntraKm : ka[u], kmb = d == ob ? kTripIntraKm : kb[u];
#pragma unroll
                for (int f = 0; f < NB; ++f) {
                    const double m = srow[f], n = srow[NB + f];
                    const double za = (m - ma[f]) + (Sa[f] * seca + Da[f] * kma), zb = (m - mb[f]) + (Sb[f] * secb + Db[f] * kmb);
                    const double ta = pa[u] * za, tb = pb[u] * zb;
                    acc[f * kElvAcc] = acc[f * kElvAcc] + ta;
                    acc[f * kElvAcc + 1] = acc[f * kElvAcc + 1] + tb;
                    acc[f * kElvAcc + 2] = acc[f * kElvAcc + 2] + ta * za;
                    acc[f * kElvAcc + 3] = acc[f * kElvAcc + 3] + tb * zb;
                    acc[f * kElvAcc + 4] = acc[f * kElvAcc + 4] + pa[u] * n;
                    acc[f * kElvAcc + 5] = acc[f * kElvAcc + 5] + pb[u] * n;
                }
            }
        }
    }
    // round r: accumulators r * 4 .. r * 4 + 3 of every lane; thread (i, l) adds accumulator r * 4 + i of lane l over the four
    // waves, in order
    const int i = tid >> 6;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
#pragma unroll
        for (int k = 0; k < kGradRound; ++k)
            if (r * kGradRound + k < NA) s_acc[wave][k][lane] = acc[r * kGradRound + k];
        __syncthreads();
        const int j = r * kGradRound + i;
        if (j < NA) {
            const double sum = ((s_acc[0][i][lane] + s_acc[1][i][lane]) + s_acc[2][i][lane]) + s_acc[3][i][lane];
            const int f = j / kElvAcc, k = j % kElvAcc;
            const int o = ODD ? o0 + lane + 64 * (k & 1) : o0 + 2 * lane + (k & 1);
            if (f < nf && o < Z) part[((static_cast<size_t>(seg) * 3 + (k >> 1)) * kEtvNB + f) * Zs + o] = sum;
        }
        __syncthreads();
    }
}
static_assert(kExpWaves == 4 && kExpBlock == 256 && kGradRound == 4, "k_etv_u deals destinations over four waves and hands one accumulator to each 64 threads");

// The rest of one backward operator for origin o of the functional in slot blockIdx.y of the pass.  grid = (ceil(Z / kFinishBlock), NB).
// st: the pass's [Zs][2][NB] behind the operator (zeros behind the last one).  m_t: the hour's block of the mean plane; dist: [Z][Z];
// vsec_t: the hour's row of v_sec.  gp / gd / cs / cd: the pass's first functional's A_k[j] / B_k[j] / S_k[j] / D_k[j] (cot_stride words
// apart), or nullptr in front of the day.  st_out: the pass's [Zs][2][NB]; slots nf .. NB - 1 repeat functional nf - 1.  zone:
// nullptr, or the pass's first functional's [2][Z] (2 * Z words apart): V then W, slots f < nf.
__global__ __launch_bounds__(kFinishBlock) void k_etv_finish(const double *__restrict__ part, int nseg, int Zs, const double *__restrict__ last_t,
                                                             const int *__restrict__ ell_t, const double *__restrict__ r_t, const double *__restrict__ q_t,
                                                             const double *__restrict__ m_t, const double *__restrict__ dist,
                                                             const double *__restrict__ vsec_t, const double *__restrict__ st, int NB,
                                                             const double *__restrict__ gp, const double *__restrict__ gd, const double *__restrict__ cs,
                                                             const double *__restrict__ cd, size_t cot_stride, int Z, int nf, double *__restrict__ st_out,
                                                             double *__restrict__ zone)
{
    const int o = static_cast<int>(blockIdx.x) * kFinishBlock + static_cast<int>(threadIdx.x);
    const int slot = static_cast<int>(blockIdx.y), f = slot < nf ? slot : nf - 1;
    if (o >= Z) return;
    const size_t co = static_cast<size_t>(f) * cot_stride + o;
    const double vgp = gp ? gp[co] : 0.0, vgd = gd ? gd[co] : 0.0, S = cs ? cs[co] : 0.0, D = cd ? cd[co] : 0.0;
    const double m = st[static_cast<size_t>(o) * 2 * NB + f], n = st[static_cast<size_t>(o) * 2 * NB + NB + f];
    double s1, s2, b;
    if (last_t[o] == 0.0) {  // a zero row: the driver stays in o (src/resampling.jl:35-36), a trip inside the zone
        const double z = S * kTripIntraSec + D * kTripIntraKm;
        s1 = z;
        s2 = z * z;
        b = n;
    } else {
        s1 = s2 = b = 0.0;
        const int l = ell_t[o];
        const double *__restrict__ pf = part + static_cast<size_t>(f) * Zs + o;
        const size_t kind_stride = static_cast<size_t>(kEtvNB) * Zs, seg_stride = 3 * kind_stride;
        for (int s0 = 0; s0 < nseg; s0 += kFinishUnroll) {
            double v1[kFinishUnroll], v2[kFinishUnroll], vb[kFinishUnroll];
#pragma unroll
            for (int u = 0; u < kFinishUnroll; ++u) {
                const bool in = s0 + u < nseg;
                const double *__restrict__ ps = pf + static_cast<size_t>(s0 + u) * seg_stride;
                v1[u] = in ? ps[0] : 0.0;
                v2[u] = in ? ps[kind_stride] : 0.0;
                vb[u] = in ? ps[2 * kind_stride] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < kFinishUnroll; ++u)
                if (s0 + u < nseg) {
                    s1 = s0 + u == 0 ? v1[u] : s1 + v1[u];
                    s2 = s0 + u == 0 ? v2[u] : s2 + v2[u];
                    b = s0 + u == 0 ? vb[u] : b + vb[u];
                }
        }
        if (l < Z) {  // the residual of a row total below 1 goes to the last destination with p > 0 (D1)
            const double rr = r_t[o];
            const double ml = st[static_cast<size_t>(l) * 2 * NB + f], nl = st[static_cast<size_t>(l) * 2 * NB + NB + f];
            const size_t cell = static_cast<size_t>(l) * Z + o;
            const double sec = l == o ? kTripIntraSec : m_t[cell], km = l == o ? kTripIntraKm : dist[cell];
            const double zl = (ml - m) + (S * sec + D * km), tl = rr * zl;
            s1 = s1 + tl;
            s2 = s2 + tl * zl;
            b = b + rr * nl;
        }
    }
    const double q = exp_q(q_t[o]), omq = 1.0 - q;
    const double db = vgd + s1;
    double cv = s2 - s1 * s1;  // (its exact value is not negative)
    cv = cv > 0.0 ? cv : 0.0;
    const double J = q * ((omq * (db * db) + cv) + (S * S) * vsec_t[o]);
    const double V = (vgp + m) + q * db;
    const double W = (omq * n + q * b) + J;
    st_out[static_cast<size_t>(o) * 2 * NB + slot] = V;
    st_out[static_cast<size_t>(o) * 2 * NB + NB + slot] = W;
    if (zone && slot < nf) {
        zone[static_cast<size_t>(f) * 2 * Z + o] = V;
        zone[static_cast<size_t>(f) * 2 * Z + Z + o] = W;
    }
}

}  // namespace cpm
