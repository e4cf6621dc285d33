// cpm_expected_linear_var.h -- the exact seed variance of linear functionals of a resample's counts
// (include/cpm_expected_linear_var.h): k_elv_u<NB, ODD>, k_elv_finish, k_elv_total.
//
// One backward operator is two launches, as in the adjoint (cpm_expected_grad.h, cpm_expected_grad_batch.h).  k_elv_u streams the
// hour's Z x Z block of p ONCE for the nf <= NB functionals of a pass: the strips of kGradStrip origins, the destination segments of
// grad_segments, the deal of a segment over the four waves, kGradUnroll destinations of a wave in flight and the non-temporal
// 16-byte loads (two 8-byte loads for odd Z) are those of k_exp_grad_u_b.  Per functional a lane keeps, for each of its two origins,
// the three sums the recurrence needs,
//   s1 = sum p * eta,   s2 = sum (p * eta) * eta,   b = sum p * nu[d],      eta = mu[d] - mu[o],
// and the lane's own mu[o] for the centring: per word of p and functional one subtraction, three multiplications and three
// additions, each ONE IEEE operation, acc = acc + term in ascending d of the wave's deal, from 0.
//
// The state of a pass is laid out [Zs][2][NB], functional fastest, mu then nu: the 2 * NB words of one destination are one line of
// at most 64 bytes.  The wave's index goes through readfirstlane, so d is uniform by construction and the words come through the
// scalar data path into SGPRs, as in k_exp_grad_u_b.
//
// NB = kElvNB = 4.  A lane holds 6 * NB accumulators (12 * NB VGPRs), its own mu (2 * NB doubles: 4 * NB VGPRs) and the unrolled
// loads (kGradUnroll x 2 doubles: 32 VGPRs): 96 VGPRs at NB = 4 before addresses and temporaries, 114 as compiled, no scratch --
// four waves per SIMD, the four workgroups per CU that grad_segments sizes the grid for and the B = 1 product runs at.  NB = 8 would
// need 160 VGPRs for the same and leave three workgroups per CU at best, with fewer rows in flight; NB = 2 reads p twice as often.  The
// instantiations NB = 1 and 2 serve the partial passes.  A functional's chain does not depend on NB or its slot: functional k of K
// carries the bits of a K = 1 call.
//
// The four waves are added through LDS in rounds of kGradRound accumulators, ((w0 + w1) + w2) + w3, as in exp_grad_u_b.
//
// k_elv_finish has a lane per (origin, functional), like k_exp_grad_finish_b: the segments in ascending order starting from segment
// 0's sum, then the residual terms r * eta[l], (r * eta[l]) * eta[l] and r * nu[l], the zero rows, and db, J, V and W.  k_elv_total
// forms sum w[z] * V_0[z] and sum w[z] * W_0[z]: thread i of 256 adds z = i, i + 256, ... in ascending z from 0, then the 256 sums
// are added pairwise over LDS (stride 128, 64, ... 1).
//
// Separate kernels in a header of their own: no existing kernel moves.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cpm_expected_grad_batch.h"

namespace cpm {

constexpr int kElvNB = 4;  // functionals of a pass
constexpr int kElvAcc = 6; // accumulators of a functional: s1, s2, b of the lane's two origins

// grid = (ceil(Z / kGradStrip), nseg).  p_t: the hour's block.  st: the pass's [Zs][2][NB].  part: [nseg][3][kElvNB][Zs] (s1, s2, b);
// words o < Z of functionals f < nf are all written.
template <int NB, bool ODD>
__global__ __launch_bounds__(kExpBlock) void k_elv_u(const double *__restrict__ p_t, const double *__restrict__ st, int Z, int Zs, int seg_len, int nf,
                                                     double *__restrict__ part)
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

    double ma[NB], mb[NB];  // the lane's own mu[o]: the sums are centred at it
#pragma unroll
    for (int f = 0; f < NB; ++f) {
        ma[f] = in_a ? st[static_cast<size_t>(oa) * 2 * NB + f] : 0.0;
        mb[f] = in_b ? st[static_cast<size_t>(ob) * 2 * NB + f] : 0.0;
    }
    double acc[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) acc[j] = 0.0;
    for (int d0 = d_begin + wave; d0 < d_end; d0 += kExpWaves * kGradUnroll) {
        double pa[kGradUnroll], pb[kGradUnroll];
#pragma unroll
        for (int u = 0; u < kGradUnroll; ++u) {
            const int d = d0 + u * kExpWaves;  // (uniform over the wave)
            pa[u] = pb[u] = 0.0;
            if (d < d_end) {
                const size_t row = static_cast<size_t>(d) * Z;
                if (ODD) {
                    if (in_a) pa[u] = __builtin_nontemporal_load(p_t + row + oa);
                    if (in_b) pb[u] = __builtin_nontemporal_load(p_t + row + ob);
                } else if (in_a) {
                    const exp_f64x2 pv = __builtin_nontemporal_load(reinterpret_cast<const exp_f64x2 *>(p_t + row + oa));
                    pa[u] = pv.x, pb[u] = pv.y;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kGradUnroll; ++u) {
            const int d = d0 + u * kExpWaves;
            if (d < d_end) {
                const double *__restrict__ srow = st + static_cast<size_t>(d) * 2 * NB;
#pragma unroll
                for (int f = 0; f < NB; ++f) {
                    const double m = srow[f], n = srow[NB + f];
                    const double ea = m - ma[f], eb = m - mb[f];
                    const double ta = pa[u] * ea, tb = pb[u] * eb;
                    acc[f * kElvAcc] = acc[f * kElvAcc] + ta;
                    acc[f * kElvAcc + 1] = acc[f * kElvAcc + 1] + tb;
                    acc[f * kElvAcc + 2] = acc[f * kElvAcc + 2] + ta * ea;
                    acc[f * kElvAcc + 3] = acc[f * kElvAcc + 3] + tb * eb;
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
            if (f < nf && o < Z) part[((static_cast<size_t>(seg) * 3 + (k >> 1)) * kElvNB + f) * Zs + o] = sum;
        }
        __syncthreads();
    }
}
static_assert(kExpWaves == 4 && kExpBlock == 256 && kGradRound == 4, "k_elv_u deals destinations over four waves and hands one accumulator to each 64 threads");

// The rest of one backward operator for origin o of the functional in slot blockIdx.y of the pass.  grid = (ceil(Z / kFinishBlock), NB).
// st: the pass's [Zs][2][NB] behind the operator, or nullptr (zero by construction: the last operator, no product was formed).
// gp / gd: the pass's first functional's A_k[j] / B_k[j] (cot_stride words apart), or nullptr in front of the day.
// st_out: the pass's [Zs][2][NB]; slots nf .. NB - 1 repeat functional nf - 1.  zone: nullptr, or the pass's first functional's
// [2][Z] (2 * Z words apart): V then W, slots f < nf.
__global__ __launch_bounds__(kFinishBlock) void k_elv_finish(const double *__restrict__ part, int nseg, int Zs, const double *__restrict__ last_t,
                                                             const int *__restrict__ ell_t, const double *__restrict__ r_t, const double *__restrict__ q_t,
                                                             const double *__restrict__ st, int NB, const double *__restrict__ gp,
                                                             const double *__restrict__ gd, size_t cot_stride, int Z, int nf, double *__restrict__ st_out,
                                                             double *__restrict__ zone)
{
    const int o = static_cast<int>(blockIdx.x) * kFinishBlock + static_cast<int>(threadIdx.x);
    const int slot = static_cast<int>(blockIdx.y), f = slot < nf ? slot : nf - 1;
    if (o >= Z) return;
    const double m = st ? st[static_cast<size_t>(o) * 2 * NB + f] : 0.0, n = st ? st[static_cast<size_t>(o) * 2 * NB + NB + f] : 0.0;
    double s1 = 0.0, s2 = 0.0, b = 0.0;
    if (st) {
        if (last_t[o] == 0.0) {  // a zero row: the driver stays in o (src/resampling.jl:35-36)
            b = n;
        } else {
            const int l = ell_t[o];
            const double rr = r_t[o];
            const double ml = l < Z ? st[static_cast<size_t>(l) * 2 * NB + f] : 0.0, nl = l < Z ? st[static_cast<size_t>(l) * 2 * NB + NB + f] : 0.0;
            const double *__restrict__ pf = part + static_cast<size_t>(f) * Zs + o;
            const size_t kind_stride = static_cast<size_t>(kElvNB) * Zs, seg_stride = 3 * kind_stride;
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
                const double el = ml - m, tl = rr * el;
                s1 = s1 + tl;
                s2 = s2 + tl * el;
                b = b + rr * nl;
            }
        }
    }
    const size_t co = static_cast<size_t>(f) * cot_stride + o;
    const double vgp = gp ? gp[co] : 0.0, vgd = gd ? gd[co] : 0.0;
    const double q = exp_q(q_t[o]), omq = 1.0 - q;
    const double db = vgd + s1;
    double cv = s2 - s1 * s1;  // (its exact value is not negative)
    cv = cv > 0.0 ? cv : 0.0;
    const double J = q * (omq * (db * db) + cv);
    const double V = (vgp + m) + q * db;
    const double W = (omq * n + q * b) + J;
    st_out[static_cast<size_t>(o) * 2 * NB + slot] = V;
    st_out[static_cast<size_t>(o) * 2 * NB + NB + slot] = W;
    if (zone && slot < nf) {
        zone[static_cast<size_t>(f) * 2 * Z + o] = V;
        zone[static_cast<size_t>(f) * 2 * Z + Z + o] = W;
    }
}

// out[k][i] = the sum over z of w[z] * zone[k][i][z], i = 0 (mean), 1 (variance).  grid = (2, K).  w: nullptr = 1 per zone (the
// product by 1 is exact: the bits of w = ones).
__global__ __launch_bounds__(kExpBlock) void k_elv_total(const double *__restrict__ zone, const double *__restrict__ w, int Z, double *__restrict__ out)
{
    __shared__ double s_sum[kExpBlock];
    const int tid = static_cast<int>(threadIdx.x);
    const size_t word = static_cast<size_t>(blockIdx.y) * 2 + blockIdx.x;
    const double *__restrict__ x = zone + word * Z;
    double acc = 0.0;
    for (int z = tid; z < Z; z += kExpBlock) acc = acc + (w ? w[z] : 1.0) * x[z];
    s_sum[tid] = acc;
    __syncthreads();
    for (int h = kExpBlock / 2; h > 0; h >>= 1) {
        if (tid < h) s_sum[tid] = s_sum[tid] + s_sum[tid + h];
        __syncthreads();
    }
    if (tid == 0) out[word] = s_sum[0];
}

}  // namespace cpm
