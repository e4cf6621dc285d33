// cpm_expected_grad.h -- the adjoint of the expected densities (include/cpm_expected_grad.h): k_exp_grad_u, k_exp_grad_finish.
//
// One backward operator is two launches.  k_exp_grad_u forms the transposed product u[o] = sum over d of p[t][d][o] * mu[d] while the
// hour's Z x Z block of p ([Z dest][Z origin], origin fastest) is read ONCE: these are column sums weighted by mu[d], the access
// pattern of k_exp_trip (cpm_expected_travel.h).  A workgroup of 256 threads takes a strip of kGradStrip = 128 origins and one
// segment of the destinations; a lane owns two origins and keeps two accumulators.  p comes through non-temporal loads (read once per
// operator: it must not displace mu and the vectors of the finishing kernel from the L2), mu[d] is one word per destination and
// wave, served by the L2.  k_exp_grad_finish adds the segments, the residual term and the zero rows and forms c, dq and lambda: a
// lane per origin in one-wave workgroups, the segments' sums requested eight at a time (one load per addition in a loop of unknown
// length was one L2 round trip per segment: 10.9 us per operator at Z = 4,096 against 5.9 us this way, profiles/expected_grad_notes.md).
//
// k_exp_trip covers all hours in one launch; the hours of the adjoint depend on each other, so a launch has only the hour's
// ceil(Z / 128) strips to fill the chip with.  The number of segments is therefore the main choice: grad_segments aims at about
// 1,024 workgroups (four per CU, each wave with kGradUnroll = 8 rows of 1 KiB in flight: 128 KiB per CU), keeps a segment at least
// one round of the four waves long (32 destinations) and is a function of Z alone, so the order of the sums does not depend on the
// device.
//
// Z even: a lane's two origins are neighbours and come with one 16-byte load (every row then starts on a 16-byte line).  Z odd: every
// other row starts 8 bytes behind a line; the kernel falls back to two 8-byte loads, origins lane and lane + 64 of the strip (each
// load of a wave still covers 512 consecutive bytes).  Which origin a lane owns changes no sum.
//
// Order of every sum (no floating-point atomics): the destinations of a segment are dealt over the four waves, wave v takes
// d = begin + v, begin + v + 4, ...; a lane adds its products in ascending d, acc = acc + p * mu[d], starting from 0; the four waves
// are added in order, ((w0 + w1) + w2) + w3; k_exp_grad_finish adds the segments in ascending order, starting from segment 0's sum,
// and then the residual term r * mu[ell].  grad_p_drive of an hour with two operators (CPM_EXPECT_IVP): the day's dq is stored, the
// IVP's is added to it by the later launch.
//
// Separate kernels in a header of their own: k_exp_hour, k_exp_trip and the hourly sampler's code do not move.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cpm_expected.h"

namespace cpm {

constexpr int kGradStrip = 2 * 64;  // origins of a workgroup: two per lane, every wave sees the whole strip
constexpr int kGradUnroll = 8;      // destinations of a wave in flight (one 16-byte load, or two 8-byte loads, per lane each)
constexpr int kGradMaxSeg = 64;
constexpr int kGradSegMin = kExpWaves * kGradUnroll;  // a segment keeps at least one round of the four waves
constexpr int kFinishUnroll = 8;    // segments' sums of an origin in flight in k_exp_grad_finish
constexpr int kFinishBlock = 64;    // one wave per workgroup: the Z threads of the finishing kernel spread over as many CUs as they can

// destination segments of k_exp_grad_u: a function of Z alone
inline int grad_segments(int Z)
{
    const int strips = (Z + kGradStrip - 1) / kGradStrip;
    int n = (1024 + strips - 1) / strips;
    const int most = Z / kGradSegMin;
    if (n > most) n = most;
    if (n > kGradMaxSeg) n = kGradMaxSeg;
    return n < 1 ? 1 : n;
}
inline int grad_segment_len(int Z, int nseg) { return (Z + nseg - 1) / nseg; }

// grid = (ceil(Z / kGradStrip), nseg).  p_t: the hour's block.  part: [nseg][Zs] the segments' sums; words o < Z are all written.
template <bool ODD>
__global__ __launch_bounds__(kExpBlock) void k_exp_grad_u(const double *__restrict__ p_t, const double *__restrict__ mu, int Z, int Zs, int seg_len,
                                                          double *__restrict__ part)
{
    __shared__ double s_acc[kExpWaves][2][64];
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int seg = static_cast<int>(blockIdx.y);
    const int o0 = static_cast<int>(blockIdx.x) * kGradStrip;
    const int oa = ODD ? o0 + lane : o0 + 2 * lane, ob = ODD ? oa + 64 : oa + 1;
    const bool in_a = oa < Z, in_b = ob < Z;  // (Z even: both or neither)
    const int d_begin = seg * seg_len, d_end = d_begin + seg_len < Z ? d_begin + seg_len : Z;

    double ua = 0.0, ub = 0.0;
    for (int d0 = d_begin + wave; d0 < d_end; d0 += kExpWaves * kGradUnroll) {
        double pa[kGradUnroll], pb[kGradUnroll], m[kGradUnroll];
#pragma unroll
        for (int u = 0; u < kGradUnroll; ++u) {
            const int d = d0 + u * kExpWaves;  // (uniform over the wave)
            pa[u] = pb[u] = m[u] = 0.0;
            if (d < d_end) {
                const size_t row = static_cast<size_t>(d) * Z;
                m[u] = mu[d];
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
                ua = ua + pa[u] * m[u];
                ub = ub + pb[u] * m[u];
            }
        }
    }
    s_acc[wave][0][lane] = ua;
    s_acc[wave][1][lane] = ub;
    __syncthreads();
    // thread (i, l): accumulator i of lane l over the four waves, in order
    if (tid < 2 * 64) {
        const int i = tid >> 6, l = tid & 63;
        const double sum = ((s_acc[0][i][l] + s_acc[1][i][l]) + s_acc[2][i][l]) + s_acc[3][i][l];
        const int o = ODD ? o0 + l + 64 * i : o0 + 2 * l + i;
        if (o < Z) part[static_cast<size_t>(seg) * Zs + o] = sum;
    }
}
static_assert(kExpWaves == 4 && kExpBlock == 256, "k_exp_grad_u deals destinations over four waves and reduces 2 x 64 accumulators");

// The rest of one backward operator for origin o.  grid = ceil(Z / kFinishBlock).  Pointers are the hour's / the operator's slices.
//   a = mu[o] for a zero row, else (the segments in order) + r[o] * mu[ell[o]];  c = (gd - mu) + a;  dq = pi * c;
//   mu_out = (gp + mu) + q * c.
// mu == nullptr: mu is zero by construction (the last operator without G_next) and no product was formed: a = 0, part is not read.
// gp / gd == nullptr: an operator in front of the day (CPM_EXPECT_IVP), whose state is no output.
// grad_t: grad_p_drive of the hour; accumulate: the hour's second operator adds to what the day's stored.  0 wherever the
// installed p_drive is not strictly inside (0, 1): exp_q is flat there.
__global__ __launch_bounds__(kFinishBlock) void k_exp_grad_finish(const double *__restrict__ part, int nseg, int Zs, const double *__restrict__ last_t,
                                                               const int *__restrict__ ell_t, const double *__restrict__ r_t,
                                                               const double *__restrict__ q_t, const double *__restrict__ pi_s,
                                                               const double *__restrict__ mu, const double *__restrict__ gp,
                                                               const double *__restrict__ gd, int Z, int accumulate, double *__restrict__ mu_out,
                                                               double *grad_t)
{
    const int o = static_cast<int>(blockIdx.x) * kFinishBlock + static_cast<int>(threadIdx.x);
    if (o >= Z) return;
    const double m = mu ? mu[o] : 0.0;
    double a = 0.0;
    if (mu) {
        if (last_t[o] == 0.0) {  // a zero row: the driver stays in o (src/resampling.jl:35-36)
            a = m;
        } else {
            // (what the chain of segments does not depend on is requested first; the segments come kFinishUnroll loads at a time:
            //  one load per addition in a loop of unknown length is one L2 round trip per segment)
            const int l = ell_t[o];
            const double rr = r_t[o];
            const double ml = l < Z ? mu[l] : 0.0;
            for (int s0 = 0; s0 < nseg; s0 += kFinishUnroll) {
                double v[kFinishUnroll];
#pragma unroll
                for (int u = 0; u < kFinishUnroll; ++u) v[u] = s0 + u < nseg ? part[static_cast<size_t>(s0 + u) * Zs + o] : 0.0;
#pragma unroll
                for (int u = 0; u < kFinishUnroll; ++u)
                    if (s0 + u < nseg) a = s0 + u == 0 ? v[u] : a + v[u];
            }
            if (l < Z) a = a + rr * ml;  // the residual of a row total below 1 goes to the last destination with p > 0 (D1)
        }
    }
    const double vgp = gp ? gp[o] : 0.0, vgd = gd ? gd[o] : 0.0;
    const double qraw = q_t[o];
    const double c = (vgd - m) + a;
    const double dq = pi_s[o] * c;
    mu_out[o] = (vgp + m) + exp_q(qraw) * c;
    const bool inside = qraw > 0.0 && qraw < 1.0;  // (false for NaN)
    grad_t[o] = inside ? (accumulate ? grad_t[o] + dq : dq) : 0.0;
}

}  // namespace cpm
