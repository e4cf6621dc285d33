// cpm_expected_grad_batch.h -- the adjoint of the expected densities for the fleets of a batch (include/cpm_expected_grad_batch.h):
// k_exp_grad_u_b<NB, ODD>, k_exp_grad_dest_u_b<NB, ODD>, k_exp_grad_finish_b, k_exp_grad_dest_finish_b, k_exp_grad_pack_b.
//
// The product kernels do the work of k_exp_grad_u / k_exp_grad_dest_u (cpm_expected_grad.h, cpm_expected_grad_dest.h) for the
// nf <= NB fleets of a pass while the hour's block of p -- and of the tangent dP -- is streamed ONCE: the same strips of kGradStrip
// origins, the same destination segments (grad_segments), the same deal of a segment over the four waves, kGradUnroll destinations of
// a wave in flight, the same non-temporal 16-byte loads (two 8-byte loads for odd Z).  A lane keeps 2 * NB accumulators, 4 * NB with
// the tangent.  Per fleet the chain is that of the B = 1 kernel operation for operation: from 0, acc = acc + p * mu_f[d] in
// ascending d of the wave's deal, then ((w0 + w1) + w2) + w3 through LDS.  Fleet b's words therefore carry the bits of the B = 1
// call whatever NB is and wherever the fleet stands in its pass.
//
// mu of a pass is laid out [Zs][NB], fleet fastest: the NB words of one destination are one line of at most 64 bytes.  The wave's
// index goes through readfirstlane, so d is uniform by construction and the words of mu come through the scalar data path into
// SGPRs: kGradUnroll * NB doubles in VGPRs (128 registers at NB = 8) would have cost the occupancy the streaming depends on.
//
// The four waves are added in rounds of kGradRound = 4 accumulators over one 8 KiB buffer (4 waves x 4 x 64 doubles): 4 * 4 * NB * 64
// doubles at once are 64 KiB for the tangent at NB = 8, which leaves two workgroups per CU where the B = 1 kernel runs four.  A round
// changes which accumulators share the buffer, not the order of any sum.
//
// Fleets beyond nf repeat the last one and are not stored (the rule of k_exp_hour): the finishing and packing kernels fill slots
// nf .. NB - 1 of mu with fleet nf - 1's words.  A pass of one fleet goes to the B = 1 kernels.
//
// The finishing kernels are k_exp_grad_finish / k_exp_grad_dest_finish with a lane per (origin, fleet): a one-wave workgroup takes 64
// origins of one fleet, so every load of the segments' sums, q, pi and the cotangents and every store of the outputs covers whole
// lines; only the words of mu are NB apart.  c, dq, lambda and gdest are formed by the same operations in the same order.
//
// Separate kernels in a header of their own: no existing kernel moves.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cpm_expected_grad_dest.h"

namespace cpm {

constexpr int kGradRound = 4;  // accumulators of a lane per round of the four-wave reduction (one per wave's worth of threads)

// part, part_dp: [nseg][kExpMaxNB][Zs] of the pass; words o < Z of fleets f < nf are all written.  mu: [Zs][NB].
template <int NB, bool ODD, bool DEST>
__device__ __forceinline__ void exp_grad_u_b(const double *__restrict__ p_t, const double *__restrict__ dp_t, const double *__restrict__ mu, int Z, int Zs,
                                             int seg_len, int nf, double *__restrict__ part, double *__restrict__ part_dp)
{
    constexpr int A = DEST ? 4 : 2;  // accumulators of a fleet: u of the lane's two origins, then w of the two
    constexpr int NA = A * NB;
    static_assert(NA % kGradRound == 0 && kGradRound == kExpWaves, "a round hands one accumulator to each 64 threads");
    __shared__ double s_acc[kExpWaves][kGradRound][64];
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int seg = static_cast<int>(blockIdx.y);
    const int o0 = static_cast<int>(blockIdx.x) * kGradStrip;
    const int oa = ODD ? o0 + lane : o0 + 2 * lane, ob = ODD ? oa + 64 : oa + 1;
    const bool in_a = oa < Z, in_b = ob < Z;  // (Z even: both or neither)
    const int d_begin = seg * seg_len, d_end = d_begin + seg_len < Z ? d_begin + seg_len : Z;

    double acc[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) acc[j] = 0.0;
    for (int d0 = d_begin + wave; d0 < d_end; d0 += kExpWaves * kGradUnroll) {
        double pa[kGradUnroll], pb[kGradUnroll], ta[kGradUnroll], tb[kGradUnroll], m[kGradUnroll][NB];
#pragma unroll
        for (int u = 0; u < kGradUnroll; ++u) {
            const int d = d0 + u * kExpWaves;  // (uniform over the wave)
            pa[u] = pb[u] = ta[u] = tb[u] = 0.0;
#pragma unroll
            for (int f = 0; f < NB; ++f) m[u][f] = 0.0;
            if (d < d_end) {
                const size_t row = static_cast<size_t>(d) * Z;
                const double *__restrict__ mrow = mu + static_cast<size_t>(d) * NB;
#pragma unroll
                for (int f = 0; f < NB; ++f) m[u][f] = mrow[f];
                if (ODD) {
                    if (in_a) {
                        pa[u] = __builtin_nontemporal_load(p_t + row + oa);
                        if (DEST) ta[u] = __builtin_nontemporal_load(dp_t + row + oa);
                    }
                    if (in_b) {
                        pb[u] = __builtin_nontemporal_load(p_t + row + ob);
                        if (DEST) tb[u] = __builtin_nontemporal_load(dp_t + row + ob);
                    }
                } else if (in_a) {
                    const exp_f64x2 pv = __builtin_nontemporal_load(reinterpret_cast<const exp_f64x2 *>(p_t + row + oa));
                    pa[u] = pv.x, pb[u] = pv.y;
                    if (DEST) {
                        const exp_f64x2 tv = __builtin_nontemporal_load(reinterpret_cast<const exp_f64x2 *>(dp_t + row + oa));
                        ta[u] = tv.x, tb[u] = tv.y;
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kGradUnroll; ++u) {
            const int d = d0 + u * kExpWaves;
            if (d < d_end) {
#pragma unroll
                for (int f = 0; f < NB; ++f) {
                    acc[f * A] = acc[f * A] + pa[u] * m[u][f];
                    acc[f * A + 1] = acc[f * A + 1] + pb[u] * m[u][f];
                    if (DEST) {
                        acc[f * A + 2] = acc[f * A + 2] + ta[u] * m[u][f];
                        acc[f * A + 3] = acc[f * A + 3] + tb[u] * m[u][f];
                    }
                }
            }
        }
    }
    // round r: accumulators r * 4 .. r * 4 + 3 of every lane; thread (i, l) adds accumulator r * 4 + i of lane l over the four
    // waves, in order
    const int i = tid >> 6;
#pragma unroll
    for (int r = 0; r < NA / kGradRound; ++r) {
#pragma unroll
        for (int k = 0; k < kGradRound; ++k) s_acc[wave][k][lane] = acc[r * kGradRound + k];
        __syncthreads();
        const double sum = ((s_acc[0][i][lane] + s_acc[1][i][lane]) + s_acc[2][i][lane]) + s_acc[3][i][lane];
        const int j = r * kGradRound + i, f = j / A, k = j % A;
        const int o = ODD ? o0 + lane + 64 * (k & 1) : o0 + 2 * lane + (k & 1);
        if (f < nf && o < Z) (k < 2 ? part : part_dp)[(static_cast<size_t>(seg) * kExpMaxNB + f) * Zs + o] = sum;
        __syncthreads();
    }
}

// grid = (ceil(Z / kGradStrip), nseg).  p_t: the hour's block.  mu: the pass's [Zs][NB].  nf <= NB fleets are stored.
template <int NB, bool ODD>
__global__ __launch_bounds__(kExpBlock) void k_exp_grad_u_b(const double *__restrict__ p_t, const double *__restrict__ mu, int Z, int Zs, int seg_len, int nf,
                                                            double *__restrict__ part)
{
    exp_grad_u_b<NB, ODD, false>(p_t, nullptr, mu, Z, Zs, seg_len, nf, part, nullptr);
}

// ... with the hour's block of the tangent beside it
template <int NB, bool ODD>
__global__ __launch_bounds__(kExpBlock) void k_exp_grad_dest_u_b(const double *__restrict__ p_t, const double *__restrict__ dp_t,
                                                                 const double *__restrict__ mu, int Z, int Zs, int seg_len, int nf,
                                                                 double *__restrict__ part, double *__restrict__ part_dp)
{
    exp_grad_u_b<NB, ODD, true>(p_t, dp_t, mu, Z, Zs, seg_len, nf, part, part_dp);
}
static_assert(kExpWaves == 4 && kExpBlock == 256 && kExpMaxNB == 8, "the batched products deal destinations over four waves and keep up to eight fleets");

// G_next of the pass's fleets ([nf][Z], Z words apart) into the layout the product kernel reads: mu[z * NB + f], slots f >= nf
// repeating fleet nf - 1.  grid = (ceil(Z / 256), NB).
__global__ __launch_bounds__(kExpBlock) void k_exp_grad_pack_b(const double *__restrict__ gnext, int Z, int NB, int nf, double *__restrict__ mu)
{
    const int z = static_cast<int>(blockIdx.x) * kExpBlock + static_cast<int>(threadIdx.x), f = static_cast<int>(blockIdx.y);
    if (z >= Z) return;
    mu[static_cast<size_t>(z) * NB + f] = gnext[static_cast<size_t>(f < nf ? f : nf - 1) * Z + z];
}

// The rest of one backward operator for origin o of the fleet in slot f = blockIdx.y of the pass: k_exp_grad_finish (DEST:
// k_exp_grad_dest_finish) operation for operation.  grid = (ceil(Z / kFinishBlock), NB).  Pointers with a fleet stride point at the
// pass's first fleet: q_t (q_stride), pi_s (Zs), gp / gd (cot_stride), grad_t / dest_t (Z * T = grad_stride); part / part_dp are
// the pass's [nseg][kExpMaxNB][Zs]; mu is the pass's [Zs][NB] or nullptr (zero by construction: no product was formed).
// mu_out[o * mo_o + f * mo_f]: the workspace ([Zs][NB]: mo_o = NB, mo_f = 1, fill = 1: slots nf .. NB - 1 repeat fleet nf - 1) or
// grad_pi0 ([nf][Z]: mo_o = 1, mo_f = Z, fill = 0).  Slots f >= nf store nothing else.
template <bool DEST>
__device__ __forceinline__ void exp_grad_finish_b(const double *__restrict__ part, const double *__restrict__ part_dp, int nseg, int Zs,
                                                  const double *__restrict__ last_t, const int *__restrict__ ell_t, const double *__restrict__ r_t,
                                                  const double *__restrict__ q_t, size_t q_stride, const double *__restrict__ pi_s,
                                                  const double *__restrict__ mu, int NB, const double *__restrict__ gp, const double *__restrict__ gd,
                                                  size_t cot_stride, int Z, int nf, int accumulate, double *__restrict__ mu_out, size_t mo_o, size_t mo_f,
                                                  int fill, double *grad_t, double *dest_t, size_t grad_stride)
{
    const int o = static_cast<int>(blockIdx.x) * kFinishBlock + static_cast<int>(threadIdx.x);
    const int slot = static_cast<int>(blockIdx.y), f = slot < nf ? slot : nf - 1;
    if (o >= Z || (slot >= nf && !fill)) return;
    const double m = mu ? mu[static_cast<size_t>(o) * NB + f] : 0.0;
    double a = 0.0, w = 0.0;
    if (mu) {
        if (last_t[o] == 0.0) {  // a zero row: the driver stays in o (src/resampling.jl:35-36); no entry of the row carries a tangent
            a = m;
        } else {
            const int l = ell_t[o];
            const double rr = r_t[o];
            const double ml = l < Z ? mu[static_cast<size_t>(l) * NB + f] : 0.0;
            const double *__restrict__ pf = part + static_cast<size_t>(f) * Zs + o;
            const double *__restrict__ tf = DEST ? part_dp + static_cast<size_t>(f) * Zs + o : nullptr;
            const size_t seg_stride = static_cast<size_t>(kExpMaxNB) * Zs;
            for (int s0 = 0; s0 < nseg; s0 += kFinishUnroll) {
                double v[kFinishUnroll], t[kFinishUnroll];
#pragma unroll
                for (int u = 0; u < kFinishUnroll; ++u) {
                    v[u] = s0 + u < nseg ? pf[static_cast<size_t>(s0 + u) * seg_stride] : 0.0;
                    t[u] = (DEST && s0 + u < nseg) ? tf[static_cast<size_t>(s0 + u) * seg_stride] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < kFinishUnroll; ++u)
                    if (s0 + u < nseg) {
                        a = s0 + u == 0 ? v[u] : a + v[u];
                        if (DEST) w = s0 + u == 0 ? t[u] : w + t[u];
                    }
            }
            if (l < Z) a = a + rr * ml;  // the residual goes into a alone: r is held fixed along the tangent
        }
    }
    const size_t co = static_cast<size_t>(f) * cot_stride + o;
    const double vgp = gp ? gp[co] : 0.0, vgd = gd ? gd[co] : 0.0;
    const double qraw = q_t[static_cast<size_t>(f) * q_stride + o];
    const double q = exp_q(qraw), pi = pi_s[static_cast<size_t>(f) * Zs + o];
    const double c = (vgd - m) + a;
    const double dq = pi * c;
    mu_out[static_cast<size_t>(o) * mo_o + static_cast<size_t>(slot) * mo_f] = (vgp + m) + q * c;
    if (slot >= nf) return;
    const size_t go = static_cast<size_t>(f) * grad_stride + o;
    const bool inside = qraw > 0.0 && qraw < 1.0;  // (false for NaN)
    grad_t[go] = inside ? (accumulate ? grad_t[go] + dq : dq) : 0.0;
    if (DEST) {
        const double gdest = (pi * q) * w;
        dest_t[go] = accumulate ? dest_t[go] + gdest : gdest;
    }
}

__global__ __launch_bounds__(kFinishBlock) void k_exp_grad_finish_b(const double *__restrict__ part, int nseg, int Zs, const double *__restrict__ last_t,
                                                                    const int *__restrict__ ell_t, const double *__restrict__ r_t,
                                                                    const double *__restrict__ q_t, size_t q_stride, const double *__restrict__ pi_s,
                                                                    const double *__restrict__ mu, int NB, const double *__restrict__ gp,
                                                                    const double *__restrict__ gd, size_t cot_stride, int Z, int nf, int accumulate,
                                                                    double *__restrict__ mu_out, size_t mo_o, size_t mo_f, int fill, double *grad_t,
                                                                    size_t grad_stride)
{
    exp_grad_finish_b<false>(part, nullptr, nseg, Zs, last_t, ell_t, r_t, q_t, q_stride, pi_s, mu, NB, gp, gd, cot_stride, Z, nf, accumulate, mu_out, mo_o,
                             mo_f, fill, grad_t, nullptr, grad_stride);
}

__global__ __launch_bounds__(kFinishBlock) void k_exp_grad_dest_finish_b(const double *__restrict__ part, const double *__restrict__ part_dp, int nseg, int Zs,
                                                                         const double *__restrict__ last_t, const int *__restrict__ ell_t,
                                                                         const double *__restrict__ r_t, const double *__restrict__ q_t, size_t q_stride,
                                                                         const double *__restrict__ pi_s, const double *__restrict__ mu, int NB,
                                                                         const double *__restrict__ gp, const double *__restrict__ gd, size_t cot_stride,
                                                                         int Z, int nf, int accumulate, double *__restrict__ mu_out, size_t mo_o,
                                                                         size_t mo_f, int fill, double *grad_t, double *dest_t, size_t grad_stride)
{
    exp_grad_finish_b<true>(part, part_dp, nseg, Zs, last_t, ell_t, r_t, q_t, q_stride, pi_s, mu, NB, gp, gd, cot_stride, Z, nf, accumulate, mu_out, mo_o, mo_f,
                            fill, grad_t, dest_t, grad_stride);
}

}  // namespace cpm
