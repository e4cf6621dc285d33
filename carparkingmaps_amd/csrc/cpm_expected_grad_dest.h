// cpm_expected_grad_dest.h -- the adjoint of the expected densities along a tangent of p_destin (include/cpm_expected_grad_dest.h):
// k_exp_grad_dest_u, k_exp_grad_dest_finish, the builders of d p_destin / d e_dest (k_tan_log, k_tan_rowsum, k_tan_final on the dense
// route, k_tan_cells on the compact rows of cpm_dataset.h) and k_exp_trip_tan_finish.
//
// One backward operator stays two launches.  k_exp_grad_dest_u is k_exp_grad_u (cpm_expected_grad.h) with the hour's block of the
// tangent dP streamed beside the block of p: the same strips of kGradStrip origins, the same destination segments (grad_segments), the
// same deal of a segment over the four waves, kGradUnroll destinations of a wave in flight, non-temporal loads for both blocks and
// ONE load of mu[d] for both products.  A lane keeps four accumulators: u (p * mu) and w (dP * mu) of its two origins.  The chain of
// u is the chain of k_exp_grad_u operation for operation, so `part` carries that kernel's bits; `part_dp` is laid out like it.
// Fused, not a second launch: at Z = 2,357 the product is launch- and occupancy-bound, not byte-bound
// (profiles/expected_grad_notes.md), and a second launch per operator would pay that twice.
//
// k_exp_grad_dest_finish is k_exp_grad_finish plus the segments of part_dp, requested kFinishUnroll at a time like those of part, and
//   grad_dest_s[o] = (pi_s[o] * q[o]) * w[o],   w[o] = 0 for a zero row, no residual term.
// c, dq, lambda and grad_p_drive are formed by the same operations in the same order as in k_exp_grad_finish.
//
// Order of the sums of w: exactly that of a in cpm_expected_grad.h without the residual term -- segment, chain (d - begin) mod 4 in
// ascending d from 0, ((c0 + c1) + c2) + c3, the segments in ascending order.  No floating-point atomics.
//
// The tangent of e_dest (d/de of x^e / sum x^e = p * (ln x - sum p ln x)) is built once per e_dest; lanes are origins in every kernel,
// so each load and store of the origin-fastest arrays covers whole lines.  Dense route, three passes over [T][Z dest][Z origin]:
//   k_tan_log     a thread per (origin, destination) pair loads the pair's T means for the extrema as k_pdest_weights does and stores
//                 l = log(x) where the installed p > 0, else 0;
//   k_tan_rowsum  a lane per (origin, hour) adds m = m + p * l over ascending destinations from 0 (p > 0 only);
//   k_tan_final   dP = p * (l - m) where p > 0, else 0.
// Compact-row route: k_tan_cells, a lane per (hour, origin) row, walks the row's cells (sorted by destination) twice and scatters into
// the zeroed dense array.  The cells keep x, the table's sp / sj the installed p and the destination, entry for entry.
//
// Separate kernels in a header of their own: k_exp_grad_u, k_exp_grad_finish, k_exp_trip and everything else do not move.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cpm_dataset.h"
#include "cpm_expected_grad.h"
#include "cpm_expected_travel.h"

namespace cpm {

// grid = (ceil(Z / kGradStrip), nseg).  p_t, dp_t: the hour's blocks.  part, part_dp: [nseg][Zs]; words o < Z are all written.
template <bool ODD>
__global__ __launch_bounds__(kExpBlock) void k_exp_grad_dest_u(const double *__restrict__ p_t, const double *__restrict__ dp_t,
                                                               const double *__restrict__ mu, int Z, int Zs, int seg_len,
                                                               double *__restrict__ part, double *__restrict__ part_dp)
{
    __shared__ double s_acc[kExpWaves][4][64];
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int seg = static_cast<int>(blockIdx.y);
    const int o0 = static_cast<int>(blockIdx.x) * kGradStrip;
    const int oa = ODD ? o0 + lane : o0 + 2 * lane, ob = ODD ? oa + 64 : oa + 1;
    const bool in_a = oa < Z, in_b = ob < Z;  // (Z even: both or neither)
    const int d_begin = seg * seg_len, d_end = d_begin + seg_len < Z ? d_begin + seg_len : Z;

    double ua = 0.0, ub = 0.0, wa = 0.0, wb = 0.0;
    for (int d0 = d_begin + wave; d0 < d_end; d0 += kExpWaves * kGradUnroll) {
        double pa[kGradUnroll], pb[kGradUnroll], ta[kGradUnroll], tb[kGradUnroll], m[kGradUnroll];
#pragma unroll
        for (int u = 0; u < kGradUnroll; ++u) {
            const int d = d0 + u * kExpWaves;  // (uniform over the wave)
            pa[u] = pb[u] = ta[u] = tb[u] = m[u] = 0.0;
            if (d < d_end) {
                const size_t row = static_cast<size_t>(d) * Z;
                m[u] = mu[d];
                if (ODD) {
                    if (in_a) {
                        pa[u] = __builtin_nontemporal_load(p_t + row + oa);
                        ta[u] = __builtin_nontemporal_load(dp_t + row + oa);
                    }
                    if (in_b) {
                        pb[u] = __builtin_nontemporal_load(p_t + row + ob);
                        tb[u] = __builtin_nontemporal_load(dp_t + row + ob);
                    }
                } else if (in_a) {
                    const exp_f64x2 pv = __builtin_nontemporal_load(reinterpret_cast<const exp_f64x2 *>(p_t + row + oa));
                    const exp_f64x2 tv = __builtin_nontemporal_load(reinterpret_cast<const exp_f64x2 *>(dp_t + row + oa));
                    pa[u] = pv.x, pb[u] = pv.y, ta[u] = tv.x, tb[u] = tv.y;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kGradUnroll; ++u) {
            const int d = d0 + u * kExpWaves;
            if (d < d_end) {
                ua = ua + pa[u] * m[u];
                ub = ub + pb[u] * m[u];
                wa = wa + ta[u] * m[u];
                wb = wb + tb[u] * m[u];
            }
        }
    }
    s_acc[wave][0][lane] = ua;
    s_acc[wave][1][lane] = ub;
    s_acc[wave][2][lane] = wa;
    s_acc[wave][3][lane] = wb;
    __syncthreads();
    // thread (i, l): accumulator i of lane l over the four waves, in order; i < 2: the product with p, else with dP
    const int i = tid >> 6, l = tid & 63;
    const double sum = ((s_acc[0][i][l] + s_acc[1][i][l]) + s_acc[2][i][l]) + s_acc[3][i][l];
    const int o = ODD ? o0 + l + 64 * (i & 1) : o0 + 2 * l + (i & 1);
    if (o < Z) (i < 2 ? part : part_dp)[static_cast<size_t>(seg) * Zs + o] = sum;
}
static_assert(kExpWaves == 4 && kExpBlock == 256, "k_exp_grad_dest_u deals destinations over four waves and reduces 4 x 64 accumulators");

// The rest of one backward operator for origin o: k_exp_grad_finish's a, c, dq, lambda and grad_p_drive, operation for operation, and
//   w = (the segments of part_dp in order), 0 for a zero row;  gdest = (pi * q) * w.
// mu == nullptr: mu is zero by construction and no product was formed: a = 0, w = 0, neither part is read.
// dest_t: grad_dest of the hour; accumulate: the hour's second operator adds to what the day's stored.
__global__ __launch_bounds__(kFinishBlock) void k_exp_grad_dest_finish(const double *__restrict__ part, const double *__restrict__ part_dp, int nseg, int Zs,
                                                                    const double *__restrict__ last_t, const int *__restrict__ ell_t,
                                                                    const double *__restrict__ r_t, const double *__restrict__ q_t,
                                                                    const double *__restrict__ pi_s, const double *__restrict__ mu,
                                                                    const double *__restrict__ gp, const double *__restrict__ gd, int Z, int accumulate,
                                                                    double *__restrict__ mu_out, double *grad_t, double *dest_t)
{
    const int o = static_cast<int>(blockIdx.x) * kFinishBlock + static_cast<int>(threadIdx.x);
    if (o >= Z) return;
    const double m = mu ? mu[o] : 0.0;
    double a = 0.0, w = 0.0;
    if (mu) {
        if (last_t[o] == 0.0) {  // a zero row: the driver stays in o (src/resampling.jl:35-36); no entry of the row carries a tangent
            a = m;
        } else {
            const int l = ell_t[o];
            const double rr = r_t[o];
            const double ml = l < Z ? mu[l] : 0.0;
            for (int s0 = 0; s0 < nseg; s0 += kFinishUnroll) {
                double v[kFinishUnroll], t[kFinishUnroll];
#pragma unroll
                for (int u = 0; u < kFinishUnroll; ++u) {
                    v[u] = s0 + u < nseg ? part[static_cast<size_t>(s0 + u) * Zs + o] : 0.0;
                    t[u] = s0 + u < nseg ? part_dp[static_cast<size_t>(s0 + u) * Zs + o] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < kFinishUnroll; ++u)
                    if (s0 + u < nseg) {
                        a = s0 + u == 0 ? v[u] : a + v[u];
                        w = s0 + u == 0 ? t[u] : w + t[u];
                    }
            }
            if (l < Z) a = a + rr * ml;  // the residual goes into a alone: r is held fixed along the tangent
        }
    }
    const double vgp = gp ? gp[o] : 0.0, vgd = gd ? gd[o] : 0.0;
    const double qraw = q_t[o];
    const double q = exp_q(qraw), pi = pi_s[o];
    const double c = (vgd - m) + a;
    const double dq = pi * c;
    mu_out[o] = (vgp + m) + q * c;
    const bool inside = qraw > 0.0 && qraw < 1.0;  // (false for NaN)
    grad_t[o] = inside ? (accumulate ? grad_t[o] + dq : dq) : 0.0;
    const double gdest = (pi * q) * w;
    dest_t[o] = accumulate ? dest_t[o] + gdest : gdest;
}

// ------------------------------------------------------------------ d p_destin / d e_dest, dense route
// l = log(x) of every cell whose installed p > 0 (else 0), x as k_pdest_weights forms it.  grid = (ceil(Z / 256), Z dest).
// TT > 0: the pair's TT means in registers (T = 24); TT == 0: any T, the day is read twice.
template <int TT>
__global__ __launch_bounds__(256) void k_tan_log(const double *__restrict__ dm, const double *__restrict__ p, double *__restrict__ tan, int Z, int T)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = blockIdx.y;
    if (i >= Z) return;
    const size_t base = i + static_cast<size_t>(j) * Z;
    const size_t slab = static_cast<size_t>(Z) * Z;
    if constexpr (TT > 0) {
        double v[TT];
#pragma unroll
        for (int t = 0; t < TT; ++t) v[t] = dm[base + t * slab];
        double mx = v[0], mn = v[0];
#pragma unroll
        for (int t = 1; t < TT; ++t) {
            mx = jl_max(mx, v[t]);
            mn = jl_min(mn, v[t]);
        }
#pragma unroll
        for (int t = 0; t < TT; ++t) {
            double l = 0.0;
            if (mx > 0 && p[base + t * slab] > 0.0) l = log((v[t] - mn) / (mx - mn));
            tan[base + t * slab] = l;
        }
    } else {
        double mx = dm[base], mn = dm[base];
        for (int t = 1; t < T; ++t) {
            const double u = dm[base + t * slab];
            mx = jl_max(mx, u);
            mn = jl_min(mn, u);
        }
        for (int t = 0; t < T; ++t) {
            double l = 0.0;
            if (mx > 0 && p[base + t * slab] > 0.0) l = log((dm[base + t * slab] - mn) / (mx - mn));
            tan[base + t * slab] = l;
        }
    }
}

// m[t][i] = the sum over ascending destinations of p * l, from 0, over the cells with p > 0.  grid = (ceil(Z / 64), T).
constexpr int kTanBatch = 16;
__global__ __launch_bounds__(64) void k_tan_rowsum(const double *__restrict__ p, const double *__restrict__ tan, double *__restrict__ m_out, int Z)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int t = blockIdx.y;
    if (i >= Z) return;
    const size_t off = static_cast<size_t>(t) * Z * Z + i;
    double m = 0.0;
    for (int j0 = 0; j0 < Z; j0 += kTanBatch) {  // loads in batches, sum in order (k_pdest_rowsum; two arrays, so half its batch)
        double pv[kTanBatch], lv[kTanBatch];
#pragma unroll
        for (int u = 0; u < kTanBatch; ++u) {
            const bool in = j0 + u < Z;
            pv[u] = in ? p[off + static_cast<size_t>(j0 + u) * Z] : 0.0;
            lv[u] = in ? tan[off + static_cast<size_t>(j0 + u) * Z] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < kTanBatch; ++u)
            if (pv[u] > 0.0) m = m + pv[u] * lv[u];
    }
    m_out[static_cast<size_t>(t) * Z + i] = m;
}

// dP = p * (l - m) where p > 0, else 0, in place over l.  grid = (ceil(Z / 256), ceil(Z / kDivBatch), T).
__global__ __launch_bounds__(256) void k_tan_final(const double *__restrict__ p, const double *__restrict__ m, double *__restrict__ tan, int Z)
{
    const int t = blockIdx.z, j0 = blockIdx.y * kDivBatch;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Z) return;
    const double mm = m[static_cast<size_t>(t) * Z + i];
    const size_t off = (static_cast<size_t>(t) * Z + j0) * Z + i;
    double pv[kDivBatch], lv[kDivBatch];
#pragma unroll
    for (int u = 0; u < kDivBatch; ++u) {
        const bool in = j0 + u < Z;
        pv[u] = in ? p[off + static_cast<size_t>(u) * Z] : 0.0;
        lv[u] = in ? tan[off + static_cast<size_t>(u) * Z] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kDivBatch; ++u)
        if (j0 + u < Z) tan[off + static_cast<size_t>(u) * Z] = pv[u] > 0.0 ? pv[u] * (lv[u] - mm) : 0.0;
}

// ------------------------------------------------------------------ d p_destin / d e_dest, compact rows
// A lane per (hour, origin) row = t * Z + i: the row's cells in ascending destination, twice -- m, then dP scattered into the zeroed
// dense array (neighbouring lanes are neighbouring origins of one hour).  grid = ceil(rows / 64).
__global__ __launch_bounds__(64) void k_tan_cells(const DsCell *__restrict__ cells, const double *__restrict__ sp, const uint32_t *__restrict__ sj,
                                                  const uint32_t *__restrict__ scnt, uint32_t cap, int64_t rows, int Z, double *__restrict__ tan)
{
    const int64_t row = static_cast<int64_t>(blockIdx.x) * 64 + threadIdx.x;
    if (row >= rows) return;
    const size_t t = static_cast<size_t>(row) / static_cast<size_t>(Z), i = static_cast<size_t>(row) % static_cast<size_t>(Z);
    const uint32_t n = min(scnt[row], cap);
    const size_t at = static_cast<size_t>(row) * cap;
    double m = 0.0;
    for (uint32_t e = 0; e < n; ++e) {
        const double p = sp[at + e];
        if (p > 0.0) m = m + p * log(cells[at + e].x);
    }
    for (uint32_t e = 0; e < n; ++e) {
        const double p = sp[at + e];
        const uint32_t j = sj[at + e];
        if (p > 0.0 && j < static_cast<uint32_t>(Z)) tan[(t * Z + j) * Z + i] = p * (log(cells[at + e].x) - m);
    }
}

// ------------------------------------------------------------------ the tangent of the trip weights
// The segments of k_exp_trip launched on the tangent, in ascending order; 0 for a zero row; no residual term.
// grid = (ceil(Z / 256), T).  part: [nseg][2][T][Z]; dw: [2][T][Z].
__global__ __launch_bounds__(kExpBlock) void k_exp_trip_tan_finish(const double *__restrict__ part, int nseg, const double *__restrict__ last, int Z, int T,
                                                                   double *__restrict__ dw)
{
    const int o = static_cast<int>(blockIdx.x) * kExpBlock + static_cast<int>(threadIdx.x), t = static_cast<int>(blockIdx.y);
    if (o >= Z) return;
    const size_t zt = static_cast<size_t>(Z) * T, row = static_cast<size_t>(t) * Z + o;
    double sec = part[row], km = part[zt + row];
    for (int s = 1; s < nseg; ++s) {
        sec = sec + part[static_cast<size_t>(s) * 2 * zt + row];
        km = km + part[static_cast<size_t>(s) * 2 * zt + zt + row];
    }
    const bool zero_row = last[row] == 0.0;
    dw[row] = zero_row ? 0.0 : sec;
    dw[zt + row] = zero_row ? 0.0 : km;
}

}  // namespace cpm
