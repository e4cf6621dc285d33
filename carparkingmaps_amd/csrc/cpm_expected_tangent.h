// cpm_expected_tangent.h -- forward tangent of the expected densities (include/cpm_expected_tangent.h): k_tan_init, k_tan_hour<NB>,
// k_tan_pdrive.
//
// A tangent obeys the recurrence of the densities themselves, d pi_{s+1} = dstay + dx * P (+ residuals, zero rows), with signed inputs
// and another epilogue; the primal x is shared by all directions.  k_tan_hour<NB> is therefore k_exp_hour<NB> (cpm_expected.h) with the
// primal as vector 0 of the pass and up to kTanDirs directions as vectors 1 .. NB - 1: the hour's Z x Z block of p is read ONCE for the
// primal and seven tangents, by the same exp_stream and exp_block_sum, which keep one accumulator per (row, vector) -- the order of a
// sum is a function of Z, the row's alignment and the table, never of the vector's place or of how many ride along.  The primal's
// epilogue is k_exp_hour's operation for operation: the bits of cpm_expected_dev.
//
// u[d] = sum over o of x[o] * dP[t][d][o] (the product of the primal with the tangent table of p_destin) is one more exp_stream<1>
// over the dP rows of the same destinations in the same workgroup, on xm: the primal x with the origins of zero rows set to 0, which
// the epilogue of the operator in front (or k_tan_init) leaves next to x.  Only the first pass of an operator computes u; it leaves
// it in the workspace for the passes behind it on the stream.
//
// The vectors lie Zs = Z rounded up to even words apart in the workspace: every vector starts on a 16-byte line, as exp_stream's
// 16-byte loads of x need, whatever the parity of Z.  Stores are single words.
//
// Separate kernels in a header of their own: the hourly sampler's code and k_exp_hour do not move.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cpm_expected.h"
#include "cpm_tables.h"

namespace cpm {

constexpr int kTanDirs = kExpMaxNB - 1;  // directions of a pass: the primal takes vector 0

// dq of the definition: the direction's entry where the installed p_drive is strictly inside (0, 1), else exactly 0 (a select: a NaN
// in the direction table does not pass)
__device__ __forceinline__ double tan_dq(double p_drive, const double *__restrict__ dq, size_t i)
{
    if (!dq || !(p_drive > 0.0 && p_drive < 1.0)) return 0.0;
    return dq[i];
}

// What one launch of k_tan_hour reads and writes.  Pointers that carry a direction stride point at the pass's first direction.
struct TanHour {
    const double *p_t, *last_t, *r_t;  // the hour's slices of p, last and r
    const int *start_t, *list_t;       // ... and of the residual lists
    const double *last_next;           // last of the next operator's hour (for xm_out); nullptr when nothing follows
    const double *dp_t;                // the hour's Z x Z block of the tangent table; read when u_mode == 1
    double *u;                         // [Z] u of this operator: written when u_mode == 1, read when u_mode == 2
    int u_mode;                        // 0: no direction of the call has a c_dest; 1: compute u and keep it; 2: read it
    const double *q_cur, *q_next;      // the installed p_drive of this and the next operator's hour; q_next nullptr: nothing follows
    const double *dq_cur, *dq_next;    // the directions' d p_drive slices of those hours, dq_stride words apart; nullptr: all zero
    size_t dq_stride;
    const double *pi_in, *x_in, *xm_in;  // [NB][Zs] pi | d pi and x | dx of the pass, vector 0 the primal; xm_in: [Zs]
    double *pi_out, *x_out, *xm_out;     // xm_out nullptr: not wanted
    double *park0, *drv0;                // where the primal's pi_next and x_next also go, or nullptr
    double *dpark, *ddrv;                // where the directions' go, out_stride words apart, or nullptr
    size_t out_stride;
    double c[kExpMaxNB];  // c_dest of vectors 1 .. (c[0] unused)
    int Z, Zs, nv;        // nv: vectors of the pass, the primal included
};

// pi_0, x_0 and xm_0 of the primal and d pi_0, dx_0 of the nv - 1 directions of a pass into the workspace (and, when the day starts
// here, into hour 0 of the outputs).  grid = (ceil(Z/256), nv).  pi0 / dpi0: nullptr = uniform 1 / Z / zero.  dpi0: [.][Z].
__global__ __launch_bounds__(kExpBlock) void k_tan_init(const double *__restrict__ pi0, const double *__restrict__ dpi0, const double *__restrict__ q0,
                                                        const double *__restrict__ dq0, size_t dq_stride, const double *__restrict__ last0, int Z,
                                                        int Zs, double *__restrict__ ws_pi, double *__restrict__ ws_x, double *__restrict__ ws_xm,
                                                        double *__restrict__ park0, double *__restrict__ drv0, double *__restrict__ dpark,
                                                        double *__restrict__ ddrv, size_t out_stride)
{
    const int z = static_cast<int>(blockIdx.x) * kExpBlock + static_cast<int>(threadIdx.x), f = static_cast<int>(blockIdx.y);
    if (z >= Z) return;
    const double pi = pi0 ? pi0[z] : 1.0 / static_cast<double>(Z);
    const double qr = q0[z], q = exp_q(qr);
    if (f == 0) {
        const double x = pi * q;
        ws_pi[z] = pi;
        ws_x[z] = x;
        if (ws_xm) ws_xm[z] = last0[z] == 0.0 ? 0.0 : x;
        if (park0) {
            park0[z] = pi;
            drv0[z] = x;
        }
        return;
    }
    const size_t k = static_cast<size_t>(f - 1);
    const double dpi = dpi0 ? dpi0[k * Z + z] : 0.0;
    const double dq = tan_dq(qr, dq0, k * dq_stride + z);
    const double a = dpi * q, b = pi * dq;
    const double dx = a + b;
    ws_pi[static_cast<size_t>(f) * Zs + z] = dpi;
    ws_x[static_cast<size_t>(f) * Zs + z] = dx;
    if (dpark) {
        dpark[k * out_stride + z] = dpi;
        ddrv[k * out_stride + z] = dx;
    }
}

// One operator for the primal and the nv - 1 <= NB - 1 directions of a pass.  grid = ceil(Z / kExpRows).  Launched with NB = 2, 4, 5
// and 8: five vectors are K = 4, the model's four parameters, which the eight-vector form runs at 2 waves / SIMD.
template <int NB>
__global__ __launch_bounds__(kExpBlock) void k_tan_hour(const TanHour a)
{
    __shared__ double s_part[kExpWaves * kExpRows * NB];
    __shared__ double s_y[kExpRows * NB];
    __shared__ double s_res[kExpRows * NB];
    __shared__ double s_u[kExpRows];
    const int tid = static_cast<int>(threadIdx.x);
    const int Z = a.Z, Zs = a.Zs, nv = a.nv;
    const int d0 = static_cast<int>(blockIdx.x) * kExpRows;
    const bool odd = (Z & 1) != 0;

    // (a row past the end repeats one of the last two, the one that starts where it would: computed, not stored)
    size_t row_at[kExpRows];
#pragma unroll
    for (int r = 0; r < kExpRows; ++r) {
        int d = d0 + r;
        if (d >= Z) d -= 2 * ((d - Z) / 2 + 1);
        row_at[r] = static_cast<size_t>(d > 0 ? d : 0) * Z;
    }
    {
        const double *row[kExpRows];
#pragma unroll
        for (int r = 0; r < kExpRows; ++r) row[r] = a.p_t + row_at[r];
        const bool h0 = odd && ((reinterpret_cast<uintptr_t>(row[0]) >> 3) & 1u) != 0;
        const double *xf[NB];
#pragma unroll
        for (int f = 0; f < NB; ++f) xf[f] = a.x_in + static_cast<size_t>(f < nv ? f : nv - 1) * Zs;

        double acc[kExpRows * NB];
#pragma unroll
        for (int i = 0; i < kExpRows * NB; ++i) acc[i] = 0.0;
        if (!odd) exp_stream<NB, false, false>(row, xf, Z, acc);
        else if (h0) exp_stream<NB, true, true>(row, xf, Z, acc);
        else exp_stream<NB, true, false>(row, xf, Z, acc);
        exp_block_sum<kExpRows * NB>(acc, s_part, s_y);

        // the residuals that arrive at these destinations, as in k_exp_hour
        for (int r = 0; r < kExpRows; ++r) {
            const int d = d0 + r;
            int ka = 0, kb = 0;
            if (d < Z) {
                ka = a.start_t[d];
                kb = a.start_t[d + 1];
            }
            if (kb > ka) {  // (uniform over the workgroup)
                double a2[NB];
#pragma unroll
                for (int f = 0; f < NB; ++f) a2[f] = 0.0;
                for (int k = ka + tid; k < kb; k += kExpBlock) {
                    const int o = a.list_t[k];
                    const double rr = a.r_t[o];
#pragma unroll
                    for (int f = 0; f < NB; ++f) a2[f] = a2[f] + xf[f][o] * rr;
                }
                exp_block_sum<NB>(a2, s_part, s_res + r * NB);
            } else if (tid < NB) {
                s_res[r * NB + tid] = 0.0;
            }
        }
    }

    if (a.u_mode == 1) {  // (uniform over the grid) u of these destinations: the same stream over the rows of dP, on the masked primal
        const double *row[kExpRows];
#pragma unroll
        for (int r = 0; r < kExpRows; ++r) row[r] = a.dp_t + row_at[r];
        const bool h0 = odd && ((reinterpret_cast<uintptr_t>(row[0]) >> 3) & 1u) != 0;
        const double *xf[1] = {a.xm_in};
        double acc[kExpRows];
#pragma unroll
        for (int i = 0; i < kExpRows; ++i) acc[i] = 0.0;
        if (!odd) exp_stream<1, false, false>(row, xf, Z, acc);
        else if (h0) exp_stream<1, true, true>(row, xf, Z, acc);
        else exp_stream<1, true, false>(row, xf, Z, acc);
        exp_block_sum<kExpRows>(acc, s_part, s_u);
        if (tid < kExpRows && d0 + tid < Z) a.u[d0 + tid] = s_u[tid];
    }
    __syncthreads();

    if (tid >= kExpRows * NB) return;
    const int r = tid / NB, f = tid % NB, d = d0 + r;
    if (d >= Z || f >= nv) return;
    const bool zero_row = a.last_t[d] == 0.0;
    // the primal: k_exp_hour's epilogue, operation for operation (every thread of the row forms it: the directions read it)
    const double pi = a.pi_in[d];
    const double qr = a.q_cur[d], q = exp_q(qr);
    double v0 = pi * (1.0 - q) + s_y[r * NB];
    v0 = v0 + s_res[r * NB];
    if (zero_row) v0 = v0 + a.x_in[d];
    const double qnr = a.q_next ? a.q_next[d] : 0.0, qn = exp_q(qnr);
    if (f == 0) {
        a.pi_out[d] = v0;
        if (a.park0) a.park0[d] = v0;
        if (a.q_next) {
            const double xn = v0 * qn;
            a.x_out[d] = xn;
            if (a.drv0) a.drv0[d] = xn;
            if (a.xm_out) a.xm_out[d] = a.last_next[d] == 0.0 ? 0.0 : xn;
        }
        return;
    }
    const size_t k = static_cast<size_t>(f - 1), i = static_cast<size_t>(f) * Zs + d;
    const double dpi = a.pi_in[i];
    const double dq = tan_dq(qr, a.dq_cur, k * a.dq_stride + d);
    const double s1 = dpi * (1.0 - q), s2 = pi * dq;
    const double dstay = s1 - s2;
    double v = dstay + s_y[tid];
    v = v + s_res[tid];
    if (zero_row) v = v + a.x_in[i];
    const double c = a.c[f];
    if (c != 0.0) v = v + c * (a.u_mode == 1 ? s_u[r] : a.u[d]);
    a.pi_out[i] = v;
    if (a.dpark) a.dpark[k * a.out_stride + d] = v;
    if (a.q_next) {
        const double dqn = tan_dq(qnr, a.dq_next, k * a.dq_stride + d);
        const double t1 = v * qn, t2 = v0 * dqn;
        const double dxn = t1 + t2;
        a.x_out[i] = dxn;
        if (a.ddrv) a.ddrv[k * a.out_stride + d] = dxn;
    }
}

// The three direction tables d p_drive / d (p_min, p_max, e_drive) from mean_sum, with the s, s^e and log of k_fit_chain
// (cpm_expected_fit.h); mn / mx as k_pdrive_final forms them.  out: [3][T][Z].  grid = (ceil(Z/64), T), 64 threads.
__global__ void k_tan_pdrive(const double *__restrict__ mean_sum, double *__restrict__ out, int Z, int T, double p_min, double p_max, double e_drive)
{
    const int z = blockIdx.x * blockDim.x + threadIdx.x;
    const int t = blockIdx.y;
    if (z >= Z) return;
    double mx = mean_sum[z], mn = mean_sum[z];
    for (int h = 1; h < T; ++h) {
        const double v = mean_sum[z + static_cast<size_t>(h) * Z];
        mx = jl_max(mx, v);
        mn = jl_min(mn, v);
    }
    double d_min = 0.0, d_max = 0.0, d_e = 0.0;
    if (mx > 0) {
        const double s = (mean_sum[z + static_cast<size_t>(t) * Z] - mn) / (mx - mn);
        const double se = pow_f64(s, e_drive);
        d_min = 1.0 - se;
        d_max = se;
        if (s > 0.0) d_e = (p_max - p_min) * (se * log(s));
    }
    const size_t zt = static_cast<size_t>(Z) * T, i = z + static_cast<size_t>(t) * Z;
    out[i] = d_min;
    out[zt + i] = d_max;
    out[2 * zt + i] = d_e;
}

}  // namespace cpm
