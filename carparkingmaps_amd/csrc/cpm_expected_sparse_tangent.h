// cpm_expected_sparse_tangent.h -- the forward tangent of the expected densities from the compact rows of sparse p_destin tables
// (include/cpm_expected_sparse_tangent.h): k_exps_cells_dp, k_exps_tan_hour<NB, WU>.
//
// k_tan_hour (cpm_expected_tangent.h) streams the hour's dense Z x Z block of p under the primal and up to kTanDirs directions, and
// the block of the tangent table dP under the masked primal xm for u.  k_exps_tan_hour is that kernel with the streamed part replaced
// by k_exps_hour's cell-parallel walk of the transposed compact rows (cpm_expected_sparse.h): the stored cells of a destination column,
// sorted by (lane, place in the lane), 256 at a time, the rounded products in LDS, the head of a lane's run adding the run in order
// onto the lane's accumulator.  A cell that is not stored holds p = 0 and dP = 0 in the dense arrays: it adds +-0 to an accumulator
// that starts at +0 and is never -0, for terms of either sign (include/cpm_expected_sparse_tangent.h has the argument), so every
// column sum carries k_tan_hour's bits.  Everything behind the column sums -- exp_block_sum, the residual lists, the epilogue -- is
// k_tan_hour's code, on TanHour's fields and the same workspace.
//
// u rides along.  With WU the walk forms one more product per cell, xm[o] * cell_dp[i], on the origin already in hand: where the dense
// kernel streams a second Z x Z block, this one reads 8 more bytes per stored cell and nothing else.  Passes that read u from the
// workspace, or need none, are instantiated without WU and load no cell_dp.
//
// cell_dp is the compact tangent sdp (entry for entry with the compact rows) carried through the permutation that made cell_p of sp:
// k_exps_cells_dp finds each cell of a column in its origin's row, which is sorted by destination on both routes (k_ds_sort;
// k_up_compact emits ascending destinations), with the search k_exps_tan_check already relies on.
//
// Separate kernels in a header of their own: no existing kernel moves.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cpm_expected_sparse.h"
#include "cpm_expected_sparse_dest.h"
#include "cpm_expected_tangent.h"

namespace cpm {

// cell_dp[i] = sdp[row(t, cell_o[i]) * cap + e], e the place of destination d in that row, for every cell i of column (t, d); +0.0
// for a cell the row does not hold (there is none: the columns were filled from these rows).  Every word is written, each by one
// thread; no atomics.  grid = (Z, T).
__global__ __launch_bounds__(kExpBlock) void k_exps_cells_dp(const uint32_t *__restrict__ colptr, const uint32_t *__restrict__ cell_o,
                                                             const double *__restrict__ sdp, const uint32_t *__restrict__ sj,
                                                             const uint32_t *__restrict__ scnt, uint32_t cap, int Z, double *__restrict__ cell_dp)
{
    const uint32_t d = blockIdx.x;
    const size_t t = blockIdx.y;
    const size_t col = t * (static_cast<size_t>(Z) + 1) + d;
    const uint32_t a = colptr[col], n = colptr[col + 1] - a;
    for (uint32_t i = threadIdx.x; i < n; i += kExpBlock) {
        const uint32_t o = cell_o[a + i];
        double v = 0.0;
        if (o < static_cast<uint32_t>(Z)) {
            const size_t row = t * static_cast<size_t>(Z) + o;
            const uint32_t m = min(scnt[row], cap);
            const uint32_t e = exps_find_cell(sj + row * cap, m, d);
            if (e < m) v = sdp[row * cap + e];
        }
        cell_dp[a + i] = v;
    }
}

// What one launch of k_exps_tan_hour reads and writes: TanHour (p_t and dp_t unused) and the hour's transposed compact rows.
struct ExpsTanHour {
    TanHour h;
    const uint32_t *colptr_t;  // the hour's [Z + 1] slice: offsets into the whole cell arrays
    const uint32_t *cell_o;
    const double *cell_p;
    const double *cell_dp;     // read when h.u_mode == 1 (WU)
    int par;                   // t & 1
};

// One operator for the primal and the nv - 1 <= NB - 1 directions of a pass.  grid = ceil(Z / kExpRows).  WU <=> h.u_mode == 1.
template <int NB, bool WU>
__global__ __launch_bounds__(kExpBlock) void k_exps_tan_hour(const ExpsTanHour b)
{
    constexpr int NV = NB + (WU ? 1 : 0);  // vectors of the walk: vector NB is xm against cell_dp
    __shared__ double s_part[kExpWaves * kExpRows * NB];
    __shared__ double s_y[kExpRows * NB];
    __shared__ double s_res[kExpRows * NB];
    __shared__ double s_u[kExpRows];
    __shared__ double s_acc[NV][kExpBlock];   // the lanes' accumulators of the column in hand
    __shared__ double s_prod[NV][kExpBlock];  // the chunk's products
    __shared__ uint32_t s_lane[kExpBlock];    // ... and their lanes (kExpsNoLane: no cell)
    const TanHour &a = b.h;
    const int tid = static_cast<int>(threadIdx.x);
    const int Z = a.Z, Zs = a.Zs, nv = a.nv;
    const int d0 = static_cast<int>(blockIdx.x) * kExpRows;
    const bool odd = (Z & 1) != 0;
    const uint32_t uz = static_cast<uint32_t>(Z), utid = static_cast<uint32_t>(tid);

    const double *xf[NB];
#pragma unroll
    for (int f = 0; f < NB; ++f) xf[f] = a.x_in + static_cast<size_t>(f < nv ? f : nv - 1) * Zs;

    uint32_t ca[kExpRows], cn[kExpRows], o1[kExpRows];
    double p1[kExpRows], t1[kExpRows];
#pragma unroll
    for (int r = 0; r < kExpRows; ++r) {
        const int d = d0 + r;
        uint32_t c0 = 0, c1 = 0;
        if (d < Z) {
            c0 = b.colptr_t[d];
            c1 = b.colptr_t[d + 1];
        }
        ca[r] = c0;
        cn[r] = c1 - c0;
    }
#pragma unroll
    for (int r = 0; r < kExpRows; ++r) {  // the first chunk of every column: all in flight together
        o1[r] = 0;
        p1[r] = 0.0;
        t1[r] = 0.0;
        if (utid < cn[r]) {
            o1[r] = __builtin_nontemporal_load(b.cell_o + ca[r] + utid);
            p1[r] = __builtin_nontemporal_load(b.cell_p + ca[r] + utid);
            if (WU) t1[r] = __builtin_nontemporal_load(b.cell_dp + ca[r] + utid);
        }
    }

    double acc[kExpRows * NB], accu[kExpRows];
#pragma unroll
    for (int r = 0; r < kExpRows; ++r) {
        const bool hd = exps_head(odd, b.par, d0 + r);
#pragma unroll
        for (int f = 0; f < NV; ++f) s_acc[f][tid] = 0.0;
        for (uint32_t c = 0; c < cn[r]; c += kExpBlock) {  // (uniform over the workgroup)
            const uint32_t i = c + utid;
            const bool in = i < cn[r];
            uint32_t o = o1[r];
            double p = p1[r], tv = t1[r];
            if (c != 0) {
                o = 0;
                p = 0.0;
                tv = 0.0;
                if (in) {
                    o = __builtin_nontemporal_load(b.cell_o + ca[r] + i);
                    p = __builtin_nontemporal_load(b.cell_p + ca[r] + i);
                    if (WU) tv = __builtin_nontemporal_load(b.cell_dp + ca[r] + i);
                }
            }
            const uint32_t lane = in ? exps_key(o, uz, hd) >> kExpsLaneShift : kExpsNoLane;
            s_lane[tid] = lane;
#pragma unroll
            for (int f = 0; f < NB; ++f) s_prod[f][tid] = in ? xf[f][o] * p : 0.0;
            if (WU) s_prod[NV - 1][tid] = in ? a.xm_in[o] * tv : 0.0;
            __syncthreads();
            if (in && (tid == 0 || s_lane[tid - 1] != lane)) {  // the head of a run: the lane's cells of this chunk, in order
                double v[NV];
#pragma unroll
                for (int f = 0; f < NV; ++f) v[f] = s_acc[f][lane];
                int j = tid;
                do {
#pragma unroll
                    for (int f = 0; f < NV; ++f) v[f] = v[f] + s_prod[f][j];
                    ++j;
                } while (j < kExpBlock && s_lane[j] == lane);
#pragma unroll
                for (int f = 0; f < NV; ++f) s_acc[f][lane] = v[f];
            }
            __syncthreads();
        }
#pragma unroll
        for (int f = 0; f < NB; ++f) acc[r * NB + f] = s_acc[f][tid];
        accu[r] = WU ? s_acc[NV - 1][tid] : 0.0;
    }
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

    if (WU) {  // u of these destinations: the lanes' sums of xm * dP, reduced as k_tan_hour reduces them
        exp_block_sum<kExpRows>(accu, s_part, s_u);
        if (tid < kExpRows && d0 + tid < Z) a.u[d0 + tid] = s_u[tid];
    }
    __syncthreads();

    // k_tan_hour's epilogue, operation for operation
    if (tid >= kExpRows * NB) return;
    const int r = tid / NB, f = tid % NB, d = d0 + r;
    if (d >= Z || f >= nv) return;
    const bool zero_row = a.last_t[d] == 0.0;
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
    if (c != 0.0) v = v + c * (WU ? s_u[r] : a.u[d]);
    a.pi_out[i] = v;
    if (a.dpark) a.dpark[k * a.out_stride + d] = v;
    if (a.q_next) {
        const double dqn = tan_dq(qnr, a.dq_next, k * a.dq_stride + d);
        const double t1n = v * qn, t2n = v0 * dqn;
        const double dxn = t1n + t2n;
        a.x_out[i] = dxn;
        if (a.ddrv) a.ddrv[k * a.out_stride + d] = dxn;
    }
}

}  // namespace cpm
