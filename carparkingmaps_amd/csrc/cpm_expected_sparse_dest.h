// cpm_expected_sparse_dest.h -- the adjoint along a tangent of p_destin from the compact rows of sparse tables
// (include/cpm_expected_sparse_dest.h): k_exps_tan_cells, k_exps_grad_dest_u, k_exps_grad_dest_u_b<NB>, and the kernels that move a
// host tangent onto the stored cells and back (k_exps_tan_check, k_exps_tan_gather, k_exps_tan_scatter).
//
// The compact tangent sdp is f64 [T * Z][cap], word e of a row the tangent at the cell sj[row * cap + e], entry for entry with sp.
// The backward product along it, w[o] = sum over d of dP[t][d][o] * mu[d], is a sum along origin o's own row like u, so the walk of
// cpm_expected_sparse_grad.h carries it with a second value per cell: exps_row_walk2 below is exps_row_walk with the row of sdp
// loaded beside the row of sp (the first four chunks of both in flight together), mu[d] gathered once and used for both products --
// 2 * NB products per cell for the NB fleets of a pass, dealt to NB / kExpsDestFleets waves per row.  Segment, chain and order are
// those of the walk, which are those of k_exp_grad_dest_u (cpm_expected_grad_dest.h): segment s = d / seg_len, chain
// (d - s * seg_len) & 3, ascending d from +0, ((w0 + w1) + w2) + w3.  The chains of u are those of k_exps_grad_u operation for operation, so `part` carries that kernel's bits.
// Every word part[s][o] and part_dp[s][o], s < nseg, o < Z, is written, +0 for chains and segments without cells: the unchanged
// finishing kernels (k_exp_grad_dest_finish, k_exp_grad_dest_finish_b) read them.
//
// The tangent of the trip weights needs no kernel of its own: it is k_exps_trip (cpm_expected_sparse_grad.h) launched with the rows of
// sdp in place of those of sp, as the dense call launches k_exp_trip on the dense tangent.
//
// k_exps_tan_cells is k_tan_cells (cpm_expected_grad_dest.h) with the store into the row of sdp instead of the scatter into a zeroed
// dense array: the same lane per row, the same two passes, the same operations per cell.
//
// Separate kernels in a header of their own: no existing kernel moves.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cpm_dataset.h"
#include "cpm_expected_sparse_grad.h"

namespace cpm {

// exps_row_walk with two stored values per cell, p and dP.  term(d, pv, tv, prod) forms the cell's NV rounded products.
template <int NV, class Term>
__device__ __forceinline__ void exps_row_walk2(const double *__restrict__ row_p, const double *__restrict__ row_dp, const uint32_t *__restrict__ row_j,
                                               uint32_t n, uint32_t Z, uint32_t seg_len, Term term, double (&sum)[NV])
{
    __shared__ double s_prod[NV][kExpsGradBlock];
    __shared__ uint32_t s_key[kExpsGradBlock];
    __shared__ int s_start[kExpsGradBlock];
    const uint32_t lane = threadIdx.x;
    double a0[NV], a1[NV], a2[NV], a3[NV];
#pragma unroll
    for (int f = 0; f < NV; ++f) a0[f] = a1[f] = a2[f] = a3[f] = 0.0;
    uint32_t d_ahead[kExpsGradAhead];
    double p_ahead[kExpsGradAhead], t_ahead[kExpsGradAhead];
#pragma unroll
    for (int u = 0; u < kExpsGradAhead; ++u) {
        const uint32_t e = static_cast<uint32_t>(u) * kExpsGradBlock + lane;
        d_ahead[u] = 0;
        p_ahead[u] = t_ahead[u] = 0.0;
        if (e < n) {
            d_ahead[u] = row_j[e];
            p_ahead[u] = row_p[e];
            t_ahead[u] = row_dp[e];
        }
    }
    for (uint32_t c = 0; c < n; c += kExpsGradBlock) {  // (uniform over the wave)
        const uint32_t e = c + lane, chunk = c / kExpsGradBlock;
        uint32_t key = kExpsNoKey, d = 0;
        double pv = 0.0, tv = 0.0;
        if (e < n) {
            if (chunk < kExpsGradAhead) {
#pragma unroll
                for (int u = 0; u < kExpsGradAhead; ++u) {
                    d = chunk == static_cast<uint32_t>(u) ? d_ahead[u] : d;
                    pv = chunk == static_cast<uint32_t>(u) ? p_ahead[u] : pv;
                    tv = chunk == static_cast<uint32_t>(u) ? t_ahead[u] : tv;
                }
            } else {
                d = row_j[e];
                pv = row_p[e];
                tv = row_dp[e];
            }
            if (d < Z) {  // (the builders skip cells beyond the table as well)
                const uint32_t s = d / seg_len;
                key = (s << 2) | ((d - s * seg_len) & 3u);
            }
        }
        double prod[NV];
#pragma unroll
        for (int f = 0; f < NV; ++f) prod[f] = 0.0;
        if (key != kExpsNoKey) term(d, pv, tv, prod);
        s_key[lane] = key;
        s_start[lane] = -1;
#pragma unroll
        for (int f = 0; f < NV; ++f) s_prod[f][lane] = prod[f];
        __syncthreads();
        if (key != kExpsNoKey && (lane == 0 || (s_key[lane - 1] >> 2) != (key >> 2))) s_start[key >> 2] = static_cast<int>(lane);
        __syncthreads();
        int k = s_start[lane];
        if (k >= 0) {  // the run of segment `lane` in this chunk, in order
            do {
                const uint32_t v = s_key[k] & 3u;
#pragma unroll
                for (int f = 0; f < NV; ++f) {
                    double a = v == 0 ? a0[f] : v == 1 ? a1[f] : v == 2 ? a2[f] : a3[f];
                    a = a + s_prod[f][k];
                    a0[f] = v == 0 ? a : a0[f];
                    a1[f] = v == 1 ? a : a1[f];
                    a2[f] = v == 2 ? a : a2[f];
                    a3[f] = v == 3 ? a : a3[f];
                }
                ++k;
            } while (k < kExpsGradBlock && (s_key[k] >> 2) == lane);
        }
        __syncthreads();  // (the next chunk overwrites what the walk reads)
    }
#pragma unroll
    for (int f = 0; f < NV; ++f) sum[f] = ((a0[f] + a1[f]) + a2[f]) + a3[f];
}

// grid = Z, one wave per origin.  sp_t / sdp_t / sj_t / scnt_t: the hour's rows.  part, part_dp: [nseg][Zs]; every word s < nseg,
// o < Z of both is written.
__global__ __launch_bounds__(kExpsGradBlock) void k_exps_grad_dest_u(const double *__restrict__ sp_t, const double *__restrict__ sdp_t,
                                                                     const uint32_t *__restrict__ sj_t, const uint32_t *__restrict__ scnt_t, uint32_t cap,
                                                                     const double *__restrict__ mu, int Z, int Zs, int seg_len, int nseg,
                                                                     double *__restrict__ part, double *__restrict__ part_dp)
{
    const size_t o = blockIdx.x;
    const uint32_t n = min(scnt_t[o], cap);
    double sum[2];
    exps_row_walk2<2>(sp_t + o * cap, sdp_t + o * cap, sj_t + o * cap, n, static_cast<uint32_t>(Z), static_cast<uint32_t>(seg_len),
                      [mu](uint32_t d, double pv, double tv, double (&prod)[2]) {
                          const double m = mu[d];
                          prod[0] = pv * m;
                          prod[1] = tv * m;
                      },
                      sum);
    const int s = static_cast<int>(threadIdx.x);
    if (s < nseg) {
        part[static_cast<size_t>(s) * Zs + o] = sum[0];
        part_dp[static_cast<size_t>(s) * Zs + o] = sum[1];
    }
}

// ... for the nf <= NB fleets of a pass.  mu: the pass's [Zs][NB]; part, part_dp: [nseg][kExpMaxNB][Zs], fleets >= nf are not stored.
// Per fleet the chains are those of k_exps_grad_dest_u operation for operation.  grid = (Z, ceil(nf / kExpsDestFleets)): a wave takes
// kExpsDestFleets fleets of its origin's row, 2 * kExpsDestFleets products per cell.  The walk is a chain of LDS reads and selects per
// cell, bound by its latency and not by the bytes of the row (which the second wave finds in the cache): all eight fleets in one wave
// (64 f64 accumulators, 225 VGPRs, two waves per SIMD) took 1.8 times the dense kernel's time at Melbourne's shape
// (profiles/expected_sparse_dest_notes.md).
constexpr int kExpsDestFleets = 2;
template <int NB>
__global__ __launch_bounds__(kExpsGradBlock) void k_exps_grad_dest_u_b(const double *__restrict__ sp_t, const double *__restrict__ sdp_t,
                                                                       const uint32_t *__restrict__ sj_t, const uint32_t *__restrict__ scnt_t, uint32_t cap,
                                                                       const double *__restrict__ mu, int Z, int Zs, int seg_len, int nseg, int nf,
                                                                       double *__restrict__ part, double *__restrict__ part_dp)
{
    const size_t o = blockIdx.x;
    const uint32_t n = min(scnt_t[o], cap);
    static_assert(NB % kExpsDestFleets == 0, "a pass is dealt in whole groups of fleets");
    constexpr int NF = kExpsDestFleets;
    const int f0 = static_cast<int>(blockIdx.y) * NF;  // (f0 + NF <= NB: the grid has at most NB / NF groups)
    double sum[2 * NF];
    exps_row_walk2<2 * NF>(sp_t + o * cap, sdp_t + o * cap, sj_t + o * cap, n, static_cast<uint32_t>(Z), static_cast<uint32_t>(seg_len),
                           [mu, f0](uint32_t d, double pv, double tv, double (&prod)[2 * NF]) {
                               const double *__restrict__ mrow = mu + static_cast<size_t>(d) * NB + f0;
#pragma unroll
                               for (int f = 0; f < NF; ++f) {
                                   const double m = mrow[f];
                                   prod[f] = pv * m;
                                   prod[NF + f] = tv * m;
                               }
                           },
                           sum);
    const int s = static_cast<int>(threadIdx.x);
    if (s < nseg) {
#pragma unroll
        for (int f = 0; f < NF; ++f)
            if (f0 + f < nf) {
                part[(static_cast<size_t>(s) * kExpMaxNB + f0 + f) * Zs + o] = sum[f];
                part_dp[(static_cast<size_t>(s) * kExpMaxNB + f0 + f) * Zs + o] = sum[NF + f];
            }
    }
}

// ------------------------------------------------------------------ d p_destin / d e_dest onto the stored cells
// A lane per (hour, origin) row, as in k_tan_cells: m = m + p * log(x) over the cells with p > 0 in ascending destination, then
// p * (log(x) - m) where p > 0 and the destination lies inside the table, else +0; the words behind the row's cells are zeroed too.
// grid = ceil(rows / 64).
__global__ __launch_bounds__(64) void k_exps_tan_cells(const DsCell *__restrict__ cells, const double *__restrict__ sp, const uint32_t *__restrict__ sj,
                                                       const uint32_t *__restrict__ scnt, uint32_t cap, int64_t rows, int Z, double *__restrict__ sdp)
{
    const int64_t row = static_cast<int64_t>(blockIdx.x) * 64 + threadIdx.x;
    if (row >= rows) return;
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
        double v = 0.0;
        if (p > 0.0 && j < static_cast<uint32_t>(Z)) v = p * (log(cells[at + e].x) - m);
        sdp[at + e] = v;
    }
    for (uint32_t e = n; e < cap; ++e) sdp[at + e] = 0.0;
}

// ------------------------------------------------------------------ a host tangent onto the stored cells, and back
// Where destination d stands in a row (sorted by destination; cells beyond the table sort last), or n.
__device__ __forceinline__ uint32_t exps_find_cell(const uint32_t *__restrict__ row_j, uint32_t n, uint32_t d)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (row_j[mid] < d) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && row_j[lo] == d ? lo : n;
}

// stage: one hour's [Z dest][Z origin] block.  A non-zero word at a cell the hour's rows do not store lowers *bad to its index in
// the whole [T][Z][Z] array (cell_base = t * Z * Z).  grid = (ceil(Z / 256), Z dest); lanes are origins.
__global__ __launch_bounds__(256) void k_exps_tan_check(const double *__restrict__ stage, const uint32_t *__restrict__ sj_t, const uint32_t *__restrict__ scnt_t,
                                                        uint32_t cap, int Z, unsigned long long cell_base, unsigned long long *__restrict__ bad)
{
    const int o = static_cast<int>(blockIdx.x) * 256 + static_cast<int>(threadIdx.x);
    const uint32_t d = blockIdx.y;
    if (o >= Z) return;
    const size_t cell = static_cast<size_t>(d) * Z + o;
    if (stage[cell] == 0.0) return;
    const uint32_t n = min(scnt_t[o], cap);
    if (exps_find_cell(sj_t + static_cast<size_t>(o) * cap, n, d) == n) atomicMin(bad, cell_base + cell);
}

// sdp_t[o][e] = stage[sj[e]][o] for the stored cells inside the table, +0 for every other word of the row.
// grid = (ceil(cap / 64), Z origins): a wave per 64 words of a row.
__global__ __launch_bounds__(64) void k_exps_tan_gather(const double *__restrict__ stage, const uint32_t *__restrict__ sj_t, const uint32_t *__restrict__ scnt_t,
                                                        uint32_t cap, int Z, double *__restrict__ sdp_t)
{
    const uint32_t e = blockIdx.x * 64 + threadIdx.x;
    const size_t o = blockIdx.y;
    if (e >= cap) return;
    const uint32_t n = min(scnt_t[o], cap);
    double v = 0.0;
    if (e < n) {
        const uint32_t d = sj_t[o * cap + e];
        if (d < static_cast<uint32_t>(Z)) v = stage[static_cast<size_t>(d) * Z + o];
    }
    sdp_t[o * cap + e] = v;
}

// stage[sj[e]][o] = sdp_t[o][e] for the stored cells inside the table (the block was zeroed).  Same grid.
__global__ __launch_bounds__(64) void k_exps_tan_scatter(const double *__restrict__ sdp_t, const uint32_t *__restrict__ sj_t, const uint32_t *__restrict__ scnt_t,
                                                         uint32_t cap, int Z, double *__restrict__ stage)
{
    const uint32_t e = blockIdx.x * 64 + threadIdx.x;
    const size_t o = blockIdx.y;
    if (e >= cap) return;
    const uint32_t n = min(scnt_t[o], cap);
    if (e >= n) return;
    const uint32_t d = sj_t[o * cap + e];
    if (d < static_cast<uint32_t>(Z)) stage[static_cast<size_t>(d) * Z + o] = sdp_t[o * cap + e];
}

}  // namespace cpm
