// cpm_expected_sparse_grad.h -- the backward operator and the trip weights from the compact rows of sparse p_destin tables
// (include/cpm_expected_sparse_grad.h): k_exps_grad_u, k_exps_grad_u_b<NB>, k_exps_trip.
//
// The backward product u[o] = sum over d of p[t][d][o] * mu[d] is a sum along origin o's OWN row, and that row is what d_sp / d_sj /
// d_scnt store, sorted by destination: no transpose and no per-table array.  k_exp_grad_u (cpm_expected_grad.h) fixes the order of the
// sum: destination d belongs to segment s = d / seg_len and, inside it, to chain v = (d - s * seg_len) & 3 (the wave of the dense
// kernel that is dealt d); a chain starts at +0 and adds acc = acc + p * mu[d] in ascending d; the four chains of a segment are added
// as ((w0 + w1) + w2) + w3.  A cell with p = 0 adds +-0 for finite mu, and a chain that starts at +0 and is +0 or non-zero after every
// step never becomes -0 (+0 + -0 = +0, exact cancellation rounds to +0): skipping it changes no bit.  So the kernels here give every
// STORED cell with d < Z to chain (s, v) in ascending d and write +0 for chains and segments without cells -- every word part[s][o],
// s < nseg, o < Z, the empty trailing segments of sizes like Z = 1,089 included, because the unchanged finishing kernels read them.
//
// One wave per origin row (a one-wave workgroup, so its barriers cost nothing and no loop has to be uniform over rows).  The row's
// cells are read 64 at a time with coalesced loads, the first four chunks requested together (1 to 3 % at Melbourne's shape: the cells'
// latency is not what binds the kernel).  The loads are plain, not non-temporal: the rows of a day are 139 MB at that shape and are
// read again by every operator of a warm call, so they may stay in the last-level cache; measured, the two kinds of load are equal
// within 0.5 % (profiles/expected_sparse_grad_notes.md).  Lane i forms its cell's rounded products p * mu_f[d] (mu gathered through
// the cache, all 64 gathers in flight together) and leaves them in LDS with the cell's key (segment << 2 | chain).  A cell whose
// predecessor lies in another segment marks its segment's start -- the row is sorted, so a segment's cells are a run of neighbours and
// there is no search.  Lane s then walks segment s's run in order and adds each product onto one of four named accumulators chosen by
// select; a run that continues in the next chunk of 64 continues the same sums.  kGradMaxSeg = 64: a lane can own a segment.
//
// k_exps_trip is the same walk with two values per cell, p * sec(o, d, t) and p * km(o, d), gathered at the stored cells only, the
// diagonal a select per cell, over trip_segments(Z, T) segments; all hours in one launch.  It runs once per table.
//
// Separate kernels in a header of their own: no existing kernel moves.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cpm_expected_grad_batch.h"
#include "cpm_expected_travel.h"

namespace cpm {

constexpr int kExpsGradBlock = 64;  // one wave: lane i loads cell i of the chunk, lane s owns segment s
constexpr int kExpsGradAhead = 4;   // chunks of a row whose cells are loaded before the first is used
constexpr uint32_t kExpsNoKey = 0xffffffffu;
static_assert(kGradMaxSeg <= kExpsGradBlock && kTripMaxSeg <= kExpsGradBlock, "a lane owns a segment");

// The walk over one compact row.  NV values per cell; term(d, pv, prod) forms the cell's NV rounded products.  acc[f][v]: chain v of
// value f of the lane's segment.  Returns with sum[f] = ((w0 + w1) + w2) + w3 of segment `lane`.
template <int NV, class Term>
__device__ __forceinline__ void exps_row_walk(const double *__restrict__ row_p, const uint32_t *__restrict__ row_j, uint32_t n, uint32_t Z, uint32_t seg_len,
                                              Term term, double (&sum)[NV])
{
    __shared__ double s_prod[NV][kExpsGradBlock];
    __shared__ uint32_t s_key[kExpsGradBlock];
    __shared__ int s_start[kExpsGradBlock];
    const uint32_t lane = threadIdx.x;
    double a0[NV], a1[NV], a2[NV], a3[NV];
#pragma unroll
    for (int f = 0; f < NV; ++f) a0[f] = a1[f] = a2[f] = a3[f] = 0.0;
    // the first kExpsGradAhead chunks are requested up front: one round trip to memory for a row of up to 256 cells, not one per chunk
    uint32_t d_ahead[kExpsGradAhead];
    double p_ahead[kExpsGradAhead];
#pragma unroll
    for (int u = 0; u < kExpsGradAhead; ++u) {
        const uint32_t e = static_cast<uint32_t>(u) * kExpsGradBlock + lane;
        d_ahead[u] = 0;
        p_ahead[u] = 0.0;
        if (e < n) {
            d_ahead[u] = row_j[e];
            p_ahead[u] = row_p[e];
        }
    }
    for (uint32_t c = 0; c < n; c += kExpsGradBlock) {  // (uniform over the wave)
        const uint32_t e = c + lane, chunk = c / kExpsGradBlock;
        uint32_t key = kExpsNoKey, d = 0;
        double pv = 0.0;
        if (e < n) {
            if (chunk < kExpsGradAhead) {
#pragma unroll
                for (int u = 0; u < kExpsGradAhead; ++u) {
                    d = chunk == static_cast<uint32_t>(u) ? d_ahead[u] : d;
                    pv = chunk == static_cast<uint32_t>(u) ? p_ahead[u] : pv;
                }
            } else {
                d = row_j[e];
                pv = row_p[e];
            }
            if (d < Z) {  // (the builders skip cells beyond the table as well)
                const uint32_t s = d / seg_len;
                key = (s << 2) | ((d - s * seg_len) & 3u);
            }
        }
        double prod[NV];
#pragma unroll
        for (int f = 0; f < NV; ++f) prod[f] = 0.0;
        if (key != kExpsNoKey) term(d, pv, prod);
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

// grid = Z, one wave per origin.  sp_t / sj_t / scnt_t: the hour's rows.  part: [nseg][Zs]; every word s < nseg, o < Z is written.
__global__ __launch_bounds__(kExpsGradBlock) void k_exps_grad_u(const double *__restrict__ sp_t, const uint32_t *__restrict__ sj_t,
                                                                const uint32_t *__restrict__ scnt_t, uint32_t cap, const double *__restrict__ mu, int Z,
                                                                int Zs, int seg_len, int nseg, double *__restrict__ part)
{
    const size_t o = blockIdx.x;
    const uint32_t n = min(scnt_t[o], cap);
    double sum[1];
    exps_row_walk<1>(sp_t + o * cap, sj_t + o * cap, n, static_cast<uint32_t>(Z), static_cast<uint32_t>(seg_len),
                     [mu](uint32_t d, double pv, double (&prod)[1]) { prod[0] = pv * mu[d]; }, sum);
    const int s = static_cast<int>(threadIdx.x);
    if (s < nseg) part[static_cast<size_t>(s) * Zs + o] = sum[0];
}

// ... for the nf <= NB fleets of a pass.  mu: the pass's [Zs][NB]; part: [nseg][kExpMaxNB][Zs], fleets >= nf are not stored.  Per fleet
// the chains are those of k_exps_grad_u operation for operation.
template <int NB>
__global__ __launch_bounds__(kExpsGradBlock) void k_exps_grad_u_b(const double *__restrict__ sp_t, const uint32_t *__restrict__ sj_t,
                                                                  const uint32_t *__restrict__ scnt_t, uint32_t cap, const double *__restrict__ mu, int Z,
                                                                  int Zs, int seg_len, int nseg, int nf, double *__restrict__ part)
{
    const size_t o = blockIdx.x;
    const uint32_t n = min(scnt_t[o], cap);
    double sum[NB];
    exps_row_walk<NB>(sp_t + o * cap, sj_t + o * cap, n, static_cast<uint32_t>(Z), static_cast<uint32_t>(seg_len),
                      [mu](uint32_t d, double pv, double (&prod)[NB]) {
                          const double *__restrict__ mrow = mu + static_cast<size_t>(d) * NB;
#pragma unroll
                          for (int f = 0; f < NB; ++f) prod[f] = pv * mrow[f];
                      },
                      sum);
    const int s = static_cast<int>(threadIdx.x);
    if (s < nseg) {
#pragma unroll
        for (int f = 0; f < NB; ++f)
            if (f < nf) part[(static_cast<size_t>(s) * kExpMaxNB + f) * Zs + o] = sum[f];
    }
}

// grid = (Z, T), one wave per row.  sp / sj / scnt: all rows [T][Z].  part: [nseg][2][T][Z], seconds then kilometres; every word
// written.  mean: [T][Z dest][Z origin], dist: [Z dest][Z origin], read at the stored cells only.
__global__ __launch_bounds__(kExpsGradBlock) void k_exps_trip(const double *__restrict__ sp, const uint32_t *__restrict__ sj, const uint32_t *__restrict__ scnt,
                                                              uint32_t cap, const double *__restrict__ mean, const double *__restrict__ dist, int Z, int T,
                                                              int seg_len, int nseg, double *__restrict__ part)
{
    const uint32_t o = blockIdx.x;
    const size_t t = blockIdx.y, row = t * Z + o;
    const uint32_t n = min(scnt[row], cap);
    const double *__restrict__ m_t = mean + t * Z * Z;
    double sum[2];
    exps_row_walk<2>(sp + row * cap, sj + row * cap, n, static_cast<uint32_t>(Z), static_cast<uint32_t>(seg_len),
                     [m_t, dist, o, Z](uint32_t d, double pv, double (&prod)[2]) {
                         const size_t cell = static_cast<size_t>(d) * Z + o;
                         const double m = m_t[cell], k = dist[cell];
                         prod[0] = pv * (d == o ? kTripIntraSec : m);
                         prod[1] = pv * (d == o ? kTripIntraKm : k);
                     },
                     sum);
    const int s = static_cast<int>(threadIdx.x);
    if (s < nseg) {
        part[((static_cast<size_t>(s) * 2 + 0) * T + t) * Z + o] = sum[0];
        part[((static_cast<size_t>(s) * 2 + 1) * T + t) * Z + o] = sum[1];
    }
}

}  // namespace cpm
