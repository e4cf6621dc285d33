// cpm_expected.h -- expected parking and driving densities by Markov propagation (include/cpm_expected.h): k_exp_aux, k_exp_lists,
// k_exp_init, k_exp_hour<NB>.
//
// One launch of k_exp_hour per hour (and per pass of at most NB fleets): pi_next = pi * M_t for the fleets of the pass while the
// hour's Z x Z block of p ([Z dest][Z origin], row d contiguous over origins) is read ONCE.  A workgroup of 256 threads takes
// kExpRows consecutive destination rows over all origins; a lane walks the rows' 16-byte grid (two origins per load, kExpRows *
// kExpUnroll loads in flight, non-temporal: a row is read once per hour and must not displace the x vectors from the L2) and keeps
// one accumulator per (row, fleet).  The x vectors come from the L2 through 16-byte loads of an aligned workspace, not from LDS: a
// lane uses every x word it loads for all kExpRows rows at once, so staging x in LDS would read the same words from the L2 once
// per workgroup as well and add an LDS round trip, and it would cap Z * NB at the LDS size (eight fleets at Z = 4,096 are 256 KB).
//
// Rows start off a 16-byte boundary when Z is odd (every other row).  As row_store_shifted does for stores, the loads stay on the
// 16-byte grid: a row that starts 8 bytes behind a grid line gives its first word, a row that ends 8 bytes behind one its last word,
// to a single 8-byte load of thread 0; the pairs in between are (1 + 2k, 2 + 2k) instead of (2k, 2k + 1).
//
// Order of every sum (no floating-point atomics): a lane adds its pairs in ascending k, low word first, thread 0 then the row's odd
// end; the 64 lanes of a wave go through the fixed shuffle tree (obj_wave_sum); the four waves are added in order.  The residual
// list of a destination (origins whose last positive entry it is, ascending) is reduced the same way by the same workgroup.  The
// order is a function of Z, the row's alignment and the table; nothing depends on the number of fleets or a fleet's place.
//
// Separate kernels in a header of their own: the hourly sampler's code does not move.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cpm_objectives.h"

namespace cpm {

constexpr int kExpBlock = 256;
constexpr int kExpWaves = kExpBlock / 64;
constexpr int kExpRows = 4;    // destination rows of a workgroup
constexpr int kExpUnroll = 2;  // 16-byte loads of a row in flight per lane
constexpr int kExpMaxNB = 8;   // fleets of a pass (accumulators per row and lane)

typedef double exp_f64x2 __attribute__((ext_vector_type(2)));

// p_drive as the sampler's Bernoulli maps it (bernoulli_threshold): NaN, negative (and -0.0) -> 0, >= 1 -> 1
__device__ __forceinline__ double exp_q(double v)
{
    if (!(v > 0.0)) return 0.0;
    return v >= 1.0 ? 1.0 : v;
}

// ell[t][o]: the last destination with p > 0 (Z for a zero row: in no list), r[t][o] = max(0, 1 - last).  A lane walks down from
// Z - 1 for its origin: a wave's loads of one destination are 64 consecutive words.  bad: the smallest t * Z + o whose non-zero
// row total exceeds 1 by more than Z * 2^-52 (an integer atomicMin: order-free).  grid = (ceil(Z/256), T).
__global__ __launch_bounds__(kExpBlock) void k_exp_aux(const double *__restrict__ p, const double *__restrict__ last, int Z, int *__restrict__ ell,
                                                       double *__restrict__ r, unsigned long long *__restrict__ bad)
{
    const int o = static_cast<int>(blockIdx.x) * kExpBlock + static_cast<int>(threadIdx.x), t = static_cast<int>(blockIdx.y);
    if (o >= Z) return;
    const size_t row = static_cast<size_t>(t) * Z + o;
    const double tot = last[row];
    const double res = 1.0 - tot;
    r[row] = res > 0.0 ? res : 0.0;
    int d = Z;
    if (tot != 0.0) {
        const double *__restrict__ col = p + static_cast<size_t>(t) * Z * Z + o;
        d = Z - 1;
        while (d >= 0 && !(col[static_cast<size_t>(d) * Z] > 0.0)) --d;
        if (d < 0) d = Z;
        if (tot > 1.0 + static_cast<double>(Z) * 0x1.0p-52) atomicMin(bad, static_cast<unsigned long long>(row));
    }
    ell[row] = d;
}

// The origins of an hour sorted by (ell, origin): list[t][.], and start[t][d] = where destination d's origins begin (start[t][Z]:
// where the zero rows begin).  Origin i's place is the number of origins in front of it, counted over the hour's ell in LDS (every
// lane reads the same word: a broadcast); the places are a permutation, so every word of list is written.  grid = (ceil(Z/256), T),
// LDS = Z ints.
__global__ __launch_bounds__(kExpBlock) void k_exp_lists(const int *__restrict__ ell, int Z, int *__restrict__ start, int *__restrict__ list)
{
    extern __shared__ int s_ell[];
    const int t = static_cast<int>(blockIdx.y), tid = static_cast<int>(threadIdx.x);
    for (int o = tid; o < Z; o += kExpBlock) s_ell[o] = ell[static_cast<size_t>(t) * Z + o];
    __syncthreads();
    const int i = static_cast<int>(blockIdx.x) * kExpBlock + tid;
    if (i >= Z) return;
    const int mine = s_ell[i];
    int before = 0, below_i = 0, below_z = 0;
    for (int o = 0; o < Z; ++o) {
        const int e = s_ell[o];
        before += (e < mine || (e == mine && o < i)) ? 1 : 0;
        below_i += e < i ? 1 : 0;
        below_z += e < Z ? 1 : 0;
    }
    list[static_cast<size_t>(t) * Z + before] = i;
    start[static_cast<size_t>(t) * (Z + 1) + i] = below_i;
    if (i == 0) start[static_cast<size_t>(t) * (Z + 1) + Z] = below_z;
}

// pi_0 and x_0 = pi_0 * q of every fleet into the workspace (and, when the day starts here, into hour 0 of the outputs).
// grid = (ceil(Z/256), B).  pi0: nullptr = uniform 1 / Z.
__global__ __launch_bounds__(kExpBlock) void k_exp_init(const double *__restrict__ pi0, const double *__restrict__ q0, size_t q_stride, int Z, int Zs,
                                                        double *__restrict__ ws_pi, double *__restrict__ ws_x, double *__restrict__ park,
                                                        double *__restrict__ drv, size_t out_stride)
{
    const int z = static_cast<int>(blockIdx.x) * kExpBlock + static_cast<int>(threadIdx.x), b = static_cast<int>(blockIdx.y);
    if (z >= Z) return;
    const double pi = pi0 ? pi0[z] : 1.0 / static_cast<double>(Z);
    const double x = pi * exp_q(q0[static_cast<size_t>(b) * q_stride + z]);
    ws_pi[static_cast<size_t>(b) * Zs + z] = pi;
    ws_x[static_cast<size_t>(b) * Zs + z] = x;
    if (park) {
        park[static_cast<size_t>(b) * out_stride + z] = pi;
        drv[static_cast<size_t>(b) * out_stride + z] = x;
    }
}

// sum of v[i] over the workgroup for every i, into out[i]: the wave tree, then the waves in order.  Every thread calls it.
template <int NV>
__device__ __forceinline__ void exp_block_sum(const double (&v)[NV], double *s_part, double *out)
{
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const double w = obj_wave_sum(v[i]);
        if (lane == 0) s_part[wave * NV + i] = w;
    }
    __syncthreads();
    if (tid < NV) out[tid] = ((s_part[tid] + s_part[NV + tid]) + s_part[2 * NV + tid]) + s_part[3 * NV + tid];
    __syncthreads();
}
static_assert(kExpWaves == 4, "exp_block_sum adds four waves");

// The streamed part of k_exp_hour: acc[r * NB + f] += x_f[o] * row_r[o] over this lane's origins.  ODD: Z is odd, so the rows alternate
// between starting on a 16-byte line and 8 bytes behind one; H0: row 0 of the workgroup is of the second kind.  Both are compile-time
// here (the kernel branches once, uniformly): no select stands between a load and its multiply.
template <int NB, bool ODD, bool H0>
__device__ __forceinline__ void exp_stream(const double *(&row)[kExpRows], const double *(&xf)[NB], int Z, double (&acc)[kExpRows * NB])
{
    const int tid = static_cast<int>(threadIdx.x);
    const int npairs = Z >> 1;
    for (int k0 = tid; k0 < npairs; k0 += kExpBlock * kExpUnroll) {
        exp_f64x2 pv[kExpUnroll][kExpRows];
        exp_f64x2 x01[kExpUnroll][NB];
        double x2[kExpUnroll][NB];
#pragma unroll
        for (int u = 0; u < kExpUnroll; ++u) {
            const int k = k0 + u * kExpBlock;
            const bool in = k < npairs;
#pragma unroll
            for (int r = 0; r < kExpRows; ++r) {
                const int head = (ODD && (H0 != ((r & 1) != 0))) ? 1 : 0;  // 1: the row's pairs are (1 + 2k, 2 + 2k)
                exp_f64x2 v = {0.0, 0.0};
                if (in) v = __builtin_nontemporal_load(reinterpret_cast<const exp_f64x2 *>(row[r] + head + 2 * k));
                pv[u][r] = v;
            }
#pragma unroll
            for (int f = 0; f < NB; ++f) {
                exp_f64x2 v = {0.0, 0.0};
                double w = 0.0;
                if (in) {
                    v = *reinterpret_cast<const exp_f64x2 *>(xf[f] + 2 * k);
                    if (ODD) w = xf[f][2 * k + 2];  // (2k + 2 <= Z - 1 for k < (Z - 1) / 2)
                }
                x01[u][f] = v;
                x2[u][f] = w;
            }
        }
        // (a pair past the end is 0 * 0: adding +0 to a sum of non-negative terms changes no bit)
#pragma unroll
        for (int u = 0; u < kExpUnroll; ++u)
#pragma unroll
            for (int r = 0; r < kExpRows; ++r)
#pragma unroll
                for (int f = 0; f < NB; ++f) {
                    const bool head = ODD && (H0 != ((r & 1) != 0));
                    const double xa = head ? x01[u][f].y : x01[u][f].x;
                    const double xb = head ? x2[u][f] : x01[u][f].y;
                    double a = acc[r * NB + f];
                    a = a + xa * pv[u][r].x;
                    a = a + xb * pv[u][r].y;
                    acc[r * NB + f] = a;
                }
    }
    if (ODD && tid == 0) {  // the word of the row that shares its 16 bytes with a neighbour
#pragma unroll
        for (int r = 0; r < kExpRows; ++r) {
            const bool head = H0 != ((r & 1) != 0);
            const int oe = head ? 0 : Z - 1;
            const double pe = row[r][oe];
#pragma unroll
            for (int f = 0; f < NB; ++f) acc[r * NB + f] = acc[r * NB + f] + xf[f][oe] * pe;
        }
    }
}

// One hour for the nf <= NB fleets of a pass.  grid = ceil(Z / kExpRows).  Pointers that carry a fleet stride point at the pass's
// first fleet.  p_t / last_t / r_t / start_t / list_t: the hour's slices.  q_next: nullptr when nothing follows (no x is written).
// park / drv: where pi_next and x_next also go (nullptr: the workspace only).
template <int NB>
__global__ __launch_bounds__(kExpBlock) void k_exp_hour(const double *__restrict__ p_t, const double *__restrict__ last_t, const double *__restrict__ r_t,
                                                        const int *__restrict__ start_t, const int *__restrict__ list_t,
                                                        const double *__restrict__ q_cur, const double *__restrict__ q_next, size_t q_stride,
                                                        const double *__restrict__ pi_in, const double *__restrict__ x_in,
                                                        double *__restrict__ pi_out, double *__restrict__ x_out, double *__restrict__ park,
                                                        double *__restrict__ drv, size_t out_stride, int Z, int Zs, int nf)
{
    __shared__ double s_part[kExpWaves * kExpRows * NB];
    __shared__ double s_y[kExpRows * NB];
    __shared__ double s_res[kExpRows * NB];
    const int tid = static_cast<int>(threadIdx.x);
    const int d0 = static_cast<int>(blockIdx.x) * kExpRows;
    const bool odd = (Z & 1) != 0;

    const double *row[kExpRows];
#pragma unroll
    for (int r = 0; r < kExpRows; ++r) {
        // (a row past the end repeats one of the last two, the one that starts where it would: computed, not stored)
        int d = d0 + r;
        if (d >= Z) d -= 2 * ((d - Z) / 2 + 1);
        row[r] = p_t + static_cast<size_t>(d > 0 ? d : 0) * Z;
    }
    const bool h0 = odd && ((reinterpret_cast<uintptr_t>(row[0]) >> 3) & 1u) != 0;  // (Z odd: row r starts as row 0 does iff r is even)
    const double *xf[NB];
#pragma unroll
    for (int f = 0; f < NB; ++f) xf[f] = x_in + static_cast<size_t>(f < nf ? f : nf - 1) * Zs;

    double acc[kExpRows * NB];
#pragma unroll
    for (int i = 0; i < kExpRows * NB; ++i) acc[i] = 0.0;
    if (!odd) exp_stream<NB, false, false>(row, xf, Z, acc);
    else if (h0) exp_stream<NB, true, true>(row, xf, Z, acc);
    else exp_stream<NB, true, false>(row, xf, Z, acc);
    exp_block_sum<kExpRows * NB>(acc, s_part, s_y);

    // the residuals that arrive at these destinations (D1): x[o] * r[o] over the destination's origins, ascending
    for (int r = 0; r < kExpRows; ++r) {
        const int d = d0 + r;
        int ka = 0, kb = 0;
        if (d < Z) {
            ka = start_t[d];
            kb = start_t[d + 1];
        }
        if (kb > ka) {  // (uniform over the workgroup)
            double a2[NB];
#pragma unroll
            for (int f = 0; f < NB; ++f) a2[f] = 0.0;
            for (int k = ka + tid; k < kb; k += kExpBlock) {
                const int o = list_t[k];
                const double rr = r_t[o];
#pragma unroll
                for (int f = 0; f < NB; ++f) a2[f] = a2[f] + xf[f][o] * rr;
            }
            exp_block_sum<NB>(a2, s_part, s_res + r * NB);
        } else if (tid < NB) {
            s_res[r * NB + tid] = 0.0;
        }
    }
    __syncthreads();

    if (tid < kExpRows * NB) {
        const int r = tid / NB, f = tid % NB, d = d0 + r;
        if (d < Z && f < nf) {
            const size_t i = static_cast<size_t>(f) * Zs + d;
            const double pi = pi_in[i];
            const double stay = pi * (1.0 - exp_q(q_cur[static_cast<size_t>(f) * q_stride + d]));
            double v = stay + s_y[tid];
            v = v + s_res[tid];
            if (last_t[d] == 0.0) v = v + x_in[i];  // a zero row: the driver stays where it is (src/resampling.jl:35-36)
            pi_out[i] = v;
            if (park) park[static_cast<size_t>(f) * out_stride + d] = v;
            if (q_next) {
                const double xn = v * exp_q(q_next[static_cast<size_t>(f) * q_stride + d]);
                x_out[i] = xn;
                if (drv) drv[static_cast<size_t>(f) * out_stride + d] = xn;
            }
        }
    }
}

}  // namespace cpm
