// cpm_expected_fit.h -- value and four-parameter gradient of the noise-free objectives (include/cpm_expected_fit.h): k_fit_params,
// k_fit_dens, k_fit_zones, k_fit_final, k_fit_cot, k_fit_mean_range, k_fit_chain, k_fit_chain_total.
//
// The new work is O(B * T * Z) beside the O(T * Z * Z) operators of the propagation it sits between, so every kernel here is a plain
// streaming pass with a zone on the lane (an hour's loads of a wave are 64 consecutive words):
//   k_fit_dens    the densities of the day from the kept pi_s: parking = pi, driving = pi * q (ONE multiplication: k_exp_hour's bits);
//   k_fit_zones   ONE walk over a fleet's densities for the hour sums of driving and the zones' extremes of parking, a second walk over
//                 the parking rows of the valid zones (in L2 by then) for e_z and the two sums of the argmin / argmax terms;
//   k_fit_final   one wave per fleet: the hour sums' partials in order, the activity, its error and cotangent, the scalars, the record;
//   k_fit_cot     ONE walk: the cotangent [2][T][Z] of a fleet from the zones' records, the hours' activity terms and w_sec;
//   k_fit_chain   ONE walk over grad_p_drive (and grad_dest, driving, dw_sec): the chunks' sums of the chain rule's terms;
//   k_fit_chain_total  one wave per fleet: the chunks in order, words 5 .. 8 of the record.
//
// Order of every sum over zones (no floating-point atomics): a workgroup of 256 consecutive zones goes through the fixed tree of a
// wave (obj_wave_sum) and its four waves in order; one wave then adds a fleet's partials -- lane l takes partials l, l + 64, ... in
// ascending order, then the same tree.  The chain rule's chunks are those of k_exp_travel: 1,024 consecutive words of [T][Z], thread i
// adds words i, i + 256, i + 512, i + 768 in that order, exp_block_sum's tree, the chunks as above.  Everything else is a fixed
// sequence of IEEE f64 operations per word (the library is built with -ffp-contract=off).
//
// A word that is read once and not again by these kernels comes through a non-temporal load (driving in k_fit_zones, parking in
// k_fit_cot, the gradients in k_fit_chain); what the next kernel reads again (the densities, the cotangent) is stored plainly.
//
// Separate kernels in a header of their own: no existing kernel's code moves.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/cpm_batch.h"
#include "cpm_expected_travel.h"
#include "cpm_tables.h"

namespace cpm {

constexpr int kFitWords = 16;  // CPM_FIT_WORDS
constexpr int kFitChainTerms = 5;

// what a call copies from the host: by value through the kernel's arguments (3 KB), so that nothing of the caller's is read later.
// [B][3] weights, then [B][3] p_min, p_max, e_drive.
struct FitParams {
    double w[6 * CPM_MAX_BATCH];
};

// grid = 1.  out: the n words of p
__global__ __launch_bounds__(64) void k_fit_params(FitParams p, int n, double *__restrict__ out)
{
    for (int i = static_cast<int>(threadIdx.x); i < n; i += 64) out[i] = p.w[i];
}

// grid = (ceil(Z/256), T, B).  pi_day: pi_s of the day's first operator, fleet b's vector of operator s at (s * B + b) * Zs.
// q: the fleets' p_drive tables, q_stride apart.  out: [B][2][T][Z].
__global__ __launch_bounds__(kExpBlock) void k_fit_dens(const double *__restrict__ pi_day, const double *__restrict__ q, size_t q_stride, int Z, int Zs, int T,
                                                        int B, double *__restrict__ out)
{
    const int z = static_cast<int>(blockIdx.x) * kExpBlock + static_cast<int>(threadIdx.x), j = static_cast<int>(blockIdx.y), b = static_cast<int>(blockIdx.z);
    if (z >= Z) return;
    const double pi = pi_day[(static_cast<size_t>(j) * B + b) * Zs + z];
    const size_t zt = static_cast<size_t>(Z) * T, i = static_cast<size_t>(j) * Z + z;
    out[static_cast<size_t>(b) * 2 * zt + i] = pi;
    out[static_cast<size_t>(b) * 2 * zt + zt + i] = pi * exp_q(q[static_cast<size_t>(b) * q_stride + i]);
}

// grid = (ceil(Z/256), B), LDS = 4 * T doubles.  expected: [B][2][T][Z].  measured [T][Z] / flag [Z]: nullptr without measured parking.
// hpart: [B][T][gridDim.x] the workgroups' hour sums of driving.  zone: [5][B][Z] lo, range, S1, S2, e_z of the valid zones (others:
// not written, arg < 0).  arg: [B][Z] imin | imax << 16, or -1 for a zone that is not valid.  epart / npart: [B][gridDim.x].
// Every thread stays until the end (the wave reductions take all lanes).
__global__ __launch_bounds__(kExpBlock) void k_fit_zones(const double *__restrict__ expected, const double *__restrict__ measured,
                                                         const int *__restrict__ flag, int Z, int T, int B, double *__restrict__ hpart,
                                                         double *__restrict__ zone, int *__restrict__ arg, double *__restrict__ epart,
                                                         int *__restrict__ npart)
{
    extern __shared__ double s_hour[];  // [kExpWaves][T]
    __shared__ double s_e[kExpWaves];
    __shared__ int s_n[kExpWaves];
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int b = static_cast<int>(blockIdx.y);
    const int z = static_cast<int>(blockIdx.x) * kExpBlock + tid;
    const bool in = z < Z;
    const size_t zt = static_cast<size_t>(Z) * T;
    const double *__restrict__ park = expected + static_cast<size_t>(b) * 2 * zt;
    const double *__restrict__ drv = park + zt;

    double lo = 0.0, hi = 0.0;
    int imin = 0, imax = 0;
    for (int t = 0; t < T; ++t) {
        const size_t i = static_cast<size_t>(t) * Z + z;
        const double p = in ? park[i] : 0.0;
        const double d = in ? __builtin_nontemporal_load(drv + i) : 0.0;
        if (t == 0) {
            lo = hi = p;
        } else {
            if (p < lo) lo = p, imin = t;  // (strict: the first hour where several tie)
            if (p > hi) hi = p, imax = t;
        }
        const double w = obj_wave_sum(d);
        if (lane == 0) s_hour[wave * T + t] = w;
    }

    const bool valid = in && measured != nullptr && flag[z] != 0 && lo != hi;
    double e = 0.0;
    if (valid) {
        const double range = hi - lo, n = static_cast<double>(T);
        double acc = 0.0, s1 = 0.0, s2 = 0.0;
        for (int t = 0; t < T; ++t) {
            const size_t i = static_cast<size_t>(t) * Z + z;
            const double vn = (park[i] - lo) / range;
            const double d = vn - measured[i];
            acc = acc + d * d;
            const double ee = (2.0 * d) / n;
            s1 = s1 + ee * (1.0 - vn);
            s2 = s2 + ee * vn;
        }
        e = acc / n;
        const size_t k = static_cast<size_t>(b) * Z + z, bz = static_cast<size_t>(B) * Z;
        zone[k] = lo;
        zone[bz + k] = range;
        zone[2 * bz + k] = s1;
        zone[3 * bz + k] = s2;
        zone[4 * bz + k] = e;
    }
    if (in) arg[static_cast<size_t>(b) * Z + z] = valid ? (imin | (imax << 16)) : -1;

    const double we = obj_wave_sum(e);
    int wn = valid ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) wn += __shfl_down(wn, o, 64);
    if (lane == 0) {
        s_e[wave] = we;
        s_n[wave] = wn;
    }
    __syncthreads();
    const size_t k = static_cast<size_t>(b) * gridDim.x + blockIdx.x;
    for (int t = tid; t < T; t += kExpBlock)
        hpart[(static_cast<size_t>(b) * T + t) * gridDim.x + blockIdx.x] = ((s_hour[t] + s_hour[T + t]) + s_hour[2 * T + t]) + s_hour[3 * T + t];
    if (tid == 0) {
        epart[k] = ((s_e[0] + s_e[1]) + s_e[2]) + s_e[3];
        npart[k] = s_n[0] + s_n[1] + s_n[2] + s_n[3];
    }
}
static_assert(kExpWaves == 4, "k_fit_zones adds four waves");

// grid = B, one wave, LDS = T doubles.  totals: [B][2] of k_exp_travel_total.  act_meas: [T] or nullptr.  weights: [B][3].
// record: [B][rec_stride], words 0 .. 4, 9 .. 15 and the activity.  ga: [B][T] the hours' activity cotangent, scaled by w_act.
// nval: [B] the fleet's n_valid for k_fit_cot.
__global__ __launch_bounds__(64) void k_fit_final(const double *__restrict__ hpart, const double *__restrict__ epart, const int *__restrict__ npart, int nb,
                                                  int T, const double *__restrict__ totals, const double *__restrict__ act_meas,
                                                  const double *__restrict__ weights, double *__restrict__ record, size_t rec_stride,
                                                  double *__restrict__ ga, double *__restrict__ nval)
{
    extern __shared__ double s_a[];  // [T]
    const int lane = static_cast<int>(threadIdx.x), b = static_cast<int>(blockIdx.x);
    for (int t = 0; t < T; ++t) {
        double s = 0.0;
        for (int i = lane; i < nb; i += 64) s = s + hpart[(static_cast<size_t>(b) * T + t) * nb + i];
        s = obj_wave_sum(s);
        if (lane == 0) s_a[t] = s;
    }
    double se = 0.0;
    int n = 0;
    for (int i = lane; i < nb; i += 64) {
        se = se + epart[static_cast<size_t>(b) * nb + i];
        n += npart[static_cast<size_t>(b) * nb + i];
    }
    se = obj_wave_sum(se);
    for (int o = 32; o > 0; o >>= 1) n += __shfl_down(n, o, 64);
    if (lane != 0) return;

    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double w_act = weights[3 * b], w_park = weights[3 * b + 1], w_adr = weights[3 * b + 2];
    double *rec = record + static_cast<size_t>(b) * rec_stride;
    double *g = ga + static_cast<size_t>(b) * T;
    const double nt = static_cast<double>(T);

    double lo = s_a[0], hi = s_a[0];
    int imin = 0, imax = 0;
    for (int t = 1; t < T; ++t) {
        const double a = s_a[t];
        if (a < lo) lo = a, imin = t;
        if (a > hi) hi = a, imax = t;
    }
    const double range = hi - lo;
    double act_err = nan;
    if (range != 0.0) {
        double acc = 0.0, s1 = 0.0, s2 = 0.0;
        for (int t = 0; t < T; ++t) {
            const double vn = (s_a[t] - lo) / range;
            rec[kFitWords + t] = vn;
            if (act_meas) {
                const double d = vn - act_meas[t];
                acc = acc + d * d;
                const double ee = (2.0 * d) / nt;
                s1 = s1 + ee * (1.0 - vn);
                s2 = s2 + ee * vn;
                g[t] = ee / range;
            } else {
                g[t] = 0.0;
            }
        }
        if (act_meas) {
            act_err = acc / nt;
            g[imin] = g[imin] - s1 / range;
            g[imax] = g[imax] - s2 / range;
            for (int t = 0; t < T; ++t) g[t] = w_act * g[t];
        }
    } else {
        for (int t = 0; t < T; ++t) {
            rec[kFitWords + t] = nan;  // (0 / 0 of the host's traffic_activity)
            g[t] = 0.0;
        }
    }
    const double park_err = n == 0 ? nan : se / static_cast<double>(n);
    const double sec = totals[2 * b], km = totals[2 * b + 1];
    const double a_drive = sec / (nt * 3600.0);
    double f = 0.0;
    if (w_act != 0.0) f = f + w_act * act_err;
    if (w_park != 0.0) f = f + w_park * park_err;
    if (w_adr != 0.0) f = f + w_adr * a_drive;
    rec[0] = f;
    rec[1] = act_err;
    rec[2] = park_err;
    rec[3] = a_drive;
    rec[4] = static_cast<double>(n);
    rec[9] = sec;
    rec[10] = km;
    for (int i = 11; i < kFitWords; ++i) rec[i] = 0.0;
    nval[b] = static_cast<double>(n);
}

// grid = (ceil(Z/256), B).  cot: [B][2][T][Z], every word written.  w_sec: [T][Z] (read where w_adrive != 0 only).
__global__ __launch_bounds__(kExpBlock) void k_fit_cot(const double *__restrict__ expected, const double *__restrict__ measured, const double *__restrict__ zone,
                                                       const int *__restrict__ arg, const double *__restrict__ ga, const double *__restrict__ nval,
                                                       const double *__restrict__ w_sec, const double *__restrict__ weights, int Z, int T, int B,
                                                       double *__restrict__ cot)
{
    const int z = static_cast<int>(blockIdx.x) * kExpBlock + static_cast<int>(threadIdx.x), b = static_cast<int>(blockIdx.y);
    if (z >= Z) return;
    const size_t zt = static_cast<size_t>(Z) * T, k = static_cast<size_t>(b) * Z + z, bz = static_cast<size_t>(B) * Z;
    const double *__restrict__ park = expected + static_cast<size_t>(b) * 2 * zt;
    const double *__restrict__ g_act = ga + static_cast<size_t>(b) * T;
    double *__restrict__ cp = cot + static_cast<size_t>(b) * 2 * zt;
    double *__restrict__ cd = cp + zt;
    const double w_act = weights[3 * b], w_park = weights[3 * b + 1], w_adr = weights[3 * b + 2];
    const int a = arg[k];
    const bool zone_on = w_park != 0.0 && a >= 0;  // (a valid zone exists: n_valid >= 1)
    const int imin = a & 0xffff, imax = (a >> 16) & 0xffff;
    double lo = 0.0, range = 1.0, s1 = 0.0, s2 = 0.0, nv = 1.0;
    if (zone_on) {
        lo = zone[k];
        range = zone[bz + k];
        s1 = zone[2 * bz + k];
        s2 = zone[3 * bz + k];
        nv = nval[b];
    }
    const double nt = static_cast<double>(T), day = nt * 3600.0;
    for (int t = 0; t < T; ++t) {
        const size_t i = static_cast<size_t>(t) * Z + z;
        double gp = 0.0;
        if (zone_on) {
            const double vn = (__builtin_nontemporal_load(park + i) - lo) / range;
            const double d = vn - measured[i];
            const double ee = (2.0 * d) / nt;
            double g = ee / range;
            if (t == imin) g = g - s1 / range;
            if (t == imax) g = g - s2 / range;
            g = g / nv;
            gp = w_park * g;
        }
        double gd = 0.0;
        if (w_act != 0.0) gd = g_act[t];
        if (w_adr != 0.0) gd = gd + w_adr * (w_sec[i] / day);
        cp[i] = gp;
        cd[i] = gd;
    }
}

// grid = ceil(Z/256).  range: [2][Z] mn | mx of the zone's mean_sum over the day, as k_pdrive_final forms them.
__global__ __launch_bounds__(kExpBlock) void k_fit_mean_range(const double *__restrict__ mean_sum, int Z, int T, double *__restrict__ range)
{
    const int z = static_cast<int>(blockIdx.x) * kExpBlock + static_cast<int>(threadIdx.x);
    if (z >= Z) return;
    double mx = mean_sum[z], mn = mean_sum[z];
    for (int h = 1; h < T; ++h) {
        const double v = mean_sum[z + static_cast<size_t>(h) * Z];
        mx = jl_max(mx, v);
        mn = jl_min(mn, v);
    }
    range[z] = mn;
    range[Z + z] = mx;
}

// grid = (chunks of kTravelChunk words of [T][Z], B).  grad_pd / grad_dest: [B][T][Z]; grad_dest nullptr without the tangent.
// dw_sec: [T][Z] or nullptr (no direct term).  par: [B][3] p_min, p_max, e_drive.  part: [B][gridDim.x][5].
__global__ __launch_bounds__(kExpBlock) void k_fit_chain(const double *__restrict__ grad_pd, const double *__restrict__ grad_dest,
                                                         const double *__restrict__ expected, const double *__restrict__ dw_sec,
                                                         const double *__restrict__ mean_sum, const double *__restrict__ range,
                                                         const double *__restrict__ par, const double *__restrict__ weights, int Z, size_t zt,
                                                         double *__restrict__ part)
{
    __shared__ double s_part[kExpWaves * kFitChainTerms];
    __shared__ double s_tot[kFitChainTerms];
    const int tid = static_cast<int>(threadIdx.x);
    const size_t b = blockIdx.y, i0 = static_cast<size_t>(blockIdx.x) * kTravelChunk + tid;
    const double p_min = par[3 * b], p_max = par[3 * b + 1], e_drive = par[3 * b + 2];
    const double span = p_max - p_min;
    const bool direct = dw_sec != nullptr && weights[3 * b + 2] != 0.0;
    const double *__restrict__ g_pd = grad_pd + b * zt;
    const double *__restrict__ g_de = grad_dest ? grad_dest + b * zt : nullptr;
    const double *__restrict__ drv = expected + b * 2 * zt + zt;
    double acc[kFitChainTerms] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < kTravelPerThread; ++j) {
        const size_t i = i0 + static_cast<size_t>(j) * kExpBlock;
        if (i < zt) {
            const double g = __builtin_nontemporal_load(g_pd + i);
            if (g != 0.0) {
                const int z = static_cast<int>(i % static_cast<size_t>(Z));
                const double mn = range[z], mx = range[Z + z];
                if (mx > 0) {
                    const double s = (mean_sum[i] - mn) / (mx - mn);
                    const double se = pow_f64(s, e_drive);
                    acc[0] = acc[0] + g * (1.0 - se);
                    acc[1] = acc[1] + g * se;
                    if (s > 0.0) acc[2] = acc[2] + (g * span) * (se * log(s));
                }
            }
            if (g_de) acc[3] = acc[3] + __builtin_nontemporal_load(g_de + i);
            if (direct) acc[4] = acc[4] + drv[i] * dw_sec[i];
        }
    }
    exp_block_sum<kFitChainTerms>(acc, s_part, s_tot);
    if (tid < kFitChainTerms) part[(b * gridDim.x + blockIdx.x) * kFitChainTerms + tid] = s_tot[tid];
}

// grid = B, one wave.  Words 5 .. 8 of every record.  dest: the call ran along the tangent.  T: the hours of the day.
__global__ __launch_bounds__(64) void k_fit_chain_total(const double *__restrict__ part, int nchunk, const double *__restrict__ weights, int dest, int T,
                                                        double *__restrict__ record, size_t rec_stride)
{
    const int lane = static_cast<int>(threadIdx.x);
    const size_t b = blockIdx.x;
    double a[kFitChainTerms] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int g = lane; g < nchunk; g += 64)
#pragma unroll
        for (int i = 0; i < kFitChainTerms; ++i) a[i] = a[i] + part[(b * nchunk + g) * kFitChainTerms + i];
#pragma unroll
    for (int i = 0; i < kFitChainTerms; ++i) a[i] = obj_wave_sum(a[i]);
    if (lane != 0) return;
    double *rec = record + b * rec_stride;
    rec[5] = a[0];
    rec[6] = a[1];
    rec[7] = a[2];
    double d = __longlong_as_double(0x7ff8000000000000ll);
    if (dest) {
        d = a[3];
        const double w_adr = weights[3 * b + 2];
        if (w_adr != 0.0) d = d + w_adr * (a[4] / (static_cast<double>(T) * 3600.0));
    }
    rec[8] = d;
}

}  // namespace cpm
