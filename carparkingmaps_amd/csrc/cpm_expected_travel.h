// cpm_expected_travel.h -- expected travel time and distance per zone and hour (include/cpm_expected_travel.h): k_exp_trip,
// k_exp_trip_finish, k_exp_travel.
//
// The trip weights w_sec[t][o], w_km[t][o] are column sums of an elementwise product: p[t][d][o] * sec(o, d, t) over d, with the mean
// plane of the datamatrix and the distance matrix laid out like p (origin fastest).  They depend on the tables alone, so ONE launch
// of k_exp_trip covers all hours.  A workgroup of 256 threads takes a strip of kTripStrip = 128 origins of one hour and one segment
// of the destinations; a lane owns two origins and keeps four accumulators (seconds and kilometres of each).  p and the mean plane
// are read once (non-temporal loads); the distance matrix is read again by every hour and stays in the last-level cache (plain loads).
//
// Z even: a lane's two origins are neighbours and come with one 16-byte load per array (every row then starts on a 16-byte line).
// Z odd: every other row starts 8 bytes behind a line; the kernel falls back to two 8-byte loads per array, origins lane and lane + 64
// of the strip (each load of a wave still covers 512 consecutive bytes).  Which origin a lane owns changes no sum.
//
// Order of every sum (no floating-point atomics): the destinations of a segment are dealt over the four waves, wave v takes
// d = begin + v, begin + v + 4, ...; a lane adds its products in ascending d, acc = acc + p * value, starting from 0; the four waves
// are added in order, ((w0 + w1) + w2) + w3; k_exp_trip_finish adds the segments in ascending order and then the residual term
// r * value(o, ell).  The number of segments is a function of Z and T alone (trip_segments).  The diagonal is a select per element:
// sec(o, o, t) = 300, km(o, o) = 1 whatever the arrays hold there.
//
// k_exp_travel: per fleet the products x * w_sec, x * w_km with the driving density x; a workgroup takes a chunk of 1,024 consecutive
// words of [T][Z], thread i adds the chunk's words i, i + 256, i + 512, i + 768 in that order, then exp_block_sum's fixed tree.
// k_exp_travel_total adds a fleet's chunks in fixed order (lane l of one wave: chunks l, l + 64, ... ascending, then the wave's tree).
//
// Separate kernels in a header of their own: k_exp_hour and the hourly sampler's code do not move.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cpm_expected.h"

namespace cpm {

constexpr int kTripStrip = 2 * 64;  // origins of a workgroup: two per lane, every wave sees the whole strip
constexpr int kTripUnroll = 4;      // destinations of a wave in flight (three arrays each)
constexpr int kTripMaxSeg = 8;
constexpr double kTripIntraSec = 300.0, kTripIntraKm = 1.0;  // a trip inside a zone (src/resampling.jl:58-60)

// destination segments of k_exp_trip: enough workgroups for the chip at small Z * T (about 1,024), a function of Z and T alone so that
// the order of the sums does not depend on the device
inline int trip_segments(int Z, int T)
{
    const long long base = static_cast<long long>((Z + kTripStrip - 1) / kTripStrip) * T;
    long long n = (1024 + base - 1) / base;
    const long long most = (Z + 63) / 64;  // (a segment keeps at least 64 destinations)
    if (n > most) n = most;
    if (n > kTripMaxSeg) n = kTripMaxSeg;
    return n < 1 ? 1 : static_cast<int>(n);
}
inline int trip_segment_len(int Z, int nseg) { return (Z + nseg - 1) / nseg; }

// grid = (ceil(Z / kTripStrip), T, nseg).  part: [nseg][2][T][Z] the segments' sums, seconds then kilometres; every word written.
template <bool ODD>
__global__ __launch_bounds__(kExpBlock) void k_exp_trip(const double *__restrict__ p, const double *__restrict__ mean, const double *__restrict__ dist,
                                                        int Z, int T, int seg_len, double *__restrict__ part)
{
    __shared__ double s_acc[kExpWaves][4][64];
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int t = static_cast<int>(blockIdx.y), seg = static_cast<int>(blockIdx.z);
    const int o0 = static_cast<int>(blockIdx.x) * kTripStrip;
    const int oa = ODD ? o0 + lane : o0 + 2 * lane, ob = ODD ? oa + 64 : oa + 1;
    const bool in_a = oa < Z, in_b = ob < Z;  // (Z even: both or neither)
    const int d_begin = seg * seg_len, d_end = d_begin + seg_len < Z ? d_begin + seg_len : Z;
    const size_t plane = static_cast<size_t>(t) * Z * Z;
    const double *__restrict__ p_t = p + plane;
    const double *__restrict__ m_t = mean + plane;

    double sa = 0.0, sb = 0.0, ka = 0.0, kb = 0.0;
    for (int d0 = d_begin + wave; d0 < d_end; d0 += kExpWaves * kTripUnroll) {
        double pa[kTripUnroll], pb[kTripUnroll], ma[kTripUnroll], mb[kTripUnroll], da[kTripUnroll], db[kTripUnroll];
#pragma unroll
        for (int u = 0; u < kTripUnroll; ++u) {
            const int d = d0 + u * kExpWaves;  // (uniform over the wave)
            pa[u] = pb[u] = ma[u] = mb[u] = da[u] = db[u] = 0.0;
            if (d < d_end) {
                const size_t row = static_cast<size_t>(d) * Z;
                if (ODD) {
                    if (in_a) {
                        pa[u] = __builtin_nontemporal_load(p_t + row + oa);
                        ma[u] = __builtin_nontemporal_load(m_t + row + oa);
                        da[u] = dist[row + oa];
                    }
                    if (in_b) {
                        pb[u] = __builtin_nontemporal_load(p_t + row + ob);
                        mb[u] = __builtin_nontemporal_load(m_t + row + ob);
                        db[u] = dist[row + ob];
                    }
                } else if (in_a) {
                    const exp_f64x2 pv = __builtin_nontemporal_load(reinterpret_cast<const exp_f64x2 *>(p_t + row + oa));
                    const exp_f64x2 mv = __builtin_nontemporal_load(reinterpret_cast<const exp_f64x2 *>(m_t + row + oa));
                    const exp_f64x2 dv = *reinterpret_cast<const exp_f64x2 *>(dist + row + oa);
                    pa[u] = pv.x, pb[u] = pv.y, ma[u] = mv.x, mb[u] = mv.y, da[u] = dv.x, db[u] = dv.y;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kTripUnroll; ++u) {
            const int d = d0 + u * kExpWaves;
            if (d < d_end) {
                sa = sa + pa[u] * (d == oa ? kTripIntraSec : ma[u]);
                sb = sb + pb[u] * (d == ob ? kTripIntraSec : mb[u]);
                ka = ka + pa[u] * (d == oa ? kTripIntraKm : da[u]);
                kb = kb + pb[u] * (d == ob ? kTripIntraKm : db[u]);
            }
        }
    }
    s_acc[wave][0][lane] = sa;
    s_acc[wave][1][lane] = sb;
    s_acc[wave][2][lane] = ka;
    s_acc[wave][3][lane] = kb;
    __syncthreads();
    // thread (i, l): accumulator i of lane l over the four waves, in order
    const int i = tid >> 6, l = tid & 63;
    const double sum = ((s_acc[0][i][l] + s_acc[1][i][l]) + s_acc[2][i][l]) + s_acc[3][i][l];
    const int o = ODD ? o0 + l + 64 * (i & 1) : o0 + 2 * l + (i & 1);
    if (o < Z) part[((static_cast<size_t>(seg) * 2 + (i >> 1)) * T + t) * Z + o] = sum;
}
static_assert(kExpWaves == 4 && kExpBlock == 256, "k_exp_trip deals destinations over four waves and reduces 4 x 64 accumulators");

// The segments in order, the residual term and the zero rows.  grid = (ceil(Z / 256), T).  w: [2][T][Z].
__global__ __launch_bounds__(kExpBlock) void k_exp_trip_finish(const double *__restrict__ part, int nseg, const double *__restrict__ mean,
                                                               const double *__restrict__ dist, const double *__restrict__ last,
                                                               const int *__restrict__ ell, const double *__restrict__ r, int Z, int T,
                                                               double *__restrict__ w)
{
    const int o = static_cast<int>(blockIdx.x) * kExpBlock + static_cast<int>(threadIdx.x), t = static_cast<int>(blockIdx.y);
    if (o >= Z) return;
    const size_t zt = static_cast<size_t>(Z) * T, row = static_cast<size_t>(t) * Z + o;
    double sec = part[row], km = part[zt + row];
    for (int s = 1; s < nseg; ++s) {
        sec = sec + part[static_cast<size_t>(s) * 2 * zt + row];
        km = km + part[static_cast<size_t>(s) * 2 * zt + zt + row];
    }
    if (last[row] == 0.0) {  // a zero row: the driver stays in o (src/resampling.jl:35-36), a trip inside the zone
        sec = kTripIntraSec;
        km = kTripIntraKm;
    } else {
        const int l = ell[row];
        if (l < Z) {  // the residual of a row total below 1 goes to the last destination with p > 0 (D1)
            const double rr = r[row];
            const size_t cell = static_cast<size_t>(l) * Z + o;
            sec = sec + rr * (l == o ? kTripIntraSec : mean[static_cast<size_t>(t) * Z * Z + cell]);
            km = km + rr * (l == o ? kTripIntraKm : dist[cell]);
        }
    }
    w[row] = sec;
    w[zt + row] = km;
}

// Fleet b = blockIdx.y, chunk g = blockIdx.x of kTravelChunk consecutive words of [T][Z]: seconds = x * w_sec, km = x * w_km over the
// fleet's driving half, and the chunk's two sums.  expected: [B][2][T][Z] (parking | driving), travel: [B][2][T][Z] (seconds | km) or
// nullptr, part: [B][gridDim.x][2] or nullptr (no totals wanted).  (One workgroup per fleet was measured first: 384 dependent rounds
// of three loads at the headline shape, 0.13 ms -- a sixth of the propagation it follows.)
constexpr int kTravelPerThread = 4;
constexpr int kTravelChunk = kExpBlock * kTravelPerThread;
__global__ __launch_bounds__(kExpBlock) void k_exp_travel(const double *__restrict__ expected, const double *__restrict__ w, size_t zt,
                                                          double *__restrict__ travel, double *__restrict__ part)
{
    __shared__ double s_part[kExpWaves * 2];
    __shared__ double s_tot[2];
    const int tid = static_cast<int>(threadIdx.x);
    const size_t b = blockIdx.y, i0 = static_cast<size_t>(blockIdx.x) * kTravelChunk + tid;
    const double *__restrict__ x = expected + b * 2 * zt + zt;
    double *__restrict__ out = travel ? travel + b * 2 * zt : nullptr;
    double xs[kTravelPerThread], ws[kTravelPerThread], wk[kTravelPerThread];
#pragma unroll
    for (int j = 0; j < kTravelPerThread; ++j) {
        const size_t i = i0 + static_cast<size_t>(j) * kExpBlock;
        xs[j] = ws[j] = wk[j] = 0.0;
        if (i < zt) {
            xs[j] = x[i];
            ws[j] = w[i];
            wk[j] = w[zt + i];
        }
    }
    double acc[2] = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < kTravelPerThread; ++j) {
        const size_t i = i0 + static_cast<size_t>(j) * kExpBlock;
        if (i < zt) {
            const double s = xs[j] * ws[j], k = xs[j] * wk[j];
            if (out) {
                out[i] = s;
                out[zt + i] = k;
            }
            acc[0] = acc[0] + s;
            acc[1] = acc[1] + k;
        }
    }
    if (!part) return;  // (uniform)
    exp_block_sum<2>(acc, s_part, s_tot);
    if (tid < 2) part[(b * gridDim.x + blockIdx.x) * 2 + tid] = s_tot[tid];
}

// The chunks of fleet b = blockIdx.x in fixed order: lane l of ONE wave adds chunks l, l + 64, ... in ascending order, then the wave's
// tree.  part: [B][nchunk][2], totals: [B][2].
__global__ __launch_bounds__(64) void k_exp_travel_total(const double *__restrict__ part, int nchunk, double *__restrict__ totals)
{
    const int lane = static_cast<int>(threadIdx.x);
    const size_t b = blockIdx.x;
    double s = 0.0, k = 0.0;
    for (int g = lane; g < nchunk; g += 64) {
        s = s + part[(b * nchunk + g) * 2];
        k = k + part[(b * nchunk + g) * 2 + 1];
    }
    s = obj_wave_sum(s);
    k = obj_wave_sum(k);
    if (lane == 0) {
        totals[b * 2] = s;
        totals[b * 2 + 1] = k;
    }
}

}  // namespace cpm
