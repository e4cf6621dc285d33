// cpm_charge.h -- the state of charge of every car's battery over the day (include/cpm_charge.h): Wh delivered by the chargers and Wh
// taken by trips, by zone and hour, and the trips the battery did not cover.  Hours are 0-based: t = 0 .. T-1 is the reference's
// hour t+1.  The first side output that carries a QUANTITY from hour to hour: the side array ebat[n], indexed by the context-local
// car id of a driver's run entry (cpm_runs.h), holds one 8-byte word per car,
//   ebat[i] = {since << 24 | zone, E}: the car has been parked in `zone` since hour `since` (as last[] of cpm_stays.h) and held E Wh
//   when that stay began.
// The hourly kernels are lazy: a parked car is never touched.  Its charging is settled in closed form when it next drives, by the
// block of its origin zone -- the zone it has been parked in, so the charger power P_z is uniform across the block -- and the
// stays still open when the day ends are settled by k_charge_close.  k_charge_init fills the side array at the start of EVERY attempt,
// so a repaired step never sees a discarded attempt's words; `charge` is zeroed there too.  A car drives at most once an hour, so
// the launches of ONE hour never touch a word twice; the launches of consecutive hours run in hour order (never a grid of (Z, T)).
// No kernel here waits for another block, and nothing here touches a sampler or a placing kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "cpm_kernels.h"
#include "cpm_rng.h"
#include "cpm_runs.h"
#include "cpm_stays.h"

namespace cpm {

constexpr int kChargeWaves = kRunsBlock / 64;
constexpr int kChargeSmall = 3;  // parked hours t-1, t-2, t-3 are summed in registers (most stays are short: one LDS address would serialise)

inline size_t charge_lds_bytes(int T) { return sizeof(unsigned long long) * kChargeWaves * static_cast<size_t>(T); }

// what the kernels of one hour share
struct ChargeHour {
    const double *dist;  // [Z][Z] origin-major: the distance from o to d is dist[o * Z + d] (k_charge_dist_rows; measured against a gather from the resident matrix: DESIGN.md 8)
    const uint32_t *zone_power;
    uint2 *ebat;
    int64_t *charge, *used;
    int32_t *shrt;
    double wh_per_km;
    uint64_t seed;
    CarIndex cars;
    uint32_t capacity, power;
    uint32_t step;  // the Philox step of the hour: T - 1 + t
};

// The mass of the distance draw's window: sigma = 0.1 mu makes a = (0.1 mu) / sigma = 1 for every finite non-zero mean, so the mass
// is one number (truncnormal_mass of such a cell).  mu = 0, NaN or infinite gives a NaN there and a mass of 0: the draw is the mean.
__device__ __forceinline__ double charge_mass1() { return truncnormal_mass(10.0, 0.1 * 10.0); }

// Wh of the trip of global car `car` from o to d at Philox step `step` (include/cpm_charge.h: u)
__device__ __forceinline__ double charge_trip_wh(const ChargeHour &a, uint64_t car, uint32_t o, uint32_t d, int Z, double mass1)
{
    double km = 1.0;  // a trip inside a zone (src/resampling.jl:58-60)
    if (d != o) {
        const double mu = a.dist[static_cast<size_t>(o) * Z + d];
        const double sigma = 0.1 * mu;
        double u1, u2;
        car_uniforms(a.seed, car, a.step, 2u, u1, u2);
        km = truncnormal_draw(u1, mu, sigma, (sigma > 0.0 && sigma < __builtin_inf()) ? mass1 : 0.0);
    }
    double u = __builtin_rint(km * a.wh_per_km);
    if (!(u >= 0.0)) u = 0.0;
    return u;
}

// The stay [since, until) of a car that held E <= cap Wh when it began, at P Wh per hour: add(hour, wh) for every hour that
// delivers something -- P for k = need / P hours, the remainder in the next, nothing after -- and the charge when it ends.
template <typename F>
__device__ __forceinline__ uint32_t charge_settle(uint32_t E, uint32_t cap, uint32_t P, uint32_t since, uint32_t until, F &&add)
{
    const uint32_t need = cap - E;
    if (P == 0u || need == 0u || since >= until) return E;
    const uint32_t L = until - since;
    const uint32_t k = need / P, rem = need - k * P;
    const uint32_t full = min(k, L);
    for (uint32_t j = 0; j < full; ++j) add(since + j, P);
    if (k < L && rem) add(since + k, rem);
    return k < L ? cap : E + full * P;
}

// The origin-major copy of the distance matrix, rows[o * Z + d] = dist[o + Z * d], built once per distance matrix: 32 x 32 tiles through
// LDS, so that both sides are read and written along their rows.  A block of k_grouped_charge then reads ONE row of 8 * Z bytes.
__global__ __launch_bounds__(256) void k_charge_dist_rows(const double *__restrict__ dist, int Z, double *__restrict__ rows)
{
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
    const int o0 = blockIdx.x * 32, d0 = blockIdx.y * 32;
    for (int k = ty; k < 32; k += 8) {  // tile[d][o], read along o
        const int o = o0 + tx, d = d0 + k;
        tile[k][tx] = (o < Z && d < Z) ? dist[o + static_cast<size_t>(Z) * d] : 0.0;
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {  // written along d
        const int o = o0 + k, d = d0 + tx;
        if (o < Z && d < Z) rows[static_cast<size_t>(o) * Z + d] = tile[tx][k];
    }
}

inline hipError_t charge_launch_dist_rows(hipStream_t stream, const double *dist, int Z, double *rows)
{
    const unsigned g = static_cast<unsigned>((Z + 31) / 32);
    launch(k_charge_dist_rows, dim3(g, g), dim3(256), 0, stream, dist, Z, rows);
    return hipGetLastError();
}

// the side array and the charging load at the start of an attempt: one coalesced pass
__global__ __launch_bounds__(256) void k_charge_init(const uint32_t *__restrict__ zone0, const uint32_t *__restrict__ soc_in, uint32_t initial, uint32_t capacity,
                                                     int64_t n, uint2 *__restrict__ ebat, int64_t *__restrict__ charge, int64_t cells)
{
    const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n || i < cells; i += stride) {
        if (i < n) ebat[i] = make_uint2(zone0[i] & kStayZoneMask, soc_in ? min(soc_in[i], capacity) : initial);
        if (i < cells) charge[i] = 0;
    }
}

// One block per origin zone, ONE hour (t) per launch: the runs of the hour at D / cntg.  After the barrier the block is the only
// writer of zone z's rows in this launch: it adds its bins to charge[z][0 .. t-1] with plain loads and stores (stream order carries
// the sums from one hour's launch to the next) and writes used[z][t] and short[z][t], empty zones included: no global atomic.
__global__ __launch_bounds__(kRunsBlock) void k_grouped_charge(const uint32_t *__restrict__ D, const uint32_t *__restrict__ cntg, int Z, uint32_t scap,
                                                               uint32_t idbits, uint32_t zpg, int T, int t, uint32_t n, ChargeHour a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned long long charge_bins[];  // [kChargeWaves][T]: a histogram per wave
    __shared__ unsigned long long s_used;
    __shared__ uint32_t s_short;
    const int tid = threadIdx.x;
    RunLane r = run_open(D, cntg, scap, 0, 0);
    for (int i = tid; i < kChargeWaves * T; i += kRunsBlock) charge_bins[i] = 0ull;
    if (tid == 0) {
        s_used = 0ull;
        s_short = 0u;
    }
    const uint32_t z = blockIdx.x;
    const uint32_t P = a.zone_power ? a.zone_power[z] : a.power;  // (uniform: one scalar load)
    const uint32_t cap = a.capacity;
    const double mass1 = charge_mass1();
    __syncthreads();
    const uint32_t idmask = (idbits >= 32) ? 0xFFFFFFFFu : ((1u << idbits) - 1u);
    const uint32_t gbase = r.g * zpg;
    const uint32_t ut = static_cast<uint32_t>(t);
    const uint32_t now = (ut + 1u) << kStaySinceShift;
    unsigned long long *wbins = charge_bins + (static_cast<uint32_t>(tid) >> 6) * T;
    unsigned long long small[kChargeSmall] = {};  // Wh of the parked hours t-1-l
    unsigned long long used = 0ull;
    uint32_t shrt = 0u;
    // a pass: the lane's 16 entries -> 16 gathers in flight -> the stays settled, the trips taken, the new words
    run_walk(r, [&](uint32_t k0, uint32_t len) {
        uint32_t id[4 * kRunsQuads], dest[4 * kRunsQuads];
        uint2 w[4 * kRunsQuads];
        bool ok[4 * kRunsQuads];
        run_entries(r, k0, len, [&](int s, uint32_t entry, bool live) {
            id[s] = entry & idmask;
            dest[s] = gbase + (entry >> idbits);
            ok[s] = live && id[s] < n && dest[s] < static_cast<uint32_t>(Z);  // (nothing is gathered or stored out of range)
        });
#pragma unroll
        for (int s = 0; s < 4 * kRunsQuads; ++s) w[s] = ok[s] ? a.ebat[id[s]] : make_uint2(0u, 0u);
#pragma unroll
        for (int s = 0; s < 4 * kRunsQuads; ++s) {
            if (!ok[s]) continue;
            const uint32_t since = min(w[s].x >> kStaySinceShift, ut);  // (since <= t in a valid attempt; else clamped: no bin out of range)
            uint32_t E = min(w[s].y, cap);
            const uint32_t need = cap - E, L = ut - since;
            if (P != 0u && need != 0u && L != 0u) {
                const uint32_t k = need / P, rem = need - k * P;
                // hour since + j is the parked hour t-1-l, l = L-1-j: the nearest ones in registers ...
#pragma unroll
                for (int l = 0; l < kChargeSmall; ++l) {
                    const uint32_t j = L - 1u - static_cast<uint32_t>(l);
                    const uint32_t amt = j < k ? P : (j == k ? rem : 0u);
                    small[l] += (static_cast<uint32_t>(l) < L) ? amt : 0u;
                }
                // ... the hours of a longer stay in the wave's histogram
                if (L > static_cast<uint32_t>(kChargeSmall)) {
                    const uint32_t jn = min(L - static_cast<uint32_t>(kChargeSmall), k + 1u);
                    for (uint32_t j = 0; j < jn; ++j) {
                        const uint32_t amt = j < k ? P : rem;
                        if (amt) atomicAdd(&wbins[since + j], static_cast<unsigned long long>(amt));
                    }
                }
                E = k < L ? cap : E + L * P;
            }
            const double u = charge_trip_wh(a, a.cars.global(id[s]), z, dest[s], Z, mass1);
            uint32_t drawn;
            if (u > static_cast<double>(E)) {
                ++shrt;
                drawn = E;
            } else {
                drawn = static_cast<uint32_t>(u);
            }
            used += drawn;
            a.ebat[id[s]] = make_uint2(now | dest[s], E - drawn);
        }
    });
    // the short stays, the energy used and the uncovered trips: summed across the wave, one LDS add per wave and word
#pragma unroll
    for (int l = 0; l < kChargeSmall; ++l) {
        unsigned long long v = small[l];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((tid & 63) == 0 && l < t && v) atomicAdd(&wbins[t - 1 - l], v);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        used += __shfl_xor(used, off, 64);
        shrt += __shfl_xor(shrt, off, 64);
    }
    if ((tid & 63) == 0) {
        if (used) atomicAdd(&s_used, used);
        if (shrt) atomicAdd(&s_short, shrt);
    }
    __syncthreads();
    const size_t row = static_cast<size_t>(z) * T;
    if (tid < t) {
        unsigned long long v = 0ull;
#pragma unroll
        for (int wv = 0; wv < kChargeWaves; ++wv) v += charge_bins[wv * T + tid];
        if (v) a.charge[row + tid] += static_cast<int64_t>(v);
    }
    if (tid == 0) {
        a.used[row + t] = static_cast<int64_t>(s_used);
        a.shrt[row + t] = static_cast<int32_t>(s_short);
    }
}

inline ChargeHour charge_hour_args(const ChargeDest &cd, CarIndex cars, uint64_t seed, int T, int t)
{
    ChargeHour a{};
    a.dist = cd.dist;
    a.zone_power = cd.zone_power;
    a.ebat = cd.ebat;
    a.charge = cd.charge;
    a.used = cd.used;
    a.shrt = cd.shrt;
    a.wh_per_km = cd.wh_per_km;
    a.seed = seed;
    a.cars = cars;
    a.capacity = cd.capacity;
    a.power = cd.power;
    a.step = static_cast<uint32_t>(T - 1 + t);
    return a;
}

inline hipError_t charge_launch_init(hipStream_t stream, const uint32_t *zone0, int64_t n, int Z, int T, const ChargeDest &cd)
{
    const int64_t cells = static_cast<int64_t>(Z) * T;
    const int64_t work = n > cells ? n : cells;
    const unsigned grid = static_cast<unsigned>(std::min<int64_t>((work + 255) / 256, 65536));
    launch(k_charge_init, dim3(grid ? grid : 1u), dim3(256), 0, stream, zone0, cd.soc_in, cd.initial, cd.capacity, n, cd.ebat, cd.charge, cells);
    return hipGetLastError();
}

// hour t from the runs at D / cntg
inline int32_t charge_launch_grouped(hipStream_t stream, const uint32_t *D, const uint32_t *cntg, int Z, uint32_t scap, uint32_t idbits, uint32_t zpg, int T,
                                     int t, int64_t n, CarIndex cars, uint64_t seed, const ChargeDest &cd, std::string &err)
{
    launch(k_grouped_charge, dim3(static_cast<unsigned>(Z)), dim3(kRunsBlock), charge_lds_bytes(T), stream, D, cntg, Z, scap, idbits, zpg, T, t,
           static_cast<uint32_t>(n), charge_hour_args(cd, cars, seed, T, t));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        err = std::string("charge of the hour: ") + hipGetErrorString(e);
        return CPM_ERR_HIP;
    }
    return CPM_OK;
}

// The per-car families: one thread per slot of ONE hour, the records as k_stays_cars reads them (rec_t, ids, zsrc / off).  charge,
// used and short (zeroed by the caller) take global atomics.
__global__ __launch_bounds__(256) void k_charge_cars(const uint32_t *__restrict__ ids, const uint32_t *__restrict__ zsrc, const uint32_t *__restrict__ off,
                                                     const uint32_t *__restrict__ rec_t, int64_t n, int Z, int T, int t, ChargeHour a)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = rec_t[i];
    if (!(r & kDriveBit)) return;
    const uint32_t o = off ? slot_bucket(off, Z, static_cast<uint32_t>(i)) : zsrc[i] & kZoneMask;
    const uint32_t car = ids ? ids[i] : static_cast<uint32_t>(i);
    const uint32_t d = r & kZoneMask;
    if (o >= static_cast<uint32_t>(Z) || d >= static_cast<uint32_t>(Z) || car >= static_cast<uint64_t>(n)) return;
    const uint2 w = a.ebat[car];
    const uint32_t ut = static_cast<uint32_t>(t);
    const uint32_t since = min(w.x >> kStaySinceShift, ut);
    const uint32_t P = a.zone_power ? a.zone_power[o] : a.power;
    const size_t row = static_cast<size_t>(o) * T;
    unsigned long long *charge = reinterpret_cast<unsigned long long *>(a.charge);
    const uint32_t E = charge_settle(min(w.y, a.capacity), a.capacity, P, since, ut,
                                     [&](uint32_t h, uint32_t wh) { atomicAdd(&charge[row + h], static_cast<unsigned long long>(wh)); });
    const double u = charge_trip_wh(a, a.cars.global(car), o, d, Z, charge_mass1());
    uint32_t drawn;
    if (u > static_cast<double>(E)) {
        atomicAdd(&a.shrt[row + t], 1);
        drawn = E;
    } else {
        drawn = static_cast<uint32_t>(u);
    }
    if (drawn) atomicAdd(reinterpret_cast<unsigned long long *>(a.used) + row + t, static_cast<unsigned long long>(drawn));
    a.ebat[car] = make_uint2(((ut + 1u) << kStaySinceShift) | d, E - drawn);
}

inline hipError_t charge_launch_cars(hipStream_t stream, const uint32_t *ids, const uint32_t *zsrc, const uint32_t *off, const uint32_t *rec_t, int64_t n, int Z,
                                     int T, int t, CarIndex cars, uint64_t seed, const ChargeDest &cd)
{
    launch(k_charge_cars, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, stream, ids, zsrc, off, rec_t, n, Z, T, t,
           charge_hour_args(cd, cars, seed, T, t));
    return hipGetLastError();
}

// The stays still open when the day ends, behind the last hour of every family: one thread per car settles [since, T) of a car that
// did not drive in hour T-1 (since < T) into charge[zone][.] and writes soc_out.  Global int64 atomics; cars that never left their
// zone lie side by side in a fleet built zone by zone, so a wave whose charging cars all stand in one zone sums each hour across its
// lanes first and adds once per hour.
__global__ __launch_bounds__(256) void k_charge_close(const uint2 *__restrict__ ebat, const uint32_t *__restrict__ zone_power, uint32_t power, uint32_t capacity,
                                                      int64_t n, int Z, int T, int64_t *__restrict__ charge_out, uint32_t *__restrict__ soc_out)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    unsigned long long *charge = reinterpret_cast<unsigned long long *>(charge_out);
    const uint32_t uT = static_cast<uint32_t>(T);
    uint32_t E = 0u, zone = 0u, since = uT, P = 0u;
    if (i < n) {
        const uint2 w = ebat[i];
        E = min(w.y, capacity);
        zone = w.x & kStayZoneMask;
        since = w.x >> kStaySinceShift;
        if (since < uT && zone < static_cast<uint32_t>(Z)) P = zone_power ? zone_power[zone] : power;
    }
    const uint32_t need = capacity - E;
    const bool act = P != 0u && need != 0u && since < uT;  // (the lane has something to add)
    uint32_t k = 0u, rem = 0u, end = since;               // hours [since, end) deliver: P for k of them, then the remainder
    if (act) {
        const uint32_t L = uT - since;
        k = need / P;
        rem = need - k * P;
        end = since + min(L, rem ? k + 1u : k);
        E = k < L ? capacity : E + L * P;
    }
    const unsigned long long acts = __ballot(act);
    if (acts) {
        const uint32_t z0 = __shfl(zone, __ffsll(static_cast<long long>(acts)) - 1, 64);
        if (__all(!act || zone == z0)) {
            uint32_t lo = act ? since : uT, hi = act ? end : 0u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                lo = min(lo, static_cast<uint32_t>(__shfl_xor(lo, o, 64)));
                hi = max(hi, static_cast<uint32_t>(__shfl_xor(hi, o, 64)));
            }
            for (uint32_t h = lo; h < hi; ++h) {
                unsigned long long v = 0ull;
                if (act && h >= since && h < end) v = (h - since) < k ? P : rem;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
                if ((threadIdx.x & 63) == 0 && v) atomicAdd(&charge[static_cast<size_t>(z0) * T + h], v);
            }
        } else if (act) {
            for (uint32_t h = since; h < end; ++h) atomicAdd(&charge[static_cast<size_t>(zone) * T + h], static_cast<unsigned long long>((h - since) < k ? P : rem));
        }
    }
    if (soc_out && i < n) soc_out[i] = E;
}

inline hipError_t charge_launch_close(hipStream_t stream, int64_t n, int Z, int T, const ChargeDest &cd)
{
    launch(k_charge_close, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, stream, cd.ebat, cd.zone_power, cd.power, cd.capacity, n, Z, T, cd.charge,
           cd.soc);
    return hipGetLastError();
}

}  // namespace cpm
