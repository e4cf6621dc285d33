// cpm_stays.h -- how long a car stays parked before it drives again (include/cpm_stays.h), by zone and hour.  Hours are 0-based:
// t = 0 .. T-1 is the reference's hour t+1.
//   arrival hour  a(i,t) = 0 if car i drove in no hour s < t, else (the last s < t with transition_matrix[i,s,1] == 1) + 1.
//   stays[(t*Z + z)*T + L] = cars with state_matrix[i,t] == z+1, transition_matrix[i,t,1] == 1 and t - a(i,t) == L.
//   parked[z*T + a]        = cars with state_matrix[i,T-1] == z+1 that did not drive in hour T-1 and have a(i,T-1) == a.
// This is the first per-car quantity carried ACROSS hours on the grouped path, whose buckets forget which car is which: a driver's
// entry in its origin zone's runs (cpm_runs.h) is id | local destination << idbits, id the context-local car index, and the side
// array last[n] is indexed by it:
//   last[i] = since << 24 | zone: the car has been parked in `zone` since hour `since` (= the hour of its last drive + 1, at most T:
//   8 bits, T <= 255; zone < 2^24); 0 = where the day began (the context's zone0[i]), since hour 0.
// Zeroed at the start of every attempt.  A car drives at most once an hour and sits in one zone, so the launches of ONE hour never
// touch a word twice; the launches of consecutive hours must run in hour order (never a grid of (Z, T)).  Nothing here touches a
// sampler or a placing kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "cpm_kernels.h"
#include "cpm_runs.h"

namespace cpm {

constexpr int kStaysWaves = kRunsBlock / 64;
constexpr int kStaysSmall = 4;         // stay lengths counted in registers (most stays are short: one LDS address would serialise)
constexpr int kStaysMaxT = 255;        // `since` is 8 bits of the word
constexpr uint32_t kStaySinceShift = 24;
constexpr uint32_t kStayZoneMask = (1u << kStaySinceShift) - 1u;

inline size_t stays_lds_bytes(int T) { return sizeof(uint32_t) * kStaysWaves * static_cast<size_t>(T); }

// One block per origin zone, ONE hour (t) per launch: the runs of the hour at D / cntg.  stays_t is the hour's [Z][T] block.
// Every (t, z) row is written by exactly one block, empty zones included: no global atomic, no memset of the output.
__global__ __launch_bounds__(kRunsBlock) void k_grouped_stays(const uint32_t *__restrict__ D, const uint32_t *__restrict__ cntg, int Z, uint32_t scap,
                                                              uint32_t idbits, uint32_t zpg, int T, int t, uint32_t n, uint32_t *__restrict__ last,
                                                              int32_t *__restrict__ stays_t)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t stay_bins[];  // [kStaysWaves][T]: a histogram per wave
    const int tid = threadIdx.x;
    RunLane r = run_open(D, cntg, scap, 0, 0);
    for (int i = tid; i < kStaysWaves * T; i += kRunsBlock) stay_bins[i] = 0u;
    __syncthreads();
    const uint32_t idmask = (idbits >= 32) ? 0xFFFFFFFFu : ((1u << idbits) - 1u);
    const uint32_t gbase = r.g * zpg;
    const uint32_t now = static_cast<uint32_t>(t + 1) << kStaySinceShift;
    uint32_t *wbins = stay_bins + (static_cast<uint32_t>(tid) >> 6) * T;
    uint32_t small[kStaysSmall] = {};
    // a pass: the lane's 16 entries -> 16 gathers in flight -> bins and the new words
    run_walk(r, [&](uint32_t k0, uint32_t len) {
        uint32_t id[4 * kRunsQuads], dest[4 * kRunsQuads], w[4 * kRunsQuads];
        bool ok[4 * kRunsQuads];
        run_entries(r, k0, len, [&](int s, uint32_t entry, bool live) {
            id[s] = entry & idmask;
            dest[s] = gbase + (entry >> idbits);
            ok[s] = live && id[s] < n && dest[s] < static_cast<uint32_t>(Z);  // (nothing is gathered or stored out of range)
        });
#pragma unroll
        for (int s = 0; s < 4 * kRunsQuads; ++s) w[s] = ok[s] ? last[id[s]] : 0u;
#pragma unroll
        for (int s = 0; s < 4 * kRunsQuads; ++s) {
            if (!ok[s]) continue;
            const uint32_t L = static_cast<uint32_t>(t) - (w[s] >> kStaySinceShift);  // (since <= t in a valid attempt; else masked)
#pragma unroll
            for (int l = 0; l < kStaysSmall; ++l) small[l] += (L == static_cast<uint32_t>(l)) ? 1u : 0u;
            if (L >= static_cast<uint32_t>(kStaysSmall) && L < static_cast<uint32_t>(T)) atomicAdd(&wbins[L], 1u);
            last[id[s]] = now | dest[s];
        }
    });
    // the short stays: summed across the wave, one LDS add per wave and length
#pragma unroll
    for (int l = 0; l < kStaysSmall; ++l) {
        uint32_t v = small[l];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((tid & 63) == 0 && l < T && v) atomicAdd(&wbins[l], v);
    }
    __syncthreads();
    // the row: T words, the waves' histograms summed (rows are 16-byte aligned at T = 24, not at T = 7)
    row_store_shifted(stays_t + static_cast<size_t>(blockIdx.x) * T, static_cast<uint32_t>(T), [&](uint32_t i, uint32_t shift) {
        uint32_t v[4];
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const uint32_t wd = 4u * i + x - shift;  // (the row's word; wraps for the words in front of it)
            uint32_t s = 0u;
            if (wd < static_cast<uint32_t>(T)) {
#pragma unroll
                for (int wv = 0; wv < kStaysWaves; ++wv) s += stay_bins[wv * T + wd];
            }
            v[x] = s;
        }
        return runs_u32x4{v[0], v[1], v[2], v[3]};
    });
}

// hour t from the runs at D / cntg
inline int32_t stays_launch_grouped(hipStream_t stream, const uint32_t *D, const uint32_t *cntg, int Z, uint32_t scap, uint32_t idbits, uint32_t zpg, int T,
                                    int t, int64_t n, const StaysDest &sd, std::string &err)
{
    launch(k_grouped_stays, dim3(static_cast<unsigned>(Z)), dim3(kRunsBlock), stays_lds_bytes(T), stream, D, cntg, Z, scap, idbits, zpg, T, t,
           static_cast<uint32_t>(n), sd.last, sd.stays + static_cast<size_t>(t) * Z * T);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        err = std::string("stays of the hour: ") + hipGetErrorString(e);
        return CPM_ERR_HIP;
    }
    return CPM_OK;
}

// The per-car families: one thread per slot of ONE hour.  rec_t[i] = destination | drive flag << 31 of slot i; the slot's car is
// ids[i] (CPM_KERNEL_ZONE_LDS: the exact layout, bucket by bucket) or i itself (ids == nullptr, CPM_KERNEL_CAR); its zone is zsrc[i]
// or, off != nullptr, the bucket z with off[z] <= i < off[z + 1].  stays_t (zeroed by the caller) is the hour's [Z][T] block.
__global__ __launch_bounds__(256) void k_stays_cars(const uint32_t *__restrict__ ids, const uint32_t *__restrict__ zsrc, const uint32_t *__restrict__ off,
                                                    const uint32_t *__restrict__ rec_t, int64_t n, int Z, int T, int t, uint32_t *__restrict__ last,
                                                    int32_t *__restrict__ stays_t)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = rec_t[i];
    if (!(r & kDriveBit)) return;
    const uint32_t o = off ? slot_bucket(off, Z, static_cast<uint32_t>(i)) : zsrc[i] & kZoneMask;
    const uint32_t car = ids ? ids[i] : static_cast<uint32_t>(i);
    const uint32_t d = r & kZoneMask;
    if (o >= static_cast<uint32_t>(Z) || d >= static_cast<uint32_t>(Z) || car >= static_cast<uint64_t>(n)) return;
    const uint32_t L = static_cast<uint32_t>(t) - (last[car] >> kStaySinceShift);
    if (L < static_cast<uint32_t>(T)) atomicAdd(&stays_t[static_cast<size_t>(o) * T + L], 1);
    last[car] = (static_cast<uint32_t>(t + 1) << kStaySinceShift) | d;
}

inline hipError_t stays_launch_cars(hipStream_t stream, const uint32_t *ids, const uint32_t *zsrc, const uint32_t *off, const uint32_t *rec_t, int64_t n, int Z,
                                    int T, int t, const StaysDest &sd)
{
    launch(k_stays_cars, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, stream, ids, zsrc, off, rec_t, n, Z, T, t, sd.last,
           sd.stays + static_cast<size_t>(t) * Z * T);
    return hipGetLastError();
}

// The stays still open when the day ends, behind the last hour of every family: one thread per car.  A car that drove in hour
// T-1 (since == T) has ended its stay; one that never drove is where the day began (zone0).  parked (zeroed by the caller) gets one
// add per run of neighbouring lanes with the same cell: cars that never left their zone lie side by side in a fleet built zone by
// zone, and the rest of the cells are spread over Z * T addresses.
__global__ __launch_bounds__(256) void k_stays_parked(const uint32_t *__restrict__ last, const uint32_t *__restrict__ zone0, int64_t n, int Z, int T,
                                                      int32_t *__restrict__ parked)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    uint32_t key = 0xFFFFFFFFu;  // no cell
    if (i < n) {
        const uint32_t w = last[i];
        const uint32_t a = w >> kStaySinceShift;
        const uint32_t z = w ? (w & kStayZoneMask) : (zone0[i] & kZoneMask);
        if (a < static_cast<uint32_t>(T) && z < static_cast<uint32_t>(Z)) key = z * static_cast<uint32_t>(T) + a;
    }
    const uint32_t lane = static_cast<uint32_t>(threadIdx.x) & 63u;
    const uint32_t prev = __shfl_up(key, 1, 64);
    const bool head = lane == 0 || prev != key;
    const unsigned long long heads = __ballot(head);
    if (head && key != 0xFFFFFFFFu) {
        const unsigned long long above = lane == 63u ? 0ull : (heads >> (lane + 1u));
        const uint32_t run = above ? static_cast<uint32_t>(__ffsll(static_cast<long long>(above))) : 64u - lane;
        atomicAdd(&parked[key], static_cast<int32_t>(run));
    }
}

inline hipError_t stays_launch_parked(hipStream_t stream, const uint32_t *zone0, int64_t n, int Z, int T, const StaysDest &sd)
{
    launch(k_stays_parked, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, stream, sd.last, zone0, n, Z, T, sd.parked);
    return hipGetLastError();
}

}  // namespace cpm
