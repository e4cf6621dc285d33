// cpm_count.h -- hour T of a resample, counts only: k_grouped_count, k_batch_count.
//
// Hour T of a resample is sampled and never applied (src/resampling.jl:81-83).  Without travel times, flows or stays all it leaves
// behind is parking[T-1][z] (the bucket sizes) and driving[T-1][z] (the Bernoulli successes): nobody reads where its drivers would
// have gone.  The plain form of the sampler (k_grouped_sample<.., false>) still stages every zone's row pack (76 MB at S4k),
// searches it for every driver and writes dest | drive << 31 per car into ids_next (16 MB).  The kernels here read the ids and
// the thresholds, run Philox once per car and count -- no pack, no search, no store per car.
//
// What they leave behind is, word for word, what the plain form leaves apart from ids_next: parking_t, driving_t, status bit 1 (2)
// when the two ends of a bucket met, and the heavy-bucket words (maxn, nheavy[hour]) that the context reads back after the step to
// size the next one's heavy launch (CPM_INFO_PARTS) -- from the cars per lane the plain launch would have run with, which the
// caller passes (cpt).  A zero row (last_t[z] == 0) does not keep a car from driving -- its destination would have been its
// origin -- so last_t is not read at all.
//
// Separate functions on purpose: the hourly kernels' code does not move (profiles/last_hour_isa_compare.txt).
#pragma once
#include "cpm_grouped.h"

namespace cpm {

constexpr int kCountBlock = 256;
constexpr int kCountDeep = 6;  // id loads a lane has in flight per round: 1,536 slots, the plain form's widest workgroup

// One workgroup, one zone.  Slot s of the bucket is position s + (s >= ns ? cap - n_all : 0) of the zone's region (stayers from the
// bottom, arrivals from the top: grouped_sample_body).  A round loads kCountDeep ids per lane -- clamped to the region, so every
// lane loads and the loads are issued together -- and a wave draws only for the slots of the round in which it holds cars.
__device__ __forceinline__ void grouped_count_body(const GroupedArgs &a, const int z, const uint32_t cpt, uint32_t &s_ndrive)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t cap = a.cap;
    const uint32_t ns_raw = a.cnt_s[z], na_raw = a.cnt_a[z];
    const long long thr = a.thr_t[z];
    const uint32_t ns = min(ns_raw, cap), na = min(na_raw, cap - ns);
    const uint32_t n_all = ns + na;
    const uint32_t *__restrict__ ids = a.ids + static_cast<size_t>(z) * cap;
    if (tid == 0) {
        s_ndrive = 0;
        a.parking_t[z] = n_all;  // every car present at hour t, drivers included (src/saveresults.jl:12)
        if (static_cast<unsigned long long>(ns_raw) + na_raw > cap) atomicOr(a.rare->status, 2ull);  // the two ends of the bucket met: step invalid
        // the heavy-bucket words, as the plain form with cpt cars per lane writes them (grouped_sample_body)
        if (n_all > a.heavy_x * (cpt > 4u ? 4u : cpt) * kCountBlock) {
            const GroupedRare *r = a.rare;
            const uint32_t items = (n_all + cpt * kCountBlock - 1u) / (cpt * kCountBlock) - 1u;
            atomicMax(&r->maxn[0], n_all);
            const uint32_t idx = atomicAdd(r->nheavy + a.hour, items);
            atomicMax(&r->maxn[1], idx + items);
        }
    }
    if (n_all == 0) return;  // driving_t[z] stays 0 (zeroed by the caller)
    const uint32_t gap = cap - n_all, top = cap - 1u;
    const uint32_t wave0 = from_lane0(tid & ~63u);  // this wave's first slot of a round, in a scalar register
    const uint32_t seed_lo = static_cast<uint32_t>(a.seed), seed_hi = static_cast<uint32_t>(a.seed >> 32);
    uint32_t nd = 0;
    for (uint32_t s0 = 0; s0 < n_all; s0 += kCountDeep * kCountBlock) {
        uint32_t id[kCountDeep];
#pragma unroll
        for (int c = 0; c < kCountDeep; ++c) {
            const uint32_t s = s0 + static_cast<uint32_t>(c) * kCountBlock + tid;
            id[c] = ids[min(s + (s >= ns ? gap : 0u), top)];
        }
#pragma unroll
        for (int c = 0; c < kCountDeep; ++c) {
            const uint32_t sc = s0 + static_cast<uint32_t>(c) * kCountBlock;
            if (sc + wave0 >= n_all) break;  // none of this wave's 64 slots holds a car, nor any behind it (no barrier inside the loop)
            const uint64_t car = a.cars.global(id[c]);
            const U4 r = philox4x32_10(static_cast<uint32_t>(car), static_cast<uint32_t>(car >> 32), a.step, 0u, seed_lo, seed_hi);
            const long long kb = static_cast<long long>(((static_cast<uint64_t>(r.y) << 32) | r.x) >> 11);
            nd += ((sc + tid < n_all) & (kb <= thr)) ? 1u : 0u;  // u <= p_drive[origin,t] (src/resampling.jl:15) in integers
        }
    }
    for (int o = 32; o > 0; o >>= 1) nd += __shfl_down(nd, o, 64);
    __syncthreads();  // s_ndrive is zero
    if (lane == 0 && nd) atomicAdd(&s_ndrive, nd);
    __syncthreads();
    if (tid == 0) a.driving_t[z] = s_ndrive;
}

// grid = Z.  cpt: the cars per lane grouped_launch_sample<false> would have chosen for this launch.
__global__ __launch_bounds__(kCountBlock) void k_grouped_count(GroupedArgs a, uint32_t cpt)
{
    __shared__ uint32_t s_ndrive;
    grouped_count_body(a, blockIdx.x, cpt, s_ndrive);
}

// The batched resample's hour T (cpm_batch.h): grid = (Z, fleets), fleet f reads its resident record of the hour.
__global__ __launch_bounds__(kCountBlock) void k_batch_count(const GroupedArgs *__restrict__ fleets, uint32_t cpt)
{
    __shared__ uint32_t s_ndrive;
    grouped_count_body(fleets[blockIdx.y], blockIdx.x, cpt, s_ndrive);
}

inline hipError_t grouped_launch_count(const GroupedArgs &a, int64_t mean, bool heavy_follows, hipStream_t stream)
{
    const uint32_t cpt = static_cast<uint32_t>(heavy_follows ? grouped_cpt(mean) : grouped_cpt_wide(mean));
    launch_cells().sampler(kCellCount | cpt << 8 | (a.smap ? kCellSparse : 0u) << 24);  // (a run-time argument here: the value the kernel is handed)
    launch(k_grouped_count, dim3(a.Z), dim3(kCountBlock), 0, stream, a, cpt);
    return hipSuccess;  // (no dynamic LDS: nothing to be refused)
}

}  // namespace cpm
