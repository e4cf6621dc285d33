// cpm_flows.h -- the hourly origin-destination trip counts of a resample (include/cpm_flows.h): flows[t][o][d] = cars that drove
// (transition_matrix[i,t,1] == 1, src/resampling.jl:19-21) from zone o + 1 (state_matrix[i,t]) to zone d + 1 (transition_matrix[i,t,2],
// :47) in hour t + 1.  Nothing here touches a sampler or a placing kernel: the grouped family's drivers of an hour sit in the runs of
// their origin zone, which k_grouped_flows reads back through the reader of cpm_runs.h into an LDS histogram.  The other two families
// keep a record per car and hour (dest | drive flag << 31): k_flows_cars adds those up with global atomics.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "cpm_kernels.h"
#include "cpm_runs.h"

namespace cpm {

// LDS of a block: the row's histogram, shifted by up to three words so that a word's LDS address and its address in the output agree
// modulo 16 bytes (Z need not be a multiple of 4: a row may start off a 16-byte boundary), in whole 16-byte pieces
inline size_t flows_lds_bytes(int Z) { return (static_cast<size_t>(Z) + 3 + 3) / 4 * 16; }

// One block per (origin zone, hour): grid (Z, 1) behind an hour's launches, or (Z, T) over the kept runs of a whole resample
// (d_stride / c_stride: words between the runs / run lengths of consecutive hours).  `flows` is the row block of hour blockIdx.y = 0.
// Every (hour, origin) row is written by exactly one block, empty zones included: no global atomic, no memset of the output.
__global__ __launch_bounds__(kRunsBlock) void k_grouped_flows(const uint32_t *__restrict__ D, const uint32_t *__restrict__ cntg, int Z, uint32_t scap,
                                                              uint32_t idbits, uint32_t zpg, size_t d_stride, size_t c_stride,
                                                              int32_t *__restrict__ flows)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t flow_bins[];
    RunLane r = run_open(D, cntg, scap, d_stride * blockIdx.y, c_stride * blockIdx.y);
    int32_t *row = flows + (static_cast<size_t>(blockIdx.y) * Z + blockIdx.x) * Z;  // (64-bit: T * Z^2 passes 2^31 words from Z = 8,192 on)
    const uint32_t shift = row_shift(row);
    const uint32_t nquad = (static_cast<uint32_t>(Z) + shift + 3u) / 4u;
    runs_u32x4 *bins4 = reinterpret_cast<runs_u32x4 *>(flow_bins);
    for (uint32_t i = threadIdx.x; i < nquad; i += kRunsBlock) bins4[i] = runs_u32x4{0u, 0u, 0u, 0u};
    __syncthreads();
    const uint32_t gbase = r.g * zpg + shift;
    run_walk(r, [&](uint32_t k0, uint32_t len) {
        run_entries(r, k0, len, [&](int, uint32_t entry, bool live) {
            const uint32_t b = gbase + (entry >> idbits);
            if (live && b < static_cast<uint32_t>(Z) + shift) atomicAdd(&flow_bins[b], 1u);
        });
    });
    __syncthreads();
    row_store_shifted(row, static_cast<uint32_t>(Z), [&](uint32_t i, uint32_t) { return bins4[i]; });  // (the histogram lies on the row's grid)
}

// hours t0 .. t0 + nt - 1 from the runs at D / cntg (nt > 1: the kept runs of consecutive hours, d_stride / c_stride words apart)
inline int32_t flows_launch_grouped(hipStream_t stream, const uint32_t *D, const uint32_t *cntg, int Z, uint32_t scap, uint32_t idbits, uint32_t zpg,
                                    size_t d_stride, size_t c_stride, int t0, int nt, int32_t *d_flows, std::string &err)
{
    const size_t lds = flows_lds_bytes(Z);
    if (lds + 64 > 160 * 1024) {
        err = "flows: a row of this many zones does not fit the histogram in LDS";
        return CPM_ERR_ARG;
    }
    hipError_t e = lds_opt_in<k_grouped_flows>(lds);
    if (e == hipSuccess) {
        launch(k_grouped_flows, dim3(static_cast<unsigned>(Z), static_cast<unsigned>(nt)), dim3(kRunsBlock), lds, stream, D, cntg, Z, scap, idbits, zpg, d_stride,
               c_stride, d_flows + static_cast<size_t>(t0) * Z * Z);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        err = std::string("flows histogram (") + std::to_string(lds) + " B of LDS): " + hipGetErrorString(e);
        return CPM_ERR_HIP;
    }
    return CPM_OK;
}

// The per-car families: one thread per car of ONE hour.  rec_t[i] = destination | drive flag << 31 of slot i; the slot's zone is
// zsrc[i] (CPM_KERNEL_CAR: slots are cars) or, off != nullptr, the bucket z with off[z] <= i < off[z + 1] (CPM_KERNEL_ZONE_LDS: slots
// are the exact layout's, bucket by bucket).  flows_t (zeroed by the caller) is the hour's Z x Z block.
__global__ __launch_bounds__(256) void k_flows_cars(const uint32_t *__restrict__ zsrc, const uint32_t *__restrict__ off, const uint32_t *__restrict__ rec_t,
                                                    int64_t n, int Z, int32_t *__restrict__ flows_t)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = rec_t[i];
    if (!(r & kDriveBit)) return;
    const uint32_t o = off ? slot_bucket(off, Z, static_cast<uint32_t>(i)) : zsrc[i] & kZoneMask;
    const uint32_t d = r & kZoneMask;
    if (o < static_cast<uint32_t>(Z) && d < static_cast<uint32_t>(Z)) atomicAdd(&flows_t[static_cast<size_t>(o) * Z + d], 1);
}

inline hipError_t flows_launch_cars(hipStream_t stream, const uint32_t *zsrc, const uint32_t *off, const uint32_t *rec_t, int64_t n, int Z, int32_t *flows_t)
{
    launch(k_flows_cars, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, stream, zsrc, off, rec_t, n, Z, flows_t);
    return hipGetLastError();
}

}  // namespace cpm
