// cpm_flows.h -- the hourly origin-destination trip counts of a resample (include/cpm_flows.h): flows[t][o][d] = cars that drove
// (transition_matrix[i,t,1] == 1, src/resampling.jl:19-21) from zone o + 1 (state_matrix[i,t]) to zone d + 1 (transition_matrix[i,t,2],
// :47) in hour t + 1.  Nothing here touches a sampler or a placing kernel: the grouped family's drivers of an hour sit in the 32 runs
// of their origin zone as id | local destination << idbits (cpm_grouped.h: Dq / cntg), and k_grouped_flows reads them back the way
// k_grouped_travel does, with an LDS histogram in place of the draw.  The other two families keep a record per car and hour
// (dest | drive flag << 31): k_flows_cars adds those up with global atomics.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "cpm_kernels.h"

namespace cpm {

constexpr int kFlowRuns = 32;        // runs per origin zone (= kGroups of cpm_grouped.h, asserted where the kernel is launched)
constexpr int kFlowsBlock = 256;     // 8 lanes per run
constexpr int kFlowsQuads = 4;       // 16-byte loads a lane has in flight per pass over its run (8 lanes x 4 x 4 = 128 entries of a run)
typedef uint32_t flows_u32x4 __attribute__((ext_vector_type(4)));

// LDS of a block: the row's histogram, shifted by up to three words so that a word's LDS address and its address in the output agree
// modulo 16 bytes (Z need not be a multiple of 4: a row may start off a 16-byte boundary), in whole 16-byte pieces
inline size_t flows_lds_bytes(int Z) { return (static_cast<size_t>(Z) + 3 + 3) / 4 * 16; }

// One block per (origin zone, hour): grid (Z, 1) behind an hour's launches, or (Z, T) over the kept runs of a whole resample
// (d_stride / c_stride: words between the runs / run lengths of consecutive hours).  `flows` is the row block of hour blockIdx.y = 0.
// Every (hour, origin) row is written by exactly one block, empty zones included: no global atomic, no memset of the output.
__global__ __launch_bounds__(kFlowsBlock) void k_grouped_flows(const uint32_t *__restrict__ D, const uint32_t *__restrict__ cntg, int Z, uint32_t scap,
                                                               uint32_t idbits, uint32_t zpg, size_t d_stride, size_t c_stride,
                                                               int32_t *__restrict__ flows)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t flow_bins[];
    const int z = blockIdx.x;
    const int tid = threadIdx.x;
    const uint32_t g = static_cast<uint32_t>(tid) >> 3, j = static_cast<uint32_t>(tid) & 7u;
    D += d_stride * blockIdx.y + (static_cast<size_t>(z) * kFlowRuns + g) * scap;  // (scap is a multiple of 32 words: every run starts on a 128-byte line)
    // the run's length and the lane's first pieces are requested together: a run is scap >= 64 words whatever its length, so the
    // loads of the first pass are in bounds before the length is known (what lies behind the run's end is masked below)
    const uint32_t len_raw = cntg[c_stride * blockIdx.y + static_cast<size_t>(z) * kFlowRuns + g];
    flows_u32x4 q[kFlowsQuads];
#pragma unroll
    for (int u = 0; u < kFlowsQuads; ++u) {
        const uint32_t k = min((j + 8u * u) * 4u, scap - 4u);
        q[u] = *reinterpret_cast<const flows_u32x4 *>(D + k);
    }
    int32_t *row = flows + (static_cast<size_t>(blockIdx.y) * Z + z) * Z;  // (64-bit: T * Z^2 passes 2^31 words from Z = 8,192 on)
    const uint32_t shift = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(row) >> 2) & 3u;
    const uint32_t nquad = (static_cast<uint32_t>(Z) + shift + 3u) / 4u;
    flows_u32x4 *bins4 = reinterpret_cast<flows_u32x4 *>(flow_bins);
    for (uint32_t i = tid; i < nquad; i += kFlowsBlock) bins4[i] = flows_u32x4{0u, 0u, 0u, 0u};
    __syncthreads();
    const uint32_t len = min(len_raw, scap);  // (a run that outgrew scap has raised the status word: the attempt is discarded)
    const uint32_t gbase = g * zpg + shift;
    auto bin = [&](uint32_t entry, uint32_t at) {
        const uint32_t b = gbase + (entry >> idbits);
        if (at < len && b < static_cast<uint32_t>(Z) + shift) atomicAdd(&flow_bins[b], 1u);
    };
#pragma unroll
    for (int u = 0; u < kFlowsQuads; ++u) {
        const uint32_t k = (j + 8u * u) * 4u;
        bin(q[u].x, k);
        bin(q[u].y, k + 1u);
        bin(q[u].z, k + 2u);
        bin(q[u].w, k + 3u);
    }
    // runs longer than a pass (popular destination groups): the same again, kFlowsQuads pieces in flight per lane
    for (uint32_t k0 = 32u * kFlowsQuads; k0 < len; k0 += 32u * kFlowsQuads) {
#pragma unroll
        for (int u = 0; u < kFlowsQuads; ++u) {
            const uint32_t k = min(k0 + (j + 8u * u) * 4u, scap - 4u);
            q[u] = *reinterpret_cast<const flows_u32x4 *>(D + k);
        }
#pragma unroll
        for (int u = 0; u < kFlowsQuads; ++u) {
            const uint32_t k = k0 + (j + 8u * u) * 4u;  // (at or behind the run's end where the load above was clamped: masked)
            bin(q[u].x, k);
            bin(q[u].y, k + 1u);
            bin(q[u].z, k + 2u);
            bin(q[u].w, k + 3u);
        }
    }
    __syncthreads();
    // the row: 16-byte stores, consecutive lanes on consecutive addresses; narrower ones for the pieces its two ends share with its neighbours
    int32_t *row16 = row - shift;
    const uint32_t end = static_cast<uint32_t>(Z) + shift;
    for (uint32_t i = tid; i < nquad; i += kFlowsBlock) {
        const flows_u32x4 v = bins4[i];
        const uint32_t w0 = 4u * i;
        if (w0 >= shift && w0 + 4u <= end) {
            *reinterpret_cast<flows_u32x4 *>(row16 + w0) = v;
        } else {
            if (w0 >= shift && w0 < end) row16[w0] = static_cast<int32_t>(v.x);
            if (w0 + 1u >= shift && w0 + 1u < end) row16[w0 + 1u] = static_cast<int32_t>(v.y);
            if (w0 + 2u >= shift && w0 + 2u < end) row16[w0 + 2u] = static_cast<int32_t>(v.z);
            if (w0 + 3u >= shift && w0 + 3u < end) row16[w0 + 3u] = static_cast<int32_t>(v.w);
        }
    }
}

// The histogram above 48 KiB of LDS (Z > 12,286) is asked for by name, once per device, and the answer is read: a launch that was
// not granted its LDS comes back "invalid argument" hours later in the stream (what an unchecked one cost cpm_exact.h).
inline hipError_t flows_lds_opt_in(size_t lds)
{
    if (lds <= 48 * 1024) return hipSuccess;
    static size_t granted[64] = {};
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64 && granted[dev] >= lds) return hipSuccess;
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(k_grouped_flows), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
    if (e == hipSuccess && dev >= 0 && dev < 64) granted[dev] = lds;
    return e;
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
    hipError_t e = flows_lds_opt_in(lds);
    if (e == hipSuccess) {
        launch(k_grouped_flows, dim3(static_cast<unsigned>(Z), static_cast<unsigned>(nt)), dim3(kFlowsBlock), lds, stream, D, cntg, Z, scap, idbits, zpg, d_stride,
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
    uint32_t o;
    if (off) {
        uint32_t lo = 0, hi = static_cast<uint32_t>(Z);  // off[lo] <= i < off[hi]
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (off[mid] <= static_cast<uint32_t>(i)) lo = mid;
            else hi = mid;
        }
        o = lo;
    } else {
        o = zsrc[i] & kZoneMask;
    }
    const uint32_t d = r & kZoneMask;
    if (o < static_cast<uint32_t>(Z) && d < static_cast<uint32_t>(Z)) atomicAdd(&flows_t[static_cast<size_t>(o) * Z + d], 1);
}

inline hipError_t flows_launch_cars(hipStream_t stream, const uint32_t *zsrc, const uint32_t *off, const uint32_t *rec_t, int64_t n, int Z, int32_t *flows_t)
{
    launch(k_flows_cars, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, stream, zsrc, off, rec_t, n, Z, flows_t);
    return hipGetLastError();
}

}  // namespace cpm
