// cpm_paths.h -- the per-car record of a day (include/cpm_paths.h): one word per car and hour, resident on the device.  Hours are
// 0-based: t = 0 .. T-1 is the reference's hour t+1.
//   paths[t*n + i] = (transition_matrix[i,t,2] - 1) | (transition_matrix[i,t,1] == 1 ? kDriveBit : 0),  i the context-local car index
// which is the word the per-car family keeps in `rec` (kDriveBit, kZoneMask: cpm_kernels.h).  On the grouped path the buckets forget
// which car is which, but a driver's entry in its origin zone's runs (cpm_runs.h) is id | local destination << idbits, id that
// index: the hour's row is
//   carry    every car keeps the zone of the hour before (hour 0: the context's zone0), without the bit: n words streamed;
//   scatter  every driver of the hour overwrites its own word with destination | kDriveBit, straight from the runs.
// A car drives at most once an hour, so the scatter of ONE hour never stores a word twice; carry(t) reads what scatter(t-1) wrote, so
// the launches run in hour order on one stream (never a grid of (Z, T)).  Every word of the record is written by the carry: no memset.
// Nothing here touches a sampler or a placing kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "cpm_kernels.h"
#include "cpm_runs.h"

namespace cpm {

// runs_u32x4 at an address that is a multiple of 4 only (a row of the record starts at byte 4*t*n)
typedef uint32_t paths_u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

// One thread per four cars of ONE hour: dst[i] = src[i] & kZoneMask, src the row of the hour before (or zone0).  The pieces lie on
// dst's 16-byte grid: a piece wholly inside the row is one 16-byte load (src is 4-byte aligned against that grid whenever n is no
// multiple of 4) and one aligned 16-byte store; the pieces at the row's two ends go word by word.
__global__ __launch_bounds__(256) void k_paths_carry(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, uint32_t n)
{
    const uint32_t shift = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(dst) >> 2) & 3u;  // words of the first piece in front of the row
    const uint64_t end = static_cast<uint64_t>(n) + shift;
    const uint64_t w0 = 4ull * (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x);  // in words from dst - shift
    if (w0 >= end) return;
    if (w0 >= shift && w0 + 4u <= end) {
        const runs_u32x4 v = *reinterpret_cast<const paths_u32x4_a4 *>(src + (w0 - shift));
        *reinterpret_cast<runs_u32x4 *>(dst + (w0 - shift)) = v & kZoneMask;
    } else {
#pragma unroll
        for (uint32_t x = 0; x < 4u; ++x)
            if (w0 + x >= shift && w0 + x < end) dst[w0 + x - shift] = src[w0 + x - shift] & kZoneMask;
    }
}

// One block per origin zone, ONE hour per launch: the runs of the hour at D / cntg, paths_t the hour's row (carried already).
// This kernel reads its runs with a body of its own, word for word what run_open / run_walk / run_entries of cpm_runs.h do (keep the
// two in step): on the shared reader its listing differed by two instructions, and six interleaved runs against the parent's library
// did not show its cost inside the parent's own spread at Melbourne x 100 (profiles/runs_notes.md).
__global__ __launch_bounds__(kRunsBlock) void k_grouped_paths(const uint32_t *__restrict__ D, const uint32_t *__restrict__ cntg, int Z, uint32_t scap,
                                                              uint32_t idbits, uint32_t zpg, uint32_t n, uint32_t *__restrict__ paths_t)
{
    const int z = blockIdx.x;
    const int tid = threadIdx.x;
    const uint32_t g = static_cast<uint32_t>(tid) >> 3, j = static_cast<uint32_t>(tid) & 7u;
    D += (static_cast<size_t>(z) * kRunsPerZone + g) * scap;  // (scap is a multiple of 32 words: every run starts on a 128-byte line)
    // the run's length and the lane's first pieces are requested together, as run_open does: a run is scap >= 64 words
    // whatever its length, so the loads of the first pass are in bounds (what lies behind the run's end is masked below)
    const uint32_t len_raw = cntg[static_cast<size_t>(z) * kRunsPerZone + g];
    runs_u32x4 q[kRunsQuads];
#pragma unroll
    for (int u = 0; u < kRunsQuads; ++u) {
        const uint32_t k = min((j + 8u * u) * 4u, scap - 4u);
        q[u] = *reinterpret_cast<const runs_u32x4 *>(D + k);
    }
    const uint32_t len = min(len_raw, scap);  // (a run that outgrew scap has raised the status word: the attempt is discarded)
    const uint32_t idmask = (idbits >= 32) ? 0xFFFFFFFFu : ((1u << idbits) - 1u);
    const uint32_t gbase = g * zpg;
    // a pass: the lane's 16 entries -> 16 stores issued back to back
    auto pass = [&](uint32_t k0) {
        uint32_t id[4 * kRunsQuads], w[4 * kRunsQuads];
        bool ok[4 * kRunsQuads];
#pragma unroll
        for (int u = 0; u < kRunsQuads; ++u) {
            const uint32_t e[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const int s = 4 * u + x;
                const uint32_t at = k0 + (j + 8u * u) * 4u + x;  // (at or behind the run's end where the load was clamped: masked)
                const uint32_t dest = gbase + (e[x] >> idbits);
                id[s] = e[x] & idmask;
                w[s] = dest | kDriveBit;
                // entries of an overflowed attempt may be anything: nothing is stored out of range
                ok[s] = at < len && id[s] < n && dest < static_cast<uint32_t>(Z);
            }
        }
#pragma unroll
        for (int s = 0; s < 4 * kRunsQuads; ++s)
            if (ok[s]) paths_t[id[s]] = w[s];
    };
    pass(0u);
    // runs longer than a pass (popular destination groups): the same again
    for (uint32_t k0 = 32u * kRunsQuads; k0 < len; k0 += 32u * kRunsQuads) {
#pragma unroll
        for (int u = 0; u < kRunsQuads; ++u) {
            const uint32_t k = min(k0 + (j + 8u * u) * 4u, scap - 4u);
            q[u] = *reinterpret_cast<const runs_u32x4 *>(D + k);
        }
        pass(k0);
    }
}

// hour t of the grouped family, from the runs at D / cntg: the carry, then the scatter behind it on the stream
inline int32_t paths_launch_grouped(hipStream_t stream, const uint32_t *D, const uint32_t *cntg, int Z, uint32_t scap, uint32_t idbits, uint32_t zpg, int t,
                                    int64_t n, const uint32_t *zone0, const PathsDest &pd, std::string &err)
{
    uint32_t *row = pd.paths + static_cast<size_t>(t) * n;
    const uint32_t *prev = t == 0 ? zone0 : row - n;
    const int64_t pieces = (n + 3) / 4 + 1;  // (the row may straddle one piece more than its words fill)
    launch(k_paths_carry, dim3(static_cast<unsigned>((pieces + 255) / 256)), dim3(256), 0, stream, prev, row, static_cast<uint32_t>(n));
    launch(k_grouped_paths, dim3(static_cast<unsigned>(Z)), dim3(kRunsBlock), 0, stream, D, cntg, Z, scap, idbits, zpg, static_cast<uint32_t>(n), row);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        err = std::string("paths of the hour: ") + hipGetErrorString(e);
        return CPM_ERR_HIP;
    }
    return CPM_OK;
}

// CPM_KERNEL_ZONE_LDS: one thread per slot of ONE hour.  rec_t[i] = destination | drive flag << 31 of slot i (a car that stayed: its
// own zone), the slot's car is ids[i] (the exact layout, bucket by bucket): the access pattern of k_stays_cars, without its search.
__global__ __launch_bounds__(256) void k_paths_slots(const uint32_t *__restrict__ ids, const uint32_t *__restrict__ rec_t, int64_t n, uint32_t *__restrict__ paths_t)
{
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t car = ids[i];
    if (car < static_cast<uint64_t>(n)) paths_t[car] = rec_t[i];
}

inline hipError_t paths_launch_slots(hipStream_t stream, const uint32_t *ids, const uint32_t *rec_t, int64_t n, int t, const PathsDest &pd)
{
    launch(k_paths_slots, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, stream, ids, rec_t, n, pd.paths + static_cast<size_t>(t) * n);
    return hipGetLastError();
}

}  // namespace cpm
