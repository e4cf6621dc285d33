// cpm_runs.h -- what the side outputs of a resample share (cpm_flows.h, cpm_flows_csr.h, cpm_stays.h, cpm_paths.h, cpm_charge.h): where they go
// (SideDest), the one reader of the drivers' runs, and the helpers their kernels have in common.
// The grouped family's drivers of an hour sit in the 32 runs of their origin zone as id | local destination << idbits (cpm_grouped.h:
// Dq / cntg): run g of zone z is the scap words at D + (z * 32 + g) * scap, its length cntg[z * 32 + g].  A block of 256 threads reads
// the runs of ONE zone, 8 lanes per run, 128 entries of a run per pass:
//   run_open   asks for the run's length and the lane's pieces of the first pass together;
//   (the kernel zeroes its LDS and synchronises while those loads fly)
//   run_walk   clamps the length and hands every pass to the kernel's own body, which takes it entry by entry (run_entries).
// The clamps and the mask live here and nowhere else: they are what keeps an overflowed attempt from reading or storing out of range.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <atomic>
#include <mutex>

#include "../../include/cpm.h"
#include "cpm_kernels.h"

namespace cpm {

// Where the flows of a step go: nowhere, the dense tensor (cpm_flows.h), or CSR arrays (cpm_flows_csr.h).
struct FlowsDest {
    int32_t *dense = nullptr;    // DEVICE int32[T][Z][Z]
    int64_t *row_ptr = nullptr;  // DEVICE int64[T * Z + 1]: the CSR form
    int32_t *dest = nullptr;     // DEVICE int32[cap]
    int32_t *count = nullptr;    // DEVICE int32[cap]
    int64_t cap = 0;             // entries dest / count hold: nothing is stored at or behind it
    int32_t *hour_block = nullptr;  // DEVICE int32[Z * Z + 4], scratch of the per-car families (one hour's dense block)
    bool csr() const { return row_ptr != nullptr; }
    bool any() const { return dense != nullptr || row_ptr != nullptr; }
};

// where the stays of a step go (cpm_stays.h): nowhere, or DEVICE int32[T][Z][T] + int32[Z][T], with the side array of the context
struct StaysDest {
    int32_t *stays = nullptr;
    int32_t *parked = nullptr;
    uint32_t *last = nullptr;  // DEVICE uint32[n], zeroed by the caller at the start of the attempt
    bool any() const { return stays != nullptr; }
};

// where the record of a step goes (cpm_paths.h): nowhere, or DEVICE uint32[T][n]
struct PathsDest {
    uint32_t *paths = nullptr;
    bool any() const { return paths != nullptr; }
};

// where the charge of a step goes (cpm_charge.h): nowhere, or DEVICE int64[Z][T] x 2 + int32[Z][T] (+ uint32[n]), with the parameters
// of include/cpm_charge.h (arrays on the DEVICE), the side array of the context and its distance matrix
struct ChargeDest {
    int64_t *charge = nullptr;
    int64_t *used = nullptr;
    int32_t *shrt = nullptr;
    uint32_t *soc = nullptr;                // or null
    uint2 *ebat = nullptr;                  // DEVICE uint2[n], filled by k_charge_init at the start of the attempt
    const double *dist = nullptr;           // DEVICE f64[Z][Z], the context's origin-major copy of the distance matrix: dist[o * Z + d]
    const uint32_t *zone_power = nullptr;   // DEVICE uint32[Z] or null: `power` everywhere
    const uint32_t *soc_in = nullptr;       // DEVICE uint32[n] or null: `initial` for every car
    uint32_t capacity = 0, power = 0, initial = 0;
    double wh_per_km = 0.0;
    bool any() const { return charge != nullptr; }
};

// every side output of one step
struct SideDest {
    FlowsDest flows;
    StaysDest stays;
    PathsDest paths;
    ChargeDest charge;
    bool any() const { return flows.any() || stays.any() || paths.any() || charge.any(); }
};

constexpr int kRunsPerZone = 32;   // runs per origin zone (= kGroups of cpm_grouped.h, asserted in grouped_run)
constexpr int kRunsBlock = 256;    // 8 lanes per run
constexpr int kRunsQuads = 4;      // 16-byte loads a lane has in flight per pass over its run
constexpr uint32_t kRunsPass = 8u * 4u * kRunsQuads;  // entries of a run per pass
typedef uint32_t runs_u32x4 __attribute__((ext_vector_type(4)));

// a lane's view of its run
struct RunLane {
    const uint32_t *D;         // the run
    uint32_t len_raw, scap;    // its length as counted (an overflowed attempt: beyond scap), its words
    uint32_t g, j;             // the run of the zone, the lane of the run
    runs_u32x4 q[kRunsQuads];  // the pieces in flight: piece u holds entries k0 + (j + 8 * u) * 4 + 0 .. 3 of the pass at k0
};

// the lane's pieces of the pass at k0 (a load that would pass the run's last piece is clamped to it: run_entries masks what it brings)
__device__ __forceinline__ void run_load(RunLane &r, uint32_t k0)
{
#pragma unroll
    for (int u = 0; u < kRunsQuads; ++u) {
        const uint32_t k = min(k0 + (r.j + 8u * u) * 4u, r.scap - 4u);
        r.q[u] = *reinterpret_cast<const runs_u32x4 *>(r.D + k);
    }
}

// Zone blockIdx.x of the runs at D + d_off, their lengths at cntg + c_off (the hour's offsets in a grid over the kept runs of several
// hours; 0 in a kernel of one hour).  The length and the first pass are requested together: a run is scap >= 64 words whatever its
// length (and a multiple of 32: every run starts on a 128-byte line), so those loads are in bounds before the length is known.
__device__ __forceinline__ RunLane run_open(const uint32_t *__restrict__ D, const uint32_t *__restrict__ cntg, uint32_t scap, size_t d_off, size_t c_off)
{
    RunLane r;
    r.g = static_cast<uint32_t>(threadIdx.x) >> 3;
    r.j = static_cast<uint32_t>(threadIdx.x) & 7u;
    r.scap = scap;
    r.D = D + d_off + (static_cast<size_t>(blockIdx.x) * kRunsPerZone + r.g) * scap;
    r.len_raw = cntg[c_off + static_cast<size_t>(blockIdx.x) * kRunsPerZone + r.g];
    run_load(r, 0u);
    return r;
}

// pass(k0, len) for the pass in flight and, reloading, for every further pass of a run longer than one (popular destination groups)
template <typename F>
__device__ __forceinline__ void run_walk(RunLane &r, F &&pass)
{
    const uint32_t len = min(r.len_raw, r.scap);  // (a run that outgrew scap has raised the status word: the attempt is discarded)
    pass(0u, len);
    for (uint32_t k0 = kRunsPass; k0 < len; k0 += kRunsPass) {
        run_load(r, k0);
        pass(k0, len);
    }
}

// The lane's 16 entries of the pass at k0: f(s, entry, live), s = 0 .. 15 (a constant once unrolled).  !live: the entry lies at or
// behind the run's end (where the load was clamped, too) and must be ignored.  An entry of an overflowed attempt may hold anything: the
// kernel checks what it takes from one (an id, a destination) against its own bounds.
template <typename F>
__device__ __forceinline__ void run_entries(const RunLane &r, uint32_t k0, uint32_t len, F &&f)
{
#pragma unroll
    for (int u = 0; u < kRunsQuads; ++u) {
        const uint32_t e[4] = {r.q[u].x, r.q[u].y, r.q[u].z, r.q[u].w};
#pragma unroll
        for (int x = 0; x < 4; ++x) f(4 * u + x, e[x], k0 + (r.j + 8u * u) * 4u + x < len);
    }
}

// A row of `words` words, 4-byte aligned, stored by the whole block (kRunsBlock threads) from pieces on the row's 16-byte grid: the
// grid starts shift = row_shift(row) words in front of the row.  piece(i, shift) yields the four words of piece i of that grid: its
// word x is the row's word 4 * i + x - shift (what it yields for a word outside the row is not stored).  16-byte stores, consecutive lanes on consecutive addresses, where a piece lies wholly inside the row;
// single words for the pieces its two ends share with its neighbours.
__device__ __forceinline__ uint32_t row_shift(const void *row) { return static_cast<uint32_t>(reinterpret_cast<uintptr_t>(row) >> 2) & 3u; }

template <typename F>
__device__ __forceinline__ void row_store_shifted(int32_t *row, uint32_t words, F &&piece)
{
    const uint32_t shift = row_shift(row);
    int32_t *row16 = row - shift;
    const uint32_t end = words + shift;
    const uint32_t nquad = (end + 3u) / 4u;
    for (uint32_t i = threadIdx.x; i < nquad; i += kRunsBlock) {
        const uint32_t w0 = 4u * i;
        const runs_u32x4 v = piece(i, shift);
        if (w0 >= shift && w0 + 4u <= end) {
            *reinterpret_cast<runs_u32x4 *>(row16 + w0) = v;
        } else {
            if (w0 >= shift && w0 < end) row16[w0] = static_cast<int32_t>(v.x);
            if (w0 + 1u >= shift && w0 + 1u < end) row16[w0 + 1u] = static_cast<int32_t>(v.y);
            if (w0 + 2u >= shift && w0 + 2u < end) row16[w0 + 2u] = static_cast<int32_t>(v.z);
            if (w0 + 3u >= shift && w0 + 3u < end) row16[w0 + 3u] = static_cast<int32_t>(v.w);
        }
    }
}

// The per-car families' exact layout lies bucket by bucket: slot i belongs to the bucket z with off[z] <= i < off[z + 1].
__device__ __forceinline__ uint32_t slot_bucket(const uint32_t *__restrict__ off, int Z, uint32_t i)
{
    uint32_t lo = 0, hi = static_cast<uint32_t>(Z);  // off[lo] <= i < off[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Dynamic LDS above 48 KiB is asked for by name, once per kernel and device (and again for more), and the answer is read: a launch
// that was not granted its LDS comes back "invalid argument" hours later in the stream (what an unchecked one cost
// cpm_exact.h).  lds_opt_in<kernel>(used, ask) in front of a launch with `used` bytes of dynamic LDS: nothing below 48 KiB; above,
// one hipGetDevice and a load of what this kernel was granted on that device -- the state is the instantiation's own, so any
// number of kernels is held -- and only where that is less than max(used, ask) the library's one call that sets the attribute (lds_grant), under
// a mutex (the asking and the bookkeeping of all kernels are serialised, as they always were; the reader takes no lock).
constexpr int kLdsDevices = 64;  // (a device beyond: asked for at every launch, which is correct and merely slower)
inline hipError_t lds_grant(const void *kernel, std::atomic<size_t> *granted, size_t bytes)
{
    static std::mutex guard;
    std::lock_guard<std::mutex> lock(guard);
    if (granted && granted->load(std::memory_order_relaxed) >= bytes) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes));
    if (e == hipSuccess && granted) granted->store(bytes, std::memory_order_release);
    return e;
}
template <auto Kernel>
inline hipError_t lds_opt_in(size_t used, size_t ask = 0)
{
    if (used <= 48 * 1024) return hipSuccess;
    static std::atomic<size_t> granted[kLdsDevices] = {};
    int dev = 0;
    const hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::atomic<size_t> *g = dev >= 0 && dev < kLdsDevices ? &granted[dev] : nullptr;
    const size_t bytes = used > ask ? used : ask;
    if (g && g->load(std::memory_order_acquire) >= bytes) return hipSuccess;
    return lds_grant(reinterpret_cast<const void *>(Kernel), g, bytes);
}

}  // namespace cpm
