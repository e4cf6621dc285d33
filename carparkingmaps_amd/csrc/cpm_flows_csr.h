// cpm_flows_csr.h -- the hourly origin-destination trip counts of a resample as compressed sparse rows (include/cpm_flows_csr.h): the
// non-zero cells of flows[t][o][d] (cpm_flows.h), row r = t * Z + o, destinations ascending.  Nothing here touches a kernel of
// cpm_flows.h: the grouped family's rows come from the drivers' runs, through the reader of cpm_runs.h, by three launches
//   k_flows_csr_count   the row's histogram in LDS, its non-zero bins counted              -> row_ptr[r + 1] = nnz of row r
//   k_flows_csr_scan    one block: prefix of those in (t, o) order                         -> row_ptr[r + 1] = end of row r
//   k_flows_csr_fill    the histogram again, its non-zero bins compacted in LDS            -> dest / count [row_ptr[r] ..)
// behind an hour's launches (grid (Z, 1); the hour's base is the previous hour's end, which stream order has put in row_ptr) or once
// over the kept runs (grid (Z, T)).  Where a row lands is a function of the counts alone: no atomic touches the output.
// The other two families build an hour's dense Z x Z block with k_flows_cars and take it apart the same way (k_flows_csr_from_dense).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "cpm_flows.h"

namespace cpm {

constexpr int kCsrWaves = kRunsBlock / 64;  // (every row kernel here runs blocks of kRunsBlock threads, whether it reads runs or not)
constexpr int kCsrScanBlock = 1024;
constexpr int kCsrScanItems = 4;    // consecutive rows per thread and tile

// LDS: the histogram (as k_grouped_flows', three words of slack for a dense row off a 16-byte boundary); the fill adds the row's
// compacted destinations, shifted by up to three words so that LDS and output addresses agree modulo 16 bytes
__host__ __device__ inline uint32_t flows_csr_quads(int Z) { return (static_cast<uint32_t>(Z) + 3u + 3u) / 4u; }  // (16-byte pieces of one array: flows_lds_bytes(Z) / 16)
inline size_t flows_csr_lds_bytes(int Z, bool fill) { return static_cast<size_t>(flows_csr_quads(Z)) * 16 * (fill ? 2 : 1); }

// The tail of every row kernel.  bins[0 .. Z) is the row's histogram (LDS, complete: the caller has synchronised).
// !FILL: the number of non-zero bins -> *nnz_out.  FILL: (d, bins[d]) of the non-zero bins, d ascending -> dest / count [start ..),
// below cap.  Each wave takes a contiguous range of bins: a ballot per 64 bins, ranks by popcount, one sum across the waves.
template <bool FILL>
__device__ __forceinline__ void flows_csr_row_tail(const uint32_t *bins, uint32_t *stage, uint32_t Z, int64_t *nnz_out, int64_t start, int32_t *__restrict__ dest,
                                                   int32_t *__restrict__ count, int64_t cap)
{
    __shared__ uint32_t wave_nnz[kCsrWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t per = (Z + 64u * kCsrWaves - 1u) / (64u * kCsrWaves) * 64u;
    const uint32_t lo = min(wave * per, Z), hi = min(lo + per, Z);
    uint32_t mine = 0;
    for (uint32_t b = lo; b < hi; b += 64u) {
        const uint32_t i = b + lane;
        mine += static_cast<uint32_t>(__popcll(__ballot(i < hi && bins[i] != 0u)));
    }
    if (lane == 0) wave_nnz[wave] = mine;
    __syncthreads();
    uint32_t below = 0, nnz = 0;
#pragma unroll
    for (uint32_t w = 0; w < kCsrWaves; ++w) {
        const uint32_t v = wave_nnz[w];
        below += w < wave ? v : 0u;
        nnz += v;
    }
    if constexpr (!FILL) {
        if (tid == 0) *nnz_out = static_cast<int64_t>(nnz);
    } else {
        if (start >= cap || nnz == 0u) return;  // (the whole block alike)
        const uint32_t m = static_cast<uint32_t>(min(static_cast<int64_t>(nnz), cap - start));  // entries of this row below cap
        int32_t *drow = dest + start, *crow = count + start;
        const uint32_t shift = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(drow) >> 2) & 3u;
        const bool count_wide = (static_cast<uint32_t>(reinterpret_cast<uintptr_t>(crow) >> 2) & 3u) == shift;
        uint32_t at = shift + below;
        for (uint32_t b = lo; b < hi; b += 64u) {
            const uint32_t i = b + lane;
            const bool nz = i < hi && bins[i] != 0u;
            const unsigned long long mask = __ballot(nz);
            if (nz) stage[at + static_cast<uint32_t>(__popcll(mask & ((1ull << lane) - 1ull)))] = i;
            at += static_cast<uint32_t>(__popcll(mask));
        }
        __syncthreads();
        // the row: 16-byte stores, consecutive lanes on consecutive addresses; single words where its two ends share a piece with
        // their neighbours (and for the counts of a caller whose two arrays are aligned differently)
        const uint32_t end = shift + m;
        const uint32_t nquad = (end + 3u) / 4u;
        const runs_u32x4 *stage4 = reinterpret_cast<const runs_u32x4 *>(stage);
        int32_t *d16 = drow - shift, *c16 = crow - shift;
        for (uint32_t i = tid; i < nquad; i += kRunsBlock) {
            const uint32_t w0 = 4u * i;
            runs_u32x4 d = stage4[i], c;  // (words outside [shift, shift + nnz) are zero: a valid bin)
            c.x = bins[min(d.x, Z - 1u)];
            c.y = bins[min(d.y, Z - 1u)];
            c.z = bins[min(d.z, Z - 1u)];
            c.w = bins[min(d.w, Z - 1u)];
            const bool whole = w0 >= shift && w0 + 4u <= end;
            if (whole) *reinterpret_cast<runs_u32x4 *>(d16 + w0) = d;
            if (whole && count_wide) {
                *reinterpret_cast<runs_u32x4 *>(c16 + w0) = c;
            } else {
                const uint32_t dv[4] = {d.x, d.y, d.z, d.w}, cv[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k) {
                    if (w0 + k >= shift && w0 + k < end) {
                        if (!whole) d16[w0 + k] = static_cast<int32_t>(dv[k]);
                        c16[w0 + k] = static_cast<int32_t>(cv[k]);
                    }
                }
            }
        }
    }
}

// One block per (origin zone, hour), the arguments and the two grids of k_grouped_flows.  row_ptr is that of the launch's first hour:
// row_ptr[r], r = blockIdx.y * Z + zone.
template <bool FILL>
__device__ __forceinline__ void flows_csr_grouped(const uint32_t *__restrict__ D, const uint32_t *__restrict__ cntg, int Z, uint32_t scap, uint32_t idbits, uint32_t zpg,
                                                  size_t d_stride, size_t c_stride, int64_t *__restrict__ row_ptr, int32_t *__restrict__ dest,
                                                  int32_t *__restrict__ count, int64_t cap)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t csr_lds[];
    RunLane r = run_open(D, cntg, scap, d_stride * blockIdx.y, c_stride * blockIdx.y);
    int64_t *rp = row_ptr + static_cast<size_t>(blockIdx.y) * Z + blockIdx.x;
    int64_t start = 0;
    if constexpr (FILL) start = rp[0];
    const uint32_t nquad = flows_csr_quads(Z) * (FILL ? 2u : 1u);  // (histogram and, FILL, the staged row)
    runs_u32x4 *lds4 = reinterpret_cast<runs_u32x4 *>(csr_lds);
    for (uint32_t i = threadIdx.x; i < nquad; i += kRunsBlock) lds4[i] = runs_u32x4{0u, 0u, 0u, 0u};
    __syncthreads();
    const uint32_t gbase = r.g * zpg;
    run_walk(r, [&](uint32_t k0, uint32_t len) {
        run_entries(r, k0, len, [&](int, uint32_t entry, bool live) {
            const uint32_t b = gbase + (entry >> idbits);
            if (live && b < static_cast<uint32_t>(Z)) atomicAdd(&csr_lds[b], 1u);
        });
    });
    __syncthreads();
    flows_csr_row_tail<FILL>(csr_lds, csr_lds + 4u * flows_csr_quads(Z), static_cast<uint32_t>(Z), rp + 1, start, dest, count, cap);
}

__global__ __launch_bounds__(kRunsBlock) void k_flows_csr_count(const uint32_t *__restrict__ D, const uint32_t *__restrict__ cntg, int Z, uint32_t scap,
                                                               uint32_t idbits, uint32_t zpg, size_t d_stride, size_t c_stride, int64_t *__restrict__ row_ptr)
{
    flows_csr_grouped<false>(D, cntg, Z, scap, idbits, zpg, d_stride, c_stride, row_ptr, nullptr, nullptr, 0);
}

__global__ __launch_bounds__(kRunsBlock) void k_flows_csr_fill(const uint32_t *__restrict__ D, const uint32_t *__restrict__ cntg, int Z, uint32_t scap,
                                                              uint32_t idbits, uint32_t zpg, size_t d_stride, size_t c_stride, int64_t *__restrict__ row_ptr,
                                                              int32_t *__restrict__ dest, int32_t *__restrict__ count, int64_t cap)
{
    flows_csr_grouped<true>(D, cntg, Z, scap, idbits, zpg, d_stride, c_stride, row_ptr, dest, count, cap);
}

// One block.  On entry p[1 + i] is the nnz of row i (i < nrows) and, unless `first`, p[0] the end of the row before them; on exit
// p[1 + i] is the end of row i (p[0], first: 0).  Rows are taken in order, tile by tile: the result does not depend on any timing.
__global__ __launch_bounds__(kCsrScanBlock) void k_flows_csr_scan(int64_t *__restrict__ p, uint32_t nrows, int first)
{
    __shared__ int64_t wave_sum[kCsrScanBlock / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    int64_t base = first ? 0 : p[0];
    if (first && tid == 0) p[0] = 0;
    for (uint32_t tile = 0; tile < nrows; tile += kCsrScanBlock * kCsrScanItems) {
        const uint32_t i0 = tile + tid * kCsrScanItems;
        int64_t v[kCsrScanItems];
#pragma unroll
        for (uint32_t k = 0; k < kCsrScanItems; ++k) v[k] = i0 + k < nrows ? p[1u + i0 + k] : 0;
#pragma unroll
        for (uint32_t k = 1; k < kCsrScanItems; ++k) v[k] += v[k - 1];
        const int64_t own = v[kCsrScanItems - 1];
        int64_t x = own;  // -> inclusive over the wave
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const int64_t y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        if (lane == 63u) wave_sum[wave] = x;
        __syncthreads();
        int64_t below = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < kCsrScanBlock / 64; ++w) {
            const int64_t s = wave_sum[w];
            below += w < wave ? s : 0;
            total += s;
        }
        const int64_t before = base + below + x - own;
#pragma unroll
        for (uint32_t k = 0; k < kCsrScanItems; ++k)
            if (i0 + k < nrows) p[1u + i0 + k] = before + v[k];
        base += total;
        __syncthreads();
    }
}

// The per-car families: one block per row o of ONE hour's dense block (k_flows_cars' output, Z x Z, four words of slack behind it),
// read in 16-byte pieces into the LDS the grouped kernels build their histogram in.  row_ptr is the hour's: row_ptr[o].
template <bool FILL>
__global__ __launch_bounds__(kRunsBlock) void k_flows_csr_from_dense(const int32_t *__restrict__ block, int Z, int64_t *__restrict__ row_ptr,
                                                                    int32_t *__restrict__ dest, int32_t *__restrict__ count, int64_t cap)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t csr_lds[];
    const uint32_t o = blockIdx.x, tid = threadIdx.x;
    const size_t first = static_cast<size_t>(o) * Z;
    const uint32_t shift = static_cast<uint32_t>(first & 3u);  // (the block is 16-byte aligned: a row starts `shift` words into a piece)
    const runs_u32x4 *src4 = reinterpret_cast<const runs_u32x4 *>(block + (first - shift));
    const uint32_t nrow = (static_cast<uint32_t>(Z) + shift + 3u) / 4u;
    const uint32_t nquad = flows_csr_quads(Z);
    int64_t start = 0;
    if constexpr (FILL) start = row_ptr[o];
    runs_u32x4 *lds4 = reinterpret_cast<runs_u32x4 *>(csr_lds);
    for (uint32_t i = tid; i < nquad; i += kRunsBlock) lds4[i] = i < nrow ? src4[i] : runs_u32x4{0u, 0u, 0u, 0u};
    if constexpr (FILL)
        for (uint32_t i = tid; i < nquad; i += kRunsBlock) lds4[nquad + i] = runs_u32x4{0u, 0u, 0u, 0u};
    __syncthreads();
    flows_csr_row_tail<FILL>(csr_lds + shift, csr_lds + 4u * nquad, static_cast<uint32_t>(Z), row_ptr + o + 1, start, dest, count, cap);
}

inline int32_t flows_csr_check(int Z, const FlowsDest &fd, std::string &err)
{
    if (flows_csr_lds_bytes(Z, true) + 64 > 160 * 1024) {
        err = "flows (csr): a row of this many zones does not fit its histogram and its compacted form in LDS";
        return CPM_ERR_ARG;
    }
    if (fd.cap < 0 || (fd.cap > 0 && (!fd.dest || !fd.count))) {
        err = "flows (csr): entry arrays";
        return CPM_ERR_ARG;
    }
    return CPM_OK;
}

inline int32_t flows_csr_fail(hipError_t e, const char *what, std::string &err)
{
    err = std::string("flows (csr) ") + what + ": " + hipGetErrorString(e);
    return CPM_ERR_HIP;
}

// hours t0 .. t0 + nt - 1 from the runs at D / cntg, as flows_launch_grouped: count, scan, fill
inline int32_t flows_csr_launch_grouped(hipStream_t stream, const uint32_t *D, const uint32_t *cntg, int Z, uint32_t scap, uint32_t idbits, uint32_t zpg,
                                        size_t d_stride, size_t c_stride, int t0, int nt, const FlowsDest &fd, std::string &err)
{
    const int32_t rc = flows_csr_check(Z, fd, err);
    if (rc != CPM_OK) return rc;
    const size_t lds_c = flows_csr_lds_bytes(Z, false), lds_f = flows_csr_lds_bytes(Z, true);
    hipError_t e = lds_opt_in<k_flows_csr_count>(lds_c);
    if (e == hipSuccess) e = lds_opt_in<k_flows_csr_fill>(lds_f);
    if (e != hipSuccess) return flows_csr_fail(e, "LDS", err);
    int64_t *rp = fd.row_ptr + static_cast<size_t>(t0) * Z;
    const dim3 grid(static_cast<unsigned>(Z), static_cast<unsigned>(nt));
    launch(k_flows_csr_count, grid, dim3(kRunsBlock), lds_c, stream, D, cntg, Z, scap, idbits, zpg, d_stride, c_stride, rp);
    launch(k_flows_csr_scan, dim3(1), dim3(kCsrScanBlock), 0, stream, rp, static_cast<uint32_t>(nt) * static_cast<uint32_t>(Z), t0 == 0 ? 1 : 0);
    if (fd.cap > 0)
        launch(k_flows_csr_fill, grid, dim3(kRunsBlock), lds_f, stream, D, cntg, Z, scap, idbits, zpg, d_stride, c_stride, rp, fd.dest, fd.count, fd.cap);
    if ((e = hipGetLastError()) != hipSuccess) return flows_csr_fail(e, "launch", err);
    return CPM_OK;
}

// The flows of hour t from the per-car records (flows_launch_cars' arguments): into the dense tensor, or through the hour block into
// the CSR arrays.  The dense tensor was zeroed by the caller; the hour block is zeroed here, behind the hour before on the stream.
inline int32_t flows_hour_from_cars(hipStream_t stream, const FlowsDest &fd, const uint32_t *zsrc, const uint32_t *off, const uint32_t *rec_t, int64_t n,
                                    int Z, int t, std::string &err)
{
    hipError_t e;
    if (!fd.csr()) {
        if (!fd.dense) return CPM_OK;
        e = flows_launch_cars(stream, zsrc, off, rec_t, n, Z, fd.dense + static_cast<size_t>(t) * Z * Z);
        if (e != hipSuccess) return flows_csr_fail(e, "flows of the hour", err);
        return CPM_OK;
    }
    const int32_t rc = flows_csr_check(Z, fd, err);
    if (rc != CPM_OK) return rc;
    const size_t lds_c = flows_csr_lds_bytes(Z, false), lds_f = flows_csr_lds_bytes(Z, true);
    e = lds_opt_in<k_flows_csr_from_dense<false>>(lds_c);
    if (e == hipSuccess) e = lds_opt_in<k_flows_csr_from_dense<true>>(lds_f);
    if (e != hipSuccess) return flows_csr_fail(e, "LDS", err);
    if ((e = hipMemsetAsync(fd.hour_block, 0, sizeof(int32_t) * (static_cast<size_t>(Z) * Z + 4), stream)) != hipSuccess) return flows_csr_fail(e, "hour block", err);
    if ((e = flows_launch_cars(stream, zsrc, off, rec_t, n, Z, fd.hour_block)) != hipSuccess) return flows_csr_fail(e, "flows of the hour", err);
    int64_t *rp = fd.row_ptr + static_cast<size_t>(t) * Z;
    launch(k_flows_csr_from_dense<false>, dim3(static_cast<unsigned>(Z)), dim3(kRunsBlock), lds_c, stream, fd.hour_block, Z, rp, static_cast<int32_t *>(nullptr),
           static_cast<int32_t *>(nullptr), static_cast<int64_t>(0));
    launch(k_flows_csr_scan, dim3(1), dim3(kCsrScanBlock), 0, stream, rp, static_cast<uint32_t>(Z), t == 0 ? 1 : 0);
    if (fd.cap > 0) launch(k_flows_csr_from_dense<true>, dim3(static_cast<unsigned>(Z)), dim3(kRunsBlock), lds_f, stream, fd.hour_block, Z, rp, fd.dest, fd.count, fd.cap);
    if ((e = hipGetLastError()) != hipSuccess) return flows_csr_fail(e, "launch", err);
    return CPM_OK;
}

}  // namespace cpm
