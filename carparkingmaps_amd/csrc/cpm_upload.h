// cpm_upload.h -- sparse row packs for a p_destin the HOST hands over (cpm_set_p_dest with CPM_OPT_SPARSE_UPLOAD).
//
// cpm_dataset.h builds sparse packs from a datamatrix's compact rows; a table that arrives as the dense array p[t][d][o] -- one the
// user edited, loaded from a file or built with the reference's own createpdestin -- is 91 % zeros all the same at Uber Movement's
// density (README.md:302-310).  Two kernels bring it into the very form k_ds_pdest leaves behind, so that everything downstream (the
// SPARSE samplers, search_exact_sparse, the batched resample, largest-first dealing) is the code that runs on dataset-built tables:
//   * k_up_compact : the dense array -> the table-owned compact rows sp / sj / scnt (value, destination, cells per row), the
//                    validation of every entry (D2) and the longest row;
//   * k_up_pack    : per row the reference's running sum over the kept cells in destination order (src/resampling.jl:39; the zeros
//                    in between add nothing: x + 0.0 == x, so every value equals k_build_rows' on the dense row, bit for bit), the
//                    row total and the sparse pack as k_ds_pdest lays it out.  It is that kernel from its third phase on: the
//                    uploaded values ARE the probabilities -- no weights, no row sum, no division (rows that sum to less or more
//                    than 1 keep D1's behaviour).  Also what cpm_refresh_tables re-runs on such tables.
// The host reads the longest row between the two (the pack's geometry needs it, as in ensure_dataset) and keeps the dense packs of
// k_build_rows when a row outgrew kDsCap or the sparse pack of the longest row is above 60 % of the dense one.  Nothing here depends
// on T (k_ds_cells holds 24 means in registers: ds_fits' T == 24 is that kernel's), and no address is a 32-bit offset into a whole
// table: the loads move a two-tile window along the row as k_build_rows does, the stores use 64-bit pointers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cpm_dataset.h"
#include "cpm_grouped.h"

namespace cpm {

constexpr int kUpHalf = 32;  // loads a lane keeps in flight behind the half tile it is looking at (as row_sums)

// Lane = origin (the array's fastest index: every load a whole 512-B line), block = one wave = 64 origins of one hour, walking the
// destinations in ascending order: a lane owns its row, so its cells come out in destination order from a private counter -- no
// tickets, no sort.  An entry is kept when p != 0.0 (-0.0 goes too: x + (-0.0) == x, no sum changes; NaN stays and is flagged).  The
// cap+1-th cell of a row is counted, never stored.  stats[0] = longest row (counted, not clamped), stats[1] = 1 when a row outgrew cap:
// reduced in the wave, and lane 0 looks at the word before it issues an atomic (k_ds_cells: an atomicMax per wave on one address was
// 1.05 of that kernel's 1.2 ms).
__global__ __launch_bounds__(64) void k_up_compact(const double *__restrict__ p, double *__restrict__ sp, uint32_t *__restrict__ sj, uint32_t *__restrict__ scnt,
                                                   int Z, uint32_t cap, uint32_t *__restrict__ stats, int *err)
{
    constexpr int H = kUpHalf;
    const int t = blockIdx.y;
    const int o0 = blockIdx.x * 64;
    const int lane = threadIdx.x;
    const int o = o0 + lane;
    const bool live = o < Z;
    const size_t Zs = static_cast<size_t>(Z);
    const double *src = p + static_cast<size_t>(t) * Zs * Zs + o0;  // (wave-uniform: a load is window base + scalar row offset + the lane's 8 bytes)
    const uint32_t lane_off = static_cast<uint32_t>(live ? lane : 0) << 3;  // (lanes past the table read the tile's first origin: in range, unused)
    const uint32_t rowb = static_cast<uint32_t>(Z) * 8u;                    // bytes between consecutive destinations of one origin
    const size_t row = static_cast<size_t>(t) * Zs + (live ? o : 0);
    double *spr = sp + row * cap;
    uint32_t *sjr = sj + row * cap;
    auto window = [&](int d0) {  // (a window of 2 H destinations: 64 x Z x 8 B < 2^32 for every Z a pack fits)
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(src + static_cast<size_t>(d0) * Zs), 0, static_cast<int>(2 * H * rowb), 0x00020000);
    };
    // (destinations past the row's end are clamped to its last one and their values unused: every load is inside the hour's slab)
    auto loads = [&](double(&x)[H], __amdgpu_buffer_rsrc_t rows, int d0, int d_first) {
#pragma unroll
        for (int u = 0; u < H; ++u) x[u] = row_load(rows, lane_off, static_cast<uint32_t>(min(d_first + u, Z - 1) - d0) * rowb);
    };
    uint32_t n = 0;
    bool bad = false;
    auto keep = [&](const double(&x)[H], int d_first) {
#pragma unroll
        for (int u = 0; u < H; ++u) {
            const int d = d_first + u;
            if (d < Z) {  // (wave-uniform)
                bad |= !(x[u] >= 0.0);
                if (live && x[u] != 0.0) {
                    if (n < cap) {
                        spr[n] = x[u];
                        sjr[n] = static_cast<uint32_t>(d);
                    }
                    ++n;
                }
            }
        }
    };
    double xa[H], xb[H];
    loads(xa, window(0), 0, 0);
#pragma unroll 1
    for (int d0 = 0; d0 < Z; d0 += 2 * H) {  // one half tile of loads always in flight behind the one being looked at
        const __amdgpu_buffer_rsrc_t rows = window(d0);
        loads(xb, rows, d0, d0 + H);
        keep(xa, d0);
        if (d0 + 2 * H < Z) loads(xa, window(d0 + 2 * H), d0 + 2 * H, d0 + 2 * H);
        keep(xb, d0 + H);
    }
    if (live) scnt[row] = min(n, cap);
    if (ballot64(bad && live) != 0 && lane == 0) atomicOr(err, 1);  // NaN or negative entries: CPM_ERR_TABLE
    uint32_t longest = n;
    for (int s = 32; s > 0; s >>= 1) longest = max(longest, static_cast<uint32_t>(__shfl_down(longest, s, 64)));
    if (lane == 0 && longest > __hip_atomic_load(&stats[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
        atomicMax(&stats[0], longest);
        if (longest > cap) atomicOr(&stats[1], 1u);
    }
}

// Running sum, row total and sparse pack of one (hour, origin) from its compact row: k_ds_pdest's layout (cpm_dataset.h) -- guide over
// entries, hi[e], padding with the row's last value up to nc and 0xFFFFFFFF behind it, the u16 map.  One wave per row, four rows per block.
__global__ __launch_bounds__(kDsThreads * kDsRows) void k_up_pack(const double *__restrict__ sp, const uint32_t *__restrict__ sj, const uint32_t *__restrict__ scnt,
                                                                  uint32_t cap, int64_t rows, int nc, int Zq_c, int G_c, uint32_t *__restrict__ rp,
                                                                  double *__restrict__ last_out)
{
    __shared__ double w_all[kDsRows][kDsCap];  // the row's values, then their running sum
    __shared__ uint32_t hi_all[kDsRows][kDsCap + 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double *w = w_all[wave];
    uint32_t *hi = hi_all[wave];
    const size_t row = static_cast<size_t>(blockIdx.x) * kDsRows + wave;
    const bool live = row < static_cast<size_t>(rows);
    const uint32_t n = live ? min(min(scnt[row], cap), kDsCap) : 0u;
    const double *gp = sp + (live ? row : 0) * cap;
    const uint32_t *gj = sj + (live ? row : 0) * cap;
    for (uint32_t e = lane; e < n; e += 64) w[e] = gp[e];
    __syncthreads();
    if (lane == 0 && live) {  // range_up = range_up + distribution[j] (src/resampling.jl:39)
        double run = 0.0;
        ds_seq_walk(n, w, [&](uint32_t e, double v) {
            run = run + v;
            w[e] = run;
        });
        last_out[row] = run;
    }
    __syncthreads();
    uint32_t *pack = rp + (live ? row : 0) * static_cast<size_t>(sparse_pack_words(Zq_c, G_c));
    const int gw = pack_guide_words(G_c);
    uint32_t *hi_g = pack + gw;
    uint16_t *idx_g = reinterpret_cast<uint16_t *>(hi_g + Zq_c);
    const uint32_t v_last = n ? ((w[n - 1] < 1.0) ? static_cast<uint32_t>(floor(w[n - 1] * 0x1.0p32)) : kHiMax) : kHiMax;
    const uint32_t j_last = n ? gj[n - 1] : 0u;
    for (int e = lane; e < Zq_c; e += 64) {
        uint32_t h = kHiMax;
        if (e < static_cast<int>(n)) h = (w[e] < 1.0) ? static_cast<uint32_t>(floor(w[e] * 0x1.0p32)) : kHiMax;
        else if (e < nc) h = v_last;
        if (e < static_cast<int>(kDsCap) + 64) hi[e] = h;
        if (live) {
            hi_g[e] = h;
            idx_g[e] = static_cast<uint16_t>(e < static_cast<int>(n) ? gj[e] : j_last);
        }
    }
    __syncthreads();
    // guide[m] = min(first e with hi[e] >= m << sh, nc - 1), m = 0 .. 2^G + 7 (the pad entries behind 2^G hold nc - 1)
    const int sh = 32 - G_c;
    uint16_t *guide = reinterpret_cast<uint16_t *>(pack);
    if (live)
        for (int m = lane; m < (1 << G_c) + 8; m += 64) {
            const unsigned long long key = static_cast<unsigned long long>(m) << sh;
            int lo = 0, len = nc;  // first e in [0, nc) with hi[e] >= key
            while (len > 0) {
                const int half = len >> 1;
                if (static_cast<unsigned long long>(hi[lo + half]) < key) {
                    lo += half + 1;
                    len -= half + 1;
                } else {
                    len = half;
                }
            }
            guide[m] = static_cast<uint16_t>(min(lo, nc - 1));
        }
}

}  // namespace cpm
