// cpm_expected_sparse.h -- the expected densities from the compact rows of sparse p_destin tables (include/cpm_expected_sparse.h):
// k_exps_aux, k_exps_scan, k_exps_fill, k_exps_sort, k_exps_hour<NB>.
//
// k_exp_hour (cpm_expected.h) reads the hour's dense Z x Z block; of a sparse table most of it is zero.  A cell with p = 0 adds
// x * 0 = +0 to an accumulator that starts at +0 and only receives non-negative terms: it changes no bit.  So k_exps_hour visits only
// the STORED cells of a destination column, gives each to the lane k_exp_hour gives it to, adds a lane's cells in the same order and
// then runs the same code (exp_block_sum, the residual lists, the stay and the zero-row term): every word it writes carries the bits
// k_exp_hour writes.
//
// The lane rule (exp_stream, restated).  npairs = Z >> 1; head(t, d) = Z odd && (t * Z * Z + d * Z) odd = Z odd && (t + d) odd: the
// dense row of hour t, destination d starts 8 bytes behind a 16-byte line of the aligned d_p exactly then.
//   head = 0: origin o < 2 * npairs belongs to lane (o >> 1) & 255; for odd Z the last origin Z - 1 to lane 0, behind lane 0's pairs;
//   head = 1: origin o >= 1 belongs to lane ((o - 1) >> 1) & 255; origin 0 to lane 0, behind lane 0's pairs;
//   within a lane ascending origin, each term a = a + x[o] * p (two roundings: -ffp-contract=off).
// exps_key() packs (lane, place in the lane) into one word; the cells of a column are stored sorted by it.
//
// Per-table arrays, from d_sp / d_sj / d_scnt alone (the dense array is neither read nor built):
//   ell / r / start / list  -- word for word what k_exp_aux / k_exp_lists write (k_exps_aux, then k_exp_lists itself);
//   colptr [T][Z + 1]       -- where column (t, d) begins in the cell arrays (colptr[t][Z] = colptr[t + 1][0]);
//   cell_p (f64), cell_o (u32) -- the stored cells, column by column, each column sorted by exps_key.
// Count (integer atomics) + scan + fill (integer atomics: a column's cells in any order) + a rank sort per column: origins are unique
// within a column, so the sorted arrays are a function of the table.  No floating-point atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cpm_expected.h"

namespace cpm {

constexpr int kExpsLaneShift = 17;      // exps_key = lane << 17 | place: origins (and Z itself) lie below 2^17
constexpr int kExpsMaxZ = (1 << kExpsLaneShift) - 1;
constexpr uint32_t kExpsNoLane = 0xffffffffu;
constexpr int kExpsSortChunk = 2048;    // keys of a column in LDS at a time (k_exps_sort)

// head(t, d) for odd Z (see above); par = t & 1
__device__ __forceinline__ bool exps_head(bool odd, int par, int d) { return odd && (((par + d) & 1) != 0); }

__device__ __forceinline__ uint32_t exps_key(uint32_t o, uint32_t Z, bool head)
{
    if (!head) {
        if (o >= (Z & ~1u)) return Z;  // odd Z: origin Z - 1, thread 0's single word behind its pairs
        return (((o >> 1) & 255u) << kExpsLaneShift) | o;
    }
    if (o == 0) return Z;  // origin 0, likewise
    return ((((o - 1) >> 1) & 255u) << kExpsLaneShift) | o;
}

// ell, r and the row-total check of k_exp_aux from the compact rows, and the cells of every column counted.  One wave per row,
// grid = ds_grid(T * Z) blocks of kDsRows waves (as k_ds_dense_p).  A row's cells are sorted by destination, so the last cell with
// p > 0 is the one with the largest index (cells of weight 0 are kept by the dataset route: not simply the last cell).
// cnt: [T][Z + 1], zeroed by the caller.
__global__ __launch_bounds__(256) void k_exps_aux(const double *__restrict__ sp, const uint32_t *__restrict__ sj, const uint32_t *__restrict__ scnt,
                                                  uint32_t cap, int64_t rows, int Z, const double *__restrict__ last, int *__restrict__ ell,
                                                  double *__restrict__ r, unsigned long long *__restrict__ bad, uint32_t *__restrict__ cnt)
{
    const size_t row = static_cast<size_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (row >= static_cast<size_t>(rows)) return;
    const int lane = static_cast<int>(threadIdx.x & 63);
    const size_t t = row / static_cast<size_t>(Z);
    const uint32_t n = min(scnt[row], cap);
    const double tot = last[row];
    int e_last = -1;
    for (uint32_t e = lane; e < n; e += 64) {
        const uint32_t d = sj[row * cap + e];
        if (d < static_cast<uint32_t>(Z)) {
            atomicAdd(cnt + t * (Z + 1) + d, 1u);
            if (sp[row * cap + e] > 0.0) e_last = static_cast<int>(e);
        }
    }
    for (int o = 32; o > 0; o >>= 1) e_last = max(e_last, __shfl_xor(e_last, o, 64));
    if (lane != 0) return;
    const double res = 1.0 - tot;
    r[row] = res > 0.0 ? res : 0.0;
    int d = Z;
    if (tot != 0.0) {
        if (e_last >= 0) d = static_cast<int>(sj[row * cap + e_last]);
        if (tot > 1.0 + static_cast<double>(Z) * 0x1.0p-52) atomicMin(bad, static_cast<unsigned long long>(row));
    }
    ell[row] = d;
}

// colptr = the exclusive prefix sums of cnt over all n = T * (Z + 1) words (cnt[t][Z] = 0, so colptr[t][Z] = colptr[t + 1][0]), and
// *total = their sum.  One workgroup: a thread sums its strip of the array, the strips' sums are scanned in LDS, and the thread walks
// its strip again.
__global__ __launch_bounds__(kExpBlock) void k_exps_scan(const uint32_t *__restrict__ cnt, size_t n, uint32_t *__restrict__ colptr,
                                                         unsigned long long *__restrict__ total)
{
    __shared__ uint32_t s[kExpBlock];
    const int tid = static_cast<int>(threadIdx.x);
    const size_t per = (n + kExpBlock - 1) / kExpBlock;
    const size_t a = min(static_cast<size_t>(tid) * per, n), b = min(a + per, n);
    uint32_t sum = 0;
    for (size_t i = a; i < b; ++i) sum += cnt[i];
    s[tid] = sum;
    __syncthreads();
    for (int o = 1; o < kExpBlock; o <<= 1) {
        const uint32_t v = tid >= o ? s[tid - o] : 0u;
        __syncthreads();
        s[tid] += v;
        __syncthreads();
    }
    uint32_t run = s[tid] - sum;
    for (size_t i = a; i < b; ++i) {
        colptr[i] = run;
        run += cnt[i];
    }
    if (tid == kExpBlock - 1) *total = s[tid];
}

// every stored cell into its column, in the order the tickets come (cur: [T][Z + 1], zeroed by the caller).  One wave per row.
__global__ __launch_bounds__(256) void k_exps_fill(const double *__restrict__ sp, const uint32_t *__restrict__ sj, const uint32_t *__restrict__ scnt,
                                                   uint32_t cap, int64_t rows, int Z, const uint32_t *__restrict__ colptr, uint32_t *__restrict__ cur,
                                                   uint32_t *__restrict__ tmp_o, double *__restrict__ tmp_p)
{
    const size_t row = static_cast<size_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (row >= static_cast<size_t>(rows)) return;
    const size_t t = row / static_cast<size_t>(Z);
    const uint32_t o = static_cast<uint32_t>(row % static_cast<size_t>(Z));
    const uint32_t n = min(scnt[row], cap);
    for (uint32_t e = threadIdx.x & 63; e < n; e += 64) {
        const uint32_t d = sj[row * cap + e];
        if (d >= static_cast<uint32_t>(Z)) continue;
        const size_t col = t * (Z + 1) + d;
        const uint32_t a = colptr[col], len = colptr[col + 1] - a;
        const uint32_t k = atomicAdd(cur + col, 1u);
        if (k < len) {  // (always: k_exps_aux counted the same cells)
            tmp_o[a + k] = o;
            tmp_p[a + k] = sp[row * cap + e];
        }
    }
}

// A column's cells sorted by exps_key: cell i goes to the place given by the number of keys below its own (the keys of a column are
// distinct).  A column may hold all Z origins whatever the rows' capacity: the keys pass through LDS in chunks.  grid = (Z, T).
__global__ __launch_bounds__(kExpBlock) void k_exps_sort(const uint32_t *__restrict__ colptr, const uint32_t *__restrict__ tmp_o,
                                                         const double *__restrict__ tmp_p, int Z, uint32_t *__restrict__ cell_o,
                                                         double *__restrict__ cell_p)
{
    __shared__ uint32_t s_key[kExpsSortChunk];
    const int tid = static_cast<int>(threadIdx.x), d = static_cast<int>(blockIdx.x), t = static_cast<int>(blockIdx.y);
    const size_t col = static_cast<size_t>(t) * (Z + 1) + d;
    const uint32_t a = colptr[col], n = colptr[col + 1] - a;
    const bool head = exps_head((Z & 1) != 0, t & 1, d);
    for (uint32_t i0 = 0; i0 < n; i0 += kExpBlock) {  // (uniform over the workgroup)
        const uint32_t i = i0 + tid;
        const uint32_t o = i < n ? tmp_o[a + i] : 0u;
        const uint32_t mine = exps_key(o, static_cast<uint32_t>(Z), head);
        uint32_t rank = 0;
        for (uint32_t c0 = 0; c0 < n; c0 += kExpsSortChunk) {
            const uint32_t m = min(static_cast<uint32_t>(kExpsSortChunk), n - c0);
            __syncthreads();
            for (uint32_t j = tid; j < m; j += kExpBlock) s_key[j] = exps_key(tmp_o[a + c0 + j], static_cast<uint32_t>(Z), head);
            __syncthreads();
            for (uint32_t j = 0; j < m; ++j) rank += s_key[j] < mine ? 1u : 0u;
        }
        if (i < n && rank < n) {
            cell_o[a + rank] = o;
            cell_p[a + rank] = tmp_p[a + i];
        }
    }
}

// One hour for the nf <= NB fleets of a pass: k_exp_hour with the streamed part replaced.  grid = ceil(Z / kExpRows); thread L owns
// lane L's accumulators, one per (column, fleet).  Cell-parallel: of each of the workgroup's kExpRows columns, 256 cells at a time,
// thread i loads cell i (neighbouring threads read neighbouring cells; the first chunk of all four columns is requested up front),
// gathers x_f[o] from the aligned workspace through the L2 as k_exp_hour does, and leaves the rounded product x * p in LDS.  A
// column is sorted by (lane, place in the lane), so a lane's cells are a run of neighbours: the thread at a run's head adds the run
// IN ORDER onto the lane's accumulator in LDS -- a = a + x * p, from the accumulator's own value, so a run that continues in the next
// chunk continues the same sum -- and a barrier separates the chunks.  Behind a column's last chunk thread L takes lane L's word.
// (A search by thread L for its own segment of each column was measured first: 30.5 us per hour at Z = 2,357 against 16.1 us of
// k_exp_hour, a chain of dependent loads per workgroup; profiles/expected_sparse_notes.md.)
// colptr_t: the hour's [Z + 1] slice (offsets into the whole cell arrays); par = t & 1.  The cells are read once per hour:
// non-temporal.  Everything behind exp_block_sum is k_exp_hour's code.
template <int NB>
__global__ __launch_bounds__(kExpBlock) void k_exps_hour(const uint32_t *__restrict__ colptr_t, const uint32_t *__restrict__ cell_o,
                                                         const double *__restrict__ cell_p, int par, const double *__restrict__ last_t,
                                                         const double *__restrict__ r_t, const int *__restrict__ start_t, const int *__restrict__ list_t,
                                                         const double *__restrict__ q_cur, const double *__restrict__ q_next, size_t q_stride,
                                                         const double *__restrict__ pi_in, const double *__restrict__ x_in,
                                                         double *__restrict__ pi_out, double *__restrict__ x_out, double *__restrict__ park,
                                                         double *__restrict__ drv, size_t out_stride, int Z, int Zs, int nf)
{
    __shared__ double s_part[kExpWaves * kExpRows * NB];
    __shared__ double s_y[kExpRows * NB];
    __shared__ double s_res[kExpRows * NB];
    __shared__ double s_acc[NB][kExpBlock];   // the lanes' accumulators of the column in hand
    __shared__ double s_prod[NB][kExpBlock];  // the chunk's products
    __shared__ uint32_t s_lane[kExpBlock];    // ... and their lanes (kExpsNoLane: no cell)
    const int tid = static_cast<int>(threadIdx.x);
    const int d0 = static_cast<int>(blockIdx.x) * kExpRows;
    const bool odd = (Z & 1) != 0;
    const uint32_t uz = static_cast<uint32_t>(Z), utid = static_cast<uint32_t>(tid);

    const double *xf[NB];
#pragma unroll
    for (int f = 0; f < NB; ++f) xf[f] = x_in + static_cast<size_t>(f < nf ? f : nf - 1) * Zs;

    uint32_t ca[kExpRows], cn[kExpRows], o1[kExpRows];
    double p1[kExpRows];
#pragma unroll
    for (int r = 0; r < kExpRows; ++r) {
        const int d = d0 + r;
        uint32_t a = 0, b = 0;
        if (d < Z) {
            a = colptr_t[d];
            b = colptr_t[d + 1];
        }
        ca[r] = a;
        cn[r] = b - a;
    }
#pragma unroll
    for (int r = 0; r < kExpRows; ++r) {  // the first chunk of every column: all in flight together
        o1[r] = 0;
        p1[r] = 0.0;
        if (utid < cn[r]) {
            o1[r] = __builtin_nontemporal_load(cell_o + ca[r] + utid);
            p1[r] = __builtin_nontemporal_load(cell_p + ca[r] + utid);
        }
    }

    double acc[kExpRows * NB];
#pragma unroll
    for (int r = 0; r < kExpRows; ++r) {
        const bool hd = exps_head(odd, par, d0 + r);
#pragma unroll
        for (int f = 0; f < NB; ++f) s_acc[f][tid] = 0.0;
        for (uint32_t c = 0; c < cn[r]; c += kExpBlock) {  // (uniform over the workgroup)
            const uint32_t i = c + utid;
            const bool in = i < cn[r];
            uint32_t o = o1[r];
            double p = p1[r];
            if (c != 0) {
                o = 0;
                p = 0.0;
                if (in) {
                    o = __builtin_nontemporal_load(cell_o + ca[r] + i);
                    p = __builtin_nontemporal_load(cell_p + ca[r] + i);
                }
            }
            const uint32_t lane = in ? exps_key(o, uz, hd) >> kExpsLaneShift : kExpsNoLane;
            s_lane[tid] = lane;
#pragma unroll
            for (int f = 0; f < NB; ++f) s_prod[f][tid] = in ? xf[f][o] * p : 0.0;
            __syncthreads();
            if (in && (tid == 0 || s_lane[tid - 1] != lane)) {  // the head of a run: the lane's cells of this chunk, in order
                double a[NB];
#pragma unroll
                for (int f = 0; f < NB; ++f) a[f] = s_acc[f][lane];
                int j = tid;
                do {
#pragma unroll
                    for (int f = 0; f < NB; ++f) a[f] = a[f] + s_prod[f][j];
                    ++j;
                } while (j < kExpBlock && s_lane[j] == lane);
#pragma unroll
                for (int f = 0; f < NB; ++f) s_acc[f][lane] = a[f];
            }
            __syncthreads();
        }
#pragma unroll
        for (int f = 0; f < NB; ++f) acc[r * NB + f] = s_acc[f][tid];
    }
    exp_block_sum<kExpRows * NB>(acc, s_part, s_y);

    // the residuals that arrive at these destinations (D1): x[o] * r[o] over the destination's origins, ascending
    for (int r = 0; r < kExpRows; ++r) {
        const int d = d0 + r;
        int ka = 0, kb = 0;
        if (d < Z) {
            ka = start_t[d];
            kb = start_t[d + 1];
        }
        if (kb > ka) {  // (uniform over the workgroup)
            double a2[NB];
#pragma unroll
            for (int f = 0; f < NB; ++f) a2[f] = 0.0;
            for (int k = ka + tid; k < kb; k += kExpBlock) {
                const int o = list_t[k];
                const double rr = r_t[o];
#pragma unroll
                for (int f = 0; f < NB; ++f) a2[f] = a2[f] + xf[f][o] * rr;
            }
            exp_block_sum<NB>(a2, s_part, s_res + r * NB);
        } else if (tid < NB) {
            s_res[r * NB + tid] = 0.0;
        }
    }
    __syncthreads();

    if (tid < kExpRows * NB) {
        const int r = tid / NB, f = tid % NB, d = d0 + r;
        if (d < Z && f < nf) {
            const size_t i = static_cast<size_t>(f) * Zs + d;
            const double pi = pi_in[i];
            const double stay = pi * (1.0 - exp_q(q_cur[static_cast<size_t>(f) * q_stride + d]));
            double v = stay + s_y[tid];
            v = v + s_res[tid];
            if (last_t[d] == 0.0) v = v + x_in[i];  // a zero row: the driver stays where it is (src/resampling.jl:35-36)
            pi_out[i] = v;
            if (park) park[static_cast<size_t>(f) * out_stride + d] = v;
            if (q_next) {
                const double xn = v * exp_q(q_next[static_cast<size_t>(f) * q_stride + d]);
                x_out[i] = xn;
                if (drv) drv[static_cast<size_t>(f) * out_stride + d] = xn;
            }
        }
    }
}

}  // namespace cpm
