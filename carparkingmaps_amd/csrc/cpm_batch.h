// cpm_batch.h -- the batched resample (include/cpm_batch.h): B fleets, each with its own p_drive table and seed, from the context's
// car state and p_destin tables, in one pass over the row packs per hour.
//
// The model-selection sweep's points that share e_dest differ only in a Z x T p_drive table; one resample of the headline shape streams
// 76 MB of row packs per hour for 33 MB of per-car work.  Here each hour is
//   * k_batch_sample: one workgroup per (origin zone, sub-batch of F fleets).  The zone's row pack is staged into LDS ONCE, then the
//     workgroup walks the zone's bucket of every fleet of its sub-batch through grouped_sample_body<..., STAGED> -- the hourly sampler's
//     own code: Bernoulli draw against that fleet's thresholds, categorical draw from the staged pack with the exact f64 fallback on
//     ties, stayers and drivers into that fleet's buckets and runs, that fleet's counts.  Overflow rounds walk buckets beyond the
//     workgroup's slots (no heavy launch: parts = 1).
//   * k_batch_place: the placing of every fleet's drivers, the fleet in blockIdx.y (grouped_place_body).
//   * travel times (CPM_FLAG_TRAVEL): k_grouped_travel once per fleet, from that fleet's runs into that fleet's partial sums (a kernel of
//     its own with the fleet in the grid would give the hourly travel kernel's out-of-line helpers a second caller, and the compiler
//     what it infers from them: the hourly kernels' code must not move).
// The per-(hour, fleet) arguments are GroupedArgs records in device memory (k_batch_fill writes them from one by-value struct, as
// k_grouped_zero writes a day launch's hours): GroupedArgs itself gains no field.
//
// The batch owns its workspace (BatchWork): its own initial bucketing of the context's state (cached while the state is unchanged),
// per-fleet buckets, runs, counters and status words, its own region size.  The single path's GroupedWork is never touched.
#pragma once
#include "cpm_grouped.h"
#include "../../include/cpm_batch.h"

namespace cpm {

constexpr int kMaxBatch = CPM_MAX_BATCH;

// What the (hour, fleet) records of one run are derived from (kernel argument: no host-to-device copy in the stream)
struct BatchFill {  // (a kernel argument: at most 4 KiB)
    GroupedArgs base;                    // what every hour and fleet shares
    GroupedRare rare;                    // ... and every fleet's rare-branch tables (status filled per fleet)
    const uint32_t *ids0, *cnt0;         // the batch's initial bucketing: hour 0's buckets of every fleet
    const unsigned long long *bstatus;   // its status word: a bucket outgrew its region while bucketing -> every fleet's step is invalid
    uint32_t *ids, *cnt, *D, *cntg;      // per fleet: [2][Z*cap] ping-pong buckets, [T+1][2][Z] counts, runs, run lengths
    unsigned long long *tt_part;         // per fleet: [kTravelParts] partial travel-time sums
    GroupedRare *rare_out;               // [nf]
    GroupedArgs *args;                   // [T][nf]
    uint32_t *scratch;                   // maxn[2] + nheavy[T+1]: the sampler body's heavy-bucket bookkeeping (parts = 1: read by nobody)
    const uint32_t *rp;                  // [T][Z][rw] row packs
    const double *last;                  // [T][Z] row totals
    const long long *thr;                // [tables][T][Z] Bernoulli thresholds of the batch tables
    unsigned long long *counts;          // [slots][nwords] count tensors
    size_t rw, slots, cnt_words, run_words, len_words, nwords;
    int nf, T;
    uint32_t step0;
    uint64_t seed[kMaxBatch];            // fleet f of the run: its seed, its table, its count tensor
    int32_t tab[kMaxBatch], out[kMaxBatch];
};

static_assert(sizeof(BatchFill) <= 4096, "kernel argument segment");

__global__ __launch_bounds__(256) void k_batch_fill(BatchFill f)
{
    const int fl = blockIdx.y;
    const size_t stride = static_cast<size_t>(gridDim.x) * 256, i0 = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
    unsigned long long *counts = f.counts + static_cast<size_t>(f.out[fl]) * f.nwords;
    for (size_t i = i0; i + 1 < f.nwords; i += stride) counts[i] = 0ull;  // (the status word: below)
    uint32_t *cnt = f.cnt + static_cast<size_t>(fl) * f.cnt_words;
    for (size_t i = i0; i < f.cnt_words; i += stride) cnt[i] = 0u;  // (the arrival counts are added to)
    if (blockIdx.x != 0) return;
    f.tt_part[static_cast<size_t>(fl) * kTravelParts + threadIdx.x] = 0ull;
    if (fl == 0)
        for (int k = threadIdx.x; k < f.T + 3; k += 256) f.scratch[k] = 0u;
    if (threadIdx.x == 0) {
        counts[f.nwords - 1] = *f.bstatus;
        GroupedRare r = f.rare;
        r.status = counts + f.nwords - 1;
        f.rare_out[fl] = r;
    }
    const size_t Z = static_cast<size_t>(f.base.Z);
    uint32_t *idsA = f.ids + static_cast<size_t>(fl) * 2 * f.slots, *idsB = idsA + f.slots;
    for (int t = threadIdx.x; t < f.T; t += 256) {
        const size_t ts = static_cast<size_t>(t);
        GroupedArgs a = f.base;
        a.rare = f.rare_out + fl;
        a.seed = f.seed[fl];
        a.ids = t == 0 ? f.ids0 : (((t - 1) & 1) ? idsB : idsA);
        a.cnt_s = t == 0 ? f.cnt0 : cnt + ts * 2 * Z;
        a.cnt_a = a.cnt_s + Z;
        a.rp_t = f.rp + ts * Z * f.rw;
        a.last_t = f.last + ts * Z;
        a.thr_t = f.thr + (static_cast<size_t>(f.tab[fl]) * f.T + ts) * Z;
        a.ids_next = (t & 1) ? idsB : idsA;
        a.cnt_next = cnt + (ts + 1) * 2 * Z;
        a.D = f.D + static_cast<size_t>(fl) * f.run_words;
        a.cntg = f.cntg + static_cast<size_t>(fl) * f.len_words;
        a.parking_t = counts + ts * Z;
        a.driving_t = counts + (static_cast<size_t>(f.T) + ts) * Z;
        a.hour = t;
        a.step = f.step0 + static_cast<uint32_t>(t);
        f.args[ts * f.nf + fl] = a;
    }
}

// grid = Z x ceil(nf / per_wg): workgroup (z, s) stages zone z's pack once and walks fleets s * per_wg .. of the hour's records.
// GROUPED as in the hourly sampler: stayers and runs; !GROUPED, hour T of a resample without travel times (sampled, never placed): the
// plain form, counts only -- as the single path runs that hour with CPM_OPT_LAST_HOUR 0 (1, the default: k_batch_count, cpm_count.h).
// Between two fleets the workgroup meets: the LDS beside the pack (SampleLds: ranks, staged drivers, counters) is reset per fleet, and
// a first fleet whose bucket is empty returns from the body without a barrier -- its wait (vmcnt(0)) and this barrier put the pack
// in front of the next fleet.
template <int BLOCK, int CPT, bool GROUPED, bool SPARSE>
__global__ __launch_bounds__(BLOCK, CPM_WPS) void k_batch_sample(const GroupedArgs *__restrict__ fleets, int nf, int per_wg)
{
    extern __shared__ uint32_t pack[];  // the zone's row pack: guide (u16), then Zq high words (sparse: and the destination map)
    __shared__ SampleLds sl;
    const int z = blockIdx.x, f0 = static_cast<int>(blockIdx.y) * per_wg, f1 = min(nf, f0 + per_wg);
    {   // LDS-DMA, 64 x 16 B per wave-instruction; the last chunk of a pack is moved back to end on the pack's end (same bytes twice)
        const GroupedArgs &a = fleets[f0];
        const int pieces = pack_row_words(a.Zq, a.G, SPARSE ? 1 : 0) / 4;  // (>= 64: a pack is at least 1 KiB)
        const char *src = reinterpret_cast<const char *>(a.rp_t + static_cast<size_t>(z) * pieces * 4);
        const int lane = threadIdx.x & 63;
        for (int p0 = (threadIdx.x >> 6) * 64; p0 < pieces; p0 += BLOCK) {  // (wave-uniform trips)
            const int q = min(p0, pieces - 64);
            __builtin_amdgcn_global_load_lds(src + (static_cast<uint32_t>(q + lane) << 4), (__attribute__((address_space(3))) void *)(pack + 4 * q), 16, 0, 0);
        }
    }
    for (int f = f0; f < f1; ++f) {
        if (f != f0) __syncthreads();
        grouped_sample_body<BLOCK, CPT, 1, GROUPED, false, false, SPARSE, true>(fleets[f], z, pack, sl, nullptr);
    }
}

// the drivers of every fleet of the hour into next hour's buckets: blockIdx.x as k_grouped_place's, the fleet in blockIdx.y
template <int PB, int KRUNS, int KDEEP>
__global__ __launch_bounds__(PB) void k_batch_place(const GroupedArgs *__restrict__ fleets, int zps)
{
    __shared__ PlaceLds<PB, KRUNS, kMaxZonesPerGroup> pl;
    extern __shared__ uint32_t sorted_ids[];
    const GroupedArgs &a = fleets[blockIdx.y];
    grouped_place_body<PB, KRUNS, KDEEP, kMaxZonesPerGroup, false, false, false, 1>(blockIdx.x % kGroups, blockIdx.x / kGroups, pl, sorted_ids, a.D, a.cntg,
                                                                    static_cast<int>(gdiv_zpg(a.gdiv)), zps, a.Z, a.cap, a.scap, a.idbits,
                                                                    a.cnt_next + a.Z, a.ids_next, a.rare->status, nullptr, 0u, 0u);
}

// the status words of a batch step's nf count tensors (d_counts + f * nwords) ORed into one word: what the context learns from an
// asynchronous batch step before the next one (cpm_api.hip, as the single path learns from its status word)
__global__ __launch_bounds__(64) void k_batch_status(const unsigned long long *__restrict__ counts, size_t nwords, int nf, unsigned long long *__restrict__ out)
{
    unsigned long long v = static_cast<int>(threadIdx.x) < nf ? counts[threadIdx.x * nwords + nwords - 1] : 0ull;
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
    if (threadIdx.x == 0) *out = v;
}

// the partial sums of fleet blockIdx.x -> the sum word of its count tensor (which sits in front of its status word)
__global__ __launch_bounds__(256) void k_batch_travel_finish(const GroupedArgs *__restrict__ fleets, unsigned long long *__restrict__ tt_part)
{
    unsigned long long *p = tt_part + static_cast<size_t>(blockIdx.x) * kTravelParts;
    unsigned long long v = p[threadIdx.x];
    p[threadIdx.x] = 0;
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(fleets[blockIdx.x].rare->status - 1, v);
}

// ------------------------------------------------------------------------------------------------ workspace and driver
struct BatchWork {
    int64_t n = 0;
    int Z = 0, T = 0, nf_alloc = 0, nb0 = 1;
    int cap_mult = 4;        // bucket region = cap_mult x the mean bucket; doubled after an overflow (the batch's own, not CPM_INFO_CAP_MULT)
    int cap_mult_alloc = 0;
    uint32_t cap = 0, scap = 0, idbits = 0, gdiv = 0, zpg = 1;
    bool buckets0_valid = false;  // ids0 / cnt0 describe the context's current car state
    bool count_only = true;       // CPM_OPT_LAST_HOUR: hour T without travel times by k_batch_count (cpm_count.h)
    int last_hour_counted = 0;    // ... 1 when the last run's hour T was that launch (CPM_INFO_LAST_HOUR)
    LaunchCells last_cells;       // CPM_INFO_CELL_*: what the launch helpers of the last run wrote (launch_cells())
    uint32_t *ids0 = nullptr, *cnt0 = nullptr;
    unsigned long long *bstatus = nullptr;
    uint32_t *ids = nullptr, *cnt = nullptr, *D = nullptr, *cntg = nullptr, *scratch = nullptr;
    unsigned long long *tt_part = nullptr;
    GroupedRare *rare = nullptr;
    GroupedArgs *args = nullptr;

    size_t slots() const { return static_cast<size_t>(Z) * cap; }
    size_t cnt_words() const { return static_cast<size_t>(T + 1) * 2 * Z; }
    size_t run_words() const { return static_cast<size_t>(Z) * kGroups * scap; }
    size_t len_words() const { return static_cast<size_t>(Z) * kGroups; }
    // device bytes of one fleet: two bucket arrays, one copy of the runs (the hour's launches follow each other on one stream), counters
    static size_t fleet_bytes(int64_t n, int Z, int T, int cap_mult)
    {
        const size_t cap = grouped_cap(n, Z, cap_mult), scap = grouped_scap(static_cast<uint32_t>(cap));
        return 4 * (2 * static_cast<size_t>(Z) * cap + static_cast<size_t>(T + 1) * 2 * Z + static_cast<size_t>(Z) * kGroups * (scap + 1)) +
               8 * kTravelParts + sizeof(GroupedRare) + sizeof(GroupedArgs) * static_cast<size_t>(T);
    }
    // fleets one run takes: as many as fit the budget of grouped_path_fits (24 GiB; 80 once the regions have grown)
    static int sub_batch(int64_t n, int Z, int T, int cap_mult, int B)
    {
        const size_t budget = static_cast<size_t>(cap_mult <= 4 ? 24 : 80) << 30;
        return static_cast<int>(std::max<size_t>(1, std::min<size_t>(static_cast<size_t>(B), budget / fleet_bytes(n, Z, T, cap_mult))));
    }
    void set_groups(bool general)
    {
        idbits = grouped_idbits(Z, general);
        gdiv = grouped_gdiv_of(Z, general);
        zpg = grouped_zpg_of(Z, general);
    }
    void release()
    {
        for (uint32_t **p : {&ids0, &cnt0, &ids, &cnt, &D, &cntg, &scratch}) {
            if (*p) (void)hipFree(*p);
            *p = nullptr;
        }
        if (bstatus) (void)hipFree(bstatus);
        if (tt_part) (void)hipFree(tt_part);
        if (rare) (void)hipFree(rare);
        if (args) (void)hipFree(args);
        bstatus = nullptr;
        tt_part = nullptr;
        rare = nullptr;
        args = nullptr;
        n = 0;
        nf_alloc = 0;
        buckets0_valid = false;
    }
    hipError_t ensure(int64_t n_, int Z_, int T_, int nf, int cu_count)
    {
        if (n_ == n && Z_ == Z && T_ == T && nf <= nf_alloc && ids0 && cap_mult_alloc == cap_mult) return hipSuccess;
        release();
        n = n_;
        Z = Z_;
        T = T_;
        nf_alloc = nf;
        cap_mult_alloc = cap_mult;
        cap = grouped_cap(n, Z, cap_mult);
        scap = grouped_scap(cap);
        set_groups(false);
        nb0 = static_cast<int>(std::max<int64_t>({int64_t(1), std::min<int64_t>(2 * cu_count, (n + 4095) / 4096),
                                                  (n + int64_t(kBucketMaxPass) * 1024 - 1) / (int64_t(kBucketMaxPass) * 1024)}));
        hipError_t e = hipSuccess;
        auto alloc = [&](void **p, size_t bytes) {
            if (e == hipSuccess) e = hipMalloc(p, std::max<size_t>(bytes, 4));
        };
        const size_t F = static_cast<size_t>(nf);
        alloc(reinterpret_cast<void **>(&ids0), 4 * slots());
        alloc(reinterpret_cast<void **>(&cnt0), 4 * 2 * static_cast<size_t>(Z));
        alloc(reinterpret_cast<void **>(&bstatus), sizeof(unsigned long long));
        alloc(reinterpret_cast<void **>(&ids), 4 * F * 2 * slots());
        alloc(reinterpret_cast<void **>(&cnt), 4 * F * cnt_words());
        alloc(reinterpret_cast<void **>(&D), 4 * F * run_words());
        alloc(reinterpret_cast<void **>(&cntg), 4 * F * len_words());
        alloc(reinterpret_cast<void **>(&scratch), 4 * static_cast<size_t>(T + 3));
        alloc(reinterpret_cast<void **>(&tt_part), 8 * F * kTravelParts);
        alloc(reinterpret_cast<void **>(&rare), sizeof(GroupedRare) * F);
        alloc(reinterpret_cast<void **>(&args), sizeof(GroupedArgs) * F * static_cast<size_t>(T));
        if (e != hipSuccess) release();
        return e;
    }
};

// fleets per workgroup of k_batch_sample: the pack is staged once per workgroup, so as many fleets as still leave two rounds of
// workgroups on the chip (sampler workgroups per CU: CPM_WPS, fewer when the pack and SampleLds fill the CU's 160 KiB of LDS), dealt
// evenly over the sub-batches
inline int batch_per_wg(int nf, int Z, size_t pack_bytes, int cu_count)
{
    const int per_cu = std::max(1, std::min(CPM_WPS, static_cast<int>((160 * 1024) / (pack_bytes + sizeof(SampleLds)))));
    const int64_t slots = static_cast<int64_t>(per_cu) * std::max(cu_count, 1);
    const int F = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(nf, static_cast<int64_t>(Z) * nf / (2 * slots))));
    const int nsub = (nf + F - 1) / F;
    return (nf + nsub - 1) / nsub;
}

template <int CPT, bool GROUPED, bool SPARSE>
inline hipError_t batch_launch_sample_t(const GroupedArgs *fleets, int nf, int per_wg, int Z, size_t lds, hipStream_t stream)
{
    constexpr auto kernel = k_batch_sample<kSampleBlock, CPT, GROUPED, SPARSE>;
    const hipError_t e = lds_opt_in<kernel>(lds, kPackLds);
    if (e != hipSuccess) return e;
    (launch_cells().hour_T ? launch_cells().last : launch_cells().batch) = cell_word(kCellBatchSample, CPT, 0, GROUPED, SPARSE);
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(Z), static_cast<unsigned>((nf + per_wg - 1) / per_wg)), dim3(kSampleBlock), lds, stream, fleets, nf,
                       per_wg);
    return hipSuccess;
}
template <bool GROUPED, bool SPARSE>
inline hipError_t batch_launch_sample_s(const GroupedArgs *fleets, int nf, int per_wg, int Z, size_t lds, int64_t mean, hipStream_t stream)
{
    // (no heavy launch follows: the slots of the hourly sampler where none does)
    return ladder_walk<BatchCells::cpt>(grouped_cpt_wide(mean), [&](auto CPT) { return batch_launch_sample_t<CPT, GROUPED, SPARSE>(fleets, nf, per_wg, Z, lds, stream); });
}

template <int PB, int KRUNS>
inline hipError_t batch_launch_place_t(const GroupedArgs *fleets, int nf, int bpg, int Z, hipStream_t stream)
{
    constexpr auto kernel = k_batch_place<PB, KRUNS, 2>;
    const size_t lds = static_cast<size_t>(6) * KRUNS * 2 * PB;  // sorted ids (4 B) + their zones (2 B) per slot
    const hipError_t e = lds_opt_in<kernel>(lds);
    if (e != hipSuccess) return e;
    launch_cells().place = place_word(kCellBatchPlace, PB, KRUNS);
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(kGroups * bpg), static_cast<unsigned>(nf)), dim3(PB), lds, stream, fleets, (Z + bpg - 1) / bpg);
    return hipSuccess;
}
inline hipError_t batch_launch_place(const GroupedArgs *fleets, int nf, int Z, hipStream_t stream)
{
    const PlaceShape p = place_shape(Z);
    return place_walk(p, [&](auto PB, auto KRUNS) { return batch_launch_place_t<PB, KRUNS>(fleets, nf, p.bpg, Z, stream); });
}

// One run of nf <= BatchWork::sub_batch fleets: fleet f draws with seeds[f] against the thresholds of batch table tabs[f] and writes the
// count tensor d_counts + outs[f] * (2*T*Z + 2) (zeroed here; status word != 0: its counts are invalid -- a bucket or a run outgrew
// its region).  Enqueued on `stream`; d_zone0 is read (bucketed) only when the cached bucketing is stale.
inline int32_t batch_run(BatchWork &w, hipStream_t stream, const GroupedTables &tb, int64_t n, CarIndex cars, const uint32_t *d_zone0,
                         const long long *thr_tables, const uint64_t *seeds, const int32_t *tabs, const int32_t *outs, int nf, bool travel,
                         int64_t *d_counts, int cu_count, std::string &err)
{
    auto hip_fail = [&](hipError_t e, const char *what) {
        err = std::string(what) + ": " + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? CPM_ERR_NOMEM : CPM_ERR_HIP;
    };
    const int Z = tb.Z, T = tb.T;
    hipError_t e = w.ensure(n, Z, T, nf, cu_count);
    if (e != hipSuccess) return hip_fail(e, "batch workspace");
    w.set_groups(tb.smap != 0);
    if (!w.buckets0_valid) {  // bucket the car-indexed state once; reused until the state changes
        const size_t lds_bins = sizeof(uint32_t) * static_cast<size_t>(Z);
        if ((e = lds_opt_in<k_bucket_cars>(lds_bins)) != hipSuccess) return hip_fail(e, "LDS of the batch bucketing");
        if ((e = hipMemsetAsync(w.cnt0, 0, sizeof(uint32_t) * 2 * Z, stream)) != hipSuccess) return hip_fail(e, "memset cnt0");
        if ((e = hipMemsetAsync(w.bstatus, 0, sizeof(unsigned long long), stream)) != hipSuccess) return hip_fail(e, "memset status");
        const int64_t chunk = (n + w.nb0 - 1) / w.nb0;
        hipLaunchKernelGGL(k_bucket_cars, dim3(w.nb0), dim3(kBucketBlock), lds_bins, stream, d_zone0, n, chunk, Z, w.cap, w.cnt0, w.ids0, w.bstatus);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "batch bucketing");
        w.buckets0_valid = true;
    }
    const size_t rw = static_cast<size_t>(pack_row_words(tb.Zq, tb.G, tb.smap));
    const size_t nwords = 2 * static_cast<size_t>(T) * Z + 2;
    {
        BatchFill f;
        std::memset(&f, 0, sizeof f);
        GroupedArgs &a = f.base;
        a.Z = Z;
        a.Zq = tb.Zq;
        a.G = tb.G;
        a.Zc = tb.Zc;
        a.smap = tb.smap;
        a.cap = w.cap;
        a.scap = w.scap;
        a.idbits = w.idbits;
        a.gdiv = w.gdiv;
        a.cars = cars;
        a.lag = 1 << 20;
        a.heavy_x = kHeavy;
        GroupedRare &r = f.rare;
        r.ckpt = tb.ckpt;
        r.p = tb.p;
        r.sp = tb.sp;
        r.sj = tb.sj;
        r.scnt = tb.scnt;
        r.scap = tb.scap;
        r.maxn = w.scratch;
        r.nheavy = w.scratch + 2;
        r.parts = 1;
        r.Z = Z;
        f.ids0 = w.ids0;
        f.cnt0 = w.cnt0;
        f.bstatus = w.bstatus;
        f.ids = w.ids;
        f.cnt = w.cnt;
        f.D = w.D;
        f.cntg = w.cntg;
        f.tt_part = w.tt_part;
        f.rare_out = w.rare;
        f.args = w.args;
        f.scratch = w.scratch;
        f.rp = tb.rp;
        f.last = tb.last;
        f.thr = thr_tables;
        f.counts = reinterpret_cast<unsigned long long *>(d_counts);
        f.rw = rw;
        f.slots = w.slots();
        f.cnt_words = w.cnt_words();
        f.run_words = w.run_words();
        f.len_words = w.len_words();
        f.nwords = nwords;
        f.nf = nf;
        f.T = T;
        f.step0 = static_cast<uint32_t>(T - 1);
        for (int k = 0; k < nf; ++k) {
            f.seed[k] = seeds[k];
            f.tab[k] = tabs[k];
            f.out[k] = outs[k];
        }
        const unsigned zgrid = static_cast<unsigned>(std::min<size_t>((std::max(nwords, w.cnt_words()) + 255) / 256, 256));
        hipLaunchKernelGGL(k_batch_fill, dim3(zgrid, static_cast<unsigned>(nf)), dim3(256), 0, stream, f);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "batch records");
    }
    const int64_t mean = (n + Z - 1) / Z;
    const size_t lds = sizeof(uint32_t) * rw;
    const int per_wg = batch_per_wg(nf, Z, lds, cu_count);
    const int tblock = travel_block(mean, false);
    w.last_hour_counted = 0;
    LaunchCells &cells = launch_cells();
    cells = LaunchCells{};
    for (int t = 0; t < T; ++t) {
        cells.hour_T = t + 1 == T;
        const GroupedArgs *at = w.args + static_cast<size_t>(t) * nf;
        const bool grouped = t + 1 < T || travel;  // (hour T without travel times: counts only, as in grouped_run)
        if (!grouped && w.count_only) {  // counts only: no pack, no search, nothing stored per car (cpm_count.h)
            const uint32_t cpt = static_cast<uint32_t>(grouped_cpt_wide(mean));  // (the cars per lane of the plain launch it stands for)
            cells.last = kCellBatchCount | cpt << 8 | (tb.smap ? kCellSparse : 0u) << 24;
            hipLaunchKernelGGL(k_batch_count, dim3(static_cast<unsigned>(Z), static_cast<unsigned>(nf)), dim3(kCountBlock), 0, stream, at, cpt);
            w.last_hour_counted = 1;
        } else if (tb.smap) {
            if (grouped) e = batch_launch_sample_s<true, true>(at, nf, per_wg, Z, lds, mean, stream);
            else e = batch_launch_sample_s<false, true>(at, nf, per_wg, Z, lds, mean, stream);
        } else {
            if (grouped) e = batch_launch_sample_s<true, false>(at, nf, per_wg, Z, lds, mean, stream);
            else e = batch_launch_sample_s<false, false>(at, nf, per_wg, Z, lds, mean, stream);
        }
        if (e == hipSuccess && t + 1 < T) e = batch_launch_place(at, nf, Z, stream);  // (hour T is sampled, never applied: src/resampling.jl:81-83)
        if (e != hipSuccess) return hip_fail(e, "LDS of the batch hour's launches");
        if (travel) {
            TravelArgs tr{};
            tr.tt = tb.tt;
            tr.tts_words = tb.tts_words;
            tr.tts_off = tb.tts_stride ? tb.tts_cnt : tb.tts_off;
            tr.tts_stride = tb.tts_stride;
            tr.tts_cells = tb.tts_cells;
            tr.W = tb.tts_W;
            tr.list_off = static_cast<uint32_t>(tb.tts_lds);
            tr.tt_part = w.tt_part;
            tr.t0 = t;
            tr.zpg = static_cast<int>(w.zpg);
            tr.step0 = static_cast<uint32_t>(T - 1 + t);
            tr.cars = cars;
            for (int k = 0; k < nf; ++k) {
                tr.seed = seeds[k];
                tr.tt_part = w.tt_part + static_cast<size_t>(k) * kTravelParts;
                const uint32_t *D = w.D + static_cast<size_t>(k) * w.run_words(), *cg = w.cntg + static_cast<size_t>(k) * w.len_words();
                if (tb.tts_words) hipLaunchKernelGGL(k_grouped_travel<true>, dim3(Z, 1), dim3(tblock), travel_lds_bytes(tb.tts_lds, tblock), stream, D, cg, Z, w.scap, w.idbits, tr);
                else hipLaunchKernelGGL(k_grouped_travel<false>, dim3(Z, 1), dim3(tblock), 0, stream, D, cg, Z, w.scap, w.idbits, tr);
            }
        }
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "batch hour launch");
    }
    if (travel) {
        hipLaunchKernelGGL(k_batch_travel_finish, dim3(static_cast<unsigned>(nf)), dim3(kTravelParts), 0, stream, w.args, w.tt_part);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "batch travel-time sums");
    }
    w.last_cells = cells;
    return CPM_OK;
}

}  // namespace cpm
