// cpm_dispatch.h -- the host rules that choose an INSTANTIATION of the grouped path's hourly kernels, free of HIP: the row pack's
// geometry, the destination groups, the cars per thread, the ladders over template parameters as data, the placing geometry and the
// launch record's coding.  Plain host arithmetic: `g++ -std=c++17` compiles this header alone, and tests/dispatch_probe.cc prints these
// rules for tests/test_dispatch_cells.py to hold against their restatement in tests/dispatch_cells.py without a GPU.
//
// A family of kernels is a struct of tables (SampleCells, HourCells, ...): the CPT and NQ values it is compiled for and the NQ of a
// sparse pack.  ladder_walk turns a run-time value into the compile-time rung of such a table; the launchers (cpm_grouped.h,
// cpm_day.h, cpm_batch.h, cpm_exact.h) walk their family's tables and write only their innermost body.  A new form of the hour adds
// a struct here.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstddef>
#include <type_traits>

#if defined(__HIPCC__)
#define CPM_HD __host__ __device__
#else
#define CPM_HD
#endif

namespace cpm {

constexpr int kGroups = 32;       // destination groups
constexpr int kSampleBlock = 256;  // measured at S4k: 512 threads x 2 cars: 31 us, 256 x 4: 28, 128 x 8: 44
constexpr int kFusedZpg = 256;    // zones per destination group the fused form is built for (Z <= 8,192)
constexpr size_t kPackLds = 150 * 1024;  // the LDS a workgroup may ask for: what a row pack must fit, and what the samplers opt in to

// Destination groups: kGroups groups of zpg CONSECUTIVE zones, a power of two for dense tables, ceil(Z / kGroups) for GENERAL groups
// (the sparse instantiations); the packed divisor word and why there are two forms: grouped_gdiv_of, cpm_grouped.h.
inline uint32_t grouped_zpg_of(int Z, bool general = false)
{
    if (general) return static_cast<uint32_t>(std::max(1, (Z + kGroups - 1) / kGroups));
    uint32_t s = 0;
    while ((static_cast<int64_t>(kGroups) << s) < Z) ++s;
    return 1u << s;
}
// packed driver = id | (dest - group * zpg) << idbits: the local destination takes ceil(log2 zpg) bits, at least one
inline uint32_t grouped_idbits(int Z, bool general = false)
{
    uint32_t b = 1;
    while ((1u << b) < grouped_zpg_of(Z, general)) ++b;
    return 32u - b;
}

// ------------------------------------------------------------------------------------------------ row packs
CPM_HD constexpr int pack_guide_bits(int Z)
{
    int g = 3;  // >= 8 entries: the guide is a whole number of 16-B pieces
    while ((1 << g) < Z) ++g;
    // a quarter of an entry per destination: measured best at S4k (entries per destination 1: 32.0 us, 1/2: 29.9, 1/4: 29.1 --
    // the shorter pack outweighs the longer bracket)
    g = g - 2 < 3 ? 3 : g - 2;
    return g;
}
// high words per row: Z, then at least 31 entries of 0xFFFFFFFF (the unclamped stride walk of pack_search reads up to 30 past
// its bracket), a whole number of 128-B lines
CPM_HD constexpr int pack_zq(int Z) { return (Z + 31 + 31) / 32 * 32; }
CPM_HD constexpr int pack_guide_words(int G) { return (1 << G) / 2 + 4; }  // 2^G + 1 entries used (+7 pad: whole 16-B pieces)
// smap (sparse pack, cpm_dataset.h): Zq and G of the compact row, and a u16 destination per entry behind the high words
CPM_HD constexpr int pack_row_words(int Zq, int G, int smap = 0)  // at least 1 KiB: one whole LDS-DMA wave-instruction
{
    const int w = pack_guide_words(G) + Zq + (smap ? Zq / 2 : 0);  // (Zq is a multiple of 32, the guide of 4: whole 16-byte pieces)
    return w < 256 ? 256 : w;  // (rows rounded up to whole 128-byte lines: -0.3 % at S4k, within noise -- profiles/round4_notes.md)
}
// a row pack must fit the 150 KiB of LDS a workgroup may ask for, and a guide entry is a u16
inline bool pack_row_fits(int Z)
{
    if (Z < 2 || Z > 32768) return false;
    return sizeof(uint32_t) * static_cast<size_t>(pack_row_words(pack_zq(Z), pack_guide_bits(Z))) <= kPackLds;
}
// 16-byte pieces of a row pack over the lanes of a sampler workgroup: the LDS-DMA instructions per wave its staging NEEDS
constexpr int pack_need(int Zq, int G, int smap = 0) { return (pack_row_words(Zq, G, smap) / 4 + kSampleBlock - 1) / kSampleBlock; }

// ------------------------------------------------------------------------------------------------ cars per thread
// Cars per thread by the mean bucket size (cars of this GPU / zones): 256 x 4 slots for ~1000 cars per zone, 256 x 2 and 256 x 1
// for smaller buckets (every slot runs Philox whether a car sits in it or not); larger buckets take the overflow rounds.
inline int grouped_cpt(int64_t mean) { return mean <= 224 ? 1 : (mean <= 560 ? 2 : 4); }
// ... and where no heavy bucket has been seen (the heavy launch shares the sampler's chunking: it stays with grouped_cpt): slots for
// 1.5 x the mean bucket.  Buckets spread from half to 2.5 x the mean on flat tables, and a bucket beyond its workgroup's slots pays a
// whole serial round (ids, Philox, search, ranks) per 256 cars more, while a wave only runs the K <= CPT cars per lane it holds
// (first_pass): at S4k 42 % of the buckets needed such rounds with 4 cars per lane, 0.851 -> 0.815 ms per resample with 6 (same box,
// interleaved; 5: 0.827, 7: 0.824 with 9 vector registers spilled, 8 at five waves per SIMD: 0.856 -- profiles/round4_notes.md).
#ifndef CPM_CPT_RULE
#define CPM_CPT_RULE 1
#endif
inline int grouped_cpt_wide(int64_t mean)
{
    if (CPM_CPT_RULE == 0) return grouped_cpt(mean);
    return mean <= 170 ? 1 : (mean <= 340 ? 2 : (mean <= 700 ? 4 : 6));
}

// ------------------------------------------------------------------------------------------------ the ladders
// What each family of kernels is compiled for.  cpt: the values its cars-per-thread rule can return; nq: the rungs of its need -> NQ
// ladder (the first rung that holds the pack's need, the last one beyond); sparse_nq: a sparse pack is at most kDsCap entries -- one
// LDS-DMA instruction per wave (the heavy kernel's smallest rung is 2) -- and takes this NQ before the ladder is consulted.
struct SampleCells {  // k_grouped_sample
    static constexpr int cpt[] = {1, 2, 4, 6}, nq[] = {1, 2, 3, 4, 5, 6, 8, 12, 20, 40}, sparse_nq = 1;
};
struct HourCells {  // k_grouped_hour
    static constexpr int cpt[] = {1, 2, 4, 6}, nq[] = {1, 2, 3, 4, 5, 6, 8, 12}, sparse_nq = 1;
};
struct HourPfCells {  // k_grouped_hour_pf
    static constexpr int cpt[] = {1, 2, 4}, nq[] = {1, 2, 3, 4, 5, 6, 8, 12}, sparse_nq = 1;
};
struct DayCells {  // k_grouped_day
    static constexpr int cpt[] = {1, 2, 4}, nq[] = {1, 2, 3, 4, 5, 6, 8, 12}, sparse_nq = 1;
};
struct HeavyCells {  // k_grouped_sample_heavy
    static constexpr int cpt[] = {1, 2, 4}, nq[] = {2, 5, 12, 40}, sparse_nq = 2;
};
struct BatchCells {  // k_batch_sample (no NQ: it stages its pack in a loop)
    static constexpr int cpt[] = {1, 2, 4, 6};
};
struct PlaceCells {  // k_grouped_place, k_batch_place: threads per block, runs per 16 threads
    static constexpr int pb[] = {512, 1024}, kruns[] = {4, 8};
};
struct ExactCells {  // k_exact_sample: pairs of CDF entries per thread
    static constexpr int np[] = {1, 2, 4, 8, 16};
};

// f(std::integral_constant<int, R>{}) for the first rung R of Table with v <= R, for the last rung when there is none
template <const auto &Table, size_t I = 0, typename F>
inline auto ladder_walk(int v, F &&f)
{
    constexpr int rung = Table[I];
    if constexpr (I + 1 == std::extent_v<std::remove_reference_t<decltype(Table)>>) return f(std::integral_constant<int, rung>{});
    else return v <= rung ? f(std::integral_constant<int, rung>{}) : ladder_walk<Table, I + 1>(v, f);
}
// (cpt, need, sparse) of a family -> f(CPT, NQ, SPARSE) as compile-time constants: every launcher's choice of its instantiation
template <typename Cells, typename F>
inline auto cell_walk(int cpt, int need, bool sparse, F &&f)
{
    return ladder_walk<Cells::cpt>(cpt, [&](auto CPT) {
        if (sparse) return f(CPT, std::integral_constant<int, Cells::sparse_nq>{}, std::true_type{});
        return ladder_walk<Cells::nq>(need, [&](auto NQ) { return f(CPT, NQ, std::false_type{}); });
    });
}
// the rung alone (the probe and the shape predicates)
template <const auto &Table>
inline int ladder_rung(int v)
{
    return ladder_walk<Table>(v, [](auto R) { return static_cast<int>(R); });
}

// true when an instantiation of the one-launch hour exists for this problem (the common pack sizes; others take two launches per hour)
inline bool fused_shape_ok(int Z, int Zq, int G, int smap = 0)
{
    return static_cast<int>(grouped_zpg_of(Z)) <= kFusedZpg && pack_need(Zq, G, smap) <= 12;
}

// ------------------------------------------------------------------------------------------------ placing
// Geometry of a placing launch: threads per block, runs per 16 threads (KRUNS = 4 or 8: KRUNS / 2 passes of the 8-lane segments), blocks per destination group
struct PlaceShape {
    int pb, kruns, bpg;
};
inline PlaceShape place_shape(int Z)
{
    const int zpg = static_cast<int>(grouped_zpg_of(Z));
    PlaceShape p;
    p.pb = zpg <= 512 ? 512 : 1024;
    const int seg = p.pb / 16;
    p.bpg = Z < 1024 ? 8 : 16;
    while (p.bpg < 128 && (Z + p.bpg - 1) / p.bpg > 4 * seg) p.bpg *= 2;
    p.kruns = (Z + p.bpg - 1) / p.bpg <= 4 * seg ? 4 : 8;
    return p;
}
inline bool place_shape_fits(int Z)
{
    const PlaceShape p = place_shape(Z);
    return (Z + p.bpg - 1) / p.bpg <= 8 * (p.pb / 16);
}
// p -> f(PB, KRUNS) as compile-time constants, for both placing kernels
template <typename F>
inline auto place_walk(const PlaceShape &p, F &&f)
{
    return ladder_walk<PlaceCells::pb>(p.pb, [&](auto PB) { return ladder_walk<PlaceCells::kruns>(p.kruns, [&](auto KRUNS) { return f(PB, KRUNS); }); });
}

// ------------------------------------------------------------------------------------------------ the launch record
// What the launch helpers of the current run launched (CPM_INFO_CELL_*, include/cpm.h): one word per role, written by the INNERMOST
// helper from its own template parameters -- not from the rule that chose them, so the record is true even where a ladder is wrong.
//   word = kind | CPT << 8 | NQ << 16 | flags << 24   (placing kinds: kind | KRUNS << 8 | (PB / 64) << 16);  0: no such launch
constexpr uint32_t kCellSample = 1, kCellHour = 2, kCellHourPf = 3, kCellDay = 4, kCellHeavy = 5, kCellCount = 6, kCellPlace = 7,
                   kCellBatchSample = 8, kCellBatchPlace = 9, kCellBatchCount = 10;
constexpr uint32_t kCellGrouped = 1, kCellSparse = 2, kCellPerm = 4;
constexpr uint32_t cell_word(uint32_t kind, int cpt, int nq, bool grouped, bool sparse, bool perm = false)
{
    return kind | static_cast<uint32_t>(cpt) << 8 | static_cast<uint32_t>(nq) << 16 |
           ((grouped ? kCellGrouped : 0u) | (sparse ? kCellSparse : 0u) | (perm ? kCellPerm : 0u)) << 24;
}
constexpr uint32_t place_word(uint32_t kind, int pb, int kruns) { return kind | static_cast<uint32_t>(kruns) << 8 | static_cast<uint32_t>(pb / 64) << 16; }

}  // namespace cpm
