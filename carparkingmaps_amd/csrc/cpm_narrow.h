// cpm_narrow.h -- the NARROW row pack of the one-launch hour on dense tables: its geometry, the search on it and the rule that says
// where it is used, free of HIP like cpm_dispatch.h (`g++ -std=c++17` compiles this header alone: tests/narrow_probe.cc runs the
// search below, the product's own source, against the wide search on the host).
//
// The wide pack (cpm_grouped.h, k_build_rows) holds a guide and one 32-bit high word per destination.  The guide entry m = khi >> sh
// brackets a draw to the entries whose top G bits EQUAL m, so the search inside the bracket needs only the bits below them: the narrow
// pack keeps 16 of those per entry,
//     guide (the wide pack's words, verbatim) | one 16-byte header piece, first word hi[Z-1] | Zq entries e[j] = (hi[j] >> (sh - 16)) & 0xFFFF
// (whole 16-byte pieces and the 256-word floor as for the wide pack) -- 10,336 bytes instead of 18,576 at Z = 4,096.  Inside a bracket
// e[j] < k16 implies hi[j] < khi and e[j] > k16 implies hi[j] > khi (k16 = the same bits of the draw); only e[j] == k16 is undecided, a
// 2^-14 event per draw, which reads the wide words of the row from memory (narrow_tie_walk).  (dest, ok) are the wide search's for
// every draw, so the counts do not depend on which pack was streamed.
#pragma once
#include "cpm_dispatch.h"

#if defined(__HIPCC__)
#define CPM_UNROLL _Pragma("unroll")
#else
#define CPM_UNROLL
#endif
// a value the compiler may not trace back to its source (the sampler lives at its scalar-register ceiling: a lane mask computed twice
// is cheaper there than one kept across the search)
#if defined(__HIP_DEVICE_COMPILE__)
#define CPM_OPAQUE(x) asm volatile("" : "+v"(x))
#else
#define CPM_OPAQUE(x) (void)(x)
#endif

namespace cpm {

constexpr int kNarrowHeadWords = 4;  // one 16-byte piece between the guide and the entries: {hi[Z-1], 0, 0, 0}

// sh - 16 >= 0 for every Z whose pack fits (G <= 13)
CPM_HD constexpr int narrow_shift(int G) { return 32 - G - 16; }
CPM_HD constexpr int narrow_row_words(int Zq, int G)  // (Zq is a multiple of 32: whole 16-byte pieces; >= 64 pieces, as pack_dma asks)
{
    const int w = pack_guide_words(G) + kNarrowHeadWords + Zq / 2;
    return w < 256 ? 256 : w;
}
constexpr int narrow_need(int Zq, int G) { return (narrow_row_words(Zq, G) / 4 + kSampleBlock - 1) / kSampleBlock; }
CPM_HD constexpr uint32_t narrow_entry(uint32_t hi, int G) { return (hi >> narrow_shift(G)) & 0xFFFFu; }

// 16-byte piece q of a row's narrow pack from the row's WIDE pack (w.piece(i): its 16-byte piece i, w.word(i): its word i): the guide's
// pieces verbatim, the header, eight entries from two pieces of high words (little endian: entry 2 k in the low half of word k), zeros
// behind the entries of a row at the 256-word floor.  What k_narrow_rows stores, one piece per thread.
struct NarrowPiece {
    uint32_t v[4];
};
template <typename W>
CPM_HD inline NarrowPiece narrow_piece(const W &w, int q, int Z, int Zq, int G)
{
    const int gp = pack_guide_words(G) / 4, s = narrow_shift(G);
    if (q < gp) return w.piece(q);
    if (q == gp) return NarrowPiece{{w.word(4 * gp + Z - 1), 0u, 0u, 0u}};
    const int j = q - gp - 1;
    if (j >= Zq / 8) return NarrowPiece{{0u, 0u, 0u, 0u}};
    const NarrowPiece a = w.piece(gp + 2 * j), b = w.piece(gp + 2 * j + 1);
    auto e2 = [s](uint32_t x, uint32_t y) { return ((x >> s) & 0xFFFFu) | ((y >> s) << 16); };
    return NarrowPiece{{e2(a.v[0], a.v[1]), e2(a.v[2], a.v[3]), e2(b.v[0], b.v[1]), e2(b.v[2], b.v[3])}};
}

// The narrow twin of an instantiation of the hour keeps the wide rule's NQ rung (the launch record stays the wide rule's) and issues
// narrow_nq(rung) LDS-DMA instructions per wave: the largest narrow need of a Z in the rung's band -- the Z whose WIDE need takes that
// rung of HourCells::nq and that the one-launch hour admits (fused_shape_ok: Z <= kGroups * kFusedZpg).  Both needs grow with Z, so it
// is the need of the band's largest Z.
constexpr int kNarrowMaxZ = kGroups * kFusedZpg;
constexpr int narrow_wide_need_of(int Z) { return pack_need(pack_zq(Z), pack_guide_bits(Z)); }
constexpr int narrow_need_of(int Z) { return narrow_need(pack_zq(Z), pack_guide_bits(Z)); }
constexpr int narrow_band_top(int rung)  // the largest Z <= kNarrowMaxZ whose wide need is <= rung (1 when there is none)
{
    int lo = 1, hi = kNarrowMaxZ;  // wide need(lo) <= rung (a pack has a floor of one instruction), hi: the largest candidate
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        if (narrow_wide_need_of(mid) <= rung) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
constexpr int narrow_nq(int rung) { return narrow_need_of(narrow_band_top(rung)); }
static_assert(narrow_nq(5) == 3 && narrow_nq(1) == 1, "Z = 4,096 streams three instructions per wave instead of five");

// Where the narrow pack is streamed: dense packs, the one-launch hour chosen (k_grouped_hour, not its placing-first or day forms) and
// its sampler workgroups in zone order -- and, like fused_pays, where it PAYS unless the caller chose the form himself (CPM_OPT_FUSED
// other than 5: `where_it_pays` false, the narrow pack wherever the one-launch hour runs -- what the tests of small shapes use).
// MEASURED (the parent's library with wide packs / this one, interleaved runs on one box, ms per resample; profiles/narrow_pack_notes.md):
// Z = 4,096 x 1,000: 0.7565 / 0.7259, x 500: 0.6148 / 0.5471; Z = 3,072 x 1,000: 0.6287 / 0.6473; Z = 2,357 x 1,000 dense with the
// one-launch hour forced: 0.6278 / 0.6427.  The narrow search issues ~15 % more vector instructions per car; below 4,096 zones the
// hour has too few bytes per pack and too few rounds of workgroups for the shorter stream to pay for them.  The bound is the smallest
// Z it was measured to pay at; nothing between 3,072 and 4,096 was measured.
#ifndef CPM_NARROW_MIN_Z
#define CPM_NARROW_MIN_Z 4096
#endif
constexpr int kNarrowMinZ = CPM_NARROW_MIN_Z;
inline bool narrow_pays(int Z, bool dense, bool fused_hour, bool zone_order, bool where_it_pays)
{
    return dense && fused_hour && zone_order && Z <= kNarrowMaxZ && (!where_it_pays || Z >= kNarrowMinZ);
}

// ------------------------------------------------------------------------------------------------ the search
// CPT draws against a narrow pack in lockstep, through an accessor A (the sampler's reads LDS, the probe's a host array):
//   a.guide(m)       guide entry m
//   a.cur(j)         a CURSOR on entry j: j * A::kStep + a base of the accessor's (the sampler's is the entry's LDS byte address, so the
//                    walk below adds strides to addresses as the wide one does); cursors are compared and added to, nothing else
//   a.at(cursor)     the 16-bit entry under a cursor
//   a.idx(cursor)    its entry index
//   a.any(p)         true when p holds for any draw that searches together with this one (the sampler: a vote of the wave)
// Out: dest[c] = first j with hi[j] >= khi[c], ok[c] = that is certain, tie[c] = the 16 bits cannot tell (the caller resolves it on the
// wide words with narrow_tie_walk from dest[c]; ok[c] is false then), in[c] = the draw searched.  want[c] == false: no search.
// The same descending-stride walk as pack_search, except that a stride is taken only while it stays INSIDE the bracket (offset + s <=
// n): the entries beyond the bracket belong to other brackets, where these 16 bits mean nothing -- and the answer is at most n, so a
// stride that would pass n is one the wide walk would not take either.  The probes themselves need no clamp on the short path: they
// stay inside the row's pad (at most 15 entries past the bracket's end); the long path clamps them to the row.  An empty bracket ends at
// offset 0 whatever the probes read.
//   offset == n: every entry of the bracket lies below the draw, and hi[lo + n] >= (m + 1) << sh > khi -- certain, unless lo + n is
//                Z - 1, where the guide was clamped: there the full last high word (the header's) decides.
template <int CPT, typename A>
CPM_HD inline void narrow_search(const A &a, const uint32_t (&khi)[CPT], const bool (&want)[CPT], int sh, uint32_t hi_last, int Z, int Zq,
                                 uint32_t (&dest)[CPT], bool (&ok)[CPT], bool (&tie)[CPT], bool (&in)[CPT])
{
    constexpr uint32_t kS = A::kStep;
    uint32_t k16[CPT], lo[CPT], n[CPT], nor = 0;
    CPM_UNROLL
    for (int c = 0; c < CPT; ++c) {
        in[c] = want[c] & (khi[c] <= hi_last);
        const uint32_t kk = in[c] ? khi[c] : 0u;  // (a draw that does not search never moves: nothing is below 0)
        k16[c] = (kk >> (sh - 16)) & 0xFFFFu;
        const uint32_t m = kk >> sh;
        lo[c] = a.guide(m);
        n[c] = a.guide(m + 1);
    }
    CPM_UNROLL
    for (int c = 0; c < CPT; ++c) {
        n[c] = in[c] ? n[c] - lo[c] : 0u;
        nor |= n[c];
    }
    uint32_t p[CPT], end[CPT];  // cursors: the walk's position, the entry behind the bracket (lo + n <= Z - 1)
    CPM_UNROLL
    for (int c = 0; c < CPT; ++c) {
        p[c] = a.cur(lo[c]);
        end[c] = p[c] + n[c] * kS;
    }
#define CPM_NARROW_STEP(S, AT)                                                                          \
    do {                                                                                                \
        uint32_t v_[CPT];                                                                               \
        CPM_UNROLL for (int c = 0; c < CPT; ++c) v_[c] = a.at(AT(p[c] + ((S) - 1u) * kS));              \
        CPM_UNROLL for (int c = 0; c < CPT; ++c) {                                                      \
            const uint32_t t_ = p[c] + (S) * kS;                                                        \
            p[c] = ((v_[c] < k16[c]) & (t_ <= end[c])) ? t_ : p[c];                                     \
        }                                                                                               \
    } while (0)
#define CPM_NARROW_AT_PAD(q) (q)
#define CPM_NARROW_AT_ROW(q) ((q) < top ? (q) : top)
    if (a.any(nor >= 32u)) {  // (rows with long runs of zero-probability zones)
        const uint32_t top = a.cur(static_cast<uint32_t>(Zq - 1));
        int K = 6;
        while (a.any((nor >> K) != 0u)) ++K;
        for (uint32_t s = 1u << (K - 1); s != 0u; s >>= 1) CPM_NARROW_STEP(s, CPM_NARROW_AT_ROW);
    } else {
        const bool a16 = a.any(nor >= 16u);
        const bool a8 = a16 || a.any(nor >= 8u);
        if (a16) CPM_NARROW_STEP(16u, CPM_NARROW_AT_PAD);
        if (a8) CPM_NARROW_STEP(8u, CPM_NARROW_AT_PAD);
        CPM_NARROW_STEP(4u, CPM_NARROW_AT_PAD);
        CPM_NARROW_STEP(2u, CPM_NARROW_AT_PAD);
        CPM_NARROW_STEP(1u, CPM_NARROW_AT_PAD);
    }
#undef CPM_NARROW_AT_ROW
#undef CPM_NARROW_AT_PAD
#undef CPM_NARROW_STEP
    CPM_UNROLL
    for (int c = 0; c < CPT; ++c) {
        const bool full = p[c] == end[c];
        const uint32_t fin = a.at(p[c]);
        dest[c] = a.idx(p[c]);
        uint32_t kq = khi[c];
        CPM_OPAQUE(kq);
        const bool inc = want[c] & (kq <= hi_last);  // (in[c], drawn up again: see CPM_OPAQUE)
        tie[c] = inc & !full & (fin == k16[c]);
        ok[c] = inc & (full ? (dest[c] != static_cast<uint32_t>(Z - 1) || hi_last > khi[c]) : (fin > k16[c]));  // (in: khi <= hi_last)
    }
}

// ------------------------------------------------------------------------------------------------ dense drivers
// About half the cars of a wave drive: the search above and the drivers' slot work would run over all K register slots of the wave with
// the stayers' lanes masked off.  The narrow twin's sampler waves therefore COMPACT their drivers first (cpm_grouped.h, first_pass): a
// driver's payload {local car id, khi} goes to a per-wave LDS scratch behind the pack, at the driver's rank among the wave's drivers
// (slot by slot, lanes in order), and after the pack's barrier the wave reads ceil(drivers / 64) DENSE slots back and searches and
// places from those.  A wave's scratch holds the worst case, CPT x 64 payloads (every car drives).  The index arithmetic, free of HIP
// (tests/dense_probe.cc runs it against a plain loop):
constexpr uint32_t kDensePayloadBytes = 8;  // {id, khi}
CPM_HD constexpr uint32_t dense_cap(int cpt) { return 64u * static_cast<uint32_t>(cpt); }  // payloads of a wave's scratch
// Where compacting pays: a compile-time constant per instantiation (bit CPT of the mask), never a flag the kernel reads.  MEASURED at
// Z = 4,096, the parent's kernel / the compacting one, interleaved runs on one box, ms per resample (profiles/dense_drivers_notes.md):
// six cars per lane (x 1,000) 0.7251 / 0.7063, four (x 500) 0.5540 / 0.5448, two (x 300) 0.5179 / 0.5210 -- a loss, so it is off
// there -- and one (x 150) 0.4931 / 0.4869.
#ifndef CPM_DENSE_CPT_MASK
#define CPM_DENSE_CPT_MASK (~(1u << 2))
#endif
CPM_HD constexpr bool dense_pays(int cpt) { return ((static_cast<uint32_t>(CPM_DENSE_CPT_MASK) >> cpt) & 1u) != 0u; }
// ... and where the scratch leaves the CU as many blocks as it had: the twin <CPT, rung> compacts only if, at the LARGEST narrow pack of
// the rung's band (narrow_band_top), pack + scratch + the static LDS still fit the blocks per CU that the uncompacted twin runs there
// -- the smaller of what its registers allow (the resource remarks: six at six cars per lane, seven below) and what its own LDS
// allows.  Sizes are rounded up to 1,280 bytes, the coarsest allocation step a 160 KiB LDS is assumed to have (the rounding only
// ever switches compaction off).  At six cars per lane that is every rung up to 5 (Z <= 4,096: 26,864 B per block, six blocks in
// 161,184 B); from Z = 4,097 the guide doubles, six blocks no longer fit, and the rungs above run the uncompacted body.
constexpr size_t kCuLdsBytes = 160 * 1024, kLdsStep = 1280;
constexpr size_t kFusedStaticLds = 4240;  // SampleLds / PlaceLds of a block of the one-launch hour (asserted in cpm_grouped.h)
#ifndef CPM_FUSED_LIST_LDS
#define CPM_FUSED_LIST_LDS 10240  // (tuning builds that change the placing list's geometry say its bytes here)
#endif
constexpr size_t kFusedListLds = CPM_FUSED_LIST_LDS;  // the placing blocks' sorted list: the floor of the launch's dynamic LDS (asserted likewise)
constexpr int kDenseBlock = 256;          // threads of a block of the one-launch hour (kFusedThreads)
constexpr int dense_blocks_by_registers(int cpt) { return cpt >= 6 ? 6 : 7; }
constexpr size_t dense_scratch_raw(int block, int cpt) { return static_cast<size_t>(block / 64) * dense_cap(cpt) * kDensePayloadBytes; }
constexpr size_t lds_step_up(size_t b) { return (b + kLdsStep - 1) / kLdsStep * kLdsStep; }
constexpr bool dense_fits(int cpt, int rung)
{
    const int top = narrow_band_top(rung);
    const size_t pack = sizeof(uint32_t) * static_cast<size_t>(narrow_row_words(pack_zq(top), pack_guide_bits(top)));
    const size_t before = (pack > kFusedListLds ? pack : kFusedListLds) + kFusedStaticLds;
    const size_t scr = pack + dense_scratch_raw(kDenseBlock, cpt);
    const size_t after = lds_step_up((scr > kFusedListLds ? scr : kFusedListLds) + kFusedStaticLds);
    const size_t by_lds = kCuLdsBytes / before, by_reg = static_cast<size_t>(dense_blocks_by_registers(cpt));
    return after * (by_lds < by_reg ? by_lds : by_reg) <= kCuLdsBytes;
}
constexpr bool dense_on(int cpt, int rung) { return dense_pays(cpt) && dense_fits(cpt, rung); }
static_assert(dense_fits(6, 5) && !dense_fits(6, 6) && dense_fits(4, 5) && !dense_fits(4, 6), "the headline compacts; six / seven blocks per CU are kept above Z = 4,096");
constexpr size_t dense_scratch_bytes(int block, int cpt, int rung) { return dense_on(cpt, rung) ? dense_scratch_raw(block, cpt) : 0; }
// rank of lane `lane` of a slot whose drivers' ballot is m, with `before` drivers in the wave's earlier slots: before + the drivers in
// the lanes below.  Every lane gets a value <= before + 63 (only a driver's is its rank): an address inside the scratch either way.
CPM_HD inline uint32_t dense_rank(unsigned long long m, int lane, uint32_t before)
{
#if defined(__HIP_DEVICE_COMPILE__)
    (void)lane;
    return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), before));
#else
    return before + static_cast<uint32_t>(__builtin_popcountll(m & ((1ull << lane) - 1ull)));
#endif
}
// the dense slots that `count` payloads fill; dense slot s, lane `lane` reads position s * 64 + lane, which holds a driver below
// `count`.  With kd = dense_round_slots(count) every slot but the last is full.
CPM_HD constexpr uint32_t dense_round_slots(uint32_t count) { return (count + 63u) >> 6; }
CPM_HD constexpr uint32_t dense_read_pos(int s, int lane) { return static_cast<uint32_t>(s) * 64u + static_cast<uint32_t>(lane); }
CPM_HD constexpr bool dense_live(int s, int kd, int lane, uint32_t count) { return s < kd - 1 || dense_read_pos(s, lane) < count; }

// A draw the 16 bits could not decide, on the row's WIDE high words (w(j), j < Zq: the wide pack's entries and its 0xFFFFFFFF pad):
// the first j >= dest with hi[j] >= khi, four independent reads at a time.  Returns j | (hi[j] > khi) << 31.  The draw searched, so
// khi <= hi[Z - 1]: the walk ends inside the row.
constexpr uint32_t kNarrowTieOk = 0x80000000u;
template <typename W>
CPM_HD inline uint32_t narrow_tie_walk(const W &w, uint32_t dest, uint32_t khi, int Z, int Zq)
{
    for (uint32_t j0 = dest; j0 < static_cast<uint32_t>(Zq); j0 += 4u) {
        uint32_t v[4];
        for (uint32_t i = 0; i < 4u; ++i) v[i] = w(j0 + i < static_cast<uint32_t>(Zq) ? j0 + i : static_cast<uint32_t>(Zq) - 1u);
        for (uint32_t i = 0; i < 4u; ++i)
            if (v[i] >= khi) return (j0 + i < static_cast<uint32_t>(Z) ? j0 + i : static_cast<uint32_t>(Z) - 1u) | (v[i] > khi ? kNarrowTieOk : 0u);
    }
    return static_cast<uint32_t>(Z) - 1u;  // (not reached on a well-formed pack; uncertain: the f64 walk decides)
}

}  // namespace cpm
