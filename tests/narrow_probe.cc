// The narrow row pack of csrc/cpm_narrow.h on the host, for tests/test_narrow_pack.py: the PRODUCT'S OWN builder piece (narrow_piece),
// search (narrow_search) and tie walk (narrow_tie_walk), compiled by g++ from the header the kernels include -- no restatement of them.
//   narrow_probe ladder                 R <rung> <band top Z> <narrow_nq>  per rung of HourCells::nq, then
//                                       Z <Z> <wide need> <wide rung> <narrow need> <narrow row words>  for Z = 2 .. 8192, then
//                                       P <Z> <dense> <fused> <zone order> <where it pays> <narrow_pays>  at the rule's edges
//   narrow_probe search <in> <out>      in : u32 {Z, rows, draws}, then per row {wide pack [pack_row_words], draws [draws]}
//                                       out: per row {narrow pack [narrow_row_words], wide answer [draws], narrow answer [draws]}
//                                            an answer = dest | tie taken << 28 | walked past four words << 29 | ok << 30 | searched << 31
// The wide answer is pack_search's rule restated on the host (guide bracket, then the first entry >= the draw): the test holds both
// against numpy's searchsorted as well.
#include <cstdio>
#include <cstdlib>
#include <string_view>
#include <vector>

#include "../carparkingmaps_amd/csrc/cpm_narrow.h"

using namespace cpm;

struct WideRow {  // narrow_piece's accessor: the wide pack as 16-byte pieces and as words
    const uint32_t *w;
    NarrowPiece piece(int q) const { return NarrowPiece{{w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]}}; }
    uint32_t word(int i) const { return w[i]; }
};
struct HostPack {  // narrow_search's accessor: cursors are entry indices, a "wave" is one draw
    static constexpr uint32_t kStep = 1;
    const uint16_t *g, *e;
    uint32_t guide(uint32_t m) const { return g[m]; }
    uint32_t cur(uint32_t j) const { return j; }
    uint32_t at(uint32_t c) const { return e[c]; }
    uint32_t idx(uint32_t c) const { return c; }
    bool any(bool p) const { return p; }
};

static int ladder()
{
    for (int rung : HourCells::nq) std::printf("R %d %d %d\n", rung, narrow_band_top(rung), narrow_nq(rung));
    for (int Z = 2; Z <= kNarrowMaxZ; ++Z) {
        const int Zq = pack_zq(Z), G = pack_guide_bits(Z), need = pack_need(Zq, G);
        std::printf("Z %d %d %d %d %d\n", Z, need, ladder_rung<HourCells::nq>(need), narrow_need(Zq, G), narrow_row_words(Zq, G));
    }
    for (int Z : {kNarrowMinZ - 1, kNarrowMinZ, kNarrowMaxZ, kNarrowMaxZ + 1})
        for (int f = 0; f < 16; ++f)
            std::printf("P %d %d %d %d %d %d\n", Z, f & 1, (f >> 1) & 1, (f >> 2) & 1, (f >> 3) & 1, narrow_pays(Z, f & 1, (f >> 1) & 1, (f >> 2) & 1, (f >> 3) & 1) ? 1 : 0);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && std::string_view(argv[1]) == "ladder") return ladder();
    if (argc != 4) return 2;
    FILE *in = std::fopen(argv[2], "rb"), *out = std::fopen(argv[3], "wb");
    if (!in || !out) return 2;
    uint32_t head[3];
    if (std::fread(head, 4, 3, in) != 3) return 2;
    const int Z = static_cast<int>(head[0]), rows = static_cast<int>(head[1]);
    const size_t nd = head[2];
    const int Zq = pack_zq(Z), G = pack_guide_bits(Z), sh = 32 - G, gw = pack_guide_words(G), rw = pack_row_words(Zq, G), rn = narrow_row_words(Zq, G);
    std::vector<uint32_t> wide(rw), narrow(rn), draws(nd), aw(nd), an(nd);
    for (int r = 0; r < rows; ++r) {
        if (std::fread(wide.data(), 4, rw, in) != static_cast<size_t>(rw) || std::fread(draws.data(), 4, nd, in) != nd) return 2;
        for (int q = 0; q < rn / 4; ++q) {
            const NarrowPiece p = narrow_piece(WideRow{wide.data()}, q, Z, Zq, G);
            for (int k = 0; k < 4; ++k) narrow[4 * q + k] = p.v[k];
        }
        const uint16_t *guide = reinterpret_cast<const uint16_t *>(wide.data());
        const uint32_t *hi = wide.data() + gw;
        const HostPack np{reinterpret_cast<const uint16_t *>(narrow.data()), reinterpret_cast<const uint16_t *>(narrow.data() + gw + kNarrowHeadWords)};
        const uint32_t hi_last_w = hi[Z - 1], hi_last_n = narrow[gw];
        for (size_t i = 0; i < nd; ++i) {
            const uint32_t k = draws[i];
            {  // wide: bracket from the guide, first entry >= the draw from the bracket's start on (the pad ends the walk)
                const bool inw = k <= hi_last_w;
                const uint32_t kk = inw ? k : 0u;
                uint32_t j = guide[kk >> sh];
                while (hi[j] < kk) ++j;
                aw[i] = j | (inw && hi[j] > kk ? 1u << 30 : 0u) | (inw ? 1u << 31 : 0u);
            }
            const uint32_t khi[1] = {k};
            const bool want[1] = {true};
            uint32_t dest[1];
            bool ok[1], tie[1], inn[1];
            narrow_search<1>(np, khi, want, sh, hi_last_n, Z, Zq, dest, ok, tie, inn);
            uint32_t flags = 0;
            if (tie[0]) {
                const uint32_t r = narrow_tie_walk([hi](uint32_t j) { return hi[j]; }, dest[0], k, Z, Zq);
                flags = 1u << 28 | ((r & ~kNarrowTieOk) >= dest[0] + 4u ? 1u << 29 : 0u);
                dest[0] = r & ~kNarrowTieOk;
                ok[0] = (r & kNarrowTieOk) != 0u;
            }
            an[i] = dest[0] | flags | (ok[0] ? 1u << 30 : 0u) | (inn[0] ? 1u << 31 : 0u);
        }
        std::fwrite(narrow.data(), 4, rn, out);
        std::fwrite(aw.data(), 4, nd, out);
        std::fwrite(an.data(), 4, nd, out);
    }
    std::fclose(out);
    return 0;
}
