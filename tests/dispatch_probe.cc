// The dispatch rules of csrc/cpm_dispatch.h, printed for tests/test_dispatch_cells.py to hold against tests/dispatch_cells.py.
// A host program: it includes that header alone (no HIP) and walks the ladders with the walker the launchers use.
//   Z <Z> <pack_row_fits> <need> <NQ: sample hour hour_pf day heavy> <zpg: dense general> <idbits: dense general> <pb kruns bpg>
//     <fused_shape_ok: dense, sparse>
//   M <mean> <grouped_cpt> <grouped_cpt_wide>
//   L <kind of the record> <sparse NQ> <the rungs of the family's need -> NQ ladder>
#include <cstdio>

#include "../carparkingmaps_amd/csrc/cpm_dispatch.h"

int main()
{
    using namespace cpm;
    const int kSparseCells = 512;  // the longest compact row of a sparse pack (kDsCap, csrc/cpm_dataset.h)
    for (int Z = 2; Z <= 32768; ++Z) {
        const int Zq = pack_zq(Z), G = pack_guide_bits(Z), need = pack_need(Zq, G);
        const int Zc = Z < kSparseCells ? Z : kSparseCells;
        const PlaceShape p = place_shape(Z);
        std::printf("Z %d %d %d %d %d %d %d %d %u %u %u %u %d %d %d %d %d\n", Z, pack_row_fits(Z) ? 1 : 0, need, ladder_rung<SampleCells::nq>(need),
                    ladder_rung<HourCells::nq>(need), ladder_rung<HourPfCells::nq>(need), ladder_rung<DayCells::nq>(need), ladder_rung<HeavyCells::nq>(need),
                    grouped_zpg_of(Z), grouped_zpg_of(Z, true), grouped_idbits(Z), grouped_idbits(Z, true), p.pb, p.kruns, p.bpg,
                    fused_shape_ok(Z, Zq, G) ? 1 : 0, fused_shape_ok(Z, pack_zq(Zc), pack_guide_bits(Zc), 1) ? 1 : 0);
    }
    for (int mean = 1; mean <= 1024; ++mean) std::printf("M %d %d %d\n", mean, grouped_cpt(mean), grouped_cpt_wide(mean));
    auto ladder = [](uint32_t kind, int sparse_nq, const auto &nq) {
        std::printf("L %u %d", kind, sparse_nq);
        for (int rung : nq) std::printf(" %d", rung);
        std::printf("\n");
    };
    ladder(kCellSample, SampleCells::sparse_nq, SampleCells::nq);
    ladder(kCellHour, HourCells::sparse_nq, HourCells::nq);
    ladder(kCellHourPf, HourPfCells::sparse_nq, HourPfCells::nq);
    ladder(kCellDay, DayCells::sparse_nq, DayCells::nq);
    ladder(kCellHeavy, HeavyCells::sparse_nq, HeavyCells::nq);
    return 0;
}
