// The dense drivers' index arithmetic of csrc/cpm_narrow.h on the host, for tests/test_dense_drivers.py: the PRODUCT'S OWN helpers
// (dense_rank, dense_cap, dense_round_slots, dense_read_pos, dense_live), compiled by g++ from the header the kernels include, run the
// way a sampler wave runs them -- K slots of 64 lanes, a ballot per slot -- and held against a plain loop over (slot, lane).
// dense_rank is the one helper with two bodies: the device's is the v_mbcnt pair, which exists only there; what runs here is its host
// body (a popcount below the lane).  That the two agree is what the GPU tests of tests/test_dense_drivers_gpu.py show.
//   dense_probe fits       the rule that says which twin <CPT, rung> compacts (dense_pays, dense_fits), one line per cell
//   dense_probe            every pattern class (empty, full, single lane, alternating, random) in every slot mix, for K = 1 .. 8 slots;
//                          prints "ok <waves checked>" and returns 0, or the first mismatch and 1
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../carparkingmaps_amd/csrc/cpm_narrow.h"

using namespace cpm;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

// the ballot of one slot, by class
static uint64_t pattern(int cls, int variant)
{
    switch (cls) {
    case 0: return 0ull;                                           // empty
    case 1: return ~0ull;                                          // full
    case 2: return 1ull << (variant & 63);                         // a single lane (0, 63 and in between come from the variants)
    case 3: return (variant & 1) ? 0xAAAAAAAAAAAAAAAAull : 0x5555555555555555ull;  // alternating
    case 4: return rnd();                                          // random, about half
    case 5: return rnd() & rnd() & rnd();                          // random, sparse
    default: return rnd() | rnd() | rnd();                         // random, nearly full
    }
}

static int fail(const char *what, int K, long wave, long a, long b)
{
    std::printf("MISMATCH %s: K %d wave %ld: %ld != %ld\n", what, K, wave, a, b);
    return 1;
}

// one wave of K slots: compact as first_pass does, read back as dense_pass does
static int check(int K, const uint64_t *ballot, long wave)
{
    const uint32_t cap = dense_cap(K);
    // the plain loop: the drivers in (slot, lane) order; a payload names its source
    std::vector<uint32_t> want;
    for (int c = 0; c < K; ++c)
        for (int lane = 0; lane < 64; ++lane)
            if ((ballot[c] >> lane) & 1ull) want.push_back(static_cast<uint32_t>(c * 64 + lane));
    // the wave's way
    std::vector<uint32_t> scratch(cap, 0xFFFFFFFFu);
    uint32_t ndrv = 0;
    for (int c = 0; c < K; ++c) {
        for (int lane = 0; lane < 64; ++lane) {
            const uint32_t rk = dense_rank(ballot[c], lane, ndrv);
            if (rk >= cap) return fail("a lane's rank leaves the scratch", K, wave, rk, cap);  // (a stayer's lane too: its address is formed)
            if ((ballot[c] >> lane) & 1ull) {
                if (scratch[rk] != 0xFFFFFFFFu) return fail("two drivers at one position", K, wave, rk, scratch[rk]);
                scratch[rk] = static_cast<uint32_t>(c * 64 + lane);
            }
        }
        ndrv += static_cast<uint32_t>(__builtin_popcountll(ballot[c]));
    }
    if (ndrv != want.size()) return fail("drivers", K, wave, ndrv, static_cast<long>(want.size()));
    const int kd = static_cast<int>(dense_round_slots(ndrv));
    if (kd > K) return fail("dense slots beyond K", K, wave, kd, K);
    if (static_cast<uint32_t>(kd) * 64u < ndrv || (kd > 0 && static_cast<uint32_t>(kd - 1) * 64u >= ndrv)) return fail("dense slots", K, wave, kd, ndrv);
    size_t i = 0;
    for (int s = 0; s < kd; ++s) {
        for (int lane = 0; lane < 64; ++lane) {
            const uint32_t pos = dense_read_pos(s, lane);
            if (pos >= cap) return fail("a read leaves the scratch", K, wave, pos, cap);
            const bool live = dense_live(s, kd, lane, ndrv);
            if (live != (pos < ndrv)) return fail("live", K, wave, live, pos < ndrv);
            if (!live) continue;
            if (i >= want.size() || scratch[pos] != want[i]) return fail("payload", K, wave, scratch[pos], i < want.size() ? want[i] : -1);
            ++i;
        }
    }
    if (i != want.size()) return fail("drivers read back", K, wave, static_cast<long>(i), static_cast<long>(want.size()));
    return 0;
}

// F <cpt> <rung> <band top Z> <narrow pack bytes at the top> <pays> <fits> <on> <scratch bytes>  per CPT and rung of the hour's ladder
static int fits()
{
    for (int cpt : HourCells::cpt)
        for (int rung : HourCells::nq) {
            const int top = narrow_band_top(rung);
            std::printf("F %d %d %d %d %d %d %d %zu\n", cpt, rung, top, 4 * narrow_row_words(pack_zq(top), pack_guide_bits(top)), dense_pays(cpt) ? 1 : 0,
                        dense_fits(cpt, rung) ? 1 : 0, dense_on(cpt, rung) ? 1 : 0, dense_scratch_bytes(kDenseBlock, cpt, rung));
        }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && argv[1][0] == 'f') return fits();
    long waves = 0;
    static_assert(dense_cap(6) == 384 && dense_round_slots(0) == 0 && dense_round_slots(64) == 1 && dense_round_slots(65) == 2, "capacity rule");
    static_assert(dense_scratch_raw(256, 6) == 12288u && dense_scratch_raw(256, 1) == 2048u, "scratch bytes");
    static_assert(dense_scratch_bytes(256, 6, 5) == (dense_on(6, 5) ? 12288u : 0u) && dense_scratch_bytes(256, 6, 6) == 0u, "scratch only where it is used");
    for (int K = 1; K <= 8; ++K) {
        uint64_t b[8];
        // every slot of one class (K' = 0, K' = K, one driver per slot, ...)
        for (int cls = 0; cls < 7; ++cls) {
            for (int v = 0; v < 64; ++v) {
                for (int c = 0; c < K; ++c) b[c] = pattern(cls, v + 63 * c);
                if (check(K, b, waves++)) return 1;
            }
        }
        // mixed classes per slot
        for (int rep = 0; rep < 4000; ++rep) {
            for (int c = 0; c < K; ++c) b[c] = pattern(static_cast<int>(rnd() % 7), static_cast<int>(rnd() & 0xFF));
            if (check(K, b, waves++)) return 1;
        }
        // exactly 64 m and 64 m + 1 drivers (a dense slot exactly full, and one car more)
        for (int m = 1; m < K; ++m) {
            for (int extra = 0; extra < 2; ++extra) {
                for (int c = 0; c < K; ++c) b[c] = c < m ? ~0ull : 0ull;
                if (extra) b[K - 1] = 1ull << (rnd() & 63);
                if (check(K, b, waves++)) return 1;
            }
        }
    }
    std::printf("ok %ld\n", waves);
    return 0;
}
