"""The narrow row pack of the one-launch hour (csrc/cpm_narrow.h) on the CPU: tests/narrow_probe.cc compiles the product's own pack
builder piece, search and tie walk for the host, and this file holds them against the wide search, against numpy's searchsorted and
against a numpy restatement of the layout; then the rung -> LDS-DMA count table and the rule narrow_pays."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZS = (3, 64, 358, 600, 2357, 4096)
HOUR_NQ = (1, 2, 3, 4, 5, 6, 8, 12)   # HourCells::nq, csrc/cpm_dispatch.h
PACK_LDS = 150 * 1024                  # kPackLds
N_RANDOM = 100_000


# ------------------------------------------------------------------------------------------------ the geometry, restated
def guide_bits(Z):
    g = 3
    while (1 << g) < Z:
        g += 1
    return max(g - 2, 3)


def zq_of(Z):
    return (Z + 62) // 32 * 32


def guide_words(G):
    return (1 << G) // 2 + 4


def wide_words(Z):
    return max(256, guide_words(guide_bits(Z)) + zq_of(Z))


def narrow_words(Z):
    return max(256, guide_words(guide_bits(Z)) + 4 + zq_of(Z) // 2)


def need(words):
    return (words // 4 + 255) // 256


def rung_of(n):
    return next((r for r in HOUR_NQ if n <= r), HOUR_NQ[-1])


# ------------------------------------------------------------------------------------------------ rows and draws
def _hi_of(p):
    """high words of a row's running sum as k_build_rows writes them: floor(cdf * 2^32), 0xFFFFFFFF from 1.0 on"""
    cdf = np.cumsum(np.asarray(p, dtype=np.float64))
    return np.where(cdf >= 1.0, 0xFFFFFFFF, np.floor(np.minimum(cdf, 1.0) * 4294967296.0)).clip(0, 0xFFFFFFFF).astype(np.uint64).astype(np.uint32)


def rows_of(Z, rng):
    flat = np.full(Z, 1.0 / Z)
    sparse = np.where(rng.random(Z) < 0.9, 0.0, rng.random(Z))      # 90 % zero-probability destinations: long runs of equal words
    sparse[rng.integers(Z)] += 1e-3
    sparse /= sparse.sum()
    tiny = np.where(np.arange(Z) % 2 == 0, 1e-12, rng.random(Z) + 0.1)  # half of the entries tiny
    tiny /= tiny.sum()
    early = np.zeros(Z)                                              # saturates early: 0xFFFFFFFF pads inside Z
    early[: max(1, Z // 3)] = 1.0 / max(1, Z // 3)
    early[max(1, Z // 3) - 1] += 1e-9
    zero = np.zeros(Z)
    one = np.zeros(Z)
    one[Z // 2] = 0.75                                               # one non-zero cell (an unnormalised total below 1)
    last0 = rng.random(Z)
    last0[-1] = 0.0                                                  # the last cell zero
    last0 *= 0.999 / last0.sum()
    return {"flat": _hi_of(flat), "sparse": _hi_of(sparse), "tiny": _hi_of(tiny), "early": _hi_of(early), "zero": _hi_of(zero),
            "one": _hi_of(one), "last0": _hi_of(last0)}


def wide_pack(hi, Z):
    """guide[m] = min(first j with hi[j] >= m << sh, Z - 1), m = 0 .. 2^G (u16), then Zq high words padded with 0xFFFFFFFF"""
    G = guide_bits(Z)
    sh = 32 - G
    cuts = np.arange((1 << G) + 1, dtype=np.uint64) << np.uint64(sh)
    guide = np.minimum(np.searchsorted(hi.astype(np.uint64), cuts, side="left"), Z - 1).astype(np.uint16)
    g16 = np.zeros(2 * guide_words(G), dtype=np.uint16)
    g16[: guide.size] = guide
    hiq = np.full(zq_of(Z), 0xFFFFFFFF, dtype=np.uint32)
    hiq[:Z] = hi
    pack = np.zeros(wide_words(Z), dtype=np.uint32)
    pack[: guide_words(G)] = g16.view(np.uint32)
    pack[guide_words(G): guide_words(G) + zq_of(Z)] = hiq
    return pack


def narrow_pack_restated(wide, hi, Z):
    G = guide_bits(Z)
    gw = guide_words(G)
    pack = np.zeros(narrow_words(Z), dtype=np.uint32)
    pack[:gw] = wide[:gw]
    pack[gw] = hi[Z - 1]
    e = ((wide[gw: gw + zq_of(Z)] >> np.uint32(32 - G - 16)) & np.uint32(0xFFFF)).astype(np.uint16)
    pack[gw + 4: gw + 4 + zq_of(Z) // 2] = e.view(np.uint32)
    return pack


def draws_of(hi, Z, rng):
    G = guide_bits(Z)
    sh, s16 = 32 - G, 32 - G - 16
    h = hi.astype(np.int64)
    win = (h >> s16) << s16
    m = np.arange((1 << G) + 1, dtype=np.int64) << sh
    parts = [h - 1, h, h + 1, win, win - 1, win + (1 << s16) - 1, win + (1 << s16), m, m - 1,
             np.array([0, h[-1], h[-1] - 1, h[-1] + 1, 0xFFFFFFFF], dtype=np.int64),
             rng.integers(0, 1 << 32, N_RANDOM, dtype=np.int64)]
    return np.clip(np.concatenate(parts), 0, 0xFFFFFFFF).astype(np.uint32)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    exe = str(tmp_path_factory.mktemp("narrow") / "narrow_probe")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "narrow_probe.cc")], check=True)
    return exe


@pytest.fixture(scope="module")
def searched(probe, tmp_path_factory):
    """{Z: {row name: (hi, wide pack, draws, narrow pack, wide answers, narrow answers)}} -- one probe run per Z, shared"""
    d = tmp_path_factory.mktemp("narrow_io")
    out = {}
    for Z in ZS:
        rng = np.random.default_rng(1000 + Z)
        rows = rows_of(Z, rng)
        packs = {k: wide_pack(h, Z) for k, h in rows.items()}
        draws = {k: draws_of(h, Z, rng) for k, h in rows.items()}
        nd = {len(v) for v in draws.values()}
        assert len(nd) == 1
        nd = nd.pop()
        fin, fout = str(d / f"in{Z}.bin"), str(d / f"out{Z}.bin")
        with open(fin, "wb") as f:
            np.array([Z, len(rows), nd], dtype=np.uint32).tofile(f)
            for k in rows:
                packs[k].tofile(f)
                draws[k].tofile(f)
        subprocess.run([probe, "search", fin, fout], check=True)
        got = np.fromfile(fout, dtype=np.uint32)
        rn, per = narrow_words(Z), narrow_words(Z) + 2 * nd
        assert got.size == per * len(rows)
        out[Z] = {k: (rows[k], packs[k], draws[k], got[i * per: i * per + rn], got[i * per + rn: i * per + rn + nd], got[i * per + rn + nd: (i + 1) * per])
                  for i, k in enumerate(rows)}
    return out


@pytest.mark.parametrize("Z", ZS)
def test_narrow_search_equals_wide_search(searched, Z):
    """(dest, ok, searched) of the narrow search -- 16-bit walk, then the wide words behind an undecided draw -- equal the wide
    search's for every draw, and both equal the definition: first j with hi[j] >= khi, certain when hi[j] > khi"""
    ties = far = 0
    for name, (hi, _, draws, _, aw, an) in searched[Z].items():
        core = np.uint32(0xC0000000 | 0x0FFFFFFF)
        bad = np.flatnonzero((aw & core) != (an & core))
        assert bad.size == 0, (Z, name, draws[bad[:5]], aw[bad[:5]], an[bad[:5]])
        inside = draws <= hi[-1]
        ref = np.searchsorted(hi, np.where(inside, draws, 0), side="left")
        # (a draw of 0 on a row whose first words are 0 and a draw that does not search both sit at the guide's first bracket)
        assert np.array_equal(an >> 31, inside.astype(np.uint32)), (Z, name)
        assert np.array_equal((an & 0x0FFFFFFF)[inside], ref[inside].astype(np.uint32)), (Z, name)
        okref = inside & (hi[np.minimum(ref, Z - 1)] > draws)
        assert np.array_equal((an >> 30) & 1, okref.astype(np.uint32)), (Z, name)
        ties += int(((an >> 28) & 1).sum())
        far += int(((an >> 29) & 1).sum())
    assert ties > 0, "no draw took the 16-bit-undecided branch"
    if Z >= 64:
        assert far > 0, "no undecided draw walked past its first four wide words"


@pytest.mark.parametrize("Z", ZS)
def test_narrow_pack_layout(searched, Z):
    """guide verbatim | {hi[Z-1], 0, 0, 0} | Zq u16 entries (hi >> (sh - 16)) & 0xFFFF, the pad 0xFFFF | zeros up to the 256-word floor"""
    for name, (hi, wide, _, narrow, _, _) in searched[Z].items():
        assert np.array_equal(narrow, narrow_pack_restated(wide, hi, Z)), (Z, name)
        e = narrow[guide_words(guide_bits(Z)) + 4:].view(np.uint16)
        assert (e[Z: zq_of(Z)] == 0xFFFF).all()
    assert narrow_words(Z) % 4 == 0 and narrow_words(Z) >= 256 and 32 - guide_bits(Z) - 16 >= 0


def test_rung_to_dma_count_table_and_rule(probe):
    """For every rung of HourCells the narrow twin's LDS-DMA count covers the narrow need of every Z of the rung's band, equals it for
    at least one, and its LDS stays under kPackLds; narrow_pays at its documented edges."""
    out = subprocess.run([probe, "ladder"], check=True, capture_output=True, text=True).stdout.splitlines()
    R = {int(a): (int(b), int(c)) for a, b, c in (l.split()[1:] for l in out if l[0] == "R")}
    Zr = [[int(v) for v in l.split()[1:]] for l in out if l[0] == "Z"]
    P = [[int(v) for v in l.split()[1:]] for l in out if l[0] == "P"]
    assert sorted(R) == sorted(HOUR_NQ) and [r[0] for r in Zr] == list(range(2, 8193))
    seen = {r: [] for r in HOUR_NQ}
    for Z, wneed, rung, nneed, nwords in Zr:
        assert wneed == need(wide_words(Z)) and rung == rung_of(wneed) and nwords == narrow_words(Z) and nneed == need(nwords), Z
        assert nneed <= R[rung][1], (Z, rung)
        assert 4 * nwords <= PACK_LDS and 1024 * 4 * R[rung][1] <= PACK_LDS
        seen[rung].append(nneed)
    for rung in HOUR_NQ:
        assert seen[rung] and max(seen[rung]) == R[rung][1], rung
    assert R[5] == (4096, 3) and R[12][0] == 8192
    # the rule: dense packs, the one-launch hour, zone order, Z <= 8192 -- and Z >= kNarrowMinZ where the library chooses the form
    zs = sorted({p[0] for p in P})
    assert len(zs) == 4 and zs[1] == zs[0] + 1 and zs[2:] == [8192, 8193]
    for Z, dense, fused, order, auto, pays in P:
        assert pays == int(bool(dense and fused and order and Z <= 8192 and (not auto or Z >= zs[1]))), (Z, dense, fused, order, auto)
