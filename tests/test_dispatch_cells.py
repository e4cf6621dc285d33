"""Every reachable instantiation of the grouped sampler's dispatch (tests/dispatch_cells.py): the rules and the case table on the CPU
-- the restated rules against the library's own (csrc/cpm_dispatch.h, through tests/dispatch_probe.cc) -- and on the GPU every case
against the oracle, bit for bit, with the launch record (CPM_INFO_CELL_*, written by each family's launch body from its template
parameters) naming exactly the cell the case claims."""
import os
import re
import resource
import shutil
import subprocess

import numpy as np
import pytest

import dispatch_cells as D
from conftest import SIM_SEED, TABLE_SEED
from product_form import at_least, pinned

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ CPU: the rules and the table
def test_band_edges_of_the_sampler_ladder():
    """Z -> NQ from pack_guide_bits, pack_zq and pack_row_words: the edges the dense packs give today"""
    assert D.nq_bands() == {1: (2, 833), 2: (834, 1729), 3: (1730, 2497), 4: (2498, 3521), 5: (3522, 4096), 6: (4097, 5057),
                            8: (5058, 7105), 12: (7106, 10177), 20: (10178, 16384), 40: (16385, 32768)}
    assert D.fused_last_z() == 8192
    assert [D.cpt_wide(m) for m in (170, 171, 340, 341, 700, 701)] == [1, 2, 2, 4, 4, 6]
    assert [D.cpt_narrow(m) for m in (224, 225, 560, 561)] == [1, 2, 2, 4]
    assert D.place_shape(16384)[:2] == (512, 4) and D.place_shape(16385)[:2] == (1024, 4) and D.zpg_of(16385) == 1024
    assert D.idbits(16385) == 22 and D.idbits(8192) == 24
    # the ladders differ: need 13 is NQ 20 for the sampler and NQ 40 for the heavy kernel, need 3 is NQ 5 there
    assert D.ladder_nq(D.SAMPLE, 13) == 20 and D.ladder_nq(D.HEAVY_K, 13) == 40 and D.ladder_nq(D.HEAVY_K, 3) == 5


def test_the_case_table_covers_every_reachable_cell():
    reach, cov = D.reachable(), D.covered()
    assert reach <= D.template_grid()
    assert not (reach - cov), "reachable cells no case runs: " + ", ".join(sorted(D.describe(w) for w in reach - cov))
    assert cov <= reach, "cases that claim cells the rules cannot reach: " + ", ".join(sorted(D.describe(w) for w in cov - reach))
    assert len({c.id for c in D.CASES}) == len(D.CASES)


def test_the_unreachable_instantiations_are_exactly_the_listed_ones():
    un = D.unreachable()
    assert all("no rule found" not in why for why in un.values()), {D.describe(w): why for w, why in un.items()}
    assert sorted(D.describe(w) for w in un) == sorted(
        ["sample<CPT 4, NQ 40>", "sample<CPT 6, NQ 40>", "sample<CPT 4, NQ 40 GROUPED>", "sample<CPT 6, NQ 40 GROUPED>",
         "place<PB 512, KRUNS 8>", "place<PB 1024, KRUNS 8>", "batch_place<PB 512, KRUNS 8>", "batch_place<PB 1024, KRUNS 8>"])
    # by the rules themselves: no Z that fits takes KRUNS = 8, and the largest mean bucket at NQ = 40 is 255
    assert all(D.place_shape(Z).kruns == 4 for Z in range(2, 32769))
    lo, hi = D.nq_bands()[40]
    assert not D.grouped_path_fits(lo * 256, lo) and D.grouped_path_fits(lo * 255, lo) and D.cpt_wide(255) == D.cpt_narrow(255) == 2
    assert not D.pack_row_fits(32769)


def test_every_case_fits_and_sits_on_an_edge():
    bands = D.nq_bands()
    edges = {z for b in bands.values() for z in b}
    for c in D.CASES:
        n = c.Z * c.cpz
        assert D.grouped_path_fits(n, c.Z), c
        assert n >= 32 * c.Z and c.T == (3 if c.Z <= 8192 else 2), c
        if c.table == "synth" and c.kind == "hourly":
            assert c.Z in edges, c
        if c.fused:
            assert D.fused_shape_ok(c.Z, c.table == "sparse"), c
        if c.kind == "heavy":   # the bucket the table is sized for is heavy under both rules, and regions can grow to hold it
            assert _hot_target(c) > max(D.heavy_threshold(D.cpt_wide(c.cpz)), D.heavy_threshold(D.cpt_narrow(c.cpz))), c
            assert D.grouped_path_fits(n, c.Z, D.cap_mult_for(2 * _hot_target(c), n, c.Z)), c


def test_the_header_and_the_package_know_the_record():
    from carparkingmaps_amd import Sampler, _lib
    header = open(os.path.join(ROOT, "include", "cpm.h")).read()
    for name, val in [("CPM_INFO_CELL_APPLIED", 20), ("CPM_INFO_CELL_HEAVY", 21), ("CPM_INFO_CELL_LAST", 22), ("CPM_INFO_CELL_PLACE", 23),
                      ("CPM_INFO_CELL_BATCH", 24), ("CPM_CELL_SAMPLE", D.SAMPLE), ("CPM_CELL_HOUR", D.HOUR), ("CPM_CELL_HOUR_PF", D.HOUR_PF),
                      ("CPM_CELL_DAY", D.DAY), ("CPM_CELL_HEAVY", D.HEAVY_K), ("CPM_CELL_COUNT", D.COUNT), ("CPM_CELL_PLACE", D.PLACE),
                      ("CPM_CELL_BATCH_SAMPLE", D.BATCH_SAMPLE), ("CPM_CELL_BATCH_PLACE", D.BATCH_PLACE), ("CPM_CELL_BATCH_COUNT", D.BATCH_COUNT),
                      ("CPM_CELL_FLAG_GROUPED", D.F_GROUPED), ("CPM_CELL_FLAG_SPARSE", D.F_SPARSE), ("CPM_CELL_FLAG_PERM", D.F_PERM)]:
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", header).group(1)) == val == getattr(_lib, name), name
    assert "cells" in Sampler.last_step.__doc__


def test_the_restatement_agrees_with_the_rules_of_the_library(tmp_path):
    """tests/dispatch_probe.cc prints the rules of csrc/cpm_dispatch.h themselves (a host header: no HIP, no GPU) for every Z in
    2..32768 and every mean in 1..1024; each line must be what dispatch_cells.py says"""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    exe = str(tmp_path / "dispatch_probe")
    subprocess.run([cxx, "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "dispatch_probe.cc")], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    rows = [[int(v) for v in line.split()[1:]] for line in out]
    z_rows, m_rows, l_rows = ([r for line, r in zip(out, rows) if line[0] == k] for k in "ZML")
    assert len(z_rows) + len(m_rows) + len(l_rows) == len(out)
    kinds = (D.SAMPLE, D.HOUR, D.HOUR_PF, D.DAY, D.HEAVY_K)
    assert [r[0] for r in z_rows] == list(range(2, 32769)) and [r[0] for r in m_rows] == list(range(1, 1025))
    for r in z_rows:
        Z, need = r[0], D.need_of(r[0])
        p = D.place_shape(Z)
        assert r[1:] == [int(D.pack_row_fits(Z)), need, *(D.ladder_nq(k, need) for k in kinds), D.zpg_of(Z), D.zpg_of(Z, True), D.idbits(Z),
                         D.idbits(Z, True), p.pb, p.kruns, p.bpg, int(D.fused_shape_ok(Z)), int(D.fused_shape_ok(Z, True))], Z
    for mean, narrow, wide in m_rows:
        assert (narrow, wide) == (D.cpt_narrow(mean), D.cpt_wide(mean)), mean
    assert {r[0]: (r[1], tuple(r[2:])) for r in l_rows} == {k: (D.SPARSE_NQ[k], D.LADDERS[k]) for k in kinds}
    # the bands of the probe's own NQ column: the edges test_band_edges_of_the_sampler_ladder pins
    bands = {}
    for r in z_rows:
        if r[1]:
            lo, hi = bands.get(r[3], (r[0], r[0]))
            bands[r[3]] = (min(lo, r[0]), max(hi, r[0]))
    assert bands == D.nq_bands()


# ------------------------------------------------------------------------------------------------ GPU: the cases
def _zone0(C, cpz):
    return np.arange(C, dtype=np.int64) // cpz + 1


def _hot_target(c):
    """the steady size of the hot zone's bucket: 1.3 x the heavy threshold of the first step's sampler (the wide rule)"""
    return 13 * D.heavy_threshold(D.cpt_wide(c.cpz)) // 10


HOT_DRIVE = 0.9   # p_drive of the hand-made tables: the hot bucket is at 90 % of its steady size after one hour
_tables_key, _tables_val, _refs = None, None, {}


def _tables(O, c):
    """(p_drive, p_dest, cdf) of a case, computed once per (table, Z, T, share) and shared by the cases that follow (the table is
    sorted so that they do); only the latest set is kept"""
    global _tables_key, _tables_val
    Z, T = c.Z, c.T
    share = _hot_target(c) / (Z * c.cpz) if c.kind == "heavy" else 0.0
    key = (c.table, Z, T, share)
    if key == _tables_key:
        return _tables_val
    _tables_key = _tables_val = None
    _refs.clear()
    if c.table == "sparse":
        dm, _ = O.synth_datamatrix(Z, T, TABLE_SEED, density=0.06)      # the generator of tests/test_sparse_upload.py at this T
        p_drive, p_dest = O.synth_p_drive(Z, T, TABLE_SEED), O.createpdestin(dm, Z, T, 2)
        assert int((p_dest != 0).sum(axis=1).max()) <= 192
        if share:   # the same share of every row to zone 8: one more cell per row at most
            p_dest *= 1.0 - share
            p_dest[:, 7, :] += share
    elif c.table == "hot":
        p_drive = np.full((Z, T), HOT_DRIVE, order="F")
        row = np.full(Z, (1.0 - share) / (Z - 1))
        row[7] = share
        p_dest = np.empty((Z, Z, T), order="F")
        p_dest[:, :, :] = row[None, :, None]
    else:
        p_drive, p_dest = O.synth_p_drive(Z, T, TABLE_SEED), O.synth_p_dest_dense(Z, T, TABLE_SEED)
    cdf = O.build_cdf(p_dest)
    if c.table == "synth":
        p_dest = None   # (installed by the library's own generator, bit-identical: test_device_synth_tables_equal_oracle_synth)
    _tables_key, _tables_val = key, (p_drive, p_dest, cdf)
    return _tables_val


def _ref(O, c, p_drive, cdf, seed=SIM_SEED, do_ivp=True, tag=None):
    key = (c.cpz, seed, do_ivp, tag)
    if key not in _refs:
        C = c.Z * c.cpz
        _refs[key] = O.fast_run(p_drive, cdf, C, seed, _zone0(C, c.cpz), do_ivp=do_ivp)
    return _refs[key]


def _install(s, c, p_drive, p_dest):
    s.set_kernel(5)
    if c.table == "synth":
        s.synth_tables(TABLE_SEED)
    else:
        s.set_p_drive(p_drive)
        if c.table == "sparse":
            s.set_sparse_upload(True)
        s.set_p_dest(p_dest)
    assert (s.get_info(6) > 0) == (c.table == "sparse")      # CPM_INFO_SPARSE_TABLES
    s.init_states(c.Z * c.cpz, c.cpz)


def _cells_equal(got, want, what):
    assert got == want, f"{what}: launched " + str({k: D.describe(v) for k, v in got.items()}) + ", the rules say " + str(
        {k: D.describe(v) for k, v in want.items()})


def _same(r, ref):
    return np.array_equal(r["parking"], ref["parking"]) and np.array_equal(r["driving"], ref["driving"])


def _run_hourly(cpm, O, c):
    p_drive, p_dest, cdf = _tables(O, c)
    ref = _ref(O, c, p_drive, cdf)
    with cpm.Sampler(c.Z, c.T) as s:
        _install(s, c, p_drive, p_dest)
        s.set_fused(c.fused)
        for what, opt, want in D.case_steps(c):
            s.set_zone_order(opt["zone_order"])
            if "last_hour" in opt:
                s.set_last_hour(bool(opt["last_hour"]))
            with pinned(s, 5, fused=c.fused, cap_mult=4, parts=1) as rec:
                if what == "ivp":
                    assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"]), (c.id, "per-car state after the IVP")
                else:
                    assert _same(s.resample(SIM_SEED), ref), (c.id, opt)
            _cells_equal(rec["cells"], want, f"{c.id} {what} {opt}")
            if what == "resample":
                assert rec["form"] == D_MODE_FORM[c.fused] and s.get_info(cpm.CPM_INFO_LAST_HOUR) == (1 if (want["last"] & 255) == D.COUNT else 0)


D_MODE_FORM = {0: 0, 1: 1, 3: 3, 6: 6, 8: 6}


def _run_heavy(cpm, O, c):
    p_drive, p_dest, cdf = _tables(O, c)
    ref = _ref(O, c, p_drive, cdf)
    n = c.Z * c.cpz
    # on the oracle's counts, before the GPU runs: the largest bucket is heavy for the first step's sampler (and for the narrow rule's),
    # after the IVP already, and the regions that hold the IVP's largest bucket hold the resample's
    after_ivp = int(np.bincount(ref["zone0"], minlength=c.Z + 1).max())
    largest = int(ref["parking"].max())
    thr = max(D.heavy_threshold(D.cpt_wide(c.cpz)), D.heavy_threshold(D.cpt_narrow(c.cpz)))
    print(f"{c.id}: largest bucket {after_ivp} after the IVP, {largest} in the resample; heavy above {thr}; regions of 4x hold {D.grouped_cap(n, c.Z)}")
    assert after_ivp > thr and largest > thr, (after_ivp, largest, thr)
    cap_mult = D.cap_mult_for(largest, n, c.Z)
    assert cap_mult > 4 and D.cap_mult_for(after_ivp, n, c.Z) == cap_mult
    steps = D.case_steps(c)
    with cpm.Sampler(c.Z, c.T) as s:
        _install(s, c, p_drive, p_dest)
        s.set_fused(0)   # (the heavy launch belongs to the two-launch hour; left to itself the context would start in a one-launch form where that pays)
        # the context meets the heavy bucket: regions grown (attempts repeated), workgroups per heavy zone learned
        with pinned(s, 5, fused=0, repeats=at_least(1), cap_mult=cap_mult):
            assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"]), c.id
        with pinned(s, 5, fused=0, repeats=0, cap_mult=cap_mult, parts=at_least(2)):
            assert _same(s.resample(SIM_SEED), ref), c.id
        # ... and a step behind one that saw it splits it: the sampler under the narrow rule, the heavy launch behind it.  (What a
        # step saw decides the NEXT one: the one hour of an IVP at T = 2 draws for the buckets of the start, all of the mean size,
        # and leaves CPM_INFO_PARTS at 1.)
        for what, _, want in steps:
            if what == "ivp":
                s.init_states(n, c.cpz)
            with pinned(s, 5, fused=0, repeats=0, cap_mult=cap_mult, parts=1 if (what == "ivp" and c.T == 2) else at_least(2)) as rec:
                if what == "ivp":
                    assert np.array_equal(s.solve_ivp(SIM_SEED), ref["zone0"]), (c.id, "per-car state after the IVP")
                else:
                    assert _same(s.resample(SIM_SEED), ref), c.id
            _cells_equal(rec["cells"], want, f"{c.id} {what}")


def _run_batch(cpm, O, c):
    p_drive, p_dest, cdf = _tables(O, c)
    fleets = [p_drive, np.asfortranarray(p_drive * 0.75)]
    seeds = np.array([SIM_SEED, SIM_SEED + 1], dtype=np.uint64)
    refs = [_ref(O, c, fleets[b], cdf, seed=int(seeds[b]), do_ivp=False, tag=b) for b in range(2)]
    with cpm.Sampler(c.Z, c.T) as s:
        _install(s, c, p_drive, p_dest)
        s.set_p_drive_batch(np.asfortranarray(np.stack(fleets, axis=2)))
        for _, opt, want in D.case_steps(c):
            s.set_last_hour(bool(opt["last_hour"]))
            with pinned(s, 5, fused=0, form=cpm.CPM_FORM_BATCH, cap_mult=4, parts=1) as rec:
                rb = s.resample_batch(seeds)
            assert rec["batch_fleets"] == 2, rec
            for b in range(2):
                assert np.array_equal(rb["parking"][:, :, b], refs[b]["parking"]) and np.array_equal(rb["driving"][:, :, b], refs[b]["driving"]), (c.id, b)
            _cells_equal(rec["cells"], want, f"{c.id} batch {opt}")


# sorted so that the cases of one table follow each other: the tables and the oracle's days are computed once and shared
_ORDER = sorted(D.CASES, key=lambda c: (c.table, c.Z, c.T, c.kind == "heavy", c.cpz, c.id))
# the cells no test ran before this module: NQ = 40, PB = 1,024 and zpg = 1,024 (Z = 16,385), the heavy kernel at NQ 5 / 12 / 40
NEVER_RUN = [c for c in _ORDER if c.Z > 16384 or (c.kind == "heavy" and c.table == "hot" and c.Z > 200)]
RUN_BEFORE = [c for c in _ORDER if c not in NEVER_RUN]


def _run(cpm, O, c):
    {"hourly": _run_hourly, "heavy": _run_heavy, "batch": _run_batch}[c.kind](cpm, O, c)
    if c.Z >= 16384:
        print(f"{c.id}: peak host memory so far {resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20:.1f} GiB")


@gpu
@pytest.mark.parametrize("c", RUN_BEFORE, ids=lambda c: c.id)
def test_cell(cpm, O, c):
    _run(cpm, O, c)


@gpu
@pytest.mark.parametrize("c", NEVER_RUN, ids=lambda c: c.id)
def test_cell_never_run_before(cpm, O, c):
    """NQ = 40 (pack_dma clamps the last chunks of 40 x 256 pieces onto pieces - 64; wait_ids counts 40 LDS-DMA instructions), the u16
    guide at G = 13, k_grouped_place<1024, 4> with its 1,024 LDS bins exactly full (zpg = kMaxZonesPerGroup), idbits 22; the heavy
    kernel's NQ 5 / 12 / 40 instantiations"""
    _run(cpm, O, c)


@gpu
def test_the_record_follows_the_commit_rules(cpm, O):
    """Other kernel families leave the record empty; an asynchronous IVP's record is published when the IVP is committed; every step
    writes its own."""
    Z, T, cpz = 64, 3, 64
    n = Z * cpz
    empty = dict(applied=0, heavy=0, last=0, place=0, batch=0)
    with cpm.Sampler(Z, T) as s:
        s.synth_tables(TABLE_SEED)
        s.init_states(n, cpz)
        s.set_fused(0)
        s.set_kernel(1)
        s.resample(SIM_SEED)
        assert s.last_step()["cells"] == empty
        s.set_kernel(5)
        s.solve_ivp_async(SIM_SEED)
        _cells_equal(s.last_step()["cells"], D.predict(Z, n, T, step="ivp"), "asynchronous IVP, read before anything else committed it")
        s.resample(SIM_SEED)
        _cells_equal(s.last_step()["cells"], D.predict(Z, n, T, step="resample"), "resample behind it")
        s.set_kernel(2)
        s.solve_ivp(SIM_SEED)
        assert s.last_step()["cells"] == empty
